"""numpy / Python-integer reference of the WEIGHTED fan-out draw of the neighbour-sampled batches (sgs_nbr_select_weighted,
data.neighbor_collate_torch(weight_q=...), NeighborLoader(weight=...)).  Integer arithmetic throughout, no floating-point log2: the device
result is compared with this one by equality.  Everything that is not the draw itself (frontier, induced / directional collate, seed lists,
stream keys, the case tables) is tests/neighbor_ref.py's, imported here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ref as R  # noqa: E402

WQ_MAX = (1 << 24) - 1
NO_KEY = 0xFFFFFFFF
ONE = 1 << 24                               # 1.0 in the 24-bit fixed point of LOG2Q


# ---------------------------------------------------------------- LOG2Q
def log2_table(bits=200):
    """T[i] = floor(2^24 log2(1 + i / 256)), i = 0 .. 256, by repeated squaring with Python integers.  y is bracketed from below and from
    above at `bits` fractional bits; both ends must give the same bit at every step, which makes each word the exact floor."""
    two = 2 << bits
    out = []
    for i in range(256):
        lo = hi = (256 + i) << (bits - 8)
        t = 0
        for _ in range(24):
            lo, hi = (lo * lo) >> bits, ((hi * hi) >> bits) + 1
            assert (lo >= two) == (hi >= two), "the bracket straddles 2: raise `bits`"
            t <<= 1
            if lo >= two:
                t |= 1
                lo, hi = lo >> 1, (hi >> 1) + 1
        out.append(t)
    return out + [ONE]


TABLE = np.asarray(log2_table(), dtype=np.int64)


def floor_log2(x):
    """floor(log2 x) of int64 x in [1, 2^32), by shifts"""
    x = np.asarray(x, dtype=np.int64)
    n, t = np.zeros_like(x), x.copy()
    for s in (16, 8, 4, 2, 1):
        big = (t >> s) > 0
        n += np.where(big, s, 0)
        t = np.where(big, t >> s, t)
    return n


def log2q(x):
    """LOG2Q(x) for integers 1 <= x < 2^32 -> int64: n = floor(log2 x); m = the 32 bits below the leading one; i = m >> 24;
    r = (m >> 8) & 0xFFFF; (n << 24) + T[i] + (((T[i + 1] - T[i]) r) >> 16)"""
    x = np.asarray(x, dtype=np.int64)
    assert ((x >= 1) & (x < 1 << 32)).all()
    n = floor_log2(x)
    m = (x << (32 - n)) & R.M32.astype(np.int64)
    i, r = m >> 24, (m >> 8) & 0xFFFF
    return (n << 24) + TABLE[i] + (((TABLE[i + 1] - TABLE[i]) * r) >> 16)


def key_of_hash(h, wq):
    """the key of an edge whose id hashes to h under the quantised weight wq (arrays broadcast) -> int64 in [0, 2^30) or NO_KEY"""
    h, wq = np.broadcast_arrays(np.asarray(h, dtype=np.int64), np.asarray(wq, dtype=np.int64))
    assert ((wq >= 0) & (wq <= WQ_MAX)).all()
    nl = (32 << 24) - log2q(np.maximum(h, 1))
    key = log2q(nl) - log2q(np.maximum(wq, 1)) + (24 << 24)
    return np.where(wq >= 1, key, NO_KEY)


def weighted_keys(eid, K, wq):
    return key_of_hash(R.edge_keys(eid, K).astype(np.int64), wq)


# ---------------------------------------------------------------- quantisation
def quantize(w):
    """float weights >= 0 -> int32 in [0, 2^24 - 1]: 0 where w == 0, else clamp(floor(w / max(w) (2^24 - 1) + 0.5), 1, 2^24 - 1), in float64"""
    w = np.asarray(w, dtype=np.float64)
    if not np.isfinite(w).all():
        raise ValueError("non-finite weight")
    if (w < 0).any():
        raise ValueError("negative weight")
    if w.size and not (w > 0).any():
        raise ValueError("all weights are zero")
    if w.size == 0:
        return np.zeros(0, dtype=np.int32)
    q = np.clip(np.floor(w / w.max() * WQ_MAX + 0.5), 1, WQ_MAX)
    return np.where(w == 0, 0, q).astype(np.int32)


# ---------------------------------------------------------------- the selection
def take_row(ids, keys, f):
    """the ids of one row that a fan-out f takes, given their keys: every key below the f-th smallest t, then the first ties with t"""
    if f < 0 or ids.shape[0] <= f:
        return ids
    t = np.sort(keys)[f - 1]
    keep = keys < t
    ties = np.nonzero(keys == t)[0][:f - int(keep.sum())]
    keep[ties] = True
    assert int(keep.sum()) == f
    return ids[keep]


def select(ptr, eid, wq, N, rows, f, K):
    """-> (offs int64 [n_rows + 1], chosen int32); `wq` is aligned with `eid` (in-CSR order)"""
    out, offs = [], [0]
    for v in np.asarray(rows).tolist():
        lo, hi = (int(ptr[v]), int(ptr[v + 1])) if 0 <= v < N else (0, 0)
        ids = eid[lo:hi]
        if f >= 0 and ids.shape[0] > f:
            ids = take_row(ids, weighted_keys(ids, K, wq[lo:hi]), f)
        out.append(ids)
        offs.append(offs[-1] + ids.shape[0])
    return np.asarray(offs, dtype=np.int64), (np.concatenate(out) if out else eid[:0]).astype(np.int32)


# ---------------------------------------------------------------- one batch, one epoch
def in_order(g, wq_sorted):
    """weights by edge id (the sorted list's order) -> in-CSR order"""
    return np.asarray(wq_sorted)[g.in_eid]


def sample(g, seeds, fanouts, keys, wq_in):
    seeds = np.asarray(seeds, dtype=np.int64)
    member = np.zeros(g.N, dtype=bool)
    member[seeds] = True
    front, hop_nodes, chosen = seeds, [int(seeds.shape[0])], []
    for f, K in zip(fanouts, keys):
        _, c = select(g.in_ptr, g.in_eid, wq_in, g.N, front, f, K)
        chosen.append(c)
        front = R.frontier(c, g.ei[0], g.E, g.N, member)
        hop_nodes.append(int(front.shape[0]))
    return member, hop_nodes, chosen


def make_batch(g, data, seeds, fanouts, keys, subgraph_type, wq_in):
    """neighbor_ref.make_batch with the weighted draw; `wq_in` in in-CSR order"""
    member, hop_nodes, chosen = sample(g, seeds, fanouts, keys, wq_in)
    node_ids = np.nonzero(member)[0].astype(np.int64)
    if subgraph_type == "induced":
        ei, eid = R.induced(g.out_ptr, g.out_dst, g.out_eid, g.N, g.E, member)
    else:
        ei, eid = R.directional(np.concatenate(chosen), g.ei, g.E, g.N, member)
    seed_mask = np.zeros(g.N, dtype=bool)
    seed_mask[np.asarray(seeds, dtype=np.int64)] = True
    seed_mask = seed_mask[node_ids]
    m = data["masks"][:, node_ids] & seed_mask[None, :]
    return dict(x=data["x"][node_ids], y=data["y"][node_ids], edge_index=ei, prob=data["prob"][eid], eid=eid, node_ids=node_ids,
                seed_mask=seed_mask, n_seeds=int(len(seeds)), hop_nodes=hop_nodes, train_mask=m[0], val_mask=m[1], test_mask=m[2])


def epoch_batches(g, data, input_ids, fanouts, batch_size, shuffle, seed, epoch, subgraph_type, wq_in, drop_last=False):
    return [make_batch(g, data, s, fanouts, [R.stream_key(seed, epoch, b, h) for h in range(len(fanouts))], subgraph_type, wq_in)
            for b, s in enumerate(R.epoch_seeds(input_ids, batch_size, shuffle, seed, epoch, drop_last))]


# ---------------------------------------------------------------- weight patterns of the kernel tests
WEIGHT_PATTERNS = ("random", "equal", "mostly_zero", "zero_rows", "two_values")


def weight_pattern(name, g, seed, zero_rows=()):
    """int32 [E] in in-CSR order.  random: uniform in [1, 2^24); equal: one value; mostly_zero: 70 % zeros; zero_rows: the in-rows of
    `zero_rows` and every fifth node entirely zero; two_values: only 1 and 2^24 - 1"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 1 << 24, g.E).astype(np.int32)
    if name == "equal":
        w[:] = 12345
    elif name == "mostly_zero":
        w[rng.random(g.E) < 0.7] = 0
    elif name == "zero_rows":
        for v in list(zero_rows) + list(range(0, g.N, 5)):
            w[g.in_ptr[v]:g.in_ptr[v + 1]] = 0
    elif name == "two_values":
        w = np.where(rng.random(g.E) < 0.5, 1, WQ_MAX).astype(np.int32)
    elif name != "random":
        raise ValueError(name)
    return w
