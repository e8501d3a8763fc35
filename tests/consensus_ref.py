"""numpy restatements of the three kernels of the sparsifier export (sgs_consensus_accum, sgs_consensus_select, sgs_edge_class_counts),
integer-only where the kernels are, with the case tables the CPU and GPU tests share.  Every function takes `fault=`: None is the
contract; a name plants one deliberate mistake (FAULTS), which the case tables must expose (test_consensus_cpu.py)."""
import numpy as np

FAULTS = ("tie_high", "shift5", "byte_as_count", "count_skipped")
COUNT_MAX = 127

# ------------------------------------------------------------------ case tables
ACCUM_E = (0, 1, 15, 16, 17, 4097, 70003)
ACCUM_DC = (1, 11, 127)
ACCUM_PAD = (0, 3)                                   # mask stride E and E + 3 (unaligned rows)
SELECT_E = (0, 1, 15, 16, 17, 4097, 70003)
SELECT_LARGE_E = 2 * 1024 * 1024 + 1                 # one edge above the fused small-E path's limit (1024 chunks of 2048)
PAIR_PRIVATE_C = (2, 5, 41, 128)
PAIR_DIRECT_C = (5, 129)
PAIR_N_EDGES = (0, 1, 70003)


def select_qs(E):
    return sorted({0, 1, E // 5, E - 1, E} & set(range(0, E + 1)))


# ------------------------------------------------------------------ inputs
def make_masks(E, Dc, pad, seed):
    """A [Dc, E] view with row stride E + pad into a byte buffer whose padding holds 0xFF; mask bytes from {0, 0, 1, 2, 255}."""
    g = np.random.default_rng(seed)
    buf = np.full(Dc * (E + pad) + 1, 0xFF, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf, shape=(Dc, E), strides=(E + pad, 1))
    rows[...] = g.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), size=(Dc, E))
    return buf, rows


def make_counts_scores(E, D, seed, with_p=True):
    """Counts in 0..D with heavy ties; scores from four distinct values, pairs that differ only below bit 6, one NaN, one negative, one -0."""
    g = np.random.default_rng(seed)
    count = g.choice(np.array([0, D // 2, D // 2, D, max(D - 1, 0)], dtype=np.int32), size=E).astype(np.int32)
    if not with_p:
        return count, None
    base = np.array([0.125, 0.3, 0.30000007, 0.9], dtype=np.float32)
    p = g.choice(base, size=E).astype(np.float32)
    bits = p.view(np.uint32).copy()
    low = g.integers(0, 64, size=E, dtype=np.uint32)
    twin = g.random(E) < 0.5
    bits[twin] = (bits[twin] & ~np.uint32(63)) | low[twin]          # differ only in the 6 lowest mantissa bits: the keys tie
    p = bits.view(np.float32).copy()
    if E >= 16:
        p[3], p[7], p[11] = np.nan, -0.5, -0.0
        count[3] = count[7] = count[11] = D // 2
    return count, p


def make_pairs_case(n, N, C, seed, with_mask):
    g = np.random.default_rng(seed)
    ei = g.integers(0, N, size=(2, n), dtype=np.int64)
    y = g.integers(0, C, size=N, dtype=np.int64)
    y[np.arange(N) % 3 == 0] = 0                                    # a hot diagonal cell
    if N >= 8:
        y[1], y[2] = -100, C                                        # labels outside [0, C): edges at these nodes are skipped
    if n >= 8:
        ei[0, 5], ei[1, 6] = N, N                                   # an endpoint outside [0, N)
        ei[0, 2], ei[1, 3] = 1, 2
    mask = None
    if with_mask:
        mask = g.choice(np.array([0, 1, 255], dtype=np.uint8), size=n)
    return ei, y, mask


# ------------------------------------------------------------------ the three restatements
def accum_ref(rows, count=None, first=True, hist=None, fault=None):
    """count[e] = (0 if first else count[e]) + #{d : rows[d, e] != 0};  hist[count[e]] += 1 afterwards (hist accumulated, never cleared)."""
    Dc, E = rows.shape
    add = rows.astype(np.int64).sum(0) if fault == "byte_as_count" else (rows != 0).sum(0, dtype=np.int64)
    out = (np.zeros(E, dtype=np.int64) if first else count.astype(np.int64)) + add
    out = out.astype(np.int32)
    if hist is not None:
        hist = hist + np.bincount(np.clip(out, 0, COUNT_MAX), minlength=128).astype(np.int64)
    return out, hist


def keys_ref(count, p, fault=None):
    """uint32 key_e = (clamp(count_e) << 25) | (bits(p_e) >> 6); low part 0 when p is None or !(p_e >= 0)."""
    c = np.clip(count.astype(np.int64), 0, COUNT_MAX).astype(np.uint32)
    key = c << np.uint32(25)
    if p is not None:
        bits = p.view(np.uint32)
        with np.errstate(invalid="ignore"):
            ok = (p >= 0) & ((bits >> np.uint32(31)) == 0)
        sh = np.uint32(5 if fault == "shift5" else 6)
        key = key | np.where(ok, bits >> sh, np.uint32(0)).astype(np.uint32)
    return key.astype(np.uint32)


def select_ref(count, p, q, edge_index=None, fault=None):
    """The q largest keys, ties to the lowest edge id, in original edge order."""
    E = count.shape[0]
    keys = keys_ref(count, p, fault)
    ids = np.arange(E, dtype=np.int64)
    tie = -ids if fault == "tie_high" else ids
    order = np.lexsort((tie, -keys.astype(np.int64)))
    eid = np.sort(order[:q]).astype(np.int64)
    mask = np.zeros(E, dtype=np.uint8)
    mask[eid] = 1
    return {"keys": keys, "mask": mask, "eid": eid, "edge_index": edge_index[:, eid] if edge_index is not None else None,
            "count": np.clip(count[eid], 0, COUNT_MAX).astype(np.int32),
            "p": p[eid] if p is not None else np.ones(q, dtype=np.float32)}


def edge_class_ref(edge_index, y, N, C, mask=None, fault=None):
    """int64 [C, C]: pairs[y[src]][y[dst]] over the edges with mask unset or != 0; endpoints outside [0, N) and labels outside [0, C) skipped."""
    n = edge_index.shape[1]
    s, d = edge_index[0], edge_index[1]
    take = np.ones(n, dtype=bool) if mask is None else mask != 0
    take &= (s >= 0) & (s < N) & (d >= 0) & (d < N)
    s, d = s[take], d[take]
    a, b = y[s], y[d]
    if fault == "count_skipped":
        a, b = np.clip(a, 0, C - 1), np.clip(b, 0, C - 1)
    ok = (a >= 0) & (a < C) & (b >= 0) & (b < C)
    return np.bincount(a[ok] * C + b[ok], minlength=C * C).reshape(C, C).astype(np.int64)
