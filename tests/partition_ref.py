"""numpy reference of the device partitioner (sgs_gnn_amd/partition.py, csrc/partition.hip): balanced k-way partition by capacity-constrained
region growing and synchronous label-propagation refinement.  Every step is integer arithmetic, so the device result is compared with this
one by equality.  The kernel contracts (`propose`, `commit`, `stats`) and the phases (`partition`) are restated here independently of the
product; the small graph builders at the end are shared by the CPU and the GPU tests."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
GMAX = (1 << 20) - 1            # the gain field of a commit key
MAX_PARTS = 4096
ELIG_UNASSIGNED, ELIG_HASH = 0, 1


def fmix32(h):
    """murmur3's 32-bit finaliser, elementwise, as uint64 values below 2^32"""
    h = np.asarray(h, dtype=np.uint64) & M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def H(v, k):
    return fmix32((np.asarray(v, dtype=np.uint64) & M32) ^ fmix32(np.uint64(int(k) & 0xFFFFFFFF)))


def bounds(N, P, eps):
    """-> (cap, lo, base)"""
    return int(math.ceil((1.0 + eps) * N / P)), int(math.floor((1.0 - eps) * N / P)), -(-N // P)


def csr(edge_index, N):
    """rows by source, the entries of a row in the order of the edge list"""
    src, dst = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    order = np.argsort(src, kind="stable")
    ptr = np.zeros(N + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(src, minlength=N))
    return ptr.astype(np.int32), dst[order].astype(np.int32)


def _rows(ptr):
    return np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr.astype(np.int64)))


def eligible(part, mode, k):
    if mode == ELIG_UNASSIGNED:
        return part < 0
    return (H(np.arange(part.shape[0]), k) & np.uint64(1)).astype(bool)


def propose(ptr, col, part, P, elig, mingain):
    """-> (best, gain) int32 [N]: best = -1 and gain = 0 where the node proposes nothing"""
    N = len(ptr) - 1
    part = part.astype(np.int64)
    row, c = _rows(ptr), col.astype(np.int64)
    pc = part[c]
    m = elig[row] & (c != row) & (pc >= 0)
    uk, cnt = np.unique(row[m] * P + pc[m], return_counts=True)
    ur, up = uk // P, uk % P
    own = np.zeros(N, dtype=np.int64)
    mine = up == part[ur]
    own[ur[mine]] = cnt[mine]
    ur, up, cnt = ur[~mine], up[~mine], cnt[~mine]
    order = np.lexsort((up, -cnt, ur))                                  # per row: count descending, then part ascending
    ur, up, cnt = ur[order], up[order], cnt[order]
    first = np.ones(ur.shape[0], dtype=bool)
    first[1:] = ur[1:] != ur[:-1]
    rows, b, g = ur[first], up[first], cnt[first] - own[ur[first]]
    ok = g >= mingain
    best, gain = np.full(N, -1, dtype=np.int32), np.zeros(N, dtype=np.int32)
    best[rows[ok]], gain[rows[ok]] = b[ok], g[ok]
    return best, gain


def _first_per_segment(seg, limit):
    """seg ascending; True for the first limit[seg] entries of every run of equal values"""
    pos = np.arange(seg.shape[0], dtype=np.int64)
    head = np.ones(seg.shape[0], dtype=bool)
    head[1:] = seg[1:] != seg[:-1]
    start = np.maximum.accumulate(np.where(head, pos, 0))
    return (pos - start) < limit[seg]


def commit(best, gain, part, size, cap, lo_s):
    """applies one sweep's proposals to `part` / `size` in place -> the number of nodes moved"""
    P = size.shape[0]
    size0, part0 = size.astype(np.int64).copy(), part.astype(np.int64).copy()
    v = np.nonzero(best >= 0)[0].astype(np.int64)
    if v.size == 0:
        return 0
    low = ((GMAX - np.clip(gain[v].astype(np.int64), 0, GMAX)).astype(np.uint64) << np.uint64(31)) | v.astype(np.uint64)
    key = (best[v].astype(np.uint64) << np.uint64(51)) | low
    order = np.argsort(key, kind="stable")
    keep = _first_per_segment(best[v][order].astype(np.int64), np.maximum(cap - size0, 0))
    v, low = v[order][keep], low[order][keep]
    src = part0[v]
    free_pass = v[src < 0]
    v, low, src = v[src >= 0], low[src >= 0], src[src >= 0]
    order = np.argsort((src.astype(np.uint64) << np.uint64(51)) | low, kind="stable")
    keep = _first_per_segment(src[order], np.maximum(size0 - lo_s, 0))
    v = v[order][keep]
    assert (size0[part0[v]] > lo_s).all()                               # no node leaves a part that holds <= lo nodes
    movers = np.concatenate([free_pass, v])
    np.subtract.at(size, part0[v], 1)
    np.add.at(size, best[movers], 1)
    part[movers] = best[movers]
    assert (size <= max(cap, int(size0.max()))).all() and (size[best[movers]] <= cap).all() and int(size.min()) >= 0
    assert np.array_equal(np.bincount(part[part >= 0], minlength=P), size)
    return int(movers.size)


def stats(ptr, col, part, P):
    """-> (size int64 [P], the number of stored non-loop entries whose two ends lie in different parts)"""
    row, c = _rows(ptr), col.astype(np.int64)
    p = part.astype(np.int64)
    return np.bincount(p[p >= 0], minlength=P), int(((c != row) & (p[row] != p[c])).sum())


def seed_nodes(ptr, col, P, seed):
    N = len(ptr) - 1
    row = _rows(ptr)
    deg = np.bincount(row[col.astype(np.int64) != row], minlength=N)
    v = np.arange(N)
    return np.lexsort((v, H(v, seed), deg == 0))[:P]


def check_init(init, P, cap):
    init = np.asarray(init)
    if init.min() < 0 or init.max() >= P:
        raise ValueError("init: a value outside [0, P)")
    if np.bincount(init, minlength=P).max() > cap:
        raise ValueError("init: a part above cap")


def partition(ptr, col, P, eps=0.05, hot=40, cold=20, seed=0, init=None, trace=None):
    """-> (part int32 [N], report).  `trace(name, part)` is called after grow, after fill and after every refinement sweep."""
    N = len(ptr) - 1
    assert 1 <= P <= min(N, MAX_PARTS)
    cap, lo, base = bounds(N, P, eps)
    rep = dict(cap=cap, grow_sweeps=0, filled=0, moved=[])
    note = trace or (lambda name, part: None)
    if init is None:
        part = np.full(N, -1, dtype=np.int32)
        part[seed_nodes(ptr, col, P, seed)] = np.arange(P, dtype=np.int32)
        size = np.ones(P, dtype=np.int32)
        while True:
            best, gain = propose(ptr, col, part, P, eligible(part, ELIG_UNASSIGNED, 0), 1)
            rep["grow_sweeps"] += 1
            if commit(best, gain, part, size, cap, 0) == 0:
                break
            assert size.max() <= cap
        note("grow", part)
        left = np.nonzero(part < 0)[0]                                  # ascending id
        slots = np.repeat(np.arange(P, dtype=np.int32), np.maximum(base - size, 0))
        assert slots.size >= left.size
        part[left] = slots[:left.size]
        size = np.bincount(part, minlength=P).astype(np.int32)
        rep["filled"] = int(left.size)
        note("fill", part)
    else:
        check_init(init, P, cap)
        part = np.asarray(init).astype(np.int32).copy()
        size = np.bincount(part, minlength=P).astype(np.int32)
    assert (part >= 0).all() and size.max() <= cap
    rep["cut_edges_initial"] = stats(ptr, col, part, P)[1]
    for s in range(hot + cold):
        best, gain = propose(ptr, col, part, P, eligible(part, ELIG_HASH, seed + 1 + s), 0 if s < hot else 1)
        rep["moved"].append(commit(best, gain, part, size, cap, lo))
        assert size.max() <= cap and (part >= 0).all()
        note("refine", part)
    sizes, cut = stats(ptr, col, part, P)
    rep.update(sizes=sizes, cut_edges=cut, imbalance=float(sizes.max()) * P / N)
    return part, rep


# ---------------------------------------------------------------- graphs of the tests
def both_ways(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])])


def grid_graph(n, seed):
    """n x n 4-neighbour grid with shuffled node ids -> (edge_index [2, E] stored both ways, N)"""
    idx = np.arange(n * n).reshape(n, n)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    sigma = np.random.default_rng(seed).permutation(n * n)
    return both_ways(sigma[a], sigma[b]), n * n


def planted_graph(N, communities, intra, inter, seed):
    """per node `intra` partners drawn inside its community and `inter` drawn anywhere; multi-edges and self loops stay as drawn.
    -> (edge_index stored both ways, N, the planted part vector)"""
    rng = np.random.default_rng(seed)
    n = N // communities
    planted = rng.permutation(N) // n
    members = np.argsort(planted, kind="stable").reshape(communities, n)
    v = np.arange(N)
    a = np.concatenate([np.repeat(v, intra), np.repeat(v, inter)])
    b = np.concatenate([members[np.repeat(planted, intra), rng.integers(0, n, N * intra)], rng.integers(0, N, N * inter)])
    return both_ways(a, b), N, planted.astype(np.int32)


def hash_partition(N, P, seed):
    """a balanced partition with no regard to the edges: the p-th N / P nodes in hash order"""
    part = np.empty(N, dtype=np.int32)
    part[np.lexsort((np.arange(N), H(np.arange(N), seed)))] = (np.arange(N) * P // N).astype(np.int32)
    return part


# ---------------------------------------------------------------- hand-made cases, one per rule (CPU: the reference against the expected
# values written here; GPU: the kernels against the reference on the same inputs)
def _csr_of_rows(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, (np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if ptr[-1] else np.zeros(0, dtype=np.int32))


def propose_cases():
    """(name, ptr, col, part, P, mingain, node, (best, gain) expected of `node` when it is eligible)"""
    i32 = lambda *a: np.asarray(a, dtype=np.int32)  # noqa: E731
    out = []
    ptr, col = _csr_of_rows([[1, 2], [0], [0]])
    out.append(("tie goes to the lower part", ptr, col, i32(0, 2, 1), 3, 0, 0, (1, 1)))
    ptr, col = _csr_of_rows([[1, 2, 3, 4], [0], [0], [0], [0]])
    out.append(("own part is never best", ptr, col, i32(0, 0, 0, 0, 1), 2, -2, 0, (1, -2)))
    out.append(("a loss is not proposed", ptr, col, i32(0, 0, 0, 0, 1), 2, 0, 0, (-1, 0)))
    ptr, col = _csr_of_rows([[0, 0, 0, 1], [0, 1]])
    out.append(("self loops are ignored", ptr, col, i32(0, 1), 2, 1, 0, (1, 1)))
    ptr, col = _csr_of_rows([[1, 2, 2], [0], [0, 0]])
    out.append(("multi-edges count", ptr, col, i32(0, 1, 2), 3, 0, 0, (2, 2)))
    ptr, col = _csr_of_rows([[1, 2, 3], [0, 2], [0, 1], [0]])
    out.append(("unassigned neighbours are ignored", ptr, col, i32(-1, -1, -1, 1), 2, 1, 0, (1, 1)))
    out.append(("only unassigned neighbours: no proposal", ptr, col, i32(-1, -1, -1, 1), 2, 1, 1, (-1, 0)))
    return out


def commit_cases():
    """(name, best, gain, part, size, cap, lo, part expected afterwards)"""
    i32 = lambda *a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return [
        ("free = 0", i32(-1, -1, 1, 1), i32(0, 0, 3, 2), i32(1, 1, -1, -1), i32(0, 2), 2, 0, i32(1, 1, -1, -1)),
        ("free = 1, equal gains: the lower node", i32(-1, 1, 1, 1), i32(0, 2, 2, 2), i32(1, -1, -1, -1), i32(0, 1), 2, 0, i32(1, 1, -1, -1)),
        ("free = 1: the higher gain first", i32(-1, 1, 1, 1), i32(0, 2, 3, 2), i32(1, -1, -1, -1), i32(0, 1), 2, 0, i32(1, -1, 1, -1)),
        ("a source at lo keeps its nodes", i32(1, 1, -1, -1), i32(1, 1, 0, 0), i32(0, 0, 1, 1), i32(2, 2), 4, 2, i32(0, 0, 1, 1)),
        ("a source one above lo gives one node", i32(1, 1, -1, -1, -1), i32(1, 2, 0, 0, 0), i32(0, 0, 0, 1, 1), i32(3, 2), 4, 2, i32(0, 1, 0, 1, 1)),
        ("a negative gain ranks as zero", i32(-1, 1, 1), i32(0, -3, 0), i32(1, -1, -1), i32(0, 1), 2, 0, i32(1, 1, -1)),
    ]


def clamp_case():
    """Four nodes, P = 2, one place left in part 1.  Node 2 gains exactly 2^20 - 1 by moving there, node 3 gains 2^20 + 5: without the
    clamp node 3 would go first, with it they tie and the lower id wins.  -> (ptr, col, part, size, cap, part expected)"""
    ptr, col = _csr_of_rows([[], [], np.zeros(GMAX, dtype=np.int32), np.zeros(GMAX + 6, dtype=np.int32)])
    return ptr, col, np.asarray([1, 0, -1, -1], dtype=np.int32), np.asarray([1, 1], dtype=np.int32), 2, np.asarray([1, 0, 1, -1], dtype=np.int32)


def key_for(nodes, N):
    """a hash key under which every node of `nodes` is eligible"""
    for k in range(1, 4096):
        if (H(np.asarray(nodes), k) & np.uint64(1)).all():
            return k
    raise AssertionError("no key")


ROW_LENGTHS = (0, 1, 63, 64, 65, 1025)
HELD_LENGTHS = (256, 257, 512, 513)     # either side of what a lane of the one-wave form may keep in registers (4 or 8 entries per lane)
PARTS = (1, 2, 64, 65, 4096)


def kernel_case(P, hub_row, seed):
    """A CSR for the kernels alone (it need not be symmetric): N = max(P, 256) + 3 nodes, no multiple of the four waves of a workgroup;
    rows 0-5 of ROW_LENGTHS entries, row 6 a hub of hub_row + 301, row 7 with every neighbour in one part, rows 8-11 of HELD_LENGTHS, the rest
    0-20 entries; columns
    uniform (self loops and repeats as they fall); parts uniform with an eighth of the nodes unassigned.  -> (ptr, col, part)"""
    rng = np.random.default_rng(seed)
    N = max(P, 256) + 3
    part = rng.integers(0, P, N).astype(np.int32)
    part[rng.random(N) < 0.125] = -1
    part[:8] = np.asarray([-1, 0, P - 1, -1, P // 2, 0, -1, P - 1])[:8]
    lens = list(ROW_LENGTHS) + [hub_row + 301, 40] + list(HELD_LENGTHS) + list(rng.integers(0, 21, N - 12))
    rows = [rng.integers(0, N, n) for n in lens]
    same = np.nonzero(part == part[N - 1])[0] if part[N - 1] >= 0 else np.nonzero(part == 0)[0]
    rows[7] = same[rng.integers(0, same.size, 40)]
    ptr, col = _csr_of_rows(rows)
    return ptr, col, part
