"""Host reference of the ROC-AUC counts (include/sgs_hip.h, sgs_auc_pack / sgs_auc_counts), integers throughout.

two_u(scores, pos, mask) -> (twoU, P, Nn) of one column: the items are the entries with mask set and a non-NaN score, and
twoU = sum over positive i, negative j of (2 [x_j < x_i] + [x_j == x_i]) by two binary searches per positive item in the sorted
negatives.  brute(...) is the same figure by the O(n^2) pair count with Python float comparisons; tests/test_auc_cpu.py pins one to the
other.  pack_keys restates the key packing bit for bit; counts() gives the [3, S, 3] table of a pooled score matrix."""
import numpy as np


def order_image(x):
    """uint32 image of fp32 values whose unsigned order is the float order: -0.0 becomes +0.0, then a negative value has all its bits
    flipped and a non-negative one its sign bit."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def pack_keys(scores, y, masks, C):
    """uint64 [N * S]: the keys sgs_auc_pack writes for scores [N, S], labels y [N] and three masks."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    N, S = scores.shape
    y = np.asarray(y, dtype=np.int64)
    m = sum((np.asarray(masks[s]) != 0).astype(np.uint64) << np.uint64(s) for s in range(3))
    m = np.where((y >= 0) & (y < C), m, np.uint64(0))
    mm = np.repeat(m[:, None], S, axis=1)
    mm = np.where(np.isnan(scores), np.uint64(0), mm)
    col = np.broadcast_to(np.arange(S, dtype=np.int64)[None, :], (N, S))
    target = np.ones((N, S), dtype=np.int64) if S == 1 else col
    pos = (y[:, None] == target).astype(np.uint64) << np.uint64(3)
    key = (col.astype(np.uint64) << np.uint64(36)) | (order_image(scores.reshape(-1)).reshape(N, S).astype(np.uint64) << np.uint64(4)) | pos | mm
    return key.reshape(-1).astype(np.uint64)


def _items(scores, pos, mask):
    scores = np.asarray(scores, dtype=np.float32)
    keep = (np.asarray(mask) != 0) & ~np.isnan(scores)
    return scores[keep], np.asarray(pos, dtype=bool)[keep]


def two_u(scores, pos, mask):
    """(twoU, P, Nn) as Python ints."""
    x, p = _items(scores, pos, mask)
    img = order_image(x).astype(np.int64)
    neg = np.sort(img[~p])
    xp = img[p]
    lt = np.searchsorted(neg, xp, side="left").astype(np.int64)
    le = np.searchsorted(neg, xp, side="right").astype(np.int64)
    return int(lt.sum() + le.sum()), int(p.sum()), int((~p).sum())


def brute(scores, pos, mask):
    """The same by counting pairs, with the float comparisons themselves (-0.0 == 0.0, -inf < everything finite < +inf)."""
    x, p = _items(scores, pos, mask)
    xs, ps = [float(v) for v in x], [bool(v) for v in p]
    tot = 0
    for i, xi in enumerate(xs):
        if not ps[i]:
            continue
        for j, xj in enumerate(xs):
            if not ps[j]:
                tot += 2 * (xj < xi) + (xj == xi)
    return tot, sum(ps), len(ps) - sum(ps)


def counts(scores, y, masks, C):
    """int64 [3, S, 3] = {twoU, P, Nn} per (split, column) of the pooled scores [M, S]; a row whose label is outside [0, C) is in no split."""
    scores = np.asarray(scores, dtype=np.float32)
    M, S = scores.shape
    y = np.asarray(y, dtype=np.int64)
    ok = (y >= 0) & (y < C)
    out = np.zeros((3, S, 3), dtype=np.int64)
    for s in range(3):
        m = (np.asarray(masks[s]) != 0) & ok
        for c in range(S):
            out[s, c] = two_u(scores[:, c], y == (1 if S == 1 else c), m)
    return out


def counts_of_keys(keys, S):
    """The same table from any array of packed keys (every field read back from the key's bits; the score's order image stands in for the
    score, which test_auc_cpu.py pins to the float order)."""
    k = np.asarray(keys).astype(np.uint64)
    col = (k >> np.uint64(36)).astype(np.int64)
    img = ((k >> np.uint64(4)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    pos = ((k >> np.uint64(3)) & np.uint64(1)) != 0
    out = np.zeros((3, S, 3), dtype=np.int64)
    for s in range(3):
        m = ((k >> np.uint64(s)) & np.uint64(1)) != 0
        for c in range(S):
            sel = m & (col == c)
            neg = np.sort(img[sel & ~pos])
            xp = img[sel & pos]
            u = np.searchsorted(neg, xp, side="left").astype(np.int64).sum() + np.searchsorted(neg, xp, side="right").astype(np.int64).sum()
            out[s, c] = (int(u), xp.size, neg.size)
    return out


def auc(cnt):
    """(triple, per_class) in float64 from a [3, S, 3] table: NaN where P Nn == 0, the mean over the defined columns, 0.0 if there is none."""
    per = [[(int(u) / (2 * int(p) * int(n))) if int(p) * int(n) > 0 else float("nan") for u, p, n in row] for row in np.asarray(cnt).tolist()]
    tri = []
    for row in per:
        have = [v for v in row if v == v]
        tri.append(sum(have) / len(have) if have else 0.0)
    return tuple(tri), per
