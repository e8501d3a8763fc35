"""GPU: sgs_auc_pack and sgs_auc_counts through the C ABI, outputs and the exactly sized workspace between red zones, against
tests/auc_ref.py by exact integer equality.  With T = sgs_auc_block_items(): n in {0, 1, 2, T - 1, T, T + 1, 3 T + 5} items (the first n keys
of a packed block) for S in {1, 3, 41}; M = 7 rows of S = 41 (many columns in one tile); M = T and T + 1 rows of S = 3 (a column start on and
off a tile edge).  Score patterns: normal, small integers, all equal, one tie run from inside tile 0 to inside tile 3 of a column, signed
zeros, infinities, denormals, NaN.  Labels outside [0, C) on masked rows (dropped) and on unmasked rows (ignored).  Masks: overlapping
splits, one empty split, all rows, no rows, a split with only positives, a split with only negatives."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref as R  # noqa: E402
from zoned import DEV, Zoned  # noqa: E402

pytestmark = pytest.mark.gpu
PATTERNS = ("normal", "ints", "equal", "long run", "zeros", "inf", "denormal", "nan")
MASKS = ("overlap", "one empty", "all rows", "no rows", "only positives", "only negatives")
FILL = -(1 << 62) + 12345


@pytest.fixture(scope="module")
def lib():
    import sgs_gnn_amd as S
    return S._lib.lib()


def _T():
    import sgs_gnn_amd as S
    return S.ops.auc_block_items()


def _scores(M, S, pattern, rng, T):
    x = rng.standard_normal((M, S)).astype(np.float32)
    if pattern == "ints":
        x = rng.integers(-2, 3, (M, S)).astype(np.float32)
    elif pattern == "equal":
        x[:] = np.float32(-0.0) if S == 1 else np.float32(0.75)
    elif pattern == "long run":                     # per column: T / 2 lower items, then ONE run that ends three items before the column's end
        lo = min(T // 2, M // 3)
        for c in range(S):
            col = np.full(M, 0.25, dtype=np.float32)
            col[:lo] = -1.0 - rng.random(lo).astype(np.float32)
            col[M - min(3, M // 3):] = 5.0 + np.arange(min(3, M // 3), dtype=np.float32)
            x[:, c] = col[rng.permutation(M)]
    elif pattern == "zeros":
        x = rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45], dtype=np.float32), (M, S))
    elif pattern == "inf":
        x = rng.choice(np.array([np.inf, -np.inf, 3.4e38, -3.4e38, 0.0, 1.0], dtype=np.float32), (M, S))
    elif pattern == "denormal":
        x = (rng.integers(-5, 6, (M, S)) * np.float32(1e-45)).astype(np.float32)
        x[rng.random((M, S)) < 0.2] = np.float32(1.17549435e-38)                 # the smallest normal beside them
    elif pattern == "nan":
        x[rng.random((M, S)) < 0.3] = np.nan
        if M:
            x[0, 0] = -np.nan                                                    # the sign bit of a NaN changes nothing
    return x


def _labels_masks(M, S, C, kind, rng):
    y = rng.integers(0, C, M).astype(np.int64)
    u = rng.random(M)
    t0 = 1 if S == 1 else 0
    if kind == "overlap":
        masks = [u < 0.5, (u > 0.3) & (u < 0.7), u > 0.8]
    elif kind == "one empty":
        masks = [u < 0.4, np.zeros(M, dtype=bool), u > 0.5]
    elif kind == "all rows":
        masks = [np.ones(M, dtype=bool), u < 0.5, np.ones(M, dtype=bool)]
    elif kind == "no rows":
        masks = [np.zeros(M, dtype=bool)] * 3
    elif kind == "only positives":
        masks = [u < 0.6, y == t0, u > 0.5]
    else:
        masks = [u < 0.6, u > 0.5, (y != t0) & (u < 0.9)]
    anym = masks[0] | masks[1] | masks[2]
    out = (~anym).nonzero()[0]
    y[out[0::2]] = -100                                                          # rows outside every mask may hold any label
    y[out[1::2]] = C
    bad = anym.nonzero()[0][5::11]                                               # masked rows with a label outside [0, C): dropped
    y[bad[0::2]] = C
    y[bad[1::2]] = -1
    u8 = [np.where(m, rng.integers(1, 256, M), 0).astype(np.uint8) for m in masks]          # any non-zero byte is "in the split"
    return y, u8


def _pack(lib, x, y, u8, C):
    M, S = x.shape
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (x, y, *u8)]
    keys = Zoned(M * S, torch.int64, FILL)
    rc = lib.sgs_auc_pack(d[0].data_ptr(), M, S, C, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), keys.ptr, None)
    assert rc == 0, lib.sgs_last_error()
    torch.cuda.synchronize()
    got = keys.get().view(np.uint64)
    assert np.array_equal(got, R.pack_keys(x, y, u8, C))                         # bit for bit
    return keys, got


def _counts(lib, keys_ptr, n, S):
    out = Zoned(9 * S, torch.int64, FILL)
    nbytes = lib.sgs_auc_counts_workspace_bytes(n, S)
    assert nbytes % 8 == 0
    ws = Zoned(nbytes // 8, torch.int64, FILL)
    rc = lib.sgs_auc_counts(keys_ptr, n, S, out.ptr, ws.ptr, nbytes, None)
    assert rc == 0, lib.sgs_last_error()
    torch.cuda.synchronize()
    ws.get()                                                                     # the red zones around the workspace
    return out.get().reshape(3, S, 3).copy()


def _sizes():
    T = 2048                                                                     # test_block_items pins it to the library's answer
    out = [("n", n, S) for S in (1, 3, 41) for n in (0, 1, 2, T - 1, T, T + 1, 3 * T + 5)]
    return out + [("M", 7, 41), ("M", T, 3), ("M", T + 1, 3), ("M", 3 * T + 5, 3)]


def test_block_items(lib):
    assert lib.sgs_auc_block_items() == 2048 == _T()


@pytest.mark.parametrize("what,size,S", _sizes(), ids=lambda v: str(v))
def test_pack_and_counts_are_exact(lib, what, size, S):
    T = _T()
    C = 2 if S == 1 else S
    M = size if what == "M" else -(-size // S)
    n = M * S if what == "M" else size
    rng = np.random.default_rng(1000 * size + S)
    for pi, pattern in enumerate(PATTERNS):
        if pattern == "long run" and M < 9:
            continue
        kinds = MASKS if pattern in ("normal", "ints") else (MASKS[pi % len(MASKS)], "overlap")
        for kind in kinds:
            x = _scores(M, S, pattern, rng, T)
            y, u8 = _labels_masks(M, S, C, kind, rng)
            keys, knp = _pack(lib, x, y, u8, C)
            got = _counts(lib, keys.ptr, n, S)
            want = R.counts_of_keys(knp[:n], S)
            assert np.array_equal(got, want), (pattern, kind)
            if n == M * S:
                assert np.array_equal(got, R.counts(x, y, u8, C)), (pattern, kind)                 # from the float scores themselves
            assert np.array_equal(_counts(lib, keys.ptr, n, S), got), (pattern, kind)              # the same bits on a second call
            tu, P, Nn = got[..., 0], got[..., 1], got[..., 2]
            assert (tu >= 0).all() and (tu <= 2 * P * Nn).all()
            if pattern == "equal":
                assert np.array_equal(tu, P * Nn)
            if kind == "no rows":
                assert not got.any()
            if kind == "one empty":
                assert not got[1].any()
            if kind == "only positives" and n == M * S:
                assert not got[1, 0, 2] and (S == 1 or not got[1, 1:, 1].any())
            if kind == "only negatives" and n == M * S:
                assert not got[2, 0, 1]
    keys.get()                                                                   # sgs_auc_counts leaves its input alone: zones and payload
    assert np.array_equal(keys.get().view(np.uint64), knp)


def test_long_run_crosses_three_tile_edges(lib):
    """The planted run of the "long run" pattern really starts inside tile 0 and ends inside tile 3 of the sorted keys, in one column
    (S = 1) and in a column that starts off a tile edge (S = 3, column 1)."""
    T = _T()
    M = 3 * T + 5
    for S in (1, 3):
        C = 2 if S == 1 else S
        rng = np.random.default_rng(S)
        x = _scores(M, S, "long run", rng, T)
        y, u8 = _labels_masks(M, S, C, "overlap", rng)
        keys, knp = _pack(lib, x, y, u8, C)
        srt = np.sort(knp >> np.uint64(4), kind="stable")
        c = S - 1 if S == 1 else 1
        v = (np.uint64(c) << np.uint64(32)) | np.uint64(int(R.order_image(np.float32([0.25]))[0]))
        at = np.nonzero(srt == v)[0]
        assert at[0] // T == (c * M) // T and at[0] % T != 0 and at[-1] // T == at[0] // T + 3 and (at[-1] + 1) % T != 0
        assert at.size == at[-1] - at[0] + 1 > 2 * T
        got = _counts(lib, keys.ptr, M * S, S)
        assert np.array_equal(got, R.counts(x, y, u8, C))
        assert got[0, c, 1] > 100 and got[0, c, 2] > 100


def test_any_order_of_the_keys_and_ignored_columns(lib):
    T = _T()
    S, C, M = 3, 3, T + 77
    rng = np.random.default_rng(7)
    x = _scores(M, S, "ints", rng, T)
    y, u8 = _labels_masks(M, S, C, "overlap", rng)
    keys, knp = _pack(lib, x, y, u8, C)
    want = R.counts(x, y, u8, C)
    assert want[:, :, 0].all()                                                   # every cell is exercised
    for perm in (rng.permutation(M * S), np.arange(M * S)[::-1]):
        sh = Zoned(M * S, torch.int64, FILL)
        sh.set(knp[perm].view(np.int64))
        assert np.array_equal(_counts(lib, sh.ptr, M * S, S), want)
    # the same keys counted with S = 2 break the contract (columns < S): the counts are unspecified, but column 2 is never used as an index
    # into the [3, 2, 3] output (_counts checks the red zones around it and around the workspace)
    assert _counts(lib, keys.ptr, M * S, 2).shape == (3, 2, 3)


def test_ops_wrappers_and_calculate_auc():
    import sgs_gnn_amd as Sg
    ops = Sg.ops
    rng = np.random.default_rng(3)
    for C in (2, 5):
        M = 301
        lg = torch.from_numpy(rng.integers(-3, 4, (M, C)).astype(np.float32) * 0.5).to(DEV)
        S = 1 if C == 2 else C
        y, u8 = _labels_masks(M, S, C, "overlap", rng)
        masks = [torch.from_numpy(m != 0).to(DEV) for m in u8]
        sc = ops.auc_scores(lg)
        assert sc.shape == (M, S) and sc.dtype == torch.float32 and sc.is_contiguous()
        want_sc = (lg[:, 1] - lg[:, 0]).unsqueeze(1) if C == 2 else torch.log_softmax(lg, 1)
        assert torch.equal(sc, want_sc)
        keys = ops.auc_pack(sc, torch.from_numpy(y).to(DEV), masks, C)
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), R.pack_keys(sc.cpu().numpy(), y, u8, C))
        cnt = ops.auc_counts(keys, S)
        want = R.counts(sc.cpu().numpy(), y, u8, C)
        assert cnt.dtype == torch.int64 and cnt.shape == (3, S, 3) and np.array_equal(cnt.cpu().numpy(), want)
        two = ops.auc_counts(torch.cat([keys, keys]), S).cpu().numpy()          # a concatenation: every count doubles, every pair count x 4
        assert np.array_equal(two[..., 1:], 2 * want[..., 1:]) and np.array_equal(two[..., 0], 4 * want[..., 0])
        for s in range(3):
            got = Sg.calculate_auc(lg, torch.from_numpy(y).to(DEV), masks[s])
            assert got == R.auc(want)[0][s]
        assert Sg.calculate_auc(lg, torch.from_numpy(y).to(DEV), torch.zeros_like(masks[0])) == 0.0
        assert np.array_equal(ops.auc_counts(keys[:0], S).cpu().numpy(), np.zeros((3, S, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="C >= 2"):
        ops.auc_scores(torch.zeros(4, 1, device=DEV))
    with pytest.raises(RuntimeError, match="sgs_auc_pack"):
        ops.auc_pack(torch.zeros(4, 3, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), [torch.ones(4, dtype=torch.bool, device=DEV)] * 3, 2)
