"""GPU: sgs_spmm_csr_multi (D drawn subgraphs of one partition in one launch) against sgs_spmm_csr on each draw alone, bitwise, over every
case of tests/gcn_ref.py::SPMM_CASES with N <= 4096 -- every (VEC, LPR) of the lanes-per-row kernels, every (VEC, NW) of the waves-per-row
kernels on both sides of the 16 N / 256 N thresholds, hub rows of 200 to 7000 entries on both sides of sgs_spmm_long_rows_threshold().
The single call is pinned to fp64 by tests/test_gpu_gcn_variants.py and tests/test_gpu_spmm_long_rows.py, so the equality carries their
bound over to the multi-draw launcher, whose kernel choice has to be sgs_spmm_csr's for every draw.

Three draws per case (gcn_ref.graph seeds 0, 1, 2: the same N and nnz), stacked as ptr [3, N + 1], col / val [3, nnz + PAD]: the draw
stride of col / val is the call's `nnz` argument, the row pointers end at the real nnz.  That argument is also what the launcher picks
its kernel by, so the single call gets the same count (its result does not depend on it beyond the choice of kernel, and the two row
forms sum a row in different orders).  With PAD entries more than the table's nnz the lanes-per-row cases and the cases one entry below
a threshold land on the other side of it, so each case runs a second time on the draws packed back to back (col / val [3 * nnz] + PAD,
draw stride = the real nnz), where the launcher sees the table's own shape.  X shared (x_stride = 0), one block per draw
(N * Dc) and one block per draw at a stride that is no multiple of four floats (N * Dc + 1: draws 1 and 2 start off 16-byte alignment, so
the launch has to take VEC = 1).  Y is carved from a guarded buffer and pre-filled with NaN."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gcn_ref as R  # noqa: E402
from test_gpu_gcn_variants import DEV, SEED, SITE, dptr, guarded, red_zones_intact  # noqa: E402

pytestmark = pytest.mark.gpu
DRAWS = 3
CASES = [c for c in R.SPMM_CASES if c["N"] <= 4096]
# (diag, bias, act): every pair of settings occurs (act in {NONE, RELU}: the multi-draw launcher is forward-only, no dropout)
COMBOS = [(True, True, R.ACT_NONE), (False, False, R.ACT_NONE), (True, False, R.ACT_RELU), (False, True, R.ACT_RELU)]


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


def test_the_case_list_is_the_table_but_its_two_large_cases():
    assert len(CASES) == len(R.SPMM_CASES) - 2 and max(c["N"] for c in CASES) == 300
    assert {c["N"] for c in R.SPMM_CASES} - {c["N"] for c in CASES} == {65536, 65537}
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert {(c[a], c[b]) for c in COMBOS} == {(x, y) for x in (c[a] for c in COMBOS) for y in (c[b] for c in COMBOS)}


def x_block(X, stride, off):
    """-> (buffer, [views of the DRAWS blocks]): block d starts `off + d * stride` floats past a 256-byte boundary (stride 0: one block)."""
    n = X[0].numel()
    buf = torch.zeros(off + (DRAWS - 1) * stride + n + 4, dtype=torch.float32, device=DEV)
    views = []
    for d in range(DRAWS):
        v = buf[off + d * stride:off + d * stride + n].view(X[0].shape)
        v.copy_(X[d if stride else 0])
        views.append(v)
    return buf, views


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_every_draw_of_a_multi_launch_is_the_single_call_bitwise(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    N, Dc, nnz = case["N"], case["D"], case["nnz"]
    grs = [R.graph(N, nnz, case["nw"], case["hub"], seed=s) for s in range(DRAWS)]
    assert all(g["nnz"] == nnz and int(g["ptr"][-1]) == nnz for g in grs)
    ptr = torch.stack([g["ptr"] for g in grs]).contiguous().to(DEV)
    padded = [torch.stack([g[k] for g in grs]).reshape(-1).to(DEV) for k in ("col", "val")]                          # [3, nnz + PAD]
    packed = [torch.cat([g[k][:nnz] for g in grs] + [grs[0][k][nnz:]]).to(DEV) for k in ("col", "val")]              # [3 * nnz] + PAD
    assert padded[0].numel() == DRAWS * (nnz + R.PAD) and packed[0].numel() == DRAWS * nnz + R.PAD
    Xoff, Yoff = (1 if case["align"] == "a" else 0), (1 if case["align"] == "b" else 0)
    Xs, diags = [], []
    for s in range(DRAWS):
        X, diag, bias = R.spmm_inputs(N, Dc, 0.0, seed=5 + s)
        Xs.append(X)
        diags.append(diag)
    diag_all, bias_d = torch.stack(diags).contiguous().to(DEV), bias.to(DEV)
    st = ops._stream()
    prev = L.sgs_spmm_long_rows_set(1)
    try:
        for (col, val), cnt in ((padded, nnz + R.PAD), (packed, nnz)):         # cnt: the draw stride of col / val = the call's nnz
            if cnt == nnz:
                assert L.sgs_spmm_csr_variant(N, Dc, cnt, 0 if case["align"] else 1) == case["code"]
            for stride in (0, N * Dc, N * Dc + 1):
                xbuf, xv = x_block(Xs, stride, Xoff)
                for long_on in (1, 0):
                    L.sgs_spmm_long_rows_set(long_on)
                    for diag_on, bias_on, act in COMBOS:
                        tag = f"{case['name']} nnz arg={cnt} x_stride={stride} long={long_on} diag={diag_on} bias={bias_on} act={act}"
                        buf, Y = guarded(DRAWS * N * Dc, Yoff)
                        ops._lib.check(L.sgs_spmm_csr_multi(xv[0].data_ptr(), stride, N, Dc, cnt, DRAWS, ptr.data_ptr(), col.data_ptr(),
                                                            val.data_ptr(), dptr(diag_all if diag_on else None),
                                                            dptr(bias_d if bias_on else None), act, Y.data_ptr(), st), "sgs_spmm_csr_multi")
                        torch.cuda.synchronize()
                        assert red_zones_intact(buf, DRAWS * N * Dc, Yoff), tag
                        assert not bool(torch.isnan(Y).any()), tag
                        Y = Y.view(DRAWS, N, Dc)
                        for d in range(DRAWS):
                            sbuf, Y1 = guarded(N * Dc, Yoff)
                            ops._lib.check(L.sgs_spmm_csr(xv[d].data_ptr(), N, Dc, cnt, ptr[d].data_ptr(), col[d * cnt:].data_ptr(),
                                                          val[d * cnt:].data_ptr(), dptr(diag_all[d] if diag_on else None),
                                                          dptr(bias_d if bias_on else None), act, 0.0, SEED, SITE, Y1.data_ptr(), st),
                                           "sgs_spmm_csr")
                            torch.cuda.synchronize()
                            assert torch.equal(Y[d], Y1.view(N, Dc)) and red_zones_intact(sbuf, N * Dc, Yoff), f"{tag} draw {d}"
    finally:
        L.sgs_spmm_long_rows_set(prev)


def test_overlap_and_bad_stride_are_refused_before_any_launch(pkg):
    L, ops = pkg._lib.lib(), pkg.ops
    N, Dc, nnz = 64, 8, 16 * 64
    gr = R.graph(N, nnz, 4, 200)
    ptr, col, val = (torch.stack([gr[k]] * DRAWS).contiguous().to(DEV) for k in ("ptr", "col", "val"))
    buf = torch.full((2 * DRAWS * N * Dc,), float("nan"), device=DEV)
    X, Y = buf[:DRAWS * N * Dc], buf[DRAWS * N * Dc:]

    def call(x, stride, y):
        return L.sgs_spmm_csr_multi(x.data_ptr(), stride, N, Dc, nnz + R.PAD, DRAWS, ptr.data_ptr(), col.data_ptr(), val.data_ptr(), None, None,
                                    R.ACT_NONE, y.data_ptr(), ops._stream())
    assert call(X, N * Dc - 1, Y) == -1 and b"x_stride" in L.sgs_last_error()                     # SGS_EINVAL: draws' blocks of X overlap
    assert call(X, N * Dc, buf[(DRAWS - 1) * N * Dc + 1:]) == -1 and b"overlap" in L.sgs_last_error()      # Y starts inside X's last block
    assert call(X, 0, X[N * Dc - 1:]) == -1 and b"overlap" in L.sgs_last_error()                  # shared X: Y starts on its last element
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())                                                           # nothing was launched
