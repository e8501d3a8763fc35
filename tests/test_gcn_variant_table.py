"""CPU: the case tables of tests/test_gpu_gcn_variants.py (tests/gcn_ref.py) reach EVERY kernel variant that sgs_spmm_csr, sgs_sddmm_csr,
sgs_colsum and sgs_act_bwd_colsum can launch (asked of the built library's own dispatch queries), straddle every dispatch threshold, and
the fp64 reference they are compared with agrees with the oracle's GCN layer and stays inside its own error bounds in fp32."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gcn_ref as R  # noqa: E402
from oracle import sgs_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd._lib.lib()


# kind * 1000 + VEC * 100 + W (include/sgs_hip.h).  One line per reachable code.
CSR_REACHABLE = {
    101: "lanes, VEC 1, LPR 1: D = 1",
    102: "lanes, VEC 1, LPR 2: D = 2",
    104: "lanes, VEC 1, LPR 4: D = 3, or D = 4 off alignment",
    108: "lanes, VEC 1, LPR 8: D = 5..8 (8 off alignment)",
    116: "lanes, VEC 1, LPR 16: D = 9..16",
    132: "lanes, VEC 1, LPR 32: D = 17..32",
    164: "lanes, VEC 1, LPR 64: D >= 33 (D > 64: several column passes)",
    401: "lanes, VEC 4, LPR 1: D = 4",
    402: "lanes, VEC 4, LPR 2: D = 8",
    404: "lanes, VEC 4, LPR 4: D = 12, 16",
    408: "lanes, VEC 4, LPR 8: D = 20..32",
    416: "lanes, VEC 4, LPR 16: D = 36..64",
    432: "lanes, VEC 4, LPR 32: D = 68..128",
    464: "lanes, VEC 4, LPR 64: D >= 132 (D > 256: several column passes)",
    1104: "row-block, VEC 1, 4 waves: long rows below the 16-wave threshold",
    1116: "row-block, VEC 1, 16 waves",
    1404: "row-block, VEC 4, 4 waves",
    1416: "row-block, VEC 4, 16 waves",
}
# kind * 1000000 + F * 100000 + rows * 100 + RG.  F = 0 (sgs_colsum) and F = 1 (sgs_act_bwd_colsum) for each.
COLSUM_REACHABLE = {
    1000000: "colsum_small: 0 < N <= 2048, D % 4 != 0",
    2000000: "colsum_small_v4: 0 < N <= 2048, D % 4 == 0",
    3000000: "vecsum_small: D = 1, 2048 < N <= 2^20",
    4003204: "32-row chunks, final<4>: only N = 0 (no chunk at all; 2048 < N < 4096 gives 65..128 chunks)",
    4003216: "32-row chunks, final<16>: 2048 < N < 4096",
    4012804: "128-row chunks, final<4>: 4096 <= N <= 8192 (at most 64 chunks)",
    4012816: "128-row chunks, final<16>: 8192 < N < 16384",
    4025604: "256-row chunks, final<4>: only N = 16384 (exactly 64 chunks)",
    4025616: "256-row chunks, final<16>: N > 16384",
}


def _al(case):
    return 0 if case["align"] else 1


def test_spmm_and_sddmm_tables_reach_every_variant(L):
    for cases, query in ((R.SPMM_CASES, L.sgs_spmm_csr_variant), (R.SDDMM_CASES, L.sgs_sddmm_csr_variant)):
        got = set()
        for c in cases:
            code = query(c["N"], c["D"], c["nnz"], _al(c))
            assert code == c["code"], (c["name"], code)
            got.add(code)
        assert got == set(CSR_REACHABLE), sorted(got ^ set(CSR_REACHABLE))
        assert len({c["name"] for c in cases}) == len(cases)


def test_csr_reachable_set_is_the_dispatch_s_whole_range(L):
    """Sweep the queries over shapes on every side of every threshold: nothing outside the enumerated set comes back, all of it does."""
    for query, wide in ((L.sgs_spmm_csr_variant, 256), (L.sgs_sddmm_csr_variant, 64)):
        seen = set()
        for N in (1, 64, 65536, 65537, 70000):
            for nnz in (0, 16 * N - 1, 16 * N, wide * N - 1, wide * N, 1000 * N):
                for D in list(range(1, 140)) + [256, 260, 512, 1000]:
                    for al in (0, 1):
                        seen.add(query(N, D, nnz, al))
        assert seen == set(CSR_REACHABLE)


def test_pair_dual_and_cheb_queries_are_answers_of_the_spmm_variant(L):
    """The layer-pair / two-job predicates and the Chebyshev step's variant are read off sgs_spmm_csr_variant's choice, on a grid that
    straddles every threshold (host queries only; nothing is launched)."""
    Dn = 41
    for N in (1, 64, 65536, 65537):
        counts = (16 * N - 1, 16 * N, 256 * N - 1, 256 * N)
        for D in (1, 4, 41, 512, 513):
            for nnz in counts:
                for al in (0, 1):
                    code = L.sgs_spmm_csr_variant(N, D, nnz, al)
                    assert L.sgs_gcn_pair_ok(N, nnz, D) == int(code >= 1000 and D <= 512), (N, nnz, D, al)
                    if D % 4 == 0 or al == 0:
                        assert L.sgs_cheb_spmm_variant(N, D, nnz, D, al) == code, (N, nnz, D, al)
            for a in counts:
                for b in counts:
                    both = L.sgs_gcn_pair_ok(N, a, D) and L.sgs_gcn_pair_ok(N, b, D)
                    same_w = L.sgs_spmm_csr_variant(N, D, a, 1) % 100 == L.sgs_spmm_csr_variant(N, D, b, 1) % 100
                    assert L.sgs_gcn_dual_ok(N, a, b, D, Dn) == int(bool(both and same_w)), (N, a, b, D)


def test_colsum_table_reaches_every_variant(L):
    want = set(COLSUM_REACHABLE) | {c + R.FUSED for c in COLSUM_REACHABLE}
    got = set()
    for c in R.COLSUM_CASES:
        for fused in (0, 1):
            code = L.sgs_colsum_variant(c["N"], c["D"], fused)
            assert code == c["code"] + fused * R.FUSED, (c["name"], fused, code)
            got.add(code)
    assert got == want, sorted(got ^ want)
    seen = set()
    for N in list(range(0, 3)) + [2047, 2048, 2049, 4095, 4096, 8192, 8193, 16383, 16384, 16385, 1 << 20, (1 << 20) + 1, 1 << 22]:
        for D in (1, 2, 3, 4, 41, 64, 65, 256):
            for fused in (0, 1):
                seen.add(L.sgs_colsum_variant(N, D, fused))
    assert seen == want


def _has(cases, **kw):
    return any(all(c[k] == v for k, v in kw.items()) for c in cases)


def test_every_threshold_is_straddled():
    sp, sd, cs = R.SPMM_CASES, R.SDDMM_CASES, R.COLSUM_CASES
    for cases, wide in ((sp, 256), (sd, 64)):
        for vecD in ((256, 128), (41, 41)):                  # both VEC values at both thresholds
            for mult, D in ((16, vecD[0]), (wide, vecD[1])):
                on = [c for c in cases if c["nnz"] == mult * c["N"] and c["D"] == D and not c["align"]]
                assert on, (mult, D)
                assert any(_has(cases, N=c["N"], D=D, nnz=c["nnz"] - 1, align="") for c in on), (mult, D)
    assert _has(sp, N=65536, nnz=16 * 65536, code=1404) and _has(sp, N=65537, nnz=16 * 65537, code=402)
    assert _has(sd, N=70000, nnz=16 * 70000, code=1404) and _has(sd, N=70000, nnz=16 * 70000 - 1, code=402)
    for nw in (1104, 1116):                                  # SDDMM row-block: D = 64 VEC against 64 VEC + VEC
        assert _has(sd, code=nw, D=64) and _has(sd, code=nw, D=65)
    for nw in (1404, 1416):
        assert _has(sd, code=nw, D=256) and _has(sd, code=nw, D=260)
    for a, b in ((2048, 2049), (4095, 4096), (16383, 16384), (8192, 8193), (16384, 16385)):      # the last two: 64 against 65 chunks
        assert any(c["N"] == a and c["D"] > 1 for c in cs) and any(c["N"] == b and c["D"] > 1 for c in cs), (a, b)
    assert _has(cs, N=2048, D=1) and _has(cs, N=2049, D=1) and _has(cs, N=1 << 20, D=1) and _has(cs, N=(1 << 20) + 1, D=1)
    assert {c["D"] for c in cs} >= {1, 3, 16, 41, 64, 65, 256}
    assert {c["D"] for c in sp} >= {1, 3, 4, 8, 41, 64, 128, 256, 260, 512}
    assert any(c["spread"] for c in cs)


def test_row_length_builder_places_the_tail_lengths():
    for nw in (4, 16):
        gr = R.graph(64, 256 * 64, nw=nw, hub=5000, seed=1)
        ln = gr["lens"].tolist()
        assert sum(ln) == 256 * 64 == int(gr["ptr"][-1])
        assert ln[0] == 8 * nw + 1 and ln[-1] == 8 * nw - 1 and ln[1] == 0
        assert set(R.special_lengths(nw)) <= set(ln) and 5000 in ln
        assert sorted(gr["eid"][:gr["nnz"]].tolist()) == list(range(gr["nnz"]))
        r = R.rows_of(gr["ptr"])
        assert bool((gr["col"][:gr["nnz"]].long() == r).any())                       # self entries occur
    assert sum(R.row_lengths(70000, 16 * 70000 - 1, 4, 40000)) == 16 * 70000 - 1


@pytest.mark.parametrize("N,E,seed", [(30, 200, 1), (57, 900, 2), (12, 40, 3)])
@pytest.mark.parametrize("weighted", [True, False])
def test_reference_composes_to_the_oracle_s_gcn_layer(N, E, seed, weighted):
    """spmm / sddmm / colsum of gcn_ref.py, composed into GCNConv's forward and its hand-written backward, against oracle.gcn_conv and
    autograd in fp64: y, dx, dW (and the gradient wrt the normalised weights, against autograd through the same normalisation)."""
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei = ei[:, ei[0] != ei[1]]                       # (loops are the normalisation's business: the diag term below carries them)
    E = ei.shape[1]
    Fin, D = 5, 7
    x = torch.randn(N, Fin, generator=g, dtype=torch.float64).requires_grad_(True)
    W = torch.randn(D, Fin, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(D, generator=g, dtype=torch.float64).requires_grad_(True)
    w = (torch.rand(E, generator=g, dtype=torch.float64) + 0.1) if weighted else None
    gy = torch.randn(N, D, generator=g, dtype=torch.float64)
    y = O.gcn_conv(x, ei, w, W, b)
    y.backward(gy)
    # the normalised weights, by the oracle; CSR by destination (forward) and by source (backward), entries in edge order
    ei2, wh = O.gcn_norm(ei, w, N, dtype=torch.float64)
    what, wloop = wh[:E], wh[E:]

    def csr(rows, cols):
        order = torch.argsort(rows, stable=True)
        ptr = torch.zeros(N + 1, dtype=torch.int64)
        ptr[1:] = torch.bincount(rows, minlength=N).cumsum(0)
        return ptr, cols[order], order
    in_ptr, in_src, in_eid = csr(ei[1], ei[0])
    out_ptr, out_dst, out_eid = csr(ei[0], ei[1])
    xl = (x @ W.t()).detach()
    y_ref = R.spmm(in_ptr, in_src, what[in_eid], wloop, b.detach(), xl)
    assert float((y_ref - y.detach()).abs().max()) <= 1e-12
    dxl = R.spmm(out_ptr, out_dst, what[out_eid], wloop, None, gy)
    assert float((dxl @ W.detach() - x.grad).abs().max()) <= 1e-12
    assert float((dxl.t() @ x.detach() - W.grad).abs().max()) <= 1e-12
    assert float((R.colsum(gy) - b.grad).abs().max()) <= 1e-12
    gw, gl = R.sddmm(in_ptr, in_src, in_eid, gy, xl)
    whr = wh.clone().requires_grad_(True)
    msg = whr.unsqueeze(1) * xl[ei2[0]]
    (torch.zeros(N, D, dtype=torch.float64).index_add(0, ei2[1], msg) * gy).sum().backward()
    assert float((torch.cat([gw, gl]) - whr.grad).abs().max()) <= 1e-12


def _keep(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= R.P_DROP


@pytest.mark.parametrize("case", R.SPMM_CASES, ids=lambda c: c["name"])
def test_spmm_reference_in_fp32_is_inside_its_bound_and_dropout_cases_show_their_mask(case):
    gr = R.graph(case["N"], case["nnz"], case["nw"], case["hub"])
    n = gr["nnz"]
    ptr, col, val = gr["ptr"], gr["col"][:n], gr["val"][:n]
    for diag_on, bias_on, act in R.SPMM_COMBOS:
        X, diag, bias = R.spmm_inputs(case["N"], case["D"], R.DROP_BIAS if act == R.ACT_RELU_DROPOUT else 0.0)
        diag, bias = (diag if diag_on else None), (bias if bias_on else None)
        Z = R.spmm_pre(ptr, col, val.double(), None if diag is None else diag.double(), None if bias is None else bias.double(), X.double())
        pb = R.spmm_pre_bound(ptr, col, val, diag, bias, X)
        keep = _keep(Z.shape, 3) if act == R.ACT_RELU_DROPOUT else None
        Y = R.activate(Z, act, keep, R.P_DROP)
        Y32 = R.spmm(ptr, col, val, diag, bias, X, act, keep, R.P_DROP)
        assert Y32.dtype == torch.float32
        assert bool(((Y32.double() - Y).abs() <= R.spmm_bound(pb, Y, act, R.P_DROP)).all())
        if act == R.ACT_RELU_DROPOUT:          # a condition on the reference alone: the share of elements that hide their kept bit
            assert float(R.ambiguous(Z, pb).double().mean()) <= R.MAX_AMBIGUOUS


@pytest.mark.parametrize("case", R.SDDMM_CASES, ids=lambda c: c["name"])
def test_sddmm_reference_in_fp32_is_inside_its_bound(case):
    gr = R.graph(case["N"], case["nnz"], case["nw"], case["hub"])
    n = gr["nnz"]
    A = torch.randn(case["N"], case["D"], generator=gr["gen"])
    B = torch.randn(case["N"], case["D"], generator=gr["gen"])
    g64, d64 = R.sddmm(gr["ptr"], gr["col"][:n], gr["eid"][:n], A.double(), B.double())
    g32, d32 = R.sddmm(gr["ptr"], gr["col"][:n], gr["eid"][:n], A, B)
    bg, bd = R.sddmm_bound(gr["ptr"], gr["col"][:n], gr["eid"][:n], A, B)
    assert bool(((g32.double() - g64).abs() <= bg).all()) and bool(((d32.double() - d64).abs() <= bd).all())


@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=lambda c: c["name"])
def test_colsum_reference_in_fp32_is_inside_its_bound(case):
    A, Y = R.colsum_inputs(case)
    assert bool(((R.colsum(A).double() - R.colsum(A.double())).abs() <= R.colsum_bound(A)).all())
    for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_RELU_DROPOUT):
        dZ = R.act_bwd(A, Y, act, R.P_DROP)
        assert dZ.dtype == torch.float32 and bool((dZ[Y <= 0] == 0).all() or act == R.ACT_NONE)
        assert bool(((R.colsum(dZ).double() - R.colsum(dZ.double())).abs() <= R.colsum_bound(dZ)).all())
