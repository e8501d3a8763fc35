"""CPU: the case tables of tests/test_gpu_cheb_kernels.py (tests/cheb_kernels_ref.py) reach EVERY kernel sgs_cheb_spmm can launch (asked
of the built library's sgs_cheb_spmm_variant, which the launchers switch on), state the right code per case and straddle every dispatch
threshold; the kernel-level fp64 references, chained as ops._ChebConv chains the steps, equal the dense direct recurrence of
tests/cheb_ref.py and torch autograd through it; and every planted single fault of the references, evaluated in fp32, leaves the
element-wise bound on at least one case while the unmutated fp32 evaluation stays inside it on all of them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheb_kernels_ref as R  # noqa: E402
import cheb_ref as C  # noqa: E402
import gcn_ref as G  # noqa: E402
from gat_heads_ref import csr_of  # noqa: E402

F32, F64 = R.F32, R.F64


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd._lib.lib()


# VEC * 100 + LPR, 1000 + VEC * 100 + NW (include/sgs_hip.h, section K9).  One line per reachable code.
REACHABLE = {
    101: "lanes, VEC 1, LPR 1: D = 1",
    102: "lanes, VEC 1, LPR 2: D = 2",
    104: "lanes, VEC 1, LPR 4: D = 3, or D = 4 with X off alignment / ldx % 4 != 0",
    108: "lanes, VEC 1, LPR 8: D = 5..8",
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
    1104: "row per workgroup, VEC 1, 4 waves",
    1116: "row per workgroup, VEC 1, 16 waves",
    1404: "row per workgroup, VEC 4, 4 waves",
    1416: "row per workgroup, VEC 4, 16 waves",
}


# ------------------------------------------------------------------------------------------------ coverage
def test_every_case_states_the_query_s_code_and_the_table_reaches_every_code(L):
    assert len({c["name"] for c in R.STEP_CASES}) == len(R.STEP_CASES)
    got = set()
    for c in R.STEP_CASES:
        for combo in R.STEP_COMBOS:
            ldx, al = R.x_layout(c, combo)
            code = L.sgs_cheb_spmm_variant(c["N"], c["D"], c["nnz"], ldx, al)
            assert code == c["code"], (c["name"], combo["name"], code)
            got.add(code)
    assert got == set(REACHABLE), sorted(got ^ set(REACHABLE))


def test_reachable_set_is_the_dispatch_s_whole_range(L):
    Ds = sorted({d for p in (1, 2, 4, 8, 16, 32, 64, 128, 256) for d in (p - 1, p, p + 1) if d >= 1} | {260, 512, 1028})
    seen = set()
    for N in (1, 67, 65536, 65537):
        for D in Ds:
            for nnz in (0, 16 * N - 1, 16 * N, 256 * N - 1, 256 * N):
                for ldx in (D, D + 1, 3 * D):
                    for al in (0, 1):
                        seen.add(L.sgs_cheb_spmm_variant(N, D, nnz, ldx, al))
    assert seen == set(REACHABLE) and len(seen) == 18


def test_every_threshold_at_its_edge_and_bad_sizes(L):
    q = L.sgs_cheb_spmm_variant
    for N in (1, 67, 2100, 65536):
        for D, vec, lanes in ((64, 4, 416), (41, 1, 164)):
            assert [q(N, D, nnz, D, 1) for nnz in (16 * N - 1, 16 * N, 256 * N - 1, 256 * N)] == \
                [lanes, 1004 + 100 * vec, 1004 + 100 * vec, 1016 + 100 * vec], (N, D)
    assert q(65536, 4, 16 * 65536, 4, 1) == 1404 and q(65537, 4, 16 * 65537, 4, 1) == 401 and q(65537, 4, 300 * 65537, 4, 1) == 401
    for vec in (1, 4):                                       # LPR: the power of two >= ceil(D / VEC), at most 64
        for lg in range(7):
            D = vec << lg
            assert q(67, D, 0, D, int(vec == 4)) == 100 * vec + (1 << lg), (vec, D)
            assert q(67, D + vec, 0, D + vec, int(vec == 4)) == 100 * vec + min(2 << lg, 64), (vec, D)
    # VEC 4 needs all three: D % 4 == 0, ldx % 4 == 0, X aligned
    assert [q(67, 64, 0, 64, 1), q(67, 64, 0, 64, 0), q(67, 64, 0, 65, 1), q(67, 64, 0, 68, 1), q(67, 64, 0, 192, 1), q(67, 65, 0, 68, 1)] == \
        [416, 164, 164, 416, 416, 164]
    assert [q(0, 8, 0, 8, 1), q(8, 0, 0, 0, 1), q(0, 0, 0, 0, 0)] == [0, 0, 0]
    for bad in ((-1, 8, 0, 8), (8, -1, 0, 8), (8, 8, -1, 8), (8, 8, 0, -1)):
        assert q(*bad, 1) == -1, bad


def _has(**kw):
    return any(all(c[k] == v for k, v in kw.items()) for c in R.STEP_CASES)


def test_the_table_holds_every_case_it_promises():
    """Every case of the table is named by one assertion here: deleting one fails this test or the coverage test above."""
    for d, l in ((4, 1), (8, 2), (16, 4), (32, 8), (64, 16), (128, 32), (256, 64), (260, 64), (512, 64)):
        assert _has(N=67, D=d, nnz=1000, code=400 + l, hub=300, xoff=0, ldpad=0, yoff=0), d
    for d, l in ((1, 1), (2, 2), (3, 4), (7, 8), (13, 16), (29, 32), (41, 64), (130, 64)):
        assert _has(N=67, D=d, nnz=1000, code=100 + l, hub=300), d
    for d, l in ((16, 16), (64, 64)):                        # VEC 1 forced at D % 4 == 0, each of the three ways
        for xoff, ldpad in ((1, 0), (0, 1), (2, 4)):
            assert _has(N=67, D=d, nnz=1000, code=100 + l, xoff=xoff, ldpad=ldpad), (d, xoff, ldpad)
    assert _has(D=64, code=416, yoff=1, xoff=0, ldpad=0)     # Y, add, sub off alignment: the code stays
    for N, D, mult, code, nw in ((67, 64, 16, 1404, 4), (2100, 72, 16, 1404, 4), (67, 41, 16, 1104, 4), (67, 260, 256, 1416, 16),
                                 (520, 5, 256, 1116, 16), (67, 65, 256, 1116, 16), (67, 64, 256, 1416, 16), (67, 41, 256, 1116, 16)):
        assert _has(N=N, D=D, nnz=mult * N, code=code, nw=nw, xoff=0), (N, D, mult)
    assert _has(N=67, D=64, nnz=16 * 67, code=1104, xoff=1)
    for D, codes in ((64, (416, 1404)), (41, (164, 1104))):  # both thresholds from below, both vector widths
        assert _has(N=67, D=D, nnz=16 * 67 - 1, code=codes[0]) and _has(N=67, D=D, nnz=256 * 67 - 1, code=codes[1], nw=4), D
    assert _has(N=65536, D=4, nnz=16 * 65536, code=1404) and _has(N=65537, D=4, nnz=16 * 65537, code=401)
    assert _has(nnz=0) and _has(N=1, code=402) and _has(N=1, code=1404)
    assert any(c["lens"] is not None and sorted(c["lens"])[-2:] == [0, 300] for c in R.STEP_CASES)
    assert len(R.STEP_CASES) == 9 + 8 + 6 + 1 + 7 + 6 + 2 + 4
    for c in R.STEP_CASES:                                   # the graphs are what the table says
        if c["N"] > 3000:
            continue
        gr = R.case_graph(c)
        ln = gr["lens"].tolist()
        assert sum(ln) == c["nnz"] == int(gr["ptr"][-1]) and bool((gr["val"] < 0).all()) and gr["col"].numel() == c["nnz"] + G.PAD
        if c["lens"] is None:
            assert set(G.special_lengths(c["nw"])) <= set(ln) and max(ln) == c["hub"], c["name"]
    # each of add, sub, bias, Y2, in place, act occurs present and absent
    for f in (lambda k: k["add"] is not None, lambda k: k["sub"] is not None, lambda k: k["bias"], lambda k: k["Y2"] is not None,
              lambda k: k["add"] is not None and k["add"] == k["Y"], lambda k: k["act"] != R.ACT_NONE):
        assert {bool(f(k)) for k in R.STEP_COMBOS} == {False, True}
    assert {k["scale2"] for k in R.STEP_COMBOS if k["Y2"]} == {2.0, 0.75} and {k["alpha"] for k in R.STEP_COMBOS} == {1.0, 2.0}
    assert all(k["bias"] for k in R.STEP_COMBOS if k["act"] == R.ACT_RELU_DROPOUT)


def test_the_normalisation_graphs_plant_their_edge_cases():
    by = {c["name"]: c for c in R.NORM_CASES}
    assert len(by) == len(R.NORM_CASES) == 6
    c = by["small_directed"]
    s, d = c["ei"]
    assert c["N"] == 70 and c["n"] == 620 and int((s == d).sum()) == 3 and int((s == 11).sum()) == 0
    assert torch.unique(c["ei"], dim=1).shape[1] < 620                                   # duplicates
    c = by["long_rows"]
    assert 200 < int((c["ei"][0] == 3).sum()) < 256 and 200 < int((c["ei"][1] == 8).sum()) < 256 and int((c["ei"][0] == c["ei"][1]).sum()) >= 2
    c = by["zero_out_weights"]
    for mode in ("uniform", "log"):
        w = R.norm_weights(c, mode)
        assert int((c["ei"][0] == 7).sum()) > 0 and bool((w[c["ei"][0] == 7] == 0).all())
        assert float(R.norm_fwd(c["ei"], w, c["N"])[0][7]) == 0.0
    assert bool((by["only_self_edges"]["ei"][0] == by["only_self_edges"]["ei"][1]).all()) and by["no_edges"]["n"] == 0 and by["one_node"]["N"] == 1
    w = R.norm_weights(by["small_directed"], "log")
    assert float(w.min()) < 1e-5 and float(w.max()) > 1e2
    w = R.norm_weights(by["small_directed"], "uniform")
    assert 0.05 <= float(w.min()) and float(w.max()) <= 0.95 and R.norm_weights(by["small_directed"], "unit") is None


# ------------------------------------------------------------------------------------------------ composition
def _rel(got, ref):
    if ref.numel() == 0:
        return 0.0 if got.shape == ref.shape else float("inf")
    return float((got - ref).abs().max()) / (1.0 + float(ref.abs().max()))


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_steps_chained_as_the_layer_chains_them_equal_the_direct_recurrence(K, act):
    """ops._ChebConv.forward / backward restated over the step reference: Clenshaw's recurrence over column blocks, the backward's direct
    recurrence with Y2 = 2 U_k, dl as one SDDMM -- against cheb_ref.conv (dense, direct T_k) and torch autograd, to 1e-11 relative."""
    c = R.NORM_CASES[0]
    ei, N = c["ei"], c["N"]
    g = torch.Generator().manual_seed(K)
    Fin, D = 6, 5
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)          # noqa: E731
    x, Ws, bias, gy = rn(N, Fin), [rn(D, Fin) for _ in range(K)], rn(D), rn(N, D)
    w = torch.rand(ei.shape[1], generator=g, dtype=F64) + 0.1
    _, l0 = R.norm_fwd(ei, w, N)
    assert _rel(l0, C.laplacian(ei, w, N)[2]) <= 1e-11
    lv = [t.clone().requires_grad_(True) for t in [x, bias, l0] + Ws]
    Lh = torch.zeros(N, N, dtype=F64).index_put((ei[1], ei[0]), lv[2], accumulate=True)
    ref = C.conv(lv[0], lv[3:], lv[1], Lh)
    if act == R.ACT_RELU:
        ref = torch.relu(ref)
    ref.backward(gy)
    in_ptr, in_src, in_eid = csr_of(ei[1], ei[0], N)
    out_ptr, out_dst, out_eid = csr_of(ei[0], ei[1], N)
    l_in, l_out = l0[in_eid], l0[out_eid]
    Wcat = torch.cat(Ws)
    Y = x @ Wcat.t()
    Y0, B = Y[:, :D], Y[:, D:].clone()
    blk = lambda T, k: T[:, (k - 1) * D:k * D]                # noqa: E731  b_k's column block
    for k in range(K - 2, 0, -1):
        blk(B, k).copy_(R.step(in_ptr, in_src, l_in, blk(B, k + 1), 2.0, add=blk(B, k), sub=blk(B, k + 2) if k + 2 <= K - 1 else None))
    out = R.step(in_ptr, in_src, l_in, blk(B, 1), 1.0, add=Y0, sub=blk(B, 2) if K >= 3 else None, bias=bias, act=act)
    assert _rel(out, ref.detach()) <= 1e-11
    G_ = gy * (out > 0) if act == R.ACT_RELU else gy
    Us = [G_]
    A = [G_]
    for k in range(1, K):
        Uk = R.step(out_ptr, out_dst, l_out, Us[k - 1], 1.0 if k == 1 else 2.0, sub=None if k == 1 else Us[k - 2])
        Us.append(Uk)
        if k <= K - 2:
            A.append(2.0 * Uk)                               # Y2 = scale2 * Y
    Ucat = torch.cat(Us, dim=1)
    dW = Ucat.t() @ x
    dl, _ = G.sddmm(in_ptr, in_src, in_eid, torch.cat(A, dim=1), B)
    pairs = [("x", Ucat @ Wcat, lv[0].grad), ("bias", G_.sum(0), lv[1].grad), ("l", dl, lv[2].grad)]
    pairs += [(f"W{k}", dW[k * D:(k + 1) * D], lv[3 + k].grad) for k in range(K)]
    for name, got, want in pairs:
        assert _rel(got, want) <= 1e-11, name


@pytest.mark.parametrize("case", R.NORM_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("with_g2", [False, True])
def test_norm_references_equal_the_dense_restatement_and_its_autograd(case, with_g2):
    ei, N, n = case["ei"], case["N"], case["n"]
    for mode in R.WEIGHT_MODES:
        w = R.norm_weights(case, mode)
        w64 = (torch.ones(n, dtype=F64) if w is None else w.double()).requires_grad_(True)
        _, dis_ref, l_ref = C.laplacian(ei, w64, N)
        dis, l = R.norm_fwd(ei, w, N)
        assert _rel(dis, dis_ref.detach()) <= 1e-11 and _rel(l, l_ref.detach()) <= 1e-11
        g, g2 = R.norm_grads(case)
        gt = g.double() + g2.double() if with_g2 else g.double()
        (l_ref * gt).sum().backward()
        dw = R.norm_bwd(ei, w, g, g2 if with_g2 else None, dis, N)
        assert _rel(dw, w64.grad) <= 1e-11, mode
        assert bool((dw[ei[0] == ei[1]] == 0).all()) and bool((dw[dis[ei[0]] == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ fp32 inside the bound, faults outside
def _keep(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= R.P_DROP


def step_check(case, mut=None, combos=R.STEP_COMBOS):
    """Every combo of a case in fp32 (with `mut` planted) against fp64 and the bound -> (elements outside, worst share of ambiguous ones)."""
    gr = R.case_graph(case)
    x = R.step_inputs(case)
    bad, amb = 0, 0.0
    for combo in combos:
        X, add, sub, bias = R.combo_operands(case, combo, x)
        a = (gr["ptr"], gr["col"], gr["val"], X, combo["alpha"], add, sub, bias)
        Z = R.step_pre(*a)
        pb = R.step_pre_bound(*a)
        act = combo["act"]
        keep = _keep(Z.shape, 3) if act == R.ACT_RELU_DROPOUT else None
        Y = G.activate(Z, act, keep, R.P_DROP)
        Y32 = R.step(*a, act=act, keep=keep, p=R.P_DROP, dt=F32, mut=mut)
        assert Y32.dtype == F32
        bad += int(R.outside(Y32, Y, G.spmm_bound(pb, Y, act, R.P_DROP)).sum())
        if act == R.ACT_RELU_DROPOUT:
            amb = max(amb, float(G.ambiguous(Z, pb).double().mean()))
    return bad, amb


def norm_check(case, mode, mut=None):
    """The three normalisation references on one case in fp32 (with `mut` planted) against fp64 and the bounds -> elements outside."""
    ei, N = case["ei"], case["N"]
    w = R.norm_weights(case, mode)
    dis64, _ = R.norm_fwd(ei, w, N)
    dis32, l32 = R.norm_fwd(ei, w, N, dt=F32, mut=mut)
    assert dis32.dtype == F32 and l32.dtype == F32
    bad = int(R.outside(dis32, dis64, R.dis_bound(ei, N, dis64)).sum())
    lref = R.l_of_dis(ei, w, dis32)
    bad += int(R.outside(l32, lref, R.l_bound(lref)).sum())
    g, g2 = R.norm_grads(case)
    d32 = dis64.float()
    for second in (None, g2):
        ref, _, _, dwb = R.norm_bwd(ei, w, g, second, d32, N, bounds=True)
        got = R.norm_bwd(ei, w, g, second, d32, N, dt=F32, mut=mut)
        assert got.dtype == F32
        bad += int(R.outside(got, ref, dwb).sum())
    return bad


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: c["name"])
def test_step_in_fp32_is_inside_its_bound_and_dropout_cases_show_their_mask(case):
    bad, amb = step_check(case)
    assert bad == 0
    assert amb <= G.MAX_AMBIGUOUS                             # a condition on the reference alone


@pytest.mark.parametrize("case", R.NORM_CASES, ids=lambda c: c["name"])
def test_norm_in_fp32_is_inside_its_bounds(case):
    for mode in R.WEIGHT_MODES:
        assert norm_check(case, mode) == 0, mode


def test_every_planted_fault_leaves_the_bound_on_some_case():
    """One fault each, evaluated in fp32 like the unmutated references above; the cases named are where it must show."""
    by = {c["name"]: c for c in R.STEP_CASES}
    for name in ("lanes_v4_lpr16_D64", "lanes_v1_lpr64_D41", "rb_v4_nw4_N67_D64_at16N", "rb_v1_nw16_N67_D65"):
        for mut in ("drop_last", "past_end", "skip_last_col", "sub_added", "alpha_on_add", "bias_next"):
            assert step_check(by[name], mut)[0] > 0, (name, mut)
    # the faults that only some operand combinations can show, each on the combos that can
    pick = lambda f: [k for k in R.STEP_COMBOS if f(k)]          # noqa: E731
    c = by["lanes_v4_lpr16_D64"]
    assert step_check(c, "sub_added", pick(lambda k: k["sub"] is None))[0] == 0 < step_check(c, "sub_added", pick(lambda k: k["sub"] is not None))[0]
    assert step_check(c, "alpha_on_add", pick(lambda k: k["alpha"] == 1.0))[0] == 0 < step_check(c, "alpha_on_add", pick(lambda k: k["alpha"] == 2.0 and k["add"]))[0]
    assert step_check(c, "bias_next", pick(lambda k: not k["bias"]))[0] == 0 < step_check(c, "bias_next", pick(lambda k: k["bias"]))[0]
    assert step_check(by["all_rows_empty_but_one"], "past_end")[0] > 0 and step_check(by["one_row_long"], "drop_last")[0] > 0
    nb = {c["name"]: c for c in R.NORM_CASES}
    for name in ("small_directed", "long_rows"):
        for mode in R.WEIGHT_MODES:
            for mut in ("deg_by_dst", "count_self", "no_g2", "c_dst"):
                assert norm_check(nb[name], mode, mut) > 0, (name, mode, mut)
