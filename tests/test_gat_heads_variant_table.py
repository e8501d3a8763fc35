"""CPU: the case tables of tests/test_gpu_gat_heads_kernels.py (tests/gat_heads_ref.py) reach EVERY code sgs_gat_heads_variant can return
(asked of the built library, whose launchers decode that same code), straddle every dispatch threshold and state the right code; the fp64
references compose to the two existing GAT references (tests/gat_edge_ref.gat_edge_layer, test_gpu_gat_heads.dense_gat_heads), forward
and, through the hand-written backward chain, against autograd; and every planted single fault of the references, evaluated in fp32,
leaves the element-wise bound on at least one case of the table while the unmutated fp32 evaluation stays inside it on all of them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_heads_ref as R  # noqa: E402
import gcn_ref as G  # noqa: E402
from gat_edge_ref import gat_edge_layer  # noqa: E402
from test_gpu_gat_heads import dense_gat_heads  # noqa: E402

F32, F64 = R.F32, R.F64
SL = float(torch.tensor(R.SLOPE, dtype=F32))          # the slope the kernels get: a float argument


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd._lib.lib()


def _al(case):
    return 0 if case.get("align") or case.get("att_off") else 1


def table_codes():
    """op -> [(case name, stated code, (N, K, C, aligned16))]"""
    t = {op: [] for op in range(8)}
    for c in R.SCORES_FWD_CASES:
        t[R.OP_SCORES_FWD].append((c["name"], c["code"], (c["N"], c["K"], c["C"], _al(c))))
    for c in R.SCORES_BWD_CASES:
        t[R.OP_SCORES_BWD].append((c["name"], c["code"], (c["N"], c["K"], c["C"], 1)))
    for c in R.SPMM_CASES:
        t[R.SPMM_OP[c["mode"]]].append((c["name"], c["code"], (c["N"], c["K"], c["C"], _al(c))))
    for c in R.SDDMM_CASES:
        t[R.OP_SDDMM].append((c["name"], c["code"], (c["N"], c["K"], c["C"], _al(c))))
        t[R.OP_SDDMM_BROADCAST].append((c["name"], c["code_bcast"], (c["N"], c["K"], c["C"], _al(c))))
    for c in R.ROW_CASES:
        t[R.OP_ROW].append((c["name"], c["code"], (c["N"], c["K"], 1, 1)))
    return t


# ------------------------------------------------------------------------------------------------ coverage
def test_every_case_states_the_query_s_code(L):
    for op, rows in table_codes().items():
        assert len({n for n, _, _ in rows}) == len(rows), op
        for name, code, (N, K, C, al) in rows:
            assert L.sgs_gat_heads_variant(op, N, K, C, al) == code, (name, L.sgs_gat_heads_variant(op, N, K, C, al))


C_GRID = list(range(1, 18)) + [20, 31, 32, 33, 36, 60, 63, 64, 65, 68, 72, 100, 127, 128, 129, 132, 255, 256, 257, 260, 300, 512, 1024, 1028, 4096]


def test_tables_reach_every_code_of_the_supported_domain(L):
    """K = 1 .. 16, C on both sides of every power of two up to 64 VEC and of K C = 1024, N on both sides of 4096 and 65536, both
    alignments: the set of codes that comes back is exactly the set the tables state, per op."""
    want = {op: {code for _, code, _ in rows} for op, rows in table_codes().items()}
    for op in range(8):
        seen = set()
        for N in (1, 70, 4095, 4096, 65535, 65536, 1 << 20):
            for K in range(1, 17):
                for C in C_GRID:
                    for al in (0, 1):
                        seen.add(L.sgs_gat_heads_variant(op, N, K, C, al))
        assert seen == want[op], (op, sorted(seen ^ want[op]))
    for bad in ((R.OP_ROW, 5, 0, 1), (R.OP_ROW, 5, 17, 1), (R.OP_SDDMM, 5, 4, 0), (8, 5, 4, 4), (-1, 5, 4, 4), (R.OP_SCORES_BWD, -1, 4, 4)):
        assert L.sgs_gat_heads_variant(*bad, 1) == -1, bad


def _has(cases, **kw):
    return any(all(c.get(k) == v for k, v in kw.items()) for c in cases)


def test_every_threshold_is_straddled():
    sb, sf, sp, sd, rw = R.SCORES_BWD_CASES, R.SCORES_FWD_CASES, R.SPMM_CASES, R.SDDMM_CASES, R.ROW_CASES
    # rows per workgroup of the scores backward; 65 partial rows (the finish's four-way loop needs more than 64); D > 256
    for a, b in ((4095, 4096), (65535, 65536)):
        assert _has(sb, N=a) and _has(sb, N=b) and {c["rpw"] for c in sb if c["N"] in (a, b)} in ({16, 64}, {64, 256})
    assert _has(sb, N=1040, rpw=16) and any(c["K"] * c["C"] > 256 for c in sb)
    # VEC: every shape with C % 4 == 0 of the scores forward both ways; per SpMM mode and for the SDDMM a shape off alignment by X / A and by Y / B
    for c in sf:
        assert _has(sf, K=c["K"], C=c["C"], att_off=1 - c["att_off"])
    for mode in (R.CONCAT, R.MEAN, R.BROADCAST):
        for al in ("x", "y"):
            un = [c for c in sp if c["mode"] == mode and c["align"] == al]
            assert un and all(c["C"] % 4 == 0 and c["code"] // 100000 % 10 == 1 for c in un), (mode, al)
            assert any(_has(sp, mode=mode, K=c["K"], C=c["C"], align="", epi=False) for c in un)
    assert _has(sd, K=8, C=32, align="a") and _has(sd, K=8, C=32, align="") and _has(sd, align="b")
    # the head mean's switch at K C = 1024, from both sides and at both VEC; the walk at both VEC
    assert _has(sp, mode=R.MEAN, K=16, C=64, code=R.code(R.K_MEAN_LDS, 4, 6)) and _has(sp, mode=R.MEAN, K=16, C=64, code=R.code(R.K_MEAN_LDS, 1, 6))
    assert _has(sp, mode=R.MEAN, K=16, C=65, code=R.code(R.K_MEAN_WALK, 1, 6)) and _has(sp, mode=R.MEAN, K=16, C=68, code=R.code(R.K_MEAN_WALK, 4, 5))
    # column loops that wrap: 64 lanes exactly against more (SpMM), C / VEC above the lanes of a head (SDDMM), C / VEC above 64 (scores)
    for mode in (R.CONCAT, R.BROADCAST):
        assert _has(sp, mode=mode, K=8, C=32, align="") and _has(sp, mode=mode, K=16, C=20) and _has(sp, mode=mode, K=16, C=5)
    assert _has(sd, K=16, C=64, align="") and _has(sd, K=1, C=1024) and _has(sd, K=1, C=256) and _has(sd, K=16, C=7)
    assert _has(sf, K=2, C=300, att_off=0) and _has(sf, K=2, C=300, att_off=1) and _has(sf, K=2, C=64, att_off=1)
    # the per-row family: every K of the issue, so every KP with and without padding lanes; more than 256 workgroups once
    assert [c["K"] for c in rw if c["N"] == R.ROW_N] == [1, 2, 3, 4, 5, 7, 8, 9, 13, 16]
    assert _has(rw, N=1030) and -(-1030 * 64 // 256) == 258
    for mode in (R.CONCAT, R.BROADCAST):
        assert {(c["K"], c["C"]) for c in sp if c["mode"] == mode} >= {(1, 1), (2, 2), (3, 5), (5, 4), (8, 4), (8, 32), (16, 20)}
    assert {(c["K"], c["C"]) for c in sp if c["mode"] == R.MEAN} >= {(8, 5), (5, 4), (16, 64), (16, 65), (16, 68)}
    assert {(c["K"], c["C"]) for c in sd} >= {(16, 64), (3, 5), (1, 1024), (9, 4), (8, 32)}
    assert {(c["K"], c["C"]) for c in sf} >= {(3, 1), (16, 5), (8, 32), (2, 300)}
    assert all(c["N"] % 16 and c["N"] % 4 for c in sd)                      # dead rows take part in the SDDMM's shuffles
    assert sum(c["epi"] for c in sp) == 3 and {c["code"] // 1000000 for c in sp if c["epi"]} == {R.K_CONCAT, R.K_MEAN_LDS, R.K_MEAN_WALK}


def test_benchmark_shapes_keep_their_instantiations(L):
    """The flagship shapes, expected values derived by hand from the launchers as they stood before the query existed:
    (33869, 8, 32): scores VEC 4, lg = log2(32 / 4) = 3; backward 64 rows per workgroup (4096 <= N < 65536); SpMM 256 / 4 = 64 lanes, lg 6;
    the head mean's 4 rows x 256 floats fit the LDS form; SDDMM lgK = 3, lgG = min(log2 8, 6 - 3) = 3; KP = 8.
    (33869, 8, 5): VEC 1; scores lg = ceil log2 5 = 3; SpMM ceil log2 40 = 6; SDDMM lgG = min(3, 3) = 3.
    (1013, 4, 64): scores lg = log2 16 = 4; 16 rows per workgroup; SpMM 256 / 4 = 64 lanes; SDDMM lgK = 2, lgG = min(4, 4) = 4; KP = 4."""
    want = {(33869, 8, 32): [1430000, 2100064, 3460000, 4460000, 6460000, 7463000, 8463000, 9100008],
            (33869, 8, 5): [1130000, 2100064, 3160000, 4160000, 6160000, 7163000, 8163000, 9100008],
            (1013, 4, 64): [1440000, 2100016, 3460000, 4460000, 6460000, 7464000, 8464000, 9100004]}
    for (N, K, C), codes in want.items():
        assert [L.sgs_gat_heads_variant(op, N, K, C, 1) for op in range(8)] == codes, (N, K, C)


# ------------------------------------------------------------------------------------------------ the graphs are what the tables promise
@pytest.mark.parametrize("case", R.ROW_CASES, ids=lambda c: c["name"])
def test_row_graph_plants_its_edge_cases(case):
    N, K = case["N"], case["K"]
    gr = R.case_graph(case)
    x = R.row_inputs(gr)
    n, epw, h = gr["n"], 64 // R.kp_of(K), gr["hub_row"]
    ptr, src, eid = gr["ptr"].long(), gr["col"].long(), gr["eid"].long()
    ln = (ptr[1:] - ptr[:-1]).tolist()
    assert ln[:6] == [epw + 1, 0, 1, epw - 1, epw, 2 * epw + 1] and ln[h] == 300 and int(ptr[-1]) == n
    assert sorted(eid[:n].tolist()) == list(range(n)) and src.numel() == eid.numel() == n + G.PAD
    assert 0 <= int(src.min()) and int(src.max()) < N and int(eid.max()) < n
    r = G.rows_of(gr["ptr"])
    assert src[ptr[2]] == 2 and src[ptr[5]] == 5 and src[ptr[5] + 1] == src[ptr[5] + 2]          # only-(i, i) row, loop + duplicates
    assert bool(((src[:n] == r) & (r == h)).any())
    # pre-activation exactly 0 (entry and loops), in both forms
    e0 = gr["zero_eid"]
    k0 = int(ptr[0])
    assert eid[k0] == e0 and x["w"][e0] == 0 and 0.05 < float((x["w"] == 0).float().mean()) < 0.2
    pe = R.pre32(x["a_s"], x["a_d"], src[:n], r, x["w"][eid[:n]], x["coef"])
    assert bool((pe[k0] == 0).all()) and bool((R.pre32(x["a_s"], x["a_d"], src[:n], r)[k0] == 0).all())
    assert bool(((x["a_s"] + x["a_d"])[[1, 4]] == 0).all())
    # the hub row's spread: logits more than 104 below the maximum (expf gives 0) and some in the subnormal range
    f = R.alpha_fwd(x["a_s"], x["a_d"], gr["ptr"], gr["col"], gr["eid"], K)
    sh = f["soft"][eid[ptr[h]:ptr[h + 1]]]
    le = R.lrelu32(R.pre32(x["a_s"], x["a_d"], src[:n], r), R.SLOPE)[ptr[h]:ptr[h + 1]]
    assert float((le.max(0).values - le.min(0).values).min()) > 104
    assert bool((sh == 0).any()) and bool(((sh > 0) & (sh < 2.0 ** -126)).any())


def test_agg_graph_has_the_unroll_lengths_and_stays_in_bounds():
    gr = R.agg_graph(R.AGG_N, 5)
    ln = gr["lens"].tolist()
    n = gr["n"]
    assert ln[1:9] == R.SPMM_LENGTHS and ln[R.AGG_N // 2] == 300
    assert sorted(gr["eid"][:n].tolist()) == list(range(n)) and int(gr["col"].max()) < R.AGG_N and int(gr["col"].min()) >= 0
    r = G.rows_of(gr["ptr"])
    assert bool((gr["col"][:n].long() == r).any()) and gr["col"].numel() == n + G.PAD
    assert abs(float(R.spmm_heads_pre(gr["ptr"], gr["col"], gr["eid"], gr["val"].double(), None, None, torch.ones(R.AGG_N, 5, dtype=F64), 5, 1,
                                      R.CONCAT)[R.AGG_N // 2].mean()) - 1.0) < 0.1            # a row's weights sum to about 1


# ------------------------------------------------------------------------------------------------ reference self-checks
def _layer_graph(N, E, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[:, 1] = ei[0, 1]
    ei[:, 5] = ei[0, 5]
    ei[:, 7] = ei[:, 6]
    return ei, g


@pytest.mark.parametrize("N,E,K,C,concat,edge,p", [(30, 200, 3, 5, True, False, 0.0), (41, 500, 8, 4, False, False, 0.3), (30, 260, 5, 4, True, True, 0.3),
                                                   (25, 150, 16, 3, False, True, 0.0), (12, 40, 1, 7, True, True, 0.0)])
def test_references_chain_to_the_existing_gat_references(N, E, K, C, concat, edge, p):
    """scores -> alpha -> SpMM forward, and SpMM^T / SDDMM -> alpha backward -> edge sum -> scores backward, all from gat_heads_ref in fp64,
    against dense_gat_heads (no edge term) or gat_edge_layer (edge term) and torch autograd through them."""
    ei, g = _layer_graph(N, E, 3 * N + K)
    Fin = 6
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)          # noqa: E731
    x, W, a_s, a_d, b = rn(N, Fin), rn(K * C, Fin), rn(K, C), rn(K, C), rn(K * C if concat else C)
    w, lin_e, att_e = torch.rand(E, generator=g, dtype=F64) + 0.1, rn(K * C, 1), rn(K, C)
    keep_e = keep_l = None
    if p > 0:
        keep_e, keep_l = torch.rand(E, K, generator=g) >= p, torch.rand(N, K, generator=g) >= p
    gy = rn(N, K * C if concat else C)
    leaves = [t.clone().requires_grad_(True) for t in (x, W, a_s, a_d, b, w, lin_e, att_e)]
    if edge:
        y = gat_edge_layer(leaves[0], ei, leaves[5], *leaves[1:5], leaves[6], leaves[7], K, C, concat, slope=SL, keep_e=keep_e, keep_l=keep_l, p=p)
    else:
        y = dense_gat_heads(leaves[0], ei, *leaves[1:5], K, C, concat, slope=SL, keep_e=keep_e, keep_l=keep_l, p=p)
    y.backward(gy)
    # forward chain
    in_ptr, in_src, in_eid = R.csr_of(ei[1], ei[0], N)
    out_ptr, out_dst, out_eid = R.csr_of(ei[0], ei[1], N)
    mode = R.CONCAT if concat else R.MEAN
    xl = x @ W.t()
    s, d = R.scores_fwd(xl, a_s, a_d, K, C)
    coef = (lin_e.view(K, C) * att_e).sum(-1) if edge else None
    soft, soft_loop = R.alpha_smooth(s, d, in_ptr, in_src, in_eid, SL, w if edge else None, coef)
    sc = 1.0 / (1.0 - p)
    alpha = soft if keep_e is None else soft * keep_e * sc
    aloop = soft_loop if keep_l is None else soft_loop * keep_l * sc
    out = R.spmm_heads_pre(in_ptr, in_src, in_eid, alpha, aloop, b, xl, K, C, mode)
    tol = lambda r: 1e-11 * (1.0 + float(r.detach().abs().max()))              # noqa: E731
    assert float((out - y.detach()).abs().max()) <= tol(y)
    # backward chain
    dxl_agg = R.spmm_heads_pre(out_ptr, out_dst, out_eid, alpha, aloop, None, gy, K, C, R.CONCAT if concat else R.BROADCAST)
    galpha, gloop = R.sddmm_heads(in_ptr, in_src, in_eid, gy, xl, K, C, not concat)
    nl = ei[0] != ei[1]
    cnt = torch.zeros(N, dtype=F64).index_add_(0, ei[1][nl], torch.ones(int(nl.sum()), dtype=F64))
    kw = {}
    if edge:
        wb = torch.zeros(N, dtype=F64).index_add_(0, ei[1][nl], w[nl]) / cnt.clamp(min=1.0)
        kw = dict(edge_w=w, coef=coef, loop_w=wb, loop_inv_cnt=torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0), torch.zeros_like(cnt)))
    # the scores go in as fp32 (the branch is decided on their fp32 sum; no fp64 value here is within 1e-6 of a sign change).  Under dropout
    # g' = fp32(galpha drop_scale) as in the kernels, so the gradients are compared at fp32 resolution there
    if p > 0:
        galpha, gloop = galpha.float(), gloop.float()
        tol = lambda r: 1e-6 * (1.0 + float(r.detach().abs().max()))           # noqa: E731
    bw = R.alpha_bwd(s.float(), d.float(), in_ptr, in_src, in_eid, K, soft, soft_loop, galpha, gloop, R.SLOPE, keep_e, keep_l, p, **kw)
    d_a_src = R.edge_sum_by_row(bw["g_edge"], bw["g_selfloop"], out_ptr, out_eid)
    dxl, das, dad = R.scores_bwd(xl, a_s, a_d, d_a_src, bw["d_a_dst"], K, C, dxl0=dxl_agg)
    for name, got, ref in (("x", dxl @ W, leaves[0].grad), ("W", dxl.t() @ x, leaves[1].grad), ("att_src", das.view(K, C), leaves[2].grad),
                           ("att_dst", dad.view(K, C), leaves[3].grad)):
        assert float((got - ref).abs().max()) <= tol(ref), name
    if edge:
        dw_ref = leaves[5].grad
        assert float((bw["d_edge_w"] - dw_ref).abs().max()) <= tol(dw_ref) and bool((bw["d_edge_w"][~nl] == 0).all())
        dc = bw["d_edge_coef"]
        assert float(((dc[:, None] * att_e).reshape(-1, 1) - leaves[6].grad).abs().max()) <= tol(leaves[6].grad)
        assert float((dc[:, None] * lin_e.view(K, C) - leaves[7].grad).abs().max()) <= tol(leaves[7].grad)


@pytest.mark.parametrize("case", [R.ROW_CASES[2], R.ROW_CASES[6]], ids=lambda c: c["name"])
@pytest.mark.parametrize("edge", [False, True])
def test_softmax_on_fp32_arguments_is_the_smooth_softmax_and_its_backward_is_autograd_s(case, edge):
    """On the planted graph (exact zeros, underflowing rows, (i, i) entries): alpha_fwd (expf arguments formed in fp32) against the plain
    fp64 softmax, and alpha_bwd on the latter's soft against autograd through it -- d a_dst, d a_src (via edge_sum_by_row), d w, d c."""
    K = case["K"]
    gr = R.case_graph(case)
    x = R.row_inputs(gr)
    ptr, src, eid, n, N = gr["ptr"], gr["col"], gr["eid"], gr["n"], gr["N"]
    lv = {k: x[k].double().requires_grad_(True) for k in ("a_s", "a_d", "w", "coef")}
    ekw = dict(edge_w=lv["w"], coef=lv["coef"]) if edge else {}
    soft, soft_loop = R.alpha_smooth(lv["a_s"], lv["a_d"], ptr, src, eid, SL, **ekw)
    f = R.alpha_fwd(x["a_s"], x["a_d"], ptr, src, eid, K, edge_w=x["w"] if edge else None, coef=x["coef"] if edge else None)
    for a, b in ((f["soft"], soft.detach()), (f["soft_loop"], soft_loop.detach())):
        assert bool(((a - b).abs() <= 1e-4 * b + 1e-300).all())
    (soft * x["galpha"].double()).sum().add((soft_loop * x["gloop"].double()).sum()).backward()
    kw = dict(edge_w=x["w"], coef=x["coef"], loop_w=f["loop_w"], loop_inv_cnt=f["loop_inv_cnt"]) if edge else {}
    bw = R.alpha_bwd(x["a_s"], x["a_d"], ptr, src, eid, K, soft.detach(), soft_loop.detach(), x["galpha"], x["gloop"], **kw)
    tol = lambda r: 1e-11 * (1.0 + float(r.detach().abs().max()))              # noqa: E731
    assert float((bw["d_a_dst"] - lv["a_d"].grad).abs().max()) <= tol(lv["a_d"].grad)
    out_ptr, _, out_eid = R.csr_of(src[:n].long(), G.rows_of(ptr), N)
    order = torch.argsort(src[:n].long(), stable=True)
    d_a_src = R.edge_sum_by_row(bw["g_edge"], bw["g_selfloop"], out_ptr, eid[:n].long()[order])
    assert float((d_a_src - lv["a_s"].grad).abs().max()) <= tol(lv["a_s"].grad)
    if edge:
        assert float((bw["d_edge_w"] - lv["w"].grad).abs().max()) <= tol(lv["w"].grad)
        assert float((bw["d_edge_coef"] - lv["coef"].grad).abs().max()) <= tol(lv["coef"].grad)


# ------------------------------------------------------------------------------------------------ fp32 inside the bound, faults outside
def _keep(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= R.P_DROP


def row_check(case, mut=None, drop=False, by_pos=False):
    """The per-row family on one case in fp32 (with `mut` planted) against fp64 and the bounds: -> number of elements outside."""
    K = case["K"]
    gr = R.case_graph(case)
    x = R.row_inputs(gr)
    ptr, src, eid, n, N = gr["ptr"], gr["col"], gr["eid"], gr["n"], gr["N"]
    keep_e, keep_l = (_keep((n, K), 1), _keep((N, K), 2)) if drop else (None, None)
    p = R.P_DROP if drop else 0.0
    bad = 0
    for edge in (False, True):
        ekw = dict(edge_w=x["w"], coef=x["coef"]) if edge else {}
        ref = R.alpha_fwd(x["a_s"], x["a_d"], ptr, src, eid, K, **ekw)
        got = R.alpha_fwd(x["a_s"], x["a_d"], ptr, src, eid, K, dt=F32, mut=mut, **ekw)
        assert got["soft"].dtype == F32
        bs, bl = R.soft_bound(ref, ptr, src, eid)
        bad += int(R.outside(got["soft"], ref["soft"], bs).sum()) + int(R.outside(got["soft_loop"], ref["soft_loop"], bl).sum())
        if edge:
            bad += int(R.outside(got["loop_w"].float(), ref["loop_w"], ref["loop_w_bound"]).sum())
            bad += int(R.outside(got["loop_inv_cnt"].float(), ref["loop_inv_cnt"], ref["loop_inv_cnt_bound"]).sum())
        s32, l32 = ref["soft"].float(), ref["soft_loop"].float()
        if drop:          # alpha is exact given soft and the mask
            bad += int((R.alpha_of(s32, keep_e, p, eid if by_pos else None) != R.alpha_of(s32, keep_e, p)).sum())
        bkw = dict(ekw, loop_w=ref["loop_w"].float(), loop_inv_cnt=ref["loop_inv_cnt"].float(), dw_add=x["dw_add"] if drop else None) if edge else {}
        args = (x["a_s"], x["a_d"], ptr, src, eid, K, s32, l32, x["galpha"], x["gloop"], R.SLOPE, keep_e, keep_l, p)
        bref = R.alpha_bwd(*args, bounds=True, **bkw)
        bgot = R.alpha_bwd(*args, dt=F32, mut=mut, keep_by_pos=by_pos, **bkw)
        for k in bgot:
            assert bgot[k].dtype == F32
            bad += int(R.outside(bgot[k], bref[k], bref[k + "_bound"]).sum())
        for gs in (None, x["g_self"]):
            eref, eb = R.edge_sum_by_row(x["galpha"], gs, ptr, eid), R.edge_sum_by_row_bound(x["galpha"], gs, ptr, eid)
            bad += int(R.outside(R.edge_sum_by_row(x["galpha"], gs, ptr, eid, dt=F32, mut=mut), eref, eb).sum())
    return bad


def scores_check(case, mut=None):
    N, K, C = case["N"], case["K"], case["C"]
    xl, a_s, a_d, g_s, g_d, dx0 = (R.scores_inputs(case)[k] for k in ("xl", "att_s", "att_d", "g_s", "g_d", "dxl0"))
    bad = 0
    for ref, got, bd in zip(R.scores_fwd(xl, a_s, a_d, K, C), R.scores_fwd(xl, a_s, a_d, K, C, dt=F32), R.scores_fwd_bound(xl, a_s, a_d, K, C)):
        bad += int(R.outside(got, ref, bd).sum())
    for acc in (None, dx0):
        ref, bd = R.scores_bwd(xl, a_s, a_d, g_s, g_d, K, C, acc), R.scores_bwd_bound(xl, a_s, a_d, g_s, g_d, K, C, acc, case.get("rpw", 16))
        got = R.scores_bwd(xl, a_s, a_d, g_s, g_d, K, C, acc, dt=F32, mut=mut, rows_per_wg=case.get("rpw", 16))
        bad += sum(int(R.outside(a, b, c).sum()) for a, b, c in zip(got, ref, bd))
    return bad


def spmm_check(case, mut=None):
    K, C, N, mode = case["K"], case["C"], case["N"], case["mode"]
    gr = R.case_graph(case)
    walk = case["code"] // 1000000 == R.K_MEAN_WALK
    bad = 0
    for diag_on, bias_on, act in (R.SPMM_EPI_COMBOS if case["epi"] else R.SPMM_COMBOS):
        drop = act == G.ACT_RELU_DROPOUT
        X, bias = R.spmm_x(case, drop)
        diag, bias = (gr["diag"] if diag_on else None), (bias if bias_on else None)
        a = (gr["ptr"], gr["col"], gr["eid"])
        Z = R.spmm_heads_pre(*a, gr["val"], diag, bias, X.double(), K, C, mode)
        pb = R.spmm_heads_pre_bound(*a, gr["val"], diag, bias, X, K, C, mode, walk)
        keep = _keep(Z.shape, 3) if drop else None
        Y = G.activate(Z, act, keep, R.P_DROP)
        Y32 = G.activate(R.spmm_heads_pre(*a, gr["val"], diag, bias, X, K, C, mode, mut=mut), act, keep, R.P_DROP)
        assert Y32.dtype == F32
        bad += int(R.outside(Y32, Y, G.spmm_bound(pb, Y, act, R.P_DROP)).sum())
        if drop:          # a condition on the reference alone: the share of elements that hide their kept bit
            assert float(G.ambiguous(Z, pb).double().mean()) <= G.MAX_AMBIGUOUS
    return bad


def sddmm_check(case):
    K, C, N = case["K"], case["C"], case["N"]
    gr = R.case_graph(case)
    a = (gr["ptr"], gr["col"], gr["eid"])
    bad = 0
    for bc in (False, True):
        A, B = R.sddmm_ab(case, bc)
        ref, got, bd = R.sddmm_heads(*a, A.double(), B.double(), K, C, bc), R.sddmm_heads(*a, A, B, K, C, bc), R.sddmm_heads_bound(*a, A, B, K, C, bc)
        bad += sum(int(R.outside(x, y, z).sum()) for x, y, z in zip(got, ref, bd))
    return bad


@pytest.mark.parametrize("case", R.ROW_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("drop", [False, True])
def test_row_family_in_fp32_is_inside_its_bounds(case, drop):
    assert row_check(case, drop=drop) == 0


@pytest.mark.parametrize("case", R.SCORES_FWD_CASES[::2] + R.SCORES_BWD_CASES, ids=lambda c: c["name"])
def test_scores_in_fp32_are_inside_their_bounds(case):
    assert scores_check(case) == 0


@pytest.mark.parametrize("case", R.SPMM_CASES, ids=lambda c: c["name"])
def test_spmm_heads_in_fp32_is_inside_its_bound_and_dropout_cases_show_their_mask(case):
    assert spmm_check(case) == 0


@pytest.mark.parametrize("case", R.SDDMM_CASES, ids=lambda c: c["name"])
def test_sddmm_heads_in_fp32_is_inside_its_bound(case):
    assert sddmm_check(case) == 0


def test_every_planted_fault_leaves_the_bound_on_some_case():
    """One fault each, evaluated in fp32 like the unmutated references above; the cases named are where it must show."""
    by = {c["name"]: c for c in R.ROW_CASES + R.SCORES_BWD_CASES + R.SPMM_CASES}
    padded = [c for c in R.ROW_CASES if R.kp_of(c["K"]) != c["K"]]
    assert len(padded) == 6
    for c in padded:                                      # a padding lane's head 0 stored as head K - 1: every K that has padding lanes
        assert row_check(c, mut="pad_alias") > 0, c["name"]
    assert all(row_check(c, mut="pad_alias") == 0 for c in R.ROW_CASES if R.kp_of(c["K"]) == c["K"])
    for c in R.ROW_CASES:
        assert row_check(c, mut="max_no_loop") > 0, c["name"]                    # node N - 1's loop logit overflows expf: NaN
        assert row_check(c, mut="count_self") > 0, c["name"]                     # softmax rows with (i, i) entries, and wbar's count
        assert row_check(c, drop=True, by_pos=True) > 0, c["name"]               # the mask of entry k read at row k, not at eid[k]
        assert row_check(c, mut="slope_side") > 0, c["name"]                     # the planted pre-activations of exactly 0
    # d edge_coef without one workgroup's partial row: the 65th of 258 (the last workgroup of N = 70 holds nodes N - 2, N - 1, whose loops
    # take all of their softmax and leave no gradient to lose)
    assert row_check(by["row_K5_N1030"], mut="drop_partial") > 0
    for c in R.SCORES_BWD_CASES:
        assert scores_check(c, mut="drop_partial") > 0, c["name"]                # d att without one workgroup's partial row
    for mode in (R.MEAN, R.BROADCAST):                                            # 1 / KP for 1 / K wherever K is no power of two
        hit = [c for c in R.SPMM_CASES if c["mode"] == mode and R.kp_of(c["K"]) != c["K"]]
        assert len(hit) >= 3 and all(spmm_check(c, mut="mean_div_kp") > 0 for c in hit)
    for c in R.SPMM_CASES:                                                        # rows of length 1, 3, 5, 7, 9 lose their tail
        assert spmm_check(c, mut="skip_tail") > 0, c["name"]
