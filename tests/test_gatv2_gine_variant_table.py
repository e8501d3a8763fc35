"""CPU: the case tables of tests/test_gpu_gatv2_gine_kernels.py (tests/gatv2_kernels_ref.py, tests/gine_kernels_ref.py) reach EVERY code
sgs_gatv2_variant and sgs_gine_variant can return (asked of the built library, whose launchers decode those same codes), state the right
code per case, straddle every dispatch threshold, and fit the workspace queries; the kernel-level fp64 references compose to the two
existing layer references (tests/gatv2_ref.gatv2_layer, tests/gine_ref.gine_aggregate), forward and, through the hand-written backward
chain, against autograd; and every planted single fault of the references, evaluated in fp32, leaves the element-wise bound on at least
one case of the tables while the unmutated fp32 evaluation stays inside it on all of them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_heads_ref as H  # noqa: E402
import gatv2_kernels_ref as V  # noqa: E402
import gine_kernels_ref as E  # noqa: E402
from gatv2_ref import gatv2_layer  # noqa: E402
from gine_ref import gine_aggregate  # noqa: E402

F32, F64 = V.F32, V.F64
SL = float(torch.tensor(V.SLOPE, dtype=F32))          # the slope the kernels get: a float argument


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd._lib.lib()


# ------------------------------------------------------------------------------------------------ coverage
def test_every_case_states_the_query_s_code(L):
    assert len({c["name"] for c in V.ALL_CASES}) == len(V.ALL_CASES) and len({c["name"] for c in E.ALL_CASES}) == len(E.ALL_CASES)
    for c in V.ALL_CASES:
        for edge in (False, True):
            got = [L.sgs_gatv2_variant(op, c["N"], c["K"], c["C"], V.case_aligned(c, op, edge)) for op in range(3)]
            assert got == V.case_codes(c, edge), (c["name"], edge, got)
            # the restated geometry (what the references' chain lengths and faults use) is the code's
            g = V.geom(c["N"], c["K"], c["C"], got[1] // 100000 % 10)
            assert V.code(2, g["vec"], g["lg"], g["lgG"], g["one"], g["iters"]) == got[1] and V.geom_of_code(got[1], c["N"]) == g
    for c in E.ALL_CASES:
        for bw in (False, True):
            got = L.sgs_gine_variant(c["N"], c["D"], c["nnz"], E.case_align(c, bw))
            assert got == E.case_code(c, bw) == E.variant(c["N"], c["D"], c["nnz"], E.case_align(c, bw)), (c["name"], bw, got)


C_GRID = list(range(1, 18)) + [20, 31, 32, 33, 36, 60, 63, 64, 65, 68, 72, 100, 127, 128, 129, 132, 255, 256, 257, 260, 300, 512, 1024, 1028]


def test_tables_reach_every_code_of_the_supported_domain(L):
    """K = 1 .. 16, C on both sides of every power of two up to 64 VEC, both alignments, at one row pass per workgroup: the set of codes that
    comes back is exactly the set the small cases state -- 60 per by-destination entry point, 14 for dxl; the large cases add iters 2, 16."""
    want = {op: set() for op in range(3)}
    for c in V.SMALL_CASES:
        for edge in (False, True):
            for op, code in enumerate(V.case_codes(c, edge)):
                want[op].add(code)
    for op in range(3):
        seen = {L.sgs_gatv2_variant(op, N, K, C, al) for N in (1, 67, 4000) for K in range(1, 17) for C in C_GRID for al in (0, 1)}
        assert seen == want[op], (op, sorted(seen ^ want[op]))
        assert len(seen) == (14 if op == V.OP_DXL else 60)
    assert {c["code_bwd"] % 100 for c in V.ITERS_CASES} == {2, 16}
    assert {c["code_bwd"] // 100 % 10000 for c in V.ITERS_CASES} == {1621, 1620, 4621}           # VEC 1 ONE, VEC 1 !ONE, VEC 4 ONE
    for bad in ((0, 5, 0, 1), (1, 5, 17, 1), (2, 5, 4, 0), (3, 5, 4, 4), (-1, 5, 4, 4), (1, -1, 4, 4)):
        assert L.sgs_gatv2_variant(*bad, 1) == -1, bad
    gine = {L.sgs_gine_variant(N, D, nnz, al) for N in (1, 67, 65536, 65537) for D in C_GRID for nnz in (0, 15 * N, 16 * N, 256 * N) for al in (4, 8, 16)}
    for bw in (False, True):
        assert {E.case_code(c, bw) for c in E.ALL_CASES} == gine
    assert len(gine) == 9


def test_every_threshold_is_straddled(L):
    q = L.sgs_gatv2_variant
    for K in range(1, 17):                                   # ONE -> !ONE at C = VEC << lgG and one channel group above, per head-slot count
        lgK = V.log2_ceil(K)
        for vec in (1, 4):
            C0 = vec << (6 - lgK)
            for op in (0, 1):
                it = op
                al = int(vec == 4)
                assert q(op, 67, K, C0, al) == V.code(op + 1, vec, 6, 6 - lgK, 1, it) and q(op, 67, K, C0 + vec, al) == V.code(op + 1, vec, 6, 6 - lgK, 0, it)
        assert q(0, 67, K, 1, 1) // 10000 % 10 == lgK        # K at each power of two and one above: the head slots KP
    assert [V.log2_ceil(K) for K in (1, 2, 3, 4, 5, 8, 9, 16)] == [0, 1, 2, 2, 3, 3, 4, 4]
    # row passes per workgroup: K = 16, C = 3 has 4 rows per pass
    for passes, iters in ((4095, 1), (4096, 2), (6143, 2), (6144, 3), (32767, 15), (32768, 16), (40000, 16)):
        assert q(1, 4 * passes, 16, 3, 1) == V.code(2, 1, 6, 2, 1, iters), passes
        assert q(1, 4 * passes - 3, 16, 3, 1) == V.code(2, 1, 6, 2, 1, iters), passes
        assert q(0, 4 * passes, 16, 3, 1) == V.code(1, 1, 6, 2, 1)
    g = L.sgs_gine_variant
    for N in (67, 2100):
        assert [g(N, 256, nnz, 16) for nnz in (16 * N - 1, 16 * N, 256 * N - 1, 256 * N)] == [464, 1404, 1404, 1416]
    assert g(65536, 256, 16 * 65536, 16) == 1404 and g(65537, 256, 16 * 65537, 16) == 464
    for vec, m in ((4, 4), (2, 2)):                          # the halving rule at D = 32 VEC and one column group above
        assert g(67, 32 * vec, 0, 16) == (vec // 2) * 100 + 64 and g(67, 32 * vec + m, 0, 16) == (vec if (32 * vec + m) % vec == 0 else 1) * 100 + 64
    assert [g(67, 128, 0, 16), g(67, 132, 0, 16), g(67, 64, 0, 16), g(67, 66, 0, 16), g(67, 32, 0, 16), g(67, 33, 0, 16)] == [264, 464, 164, 264, 164, 164]
    for D, row in ((132, {4: 164, 8: 264, 16: 464}), (130, {4: 164, 8: 264, 16: 264}), (133, {4: 164, 8: 164, 16: 164})):
        assert {al: g(67, D, 0, al) for al in (4, 8, 16)} == row, D
    # the tables straddle what needs a launch to be seen
    names = {c["name"] for c in E.ALL_CASES}
    assert {"wave_N8200_D33", "block4_N2100_D70", "block16_N520_D5"} <= names
    assert E.bwd_geom(8200, 164)["rows_per_block"] == 8 and E.bwd_geom(8192, 164)["rows_per_block"] == 4
    assert E.bwd_geom(2100, 1204)["nparts"] == 2048 and E.bwd_geom(520, 1116)["nparts"] == 512 and E.bwd_geom(520, 1104)["nparts"] == 520
    assert all(c["N"] % 4 for c in V.SMALL_CASES if c["kind"] == "std")


def test_workspace_queries_cover_every_case(L):
    for c in V.ALL_CASES:
        N, K, C = c["N"], c["K"], c["C"]
        have = L.sgs_gatv2_alpha_heads_bwd_workspace_bytes(N, K, C)
        for al in (0, 1):
            nwg = V.geom_of_code(L.sgs_gatv2_variant(1, N, K, C, al), N)["nwg"]
            assert have >= nwg * 2 * K * C * 4, c["name"]
    assert V.geom_of_code(L.sgs_gatv2_variant(1, 131077, 16, 3, 1), 131077)["nwg"] == 2049
    shapes = [(c["N"], c["D"], E.case_code(c, True)) for c in E.ALL_CASES]
    shapes += [(2049, 8, 1204), (2049, 8, 1404), (513, 8, 1216), (513, 5, 1116), (8193, 33, 164), (70000, 8, 264), (1 << 20, 4, 164)]
    for N, D, var in shapes:
        assert L.sgs_gine_aggregate_bwd_workspace_bytes(N, D) >= E.bwd_geom(N, var)["nparts"] * 2 * D * 4, (N, D, var)
    assert E.bwd_geom(2049, 1204)["nparts"] == 2048 and E.bwd_geom(513, 1216)["nparts"] == 512 and E.bwd_geom(8193, 164)["nparts"] == 1025


def test_product_shapes_keep_their_instantiations(L):
    """The shapes tools/gat_v2_probe.py and tools/gin_edge_probe.py run (both layers, K in {1, 8}), derived by hand from the launchers:
    GATv2 at N = 33 869, hidden 256, 5 classes: (K, C) = (1, 256): VEC 4, 64 lanes per head, ONE, 4 rows per pass -> 8 468 passes, iters 4;
    (8, 32): 8 lanes per head, ONE, iters 4; (1, 5): VEC 1, 8 lanes per row, 32 rows per pass -> 1 059 passes, iters 1; (8, 5): 64 lanes,
    iters 4.  GINE: s3 = (1 013, 602 | 256, 70 200 entries >= 16 N): 4 waves per row, VEC 2 (602 % 4 != 0) | 4; s4 = (33 869, 128 | 256,
    100 000 < 16 N): one wave per row, VEC 2 (128 <= 32 * 4: halved) | 4."""
    want = {(1, 256): [1466100, 2466104, 3460000], (8, 32): [1463100, 2463104, 3460000], (1, 5): [1133100, 2133101, 3130000],
            (8, 5): [1163100, 2163104, 3160000]}
    for (K, C), codes in want.items():
        assert [L.sgs_gatv2_variant(op, 33869, K, C, 1) for op in range(3)] == codes, (K, C)
    assert [L.sgs_gine_variant(1013, 602, 70200, 16), L.sgs_gine_variant(1013, 256, 70200, 16)] == [1204, 1404]
    assert [L.sgs_gine_variant(33869, 128, 100000, 16), L.sgs_gine_variant(33869, 256, 100000, 16)] == [264, 464]


# ------------------------------------------------------------------------------------------------ the graphs are what the tables promise
def test_graphs_plant_their_edge_cases():
    gr = V.graph(V.V2_N)
    N, n, h = gr["N"], gr["n"], gr["hub_row"]
    ptr, src, eid = gr["ptr"].long(), gr["col"].long(), gr["eid"].long()
    ln = (ptr[1:] - ptr[:-1]).tolist()
    assert ln[:3] == [0, 1, 5] and ln[h] == V.HUB and sorted(eid[:n].tolist()) == list(range(n)) and src.numel() == n + V.G.PAD
    assert src[ptr[1]] == 1 and src[ptr[2]] == 2 and src[ptr[2] + 1] == src[ptr[2] + 2] and bool((src[ptr[h]:ptr[h + 1]] == h).any())
    assert int((src[:n] == N - 3).sum()) >= 100 and int((src[:n] == N - 1).sum()) == 1 and int(src.max()) < N and int(src.min()) >= 0
    x = V.inputs(gr, 5, 5, "spread")
    assert 0.05 < float((x["w"] == 0).float().mean()) < 0.2
    for edge in (False, True):           # the hub row: some soft subnormal, some 0 (logits more than 104 below the maximum)
        f = V.alpha_fwd(x["xl"], x["xr"], x["att"], gr["ptr"], gr["col"], gr["eid"], 5, 5, edge_w=x["w"] if edge else None, lin_edge=x["le"])
        sh = f["soft"][eid[ptr[h]:ptr[h + 1]]]
        assert bool((sh == 0).any()) and bool(((sh > 0) & (sh < 2.0 ** -126)).any()), edge
    x = V.inputs(gr, 2, 3, "equal")
    f = V.alpha_fwd(x["xl"], x["xr"], x["att"], gr["ptr"], gr["col"], gr["eid"], 2, 3)
    assert float((f["soft_loop"] * (f["n_live"] + 1)[:, None] - 1).abs().max()) < 1e-12
    for nw, case in ((1, E.CASES[0]), (4, E.CASES[8]), (16, E.CASES[-1])):
        g = E.case_graph(case)
        assert case["nw"] == nw and g["lens"].tolist()[:len(E.SPECIAL[nw])] == E.SPECIAL[nw] and int(g["lens"].sum()) == case["nnz"]
        assert {4 * nw - 1, 4 * nw + 1} <= set(g["lens"].tolist()) and int(g["lens"].max()) == case["hub"]
        x = E.inputs(case, g)
        j, k, e0 = x["zero"]
        p = E.pre(x["x"], x["w"][g["eid"][:case["nnz"]].long()], x["a"], x["b"], V.G.rows_of(g["ptr"]))
        assert p[k, 0] == 0 and int((p == 0).sum()) == 1
        if case["D"] > 1:
            assert bool((E.pre(x["x"], None, x["a"], x["b"], V.G.rows_of(g["ptr"]))[k:k + 3, -1] == 0).all())


# ------------------------------------------------------------------------------------------------ reference self-checks
@pytest.mark.parametrize("N,E_,K,C,concat,edge,p", [(30, 200, 3, 5, True, False, 0.0), (41, 500, 8, 4, False, False, 0.3), (30, 260, 5, 4, True, True, 0.3),
                                                    (25, 150, 16, 3, False, True, 0.0), (12, 40, 1, 7, True, True, 0.0)])
def test_gatv2_references_chain_to_the_layer_reference(N, E_, K, C, concat, edge, p):
    """alpha_fwd -> SpMM forward, and SpMM^T / SDDMM -> alpha_bwd -> dxl, all in fp64, against gatv2_layer and torch autograd through it."""
    g = torch.Generator().manual_seed(3 * N + K)
    ei = torch.randint(0, N, (2, E_), generator=g)
    ei[:, 1] = ei[0, 1]
    ei[:, 7] = ei[:, 6]
    Fin = 6
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)          # noqa: E731
    x, Wl, bl, Wr, br, att, b = rn(N, Fin), rn(K * C, Fin), rn(K * C), rn(K * C, Fin), rn(K * C), rn(K, C), rn(K * C if concat else C)
    w, lin_e = torch.rand(E_, generator=g, dtype=F64) + 0.1, rn(K * C, 1)
    keep_e = keep_l = None
    if p > 0:
        keep_e, keep_l = torch.rand(E_, K, generator=g) >= p, torch.rand(N, K, generator=g) >= p
    gy = rn(N, K * C if concat else C)
    lv = [t.clone().requires_grad_(True) for t in (x, Wl, bl, Wr, br, att, w, lin_e)]
    y = gatv2_layer(lv[0], ei, lv[6] if edge else None, lv[1], lv[2], lv[3], lv[4], lv[5], b, lv[7], K, C, concat, slope=SL, keep_e=keep_e, keep_l=keep_l, p=p)
    y.backward(gy)
    in_ptr, in_src, in_eid = V.csr_of(ei[1], ei[0], N)
    out_ptr, out_dst, out_eid = V.csr_of(ei[0], ei[1], N)
    xl, xr = x @ Wl.t() + bl, x @ Wr.t() + br
    ekw = dict(edge_w=w, lin_edge=lin_e.view(K, C)) if edge else {}
    f = V.alpha_fwd(xl, xr, att, in_ptr, in_src, in_eid, K, C, SL, **ekw)
    sc = 1.0 / (1.0 - p)
    alpha = f["soft"] if keep_e is None else f["soft"] * keep_e * sc
    aloop = f["soft_loop"] if keep_l is None else f["soft_loop"] * keep_l * sc
    mode = H.CONCAT if concat else H.MEAN
    out = H.spmm_heads_pre(in_ptr, in_src, in_eid, alpha, aloop, b, xl, K, C, mode)
    tol = lambda r: 1e-10 * (1.0 + float(r.detach().abs().max()))              # noqa: E731
    assert float((out - y.detach()).abs().max()) <= tol(y)
    dxl_agg = H.spmm_heads_pre(out_ptr, out_dst, out_eid, alpha, aloop, None, gy, K, C, H.CONCAT if concat else H.BROADCAST)
    galpha, gloop = H.sddmm_heads(in_ptr, in_src, in_eid, gy, xl, K, C, not concat)
    bkw = dict(ekw, loop_w=f["loop_w"], loop_inv_cnt=f["loop_inv_cnt"]) if edge else {}
    bw = V.alpha_bwd(xl, xr, att, in_ptr, in_src, in_eid, K, C, f["soft"], f["soft_loop"], galpha, gloop, SL, keep_e, keep_l, p, **bkw)
    dkw = dict(ekw, loop_w=f["loop_w"]) if edge else {}
    dxl = V.dxl(xl, xr, att, out_ptr, out_dst, out_eid, K, C, bw["g_logit"], bw["g_loop"], SL, dxl0=dxl_agg, **dkw)
    pairs = [("x", dxl @ Wl + bw["d_xr"] @ Wr, lv[0].grad), ("Wl", dxl.t() @ x, lv[1].grad), ("bl", dxl.sum(0), lv[2].grad),
             ("Wr", bw["d_xr"].t() @ x, lv[3].grad), ("br", bw["d_xr"].sum(0), lv[4].grad), ("att", bw["d_att"].view(K, C), lv[5].grad)]
    if edge:
        pairs += [("w", bw["d_edge_w"], lv[6].grad), ("lin_edge", bw["d_lin_edge"].view(-1, 1), lv[7].grad)]
        assert bool((bw["d_edge_w"][ei[0] == ei[1]] == 0).all())
    for name, got, ref in pairs:
        assert float((got - ref).abs().max()) <= tol(ref), name


@pytest.mark.parametrize("N,E_,D,unit", [(30, 200, 5, False), (12, 300, 7, True), (1, 3, 4, False), (40, 0, 3, False)])
def test_gine_references_chain_to_the_layer_reference(N, E_, D, unit):
    g = torch.Generator().manual_seed(N + D)
    ei = torch.randint(0, N, (2, E_), generator=g)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)          # noqa: E731
    x, a, b, w, gz, dw_add = rn(N, D), rn(D), rn(D), torch.rand(E_, generator=g, dtype=F64), rn(N, D), rn(E_)
    lv = [t.clone().requires_grad_(True) for t in (x, a, b, w)]
    z = gine_aggregate(lv[0], ei, None if unit else lv[3], lv[1], lv[2], E.DIAG)
    z.backward(gz)
    in_ptr, in_src, in_eid = E.csr_of(ei[1], ei[0], N)
    out_ptr, out_dst, out_eid = E.csr_of(ei[0], ei[1], N)
    wv = None if unit else w
    tol = lambda r: 1e-10 * (1.0 + float(r.detach().abs().max()))              # noqa: E731
    assert float((E.fwd(x, in_ptr, in_src, in_eid, wv, a, b) - z.detach()).abs().max()) <= tol(z)
    bw = E.bwd(x, gz, out_ptr, out_dst, out_eid, wv, a, b, dw_add=dw_add)
    pairs = [("x", bw["d_x"], lv[0].grad), ("a", bw["d_a"], lv[1].grad), ("b", bw["d_b"], lv[2].grad)]
    if not unit and E_:
        pairs.append(("w", bw["d_edge_w"] - dw_add, lv[3].grad))
    for name, got, ref in pairs:
        assert float((got - ref).abs().max()) <= tol(ref), name


# ------------------------------------------------------------------------------------------------ fp32 inside the bound, faults outside
def _keep(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= V.P_DROP


_cache = {}


def v2_setup(case):
    """Graph, inputs and src-CSR of a case, built once."""
    if case["name"] not in _cache:
        gr = V.case_graph(case)
        n, N = gr["n"], gr["N"]
        r = V.G.rows_of(gr["ptr"])
        out_ptr, out_dst, out_eid = V.csr_of(gr["col"][:n].long(), r, N)
        _cache.clear()                                  # one case at a time: the large ones are large
        _cache[case["name"]] = (gr, V.inputs(gr, case["K"], case["C"], case["mode"]), (out_ptr, out_dst, gr["eid"][:n].long()[out_eid]))
    return _cache[case["name"]]


def v2_check(case, edge, p, mut=None):
    """The three GATv2 entry points on one case in fp32 (with `mut` planted) against fp64 and the bounds: -> number of elements outside."""
    K, C, N = case["K"], case["C"], case["N"]
    gr, x, ocsr = v2_setup(case)
    a = (x["xl"], x["xr"], x["att"], gr["ptr"], gr["col"], gr["eid"], K, C, V.SLOPE)
    n = gr["n"]
    geo = V.geom_of_code(V.case_codes(case, edge)[1], N)
    keep_e, keep_l = (_keep((n, K), 1), _keep((N, K), 2)) if p else (None, None)
    ekw = dict(edge_w=x["w"], lin_edge=x["le"]) if edge else {}
    ref = V.alpha_fwd(*a, bounds=True, **ekw)
    got = V.alpha_fwd(*a, dt=F32, mut=mut, gv=geo["gv"], **ekw)
    assert got["soft"].dtype == F32
    bad = int(V.outside(got["soft"], ref["soft"], ref["soft_bound"]).sum()) + int(V.outside(got["soft_loop"], ref["soft_loop"], ref["soft_loop_bound"]).sum())
    s32, l32 = ref["soft"].float(), ref["soft_loop"].float()
    bkw = dict(ekw, loop_w=ref["loop_w"].float(), loop_inv_cnt=ref["loop_inv_cnt"].float(), dw_add=x["dw_add"] if p else None) if edge else {}
    b = a[:8] + (s32, l32, x["galpha"], x["gloop"], V.SLOPE, keep_e, keep_l, p)
    bref = V.alpha_bwd(*b, geo=geo, bounds=True, **bkw)
    bgot = V.alpha_bwd(*b, geo=geo, dt=F32, mut=mut, **bkw)
    for k in bgot:
        assert bgot[k].dtype == F32
        bad += int(V.outside(bgot[k], bref[k], bref[k + "_bound"]).sum())
    dkw = dict(ekw, loop_w=bkw["loop_w"]) if edge else {}
    d = (x["xl"], x["xr"], x["att"], *ocsr, K, C, bref["g_logit"].float(), bref["g_loop"].float(), V.SLOPE)
    for d0 in (None, x["dxl0"]):
        dref, db = V.dxl(*d, dxl0=d0, bound=True, **dkw)
        bad += int(V.outside(V.dxl(*d, dxl0=d0, dt=F32, mut=mut, **dkw), dref, db).sum())
    return bad


def gine_check(case, mut=None, unit=False, dw_add=True):
    gr = E.case_graph(case)
    x = E.inputs(case, gr)
    w = None if unit else x["w"]
    a = (gr["ptr"], gr["col"], gr["eid"], w, x["a"], x["b"])
    fmut = mut if mut in ("relu_after_sum", "skip_tail") else None
    zref, zb = E.fwd(x["x"], *a, bound=True)
    bad = int(E.outside(E.fwd(x["x"], *a, dt=F32, mut=fmut, step=case["nw"]), zref, zb).sum())
    geo = E.bwd_geom(case["N"], E.case_code(case, True))
    kw = dict(dw_add=x["dw_add"] if dw_add else None, geo=geo)
    ref = E.bwd(x["x"], x["dz"], *a, bounds=True, **kw)
    got = E.bwd(x["x"], x["dz"], *a, dt=F32, mut=None if fmut else mut, **kw)
    for k in got:
        assert got[k].dtype == F32
        bad += int(E.outside(got[k], ref[k], ref[k + "_bound"]).sum())
    return bad


@pytest.mark.parametrize("case", V.ALL_CASES, ids=lambda c: c["name"])
def test_gatv2_in_fp32_is_inside_its_bounds(case):
    for edge, p in V.case_combos(case):
        assert v2_check(case, edge, p) == 0, (edge, p)


@pytest.mark.parametrize("case", E.ALL_CASES, ids=lambda c: c["name"])
def test_gine_in_fp32_is_inside_its_bounds(case):
    assert gine_check(case) == 0 and gine_check(case, unit=True, dw_add=False) == 0


def test_every_planted_gatv2_fault_leaves_the_bound_on_some_case():
    """One fault each, evaluated in fp32 like the unmutated references above; the cases named are where it must show."""
    by = {c["name"]: c for c in V.ALL_CASES}
    std, chunks = by["v1_K5_C5"], [c for c in V.SMALL_CASES if not c["code_fwd"] // 100 % 10]
    assert len(chunks) == 11
    for c in (std, by["v4_K2_C16"], by["v1_K9_C1"]):
        for edge in (False, True):
            assert v2_check(c, edge, 0.0, "no_loop_in_sum") > 0, c["name"]       # the loop left out of the row sum
            assert v2_check(c, edge, 0.0, "keep_self") > 0, c["name"]            # an (i, i) entry not removed
            assert v2_check(c, edge, 0.0, "slope_side") > 0, c["name"]           # the slope taken at s > 0
            assert v2_check(c, edge, 0.0, "no_loop_dxl") > 0, c["name"]          # the loop term of d_xl missing
            assert v2_check(c, edge, 0.0, "no_accumulate") > 0, c["name"]        # accumulate ignored
            assert v2_check(c, edge, V.P_DROP, "no_drop_scale") > 0, c["name"]   # drop_scale missing in the backward
        assert v2_check(c, True, 0.0, "loop_sum_w") > 0, c["name"]               # the loop carrying the sum, not the mean weight
        assert v2_check(c, True, 0.0, "no_loop_dw") > 0, c["name"]               # the loop's share of d_edge_w missing
        assert v2_check(c, True, V.P_DROP, "no_dw_add") > 0, c["name"]           # dw_add ignored
        assert v2_check(c, True, 0.0, "drop_partial") > 0, c["name"]             # one workgroup's partial row missing in the finish
    for c in chunks:                                                              # the channels beyond the first G VEC skipped
        assert v2_check(c, True, 0.0, "skip_chunks") > 0, c["name"]
    for c in V.ITERS_CASES[:3]:                                                   # a workgroup's last row pass missing from d att
        assert v2_check(c, True, 0.0, "drop_last_pass") > 0, c["name"]


def test_every_planted_gine_fault_leaves_the_bound_on_some_case():
    by = {c["name"]: c for c in E.ALL_CASES}
    for c in E.CASES:
        assert gine_check(c, "relu_after_sum") > 0, c["name"]                     # ReLU applied after the sum
        assert gine_check(c, "skip_tail") > 0, c["name"]                          # the entries past the last full group of 4 step dropped
        assert gine_check(c, "no_diag") > 0, c["name"]                            # diag missing in d_x
        assert gine_check(c, "da_no_w") > 0, c["name"]                            # d_a summed without w
        assert gine_check(c, "relu0") > 0, c["name"]                              # relu'(0) = 1, weights as given
        if c["D"] > 1:
            assert gine_check(c, "relu0", unit=True) > 0, c["name"]               # ... and unit weights
    two = [c for c in E.ALL_CASES if c["D"] > 64 * (E.case_code(c, True) // 100 % 10)]
    assert {E.case_code(c, True) // 100 % 10 for c in two} == {1, 2, 4}
    for c in two:                                                                 # the second column chunk's share of d_edge_w dropped
        assert gine_check(c, "drop_chunk2") > 0, c["name"]
    for name in ("block4_N2100_D70", "block16_N520_D5"):                          # the rows a workgroup reaches by striding dropped
        assert gine_check(by[name], "no_stride") > 0, name
