"""GPU: every kernel variant behind the GATv2 and GINE entry points (sections K8c / K8d of include/sgs_hip.h) against the fp64 references
of tests/gatv2_kernels_ref.py and tests/gine_kernels_ref.py, through the C ABI.  The case tables live in those files;
tests/test_gatv2_gine_variant_table.py proves on the CPU that they reach every code sgs_gatv2_variant / sgs_gine_variant can return,
straddle every threshold, and that the bounds see single planted faults.

Calling convention of tests/test_gpu_gat_heads_kernels.py (its helpers are imported): every output is carved from a larger buffer with 64
words of a sentinel bit pattern on both sides, the output region pre-filled with NaN; the workspace is sized exactly to its query and sits
in a red zone of its own; inputs are passed at a chosen float offset, so alignment is the test's choice.  Each case asserts, in order: the
variant code, the red zones, no NaN, |got - ref64| <= the a-priori bound ELEMENT BY ELEMENT, the exact relations (alpha from the kernel's
own soft and the exported dropout mask; the zeros of (i, i) entries; buffers a NULL edge_w leaves untouched; unit weights bitwise a vector
of ones; outputs unchanged by the absence of another), and bitwise equality of a second call.  The largest error / bound ratio per
compared quantity is printed ("gatv2_gine_ratio")."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_heads_ref as H  # noqa: E402
import gatv2_kernels_ref as V  # noqa: E402
import gcn_ref as G  # noqa: E402
import gine_kernels_ref as E  # noqa: E402
from test_gpu_gat_heads_kernels import DEV, RATIOS, SEED, SITE, Outs, dptr, guarded, red_zones_intact, shifted, within  # noqa: E402

pytestmark = pytest.mark.gpu
SLOPE = V.SLOPE


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


def report(prefix):
    for e in sorted(RATIOS):
        if e.startswith(prefix):
            print("gatv2_gine_ratio", e, f"{RATIOS[e]:.4f}")


def al16(*ts):
    return int(all(t.data_ptr() % 16 == 0 for t in ts))


def padded_i32(t):
    """An int32 index array with gcn_ref.PAD valid (zero) entries behind it."""
    out = torch.zeros(t.numel() + G.PAD, dtype=torch.int32)
    out[:t.numel()] = t.int()
    return out


def untouched(o):
    """Every output of `o` still NaN and its red zones intact."""
    return all(red_zones_intact(o.buf[k], v.numel(), o.off[k]) and bool(torch.isnan(v).all()) for k, v in o.out.items())


class Workspace:
    """A workspace of exactly `nbytes`, in its own red zone."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.nbytes, (self.buf, self.out) = nbytes, guarded(nbytes // 4)

    def args(self):
        return self.out.data_ptr(), self.nbytes

    def intact(self):
        return red_zones_intact(self.buf, self.nbytes // 4)


# ------------------------------------------------------------------------------------------------ GATv2
@pytest.mark.parametrize("case", V.ALL_CASES, ids=lambda c: c["name"])
def test_gatv2_vs_fp64(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    chk, st = ops._lib.check, ops._stream()
    N, K, C, un = case["N"], case["K"], case["C"], case["un"]
    D = K * C
    gr = V.case_graph(case)
    x = V.inputs(gr, K, C, case["mode"])
    n = gr["n"]
    ptr, src, eid = gr["ptr"], gr["col"], gr["eid"]
    r = G.rows_of(ptr)
    optr, odst, oord = V.csr_of(src[:n].long(), r, N)
    ocsr = (optr.int(), padded_i32(odst), padded_i32(eid[:n].long()[oord]))
    cp = [t.to(DEV) for t in (ptr, src, eid)]
    cpp = [t.data_ptr() for t in cp]
    ocp = [t.to(DEV) for t in ocsr]
    ocpp = [t.data_ptr() for t in ocp]
    d = {k: (shifted(v, 1 if un == k else 0) if k in ("xl", "xr", "att") else v.to(DEV)) for k, v in x.items()}
    d["le"] = shifted(x["le"], 1 if un == "lin_edge" else 0)
    # without entries the per-entry arrays are empty (a null pointer): edge_w and d_edge_w, whose presence selects the edge term, get a
    # four-float stand-in that must come back untouched
    stand_in = torch.full((4,), float("nan"), device=DEV)
    if n == 0:
        d["w"] = stand_in
    self_eid = eid[:n].long()[src[:n].long() == r]
    assert case["kind"] != "std" or self_eid.numel() >= 3
    for edge, p in V.case_combos(case):
        tag = f"{case['name']} edge={edge} p={p}"
        codes = V.case_codes(case, edge)
        geo = V.geom_of_code(codes[1], N)
        vin = [d["xl"], d["xr"], d["att"]] + ([d["le"]] if edge else [])
        keep_e = ops.dropout_keep(SEED, SITE, n, K, p, DEV).cpu() if (p and n) else (torch.ones(n, K, dtype=torch.bool) if p else None)
        keep_l = ops.dropout_keep(SEED, SITE + 1, N, K, p, DEV).cpu() if p else None
        head = [d["xl"].data_ptr(), d["xr"].data_ptr(), d["att"].data_ptr(), d["w"].data_ptr() if edge else None, d["le"].data_ptr()]
        assert L.sgs_gatv2_variant(V.OP_FWD, N, K, C, al16(*vin)) == codes[0], tag                          # 1

        def fwd():
            o, lo = Outs(soft=n * K, soft_loop=N * K, alpha=n * K, alpha_loop=N * K), Outs(loop_w=N, loop_inv_cnt=N)
            chk(L.sgs_gatv2_alpha_heads_fwd(*head, N, K, C, n, *cpp, SLOPE, p, SEED, SITE, o.ptr("soft"), o.ptr("soft_loop"), o.ptr("alpha"),
                                            o.ptr("alpha_loop"), lo.ptr("loop_w"), lo.ptr("loop_inv_cnt"), st), "sgs_gatv2_alpha_heads_fwd")
            torch.cuda.synchronize()
            return o, lo
        o, lo = fwd()
        assert not o.clean(), f"{tag}: {o.clean()}"                                                         # 2, 3
        assert (not lo.clean()) if edge else untouched(lo), tag
        ekw = dict(edge_w=x["w"], lin_edge=x["le"]) if edge else {}
        ref = V.alpha_fwd(x["xl"], x["xr"], x["att"], ptr, src, eid, K, C, SLOPE, loop_w=lo.cpu("loop_w", N) if edge else None, bounds=True, **ekw)
        soft, soft_loop = o.cpu("soft", n, K), o.cpu("soft_loop", N, K)
        fname = "gatv2_alpha_heads_fwd"
        msg = within(fname + ":soft", soft, ref["soft"], ref["soft_bound"]) or within(fname + ":soft", soft_loop, ref["soft_loop"], ref["soft_loop_bound"])
        if edge:
            msg = msg or within(fname + ":loop_w", lo.cpu("loop_w", N), ref["loop_w"], ref["loop_w_bound"])
            msg = msg or within(fname + ":loop_w", lo.cpu("loop_inv_cnt", N), ref["loop_inv_cnt"], ref["loop_inv_cnt_bound"])
        assert not msg, f"{tag}: {msg}"                                                                     # 4
        assert torch.equal(o.cpu("alpha", n, K), H.alpha_of(soft, keep_e, p)), tag                          # 5: exact given soft and the mask
        assert torch.equal(o.cpu("alpha_loop", N, K), H.dropped(soft_loop, keep_l, p)), tag
        assert bool((soft[self_eid] == 0).all()) and bool((o.cpu("alpha", n, K)[self_eid] == 0).all()), tag
        o2, lo2 = fwd()
        assert o.same(o2) and (not edge or lo.same(lo2)), tag                                               # 6

        # backward, judged on its own: soft from the fp64 forward rounded to fp32, seeded gradients
        s32, l32 = ref["soft"].float(), ref["soft_loop"].float()
        lw32, ic32 = (ref["loop_w"].float(), ref["loop_inv_cnt"].float()) if edge else (torch.zeros(N), torch.zeros(N))
        dw_add = x["dw_add"] if (edge and p) else None
        ins = [t.to(DEV) for t in (s32, l32, lw32, ic32)]
        bname = "gatv2_alpha_heads_bwd"

        def bwd():
            o = Outs(g_logit=n * K, g_loop=N * K, d_xr=(N * D, 1 if un == "d_xr" else 0, None), d_att=D)
            eo = Outs(d_lin_edge=D, d_edge_w=n)
            ws = Workspace(L.sgs_gatv2_alpha_heads_bwd_workspace_bytes(N, K, C))
            assert L.sgs_gatv2_variant(V.OP_BWD, N, K, C, al16(*vin, o.out["d_xr"])) == codes[1], tag       # 1
            chk(L.sgs_gatv2_alpha_heads_bwd(*head, ins[2].data_ptr(), ins[3].data_ptr(), N, K, C, n, *cpp, SLOPE, p, SEED, SITE, ins[0].data_ptr(),
                                            ins[1].data_ptr(), d["galpha"].data_ptr(), d["gloop"].data_ptr(),
                                            dptr(d["dw_add"] if dw_add is not None else None), o.ptr("g_logit"), o.ptr("g_loop"), o.ptr("d_xr"),
                                            o.ptr("d_att"), eo.ptr("d_lin_edge"), eo.ptr("d_edge_w") if n else stand_in.data_ptr(), *ws.args(), st),
                "sgs_gatv2_alpha_heads_bwd")
            torch.cuda.synchronize()
            assert ws.intact(), f"{tag}: red zone of the workspace"
            return o, eo
        o, eo = bwd()
        assert not o.clean(), f"{tag}: {o.clean()}"
        assert (not eo.clean()) if edge else untouched(eo), tag
        bkw = dict(ekw, loop_w=lw32, loop_inv_cnt=ic32, dw_add=dw_add) if edge else {}
        bref = V.alpha_bwd(x["xl"], x["xr"], x["att"], ptr, src, eid, K, C, s32, l32, x["galpha"], x["gloop"], SLOPE, keep_e, keep_l, p, geo=geo,
                           bounds=True, **bkw)
        shapes = dict(g_logit=(n, K), g_loop=(N, K), d_xr=(N, D), d_att=(D,), d_lin_edge=(D,), d_edge_w=(n,))
        for oo in ((o, eo) if edge else (o,)):
            for k in oo.out:
                msg = within(f"{bname}:{k}" + (":iters" if geo["iters"] > 1 and k in ("d_att", "d_lin_edge") else ""), oo.cpu(k, *shapes[k]),
                             bref[k], bref[k + "_bound"])
                assert not msg, f"{tag}: {msg}"
        assert bool((o.cpu("g_logit", n, K)[self_eid] == 0).all()), tag
        if edge:
            assert torch.equal(eo.cpu("d_edge_w", n)[self_eid], torch.zeros(self_eid.numel()) if dw_add is None else dw_add[self_eid]), tag
        o2, eo2 = bwd()
        assert o.same(o2) and (not edge or eo.same(eo2)) and bool(torch.isnan(stand_in).all()), tag

        # by source, from the reference's g_logit / g_loop rounded to fp32
        gins = [bref["g_logit"].float().to(DEV), bref["g_loop"].float().to(DEV)]
        dkw = dict(ekw, loop_w=lw32) if edge else {}
        for acc in (0, 1):
            def dxl():
                o = Outs(d_xl=(N * D, 1 if un == "d_xl" else 0, x["dxl0"] if acc else None))
                assert L.sgs_gatv2_variant(V.OP_DXL, N, K, C, al16(*vin, o.out["d_xl"])) == codes[2], tag   # 1
                chk(L.sgs_gatv2_dxl_heads(*head, ins[2].data_ptr(), gins[0].data_ptr(), gins[1].data_ptr(), N, K, C, n, *ocpp, SLOPE, acc,
                                          o.ptr("d_xl"), st), "sgs_gatv2_dxl_heads")
                torch.cuda.synchronize()
                return o
            o = dxl()
            assert not o.clean(), f"{tag} accumulate={acc}: {o.clean()}"
            dref, db = V.dxl(x["xl"], x["xr"], x["att"], *ocsr, K, C, bref["g_logit"].float(), bref["g_loop"].float(), SLOPE,
                             dxl0=x["dxl0"] if acc else None, bound=True, **dkw)
            msg = within("gatv2_dxl_heads", o.cpu("d_xl", N, D), dref, db)
            assert not msg, f"{tag} accumulate={acc}: {msg}"
            assert o.same(dxl()), tag
    report("gatv2_")


def test_gatv2_without_rows_returns_and_writes_nothing(pkg):
    L, ops = pkg._lib.lib(), pkg.ops
    st = ops._stream()
    K, C = 3, 5
    o = Outs(soft=8, soft_loop=8, alpha=8, alpha_loop=8, loop_w=8, loop_inv_cnt=8, g_logit=8, g_loop=8, d_xr=16, d_att=16, d_lin_edge=16,
             d_edge_w=8, d_xl=16)
    f = torch.ones(64, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    fp, ip = f.data_ptr(), i.data_ptr()
    ws = Workspace(L.sgs_gatv2_alpha_heads_bwd_workspace_bytes(0, K, C))
    assert L.sgs_gatv2_variant(V.OP_BWD, 0, K, C, 1) == V.code(2, 1, 5, 3, 1, 1)
    assert L.sgs_gatv2_alpha_heads_fwd(fp, fp, fp, fp, fp, 0, K, C, 0, ip, ip, ip, SLOPE, 0.0, SEED, SITE, o.ptr("soft"), o.ptr("soft_loop"),
                                       o.ptr("alpha"), o.ptr("alpha_loop"), o.ptr("loop_w"), o.ptr("loop_inv_cnt"), st) == 0
    assert L.sgs_gatv2_alpha_heads_bwd(fp, fp, fp, fp, fp, fp, fp, 0, K, C, 0, ip, ip, ip, SLOPE, 0.0, SEED, SITE, fp, fp, fp, fp, None,
                                       o.ptr("g_logit"), o.ptr("g_loop"), o.ptr("d_xr"), o.ptr("d_att"), o.ptr("d_lin_edge"), o.ptr("d_edge_w"),
                                       *ws.args(), st) == 0
    assert L.sgs_gatv2_dxl_heads(fp, fp, fp, fp, fp, fp, fp, fp, 0, K, C, 0, ip, ip, ip, SLOPE, 0, o.ptr("d_xl"), st) == 0
    torch.cuda.synchronize()
    assert untouched(o) and ws.intact() and bool(torch.isnan(ws.out).all())


# ------------------------------------------------------------------------------------------------ GINE
def _align_of(*ts):
    return min(16 if t.data_ptr() % 16 == 0 else 8 if t.data_ptr() % 8 == 0 else 4 for t in ts)


@pytest.mark.parametrize("case", E.ALL_CASES, ids=lambda c: c["name"])
def test_gine_vs_fp64(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    chk, st = ops._lib.check, ops._stream()
    N, D, n, un, off = case["N"], case["D"], case["nnz"], case["un"], case["off"]
    gr = E.case_graph(case)
    x = E.inputs(case, gr)
    csr = (gr["ptr"], gr["col"], gr["eid"])
    cp = [t.to(DEV) for t in csr]
    cpp = [t.data_ptr() for t in cp]
    sh = lambda k, name=None: shifted(x[k], off if un == (name or k) else 0)          # noqa: E731
    d = dict(x=sh("x"), a=sh("a"), b=sh("b"), dz=sh("dz", "zdz"), w=x["w"].to(DEV), ones=torch.ones(n, device=DEV), dw_add=x["dw_add"].to(DEV))
    zoff, xoff = (off if un == "zdz" else 0), (off if un == "d_x" else 0)

    def fwd(w):
        o = Outs(z=(N * D, zoff, None))
        assert L.sgs_gine_variant(N, D, n, _align_of(d["x"], d["a"], d["b"], o.out["z"])) == E.case_code(case, False)       # 1
        chk(L.sgs_gine_aggregate_fwd(d["x"].data_ptr(), dptr(w), d["a"].data_ptr(), d["b"].data_ptr(), E.DIAG, N, D, n, *cpp, o.ptr("z"), st),
            "sgs_gine_aggregate_fwd")
        torch.cuda.synchronize()
        return o
    for unit in (False, True):
        tag = f"{case['name']} unit={unit}"
        o = fwd(None if unit else d["w"])
        assert not o.clean(), f"{tag}: {o.clean()}"                                                          # 2, 3
        zref, zb = E.fwd(x["x"], *csr, None if unit else x["w"], x["a"], x["b"], bound=True)
        msg = within("gine_aggregate_fwd", o.cpu("z", N, D), zref, zb)                                       # 4
        assert not msg, f"{tag}: {msg}"
        assert o.same(fwd(d["ones"] if unit else d["w"])), tag                                               # 5 (unit weights = ones), 6

    geo = E.bwd_geom(N, E.case_code(case, True))
    shapes = dict(d_x=(N, D), d_edge_w=(n,), d_a=(D,), d_b=(D,))

    def bwd(w, want, dw_add=None):
        o = Outs(**{k: ((N * D, xoff, None) if k == "d_x" else n if k == "d_edge_w" else D) for k in want})
        ws = Workspace(L.sgs_gine_aggregate_bwd_workspace_bytes(N, D)) if "d_a" in want else None
        al = _align_of(d["x"], d["a"], d["b"], d["dz"], *([o.out["d_x"]] if "d_x" in want else []))
        assert L.sgs_gine_variant(N, D, n, al) == (E.case_code(case, True) if ("d_x" in want or un != "d_x") else 464)           # 1
        p = lambda k: o.ptr(k) if k in want else None          # noqa: E731
        chk(L.sgs_gine_aggregate_bwd(d["x"].data_ptr(), d["dz"].data_ptr(), dptr(w), d["a"].data_ptr(), d["b"].data_ptr(), E.DIAG, N, D, n, *cpp,
                                     dptr(dw_add), p("d_x"), p("d_edge_w"), p("d_a"), p("d_b"), *(ws.args() if ws else (None, 0)), st),
            "sgs_gine_aggregate_bwd")
        torch.cuda.synchronize()
        assert ws is None or ws.intact(), "red zone of the workspace"
        return o
    every = tuple(shapes)
    for unit, add in ((False, True), (False, False), (True, False)):
        tag = f"{case['name']} unit={unit} dw_add={add}"
        w, dwa = (None if unit else d["w"]), (d["dw_add"] if add else None)
        o = bwd(w, every, dwa)
        assert not o.clean(), f"{tag}: {o.clean()}"
        ref = E.bwd(x["x"], x["dz"], *csr, None if unit else x["w"], x["a"], x["b"], dw_add=x["dw_add"] if add else None, geo=geo, bounds=True)
        for k in every:
            msg = within(f"gine_aggregate_bwd:{'d_ab' if k in ('d_a', 'd_b') else k}", o.cpu(k, *shapes[k]), ref[k], ref[k + "_bound"])
            assert not msg, f"{tag}: {msg}"
        assert o.same(bwd(d["ones"] if unit else w, every, dwa)), tag                                        # unit weights = ones; second call
        if not add and not unit:
            # each output on its own: the others' absence changes no bit of it (an absent d_x is not part of the alignment: the case that
            # moves d_x off alignment then runs another variant and is compared with its bound alone)
            for want in (("d_x",), ("d_edge_w",), ("d_a", "d_b")):
                part = bwd(w, want)
                assert not part.clean(), f"{tag} {want}: {part.clean()}"
                for k in want:
                    if un == "d_x" and "d_x" not in want:
                        msg = within(f"gine_aggregate_bwd:{'d_ab' if k in ('d_a', 'd_b') else k}", part.cpu(k, *shapes[k]), ref[k], ref[k + "_bound"])
                        assert not msg, f"{tag} {want}: {msg}"
                    else:
                        assert torch.equal(part.out[k], o.out[k]), f"{tag} {want}: {k}"
    if x["zero"] is not None:            # the planted pre-activation of exactly 0 passes neither ReLU: checked by the bounds above; it exists
        j, k, e0 = x["zero"]
        assert E.pre(x["x"], x["w"][gr["eid"][k:k + 1].long()], x["a"], x["b"], torch.tensor([j]))[0, 0] == 0
    report("gine_")


def test_gine_without_rows_writes_zero_parameter_gradients(pkg):
    L, ops = pkg._lib.lib(), pkg.ops
    D = 70
    o, hid = Outs(d_a=D, d_b=D), Outs(d_x=16, d_edge_w=16, z=16)
    f = torch.ones(256, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    fp, ip = f.data_ptr(), i.data_ptr()
    ws = Workspace(L.sgs_gine_aggregate_bwd_workspace_bytes(0, D))
    assert L.sgs_gine_aggregate_fwd(fp, fp, fp, fp, E.DIAG, 0, D, 0, ip, ip, ip, hid.ptr("z"), ops._stream()) == 0
    assert L.sgs_gine_aggregate_bwd(fp, fp, fp, fp, fp, E.DIAG, 0, D, 0, ip, ip, ip, None, hid.ptr("d_x"), hid.ptr("d_edge_w"), o.ptr("d_a"),
                                    o.ptr("d_b"), *ws.args(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert not o.clean() and ws.intact() and untouched(hid)
    assert bool((o.out["d_a"] == 0).all()) and bool((o.out["d_b"] == 0).all())
