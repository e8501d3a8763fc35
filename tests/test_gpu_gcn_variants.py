"""GPU: every kernel variant behind sgs_spmm_csr, sgs_sddmm_csr, sgs_colsum and sgs_act_bwd_colsum against the fp64 reference of
tests/gcn_ref.py, through the C ABI.  The case tables live in gcn_ref.py; tests/test_gcn_variant_table.py proves on the CPU that they reach
every variant the launchers can pick and straddle every threshold.

Every output is carved from a larger buffer: 64 floats of a sentinel bit pattern on both sides (checked bitwise afterwards), the output
region itself pre-filled with NaN (so an element that is not written shows).  Each case asserts, in order: the variant code, the red zones,
no NaN, |got - ref64| <= the a-priori bound of gcn_ref.py element-wise, and bitwise equality of a second call.  The CSR index arrays
carry gcn_ref.PAD valid entries behind the last row, so a kernel that walks past a row's end produces a wrong number, not a fault."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gcn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RED = 64
SENTINEL = 0x5EA1DEAD
SEED, SITE = 0x51F15EED, 3
GOLD = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


def guarded(n, off=0):
    """-> (buffer, view of n floats at float offset RED + off): sentinel everywhere else, NaN inside."""
    buf = torch.empty(RED + off + n + RED, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(SENTINEL)
    out = buf[RED + off:RED + off + n]
    out.fill_(float("nan"))
    return buf, out


def red_zones_intact(buf, n, off=0):
    w = buf.view(torch.int32)
    return bool((w[:RED + off] == SENTINEL).all()) and bool((w[RED + off + n:] == SENTINEL).all())


def shifted(t, off):
    """A device copy of `t` whose first element sits `off` floats past a 256-byte boundary."""
    buf = torch.empty(t.numel() + off + 4, dtype=torch.float32, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def aligned16(*ts):
    return int(all(t.data_ptr() % 16 == 0 for t in ts))


def dptr(t):
    return None if t is None else t.data_ptr()


def within(got, ref64, bound):
    err = (got.double().cpu() - ref64).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        return f"{int(bad.sum())} elements out of bound; first flat index {i}: err {float(err.flatten()[i]):.3e} > {float(bound.flatten()[i]):.3e}"
    return ""


def run_spmm(pkg, case, gr, dev, X, diag, bias, act, Yoff):
    L, ops = pkg._lib.lib(), pkg.ops
    N, D, n = case["N"], case["D"], gr["nnz"]
    buf, Y = guarded(N * D, Yoff)
    ops._lib.check(L.sgs_spmm_csr(X.data_ptr(), N, D, n, dev["ptr"].data_ptr(), dev["col"].data_ptr(), dev["val"].data_ptr(), dptr(diag),
                                  dptr(bias), act, R.P_DROP if act == R.ACT_RELU_DROPOUT else 0.0, SEED, SITE, Y.data_ptr(), ops._stream()),
                   "sgs_spmm_csr")
    torch.cuda.synchronize()
    return buf, Y.view(N, D)


def check_spmm_case(pkg, case, combos):
    L, ops = pkg._lib.lib(), pkg.ops
    N, D = case["N"], case["D"]
    gr = R.graph(N, case["nnz"], case["nw"], case["hub"])
    n = gr["nnz"]
    dev = {k: gr[k].to(DEV) for k in ("ptr", "col", "val")}
    ptr, col, val = gr["ptr"], gr["col"][:n], gr["val"][:n]
    Xoff, Yoff = (1 if case["align"] == "a" else 0), (1 if case["align"] == "b" else 0)
    for diag_on, bias_on, act in combos:
        drop = act == R.ACT_RELU_DROPOUT
        X, diag, bias = R.spmm_inputs(N, D, R.DROP_BIAS if drop else 0.0)
        diag, bias = (diag if diag_on else None), (bias if bias_on else None)
        Xd = shifted(X, Xoff)
        dd, bd = (None if diag is None else diag.to(DEV)), (None if bias is None else bias.to(DEV))
        buf, Y = run_spmm(pkg, case, gr, dev, Xd, dd, bd, act, Yoff)
        tag = f"{case['name']} diag={diag_on} bias={bias_on} act={act}"
        assert L.sgs_spmm_csr_variant(N, D, n, aligned16(Xd, Y)) == case["code"], tag                      # 1
        assert red_zones_intact(buf, N * D, Yoff), tag                                                      # 2
        assert not bool(torch.isnan(Y).any()), tag                                                          # 3
        keep = ops.dropout_keep(SEED, SITE, N, D, R.P_DROP, DEV).cpu() if drop else None
        Z = R.spmm_pre(ptr, col, val.double(), None if diag is None else diag.double(), None if bias is None else bias.double(), X.double())
        pb = R.spmm_pre_bound(ptr, col, val, diag, bias, X)
        Yref = R.activate(Z, act, keep, R.P_DROP)
        msg = within(Y, Yref, R.spmm_bound(pb, Yref, act, R.P_DROP))                                         # 4
        assert not msg, f"{tag}: {msg}"
        if drop:            # the kept set, wherever the output can show it (gcn_ref.ambiguous; capped on the reference alone)
            amb = R.ambiguous(Z, pb)
            assert float(amb.double().mean()) <= R.MAX_AMBIGUOUS, tag
            assert torch.equal((Y.cpu() != 0)[~amb], keep[~amb]), tag
        buf2, Y2 = run_spmm(pkg, case, gr, dev, Xd, dd, bd, act, Yoff)                                       # 5
        assert torch.equal(Y2, Y) and red_zones_intact(buf2, N * D, Yoff), tag


@pytest.mark.parametrize("case", R.SPMM_CASES, ids=lambda c: c["name"])
def test_spmm_variant_vs_fp64(pkg, case):
    check_spmm_case(pkg, case, R.SPMM_COMBOS)


@pytest.mark.parametrize("name", ["spmm_v4_lpr16_D64", "spmm_v1_lpr64_D41", "spmm_rb_v4_nw4_D64", "spmm_rb_v1_nw16_D41_at256N"])
def test_spmm_dropout_mask_follows_the_epoch_buffer(pkg, name):
    """Both dropout hash paths (dropout_keep_at in spmm_csr; dropout_row_key + dropout_keep_col in the row-block form) under a registered
    non-zero epoch: the kept set is sgs_dropout_keep's under the same epoch, which is the epoch-free mask of seed + epoch * 2^64 / phi."""
    ops = pkg.ops
    case = next(c for c in R.SPMM_CASES if c["name"] == name)
    N, D = case["N"], case["D"]
    base = ops.dropout_keep(SEED, SITE, N, D, R.P_DROP, DEV)
    shifted_seed = ops.dropout_keep((SEED + 5 * GOLD) % (1 << 64), SITE, N, D, R.P_DROP, DEV)
    epoch = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    try:
        ops.set_rng_epoch_buffer(epoch)
        k5 = ops.dropout_keep(SEED, SITE, N, D, R.P_DROP, DEV)
        check_spmm_case(pkg, case, [(True, True, R.ACT_RELU_DROPOUT)])
        torch.cuda.synchronize()
    finally:
        ops.set_rng_epoch_buffer(None)
    assert torch.equal(k5, shifted_seed) and not torch.equal(k5, base)


def run_sddmm(pkg, case, gr, dev, A, B, with_diag):
    L, ops = pkg._lib.lib(), pkg.ops
    N, D, n = case["N"], case["D"], gr["nnz"]
    gbuf, g = guarded(n)
    dbuf, gd = guarded(N)
    ops._lib.check(L.sgs_sddmm_csr(A.data_ptr(), B.data_ptr(), N, D, n, dev["ptr"].data_ptr(), dev["col"].data_ptr(), dev["eid"].data_ptr(),
                                   g.data_ptr(), gd.data_ptr() if with_diag else None, ops._stream()), "sgs_sddmm_csr")
    torch.cuda.synchronize()
    return gbuf, g, dbuf, gd


@pytest.mark.parametrize("case", R.SDDMM_CASES, ids=lambda c: c["name"])
def test_sddmm_variant_vs_fp64(pkg, case):
    L = pkg._lib.lib()
    N, D = case["N"], case["D"]
    gr = R.graph(N, case["nnz"], case["nw"], case["hub"])
    n = gr["nnz"]
    dev = {k: gr[k].to(DEV) for k in ("ptr", "col", "eid")}
    A = torch.randn(N, D, generator=gr["gen"])
    B = torch.randn(N, D, generator=gr["gen"])
    Ad, Bd = shifted(A, 1 if case["align"] == "a" else 0), shifted(B, 1 if case["align"] == "b" else 0)
    g64, d64 = R.sddmm(gr["ptr"], gr["col"][:n], gr["eid"][:n], A.double(), B.double())
    bg, bdg = R.sddmm_bound(gr["ptr"], gr["col"][:n], gr["eid"][:n], A, B)
    for with_diag in (True, False):
        tag = f"{case['name']} gdiag={with_diag}"
        gbuf, g, dbuf, gd = run_sddmm(pkg, case, gr, dev, Ad, Bd, with_diag)
        assert L.sgs_sddmm_csr_variant(N, D, n, aligned16(Ad, Bd)) == case["code"], tag                    # 1
        assert red_zones_intact(gbuf, n) and red_zones_intact(dbuf, N), tag                                 # 2
        assert not bool(torch.isnan(g).any()), tag                                                          # 3: every eid slot written
        if with_diag:
            assert not bool(torch.isnan(gd).any()), tag
        else:
            assert bool(torch.isnan(gd).all()), tag                                                         # a null gdiag: nothing written
        msg = within(g, g64, bg) or (with_diag and within(gd, d64, bdg))                                    # 4
        assert not msg, f"{tag}: {msg}"
        gbuf2, g2, dbuf2, gd2 = run_sddmm(pkg, case, gr, dev, Ad, Bd, with_diag)                            # 5
        assert torch.equal(g2, g) and (not with_diag or torch.equal(gd2, gd)), tag
        assert red_zones_intact(gbuf2, n) and red_zones_intact(dbuf2, N), tag


def poisoned_ws(L, N, D):
    ws = torch.empty(L.sgs_colsum_workspace_bytes(N, D), dtype=torch.uint8, device=DEV)
    ws.fill_(0xFF)
    return ws


def run_colsum(pkg, A, N, D):
    L, ops = pkg._lib.lib(), pkg.ops
    buf, out = guarded(D)
    ws = poisoned_ws(L, N, D)
    ops._lib.check(L.sgs_colsum(dptr(A), N, D, out.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "sgs_colsum")
    torch.cuda.synchronize()
    return buf, out


def run_act_bwd_colsum(pkg, dY, Y, N, D, act):
    L, ops = pkg._lib.lib(), pkg.ops
    zbuf, dZ = guarded(N * D)
    buf, out = guarded(D)
    ws = poisoned_ws(L, N, D)
    ops._lib.check(L.sgs_act_bwd_colsum(dptr(dY), dptr(Y), N, D, act, R.P_DROP if act == R.ACT_RELU_DROPOUT else 0.0, dZ.data_ptr(),
                                        out.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "sgs_act_bwd_colsum")
    torch.cuda.synchronize()
    return zbuf, dZ.view(N, D), buf, out


@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=lambda c: c["name"])
def test_colsum_variant_vs_fp64(pkg, case):
    L = pkg._lib.lib()
    N, D = case["N"], case["D"]
    A, Y = R.colsum_inputs(case)
    Ad, Yd = (A.to(DEV), Y.to(DEV)) if N else (None, None)
    assert L.sgs_colsum_variant(N, D, 0) == case["code"]                                                    # 1
    buf, out = run_colsum(pkg, Ad, N, D)
    assert red_zones_intact(buf, D)                                                                         # 2
    assert not bool(torch.isnan(out).any())                                                                 # 3
    msg = within(out, R.colsum(A.double()), R.colsum_bound(A))                                              # 4
    assert not msg, f"{case['name']}: {msg}"
    buf2, out2 = run_colsum(pkg, Ad, N, D)                                                                  # 5
    assert torch.equal(out2, out) and red_zones_intact(buf2, D)
    assert L.sgs_colsum_variant(N, D, 1) == case["code"] + R.FUSED
    for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_RELU_DROPOUT):
        tag = f"{case['name']} act={act}"
        zbuf, dZ, buf, out = run_act_bwd_colsum(pkg, Ad, Yd, N, D, act)
        assert red_zones_intact(zbuf, N * D) and red_zones_intact(buf, D), tag
        assert not bool(torch.isnan(dZ).any()) and not bool(torch.isnan(out).any()), tag
        dZref = R.act_bwd(A, Y, act, R.P_DROP)
        assert torch.equal(dZ.cpu(), dZref), tag                                   # a select and one multiply: exact
        msg = within(out, R.colsum(dZref.double()), R.colsum_bound(dZref))
        assert not msg, f"{tag}: {msg}"
        zbuf2, dZ2, buf2, out2 = run_act_bwd_colsum(pkg, Ad, Yd, N, D, act)
        assert torch.equal(dZ2, dZ) and torch.equal(out2, out), tag


# ------------------------------------------------------------------------------------------------ gcn_norm forward / backward
# rsqrt on the device is not correctly rounded, so there is no a-priori bound here: the criterion is the one of
# test_gpu_gcn.py::test_gcn_conv_forward_backward_vs_oracle -- the error against the fp64 oracle is at most 5 x the fp32 oracle's own
# on the same case (floor 2e-6) and below 1e-4, relative to the largest fp64 entry.
from oracle import sgs_oracle as O  # noqa: E402


def norm_edges(N, nnz, hub):
    """An edge list over the row-length graph (rows = destinations), in shuffled edge order: node 1 has no edge at all, node 0 carries two
    self-loop edges, one destination has `hub` in-edges; duplicates occur."""
    gr = R.graph(N, nnz, 4, hub, seed=9)
    dst = R.rows_of(gr["ptr"])
    src = gr["col"][:nnz].long().clone()
    src[src == 1] = 2
    src[0] = 0
    src[1] = 0
    perm = torch.randperm(nnz, generator=gr["gen"])
    return torch.stack([src, dst])[:, perm].contiguous(), gr["gen"]


def oracle_norm(ei, w, N, dt, gw, gl):
    """-> (what [n] by edge id, 0 at self-loop edges; what_loop [N]; d w [n]) for the upstream gradients gw [n], gl [N]."""
    n = ei.shape[1]
    wv = (torch.ones(n) if w is None else w).detach().clone().to(dt).requires_grad_(True)
    _, wh = O.gcn_norm(ei, wv, N, dtype=dt)
    mask = ei[0] != ei[1]
    m = int(mask.sum())
    ((wh[:m] * gw.to(dt)[mask]).sum() + (wh[m:] * gl.to(dt)).sum()).backward()
    what = torch.zeros(n, dtype=dt)
    what[mask] = wh[:m].detach()
    return what, wh[m:].detach(), wv.grad


def oracle_close(got, r32, r64, tag):
    scale = float(r64.abs().max()) + 1e-12
    err = float((got.double().cpu() - r64).abs().max()) / scale
    err32 = float((r32.double() - r64).abs().max()) / scale
    assert err <= max(5 * err32, 2e-6) and err < 1e-4, f"{tag}: rel err {err:.2e} (fp32 oracle {err32:.2e})"


@pytest.mark.parametrize("N,nnz,hub", [(300, 46000, 40000), (70, 900, 300)])
@pytest.mark.parametrize("weighted", [True, False])
def test_gcn_norm_fwd_bwd_on_row_length_graphs_vs_oracle(pkg, N, nnz, hub, weighted):
    L, ops = pkg._lib.lib(), pkg.ops
    ei, g = norm_edges(N, nnz, hub)
    n = ei.shape[1]
    w = (torch.rand(n, generator=g) + 0.05) if weighted else None
    gws = [torch.randn(n, generator=g) for _ in range(2)]
    gls = [torch.randn(N, generator=g) for _ in range(2)]
    add = torch.randn(n, generator=g)
    gr = ops.Graph(ei.to(DEV), N)
    eid = ei.to(DEV)
    csr = [gr.in_ptr, gr.in_src, gr.in_eid, gr.out_ptr, gr.out_dst, gr.out_eid]
    wd = None if w is None else w.to(DEV)

    def fwd():
        bufs = {k: guarded(z) for k, z in (("dis", N), ("loopw", N), ("what_in", n), ("what_out", n), ("what_loop", N))}
        ops._lib.check(L.sgs_gcn_norm_fwd(dptr(wd), n, N, *[t.data_ptr() for t in csr], gr.loop_eid.data_ptr(),
                                          *[bufs[k][1].data_ptr() for k in ("dis", "loopw", "what_in", "what_out", "what_loop")],
                                          ops._stream()), "sgs_gcn_norm_fwd")
        torch.cuda.synchronize()
        return bufs
    bufs = fwd()
    ref = {dt: oracle_norm(ei, w, N, dt, gws[0], gls[0]) for dt in (torch.float32, torch.float64)}
    for k, (buf, out) in bufs.items():
        assert red_zones_intact(buf, out.numel()) and not bool(torch.isnan(out).any()), k
    in_eid, out_eid = gr.in_eid.cpu().long()[:n], gr.out_eid.cpu().long()[:n]
    for k, pick in (("what_in", lambda r: r[0][in_eid]), ("what_out", lambda r: r[0][out_eid]), ("what_loop", lambda r: r[1])):
        oracle_close(bufs[k][1], pick(ref[torch.float32]), pick(ref[torch.float64]), k)
    for k, (buf, out) in fwd().items():
        assert torch.equal(out, bufs[k][1]), k
    dis, loopw = bufs["dis"][1], bufs["loopw"][1]
    w1 = torch.ones(n, device=DEV) if wd is None else wd            # the backward reads w: unit weights as ones

    def bwd(second, dw_add):
        """dw_add: None | "separate" | "alias" (dw_add is dw itself, which then starts out holding the addend instead of NaN)."""
        buf, dw = guarded(n)
        ws = torch.empty(L.sgs_gcn_norm_bwd_workspace_bytes(N), dtype=torch.uint8, device=DEV).fill_(0xFF)
        g1, l1, g2, l2 = gws[0].to(DEV), gls[0].to(DEV), gws[1].to(DEV), gls[1].to(DEV)
        tail = [n, N, dis.data_ptr(), loopw.data_ptr(), *[t.data_ptr() for t in csr], gr.loop_eid.data_ptr(), eid.data_ptr(), dw.data_ptr(),
                ws.data_ptr(), ws.numel(), ops._stream()]
        if second is None:
            ops._lib.check(L.sgs_gcn_norm_bwd(w1.data_ptr(), g1.data_ptr(), l1.data_ptr(), *tail), "sgs_gcn_norm_bwd")
        else:
            a = None
            if dw_add == "alias":
                dw.copy_(add)
                a = dw
            elif dw_add == "separate":
                a = add.to(DEV)
            ops._lib.check(L.sgs_gcn_norm_bwd_sum(w1.data_ptr(), g1.data_ptr(), l1.data_ptr(), g2.data_ptr() if second else None,
                                                  l2.data_ptr() if second else None, dptr(a), *tail), "sgs_gcn_norm_bwd_sum")
        torch.cuda.synchronize()
        return buf, dw

    for second in (None, False, True):
        for dw_add in ((None,) if second is None else (None, "separate", "alias")):
            tag = f"second={second} dw_add={dw_add}"
            buf, dw = bwd(second, dw_add)
            assert red_zones_intact(buf, n) and not bool(torch.isnan(dw).any()), tag
            gw, gl = (gws[0] + gws[1], gls[0] + gls[1]) if second else (gws[0], gls[0])
            r = {dt: oracle_norm(ei, w, N, dt, gw, gl)[2] + (add.to(dt) if dw_add else 0) for dt in (torch.float32, torch.float64)}
            oracle_close(dw, r[torch.float32], r[torch.float64], tag)
            assert torch.equal(bwd(second, dw_add)[1], dw), tag
