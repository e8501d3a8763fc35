"""GPU: every kernel variant behind the multi-head GAT entry points (section K8h of include/sgs_hip.h) against the fp64 references of
tests/gat_heads_ref.py, through the C ABI.  The case tables live in gat_heads_ref.py; tests/test_gat_heads_variant_table.py proves on the
CPU that they reach every code sgs_gat_heads_variant can return, straddle every threshold, and that the bounds see single planted faults.

Every output is carved from a larger buffer: 64 words of a sentinel bit pattern on both sides (checked bitwise afterwards), the output
region itself pre-filled with NaN (so an element that is not written shows; what the contract sets to 0 must be 0).  Each case asserts, in
order: the variant code, the red zones, no NaN, |got - ref64| <= the a-priori bound ELEMENT BY ELEMENT, the exact relations (alpha from the
kernel's own soft and the exported dropout mask; the zeros of (i, i) entries), and bitwise equality of a second call.  The CSR index arrays
carry gcn_ref.PAD valid entries behind the last row.  The largest error / bound ratio per entry point is printed ("gat_heads_ratio")."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_heads_ref as R  # noqa: E402
import gcn_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RED = 64
SENTINEL = 0x5EA1DEAD
SEED, SITE = 0x51F15EED, 3
SLOPE = R.SLOPE
RATIOS = {}


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


def guarded(n, off=0, fill=None):
    """-> (buffer, view of n floats at float offset RED + off): sentinel everywhere else, NaN (or `fill`) inside."""
    buf = torch.empty(RED + off + n + RED, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(SENTINEL)
    out = buf[RED + off:RED + off + n]
    if fill is None:
        out.fill_(float("nan"))
    else:
        out.copy_(fill.reshape(-1))
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


def within(entry, got, ref64, bound):
    """'' if |got - ref64| <= bound everywhere, else a description; records the largest error / bound ratio of `entry`."""
    ref64, bound = ref64.reshape(-1), bound.reshape(-1)
    err = (got.double().cpu().reshape(-1) - ref64).abs()
    pos = bound > 0
    if bool(pos.any()):
        RATIOS[entry] = max(RATIOS.get(entry, 0.0), float((err[pos] / bound[pos]).max()))
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        return f"{entry}: {int(bad.sum())} elements out of bound; first flat index {i}: err {float(err[i]):.3e} > {float(bound[i]):.3e}"
    return ""


def report(*entries):
    for e in entries:
        print("gat_heads_ratio", e, f"{RATIOS.get(e, 0.0):.4f}")


class Outs:
    """Named guarded outputs of one call."""

    def __init__(self, **sizes):
        self.buf, self.out, self.off = {}, {}, {}
        for k, v in sizes.items():
            n, off, fill = v if isinstance(v, tuple) else (v, 0, None)
            self.buf[k], self.out[k] = guarded(n, off, fill)
            self.off[k] = off

    def ptr(self, k):
        return self.out[k].data_ptr()

    def clean(self):
        """Red zones intact and no NaN left: -> the name of the first output that fails, or ''."""
        for k, o in self.out.items():
            if not red_zones_intact(self.buf[k], o.numel(), self.off[k]):
                return f"red zone of {k}"
            if bool(torch.isnan(o).any()):
                return f"NaN in {k}"
        return ""

    def same(self, other):
        return all(torch.equal(self.out[k], other.out[k]) for k in self.out)

    def cpu(self, k, *shape):
        return self.out[k].cpu().view(*shape)


def poisoned(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV).fill_(0xFF)


# ------------------------------------------------------------------------------------------------ the per-row family
@pytest.mark.parametrize("case", R.ROW_CASES, ids=lambda c: c["name"])
def test_row_family_vs_fp64(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    chk, st = ops._lib.check, ops._stream()
    N, K = case["N"], case["K"]
    gr = R.case_graph(case)
    x = R.row_inputs(gr)
    n = gr["n"]
    ptr, src, eid = gr["ptr"], gr["col"], gr["eid"]
    csr = [t.to(DEV) for t in (ptr, src, eid)]
    cp = [t.data_ptr() for t in csr]
    d = {k: v.to(DEV) for k, v in x.items()}
    self_eid = eid[:n].long()[src[:n].long() == G.rows_of(ptr)]
    assert self_eid.numel() >= 3
    assert L.sgs_gat_heads_variant(R.OP_ROW, N, K, 1, 1) == case["code"]                                    # 1
    for p in (0.0, R.P_DROP):
        keep_e = ops.dropout_keep(SEED, SITE, n, K, p, DEV).cpu() if p else None
        keep_l = ops.dropout_keep(SEED, SITE + 1, N, K, p, DEV).cpu() if p else None
        for edge in (False, True):
            tag = f"{case['name']} p={p} edge={edge}"
            fname = "sgs_gat_alpha_heads_edge_fwd" if edge else "sgs_gat_alpha_heads_fwd"

            def fwd():
                o = Outs(soft=n * K, soft_loop=N * K, alpha=n * K, alpha_loop=N * K, **(dict(loop_w=N, loop_inv_cnt=N) if edge else {}))
                tail = [SLOPE, p, SEED, SITE, o.ptr("soft"), o.ptr("soft_loop"), o.ptr("alpha"), o.ptr("alpha_loop")]
                if edge:
                    chk(L.sgs_gat_alpha_heads_edge_fwd(d["a_s"].data_ptr(), d["a_d"].data_ptr(), d["w"].data_ptr(), d["coef"].data_ptr(), N, K, n, *cp,
                                                       *tail, o.ptr("loop_w"), o.ptr("loop_inv_cnt"), st), fname)
                else:
                    chk(L.sgs_gat_alpha_heads_fwd(d["a_s"].data_ptr(), d["a_d"].data_ptr(), N, K, n, *cp, *tail, st), fname)
                torch.cuda.synchronize()
                return o
            o = fwd()
            assert not o.clean(), f"{tag}: {o.clean()}"                                                     # 2, 3
            ekw = dict(edge_w=x["w"], coef=x["coef"], loop_w=o.cpu("loop_w", N)) if edge else {}
            ref = R.alpha_fwd(x["a_s"], x["a_d"], ptr, src, eid, K, **ekw)
            bs, bl = R.soft_bound(ref, ptr, src, eid)
            soft, soft_loop = o.cpu("soft", n, K), o.cpu("soft_loop", N, K)
            msg = within(fname, soft, ref["soft"], bs) or within(fname, soft_loop, ref["soft_loop"], bl)   # 4
            if edge:
                msg = msg or within(fname + ":loop_w", o.cpu("loop_w", N), ref["loop_w"], ref["loop_w_bound"])
                msg = msg or within(fname + ":loop_w", o.cpu("loop_inv_cnt", N), ref["loop_inv_cnt"], ref["loop_inv_cnt_bound"])
            assert not msg, f"{tag}: {msg}"
            assert torch.equal(o.cpu("alpha", n, K), R.alpha_of(soft, keep_e, p)), tag                      # 5: exact given soft and the mask
            assert torch.equal(o.cpu("alpha_loop", N, K), R.dropped(soft_loop, keep_l, p)), tag
            assert bool((soft[self_eid] == 0).all()) and bool((o.cpu("alpha", n, K)[self_eid] == 0).all()), tag
            assert o.same(fwd()), tag                                                                       # 6

            # backward, judged on its own: soft from the fp64 forward rounded to fp32, seeded gradients
            s32, l32 = ref["soft"].float(), ref["soft_loop"].float()
            bname = "sgs_gat_alpha_heads_edge_bwd" if edge else "sgs_gat_alpha_heads_bwd"
            lw32, ic32 = (ref["loop_w"].float(), ref["loop_inv_cnt"].float()) if edge else (None, None)
            dw_add = x["dw_add"] if (edge and p) else None
            ins = [t.to(DEV) for t in (s32, l32)]
            einp = [t.to(DEV) for t in (lw32, ic32)] if edge else []

            def bwd():
                o = Outs(g_edge=n * K, g_selfloop=N * K, d_a_dst=N * K, **(dict(d_edge_w=n, d_edge_coef=K) if edge else {}))
                mid = [N, K, n, *cp, SLOPE, p, SEED, SITE, ins[0].data_ptr(), ins[1].data_ptr(), d["galpha"].data_ptr(), d["gloop"].data_ptr()]
                if edge:
                    ws = poisoned(L.sgs_gat_alpha_heads_edge_bwd_workspace_bytes(N, K))
                    chk(L.sgs_gat_alpha_heads_edge_bwd(d["a_s"].data_ptr(), d["a_d"].data_ptr(), d["w"].data_ptr(), d["coef"].data_ptr(),
                                                       einp[0].data_ptr(), einp[1].data_ptr(), *mid, dptr(d["dw_add"] if dw_add is not None else None),
                                                       o.ptr("g_edge"), o.ptr("g_selfloop"), o.ptr("d_a_dst"), o.ptr("d_edge_w"), o.ptr("d_edge_coef"),
                                                       ws.data_ptr(), ws.numel(), st), bname)
                else:
                    chk(L.sgs_gat_alpha_heads_bwd(d["a_s"].data_ptr(), d["a_d"].data_ptr(), *mid, o.ptr("g_edge"), o.ptr("g_selfloop"),
                                                  o.ptr("d_a_dst"), st), bname)
                torch.cuda.synchronize()
                return o
            o = bwd()
            assert not o.clean(), f"{tag}: {o.clean()}"
            bkw = dict(edge_w=x["w"], coef=x["coef"], loop_w=lw32, loop_inv_cnt=ic32, dw_add=dw_add) if edge else {}
            bref = R.alpha_bwd(x["a_s"], x["a_d"], ptr, src, eid, K, s32, l32, x["galpha"], x["gloop"], R.SLOPE, keep_e, keep_l, p, bounds=True, **bkw)
            shapes = dict(g_edge=(n, K), g_selfloop=(N, K), d_a_dst=(N, K), d_edge_w=(n,), d_edge_coef=(K,))
            for k in o.out:
                msg = within(f"{bname}:{k}", o.cpu(k, *shapes[k]), bref[k], bref[k + "_bound"])
                assert not msg, f"{tag}: {msg}"
            assert bool((o.cpu("g_edge", n, K)[self_eid] == 0).all()), tag
            if edge and dw_add is None:
                assert bool((o.cpu("d_edge_w", n)[self_eid] == 0).all()), tag
            assert o.same(bwd()), tag
        # the by-row sum over the same CSR, with and without the loop term
        for gs in (None, "g_self"):
            def esum():
                o = Outs(out=N * K)
                chk(L.sgs_edge_sum_by_row_heads(d["galpha"].data_ptr(), dptr(d[gs]) if gs else None, N, K, n, cp[0], cp[2], o.ptr("out"), st),
                    "sgs_edge_sum_by_row_heads")
                torch.cuda.synchronize()
                return o
            o = esum()
            assert not o.clean(), f"{case['name']}: {o.clean()}"
            g_self = x[gs] if gs else None
            msg = within("sgs_edge_sum_by_row_heads", o.cpu("out", N, K), R.edge_sum_by_row(x["galpha"], g_self, ptr, eid),
                         R.edge_sum_by_row_bound(x["galpha"], g_self, ptr, eid))
            assert not msg, f"{case['name']} g_self={gs}: {msg}"
            assert o.same(esum())
    report("sgs_gat_alpha_heads_fwd", "sgs_gat_alpha_heads_edge_fwd", "sgs_gat_alpha_heads_edge_fwd:loop_w",
           *[f"sgs_gat_alpha_heads_bwd:{k}" for k in ("g_edge", "g_selfloop", "d_a_dst")],
           *[f"sgs_gat_alpha_heads_edge_bwd:{k}" for k in ("g_edge", "g_selfloop", "d_a_dst", "d_edge_w", "d_edge_coef")], "sgs_edge_sum_by_row_heads")



# ------------------------------------------------------------------------------------------------ node scores
@pytest.mark.parametrize("case", R.SCORES_FWD_CASES, ids=lambda c: c["name"])
def test_scores_fwd_vs_fp64(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    N, K, C = case["N"], case["K"], case["C"]
    x = R.scores_inputs(case)
    xl, att_s, att_d = shifted(x["xl"], 0), shifted(x["att_s"], case["att_off"]), shifted(x["att_d"], case["att_off"])
    assert L.sgs_gat_heads_variant(R.OP_SCORES_FWD, N, K, C, aligned16(xl, att_s, att_d)) == case["code"]  # 1

    def run():
        o = Outs(a_s=N * K, a_d=N * K)
        ops._lib.check(L.sgs_gat_scores_heads_fwd(xl.data_ptr(), N, K, C, att_s.data_ptr(), att_d.data_ptr(), o.ptr("a_s"), o.ptr("a_d"),
                                                  ops._stream()), "sgs_gat_scores_heads_fwd")
        torch.cuda.synchronize()
        return o
    o = run()
    assert not o.clean(), o.clean()                                                                         # 2, 3
    refs, bds = R.scores_fwd(x["xl"], x["att_s"], x["att_d"], K, C), R.scores_fwd_bound(x["xl"], x["att_s"], x["att_d"], K, C)
    for k, r, b in zip(("a_s", "a_d"), refs, bds):
        msg = within("sgs_gat_scores_heads_fwd", o.cpu(k, N, K), r, b)                                      # 4
        assert not msg, f"{case['name']}: {msg}"
    assert o.same(run())                                                                                    # 6
    report("sgs_gat_scores_heads_fwd")


@pytest.mark.parametrize("case", R.SCORES_BWD_CASES, ids=lambda c: c["name"])
def test_scores_bwd_vs_fp64(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    N, K, C = case["N"], case["K"], case["C"]
    D = K * C
    x = R.scores_inputs(case)
    d = {k: v.to(DEV) for k, v in x.items()}
    assert L.sgs_gat_heads_variant(R.OP_SCORES_BWD, N, K, C, 1) == case["code"]                             # 1
    for acc in (0, 1):
        def run():
            o = Outs(dxl=(N * D, 0, x["dxl0"] if acc else None), datt_s=D, datt_d=D)
            ws = poisoned(L.sgs_gat_scores_heads_bwd_workspace_bytes(N, K, C))
            ops._lib.check(L.sgs_gat_scores_heads_bwd(d["xl"].data_ptr(), N, K, C, d["att_s"].data_ptr(), d["att_d"].data_ptr(), d["g_s"].data_ptr(),
                                                      d["g_d"].data_ptr(), acc, o.ptr("dxl"), o.ptr("datt_s"), o.ptr("datt_d"), ws.data_ptr(),
                                                      ws.numel(), ops._stream()), "sgs_gat_scores_heads_bwd")
            torch.cuda.synchronize()
            return o
        o = run()
        tag = f"{case['name']} accumulate={acc}"
        assert not o.clean(), f"{tag}: {o.clean()}"                                                         # 2, 3
        a = (x["xl"], x["att_s"], x["att_d"], x["g_s"], x["g_d"], K, C, x["dxl0"] if acc else None)
        refs, bds = R.scores_bwd(*a), R.scores_bwd_bound(*a, rows_per_wg=case["rpw"])
        for k, sh, r, b in zip(("dxl", "datt_s", "datt_d"), ((N, D), (D,), (D,)), refs, bds):
            msg = within("sgs_gat_scores_heads_bwd:" + ("dxl" if k == "dxl" else "d_att"), o.cpu(k, *sh), r, b)      # 4
            assert not msg, f"{tag}: {msg}"
        assert o.same(run()), tag                                                                           # 6
    report("sgs_gat_scores_heads_bwd:dxl", "sgs_gat_scores_heads_bwd:d_att")


# ------------------------------------------------------------------------------------------------ SpMM / SDDMM per head
@pytest.mark.parametrize("case", R.SPMM_CASES, ids=lambda c: c["name"])
def test_spmm_heads_vs_fp64(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    N, K, C, mode = case["N"], case["K"], case["C"], case["mode"]
    gr = R.case_graph(case)
    n = gr["n"]
    a = (gr["ptr"], gr["col"], gr["eid"])
    cp = [t.to(DEV) for t in a]
    val, diag_d = gr["val"].to(DEV), gr["diag"].to(DEV)
    W = C if mode == R.MEAN else K * C
    yoff = 1 if case["align"] == "y" else 0
    walk = case["code"] // 1000000 == R.K_MEAN_WALK
    entry = f"sgs_spmm_csr_heads:{R._KIND_NAME[case['code'] // 1000000]}"
    for diag_on, bias_on, act in (R.SPMM_EPI_COMBOS if case["epi"] else R.SPMM_COMBOS):
        drop = act == G.ACT_RELU_DROPOUT
        X, bias = R.spmm_x(case, drop)
        diag, bias = (gr["diag"] if diag_on else None), (bias if bias_on else None)
        Xd = shifted(X, 1 if case["align"] == "x" else 0)
        bd = None if bias is None else bias.to(DEV)
        tag = f"{case['name']} diag={diag_on} bias={bias_on} act={act}"

        def run():
            o = Outs(Y=(N * W, yoff, None))
            ops._lib.check(L.sgs_spmm_csr_heads(Xd.data_ptr(), N, K, C, n, cp[0].data_ptr(), cp[1].data_ptr(), cp[2].data_ptr(), val.data_ptr(),
                                                diag_d.data_ptr() if diag_on else None, mode, dptr(bd), act, R.P_DROP if drop else 0.0, SEED, SITE,
                                                o.ptr("Y"), ops._stream()), "sgs_spmm_csr_heads")
            torch.cuda.synchronize()
            return o
        o = run()
        assert L.sgs_gat_heads_variant(R.SPMM_OP[mode], N, K, C, aligned16(Xd, o.out["Y"])) == case["code"], tag       # 1
        assert not o.clean(), f"{tag}: {o.clean()}"                                                         # 2, 3
        Y = o.cpu("Y", N, W)
        keep = ops.dropout_keep(SEED, SITE, N, W, R.P_DROP, DEV).cpu() if drop else None
        Z = R.spmm_heads_pre(*a, gr["val"], diag, bias, X.double(), K, C, mode)
        pb = R.spmm_heads_pre_bound(*a, gr["val"], diag, bias, X, K, C, mode, walk)
        Yref = G.activate(Z, act, keep, R.P_DROP)
        msg = within(entry, Y, Yref, G.spmm_bound(pb, Yref, act, R.P_DROP))                                 # 4
        assert not msg, f"{tag}: {msg}"
        if drop:            # 5: the kept set, wherever the output can show it (gcn_ref.ambiguous; capped on the reference alone)
            amb = G.ambiguous(Z, pb)
            assert float(amb.double().mean()) <= G.MAX_AMBIGUOUS, tag
            assert torch.equal((Y != 0)[~amb], keep[~amb]), tag
        assert o.same(run()), tag                                                                           # 6
    report(entry)


@pytest.mark.parametrize("case", R.SDDMM_CASES, ids=lambda c: c["name"])
def test_sddmm_heads_vs_fp64(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    N, K, C = case["N"], case["K"], case["C"]
    gr = R.case_graph(case)
    n = gr["n"]
    a = (gr["ptr"], gr["col"], gr["eid"])
    cp = [t.to(DEV) for t in a]
    for bc in (0, 1):
        A, B = R.sddmm_ab(case, bool(bc))
        Ad, Bd = shifted(A, 1 if case["align"] == "a" else 0), shifted(B, 1 if case["align"] == "b" else 0)
        tag = f"{case['name']} broadcast={bc}"
        want = case["code_bcast"] if bc else case["code"]
        assert L.sgs_gat_heads_variant(R.OP_SDDMM_BROADCAST if bc else R.OP_SDDMM, N, K, C, aligned16(Ad, Bd)) == want, tag    # 1

        def run():
            o = Outs(g=n * K, gdiag=N * K)
            ops._lib.check(L.sgs_sddmm_csr_heads(Ad.data_ptr(), Bd.data_ptr(), N, K, C, n, cp[0].data_ptr(), cp[1].data_ptr(), cp[2].data_ptr(), bc,
                                                 o.ptr("g"), o.ptr("gdiag"), ops._stream()), "sgs_sddmm_csr_heads")
            torch.cuda.synchronize()
            return o
        o = run()
        assert not o.clean(), f"{tag}: {o.clean()}"                                                         # 2, 3: every eid slot written
        refs, bds = R.sddmm_heads(*a, A.double(), B.double(), K, C, bool(bc)), R.sddmm_heads_bound(*a, A, B, K, C, bool(bc))
        entry = "sgs_sddmm_csr_heads" + (":broadcast" if bc else "")
        msg = within(entry, o.cpu("g", n, K), refs[0], bds[0]) or within(entry, o.cpu("gdiag", N, K), refs[1], bds[1])      # 4
        assert not msg, f"{tag}: {msg}"
        assert o.same(run()), tag                                                                           # 6
    report("sgs_sddmm_csr_heads", "sgs_sddmm_csr_heads:broadcast")
