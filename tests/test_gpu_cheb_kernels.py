"""GPU: every kernel variant behind sgs_cheb_spmm, and sgs_cheb_norm_fwd / sgs_cheb_norm_bwd (section K9 of include/sgs_hip.h), against
the fp64 references of tests/cheb_kernels_ref.py, through the C ABI.  The case tables live in cheb_kernels_ref.py;
tests/test_cheb_variant_table.py proves on the CPU that they reach every code sgs_cheb_spmm_variant can return, straddle every threshold,
and that the bounds see single planted faults.

Calling convention of tests/test_gpu_gat_heads_kernels.py and tests/test_gpu_gatv2_gine_kernels.py (their helpers are imported): every
buffer a call may write is carved from a larger one with 64 sentinel words on each side; a block-strided output is the column block of a
whole carved [N, ld] buffer whose target block is pre-filled with NaN and whose every other column holds inputs or the sentinel, and the
whole buffer outside the target block is compared bitwise with its state before the call; inputs sit at the case's float offset; the
workspace is sized exactly to its query and sits in a red zone of its own.  Each case asserts, in order: the variant code, the red zones
and untouched columns, no NaN, |got - ref64| <= the a-priori bound ELEMENT BY ELEMENT, the exact relations (Y2 = fp32(scale2 * Y) of the
kernel's own Y; the kept set of the exported dropout mask; in place = out of place; aligned against unaligned operands; the zeros of
(i, i) edges and of nodes without out-weight; l_in = l_out; unit weights = a vector of ones), and bitwise equality of a second call.  The
largest error / bound ratio per compared quantity is printed ("cheb_ratio")."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheb_kernels_ref as R  # noqa: E402
import gcn_ref as G  # noqa: E402
from gat_heads_ref import csr_of  # noqa: E402
from test_gpu_gat_heads_kernels import DEV, RATIOS, RED, SEED, SENTINEL, SITE, Outs, dptr, guarded, red_zones_intact, shifted, within  # noqa: E402,F401
from test_gpu_gatv2_gine_kernels import Workspace, padded_i32, untouched  # noqa: E402
from test_gpu_gcn_variants import GOLD  # noqa: E402

pytestmark = pytest.mark.gpu
K_ANY = 3            # the order is only validated by sgs_cheb_spmm: the step does not depend on it


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


def report(prefix):
    for e in sorted(RATIOS):
        if e.startswith(prefix):
            print("cheb_ratio", e, f"{RATIOS[e]:.4f}")


class Buf:
    """An [N, ld] float buffer carved from a guarded one at float offset `off`: `host` ([N, <= ld]) in its leading columns, the sentinel
    in every other word."""

    def __init__(self, host, N, ld, off):
        self.n, self.off = N * ld, off
        self.buf, flat = guarded(N * ld, off)
        flat.view(torch.int32).fill_(SENTINEL)
        self.v = flat.view(N, ld)
        if host is not None:
            self.v[:, :host.shape[1]].copy_(host)
        self.ld, self.snap, self.written = ld, None, []

    def block(self, blk, D):
        return self.v[:, blk * D:(blk + 1) * D]

    def ptr(self, blk, D):
        return self.v.data_ptr() + 4 * blk * D

    def target(self, blk, D, nan=True):
        """Declare block `blk` an output of the call (pre-filled with NaN unless it is also the add operand)."""
        if nan:
            self.block(blk, D).fill_(float("nan"))
        self.written.append((blk, D))

    def freeze(self):
        self.snap = self.buf.clone()

    def unchanged_outside_targets(self):
        """Red zones, padding columns and every block that is not a declared output: bitwise what they were before the call."""
        now = self.buf.clone()
        inner = slice(RED + self.off, RED + self.off + self.n)
        nv, sv = now[inner].view(self.v.shape), self.snap[inner].view(self.v.shape)
        for blk, D in self.written:
            nv[:, blk * D:(blk + 1) * D] = sv[:, blk * D:(blk + 1) * D]
        return torch.equal(now.view(torch.int32), self.snap.view(torch.int32)) and red_zones_intact(self.buf, self.n, self.off)


def run_step(pkg, case, combo, dev, x, xoff=None, ldpad=None, yoff=None, in_place=True):
    """One sgs_cheb_spmm call of `combo` on the case's buffers -> dict(code, Y, Y2, bufs).  xoff / ldpad / yoff default to the case's;
    in_place=False passes a copy of the add operand in a buffer of its own instead of Y itself."""
    L, ops = pkg._lib.lib(), pkg.ops
    N, D, n = case["N"], case["D"], case["nnz"]
    xoff, ldpad, yoff = (case[k] if v is None else v for k, v in (("xoff", xoff), ("ldpad", ldpad), ("yoff", yoff)))
    own_x = yoff != 0                                        # Y, add, sub moved: X stays in an aligned buffer of its own
    xkey = combo["X"][0] + ("@x" if own_x else "")
    bufs = {}

    def buf(name, key=None):
        key = key or name
        if key not in bufs:
            off, pad = (xoff, ldpad) if key == xkey else (yoff, 0)
            bufs[key] = Buf(x.get(name), N, R.WIDTH[name] * D + pad, off)
        return bufs[key]

    def arg(spec, key=None):
        if spec is None:
            return None, 0
        b = buf(spec[0], key)
        return b.ptr(spec[1], D), b.ld
    Xp, ldx = arg(combo["X"], xkey)
    aliased = combo["add"] is not None and combo["add"] == combo["Y"]
    addp, ldadd = arg(combo["add"], None if (in_place or not aliased) else combo["add"][0] + "@add")
    subp, ldsub = arg(combo["sub"])
    Yp, ldy = arg(combo["Y"])
    buf(combo["Y"][0]).target(combo["Y"][1], D, nan=not (aliased and in_place))
    a2 = buf("A")                                            # the Y2 buffer exists in every call: a NULL Y2 must leave it alone
    y2 = combo["Y2"]
    if y2 is not None:
        a2.target(y2[1], D)
    drop = combo["act"] == R.ACT_RELU_DROPOUT
    bias = None if not combo["bias"] else x["bias_drop" if drop else "bias"].to(DEV)
    for b in bufs.values():
        b.freeze()
    al = int(Xp % 16 == 0)
    code = L.sgs_cheb_spmm_variant(N, D, n, ldx, al)
    ops._lib.check(L.sgs_cheb_spmm(K_ANY, Xp, ldx, N, D, n, dev["ptr"].data_ptr(), dptr(dev["col"]), dptr(dev["val"]), float(combo["alpha"]), addp,
                                   ldadd, subp, ldsub, dptr(bias), combo["act"], R.P_DROP if drop else 0.0, SEED, SITE, Yp, ldy,
                                   a2.ptr(y2[1], D) if y2 else None, a2.ld if y2 else 0, float(combo["scale2"]), ops._stream()), "sgs_cheb_spmm")
    torch.cuda.synchronize()
    return dict(code=code, bufs=bufs, ldx=ldx, al=al, Y=buf(combo["Y"][0]).block(combo["Y"][1], D).cpu(), Y2=a2.block(y2[1], D).cpu() if y2 else None)


def check_step_case(pkg, case, combos):
    ops = pkg.ops
    N, D, n = case["N"], case["D"], case["nnz"]
    gr = R.case_graph(case)
    dev = dict(ptr=gr["ptr"].to(DEV), col=gr["col"].to(DEV) if n else None, val=gr["val"].to(DEV) if n else None)     # nnz = 0: NULL col, val
    x = R.step_inputs(case)
    entry = f"cheb_spmm:{'rowblock' if case['code'] >= 1000 else 'rows'}_v{case['code'] // 100 % 10}"
    for combo in combos:
        tag = f"{case['name']} {combo['name']}"
        act, drop = combo["act"], combo["act"] == R.ACT_RELU_DROPOUT
        r = run_step(pkg, case, combo, dev, x)
        assert (r["ldx"], r["al"]) == R.x_layout(case, combo), tag          # the layout the CPU table asked the query about
        assert r["code"] == case["code"], tag                                                               # 1
        for k, b in r["bufs"].items():
            assert b.unchanged_outside_targets(), f"{tag}: buffer {k} changed outside the written block"   # 2 (a NULL Y2: all of A)
        Y, Y2 = r["Y"], r["Y2"]
        assert not bool(torch.isnan(Y).any()) and (Y2 is None or not bool(torch.isnan(Y2).any())), tag      # 3
        X, add, sub, bias = R.combo_operands(case, combo, x)
        a = (gr["ptr"], gr["col"], gr["val"], X, combo["alpha"], add, sub, bias)
        Z, pb = R.step_pre(*a), R.step_pre_bound(*a)
        keep = ops.dropout_keep(SEED, SITE, N, D, R.P_DROP, DEV).cpu() if drop else None
        Yref = G.activate(Z, act, keep, R.P_DROP)
        bound = G.spmm_bound(pb, Yref, act, R.P_DROP)
        msg = within(entry, Y, Yref, bound)                                                                 # 4
        assert not msg, f"{tag}: {msg}"
        if Y2 is not None:                                                                                  # 5: exact relations
            assert torch.equal(Y2, Y * torch.tensor(combo["scale2"], dtype=torch.float32)), tag
        if drop:
            amb = G.ambiguous(Z, pb)
            assert float(amb.double().mean()) <= G.MAX_AMBIGUOUS, tag
            assert torch.equal((Y != 0)[~amb], keep[~amb]), tag
        if combo["add"] is not None and combo["add"] == combo["Y"]:
            r2 = run_step(pkg, case, combo, dev, x, in_place=False)
            assert torch.equal(r2["Y"], Y) and all(b.unchanged_outside_targets() for b in r2["bufs"].values()), f"{tag}: in place != out of place"
        if case["xoff"] or case["ldpad"]:                    # the same inputs with X aligned: another kernel, the same bound
            t = run_step(pkg, case, combo, dev, x, xoff=0, ldpad=0)
            assert t["code"] != case["code"] and t["code"] // 100 % 10 == 4, tag
            msg = within(entry + ":aligned_twin", t["Y"], Yref, bound)
            assert not msg, f"{tag}: {msg}"
        if case["yoff"]:                                     # only Y, add, sub moved: the same kernel, the same bits
            t = run_step(pkg, case, combo, dev, x, yoff=0)
            assert t["code"] == case["code"] and torch.equal(t["Y"], Y), tag
        again = run_step(pkg, case, combo, dev, x)                                                          # 6
        assert torch.equal(again["Y"], Y) and (Y2 is None or torch.equal(again["Y2"], Y2)), tag
    report("cheb_spmm")


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: c["name"])
def test_step_variant_vs_fp64(pkg, case):
    check_step_case(pkg, case, R.STEP_COMBOS)


@pytest.mark.parametrize("name", ["lanes_v4_lpr16_D64", "rb_v1_nw4_N67_D41_at16N"])
def test_step_dropout_mask_follows_the_epoch_buffer(pkg, name):
    """Both forms compute the mask from dropout_row_key + dropout_keep_col; under a registered non-zero epoch the kept set is
    sgs_dropout_keep's under the same epoch, which is the epoch-free mask of seed + epoch * 2^64 / phi."""
    ops = pkg.ops
    case = next(c for c in R.STEP_CASES if c["name"] == name)
    N, D = case["N"], case["D"]
    base = ops.dropout_keep(SEED, SITE, N, D, R.P_DROP, DEV)
    shifted_seed = ops.dropout_keep((SEED + 5 * GOLD) % (1 << 64), SITE, N, D, R.P_DROP, DEV)
    epoch = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    try:
        ops.set_rng_epoch_buffer(epoch)
        k5 = ops.dropout_keep(SEED, SITE, N, D, R.P_DROP, DEV)
        check_step_case(pkg, case, [R.DROP_COMBO])
        torch.cuda.synchronize()
    finally:
        ops.set_rng_epoch_buffer(None)
    assert torch.equal(k5, shifted_seed) and not torch.equal(k5, base)


# ------------------------------------------------------------------------------------------------ the normalisation
def _by_eid(eid, v, n):
    out = torch.full((n,), float("nan"))
    out[eid] = v
    return out


@pytest.mark.parametrize("case", R.NORM_CASES, ids=lambda c: c["name"])
def test_norm_fwd_bwd_vs_fp64(pkg, case):
    L, ops = pkg._lib.lib(), pkg.ops
    chk, st = ops._lib.check, ops._stream()
    ei, N, n = case["ei"], case["N"], case["n"]
    in_ptr, in_src, in_eid = csr_of(ei[1], ei[0], N)
    out_ptr, out_dst, out_eid = csr_of(ei[0], ei[1], N)
    csr = [t.to(DEV) for t in (in_ptr.int(), padded_i32(in_src), padded_i32(in_eid), out_ptr.int(), padded_i32(out_dst), padded_i32(out_eid))]
    cp = [t.data_ptr() for t in csr]
    eid_d = ei.to(DEV)
    self_e = ei[0] == ei[1]
    g, g2 = R.norm_grads(case)
    gd, g2d = g.to(DEV), g2.to(DEV)
    ones = torch.ones(max(n, 1), device=DEV)
    for mode in R.WEIGHT_MODES:
        tag = f"{case['name']} {mode}"
        w = R.norm_weights(case, mode)
        wd = None if w is None else w.to(DEV)

        def fwd(wp):
            o = Outs(dis=N, l_in=n, l_out=n)
            chk(L.sgs_cheb_norm_fwd(dptr(wp), n, N, *cp, o.ptr("dis"), o.ptr("l_in"), o.ptr("l_out"), st), "sgs_cheb_norm_fwd")
            torch.cuda.synchronize()
            return o
        o = fwd(wd)
        assert not o.clean(), f"{tag}: {o.clean()}"                                                         # 2, 3
        dis64, _ = R.norm_fwd(ei, w, N)
        dis = o.cpu("dis", N)
        msg = within("cheb_norm_fwd:dis", dis, dis64, R.dis_bound(ei, N, dis64))                            # 4
        assert not msg, f"{tag}: {msg}"
        l_e, l_o = _by_eid(in_eid, o.cpu("l_in", n), n), _by_eid(out_eid, o.cpu("l_out", n), n)
        lref = R.l_of_dis(ei, w, dis)                        # given the kernel's own dis
        msg = within("cheb_norm_fwd:l", l_e, lref, R.l_bound(lref))
        assert not msg, f"{tag}: {msg}"
        assert torch.equal(l_e, l_o) and bool((l_e[self_e] == 0).all()) and bool((dis[dis64 == 0] == 0).all()), tag      # 5
        if case["zero_node"] is not None and w is not None:
            assert float(dis[case["zero_node"]]) == 0.0 and bool((l_e[ei[0] == case["zero_node"]] == 0).all()), tag
        assert o.same(fwd(wd)), tag                                                                         # 6
        if w is None:
            assert o.same(fwd(ones)), f"{tag}: w == NULL is not a vector of ones"

        # the backward, judged on its own inputs: dis from the fp64 forward rounded to fp32
        d32 = dis64.float()
        d32d = d32.to(DEV)
        w1 = ones if wd is None else wd
        for second in (None, g2):
            btag = f"{tag} g2={second is not None}"

            def bwd():
                o = Outs(dw=n)
                ws = Workspace(L.sgs_cheb_norm_bwd_workspace_bytes(N))
                chk(L.sgs_cheb_norm_bwd(w1.data_ptr(), gd.data_ptr(), None if second is None else g2d.data_ptr(), n, N, d32d.data_ptr(), *cp,
                                        eid_d.data_ptr(), o.ptr("dw"), *ws.args(), st), "sgs_cheb_norm_bwd")
                torch.cuda.synchronize()
                assert ws.intact(), f"{btag}: red zone of the workspace"
                return o
            o = bwd()
            assert not o.clean(), f"{btag}: {o.clean()}"
            ref, _, _, dwb = R.norm_bwd(ei, w, g, second, d32, N, bounds=True)
            dw = o.cpu("dw", n)
            msg = within("cheb_norm_bwd:dw", dw, ref, dwb)
            assert not msg, f"{btag}: {msg}"
            assert bool((dw[self_e] == 0).all()) and bool((dw[d32[ei[0]] == 0] == 0).all()), btag
            assert o.same(bwd()), btag
    report("cheb_norm")


# ------------------------------------------------------------------------------------------------ error paths (no launch)
def test_error_paths_report_and_write_nothing(pkg):
    L, ops = pkg._lib.lib(), pkg.ops
    st = ops._stream()
    N, D = 8, 4
    o = Outs(Y=N * D, Y2=N * D, dw=N)
    X = torch.ones(N * D, device=DEV)
    i32 = torch.zeros(N + 1 + G.PAD, dtype=torch.int32, device=DEV)
    ei = torch.zeros(2, N, dtype=torch.int64, device=DEV)
    fp, ip = X.data_ptr(), i32.data_ptr()

    def spmm(K, Xp, Yp, ldy):
        return L.sgs_cheb_spmm(K, Xp, D, N, D, 0, ip, None, None, 1.0, None, 0, None, 0, None, 0, 0.0, SEED, SITE, Yp, ldy, o.ptr("Y2"), D, 1.0, st)
    for K in (0, 9):
        assert spmm(K, fp, o.ptr("Y"), D) == -1 and b"unsupported" in L.sgs_last_error()
    assert spmm(3, fp, o.ptr("Y"), D - 1) == -1 and b"leading dimension" in L.sgs_last_error()               # SGS_EINVAL
    assert spmm(3, o.ptr("Y"), o.ptr("Y"), D) == -1 and b"aliased" in L.sgs_last_error()
    assert spmm(3, o.ptr("Y2"), o.ptr("Y"), D) == -1 and b"aliased" in L.sgs_last_error()                    # X == Y2
    ws = Workspace(L.sgs_cheb_norm_bwd_workspace_bytes(N))
    assert L.sgs_cheb_norm_bwd(fp, fp, None, N, N, fp, ip, ip, ip, ip, ip, ip, ei.data_ptr(), o.ptr("dw"), ws.out.data_ptr(), ws.nbytes - 1,
                               st) == -2 and b"workspace" in L.sgs_last_error()                             # SGS_EWORKSPACE
    torch.cuda.synchronize()
    assert untouched(o) and ws.intact() and bool(torch.isnan(ws.out).all())
