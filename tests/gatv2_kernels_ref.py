"""fp64 restatement of the contracts of the GATv2 entry points (section K8c of include/sgs_hip.h: sgs_gatv2_alpha_heads_fwd,
sgs_gatv2_alpha_heads_bwd with gatv2_param_finish, sgs_gatv2_dxl_heads), the first-order fp32 error bounds the GPU results are held to
ELEMENT BY ELEMENT, the launch geometry restated from csrc/gatv2.hip's geom(), graph builders with chosen rows, and the case tables of
tests/test_gpu_gatv2_gine_kernels.py (checked on the CPU by tests/test_gatv2_gine_variant_table.py).  Plain torch on the CPU; nothing here
imports the product.  Every reference takes the fp32 inputs the kernel gets; `dt` = float32 evaluates the same formulas in fp32 and `mut`
plants one fault (both for the CPU test only).  With fp64 inputs the same functions are the plain fp64 formulas (the composition check).

The leaky_relu branch is a fact about the fp32 inputs: v2_pre = fmaf(w, le, fp32(xl + xr)), and `pre` reproduces that value: the add in
fp32, then product and sum in fp64 (the product of two fp32 is exact there), rounded once; without the edge term it is the fp32 add.  The
loop's pre-activation uses wbar_i, an fp32 sum the kernel forms in its own order: the reference takes the kernel's OWN loop_w output for it
(loop_w itself is held to its bound).  No element is excluded as "ambiguous".

Bounds (u = 2^-24; nothing in them is measured; M_x = the formula of x on absolute values; n_i = non-loop entries of row i):
  logit      l = sum_c att lrelu(s): the product slope s, C fmas in a lane's chain and the xor tree:   E_l = (C + 3) u sum_c |att| |lrelu(s)|
  softmax    soft = exp(l - m) / (sum exp(l_k - m) + 1e-16f), the sum taken ONLINE: on every entry ssum = ssum expf(m_old - m_new) +
             expf(l - m_new).  A term passes at most n_i + 1 such steps, each an expf (2 EXP_ULPS u), a product and an add:
             (n_i + 1)(2 EXP_ULPS + 2) u; the arguments of the expf chain of a term telescope to l_k - m, each difference rounded in fp32:
             weighted by soft_k they add up to at most u log(n_i + 1) <= n_i u (Gibbs' inequality, the row's largest term being 1);
             the numerator's and the term's own expf: 4 EXP_ULPS u; the numerator's argument fp32(l - m): u |l - m|; the 1e-16 add, the
             reciprocal, the product, +1: 4 u.  The logits are not exported, so their error enters as a perturbation: d soft_e =
             soft_e (d l_e - sum_k soft_k d l_k), at most soft_e 2 max_row E_l.  Together
               |soft - ref| <= ref ([(n_i + 1)(2 EXP_ULPS + 2) + n_i + 4 EXP_ULPS + 4] u + u |l - m| + 2 max_row E_l) + 2^-125
             (2^-125: subnormal or flushed expf results, the row sum being >= 1).  EXP_ULPS = 4 as in loss_ref.py / gat_heads_ref.py.
             loop_w: (cnt + 2) u mean |w|;  loop_inv_cnt: u / cnt;  alpha: EXACT given the kernel's soft and the exported mask.
  backward   with g' = fp32(galpha drop_scale) where kept else 0 (exact), D = sum soft |g'| (loop included):
             E_dot = (n_i + 3) u D;   g = soft (g' - dot):  E_g = soft (E_dot + 3 u (|g'| + D)) + 2^-125,  M_g = soft (|g'| + D)
             t = g att lrelu'(s) (two products):  E_t = E_g |att| sf + 2 u M_t + 2^-125
             (every product of a g that small may underflow, whatever its other factor: 2^-125 per term also in d_att, d_edge_w and dxl)
             d_xr[i]     sum E_t + (n_i + 2) u sum M_t                       the loop and n_i entries in the lane's own order
             d_att       sum E_g |lrelu s| + (L + 4) u sum M_g |lrelu s|     (the product slope s and the fma on top of the chain)
             d_lin_edge  sum E_t |w| + (L + 3) u sum M_t |w|
               L = the longest chain of additions a term can pass: lane-private over the entries and loops of the `iters` rows a lane
               owns, the workgroup's rows-per-pass rows in LDS, gatv2_param_finish's strided adds (ceil(nwg / 16)) and its 16 groups;
               `chain` computes it from the row lengths and the query's (iters, rows per pass, nwg).  Always L <= the number of terms.
             d_edge_w[e] sum_{h, c} |le| (E_t + E_t,loop / cnt) + (K C + 5) u (sum |le| (M_t + M_t,loop / cnt) + |dw_add|)
  dxl        (len_j + 5) u (sum |g att sf| + |d_xl before|) + (len_j + 1) 2^-125     two products per term, len_j + 1 terms, the accumulate"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_heads_ref as H  # noqa: E402
import gcn_ref as G  # noqa: E402
from gat_heads_ref import EXP_ULPS, F32, F64, P_DROP, SLOPE, TINY, U, csr_of, dropped, outside  # noqa: E402,F401

OP_FWD, OP_BWD, OP_DXL = 0, 1, 2
K_MAX_ITERS = 16
# the pointers each launcher tests for 16-byte alignment (lin_edge only with edge_w)
AL16 = {OP_FWD: ("xl", "xr", "att", "lin_edge"), OP_BWD: ("xl", "xr", "att", "lin_edge", "d_xr"), OP_DXL: ("xl", "xr", "att", "lin_edge", "d_xl")}


def cdiv(a, b):
    return -(-a // b)


def log2_ceil(v):
    return max(0, (int(v) - 1).bit_length())


# ------------------------------------------------------------------------------------------------ the launch choice, restated
def geom(N, K, C, vec):
    """csrc/gatv2.hip's geom(), restated: dict(vec, lg, lgG, one, rpp [rows per pass], iters, nwg, gv [channels of a head per chunk])."""
    lgK = log2_ceil(K)
    lgG = min(log2_ceil(cdiv(C, vec)), 6 - lgK)
    lg = lgK + lgG
    rpp = 256 >> lg
    passes = cdiv(max(N, 1), rpp)
    iters = min(max(passes // 2048, 1), K_MAX_ITERS)
    return dict(vec=vec, lg=lg, lgG=lgG, one=int((vec << lgG) >= C), rpp=rpp, iters=iters, nwg=cdiv(passes, iters), gv=vec << lgG)


def code(kind, vec, lg, lgG=0, one=0, iters=0):
    return kind * 1000000 + vec * 100000 + lg * 10000 + lgG * 1000 + one * 100 + iters


def geom_of_code(c, N):
    """The geometry a by-destination code states, for N rows."""
    vec, lg, lgG, one, iters = c // 100000 % 10, c // 10000 % 10, c // 1000 % 10, c // 100 % 10, max(c % 100, 1)
    rpp = 256 >> lg
    return dict(vec=vec, lg=lg, lgG=lgG, one=one, rpp=rpp, iters=iters, nwg=cdiv(cdiv(max(N, 1), rpp), iters), gv=vec << lgG)


def chain(n_live, geo):
    """Longest chain of additions of a d_att / d_lin_edge term (see the module docstring)."""
    N = n_live.numel()
    rpp, iters, nwg = geo["rpp"], geo["iters"], geo["nwg"]
    t = torch.zeros(nwg * iters * rpp, dtype=torch.int64)
    t[:N] = n_live.long() + 1
    return int(t.view(nwg, iters, rpp).sum(1).max()) + rpp + cdiv(nwg, 16) + 16


# ------------------------------------------------------------------------------------------------ references
def _by_eid(e, v):
    out = torch.zeros_like(v)
    out[e] = v
    return out


def pre(xl, xr, s, r, K, C, w=None, le=None):
    """[m, K, C]: the pre-activation of entries (source s, destination r) in the inputs' dtype; fp32: the kernels' value bit for bit."""
    p = xl.reshape(-1, K, C)[s] + xr.reshape(-1, K, C)[r]
    if w is not None:
        if p.dtype == F32:
            p = (w.double()[:, None, None] * le.double().reshape(1, K, C) + p.double()).float()
        else:
            p = p + w[:, None, None] * le.reshape(1, K, C)
    return p


def _sides(p, slope, dt, mut):
    """-> (leaky_relu(p) in dt, leaky_relu'(p) in dt).  mut "slope_side": the slope taken at s > 0."""
    pos = p <= 0 if mut == "slope_side" else p > 0
    sl = torch.tensor(slope, dtype=F32).to(dt)
    pd = p.to(dt)
    return torch.where(pos, pd, pd * sl), torch.where(pos, torch.ones((), dtype=dt), sl)


def _chan_mask(K, C, gv, dt):
    return (torch.arange(C) < gv).to(dt).reshape(1, 1, C)


def alpha_fwd(xl, xr, att, ptr, src, eid, K, C, slope=SLOPE, edge_w=None, lin_edge=None, loop_w=None, dt=F64, mut=None, gv=None, bounds=False):
    """sgs_gatv2_alpha_heads_fwd -> dict soft [n, K] by edge id (0 at (i, i) entries), soft_loop [N, K], n_live [N]; with edge_w: loop_w,
    loop_inv_cnt [N] (fp64) and their bounds; bounds = True: soft_bound, soft_loop_bound.  loop_w: the kernel's own fp32 wbar for the
    loop's pre-activation (None: the mean rounded to the inputs' dtype).  mut: "no_loop_in_sum", "keep_self", "loop_sum_w",
    "skip_chunks" (channels >= gv of a head skipped), "slope_side"."""
    N = ptr.numel() - 1
    n, r, s, e, ok = H._entries(ptr, src, eid)
    if mut == "keep_self":
        ok = torch.ones_like(ok)
    edge = edge_w is not None
    cnt = torch.zeros(N, dtype=F64).index_add_(0, r[ok], torch.ones(int(ok.sum()), dtype=F64))
    out = {"n_live": cnt}
    we = lw = None
    if edge:
        we = edge_w[e]
        wsum = torch.zeros(N, dtype=F64).index_add_(0, r[ok], we[ok].double())
        wabs = torch.zeros(N, dtype=F64).index_add_(0, r[ok], we[ok].double().abs())
        icnt = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0), torch.zeros_like(cnt))
        out.update(loop_w=wsum * icnt, loop_inv_cnt=icnt, loop_w_bound=(cnt + 2) * U * wabs * icnt, loop_inv_cnt_bound=U * icnt)
        lw = out["loop_w"].to(edge_w.dtype) if loop_w is None else loop_w
        if mut == "loop_sum_w":
            lw = wsum.to(edge_w.dtype)
    i = torch.arange(N)
    a = att.to(dt).reshape(1, K, C)
    if mut == "skip_chunks":
        a = a * _chan_mask(K, C, gv, dt)
    lre, _ = _sides(pre(xl, xr, s, r, K, C, we, lin_edge), slope, dt, mut)
    lrl, _ = _sides(pre(xl, xr, i, i, K, C, lw, lin_edge), slope, dt, mut)
    le, ll = (a * lre).sum(-1), (a * lrl).sum(-1)
    idx = r[ok][:, None].expand(-1, K)
    mx = ll.clone().scatter_reduce(0, idx, le[ok], "amax", include_self=True)
    xe, xo = le - mx[r], ll - mx
    ee, el = torch.exp(xe) * ok[:, None].to(dt), torch.exp(xo)
    den = torch.zeros(N, K, dtype=dt).index_add_(0, r, ee)
    if mut != "no_loop_in_sum":
        den = den + el
    if dt == F64:
        den = den + float(np.float32(1e-16))
        se, sl = ee / den[r], el / den
    else:
        inv = 1.0 / (den + torch.tensor(1e-16, dtype=F32))
        se, sl = ee * inv[r], el * inv
    se = torch.where(ok[:, None], se, torch.zeros_like(se))
    out["soft"], out["soft_loop"] = _by_eid(e, se), sl
    if bounds:
        assert dt == F64
        aa = a.abs()
        Ee, El = (C + 3) * U * (aa * lre.abs()).sum(-1), (C + 3) * U * (aa * lrl.abs()).sum(-1)
        Erow = El.clone().scatter_reduce(0, idx, Ee[ok], "amax", include_self=True)
        f = ((cnt + 1) * (2 * EXP_ULPS + 2) + cnt + 4 * EXP_ULPS + 4) * U
        out["soft_bound"] = _by_eid(e, se * (f[r][:, None] + U * xe.abs() + 2 * Erow[r]) + TINY)
        out["soft_loop_bound"] = sl * (f[:, None] + U * xo.abs() + 2 * Erow) + TINY
    return out


def gprime(g, keep, p, mut=None):
    """g' = g drop_scale where kept, else 0: fp32 g -> the kernels' one fp32 multiply, exactly; fp64 g -> g / (1 - p)."""
    if mut == "no_drop_scale" and keep is not None:
        return torch.where(keep.bool(), g, torch.zeros_like(g))
    if g.dtype == F32 or keep is None:
        return dropped(g, keep, p)
    return torch.where(keep.bool(), g / (1.0 - p), torch.zeros_like(g))


def alpha_bwd(xl, xr, att, ptr, src, eid, K, C, soft, soft_loop, galpha, gloop, slope=SLOPE, keep_e=None, keep_l=None, p=0.0, edge_w=None,
              lin_edge=None, loop_w=None, loop_inv_cnt=None, dw_add=None, dt=F64, mut=None, geo=None, bounds=False):
    """sgs_gatv2_alpha_heads_bwd with soft / soft_loop / galpha / gloop (and loop_w / loop_inv_cnt) as INPUTS -> dict g_logit [n, K] by
    edge id, g_loop [N, K], d_xr [N, K C], d_att [K C]; with edge_w: d_lin_edge [K C], d_edge_w [n]; bounds = True adds "<name>_bound".
    geo: geom()'s dict (the faults that need it and the chain length; None: the term count).  mut: "slope_side", "skip_chunks",
    "drop_last_pass" (a workgroup's last row pass missing from d att / d lin_edge), "drop_partial" (one workgroup's partial row missing),
    "no_loop_dw", "no_dw_add", "no_drop_scale"."""
    N = ptr.numel() - 1
    n, r, s, e, ok = H._entries(ptr, src, eid)
    i = torch.arange(N)
    okk = ok[:, None]
    edge = edge_w is not None
    we = edge_w[e] if edge else None
    pe, pl = pre(xl, xr, s, r, K, C, we, lin_edge), pre(xl, xr, i, i, K, C, loop_w if edge else None, lin_edge)
    lre, sfe = _sides(pe, slope, dt, mut)
    lrl, sfl = _sides(pl, slope, dt, mut)
    gp, gl = gprime(galpha, keep_e, p, mut)[e].to(dt), gprime(gloop, keep_l, p, mut).to(dt)
    sp, slp = soft.to(dt)[e], soft_loop.to(dt)
    z = torch.zeros(N, K, dtype=dt)
    zero = torch.zeros((), dtype=dt)
    dot = z.index_add(0, r, sp * gp * okk) + slp * gl
    ge, gL = torch.where(okk, sp * (gp - dot[r]), zero), slp * (gl - dot)
    a = att.to(dt).reshape(1, K, C)
    ch = _chan_mask(K, C, geo["gv"], dt) if mut == "skip_chunks" else 1.0
    te, tl = ge[:, :, None] * a * sfe * ch, gL[:, :, None] * a * sfl * ch
    z3 = torch.zeros(N, K, C, dtype=dt)
    live_n = torch.ones(N, dtype=dt)
    if mut == "drop_last_pass":
        live_n = ((i // geo["rpp"]) % geo["iters"] != geo["iters"] - 1).to(dt)
    if mut == "drop_partial":
        wg = min(3, geo["nwg"] - 1)
        live_n = (i // (geo["rpp"] * geo["iters"]) != wg).to(dt)
    live_e = live_n[r]
    out = dict(g_logit=_by_eid(e, ge), g_loop=gL, d_xr=(z3.index_add(0, r, te) + tl).reshape(N, K * C),
               d_att=((ge * live_e[:, None])[:, :, None] * lre).sum(0).reshape(-1) + ((gL * live_n[:, None])[:, :, None] * lrl).sum(0).reshape(-1))
    if edge:
        ic, wb, L = loop_inv_cnt.to(dt), loop_w.to(dt), lin_edge.to(dt).reshape(1, K, C)
        wed = we.to(dt)
        out["d_lin_edge"] = ((te * (wed * live_e)[:, None, None]).sum(0) + (tl * (wb * live_n)[:, None, None]).sum(0)).reshape(-1)
        loop_term = torch.zeros(N, dtype=dt) if mut == "no_loop_dw" else (tl * L).sum((1, 2)) * ic
        dw = _by_eid(e, ((te * L).sum((1, 2)) + loop_term[r]) * ok)
        out["d_edge_w"] = dw if (dw_add is None or mut == "no_dw_add") else dw + dw_add.to(dt)
    if bounds:
        assert dt == F64
        nl = torch.zeros(N, dtype=F64).index_add_(0, r, ok.double())
        D = z.index_add(0, r, sp * gp.abs() * okk) + slp * gl.abs()
        Edot = (nl + 3)[:, None] * U * D
        Mge, Ege = sp * (gp.abs() + D[r]) * okk, (sp * (Edot[r] + 3 * U * (gp.abs() + D[r])) + TINY) * okk
        Mgl, Egl = slp * (gl.abs() + D), slp * (Edot + 3 * U * (gl.abs() + D)) + TINY
        aa = a.abs()
        Mte, Mtl = Mge[:, :, None] * aa * sfe, Mgl[:, :, None] * aa * sfl
        Ete, Etl = (Ege[:, :, None] * aa * sfe + 2 * U * Mte + TINY) * okk[:, :, None], Egl[:, :, None] * aa * sfl + 2 * U * Mtl + TINY
        terms = int(nl.sum()) + N
        Lp = terms if geo is None else min(terms, chain(nl, geo))
        out.update(g_logit_bound=_by_eid(e, Ege), g_loop_bound=Egl,
                   d_xr_bound=(z3.index_add(0, r, Ete) + Etl + (nl + 2)[:, None, None] * U * (z3.index_add(0, r, Mte) + Mtl)).reshape(N, K * C),
                   d_att_bound=((Ege[:, :, None] * lre.abs()).sum(0) + (Egl[:, :, None] * lrl.abs()).sum(0)
                                + (Lp + 4) * U * ((Mge[:, :, None] * lre.abs()).sum(0) + (Mgl[:, :, None] * lrl.abs()).sum(0)) + terms * TINY).reshape(-1))
        if edge:
            wa, wba, La = wed.abs()[:, None, None], wb.abs()[:, None, None], L.abs()
            out["d_lin_edge_bound"] = ((Ete * wa).sum(0) + (Etl * wba).sum(0) + (Lp + 3) * U * ((Mte * wa).sum(0) + (Mtl * wba).sum(0))).reshape(-1)
            Mw = (Mte * La).sum((1, 2)) + ((Mtl * La).sum((1, 2)) * ic)[r] + (0 if dw_add is None else dw_add.double().abs()[e])
            Ew = ((Ete * La).sum((1, 2)) + ((Etl * La).sum((1, 2)) * ic)[r] + 2 * K * C * TINY) * ok + (K * C + 5) * U * Mw
            out["d_edge_w_bound"] = _by_eid(e, Ew)
    return out


def dxl(xl, xr, att, ptr, dst, eid, K, C, g_logit, g_loop, slope=SLOPE, edge_w=None, lin_edge=None, loop_w=None, dxl0=None, dt=F64, mut=None,
        bound=False):
    """sgs_gatv2_dxl_heads over the src-CSR with g_logit / g_loop as INPUTS -> d_xl [N, K C] (and its bound).  dxl0: d_xl's contents
    with accumulate = 1.  mut: "no_loop_dxl", "no_accumulate", "slope_side"."""
    N = ptr.numel() - 1
    n, j, d, e, ok = H._entries(ptr, dst, eid)
    i = torch.arange(N)
    edge = edge_w is not None
    _, sfe = _sides(pre(xl, xr, j, d, K, C, edge_w[e] if edge else None, lin_edge), slope, dt, mut)
    _, sfl = _sides(pre(xl, xr, i, i, K, C, loop_w if edge else None, lin_edge), slope, dt, mut)
    a = att.to(dt).reshape(1, K, C)
    te = g_logit.to(dt)[e][:, :, None] * a * sfe * ok[:, None, None].to(dt)
    tl = g_loop.to(dt)[:, :, None] * a * sfl
    if mut == "no_loop_dxl":
        tl = torch.zeros_like(tl)
    z3 = torch.zeros(N, K, C, dtype=dt)
    out = (z3.index_add(0, j, te) + tl).reshape(N, K * C)
    if dxl0 is not None and mut != "no_accumulate":
        out = out + dxl0.to(dt)
    if not bound:
        return out
    ln = (ptr[1:] - ptr[:-1]).double()
    mag = (z3.index_add(0, j, te.abs()) + tl.abs()).reshape(N, K * C) + (0 if dxl0 is None else dxl0.double().abs())
    return out, (ln + 5)[:, None] * U * mag + (ln + 1)[:, None] * TINY


# ------------------------------------------------------------------------------------------------ graphs and inputs
HUB = 200


def graph(N, kind="std", lo=2, hi=10, seed=0):
    """dst-CSR.  "std": row 0 empty, row 1 holds only (1, 1), row 2 begins with (2, 2) and a duplicated pair, a hub of HUB entries in
    the middle (in-degree >> 64) of which 100 come from node N - 3 (out-degree >> 64), one from N - 1 (the source the "spread" inputs boost)
    and one is (h, h); the other rows have lo .. hi - 1 entries from nodes < N - 3.  "empty": no entry at all.  "single": N = 1, two (0, 0)
    entries.  eid is a permutation; gcn_ref.PAD valid entries follow the last row."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * N)
    if kind == "single":
        assert N == 1
        return H._finish(1, torch.tensor([2]), torch.zeros(2, dtype=torch.int64), g)
    if kind == "empty":
        return H._finish(N, torch.zeros(N, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), g)
    lens = torch.randint(lo, hi, (N,), generator=g)
    h = N // 2
    for k, v in {0: 0, 1: 1, 2: 5, h: HUB}.items():
        lens[k] = v
    n = int(lens.sum())
    col = torch.randint(0, N - 3, (n,), generator=g)
    b = torch.zeros(N, dtype=torch.int64)
    b[1:] = lens.cumsum(0)[:-1]
    col[b[1]] = 1
    col[b[2]] = 2
    col[b[2] + 2] = col[b[2] + 1]
    col[b[h] + 10:b[h] + 110] = N - 3
    col[b[h] + 3], col[b[h] + 5] = N - 1, h
    gr = H._finish(N, lens, col, g)
    gr.update(hub_row=h)
    return gr


def inputs(gr, K, C, mode=""):
    """Seeded fp32 inputs for `graph`'s graph: a tenth of the weights exactly 0.  mode "spread": xl[N - 1] puts the hub row's logit of
    that source at 102 in every head (the other logits are O(1): their soft is subnormal or 0); "equal": every row of xl the same and
    (used without the edge term) all logits of a row equal."""
    N, n = gr["N"], gr["n"]
    g = torch.Generator().manual_seed(N * 131 + K * 17 + C)
    rn = lambda *sh: torch.randn(*sh, generator=g)          # noqa: E731
    x = dict(xl=rn(N, K * C), xr=rn(N, K * C), att=rn(K, C), le=rn(K, C), galpha=rn(n, K), gloop=rn(N, K), dw_add=rn(n), dxl0=rn(N, K * C))
    w = 0.05 + 0.95 * torch.rand(n, generator=g)
    w[torch.rand(n, generator=g) < 0.1] = 0.0
    x["w"] = w
    if mode == "spread":
        att, h = x["att"], gr["hub_row"]
        gain = (att.abs() * torch.where(att > 0, 1.0, SLOPE)).sum(1, keepdim=True)          # logit per unit of t in s = t sign(att)
        x["xl"][N - 1] = (102.0 / gain * torch.sign(att)).reshape(-1) - x["xr"][h]
    if mode == "equal":
        x["xl"] = x["xl"][:1].expand(N, -1).contiguous()
    return x


# ------------------------------------------------------------------------------------------------ case tables
V2_N = 67                      # not a multiple of any rows-per-pass count (4 .. 256): dead rows share a wave with live ones
_K_OF = {0: 1, 1: 2, 2: 3, 3: 5, 4: 9}


def _case(name, N, K, C, vec, lg, lgG, one, iters=1, un="", mode="", kind="std", **kw):
    """`code_fwd` / `code_bwd` / `code_dxl`: what sgs_gatv2_variant must return with every pointer aligned (or `un` one float off)."""
    dvec = vec
    lgd = min(log2_ceil(cdiv(K * C, dvec)), 6)
    c = dict(name=name, N=N, K=K, C=C, un=un, mode=mode, kind=kind, code_fwd=code(1, vec, lg, lgG, one), code_bwd=code(2, vec, lg, lgG, one, iters),
             code_dxl=code(3, dvec, lgd), lo=2, hi=10, full=True)
    c.update(kw)
    return c


# every (KP = 2^lgK head slots, 2^lgG lanes per head) at both VEC, ONE; then per lgK the widest lgG with one channel group too many (!ONE)
BYDST_CASES = []
for _lk in range(5):
    _K = _K_OF[_lk]
    for _lgG in range(7 - _lk):
        _C1, _C4 = (1, 2, 3, 5, 9, 17, 33)[_lgG], 4 << _lgG
        BYDST_CASES.append(_case(f"v1_K{_K}_C{_C1}", V2_N, _K, _C1, 1, _lk + _lgG, _lgG, 1))
        BYDST_CASES.append(_case(f"v4_K{_K}_C{_C4}", V2_N, _K, _C4, 4, _lk + _lgG, _lgG, 1))
    BYDST_CASES.append(_case(f"v1_K{_K}_C{(1 << (6 - _lk)) + 1}_chunks", V2_N, _K, (1 << (6 - _lk)) + 1, 1, 6, 6 - _lk, 0))
    BYDST_CASES.append(_case(f"v4_K{_K}_C{(4 << (6 - _lk)) + 4}_chunks", V2_N, _K, (4 << (6 - _lk)) + 4, 4, 6, 6 - _lk, 0))
# further shapes: E = 0, N = 1, K = 3 with three chunks, K = 16 (no padding lanes), the underflowing and the all-equal softmax
EXTRA_CASES = [_case("empty_K2_C8", V2_N, 2, 8, 4, 2, 1, 1, kind="empty"), _case("single_K3_C5", 1, 3, 5, 1, 5, 3, 1, kind="single"),
               _case("v1_K3_C41_chunks", V2_N, 3, 41, 1, 6, 4, 0), _case("v4_K16_C8", V2_N, 16, 8, 4, 5, 1, 1),
               _case("spread_K5_C5", V2_N, 5, 5, 1, 6, 3, 1, mode="spread"), _case("equal_K2_C3", V2_N, 2, 3, 1, 3, 2, 1, mode="equal")]
# C % 4 == 0 with one pointer a float off 16-byte alignment: the launches that test it drop to VEC 1 (K = 2, C = 8: VEC 4 -> lg 2, lgG 1;
# VEC 1 -> lg 4, lgG 3; dxl 16 / 4 = 4 -> lg 2, 16 -> lg 4)
ALIGN_CASES = [_case(f"un_{un}_K2_C8", V2_N, 2, 8, 4, 2, 1, 1, un=un) for un in ("xl", "xr", "att", "lin_edge", "d_xr", "d_xl")]
UN_GEO = dict(by_dst=(1, 4, 3, 1), dxl=(1, 4))
# several row passes per workgroup (E about 2 N): iters 2 ONE / !ONE / VEC 4, and the cap of 16 with nwg = 2049
ITERS_CASES = [_case("iters2_K16_C3", 16389, 16, 3, 1, 6, 2, 1, iters=2, lo=0, hi=5, full=False),
               _case("iters2_K16_C7_chunks", 16389, 16, 7, 1, 6, 2, 0, iters=2, lo=0, hi=5, full=False),
               _case("iters2_K16_C16_v4", 16389, 16, 16, 4, 6, 2, 1, iters=2, lo=0, hi=5, full=False),
               _case("iters16_K16_C3", 131077, 16, 3, 1, 6, 2, 1, iters=16, lo=0, hi=5, full=False)]
SMALL_CASES = BYDST_CASES + EXTRA_CASES + ALIGN_CASES
ALL_CASES = SMALL_CASES + ITERS_CASES


def case_codes(case, edge):
    """(forward, backward, dxl) codes of a case; a pointer off alignment lowers the launches that test it (lin_edge only with edge_w)."""
    out = []
    for op, key in ((OP_FWD, "code_fwd"), (OP_BWD, "code_bwd"), (OP_DXL, "code_dxl")):
        c = case[key]
        if case["un"] in AL16[op] and (case["un"] != "lin_edge" or edge):
            c = code(3, *UN_GEO["dxl"]) if op == OP_DXL else code(op + 1, *UN_GEO["by_dst"], iters=c % 100)
        out.append(c)
    return out


def case_aligned(case, op, edge):
    return 0 if case["un"] in AL16[op] and (case["un"] != "lin_edge" or edge) else 1


def case_graph(case):
    return graph(case["N"], case["kind"], case["lo"], case["hi"])


def case_combos(case):
    """(edge term, dropout p) per case: all four on the small cases, two on the large ones."""
    if case["mode"] == "equal":
        return [(False, 0.0), (False, P_DROP)]
    return [(False, 0.0), (True, 0.0), (False, P_DROP), (True, P_DROP)] if case["full"] else [(False, 0.0), (True, P_DROP)]
