"""fp64 restatement of the contracts of the multi-head GAT entry points (section K8h of include/sgs_hip.h: sgs_gat_scores_heads_fwd / _bwd,
sgs_gat_alpha_heads_fwd / _bwd, sgs_gat_alpha_heads_edge_fwd / _bwd, sgs_edge_sum_by_row_heads, sgs_spmm_csr_heads, sgs_sddmm_csr_heads),
the first-order fp32 error bounds the GPU results are held to ELEMENT BY ELEMENT, graph builders with chosen row lengths, and the case
tables of tests/test_gpu_gat_heads_kernels.py (checked on the CPU by tests/test_gat_heads_variant_table.py).  Plain torch on the CPU;
nothing here imports the product.  Every reference takes the fp32 inputs the kernel gets; `dt` = float32 evaluates the same formulas in
fp32 and `mut` plants one fault (both for the CPU test only).

The leaky_relu branch is a fact about the fp32 inputs: the kernels decide it from a_s + a_d (an fp32 add) or fmaf(w, c, a_s + a_d), and
`pre32` reproduces that value: the add in fp32, then product and sum in fp64 (the product of two fp32 is exact there), rounded once.  Hence
the argument of every expf, fp32(logit - row max), is reproduced bit for bit and no element is excluded as "ambiguous".  The edge form's
loop logit depends on wbar_i, an fp32 sum the kernel forms in its own order: the reference takes the kernel's OWN loop_w output for it
(loop_w itself is held to its bound), as alpha is held exactly to the kernel's own soft.

Bounds (u = 2^-24; nothing in them is measured; magnitudes = the same formula on absolute values; n_i = non-loop entries of row i):
  dot product of length L        |err| <= (L + 2) u sum |a| |b|           scores fwd (L = C), SDDMM (L = C; broadcast: L + 2 for 1 / K)
  scores bwd  dxl                |err| <= 3 u (|g_s att_s| + |g_d att_d| + |dxl_in|)      product, fma, the accumulate's add
              d att              |err| <= (L + 2) u sum_i |g| |x|,  L = W + ceil(N / W) <= N + 1 for W rows per workgroup: a term
                                 passes at most W additions in its workgroup's partial row and one per workgroup in the finish
  SpMM        CONCAT             gcn_ref's: (len_i + 3) u mag             len products, diag, bias, +1
              BROADCAST          (len_i + 5) u mag                        + the rounding of 1.0f / K and the product with it
              MEAN, LDS kernel   (len_i + K + 5) u mag                    per-head sums of len + 1 terms, the K-term sum, 1 / K twice, bias, +1
              MEAN, walking      (K (len_i + 1) + 4) u mag                ONE chain over all K (len + 1) products (spmm_csr_heads_mean)
              under dropout      gcn_ref.spmm_bound: times 1 / (1 - p) plus one ulp of the result
  softmax fwd soft = exp64(x32) / (sum exp64(x32) + 1e-16f);  |soft - ref| <= ref (n_i + 4 EXP_ULPS + 4) u + 2^-125
              (EXP_ULPS ulp = 2 EXP_ULPS u per expf, twice: numerator and row sum; n_i u for the sum's order; the 1e-16 add, the
              reciprocal, the product, +1; 2^-125 covers subnormal or flushed expf results, the row sum being >= 1).
              EXP_ULPS = 4 is tests/loss_ref.py's allowance for the device's expf / logf, not a new measurement.
              loop_w: (cnt + 2) u mean |w|;  loop_inv_cnt: u / cnt;  alpha: EXACT given the kernel's soft and the exported mask.
  softmax bwd with g' = fp32(galpha drop_scale) where kept else 0 (exact), D = sum soft |g'| (loop included), sf = 1 or slope:
              E_dot = (n_i + 3) u D
              dpre  = soft (g' - dot) sf:   E_pre = soft sf (E_dot + 3 u (|g'| + D)) + 2^-125     three further roundings; the two
                                            products of a subnormal soft may underflow (or be flushed): 2^-126 each
              d_a_dst:   sum E_pre + E_loop + (n_i + 2) u (sum M_pre + M_loop),   M_pre = soft sf (|g'| + D)
              d_edge_w:  sum_h |c_h| (E_pre + E_loop / cnt) + (K + 4) u (sum_h |c_h| (M_pre + M_loop / cnt) + |dw_add|)
              d_edge_coef: sum |w| E_pre + sum |wbar| E_loop + sum_i (n_i + N + 2) u (sum_{e into i} |w| M_pre + |wbar_i| M_loop)
                           (a term of row i passes at most n_i additions inside its row and at most N across the rows, in any order)
  edge sum by row                (len_j + 2) u (sum |g_edge| + |g_self|)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gcn_ref as G  # noqa: E402

U = G.U
EXP_ULPS = 4
TINY = 2.0 ** -125
SLOPE = 0.2
P_DROP = G.P_DROP
F32, F64 = torch.float32, torch.float64
CONCAT, MEAN, BROADCAST = 0, 1, 2
OP_SCORES_FWD, OP_SCORES_BWD, OP_SPMM_CONCAT, OP_SPMM_MEAN, OP_SPMM_BROADCAST, OP_SDDMM, OP_SDDMM_BROADCAST, OP_ROW = range(8)
SPMM_OP = {CONCAT: OP_SPMM_CONCAT, MEAN: OP_SPMM_MEAN, BROADCAST: OP_SPMM_BROADCAST}
# kinds of sgs_gat_heads_variant's code (include/sgs_hip.h)
K_SCORES_FWD, K_SCORES_BWD, K_CONCAT, K_MEAN_LDS, K_MEAN_WALK, K_BCAST, K_SDDMM, K_SDDMM_BCAST, K_ROW = range(1, 10)
SPMM_KINDS = {CONCAT: (K_CONCAT,), MEAN: (K_MEAN_LDS, K_MEAN_WALK), BROADCAST: (K_BCAST,)}


def code(kind, vec=1, lg=0, lgG=0, w=0):
    return kind * 1000000 + vec * 100000 + lg * 10000 + lgG * 1000 + w


def kp_of(K):
    return 1 << (K - 1).bit_length()


def csr_of(rows, cols, N):
    """CSR of an edge list by `rows`, entries in edge order: (ptr [N + 1], col [E], eid [E]), int64."""
    order = torch.argsort(rows, stable=True)
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    ptr[1:] = torch.bincount(rows, minlength=N).cumsum(0)
    return ptr, cols[order], order


def _by_eid(e, v):
    out = torch.zeros_like(v)
    out[e] = v
    return out


def outside(got, ref, bound):
    """Elements of `got` not within `bound` of `ref` (NaN counts as outside)."""
    return ~((got.double() - ref.double()).abs() <= bound)


# ------------------------------------------------------------------------------------------------ node scores
def scores_fwd(xl, att_s, att_d, K, C, dt=F64):
    x = xl.to(dt).reshape(-1, K, C)
    return (x * att_s.to(dt).reshape(K, C)).sum(-1), (x * att_d.to(dt).reshape(K, C)).sum(-1)


def scores_fwd_bound(xl, att_s, att_d, K, C):
    s, d = scores_fwd(xl.abs(), att_s.abs(), att_d.abs(), K, C)
    return (C + 2) * U * s, (C + 2) * U * d


def scores_bwd(xl, att_s, att_d, g_s, g_d, K, C, dxl0=None, dt=F64, mut=None, rows_per_wg=16):
    """-> (dxl [N, K C], d att_src [K C], d att_dst [K C]).  mut "drop_partial": one workgroup's partial row (its rows_per_wg rows) is
    missing from d att."""
    N = xl.shape[0]
    x, gs, gd = xl.to(dt).reshape(N, K, C), g_s.to(dt), g_d.to(dt)
    dxl = (gs[:, :, None] * att_s.to(dt).reshape(1, K, C) + gd[:, :, None] * att_d.to(dt).reshape(1, K, C)).reshape(N, K * C)
    if dxl0 is not None:
        dxl = dxl + dxl0.to(dt)
    if mut == "drop_partial":
        wg = min(64, (N - 1) // rows_per_wg)
        live = torch.ones(N, dtype=dt)
        live[wg * rows_per_wg:(wg + 1) * rows_per_wg] = 0
        gs, gd = gs * live[:, None], gd * live[:, None]
    return dxl, (gs[:, :, None] * x).sum(0).reshape(-1), (gd[:, :, None] * x).sum(0).reshape(-1)


def scores_bwd_bound(xl, att_s, att_d, g_s, g_d, K, C, dxl0=None, rows_per_wg=1):
    """rows_per_wg: the W of the variant code.  A term passes at most rows_per_wg additions inside its workgroup's partial row and at most
    one per workgroup in the finish, whatever their order: L = rows_per_wg + ceil(N / rows_per_wg) (N + 1 at rows_per_wg = 1: any order)."""
    N = xl.shape[0]
    m, ms, md = scores_bwd(xl.abs(), att_s.abs(), att_d.abs(), g_s.abs(), g_d.abs(), K, C, None if dxl0 is None else dxl0.abs())
    L = rows_per_wg + -(-N // rows_per_wg)
    return 3 * U * m, (L + 2) * U * ms, (L + 2) * U * md


# ------------------------------------------------------------------------------------------------ the per-row family
def _entries(ptr, src, eid):
    n = int(ptr[-1])
    r, s, e = G.rows_of(ptr), src[:n].long(), eid[:n].long()
    return n, r, s, e, s != r


def pre32(a_s, a_d, s, r, w=None, coef=None):
    """The fp32 pre-activation the kernels branch on: a_s[s] + a_d[r] in fp32, then (edge form) fmaf(w, c, .) = product and sum in fp64,
    rounded once."""
    p = a_s[s] + a_d[r]
    assert p.dtype == F32
    if coef is not None:
        p = (w.double()[:, None] * coef.double()[None, :] + p.double()).float()
    return p


def lrelu32(p, slope):
    return torch.where(p > 0, p, p * torch.tensor(slope, dtype=F32))


def _pad_alias(K, *ts):
    """The planted fault of a padding lane (h >= K reads head 0) storing through head K - 1's index."""
    if kp_of(K) != K:
        for t in ts:
            t[:, K - 1] = t[:, 0]


def alpha_fwd(a_s, a_d, ptr, src, eid, K, slope=SLOPE, edge_w=None, coef=None, loop_w=None, dt=F64, mut=None):
    """sgs_gat_alpha_heads_fwd (coef None) / sgs_gat_alpha_heads_edge_fwd.  -> dict: soft [n, K] by edge id (0 at (i, i) entries),
    soft_loop [N, K], n_live [N]; edge form: loop_w, loop_inv_cnt [N] (fp64) and their bounds.  loop_w: the kernel's own fp32 wbar for the
    loop logit (None: the fp64 mean rounded to fp32).  mut: "max_no_loop", "count_self", "pad_alias"."""
    N = ptr.numel() - 1
    n, r, s, e, ok = _entries(ptr, src, eid)
    if mut == "count_self":
        ok = torch.ones_like(ok)
    out = {}
    cnt = torch.zeros(N, dtype=F64).index_add_(0, r[ok], torch.ones(int(ok.sum()), dtype=F64))
    out["n_live"] = cnt
    we = lw = None
    if coef is not None:
        we = edge_w[e]
        wsum = torch.zeros(N, dtype=F64).index_add_(0, r[ok], we[ok].double())
        wabs = torch.zeros(N, dtype=F64).index_add_(0, r[ok], we[ok].double().abs())
        icnt = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0), torch.zeros_like(cnt))
        out.update(loop_w=wsum * icnt, loop_inv_cnt=icnt, loop_w_bound=(cnt + 2) * U * wabs * icnt, loop_inv_cnt_bound=U * icnt)
        lw = out["loop_w"].float() if loop_w is None else loop_w
    i = torch.arange(N)
    le, ll = lrelu32(pre32(a_s, a_d, s, r, we, coef), slope), lrelu32(pre32(a_s, a_d, i, i, lw, coef), slope)
    mx = ll.clone()
    if mut == "max_no_loop":
        mx[cnt > 0] = float("-inf")
    mx = mx.scatter_reduce(0, r[ok][:, None].expand(-1, K), le[ok], "amax", include_self=True)
    xe, xl = (le - mx[r]).to(dt), (ll - mx).to(dt)                     # fp32 subtractions: the arguments of expf
    ee, el = torch.exp(xe) * ok[:, None].to(dt), torch.exp(xl)
    den = torch.zeros(N, K, dtype=dt).index_add_(0, r, ee) + el
    if dt == F64:
        den = den + float(np.float32(1e-16))
        se, sl = ee / den[r], el / den
    else:
        inv = 1.0 / (den + torch.tensor(1e-16, dtype=F32))
        se, sl = ee * inv[r], el * inv
    se = torch.where(ok[:, None], se, torch.zeros_like(se))
    out["soft"], out["soft_loop"] = _by_eid(e, se), sl
    if mut == "pad_alias":
        _pad_alias(K, out["soft"], out["soft_loop"])
    return out


def soft_bound(ref, ptr, src, eid):
    """-> (bound on soft [n, K] by edge id, bound on soft_loop) for the fp64 result `ref` of alpha_fwd."""
    n, r, s, e, ok = _entries(ptr, src, eid)
    f = (ref["n_live"] + 4 * EXP_ULPS + 4) * U
    return ref["soft"] * _by_eid(e, f[r])[:, None] + TINY, ref["soft_loop"] * f[:, None] + TINY


def dropped(v32, keep, p):
    """where(keep, fp32(v drop_scale(p)), 0): the kernels' one fp32 multiply, exactly (keep None: no dropout)."""
    if keep is None:
        return v32.clone()
    return torch.where(keep.bool(), (v32.double() * G.drop_scale(p)).float(), torch.zeros_like(v32))


def alpha_of(soft32, keep, p, eid=None):
    """alpha from the kernel's own soft [n, K] by edge id.  eid given: the planted fault of a mask keyed by CSR position (row k of `keep`
    for the entry at position k) instead of by edge id."""
    if eid is None or keep is None:
        return dropped(soft32, keep, p)
    e = eid[:soft32.shape[0]].long()
    return _by_eid(e, dropped(soft32[e], keep, p))


def alpha_bwd(a_s, a_d, ptr, src, eid, K, soft, soft_loop, galpha, gloop, slope=SLOPE, keep_e=None, keep_l=None, p=0.0, edge_w=None, coef=None,
              loop_w=None, loop_inv_cnt=None, dw_add=None, dt=F64, mut=None, bounds=False, keep_by_pos=False):
    """sgs_gat_alpha_heads_bwd (coef None) / sgs_gat_alpha_heads_edge_bwd with soft / soft_loop / galpha / gloop (and, edge form, loop_w /
    loop_inv_cnt) as INPUTS.  -> dict g_edge [n, K] by edge id, g_selfloop, d_a_dst [N, K], d_edge_w [n], d_edge_coef [K]; bounds = True
    adds "<name>_bound" (fp64).  mut: "slope_side", "drop_partial", "pad_alias"; keep_by_pos: the mask row of an entry is its CSR position."""
    N = ptr.numel() - 1
    n, r, s, e, ok = _entries(ptr, src, eid)
    i = torch.arange(N)
    okk = ok[:, None]
    edge = coef is not None
    we = edge_w[e] if edge else None
    pe, pl = pre32(a_s, a_d, s, r, we, coef), pre32(a_s, a_d, i, i, loop_w if edge else None, coef)
    side = (lambda q: q >= 0) if mut == "slope_side" else (lambda q: q > 0)
    one, sl32 = torch.ones((), dtype=dt), torch.tensor(slope, dtype=F32).to(dt)
    sfe, sfl = torch.where(side(pe), one, sl32), torch.where(side(pl), one, sl32)
    gp = dropped(galpha[e], keep_e[:n], p) if keep_by_pos and keep_e is not None else dropped(galpha, keep_e, p)[e]
    gp, gl = gp.to(dt), dropped(gloop, keep_l, p).to(dt)
    sp, sl = soft.to(dt)[e], soft_loop.to(dt)
    z = torch.zeros(N, K, dtype=dt)
    dot = z.index_add(0, r, sp * gp * okk) + sl * gl
    dpre = torch.where(okk, sp * (gp - dot[r]) * sfe, torch.zeros((), dtype=dt))
    dl = sl * (gl - dot) * sfl
    out = dict(g_edge=_by_eid(e, dpre), g_selfloop=dl, d_a_dst=z.index_add(0, r, dpre) + dl)
    if edge:
        c, ic, wb = coef.to(dt), loop_inv_cnt.to(dt), loop_w.to(dt)
        t = (c * (dpre + (dl * ic[:, None])[r])).sum(1) * ok
        dw = _by_eid(e, t)
        out["d_edge_w"] = dw if dw_add is None else dw + dw_add.to(dt)
        live_e, live_n = torch.ones(n, dtype=dt), torch.ones(N, dtype=dt)
        if mut == "drop_partial":                                         # workgroup 64's four rows (or the last workgroup's)
            wg = min(64, (N - 1) // 4)
            live_n[4 * wg:4 * wg + 4] = 0
            live_e = live_n[r]
        out["d_edge_coef"] = (we.to(dt)[:, None] * dpre * live_e[:, None]).sum(0) + (wb[:, None] * dl * live_n[:, None]).sum(0)
    if mut == "pad_alias":
        _pad_alias(K, out["g_edge"], out["g_selfloop"], out["d_a_dst"])
    if bounds:
        assert dt == F64
        nl = torch.zeros(N, dtype=F64).index_add_(0, r, ok.double())
        D = z.index_add(0, r, sp * gp.abs() * okk) + sl * gl.abs()
        Edot = (nl + 3)[:, None] * U * D
        Mpre, Epre = sp * sfe * (gp.abs() + D[r]) * okk, (sp * sfe * (Edot[r] + 3 * U * (gp.abs() + D[r])) + TINY) * okk
        Ml, El = sl * sfl * (gl.abs() + D), sl * sfl * (Edot + 3 * U * (gl.abs() + D)) + TINY
        out.update(g_edge_bound=_by_eid(e, Epre), g_selfloop_bound=El,
                   d_a_dst_bound=z.index_add(0, r, Epre) + El + (nl + 2)[:, None] * U * (z.index_add(0, r, Mpre) + Ml))
        if edge:
            ca = c.abs()
            Mt = (ca * (Mpre + (Ml * ic[:, None])[r])).sum(1) + (0 if dw_add is None else dw_add.double().abs()[e])
            Et = (ca * (Epre + (El * ic[:, None])[r])).sum(1) * ok + (K + 4) * U * Mt
            out["d_edge_w_bound"] = _by_eid(e, Et)
            wa, wba = we.double().abs()[:, None], wb.abs()[:, None]
            Mrow = z.index_add(0, r, wa * Mpre) + wba * Ml                    # row i's terms: n_i additions inside the row, at most N across rows
            out["d_edge_coef_bound"] = (wa * Epre).sum(0) + (wba * El).sum(0) + ((nl + N + 2)[:, None] * U * Mrow).sum(0)
    return out


def alpha_smooth(a_s, a_d, ptr, src, eid, slope=SLOPE, edge_w=None, coef=None):
    """The same softmax in the inputs' own dtype with no fp32 step: differentiable, for the CPU self-checks.  -> (soft by eid, soft_loop)."""
    N, K = a_s.shape
    n, r, s, e, ok = _entries(ptr, src, eid)
    dt = a_s.dtype
    pe, pl = a_s[s] + a_d[r], a_s + a_d
    if coef is not None:
        okd = ok.to(dt)
        cnt = torch.zeros(N, dtype=dt).index_add(0, r, okd)
        wb = torch.zeros(N, dtype=dt).index_add(0, r, edge_w[e] * okd) / cnt.clamp(min=1.0)
        pe, pl = pe + edge_w[e][:, None] * coef, pl + wb[:, None] * coef
    le, ll = torch.nn.functional.leaky_relu(pe, slope), torch.nn.functional.leaky_relu(pl, slope)
    mx = ll.detach().scatter_reduce(0, r[ok][:, None].expand(-1, K), le.detach()[ok], "amax", include_self=True)
    ee, el = torch.exp(le - mx[r]) * ok[:, None].to(dt), torch.exp(ll - mx)
    den = torch.zeros(N, K, dtype=dt).index_add(0, r, ee) + el + 1e-16
    return torch.zeros(n, K, dtype=dt).index_add(0, e, ee / den[r]), el / den


def edge_sum_by_row(g_edge, g_self, ptr, eid, dt=F64, mut=None):
    n = int(ptr[-1])
    r, e = G.rows_of(ptr), eid[:n].long()
    out = torch.zeros(ptr.numel() - 1, g_edge.shape[1], dtype=dt).index_add_(0, r, g_edge.to(dt)[e])
    if g_self is not None:
        out = out + g_self.to(dt)
    if mut == "pad_alias":
        _pad_alias(g_edge.shape[1], out)
    return out


def edge_sum_by_row_bound(g_edge, g_self, ptr, eid):
    ln = (ptr[1:] - ptr[:-1]).double()
    return (ln + 2)[:, None] * U * edge_sum_by_row(g_edge.abs(), None if g_self is None else g_self.abs(), ptr, eid)


# ------------------------------------------------------------------------------------------------ SpMM / SDDMM per head
def spmm_heads_pre(ptr, col, eid, val, diag, bias, X, K, C, mode, mut=None):
    """Pre-activation of sgs_spmm_csr_heads in X's dtype; val [n, K] by edge id, diag [N, K] or None, X [N, K C] ([N, C]: BROADCAST).
    mut: "skip_tail" (the last len % 4 entries of a row), "mean_div_kp" (1 / KP for 1 / K)."""
    dt = X.dtype
    N = ptr.numel() - 1
    n = int(ptr[-1])
    r, c, e = G.rows_of(ptr), col[:n].long(), eid[:n].long()
    w = val.to(dt)[e]
    if mut == "skip_tail":
        ln = (ptr[1:] - ptr[:-1]).long()
        pos = torch.arange(n) - ptr[:-1].long()[r]
        w = torch.where((pos >= (ln - ln % 4)[r])[:, None], torch.zeros((), dtype=dt), w)
    Xh = X.reshape(N, 1, C) if mode == BROADCAST else X.reshape(N, K, C)
    Z = torch.zeros(N, K, C, dtype=dt).index_add_(0, r, w[:, :, None] * Xh[c])
    if diag is not None:
        Z = Z + diag.to(dt)[:, :, None] * Xh
    div = kp_of(K) if mut == "mean_div_kp" else K
    Z = Z.reshape(N, K * C) if mode == CONCAT else (Z.reshape(N, K * C) / div if mode == BROADCAST else Z.sum(1) / div)
    return Z if bias is None else Z + bias.to(dt)


def spmm_heads_pre_bound(ptr, col, eid, val, diag, bias, X, K, C, mode, walk=False):
    ab = lambda t: None if t is None else t.double().abs()          # noqa: E731
    mag = spmm_heads_pre(ptr, col, eid, ab(val), ab(diag), ab(bias), ab(X), K, C, mode)
    ln = (ptr[1:] - ptr[:-1]).double()
    terms = {CONCAT: ln + 3, BROADCAST: ln + 5, MEAN: K * (ln + 1) + 4 if walk else ln + K + 5}[mode]
    return terms[:, None] * U * mag


def sddmm_heads(ptr, col, eid, A, B, K, C, broadcast):
    """-> (g [n, K] by edge id, gdiag [N, K]) in A's dtype; A [N, K C] ([N, C], products / K: broadcast), B [N, K C]."""
    N = ptr.numel() - 1
    n = int(ptr[-1])
    r, c, e = G.rows_of(ptr), col[:n].long(), eid[:n].long()
    Ah, Bh = (A.reshape(N, 1, C) if broadcast else A.reshape(N, K, C)), B.reshape(N, K, C)
    g, gd = (Ah[r] * Bh[c]).sum(-1), (Ah * Bh).sum(-1)
    if broadcast:
        g, gd = g / K, gd / K
    return _by_eid(e, g), gd


def sddmm_heads_bound(ptr, col, eid, A, B, K, C, broadcast):
    g, gd = sddmm_heads(ptr, col, eid, A.double().abs(), B.double().abs(), K, C, broadcast)
    L = C + 2 + (2 if broadcast else 0)
    return L * U * g, L * U * gd


# ------------------------------------------------------------------------------------------------ graphs and inputs
def _finish(N, lens, col, g, K=None):
    n = int(lens.sum())
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    ptr[1:] = lens.cumsum(0)
    eid = torch.zeros(n + G.PAD, dtype=torch.int32)
    eid[:n] = torch.randperm(n, generator=g).int()
    colp = torch.zeros(n + G.PAD, dtype=torch.int32)
    colp[:n] = col.int()
    return dict(N=N, n=n, ptr=ptr.int(), col=colp, eid=eid, lens=lens, gen=g)


BIG, SUB = 110.0, 20.0        # a_s of the two planted sources of the hub row: logits 110 resp. 90 below the row maximum


def row_graph(N, K, hub=300, seed=0):
    """dst-CSR for the per-row family with EPW = 64 / KP entries per step: rows of length EPW + 1 (row 0), 0 (row 1), 1 (row 2: its ONLY
    entry is (2, 2)), EPW - 1, EPW, 2 EPW + 1 (row 5: begins with (5, 5), then a duplicate pair), a hub of `hub` entries (row N // 2: holds
    sources N - 1 and N - 2, whose scores put the other logits 110 resp. 90 below the maximum, and an (i, i) entry), the others 2..9.  Entry
    0 of row 0 comes from node 7 (a_s[7] = -a_d[0]: pre-activation exactly 0; its weight is 0 in the edge form).  Sources N - 1, N - 2
    occur nowhere else.  eid is a permutation; G.PAD valid entries follow the last row."""
    epw = 64 // kp_of(K)
    g = torch.Generator().manual_seed(7919 * seed + 31 * N + K)
    lens = torch.randint(2, 10, (N,), generator=g)
    h = N // 2
    for i, v in {0: epw + 1, 1: 0, 2: 1, 3: epw - 1, 4: epw, 5: 2 * epw + 1, h: hub}.items():
        lens[i] = v
    n = int(lens.sum())
    col = torch.randint(0, N - 2, (n,), generator=g)
    b = torch.zeros(N, dtype=torch.int64)
    b[1:] = lens.cumsum(0)[:-1]
    col[b[0]] = 7
    col[b[2]] = 2
    col[b[5]] = 5
    col[b[5] + 2] = col[b[5] + 1]
    col[b[h] + 3], col[b[h] + 4], col[b[h] + 5] = N - 1, N - 2, h
    gr = _finish(N, lens, col, g)
    gr.update(K=K, hub_row=h, zero_eid=int(gr["eid"][b[0]]))
    return gr


def row_inputs(gr):
    """Scores, edge weights (a tenth exactly 0), coefficients and upstream gradients for row_graph's graph."""
    N, K, n, g = gr["N"], gr["K"], gr["n"], torch.Generator().manual_seed(gr["N"] * 131 + gr["K"])
    a_s, a_d = torch.randn(N, K, generator=g), torch.randn(N, K, generator=g)
    a_s[7] = -a_d[0]                 # entry (0 <- 7): pre-activation exactly 0 in every head
    a_s[4] = -a_d[4]                 # the loops of nodes 4 and 1 (no in-edges: wbar = 0) likewise
    a_s[1] = -a_d[1]
    a_s[N - 1] += BIG
    a_s[N - 2] += SUB
    w = 0.05 + 0.95 * torch.rand(n, generator=g)
    w[torch.rand(n, generator=g) < 0.1] = 0.0
    w[gr["zero_eid"]] = 0.0
    return dict(a_s=a_s, a_d=a_d, w=w, coef=torch.randn(K, generator=g), galpha=torch.randn(n, K, generator=g),
                gloop=torch.randn(N, K, generator=g), dw_add=torch.randn(n, generator=g), g_self=torch.randn(N, K, generator=g))


SPMM_LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9]       # around the 4-way unroll of spmm_heads_acc


def agg_graph(N, K, hub=300, seed=0):
    """CSR for the SpMM / SDDMM: rows 1.. of the lengths SPMM_LENGTHS, a hub in the middle, the others 0..12; uniform columns (self and
    duplicate entries occur); val [n, K] by edge id = U(0.5, 1.5) / max(len_i, 1); diag [N, K]."""
    g = torch.Generator().manual_seed(104729 * seed + 17 * N + K)
    lens = torch.randint(0, 13, (N,), generator=g)
    for t, v in enumerate(SPMM_LENGTHS):
        lens[1 + t] = v
    lens[N // 2] = hub
    n = int(lens.sum())
    gr = _finish(N, lens, torch.randint(0, N, (n,), generator=g), g)
    per_row = torch.repeat_interleave(lens.clamp(min=1), lens).float()
    val = torch.zeros(n, K)
    val[gr["eid"][:n].long()] = (0.5 + torch.rand(n, K, generator=g)) / per_row[:, None]
    gr.update(K=K, val=val, diag=torch.rand(N, K, generator=g))
    return gr


# ------------------------------------------------------------------------------------------------ case tables
ROW_N = 70
# (K, KP): every instantiation, with and without padding lanes
HUB = 300
# `rows`: the CSR row-length recipe (the builder above that takes N, K and `hub`)
ROW_CASES = [dict(name=f"row_K{K}", N=ROW_N, K=K, rows="row_graph", hub=HUB, code=code(K_ROW, w=kp)) for K, kp in
             ((1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (7, 8), (8, 8), (9, 16), (13, 16), (16, 16))]
# 258 workgroups of 4 rows: gat_edge_dc_finish makes five passes, the last workgroup is half live
ROW_CASES.append(dict(name="row_K5_N1030", N=1030, K=5, rows="row_graph", hub=HUB, code=code(K_ROW, w=8)))

SCORES_N = 67


def _sf(K, C, vec, lg, att_off=0):
    return dict(name=f"scores_fwd_K{K}_C{C}" + ("_unatt" if att_off else ""), N=SCORES_N, K=K, C=C, att_off=att_off,
                code=code(K_SCORES_FWD, vec, lg))


# (K, C, lg aligned [VEC 4 when C % 4 == 0], lg with the att pointers one float off [VEC 1])
SCORES_FWD_CASES = [c for K, C, la, lu in
                    ((3, 1, 0, 0), (16, 5, 3, 3), (8, 32, 3, 5), (2, 300, 6, 6),                 # C = 300: the column loop wraps at both VEC
                     (2, 2, 1, 1), (2, 3, 2, 2), (2, 4, 0, 2), (2, 8, 1, 3), (2, 16, 2, 4), (2, 64, 4, 6), (2, 128, 5, 6), (3, 9, 4, 4))
                    for c in (_sf(K, C, 4 if C % 4 == 0 else 1, la), _sf(K, C, 1, lu, 1))]


def _sb(N, K, C, rpw):
    return dict(name=f"scores_bwd_N{N}_K{K}_C{C}", N=N, K=K, C=C, rpw=rpw, code=code(K_SCORES_BWD, w=rpw))


# N = 1040: 65 partial rows, the finish enters its four-way loop; 4095 | 4096 and 65535 | 65536: the rows-per-workgroup thresholds;
# (16, 17): D = 272 > 256, the column loop of the backward wraps
SCORES_BWD_CASES = [_sb(1040, 2, 4, 16), _sb(4095, 2, 4, 16), _sb(4096, 2, 4, 64), _sb(65535, 2, 4, 64), _sb(65536, 2, 4, 256),
                    _sb(50, 16, 17, 16)]

AGG_N = 67
_KIND_NAME = {K_CONCAT: "concat", K_MEAN_LDS: "meanlds", K_MEAN_WALK: "meanwalk", K_BCAST: "bcast"}


def _sp(mode, kind, K, C, vec, lg, align="", epi=False):
    return dict(name=f"spmm_{_KIND_NAME[kind]}_K{K}_C{C}" + (f"_un{align}" if align else "") + ("_epi" if epi else ""), N=AGG_N, K=K, C=C,
                mode=mode, align=align, epi=epi, rows="agg_graph", hub=HUB, code=code(kind, vec, lg))


# (K, C, VEC, lg): 2^lg lanes own the K C / VEC column groups of a row (64 at most, the column loop wraps above)
_WIDE = [(1, 1, 1, 0), (2, 1, 1, 1), (2, 2, 1, 2), (5, 1, 1, 3), (3, 5, 1, 4), (7, 3, 1, 5), (16, 5, 1, 6),
         (1, 4, 4, 0), (2, 4, 4, 1), (4, 4, 4, 2), (5, 4, 4, 3), (8, 4, 4, 3), (4, 16, 4, 4), (8, 16, 4, 5), (8, 32, 4, 6), (16, 20, 4, 6)]
SPMM_CASES = []
for _mode, _kind in ((CONCAT, K_CONCAT), (BROADCAST, K_BCAST)):
    SPMM_CASES += [_sp(_mode, _kind, K, C, v, lg) for K, C, v, lg in _WIDE]
    SPMM_CASES += [_sp(_mode, _kind, 8, 32, 1, 6, "x"), _sp(_mode, _kind, 8, 4, 1, 5, "y")]     # C % 4 == 0 off alignment: VEC 1
SPMM_CASES += [_sp(MEAN, K_MEAN_LDS, K, C, v, lg) for K, C, v, lg in _WIDE + [(8, 5, 1, 6), (16, 64, 4, 6)]]     # K C = 1024: still LDS
SPMM_CASES += [_sp(MEAN, K_MEAN_LDS, 16, 64, 1, 6, "x"), _sp(MEAN, K_MEAN_LDS, 5, 4, 1, 5, "y"),
               _sp(MEAN, K_MEAN_WALK, 16, 65, 1, 6), _sp(MEAN, K_MEAN_WALK, 16, 68, 4, 5), _sp(MEAN, K_MEAN_WALK, 8, 132, 4, 6),
               _sp(MEAN, K_MEAN_WALK, 16, 68, 1, 6, "x"), _sp(MEAN, K_MEAN_WALK, 16, 68, 1, 6, "y"),
               # the bias / ReLU / dropout epilogue
               _sp(CONCAT, K_CONCAT, 5, 4, 4, 3, epi=True), _sp(MEAN, K_MEAN_LDS, 8, 5, 1, 6, epi=True),
               _sp(MEAN, K_MEAN_WALK, 16, 68, 4, 5, epi=True)]
# (diag, bias, act) per case; with `epi` also dropout (bias gcn_ref.DROP_BIAS, so the output shows its kept set)
SPMM_COMBOS = [(True, False, G.ACT_NONE), (False, True, G.ACT_RELU)]
SPMM_EPI_COMBOS = SPMM_COMBOS + [(True, True, G.ACT_NONE), (True, True, G.ACT_RELU_DROPOUT)]


def spmm_x(case, drop):
    K, C, N = case["K"], case["C"], case["N"]
    g = torch.Generator().manual_seed(1 + K * 1000 + C)
    X = torch.randn(N, C if case["mode"] == BROADCAST else K * C, generator=g)
    W = C if case["mode"] == MEAN else K * C
    return X, (G.DROP_BIAS if drop else 0.0) + torch.rand(W, generator=g) - 0.5


def _sd(K, C, vec, lgK, lgG, align=""):
    return dict(name=f"sddmm_K{K}_C{C}" + (f"_un{align}" if align else ""), N=AGG_N, K=K, C=C, align=align, rows="agg_graph", hub=HUB,
                code=code(K_SDDMM, vec, lgK + lgG, lgG), code_bcast=code(K_SDDMM_BCAST, vec, lgK + lgG, lgG))


# every (KP = 2^lgK head slots, 2^lgG lanes per head) at both VEC; then the issue's shapes: (16, 64) and (1, 1024) wrap the column loop
_K_OF = {0: 1, 1: 2, 2: 3, 3: 5, 4: 9}
SDDMM_CASES = [_sd(_K_OF[lk], (1, 2, 3, 5, 9, 17, 33)[lg], 1, lk, lg) for lk in range(5) for lg in range(7 - lk)]
SDDMM_CASES += [_sd(_K_OF[lk], 4 << lg, 4, lk, lg) for lk in range(5) for lg in range(7 - lk)]
SDDMM_CASES += [_sd(16, 64, 4, 4, 2), _sd(1, 1024, 4, 0, 6), _sd(8, 32, 4, 3, 3), _sd(8, 32, 1, 3, 3, "a"),
                _sd(16, 64, 1, 4, 2, "b"), _sd(7, 300, 4, 3, 3), _sd(16, 7, 1, 4, 2)]


def sddmm_ab(case, broadcast):
    K, C, N = case["K"], case["C"], case["N"]
    g = torch.Generator().manual_seed(3 + K * 1000 + C)
    return torch.randn(N, C if broadcast else K * C, generator=g), torch.randn(N, K * C, generator=g)


def scores_inputs(case):
    N, K, C = case["N"], case["K"], case["C"]
    g = torch.Generator().manual_seed(N + K * C)
    rn = lambda *sh: torch.randn(*sh, generator=g)          # noqa: E731
    return dict(xl=rn(N, K * C), att_s=rn(K, C), att_d=rn(K, C), g_s=rn(N, K), g_d=rn(N, K), dxl0=rn(N, K * C))


def case_graph(case):
    """The graph of a case of the per-row, SpMM or SDDMM tables, by its `rows` recipe."""
    return {"row_graph": row_graph, "agg_graph": agg_graph}[case["rows"]](case["N"], case["K"], case["hub"])
