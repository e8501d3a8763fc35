"""fp64 restatement of the contracts of sgs_cheb_spmm, sgs_cheb_norm_fwd and sgs_cheb_norm_bwd (section K9 of include/sgs_hip.h), the
first-order fp32 error bounds the GPU results are held to, and the case tables of tests/test_gpu_cheb_kernels.py (checked for coverage,
thresholds, composition and planted faults on the CPU by tests/test_cheb_variant_table.py).  Plain torch on the CPU; nothing here imports
the product.  Conventions, CSR builder, activation / dropout and the ambiguity rule are those of tests/gcn_ref.py.

Bounds (u = 2^-24; valid for an fp32 evaluation in ANY summation order, fma or not; nothing in them is measured):
  step      pre-activation  |err[i, c]| <= (len_i + 5) u (|alpha| sum_k |val_k| |X[col_k, c]| + |add| + |sub| + |bias|)
                            len_i products, the alpha multiply, three adds, one spare; activation / dropout: gcn_ref.spmm_bound
  norm_fwd  dis             |err| <= (len_out / 2 + 4) u dis       the sum of len_out non-negative terms under a square root, then a sqrt and
                            a divide at up to 2 ulp each (both are correctly rounded in this build: the second ulp is margin)
            l               given the kernel's OWN dis:  |l - (-dis[s] w dis[d])| <= 3 u |l|  (two products, one spare); (i, i): exactly 0
  norm_bwd  c_n             |err| <= (len_out + len_in + 7) u * 1/2 dis_n^3 sum |g| |w| |dis|     (three roundings per term, the sum, the
                            three products in front, one spare)
            dw_e            that of c[s_e] plus 5 u (|c[s_e]| + |g dis[s] dis[d]|): g + g2, two products, the difference, one spare;
                            exactly 0 on (i, i) edges and wherever dis[s] == 0"""
import torch

import gcn_ref as G

U = G.U
F32, F64 = torch.float32, torch.float64
ACT_NONE, ACT_RELU, ACT_RELU_DROPOUT = G.ACT_NONE, G.ACT_RELU, G.ACT_RELU_DROPOUT
P_DROP = G.P_DROP


def outside(got, ref, bound):
    """Elements of `got` not within `bound` of `ref` (NaN counts as outside)."""
    return ~((got.double() - ref.double()).abs() <= bound)


# ------------------------------------------------------------------------------------------------ the recurrence step
def row_sum(ptr, col, val, X, mut=None):
    """S[i, :] = sum_{k in row i} val[k] X[col[k], :] in X's dtype.  `col` / `val` may carry entries behind the last row (gcn_ref.PAD)."""
    ptr = ptr.long()
    N, n = ptr.numel() - 1, int(ptr[-1])
    r, c, v = G.rows_of(ptr), col[:n].long(), val[:n].to(X.dtype)
    if mut == "drop_last":                                   # the last entry of every row dropped
        live = torch.ones(n, dtype=torch.bool)
        live[ptr[1:][ptr[1:] > ptr[:-1]] - 1] = False
        r, c, v = r[live], c[live], v[live]
    elif mut == "past_end":                                  # the entry past every row's end included
        r = torch.cat([r, torch.arange(N)])
        c = torch.cat([c, col[ptr[1:]].long()])
        v = torch.cat([v, val[ptr[1:]].to(X.dtype)])
    S = torch.zeros(N, X.shape[1], dtype=X.dtype).index_add_(0, r, v[:, None] * X[c])
    if mut == "skip_last_col":                               # column D - 1 left out of the gather
        S[:, -1] = 0
    return S


def step_pre(ptr, col, val, X, alpha=1.0, add=None, sub=None, bias=None, dt=F64, mut=None):
    """Z = add + alpha * sum_k val[k] X[col[k], :] - sub + bias, evaluated in `dt`; add, sub, bias may be None."""
    t = lambda a: None if a is None else a.to(dt)              # noqa: E731
    X, add, sub, bias = t(X), t(add), t(sub), t(bias)
    Z = alpha * row_sum(ptr, col, val, X, mut)
    if add is not None:
        Z = (alpha * add if mut == "alpha_on_add" else add) + Z
    if sub is not None:
        Z = Z + sub if mut == "sub_added" else Z - sub
    if bias is not None:
        Z = Z + (torch.roll(bias, -1) if mut == "bias_next" else bias)
    return Z


def step_pre_bound(ptr, col, val, X, alpha=1.0, add=None, sub=None, bias=None):
    a = lambda t: None if t is None else t.double().abs()      # noqa: E731
    mag = abs(alpha) * row_sum(ptr, col, val.double().abs(), X.double().abs())
    for t in (a(add), a(sub), a(bias)):
        if t is not None:
            mag = mag + t
    ln = (ptr[1:] - ptr[:-1]).double()
    return (ln + 5.0)[:, None] * U * mag


def step(ptr, col, val, X, alpha=1.0, add=None, sub=None, bias=None, act=ACT_NONE, keep=None, p=0.0, dt=F64, mut=None):
    """The sgs_cheb_spmm contract: Y = act(add + alpha * sum_k val[k] X[col[k], :] - sub + bias); dropout as gcn_ref.activate."""
    return G.activate(step_pre(ptr, col, val, X, alpha, add, sub, bias, dt, mut), act, keep, p)


# ------------------------------------------------------------------------------------------------ the normalisation
def norm_fwd(ei, w, N, dt=F64, mut=None):
    """-> (dis [N], l [n] by edge id).  The degree is summed by SOURCE over the edges that are not (i, i), dis = deg^-1/2 and 0 where
    deg = 0, l_e = -(dis[s] w_e) dis[d] and exactly 0 on (i, i) edges; w None = unit weights."""
    s, d = ei[0].long(), ei[1].long()
    wv = torch.ones(s.numel(), dtype=dt) if w is None else w.to(dt)
    live = s != d
    wd = wv if mut == "count_self" else torch.where(live, wv, torch.zeros_like(wv))
    deg = torch.zeros(N, dtype=dt).index_add_(0, d if mut == "deg_by_dst" else s, wd)
    pos = deg > 0
    dis = torch.where(pos, 1.0 / torch.sqrt(torch.where(pos, deg, torch.ones_like(deg))), torch.zeros_like(deg))
    return dis, l_of_dis(ei, w, dis, dt)


def l_of_dis(ei, w, dis, dt=F64):
    """l by edge id from a GIVEN dis (the kernel's own, for the relation the GPU test holds l to)."""
    s, d = ei[0].long(), ei[1].long()
    wv = torch.ones(s.numel(), dtype=dt) if w is None else w.to(dt)
    dis = dis.to(dt)
    return torch.where(s != d, -((dis[s] * wv) * dis[d]), torch.zeros_like(wv))


def out_lengths(ei, N):
    return torch.bincount(ei[0].long(), minlength=N).double()


def in_lengths(ei, N):
    return torch.bincount(ei[1].long(), minlength=N).double()


def dis_bound(ei, N, dis64):
    return (out_lengths(ei, N) / 2.0 + 4.0) * U * dis64


def l_bound(l64):
    return 3.0 * U * l64.abs()


def norm_bwd(ei, w, g, g2, dis, N, dt=F64, mut=None, bounds=False):
    """-> dw [n] (and, with bounds, c [N] and the two bounds) for g (+ g2) = dLoss/dl by edge id:
    dw_e = c[s_e] - g_e dis[s] dis[d],  c_n = -1/2 dis_n^3 (sum_{e: s_e = n} -w_e dis[d_e] g_e + sum_{e: d_e = n} -dis[s_e] w_e g_e),
    (i, i) edges excluded from the sums and dw_e = 0 on them.  `dis` is an input (the forward's)."""
    s, d = ei[0].long(), ei[1].long()
    wv = torch.ones(s.numel(), dtype=dt) if w is None else w.to(dt)
    ge = g.to(dt)
    if g2 is not None and mut != "no_g2":
        ge = ge + g2.to(dt)
    dis = dis.to(dt)
    live = s != d
    z = torch.zeros_like(wv)
    t_out, t_in = torch.where(live, ge * wv * dis[d], z), torch.where(live, ge * wv * dis[s], z)
    acc = torch.zeros(N, dtype=dt).index_add_(0, s, -t_out).index_add_(0, d, -t_in)
    c = -0.5 * dis * dis * dis * acc
    cs = c[d] if mut == "c_dst" else c[s]
    prod = ge * dis[s] * dis[d]
    dw = torch.where(live, cs - prod, z)
    if not bounds:
        return dw
    mag = torch.zeros(N, dtype=F64).index_add_(0, s, t_out.double().abs()).index_add_(0, d, t_in.double().abs())
    cb = (out_lengths(ei, N) + in_lengths(ei, N) + 7.0) * U * 0.5 * dis.double() ** 3 * mag
    dwb = torch.where(live, cb[s] + 5.0 * U * (c[s].double().abs() + prod.double().abs()), torch.zeros(s.numel(), dtype=F64))
    return dw, c, cb, dwb


# ------------------------------------------------------------------------------------------------ step cases
# Operand layouts of one call.  A dense operand is column block `blk` (width D) of a named buffer of WIDTH[name] blocks; an operand of
# the same name shares that buffer, so "B" below is ONE [N, 3 D] buffer whose blocks the step reads and overwrites in place.
WIDTH = dict(B=3, U=3, A=2, Y0=1, G=1, out=1)
STEP_COMBOS = [
    # Clenshaw's inner step b_k = Y_k + 2 L_hat b_{k+1} - b_{k+2}: in place (add == Y), all three operands blocks of one buffer
    dict(name="inner", alpha=2.0, X=("B", 1), add=("B", 0), sub=("B", 2), bias=False, act=ACT_NONE, Y=("B", 0), Y2=None, scale2=1.0),
    # ... its first step (k = K - 2): no b_{k+2} yet
    dict(name="inner_top", alpha=2.0, X=("B", 2), add=("B", 1), sub=None, bias=False, act=ACT_NONE, Y=("B", 1), Y2=None, scale2=1.0),
    # the final step out = act(Y_0 + L_hat b_1 - b_2 + bias): add and Y dense, sub a block
    dict(name="final_relu", alpha=1.0, X=("B", 0), add=("Y0", 0), sub=("B", 1), bias=True, act=ACT_RELU, Y=("out", 0), Y2=None, scale2=1.0),
    dict(name="final_drop", alpha=1.0, X=("B", 0), add=("Y0", 0), sub=("B", 1), bias=True, act=ACT_RELU_DROPOUT, Y=("out", 0), Y2=None,
         scale2=1.0),
    # backward k = 1: U_1 = L_hat^T G into a block of [N, 3 D], 2 U_1 into a block of [N, 2 D]
    dict(name="bwd_k1", alpha=1.0, X=("G", 0), add=None, sub=None, bias=False, act=ACT_NONE, Y=("U", 1), Y2=("A", 1), scale2=2.0),
    # backward k >= 2: U_k = 2 L_hat^T U_{k-1} - U_{k-2}
    dict(name="bwd_k2", alpha=2.0, X=("U", 1), add=None, sub=("U", 0), bias=False, act=ACT_NONE, Y=("U", 2), Y2=("A", 0), scale2=0.75),
]
DROP_COMBO = next(c for c in STEP_COMBOS if c["act"] == ACT_RELU_DROPOUT)


def _case(name, N, D, nnz, code, nw=4, hub=0, xoff=0, ldpad=0, yoff=0, lens=None):
    """xoff: floats between a 16-byte boundary and the start of X's buffer; ldpad: floats added to that buffer's leading dimension; yoff:
    the float offset of Y's, add's and sub's buffers (X then lives in an aligned buffer of its own); lens: explicit row lengths."""
    return dict(name=name, N=N, D=D, nnz=nnz, code=code, nw=nw, hub=hub, xoff=xoff, ldpad=ldpad, yoff=yoff, lens=lens)


_LN, _LNNZ = 67, 1000
UNALIGNED = dict(off1=dict(xoff=1), ld1=dict(ldpad=1), blk2=dict(xoff=2, ldpad=4))      # the three ways to VEC 1 at D % 4 == 0
STEP_CASES = (
    [_case(f"lanes_v4_lpr{l}_D{d}", _LN, d, _LNNZ, 400 + l, hub=300) for d, l in
     ((4, 1), (8, 2), (16, 4), (32, 8), (64, 16), (128, 32), (256, 64), (260, 64), (512, 64))]
    + [_case(f"lanes_v1_lpr{l}_D{d}", _LN, d, _LNNZ, 100 + l, hub=300) for d, l in
       ((1, 1), (2, 2), (3, 4), (7, 8), (13, 16), (29, 32), (41, 64), (130, 64))]
    + [_case(f"lanes_v1_lpr{l}_D{d}_{how}", _LN, d, _LNNZ, 100 + l, hub=300, **kw) for d, l in ((16, 16), (64, 64)) for how, kw in UNALIGNED.items()]
    + [_case("lanes_v4_lpr16_D64_yas_off1", _LN, 64, _LNNZ, 416, hub=300, yoff=1)]
    + [
        # a workgroup per row: nnz >= 16 N (N <= 65536), 16 waves from 256 N; `nw` places the 8 NW unroll tails
        _case("rb_v4_nw4_N67_D64_at16N", 67, 64, 16 * 67, 1404, nw=4, hub=200),
        _case("rb_v4_nw4_N2100_D72", 2100, 72, 16 * 2100, 1404, nw=4, hub=900),
        _case("rb_v1_nw4_N67_D41_at16N", 67, 41, 16 * 67, 1104, nw=4, hub=200),
        _case("rb_v1_nw4_N67_D64_off1", 67, 64, 16 * 67, 1104, nw=4, hub=200, xoff=1),
        _case("rb_v4_nw16_N67_D260_at256N", 67, 260, 256 * 67, 1416, nw=16, hub=3000),
        _case("rb_v1_nw16_N520_D5", 520, 5, 256 * 520, 1116, nw=16, hub=5000),
        _case("rb_v1_nw16_N67_D65", 67, 65, 256 * 67, 1116, nw=16, hub=3000),
        # the thresholds, from both sides, at both vector widths
        _case("lanes_v4_N67_D64_below16N", 67, 64, 16 * 67 - 1, 416, nw=4, hub=200),
        _case("rb_v4_nw4_N67_D64_below256N", 67, 64, 256 * 67 - 1, 1404, nw=4, hub=3000),
        _case("rb_v4_nw16_N67_D64_at256N", 67, 64, 256 * 67, 1416, nw=16, hub=3000),
        _case("lanes_v1_N67_D41_below16N", 67, 41, 16 * 67 - 1, 164, nw=4, hub=200),
        _case("rb_v1_nw4_N67_D41_below256N", 67, 41, 256 * 67 - 1, 1104, nw=4, hub=3000),
        _case("rb_v1_nw16_N67_D41_at256N", 67, 41, 256 * 67, 1116, nw=16, hub=3000),
        # the row limit of the row-per-workgroup form (its grid is N workgroups)
        _case("rb_v4_nw4_N65536_D4_at16N", 65536, 4, 16 * 65536, 1404, nw=4, hub=5000),
        _case("lanes_v4_N65537_D4_at16N", 65537, 4, 16 * 65537, 401, nw=4, hub=5000),
        # degenerate graphs
        _case("no_entries_null_col_val", 67, 8, 0, 402, lens=[0] * 67),
        _case("one_row_short", 1, 8, 5, 402, lens=[5]),
        _case("one_row_long", 1, 8, 20, 1404, lens=[20]),
        _case("all_rows_empty_but_one", 67, 8, 300, 402, lens=[0] * 33 + [300] + [0] * 33),
    ])


def graph_from_lens(lens, seed=0):
    """gcn_ref.graph with the row lengths given."""
    ln = torch.tensor(lens, dtype=torch.int64)
    N, nnz = ln.numel(), int(ln.sum())
    g = torch.Generator().manual_seed(1000003 * seed + N + 7 * nnz)
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    ptr[1:] = ln.cumsum(0)
    col = torch.zeros(nnz + G.PAD, dtype=torch.int32)
    col[:nnz] = torch.randint(0, N, (nnz,), generator=g).int()
    val = torch.ones(nnz + G.PAD)
    val[:nnz] = (0.5 + torch.rand(nnz, generator=g)) / torch.repeat_interleave(ln.clamp(min=1), ln).float()
    return dict(ptr=ptr.int(), col=col, val=val, lens=ln, nnz=nnz, N=N, gen=g)


def case_graph(case):
    """The case's CSR (gcn_ref.graph: PAD valid entries behind the last row, the special row lengths for the case's NW) with val NEGATED:
    the entries of L_hat are negative."""
    gr = graph_from_lens(case["lens"]) if case["lens"] is not None else G.graph(case["N"], case["nnz"], case["nw"], case["hub"])
    gr["val"] = -gr["val"]
    return gr


def step_inputs(case):
    """The dense buffers of a case, one set for all its combos: B, U [N, 3 D], Y0, G [N, D], a zero-centred bias and the dropout one."""
    N, D = case["N"], case["D"]
    g = torch.Generator().manual_seed(77 + 13 * N + D)
    x = {k: torch.randn(N, WIDTH[k] * D, generator=g) for k in ("B", "U", "Y0", "G")}
    x["bias"] = torch.rand(D, generator=g) - 0.5
    x["bias_drop"] = G.DROP_BIAS + torch.rand(D, generator=g) - 0.5
    return x


def operand(x, spec, D):
    if spec is None:
        return None
    return x[spec[0]][:, spec[1] * D:(spec[1] + 1) * D]


def combo_operands(case, combo, x):
    """-> (X, add, sub, bias) of `combo` as [N, D] views of the case's buffers."""
    D = case["D"]
    bias = None if not combo["bias"] else x["bias_drop" if combo["act"] == ACT_RELU_DROPOUT else "bias"]
    return operand(x, combo["X"], D), operand(x, combo["add"], D), operand(x, combo["sub"], D), bias


def x_layout(case, combo):
    """-> (ldx, aligned16) of the gathered operand as the GPU test lays it out: block `blk` of a buffer that starts `xoff` floats past
    a 16-byte boundary and whose rows are WIDTH * D + ldpad floats apart."""
    name, blk = combo["X"]
    return WIDTH[name] * case["D"] + case["ldpad"], int((case["xoff"] + blk * case["D"]) % 4 == 0)


# ------------------------------------------------------------------------------------------------ normalisation cases
def _ncase(name, N, ei, zero_node=None):
    return dict(name=name, N=N, ei=ei.contiguous(), n=ei.shape[1], zero_node=zero_node)


def _small_directed(zero_node=None, name="small_directed"):
    """N = 70, 620 edges: 612 directed edges none of which leaves node 11 (out-degree 0), 5 of them repeated, and three (i, i) edges."""
    g = torch.Generator().manual_seed(3)
    s = torch.randint(0, 69, (612,), generator=g)
    s = s + (s >= 11).long()
    d = torch.randint(0, 69, (612,), generator=g)
    d = d + (d >= s).long()                                   # d != s
    ei = torch.stack([s, d])
    ei = torch.cat([ei, ei[:, :5], torch.tensor([[5, 17, 17], [5, 17, 17]])], dim=1)
    return _ncase(name, 70, ei[:, torch.randperm(620, generator=g)], zero_node)


def _long_rows():
    """N = 300: node 3 has 200 out-edges and node 8 has 200 in-edges (more than one pass of 64 lanes, not a multiple of 64), among 400
    other edges, two of them (i, i)."""
    g = torch.Generator().manual_seed(4)
    hub_out = torch.stack([torch.full((200,), 3), torch.randint(4, 300, (200,), generator=g)])
    hub_in = torch.stack([torch.randint(9, 300, (200,), generator=g), torch.full((200,), 8)])
    rest = torch.randint(0, 300, (2, 400), generator=g)
    rest[:, 0] = 3
    rest[:, 1] = 8
    ei = torch.cat([hub_out, hub_in, rest], dim=1)
    return _ncase("long_rows", 300, ei[:, torch.randperm(800, generator=g)])


NORM_CASES = [
    _small_directed(),
    _long_rows(),
    _small_directed(zero_node=7, name="zero_out_weights"),      # every out-weight of node 7 exactly 0 (weighted modes): dis = 0 there
    _ncase("only_self_edges", 10, torch.tensor([[0, 3, 3, 9, 5, 5, 5, 1, 2, 2, 8, 0], [0, 3, 3, 9, 5, 5, 5, 1, 2, 2, 8, 0]])),
    _ncase("no_edges", 9, torch.zeros(2, 0, dtype=torch.int64)),
    _ncase("one_node", 1, torch.zeros(2, 3, dtype=torch.int64)),
]
WEIGHT_MODES = ("uniform", "log", "unit")


def norm_weights(case, mode):
    """uniform: U(0.05, 0.95); log: log-uniform over 1e-6 .. 1e3; unit: None (w == NULL)."""
    if mode == "unit":
        return None
    g = torch.Generator().manual_seed(5 + case["n"])
    r = torch.rand(case["n"], generator=g)
    w = r * 0.9 + 0.05 if mode == "uniform" else torch.pow(10.0, r.double() * 9.0 - 6.0).float()
    if case["zero_node"] is not None:
        w[case["ei"][0] == case["zero_node"]] = 0.0
    return w


def norm_grads(case):
    g = torch.Generator().manual_seed(9 + case["n"])
    return torch.randn(case["n"], generator=g), torch.randn(case["n"], generator=g)
