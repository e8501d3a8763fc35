"""fp64 restatement of the contracts of sgs_spmm_csr, sgs_sddmm_csr, sgs_colsum and sgs_act_bwd_colsum (include/sgs_hip.h), the
first-order fp32 error bounds the GPU results are held to, a CSR builder with chosen row lengths, and the case tables of
tests/test_gpu_gcn_variants.py (checked for coverage on the CPU by tests/test_gcn_variant_table.py).  Plain torch on the CPU; nothing
here imports the product.

Bounds (u = 2^-24, the unit roundoff of fp32; valid for an fp32 sum of that length in ANY order, fma or not):
  SpMM   |err[i, c]| <= (len_i + 3) u (sum_k |val_k| |X[col_k, c]| + |diag_i| |X[i, c]| + |bias_c|)     len_i products, diag, bias, +1
         under dropout: times 1 / (1 - p), plus one ulp (2^-23 |y|) of the result for the scaling
  SDDMM  |err[e]|    <= D u sum_c |A[i, c]| |B[j, c]|
  colsum |err[c]|    <= N u sum_r |A[r, c]|
Nothing in them is measured."""
import numpy as np
import torch

U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_RELU_DROPOUT = 0, 1, 2
P_DROP = 0.3


def drop_scale(p):
    """1 / (1 - p) as the C ABI evaluates it: p is a float argument and the scale an fp32 quotient."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def rows_of(ptr):
    """Row index of every CSR entry."""
    ptr = ptr.long()
    return torch.repeat_interleave(torch.arange(ptr.numel() - 1), ptr[1:] - ptr[:-1])


# ------------------------------------------------------------------------------------------------ SpMM
def spmm_pre(ptr, col, val, diag, bias, X):
    """Pre-activation Z[i, :] = sum_k val[k] X[col[k], :] + diag[i] X[i, :] + bias, in X's dtype (fp64 for the reference, fp32 for its
    self-check)."""
    r = rows_of(ptr)
    Z = torch.zeros_like(X).index_add_(0, r, val.to(X.dtype)[:, None] * X[col.long()])
    if diag is not None:
        Z = Z + diag.to(X.dtype)[:, None] * X
    if bias is not None:
        Z = Z + bias.to(X.dtype)
    return Z


def activate(Z, act, keep=None, p=0.0):
    if act == ACT_NONE:
        return Z
    Y = torch.relu(Z)
    if act == ACT_RELU_DROPOUT:
        Y = torch.where(keep.bool(), Y * drop_scale(p), torch.zeros_like(Y))
    return Y


def spmm(ptr, col, val, diag, bias, X, act=ACT_NONE, keep=None, p=0.0):
    """Y = act(Z);  ReLU, or ReLU then dropout with the 0/1 matrix `keep` [N, D] scaled by drop_scale(p)."""
    return activate(spmm_pre(ptr, col, val, diag, bias, X), act, keep, p)


def spmm_pre_bound(ptr, col, val, diag, bias, X):
    """Bound on the PRE-activation's error (ReLU is 1-Lipschitz: it carries over to relu(Z))."""
    X = X.double()
    mag = spmm_pre(ptr, col, val.double().abs(), None if diag is None else diag.double().abs(),
                   None if bias is None else bias.double().abs(), X.abs())
    ln = (ptr[1:] - ptr[:-1]).double()
    return (ln + 3.0)[:, None] * U * mag


def spmm_bound(pre_bound, Y, act, p=0.0):
    """Bound on act(Z) given the pre-activation's; Y the fp64 result."""
    if act != ACT_RELU_DROPOUT:
        return pre_bound
    return pre_bound * drop_scale(p) + 2.0 * U * Y.abs()


# ------------------------------------------------------------------------------------------------ SDDMM
def sddmm(ptr, col, eid, A, B):
    """-> (g [nnz] with g[eid[k]] = <A[i, :], B[col[k], :]> for k in row i, gdiag [N] = <A[i, :], B[i, :]>), in A's dtype."""
    r = rows_of(ptr)
    g = torch.zeros(col.numel(), dtype=A.dtype)
    g[eid.long()] = (A[r] * B[col.long()]).sum(1)
    return g, (A * B).sum(1)


def sddmm_bound(ptr, col, eid, A, B):
    g, gd = sddmm(ptr, col, eid, A.double().abs(), B.double().abs())
    D = A.shape[1]
    return D * U * g, D * U * gd


# ------------------------------------------------------------------------------------------------ column sums
def colsum(A):
    return A.sum(0)


def colsum_bound(A):
    return A.shape[0] * U * A.double().abs().sum(0)


def act_bwd(dY, Y, act, p=0.0):
    """dZ = dY * act'(Y) as fp32 arithmetic defines it (a select and, under dropout, ONE fp32 multiply by drop_scale(p)): an fp32 tensor
    that the kernels must reproduce exactly."""
    dY = dY.float()
    if act == ACT_NONE:
        return dY.clone()
    g = dY if act == ACT_RELU else (dY.double() * drop_scale(p)).float()        # (the product of two fp32 is exact in fp64)
    return torch.where(Y > 0, g, torch.zeros_like(g))


# ------------------------------------------------------------------------------------------------ graphs with chosen row lengths
def special_lengths(nw):
    """Row lengths at which the tails of the kernels change behaviour, for NW waves per row (and the 4-way unroll of spmm_csr)."""
    return [0, 1, 3, 4, 5, 8 * nw - 1, 8 * nw, 8 * nw + 1, 4 * nw * 3 - 1, 4 * nw * 3 + 1]


def row_lengths(N, nnz, nw, hub):
    """N row lengths that sum to exactly `nnz`: the special lengths for `nw` at fixed positions (row 0 gets 8 nw + 1, the last row 8 nw - 1,
    row 1 is empty, the others spread out), one hub row of `hub` entries (0: none) in the middle, and ordinary rows sharing what is left as
    evenly as possible."""
    sp = special_lengths(nw)
    ln = [-1] * N
    if N >= 2 * len(sp) + 2:
        place = {0: 8 * nw + 1, N - 1: 8 * nw - 1, 1: 0}
        rest = [x for x in sp if x not in (8 * nw + 1, 8 * nw - 1, 0)]
        for t, x in enumerate(rest):
            place[2 + (t + 1) * (N - 4) // (len(rest) + 1)] = x
        if hub:
            place[N // 2 + 1 if (N // 2 + 1) not in place else N // 2 + 2] = hub
        for i, x in place.items():
            ln[i] = x
    fixed = sum(x for x in ln if x >= 0)
    free = [i for i in range(N) if ln[i] < 0]
    rem = nnz - fixed
    assert rem >= 0 and (free or rem == 0), (N, nnz, nw, hub, fixed)
    for t, i in enumerate(free):
        ln[i] = rem // len(free) + (1 if t < rem % len(free) else 0)
    assert sum(ln) == nnz
    return ln


PAD = 128      # valid entries kept behind the last row: a kernel that reads past a row's end sees them instead of unmapped memory


def graph(N, nnz, nw=4, hub=0, seed=0):
    """-> dict(ptr [N + 1] i32, col, eid [nnz + PAD] i32, val [nnz + PAD] f32, lens).  Columns are uniform (duplicates and self entries
    occur), eid a permutation of 0..nnz-1, val = U(0.5, 1.5) / max(len_i, 1) (a row's sum stays O(1) whatever its length).  The PAD entries
    behind the last row are (col 0, val 1, eid 0): in bounds, and visible in the result if a kernel reads them."""
    g = torch.Generator().manual_seed(1000003 * seed + N + 7 * nnz)
    ln = torch.tensor(row_lengths(N, nnz, nw, hub), dtype=torch.int64)
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    ptr[1:] = ln.cumsum(0)
    col = torch.zeros(nnz + PAD, dtype=torch.int32)
    col[:nnz] = torch.randint(0, max(N, 1), (nnz,), generator=g).int()
    eid = torch.zeros(nnz + PAD, dtype=torch.int32)
    eid[:nnz] = torch.randperm(nnz, generator=g).int()
    val = torch.ones(nnz + PAD)
    val[:nnz] = (0.5 + torch.rand(nnz, generator=g)) / torch.repeat_interleave(ln.clamp(min=1), ln).float()
    return dict(ptr=ptr.int(), col=col, eid=eid, val=val, lens=ln, nnz=nnz, N=N, gen=g)


def spmm_inputs(N, D, bias_offset, seed=5):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g)
    diag = torch.rand(N, generator=g)
    bias = bias_offset + torch.rand(D, generator=g) - 0.5
    return X, diag, bias


# A dropout case must SHOW its kept set: an element reveals whether it was kept only if its pre-activation is positive beyond the bound.
# Rows sum to O(1) (see graph), so a bias around +8 puts every pre-activation eight standard deviations above zero; the other
# activations run with a zero-centred bias, where ReLU clips half of the elements.
DROP_BIAS = 8.0
MAX_AMBIGUOUS = 1e-3


def ambiguous(Z, pre_bound):
    """Elements whose kept bit the output cannot show: the fp64 pre-activation is not above zero by more than the bound."""
    return ~(Z > pre_bound)


# ------------------------------------------------------------------------------------------------ case tables
# (diag, bias, act): every pair of settings occurs; dropout only with a bias (DROP_BIAS)
SPMM_COMBOS = [(True, True, ACT_RELU_DROPOUT), (False, False, ACT_NONE), (True, False, ACT_RELU), (False, True, ACT_RELU),
               (False, True, ACT_RELU_DROPOUT), (True, True, ACT_NONE)]


def _case(name, N, D, nnz, code, nw=4, hub=0, align=""):
    return dict(name=name, N=N, D=D, nnz=nnz, code=code, nw=nw, hub=hub, align=align)


def _lanes_cases(prefix):
    """The row-per-lanes kernels (kind 0): every (VEC, LPR), N = 67 rows (not a multiple of any rows-per-workgroup count), nnz < 16 N.
    `align`: which dense operand is moved off 16-byte alignment by one float ("" none)."""
    N, nnz = 67, 1000
    c = [_case(f"{prefix}_v4_lpr{l}_D{d}", N, d, nnz, 400 + l, hub=300) for d, l in
         ((4, 1), (8, 2), (16, 4), (32, 8), (64, 16), (128, 32), (256, 64), (260, 64), (512, 64))]
    c += [_case(f"{prefix}_v1_lpr{l}_D{d}", N, d, nnz, 100 + l, hub=300) for d, l in ((1, 1), (2, 2), (3, 4), (41, 64))]
    c += [_case(f"{prefix}_v1_lpr{l}_D{d}_un{a}", N, d, nnz, 100 + l, hub=300, align=a) for d, l, a in
          ((4, 4, "a"), (8, 8, "b"), (16, 16, "a"), (32, 32, "b"), (64, 64, "a"), (260, 64, "b"))]
    return c


SPMM_CASES = _lanes_cases("spmm") + [
    # row-block kernels: nnz = 16 N is the threshold (N <= 65536), 256 N the 16-wave threshold
    _case("spmm_rb_v4_nw4_at16N", 64, 256, 16 * 64, 1404, nw=4, hub=200),
    _case("spmm_below16N_v4", 64, 256, 16 * 64 - 1, 464, nw=4, hub=200),
    _case("spmm_rb_v4_nw4_below256N", 64, 128, 256 * 64 - 1, 1404, nw=4, hub=5000),
    _case("spmm_rb_v4_nw16_at256N", 64, 128, 256 * 64, 1416, nw=16, hub=5000),
    _case("spmm_rb_v4_nw16_D8", 61, 8, 300 * 61, 1416, nw=16, hub=7000),
    _case("spmm_rb_v4_nw4_D4", 131, 4, 20 * 131, 1404, nw=4, hub=900),
    _case("spmm_rb_v4_nw4_D64", 131, 64, 20 * 131, 1404, nw=4, hub=900),
    _case("spmm_rb_v4_nw4_D260", 64, 260, 40 * 64, 1404, nw=4, hub=700),
    _case("spmm_rb_v4_nw16_D512", 64, 512, 256 * 64, 1416, nw=16, hub=3000),
    _case("spmm_rb_v1_nw4_D41_at16N", 300, 41, 16 * 300, 1104, nw=4, hub=1200),
    _case("spmm_below16N_v1_D41", 300, 41, 16 * 300 - 1, 164, nw=4, hub=1200),
    _case("spmm_rb_v1_nw4_D1", 131, 1, 20 * 131, 1104, nw=4, hub=900),
    _case("spmm_rb_v1_nw4_D3", 131, 3, 20 * 131, 1104, nw=4, hub=900),
    _case("spmm_rb_v1_nw16_D41_at256N", 64, 41, 256 * 64, 1116, nw=16, hub=5000),
    _case("spmm_rb_v1_nw4_D41_below256N", 64, 41, 256 * 64 - 1, 1104, nw=4, hub=5000),
    _case("spmm_rb_v1_nw16_D3", 61, 3, 300 * 61, 1116, nw=16, hub=7000),
    _case("spmm_rb_v1_nw4_D256_unx", 64, 256, 40 * 64, 1104, nw=4, hub=700, align="a"),      # unaligned fallback, four column passes
    _case("spmm_rb_v1_nw16_D128_uny", 64, 128, 256 * 64, 1116, nw=16, hub=5000, align="b"),
    # the row limit of the row-block path (its grid is N workgroups)
    _case("spmm_rb_N65536_at16N", 65536, 8, 16 * 65536, 1404, nw=4, hub=40000),
    _case("spmm_N65537_at16N", 65537, 8, 16 * 65537, 402, nw=4, hub=40000),
]

SDDMM_CASES = _lanes_cases("sddmm") + [
    # row-block kernels: nnz = 16 N (any N), 64 N the 16-wave threshold; inside them one pass of the wave at D <= 64 VEC, several above
    _case("sddmm_rb_v4_nw4_at16N", 64, 256, 16 * 64, 1404, nw=4, hub=200),
    _case("sddmm_below16N_v4", 64, 256, 16 * 64 - 1, 464, nw=4, hub=200),
    _case("sddmm_rb_v4_nw4_below64N", 64, 128, 64 * 64 - 1, 1404, nw=4, hub=1500),
    _case("sddmm_rb_v4_nw16_at64N", 64, 128, 64 * 64, 1416, nw=16, hub=1500),
    _case("sddmm_rb_v4_nw4_D4", 131, 4, 20 * 131, 1404, nw=4, hub=900),
    _case("sddmm_rb_v4_nw4_D260", 64, 260, 40 * 64, 1404, nw=4, hub=700),                    # 64 VEC + VEC: the multi-pass path
    _case("sddmm_rb_v4_nw4_D512", 64, 512, 40 * 64, 1404, nw=4, hub=700),
    _case("sddmm_rb_v4_nw16_D256", 64, 256, 100 * 64, 1416, nw=16, hub=3000),                # 64 VEC: the last one-pass width
    _case("sddmm_rb_v4_nw16_D260", 64, 260, 100 * 64, 1416, nw=16, hub=3000),
    _case("sddmm_rb_v4_nw16_D512", 64, 512, 100 * 64, 1416, nw=16, hub=3000),
    _case("sddmm_rb_v1_nw4_D41_at16N", 300, 41, 16 * 300, 1104, nw=4, hub=1200),
    _case("sddmm_below16N_v1_D41", 300, 41, 16 * 300 - 1, 164, nw=4, hub=1200),
    _case("sddmm_rb_v1_nw4_D1", 131, 1, 20 * 131, 1104, nw=4, hub=900),
    _case("sddmm_rb_v1_nw4_D64_una", 131, 64, 20 * 131, 1104, nw=4, hub=900, align="a"),      # 64 VEC at VEC = 1 (unaligned fallback)
    _case("sddmm_rb_v1_nw4_D65", 131, 65, 20 * 131, 1104, nw=4, hub=900),                     # 64 VEC + VEC at VEC = 1
    _case("sddmm_rb_v1_nw16_D41_at64N", 64, 41, 64 * 64, 1116, nw=16, hub=1500),
    _case("sddmm_rb_v1_nw4_D41_below64N", 64, 41, 64 * 64 - 1, 1104, nw=4, hub=1500),
    _case("sddmm_rb_v1_nw16_D64_unb", 64, 64, 100 * 64, 1116, nw=16, hub=3000, align="b"),
    _case("sddmm_rb_v1_nw16_D65", 64, 65, 100 * 64, 1116, nw=16, hub=3000),
    _case("sddmm_rb_v1_nw16_D260_una", 64, 260, 100 * 64, 1116, nw=16, hub=3000, align="a"),
    # no row limit on the row-block path: 70 000 workgroups
    _case("sddmm_rb_N70000_at16N", 70000, 8, 16 * 70000, 1404, nw=4, hub=40000),
    _case("sddmm_N70000_below16N", 70000, 8, 16 * 70000 - 1, 402, nw=4, hub=40000),
]


def _cs(N, D, code, spread=False):
    return dict(name=f"colsum_N{N}_D{D}" + ("_spread" if spread else ""), N=N, D=D, code=code, spread=spread)


SMALL, SMALL4, VECSUM, TWO = 1000000, 2000000, 3000000, 4000000
# `code` is sgs_colsum's; sgs_act_bwd_colsum's is code + FUSED.  spread: column c scaled by 10^(+-3) alternately
FUSED = 100000
COLSUM_CASES = [
    _cs(1, 3, SMALL), _cs(1013, 41, SMALL), _cs(1013, 256, SMALL4), _cs(2048, 1, SMALL), _cs(2048, 65, SMALL), _cs(2048, 64, SMALL4),
    _cs(2047, 16, SMALL4, spread=True), _cs(2048, 3, SMALL),
    _cs(2049, 1, VECSUM), _cs(1 << 20, 1, VECSUM), _cs((1 << 20) + 1, 1, TWO + 25616), _cs(5000, 1, VECSUM),
    _cs(0, 3, TWO + 3204),
    _cs(2049, 64, TWO + 3216), _cs(2049, 65, TWO + 3216), _cs(4095, 41, TWO + 3216), _cs(4095, 256, TWO + 3216),
    _cs(4096, 41, TWO + 12804), _cs(4096, 256, TWO + 12804), _cs(8192, 16, TWO + 12804), _cs(8193, 16, TWO + 12816),
    _cs(8193, 65, TWO + 12816, spread=True), _cs(16383, 3, TWO + 12816), _cs(16383, 64, TWO + 12816),
    _cs(16384, 3, TWO + 25604), _cs(16384, 64, TWO + 25604), _cs(16385, 41, TWO + 25616), _cs(16385, 256, TWO + 25616),
]


def colsum_inputs(case):
    N, D = case["N"], case["D"]
    g = torch.Generator().manual_seed(31 * N + D)
    A = torch.randn(N, D, generator=g)
    if case["spread"]:
        A = A * torch.tensor([1e3 if c % 2 == 0 else 1e-3 for c in range(D)])
    Y = torch.relu(torch.randn(N, D, generator=g))            # about half the activations off
    return A, Y
