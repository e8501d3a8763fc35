"""fp64 restatement of the contracts of the GINE entry points (section K8d of include/sgs_hip.h: sgs_gine_aggregate_fwd, sgs_gine_aggregate_bwd
with gine_dab_final), the first-order fp32 error bounds the GPU results are held to ELEMENT BY ELEMENT, the launch geometry of the backward
restated from the launcher, graph builders with chosen row lengths, and the case tables of tests/test_gpu_gatv2_gine_kernels.py (checked
on the CPU by tests/test_gatv2_gine_variant_table.py).  Plain torch on the CPU; nothing here imports the product.  Every reference takes
the fp32 inputs the kernel gets; `dt` = float32 evaluates the same formulas in fp32 and `mut` plants one fault (both for the CPU test).

The pre-activation is a fact about the fp32 inputs.  gine_pre = x + (w a + b) is three separate fp32 roundings (the library is built with
-ffp-contract=off; w = 1.0f when edge_w is NULL) and `pre` evaluates exactly that in fp32 on the CPU: the ReLU mask and every summand
relu(pre) resp. m = dz where pre > 0 are the kernel's bit for bit, no element is excluded as "ambiguous", and only the ORDER of the
sums is left to bound.  With fp64 inputs the same functions are the plain fp64 formulas (the composition check against gine_ref).

Bounds (u = 2^-24; nothing in them is measured; magnitudes = the same sum over absolute values):
  forward  z        |err| <= (len_i + 3) u (|diag x_i| + sum relu(pre))          len_i exact summands in any order, the diag product, +1
  backward d_x      |err| <= (len_j + 3) u (|diag dz_j| + sum |m|)               likewise over row j of the src-CSR
           d_edge_w |err| <= (D + 3) u (sum_c |a_c m_c| + |dw_add|)              D products and their sum (per chunk: VEC in a lane, the wave
                                                                                tree; then the running add over the chunks), dw_add's add
           d_a, d_b |err| <= (L + 3) u sum_e |w_e m|  resp.  (L + 2) u sum_e |m|  with L the longest chain of additions a term can pass:
                    lane-private over the entries a wave takes of its workgroup's rows (`chain`, from the row lengths and the restated
                    rows_per_block / nparts), the NW-wave tree (<= NW), gine_dab_final's strided adds (ceil(nparts / 16)) and its tree of
                    16 (<= 16); d_a has the product w m on top.  Always L <= the number of terms."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gcn_ref as G  # noqa: E402
from gat_heads_ref import F32, F64, U, csr_of, outside  # noqa: E402,F401

DIAG = 1.25            # 1 + eps with eps = 0.25: exact in fp32, and visible where it is left out
K_MAX_PARTS = 2048


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launch choice, restated
def variant(N, D, nnz, align_bytes):
    """sgs_gine_variant's formula (csrc/gine.hip), restated: kind * 1000 + VEC * 100 + W."""
    vec = 4 if (D % 4 == 0 and align_bytes >= 16) else 2 if (D % 2 == 0 and align_bytes >= 8) else 1
    while vec > 1 and D <= 32 * vec:
        vec //= 2
    if N <= 65536 and nnz >= 16 * N:
        return 1000 + vec * 100 + (16 if nnz >= 256 * N else 4)
    return vec * 100 + 64


def bwd_geom(N, var):
    """The backward launcher's workgroup layout for variant code `var`: dict(block, nw, rows_per_block, nparts, vec)."""
    vec = var // 100 % 10
    if var >= 1000:
        nw = var % 100
        cap = K_MAX_PARTS // 4 if nw == 16 else K_MAX_PARTS
        return dict(block=True, nw=nw, rows_per_block=0, nparts=min(N, cap), vec=vec)
    rpb = cdiv(cdiv(N, 4), K_MAX_PARTS) * 4 if N > 0 else 4
    return dict(block=False, nw=4, rows_per_block=rpb, nparts=cdiv(N, rpb), vec=vec)


def chain(lens, geo):
    """Longest chain of additions of a d_a / d_b term (see the module docstring)."""
    N = lens.numel()
    if N == 0:
        return 0
    nw, P = geo["nw"], geo["nparts"]
    if geo["block"]:
        per = torch.zeros(P, dtype=torch.int64).index_add_(0, torch.arange(N) % P, (lens + nw - 1) // nw)
    else:
        j = torch.arange(N)
        slot = (j // geo["rows_per_block"]) * 4 + (j % geo["rows_per_block"]) % 4
        per = torch.zeros(P * 4, dtype=torch.int64).index_add_(0, slot, lens)
    return int(per.max()) + nw + cdiv(P, 16) + 16


# ------------------------------------------------------------------------------------------------ references
def pre(x, w, a, b, j):
    """x[j] + (w a + b) in x's dtype, w [n] or None (ones): fp32 inputs give the kernels' three fp32 roundings."""
    wa = a[None, :] if w is None else w[:, None] * a[None, :]          # (1.0f a = a, bit for bit)
    return x[j] + (wa + b[None, :])


def _csr(ptr, col, eid):
    n = int(ptr[-1])
    return n, G.rows_of(ptr), col[:n].long(), eid[:n].long()


def _by_eid(e, v):
    out = torch.zeros_like(v)
    out[e] = v
    return out


def fwd(x, ptr, src, eid, w, a, b, diag=DIAG, dt=F64, mut=None, step=1, bound=False):
    """sgs_gine_aggregate_fwd over the dst-CSR -> z [N, D] (and its bound).  mut: "relu_after_sum"; "skip_tail": of the entries a wave
    takes (every `step`-th) those past its last full group of four are dropped."""
    n, r, s, e = _csr(ptr, src, eid)
    p = pre(x, None if w is None else w[e], a, b, s)
    m = torch.relu(p).to(dt)
    xd = x.to(dt)
    if mut == "relu_after_sum":
        return diag * xd + torch.relu(torch.zeros_like(xd).index_add_(0, r, p.to(dt)))
    if mut == "skip_tail":
        ln = (ptr[1:] - ptr[:-1]).long()
        pos = torch.arange(n) - ptr[:-1].long()[r]
        wave, k = pos % step, pos // step
        cnt = (ln[r] - wave + step - 1) // step
        m = torch.where((k >= cnt - cnt % 4)[:, None], torch.zeros((), dtype=dt), m)
    z = diag * xd + torch.zeros_like(xd).index_add_(0, r, m)
    if not bound:
        return z
    ln = (ptr[1:] - ptr[:-1]).double()
    mag = (diag * xd).abs() + torch.zeros_like(xd).index_add_(0, r, m.abs())
    return z, (ln + 3)[:, None] * U * mag


def bwd(x, dz, ptr, dst, eid, w, a, b, diag=DIAG, dw_add=None, dt=F64, mut=None, geo=None, bounds=False):
    """sgs_gine_aggregate_bwd over the src-CSR -> dict d_x [N, D], d_edge_w [n] by edge id, d_a, d_b [D] (+ "<name>_bound").  geo: bwd_geom's
    dict (the faults that need it, and the chain length of d_a / d_b; None: the term count).  mut: "relu0" (relu'(0) = 1), "no_diag",
    "da_no_w", "drop_chunk2" (columns [64 VEC, 128 VEC) missing from d_edge_w), "no_stride" (rows j >= nparts never visited)."""
    n, j, d, e = _csr(ptr, dst, eid)
    N, D = x.shape
    we = None if w is None else w[e]
    p = pre(x, we, a, b, j)
    mask = p >= 0 if mut == "relu0" else p > 0
    m = torch.where(mask, dz[d], torch.zeros((), dtype=dz.dtype)).to(dt)
    if mut == "no_stride":
        m = m * (j < geo["nparts"]).to(dt)[:, None]
    dzd, ad = dz.to(dt), a.to(dt)
    wd = torch.ones(n, dtype=dt) if we is None else we.to(dt)
    out = {"d_x": (0.0 if mut == "no_diag" else diag * dzd) + torch.zeros_like(dzd).index_add_(0, j, m)}
    am = ad[None, :] * m
    if mut == "drop_chunk2":
        cw = 64 * geo["vec"]
        am[:, cw:2 * cw] = 0
    dw = _by_eid(e, am.sum(1))
    out["d_edge_w"] = dw if dw_add is None else dw + dw_add.to(dt)
    out["d_a"] = m.sum(0) if mut == "da_no_w" else (wd[:, None] * m).sum(0)
    out["d_b"] = m.sum(0)
    if bounds:
        assert dt == F64
        ln = (ptr[1:] - ptr[:-1]).long()
        L = n if geo is None else min(n, chain(ln, geo))
        ma = m.abs()
        out["d_x_bound"] = (ln.double() + 3)[:, None] * U * ((diag * dzd).abs() + torch.zeros_like(dzd).index_add_(0, j, ma))
        out["d_edge_w_bound"] = (D + 3) * U * (_by_eid(e, (ad.abs()[None, :] * ma).sum(1)) + (0 if dw_add is None else dw_add.double().abs()))
        out["d_a_bound"] = (L + 3) * U * (wd.abs()[:, None] * ma).sum(0)
        out["d_b_bound"] = (L + 2) * U * ma.sum(0)
    return out


# ------------------------------------------------------------------------------------------------ graphs and inputs
# row lengths around the kernels' tails, per entry stride `nw` of a wave (1: one wave per row): rows shorter than nw, 4 nw - 1 | 4 nw | 4 nw + 1
SPECIAL = {1: [0, 1, 2, 3, 4, 5, 7, 8, 9], 4: [0, 1, 3, 5, 15, 16, 17, 33], 16: [0, 5, 15, 63, 64, 65]}


def graph(N, nnz, nw, hub=0, seed=0):
    """CSR with SPECIAL[nw] as the lengths of rows 0.., a hub row in the middle, the others sharing what is left of `nnz` evenly; uniform
    columns ((i, i) and duplicate entries occur), eid a permutation, gcn_ref.PAD valid entries behind the last row."""
    g = torch.Generator().manual_seed(1000003 * seed + N + 7 * nnz)
    ln = [-1] * N
    sp = SPECIAL[nw] if N >= len(SPECIAL[nw]) + 2 else []
    for t, v in enumerate(sp):
        ln[t] = v
    if hub and N > len(sp) + 1:
        ln[max(N // 2, len(sp))] = hub
    free = [i for i in range(N) if ln[i] < 0]
    rem = nnz - sum(v for v in ln if v >= 0)
    assert rem >= 0 and (free or rem == 0), (N, nnz, nw, hub)
    for t, i in enumerate(free):
        ln[i] = rem // len(free) + (1 if t < rem % len(free) else 0)
    ln = torch.tensor(ln, dtype=torch.int64)
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    ptr[1:] = ln.cumsum(0)
    col = torch.zeros(nnz + G.PAD, dtype=torch.int32)
    col[:nnz] = torch.randint(0, max(N, 1), (nnz,), generator=g).int()
    eid = torch.zeros(nnz + G.PAD, dtype=torch.int32)
    eid[:nnz] = torch.randperm(nnz, generator=g).int()
    return dict(N=N, nnz=nnz, ptr=ptr.int(), col=col, eid=eid, lens=ln)


def inputs(case, gr):
    """Seeded fp32 inputs.  Pre-activations are planted at exactly 0, read as the src-CSR (row j = the source whose x enters), in the
    longest row: its entry 0 in column 0 for the weights as given (x = -(w a + b) in fp32), and with D > 1 all its entries in column
    D - 1 for unit weights (x = -(a + b)).  "zero": (row j, CSR position, edge id)."""
    N, D, n = case["N"], case["D"], gr["nnz"]
    g = torch.Generator().manual_seed(97 * N + D)
    x = torch.randn(N, D, generator=g)
    a, b = torch.rand(D, generator=g) * 2 - 1, torch.rand(D, generator=g) * 2 - 1
    w = torch.rand(n, generator=g) * 0.9 + 0.05
    out = dict(x=x, a=a, b=b, w=w, dz=torch.randn(N, D, generator=g), dw_add=torch.randn(n, generator=g), zero=None)
    if n:
        j = int(gr["lens"].argmax())
        k = int(gr["ptr"][j])
        e0 = int(gr["eid"][k])
        x[j, 0] = -(w[e0] * a[0] + b[0])
        if D > 1:
            x[j, D - 1] = -(a[D - 1] + b[D - 1])
        out["zero"] = (j, k, e0)
    return out


# ------------------------------------------------------------------------------------------------ case tables
def _c(name, N, D, nnz, nw, code, hub=0, un="", off=0):
    return dict(name=name, N=N, D=D, nnz=nnz, nw=nw, code=code, hub=hub, un=un, off=off)


WAVE_N, WAVE_NNZ = 67, 1000            # nnz < 16 N: one wave per row
B4_N, B4_NNZ = 21, 40 * 21             # 16 N <= nnz < 256 N: 4 waves per row
B16_N, B16_NNZ = 11, 300 * 11          # nnz >= 256 N: 16 waves per row
# D -> VEC after the halving rule: 1, 5, 33 -> 1 (33: one chunk with a tail); 70, 130 -> 2 (130: two chunks of 128 with a tail);
# 132, 260 -> 4 (260: two chunks of 256 with a tail)
_VEC_OF = {1: 1, 5: 1, 33: 1, 70: 2, 130: 2, 132: 4, 260: 4}
CASES = [_c(f"wave_D{D}", WAVE_N, D, WAVE_NNZ, 1, v * 100 + 64, hub=300) for D, v in _VEC_OF.items()]
CASES += [_c(f"block4_D{D}", B4_N, D, B4_NNZ, 4, 1000 + _VEC_OF[D] * 100 + 4, hub=200) for D in (5, 33, 70, 130, 132, 260)]
CASES += [_c(f"block16_D{D}", B16_N, D, B16_NNZ, 16, 1000 + _VEC_OF[D] * 100 + 16, hub=900) for D in (1, 33, 70, 260)]
# sizes that leave the small-N path: rows_per_block 8 on the wave path; the nparts caps 2048 (W = 4) and 512 (W = 16): workgroups stride
BIG_CASES = [_c("wave_N8200_D33", 8200, 33, 3 * 8200, 1, 164, hub=300),
             _c("block4_N2100_D70", 2100, 70, 16 * 2100, 4, 1204, hub=500),
             _c("block16_N520_D5", 520, 5, 256 * 520, 16, 1116, hub=2000)]
# D % 4 == 0 with one operand moved off 16-byte alignment by `off` floats: 8 bytes -> VEC 2, 4 bytes -> VEC 1.  "zdz" = z (forward) / dz
# (backward); d_x exists in the backward only (the forward keeps VEC 4)
FWD_ALIGNED = ("x", "zdz", "a", "b")
BWD_ALIGNED = ("x", "zdz", "a", "b", "d_x")
ALIGN_CASES = [_c(f"wave_D132_un_{un}_{4 * off}B", WAVE_N, 132, WAVE_NNZ, 1, {2: 264, 1: 164}[off], hub=300, un=un, off=off)
               for un in BWD_ALIGNED for off in (2, 1)]
ALL_CASES = CASES + BIG_CASES + ALIGN_CASES


def case_code(case, backward):
    """The code a case states for the forward / backward launch (an operand the launch does not take keeps VEC 4)."""
    if case["un"] and case["un"] not in (BWD_ALIGNED if backward else FWD_ALIGNED):
        return 464
    return case["code"]


def case_align(case, backward):
    """align_bytes as gine_align finds it for the case."""
    return 4 * case["off"] if case["un"] and case["un"] in (BWD_ALIGNED if backward else FWD_ALIGNED) else 16


def case_graph(case):
    return graph(case["N"], case["nnz"], case["nw"], case["hub"])
