"""The long-row path of the row-block SpMM kernels (sgs_spmm_long_rows_set; csrc/gcn.hip: spmm_long_row_gather), through the C ABI on
raw CSR arrays.

GPU: with the switch on, every entry point that gathers through the two shared bodies (sgs_spmm_csr, sgs_spmm_csr_next,
sgs_spmm_csr_bwd_prev in both modes, sgs_spmm_csr_dual, sgs_spmm_csr_next_dual) writes bit for bit what it writes with the switch off,
twice; the on-path output is inside gcn_ref.py's a-priori fp32 bound of the fp64 evaluation; and a GNNModel forward + backward on a
skewed partition is bitwise the same either way.  Two graphs:
  nw4   N = 1037 (not a multiple of the 4 rows a pair workgroup owns): one row of every length at which the old loop, the long path's
        64-entry chunks or its batches of 4 / 6 / 8 rows change behaviour, long rows first, last and inside 4-row groups (two of them
        side by side), the other rows 10..30 entries.  Every row's columns are distinct (1036 = every other node).
  nw16  N = 301, every row 256..300 entries: the 16-wave kernels, every row on the long path.
Outputs are pre-filled with NaN, so an element that is not written fails the comparison.

CPU (unmarked): the switch and its queries work without a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gcn_ref as R  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
SEED, SITE = 0x51F15EED, 3
GU, NW = 8, 4               # the 4-wave kernels' short loop: batches of GU entries per wave


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()                      # hipcc cross-compiles without a GPU
    import sgs_gnn_amd
    return sgs_gnn_amd


# ------------------------------------------------------------------------------------------------ CPU
def test_switch_and_queries_need_no_gpu(built):
    L = built._lib.lib()
    thr = L.sgs_spmm_long_rows_threshold()
    assert thr == 256                                   # a compile-time constant of the library
    first = L.sgs_spmm_long_rows_set(1)
    assert first == 1                                   # on by default
    try:
        assert L.sgs_spmm_long_rows_set(0) == 1 and L.sgs_spmm_long_rows_active(1013, 256) == 0
        assert L.sgs_spmm_long_rows_set(0) == 0
        assert L.sgs_spmm_long_rows_set(7) == 0 and L.sgs_spmm_long_rows_set(1) == 1        # any non-zero value is "on"
        assert L.sgs_spmm_long_rows_active(1013, 256) == 1 and L.sgs_spmm_long_rows_active(1037, 41) == 1
        assert L.sgs_spmm_long_rows_active(4096, 256) == 1 and L.sgs_spmm_long_rows_active(4097, 256) == 0   # large grids: plain kernels
    finally:
        L.sgs_spmm_long_rows_set(first)
    assert L.sgs_spmm_long_rows_threshold() == thr


def special_lengths(thr):
    s = [0, 1, 3, 4, 5, GU * NW - 1, GU * NW, GU * NW + 1, 2 * GU * NW - 1, 2 * GU * NW + 1, 63, 64, 65, thr - 1, thr, thr + 1,
         255, 256, 257, 700, 1000, 1036]
    # the long path itself: a wave's share is len / 4 entries in chunks of 64 and batches of 4, 6 or 8 (+- 1 entry on one wave and on all)
    s += [thr + 4 * b + d for b in (4, 6, 8, 12, 16) for d in (-1, 0, 1)] + [thr + 4 * 7 + 3, 511, 512, 513, 516, 768, 771, 900]
    return sorted(set(s))


def test_nw4_graph_has_every_edge_length_in_every_position(built):
    thr = built._lib.lib().sgs_spmm_long_rows_threshold()
    ln = nw4_lengths(thr)
    N = len(ln)
    assert N == 1037 and N % 4 != 0 and sum(ln) >= 16 * N and sum(ln) < 256 * N
    assert set(special_lengths(thr)) <= set(ln)
    long_rows = [i for i, x in enumerate(ln) if x >= thr]
    assert 0 in long_rows and N - 1 in long_rows
    assert {i % 4 for i in long_rows} == {0, 1, 2, 3}
    assert any(i + 1 in long_rows and i // 4 == (i + 1) // 4 for i in long_rows)          # two long rows in one 4-row group
    assert all(10 <= x <= 30 for x in ln if x not in special_lengths(thr))
    assert max(ln) == N - 1


# ------------------------------------------------------------------------------------------------ graphs
def nw4_lengths(thr, N=1037):
    g = torch.Generator().manual_seed(77)
    ln = torch.randint(10, 31, (N,), generator=g).tolist()
    sp = special_lengths(thr)
    long_, short = [x for x in sp if x >= thr], [x for x in sp if x < thr]
    ln[0], ln[N - 1] = 1036, 1000
    rest = [x for x in long_ if x not in (1036, 1000)]
    # long rows at i % 4 = 1, 2, 3, 0, ... over the middle of the graph; 700 and 257 side by side in one group
    pos = 41
    for t, x in enumerate(rest):
        ln[pos] = x
        pos += 4 * 5 + 1
    ln[402], ln[403] = 700, 257
    for t, x in enumerate(short):
        ln[7 + 13 * t] = x
    return ln


def build_csr(ln, seed):
    """Distinct columns per row (never the row itself), val = U(0.5, 1.5) / len; gcn_ref.PAD valid entries behind the last row."""
    N = len(ln)
    g = torch.Generator().manual_seed(seed)
    nnz = sum(ln)
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    ptr[1:] = torch.tensor(ln).cumsum(0)
    col = torch.zeros(nnz + R.PAD, dtype=torch.int32)
    for i, x in enumerate(ln):
        if x:
            c = torch.randperm(N - 1, generator=g)[:x]
            col[ptr[i]:ptr[i + 1]] = (c + (c >= i)).int()
    lens = torch.tensor(ln)
    val = torch.ones(nnz + R.PAD)
    val[:nnz] = (0.5 + torch.rand(nnz, generator=g)) / torch.repeat_interleave(lens.clamp(min=1), lens).float()
    cpu = dict(ptr=ptr.int(), col=col, val=val, nnz=nnz, N=N)
    return dict(cpu, dev={k: cpu[k].to(DEV) for k in ("ptr", "col", "val")})


@pytest.fixture(scope="module")
def graphs(pkg):
    thr = pkg._lib.lib().sgs_spmm_long_rows_threshold()
    ln4 = nw4_lengths(thr)
    g = torch.Generator().manual_seed(5)
    ln16 = torch.randint(256, 301, (301,), generator=g).tolist()
    ln16[0], ln16[150], ln16[300] = 256, 300, 257
    out = {"nw4": (4, build_csr(ln4, 1), build_csr(ln4, 2)), "nw16": (16, build_csr(ln16, 3), build_csr(ln16, 4))}
    assert out["nw16"][1]["nnz"] >= 256 * 301 and min(ln16) >= thr
    return out


# ------------------------------------------------------------------------------------------------ calls
class switch:
    def __init__(self, L, on):
        self.L, self.on = L, on

    def __enter__(self):
        self.prev = self.L.sgs_spmm_long_rows_set(self.on)

    def __exit__(self, *a):
        self.L.sgs_spmm_long_rows_set(self.prev)


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def shifted(t, off):
    buf = torch.empty(t.numel() + off + 4, dtype=torch.float32, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def dptr(t):
    return None if t is None else t.data_ptr()


def expect_variant(pkg, G, D, nw, X, Y, on):
    L = pkg._lib.lib()
    al = int(X.data_ptr() % 16 == 0 and Y.data_ptr() % 16 == 0)
    vec = 4 if (D % 4 == 0 and al) else 1
    assert L.sgs_spmm_csr_variant(G["N"], D, G["nnz"], al) == 1000 + 100 * vec + nw
    assert L.sgs_spmm_long_rows_active(G["N"], D) == int(on)
    return vec


def p_of(act):
    return R.P_DROP if act == R.ACT_RELU_DROPOUT else 0.0


def call_spmm(pkg, G, X, diag, bias, act):
    L, ops = pkg._lib.lib(), pkg.ops
    N, D, d = G["N"], X.shape[1], G["dev"]
    Y = nan(N, D)
    ops._lib.check(L.sgs_spmm_csr(X.data_ptr(), N, D, G["nnz"], d["ptr"].data_ptr(), d["col"].data_ptr(), d["val"].data_ptr(), dptr(diag),
                                  dptr(bias), act, p_of(act), SEED, SITE, Y.data_ptr(), ops._stream()), "sgs_spmm_csr")
    return [Y]


def call_next(pkg, G, X, diag, bias, act, Wn):
    L, ops = pkg._lib.lib(), pkg.ops
    N, D, d, Dn = G["N"], X.shape[1], G["dev"], Wn.shape[0]
    Y, Z = nan(N, D), nan(N, Dn)
    ops._lib.check(L.sgs_spmm_csr_next(X.data_ptr(), N, D, G["nnz"], d["ptr"].data_ptr(), d["col"].data_ptr(), d["val"].data_ptr(),
                                       dptr(diag), dptr(bias), act, p_of(act), SEED, SITE, Wn.data_ptr(), Dn, Y.data_ptr(), Z.data_ptr(),
                                       ops._stream()), "sgs_spmm_csr_next")
    return [Y, Z]


def call_bwd(pkg, G, dZ, diag, W, Yp, act):
    L, ops = pkg._lib.lib(), pkg.ops
    N, D, d = G["N"], dZ.shape[1], G["dev"]
    Dp = W.shape[1] if W is not None else 0
    dX, cs = nan(N, D), nan(D)
    dZp = nan(N, Dp) if W is not None else None
    ops._lib.check(L.sgs_spmm_csr_bwd_prev(dZ.data_ptr(), N, D, G["nnz"], d["ptr"].data_ptr(), d["col"].data_ptr(), d["val"].data_ptr(),
                                           dptr(diag), dptr(W), Dp, dptr(Yp), act if W is not None else R.ACT_NONE,
                                           p_of(act) if W is not None else 0.0, dX.data_ptr(), dptr(dZp), cs.data_ptr(), ops._stream()),
                   "sgs_spmm_csr_bwd_prev")
    return [dX, cs] + ([dZp] if W is not None else [])


def call_dual(pkg, GA, GB, XA, XB, diagA, diagB, bias, act):
    L, ops = pkg._lib.lib(), pkg.ops
    N, D, a, b = GA["N"], XA.shape[1], GA["dev"], GB["dev"]
    YA, YB = nan(N, D), nan(N, D)
    ops._lib.check(L.sgs_spmm_csr_dual(XA.data_ptr(), XB.data_ptr(), N, D, dptr(bias), act, p_of(act), SITE,
                                       GA["nnz"], a["ptr"].data_ptr(), a["col"].data_ptr(), a["val"].data_ptr(), dptr(diagA), SEED, YA.data_ptr(),
                                       GB["nnz"], b["ptr"].data_ptr(), b["col"].data_ptr(), b["val"].data_ptr(), dptr(diagB), SEED + 1,
                                       YB.data_ptr(), ops._stream()), "sgs_spmm_csr_dual")
    return [YA, YB]


def call_next_dual(pkg, GA, GB, X, diagA, diagB, bias, act, Wn):
    L, ops = pkg._lib.lib(), pkg.ops
    N, D, a, b, Dn = GA["N"], X.shape[1], GA["dev"], GB["dev"], Wn.shape[0]
    YA, YB, ZA, ZB = nan(N, D), nan(N, D), nan(N, Dn), nan(N, Dn)
    ops._lib.check(L.sgs_spmm_csr_next_dual(X.data_ptr(), N, D, dptr(bias), act, p_of(act), SITE, Wn.data_ptr(), Dn,
                                            GA["nnz"], a["ptr"].data_ptr(), a["col"].data_ptr(), a["val"].data_ptr(), dptr(diagA), SEED,
                                            YA.data_ptr(), ZA.data_ptr(),
                                            GB["nnz"], b["ptr"].data_ptr(), b["col"].data_ptr(), b["val"].data_ptr(), dptr(diagB), SEED + 1,
                                            YB.data_ptr(), ZB.data_ptr(), ops._stream()), "sgs_spmm_csr_next_dual")
    return [YA, ZA, YB, ZB]


def on_off_on(pkg, fn):
    """fn() with the switch on, off, on -> the on result, after asserting all three bitwise equal and fully written."""
    L = pkg._lib.lib()
    with switch(L, 1):
        a = fn()
    with switch(L, 0):
        b = fn()
    with switch(L, 1):
        a2 = fn()
    torch.cuda.synchronize()
    for t, (x, y, x2) in enumerate(zip(a, b, a2)):
        assert not bool(torch.isnan(y).any()), f"output {t}: the plain kernel left elements unwritten"
        assert torch.equal(x, y), f"output {t}: long-row path differs from the plain loop ({int((x != y).sum())} elements)"
        assert torch.equal(x, x2), f"output {t}: long-row path not run-to-run bitwise"
    return a


# D: 256 / 64 one column block at VEC 4 (full / a quarter); 320 a second, partly filled block; 41 / 30 VEC 1, partly filled;
# "256u": X one float off 16-byte alignment -> VEC 1, four column blocks
WIDTHS = [256, 320, 64, 41, 30, "256u"]
COMBOS = R.SPMM_COMBOS          # (diag, bias, act): every activation, with and without diag and bias


def inputs(G, width, act, seed=5):
    D = 256 if width == "256u" else width
    off = 1 if width == "256u" else 0
    X, diag, bias = R.spmm_inputs(G["N"], D, R.DROP_BIAS if act == R.ACT_RELU_DROPOUT else 0.0, seed=seed)
    return D, X, diag, bias, off


@gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("gname", ["nw4", "nw16"])
def test_spmm_csr_on_vs_off_and_against_fp64(pkg, graphs, gname, width):
    ops = pkg.ops
    nw, G, _ = graphs[gname]
    n = G["nnz"]
    ptr, col, val = G["ptr"], G["col"][:n], G["val"][:n]
    for t, (diag_on, bias_on, act) in enumerate(COMBOS):
        D, X, diag, bias, off = inputs(G, width, act)
        diag, bias = (diag if diag_on else None), (bias if bias_on else None)
        Xd = shifted(X, off)
        dd, bd = (None if diag is None else diag.to(DEV)), (None if bias is None else bias.to(DEV))
        (Y,) = on_off_on(pkg, lambda: call_spmm(pkg, G, Xd, dd, bd, act))
        vec = expect_variant(pkg, G, D, nw, Xd, Y, True)
        assert vec == (1 if (width == "256u" or D % 4) else 4)
        if t >= 3:
            continue
        # fp64, independent of the code under test: the bound of the variant-table tests
        drop = act == R.ACT_RELU_DROPOUT
        keep = ops.dropout_keep(SEED, SITE, G["N"], D, R.P_DROP, DEV).cpu() if drop else None
        Z = R.spmm_pre(ptr, col, val.double(), None if diag is None else diag.double(), None if bias is None else bias.double(), X.double())
        pb = R.spmm_pre_bound(ptr, col, val, diag, bias, X)
        Yref = R.activate(Z, act, keep, R.P_DROP)
        err = (Y.double().cpu() - Yref).abs()
        bad = ~(err <= R.spmm_bound(pb, Yref, act, R.P_DROP))
        assert not bool(bad.any()), f"{gname} D={width} combo {t}: {int(bad.sum())} elements out of bound, rows {torch.nonzero(bad)[:4, 0].tolist()}"


@gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("gname", ["nw4", "nw16"])
def test_pair_kernels_on_vs_off(pkg, graphs, gname, width):
    """sgs_spmm_csr_next, and sgs_spmm_csr_bwd_prev with and without the previous layer's product (column sums in both)."""
    nw, G, _ = graphs[gname]
    g = torch.Generator().manual_seed(9)
    for diag_on, bias_on, act in COMBOS:
        D, X, diag, bias, off = inputs(G, width, act)
        Dn = 41 if D >= 64 else 64
        Xd = shifted(X, off)
        dd, bd = (diag.to(DEV) if diag_on else None), (bias.to(DEV) if bias_on else None)
        Wn = torch.randn(Dn, D, generator=g).to(DEV)
        Y, Z = on_off_on(pkg, lambda: call_next(pkg, G, Xd, dd, bd, act, Wn))
        expect_variant(pkg, G, D, nw, Xd, Y, True)
        with switch(pkg._lib.lib(), 1):
            assert torch.equal(Y, call_spmm(pkg, G, Xd, dd, bd, act)[0])              # (and so inside the fp64 bound checked above)
        W = torch.randn(D, Dn, generator=g).to(DEV)
        Yp = torch.relu(torch.randn(G["N"], Dn, generator=g)).to(DEV)
        on_off_on(pkg, lambda: call_bwd(pkg, G, Xd, dd, W, Yp, act))
        on_off_on(pkg, lambda: call_bwd(pkg, G, Xd, dd, None, None, R.ACT_NONE))


@gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("gname", ["nw4", "nw16"])
def test_two_job_kernels_on_vs_off(pkg, graphs, gname, width):
    """sgs_spmm_csr_dual and sgs_spmm_csr_next_dual: two graphs of the same row lengths, different columns, weights and dropout seeds."""
    L = pkg._lib.lib()
    nw, GA, GB = graphs[gname]
    g = torch.Generator().manual_seed(10)
    for diag_on, bias_on, act in COMBOS:
        D, XA, diag, bias, off = inputs(GA, width, act)
        _, XB, diagB, _, _ = inputs(GB, width, act, seed=6)
        Dn = 41 if D >= 64 else 64
        assert L.sgs_gcn_dual_ok(GA["N"], GA["nnz"], GB["nnz"], D, Dn) == 1
        XAd, XBd = shifted(XA, off), shifted(XB, off)
        da, db = (diag.to(DEV) if diag_on else None), (diagB.to(DEV) if diag_on else None)
        bd = bias.to(DEV) if bias_on else None
        Wn = torch.randn(Dn, D, generator=g).to(DEV)
        YA, YB = on_off_on(pkg, lambda: call_dual(pkg, GA, GB, XAd, XBd, da, db, bd, act))
        expect_variant(pkg, GA, D, nw, XAd, YA, True)
        YA2, ZA, YB2, ZB = on_off_on(pkg, lambda: call_next_dual(pkg, GA, GB, XAd, da, db, bd, act, Wn))
        with switch(L, 1):
            assert torch.equal(YA, call_spmm(pkg, GA, XAd, da, bd, act)[0]) and torch.equal(YA2, YA)
            one = call_next(pkg, GA, XAd, da, bd, act, Wn)
            assert torch.equal(one[0], YA2) and torch.equal(one[1], ZA)


# ------------------------------------------------------------------------------------------------ model level
def _gnn(M, Fin, H, C, p):
    m = M.GNNModel.__new__(M.GNNModel)
    torch.nn.Module.__init__(m)
    torch.manual_seed(3)
    m.gcn1, m.gcn2, m.dropout = M.GCNConv(Fin, H), M.GCNConv(H, C), torch.nn.Dropout(p)
    with torch.no_grad():
        m.gcn1.bias.uniform_(-0.2, 0.2)
        m.gcn2.bias.uniform_(-0.2, 0.2)
    return m.to(DEV).train()


@gpu
def test_gnn_model_on_a_skewed_partition_is_bitwise_the_same_on_and_off(pkg):
    """GNNModel forward + backward at the S3 shape (N = 1013, H = 256, C = 41) on a power-law partition of ~60 000 edges whose hub rows
    have 900+ entries against a mean of ~60: logits and every gradient, switch on vs off."""
    from sgs_gnn_amd import model as M
    ops, L = pkg.ops, pkg._lib.lib()
    N, Fin, H, C = 1013, 128, 256, 41
    b = pkg.synthetic_graph(N, 60128, Fin, C, 1000 * 1000 + 41)                     # the S3 stream's smallest partition
    ei = b.edge_index
    deg = torch.bincount(ei[1], minlength=N)
    assert int(deg.max()) >= 900 and int((deg >= L.sgs_spmm_long_rows_threshold()).sum()) >= 10
    assert L.sgs_gcn_pair_ok(N, ei.shape[1], H) == 1 and L.sgs_gcn_pair_ok(N, ei.shape[1], C) == 1
    g = torch.Generator().manual_seed(11)
    ei = ei.to(DEV)
    w = torch.rand(ei.shape[1], generator=g).to(DEV)

    class D_:
        pass
    data = D_()
    data.x = b.x.to(DEV)
    gy = torch.randn(N, C, generator=g).to(DEV)

    def run(on):
        with switch(L, on):
            assert L.sgs_spmm_long_rows_active(N, H) == on
            m = _gnn(M, Fin, H, C, 0.3)
            M.set_dropout_seed(99)
            ops.new_memo_scope()
            wd = w.clone().requires_grad_(True)
            out = m(data, ei, wd)
            out.backward(gy)
            torch.cuda.synchronize()
        return [out.detach(), wd.grad, m.gcn1.lin.weight.grad, m.gcn1.bias.grad, m.gcn2.lin.weight.grad, m.gcn2.bias.grad]

    a, off, a2 = run(1), run(0), run(1)
    for n, x, y, x2 in zip(["logits", "d w", "d W1", "d b1", "d W2", "d b2"], a, off, a2):
        assert bool(torch.isfinite(x).all()), n
        assert torch.equal(x, y), f"{n}: long-row path differs from the plain loop"
        assert torch.equal(x, x2), f"{n}: long-row path not run-to-run bitwise"
