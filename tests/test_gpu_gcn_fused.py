"""GPU: the GCN layer-pair kernels (sgs_spmm_csr_next, sgs_spmm_csr_bwd_prev) against the unfused composition they replace
(sgs_spmm_csr + a dense product + sgs_act_bwd_colsum / sgs_colsum), and GNNModel with the fused pair against the unfused layers.

The fp32 products (Z = Y Wn^T, dZp = (dX W) * act') sum in the order of the library GEMMs they replace at the GNN head's shapes
(N = 1013, H = 256, C = 41): there they are bitwise torch's products, and so is a whole forward + backward of GNNModel.  At every other
shape they are held to |err| <= n * 2^-24 * (|A| |B|)[i, j] against a float64 product, n the contraction length -- the textbook bound
for a length-n fp32 dot product in any summation order.  Everything else is bitwise."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 1013                     # a METIS partition's row count: not a multiple of the 4 rows a workgroup owns


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


def partition_graph(pkg, per_row, seed, loops):
    """N nodes, ~per_row entries per row, rows 0..4 and N-3..N-1 without in- or out-edges, unit or random weights; the normalisation
    with (loops) or without its self-loop term."""
    g = torch.Generator().manual_seed(seed)
    E = per_row * N
    ei = torch.randint(5, N - 3, (2, E), generator=g)
    gr = pkg.ops.Graph(ei.to(DEV), N)
    w = torch.rand(E, generator=g).to(DEV)
    nm = pkg.ops.gcn_norm(gr, w)
    assert pkg._lib.lib().sgs_gcn_pair_ok(N, gr.n_edges, 256) == 1
    diag = nm.what_loop if loops else None
    return gr, nm, diag, g


def prod_bound(A, B):
    """n 2^-24 (|A| |B|) for the fp32 product A B (contraction length n)."""
    n = A.shape[1]
    return n * 2.0 ** -24 * (A.double().abs() @ B.double().abs()) + 1e-30


def spmm_next(pkg, X, gr, nm, diag, bias, act, p, seed, Wn):
    L = pkg._lib.lib()
    ops = pkg.ops
    D, Dn = X.shape[1], Wn.shape[0]
    Y = torch.empty(N, D, device=DEV)
    Z = torch.empty(N, Dn, device=DEV)
    ops._lib.check(L.sgs_spmm_csr_next(X.data_ptr(), N, D, gr.n_edges, gr.in_ptr.data_ptr(), gr.in_src.data_ptr(), nm.what_in.data_ptr(),
                                       ops._ptr(diag), ops._ptr(bias), act, p, seed, 3, Wn.data_ptr(), Dn, Y.data_ptr(), Z.data_ptr(),
                                       ops._stream()), "sgs_spmm_csr_next")
    return Y, Z


def spmm_bwd_prev(pkg, dZ, gr, nm, diag, W, Yp, act, p, colsum=True):
    L = pkg._lib.lib()
    ops = pkg.ops
    D = dZ.shape[1]
    Dp = W.shape[1] if W is not None else 0
    dX = torch.empty(N, D, device=DEV)
    dZp = torch.empty(N, Dp, device=DEV) if W is not None else None
    cs = torch.empty(D, device=DEV) if colsum else None
    ops._lib.check(L.sgs_spmm_csr_bwd_prev(dZ.data_ptr(), N, D, gr.n_edges, gr.out_ptr.data_ptr(), gr.out_dst.data_ptr(),
                                           nm.what_out.data_ptr(), ops._ptr(diag), ops._ptr(W), Dp, ops._ptr(Yp), act, p, dX.data_ptr(),
                                           ops._ptr(dZp), ops._ptr(cs), ops._stream()), "sgs_spmm_csr_bwd_prev")
    return dX, dZp, cs


CASES = [(D, Dn, per_row, loops, p) for D in (41, 256) for Dn in (41, 256) for per_row, loops, p in ((100, True, 0.3), (350, False, 0.0))]
CASES += [(256, 41, 100, False, 0.3), (41, 256, 350, True, 0.3), (256, 41, 300, True, 0.0)]


@pytest.mark.parametrize("D,Dn,per_row,loops,p", CASES)
def test_spmm_next_vs_spmm_then_product(pkg, D, Dn, per_row, loops, p):
    ops = pkg.ops
    gr, nm, diag, g = partition_graph(pkg, per_row, D * 7 + Dn + per_row, loops)
    X = torch.randn(N, D, generator=g).to(DEV)
    bias = (torch.rand(D, generator=g) - 0.3).to(DEV)
    Wn = torch.randn(Dn, D, generator=g).to(DEV)
    act = ops.ACT_RELU_DROPOUT if p > 0 else ops.ACT_RELU
    seed = 0x1234567 + D
    Y, Z = spmm_next(pkg, X, gr, nm, diag, bias, act, p, seed, Wn)
    Yref = ops._spmm(X, gr.in_ptr, gr.in_src, nm.what_in, diag, bias, act, p, seed, 3, N, D, gr.n_edges)
    torch.cuda.synchronize()
    assert torch.equal(Y, Yref)                                    # gather order, wave sum, bias, ReLU and the dropout pattern
    Zref = Yref.double() @ Wn.double().t()
    assert bool(((Z.double() - Zref).abs() <= prod_bound(Yref, Wn.t())).all())
    if (D, Dn) == (256, 41):                                       # the GNN head's h1 W2^T: bitwise the library GEMM
        assert torch.equal(Z, Yref @ Wn.t())
    Y2, Z2 = spmm_next(pkg, X, gr, nm, diag, bias, act, p, seed, Wn)
    assert torch.equal(Y2, Y) and torch.equal(Z2, Z)


@pytest.mark.parametrize("D,Dp,per_row,loops,p", CASES)
def test_spmm_bwd_prev_vs_spmm_product_act_bwd_colsum(pkg, D, Dp, per_row, loops, p):
    ops = pkg.ops
    gr, nm, diag, g = partition_graph(pkg, per_row, D * 5 + Dp + per_row, loops)
    dZ = torch.randn(N, D, generator=g).to(DEV)
    W = torch.randn(D, Dp, generator=g).to(DEV)
    Yp = torch.relu(torch.randn(N, Dp, generator=g)).to(DEV)           # about half the activations off
    act = ops.ACT_RELU_DROPOUT if p > 0 else ops.ACT_RELU
    dX, dZp, cs = spmm_bwd_prev(pkg, dZ, gr, nm, diag, W, Yp, act, p)
    dXref = ops._spmm(dZ, gr.out_ptr, gr.out_dst, nm.what_out, diag, None, ops.ACT_NONE, 0.0, 0, 0, N, D, gr.n_edges)
    csref = ops._colsum(dZ)
    dZp_lib, cs_act = ops._act_bwd_colsum(dXref @ W, Yp, act, p)
    torch.cuda.synchronize()
    assert torch.equal(dX, dXref)
    assert torch.equal(cs, csref)
    scale = 1.0 / (1.0 - p)
    mask = (Yp > 0).double() * scale
    ref = (dXref.double() @ W.double()) * mask
    assert bool(((dZp.double() - ref).abs() <= prod_bound(dXref, W) * scale).all())
    assert bool((dZp[Yp <= 0] == 0).all())
    if (D, Dp) == (41, 256):                                       # the GNN head's (dxl2 W2) * act'(h1): bitwise the library GEMM's
        assert torch.equal(dZp, dZp_lib)
    # the previous layer's bias gradient, summed from dZp in the following launch, against sgs_act_bwd_colsum's: the products' bound
    # summed over the rows plus twice an N-term fp32 sum's
    _, _, cs_p = spmm_bwd_prev(pkg, dZp, gr, nm, diag, None, None, ops.ACT_NONE, 0.0)
    tol = (prod_bound(dXref, W) * mask).sum(0) * 2 + 2 * N * 2.0 ** -24 * ref.abs().sum(0)
    assert bool(((cs_p.double() - cs_act.double()).abs() <= tol).all())
    dX2, dZp2, cs2 = spmm_bwd_prev(pkg, dZ, gr, nm, diag, W, Yp, act, p)
    assert torch.equal(dX2, dX) and torch.equal(dZp2, dZp) and torch.equal(cs2, cs)
    dX3, _, cs3 = spmm_bwd_prev(pkg, dZ, gr, nm, diag, None, None, ops.ACT_NONE, 0.0, colsum=False)
    assert torch.equal(dX3, dX) and cs3 is None


def test_pair_entry_points_refuse_shapes_off_the_row_block_path(pkg):
    L = pkg._lib.lib()
    assert L.sgs_gcn_pair_ok(N, 15 * N, 256) == 0              # short rows: sgs_spmm_csr's row-per-lanes kernel
    assert L.sgs_gcn_pair_ok(70000, 16 * 70000, 256) == 0      # too many rows
    assert L.sgs_gcn_pair_ok(N, 16 * N, 513) == 0              # a row wider than the LDS copy
    assert L.sgs_gcn_pair_ok(N, 16 * N, 512) == 1
    rc = L.sgs_spmm_csr_next(None, N, 256, 15 * N, None, None, None, None, None, 0, 0.0, 0, 0, None, 41, None, None, None)
    assert rc == -1 and b"row-block" in L.sgs_last_error()


def _gnn(M, Fin, H, C, p):
    m = M.GNNModel.__new__(M.GNNModel)
    torch.nn.Module.__init__(m)
    torch.manual_seed(3)
    m.gcn1, m.gcn2, m.dropout = M.GCNConv(Fin, H), M.GCNConv(H, C), torch.nn.Dropout(p)
    with torch.no_grad():
        m.gcn1.bias.uniform_(-0.2, 0.2)
        m.gcn2.bias.uniform_(-0.2, 0.2)
    return m.to(DEV).train()


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("per_row", [100, 350])
def test_gnn_model_fused_pair_vs_unfused_layers_at_partition_size(pkg, monkeypatch, p, per_row):
    """GNNModel forward + backward at the S3 shape (N = 1013, H = 256, C = 41, ~100 / ~350 entries per row), fused pair vs the unfused calls:
    bitwise equal, output and every gradient."""
    from sgs_gnn_amd import model as M
    ops = pkg.ops
    Fin, H, C = 128, 256, 41
    g = torch.Generator().manual_seed(11)
    E = per_row * N
    ei = torch.randint(0, N, (2, E), generator=g).to(DEV)
    w = torch.rand(E, generator=g).to(DEV)

    class D_:
        pass
    data = D_()
    data.x = torch.randn(N, Fin, generator=g).to(DEV)
    gy = torch.randn(N, C, generator=g).to(DEV)

    def run(fused):
        if not fused:
            monkeypatch.setattr(ops, "_pair_ok", lambda *a: False)
        m = _gnn(M, Fin, H, C, p)
        M.set_dropout_seed(99)
        ops.new_memo_scope()
        wd = w.clone().requires_grad_(True)
        out = m(data, ei, wd)
        out.backward(gy)
        monkeypatch.undo()
        return [out.detach(), wd.grad, m.gcn1.lin.weight.grad, m.gcn1.bias.grad, m.gcn2.lin.weight.grad, m.gcn2.bias.grad]

    a, b, a2 = run(True), run(False), run(True)
    names = ["out", "d w", "d W1", "d b1", "d W2", "d b2"]
    for n, x, y, x2 in zip(names, a, b, a2):
        assert torch.equal(x, x2), f"{n}: fused pair not run-to-run bitwise"
        assert torch.equal(x, y), f"{n}: fused pair differs from the unfused layers"
