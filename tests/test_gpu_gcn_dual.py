"""GPU: the two-job forms of the GNN head's two forward launches (sgs_spmm_csr_next_dual, sgs_spmm_csr_dual), ops.gcn2_dual and the
captured sampled step built on them, against the single-job calls / two gcn2 nodes / the two-launch step they replace.

Two jobs per launch leave every job's arithmetic as it was (same entry order, same fixed-order combination of the wave partials, same
product order, same dropout hash), so every comparison here is torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SITE = 3


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


def _graph(pkg, n, E, seed, empty_row=None, weighted=True):
    """n nodes, E random edges (src -> dst); `empty_row`: a node that is nobody's dst (an in-CSR row without neighbours)."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (E,), generator=g)
    if empty_row is None:
        dst = torch.randint(0, n, (E,), generator=g)
    else:
        dst = torch.randint(0, n - 1, (E,), generator=g)
        dst = dst + (dst >= empty_row).long()
    ei = torch.stack([src, dst]).to(DEV)
    gr = pkg.ops.Graph(ei, n)
    w = torch.rand(E, generator=g).to(DEV) if weighted else None
    return ei, gr, pkg.ops.gcn_norm(gr, w), w


def _single(pkg, X, gr, nm, b1, act, p, seed, Wn, b2):
    """(Y, Z, out) of the single-job calls: sgs_spmm_csr_next, then sgs_spmm_csr over Z."""
    L, ops = pkg._lib.lib(), pkg.ops
    n, D = X.shape
    Dn = Wn.shape[0]
    Y, Z, out = torch.empty(n, D, device=DEV), torch.empty(n, Dn, device=DEV), torch.empty(n, Dn, device=DEV)
    ops._lib.check(L.sgs_spmm_csr_next(X.data_ptr(), n, D, gr.n_edges, gr.in_ptr.data_ptr(), gr.in_src.data_ptr(), nm.what_in.data_ptr(),
                                       nm.what_loop.data_ptr(), b1.data_ptr(), act, p, seed, SITE, Wn.data_ptr(), Dn, Y.data_ptr(), Z.data_ptr(),
                                       ops._stream()), "sgs_spmm_csr_next")
    ops._lib.check(L.sgs_spmm_csr(Z.data_ptr(), n, Dn, gr.n_edges, gr.in_ptr.data_ptr(), gr.in_src.data_ptr(), nm.what_in.data_ptr(),
                                  nm.what_loop.data_ptr(), b2.data_ptr(), ops.ACT_NONE, 0.0, 0, 0, out.data_ptr(), ops._stream()), "sgs_spmm_csr")
    return Y, Z, out


def _dual(pkg, X, ja, jb, b1, act, p, Wn, b2):
    """((Y, Z, out) of job a, the same of job b) from the two two-job launches; j = (gr, nm, seed)."""
    L, ops = pkg._lib.lib(), pkg.ops
    n, D = X.shape
    Dn = Wn.shape[0]
    (ga, na, sa), (gb, nb, sb) = ja, jb
    Y = [torch.empty(n, D, device=DEV) for _ in range(2)]
    Z = [torch.empty(n, Dn, device=DEV) for _ in range(2)]
    out = [torch.empty(n, Dn, device=DEV) for _ in range(2)]
    ops._lib.check(L.sgs_spmm_csr_next_dual(X.data_ptr(), n, D, b1.data_ptr(), act, p, SITE, Wn.data_ptr(), Dn,
                                            ga.n_edges, ga.in_ptr.data_ptr(), ga.in_src.data_ptr(), na.what_in.data_ptr(), na.what_loop.data_ptr(),
                                            sa, Y[0].data_ptr(), Z[0].data_ptr(),
                                            gb.n_edges, gb.in_ptr.data_ptr(), gb.in_src.data_ptr(), nb.what_in.data_ptr(), nb.what_loop.data_ptr(),
                                            sb, Y[1].data_ptr(), Z[1].data_ptr(), ops._stream()), "sgs_spmm_csr_next_dual")
    ops._lib.check(L.sgs_spmm_csr_dual(Z[0].data_ptr(), Z[1].data_ptr(), n, Dn, b2.data_ptr(), ops.ACT_NONE, 0.0, 0,
                                       ga.n_edges, ga.in_ptr.data_ptr(), ga.in_src.data_ptr(), na.what_in.data_ptr(), na.what_loop.data_ptr(), 0,
                                       out[0].data_ptr(),
                                       gb.n_edges, gb.in_ptr.data_ptr(), gb.in_src.data_ptr(), nb.what_in.data_ptr(), nb.what_loop.data_ptr(), 0,
                                       out[1].data_ptr(), ops._stream()), "sgs_spmm_csr_dual")
    return (Y[0], Z[0], out[0]), (Y[1], Z[1], out[1])


def _check_kernels(pkg, n, D, Dn, Ea, Eb, drop, empty_row):
    ops = pkg.ops
    _, ga, na, _ = _graph(pkg, n, Ea, 21)
    _, gb, nb, _ = _graph(pkg, n, Eb, 22, empty_row=empty_row, weighted=False)
    assert pkg._lib.lib().sgs_gcn_dual_ok(n, ga.n_edges, gb.n_edges, D, Dn) == 1
    if empty_row is not None:
        ptr = gb.in_ptr.tolist()
        assert ptr[empty_row] == ptr[empty_row + 1] and ga.n_edges != gb.n_edges
    g = torch.Generator().manual_seed(5)
    X = torch.randn(n, D, generator=g).to(DEV)
    Wn = (torch.randn(Dn, D, generator=g) / D ** 0.5).to(DEV)
    b1, b2 = (0.2 * torch.randn(D, generator=g)).to(DEV), (0.2 * torch.randn(Dn, generator=g)).to(DEV)
    act, p, sa, sb = (ops.ACT_RELU_DROPOUT, 0.3, 1234567, 7654321) if drop else (ops.ACT_RELU, 0.0, 0, 0)
    ra = _single(pkg, X, ga, na, b1, act, p, sa, Wn, b2)
    rb = _single(pkg, X, gb, nb, b1, act, p, sb, Wn, b2)
    da, db = _dual(pkg, X, (ga, na, sa), (gb, nb, sb), b1, act, p, Wn, b2)
    for job, r, d in (("a", ra, da), ("b", rb, db)):
        for name, u, v in zip(("Y", "Z", "out"), r, d):
            assert torch.equal(u, v), f"job {job}: {name} differs from the single-job call"
    if drop:
        assert not torch.equal((da[0] == 0), (db[0] == 0))        # two seeds: two masks
        assert (da[0] == 0).float().mean() > 0.3


@pytest.mark.parametrize("drop", [True, False])
@pytest.mark.parametrize("Dn", [41, 7])
@pytest.mark.parametrize("D", [256, 64, 30])
def test_two_job_launches_vs_single_job_calls(pkg, D, Dn, drop):
    """N = 37 (not a multiple of the 4-row group; 10 x 2 workgroups), graph b with another nnz and a row without neighbours; D = 30: VEC = 1."""
    _check_kernels(pkg, 37, D, Dn, 20 * 37, 24 * 37 + 5, drop, empty_row=11)


def test_two_job_launches_at_the_benchmarked_shape(pkg):
    """N = 1 013, H = 256, C = 41, 100 000 edges per graph: the layer-1 grid of 2 x 254 workgroups."""
    _check_kernels(pkg, 1013, 256, 41, 100000, 100000, True, empty_row=None)


def _params(H, F, C, seed=3):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=g) / s[-1] ** 0.5).to(DEV).requires_grad_(True)
    return mk(H, F), (0.2 * torch.randn(H, generator=g)).to(DEV).requires_grad_(True), mk(C, H), \
        (0.2 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)


def _two_nodes(ops, x, P, nm_a, nm_b, act, p, sa, sb):
    out_a, xl1 = ops.gcn2(x, *P, nm_a, act=act, p=p, seed=sa, site=SITE)
    out_b, _ = ops.gcn2(x, *P, nm_b, act=act, p=p, seed=sb, site=SITE, xl1=xl1)
    return out_a, out_b


def test_mismatched_variants_fall_back_to_two_single_calls(pkg):
    """nnz >= 256 N for graph a only: the jobs would run different kernel variants, so the query says no, the entry point refuses
    and gcn2_dual is the two gcn2 calls."""
    ops, L = pkg.ops, pkg._lib.lib()
    n, F, H, C = 37, 20, 64, 7
    _, ga, _, wa = _graph(pkg, n, 260 * n, 31)
    _, gb, nb, _ = _graph(pkg, n, 20 * n, 32, weighted=False)
    assert ga.n_edges >= 256 * n > gb.n_edges >= 16 * n
    assert L.sgs_gcn_dual_ok(n, ga.n_edges, gb.n_edges, H, C) == 0 and not ops.gcn_dual_ok(ga, gb, H, C)
    assert L.sgs_gcn_dual_ok(n, gb.n_edges, gb.n_edges, H, C) == 1 and L.sgs_gcn_dual_ok(n, ga.n_edges, ga.n_edges, H, C) == 1
    rc = L.sgs_spmm_csr_next_dual(None, n, H, None, 0, 0.0, 0, None, C, ga.n_edges, None, None, None, None, 0, None, None,
                                  gb.n_edges, None, None, None, None, 0, None, None, None)
    assert rc == -1 and b"variant" in L.sgs_last_error()
    x = torch.randn(n, F, generator=torch.Generator().manual_seed(1)).to(DEV)
    P = _params(H, F, C)
    na = ops.gcn_norm(ga, wa)
    with torch.no_grad():
        ra, rb = _two_nodes(ops, x, P, na, nb, ops.ACT_RELU_DROPOUT, 0.3, 11, 12)
        n0 = ops.GCN_DUAL_FORWARDS["shared"]
        da, db, _ = ops.gcn2_dual(x, *P, na, nb, act=ops.ACT_RELU_DROPOUT, p=0.3, seed_a=11, seed_b=12, site=SITE)
    assert ops.GCN_DUAL_FORWARDS["shared"] == n0                      # the fall-back: two single calls
    assert torch.equal(ra, da) and torch.equal(rb, db)


@pytest.mark.parametrize("order", ["a", "b", "ab", "sum"])
def test_gcn2_dual_autograd_vs_two_gcn2_nodes(pkg, order):
    """gcn2_dual (two launches for both forwards) against two gcn2 calls (four), with edge weights that require a gradient on branch a:
    a alone, b alone, a then b with retain_graph, and both in one backward call.  Every gradient bitwise equal, and None where the two
    calls leave None (b alone: nothing behind the edge weights may run)."""
    ops = pkg.ops
    n, F, H, C = 37, 20, 64, 7
    _, ga, _, wa = _graph(pkg, n, 20 * n, 41)
    _, gb, nb, _ = _graph(pkg, n, 24 * n + 5, 42, empty_row=11, weighted=False)
    assert ops.gcn_dual_ok(ga, gb, H, C)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, F, generator=g).to(DEV)
    gya, gyb = torch.randn(n, C, generator=g).to(DEV), torch.randn(n, C, generator=g).to(DEV)

    def run(dual):
        P = _params(H, F, C)
        w = wa.clone().requires_grad_(True)
        na = ops.gcn_norm(ga, w)
        ops.new_memo_scope()
        if dual:
            n0 = ops.GCN_DUAL_FORWARDS["shared"]
            out_a, out_b, _ = ops.gcn2_dual(x, *P, na, nb, act=ops.ACT_RELU_DROPOUT, p=0.3, seed_a=11, seed_b=12, site=SITE)
            assert ops.GCN_DUAL_FORWARDS["shared"] == n0 + 1         # the two-job launches ran
        else:
            out_a, out_b = _two_nodes(ops, x, P, na, nb, ops.ACT_RELU_DROPOUT, 0.3, 11, 12)
        if order == "a":
            out_a.backward(gya)
        elif order == "b":
            out_b.backward(gyb)
        elif order == "ab":
            out_a.backward(gya, retain_graph=True)
            out_b.backward(gyb)
        else:                                           # one backward over both branches
            torch.autograd.backward([out_a, out_b], [gya, gyb])
        return [out_a.detach(), out_b.detach()] + [t.grad for t in (*P, w)]

    names = ["out_a", "out_b", "d W1", "d b1", "d W2", "d b2", "d w"]
    for name, u, v in zip(names, run(False), run(True)):
        if u is None:
            assert v is None, f"{name}: the two-node form leaves it None"
        else:
            assert v is not None and torch.equal(u, v), name
    if order == "b":
        assert run(True)[-1] is None                    # the random branch reaches no edge weight


def test_captured_step_with_and_without_shared_launches(pkg):
    """A hybrid run on captured HIP graphs, the switch off and on from the same seeds: bitwise the same parameters and train() results,
    with both outcomes of the gate among the steps (from the returned update counts)."""
    from test_gpu_stepgraph import _args, _batches
    S, ops = pkg, pkg.ops
    crit = torch.nn.CrossEntropyLoss()
    n, q, epochs = 120, 2000, 5                          # q >= 16 n: both sampled graphs are on the row-block path
    bs = _batches(S, [5000, 900, 4000], n=n)
    results = []
    try:
        for on in (False, True):
            ops.set_gcn_dual(on)
            n0 = ops.GCN_DUAL_FORWARDS["shared"]
            torch.manual_seed(CAPTURE_SEED)
            S.fix_seeds(CAPTURE_SEED)
            m = S.GNNModel(24, 32, 5, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
            og = S.FusedAdam([p for k, p in m.named_parameters() if "gcn" in k], lr=1e-2)
            oe = S.FusedAdam([p for k, p in m.named_parameters() if "edge_prob_mlp" in k], lr=1e-2)
            a = _args(sgs_hipgraph=True)
            rets = [S.train(a, ep, epochs, m, og, oe, None, crit, bs, q=q) for ep in range(epochs)]
            assert m._sgs_stepgraphs.slots[True]
            assert (ops.GCN_DUAL_FORWARDS["shared"] > n0) == on       # the captured sampled step holds the shared launches, or not
            results.append((rets, {k: p.detach().clone() for k, p in m.named_parameters()}))
    finally:
        ops.set_gcn_dual(True)
    (r_off, p_off), (r_on, p_on) = results
    learned = sum(r[2] for r in r_off)
    print("learned steps per epoch (switch off):", [r[2] for r in r_off], "(switch on):", [r[2] for r in r_on])
    assert 0 < learned < 2 * epochs, "the gate took one branch only: choose another CAPTURE_SEED"
    assert r_on == r_off
    for k in p_on:
        assert torch.equal(p_on[k], p_off[k]), k


CAPTURE_SEED = 3
