"""GPU: the Chebyshev head of order K > 1 (ops.cheb_norm / ops.cheb_conv / ChebModel(cheb_k=K)) against the fp64 dense restatement in
tests/cheb_ref.py (direct T_k recurrence + torch autograd; the product runs Clenshaw's recurrence at the output width, so the two share
no algebra).  Tolerances are the heads' own (tests/test_gpu_heads.py): logits < 1e-4 absolute, every gradient -- the edge weights'
included -- within 2e-4 (1 + max |ref|).  These are model-level checks of the autograd plumbing; every kernel variant behind sgs_cheb_spmm
and the two normalisation entry points are held to fp64 element by element in tests/test_gpu_cheb_kernels.py (references, bounds and case
tables: tests/cheb_kernels_ref.py; coverage of the tables: tests/test_cheb_variant_table.py)."""
import argparse
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _small_graph(S, f=9, seed=3):
    """synthetic_graph(70, 600, seed 3) + 5 duplicated edges + 3 self loops appended.  The duplicates make the list directed (L_hat is
    not symmetric); the seed is chosen so that a node without out-edges exists (dis = 0 there)."""
    b = S.synthetic_graph(70, 600, f, 4, seed=seed)
    ei = torch.cat([b.edge_index, b.edge_index[:, :5], torch.tensor([[5, 17, 17], [5, 17, 17]])], dim=1).contiguous()
    nonloop = ei[:, ei[0] != ei[1]]
    outdeg = torch.bincount(nonloop[0], minlength=70)
    assert int((outdeg == 0).sum()) > 0, "pick a seed with a node of out-degree 0"
    return b, ei, int((outdeg == 0).nonzero()[0])


def _weights(n, seed=5):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.05


def _close(got, ref, name):
    err = float((got.detach().cpu().double() - ref).abs().max())
    bound = 2e-4 * (1.0 + float(ref.abs().max()))
    print(f"{name}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, name


def test_cheb_norm_against_the_dense_restatement():
    import sgs_gnn_amd as S
    b, ei, victim = _small_graph(S)
    N, n = 70, ei.shape[1]
    w = _weights(n)
    gr = S.ops.get_graph(ei.to(DEV), N)
    for weights in (None, w):
        wd = None if weights is None else weights.to(DEV).requires_grad_()
        nm = S.ops.cheb_norm(gr, wd)
        w64 = None if weights is None else weights.double().requires_grad_()
        Lh, dis, l = R.laplacian(ei, w64, N)
        assert torch.isfinite(nm.dis).all() and float(nm.dis[victim]) == 0.0
        assert float((nm.dis.cpu().double() - dis.detach()).abs().max()) < 1e-6
        l_in = torch.empty(n, device=DEV).scatter_(0, gr.in_eid.long(), nm.what_in[:n])     # CSR entry order -> edge-id order
        l_out = torch.empty(n, device=DEV).scatter_(0, gr.out_eid.long(), nm.what_out[:n])
        assert torch.equal(l_in, l_out)
        assert float((l_in.cpu().double() - l.detach()).abs().max()) < 1e-6
        assert bool((l_in[-3:] == 0).all())                                                 # the self loops
        assert nm.what_loop is None and nm.loopw is None
        if weights is None:
            assert S.ops.cheb_norm(gr) is nm and nm.handle is None                          # cached on the graph
            continue
        g = torch.randn(n, generator=torch.Generator().manual_seed(9))
        nm.handle.backward(g.to(DEV))
        l.backward(g.double())
        _close(wd.grad, w64.grad, "dLoss/dw through the normalisation")
        assert bool((wd.grad[-3:] == 0).all())                                              # exactly 0 on the self loops
        assert torch.isfinite(wd.grad).all()


def _run_model(S, K, x, ei, w, f, h, c, p=0.0, train=False, seed=1):
    torch.manual_seed(seed)
    m = S.ChebModel(f, h, c, dropout_prob=p, edge_mlp_type="GCN", cheb_k=K).to(DEV)
    with torch.no_grad():
        m.gcn1.bias.uniform_(-0.5, 0.5)
        m.gcn2.bias.uniform_(-0.5, 0.5)
    m.train(train)
    wd = None if w is None else w.to(DEV).requires_grad_()
    bd = S.Batch(x=x.to(DEV), edge_index=ei.to(DEV))
    out = m(bd, bd.edge_index, wd)
    return m, wd, out


def _check_model(S, K, x, ei, w, f, h, c, tag):
    m, wd, out = _run_model(S, K, x, ei, w, f, h, c)
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items() if "edge_prob_mlp" not in k}
    w64 = None if w is None else w.double().requires_grad_()
    ref = R.model(P, x.double(), ei, w64, K)
    err = float((out.detach().cpu().double() - ref.detach()).abs().max())
    print(f"{tag}: logits max err {err:.3e}, max |ref| {float(ref.detach().abs().max()):.3f}")
    assert err < 1e-4, tag
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
    out.backward(g.to(DEV))
    ref.backward(g.double())
    for n_, p in m.named_parameters():
        if "edge_prob_mlp" in n_:
            assert p.grad is None
            continue
        _close(p.grad, P[n_].grad, f"{tag} {n_}")
    if w is not None:
        _close(wd.grad, w64.grad, f"{tag} edge_weight.grad")
        assert float(wd.grad.abs().max()) > 0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_model_forward_backward_small_directed_graph(K, weighted):
    import sgs_gnn_amd as S
    b, ei, _ = _small_graph(S)
    Lh, _, _ = R.laplacian(ei, None, 70)
    assert float(torch.linalg.matrix_norm(Lh, 2)) > 1.0                   # a directed L_hat: not a contraction
    _check_model(S, K, b.x, ei, _weights(ei.shape[1]) if weighted else None, 9, 12, 5, f"small K={K} weighted={weighted}")


@pytest.mark.parametrize("K", [2, 3, 5])
def test_model_forward_backward_long_rows(K):
    """N = 2 000, F = H = 64, C = 8, the row-per-workgroup kernels.  The edge list is a random 50 000-edge subset of
    synthetic_graph(2000, 60000): the generator gives a symmetric list, and a directed one is what must be right here; 25 entries per row
    on average, still on the long-row side of the kernels' switch (asserted)."""
    import sgs_gnn_amd as S
    b = S.synthetic_graph(2000, 60000, 64, 8, seed=13)
    ei = b.edge_index[:, torch.randperm(b.edge_index.shape[1], generator=torch.Generator().manual_seed(1))[:50000]].contiguous()   # directed
    assert ei.shape[1] >= 16 * 2000
    _check_model(S, K, b.x, ei, _weights(ei.shape[1]), 64, 64, 8, f"long rows K={K}")


def test_model_forward_backward_very_long_rows():
    """300 nodes x ~260 entries per row: the 16-wave row-per-workgroup variant."""
    import sgs_gnn_amd as S
    b = S.synthetic_graph(300, 80000, 16, 8, seed=14, power=0.1)
    ei = b.edge_index
    assert ei.shape[1] >= 256 * 300
    _check_model(S, 3, b.x, ei, _weights(ei.shape[1]), 16, 64, 8, "very long rows K=3")


def test_model_forward_backward_wide_rows_on_a_short_row_graph():
    """H = 300 and C = 41 (bench S3's class count) on a graph of ~5 entries per row: the row-per-lanes kernels with a row wider than one
    pass of the 64-lane group (300 > 64 * 4: the column loop runs twice) and the column-by-column form at 41 columns."""
    import sgs_gnn_amd as S
    b = S.synthetic_graph(400, 2400, 20, 41, seed=17)
    ei = b.edge_index[:, torch.randperm(b.edge_index.shape[1], generator=torch.Generator().manual_seed(2))[:2000]].contiguous()   # directed
    assert ei.shape[1] < 16 * 400
    _check_model(S, 3, b.x, ei, _weights(ei.shape[1]), 20, 300, 41, "wide rows K=3")


def test_model_forward_backward_at_the_highest_supported_order():
    """K = 8, the upper bound, on the small directed graph (||L_hat|| > 1, so the high orders grow): the same tolerances."""
    import sgs_gnn_amd as S
    b, ei, _ = _small_graph(S)
    _check_model(S, 8, b.x, ei, _weights(ei.shape[1]), 9, 12, 5, "small K=8")


def test_default_order_is_bitwise_todays_model():
    import sgs_gnn_amd as S
    b, ei, _ = _small_graph(S)
    res = []
    for kw in ({}, {"cheb_k": 1}):
        torch.manual_seed(4)
        m = S.ChebModel(9, 12, 4, dropout_prob=0.0, edge_mlp_type="GCN", **kw).to(DEV)
        bd = S.Batch(x=b.x.to(DEV), edge_index=ei.to(DEV))
        out = m(bd, bd.edge_index)
        out.backward(torch.ones_like(out))
        res.append((out.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and set(res[0][1]) == set(res[1][1]) and len(res[0][1]) == 4
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


def test_dropout_mask_is_the_exported_one_and_eval_ignores_the_clock():
    import sgs_gnn_amd as S
    from sgs_gnn_amd.model import SITE_GNN, _DropoutClock
    b, ei, _ = _small_graph(S)
    w = _weights(ei.shape[1])
    K, H, p = 3, 12, 0.3
    S.manual_seed(21)
    tick0 = _DropoutClock.tick
    m, wd, out = _run_model(S, K, b.x, ei, w, 9, H, 5, p=p, train=True)
    assert _DropoutClock.tick == tick0 + 1                                # one seed per training forward
    seed = (_DropoutClock.base * 0x9E3779B97F4A7C15 + _DropoutClock.tick * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    keep = S.ops.dropout_keep(seed, SITE_GNN, 70, H, p, torch.device(DEV)).cpu().double()
    assert 0.5 < float(keep.mean()) < 0.9
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items() if "edge_prob_mlp" not in k}
    w64 = w.double().requires_grad_()
    ref = R.model(P, b.x.double(), ei, w64, K, keep=keep, p=p)
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) < 1e-4
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
    out.backward(g.to(DEV))
    ref.backward(g.double())
    for n_, p_ in m.named_parameters():
        if "edge_prob_mlp" not in n_:
            _close(p_.grad, P[n_].grad, f"dropout {n_}")
    _close(wd.grad, w64.grad, "dropout edge_weight.grad")
    # eval mode: no seed drawn, result independent of the clock
    m.eval()
    bd = S.Batch(x=b.x.to(DEV), edge_index=ei.to(DEV))
    t = _DropoutClock.tick
    with torch.no_grad():
        o1 = m(bd, bd.edge_index, w.to(DEV))
        assert _DropoutClock.tick == t
        S.manual_seed(99)
        o2 = m(bd, bd.edge_index, w.to(DEV))
    assert torch.equal(o1, o2)


def test_two_identical_passes_are_bitwise_equal():
    import sgs_gnn_amd as S
    b = S.synthetic_graph(2000, 60000, 64, 8, seed=13)
    ei, w = b.edge_index, _weights(b.edge_index.shape[1])
    res = []
    for _ in range(2):
        m, wd, out = _run_model(S, 3, b.x, ei, w, 64, 64, 8)
        out.backward(torch.ones_like(out))
        res.append([out.detach().clone(), wd.grad.clone()] + [p.grad.clone() for n, p in m.named_parameters() if p.grad is not None])
    assert len(res[0]) == 2 + 8 and all(torch.equal(a, c) for a, c in zip(*res))


def test_the_edge_weights_reach_the_loss():
    """The point of the feature: with cheb_k = 3 the logits depend on the edge weights; with the reference's K = 1 they do not."""
    import sgs_gnn_amd as S
    b, ei, _ = _small_graph(S)
    bd = S.Batch(x=b.x.to(DEV), edge_index=ei.to(DEV))
    for K in (3, 1):
        torch.manual_seed(0)
        m = S.ChebModel(9, 12, 4, dropout_prob=0.0, edge_mlp_type="GCN", cheb_k=K).to(DEV)
        w = torch.rand(ei.shape[1], device=DEV).requires_grad_()
        m(bd, bd.edge_index, w).sum().backward()
        if K == 3:
            assert w.grad is not None and torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0
        else:
            assert w.grad is None


def _train_args(**kw):
    a = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", conditional=True, sparse_edge_mlp=True, t_init=0.7, t_min=0.5,
                           degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0, consist_reg_coef=0.5, hybrid_checkpoint=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_hybrid_training_loop_eager_and_replayed():
    import sgs_gnn_amd as S
    torch.manual_seed(0)
    S.fix_seeds(0)
    bs = [S.synthetic_graph(150, e, 9, 4, seed=20 + i, device=DEV) for i, e in enumerate([5000, 900])]
    m = S.ChebModel(9, 16, 4, dropout_prob=0.3, edge_mlp_type="GCN", cheb_k=3).to(DEV)
    og = S.FusedAdam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-2)                      # main.py:100-109 routing
    oe = S.FusedAdam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-2)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    a = _train_args()
    for hip in (False, True):
        a.sgs_hipgraph = hip
        for ep in range(3):
            loss, _, cond, tot = S.train(a, ep, 3, m, og, oe, None, torch.nn.CrossEntropyLoss(), bs, q=1000)
            assert tot == 2 and loss == loss and abs(loss) != float("inf")
    for n, p in m.named_parameters():
        assert torch.isfinite(p).all(), n
    assert all(not torch.equal(p, before[n]) for n, p in m.named_parameters() if n.startswith("gcn"))


def test_replayed_unsampled_step_equals_its_eager_recomputation():
    """Graph mode against eager, the way tests/test_gpu_stepgraph.py compares them (test_one_capture_serves_partitions_of_different_sizes:
    loss rtol 1e-5 / atol 1e-6, gradients rtol 2e-4 / atol 2e-6): ONE captured step serves partitions of different sizes, so the
    normalisation must be recomputed from the staged CSR on every replay, not remembered from the capture."""
    import sgs_gnn_amd as S
    from sgs_gnn_amd.stepgraph import StepGraphs
    from sgs_gnn_amd.training import _ce
    torch.manual_seed(3)
    S.fix_seeds(3)
    crit = torch.nn.CrossEntropyLoss()
    shapes = [(110, 900), (140, 1500), (100, 700)]
    bs = [S.synthetic_graph(n, E, 24, 5, seed=40 + i, device=DEV) for i, (n, E) in enumerate(shapes)]
    m = S.ChebModel(24, 32, 5, dropout_prob=0.0, edge_mlp_type="GCN", cheb_k=3).to(DEV)
    a = _train_args(edge_mlp_type="GCN", drop_rate=0.0, lr=1e-2)
    sg = StepGraphs.attach(m, "hybrid", a, crit, 5000, False, loader=bs)
    params = list(m.parameters())
    try:
        for rnd in range(2):
            for b in bs:
                h = sg.forward(b)
                assert not h.sampled
                loss = h.backward(None).clone()
                got = {i: g.clone() for i, g in h.c.grads.items()}
                torch.cuda.synchronize()
                for p in params:
                    p.grad = None
                ref = _ce(crit, m(b, b.edge_index), b)
                ref.backward()
                assert torch.allclose(ref.detach(), loss, rtol=1e-5, atol=1e-6)
                n_checked = 0
                for i, p in enumerate(params):
                    if p.grad is None:
                        assert i not in got
                    else:
                        assert torch.allclose(p.grad, got[i], rtol=2e-4, atol=2e-6), i
                        n_checked += 1
                assert n_checked == 8
                for p in params:
                    p.grad = None
    finally:
        sg.release()


def test_replayed_sampled_step_equals_its_eager_recomputation():
    """The step this feature exists for, under graph mode: the learned branch (cheb_norm with its autograd handle, both layers' gradients
    wrt l -- the second parked and summed on read --, the SDDMMs and sgs_cheb_norm_bwd, the task gradient reaching the scorer through the
    edge weights) and the random branch (unit normalisation of a subgraph built inside the capture).  As
    tests/test_gpu_stepgraph.py::test_one_capture_serves_partitions_of_different_sizes: every replayed step is recomputed eagerly from
    the replay's own draws (that file's _kept / _check_sampled_replay, its tolerances), over partitions of different sizes -- visited
    in an order that leaves a larger partition's leftovers in the slot -- and two rounds; unsampled partitions in between."""
    import sgs_gnn_amd as S
    import test_gpu_stepgraph as TS
    from sgs_gnn_amd.stepgraph import StepGraphs
    from sgs_gnn_amd.training import _ce
    torch.manual_seed(3)
    S.fix_seeds(3)
    crit = torch.nn.CrossEntropyLoss()
    shapes, q = [(150, 6100), (90, 2600), (120, 4000), (110, 900), (140, 1500), (100, 700)], 1000
    bs = [S.synthetic_graph(n, E, 24, 5, seed=40 + i, device=DEV) for i, (n, E) in enumerate(shapes)]
    m = S.ChebModel(24, 32, 5, dropout_prob=0.0, edge_mlp_type="GCN", cheb_k=3).to(DEV)
    a = TS._args(pipeline="hybrid")
    sg = StepGraphs.attach(m, "hybrid", a, crit, q, False, loader=bs)
    sg.debug_keep = True
    params = list(m.parameters())
    names = [n for n, _ in m.named_parameters()]
    n_sampled = 0
    try:
        for rnd in range(2):
            for b in bs:
                E = b.edge_index.shape[1]
                h = sg.forward(b)
                c = h.c
                assert c.live is b and int(c.dims[0]) == E and h.sampled == (E > q)
                if h.sampled:
                    cnt = h.gate_counts()
                    k = TS._kept(c, b)
                    c.g2l.replay()
                    gl = {i: g.clone() for i, g in c.grads_l.items()}
                    ll = c.loss_l.clone()
                    c.g2r.replay()
                    gr = {i: g.clone() for i, g in c.grads_r.items()}
                    lr_ = c.loss_r.clone()
                    sg.host_epoch += 2
                    torch.cuda.synchronize()
                    # the learned branch's gradients include the scorer's (the edge weights carry the task gradient) and all 8 of the head's
                    assert sum(1 for i in gl if names[i].startswith("gcn")) == 8
                    assert any(names[i].startswith("edge_prob_mlp") and float(gl[i].abs().max()) > 0 for i in gl)
                    TS._check_sampled_replay(S, m, a, crit, b, q, "hybrid", k, cnt, gl, ll, gr, lr_)
                    n_sampled += 1
                else:
                    loss = h.backward(None).clone()
                    got = {i: g.clone() for i, g in c.grads.items()}
                    torch.cuda.synchronize()
                    for p in params:
                        p.grad = None
                    ref = _ce(crit, m(b, b.edge_index), b)
                    ref.backward()
                    assert torch.allclose(ref.detach(), loss, rtol=1e-5, atol=1e-6)
                    for i, p in enumerate(params):
                        if p.grad is None:
                            assert i not in got
                        else:
                            assert torch.allclose(p.grad, got[i], rtol=2e-4, atol=2e-6), i
                for p in params:
                    p.grad = None
        assert n_sampled == 8 and sg.captures == 4
    finally:
        sg.release()


def test_ensemble_evaluation_takes_the_serial_loop_and_agrees_with_itself():
    import sgs_gnn_amd as S
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    torch.manual_seed(4)
    m = S.ChebModel(12, 16, 5, dropout_prob=0.3, edge_mlp_type="GCN", cheb_k=3).to(DEV)
    bs = [S.synthetic_graph(200, E, 12, 5, seed=21 + i, train_frac=0.4) for i, E in enumerate([4000, 1500])]
    got, edges, logits = {}, {}, {}
    for engine in (False, True):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=5, _sgs_trace_eval={})
        if engine:
            args.sgs_eval_batch, args.sgs_eval_batch_heads = True, "all"
        S.manual_seed(7)
        before = dict(ev.PATH_COUNTS)
        got[engine] = S.ensemble_evaluate(args, m, bs, DEV, q=2000, mode="learned")
        assert ev.PATH_COUNTS["serial"] == before["serial"] + 1 and ev.PATH_COUNTS["batched"] == before["batched"]
        edges[engine], logits[engine] = args._sgs_trace_eval["edges"].clone(), args._sgs_trace_eval["logits"].clone()
    assert len(got[True]) == 3 and got[True] == got[False]
    assert torch.equal(edges[True], edges[False]) and torch.equal(logits[True], logits[False])
    # and the draws matter: two draws of one partition give different logits (at K = 1 they would be identical)
    S.manual_seed(7)
    args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=2, _sgs_trace_eval={})
    S.ensemble_evaluate(args, m, bs[:1], DEV, q=2000, mode="learned")
    lg = args._sgs_trace_eval["logits"]
    assert not torch.equal(lg[0], lg[1])
    f1 = S.evaluate(argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=1), m, bs, DEV, q=2000, mode="learned")
    assert all(0.0 <= v <= 1.0 for v in f1)
