"""GPU: the GATv2 head (GATModel(gat_v2=True): PyG 2.3.1 GAT(..., v2=True), optionally with edge_dim=1 and the sampled edge weight as the
attribute) on the gathering per-head kernels of csrc/gatv2.hip, against tests/gatv2_ref.py (fp64, edge-list form, torch autograd).
Tolerances are tests/test_gpu_gat_heads.py's (forward < 1e-5, gradients < 1e-4, max-abs error over max-abs reference): per entry the
arithmetic is a C-term fp32 dot product in place of GATConv's three-term sum, then the same softmax and aggregation.  Third-party layer
restated from its published algorithm: parity with PyG itself unpinned."""
import argparse
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gatv2_ref as R  # noqa: E402
from test_gpu_gat_edge import _weights  # noqa: E402
from test_gpu_gat_heads import CASES, _graph, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# test_gpu_gat_heads.py's shapes (duplicate edge, removed self loops, E = 0, K = 3, in-degree >> 64) plus one head, C % 4 != 0 and a
# head wider than its lanes' stride (gatv2_ref.EXTRA_CASES)
V2_CASES = CASES + R.EXTRA_CASES
V2_KEYS = ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")


class _Data:
    pass


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("N,E,Fin,K,C,concat", V2_CASES)
def test_gatv2conv_forward_backward(N, E, Fin, K, C, concat, edge):
    from sgs_gnn_amd.model import GATv2Conv
    ei, g = _graph(N, E, N + K * C)
    x = torch.randn(N, Fin, generator=g)
    w = _weights(E, g) if edge else None
    # the parameters are seeded: a pre-activation x_l[j] + x_r[i] (+ w le) within fp32 rounding of 0 may take the other slope of the
    # leaky_relu on the GPU, which moves that (entry, channel)'s gradient term by 0.8 g att -- with E K C pre-activations per layer (GATConv
    # has E K) an unseeded draw meets such a point every few runs, and the comparison has to be reproducible
    torch.manual_seed(N + K * C)
    conv = GATv2Conv(Fin, C, heads=K, concat=concat, edge_dim=1)
    with torch.no_grad():
        conv.bias.uniform_(-0.3, 0.3)
        conv.lin_l.bias.uniform_(-0.3, 0.3)
        conv.lin_r.bias.uniform_(-0.3, 0.3)
    P = [t.detach().clone().double() for t in (conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, conv.lin_r.bias, conv.att.reshape(K, C),
                                               conv.bias, conv.lin_edge.weight)]
    width = K * C if concat else C
    gy = torch.randn(N, width, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in [x.double()] + P]
    wr = w.double().requires_grad_(True) if edge else None
    yo = R.gatv2_layer(leaves[0], ei, wr, *leaves[1:], K, C, concat)
    yo.backward(gy.double())

    conv = conv.to(DEV)
    xd = x.clone().to(DEV).requires_grad_(True)
    wd = w.clone().to(DEV).requires_grad_(True) if edge else None
    yd = conv(xd, ei.to(DEV), wd)
    assert tuple(yd.shape) == (N, width)
    yd.backward(gy.to(DEV))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    errs = {"out": rel(yd.detach(), yo.detach()), "x": rel(xd.grad, leaves[0].grad), "lin_l.weight": rel(conv.lin_l.weight.grad, leaves[1].grad),
            "lin_l.bias": rel(conv.lin_l.bias.grad, leaves[2].grad), "lin_r.weight": rel(conv.lin_r.weight.grad, leaves[3].grad),
            "lin_r.bias": rel(conv.lin_r.bias.grad, leaves[4].grad), "att": rel(conv.att.grad.reshape(K, C), leaves[5].grad),
            "bias": rel(conv.bias.grad, leaves[6].grad)}
    if edge:
        errs["lin_edge.weight"] = rel(conv.lin_edge.weight.grad, zero(leaves[7]))
        if E > 0:
            errs["edge_weight"] = rel(wd.grad, wr.grad)
    print("gatv2_parity", (N, E, Fin, K, C, concat, edge), errs)
    if edge:
        assert wd.grad is None or wd.grad.shape == (E,)
        if E > 8:
            assert float(wd.grad.abs().max()) > 0
            loops = ei[0] == ei[1]
            assert bool(loops.any()) and float(wd.grad.cpu()[loops].abs().max()) == 0.0      # removed (i, i) entries: gradient exactly 0
    else:
        le = conv.lin_edge.weight.grad
        assert le is None or float(le.abs().max()) == 0.0
    assert errs.pop("out") < 1e-5
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


def _model_and_batch(S, K, flag, p=0.0, seed=0, N=120, E=2500, hid=32, v2=True):
    torch.manual_seed(seed)
    m = S.GATModel(12, hid, 5, dropout_prob=p, edge_mlp_type="GCN", gat_heads=K, gat_edge_weight=flag, gat_v2=v2)
    with torch.no_grad():
        for c in m.GAT.convs:
            c.bias.uniform_(-0.3, 0.3)
            if v2:
                c.lin_l.bias.uniform_(-0.3, 0.3)
                c.lin_r.bias.uniform_(-0.3, 0.3)
    ei, g = _graph(N, E, 9)
    x = torch.randn(N, 12, generator=g)
    w = _weights(E, g)
    data = _Data()
    data.x = x.to(DEV)
    return m.to(DEV), data, x, ei, w


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("K", [1, 8])
def test_two_layer_head_logits_and_gradients(K, flag):
    """Both layers consume the same edge weights: their d w are summed (the second layer to finish adds the first one's on its way out)."""
    import sgs_gnn_amd as S
    m, data, x, ei, w = _model_and_batch(S, K, flag, hid=64)
    names = [n for n, _ in m.named_parameters() if n.startswith("GAT.")]
    assert len(names) == (14 if flag else 12)
    P = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    for n in names:
        P[n].requires_grad_(True)
    wr = w.double().requires_grad_(True) if flag else None
    ref = R.gatv2_model(P, x.double(), ei, wr, K, 64, 5)
    ref.square().sum().backward()
    m.eval()
    wd = w.to(DEV).requires_grad_(True)
    logits = m(data, ei.to(DEV), wd)
    logits.square().sum().backward()
    params = dict(m.named_parameters())
    errs = {"logits": rel(logits.detach(), ref.detach())}
    if flag:
        errs["edge_weight"] = rel(wd.grad, wr.grad)
    else:
        assert wd.grad is None
    for n in names:
        errs[n] = rel(params[n].grad, P[n].grad)
    print("gatv2_two_layer", K, flag, errs)
    assert errs.pop("logits") < 1e-5
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


def test_the_edge_weights_reach_the_logits():
    import sgs_gnn_amd as S
    for flag in (True, False):
        m, data, x, ei, w = _model_and_batch(S, 4, flag)
        m.eval()
        eid = ei.to(DEV)
        w1 = w.to(DEV).requires_grad_(True)
        w2 = (1.0 - w).to(DEV)
        o1, o2 = m(data, eid, w1), m(data, eid, w2)
        o1.square().sum().backward()
        if flag:
            assert not torch.equal(o1, o2) and float((o1 - o2).abs().max()) > 1e-4
            assert w1.grad is not None and bool(torch.isfinite(w1.grad).all()) and float(w1.grad.abs().max()) > 0
        else:
            assert torch.equal(o1, o2) and torch.equal(o1, m(data, eid))
            assert w1.grad is None


def test_dropout_replay_with_exported_masks():
    import sgs_gnn_amd as S
    from sgs_gnn_amd import model as M
    K, hid, p = 4, 16, 0.3
    N, E = 80, 1200
    torch.manual_seed(1)
    m = S.GATModel(12, hid, 5, dropout_prob=p, edge_mlp_type="GCN", gat_heads=K, gat_edge_weight=True, gat_v2=True).to(DEV).train()
    ei, g = _graph(N, E, 3)
    x = torch.randn(N, 12, generator=g)
    w = _weights(E, g)
    data = _Data()
    data.x = x.to(DEV)
    M.set_dropout_seed(5)
    seed = (M._DropoutClock.base * 0x9E3779B97F4A7C15 + 1 * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    wd = w.to(DEV).requires_grad_(True)
    out = m(data, ei.to(DEV), wd)
    keep = lambda site, rows, cols: S.ops.dropout_keep(seed, site, rows, cols, p, DEV).cpu().reshape(rows, cols)
    masks = {"e0": keep(M.SITE_GAT_ATT, E, K), "l0": keep(M.SITE_GAT_ATT + 1, N, K), "e1": keep(M.SITE_GAT_ATT + 2, E, K),
             "l1": keep(M.SITE_GAT_ATT + 3, N, K), "h": keep(M.SITE_GAT_ACT, N, hid)}
    for v in masks.values():
        assert 0.5 < float(v.double().mean()) < 0.9                     # masks are live, not all-ones
    names = [n for n, _ in m.named_parameters() if n.startswith("GAT.")]
    P = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    for n in names:
        P[n].requires_grad_(True)
    wr = w.double().requires_grad_(True)
    ref = R.gatv2_model(P, x.double(), ei, wr, K, hid, 5, masks, p)
    ref.square().sum().backward()
    out.square().sum().backward()
    params = dict(m.named_parameters())
    errs = {"logits": rel(out.detach(), ref.detach()), "edge_weight": rel(wd.grad, wr.grad)}
    for n in names:
        errs[n] = rel(params[n].grad, P[n].grad)
    print("gatv2_dropout_replay", errs)
    assert errs.pop("logits") < 1e-5
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


@pytest.mark.parametrize("K", [1, 8])
def test_two_identical_passes_are_bitwise_equal(K):
    import sgs_gnn_amd as S
    b = S.synthetic_graph(2000, 60000, 12, 5, seed=13)
    res = []
    for _ in range(2):
        torch.manual_seed(3)
        m = S.GATModel(12, 64, 5, dropout_prob=0.3, edge_mlp_type="GCN", gat_heads=K, gat_edge_weight=True, gat_v2=True).to(DEV).train()
        S.set_dropout_seed(9)
        g = torch.Generator().manual_seed(1)
        wd = torch.rand(b.edge_index.shape[1], generator=g).to(DEV).requires_grad_(True)
        data = _Data()
        data.x = b.x.to(DEV)
        out = m(data, b.edge_index.to(DEV), wd)
        out.backward(torch.ones_like(out))
        res.append([out.detach().clone(), wd.grad.clone()] + [p.grad.clone() for n, p in m.named_parameters() if p.grad is not None])
    assert len(res[0]) == 2 + 14 and all(torch.equal(a, c) for a, c in zip(*res))


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("K", [1, 8])
def test_default_is_the_model_without_the_keyword_bitwise(K, flag):
    import sgs_gnn_amd as S
    b = S.synthetic_graph(300, 6000, 12, 5, seed=2)
    data = _Data()
    data.x = b.x.to(DEV)
    eid = b.edge_index.to(DEV)
    res = []
    for kw in ({}, {"gat_v2": False}):
        torch.manual_seed(6)
        m = S.GATModel(12, 64, 5, dropout_prob=0.3, edge_mlp_type="GCN", gat_heads=K, gat_edge_weight=flag, **kw).to(DEV).train()
        S.set_dropout_seed(4)
        w = torch.rand(eid.shape[1], generator=torch.Generator().manual_seed(8)).to(DEV).requires_grad_(True)
        out = m(data, eid, w)
        out.square().sum().backward()
        res.append([out.detach()] + [p.grad for n, p in m.named_parameters() if n.startswith("GAT.")] + ([w.grad] if flag else []))
    assert len(res[0]) == (1 + 12 + 1 if flag else 1 + 8) and all(a is not None and torch.equal(a, c) for a, c in zip(*res))
    from sgs_gnn_amd import model as M
    assert M._DropoutClock.tick == 1                      # one seed per forward, as before the keyword


def _st_args(**kw):
    a = argparse.Namespace(device=DEV, mode="learned", pipeline="straight_through", conditional=True, sparse_edge_mlp=False, t_init=0.7,
                           t_min=0.5, degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0, consist_reg_coef=0.5)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("pipeline", ["straight_through", "hybrid"])
def test_training_loop_eager_and_replayed(pipeline):
    import sgs_gnn_amd as S
    torch.manual_seed(5)
    S.fix_seeds(5)
    crit = torch.nn.CrossEntropyLoss()
    bs = [S.synthetic_graph(150, E, 24, 5, seed=11 + i, device=DEV) for i, E in enumerate([5000, 900, 4000])]
    m = S.GATModel(24, 32, 5, dropout_prob=0.3, edge_mlp_type="GCN", gat_heads=4, gat_edge_weight=True, gat_v2=True).to(DEV)
    og = S.FusedAdam([p for n, p in m.named_parameters() if "GAT" in n or "gcn" in n], lr=1e-2)
    oe = S.FusedAdam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-2)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    for hip in (False, True):
        a = _st_args(pipeline=pipeline, edge_mlp_type="GCN", sparse_edge_mlp=True, hybrid_checkpoint=False, drop_rate=0.0, lr=1e-2,
                     sgs_hipgraph=hip)
        for ep in range(3):
            loss, _, cond, tot = S.train(a, ep, 3, m, og, oe, None, crit, bs, q=1000)
            assert tot == 3 and loss == loss and abs(loss) != float("inf")
    for n, p in m.named_parameters():
        assert torch.isfinite(p).all(), n
    assert all(not torch.equal(p, before[n]) for n, p in m.named_parameters() if n.startswith("GAT."))
    assert m._sgs_stepgraphs.captures <= 4


@pytest.mark.parametrize("pipeline", ["straight_through", "hybrid"])
@pytest.mark.parametrize("flag", [True, False])
def test_the_cross_entropy_reaches_the_scorer_only_with_the_flag(pipeline, flag):
    """One learned step with both regularisers off: the loss is the cross entropy alone, and the scorer's fc1.weight gets a gradient only
    through the edge weights inside the v2 logits."""
    import sgs_gnn_amd as S
    from sgs_gnn_amd.training import learned_loss, sampled_forward
    b = S.synthetic_graph(300, 6000, 12, 5, seed=1, train_frac=0.5).to(DEV)
    q = int(b.edge_index.shape[1] * 0.2)
    torch.manual_seed(11)
    S.fix_seeds(0)
    m = S.GATModel(12, 64, 5, 0.3, edge_mlp_type="GCN", gat_heads=8, gat_edge_weight=flag, gat_v2=True).to(DEV).train()
    args = _st_args(pipeline=pipeline, reg1=False, reg2=False)
    S.ops.new_memo_scope()
    S.ops.get_pairs(b.edge_index, b.x.shape[0], build=True)
    st = sampled_forward(pipeline, args, m, b, q)
    loss = learned_loss(args, torch.nn.CrossEntropyLoss(), st, b)
    loss.backward()
    g = m.edge_prob_mlp.fc1.weight.grad
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in m.named_parameters() if n.startswith("GAT."))
    if flag:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        for n, p in m.named_parameters():
            if "lin_edge" in n:
                assert float(p.grad.abs().max()) > 0, n
    else:
        assert g is None or float(g.abs().max()) == 0.0


def test_replayed_steps_equal_their_eager_recomputation():
    """tests/test_gpu_gat_edge.py::test_replayed_steps_equal_their_eager_recomputation with the v2 edge-weighted head: every replayed
    sampled hybrid step is recomputed eagerly from the replay's own draws, unsampled partitions (edge_weight=None) in between; that
    file's tolerances (rtol 1e-5 / atol 1e-6 on the loss, rtol 2e-4 / atol 2e-6 on gradients)."""
    import sgs_gnn_amd as S
    import test_gpu_stepgraph as TS
    from sgs_gnn_amd.stepgraph import StepGraphs
    from sgs_gnn_amd.training import _ce
    torch.manual_seed(3)
    S.fix_seeds(3)
    crit = torch.nn.CrossEntropyLoss()
    shapes, q = [(150, 6100), (90, 2600), (110, 900), (100, 700)], 1000
    bs = [S.synthetic_graph(n, E, 24, 5, seed=40 + i, device=DEV) for i, (n, E) in enumerate(shapes)]
    m = S.GATModel(24, 32, 5, dropout_prob=0.0, edge_mlp_type="GCN", gat_heads=4, gat_edge_weight=True, gat_v2=True).to(DEV)
    a = TS._args(pipeline="hybrid")
    sg = StepGraphs.attach(m, "hybrid", a, crit, q, False, loader=bs)
    sg.debug_keep = True
    params = list(m.parameters())
    names = [n for n, _ in m.named_parameters()]
    n_sampled = n_unsampled = 0
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
                    assert sum(1 for i in gl if names[i].startswith("GAT.")) == 14
                    assert all(float(gl[i].abs().max()) > 0 for i in gl if "lin_edge" in names[i])
                    assert any(names[i].startswith("edge_prob_mlp") and float(gl[i].abs().max()) > 0 for i in gl)
                    assert not any("lin_edge" in names[i] for i in gr)
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
                    n_unsampled += 1
                for p in params:
                    p.grad = None
        assert n_sampled == 4 and n_unsampled == 4
    finally:
        sg.release()


def test_ensemble_evaluation_takes_the_serial_loop():
    import sgs_gnn_amd as S
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    torch.manual_seed(4)
    m = S.GATModel(12, 16, 5, dropout_prob=0.3, edge_mlp_type="GCN", gat_heads=4, gat_edge_weight=True, gat_v2=True).to(DEV)
    bs = [S.synthetic_graph(200, E, 12, 5, seed=21 + i, train_frac=0.4) for i, E in enumerate([4000, 1500])]
    got = {}
    for engine in (False, True):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=5)
        if engine:
            args.sgs_eval_batch, args.sgs_eval_batch_heads, args.sgs_eval_batch_variants = True, "all", True
        S.manual_seed(7)
        before = dict(ev.PATH_COUNTS)
        got[engine] = S.ensemble_evaluate(args, m, bs, DEV, q=2000, mode="learned")
        assert ev.PATH_COUNTS["serial"] == before["serial"] + 1 and ev.PATH_COUNTS["batched"] == before["batched"]
    assert len(got[True]) == 3 and got[True] == got[False]
    assert all(0.0 <= v <= 1.0 for v in got[True])
