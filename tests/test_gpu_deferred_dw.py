"""GPU: the leaf weight gradients of a backward pass deferred to ONE grouped launch (ops.deferred_weight_grads) against the same step
with every product launched where it is formed.  Same seeds, so the draws and dropout masks agree; the grouped kernel runs the single
kernel's arithmetic, so every parameter gradient and every parameter after the Adam step must be EQUAL (torch.equal).  The library
calls made for these products are counted (ops.GEMM_TN_LAUNCHES): deferred, a backward makes one."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_NODES, NFEAT, HID, NCLS = 600, 24, 128, 5          # K = 600 rows >= 512: every product takes the 16-wave kernel


def _args():
    return argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", edge_mlp_type="GCN", conditional=True, sparse_edge_mlp=True,
                              t_init=0.7, t_min=0.5, degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0,
                              consist_reg_coef=0.5, hybrid_checkpoint=False, drop_rate=0.0, lr=1e-2)


@pytest.fixture(scope="module")
def S():
    import sgs_gnn_amd
    return sgs_gnn_amd


@pytest.fixture(scope="module")
def batches(S):
    """(a partition above q = 4 000 edges, one below it, one whose draw of q = 70 000 puts the scorer backward on its mask-form kernels)"""
    return {"sampled": (S.synthetic_graph(N_NODES, 20_000, NFEAT, NCLS, seed=31, device=DEV), 4_000),
            "unsampled": (S.synthetic_graph(N_NODES, 3_000, NFEAT, NCLS, seed=32, device=DEV), 4_000),
            "sampled_large": (S.synthetic_graph(N_NODES, 150_000, NFEAT, NCLS, seed=33, device=DEV), 70_000)}


def _setup(S, p_drop=0.3):
    torch.manual_seed(5)
    S.fix_seeds(5)
    m = S.GNNModel(NFEAT, HID, NCLS, dropout_prob=p_drop, edge_mlp_type="GCN").to(DEV)
    og = S.FusedAdam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-2)
    oe = S.FusedAdam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-2)
    return m, og, oe


def _eager_step(S, batches, kind, defer, preset=None):
    """One eager step of `kind` (learned | learned_large | random | unsampled) -> (library calls of the backward, gradients, parameters
    after the optimiser step).  `preset`: name of a parameter that already holds a .grad when the backward starts."""
    from sgs_gnn_amd.training import _ce, learned_loss, sampled_forward
    ops = S.ops
    crit, a = torch.nn.CrossEntropyLoss(), _args()
    m, og, oe = _setup(S)
    b, q = batches["unsampled" if kind == "unsampled" else "sampled_large" if kind == "learned_large" else "sampled"]
    ops.new_memo_scope()
    if kind == "unsampled":
        loss = _ce(crit, m(b, b.edge_index), b)
    else:
        ops.get_pairs(b.edge_index, b.x.shape[0], build=True)
        st = sampled_forward("hybrid", a, m, b, q)
        loss = _ce(crit, st.random_out, b) if kind == "random" else learned_loss(a, crit, st, b)
    if preset is not None:
        p = dict(m.named_parameters())[preset]
        p.grad = torch.full_like(p, 0.25)
    ops.GEMM_TN_LAUNCHES.update(single=0, group=0)
    if defer:
        with ops.deferred_weight_grads(loss):
            loss.backward()
    else:
        loss.backward()
    calls = dict(ops.GEMM_TN_LAUNCHES)
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    if kind.startswith("learned"):
        oe.step()
    og.step()
    torch.cuda.synchronize()
    return calls, grads, {n: p.detach().clone() for n, p in m.named_parameters()}


def _same(x, y):
    assert x.keys() == y.keys()
    for n in x:
        assert torch.equal(x[n], y[n]), n


# (kind, weight gradients of its backward: GNN dW2 + dW1 [+ scorer dW1b + its encoder's two layers])
@pytest.mark.parametrize("kind,products", [("learned", 5), ("learned_large", 5), ("random", 2), ("unsampled", 2)])
def test_eager_step_deferred_equals_immediate(S, batches, kind, products):
    c0, g0, p0 = _eager_step(S, batches, kind, defer=False)
    c1, g1, p1 = _eager_step(S, batches, kind, defer=True)
    assert c0 == {"single": products, "group": 0}
    assert c1 == {"single": 0, "group": 1}
    assert len(g0) == (12 if kind.startswith("learned") else 4)
    _same(g0, g1)
    _same(p0, p1)


def test_parameter_with_a_gradient_already_is_not_deferred(S, batches):
    """AccumulateGrad ADDS to an existing .grad, i.e. reads dW on the spot: that product must be launched where it is formed."""
    c0, g0, p0 = _eager_step(S, batches, "learned", defer=False, preset="gcn2.lin.weight")
    c1, g1, p1 = _eager_step(S, batches, "learned", defer=True, preset="gcn2.lin.weight")
    assert c0 == {"single": 5, "group": 0}
    assert c1 == {"single": 1, "group": 1}
    _same(g0, g1)
    _same(p0, p1)
    _, g_plain, _ = _eager_step(S, batches, "learned", defer=True)
    assert torch.equal(g1["gcn2.lin.weight"], g_plain["gcn2.lin.weight"] + 0.25)


def test_second_producer_of_a_weight_is_not_deferred(S, batches):
    """Two nodes of one backward give a gradient to the same weight (autograd sums them before AccumulateGrad: a read): both immediate."""
    ops = S.ops
    b, _ = batches["unsampled"]

    def run(defer):
        m, _, _ = _setup(S, p_drop=0.0)
        W = m.gcn1.lin.weight
        loss = (ops.linear_nobias(b.x, W) * 0.5).sum() + ops.linear_nobias(b.x * 2.0, W).sum() + ops.linear_nobias(b.x, m.edge_prob_mlp.gcn1.lin.weight).sum()
        ops.GEMM_TN_LAUNCHES.update(single=0, group=0)
        if defer:
            with ops.deferred_weight_grads(loss):
                loss.backward()
        else:
            loss.backward()
        torch.cuda.synchronize()
        return dict(ops.GEMM_TN_LAUNCHES), W.grad.clone(), m.edge_prob_mlp.gcn1.lin.weight.grad.clone()

    c0, a0, e0 = run(False)
    c1, a1, e1 = run(True)
    assert c0 == {"single": 3, "group": 0} and c1 == {"single": 2, "group": 1}
    assert torch.equal(a0, a1) and torch.equal(e0, e1)


def test_backward_that_raises_leaves_no_queue_behind(S, batches):
    ops = S.ops
    b, _ = batches["unsampled"]
    m, _, _ = _setup(S, p_drop=0.0)

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            raise ValueError("boom")

    y = ops.linear_nobias(b.x, m.gcn1.lin.weight)
    loss = y.sum() + Boom.apply(ops.linear_nobias(b.x, m.edge_prob_mlp.gcn1.lin.weight)).sum()
    scope = ops.deferred_weight_grads(loss)
    with pytest.raises((ValueError, RuntimeError), match="boom"):
        with scope:
            loss.backward()
    torch.cuda.synchronize()
    assert ops._defer is None and scope.queue == [] and not scope.armed
    # the next backward is a clean one
    for p in m.parameters():
        p.grad = None
    loss = ops.linear_nobias(b.x, m.gcn1.lin.weight).sum()
    ops.GEMM_TN_LAUNCHES.update(single=0, group=0)
    with ops.deferred_weight_grads(loss):
        loss.backward()
    assert ops.GEMM_TN_LAUNCHES == {"single": 0, "group": 1}
    ref = b.x.sum(0).expand(HID, NFEAT)
    assert torch.allclose(m.gcn1.lin.weight.grad, ref, rtol=1e-4, atol=1e-3)


def _replayed_steps(S, batches, defer):
    """Two learned steps through StepGraphs (capture, then replays), optimiser steps inside the graphs."""
    from sgs_gnn_amd.stepgraph import StepGraphs
    ops = S.ops
    crit, a = torch.nn.CrossEntropyLoss(), _args()
    b, q = batches["sampled"]
    ops.set_deferred_weight_grads(defer)
    try:
        m, og, oe = _setup(S)
        ops.GEMM_TN_LAUNCHES.update(single=0, group=0)
        sg = StepGraphs.attach(m, "hybrid", a, crit, q, False, optimizers=(oe, og), loader=[b])
        try:
            assert sg.optimizers is not None
            for _ in range(2):
                h = sg.forward(b)
                h.gate_counts()
                h.backward(True)
            torch.cuda.synchronize()
            calls = dict(ops.GEMM_TN_LAUNCHES)
            grads = {i: g.clone() for i, g in h.c.grads_l.items()}
            return calls, grads, {n: p.detach().clone() for n, p in m.named_parameters()}
        finally:
            sg.release()
    finally:
        ops.set_deferred_weight_grads(True)


def test_replayed_learned_step_deferred_equals_immediate(S, batches):
    c0, g0, p0 = _replayed_steps(S, batches, defer=False)
    c1, g1, p1 = _replayed_steps(S, batches, defer=True)
    # one slot is warmed up (random + learned backward) and captured (G2L + G2R): four backward passes in all, none at replay
    assert c0 == {"single": 2 * (5 + 2), "group": 0}
    assert c1 == {"single": 0, "group": 4}
    assert len(g0) == 12
    _same(g0, g1)
    _same(p0, p1)
