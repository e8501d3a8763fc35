"""GPU, end to end: models with a hidden width above 256 (--nhid 384 / 512), whose edge scorer runs the wide-H kernels, through eager
train(), HIP-graph train() and both ensemble-evaluation engines."""
import argparse
import copy

import pytest
import torch
import torch.nn as nn

from oracle import sgs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _args(**kw):
    a = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", edge_mlp_type="GCN", conditional=True, sparse_edge_mlp=True,
                           t_init=0.7, t_min=0.5, degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0, consist_reg_coef=0.5,
                           hybrid_checkpoint=False, drop_rate=0.0, lr=1e-3)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _opts(m, lr=1e-3, cls=torch.optim.Adam):
    og = cls([p for n, p in m.named_parameters() if "gcn" in n or "GAT" in n], lr=lr)
    oe = cls([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=lr)
    return og, oe


def test_hybrid_step_at_nhid_512_matches_oracle():
    """One eager hybrid learned step, GNNModel(F, 512, C) with the GCN scorer, against the oracle's step with both draws and the gate
    forced to the product's outcomes (the draws themselves are checked as in test_gpu_configs_at_size.py).  Unconditional (the learned
    branch's loss, --sparse_edge_mlp keeps the prior draw), so the scorer's gradients exist and all 12 are compared."""
    import sgs_gnn_amd as S
    ops = S.ops
    N, Eb, Fin, C, H = 1_000, 70_000, 64, 5, 512
    b = S.synthetic_graph(N, Eb, Fin, C, seed=51, train_frac=0.3, power=0.5, device=DEV)
    E = b.edge_index.shape[1]
    q = int(0.2 * E)
    torch.manual_seed(5)
    m = S.GNNModel(Fin, H, C, dropout_prob=0.0, edge_mlp_type="GCN").to(DEV)
    og, oe = _opts(m)
    oa = torch.optim.Adam(m.parameters(), lr=1e-3)
    P0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    n1, n2 = ops.exp_noise(11, 1, E, DEV), ops.exp_noise(11, 2, E, DEV)
    args = _args(conditional=False)
    args._sgs_noise = {"prior": n1, "sample": n2}
    args._sgs_trace = tr = {}
    ret = S.train(args, 0, 10, m, og, oe, oa, nn.CrossEntropyLoss(), [b], q=q, alternate_frequency=0)
    bc = b.to("cpu")
    batch = dict(x=bc.x, edge_index=bc.edge_index, y=bc.y, train_mask=bc.train_mask, prob=bc.prob)
    rs_cols = tr["rsei"].cpu()
    key = bc.edge_index[0] * N + bc.edge_index[1]
    rid = torch.searchsorted(key, rs_cols[0] * N + rs_cols[1])
    assert torch.equal(bc.edge_index[:, rid], rs_cols) and rid.numel() == q
    md = torch.zeros(E, dtype=torch.bool)
    md[rid] = True
    mo = torch.zeros(E, dtype=torch.bool)
    mo[O.prior_draw(bc.prob, n1.cpu(), q)] = True
    assert int((md ^ mo).sum()) <= 8
    p_dev = tr["edge_probs_full"].cpu()
    mask_o, _ = O.gumbel_softmax_sampling(bc.prob, p_dev, q, 0.3, False, n2.cpu(), Z=tr["sample"].stats[0].cpu())
    assert torch.equal(mask_o, tr["sample"].mask.cpu())
    P = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    cfg = O.StepConfig(pipeline="hybrid", scorer="GCN", q=q, conditional=False, sparse_edge_mlp=True, drop_rate=0.0)
    R = O.learned_step_forward(P, batch, cfg, O.StepNoise(prior_noise=n1.cpu(), sample_noise=n2.cpu()), force_gate=bool(tr["update_edge_mlp"]),
                               force_random_idx=rid, force_mask=mask_o)
    R["loss"].backward()
    torch.testing.assert_close(p_dev, R["edge_probs_full"].detach(), rtol=0, atol=2e-6)
    torch.testing.assert_close(tr["learned_out"].cpu(), R["learned_out"].detach(), rtol=1e-4, atol=1e-4)
    assert bool(tr["update_edge_mlp"]) and bool(R["update_edge_mlp"])
    assert abs(float(ret[0]) - float(R["loss"])) < 2e-4
    n_cmp = 0
    for k, v in m.named_parameters():
        g = P[k].grad
        if g is None:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
            continue
        tol = 2e-3 * float(g.abs().max())
        torch.testing.assert_close(v.grad.cpu(), g, rtol=2e-3, atol=tol, msg=lambda s_: f"grad {k}: {s_}")
        n_cmp += 1
    assert n_cmp == len(list(m.parameters())) == 12


@pytest.mark.parametrize("scorer,head", [("GSAGE", "GCN"), ("MLP", "GCN"), ("GCN", "GAT")])
def test_one_step_at_nhid_384(scorer, head):
    """One eager hybrid step with dropout on: the GSAGE scorer, the MLP scorer (its endpoint-dropout kernels) and the GAT head, at
    H = 384.  The step runs, the scorer's forward ran in fp32, and every gradient is finite with the scorer's non-zero."""
    import sgs_gnn_amd as S
    N, Eb, Fin, C, H = 800, 40_000, 48, 4, 384
    b = S.synthetic_graph(N, Eb, Fin, C, seed=61, train_frac=0.3, power=0.5, device=DEV)
    torch.manual_seed(6)
    cls = S.GATModel if head == "GAT" else S.GNNModel
    m = cls(Fin, H, C, dropout_prob=0.3, edge_mlp_type=scorer).to(DEV)
    og, oe = _opts(m)
    # EdgeProbMLP scores only the prior draw's edges under --conditional / --sparse_edge_mlp (the reference fails the same way):
    # it trains unconditionally over every edge
    args = _args(edge_mlp_type=scorer, drop_rate=0.3, **(dict(conditional=False, sparse_edge_mlp=False) if scorer == "MLP" else {}))
    args._sgs_trace = tr = {}
    n0 = S.ops.PRECISION_COUNTS["fwd_fp32"]
    m.train()
    ret = S.train(args, 0, 10, m, og, oe, None, nn.CrossEntropyLoss(), [b], q=int(0.2 * b.edge_index.shape[1]), alternate_frequency=0)
    assert torch.isfinite(torch.tensor(float(ret[0])))
    if scorer != "MLP":
        assert S.ops.PRECISION_COUNTS["fwd_fp32"] > n0
    p = tr["edge_probs_full"]
    assert p.shape[0] == b.edge_index.shape[1] and bool(((p > 0) & (p < 1)).all())
    for k, v in m.named_parameters():
        if v.grad is not None:
            assert bool(torch.isfinite(v.grad).all()), k
    if bool(tr["update_edge_mlp"]):
        assert any(float(v.grad.abs().max()) > 0 for k, v in m.named_parameters() if "edge_prob_mlp" in k and v.grad is not None)


def test_graph_mode_replay_at_nhid_512_matches_eager_recomputation():
    """HIP-graph mode (FusedAdam) at H = 512: a replayed sampled step equals its eager recomputation from the replay's own draws."""
    import sgs_gnn_amd as S
    from sgs_gnn_amd.stepgraph import StepGraphs
    from test_gpu_stepgraph import _check_sampled_replay, _kept
    crit = nn.CrossEntropyLoss()
    b = S.synthetic_graph(300, 20_000, 24, 5, seed=71, device=DEV)
    q = 4_000
    torch.manual_seed(7)
    S.fix_seeds(7)
    m = S.GNNModel(24, 512, 5, dropout_prob=0.0, edge_mlp_type="GCN").to(DEV)
    og, oe = _opts(m, lr=1e-2, cls=S.FusedAdam)
    a = _args(lr=1e-2, sgs_hipgraph=True)
    sg = StepGraphs.attach(m, "hybrid", a, crit, q, False, loader=[b])
    sg.debug_keep = True
    try:
        sg.step(b, 0)
        for p in m.parameters():
            p.grad = None
        c = next(s_ for s_ in sg.slots[True] if s_.live is b)
        for _ in range(2):
            sg.replay_g1(c)
            k = _kept(c, b)
            cnt = c.cbuf.tolist()
            c.g2l.replay()
            gl = {i: g.clone() for i, g in c.grads_l.items()}
            ll = c.loss_l.clone()
            c.g2r.replay()
            gr = {i: g.clone() for i, g in c.grads_r.items()}
            lr_ = c.loss_r.clone()
            torch.cuda.synchronize()
            _check_sampled_replay(S, m, a, crit, b, q, "hybrid", k, cnt, gl, ll, gr, lr_, rel_max=2e-3)
    finally:
        sg.release()
    # and train() in graph mode runs and stays finite
    og, oe = _opts(m, lr=1e-2, cls=S.FusedAdam)
    r = S.train(_args(lr=1e-2, sgs_hipgraph=True), 0, 10, m, og, oe, None, crit, [b], q=q)
    assert torch.isfinite(torch.tensor(float(r[0])))


def test_batched_ensemble_evaluate_at_nhid_512_equals_serial():
    """ensemble_evaluate at H = 512: the batched engine draws the serial loop's edge sets and gives its F1."""
    import sgs_gnn_amd as S
    import sys
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    torch.manual_seed(8)
    b = S.synthetic_graph(600, 30_000, 32, 5, seed=81, train_frac=0.3, power=0.5, device=DEV)
    m = S.GNNModel(32, 512, 5, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
    m.eval()
    q = int(0.2 * b.edge_index.shape[1])
    res = {}
    for path in ("serial", "batched"):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=4)
        if path == "batched":
            args.sgs_eval_batch = True
        args._sgs_trace_eval = {}
        S.manual_seed(3)
        before = dict(ev.PATH_COUNTS)
        f1 = S.ensemble_evaluate(args, copy.deepcopy(m), [b], DEV, q=q, mode="learned")
        assert ev.PATH_COUNTS[path] == before[path] + 1
        res[path] = (f1, args._sgs_trace_eval)
    (f_s, t_s), (f_b, t_b) = res["serial"], res["batched"]
    assert torch.equal(t_s["edges"], t_b["edges"])
    assert f_s == f_b
