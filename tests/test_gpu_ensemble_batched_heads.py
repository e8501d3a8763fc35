"""GPU: the batched ensemble-evaluation engine for the GAT, GIN and Chebyshev heads (args.sgs_eval_batch_heads): the multi-draw GAT
attention kernel against the single-draw one, the engine against the oracle and against the serial loop (same drawn edge sets, same
clocks, same F1), at bench S4's partition size, and the dropout clock that training sees afterwards."""
import argparse
import sys

import pytest
import torch

from conftest import load_golden
from oracle import sgs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = ("GAT", "GIN", "Cheb")


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


# ------------------------------------------------------------------ 1. sgs_gat_alpha_fwd_multi == sgs_gat_alpha_fwd (p = 0), per draw
def _kernel_graph():
    """300 nodes: 50 isolated (250..299), self loops on nodes 5..39, one duplicated edge, and node 0 with 200 in-edges, so that every
    draw of 600 of the ~880 edges leaves it more than 64 (the wave walks its row more than once)."""
    g = torch.Generator().manual_seed(5)
    hub = torch.stack([torch.arange(1, 201), torch.zeros(200, dtype=torch.int64)])
    rnd = torch.randint(1, 250, (2, 600), generator=g)
    loops = torch.arange(5, 40).repeat(2, 1)
    ei = torch.cat([hub, rnd, loops, rnd[:, :3]], dim=1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous(), 300


def _single_alpha(S, a_s, a_d, graph):
    L = S._lib.lib()
    ops = S.ops
    N, n = graph.N, graph.n_edges
    f32 = dict(dtype=torch.float32, device=DEV)
    soft_in, alpha_in = torch.empty(max(n, 1), **f32), torch.empty(max(n, 1), **f32)
    soft_loop, alpha_loop = torch.empty(N, **f32), torch.empty(N, **f32)
    S._lib.check(L.sgs_gat_alpha_fwd(ops._ptr(a_s), ops._ptr(a_d), N, n, ops._ptr(graph.in_ptr), ops._ptr(graph.in_src), ops._ptr(graph.in_eid),
                                     0.2, 0.0, 0, 16, ops._ptr(soft_in), ops._ptr(soft_loop), ops._ptr(alpha_in), ops._ptr(alpha_loop),
                                     ops._stream()), "sgs_gat_alpha_fwd")
    return alpha_in[:n], alpha_loop


@pytest.mark.parametrize("D", [1, 3, 11])
@pytest.mark.parametrize("shared", [True, False])
def test_gat_alpha_multi_equals_single_draw_kernel(D, shared):
    import sgs_gnn_amd as S
    ops = S.ops
    ei, N = _kernel_graph()
    ei = ei.to(DEV)
    q = 600
    g = torch.Generator().manual_seed(D)
    p = torch.rand(ei.shape[1], generator=g).to(DEV)
    smp = ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.0, q, ei, D, seed=9, stream_id0=1, want_edge_index=True)
    csr = ops.graph_filter_multi(ops.get_graph(ei, N), smp)
    if shared:
        a_s, a_d, stride = torch.randn(N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV), 0
    else:
        a_s, a_d, stride = torch.randn(D, N, generator=g).to(DEV), torch.randn(D, N, generator=g).to(DEV), N
    alpha_in, alpha_loop = ops.gat_alpha_multi(a_s, a_d, stride, csr, q, N, 0.2)
    saw_loop = False
    for d in range(D):
        gd = ops.Graph(smp.edge_index[d].contiguous(), N)
        assert torch.equal(gd.in_ptr, csr[0][d]) and torch.equal(gd.in_src[:q], csr[1][d, :q])
        deg = gd.in_ptr[1:] - gd.in_ptr[:-1]
        assert int(deg[0]) > 64 and int((deg[250:] != 0).sum()) == 0
        src = gd.in_src[:q].long()
        row = torch.repeat_interleave(torch.arange(N, device=DEV), deg.long())
        saw_loop |= bool((src == row).any())
        sa, sd = (a_s, a_d) if shared else (a_s[d].contiguous(), a_d[d].contiguous())
        want_in, want_loop = _single_alpha(S, sa, sd, gd)
        assert torch.equal(alpha_in[d, :q], want_in), d
        assert torch.equal(alpha_loop[d], want_loop), d
        assert bool((alpha_in[d, :q][src == row] == 0).all())
    assert saw_loop


def test_gat_scores_over_stacked_draws_is_per_row():
    import sgs_gnn_amd as S
    g = torch.Generator().manual_seed(3)
    D, N, C = 5, 777, 5
    z = torch.randn(D * N, C, generator=g).to(DEV)
    att_s, att_d = torch.randn(1, 1, C, generator=g).to(DEV), torch.randn(1, 1, C, generator=g).to(DEV)
    a_s, a_d = S.ops.gat_scores(z, att_s, att_d)
    for d in range(D):
        s1, d1 = S.ops.gat_scores(z[d * N:(d + 1) * N].contiguous(), att_s, att_d)
        assert torch.equal(a_s[d * N:(d + 1) * N], s1) and torch.equal(a_d[d * N:(d + 1) * N], d1)


# ------------------------------------------------------------------ 2.-5. the engine
def _model(S, head, fin, hid, ncls, scorer_state=None, seed=0):
    torch.manual_seed(seed)
    cls = {"GAT": S.GATModel, "GIN": S.GINModel, "Cheb": S.ChebModel}[head]
    m = cls(fin, hid, ncls, dropout_prob=0.3, edge_mlp_type="GCN")
    if scorer_state is not None:
        m.load_state_dict({k: v for k, v in scorer_state.items() if k.startswith("edge_prob_mlp.")}, strict=False)
    return m.to(DEV)


def _fixture(head):
    import sgs_gnn_amd as S
    fx = load_golden("pipeline_hybrid_gcn.pt")
    m = _model(S, head, fx["x"].shape[1], 16, 5, fx["state0"])
    n = fx["x"].shape[0]
    g = torch.Generator().manual_seed(1)
    val = torch.rand(n, generator=g) < 0.5
    b = S.Batch(x=fx["x"], edge_index=fx["edge_index"], y=fx["y"], train_mask=fx["train_mask"], val_mask=val & ~fx["train_mask"],
                test_mask=~val & ~fx["train_mask"], prob=fx["prob"])
    return fx, m, b, g


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("flag", [True, 2])
def test_batched_heads_match_oracle_with_explicit_noise(head, flag):
    import sgs_gnn_amd as S
    fx, m, b, g = _fixture(head)
    E, q, draws = fx["edge_index"].shape[1], fx["q"], 5
    noises = [torch.empty(E).exponential_(1, generator=g) for _ in range(draws)]
    args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws, sgs_eval_batch=flag, sgs_eval_batch_heads="all")
    args._sgs_noise_eval = [t.to(DEV) for t in noises]
    before = dict(_ev().PATH_COUNTS)
    got = S.ensemble_evaluate(args, m, [b], DEV, q=q, mode="learned")
    assert _ev().PATH_COUNTS["batched"] == before["batched"] + 1 and _ev().PATH_COUNTS["serial"] == before["serial"]
    P = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    probs = O.edge_prob_gcn(P, fx["x"], fx["edge_index"], None).squeeze()
    outs = []
    for nz in noises:
        mask, _ = O.gumbel_softmax_sampling(None, probs, q, 0.3, True, nz)
        ei = fx["edge_index"][:, mask]
        outs.append(O.gat_forward(P, fx["x"], ei) if head == "GAT" else O.gin_forward(P, fx["x"], ei) if head == "GIN" else O.cheb_forward(P, fx["x"]))
    out = torch.stack(outs).mean(0)
    want = tuple(O.micro_f1(out, fx["y"], mk) for mk in (b.train_mask, b.val_mask, b.test_mask))
    assert got == pytest.approx(want, abs=1e-12)


def _both(S, m, batches, q, mode, draws, flag, seed=7):
    """Both paths from the same randomness state; each result's third entry is (noise-clock tick, dropout-clock tick) afterwards."""
    res = {}
    for path in ("serial", "batched"):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws)
        if path == "batched":
            args.sgs_eval_batch, args.sgs_eval_batch_heads = flag, "all"
        args._sgs_trace_eval = {}
        S.manual_seed(seed)
        before = dict(_ev().PATH_COUNTS)
        f1 = S.ensemble_evaluate(args, m, batches, DEV, q=q, mode=mode)
        assert _ev().PATH_COUNTS[path] == before[path] + 1
        res[path] = (f1, args._sgs_trace_eval, (S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
    return res


def _assert_same(res):
    (f_s, t_s, k_s), (f_b, t_b, k_b) = res["serial"], res["batched"]
    assert set(t_b) == set(t_s) == {"logits", "mean", "edges"}
    assert k_s == k_b                     # both clocks: the noise clock and the dropout clock
    assert torch.equal(t_s["edges"], t_b["edges"])
    assert f_s == f_b
    scale = float(t_s["logits"].abs().max())
    assert t_b["logits"].shape == t_s["logits"].shape
    assert torch.allclose(t_b["logits"], t_s["logits"], rtol=0, atol=1e-5 * scale)


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("mode", ["learned", "edge", "random", "full"])
@pytest.mark.parametrize("flag", [True, 3])
def test_batched_heads_equal_serial_with_the_noise_clock(head, mode, flag):
    import sgs_gnn_amd as S
    fx, m, b, _ = _fixture(head)
    _assert_same(_both(S, m, [b, b], fx["q"], mode, 5, flag))


def test_gat_s4_size_per_draw_logits_counts_and_determinism():
    import sgs_gnn_amd as S
    big = S.synthetic_graph(33_869, 463_000, 128, 5, seed=300, train_frac=0.2, power=0.6, device=DEV)
    small = S.synthetic_graph(33_869, 90_000, 128, 5, seed=301, train_frac=0.2, power=0.6, device=DEV)
    assert big.edge_index.shape[1] > 400_000 and small.edge_index.shape[1] <= 100_000
    m = _model(S, "GAT", 128, 256, 5)
    for only in ([big], [small]):
        res = _both(S, m, only, 100_000, "learned", 11, True)
        _assert_same(res)
        f_b, t_b = res["batched"][0], res["batched"][1]
        bt = only[0]
        pred = t_b["mean"].argmax(1)
        want = tuple(float(((pred == bt.y) & mk).sum()) / float(mk.sum()) for mk in (bt.train_mask, bt.val_mask, bt.test_mask))
        assert f_b == want
        again = _both(S, m, only, 100_000, "learned", 11, True)["batched"]
        assert again[0] == f_b and again[2] == res["batched"][2]
        assert torch.equal(again[1]["logits"], t_b["logits"]) and torch.equal(again[1]["mean"], t_b["mean"])


@pytest.mark.parametrize("head", ["GAT", "GIN"])
def test_training_after_batched_evaluation_draws_the_same_dropout_seed(head):
    """Sampled partitions, then whole partitions (E <= q): the next training forward draws the same dropout seed, and so the same masks,
    whichever path evaluated."""
    import sgs_gnn_amd as S
    fx, m, b, _ = _fixture(head)
    E = fx["edge_index"].shape[1]
    bd = b.to(DEV)
    state, seeds, outs = [], [], []
    for path in ("serial", "batched"):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=4)
        if path == "batched":
            args.sgs_eval_batch, args.sgs_eval_batch_heads = True, [head]
        S.manual_seed(3)
        S.ensemble_evaluate(args, m, [b, b], DEV, q=fx["q"], mode="learned")      # sampled
        S.ensemble_evaluate(args, m, [b], DEV, q=E, mode="learned")               # E <= q: whole partition
        state.append((S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
        m.train()
        with torch.no_grad():
            outs.append(m(bd, bd.edge_index))                                     # a training forward: dropout on
        m.eval()
        seeds.append(S.model._DropoutClock.next_seed())
    assert state[0] == state[1] and state[0][1] > 0
    assert seeds[0] == seeds[1]
    assert torch.equal(outs[0], outs[1])
