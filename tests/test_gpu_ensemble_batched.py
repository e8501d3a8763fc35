"""GPU: the batched ensemble-evaluation engine (args.sgs_eval_batch) against the oracle, against the serial loop it replaces (same
drawn edge sets, same F1, same noise-clock position), at S3 partition size, and its fall-back to the serial loop for other heads."""
import argparse
import sys

import pytest
import torch

from conftest import load_golden
from oracle import sgs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


def _fixture():
    import sgs_gnn_amd as S
    fx = load_golden("pipeline_hybrid_gcn.pt")
    m = S.GNNModel(fx["x"].shape[1], 16, 5, dropout_prob=0.3, edge_mlp_type="GCN")
    m.load_state_dict(fx["state0"])
    m = m.to(DEV)
    n = fx["x"].shape[0]
    g = torch.Generator().manual_seed(1)
    val = torch.rand(n, generator=g) < 0.5
    b = S.Batch(x=fx["x"], edge_index=fx["edge_index"], y=fx["y"], train_mask=fx["train_mask"], val_mask=val & ~fx["train_mask"],
                test_mask=~val & ~fx["train_mask"], prob=fx["prob"])
    return fx, m, b, g


@pytest.mark.parametrize("flag", [True, 2])
def test_batched_matches_oracle_with_explicit_noise(flag):
    import sgs_gnn_amd as S
    fx, m, b, g = _fixture()
    E, q, draws = fx["edge_index"].shape[1], fx["q"], 5
    noises = [torch.empty(E).exponential_(1, generator=g) for _ in range(draws)]
    args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws, sgs_eval_batch=flag)
    args._sgs_noise_eval = [t.to(DEV) for t in noises]
    before = dict(_ev().PATH_COUNTS)
    got = S.ensemble_evaluate(args, m, [b], DEV, q=q, mode="learned")
    assert _ev().PATH_COUNTS["batched"] == before["batched"] + 1 and _ev().PATH_COUNTS["serial"] == before["serial"]
    P = fx["state0"]
    probs = O.edge_prob_gcn(P, fx["x"], fx["edge_index"], None).squeeze()
    outs = []
    for nz in noises:
        mask, w = O.gumbel_softmax_sampling(None, probs, q, 0.3, True, nz)
        outs.append(O.gnn_forward(P, fx["x"], fx["edge_index"][:, mask], w))
    out = torch.stack(outs).mean(0)
    want = tuple(O.micro_f1(out, fx["y"], mk) for mk in (b.train_mask, b.val_mask, b.test_mask))
    assert got == pytest.approx(want, abs=1e-12)


def _both(S, m, batches, q, mode, draws, flag, seed=7):
    """Both paths from the same randomness state; each result's third entry is (noise-clock tick, dropout-clock tick) afterwards."""
    res = {}
    for path in ("serial", "batched"):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws)
        if path == "batched":
            args.sgs_eval_batch = flag
        args._sgs_trace_eval = {}
        S.manual_seed(seed)
        f1 = S.ensemble_evaluate(args, m, batches, DEV, q=q, mode=mode)
        res[path] = (f1, args._sgs_trace_eval, (S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
    return res


@pytest.mark.parametrize("mode", ["learned", "edge", "random", "full"])
@pytest.mark.parametrize("flag", [True, 3])
def test_batched_equals_serial_with_the_noise_clock(mode, flag):
    import sgs_gnn_amd as S
    fx, m, b, _ = _fixture()
    res = _both(S, m, [b, b], fx["q"], mode, 5, flag)
    (f_s, t_s, k_s), (f_b, t_b, k_b) = res["serial"], res["batched"]
    assert k_s == k_b                     # both clocks: the noise clock and the dropout clock
    assert torch.equal(t_s["edges"], t_b["edges"])
    assert f_s == f_b
    scale = float(t_s["logits"].abs().max())
    assert torch.allclose(t_b["logits"], t_s["logits"], rtol=0, atol=1e-5 * scale)


def _s3_batches():
    import sgs_gnn_amd as S
    sizes = S.reddit_partition_sizes(230, 1000)
    big = min(range(230), key=lambda i: abs(sizes[i] - 351_000))
    small = next(i for i in range(230) if sizes[i] < 100_000)
    parts = S.reddit_partition_stream(num_parts=230, seed=1000, only={big, small})
    return [parts[big].to(DEV), parts[small].to(DEV)]


def test_s3_size_per_draw_logits_counts_and_determinism():
    import sgs_gnn_amd as S
    torch.manual_seed(0)
    batches = _s3_batches()
    assert batches[0].edge_index.shape[1] > 300_000 and batches[1].edge_index.shape[1] < 100_000
    m = S.GNNModel(602, 256, 41, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
    for only in ([batches[0]], [batches[1]]):
        res = _both(S, m, only, 100_000, "learned", 11, True)
        (f_s, t_s, k_s), (f_b, t_b, k_b) = res["serial"], res["batched"]
        assert k_s == k_b                     # both clocks: the noise clock and the dropout clock
        assert torch.equal(t_s["edges"], t_b["edges"])
        scale = float(t_s["logits"].abs().max())
        assert torch.allclose(t_b["logits"], t_s["logits"], rtol=0, atol=1e-5 * scale)
        mean = t_b["mean"]
        bt = only[0]
        pred = mean.argmax(1)
        want = tuple(float(((pred == bt.y) & mk).sum()) / float(mk.sum()) for mk in (bt.train_mask, bt.val_mask, bt.test_mask))
        assert f_b == want
        again = _both(S, m, only, 100_000, "learned", 11, True)["batched"]
        assert again[0] == f_b and torch.equal(again[1]["logits"], t_b["logits"]) and torch.equal(again[1]["mean"], mean)


def test_gat_head_keeps_the_serial_loop():
    import sgs_gnn_amd as S
    fx, _, b, _ = _fixture()
    m = S.GATModel(fx["x"].shape[1], 16, 5, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
    before = dict(_ev().PATH_COUNTS)
    res = _both(S, m, [b], fx["q"], "learned", 3, True)
    assert _ev().PATH_COUNTS["serial"] == before["serial"] + 2 and _ev().PATH_COUNTS["batched"] == before["batched"]
    assert res["serial"][0] == res["batched"][0] and res["serial"][2] == res["batched"][2]
    assert torch.equal(res["serial"][1]["logits"], res["batched"][1]["logits"])


def test_both_clocks_after_sampled_and_whole_partitions_then_training_masks_agree():
    """Sampled partitions, whole partitions (E <= q) and another mode in a row: the dropout clock ends where the serial loop leaves it,
    so the next training forward draws the same dropout seed whichever path evaluated."""
    import sgs_gnn_amd as S
    fx, m, b, _ = _fixture()
    E = fx["edge_index"].shape[1]
    state, seeds = [], []
    for path in ("serial", "batched"):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=4)
        if path == "batched":
            args.sgs_eval_batch = True
        S.manual_seed(3)
        S.ensemble_evaluate(args, m, [b, b], DEV, q=fx["q"], mode="learned")      # sampled
        S.ensemble_evaluate(args, m, [b, b], DEV, q=E, mode="learned")            # E <= q: whole partitions
        S.ensemble_evaluate(args, m, [b], DEV, q=fx["q"], mode="full")
        state.append((S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
        seeds.append(S.model._DropoutClock.next_seed())
    assert state[0] == state[1] and state[0][1] > 0
    assert seeds[0] == seeds[1]
