"""GPU: sparsify (the consensus export) on three synthetic partitions of 300 nodes with about 4 000, 6 000 and 900 edges at q = 1 000 (the
last is kept whole).  Everything is compared exactly: the per-edge counts against those recomputed from ensemble_evaluate's traced edge
lists under the same seed, the selection against tests/consensus_ref.py, the noise clock against ensemble_evaluate's, the report against a
torch recomputation, evaluate(mode='full') on the returned list against the model's own forward on the kept edges."""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consensus_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, Q, D, NFEAT, NCLS, SEED = 300, 1000, 11, 8, 4, 123


@pytest.fixture(scope="module")
def world():
    import sgs_gnn_amd as S
    torch.manual_seed(0)
    model = S.GNNModel(NFEAT, 16, NCLS, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
    parts = [S.synthetic_graph(N, e, NFEAT, NCLS, 50 + i).to(DEV) for i, e in enumerate((4000, 6000, 900))]
    assert parts[0].edge_index.shape[1] > Q and parts[1].edge_index.shape[1] > Q and parts[2].edge_index.shape[1] <= Q
    return S, model, parts


def _args(draws=D, **kw):
    return argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws, **kw)


def _traced_counts(S, model, batch, mode, draws=D, **kw):
    """Per-edge keep counts recomputed from the edge lists ensemble_evaluate draws on a one-partition loader, and the noise clock after."""
    args = _args(draws, **kw)
    args._sgs_trace_eval = {}
    S.manual_seed(SEED)
    S.ensemble_evaluate(args, model, [batch], DEV, q=Q, mode=mode)
    edges = args._sgs_trace_eval["edges"].cpu()                                  # [D, 2, q]
    ei = batch.edge_index.cpu()
    key = ei[0] * N + ei[1]
    assert bool((key[1:] > key[:-1]).all())                                      # coalesced and row-sorted: the key names the edge
    ids = torch.searchsorted(key, (edges[:, 0] * N + edges[:, 1]).reshape(-1))
    assert torch.equal(key[ids], (edges[:, 0] * N + edges[:, 1]).reshape(-1))
    return torch.bincount(ids, minlength=key.numel()).numpy().astype(np.int32), S.sampling._NoiseClock.tick


def _score(S, model, batch, mode):
    if mode == "edge":
        return batch.prob.cpu().numpy()
    model.eval()
    with torch.no_grad():
        return model.edge_prob_mlp(batch.x, batch.edge_index).reshape(-1).cpu().numpy()


def _run(S, model, loader, draws=D, mode="learned", **kw):
    args = _args(draws, **{k: v for k, v in kw.items() if k.startswith("sgs_")})
    S.manual_seed(SEED)
    out, rep = S.sparsify(args, model, loader, DEV, q=Q, mode=mode, **{k: v for k, v in kw.items() if not k.startswith("sgs_")})
    return out, rep, S.sampling._NoiseClock.tick


@pytest.mark.parametrize("mode", ["learned", "edge"])
def test_counts_selection_and_clock_match_ensemble_evaluate(world, mode):
    S, model, parts = world
    b = parts[0]
    E = b.edge_index.shape[1]
    count, tick = _traced_counts(S, model, b, mode)
    assert tick == D and int(count.sum()) == D * Q
    out, rep, tick2 = _run(S, model, [b], mode=mode)
    assert tick2 == tick                                                         # the noise clock stands where ensemble_evaluate leaves it
    p = _score(S, model, b, mode)
    want = R.select_ref(count, p, Q, b.edge_index.cpu().numpy())
    k = out[0]
    assert torch.equal(k.edge_id.cpu(), torch.from_numpy(want["eid"]))
    assert torch.equal(k.edge_index.cpu(), torch.from_numpy(want["edge_index"]))
    assert torch.equal(k.edge_freq.cpu(), torch.from_numpy(want["count"]).float() / D)
    assert np.array_equal(k.edge_score.cpu().numpy().view(np.uint32), want["p"].view(np.uint32))
    assert k.x is b.x and k.y is b.y and k.train_mask is b.train_mask and k.val_mask is b.val_mask and k.test_mask is b.test_mask
    assert k.prob.shape == (Q,) and torch.equal(k.prob, S.ops.degree_prior(k.edge_index.clone(), N))     # the kept graph's own prior
    assert torch.equal(rep["freq_hist"], torch.from_numpy(np.bincount(count, minlength=D + 1).astype(np.int64)))
    assert rep["freq_hist"].shape == (D + 1,) and int(rep["freq_hist"].sum()) == E
    assert rep["edges"] == {"original": E, "kept": Q}


def test_result_does_not_depend_on_the_pass_size(world):
    S, model, parts = world
    ref = None
    for k in (1, 4, 11, None):
        out, rep, tick = _run(S, model, parts[:2], sgs_sparsify_pass=k)
        got = ([o.edge_id.cpu() for o in out], [o.edge_freq.cpu() for o in out], rep["freq_hist"], rep["class_pairs"], tick)
        if ref is None:
            ref = got
            continue
        assert all(torch.equal(a, b) for a, b in zip(got[0], ref[0])) and all(torch.equal(a, b) for a, b in zip(got[1], ref[1])), k
        assert torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3]) and got[4] == ref[4] == 2 * D, k


def test_one_draw_returns_the_draw(world):
    S, model, parts = world
    b = parts[1]
    count, tick = _traced_counts(S, model, b, "learned", draws=1)
    assert tick == 1 and set(np.unique(count).tolist()) == {0, 1}
    out, rep, tick2 = _run(S, model, [b], draws=1)
    assert tick2 == 1
    assert torch.equal(out[0].edge_id.cpu(), torch.from_numpy(np.flatnonzero(count)))
    assert bool((out[0].edge_freq == 1).all())
    out2, _, _ = _run(S, model, [b], draws=5, n_draws=1)                         # n_draws overrides args.num_samples_eval
    assert torch.equal(out2[0].edge_id, out[0].edge_id)


@pytest.mark.parametrize("min_freq", [0.5, 1.0, 0.05])
def test_threshold_rule_keeps_exactly_the_frequent_edges(world, min_freq):
    S, model, parts = world
    b = parts[0]
    count, tick = _traced_counts(S, model, b, "learned")
    need = math.ceil(min_freq * D)
    out, rep, tick2 = _run(S, model, [b], rule="threshold", min_freq=min_freq)
    assert tick2 == tick
    keep = np.flatnonzero(count >= need)
    assert torch.equal(out[0].edge_id.cpu(), torch.from_numpy(keep))
    assert torch.equal(out[0].edge_freq.cpu(), torch.from_numpy(count[keep]).float() / D)
    assert rep["edges"]["kept"] == keep.size
    assert keep.size < count.size
    if min_freq == 0.5:
        assert keep.size > 0


def test_small_partition_is_kept_whole(world):
    S, model, parts = world
    b = parts[2]
    E = b.edge_index.shape[1]
    out, rep, tick = _run(S, model, [b])
    assert tick == 0                                                             # no draw is made, as in evaluation
    k = out[0]
    assert torch.equal(k.edge_index, b.edge_index) and torch.equal(k.edge_id.cpu(), torch.arange(E))
    assert bool((k.edge_freq == 1).all()) and k.edge_score.shape == (E,)
    assert int(rep["freq_hist"][D]) == E and int(rep["freq_hist"].sum()) == E
    assert rep["edges"] == {"original": E, "kept": E}
    args = _args()
    S.manual_seed(SEED)
    S.ensemble_evaluate(args, model, [b], DEV, q=Q, mode="learned")
    assert S.sampling._NoiseClock.tick == 0


def _report_by_torch(parts, kept):
    pairs = torch.zeros(2, NCLS, NCLS, dtype=torch.int64)
    holes = [0, 0]
    diff = [0, 0]
    for b, k in zip(parts, kept):
        y = b.y.cpu()
        for s, ei in enumerate((b.edge_index.cpu(), k.edge_index.cpu())):
            pairs[s] += torch.bincount(y[ei[0]] * NCLS + y[ei[1]], minlength=NCLS * NCLS).reshape(NCLS, NCLS)
            holes[s] += int((torch.bincount(ei[1], minlength=N) == 0).sum())
            diff[s] += int((y[ei[0]] != y[ei[1]]).sum())
    return pairs, holes, diff


def test_report_equals_a_torch_recomputation(world):
    S, model, parts = world
    out, rep, tick = _run(S, model, parts)
    assert tick == 2 * D and len(out) == 3
    pairs, holes, diff = _report_by_torch(parts, out)
    n_orig = sum(b.edge_index.shape[1] for b in parts)
    n_kept = 2 * Q + parts[2].edge_index.shape[1]
    assert rep["edges"] == {"original": n_orig, "kept": n_kept}
    assert rep["class_pairs"].dtype == torch.int64 and torch.equal(rep["class_pairs"], pairs)
    assert rep["nodes_without_in_edge"] == {"original": holes[0], "kept": holes[1]}
    for s, (name, tot) in enumerate((("original_graph", n_orig), ("sampled_graph", n_kept))):
        assert rep[name] == {"different_label_edges": diff[s], "total_edges": tot, "percentage": diff[s] / tot * 100}
    assert int(rep["freq_hist"].sum()) == n_orig
    # pooled: a reversed loader (whose partitions meet other ticks of the noise clock, so other draws) reports the same original graph
    out_r, rep_r, _ = _run(S, model, parts[::-1])
    assert torch.equal(rep_r["class_pairs"][0], rep["class_pairs"][0]) and rep_r["original_graph"] == rep["original_graph"]
    assert rep_r["edges"] == rep["edges"] and torch.equal(rep_r["class_pairs"][1], _report_by_torch(parts[::-1], out_r)[0][1])


def test_count_edges_with_different_labels(world):
    S, model, parts = world
    b = parts[1]
    out, _, _ = _run(S, model, [b])
    got = S.count_edges_with_different_labels(b, out[0].edge_index)
    y = b.y.cpu()
    for name, ei in (("original_graph", b.edge_index.cpu()), ("sampled_graph", out[0].edge_index.cpu())):
        d, t = int((y[ei[0]] != y[ei[1]]).sum()), ei.shape[1]
        assert got[name] == {"different_label_edges": d, "total_edges": t, "percentage": d / t * 100}
    empty = S.count_edges_with_different_labels(b, out[0].edge_index[:, :0])
    assert empty["sampled_graph"] == {"different_label_edges": 0, "total_edges": 0, "percentage": 0}


def test_evaluate_full_runs_on_the_returned_list(world):
    S, model, parts = world
    out, _, _ = _run(S, model, parts)
    got = S.evaluate(_args(), model, out, DEV, q=Q, mode="full")
    model.eval()
    hit, tot = [0, 0, 0], [0, 0, 0]
    with torch.no_grad():
        for k in out:
            pred = model(k, k.edge_index).argmax(1)
            for s, m in enumerate((k.train_mask, k.val_mask, k.test_mask)):
                hit[s] += int(((pred == k.y) & m).sum())
                tot[s] += int(m.sum())
    assert got == tuple(h / t for h, t in zip(hit, tot))


def test_cover_nodes_draws(world):
    S, model, parts = world
    plain, rep0, t0 = _run(S, model, parts)
    cover, rep1, t1 = _run(S, model, parts, sgs_cover_nodes=True)
    assert t0 == t1 == 2 * D
    assert rep1["edges"] == rep0["edges"] and all(c.edge_index.shape == p.edge_index.shape for c, p in zip(cover, plain))
    assert rep1["nodes_without_in_edge"]["original"] == rep0["nodes_without_in_edge"]["original"]
    assert rep1["nodes_without_in_edge"]["kept"] <= rep0["nodes_without_in_edge"]["kept"]
    count, _ = _traced_counts(S, model, parts[0], "learned", sgs_cover_nodes=True)        # the covering draws are ensemble_evaluate's too
    want = R.select_ref(count, _score(S, model, parts[0], "learned"), Q)
    assert torch.equal(cover[0].edge_id.cpu(), torch.from_numpy(want["eid"]))
