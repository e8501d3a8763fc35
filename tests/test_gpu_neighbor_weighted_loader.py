"""GPU: NeighborLoader(weight=...) on the device (every hop drawn by sgs_nbr_select_weighted) against tests/neighbor_weighted_ref.py field by
field, epochs and set_weight, weight=None against the unweighted reference, and a fixed weighted loader through the trainer, eager and
replayed.  Graphs: one directed multigraph and the shuffled 32 x 32 grid."""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ref as R  # noqa: E402
import neighbor_weighted_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = 300
FIELDS = ("x", "y", "edge_index", "prob", "eid", "node_ids", "seed_mask", "train_mask", "val_mask", "test_mask")


@pytest.fixture(scope="module")
def worlds():
    import sgs_gnn_amd as S
    cache = {}

    def get(name):
        if name not in cache:
            ei, N = R.grid_graph(32, 11) if name == "grid" else R.directed_graph(700, 9000, 8)
            g = R.Graph(ei, N)
            data = R.node_data(g, 7, 3, 2)
            rng = np.random.default_rng(5)
            data["prob"] = (data["prob"] * rng.random(g.E) ** 3).astype(np.float32)        # a prior with a heavy tail, so that it moves the draw
            prob = np.empty_like(data["prob"])
            prob[g.order] = data["prob"]                                   # the caller's prior, in the caller's edge order
            w_sorted = rng.random(g.E) ** 4
            w_sorted[rng.random(g.E) < 0.2] = 0.0
            w = np.empty_like(w_sorted)
            w[g.order] = w_sorted                                          # explicit weights, in the caller's edge order
            t = torch.from_numpy
            rg = S.ResidentGraph(t(data["x"]), t(np.ascontiguousarray(ei)), t(data["y"]), t(data["masks"][0]), t(data["masks"][1]),
                                 t(data["masks"][2]), device=DEV, prob=t(prob))
            wqs = {"prob": W.in_order(g, W.quantize(data["prob"])), "tensor": W.in_order(g, W.quantize(w_sorted))}
            cache[name] = (g, data, rg, {"prob": "prob", "tensor": t(w)}, wqs)
        return cache[name]
    return S, get


def _same(batch, want):
    for k in FIELDS:
        t = getattr(batch, k)
        got = t.cpu().numpy()
        assert t.is_cuda and t.is_contiguous() and got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    assert batch.n_seeds == want["n_seeds"] and batch.hop_nodes == want["hop_nodes"]


@pytest.mark.parametrize("kind", ["prob", "tensor"])
@pytest.mark.parametrize("name", ["directed", "grid"])
def test_device_batches_equal_the_reference(worlds, name, kind):
    S, get = worlds
    g, data, rg, weights, wqs = get(name)
    fan, bs = ([5, 3] if name == "directed" else [3, 2]), g.N // 4
    ids = np.nonzero(data["masks"][0])[0]
    for sub in R.SUBGRAPH_TYPES:
        ld = rg.neighbor_loader(fan, bs, input_nodes="train", shuffle=True, seed=3, subgraph_type=sub, weight=weights[kind])
        assert ld.weight_q.is_cuda and np.array_equal(ld.weight_q.cpu().numpy(), wqs[kind])
        eids = []
        for ep in range(2):                                                 # the epoch advances at every __iter__: other batches
            got, want = list(ld), W.epoch_batches(g, data, ids, fan, bs, True, 3, ep, sub, wqs[kind])
            assert len(got) == len(want) == len(ld) >= 2
            for a, b in zip(got, want):
                _same(a, b)
            eids.append(torch.cat([b.eid for b in got]).cpu())
        assert not torch.equal(eids[0], eids[1])
        plain = R.epoch_batches(g, data, ids, fan, bs, True, 3, 0, sub)
        assert not np.array_equal(np.concatenate([b["eid"] for b in plain]), eids[0].numpy())   # the weights move the draw
    # the torch composition on the same device tensors is the same batch
    keys = [S.neighbor_stream_key(3, 1, 0, h) for h in range(2)]
    seeds = R.epoch_seeds(ids, bs, True, 3, 1)[0]
    _same(S.neighbor_collate_torch(rg, torch.from_numpy(seeds), fan, keys, "induced", weight_q=ld.weight_q),
          W.make_batch(g, data, seeds, fan, keys, "induced", wqs[kind]))
    assert int(rg.collate_mismatch.item()) == 0


def test_set_weight_changes_the_next_epoch_and_none_is_the_uniform_draw(worlds):
    S, get = worlds
    g, data, rg, weights, wqs = get("directed")
    ids = np.nonzero(data["masks"][0])[0]
    ld = rg.neighbor_loader([5, 3], 200, input_nodes="train", shuffle=True, seed=4, subgraph_type="directional")
    assert ld.weight_q is None
    for a, b in zip(ld, R.epoch_batches(g, data, ids, [5, 3], 200, True, 4, 0, "directional")):       # weight=None: the unweighted reference
        _same(a, b)
    ld.set_weight(weights["tensor"])
    for a, b in zip(ld, W.epoch_batches(g, data, ids, [5, 3], 200, True, 4, 1, "directional", wqs["tensor"])):
        _same(a, b)
    ld.set_epoch(1)
    ld.set_weight("prob")
    got = list(ld)
    for a, b in zip(got, W.epoch_batches(g, data, ids, [5, 3], 200, True, 4, 1, "directional", wqs["prob"])):
        _same(a, b)
    other = W.epoch_batches(g, data, ids, [5, 3], 200, True, 4, 1, "directional", wqs["tensor"])
    assert not np.array_equal(np.concatenate([b["eid"] for b in other]), torch.cat([b.eid for b in got]).cpu().numpy())
    ld.set_weight(None)
    for a, b in zip(ld, R.epoch_batches(g, data, ids, [5, 3], 200, True, 4, 1, "directional")):
        _same(a, b)
    assert int(rg.collate_mismatch.item()) == 0


def _model(S):
    torch.manual_seed(0)
    m = S.GNNModel(7, 16, 3, dropout_prob=0.2, edge_mlp_type="GCN").to(DEV)
    og = S.FusedAdam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-2)
    oe = S.FusedAdam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-2)
    return m, og, oe


def _train_args(**kw):
    return argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", conditional=True, sparse_edge_mlp=True, t_init=0.7, t_min=0.5,
                              degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0, consist_reg_coef=0.5, hybrid_checkpoint=False,
                              **kw)


def test_fixed_weighted_loader_trains_eagerly_and_under_replay(worlds):
    S, get = worlds
    g, data, rg, weights, wqs = get("directed")
    ids = np.nonzero(data["masks"][0])[0]
    ld = rg.neighbor_loader([5, 3], 175, seed=3, resample="fixed", weight="prob")
    assert len(ld.batches) == len(ld) >= 2 and all(int(b.edge_index.shape[1]) > Q for b in ld.batches)
    for a, b in zip(ld, W.epoch_batches(g, data, ids, [5, 3], 175, True, 3, 0, "induced", wqs["prob"])):
        _same(a, b)
    with pytest.raises(ValueError, match="fixed"):
        ld.set_weight(None)
    for args in (_train_args(), _train_args(sgs_hipgraph=True)):
        m, og, oe = _model(S)
        for ep in range(2 if hasattr(args, "sgs_hipgraph") else 1):         # 2 eager steps; 2 captured and 2 replayed ones
            loss, _, _, tot = S.train(args, ep, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(), ld, q=Q)
            assert tot == len(ld) and math.isfinite(float(loss))
        if hasattr(args, "sgs_hipgraph"):
            assert m._sgs_stepgraphs.captures >= 1
    # a resampling weighted loader is refused under replay like the unweighted one
    m, og, oe = _model(S)
    with pytest.raises(ValueError, match="resample='epoch'"):
        S.train(_train_args(sgs_hipgraph=True), 0, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(),
                rg.neighbor_loader([5, 3], 175, seed=3, weight="prob"), q=Q)
    assert int(rg.collate_mismatch.item()) == 0
