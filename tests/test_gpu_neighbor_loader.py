"""GPU: NeighborLoader on the device (batches built by ops.neighbor_batch) against tests/neighbor_ref.py field by field, and through the
trainer, the captured replay and the evaluation.  Graphs: the shuffled 32 x 32 grid, a 4 096-node planted graph, one directed multigraph."""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = 300
FIELDS = ("x", "y", "edge_index", "prob", "eid", "node_ids", "seed_mask", "train_mask", "val_mask", "test_mask")


def _make(name):
    if name == "grid":
        ei, N = R.grid_graph(32, 11)
    elif name == "planted":
        ei, N, _ = R.planted_graph(4096, 8, 12, 3, 5)
    else:
        ei, N = R.directed_graph(700, 9000, 8)
    return ei, N


@pytest.fixture(scope="module")
def worlds():
    import sgs_gnn_amd as S
    cache = {}

    def get(name):
        if name not in cache:
            ei, N = _make(name)
            g = R.Graph(ei, N)
            data = R.node_data(g, 7, 3, 2)
            prob = np.empty_like(data["prob"])
            prob[g.order] = data["prob"]                                   # the caller's prior, in the caller's edge order
            t = torch.from_numpy
            rg = S.ResidentGraph(t(data["x"]), t(np.ascontiguousarray(ei)), t(data["y"]), t(data["masks"][0]), t(data["masks"][1]),
                                 t(data["masks"][2]), device=DEV, prob=t(prob))
            cache[name] = (g, data, rg)
        return cache[name]
    return S, get


def _same(batch, want):
    for k in FIELDS:
        t = getattr(batch, k)
        got = t.cpu().numpy()
        assert t.is_cuda and t.is_contiguous() and got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    assert batch.n_seeds == want["n_seeds"] and batch.hop_nodes == want["hop_nodes"]


@pytest.mark.parametrize("fan", [[5, 3], [25, 10], [-1, -1]], ids=str)
@pytest.mark.parametrize("name", ["grid", "planted"])
def test_device_batches_equal_the_reference(worlds, name, fan):
    S, get = worlds
    g, data, rg = get(name)
    assert rg.on_device and torch.equal(rg.edge_index.cpu(), torch.from_numpy(g.ei))
    assert np.array_equal(rg.in_eid.cpu().numpy(), g.in_eid) and np.array_equal(rg.out_dst.cpu().numpy(), g.out_dst)
    bs = g.N // 8
    ids = np.nonzero(data["masks"][0])[0]
    for sub in R.SUBGRAPH_TYPES:
        ld = rg.neighbor_loader(fan, bs, input_nodes="train", shuffle=True, seed=3, subgraph_type=sub)
        ld.set_epoch(1)
        got, want = list(ld), R.epoch_batches(g, data, ids, fan, bs, True, 3, 1, sub)
        assert len(got) == len(want) == len(ld) >= 3
        for a, b in zip(got, want):
            _same(a, b)
    assert int(rg.collate_mismatch.item()) == 0
    # the torch composition on the same device tensors is the same batch
    keys = [S.neighbor_stream_key(3, 1, 0, h) for h in range(2)]
    seeds = R.epoch_seeds(ids, bs, True, 3, 1)[0]
    _same(S.neighbor_collate_torch(rg, torch.from_numpy(seeds), fan, keys, "induced"), R.make_batch(g, data, seeds, fan, keys, "induced"))


def test_directed_graph_tiny_batches_and_epochs(worlds):
    S, get = worlds
    g, data, rg = get("directed")
    for sub in R.SUBGRAPH_TYPES:
        ld = rg.neighbor_loader([3, 2, 2], 100, input_nodes="all", shuffle=False, subgraph_type=sub)
        for ep in range(2):                                                 # the epoch advances at every __iter__
            for a, b in zip(ld, R.epoch_batches(g, data, np.arange(g.N), [3, 2, 2], 100, False, 0, ep, sub)):
                _same(a, b)
        assert ld.epoch == 2
    one = rg.neighbor_loader([4], 1, input_nodes=[5, 6], shuffle=False)
    for a, b in zip(one, R.epoch_batches(g, data, [5, 6], [4], 1, False, 0, 0)):
        _same(a, b)
    with pytest.raises(ValueError, match="hops"):
        rg.neighbor_loader([2] * (S.ops.nbr_max_hops() + 1), 10)
    with pytest.raises(ValueError, match="bidirectional"):
        rg.neighbor_loader([2], 10, subgraph_type="bidirectional")


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


def test_one_eager_epoch_equals_the_same_batches_as_a_list(worlds):
    S, get = worlds
    _, _, rg = get("planted")
    ld = rg.neighbor_loader([5, 3], 512, shuffle=True, seed=2)
    ld.set_epoch(0)
    batches = list(ld)
    assert len(batches) == len(ld) and all(int(b.edge_index.shape[1]) > Q for b in batches)
    losses = []
    for loader in (ld, batches):
        m, og, oe = _model(S)
        S.manual_seed(9)
        loss, _, _, tot = S.train(_train_args(), 0, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(), loader, q=Q)
        assert tot == len(ld) and math.isfinite(float(loss))
        losses.append(float(loss))
    assert losses[0] == losses[1]                                           # bitwise: the loader adds nothing to the step


def test_resampling_loader_is_refused_under_replay(worlds):
    S, get = worlds
    _, _, rg = get("planted")
    m, og, oe = _model(S)
    ld = rg.neighbor_loader([5, 3], 512, seed=2)
    with pytest.raises(ValueError, match="resample='epoch'"):
        S.train(_train_args(sgs_hipgraph=True), 0, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(), ld, q=Q)
    assert ld.epoch == 0                                                    # refused before the first batch was drawn


def test_fixed_loader_trains_under_replay(worlds):
    S, get = worlds
    _, _, rg = get("planted")
    m, og, oe = _model(S)
    ld = rg.neighbor_loader([5, 3], 512, seed=3, resample="fixed")
    assert len(ld.batches) == len(ld) and [b for b in ld][0] is ld.batches[0]
    args = _train_args(sgs_hipgraph=True)
    for ep in range(3):
        loss, _, _, tot = S.train(args, ep, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(), ld, q=Q)
        assert tot == len(ld) and loss == loss
    assert m._sgs_stepgraphs.captures >= 1


def test_evaluate_counts_every_node_once(worlds):
    S, get = worlds
    g, data, rg = get("planted")
    m, _, _ = _model(S)
    ld = rg.neighbor_loader([5, 3], 512, input_nodes="all", shuffle=False)
    rep = {}
    S.manual_seed(4)
    res = S.evaluate(argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=1, sgs_eval_report=rep), m, ld, DEV, q=Q, mode="learned")
    assert len(res) == 3
    per_split = rep["confusion"].sum((1, 2)).tolist()
    assert per_split == data["masks"].sum(1).tolist() and sum(per_split) == g.N
