"""GPU: ResidentClusterLoader on the device (batches built by ops.cluster_collate) against the class's CPU path, and through the
trainers, the evaluation and the export.  One synthetic partitioned graph: 5 partitions of 80 nodes, ~1 200 stored edges inside each,
a quarter as many again between them."""
import argparse
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, NPER, Q = 5, 80, 300
KEYS = ("x", "edge_index", "y", "train_mask", "val_mask", "test_mask", "prob", "node_ids")


@pytest.fixture(scope="module")
def world():
    import sgs_gnn_amd as S
    b, part = S.synthetic_partitioned_graph(P, NPER, 1200, 0.25, 7, 3, seed=4)
    # the caller's prior on both devices: the device's own degree prior differs from torch's in the last bits, a gathered one cannot
    mk = lambda dev, **kw: S.ResidentPartitions(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, part, num_parts=P, device=dev,  # noqa: E731
                                                keep_cut_edges=True, **kw)
    return dict(S=S, b=b, part=part, cpu=mk("cpu", prob=b.prob), gpu=mk(DEV, prob=b.prob), mk=mk)


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


def _same(a, c):
    for k in KEYS:
        ta, tc = getattr(a, k), getattr(c, k)
        assert ta.is_cuda and ta.dtype == tc.dtype and ta.is_contiguous() and torch.equal(ta.cpu(), tc), k
    assert a.parts == c.parts and a.restored_edges == c.restored_edges


@pytest.mark.parametrize("k,regroup,shuffle", [(1, "fixed", False), (2, "fixed", False), (3, "fixed", True), (2, "epoch", True),
                                               (3, "epoch", False), (P, "epoch", True)])
def test_device_loader_equals_the_cpu_path(world, k, regroup, shuffle):
    g = world["gpu"].loader(k, regroup=regroup, shuffle=shuffle, seed=7)
    c = world["cpu"].loader(k, regroup=regroup, shuffle=shuffle, seed=7)
    assert len(g) == len(c) == math.ceil(P / k) and g.size_path == c.size_path == "table"
    for _ in range(2):
        got, want = list(g), list(c)
        assert len(got) == len(want) == len(g) and g.groups == c.groups
        for a, b in zip(got, want):
            _same(a, b)
        assert g.dropped_edges == c.dropped_edges and g.dropped_edges is not None
    assert (g.batches is None) == (regroup == "epoch")
    assert int(world["gpu"].collate_mismatch.item()) == 0                      # the block table's E_b is the device's count


def test_local_prior_and_read_back_path_on_the_device(world, monkeypatch):
    S = world["S"]
    loc_g, loc_c = world["mk"](DEV, prior="local"), world["mk"]("cpu", prior="local")
    for a, b in zip(loc_g.loader(2), loc_c.loader(2)):
        assert torch.equal(a.edge_index.cpu(), b.edge_index)
        torch.testing.assert_close(a.prob.cpu(), b.prob, rtol=1e-5, atol=1e-9)
    monkeypatch.setattr(S.ResidentPartitions, "CUT_TABLE_MAX_PARTS", 4)
    rb = world["mk"](DEV, prob=world["b"].prob)
    assert rb.size_path == "readback" and rb.block_edges is None
    for a, b in zip(rb.loader(3), world["cpu"].loader(3)):
        _same(a, b)


def test_batch_size_above_the_device_cap_is_refused(world):
    S, b = world["S"], world["b"]
    many = S.ResidentPartitions(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, torch.arange(P * NPER) % 40, num_parts=40,
                                device=DEV, prob=b.prob, keep_cut_edges=True)
    cap = S.ops.cluster_collate_max_parts()
    assert 16 <= cap < 40
    with pytest.raises(ValueError, match="limit"):
        many.loader(cap + 1)
    with pytest.raises(ValueError, match="limit"):
        S.ops.cluster_collate(many, tuple(range(cap + 1)))
    assert many.loader(cap).dropped_edges == many.num_edges - sum(int(x.edge_index.shape[1]) for x in many.loader(cap))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.cluster_collate(world["cpu"], (0, 1))


def test_whole_graph_batch_evaluates_like_a_hand_built_one(world):
    S, b, rp = world["S"], world["b"], world["gpu"]
    N = P * NPER
    perm = rp.perm.cpu()
    new_id = torch.empty(N, dtype=torch.int64)
    new_id[perm] = torch.arange(N)
    s, d = new_id[b.edge_index[0]], new_id[b.edge_index[1]]
    order = torch.argsort(s * N + d)
    whole = S.Batch(x=b.x[perm], edge_index=torch.stack([s[order], d[order]]).contiguous(), y=b.y[perm], train_mask=b.train_mask[perm],
                    val_mask=b.val_mask[perm], test_mask=b.test_mask[perm], prob=b.prob[order]).to(DEV)
    m, _, _ = _model(S)
    ld = rp.loader(P)
    assert len(ld) == 1 and ld.dropped_edges == 0
    for extra in ({}, {"sgs_eval_batch": 2}):
        res = []
        for loader in ([whole], ld):
            S.manual_seed(31)
            res.append(S.ensemble_evaluate(argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, **extra), m, loader, DEV, q=1000,
                                           mode="learned"))
        assert len(res[0]) == 3 and tuple(res[0]) == tuple(res[1]), (extra, res)


def test_one_eager_epoch_on_a_regrouping_loader(world):
    S = world["S"]
    m, og, oe = _model(S)
    ld = world["gpu"].loader(2, regroup="epoch", shuffle=True, seed=2)
    loss, _, _, tot = S.train(_train_args(), 0, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(), ld, q=Q)
    want = sum(1 for g in ld.groups if any(bool(world["gpu"].batches[p].train_mask.any()) for p in g))
    assert tot == want == len(ld) and math.isfinite(float(loss))
    assert ld.dropped_edges is not None and 0 <= ld.dropped_edges < world["gpu"].dropped_edges


def test_regrouping_loader_is_refused_under_replay(world):
    S = world["S"]
    m, og, oe = _model(S)
    ld = world["gpu"].loader(2, regroup="epoch", shuffle=True, seed=2)
    with pytest.raises(ValueError, match="regroup='epoch'"):
        S.train(_train_args(sgs_hipgraph=True), 0, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(), ld, q=Q)
    assert ld.groups is None                                                    # refused before the first batch was drawn


def test_fixed_loader_trains_under_replay(world):
    S = world["S"]
    m, og, oe = _model(S)
    ld = world["gpu"].loader(2, shuffle=True, seed=3)
    args = _train_args(sgs_hipgraph=True)
    for ep in range(4):
        loss, _, _, tot = S.train(args, ep, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(), ld, q=Q)
        assert tot == len(ld) and loss == loss
    assert 1 <= m._sgs_stepgraphs.captures <= 4


def test_sparsify_runs_on_a_fixed_loader(world):
    S = world["S"]
    m, _, _ = _model(S)
    ld = world["gpu"].loader(2)
    S.manual_seed(5)
    out, rep = S.sparsify(argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3), m, ld, DEV, q=Q, mode="learned")
    assert len(out) == len(ld) and rep["edges"]["original"] == sum(int(b.edge_index.shape[1]) for b in ld)
    assert rep["edges"]["original"] == world["gpu"].num_edges - ld.dropped_edges
