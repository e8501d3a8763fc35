"""GPU: ResidentPartitions.from_graph -- partition_graph plus the constructor -- on a 16-part synthetic graph with shuffled node ids, through
the multi-partition loader and one epoch of the hybrid trainer."""
import argparse
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, NPER, Q = 16, 80, 300


@pytest.fixture(scope="module")
def world():
    import sgs_gnn_amd as S
    b, planted = S.synthetic_partitioned_graph(P, NPER, 1200, 0.25, 7, 3, seed=4)
    rep = {}
    rp = S.ResidentPartitions.from_graph(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, P, partition=dict(seed=1, report=rep),
                                         device=DEV, prob=b.prob, keep_cut_edges=True)
    return dict(S=S, b=b, rp=rp, rep=rep, planted=planted)


def test_partitions_hold_every_edge_but_the_cut(world):
    b, rp, rep = world["b"], world["rp"], world["rep"]
    N, E = P * NPER, int(b.edge_index.shape[1])
    assert rp.num_parts == len(rp) == P and rp.part_id.is_cuda and rp.part_id.dtype == torch.int64 and rp.part_id.shape == (N,)
    sizes = torch.bincount(rp.part_id, minlength=P).cpu()
    assert torch.equal(sizes, rep["sizes"].cpu()) and int(sizes.max()) <= rep["cap"] == math.ceil(1.05 * N / P)
    assert [int(x.x.shape[0]) for x in rp.batches] == sizes.tolist()
    assert sum(int(x.edge_index.shape[1]) for x in rp.batches) == E - rep["cut_edges"]
    assert rp.dropped_edges == rep["cut_edges"] <= rep["cut_edges_initial"]
    ps, pd = rp.part_id.cpu()[b.edge_index[0]], rp.part_id.cpu()[b.edge_index[1]]
    assert int((ps != pd).sum()) == rep["cut_edges"]
    hashed = torch.randperm(N, generator=torch.Generator().manual_seed(0)) % P      # a balanced partition blind to the edges
    assert rep["cut_edges"] < 0.8 * int((hashed[b.edge_index[0]] != hashed[b.edge_index[1]]).sum())


def test_hybrid_epoch_on_the_pairs_loader_accounts_for_the_cut(world):
    S, rp, rep = world["S"], world["rp"], world["rep"]
    torch.manual_seed(0)
    m = S.GNNModel(7, 16, 3, dropout_prob=0.2, edge_mlp_type="GCN").to(DEV)
    og = S.FusedAdam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-2)
    oe = S.FusedAdam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-2)
    args = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", conditional=True, sparse_edge_mlp=True, t_init=0.7, t_min=0.5,
                              degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0, consist_reg_coef=0.5, hybrid_checkpoint=False)
    ld = rp.loader(2, "fixed")
    loss, _, _, tot = S.train(args, 0, 4, m, og, oe, None, torch.nn.CrossEntropyLoss(), ld, q=Q)
    assert tot == len(ld) == P // 2 and math.isfinite(float(loss))
    restored = sum(int(x.restored_edges) for x in ld)
    assert ld.dropped_edges is not None and ld.dropped_edges + restored == rep["cut_edges"] == rp.dropped_edges
    assert restored > 0


def test_partition_graph_refuses_cpu_tensors(world):
    S, b = world["S"], world["b"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.partition_graph(b.edge_index, P * NPER, P)
