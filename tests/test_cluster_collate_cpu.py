"""CPU: multi-partition batches with cut edges restored (ResidentPartitions(keep_cut_edges=True) + ResidentClusterLoader) through the
class's CPU path, against the loop restatement of tests/cluster_collate_ref.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cluster_collate_ref import collate_ref, groups_ref  # noqa: E402

P = 7
KEYS = ("x", "edge_index", "y", "train_mask", "val_mask", "test_mask", "prob", "node_ids")


@pytest.fixture(scope="module")
def S():
    import sgs_gnn_amd
    return sgs_gnn_amd


@pytest.fixture(scope="module")
def graph(S):
    b = S.synthetic_graph(90, 900, 7, 3, seed=0)
    part = torch.randint(0, P, (90,), generator=torch.Generator().manual_seed(1))
    return b, part


def _parts(S, b, part, **kw):
    return S.ResidentPartitions(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, part, num_parts=P, device="cpu",
                                keep_cut_edges=True, **kw)


@pytest.fixture(scope="module")
def parts(S, graph):
    return _parts(S, *graph)


def _equals_ref(bt, b, part, prob):
    ref = collate_ref(b.edge_index.numpy(), part.numpy(), bt.parts, prob.numpy())
    ids = torch.from_numpy(ref["node_ids"])
    assert torch.equal(bt.node_ids, ids)
    assert torch.equal(bt.edge_index, torch.from_numpy(ref["edge_index"]))
    assert np.array_equal(bt.prob.numpy().view(np.uint32), ref["prob"].view(np.uint32))          # gathered bit for bit
    assert bt.restored_edges == ref["restored"]
    assert torch.equal(bt.x, b.x[ids]) and torch.equal(bt.y, b.y[ids])
    for k in ("train_mask", "val_mask", "test_mask"):
        assert torch.equal(getattr(bt, k), getattr(b, k)[ids]) and getattr(bt, k).dtype == torch.bool
    return ref


def test_default_arguments_build_the_same_partitions(S, graph, parts):
    b, part = graph
    plain = S.ResidentPartitions(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, part, num_parts=P, device="cpu")
    assert plain.keep_cut_edges is False and not hasattr(plain, "full_ptr")
    assert plain.dropped_edges == parts.dropped_edges
    for a, c in zip(plain.batches, parts.batches):
        for k in KEYS:
            assert torch.equal(getattr(a, k), getattr(c, k)), k


def test_k1_fixed_unshuffled_equals_the_resident_partitions(parts):
    ld = parts.loader(1)
    assert len(ld) == P and ld.batch_size == 1 and ld.regroup == "fixed" and ld.groups == [(p,) for p in range(P)]
    got = list(ld)
    assert len(got) == P
    for a, c in zip(got, parts.batches):
        for k in KEYS:
            assert torch.equal(getattr(a, k), getattr(c, k)) and getattr(a, k).dtype == getattr(c, k).dtype, k
        assert a.restored_edges == 0 and a.parts == (c.part,)
    assert ld.dropped_edges == parts.dropped_edges


def test_k_equals_P_is_the_whole_graph_relabelled(S, graph, parts):
    b, part = graph
    ld = S.ResidentClusterLoader(parts, P)
    assert len(ld) == 1 and ld.dropped_edges == 0
    (bt,) = list(ld)
    assert bt.restored_edges == parts.dropped_edges and bt.edge_index.shape[1] == b.edge_index.shape[1]
    assert torch.equal(bt.node_ids, parts.perm)
    new_id = torch.empty(90, dtype=torch.int64)
    new_id[parts.perm] = torch.arange(90)
    s, d = new_id[b.edge_index[0]], new_id[b.edge_index[1]]
    order = torch.argsort(s * 90 + d)
    assert torch.equal(bt.edge_index, torch.stack([s[order], d[order]]))
    assert torch.equal(bt.prob, b.prob[order])
    _equals_ref(bt, b, part, b.prob)


def test_three_groups_last_of_size_one(graph, parts):
    b, part = graph
    ld = parts.loader(3)
    assert len(ld) == 3 and ld.groups == [(0, 1, 2), (3, 4, 5), (6,)] and ld.batches is not None
    seen = 0
    for bt, g in zip(ld, ld.groups):
        assert bt.parts == g
        _equals_ref(bt, b, part, b.prob)
        seen += bt.edge_index.shape[1]
    assert seen + ld.dropped_edges == b.edge_index.shape[1]
    assert ld.dropped_edges < parts.dropped_edges                      # some cut edges came back


def test_shuffled_epoch_mode(graph, parts):
    b, part = graph
    ld = parts.loader(3, regroup="epoch", shuffle=True, seed=5)
    assert ld.batches is None and ld.dropped_edges is None and len(ld) == 3
    epochs = []
    for _ in range(3):
        seen = 0
        for bt in ld:
            _equals_ref(bt, b, part, b.prob)
            seen += bt.edge_index.shape[1]
        assert ld.dropped_edges == b.edge_index.shape[1] - seen
        assert sorted(p for g in ld.groups for p in g) == list(range(P))            # a partition of range(P)
        assert all(list(g) == sorted(g) for g in ld.groups) and [len(g) for g in ld.groups] == [3, 3, 1]
        epochs.append(ld.groups)
    assert epochs[0] != epochs[1] or epochs[1] != epochs[2]
    again = parts.loader(3, regroup="epoch", shuffle=True, seed=5)
    for want in epochs:
        list(again)
        assert again.groups == want
    gen = torch.Generator().manual_seed(5)                                           # DataLoader(range(P), batch_size=3, shuffle=True)
    assert epochs[0] == groups_ref(torch.randperm(P, generator=gen).tolist(), 3)
    fixed = parts.loader(3, regroup="fixed", shuffle=True, seed=5)
    assert fixed.groups == epochs[0] and [bt.parts for bt in fixed] == epochs[0] and [bt.parts for bt in fixed] == epochs[0]


def test_symmetric_input_gives_symmetric_batches(parts):
    for k in (2, 3):
        for bt in parts.loader(k, shuffle=True, seed=k):
            n = bt.x.shape[0]
            key = bt.edge_index[0] * n + bt.edge_index[1]
            assert bool((key[1:] > key[:-1]).all())                                   # row-sorted and coalesced
            assert torch.equal(torch.sort(bt.edge_index[1] * n + bt.edge_index[0]).values, key)


def test_local_prior_is_the_degree_prior_of_the_batch(S, graph):
    b, part = graph
    rp = _parts(S, b, part, prior="local")
    assert rp.full_prob is None
    for bt in rp.loader(3):
        assert torch.equal(bt.prob, S.degree_prior(bt.edge_index, bt.x.shape[0]))
    for a, c in zip(rp.loader(1), rp.batches):
        assert torch.equal(a.prob, c.prob)


def test_caller_supplied_prob_is_gathered_exactly(S, graph):
    b, part = graph
    mine = torch.rand(b.edge_index.shape[1], generator=torch.Generator().manual_seed(9))
    rp = _parts(S, b, part, prob=mine)
    for bt in rp.loader(2, shuffle=True, seed=1):
        _equals_ref(bt, b, part, mine)


def test_argument_errors(S, graph, parts, tmp_path):
    b, part = graph
    plain = S.ResidentPartitions(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, part, num_parts=P, device="cpu")
    with pytest.raises(ValueError, match="keep_cut_edges"):
        S.ResidentClusterLoader(plain, 2)
    with pytest.raises(ValueError, match="keep_cut_edges"):
        plain.loader(2)
    with pytest.raises(ValueError, match="batch_size"):
        parts.loader(0)
    with pytest.raises(ValueError, match="regroup"):
        parts.loader(2, regroup="sometimes")
    plain.save(str(tmp_path))
    with pytest.raises(ValueError, match="keep_cut_edges"):
        S.ResidentPartitions.load(str(tmp_path), P, device="cpu", keep_cut_edges=True)
    assert S.ResidentPartitions.load(str(tmp_path), P, device="cpu").keep_cut_edges is False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.cluster_collate(parts, (0, 1))


def test_library_refuses_bad_groups_without_a_device(S):
    """The checks of sgs_cluster_collate run before any launch, so the error channel can be exercised on a CPU-only host."""
    L = S._lib.lib()
    cap = L.sgs_cluster_collate_max_parts()
    assert cap >= 16 and cap == S.ops.cluster_collate_max_parts()
    assert L.sgs_cluster_collate_workspace_bytes(1000) >= 1001 * 8              # the int64 rowptr, counted and scanned in place

    def call(ranges, n_b, ws_bytes=1 << 20, k=None):
        arr = (ctypes.c_int64 * max(len(ranges), 1))(*ranges)
        return L.sgs_cluster_collate(64, 64, None, arr, len(ranges) // 2 if k is None else k, n_b, 0, None, None, None, None, None, 0, 100,
                                     None, 64, ws_bytes, None)

    assert call([], 0) == -1 and b"k = 0" in L.sgs_last_error()
    assert call([0, 1] * (cap + 1), cap + 1) == -1 and b"must be in" in L.sgs_last_error()
    assert call([10, 20, 0, 5], 15) == -1 and b"ascending" in L.sgs_last_error()                 # unsorted
    assert call([0, 10, 9, 20], 21) == -1 and b"overlap" in L.sgs_last_error()                    # overlapping
    assert call([0, 10, 10, 20], 19) == -1 and b"n_b" in L.sgs_last_error()
    assert call([0, 10, 10, 20], 20, ws_bytes=64) == -1 and b"workspace too small" in L.sgs_last_error()


def test_block_table_gives_the_counted_edge_numbers(S, graph, parts):
    b, part = graph
    assert parts.size_path == "table" and tuple(parts.block_edges.shape) == (P, P)
    assert int(parts.block_edges.sum()) == b.edge_index.shape[1]
    assert int(parts.block_edges.diagonal().sum()) == b.edge_index.shape[1] - parts.dropped_edges
    loaders = [parts.loader(1), parts.loader(3), parts.loader(P), parts.loader(3, shuffle=True, seed=5), parts.loader(2, shuffle=True, seed=1)]
    for ld in loaders:
        for bt in ld:
            n_b, E_b = parts.batch_sizes(bt.parts)
            ref = collate_ref(b.edge_index.numpy(), part.numpy(), bt.parts)
            assert (n_b, E_b) == (bt.x.shape[0], bt.edge_index.shape[1]) == (ref["node_ids"].shape[0], ref["edge_index"].shape[1])


def test_read_back_path_counts_instead(S, graph, monkeypatch):
    b, part = graph
    monkeypatch.setattr(S.ResidentPartitions, "CUT_TABLE_MAX_PARTS", 4)
    rp = _parts(S, b, part)
    assert rp.size_path == "readback" and rp.block_edges is None and rp.batch_sizes((0, 3)) == (int((part == 0).sum() + (part == 3).sum()), None)
    ld = rp.loader(3)
    assert ld.size_path == "readback"
    for bt in ld:
        _equals_ref(bt, b, part, b.prob)


def test_synthetic_partitioned_graph(S):
    Pn, n, e_intra, cut_frac = 6, 60, 500, 0.25
    b, part = S.synthetic_partitioned_graph(Pn, n, e_intra, cut_frac, 5, 3, seed=2)
    N = Pn * n
    ei = b.edge_index
    assert b.x.shape == (N, 5) and part.shape == (N,) and ei.dtype == torch.int64
    assert torch.equal(torch.bincount(part, minlength=Pn), torch.full((Pn,), n))                  # the stated partitions
    assert not bool((part[1:] >= part[:-1]).all())                                               # not contiguous in the node numbering
    key = ei[0] * N + ei[1]
    assert bool((key[1:] > key[:-1]).all()) and bool((ei[0] != ei[1]).all())                      # coalesced, row-sorted, loop-free
    assert torch.equal(torch.sort(ei[1] * N + ei[0]).values, key)                                 # stored both ways
    assert abs(float(b.prob.sum()) - 1.0) < 1e-4
    cut = int((part[ei[0]] != part[ei[1]]).sum())
    intra = ei.shape[1] - cut
    # every partition holds exactly e_intra // 2 undirected edges (synthetic_graph tops its draw up; 250 is far below its 0.9 * C(60, 2)
    # cap) and the cut pairs are topped up to floor(cut_frac * intra / 2) distinct ones: no dedupe loss is left, so the counts are exact
    # and the share differs from cut_frac / (1 + cut_frac) only by the floor, i.e. by less than 1 / (undirected intra edges)
    assert intra == Pn * 2 * (e_intra // 2)
    assert cut == 2 * int(cut_frac * (intra // 2))
    assert abs(cut / ei.shape[1] - cut_frac / (1 + cut_frac)) < 1.0 / (intra // 2)
    b2, part2 = S.synthetic_partitioned_graph(Pn, n, e_intra, cut_frac, 5, 3, seed=2)
    assert torch.equal(b2.edge_index, ei) and torch.equal(part2, part) and torch.equal(b2.x, b.x)
    rp = S.ResidentPartitions(b.x, ei, b.y, b.train_mask, b.val_mask, b.test_mask, part, num_parts=Pn, device="cpu", keep_cut_edges=True)
    assert rp.dropped_edges == cut and rp.loader(Pn).dropped_edges == 0
