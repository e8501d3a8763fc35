"""CPU: the rules of a neighbour-sampled batch, one hand case each, against tests/neighbor_ref.py; the reference's own properties on the grid
and planted graphs; the uniformity of its selection; and the NeighborLoader class on CPU tensors (data.neighbor_collate_torch) against the
reference, field by field."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ref as R  # noqa: E402

FIELDS = ("x", "y", "edge_index", "prob", "eid", "node_ids", "seed_mask", "train_mask", "val_mask", "test_mask")


def _graph(edges, N):
    return R.Graph(np.asarray(edges, dtype=np.int64).T.reshape(2, -1), N)


def _ids(g, pairs):
    """ids (positions in the sorted list) of the edges (src, dst), first occurrence"""
    return [int(np.nonzero((g.ei[0] == s) & (g.ei[1] == d))[0][0]) for s, d in pairs]


# ---------------------------------------------------------------- hand cases, one per rule
def test_row_shorter_than_the_fan_out_is_taken_whole():
    g = _graph([(1, 0), (2, 0), (3, 0)], 5)
    member, hops, chosen = R.sample(g, [0], [5], [123])
    assert sorted(chosen[0].tolist()) == _ids(g, [(1, 0), (2, 0), (3, 0)]) and hops == [1, 3] and member.tolist() == [True] * 4 + [False]


def test_fan_out_minus_one_takes_every_in_edge():
    g = _graph([(i, 0) for i in range(1, 40)], 40)
    _, hops, chosen = R.sample(g, [0], [-1], [9])
    assert chosen[0].shape[0] == 39 and hops == [1, 39]


def test_longer_row_keeps_the_smallest_keys():
    g = _graph([(i, 0) for i in range(1, 40)], 40)
    K = R.stream_key(0, 0, 0, 0)
    _, hops, chosen = R.sample(g, [0], [4], [K])
    keys = R.edge_keys(np.arange(39), K)
    assert sorted(chosen[0].tolist()) == sorted(np.argsort(keys)[:4].tolist()) and hops == [1, 4]
    assert chosen[0].tolist() == sorted(chosen[0].tolist())                 # row order = ascending id here


def test_a_self_loop_is_an_ordinary_member_of_its_row():
    g = _graph([(0, 0), (1, 0)], 2)
    loop = _ids(g, [(0, 0)])[0]
    K = next(k for k in range(64) if R.edge_keys(np.asarray([loop]), k)[0] < R.edge_keys(np.asarray([1 - loop]), k)[0])
    member, hops, chosen = R.sample(g, [0], [1], [K])
    assert chosen[0].tolist() == [loop] and hops == [1, 0] and member.tolist() == [True, False]
    b = R.make_batch(g, R.node_data(g, 2, 2, 0), [0], [1], [K], "directional")
    assert b["edge_index"].tolist() == [[0], [0]]


def test_a_node_reached_twice_enters_the_frontier_once():
    g = _graph([(2, 0), (2, 1), (3, 2)], 4)
    member, hops, chosen = R.sample(g, [0, 1], [-1, -1], [1, 2])
    assert hops == [2, 1, 1] and chosen[1].tolist() == _ids(g, [(3, 2)]) and member.all()


def test_a_node_reached_at_two_hops_belongs_to_the_first():
    # 0 <- 1, 0 <- 2, 1 <- 2: node 2 is reached at hop 0 and again from 1 at hop 1
    g = _graph([(1, 0), (2, 0), (2, 1), (3, 2)], 4)
    _, hops, chosen = R.sample(g, [0], [-1, -1], [1, 2])
    assert hops == [1, 2, 1]
    assert sorted(chosen[1].tolist()) == sorted(_ids(g, [(2, 1), (3, 2)]))   # 2's own row is walked once, at hop 1
    cat = np.concatenate(chosen)
    assert np.unique(cat).shape[0] == cat.shape[0]


def test_a_directed_graph_is_followed_against_its_arrows_only():
    g = _graph([(0, 1), (1, 2), (2, 3)], 4)
    member, hops, _ = R.sample(g, [2], [-1, -1, -1], [1, 2, 3])
    assert hops == [1, 1, 1, 0] and member.tolist() == [True, True, True, False]
    b = R.make_batch(g, R.node_data(g, 2, 2, 0), [2], [-1, -1, -1], [1, 2, 3], "induced")
    assert b["edge_index"].tolist() == [[0, 1], [1, 2]] and b["seed_mask"].tolist() == [False, False, True]


# ---------------------------------------------------------------- properties
def _worlds():
    ei, N = R.grid_graph(32, 11)
    yield "grid", ei, N
    ei, N, _ = R.planted_graph(1024, 8, 6, 2, 3)
    yield "planted", ei, N


@pytest.fixture(scope="module", params=list(_worlds()), ids=lambda w: w[0])
def world(request):
    _, ei, N = request.param
    g = R.Graph(ei, N)
    return g, R.node_data(g, 5, 4, 1)


def _bfs(g, seeds, L):
    seen = np.zeros(g.N, dtype=bool)
    seen[seeds] = True
    front = np.asarray(seeds)
    for _ in range(L):
        nb = g.ei[0][np.isin(g.ei[1], front)]
        front = np.unique(nb[~seen[nb]])
        seen[front] = True
    return np.nonzero(seen)[0]


@pytest.mark.parametrize("fan", [[5, 3], [2, 2, 2], [-1, -1]])
def test_batch_properties(world, fan):
    g, data = world
    seeds = np.random.default_rng(4).permutation(g.N)[:37]
    keys = [R.stream_key(7, 1, 2, h) for h in range(len(fan))]
    member, hops, chosen = R.sample(g, seeds, fan, keys)
    # every frontier node gets exactly min(f, deg) distinct in-edges
    seen = np.zeros(g.N, dtype=bool)
    seen[seeds] = True
    front = np.sort(seeds)
    deg = np.diff(g.in_ptr.astype(np.int64))
    for f, c in zip(fan, chosen):
        assert np.unique(c).shape[0] == c.shape[0]
        got = np.bincount(g.ei[1][c], minlength=g.N)
        want = np.zeros(g.N, dtype=np.int64)
        want[front] = deg[front] if f < 0 else np.minimum(deg[front], f)
        assert np.array_equal(got, want)
        nb = g.ei[0][c]
        front = np.unique(nb[~seen[nb]])
        seen[front] = True
    assert np.array_equal(seen, member) and sum(hops) == int(member.sum())
    ind = R.make_batch(g, data, seeds, fan, keys, "induced")
    dire = R.make_batch(g, data, seeds, fan, keys, "directional")
    # induced = the brute-force isin subgraph, in ascending edge id, and symmetric on symmetric input
    keep = np.isin(g.ei[0], ind["node_ids"]) & np.isin(g.ei[1], ind["node_ids"])
    assert np.array_equal(ind["eid"], np.nonzero(keep)[0])
    assert np.array_equal(ind["node_ids"][ind["edge_index"]], g.ei[:, keep])
    pairs = set(map(tuple, ind["edge_index"].T.tolist()))
    assert all((b, a) in pairs for a, b in pairs)
    key = ind["edge_index"][0] * g.N + ind["edge_index"][1]
    assert (np.diff(key) >= 0).all()                                        # sorted by (local src, local dst): the relabelling is monotone
    assert np.isin(dire["eid"], ind["eid"]).all() and np.array_equal(dire["eid"], np.sort(np.concatenate(chosen)))
    assert np.array_equal(dire["node_ids"], ind["node_ids"]) and (np.diff(ind["node_ids"]) > 0).all()
    if fan[0] < 0:
        assert np.array_equal(ind["node_ids"], _bfs(g, seeds, len(fan)))
    # masks are restricted to the seeds
    for i, k in enumerate(("train_mask", "val_mask", "test_mask")):
        want = np.zeros(g.N, dtype=bool)
        want[seeds] = data["masks"][i][seeds]
        assert np.array_equal(ind[k], want[ind["node_ids"]])
    assert int(ind["seed_mask"].sum()) == ind["n_seeds"] == 37 and ind["hop_nodes"] == hops


def test_epochs(world):
    g, data = world
    ids = np.nonzero(data["masks"][0])[0]
    a = R.epoch_batches(g, data, ids, [3, 2], 50, True, 5, 0)
    b = R.epoch_batches(g, data, ids, [3, 2], 50, True, 5, 0)
    c = R.epoch_batches(g, data, ids, [3, 2], 50, True, 5, 1)
    assert len(a) == -(-ids.shape[0] // 50)
    for x, y in zip(a, b):
        assert all(np.array_equal(x[k], y[k]) for k in FIELDS)
    seeds = np.concatenate([x["node_ids"][x["seed_mask"]] for x in a])
    assert np.array_equal(np.sort(seeds), ids)                              # every input node is a seed exactly once per epoch
    assert not np.array_equal(np.concatenate([x["eid"] for x in a]), np.concatenate([x["eid"] for x in c]))
    # the same seeds under another epoch's keys: other neighbours
    s = ids[:50]
    e0 = R.make_batch(g, data, s, [2, 2], [R.stream_key(5, 0, 0, h) for h in range(2)], "directional")["eid"]
    e1 = R.make_batch(g, data, s, [2, 2], [R.stream_key(5, 1, 0, h) for h in range(2)], "directional")["eid"]
    assert not np.array_equal(e0, e1)
    assert len(R.epoch_seeds(ids, 50, True, 5, 0, drop_last=True)) == ids.shape[0] // 50


@pytest.mark.parametrize("d,f,first", [(40, 10, 1000), (65, 25, 123456), (7, 3, 0)])
def test_selection_is_uniform(d, f, first):
    """T = 4096 streams K(0, ep, 3, 1); every edge of a row of d is chosen T f / d times within 6 sigma (binomial, p = f / d)"""
    T = 4096
    ptr, eid = np.asarray([0, d], dtype=np.int32), np.arange(first, first + d, dtype=np.int32)
    count = np.zeros(d, dtype=np.int64)
    for ep in range(T):
        _, c = R.select(ptr, eid, 1, [0], f, R.stream_key(0, ep, 3, 1))
        assert c.shape[0] == f
        count[c - first] += 1
    p = f / d
    dev = np.abs(count - T * p) / np.sqrt(T * p * (1 - p))
    print("worst deviation in sigmas:", float(dev.max()))
    assert dev.max() <= 6.0


def test_stream_keys_of_consecutive_ids_are_distinct():
    K = R.stream_key(1, 2, 3, 4)
    assert np.unique(R.edge_keys(np.arange(1 << 16), K)).shape[0] == 1 << 16
    import sgs_gnn_amd as S
    for args in ((0, 0, 0, 0), (1, 2, 3, 4), (2 ** 31, 2 ** 32 - 1, 77, 1)):
        assert S.neighbor_stream_key(*args) == R.stream_key(*args)


# ---------------------------------------------------------------- the loader class on CPU tensors
def _resident(S, g_ei, N, data_of, device="cpu", **kw):
    g = R.Graph(g_ei, N)
    data = data_of(g)
    prob_unsorted = np.empty_like(data["prob"])
    prob_unsorted[g.order] = data["prob"]
    t = torch.from_numpy
    rg = S.ResidentGraph(t(data["x"]), t(np.ascontiguousarray(g_ei)), t(data["y"]), t(data["masks"][0]), t(data["masks"][1]), t(data["masks"][2]),
                         device=device, prob=t(prob_unsorted), **kw)
    return g, data, rg


def _same(batch, want):
    for k in FIELDS:
        got = getattr(batch, k).cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    assert batch.n_seeds == want["n_seeds"] and batch.hop_nodes == want["hop_nodes"]


@pytest.mark.parametrize("sub", R.SUBGRAPH_TYPES)
@pytest.mark.parametrize("fan", [[5, 3], [-1, -1], [2]])
def test_cpu_loader_equals_the_reference(sub, fan):
    import sgs_gnn_amd as S
    for ei, N in (R.grid_graph(12, 3), R.directed_graph(150, 1200, 8)):
        g, data, rg = _resident(S, ei, N, lambda g: R.node_data(g, 4, 3, 2))
        assert torch.equal(rg.edge_index, torch.from_numpy(g.ei)) and not rg.on_device
        ld = rg.neighbor_loader(fan, 32, input_nodes="train", shuffle=True, seed=3, subgraph_type=sub)
        ids = np.nonzero(data["masks"][0])[0]
        for ep in range(2):
            got, want = list(ld), R.epoch_batches(g, data, ids, fan, 32, True, 3, ep, sub)
            assert len(got) == len(want) == len(ld)
            for a, b in zip(got, want):
                _same(a, b)
        ld.set_epoch(0)
        _same(next(iter(ld)), R.epoch_batches(g, data, ids, fan, 32, True, 3, 0, sub)[0])
        fixed = rg.neighbor_loader(fan, 32, input_nodes=torch.from_numpy(ids[:40]), shuffle=False, subgraph_type=sub, resample="fixed", drop_last=True)
        assert len(fixed) == len(fixed.batches) == 1 and list(fixed)[0] is fixed.batches[0]
        _same(fixed.batches[0], R.epoch_batches(g, data, ids[:40], fan, 32, False, 0, 0, sub, drop_last=True)[0])


def test_argument_errors():
    import sgs_gnn_amd as S
    ei, N = R.grid_graph(6, 1)
    _, _, rg = _resident(S, ei, N, lambda g: R.node_data(g, 3, 2, 0))
    for kw, match in ((dict(num_neighbors=[]), "at least one hop"), (dict(num_neighbors=[3, 0]), "fan-out"), (dict(num_neighbors=[-2]), "fan-out"),
                      (dict(subgraph_type="bidirectional"), "bidirectional"), (dict(subgraph_type="other"), "subgraph_type"),
                      (dict(batch_size=0), "batch_size"), (dict(input_nodes=[0, N]), "outside"), (dict(input_nodes=[-1]), "outside"),
                      (dict(input_nodes=[1, 1]), "distinct"), (dict(resample="never"), "resample"), (dict(input_nodes="some"), "input_nodes")):
        args = dict(num_neighbors=[2], batch_size=4)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            rg.neighbor_loader(**args)
    with pytest.raises(ValueError, match="outside"):
        rg.batch([N], [2], [0])
