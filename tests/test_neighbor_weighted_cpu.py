"""CPU: the weighted fan-out draw.  The library's two host-callable pins (sgs_nbr_log2_table, sgs_nbr_weighted_key) against
tests/neighbor_weighted_ref.py by equality; LOG2Q's error and monotonicity; the distribution of the reference's draw; the tie and zero-weight
rules by hand; the quantisation; and NeighborLoader(weight=...) on CPU tensors (data.neighbor_collate_torch) against the reference."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ref as R  # noqa: E402
import neighbor_weighted_ref as W  # noqa: E402

FIELDS = ("x", "y", "edge_index", "prob", "eid", "node_ids", "seed_mask", "train_mask", "val_mask", "test_mask")
HASHES = sorted({0, 1, 2, 2 ** 32 - 1} | {v for k in range(1, 32) for v in (2 ** k - 1, 2 ** k, 2 ** k + 1)})
WQS = (0, 1, 2, 3, 255, 256, 257, 2 ** 24 - 1)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd as S
    return S._lib.lib()


# ---------------------------------------------------------------- the pins
def test_log2_table_equals_the_reference(lib):
    out = (ctypes.c_int32 * 257)()
    lib.sgs_nbr_log2_table(out)
    assert list(out) == W.TABLE.tolist()
    assert out[0] == 0 and out[256] == 1 << 24 and out[128] == int(math.floor(math.log2(1.5) * 2 ** 24))
    import sgs_gnn_amd.data as D
    assert D._log2_table() == W.TABLE.tolist()


def test_weighted_key_equals_the_reference(lib):
    assert all(0 <= h < 2 ** 32 for h in HASHES) and {0, 1, 2, 3, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1} <= set(HASHES)
    want = W.key_of_hash(np.asarray(HASHES)[:, None], np.asarray(WQS)[None, :])
    got = np.asarray([[lib.sgs_nbr_weighted_key(h, wq) for wq in WQS] for h in HASHES], dtype=np.int64)
    assert np.array_equal(got, want)
    assert (want[:, 0] == W.NO_KEY).all() and (want[:, 1:] < 2 ** 30).all() and (want[:, 1:] >= 0).all()
    rng = np.random.default_rng(0)
    h, wq = rng.integers(0, 2 ** 32, 2000), rng.integers(0, 2 ** 24, 2000)
    assert [lib.sgs_nbr_weighted_key(int(a), int(b)) for a, b in zip(h, wq)] == W.key_of_hash(h, wq).tolist()
    import sgs_gnn_amd.data as D
    assert torch.equal(D._weighted_key_tensor(torch.from_numpy(h), torch.from_numpy(wq)), torch.from_numpy(W.key_of_hash(h, wq)))


def test_log2q_is_monotone_and_within_3e_6_below_log2():
    x = np.arange(1, 70001)
    q = W.log2q(x)
    assert (np.diff(q) >= 0).all() and q[0] == 0
    err = q / 2.0 ** 24 - np.log2(x)
    print("LOG2Q - log2 on 1 .. 70 000: [%.3g, %.3g]" % (err.min(), err.max()))
    assert err.min() >= -3e-6 and err.max() <= 0
    big = np.asarray([2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, 2 ** 29, 3 << 24])
    err = W.log2q(big) / 2.0 ** 24 - np.log2(big.astype(np.float64))
    assert err.min() >= -3e-6 and err.max() <= 1e-12
    assert np.array_equal(W.floor_log2(np.asarray([1, 2, 3, 4, 2 ** 31, 2 ** 32 - 1])), [0, 1, 1, 2, 31, 31])


def test_every_key_of_a_positive_weight_is_below_2_30():
    # the extremes: the largest clock (hash 0 or 1) under the smallest weight, the smallest clock under the largest weight
    assert int(W.key_of_hash(0, 1)) == int(W.key_of_hash(1, 1)) == (29 << 24) + (24 << 24) < 2 ** 30
    assert 0 <= int(W.key_of_hash(2 ** 32 - 1, W.WQ_MAX)) < 1 << 24
    rng = np.random.default_rng(1)
    k = W.key_of_hash(rng.integers(0, 2 ** 32, 100000), rng.integers(1, 2 ** 24, 100000))
    assert k.min() >= 0 and k.max() < 2 ** 30


# ---------------------------------------------------------------- the distribution of the reference's draw
def _counts(ids, wq, f, streams):
    ids, wq = np.asarray(ids, dtype=np.int32), np.asarray(wq, dtype=np.int32)
    ptr = np.asarray([0, ids.shape[0]], dtype=np.int32)
    count = np.zeros(ids.shape[0], dtype=np.int64)
    for K in streams:
        _, c = W.select(ptr, ids, wq, 1, [0], f, K)
        assert c.shape[0] == f
        count[np.searchsorted(ids, c)] += 1
    return count


def _sigmas(count, T, p):
    ok = p > 0
    dev = np.abs(count[ok] - T * p[ok]) / np.sqrt(T * p[ok] * (1 - p[ok]))
    print("worst deviation in sigmas:", float(dev.max()))
    return float(dev.max())


def test_one_draw_is_proportional_to_the_weight():
    T = 8192
    w = np.asarray([1, 2, 3, 5, 8, 13, 100, 1000, 5000, 20000, 65535, 0])
    count = _counts(np.arange(1000, 1012), w, 1, [R.stream_key(7, t, 0, 0) for t in range(T)])
    assert count[-1] == 0 and count.sum() == T                          # the zero-weight edge is never chosen
    assert _sigmas(count, T, w / w.sum()) <= 6.0


def _inclusion(w, f):
    """exact inclusion probabilities of successive sampling without replacement, f draws proportional to w"""
    w = np.asarray(w, dtype=np.float64)
    p = np.zeros(w.shape[0])

    def go(left, prob, depth):
        if depth == f:
            return
        tot = w[left].sum()
        for j in left:
            q = prob * w[j] / tot
            p[j] += q
            go([i for i in left if i != j], q, depth + 1)
    go(list(range(w.shape[0])), 1.0, 0)
    return p


def test_two_draws_follow_successive_sampling():
    T = 8192
    w = np.asarray([1, 2, 3, 4, 10])
    p = _inclusion(w, 2)
    assert np.allclose(p, [0.1269, 0.2479, 0.3621, 0.4680, 0.7951], atol=5e-5) and abs(p.sum() - 2) < 1e-12
    count = _counts(np.arange(50, 55), w, 2, [R.stream_key(3, t, 1, 1) for t in range(T)])
    assert _sigmas(count, T, p) <= 6.0


def test_equal_weights_draw_uniformly():
    T, d, f = 4096, 65, 25
    count = _counts(3 + 7 * np.arange(d), np.full(d, 777), f, [R.stream_key(1, t, 2, 0) for t in range(T)])
    assert _sigmas(count, T, np.full(d, f / d)) <= 6.0


# ---------------------------------------------------------------- hand cases
def test_ties_at_the_threshold_take_the_earliest_and_displace_no_smaller_key():
    ids = np.arange(10, 18, dtype=np.int32)
    keys = np.asarray([5, 9, 5, 1, 5, 5, 9, 0], dtype=np.int64)
    assert W.take_row(ids, keys, 1).tolist() == [17]
    assert W.take_row(ids, keys, 2).tolist() == [13, 17]
    assert W.take_row(ids, keys, 3).tolist() == [10, 13, 17]                 # the first 5 in row order
    assert W.take_row(ids, keys, 4).tolist() == [10, 12, 13, 17]
    assert W.take_row(ids, keys, 6).tolist() == [10, 12, 13, 14, 15, 17]
    assert W.take_row(ids, keys, 7).tolist() == [10, 11, 12, 13, 14, 15, 17]  # the first 9, every 5 kept
    assert W.take_row(ids, keys, 8).tolist() == ids.tolist() and W.take_row(ids, keys, -1).tolist() == ids.tolist()


def test_a_row_short_of_positive_weights_takes_them_and_the_first_zeros():
    ids = np.asarray([40, 41, 42, 43, 44, 45, 46], dtype=np.int32)
    wq = np.asarray([0, 9, 0, 0, 5, 0, 0], dtype=np.int32)
    ptr = np.asarray([0, 7], dtype=np.int32)
    for K in (0, 1, R.stream_key(2, 3, 4, 5)):
        assert W.select(ptr, ids, wq, 1, [0], 4, K)[1].tolist() == [40, 41, 42, 44]
        assert W.select(ptr, ids, wq, 1, [0], 2, K)[1].tolist() == [41, 44]
        one = W.select(ptr, ids, wq, 1, [0], 1, K)[1].tolist()
        assert one in ([41], [44])
        offs, c = W.select(ptr, ids, wq, 1, [0, 5, 0], 3, K)                 # a row outside [0, N) is empty
        assert offs.tolist() == [0, 3, 3, 6] and c.tolist() == [40, 41, 44] * 2


# ---------------------------------------------------------------- quantisation
def test_quantisation():
    import sgs_gnn_amd as S
    rng = np.random.default_rng(3)
    w = np.concatenate([rng.random(500), [0.0, 0.0, 1e-12, 1e-30, 7.5, 7.5 / 2 ** 24, 7.5 / 2 ** 25]])
    q = S.ops.nbr_quantize_weights(torch.from_numpy(w))
    assert q.dtype == torch.int32 and np.array_equal(q.numpy(), W.quantize(w))
    q = q.numpy()
    assert np.array_equal(q == 0, w == 0) and q.max() == q[w == 7.5][0] == 2 ** 24 - 1 and (q[w > 0] >= 1).all()
    order = np.argsort(w, kind="stable")
    assert (np.diff(q[order]) >= 0).all()                                   # monotone
    assert q[-2] == 1 and q[-1] == 1                                        # below max / 2^24: rounded up to one step
    assert np.array_equal(S.ops.nbr_quantize_weights(torch.from_numpy(w.astype(np.float32))).numpy(), W.quantize(w.astype(np.float32)))
    assert S.ops.nbr_quantize_weights(torch.zeros(0)).numel() == 0
    for bad, match in (([1.0, -0.5], "negative"), ([1.0, float("nan")], "finite"), ([1.0, float("inf")], "finite"), ([0.0, 0.0], "zero")):
        with pytest.raises(ValueError, match=match):
            S.ops.nbr_quantize_weights(torch.tensor(bad))
        with pytest.raises(ValueError):
            W.quantize(bad)


# ---------------------------------------------------------------- the loader class on CPU tensors
def _resident(S, g_ei, N, **kw):
    g = R.Graph(g_ei, N)
    data = R.node_data(g, 4, 3, 2)
    prob_unsorted = np.empty_like(data["prob"])
    prob_unsorted[g.order] = data["prob"]
    t = torch.from_numpy
    kw.setdefault("prob", t(prob_unsorted))
    rg = S.ResidentGraph(t(data["x"]), t(np.ascontiguousarray(g_ei)), t(data["y"]), t(data["masks"][0]), t(data["masks"][1]), t(data["masks"][2]),
                         device="cpu", **kw)
    return g, data, rg


def _same(batch, want):
    for k in FIELDS:
        got = getattr(batch, k).cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    assert batch.n_seeds == want["n_seeds"] and batch.hop_nodes == want["hop_nodes"]


def _caller_weights(g, seed):
    """float weights in the CALLER's edge order with zeros and a heavy tail -> (tensor, the reference's wq in in-CSR order)"""
    rng = np.random.default_rng(seed)
    w_sorted = rng.random(g.E) ** 4
    w_sorted[rng.random(g.E) < 0.2] = 0.0
    w_caller = np.empty_like(w_sorted)
    w_caller[g.order] = w_sorted
    return torch.from_numpy(w_caller), W.in_order(g, W.quantize(w_sorted))


@pytest.mark.parametrize("sub", R.SUBGRAPH_TYPES)
@pytest.mark.parametrize("fan", [[3, 2], [25, -1]], ids=str)
def test_cpu_weighted_loader_equals_the_reference(sub, fan):
    import sgs_gnn_amd as S
    for s, (ei, N) in enumerate((R.directed_graph(300, 4000, 5), R.grid_graph(12, 6))):
        g, data, rg = _resident(S, ei, N)
        ids = np.nonzero(data["masks"][0])[0]
        w, wq_in = _caller_weights(g, s)
        ld = rg.neighbor_loader(fan, 32, input_nodes="train", shuffle=True, seed=3, subgraph_type=sub, weight=w)
        assert np.array_equal(ld.weight_q.numpy(), wq_in) and ld.weight_q.dtype == torch.int32
        for ep in range(2):
            got, want = list(ld), W.epoch_batches(g, data, ids, fan, 32, True, 3, ep, sub, wq_in)
            assert len(got) == len(want) == len(ld)
            for a, b in zip(got, want):
                _same(a, b)
        # the graph's own prior as the weight
        wq_prob = W.in_order(g, W.quantize(data["prob"]))
        lp = rg.neighbor_loader(fan, 32, input_nodes="train", shuffle=True, seed=3, subgraph_type=sub, weight="prob")
        assert np.array_equal(lp.weight_q.numpy(), wq_prob)
        for a, b in zip(lp, W.epoch_batches(g, data, ids, fan, 32, True, 3, 0, sub, wq_prob)):
            _same(a, b)
        # one batch through ResidentGraph.batch and through the composition itself
        keys = [R.stream_key(9, 0, 1, h) for h in range(len(fan))]
        want = W.make_batch(g, data, ids[:20], fan, keys, sub, wq_in)
        _same(rg.batch(ids[:20], fan, keys, sub, weight_q=ld.weight_q), want)
        _same(S.neighbor_collate_torch(rg, torch.from_numpy(ids[:20]), fan, keys, sub, weight_q=ld.weight_q), want)
        # set_weight: the next epoch draws with the new weights; None is the uniform draw again
        ld.set_weight("prob")
        ld.set_epoch(1)
        for a, b in zip(ld, W.epoch_batches(g, data, ids, fan, 32, True, 3, 1, sub, wq_prob)):
            _same(a, b)
        ld.set_weight(None)
        for a, b in zip(ld, R.epoch_batches(g, data, ids, fan, 32, True, 3, 1, sub)):
            _same(a, b)


def test_weighted_draw_differs_from_the_uniform_one_and_prefers_heavy_edges():
    import sgs_gnn_amd as S
    ei, N = R.directed_graph(300, 4000, 5)
    g, data, rg = _resident(S, ei, N)
    w, _ = _caller_weights(g, 0)
    w_sorted = w[rg.edge_order]
    keys = [R.stream_key(1, 0, 0, 0)]
    seeds = np.arange(N)
    a = rg.batch(seeds, [3], keys, "directional")
    b = rg.batch(seeds, [3], keys, "directional", weight_q=rg.neighbor_weights(w))
    assert a.eid.numel() == b.eid.numel() and not torch.equal(a.eid, b.eid)
    assert float(w_sorted[b.eid].mean()) > 2 * float(w_sorted[a.eid].mean())


def test_weight_none_equals_the_unweighted_reference():
    import sgs_gnn_amd as S
    ei, N = R.directed_graph(300, 4000, 5)
    g, data, rg = _resident(S, ei, N)
    ids = np.nonzero(data["masks"][0])[0]
    for sub in R.SUBGRAPH_TYPES:
        ld = rg.neighbor_loader([3, 2], 32, input_nodes="train", shuffle=True, seed=3, subgraph_type=sub, weight=None)
        assert ld.weight_q is None
        for a, b in zip(ld, R.epoch_batches(g, data, ids, [3, 2], 32, True, 3, 0, sub)):
            _same(a, b)


def test_argument_errors():
    import sgs_gnn_amd as S
    ei, N = R.grid_graph(6, 1)
    g, _, rg = _resident(S, ei, N)
    _, _, local = _resident(S, ei, N, prior="local", prob=None)
    assert local.prob is None
    with pytest.raises(ValueError, match="prior='local'"):
        local.neighbor_loader([2], 4, weight="prob")
    fixed = rg.neighbor_loader([2], 4, resample="fixed", weight="prob")
    assert fixed.weight_q is not None and len(fixed.batches) == len(fixed)
    with pytest.raises(ValueError, match="fixed"):
        fixed.set_weight(None)
    for bad, match in (("degree", "weight must be"), (torch.ones(g.E + 1), "one floating-point weight per edge"),
                       (torch.ones(g.E, dtype=torch.int64), "one floating-point weight per edge"), (-torch.ones(g.E), "negative"),
                       (torch.zeros(g.E), "zero"), (torch.full((g.E,), float("nan")), "finite")):
        with pytest.raises(ValueError, match=match):
            rg.neighbor_loader([2], 4, weight=bad)
    with pytest.raises(ValueError, match="weight_q"):
        rg.batch([0], [2], [0], weight_q=torch.ones(g.E, dtype=torch.int64))
