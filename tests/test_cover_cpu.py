"""CPU: the node-covering draw's rule (tests/cover_ref.py), the C entry point's checks and host functions, the option's parsing and
its routing.  Nothing here needs a GPU."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import cover_ref as CR


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _random_case(seed, E, N, levels=None, loops=0.15, zeros=0.1):
    """Edges with self-loops, parallel edges (small N), nodes without in-edges (dst drawn from the lower half) and keys from a few
    levels (ties) with some exact zeros."""
    g = np.random.default_rng(seed)
    src = g.integers(0, N, E)
    dst = g.integers(0, max(1, (N + 1) // 2), E)
    loop = g.random(E) < loops
    src[loop] = dst[loop]
    keys = g.random(E).astype(np.float32)
    if levels:
        keys = (np.floor(keys * levels) / levels).astype(np.float32)
    keys[g.random(E) < zeros] = 0.0
    return keys, np.stack([src, dst]), N


CASES = [(s, E, N, lv) for s, (E, N, lv) in enumerate([(1, 2, None), (7, 5, 3), (40, 6, 4), (64, 9, None), (120, 30, 5), (200, 12, 2),
                                                       (200, 150, None), (150, 3, 1)])]


@pytest.mark.parametrize("seed,E,N,levels", CASES)
def test_reference_agrees_with_the_per_node_loop(seed, E, N, levels):
    keys, ei, N = _random_case(seed, E, N, levels)
    for q in sorted({0, 1, E // 5, E // 2, E - 1, E} & set(range(E + 1))):
        a, b = CR.cover_ref(keys, ei, N, q), CR.cover_ref_loop(keys, ei, N, q)
        assert np.array_equal(a["forced"], b["forced"]) and a["M"] == b["M"]
        assert np.array_equal(a["mask"], b["mask"]), q


def test_loops_only_parallel_edges_and_zero_keys():
    # self-loops only: nothing is forced
    keys = np.array([0.5, 0.25, 0.75], dtype=np.float32)
    ei = np.array([[0, 1, 2], [0, 1, 2]])
    r = CR.cover_ref(keys, ei, 3, 2)
    assert r["M"] == 0 and np.array_equal(r["mask"], CR.plain_ref(keys, 2))
    # parallel edges with equal keys: the lowest id is forced; a zero key can be forced; the loop of node 1 never is
    keys = np.array([0.5, 0.5, 0.0, 0.9, 0.0], dtype=np.float32)
    ei = np.array([[0, 0, 2, 1, 3], [1, 1, 0, 1, 0]])
    r = CR.cover_ref(keys, ei, 4, 2)
    assert list(np.nonzero(r["forced"])[0]) == [0, 2] and r["M"] == 2
    assert list(r["eid"]) == [0, 2] and r["threshold_bits"] == 0 and r["ties"] == 1


@pytest.mark.parametrize("seed,E,N,levels", CASES)
def test_consequences_of_the_rule(seed, E, N, levels):
    keys, ei, N = _random_case(seed, E, N, levels)
    bits = CR.key_bits(keys)
    for q in range(0, E + 1, max(1, E // 7)):
        r = CR.cover_ref(keys, ei, N, q)
        M, mask, forced = r["M"], r["mask"], r["forced"]
        assert int(mask.sum()) == q                                         # exactly q, always
        assert r["n_forced_selected"] == min(M, q)
        if M <= q:
            assert bool(mask[forced].all()) and CR.uncovered_nodes(mask, ei, N) == 0
            rest = np.nonzero(~forced)[0]                                   # the other q - M: the plain draw over the rest
            want = rest[CR.top_q(bits[rest], q - M)]
            assert np.array_equal(np.nonzero(mask & ~forced)[0], want)
        else:
            f = np.nonzero(forced)[0]                                       # the q largest-keyed forced edges
            assert np.array_equal(np.nonzero(mask)[0], f[CR.top_q(bits[f], q)])
    loops = np.stack([ei[1], ei[1]])
    for q in (0, E // 2, E):
        r = CR.cover_ref(keys, loops, N, q)                                 # M == 0: the plain draw
        assert r["M"] == 0 and np.array_equal(r["mask"], CR.plain_ref(keys, q))
    assert not CR.cover_ref(keys, ei, N, 0)["mask"].any() and CR.cover_ref(keys, ei, N, E)["mask"].all()


def test_entry_point_validates_without_a_gpu(pkg):
    L = pkg._lib.lib()
    buf = (ctypes.c_int32 * 16)()
    p = ctypes.addressof(buf)

    def call(E, q, N, in_ptr=p, in_src=p, in_eid=p, mode=0):
        return L.sgs_sample_topq_cover(mode, None, None, 0.3, None, 0, 0, E, q, None, N, in_ptr, in_src, in_eid,
                                       None, None, None, None, None, None, None, None, 0, None)

    assert call(10, 11, 4) == -1 and b"sgs_sample_topq_cover" in L.sgs_last_error() and b"without replacement" in L.sgs_last_error()
    assert call(10, 3, -1) == -1 and b"negative node count" in L.sgs_last_error()
    for kw in (dict(in_ptr=None), dict(in_src=None), dict(in_eid=None)):
        assert call(10, 3, 4, **kw) == -1 and b"null destination CSR" in L.sgs_last_error()
    assert call(1 << 32, 3, 4) == -1 and b"exceeds 2^32-1" in L.sgs_last_error()
    assert call(1 << 31, 3, 4) == -1 and b"int32 CSR" in L.sgs_last_error()
    assert call(-1, 0, 4) == -1 and b"negative size" in L.sgs_last_error()
    assert call(10, 3, 4, mode=7) == -1 and b"bad mode" in L.sgs_last_error()
    assert call(10, 3, 4) == -1 and b"null mask" in L.sgs_last_error()       # the CSR passed: the next check is the plain draw's
    assert call(0, 0, 0, in_ptr=None, in_src=None, in_eid=None) == 0         # E == 0: nothing to do, NULL CSR allowed
    # the plain entry point reports under its own name, as before
    rc = L.sgs_sample_topq(0, None, None, 0.3, None, 0, 0, 10, 11, None, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and L.sgs_last_error().startswith(b"sgs_sample_topq: cannot sample")


def test_workspace_query(pkg):
    L = pkg._lib.lib()
    shapes = [(0, 0), (1, 2), (2048, 300), (2049, 300), (100_003, 20_000), (2_097_153, 50_000), (1 << 24, 1 << 20)]
    for E, N in shapes:
        assert L.sgs_sample_topq_cover_workspace_bytes(E, N) >= L.sgs_sample_topq_workspace_bytes(E)
    Es, Ns = sorted({e for e, _ in shapes}), sorted({n for _, n in shapes})
    for N in Ns:
        w = [L.sgs_sample_topq_cover_workspace_bytes(E, N) for E in Es]
        assert w == sorted(w)
    for E in Es:
        w = [L.sgs_sample_topq_cover_workspace_bytes(E, N) for N in Ns]
        assert w == sorted(w)
    assert L.sgs_sample_topq_cover_workspace_bytes(-5, -5) == L.sgs_sample_topq_cover_workspace_bytes(0, 0)


def test_every_variant_is_reached(pkg):
    """Lanes per row of the forced-edge kernel: 4 below a mean in-degree of 8, 16 below 64, else 64."""
    v = pkg._lib.lib().sgs_sample_topq_cover_variant
    assert v(20_000, 160_000 - 1) == 4 and v(20_000, 60_000) == 4 and v(0, 100) == 4 and v(5, 0) == 4
    assert v(20_000, 160_000) == 16 and v(33_869, 463_000) == 16 and v(1000, 63_999) == 16
    assert v(1000, 64_000) == 64 and v(1013, 351_000) == 64 and v(1, 20_000) == 64
    assert {v(n, e) for n, e in ((100, 300), (100, 800), (100, 6400))} == {4, 16, 64}


def test_flag_parsing(pkg):
    from sgs_gnn_amd.sampling import cover_nodes
    assert cover_nodes(argparse.Namespace()) is False
    assert cover_nodes(argparse.Namespace(sgs_cover_nodes=None)) is False
    assert cover_nodes(argparse.Namespace(sgs_cover_nodes=False)) is False
    assert cover_nodes(argparse.Namespace(sgs_cover_nodes=True)) is True
    for bad in (1, 0, "yes", "True", [True], 1.0):
        with pytest.raises(ValueError, match="sgs_cover_nodes"):
            cover_nodes(argparse.Namespace(sgs_cover_nodes=bad))


def _ev():
    import importlib
    return importlib.import_module("sgs_gnn_amd.evaluate")


class _Untouchable:
    """A loader that must not be read."""

    def __iter__(self):
        raise AssertionError("a partition was read")

    def __len__(self):
        raise AssertionError("a partition was read")


def test_a_bad_flag_is_refused_before_any_partition_is_read(pkg):
    S = pkg
    ev = _ev()
    m = S.GNNModel(12, 16, 5, 0.3, "GCN")
    bad = argparse.Namespace(sgs_cover_nodes="on", device="cpu", mode="learned", num_samples_eval=3)
    before = dict(ev.PATH_COUNTS)
    for pipeline in ("hybrid", "straight_through", "two_pass"):
        bad.pipeline = pipeline
        with pytest.raises(ValueError, match="sgs_cover_nodes"):
            S.train(bad, 0, 1, m, None, None, None, torch.nn.CrossEntropyLoss(), _Untouchable(), q=10)
    for mode in ("learned", "random", "edge", "full"):
        with pytest.raises(ValueError, match="sgs_cover_nodes"):
            ev.evaluate(bad, m, _Untouchable(), "cpu", q=10, mode=mode)
        with pytest.raises(ValueError, match="sgs_cover_nodes"):
            ev.ensemble_evaluate(bad, m, _Untouchable(), "cpu", q=10, mode=mode)
    assert ev.PATH_COUNTS == before


def _heads(S):
    return {"GCN": S.GNNModel(12, 16, 5, 0.3, "GCN"), "GAT": S.GATModel(12, 16, 5), "GIN": S.GINModel(12, 16, 5), "Cheb": S.ChebModel(12, 16, 5)}


def test_batched_engine_is_off_under_the_flag_and_unchanged_without_it(pkg):
    ev = _ev()
    for h, m in _heads(pkg).items():
        on = dict(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True)
        assert ev._batched_ok(argparse.Namespace(**on), m, 11) is True, h
        assert ev._batched_ok(argparse.Namespace(**on, sgs_cover_nodes=False), m, 11) is True, h
        assert ev._batched_ok(argparse.Namespace(**on, sgs_cover_nodes=None), m, 11) is True, h
        assert ev._batched_ok(argparse.Namespace(**on, sgs_cover_nodes=True), m, 11) is False, h
        assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=4, sgs_eval_batch_heads=[h], sgs_cover_nodes=True), m, 11) is False, h
        assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True), m, 11) is (h == "GCN"), h
        with pytest.raises(ValueError, match="sgs_cover_nodes"):
            ev._batched_ok(argparse.Namespace(**on, sgs_cover_nodes="all"), m, 11)


def test_sharded_entry_points_refuse_the_flag(pkg):
    from sgs_gnn_amd import sharded
    a = argparse.Namespace(sgs_cover_nodes=True)
    with pytest.raises(NotImplementedError, match="sgs_cover_nodes"):
        sharded.sharded_evaluate_forward(a, None, None, 10)
    with pytest.raises(NotImplementedError, match="sgs_cover_nodes"):
        sharded.train_step_sharded(a, None, None, None, None, None, 10)
    with pytest.raises(NotImplementedError, match="sgs_cover_nodes"):
        sharded.train_step_blocksharded(a, None, None, None, None, None, 10)
    with pytest.raises(NotImplementedError, match="sgs_cover_nodes"):
        sharded.dist_sample_topq(0, None, None, 0.3, 10, None, 0, [0, 10], cover=object())
    with pytest.raises(ValueError, match="sgs_cover_nodes"):
        sharded.train_step_sharded(argparse.Namespace(sgs_cover_nodes=2), None, None, None, None, None, 10)


def test_step_graph_key_and_draw_signatures(pkg):
    """The flag is part of what a captured step bakes in; the draws' positional signatures stay the reference's."""
    import inspect
    from sgs_gnn_amd import sampling
    from sgs_gnn_amd.stepgraph import StepGraphs
    src = inspect.getsource(StepGraphs._config_key)
    assert "cover_nodes(a)" in src
    for fn in (sampling.draw_learned, sampling.draw_prior, sampling.gumbel_softmax_sampling, sampling.random_edge_sampling):
        prm = inspect.signature(fn).parameters["cover"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is None
    assert list(inspect.signature(sampling.gumbel_softmax_sampling).parameters)[:9] == [
        "batch", "edge_probs", "edge_index", "q", "temperature", "degree_bias_coef", "log", "istest", "epoch"]
    with pytest.raises(ValueError, match="node-covering"):
        sampling.random_edge_sampling(torch.zeros(2, 4, dtype=torch.int64), 2, perm=torch.arange(4), cover=object())
