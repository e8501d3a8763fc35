"""CPU: the batched covering draw's C entry point (export, workspace query, every guard through the error channel), the routing opt-in
`args.sgs_eval_batch_cover` and the planner's `cover` term.  Nothing here needs a GPU."""
import argparse
import ctypes
import itertools

import pytest


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _ev():
    import importlib
    return importlib.import_module("sgs_gnn_amd.evaluate")


# ------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_bound_from_the_header(pkg):
    L = pkg._lib.lib()
    protos = pkg._lib.parse_header()
    for name in ("sgs_sample_topq_multi_cover", "sgs_sample_topq_multi_cover_workspace_bytes", "sgs_sample_topq_multi_cover_group_set"):
        assert name in protos and hasattr(L, name)
    plain, cover = protos["sgs_sample_topq_multi"][2], protos["sgs_sample_topq_multi_cover"][2]
    # sgs_sample_topq_multi's arguments plus the destination CSR and cover_info
    assert [a for a in cover if a not in ("N", "in_ptr", "in_src", "in_eid", "cover_info")] == plain
    assert cover[cover.index("N"):cover.index("N") + 4] == ["N", "in_ptr", "in_src", "in_eid"]


def test_workspace_query(pkg):
    L = pkg._lib.lib()
    for E, N in [(0, 0), (1, 2), (2049, 300), (4097, 900), (100_003, 20_000), (2_097_153, 50_000)]:
        for D in (1, 2, 5, 11, 64):
            got = L.sgs_sample_topq_multi_cover_workspace_bytes(E, N, D)
            assert got >= L.sgs_sample_topq_multi_workspace_bytes(E, D) + 4 * 1024 * D, (E, N, D)
        w = [L.sgs_sample_topq_multi_cover_workspace_bytes(E, N, D) for D in (1, 2, 5, 11, 64)]
        assert w == sorted(w)
    assert L.sgs_sample_topq_multi_cover_workspace_bytes(-5, -5, 0) == L.sgs_sample_topq_multi_cover_workspace_bytes(0, 0, 1)


def test_every_guard_is_reached_without_a_gpu(pkg):
    L = pkg._lib.lib()
    buf = (ctypes.c_int32 * 1024)()
    p = ctypes.addressof(buf)
    aligned = (p + 255) & ~255
    ws_need = L.sgs_sample_topq_multi_cover_workspace_bytes(10, 4, 3)

    def call(E=10, q=3, N=4, D=3, mode=0, in_ptr=p, in_src=p, in_eid=p, mask=None, pp=None, prior=None, ei=None, eid=None, sei=None,
             stats=None, w=None, ws=None, nws=0):
        return L.sgs_sample_topq_multi_cover(mode, pp, prior, 0.3, None, 0, 0, D, E, q, ei, N, in_ptr, in_src, in_eid, mask, eid, sei, stats,
                                             w, None, ws, nws, None)

    err = L.sgs_last_error
    # sgs_sample_topq_multi's checks, reported under the new name
    assert call(mode=7) == -1 and err().startswith(b"sgs_sample_topq_multi_cover: bad mode")
    for D in (0, -1, 65536):
        assert call(D=D) == -1 and b"sgs_sample_topq_multi_cover" in err() and b"1 <= D <= 65535" in err()
    assert call(E=-1, q=0) == -1 and b"negative size" in err()
    assert call(q=-1) == -1 and b"negative size" in err()
    assert call(E=10, q=11) == -1 and b"without replacement" in err()
    assert call(E=1 << 32) == -1 and b"exceeds 2^32-1" in err()
    # sgs_sample_topq_cover's checks
    assert call(N=-1) == -1 and b"negative node count" in err()
    for kw in (dict(in_ptr=None), dict(in_src=None), dict(in_eid=None)):
        assert call(**kw) == -1 and b"null destination CSR" in err()
    assert call(E=1 << 31) == -1 and b"int32 CSR" in err()
    assert call(N=1 << 31) == -1 and b"int32 CSR" in err()
    # E == 0 returns at once (NULL CSR allowed, nothing written)
    assert call(E=0, q=0, N=0, in_ptr=None, in_src=None, in_eid=None) == 0
    # the rest of the plain multi call's checks, in its order
    assert call() == -1 and b"null mask" in err()
    assert call(mask=p, mode=1) == -1 and b"p == NULL" in err()
    assert call(mask=p, prior=p) == -1 and b"p == NULL" in err()
    assert call(mask=p, sei=p) == -1 and b"edge_index required" in err()
    for kw in (dict(w=p), dict(w=p, pp=p, eid=p), dict(w=p, pp=p, stats=p), dict(w=p, pp=p, eid=p, stats=p, mode=1)):
        assert call(mask=p, **kw) == -1 and b"st_weights needs" in err(), kw
    assert call(mask=p) == -2 and b"workspace too small" in err()
    assert call(mask=p, ws=aligned, nws=ws_need - 1) == -2 and b"workspace too small" in err()
    # the plain call's size is not enough for the covering form
    assert call(mask=p, ws=aligned, nws=L.sgs_sample_topq_multi_workspace_bytes(10, 3)) == -2 and b"workspace too small" in err()
    assert call(mask=p, ws=aligned + 64, nws=ws_need) == -1 and b"256-B aligned" in err()
    # the plain entry point reports under its own name, as before
    rc = L.sgs_sample_topq_multi(0, None, None, 0.3, None, 0, 0, 3, 10, 11, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and err().startswith(b"sgs_sample_topq_multi: cannot sample")


def test_a_dynamic_edge_count_is_refused(pkg):
    L = pkg._lib.lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    assert L.sgs_dyn_edges_set(p) == 0
    try:
        rc = L.sgs_sample_topq_multi_cover(0, None, None, 0.3, None, 0, 0, 3, 10, 3, None, 4, p, p, p, p, None, None, None, None, None, None, 0,
                                           None)
        assert rc == -1 and b"sgs_sample_topq_multi_cover" in L.sgs_last_error() and b"sgs_dyn_edges_set" in L.sgs_last_error()
    finally:
        assert L.sgs_dyn_edges_set(None) == 0


def test_group_size_hook(pkg):
    L = pkg._lib.lib()
    for bad in (3, 8, -1, 5):
        assert L.sgs_sample_topq_multi_cover_group_set(bad) == -1 and b"need 1, 2 or 4" in L.sgs_last_error()
    for g in (1, 2, 4, 0):                                                           # 0: back to the built-in default
        assert L.sgs_sample_topq_multi_cover_group_set(g) == 0


# ------------------------------------------------------------------ routing
class _Untouchable:
    """A loader that must not be read."""

    def __iter__(self):
        raise AssertionError("a partition was read")

    def __len__(self):
        raise AssertionError("a partition was read")


def _models(S):
    """name -> (model, opt-ins beside sgs_eval_batch under which it takes the engine without the cover flag, or None: never)."""
    all_, var = dict(sgs_eval_batch_heads="all"), dict(sgs_eval_batch_heads="all", sgs_eval_batch_variants=True)
    return {
        "GCN": (S.GNNModel(12, 16, 5, 0.3, "GCN"), {}),
        "GAT": (S.GATModel(12, 16, 5), all_),
        "GIN": (S.GINModel(12, 16, 5), all_),
        "Cheb": (S.ChebModel(12, 16, 5), all_),
        "GAT heads=8": (S.GATModel(12, 16, 5, gat_heads=8), var),
        "GAT edge": (S.GATModel(12, 16, 5, gat_edge_weight=True), var),
        "Cheb K=3": (S.ChebModel(12, 16, 5, cheb_k=3), var),
        "GATv2": (S.GATModel(12, 16, 5, gat_v2=True), None),
        "GINE": (S.GINModel(12, 16, 5, gin_edge_weight=True), None),
    }


_ABSENT = object()
OPTINS = [dict(sgs_eval_batch=True), dict(sgs_eval_batch=4), dict(sgs_eval_batch=True, sgs_eval_batch_heads="all"),
          dict(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True),
          dict(sgs_eval_batch=True, sgs_eval_batch_heads=["GAT", "Cheb"], sgs_eval_batch_variants=True), dict(sgs_eval_batch=False), {}]


def test_truth_table(pkg):
    ev = _ev()
    for (name, (m, _)), base in itertools.product(_models(pkg).items(), OPTINS):
        today = ev._batched_ok(argparse.Namespace(**base), m, 11)                    # no cover flag, opt-in absent: unchanged routing
        for cover_flag, optin in itertools.product((_ABSENT, None, False, True), (_ABSENT, None, False, True)):
            kw = dict(base)
            if cover_flag is not _ABSENT:
                kw["sgs_cover_nodes"] = cover_flag
            if optin is not _ABSENT:
                kw["sgs_eval_batch_cover"] = optin
            got = ev._batched_ok(argparse.Namespace(**kw), m, 11)
            if cover_flag is True and optin is not True:
                assert got is False, (name, kw)                                      # today's routing under the flag: the serial loop
            else:
                assert got is today, (name, kw)                                      # the other opt-ins decide exactly as without the flag


def test_the_table_is_not_trivial(pkg):
    """Every head and option has a setting under which the flag plus the opt-in reach the engine, and gat_v2 / gin_edge_weight none."""
    ev = _ev()
    for name, (m, need) in _models(pkg).items():
        full = dict(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True, sgs_cover_nodes=True, sgs_eval_batch_cover=True)
        assert ev._batched_ok(argparse.Namespace(**full), m, 11) is (need is not None), name
        if need is not None:
            a = dict(sgs_eval_batch=True, sgs_cover_nodes=True, sgs_eval_batch_cover=True, **need)
            assert ev._batched_ok(argparse.Namespace(**a), m, 11) is True, name
            if need:                                                                 # one opt-in fewer: the serial loop, as without the flag
                fewer = dict(a)
                fewer.pop(sorted(need)[-1])
                assert ev._batched_ok(argparse.Namespace(**fewer), m, 11) is False, name
    gcn = _models(pkg)["GCN"][0]
    assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_cover_nodes=True, sgs_eval_batch_cover=True), gcn, 0) is False


def test_invalid_values_raise_before_a_loader_is_touched(pkg):
    ev = _ev()
    m = _models(pkg)["GCN"][0]
    for bad in (1, 0, "yes", "True", [True], 1.0):
        for cover_flag in (_ABSENT, False, True):
            kw = dict(sgs_eval_batch=True, sgs_eval_batch_cover=bad, device="cpu", num_samples_eval=3)
            if cover_flag is not _ABSENT:
                kw["sgs_cover_nodes"] = cover_flag
            a = argparse.Namespace(**kw)
            with pytest.raises(ValueError, match="sgs_eval_batch_cover"):
                ev._batched_ok(a, m, 3)
            before = dict(ev.PATH_COUNTS)
            for mode in ("learned", "random", "edge", "full"):
                with pytest.raises(ValueError, match="sgs_eval_batch_cover"):
                    ev.ensemble_evaluate(a, m, _Untouchable(), "cpu", q=10, mode=mode)
            assert ev.PATH_COUNTS == before
        # consulted only when sgs_eval_batch is truthy, as the other opt-ins
        for off in (False, None, 0):
            assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=off, sgs_eval_batch_cover=bad, sgs_cover_nodes=True), m, 3) is False
        assert ev._batched_ok(argparse.Namespace(sgs_eval_batch_cover=bad), m, 3) is False
    # a bad cover flag is still refused first
    with pytest.raises(ValueError, match="sgs_cover_nodes"):
        ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_cover=True, sgs_cover_nodes="on"), m, 3)


# ------------------------------------------------------------------ the planner
SHAPES = [(4097, 2000, 900, 16, 5), (100_003, 20_000, 20_000, 64, 7), (463_000, 90_000, 33_869, 256, 40), (2_097_153, 400_000, 50_000, 128, 10)]
HEAD_KW = [("GCN", {}), ("GAT", {}), ("GIN", {}), ("Cheb", {}), ("GAT", dict(gat_heads=8)), ("GAT", dict(gat_edge=True)),
           ("GAT", dict(gat_heads=4, gat_edge=True)), ("Cheb", dict(cheb_k=3))]


def test_plan_draws_cover_term(pkg):
    ev = _ev()
    smaller = 0
    for (E, q, N, H, C), (head, kw), D in itertools.product(SHAPES, HEAD_KW, (1, 3, 11, 64)):
        budgets = [True, 1, 4, 100] + [("bytes", n) for n in (1, 1 << 20, 8 << 20, 64 << 20, 1 << 30)]
        # budgets at which one more per-draw term can tip a pass: multiples of the per-draw bytes themselves
        for budget in budgets:
            plain = ev.plan_draws(E, q, N, H, C, D, budget, head=head, **kw)
            assert ev.plan_draws(E, q, N, H, C, D, budget, head=head, cover=False, **kw) == plain         # the default is today's list
            cov = ev.plan_draws(E, q, N, H, C, D, budget, head=head, cover=True, **kw)
            assert sum(cov) == D and min(cov) >= 1 and max(cov) <= max(plain)                            # never a larger pass
            if not isinstance(budget, tuple) and budget is not True:
                assert cov == plain                                                                       # "at most k": no byte model
            smaller += max(cov) < max(plain)
    # the term is there: a budget of exactly k plain draws' bytes holds k plain draws and fewer covering ones
    E, q, N, H, C = SHAPES[0]
    per = 4 * ((E + 63) & ~63) + 5 * E + 40 * q + 36 * (N + 1) + 4 * N * H + 8 * N * C + 3 * 2048 * 4 + 64
    assert ev.plan_draws(E, q, N, H, C, 11, ("bytes", 11 * per)) == [11]
    assert ev.plan_draws(E, q, N, H, C, 11, ("bytes", 11 * per), cover=True) == [10, 1]
    assert ev.plan_draws(E, q, N, H, C, 11, ("bytes", 11 * (per + 4 * 1024 + 8)), cover=True) == [11]
    with pytest.raises(TypeError):
        ev.plan_draws(E, q, N, H, C, 11, True, "GCN", 1, False, 1, True)                                 # keyword-only


# ------------------------------------------------------------------ what stays refused
def test_sharded_entry_points_still_raise(pkg):
    from sgs_gnn_amd import sharded
    a = argparse.Namespace(sgs_cover_nodes=True, sgs_eval_batch=True, sgs_eval_batch_cover=True)
    with pytest.raises(NotImplementedError, match="sgs_cover_nodes"):
        sharded.sharded_evaluate_forward(a, None, None, 10)
    with pytest.raises(NotImplementedError, match="sgs_cover_nodes"):
        sharded.train_step_sharded(a, None, None, None, None, None, 10)
    with pytest.raises(NotImplementedError, match="sgs_cover_nodes"):
        sharded.train_step_blocksharded(a, None, None, None, None, None, 10)
    with pytest.raises(NotImplementedError, match="sgs_cover_nodes"):
        sharded.dist_sample_topq(0, None, None, 0.3, 10, None, 0, [0, 10], cover=object())


def test_ops_signatures(pkg):
    import inspect
    ops = pkg.ops
    assert inspect.signature(ops.sample_topq_multi).parameters["cover"].default is None
    for fn in (pkg.eval_batch.ensemble_partition, pkg.eval_batch.ensemble_partition_head):
        prm = inspect.signature(fn).parameters["cover"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is None
    assert "cover_info" in ops.MultiSampleResult.__slots__
    assert not hasattr(pkg.torch_ops, "sample_topq_multi")
