"""CPU: the multi-draw GAT attention entry point is declared and exported, args.sgs_eval_batch_heads is validated before any partition
is read, and the draws-per-pass planner's per-head byte counts cover every draw within the budget."""
import argparse
import ctypes
import subprocess
import sys

import pytest


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


def _models(S):
    return {"GCN": S.GNNModel(4, 4, 2), "GAT": S.GATModel(4, 4, 2), "GIN": S.GINModel(4, 4, 2), "Cheb": S.ChebModel(4, 4, 2)}


def test_gat_alpha_multi_declared_and_exported(pkg):
    name = "sgs_gat_alpha_fwd_multi"
    protos = pkg._lib.parse_header()
    assert name in protos
    assert [n for n in protos[name][2]] == ["a_src", "a_dst", "a_stride", "N", "D", "nnz", "in_ptr", "in_src", "negative_slope", "alpha_in",
                                            "alpha_loop", "stream"]
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    assert name in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert hasattr(ctypes.CDLL(pkg._lib.LIB_PATH), name)
    assert callable(pkg.ops.gat_alpha_multi)
    for fn in ("ensemble_partition_head", "ensemble_partition"):
        assert callable(getattr(pkg.eval_batch, fn)) and not hasattr(pkg.ops, fn)


def test_gat_alpha_multi_argument_validation(pkg):
    L = pkg._lib.lib()
    # (a_src, a_dst, a_stride, N, D, nnz, in_ptr, in_src, slope, alpha_in, alpha_loop, stream)
    assert L.sgs_gat_alpha_fwd_multi(None, None, 0, 10, 0, 5, None, None, 0.2, None, None, None) == -1
    assert b"bad sizes" in L.sgs_last_error()
    assert L.sgs_gat_alpha_fwd_multi(None, None, 3, 10, 2, 5, None, None, 0.2, None, None, None) == -1       # 0 < a_stride < N
    assert b"a_stride" in L.sgs_last_error()
    assert L.sgs_gat_alpha_fwd_multi(None, None, 10, 10, 2, 5, None, None, 0.2, None, None, None) == -1
    assert b"null pointer" in L.sgs_last_error()
    assert L.sgs_gat_alpha_fwd_multi(None, None, 0, 0, 2, 0, None, None, 0.2, None, None, None) == 0         # N = 0: nothing to do


def test_heads_flag_accepted_values():
    import sgs_gnn_amd as S
    ev = _ev()
    ms = _models(S)
    on = dict(sgs_eval_batch=True)
    for h, m in ms.items():
        assert ev._batched_ok(argparse.Namespace(**on, sgs_eval_batch_heads="all"), m, 11) is True, h
        assert ev._batched_ok(argparse.Namespace(**on, sgs_eval_batch_heads=["GAT"]), m, 11) is (h == "GAT"), h
        assert ev._batched_ok(argparse.Namespace(**on, sgs_eval_batch_heads=None), m, 11) is (h == "GCN"), h
        assert ev._batched_ok(argparse.Namespace(**on), m, 11) is (h == "GCN"), h                  # absent: today's behaviour
        assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=2, sgs_eval_batch_heads=("GIN", "Cheb")), m, 11) is (h in ("GIN", "Cheb")), h


@pytest.mark.parametrize("bad", ["GATX", 3, ["GCN", "Foo"], "GAT", [3], {"GAT": 1}])
def test_heads_flag_bad_values_fail_before_evaluation(bad):
    import sgs_gnn_amd as S
    ev = _ev()
    m = S.GATModel(4, 4, 2)
    before = dict(ev.PATH_COUNTS)

    class Loader:
        def __iter__(self):
            raise AssertionError("a partition was read")

    with pytest.raises(ValueError, match="sgs_eval_batch_heads"):
        S.ensemble_evaluate(argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads=bad, num_samples_eval=11), m, Loader(), "cpu", q=10,
                            mode="learned")
    assert ev.PATH_COUNTS == before


def test_heads_flag_ignored_when_the_engine_is_off():
    import sgs_gnn_amd as S
    ev = _ev()
    for m in _models(S).values():
        for heads in ("all", ["GAT", "GIN", "Cheb", "GCN"], "GATX", 3, None):
            for off in (False, None, 0):
                assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=off, sgs_eval_batch_heads=heads), m, 11) is False
            assert ev._batched_ok(argparse.Namespace(sgs_eval_batch_heads=heads), m, 11) is False


SHAPES = [(351_000, 100_000, 1013, 256, 41), (463_000, 100_000, 33_869, 256, 5), (4_000_000, 1_000_000, 50_000, 256, 41), (64, 10, 8, 16, 5)]


@pytest.mark.parametrize("E,q,N,H,C", SHAPES)
@pytest.mark.parametrize("D", [1, 2, 11])
def test_planner_default_head_is_unchanged(E, q, N, H, C, D):
    ev = _ev()
    for budget in (1, 1 << 20, 64 << 20, 1 << 30, True, 1, 3, 4, 20):
        b = budget if budget is True or budget < 1000 else ("bytes", budget)
        assert ev.plan_draws(E, q, N, H, C, D, b, head="GCN") == ev.plan_draws(E, q, N, H, C, D, b)


@pytest.mark.parametrize("E,q,N,H,C", SHAPES)
@pytest.mark.parametrize("D", [1, 2, 11])
@pytest.mark.parametrize("head", ["GAT", "GIN", "Cheb"])
def test_planner_other_heads_cover_all_draws_within_budget(E, q, N, H, C, D, head):
    ev = _ev()
    base = 4 * ((E + 63) & ~63) + 5 * E + 40 * q + 36 * (N + 1) + 4 * N * H + 8 * N * C
    extra = {"GAT": 4 * q + 12 * N, "GIN": 4 * N * H + 8 * N * C + 4 * q + 4 * N, "Cheb": 0}[head]
    for budget in (1, 1 << 20, 64 << 20, 1 << 30):
        passes = ev.plan_draws(E, q, N, H, C, D, ("bytes", budget), head=head)
        assert sum(passes) == D and all(k >= 1 for k in passes)
        if max(passes) > 1:
            assert max(passes) * (base + extra) <= budget
        gcn = ev.plan_draws(E, q, N, H, C, D, ("bytes", budget))
        assert max(passes) <= max(gcn)                 # a head that allocates more never packs more draws per pass
    for k in (1, 3, 4, 20):
        passes = ev.plan_draws(E, q, N, H, C, D, k, head=head)
        assert sum(passes) == D and max(passes) <= k and min(passes) >= 1
    assert sum(ev.plan_draws(E, q, N, H, C, D, True, head=head)) == D
    with pytest.raises(ValueError):
        ev.plan_draws(E, q, N, H, C, D, True, head="SAGE")
