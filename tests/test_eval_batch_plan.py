"""CPU: the batched ensemble-evaluation entry points are declared and exported, the multi-draw sampler validates its arguments
through sgs_last_error, and the draws-per-pass planner respects its budget."""
import ctypes
import subprocess
import sys

import pytest

NEW = ("sgs_sample_topq_multi_workspace_bytes", "sgs_sample_topq_multi", "sgs_graph_filter_multi_workspace_bytes", "sgs_graph_filter_multi",
       "sgs_gcn_norm_fwd_multi", "sgs_spmm_csr_multi", "sgs_ensemble_mean_correct")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


def test_new_symbols_declared_and_exported(pkg):
    protos = pkg._lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in protos, name
        assert name in exported and hasattr(L, name), name
    for name in ("sample_topq_multi", "ensemble_mean_correct"):
        assert callable(getattr(pkg.ops, name))
    assert callable(pkg.eval_batch.ensemble_partition)


def test_sample_topq_multi_argument_validation(pkg):
    L = pkg._lib.lib()
    # (mode, p, prior, c, noise, seed, sid0, D, E, q, edge_index, mask, eid, sei, stats, st_w, ws, ws_bytes, stream)
    rc = L.sgs_sample_topq_multi(0, None, None, 0.3, None, 0, 0, 0, 10, 5, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"D=0" in L.sgs_last_error()
    rc = L.sgs_sample_topq_multi(0, None, None, 0.3, None, 0, 0, 3, 10, 11, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"without replacement" in L.sgs_last_error()
    rc = L.sgs_sample_topq_multi(0, None, None, 0.3, None, 0, 0, 3, 10, 5, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"null mask" in L.sgs_last_error()
    assert L.sgs_sample_topq_multi_workspace_bytes(500000, 11) >= 11 * 4 * 500000
    assert L.sgs_sample_topq_multi_workspace_bytes(500000, 11) > L.sgs_sample_topq_multi_workspace_bytes(500000, 4)


@pytest.mark.parametrize("E,q,N,H,C", [(351_000, 100_000, 1013, 256, 41), (4_000_000, 1_000_000, 50_000, 256, 41), (64, 10, 8, 16, 5)])
@pytest.mark.parametrize("D", [1, 2, 11])
def test_planner_respects_budget_and_covers_all_draws(E, q, N, H, C, D):
    ev = _ev()
    for budget in (1, 1 << 20, 64 << 20, 1 << 30):
        passes = ev.plan_draws(E, q, N, H, C, D, ("bytes", budget))
        assert sum(passes) == D and all(k >= 1 for k in passes)
        one = ev.plan_draws(E, q, N, H, C, 1, ("bytes", 1 << 62))      # per-draw bytes: a pass of k draws needs k times that
        assert one == [1]
        per = 4 * ((E + 63) & ~63) + 5 * E + 40 * q + 36 * (N + 1) + 4 * N * H + 8 * N * C
        if max(passes) > 1:
            assert max(passes) * per <= budget
    for k in (1, 3, 4, 20):
        passes = ev.plan_draws(E, q, N, H, C, D, k)
        assert sum(passes) == D and max(passes) <= k and min(passes) >= 1
    assert sum(ev.plan_draws(E, q, N, H, C, D, True)) == D
    with pytest.raises(ValueError):
        ev.plan_draws(E, q, N, H, C, D, -1)
    with pytest.raises(ValueError):
        ev.plan_draws(E, q, N, H, C, 0, True)


def test_chunking_4_4_3():
    assert _ev().plan_draws(1000, 100, 10, 16, 5, 11, 4) == [4, 4, 3]


def test_flag_falsy_means_off_and_bad_values_fail_before_evaluation():
    import argparse
    import sgs_gnn_amd as S
    ev = _ev()
    m = S.GNNModel(4, 4, 2)
    for off in (False, None, 0):
        assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=off), m, 11) is False
    assert ev._batched_ok(argparse.Namespace(), m, 11) is False
    assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True), m, 11) and ev._batched_ok(argparse.Namespace(sgs_eval_batch=3), m, 11)
    before = dict(ev.PATH_COUNTS)
    for bad in (-1, 2.5, "4"):
        with pytest.raises(ValueError, match="sgs_eval_batch"):
            S.ensemble_evaluate(argparse.Namespace(sgs_eval_batch=bad, num_samples_eval=11), m, [], "cpu", q=10, mode="learned")
    assert ev.PATH_COUNTS == before                       # refused before a path was counted or a partition was read
