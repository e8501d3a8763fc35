"""CPU: the third evaluation opt-in, args.sgs_eval_batch_variants (multi-head / edge-weighted GAT and Chebyshev K > 1 on the batched
ensemble engine): routing, flag validation, plan_draws' keyword-only parameters and the new C-ABI declarations."""
import argparse
import sys

import pytest


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


def _models():
    import sgs_gnn_amd as S
    return {"gat_heads4": ("GAT", lambda: S.GATModel(12, 16, 5, gat_heads=4)),
            "gat_edge": ("GAT", lambda: S.GATModel(12, 16, 5, gat_edge_weight=True)),
            "gat_heads4_edge": ("GAT", lambda: S.GATModel(12, 16, 5, gat_heads=4, gat_edge_weight=True)),
            "cheb_k3": ("Cheb", lambda: S.ChebModel(12, 16, 5, cheb_k=3)),
            "gat_heads16": ("GAT", lambda: S.GATModel(12, 16, 5, gat_heads=16)),
            "cheb_k8": ("Cheb", lambda: S.ChebModel(12, 16, 5, cheb_k=8))}


NAMES = ("gat_heads4", "gat_edge", "gat_heads4_edge", "cheb_k3", "gat_heads16", "cheb_k8")


@pytest.mark.parametrize("name", NAMES)
def test_variants_take_the_engine_only_with_all_three_flags(name):
    ev = _ev()
    head, make = _models()[name]
    m = make()
    for flag in (True, 3):
        for heads in ("all", [head]):
            on = argparse.Namespace(sgs_eval_batch=flag, sgs_eval_batch_heads=heads, sgs_eval_batch_variants=True)
            assert ev._batched_ok(on, m, 11) is True
    # absent, None, False: today's routing
    assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all"), m, 11) is False
    for off in (None, False):
        assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=off), m, 11) is False
    # head not selected
    other = ["Cheb"] if head == "GAT" else ["GAT"]
    for heads in (None, other, ["GCN", "GIN"]):
        assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads=heads, sgs_eval_batch_variants=True), m, 11) is False
    # the first opt-in off: nothing else is consulted
    assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=False, sgs_eval_batch_variants="bad"), m, 11) is False
    assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True), m, 0) is False


def test_default_models_route_as_before_whatever_the_new_flag():
    import sgs_gnn_amd as S
    ev = _ev()
    for v in (None, False, True):
        a = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=v)
        for m in (S.GNNModel(12, 16, 5), S.GATModel(12, 16, 5), S.GINModel(12, 16, 5), S.ChebModel(12, 16, 5)):
            assert ev._batched_ok(a, m, 11) is True
        b = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_variants=v)
        assert ev._batched_ok(b, S.GNNModel(12, 16, 5), 11) is True and ev._batched_ok(b, S.GATModel(12, 16, 5), 11) is False


@pytest.mark.parametrize("bad", [1, 0, "all", "True", [True], 2.0])
def test_bad_variant_flags_raise_before_any_partition_is_read(bad):
    import sgs_gnn_amd as S
    ev = _ev()
    a = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=bad, num_samples_eval=3)
    with pytest.raises(ValueError, match="sgs_eval_batch_variants"):
        ev._batched_ok(a, S.GNNModel(12, 16, 5), 3)
    with pytest.raises(ValueError, match="sgs_eval_batch_variants"):
        ev._batched_ok(a, S.GATModel(12, 16, 5, gat_heads=4), 0)

    class Loader:
        def __iter__(self):
            raise AssertionError("a partition was read")
    with pytest.raises(ValueError, match="sgs_eval_batch_variants"):
        S.ensemble_evaluate(a, S.GATModel(12, 16, 5, gat_heads=4), Loader(), "cpu", q=10, mode="learned")


PLAN_CASES = [(351_000, 100_000, 1013, 256, 41), (4_000_000, 1_000_000, 50_000, 256, 41), (64, 10, 8, 16, 5)]      # tests/test_eval_batch_plan.py's


def _todays_plan(E, q, N, H, C, D, budget, head="GCN"):
    """plan_draws as it stood before the keyword-only parameters (restated): the lists every existing call must keep."""
    if budget is True or isinstance(budget, tuple):
        nbytes = (512 << 20) if budget is True else budget[1]
        per = 4 * ((E + 63) & ~63) + E + 4 * E + 40 * q + 36 * (N + 1) + 4 * N * H + 8 * N * C + 3 * 2048 * 4 + 64
        per += {"GCN": 0, "Cheb": 0, "GAT": 4 * q + 12 * N, "GIN": 4 * N * H + 8 * N * C + 4 * q + 4 * N}[head]
        k = max(1, min(D, nbytes // per))
    else:
        k = min(budget, D)
    return [k] * (D // k) + ([D % k] if D % k else [])


@pytest.mark.parametrize("E,q,N,H,C", PLAN_CASES)
@pytest.mark.parametrize("D", [1, 2, 11])
def test_plan_draws_default_keywords_are_todays_lists(E, q, N, H, C, D):
    ev = _ev()
    assert ev.EVAL_BATCH_BUDGET == 512 << 20
    for head in ev.HEADS:
        for budget in (True, 1, 3, 4, 20, ("bytes", 1), ("bytes", 1 << 20), ("bytes", 64 << 20), ("bytes", 1 << 30), ("bytes", 1 << 62)):
            want = _todays_plan(E, q, N, H, C, D, budget, head)
            assert ev.plan_draws(E, q, N, H, C, D, budget, head) == want
            assert ev.plan_draws(E, q, N, H, C, D, budget, head=head, gat_heads=1, gat_edge=False, cheb_k=1) == want
    assert ev.plan_draws(1000, 100, 10, 16, 5, 11, 4) == [4, 4, 3]


def test_plan_draws_variant_keywords_are_keyword_only_monotone_and_sum_to_d():
    ev = _ev()
    big = dict(E=463_000, q=100_000, N=33_869, H=256, C=41)
    with pytest.raises(TypeError):
        ev.plan_draws(463_000, 100_000, 33_869, 256, 41, 11, True, "GAT", 8)
    for D in (1, 5, 11):
        for nbytes in (1 << 20, 64 << 20, 256 << 20, 512 << 20, 4 << 30):
            last = None
            for K in range(1, 17):
                for edge in (False, True):
                    plan = ev.plan_draws(D=D, budget=("bytes", nbytes), head="GAT", gat_heads=K, gat_edge=edge, **big)
                    assert sum(plan) == D and min(plan) >= 1
                    assert max(plan) <= max(ev.plan_draws(D=D, budget=("bytes", nbytes), head="GAT", gat_heads=K, **big))
                k = max(ev.plan_draws(D=D, budget=("bytes", nbytes), head="GAT", gat_heads=K, **big))
                assert last is None or k <= last
                last = k
            last = None
            for K in range(1, 9):
                plan = ev.plan_draws(D=D, budget=("bytes", nbytes), head="Cheb", cheb_k=K, **big)
                assert sum(plan) == D and min(plan) >= 1
                assert last is None or max(plan) <= last
                last = max(plan)
            assert ev.plan_draws(D=D, budget=3, head="GAT", gat_heads=8, gat_edge=True, **big) == ev.plan_draws(D=D, budget=3, **big)
    for kw in (dict(gat_heads=0), dict(gat_heads=17), dict(cheb_k=0), dict(cheb_k=9)):
        with pytest.raises(ValueError):
            ev.plan_draws(D=3, budget=True, head="GAT", **big, **kw)


MULTI_EXPORTS = ("sgs_gat_alpha_heads_fwd_multi", "sgs_spmm_csr_heads_multi", "sgs_cheb_norm_fwd_multi_workspace_bytes", "sgs_cheb_norm_fwd_multi",
                 "sgs_cheb_spmm_multi")


def test_header_declares_the_multi_draw_entry_points_and_the_library_resolves_them():
    import sgs_gnn_amd
    protos = sgs_gnn_amd._lib.parse_header()
    L = sgs_gnn_amd._lib.lib()
    for name in MULTI_EXPORTS:
        assert name in protos, name
        assert getattr(L, name) is not None
    assert protos["sgs_gat_alpha_heads_fwd_multi"][2][:5] == ["a_src", "a_dst", "a_stride", "edge_w", "edge_coef"]
    assert L.sgs_cheb_norm_fwd_multi_workspace_bytes(1000, 11) >= 4 * 1000 * 11


def test_multi_draw_entry_points_validate_on_the_host():
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()
    rc = L.sgs_gat_alpha_heads_fwd_multi(None, None, 0, None, None, 10, 17, 3, 0, None, None, None, 0.2, None, None, None)
    assert rc == -1 and b"unsupported heads" in L.sgs_last_error()
    rc = L.sgs_spmm_csr_heads_multi(None, 0, 10, 4, 8, 0, 0, None, None, None, None, None, 0, None, 0, None, None)
    assert rc == -1 and b"1 <= D <= 65535" in L.sgs_last_error()
    rc = L.sgs_cheb_spmm_multi(9, None, 4, 0, 10, 4, 0, 3, None, None, None, 1.0, None, 0, 0, None, 0, 0, None, 0, None, 4, 40, None)
    assert rc == -1 and b"unsupported Chebyshev order" in L.sgs_last_error()
    assert L.sgs_gat_alpha_heads_fwd_multi(None, None, 0, None, None, 0, 8, 3, 0, None, None, None, 0.2, None, None, None) == 0      # N = 0
