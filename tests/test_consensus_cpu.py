"""CPU: the host side of the sparsifier export.  The new C-ABI symbols are declared and exported; the host-only functions follow their
documented rules; argument validation comes through the error channel without a GPU; the ops wrappers and sparsify refuse CPU tensors
and bad arguments; tests/consensus_ref.py has the properties the issue states of the selection, and its case tables expose each of the
planted faults (consensus_ref.FAULTS)."""
import argparse
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consensus_ref as R  # noqa: E402

NEW = ("sgs_consensus_accum", "sgs_consensus_select_workspace_bytes", "sgs_consensus_select", "sgs_edge_class_counts",
       "sgs_edge_class_variant", "sgs_edge_class_variant_set")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def test_new_symbols_declared_and_exported(pkg):
    protos = pkg._lib.parse_header()
    L = pkg._lib.lib()
    for name in NEW:
        assert name in protos, name
        assert hasattr(L, name), name
    assert protos["sgs_consensus_accum"][2] == ["mask", "mask_stride", "Dc", "E", "first", "count", "hist", "stream"]
    assert protos["sgs_consensus_select"][2] == ["count", "p", "E", "q", "edge_index", "mask", "eid", "edge_index_out", "count_out", "p_out",
                                                 "keys_out", "ws", "ws_bytes", "stream"]
    assert protos["sgs_edge_class_counts"][2] == ["edge_index", "n", "mask", "y", "N", "C", "pairs", "stream"]
    assert L.sgs_abi_version() == 1
    assert callable(pkg.sparsify) and callable(pkg.count_edges_with_different_labels)
    for name in ("consensus_accum", "consensus_select", "edge_class_counts", "edge_class_variant", "edge_class_variant_set"):
        assert callable(getattr(pkg.ops, name)), name


def test_host_only_functions(pkg):
    L = pkg._lib.lib()
    prev = -1
    for E in (-5, 0, 1, 2047, 2048, 2049, 70003, 1 << 21, (1 << 21) + 1, 1 << 26):
        b = L.sgs_consensus_select_workspace_bytes(E)
        assert b >= prev and b >= 12 * max(E, 0)                 # keys 4 E + edge ids 8 E
        assert b >= L.sgs_sample_topq_workspace_bytes(E)
        prev = b
    try:
        for n in (1, 4096, (1 << 31) - 1, 1 << 31, 1 << 33):
            for C in (1, 2, 41, 127, 128, 129, 1000):
                want = 2 if (C <= 128 and n < (1 << 31)) else 1
                assert L.sgs_edge_class_variant(n, C) == want, (n, C)
                L.sgs_edge_class_variant_set(1)
                assert L.sgs_edge_class_variant(n, C) == 1
                L.sgs_edge_class_variant_set(2)
                assert L.sgs_edge_class_variant(n, C) == (2 if want == 2 else -1)
                L.sgs_edge_class_variant_set(0)
        assert L.sgs_edge_class_variant(0, 5) == 0
        assert L.sgs_edge_class_variant(-1, 5) == -1 and L.sgs_edge_class_variant(5, 0) == -1
        assert L.sgs_edge_class_variant_set(3) == -1 and b"sgs_edge_class_variant_set" in L.sgs_last_error()
        assert L.sgs_edge_class_variant(10, 5) == 2                   # a refused code leaves the setting alone
    finally:
        L.sgs_edge_class_variant_set(0)


def test_argument_validation_through_error_channel(pkg):
    L = pkg._lib.lib()
    rc = L.sgs_consensus_select(None, None, 10, 11, None, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"without replacement" in L.sgs_last_error() and b"sgs_consensus_select" in L.sgs_last_error()
    rc = L.sgs_consensus_accum(None, 10, 128, 10, 1, None, None, None)
    assert rc == -1 and b"Dc=128" in L.sgs_last_error()
    assert L.sgs_consensus_accum(None, 0, 0, 0, 1, None, None, None) == 0       # E = 0: nothing to do
    assert L.sgs_consensus_accum(None, 0, 5, 0, 1, None, None, None) == 0
    assert L.sgs_consensus_select(None, None, 0, 0, None, None, None, None, None, None, None, None, 0, None) == 0
    rc = L.sgs_edge_class_counts(None, 10, None, None, 5, 0, None, None)
    assert rc == -1 and b"sgs_edge_class_counts" in L.sgs_last_error()
    assert L.sgs_edge_class_counts(None, 0, None, None, 5, 3, None, None) == 0  # n = 0: nothing launched
    try:
        L.sgs_edge_class_variant_set(2)
        rc = L.sgs_edge_class_counts(None, 10, None, None, 5, 129, None, None)
        assert rc == -1 and b"privatised" in L.sgs_last_error()
    finally:
        L.sgs_edge_class_variant_set(0)


def test_wrappers_refuse_cpu_tensors(pkg):
    ops = pkg.ops
    E = 20
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.consensus_accum(torch.ones(3, E, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.consensus_select(torch.zeros(E, dtype=torch.int32), torch.rand(E), 5, torch.zeros(2, E, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edge_class_counts(torch.zeros(2, E, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.count_edges_with_different_labels(pkg.Batch(edge_index=torch.zeros(2, E, dtype=torch.int64), y=torch.zeros(4, dtype=torch.int64)),
                                              torch.zeros(2, 3, dtype=torch.int64))


def test_sparsify_refuses_bad_arguments_and_cpu(pkg):
    b = pkg.synthetic_graph(40, 200, 6, 3, 1)
    model = pkg.GNNModel(6, 8, 3, 0.3, "GCN")
    args = argparse.Namespace(num_samples_eval=128, degree_bias_coef=0.3)

    class Untouched:                                  # bad arguments are refused before the loader is read
        def __iter__(self):
            raise AssertionError("the loader was read")

    with pytest.raises(ValueError, match="n_draws"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50)                     # args.num_samples_eval = 128
    with pytest.raises(ValueError, match="n_draws"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50, n_draws=0)
    with pytest.raises(ValueError, match="mode"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50, n_draws=3, mode="random")
    with pytest.raises(ValueError, match="mode"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50, n_draws=3, mode="full")
    with pytest.raises(ValueError, match="min_freq"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50, n_draws=3, rule="threshold", min_freq=0)
    with pytest.raises(ValueError, match="min_freq"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50, n_draws=3, rule="threshold", min_freq=1.5)
    with pytest.raises(ValueError, match="min_freq"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50, n_draws=3, rule="threshold")
    with pytest.raises(ValueError, match="rule"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50, n_draws=3, rule="majority")
    args.sgs_cover_nodes = "yes"
    with pytest.raises(ValueError, match="sgs_cover_nodes"):
        pkg.sparsify(args, model, Untouched(), "cpu", q=50, n_draws=3)
    args.sgs_cover_nodes = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.sparsify(args, model, [b], "cpu", q=50, n_draws=3)
    mod = importlib.import_module("sgs_gnn_amd.sparsify")
    assert mod.threshold_count(0.5, 11) == 6 and mod.threshold_count(1.0, 11) == 11 and mod.threshold_count(0.3, 10) == 3
    assert mod.threshold_count(1e-6, 11) == 1
    assert mod.EVAL_BATCH_BUDGET == importlib.import_module("sgs_gnn_amd.eval_batch").EVAL_BATCH_BUDGET


# ------------------------------------------------------------------ the reference's own properties
def test_one_draw_selects_exactly_the_draw():
    g = np.random.default_rng(5)
    for E in (1, 17, 4097):
        for q in R.select_qs(E):
            draw = np.zeros(E, dtype=np.uint8)
            draw[g.permutation(E)[:q]] = 255
            count, _ = R.accum_ref(draw[None, :])
            _, p = R.make_counts_scores(E, 1, E + q)
            r = R.select_ref(count, p, q)
            assert np.array_equal(r["mask"], (draw != 0).astype(np.uint8)), (E, q)
            assert np.array_equal(r["eid"], np.flatnonzero(draw))


def test_threshold_rule_is_topq_at_the_histogram_size():
    for E, D in ((17, 3), (4097, 11), (70003, 127)):
        _, rows = R.make_masks(E, D, 3, E + D)
        count, hist = R.accum_ref(rows, hist=np.zeros(128, dtype=np.int64))
        assert int(hist.sum()) == E and np.array_equal(hist, np.bincount(count, minlength=128))
        _, p = R.make_counts_scores(E, D, 7 * E)
        for need in (1, (D + 1) // 2, D):
            size = int(hist[need:].sum())
            r = R.select_ref(count, p, size)
            assert np.array_equal(r["mask"], (count >= need).astype(np.uint8)), (E, D, need)


def test_scores_below_bit_6_tie_to_the_lower_id():
    a = np.float32(0.3)
    hi = (a.view(np.uint32) | np.uint32(63)).view(np.float32)       # the same key, a larger score
    lo = (a.view(np.uint32) & ~np.uint32(63)).view(np.float32)
    assert hi > lo
    count = np.full(4, 5, dtype=np.int32)
    p = np.array([lo, hi, hi, lo], dtype=np.float32)
    keys = R.keys_ref(count, p)
    assert len(set(keys.tolist())) == 1
    assert R.select_ref(count, p, 2)["eid"].tolist() == [0, 1]
    nxt = (a.view(np.uint32) + np.uint32(64)).view(np.float32)      # one step above bit 6: a larger key
    p2 = np.array([lo, hi, nxt, lo], dtype=np.float32)
    assert R.select_ref(count, p2, 1)["eid"].tolist() == [2]
    bad = np.array([np.nan, -1.0, -0.0, 0.0], dtype=np.float32)     # NaN, negative and -0 score as 0
    assert len(set(R.keys_ref(count, bad).tolist())) == 1
    assert R.keys_ref(np.array([-3, 200], dtype=np.int32), None).tolist() == [0, 127 << 25]      # counts are clamped


# ------------------------------------------------------------------ planted faults
def _select_outputs(fault):
    out = []
    for E in R.SELECT_E:
        for D in (1, 11):
            count, p = R.make_counts_scores(E, D, 1000 * D + E)
            for q in R.select_qs(E):
                r = R.select_ref(count, p, q, fault=fault)
                out.append((r["keys"], r["mask"], r["eid"], r["count"]))
    return out


def _same(a, b):
    return all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_planted_faults_are_caught_by_the_case_tables():
    good = _select_outputs(None)
    assert _same(good, _select_outputs(None))
    assert not _same(good, _select_outputs("tie_high"))
    assert not _same(good, _select_outputs("shift5"))
    # the tie fault must show in the SELECTION, not only in the keys
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(good, _select_outputs("tie_high")))
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(good, _select_outputs("shift5")))
    hit = False
    for E in R.ACCUM_E:
        for Dc in R.ACCUM_DC:
            _, rows = R.make_masks(E, Dc, 3, E + Dc)
            hit |= not np.array_equal(R.accum_ref(rows)[0], R.accum_ref(rows, fault="byte_as_count")[0])
    assert hit
    hit = False
    for C in R.PAIR_PRIVATE_C + R.PAIR_DIRECT_C:
        for n in R.PAIR_N_EDGES:
            ei, y, mask = R.make_pairs_case(n, 300, C, n + C, True)
            a, b = R.edge_class_ref(ei, y, 300, C, mask), R.edge_class_ref(ei, y, 300, C, mask, fault="count_skipped")
            hit |= not np.array_equal(a, b)
            assert int(a.sum()) <= n
    assert hit
