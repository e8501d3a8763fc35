"""CPU: the host side of the ROC-AUC evaluation metric.  tests/auc_ref.py's sort-and-search two_u against the O(n^2) pair count (random,
tie-heavy, signed zeros, infinities, denormals, NaN), and against sklearn where it is installed; the numpy key packing's order image
against the float order; utils.auc_from_counts on hand-made counts; the new prototypes, the two host-only queries and argument validation
through the error channel; validation of args.sgs_eval_auc / args.sgs_eval_auc_report before the loader is touched."""
import argparse
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _cases():
    rng = np.random.default_rng(29)
    out = []
    for k in range(60):
        n = int(rng.integers(0, 40))
        kind = k % 4
        if kind == 0:
            x = rng.standard_normal(n)
        elif kind == 1:
            x = rng.integers(-2, 3, n).astype(np.float64)                        # ties everywhere
        elif kind == 2:
            x = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, np.nan, 1.5, -1.5]), n)
        else:
            x = np.zeros(n)                                                      # one run
        pos = rng.random(n) < (0.5 if k % 3 else 0.1)
        mask = rng.random(n) < 0.8
        out.append((x.astype(np.float32), pos, mask))
    return out


def test_two_u_matches_the_pair_count():
    seen_nan = False
    for x, pos, mask in _cases():
        got, want = R.two_u(x, pos, mask), R.brute(x, pos, mask)
        assert got == want and all(isinstance(v, int) for v in got)
        assert 0 <= got[0] <= 2 * got[1] * got[2]
        seen_nan |= bool(np.isnan(x[mask]).any())
    assert seen_nan
    # by hand: positives {1, 2}, negatives {1, 0}: pairs (1,1) tie, (1,0) win, (2,1) win, (2,0) win -> twoU = 1 + 2 + 2 + 2
    assert R.two_u([1, 2, 1, 0], [1, 1, 0, 0], [1, 1, 1, 1]) == (7, 2, 2)
    assert R.two_u([0.0, -0.0], [1, 0], [1, 1]) == (1, 1, 1)                     # signed zeros tie
    assert R.two_u([np.nan, 1.0, 0.0], [1, 1, 0], [1, 1, 1]) == (2, 1, 1)        # a NaN item is dropped
    assert R.two_u([1.0, 0.0], [1, 0], [0, 0]) == (0, 0, 0)


def test_order_image_is_the_float_order():
    v = np.array([-np.inf, -3.0, -1e-39, -1e-45, -0.0, 0.0, 1e-45, 1e-39, 2.5, np.inf], dtype=np.float32)
    img = R.order_image(v).astype(np.int64)
    assert img[4] == img[5] == 0x80000000
    d = np.diff(img)
    assert (d[:4] > 0).all() and d[4] == 0 and (d[5:] > 0).all()
    x = np.random.default_rng(1).standard_normal(2000).astype(np.float32)
    assert np.array_equal(np.argsort(R.order_image(x), kind="stable"), np.argsort(x, kind="stable"))


def test_pack_keys_fields():
    sc = np.array([[0.5, -0.5, np.nan], [1.0, 2.0, 3.0], [0.0, -0.0, 1.0], [7.0, 7.0, 7.0]], dtype=np.float32)
    y = np.array([2, 0, 3, -1])
    masks = [np.array([1, 1, 1, 1]), np.array([0, 2, 0, 0]), np.array([0, 0, 1, 1])]
    k = R.pack_keys(sc, y, masks, 3).reshape(4, 3)
    assert [int(v) & 7 for v in k[0]] == [1, 1, 0]                               # the NaN item is in no split
    assert [int(v) & 7 for v in k[1]] == [3, 3, 3]                               # a mask byte of 2 counts as set
    assert [int(v) & 7 for v in k[2]] == [0, 0, 0] and [int(v) & 7 for v in k[3]] == [0, 0, 0]        # labels 3 and -1 are outside [0, 3)
    assert [(int(v) >> 3) & 1 for v in k[0]] == [0, 0, 1] and [(int(v) >> 3) & 1 for v in k[1]] == [1, 0, 0]
    assert [int(v) >> 36 for v in k[1]] == [0, 1, 2]
    assert (int(k[2, 0]) >> 4) & 0xFFFFFFFF == (int(k[2, 1]) >> 4) & 0xFFFFFFFF == 0x80000000
    kb = R.pack_keys(sc[:, :1], np.array([1, 0, 1, 2]), masks, 2)
    assert [(int(v) >> 3) & 1 for v in kb] == [1, 0, 1, 0] and [int(v) & 7 for v in kb] == [1, 3, 5, 0]


def test_counts_from_keys_equal_counts_from_scores():
    rng = np.random.default_rng(5)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, np.nan, 1.5, -1.5, 2.0], dtype=np.float32)
    for S, C in ((1, 2), (3, 3), (6, 6)):
        for M in (0, 1, 50):
            x = rng.choice(vals, (M, S))
            y = rng.integers(-1, C + 1, M)
            masks = [rng.integers(0, 3, M).astype(np.uint8) for _ in range(3)]
            want = R.counts(x, y, masks, C)
            assert want.shape == (3, S, 3) and np.array_equal(R.counts_of_keys(R.pack_keys(x, y, masks, C), S), want)
            for s in range(3):
                for c in range(S):
                    ok = (masks[s] != 0) & (y >= 0) & (y < C)
                    assert tuple(want[s, c]) == R.brute(x[:, c], y == (1 if S == 1 else c), ok)


def test_against_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    for x, pos, mask in _cases():
        keep = mask & ~np.isnan(x)
        u, p, n = R.two_u(x, pos, mask)
        if p * n == 0:
            continue
        xs = np.clip(x[keep].astype(np.float64), -1e300, 1e300)                  # sklearn refuses infinities; the order is kept
        assert u / (2 * p * n) == pytest.approx(sk.roc_auc_score(pos[keep], xs), abs=1e-12)


def test_auc_from_counts(pkg):
    U = pkg.utils
    assert pkg.auc_from_counts is U.auc_from_counts and pkg.calculate_auc is U.calculate_auc
    cnt = [[[7, 2, 2], [0, 0, 5], [3, 1, 3]],            # defined, undefined (no positive), defined
           [[0, 3, 0], [0, 0, 0], [0, 0, 4]],            # all undefined
           [[12, 2, 3], [9, 3, 3], [0, 1, 1]]]
    for c in (cnt, torch.tensor(cnt), np.array(cnt)):
        tri, per = U.auc_from_counts(c)
        assert tri == pytest.approx(((7 / 8 + 3 / 6) / 2, 0.0, (1.0 + 0.5 + 0.0) / 3), abs=1e-15)
        assert per[0][0] == 7 / 8 and math.isnan(per[0][1]) and per[0][2] == 0.5
        assert all(math.isnan(v) for v in per[1]) and tri[1] == 0.0
        assert (tri, [[v == v for v in r] for r in per]) == (R.auc(c)[0], [[v == v for v in r] for r in R.auc(c)[1]])
    big = [[[2 * (3 << 40) * (5 << 20) - 1, 3 << 40, 5 << 20]]] * 3                 # exact integers beyond 2^53 before the division
    assert U.auc_from_counts(big)[0][0] == pytest.approx(1.0, abs=1e-15)
    with pytest.raises(ValueError, match="auc_from_counts"):
        U.auc_from_counts([[[1, 2, 3]]])


def test_prototypes_and_host_only_queries(pkg):
    protos = pkg._lib.parse_header()
    assert protos["sgs_auc_block_items"] == (ctypes.c_int64, [], [])
    assert protos["sgs_auc_pack"][2] == ["scores", "N", "S", "C", "y", "m0", "m1", "m2", "keys", "stream"]
    assert protos["sgs_auc_counts_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64], ["n", "S"])
    assert protos["sgs_auc_counts"][2] == ["keys", "n", "S", "out", "ws", "ws_bytes", "stream"]
    L = pkg._lib.lib()
    T = L.sgs_auc_block_items()
    assert T == pkg.ops.auc_block_items() and T >= 64 and T % 64 == 0
    assert L.sgs_auc_counts_workspace_bytes(0, 1) > 0
    for n, S in ((1, 1), (T, 3), (3 * T + 5, 41), (230 * 1013 * 41, 41)):
        assert L.sgs_auc_counts_workspace_bytes(n, S) >= 8 * n + 12 * (n // T + 1)        # the sorted keys and the per-tile counts
    assert all(hasattr(pkg.ops, n) for n in ("auc_scores", "auc_pack", "auc_counts"))


def test_argument_validation_reports_through_the_error_channel(pkg):
    L = pkg._lib.lib()
    for N, S, C in ((4, 1, 1), (4, 3, 2), (4, 2, 3), (4, 1, 3), (-1, 1, 2), (4, 65537, 65537), (1 << 30, 5, 5)):
        assert L.sgs_auc_pack(None, N, S, C, None, None, None, None, None, None) == -1 and b"sgs_auc_pack" in L.sgs_last_error(), (N, S, C)
    assert L.sgs_auc_pack(None, 4, 1, 2, None, None, None, None, None, None) == -1 and b"null pointer" in L.sgs_last_error()
    assert L.sgs_auc_pack(None, 0, 3, 3, None, None, None, None, None, None) == 0                     # nothing to do
    assert L.sgs_auc_counts(None, 1 << 31, 1, None, None, 0, None) == -1 and b"2^31" in L.sgs_last_error()
    assert L.sgs_auc_counts(None, -1, 1, None, None, 0, None) == -1
    assert L.sgs_auc_counts(None, 5, 0, None, None, 0, None) == -1 and b"sgs_auc_counts" in L.sgs_last_error()
    assert L.sgs_auc_counts(None, 5, 65537, None, None, 0, None) == -1
    assert L.sgs_auc_counts(None, 5, 1, None, None, 0, None) == -1 and b"null pointer" in L.sgs_last_error()


def test_no_cpu_fallback(pkg):
    ops = pkg.ops
    m = torch.ones(4, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.auc_scores(torch.randn(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.auc_pack(torch.randn(4, 3), torch.zeros(4, dtype=torch.long), (m, m, m), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.auc_counts(torch.zeros(12, dtype=torch.int64), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.calculate_auc(torch.randn(4, 3), torch.zeros(4, dtype=torch.long), m)


class _Untouchable:
    """A loader that must not be read."""

    def __iter__(self):
        raise AssertionError("the loader was read")


def _each_path(pkg):
    return ((pkg.evaluate, {}), (pkg.ensemble_evaluate, {}), (pkg.ensemble_evaluate, {"sgs_eval_batch": True}))


@pytest.mark.parametrize("attr,bad", [("sgs_eval_auc", "yes"), ("sgs_eval_auc", 1), ("sgs_eval_auc", 0), ("sgs_eval_auc", "macro"), ("sgs_eval_auc", {}),
                                      ("sgs_eval_auc_report", True), ("sgs_eval_auc_report", "yes"), ("sgs_eval_auc_report", [])])
def test_bad_flag_values_raise_before_the_loader_is_read(pkg, attr, bad):
    model = torch.nn.Identity()
    for fn, extra in _each_path(pkg):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, **extra, **{attr: bad})
        with pytest.raises(ValueError, match=attr):
            fn(args, model, _Untouchable(), "cpu", q=10, mode="learned")


@pytest.mark.parametrize("avg", ["macro", "weighted"])
def test_the_flag_conflict_raises_before_the_loader_is_read(pkg, avg):
    model = torch.nn.Identity()
    for fn, extra in _each_path(pkg):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, sgs_eval_auc=True, sgs_f1_average=avg, **extra)
        with pytest.raises(ValueError) as e:
            fn(args, model, _Untouchable(), "cpu", q=10, mode="learned")
        assert "sgs_eval_auc" in str(e.value) and "sgs_f1_average" in str(e.value)


def test_good_flag_values_reach_the_loader_and_empty_loaders(pkg):
    model = torch.nn.Identity()
    for on in (None, False, True):
        for rep in (None, {}):
            for avg in (None, "micro") + (("macro",) if not on else ()):
                args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, sgs_eval_auc=on, sgs_eval_auc_report=rep, sgs_f1_average=avg)
                with pytest.raises(AssertionError, match="the loader was read"):
                    pkg.evaluate(args, model, _Untouchable(), "cpu", q=10, mode="learned")
    keys = {"counts", "per_class", "auc", "kind", "classes_defined"}
    for fn, extra in _each_path(pkg):
        for on in (True, False):
            rep = {"counts": 1}
            args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, sgs_eval_auc=on, sgs_eval_auc_report=rep, **extra)
            assert fn(args, model, [], "cpu", q=10, mode="learned") == (0, 0, 0)
            assert rep == dict.fromkeys(keys)
