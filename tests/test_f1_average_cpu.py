"""CPU: the host side of the per-class evaluation metrics.  utils.f1_from_confusion / classification_report against tests/f1_ref.py (a
numpy restatement from label and prediction arrays, written independently of them), planted and seeded random cases, at 1e-12 absolute (the
bound tests/test_gpu_evaluate.py uses for these fractions; the two computations differ by rounding in a handful of float64 operations);
the same cases against sklearn where it is installed; sgs_confusion_variant's documented rule at its thresholds; validation of
args.sgs_f1_average / args.sgs_eval_report before the loader is touched; the new prototypes in the header."""
import argparse
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f1_ref as R  # noqa: E402

TOL = 1e-12
PRIV_MAX_C = 73            # 12 C^2 <= 65536 bytes of LDS (include/sgs_hip.h)
AUTO_MIN_ROWS = 4096       # the automatic rule (include/sgs_hip.h): privatised iff C <= 12 and 4096 <= N < 2^31
AUTO_MAX_C = 12


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _planted():
    """(name, y, pred, C)"""
    return [
        ("class absent from truth and prediction", [0, 0, 2, 2, 0], [0, 2, 2, 0, 0], 4),
        ("class only predicted", [0, 0, 1, 1, 0], [0, 2, 1, 1, 2], 3),
        ("class only in the truth", [0, 2, 1, 1, 2], [0, 0, 1, 1, 1], 3),
        ("one row, right", [1], [1], 3),
        ("one row, wrong", [1], [2], 3),
        ("empty split", [], [], 3),
        ("C = 1", [0, 0, 0], [0, 0, 0], 1),
        ("perfect", [0, 1, 2, 3, 3, 1], [0, 1, 2, 3, 3, 1], 4),
        ("all wrong", [0, 1, 2], [1, 2, 0], 3),
    ]


def _random_cases(n_cases=400, seed=20):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_cases):
        C = int(rng.integers(1, 9))
        n = int(rng.integers(0, 41)) if k % 7 else int(rng.integers(0, 3))
        ty = rng.permutation(C)[: int(rng.integers(1, C + 1))]          # truth and prediction draw from their own class subsets
        tp = rng.permutation(C)[: int(rng.integers(1, C + 1))]
        y = rng.choice(ty, size=n)
        pred = np.where(rng.random(n) < 0.5, y, rng.choice(tp, size=n))
        out.append((f"random {k}", y.tolist(), pred.tolist(), C))
    return out


CASES = _planted() + _random_cases()


def _check_report(got, want, name):
    for key in ("precision", "recall", "f1"):
        assert got[key] == pytest.approx(want[key], abs=TOL), (name, key)
    assert list(got["support"]) == list(want["support"]), name
    for key in ("micro", "macro", "weighted", "balanced_accuracy"):
        assert got[key] == pytest.approx(want[key], abs=TOL), (name, key)


def test_f1_from_confusion_and_report_match_the_array_reference(pkg):
    U = pkg.utils
    assert pkg.f1_from_confusion is U.f1_from_confusion and pkg.classification_report is U.classification_report
    kinds = set()
    for name, y, pred, C in CASES:
        M = R.confusion(y, pred, C)
        assert int(M.sum()) == len(y)
        for avg in R.AVERAGES:
            want = R.f1(y, pred, avg)
            assert U.f1_from_confusion(M, avg) == pytest.approx(want, abs=TOL), (name, avg)
            assert U.f1_from_confusion(torch.from_numpy(M), avg) == pytest.approx(want, abs=TOL), (name, avg)
            assert U.f1_from_confusion(M.tolist(), avg) == pytest.approx(want, abs=TOL), (name, avg)
        _check_report(U.classification_report(M), R.report(y, pred, C), name)
        sup, prd = M.sum(1), M.sum(0)
        kinds |= {"absent"} if ((sup + prd) == 0).any() else set()
        kinds |= {"predicted only"} if ((sup == 0) & (prd > 0)).any() else set()
        kinds |= {"truth only"} if ((sup > 0) & (prd == 0)).any() else set()
        kinds |= {"empty"} if len(y) == 0 else set()
        kinds |= {"one row"} if len(y) == 1 else set()
    assert kinds == {"absent", "predicted only", "truth only", "empty", "one row"}       # the cases reach every corner they are meant to


def test_stacked_matrices_and_the_stated_values(pkg):
    U = pkg.utils
    (_, y0, p0, _), (_, y1, p1, _) = CASES[1], CASES[2]
    M3 = np.stack([R.confusion(y0, p0, 3), R.confusion(y1, p1, 3), np.zeros((3, 3), dtype=np.int64)])
    for avg in R.AVERAGES:
        got = U.f1_from_confusion(torch.from_numpy(M3), avg)
        assert isinstance(got, tuple) and len(got) == 3 and got[2] == 0
        assert got == pytest.approx((R.f1(y0, p0, avg), R.f1(y1, p1, avg), 0.0), abs=TOL)
    rep = U.classification_report(M3)
    assert isinstance(rep, list) and len(rep) == 3
    _check_report(rep[0], R.report(y0, p0, 3), "split 0")
    _check_report(rep[2], R.report([], [], 3), "empty split")
    # by hand: truth [0, 0, 1], prediction [0, 1, 1]: f_0 = 2 / 3, f_1 = 2 / 3; with class 2 absent macro = 2 / 3, not 4 / 9
    M = [[1, 1, 0], [0, 1, 0], [0, 0, 0]]
    assert U.f1_from_confusion(M, "macro") == pytest.approx(2 / 3, abs=TOL)
    assert U.f1_from_confusion(M, "micro") == pytest.approx(2 / 3, abs=TOL)
    assert U.f1_from_confusion(M, "weighted") == pytest.approx(2 / 3, abs=TOL)
    # truth [0, 0, 0, 1], prediction [0, 0, 0, 0]: f_0 = 6 / 7, f_1 = 0
    M = [[3, 0], [1, 0]]
    assert U.f1_from_confusion(M, "macro") == pytest.approx(3 / 7, abs=TOL)
    assert U.f1_from_confusion(M, "weighted") == pytest.approx(18 / 28, abs=TOL)
    assert U.classification_report(M)["balanced_accuracy"] == pytest.approx(0.5, abs=TOL)
    with pytest.raises(ValueError, match="micro"):
        U.f1_from_confusion(M, "samples")
    with pytest.raises(ValueError, match="micro"):
        U.calculate_f1(torch.zeros(2, 2), torch.zeros(2, dtype=torch.long), torch.ones(2, dtype=torch.bool), average="binary")


def test_against_sklearn(pkg):
    sk = pytest.importorskip("sklearn.metrics")
    U = pkg.utils
    warnings.simplefilter("ignore")          # sklearn warns about absent classes, which the cases plant on purpose (reset per test by pytest)
    for name, y, pred, C in CASES:
        if not y:
            continue
        M = R.confusion(y, pred, C)
        for avg in R.AVERAGES:
            assert U.f1_from_confusion(M, avg) == pytest.approx(sk.f1_score(y, pred, average=avg, zero_division=0), abs=TOL), (name, avg)
        p, r, f, s = sk.precision_recall_fscore_support(y, pred, labels=list(range(C)), zero_division=0)
        rep = U.classification_report(M)
        assert rep["precision"] == pytest.approx(p.tolist(), abs=TOL) and rep["recall"] == pytest.approx(r.tolist(), abs=TOL), name
        assert rep["f1"] == pytest.approx(f.tolist(), abs=TOL) and rep["support"] == s.tolist(), name
        assert rep["balanced_accuracy"] == pytest.approx(sk.balanced_accuracy_score(y, pred), abs=TOL), name


def test_confusion_variant_rule_on_cpu(pkg):
    """sgs_confusion_variant is a pure host function: the documented rule at its thresholds."""
    L = pkg._lib.lib()
    ops = pkg.ops
    try:
        assert L.sgs_confusion_variant_set(0) == 0
        big = AUTO_MIN_ROWS
        for C in (1, 5, AUTO_MAX_C):
            assert L.sgs_confusion_variant(big, C) == 2 and L.sgs_confusion_variant(big - 1, C) == 1, C
            assert L.sgs_confusion_variant(1, C) == 1 and L.sgs_confusion_variant(232965, C) == 2, C
            assert L.sgs_confusion_variant((1 << 31) - 1, C) == 2 and L.sgs_confusion_variant(1 << 31, C) == 1, C
        for C in (AUTO_MAX_C + 1, 41, 70, PRIV_MAX_C, PRIV_MAX_C + 1, 130, 1000):
            assert L.sgs_confusion_variant(big, C) == 1 and L.sgs_confusion_variant(1 << 20, C) == 1, C
        assert 12 * PRIV_MAX_C ** 2 <= 65536 < 12 * (PRIV_MAX_C + 1) ** 2
        assert L.sgs_confusion_variant(0, 5) == 0
        assert L.sgs_confusion_variant(-1, 5) == -1 and L.sgs_confusion_variant(10, 0) == -1
        assert [ops.confusion_variant(1013, 41), ops.confusion_variant(33869, 5), ops.confusion_variant(19793, 70),
                ops.confusion_variant(232965, 41)] == [1, 2, 1, 1]                      # bench S3, S4, S2, S5
        # code 1 is always accepted (the forced-form GPU cases cannot become vacuous); code 2 is refused beyond the LDS limit
        assert L.sgs_confusion_variant_set(1) == 0
        assert all(L.sgs_confusion_variant(N, C) == 1 for N in (1, big, 1 << 31) for C in (1, PRIV_MAX_C, PRIV_MAX_C + 1, 1000))
        assert L.sgs_confusion_variant_set(2) == 0
        assert L.sgs_confusion_variant(1, PRIV_MAX_C) == 2 and L.sgs_confusion_variant(1, PRIV_MAX_C + 1) == -1
        assert L.sgs_confusion_variant(1 << 31, 5) == -1
        # unknown codes are rejected through the error channel and leave the setting alone
        for bad in (-1, 3, 7):
            assert L.sgs_confusion_variant_set(bad) == -1 and b"sgs_confusion_variant_set" in L.sgs_last_error(), bad
            assert L.sgs_confusion_variant(1, PRIV_MAX_C) == 2
        with pytest.raises(RuntimeError, match="sgs_confusion_variant_set"):
            ops.confusion_variant_set(3)
        ops.confusion_variant_set(0)
        assert ops.confusion_variant(1, 5) == 1
        # argument validation of the call itself needs no GPU either: it reports before anything is launched
        assert L.sgs_confusion_counts(None, 4, 0, None, None, None, None, None, None) == -1 and b"sgs_confusion_counts" in L.sgs_last_error()
        assert L.sgs_confusion_counts(None, 4, 3, None, None, None, None, None, None) == -1
    finally:
        L.sgs_confusion_variant_set(0)


class _Untouchable:
    """A loader that must not be read."""

    def __iter__(self):
        raise AssertionError("the loader was read")


@pytest.mark.parametrize("attr,bad", [("sgs_f1_average", "binary"), ("sgs_f1_average", "Macro"), ("sgs_f1_average", 1), ("sgs_f1_average", True),
                                      ("sgs_eval_report", True), ("sgs_eval_report", "yes"), ("sgs_eval_report", [])])
def test_bad_flag_values_raise_before_the_loader_is_read(pkg, attr, bad):
    model = torch.nn.Identity()
    for fn, extra in ((pkg.evaluate, {}), (pkg.ensemble_evaluate, {}), (pkg.ensemble_evaluate, {"sgs_eval_batch": True})):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, **extra, **{attr: bad})
        with pytest.raises(ValueError, match=attr) as e:
            fn(args, model, _Untouchable(), "cpu", q=10, mode="learned")
        if attr == "sgs_f1_average":
            assert all(name in str(e.value) for name in ("micro", "macro", "weighted"))


def test_good_flag_values_reach_the_loader(pkg):
    model = torch.nn.Identity()
    for avg in (None, "micro", "macro", "weighted"):
        for rep in (None, {}):
            args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, sgs_f1_average=avg, sgs_eval_report=rep)
            with pytest.raises(AssertionError, match="the loader was read"):
                pkg.evaluate(args, model, _Untouchable(), "cpu", q=10, mode="learned")
    # an empty loader: zeros as ever, None in both report entries
    rep = {"confusion": 1}
    args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, sgs_f1_average="macro", sgs_eval_report=rep)
    assert pkg.evaluate(args, model, [], "cpu", q=10, mode="learned") == (0, 0, 0)
    assert rep == {"confusion": None, "report": None}
    assert pkg.ensemble_evaluate(args, model, [], "cpu", q=10, mode="learned") == (0, 0, 0)


def test_new_prototypes_are_parsed_from_the_header(pkg):
    import ctypes
    protos = pkg._lib.parse_header()
    assert protos["sgs_confusion_counts"][2] == ["logits", "N", "C", "y", "m0", "m1", "m2", "conf", "stream"]
    assert protos["sgs_confusion_counts"][1][1:3] == [ctypes.c_int64, ctypes.c_int64]
    assert protos["sgs_confusion_variant"][1] == [ctypes.c_int64, ctypes.c_int64] and protos["sgs_confusion_variant"][0] is ctypes.c_int
    assert protos["sgs_confusion_variant_set"][1] == [ctypes.c_int]
    L = pkg._lib.lib()
    assert L.sgs_abi_version() == 1
    for name in ("sgs_confusion_counts", "sgs_confusion_variant", "sgs_confusion_variant_set"):
        assert getattr(L, name).argtypes == protos[name][1]
    assert all(hasattr(pkg.ops, n) for n in ("confusion_counts", "confusion_variant", "confusion_variant_set"))
