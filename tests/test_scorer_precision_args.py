"""CPU: the scorer precision switch (args.sgs_precision, sgs_gnn_amd.scorer_precision) validates its value before any work."""
import argparse

import pytest


class _Untouchable:
    """A partition stream that fails the test if anything reads it."""

    def __iter__(self):
        raise AssertionError("a partition was read before the precision was checked")

    batches = property(lambda self: iter(self))


def test_check_precision_values():
    import sgs_gnn_amd as S
    assert S.ops.check_precision(None) == "fp32"
    assert S.ops.check_precision("fp32") == "fp32" and S.ops.check_precision("bf16") == "bf16"
    for bad in ("fp16", "BF16", "", 16, True):
        with pytest.raises(ValueError):
            S.ops.check_precision(bad)


def test_context_manager_restores_and_rejects():
    import sgs_gnn_amd as S
    assert S.ops.get_scorer_precision() == "fp32"
    with S.scorer_precision("bf16"):
        assert S.ops.get_scorer_precision() == "bf16"
        with S.scorer_precision("fp32"):
            assert S.ops.get_scorer_precision() == "fp32"
        assert S.ops.get_scorer_precision() == "bf16"
    assert S.ops.get_scorer_precision() == "fp32"
    with pytest.raises(ValueError):
        S.scorer_precision("half")
    assert set(S.ops.PRECISION_COUNTS) == {"fwd_fp32", "fwd_bf16", "bwd_fp32", "bwd_bf16"}


@pytest.mark.parametrize("entry", ["train", "prepare_step_graphs", "evaluate", "ensemble_evaluate"])
def test_invalid_sgs_precision_raises_before_reading_partitions(entry):
    import sgs_gnn_amd as S
    a = argparse.Namespace(device="cpu", mode="learned", pipeline="hybrid", sgs_precision="fp16", num_samples_eval=2)
    with pytest.raises(ValueError):
        if entry == "train":
            S.train(a, 0, 1, None, None, None, None, None, _Untouchable(), q=10)
        elif entry == "prepare_step_graphs":
            S.prepare_step_graphs(a, None, None, None, None, _Untouchable(), q=10)
        elif entry == "evaluate":
            S.evaluate(a, None, _Untouchable(), "cpu", q=10)
        else:
            S.ensemble_evaluate(a, None, _Untouchable(), "cpu", q=10)
    assert S.ops.get_scorer_precision() == "fp32"
