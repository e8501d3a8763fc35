"""GPU: evaluate / ensemble_evaluate with args.sgs_f1_average and args.sgs_eval_report, on the serial draw loop and on the batched engine.
The 48-node fixture and its batch are built as in tests/test_gpu_evaluate.py.  The expected confusion matrix is counted on the CPU from
trace["mean"], the device's own mean logits, so it is exact (no float tolerance on the matrix); the expected averages come from
tests/f1_ref.py (from label and prediction arrays) at 1e-12, the bound tests/test_gpu_evaluate.py uses for these fractions.  The untrained
checkpoint predicts one class for nearly every node, so the fixture first centres the last layer's bias on the full-graph mean logits: the
predictions then spread over several classes."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f1_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
DRAWS = 5


@pytest.fixture(scope="module")
def env():
    import sgs_gnn_amd as S
    fx = load_golden("pipeline_hybrid_gcn.pt")
    m = S.GNNModel(fx["x"].shape[1], 16, 5, dropout_prob=0.3, edge_mlp_type="GCN")
    m.load_state_dict(fx["state0"])
    m = m.to(DEV)
    n = fx["x"].shape[0]
    g = torch.Generator().manual_seed(1)
    val = torch.rand(n, generator=g) < 0.5
    b1 = S.Batch(x=fx["x"], edge_index=fx["edge_index"], y=fx["y"], train_mask=fx["train_mask"], val_mask=val & ~fx["train_mask"],
                 test_mask=~val & ~fx["train_mask"], prob=fx["prob"])
    E, q = fx["edge_index"].shape[1], fx["q"]
    noises = [torch.empty(E).exponential_(1, generator=g).to(DEV) for _ in range(2 * DRAWS)]
    # a second partition: other masks, and labels without classes 3 and 4 (a class absent from a partition is what separates the pooled
    # macro average from the size-weighted per-partition one)
    u = torch.rand(n, generator=torch.Generator().manual_seed(2))
    y2 = torch.where(fx["y"] >= 3, torch.zeros_like(fx["y"]), fx["y"])
    b2 = S.Batch(x=fx["x"], edge_index=fx["edge_index"], y=y2, train_mask=u < 0.3, val_mask=(u >= 0.3) & (u < 0.5), test_mask=u >= 0.5,
                 prob=fx["prob"])
    tr = {}
    a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=1, _sgs_trace_eval=tr)
    S.evaluate(a, m, [b1], DEV, q=q, mode="full")
    with torch.no_grad():
        m.gcn2.bias -= tr["mean"].mean(0)
    return dict(S=S, model=m, b1=b1, b2=b2, q=q, noises=noises)


def _args(env, batched, noises=None, **kw):
    a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=DRAWS, **kw)
    a._sgs_noise_eval = list(env["noises"][:DRAWS] if noises is None else noises)
    if batched:
        a.sgs_eval_batch = 2                # 5 draws in passes of 2, 2 and 1: the mean spans several passes
    return a


def _run(env, a, loader, mode):
    S = env["S"]
    EV = sys.modules["sgs_gnn_amd.evaluate"]
    before = dict(EV.PATH_COUNTS)
    got = S.ensemble_evaluate(a, env["model"], loader, DEV, q=env["q"], mode=mode)
    path = "batched" if getattr(a, "sgs_eval_batch", False) else "serial"
    other = "serial" if path == "batched" else "batched"
    assert EV.PATH_COUNTS[path] == before[path] + 1 and EV.PATH_COUNTS[other] == before[other]      # PATH_COUNTS moves as before
    return got


def _masks(b):
    return [b.train_mask.numpy(), b.val_mask.numpy(), b.test_mask.numpy()]


def _expected(mean, b):
    """(confusion [3, C, C], predictions) from a partition's mean logits, on the CPU."""
    pred = torch.argmax(mean.cpu(), dim=1).numpy()
    return R.confusion3(b.y.numpy(), pred, _masks(b), mean.shape[1]), pred


def _ref_triple(b, pred, avg):
    return tuple(R.f1(b.y.numpy()[m], pred[m], avg) for m in _masks(b))


@pytest.mark.parametrize("mode", ["learned", "full"])
@pytest.mark.parametrize("batched", [False, True], ids=["serial", "batched"])
def test_macro_weighted_and_report_on_both_paths(env, batched, mode):
    b = env["b1"]
    tr, rep = {}, {}
    got = _run(env, _args(env, batched, sgs_f1_average="macro", sgs_eval_report=rep, _sgs_trace_eval=tr), [b], mode)
    assert tr["logits"].shape[0] == DRAWS
    conf, pred = _expected(tr["mean"], b)
    assert len(set(pred.tolist())) >= 2                                          # the predictions are not one class
    assert rep["confusion"].dtype == torch.int64 and rep["confusion"].device.type == "cpu"
    assert np.array_equal(rep["confusion"].numpy(), conf)                        # exact
    assert got == pytest.approx(_ref_triple(b, pred, "macro"), abs=TOL)
    for s, m in enumerate(_masks(b)):
        want = R.report(b.y.numpy()[m], pred[m], 5)
        for key in ("precision", "recall", "f1", "micro", "macro", "weighted", "balanced_accuracy"):
            assert rep["report"][s][key] == pytest.approx(want[key], abs=TOL), (s, key)
        assert rep["report"][s]["support"] == want["support"]
    tr2 = {}
    got_w = _run(env, _args(env, batched, sgs_f1_average="weighted", _sgs_trace_eval=tr2), [b], mode)
    assert torch.equal(tr2["mean"], tr["mean"])                                  # the same explicit noise: the same mean logits
    assert got_w == pytest.approx(_ref_triple(b, pred, "weighted"), abs=TOL)
    # "micro" with a report: the triple is today's, bit for bit, and the matrix is the same
    plain = _run(env, _args(env, batched), [b], mode)
    rep_m = {}
    assert _run(env, _args(env, batched, sgs_f1_average="micro", sgs_eval_report=rep_m), [b], mode) == plain
    assert np.array_equal(rep_m["confusion"].numpy(), conf)
    assert plain == pytest.approx(_ref_triple(b, pred, "micro"), abs=TOL)


@pytest.mark.parametrize("batched", [False, True], ids=["serial", "batched"])
def test_two_partitions_are_pooled(env, batched):
    b1, b2, ns = env["b1"], env["b2"], env["noises"]
    parts = []
    for b, nz in ((b1, ns[:DRAWS]), (b2, ns[DRAWS:])):                          # each partition alone, with the noise it gets in the loader
        tr = {}
        _run(env, _args(env, batched, noises=nz, _sgs_trace_eval=tr), [b], "learned")
        parts.append(_expected(tr["mean"], b))
    rep = {}
    got = _run(env, _args(env, batched, noises=ns, sgs_f1_average="macro", sgs_eval_report=rep), [b1, b2], "learned")
    assert np.array_equal(rep["confusion"].numpy(), parts[0][0] + parts[1][0])
    ys = [np.concatenate([b1.y.numpy()[m1], b2.y.numpy()[m2]]) for m1, m2 in zip(_masks(b1), _masks(b2))]
    ps = [np.concatenate([parts[0][1][m1], parts[1][1][m2]]) for m1, m2 in zip(_masks(b1), _masks(b2))]
    pooled = tuple(R.f1(y, p, "macro") for y, p in zip(ys, ps))
    assert got == pytest.approx(pooled, abs=TOL)
    for s, (m1, m2) in enumerate(zip(_masks(b1), _masks(b2))):                   # the pooling is really exercised
        sw = (R.f1(b1.y.numpy()[m1], parts[0][1][m1], "macro") * m1.sum() + R.f1(b2.y.numpy()[m2], parts[1][1][m2], "macro") * m2.sum()) \
            / (m1.sum() + m2.sum())
        assert abs(sw - pooled[s]) > 1e-6, (s, sw, pooled[s])
    got_w = _run(env, _args(env, batched, noises=ns, sgs_f1_average="weighted"), [b1, b2], "learned")
    assert got_w == pytest.approx(tuple(R.f1(y, p, "weighted") for y, p in zip(ys, ps)), abs=TOL)
    got_m = _run(env, _args(env, batched, noises=ns), [b1, b2], "learned")
    assert got_m == pytest.approx(tuple(R.f1(y, p, "micro") for y, p in zip(ys, ps)), abs=TOL)


@pytest.mark.parametrize("batched", [False, True], ids=["serial", "batched"])
def test_flags_unset_or_micro_launch_nothing_new(env, batched, monkeypatch):
    S = env["S"]
    calls = []
    real = S.ops.confusion_counts
    monkeypatch.setattr(S.ops, "confusion_counts", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    loader = [env["b1"], env["b2"]]
    plain = _run(env, _args(env, batched, noises=env["noises"]), loader, "learned")
    for kw in (dict(sgs_f1_average=None), dict(sgs_f1_average="micro"), dict(sgs_eval_report=None),
               dict(sgs_f1_average="micro", sgs_eval_report=None)):
        assert _run(env, _args(env, batched, noises=env["noises"], **kw), loader, "learned") == plain, kw
    assert calls == []
    one = S.evaluate(_args(env, False, sgs_f1_average="micro"), env["model"], loader, DEV, q=env["q"], mode="full")
    assert one == S.evaluate(_args(env, False), env["model"], loader, DEV, q=env["q"], mode="full") and calls == []
    _run(env, _args(env, batched, noises=env["noises"], sgs_f1_average="macro"), loader, "learned")
    assert len(calls) == 2                                                       # one launch per partition
    S.evaluate(_args(env, False, sgs_eval_report={}), env["model"], loader, DEV, q=env["q"], mode="full")
    assert len(calls) == 4


def test_calculate_f1_averages(env):
    S = env["S"]
    b = env["b1"]
    tr = {}
    S.evaluate(_args(env, False, _sgs_trace_eval=tr), env["model"], [b], DEV, q=env["q"], mode="full")
    logits = tr["mean"]
    pred = torch.argmax(logits.cpu(), dim=1).numpy()
    y, mask = b.y.to(DEV), b.val_mask.to(DEV)
    m = b.val_mask.numpy()
    for avg in R.AVERAGES:
        assert S.calculate_f1(logits, y, mask, average=avg) == pytest.approx(R.f1(b.y.numpy()[m], pred[m], avg), abs=TOL), avg
    assert S.calculate_f1(logits, y, mask) == S.calculate_f1(logits, y, mask, average="micro")
    assert S.calculate_f1(logits, y, torch.zeros_like(mask), average="macro") == 0
