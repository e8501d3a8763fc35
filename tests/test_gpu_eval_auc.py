"""GPU: evaluate / ensemble_evaluate with args.sgs_eval_auc and args.sgs_eval_auc_report, on the serial loop, the `full` / E <= q shortcut
and the batched GCN engine.  Three synthetic partitions of 50, 120 and 200 nodes (the first below q edges), C = 2 and C = 5.  Every count
is compared with tests/auc_ref.py on that run's OWN traced scores (args._sgs_trace_auc) by exact integer equality: each engine against the
reference, never against another engine."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DRAWS = 3
Q = 300
ENGINES = ("evaluate", "serial", "batched")


@pytest.fixture(scope="module", params=[2, 5], ids=["C2", "C5"])
def env(request):
    import sgs_gnn_amd as S
    C = request.param
    torch.manual_seed(29 + C)
    model = S.GNNModel(12, 16, C, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
    parts = [S.synthetic_graph(n, e, 12, C, seed=100 * C + k) for k, (n, e) in enumerate(((50, 200), (120, 900), (200, 1600)))]
    assert parts[0].edge_index.shape[1] <= Q < parts[1].edge_index.shape[1]
    parts[2].val_mask = parts[2].val_mask | (parts[2].train_mask & (torch.arange(200) % 3 == 0))     # a row in two splits counts in each
    return dict(S=S, C=C, model=model, parts=parts)


def _run(env, engine, mode, loader, **kw):
    """-> (triple, (noise clock, dropout clock) afterwards)"""
    S = env["S"]
    EV = sys.modules["sgs_gnn_amd.evaluate"]
    a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=DRAWS, **kw)
    if engine == "batched":
        a.sgs_eval_batch = True
    S.manual_seed(11)
    before = dict(EV.PATH_COUNTS)
    fn = S.evaluate if engine == "evaluate" else S.ensemble_evaluate
    got = fn(a, env["model"], loader, DEV, q=Q, mode=mode)
    if engine != "evaluate":
        assert EV.PATH_COUNTS[engine] == before[engine] + 1
    return got, (S.sampling._NoiseClock.tick, S.model._DropoutClock.tick)


def _noises(env, order, engine):
    """Explicit Exp(1) noise, one tensor per draw, for the partitions in `order`: a partition gets the same noise wherever it stands."""
    out = []
    for k in order:
        g = torch.Generator().manual_seed(500 + k)
        E = env["parts"][k].edge_index.shape[1]
        out += [torch.empty(E).exponential_(1, generator=g).to(DEV) for _ in range(1 if engine == "evaluate" else DRAWS)]
    return out


def _ref(tr, C):
    return R.counts(tr["scores"].cpu().numpy(), tr["y"].cpu().numpy(), tr["masks"].cpu().numpy(), C)


@pytest.mark.parametrize("mode", ["learned", "full"])
@pytest.mark.parametrize("engine", ENGINES)
def test_report_and_triple(env, engine, mode):
    C, parts = env["C"], env["parts"]
    S_cols = 1 if C == 2 else C
    M = sum(b.x.shape[0] for b in parts)
    off, clocks_off = _run(env, engine, mode, parts)
    rep, tr = {}, {}
    got, clocks = _run(env, engine, mode, parts, sgs_eval_auc_report=rep, _sgs_trace_auc=tr)
    assert got == off and clocks == clocks_off                                   # only the report flag: the triple and both clocks as without it
    assert tr["scores"].shape == (M, S_cols) and tr["y"].shape == (M,) and tr["masks"].shape == (3, M)
    assert torch.equal(tr["y"].cpu(), torch.cat([b.y for b in parts]))           # loader order
    want = _ref(tr, C)
    assert rep["counts"].dtype == torch.int64 and rep["counts"].device.type == "cpu" and rep["counts"].shape == (3, S_cols, 3)
    assert np.array_equal(rep["counts"].numpy(), want)                           # exact
    assert (want[:, :, 1] > 0).all() and (want[:, :, 2] > 0).all() and (want[:, :, 0] > 0).all()      # nothing vacuous: every column is defined
    tri, per = R.auc(want)
    assert rep["auc"] == tri and rep["per_class"] == per and rep["kind"] == ("binary" if C == 2 else "ovr_macro")
    assert rep["classes_defined"] == [S_cols] * 3
    # the loader in another order, every partition with the explicit noise it had before: the same counts
    reps = []
    for order in ((0, 1, 2), (2, 0, 1)):
        rep_p, tr_p = {}, {}
        _run(env, engine, mode, [parts[k] for k in order], sgs_eval_auc_report=rep_p, _sgs_trace_auc=tr_p, _sgs_noise_eval=_noises(env, order, engine))
        assert np.array_equal(rep_p["counts"].numpy(), _ref(tr_p, C))
        reps.append(rep_p["counts"])
    assert torch.equal(reps[0], reps[1])
    # the AUC triple
    rep_a = {}
    got_a, clocks_a = _run(env, engine, mode, parts, sgs_eval_auc=True, sgs_eval_auc_report=rep_a)
    assert got_a == rep_a["auc"] == tri and clocks_a == clocks_off
    assert _run(env, engine, mode, parts, sgs_eval_auc=True)[0] == tri
    assert _run(env, engine, mode, parts, sgs_eval_auc=True, sgs_f1_average="micro", sgs_eval_report={})[0] == tri


@pytest.mark.parametrize("engine", ENGINES)
def test_two_partitions_are_pooled(env, engine):
    S, C = env["S"], env["C"]
    b1, b2 = env["parts"][1], env["parts"][2]
    t1 = 1 if C == 2 else 0
    y2 = b2.y.clone()
    y2[b2.val_mask] = t1                                                         # planted: alone, partition 2 has no negative of that class in val
    b2p = S.Batch(x=b2.x, edge_index=b2.edge_index, y=y2, train_mask=b2.train_mask, val_mask=b2.val_mask, test_mask=b2.test_mask, prob=b2.prob)
    alone = []
    for b in (b1, b2p):
        rep = {}
        _run(env, engine, "full", [b], sgs_eval_auc_report=rep)
        alone.append((rep["auc"], [int(m.sum()) for m in (b.train_mask, b.val_mask, b.test_mask)]))
    rep, tr = {}, {}
    got, _ = _run(env, engine, "full", [b1, b2p], sgs_eval_auc=True, sgs_eval_auc_report=rep, _sgs_trace_auc=tr)
    assert tr["scores"].shape[0] == b1.x.shape[0] + b2.x.shape[0]
    want = _ref(tr, C)
    assert np.array_equal(rep["counts"].numpy(), want) and got == R.auc(want)[0]
    col = 0
    assert want[1, col, 1] > 0 and want[1, col, 2] > 0                           # pooled, the column is defined in val
    (a1, n1), (a2, n2) = alone
    assert a2[1] == 0.0                                                          # ... so its own val figure is the "undefined" 0.0
    weighted = (a1[1] * n1[1] + a2[1] * n2[1]) / (n1[1] + n2[1])
    assert abs(weighted - got[1]) > 1e-6, (weighted, got[1])                     # the size-weighted per-partition mean is another number


@pytest.mark.parametrize("engine", ENGINES)
def test_flags_off_launch_nothing_new(env, engine, monkeypatch):
    S = env["S"]
    calls = []
    real = S.ops.auc_pack

    def boom(*a, **k):
        raise AssertionError("ops.auc_pack was called with both flags off")
    monkeypatch.setattr(S.ops, "auc_pack", boom)
    plain = _run(env, engine, "learned", env["parts"])
    for kw in (dict(sgs_eval_auc=None), dict(sgs_eval_auc=False), dict(sgs_eval_auc_report=None), dict(sgs_eval_auc=False, sgs_eval_auc_report=None),
               dict(sgs_eval_auc=False, sgs_f1_average="macro")):
        if "sgs_f1_average" not in kw:
            assert _run(env, engine, "learned", env["parts"], **kw) == plain, kw
        else:
            _run(env, engine, "learned", env["parts"], **kw)
    monkeypatch.setattr(S.ops, "auc_pack", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    _run(env, engine, "learned", env["parts"], sgs_eval_auc_report={})
    assert len(calls) == len(env["parts"])                                       # one pack per partition
