"""GPU: ensemble_evaluate pinned to the REFERENCE (tests/golden/ensemble_eval_gcn.pt, made by tests/golden/gen_golden_eval.py running
the reference's evaluate.ensemble_evaluate unmodified): with the reference's own per-draw Exp(1) noise, both the serial loop and the
batched engine give the reference's per-draw and averaged logits (1e-4) and its F1 triple.  The PyG GCN layer is the oracle's
restatement in the generator, so that layer stays unpinned, as in the other fixtures."""
import argparse
import sys

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _setup():
    import sgs_gnn_amd as S
    fx = load_golden("ensemble_eval_gcn.pt")
    m = S.GNNModel(12, 16, 5, dropout_prob=0.3, edge_mlp_type="GCN")
    m.load_state_dict(fx["state0"])
    batches = [S.Batch(**{k: v.to(DEV) for k, v in b.items()}) for b in fx["batches"]]
    return S, fx, m.to(DEV), batches


def _noise_list(fx, mode, batches):
    """The noise hook pops one entry per draw and partition, in loader order; the reference drew only for partitions with E > q."""
    it = iter(fx["modes"][mode]["noise"])
    out = []
    for b in batches:
        out += [next(it).to(DEV) if b.edge_index.shape[1] > fx["q"] else None for _ in range(fx["draws"])]
    return out


@pytest.mark.parametrize("mode", ["learned", "edge"])
@pytest.mark.parametrize("path", ["serial", "batched"])
def test_matches_reference_ensemble_evaluate(mode, path):
    S, fx, m, batches = _setup()
    ref = fx["modes"][mode]
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    for order in ([0, 1], [1, 0]):                       # the trace keeps the LAST partition: each one is last once
        bs = [batches[i] for i in order]
        args = argparse.Namespace(degree_bias_coef=fx["degree_bias_coef"], num_samples_eval=fx["draws"])
        if path == "batched":
            args.sgs_eval_batch = True
        args._sgs_noise_eval = _noise_list(fx, mode, bs)
        args._sgs_trace_eval = {}
        before = dict(ev.PATH_COUNTS)
        f1 = S.ensemble_evaluate(args, m, bs, DEV, q=fx["q"], mode=mode)
        assert ev.PATH_COUNTS[path] == before[path] + 1
        last = order[-1]
        tr = args._sgs_trace_eval
        assert torch.allclose(tr["logits"].cpu(), ref["logits"][last], rtol=0, atol=1e-4)
        assert torch.allclose(tr["mean"].cpu(), ref["mean"][last], rtol=0, atol=1e-4)
        assert f1 == pytest.approx(ref["f1"], rel=0, abs=1e-12)      # the reference re-weights per-batch F1s: equal up to rounding
