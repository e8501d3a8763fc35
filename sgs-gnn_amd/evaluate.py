"""Mirror of the reference's evaluate.py: `evaluate` and `ensemble_evaluate` (same signatures and
return tuple).  The three kernels of the training path are reused forward-only; differences that do
not change results: the scorer runs ONCE per batch instead of once per ensemble draw (model.eval():
no dropout, identical inputs => identical probabilities, evaluate.py:84), logits are averaged with a
running sum, and the per-split correct counts stay on the device until the end of the loader.

Test hooks: `args._sgs_noise_eval = [noise_0, noise_1, ...]` feeds explicit Exp(1) noise per draw; `args._sgs_trace_eval = {}`
receives the last partition's per-draw logits [D, N, C] ("logits"), averaged logits ("mean") and drawn edge lists ("edges").

Batched engine (opt-in, `args.sgs_eval_batch` and five further opt-ins: eval_batch.py's module docstring has the rules): all draws of a
partition run as passes of batched kernels (eval_batch.run_partition) instead of the serial loop below, with the same drawn
edge sets and the same clocks afterwards.  `PATH_COUNTS` records which path each ensemble_evaluate call took.

Per-class metrics (both functions, the serial loop and every batched engine): `args.sgs_f1_average` (absent / None / "micro" = the accuracy
triple as ever; "macro" / "weighted" = the returned triple holds that F1 average) and `args.sgs_eval_report` (absent / None = off; a dict
receives "confusion", an int64 CPU tensor [3, C, C] (split, true class, predicted class), and "report", utils.classification_report of it;
both None for an empty loader).  When either asks for per-class counts, one [3, C, C] int64 buffer is zeroed per evaluation, every partition
adds one ops.confusion_counts launch on its final mean logits, and the buffer is read once after the loader is exhausted; otherwise nothing
new is launched or allocated, and with "micro" the triple always comes from the six counters.  The averages are POOLED over the loader:
they are taken from the confusion matrix of all masked nodes of all partitions.  (The reference, with its macro line switched on, would
weight per-partition macro values by partition size; the two agree for micro and on a one-partition loader.  The pooled value does not
depend on how the graph was partitioned and does not drop a class from the partitions where it happens to be absent.)

ROC-AUC (both functions, the serial loop, the `full` / E <= q shortcut and every batched engine): `args.sgs_eval_auc` (absent / None / False
= off; True = the returned triple is the AUC triple; together with a macro / weighted sgs_f1_average it raises: two claims on one triple) and
`args.sgs_eval_auc_report` (None or a dict that receives "counts", an int64 CPU tensor [3, S, 3] = {twoU, P, Nn} per (split, column), "per_class",
"auc", "kind" ("binary" for C = 2, "ovr_macro" otherwise) and "classes_defined"; all None for an empty loader).  The definition is
include/sgs_hip.h's (sklearn.metrics.roc_auc_score: ties count one half; NaN scores and labels outside [0, C) drop the item).  When either is
set, every partition runs the score ops (ops.auc_scores) and ONE sgs_auc_pack on its final mean logits into its own key tensor, and after
the loader there is one concatenation, one sgs_auc_counts and one read-back; otherwise nothing new is launched or allocated.  Like the F1
averages the figure is POOLED over the loader: the ranking is over all masked nodes of all partitions.  Neither clock moves.  Test hook:
`args._sgs_trace_auc = {}` receives the pooled "scores" [M, S], "y" [M] and "masks" [3, M] in loader order.
"""
from __future__ import annotations

import torch

from . import ops
from .eval_batch import (EVAL_BATCH_BUDGET, HEADS, _head_dims, _head_of,  # noqa: F401  (these four: reached as evaluate.X by tests and tools)
                         _batched_ok, engine_of, plan_draws, run_partition, split_passes)
from .model import _DropoutClock
from .utils import F1_AVERAGES, auc_from_counts, classification_report, f1_from_confusion
from .sampling import _NoiseClock, cover_graph, cover_nodes, draw_learned, draw_prior, random_edge_sampling

PATH_COUNTS = {"serial": 0, "batched": 0}


def _one_draw(args, model, batch, q, mode, edge_probs, noise):
    """-> (logits, the edge list the model ran on)."""
    if mode == 'learned':
        if batch.edge_index.shape[1] > q:
            smp = draw_learned(None, edge_probs, batch.edge_index, q, args.degree_bias_coef, istest=True, noise=noise,
                               cover=cover_graph(args, batch))
            w = ops.st_weights(edge_probs, None, args.degree_bias_coef, smp.stats, smp.eid)     # sampling.py:137-155
            return model(batch, smp.edge_index, w), smp.edge_index
        return model(batch, batch.edge_index), batch.edge_index
    if mode == 'random':
        if batch.edge_index.shape[1] > q:
            ei = random_edge_sampling(batch.edge_index, q=q, cover=cover_graph(args, batch))
            return model(batch, ei), ei
        return model(batch, batch.edge_index), batch.edge_index
    if mode == 'edge':
        if batch.edge_index.shape[1] > q:
            ei = draw_prior(batch.prob, batch.edge_index, q, noise=noise, cover=cover_graph(args, batch)).edge_index
            return model(batch, ei), ei
        return model(batch, batch.edge_index), batch.edge_index
    if mode == 'full':
        return model(batch, batch.edge_index), batch.edge_index
    raise ValueError("Invalid mode. Choose 'learned', 'random', or 'full'.")


def _f1_opts(args):
    """(average, report dict or None, whether per-class counts are needed) from args.sgs_f1_average and args.sgs_eval_report; a bad value
    raises ValueError here, before any partition is read."""
    avg = getattr(args, "sgs_f1_average", None)
    if avg is None:
        avg = "micro"
    if not isinstance(avg, str) or avg not in F1_AVERAGES:
        raise ValueError(f"args.sgs_f1_average={avg!r}: need None or one of {F1_AVERAGES}")
    rep = getattr(args, "sgs_eval_report", None)
    if rep is not None and not isinstance(rep, dict):
        raise ValueError(f"args.sgs_eval_report={rep!r}: need None or a dict (it receives 'confusion' and 'report')")
    return avg, rep, avg != "micro" or rep is not None


def _add_confusion(conf, out, batch):
    """One partition's confusion counts of its final mean logits `out`, added to the evaluation's buffer (made on the first partition)."""
    if conf is None:
        conf = torch.zeros(3, out.shape[1], out.shape[1], dtype=torch.int64, device=out.device)
    return ops.confusion_counts(out, batch.y, (batch.train_mask, batch.val_mask, batch.test_mask), out=conf)


def _finish(avg, rep, conf, micro, auc=None):
    """The triple to return: `micro` (from the six counters) unless another average or the AUC was asked for; fills the report dicts."""
    if auc is not None:
        micro = auc.finish(micro)
    if rep is not None:
        rep["confusion"] = rep["report"] = None
    if conf is None:
        return micro
    M = conf.cpu()
    if rep is not None:
        rep["confusion"], rep["report"] = M, classification_report(M)
    return micro if avg == "micro" else f1_from_confusion(M, avg)


AUC_REPORT_KEYS = ("counts", "per_class", "auc", "kind", "classes_defined")


class _AucPool:
    """The ROC-AUC side of one evaluation: per partition the score ops and ONE sgs_auc_pack into that partition's own key tensor; after the
    loader one concatenation, one sgs_auc_counts and one read-back of the [3, S, 3] counts."""

    def __init__(self, on, rep, trace):
        self.on, self.rep, self.trace = on, rep, trace
        self.keys, self.S, self.traced = [], None, []

    def add(self, out, batch):
        scores = ops.auc_scores(out)                                                 # [N, 1] (C = 2) or log_softmax [N, C]; C = 1: ValueError
        masks = (batch.train_mask, batch.val_mask, batch.test_mask)
        self.keys.append(ops.auc_pack(scores, batch.y, masks, out.shape[1]))
        self.S = scores.shape[1]
        if self.trace is not None:
            self.traced.append((scores, batch.y, torch.stack(masks)))

    def finish(self, triple):
        """`triple` unless args.sgs_eval_auc asked for the AUC triple; fills the report dict (None everywhere for an empty loader)."""
        if self.rep is not None:
            self.rep.update(dict.fromkeys(AUC_REPORT_KEYS))
        if not self.keys:
            return (0, 0, 0) if self.on else triple
        if self.trace is not None:
            self.trace["scores"] = torch.cat([t[0] for t in self.traced])
            self.trace["y"] = torch.cat([t[1] for t in self.traced])
            self.trace["masks"] = torch.cat([t[2] for t in self.traced], dim=1)
        keys = self.keys[0] if len(self.keys) == 1 else torch.cat(self.keys)
        counts = ops.auc_counts(keys, self.S).cpu()
        auc, per_class = auc_from_counts(counts)
        if self.rep is not None:
            self.rep.update(counts=counts, per_class=per_class, auc=auc, kind="binary" if self.S == 1 else "ovr_macro",
                            classes_defined=[sum(1 for v in row if v == v) for row in per_class])
        return auc if self.on else triple


def _auc_opts(args, avg):
    """The evaluation's _AucPool, or None when neither args.sgs_eval_auc nor args.sgs_eval_auc_report asks for one; a bad value, or
    sgs_eval_auc together with a macro / weighted sgs_f1_average (two claims on the one returned triple), raises ValueError here, before
    any partition is read."""
    on = getattr(args, "sgs_eval_auc", None)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"args.sgs_eval_auc={on!r}: need None, False or True")
    rep = getattr(args, "sgs_eval_auc_report", None)
    if rep is not None and not isinstance(rep, dict):
        raise ValueError(f"args.sgs_eval_auc_report={rep!r}: need None or a dict (it receives {AUC_REPORT_KEYS})")
    if on and avg != "micro":
        raise ValueError(f"args.sgs_eval_auc=True together with args.sgs_f1_average={avg!r}: both claim the returned triple; set one of them")
    if not on and rep is None:
        return None
    return _AucPool(on, rep, getattr(args, "_sgs_trace_auc", None))


def _run(args, model, cluster_loader, device, q, mode, n_draws):
    cover_nodes(args)                       # args.sgs_cover_nodes: validated before any partition is read
    avg, rep, per_class = _f1_opts(args)
    auc = _auc_opts(args, avg)
    model.eval()
    counts = conf = None
    noises = list(getattr(args, "_sgs_noise_eval", None) or [])
    trace = getattr(args, "_sgs_trace_eval", None)
    with torch.no_grad():
        for batch in cluster_loader:
            batch = batch.to(device)
            ops.new_memo_scope()
            edge_probs = None
            if mode == 'learned' and batch.edge_index.shape[1] > q:
                ops.get_pairs(batch.edge_index, batch.x.shape[0], build=True)     # once per partition (cached)
                edge_probs = model.edge_prob_mlp(batch.x, batch.edge_index).squeeze()         # encoder over the FULL batch graph
            out = None
            logs, edges = [], []
            for _ in range(n_draws):
                o, ei = _one_draw(args, model, batch, q, mode, edge_probs, noises.pop(0) if noises else None)
                out = o if out is None else out + o
                if trace is not None:
                    logs.append(o)
                    edges.append(ei)
            if n_draws > 1:
                out = out / n_draws                                                           # torch.mean(torch.stack(outs))
            if trace is not None:
                trace["logits"], trace["mean"], trace["edges"] = torch.stack(logs), out, torch.stack(edges)
            c = torch.stack([ops.masked_correct(out, batch.y, m) for m in (batch.train_mask, batch.val_mask, batch.test_mask)])
            counts = c.to(torch.int64) if counts is None else counts + c
            if per_class:
                conf = _add_confusion(conf, out, batch)
            if auc is not None:
                auc.add(out, batch)
    if counts is None:
        return _finish(avg, rep, None, (0, 0, 0), auc)
    c = counts.tolist()
    # sum_b f1_b * n_b / sum_b n_b  ==  sum_b correct_b / sum_b n_b   (utils.calculate_f1 is accuracy)
    return _finish(avg, rep, conf, tuple((c[s][0] / c[s][1]) if c[s][1] > 0 else 0 for s in range(3)), auc)


def _run_batched(args, model, cluster_loader, device, q, mode, n_draws):
    """The serial loop's result with every partition's draws in batched passes (eval_batch.run_partition: one host call per partition)."""
    if mode not in ('learned', 'random', 'edge', 'full'):
        raise ValueError("Invalid mode. Choose 'learned', 'random', or 'full'.")
    avg, rep, per_class = _f1_opts(args)
    auc = _auc_opts(args, avg)
    model.eval()
    counts = conf = None
    noises = list(getattr(args, "_sgs_noise_eval", None) or [])
    trace = getattr(args, "_sgs_trace_eval", None)
    engine = engine_of(model)
    H, C = engine.dims(model)
    prepare = lambda b, weighted: engine.prepare(model, b, weighted)                 # (the row is looked up once per call, not per partition)
    plan_kw = dict(engine.plan_kw(model), head=engine.head, cover=cover_nodes(args))   # (under the flag only with sgs_eval_batch_cover: _batched_ok)
    with torch.no_grad():
        for batch in cluster_loader:
            batch = batch.to(device)
            ops.new_memo_scope()
            if counts is None:
                counts = torch.zeros(6, dtype=torch.int64, device=device)
            E, N = batch.edge_index.shape[1], batch.x.shape[0]
            given = [noises.pop(0) if noises else None for _ in range(n_draws)]     # the serial loop pops one per draw, whatever the mode
            if mode == 'full' or E <= q:
                out = model(batch, batch.edge_index)                                 # every draw runs on the whole partition
                _DropoutClock.tick += (n_draws - 1) * engine.ticks                          # the serial loop's other n_draws - 1 forwards
                acc = torch.empty_like(out)
                ops.ensemble_mean_correct(out, 0, n_draws, acc, True, True, n_draws, batch.y,
                                          (batch.train_mask, batch.val_mask, batch.test_mask), counts)
                if trace is not None:
                    trace["logits"], trace["mean"] = out.unsqueeze(0).expand(n_draws, *out.shape), acc
                    trace["edges"] = batch.edge_index.unsqueeze(0).expand(n_draws, *batch.edge_index.shape)
                if per_class:
                    conf = _add_confusion(conf, acc, batch)
                if auc is not None:
                    auc.add(acc, batch)
                continue
            if mode == 'learned':
                ops.get_pairs(batch.edge_index, N, build=True)
                p = model.edge_prob_mlp(batch.x, batch.edge_index).squeeze().contiguous()
                kind = ops.SAMPLE_LEARNED
            elif mode == 'edge':
                p, kind = batch.prob, ops.SAMPLE_PRIOR
            else:
                p, kind = None, ops.SAMPLE_LEARNED
                given = [None] * n_draws                                             # random_edge_sampling takes no noise
            plan = plan_draws(E, q, N, H, C, n_draws, args.sgs_eval_batch, **plan_kw)
            passes, used = split_passes(plan, given, _NoiseClock.seed, _NoiseClock.tick, device)
            _NoiseClock.tick += used
            acc = run_partition(batch, prepare, q, kind, p, passes, counts, trace, cover_graph(args, batch))
            if per_class:
                conf = _add_confusion(conf, acc, batch)                              # the mean the last sgs_ensemble_mean_correct pass left
            if auc is not None:
                auc.add(acc, batch)
            # GNNModel.forward and GAT.forward take one dropout seed per call, in eval mode too (GIN and Cheb none): leave the dropout
            # clock where the serial loop's n_draws forwards leave it, so that training after an evaluation draws the same masks whichever
            # path evaluated
            _DropoutClock.tick += n_draws * engine.ticks
    if counts is None:
        return _finish(avg, rep, None, (0, 0, 0), auc)
    c = counts.tolist()
    return _finish(avg, rep, conf, tuple((c[2 * s] / c[2 * s + 1]) if c[2 * s + 1] > 0 else 0 for s in range(3)), auc)


def evaluate(args, model, cluster_loader, device, q=500, mode=None, temperature=1.0):
    """evaluate.py:6-67.  args.sgs_precision ("fp32" default / "bf16"): the scorer's precision for the pass (ops.scorer_precision)."""
    with ops.scorer_precision(getattr(args, "sgs_precision", None)):
        return _run(args, model, cluster_loader, device, q, mode, 1)


def ensemble_evaluate(args, model, cluster_loader, device, q=500, mode=None, temperature=1.0):
    """evaluate.py:70-173: mean of the logits of args.num_samples_eval independent draws."""
    with ops.scorer_precision(getattr(args, "sgs_precision", None)):
        n_draws = int(args.num_samples_eval)
        if _batched_ok(args, model, n_draws):
            PATH_COUNTS["batched"] += 1
            return _run_batched(args, model, cluster_loader, device, q, mode, n_draws)
        PATH_COUNTS["serial"] += 1
        return _run(args, model, cluster_loader, device, q, mode, n_draws)
