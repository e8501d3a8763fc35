"""Export of the learned sparse graph: the consensus of D draws, with a report.

`sparsify` turns a trained sparsifier and a partition loader into ONE fixed sparse graph per partition: every candidate edge is counted
over `n_draws` draws (the very draws `ensemble_evaluate` makes from the same seed), and the edges drawn most often are kept -- the q of
them with the largest (count, score) keys (`rule='topq'`), or every edge drawn in at least ceil(min_freq * n_draws) draws
(`rule='threshold'`).  Inference then runs one forward on the fixed graph (`evaluate(..., mode='full')` on the returned list) instead of
n_draws forwards on n_draws draws.

Per partition: the scores once, the draws in passes of ops.sample_topq_multi each followed by one ops.consensus_accum, then one
ops.consensus_select; two ops.edge_class_counts launches feed the report.  Nothing is read back inside the loop except, under
`rule='threshold'`, the partition's count histogram (128 integers) that gives the kept size; the report's numbers stay on the device until
one copy after the loader is exhausted.  The export is not a captured path.

The selection is by frequency alone: under args.sgs_cover_nodes the DRAWS are node-covering, the consensus itself makes no covering
promise (the report's "nodes_without_in_edge" shows what it covers).  Scores that differ only in their 6 lowest mantissa bits tie (and go
to the lower edge id): the selection key is 32 bits, 7 of count and 25 of score (sgs_consensus_select).

Test hooks: `args._sgs_noise_eval` as in evaluate.py (explicit Exp(1) noise per draw); `args.sgs_sparsify_pass` (absent / None: passes sized
by the byte budget; an int k >= 1: at most k draws per pass) -- the result does not depend on it."""
from __future__ import annotations

import math

import torch

from . import ops
from .data import Batch
from .eval_batch import EVAL_BATCH_BUDGET, engine_of, split_passes
from .sampling import _NoiseClock, cover_graph, cover_nodes
from .utils import different_label_stats

MODES = ("learned", "edge")
RULES = ("topq", "threshold")
MAX_DRAWS = ops.CONSENSUS_MAX_DRAWS


def threshold_count(min_freq: float, n_draws: int) -> int:
    """ceil(min_freq * n_draws), at least 1: the keep count from which `rule='threshold'` keeps an edge.  (A product that exceeds an
    integer by less than 1e-9 counts as that integer: 0.3 * 10 is 3 draws, not 4.)"""
    return max(1, math.ceil(min_freq * n_draws - 1e-9))


def _check(mode, n_draws, rule, min_freq, q):
    if mode not in MODES:
        raise ValueError(f"sparsify: mode={mode!r}, need one of {MODES}")
    if isinstance(n_draws, bool) or not isinstance(n_draws, int) or not 1 <= n_draws <= MAX_DRAWS:
        raise ValueError(f"sparsify: n_draws={n_draws!r}, need an int in 1..{MAX_DRAWS}")
    if rule not in RULES:
        raise ValueError(f"sparsify: rule={rule!r}, need one of {RULES}")
    if rule == "threshold":
        if isinstance(min_freq, bool) or not isinstance(min_freq, (int, float)) or not 0 < min_freq <= 1:
            raise ValueError(f"sparsify: min_freq={min_freq!r}, need a number in (0, 1] with rule='threshold'")
    elif min_freq is not None:
        raise ValueError("sparsify: min_freq is only meaningful with rule='threshold'")
    if isinstance(q, bool) or not isinstance(q, int) or q < 0:
        raise ValueError(f"sparsify: q={q!r}, need an int >= 0")


def _pass_plan(args, E: int, q: int, n_draws: int) -> list:
    """Draws per pass: the largest pass whose per-draw buffers (mask E, keys 4 E, ids 8 q) fit eval_batch's byte budget, or at most
    args.sgs_sparsify_pass draws."""
    k = getattr(args, "sgs_sparsify_pass", None)
    if k is None:
        k = max(1, EVAL_BATCH_BUDGET // max(5 * E + 8 * q + 64, 1))
    elif isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"args.sgs_sparsify_pass={k!r}: need None or an int >= 1")
    k = min(k, n_draws)
    return [k] * (n_draws // k) + ([n_draws % k] if n_draws % k else [])


def _num_classes(model, y) -> int:
    e = engine_of(model)
    if e is not None:
        return int(e.dims(model)[1])
    return int(y.max()) + 1 if y.numel() else 1


def _no_in_edge(edge_index, N: int):
    """Number of nodes without an in-edge, a device scalar, from the graph's destination-row CSR pointers."""
    if edge_index.shape[1] == 0:
        return N
    ptr = ops.get_graph(edge_index, N).in_ptr
    return (ptr[1:N + 1] == ptr[:N]).sum()


def sparsify(args, model, cluster_loader, device, q=500, mode='learned', n_draws=None, rule='topq', min_freq=None):
    """-> (list of Batch, report).  One fixed sparse graph per partition of `cluster_loader`: the consensus of `n_draws` (default
    args.num_samples_eval; 1..127) draws of q edges, drawn exactly as ensemble_evaluate draws them in `mode` 'learned' (scores from
    model.edge_prob_mlp) or 'edge' (the degree prior batch.prob), under args.sgs_cover_nodes / args.sgs_precision as there; the noise
    clock afterwards stands where ensemble_evaluate leaves it.  A partition with E <= q is kept whole (every count n_draws, no draw).

    Each returned Batch shares x, y and the three masks with its partition and carries edge_index [2, n] (original edge order), edge_id
    [n] (int64 ids into the partition's edge_index), edge_freq [n] (float32 count / n_draws), edge_score [n] (the score or prior of the
    kept edges) and prob (the degree prior of the kept graph); evaluate(args, model, batches, device, q, mode='full') runs on the list.

    report (pooled over the loader): "edges" {original, kept}; "original_graph" / "sampled_graph" {different_label_edges, total_edges,
    percentage}; "class_pairs" int64 [2, C, C] (original, kept; source class x destination class); "freq_hist" int64 [n_draws + 1] over all
    candidate edges; "nodes_without_in_edge" {original, kept}."""
    if n_draws is None:
        n_draws = int(args.num_samples_eval)
    _check(mode, n_draws, rule, min_freq, q)
    cover_nodes(args)                            # validated before any partition is read
    need = threshold_count(min_freq, n_draws) if rule == "threshold" else None
    noises = list(getattr(args, "_sgs_noise_eval", None) or [])
    out = []
    pairs = hist = holes = None
    n_orig = n_kept = 0
    model.eval()
    with ops.scorer_precision(getattr(args, "sgs_precision", None)), torch.no_grad():
        for batch in cluster_loader:
            batch = batch.to(device)
            ops._need_gpu(batch.x, batch.edge_index, batch.y)
            ops.new_memo_scope()
            ei, y = batch.edge_index.contiguous(), batch.y
            E, N = ei.shape[1], batch.x.shape[0]
            dev = ei.device
            if pairs is None:
                C = _num_classes(model, y)
                pairs = torch.zeros(2, C, C, dtype=torch.int64, device=dev)
                hist = torch.zeros(128, dtype=torch.int64, device=dev)
                holes = torch.zeros(2, dtype=torch.int64, device=dev)
            given = [noises.pop(0) if noises else None for _ in range(n_draws)]       # one per draw, as the evaluation loops pop them
            if mode == 'learned':
                if E > 0:
                    ops.get_pairs(ei, N, build=True)
                    score = model.edge_prob_mlp(batch.x, ei).reshape(-1).contiguous()
                else:
                    score = torch.zeros(0, dtype=torch.float32, device=dev)
                kind = ops.SAMPLE_LEARNED
            else:
                score, kind = batch.prob.contiguous(), ops.SAMPLE_PRIOR
            if E <= q:
                hist[n_draws] += E
                kept = Batch(x=batch.x, y=y, train_mask=batch.train_mask, val_mask=batch.val_mask, test_mask=batch.test_mask, edge_index=ei,
                             edge_id=torch.arange(E, dtype=torch.int64, device=dev),
                             edge_freq=torch.ones(E, dtype=torch.float32, device=dev), edge_score=score)
            else:
                passes, used = split_passes(_pass_plan(args, E, q, n_draws), given, _NoiseClock.seed, _NoiseClock.tick, dev)
                _NoiseClock.tick += used
                cover = cover_graph(args, batch)
                part_hist = torch.zeros(128, dtype=torch.int64, device=dev)
                count = None
                for k, (Dc, noise, seed, sid0) in enumerate(passes):
                    smp = ops.sample_topq_multi(kind, score, None, 0.0, q, ei, Dc, noise=noise, seed=seed, stream_id0=sid0,
                                                want_edge_index=False, cover=cover)
                    count = ops.consensus_accum(smp, count, first=k == 0, hist=part_hist if k == len(passes) - 1 else None)
                hist += part_hist
                size = q if rule == "topq" else int(part_hist[need:].sum())      # (threshold: the one small read-back per partition)
                r = ops.consensus_select(count, score, size, ei)
                kept = Batch(x=batch.x, y=y, train_mask=batch.train_mask, val_mask=batch.val_mask, test_mask=batch.test_mask,
                             edge_index=r.edge_index, edge_id=r.eid, edge_freq=r.count.to(torch.float32) / n_draws, edge_score=r.p)
            kept.prob = ops.degree_prior(kept.edge_index, N) if kept.edge_index.shape[1] > 0 else torch.zeros(0, dtype=torch.float32, device=dev)
            ops.edge_class_counts(ei, y, N, C, out=pairs[0])
            ops.edge_class_counts(kept.edge_index, y, N, C, out=pairs[1])
            holes[0] += _no_in_edge(ei, N)
            holes[1] += _no_in_edge(kept.edge_index, N)
            n_orig += E
            n_kept += kept.edge_index.shape[1]
            out.append(kept)
    if pairs is None:
        z = torch.zeros(2, 0, 0, dtype=torch.int64)
        return out, {"edges": {"original": 0, "kept": 0}, "original_graph": different_label_stats(z[0], 0),
                     "sampled_graph": different_label_stats(z[1], 0), "class_pairs": z,
                     "freq_hist": torch.zeros(n_draws + 1, dtype=torch.int64), "nodes_without_in_edge": {"original": 0, "kept": 0}}
    flat = torch.cat([pairs.reshape(-1), hist, holes]).cpu()                      # the one read-back of the report
    cc = pairs.numel()
    P, H, Z = flat[:cc].reshape(pairs.shape), flat[cc:cc + 128], flat[cc + 128:].tolist()
    return out, {"edges": {"original": n_orig, "kept": n_kept},
                 "original_graph": different_label_stats(P[0], n_orig), "sampled_graph": different_label_stats(P[1], n_kept),
                 "class_pairs": P, "freq_hist": H[:n_draws + 1].clone(),
                 "nodes_without_in_edge": {"original": int(Z[0]), "kept": int(Z[1])}}
