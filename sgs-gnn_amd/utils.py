"""Mirror of the hot-path helpers of the reference's utils.py."""
from __future__ import annotations

import ctypes
import os
import random

import numpy as np
import torch

from . import ops


F1_AVERAGES = ("micro", "macro", "weighted")


def calculate_f1(logits, labels, mask, average="micro") -> float:
    """utils.py:163-169: sklearn micro-F1 of the argmax on masked rows == accuracy.  Computed on
    the device (sgs_masked_correct); only two ints cross to the host.  average="macro" / "weighted" (the lines the reference keeps
    commented out beside the micro one): the confusion matrix of the masked rows is counted on the device (ops.confusion_counts, the mask
    as split 0) and C * C ints cross to the host."""
    if average not in F1_AVERAGES:
        raise ValueError(f"calculate_f1: average={average!r}, need one of {F1_AVERAGES}")
    if average == "micro":
        c = ops.masked_correct(logits, labels, mask).tolist()
        return c[0] / c[1] if c[1] else 0.0
    none = torch.zeros_like(mask)
    return f1_from_confusion(ops.confusion_counts(logits, labels, (mask, none, none))[0].cpu(), average)


def _confusion_lists(conf):
    """-> a list of [C][C] lists of Python ints, one per split, and whether `conf` had the split axis."""
    M = conf.tolist() if hasattr(conf, "tolist") else conf
    if not M or not isinstance(M[0], (list, tuple)):
        raise ValueError("confusion matrix: need [C, C] or [S, C, C] integers")
    stacked = bool(M[0]) and isinstance(M[0][0], (list, tuple))
    Ms = M if stacked else [M]
    for m in Ms:
        if any(len(r) != len(m) for r in m):
            raise ValueError("confusion matrix: need square [C, C] blocks")
    return Ms, stacked


def _class_stats(m):
    """Per class of one [C][C] matrix (rows: truth, columns: prediction): (tp, support, predicted, f1)."""
    C = len(m)
    tp = [m[c][c] for c in range(C)]
    sup = [sum(m[c]) for c in range(C)]
    pred = [sum(m[t][c] for t in range(C)) for c in range(C)]
    f = [2.0 * tp[c] / (sup[c] + pred[c]) if sup[c] + pred[c] > 0 else 0.0 for c in range(C)]
    return tp, sup, pred, f


def _f1_one(m, average):
    tp, sup, pred, f = _class_stats(m)
    n = sum(sup)
    if n == 0:
        return 0.0
    if average == "micro":
        return sum(tp) / n
    if average == "macro":
        seen = [c for c in range(len(m)) if sup[c] + pred[c] > 0]          # sklearn's labels=None: present in the truth or the prediction
        return sum(f[c] for c in seen) / len(seen)
    return sum(f[c] * sup[c] for c in range(len(m))) / n


def f1_from_confusion(conf, average="micro"):
    """F1 of a confusion matrix (rows: truth, columns: prediction), as sklearn.metrics.f1_score(average=...) gives it on the labels and
    predictions the matrix counts; computed on the host in float64.  With tp_c = M[c][c], sup_c = sum_p M[c][p], pred_c = sum_t M[t][c]:
    f_c = 2 tp_c / (sup_c + pred_c) (0 where the denominator is 0);  "micro" = sum tp / sum M;  "macro" = the mean of f_c over the classes
    with sup_c + pred_c > 0;  "weighted" = sum f_c sup_c / sum sup_c.  An empty matrix gives 0.  `conf`: an integer tensor, array or nested
    list, [C, C] -> a float, or [S, C, C] -> a tuple of S floats."""
    if average not in F1_AVERAGES:
        raise ValueError(f"f1_from_confusion: average={average!r}, need one of {F1_AVERAGES}")
    Ms, stacked = _confusion_lists(conf)
    vals = tuple(_f1_one(m, average) for m in Ms)
    return vals if stacked else vals[0]


def classification_report(conf):
    """Per split of a confusion matrix ([C, C] -> one dict, [S, C, C] -> a list of S dicts): "precision", "recall", "f1" and "support" per
    class (lists of C; a ratio with a zero denominator is 0), the three averages "micro", "macro", "weighted" (f1_from_confusion) and
    "balanced_accuracy", the mean recall over the classes that have support (0 for an empty split)."""
    Ms, stacked = _confusion_lists(conf)
    out = []
    for m in Ms:
        tp, sup, pred, f = _class_stats(m)
        C = len(m)
        rec = [tp[c] / sup[c] if sup[c] else 0.0 for c in range(C)]
        have = [c for c in range(C) if sup[c]]
        out.append({"precision": [tp[c] / pred[c] if pred[c] else 0.0 for c in range(C)], "recall": rec, "f1": f, "support": sup,
                    "micro": _f1_one(m, "micro"), "macro": _f1_one(m, "macro"), "weighted": _f1_one(m, "weighted"),
                    "balanced_accuracy": sum(rec[c] for c in have) / len(have) if have else 0.0})
    return out if stacked else out[0]


def auc_from_counts(counts):
    """ROC-AUC from the integer counts of ops.auc_counts: `counts` is [3, S, 3] = {twoU, P, Nn} per (split, column) (an integer tensor, array
    or nested list).  -> (triple, per_class): per_class[s][c] = twoU / (2 P Nn) in float64 from exact Python integers, NaN where P Nn == 0
    (a column without a positive or without a negative item has no ROC curve); triple[s] = the unweighted mean over the split's defined
    columns (the binary figure for S = 1, one-vs-rest macro otherwise), 0.0 for a split with no defined column."""
    M = counts.tolist() if hasattr(counts, "tolist") else counts
    if len(M) != 3 or any(len(cell) != 3 for row in M for cell in row):
        raise ValueError("auc_from_counts: need [3, S, 3] integers {twoU, P, Nn}")
    per_class = [[int(u) / (2 * int(p) * int(n)) if int(p) * int(n) > 0 else float("nan") for u, p, n in row] for row in M]
    triple = []
    for row in per_class:
        have = [v for v in row if v == v]
        triple.append(sum(have) / len(have) if have else 0.0)
    return tuple(triple), per_class


def calculate_auc(logits, labels, mask) -> float:
    """ROC-AUC of `logits` [N, C] on the masked rows, as sklearn.metrics.roc_auc_score gives it (ties count one half): binary for C = 2 (the
    score is logits[:, 1] - logits[:, 0]), the unweighted one-vs-rest mean over the classes that have both kinds of rows for C > 2 (scores:
    log_softmax).  Sorted and counted on the device (ops.auc_pack, ops.auc_counts); 9 S integers cross to the host.  0.0 when no class is
    defined; C = 1 raises ValueError."""
    scores = ops.auc_scores(logits)
    none = torch.zeros_like(mask)
    keys = ops.auc_pack(scores, labels, (mask, none, none), logits.shape[1])
    return auc_from_counts(ops.auc_counts(keys, scores.shape[1]).cpu())[0][0]


def different_label_stats(pairs, total_edges: int) -> dict:
    """One graph's entry of count_edges_with_different_labels' dictionary from its class-pair table `pairs` (int [C, C], rows: the
    source's class, columns: the destination's; ops.edge_class_counts) and its number of edges: the off-diagonal mass, the edge count and
    their ratio in per cent (0 for a graph without edges)."""
    M = pairs.tolist() if hasattr(pairs, "tolist") else pairs
    diff = sum(int(v) for r, row in enumerate(M) for c, v in enumerate(row) if r != c)
    total = int(total_edges)
    return {"different_label_edges": diff, "total_edges": total, "percentage": (diff / total) * 100 if total > 0 else 0}


def count_edges_with_different_labels(data, sampled_edge_index) -> dict:
    """utils.py:291-343: how many edges join nodes of different labels, in `data.edge_index` ("original_graph") and in `sampled_edge_index`
    ("sampled_graph"); each entry holds "different_label_edges", "total_edges" and "percentage".  Two ops.edge_class_counts launches over
    the edge lists in place of the reference's Python loops over edges; the two [C, C] tables cross to the host in one copy.  The number of
    classes is read from the labels (max + 1)."""
    y = data.y.reshape(-1).to(torch.int64)
    N = y.numel()
    C = int(y.max()) + 1 if N else 1
    both = torch.zeros(2, C, C, dtype=torch.int64, device=y.device)
    ops.edge_class_counts(data.edge_index, y, N, C, out=both[0])
    ops.edge_class_counts(sampled_edge_index, y, N, C, out=both[1])
    M = both.cpu()
    return {"original_graph": different_label_stats(M[0], data.edge_index.shape[1]),
            "sampled_graph": different_label_stats(M[1], sampled_edge_index.shape[1])}


def consistency_loss(edge_probs, edge_indices, node_embeddings):
    """utils.py:187-211: MSE(edge_probs, cos(emb[src], emb[dst]))."""
    N = node_embeddings.shape[0]
    dev = node_embeddings.device
    y = torch.zeros(N, dtype=torch.int64, device=dev)
    tm = torch.zeros(N, dtype=torch.bool, device=dev)
    total, _ = ops.edge_regularizers(edge_probs, node_embeddings, edge_indices, y, tm, 0.0, 1.0)
    return total


def fix_seeds(seed=42):
    """utils.py:82-89, plus the counter-based noise / dropout streams of this package."""
    from .sampling import manual_seed
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    manual_seed(seed)


# ------------------------------------------------------------------ segment profiler (utils.py:13-80) + rocTX ranges
class _RocTx:
    """roctxRangePushA / roctxRangePop of the rocprofv3 marker library (librocprofiler-sdk-roctx.so; no-ops unless a profiler is
    attached: `rocprofv3 --marker-trace --kernel-trace -- python3 ...` shows the ranges beside the kernels)."""
    _lib = False            # False: not looked for yet; None: not available

    @classmethod
    def lib(cls):
        if cls._lib is False:
            cls._lib = None
            root = os.environ.get("ROCM_PATH", "/opt/rocm")
            for name in ("librocprofiler-sdk-roctx.so", "libroctx64.so"):
                try:
                    L = ctypes.CDLL(os.path.join(root, "lib", name))
                    L.roctxRangePushA.argtypes = [ctypes.c_char_p]
                    L.roctxRangePushA.restype = ctypes.c_int
                    L.roctxRangePop.restype = ctypes.c_int
                    cls._lib = L
                    break
                except (OSError, AttributeError):
                    continue
        return cls._lib

    @classmethod
    def push(cls, name: str) -> None:
        L = cls.lib()
        if L is not None:
            L.roctxRangePushA(name.encode())

    @classmethod
    def pop(cls) -> None:
        L = cls.lib()
        if L is not None:
            L.roctxRangePop()


SEGMENTS = ("edge_mlp_pre", "edge_score", "gnn_forward", "backward")      # model.py:17-43,103-131,156-163; training_hybrid.py:22-27


class GpuMemoryProfiler:
    """Drop-in for the reference's `GpuMemoryProfiler` (utils.py:13-80; attached as `model.gpu_profiler` and
    `model.edge_prob_mlp.gpu_profiler`, main.py:116-119): `begin(name)` / `end(name)` around the four segments `SEGMENTS`, per-epoch
    summaries with the reference's keys.  Two things on top: every segment is also a rocTX range of the same name (visible in a
    rocprofv3 trace next to the kernels it launched), and `memory=False` keeps the ranges but skips the two device synchronisations
    per segment that the memory snapshots cost (the reference's epoch times under --gpu_profile are pessimistic for that reason,
    SURVEY.md section 6).  In HIP-graph mode a step's segments are replayed, not launched: the ranges then bracket the replays
    (`replay:G1`, `backward`)."""

    def __init__(self, enabled=False, device=None, memory=True, roctx=True):
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.enabled = bool(enabled) and torch.cuda.is_available() and self.device.type == "cuda"
        self.memory, self.roctx = bool(memory), bool(roctx)
        self._epoch = None
        self._rows = {}            # epoch -> segment -> [(peak increase, allocated after, allocated increase)]
        self._open = {}

    def start_epoch(self, epoch):
        if self.enabled:
            self._epoch = epoch
            self._rows.setdefault(epoch, {})

    def end_epoch(self):
        if self.enabled:
            self._epoch = None
            self._open.clear()

    def _snapshot(self):
        torch.cuda.synchronize(self.device)
        return torch.cuda.max_memory_allocated(self.device), torch.cuda.memory_allocated(self.device)

    def begin(self, name):
        if not self.enabled or self._epoch is None:
            return
        if self.roctx:
            _RocTx.push(name)
        self._open[name] = self._snapshot() if self.memory else (0, 0)

    def end(self, name):
        if not self.enabled or self._epoch is None:
            return 0, 0
        was = self._open.pop(name, None)
        if was is None:
            return 0, 0
        peak, alloc = self._snapshot() if self.memory else (0, 0)
        if self.roctx:
            _RocTx.pop()
        row = (max(0, peak - was[0]), alloc, alloc - was[1])
        self._rows.setdefault(self._epoch, {}).setdefault(name, []).append(row)
        return row[0], row[1]

    def summarize_epoch(self, epoch):
        out = {}
        if not self.enabled:
            return out
        mb = float(1024 ** 2)
        for name, rows in self._rows.get(epoch, {}).items():
            if not rows:
                continue
            cols = list(zip(*rows))
            d = {"calls": len(rows)}
            for key, vals in (("peak_inc", cols[0]), ("alloc_after", cols[1]), ("alloc_inc", cols[2])):
                d[f"max_{key}_bytes"] = max(vals)
                d[f"max_{key}_mb"] = max(vals) / mb
                d[f"mean_{key}_mb"] = (sum(vals) / len(vals)) / mb
            out[name] = d
        return out


class segment:
    """`with segment(module_or_profiler, "edge_score"):` -- begin / end on the object's `gpu_profiler` when it has one (no-op otherwise)."""
    __slots__ = ("prof", "name")

    def __init__(self, owner, name):
        self.prof = owner if isinstance(owner, GpuMemoryProfiler) else getattr(owner, "gpu_profiler", None)
        self.name = name

    def __enter__(self):
        if self.prof is not None:
            self.prof.begin(self.name)
        return self

    def __exit__(self, *exc):
        if self.prof is not None:
            self.prof.end(self.name)
        return False
