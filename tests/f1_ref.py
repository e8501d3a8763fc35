"""Reference for the per-class evaluation metrics (a helper, not a test file): micro / macro / weighted F1, per-class precision, recall,
F1 and support, and balanced accuracy, restated in numpy from LABEL AND PREDICTION ARRAYS (sklearn.metrics.f1_score's definitions with
labels=None and zero_division=0), without going through a confusion matrix; and a confusion matrix built with np.add.at."""
import numpy as np

AVERAGES = ("micro", "macro", "weighted")


def confusion(y, pred, C):
    """int64 [C, C]: M[t][p] = #{i : y_i == t and pred_i == p}."""
    M = np.zeros((C, C), dtype=np.int64)
    np.add.at(M, (np.asarray(y, dtype=np.int64), np.asarray(pred, dtype=np.int64)), 1)
    return M


def confusion3(y, pred, masks, C):
    """int64 [len(masks), C, C] over the rows each mask selects."""
    y, pred = np.asarray(y), np.asarray(pred)
    return np.stack([confusion(y[np.asarray(m, dtype=bool)], pred[np.asarray(m, dtype=bool)], C) for m in masks])


def _per_class(y, pred, c):
    tp = int(np.sum((y == c) & (pred == c)))
    fp = int(np.sum((y != c) & (pred == c)))
    fn = int(np.sum((y == c) & (pred != c)))
    return tp, fp, fn


def f1(y, pred, average):
    """sklearn.metrics.f1_score(y, pred, average=average, zero_division=0); 0 for no rows."""
    y, pred = np.asarray(y, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    if y.size == 0:
        return 0.0
    if average == "micro":
        return float(np.sum(y == pred)) / y.size
    labels = np.union1d(y, pred)                      # labels=None: the classes present in the truth or in the prediction
    fs, sups = [], []
    for c in labels:
        tp, fp, fn = _per_class(y, pred, c)
        fs.append(2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn > 0 else 0.0)
        sups.append(tp + fn)
    if average == "macro":
        return float(sum(fs)) / len(fs)
    if average == "weighted":
        return float(sum(f * s for f, s in zip(fs, sups))) / y.size
    raise ValueError(average)


def report(y, pred, C):
    """precision / recall / f1 / support per class 0..C-1 (zero_division=0), the three averages and balanced accuracy (the mean recall over
    the classes with support; 0 for no rows)."""
    y, pred = np.asarray(y, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    P, R, F, S = [], [], [], []
    for c in range(C):
        tp, fp, fn = _per_class(y, pred, c)
        P.append(tp / (tp + fp) if tp + fp else 0.0)
        R.append(tp / (tp + fn) if tp + fn else 0.0)
        F.append(2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
        S.append(tp + fn)
    have = [R[c] for c in range(C) if S[c]]
    return {"precision": P, "recall": R, "f1": F, "support": S, "micro": f1(y, pred, "micro"), "macro": f1(y, pred, "macro"),
            "weighted": f1(y, pred, "weighted"), "balanced_accuracy": sum(have) / len(have) if have else 0.0}
