"""Cost of the class-weighted / label-smoothed cross entropy on the hot path, measured on the GPU.

    python tools/weighted_ce_probe.py kernels [--shapes s3,s4] [--reps 50] [--rounds 7] [--out profiles/r14_weighted_ce_probe.json]
    python tools/weighted_ce_probe.py steps [--parts 60] [--epochs 3] [--criterion weighted|plain] [--out profiles/r14_weighted_ce_steps.json]

kernels: forward + backward of the cross entropy alone on a partition's logits at bench S3's partition shape (N = 1 013, C = 41) and
S4's (N = 33 869, C = 5), 60 % train rows, HIP events around one forward + backward, three arms alternating in one process:
  (a) plain     ops.masked_cross_entropy(logits, y, mask)                                    (ce_rows, ce_final, ce_bwd)
  (b) weighted  ops.masked_cross_entropy(logits, y, mask, weight=w, label_smoothing=0.1)     (ce_rows<true>, ce_final<true>, ce_bwd<true, false>)
  (c) as given  nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)(logits[mask], y[mask])    (the boolean-index gathers and their
                device-to-host sync; what a run did with this criterion before the fused chain took it)
(b) and (c) must agree to 1e-5 relative in loss and gradient, else the timing is void and the probe raises.  3 untimed rounds, then
`rounds` rounds of `reps` alternating repeats, the arm that opens a repeat rotating so that no arm always follows the same one;
reported: the median over all repeats, the min / max of the per-round medians, and the ratios weighted / plain and as given / weighted of the medians.

steps: steps / s of hybrid training (gate, both regularisers, dropout 0.3, FusedAdam, args.sgs_hipgraph) over `parts` S3-like partitions
of bench.py's stream under nn.CrossEntropyLoss(weight=w, label_smoothing=0.1) (or the plain criterion): one untimed epoch (captures,
gate mix), then `epochs` timed epochs between device synchronisations; the median epoch is reported.  The same command on a commit
without the weighted chain runs every step eagerly under the weighted criterion: that is the baseline."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"s3": dict(N=1013, C=41), "s4": dict(N=33_869, C=5)}
EPS = 0.1


def _weight(C, dev):
    return (torch.rand(C, generator=torch.Generator().manual_seed(7)) * 4.8 + 0.2).to(dev)


def kernels(S, a):
    ops, dev = S.ops, "cuda:0"
    out = {}
    for name in a.shapes.split(","):
        N, C = SHAPES[name]["N"], SHAPES[name]["C"]
        g = torch.Generator().manual_seed(11)
        logits = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
        y = torch.randint(0, C, (N,), generator=g).to(dev)
        mask = (torch.rand(N, generator=g) < 0.6).to(dev)
        w = _weight(C, dev)
        crit = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=EPS)
        arms = {"plain": lambda: ops.masked_cross_entropy(logits, y, mask),
                "weighted": lambda: ops.masked_cross_entropy(logits, y, mask, weight=w, label_smoothing=EPS),
                "as_given": lambda: crit(logits[mask], y[mask])}

        def once(fn):
            logits.grad = None
            loss = fn()
            loss.backward()
            return loss.detach(), logits.grad

        lb, gb = once(arms["weighted"])
        lc, gc = once(arms["as_given"])
        gb, gc = gb.clone(), gc.clone()
        el, eg = float((lb - lc).abs() / lc.abs()), float((gb - gc).abs().max() / gc.abs().max())
        if not (el < 1e-5 and eg < 1e-5):
            raise SystemExit(f"{name}: weighted and as-given disagree (loss {el:.2e}, gradient {eg:.2e}): timing void")

        def timed(fn):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            once(fn)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3          # us

        for _ in range(3):
            for fn in arms.values():
                for _ in range(a.reps):
                    once(fn)
        ts, order = {k: [] for k in arms}, list(arms)
        for _ in range(a.rounds):
            rt = {k: [] for k in arms}
            for rep in range(a.reps):
                for j in range(len(order)):                       # the arm that opens a repeat rotates: no arm always follows the same one
                    k = order[(rep + j) % len(order)]
                    rt[k].append(timed(arms[k]))
            for k in arms:
                ts[k].append(rt[k])
        rec = {"N": N, "C": C, "train_rows": int(mask.sum()), "label_smoothing": EPS, "agree_loss": el, "agree_grad": eg,
               "reps": a.reps, "rounds": a.rounds, "unit": "us per forward + backward (HIP events, host launch time included)"}
        for k in arms:
            meds = [statistics.median(r) for r in ts[k]]
            rec[k] = {"median": round(statistics.median([t for r in ts[k] for t in r]), 2), "round_median_min": round(min(meds), 2),
                      "round_median_max": round(max(meds), 2)}
        rec["weighted_over_plain"] = round(rec["weighted"]["median"] / rec["plain"]["median"], 3)
        rec["as_given_over_weighted"] = round(rec["as_given"]["median"] / rec["weighted"]["median"], 3)
        out[name] = rec
        print(json.dumps({name: rec}))
    return out


def steps(S, a):
    import bench
    dev = "cuda:0"
    model, opt_gnn, opt_edge, opt_all = bench.build_model(S, dev, fused=True)
    w = _weight(bench.NCLS, dev)
    crit = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=EPS) if a.criterion == "weighted" else torch.nn.CrossEntropyLoss()
    args = bench.make_args(dev, sgs_hipgraph=True)
    pool = bench.make_pool(S, 0, 1, a.parts, dev)
    torch.cuda.synchronize()

    def epoch(e):
        with contextlib.redirect_stdout(io.StringIO()):
            return S.train(args, e, 10, model, opt_gnn, opt_edge, opt_all, crit, pool, q=bench.Q, alternate_frequency=0)
    epoch(0)
    torch.cuda.synchronize()
    dts, losses = [], []
    for e in range(a.epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = epoch(1 + e)
        torch.cuda.synchronize()
        dts.append(time.perf_counter() - t0)
        losses.append(r[0])
    sg = getattr(model, "_sgs_stepgraphs", None)
    rec = {"criterion": a.criterion, "parts": len(pool), "epochs": a.epochs, "replayed": sg is not None,
           "captures": None if sg is None else sg.captures, "steps_per_s": round(len(pool) / statistics.median(dts), 1),
           "steps_per_s_per_epoch": [round(len(pool) / d, 1) for d in dts], "mean_loss_per_epoch": [round(float(v), 5) for v in losses]}
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "steps"))
    ap.add_argument("--shapes", default="s3,s4")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--criterion", choices=("weighted", "plain"), default="weighted")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weighted_ce_probe: no GPU visible (timings are taken on the device only)")
    import sgs_gnn_amd as S
    rec = kernels(S, a) if a.mode == "kernels" else steps(S, a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
