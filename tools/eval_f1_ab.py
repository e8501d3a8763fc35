"""ensemble_evaluate with and without the per-class counts (args.sgs_f1_average="macro"), on the serial draw loop and on the batched GCN
engine, alternating in one process; and the confusion kernel alone in both forced forms.

    python tools/eval_f1_ab.py [--rounds 5] [--reps 3] [--shapes s3,s4] [--out profiles/r20_eval_f1_ab.json]
    python tools/eval_f1_ab.py --path off --root DIR --out profiles/r20_eval_f1_ab_parent.json    # one tree's flag-off arms alone
    python tools/eval_f1_ab.py --kernels [--out profiles/r20_confusion_kernels.json]              # sgs_confusion_counts alone, HIP events

Shapes: s3 = bench S3's 230-partition Reddit-like stream (reddit_partition_stream(num_parts=230, seed=1000); F = 602, C = 41), s4 = bench
S4's five partitions (synthetic_graph(33 869, 463 000, 128, 5, seed=300 + i, train_frac=0.2, power=0.6)); both with GNNModel(F, 256, C)
and the GCN scorer, num_samples_eval = 11, mode 'learned', q = 100 000, as tools/eval_ab.py and tools/eval_gine_ab.py.  Arms: serial and
batched (sgs_eval_batch=True) with the flag off, serial_macro and batched_macro with sgs_f1_average="macro" (one sgs_confusion_counts launch
per partition and one [3, C, C] read-back per evaluation on top).  One untimed pass of every arm first, then `rounds` rounds (whether the
serial and the batched triples are equal is recorded as f1_equal_off / f1_equal_macro); in a round the arms alternate `reps` times; a pass is timed
on the host clock around a device synchronise; reported: the median of all passes and [min, max] of the per-round medians.  Every pass
starts from the same noise-clock position, so all arms draw the same edge sets.

The yardstick is the PARENT commit's flag-off pass: `--path off --root DIR` runs the two flag-off arms alone on another checkout (library
built); they set no attribute the parent does not know, so this file runs there unchanged.

--kernels: ops.confusion_counts alone at the S3, S4, S2 and S5 partition shapes (1 013 x 41, 33 869 x 5, 19 793 x 70, 232 965 x 41), forced
direct (code 1) and forced privatised (code 2), alternating; logits whose argmax is the label on 80 % of the rows (the diagonal of the
matrix is hot, as with a trained model) and on uniformly random logits; masks 20 / 40 / 40 % disjoint; then sweeps for the automatic
rule's two thresholds: over N at C = 5 and C = 41 (256 to 16 384 rows) and over C (8 to 32) at 4 096, 33 869 and 232 965 rows.  Per form: `rounds` rounds of `iters`
back-to-back launches between two HIP events; reported: the median and [min, max] of the per-round microseconds per launch."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ARMS = ("serial", "serial_macro", "batched", "batched_macro")
OFF = ("serial", "batched")
Q = 100_000
KERNEL_SHAPES = (("S3", 1_013, 41), ("S4", 33_869, 5), ("S2", 19_793, 70), ("S5", 232_965, 41))
# where the automatic rule's two thresholds lie: over N at few and at many classes, over C at two partition sizes
SWEEP_SHAPES = tuple((f"n{n}_c{c}", n, c) for c in (5, 41) for n in (256, 1_024, 2_048, 4_096, 16_384)) + \
    tuple((f"n{n}_c{c}", n, c) for c in (8, 12, 16, 20, 24, 32) for n in (4_096, 33_869, 232_965))


def _load(shape, S, dev, torch):
    torch.manual_seed(0)
    if shape == "s3":
        parts = S.reddit_partition_stream(num_parts=230, seed=1000, device=dev)
        fin, ncls = 602, 41
    else:
        parts = [S.synthetic_graph(33_869, 463_000, 128, 5, seed=300 + i, train_frac=0.2, power=0.6, device=dev) for i in range(5)]
        fin, ncls = 128, 5
    model = S.GNNModel(fin, 256, ncls, dropout_prob=0.3, edge_mlp_type="GCN").to(dev)
    return parts, model


def _args(arm, draws):
    a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws)
    if arm.startswith("batched"):
        a.sgs_eval_batch = True
    if arm.endswith("_macro"):
        a.sgs_f1_average = "macro"
    return a


def _summary(rounds):
    flat = [t for r in rounds for t in r]
    meds = [statistics.median(r) for r in rounds]
    return {"median_s": statistics.median(flat), "round_median_min_s": min(meds), "round_median_max_s": max(meds), "passes": len(flat)}


def measure(shape, arms, rounds, reps, draws):
    import torch
    import sgs_gnn_amd as S
    EV = sys.modules["sgs_gnn_amd.evaluate"]
    dev = "cuda:0"
    parts, model = _load(shape, S, dev, torch)

    def one(arm):
        a = _args(arm, draws)
        path = arm.split("_")[0]
        S.manual_seed(11)
        torch.cuda.synchronize()
        before = dict(EV.PATH_COUNTS)
        t0 = time.perf_counter()
        f1 = S.ensemble_evaluate(a, model, parts, dev, q=Q, mode="learned")
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        assert EV.PATH_COUNTS[path] == before[path] + 1, f"{arm} took the other path"
        return t, f1

    for arm in arms:                                    # warm-up: allocator growth, library load
        one(arm)
    times = {arm: [] for arm in arms}
    f1 = {}
    for _ in range(rounds):
        rnd = {arm: [] for arm in arms}
        for _ in range(reps):
            for arm in arms:
                t, f1[arm] = one(arm)
                rnd[arm].append(t)
        for arm in arms:
            times[arm].append(rnd[arm])
    out = {"shape": shape, "head": "GCN", "partitions": len(parts), "draws": draws, "q": Q, "mode": "learned", "rounds": rounds,
           "reps": reps, "edges_sampled_partitions": sum(1 for b in parts if b.edge_index.shape[1] > Q),
           "arms": {arm: {**_summary(times[arm]), "f1": f1[arm]} for arm in arms}, "device": torch.cuda.get_device_name(0)}
    if "serial" in f1 and "batched" in f1:
        out["f1_equal_off"] = f1["serial"] == f1["batched"]
    if "serial_macro" in f1 and "batched_macro" in f1:
        out["f1_equal_macro"] = f1["serial_macro"] == f1["batched_macro"]
    for path in OFF:
        if path in times and path + "_macro" in times:
            out[f"{path}_macro_over_off"] = out["arms"][path + "_macro"]["median_s"] / out["arms"][path]["median_s"]
    return out


def kernels(rounds, iters):
    import torch
    import sgs_gnn_amd as S
    ops = S.ops
    dev = "cuda:0"
    res = {"timer": f"two HIP events around {iters} back-to-back ops.confusion_counts launches into one zeroed buffer; microseconds per launch; "
                    f"median and [min, max] of {rounds} rounds; forms alternating per round", "device": torch.cuda.get_device_name(0), "shapes": {}}
    try:
        for name, N, C in KERNEL_SHAPES + SWEEP_SHAPES:
            g = torch.Generator().manual_seed(N)
            y = torch.randint(0, C, (N,), generator=g)
            u = torch.rand(N, generator=g)
            masks = [(u < 0.2).to(dev), ((u >= 0.2) & (u < 0.6)).to(dev), (u >= 0.6).to(dev)]
            rnd = torch.randn(N, C, generator=g)
            hot = rnd.clone()
            right = torch.rand(N, generator=g) < 0.8
            hot[right, y[right]] = 10.0
            ops.confusion_variant_set(0)
            entry = {"N": N, "C": C, "automatic_form": ops.confusion_variant(N, C), "data": {}}
            for tag, x in (("argmax_is_label_80pct", hot), ("random_logits", rnd)):
                xd, yd = x.to(dev), y.to(dev)
                ref = None
                times = {1: [], 2: []}
                for code in (1, 2):                                   # warm-up and agreement of the two forms
                    ops.confusion_variant_set(code)
                    assert ops.confusion_variant(N, C) == code
                    c = ops.confusion_counts(xd, yd, masks)
                    ref = c if ref is None else ref
                    assert torch.equal(c, ref), "the two forms disagree"
                for _ in range(rounds):
                    for code in (1, 2):
                        ops.confusion_variant_set(code)
                        buf = torch.zeros(3, C, C, dtype=torch.int64, device=dev)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record()
                        for _ in range(iters):
                            ops.confusion_counts(xd, yd, masks, out=buf)
                        e1.record()
                        torch.cuda.synchronize()
                        times[code].append(e0.elapsed_time(e1) * 1000.0 / iters)
                        assert torch.equal(buf, ref * iters)
                entry["data"][tag] = {form: {"median_us": statistics.median(times[code]), "min_us": min(times[code]), "max_us": max(times[code])}
                                      for code, form in ((1, "direct"), (2, "privatised"))}
            res["shapes"][name] = entry
    finally:
        ops.confusion_variant_set(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", type=int, default=11)
    ap.add_argument("--shapes", default="s3,s4")
    ap.add_argument("--path", default="all", choices=ARMS + ("all", "off"))
    ap.add_argument("--kernels", action="store_true", help="time ops.confusion_counts alone in both forced forms and nothing else")
    ap.add_argument("--iters", type=int, default=200, help="--kernels: launches between the two events")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package and library are measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [s for s in a.shapes.split(",") if s]
    if any(s not in ("s3", "s4") for s in shapes):
        ap.error("--shapes from s3, s4")
    arms = list(ARMS) if a.path == "all" else list(OFF) if a.path == "off" else [a.path]
    sys.path.insert(0, os.path.abspath(a.root))
    import sgs_gnn_amd
    assert os.path.abspath(sgs_gnn_amd.__file__).startswith(os.path.abspath(a.root) + os.sep), "the package came from another tree"
    if a.kernels:
        res = kernels(a.rounds, a.iters)
    else:
        res = {"timer": "host clock around one ensemble_evaluate pass ending in a device synchronise; median of all passes, [min, max] of the "
                        "per-round medians; arms alternating in one process", "root": "this tree" if a.root == os.path.dirname(HERE) else "--root",
               "shapes": {}}
        for shape in shapes:
            res["shapes"][shape] = measure(shape, arms, a.rounds, a.reps, a.draws)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
