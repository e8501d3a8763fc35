"""ensemble_evaluate with the GATv2 head (GATModel(gat_v2=True)): the serial draw loop against the batched engine
(args.sgs_eval_batch_gatv2), alternating in one process.

    python tools/eval_gatv2_ab.py [--rounds 5] [--reps 3] [--shapes s3,s4] [--out profiles/r19_eval_gatv2_ab.json]
    python tools/eval_gatv2_ab.py --path serial --root DIR --out profiles/r19_eval_gatv2_ab_parent.json    # one tree's serial loop alone
    python tools/eval_gatv2_ab.py --path batched --passes 3 --shapes s3 --configs heads8_edge      # untimed passes of one arm, for a kernel trace

Shapes: s3 = bench S3's 230-partition Reddit-like stream (reddit_partition_stream(num_parts=230, seed=1000); F = 602, C = 41), s4 = bench
S4's five partitions (synthetic_graph(33 869, 463 000, 128, 5, seed=300 + i, train_frac=0.2, power=0.6)); the GCN scorer,
num_samples_eval = 11, mode 'learned', q = 100 000, as tools/eval_ab.py and tools/eval_gine_ab.py.  Configurations: heads8_edge =
GATModel(F, 256, C, gat_heads=8, gat_edge_weight=True, gat_v2=True), heads1 = GATModel(F, 256, C, gat_heads=1, gat_v2=True) (one head, no
edge term).  Arms: serial (no opt-in: the serial loop) and batched (sgs_eval_batch=True, heads ["GAT"], sgs_eval_batch_gatv2: the
engine).  One untimed pass of every arm first -- with both arms present their F1 triples are asserted equal there, before anything is
timed -- then `rounds` rounds; in a round the arms alternate `reps` times; a pass is timed on the host clock around a device synchronise;
reported: the median of all passes and [min, max] of the per-round medians.  Every pass starts from the same noise-clock position, so the
two arms draw the same edge sets.

The yardstick is the PARENT commit's serial loop: `--path serial --root DIR` runs the serial arm alone on another checkout (library
built); that arm sets no attribute the parent does not know, so this file runs there unchanged.

--passes K: K untimed passes of the chosen arm(s) and nothing else, so that `rocprofv3 --kernel-trace --stats -- python
tools/eval_gatv2_ab.py --path batched --passes 3 --shapes s3` counts the launches of one arm."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ARMS = ("serial", "batched")
Q = 100_000


CONFIGS = {"heads8_edge": dict(gat_heads=8, gat_edge_weight=True), "heads1": dict(gat_heads=1, gat_edge_weight=False)}


def _load(shape, config, S, dev, torch):
    torch.manual_seed(0)
    if shape == "s3":
        parts = S.reddit_partition_stream(num_parts=230, seed=1000, device=dev)
        fin, ncls = 602, 41
    else:
        parts = [S.synthetic_graph(33_869, 463_000, 128, 5, seed=300 + i, train_frac=0.2, power=0.6, device=dev) for i in range(5)]
        fin, ncls = 128, 5
    model = S.GATModel(fin, 256, ncls, dropout_prob=0.3, edge_mlp_type="GCN", gat_v2=True, **CONFIGS[config]).to(dev)
    return parts, model


def _args(arm, draws):
    a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws)
    if arm == "batched":
        a.sgs_eval_batch, a.sgs_eval_batch_heads, a.sgs_eval_batch_gatv2 = True, ["GAT"], True
    return a


def _summary(rounds):
    flat = [t for r in rounds for t in r]
    meds = [statistics.median(r) for r in rounds]
    return {"median_s": statistics.median(flat), "round_median_min_s": min(meds), "round_median_max_s": max(meds), "passes": len(flat)}


def measure(shape, config, arms, rounds, reps, draws, passes):
    import torch
    import sgs_gnn_amd as S
    EV = sys.modules["sgs_gnn_amd.evaluate"]
    dev = "cuda:0"
    parts, model = _load(shape, config, S, dev, torch)

    def one(arm):
        a = _args(arm, draws)
        S.manual_seed(11)
        torch.cuda.synchronize()
        before = dict(EV.PATH_COUNTS)
        t0 = time.perf_counter()
        f1 = S.ensemble_evaluate(a, model, parts, dev, q=Q, mode="learned")
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        assert EV.PATH_COUNTS[arm] == before[arm] + 1, f"{arm} took the other path"
        return t, f1

    warm = {arm: one(arm)[1] for arm in arms}           # warm-up: allocator growth, library load
    if len(arms) == 2:
        assert warm["serial"] == warm["batched"], f"F1 triples differ: {warm}"
    if passes:
        for _ in range(passes - 1):
            for arm in arms:
                one(arm)
        return {"shape": shape, "config": config, "passes": passes, "arms": {arm: {"f1": warm[arm]} for arm in arms}}
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
    out = {"shape": shape, "head": "GAT (gat_v2)", "config": config, "model": CONFIGS[config], "partitions": len(parts), "draws": draws, "q": Q,
           "mode": "learned", "rounds": rounds, "reps": reps, "edges_sampled_partitions": sum(1 for b in parts if b.edge_index.shape[1] > Q),
           "arms": {arm: {**_summary(times[arm]), "f1": f1[arm]} for arm in arms}, "device": torch.cuda.get_device_name(0)}
    if len(arms) == 2:
        out["f1_equal"] = f1["serial"] == f1["batched"]
        out["serial_over_batched_this_commit"] = out["arms"]["serial"]["median_s"] / out["arms"]["batched"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", type=int, default=11)
    ap.add_argument("--shapes", default="s3,s4")
    ap.add_argument("--configs", default="heads8_edge,heads1")
    ap.add_argument("--path", default="both", choices=ARMS + ("both",))
    ap.add_argument("--passes", type=int, default=0, help="K > 0: K untimed passes per arm and no timing (for a kernel trace)")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package and library are measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [s for s in a.shapes.split(",") if s]
    if any(s not in ("s3", "s4") for s in shapes):
        ap.error("--shapes from s3, s4")
    configs = [c for c in a.configs.split(",") if c]
    if any(c not in CONFIGS for c in configs):
        ap.error(f"--configs from {', '.join(CONFIGS)}")
    arms = list(ARMS) if a.path == "both" else [a.path]
    sys.path.insert(0, os.path.abspath(a.root))
    import sgs_gnn_amd
    assert os.path.abspath(sgs_gnn_amd.__file__).startswith(os.path.abspath(a.root) + os.sep), "the package came from another tree"
    res = {"timer": "host clock around one ensemble_evaluate pass ending in a device synchronise; median of all passes, [min, max] of the "
                    "per-round medians; arms alternating in one process", "root": "this tree" if a.root == os.path.dirname(HERE) else "--root",
           "shapes": {}}
    for shape in shapes:
        res["shapes"][shape] = {c: measure(shape, c, arms, a.rounds, a.reps, a.draws, a.passes) for c in configs}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
