"""Same-process A/B of ensemble_evaluate: the serial draw loop vs the batched engine (args.sgs_eval_batch) over bench S3's or S4's stream.

    python tools/eval_ab.py [--reps 3] [--parts 230] [--head GCN] [--stream S3] [--gat-heads K] [--gat-edge-weight] [--cheb-k K]
                            [--out profiles/r04_eval_ab.json]

--stream S3 (default): the 230-partition Reddit-like stream on the device (reddit_partition_stream(num_parts=230, seed=1000), as bench.py
S3 builds it).  --stream S4: bench.py run_s4's partitions, synthetic_graph(33 869, 463 000, 128, 5, seed=300 + i, train_frac=0.2,
power=0.6) for i < --parts (default 5).  --head GCN (default) / GAT / GIN / Cheb picks the model (GNNModel, GATModel, ...) and is the
batched run's args.sgs_eval_batch_heads.  --gat-heads K / --gat-edge-weight (GATModel's gat_heads / gat_edge_weight) and --cheb-k K
(ChebModel's cheb_k) pick the heads' options; the batched run then also sets args.sgs_eval_batch_variants.  H = 256 and the GCN scorer, num_samples_eval = 11, mode 'learned', q = 100 000.  One untimed
pass of each path, then the two alternate; a pass is timed on the host clock around a device synchronise.  Both paths start every pass from the same noise-clock
position, so they draw the same edge sets; the F1 triples are reported as they come out (a near-tie in an argmax can flip a node
between logits that agree to 1e-5), with the node-count difference of every split.  Run it once more under
`rocprofv3 --kernel-trace --stats -- python tools/eval_ab.py --reps 1 --path batched` (and `--path serial`) for launch counts and the
top kernels of one path (its warm-up pass + the timed one)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parts", type=int, default=None, help="partitions (default: 230 for S3, 5 for S4)")
    ap.add_argument("--head", choices=("GCN", "GAT", "GIN", "Cheb"), default="GCN")
    ap.add_argument("--stream", choices=("S3", "S4"), default="S3")
    ap.add_argument("--draws", type=int, default=11)
    ap.add_argument("--gat-heads", type=int, default=1, help="GATModel(gat_heads=K), 1..16 (--head GAT)")
    ap.add_argument("--gat-edge-weight", action="store_true", help="GATModel(gat_edge_weight=True) (--head GAT)")
    ap.add_argument("--cheb-k", type=int, default=1, help="ChebModel(cheb_k=K), 1..8 (--head Cheb)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--path", choices=("both", "serial", "batched"), default="both")
    a = ap.parse_args()
    import sgs_gnn_amd as S
    EV = sys.modules["sgs_gnn_amd.evaluate"]
    dev = "cuda:0"
    torch.manual_seed(0)
    if a.stream == "S3":
        a.parts = 230 if a.parts is None else a.parts
        parts = S.reddit_partition_stream(num_parts=a.parts, seed=1000, device=dev)
        fin, ncls = 602, 41
    else:
        a.parts = 5 if a.parts is None else a.parts
        parts = [S.synthetic_graph(33_869, 463_000, 128, 5, seed=300 + i, train_frac=0.2, power=0.6, device=dev) for i in range(a.parts)]
        fin, ncls = 128, 5
    cls = {"GCN": S.GNNModel, "GAT": S.GATModel, "GIN": S.GINModel, "Cheb": S.ChebModel}[a.head]
    if (a.head != "GAT" and (a.gat_heads != 1 or a.gat_edge_weight)) or (a.head != "Cheb" and a.cheb_k != 1):
        ap.error("--gat-heads / --gat-edge-weight need --head GAT, --cheb-k needs --head Cheb")
    opts = {"GAT": dict(gat_heads=a.gat_heads, gat_edge_weight=a.gat_edge_weight), "Cheb": dict(cheb_k=a.cheb_k)}.get(a.head, {})
    variant = a.gat_heads != 1 or a.gat_edge_weight or a.cheb_k != 1
    model = cls(fin, 256, ncls, dropout_prob=0.3, edge_mlp_type="GCN", **opts).to(dev)

    def one(path):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=a.draws)
        if path == "batched":
            args.sgs_eval_batch, args.sgs_eval_batch_heads = True, [a.head]
            if variant:
                args.sgs_eval_batch_variants = True
        S.manual_seed(11)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        before = dict(EV.PATH_COUNTS)
        f1 = S.ensemble_evaluate(args, model, parts, dev, q=100_000, mode="learned")
        torch.cuda.synchronize()
        assert EV.PATH_COUNTS[path] == before[path] + 1, f"the {path} run took the other path"
        return time.perf_counter() - t0, f1

    paths = ("serial", "batched") if a.path == "both" else (a.path,)
    for path in paths:                                  # warm-up: allocator growth, library load, feature CSRs
        one(path)
    times = {"serial": [], "batched": []}
    f1s = {}
    for _ in range(a.reps):
        for path in paths:
            t, f1 = one(path)
            times[path].append(t)
            f1s[path] = f1
    if a.path != "both":
        print(json.dumps({"path": a.path, "head": a.head, **opts, "stream": a.stream, "seconds": times[a.path], "f1": f1s[a.path]}))
        return
    tm, vm, te = (sum(int(b.train_mask.sum()) for b in parts), sum(int(b.val_mask.sum()) for b in parts), sum(int(b.test_mask.sum()) for b in parts))
    totals = (tm, vm, te)
    res = {"stream": a.stream, "head": a.head, **opts, "partitions": a.parts, "draws": a.draws, "q": 100_000, "mode": "learned", "reps": a.reps,
           "serial_s": times["serial"], "batched_s": times["batched"],
           "serial_median_s": statistics.median(times["serial"]), "batched_median_s": statistics.median(times["batched"]),
           "serial_spread_s": max(times["serial"]) - min(times["serial"]), "batched_spread_s": max(times["batched"]) - min(times["batched"]),
           "speedup": statistics.median(times["serial"]) / statistics.median(times["batched"]),
           "f1_serial": f1s["serial"], "f1_batched": f1s["batched"],
           "node_diff": [round((f1s["batched"][s] - f1s["serial"][s]) * totals[s]) for s in range(3)], "split_totals": totals,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
