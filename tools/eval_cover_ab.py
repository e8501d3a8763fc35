"""ensemble_evaluate under node-covering draws (args.sgs_cover_nodes): the serial draw loop against the batched engine
(args.sgs_eval_batch_cover), alternating in one process, with the no-flag engine beside them.

    python tools/eval_cover_ab.py [--rounds 5] [--reps 5] [--shapes s3,s4] [--parent-root DIR] [--out profiles/r17_eval_cover_ab.json]
    python tools/eval_cover_ab.py --arms serial_cover --root DIR --shapes s3      # one tree's serial loop alone (the yardstick child)
    python tools/eval_cover_ab.py --kernels [--shapes s3,s4]                      # the forced-edge kernels alone, for a kernel trace

Shapes: s3 = bench S3's 230-partition Reddit-like stream (reddit_partition_stream(num_parts=230, seed=1000)) with the GCN head, s4 =
bench S4's five partitions (synthetic_graph(33 869, 463 000, 128, 5, seed=300 + i, train_frac=0.2, power=0.6)) with the GAT head; H = 256,
the GCN scorer, num_samples_eval = 11, mode 'learned', q = 100 000, as tools/eval_ab.py.  Arms: serial_cover (the flag, the serial loop),
engine_cover (the flag and every opt-in: the engine), engine_plain (no flag: the engine on plain draws, context only).  One untimed pass
of every arm, then `rounds` rounds; in a round the arms alternate `reps` times; a pass is timed on the host clock around a device
synchronise; reported: the median of all passes and [min, max] of the per-round medians.  Every pass starts from the same noise-clock
position, so serial_cover and engine_cover draw the same edge sets; their F1 triples are reported as they come out.

The yardstick is the PARENT commit's serial loop under the flag: `--parent-root DIR` (a checkout of the parent with its library built)
runs this file in a child process on that tree, arm serial_cover alone, once before and once after this tree's rounds; both sessions are
reported and the acceptance compares the engine's spread with the union of the two.

--kernels: per shape one representative partition (s3: the partition nearest 351 000 edges; s4: partition 0), q = 100 000, no timing
of its own: per group size G in {1, 2, 4} it issues 20 calls of ops.sample_topq_multi(..., cover=) with D = 11, then 20 x 11 single
ops.sample_topq(..., cover=) calls, so that `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/eval_cover_ab.py
--kernels --shapes s3` lists cover_rows_group<LPR, G> (one dispatch per call) beside cover_rows<LPR> (eleven per round of singles).
--trace-csv s3=DIR,s4=DIR --out FILE.csv turns such traces (one per shape) into the table of the forced-edge and finishing kernels."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ARMS = ("serial_cover", "engine_cover", "engine_plain")


def _load(shape, S, dev, torch):
    torch.manual_seed(0)
    if shape == "s3":
        parts = S.reddit_partition_stream(num_parts=230, seed=1000, device=dev)
        model = S.GNNModel(602, 256, 41, dropout_prob=0.3, edge_mlp_type="GCN").to(dev)
        return parts, model, "GCN"
    parts = [S.synthetic_graph(33_869, 463_000, 128, 5, seed=300 + i, train_frac=0.2, power=0.6, device=dev) for i in range(5)]
    model = S.GATModel(128, 256, 5, dropout_prob=0.3, edge_mlp_type="GCN").to(dev)
    return parts, model, "GAT"


def _args(arm, head, draws):
    a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws)
    if arm != "engine_plain":
        a.sgs_cover_nodes = True
    if arm != "serial_cover":
        a.sgs_eval_batch, a.sgs_eval_batch_heads = True, [head]
    if arm == "engine_cover":
        a.sgs_eval_batch_cover = True
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
    parts, model, head = _load(shape, S, dev, torch)

    def one(arm):
        a = _args(arm, head, draws)
        S.manual_seed(11)
        torch.cuda.synchronize()
        before = dict(EV.PATH_COUNTS)
        t0 = time.perf_counter()
        f1 = S.ensemble_evaluate(a, model, parts, dev, q=100_000, mode="learned")
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        path = "serial" if arm == "serial_cover" else "batched"
        assert EV.PATH_COUNTS[path] == before[path] + 1, f"{arm} took the other path"
        return t, f1

    for arm in arms:                                    # warm-up: allocator growth, library load, feature CSRs
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
    out = {"shape": shape, "head": head, "partitions": len(parts), "draws": draws, "q": 100_000, "mode": "learned", "rounds": rounds, "reps": reps,
           "edges_sampled_partitions": sum(1 for b in parts if b.edge_index.shape[1] > 100_000),
           "arms": {arm: {**_summary(times[arm]), "f1": f1[arm]} for arm in arms}, "device": torch.cuda.get_device_name(0)}
    return out


def kernels(shapes):
    """Issue the forced-edge kernels for a kernel trace (see the module docstring)."""
    import torch
    import sgs_gnn_amd as S
    ops = S.ops
    L = S._lib.lib()
    dev = "cuda:0"
    for shape in shapes:
        if shape == "s3":
            sizes = S.reddit_partition_sizes(230, 1000)
            big = min(range(230), key=lambda i: abs(sizes[i] - 351_000))
            b = S.reddit_partition_stream(num_parts=230, seed=1000, only={big})[big].to(dev)
        else:
            b = S.synthetic_graph(33_869, 463_000, 128, 5, seed=300, train_frac=0.2, power=0.6, device=dev)
        E, N = b.edge_index.shape[1], b.x.shape[0]
        q = 100_000
        p = torch.rand(E, generator=torch.Generator().manual_seed(1)).to(dev)
        g = ops.get_graph(b.edge_index, N)
        print(json.dumps({"shape": shape, "N": N, "E": E, "q": q, "lanes_per_row": L.sgs_sample_topq_cover_variant(N, E)}), flush=True)
        try:
            for G in (1, 2, 4):
                assert L.sgs_sample_topq_multi_cover_group_set(G) == 0
                for i in range(20):
                    ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.3, q, b.edge_index, 11, seed=5, stream_id0=1 + 11 * i, want_w=True, cover=g)
                torch.cuda.synchronize()
        finally:
            L.sgs_sample_topq_multi_cover_group_set(0)
        for i in range(20):
            for d in range(11):
                ops.sample_topq(ops.SAMPLE_LEARNED, p, None, 0.3, q, b.edge_index, seed=5, stream_id=1 + 11 * i + d, want_p=False, cover=g)
        torch.cuda.synchronize()


def trace_csv(spec, out):
    """rocprofv3 kernel traces (shape=DIR, ...) -> kernel, shape, grid_threads, workgroup, dispatches, median_us, min_us, max_us."""
    import csv
    import glob
    import re
    rows_out = []
    for item in spec.split(","):
        shape, d = item.split("=", 1)
        by = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(fn)):
                m = re.search(r"(cover_rows_group|cover_rows|cover_finish|multi_keys_hist0|small_keys_hist0)(<[0-9, ]+>)?", r["Kernel_Name"])
                if not m:
                    continue
                name = m.group(1) + (m.group(2) or "").replace(" ", "")
                grid = int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0) * int(r.get("Grid_Size_Y", 1) or 1)
                by.setdefault((name, grid, int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 0)) or 0)), []).append(
                    (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for (name, grid, wg), us in sorted(by.items()):
            rows_out.append([name, shape, grid, wg, len(us), f"{statistics.median(us):.2f}", f"{min(us):.2f}", f"{max(us):.2f}"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "shape", "grid_threads", "workgroup", "dispatches", "median_us", "min_us", "max_us"])
        w.writerows(rows_out)
    for r in rows_out:
        print(",".join(str(x) for x in r))


def _child(root, shape, rounds, reps, draws):
    """This file on another tree (the parent's checkout), arm serial_cover alone, in a fresh process."""
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--arms", "serial_cover", "--shapes", shape, "--rounds", str(rounds),
           "--reps", str(reps), "--draws", str(draws)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"the yardstick run on {root} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])["shapes"][shape]["arms"]["serial_cover"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=11)
    ap.add_argument("--shapes", default="s3,s4")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package and library are measured")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit (library built): its serial loop is the yardstick")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--trace-csv", default=None, help="shape=DIR,... of rocprofv3 kernel traces of --kernels runs; writes --out as CSV")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_csv:
        if not a.out:
            ap.error("--trace-csv needs --out")
        trace_csv(a.trace_csv, a.out)
        return
    shapes = [s for s in a.shapes.split(",") if s]
    arms = [s for s in a.arms.split(",") if s]
    if any(s not in ("s3", "s4") for s in shapes) or any(s not in ARMS for s in arms):
        ap.error("--shapes from s3, s4; --arms from " + ", ".join(ARMS))
    sys.path.insert(0, os.path.abspath(a.root))
    import sgs_gnn_amd
    assert os.path.abspath(sgs_gnn_amd.__file__).startswith(os.path.abspath(a.root) + os.sep), "the package came from another tree"
    if a.kernels:
        kernels(shapes)
        return
    res = {"timer": "host clock around one ensemble_evaluate pass ending in a device synchronise; median of all passes, [min, max] of the "
                    "per-round medians; arms alternating in one process; parent: the same file on the parent's tree in a child process, "
                    "before and after", "shapes": {}}
    for shape in shapes:
        before = _child(a.parent_root, shape, a.rounds, a.reps, a.draws) if a.parent_root else None
        r = measure(shape, arms, a.rounds, a.reps, a.draws)
        if a.parent_root:
            after = _child(a.parent_root, shape, a.rounds, a.reps, a.draws)
            r["parent_serial_cover"] = {"before": before, "after": after}
            lo = min(before["round_median_min_s"], after["round_median_min_s"])
            hi = max(before["round_median_max_s"], after["round_median_max_s"])
            med = statistics.median([before["median_s"], after["median_s"]])
            r["parent_serial_cover"].update(median_s=med, round_median_min_s=lo, round_median_max_s=hi)
            if "engine_cover" in r["arms"]:
                e = r["arms"]["engine_cover"]
                r["acceptance"] = {"engine_spread_wholly_below_parent_serial_spread": e["round_median_max_s"] < lo,
                                   "parent_serial_over_engine": med / e["median_s"]}
        A = r["arms"]
        if "engine_cover" in A and "serial_cover" in A:
            r["serial_over_engine_this_commit"] = A["serial_cover"]["median_s"] / A["engine_cover"]["median_s"]
        if "engine_cover" in A and "engine_plain" in A:
            r["engine_cover_over_engine_plain"] = A["engine_cover"]["median_s"] / A["engine_plain"]["median_s"]
        res["shapes"][shape] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
