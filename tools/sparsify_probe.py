"""The sparsifier export (sgs_gnn_amd.sparsify) measured on the GPU: its three kernels against the torch composition they replace, one
export beside one batched ensemble evaluation, and inference on the consensus graphs against the ensemble.

    python tools/sparsify_probe.py [--steps kernels,export,quality] [--out profiles/r28_sparsify_probe.json]
    python tools/sparsify_probe.py --step kernels|export|quality [...]          # one step in this process (what the launcher starts)

The launcher opens no GPU: it starts every step as a child process under its own `timeout`, one after the other, and ends at the first
step that does not exit 0 (a fault, an abort or a time limit: nothing more is started on the device).  Each step prints one JSON line; the
launcher merges them into --out.

kernels  At bench S3's partition shape (N = 1 013, C = 41, the stream's partition nearest 351 000 edges) and bench S4's (N = 33 869,
         C = 5, 463 000 edges target), 11 draws of q = 100 000 edges by ops.sample_topq_multi over random scores.  Per stage the library
         call and the torch composition, alternating inside every round in one process (the one that opens a round alternates too), two
         HIP events around `iters` back-to-back calls, microseconds per call; median and [min, max] of the rounds:
           fold    ops.consensus_accum(mask block, hist)            | mask.sum(0, dtype=int32)
           select  ops.consensus_select(count, p, q, edge_index)    | topk(q) of the 64-bit composite (key << 32) | ~id, ids sorted, columns
                                                                     gathered (a full sort of the composite is timed as a third arm)
           pairs   ops.edge_class_counts(edge_index, y, N, C)       | bincount(y[src] * C + y[dst], minlength=C * C)
         The two sides' results are asserted equal before anything is timed.  There is no pass / fail ratio.
export   One sparsify over the S3 stream (230 partitions, 11 draws, learned mode) beside one batched ensemble_evaluate of the same model
         from the same seed, alternating; host clock around a call ending in a device synchronise.
quality  A GCN model trained for `--epochs` epochs on `--parts` partitions of the S3 stream, then on the same partitions: ensemble_evaluate
         (batched, 11 draws), evaluate(mode='full') on sparsify's consensus graphs (top-q, and threshold at min_freq 0.5), and
         evaluate(mode='full') on the original graphs; seconds per evaluation (alternating, median) and the F1 triples.  THE DATA ARE
         SYNTHETIC (data.synthetic_graph: uniform random labels with a weak class signal in the features, edges drawn without regard to
         the labels), so the triples say whether a consensus graph reproduces the ensemble's prediction, not what a sparsifier gains on a
         real graph."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q, D = 100_000, 11
LIMITS = {"kernels": 300, "export": 420, "quality": 420}           # seconds per step


def _events(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def _paired(torch, arms, rounds, iters):
    for fn in arms.values():
        for _ in range(3):
            fn()
    ts, names = {k: [] for k in arms}, list(arms)
    for r in range(rounds):
        for j in range(len(names)):
            k = names[(r + j) % len(names)]
            ts[k].append(_events(torch, arms[k], iters))
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in ts.items()}


def step_kernels(a):
    import torch
    import sgs_gnn_amd as S
    ops, dev = S.ops, "cuda:0"
    sizes = S.reddit_partition_sizes(230, 1000)
    big = min(range(230), key=lambda i: abs(sizes[i] - 351_000))
    shapes = {"s3": (S.reddit_partition_stream(num_parts=230, seed=1000, only={big})[big], 41),
              "s4": (S.synthetic_graph(33_869, 463_000, 128, 5, seed=300, train_frac=0.2, power=0.6), 5)}
    out = {"timer": f"two HIP events around {a.iters} back-to-back calls, microseconds per call (host launch time included); median and "
                    f"[min, max] of {a.rounds} rounds; arms alternating inside a round", "draws": D, "q": Q,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, (b, C) in shapes.items():
        b = b.to(dev)
        ei, y, N = b.edge_index.contiguous(), b.y, b.x.shape[0]
        E = ei.shape[1]
        p = torch.rand(E, generator=torch.Generator().manual_seed(E)).to(dev)
        smp = ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.0, Q, ei, D, seed=5, stream_id0=1, want_edge_index=False)
        mask = smp.mask
        hist = torch.zeros(128, dtype=torch.int64, device=dev)
        count = ops.consensus_accum(smp, hist=hist)
        ids = torch.arange(E, dtype=torch.int64, device=dev)
        inv = (~ids) & 0xFFFFFFFF

        def torch_fold():
            return mask.sum(0, dtype=torch.int32)

        def composite(c):
            key = (c.to(torch.int64) << 25) | (p.view(torch.int32).to(torch.int64) >> 6)
            return (key << 32) | inv

        def torch_select(c=count):
            top = torch.topk(composite(c), Q).values
            sel = torch.sort(~top & 0xFFFFFFFF).values
            return sel, ei[:, sel]

        def torch_sort(c=count):
            top = torch.sort(composite(c), descending=True).values[:Q]
            sel = torch.sort(~top & 0xFFFFFFFF).values
            return sel, ei[:, sel]

        def torch_pairs():
            return torch.bincount(y[ei[0]] * C + y[ei[1]], minlength=C * C)

        r = ops.consensus_select(count, p, Q, ei)
        assert torch.equal(torch_fold(), count), "fold: the two sides disagree"
        assert torch.equal(torch_select()[0], r.eid) and torch.equal(torch_select()[1], r.edge_index), "select: the two sides disagree"
        assert torch.equal(torch_sort()[0], r.eid), "select (sort): the two sides disagree"
        assert torch.equal(torch_pairs().reshape(C, C), ops.edge_class_counts(ei, y, N, C)), "pairs: the two sides disagree"
        pairs = torch.zeros(C, C, dtype=torch.int64, device=dev)
        rec = {"N": N, "C": C, "E": E, "mask_rows_16B_aligned": E % 16 == 0, "edge_class_form": ops.edge_class_variant(E, C),
               "fold": _paired(torch, {"library": lambda: ops.consensus_accum(smp, count, hist=hist), "torch": torch_fold}, a.rounds, a.iters),
               "select": _paired(torch, {"library": lambda: ops.consensus_select(count, p, Q, ei), "torch_topk": torch_select,
                                         "torch_sort": torch_sort}, a.rounds, a.iters),
               "pairs": _paired(torch, {"library": lambda: ops.edge_class_counts(ei, y, N, C, out=pairs), "torch": torch_pairs}, a.rounds,
                                a.iters)}
        for stage, base in (("fold", "torch"), ("select", "torch_topk"), ("pairs", "torch")):
            rec[stage]["torch_over_library"] = round(rec[stage][base]["median_us"] / rec[stage]["library"]["median_us"], 2)
        out["shapes"][name] = rec
    return out


def _s3(S, dev, torch, parts=230):
    torch.manual_seed(0)
    return S.reddit_partition_stream(num_parts=parts, seed=1000, device=dev)


def _host_timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def _alternate(torch, arms, rounds):
    res = {k: None for k in arms}
    for k, fn in arms.items():                              # warm-up: allocator growth, cached CSRs
        fn()
    ts, names = {k: [] for k in arms}, list(arms)
    for r in range(rounds):
        for j in range(len(names)):
            k = names[(r + j) % len(names)]
            t, res[k] = _host_timed(torch, arms[k])
            ts[k].append(t)
    return {k: {"median_s": round(statistics.median(v), 5), "min_s": round(min(v), 5), "max_s": round(max(v), 5)} for k, v in ts.items()}, res


def step_export(a):
    import torch
    import sgs_gnn_amd as S
    dev = "cuda:0"
    parts = _s3(S, dev, torch)
    model = S.GNNModel(602, 256, 41, dropout_prob=0.3, edge_mlp_type="GCN").to(dev)

    def export():
        S.manual_seed(11)
        return S.sparsify(argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=D), model, parts, dev, q=Q, mode="learned")[1]["edges"]

    def ensemble():
        S.manual_seed(11)
        return S.ensemble_evaluate(argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=D, sgs_eval_batch=True), model, parts, dev, q=Q,
                                   mode="learned")

    times, res = _alternate(torch, {"sparsify": export, "ensemble_evaluate_batched": ensemble}, a.rounds)
    return {"timer": "host clock around one call over the stream ending in a device synchronise; the two calls alternating; median and "
                     f"[min, max] of {a.rounds} calls each", "stream": "S3, 230 partitions", "draws": D, "q": Q, "edges": res["sparsify"],
            "sampled_partitions": sum(1 for b in parts if b.edge_index.shape[1] > Q), "times": times, "device": torch.cuda.get_device_name(0)}


def step_quality(a):
    import torch
    import bench
    import sgs_gnn_amd as S
    dev = "cuda:0"
    model, opt_gnn, opt_edge, opt_all = bench.build_model(S, dev, fused=False)       # eager steps, torch's Adam: a short run, nothing captured
    pool = bench.make_pool(S, 0, 1, a.parts, dev)
    targs = bench.make_args(dev, sgs_hipgraph=False)
    crit = torch.nn.CrossEntropyLoss()
    losses = []
    for e in range(a.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            losses.append(float(S.train(targs, e, 10, model, opt_gnn, opt_edge, opt_all, crit, pool, q=bench.Q, alternate_frequency=0)[0]))
    torch.cuda.synchronize()
    ns = lambda **kw: argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=D, **kw)
    S.manual_seed(11)
    kept, rep = S.sparsify(ns(), model, pool, dev, q=Q, mode="learned")
    S.manual_seed(11)
    kept_t, rep_t = S.sparsify(ns(), model, pool, dev, q=Q, mode="learned", rule="threshold", min_freq=0.5)

    def ensemble():
        S.manual_seed(11)
        return S.ensemble_evaluate(ns(sgs_eval_batch=True), model, pool, dev, q=Q, mode="learned")

    arms = {"ensemble_evaluate_batched_11_draws": ensemble,
            "evaluate_full_on_consensus_topq": lambda: S.evaluate(ns(), model, kept, dev, q=Q, mode="full"),
            "evaluate_full_on_consensus_threshold_0.5": lambda: S.evaluate(ns(), model, kept_t, dev, q=Q, mode="full"),
            "evaluate_full_on_original": lambda: S.evaluate(ns(), model, pool, dev, q=Q, mode="full")}
    times, res = _alternate(torch, arms, a.rounds)
    brief = lambda r: {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.items() if k != "class_pairs"}
    return {"data": "SYNTHETIC (data.synthetic_graph: uniform random labels, a weak class signal in the features, edges drawn without regard to "
                    "the labels)", "partitions": len(pool), "epochs": a.epochs, "mean_loss_per_epoch": [round(v, 5) for v in losses], "draws": D,
            "q": Q, "timer": f"host clock around one evaluation of the {len(pool)} partitions ending in a device synchronise; arms alternating; "
                             f"median and [min, max] of {a.rounds}",
            "times": times, "f1_train_val_test": {k: [round(float(x), 6) for x in v] for k, v in res.items()},
            "report_topq": brief(rep), "report_threshold_0.5": brief(rep_t), "device": torch.cuda.get_device_name(0)}


STEPS = {"kernels": step_kernels, "export": step_export, "quality": step_quality}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="kernels,export,quality")
    ap.add_argument("--step", choices=tuple(STEPS), default=None, help="run this one step in this process")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parts", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("sparsify_probe: no GPU visible (timings are taken on the device only)")
        print("RESULT " + json.dumps(STEPS[a.step](a)), flush=True)
        return
    steps = [s for s in a.steps.split(",") if s]
    if any(s not in STEPS for s in steps):
        ap.error(f"--steps from {tuple(STEPS)}")
    res = {}
    for s in steps:                                         # the launcher opens no GPU; the first step that fails ends the run
        cmd = ["timeout", "-k", "10", str(LIMITS[s]), sys.executable, os.path.abspath(__file__), "--step", s, "--rounds", str(a.rounds),
               "--iters", str(a.iters), "--parts", str(a.parts), "--epochs", str(a.epochs)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            res[s] = {"failed": True, "exit_status": r.returncode}
            print(json.dumps({s: res[s]}), flush=True)
            break
        res[s] = json.loads(line[len("RESULT "):])
        print(json.dumps({s: res[s]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if any(v.get("failed") for v in res.values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
