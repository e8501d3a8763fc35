"""Multi-partition batches on the MI355X: what a batch costs to build and what an epoch over them costs.

    python tools/cluster_batch_probe.py [--parts 64] [--cut-frac 0.25] [--rounds 5] [--out profiles/r31_cluster_batch_probe.json]
                                        [--collate-only --root DIR]

Graph: data.synthetic_partitioned_graph of `--parts` partitions at bench S3's partition shape (n = 1 013, F = 602, 41 classes, stored
edges per partition from reddit_partition_sizes, seed 1000) plus cut_frac as many undirected edges again between partitions.  The cut
structure is SYNTHETIC (uniform random pairs of nodes of different partitions); no real graph is measured and no F1 is reported.

collate   time per batch of ops.cluster_collate ("hip") against data.collate_torch on the same device tensors ("torch": the composition
          a user would otherwise write -- arange / repeat_interleave / gather / boolean mask), k in {2, 4, 8}: a host clock around
          all batches of one shuffled grouping, ending in a device synchronise, divided by the number of batches; arms alternating,
          median and [min, max] over the rounds after one untimed round.  Launches per batch: device kernel records of
          torch.profiler around one batch (or "not measured" with the reason).  Both arms' batches are compared first.
epoch     one training epoch (hybrid pipeline, GCN head, bench.py's model and arguments) for k in {1, 2, 4, 8} with q = k * 100 000:
          `fixed` loader replayed from captured HIP graphs, `fixed` eager, `epoch` (regrouped every epoch, every batch built by
          ops.cluster_collate inside the timed epoch) eager; for k = 1 also the plain ResidentPartitions under replay (the code path
          that exists without this loader).  An arm whose batches exceed what the captured step accepts is recorded as not run.
          Two untimed epochs per arm, then the arms alternate for `rounds` epochs each.  Per arm: steps/s, sampled edges/s (sum
          over the epoch's batches of min(E_b, q), over the epoch's time) and the share of the graph's edges the epoch sees
          (1 - dropped / E).
`--collate-only --root DIR`: the "hip" arm of `collate` alone, with the package imported from DIR (a checkout of another commit with its
library built); tools/batch_rows_ab.py runs this tree and the parent's that way, in child processes of their own."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 100_000
REPLAY_MAX_EDGES = 2_097_152      # the captured step's sampler reads its edge count from a device word up to this capacity (csrc/sampler.hip)


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def _launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n if n > 0 else "not measured (the profiler returned no device records)"
    except Exception as exc:                                             # noqa: BLE001
        return f"not measured ({type(exc).__name__}: {exc})"


def collate_cost(S, parts, rounds, hip_only=False):
    from sgs_gnn_amd.data import collate_torch
    out = {}
    for k in (2, 4, 8):
        groups = parts.loader(k, regroup="epoch", shuffle=True, seed=k)._draw()
        arms = {"hip": lambda g: S.ops.cluster_collate(parts, g), "torch": lambda g: collate_torch(parts, g)}
        if hip_only:
            del arms["torch"]
        for g in groups[:0 if hip_only else 2]:
            a, b = arms["hip"](g), arms["torch"](g)
            for key in ("x", "edge_index", "y", "train_mask", "val_mask", "test_mask", "prob", "node_ids"):
                assert torch.equal(getattr(a, key), getattr(b, key)), (k, g, key)
        t = {n: [] for n in arms}
        for r in range(rounds + 1):
            for n, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for g in groups:
                    fn(g)
                torch.cuda.synchronize()
                if r:
                    t[n].append((time.perf_counter() - t0) / len(groups) * 1e6)
        b0 = arms["hip"](groups[0])
        out[f"k={k}"] = {"batches": len(groups), "nodes_first_batch": int(b0.x.shape[0]), "edges_first_batch": int(b0.edge_index.shape[1]),
                         "us_per_batch": {n: _stat(v) for n, v in t.items()}}
        if not hip_only:
            out[f"k={k}"].update(torch_over_hip=statistics.median(t["torch"]) / statistics.median(t["hip"]),
                                 launches_per_batch={n: _launches(lambda fn=fn: fn(groups[0])) for n, fn in arms.items()})
        print(f"[collate] k={k}: " + json.dumps(out[f"k={k}"]["us_per_batch"]), flush=True)
    return out


def epoch_cost(S, parts, rounds):
    import bench
    dev = "cuda:0"
    crit = torch.nn.CrossEntropyLoss()
    out = {}
    for k in (1, 2, 4, 8):
        q = Q * k
        arms = {"fixed_hipgraph": (parts.loader(k, shuffle=True, seed=1), True), "fixed_eager": (parts.loader(k, shuffle=True, seed=1), False),
                "epoch_eager": (parts.loader(k, regroup="epoch", shuffle=True, seed=1), False)}
        if k == 1:
            arms["resident_partitions_hipgraph"] = (parts, True)
        skipped = {}
        largest = max(int(b.edge_index.shape[1]) for b in arms["fixed_hipgraph"][0].batches)
        if largest > REPLAY_MAX_EDGES:
            skipped["fixed_hipgraph"] = (f"not run: the largest batch holds {largest} edges, above the {REPLAY_MAX_EDGES} candidate edges the captured "
                                         "step's sampler accepts (sgs_sample_topq under sgs_dyn_edges_set refuses the capture)")
            del arms["fixed_hipgraph"]
        state = {}
        for n, (ld, graph) in arms.items():
            m, og, oe, _ = bench.build_model(S, dev)
            state[n] = (m, og, oe, bench.make_args(dev, sgs_hipgraph=graph))
        t, rate, seen = {n: [] for n in arms}, {n: [] for n in arms}, {}
        for r in range(rounds + 2):
            for n, (ld, _) in arms.items():
                m, og, oe, args = state[n]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, _, _, tot = S.train(args, r, rounds + 2, m, og, oe, None, crit, ld, q=q)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                # edges per batch of THIS epoch from the host tables (an `epoch` loader has drawn new groups)
                sizes = [parts.batch_sizes(g)[1] for g in ld.groups] if hasattr(ld, "groups") else [int(b.edge_index.shape[1]) for b in ld.batches]
                if r >= 2:
                    t[n].append(dt)
                    rate[n].append(sum(min(e, q) for e in sizes) / dt)
                seen[n] = (tot, ld.dropped_edges)
        res = {}
        for n in arms:
            tot, dropped = seen[n]
            res[n] = {"steps": tot, "seconds": _stat(t[n]), "steps_per_s": _stat([tot / d for d in t[n]]),
                      "sampled_edges_per_s": _stat(rate[n]), "edge_share_seen": 1.0 - dropped / parts.num_edges}
            print(f"[epoch] k={k} {n}: {res[n]['steps_per_s']['median']:.1f} steps/s, {res[n]['sampled_edges_per_s']['median'] / 1e6:.1f} M sampled "
                  f"edges/s, share {res[n]['edge_share_seen']:.4f}", flush=True)
        res.update(skipped)
        out[f"k={k}"] = {"q": q, "largest_batch_edges": largest, "arms": res}
        del arms, state
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=64)
    ap.add_argument("--cut-frac", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_cluster_batch_probe.json"))
    ap.add_argument("--bench-ab", default=None, help="a JSON file of bench.py results (parent / branch) to embed as `bench_ab`")
    ap.add_argument("--collate-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_batch_probe: needs the MI355X (there is no CPU timing)")
    sys.path[:0] = [a.root, ROOT]
    import sgs_gnn_amd as S
    assert os.path.abspath(os.path.dirname(S.__file__)).startswith(os.path.abspath(a.root)), (S.__file__, a.root)
    dev = "cuda:0"
    sizes = S.reddit_partition_sizes(a.parts, seed=1000, q=Q)
    b, part = S.synthetic_partitioned_graph(a.parts, 1013, sizes, a.cut_frac, 602, 41, seed=31, device=dev)
    parts = S.ResidentPartitions(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, part, num_parts=a.parts, device=dev, prob=b.prob,
                                 keep_cut_edges=True)
    E = int(b.edge_index.shape[1])
    res = {"tool": "tools/cluster_batch_probe.py", "device": torch.cuda.get_device_name(0),
           "graph": {"partitions": a.parts, "nodes": int(b.x.shape[0]), "features": 602, "edges": E, "cut_edges": parts.dropped_edges,
                     "cut_share": parts.dropped_edges / E, "cut_frac": a.cut_frac,
                     "note": "synthetic cut structure (uniform random pairs between partitions); no real graph, no F1 measured"},
           "rounds": a.rounds, "collate": collate_cost(S, parts, max(a.rounds, 7), a.collate_only)}
    if not a.collate_only:
        res["epoch"] = epoch_cost(S, parts, a.rounds)
    res["collate_mismatch_word"] = int(parts.collate_mismatch.item())
    if a.bench_ab and os.path.exists(a.bench_ab):
        res["bench_ab"] = json.load(open(a.bench_ab))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
