"""Weighted fan-out draws of the neighbour loader on the MI355X: what the weighted selection and a weighted batch cost against the uniform
ones, and what the option does to the edges a batch holds.

    python tools/neighbor_weighted_probe.py [--parts 64] [--cut-frac 0.25] [--rounds 3] [--parent-root DIR]
                                            [--sections select,collate,weights] [--out profiles/r34_neighbor_weighted_probe.json]

Graph and settings: tools/neighbor_probe.py's (data.synthetic_partitioned_graph at bench S3's partition shape; a SYNTHETIC cut structure, no
real graph, no F1 measured; B = 1024 seeds, fan-outs [25, 10] and [10, 5], both subgraph types).  Method: arms alternating, median and
[min, max] over `--rounds` rounds after one untimed round.

select    the selection of the widest hop alone (ops.nbr_select on hop 1's frontier), uniform against weighted (weight="prob" and a
          heavy-tailed random weight with 20 % zeros): device events around `reps` calls.
collate   one batch of ResidentGraph.batch: uniform, weighted ("prob"), and data.neighbor_collate_torch with the same weights on the same
          device tensors: a host clock around the first `--batches` seed lists of an epoch, ending in a device synchronise, per batch.  The
          weighted device batch and the torch composition are compared field by field first.
weights   mean weight of the edges hop 0 chose over the mean weight of the in-edges of its seeds (the candidates), when the draw uses the
          weights and when it is uniform; for weight="prob" and for the random weights: what the option does.
parent    (--parent-root DIR: a checkout of the parent commit with its library built) the uniform arms of `select` and `collate` from DIR
          and from this tree, each in child processes of its own, alternating; the uniform path is meant to be the same code.
`--uniform-only --root DIR` is what those child processes run: the uniform arms alone, with the package imported from DIR."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 100_000
B = 1024
FANS = ([25, 10], [10, 5])
FIELDS = ("x", "edge_index", "y", "train_mask", "val_mask", "test_mask", "prob", "eid", "node_ids", "seed_mask")


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def _alternate(arms, rounds, timed):
    """arms: {name: fn}; timed(fn) -> one figure; one untimed round, then `rounds` rounds with the arms in turn"""
    t = {n: [] for n in arms}
    for r in range(rounds + 1):
        for n, fn in arms.items():
            v = timed(fn)
            if r:
                t[n].append(v)
    return {n: _stat(v) for n, v in t.items()}


def _events(reps):
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    return timed


def _random_weights(rg, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(rg.num_edges, generator=g, dtype=torch.float64) ** 4
    w[torch.rand(rg.num_edges, generator=g) < 0.2] = 0.0
    return w


def select_cost(S, rg, rounds, weights, reps=20):
    out = {}
    for fan in FANS:
        b = rg.batch(rg.neighbor_loader(fan, B, seed=1).seed_lists(0)[0], [fan[0]], [S.neighbor_stream_key(1, 0, 0, 0)], "directional")
        front = b.node_ids[~b.seed_mask].to(torch.int32).contiguous()      # the frontier of hop 1
        deg = rg.in_deg_host[front.cpu().long()]
        total = int(deg.clamp(max=fan[1]).sum())
        K = S.neighbor_stream_key(1, 0, 0, 1)
        arms = {"uniform": lambda: S.ops.nbr_select(rg.in_ptr, rg.in_eid, rg.num_nodes, front, fan[1], K, total)}
        for name, wq in weights.items():
            arms["weighted_" + name] = lambda wq=wq: S.ops.nbr_select(rg.in_ptr, rg.in_eid, rg.num_nodes, front, fan[1], K, total, wq=wq)
        res = {"rows": int(front.numel()), "stored_in_edges": int(deg.sum()), "longest_row": int(deg.max()), "rows_cut": int((deg > fan[1]).sum()),
               "chosen": total, "us_per_call_two_launches": _alternate(arms, rounds, _events(reps))}
        u = res["us_per_call_two_launches"]
        res["weighted_over_uniform"] = {n: u[n]["median"] / u["uniform"]["median"] for n in u if n != "uniform"}
        out[f"fan={fan} hop 1"] = res
        print(f"[select] fan={fan}: " + json.dumps(res), flush=True)
    return out


def collate_cost(S, rg, rounds, n_batches, wq):
    out = {}

    def host_clock(lists, keys):
        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s, k in zip(lists, keys):
                fn(s, k)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / len(lists) * 1e6
        return timed
    for fan in FANS:
        for sub in ("induced", "directional"):
            lists = rg.neighbor_loader(fan, B, input_nodes="train", shuffle=True, seed=1, subgraph_type=sub).seed_lists(0)[:n_batches]
            keys = [[S.neighbor_stream_key(1, 0, b, h) for h in range(len(fan))] for b in range(len(lists))]
            arms = {"hip_uniform": lambda s, k: rg.batch(s, fan, k, sub)}
            if wq is not None:
                arms["hip_weighted"] = lambda s, k: rg.batch(s, fan, k, sub, weight_q=wq)
                arms["torch_weighted"] = lambda s, k: S.neighbor_collate_torch(rg, s, fan, k, sub, weight_q=wq)
                a, b = arms["hip_weighted"](lists[0], keys[0]), arms["torch_weighted"](lists[0], keys[0])
                for f in FIELDS:
                    assert torch.equal(getattr(a, f), getattr(b, f)), (fan, sub, f)
                assert a.hop_nodes == b.hop_nodes
            sizes = {n: [int(v) for v in (fn(lists[0], keys[0]).x.shape[0], fn(lists[0], keys[0]).edge_index.shape[1])] for n, fn in arms.items()
                     if n.startswith("hip")}
            res = {"batches": len(lists), "first_batch_nodes_edges": sizes, "us_per_batch": _alternate(arms, rounds, host_clock(lists, keys))}
            u = res["us_per_batch"]
            if wq is not None:
                res["hip_weighted_over_hip_uniform"] = u["hip_weighted"]["median"] / u["hip_uniform"]["median"]
                res["torch_weighted_over_hip_weighted"] = u["torch_weighted"]["median"] / u["hip_weighted"]["median"]
            out[f"fan={fan} {sub}"] = res
            print(f"[collate] fan={fan} {sub}: " + json.dumps(res), flush=True)
    return out


def weight_ratio(S, rg, n_batches, weights):
    """hop 0 of the first batches, per weight vector {name: (wq, the float weights by edge id)}: the mean weight of the chosen in-edges over
    the mean weight of all in-edges of the seeds, when the draw uses the weights and when it is uniform"""
    out = {}
    for fan in FANS:
        lists = rg.neighbor_loader(fan, B, input_nodes="train", shuffle=True, seed=1).seed_lists(0)[:n_batches]
        acc = {n: {"weighted": [], "uniform": []} for n in weights}
        for b, seeds in enumerate(lists):
            K = [S.neighbor_stream_key(1, 0, b, 0)]
            is_seed = torch.zeros(rg.num_nodes, dtype=torch.bool, device=rg.edge_index.device)
            is_seed[seeds.to(rg.edge_index.device)] = True
            cand = is_seed[rg.edge_index[1]]
            uni = rg.batch(seeds, [fan[0]], K, "directional")                # directional, one hop: the batch's edges are the chosen ones
            for n, (wq, val) in weights.items():
                base = float(val[cand].double().mean())
                acc[n]["weighted"].append(float(val[rg.batch(seeds, [fan[0]], K, "directional", weight_q=wq).eid].double().mean()) / base)
                acc[n]["uniform"].append(float(val[uni.eid].double().mean()) / base)
        out[f"fan={fan[0]} hop 0"] = {n: {k: _stat(v) for k, v in d.items()} for n, d in acc.items()}
        print(f"[weights] fan={fan[0]}: " + json.dumps(out[f"fan={fan[0]} hop 0"]), flush=True)
    return out


def make_graph(S, a):
    dev = "cuda:0"
    sizes = S.reddit_partition_sizes(a.parts, seed=1000, q=Q)
    b, _ = S.synthetic_partitioned_graph(a.parts, 1013, sizes, a.cut_frac, 602, 41, seed=31, device=dev)
    return S.ResidentGraph(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, device=dev, prob=b.prob)


def parent_comparison(a):
    """the uniform arms from this tree and from the parent's, three child processes each, in the order b p p b b p"""
    runs = []
    trees = {"branch": HERE, "parent": a.parent_root}
    for i, (name, root) in enumerate((n, trees[n]) for n in ("branch", "parent", "parent", "branch", "branch", "parent")):
        tmp = a.out + f".{name}{i}.tmp"
        cmd = [sys.executable, os.path.abspath(__file__), "--uniform-only", "--root", root, "--out", tmp, "--parts", str(a.parts), "--cut-frac",
               str(a.cut_frac), "--rounds", str(a.rounds), "--batches", str(a.batches)]
        subprocess.run(cmd, check=True, timeout=600, env={k: v for k, v in os.environ.items() if k != "SGS_LIB_PATH"})
        with open(tmp) as f:
            runs.append({"tree": name, **json.load(f)})
        os.remove(tmp)
    out = {"runs": runs, "verdict": {}}
    for sect, field in (("select", "us_per_call_two_launches"), ("collate", "us_per_batch")):
        for case in runs[0][sect]:
            arm = "uniform" if sect == "select" else "hip_uniform"
            med = {t: [r[sect][case][field][arm]["median"] for r in runs if r["tree"] == t] for t in ("branch", "parent")}
            lo = min(r[sect][case][field][arm]["min"] for r in runs if r["tree"] == "parent")
            hi = max(r[sect][case][field][arm]["max"] for r in runs if r["tree"] == "parent")
            excess = statistics.mean(med["branch"]) - statistics.mean(med["parent"])
            out["verdict"][f"{sect} {case}"] = {"branch_medians_us": med["branch"], "parent_medians_us": med["parent"], "parent_spread_us": hi - lo,
                                                "branch_minus_parent_us": excess, "within_parent_spread": excess <= hi - lo}
    print("[parent] " + json.dumps(out["verdict"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=64)
    ap.add_argument("--cut-frac", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--sections", default="select,collate,weights", help="of the full run: a comma-separated subset of select, collate, weights")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r34_neighbor_weighted_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbor_weighted_probe: needs the MI355X (there is no CPU timing)")
    sys.path.insert(0, a.root)
    import sgs_gnn_amd as S
    assert os.path.abspath(os.path.dirname(S.__file__)).startswith(os.path.abspath(a.root)), (S.__file__, a.root)
    rg = make_graph(S, a)
    res = {"tool": "tools/neighbor_weighted_probe.py", "device": torch.cuda.get_device_name(0),
           "graph": {"partitions": a.parts, "nodes": rg.num_nodes, "features": 602, "edges": rg.num_edges, "longest_in_row": int(rg.in_deg_host.max()),
                     "cut_frac": a.cut_frac, "note": "synthetic cut structure (uniform random pairs between partitions); no real graph, no F1 measured"},
           "batch_size": B, "rounds": a.rounds, "hub_row": S.ops.nbr_select_hub_row()}
    if a.uniform_only:
        res["select"] = select_cost(S, rg, a.rounds, {})
        res["collate"] = collate_cost(S, rg, a.rounds, a.batches, None)
    else:
        wq_prob, w_rand = rg.neighbor_weights("prob"), _random_weights(rg, 7)
        wq_rand = rg.neighbor_weights(w_rand)
        sections = a.sections.split(",")
        if "select" in sections:
            res["select"] = select_cost(S, rg, a.rounds, {"prob": wq_prob, "random_20pct_zero": wq_rand})
        if "collate" in sections:
            res["collate"] = collate_cost(S, rg, a.rounds, a.batches, wq_prob)
        if "weights" in sections:
            res["weights"] = weight_ratio(S, rg, a.batches, {"prob": (wq_prob, rg.prob),
                                                             "random_20pct_zero": (wq_rand, w_rand.to(rg.edge_index.device)[rg.edge_order])})
            res["weights"]["prior_max_over_min"] = float(rg.prob.max() / rg.prob.min())
        if a.parent_root:
            res["uniform_against_parent"] = parent_comparison(a)
    res["collate_mismatch_word"] = int(rg.collate_mismatch.item())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
