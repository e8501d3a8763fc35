"""Neighbour-sampled batches on the MI355X: what a batch costs to build, against the torch composition, and what an epoch over them costs.

    python tools/neighbor_probe.py [--parts 64] [--cut-frac 0.25] [--rounds 5] [--out profiles/r33_neighbor_probe.json]

Graph: tools/cluster_batch_probe.py's (data.synthetic_partitioned_graph at bench S3's partition shape; a SYNTHETIC cut structure, no real
graph, no F1 measured).  B = 1024 seeds, fan-outs [25, 10] and [10, 5], both subgraph types.

collate   per batch of ResidentGraph.batch ("hip": ops.neighbor_batch) against data.neighbor_collate_torch on the same device tensors
          ("torch"): a host clock around all batches of one epoch's first `--batches` seed lists, ending in a device synchronise, divided by
          the number of batches; arms alternating, median and [min, max] over the rounds after one untimed round.  Launches and read-backs
          per batch: device kernel records and device-to-host copy records of torch.profiler around one batch (or "not measured" with
          the reason).  Mean nodes and edges per batch.  Both arms' batches are compared first.
select    the selection of the widest hop alone (ops.nbr_select on that hop's frontier): device events around `reps` calls, against the
          time to read the frontier's rows once (4 B per stored in-edge id + 8 B of ptr per row) and write the chosen ids, at 6.29 TB/s.
epoch     one eager training epoch (hybrid pipeline, bench.py's model and arguments, q = 100 000) over the neighbour loader
          (resample="epoch", every batch built inside the timed epoch) and over ResidentClusterLoader(regroup="epoch") at the k whose
          batches hold the nearest number of edges, in the same process, arms alternating: steps/s and sampled edges/s."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q = 100_000
B = 1024
FANS = ([25, 10], [10, 5])
HBM_BYTES_PER_S = 6.29e12
FIELDS = ("x", "edge_index", "y", "train_mask", "val_mask", "test_mask", "prob", "eid", "node_ids", "seed_mask")


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def _records(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        if not dev:
            return {"launches": "not measured (the profiler returned no device records)", "read_backs": "not measured"}
        copies = [e for e in dev if "memcpy" in e.name.lower()]
        return {"launches": len(dev) - len(copies), "read_backs": sum(1 for e in copies if "dtoh" in e.name.lower().replace(" ", "")),
                "other_copies": sum(1 for e in copies if "dtoh" not in e.name.lower().replace(" ", ""))}
    except Exception as exc:                                             # noqa: BLE001
        return {"launches": f"not measured ({type(exc).__name__}: {exc})", "read_backs": "not measured"}


def collate_cost(S, rg, rounds, n_batches):
    out = {}
    for fan in FANS:
        for sub in ("induced", "directional"):
            ld = rg.neighbor_loader(fan, B, input_nodes="train", shuffle=True, seed=1, subgraph_type=sub)
            lists = ld.seed_lists(0)[:n_batches]
            keys = [[S.neighbor_stream_key(1, 0, b, h) for h in range(len(fan))] for b in range(len(lists))]
            arms = {"hip": lambda s, k: rg.batch(s, fan, k, sub), "torch": lambda s, k: S.neighbor_collate_torch(rg, s, fan, k, sub)}
            a, b = arms["hip"](lists[0], keys[0]), arms["torch"](lists[0], keys[0])
            for f in FIELDS:
                assert torch.equal(getattr(a, f), getattr(b, f)), (fan, sub, f)
            assert a.hop_nodes == b.hop_nodes
            t = {n: [] for n in arms}
            n_sum = e_sum = 0
            for r in range(rounds + 1):
                for n, fn in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for s, k in zip(lists, keys):
                        bt = fn(s, k)
                        if r == 0 and n == "hip":
                            n_sum, e_sum = n_sum + bt.x.shape[0], e_sum + bt.edge_index.shape[1]
                    torch.cuda.synchronize()
                    if r:
                        t[n].append((time.perf_counter() - t0) / len(lists) * 1e6)
            name = f"fan={fan} {sub}"
            out[name] = {"batches": len(lists), "mean_nodes": n_sum / len(lists), "mean_edges": e_sum / len(lists), "hop_nodes_first_batch": a.hop_nodes,
                         "us_per_batch": {n: _stat(v) for n, v in t.items()},
                         "torch_over_hip": statistics.median(t["torch"]) / statistics.median(t["hip"]),
                         "records_per_batch": {n: _records(lambda fn=fn: fn(lists[0], keys[0])) for n, fn in arms.items()}}
            print(f"[collate] {name}: n = {out[name]['mean_nodes']:.0f}, E_b = {out[name]['mean_edges']:.0f}, " + json.dumps(out[name]["us_per_batch"]),
                  flush=True)
    return out


def select_cost(S, rg, reps=20):
    out = {}
    for fan in FANS:
        b = rg.batch(rg.neighbor_loader(fan, B, seed=1).seed_lists(0)[0], [fan[0]], [S.neighbor_stream_key(1, 0, 0, 0)], "directional")
        seeds = b.node_ids[b.seed_mask]
        front = b.node_ids[~b.seed_mask].to(torch.int32).contiguous()      # the frontier of hop 1
        deg = rg.in_deg_host[front.cpu().long()]
        total = int(deg.clamp(max=fan[1]).sum())
        K = S.neighbor_stream_key(1, 0, 0, 1)
        call = lambda: S.ops.nbr_select(rg.in_ptr, rg.in_eid, rg.num_nodes, front, fan[1], K, total)  # noqa: E731
        call()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / reps)
        nbytes = 4 * int(deg.sum()) + 8 * int(front.numel()) + 4 * total
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        out[f"fan={fan} hop 1"] = {"rows": int(front.numel()), "seeds": int(seeds.numel()), "stored_in_edges": int(deg.sum()), "longest_row": int(deg.max()),
                                   "chosen": total, "us_per_call_two_launches": _stat(times), "one_read_floor_us": floor,
                                   "times_the_floor": statistics.median(times) / floor}
        print(f"[select] fan={fan}: " + json.dumps(out[f"fan={fan} hop 1"]), flush=True)
    return out


class _Counted:
    """a loader that notes min(E_b, q) of every batch it hands out"""

    def __init__(self, loader):
        self.loader, self.edges = loader, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for b in self.loader:
            self.edges.append(min(int(b.edge_index.shape[1]), Q))
            yield b


def epoch_cost(S, rg, parts, rounds, collate):
    import bench
    dev = "cuda:0"
    crit = torch.nn.CrossEntropyLoss()
    out = {}
    for fan, sub in (([10, 5], "induced"), ([10, 5], "directional")):
        target = collate[f"fan={fan} {sub}"]["mean_edges"]
        sizes = {k: statistics.mean(parts.batch_sizes(g)[1] for g in parts.loader(k, regroup="epoch", shuffle=True, seed=1)._draw())
                 for k in (1, 2, 4, 8, 16, 32) if k <= parts.num_parts}
        k = min(sizes, key=lambda kk: abs(sizes[kk] - target))
        arms = {"neighbor_epoch_eager": rg.neighbor_loader(fan, B, input_nodes="train", shuffle=True, seed=1, subgraph_type=sub),
                f"cluster_epoch_eager_k={k}": parts.loader(k, regroup="epoch", shuffle=True, seed=1)}
        state = {n: bench.build_model(S, dev)[:3] + (bench.make_args(dev),) for n in arms}
        t, rate, steps = {n: [] for n in arms}, {n: [] for n in arms}, {}
        for r in range(rounds + 1):
            for n, ld in arms.items():
                m, og, oe, args = state[n]
                counted = _Counted(ld)
                edges = counted.edges
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, _, _, tot = S.train(args, r, rounds + 1, m, og, oe, None, crit, counted, q=Q)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                steps[n] = tot
                if r:
                    t[n].append(dt)
                    rate[n].append(sum(edges) / dt)
        out[f"fan={fan} {sub}"] = {"q": Q, "neighbor_mean_edges": target, "cluster_k": k, "cluster_mean_edges": sizes[k],
                                   "arms": {n: {"steps": steps[n], "seconds": _stat(t[n]), "steps_per_s": _stat([steps[n] / d for d in t[n]]),
                                                "sampled_edges_per_s": _stat(rate[n])} for n in arms}}
        print(f"[epoch] fan={fan} {sub}: " + json.dumps({n: v["steps_per_s"]["median"] for n, v in out[f"fan={fan} {sub}"]["arms"].items()}), flush=True)
        del arms, state
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=64)
    ap.add_argument("--cut-frac", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_neighbor_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbor_probe: needs the MI355X (there is no CPU timing)")
    import sgs_gnn_amd as S
    dev = "cuda:0"
    sizes = S.reddit_partition_sizes(a.parts, seed=1000, q=Q)
    b, part = S.synthetic_partitioned_graph(a.parts, 1013, sizes, a.cut_frac, 602, 41, seed=31, device=dev)
    rg = S.ResidentGraph(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, device=dev, prob=b.prob)
    parts = S.ResidentPartitions(b.x, b.edge_index, b.y, b.train_mask, b.val_mask, b.test_mask, part, num_parts=a.parts, device=dev, prob=b.prob,
                                 keep_cut_edges=True)
    res = {"tool": "tools/neighbor_probe.py", "device": torch.cuda.get_device_name(0),
           "graph": {"partitions": a.parts, "nodes": rg.num_nodes, "features": 602, "edges": rg.num_edges, "longest_in_row": int(rg.in_deg_host.max()),
                     "cut_frac": a.cut_frac, "note": "synthetic cut structure (uniform random pairs between partitions); no real graph, no F1 measured"},
           "batch_size": B, "rounds": a.rounds, "hub_row": S.ops.nbr_select_hub_row()}
    res["collate"] = collate_cost(S, rg, a.rounds, a.batches)
    res["select"] = select_cost(S, rg)
    res["epoch"] = epoch_cost(S, rg, parts, min(a.rounds, 3), res["collate"])
    res["collate_mismatch_word"] = int(rg.collate_mismatch.item())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
