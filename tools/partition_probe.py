"""The device partitioner on the MI355X: what its kernels and the whole partition_graph cost, and what cut it reaches.

    python tools/partition_probe.py [--parts 64,230] [--cut-frac 0.25] [--rounds 7] [--out profiles/r32_partition_probe.json]

Graph: data.synthetic_partitioned_graph at bench S3's partition shape (n = 1 013 nodes per partition, stored edges per partition from
reddit_partition_sizes, seed 1000) plus cut_frac as many undirected edges again between partitions, node ids shuffled; 4 features (the
partitioner never reads them).  The cut structure is SYNTHETIC (uniform random pairs of nodes of different partitions); no real graph is
measured, and what the partition does to F1 is not measured.

kernels   per-call time of ops.lp_propose, ops.lp_commit and ops.partition_stats ("hip") on the state after grow + fill (hash eligibility,
          mingain 0) against a torch composition of the same sweep on the same device tensors ("torch": index_add_ into an [N, P] table and a
          max for the proposal; sort, searchsorted ranks and index updates for the commit; bincount and a compare-sum for the statistics).
          A host clock around `reps` back-to-back calls ending in a device synchronise, divided by reps; arms alternating; median and
          [min, max] over the rounds after one untimed round.  The arms' results are compared first (equal, or the probe stops).
          propose_floor: one read of col (4 nnz bytes) at the 6.29 TB/s a streaming copy reaches on this chip, over the measured time --
          the part gathers are taken as cache hits (N * 4 bytes fit the L2).  The floor counts ALL of col although a sweep reads only the
          rows of the eligible nodes (about half): against a floor of those rows alone the fraction would be about half as large.
whole     partition_graph end to end at the defaults (host clock, device synchronise at the end; it reads one counter back per growing
          sweep), first call (which builds the CSR; later calls find it cached on the edge_index tensor) and the median of `rounds` more.
cuts      cut fraction (stored entries between parts over E) of the result, of the state after grow + fill, of a hash-random balanced
          partition, of the planted one, and of part[v] = v * P // N on the UNSHUFFLED ids (the planted one again, by construction)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBPS = 6.29


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def _time_arms(arms, rounds, reps):
    t = {n: [] for n in arms}
    for r in range(rounds + 1):
        for n, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            if r:
                t[n].append((time.perf_counter() - t0) / reps * 1e6)
    return {n: _stat(v) for n, v in t.items()}


# ---------------------------------------------------------------- the torch composition of one sweep
def torch_propose(row, col, part, P, elig, mingain):
    N = part.numel()
    p64 = part.to(torch.int64)
    pc = p64[col]
    m = elig[row] & (col != row) & (pc >= 0)
    table = torch.zeros(N * P, dtype=torch.int64, device=part.device)
    table.index_add_(0, (row * P + pc)[m], torch.ones(int(m.sum()), dtype=torch.int64, device=part.device))
    table = table.view(N, P)
    has = p64 >= 0
    own = torch.where(has, table.gather(1, p64.clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros_like(p64))
    table[has.nonzero().flatten(), p64[has]] = 0
    top = (table * P + (P - 1 - torch.arange(P, device=part.device))).max(1).values       # count descending, then part ascending
    cnt, best = top // P, P - 1 - top % P
    gain = cnt - own
    ok = elig & (cnt > 0) & (gain >= mingain)
    return torch.where(ok, best, torch.full_like(best, -1)).to(torch.int32), torch.where(ok, gain, torch.zeros_like(gain)).to(torch.int32)


def _first_per_segment(seg, limit):
    pos = torch.arange(seg.numel(), device=seg.device)
    return (pos - torch.searchsorted(seg, seg)) < limit[seg]


def torch_commit(best, gain, part, size, cap, lo):
    v = (best >= 0).nonzero().flatten()
    b, s0, p0 = best[v].to(torch.int64), size.to(torch.int64), part.to(torch.int64)
    low = (((1 << 20) - 1 - gain[v].to(torch.int64).clamp(0, (1 << 20) - 1)) << 31) | v
    order = torch.argsort((b << 51) | low)
    keep = _first_per_segment(b[order], (cap - s0).clamp(min=0))
    v, low = v[order][keep], low[order][keep]
    src = p0[v]
    free_pass = v[src < 0]
    v, low, src = v[src >= 0], low[src >= 0], src[src >= 0]
    order = torch.argsort((src << 51) | low)
    keep = _first_per_segment(src[order], (s0 - lo).clamp(min=0))
    movers = torch.cat([free_pass, v[order][keep]])
    old = p0[movers]
    part, size = part.clone(), s0.clone()
    size.index_add_(0, old[old >= 0], -torch.ones(int((old >= 0).sum()), dtype=torch.int64, device=part.device))
    size.index_add_(0, best[movers].to(torch.int64), torch.ones(movers.numel(), dtype=torch.int64, device=part.device))
    part[movers] = best[movers]
    return part, size.to(torch.int32), movers.numel()


def torch_stats(row, col, part, P):
    p = part.to(torch.int64)
    return torch.bincount(p[p >= 0], minlength=P), ((col != row) & (p[row] != p[col])).sum()


# ---------------------------------------------------------------- one graph
def probe(S, parts, cut_frac, rounds):
    from sgs_gnn_amd import partition as PT
    dev = "cuda:0"
    ops = S.ops
    sizes = S.reddit_partition_sizes(parts, seed=1000, q=100_000)
    b, planted = S.synthetic_partitioned_graph(parts, 1013, sizes, cut_frac, 4, 41, seed=31, device=dev)
    ei, N, P = b.edge_index, int(b.x.shape[0]), parts
    E = int(ei.shape[1])
    out = {"graph": {"partitions": P, "nodes": N, "edges": E, "mean_degree": E / N}}
    # whole call
    rep = {"trace": []}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    part = S.partition_graph(ei, N, P, report=rep)
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    filled_state = next(p for n, p in rep["trace"] if n == "fill").clone()
    del rep["trace"]
    whole = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = S.partition_graph(ei, N, P)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    assert torch.equal(again, part)
    out["whole"] = {"first_call_s": first, "seconds": _stat(whole), "grow_sweeps": rep["grow_sweeps"], "filled": rep["filled"],
                    "refine_sweeps": len(rep["moved"]), "moved_first_last": [rep["moved"][0], rep["moved"][-1]], "imbalance": rep["imbalance"],
                    "cap": rep["cap"]}
    # cuts
    g = ops.get_graph(ei, N)
    ptr, col32 = g.out_ptr, g.out_dst[:E]
    cut_of = lambda p: int(ops.partition_stats(ptr, col32, p.to(torch.int32).contiguous(), P)[1].item()) / E  # noqa: E731
    hashed = torch.empty(N, dtype=torch.int64, device=dev)
    hashed[torch.sort(PT.node_hash(N, 12345, dev), stable=True).indices] = torch.arange(N, device=dev) * P // N
    out["cuts"] = {"partition_graph": rep["cut_edges"] / E, "after_grow_and_fill": rep["cut_edges_initial"] / E, "hash_random_balanced": cut_of(hashed),
                   "planted": cut_of(planted.to(dev)), "contiguous_blocks_of_unshuffled_ids": cut_of(planted.to(dev)),
                   "note": "contiguous blocks of the unshuffled ids ARE the planted partition in this generator (partition p = ids p n .. (p + 1) n)"}
    # kernels against the torch composition, on the state after grow + fill
    st = filled_state
    size = torch.bincount(st.to(torch.int64), minlength=P).to(torch.int32)
    cap, lo, _ = PT.bounds(N, P, 0.05)
    col = g.out_dst[:E].to(torch.int64)
    row = torch.repeat_interleave(torch.arange(N, device=dev), (ptr[1:] - ptr[:-1]).to(torch.int64))
    key = 7
    elig = (PT.node_hash(N, key, dev) & 1).bool()
    best, gain = ops.lp_propose(ptr, col32, st, P, ops.LP_HASH, key, 0)
    tb, tg = torch_propose(row, col, st, P, elig, 0)
    assert torch.equal(best, tb) and torch.equal(gain, tg), "propose: hip and torch differ"
    p_hip, s_hip = st.clone(), size.clone()
    moved = ops.lp_commit(best, gain, p_hip, s_hip, cap, lo)
    p_t, s_t, m_t = torch_commit(best, gain, st, size, cap, lo)
    assert torch.equal(p_hip, p_t) and torch.equal(s_hip, s_t) and int(moved.item()) == m_t, "commit: hip and torch differ"
    hs, hc = ops.partition_stats(ptr, col32, st, P)
    ts, tc = torch_stats(row, col, st, P)
    assert torch.equal(hs.to(torch.int64), ts) and int(hc.item()) == int(tc.item()), "stats: hip and torch differ"
    bb, gg = torch.empty_like(best), torch.empty_like(gain)

    def commit_hip():
        ops.lp_commit(best, gain, st.clone(), size.clone(), cap, lo)
    k = {"propose": _time_arms({"hip": lambda: ops.lp_propose(ptr, col32, st, P, ops.LP_HASH, key, 0, bb, gg),
                                "torch": lambda: torch_propose(row, col, st, P, elig, 0)}, rounds, 5),
         "commit": _time_arms({"hip": commit_hip, "torch": lambda: torch_commit(best, gain, st, size, cap, lo)}, rounds, 5),
         "stats": _time_arms({"hip": lambda: ops.partition_stats(ptr, col32, st, P), "torch": lambda: torch_stats(row, col, st, P)}, rounds, 5)}
    for name, v in k.items():
        v["torch_over_hip"] = v["torch"]["median"] / v["hip"]["median"]
    floor_us = 4.0 * E / (COPY_TBPS * 1e12) * 1e6
    k["propose_floor"] = {"col_bytes": 4 * E, "floor_us": floor_us, "achieved_fraction": floor_us / k["propose"]["hip"]["median"],
                          "proposals": int((best >= 0).sum()), "eligible": int(elig.sum()), "moved": m_t}
    out["kernels_us_per_call"] = k
    print(json.dumps(out, indent=1), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="64,230")
    ap.add_argument("--cut-frac", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_partition_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("partition_probe: needs the MI355X (there is no CPU timing)")
    import sgs_gnn_amd as S
    res = {"tool": "tools/partition_probe.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cut_frac": a.cut_frac,
           "note": "synthetic cut structure (uniform random pairs between partitions); no real graph measured; the effect of the partition on "
                   "F1 is not measured; the commit's hip arm includes two clones (part, size) that the torch arm makes too",
           "graphs": {}}
    for parts in [int(p) for p in a.parts.split(",")]:
        res["graphs"][f"P={parts}"] = probe(S, parts, a.cut_frac, a.rounds)
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                                      # after every graph: a later one that runs out of time loses nothing
            json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
