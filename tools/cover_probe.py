"""Same-process timing of one learned draw, plain (sgs_sample_topq) against node-covering (sgs_sample_topq_cover):

    python tools/cover_probe.py [--shapes s3,s4,low] [--reps 30] [--rounds 5] [--out profiles/r15_cover_probe.json]
                                [--only plain|cover] [--root DIR --label parent]

Shapes: s3 / s4 = bench S3's / S4's partition (tools/cheb_probe.py's SHAPES: N = 1 013, E ~ 351 k, long rows; N = 33 869, E ~ 463 k,
short rows), low = a uniform random undirected multigraph of 20 000 nodes and 80 000 pairs, both directions stored (E = 160 000, mean
degree 8), q = 0.2 E.  Scores are sigmoid(N(0, 1)), the prior is the partition's degree prior (uniform on `low`); noise in-register,
a fresh stream id per draw.  Each arm is timed twice:
  eager     HIP events around `--chain` draws issued back to back after a device synchronise, per draw;
  captured  the draw chain of a learned step -- ops.sample_topq + ops.get_subgraph of the drawn edges, `--chain` times with different
            stream ids -- recorded into one HIP graph and replayed, HIP events around the replay, per draw.
3 untimed rounds, then `rounds` rounds of `reps` alternating repeats; reported: the median over all repeats, the min / max of the
per-round medians (the yardstick's own spread) and the ratio cover / plain of the medians.  The covering arm's results are checked
first: keys bitwise the plain draw's, exactly q edges, cover_info == (M, min(M, q)) with M counted from the edge list, every node
with a non-loop in-edge covered when M <= q -- else the timing is void and the probe raises.  On every shape it also records the
fraction of the nodes that have a non-loop in-edge but no drawn one, plain against covering, over 8 draws (a property of the draw, not a
timing).  --only runs one arm (`--only plain --root <a checkout of the parent commit>` is the yardstick on the parent's library;
`rocprofv3 --kernel-trace --stats -- python tools/cover_probe.py --shapes s4 --only cover --rounds 1 --reps 5` gives the kernel split)."""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"s3": dict(N=1013, E=351_000, q=70_200, kw={}),
          "s4": dict(N=33_869, E=463_000, q=100_000, kw=dict(train_frac=0.2, power=0.6)),
          "low": dict(N=20_000, E=160_000, q=32_000, kw=None)}


def _partition(S, name, dev):
    sh = SHAPES[name]
    N = sh["N"]
    if sh["kw"] is not None:
        b = S.synthetic_graph(N, sh["E"], 16, 5, seed=300, device=dev, **sh["kw"])
        return b.edge_index.contiguous(), b.prob.contiguous(), N
    g = torch.Generator().manual_seed(300)
    a = torch.randint(0, N, (sh["E"] // 2,), generator=g)
    b = (a + 1 + torch.randint(0, N - 1, (sh["E"] // 2,), generator=g)) % N
    ei = torch.stack([torch.cat([a, b]), torch.cat([b, a])]).to(dev).contiguous()
    return ei, torch.full((ei.shape[1],), 1.0 / ei.shape[1], device=dev), N


def _uncovered(mask, ei, N):
    real = ei[0] != ei[1]
    has = torch.zeros(N, dtype=torch.bool, device=ei.device)
    has[ei[1][real]] = True
    got = torch.zeros(N, dtype=torch.bool, device=ei.device)
    got[ei[1][real & mask]] = True
    return int((has & ~got).sum()), int(has.sum())


def probe(S, name, a):
    ops = S.ops
    dev = torch.device("cuda:0")
    ei, prior, N = _partition(S, name, dev)
    E, q = int(ei.shape[1]), SHAPES[name]["q"]
    p = torch.sigmoid(torch.randn(E, device=dev, generator=torch.Generator(device=dev).manual_seed(5)))
    graph = ops.get_graph(ei, N)
    arms = [k for k in ("plain", "cover") if not a.only or k == a.only]

    def draw(arm, sid, **kw):
        extra = dict(cover=graph) if arm == "cover" else {}
        return ops.sample_topq(ops.SAMPLE_LEARNED, p, prior, 0.3, q, ei, seed=7, stream_id=sid, **extra, **kw)

    entry = {"shape": dict(name=name, N=N, candidate_edges=E, q=q, chain=a.chain, reps=a.reps, rounds=a.rounds)}
    if "cover" in arms:
        entry["shape"]["lanes_per_row"] = int(S._lib.lib().sgs_sample_topq_cover_variant(N, E))
        tot = {"plain": 0, "cover": 0}
        has = 0
        for d in range(8):
            rp, rc = draw("plain", 100 + d, want_keys=True), draw("cover", 100 + d, want_keys=True)
            torch.cuda.synchronize()
            M = _uncovered(torch.zeros(E, dtype=torch.bool, device=dev), ei, N)[1]
            up, has = _uncovered(rp.mask, ei, N)
            uc, _ = _uncovered(rc.mask, ei, N)
            ok = (torch.equal(rp.keys.view(torch.int32), rc.keys.view(torch.int32)) and int(rc.mask.sum()) == q
                  and rc.cover_info.tolist() == [M, min(M, q)] and (M > q or uc == 0))
            if not ok:
                raise SystemExit(f"{name}: the covering draw is wrong (M={M}, cover_info={rc.cover_info.tolist()}, uncovered={uc}): timing void")
            tot["plain"] += up
            tot["cover"] += uc
        entry["nodes_without_a_drawn_in_edge"] = {"nodes_with_a_non_loop_in_edge": has, "M_le_q": has <= q, "draws": 8,
                                                  "plain_fraction": round(tot["plain"] / (8 * has), 4),
                                                  "cover_fraction": round(tot["cover"] / (8 * has), 4)}

    sid = [1000]

    def chain_eager(arm):
        for _ in range(a.chain):
            sid[0] += 1
            draw(arm, sid[0], want_p=True)

    def chain_graph(arm):
        for i in range(a.chain):
            r = draw(arm, 5000 + i, want_p=True)
            ops.get_subgraph(ei, N, r)

    graphs = {}
    if not a.no_captured:
        ops.pin_workspaces(True)
        side = torch.cuda.Stream()
        for arm in arms:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                chain_graph(arm)                            # warm-up on the capture stream: code objects, scratch arena
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                chain_graph(arm)
            torch.cuda.synchronize()
            graphs[arm] = g

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.chain           # us per draw

    runs = {("eager", k): (lambda k=k: chain_eager(k)) for k in arms}
    runs.update({("captured", k): graphs[k].replay for k in graphs})
    times = {k: [] for k in runs}
    for rnd in range(3 + a.rounds):
        cur = {k: [] for k in runs}
        for _ in range(a.reps if rnd >= 3 else 2):
            for k, fn in runs.items():
                cur[k].append(timed(fn))
        if rnd >= 3:
            for k in runs:
                times[k].append(cur[k])
    med = {}
    for (how, arm), rounds in times.items():
        meds = [statistics.median(r) for r in rounds]
        med[how, arm] = statistics.median([t for r in rounds for t in r])
        entry.setdefault(how, {})[arm] = {"us_per_draw": {"median": round(med[how, arm], 2), "round_median_min": round(min(meds), 2),
                                                          "round_median_max": round(max(meds), 2)}}
    for how in ("eager", "captured"):
        if (how, "plain") in med and (how, "cover") in med:
            entry[how]["ratio_cover_over_plain"] = round(med[how, "cover"] / med[how, "plain"], 4)
    entry["byte_model"] = {"extra_bytes_per_draw": 12 * E + 8 * (N + 1),
                           "note": "4 E gathered key bytes + 8 E of in_src / in_eid + two reads of in_ptr; 4 bytes written and two integer "
                                   "atomics per forced edge on top", "extra_launches": 2}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s3,s4,low")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chain", type=int, default=8, help="draws per timed window / per captured graph")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("plain", "cover"), default=None)
    ap.add_argument("--no-captured", action="store_true")
    ap.add_argument("--label", default="branch", help="recorded in the result: which tree was measured")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package and library are measured")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import sgs_gnn_amd as S
    res = {"timer": "HIP events around `chain` draws (eager: issued back to back; captured: one replay of a HIP graph of `chain` x "
                    "[draw + get_subgraph]), device synchronised before, per draw; median over all repeats, min / max of the per-round "
                    "medians; arms alternating", "tree": a.label, "only": a.only, "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = probe(S, name, a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
