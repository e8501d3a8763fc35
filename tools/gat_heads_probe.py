"""Same-process timing of the two-layer GAT head at bench S4's partition shape, three variants alternating:

    python tools/gat_heads_probe.py [--reps 25] [--heads 8] [--out profiles/r08_gat_heads_probe.json] [--only a|b|c]

Shape: synthetic_graph(33 869, 463 000, 128, 5, seed=300, train_frac=0.2, power=0.6) as bench.py run_s4 builds it, one prior draw of
q = 100 000 edges squeezed out of the parent CSR (ops.get_subgraph), hidden 256, training mode with dropout 0.3.
  (a) heads1    GAT(128, 256, 2, 5)            the existing one-head kernels (what the parent commit measures)
  (b) headsK    GAT(128, 256, 2, 5, heads=K)   the fused per-head kernels
  (c) looped    the construction (b) replaces: K one-head layers of width 256 / K (layer 1: width 5) run one after another on the
                one-head entry points over contiguous column slices of x', concatenated (layer 1: averaged); same parameters as (b)
Each repeat times forward alone (no autograd) and forward + backward (loss = out.square().sum()) with HIP events after a device
synchronise; medians over --reps repeats after 3 untimed rounds.  The subgraph's CSR is built once and shared (it is not part of the
layer).  --only runs one variant (for `rocprofv3 --kernel-trace --stats -- python tools/gat_heads_probe.py --only b --reps 5`)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    a = ap.parse_args()
    import sgs_gnn_amd as S
    from sgs_gnn_amd import model as M
    ops = S.ops
    dev = "cuda:0"
    N, Fin, H, C, q, K, p = 33_869, 128, 256, 5, 100_000, a.heads, 0.3
    b0 = S.synthetic_graph(N, 463_000, Fin, C, seed=300, train_frac=0.2, power=0.6, device=dev)
    smp = ops.sample_topq(ops.SAMPLE_PRIOR, b0.prob, None, 0.0, q, b0.edge_index, seed=1, stream_id=1, want_p=False)
    graph = ops.get_subgraph(b0.edge_index, N, smp)
    ei = smp.edge_index
    torch.manual_seed(0)
    gat1 = M.GAT(Fin, H, 2, C, dropout=p).to(dev).train()
    gatK = M.GAT(Fin, H, 2, C, dropout=p, heads=K).to(dev).train()
    x = b0.x

    def looped(x_in):
        """K one-head layers per GATConv on the one-head entry points, parameters of gatK."""
        seed = M._DropoutClock.next_seed()
        c0, c1 = gatK.convs
        C0 = H // K
        xl = c0.lin_src(x_in)
        outs = []
        for h in range(K):
            xs = xl[:, h * C0:(h + 1) * C0].contiguous()
            a_s, a_d = ops.gat_scores(xs, c0.att_src[0, h], c0.att_dst[0, h])
            outs.append(ops.gat_aggregate(xs, a_s, a_d, c0.bias[h * C0:(h + 1) * C0].contiguous(), graph, 0.2, p, seed, M.SITE_GAT_ATT + 64 * h,
                                          ops.ACT_RELU_DROPOUT, p, seed, M.SITE_GAT_ACT + 64 * h))
        hcat = torch.cat(outs, dim=1)
        xl = c1.lin_src(hcat)
        outs = []
        for h in range(K):
            xs = xl[:, h * C:(h + 1) * C].contiguous()
            a_s, a_d = ops.gat_scores(xs, c1.att_src[0, h], c1.att_dst[0, h])
            outs.append(ops.gat_aggregate(xs, a_s, a_d, None, graph, 0.2, p, seed, M.SITE_GAT_ATT + 64 * h + 2))
        return torch.stack(outs).mean(0) + c1.bias

    variants = {"a": ("heads1", lambda: gat1(x, ei), list(gat1.parameters())),
                "b": (f"heads{K}", lambda: gatK(x, ei), list(gatK.parameters())),
                "c": (f"looped{K}", lambda: looped(x), list(gatK.parameters()))}
    if a.only:
        variants = {a.only: variants[a.only]}
    assert getattr(ei, "_sgs_graph", None) is graph       # every variant reuses the one CSR

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def fwd(f):
        with torch.no_grad():
            f()

    def fwd_bwd(f, params):
        for q_ in params:
            q_.grad = None
        f().square().sum().backward()

    times = {k: {"fwd_ms": [], "fwd_bwd_ms": []} for k in variants}
    for rep in range(3 + a.reps):
        for k, (_, f, params) in variants.items():
            t_f = timed(lambda: fwd(f))
            t_fb = timed(lambda: fwd_bwd(f, params))
            if rep >= 3:
                times[k]["fwd_ms"].append(t_f)
                times[k]["fwd_bwd_ms"].append(t_fb)
    res = {"shape": {"N": N, "Fin": Fin, "hidden": H, "classes": C, "q": q, "heads": K, "dropout": p, "reps": a.reps},
           "timer": "HIP events around one call, device synchronised before; median / min over reps, variants alternating",
           "variants": {}}
    for k, (name, _, _) in variants.items():
        res["variants"][name] = {m: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                 for m, v in times[k].items()}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
