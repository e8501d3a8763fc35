"""Same-process timing of the two-layer GAT head at bench S4's partition shape with and without the edge term, variants alternating:

    python tools/gat_edge_probe.py [--reps 25] [--out profiles/r10_gat_edge_probe.json] [--only heads8_on]

Shape: synthetic_graph(33 869, 463 000, 128, 5, seed=300, train_frac=0.2, power=0.6) as bench.py run_s4 builds it, one prior draw of
q = 100 000 edges squeezed out of the parent CSR (ops.get_subgraph), hidden 256, training mode with dropout 0.3; edge weights uniform
in (0, 1), requiring a gradient.  For heads in {1, 8}:
  headsK_off  GAT(128, 256, 2, 5, heads=K)              edge_weight dropped: the parent commit's code path (the comparison's base)
  headsK_on   GAT(128, 256, 2, 5, heads=K, edge_dim=1)  edge_weight in both layers' attention logits (gat_alpha_heads_edge_*)
Each repeat times forward alone (no autograd) and forward + backward (loss = out.square().sum(), gradients to the parameters and, for
`on`, to the edge weights) with HIP events after a device synchronise; medians over --reps repeats after 3 untimed rounds.  The
subgraph's CSR is built once and shared (it is not part of the layer).  --only runs one variant (for
`rocprofv3 --kernel-trace --stats -- python tools/gat_edge_probe.py --only heads8_on --reps 5`)."""
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import sgs_gnn_amd as S
    from sgs_gnn_amd import model as M
    ops = S.ops
    dev = "cuda:0"
    N, Fin, H, C, q, p = 33_869, 128, 256, 5, 100_000, 0.3
    b0 = S.synthetic_graph(N, 463_000, Fin, C, seed=300, train_frac=0.2, power=0.6, device=dev)
    smp = ops.sample_topq(ops.SAMPLE_PRIOR, b0.prob, None, 0.0, q, b0.edge_index, seed=1, stream_id=1, want_p=False)
    graph = ops.get_subgraph(b0.edge_index, N, smp)
    ei = smp.edge_index
    x = b0.x
    torch.manual_seed(0)
    w = torch.rand(q, device=dev).requires_grad_(True)
    variants = {}
    for K in (1, 8):
        for on in (False, True):
            gat = M.GAT(Fin, H, 2, C, dropout=p, heads=K, edge_dim=1 if on else None).to(dev).train()
            variants[f"heads{K}_{'on' if on else 'off'}"] = (lambda g=gat: g(x, ei, w), list(gat.parameters()))
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
        w.grad = None
        f().square().sum().backward()

    times = {k: {"fwd_ms": [], "fwd_bwd_ms": []} for k in variants}
    for rep in range(3 + a.reps):
        for k, (f, params) in variants.items():
            t_f = timed(lambda: fwd(f))
            t_fb = timed(lambda: fwd_bwd(f, params))
            if rep >= 3:
                times[k]["fwd_ms"].append(t_f)
                times[k]["fwd_bwd_ms"].append(t_fb)
            if rep == 0 and k.endswith("_on"):
                assert w.grad is not None and float(w.grad.abs().max()) > 0
    res = {"shape": {"N": N, "Fin": Fin, "hidden": H, "classes": C, "q": q, "dropout": p, "reps": a.reps},
           "timer": "HIP events around one call, device synchronised before; median / min over reps, variants alternating",
           "variants": {}, "on_over_off": {}}
    for k in variants:
        res["variants"][k] = {m: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                              for m, v in times[k].items()}
    for K in (1, 8):
        on, off = res["variants"].get(f"heads{K}_on"), res["variants"].get(f"heads{K}_off")
        if on and off:
            res["on_over_off"][f"heads{K}"] = {m: round(on[m]["median"] / off[m]["median"], 4) for m in ("fwd_ms", "fwd_bwd_ms")}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
