"""Same-process timing of the two-layer GAT head at bench S4's partition shape with GATv2 attention on and off, variants alternating:

    python tools/gat_v2_probe.py [--reps 25] [--out profiles/r12_gat_v2_probe.json] [--only heads8_edge_v2]

Shape: synthetic_graph(33 869, 463 000, 128, 5, seed=300, train_frac=0.2, power=0.6) as bench.py run_s4 builds it, one prior draw of
q = 100 000 edges squeezed out of the parent CSR (ops.get_subgraph), hidden 256, training mode with dropout 0.3; edge weights uniform
in (0, 1), requiring a gradient.  For heads in {1, 8}, with and without the edge term:
  headsK[_edge]_v1        GAT(128, 256, 2, 5, heads=K[, edge_dim=1])              the GATConv kernels (the comparison's base)
  headsK[_edge]_v2        GAT(128, 256, 2, 5, heads=K[, edge_dim=1], v2=True)     the gathering kernels of csrc/gatv2.hip
  headsK[_edge]_composed  the v2 mathematics of the same module composed from device ops (index gathers, element-wise, scatter_reduce,
                          index_add; torch autograd for the backward; torch's own dropout masks): what a user would write without the kernels
Each repeat times forward alone (no autograd) and forward + backward (loss = out.square().sum(), gradients to the parameters and, with
the edge term, to the edge weights) with HIP events after a device synchronise; medians over --reps repeats after 3 untimed rounds.  The
subgraph's CSR is built once and shared (it is not part of the layer).  --only runs one variant (for
`rocprofv3 --kernel-trace --stats -- python tools/gat_v2_probe.py --only heads8_edge_v2 --reps 5`)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def composed_layer(conv, x, src, dst, w, act, p):
    """GATv2Conv.forward from device ops.  src / dst: the entries without (i, i) ones; the loops are appended here."""
    N, K, C = x.shape[0], conv.heads, conv.out_channels
    xl, xr = conv.lin_l(x).view(N, K, C), conv.lin_r(x).view(N, K, C)
    loops = torch.arange(N, device=x.device)
    src_all, dst_all = torch.cat([src, loops]), torch.cat([dst, loops])
    s = xl[src_all] + xr[dst_all]
    if w is not None:
        cnt = torch.zeros(N, device=x.device).index_add_(0, dst, torch.ones_like(w))
        wbar = torch.zeros(N, device=x.device).index_add(0, dst, w) / cnt.clamp(min=1.0)
        s = s + conv.lin_edge(torch.cat([w, wbar]).view(-1, 1)).view(-1, K, C)
    logit = (F.leaky_relu(s, conv.negative_slope) * conv.att).sum(-1)
    idx = dst_all[:, None].expand(-1, K)
    mx = torch.full((N, K), float("-inf"), device=x.device).scatter_reduce(0, idx, logit.detach(), "amax", include_self=True)
    ex = torch.exp(logit - mx[dst_all])
    den = torch.zeros(N, K, device=x.device).index_add(0, dst_all, ex)
    alpha = F.dropout(ex / (den[dst_all] + 1e-16), p=p, training=conv.training)
    out = torch.zeros(N, K, C, device=x.device).index_add(0, dst_all, alpha[:, :, None] * xl[src_all])
    out = (out.reshape(N, K * C) if conv.concat else out.mean(1)) + conv.bias
    if act:
        out = F.dropout(F.relu(out), p=p, training=conv.training)
    return out


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
    nl = ei[0] != ei[1]
    src, dst = ei[0][nl], ei[1][nl]
    variants = {}
    for K in (1, 8):
        for edge in (False, True):
            tag = f"heads{K}{'_edge' if edge else ''}"
            for v2 in (False, True):
                gat = M.GAT(Fin, H, 2, C, dropout=p, heads=K, edge_dim=1 if edge else None, v2=v2).to(dev).train()
                variants[f"{tag}_{'v2' if v2 else 'v1'}"] = (lambda g=gat: g(x, ei, w), list(gat.parameters()))
                if v2:
                    def composed(g=gat, edge=edge):
                        we = w[nl] if edge else None
                        return composed_layer(g.convs[1], composed_layer(g.convs[0], x, src, dst, we, True, p), src, dst, we, False, p)
                    variants[f"{tag}_composed"] = (composed, list(gat.parameters()))
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
            if rep == 0 and "_edge_" in k:
                assert w.grad is not None and float(w.grad.abs().max()) > 0
    res = {"shape": {"N": N, "Fin": Fin, "hidden": H, "classes": C, "q": q, "dropout": p, "reps": a.reps},
           "timer": "HIP events around one call, device synchronised before; median / min over reps, variants alternating",
           "variants": {}, "v2_over_v1": {}, "composed_over_v2": {}}
    for k in variants:
        res["variants"][k] = {m: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                              for m, v in times[k].items()}
    for K in (1, 8):
        for edge in ("", "_edge"):
            tag = f"heads{K}{edge}"
            v1, v2, cp = (res["variants"].get(f"{tag}_{s}") for s in ("v1", "v2", "composed"))
            if v1 and v2:
                res["v2_over_v1"][tag] = {m: round(v2[m]["median"] / v1[m]["median"], 4) for m in ("fwd_ms", "fwd_bwd_ms")}
            if cp and v2:
                res["composed_over_v2"][tag] = {m: round(cp[m]["median"] / v2[m]["median"], 4) for m in ("fwd_ms", "fwd_bwd_ms")}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
