"""Same-process timing of one ChebModel head forward + backward (edge weights requiring grad) at two benchmarked partition shapes:

    python tools/cheb_probe.py --shape s3|s4 [--reps 20] [--rounds 5] [--orders 1,2,3,5] [--out profiles/r09_cheb_probe_s3.json] [--only fused|composed]

Shapes: s3 = bench S3's partition (synthetic_graph(1013, 351 000, 602, 41), 20 % of the candidate edges drawn, hidden 256);
        s4 = bench S4's (synthetic_graph(33 869, 463 000, 128, 5, train_frac=0.2, power=0.6), q = 100 000, hidden 256).
One prior draw (ops.sample_topq) squeezed out of the parent CSR (ops.get_subgraph) gives the directed subgraph; its CSR is built once and
shared.  Edge weights are uniform in [0.05, 0.95] and require grad; dropout 0 so that the variants can be compared.  Per order K:
  (1) fused     ChebModel(cheb_k=K): ops.cheb_norm + ops.cheb_conv (Clenshaw at the output width, sgs_cheb_spmm steps)
  (2) composed  the same mathematics from what exists without csrc/cheb.hip: the Laplacian weights from torch element-wise ops, a
                hand-filled ops.Norm holding l (as ops.mean_norm fills one), ops.gcn_propagate for every L_hat product, torch element-wise
                ops for the three-term recurrence and ops.linear_nobias per order, in the textbook input-width order (same parameters as (1))
  K = 1 is the reference's head (no graph step), for scale.
The logits and the edge-weight gradient of (1) and (2) must agree (else the timing is void: the probe raises); with --fp64 1 (default) both
are also compared against an fp64 evaluation of the head (sparse, over the edge list) and each variant's error against it is reported.  Timing: HIP events around
one forward + backward after a device synchronise, 3 untimed rounds, then `rounds` rounds of `reps` alternating repeats; reported: the median
over all repeats and the min / max of the per-round medians (the yardstick's own spread).  --only runs one variant (for
`rocprofv3 --kernel-trace --stats -- python tools/cheb_probe.py --shape s3 --orders 3 --only fused --rounds 1 --reps 5`)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"s3": dict(N=1013, E=351_000, F=602, H=256, C=41, q=70_200, kw={}),
          "s4": dict(N=33_869, E=463_000, F=128, H=256, C=5, q=100_000, kw=dict(train_frac=0.2, power=0.6))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=tuple(SHAPES), default="s3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--orders", default="1,2,3,5")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("fused", "composed"), default=None)
    ap.add_argument("--fp64", type=int, default=1, help="1 (default): also evaluate the head in fp64 and report each variant's error against it")
    a = ap.parse_args()
    import sgs_gnn_amd as S
    ops = S.ops
    dev = "cuda:0"
    sh = SHAPES[a.shape]
    N, F, H, C, q = sh["N"], sh["F"], sh["H"], sh["C"], sh["q"]
    b0 = S.synthetic_graph(N, sh["E"], F, C, seed=300, device=dev, **sh["kw"])
    smp = ops.sample_topq(ops.SAMPLE_PRIOR, b0.prob, None, 0.0, q, b0.edge_index, seed=1, stream_id=1, want_p=False)
    graph = ops.get_subgraph(b0.edge_index, N, smp)
    ei = smp.edge_index
    n = ei.shape[1]
    batch = S.Batch(x=b0.x, edge_index=ei)
    w = (torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 0.9 + 0.05).requires_grad_()
    src, dst = ei[0], ei[1]
    nonloop = (src != dst).to(torch.float32)
    in_eid, out_eid = graph.in_eid[:n].long(), graph.out_eid[:n].long()
    zeros_n = torch.zeros(N, device=dev)

    def composed(m, K):
        wz = w * nonloop
        deg = torch.zeros(N, device=dev).index_add(0, src, wz)
        dis = torch.where(deg > 0, deg.clamp_min(1e-30).pow(-0.5), torch.zeros_like(deg))
        l = -(dis[src] * wz) * dis[dst]
        nm = ops.Norm()
        nm.graph, nm.w, nm.dis, nm.loopw, nm.what_loop = graph, None, None, None, None
        nm.what_in, nm.what_out = l.detach()[in_eid].contiguous(), l.detach()[out_eid].contiguous()
        nm.handle = torch.cat([l, zeros_n])             # the autograd edge gcn_propagate reports d l to ([n_edges] + [N] loop slots)

        def layer(conv, x):
            t0 = x
            out = ops.linear_nobias(t0, conv.lins[0].weight)
            t1 = ops.gcn_propagate(x, nm)
            out = out + ops.linear_nobias(t1, conv.lins[1].weight)
            for k in range(2, K):
                t2 = 2.0 * ops.gcn_propagate(t1, nm) - t0
                out = out + ops.linear_nobias(t2, conv.lins[k].weight)
                t0, t1 = t1, t2
            return out + conv.bias

        return layer(m.gcn2, torch.relu(layer(m.gcn1, batch.x)))

    def reference64(m, K):
        """The head in fp64 (direct T_k recurrence, L_hat products as index_add over the edge list): logits and d loss / d w."""
        w64 = w.detach().double().requires_grad_()
        wz = w64 * nonloop.double()
        deg = torch.zeros(N, device=dev, dtype=torch.float64).index_add(0, src, wz)
        dis = torch.where(deg > 0, deg.clamp_min(1e-300).pow(-0.5), torch.zeros_like(deg))
        l = -(dis[src] * wz) * dis[dst]

        def lhat(x):
            return torch.zeros_like(x).index_add(0, dst, l[:, None] * x[src])

        def layer(conv, x):
            Ws = [lin.weight.detach().double() for lin in conv.lins]
            t0, t1 = x, lhat(x)
            out = t0 @ Ws[0].t() + t1 @ Ws[1].t()
            for k in range(2, K):
                t0, t1 = t1, 2.0 * lhat(t1) - t0
                out = out + t1 @ Ws[k].t()
            return out + conv.bias.detach().double()

        out = layer(m.gcn2, torch.relu(layer(m.gcn1, batch.x.double())))
        out.square().sum().backward()
        return out.detach(), w64.grad

    def fwd_bwd(f, params):
        for p_ in params:
            p_.grad = None
        w.grad = None
        out = f()
        out.square().sum().backward()
        return out

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    res = {"shape": dict(name=a.shape, N=N, F=F, hidden=H, classes=C, candidate_edges=int(b0.edge_index.shape[1]), drawn_edges=int(n),
                         reps=a.reps, rounds=a.rounds),
           "timer": "HIP events around one forward + backward, device synchronised before; median over all repeats, min / max of the "
                    "per-round medians; variants alternating",
           "orders": {}}
    for K in [int(k) for k in a.orders.split(",")]:
        torch.manual_seed(0)
        m = S.ChebModel(F, H, C, dropout_prob=0.0, edge_mlp_type="GCN", cheb_k=K).to(dev).train()
        params = [p_ for n_, p_ in m.named_parameters() if n_.startswith("gcn")]
        variants = {"fused": lambda m=m: m(batch, ei, w)}
        if K >= 2:
            variants["composed"] = lambda m=m, K=K: composed(m, K)
        agree = None
        if K >= 2 and not a.only:
            o1 = fwd_bwd(variants["fused"], params).detach().clone()
            g1 = w.grad.clone()
            o2 = fwd_bwd(variants["composed"], params).detach()
            g2 = w.grad
            e_o = float((o1 - o2).abs().max()) / (1.0 + float(o2.abs().max()))
            e_g = float((g1 - g2).abs().max()) / (1.0 + float(g2.abs().max()))
            agree = {"logits_rel_err": e_o, "edge_weight_grad_rel_err": e_g}
            if a.fp64:
                o64, g64 = reference64(m, K)
                rel = lambda x, r: float((x.double() - r).abs().max()) / (1.0 + float(r.abs().max()))      # noqa: E731
                agree["vs_fp64"] = {"fused_logits": rel(o1, o64), "composed_logits": rel(o2, o64),
                                    "fused_edge_weight_grad": rel(g1, g64), "composed_edge_weight_grad": rel(g2, g64)}
            # the gate.  Logits: two layers of dot products of at most F = 602 fp32 terms and K sparse steps: 1e-5 relative is ~20 units of
            # eps * sqrt(F) and any wrong term is orders above it.  Edge-weight gradient: the head has a ReLU, so its gradient is not
            # continuous in the arithmetic -- a hidden unit whose pre-activation is within rounding of 0 switches its whole contribution
            # between two evaluation orders -- and a fixed bound would measure the case, not the code: with --fp64 the fused path must be
            # within 1e-5 of fp64 or no more than 4x the composition's OWN fp32 error against fp64 at the same case (two fp32
            # evaluations in different summation orders); without it, within 1e-5 of the composition.
            if a.fp64:
                v = agree["vs_fp64"]
                ok_g = v["fused_edge_weight_grad"] < max(1e-5, 4.0 * v["composed_edge_weight_grad"])
            else:
                ok_g = e_g < 1e-5
            if not (e_o < 1e-5 and ok_g):
                raise SystemExit(f"K = {K}: the fused path and the composition disagree ({agree}): timing void")
        if a.only:
            variants = {k: v for k, v in variants.items() if k == a.only}
        times = {k: [] for k in variants}
        for rnd in range(3 + a.rounds):
            cur = {k: [] for k in variants}
            for _ in range(a.reps if rnd >= 3 else 2):
                for k, f in variants.items():
                    cur[k].append(timed(lambda f=f: fwd_bwd(f, params)))
            if rnd >= 3:
                for k in variants:
                    times[k].append(cur[k])
        entry = {"agreement": agree}
        for k, rounds in times.items():
            meds = [statistics.median(r) for r in rounds]
            entry[k] = {"fwd_bwd_ms": {"median": round(statistics.median([t for r in rounds for t in r]), 4),
                                       "round_median_min": round(min(meds), 4), "round_median_max": round(max(meds), 4)}}
        res["orders"][str(K)] = entry
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
