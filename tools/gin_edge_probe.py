"""Same-process timing of one GINModel head forward + backward (edge weights requiring grad) at two benchmarked partition shapes:

    python tools/gin_edge_probe.py [--shapes s3,s4] [--reps 20] [--rounds 5] [--out profiles/r13_gin_edge_probe.json] [--only plain|fused|composed]

Shapes are tools/cheb_probe.py's SHAPES (s3 = bench S3's partition, s4 = bench S4's): one prior draw (ops.sample_topq) squeezed out of the
parent CSR (ops.get_subgraph) gives the directed subgraph; its CSR is built once and shared.  Edge weights are uniform in [0.05, 0.95]
and require grad; dropout 0 so that the arms can be compared.  Three arms:
  (a) plain     GINModel(gin_edge_weight=False): today's head (one SpMM per layer at the hidden width; the weights are dropped), for scale
  (b) fused     GINModel(gin_edge_weight=True): ops.gine_aggregate (csrc/gine.hip) + the layer's two Linears
  (c) composed  the same mathematics as (b), same parameters, from x[src], element-wise ops, index_add_ and nn.Linear on the GPU
The logits and the edge-weight gradient of (b) and (c) must agree -- forward < 1e-5, gradient < 1e-4, max-abs error over max-abs
reference, the bounds of tests/test_gpu_gine.py -- else the timing is void and the probe raises.  (Both are fp32 and (c) adds with
atomics in no fixed order, so (c) is a yardstick here, not a reference: the fp64 comparison is the test suite's.)  As in the tests, the
comparison needs inputs on which two fp32 evaluations take the same ReLU branch: a message's pre-activation within rounding of zero
switches a whole gradient term between them.  So, before anything is timed, the columns (a[c], b[c]) of each layer's lin that put a
pre-activation within 1e-5 (1 + |x_j[c]|) of zero are redrawn from Linear's own range until none is left (a condition on the inputs;
the second layer's input is the fused first layer's output).  Timing: HIP events
around one forward + backward after a device synchronise, 3 untimed rounds, then `rounds` rounds of `reps` alternating repeats; reported:
the median over all repeats and the min / max of the per-round medians (the yardstick's own spread), and the ratios fused / composed and
fused / plain of the medians.  --only runs one arm (for `rocprofv3 --kernel-trace --stats -- python tools/gin_edge_probe.py --shapes s3
--only fused --rounds 1 --reps 5`)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cheb_probe import SHAPES  # noqa: E402


def probe(S, name, a):
    ops = S.ops
    dev = "cuda:0"
    sh = SHAPES[name]
    N, F, H, C, q = sh["N"], sh["F"], sh["H"], sh["C"], sh["q"]
    b0 = S.synthetic_graph(N, sh["E"], F, C, seed=300, device=dev, **sh["kw"])
    smp = ops.sample_topq(ops.SAMPLE_PRIOR, b0.prob, None, 0.0, q, b0.edge_index, seed=1, stream_id=1, want_p=False)
    ops.get_subgraph(b0.edge_index, N, smp)
    ei = smp.edge_index
    n = ei.shape[1]
    batch = S.Batch(x=b0.x, edge_index=ei)
    w = (torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 0.9 + 0.05).requires_grad_()
    src, dst = ei[0], ei[1]
    torch.manual_seed(0)
    plain = S.GINModel(F, H, C, dropout_prob=0.0, edge_mlp_type="GCN").to(dev).train()
    torch.manual_seed(0)
    fused = S.GINModel(F, H, C, dropout_prob=0.0, edge_mlp_type="GCN", gin_edge_weight=True).to(dev).train()

    def condition(conv, x):
        a_, b_ = conv.lin.weight.data[:, 0], conv.lin.bias.data
        xs, wv = x[src], w.detach()[:, None]
        for _ in range(200):
            bad = ((xs + (wv * a_ + b_)).abs() <= 1e-5 * (1.0 + xs.abs())).any(0)
            k = int(bad.sum())
            if k == 0:
                return
            a_[bad] = torch.rand(k, device=dev) * 2 - 1
            b_[bad] = torch.rand(k, device=dev) * 2 - 1
        raise SystemExit(f"{name}: could not condition the inputs")

    with torch.no_grad():
        condition(fused.GIN.convs[0], batch.x)
        condition(fused.GIN.convs[1], torch.relu(fused.GIN.convs[0](batch.x, ei, w.detach())))

    def composed():
        def layer(conv, x):
            msg = torch.relu(x[src] + (w[:, None] * conv.lin.weight[:, 0] + conv.lin.bias))
            z = (1.0 + conv._eps) * x
            z = z.index_add(0, dst, msg)
            l0, l1 = conv.nn.lins
            return l1(torch.relu(l0(z)))
        c0, c1 = fused.GIN.convs
        return layer(c1, torch.relu(layer(c0, batch.x)))

    arms = {"plain": (lambda: plain(batch, ei, w), [p for k, p in plain.named_parameters() if k.startswith("GIN.")]),
            "fused": (lambda: fused(batch, ei, w), [p for k, p in fused.named_parameters() if k.startswith("GIN.")]),
            "composed": (composed, [p for k, p in fused.named_parameters() if k.startswith("GIN.")])}

    def fwd_bwd(arm):
        f, params = arms[arm]
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

    entry = {"shape": dict(name=name, N=N, F=F, hidden=H, classes=C, candidate_edges=int(b0.edge_index.shape[1]), drawn_edges=int(n),
                           reps=a.reps, rounds=a.rounds)}
    if not a.only:
        rel = lambda x, r: float((x - r).abs().max()) / float(r.abs().max())      # noqa: E731
        o1 = fwd_bwd("fused").detach().clone()
        g1 = w.grad.clone()
        o2 = fwd_bwd("composed").detach()
        g2 = w.grad
        entry["agreement"] = agree = {"logits_rel_err": rel(o1, o2), "edge_weight_grad_rel_err": rel(g1, g2)}
        if not (agree["logits_rel_err"] < 1e-5 and agree["edge_weight_grad_rel_err"] < 1e-4):
            raise SystemExit(f"{name}: the fused head and the composition disagree ({agree}): timing void")
    run = [k for k in arms if not a.only or k == a.only]
    times = {k: [] for k in run}
    for rnd in range(3 + a.rounds):
        cur = {k: [] for k in run}
        for _ in range(a.reps if rnd >= 3 else 2):
            for k in run:
                cur[k].append(timed(lambda k=k: fwd_bwd(k)))
        if rnd >= 3:
            for k in run:
                times[k].append(cur[k])
    med = {}
    for k, rounds in times.items():
        meds = [statistics.median(r) for r in rounds]
        med[k] = statistics.median([t for r in rounds for t in r])
        entry[k] = {"fwd_bwd_ms": {"median": round(med[k], 4), "round_median_min": round(min(meds), 4), "round_median_max": round(max(meds), 4)}}
    if not a.only:
        entry["ratio_fused_over_composed"] = round(med["fused"] / med["composed"], 4)
        entry["ratio_fused_over_plain"] = round(med["fused"] / med["plain"], 4)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s3,s4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("plain", "fused", "composed"), default=None)
    a = ap.parse_args()
    import sgs_gnn_amd as S
    res = {"timer": "HIP events around one forward + backward, device synchronised before; median over all repeats, min / max of the "
                    "per-round medians; arms alternating", "shapes": {}}
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
