"""Bitwise and launch-for-launch A/B of the edge scorer's autograd glue (ops.py from the path switches to edge_score_epd, and
torch_ops.edge_score_backward) between two checkouts that load the same built library (SGS_LIB_PATH).

    python tools/scorer_glue_ab.py --root CHECKOUT --out FILE.pt    one process per checkout: the scores and every gradient of
                                                                    ops.edge_score on each of its forward / backward forms, of
                                                                    ops.edge_score_epd, of torch.ops.sgs.edge_score and of one eager
                                                                    and one graph-replayed hybrid training step, written to FILE.pt
    python tools/scorer_glue_ab.py --compare A.pt B.pt              arrays compared with torch.equal; prints one JSON line
    python tools/scorer_glue_ab.py --compare-traces DIR_A DIR_B     the ordered (kernel, grid, workgroup, LDS bytes) lists of one
                                                                    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
                                                                    tools/scorer_glue_ab.py --root ... --out ...` run per checkout

The two comparing halves and the training steps are tools/layer_ops_ab.py's.  Same seeds in every run; nothing is timed here."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_ops_ab as AB  # noqa: E402

DEV = AB.DEV


def edges(N, E, gen, row_sorted=False, undirected=False):
    if undirected:                                  # E / 2 distinct pairs u < v, stored both ways, coalesced
        keys = torch.randperm(N * N, generator=gen)
        u, v = keys // N, keys % N
        keep = (u < v).nonzero().flatten()[:E // 2]
        u, v = u[keep], v[keep]
        src, dst = torch.cat([u, v]), torch.cat([v, u])
        order = torch.argsort(src * N + dst)
        return torch.stack([src[order], dst[order]])
    src, dst = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    if row_sorted:
        src = torch.sort(src).values
    return torch.stack([src, dst])


def scorer_case(S, out, key, N, H, E, n_active=None, shuffled=False, row_sorted=False, undirected=False, build_pairs=False, precision=None,
                switches=(), codes_grad=True, defer=False, epd=False, torch_op=False, p=0.3):
    ops = S.ops
    g = torch.Generator().manual_seed(11)
    ei = edges(N, E, g, row_sorted, undirected).to(DEV)
    E = ei.shape[1]
    codes = torch.relu(torch.randn(N, H, generator=g)).to(DEV).requires_grad_(codes_grad)
    W1 = (torch.randn(H, 2 * H, generator=g) * (2.0 / H) ** 0.5).to(DEV).requires_grad_(True)
    b1 = (torch.randn(H, generator=g) * 0.1).to(DEV).requires_grad_(True)
    w2 = (torch.randn(1, H, generator=g) * 0.3).to(DEV).requires_grad_(True)
    b2 = (torch.randn(1, generator=g) * 0.1).to(DEV).requires_grad_(True)
    act = None
    gp = torch.randn(E, generator=g).to(DEV)
    if n_active is not None:
        eid = torch.randperm(E, generator=g)[:n_active]
        eid = (eid if shuffled else torch.sort(eid).values).to(DEV)
        act = ops.ActiveSet()
    if build_pairs:
        ops.get_pairs(ei, N, build=True)
    ops.reset_precision_counts()
    prev = {name: getattr(ops, name) for name, _ in switches}
    try:
        for name, value in switches:
            setattr(ops, name, value)
        if torch_op:
            w2f = w2.detach().reshape(-1).requires_grad_(True)
            w2 = w2f
            pr = torch.ops.sgs.edge_score(codes, ei, W1, b1, w2f, b2, p, 5, 0, True)
        elif epd:
            pr = ops.edge_score_epd(codes, W1, b1, w2, b2, ei, active=act, p=p, seed=5, site=2, p_ep=0.2, seed_x=6, site_x=3, seed_y=7, site_y=4)
        else:
            pr = ops.edge_score(codes, W1, b1, w2, b2, ei, active=act, p=p, seed=5, site=2, precision=precision)
        if act is not None:
            act.set(eid, ops.Graph(ei[:, eid].contiguous(), N))
        if defer:
            with ops.deferred_weight_grads(pr):
                pr.backward(gp)
        else:
            pr.backward(gp)
    finally:
        for name, value in prev.items():
            setattr(ops, name, value)
    torch.cuda.synchronize()
    out[f"scorer/{key}/p"] = pr.detach().cpu()
    for name, leaf in (("codes", codes), ("W1", W1), ("b1", b1), ("w2", w2), ("b2", b2)):
        if leaf.grad is not None:
            out[f"scorer/{key}/d{name}"] = leaf.grad.cpu()
    out[f"scorer/{key}/precision_counts"] = torch.tensor([ops.PRECISION_COUNTS[k] for k in sorted(ops.PRECISION_COUNTS)])


def run_scorer(S, out):
    for N, H, E in ((300, 64, 5000), (777, 128, 65535), (777, 128, 65536)):
        scorer_case(S, out, f"all_active/N{N}_H{H}_E{E}", N, H, E)
    fused = dict(N=777, H=256, E=70001, n_active=66000, row_sorted=True)
    scorer_case(S, out, "fused", **fused)
    scorer_case(S, out, "kept_shuffled", shuffled=True, **fused)
    scorer_case(S, out, "recompute", switches=(("_fwd_mask", False),), **fused)
    scorer_case(S, out, "no_mask_backward", switches=(("_mask_backward", False),), **fused)
    scorer_case(S, out, "unfused_switch", switches=(("_fused_backward", False),), **fused)
    scorer_case(S, out, "bf16/all_active", 777, 128, 65536, precision="bf16")
    scorer_case(S, out, "bf16/fused", precision="bf16", **fused)
    scorer_case(S, out, "bf16/kept_shuffled", precision="bf16", shuffled=True, **fused)
    scorer_case(S, out, "bf16/recompute", precision="bf16", switches=(("_fwd_mask", False),), **fused)
    und = dict(N=777, H=128, E=70000, undirected=True, build_pairs=True)
    scorer_case(S, out, "undirected/mask_with_pairs", **und)
    scorer_case(S, out, "undirected/paired", switches=(("_fwd_mask", False),), **und)
    scorer_case(S, out, "undirected/paired_bf16", precision="bf16", codes_grad=False, **und)
    scorer_case(S, out, "wide/H320", 777, 320, 70001, n_active=66000, row_sorted=True)
    scorer_case(S, out, "wide/H320_undirected", **dict(und, H=320))
    scorer_case(S, out, "codes_frozen", codes_grad=False, **fused)
    scorer_case(S, out, "codes_frozen_small", 300, 64, 5000, codes_grad=False)
    scorer_case(S, out, "hidden_100", 60, 100, 700)
    scorer_case(S, out, "fused_deferred", defer=True, **fused)
    scorer_case(S, out, "epd/large", 500, 256, 70001, n_active=20000, epd=True)
    scorer_case(S, out, "epd/small", 200, 32, 3000, n_active=500, epd=True)
    scorer_case(S, out, "epd/all_active", 200, 32, 3000, epd=True)
    scorer_case(S, out, "torch_op/E700", 60, 16, 700, torch_op=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--parts", default="scorer,steps")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--compare-traces", nargs=2)
    a = ap.parse_args()
    if a.compare:
        return AB.compare(*a.compare)
    if a.compare_traces:
        return AB.compare_traces(*a.compare_traces)
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import sgs_gnn_amd as S
    assert os.path.abspath(S.ops.__file__).startswith(root), S.ops.__file__
    out = {}
    parts = a.parts.split(",")
    if "scorer" in parts:
        run_scorer(S, out)
    if "steps" in parts:
        import bench as B
        AB.run_steps(S, B, out)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save(out, a.out)
    print(json.dumps({"root": root, "arrays": len(out), "ops_file": S.ops.__file__, "lib": S._lib.LIB_PATH}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
