"""Bitwise and launch-for-launch A/B of the layer ops' autograd glue (ops.py) between two checkouts.

    python tools/layer_ops_ab.py --root CHECKOUT --out FILE.pt      one process per checkout: every output and every gradient of
                                                                    each layer op, of a two-layer model per head and of one eager
                                                                    and one graph-replayed hybrid training step, written to FILE.pt
    python tools/layer_ops_ab.py --compare A.pt B.pt                arrays compared with torch.equal; prints one JSON line
    python tools/layer_ops_ab.py --compare-traces DIR_A DIR_B       the ordered (kernel, grid, workgroup, LDS bytes) lists of one
                                                                    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
                                                                    tools/layer_ops_ab.py --root ... --out ...` run per checkout

`--root` is the checkout whose sgs_gnn_amd (and bench.py) is imported; the default is the one this file lives in.  Same seeds in every
run; nothing is timed here."""
import argparse
import contextlib
import csv
import glob
import io
import json
import os
import sys

import torch

DEV = "cuda:0"
ACTS = {"none": (0, 0.0), "relu": (1, 0.0), "relu_dropout": (2, 0.3)}


def graph_edges(N, E, seed):
    """E directed edges over N nodes with one self-loop, one duplicated edge and the last node without in-edges."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E,), generator=g)
    dst = torch.randint(0, N - 1, (E,), generator=g)
    clash = src == dst
    src[clash] = (src[clash] + 1) % N
    src[0], dst[0] = 3, 3
    src[1], dst[1], src[2], dst[2] = 1, 2, 1, 2
    return torch.stack([src, dst])


def run_ops(S, out):
    ops = S.ops

    def leaf(g, *shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(DEV).requires_grad_(True)

    for tag, N, E, chans, fin in (("tiny", 37, 150, (5, 8), 7), ("part", 1000, 20000, (16,), 64)):
        ei = graph_edges(N, E, 1234).to(DEV)
        gr = ops.get_graph(ei, N)
        for C in chans:
            for act_name, (act, p) in ACTS.items():
                ops_here = ("gcn_propagate", "gcn_layer", "gcn2", "cheb_conv", "gat_h1", "gat_h3", "gat_h3_mean", "gat_h3_edge", "gat_h1_edge",
                            "gatv2_h3", "gatv2_h3_edge", "gine")
                # a bias that is trainable everywhere; on the tiny graph also absent and frozen (the prologue's other two choices)
                for op, bias_mode in [(o, b) for b in (("trainable", "absent", "frozen") if tag == "tiny" else ("trainable",)) for o in ops_here]:
                    if op == "gine" and bias_mode != "trainable":
                        continue                                         # (no bias in this op)
                    g = torch.Generator().manual_seed(77)
                    K = 3 if "_h3" in op else 1
                    concat = not op.endswith("_mean")
                    width = K * C if concat else C
                    w = (torch.rand(E, generator=g) + 0.1).to(DEV).requires_grad_(True)
                    bias = leaf(g, width, scale=0.3)
                    L = {"w": w, "bias": bias}
                    if bias_mode == "absent":
                        bias = None
                        del L["bias"]
                    elif bias_mode == "frozen":
                        bias.requires_grad_(False)
                    kw = dict(act=act, p=p, seed=5, site=2)
                    akw = dict(act=act, p_act=p, seed_act=5, site_act=2, heads=K, concat=concat, p_att=0.3 if act == 2 else 0.0, seed_att=9, site_att=3)
                    if op == "gcn_propagate":
                        L["X"] = leaf(g, N, C)
                        Y = ops.gcn_propagate(L["X"], ops.gcn_norm(gr, w), bias, **kw)
                    elif op == "gcn_layer":
                        L["x"], L["W"] = leaf(g, N, fin), leaf(g, C, fin, scale=0.4)
                        Y, _ = ops.gcn_layer(L["x"], L["W"], bias, ops.gcn_norm(gr, w), **kw)
                    elif op == "gcn2":
                        if act == 0:
                            continue                                     # (the head's hidden layer always has an activation)
                        L["x"], L["W1"], L["W2"], L["b2"] = leaf(g, N, fin), leaf(g, C, fin, scale=0.4), leaf(g, 4, C, scale=0.4), leaf(g, 4)
                        Y, _ = ops.gcn2(L["x"], L["W1"], bias, L["W2"], L["b2"], ops.gcn_norm(gr, w), **kw)
                    elif op == "cheb_conv":
                        L["x"], L["W"] = leaf(g, N, fin), leaf(g, 3 * C, fin, scale=0.4)
                        Y = ops.cheb_conv(L["x"], L["W"], bias, ops.cheb_norm(gr, w), 3, **kw)
                    elif op == "gine":
                        L["x"], L["a"], L["b"] = leaf(g, N, C), leaf(g, C), leaf(g, C)
                        del L["bias"]
                        ea = ops.edge_attr(gr, w)
                        Y = ops.gine_aggregate(ops.gine_aggregate(L["x"], ea, L["a"], L["b"]), ea, L["a"], L["b"], 1.5)   # two layers, one EdgeAttr
                    elif op.startswith("gatv2"):
                        L["xl"], L["xr"], L["att"] = leaf(g, N, K * C), leaf(g, N, K * C), leaf(g, K * C, scale=0.5)
                        if op.endswith("_edge"):
                            L["lin_edge"] = leaf(g, K * C, scale=0.5)
                            akw.update(edge_weight=w, lin_edge=L["lin_edge"])
                        Y = ops.gatv2_aggregate(L["xl"], L["xr"], L["att"], bias, gr, **akw)
                    else:
                        shape = (N,) if (K == 1 and not op.endswith("_edge")) else (N, K)
                        L["xl"], L["a_s"], L["a_d"] = leaf(g, N, K * C), leaf(g, *shape), leaf(g, *shape)
                        if op.endswith("_edge"):
                            L["coef"] = leaf(g, K, scale=0.5)
                            akw.update(edge_weight=w, edge_coef=L["coef"])
                        Y = ops.gat_aggregate(L["xl"], L["a_s"], L["a_d"], bias, gr, **akw)
                    Y.backward(torch.randn(*Y.shape, generator=g).to(DEV))
                    key = f"op/{tag}/C{C}/{act_name}/{op}" + ("" if bias_mode == "trainable" else f"/bias_{bias_mode}")
                    out[f"{key}/Y"] = Y.detach().cpu()
                    for k, v in L.items():
                        if v.grad is not None:
                            out[f"{key}/d{k}"] = v.grad.cpu()


class _Data:
    pass


def run_models(S, out):
    N, E, fin, hid, ncls = 1000, 20000, 64, 32, 7
    ei = graph_edges(N, E, 4321).to(DEV)
    g = torch.Generator().manual_seed(5)
    data = _Data()
    data.x = torch.randn(N, fin, generator=g).to(DEV)
    w0 = torch.rand(E, generator=g) + 0.1
    heads = {"gcn": lambda: S.GNNModel(fin, hid, ncls, edge_mlp_type="GCN"),
             "gat_h1": lambda: S.GATModel(fin, hid, ncls, edge_mlp_type="GCN", gat_heads=1),
             "gat_h8": lambda: S.GATModel(fin, hid, ncls, edge_mlp_type="GCN", gat_heads=8),
             "gat_h8_edge": lambda: S.GATModel(fin, hid, ncls, edge_mlp_type="GCN", gat_heads=8, gat_edge_weight=True),
             "gat_h1_edge": lambda: S.GATModel(fin, hid, ncls, edge_mlp_type="GCN", gat_heads=1, gat_edge_weight=True),
             "gatv2_h8": lambda: S.GATModel(fin, hid, ncls, edge_mlp_type="GCN", gat_heads=8, gat_v2=True),
             "gatv2_h8_edge": lambda: S.GATModel(fin, hid, ncls, edge_mlp_type="GCN", gat_heads=8, gat_v2=True, gat_edge_weight=True),
             "gine": lambda: S.GINModel(fin, hid, ncls, edge_mlp_type="GCN", gin_edge_weight=True),
             "cheb_k3": lambda: S.ChebModel(fin, hid, ncls, edge_mlp_type="GCN", cheb_k=3)}
    for name, make in heads.items():
        for mode in ("train", "eval"):                       # dropout 0.3 / none
            S.fix_seeds(42)
            m = make().to(DEV)
            m.train(mode == "train")
            w = w0.to(DEV).requires_grad_(True)
            logits = m(data, ei, w)
            logits.square().sum().backward()
            key = f"model/{name}/{mode}"
            out[f"{key}/logits"] = logits.detach().cpu()
            if w.grad is not None:
                out[f"{key}/dw"] = w.grad.cpu()
            for n, p in m.named_parameters():
                if p.grad is not None:
                    out[f"{key}/d{n}"] = p.grad.cpu()


def run_steps(S, B, out):
    crit = torch.nn.CrossEntropyLoss()
    for form in ("eager", "graph"):
        S.fix_seeds(42)
        model, og, oe, oa = B.build_model(S, DEV, fused=True)
        args = B.make_args(DEV)
        args.sgs_hipgraph = form == "graph"
        pool = S.reddit_partition_stream(num_parts=2, seed=1000, nfeat=B.NFEAT, ncls=B.NCLS, n=B.N_NODES, q=B.Q, device=DEV)
        with contextlib.redirect_stdout(io.StringIO()):
            if form == "graph":
                S.prepare_step_graphs(args, model, og, oe, crit, pool, q=B.Q)
            ret = S.train(args, 0, 10, model, og, oe, oa, crit, pool, q=B.Q)
        torch.cuda.synchronize()
        out[f"step/{form}/loss"] = torch.tensor([float(ret[0])], dtype=torch.float64)
        for n, p in model.named_parameters():
            out[f"step/{form}/{n}"] = p.detach().cpu()


def compare(a, b):
    A, Bv = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    bits = lambda t: t.contiguous().reshape(-1).view(torch.uint8)           # (bytes: a NaN equals itself)
    differing = [k for k in A if k in Bv and not (A[k].shape == Bv[k].shape and A[k].dtype == Bv[k].dtype and torch.equal(bits(A[k]), bits(Bv[k])))]
    groups = {}
    for k in A:
        groups[k.split("/")[0]] = groups.get(k.split("/")[0], 0) + 1
    print(json.dumps({"arrays_compared": len([k for k in A if k in Bv]), "by_group": groups, "only_in_a": sorted(set(A) - set(Bv)),
                      "only_in_b": sorted(set(Bv) - set(A)), "arrays_differing": differing,
                      "bytes_compared": sum(v.numel() * v.element_size() for k, v in A.items() if k in Bv)}))
    return 0 if not differing and set(A) == set(Bv) else 1


def launches(d):
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(fn)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    I = lambda r, k: int(r.get(k, 0) or 0)
    return [(r["Kernel_Name"], (I(r, "Grid_Size_X"), I(r, "Grid_Size_Y"), I(r, "Grid_Size_Z")),
             (I(r, "Workgroup_Size_X"), I(r, "Workgroup_Size_Y"), I(r, "Workgroup_Size_Z")), I(r, "LDS_Block_Size")) for r in rows]


def compare_traces(da, db):
    a, b = launches(da), launches(db)
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    same_order = len(a) == len(b) and first is None
    res = {"launches_a": len(a), "launches_b": len(b), "ordered_lists_identical": same_order, "multisets_identical": sorted(a) == sorted(b),
           "distinct_kernels": len({x[0] for x in a})}
    if not same_order and first is not None:
        res["first_difference"] = {"index": first, "a": a[first], "b": b[first]}
    print(json.dumps(res))
    return 0 if same_order else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--parts", default="ops,models,steps")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--compare-traces", nargs=2)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if a.compare_traces:
        return compare_traces(*a.compare_traces)
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import sgs_gnn_amd as S
    assert os.path.abspath(S.ops.__file__).startswith(root), S.ops.__file__
    out = {}
    parts = a.parts.split(",")
    if "ops" in parts:
        run_ops(S, out)
    if "models" in parts:
        run_models(S, out)
    if "steps" in parts:
        import bench as B
        run_steps(S, B, out)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save(out, a.out)
    print(json.dumps({"root": root, "arrays": len(out), "ops_file": S.ops.__file__}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
