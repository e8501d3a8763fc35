"""Bitwise and launch-for-launch A/B of the cross entropy / hybrid loss family (csrc/losses.hip, ops.py, sharded.py) between two checkouts.

    python tools/loss_family_ab.py --root CHECKOUT --out FILE.pt    one process per checkout: every array the ten C entry points of the
                                                                    family write, the Python paths on top of them, the node-block
                                                                    cross entropy and one eager and one graph-replayed hybrid step per
                                                                    criterion, written to FILE.pt
    python tools/loss_family_ab.py --compare A.pt B.pt              arrays compared byte for byte (a NaN equals itself); one JSON line
    python tools/loss_family_ab.py --compare-traces DIR_A DIR_B     the ordered (kernel up to its template arguments, grid, workgroup,
                                                                    LDS bytes) lists of one `rocprofv3 --kernel-trace --output-format
                                                                    csv -d DIR -- python tools/loss_family_ab.py --root ... --out ...`
                                                                    run per checkout

`--root` is the checkout whose sgs_gnn_amd, bench.py and tests/*_ref.py are imported; the default is the one this file lives in.  Inputs are
the seeded tables of tests/loss_ref.py and tests/ce_weighted_ref.py.  Output buffers start as NaN (int32 words as INT_MIN), the accumulating
entries' as a seeded array.  Same seeds in every run; nothing is timed here."""
import argparse
import contextlib
import csv
import glob
import gzip
import io
import json
import os
import re
import sys

import torch

DEV = "cuda:0"
HYBRID = ("N257_C41_q65", "N257_C130_q65", "coef_1.0_0.0", "coef_0.0_0.5", "mask_one", "mask_none", "w_0_and_1", "labelsum_0", "labelsum_1",
          "labelsum_2", "N1_C41_q5000")
G = 2.5


def _nan(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -(2 ** 31), dtype=dtype, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _seeded(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(99)).to(DEV)


def class_weights(C, kind):
    if kind == "none":
        return None
    w = torch.rand(C, generator=torch.Generator().manual_seed(17 + C)) * 4.8 + 0.2
    if kind == "zero1":
        w[C // 2] = 0.0
    return w.to(DEV)


def criteria(C):
    """(tag, weighted entry?, weight, eps): the plain criterion, then weight in {none, random, one zero entry} x eps in {0, 0.1, 1}."""
    yield "plain", False, None, 0.0
    for wk in ("none", "rand", "zero1"):
        for eps in (0.0, 0.1, 1.0):
            yield f"w{wk}_eps{eps}", True, class_weights(C, wk), eps


def masked_ce_abi(S, key, lg, y, mk, out, crits=None):
    """The six sgs_masked_ce* entries on one (logits, y, mask), for `crits` (default: every criterion of `criteria`)."""
    ops, lib = S.ops, S._lib
    L, p, st = lib.lib(), ops._ptr, ops._stream
    N, C = lg.shape
    gl = torch.tensor([G], dtype=torch.float32, device=DEV)
    for tag, wd, wt, eps in crits or criteria(C):
        crit = (p(wt), eps) if wd else ()
        w_ = "_w" if wd else ""
        o = dict(loss=_nan(1), row_lse=_nan(N), rowloss=_nan(N), norm=_nan(1, dtype=torch.float32 if wd else torch.int32), d=_nan(N, C), acc=_seeded(N, C))
        lib.check(getattr(L, f"sgs_masked_ce{w_}_fwd")(p(lg), N, C, p(y), p(mk), *crit, p(o["loss"]), p(o["row_lse"]), p(o["rowloss"]), p(o["norm"]), st()), "fwd")
        lib.check(getattr(L, f"sgs_masked_ce{w_}_bwd")(p(lg), N, C, p(y), p(mk), *crit, p(o["row_lse"]), p(o["norm"]), p(gl), p(o["d"]), st()), "bwd")
        lib.check(getattr(L, f"sgs_masked_ce{w_}_bwd_acc")(p(lg), N, C, p(y), p(mk), *crit, p(o["row_lse"]), p(o["norm"]), p(gl), p(o["acc"]), st()), "bwd_acc")
        for k, v in o.items():
            out[f"abi/{key}/{tag}/masked_ce/{k}"] = v.cpu()


def hybrid_abi(S, name, c, out):
    """sgs_hybrid_loss(_w)_fwd and sgs_hybrid_loss_fused_fwd / _bwd (weighted 0 and 1) on one case of tests/loss_ref.py."""
    ops, lib = S.ops, S._lib
    L, p, st = lib.lib(), ops._ptr, ops._stream
    N, C, q = c["N"], c["C"], c["q"]
    lg, y, mk, w, sei = c["logits"].to(DEV), c["y"].to(DEV), ops._u8(c["mask"].to(DEV)), c["w"].to(DEV), c["sei"].to(DEV)
    gl = torch.tensor([G], dtype=torch.float32, device=DEV)
    gr = ops.get_graph(sei, N)
    ws = ops.workspace(L.sgs_edge_reg_workspace_bytes(q), lg.device)
    masked_ce_abi(S, name, lg, y, mk, out)
    for tag, wd, wt, eps in criteria(C):
        crit = (p(wt), eps) if wd else ()
        ndt = torch.float32 if wd else torch.int32
        o = dict(out=_nan(7), row_lse=_nan(N), rowloss=_nan(N), norm=_nan(1, dtype=ndt))
        fn = "sgs_hybrid_loss_w_fwd" if wd else "sgs_hybrid_loss_fwd"
        lib.check(getattr(L, fn)(p(lg), N, C, p(y), p(mk), p(w), p(sei), q, c["c1"], c["c2"], *crit, p(o["out"]), p(o["row_lse"]), p(o["rowloss"]),
                                 p(o["norm"]), ws.data_ptr(), ws.numel(), st()), fn)
        for k, v in o.items():
            out[f"abi/{name}/{tag}/hybrid_fwd/{k}"] = v.cpu()
        for with_stash in (True, False):
            f = dict(out=_nan(7), row_lse=_nan(N), rowloss=_nan(N), norm=_nan(1, dtype=ndt))
            stash = _nan(q, 4) if with_stash else None
            lib.check(L.sgs_hybrid_loss_fused_fwd(p(lg), N, C, p(y), p(mk), p(w), p(sei), q, c["c1"], c["c2"], int(wd), p(wt), eps, p(f["out"]),
                                                  p(f["row_lse"]), p(f["rowloss"]), p(f["norm"]), p(stash), ws.data_ptr(), ws.numel(), st()), "fused_fwd")
            if with_stash:
                f.update(stash=stash, dw=_nan(q), dlogits=_nan(N, C))
                lib.check(L.sgs_hybrid_loss_fused_bwd(p(lg), N, C, p(y), p(mk), p(w), q, p(stash), p(f["out"]), c["c1"], int(wd), p(wt), eps,
                                                      p(f["row_lse"]), p(f["norm"]), p(gl), p(gr.in_ptr), p(gr.in_src), p(gr.in_eid), p(gr.out_ptr),
                                                      p(gr.out_dst), p(gr.out_eid), p(f["dw"]), p(f["dlogits"]), st()), "fused_bwd")
            for k, v in f.items():
                out[f"abi/{name}/{tag}/fused_{'stash' if with_stash else 'nostash'}/{k}"] = v.cpu()


def python_paths(S, name, c, out):
    """ops.masked_cross_entropy, ops.edge_regularizers and ops.hybrid_loss: no keywords, neutral keywords, every weighted criterion."""
    ops = S.ops
    y, mk, sei = c["y"].to(DEV), c["mask"].to(DEV), c["sei"].to(DEV)
    settings = [("nokw", {}), ("neutral", dict(weight=None, label_smoothing=0.0))]
    settings += [(tag, dict(weight=wt, label_smoothing=eps)) for tag, wd, wt, eps in criteria(c["C"]) if wd]
    for tag, kw in settings:
        ld = c["logits"].to(DEV).requires_grad_(True)
        loss = ops.masked_cross_entropy(ld, y, mk, **kw)
        (loss * G).backward()
        out[f"py/{name}/{tag}/ce/loss"], out[f"py/{name}/{tag}/ce/dlogits"] = loss.detach().cpu(), ld.grad.cpu()
        ld, wd_ = c["logits"].to(DEV).requires_grad_(True), c["w"].to(DEV).requires_grad_(True)
        loss, o7 = ops.hybrid_loss(ld, y, mk, wd_, sei, c["c1"], c["c2"], **kw)
        (loss * G).backward()
        out[f"py/{name}/{tag}/hybrid/loss"], out[f"py/{name}/{tag}/hybrid/out"] = loss.detach().cpu(), o7.cpu()
        out[f"py/{name}/{tag}/hybrid/dlogits"], out[f"py/{name}/{tag}/hybrid/dw"] = ld.grad.cpu(), wd_.grad.cpu()
        with torch.no_grad():
            out[f"py/{name}/{tag}/hybrid/out_nograd"] = ops.hybrid_loss(ld, y, mk, wd_, sei, c["c1"], c["c2"], **kw)[1].cpu()
    ld, wd_ = c["logits"].to(DEV).requires_grad_(True), c["w"].to(DEV).requires_grad_(True)
    total, o5 = ops.edge_regularizers(wd_, ld, sei, y, mk, c["c1"], c["c2"])
    (total * G).backward()
    out[f"py/{name}/reg/total"], out[f"py/{name}/reg/out"] = total.detach().cpu(), o5.cpu()
    out[f"py/{name}/reg/dw"] = wd_.grad.cpu()
    if ld.grad is not None:
        out[f"py/{name}/reg/dlogits"] = ld.grad.cpu()


def block_node(S, name, c, out):
    """sharded's node-block cross entropy called directly on the row blocks [0, 0) (empty), [0, N // 3) and [N // 3, N)."""
    from importlib import import_module
    sh, ops = import_module("sgs_gnn_amd.sharded"), S.ops
    N, C = c["logits"].shape
    y, m = c["y"].to(DEV), c["mask"].to(DEV)
    n_train = m.sum().to(torch.int32).reshape(1).contiguous()
    for tag, wd, wt, eps in criteria(C):
        wd = wt is not None or eps != 0.0                 # (as the trainer: no weight and no smoothing is the plain criterion)
        if wt is None:
            den = n_train.to(torch.float32)
        else:
            wy = wt[y.clamp(0, C - 1)]
            den = torch.where(m, wy, torch.zeros_like(wy)).sum().reshape(1)
        for lo, hi in ((0, 0), (0, N // 3), (N // 3, N)):
            lb = c["logits"][lo:hi].contiguous().to(DEV).requires_grad_(True)
            a = (lb, y[lo:hi].contiguous(), ops._u8(m[lo:hi].contiguous()))
            if hasattr(sh, "_BlockCEW"):                                      # a checkout with one node per criterion
                v = sh._BlockCEW.apply(*a, den, wt, eps) if wd else sh._BlockCE.apply(*a, n_train)
            else:
                v = sh._BlockCE.apply(*a, den if wd else n_train, wt, eps)
            (v * G).backward()
            out[f"block/{name}/{tag}/{lo}_{hi}/share"], out[f"block/{name}/{tag}/{lo}_{hi}/dlogits"] = v.detach().cpu(), lb.grad.cpu()


def run_steps(S, B, out):
    w = (torch.rand(B.NCLS, generator=torch.Generator().manual_seed(3)) + 0.5).to(DEV)
    for cname, crit in (("plain", torch.nn.CrossEntropyLoss()), ("weighted", torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1))):
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
            out[f"step/{cname}/{form}/loss"] = torch.tensor([float(ret[0])], dtype=torch.float64)
            for n, p in model.named_parameters():
                out[f"step/{cname}/{form}/{n}"] = p.detach().cpu()


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


def _stem(kernel):
    """A kernel's name up to its template arguments and its argument list, without return type and namespaces."""
    k = re.sub(r"\s*\[clone .*$", "", kernel).replace("(anonymous namespace)::", "")
    k = re.sub(r"\.kd$", "", re.split(r"[<(]", k, 1)[0])
    return k.split()[-1].split("::")[-1]


def launches(d):
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv*"), recursive=True):       # (.csv, or .csv.gz as the records are kept)
        rows += list(csv.DictReader(gzip.open(fn, "rt") if fn.endswith(".gz") else open(fn)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    I = lambda r, k: int(r.get(k, 0) or 0)
    return [(_stem(r["Kernel_Name"]), (I(r, "Grid_Size_X"), I(r, "Grid_Size_Y"), I(r, "Grid_Size_Z")),
             (I(r, "Workgroup_Size_X"), I(r, "Workgroup_Size_Y"), I(r, "Workgroup_Size_Z")), I(r, "LDS_Block_Size")) for r in rows]


# a checkout with one kernel per criterion names the weighted ones with a suffix or a kernel of their own
_SAME = {"ce_rows_w": "ce_rows", "ce_final_w": "ce_final", "ce_bwd_w": "ce_bwd", "ce_bwd_acc": "ce_bwd", "hybrid_loss_final_w": "hybrid_loss_final"}


def compare_traces(da, db):
    canon = lambda rows: [(_SAME.get(k, k),) + tuple(rest) for k, *rest in rows]
    a, b = canon(launches(da)), canon(launches(db))
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    same_order = len(a) == len(b) and first is None
    fam = {}
    for x in b:
        if x[0] in ("ce_rows", "ce_final", "ce_bwd", "hybrid_loss_final", "hybrid_fwd_pair", "reg_fwd_partial", "reg_fwd_final", "reg_bwd_edges",
                    "endpoint_reduce", "endpoint_reduce_rowblock"):
            fam[x[0]] = fam.get(x[0], 0) + 1
    res = {"launches_a": len(a), "launches_b": len(b), "ordered_lists_identical": same_order, "multisets_identical": sorted(a) == sorted(b),
           "distinct_kernels": len({x[0] for x in a}), "family_launches_b": fam}
    if not same_order and first is not None:
        res["first_difference"] = {"index": first, "a": a[first], "b": b[first]}
    print(json.dumps(res))
    return 0 if same_order else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--parts", default="abi,python,block,steps")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--compare-traces", nargs=2)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if a.compare_traces:
        return compare_traces(*a.compare_traces)
    root = os.path.abspath(a.root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import sgs_gnn_amd as S
    import ce_weighted_ref as CW
    import loss_ref as R
    assert os.path.abspath(S.ops.__file__).startswith(root) and os.path.abspath(R.__file__).startswith(root), (S.ops.__file__, R.__file__)
    out = {}
    parts = a.parts.split(",")
    for name in HYBRID:
        c = R.make_case(name)
        if "abi" in parts:
            hybrid_abi(S, name, c, out)
        if "python" in parts:
            python_paths(S, name, c, out)
    for name in CW.CASES:
        c = CW.make_case(name)
        if "abi" in parts:                       # the plain entries and the case's own (weight, eps) through the weighted ones
            own = [("plain", False, None, 0.0), ("own", True, None if c["w"] is None else c["w"].to(DEV), c["eps"])]
            masked_ce_abi(S, name, c["logits"].to(DEV), c["y"].to(DEV), S.ops._u8(c["mask"].to(DEV)), out, own)
        if "block" in parts and c["N"] >= 3 and c["eps"] == 0.1 and name.endswith("_wrand_m60"):
            block_node(S, name, c, out)
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
