"""Bitwise, collective-for-collective and launch-for-launch A/B of the sharded training steps (sharded.py: `train_step_sharded`, the
all-reduce form, and `train_step_blocksharded`, the node-block form) between two checkouts.

    python tools/sharded_ab.py --root CHECKOUT --out FILE.pt        one checkout: world 1 without a process group, then worlds 2 and 3
                                                                    as gloo ranks sharing cuda:0 -- one child process per rank, each
                                                                    under its own time limit, at most three at a time; stops at the
                                                                    first non-zero exit.  Every rank's dump lands in FILE.pt
    python tools/sharded_ab.py --compare A.pt B.pt [--again A2.pt]  B against A.  With --again (a second run of A's checkout): every
                                                                    entry A reproduces must be equal in B; the others are listed and
                                                                    held to the bounds of test_sharded_training_step_matches_single_
                                                                    gpu_train.  Collective lists equal, peak memory not above A's
    python tools/sharded_ab.py --compare-traces DIR_A DIR_B         the ordered (kernel, grid, workgroup, LDS bytes) lists of one
                                                                    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
                                                                    tools/sharded_ab.py --root ... --world 1 --rank 0 --out ...` run
                                                                    per checkout (a rank run directly, so the trace sees its launches)
    python tools/sharded_ab.py --root CHECKOUT --time --out F.json  median wall time of one step, case "std", world 1, both forms

Cases (both forms on each; graph, model and arguments of tests/test_gpu_sharded.py::_train_setup, q = E // 5): "std" the plain criterion,
"weighted" class weights and label smoothing 0.1, "nogate" conditional=False, "hub" a source-sorted list in which node 5 has 9 000 of the
11 990 edges (repeated destinations), so that at world 3 rank 1's shard lies inside the hub's row (edges, but an empty node block) and
rank 0 reads a halo row -- checked with `block_layout` on the CPU before any rank starts.  Per rank and step the dump holds the loss, the
gate's decision and counts, both draw masks, the logits, the collectives issued (name, dtype, numel; recorded by wrapping torch.distributed
here), after step 0 every parameter gradient, after the last step every parameter, and the peak of allocated device memory (the garbage
collector runs between the steps and not inside them: the norm's autograd node and its Norm refer to each other, and the moment such a
cycle happens to be freed must not decide the peak)."""
import argparse
import csv
import gc
import glob
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import torch

DEV = "cuda:0"
CASES = ("std", "weighted", "nogate", "hub")
FORMS = {"allreduce": "train_step_sharded", "blocks": "train_step_blocksharded"}
HUB = dict(N=300, node=5, hub_edges=9000, others=10)
COLLECTIVES = ("all_reduce", "all_gather", "reduce_scatter", "broadcast", "all_gather_into_tensor", "reduce_scatter_tensor", "all_to_all")


def hub_edges():
    """Source-sorted [2, 11 990]: node 5 points 9 000 times round the other nodes, every other node at 10 distinct ones."""
    N, h = HUB["N"], HUB["node"]
    g = torch.Generator().manual_seed(11)
    src, dst = [], []
    for s in range(N):
        if s == h:
            d = torch.arange(HUB["hub_edges"]) % (N - 1)
        else:
            d = torch.randperm(N - 1, generator=g)[:HUB["others"]].sort().values
        src.append(torch.full_like(d, s))
        dst.append(d + (d >= s))                                             # (no self-loop)
    return torch.stack([torch.cat(src), torch.cat(dst)])


def check_hub_layout(sh, chunk):
    """At world 3: a rank with edges and an empty block, and a rank with a halo row -- by the checkout's own arithmetic where it has the
    pure function (the parent does not; the layout is a property of the list, so the branch's answer stands for both)."""
    ei = hub_edges()
    b = sh.shard_bounds(ei.shape[1], 3, chunk)
    firsts = [int(ei[0, b[r]]) if b[r + 1] > b[r] else HUB["N"] for r in range(3)]
    if not hasattr(sh, "block_layout"):
        return dict(bounds=b, firsts=firsts)
    lay = [sh.block_layout(firsts, HUB["N"], r, 3) for r in range(3)]
    empty_block = [r for r in range(3) if b[r + 1] > b[r] and lay[r][1] == lay[r][2]]
    halo = [r for r in range(3) if lay[r][4]]
    assert empty_block and halo, (b, firsts, lay)
    return dict(bounds=b, firsts=firsts, nb=lay[0][0], ranks_with_edges_and_an_empty_block=empty_block, ranks_with_a_halo=halo)


def setup(S, case):
    import torch.nn as nn
    b = S.synthetic_graph(300, 21000, 16, 5, seed=3, train_frac=0.5, device=DEV)
    if case == "hub":
        ei = hub_edges()
        b.edge_index, b.prob = ei.to(DEV), S.degree_prior(ei, HUB["N"]).to(DEV)
    torch.manual_seed(0)
    m = S.GNNModel(16, 64, 5, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
    og = torch.optim.Adam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-3)
    oe = torch.optim.Adam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-3)
    args = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", conditional=case != "nogate", sparse_edge_mlp=True, t_init=0.7,
                              t_min=0.5, degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0, consist_reg_coef=0.5,
                              hybrid_checkpoint=False)
    crit = nn.CrossEntropyLoss()
    if case == "weighted":
        crit = nn.CrossEntropyLoss(weight=torch.tensor([0.5, 1.0, 2.0, 1.5, 0.75], device=DEV), label_smoothing=0.1)
    return b, m, og, oe, args, crit


def record_collectives(log):
    import torch.distributed as dist

    def wrap(name, fn):
        def f(*a, **kw):
            t = next(x for x in list(a) + list(kw.values()) if torch.is_tensor(x) or (isinstance(x, list) and x and torch.is_tensor(x[0])))
            t = t[0] if isinstance(t, list) else t
            log.append((name, str(t.dtype), int(t.numel())))
            return fn(*a, **kw)
        return f
    for name in COLLECTIVES:
        if hasattr(dist, name):
            setattr(dist, name, wrap(name, getattr(dist, name)))


def import_checkout(root):
    sys.path.insert(0, root)
    import sgs_gnn_amd as S
    from importlib import import_module
    sh = import_module("sgs_gnn_amd.sharded")
    assert os.path.abspath(sh.__file__).startswith(root), sh.__file__
    return S, sh


def run_rank(a):
    import torch.distributed as dist
    root = os.path.abspath(a.root)
    torch.cuda.set_device(0)
    if a.world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world))
        dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    try:
        S, sh = import_checkout(root)
        if a.time:
            return time_steps(S, sh, a)
        log, out = [], {}
        record_collectives(log)
        gc.disable()                                     # (the peak must not depend on when the collector happens to free a step's cycles)
        for case in a.cases.split(","):
            for form, fn in FORMS.items():
                b, m, og, oe, args, crit = setup(S, case)
                shard = sh.EdgeShard(b, a.rank, a.world)
                q = b.edge_index.shape[1] // 5
                S.fix_seeds(a.seed)
                key = f"{case}/{form}"
                tr = None
                for step in range(a.steps):
                    gc.collect()
                    if step == 0:
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                    del log[:]
                    tr = getattr(sh, fn)(args, m, shard, og, oe, crit, q)
                    k = f"{key}/s{step}"
                    out[f"{k}/loss"] = tr["loss"].detach().reshape(1).cpu()
                    out[f"{k}/update_edge_mlp"] = bool(tr["update_edge_mlp"])
                    out[f"{k}/counts"] = tr["counts"]
                    out[f"{k}/mask"], out[f"{k}/rmask"] = tr["sample"].mask.cpu(), tr["random"].mask.cpu()
                    out[f"{k}/learned_out"] = tr["learned_out"].cpu()
                    out[f"{k}/collectives"] = list(log)
                    if step == 0:
                        for n, p in m.named_parameters():
                            if p.grad is not None:
                                out[f"{k}/grad/{n}"] = p.grad.detach().cpu()
                for n, p in m.named_parameters():
                    out[f"{key}/param/{n}"] = p.detach().cpu()
                torch.cuda.synchronize()
                out[f"{key}/peak_bytes"] = int(torch.cuda.max_memory_allocated())
        torch.save(out, a.out)
        print(json.dumps({"root": root, "world": a.world, "rank": a.rank, "entries": len(out), "sharded_file": sh.__file__}))
        return 0
    finally:
        if a.world > 1:
            dist.destroy_process_group()


def time_steps(S, sh, a):
    """Median wall time of one step (torch.cuda.synchronize() on both sides), case "std", world 1 without a process group."""
    res = {"root": os.path.abspath(a.root), "label": a.label, "warmup": a.warmup, "steps": a.timed_steps}
    for form, fn in FORMS.items():
        b, m, og, oe, args, crit = setup(S, "std")
        shard = sh.EdgeShard(b, 0, 1)
        q = b.edge_index.shape[1] // 5
        S.fix_seeds(a.seed)
        ts = []
        for i in range(a.warmup + a.timed_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            getattr(sh, fn)(args, m, shard, og, oe, crit, q)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts = ts[a.warmup:]
        res[form] = {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"))
    return 0


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(a):
    """The launcher opens no GPU: world by world, one child per rank under `timeout`, the first non-zero exit ends the run."""
    root = os.path.abspath(a.root)
    if "hub" in a.cases.split(","):
        S, sh = import_checkout(root)
        print(json.dumps({"hub_layout_world3": check_hub_layout(sh, int(S._lib.lib().sgs_sampler_chunk()))}))
    merged = {}
    for world in [int(w) for w in a.worlds.split(",")]:
        port = free_port()
        parts = [f"{a.out}.w{world}r{r}" for r in range(world)]
        procs = [subprocess.Popen(["timeout", "-k", "10", str(a.rank_timeout), sys.executable, os.path.abspath(__file__), "--root", root,
                                   "--world", str(world), "--rank", str(r), "--port", str(port), "--out", parts[r], "--cases", a.cases,
                                   "--steps", str(a.steps), "--seed", str(a.seed)]) for r in range(world)]
        codes = [p.wait() for p in procs]
        if any(codes):
            print(json.dumps({"world": world, "exit_codes": codes}))
            return next(c for c in codes if c)
        for r, fn in enumerate(parts):
            merged.update({f"w{world}/r{r}/{k}": v for k, v in torch.load(fn, weights_only=True).items()})
            os.remove(fn)
    torch.save(merged, a.out)
    gates = {}
    for k, v in merged.items():
        if k.endswith("/update_edge_mlp"):
            w, _, case, form, _, _ = k.split("/")
            gates.setdefault(f"{case}/{form}/{w}", set()).add(v)
    print(json.dumps({"root": root, "entries": len(merged), "both_gate_branches_in": sorted(k for k, v in gates.items() if len(v) == 2)}))
    return 0


def same(x, y):
    if torch.is_tensor(x) != torch.is_tensor(y):
        return False
    if not torch.is_tensor(x):
        return json.dumps(x) == json.dumps(y)
    bits = lambda t: t.contiguous().reshape(-1).view(torch.uint8)               # (bytes: a NaN equals itself)
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y))


def within_test_bounds(key, x, y):
    """For an entry the parent does not reproduce: the bound tests/test_gpu_sharded.py holds that quantity to (None: it holds it to
    equality -- masks, the gate -- or does not look at it; then nothing but equality passes here)."""
    name = key.split("/")
    if name[-1] == "loss":
        return abs(float(x) - float(y)) < 2e-5
    if name[-1] == "learned_out":
        return torch.allclose(y, x, rtol=1e-4, atol=1e-5)
    if "grad" in name:
        return float((y - x).abs().max()) / (float(x.abs().max()) + 1e-12) < 2e-3
    if "param" in name:
        return torch.allclose(y, x, rtol=0, atol=2.5e-3)
    return False


def compare(fa, fb, again):
    A, B = torch.load(fa, weights_only=True), torch.load(fb, weights_only=True)
    A2 = torch.load(again, weights_only=True) if again else A
    peak = lambda k: k.endswith("/peak_bytes")
    unstable = sorted(k for k in A if not peak(k) and not same(A[k], A2.get(k)))
    differing = [k for k in A if k in B and not peak(k) and k not in unstable and not same(A[k], B[k])]
    out_of_bounds = [k for k in unstable if k in B and not same(A[k], B[k]) and not within_test_bounds(k, A[k], B[k])]
    peak_above = {k: (max(A[k], A2[k]), B[k]) for k in A if peak(k) and k in B and B[k] > max(A[k], A2[k])}
    coll = [k for k in A if k.endswith("/collectives")]
    res = {"entries_compared": len([k for k in A if k in B]), "only_in_a": sorted(set(A) - set(B)), "only_in_b": sorted(set(B) - set(A)),
           "parent_runs": 2 if again else 1, "not_reproduced_by_the_parent": unstable, "of_those_outside_the_test_bounds": out_of_bounds,
           "differing": differing, "collective_lists": len(coll), "collectives_issued": sum(len(A[k]) for k in coll),
           "collective_lists_differing": [k for k in coll if k in B and not same(A[k], B[k])], "peak_bytes_above_parent": peak_above,
           "peak_bytes_max": max([A[k] for k in A if peak(k)], default=0),
           "bytes_compared": sum(v.numel() * v.element_size() for k, v in A.items() if k in B and torch.is_tensor(v))}
    print(json.dumps(res))
    return 0 if not (differing or out_of_bounds or peak_above or res["only_in_a"] or res["only_in_b"]) else 1


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
    same_order = len(a) == len(b) and first is None and len(a) > 0
    res = {"launches_a": len(a), "launches_b": len(b), "ordered_lists_identical": same_order, "multisets_identical": sorted(a) == sorted(b),
           "distinct_kernels": len({x[0] for x in a})}
    if first is not None:
        res["first_difference"] = {"index": first, "a": a[first], "b": b[first]}
    print(json.dumps(res))
    return 0 if same_order else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--worlds", default="1,2,3")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--rank-timeout", type=int, default=240, help="seconds each rank process may take")
    ap.add_argument("--world", type=int, default=1, help="with --rank: this process is one rank of a world of this size")
    ap.add_argument("--rank", type=int)
    ap.add_argument("--port", type=int, default=0)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed-steps", type=int, default=40)
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--again")
    ap.add_argument("--compare-traces", nargs=2)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare, a.again)
    if a.compare_traces:
        return compare_traces(*a.compare_traces)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.time:
        a.rank, a.world = 0, 1
    return run_rank(a) if a.rank is not None else launch(a)


if __name__ == "__main__":
    sys.exit(main())
