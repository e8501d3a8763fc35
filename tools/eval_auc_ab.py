"""ROC-AUC on the device: what it costs.  (a) --kernels: ops.auc_pack + ops.auc_counts against a torch composition on the same keys;
(b) default: one ensemble_evaluate with args.sgs_eval_auc on and off, alternating in one process.

    python tools/eval_auc_ab.py [--rounds 7] [--reps 3] [--shapes s3,s4] [--out profiles/r29_eval_auc_ab.json]
    python tools/eval_auc_ab.py --path off --root DIR --out profiles/r29_eval_auc_ab_parent.json      # another tree's flag-off arm alone
    python tools/eval_auc_ab.py --kernels [--out profiles/r29_auc_kernels.json]
    python tools/eval_auc_ab.py --kernels --torch-only --root DIR --out profiles/r29_auc_kernels_parent.json

(a) Pooled shapes [M, S]: bench S3 = 230 x 1 013 rows of 41 log-softmax columns, bench S4 = 5 x 33 869 rows of 5, binary = the S4 rows with
one column.  Scores: log_softmax of 3 N(0, 1) logits (the difference of the first two for the binary shape); on 30 % of the rows one logit is
raised by 40, which makes that column's log p exactly -0.0 (one long tie run per column) as a confident model does.  Labels uniform, masks
20 / 40 / 40 % disjoint.  Arms, alternating per round: "hip" = ops.auc_pack + ops.auc_counts (device radix sort + the rank-sum pass);
"torch" = torch.sort of the keys' sort bits, torch.searchsorted for every item's tie-run start and end, torch.cumsum of the negatives per
split and index_add_ per column, given the keys (under --torch-only the keys are packed by torch ops as well, so the arm runs on a tree
without the entry points); "pack" = ops.auc_pack alone.  The two count tables must be equal.  Per arm: `iters` back-to-back calls between
two HIP events; reported: the median and [min, max] of the rounds' microseconds per call.

(b) s3 = bench S3's 230-partition stream (reddit_partition_stream(num_parts=230, seed=1000); F = 602, C = 41) with GNNModel(F, 256, C) on
the batched GCN engine (sgs_eval_batch=True); s4 = bench S4's five partitions (synthetic_graph(33 869, 463 000, 128, 5, seed=300 + i,
train_frac=0.2, power=0.6)) with GATModel(128, 256, 5) on the serial loop; num_samples_eval = 11, mode 'learned', q = 100 000.  Arms: off,
auc (sgs_eval_auc=True: per partition the score ops and one sgs_auc_pack, after the loader one concatenation, one sgs_auc_counts and one
read-back).  One untimed pass of every arm, then `rounds` rounds in which the arms alternate `reps` times; a pass is timed on the host clock
around a device synchronise; reported: the median of all passes and [min, max] of the per-round medians.  Every pass starts from the same
noise-clock position.  The yardstick of the off arm is the PARENT commit's: `--path off --root DIR` runs it alone on another checkout
(library built); it sets no attribute the parent does not know."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ARMS = ("off", "auc")
Q = 100_000
KERNEL_SHAPES = (("bench_S3", 230 * 1_013, 41), ("bench_S4", 5 * 33_869, 5), ("binary", 5 * 33_869, 1))


def _load(shape, S, dev, torch):
    torch.manual_seed(0)
    if shape == "s3":
        parts = S.reddit_partition_stream(num_parts=230, seed=1000, device=dev)
        return parts, S.GNNModel(602, 256, 41, dropout_prob=0.3, edge_mlp_type="GCN").to(dev), True
    parts = [S.synthetic_graph(33_869, 463_000, 128, 5, seed=300 + i, train_frac=0.2, power=0.6, device=dev) for i in range(5)]
    return parts, S.GATModel(128, 256, 5, dropout_prob=0.3, edge_mlp_type="GCN").to(dev), False


def _summary(rounds):
    flat = [t for r in rounds for t in r]
    meds = [statistics.median(r) for r in rounds]
    return {"median_s": statistics.median(flat), "round_median_min_s": min(meds), "round_median_max_s": max(meds), "passes": len(flat)}


def measure(shape, arms, rounds, reps, draws):
    import torch
    import sgs_gnn_amd as S
    EV = sys.modules["sgs_gnn_amd.evaluate"]
    dev = "cuda:0"
    parts, model, batched = _load(shape, S, dev, torch)

    def one(arm):
        a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws)
        if batched:
            a.sgs_eval_batch = True
        if arm == "auc":
            a.sgs_eval_auc = True
        S.manual_seed(11)
        torch.cuda.synchronize()
        before = dict(EV.PATH_COUNTS)
        t0 = time.perf_counter()
        res = S.ensemble_evaluate(a, model, parts, dev, q=Q, mode="learned")
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        path = "batched" if batched else "serial"
        assert EV.PATH_COUNTS[path] == before[path] + 1, f"{arm} took the other path"
        return t, res

    for arm in arms:                                    # warm-up: allocator growth, library load
        one(arm)
    times = {arm: [] for arm in arms}
    triple = {}
    for _ in range(rounds):
        rnd = {arm: [] for arm in arms}
        for _ in range(reps):
            for arm in arms:
                t, triple[arm] = one(arm)
                rnd[arm].append(t)
        for arm in arms:
            times[arm].append(rnd[arm])
    out = {"shape": shape, "head": "GCN" if batched else "GAT", "engine": "batched" if batched else "serial", "partitions": len(parts),
           "nodes": sum(b.x.shape[0] for b in parts), "draws": draws, "q": Q, "mode": "learned", "rounds": rounds, "reps": reps,
           "arms": {arm: {**_summary(times[arm]), "triple": triple[arm]} for arm in arms}, "device": torch.cuda.get_device_name(0)}
    if "off" in times and "auc" in times:
        out["auc_over_off"] = out["arms"]["auc"]["median_s"] / out["arms"]["off"]["median_s"]
        out["auc_minus_off_s"] = out["arms"]["auc"]["median_s"] - out["arms"]["off"]["median_s"]
    return out


def torch_pack(torch, scores, y, masks, C):
    """The keys of sgs_auc_pack by torch ops (include/sgs_hip.h)."""
    N, S = scores.shape
    u = scores.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    img = torch.where(u >= 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000)
    ok = (y >= 0) & (y < C)
    m = (masks[0].to(torch.int64) | (masks[1].to(torch.int64) << 1) | (masks[2].to(torch.int64) << 2)) * ok
    mm = m[:, None] * (~torch.isnan(scores))
    col = torch.arange(S, device=scores.device, dtype=torch.int64)[None, :].expand(N, S)
    pos = (y[:, None] == (torch.ones_like(col) if S == 1 else col)).to(torch.int64) << 3
    return ((col << 36) | (img << 4) | pos | mm).reshape(-1)


def torch_counts(torch, keys, S):
    """int64 [3, S, 3] = {twoU, P, Nn} of packed keys by library ops: one sort, two binary searches per item, one cumsum per split."""
    sk, idx = torch.sort(keys >> 4)
    fl = keys[idx] & 15
    pos = (fl >> 3) & 1
    col = sk >> 32
    b = torch.searchsorted(sk, sk, right=False)
    e1 = torch.searchsorted(sk, sk, right=True)
    out = torch.zeros(3, S, 3, dtype=torch.int64, device=keys.device)
    zero = torch.zeros(1, dtype=torch.int64, device=keys.device)
    for s in range(3):
        m = (fl >> s) & 1
        neg, p = m * (1 - pos), m * pos
        cn0 = torch.cat([zero, torch.cumsum(neg, 0)])                  # cn0[k] = the split's negatives among sorted positions [0, k)
        Nn = torch.zeros(S, dtype=torch.int64, device=keys.device).index_add_(0, col, neg)
        P = torch.zeros(S, dtype=torch.int64, device=keys.device).index_add_(0, col, p)
        base = torch.cumsum(Nn, 0) - Nn
        contrib = p * (cn0[e1] + cn0[b] - 2 * base[col])
        out[s, :, 0] = torch.zeros(S, dtype=torch.int64, device=keys.device).index_add_(0, col, contrib)
        out[s, :, 1], out[s, :, 2] = P, Nn
    return out


def kernels(rounds, iters, torch_only):
    import torch
    import sgs_gnn_amd as S
    ops = S.ops
    dev = "cuda:0"
    res = {"timer": f"two HIP events around back-to-back calls ({iters} for hip and pack, {max(iters // 4, 2)} for torch); microseconds per call; median "
                    f"and [min, max] of {rounds} rounds; arms alternating per round", "device": torch.cuda.get_device_name(0), "shapes": {}}

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / k

    for name, M, Scols in KERNEL_SHAPES:
        C = 2 if Scols == 1 else Scols
        g = torch.Generator().manual_seed(M + Scols)
        lg = 3.0 * torch.randn(M, C, generator=g)
        sure = torch.rand(M, generator=g) < 0.3
        lg[sure, torch.randint(0, C, (int(sure.sum()),), generator=g)] += 40.0
        y = torch.randint(0, C, (M,), generator=g).to(dev)
        u = torch.rand(M, generator=g)
        masks = [(u < 0.2).to(dev), ((u >= 0.2) & (u < 0.6)).to(dev), (u >= 0.6).to(dev)]
        lg = lg.to(dev)
        scores = (lg[:, 1] - lg[:, 0]).unsqueeze(1).contiguous() if C == 2 else torch.log_softmax(lg, 1).contiguous()
        keys = torch_pack(torch, scores, y, masks, C)
        arms = {"torch": (lambda: torch_counts(torch, torch_pack(torch, scores, y, masks, C) if torch_only else keys, Scols), max(iters // 4, 2))}
        ref = torch_counts(torch, keys, Scols)
        entry = {"M": M, "S": Scols, "items": M * Scols, "longest_tie_run": int(torch.unique(keys >> 4, return_counts=True)[1].max())}
        if not torch_only:
            assert torch.equal(ops.auc_pack(scores, y, masks, C), keys), "pack differs from its torch restatement"
            got = ops.auc_counts(keys, Scols)
            assert torch.equal(got, ref), "sgs_auc_counts differs from the torch composition"
            assert torch.equal(ops.auc_counts(keys, Scols), got)
            arms["hip"] = (lambda: ops.auc_counts(ops.auc_pack(scores, y, masks, C), Scols), iters)
            arms["pack"] = (lambda: ops.auc_pack(scores, y, masks, C), iters)
            entry["auc"] = S.auc_from_counts(got.cpu())[0]
        times = {a: [] for a in arms}
        for a, (fn, k) in arms.items():
            timed(fn, 2)                                               # warm-up
        for _ in range(rounds):
            for a, (fn, k) in arms.items():
                times[a].append(timed(fn, k))
        entry["arms"] = {a: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)} for a, t in times.items()}
        if "hip" in times:
            entry["torch_over_hip"] = entry["arms"]["torch"]["median_us"] / entry["arms"]["hip"]["median_us"]
        res["shapes"][name] = entry
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", type=int, default=11)
    ap.add_argument("--shapes", default="s3,s4")
    ap.add_argument("--path", default="all", choices=ARMS + ("all",))
    ap.add_argument("--kernels", action="store_true", help="time ops.auc_pack + ops.auc_counts against the torch composition and nothing else")
    ap.add_argument("--torch-only", action="store_true", help="--kernels: the torch arm alone (a tree without the entry points)")
    ap.add_argument("--iters", type=int, default=20, help="--kernels: calls between the two events")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package and library are measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [s for s in a.shapes.split(",") if s]
    if any(s not in ("s3", "s4") for s in shapes):
        ap.error("--shapes from s3, s4")
    arms = list(ARMS) if a.path == "all" else [a.path]
    sys.path.insert(0, os.path.abspath(a.root))
    import sgs_gnn_amd
    assert os.path.abspath(sgs_gnn_amd.__file__).startswith(os.path.abspath(a.root) + os.sep), "the package came from another tree"
    if a.kernels:
        res = kernels(a.rounds, a.iters, a.torch_only)
    else:
        res = {"timer": "host clock around one ensemble_evaluate pass ending in a device synchronise; median of all passes, [min, max] of the "
                        "per-round medians; arms alternating in one process", "root": "this tree" if a.root == os.path.dirname(HERE) else "--root",
               "shapes": {}}
        for shape in shapes:
            res["shapes"][shape] = measure(shape, arms, a.rounds, a.reps, a.draws)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
