"""A/B of the scorer's precision modes ("fp32" / "bf16", include/sgs_hip.h "bf16 mode") in ONE process, the two alternating.

    python tools/precision_ab.py [--reps 6] [--epochs 3] [--only kernels|train] [--precision fp32|bf16]

(a) kernels, at bench S3's largest shape (n = 1 013, H = 256, E = 351 194, q = 100 000 drawn source-sorted active rows), each through its C
    entry with HIP events, `--iters` launches per sample, `--reps` samples per mode alternating the order:
      fwd      the training forward: paired, mask-keeping (sgs_edge_score_fwd_mask[_bf16], pack included)
      prep     dz / mask rows / endpoints + the pack of dfeat's operand (sgs_edge_score_bwd_prep_sd_pack[_bf16])
      dfeat    the fused dfeat + by-source sums (sgs_edge_score_bwd_dfeat_fused_packed[_bf16])
      dW1a     the weight gradient with its slab reduction (sgs_gemm_tn_mask_gather[_bf16])
(c) steady-state epochs of bench S3's stream (data.reddit_partition_stream, 230 partitions, hybrid pipeline, HIP-graph replay, FusedAdam),
    train() with args.sgs_precision, fresh model per run, runs alternating fp32 / bf16: sampled edges / s per epoch;
(d) after those epochs, the F1 triple of ensemble_evaluate (11 draws, batched engine, learned mode) in the run's own precision.
One JSON line per measurement, then a summary line (median / min / max of every series).  `--only` / `--precision` restrict the run (one
mode per process, for a kernel trace of each: rocprofv3 --kernel-trace --stats -- python tools/precision_ab.py --only kernels --precision bf16).
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sgs_gnn_amd as S  # noqa: E402
from sgs_gnn_amd.ops import _ptr, _stream, workspace  # noqa: E402

DEV = "cuda:0"
N_NODES, NFEAT, HID, NCLS, Q = 1013, 602, 256, 41, 100_000


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us per launch


def kernel_cases(E=351_194, seed=3):
    """-> {precision: {kernel: launch()}} on one shared input set."""
    L = S._lib.lib()
    N, H = N_NODES, HID
    g = torch.Generator().manual_seed(seed)
    b = S.synthetic_graph(N, E, 8, 3, seed=seed, device=DEV)              # symmetric, row-sorted
    ei = b.edge_index
    E = ei.shape[1]
    canon, mate = S.ops.get_pairs(ei, N, build=True)
    codes = torch.relu(torch.randn(N, H, generator=g)).to(DEV)
    W1 = ((torch.rand(H, 2 * H, generator=g) * 2 - 1) / (2 * H) ** 0.5).to(DEV)
    b1 = ((torch.rand(H, generator=g) * 2 - 1) / (2 * H) ** 0.5).to(DEV)
    w2 = ((torch.rand(H, generator=g) * 2 - 1) / H ** 0.5).to(DEV)
    b2 = torch.zeros(1, device=DEV)
    U = torch.mm(codes, W1[:, H:].t())
    eid = torch.sort(torch.randperm(E, generator=g)[:Q]).values.to(DEV)
    gq = torch.randn(Q, generator=g).to(DEV)
    p_drop = 0.3
    scale = 1.0 / (1.0 - p_drop)
    f32 = dict(dtype=torch.float32, device=DEV)
    p_out, maskbits = torch.empty(E, **f32), torch.empty(E, H // 32, dtype=torch.int32, device=DEV)
    ws_f = torch.empty(L.sgs_edge_score_workspace_bytes(N, H, E), dtype=torch.uint8, device=DEV)
    ws_d = torch.empty(L.sgs_edge_score_workspace_bytes(0, H, 0), dtype=torch.uint8, device=DEV)
    ws_g = torch.empty(L.sgs_gemm_tn_workspace_bytes(Q, H, H), dtype=torch.uint8, device=DEV)
    dz, bits, sd = torch.empty(Q, **f32), torch.empty(Q, H // 32, dtype=torch.int32, device=DEV), torch.empty(Q, 2, dtype=torch.int32, device=DEV)
    G, opart = torch.empty(Q, H, **f32), torch.empty(L.sgs_edge_score_bwd_fused_opart_rows(Q, N), H, **f32)
    dW1, db1, db2 = torch.empty(H, 2 * H, **f32), torch.empty(H, **f32), torch.empty(1, **f32)
    Traw, craw = torch.empty(H, H, **f32), torch.empty(H, **f32)
    cases = {}
    for pr in ("fp32", "bf16"):
        sfx = "_bf16" if pr == "bf16" else ""
        fwd_fn = getattr(L, "sgs_edge_score_fwd_mask" + sfx)
        prep_fn = getattr(L, "sgs_edge_score_bwd_prep_sd_pack" + sfx)
        dfeat_fn = getattr(L, "sgs_edge_score_bwd_dfeat_fused_packed" + sfx)
        gemm_fn = getattr(L, "sgs_gemm_tn_mask_gather" + sfx)

        def fwd(fwd_fn=fwd_fn):
            S._lib.check(fwd_fn(_ptr(codes), _ptr(U), N, H, _ptr(ei), E, 0, _ptr(canon), canon.numel(), _ptr(mate), _ptr(W1), _ptr(b1), _ptr(w2),
                                _ptr(b2), p_drop, 1, 2, _ptr(p_out), _ptr(maskbits), ws_f.data_ptr(), ws_f.numel(), _stream()), "fwd")

        def prep(prep_fn=prep_fn):
            S._lib.check(prep_fn(_ptr(codes), N, H, _ptr(ei), E, _ptr(eid), Q, _ptr(gq), _ptr(p_out), _ptr(maskbits), _ptr(dz), _ptr(bits), _ptr(sd),
                                 _ptr(W1), _ptr(w2), p_drop, ws_d.data_ptr(), ws_d.numel(), _stream()), "prep")

        def dfeat(dfeat_fn=dfeat_fn):
            S._lib.check(dfeat_fn(_ptr(bits), _ptr(dz), _ptr(sd), _ptr(codes), Q, N, H, _ptr(G), _ptr(opart), ws_d.data_ptr(), ws_d.numel(),
                                  _stream()), "dfeat")

        def gemm(gemm_fn=gemm_fn):
            S._lib.check(gemm_fn(_ptr(bits), _ptr(dz), _ptr(w2), scale, _ptr(codes), N, _ptr(sd), Q, H, H, _ptr(dW1), 2 * H, _ptr(db1), _ptr(db2),
                                 _ptr(Traw), _ptr(craw), ws_g.data_ptr(), ws_g.numel(), _stream()), "dW1a")
        # every launch needs its inputs of ITS mode: the forward's mask, then the prep's pack (the dfeat operand's layout is the mode's)
        cases[pr] = {"fwd": (fwd, ()), "prep": (prep, (fwd,)), "dfeat": (dfeat, (fwd, prep)), "dW1a": (gemm, (fwd, prep))}
    return cases


def run_kernels(args, modes, out):
    cases = kernel_cases()
    for rep in range(args.reps):
        for pr in (modes if rep % 2 == 0 else modes[::-1]):
            for k, (fn, setup) in cases[pr].items():
                for f in setup:
                    f()
                us = _time(fn, args.iters)
                out.setdefault(("kernel", pr, k), []).append(us)
                print(json.dumps({"rep": rep, "precision": pr, "kernel": k, "us": round(us, 1)}), flush=True)


def run_train(args, modes, out):
    pool = S.reddit_partition_stream(num_parts=230, seed=1000, nfeat=NFEAT, ncls=NCLS, n=N_NODES, q=Q, device=DEV)
    P = len(pool)
    for run in range(args.runs):
        for pr in (modes if run % 2 == 0 else modes[::-1]):
            torch.manual_seed(42)
            S.fix_seeds(42)
            m = S.GNNModel(NFEAT, HID, NCLS, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
            og = S.FusedAdam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-3)
            oe = S.FusedAdam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-3)
            oa = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
            crit = torch.nn.CrossEntropyLoss()
            a = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", edge_mlp_type="GCN", conditional=True, sparse_edge_mlp=True,
                                   t_init=0.7, t_min=0.5, degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0,
                                   consist_reg_coef=0.5, hybrid_checkpoint=True, drop_rate=0.3, lr=1e-3, sgs_hipgraph=True, sgs_precision=pr)
            S.prepare_step_graphs(a, m, og, oe, crit, pool, q=Q)
            for e in range(args.epochs + 1):                                  # epoch 0: settle (not recorded)
                batches = [pool[i] for i in random.Random(100 + e).sample(range(P), P)]
                torch.cuda.synchronize()
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                ret = S.train(a, e, 10, m, og, oe, oa, crit, batches, q=Q, alternate_frequency=0)
                t1.record()
                torch.cuda.synchronize()
                if e == 0:
                    continue
                n_s = sum(1 for b in batches if b.edge_index.shape[1] > Q)
                eps = n_s * Q / (t0.elapsed_time(t1) / 1e3)
                out.setdefault(("epoch", pr, "sampled_edges_per_s"), []).append(eps)
                print(json.dumps({"run": run, "precision": pr, "epoch": e, "sampled_edges_per_s": round(eps, 1), "learned_steps": ret[2],
                                  "mean_loss": round(ret[0], 4)}), flush=True)
            ev = argparse.Namespace(**vars(a))
            ev.num_samples_eval, ev.sgs_eval_batch = 11, True
            S.manual_seed(7)
            f1 = S.ensemble_evaluate(ev, m, pool, DEV, q=Q, mode="learned")
            print(json.dumps({"run": run, "precision": pr, "ensemble_f1": [round(float(x), 5) for x in f1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--only", choices=["kernels", "train"], default=None)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default=None)
    args = ap.parse_args()
    modes = [args.precision] if args.precision else ["fp32", "bf16"]
    out = {}
    if args.only in (None, "kernels"):
        run_kernels(args, modes, out)
    if args.only in (None, "train"):
        run_train(args, modes, out)
    summ = {"/".join(k): {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "n": len(v)}
            for k, v in out.items()}
    print(json.dumps({"summary": summ}), flush=True)


if __name__ == "__main__":
    main()
