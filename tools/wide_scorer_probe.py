"""Timing of the edge scorer at wide hidden sizes (edge_score_wide_kernel) against the H = 256 fp32-MFMA baseline.

    python tools/wide_scorer_probe.py [--reps 10] [--out FILE]

E = 351 194 candidate edges (the bench's partition size) on an undirected synthetic graph, q = 100 000 active rows for the backward.
Per H: the unpaired forward (sgs_edge_score_fwd), the paired forward (sgs_edge_score_fwd_paired, M canonical edges) and the backward
core (sgs_edge_score_bwd_core, dense dv form).  A launch includes the W1a transpose / pack of that entry point.  TFLOP/s are on ISSUED
flops of the H x H contraction, 2 H^2 per contracted row (E, M or q rows), against the 157.3 TFLOP/s fp32 matrix peak.
At H = 256 the forward is pinned to variant 3 (the 64-edge fp32-MFMA streaming kernel) and the backward to variant 0 (the LDS-tiled
core, the loop the wide kernel sweeps); the paired forward has no fp32-MFMA form at H = 256 (bf16x6), so it is listed for reference."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sgs_gnn_amd as S  # noqa: E402

DEV = "cuda:0"
PEAK_TF = 157.3


def _time(f, reps):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    ops, L = S.ops, S._lib.lib()
    N, E_target, q = 20_000, 351_194, 100_000
    b = S.synthetic_graph(N, E_target, 8, 3, seed=5, device=DEV)
    ei = b.edge_index
    E = ei.shape[1]
    canon, mate = ops.get_pairs(ei, N, build=True)
    M = canon.numel()
    g = torch.Generator(device=DEV).manual_seed(0)
    eid = torch.randperm(E, device=DEV, generator=g)[:q]
    res = {"E": E, "M": M, "q": q, "N": N, "peak_tflops": PEAK_TF, "rows": []}
    for H, fv, bv in ((256, 3, 0), (384, -1, -1), (512, -1, -1), (1024, -1, -1)):
        L.sgs_edge_score_set_variant(fv)
        L.sgs_edge_score_set_bwd_variant(bv)
        codes = torch.relu(torch.randn(N, H, device=DEV, generator=g))
        W1 = torch.randn(H, 2 * H, device=DEV, generator=g) / (2 * H) ** 0.5
        b1 = torch.randn(H, device=DEV, generator=g) * 0.01
        w2 = torch.randn(H, device=DEV, generator=g) / H ** 0.5
        b2 = torch.zeros(1, device=DEV)
        U = (codes @ W1[:, H:].t()).contiguous()
        p_out = torch.empty(E, device=DEV)
        ws = ops.workspace(L.sgs_edge_score_workspace_bytes(N, H, E), codes.device)
        gp = torch.randn(q, device=DEV, generator=g)
        dv, feat, dz = torch.empty(q, H, device=DEV), torch.empty(q, H, device=DEV), torch.empty(q, device=DEV)
        hdz = torch.empty((q + 63) // 64, H, device=DEV)
        st = ops._stream()

        def fwd():
            S._lib.check(L.sgs_edge_score_fwd(codes.data_ptr(), U.data_ptr(), N, H, ei.data_ptr(), E, 0, W1.data_ptr(), b1.data_ptr(),
                                              w2.data_ptr(), b2.data_ptr(), 0.3, 7, 2, p_out.data_ptr(), ws.data_ptr(), ws.numel(), st), "fwd")

        def fwd_paired():
            S._lib.check(L.sgs_edge_score_fwd_paired(codes.data_ptr(), U.data_ptr(), N, H, ei.data_ptr(), E, 0, canon.data_ptr(), M,
                                                     mate.data_ptr(), W1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), 0.3, 7, 2,
                                                     p_out.data_ptr(), ws.data_ptr(), ws.numel(), st), "fwd_paired")

        def bwd():
            S._lib.check(L.sgs_edge_score_bwd_core(codes.data_ptr(), U.data_ptr(), N, H, ei.data_ptr(), E, 0, eid.data_ptr(), q, gp.data_ptr(),
                                                   W1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), 0.3, 7, 2, dv.data_ptr(),
                                                   hdz.data_ptr(), dz.data_ptr(), feat.data_ptr(), ws.data_ptr(), ws.numel(), st), "bwd_core")

        for name, f, rows in (("fwd", fwd, E), ("fwd_paired", fwd_paired, M), ("bwd_core", bwd, q)):
            us = _time(f, o.reps)
            tf = 2.0 * rows * H * H / us / 1e6
            row = {"H": H, "form": name, "us": round(us, 1), "tflops_issued": round(tf, 1), "frac_peak": round(tf / PEAK_TF, 3)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    L.sgs_edge_score_set_variant(-1)
    L.sgs_edge_score_set_bwd_variant(-1)
    txt = json.dumps(res, indent=1)
    print(txt)
    if o.out:
        with open(o.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
