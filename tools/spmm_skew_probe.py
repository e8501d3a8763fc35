"""Row skew in the row-block SpMM kernels: HIP-event medians of every entry point on the GNN head's path, long-row path on and off
(sgs_spmm_long_rows_set), alternating, on three graphs of N = 1013 built on the device:

  skew_small  the S3 stream's smallest partition (~60 000 edges, hub rows of ~900 against a mean of ~60), unsampled
  skew_draw   a 100 000-edge draw (prior weights) of the stream's ~105 000-edge partition: a sampled step that keeps its hubs
  flat        the first graph's nnz spread evenly over the rows (every row nnz / N entries): the yardstick

Timed: sgs_spmm_csr at D = 256 and 41 (the GNN head's widths) and at D = 64, 128, 512 (does the hub cost follow the row's bytes?),
sgs_spmm_csr_next, and sgs_spmm_csr_bwd_prev with the previous layer's product and with the column sums only.
"skewed / flat" of a call says how much of the hub penalty is left (flat has the nnz of skew_small; skew_draw is shown per entry).
One GPU process; prints one JSON document (and writes it to out.json if given).

    python tools/spmm_skew_probe.py [out.json] [--root DIR]

`--root DIR`: the package is imported from DIR (a checkout of another commit with its library built); tools/gcn_spmm_ab.py runs this
tree and the parent's that way, in child processes of their own.
"""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
ROOT = HERE
if "--root" in ARGS:
    ROOT = os.path.abspath(ARGS[ARGS.index("--root") + 1])
    del ARGS[ARGS.index("--root"):ARGS.index("--root") + 2]
sys.path[:0] = [ROOT, HERE]
import torch  # noqa: E402

import sgs_gnn_amd as S  # noqa: E402

assert os.path.abspath(os.path.dirname(S.__file__)).startswith(ROOT), (S.__file__, ROOT)

DEV = "cuda:0"
N, H, C, Q = 1013, 256, 41, 100_000
SMALL, DRAWN = 41, 84                 # indices into reddit_partition_stream(seed=1000): 60 128 and 105 220 target edges
REPS, INNER = 9, 25
ops, L = S.ops, S._lib.lib()


def flat_graph(nnz, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base, rem = divmod(nnz, N)
    lens = base + (torch.arange(N, device=DEV) < rem).long()
    rank = torch.rand(N, N - 1, generator=g, device=DEV).argsort(1).argsort(1)          # per row, a random order of the other nodes
    dst, c = torch.nonzero(rank < lens[:, None], as_tuple=True)
    src = c + (c >= dst).long()
    return torch.stack([src, dst])


def graphs():
    parts = S.reddit_partition_stream(num_parts=DRAWN + 1, seed=1000, nfeat=8, ncls=C, n=N, q=Q, device=DEV, only={SMALL, DRAWN})
    small, big = parts[SMALL], parts[DRAWN]
    smp = ops.sample_topq(ops.SAMPLE_PRIOR, big.prob, None, 0.0, Q, big.edge_index, seed=1, stream_id=1, want_p=False)
    out = {"skew_small": small.edge_index, "skew_draw": smp.edge_index.contiguous()}
    out["flat"] = flat_graph(small.edge_index.shape[1])
    return out


def calls(ei):
    gr = ops.Graph(ei, N)
    nm = ops.gcn_norm(gr)
    n = gr.n_edges
    g = torch.Generator(device=DEV).manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    X256, X41, b256, b41 = r(N, H), r(N, C), r(H), r(C)
    W2, Yp = r(C, H), torch.relu(r(N, H))
    Y256, Y41, Z41, dZp, cs41, cs256 = (torch.empty(*s, device=DEV) for s in ((N, H), (N, C), (N, C), (N, H), (C,), (H,)))
    inp = (gr.in_ptr.data_ptr(), gr.in_src.data_ptr(), nm.what_in.data_ptr(), nm.what_loop.data_ptr())
    outp = (gr.out_ptr.data_ptr(), gr.out_dst.data_ptr(), nm.what_out.data_ptr(), nm.what_loop.data_ptr())
    st = ops._stream()
    ck = ops._lib.check
    keep = (gr, nm, X256, X41, b256, b41, W2, Yp, Y256, Y41, Z41, dZp, cs41, cs256)
    deg = (gr.in_ptr[1:] - gr.in_ptr[:-1]).sort(descending=True).values
    info = {"nnz": n, "mean_row": round(n / N, 1), "longest_rows": deg[:4].tolist(),
            "rows_ge_threshold": int((deg >= L.sgs_spmm_long_rows_threshold()).sum())}
    sweep = {}
    for Dw in (64, 128, 512):
        Xw, Yw = r(N, Dw), torch.empty(N, Dw, device=DEV)
        keep += (Xw, Yw)
        sweep[f"spmm_csr_D{Dw}"] = (lambda Xw=Xw, Yw=Yw, Dw=Dw: ck(L.sgs_spmm_csr(Xw.data_ptr(), N, Dw, n, *inp, None, ops.ACT_NONE, 0.0, 7, 3,
                                                                                 Yw.data_ptr(), st)))
    return info, keep, {
        **sweep,
        "spmm_csr_D256": lambda: ck(L.sgs_spmm_csr(X256.data_ptr(), N, H, n, *inp, b256.data_ptr(), ops.ACT_RELU_DROPOUT, 0.3, 7, 3,
                                                   Y256.data_ptr(), st)),
        "spmm_csr_D41": lambda: ck(L.sgs_spmm_csr(X41.data_ptr(), N, C, n, *inp, b41.data_ptr(), ops.ACT_NONE, 0.0, 7, 3, Y41.data_ptr(), st)),
        "spmm_csr_next_D256_Dn41": lambda: ck(L.sgs_spmm_csr_next(X256.data_ptr(), N, H, n, *inp, b256.data_ptr(), ops.ACT_RELU_DROPOUT, 0.3, 7, 3,
                                                                  W2.data_ptr(), C, Y256.data_ptr(), Z41.data_ptr(), st)),
        "spmm_csr_bwd_prev_D41_W": lambda: ck(L.sgs_spmm_csr_bwd_prev(X41.data_ptr(), N, C, n, *outp, W2.data_ptr(), H, Yp.data_ptr(),
                                                                     ops.ACT_RELU_DROPOUT, 0.3, Y41.data_ptr(), dZp.data_ptr(), cs41.data_ptr(), st)),
        "spmm_csr_bwd_prev_D256_colsum": lambda: ck(L.sgs_spmm_csr_bwd_prev(X256.data_ptr(), N, H, n, *outp, None, 0, None, ops.ACT_NONE, 0.0,
                                                                           Y256.data_ptr(), None, cs256.data_ptr(), st)),
    }


def time_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER * 1e3


def main():
    res = {"threshold": L.sgs_spmm_long_rows_threshold(), "reps": REPS, "inner": INNER, "graphs": {}, "us": {}}
    for name, ei in graphs().items():
        info, keep, fns = calls(ei)
        res["graphs"][name] = info
        for ename, fn in fns.items():
            t = {1: [], 0: []}
            for on in (1, 0):                 # warm both kernels
                L.sgs_spmm_long_rows_set(on)
                fn()
            torch.cuda.synchronize()
            for _ in range(REPS):
                for on in (1, 0):
                    L.sgs_spmm_long_rows_set(on)
                    t[on].append(time_us(fn))
            L.sgs_spmm_long_rows_set(1)
            res["us"].setdefault(ename, {})[name] = {"on": round(statistics.median(t[1]), 2), "off": round(statistics.median(t[0]), 2),
                                                     "on_min_max": [round(min(t[1]), 2), round(max(t[1]), 2)],
                                                     "off_min_max": [round(min(t[0]), 2), round(max(t[0]), 2)]}
    res["skewed_over_flat"] = {e: {sw: round(v["skew_small"][sw] / v["flat"][sw], 3) for sw in ("on", "off")} for e, v in res["us"].items()}
    txt = json.dumps(res, indent=1)
    print(txt)
    if ARGS:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS[0])), exist_ok=True)
        open(ARGS[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
