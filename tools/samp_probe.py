"""HIP-event times of the top-q sampler's draws at the bench partition's size (E = 351 194, q = 100 000; the fused small-E path):
    learned      ops.sample_topq, mode LEARNED with the prior
    prior        ops.sample_topq, mode PRIOR
    cover        the learned draw, node-covering
    multi        ops.sample_topq_multi, D = 11
    multi_cover  the same, node-covering
Each case has its own warm-up and is timed with device events over --repeats windows of --calls calls (50 or more) each; one line
per case with the median, the fastest and the slowest window:
    python tools/samp_probe.py [--calls 50] [--repeats 5] [--cases learned,prior,...]
--once runs each case exactly once and times nothing, for rocprofv3 --kernel-trace: the trace is then the launch list of each entry."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sgs_gnn_amd as S  # noqa: E402
from sgs_gnn_amd import ops  # noqa: E402

CASES = ("learned", "prior", "cover", "multi", "multi_cover")
N, E_TARGET, Q, D, C = 1013, 351194, 100000, 11, 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--once", action="store_true", help="one call per case, no timing (for a kernel trace)")
    a = ap.parse_args()
    assert a.once or a.calls >= 50, "time over at least 50 calls"
    dev = torch.device("cuda:0")
    b = S.synthetic_graph(N, E_TARGET, 16, 5, seed=3, train_frac=0.5, device=dev)
    ei = b.edge_index
    E = ei.shape[1]
    p = torch.rand(E, device=dev)
    logits = torch.randn(E, device=dev)
    graph = ops.get_graph(ei, b.x.shape[0])
    run = {
        "learned": lambda i: ops.sample_topq(ops.SAMPLE_LEARNED, p, b.prob, C, Q, ei, seed=1, stream_id=2 + i),
        "prior": lambda i: ops.sample_topq(ops.SAMPLE_PRIOR, logits, None, 0.0, Q, ei, seed=1, stream_id=2 + i),
        "cover": lambda i: ops.sample_topq(ops.SAMPLE_LEARNED, p, b.prob, C, Q, ei, seed=1, stream_id=2 + i, cover=graph),
        "multi": lambda i: ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, b.prob, C, Q, ei, D, seed=1, stream_id0=2 + D * i),
        "multi_cover": lambda i: ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, b.prob, C, Q, ei, D, seed=1, stream_id0=2 + D * i, cover=graph),
    }
    torch.cuda.synchronize()
    print("tree", os.path.dirname(os.path.abspath(S.__file__)))
    for case in a.cases.split(","):
        f = run[case]
        if a.once:
            f(0)
            torch.cuda.synchronize()
            print(f"case {case} E {E} q {Q} D {D if case.startswith('multi') else 1} once")
            continue
        for i in range(a.warmup):
            f(i)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.calls):
                f(i)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / a.calls * 1e3)
        print(f"case {case} E {E} q {Q} D {D if case.startswith('multi') else 1} calls {a.calls} x {a.repeats} us_per_call median "
              f"{statistics.median(us):.2f} min {min(us):.2f} max {max(us):.2f}")


if __name__ == "__main__":
    main()
