"""Balanced k-way graph partitioning on the device: the node -> partition vector that ResidentPartitions, the cluster loader, the captured
step and sparsify start from, without a host METIS.

Single level: capacity-constrained region growing from P hashed seeds, the leftovers filled by id, then synchronous label-propagation
refinement ("Partitioner").  A sweep is two library calls -- every eligible node proposes the neighbouring part that holds
most of its neighbours (ops.lp_propose), a two-sided commit accepts as many proposals as the target has room for and the source can spare
(ops.lp_commit) -- and everything in it is integer arithmetic, so the result is a pure function of (graph, P, eps, hot, cold, seed) and equals
the numpy restatement in tests/partition_ref.py element for element.  torch is used for the seeding order, the fill and the checks; the growing
phase reads one counter back per sweep, the refinement reads nothing back.  This is one-time set-up work: it is never captured."""
import math

import torch

from . import ops
from .data import fmix32, fmix32_tensor

MAX_PARTS = 4096


def bounds(N: int, P: int, eps: float):
    """-> (cap, lo, base): no part grows above cap, no node leaves a part of lo or fewer, the fill tops parts up to base"""
    return int(math.ceil((1.0 + eps) * N / P)), int(math.floor((1.0 - eps) * N / P)), -(-N // P)


def node_hash(N: int, k: int, device) -> torch.Tensor:
    """H(v, k) = fmix32(v ^ fmix32(k)) for v < N, int64 values below 2^32"""
    return fmix32_tensor(torch.arange(N, dtype=torch.int64, device=device) ^ fmix32(int(k)))


def _check_init(init, N, P, cap, dev):
    ops._need_gpu(init)
    if init.dim() != 1 or init.numel() != N or init.dtype not in (torch.int32, torch.int64):
        raise ValueError("partition_graph: init must be an int tensor with one entry per node")
    if int(init.min()) < 0 or int(init.max()) >= P:
        raise ValueError(f"partition_graph: init holds a value outside [0, {P})")
    sizes = torch.bincount(init.to(torch.int64), minlength=P)
    if int(sizes.max()) > cap:
        raise ValueError(f"partition_graph: init holds a part of {int(sizes.max())} nodes, above cap = {cap} (an over-capacity start is not repaired)")
    return init.to(dev).to(torch.int32).contiguous().clone(), sizes.to(torch.int32)


def partition_graph(edge_index, num_nodes, num_parts, eps=0.05, hot=40, cold=20, seed=0, init=None, report=None):
    """part_id, int64 [N] on the device, of a balanced `num_parts`-way partition of the undirected graph `edge_index` (int64 [2, E] on the
    device, every edge stored both ways; self loops are ignored, repeated edges count with their multiplicity).

    No part holds more than cap = ceil((1 + eps) N / P) nodes.  `hot` refinement sweeps accept zero-gain moves, `cold` further ones only
    strict improvements.  `init` (int tensor [N], values in [0, P), no part above cap) replaces seeding, growing and filling: the given
    partition is refined.  `report`, if a dict, receives sizes, cap, lo, grow_sweeps, filled, cut_edges_initial (after grow + fill, or of
    init), cut_edges (after refinement; both count every undirected edge twice, like E), moved (per refinement sweep) and
    imbalance = max(size) P / N; if it holds a list under "trace", (phase, part clone) pairs are appended to that list after grow, after
    fill and after every refinement sweep."""
    ops._need_gpu(edge_index)
    N, P = int(num_nodes), int(num_parts)
    if not 1 <= P <= min(N, MAX_PARTS):
        raise ValueError(f"partition_graph: num_parts = {P}, need 1 <= num_parts <= min(num_nodes, {MAX_PARTS})")
    if eps < 0 or hot < 0 or cold < 0:
        raise ValueError("partition_graph: eps, hot and cold must not be negative")
    dev = edge_index.device
    cap, lo, base = bounds(N, P, eps)
    if init is not None:                                                # checked once, before anything is launched
        part, size = _check_init(init, N, P, cap, dev)
    g = ops.get_graph(edge_index, N)
    # undirected and stored both ways: at least every node's in-degree equals its out-degree
    if not torch.equal(g.in_ptr, g.out_ptr):
        raise ValueError("partition_graph: the graph must be undirected with every edge stored both ways (in- and out-degrees differ)")
    ptr, col = g.out_ptr, g.out_dst[:g.n_edges]
    trace = report.get("trace") if isinstance(report, dict) and isinstance(report.get("trace"), list) else None
    best = torch.empty(N, dtype=torch.int32, device=dev)
    gain = torch.empty(N, dtype=torch.int32, device=dev)
    grow_sweeps = filled = 0
    if init is None:
        src, dst = edge_index[0], edge_index[1]
        deg = torch.bincount(src[src != dst], minlength=N)
        order = torch.sort(((deg == 0).to(torch.int64) << 32) | node_hash(N, seed, dev), stable=True).indices      # ties: ascending id
        part = torch.full((N,), -1, dtype=torch.int32, device=dev)
        part[order[:P]] = torch.arange(P, dtype=torch.int32, device=dev)
        size = torch.ones(P, dtype=torch.int32, device=dev)
        moved = torch.empty(1, dtype=torch.int32, device=dev)
        while True:
            ops.lp_propose(ptr, col, part, P, ops.LP_UNASSIGNED, 0, 1, best, gain)
            ops.lp_commit(best, gain, part, size, cap, 0, moved)
            grow_sweeps += 1
            if int(moved.item()) == 0:                                   # the one read-back per sweep
                break
        if trace is not None:
            trace.append(("grow", part.clone()))
        left = (part < 0).nonzero().flatten()                           # ascending id
        filled = int(left.numel())
        if filled:
            slots = torch.repeat_interleave(torch.arange(P, dtype=torch.int32, device=dev), (base - size).clamp_(min=0).to(torch.int64))
            part[left] = slots[:filled]
            size = torch.bincount(part.to(torch.int64), minlength=P).to(torch.int32)
        if trace is not None:
            trace.append(("fill", part.clone()))
    cut0 = ops.partition_stats(ptr, col, part, P)[1] if isinstance(report, dict) else None
    sweeps = int(hot) + int(cold)
    moved = torch.zeros(max(sweeps, 1), dtype=torch.int32, device=dev)
    for s in range(sweeps):
        ops.lp_propose(ptr, col, part, P, ops.LP_HASH, seed + 1 + s, 0 if s < hot else 1, best, gain)
        ops.lp_commit(best, gain, part, size, cap, lo, moved[s:s + 1])
        if trace is not None:
            trace.append(("refine", part.clone()))
    if isinstance(report, dict):
        sizes, cut = ops.partition_stats(ptr, col, part, P)
        report.update(sizes=sizes.to(torch.int64), cap=cap, lo=lo, grow_sweeps=grow_sweeps, filled=filled, cut_edges_initial=int(cut0.item()),
                      cut_edges=int(cut.item()), moved=moved[:sweeps].tolist(), imbalance=float(sizes.max().item()) * P / N)
    return part.to(torch.int64)
