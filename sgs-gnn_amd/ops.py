"""Host-side wrappers over the C ABI (include/sgs_hip.h): tensor checks, workspace, stream
plumbing and the torch.autograd.Function glue.  PyTorch is used for device memory, streams
and autograd bookkeeping only; every numeric step of the hot path runs in libsgs_hip.so.
Nothing here computes on the CPU: a non-HIP tensor raises."""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

SAMPLE_LEARNED, SAMPLE_PRIOR = 0, 1
ACT_NONE, ACT_RELU, ACT_RELU_DROPOUT = 0, 1, 2

_workspaces = {}
_retired_workspaces = []      # arenas outgrown while HIP graphs may still reference them (pin_workspaces)
_pin_workspaces = False


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("sgs_gnn_amd: the SGS hot path runs only on a HIP device (got a CPU tensor); "
                               "there is no CPU fallback")


def _ptr(t, dtype=None):
    if t is None:
        return None
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"sgs_gnn_amd: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("sgs_gnn_amd: tensor must be contiguous")
    return t.data_ptr()


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream            # fast path: no Stream object per call
except AttributeError:                                         # pragma: no cover
    _raw_stream = None


def _stream():
    """hipStream_t of torch's current stream on the current device, as an integer."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_ws_slot = 0


class workspace_slot:
    """Kernels launched inside this context take their scratch from arena `slot` instead of arena 0.  An arena is reused in
    stream order, so work that may run CONCURRENTLY with the main stream's (stepgraph.py replays the parameter-independent
    prefix of the next partition on a second stream) must be recorded with its own."""

    def __init__(self, slot: int):
        self.slot, self.prev = int(slot), 0

    def __enter__(self):
        global _ws_slot
        self.prev, _ws_slot = _ws_slot, self.slot
        return self

    def __exit__(self, *exc):
        global _ws_slot
        _ws_slot = self.prev
        return False


# Stream ownership of the arenas.  An arena is reused in STREAM ORDER: two kernels that take scratch from the same slot are safe only
# if one stream orders them.  Round 2 lost a bench run to exactly this (a partition's CSR build issued on the prefetch stream took
# scratch from arena 0 while the replayed step's sampler was using it) and fixed it by convention.  The
# guard makes the convention checkable: each slot remembers the raw stream that last took scratch from it, and -- with
# SGS_WS_GUARD=1 (the test suite sets it) -- a request from ANOTHER stream raises, unless the caller declared the hand-over
# (`workspace_handover`: "the current stream has been ordered after the owner", e.g. right after stream.wait_stream(owner)).
_ws_owner = {}
_ws_guard = os.environ.get("SGS_WS_GUARD") == "1"


def set_workspace_guard(on: bool) -> None:
    global _ws_guard
    _ws_guard = bool(on)
    _ws_owner.clear()


def workspace_handover(device=None, slot=None) -> None:
    """The caller has made the CURRENT stream wait for everything issued so far on this device's arenas' owners (wait_stream /
    wait_event / a device synchronisation): the current stream owns every slot (or just `slot`) from here on."""
    if not _ws_guard:
        return
    dev = torch.cuda.current_device() if device is None else (device.index if device.index is not None else torch.cuda.current_device())
    cur = _stream()
    if slot is not None:
        _ws_owner[(dev, int(slot))] = cur
        return
    for key in list(_ws_owner):
        if key[0] == dev:
            _ws_owner[key] = cur


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only per-device scratch arena (stream-ordered reuse on the current stream; see workspace_slot)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _ws_slot)
    if _ws_guard:
        cur = _stream()
        own = _ws_owner.setdefault(key, cur)
        if own != cur:
            raise RuntimeError(f"sgs_gnn_amd: scratch arena {key[1]} of device {key[0]} is owned by stream {own:#x} and was asked for from stream "
                               f"{cur:#x} without a hand-over (ops.workspace_handover): kernels on two streams would share scratch memory; "
                               "use ops.workspace_slot(k) for work that runs beside the main stream")
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None and _pin_workspaces:
            _retired_workspaces.append(ws)
        ws = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def pin_workspaces(on: bool = True) -> None:
    """Once captured HIP graphs hold the arena's address, an outgrown arena must stay allocated."""
    global _pin_workspaces
    _pin_workspaces = _pin_workspaces or bool(on)


# ------------------------------------------------------------------ memo scope
_memo_scope = 0


def memo_scope() -> int:
    """Identifier of the current memo scope: per-step memos (GCNConv's x W^T shared by the learned and the random forward of one
    step) are keyed on it, so they can only be hit inside the step that made them."""
    return _memo_scope


def new_memo_scope() -> int:
    """Open a new scope (called once per batch by train / evaluate): every memo made before is dead from here on."""
    global _memo_scope
    _memo_scope += 1
    return _memo_scope


def drop_memos(module) -> None:
    """Forget every memoised x W^T held by `module`'s layers (after a capture: the memo would point into a graph's pool)."""
    for mod in module.modules():
        if getattr(mod, "_lin_cache", None) is not None:
            mod._lin_cache = None


# ------------------------------------------------------------------ deferred leaf weight gradients
# The node-level weight gradients dW = dY^T x (sgs_gemm_tn) are leaves of a backward pass: nothing in it reads them, only the optimiser
# does.  Inside a `deferred_weight_grads` scope the autograd functions below do not launch such a product where they form it: they
# allocate dW, queue (dY, x, dW) and return dW, and ONE sgs_gemm_tn_group call at the end of the backward (autograd's end-of-backward
# callback) runs all of them -- a launch of 16 .. 152 workgroups is latency-bound, so together they cost about what the largest costs
# alone.  Opt-in: without a scope every product is launched immediately, as before.  Inside one, a product is
# deferred only if nothing can read dW before the flush (_leaf_slot_ok): the parameter's gradient is formed by exactly one node of this
# backward, its .grad is None (AccumulateGrad then takes the tensor as it is) and it carries no hooks.  The flush checks that this is
# what happened -- .grad IS the queued buffer -- and raises otherwise.
GEMM_TN_LAUNCHES = {"single": 0, "group": 0}     # library calls made for leaf weight gradients (tests)
_defer = None                                    # the open deferred_weight_grads scope
_defer_enabled = True                            # False: the scopes do nothing (A/B switch: set_deferred_weight_grads)


def set_deferred_weight_grads(on: bool) -> None:
    """A/B switch (tests, tools): with False every deferred_weight_grads scope is inert and each product is launched where it is formed."""
    global _defer_enabled
    _defer_enabled = bool(on)


class deferred_weight_grads:
    """with deferred_weight_grads(loss): loss.backward(...) -- see above.  `roots`: the tensors backward() is called on (their graph is
    walked once, to count the gradient producers of every parameter)."""

    def __init__(self, *roots):
        self.roots = roots
        self.producers, self.queue, self.armed, self.prev = {}, [], False, None

    def __enter__(self):
        global _defer
        self.prev = _defer
        if not _defer_enabled:
            return self
        seen, stack = set(), [r.grad_fn for r in self.roots if r.grad_fn is not None]
        prod = self.producers = {}
        while stack:
            fn = stack.pop()
            if fn in seen:
                continue
            seen.add(fn)
            for nxt, _ in fn.next_functions:
                if nxt is None:
                    continue
                if hasattr(nxt, "variable"):                   # AccumulateGrad
                    prod[nxt] = prod.get(nxt, 0) + 1
                else:
                    stack.append(nxt)
        self.queue, self.armed = [], False
        self.prev, _defer = _defer, self
        return self

    def __exit__(self, *exc):
        global _defer
        _defer = self.prev
        pending = len(self.queue)
        self.queue, self.producers, self.armed = [], {}, False          # (a backward that raised never reaches its callback)
        if pending and exc[0] is None:
            raise RuntimeError("sgs_gnn_amd: deferred weight gradients were queued but the backward pass ended without flushing them")
        return False

    def _leaf_slot_ok(self, ctx, slot):
        """The AccumulateGrad node behind input `slot` of the running backward node if dW may be deferred, else None."""
        node = ctx.next_functions[slot][0]
        if node is None or self.producers.get(node) != 1:
            return None
        p = node.variable
        if p.grad is not None or getattr(p, "_backward_hooks", None) or getattr(p, "_post_accumulate_grad_hooks", None):
            return None
        return node

    def _enqueue(self, node, dY, x, grad, c_ptr, K, M, N, ldc):
        if not self.armed:
            torch.autograd.Variable._execution_engine.queue_callback(self._flush)
            self.armed = True
        # (the operands are kept alive -- and their memory out of the allocator's hands -- until the flush; `grad` is NOT: a second
        # reference would make AccumulateGrad copy the still unwritten tensor instead of taking it)
        self.queue.append((node, dY, x, grad.data_ptr(), c_ptr, K, M, N, ldc, grad.device.index))

    def _flush(self):
        q, self.queue, self.armed = self.queue, [], False
        if not q:
            return
        L = _lib.lib()
        for node, _, _, base, *_ in q:
            g = node.variable.grad
            if g is None or g.data_ptr() != base:
                raise RuntimeError("sgs_gnn_amd: a deferred weight gradient did not become its parameter's .grad as it was (the values "
                                   "autograd passed on were read before they were written)")
        words = []
        for _, dY, x, _, c_ptr, K, M, N, ldc, _ in q:
            words += [dY.data_ptr(), x.data_ptr(), K, M, N, c_ptr, ldc, 0, 0]
        arr = (ctypes.c_int64 * len(words))(*words)
        dev = q[0][9]
        stream = _raw_stream(dev) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream
        GEMM_TN_LAUNCHES["group"] += 1
        _lib.check(L.sgs_gemm_tn_group(arr, len(q), stream), "sgs_gemm_tn_group")


def _leaf_dw(dY, x, K, M, N, leaf=None, out=None, col0=0):
    """dW [M, N] = dY^T x by sgs_gemm_tn, written into `out` [M, ldc] from column col0 on when given (else a new tensor).  `leaf` =
    (ctx, input slot) of the weight in the running backward node: inside a deferred_weight_grads scope the product joins the scope's
    grouped launch when it may (see there); otherwise it is launched here."""
    L = _lib.lib()
    dW = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=x.device)
    ldc = dW.shape[1]
    c_ptr = _ptr(dW) + 4 * col0
    dY_p, x_p = _ptr(dY, torch.float32), _ptr(x, torch.float32)
    if _defer is not None and leaf is not None and L.sgs_gemm_tn_group_supported(K, M, N) > 0:
        node = _defer._leaf_slot_ok(*leaf)
        if node is not None:
            _defer._enqueue(node, dY, x, dW, c_ptr, K, M, N, ldc)
            return dW
    ws = workspace(L.sgs_gemm_tn_workspace_bytes(K, M, N), x.device)
    GEMM_TN_LAUNCHES["single"] += 1
    if out is None:
        _lib.check(L.sgs_gemm_tn(dY_p, x_p, K, M, N, c_ptr, ws.data_ptr(), ws.numel(), _stream()), "sgs_gemm_tn")
    else:
        _lib.check(L.sgs_gemm_tn_ld(dY_p, x_p, K, M, N, c_ptr, ldc, None, ws.data_ptr(), ws.numel(), _stream()), "sgs_gemm_tn_ld")
    return dW


# ------------------------------------------------------------------ randomness
_rng_epoch = None       # keeps the registered device word alive


def set_rng_epoch_buffer(epoch) -> None:
    """Register (or clear with None) the device word every RNG-consuming kernel folds into its seed
    (sgs_rng_set_epoch_buffer): a HIP graph that increments it draws fresh noise on every replay."""
    global _rng_epoch
    L = _lib.lib()
    if epoch is not None:
        _need_gpu(epoch)
        if epoch.dtype != torch.int64 or epoch.numel() != 1:
            raise RuntimeError("sgs_gnn_amd: the RNG epoch buffer is one int64 device word")
    _lib.check(L.sgs_rng_set_epoch_buffer(None if epoch is None else epoch.data_ptr()), "sgs_rng_set_epoch_buffer")
    _rng_epoch = epoch


_dyn_edges = None       # keeps the registered device word alive


def set_dyn_edges(word) -> None:
    """Register (or clear with None) the device word holding the live candidate-edge count (sgs_dyn_edges_set): kernels over the
    candidate edges launched while it is registered -- i.e. captured into a HIP graph -- take their size from it at run time."""
    global _dyn_edges
    L = _lib.lib()
    if word is not None:
        _need_gpu(word)
        if word.dtype != torch.int64 or word.numel() not in (1, 2):
            raise RuntimeError("sgs_gnn_amd: the dynamic sizes are one or two int64 device words (live E[, live canonical edges])")
    _lib.check(L.sgs_dyn_edges_set(None if word is None else word.data_ptr()), "sgs_dyn_edges_set")
    _dyn_edges = word


def exp_noise(seed: int, stream_id: int, E: int, device) -> torch.Tensor:
    L = _lib.lib()
    out = torch.empty(E, dtype=torch.float32, device=device)
    _need_gpu(out)
    _lib.check(L.sgs_exp_noise(seed, stream_id, E, _ptr(out), _stream()), "sgs_exp_noise")
    return out


def dropout_keep(seed: int, site: int, rows: int, cols: int, p: float, device) -> torch.Tensor:
    L = _lib.lib()
    out = torch.empty(rows, cols, dtype=torch.uint8, device=device)
    _need_gpu(out)
    _lib.check(L.sgs_dropout_keep(seed, site, rows, cols, p, _ptr(out), _stream()), "sgs_dropout_keep")
    return out.bool()


# ------------------------------------------------------------------ sampler
class SampleResult:
    __slots__ = ("mask", "eid", "edge_index", "p", "stats", "keys", "E", "q", "cover_info")

    def check(self) -> None:
        """torch.multinomial(replacement=False) raises when fewer than q categories have a positive weight; the fused draw cannot
        raise from the device.  It reports the case through `stats`: the threshold key is then 0 (zero-weight edges were admitted
        by the lowest-id tie-break).  Calling this reads stats back (one synchronisation) and raises like the reference.
        (A covering draw reports the threshold without its flag bit, so the meaning is the same there.)"""
        if self.q > 0 and float(self.stats[2]) <= 0.0:
            raise RuntimeError("invalid multinomial distribution (with replacement=False, not enough non-negative category to sample)")


def sample_topq(mode: int, p: torch.Tensor, prior, c: float, q: int, edge_index, noise=None, seed: int = 0,
                stream_id: int = 0, want_keys: bool = False, want_p: bool = True, cover: "Graph | None" = None) -> SampleResult:
    """K0/K2/K3 (see sgs_sample_topq).  p [E] f32 (None: uniform weights); prior [E] f32 or None; edge_index [2,E] i64.
    `cover`: the Graph of the candidate edges (get_graph(edge_index, N)) makes it a node-covering draw (sgs_sample_topq_cover: every
    node keeps its best non-loop in-edge while the budget lasts); the result then carries cover_info int32 [2] = {M, min(M, q)}."""
    L = _lib.lib()
    _need_gpu(p, prior, edge_index, noise)
    if p is None and edge_index is None:
        raise RuntimeError("sample_topq: uniform weights (p=None) need edge_index for the number of candidates")
    E = p.numel() if p is not None else edge_index.shape[1]
    dev = p.device if p is not None else edge_index.device
    if q > E:
        raise RuntimeError(f"cannot sample q={q} > E={E} edges without replacement")
    r = SampleResult()
    r.E, r.q = E, q
    r.mask = torch.empty(E, dtype=torch.bool, device=dev)
    r.eid = torch.empty(q, dtype=torch.int64, device=dev)
    r.edge_index = torch.empty(2, q, dtype=torch.int64, device=dev) if edge_index is not None else None
    r.p = torch.empty(q, dtype=torch.float32, device=dev) if (want_p and p is not None) else None
    r.stats = torch.empty(4, dtype=torch.float32, device=dev)
    r.keys = torch.empty(E, dtype=torch.float32, device=dev) if want_keys else None
    r.cover_info = None
    if cover is not None:
        if not isinstance(cover, Graph) or cover.n_edges != E:
            raise RuntimeError(f"sample_topq: cover must be the Graph of the E={E} candidate edges"
                               + (f" (it has {cover.n_edges})" if isinstance(cover, Graph) else ""))
        r.cover_info = (torch.empty if E > 0 else torch.zeros)(2, dtype=torch.int32, device=dev)      # (E == 0: the call writes nothing)
        ws = workspace(L.sgs_sample_topq_cover_workspace_bytes(E, cover.N), dev)
        _lib.check(L.sgs_sample_topq_cover(mode, _ptr(p, torch.float32), _ptr(prior, torch.float32), float(c),
                                           _ptr(noise, torch.float32), seed, stream_id, E, q, _ptr(edge_index, torch.int64),
                                           cover.N, _ptr(cover.in_ptr), _ptr(cover.in_src), _ptr(cover.in_eid),
                                           _ptr(r.mask), _ptr(r.eid), _ptr(r.edge_index), _ptr(r.p), _ptr(r.stats),
                                           _ptr(r.keys), _ptr(r.cover_info), ws.data_ptr(), ws.numel(), _stream()), "sgs_sample_topq_cover")
        return r
    nws = L.sgs_sample_topq_workspace_bytes(E)
    ws = workspace(nws, dev)
    _lib.check(L.sgs_sample_topq(mode, _ptr(p, torch.float32), _ptr(prior, torch.float32), float(c),
                                 _ptr(noise, torch.float32), seed, stream_id, E, q, _ptr(edge_index, torch.int64),
                                 _ptr(r.mask), _ptr(r.eid), _ptr(r.edge_index), _ptr(r.p), _ptr(r.stats),
                                 _ptr(r.keys), ws.data_ptr(), ws.numel(), _stream()), "sgs_sample_topq")
    return r


def gather_columns(edge_index: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """edge_index[:, idx] (sampling.py:163) as one launch."""
    L = _lib.lib()
    _need_gpu(edge_index, idx)
    q = idx.numel()
    out = torch.empty(2, q, dtype=torch.int64, device=edge_index.device)
    _lib.check(L.sgs_gather_columns(_ptr(edge_index, torch.int64), edge_index.shape[1], _ptr(idx.contiguous(), torch.int64), q, _ptr(out),
                                    _stream()), "sgs_gather_columns")
    return out


class _STWeights(torch.autograd.Function):
    """sampling.py:137-138,155: clamp(p * ((one_hot - s).detach() + s), 0, 1)[mask]."""

    @staticmethod
    def forward(ctx, p, prior, c, stats, eid):
        L = _lib.lib()
        E, q = p.numel(), eid.numel()
        w = torch.empty(q, dtype=torch.float32, device=p.device)
        _lib.check(L.sgs_st_weights_fwd(_ptr(p, torch.float32), _ptr(prior, torch.float32), float(c), _ptr(stats),
                                        _ptr(eid, torch.int64), E, q, _ptr(w), _stream()), "sgs_st_weights_fwd")
        ctx.save_for_backward(p, prior if prior is not None else torch.empty(0, device=p.device), stats, eid)
        ctx.c, ctx.has_prior = float(c), prior is not None
        return w

    @staticmethod
    def backward(ctx, gw):
        L = _lib.lib()
        p, prior, stats, eid = ctx.saved_tensors
        prior = prior if ctx.has_prior else None
        E, q = p.numel(), eid.numel()
        gw = gw.contiguous()
        gp = torch.empty(E, dtype=torch.float32, device=p.device)
        nws = L.sgs_st_weights_bwd_workspace_bytes(E, q)
        ws = workspace(nws, p.device)
        _lib.check(L.sgs_st_weights_bwd(_ptr(p), _ptr(prior), ctx.c, _ptr(stats), _ptr(eid), _ptr(gw), E, q, _ptr(gp),
                                        ws.data_ptr(), ws.numel(), _stream()), "sgs_st_weights_bwd")
        return gp, None, None, None, None


_zero_tokens = {}


def _zero_token(device) -> torch.Tensor:
    """One persistent zero per device; `.expand(E)` of it is the "all zeros, look at ActiveSet.gq" gradient below (no launch)."""
    key = (device.type, device.index)
    t = _zero_tokens.get(key)
    if t is None:
        t = _zero_tokens[key] = torch.zeros(1, dtype=torch.float32, device=device)
    return t


class _SelectSampled(torch.autograd.Function):
    """probs[eid] with the VALUES the sampler's compaction already gathered (sgs_sample_topq's sampled_p): the forward
    launches nothing; the backward is index_select's (scatter of the q gradients into zeros [E]; the eids are unique).
    With `active` (the scorer's ActiveSet for these very edges, hybrid pipeline) the q gradients are handed to the scorer's
    backward directly (`active.gq`) and the [E] gradient that autograd wants is a stride-0 view of a persistent zero: the
    zero-fill of [E], the scatter and the scorer's gather back to [q] -- three launches -- disappear."""

    @staticmethod
    def forward(ctx, probs, eid, values, active):
        ctx.save_for_backward(eid)
        ctx.E, ctx.active = probs.numel(), active
        return values.view_as(values)

    @staticmethod
    def backward(ctx, g):
        (eid,) = ctx.saved_tensors
        act = ctx.active
        if act is not None and act.eid is not None and act.eid.data_ptr() == eid.data_ptr() and act.eid.numel() == eid.numel():
            act.gq = g.contiguous()
            return _zero_token(g.device).expand(ctx.E), None, None, None
        gp = torch.zeros(ctx.E, dtype=g.dtype, device=g.device)
        gp.index_copy_(0, eid, g.contiguous())
        return gp, None, None, None


def select_sampled(probs, eid, values, active=None):
    _need_gpu(probs, eid, values)
    return _SelectSampled.apply(probs, eid, values, active)


def st_weights(p, prior, c, stats, eid):
    _need_gpu(p, prior, stats, eid)
    return _STWeights.apply(p.contiguous(), prior, c, stats, eid)


# ------------------------------------------------------------------ graph + GCN
class Graph:
    """Both CSR orientations of one edge list (sgs_graph_build).  Built once per sampled graph
    and shared by every layer / pass that runs over it.  Results that depend on the graph alone are cached on the object (`_norm_unit`,
    `_cheb_norm_unit`, `_norm_sum`).  A step-graph slot's graph (stepgraph.py) carries `restaged = True`: its arrays are refilled for every
    partition, so a cached result is only valid if the slot stages it too (gcn_norm: the slot pre-seeds `_norm_unit` and copies the
    partition's own into it); cheb_norm honours the flag and does not cache there."""

    def __init__(self, edge_index: torch.Tensor, N: int):
        L = _lib.lib()
        _need_gpu(edge_index)
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise RuntimeError("edge_index must be an int64 [2, E] tensor")
        ei = edge_index.contiguous()
        dev = ei.device
        n = ei.shape[1]
        self.edge_index, self.n_edges, self.N = ei, n, int(N)
        # one allocation, seven views (host time matters: the step is launch-bound at partition scale)
        ne = max(n, 1)
        sizes = [N + 1, N + 1, ne, ne, ne, ne, max(N, 1)]
        offs = [0]
        for z in sizes:
            offs.append(offs[-1] + ((z + 63) & ~63))             # keep every view 256-B aligned
        buf = torch.empty(offs[-1], dtype=torch.int32, device=dev)
        (self.in_ptr, self.out_ptr, self.in_src, self.in_eid, self.out_dst, self.out_eid, self.loop_eid) = (
            buf[offs[i]:offs[i] + sizes[i]] for i in range(7))
        nws = L.sgs_graph_build_workspace_bytes(n, N)
        ws = workspace(nws, dev)
        _lib.check(L.sgs_graph_build(_ptr(ei), n, N, _ptr(self.in_ptr), _ptr(self.in_src), _ptr(self.in_eid),
                                     _ptr(self.out_ptr), _ptr(self.out_dst), _ptr(self.out_eid), _ptr(self.loop_eid),
                                     ws.data_ptr(), ws.numel(), _stream()), "sgs_graph_build")


_SORT_SUBGRAPH_EDGES = int(os.environ.get("SGS_SORT_SUBGRAPH_EDGES", 1 << 22))     # drawn edges from which get_subgraph sorts instead of filtering


def get_subgraph(parent_edge_index: torch.Tensor, N: int, sample, eid=None) -> Graph:
    """CSR of a drawn subgraph (`sample` = SampleResult of a draw over `parent_edge_index`) squeezed out of the parent's cached
    CSR (sgs_graph_filter): no atomics and no per-row sort, identical arrays to Graph(sample.edge_index).  The result is cached
    on `sample.edge_index`, so every later get_graph() on the drawn edge list reuses it.  `eid`: the selected edges' positions in
    `parent_edge_index` when they differ from `sample.eid` (edge-sharded draws report GLOBAL ids: pass the local ones)."""
    L = _lib.lib()
    parent = get_graph(parent_edge_index, N)
    ei = sample.edge_index
    n = ei.shape[1]
    g = Graph.__new__(Graph)
    g.edge_index, g.n_edges, g.N = ei, n, int(N)
    ne = max(n, 1)
    sizes = [N + 1, N + 1, ne, ne, ne, ne, max(N, 1)]
    offs = [0]
    for z in sizes:
        offs.append(offs[-1] + ((z + 63) & ~63))
    buf = torch.empty(offs[-1], dtype=torch.int32, device=ei.device)
    (g.in_ptr, g.out_ptr, g.in_src, g.in_eid, g.out_dst, g.out_eid, g.loop_eid) = (buf[offs[i]:offs[i] + sizes[i]] for i in range(7))
    if n >= _SORT_SUBGRAPH_EDGES and src_sorted(parent_edge_index):
        # whole-graph scale: one packed radix sort of the DRAWN edges instead of two passes over the parent's CSR (sgs_graph_build_src_sorted)
        ws = workspace(L.sgs_graph_build_src_sorted_workspace_bytes(n, N), ei.device)
        _lib.check(L.sgs_graph_build_src_sorted(_ptr(ei), n, N, _ptr(g.in_ptr), _ptr(g.in_src), _ptr(g.in_eid), _ptr(g.out_ptr), _ptr(g.out_dst),
                                                _ptr(g.out_eid), _ptr(g.loop_eid), None, ws.data_ptr(), ws.numel(), _stream()),
                   "sgs_graph_build_src_sorted")
        try:
            ei._sgs_graph = g
            ei._sgs_graph_version = ei._version
        except Exception:
            pass
        return g
    ws = workspace(L.sgs_graph_filter_workspace_bytes(parent.n_edges, N), ei.device)
    _lib.check(L.sgs_graph_filter(_ptr(parent.in_ptr), _ptr(parent.in_src), _ptr(parent.in_eid), _ptr(parent.out_ptr), _ptr(parent.out_dst),
                                  _ptr(parent.out_eid), parent.n_edges, N, _ptr(_u8(sample.mask)), _ptr(sample.eid if eid is None else eid, torch.int64), n,
                                  _ptr(g.in_ptr), _ptr(g.in_src), _ptr(g.in_eid), _ptr(g.out_ptr), _ptr(g.out_dst), _ptr(g.out_eid),
                                  _ptr(g.loop_eid), ws.data_ptr(), ws.numel(), _stream()), "sgs_graph_filter")
    try:
        ei._sgs_graph = g
        ei._sgs_graph_version = ei._version
    except Exception:
        pass
    return g


def get_graph(edge_index: torch.Tensor, N: int) -> Graph:
    """Graph for `edge_index`, cached ON the tensor object (dies with it; keyed by its version
    counter), so the encoder and the GNN that receive the same tensor share one build."""
    g = getattr(edge_index, "_sgs_graph", None)
    if g is None or g.N != N or getattr(edge_index, "_sgs_graph_version", -1) != edge_index._version:
        g = Graph(edge_index, N)
        try:
            edge_index._sgs_graph = g
            edge_index._sgs_graph_version = edge_index._version
        except Exception:
            pass
    return g


def get_pairs(edge_index: torch.Tensor, N: int, build: bool = False):
    """(canon int32 [M], mate int32 [E]) of the paired scorer forward (sgs_edge_mates / sgs_edge_score_fwd_paired), cached on the
    tensor like its Graph; None when it has not been built.  `build=True` builds it (two launches over the cached CSR + one
    compaction with a read-back of M: set-up work, done once per partition by the trainers, never inside a captured step)."""
    c = getattr(edge_index, "_sgs_pairs", None)
    if c is not None and c[2] == edge_index._version:
        return c[0], c[1]
    if not build:
        return None
    L = _lib.lib()
    _need_gpu(edge_index)
    g = get_graph(edge_index, N)
    E = g.n_edges
    dev = edge_index.device
    mate = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    if E > 0:
        ws = workspace(L.sgs_edge_mates_workspace_bytes(E), dev)
        _lib.check(L.sgs_edge_mates(_ptr(g.edge_index), E, N, _ptr(g.out_ptr), _ptr(g.out_dst), _ptr(g.out_eid), _ptr(mate), ws.data_ptr(),
                                    ws.numel(), _stream()), "sgs_edge_mates")
    ar = torch.arange(E, dtype=torch.int32, device=dev)
    canon = ar[(mate[:E] < 0) | (ar < mate[:E])].contiguous()
    try:
        edge_index._sgs_pairs = (canon, mate, edge_index._version)
    except Exception:
        pass
    return canon, mate


class Norm:
    """gcn_norm result for (graph, w): dis, loopw and the normalised weights in both CSR orders.
    `handle` is the autograd edge through which the layers' gradients wrt the normalised
    weights ([n_edges] edge order + [N] loops) flow back to `w`; its storage is never read."""
    __slots__ = ("graph", "w", "dis", "loopw", "what_in", "what_out", "what_loop", "handle", "_g_first", "_g_extra", "_dw_first", "_park_ok",
                 "_extra_total", "__weakref__")

    def __init__(self):
        self.graph = self.w = self.dis = self.loopw = self.what_in = self.what_out = self.what_loop = self.handle = None
        self._g_first = self._g_extra = self._dw_first = None          # the edge-weight gradient side band: see _handle_grad
        self._park_ok = self._extra_total = False


def _norm_forward(graph: Graph, w):
    L = _lib.lib()
    dev = graph.edge_index.device
    nm = Norm()
    nm.graph, nm.w = graph, w
    ne, Nn = max(graph.n_edges, 1), graph.N
    sizes = [Nn, Nn, ne, ne, Nn]
    offs = [0]
    for z in sizes:
        offs.append(offs[-1] + ((z + 63) & ~63))
    buf = torch.empty(offs[-1], dtype=torch.float32, device=dev)
    nm.dis, nm.loopw, nm.what_in, nm.what_out, nm.what_loop = (buf[offs[i]:offs[i] + sizes[i]] for i in range(5))
    _lib.check(L.sgs_gcn_norm_fwd(_ptr(w, torch.float32), graph.n_edges, graph.N, _ptr(graph.in_ptr), _ptr(graph.in_src),
                                  _ptr(graph.in_eid), _ptr(graph.out_ptr), _ptr(graph.out_dst), _ptr(graph.out_eid),
                                  _ptr(graph.loop_eid), _ptr(nm.dis), _ptr(nm.loopw), _ptr(nm.what_in), _ptr(nm.what_out),
                                  _ptr(nm.what_loop), _stream()), "sgs_gcn_norm_fwd")
    return nm


class _GCNNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, graph, box):
        nm = _norm_forward(graph, w)
        box.append(nm)
        ctx.nm = nm
        return torch.empty(graph.n_edges + graph.N, dtype=torch.float32, device=w.device)

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        nm, gr = ctx.nm, ctx.nm.graph
        g = g.contiguous()
        n = gr.n_edges
        extra, _, first = _take_parked(nm)                # the side band: see _handle_grad
        if first is not None and (first.numel() != n or not first.is_contiguous() or first.dtype != torch.float32):
            first = None
        dw = first if first is not None else torch.empty(n, dtype=torch.float32, device=g.device)
        if n > 0:
            gw, gl = g[:n], g[n:]
            g2w = g2l = None
            if extra is not None and extra.numel() == g.numel():
                g2w, g2l = extra[:n].data_ptr(), extra[n:].data_ptr()
            elif extra is not None:
                g = g + extra
                gw, gl = g[:n], g[n:]
            nws = L.sgs_gcn_norm_bwd_workspace_bytes(gr.N)
            ws = workspace(nws, g.device)
            _lib.check(L.sgs_gcn_norm_bwd_sum(_ptr(nm.w), gw.data_ptr(), gl.data_ptr(), g2w, g2l, None if first is None else first.data_ptr(), n, gr.N,
                                              _ptr(nm.dis), _ptr(nm.loopw), _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid), _ptr(gr.out_ptr),
                                              _ptr(gr.out_dst), _ptr(gr.out_eid), _ptr(gr.loop_eid), _ptr(gr.edge_index), _ptr(dw), ws.data_ptr(),
                                              ws.numel(), _stream()), "sgs_gcn_norm_bwd_sum")
        return (None if first is not None else dw), None, None


def _handle_grad(nm, g):
    """What a layer's backward returns for the handle of the Norm (or EdgeAttr) it ran over -- and the one description of the side band
    through which the edge weights' gradient is handed over without autograd's add launches.

    The layers of a model share one Norm, so autograd would add their gradients with a launch of its own before the Norm's backward.
    Instead, on a Norm whose backward reads the side band (`_park_ok`: set by gcn_norm, cheb_norm and gat_edge_attr when they make a
    handle; False everywhere else, and then every layer simply returns its gradient):
      * who parks.  The first layer to finish is noted in `_g_first` and returns its gradient as usual.  The second parks its own in
        `_g_extra` and returns None; later ones return theirs again.  The edge-attribute layers (edge GAT, GATv2, GINE) first ask
        _dw_to_add for the noted gradient and add it inside their own kernel, so that what they park is already the total; _report_dw
        then says so in `_extra_total`.  The hybrid loss parks a weak reference to its own d w in `_dw_first` (GCN norms only).
      * who reads.  The three handle backwards, through _take_parked: _GCNNorm (the kernel sums `_g_extra` on read and accumulates into
        `_dw_first` in place), _ChebNorm (`_g_extra` summed on read) and _GATEdgeAttr (`_g_extra` added, or returned as it is when it is
        the total).  Each runs after every layer over the Norm has reported, so a parked gradient has exactly one consumer.
      * who resets.  _take_parked, and nobody else: after a backward the side band is neutral again."""
    if not nm._park_ok:
        return g
    if nm._g_first is None:
        nm._g_first = g
        return g
    if nm._g_extra is None:
        nm._g_extra = g
        return None
    return g


def _dw_to_add(nm, n):
    """(second, dw_add) for an edge-attribute layer about to form its d w [n]: the other layer's, if it has reported already and nothing
    is parked yet, to be added by this layer's own kernel (_handle_grad)."""
    second = nm._park_ok and nm._g_first is not None and nm._g_extra is None and nm._g_first.numel() == n
    return second, (nm._g_first.contiguous() if second else None)


def _report_dw(nm, dw, second):
    """_handle_grad for a d w formed with _dw_to_add's `second`: when it is parked, it holds both layers' sum."""
    g_handle = _handle_grad(nm, dw)
    if second and g_handle is None:
        nm._extra_total = True
    return g_handle


def _take_parked(nm):
    """(extra, total, first): the parked gradient, whether it is already the layers' sum, and the loss's live d w (or None); the side
    band is neutral afterwards (_handle_grad)."""
    extra, total, first = nm._g_extra, nm._extra_total, nm._dw_first
    nm._g_first = nm._g_extra = nm._dw_first = None
    nm._extra_total = False
    return extra, total, (first() if first is not None else None)


def gcn_norm(graph: Graph, w=None) -> Norm:
    """K4.  `w` [n_edges] f32 or None (unit weights).  The unit-weight result depends on the graph alone and is kept on it:
    the scorer's encoder and the GNN's random forward normalise the same random subgraph (training_hybrid.py:52,93)."""
    if w is None:
        nm = getattr(graph, "_norm_unit", None)
        if nm is None:
            nm = graph._norm_unit = _norm_forward(graph, None)
        return nm
    _need_gpu(w)
    w = w.contiguous()
    if w.dtype != torch.float32 or w.numel() != graph.n_edges:
        raise RuntimeError(f"edge_weight must be float32 [{graph.n_edges}]")
    if not (w.requires_grad and torch.is_grad_enabled()):
        return _norm_forward(graph, w.detach())
    box = []
    handle = _GCNNorm.apply(w, graph, box)
    nm = box[0]
    nm.handle = handle
    nm._park_ok = True
    try:
        import weakref
        w._sgs_norm = weakref.ref(nm)          # (note_first_dw: the loss finds the normalisation that differentiates these weights)
    except Exception:
        pass
    return nm


def _spmm(X, ptr, col, val, diag, bias, act, p, seed, site, N, D, nnz):
    L = _lib.lib()
    Y = torch.empty(N, D, dtype=torch.float32, device=X.device)
    _lib.check(L.sgs_spmm_csr(_ptr(X, torch.float32), N, D, nnz, _ptr(ptr), _ptr(col), _ptr(val), _ptr(diag), _ptr(bias),
                              act, float(p), seed, site, _ptr(Y), _stream()), "sgs_spmm_csr")
    return Y


class _Propagate(torch.autograd.Function):
    """Y = act(A_hat X + bias); A_hat from `nm` (K5 forward + its three backward products)."""

    @staticmethod
    def forward(ctx, X, handle, bias, nm, act, p, seed, site):
        gr = nm.graph
        N, D = X.shape
        Y = _spmm(X, gr.in_ptr, gr.in_src, nm.what_in, nm.what_loop, bias, act, p, seed, site, N, D, gr.n_edges)
        ctx.nm, ctx.act, ctx.p = nm, act, p
        ctx.has_bias, ctx.has_handle = bias is not None, handle is not None
        ctx.save_for_backward(X, Y if act != ACT_NONE else None)
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = _lib.lib()
        nm, gr = ctx.nm, ctx.nm.graph
        X, Y = ctx.saved_tensors
        N, D = X.shape
        dY = dY.contiguous()
        dX = g = None
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        dZ, dbias = _grad_through_act(dY, Y, ctx.act, ctx.p, want_db, colsum_now=False)
        if ctx.needs_input_grad[0]:
            dX = _spmm(dZ, gr.out_ptr, gr.out_dst, nm.what_out, nm.what_loop, None, ACT_NONE, 0.0, 0, 0, N, D, gr.n_edges)
        if ctx.has_handle and ctx.needs_input_grad[1]:
            g = torch.empty(gr.n_edges + gr.N, dtype=torch.float32, device=dY.device)
            gw, gl = g[:gr.n_edges], g[gr.n_edges:]
            _lib.check(L.sgs_sddmm_csr(_ptr(dZ), _ptr(X), N, D, gr.n_edges, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid),
                                       gw.data_ptr(), gl.data_ptr(), _stream()), "sgs_sddmm_csr")
        if want_db and dbias is None:
            dbias = _colsum(dZ)
        return dX, (_handle_grad(nm, g) if g is not None else None), dbias, None, None, None, None, None


def gcn_propagate(X, nm: Norm, bias=None, act=ACT_NONE, p=0.0, seed=0, site=0):
    """K5: act(A_hat X + bias) with autograd to X, bias and (through nm.handle) the edge weights."""
    _need_gpu(X, bias)
    if X.dtype != torch.float32 or X.dim() != 2 or X.shape[0] != nm.graph.N:
        raise RuntimeError("gcn_propagate: X must be float32 [N, D]")    # nm.what_loop may be None (no self-loop term)
    return _Propagate.apply(X.contiguous(), nm.handle, bias, nm, act, float(p), int(seed), int(site))


# ------------------------------------------------------------------ edge scorer (K1b)
class ActiveSet:
    """Which edges can carry a non-zero upstream gradient into the scorer's backward.
    None = all (dense backward over every scored edge).  The hybrid pipeline sets it to the
    q sampled edges after the draw (every other entry of dL/dp is exactly zero there,
    training_hybrid.py:86), which cuts the scorer's backward from E to q rows."""
    __slots__ = ("eid", "graph", "gq", "ascending")

    def __init__(self):
        self.eid, self.graph, self.gq = None, None, None      # gq: the active rows' upstream gradient, handed over by _SelectSampled
        self.ascending = False

    def set(self, eid: torch.Tensor, graph: Graph, ascending=None):
        """eid: the active edges' ids into the scored edge list, any order, each at most once; graph: the Graph of edge_index[:, eid] in
        that same order (its edge k is active row k).  The fused scorer backward (_score_bwd_fused) additionally needs the rows
        grouped by source -- `eid` ascending on a source-sorted edge list -- and runs only when `ascending` holds; any other order takes
        the unfused mask-form backward, which is correct for every order.  ascending=True: the caller guarantees it (the sampler's
        compaction and the sharded local ids emit edge order); nothing is checked.  None: checked here with one read-back, and taken as
        False inside a stream capture (no host sync there).  False: the caller does not know."""
        if ascending is None:
            if torch.cuda.is_current_stream_capturing() or not eid.is_cuda:
                ascending = False
            else:
                ascending = eid.numel() < 2 or bool((eid[1:] > eid[:-1]).all())
        self.eid, self.graph, self.ascending = eid, graph, bool(ascending)


def _act_bwd_colsum(dY, Y, act, p):
    """(dZ, colsum(dZ)) with dZ = dY * act'(Y): the activation and bias gradients of a layer in one pass."""
    L = _lib.lib()
    N, D = dY.shape
    dZ = torch.empty_like(dY)
    out = torch.empty(D, dtype=torch.float32, device=dY.device)
    ws = workspace(L.sgs_colsum_workspace_bytes(N, D), dY.device)
    _lib.check(L.sgs_act_bwd_colsum(_ptr(dY), _ptr(Y), N, D, act, float(p), _ptr(dZ), _ptr(out), ws.data_ptr(), ws.numel(), _stream()),
               "sgs_act_bwd_colsum")
    return dZ, out


def _colsum(A):
    L = _lib.lib()
    N, D = A.shape
    out = torch.empty(D, dtype=torch.float32, device=A.device)
    ws = workspace(L.sgs_colsum_workspace_bytes(N, D), A.device)
    _lib.check(L.sgs_colsum(_ptr(A), N, D, _ptr(out), ws.data_ptr(), ws.numel(), _stream()), "sgs_colsum")
    return out


def _act_bwd(dY, Y, act, p):
    """dZ = dY * act'(Y) (one sgs_act_bwd launch, also for ACT_NONE)."""
    dZ = torch.empty_like(dY)
    _lib.check(_lib.lib().sgs_act_bwd(_ptr(dY), _ptr(Y), dY.numel(), act, float(p), _ptr(dZ), _stream()), "sgs_act_bwd")
    return dZ


def _grad_through_act(dY, Y, act, p, want_db, colsum_now=True):
    """The prologue of a layer's backward, (dZ, dbias): dZ = dY * act'(Y) -- dY itself without an activation -- and, when `want_db`,
    dbias = colsum(dZ).  With an activation and a bias gradient both come from one pass; without an activation the plain column sum is
    taken here, or, with colsum_now=False, left to the caller (dbias None), who takes it with _colsum after its SpMM / SDDMM.
    `want_db` is the caller's own: the GCN / Chebyshev layers ask has_bias and needs_input_grad, the attention layers has_bias alone."""
    if act != ACT_NONE:
        return _act_bwd_colsum(dY, Y, act, p) if want_db else (_act_bwd(dY, Y, act, p), None)
    return dY, (_colsum(dY) if want_db and colsum_now else None)


def _endpoint_reduce(M_out, M_in, T, graph: Graph, s_out, s_in, H):
    L = _lib.lib()
    out = torch.empty(graph.N, H, dtype=torch.float32, device=M_out.device)
    _lib.check(L.sgs_endpoint_reduce(_ptr(M_out), _ptr(M_in), _ptr(T), graph.N, H, graph.n_edges, _ptr(graph.in_ptr), _ptr(graph.in_src), _ptr(graph.in_eid),
                                     _ptr(graph.out_ptr), _ptr(graph.out_dst), _ptr(graph.out_eid), float(s_out), float(s_in),
                                     _ptr(out), _stream()), "sgs_endpoint_reduce")
    return out


_mask_backward = True        # False: the dense fp32 dv path at every size (tests compare the two)
_fwd_mask = True             # False: the forward keeps no mask; the backward recomputes the hidden layer (sgs_edge_score_bwd_core_bits)
_fused_backward = os.environ.get("SGS_FUSED_BWD", "1") != "0"   # False: feat / dfeat as [n, H] arrays and sgs_endpoint_reduce_pair_bits (the form for edge lists not sorted by source)
_PRODUCTION_ROWS = 65536     # rows (scored edges in the forward, active rows in the backward) from which the production-size kernels are chosen


def src_sorted(edge_index: torch.Tensor) -> bool:
    """Is the edge list sorted by source (PyG's coalesced / row-sorted layout: every loader of the reference emits it)?  Cached on the
    tensor like its Graph; computing it reads one word back, so it is never computed inside a stream capture (unknown = False there:
    the unfused backward is correct for any order).  stepgraph.py stamps its static slot tensors after checking the partitions."""
    c = getattr(edge_index, "_sgs_src_sorted", None)
    if c is not None and c[1] == edge_index._version:
        return c[0]
    if torch.cuda.is_current_stream_capturing():
        return False
    n = edge_index.shape[1]
    ok = True if n < 2 else bool((edge_index[0, 1:] >= edge_index[0, :-1]).all())
    try:
        edge_index._sgs_src_sorted = (ok, edge_index._version)
    except Exception:
        pass
    return ok


# ---- precision of the scorer's matrix-core contractions (include/sgs_hip.h, "bf16 mode").  "fp32" (default): every product fp32-faithful,
# the parity mode.  "bf16": where the fp32-faithful path runs a bf16x6 / mask kernel (E >= 65 536, H in {128, 256}, the variant overrides
# at their defaults, the mask-form backward), the one-product kernels run instead: bf16(a) x bf16(b), fp32 accumulation.  Elsewhere the
# mode has no effect.  The choice is read when a forward is recorded and travels with it to its backward (ctx), never as library state.
PRECISIONS = ("fp32", "bf16")
_precision = "fp32"
# launches per form that ran: forward / backward x fp32 / bf16 (tests prove which path was taken; reset with reset_precision_counts())
PRECISION_COUNTS = {"fwd_fp32": 0, "fwd_bf16": 0, "bwd_fp32": 0, "bwd_bf16": 0}


def reset_precision_counts() -> None:
    for k in PRECISION_COUNTS:
        PRECISION_COUNTS[k] = 0


def check_precision(value) -> str:
    """"fp32" / "bf16" (None: "fp32"); anything else raises ValueError."""
    if value is None:
        return "fp32"
    if not isinstance(value, str) or value not in PRECISIONS:
        raise ValueError(f"scorer precision must be one of {PRECISIONS}, got {value!r}")
    return value


def get_scorer_precision() -> str:
    return _precision


class scorer_precision:
    """Context manager: the ambient precision of ops.edge_score inside the block (sgs_gnn_amd.scorer_precision("bf16"))."""

    def __init__(self, value):
        self.value = check_precision(value)

    def __enter__(self):
        global _precision
        self.prev, _precision = _precision, self.value
        return self

    def __exit__(self, *exc):
        global _precision
        _precision = self.prev
        return False


class _FwdPlan(NamedTuple):
    form: str              # "mask": keeps the ReLU x dropout bit of every hidden unit for the backward / "paired" / "plain"
    bf16: bool             # the one-product kernels (the entry point's "_bf16" twin)
    ask_sorted: bool       # the fused backward may follow if the edge list is sorted by source: worth asking src_sorted() (after the launch)


class _BwdPlan(NamedTuple):
    form: str              # "dense" / "recompute" (mask form, hidden layer recomputed) / "kept" (mask form on the forward's bits) / "fused"
    bf16: bool
    core: bool = True      # the dense form's own choices: run the core at all (no active row: nothing to launch),
    row_gemm: bool = False       # dfeat as the bf16x6 row GEMM (else F.linear),
    fused_colsum: bool = False   # d b1 as a by-product of the d W1a GEMM (else a column sum of its own),
    pair_reduce: bool = False    # both endpoint reductions in one pass (H % 4 == 0)


_FWD_ENTRY = {"mask": "sgs_edge_score_fwd_mask", "paired": "sgs_edge_score_fwd_paired", "plain": "sgs_edge_score_fwd"}


def _plan_forward(L, E, H, precision, want_dcodes, has_pairs) -> _FwdPlan:
    """Every choice of one scorer forward, from sizes, switches and the library's host answers alone (no tensor is touched).  The
    library's variant overrides (sgs_edge_score_set_variant / _set_bwd_variant) win over the bf16 mode and over the mask-keeping forward,
    which is always the bf16x6 loop: only at their defaults may either stand in for the kernels a test or the bench asked for by name."""
    big = E >= _PRODUCTION_ROWS
    default = big and L.sgs_edge_score_get_variant() < 0 and L.sgs_edge_score_get_bwd_variant() < 0
    bf16 = bool(default and precision == "bf16" and L.sgs_edge_score_bf16_supported(H))
    if default and _fwd_mask and _mask_backward and want_dcodes and L.sgs_edge_score_bwd_bits_supported(H):
        return _FwdPlan("mask", bf16, bool(_fused_backward))       # a forward whose backward will follow
    if has_pairs and big and L.sgs_edge_score_paired_supported(H):
        return _FwdPlan("paired", bf16, False)       # undirected graph stored both ways: the canonical half runs the contraction, every mate rides along
    return _FwdPlan("plain", bf16, False)


def _plan_backward(L, n, H, kept, bf16, src_sorted, want_dcodes, ascending) -> _BwdPlan:
    """Every choice of one scorer backward over n active rows.  kept / bf16 / src_sorted: what the forward recorded (_ScoreSaved);
    ascending: ActiveSet.ascending, None when every edge is active (in edge order).  The one-product contractions need the mask the forward
    kept (a recompute would be the fp32 function's), and a kept mask goes unused when the active set turns out too small for the mask-form
    kernels: the dense form recomputes.  The fused form needs the active rows grouped by source: a source-sorted edge list read in
    ascending edge order."""
    big = n >= _PRODUCTION_ROWS
    if _mask_backward and big and L.sgs_edge_score_bwd_bits_supported(H) and L.sgs_gemm_tn_mask_supported(n, H, H) and want_dcodes:
        if not kept:
            return _BwdPlan("recompute", False)
        return _BwdPlan("fused" if src_sorted and _fused_backward and ascending is not False else "kept", bool(bf16))
    return _BwdPlan("dense", False, n > 0, bool(big and L.sgs_edge_score_bwd_dfeat_supported(H)), bool(L.sgs_gemm_tn_can_colsum(n, H, H)), H % 4 == 0)


def _call(L, name, bf16, *args):
    """Run entry point `name`, or its one-product twin `name`_bf16, and check the answer under the name that ran."""
    name = name + "_bf16" if bf16 else name
    _lib.check(getattr(L, name)(*args), name)


class _ScoreSaved(NamedTuple):
    """What the scorer's backward reads (_edge_score_backward): _EdgeScore.backward builds it from its ctx, torch_ops.edge_score_backward
    from its arguments."""
    codes: torch.Tensor
    U: torch.Tensor                   # codes W1b^T
    W1: torch.Tensor
    b1: torch.Tensor
    w2: torch.Tensor
    b2: torch.Tensor
    edge_index: torch.Tensor
    kept: Optional[tuple]             # (maskbits, scores) of a mask-keeping forward, else None
    active: Optional[ActiveSet]
    p: float
    seed: int
    site: int
    offset: int
    bf16: bool = False                # the forward ran the one-product kernels
    src_sorted: bool = False          # a mask-keeping forward found its edge list sorted by source (_FwdPlan.ask_sorted)
    want_dcodes: bool = True          # codes wants a gradient


class _EdgeScore(torch.autograd.Function):
    """K1b with the node-level half of fc1 inside: U = codes W1b^T (library GEMM) in forward; in backward d codes gets dU W1b on
    top of the direct term, and BOTH halves of d fc1.weight [H, 2H] are written in place by the two weight-gradient GEMMs
    (d W1a = dv^T feat, d W1b = dU^T codes; sgs_gemm_tn_ld with ldc = 2H) -- no slice views, zero fills or gradient adds."""

    @staticmethod
    def forward(ctx, codes, W1, b1, w2, b2, edge_index, active, p, seed, site, edge_id_offset, pairs, precision="fp32"):
        L = _lib.lib()
        N, H = codes.shape
        E = edge_index.shape[1]
        U = torch.mm(codes, W1[:, H:].t())
        out = torch.empty(E, dtype=torch.float32, device=codes.device)
        ws = workspace(L.sgs_edge_score_workspace_bytes(N, H, E), codes.device)
        plan = _plan_forward(L, E, H, precision, ctx.needs_input_grad[0], pairs is not None)
        maskbits = torch.empty(E, H // 32, dtype=torch.int32, device=codes.device) if plan.form == "mask" else None
        canon, mate = pairs if pairs is not None else (None, None)
        # the three forms take the same arguments but for the pairs (mask, paired) and the mask to keep (mask)
        pair_args = () if plan.form == "plain" else (_ptr(canon, torch.int32), 0 if canon is None else canon.numel(), _ptr(mate, torch.int32))
        _call(L, _FWD_ENTRY[plan.form], plan.bf16, _ptr(codes, torch.float32), _ptr(U, torch.float32), N, H, _ptr(edge_index, torch.int64), E,
              edge_id_offset, *pair_args, _ptr(W1, torch.float32), _ptr(b1), _ptr(w2), _ptr(b2), float(p), seed, site, _ptr(out),
              *(() if maskbits is None else (_ptr(maskbits),)), ws.data_ptr(), ws.numel(), _stream())
        PRECISION_COUNTS["fwd_bf16" if plan.bf16 else "fwd_fp32"] += 1
        ctx.save_for_backward(codes, U, W1, b1, w2, b2, edge_index, *((maskbits, out) if maskbits is not None else ()))
        # (src_sorted may read a word back the first time it sees an edge list: asked only where the plan needs it, and after the launch)
        ctx.active, ctx.cfg = active, (float(p), seed, site, edge_id_offset, plan.bf16, plan.ask_sorted and src_sorted(edge_index))
        return out

    @staticmethod
    def backward(ctx, gp):
        t = ctx.saved_tensors
        saved = _ScoreSaved(*t[:7], t[7:] or None, ctx.active, *ctx.cfg, ctx.needs_input_grad[0])
        return _edge_score_backward(saved, gp, leaf=(ctx, 1)) + (None,) * 8


def _active_rows(act, gp, edge_index, N):
    """The rows a scorer backward runs over, (eid, graph, n, gp_act): the ActiveSet's, with their upstream gradient -- act.gq as it is when
    _SelectSampled handed it over and `gp` is its stride-0 zero (nothing to gather), else gp[eid] (+ act.gq) -- or every edge (eid None).
    act.gq is taken: it is None afterwards."""
    if act is None or act.eid is None:
        return None, get_graph(edge_index, N), edge_index.shape[1], gp.contiguous()
    eid, tok = act.eid, _zero_token(gp.device)
    if act.gq is not None and gp.numel() == edge_index.shape[1] and gp.stride(0) == 0 and gp.data_ptr() == tok.data_ptr():
        gp_act = act.gq
    else:
        gp_act = gp.index_select(0, eid)
        if act.gq is not None:              # another consumer of the scores contributed a dense gradient as well
            gp_act = gp_act + act.gq
    act.gq = None
    return eid, act.graph, eid.numel(), gp_act


def _edge_score_backward(s: _ScoreSaved, gp, leaf=None):
    """-> (d codes, d fc1.weight, d fc1.bias, d fc2.weight, d fc2.bias).  `leaf`: _leaf_dw's handle on fc1.weight in the running
    backward node, None outside one."""
    L = _lib.lib()
    N, H = s.codes.shape
    eid, graph, n, gp_act = _active_rows(s.active, gp, s.edge_index, N)
    plan = _plan_backward(L, n, H, s.kept is not None, s.bf16, s.src_sorted, s.want_dcodes, None if eid is None else s.active.ascending)
    PRECISION_COUNTS["bwd_bf16" if plan.bf16 else "bwd_fp32"] += 1
    dcodes, dU, dW1, db1, dw2, db2 = _SCORE_BWD[plan.form](L, s, plan, eid, graph, n, gp_act)
    # the node-level half: U = codes W1b^T  ->  d codes += dU W1b (library GEMM, accumulating),  d W1b = dU^T codes (right half of
    # d fc1.weight, in place)
    if s.want_dcodes:
        dcodes.addmm_(dU, s.W1[:, H:])                             # in place (beta = 1): no copy of dcodes
    _leaf_dw(dU, s.codes, N, H, H, leaf=leaf, out=dW1, col0=H)
    return dcodes, dW1, db1, dw2, db2


def _score_bwd_dense(L, s, plan, eid, graph, n, gp_act):
    """dv as an fp32 [n, H] matrix, the hidden layer recomputed: every size and hidden width.  (With no row at all only the core is
    skipped; the other launches accept n = 0 and write the zeros -- _EdgeScoreEPD returns early instead, both on purpose.  d w2 / d b2 are
    this form's own column sums of hdz / dz: the mask forms get them from their consumers.)"""
    N, H = s.codes.shape
    dev = s.codes.device
    dv, feat = _empty_f32(n, H, device=dev), _empty_f32(n, H, device=dev)
    tile = L.sgs_edge_score_bwd_tile()
    hdz = _empty_f32((n + tile - 1) // tile, H, device=dev)          # per-tile column sums of dz * hidden (rows sum to d w2)
    dz = _empty_f32(n, device=dev)
    if plan.core:
        ws = workspace(L.sgs_edge_score_workspace_bytes(N, H, 0), dev)
        _lib.check(L.sgs_edge_score_bwd_core(_ptr(s.codes), _ptr(s.U), N, H, _ptr(s.edge_index), s.edge_index.shape[1], s.offset, _ptr(eid), n,
                                             _ptr(gp_act), _ptr(s.W1), _ptr(s.b1), _ptr(s.w2), _ptr(s.b2), s.p, s.seed, s.site, _ptr(dv),
                                             _ptr(hdz), _ptr(dz), _ptr(feat), ws.data_ptr(), ws.numel(), _stream()), "sgs_edge_score_bwd_core")
    if plan.row_gemm:
        # dfeat = dv W1a on the forward's bf16x6 loop as a row GEMM (fp32-faithful): ~75 us at 100 k rows against 122 us below
        dfeat = _empty_f32(n, H, device=dev)
        wsd = workspace(L.sgs_edge_score_workspace_bytes(0, H, 0), dev)
        _lib.check(L.sgs_edge_score_bwd_dfeat(_ptr(dv), n, H, _ptr(s.W1), _ptr(dfeat), wsd.data_ptr(), wsd.numel(), _stream()),
                   "sgs_edge_score_bwd_dfeat")
    else:
        # as F.linear with a contiguous W1a^T: the vendor GEMM runs that form at 110 TFLOP/s (85 with the strided view)
        dfeat = torch.nn.functional.linear(dv, s.W1[:, :H].t().contiguous())          # [n,H]
    # d fc1.weight [H, 2H], both halves written in place.  Left: dW1a = dv^T feat (K = n rows): sgs_gemm_tn's tall-K kernel (the
    # vendor GEMM picks a 42 TFLOP/s kernel for this shape), with d b1 = colsum(dv) as a by-product of the same pass over dv
    dW1 = torch.empty_like(s.W1)
    wsg = workspace(L.sgs_gemm_tn_workspace_bytes(n, H, H), dev)
    db1 = _empty_f32(H, device=dev) if plan.fused_colsum else None
    _lib.check(L.sgs_gemm_tn_ld(_ptr(dv), _ptr(feat), n, H, H, _ptr(dW1), 2 * H, _ptr(db1), wsg.data_ptr(), wsg.numel(), _stream()),
               "sgs_gemm_tn_ld")
    if db1 is None:
        db1 = _colsum(dv)
    dw2 = _colsum(hdz)
    db2 = _colsum(dz.view(n, 1)).reshape(1)
    if plan.pair_reduce:                                   # both endpoint reductions in one pass over the incident-edge lists
        dcodes, dU = _empty_f32(N, H, device=dev), _empty_f32(N, H, device=dev)
        _lib.check(L.sgs_endpoint_reduce_pair(_ptr(dfeat), _ptr(dv), _ptr(s.codes), N, H, graph.n_edges, _ptr(graph.in_ptr), _ptr(graph.in_src),
                                              _ptr(graph.in_eid), _ptr(graph.out_ptr), _ptr(graph.out_dst), _ptr(graph.out_eid),
                                              _ptr(dcodes), _ptr(dU), _stream()), "sgs_endpoint_reduce_pair")
    else:
        dcodes = _endpoint_reduce(dfeat, dfeat, s.codes, graph, 1.0, 1.0, H)
        dU = _endpoint_reduce(dv, dv, None, graph, 1.0, -1.0, H)
    return dcodes, dU, dW1, db1, dw2, db2


def _dropout_scale(p):
    """1 / (1 - p) as the kernels form it: 1.0f / (1.0f - p)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _dw2_parts(N, H, dev):
    """(Traw, craw, Rraw): what the weight-gradient GEMM and the endpoint reduction leave for sgs_edge_score_dw2_from_parts."""
    return _empty_f32(H, H, device=dev), _empty_f32(H, device=dev), _empty_f32(N, H, device=dev)


def _dw2_from_parts(L, s, Traw, craw, Rraw):
    N, H = s.codes.shape
    dw2 = _empty_f32(H, device=s.codes.device)
    _lib.check(L.sgs_edge_score_dw2_from_parts(_ptr(s.W1), _ptr(Traw), _ptr(s.U), _ptr(Rraw), _ptr(s.b1), _ptr(craw), N, H, s.p, _ptr(dw2), _stream()),
               "sgs_edge_score_dw2_from_parts")
    return dw2


def _score_bwd_mask(L, s, plan, eid, graph, n, gp_act):
    """The backward at production size in its MASK form (include/sgs_hip.h, sgs_edge_score_bwd_core_bits): dv = dz x [hidden > 0] x w2 / (1 - p)
    never exists as an fp32 [n, H] matrix -- the core writes one bit per entry and the three consumers rebuild what they need, the two
    contractions with a 0 / 1 operand at half the MFMA work.  "kept": the forward kept the mask and p, so nothing is recomputed -- dz, the
    active rows' mask and feat in one pass, d fc2.weight from the consumers' parts; "recompute": the core forms them, and d fc2.weight's
    per-tile sums."""
    N, H = s.codes.shape
    E = s.edge_index.shape[1]
    dev = s.codes.device
    bits = torch.empty(n, H // 32, dtype=torch.int32, device=dev)
    dz, feat = _empty_f32(n, device=dev), _empty_f32(n, H, device=dev)
    hdz = Traw = craw = Rraw = None
    if plan.form == "kept":
        maskbits, p_out = s.kept
        _lib.check(L.sgs_edge_score_bwd_prep(_ptr(s.codes), N, H, _ptr(s.edge_index), E, _ptr(eid), n, _ptr(gp_act), _ptr(p_out), _ptr(maskbits),
                                             _ptr(dz), _ptr(bits), _ptr(feat), _stream()), "sgs_edge_score_bwd_prep")
        Traw, craw, Rraw = _dw2_parts(N, H, dev)
    else:
        tile = L.sgs_edge_score_bwd_tile()
        hdz = _empty_f32((n + tile - 1) // tile, H, device=dev)
        ws = workspace(L.sgs_edge_score_workspace_bytes(N, H, 0), dev)
        _lib.check(L.sgs_edge_score_bwd_core_bits(_ptr(s.codes), _ptr(s.U), N, H, _ptr(s.edge_index), E, s.offset, _ptr(eid), n, _ptr(gp_act),
                                                  _ptr(s.W1), _ptr(s.b1), _ptr(s.w2), _ptr(s.b2), s.p, s.seed, s.site, _ptr(bits), _ptr(hdz), _ptr(dz),
                                                  _ptr(feat), ws.data_ptr(), ws.numel(), _stream()), "sgs_edge_score_bwd_core_bits")
    dfeat = _empty_f32(n, H, device=dev)
    wsd = workspace(L.sgs_edge_score_workspace_bytes(0, H, 0), dev)
    _call(L, "sgs_edge_score_bwd_dfeat_bits", plan.bf16, _ptr(bits), _ptr(dz), n, H, _ptr(s.W1), _ptr(s.w2), s.p, _ptr(dfeat), wsd.data_ptr(),
          wsd.numel(), _stream())
    dW1 = torch.empty_like(s.W1)
    db1, db2 = _empty_f32(H, device=dev), _empty_f32(1, device=dev)
    wsg = workspace(L.sgs_gemm_tn_workspace_bytes(n, H, H), dev)
    _call(L, "sgs_gemm_tn_mask", plan.bf16, _ptr(bits), _ptr(dz), _ptr(s.w2), _dropout_scale(s.p), _ptr(feat), n, H, H, _ptr(dW1), 2 * H, _ptr(db1),
          _ptr(db2), _ptr(Traw), _ptr(craw), wsg.data_ptr(), wsg.numel(), _stream())
    dw2 = _colsum(hdz) if hdz is not None else None
    dcodes, dU = _empty_f32(N, H, device=dev), _empty_f32(N, H, device=dev)
    _lib.check(L.sgs_endpoint_reduce_pair_bits(_ptr(dfeat), _ptr(bits), _ptr(dz), _ptr(s.w2), s.p, _ptr(s.codes), N, H, graph.n_edges, _ptr(graph.in_ptr),
                                               _ptr(graph.in_src), _ptr(graph.in_eid), _ptr(graph.out_ptr), _ptr(graph.out_dst),
                                               _ptr(graph.out_eid), _ptr(dcodes), _ptr(dU), _ptr(Rraw), _stream()), "sgs_endpoint_reduce_pair_bits")
    return dcodes, dU, dW1, db1, (dw2 if dw2 is not None else _dw2_from_parts(L, s, Traw, craw, Rraw)), db2


def _score_bwd_fused(L, s, plan, eid, graph, n, gp_act):
    """The no-recompute backward with neither feat nor dfeat as [n, H] arrays (include/sgs_hip.h, "FUSED form"): the active rows are sorted
    by source, so the by-source half of d codes is reduced inside the dfeat contraction's epilogue, and the weight-gradient GEMM gathers
    x_s * x_d itself.  Six launches: prep (dz, mask rows, endpoints; it also packs dfeat's W1a operand), dfeat + by-source sums, d W1a and
    its slab reduction, the endpoint reductions, d fc2.weight."""
    N, H = s.codes.shape
    dev = s.codes.device
    maskbits, p_out = s.kept
    bits = torch.empty(n, H // 32, dtype=torch.int32, device=dev)
    dz = _empty_f32(n, device=dev)
    sd = torch.empty(n, 2, dtype=torch.int32, device=dev)
    wsd = workspace(L.sgs_edge_score_workspace_bytes(0, H, 0), dev)
    _call(L, "sgs_edge_score_bwd_prep_sd_pack", plan.bf16, _ptr(s.codes), N, H, _ptr(s.edge_index), s.edge_index.shape[1], _ptr(eid), n, _ptr(gp_act),
          _ptr(p_out), _ptr(maskbits), _ptr(dz), _ptr(bits), _ptr(sd), _ptr(s.W1), _ptr(s.w2), s.p, wsd.data_ptr(), wsd.numel(), _stream())
    G = _empty_f32(n, H, device=dev)
    opart = _empty_f32(L.sgs_edge_score_bwd_fused_opart_rows(n, N), H, device=dev)
    _call(L, "sgs_edge_score_bwd_dfeat_fused_packed", plan.bf16, _ptr(bits), _ptr(dz), _ptr(sd), _ptr(s.codes), n, N, H, _ptr(G), _ptr(opart),
          wsd.data_ptr(), wsd.numel(), _stream())
    dW1 = torch.empty_like(s.W1)
    db1, db2 = _empty_f32(H, device=dev), _empty_f32(1, device=dev)
    Traw, craw, Rraw = _dw2_parts(N, H, dev)
    wsg = workspace(L.sgs_gemm_tn_workspace_bytes(n, H, H), dev)
    _call(L, "sgs_gemm_tn_mask_gather", plan.bf16, _ptr(bits), _ptr(dz), _ptr(s.w2), _dropout_scale(s.p), _ptr(s.codes), N, _ptr(sd), n, H, H, _ptr(dW1),
          2 * H, _ptr(db1), _ptr(db2), _ptr(Traw), _ptr(craw), wsg.data_ptr(), wsg.numel(), _stream())
    dcodes, dU = _empty_f32(N, H, device=dev), _empty_f32(N, H, device=dev)
    _lib.check(L.sgs_edge_score_bwd_reduce_fused(_ptr(G), _ptr(opart), _ptr(bits), _ptr(dz), _ptr(s.w2), s.p, N, H, graph.n_edges, _ptr(graph.in_ptr),
                                                 _ptr(graph.in_eid), _ptr(graph.out_ptr), _ptr(dcodes), _ptr(dU), _ptr(Rraw), _stream()),
               "sgs_edge_score_bwd_reduce_fused")
    return dcodes, dU, dW1, db1, _dw2_from_parts(L, s, Traw, craw, Rraw), db2


_SCORE_BWD = {"dense": _score_bwd_dense, "recompute": _score_bwd_mask, "kept": _score_bwd_mask, "fused": _score_bwd_fused}


def edge_score(codes, fc1_w, fc1_b, fc2_w, fc2_b, edge_index, active=None, p=0.0, seed=0, site=0, edge_id_offset=0, pairs="cached",
               precision=None):
    """K1b.  codes [N,H]; fc1_w [H,2H]; fc1_b [H]; fc2_w [1,H]; fc2_b [1]; edge_index [2,E] -> p [E].
    `pairs`: (canon, mate) of get_pairs for the paired forward, None for the plain one, "cached" (default) = whatever
    get_pairs(edge_index) holds (nothing is built here).  `precision`: None = the ambient setting (scorer_precision), else "fp32" / "bf16"."""
    precision = _precision if precision is None else check_precision(precision)
    _need_gpu(codes, fc1_w, edge_index)
    if isinstance(pairs, str):
        pairs = get_pairs(edge_index, codes.shape[0])
    return _EdgeScore.apply(codes.contiguous(), fc1_w.contiguous(), fc1_b.contiguous(), fc2_w.reshape(-1).contiguous(), fc2_b.contiguous(),
                            edge_index.contiguous(), active, float(p), int(seed), int(site), int(edge_id_offset), pairs, precision)


class _EdgeScoreEPD(torch.autograd.Function):
    """EdgeProbMLP with dropout > 0 (model.py:16-45): `_edge_score(drop(A[src]), drop(A[dst]))` with the two endpoint masks drawn per (edge,
    endpoint), straight from the node table A = relu(fcdim(X)) [N, H] and the scored edge list -- no [E', H] gathers, masks or
    concatenations on the way (include/sgs_hip.h, "Endpoint-dropout scorer").  The backward runs over the active rows only (the trainer's
    ActiveSet: the q sampled edges in the hybrid pipeline) and materialises the features of THOSE rows alone."""

    @staticmethod
    def forward(ctx, A, W1, b1, w2, b2, edge_index, active, p, seed, site, p_ep, seed_x, site_x, seed_y, site_y, edge_id_offset):
        L = _lib.lib()
        N, H = A.shape
        E = edge_index.shape[1]
        out = torch.empty(E, dtype=torch.float32, device=A.device)
        ws = workspace(L.sgs_edge_score_epd_workspace_bytes(H), A.device)
        _lib.check(L.sgs_edge_score_epd_fwd(_ptr(A, torch.float32), N, H, _ptr(edge_index, torch.int64), E, edge_id_offset, _ptr(W1, torch.float32),
                                            _ptr(b1), _ptr(w2), _ptr(b2), float(p), seed, site, float(p_ep), seed_x, site_x, seed_y, site_y, _ptr(out),
                                            ws.data_ptr(), ws.numel(), _stream()), "sgs_edge_score_epd_fwd")
        ctx.save_for_backward(A, W1, b1, w2, b2, edge_index)
        ctx.active, ctx.cfg = active, (float(p), seed, site, float(p_ep), seed_x, site_x, seed_y, site_y, edge_id_offset)
        return out

    @staticmethod
    def backward(ctx, gp):
        L = _lib.lib()
        A, W1, b1, w2, b2, edge_index = ctx.saved_tensors
        p, seed, site, p_ep, seed_x, site_x, seed_y, site_y, offset = ctx.cfg
        N, H = A.shape
        E = edge_index.shape[1]
        dev = A.device
        eid, graph, n, gp_act = _active_rows(ctx.active, gp, edge_index, N)
        f32 = dict(dtype=torch.float32, device=dev)
        dv, feat2, dz = torch.empty(n, H, **f32), torch.empty(n, 2 * H, **f32), torch.empty(n, **f32)
        tile = L.sgs_edge_score_bwd_tile()
        hdz = torch.empty((n + tile - 1) // tile, H, **f32)
        dA = torch.zeros(N, H, **f32) if n == 0 else torch.empty(N, H, **f32)
        dW1 = torch.zeros_like(W1) if n == 0 else torch.empty_like(W1)
        if n == 0:          # (no active row: zeros, nothing launched -- _score_bwd_dense skips only its core; both on purpose)
            return dA, dW1, torch.zeros(H, **f32), torch.zeros(H, **f32), torch.zeros(1, **f32), *([None] * 11)
        ws = workspace(L.sgs_edge_score_epd_workspace_bytes(H), dev)
        _lib.check(L.sgs_edge_score_epd_bwd_core(_ptr(A), N, H, _ptr(edge_index), E, offset, _ptr(eid), n, _ptr(gp_act), _ptr(W1), _ptr(b1), _ptr(w2),
                                                 _ptr(b2), p, seed, site, p_ep, seed_x, site_x, seed_y, site_y, _ptr(dv), _ptr(hdz), _ptr(dz), _ptr(feat2),
                                                 ws.data_ptr(), ws.numel(), _stream()), "sgs_edge_score_epd_bwd_core")
        wsg = workspace(L.sgs_gemm_tn_workspace_bytes(n, H, 2 * H), dev)
        _lib.check(L.sgs_gemm_tn(_ptr(dv), _ptr(feat2), n, H, 2 * H, _ptr(dW1), wsg.data_ptr(), wsg.numel(), _stream()), "sgs_gemm_tn")
        db1, dw2 = _colsum(dv), _colsum(hdz)
        db2 = _colsum(dz.view(n, 1)).reshape(1)
        dfeat2 = torch.mm(dv, W1)                               # [n, 2H] = [d (x_m * y_m) | d (x_m - y_m)]  (library GEMM)
        _lib.check(L.sgs_edge_score_epd_reduce(_ptr(dfeat2), _ptr(A), N, H, _ptr(graph.in_ptr), _ptr(graph.in_src), _ptr(graph.in_eid), _ptr(graph.out_ptr),
                                               _ptr(graph.out_dst), _ptr(graph.out_eid), _ptr(eid), offset, p_ep, seed_x, site_x, seed_y, site_y, _ptr(dA),
                                               _stream()), "sgs_edge_score_epd_reduce")
        return dA, dW1, db1, dw2, db2, *([None] * 11)


def edge_score_epd(A, fc1_w, fc1_b, fc2_w, fc2_b, edge_index, active=None, p=0.0, seed=0, site=0, p_ep=0.0, seed_x=0, site_x=0, seed_y=0,
                   site_y=0, edge_id_offset=0):
    """The scorer of EdgeProbMLP when its endpoint dropout is on (see _EdgeScoreEPD): A [N,H] = relu(fcdim(X)); -> p [E]."""
    _need_gpu(A, fc1_w, edge_index)
    return _EdgeScoreEPD.apply(A.contiguous(), fc1_w.contiguous(), fc1_b.contiguous(), fc2_w.reshape(-1).contiguous(), fc2_b.contiguous(),
                               edge_index.contiguous(), active, float(p), int(seed), int(site), float(p_ep), int(seed_x), int(site_x), int(seed_y),
                               int(site_y), int(edge_id_offset))


# ------------------------------------------------------------------ gate + losses (K6)
def _u8(mask: torch.Tensor) -> torch.Tensor:
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    raise RuntimeError("mask must be a bool tensor")


def masked_correct(logits, y, train_mask, out=None) -> torch.Tensor:
    """int32 [2] on device: (#correct argmax on train rows, #train rows) -- no host sync."""
    L = _lib.lib()
    _need_gpu(logits, y, train_mask)
    if out is None:
        out = torch.empty(2, dtype=torch.int32, device=logits.device)
    N, C = logits.shape
    _lib.check(L.sgs_masked_correct(_ptr(logits.contiguous(), torch.float32), N, C, _ptr(y, torch.int64), _ptr(_u8(train_mask)),
                                    _ptr(out), _stream()), "sgs_masked_correct")
    return out


def confusion_counts(logits, y, masks, out=None) -> torch.Tensor:
    """int64 [3, C, C] on device: out[s][t][p] += #{rows i in masks[s] with y_i == t and argmax logits[i] == p} (sgs_confusion_counts; the
    argmax is masked_correct's).  `out` is accumulated into when given, else a zeroed buffer is made.  Labels of masked rows lie in
    [0, C); rows outside every mask may hold any label.  No host sync."""
    L = _lib.lib()
    _need_gpu(logits, y, *masks)
    N, C = logits.shape
    if len(masks) != 3:
        raise RuntimeError("confusion_counts: need three masks (train, val, test)")
    if out is None:
        out = torch.zeros(3, C, C, dtype=torch.int64, device=logits.device)
    elif out.shape != (3, C, C) or not out.is_contiguous():
        raise RuntimeError(f"confusion_counts: out must be a contiguous int64 [3, {C}, {C}] tensor")
    lg, m = logits.contiguous(), [_u8(x) for x in masks]
    if any(x.numel() != N for x in m) or y.numel() != N:
        raise RuntimeError("confusion_counts: y and the masks need one entry per row of logits")
    _lib.check(L.sgs_confusion_counts(_ptr(lg, torch.float32), N, C, _ptr(y, torch.int64), _ptr(m[0]), _ptr(m[1]), _ptr(m[2]),
                                      _ptr(out, torch.int64), _stream()), "sgs_confusion_counts")
    return out


def confusion_variant(N: int, C: int) -> int:
    """sgs_confusion_variant: the form a confusion_counts call on [N, C] logits launches now: 1 direct, 2 privatised, 0 nothing (N = 0), -1 when
    the call would be refused.  Host-only."""
    return int(_lib.lib().sgs_confusion_variant(int(N), int(C)))


def confusion_variant_set(code: int) -> None:
    """sgs_confusion_variant_set: 0 = automatic (default), 1 = direct, 2 = privatised; any other code raises."""
    _lib.check(_lib.lib().sgs_confusion_variant_set(int(code)), "sgs_confusion_variant_set")


def auc_scores(logits) -> torch.Tensor:
    """The fp32 score matrix [N, S] whose ranking ROC-AUC is taken of (include/sgs_hip.h): C = 2 -> S = 1, logits[:, 1] - logits[:, 0];
    C > 2 -> S = C, log_softmax over the classes (one-vs-rest).  Plain torch ops on the device, outside any kernel, so that the key bits
    can be restated on the host from the same values.  C = 1 raises ValueError."""
    _need_gpu(logits)
    if logits.dim() != 2 or logits.shape[1] < 2:
        raise ValueError(f"auc_scores: need [N, C] logits with C >= 2 (ROC-AUC of one class is undefined), got {tuple(logits.shape)}")
    lg = logits.float()
    if lg.shape[1] == 2:
        return (lg[:, 1] - lg[:, 0]).unsqueeze(1).contiguous()
    return torch.log_softmax(lg, 1).contiguous()


def auc_block_items() -> int:
    """sgs_auc_block_items: the sorted items one workgroup of auc_counts' rank-sum pass owns.  Host-only."""
    return int(_lib.lib().sgs_auc_block_items())


def auc_pack(scores, y, masks, C: int, out=None) -> torch.Tensor:
    """int64 [N * S] on device: one sort key per (row, column) item of `scores` [N, S] (sgs_auc_pack: masks in bits 0-2, positive in bit 3,
    the order-preserving image of the score in bits 4-35, the column above).  C = 2 needs S = 1, C > 2 needs S = C.  One launch, no host
    sync."""
    L = _lib.lib()
    _need_gpu(scores, y, *masks)
    if len(masks) != 3:
        raise RuntimeError("auc_pack: need three masks (train, val, test)")
    if scores.dim() != 2:
        raise RuntimeError("auc_pack: scores must be [N, S]")
    N, S = scores.shape
    sc, m = scores.contiguous(), [_u8(x) for x in masks]
    if any(x.numel() != N for x in m) or y.numel() != N:
        raise RuntimeError("auc_pack: y and the masks need one entry per row of scores")
    if out is None:
        out = torch.empty(N * S, dtype=torch.int64, device=scores.device)
    elif out.numel() != N * S:
        raise RuntimeError(f"auc_pack: out must hold {N * S} int64 keys")
    _lib.check(L.sgs_auc_pack(_ptr(sc, torch.float32), N, S, int(C), _ptr(y, torch.int64), _ptr(m[0]), _ptr(m[1]), _ptr(m[2]),
                              _ptr(out, torch.int64), _stream()), "sgs_auc_pack")
    return out


def auc_counts(keys, S: int) -> torch.Tensor:
    """int64 [3, S, 3] on device: {twoU, P, Nn} per (split, column) of any concatenation of auc_pack blocks (sgs_auc_counts: one device
    radix sort, then the tie-aware rank-sum pass; exact integers, the same bits on every call).  No host sync; not capturable."""
    L = _lib.lib()
    _need_gpu(keys)
    n, S = keys.numel(), int(S)
    out = torch.empty(3, S, 3, dtype=torch.int64, device=keys.device)
    nbytes = int(L.sgs_auc_counts_workspace_bytes(n, S))
    ws = workspace(nbytes, keys.device)
    _lib.check(L.sgs_auc_counts(_ptr(keys, torch.int64), n, S, _ptr(out), _ptr(ws), nbytes, _stream()), "sgs_auc_counts")
    return out


def masked_correct_pair(logits_a, logits_b, y, train_mask, out) -> torch.Tensor:
    """The gate's two counts in one launch: out[0:4] = (#correct_a, #train, #correct_b, #train); `out` (int32, >= 4 entries)
    must be zero on entry."""
    L = _lib.lib()
    _need_gpu(logits_a, logits_b, y, train_mask, out)
    N, C = logits_a.shape
    if logits_b.shape != logits_a.shape:
        raise RuntimeError("masked_correct_pair: logits shapes differ")
    _lib.check(L.sgs_masked_correct_pair(_ptr(logits_a.contiguous(), torch.float32), _ptr(logits_b.contiguous(), torch.float32), N, C,
                                         _ptr(y, torch.int64), _ptr(_u8(train_mask)), _ptr(out, torch.int32), _stream()),
               "sgs_masked_correct_pair")
    return out


def gate_counts(logits_a, logits_b, y, train_mask, publish=None) -> torch.Tensor:
    """The gate's counts: int32[5] on the device = (#correct_a, #train, #correct_b, #train, 0), two launches, no zero fill.
    `publish` = (seq, dst_pinned): the finishing launch also hands the four counts to the host (as publish_to_host)."""
    L = _lib.lib()
    _need_gpu(logits_a, logits_b, y, train_mask)
    N, C = logits_a.shape
    if logits_b.shape != logits_a.shape:
        raise RuntimeError("gate_counts: logits shapes differ")
    out = torch.empty(5, dtype=torch.int32, device=logits_a.device)
    seq_p = dst_p = None
    if publish is not None:
        seq, dst = publish
        if dst.is_cuda or not dst.is_pinned() or dst.dtype != torch.int32 or dst.numel() < 5:
            raise RuntimeError("gate_counts: the publish destination must be a pinned host int32 tensor with 5 entries")
        seq_p, dst_p = (None if seq is None else seq.data_ptr()), dst.data_ptr()
    ws = workspace(L.sgs_gate_counts_workspace_bytes(N), logits_a.device)
    _lib.check(L.sgs_gate_counts(_ptr(logits_a.contiguous(), torch.float32), _ptr(logits_b.contiguous(), torch.float32), N, C, _ptr(y, torch.int64),
                                 _ptr(_u8(train_mask)), _ptr(out, torch.int32), seq_p, dst_p, ws.data_ptr(), ws.numel(), _stream()),
               "sgs_gate_counts")
    return out


def loss_tick(loss_sum, loss, epoch) -> None:
    """sgs_loss_tick: loss_sum += loss and epoch += 1 in one launch (the last kernel of a replayed step)."""
    L = _lib.lib()
    _need_gpu(loss_sum, loss, epoch)
    _lib.check(L.sgs_loss_tick(_ptr(loss_sum, torch.float32), _ptr(loss.detach().reshape(1), torch.float32), epoch.data_ptr(), _stream()),
               "sgs_loss_tick")


def publish_to_host(src, n, seq, dst_pinned) -> None:
    """sgs_publish_to_host: src (device int32) -> dst_pinned (pinned host int32, >= n + 1 entries); seq: device int64 word."""
    L = _lib.lib()
    _need_gpu(src, seq)
    if dst_pinned.is_cuda or not dst_pinned.is_pinned() or dst_pinned.dtype != torch.int32 or dst_pinned.numel() < n + 1:
        raise RuntimeError("publish_to_host: destination must be a pinned host int32 tensor with n + 1 entries")
    _lib.check(L.sgs_publish_to_host(_ptr(src, torch.int32), n, None if seq is None else seq.data_ptr(), dst_pinned.data_ptr(), _stream()),
               "sgs_publish_to_host")


def _ce_kind(weight, eps):
    """Which entries of the library a criterion takes: ("", int32, ()) for the plain one (no class weight, no smoothing: sgs_masked_ce_*,
    sgs_hybrid_loss_fwd, the divisor word a count of train rows) and ("_w", float32, (weight, eps)) otherwise (sgs_masked_ce_w_*,
    sgs_hybrid_loss_w_fwd, the divisor `den` a sum of class weights).  The third item is what the weighted entries take in addition."""
    if weight is None and eps == 0.0:
        return "", torch.int32, ()
    return "_w", torch.float32, (_ptr(weight), eps)


def _masked_ce_fwd(logits, y, mask_u8, weight, eps):
    """Two launches: (loss [1], row_lse [N], rowloss [N], the divisor word [1]) of the rows on the mask."""
    L = _lib.lib()
    N, C = logits.shape
    dev = logits.device
    w_, norm_dtype, crit = _ce_kind(weight, eps)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    row_lse = torch.empty(N, dtype=torch.float32, device=dev)
    rowloss = torch.empty(N, dtype=torch.float32, device=dev)
    norm = torch.empty(1, dtype=norm_dtype, device=dev)
    name = f"sgs_masked_ce{w_}_fwd"
    _lib.check(getattr(L, name)(_ptr(logits), N, C, _ptr(y), _ptr(mask_u8), *crit, _ptr(loss), _ptr(row_lse), _ptr(rowloss), _ptr(norm), _stream()),
               name)
    return loss, row_lse, rowloss, norm


def _masked_ce_bwd(logits, y, mask_u8, weight, eps, row_lse, norm, g):
    """One launch: d logits (written, zero off the mask) for the upstream gradient g [1] and the divisor word `norm`."""
    L = _lib.lib()
    N, C = logits.shape
    w_, _, crit = _ce_kind(weight, eps)
    d = torch.empty_like(logits)
    name = f"sgs_masked_ce{w_}_bwd"
    _lib.check(getattr(L, name)(_ptr(logits), N, C, _ptr(y), _ptr(mask_u8), *crit, _ptr(row_lse), _ptr(norm), _ptr(g), _ptr(d), _stream()), name)
    return d


class _MaskedCE(torch.autograd.Function):
    """nn.CrossEntropyLoss(weight=w, label_smoothing=eps) over the rows on the mask: two launches forward, one backward; the divisor word
    (_ce_kind) is kept on the device for the backward."""

    @staticmethod
    def forward(ctx, logits, y, mask_u8, weight, eps):
        loss, row_lse, _, norm = _masked_ce_fwd(logits, y, mask_u8, weight, eps)
        ctx.save_for_backward(logits, y, mask_u8, weight, row_lse, norm)
        ctx.eps = eps
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        logits, y, mask_u8, weight, row_lse, norm = ctx.saved_tensors
        return _masked_ce_bwd(logits, y, mask_u8, weight, ctx.eps, row_lse, norm, g.reshape(1).contiguous().float()), None, None, None, None


def check_ce_spec(logits, weight, label_smoothing):
    """The class weight and smoothing of a weighted cross entropy as the library takes them: (weight or None, eps).  `weight` must be an
    fp32, contiguous tensor of length C on the logits' device; eps a number in [0, 1].  Raises ValueError naming the mismatch (before any
    device work: the kernels read `weight` through its pointer)."""
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"sgs_gnn_amd: label_smoothing must lie in [0, 1], got {label_smoothing!r}")
    if weight is None:
        return None, eps
    if not torch.is_tensor(weight):
        raise ValueError(f"sgs_gnn_amd: class weight must be a tensor, got {type(weight).__name__}")
    C = logits.shape[-1]
    if weight.dtype != torch.float32:
        raise ValueError(f"sgs_gnn_amd: class weight must be float32, got dtype {weight.dtype}")
    if weight.dim() != 1 or weight.numel() != C:
        raise ValueError(f"sgs_gnn_amd: class weight must have length C = {C}, got shape {tuple(weight.shape)}")
    if weight.device != logits.device:
        raise ValueError(f"sgs_gnn_amd: class weight is on device {weight.device}, the logits on {logits.device}")
    if not weight.is_contiguous():
        raise ValueError("sgs_gnn_amd: class weight must be contiguous")
    return weight.detach(), eps


def masked_cross_entropy(logits, y, train_mask, *, weight=None, label_smoothing=0.0):
    """nn.CrossEntropyLoss(weight=weight, label_smoothing=label_smoothing)(logits[train_mask], y[train_mask]) without the boolean-index
    sync.  With both keywords at their defaults: the plain chain (sgs_masked_ce_fwd / _bwd), otherwise the weighted one
    (sgs_masked_ce_w_fwd / _w_bwd); `weight`: check_ce_spec."""
    eps = 0.0
    if weight is not None or label_smoothing != 0.0:
        weight, eps = check_ce_spec(logits, weight, label_smoothing)
    _need_gpu(logits, y, train_mask)
    return _MaskedCE.apply(logits.contiguous(), y.contiguous(), _u8(train_mask), weight, eps)


class _EdgeReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, logits, sei, y, mask_u8, graph, coef1, coef2, box):
        L = _lib.lib()
        q = w.numel()
        N, C = logits.shape
        dev = w.device
        out = torch.empty(5, dtype=torch.float32, device=dev)
        ws = workspace(L.sgs_edge_reg_workspace_bytes(q), dev)
        _lib.check(L.sgs_edge_reg_fwd(_ptr(w), _ptr(sei), q, _ptr(logits), N, C, _ptr(y), _ptr(mask_u8), float(coef1), float(coef2),
                                      _ptr(out), None, ws.data_ptr(), ws.numel(), _stream()), "sgs_edge_reg_fwd")
        ctx.save_for_backward(w, logits, sei, y, mask_u8, out)
        ctx.graph, ctx.coef1, ctx.coef2 = graph, float(coef1), float(coef2)
        box.append(out)
        return out[4]              # 0-dim view of the saved [5] vector (no copy launch)

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        w, logits, sei, y, mask_u8, out = ctx.saved_tensors
        q = w.numel()
        N, C = logits.shape
        dev = w.device
        g = g.reshape(1).contiguous().float()
        dw = torch.empty(q, dtype=torch.float32, device=dev)
        Gs = torch.empty(q, C, dtype=torch.float32, device=dev)
        Gd = torch.empty(q, C, dtype=torch.float32, device=dev)
        _lib.check(L.sgs_edge_reg_bwd(_ptr(w), _ptr(sei), q, q, _ptr(logits), N, C, _ptr(y), _ptr(mask_u8), _ptr(out), ctx.coef1,
                                      ctx.coef2, _ptr(g), _ptr(dw), _ptr(Gs), _ptr(Gd), _stream()), "sgs_edge_reg_bwd")
        dlogits = _endpoint_reduce(Gs, Gd, None, ctx.graph, 1.0, 1.0, C) if ctx.coef2 != 0.0 else None
        return dw, dlogits, None, None, None, None, None, None, None


def edge_regularizers(w, logits, sampled_edge_index, y, train_mask, coef1, coef2):
    """coef1 * reg1 + coef2 * reg2 (training_hybrid.py:107-133) as one scalar, plus the detached
    [reg1, reg2, #valid, sum labels, total] vector."""
    _need_gpu(w, logits, sampled_edge_index, y, train_mask)
    graph = get_graph(sampled_edge_index, logits.shape[0])
    box = []
    total = _EdgeReg.apply(w.contiguous(), logits.contiguous(), sampled_edge_index.contiguous(), y.contiguous(),
                           _u8(train_mask), graph, float(coef1), float(coef2), box)
    return total, box[0]


class _HybridLoss(torch.autograd.Function):
    """criterion + coef1 reg1 + coef2 reg2 as ONE node: two launches forward (row losses and per-edge terms in one, one finishing
    block), one backward (the endpoint reduction forms each per-edge gradient term where it adds it, writes d w and adds the cross
    entropy's gradient) -- as separate nodes the same sum took ten, two of them the adds autograd inserts.  With coef2 == 0 the
    earlier chain (three launches forward, two backward): there the cross entropy's gradient is written, not accumulated."""

    @staticmethod
    def forward(ctx, logits, y, mask_u8, w, sei, graph, coef1, coef2, box, weight=None, eps=0.0):
        L = _lib.lib()
        q = w.numel()
        N, C = logits.shape
        dev = w.device
        out = torch.empty(7, dtype=torch.float32, device=dev)
        row_lse = torch.empty(N, dtype=torch.float32, device=dev)
        rowloss = torch.empty(N, dtype=torch.float32, device=dev)
        ws = workspace(L.sgs_edge_reg_workspace_bytes(q), dev)
        w_, norm_dtype, crit = _ce_kind(weight, eps)
        ctx.weighted = 1 if w_ else 0
        n_rows = torch.empty(1, dtype=norm_dtype, device=dev)          # the divisor word of the criterion (_ce_kind)
        stash = None
        if coef2 != 0.0:    # two launches; the per-edge scalars of the backward are kept (16 B per edge) when a gradient is wanted
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[3]:
                stash = torch.empty(q, 4, dtype=torch.float32, device=dev)
            _lib.check(L.sgs_hybrid_loss_fused_fwd(_ptr(logits), N, C, _ptr(y), _ptr(mask_u8), _ptr(w), _ptr(sei), q, float(coef1), float(coef2),
                                                   ctx.weighted, _ptr(weight), eps, _ptr(out), _ptr(row_lse), _ptr(rowloss), _ptr(n_rows),
                                                   _ptr(stash), ws.data_ptr(), ws.numel(), _stream()), "sgs_hybrid_loss_fused_fwd")
        else:
            name = f"sgs_hybrid_loss{w_}_fwd"
            _lib.check(getattr(L, name)(_ptr(logits), N, C, _ptr(y), _ptr(mask_u8), _ptr(w), _ptr(sei), q, float(coef1), float(coef2), *crit, _ptr(out),
                                        _ptr(row_lse), _ptr(rowloss), _ptr(n_rows), ws.data_ptr(), ws.numel(), _stream()), name)
        ctx.save_for_backward(logits, y, mask_u8, w, sei, out, row_lse, n_rows, weight, stash)
        ctx.eps = eps
        ctx.graph, ctx.coef1, ctx.coef2 = graph, float(coef1), float(coef2)
        ctx.nm_ref = getattr(w, "_sgs_norm", None)         # the normalisation that differentiates these weights, if any (note_first_dw)
        box.append(out)
        return out[6]

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        logits, y, mask_u8, w, sei, out, row_lse, n_rows, weight, stash = ctx.saved_tensors
        q = w.numel()
        N, C = logits.shape
        dev = w.device
        g = g.reshape(1).contiguous().float()
        dw = torch.empty(q, dtype=torch.float32, device=dev)
        if ctx.coef2 != 0.0:
            gr = ctx.graph
            dlogits = torch.empty_like(logits)
            _lib.check(L.sgs_hybrid_loss_fused_bwd(_ptr(logits), N, C, _ptr(y), _ptr(mask_u8), _ptr(w), q, _ptr(stash), _ptr(out), ctx.coef1,
                                                   ctx.weighted, _ptr(weight), ctx.eps, _ptr(row_lse), _ptr(n_rows), _ptr(g), _ptr(gr.in_ptr),
                                                   _ptr(gr.in_src), _ptr(gr.in_eid), _ptr(gr.out_ptr), _ptr(gr.out_dst), _ptr(gr.out_eid), _ptr(dw),
                                                   _ptr(dlogits), _stream()), "sgs_hybrid_loss_fused_bwd")
        else:               # today's chain: with coef2 == 0 the cross entropy's gradient is written, not accumulated
            Gs = torch.empty(q, C, dtype=torch.float32, device=dev)
            Gd = torch.empty(q, C, dtype=torch.float32, device=dev)
            _lib.check(L.sgs_edge_reg_bwd(_ptr(w), _ptr(sei), q, q, _ptr(logits), N, C, _ptr(y), _ptr(mask_u8), _ptr(out), ctx.coef1,
                                          ctx.coef2, _ptr(g), _ptr(dw), _ptr(Gs), _ptr(Gd), _stream()), "sgs_edge_reg_bwd")
            dlogits = _masked_ce_bwd(logits, y, mask_u8, weight, ctx.eps, row_lse, n_rows, g)
        nm = ctx.nm_ref() if ctx.nm_ref is not None else None
        if nm is not None and nm._park_ok and dw.numel() == nm.graph.n_edges:
            import weakref
            nm._dw_first = weakref.ref(dw)                 # the normalisation's backward accumulates into dw in place (no autograd add)
        return dlogits, None, None, dw, None, None, None, None, None, None, None


def hybrid_loss(logits, y, train_mask, w, sampled_edge_index, coef1, coef2, *, weight=None, label_smoothing=0.0):
    """nn.CrossEntropyLoss(weight=weight, label_smoothing=label_smoothing)(logits[train], y[train]) + coef1 * reg1 + coef2 * reg2
    (training_hybrid.py:105-133) as one scalar, plus the detached [reg1, reg2, #valid, sum labels, coef1 reg1 + coef2 reg2, cross entropy,
    loss] vector.  The regularisers never see the criterion; `weight`: check_ce_spec."""
    eps = 0.0
    if weight is not None or label_smoothing != 0.0:
        weight, eps = check_ce_spec(logits, weight, label_smoothing)
    _need_gpu(w, logits, sampled_edge_index, y, train_mask)
    graph = get_graph(sampled_edge_index, logits.shape[0])
    box = []
    total = _HybridLoss.apply(logits.contiguous(), y.contiguous(), _u8(train_mask), w.contiguous(), sampled_edge_index.contiguous(), graph,
                              float(coef1), float(coef2), box, weight, eps)
    return total, box[0]


# ------------------------------------------------------------------ GAT attention (K8)
class _GATAggregate(torch.autograd.Function):
    """out = act( sum_k alpha_k x'[src_k] + alpha_loop x'[i] + bias ), alpha = dropout(softmax(leaky_relu(a_s+a_d)))."""

    @staticmethod
    def forward(ctx, xl, a_s, a_d, bias, graph, slope, p_att, seed_att, site_att, act, p_act, seed_act, site_act):
        L = _lib.lib()
        N, D = xl.shape
        n = graph.n_edges
        dev = xl.device
        f32 = dict(dtype=torch.float32, device=dev)
        soft_in, alpha_in = torch.empty(max(n, 1), **f32), torch.empty(max(n, 1), **f32)
        soft_loop, alpha_loop = torch.empty(N, **f32), torch.empty(N, **f32)
        _lib.check(L.sgs_gat_alpha_fwd(_ptr(a_s), _ptr(a_d), N, n, _ptr(graph.in_ptr), _ptr(graph.in_src), _ptr(graph.in_eid),
                                       float(slope), float(p_att), seed_att, site_att, _ptr(soft_in), _ptr(soft_loop),
                                       _ptr(alpha_in), _ptr(alpha_loop), _stream()), "sgs_gat_alpha_fwd")
        Y = _spmm(xl, graph.in_ptr, graph.in_src, alpha_in, alpha_loop, bias, act, p_act, seed_act, site_act, N, D, n)
        ctx.save_for_backward(xl, a_s, a_d, soft_in, soft_loop, alpha_in, alpha_loop, Y if act != ACT_NONE else None)
        ctx.graph, ctx.slope, ctx.p_att, ctx.seed_att, ctx.site_att = graph, float(slope), float(p_att), seed_att, site_att
        ctx.act, ctx.p_act, ctx.has_bias = act, float(p_act), bias is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = _lib.lib()
        xl, a_s, a_d, soft_in, soft_loop, alpha_in, alpha_loop, Y = ctx.saved_tensors
        gr = ctx.graph
        N, D = xl.shape
        n = gr.n_edges
        dev = xl.device
        f32 = dict(dtype=torch.float32, device=dev)
        dZ, dbias = _grad_through_act(dY.contiguous(), Y, ctx.act, ctx.p_act, ctx.has_bias)
        # alpha re-ordered into src-CSR entry order for the transposed aggregation
        by_eid = torch.empty(max(n, 1), **f32)
        alpha_out = torch.empty(max(n, 1), **f32)
        _lib.check(L.sgs_scatter_by_eid(_ptr(alpha_in), _ptr(gr.in_eid), n, _ptr(by_eid), _stream()), "sgs_scatter_by_eid")
        _lib.check(L.sgs_gather_by_eid(_ptr(by_eid), _ptr(gr.out_eid), n, _ptr(alpha_out), _stream()), "sgs_gather_by_eid")
        dxl = _spmm(dZ, gr.out_ptr, gr.out_dst, alpha_out, alpha_loop, None, ACT_NONE, 0.0, 0, 0, N, D, n)
        galpha, gloop = torch.empty(max(n, 1), **f32), torch.empty(N, **f32)
        _lib.check(L.sgs_sddmm_csr(_ptr(dZ), _ptr(xl), N, D, n, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid), _ptr(galpha),
                                   _ptr(gloop), _stream()), "sgs_sddmm_csr")
        g_edge, g_self, d_ad = torch.empty(max(n, 1), **f32), torch.empty(N, **f32), torch.empty(N, **f32)
        _lib.check(L.sgs_gat_alpha_bwd(_ptr(a_s), _ptr(a_d), N, n, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid), ctx.slope,
                                       ctx.p_att, ctx.seed_att, ctx.site_att, _ptr(soft_in), _ptr(soft_loop), _ptr(galpha),
                                       _ptr(gloop), _ptr(g_edge), _ptr(g_self), _ptr(d_ad), _stream()), "sgs_gat_alpha_bwd")
        g_out = torch.empty(max(n, 1), **f32)
        _lib.check(L.sgs_gather_by_eid(_ptr(g_edge), _ptr(gr.out_eid), n, _ptr(g_out), _stream()), "sgs_gather_by_eid")
        ones = torch.ones(N, 1, **f32)
        d_as = _spmm(ones, gr.out_ptr, gr.out_dst, g_out, g_self, None, ACT_NONE, 0.0, 0, 0, N, 1, n).reshape(N)
        return dxl, d_as, d_ad, dbias, None, None, None, None, None, None, None, None, None


class _GATScores(torch.autograd.Function):
    """a_s = x' att_src, a_d = x' att_dst (GATConv's node-level dots) in one pass over x' (sgs_gat_scores_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, xl, att_s, att_d):
        L = _lib.lib()
        N, D = xl.shape
        a_s, a_d = torch.empty(N, dtype=torch.float32, device=xl.device), torch.empty(N, dtype=torch.float32, device=xl.device)
        _lib.check(L.sgs_gat_scores_fwd(_ptr(xl, torch.float32), N, D, _ptr(att_s), _ptr(att_d), _ptr(a_s), _ptr(a_d), _stream()), "sgs_gat_scores_fwd")
        ctx.save_for_backward(xl, att_s, att_d)
        return a_s, a_d

    @staticmethod
    def backward(ctx, g_s, g_d):
        L = _lib.lib()
        xl, att_s, att_d = ctx.saved_tensors
        N, D = xl.shape
        dev = xl.device
        g_s = torch.zeros(N, dtype=torch.float32, device=dev) if g_s is None else g_s.contiguous()
        g_d = torch.zeros(N, dtype=torch.float32, device=dev) if g_d is None else g_d.contiguous()
        dxl = torch.empty_like(xl)
        das, dad = torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
        ws = workspace(L.sgs_gat_scores_bwd_workspace_bytes(N, D), dev)
        _lib.check(L.sgs_gat_scores_bwd(_ptr(xl), N, D, _ptr(att_s), _ptr(att_d), _ptr(g_s), _ptr(g_d), 0, _ptr(dxl), _ptr(das), _ptr(dad), ws.data_ptr(),
                                        ws.numel(), _stream()), "sgs_gat_scores_bwd")
        return dxl, das, dad


# ---- multi-head GATConv (sgs_*_heads).  Per-edge arrays are [n, K] by edge id, so forward, transposed aggregation and the softmax
# backward share them through the CSRs' eid columns: backward = activation (as the one-head path) + 4 launches (transposed per-head SpMM,
# per-head SDDMM, softmax backward, by-source sum) against the one-head path's activation + 8.
HEADS_CONCAT, HEADS_MEAN, HEADS_BROADCAST = 0, 1, 2


def gat_heads_supported(heads: int, channels: int) -> bool:
    """Host-only: can the multi-head kernels take (heads, channels per head)?  (1 <= heads <= 16, channels >= 1.)"""
    return bool(_lib.lib().sgs_gat_heads_supported(int(heads), int(channels)))


def _spmm_heads(X, ptr, col, eid, val, diag, mode, bias, act, p, seed, site, N, K, C, nnz):
    L = _lib.lib()
    Y = torch.empty(N, C if mode == HEADS_MEAN else K * C, dtype=torch.float32, device=X.device)
    _lib.check(L.sgs_spmm_csr_heads(_ptr(X, torch.float32), N, K, C, nnz, _ptr(ptr), _ptr(col), _ptr(eid), _ptr(val), _ptr(diag), mode, _ptr(bias),
                                    act, float(p), seed, site, _ptr(Y), _stream()), "sgs_spmm_csr_heads")
    return Y


def _heads_alloc(n, N, K, f32):
    """(soft, alpha, soft_loop, alpha_loop): the per-edge [max(n, 1), K] (by edge id) and per-node [N, K] arrays a per-head softmax fills."""
    return torch.empty(max(n, 1), K, **f32), torch.empty(max(n, 1), K, **f32), torch.empty(N, K, **f32), torch.empty(N, K, **f32)


def _heads_forward(ctx, xl, graph, alpha, alpha_loop, bias, K, concat, sm, epi):
    """The aggregation launch of a per-head attention forward, and the context fields its backward reads whatever the softmax's family:
    `sm` = (slope, p_att, seed_att, site_att) of the softmax, `epi` = (act, p_act, seed_act, site_act) of the epilogue.  Returns Y."""
    N, D = xl.shape
    act, p_act, seed_act, site_act = epi
    Y = _spmm_heads(xl, graph.in_ptr, graph.in_src, graph.in_eid, alpha, alpha_loop, HEADS_CONCAT if concat else HEADS_MEAN, bias, act,
                    p_act, seed_act, site_act, N, K, D // K, graph.n_edges)
    ctx.graph, (ctx.slope, ctx.p_att, ctx.seed_att, ctx.site_att) = graph, sm
    ctx.act, ctx.p_act, ctx.has_bias, ctx.K, ctx.concat = act, p_act, bias is not None, K, bool(concat)
    return Y


def _heads_backward_head(ctx, dY, Y, xl, alpha, alpha_loop, f32):
    """What every per-head attention backward starts with, (dbias, dxl, galpha, gloop): the prologue, d x' over the src-CSR (the same
    alpha array through out_eid; concat = False: dZ [N, C] is shared by the heads, scaled by 1 / K) and the per-head SDDMM."""
    gr, K = ctx.graph, ctx.K
    N, D = xl.shape
    C, n = D // K, gr.n_edges
    dZ, dbias = _grad_through_act(dY.contiguous(), Y, ctx.act, ctx.p_act, ctx.has_bias)
    dxl = _spmm_heads(dZ, gr.out_ptr, gr.out_dst, gr.out_eid, alpha, alpha_loop, HEADS_CONCAT if ctx.concat else HEADS_BROADCAST, None,
                      ACT_NONE, 0.0, 0, 0, N, K, C, n)
    galpha, gloop = torch.empty(max(n, 1), K, **f32), torch.empty(N, K, **f32)
    _lib.check(_lib.lib().sgs_sddmm_csr_heads(_ptr(dZ), _ptr(xl), N, K, C, n, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid),
                                              0 if ctx.concat else 1, _ptr(galpha), _ptr(gloop), _stream()), "sgs_sddmm_csr_heads")
    return dbias, dxl, galpha, gloop


# ---- edge-weighted attention (GATConv edge_dim = 1 with the edge weight as the attribute; csrc/gat.hip, gat_alpha_heads_edge_*)
class EdgeAttr(Norm):
    """The edge weights of one forward as the GAT layers consume them: `w` [n_edges] by edge id and, when they require a gradient, the
    autograd `handle` through which the layers' d w flow back (a Norm, so that the layers report through _handle_grad like the GCN and
    Chebyshev heads: the second layer to finish adds the first one's d w on its way out and parks the total)."""
    __slots__ = ()


class _GATEdgeAttr(torch.autograd.Function):
    """The autograd edge from the layers' d w ([n_edges], edge-id order) back to the edge weights."""

    @staticmethod
    def forward(ctx, w, nm):
        ctx.nm = nm
        return torch.empty(w.numel(), dtype=torch.float32, device=w.device)

    @staticmethod
    def backward(ctx, g):
        extra, total, _ = _take_parked(ctx.nm)
        if extra is None:
            return g, None
        return (extra if total else g + extra), None         # total: the parked gradient already holds both layers' sum


def gat_edge_attr(graph: Graph, w) -> EdgeAttr:
    """Wrap the edge weights `w` [n_edges] f32 for ops.gat_aggregate(edge_weight=...).  One wrapper per forward is meant to be shared by
    both layers of the head, as one normalisation is by the GCN / Chebyshev layers."""
    _need_gpu(w)
    w = w.contiguous()
    if w.dtype != torch.float32 or w.numel() != graph.n_edges:
        raise RuntimeError(f"edge_weight must be float32 [{graph.n_edges}]")
    nm = EdgeAttr()
    nm.graph, nm.w = graph, w.detach()
    if w.requires_grad and torch.is_grad_enabled():
        nm.handle = _GATEdgeAttr.apply(w, nm)
        nm._park_ok = True        # _GATEdgeAttr.backward reads the parked second gradient
    return nm


class _GATAggregateHeads(torch.autograd.Function):
    """_GATAggregate for K heads: xl [N, K C] head-major, a_s / a_d [N, K]; out [N, K C] (concat) or the head mean [N, C].  With `nm`
    (an EdgeAttr; `coef` [K] and `handle` come with it, all three None otherwise) the logit carries the edge term w_e c_h (the loop's
    wbar_i c_h), K = 1 included.  Forward: 2 launches (softmax -- with the row's mean weight under the edge term --, aggregation);
    backward: the activation's + 4 (transposed per-head SpMM, per-head SDDMM, softmax backward, by-source sum), the softmax backward
    with its finishing sum of d c under the edge term (d w comes out of it too)."""

    @staticmethod
    def forward(ctx, xl, a_s, a_d, bias, coef, handle, nm, graph, K, concat, sm, epi):
        L = _lib.lib()
        N, n = xl.shape[0], graph.n_edges
        slope, p_att, seed_att, site_att = sm
        f32 = dict(dtype=torch.float32, device=xl.device)
        soft, alpha, soft_loop, alpha_loop = _heads_alloc(n, N, K, f32)
        loop = None
        if nm is None:
            _lib.check(L.sgs_gat_alpha_heads_fwd(_ptr(a_s), _ptr(a_d), N, K, n, _ptr(graph.in_ptr), _ptr(graph.in_src), _ptr(graph.in_eid),
                                                 slope, p_att, seed_att, site_att, _ptr(soft), _ptr(soft_loop), _ptr(alpha),
                                                 _ptr(alpha_loop), _stream()), "sgs_gat_alpha_heads_fwd")
        else:
            loop = torch.empty(2, max(N, 1), **f32)                # wbar, 1 / cnt
            _lib.check(L.sgs_gat_alpha_heads_edge_fwd(_ptr(a_s), _ptr(a_d), _ptr(nm.w, torch.float32), _ptr(coef, torch.float32), N, K, n,
                                                      _ptr(graph.in_ptr), _ptr(graph.in_src), _ptr(graph.in_eid), slope, p_att, seed_att,
                                                      site_att, _ptr(soft), _ptr(soft_loop), _ptr(alpha), _ptr(alpha_loop), loop[0].data_ptr(),
                                                      loop[1].data_ptr(), _stream()), "sgs_gat_alpha_heads_edge_fwd")
        Y = _heads_forward(ctx, xl, graph, alpha, alpha_loop, bias, K, concat, sm, epi)
        ctx.save_for_backward(xl, a_s, a_d, coef, soft, soft_loop, alpha, alpha_loop, loop, Y if ctx.act != ACT_NONE else None)
        ctx.nm = nm
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = _lib.lib()
        xl, a_s, a_d, coef, soft, soft_loop, alpha, alpha_loop, loop, Y = ctx.saved_tensors
        nm, gr, K = ctx.nm, ctx.graph, ctx.K
        N, n = xl.shape[0], gr.n_edges
        f32 = dict(dtype=torch.float32, device=xl.device)
        dbias, dxl, galpha, gloop = _heads_backward_head(ctx, dY, Y, xl, alpha, alpha_loop, f32)
        g_edge, g_self, d_ad = torch.empty(max(n, 1), K, **f32), torch.empty(N, K, **f32), torch.empty(N, K, **f32)
        dcoef = g_handle = None
        if nm is None:
            _lib.check(L.sgs_gat_alpha_heads_bwd(_ptr(a_s), _ptr(a_d), N, K, n, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid), ctx.slope,
                                                 ctx.p_att, ctx.seed_att, ctx.site_att, _ptr(soft), _ptr(soft_loop), _ptr(galpha), _ptr(gloop),
                                                 _ptr(g_edge), _ptr(g_self), _ptr(d_ad), _stream()), "sgs_gat_alpha_heads_bwd")
        else:
            second, dw_add = _dw_to_add(nm, n)
            dw, dcoef = torch.empty(n, **f32), (torch.empty(K, **f32) if N > 0 else torch.zeros(K, **f32))
            ws = workspace(L.sgs_gat_alpha_heads_edge_bwd_workspace_bytes(N, K), xl.device)
            _lib.check(L.sgs_gat_alpha_heads_edge_bwd(_ptr(a_s), _ptr(a_d), _ptr(nm.w), _ptr(coef), loop[0].data_ptr(), loop[1].data_ptr(), N, K,
                                                      n, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid), ctx.slope, ctx.p_att, ctx.seed_att,
                                                      ctx.site_att, _ptr(soft), _ptr(soft_loop), _ptr(galpha), _ptr(gloop), _ptr(dw_add),
                                                      _ptr(g_edge), _ptr(g_self), _ptr(d_ad), _ptr(dw), _ptr(dcoef), ws.data_ptr(), ws.numel(),
                                                      _stream()), "sgs_gat_alpha_heads_edge_bwd")
        d_as = torch.empty(N, K, **f32)
        _lib.check(L.sgs_edge_sum_by_row_heads(_ptr(g_edge), _ptr(g_self), N, K, n, _ptr(gr.out_ptr), _ptr(gr.out_eid), _ptr(d_as), _stream()),
                   "sgs_edge_sum_by_row_heads")
        if nm is not None and ctx.needs_input_grad[5]:
            g_handle = _report_dw(nm, dw, second)
        return (dxl, d_as, d_ad, dbias, dcoef, g_handle) + (None,) * 6


class _GATScoresHeads(torch.autograd.Function):
    """a_s[i, h] = <x'[i, h, :], att_src[h, :]>, a_d likewise, for K heads in one pass over x' (sgs_gat_scores_heads_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, xl, att_s, att_d, K):
        L = _lib.lib()
        N, D = xl.shape
        C = D // K
        a_s, a_d = torch.empty(N, K, dtype=torch.float32, device=xl.device), torch.empty(N, K, dtype=torch.float32, device=xl.device)
        _lib.check(L.sgs_gat_scores_heads_fwd(_ptr(xl, torch.float32), N, K, C, _ptr(att_s), _ptr(att_d), _ptr(a_s), _ptr(a_d), _stream()),
                   "sgs_gat_scores_heads_fwd")
        ctx.save_for_backward(xl, att_s, att_d)
        ctx.K = K
        return a_s, a_d

    @staticmethod
    def backward(ctx, g_s, g_d):
        L = _lib.lib()
        xl, att_s, att_d = ctx.saved_tensors
        K = ctx.K
        N, D = xl.shape
        C = D // K
        dev = xl.device
        g_s = torch.zeros(N, K, dtype=torch.float32, device=dev) if g_s is None else g_s.contiguous()
        g_d = torch.zeros(N, K, dtype=torch.float32, device=dev) if g_d is None else g_d.contiguous()
        dxl = torch.empty_like(xl)
        das, dad = torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
        ws = workspace(L.sgs_gat_scores_heads_bwd_workspace_bytes(N, K, C), dev)
        _lib.check(L.sgs_gat_scores_heads_bwd(_ptr(xl), N, K, C, _ptr(att_s), _ptr(att_d), _ptr(g_s), _ptr(g_d), 0, _ptr(dxl), _ptr(das), _ptr(dad),
                                              ws.data_ptr(), ws.numel(), _stream()), "sgs_gat_scores_heads_bwd")
        return dxl, das, dad, None


def _check_heads(xl, heads):
    heads = int(heads)
    if xl.dim() != 2 or heads < 1 or xl.shape[1] % heads != 0:
        raise RuntimeError(f"gat: x' must be [N, heads * channels] (got {tuple(xl.shape)} for heads = {heads})")
    if not gat_heads_supported(heads, xl.shape[1] // heads):
        raise RuntimeError(f"gat: unsupported heads = {heads} x channels = {xl.shape[1] // heads} (1 <= heads <= 16, channels >= 1)")
    return heads


def gat_scores(xl, att_src, att_dst, heads=1):
    """Node-level attention scores: heads = 1 -> two [N] vectors (the one-head kernels); heads = K > 1 -> two [N, K] matrices from
    x' [N, K C] (head-major columns) and att_* with K C elements ([1, K, C])."""
    _need_gpu(xl, att_src, att_dst)
    if heads == 1:
        return _GATScores.apply(xl.contiguous(), att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous())
    heads = _check_heads(xl, heads)
    return _GATScoresHeads.apply(xl.contiguous(), att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous(), heads)


def gat_aggregate(xl, a_s, a_d, bias, graph: Graph, negative_slope=0.2, p_att=0.0, seed_att=0, site_att=0, act=ACT_NONE,
                  p_act=0.0, seed_act=0, site_act=0, heads=1, concat=True, *, edge_weight=None, edge_coef=None):
    """Attention softmax + aggregation (+ bias / act / dropout).  heads = 1: the one-head kernels (`concat` has no effect on one head).
    heads = K > 1: per-head softmax over x' [N, K C]; concat=True -> [N, K C], False -> the mean over heads [N, C]; `bias` matches.
    `edge_weight` ([n_edges] f32 by edge id, or the EdgeAttr that gat_edge_attr made of it for both layers) with `edge_coef` [heads] adds
    edge_weight[e] * edge_coef[h] to the logits (GATConv edge_dim = 1; the added loops carry their node's mean in-weight) on the per-head
    kernels for every 1 <= heads <= 16, differentiable wrt both; both None (the default) = the kernels above, unchanged."""
    _need_gpu(xl, a_s, a_d, bias)
    if (edge_weight is None) != (edge_coef is None):
        raise RuntimeError("gat_aggregate: edge_weight and edge_coef come together")
    if edge_weight is not None:
        return _gat_aggregate_edge(xl, a_s, a_d, bias, graph, negative_slope, p_att, seed_att, site_att, act, p_act, seed_act, site_act, heads,
                                   concat, edge_weight, edge_coef)
    if heads == 1:
        return _GATAggregate.apply(xl.contiguous(), a_s.contiguous(), a_d.contiguous(), bias, graph, float(negative_slope),
                                   float(p_att), int(seed_att), int(site_att), act, float(p_act), int(seed_act), int(site_act))
    heads = _check_heads(xl, heads)
    if tuple(a_s.shape) != (xl.shape[0], heads) or tuple(a_d.shape) != (xl.shape[0], heads):
        raise RuntimeError("gat_aggregate: a_s / a_d must be [N, heads]")
    width = xl.shape[1] if concat else xl.shape[1] // heads
    if bias is not None and bias.numel() != width:
        raise RuntimeError(f"gat_aggregate: bias must have {width} elements")
    return _GATAggregateHeads.apply(xl.contiguous(), a_s.contiguous(), a_d.contiguous(), bias, None, None, None, graph, heads, bool(concat),
                                    (float(negative_slope), float(p_att), int(seed_att), int(site_att)),
                                    (act, float(p_act), int(seed_act), int(site_act)))


def _gat_aggregate_edge(xl, a_s, a_d, bias, graph, negative_slope, p_att, seed_att, site_att, act, p_act, seed_act, site_act, heads, concat,
                        edge_weight, edge_coef):
    nm = edge_weight if isinstance(edge_weight, EdgeAttr) else gat_edge_attr(graph, edge_weight)
    _need_gpu(nm.w, edge_coef)
    if nm.graph is not graph:
        raise RuntimeError("gat_aggregate: edge_weight was wrapped for another graph")
    heads = _check_heads(xl, heads)
    N = xl.shape[0]
    if a_s.numel() != N * heads or a_d.numel() != N * heads:
        raise RuntimeError("gat_aggregate: a_s / a_d must be [N, heads]")
    if edge_coef.numel() != heads or edge_coef.dtype != torch.float32:
        raise RuntimeError(f"gat_aggregate: edge_coef must be float32 [{heads}]")
    width = xl.shape[1] if concat else xl.shape[1] // heads
    if bias is not None and bias.numel() != width:
        raise RuntimeError(f"gat_aggregate: bias must have {width} elements")
    return _GATAggregateHeads.apply(xl.contiguous(), a_s.reshape(N, heads).contiguous(), a_d.reshape(N, heads).contiguous(), bias,
                                    edge_coef.reshape(heads).contiguous(), nm.handle, nm, graph, heads, bool(concat),
                                    (float(negative_slope), float(p_att), int(seed_att), int(site_att)),
                                    (act, float(p_act), int(seed_act), int(site_act)))


# ---- GATv2 attention (GATv2Conv: the non-linearity inside the dot product; csrc/gatv2.hip, sgs_gatv2_*)
class _GATv2Aggregate(torch.autograd.Function):
    """out = act( sum_k alpha_k xl[src_k] + alpha_loop xl[i] + bias ), alpha = dropout(softmax_h(att_h . leaky_relu(xl[src] + xr[i] (+ w le)))).
    Forward: 2 launches (gathering softmax, aggregation); backward: the activation's + 5 (transposed per-head SpMM, per-head SDDMM, the
    by-destination softmax backward with its finishing sum, the by-source d xl).  `nm` None: no edge term."""

    @staticmethod
    def forward(ctx, xl, xr, att, bias, le, handle, nm, graph, K, concat, sm, epi):
        L = _lib.lib()
        N, D = xl.shape
        C = D // K
        n = graph.n_edges
        slope, p_att, seed_att, site_att = sm
        f32 = dict(dtype=torch.float32, device=xl.device)
        edge = nm is not None and n > 0                        # without edges every loop carries weight 0: the term vanishes
        soft, alpha, soft_loop, alpha_loop = _heads_alloc(n, N, K, f32)
        loop = torch.empty(2, max(N, 1), **f32) if edge else None                  # wbar, 1 / cnt
        _lib.check(L.sgs_gatv2_alpha_heads_fwd(_ptr(xl, torch.float32), _ptr(xr, torch.float32), _ptr(att, torch.float32),
                                               _ptr(nm.w, torch.float32) if edge else None, _ptr(le, torch.float32) if edge else None, N, K, C, n,
                                               _ptr(graph.in_ptr), _ptr(graph.in_src), _ptr(graph.in_eid), slope, p_att, seed_att,
                                               site_att, _ptr(soft), _ptr(soft_loop), _ptr(alpha), _ptr(alpha_loop),
                                               loop[0].data_ptr() if edge else None, loop[1].data_ptr() if edge else None, _stream()),
                   "sgs_gatv2_alpha_heads_fwd")
        Y = _heads_forward(ctx, xl, graph, alpha, alpha_loop, bias, K, concat, sm, epi)
        ctx.save_for_backward(xl, xr, att, le, soft, soft_loop, alpha, alpha_loop, loop, Y if ctx.act != ACT_NONE else None)
        ctx.nm, ctx.edge = nm, edge
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = _lib.lib()
        xl, xr, att, le, soft, soft_loop, alpha, alpha_loop, loop, Y = ctx.saved_tensors
        nm, gr, K, edge = ctx.nm, ctx.graph, ctx.K, ctx.edge
        N, D = xl.shape
        C = D // K
        n = gr.n_edges
        f32 = dict(dtype=torch.float32, device=xl.device)
        dbias, dxl, galpha, gloop = _heads_backward_head(ctx, dY, Y, xl, alpha, alpha_loop, f32)
        g_logit, g_loop = torch.empty(max(n, 1), K, **f32), torch.empty(N, K, **f32)
        dxr = torch.empty_like(xr)
        datt = torch.empty(D, **f32) if N > 0 else torch.zeros(D, **f32)
        dle = dw = dw_add = None
        second = False
        if edge:
            second, dw_add = _dw_to_add(nm, n)
            dw, dle = torch.empty(n, **f32), torch.empty(D, **f32)
        elif le is not None:
            dle = torch.zeros(D, **f32)
        ws = workspace(L.sgs_gatv2_alpha_heads_bwd_workspace_bytes(N, K, C), xl.device)
        w_ptr, le_ptr = (_ptr(nm.w), _ptr(le)) if edge else (None, None)
        wb_ptr, ic_ptr = (loop[0].data_ptr(), loop[1].data_ptr()) if edge else (None, None)
        _lib.check(L.sgs_gatv2_alpha_heads_bwd(_ptr(xl), _ptr(xr), _ptr(att), w_ptr, le_ptr, wb_ptr, ic_ptr, N, K, C, n, _ptr(gr.in_ptr),
                                               _ptr(gr.in_src), _ptr(gr.in_eid), ctx.slope, ctx.p_att, ctx.seed_att, ctx.site_att, _ptr(soft),
                                               _ptr(soft_loop), _ptr(galpha), _ptr(gloop), _ptr(dw_add), _ptr(g_logit), _ptr(g_loop), _ptr(dxr),
                                               _ptr(datt), _ptr(dle) if edge else None, _ptr(dw), ws.data_ptr(), ws.numel(), _stream()),
                   "sgs_gatv2_alpha_heads_bwd")
        _lib.check(L.sgs_gatv2_dxl_heads(_ptr(xl), _ptr(xr), _ptr(att), w_ptr, le_ptr, wb_ptr, _ptr(g_logit), _ptr(g_loop), N, K, C, n,
                                         _ptr(gr.out_ptr), _ptr(gr.out_dst), _ptr(gr.out_eid), ctx.slope, 1, _ptr(dxl), _stream()),
                   "sgs_gatv2_dxl_heads")
        g_handle = None
        if ctx.needs_input_grad[5]:
            g_handle = _report_dw(nm, dw, second) if edge else _handle_grad(nm, torch.zeros(n, **f32))
        return (dxl, dxr, datt, dbias, dle, g_handle) + (None,) * 6


def gatv2_aggregate(xl, xr, att, bias, graph: Graph, negative_slope=0.2, p_att=0.0, seed_att=0, site_att=0, act=ACT_NONE, p_act=0.0,
                    seed_act=0, site_act=0, heads=1, concat=True, *, edge_weight=None, lin_edge=None):
    """GATv2Conv's attention softmax + aggregation (+ bias / act / dropout) as one autograd node, for 1 <= heads <= 16:
    xl = lin_l(x), xr = lin_r(x) [N, heads C] (head-major columns), att with heads C elements ([1, heads, C]); the logit of an entry j -> i
    is att_h . leaky_relu(xl[j, h] + xr[i, h]) (+ edge_weight[e] lin_edge[h] inside the leaky_relu).  concat=True -> [N, heads C], False ->
    the mean over heads [N, C]; `bias` matches.  `edge_weight` ([n_edges] f32 by edge id, or the EdgeAttr that gat_edge_attr made of it for
    both layers) comes with `lin_edge` (lin_edge.weight, heads C elements); the added loops carry their node's mean in-weight.
    Differentiable wrt xl, xr, att, bias, lin_edge and the edge weights; dropout sites and keys are gat_aggregate's."""
    _need_gpu(xl, xr, att, bias, lin_edge)
    if (edge_weight is None) != (lin_edge is None):
        raise RuntimeError("gatv2_aggregate: edge_weight and lin_edge come together")
    heads = _check_heads(xl, heads)
    N, D = xl.shape
    if tuple(xr.shape) != (N, D) or att.numel() != D or xl.dtype != torch.float32 or xr.dtype != torch.float32 or att.dtype != torch.float32:
        raise RuntimeError(f"gatv2_aggregate: xr must be float32 [{N}, {D}] like xl and att have {D} elements")
    width = D if concat else D // heads
    if bias is not None and bias.numel() != width:
        raise RuntimeError(f"gatv2_aggregate: bias must have {width} elements")
    nm = handle = le = None
    if edge_weight is not None:
        nm = edge_weight if isinstance(edge_weight, EdgeAttr) else gat_edge_attr(graph, edge_weight)
        _need_gpu(nm.w)
        if nm.graph is not graph:
            raise RuntimeError("gatv2_aggregate: edge_weight was wrapped for another graph")
        if lin_edge.numel() != D or lin_edge.dtype != torch.float32:
            raise RuntimeError(f"gatv2_aggregate: lin_edge must be float32 with {D} elements")
        handle, le = nm.handle, lin_edge.reshape(D).contiguous()
    return _GATv2Aggregate.apply(xl.contiguous(), xr.contiguous(), att.reshape(D).contiguous(), bias, le, handle, nm, graph, heads, bool(concat),
                                 (float(negative_slope), float(p_att), int(seed_att), int(site_att)),
                                 (act, float(p_act), int(seed_act), int(site_act)))


# ---- GINE aggregation (GINEConv, edge_dim = 1 with the edge weight as the attribute; csrc/gine.hip, sgs_gine_aggregate_*)
def edge_attr(graph: Graph, w=None) -> EdgeAttr:
    """The edge weights of one forward as the edge-attribute layers consume them (gat_edge_attr under its general name), shared by both
    layers of a head.  `w` None: unit weights (an EdgeAttr without weights and without an autograd handle)."""
    if w is not None:
        return gat_edge_attr(graph, w)
    nm = EdgeAttr()
    nm.graph = graph
    return nm


class _GINEAggregate(torch.autograd.Function):
    """z = diag x + sum_{j -> i} relu(x_j + (w_e a + b)): one launch forward; backward one launch over the src-CSR (d x, d w by edge id,
    per-workgroup partials of d a / d b) plus their finishing sum.  No mask is saved: the backward recomputes it (see csrc/gine.hip)."""

    @staticmethod
    def forward(ctx, x, a, b, handle, nm, diag):
        L = _lib.lib()
        gr = nm.graph
        N, D = x.shape
        z = torch.empty(N, D, dtype=torch.float32, device=x.device)
        _lib.check(L.sgs_gine_aggregate_fwd(_ptr(x, torch.float32), _ptr(nm.w, torch.float32), _ptr(a, torch.float32), _ptr(b, torch.float32),
                                            diag, N, D, gr.n_edges, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid), _ptr(z), _stream()),
                   "sgs_gine_aggregate_fwd")
        ctx.save_for_backward(x, a, b)
        ctx.nm, ctx.diag = nm, diag
        return z

    @staticmethod
    def backward(ctx, dZ):
        L = _lib.lib()
        x, a, b = ctx.saved_tensors
        nm, gr = ctx.nm, ctx.nm.graph
        N, D = x.shape
        n = gr.n_edges
        f32 = dict(dtype=torch.float32, device=x.device)
        dZ = dZ.contiguous()
        dx = torch.empty(N, D, **f32) if ctx.needs_input_grad[0] else None      # (the first layer's input: neither written nor allocated)
        want_ab = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dab = torch.empty(2, D, **f32) if want_ab else None
        want_w = nm.handle is not None and ctx.needs_input_grad[3]
        dw = dw_add = None
        second = False
        if want_w:
            second, dw_add = _dw_to_add(nm, n)
            dw = torch.empty(n, **f32)
        ws = workspace(L.sgs_gine_aggregate_bwd_workspace_bytes(N, D), x.device) if want_ab else None
        _lib.check(L.sgs_gine_aggregate_bwd(_ptr(x), _ptr(dZ, torch.float32), _ptr(nm.w), _ptr(a), _ptr(b), ctx.diag, N, D, n, _ptr(gr.out_ptr),
                                            _ptr(gr.out_dst), _ptr(gr.out_eid), _ptr(dw_add), _ptr(dx), _ptr(dw),
                                            dab[0].data_ptr() if want_ab else None, dab[1].data_ptr() if want_ab else None,
                                            ws.data_ptr() if want_ab else None, ws.numel() if want_ab else 0, _stream()),
                   "sgs_gine_aggregate_bwd")
        g_handle = _report_dw(nm, dw, second) if want_w else None
        return dx, (dab[0] if want_ab else None), (dab[1] if want_ab else None), g_handle, None, None


def gine_aggregate(x, attr: EdgeAttr, a, b, diag: float = 1.0):
    """GINEConv's aggregation z_i = diag x_i + sum_{e: j -> i} relu(x_j + (w_e a + b)) as one autograd node.  x float32 [N, D]; `attr` =
    ops.edge_attr(graph, edge_weight) (one per forward, shared by both layers; without weights every w_e is 1 and there is no gradient to
    them); a, b with D elements (lin.weight of Linear(1, D) and its bias).  Differentiable wrt x, a, b and the edge weights."""
    if not isinstance(attr, EdgeAttr):
        raise RuntimeError("gine_aggregate: attr must come from ops.edge_attr(graph, edge_weight)")
    _need_gpu(x, a, b, attr.w)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != attr.graph.N or x.shape[1] < 1:
        raise RuntimeError(f"gine_aggregate: x must be float32 [{attr.graph.N}, D >= 1]")
    D = x.shape[1]
    if a.numel() != D or b.numel() != D or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError(f"gine_aggregate: a and b must be float32 with {D} elements")
    return _GINEAggregate.apply(x.contiguous(), a.reshape(D).contiguous(), b.reshape(D).contiguous(), attr.handle, attr, float(diag))


# ------------------------------------------------------------------ node-level Linear with a hand-written weight gradient
class _LinearNoBias(torch.autograd.Function):
    """y = x W^T (library GEMM); dW = dY^T x on the f32 matrix cores (sgs_gemm_tn); dx = dY W (library)."""

    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return x @ W.t()                     # W may be a strided view (e.g. fc1.weight[:, H:])

    @staticmethod
    def backward(ctx, dY):
        L = _lib.lib()
        x, W = ctx.saved_tensors
        dx = dW = None
        dY = dY.contiguous()
        if ctx.needs_input_grad[0]:
            dx = dY @ W
        if ctx.needs_input_grad[1]:
            dW = _leaf_dw(dY, x.contiguous(), x.shape[0], W.shape[0], W.shape[1], leaf=(ctx, 1))
        return dx, dW


def linear_nobias(x, W):
    _need_gpu(x, W)
    return _LinearNoBias.apply(x, W)


# ------------------------------------------------------------------ GraphSAGE mean aggregation, device-side degree prior
def mean_norm(graph: Graph) -> Norm:
    """Norm-like object for SAGEConv's mean aggregation: weights 1/indeg(dst), no self-loop term."""
    L = _lib.lib()
    dev = graph.edge_index.device
    nm = Norm()
    nm.graph = graph
    ne = max(graph.n_edges, 1)
    nm.what_in = torch.empty(ne, dtype=torch.float32, device=dev)
    nm.what_out = torch.empty(ne, dtype=torch.float32, device=dev)
    _lib.check(L.sgs_mean_weights(graph.n_edges, graph.N, _ptr(graph.in_ptr), _ptr(graph.out_ptr), _ptr(graph.out_dst),
                                  _ptr(nm.what_in), _ptr(nm.what_out), _stream()), "sgs_mean_weights")
    return nm


def sum_norm(graph: Graph, diag: float = 1.0) -> Norm:
    """Norm-like object for GINConv's sum aggregation: unit edge weights and `diag` = 1 + eps on the node itself."""
    nm = getattr(graph, "_norm_sum", None)
    if nm is not None and nm[0] == diag:
        return nm[1]
    dev = graph.edge_index.device
    nm = Norm()
    nm.graph = graph
    ne = max(graph.n_edges, 1)
    nm.what_in = torch.ones(ne, dtype=torch.float32, device=dev)
    nm.what_out = nm.what_in
    nm.what_loop = torch.full((max(graph.N, 1),), float(diag), dtype=torch.float32, device=dev)
    graph._norm_sum = (diag, nm)
    return nm


def degree_prior(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """`data.prob` of datasets.py:141-156 (add_degree) computed on the device."""
    L = _lib.lib()
    _need_gpu(edge_index)
    g = get_graph(edge_index, num_nodes)
    E = edge_index.shape[1]
    logits = torch.empty(E, dtype=torch.float32, device=edge_index.device)
    _lib.check(L.sgs_degree_prior_logits(_ptr(g.edge_index), E, num_nodes, _ptr(g.in_ptr), _ptr(g.out_ptr), _ptr(logits), _stream()),
               "sgs_degree_prior_logits")
    return torch.softmax(logits, dim=0)


def er_prior(edge_index: torch.Tensor, num_nodes: int, seed: int = 0, walk_lengths: int = 4, walks: int = 100, raw: bool = False) -> torch.Tensor:
    """`data.prob` of datasets.py:159-173 (add_ER) computed on the device: random-walk effective-resistance weights
    (sgs_er_weight) then softmax(weight * E^-1/2).  `edge_index` must be symmetric and coalesced (what the reference's
    to_networkx(to_undirected=True) walks on); raw=True returns the un-normalised weights."""
    L = _lib.lib()
    _need_gpu(edge_index)
    g = get_graph(edge_index, num_nodes)
    E = edge_index.shape[1]
    w = torch.empty(E, dtype=torch.float32, device=edge_index.device)
    _lib.check(L.sgs_er_weight(_ptr(g.edge_index), E, num_nodes, _ptr(g.out_ptr), _ptr(g.out_dst), int(walk_lengths), int(walks), int(seed),
                               _ptr(w), _stream()), "sgs_er_weight")
    return w if raw else torch.softmax(w * E ** -0.5, dim=0)


# ------------------------------------------------------------------ sparse node features (CitationFull-Cora: bag-of-words rows, 0.7 % dense)
class FeatCSR:
    """CSR of a sparse feature matrix x [N, F] and of its transpose, built once per graph: the node-level products of the first GCN
    layers, x W^T and d W = d Y^T x, are then two SpMMs over nnz(x) instead of two dense [N, F] x [F, H] GEMMs (model.py:159 feeds the
    raw bag-of-words rows to GCNConv.lin: 88 GFLOP per product at CitationFull-Cora's size, 0.6 GFLOP of it on non-zeros)."""
    __slots__ = ("N", "F", "nnz", "ptr", "col", "val", "tptr", "trow", "tval")


_FEAT_SPARSE_MAX_DENSITY = 0.05        # above this the library GEMM wins
_FEAT_SPARSE_MIN_ELEMS = 1 << 22       # small matrices: not worth a second code path


def feature_csr(x: torch.Tensor, build: bool = False):
    """FeatCSR of `x` if it is sparse enough (cached on the tensor, keyed by its version), else None.  Building reads the non-zero count
    back (set-up work, once per graph): only the models' FIRST layers ask for it (`build=True`, on the batch's resident x); the products
    themselves just look the cache up.  Inside a stream capture only an existing cache entry is used."""
    c = getattr(x, "_sgs_fcsr", None)
    if c is not None and c[1] == x._version:
        return c[0]
    if not build or not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32 or x.numel() < _FEAT_SPARSE_MIN_ELEMS or x.requires_grad:
        return None
    if torch.cuda.is_current_stream_capturing():
        return None
    N, F_ = x.shape
    nz = x != 0
    nnz = int(nz.sum())
    fc = None
    if nnz <= _FEAT_SPARSE_MAX_DENSITY * x.numel() and nnz < 2**31:
        fc = FeatCSR()
        idx = torch.nonzero(nz)                                    # row-major: sorted by (row, col)
        rows, cols = idx[:, 0], idx[:, 1]
        val = x[rows, cols].contiguous()
        i32 = dict(dtype=torch.int32, device=x.device)
        fc.N, fc.F, fc.nnz = N, F_, nnz
        fc.ptr = torch.zeros(N + 1, **i32)
        fc.ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0).to(torch.int32)
        fc.col, fc.val = cols.to(torch.int32).contiguous(), val
        order = torch.argsort(cols, stable=True)                   # the transpose: sorted by (col, row)
        fc.tptr = torch.zeros(F_ + 1, **i32)
        fc.tptr[1:] = torch.cumsum(torch.bincount(cols, minlength=F_), 0).to(torch.int32)
        fc.trow, fc.tval = rows[order].to(torch.int32).contiguous(), val[order].contiguous()
    try:
        x._sgs_fcsr = (fc, x._version)
    except Exception:
        pass
    return fc


def _x_wt(x, W):
    """x W^T: over the non-zeros of x when it has a FeatCSR (gathering rows of W^T), else the library GEMM."""
    fc = feature_csr(x)
    if fc is None:
        return x @ W.t()
    Wt = W.t().contiguous()                                        # [F, H]
    return _spmm(Wt, fc.ptr, fc.col, fc.val, None, None, ACT_NONE, 0.0, 0, 0, fc.N, W.shape[0], fc.nnz)


def _dyt_x(dY, x, W_shape, leaf=None):
    """d W [M, F] = d Y^T x: over the non-zeros of x^T when x has a FeatCSR, else sgs_gemm_tn (`leaf`: see _leaf_dw)."""
    fc = feature_csr(x)
    M, Nn = W_shape
    if fc is not None:
        dWt = _spmm(dY.contiguous(), fc.tptr, fc.trow, fc.tval, None, None, ACT_NONE, 0.0, 0, 0, fc.F, M, fc.nnz)      # [F, M]
        return dWt.t().contiguous()
    return _leaf_dw(dY, x.contiguous(), x.shape[0], M, Nn, leaf=leaf)


# ------------------------------------------------------------------ one GCN layer as ONE autograd node
class _GCNLayer(torch.autograd.Function):
    """Y = act(A_hat (x W^T) + bias): the node-level product (library GEMM) and the propagation (K5) in a single
    autograd node -- the step is launch/host-bound at partition scale, so halving the Python nodes per layer matters.
    `xl` may be supplied (memoised x W^T shared by the learned and the random forward of one step)."""

    @staticmethod
    def forward(ctx, x, W, handle, bias, nm, act, p, seed, site, xl):
        gr = nm.graph
        if xl is None:
            xl = _x_wt(x, W)
        N, D = xl.shape
        Y = _spmm(xl, gr.in_ptr, gr.in_src, nm.what_in, nm.what_loop, bias, act, p, seed, site, N, D, gr.n_edges)
        ctx.nm, ctx.act, ctx.p = nm, act, p
        ctx.has_bias, ctx.has_handle = bias is not None, handle is not None
        ctx.save_for_backward(x, W, xl, Y if act != ACT_NONE else None)
        ctx.mark_non_differentiable(xl)
        ctx.set_materialize_grads(False)        # no zero-filled [N, D] gradient for the (never differentiated) xl output
        return Y, xl

    @staticmethod
    def backward(ctx, dY, _dxl_unused):
        L = _lib.lib()
        nm, gr = ctx.nm, ctx.nm.graph
        x, W, xl, Y = ctx.saved_tensors
        N, D = xl.shape
        dY = dY.contiguous()
        dx = dW = g = None
        want_db = ctx.has_bias and ctx.needs_input_grad[3]
        dZ, dbias = _grad_through_act(dY, Y, ctx.act, ctx.p, want_db, colsum_now=False)
        need_x, need_W = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if need_x or need_W:
            dxl = _spmm(dZ, gr.out_ptr, gr.out_dst, nm.what_out, nm.what_loop, None, ACT_NONE, 0.0, 0, 0, N, D, gr.n_edges)
            if need_W:
                dW = _dyt_x(dxl, x, W.shape, leaf=(ctx, 1))
            if need_x:
                dx = dxl @ W
        if ctx.has_handle and ctx.needs_input_grad[2]:
            g = torch.empty(gr.n_edges + gr.N, dtype=torch.float32, device=dY.device)
            gw, gl = g[:gr.n_edges], g[gr.n_edges:]
            _lib.check(L.sgs_sddmm_csr(_ptr(dZ), _ptr(xl), N, D, gr.n_edges, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid),
                                       gw.data_ptr(), gl.data_ptr(), _stream()), "sgs_sddmm_csr")
        if want_db and dbias is None:
            dbias = _colsum(dZ)
        return dx, dW, (_handle_grad(nm, g) if g is not None else None), dbias, None, None, None, None, None, None


def gcn_layer(x, W, bias, nm: Norm, act=ACT_NONE, p=0.0, seed=0, site=0, xl=None):
    """act(A_hat (x W^T) + bias) with autograd to x, W, bias and (through nm.handle) the edge weights.
    Returns (Y, xl) where xl = x W^T (detached) can be passed back in for another graph over the same x, W."""
    _need_gpu(x, W, bias)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != nm.graph.N:
        raise RuntimeError("gcn_layer: x must be float32 [N, F]")
    return _GCNLayer.apply(x, W, nm.handle, bias, nm, act, float(p), int(seed), int(site), xl)


# ------------------------------------------------------------------ two GCN layers as ONE autograd node (the GNN head)
def _pair_ok(gr, *widths):
    """sgs_gcn_pair_ok for every LDS-kept row width: the fused pair kernels apply (partition scale: sgs_spmm_csr's row-block path)."""
    L = _lib.lib()
    return all(L.sgs_gcn_pair_ok(gr.N, gr.n_edges, int(w)) for w in widths)


class _GCN2(torch.autograd.Function):
    """out = A_hat (h W2^T) + b2 with h = act(A_hat (x W1^T) + b1).  On the row-block path the first SpMM also emits h W2^T
    (sgs_spmm_csr_next) and the backward's second-layer SpMM also emits dZ1 = (dxl2 W2) * act'(h) and d b2 (sgs_spmm_csr_bwd_prev),
    the first-layer one d b1: the library GEMMs and column sums between the SpMMs lose their launches.  Elsewhere the two layers are
    exactly _GCNLayer's calls.  `xl1` may be supplied (memoised x W1^T shared by the learned and the random forward of one step)."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, handle, nm, act, p, seed, site, xl1, pre=None):
        L = _lib.lib()
        gr = nm.graph
        if xl1 is None:
            xl1 = _x_wt(x, W1)
        N, H = xl1.shape
        C = W2.shape[0]
        fused = _pair_ok(gr, H, C) and xl1.is_contiguous() and W2.is_contiguous() and W2.shape[1] == H
        if pre is not None:       # (h, xl2, out) of this very forward, already computed on the fused path as one job of gcn2_dual's launches
            h, xl2, out = pre
        elif fused:
            h = torch.empty(N, H, dtype=torch.float32, device=xl1.device)
            xl2 = torch.empty(N, C, dtype=torch.float32, device=xl1.device)
            _lib.check(L.sgs_spmm_csr_next(_ptr(xl1, torch.float32), N, H, gr.n_edges, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(nm.what_in),
                                           _ptr(nm.what_loop), _ptr(b1), act, float(p), seed, site, _ptr(W2, torch.float32), C, _ptr(h),
                                           _ptr(xl2), _stream()), "sgs_spmm_csr_next")
        else:
            h = _spmm(xl1, gr.in_ptr, gr.in_src, nm.what_in, nm.what_loop, b1, act, p, seed, site, N, H, gr.n_edges)
            xl2 = h @ W2.t()
        if pre is None:
            out = _spmm(xl2, gr.in_ptr, gr.in_src, nm.what_in, nm.what_loop, b2, ACT_NONE, 0.0, 0, 0, N, C, gr.n_edges)
        ctx.nm, ctx.act, ctx.p, ctx.fused = nm, act, p, fused
        ctx.has_b1, ctx.has_b2, ctx.has_handle = b1 is not None, b2 is not None, handle is not None
        ctx.save_for_backward(x, W1, xl1, h, W2, xl2)
        ctx.mark_non_differentiable(xl1)
        ctx.set_materialize_grads(False)
        return out, xl1

    @staticmethod
    def backward(ctx, dout, _dxl_unused):
        L = _lib.lib()
        nm, gr = ctx.nm, ctx.nm.graph
        x, W1, xl1, h, W2, xl2 = ctx.saved_tensors
        N, H = h.shape
        C = W2.shape[0]
        need_x, need_W1, need_b1, need_W2, need_b2, need_g = (ctx.needs_input_grad[i] for i in range(6))
        need_b1, need_b2, need_g = need_b1 and ctx.has_b1, need_b2 and ctx.has_b2, need_g and ctx.has_handle
        dx = dW1 = db1 = dW2 = db2 = g = None
        dZ2 = dout.contiguous()
        f32 = dict(dtype=torch.float32, device=dZ2.device)

        def sddmm(dZ, xl, D):
            gg = torch.empty(gr.n_edges + gr.N, **f32)
            _lib.check(L.sgs_sddmm_csr(_ptr(dZ), _ptr(xl), N, D, gr.n_edges, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid),
                                       gg[:gr.n_edges].data_ptr(), gg[gr.n_edges:].data_ptr(), _stream()), "sgs_sddmm_csr")
            return gg

        # ---- layer 2 (no activation): dxl2 = A_hat^T dZ2, dZ1 = (dxl2 W2) * act'(h), d b2 = colsum(dZ2)
        want_1 = need_x or need_W1 or need_b1 or need_g
        dxl2 = dZ1 = None
        if want_1 or need_W2:
            dxl2 = torch.empty(N, C, **f32)
            if ctx.fused:
                dZ1 = torch.empty(N, H, **f32) if want_1 else None
                db2 = torch.empty(C, **f32) if need_b2 else None
                _lib.check(L.sgs_spmm_csr_bwd_prev(_ptr(dZ2), N, C, gr.n_edges, _ptr(gr.out_ptr), _ptr(gr.out_dst), _ptr(nm.what_out),
                                                   _ptr(nm.what_loop), _ptr(W2 if want_1 else None, torch.float32), H, _ptr(h), ctx.act,
                                                   float(ctx.p), _ptr(dxl2), _ptr(dZ1), _ptr(db2), _stream()), "sgs_spmm_csr_bwd_prev")
            else:
                dxl2 = _spmm(dZ2, gr.out_ptr, gr.out_dst, nm.what_out, nm.what_loop, None, ACT_NONE, 0.0, 0, 0, N, C, gr.n_edges)
        if need_W2:
            dW2 = _dyt_x(dxl2, h, W2.shape, leaf=(ctx, 3))
        if want_1 and not ctx.fused:
            dZ1h = dxl2 @ W2         # (not _grad_through_act: this product always goes through the activation kernel, ACT_NONE included)
            dZ1, db1 = _act_bwd_colsum(dZ1h, h, ctx.act, ctx.p) if need_b1 else (_act_bwd(dZ1h, h, ctx.act, ctx.p), None)
        g2 = sddmm(dZ2, xl2, C) if need_g else None
        if need_b2 and db2 is None:
            db2 = _colsum(dZ2)
        # ---- layer 1: dxl1 = A_hat^T dZ1 (+ d b1 = colsum(dZ1) in the same launch when fused)
        if need_x or need_W1 or (need_b1 and db1 is None and ctx.fused):
            if ctx.fused:
                dxl1 = torch.empty(N, H, **f32)
                db1 = torch.empty(H, **f32) if need_b1 else None
                _lib.check(L.sgs_spmm_csr_bwd_prev(_ptr(dZ1), N, H, gr.n_edges, _ptr(gr.out_ptr), _ptr(gr.out_dst), _ptr(nm.what_out),
                                                   _ptr(nm.what_loop), None, 0, None, ACT_NONE, 0.0, _ptr(dxl1), None, _ptr(db1), _stream()),
                           "sgs_spmm_csr_bwd_prev")
            else:
                dxl1 = _spmm(dZ1, gr.out_ptr, gr.out_dst, nm.what_out, nm.what_loop, None, ACT_NONE, 0.0, 0, 0, N, H, gr.n_edges)
            if need_W1:
                dW1 = _dyt_x(dxl1, x, W1.shape, leaf=(ctx, 1))
            if need_x:
                dx = dxl1 @ W1
        g1 = sddmm(dZ1, xl1, H) if need_g else None
        if need_b1 and db1 is None:
            db1 = _colsum(dZ1)
        if need_g:          # the two layers' gradients wrt the shared normalisation, in _handle_grad's contract (layer 2 reports first)
            r2, r1 = _handle_grad(nm, g2), _handle_grad(nm, g1)
            g = r2 if r1 is None else (r1 if r2 is None else r2 + r1)
        return dx, dW1, db1, dW2, db2, g, None, None, None, None, None, None, None


def gcn2(x, W1, b1, W2, b2, nm: Norm, act=ACT_RELU, p=0.0, seed=0, site=0, xl1=None):
    """Two GCN layers, A_hat (act(A_hat (x W1^T) + b1) W2^T) + b2, with autograd to x, W1, b1, W2, b2 and (through nm.handle) the
    edge weights.  Returns (out, xl1) where xl1 = x W1^T (detached) can be passed back in for another graph over the same x, W1."""
    _need_gpu(x, W1, b1, W2, b2)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != nm.graph.N:
        raise RuntimeError("gcn2: x must be float32 [N, F]")
    return _GCN2.apply(x, W1, b1, W2, b2, nm.handle, nm, act, float(p), int(seed), int(site), xl1)


# ------------------------------------------------------------------ the GNN head over two graphs: both forwards in two launches
_gcn_dual_enabled = True                         # False: gcn2_dual is two plain gcn2 calls (A/B switch: set_gcn_dual)
GCN_DUAL_FORWARDS = {"shared": 0}                # forwards that ran as the two two-job launches (tests)


def set_gcn_dual(on: bool) -> None:
    """A/B switch (tests, tools): with False gcn2_dual makes two gcn2 calls and the sampled step its two separate GNN forwards."""
    global _gcn_dual_enabled
    _gcn_dual_enabled = bool(on)


def gcn_dual_enabled() -> bool:
    return _gcn_dual_enabled


def gcn_dual_ok(gr_a, gr_b, H: int, C: int) -> bool:
    """sgs_gcn_dual_ok: the two graphs' forwards can share their launches (both on the row-block path, one kernel variant)."""
    return (gr_a.N == gr_b.N and bool(_lib.lib().sgs_gcn_dual_ok(gr_a.N, gr_a.n_edges, gr_b.n_edges, int(H), int(C)))
            and _pair_ok(gr_a, H, C) and _pair_ok(gr_b, H, C))          # (as _GCN2 decides `fused`: its backward keeps rows of width C in LDS)


def _gcn2_dual_forward(xl1, b1, W2, b2, nm_a, nm_b, act, p, seed_a, seed_b, site):
    """Both graphs' two layers in two launches (sgs_spmm_csr_next_dual, sgs_spmm_csr_dual): ((h, xl2, out) of a, the same of b), each
    bitwise what _GCN2's fused forward computes for that graph alone."""
    L = _lib.lib()
    GCN_DUAL_FORWARDS["shared"] += 1
    ga, gb = nm_a.graph, nm_b.graph
    N, H = xl1.shape
    C = W2.shape[0]
    f32 = dict(dtype=torch.float32, device=xl1.device)
    h_a, xl2_a, out_a = torch.empty(N, H, **f32), torch.empty(N, C, **f32), torch.empty(N, C, **f32)
    h_b, xl2_b, out_b = torch.empty(N, H, **f32), torch.empty(N, C, **f32), torch.empty(N, C, **f32)
    _lib.check(L.sgs_spmm_csr_next_dual(_ptr(xl1, torch.float32), N, H, _ptr(b1), act, float(p), site, _ptr(W2, torch.float32), C,
                                        ga.n_edges, _ptr(ga.in_ptr), _ptr(ga.in_src), _ptr(nm_a.what_in), _ptr(nm_a.what_loop), seed_a,
                                        _ptr(h_a), _ptr(xl2_a),
                                        gb.n_edges, _ptr(gb.in_ptr), _ptr(gb.in_src), _ptr(nm_b.what_in), _ptr(nm_b.what_loop), seed_b,
                                        _ptr(h_b), _ptr(xl2_b), _stream()), "sgs_spmm_csr_next_dual")
    _lib.check(L.sgs_spmm_csr_dual(_ptr(xl2_a), _ptr(xl2_b), N, C, _ptr(b2), ACT_NONE, 0.0, 0,
                                   ga.n_edges, _ptr(ga.in_ptr), _ptr(ga.in_src), _ptr(nm_a.what_in), _ptr(nm_a.what_loop), 0, _ptr(out_a),
                                   gb.n_edges, _ptr(gb.in_ptr), _ptr(gb.in_src), _ptr(nm_b.what_in), _ptr(nm_b.what_loop), 0, _ptr(out_b),
                                   _stream()), "sgs_spmm_csr_dual")
    return (h_a, xl2_a, out_a), (h_b, xl2_b, out_b)


def gcn2_dual(x, W1, b1, W2, b2, nm_a: Norm, nm_b: Norm, act=ACT_RELU, p=0.0, seed_a=0, seed_b=0, site=0, xl1=None):
    """gcn2 over two graphs of the same nodes, (out_a, out_b, xl1): out_a = gcn2(..., nm_a, seed_a), out_b = gcn2(..., nm_b, seed_b), bitwise,
    with the same autograd (to x, W1, b1, W2, b2 from both and, through nm_a.handle, to branch a's edge weights; nm_b carries no handle).
    Where the two forwards can share their launches (gcn_dual_ok, contiguous operands, the switch on) they run as two launches instead of
    four and each branch gets _GCN2's node over its precomputed forward; elsewhere these ARE the two gcn2 calls.
    Two nodes, not one: a node holding both branches would have nm_a.handle among its inputs, and a backward from out_b alone would then
    run everything behind the handle (the normalisation's and the scorer's backward) on zero-filled gradients -- the two-node graph leaves
    those parameters' .grad None, which the optimisers rely on."""
    _need_gpu(x, W1, b1, W2, b2)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != nm_a.graph.N or x.shape[0] != nm_b.graph.N:
        raise RuntimeError("gcn2_dual: x must be float32 [N, F] over both graphs' N nodes")
    if nm_b.handle is not None:
        raise RuntimeError("gcn2_dual: branch b takes no edge-weight gradient (nm_b.handle must be None)")
    H, C = W1.shape[0], W2.shape[0]
    pre_a = pre_b = None
    if (_gcn_dual_enabled and gcn_dual_ok(nm_a.graph, nm_b.graph, H, C) and W2.is_contiguous() and W2.shape[1] == H
            and (xl1 is None or xl1.is_contiguous())):
        with torch.no_grad():
            if xl1 is None:
                xl1 = _x_wt(x, W1).contiguous()
            pre_a, pre_b = _gcn2_dual_forward(xl1, b1, W2, b2, nm_a, nm_b, act, float(p), int(seed_a), int(seed_b), int(site))
    out_a, xl1 = _GCN2.apply(x, W1, b1, W2, b2, nm_a.handle, nm_a, act, float(p), int(seed_a), int(site), xl1, pre_a)
    out_b, xl1 = _GCN2.apply(x, W1, b1, W2, b2, None, nm_b, act, float(p), int(seed_b), int(site), xl1, pre_b)
    return out_a, out_b, xl1


# ------------------------------------------------------------------ batched ensemble evaluation (forward only; composed in eval_batch.py)
def _empty_f32(*shape, device):
    """An uninitialised float32 buffer that a kernel fills, for callers outside this module: allocated here, through this module's
    `torch`, so that the SGS_POISON test hook (tests/conftest.py patches ops.torch) poisons it like every other such buffer."""
    return torch.empty(*shape, dtype=torch.float32, device=device)


class MultiSampleResult:
    """D draws over one candidate set (sgs_sample_topq_multi): mask [D, E] bool, eid [D, q], edge_index [D, 2, q] or None,
    stats [D, 4], w [D, q] (straight-through weights) or None.  Row d is what sample_topq returns for stream id stream_id0 + d.
    cover_info: [D, 2] int32 = {M_d, min(M_d, q)} for node-covering draws (sgs_sample_topq_multi_cover), else None."""
    __slots__ = ("mask", "eid", "edge_index", "stats", "w", "D", "E", "q", "cover_info")


def sample_topq_multi(mode: int, p, prior, c: float, q: int, edge_index, D: int, noise=None, seed: int = 0, stream_id0: int = 0,
                      want_edge_index: bool = True, want_w: bool = False, cover: "Graph | None" = None) -> MultiSampleResult:
    """D exponential-race top-q draws in one pass.  p [E] f32 (None: uniform weights), prior [E] or None, noise [D, E] f32 or None
    (then draw d uses (seed, stream_id0 + d)).  `want_w`: also the straight-through weights of each draw (mode LEARNED).
    `cover`: the Graph of the candidate edges (get_graph(edge_index, N)) makes every draw node-covering (sgs_sample_topq_multi_cover:
    row d is sample_topq(..., cover=)'s draw for stream id stream_id0 + d); the result then carries cover_info int32 [D, 2]."""
    L = _lib.lib()
    _need_gpu(p, prior, edge_index, noise)
    if p is None and edge_index is None:
        raise RuntimeError("sample_topq_multi: uniform weights (p=None) need edge_index for the number of candidates")
    E = p.numel() if p is not None else edge_index.shape[1]
    dev = p.device if p is not None else edge_index.device
    D = int(D)
    if noise is not None and (noise.dim() != 2 or tuple(noise.shape) != (D, E)):
        raise RuntimeError(f"sample_topq_multi: noise must be [D={D}, E={E}]")
    r = MultiSampleResult()
    r.D, r.E, r.q = D, E, q
    r.mask = torch.empty(max(D, 1), E, dtype=torch.bool, device=dev)
    r.eid = torch.empty(max(D, 1), q, dtype=torch.int64, device=dev)
    r.edge_index = torch.empty(max(D, 1), 2, q, dtype=torch.int64, device=dev) if (want_edge_index and edge_index is not None) else None
    r.stats = torch.empty(max(D, 1), 4, dtype=torch.float32, device=dev)
    r.w = torch.empty(max(D, 1), q, dtype=torch.float32, device=dev) if want_w else None
    r.cover_info = None
    if cover is not None:
        if not isinstance(cover, Graph) or cover.n_edges != E:
            raise RuntimeError(f"sample_topq_multi: cover must be the Graph of the E={E} candidate edges"
                               + (f" (it has {cover.n_edges})" if isinstance(cover, Graph) else ""))
        r.cover_info = (torch.empty if E > 0 else torch.zeros)(max(D, 1), 2, dtype=torch.int32, device=dev)     # (E == 0: nothing is written)
        ws = workspace(L.sgs_sample_topq_multi_cover_workspace_bytes(E, cover.N, max(D, 1)), dev)
        _lib.check(L.sgs_sample_topq_multi_cover(mode, _ptr(p, torch.float32), _ptr(prior, torch.float32), float(c), _ptr(noise, torch.float32),
                                                 seed, stream_id0, D, E, q, _ptr(edge_index, torch.int64), cover.N, _ptr(cover.in_ptr),
                                                 _ptr(cover.in_src), _ptr(cover.in_eid), _ptr(r.mask), _ptr(r.eid), _ptr(r.edge_index),
                                                 _ptr(r.stats), _ptr(r.w), _ptr(r.cover_info), ws.data_ptr(), ws.numel(), _stream()),
                   "sgs_sample_topq_multi_cover")
        return r
    ws = workspace(L.sgs_sample_topq_multi_workspace_bytes(E, max(D, 1)), dev)
    _lib.check(L.sgs_sample_topq_multi(mode, _ptr(p, torch.float32), _ptr(prior, torch.float32), float(c), _ptr(noise, torch.float32), seed,
                                       stream_id0, D, E, q, _ptr(edge_index, torch.int64), _ptr(r.mask), _ptr(r.eid), _ptr(r.edge_index),
                                       _ptr(r.stats), _ptr(r.w), ws.data_ptr(), ws.numel(), _stream()), "sgs_sample_topq_multi")
    return r


# ------------------------------------------------------------------ consensus of D draws (the sparsifier export; composed in sparsify.py)
CONSENSUS_MAX_DRAWS = 127          # a keep count fills 7 bits of the selection key (sgs_consensus_select)


def consensus_accum(smp_or_mask, count=None, first: bool = True, hist=None) -> torch.Tensor:
    """sgs_consensus_accum: count[e] = (0 if first else count[e]) + #{d : mask[d, e] != 0}, int32 [E] on the device.  `smp_or_mask`: a
    MultiSampleResult (its D draws) or a bool / uint8 tensor [Dc, E] with unit column stride (rows may be strided and unaligned).  `count`
    None (only with first=True): a new buffer.  `hist` (int64 [128] or None) is accumulated into, never cleared: hist[count[e]] += 1 for
    every e after this pass.  At most 127 draws per call, and in total.  No host sync."""
    L = _lib.lib()
    if isinstance(smp_or_mask, MultiSampleResult):
        mask, Dc = smp_or_mask.mask, int(smp_or_mask.D)
    else:
        mask = smp_or_mask
        if not torch.is_tensor(mask) or mask.dim() != 2:
            raise RuntimeError("consensus_accum: mask must be a MultiSampleResult or a [Dc, E] tensor")
        Dc = mask.shape[0]
    _need_gpu(mask, count, hist)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"consensus_accum: mask must be a bool or uint8 tensor, got {mask.dtype}")
    E = mask.shape[1]
    if E > 1 and mask.stride(1) != 1:
        raise RuntimeError("consensus_accum: mask must have unit column stride")
    stride = mask.stride(0) if mask.shape[0] > 1 else E
    if Dc > 1 and stride < E:
        raise RuntimeError("consensus_accum: mask rows overlap")
    if count is None:
        if not first:
            raise RuntimeError("consensus_accum: count is required when first=False")
        count = torch.empty(E, dtype=torch.int32, device=mask.device)
    elif count.dtype != torch.int32 or count.dim() != 1 or count.numel() != E or not count.is_contiguous():
        raise RuntimeError(f"consensus_accum: count must be a contiguous int32 [{E}] tensor")
    if hist is not None and (hist.dtype != torch.int64 or hist.dim() != 1 or hist.numel() != 128 or not hist.is_contiguous()):
        raise RuntimeError("consensus_accum: hist must be a contiguous int64 [128] tensor")
    _lib.check(L.sgs_consensus_accum(mask.data_ptr() if Dc > 0 and E > 0 else None, stride, Dc, E, 1 if first else 0, _ptr(count),
                                     _ptr(hist), _stream()), "sgs_consensus_accum")
    return count


class ConsensusResult:
    """sgs_consensus_select's outputs: mask [E] bool, eid [q] (ascending), edge_index [2, q] or None, count [q] int32, p [q] float32
    (ones when no scores were given), keys [E] (int64 holding the uint32 keys; only with want_keys), E, q."""
    __slots__ = ("mask", "eid", "edge_index", "count", "p", "keys", "E", "q")


def consensus_select(count, p, q: int, edge_index, want_keys: bool = False) -> ConsensusResult:
    """The q edges with the largest (count, score) keys, ties to the lowest edge id, in original edge order (sgs_consensus_select).
    count int32 [E] in [0, 127]; p float32 [E] or None (the count alone); edge_index int64 [2, E] or None.  Scores that differ only in
    their 6 lowest mantissa bits tie.  q > E raises.  No host sync."""
    L = _lib.lib()
    _need_gpu(count, p, edge_index)
    if count.dtype != torch.int32 or count.dim() != 1 or not count.is_contiguous():
        raise RuntimeError("consensus_select: count must be a contiguous int32 [E] tensor")
    E, q = count.numel(), int(q)
    if p is not None and (p.dtype != torch.float32 or p.dim() != 1 or p.numel() != E or not p.is_contiguous()):
        raise RuntimeError(f"consensus_select: p must be a contiguous float32 [{E}] tensor")
    if edge_index is not None and (edge_index.dtype != torch.int64 or tuple(edge_index.shape) != (2, E) or not edge_index.is_contiguous()):
        raise RuntimeError(f"consensus_select: edge_index must be a contiguous int64 [2, {E}] tensor")
    if q < 0:
        raise RuntimeError(f"consensus_select: q={q} is negative")
    dev = count.device
    r = ConsensusResult()
    r.E, r.q = E, q
    n = min(q, E)                                 # (q > E: the library refuses below; nothing of size q is allocated first)
    r.mask = torch.empty(E, dtype=torch.bool, device=dev)
    r.eid = torch.empty(n, dtype=torch.int64, device=dev)
    r.edge_index = torch.empty(2, n, dtype=torch.int64, device=dev) if edge_index is not None else None
    r.count = torch.empty(n, dtype=torch.int32, device=dev)
    r.p = torch.empty(n, dtype=torch.float32, device=dev)
    keys = torch.empty(E, dtype=torch.int32, device=dev) if want_keys else None
    ws = workspace(L.sgs_consensus_select_workspace_bytes(E), dev)
    _lib.check(L.sgs_consensus_select(_ptr(count), _ptr(p), E, q, _ptr(edge_index), _ptr(r.mask), _ptr(r.eid), _ptr(r.edge_index),
                                      _ptr(r.count), _ptr(r.p), _ptr(keys), ws.data_ptr(), ws.numel(), _stream()), "sgs_consensus_select")
    r.keys = (keys.to(torch.int64) & 0xFFFFFFFF) if want_keys else None
    return r


def edge_class_counts(edge_index, y, N: int, C: int, mask=None, out=None) -> torch.Tensor:
    """int64 [C, C] on device: out[y[src_e]][y[dst_e]] += 1 for every edge e (with mask[e] set, when a mask is given)
    (sgs_edge_class_counts).  `out` is accumulated into when given, else a zeroed buffer is made.  Edges with an endpoint outside [0, N) or
    a label outside [0, C) are skipped.  No host sync."""
    L = _lib.lib()
    _need_gpu(edge_index, y, mask, out)
    N, C = int(N), int(C)
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise RuntimeError("edge_class_counts: edge_index must be an int64 [2, n] tensor")
    if y.dtype != torch.int64 or y.dim() != 1 or y.numel() != N:
        raise RuntimeError(f"edge_class_counts: y must be an int64 [{N}] tensor")
    if C < 1:
        raise RuntimeError(f"edge_class_counts: C={C} classes")
    n = edge_index.shape[1]
    if mask is not None:
        mask = _u8(mask)
        if mask.numel() != n:
            raise RuntimeError("edge_class_counts: mask needs one entry per edge")
    if out is None:
        out = torch.zeros(C, C, dtype=torch.int64, device=edge_index.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (C, C) or not out.is_contiguous():
        raise RuntimeError(f"edge_class_counts: out must be a contiguous int64 [{C}, {C}] tensor")
    _lib.check(L.sgs_edge_class_counts(_ptr(edge_index.contiguous()), n, _ptr(mask), _ptr(y.contiguous()), N, C, _ptr(out), _stream()),
               "sgs_edge_class_counts")
    return out


def edge_class_variant(n: int, C: int) -> int:
    """sgs_edge_class_variant: the form an edge_class_counts call launches now: 2 privatised, 1 direct, 0 nothing (n = 0), -1 refused.  Host-only."""
    return int(_lib.lib().sgs_edge_class_variant(int(n), int(C)))


def edge_class_variant_set(code: int) -> None:
    """sgs_edge_class_variant_set: 0 = automatic (default), 1 = direct, 2 = privatised; any other code raises."""
    _lib.check(_lib.lib().sgs_edge_class_variant_set(int(code)), "sgs_edge_class_variant_set")


def graph_filter_multi(parent: Graph, smp: MultiSampleResult):
    """In-CSRs of the D drawn subgraphs of `parent` (sgs_graph_filter_multi): (in_ptr [D, N+1], in_src [D, q], in_eid [D, q],
    loop_eid [D, N]) int32; row d equals sgs_graph_filter's arrays for draw d."""
    L = _lib.lib()
    D, q, N = smp.D, smp.q, parent.N
    dev = parent.edge_index.device
    i32 = dict(dtype=torch.int32, device=dev)
    in_ptr = torch.empty(D, N + 1, **i32)
    in_src = torch.empty(D, max(q, 1), **i32)
    in_eid = torch.empty(D, max(q, 1), **i32)
    loop = torch.empty(D, max(N, 1), **i32)
    ws = workspace(L.sgs_graph_filter_multi_workspace_bytes(parent.n_edges, N, D), dev)
    _lib.check(L.sgs_graph_filter_multi(_ptr(parent.in_ptr), _ptr(parent.in_src), _ptr(parent.in_eid), parent.n_edges, N, D, _ptr(_u8(smp.mask)),
                                        _ptr(smp.eid), q, _ptr(in_ptr), _ptr(in_src), _ptr(in_eid), _ptr(loop), ws.data_ptr(), ws.numel(),
                                        _stream()), "sgs_graph_filter_multi")
    return in_ptr, in_src, in_eid, loop


def gcn_norm_multi(csr, w, q: int, N: int):
    """sgs_gcn_norm_fwd_multi over graph_filter_multi's CSRs: (dis, loopw, what_in [D, q], what_loop) for w [D, q] or None (unit)."""
    L = _lib.lib()
    in_ptr, in_src, in_eid, loop = csr
    D = in_ptr.shape[0]
    f32 = dict(dtype=torch.float32, device=in_ptr.device)
    dis, loopw, what_loop = torch.empty(D, N, **f32), torch.empty(D, N, **f32), torch.empty(D, N, **f32)
    what_in = torch.empty(D, max(q, 1), **f32)
    _lib.check(L.sgs_gcn_norm_fwd_multi(_ptr(w, torch.float32), q, N, D, _ptr(in_ptr), _ptr(in_src), _ptr(in_eid), _ptr(loop), _ptr(dis),
                                        _ptr(loopw), _ptr(what_in), _ptr(what_loop), _stream()), "sgs_gcn_norm_fwd_multi")
    return dis, loopw, what_in, what_loop


def _spmm_multi(X, x_stride: int, csr, val, diag, bias, act, q: int, N: int, Dc: int):
    """sgs_spmm_csr_multi over graph_filter_multi's CSRs: Y [D, N, Dc], Y[d] = act(A_d X_d + bias) with X_d = X + d * x_stride."""
    L = _lib.lib()
    in_ptr, in_src = csr[0], csr[1]
    D = in_ptr.shape[0]
    Y = torch.empty(D, N, Dc, dtype=torch.float32, device=X.device)
    _lib.check(L.sgs_spmm_csr_multi(_ptr(X, torch.float32), int(x_stride), N, Dc, q, D, _ptr(in_ptr), _ptr(in_src), _ptr(val), _ptr(diag), _ptr(bias),
                                    act, _ptr(Y), _stream()), "sgs_spmm_csr_multi")
    return Y


def ensemble_mean_correct(logits, x_stride: int, Dc: int, acc, first: bool, last: bool, D_total: int, y, masks, counts) -> None:
    """sgs_ensemble_mean_correct: fold Dc logit blocks into the running sum `acc` [N, C]; on the last pass acc becomes the mean and the
    three (correct, total) counts are added to `counts` (int64 [6])."""
    L = _lib.lib()
    N, C = acc.shape
    m = [_u8(x) for x in masks]
    _lib.check(L.sgs_ensemble_mean_correct(_ptr(logits, torch.float32), int(x_stride), int(Dc), N, C, _ptr(acc, torch.float32), int(first), int(last),
                                           int(D_total), _ptr(y, torch.int64), _ptr(m[0]), _ptr(m[1]), _ptr(m[2]), _ptr(counts, torch.int64),
                                           _stream()), "sgs_ensemble_mean_correct")


def gat_alpha_multi(a_s, a_d, a_stride: int, csr, q: int, N: int, negative_slope: float, out=None):
    """sgs_gat_alpha_fwd_multi over graph_filter_multi's CSRs: (alpha_in [D, q], alpha_loop [D, N]), row d bitwise sgs_gat_alpha_fwd's (p = 0)
    for draw d.  Draw d's node scores are a_s / a_d + d * a_stride (0: one [N] pair shared by all draws; N: [D, N] blocks).  `out`: reuse
    an (alpha_in, alpha_loop) pair of these shapes."""
    L = _lib.lib()
    in_ptr, in_src = csr[0], csr[1]
    D = in_ptr.shape[0]
    f32 = dict(dtype=torch.float32, device=in_ptr.device)
    alpha_in, alpha_loop = out if out is not None else (torch.empty(D, max(q, 1), **f32), torch.empty(D, max(N, 1), **f32))
    _lib.check(L.sgs_gat_alpha_fwd_multi(_ptr(a_s, torch.float32), _ptr(a_d, torch.float32), int(a_stride), N, D, q, _ptr(in_ptr), _ptr(in_src),
                                         float(negative_slope), _ptr(alpha_in), _ptr(alpha_loop), _stream()), "sgs_gat_alpha_fwd_multi")
    return alpha_in, alpha_loop


def gine_aggregate_multi(x, x_stride: int, csr, w, a, b, diag: float, q: int, N: int, Dc: int):
    """sgs_gine_aggregate_fwd_multi over graph_filter_multi's CSRs: z [D, N, Dc], block d bitwise sgs_gine_aggregate_fwd's for draw d with
    x_d = x + d * x_stride (0: one [N, Dc] block shared by all draws; N Dc: [D, N, Dc] blocks).  `w` [D, q] by the draw's edge id
    (sample_topq_multi(..., want_w=True).w) or None (unit weights); a, b with Dc elements.  Forward only: no autograd node."""
    L = _lib.lib()
    _need_gpu(x, w, a, b)
    in_ptr, in_src, in_eid = csr[0], csr[1], csr[2]
    D = in_ptr.shape[0]
    x_stride = int(x_stride)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < (D - 1) * x_stride + N * Dc or (x_stride != 0 and x_stride < N * Dc):
        raise RuntimeError(f"gine_aggregate_multi: x must be contiguous float32 with (D - 1) x_stride + N Dc = {(D - 1) * x_stride + N * Dc} elements")
    if a.numel() != Dc or b.numel() != Dc or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError(f"gine_aggregate_multi: a and b must be float32 with {Dc} elements")
    if w is not None and (tuple(w.shape) != (D, q) or w.dtype != torch.float32):
        raise RuntimeError(f"gine_aggregate_multi: w must be float32 [D={D}, q={q}]")
    if tuple(in_ptr.shape) != (D, N + 1) or tuple(in_src.shape) != (D, max(q, 1)) or tuple(in_eid.shape) != (D, max(q, 1)):
        raise RuntimeError(f"gine_aggregate_multi: csr must be graph_filter_multi's arrays for D={D}, N={N}, q={q}")
    z = torch.empty(D, N, Dc, dtype=torch.float32, device=x.device)
    w = w.contiguous() if w is not None and q > 0 else None
    a, b = a.reshape(Dc).contiguous(), b.reshape(Dc).contiguous()
    _lib.check(L.sgs_gine_aggregate_fwd_multi(_ptr(x, torch.float32), x_stride, _ptr(w), _ptr(a), _ptr(b), float(diag), N, Dc, q, D, _ptr(in_ptr),
                                              _ptr(in_src), _ptr(in_eid), _ptr(z), _stream()), "sgs_gine_aggregate_fwd_multi")
    return z


def gat_alpha_heads_multi(a_s, a_d, a_stride: int, csr, q: int, N: int, K: int, negative_slope: float, edge_w=None, edge_coef=None, out=None):
    """sgs_gat_alpha_heads_fwd_multi over graph_filter_multi's CSRs: (alpha [D, q, K] by the draw's edge id, alpha_loop [D, N, K]), row d
    bitwise sgs_gat_alpha_heads_fwd's (p = 0) for draw d -- or, with `edge_w` [D, q] and `edge_coef` [K], sgs_gat_alpha_heads_edge_fwd's
    (every 1 <= K <= 16).  Draw d's node scores are a_s / a_d + d * a_stride (0: one [N, K] pair shared by all draws; N K: [D, N, K]
    blocks).  `out`: reuse an (alpha, alpha_loop) pair of these shapes."""
    L = _lib.lib()
    in_ptr, in_src, in_eid = csr[0], csr[1], csr[2]
    D = in_ptr.shape[0]
    if (edge_w is None) != (edge_coef is None):
        raise RuntimeError("gat_alpha_heads_multi: edge_w and edge_coef come together")
    if edge_w is not None and (tuple(edge_w.shape) != (D, q) or edge_coef.numel() != K):
        raise RuntimeError(f"gat_alpha_heads_multi: edge_w must be [D={D}, q={q}] and edge_coef [{K}]")
    f32 = dict(dtype=torch.float32, device=in_ptr.device)
    alpha, alpha_loop = out if out is not None else (torch.empty(D, max(q, 1), K, **f32), torch.empty(D, max(N, 1), K, **f32))
    _lib.check(L.sgs_gat_alpha_heads_fwd_multi(_ptr(a_s, torch.float32), _ptr(a_d, torch.float32), int(a_stride), _ptr(edge_w, torch.float32),
                                               _ptr(edge_coef, torch.float32), N, K, D, q, _ptr(in_ptr), _ptr(in_src), _ptr(in_eid),
                                               float(negative_slope), _ptr(alpha), _ptr(alpha_loop), _stream()), "sgs_gat_alpha_heads_fwd_multi")
    return alpha, alpha_loop


def _spmm_heads_multi(X, x_stride: int, csr, val, diag, mode, bias, act, q: int, N: int, K: int, C: int):
    """sgs_spmm_csr_heads_multi over graph_filter_multi's CSRs: Y [D, N, K C] (HEADS_CONCAT) or [D, N, C] (HEADS_MEAN), block d bitwise
    sgs_spmm_csr_heads' for draw d with X_d = X + d * x_stride."""
    L = _lib.lib()
    in_ptr, in_src, in_eid = csr[0], csr[1], csr[2]
    D = in_ptr.shape[0]
    Y = torch.empty(D, N, C if mode == HEADS_MEAN else K * C, dtype=torch.float32, device=X.device)
    _lib.check(L.sgs_spmm_csr_heads_multi(_ptr(X, torch.float32), int(x_stride), N, K, C, q, D, _ptr(in_ptr), _ptr(in_src), _ptr(in_eid), _ptr(val),
                                          _ptr(diag), mode, _ptr(bias), act, _ptr(Y), _stream()), "sgs_spmm_csr_heads_multi")
    return Y


def gatv2_alpha_heads_multi(xl, xr, x_stride: int, att, csr, q: int, N: int, K: int, negative_slope: float, edge_w=None, lin_edge=None, out=None):
    """sgs_gatv2_alpha_heads_fwd_multi over graph_filter_multi's CSRs: (alpha [D, max(q, 1), K] by the draw's edge id, alpha_loop
    [D, max(N, 1), K]), block d bitwise what sgs_gatv2_alpha_heads_fwd (p = 0) writes for draw d with xl_d / xr_d = xl / xr + d * x_stride
    (0: one [N, K C] pair shared by all draws; exactly N K C: dense [D, N, K C] blocks; nothing else: the kernel's vector width, and with
    it the bits, must be the single-draw call's for every block).  att with K C elements; `edge_w` [D, q] by the draw's edge id
    (sample_topq_multi(..., want_w=True).w) comes with `lin_edge` (lin_edge.weight, K C elements), both None = no edge term.  `out`: reuse
    an (alpha, alpha_loop) pair of these shapes.  Forward only (eval: no attention dropout): no autograd node."""
    L = _lib.lib()
    _need_gpu(xl, xr, att, edge_w, lin_edge)
    in_ptr, in_src, in_eid = csr[0], csr[1], csr[2]
    D = in_ptr.shape[0]
    K, x_stride = int(K), int(x_stride)
    if att.dtype != torch.float32 or att.numel() % K != 0 or att.numel() < K:
        raise RuntimeError(f"gatv2_alpha_heads_multi: att must be float32 with K C elements (K={K})")
    W = att.numel()
    C = W // K
    if x_stride not in (0, N * W):
        raise RuntimeError(f"gatv2_alpha_heads_multi: x_stride={x_stride}: need 0 (one shared pair) or N K C = {N * W} (dense per-draw blocks)")
    need = (D - 1) * x_stride + N * W
    for name, t in (("xl", xl), ("xr", xr)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != need:
            raise RuntimeError(f"gatv2_alpha_heads_multi: {name} must be contiguous float32 with (D - 1) x_stride + N K C = {need} elements")
    if edge_w is not None and lin_edge is None:
        raise RuntimeError("gatv2_alpha_heads_multi: edge_w needs lin_edge")
    if edge_w is not None and (tuple(edge_w.shape) != (D, q) or edge_w.dtype != torch.float32):
        raise RuntimeError(f"gatv2_alpha_heads_multi: edge_w must be float32 [D={D}, q={q}]")
    if edge_w is not None and (lin_edge.numel() != W or lin_edge.dtype != torch.float32):
        raise RuntimeError(f"gatv2_alpha_heads_multi: lin_edge must be float32 with {W} elements")
    if tuple(in_ptr.shape) != (D, N + 1) or tuple(in_src.shape) != (D, max(q, 1)) or tuple(in_eid.shape) != (D, max(q, 1)):
        raise RuntimeError(f"gatv2_alpha_heads_multi: csr must be graph_filter_multi's arrays for D={D}, N={N}, q={q}")
    f32 = dict(dtype=torch.float32, device=in_ptr.device)
    if out is not None:
        alpha, alpha_loop = out
        if tuple(alpha.shape) != (D, max(q, 1), K) or tuple(alpha_loop.shape) != (D, max(N, 1), K) or not alpha.is_contiguous() \
                or not alpha_loop.is_contiguous() or alpha.dtype != torch.float32 or alpha_loop.dtype != torch.float32:
            raise RuntimeError(f"gatv2_alpha_heads_multi: out must be contiguous float32 ([{D}, {max(q, 1)}, {K}], [{D}, {max(N, 1)}, {K}])")
    else:
        alpha, alpha_loop = torch.empty(D, max(q, 1), K, **f32), torch.empty(D, max(N, 1), K, **f32)
    edge = edge_w is not None and q > 0                               # without edges every loop carries weight 0: the term vanishes
    w = edge_w.contiguous() if edge else None
    le = lin_edge.reshape(W).contiguous() if edge else None
    _lib.check(L.sgs_gatv2_alpha_heads_fwd_multi(_ptr(xl), _ptr(xr), x_stride, _ptr(att.reshape(W).contiguous()), _ptr(w), _ptr(le), N, K, C, D, q,
                                                 _ptr(in_ptr), _ptr(in_src), _ptr(in_eid), float(negative_slope), _ptr(alpha), _ptr(alpha_loop),
                                                 _stream()), "sgs_gatv2_alpha_heads_fwd_multi")
    return alpha, alpha_loop


def cheb_norm_multi(parent: Graph, smp: MultiSampleResult, csr, w=None):
    """sgs_cheb_norm_fwd_multi: (dis [D, N], l_in [D, q]) of the D drawn subgraphs, row d bitwise sgs_cheb_norm_fwd's dis / l_in for draw d.
    `w` [D, q] by the draw's edge id, or None (unit weights).  The by-source degree walks the parent's out-CSR under each draw's mask."""
    L = _lib.lib()
    in_ptr, in_src, in_eid = csr[0], csr[1], csr[2]
    D, q, N, E = smp.D, smp.q, parent.N, parent.n_edges
    f32 = dict(dtype=torch.float32, device=in_ptr.device)
    dis, l_in = torch.empty(D, max(N, 1), **f32), torch.empty(D, max(q, 1), **f32)
    ws = workspace(L.sgs_cheb_norm_fwd_multi_workspace_bytes(E, D), in_ptr.device)
    _lib.check(L.sgs_cheb_norm_fwd_multi(_ptr(w, torch.float32), _ptr(smp.eid, torch.int64), _ptr(_u8(smp.mask)), q, N, E, D, _ptr(parent.out_ptr),
                                         _ptr(parent.out_dst), _ptr(parent.out_eid), _ptr(in_ptr), _ptr(in_src), _ptr(in_eid), _ptr(dis),
                                         _ptr(l_in), ws.data_ptr(), ws.numel(), _stream()), "sgs_cheb_norm_fwd_multi")
    return dis, l_in


def _cheb_step_multi(K, X, ldx, xs, N, W, q, D, csr, val, alpha, add, ldadd, adds, sub, ldsub, subs, bias, act, Y, ldy, ys):
    """One sgs_cheb_spmm_multi launch; X, add, sub, Y are raw addresses (column blocks of wider buffers) or None, each with its leading
    dimension and draw stride."""
    _lib.check(_lib.lib().sgs_cheb_spmm_multi(K, X, ldx, xs, N, W, q, D, _ptr(csr[0]), _ptr(csr[1]), _ptr(val), float(alpha), add, ldadd, adds,
                                              sub, ldsub, subs, _ptr(bias), act, Y, ldy, ys, _stream()), "sgs_cheb_spmm_multi")


# ------------------------------------------------------------------ Chebyshev head, K > 1 (csrc/cheb.hip)
def cheb_supported(K: int) -> bool:
    """Whether the fused Chebyshev kernels serve order K (sgs_cheb_supported: 1 <= K <= 8; host-only)."""
    return bool(_lib.lib().sgs_cheb_supported(int(K)))


def _cheb_norm_forward(graph: Graph, w):
    L = _lib.lib()
    dev = graph.edge_index.device
    nm = Norm()
    nm.graph, nm.w = graph, w
    ne, Nn = max(graph.n_edges, 1), max(graph.N, 1)
    sizes = [Nn, ne, ne]
    offs = [0]
    for z in sizes:
        offs.append(offs[-1] + ((z + 63) & ~63))
    buf = torch.empty(offs[-1], dtype=torch.float32, device=dev)
    nm.dis, nm.what_in, nm.what_out = (buf[offs[i]:offs[i] + sizes[i]] for i in range(3))
    _lib.check(L.sgs_cheb_norm_fwd(_ptr(w, torch.float32), graph.n_edges, graph.N, _ptr(graph.in_ptr), _ptr(graph.in_src), _ptr(graph.in_eid),
                                   _ptr(graph.out_ptr), _ptr(graph.out_dst), _ptr(graph.out_eid), _ptr(nm.dis), _ptr(nm.what_in),
                                   _ptr(nm.what_out), _stream()), "sgs_cheb_norm_fwd")
    return nm


class _ChebNorm(torch.autograd.Function):
    """The autograd edge from the layers' gradients wrt l ([n_edges], edge-id order) back to the edge weights."""

    @staticmethod
    def forward(ctx, w, graph, box):
        nm = _cheb_norm_forward(graph, w)
        box.append(nm)
        ctx.nm = nm
        return torch.empty(graph.n_edges, dtype=torch.float32, device=w.device)

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        nm, gr = ctx.nm, ctx.nm.graph
        g = g.contiguous()
        n = gr.n_edges
        extra, _, _ = _take_parked(nm)                 # the other layer's gradient (_handle_grad): summed on read
        if extra is not None and extra.numel() != g.numel():
            g, extra = g + extra, None
        dw = torch.empty(n, dtype=torch.float32, device=g.device)
        if n > 0:
            ws = workspace(L.sgs_cheb_norm_bwd_workspace_bytes(gr.N), g.device)
            _lib.check(L.sgs_cheb_norm_bwd(_ptr(nm.w), _ptr(g), _ptr(extra), n, gr.N, _ptr(nm.dis), _ptr(gr.in_ptr), _ptr(gr.in_src),
                                           _ptr(gr.in_eid), _ptr(gr.out_ptr), _ptr(gr.out_dst), _ptr(gr.out_eid), _ptr(gr.edge_index), _ptr(dw),
                                           ws.data_ptr(), ws.numel(), _stream()), "sgs_cheb_norm_bwd")
        return dw, None, None


def cheb_norm(graph: Graph, w=None) -> Norm:
    """The scaled-Laplacian analogue of gcn_norm (PyG ChebConv, 'sym', lambda_max = 2): dis = deg^-1/2 with the degree summed by SOURCE
    and (i, i) edges removed, and l_e = -dis[s] w_e dis[d] in both CSR orders (`what_in` / `what_out`; there is no loop term, so `loopw` /
    `what_loop` are None).  `handle` carries the layers' gradients wrt l ([n_edges], edge-id order) back to `w`.  The unit-weight result
    depends on the graph alone and is kept on it -- except on a step-graph slot's graph (`restaged`), whose arrays are refilled per
    partition: there the kernels run on every call, so that they are part of every replay.  One normalisation per forward is meant to
    be shared by both layers of the head: the second layer's gradient is then summed on read (_handle_grad) instead of by an autograd
    add."""
    if w is None:
        if getattr(graph, "restaged", False):      # a step-graph slot's CSR is refilled per partition: the kernels belong in every replay
            return _cheb_norm_forward(graph, None)
        nm = getattr(graph, "_cheb_norm_unit", None)
        if nm is None:
            nm = graph._cheb_norm_unit = _cheb_norm_forward(graph, None)
        return nm
    _need_gpu(w)
    w = w.contiguous()
    if w.dtype != torch.float32 or w.numel() != graph.n_edges:
        raise RuntimeError(f"edge_weight must be float32 [{graph.n_edges}]")
    if not (w.requires_grad and torch.is_grad_enabled()):
        return _cheb_norm_forward(graph, w.detach())
    box = []
    handle = _ChebNorm.apply(w, graph, box)
    nm = box[0]
    nm.handle = handle
    nm._park_ok = True            # _ChebNorm.backward reads the parked second gradient
    return nm


def _cheb_step(K, X, ldx, N, D, gr_ptr, gr_col, val, nnz, alpha, add, ldadd, sub, ldsub, bias, act, p, seed, site, Y, ldy, Y2=None, ldy2=0,
               scale2=1.0):
    """One sgs_cheb_spmm launch; X, add, sub, Y, Y2 are raw addresses (column blocks of wider buffers) or None."""
    _lib.check(_lib.lib().sgs_cheb_spmm(K, X, ldx, N, D, nnz, _ptr(gr_ptr), _ptr(gr_col), _ptr(val), float(alpha), add, ldadd, sub, ldsub,
                                        _ptr(bias), act, float(p), seed, site, Y, ldy, Y2, ldy2, float(scale2), _stream()), "sgs_cheb_spmm")


class _ChebConv(torch.autograd.Function):
    """out = act(sum_k T_k(L_hat) x W_k^T + bias) by Clenshaw's recurrence at the output width:
        Y = x [W_0 | ... | W_{K-1}]^T,   b_k = Y_k + 2 L_hat b_{k+1} - b_{k+2} (k = K-1 .. 1),   out = act(Y_0 + L_hat b_1 - b_2 + bias)
    K - 1 fused steps (sgs_cheb_spmm) over the dst-CSR.  Kept for the backward: [b_1 | ... | b_{K-1}] (the steps overwrite the GEMM's
    column blocks in place) and, for the activation's derivative, the output.  Backward, with G = d out after the activation:
        U_0 = G, U_1 = L_hat^T G, U_k = 2 L_hat^T U_{k-1} - U_{k-2}  (K - 1 steps over the src-CSR)
        dW = [U_0 | ... | U_{K-1}]^T x,   dx = [U_0 | ... | U_{K-1}] Wcat,   dl = one SDDMM of [G | 2 U_1 | ... | 2 U_{K-2}] with [b_1 | ... | b_{K-1}]
    and nothing is recomputed."""

    @staticmethod
    def forward(ctx, x, Wcat, bias, handle, nm, K, act, p, seed, site):
        gr = nm.graph
        N = x.shape[0]
        D = Wcat.shape[0] // K
        ldb = (K - 1) * D
        Y0 = _x_wt(x, Wcat[:D])                                  # [N, D]
        B = _x_wt(x, Wcat[D:])                                   # [N, (K - 1) D]: Y_1 .. Y_{K-1}, becoming b_1 .. b_{K-1} in place
        b0 = B.data_ptr()
        blk = lambda k: b0 + 4 * (k - 1) * D                     # b_k's column block
        for k in range(K - 2, 0, -1):
            _cheb_step(K, blk(k + 1), ldb, N, D, gr.in_ptr, gr.in_src, nm.what_in, gr.n_edges, 2.0, blk(k), ldb,
                       blk(k + 2) if k + 2 <= K - 1 else None, ldb, None, ACT_NONE, 0.0, 0, 0, blk(k), ldb)
        out = torch.empty(N, D, dtype=torch.float32, device=x.device)
        _cheb_step(K, blk(1), ldb, N, D, gr.in_ptr, gr.in_src, nm.what_in, gr.n_edges, 1.0, Y0.data_ptr(), D, blk(2) if K >= 3 else None, ldb,
                   bias, act, p, seed, site, out.data_ptr(), D)
        ctx.nm, ctx.K, ctx.act, ctx.p = nm, K, act, p
        ctx.has_bias, ctx.has_handle = bias is not None, handle is not None
        ctx.save_for_backward(x, Wcat, B, out if act != ACT_NONE else None)
        return out

    @staticmethod
    def backward(ctx, dY):
        L = _lib.lib()
        nm, gr, K = ctx.nm, ctx.nm.graph, ctx.K
        x, Wcat, B, out = ctx.saved_tensors
        N, D = dY.shape
        dY = dY.contiguous()
        dx = dW = g = None
        G, dbias = _grad_through_act(dY, out, ctx.act, ctx.p, ctx.has_bias and ctx.needs_input_grad[2])
        need_x, need_W = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_h = ctx.has_handle and ctx.needs_input_grad[3]
        last = K - 1 if (need_x or need_W) else (K - 2 if need_h else 0)       # highest U_k anything asks for
        ldu, lda = K * D, (K - 1) * D
        U = torch.empty(N, ldu, dtype=torch.float32, device=dY.device)
        U[:, :D].copy_(G)
        A = G                                                    # the SDDMM's left operand [G | 2 U_1 | ... | 2 U_{K-2}]
        if need_h and K > 2:
            A = torch.empty(N, lda, dtype=torch.float32, device=dY.device)
            A[:, :D].copy_(G)
        u0, a0 = U.data_ptr(), A.data_ptr()
        for k in range(1, last + 1):
            y2 = a0 + 4 * k * D if (need_h and k <= K - 2) else None
            if k == 1:
                _cheb_step(K, G.data_ptr(), D, N, D, gr.out_ptr, gr.out_dst, nm.what_out, gr.n_edges, 1.0, None, 0, None, 0, None, ACT_NONE, 0.0,
                           0, 0, u0 + 4 * D, ldu, y2, lda, 2.0)
            else:
                _cheb_step(K, u0 + 4 * (k - 1) * D, ldu, N, D, gr.out_ptr, gr.out_dst, nm.what_out, gr.n_edges, 2.0, None, 0,
                           u0 + 4 * (k - 2) * D, ldu, None, ACT_NONE, 0.0, 0, 0, u0 + 4 * k * D, ldu, y2, lda, 2.0)
        if need_W:
            dW = _dyt_x(U, x, Wcat.shape)
        if need_x:
            dx = U @ Wcat
        if need_h:
            g = torch.empty(gr.n_edges, dtype=torch.float32, device=dY.device)
            _lib.check(L.sgs_sddmm_csr(_ptr(A), _ptr(B), N, lda, gr.n_edges, _ptr(gr.in_ptr), _ptr(gr.in_src), _ptr(gr.in_eid), _ptr(g), None,
                                       _stream()), "sgs_sddmm_csr")
        return dx, dW, dbias, (_handle_grad(nm, g) if g is not None else None), None, None, None, None, None, None


def cheb_conv(x, Wcat, bias, nm: Norm, K: int, act=ACT_NONE, p=0.0, seed=0, site=0):
    """One Chebyshev layer of order K >= 2 as one autograd node: act(sum_k T_k(L_hat) x W_k^T + bias), L_hat from `nm` (cheb_norm).
    `Wcat` [K out, in] holds W_0 .. W_{K-1} stacked by rows.  Gradients go to x, Wcat, bias and, through nm.handle, the edge weights.
    K = 1 is a plain Linear and has no graph step: ChebConv keeps that path."""
    _need_gpu(x, Wcat, bias)
    K = int(K)
    if K < 2:
        raise ValueError(f"cheb_conv: K = {K}: the fused recurrence starts at K = 2 (K = 1 is x W_0^T + bias, no graph step)")
    if not cheb_supported(K):
        raise ValueError(f"cheb_conv: K = {K} is not supported (1 <= K <= 8)")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != nm.graph.N:
        raise RuntimeError("cheb_conv: x must be float32 [N, F]")
    if Wcat.dim() != 2 or Wcat.shape[0] % K != 0 or Wcat.shape[1] != x.shape[1] or Wcat.dtype != torch.float32:
        raise RuntimeError(f"cheb_conv: Wcat must be float32 [K * out, {x.shape[1]}]")
    if nm.what_loop is not None or nm.dis is None:
        raise RuntimeError("cheb_conv: `nm` must come from cheb_norm")
    return _ChebConv.apply(x.contiguous(), Wcat.contiguous(), bias, nm.handle, nm, K, act, float(p), int(seed), int(site))


# ------------------------------------------------------------------ multi-partition batches (csrc/cluster.hip)
def cluster_collate_max_parts() -> int:
    return int(_lib.lib().sgs_cluster_collate_max_parts())


def _stage_spans(spans) -> int:
    """(src address, dst address, bytes) spans -> sgs_stage_segments, as few launches as its segment limit allows.  Returns the launches."""
    L = _lib.lib()
    spans = [s for s in spans if s[2] > 0]
    cap = int(L.sgs_stage_max_segments())
    for i in range(0, len(spans), cap):
        words = []
        for s, d, nb in spans[i:i + cap]:
            words += [s, d, nb, nb, 0]
        arr = (ctypes.c_int64 * len(words))(*words)
        _lib.check(L.sgs_stage_segments(arr, len(words) // 5, None, None, 0, _stream()), "sgs_stage_segments")
    return -(-len(spans) // cap)


def _edge_outputs(E_b: int, dev, want_prob: bool, want_eid: bool):
    """The edge outputs of a device collate, uninitialised: (edge_index [2, E_b], prob [E_b] or None, eid [E_b] or None)"""
    return (torch.empty(2, E_b, dtype=torch.int64, device=dev), torch.empty(E_b, dtype=torch.float32, device=dev) if want_prob else None,
            torch.empty(E_b, dtype=torch.int64, device=dev) if want_eid else None)


def _collated_batch(x, ei, y, masks, prob, node_ids, **extra):
    """The tail of a device collate: `prob` None (prior="local") -> the prior of the batch's own edge list; `masks` (uint8 [3, n], the
    kernels' output) handed over as the three bool masks; the caller's extra fields."""
    from .data import Batch, batch_prior
    if prob is None:
        prob = batch_prior(None, None, ei, x.shape[0])
    m = masks.view(torch.bool)
    return Batch(x=x, edge_index=ei, y=y, train_mask=m[0], val_mask=m[1], test_mask=m[2], prob=prob, node_ids=node_ids, **extra)


def cluster_collate(parts, group, want_eid: bool = False):
    """The batch of the partitions in `group` (a data.ResidentPartitions built with keep_cut_edges=True), cut edges between them
    restored: data.collate_torch's result, built by sgs_cluster_collate (count, scan, fill: edges, prior and masks) and one
    sgs_stage_segments launch per 24 spans (x, y, node ids).  The sizes come from the host tables, so nothing is read back --
    unless `parts.size_path == "readback"` (more partitions than the block table holds): then the edge count is one 8-byte
    read-back.  `want_eid`: also return, as `batch.eid`, each edge's position in `parts.full_col`."""
    from .data import _check_group, _intra_edges
    L = _lib.lib()
    _need_gpu(parts.full_ptr, parts.full_col, parts.x_all)
    group = _check_group(parts, group)
    k = len(group)
    if k > cluster_collate_max_parts():
        raise ValueError(f"cluster_collate: {k} partitions in one batch, the limit is {cluster_collate_max_parts()}")
    n_b, E_b = parts.batch_sizes(group)
    dev = parts.full_ptr.device
    nptr = parts.node_ptr_host
    ranges = (ctypes.c_int64 * (2 * k))(*[v for p in group for v in (nptr[p], nptr[p + 1])])
    nbytes = int(L.sgs_cluster_collate_workspace_bytes(n_b))
    ws = workspace(nbytes, dev)
    if E_b is None:
        total = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(L.sgs_cluster_collate_count(_ptr(parts.full_ptr, torch.int64), _ptr(parts.full_col, torch.int64), ranges, k, n_b,
                                               _ptr(total), ws.data_ptr(), ws.numel(), _stream()), "sgs_cluster_collate_count")
        E_b = int(total.item())
        if E_b >= 2 ** 31:
            raise ValueError(f"a batch of {E_b} edges does not fit the int32 graph kernels (limit 2^31)")
    x_all, y_all = parts.x_all, parts.y_all
    F = int(x_all.shape[1])
    if (F * x_all.element_size()) % 4 or y_all.element_size() % 4 or not x_all.is_contiguous() or not y_all.is_contiguous() or y_all.dim() != 1:
        raise RuntimeError("cluster_collate: x rows and y entries must be contiguous whole 4-byte words")
    ei, prob, eid = _edge_outputs(E_b, dev, parts.full_prob is not None, want_eid)
    masks = torch.empty(3, n_b, dtype=torch.uint8, device=dev)
    x = torch.empty(n_b, F, dtype=x_all.dtype, device=dev)
    y = torch.empty(n_b, dtype=y_all.dtype, device=dev)
    node_ids = torch.empty(n_b, dtype=torch.int64, device=dev)
    _lib.check(L.sgs_cluster_collate(_ptr(parts.full_ptr, torch.int64), _ptr(parts.full_col, torch.int64), _ptr(parts.full_prob), ranges, k,
                                     n_b, E_b, _ptr(ei), _ptr(prob), _ptr(eid), _ptr(parts.masks_all, torch.uint8), _ptr(masks), 3,
                                     parts.num_nodes, _ptr(parts.collate_mismatch, torch.int32), ws.data_ptr(), ws.numel(), _stream()),
               "sgs_cluster_collate")
    spans, at = [], 0
    xb, yb = F * x_all.element_size(), y_all.element_size()
    for p in group:
        a, n = nptr[p], nptr[p + 1] - nptr[p]
        spans += [(x_all.data_ptr() + a * xb, x.data_ptr() + at * xb, n * xb), (y_all.data_ptr() + a * yb, y.data_ptr() + at * yb, n * yb),
                  (parts.perm.data_ptr() + a * 8, node_ids.data_ptr() + at * 8, n * 8)]
        at += n
    _stage_spans(spans)
    b = _collated_batch(x, ei, y, masks, prob, node_ids, parts=group, restored_edges=E_b - _intra_edges(parts, group))
    if want_eid:
        b.eid = eid
    return b


# ------------------------------------------------------------------ device partitioner (csrc/partition.hip; partition.py)
LP_UNASSIGNED, LP_HASH = 0, 1          # sgs_lp_propose's eligibility rule


def _lp_csr(ptr, col, part, P):
    _need_gpu(ptr, col, part)
    N, P = part.numel(), int(P)
    if ptr.numel() != N + 1:
        raise RuntimeError("partitioner: ptr must hold N + 1 entries for part's N nodes")
    return N, col.numel(), P


def lp_propose(ptr, col, part, P: int, eligible: int, hash_key: int = 0, mingain: int = 0, best=None, gain=None):
    """(best, gain) int32 [N] of one sweep's proposals (sgs_lp_propose): per eligible node the neighbouring part with the most entries
    other than its own, and how many more entries that is; best = -1 where a node proposes nothing.  int32 CSR and part; one launch."""
    L = _lib.lib()
    N, nnz, P = _lp_csr(ptr, col, part, P)
    _need_gpu(best, gain)
    best = torch.empty(N, dtype=torch.int32, device=part.device) if best is None else best
    gain = torch.empty(N, dtype=torch.int32, device=part.device) if gain is None else gain
    if best.numel() != N or gain.numel() != N:
        raise RuntimeError("lp_propose: best and gain need one entry per node")
    _lib.check(L.sgs_lp_propose(_ptr(ptr, torch.int32), _ptr(col, torch.int32), N, nnz, P, _ptr(part, torch.int32), int(eligible),
                                int(hash_key) & 0xFFFFFFFF, int(mingain), _ptr(best, torch.int32), _ptr(gain, torch.int32), _stream()),
               "sgs_lp_propose")
    return best, gain


def lp_commit(best, gain, part, size, cap: int, lo: int, moved=None) -> torch.Tensor:
    """Accepts the reference's subset of one sweep's proposals (sgs_lp_commit) and moves those nodes: `part` [N] and `size` [P] (int32) are
    updated in place; returns `moved`, a device int32 [1] set to the number moved.  No host sync; not capturable (library sorts)."""
    L = _lib.lib()
    _need_gpu(best, gain, part, size, moved)
    N, P = part.numel(), size.numel()
    if best.numel() != N or gain.numel() != N:
        raise RuntimeError("lp_commit: best and gain need one entry per node")
    moved = torch.empty(1, dtype=torch.int32, device=part.device) if moved is None else moved
    nbytes = int(L.sgs_lp_commit_workspace_bytes(N, P))
    ws = workspace(nbytes, part.device)
    _lib.check(L.sgs_lp_commit(_ptr(best, torch.int32), _ptr(gain, torch.int32), N, P, int(cap), int(lo), _ptr(part, torch.int32),
                               _ptr(size, torch.int32), _ptr(moved, torch.int32), _ptr(ws), nbytes, _stream()), "sgs_lp_commit")
    return moved


def partition_stats(ptr, col, part, P: int):
    """(size int32 [P], cut int64 [1]) on device (sgs_partition_stats): the nodes of every part and the stored non-loop entries whose ends
    lie in different parts (every undirected edge twice).  One pass, no host sync."""
    L = _lib.lib()
    N, nnz, P = _lp_csr(ptr, col, part, P)
    size = torch.empty(max(P, 1), dtype=torch.int32, device=part.device)
    cut = torch.empty(1, dtype=torch.int64, device=part.device)
    _lib.check(L.sgs_partition_stats(_ptr(ptr, torch.int32), _ptr(col, torch.int32), N, nnz, P, _ptr(part, torch.int32), _ptr(size),
                                     _ptr(cut), _stream()), "sgs_partition_stats")
    return size, cut


# ------------------------------------------------------------------ neighbour-sampled batches (csrc/neighbor.hip; data.py: ResidentGraph)
NBR_WQ_MAX = (1 << 24) - 1                 # the largest quantised weight of the weighted fan-out draw


def nbr_select_hub_row() -> int:
    return int(_lib.lib().sgs_nbr_select_hub_row())


def nbr_max_hops() -> int:
    return int(_lib.lib().sgs_nbr_max_hops())


def nbr_state(N: int, device) -> torch.Tensor:
    """The three node bitmaps of a batch under construction (sgs_nbr_state_bytes), uninitialised: nbr_begin clears them."""
    return torch.empty(int(_lib.lib().sgs_nbr_state_bytes(int(N))), dtype=torch.uint8, device=device)


def nbr_quantize_weights(w) -> torch.Tensor:
    """int32 [E] quantised weights in [0, 2^24 - 1] for the weighted fan-out draw, on w's device, in float64: 0 where w == 0, else
    clamp(floor(w / max(w) (2^24 - 1) + 0.5), 1, 2^24 - 1).  Only the ratios of the weights inside one in-row matter to the draw; a positive
    weight below max(w) / 2^24 is rounded UP to that size (it stays drawable).  ValueError: a negative or non-finite weight, or no positive one."""
    w = torch.as_tensor(w).reshape(-1).to(torch.float64)
    if w.numel() == 0:
        return torch.zeros(0, dtype=torch.int32, device=w.device)
    if not bool(torch.isfinite(w).all()):
        raise ValueError("nbr_quantize_weights: a weight is not finite")
    if bool((w < 0).any()):
        raise ValueError("nbr_quantize_weights: a weight is negative")
    top = w.max()
    if not bool(top > 0):
        raise ValueError("nbr_quantize_weights: every weight is zero")
    q = torch.floor(w / top * float(NBR_WQ_MAX) + 0.5).clamp(1, NBR_WQ_MAX)
    return torch.where(w == 0, torch.zeros_like(q), q).to(torch.int32)


def nbr_select(in_ptr, in_eid, N: int, rows, fanout: int, key: int, total: int, wq=None):
    """int32 [total] chosen edge ids (sgs_nbr_select): per frontier row min(fanout, in-degree) of its in-edges, of a longer row the ones with
    the `fanout` smallest keys fmix32(id ^ key), in row order; rows back to back.  `total` is the caller's (nbr_frontier reports it for the
    next hop; for the seeds it follows from the in-degrees).  Two launches, no host sync.  `wq` (int32 [nnz] quantised weights aligned with
    in_eid, nbr_quantize_weights): the weighted draw of sgs_nbr_select_weighted instead, same launches."""
    L = _lib.lib()
    _need_gpu(in_ptr, in_eid, rows)
    n_rows = rows.numel()
    chosen = torch.empty(int(total), dtype=torch.int32, device=in_ptr.device)
    nbytes = int(L.sgs_nbr_select_workspace_bytes(n_rows))
    ws = workspace(nbytes, in_ptr.device)
    name, weights = "sgs_nbr_select", ()
    if wq is not None:
        _need_gpu(wq)
        if wq.numel() != in_eid.numel():
            raise ValueError(f"nbr_select: {wq.numel()} weights for {in_eid.numel()} in-CSR entries")
        name, weights = "sgs_nbr_select_weighted", (_ptr(wq, torch.int32),)
    _lib.check(getattr(L, name)(_ptr(in_ptr, torch.int32), _ptr(in_eid, torch.int32), *weights, int(N), in_eid.numel(), _ptr(rows, torch.int32),
                                n_rows, int(fanout), int(key) & 0xFFFFFFFF, _ptr(chosen), int(total), None, _ptr(ws), ws.numel(), _stream()), name)
    return chosen


def nbr_begin(seeds, N: int, state) -> None:
    """Clears `state` and marks the seeds (int32 node ids) as members and as seeds (sgs_nbr_begin)."""
    _need_gpu(seeds, state)
    _lib.check(_lib.lib().sgs_nbr_begin(_ptr(seeds, torch.int32), seeds.numel(), int(N), _ptr(state), state.numel(), _stream()), "sgs_nbr_begin")


def nbr_frontier(chosen, edge_index, N: int, in_ptr, next_fanout: int, state, cap: int):
    """(frontier int32 [cap], sizes int64 [2] on the device) of sgs_nbr_frontier: the sources of the chosen edges that are new to the batch,
    ascending, merged into the members; sizes = (their number, what the next nbr_select will emit for them under `next_fanout`; 0: no next hop)."""
    _need_gpu(chosen, edge_index, in_ptr, state)
    dev = chosen.device
    frontier = torch.empty(int(cap), dtype=torch.int32, device=dev)
    sizes = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().sgs_nbr_frontier(_ptr(chosen, torch.int32), chosen.numel(), _ptr(edge_index, torch.int64), edge_index.shape[1], int(N),
                                           _ptr(in_ptr, torch.int32), int(next_fanout), _ptr(state), state.numel(), _ptr(frontier), int(cap),
                                           _ptr(sizes), _stream()), "sgs_nbr_frontier")
    return frontier, sizes


def nbr_collate(graph, n: int, chosen, subgraph_type: str, n_seeds: int, hop_nodes):
    """The Batch of the members in `graph._nbr_state` (a data.ResidentGraph on a HIP device; `n` of them): node ids and word prefixes
    (sgs_nbr_nodes), the edges -- induced: count, scan, ONE 8-byte read-back of the edge count, fill; directional: `chosen` (the per-hop id
    tensors) sorted and gathered, no read-back -- and one gathering launch for x, y, the masks and the seed flags."""
    L = _lib.lib()
    st, N, E, dev = graph._nbr_state, graph.num_nodes, graph.num_edges, graph.edge_index.device
    sp, sb = _ptr(st), st.numel()
    wpre = torch.empty((N + 31) // 32, dtype=torch.int32, device=dev)
    node_ids = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(L.sgs_nbr_nodes(sp, sb, N, n, _ptr(wpre), _ptr(node_ids), _ptr(graph.collate_mismatch, torch.int32), _stream()), "sgs_nbr_nodes")
    want_prob = graph.prob is not None
    if subgraph_type == "induced":
        rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        csr = (_ptr(graph.out_ptr, torch.int32), _ptr(graph.out_dst, torch.int32), _ptr(graph.out_eid, torch.int32))
        _lib.check(L.sgs_nbr_induced_count(*csr, N, E, sp, sb, _ptr(wpre), _ptr(node_ids), n, _ptr(rowptr), _ptr(total), _stream()),
                   "sgs_nbr_induced_count")
        E_b = int(total.item())
        ei, prob, eid = _edge_outputs(E_b, dev, want_prob, True)
        _lib.check(L.sgs_nbr_induced_fill(*csr, _ptr(graph.prob), N, E, sp, sb, _ptr(wpre), _ptr(node_ids), n, _ptr(rowptr), E_b, _ptr(ei),
                                          _ptr(prob), _ptr(eid), _stream()), "sgs_nbr_induced_fill")
    else:
        segs = [(c.data_ptr(), c.numel()) for c in chosen if c.numel() > 0] or [(0, 0)]
        E_b = sum(c for _, c in segs)
        ei, prob, eid = _edge_outputs(E_b, dev, want_prob, True)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        table = (ctypes.c_int64 * (2 * len(segs)))(*[v for s in segs for v in s])
        nbytes = int(L.sgs_nbr_directional_workspace_bytes(E_b))
        ws = workspace(nbytes, dev)
        _lib.check(L.sgs_nbr_directional(table, len(segs), E_b, _ptr(graph.edge_index, torch.int64), E, N, _ptr(graph.prob), sp, sb, _ptr(wpre),
                                         _ptr(ei), _ptr(prob), _ptr(eid), _ptr(total), _ptr(ws), ws.numel(), _stream()), "sgs_nbr_directional")
    x_all, y_all = graph.x, graph.y
    row_bytes = int(x_all.shape[1]) * x_all.element_size()
    if row_bytes % 4 or y_all.dtype != torch.int64 or not x_all.is_contiguous() or y_all.dim() != 1:
        raise RuntimeError("nbr_collate: x rows must be contiguous whole 4-byte words and y an int64 vector")
    x = torch.empty(n, x_all.shape[1], dtype=x_all.dtype, device=dev)
    y = torch.empty(n, dtype=torch.int64, device=dev)
    masks = torch.empty(3, n, dtype=torch.uint8, device=dev)
    seed_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    _lib.check(L.sgs_nbr_gather(_ptr(node_ids), n, N, _ptr(x_all), row_bytes, _ptr(x), _ptr(y_all), _ptr(y), _ptr(graph.masks, torch.uint8), sp, sb,
                                _ptr(masks), _ptr(seed_mask), _stream()), "sgs_nbr_gather")
    return _collated_batch(x, ei, y, masks, prob, node_ids, eid=eid, seed_mask=seed_mask.view(torch.bool), n_seeds=int(n_seeds),
                           hop_nodes=list(hop_nodes))


def neighbor_batch(graph, seeds, fanouts, keys, subgraph_type: str = "induced", weight_q=None):
    """One neighbour-sampled Batch on the device: `seeds` (distinct node ids on the host), one fan-out and one stream key per hop.  Per hop
    two selection launches, two frontier launches and ONE 16-byte read-back (the new frontier's size and what its rows will emit); then
    nbr_collate.  data.neighbor_collate_torch is the same batch as a torch composition.  `weight_q` (int32 [E] in in-CSR order, aligned with
    graph.in_eid): every hop draws in proportion to it (nbr_select's `wq`); the launches and read-backs are the same."""
    _need_gpu(graph.edge_index)
    dev, N = graph.edge_index.device, graph.num_nodes
    seeds = torch.as_tensor(seeds, dtype=torch.int64)
    front = seeds.to(torch.int32).to(dev)
    deg = graph.in_deg_host[seeds]
    total = int(deg.sum() if fanouts[0] < 0 else deg.clamp(max=int(fanouts[0])).sum())
    nbr_begin(front, N, graph._nbr_state)
    hop_nodes, chosen, n = [int(seeds.numel())], [], int(seeds.numel())
    for h, (f, K) in enumerate(zip(fanouts, keys)):
        if front.numel() == 0 or total == 0:
            hop_nodes.append(0)
            front, total = front[:0], 0
            continue
        c = nbr_select(graph.in_ptr, graph.in_eid, N, front, f, K, total, weight_q)
        chosen.append(c)
        nxt = int(fanouts[h + 1]) if h + 1 < len(fanouts) else 0
        front, sizes = nbr_frontier(c, graph.edge_index, N, graph.in_ptr, nxt, graph._nbr_state, min(total, N - n))
        n_new, total = (int(v) for v in sizes.tolist())
        front = front[:n_new]
        hop_nodes.append(n_new)
        n += n_new
    return nbr_collate(graph, n, chosen, subgraph_type, int(seeds.numel()), hop_nodes)
