"""The batched ensemble-evaluation engines: everything that knows both the models and the batched (`*_multi`) ops.  evaluate.py routes a
call here (`_batched_ok`), plans its passes (`plan_draws`, `split_passes`) and hands each partition to `run_partition` with the model's row; the
ctypes wrappers of the kernels are in ops.py, which knows nothing of the models.  All draws of a partition run as passes of batched
kernels; draw d uses the same (seed, stream id) as the serial loop's d-th draw, so the drawn edge sets are identical.

One table, ENGINES, has a row per engine: which models it serves, its head name, its extra opt-in, (H, C), dropout-clock ticks per eval
forward, per-draw bytes for the planner and `prepare`.  A call takes the engine iff all of these hold (else the serial loop):

  args.sgs_eval_batch           truthy: True (draws per pass from a byte budget) or an int k >= 1 (at most k per pass); falsy = off, and
                                then nothing else is looked at.  Anything else raises ValueError, as does a malformed opt-in below --
                                before a path is counted or a partition is read.
  args.sgs_eval_batch_cover     True, needed only under args.sgs_cover_nodes (node-covering draws; every pass then draws with
                                ops.sample_topq_multi(..., cover=)).  Without it the cover flag keeps the serial loop and no other
                                opt-in is even validated; with it the others decide exactly as they do without the flag.
  args.sgs_eval_batch_heads     selects the row's head: absent / None = ("GCN",), "all", or a collection of names from HEADS.
  the row's own opt-in          True, for the rows that have one: sgs_eval_batch_variants (GAT with heads in 2..16 and / or
                                gat_edge_weight; Chebyshev K in 2..8), sgs_eval_batch_gatv2 (gat_v2, every head count, with and without
                                the edge term; sgs_eval_batch_variants plays no part), sgs_eval_batch_gine (gin_edge_weight).
  n_draws >= 1, and the model has a row at all.

The four boolean opt-ins take absent / None / False = off and True = on."""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from .model import ChebModel, GATModel, GINModel, GNNModel
from .ops import (ACT_NONE, ACT_RELU, HEADS_CONCAT, HEADS_MEAN, SAMPLE_LEARNED, Graph, MultiSampleResult, _cheb_step_multi, _empty_f32,
                  _spmm_heads_multi, _spmm_multi, _x_wt, cheb_norm_multi, ensemble_mean_correct, feature_csr, gat_alpha_heads_multi,
                  gat_alpha_multi, gat_scores, gatv2_alpha_heads_multi, gcn_norm_multi, get_graph, gine_aggregate_multi, graph_filter_multi,
                  linear_nobias, sample_topq_multi)
from .sampling import cover_nodes

EVAL_BATCH_BUDGET = 512 << 20          # bytes of per-pass buffers when args.sgs_eval_batch is True
HEADS = ("GCN", "GAT", "GIN", "Cheb")
OPTINS = ("sgs_eval_batch_variants", "sgs_eval_batch_cover", "sgs_eval_batch_gine", "sgs_eval_batch_gatv2")    # in validation order


# ------------------------------------------------------------------ per-draw logits of each engine (forward only)
def _drawn_gcn_logits(parent: Graph, smp: MultiSampleResult, w, xl1, b1, W2, b2):
    """Logits [D, N, C] of the two GCN layers over each of the D drawn subgraphs of `parent` (one launch per stage for all draws):
    in-CSRs filtered out of the parent's, weighted (w [D, q]) or unit gcn_norm, layer 1 over the shared x W1^T, one library GEMM
    [D N, H] x W2^T for layer 2."""
    D, q, N = smp.D, smp.q, parent.N
    csr = graph_filter_multi(parent, smp)
    _, _, what_in, what_loop = gcn_norm_multi(csr, w, q, N)
    H = xl1.shape[1]
    h = _spmm_multi(xl1, 0, csr, what_in, what_loop, b1, ACT_RELU, q, N, H)
    z = (h.view(D * N, H) @ W2.t()).contiguous()
    return _spmm_multi(z, N * z.shape[1], csr, what_in, what_loop, b2, ACT_NONE, q, N, z.shape[1])


def _drawn_gat_logits(parent: Graph, smp: MultiSampleResult, convs, xl1, a_s1, a_d1):
    """Logits [D, N, C] of the two GATConv layers (heads = 1, eval: no attention dropout) over each of the D drawn subgraphs: layer 1 over
    the shared x' = lin_src(x) and its node scores, one library GEMM [D N, H] x W2^T and one sgs_gat_scores_fwd over the D N rows (row-local:
    draw d's scores are what that kernel gives on draw d's block alone) for layer 2.  The alpha buffers are reused by layer 2."""
    D, q, N = smp.D, smp.q, parent.N
    c1, c2 = convs
    csr = graph_filter_multi(parent, smp)
    alpha = gat_alpha_multi(a_s1, a_d1, 0, csr, q, N, c1.negative_slope)
    H = xl1.shape[1]
    h = _spmm_multi(xl1, 0, csr, alpha[0], alpha[1], c1.bias, ACT_RELU, q, N, H)
    z = c2.lin_src(h.view(D * N, H)).contiguous()                    # nn.Linear, as GATConv.forward
    C = z.shape[1]
    a_s2, a_d2 = gat_scores(z, c2.att_src, c2.att_dst)
    alpha = gat_alpha_multi(a_s2, a_d2, N, csr, q, N, c2.negative_slope, out=alpha)
    return _spmm_multi(z, N * C, csr, alpha[0], alpha[1], c2.bias, ACT_NONE, q, N, C)


def _drawn_gin_logits(parent: Graph, smp: MultiSampleResult, convs, u1):
    """Logits [D, N, C] of the two GINConv layers over each of the D drawn subgraphs: the sum aggregation of sum_norm (unit value on every
    drawn entry, existing (i,i) entries included, diagonal 1 + eps) as the draw-strided SpMM, then each MLP's second Linear over [D N, .]
    in one library GEMM.  u1 = x W0^T of the first conv, shared by all draws."""
    D, q, N = smp.D, smp.q, parent.N
    f32 = dict(dtype=torch.float32, device=u1.device)
    csr = graph_filter_multi(parent, smp)
    ones = torch.ones(D, max(q, 1), **f32)
    h = u1
    for k, conv in enumerate(convs):
        l0, l1 = conv.nn.lins
        x_stride = 0 if k == 0 else N * l0.out_features
        if k > 0:
            h = linear_nobias(h, l0.weight).contiguous()
        diag = torch.full((D, max(N, 1)), 1.0 + conv._eps, **f32)
        a = _spmm_multi(h, x_stride, csr, ones, diag, l0.bias, ACT_RELU, q, N, l0.out_features)
        h = linear_nobias(a.view(D * N, -1), l1.weight)
        h += l1.bias                                                  # GINConv.forward: linear_nobias(h, W1) + b1
        if k == 0:
            h.relu_()                                                 # GIN.forward: F.relu between the convs (eval: no dropout)
    return h.view(D, N, -1)


def _drawn_gine_logits(parent: Graph, smp: MultiSampleResult, w, convs, x):
    """Logits [D, N, C] of the two GINEConv layers (GIN.forward in eval mode: ReLU between the convs, no dropout and no dropout seed) over
    each of the D drawn subgraphs of `parent`: one gine_aggregate_multi launch per layer for all draws -- layer 1 at the input width over
    the shared `x` (x_stride = 0), layer 2 at the hidden width over the per-draw blocks (x_stride = N H) -- and each MLP Linear as one
    library GEMM over the [D N, .] rows.  `w` [D, q]: the draws' straight-through weights (learned mode), or None (unit weights, as
    edge_weight=None in the model)."""
    D, q, N = smp.D, smp.q, parent.N
    csr = graph_filter_multi(parent, smp)
    h, x_stride = x, 0
    for k, conv in enumerate(convs):
        l0, l1 = conv.nn.lins
        z = gine_aggregate_multi(h, x_stride, csr, w, conv.lin.weight, conv.lin.bias, 1.0 + conv._eps, q, N, conv.in_channels)
        h = linear_nobias(z.view(D * N, -1), l0.weight)
        h += l0.bias
        h.relu_()                                                     # GINEConv.forward: relu(linear_nobias(z, W0) + b0)
        h = linear_nobias(h, l1.weight)
        h += l1.bias
        if k == 0:
            h.relu_()                                                 # GIN.forward: F.relu between the convs (eval: no dropout)
            x_stride = N * h.shape[1]
    return h.view(D, N, -1)


def _drawn_gat_heads_logits(parent: Graph, smp: MultiSampleResult, convs, xl1, a_s1, a_d1, w=None, coefs=None):
    """Logits [D, N, C] of the two GATConv layers on the per-head kernels (heads K >= 2, or any K with the edge term; eval: no attention
    dropout) over each of the D drawn subgraphs.  Layer 1 (concat) runs over the shared x' = lin_src(x) and its node scores [N, K]; layer 2
    (head mean) is one library GEMM [D N, H] x W2^T and one gat_scores call over the D N rows (row-local).  `w` [D, q] (the draws'
    straight-through weights) with `coefs` = the two layers' edge_coef [K] adds the edge term, as edge_weight does in GAT.forward; both
    None = the unweighted per-head softmax.  The alpha buffers are reused by layer 2."""
    D, q, N = smp.D, smp.q, parent.N
    c1, c2 = convs
    K = c1.heads
    csr = graph_filter_multi(parent, smp)
    edge = (lambda k: dict(edge_w=w, edge_coef=coefs[k])) if w is not None else (lambda k: {})
    alpha = gat_alpha_heads_multi(a_s1, a_d1, 0, csr, q, N, K, c1.negative_slope, **edge(0))
    H = xl1.shape[1]
    h = _spmm_heads_multi(xl1, 0, csr, alpha[0], alpha[1], HEADS_CONCAT if c1.concat else HEADS_MEAN, c1.bias, ACT_RELU, q, N, K, H // K)
    z = c2.lin_src(h.view(D * N, -1)).contiguous()                   # nn.Linear, as GATConv.forward
    C = z.shape[1] // K
    a_s2, a_d2 = gat_scores(z, c2.att_src, c2.att_dst, heads=K)
    alpha = gat_alpha_heads_multi(a_s2, a_d2, N * K, csr, q, N, K, c2.negative_slope, out=alpha, **edge(1))
    return _spmm_heads_multi(z, N * K * C, csr, alpha[0], alpha[1], HEADS_CONCAT if c2.concat else HEADS_MEAN, c2.bias, ACT_NONE, q, N, K, C)


def _drawn_gatv2_logits(parent: Graph, smp: MultiSampleResult, convs, xl1, xr1, w=None):
    """Logits [D, N, C] of the two GATv2Conv layers (eval: no attention dropout) over each of the D drawn subgraphs of `parent`, every
    1 <= heads <= 16: one gatv2_alpha_heads_multi launch and one _spmm_heads_multi launch per layer for all draws.  Layer 1 (concat, ReLU)
    runs over the shared xl1 = lin_l(x), xr1 = lin_r(x) (x_stride = 0).  Layer 2 (head mean) takes one library product over the [D N, H]
    hidden rows with cat(lin_l.weight, lin_r.weight) plus the two biases -- GATv2Conv.forward's call --, sliced into contiguous
    xl2 / xr2 [D, N, K C] (x_stride = N K C); the alpha buffers are reused.  `w` [D, q] (the draws' straight-through weights) adds the edge
    term with each layer's lin_edge.weight, as edge_weight does in GAT.forward; None = no edge term."""
    D, q, N = smp.D, smp.q, parent.N
    c1, c2 = convs
    K = c1.heads
    csr = graph_filter_multi(parent, smp)
    edge = (lambda c: dict(edge_w=w, lin_edge=c.lin_edge.weight)) if w is not None else (lambda c: {})
    alpha = gatv2_alpha_heads_multi(xl1, xr1, 0, c1.att, csr, q, N, K, c1.negative_slope, **edge(c1))
    H = xl1.shape[1]
    h = _spmm_heads_multi(xl1, 0, csr, alpha[0], alpha[1], HEADS_CONCAT if c1.concat else HEADS_MEAN, c1.bias, ACT_RELU, q, N, K, H // K)
    W2 = c2.heads * c2.out_channels
    y = linear_nobias(h.view(D * N, -1), torch.cat([c2.lin_l.weight, c2.lin_r.weight], 0))
    y += torch.cat([c2.lin_l.bias, c2.lin_r.bias])                   # in place: the same sums as GATv2Conv.forward's, no second [D N, 2 K C]
    xl2, xr2 = y[:, :W2].contiguous(), y[:, W2:].contiguous()
    alpha = gatv2_alpha_heads_multi(xl2, xr2, N * W2, c2.att, csr, q, N, K, c2.negative_slope, out=alpha, **edge(c2))
    return _spmm_heads_multi(xl2, N * W2, csr, alpha[0], alpha[1], HEADS_CONCAT if c2.concat else HEADS_MEAN, c2.bias, ACT_NONE, q, N, K,
                             c2.out_channels)


def _cheb_layer_multi(K, Y0, y0_stride, B, b_stride, csr, l_in, bias, act, q, N, D):
    """_ChebConv.forward's Clenshaw steps for D draws at once: Y0 [., N, W] and B [., N, (K - 1) W] = [Y_1 | ... | Y_{K-1}] with draw
    strides (0: the layer-1 products, shared by all draws).  The steps k = K - 2 .. 1 overwrite B's column blocks in place, so a shared B
    is copied per draw first when there are any (K >= 3); at K = 2 the last step only reads it.  -> [D, N, W]."""
    W = Y0.shape[-1]
    ldb = (K - 1) * W
    if K >= 3 and b_stride == 0:
        B = B.unsqueeze(0).expand(D, N, ldb).contiguous()
        b_stride = N * ldb
    b0 = B.data_ptr()
    blk = lambda k: b0 + 4 * (k - 1) * W                          # b_k's column block
    for k in range(K - 2, 0, -1):
        _cheb_step_multi(K, blk(k + 1), ldb, b_stride, N, W, q, D, csr, l_in, 2.0, blk(k), ldb, b_stride,
                         blk(k + 2) if k + 2 <= K - 1 else None, ldb, b_stride, None, ACT_NONE, blk(k), ldb, b_stride)
    out = _empty_f32(D, N, W, device=Y0.device)
    _cheb_step_multi(K, blk(1), ldb, b_stride, N, W, q, D, csr, l_in, 1.0, Y0.data_ptr(), W, y0_stride, blk(2) if K >= 3 else None, ldb, b_stride,
                     bias, act, out.data_ptr(), W, N * W)
    return out


def _drawn_cheb_logits(parent: Graph, smp: MultiSampleResult, w, convs, K: int, Y0, B):
    """Logits [D, N, C] of the two ChebConv layers of order K >= 2 (eval: ReLU between them, no dropout) over each of the D drawn subgraphs:
    one normalisation per draw for both layers (weighted by `w` [D, q], or unit), layer 1 from the shared products Y0 = x W_0^T and
    B = x [W_1 | ... | W_{K-1}]^T, layer 2 from the same two library products over the [D N, H] hidden rows."""
    D, q, N = smp.D, smp.q, parent.N
    c1, c2 = convs
    csr = graph_filter_multi(parent, smp)
    _, l_in = cheb_norm_multi(parent, smp, csr, w)
    h = _cheb_layer_multi(K, Y0, 0, B, 0, csr, l_in, c1.bias, ACT_RELU, q, N, D)
    hf = h.view(D * N, -1)
    C = c2.out_channels
    Wcat = torch.cat([lin.weight for lin in c2.lins], 0)
    Y0b, Bb = _x_wt(hf, Wcat[:C]), _x_wt(hf, Wcat[C:])               # the serial layer's two products, over all draws' rows
    return _cheb_layer_multi(K, Y0b, N * C, Bb, N * (K - 1) * C, csr, l_in, c2.bias, ACT_NONE, q, N, D)


# ------------------------------------------------------------------ each engine's `prepare`
# prepare(model, batch, weighted) -> (want_w, logits): the draw-independent first product, computed once per partition by the very call the
# serial path makes (so its bits are the serial path's), and `logits(parent, smp)` -> [D, N, C] for a pass -- or, for an engine that
# ignores the graph, the fixed logits [N, C] themselves.  `weighted`: learned mode, the draws can carry straight-through weights;
# `want_w` asks for them (smp.w is None otherwise: unit weights / no edge term, as edge_weight=None in the model).
def _prepare_gcn_layers(gcn1, gcn2, batch, weighted):
    feature_csr(batch.x, build=True)
    xl1 = _x_wt(batch.x, gcn1.lin.weight).contiguous()
    return weighted, lambda parent, smp: _drawn_gcn_logits(parent, smp, smp.w, xl1, gcn1.bias, gcn2.lin.weight, gcn2.bias)


def _prepare_gat(model, batch, weighted):
    """Both GAT v1 engines.  One head without the edge term ignores edge weights: none are drawn."""
    convs = tuple(model.GAT.convs)
    xl1 = convs[0].lin_src(batch.x).contiguous()
    K = convs[0].heads
    edge = weighted and convs[0].edge_dim is not None                # GAT.forward: the edge term needs edge_dim and weights
    if K == 1 and not edge:
        a_s1, a_d1 = gat_scores(xl1, convs[0].att_src, convs[0].att_dst)
        return False, lambda parent, smp: _drawn_gat_logits(parent, smp, convs, xl1, a_s1, a_d1)
    a_s1, a_d1 = gat_scores(xl1, convs[0].att_src, convs[0].att_dst, heads=K)
    coefs = tuple(c.edge_coef().reshape(K).contiguous() for c in convs) if edge else None
    return edge, lambda parent, smp: _drawn_gat_heads_logits(parent, smp, convs, xl1, a_s1, a_d1, smp.w, coefs)


def _prepare_gatv2(model, batch, weighted):
    convs = tuple(model.GAT.convs)                                    # GATv2Conv: the softmax gathers rows of x_l and x_r
    c1 = convs[0]
    W1 = c1.heads * c1.out_channels
    y1 = linear_nobias(batch.x, torch.cat([c1.lin_l.weight, c1.lin_r.weight], 0)) + torch.cat([c1.lin_l.bias, c1.lin_r.bias])
    xl1, xr1 = y1[:, :W1].contiguous(), y1[:, W1:].contiguous()      # GATv2Conv.forward's call: x_l and x_r as one product
    edge = weighted and c1.edge_dim is not None                       # GAT.forward: the edge term needs edge_dim and weights
    return edge, lambda parent, smp: _drawn_gatv2_logits(parent, smp, convs, xl1, xr1, smp.w)


def _prepare_gin(model, batch, weighted):
    convs = tuple(model.GIN.convs)                                    # GINConv ignores edge weights: none are drawn
    u1 = linear_nobias(batch.x, convs[0].nn.lins[0].weight).contiguous()
    return False, lambda parent, smp: _drawn_gin_logits(parent, smp, convs, u1)


def _prepare_gine(model, batch, weighted):
    convs = tuple(model.GIN.convs)                                    # GINEConv: nothing to precompute, the aggregation reads x itself
    xc = batch.x.contiguous()
    return weighted, lambda parent, smp: _drawn_gine_logits(parent, smp, smp.w, convs, xc)


def _prepare_cheb(model, batch, weighted):
    convs, K = (model.gcn1, model.gcn2), model.cheb_k
    H = convs[0].out_channels
    Wcat = torch.cat([lin.weight for lin in convs[0].lins], 0)
    Y0, B = _x_wt(batch.x, Wcat[:H]), _x_wt(batch.x, Wcat[H:])        # _ChebConv.forward's two products
    return weighted, lambda parent, smp: _drawn_cheb_logits(parent, smp, smp.w, convs, K, Y0, B)


def _prepare_cheb_k1(model, batch, weighted):
    return False, model(batch, batch.edge_index).contiguous()         # K = 1 ignores the graph: [N, C], the same for every draw


# ------------------------------------------------------------------ each engine's per-draw bytes on top of plan_draws' common term
# GCN and Chebyshev K = 1 allocate nothing beside the common term.
_no_bytes = lambda E, q, N, H, C, **_: 0
# GAT v1, K = gat_heads: attention values [q, K], loop terms [N, K] and layer-2 node scores 2 [N, K], 4 q K + 12 N K, plus the layer-2
# product [N, K C] beside the logits, 4 N C (K - 1); gat_edge adds 8 N (the mean loop weight and count of the edge term; the kernels take
# them as optional outputs, counted always).
_gat_bytes = lambda E, q, N, H, C, gat_heads, gat_edge, **_: (4 * q * gat_heads + 12 * N * gat_heads + 4 * N * C * (gat_heads - 1)
                                                              + (8 * N if gat_edge else 0))
# GATv2: attention values [q, K] and loop attentions [N, K] (one pair, reused by layer 2; eval takes no soft copies and no mean loop weight /
# count, so gat_edge adds nothing), the layer-2 product [N, 2 K C] (lin_l and lin_r in one GEMM, the biases added in place) and its two
# contiguous halves x_l, x_r [N, K C] each.  Never below _gat_bytes at the same arguments (12 N K C + 4 N C >= 8 N K + 8 N for K, C >= 1),
# so never a larger pass than that term's.
_gatv2_bytes = lambda E, q, N, H, C, gat_heads, **_: 4 * q * gat_heads + 4 * N * gat_heads + 16 * N * gat_heads * C
# GIN: the MLP's second hidden block 4 N H, the second conv's product and aggregate 8 N C, unit edge values 4 q, the 1 + eps diagonal 4 N.
_gin_bytes = lambda E, q, N, H, C, **_: 4 * N * H + 8 * N * C + 4 * q + 4 * N
# GINE at input width F = gine_in, beside the counted hidden block and two logit blocks (the second MLP's two [N, C] products): the first
# aggregate [N, F], the first MLP's second product [N, H] and the second aggregate [N, H] (unit weights are a NULL pointer and 1 + eps a
# scalar: neither is allocated; the straight-through weights are the 4 B per drawn edge of the common term).
_gine_bytes = lambda E, q, N, H, C, gine_in, **_: 4 * N * gine_in + 8 * N * H
# Chebyshev K = cheb_k >= 2: the (K - 1) out-wide block of b's of each layer, 4 N (K - 1) (H + C), the per-draw Laplacian values 4 q,
# dis 4 N and the weights scattered by parent edge id 4 E.
_cheb_bytes = lambda E, q, N, H, C, cheb_k, **_: 4 * N * (cheb_k - 1) * (H + C) + 4 * q + 4 * N + 4 * E


# ------------------------------------------------------------------ the engine table
class Engine(NamedTuple):
    name: str
    head: str                       # its name in args.sgs_eval_batch_heads and plan_draws' `head`
    serves: Callable                # model -> bool; every model has at most one row
    dims: Callable                  # model -> (hidden width H, classes C)
    extra_bytes: Callable           # (E, q, N, H, C, gat_heads=, gat_edge=, cheb_k=, gine_in=) -> per-draw bytes beside the common term
    prepare: Callable               # (model, batch, weighted) -> (want_w, logits callable or fixed logits tensor), see above
    plan_kw: Callable = lambda m: {}    # model -> plan_draws' keywords describing it
    ticks: int = 0                  # dropout seeds one eval-mode forward takes (GNNModel and GAT one per call; GIN and Cheb none)
    optin: Optional[str] = None     # the extra opt-in a model of this row needs
    own_term: bool = False          # plan_draws takes this row's extra_bytes, not the head's plain row's, under gat_v2 / gine_in / cheb_k >= 2


_gcn_dims = lambda m: (m.gcn1.out_channels, m.gcn2.out_channels)
_gat_dims = lambda m: (m.GAT.convs[0].out_channels * m.GAT.convs[0].heads, m.GAT.convs[1].out_channels)
_gin_dims = lambda m: (m.GIN.convs[0].nn.lins[0].out_features, m.GIN.convs[1].nn.lins[0].out_features)
_cheb_dims = lambda m: (m.gcn1.lins[0].out_features, m.gcn2.lins[0].out_features)
_gat_kw = lambda m: dict(gat_heads=m.gat_heads, gat_edge=bool(m.gat_edge_weight))

ENGINES = (
    Engine("GCN", "GCN", lambda m: isinstance(m, GNNModel), _gcn_dims, _no_bytes,
           lambda m, batch, weighted: _prepare_gcn_layers(m.gcn1, m.gcn2, batch, weighted), ticks=1),
    Engine("GAT, one head", "GAT", lambda m: isinstance(m, GATModel) and not m.gat_v2 and m.gat_heads == 1 and not m.gat_edge_weight,
           _gat_dims, _gat_bytes, _prepare_gat, plan_kw=_gat_kw, ticks=1),
    Engine("GAT, per-head kernels", "GAT",
           lambda m: isinstance(m, GATModel) and not m.gat_v2 and (2 <= m.gat_heads <= 16 or (m.gat_heads == 1 and m.gat_edge_weight)),
           _gat_dims, _gat_bytes, _prepare_gat, plan_kw=_gat_kw, ticks=1, optin="sgs_eval_batch_variants"),
    Engine("GATv2", "GAT", lambda m: isinstance(m, GATModel) and m.gat_v2 and 1 <= m.gat_heads <= 16, _gat_dims, _gatv2_bytes, _prepare_gatv2,
           plan_kw=lambda m: dict(_gat_kw(m), gat_v2=True), ticks=1, optin="sgs_eval_batch_gatv2", own_term=True),
    Engine("GIN", "GIN", lambda m: isinstance(m, GINModel) and not m.gin_edge_weight, _gin_dims, _gin_bytes, _prepare_gin),
    Engine("GINE", "GIN", lambda m: isinstance(m, GINModel) and m.gin_edge_weight, _gin_dims, _gine_bytes, _prepare_gine,
           plan_kw=lambda m: dict(gine_in=m.GIN.convs[0].in_channels), optin="sgs_eval_batch_gine", own_term=True),
    Engine("Chebyshev K >= 2", "Cheb", lambda m: isinstance(m, ChebModel) and 2 <= m.cheb_k <= 8, _cheb_dims, _cheb_bytes, _prepare_cheb,
           plan_kw=lambda m: dict(cheb_k=m.cheb_k), optin="sgs_eval_batch_variants", own_term=True),
    Engine("Chebyshev K = 1", "Cheb", lambda m: isinstance(m, ChebModel) and m.cheb_k == 1, _cheb_dims, _no_bytes, _prepare_cheb_k1),
)


def engine_of(model) -> Optional[Engine]:
    """The model's row of ENGINES, or None for a module no engine serves."""
    return next((e for e in ENGINES if e.serves(model)), None)


def _head_of(model):
    """-> "GCN" / "GAT" / "GIN" / "Cheb" for the four heads, None for any other module."""
    return getattr(engine_of(model), "head", None)


def _head_dims(model, head):
    """(hidden width, classes) of a head, from the model's row; `head` is unused (kept for the callers that pass _head_of(model))."""
    return engine_of(model).dims(model)


# ------------------------------------------------------------------ routing and planning
def _opt_bool(args, name) -> bool:
    """args.<name>: absent / None / False -> False, True -> True.  Anything else raises ValueError."""
    v = getattr(args, name, None)
    if v is None or v is False:
        return False
    if v is True:
        return True
    raise ValueError(f"args.{name}={v!r}: need None, False or True")


def _eval_heads(args) -> frozenset:
    """The heads args.sgs_eval_batch_heads sends to the batched engine: absent / None -> {"GCN"}, "all" -> all four, else a list, tuple or
    set of names from HEADS.  Anything else raises ValueError."""
    v = getattr(args, "sgs_eval_batch_heads", None)
    if v is None:
        return frozenset(("GCN",))
    if isinstance(v, str):
        if v == "all":
            return frozenset(HEADS)
    elif isinstance(v, (list, tuple, set, frozenset)) and all(isinstance(h, str) and h in HEADS for h in v):
        return frozenset(v)
    raise ValueError(f"args.sgs_eval_batch_heads={v!r}: need None, 'all' or a collection of names from {HEADS}")


def _batched_ok(args, model, n_draws) -> bool:
    """Whether this call takes the batched engine: the rules of the module docstring, checked in this order before any partition is read."""
    cover = cover_nodes(args)
    flag = getattr(args, "sgs_eval_batch", False)
    if not flag:
        return False
    if cover and (getattr(args, "sgs_eval_batch_cover", None) is None or getattr(args, "sgs_eval_batch_cover", None) is False):
        return False                            # the routing from before the opt-in existed: nothing else is consulted
    if flag is not True and (isinstance(flag, bool) or not isinstance(flag, int) or flag < 1):
        raise ValueError(f"args.sgs_eval_batch={flag!r}: need True (draws per pass from a byte budget) or an int >= 1 (at most k per pass)")
    heads = _eval_heads(args)
    on = {name: _opt_bool(args, name) for name in OPTINS}
    e = engine_of(model)
    if n_draws < 1 or e is None or (e.optin is not None and not on[e.optin]):
        return False
    return e.head in heads


def plan_draws(E: int, q: int, N: int, H: int, C: int, D: int, budget, head: str = "GCN", *, gat_heads: int = 1, gat_edge: bool = False,
               cheb_k: int = 1, cover: bool = False, gine_in: int = 0, gat_v2: bool = False) -> list:
    """Draws per pass of the batched engine: a list of pass sizes summing to D, each >= 1.  `budget` is True (the largest pass whose
    per-draw buffers fit EVAL_BATCH_BUDGET bytes), an int number of bytes via ("bytes", n), or an int k >= 1 (at most k draws per pass).
    Per draw (an upper estimate of the engine's per-draw allocations), common to all engines: keys 4 E + mask E + filter positions 4 E;
    per drawn edge 40 B (int64 id 8, int64 endpoints 16 -- allocated only under the trace hook, counted always --, weight 4, CSR source
    and id 8, normalised weight 4); per-node arrays 36 N; hidden 4 N H; two logit blocks 8 N C.  The engine's row of ENGINES adds its own
    term (see the *_bytes functions); the row is that of `head`, or the head's own-term row under `gat_v2` (head "GAT" only), `gine_in`
    = the input width F > 0 (head "GIN" only) or `cheb_k` >= 2 (head "Cheb"); gat_heads and gat_edge describe a GAT model.  `cover`
    (node-covering draws) adds sample_topq_multi(..., cover=)'s per-draw workspace and output: 1024 per-workgroup counts of forced edges
    (4096 B) and the cover_info pair (8 B); it never makes a pass larger.  The result of the engine does not depend on the split."""
    D = int(D)
    if D < 1:
        raise ValueError(f"plan_draws: D={D} draws")
    if head not in HEADS:
        raise ValueError(f"plan_draws: head={head!r}, need one of {HEADS}")
    if not 1 <= int(gat_heads) <= 16 or not 1 <= int(cheb_k) <= 8:
        raise ValueError(f"plan_draws: gat_heads={gat_heads}, cheb_k={cheb_k}: need 1..16 and 1..8")
    gine_in = int(gine_in)
    if gine_in < 0 or (gine_in and head != "GIN"):
        raise ValueError(f"plan_draws: gine_in={gine_in} with head={head!r}: need 0, or the GINE head's input width >= 1 with head 'GIN'")
    if not isinstance(gat_v2, bool) or (gat_v2 and head != "GAT"):
        raise ValueError(f"plan_draws: gat_v2={gat_v2!r} with head={head!r}: need False, or True with head 'GAT'")
    if budget is True or (isinstance(budget, tuple) and budget[0] == "bytes"):
        nbytes = EVAL_BATCH_BUDGET if budget is True else int(budget[1])
        E, q, N, H, C = int(E), int(q), int(N), int(H), int(C)
        own = gat_v2 or gine_in > 0 or (head == "Cheb" and int(cheb_k) > 1)
        row = next(e for e in ENGINES if e.head == head and e.own_term == own)
        per = 4 * ((E + 63) & ~63) + E + 4 * E + 40 * q + 36 * (N + 1) + 4 * N * H + 8 * N * C + 3 * 2048 * 4 + 64
        per += row.extra_bytes(E, q, N, H, C, gat_heads=int(gat_heads), gat_edge=gat_edge, cheb_k=int(cheb_k), gine_in=gine_in)
        if cover:
            per += 4 * 1024 + 8
        k = max(1, min(D, int(nbytes) // per))
    else:
        k = int(budget)
        if k < 1:
            raise ValueError(f"sgs_eval_batch={budget}: need True or an int >= 1")
        k = min(k, D)
    return [k] * (D // k) + ([D % k] if D % k else [])


def split_passes(plan, given, seed: int, tick: int, device=None):
    """The passes of one partition, as run_partition takes them, from `plan` (plan_draws' list) and `given` (per draw: explicit
    noise [E] or None = a draw from the noise clock now at (seed, tick)).  A pass never mixes explicit noise and clock draws, so a plan
    entry is cut where the kind changes.  -> ([(n, noise [n, E] float32 on `device` or None, seed, first stream id), ...] in draw order,
    the number of clock ticks consumed -- the caller advances the clock)."""
    passes, d, used = [], 0, 0
    for k in plan:
        while k > 0:
            explicit = given[d] is not None
            n = 1
            while n < k and (given[d + n] is not None) == explicit:
                n += 1
            if explicit:
                passes.append((n, torch.stack([t.to(device=device, dtype=torch.float32) for t in given[d:d + n]]).contiguous(), 0, 0))
            else:
                passes.append((n, None, seed, tick + used + 1))
                used += n
            d += n
            k -= n
    return passes, used


# ------------------------------------------------------------------ the partition driver
def run_partition(batch, prepare, q, mode, p, passes, counts, trace, cover):
    """All draws of one partition for any engine: prepare(batch, weighted) once, then per pass the draws (sample_topq_multi), the engine's
    logits for all of them and their fold into the running mean and the counts (ensemble_mean_correct).  An engine with fixed logits
    folds them D times and draws only when `trace` asks for the edge lists; the parent graph is built only for an engine that draws."""
    x, ei = batch.x, batch.edge_index
    N = x.shape[0]
    want_w, logits = prepare(batch, mode == SAMPLE_LEARNED and p is not None)     # (weighted: the draws carry straight-through weights)
    draws = not isinstance(logits, torch.Tensor)                                  # (a tensor: fixed logits, the same for every draw)
    parent = get_graph(ei, N) if draws else None
    D_total = sum(int(ps[0]) for ps in passes)
    acc = None
    done = 0
    logs, edges = [], []
    for k, (Dc, noise, seed, sid0) in enumerate(passes):
        if draws or trace is not None:
            smp = sample_topq_multi(mode, p, None, 0.0, q, ei, Dc, noise=noise, seed=seed, stream_id0=sid0, want_edge_index=trace is not None,
                                    want_w=want_w, cover=cover)
        if draws:
            out = logits(parent, smp)
            stride = N * out.shape[2]
        else:
            out, stride = logits, 0
        if acc is None:
            acc = _empty_f32(N, out.shape[-1], device=x.device)
        done += Dc
        ensemble_mean_correct(out, stride, Dc, acc, k == 0, done == D_total, D_total, batch.y,
                              (batch.train_mask, batch.val_mask, batch.test_mask), counts)
        if trace is not None:
            logs.append(out if stride else out.unsqueeze(0).expand(Dc, *out.shape))
            edges.append(smp.edge_index)
    if trace is not None:
        trace["logits"], trace["mean"], trace["edges"] = torch.cat(logs), acc, torch.cat(edges)
    return acc


def ensemble_partition(batch, gcn1, gcn2, q: int, mode: int, p, passes, counts, trace=None, *, cover=None):
    """All draws of ONE partition on the GCN engine, batched: `passes` is a list of (Dc, noise [Dc, E] or None, seed, stream_id0), in draw
    order (split_passes).  mode SAMPLE_LEARNED with p (the scorer's probabilities, istest: straight-through weights on the edges),
    SAMPLE_PRIOR with p = batch.prob (unit weights), or SAMPLE_LEARNED with p None (uniform draw, unit weights).  Adds the partition's three
    (correct, total) counts to `counts` and returns the mean logits [N, C].  `trace` (dict or None): receives per-draw logits [D, N, C],
    mean [N, C] and the drawn edge lists [D, 2, q].  `cover` (the partition's cached get_graph(edge_index, N), the same object as the
    filter's parent, or None): every draw is node-covering."""
    return run_partition(batch, lambda b, weighted: _prepare_gcn_layers(gcn1, gcn2, b, weighted), q, mode, p, passes, counts, trace, cover)


def ensemble_partition_head(batch, model, q: int, mode: int, p, passes, counts, trace=None, *, cover=None):
    """ensemble_partition for any model with a row in ENGINES, same arguments and result."""
    e = engine_of(model)
    if e is None:
        raise TypeError(f"ensemble_partition_head: no batched engine for {type(model).__name__}")
    return run_partition(batch, lambda b, weighted: e.prepare(model, b, weighted), q, mode, p, passes, counts, trace, cover)
