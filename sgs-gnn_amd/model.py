"""Host-side mirror of the reference's model.py: same class names, constructor signatures,
forward signatures and state_dict keys, with every sparse / per-edge
op running in libsgs_hip.so.  Dense node-level X W^T products are library GEMMs (torch ->
hipBLASLt), as the hot-path scope allows.

Dropout: the reference draws nn.Dropout masks from torch's global generator; here masks are
counter-based, a pure function of (seed, site, row, col) (sgs_dropout_keep), fused into the
producing kernel.  `set_dropout_seed` / the per-forward step counter make every training
forward draw fresh masks.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

# dropout sites (model.py:107 scorer encoder, :121 _edge_score hidden, :160 GNN hidden, :21-25 MLP pre)
SITE_ENC, SITE_SCORE, SITE_GNN, SITE_MLP_X, SITE_MLP_Y = 1, 2, 3, 4, 5


class _DropoutClock:
    """Process-wide source of dropout seeds: seed = hash(base_seed, forward counter)."""
    base = 0x5D5C0FFEE
    tick = 0

    @classmethod
    def next_seed(cls) -> int:
        cls.tick += 1
        return (cls.base * 0x9E3779B97F4A7C15 + cls.tick * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF


def set_dropout_seed(seed: int) -> None:
    _DropoutClock.base = int(seed) & 0xFFFFFFFFFFFFFFFF
    _DropoutClock.tick = 0


class GCNConv(nn.Module):
    """PyG GCNConv(in, out) as the reference instantiates it (model.py:94-95,151-153): keys
    `lin.weight` [out,in] (glorot), `bias` [out] (zeros).  forward = lin -> gcn_norm ->
    propagate -> + bias, with optional fused ReLU / dropout epilogue."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))
        nn.init.uniform_(self.lin.weight, -a, a)
        nn.init.zeros_(self.bias)

    def _memo(self, x):
        """Memoised x W^T (plain tensor, no autograd graph) keyed on (x, W) identity + version: the hybrid step runs
        GNNModel twice on the same batch.x with the same weights (learned and random forward,
        training_hybrid.py:88,93); the weight gradient is computed by hand in the layer's backward."""
        W = self.lin.weight
        # `ops.memo_scope()`: the trainers / evaluators open a new scope per batch, so a memo never outlives the step it was
        # made in -- version counters alone are not enough (a replayed optimiser graph writes W without touching them)
        key = (ops.memo_scope(), x.data_ptr(), x._version, tuple(x.shape), W.data_ptr(), W._version)
        c = getattr(self, "_lin_cache", None)
        if c is not None and c[0] == key and c[1]() is x:
            return c[2], key
        return None, key

    def forward(self, x, edge_index, edge_weight=None, *, norm=None, act=ops.ACT_NONE, p=0.0, seed=0, site=0):
        if norm is None:
            norm = ops.gcn_norm(ops.get_graph(edge_index, x.shape[0]), edge_weight)
        xl, key = self._memo(x)
        y, xl = ops.gcn_layer(x, self.lin.weight, self.bias, norm, act=act, p=p, seed=seed, site=site, xl=xl)
        self._remember(key, x, xl)
        return y

    def _remember(self, key, x, xl):
        try:
            import weakref
            self._lin_cache = (key, weakref.ref(x), xl)
        except TypeError:
            self._lin_cache = None


class GNNModel(nn.Module):
    """model.py:147-164."""

    def __init__(self, in_channels, hidden_dim, num_classes, dropout_prob=0.3, edge_mlp_type='MLP'):
        super().__init__()
        from .scorer import get_edge_mlp
        self.edge_prob_mlp = get_edge_mlp(in_channels, hidden_dim, dropout_prob, edge_mlp_type)
        self.gcn1 = GCNConv(in_channels, hidden_dim)
        self.dropout = nn.Dropout(dropout_prob)
        self.gcn2 = GCNConv(hidden_dim, num_classes)

    def forward(self, data, edge_index, edge_weight=None):
        from .utils import segment
        x = data.x
        ops.feature_csr(x, build=True)                            # bag-of-words features: the first layer runs over their non-zeros (once per graph)
        with segment(self, "gnn_forward"):                        # model.py:156-163
            norm = ops.gcn_norm(ops.get_graph(edge_index, x.shape[0]), edge_weight)   # once for both layers
            p = self.dropout.p if self.training else 0.0
            act = ops.ACT_RELU_DROPOUT if p > 0 else ops.ACT_RELU
            # both layers in one autograd node (ops.gcn2): at partition scale the SpMMs carry h W2^T and the backward's dense work
            xl1, key = self.gcn1._memo(x)
            out, xl1 = ops.gcn2(x, self.gcn1.lin.weight, self.gcn1.bias, self.gcn2.lin.weight, self.gcn2.bias, norm, act=act, p=p,
                                seed=_DropoutClock.next_seed(), site=SITE_GNN, xl1=xl1)
            self.gcn1._remember(key, x, xl1)
            return out

    def forward_pair(self, data, edge_index_a, edge_weight_a, edge_index_b):
        """(forward(data, edge_index_a, edge_weight_a), forward(data, edge_index_b)), bitwise and with the same autograd graph, but with
        both graphs' jobs in each of the two forward launches (ops.gcn2_dual): the sampled step's learned and random forward.  Dropout
        seeds are drawn in the order of the two calls (a, then b)."""
        from .utils import segment
        x = data.x
        ops.feature_csr(x, build=True)
        with segment(self, "gnn_forward"):
            N = x.shape[0]
            norm_a = ops.gcn_norm(ops.get_graph(edge_index_a, N), edge_weight_a)
            norm_b = ops.gcn_norm(ops.get_graph(edge_index_b, N), None)
            p = self.dropout.p if self.training else 0.0
            act = ops.ACT_RELU_DROPOUT if p > 0 else ops.ACT_RELU
            xl1, key = self.gcn1._memo(x)
            seed_a = _DropoutClock.next_seed()
            seed_b = _DropoutClock.next_seed()
            out_a, out_b, xl1 = ops.gcn2_dual(x, self.gcn1.lin.weight, self.gcn1.bias, self.gcn2.lin.weight, self.gcn2.bias, norm_a, norm_b,
                                              act=act, p=p, seed_a=seed_a, seed_b=seed_b, site=SITE_GNN, xl1=xl1)
            self.gcn1._remember(key, x, xl1)
            return out_a, out_b


# ------------------------------------------------------------------ GAT head (model.py:189-208)
SITE_GAT_ATT, SITE_GAT_ACT = 16, 32          # attention dropout uses site, site + 1 per layer


class GATConv(nn.Module):
    """PyG 2.3.1 GATConv as torch_geometric.nn.models.GAT instantiates it: parameters `lin_src.weight` [heads * out, in] (shared with
    `lin_dst.weight`), `att_src`, `att_dst` [1, heads, out], `bias` [heads * out] (concat) or [out] (mean over heads).  heads = 1 runs the
    one-head kernels; 2 <= heads <= 16 the fused per-head ones (x' = lin_src(x) viewed as [N, heads, out], head-major columns).
    edge_dim = 1 adds `lin_edge.weight` [heads * out, 1] (no bias) and `att_edge` [1, heads, out]: a forward given `edge_weight` then adds
    edge_weight[e] * c_h, c_h = <lin_edge.weight[h, :], att_edge[h, :]>, to the logits (the added loops carry the mean weight of their
    node's in-edges), on the per-head kernels for every head count; without `edge_weight` it is the layer above and the two parameters
    get no gradient."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, edge_dim=None):
        super().__init__()
        heads = int(heads)
        if not 1 <= heads <= 16 or out_channels < 1:
            raise ValueError(f"GATConv: heads = {heads}, out_channels = {out_channels}: 1 <= heads <= 16 and out_channels >= 1 are supported")
        if edge_dim not in (None, 1):
            raise ValueError(f"GATConv: edge_dim = {edge_dim!r}: None and 1 (the edge weight as the attribute) are supported")
        self.in_channels, self.out_channels, self.negative_slope, self.dropout = in_channels, out_channels, negative_slope, dropout
        self.heads, self.concat, self.edge_dim = heads, bool(concat), edge_dim
        self.lin_src = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels))
        a = math.sqrt(6.0 / (in_channels + heads * out_channels))     # glorot on the parameter's own shape, as PyG
        nn.init.uniform_(self.lin_src.weight, -a, a)
        b = math.sqrt(6.0 / (heads + out_channels))                   # [1, heads, out]: size(-2) + size(-1)
        nn.init.uniform_(self.att_src, -b, b)
        nn.init.uniform_(self.att_dst, -b, b)
        if edge_dim is not None:                                      # after today's parameters: the default layer draws exactly as before
            self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)
            self.att_edge = nn.Parameter(torch.empty(1, heads, out_channels))
            e = math.sqrt(6.0 / (edge_dim + heads * out_channels))
            nn.init.uniform_(self.lin_edge.weight, -e, e)
            nn.init.uniform_(self.att_edge, -b, b)

    def edge_coef(self):
        """c [heads]: (lin_edge(w).view(-1, heads, out) * att_edge).sum(-1) = w * c for a one-column attribute."""
        return (self.lin_edge.weight.view(self.heads, self.out_channels) * self.att_edge.view(self.heads, self.out_channels)).sum(-1)

    def forward(self, x, edge_index, edge_weight=None, *, act=ops.ACT_NONE, p_act=0.0, seed=0, layer=0):
        graph = ops.get_graph(edge_index, x.shape[0])
        xl = self.lin_src(x)
        a_s, a_d = ops.gat_scores(xl, self.att_src, self.att_dst, heads=self.heads)      # node-level dots, one pass over x'
        p_att = self.dropout if self.training else 0.0
        if edge_weight is not None and self.edge_dim is None:
            raise ValueError("GATConv: edge_weight needs edge_dim = 1")
        edge = {} if edge_weight is None else {"edge_weight": edge_weight, "edge_coef": self.edge_coef()}
        return ops.gat_aggregate(xl, a_s, a_d, self.bias, graph, self.negative_slope, p_att, seed, SITE_GAT_ATT + 2 * layer, act,
                                 p_act, seed, SITE_GAT_ACT + layer, heads=self.heads, concat=self.concat, **edge)


class GATv2Conv(nn.Module):
    """PyG 2.3.1 GATv2Conv(in, out, heads, concat, negative_slope, dropout, edge_dim in {None, 1}) with share_weights=False, bias=True, as
    torch_geometric.nn.models.GAT(..., v2=True) instantiates it (restated from its published algorithm): parameters `lin_l.weight` /
    `lin_r.weight` [heads * out, in] with `lin_l.bias` / `lin_r.bias` [heads * out] (two separate Linears), `att` [1, heads, out], `bias`
    [heads * out] (concat) or [out] (mean over heads); edge_dim = 1 adds `lin_edge.weight` [heads * out, 1] (no bias).  The logit of an
    entry j -> i is att_h . leaky_relu(x_l[j, h] + x_r[i, h] (+ edge_weight[e] * lin_edge.weight[h])): the non-linearity sits inside the dot
    product, so the ranking of the neighbours depends on the destination ("dynamic attention").  The softmax, the removed (i, i) entries,
    the added loops (carrying the mean weight of their node's in-edges) and the output are GATConv's, with x_l as the message.  Runs on
    the gathering per-head kernels of csrc/gatv2.hip for every 1 <= heads <= 16; without `edge_weight` the edge parameter gets no gradient."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, edge_dim=None):
        super().__init__()
        heads = int(heads)
        if not 1 <= heads <= 16 or out_channels < 1:
            raise ValueError(f"GATv2Conv: heads = {heads}, out_channels = {out_channels}: 1 <= heads <= 16 and out_channels >= 1 are supported")
        if edge_dim not in (None, 1):
            raise ValueError(f"GATv2Conv: edge_dim = {edge_dim!r}: None and 1 (the edge weight as the attribute) are supported")
        self.in_channels, self.out_channels, self.negative_slope, self.dropout = in_channels, out_channels, negative_slope, dropout
        self.heads, self.concat, self.edge_dim = heads, bool(concat), edge_dim
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=True)
        self.lin_r = nn.Linear(in_channels, heads * out_channels, bias=True)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels))
        a = math.sqrt(6.0 / (in_channels + heads * out_channels))     # glorot on the parameter's own shape, as PyG
        for lin in (self.lin_l, self.lin_r):
            nn.init.uniform_(lin.weight, -a, a)
            nn.init.zeros_(lin.bias)
        b = math.sqrt(6.0 / (heads + out_channels))                   # [1, heads, out]: size(-2) + size(-1)
        nn.init.uniform_(self.att, -b, b)
        if edge_dim is not None:
            self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)
            e = math.sqrt(6.0 / (edge_dim + heads * out_channels))
            nn.init.uniform_(self.lin_edge.weight, -e, e)

    def forward(self, x, edge_index, edge_weight=None, *, act=ops.ACT_NONE, p_act=0.0, seed=0, layer=0):
        graph = ops.get_graph(edge_index, x.shape[0])
        if edge_weight is not None and self.edge_dim is None:
            raise ValueError("GATv2Conv: edge_weight needs edge_dim = 1")
        D = self.heads * self.out_channels
        Wcat = torch.cat([self.lin_l.weight, self.lin_r.weight], 0)   # [2 heads out, in]: the two Linears share x, one product
        y = ops.linear_nobias(x, Wcat) + torch.cat([self.lin_l.bias, self.lin_r.bias])
        p_att = self.dropout if self.training else 0.0
        edge = {} if edge_weight is None else {"edge_weight": edge_weight, "lin_edge": self.lin_edge.weight}
        return ops.gatv2_aggregate(y[:, :D], y[:, D:], self.att, self.bias, graph, self.negative_slope, p_att, seed, SITE_GAT_ATT + 2 * layer,
                                   act, p_act, seed, SITE_GAT_ACT + layer, heads=self.heads, concat=self.concat, **edge)


class GAT(nn.Module):
    """torch_geometric.nn.models.GAT(in, hidden, num_layers=2, out_channels, dropout, act='relu', heads=K): as PyG's GAT.init_conv, layer 0 is
    GATConv(in, hidden // K, heads=K, concat=True) and the last layer GATConv(hidden, out, heads=K, concat=False).  edge_dim = 1 is handed
    to both layers, and `edge_weight` then reaches them as their edge attribute (PyG: GAT(..., edge_dim=1) with
    edge_attr = edge_weight.view(-1, 1)).  v2=True builds the same two shapes from GATv2Conv (PyG: GAT(..., v2=True))."""
    supports_edge_weight = False

    def __init__(self, in_channels, hidden_channels, num_layers, out_channels, dropout=0.0, act='relu', heads=1, edge_dim=None, v2=False):
        super().__init__()
        if num_layers != 2 or act != 'relu':
            raise NotImplementedError
        if hidden_channels % heads != 0:
            raise ValueError(f"Ensure that the number of output channels of 'GATConv' (got '{hidden_channels}') is divisible by the number "
                             f"of heads (got '{heads}')")
        self.dropout, self.heads, self.edge_dim, self.v2 = dropout, int(heads), edge_dim, bool(v2)
        Conv = GATv2Conv if self.v2 else GATConv
        self.convs = nn.ModuleList([Conv(in_channels, hidden_channels // heads, heads=heads, concat=True, dropout=dropout, edge_dim=edge_dim),
                                    Conv(hidden_channels, out_channels, heads=heads, concat=False, dropout=dropout, edge_dim=edge_dim)])

    def forward(self, x, edge_index, edge_weight=None):
        # without edge_dim, edge_weight is dropped, exactly as PyG's BasicGNN does for a conv without edge-weight support
        p = self.dropout if self.training else 0.0
        act = ops.ACT_RELU_DROPOUT if p > 0 else ops.ACT_RELU
        seed = _DropoutClock.next_seed()
        if self.edge_dim is None or edge_weight is None:
            h = self.convs[0](x, edge_index, act=act, p_act=p, seed=seed, layer=0)
            return self.convs[1](h, edge_index, seed=seed, layer=1)
        attr = ops.gat_edge_attr(ops.get_graph(edge_index, x.shape[0]), edge_weight)     # one autograd edge to the weights for both layers
        h = self.convs[0](x, edge_index, attr, act=act, p_act=p, seed=seed, layer=0)
        return self.convs[1](h, edge_index, attr, seed=seed, layer=1)


class GATModel(nn.Module):
    """model.py:189-208.  `heads` is accepted and unused, as in the reference (its GATModel never hands it to GAT, so reference
    checkpoints are one-head); the keyword-only `gat_heads` is what reaches GAT (default 1 = the reference's model).  The keyword-only
    `gat_edge_weight=True` builds GAT(..., edge_dim=1): the sampled edge weights enter the attention logits and receive the task
    gradient (default False = the reference's model, which drops them).  The keyword-only `gat_v2=True` builds GAT(..., v2=True): both
    layers are GATv2Conv (dynamic attention); it combines with `gat_heads` and `gat_edge_weight`, and the default False draws, computes and
    counts dropout seeds exactly as the model without the keyword."""

    def __init__(self, in_channels, hidden_dim, num_classes, dropout_prob=0.3, heads=8, edge_mlp_type='MLP', *, gat_heads=1, gat_edge_weight=False,
                 gat_v2=False):
        super().__init__()
        from .scorer import get_edge_mlp
        self.edge_prob_mlp = get_edge_mlp(in_channels, hidden_dim, dropout_prob, edge_mlp_type)
        self.dropout_prob = dropout_prob
        self.gat_heads = int(gat_heads)
        self.gat_edge_weight = bool(gat_edge_weight)
        self.gat_v2 = bool(gat_v2)
        self.GAT = GAT(in_channels=in_channels, hidden_channels=hidden_dim, num_layers=2, out_channels=num_classes,
                       dropout=dropout_prob, act='relu', heads=self.gat_heads, edge_dim=1 if self.gat_edge_weight else None, v2=self.gat_v2)

    def forward(self, data, edge_index, edge_weight=None):
        from .utils import segment
        with segment(self, "gnn_forward"):
            return self.GAT(data.x, edge_index, edge_weight=edge_weight)


# ------------------------------------------------------------------ GIN head (model.py:165-184)
SITE_GIN = 48


class _MLP2(nn.Module):
    """torch_geometric.nn.MLP([a, b, b], act='relu', norm=None) as GIN.init_conv builds it (PyG 2.3.1, from memory):
    Linear -> ReLU -> Linear; state_dict keys `lins.0.{weight,bias}`, `lins.1.{weight,bias}`."""

    def __init__(self, a, b):
        super().__init__()
        self.lins = nn.ModuleList([nn.Linear(a, b), nn.Linear(b, b)])


class GINConv(nn.Module):
    """PyG GINConv(nn=MLP, eps=0, train_eps=False): out_i = nn((1 + eps) x_i + sum_{j -> i} x_j); `edge_weight` is not
    supported by GIN (BasicGNN calls conv(x, edge_index)).  The first Linear commutes with the sum, so the aggregation runs
    on the transformed features (hidden width instead of the input width): one SpMM with unit weights and diagonal 1 + eps."""

    def __init__(self, in_channels, out_channels, eps=0.0):
        super().__init__()
        self.nn = _MLP2(in_channels, out_channels)
        self.register_buffer("eps", torch.tensor([float(eps)]))      # state_dict key, as PyG (train_eps=False)
        self._eps = float(eps)                                       # host copy: reading the buffer would synchronise

    def forward(self, x, edge_index):
        nm = ops.sum_norm(ops.get_graph(edge_index, x.shape[0]), 1.0 + self._eps)
        l0, l1 = self.nn.lins
        h = ops.gcn_propagate(ops.linear_nobias(x, l0.weight), nm, l0.bias, ops.ACT_RELU)
        return ops.linear_nobias(h, l1.weight) + l1.bias


class GINEConv(nn.Module):
    """PyG 2.3.1 GINEConv(nn=MLP, eps=0, train_eps=False, edge_dim=1) with the edge weight as the attribute (restated from its published
    algorithm; parity with PyG itself is not fixture-pinned): out_i = nn((1 + eps) x_i + sum_{j -> i} relu(x_j + lin(w_e))), lin =
    Linear(1, in_channels).  On top of GINConv's keys it has `lin.weight` [in, 1] and `lin.bias` [in] (torch.nn.Linear's default
    initialisation).  The ReLU sits inside the sum, so the aggregation runs at the input width on its own gathering kernels
    (ops.gine_aggregate); (i, i) and duplicate edges are ordinary entries.  Without edge weights every w_e is 1."""

    def __init__(self, in_channels, out_channels, eps=0.0, edge_dim=1):
        super().__init__()
        if edge_dim != 1:
            raise ValueError(f"GINEConv: edge_dim = {edge_dim!r}: 1 (the edge weight as the attribute) is supported")
        self.in_channels, self.out_channels, self.edge_dim = in_channels, out_channels, edge_dim
        self.nn = _MLP2(in_channels, out_channels)
        self.register_buffer("eps", torch.tensor([float(eps)]))      # state_dict key, as PyG (train_eps=False)
        self._eps = float(eps)                                       # host copy: reading the buffer would synchronise
        self.lin = nn.Linear(edge_dim, in_channels)                   # after GINConv's parameters: those draw exactly as without it

    def forward(self, x, edge_index, edge_weight=None):
        """`edge_weight`: None, a float32 [n_edges] tensor, or the ops.edge_attr wrapper that both layers of a head share."""
        attr = edge_weight if isinstance(edge_weight, ops.EdgeAttr) else ops.edge_attr(ops.get_graph(edge_index, x.shape[0]), edge_weight)
        z = ops.gine_aggregate(x, attr, self.lin.weight, self.lin.bias, 1.0 + self._eps)
        l0, l1 = self.nn.lins
        h = torch.relu(ops.linear_nobias(z, l0.weight) + l0.bias)
        return ops.linear_nobias(h, l1.weight) + l1.bias


class GIN(nn.Module):
    """torch_geometric.nn.models.GIN(in, hidden, num_layers=2, out, dropout, act='relu'): conv -> relu -> dropout -> conv.  edge_dim = 1
    builds both layers as GINEConv, and `edge_weight` then reaches them as their edge attribute (edge_attr = edge_weight.view(-1, 1));
    without edge_dim it is dropped, as PyG's BasicGNN does for a conv without edge-weight support."""

    def __init__(self, in_channels, hidden_channels, num_layers, out_channels, dropout=0.0, act='relu', edge_dim=None):
        super().__init__()
        if num_layers != 2 or act != 'relu':
            raise NotImplementedError("the reference instantiates GIN(num_layers=2, act='relu')")
        if edge_dim not in (None, 1):
            raise ValueError(f"GIN: edge_dim = {edge_dim!r}: None and 1 (the edge weight as the attribute) are supported")
        self.dropout, self.edge_dim = dropout, edge_dim
        if edge_dim is None:
            self.convs = nn.ModuleList([GINConv(in_channels, hidden_channels), GINConv(hidden_channels, out_channels)])
        else:
            self.convs = nn.ModuleList([GINEConv(in_channels, hidden_channels, edge_dim=edge_dim),
                                        GINEConv(hidden_channels, out_channels, edge_dim=edge_dim)])

    def forward(self, x, edge_index, edge_weight=None):
        # one wrapper of the weights for both layers: one autograd edge back to them
        edge = () if self.edge_dim is None else (ops.edge_attr(ops.get_graph(edge_index, x.shape[0]), edge_weight),)
        h = F.relu(self.convs[0](x, edge_index, *edge))
        p = self.dropout if self.training else 0.0
        if p > 0:
            keep = ops.dropout_keep(_DropoutClock.next_seed(), SITE_GIN, h.shape[0], h.shape[1], p, h.device)
            h = h * keep / (1.0 - p)
        return self.convs[1](h, edge_index, *edge)


class GINModel(nn.Module):
    """model.py:165-184.  The keyword-only `gin_edge_weight=True` builds GIN(..., edge_dim=1): both layers are GINEConv, the sampled edge
    weights enter the messages and receive the task gradient (default False = the reference's model, which drops them: same state_dict
    keys, same dropout-seed accounting, bitwise the same logits as the model without the keyword)."""

    def __init__(self, in_channels, hidden_dim, num_classes, dropout_prob=0.3, edge_mlp_type='MLP', *, gin_edge_weight=False):
        super().__init__()
        from .scorer import get_edge_mlp
        self.edge_prob_mlp = get_edge_mlp(in_channels, hidden_dim, dropout_prob, edge_mlp_type)
        self.dropout_prob = dropout_prob
        self.gin_edge_weight = bool(gin_edge_weight)
        self.GIN = GIN(in_channels=in_channels, hidden_channels=hidden_dim, num_layers=2, out_channels=num_classes,
                       dropout=dropout_prob, act='relu', edge_dim=1 if self.gin_edge_weight else None)

    def forward(self, data, edge_index, edge_weight=None):
        from .utils import segment
        with segment(self, "gnn_forward"):
            return self.GIN(data.x, edge_index, edge_weight=edge_weight)


# ------------------------------------------------------------------ Chebyshev head (model.py:211-230)
class ChebConv(nn.Module):
    """PyG 2.3.1 ChebConv(in, out, K, normalization='sym') with lambda_max = 2 (PyG's default for 'sym'; restated, not fixture-pinned):
    out = sum_{k<K} T_k(L_hat) x W_k^T + bias, T_0 = x, T_1 = L_hat x, T_k = 2 L_hat T_{k-1} - T_{k-2}.  Keys: `lins.{k}.weight` [out, in]
    (glorot, no bias), `bias` [out] (zeros).  K = 1 is what the reference instantiates: only T_0 is used, out = lins[0](x) + bias, and
    edge_index / edge_weight do not influence the output (kept in the signature).  2 <= K <= 8 runs the fused recurrence
    (ops.cheb_conv), where the edge weights reach the output and receive a gradient."""

    def __init__(self, in_channels, out_channels, K=1, normalization='sym'):
        super().__init__()
        K = int(K)
        if not 1 <= K <= 8:
            raise ValueError(f"ChebConv: K = {K}: 1 <= K <= 8 is supported")
        if normalization != 'sym':
            raise NotImplementedError(f"ChebConv: normalization = {normalization!r}: only 'sym' is built")
        self.in_channels, self.out_channels, self.K, self.normalization = in_channels, out_channels, K, normalization
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        self.bias = nn.Parameter(torch.zeros(out_channels))
        a = math.sqrt(6.0 / (in_channels + out_channels))            # glorot, as PyG's Linear(weight_initializer='glorot')
        for lin in self.lins:
            nn.init.uniform_(lin.weight, -a, a)

    def forward(self, x, edge_index=None, edge_weight=None, *, norm=None, act=ops.ACT_NONE, p=0.0, seed=0, site=0):
        if self.K == 1:
            if norm is not None or act != ops.ACT_NONE or p != 0.0:
                raise ValueError("ChebConv: K = 1 is a plain Linear: it has no normalisation and no fused activation / dropout epilogue")
            return ops.linear_nobias(x, self.lins[0].weight) + self.bias
        if norm is None:
            norm = ops.cheb_norm(ops.get_graph(edge_index, x.shape[0]), edge_weight)
        Wcat = torch.cat([lin.weight for lin in self.lins], 0)       # [K out, in]: one product for all orders
        return ops.cheb_conv(x, Wcat, self.bias, norm, self.K, act=act, p=p, seed=seed, site=site)


class ChebModel(nn.Module):
    """model.py:211-230.  The keyword-only `cheb_k` is the Chebyshev order of both layers (default 1 = the reference's model, in which
    the graph never enters); with cheb_k >= 2 the sampled subgraph and its edge weights reach the logits through message passing."""

    def __init__(self, in_channels, hidden_dim, num_classes, dropout_prob=0.3, edge_mlp_type='MLP', *, cheb_k=1):
        super().__init__()
        from .scorer import get_edge_mlp
        self.edge_prob_mlp = get_edge_mlp(in_channels, hidden_dim, dropout_prob, edge_mlp_type)
        self.dropout_prob = dropout_prob
        self.cheb_k = int(cheb_k)
        self.gcn1 = ChebConv(in_channels, hidden_dim, K=self.cheb_k, normalization='sym')
        self.dropout = nn.Dropout(dropout_prob)
        self.gcn2 = ChebConv(hidden_dim, num_classes, K=self.cheb_k, normalization='sym')

    def forward(self, data, edge_index, edge_weight=None):
        if self.cheb_k > 1:
            return self._forward_graph(data.x, edge_index, edge_weight)
        h = F.relu(self.gcn1(data.x, edge_index, edge_weight))
        p = self.dropout.p if self.training else 0.0
        if p > 0:
            keep = ops.dropout_keep(_DropoutClock.next_seed(), SITE_GNN, h.shape[0], h.shape[1], p, h.device)
            h = h * keep / (1.0 - p)
        return self.gcn2(h, edge_index, edge_weight)

    def _forward_graph(self, x, edge_index, edge_weight):
        """cheb_k >= 2: one normalisation for both layers; ReLU and the dropout mask (the same site and seed accounting as above: one seed
        per training forward with p > 0, none otherwise) ride on the first layer's last recurrence step."""
        from .utils import segment
        with segment(self, "gnn_forward"):
            norm = ops.cheb_norm(ops.get_graph(edge_index, x.shape[0]), edge_weight)
            p = self.dropout.p if self.training else 0.0
            seed = _DropoutClock.next_seed() if p > 0 else 0
            h = self.gcn1(x, norm=norm, act=ops.ACT_RELU_DROPOUT if p > 0 else ops.ACT_RELU, p=p, seed=seed, site=SITE_GNN)
            return self.gcn2(h, norm=norm)
