"""fp64 CPU restatement of PyG 2.3.1's GATConv(..., edge_dim=1) / GAT(..., edge_dim=1) with edge_attr = edge_weight.view(-1, 1), in
edge-list form (parallel edges carry their own weights, so no dense multiplicity matrix): the contract of the `gat_edge_weight` head
(parity with PyG unpinned: PyG is not installed and no fixture pins it).  Gradients come from torch autograd.

    remove_self_loops -> add_self_loops(fill_value='mean'): loop i carries the mean attribute of the remaining edges INTO i (0 without any)
    logit(e, h) = leaky_relu(a_s[src_e, h] + a_d[dst_e, h] + ((lin_edge(attr_e).view(K, C) * att_edge).sum(-1))[h])
    alpha = softmax per (destination, head), / (sum + 1e-16); attention dropout on alpha; out = sum alpha x'[src] (+ bias), concat / mean

The edge term is computed the way PyG writes it (a [E, K C] product), NOT as w_e * c_h: the collapse is what the kernels rely on and this
file is what checks it."""
import torch
import torch.nn.functional as F


def gat_edge_layer(x, ei, w, W, att_s, att_d, bias, lin_edge, att_edge, K, C, concat, slope=0.2, keep_e=None, keep_l=None, p=0.0):
    """x [N, F], ei [2, E] (long), w [E] or None, W [K C, F], att_* [K, C], lin_edge [K C, 1], att_edge [K, C] (both ignored when w is
    None: PyG's `if edge_attr is not None`); keep_e [E, K] / keep_l [N, K]: attention-dropout masks by edge id / node, scaled 1 / (1 - p)."""
    N = x.shape[0]
    dt = x.dtype
    xl = (x @ W.t()).view(N, K, C)
    a_s, a_d = (xl * att_s).sum(-1), (xl * att_d).sum(-1)                         # [N, K]
    nl = ei[0] != ei[1]
    src, dst = ei[0][nl], ei[1][nl]
    loops = torch.arange(N)
    src_all, dst_all = torch.cat([src, loops]), torch.cat([dst, loops])
    logit = a_s[src_all] + a_d[dst_all]
    if w is not None:
        we = w[nl]
        cnt = torch.zeros(N, dtype=dt).index_add_(0, dst, torch.ones(src.numel(), dtype=dt))
        wbar = torch.zeros(N, dtype=dt).index_add(0, dst, we) / cnt.clamp(min=1.0)       # scatter(..., reduce='mean'): 0 where empty
        attr = torch.cat([we, wbar]).view(-1, 1)
        logit = logit + ((attr @ lin_edge.t()).view(-1, K, C) * att_edge).sum(-1)
    logit = F.leaky_relu(logit, slope)
    idx = dst_all[:, None].expand(-1, K)
    mx = torch.full((N, K), float("-inf"), dtype=dt).scatter_reduce(0, idx, logit.detach(), "amax", include_self=True)
    ex = torch.exp(logit - mx[dst_all])
    den = torch.zeros(N, K, dtype=dt).index_add(0, dst_all, ex)
    alpha = ex / (den[dst_all] + 1e-16)
    if keep_e is not None:
        alpha = alpha * torch.cat([keep_e[nl], keep_l]).to(dt) / (1.0 - p)
    out = torch.zeros(N, K, C, dtype=dt).index_add(0, dst_all, alpha[:, :, None] * xl[src_all])
    out = out.reshape(N, K * C) if concat else out.mean(1)
    return out + bias


def gat_edge_model(P, x, ei, w, K, hidden, ncls, masks=None, p=0.0, prefix="GAT.convs."):
    """The two-layer head from a state_dict-like mapping P (fp64 tensors; GATModel's keys): conv 0 concat -> relu -> dropout -> conv 1 mean.
    masks: {"e0", "l0", "e1", "l1", "h"} from ops.dropout_keep (absent = no dropout at that site)."""
    m = masks or {}
    C0 = hidden // K

    def conv(l, h, C, concat):
        g = lambda k: P[f"{prefix}{l}.{k}"]
        le = g("lin_edge.weight") if w is not None else None
        ae = g("att_edge").reshape(K, C) if w is not None else None
        return gat_edge_layer(h, ei, w, g("lin_src.weight"), g("att_src").reshape(K, C), g("att_dst").reshape(K, C), g("bias"), le, ae, K, C,
                              concat, keep_e=m.get(f"e{l}"), keep_l=m.get(f"l{l}"), p=p)
    h = F.relu(conv(0, x, C0, True))
    if "h" in m:
        h = h * m["h"].to(h.dtype) / (1.0 - p)
    return conv(1, h, ncls, False)
