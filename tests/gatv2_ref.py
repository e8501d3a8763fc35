"""fp64 CPU restatement of PyG 2.3.1's GATv2Conv(in, C, heads=K, concat, negative_slope=0.2, dropout, edge_dim in {None, 1},
share_weights=False, bias=True) / GAT(..., v2=True) with edge_attr = edge_weight.view(-1, 1), from its published algorithm: the contract of
the `gat_v2` head (parity with PyG itself unpinned: PyG is not installed and no fixture pins it).  Gradients come from torch autograd.

    x_l = lin_l(x), x_r = lin_r(x): two Linears with bias, viewed [N, K, C]
    remove_self_loops -> add_self_loops(fill_value='mean'): loop i carries the mean attribute of the remaining edges INTO i (0 without any)
    s(e) = x_l[src_e] + x_r[dst_e] (+ lin_edge(attr_e).view(K, C));   logit(e, h) = sum_c att[h, c] leaky_relu(s(e)[h, c])
    alpha = softmax per (destination, head), / (sum + 1e-16); attention dropout on alpha; out = sum alpha x_l[src] (+ bias), concat / mean

Two forms: `gatv2_layer` in edge-list form (parallel edges are entries of their own) and `gatv2_layer_dense`, written independently: the
r-th parallel edge of every (src, dst) pair goes into an [N, N] matrix of its own, the loops into a diagonal one, and the softmax runs over
the concatenated columns.  tests/test_gatv2_cpu.py holds the two against each other."""
import torch
import torch.nn.functional as F


def gatv2_layer(x, ei, w, Wl, bl, Wr, br, att, bias, lin_edge, K, C, concat, slope=0.2, keep_e=None, keep_l=None, p=0.0):
    """x [N, F], ei [2, E] (long), w [E] or None, Wl / Wr [K C, F], bl / br [K C], att [K, C], lin_edge [K C, 1] (ignored when w is None:
    PyG's `if edge_attr is not None`); keep_e [E, K] / keep_l [N, K]: attention-dropout masks by edge id / node, scaled 1 / (1 - p)."""
    N = x.shape[0]
    dt = x.dtype
    xl, xr = (x @ Wl.t() + bl).view(N, K, C), (x @ Wr.t() + br).view(N, K, C)
    nl = ei[0] != ei[1]
    src, dst = ei[0][nl], ei[1][nl]
    loops = torch.arange(N)
    src_all, dst_all = torch.cat([src, loops]), torch.cat([dst, loops])
    s = xl[src_all] + xr[dst_all]
    if w is not None:
        we = w[nl]
        cnt = torch.zeros(N, dtype=dt).index_add_(0, dst, torch.ones(src.numel(), dtype=dt))
        wbar = torch.zeros(N, dtype=dt).index_add(0, dst, we) / cnt.clamp(min=1.0)       # scatter(..., reduce='mean'): 0 where empty
        attr = torch.cat([we, wbar]).view(-1, 1)
        s = s + (attr @ lin_edge.t()).view(-1, K, C)
    logit = (F.leaky_relu(s, slope) * att).sum(-1)                                       # [entries, K]
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


def gatv2_layer_dense(x, ei, w, Wl, bl, Wr, br, att, bias, lin_edge, K, C, concat, slope=0.2, keep_e=None, keep_l=None, p=0.0):
    """The same layer over dense matrices.  Parallel edges may carry different weights, so the r-th occurrence of a (src, dst) pair (in
    edge order) is an entry of the r-th [N, N] multiplicity layer; the added loops are the identity layer.  Per head the softmax of row i
    runs over all layers' columns at once."""
    N = x.shape[0]
    dt = x.dtype
    xl, xr = F.linear(x, Wl, bl).view(N, K, C), F.linear(x, Wr, br).view(N, K, C)
    nl = (ei[0] != ei[1]).nonzero().flatten()
    src, dst = ei[0][nl], ei[1][nl]
    key = (dst * N + src).tolist()
    seen, rank = {}, []
    for k in key:
        rank.append(seen.get(k, 0))
        seen[k] = rank[-1] + 1
    rank = torch.tensor(rank, dtype=torch.long)
    R = int(rank.max()) + 1 if rank.numel() else 0
    S = xl[None, :, :, :] + xr[:, None, :, :]                                          # [dst, src, K, C]
    le = lin_edge.view(K, C) if w is not None else None
    base = None if w is not None else (F.leaky_relu(S, slope) * att).sum(-1)             # without weights every layer has the same logits
    ninf = float("-inf")
    blocks, keeps = [], []
    mult, wsum = torch.zeros(N, N, dtype=dt), torch.zeros(N, N, dtype=dt)
    for r in range(R):
        sel = rank == r
        M = torch.zeros(N, N, dtype=torch.bool)
        M[dst[sel], src[sel]] = True
        mult = mult + M.to(dt)
        if w is not None:
            Wd = torch.zeros(N, N, dtype=dt).index_put((dst[sel], src[sel]), w[nl][sel])
            wsum = wsum + Wd
            logit = (F.leaky_relu(S + Wd[:, :, None, None] * le, slope) * att).sum(-1)
        else:
            logit = base
        blocks.append(logit.masked_fill(~M[:, :, None], ninf))
        if keep_e is not None:
            Kd = torch.zeros(N, N, K, dtype=dt)
            Kd[dst[sel], src[sel]] = keep_e[nl][sel].to(dt)
            keeps.append(Kd)
    s_loop = xl + xr
    if w is not None:
        wbar = wsum.sum(1) / mult.sum(1).clamp(min=1.0)
        s_loop = s_loop + wbar[:, None, None] * le
    l_loop = (F.leaky_relu(s_loop, slope) * att).sum(-1)                                 # [N, K]
    eye = torch.eye(N, dtype=torch.bool)
    blocks.append(torch.where(eye[:, :, None], l_loop[:, None, :].expand(N, N, K), torch.full((), ninf, dtype=dt)))
    alpha = torch.softmax(torch.cat(blocks, dim=1), dim=1)                               # [N, (R + 1) N, K]
    if keep_e is not None:
        keeps.append(torch.diag_embed(keep_l.to(dt).t()).permute(1, 2, 0))
        alpha = alpha * torch.cat(keeps, dim=1) / (1.0 - p)
    a = alpha.view(N, R + 1, N, K).sum(1)                                                # messages of parallel entries share x_l[src]
    out = torch.einsum("dsk,skc->dkc", a, xl)
    out = out.reshape(N, K * C) if concat else out.mean(1)
    return out + bias


def gatv2_model(P, x, ei, w, K, hidden, ncls, masks=None, p=0.0, prefix="GAT.convs.", layer=gatv2_layer):
    """The two-layer head from a state_dict-like mapping P (fp64 tensors; GATModel(gat_v2=True)'s keys): conv 0 concat -> relu -> dropout ->
    conv 1 mean.  masks: {"e0", "l0", "e1", "l1", "h"} from ops.dropout_keep (absent = no dropout at that site)."""
    m = masks or {}
    C0 = hidden // K

    def conv(l, h, C, concat):
        g = lambda k: P[f"{prefix}{l}.{k}"]
        le = g("lin_edge.weight") if w is not None else None
        return layer(h, ei, w, g("lin_l.weight"), g("lin_l.bias"), g("lin_r.weight"), g("lin_r.bias"), g("att").reshape(K, C), g("bias"), le, K, C,
                     concat, keep_e=m.get(f"e{l}"), keep_l=m.get(f"l{l}"), p=p)
    h = F.relu(conv(0, x, C0, True))
    if "h" in m:
        h = h * m["h"].to(h.dtype) / (1.0 - p)
    return conv(1, h, ncls, False)


# the shapes both test files add to test_gpu_gat_heads.CASES, (N, E, Fin, K, C, concat): one head, C % 4 != 0 (3, 5, 65), E = 0,
# in- and out-degree >> 64 (150 at N = 40), C above one lane-group stride (K = 16, C = 65: 4 lanes per head)
EXTRA_CASES = [(30, 200, 7, 1, 16, True), (200, 5000, 20, 1, 64, False), (25, 0, 4, 1, 3, True), (40, 6000, 6, 1, 5, True),
               (20, 150, 5, 16, 65, False)]
