"""fp64 CPU restatement of PyG 2.3.1's GINEConv(nn, eps=0, train_eps=False, edge_dim=1) / GIN with edge_attr = edge_weight.view(-1, 1),
from its published algorithm: the contract of the `gin_edge_weight` head (parity with PyG itself unpinned: PyG is not installed and no
fixture pins it).  Gradients come from torch autograd.

    t_e   = lin(w_e) = w_e a + b                       a = lin.weight[:, 0], b = lin.bias, lin = Linear(1, in_channels)
    z_i   = (1 + eps) x_i + sum_{e: j -> i} relu(x_j + t_e)        (i, i) and duplicate edges are ordinary entries; w None = all ones
    out_i = nn(z_i),  nn = Linear -> ReLU -> Linear

Two forms: `gine_aggregate` in edge-list form (index_add) and `gine_aggregate_dense`, written independently: the r-th parallel edge of
every (src, dst) pair goes into an [N, N] mask and weight matrix of its own and the ReLU is applied per (i, j, c).
tests/test_gine_cpu.py holds the two against each other.

The seeded inputs of tests/test_gpu_gine.py are built HERE (layer_case / head_case), so that the CPU suite can check the condition under
which an fp32 kernel can be compared at all: no pre-activation x_j[c] + t_e[c] within 1e-4 of zero (min_abs_preact), for the weights as
given and as ones.  The builders make it hold by redrawing single elements of x (a layer's input) or single columns of (a, b) (the second
layer of a head, whose input is computed) until it does -- a condition on the inputs, checked in fp64, not a tolerance."""
import torch
import torch.nn.functional as F

MARGIN = 1e-4


def _w_or_ones(w, E, dt):
    return torch.ones(E, dtype=dt) if w is None else w


def gine_aggregate(x, ei, w, a, b, diag=1.0):
    """z [N, D] in edge-list form.  x [N, D], ei [2, E] long, w [E] or None, a / b [D]."""
    src, dst = ei[0], ei[1]
    w = _w_or_ones(w, ei.shape[1], x.dtype)
    msg = F.relu(x[src] + (w[:, None] * a[None, :] + b[None, :]))
    return diag * x + torch.zeros_like(x).index_add(0, dst, msg)


def gine_aggregate_dense(x, ei, w, a, b, diag=1.0):
    """The same over dense matrices: multiplicity layer r holds the r-th occurrence (in edge order) of every (src, dst) pair."""
    N, D = x.shape
    dt = x.dtype
    E = ei.shape[1]
    w = _w_or_ones(w, E, dt)
    src, dst = ei[0], ei[1]
    seen, rank = {}, []
    for k in (dst * N + src).tolist():
        rank.append(seen.get(k, 0))
        seen[k] = rank[-1] + 1
    rank = torch.tensor(rank, dtype=torch.long)
    rows = [diag * x[i] for i in range(N)]
    for r in range(int(rank.max()) + 1 if E else 0):
        sel = rank == r
        M = torch.zeros(N, N, dtype=dt)
        M[dst[sel], src[sel]] = 1.0
        Wd = torch.zeros(N, N, dtype=dt).index_put((dst[sel], src[sel]), w[sel])
        for i in M.sum(1).nonzero().flatten().tolist():                              # (row by row: [N, N, D] at once is only memory)
            pre = x + Wd[i][:, None] * a + b                                        # [src j, c] for destination i
            rows[i] = rows[i] + M[i] @ torch.clamp(pre, min=0.0)
    return torch.stack(rows) if N else diag * x


def gine_layer(x, ei, w, a, b, W0, b0, W1, b1, diag=1.0, aggregate=gine_aggregate):
    z = aggregate(x, ei, w, a, b, diag)
    return F.relu(z @ W0.t() + b0) @ W1.t() + b1


def min_abs_preact(x, ei, w, a, b):
    """min over entries and columns of |x_j[c] + w_e a[c] + b[c]| (inf without entries)."""
    if ei.shape[1] == 0:
        return float("inf")
    w = _w_or_ones(w, ei.shape[1], x.dtype)
    return float((x[ei[0]] + (w[:, None] * a[None, :] + b[None, :])).abs().min())


def gine_model(P, x, ei, w, keep=None, p=0.0, prefix="GIN.convs.", aggregate=gine_aggregate, hidden_out=None):
    """The two-layer head from a state_dict-like mapping P (fp64; GINModel(gin_edge_weight=True)'s keys): conv -> relu -> dropout -> conv.
    keep: the [N, hidden] dropout mask (absent = none).  hidden_out: a list that receives the second layer's input."""
    def conv(l, h):
        g = lambda k: P[f"{prefix}{l}.{k}"]
        return gine_layer(h, ei, w, g("lin.weight")[:, 0], g("lin.bias"), g("nn.lins.0.weight"), g("nn.lins.0.bias"), g("nn.lins.1.weight"),
                          g("nn.lins.1.bias"), aggregate=aggregate)
    h = F.relu(conv(0, x))
    if keep is not None:
        h = h * keep.to(h.dtype) / (1.0 - p)
    if hidden_out is not None:
        hidden_out.append(h.detach())
    return conv(1, h)


# ---------------------------------------------------------------------------------------------------- the dropout mask, restated
_M64, _M32 = (1 << 64) - 1, (1 << 32) - 1


def dropout_keep_host(seed, site, rows, cols, p):
    """sgs_dropout_keep (csrc/sgs_common.h: dropout_row_key / dropout_pair_bits, integer only) -> bool [rows, cols]."""
    th = min(max(int(p * 65536.0 + 0.5), 0), 65535)
    out = torch.zeros(rows, cols, dtype=torch.bool)
    for r in range(rows):
        z = (seed ^ ((0x9E3779B97F4A7C15 * (site + 1)) & _M64)) & _M64
        z = ((z ^ r) * 0xD6E8FEB86659FD93) & _M64
        z ^= z >> 33; z = (z * 0xff51afd7ed558ccd) & _M64
        z ^= z >> 33; z = (z * 0xc4ceb9fe1a85ec53) & _M64
        z ^= z >> 33
        rk = z >> 32
        for c in range(cols):
            pair = c >> 1
            h = rk ^ (((pair >> 1) * 0x9E3779B1) & _M32)
            h ^= h >> 16; h = (h * 0x85EBCA6B) & _M32
            h ^= h >> 13; h = (h * 0xC2B2AE35) & _M32
            h ^= h >> 16
            if pair & 1:
                h = (h * 0x9E3779B1) & _M32
                h ^= h >> 16
            out[r, c] = ((h >> 16) if (c & 1) else (h & 0xFFFF)) >= th
    return out


# ---------------------------------------------------------------------------------------------------- seeded inputs
# (N, E, D_in, D_out); "star": N = 800, D = 33, node 0 with 700 in-edges, node 1 with 700 out-edges, 500 random edges (long rows in both
# orientations next to short ones).  The last case has 500 entries per row: the 16-waves-per-row kernels (nnz >= 256 N).
LAYER_CASES = [(1, 0, 4, 3), (7, 0, 5, 5), (50, 400, 7, 6), (120, 2500, 41, 16), (64, 3000, 602, 32), (300, 6000, 256, 5), "star",
               (8, 4000, 70, 9)]


def case_id(c):
    return c if isinstance(c, str) else "N{}_E{}_D{}_O{}".format(*c)


def _edges(case, g):
    if case == "star":
        N, D, O = 800, 33, 8
        hub_in = torch.stack([torch.randint(0, N, (700,), generator=g), torch.zeros(700, dtype=torch.long)])
        hub_out = torch.stack([torch.ones(700, dtype=torch.long), torch.randint(0, N, (700,), generator=g)])
        ei = torch.cat([hub_in, hub_out, torch.randint(0, N, (2, 500), generator=g)], 1)
        return N, D, O, ei[:, torch.randperm(ei.shape[1], generator=g)]
    N, E, D, O = case
    ei = torch.randint(0, N, (2, E), generator=g)
    if E >= 8:
        ei[:, 1] = ei[:, 0]                     # a duplicate edge
        ei[1, 2] = ei[0, 2]                     # an (i, i) edge
        ei[:, 3] = ei[:, 2]                     # ... twice
    return N, D, O, ei


def _condition_x(x, ei, w, a, b, g):
    """Redraw the elements x[j, c] that put a pre-activation of an out-edge of j within MARGIN of zero (weights as given or ones)."""
    E = ei.shape[1]
    if E == 0:
        return x
    x64, a64, b64 = x.double(), a.double(), b.double()
    ts = [w.double()[:, None] * a64 + b64, a64 + b64]
    for _ in range(200):
        bad = torch.zeros_like(x, dtype=torch.bool)
        for t in ts:
            t = t if t.dim() == 2 else t[None, :].expand(E, -1)
            v = (x64[ei[0]] + t).abs() <= 2 * MARGIN
            bad.index_put_((ei[0][:, None].expand_as(v)[v], torch.arange(x.shape[1])[None, :].expand_as(v)[v]), torch.tensor(True))
        n = int(bad.sum())
        if n == 0:
            return x
        x = x.clone()
        x[bad] = torch.randn(n, generator=g)
        x64 = x.double()
    raise AssertionError("could not condition x")


def layer_case(case):
    """Seeded fp32 inputs and parameters of one GINEConv comparison (CPU tensors)."""
    g = torch.Generator().manual_seed(1234 + (len(case) if isinstance(case, str) else sum(case)))
    N, D, O, ei = _edges(case, g)
    E = ei.shape[1]
    w = torch.rand(E, generator=g) * 0.9 + 0.05
    a, b = torch.rand(D, generator=g) * 2 - 1, torch.rand(D, generator=g) * 2 - 1          # Linear(1, D)'s default range
    x = _condition_x(torch.randn(N, D, generator=g), ei, w, a, b, g)
    k0, k1 = D ** -0.5, O ** -0.5
    return dict(N=N, E=E, D=D, O=O, ei=ei, x=x, w=w, a=a, b=b,
                W0=(torch.rand(O, D, generator=g) * 2 - 1) * k0, b0=(torch.rand(O, generator=g) * 2 - 1) * k0,
                W1=(torch.rand(O, O, generator=g) * 2 - 1) * k1, b1=(torch.rand(O, generator=g) * 2 - 1) * k1,
                gy=torch.randn(N, O, generator=g))


HEAD = dict(N=120, E=2500, F=12, H=64, C=5)


DROPOUT_SEED, DROPOUT_P = 5, 0.3        # the head's dropout case: set_dropout_seed(DROPOUT_SEED), the first forward's mask


def head_case(keeps=(None,), first_lin_zero=False):
    """Seeded inputs and a state dict (fp32, CPU) of the two-layer head comparison.  `keeps`: the dropout masks (None = no dropout) under
    which the second layer's input is formed; the second layer's (a, b) columns are redrawn until the input condition holds under all.
    first_lin_zero: the first layer's lin is zero and x > 0 (its messages are x_j itself and its share of d w is exactly zero)."""
    g = torch.Generator().manual_seed(77)
    N, E, Fi, H, C = (HEAD[k] for k in ("N", "E", "F", "H", "C"))
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[:, 1] = ei[:, 0]
    ei[1, 2] = ei[0, 2]
    w = torch.rand(E, generator=g) * 0.9 + 0.05
    u = lambda *s, k=1.0: (torch.rand(*s, generator=g) * 2 - 1) * k
    P = {}
    for l, (i, o) in enumerate(((Fi, H), (H, C))):
        pre = f"GIN.convs.{l}."
        P[pre + "nn.lins.0.weight"], P[pre + "nn.lins.0.bias"] = u(o, i, k=i ** -0.5), u(o, k=i ** -0.5)
        P[pre + "nn.lins.1.weight"], P[pre + "nn.lins.1.bias"] = u(o, o, k=o ** -0.5), u(o, k=o ** -0.5)
        P[pre + "lin.weight"], P[pre + "lin.bias"] = u(i, 1), u(i)
    if first_lin_zero:
        P["GIN.convs.0.lin.weight"].zero_()
        P["GIN.convs.0.lin.bias"].zero_()
        x = torch.rand(N, Fi, generator=g) * 2 + 0.05
    else:
        x = _condition_x(torch.randn(N, Fi, generator=g), ei, w, P["GIN.convs.0.lin.weight"][:, 0], P["GIN.convs.0.lin.bias"], g)
    P64 = lambda: {k: v.double() for k, v in P.items()}
    for _ in range(200):
        bad = torch.zeros(H, dtype=torch.bool)
        for keep in keeps:
            for ww in (w.double(), None):
                hs = []
                gine_model(P64(), x.double(), ei, ww, keep=keep, p=DROPOUT_P, hidden_out=hs)
                a1, b1 = P["GIN.convs.1.lin.weight"][:, 0].double(), P["GIN.convs.1.lin.bias"].double()
                wv = _w_or_ones(ww, E, torch.float64)
                bad |= ((hs[0][ei[0]] + (wv[:, None] * a1 + b1)).abs() <= 2 * MARGIN).any(0)
        if not bool(bad.any()):
            return dict(ei=ei, x=x, w=w, P=P)
        n = int(bad.sum())
        P["GIN.convs.1.lin.weight"][bad, 0] = u(n)
        P["GIN.convs.1.lin.bias"][bad] = u(n)
    raise AssertionError("could not condition the second layer")
