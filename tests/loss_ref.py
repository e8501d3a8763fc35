"""fp64 CPU restatement of the learned step's loss chain (csrc/losses.hip: the masked cross entropy, the two edge regularisers, their fused
form `hybrid_loss`, the gate's argmax counts) and the seeded inputs of tests/test_gpu_loss_chain.py.  Plain torch on the CPU; nothing here
imports the product or oracle/.

    ce    = mean over train rows of (lse_i - logits[i, y_i]),  lse_i = max_i + log sum_c exp(logits[i, c] - max_i);   0/0 = nan
            d logits[i, c] = (exp(logits[i, c] - lse_i) - [c = y_i]) g / #train on train rows
    cos_j = <x, y> / sqrt(max(|x|^2 |y|^2, 1e-16)),  x = logits[src_j], y = logits[dst_j]          (the kernel's documented clamp: the
            form of torch 2.0's F.cosine_similarity; while the clamp is active the denominator is a constant, d cos / d x = y 1e8)
            d cos / d x = y inv - cos x / |x|^2,  inv = 1 / sqrt(max(...))
    reg2  = sum_j (w_j - cos_j)^2 / q_global
    reg1  = mean over valid edges (both endpoints train rows) of BCE(w_j, [y_src = y_dst]) with each log clamped at -100, taken only when
            sum of labels > 1 (strictly); backward (w - t) / max((1 - w) w, 1e-12) / #valid (torch's own BCE backward)
    out   = [reg1, reg2, #valid, sum labels, c1 reg1 + c2 reg2, ce, ce + c1 reg1 + c2 reg2]
    d logits += scatter-add of the per-edge rows Gs_j = -r_j d cos_j / d x at src_j and Gd_j at dst_j, r_j = 2 (w_j - cos_j) c2 g / q_global
            (a self-loop adds both rows to its node; duplicate edges accumulate)

Two independent forms: `closed_form` (the formulas above written out, in any dtype: fp64 is the reference, fp32 its error model) and
`autograd_form` (torch.logsumexp, F.binary_cross_entropy and autograd, fp64).  tests/test_loss_ref_cpu.py holds them against each other
and against oracle/; `closed_form(mut=...)` carries the single-term faults whose visibility that file proves.

Bounds are not constants: `bound(ref64, ref32)` = 8 x the largest deviation of the fp32 evaluation of the closed form from the fp64 one
plus 4 ulp (fp32) at the quantity's largest magnitude.  The 8 covers another legitimate fp32 summation order and the device's expf / logf
against torch's CPU routines."""
import math

import torch
import torch.nn.functional as F

EPS2 = float(torch.tensor(1e-16, dtype=torch.float32))        # the kernel's constants are fp32 literals (1e-16f, 1e-12f): their values, not
EPS_BCE = float(torch.tensor(1e-12, dtype=torch.float32))     # the decimal ones, are the function's (torch's own BCE backward clamps at 1e-12f too)
G = 2.5                      # the upstream gradient of every comparison: backward runs through (loss * G)
MUTATIONS = ("ge1", "loop_one_row", "local_q", "no_g")          # + "last_max" in argmax_counts


# ---------------------------------------------------------------------------------------------------- bounds
def ulp32(x):
    """Spacing of fp32 at |x| (the smallest normal's for 0)."""
    x = abs(float(x))
    if x == 0.0 or math.isnan(x) or math.isinf(x):
        return 2.0 ** -149
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


def bound(ref64, ref32):
    a, b = torch.as_tensor(ref64, dtype=torch.float64), torch.as_tensor(ref32).double()
    if a.numel() == 0:
        return 0.0
    ok = ~torch.isnan(a)
    if not bool(ok.any()):
        return 0.0
    return 8.0 * float((a - b)[ok].abs().max()) + 4.0 * ulp32(a[ok].abs().max())


# ---------------------------------------------------------------------------------------------------- closed form
def closed_form(c, dtype=torch.float64, g=G, mut=None, q_div=None):
    """Every quantity of the chain for case `c` (make_case) in `dtype`, all intermediates in that dtype.  q_div: the divisor of reg2 and
    of its gradient (q_global; default the case's q).  Returns a dict of tensors; out7 as above; Gs / Gd the per-edge rows."""
    dt = dtype
    L, w = c["logits"].to(dt), c["w"].to(dt)
    y, mask, sei = c["y"], c["mask"], c["sei"]
    N, C = L.shape
    q = w.numel()
    c1, c2 = torch.tensor(c["c1"], dtype=dt), torch.tensor(c["c2"], dtype=dt)
    gt = torch.tensor(1.0 if mut == "no_g" else g, dtype=dt)
    one, zero = torch.ones((), dtype=dt), torch.zeros((), dtype=dt)
    # ---- cross entropy
    mx = L.max(1).values
    lse = mx + torch.log(torch.exp(L - mx[:, None]).sum(1))
    rows = torch.arange(N)
    rowloss = torch.where(mask, lse - L[rows, y], zero)
    ntrain = mask.sum().to(dt)
    ce = rowloss.sum() / ntrain
    onehot = torch.zeros(N, C, dtype=dt)
    onehot[rows, y] = 1.0
    dce = torch.where(mask[:, None], (torch.exp(L - lse[:, None]) - onehot) * (gt / ntrain), zero)
    # ---- per-edge terms
    s, d = sei[0], sei[1]
    x, yv = L[s], L[d]
    dot, nx, ny = (x * yv).sum(1), (x * x).sum(1), (yv * yv).sum(1)
    eps2 = torch.tensor(EPS2, dtype=dt)
    clamped = nx * ny < eps2
    inv = one / torch.sqrt(torch.maximum(nx * ny, eps2))
    cos = dot * inv
    valid = mask[s] & mask[d]
    same = y[s] == y[d]
    t = same.to(dt)
    nvalid, lsum = valid.sum().to(dt), (valid & same).sum().to(dt)
    m100 = torch.tensor(-100.0, dtype=dt)
    bce = torch.where(same, -torch.maximum(torch.log(w), m100), -torch.maximum(torch.log(one - w), m100))
    raw = torch.stack([bce[valid].sum() if q else zero, ((w - cos) ** 2).sum(), nvalid, lsum])
    on = bool(lsum >= 1) if mut == "ge1" else bool(lsum > 1)
    qd = torch.tensor(float(q if (q_div is None or mut == "local_q") else q_div), dtype=dt)
    reg1 = raw[0] / nvalid if on else zero
    reg2 = raw[1] / qd
    tot = c1 * reg1 + c2 * reg2
    out7 = torch.stack([reg1, reg2, nvalid, lsum, tot, ce, ce + tot])
    # ---- backward
    r = 2.0 * (w - cos) / qd * c2 * gt
    dw = r.clone()
    sat = torch.zeros(q, dtype=torch.bool)
    if c["c1"] != 0.0 and on:
        dw = dw + torch.where(valid, c1 * gt * (w - t) / torch.maximum((one - w) * w, torch.tensor(EPS_BCE, dtype=dt)) / nvalid, zero)
        sat = valid & ((c["w"] == 0.0) | (c["w"] == 1.0))
    safe = lambda n: torch.where(clamped, one, n)                                           # noqa: E731
    cx, cy = torch.where(clamped, zero, cos / safe(nx)), torch.where(clamped, zero, cos / safe(ny))
    Gs = -r[:, None] * (yv * inv[:, None] - cx[:, None] * x)
    Gd = -r[:, None] * (x * inv[:, None] - cy[:, None] * yv)
    dreg = torch.zeros(N, C, dtype=dt).index_add_(0, s, Gs)
    dreg.index_add_(0, d, Gd if mut != "loop_one_row" else torch.where((s == d)[:, None], zero, Gd))
    hot = torch.zeros(N, dtype=torch.bool)                    # rows that an edge under the clamp touches (gradients of order 1e8 r)
    hot[s[clamped]] = True
    hot[d[clamped]] = True
    return dict(out7=out7, raw=raw, row_lse=torch.where(mask, lse, zero), dlogits=dce + dreg, dw=dw, Gs=Gs, Gd=Gd, cos=cos, clamped=clamped,
                hot_rows=hot, sat=sat)


def raw_sums(c, lo, hi, dtype=torch.float64):
    """[sum bce, sum (w - cos)^2, #valid, sum labels] of the edges [lo, hi) (sgs_edge_reg_partial's output for that shard)."""
    sub = dict(c, sei=c["sei"][:, lo:hi], w=c["w"][lo:hi])
    return closed_form(sub, dtype)["raw"]


# ---------------------------------------------------------------------------------------------------- autograd form
def cos_documented(x, y):
    return (x * y).sum(-1) / torch.sqrt(torch.clamp_min((x * x).sum(-1) * (y * y).sum(-1), EPS2))


def cos_torch_now(x, y):
    """The form of the installed torch's F.cosine_similarity (each norm clamped on its own), written out."""
    return (x * y).sum(-1) / (torch.clamp_min(x.norm(dim=-1), 1e-8) * torch.clamp_min(y.norm(dim=-1), 1e-8))


def loss_autograd(L, w, c, q_div=None):
    """The loss as a differentiable fp64 expression of (L, w) -> (loss, out7 detached)."""
    y, mask, sei = c["y"], c["mask"], c["sei"]
    q = w.numel()
    ce = (torch.logsumexp(L[mask], 1) - L[mask, y[mask]]).mean()
    s, d = sei[0], sei[1]
    cos = cos_documented(L[s], L[d])
    reg2 = ((w - cos) ** 2).sum() / float(q if q_div is None else q_div)
    valid = mask[s] & mask[d]
    labels = (y[s] == y[d])[valid].to(L.dtype)
    lsum = labels.sum()
    reg1 = F.binary_cross_entropy(w[valid], labels) if float(lsum) > 1 else torch.zeros((), dtype=L.dtype)
    tot = c["c1"] * reg1 + c["c2"] * reg2
    loss = ce + tot
    out7 = torch.stack([reg1.detach(), reg2.detach(), valid.sum().to(L.dtype), lsum, tot.detach(), ce.detach(), loss.detach()])
    return loss, out7


def autograd_form(c, g=G, q_div=None):
    L = c["logits"].double().requires_grad_(True)
    w = c["w"].double().requires_grad_(True)
    loss, out7 = loss_autograd(L, w, c, q_div)
    dl, dw = torch.autograd.grad(loss * g, (L, w), allow_unused=True)
    return dict(out7=out7, dlogits=dl, dw=torch.zeros_like(w) if dw is None else dw)


# ---------------------------------------------------------------------------------------------------- gate
def argmax_first(L, last=False):
    """Index of the first (last=True: the last) maximum of every row, as integers; a row of -inf gives 0 (C - 1)."""
    N, C = L.shape
    eq = L == L.max(1, keepdim=True).values
    ar = torch.arange(C)[None, :].expand(N, C)
    return torch.where(eq, ar, torch.full_like(ar, -1)).max(1).values if last else torch.where(eq, ar, torch.full_like(ar, C)).min(1).values


def argmax_counts(L, y, mask, mut=None):
    """(#rows of the mask whose first maximum is y, #rows of the mask) as Python ints."""
    if L.shape[0] == 0:
        return 0, 0
    am = argmax_first(L.double(), last=(mut == "last_max"))
    return int(((am == y) & mask).sum()), int(mask.sum())


# ---------------------------------------------------------------------------------------------------- seeded inputs: the loss
def _edges(N, q, g):
    sei = torch.randint(0, N, (2, q), generator=g)
    loop = torch.rand(q, generator=g) < 0.05
    sei[1, loop] = sei[0, loop]                                     # ~5 % self-loops
    dup = (torch.rand(q, generator=g) < 0.05).nonzero().flatten().tolist()
    for j in dup:                                                   # ~5 % repeated columns
        if j > 0:
            sei[:, j] = sei[:, j - 1]
    return sei


def _base(N, C, q, seed, c1=1.0, c2=0.5, mask="60", scale=1.0):
    g = torch.Generator().manual_seed(seed)
    L = torch.randn(N, C, generator=g)
    L[L.norm(dim=1) < 1e-2] = 0.5                                   # ordinary inputs: every row norm >= 1e-3
    y = torch.randint(0, C, (N,), generator=g)
    m = torch.rand(N, generator=g) < 0.6
    m[0] = True
    if mask == "all":
        m[:] = True
    elif mask == "one":
        m[:] = False
        m[N // 2] = True
    elif mask == "none":
        m[:] = False
    sei = _edges(N, q, g)
    w = torch.rand(q, generator=g) * 0.98 + 0.01
    if scale != 1.0:
        L = L * scale
        if scale >= 1e3:            # saturating scale: the two largest logits of every row at least 220 apart (expf underflows below -104)
            top = L.topk(2, dim=1) if C > 1 else None
            if top is not None:
                bad = (top.values[:, 0] - top.values[:, 1]) < 220.0
                L[bad, top.indices[bad, 0]] += 440.0
    return dict(N=N, C=C, q=q, logits=L.contiguous(), y=y, mask=m, sei=sei, w=w, c1=float(c1), c2=float(c2), kind="ordinary")


def _label_sum(k):
    """Eight train rows, six edges, no self-loop, exactly k same-label valid edges (k = 0, 1, 2): reg1 off, off, on."""
    c = _base(8, 4, 6, 900 + k, mask="all")
    c["y"] = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3])
    e = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4) if k >= 1 else (0, 5), (1, 5) if k >= 2 else (1, 6)]
    c["sei"] = torch.tensor(e).t().contiguous()
    c["label_sum"] = k
    return c


def _w01():
    """w exactly 0.0 and 1.0 on valid edges of both labels: both log clamps (-100) and the max((1 - w) w, 1e-12) of the backward are hit."""
    c = _base(257, 41, 5000, 31)
    s, d = c["sei"]
    valid = c["mask"][s] & c["mask"][d]
    same = c["y"][s] == c["y"][d]
    for sel in (valid & same, valid & ~same):
        idx = sel.nonzero().flatten()
        assert idx.numel() >= 8
        c["w"][idx[0:4:2]] = 0.0
        c["w"][idx[1:4:2]] = 1.0
    c["w"][(~valid).nonzero().flatten()[:2]] = torch.tensor([0.0, 1.0])
    return c


def _clamp(big):
    """The cosine's clamp.  Row 0 is zero and row 1 is [1e-10, 0, ...]: |x|^2 |y|^2 < 1e-16 on every edge that touches them.
    big: they are paired with ordinary rows (the issue's case: the gradient rows are y 1e8 r, of order 1e7);  not big: rows 0-3 are all of
    order 1e-10 and only paired with each other, self-loops included, so that every gradient stays of order 1e-2 and a fault in the clamped
    branch is not hidden below the ulp of a 1e7."""
    c = _base(12, 3, 14, 77 if big else 78, mask="all")
    L = c["logits"]
    L[0] = 0.0
    L[1] = torch.tensor([1e-10, 0.0, 0.0])
    if big:
        e = [(0, 5), (6, 0), (1, 7), (8, 1), (0, 1), (1, 1), (0, 0)]
    else:
        L[2] = torch.tensor([2e-10, 1e-10, 0.0])
        L[3] = torch.tensor([-1e-10, 3e-10, 1e-10])
        e = [(1, 2), (2, 1), (1, 1), (2, 2), (3, 3), (2, 3), (0, 1), (1, 3)]
    rest = [(4 + i % 8, 4 + (3 * i + 1) % 8) for i in range(14 - len(e))]
    c["sei"] = torch.tensor(e + rest).t().contiguous()
    c["kind"] = "clamp"
    return c


_SPINE_C = (1, 2, 15, 16, 17, 41, 64, 65, 130)
_SPINE_Q = (1, 15, 16, 17, 63, 64, 65, 5000, 16500)
_SPINE_N = (1, 5, 257, 1030)


def _table():
    t = {}
    for C in _SPINE_C:
        t[f"N257_C{C}_q65"] = lambda C=C: _base(257, C, 65, 100 + C)
    for q in _SPINE_Q:
        t.setdefault(f"N257_C41_q{q}", lambda q=q: _base(257, 41, q, 200 + q))
    for N in _SPINE_N:
        t.setdefault(f"N{N}_C41_q5000", lambda N=N: _base(N, 41, 5000, 300 + N))
    for c1, c2 in ((0.0, 0.5), (1.0, 0.0), (0.3, 0.7)):
        t[f"coef_{c1}_{c2}"] = lambda c1=c1, c2=c2: _base(257, 41, 5000, 205200, c1, c2)       # (1, 0.5): every other case
    for m in ("all", "one", "none"):
        t[f"mask_{m}"] = lambda m=m: _base(257, 41, 5000, 401, mask=m)
    for k in (0, 1, 2):
        t[f"labelsum_{k}"] = lambda k=k: _label_sum(k)
    t["w_0_and_1"] = _w01
    t["scale_80"] = lambda: _base(257, 41, 65, 141, scale=80.0)
    t["scale_1e4"] = lambda: _base(257, 41, 65, 141, scale=1e4)
    t["clamp_big"] = lambda: _clamp(True)
    t["clamp_tiny"] = lambda: _clamp(False)
    return t


_TABLE = _table()
HYBRID_CASES = tuple(_TABLE)
SHARD_CASE, SHARDS = "N257_C41_q5000", ((0, 0), (0, 1), (1, 1984), (1984, 5000))       # shards of 0, 1, 1983 and 3016 edges
FUSED_CASES = ("N257_C41_q65", "N257_C41_q5000", "N257_C130_q65", "N1030_C41_q5000", "coef_1.0_0.0", "coef_0.0_0.5", "w_0_and_1", "mask_one")
_made = {}


def make_case(name):
    """The case's inputs (fp32 / int64 / bool CPU tensors; built once, never modified)."""
    if name not in _made:
        _made[name] = _TABLE[name]()
    return _made[name]


_refs = {}


def reference(name):
    """(fp64 closed form, fp32 closed form) of a case, computed once."""
    if name not in _refs:
        c = make_case(name)
        _refs[name] = (closed_form(c, torch.float64), closed_form(c, torch.float32))
    return _refs[name]


def quantities(ref):
    """The compared floating-point quantities of a closed-form result, split where one tensor holds magnitudes that differ by 1e7 or
    more: d w on the saturated entries (w = 0 or 1 under an active reg1: 1e12 / #valid) and d logits on the rows under the cosine's
    clamp (1e8 r) are bounded on their own, so that their ulp does not become everybody's tolerance."""
    o, sat, hot = ref["out7"], ref["sat"], ref["hot_rows"]
    return {"reg1": o[0], "reg2": o[1], "regs": o[4], "ce": o[5], "loss": o[6], "dw": ref["dw"][~sat], "dw_sat": ref["dw"][sat],
            "dlogits": ref["dlogits"][~hot], "dlogits_clamp": ref["dlogits"][hot]}


def bounds(name):
    r64, r32 = reference(name)
    a, b = quantities(r64), quantities(r32)
    return {k: bound(a[k], b[k]) for k in a}


def shard_bounds():
    """{(lo, hi): {quantity: bound}} for the edge-sharded entry points on SHARD_CASE: d w, Gs, Gd are the unsharded rows [lo, hi), the two
    floating raw sums the shard's own."""
    c = make_case(SHARD_CASE)
    r64, r32 = reference(SHARD_CASE)
    out = {}
    for lo, hi in SHARDS:
        b = {k: bound(r64[k][lo:hi], r32[k][lo:hi]) for k in ("dw", "Gs", "Gd")}
        a64, a32 = raw_sums(c, lo, hi), raw_sums(c, lo, hi, torch.float32)
        b["raw0"], b["raw1"] = bound(a64[0], a32[0]), bound(a64[1], a32[1])
        out[(lo, hi)] = b
    return out


# ---------------------------------------------------------------------------------------------------- seeded inputs: the gate
GATE_N, GATE_C = (0, 1, 15, 16, 17, 1040), (1, 41, 64, 65, 130)
_GRID = 2.0 ** -6                  # every gate logit is an integer multiple of 2^-6 below 2^10: exact in fp32, distinct columns >= 1.5e-2 apart


def gate_case(N, C):
    """Two different logit matrices whose rows are permutations of a 2^-6 grid (no two columns of a row closer than 1e-3), with planted
    exact ties: columns (3, 67) -- one lane, two iterations of the row scan --, (3, 40) -- two lanes --, (0, C - 1), a constant row and a
    row of -inf.  The label sits on the first maximum on some planted rows and on the later one on others; `ties` lists the planted rows."""
    g = torch.Generator().manual_seed(5000 + 131 * N + C)
    mk = lambda: torch.stack([torch.randperm(C, generator=g) for _ in range(N)]).float() * _GRID if N else torch.zeros(0, C)     # noqa: E731
    A, B = mk(), mk()
    y = torch.randint(0, C, (N,), generator=g)
    if N:
        half = torch.rand(N, generator=g) < 0.5                    # about half the rows are classified correctly by each matrix
        y = torch.where(half, argmax_first(A), y)
        half = torch.rand(N, generator=g) < 0.5
        y = torch.where(half, argmax_first(B), y)
    mask = torch.rand(N, generator=g) < 0.6
    plans = [p for p in (((3, 67), "pair"), ((3, 40), "pair"), ((0, C - 1), "pair"), (None, "const"), (None, "ninf")) if p[0] is None or (p[0][1] < C and p[0][0] < p[0][1])]
    ties = []
    top = C * _GRID + 1.0
    for k in range(min(N, 4 * len(plans))):                         # rows 0 .. : plan k % len, label first / later alternating per round
        cols, what = plans[k % len(plans)]
        later = (k // len(plans)) % 2 == 1
        M = A if (k // (2 * len(plans))) % 2 == 0 else B            # the tie is planted in one matrix, the other keeps its permutation
        if what == "pair":
            M[k, cols[0]] = M[k, cols[1]] = top
            y[k] = cols[1] if later else cols[0]
        elif what == "const":
            M[k] = 0.25
            y[k] = C - 1 if later else 0
        else:
            M[k] = float("-inf")
            y[k] = C - 1 if later else 0
        mask[k] = True
        ties.append((k, what, later, M is A))
    return dict(N=N, C=C, A=A.contiguous(), B=B.contiguous(), y=y, mask=mask, ties=ties)


# ---------------------------------------------------------------------------------------------------- the in-place hand-over of d w
HAND = dict(N=257, F=9, H=16, C=7, q=600)


def gcn2_dense(x, W1, b1, W2, b2, ei, w, N):
    """Two GCN layers over the dense normalised adjacency (PyG gcn_norm, add_self_loops=True): every (i, i) edge leaves the adjacency and
    gives its weight to node i's loop (1 without one), deg_i = loop_i + sum of in-edge weights, A_hat = D^-1/2 (A + diag(loop)) D^-1/2,
    out = A_hat relu(A_hat x W1^T + b1) W2^T + b2.  Differentiable in w (duplicates accumulate).  w None: unit weights.  Returns
    (out, hidden pre-activation)."""
    dt = x.dtype
    s, d = ei[0], ei[1]
    w = torch.ones(ei.shape[1], dtype=dt) if w is None else w
    off = s != d
    A = torch.zeros(N, N, dtype=dt).index_put((d[off], s[off]), w[off], accumulate=True)
    loop = torch.ones(N, dtype=dt).index_put((s[~off],), w[~off])                  # (the builders plant at most one loop per node)
    dis = (A.sum(1) + loop).pow(-0.5)
    Ah = dis[:, None] * (A + torch.diag(loop)) * dis[None, :]
    pre = Ah @ (x @ W1.t()) + b1
    return Ah @ (torch.relu(pre) @ W2.t()) + b2, pre


def hand_case(seed=0, q_loss=None, draw=False):
    """Inputs of the hand-over tests: a graph with self-loops on distinct nodes and duplicate non-loop edges, a two-layer GCN whose hidden
    pre-activations all stay 1e-4 away from zero under the weights as given AND under unit weights (the seed is advanced until they do:
    a condition on the inputs, so that no ReLU decision depends on fp32 rounding).  q_loss: a second edge list of that length for the loss."""
    N, Fi, H, C, q = (HAND[k] for k in ("N", "F", "H", "C", "q"))
    for trial in range(200):
        g = torch.Generator().manual_seed(7000 + 1000 * seed + trial)
        ei = torch.randint(0, N, (2, q), generator=g)
        ei[1] = torch.where(ei[0] == ei[1], (ei[1] + 1) % N, ei[1])
        loops = torch.randperm(N, generator=g)[:30]
        ei[:, 5:35] = loops                                         # 30 self-loops, distinct nodes
        ei[:, 40:60] = ei[:, 60:80]                                 # 20 repeated columns (no loops among them)
        u = lambda *s, k=1.0: (torch.rand(*s, generator=g) * 2 - 1) * k                        # noqa: E731
        c = dict(N=N, C=C, q=q, x=torch.randn(N, Fi, generator=g), W1=u(H, Fi, k=Fi ** -0.5 * 2), b1=u(H, k=0.5), W2=u(C, H, k=H ** -0.5 * 2),
                 b2=u(C, k=0.5), sei=ei,
                 w=torch.linspace(0.35, 0.95, q)[torch.randperm(q, generator=g)] if draw else torch.rand(q, generator=g) * 0.9 + 0.05, y=torch.randint(0, C, (N,), generator=g),
                 mask=torch.rand(N, generator=g) < 0.6, c1=1.0, c2=0.5)
        if q_loss is not None:
            c["sei_loss"] = _edges(N, q_loss, g)
        d = {k: v.double() for k, v in c.items() if torch.is_tensor(v) and v.is_floating_point()}
        pres = [gcn2_dense(d["x"], d["W1"], d["b1"], d["W2"], d["b2"], ei, ww, N)[1] for ww in (d["w"], None)]
        if min(float(p.abs().min()) for p in pres) > 1e-4:
            c["min_preact"] = min(float(p.abs().min()) for p in pres)
            return c
    raise AssertionError("could not condition the hidden layer")


DRAW_E = 3000


def draw_case(seed=3):
    """hand_case's graph as the outcome of a draw of q = 600 among E = 3000 candidates: the sampled edges are the 600 candidates with the
    largest p (their weights p itself, 0.35 ... 0.95), in edge order hand_case's list; with constant explicit noise the race is decided
    by p alone (neighbouring p differ by 3e-4: no rounding decides it).  The other 2400 candidates are random edges without loops."""
    c = dict(hand_case(seed, draw=True))
    N, q, E = c["N"], c["q"], DRAW_E
    g = torch.Generator().manual_seed(9100 + seed)
    pos = torch.randperm(E, generator=g)[:q].sort().values
    sel = torch.zeros(E, dtype=torch.bool)
    sel[pos] = True
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[1] = torch.where(ei[0] == ei[1], (ei[1] + 1) % N, ei[1])
    ei[:, pos] = c["sei"]
    p = torch.empty(E)
    p[pos] = c["w"]
    p[~sel] = (torch.linspace(0.05, 0.3, E - q))[torch.randperm(E - q, generator=g)]
    c.update(E=E, p=p, parent=ei.contiguous(), sel=sel, pos=pos, noise=torch.ones(E))
    return c


def hand_reference(c, dtype=torch.float64, g=G, model_w="w", loss_edges="sei", producer=None):
    """d (loss g) / d w of `loss_autograd` over the logits of the dense two-layer GCN, by autograd in `dtype`.
    model_w: "w" (the graph is normalised with the learned weights) or None (unit weights: the weights enter the loss only).
    loss_edges: the key of the edge list the loss reads; a list shorter than w reads w's first entries.
    producer: callable(dtype) -> (leaf, w): the weights as a differentiable function of a leaf (d w is then the gradient wrt the leaf).
    -> dict(out7, logits, dw, w)."""
    f = lambda k: c[k].to(dtype)                                                                 # noqa: E731
    leaf, w = producer(dtype) if producer is not None else (None, f("w").requires_grad_(True))
    leaf = w if leaf is None else leaf
    logits, _ = gcn2_dense(f("x"), f("W1"), f("b1"), f("W2"), f("b2"), c["sei"], w if model_w == "w" else None, c["N"])
    sei = c[loss_edges]
    L, out7 = loss_autograd(logits, w[:sei.shape[1]], dict(c, sei=sei))
    (dw,) = torch.autograd.grad(L * g, (leaf,))
    return dict(out7=out7, logits=logits.detach(), dw=dw, w=w.detach())
