"""fp64 CPU restatement of the class-weighted, label-smoothed masked cross entropy (csrc/losses.hip: ce_rows<true>, ce_final<true>,
ce_bwd<true, false> / ce_bwd<true, true>, hybrid_loss_final<true>) and the seeded case table of tests/test_ce_weighted_cpu.py and
tests/test_gpu_ce_weighted.py.  Plain torch on the CPU; nothing here imports the product.

The definition of correct is F.cross_entropy(logits[mask], y[mask], weight=w, label_smoothing=eps, reduction="mean") in fp64
(`torch_form`).  `closed_form` writes it out; w_c = 1 without a weight, W = sum_c w_c, lse_i = logsumexp_c x_ic:

    row_i  = (1 - eps) w[y_i] (lse_i - x_i[y_i]) + (eps / C) (W lse_i - sum_c w_c x_ic)        train rows; 0 elsewhere
    den    = sum over train rows of w[y_i]
    loss   = sum_i row_i / den                                      nan when den = 0
    dx_ic  = g / den [ (1 - eps) w[y_i] (softmax_ic - [c = y_i]) + (eps / C) (W softmax_ic - w_c) ]      train rows; 0 elsewhere
                                                                    nan on every train row when den = 0

The two den = 0 rules are torch's, not those of the bare quotient: torch forms the two terms' means separately, so with den = 0 the hard
term is 0 / 0 = nan whatever the smoothing term is (the bare quotient would give +inf for eps > 0 when another class carries weight), and
its backward puts -w[y_i] g / den = nan into the label's column of every train row, which log_softmax's backward spreads over the row
(the bare quotient would give +-inf or nan entry by entry).  Without a train row there is no row to receive a gradient: d x = 0.

`closed_form(c, torch.float32)` is the error model of loss_ref.bound, as in tests/loss_ref.py.  It is the form above as stated;
`form="kernel"` writes the smoothing term as sum_c w_c (lse - x_c), the way ce_rows<true> sums it.  tests/test_ce_weighted_cpu.py shows that
the two fp32 evaluations give the same bound on every case, the logits x 80 ones included (W lse - sum_c w_c x_c is of the order of W lse
itself there: nothing cancels), so the stated form does not loosen the bound for the kernel.  `block_shares` is the node-block split of
sharded.train_step_blocksharded: each block's row sum over the GLOBAL den."""
import torch
import torch.nn.functional as F

from loss_ref import G

SHAPES = ((1, 1), (7, 2), (63, 5), (200, 41), (130, 70))      # C = 70: two trips of the lane loop; C = 1: every term vanishes
EPS = (0.0, 0.1, 1.0)
WEIGHTS = ("none", "rand", "zero1")                            # no weight / uniform in [0.2, 5] / the same with one class at 0
MASKS = ("60", "one", "none")


def _case(N, C, eps, wkind, mask, scale=1.0, dead_train=False):
    g = torch.Generator().manual_seed(1000 * N + 10 * C + len(wkind) + 7 * len(mask) + (3 if dead_train else 0))
    L = torch.randn(N, C, generator=g) * scale
    y = torch.randint(0, C, (N,), generator=g)
    m = torch.rand(N, generator=g) < 0.6
    m[0] = True
    if mask == "one":
        m[:] = False
        m[N // 2] = True
    elif mask == "none":
        m[:] = False
    w = None
    if wkind != "none":
        w = torch.rand(C, generator=g) * 4.8 + 0.2
        if wkind == "zero1":
            w[int(torch.randint(0, C, (1,), generator=g))] = 0.0
    if dead_train:                                              # every train row's class has weight 0, another class has not: 0 / 0
        y = torch.where(m, torch.zeros_like(y), y)
        w[0] = 0.0
        w[C - 1] = 1.5
    return dict(N=N, C=C, logits=L.contiguous(), y=y, mask=m, w=w, eps=float(eps), scale=scale)


def _table():
    t = {}
    for N, C in SHAPES:
        for eps in EPS:
            for wk in WEIGHTS:
                for mk in MASKS:
                    t[f"N{N}_C{C}_eps{eps}_w{wk}_m{mk}"] = lambda N=N, C=C, eps=eps, wk=wk, mk=mk: _case(N, C, eps, wk, mk)
    for N, C in ((63, 5), (130, 70)):
        for eps in EPS:
            t[f"N{N}_C{C}_eps{eps}_dead_train"] = lambda N=N, C=C, eps=eps: _case(N, C, eps, "rand", "60", dead_train=True)
    for eps in (0.0, 0.1):
        t[f"N200_C41_eps{eps}_scale80"] = lambda eps=eps: _case(200, 41, eps, "rand", "60", scale=80.0)
        t[f"N130_C70_eps{eps}_scale80_wnone"] = lambda eps=eps: _case(130, 70, eps, "none", "60", scale=80.0)
    return t


_TABLE = _table()
CASES = tuple(_TABLE)
_made, _refs = {}, {}


def make_case(name):
    """The case's inputs (fp32 / int64 / bool CPU tensors, `w` None or fp32 [C]; built once, never modified)."""
    if name not in _made:
        _made[name] = _TABLE[name]()
    return _made[name]


def closed_form(c, dtype=torch.float64, g=G, w=None, form="issue"):
    """loss, d (loss g) / d logits, den and the row losses of case `c` in `dtype`, all intermediates in that dtype.  `w`: a weight in place
    of the case's.  form: "issue" (W lse - sum_c w_c x_c) or "kernel" (sum_c w_c (lse - x_c)) for the smoothing term of the row loss."""
    dt = dtype
    L = c["logits"].to(dt)
    y, mask, eps = c["y"], c["mask"], torch.tensor(c["eps"], dtype=dt)
    N, C = L.shape
    w = c.get("w") if w is None else w
    wv = torch.ones(C, dtype=dt) if w is None else w.to(dt)
    one, zero = torch.ones((), dtype=dt), torch.zeros((), dtype=dt)
    W = wv.sum()
    mx = L.max(1).values
    lse = mx + torch.log(torch.exp(L - mx[:, None]).sum(1))
    rows = torch.arange(N)
    wy = wv[y]
    smooth = (W * lse - (wv[None, :] * L).sum(1)) if form == "issue" else (wv[None, :] * (lse[:, None] - L)).sum(1)
    row = (one - eps) * wy * (lse - L[rows, y]) + (eps / C) * smooth
    row = torch.where(mask, row, zero)
    den = torch.where(mask, wy, zero).sum()
    nan = torch.full((), float("nan"), dtype=dt)
    loss = row.sum() / den if float(den) != 0.0 else nan
    onehot = torch.zeros(N, C, dtype=dt)
    onehot[rows, y] = 1.0
    sm = torch.exp(L - lse[:, None])
    scale = torch.tensor(g, dtype=dt) / den if float(den) != 0.0 else nan
    d = scale * ((one - eps) * wy[:, None] * (sm - onehot) + (eps / C) * (W * sm - wv[None, :]))
    d = torch.where(mask[:, None], d, zero)
    return dict(loss=loss, dlogits=d, den=den, row=row)


def block_shares(c, bounds, dtype=torch.float64, g=G):
    """The node-block split: block k holds the rows [bounds[k], bounds[k + 1]) and contributes (sum of its row losses) / den with den taken
    over ALL train rows; its gradient rows are the whole problem's.  Returns ([share_k], [d logits of block k], den)."""
    full = closed_form(c, dtype, g)
    shares, grads = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        sub = dict(c, logits=c["logits"][lo:hi], y=c["y"][lo:hi], mask=c["mask"][lo:hi])
        r = closed_form(sub, dtype, g)
        shares.append(r["row"].sum() / full["den"])
        grads.append(r["dlogits"] * (r["den"] / full["den"]) if float(r["den"]) != 0.0 else torch.zeros_like(r["dlogits"]))
    return shares, grads, full["den"]


def torch_form(c, g=G):
    """The same two quantities by F.cross_entropy and autograd in fp64: the definition."""
    L = c["logits"].double().requires_grad_(True)
    w = None if c["w"] is None else c["w"].double()
    m = c["mask"]
    loss = F.cross_entropy(L[m], c["y"][m], weight=w, label_smoothing=c["eps"], reduction="mean")
    (d,) = torch.autograd.grad(loss * g, (L,))
    return dict(loss=loss.detach(), dlogits=d)


def reference(name):
    """(fp64 closed form, fp32 closed form) of a case, computed once."""
    if name not in _refs:
        c = make_case(name)
        _refs[name] = (closed_form(c, torch.float64), closed_form(c, torch.float32))
    return _refs[name]
