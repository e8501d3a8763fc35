"""GPU: the scorer's opt-in bf16 mode (include/sgs_hip.h, "bf16 mode"; ops.edge_score(precision=...), args.sgs_precision).

bf16 mode issues only the v1 x v1 product of the fp32-faithful path's exact operand splits (v1 = RNE_bf16(v)), accumulated in fp32.  The
forward is held to an fp64 evaluation of the bf16-ROUNDED operands, the backward's two one-piece contractions likewise, and both to the fp32
function within a bf16 bound."""
import argparse

import numpy as np
import pytest
import torch

from oracle import sgs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    import sgs_gnn_amd
    return sgs_gnn_amd


def _bf(t):
    """RNE to bf16 and back, in fp64 (as pk_bf16)."""
    return t.float().to(torch.bfloat16).to(torch.float64)


def _params(H, seed, wide=False):
    g = torch.Generator().manual_seed(seed)
    b = 1.0 / (2 * H) ** 0.5
    W1 = (torch.rand(H, 2 * H, generator=g) * 2 - 1) * b
    if wide:                                        # operands spread over many binades (as test_bf16x6_split_is_fp32_faithful)
        W1 = W1 * torch.exp2(torch.randint(-6, 7, (H, 2 * H), generator=g).float())
    b1 = (torch.rand(H, generator=g) * 2 - 1) * b
    W2 = (torch.rand(1, H, generator=g) * 2 - 1) / H ** 0.5
    b2 = (torch.rand(1, generator=g) * 2 - 1) / H ** 0.5
    return W1, b1, W2, b2


def _graph(S, ops, N, seed):
    """Undirected graph stored both ways plus self loops, one-directional and duplicate edges, sorted by (src, dst)."""
    b = S.synthetic_graph(N, 90_000, 8, 3, seed=seed, device=DEV)
    g = torch.Generator().manual_seed(seed + 1)
    extra = torch.randint(0, N, (2, 3000), generator=g)
    loops = torch.arange(0, 50).repeat(2, 1)
    dup = b.edge_index[:, :500].cpu()
    ei = torch.cat([b.edge_index.cpu(), extra, loops, dup], dim=1)
    return ei[:, torch.argsort(ei[0] * N + ei[1], stable=True)].contiguous().to(DEV)


def _emulate(codes, ei, W1, b1, W2, b2, p, keep):
    """fp64 forward of the bf16 mode: v = bf16(W1a) . bf16(x_s * x_d) + (U[s] - U[d]) + b1 with U the fp32 library GEMM, then the fp32
    function's epilogue.  Returns (prob, v, kept-and-positive mask)."""
    H = codes.shape[1]
    c = codes.float().cpu()
    eic = ei.cpu()
    feat = _bf(c[eic[0]] * c[eic[1]])
    U = (c @ W1[:, H:].t()).double()
    v = feat @ _bf(W1[:, :H]).t() + (U[eic[0]] - U[eic[1]]) + b1.double()
    on = v > 0
    scale = 1.0
    if p > 0:
        on = on & keep.bool()
        scale = 1.0 / (1.0 - p)
    h = torch.where(on, v, torch.zeros_like(v)) * scale
    z = h @ W2.double().t() + b2.double()
    return torch.sigmoid(z).squeeze(1), v, on


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_forward_forms_equal_bf16_emulation(S, H, p):
    ops = S.ops
    N = 700
    ei = _graph(S, ops, N, 4)
    E = ei.shape[1]
    assert E >= 65536
    g = torch.Generator().manual_seed(H)
    codes = torch.relu(torch.randn(N, H, generator=g))
    W1, b1, W2, b2 = _params(H, 5)
    canon, mate = ops.get_pairs(ei, N, build=True)
    seed, site = 31, 2
    keep = ops.dropout_keep(seed, site, E, H, p, DEV).cpu() if p > 0 else None
    pe, v, on = _emulate(codes, ei, W1, b1, W2, b2, p, keep)
    d = [t.to(DEV) for t in (codes, W1, b1, W2, b2)]
    ops.reset_precision_counts()
    outs = {}
    with torch.no_grad():
        outs["plain"] = ops.edge_score(*d, ei, p=p, seed=seed, site=site, pairs=None, precision="bf16")
        outs["paired"] = ops.edge_score(*d, ei, p=p, seed=seed, site=site, pairs=(canon, mate), precision="bf16")
    assert ops.PRECISION_COUNTS["fwd_bf16"] == 2 and ops.PRECISION_COUNTS["fwd_fp32"] == 0
    # the mask-keeping (training) forward, paired
    dl = [t.clone().requires_grad_(True) for t in d]
    with S.scorer_precision("bf16"):
        outs["mask"] = ops.edge_score(*dl, ei, p=p, seed=seed, site=site, pairs=(canon, mate)).detach()
    assert ops.PRECISION_COUNTS["fwd_bf16"] == 3
    assert torch.equal(outs["plain"], outs["paired"]) and torch.equal(outs["plain"], outs["mask"])
    for k, o in outs.items():
        assert float((o.cpu().double() - pe).abs().max()) < 2e-6, k
    # the mask bits, from the C entry itself (the autograd node keeps them in its ctx)
    L = S._lib.lib()
    from sgs_gnn_amd.ops import _ptr, workspace, _stream
    U = torch.mm(d[0], d[1][:, H:].t())
    bits = torch.empty(E, H // 32, dtype=torch.int32, device=DEV)
    out = torch.empty(E, device=DEV)
    ws = workspace(L.sgs_edge_score_workspace_bytes(N, H, E), DEV)
    S._lib.check(L.sgs_edge_score_fwd_mask_bf16(_ptr(d[0]), _ptr(U), N, H, _ptr(ei), E, 0, _ptr(canon), canon.numel(), _ptr(mate), _ptr(d[1]),
                                                _ptr(d[2]), _ptr(d[3].reshape(-1)), _ptr(d[4]), float(p), seed, site, _ptr(out), _ptr(bits),
                                                ws.data_ptr(), ws.numel(), _stream()), "fwd_mask_bf16")
    torch.cuda.synchronize()
    assert torch.equal(out, outs["plain"])
    bw = bits.cpu().view(torch.int32).numpy().view(np.uint32)
    got = torch.from_numpy(np.unpackbits(bw.view(np.uint8), bitorder="little").reshape(E, H).astype(bool))
    clear = v.abs() > 2e-6
    assert torch.equal(got[clear], on[clear])


def test_forward_bf16_is_within_its_bound_of_the_fp32_function(S):
    ops = S.ops
    N, H, E = 1013, 256, 100_001
    g = torch.Generator().manual_seed(9)
    codes = torch.relu(torch.randn(N, H, generator=g)) * torch.exp2(torch.randint(-4, 5, (N, H), generator=g).float())
    ei = torch.randint(0, N, (2, E), generator=g)
    W1, b1, W2, b2 = _params(H, 10, wide=True)
    p, seed, site = 0.3, 7, 2
    d = [t.to(DEV) for t in (codes, W1, b1, W2, b2)]
    ops.reset_precision_counts()
    with torch.no_grad():
        pb = ops.edge_score(*d, ei.to(DEV), p=p, seed=seed, site=site, pairs=None, precision="bf16").cpu().double()
        pf = ops.edge_score(*d, ei.to(DEV), p=p, seed=seed, site=site, pairs=None, precision="fp32").cpu().double()
    assert ops.PRECISION_COUNTS == {"fwd_fp32": 1, "fwd_bf16": 1, "bwd_fp32": 0, "bwd_bf16": 0}
    keep = ops.dropout_keep(seed, site, E, H, p, DEV).cpu()
    p64 = O.edge_score(codes[ei[0]].double(), codes[ei[1]].double(), W1.double(), b1.double(), W2.double(), b2.double(), p, keep).squeeze(1)
    # per edge: 1/4 sum_h |w2_h| / (1 - p) (2^-7 + 2^-16) sum_k |W1a[h, k]| |feat_k| + 2e-6
    feat = (codes[ei[0]] * codes[ei[1]]).double().abs()
    A = W2.double().abs().reshape(-1) / (1 - p) * (2.0 ** -7 + 2.0 ** -16)
    bound = 0.25 * (feat @ (W1[:, :H].double().abs() * A.reshape(-1, 1)).t()).sum(1) + 2e-6
    assert bool(((pb - p64).abs() <= bound).all())
    e32 = float((pf - p64).abs().max())
    assert float((pb - pf).abs().max()) > 10 * e32


def _kernel_mask(S, codes, ei, W1, b1, W2, b2, p, seed, site):
    """(p [E], mask [E, H] bool) of the bf16 mask-keeping forward, from its C entry."""
    from sgs_gnn_amd.ops import _ptr, workspace, _stream
    L = S._lib.lib()
    N, H = codes.shape
    E = ei.shape[1]
    d = [t.to(DEV).contiguous() for t in (codes, W1, b1, W2.reshape(-1), b2)]
    U = torch.mm(d[0], d[1][:, H:].t())
    bits = torch.empty(E, H // 32, dtype=torch.int32, device=DEV)
    out = torch.empty(E, device=DEV)
    ws = workspace(L.sgs_edge_score_workspace_bytes(N, H, E), DEV)
    S._lib.check(L.sgs_edge_score_fwd_mask_bf16(_ptr(d[0]), _ptr(U), N, H, _ptr(ei), E, 0, None, 0, None, _ptr(d[1]), _ptr(d[2]), _ptr(d[3]),
                                                _ptr(d[4]), float(p), seed, site, _ptr(out), _ptr(bits), ws.data_ptr(), ws.numel(), _stream()),
                 "fwd_mask_bf16")
    torch.cuda.synchronize()
    bw = bits.cpu().numpy().view(np.uint32)
    return out.cpu(), torch.from_numpy(np.unpackbits(bw.view(np.uint8), bitorder="little").reshape(E, H).astype(bool))


def _backward_emulation(codes, ei, W1, b1, W2, b2, p, keep, gp, kernel_fwd, rounded=True):
    """fp64 gradients of the mask-form backward on the forward's own p and mask (a unit with |v| within the accumulation-order rounding of
    0 may fall either way; the backward is defined given the mask the forward kept).  rounded=True: the bf16 mode's arithmetic (the dfeat
    operand bf16(diag(w2 / (1 - p)) W1a) and the weight-gradient operand bf16(dz feat), RNE); False: the same formulas exact, plus the
    element-wise bound of what those two roundings (unit roundoff 2^-8 each) can move every gradient by.  Rows with gp = 0 contribute
    nothing (dz = 0), so a drawn active set is emulated by zeroing gp outside it."""
    H = codes.shape[1]
    N = codes.shape[0]
    pe_emu, v, on_emu = _emulate(codes, ei, W1, b1, W2, b2, p, keep)
    pe, on = kernel_fwd
    clear = v.abs() > 2e-6
    assert torch.equal(on[clear], on_emu[clear]) and float((pe.double() - pe_emu).abs().max()) < 2e-6
    eic = ei.cpu()
    s, d = eic[0], eic[1]
    c32 = codes.float()
    c = c32.double()
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    dz = (gp.float() * pe.float() * (1.0 - pe.float())).double()    # as the prep forms it
    bit = on.double()
    w2 = W2.reshape(-1)
    rnd = _bf if rounded else (lambda t: t.double())
    Wd32 = W1[:, :H] * (w2 * np.float32(scale)).reshape(-1, 1)     # diag(w2 / (1 - p)) W1a, formed in fp32 as the pack forms it
    dfeat = dz.reshape(-1, 1) * (bit @ rnd(Wd32))
    B32 = (c32[s] * c32[d]) * dz.float().reshape(-1, 1)              # dz * feat, formed in fp32 as the GEMM forms it
    T = bit.t() @ rnd(B32)
    dW1a = (w2.double() * scale).reshape(-1, 1) * T
    dv = dz.reshape(-1, 1) * bit * (w2.double() * scale)
    db1 = dv.sum(0)
    dU = torch.zeros(N, H, dtype=torch.float64).index_add_(0, s, dv).index_add_(0, d, -dv)
    dcodes = torch.zeros(N, H, dtype=torch.float64).index_add_(0, s, dfeat * c[d]).index_add_(0, d, dfeat * c[s])
    dcodes = dcodes + dU @ W1[:, H:].double()
    dW1b = dU.t() @ c
    U = (c32 @ W1[:, H:].t()).double()
    Rd = (dz.reshape(-1, 1) * bit)
    dw2 = scale * ((W1[:, :H].double() * T).sum(1) + (Rd * (U[s] - U[d])).sum(0) + b1.double() * Rd.sum(0))
    db2 = dz.sum().reshape(1)
    grads = [dcodes, torch.cat([dW1a, dW1b], 1), db1, dw2.reshape(1, -1), db2]
    if rounded:
        return grads
    u = 2.0 ** -8
    Df = dz.abs().reshape(-1, 1) * (bit @ Wd32.double().abs()) * u                                   # |d dfeat|
    Bc = torch.zeros(N, H, dtype=torch.float64).index_add_(0, s, Df * c[d].abs()).index_add_(0, d, Df * c[s].abs())
    DT = (bit.t() @ B32.double().abs()) * u                                                           # |d T|
    BW1 = torch.cat([(w2.double().abs() * scale).reshape(-1, 1) * DT, torch.zeros(H, H, dtype=torch.float64)], 1)
    Bw2 = scale * (W1[:, :H].double().abs() * DT).sum(1).reshape(1, -1)
    return grads, [Bc, BW1, torch.zeros(H, dtype=torch.float64), Bw2, torch.zeros(1, dtype=torch.float64)]


def _rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-30)


@pytest.mark.parametrize("H,p", [(256, 0.3), (128, 0.0)])
@pytest.mark.parametrize("fused", [True, False])
def test_mask_backward_equals_bf16_emulation(S, H, p, fused):
    """The training form: q = 100 000 drawn (source-sorted) active rows of a source-sorted edge list, fused and unfused mask-form backward,
    against the fp64 emulation of the bf16 arithmetic at the bounds of test_fused_backward_equals_unfused_backward, and against the exact
    formulas (the fp32 function's backward on the same mask and p) within the element-wise bound of the two bf16 roundings."""
    ops = S.ops
    N, E, q = 777, 140_000, 100_000
    g = torch.Generator().manual_seed(13 + H)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[0, :6000] = 3                                              # a hub source, and sources without out-edges
    ei[0, ei[0] % 7 == 5] = 2
    ei = ei[:, torch.argsort(ei[0] * N + ei[1], stable=True)].contiguous()
    eid = torch.sort(torch.randperm(E, generator=g)[:q]).values
    codes = torch.relu(torch.randn(N, H, generator=g))
    W1, b1, W2, b2 = _params(H, 14)
    gp = torch.zeros(E)
    gp[eid] = torch.randn(q, generator=g)
    seed, site = 21, 2
    keep = ops.dropout_keep(seed, site, E, H, p, DEV).cpu() if p > 0 else None
    ei_d = ei.to(DEV)
    kf = _kernel_mask(S, codes, ei_d, W1, b1, W2, b2, p, seed, site)
    ref = _backward_emulation(codes, ei, W1, b1, W2, b2, p, keep, gp, kf)
    exact, bound = _backward_emulation(codes, ei, W1, b1, W2, b2, p, keep, gp, kf, rounded=False)
    old = ops._fused_backward
    ops._fused_backward = fused
    try:
        ops.reset_precision_counts()
        dl = [t.clone().to(DEV).requires_grad_(True) for t in (codes, W1, b1, W2, b2)]
        act = ops.ActiveSet()
        assert ops.src_sorted(ei_d)
        pd = ops.edge_score(*dl, ei_d, active=act, p=p, seed=seed, site=site, pairs=None, precision="bf16")
        act.set(eid.to(DEV), ops.Graph(ei[:, eid].to(DEV), N))
        pd.backward(gp.to(DEV))
    finally:
        ops._fused_backward = old
    assert ops.PRECISION_COUNTS["fwd_bf16"] == 1 and ops.PRECISION_COUNTS["bwd_bf16"] == 1
    for name, a, b, x, bd in zip(["dcodes", "dW1", "db1", "dw2", "db2"], dl, ref, exact, bound):
        got = a.grad.detach().cpu().double().reshape(b.shape)
        assert bool(torch.isfinite(got).all()), name
        # (d b2 is ONE sum of q signed terms: its relative error is the summation order's, not the kernels')
        assert _rel(got, b) < (2e-5 if name == "db2" else 3e-6), (name, _rel(got, b))
        slack = (2e-5 if name == "db2" else 3e-6) * float(x.abs().max())                      # fp32 accumulation, as above
        assert bool(((got - x).abs() <= bd + slack).all()), name
    # the one-piece contractions really ran: d W1a sits measurably off the exact formulas (far beyond the fp32 accumulation)
    assert _rel(dl[1].grad.detach().cpu()[:, :H], exact[1][:, :H]) > 1e-4


def _train_args(**kw):
    a = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", edge_mlp_type="GCN", conditional=True,
                           sparse_edge_mlp=True, t_init=0.7, t_min=0.5, degree_bias_coef=0.3, reg1=True, reg2=True,
                           regularizer1_coef=1.0, consist_reg_coef=0.5, hybrid_checkpoint=False, drop_rate=0.3, lr=1e-3)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _train_run(S, bs, precision, epochs=2, hipgraph=False, q=100_000):
    torch.manual_seed(4)
    S.fix_seeds(4)
    m = S.GNNModel(64, 128, 7, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
    og = torch.optim.Adam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-3)
    oe = torch.optim.Adam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    kw = {} if precision is None else {"sgs_precision": precision}
    if hipgraph:
        kw["sgs_hipgraph"] = True
    rets = [S.train(_train_args(**kw), ep, epochs, m, og, oe, None, crit, bs, q=q) for ep in range(epochs)]
    torch.cuda.synchronize()
    return rets, [p.detach().clone() for p in m.parameters()], m


def test_train_bf16_is_deterministic_and_fp32_is_today(S):
    ops = S.ops
    bs = [S.synthetic_graph(1013, E, 64, 7, seed=40 + i, device=DEV) for i, E in enumerate([180_000, 150_000])]
    ops.reset_precision_counts()
    r1, P1, _ = _train_run(S, bs, "bf16")
    assert ops.PRECISION_COUNTS["fwd_bf16"] > 0 and ops.PRECISION_COUNTS["bwd_bf16"] > 0
    r2, P2, _ = _train_run(S, bs, "bf16")
    assert r1 == r2 and all(torch.equal(a, b) for a, b in zip(P1, P2))
    ops.reset_precision_counts()
    r3, P3, _ = _train_run(S, bs, "fp32")
    assert ops.PRECISION_COUNTS["fwd_bf16"] == 0 and ops.PRECISION_COUNTS["bwd_bf16"] == 0
    r4, P4, _ = _train_run(S, bs, None)
    assert r3 == r4 and all(torch.equal(a, b) for a, b in zip(P3, P4))
    assert not all(torch.equal(a, b) for a, b in zip(P1, P3))


def test_train_hipgraph_bf16_recaptures_on_switch(S):
    from sgs_gnn_amd.stepgraph import StepGraphs
    bs = [S.synthetic_graph(1013, E, 64, 7, seed=50 + i, device=DEV) for i, E in enumerate([180_000, 150_000])]
    ops = S.ops
    torch.manual_seed(4)
    S.fix_seeds(4)
    m = S.GNNModel(64, 128, 7, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
    og = S.FusedAdam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-3)
    oe = S.FusedAdam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    ops.reset_precision_counts()
    S.train(_train_args(sgs_hipgraph=True, sgs_precision="bf16"), 0, 2, m, og, oe, None, crit, bs, q=100_000)
    sg1 = m._sgs_stepgraphs
    assert isinstance(sg1, StepGraphs) and sg1.captures > 0 and ops.PRECISION_COUNTS["fwd_bf16"] > 0
    S.train(_train_args(sgs_hipgraph=True, sgs_precision="bf16"), 1, 2, m, og, oe, None, crit, bs, q=100_000)
    assert m._sgs_stepgraphs is sg1                                       # same setting: the captures are kept
    before = ops.PRECISION_COUNTS["fwd_fp32"]
    S.train(_train_args(sgs_hipgraph=True, sgs_precision="fp32"), 1, 2, m, og, oe, None, crit, bs, q=100_000)
    assert m._sgs_stepgraphs is not sg1 and ops.PRECISION_COUNTS["fwd_fp32"] > before       # switched: dropped and re-captured
    for p in m.parameters():
        assert bool(torch.isfinite(p).all())


def test_ensemble_batched_equals_serial_in_bf16(S):
    """ensemble_evaluate in bf16 mode on a model trained (in bf16) first: the batched engine draws the serial loop's edges and gives its
    logits (to the bound of tests/test_gpu_ensemble_batched.py) and F1."""
    bs = [S.synthetic_graph(1013, E, 64, 7, seed=60 + i, device=DEV) for i, E in enumerate([180_000, 150_000])]
    _, _, m = _train_run(S, bs, "bf16", epochs=2)
    m.eval()
    res = {}
    for path in ("serial", "batched"):
        S.ops.reset_precision_counts()
        a = _train_args(num_samples_eval=3, sgs_precision="bf16")
        if path == "batched":
            a.sgs_eval_batch = True
        a._sgs_trace_eval = {}
        S.manual_seed(9)
        f1 = S.ensemble_evaluate(a, m, bs, DEV, q=100_000, mode="learned")
        assert S.ops.PRECISION_COUNTS["fwd_bf16"] > 0 and S.ops.PRECISION_COUNTS["fwd_fp32"] == 0
        res[path] = (f1, a._sgs_trace_eval, (S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
    (f_s, t_s, k_s), (f_b, t_b, k_b) = res["serial"], res["batched"]
    assert k_s == k_b
    assert torch.equal(t_s["edges"], t_b["edges"])
    assert f_s == f_b
    scale = float(t_s["logits"].abs().max())
    assert torch.allclose(t_b["logits"], t_s["logits"], rtol=0, atol=1e-5 * scale)


def test_replayed_bf16_step_at_the_benchmarked_shape_matches_its_eager_recomputation(S, monkeypatch):
    """tests/test_gpu_stepgraph.py's replay-vs-eager check of the benchmarked step (S3 shape, q = 100 000, dropout 0.3, in-graph FusedAdam),
    run with args.sgs_precision = "bf16" under scorer_precision("bf16"): the captures hold the one-piece packs and kernels, the dyn_n-bounded
    paired forward, the one-piece prep pack and the bf16 backward, and the eager recomputation from the replay's own draws runs the same."""
    import test_gpu_stepgraph as TS
    base = TS._args
    monkeypatch.setattr(TS, "_args", lambda **kw: base(**{**kw, "sgs_precision": "bf16"}))
    S.ops.reset_precision_counts()
    with S.scorer_precision("bf16"):
        TS.test_replayed_step_at_the_benchmarked_shape_matches_its_eager_recomputation()
    c = S.ops.PRECISION_COUNTS
    assert c["fwd_bf16"] > 0 and c["bwd_bf16"] > 0 and c["bwd_fp32"] == 0


def test_invalid_precision_raises(S):
    with pytest.raises(ValueError):
        S.ops.edge_score(torch.zeros(4, 128, device=DEV), torch.zeros(128, 256, device=DEV), torch.zeros(128, device=DEV),
                         torch.zeros(1, 128, device=DEV), torch.zeros(1, device=DEV), torch.zeros(2, 3, dtype=torch.int64, device=DEV),
                         precision="fp16")
