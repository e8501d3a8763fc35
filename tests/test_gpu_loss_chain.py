"""The learned step's loss chain (csrc/losses.hip through ops.hybrid_loss, ops.masked_cross_entropy, ops.edge_regularizers, the gate's
counts, the edge-sharded entry points of the C ABI, and the in-place hand-over of d w to _GCNNorm.backward) against the fp64 reference
of tests/loss_ref.py.  Integer outputs and everything that is bitwise by reading of the kernels are compared with no tolerance; every
other quantity under loss_ref.bound: 8 x the deviation of the fp32 evaluation of the closed form from the fp64 one + 4 ulp at the
quantity's largest magnitude, per case and per quantity.  Every check prints `RATIO <quantity> <case> <error / bound>` before it asserts.

What the cosine's clamp pins (cases clamp_big, clamp_tiny, test_cosine_clamp_through_the_c_abi): the kernel's documented form
cos = <x, y> / sqrt(max(|x|^2 |y|^2, 1e-16)), under which the denominator is a CONSTANT while the clamp is active.  Its gradient rows are
then -r y 1e8 and -r x 1e8: the norm term cos x / |x|^2 contributes nothing, the row that faces a zero row is exactly zero, and the zero
row itself receives y 1e8 r (autograd of the documented formula gives the same; tests/test_loss_ref_cpu.py).

Largest error / bound per quantity measured on an MI355X over all cases of this file (plain and with SGS_POISON=1: the same figures):
hybrid_loss: reg1 0.25, reg2 0.16, c1 reg1 + c2 reg2 0.21, ce 0.25, loss 0.23, d logits 0.13 (under the clamp 0.09), d w 0.10 (saturated
entries 0.06); fused against unfused: both gradients and the five regulariser outputs bitwise, loss 0.09 of twice the bound; edge-sharded: raw sums
0.07 / 0.13, d w 0.09, Gs 0.11, Gd 0.10; clamp through the C ABI: cos 0.10, rows 0.11; hand-over: logits 0.16, d w 0.19, d p 0.07, fused = unfused
bitwise.  No ratio above 0.25; fused against unfused cross entropy 0.12 of twice the bound.

Found by this file: a row of -inf had no argmax in the three gate kernels (the compiled row scan never left its "no column yet" sentinel when
nothing exceeded the initial -inf), so such a row never counted as correct where torch.argmax gives 0; fixed in csrc/losses.hip (lane_argmax)."""
import pytest
import torch

import loss_ref as R
from oracle import sgs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_WORST = {}


@pytest.fixture(scope="module")
def ops():
    import sgs_gnn_amd as S
    yield S.ops
    print("\n" + "\n".join(f"WORST {k} {v[0]:.3f} ({v[1]})" for k, v in sorted(_WORST.items())))


def _check(case, quantity, got, want, bd):
    """|got - want| <= bd over the entries where the reference is a number; nan exactly where the reference is nan."""
    got, want = torch.as_tensor(got).detach().double().cpu().flatten(), torch.as_tensor(want).double().flatten()
    assert got.shape == want.shape, (case, quantity, got.shape, want.shape)
    if want.numel() == 0:
        return
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (case, quantity, "nan pattern")
    if bool(nan.all()):
        return
    err = float((got - want)[~nan].abs().max())
    ratio = err / bd if bd > 0 else (0.0 if err == 0 else float("inf"))
    print(f"RATIO {quantity} {case} {ratio:.4f} err={err:.3e} bound={bd:.3e}")
    if ratio >= _WORST.get(quantity, (-1.0, ""))[0]:
        _WORST[quantity] = (ratio, case)
    assert err <= bd, (case, quantity, err, bd)


def _dev(c):
    return dict(y=c["y"].to(DEV), mask=c["mask"].to(DEV), sei=c["sei"].to(DEV).contiguous())


def _leaves(c):
    return c["logits"].to(DEV).requires_grad_(True), c["w"].to(DEV).requires_grad_(True)


def _fused(ops, c, d):
    ld, wd = _leaves(c)
    loss, out = ops.hybrid_loss(ld, d["y"], d["mask"], wd, d["sei"], c["c1"], c["c2"])
    gl, gw = torch.autograd.grad(loss * R.G, (ld, wd))
    return loss.detach(), out, gl, gw


# ---------------------------------------------------------------------------------------------------- hybrid_loss against the closed form
@pytest.mark.parametrize("name", R.HYBRID_CASES)
def test_hybrid_loss_against_fp64(ops, name):
    c = R.make_case(name)
    d = _dev(c)
    r64, bd = R.reference(name)[0], R.bounds(name)
    loss, out, gl, gw = _fused(ops, c, d)
    o = out.cpu().double()
    assert float(o[2]) == float(r64["out7"][2]) and float(o[3]) == float(r64["out7"][3]), (o, r64["out7"])         # the counts: exact integers
    assert torch.equal(loss.reshape(1).cpu().view(torch.int32), out[6:7].cpu().view(torch.int32))                  # the scalar IS out[6]
    got = R.quantities(dict(out7=o, dlogits=gl.cpu().double(), dw=gw.cpu().double(), sat=r64["sat"], hot_rows=r64["hot_rows"]))
    want = R.quantities(r64)
    for k in want:
        _check(name, k, got[k], want[k], bd[k])
    assert bool(torch.isfinite(o[:5]).all())
    if not bool(c["mask"].any()):
        assert bool(torch.isnan(o[5:]).all())                        # torch's mean over nothing
    else:
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(gl).all()) and bool(torch.isfinite(gw).all())
    if "label_sum" in c:
        assert float(o[3]) == c["label_sum"] and (float(o[0]) > 0) == (c["label_sum"] == 2)
    if name == "scale_1e4":                                          # the softmax is an exact one-hot: the cross entropy's share of a train row's
        only_reg = dict(c, mask=torch.zeros_like(c["mask"]))         # gradient is 0 everywhere or (+g / #train at the maximum, -g / #train at the label)
        share = gl.cpu().double() - R.closed_form(only_reg)["dlogits"]
        gn = float(torch.tensor(R.G, dtype=torch.float32) / float(c["mask"].sum()))
        big = share.abs() > 0.5 * gn
        assert bool((big.sum(1) <= 2).all()) and bool(((share[big].abs() - gn).abs() <= 1e-6 * gn).all()) and float(share[~big].abs().max()) <= 4 * bd["dlogits"]


# ---------------------------------------------------------------------------------------------------- fused against unfused
@pytest.mark.parametrize("name", R.FUSED_CASES)
def test_fused_equals_unfused(ops, name):
    """ops.hybrid_loss against ops.masked_cross_entropy + ops.edge_regularizers on the same inputs.  d w: the same kernel with the same
    arguments; d logits: the unfused path adds (softmax - onehot) g / n to the regularisers' rows by autograd's add, the fused one adds
    the same product to the same rows inside ce_bwd<false, true> (the library is built without contraction: a product, then one add) -- both
    bitwise.  The five regulariser outputs come from the same partials through the same 256-stride finish: bitwise.  The cross entropy is
    summed over 256 strides here and 1024 there: both within the case's bound of the fp64 value, so within twice it of each other."""
    c = R.make_case(name)
    d = _dev(c)
    bd = R.bounds(name)
    loss, out, gl, gw = _fused(ops, c, d)
    ld, wd = _leaves(c)
    ce = ops.masked_cross_entropy(ld, d["y"], d["mask"])
    reg, terms = ops.edge_regularizers(wd, ld, d["sei"], d["y"], d["mask"], c["c1"], c["c2"])
    gl2, gw2 = torch.autograd.grad((ce + reg) * R.G, (ld, wd), allow_unused=True)
    assert torch.equal(gw.view(torch.int32), gw2.view(torch.int32))
    assert torch.equal(gl.view(torch.int32), gl2.view(torch.int32))
    assert torch.equal(out[:5].view(torch.int32), terms.view(torch.int32))
    _check(name, "ce_fused_vs_unfused", out[5], ce.detach().double().cpu(), 2 * bd["ce"])
    _check(name, "loss_fused_vs_unfused", out[6], (ce + reg).detach().double().cpu(), 2 * bd["loss"])


# ---------------------------------------------------------------------------------------------------- the edge-sharded entry points
def _reg_bwd(ops, L, c, d, lo, hi, out5, q_global):
    """sgs_edge_reg_bwd on the edges [lo, hi) as sharded.py calls it; the outputs start as nan."""
    q, (N, C) = hi - lo, c["logits"].shape
    from sgs_gnn_amd import _lib
    w = c["w"][lo:hi].to(DEV).contiguous()
    sei = c["sei"][:, lo:hi].to(DEV).contiguous()
    lg = c["logits"].to(DEV)
    g = torch.tensor([R.G], dtype=torch.float32, device=DEV)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)             # noqa: E731
    dw, Gs, Gd = nan(q), nan(q, C), nan(q, C)
    _lib.check(L.sgs_edge_reg_bwd(ops._ptr(w), ops._ptr(sei), q, q_global, ops._ptr(lg), N, C, ops._ptr(d["y"]), ops._ptr(ops._u8(d["mask"])),
                                  ops._ptr(out5), c["c1"], c["c2"], ops._ptr(g), ops._ptr(dw), ops._ptr(Gs), ops._ptr(Gd), ops._stream()),
               "sgs_edge_reg_bwd")
    return dw, Gs, Gd


def test_edge_sharded_partials_and_backward(ops):
    """sgs_edge_reg_partial per shard (0, 1, 1983 and 3016 edges of the q = 5000 case), the four raw sums added over the shards, and
    sgs_edge_reg_bwd(q_global = 5000) per shard against the matching rows of the unsharded reference."""
    import sgs_gnn_amd as S
    L, _lib = S._lib.lib(), S._lib
    c = R.make_case(R.SHARD_CASE)
    d = _dev(c)
    N, C = c["logits"].shape
    lg = c["logits"].to(DEV)
    r64 = R.reference(R.SHARD_CASE)[0]
    bds = R.shard_bounds()
    total = torch.zeros(4, dtype=torch.float64)
    raws = []
    for lo, hi in R.SHARDS:
        q = hi - lo
        w = c["w"][lo:hi].to(DEV).contiguous()
        sei = c["sei"][:, lo:hi].to(DEV).contiguous()
        raw = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV)
        ws = ops.workspace(L.sgs_edge_reg_workspace_bytes(q), lg.device)
        _lib.check(L.sgs_edge_reg_partial(ops._ptr(w), ops._ptr(sei), q, ops._ptr(lg), N, C, ops._ptr(d["y"]), ops._ptr(ops._u8(d["mask"])),
                                          ops._ptr(raw), ws.data_ptr(), ws.numel(), ops._stream()), "sgs_edge_reg_partial")
        want = R.raw_sums(c, lo, hi)
        got = raw.cpu().double()
        assert float(got[2]) == float(want[2]) and float(got[3]) == float(want[3]), (lo, hi, got, want)
        if q == 0:
            assert torch.equal(got, torch.zeros(4, dtype=torch.float64))                     # four zeros over the nan fill
        _check(f"shard_{lo}_{hi}", "raw_bce", got[0], want[0], bds[(lo, hi)]["raw0"])
        _check(f"shard_{lo}_{hi}", "raw_sq", got[1], want[1], bds[(lo, hi)]["raw1"])
        raws.append(raw)
        total += got
    full = r64["raw"]
    assert float(total[2]) == float(full[2]) and float(total[3]) == float(full[3])
    _check("shards_summed", "raw_bce", total[0], full[0], sum(b["raw0"] for b in bds.values()))
    _check("shards_summed", "raw_sq", total[1], full[1], sum(b["raw1"] for b in bds.values()))
    # the global vector as sharded.py forms it from the all-reduced sums (the backward reads out[2] and out[3])
    rawg = torch.stack(raws).sum(0)
    reg1 = torch.where(rawg[3] > 1.0, rawg[0] / rawg[2], torch.zeros((), device=DEV))
    reg2 = rawg[1] / float(c["q"])
    out5 = torch.stack([reg1, reg2, rawg[2], rawg[3], c["c1"] * reg1 + c["c2"] * reg2]).contiguous()
    for lo, hi in R.SHARDS:
        dw, Gs, Gd = _reg_bwd(ops, L, c, d, lo, hi, out5, c["q"])
        for k, got in (("dw", dw), ("Gs", Gs), ("Gd", Gd)):
            _check(f"shard_{lo}_{hi}", "shard_" + k, got, r64[k][lo:hi], bds[(lo, hi)][k])


def test_cosine_clamp_through_the_c_abi(ops):
    """The per-edge values and rows of the clamp cases straight from sgs_edge_reg_fwd (cos_out) and sgs_edge_reg_bwd."""
    import sgs_gnn_amd as S
    L, _lib = S._lib.lib(), S._lib
    for name in ("clamp_big", "clamp_tiny"):
        c = R.make_case(name)
        d = _dev(c)
        q, (N, C) = c["q"], c["logits"].shape
        r64, r32 = R.reference(name)
        lg, w = c["logits"].to(DEV), c["w"].to(DEV)
        out5 = torch.full((5,), float("nan"), dtype=torch.float32, device=DEV)
        cos = torch.full((q,), float("nan"), dtype=torch.float32, device=DEV)
        ws = ops.workspace(L.sgs_edge_reg_workspace_bytes(q), lg.device)
        _lib.check(L.sgs_edge_reg_fwd(ops._ptr(w), ops._ptr(d["sei"]), q, ops._ptr(lg), N, C, ops._ptr(d["y"]), ops._ptr(ops._u8(d["mask"])),
                                      c["c1"], c["c2"], ops._ptr(out5), ops._ptr(cos), ws.data_ptr(), ws.numel(), ops._stream()), "sgs_edge_reg_fwd")
        _check(name, "cos", cos, r64["cos"], R.bound(r64["cos"], r32["cos"]))
        dw, Gs, Gd = _reg_bwd(ops, L, c, d, 0, q, out5, q)
        cl = r64["clamped"]
        assert int(cl.sum()) >= 5
        for k, got in (("Gs", Gs), ("Gd", Gd)):
            _check(name, "clamp_" + k, got.cpu()[cl], r64[k][cl], R.bound(r64[k][cl], r32[k][cl]))
            _check(name, "noclamp_" + k, got.cpu()[~cl], r64[k][~cl], R.bound(r64[k][~cl], r32[k][~cl]))
        _check(name, "dw", dw, r64["dw"], R.bound(r64["dw"], r32["dw"]))
        s, t = c["sei"]
        zero_row = c["logits"].abs().sum(1) == 0
        assert bool(zero_row.any())
        assert bool((cos.cpu()[zero_row[s] | zero_row[t]] == 0).all())               # the value: <0, y> / 1e-8 = 0
        assert bool((Gd.cpu()[zero_row[s]] == 0).all()) and bool((Gs.cpu()[zero_row[t]] == 0).all())     # the row facing a zero row: -r 0 1e8


# ---------------------------------------------------------------------------------------------------- the gate: exact integers
@pytest.mark.parametrize("C", R.GATE_C)
@pytest.mark.parametrize("N", R.GATE_N)
def test_gate_counts_exact(ops, N, C):
    g = R.gate_case(N, C)
    A, B, y, m = g["A"].to(DEV), g["B"].to(DEV), g["y"].to(DEV), g["mask"].to(DEV)
    want = [*R.argmax_counts(g["A"], g["y"], g["mask"]), *R.argmax_counts(g["B"], g["y"], g["mask"])]
    none = torch.zeros_like(m)
    assert ops.gate_counts(A, B, y, m).tolist() == want + [0]
    assert ops.gate_counts(A, B, y, none).tolist() == [0] * 5
    assert ops.gate_counts(B, A, y, m).tolist() == want[2:] + want[:2] + [0]
    if N == 0:
        return
    buf = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert ops.masked_correct_pair(A, B, y, m, buf).tolist() == want
    assert ops.masked_correct_pair(A, B, y, m, buf).tolist() == [2 * v for v in want]          # its contract: it accumulates
    assert ops.masked_correct_pair(A, B, y, none, torch.zeros(4, dtype=torch.int32, device=DEV)).tolist() == [0] * 4
    assert ops.masked_correct(A, y, m).tolist() == want[:2] and ops.masked_correct(B, y, m).tolist() == want[2:]
    assert ops.masked_correct(A, y, none).tolist() == [0, 0]


def test_gate_counts_publish(ops):
    g = R.gate_case(1040, 130)
    A, B, y, m = g["A"].to(DEV), g["B"].to(DEV), g["y"].to(DEV), g["mask"].to(DEV)
    want = [*R.argmax_counts(g["A"], g["y"], g["mask"]), *R.argmax_counts(g["B"], g["y"], g["mask"])]
    for seq_val, word in (((5 << 32) + 123456, 123456), (None, 1)):
        dst = torch.full((5,), -7, dtype=torch.int32).pin_memory()
        seq = None if seq_val is None else torch.tensor([seq_val], dtype=torch.int64, device=DEV)
        out = ops.gate_counts(A, B, y, m, publish=(seq, dst))
        torch.cuda.synchronize()
        assert dst.tolist() == want + [word]
        assert out.tolist() == want + [0]


# ---------------------------------------------------------------------------------------------------- the in-place hand-over of d w
def _gcn_inputs(c):
    return {k: c[k].to(DEV) for k in ("x", "W1", "b1", "W2", "b2", "y", "mask")}


def _step(ops, c, t, w, sei, fused=True, unit=False, loss_w=None, loss_sei=None, leaf=None):
    """One forward / backward of the two-layer GCN over (sei, w) with the loss on (loss_sei, loss_w) -> (d leaf, out, nm)."""
    graph = ops.get_graph(sei, c["N"])
    nm = ops.gcn_norm(graph) if unit else ops.gcn_norm(graph, w)
    logits, _ = ops.gcn2(t["x"], t["W1"], t["b1"], t["W2"], t["b2"], nm)
    lw, ls = (w if loss_w is None else loss_w), (sei if loss_sei is None else loss_sei)
    if fused:
        loss, out = ops.hybrid_loss(logits, t["y"], t["mask"], lw, ls, c["c1"], c["c2"])
    else:
        reg, out = ops.edge_regularizers(lw, logits, ls, t["y"], t["mask"], c["c1"], c["c2"])
        loss = ops.masked_cross_entropy(logits, t["y"], t["mask"]) + reg
    (gw,) = torch.autograd.grad(loss * R.G, (w if leaf is None else leaf,))
    return gw, out, nm, logits.detach()


def _clean(nm):
    return all(getattr(nm, k, None) is None for k in ("_dw_first", "_g_extra", "_g_first"))


def _hand_bound(c, **kw):
    a, b = R.hand_reference(c, **kw), R.hand_reference(c, torch.float32, **kw)
    return a, R.bound(a["dw"], b["dw"]), R.bound(a["logits"], b["logits"])


def test_dw_hand_over_leaf_two_steps_fused_equals_unfused(ops):
    """(i), (ii): w a leaf, two consecutive steps on fresh inputs.  The loss's d w is parked on the Norm and _GCNNorm.backward adds its own
    share to it in place (one fp32 add per entry inside norm_bwd_edge); the unfused loss hands autograd two gradients and autograd adds
    them (the same add, commuted): bitwise equal, and nothing is left on the Norm."""
    for seed in (0, 1):
        c = R.hand_case(seed)
        t, sei = _gcn_inputs(c), c["sei"].to(DEV).contiguous()
        ref, bd, bdl = _hand_bound(c)
        w = c["w"].to(DEV).requires_grad_(True)
        gw, out, nm, logits = _step(ops, c, t, w, sei)
        assert _clean(nm)
        _check(f"hand_leaf_{seed}", "hand_logits", logits, ref["logits"], bdl)
        _check(f"hand_leaf_{seed}", "hand_dw", gw, ref["dw"], bd)
        assert float(out[2]) == float(ref["out7"][2]) and float(out[3]) == float(ref["out7"][3])
        w2 = c["w"].to(DEV).requires_grad_(True)
        gw2, _, nm2, _ = _step(ops, c, t, w2, c["sei"].to(DEV).contiguous(), fused=False)
        assert _clean(nm2)
        assert torch.equal(gw.view(torch.int32), gw2.view(torch.int32))


def test_dw_hand_over_unit_norm_and_other_length(ops):
    """(iii) the model runs on unit weights: d w is the regularisers' alone and nothing is parked on the (cached) unit Norm.
    (iv) the loss reads another, shorter edge list with the first entries of w: the parking guard dw.numel() == n_edges is false and
    autograd adds the slice's gradient to the normalisation's.  (No public call hands hybrid_loss a tensor that carries a Norm of another
    length -- gcn_norm insists on w.numel() == n_edges --, so the slice is given the Norm's reference by hand to reach the guard itself.)"""
    c = R.hand_case(2, q_loss=450)
    t, sei = _gcn_inputs(c), c["sei"].to(DEV).contiguous()
    ref, bd, _ = _hand_bound(c, model_w=None)
    w = c["w"].to(DEV).requires_grad_(True)
    gw, _, nm, _ = _step(ops, c, t, w, sei, unit=True)
    assert _clean(nm) and getattr(w, "_sgs_norm", None) is None
    _check("hand_unit", "hand_dw", gw, ref["dw"], bd)
    only = R.closed_form(dict(c, logits=ref["logits"].float()))                      # the loss alone on the model's logits: the same d w
    assert float((only["dw"] - ref["dw"].detach()).abs().max()) < 1e-6
    ref, bd, _ = _hand_bound(c, loss_edges="sei_loss")
    w = c["w"].to(DEV).requires_grad_(True)
    sl = c["sei_loss"].to(DEV).contiguous()
    graph = ops.get_graph(sei, c["N"])
    nm = ops.gcn_norm(graph, w)
    lw = w[:450]
    lw._sgs_norm = w._sgs_norm
    logits, _ = ops.gcn2(t["x"], t["W1"], t["b1"], t["W2"], t["b2"], nm)
    loss, _ = ops.hybrid_loss(logits, t["y"], t["mask"], lw, sl, c["c1"], c["c2"])
    (gw,) = torch.autograd.grad(loss * R.G, (w,))
    assert _clean(nm)
    _check("hand_other_length", "hand_dw", gw, ref["dw"], bd)


@pytest.mark.parametrize("producer", ["select_sampled", "st_weights"])
def test_dw_hand_over_through_the_producers_of_w(ops, producer):
    """(v) w from ops.select_sampled (no ActiveSet: the scatter into [E]) and from ops.st_weights, over a draw of q = 600 among E = 3000
    made with explicit constant noise (the race is decided by p alone); d p over all E entries.  (A leaf w: the tests above.)"""
    c = R.draw_case()
    t = _gcn_inputs(c)
    E, q, sel = c["E"], c["q"], c["sel"]
    p = c["p"].to(DEV).requires_grad_(True)
    r = ops.sample_topq(ops.SAMPLE_LEARNED, p.detach(), None, 0.3, q, c["parent"].to(DEV), noise=c["noise"].to(DEV))
    assert torch.equal(r.mask.cpu(), sel) and torch.equal(r.edge_index.cpu(), c["sei"]) and torch.equal(r.eid.cpu(), c["pos"])
    if producer == "select_sampled":
        w = ops.select_sampled(p, r.eid, r.p)
        prod = lambda dt: (lambda leaf: (leaf, leaf[sel]))(c["p"].to(dt).requires_grad_(True))                            # noqa: E731
    else:
        w = ops.st_weights(p, None, 0.3, r.stats, r.eid)
        prod = lambda dt: (lambda leaf: (leaf, O.gumbel_softmax_sampling(None, leaf, q, 0.3, True, force_mask=sel, Z=None)[1]))(     # noqa: E731
            c["p"].to(dt).requires_grad_(True))
    ref, bd, _ = _hand_bound(c, producer=prod)
    wb = R.bound(ref["w"], R.hand_reference(c, torch.float32, producer=prod)["w"])
    _check(producer, "hand_w", w, ref["w"], wb)
    gp, _, nm, _ = _step(ops, c, t, w, r.edge_index, leaf=p)
    assert _clean(nm) and gp.shape == (E,)
    _check(producer, "hand_dp", gp, ref["dw"], bd)
    if producer == "select_sampled":
        assert bool((gp.cpu()[~sel] == 0).all()) and bool((ref["dw"][~sel] == 0).all())        # exact zeros at the edges that were not drawn
