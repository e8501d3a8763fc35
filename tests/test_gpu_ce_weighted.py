"""GPU: the class-weighted / label-smoothed cross entropy on the hot path (csrc/losses.hip: ce_rows<true>, ce_final<true>, ce_bwd<true, acc>,
hybrid_loss_final<true> through ops.masked_cross_entropy / ops.hybrid_loss with keywords, training.train under args.sgs_hipgraph, and the two
sharded trainers) against the fp64 closed form of tests/ce_weighted_ref.py, which tests/test_ce_weighted_cpu.py holds to torch's own
F.cross_entropy.  Every floating quantity under loss_ref.bound -- 8 x the deviation of the fp32 evaluation of the closed form from the
fp64 one + 4 ulp at the quantity's largest magnitude, per case and quantity --, nan patterns exactly, and what is bitwise by reading of the
code (the regularisers' five outputs and d w, which never see the criterion; the neutral keywords) with no tolerance.  Every check prints
`RATIO <quantity> <case> <error / bound>` before it asserts.

Replays draw their own noise, so a captured step is checked as tests/test_gpu_stepgraph.py does: recomputed eagerly, and in fp64, from
the replay's own draws.

Largest error / bound per quantity measured on an MI355X over all cases of this file: masked_cross_entropy loss 0.47, d logits 0.30;
hybrid_loss ce 0.26, loss 0.37, d logits 0.17; fused against unfused (of twice the bound) ce 0.15, loss 0.20, d logits 0.05, d w bitwise;
replayed learned loss 0.15, random 0.24, both replayed losses against their eager evaluation bitwise (asserted: within the bound);
weight = ones(C) against the plain call bitwise (loss and gradient) in the four cases run, 0.25 of the bound against fp64; sharded step
loss 0.07 (edge-sharded) and 0.19 (node blocks)."""
import argparse
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ce_weighted_ref as W
import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _wdev(w):
    return None if w is None else w.to(DEV)


# ---------------------------------------------------------------------------------------------------- masked_cross_entropy(keywords)
@pytest.mark.parametrize("name", W.CASES)
def test_masked_cross_entropy_with_keywords_against_fp64(ops, name):
    c = W.make_case(name)
    r64, r32 = W.reference(name)
    ld = c["logits"].to(DEV).requires_grad_(True)
    loss = ops.masked_cross_entropy(ld, c["y"].to(DEV), c["mask"].to(DEV), weight=_wdev(c["w"]), label_smoothing=c["eps"])
    (gl,) = torch.autograd.grad(loss * R.G, (ld,))
    _check(name, "wce", loss, r64["loss"], R.bound(r64["loss"], r32["loss"]))
    _check(name, "wce_dlogits", gl, r64["dlogits"], R.bound(r64["dlogits"], r32["dlogits"]))
    if not bool(c["mask"].any()):
        assert bool(torch.isnan(loss)) and float(gl.abs().max()) == 0.0
    elif float(r64["den"]) == 0.0:
        assert bool(torch.isnan(loss)) and bool(torch.isnan(gl[c["mask"].to(DEV)]).all())
    else:
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(gl).all())
    if c["C"] == 1 and float(r64["den"]) != 0.0:
        assert float(loss.detach()) == 0.0 and float(gl.abs().max()) == 0.0        # every term vanishes


# ---------------------------------------------------------------------------------------------------- neutral keywords
@pytest.mark.parametrize("name", ["N200_C41_eps0.0_wnone_m60", "N130_C70_eps0.0_wnone_m60", "N63_C5_eps0.0_wnone_mone", "N7_C2_eps0.0_wnone_mnone"])
def test_neutral_keywords_are_the_plain_call_bitwise_and_a_weight_of_ones_within_the_bound(ops, name):
    c = W.make_case(name)
    r64, r32 = W.reference(name)
    y, m = c["y"].to(DEV), c["mask"].to(DEV)

    def run(**kw):
        ld = c["logits"].to(DEV).requires_grad_(True)
        loss = ops.masked_cross_entropy(ld, y, m, **kw)
        return loss.detach(), torch.autograd.grad(loss * R.G, (ld,))[0]
    l0, g0 = run()
    l1, g1 = run(weight=None, label_smoothing=0.0)
    assert torch.equal(_bits(l0.reshape(1)), _bits(l1.reshape(1))) and torch.equal(_bits(g0), _bits(g1))
    l2, g2 = run(weight=torch.ones(c["C"], device=DEV))
    bl, bg = R.bound(r64["loss"], r32["loss"]), R.bound(r64["dlogits"], r32["dlogits"])
    _check(name, "ones_vs_plain", l2, l0.double().cpu(), bl)
    _check(name, "ones_vs_plain_dlogits", g2, g0.double().cpu(), bg)
    _check(name, "ones_vs_fp64", l2, r64["loss"], bl)
    print(f"BITWISE ones_vs_plain {name} loss={bool(torch.equal(_bits(l0.reshape(1)), _bits(l2.reshape(1))))} dlogits={bool(torch.equal(_bits(g0), _bits(g2)))}")


# ---------------------------------------------------------------------------------------------------- hybrid_loss(keywords)
_HY_W = {"rand_0.1": ("rand", 0.1), "none_0.1": (None, 0.1), "rand_0.0": ("rand", 0.0), "zero_1.0": ("zero", 1.0)}


def _hy_weight(kind, C, seed):
    if kind is None:
        return None
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(C, generator=g) * 4.8 + 0.2
    if kind == "zero":
        w[C // 2] = 0.0
    return w


@pytest.mark.parametrize("wk", list(_HY_W))
@pytest.mark.parametrize("name", R.FUSED_CASES)
def test_hybrid_loss_with_keywords(ops, name, wk):
    """out[0..4] and d w bitwise the plain call's; out[5], out[6] and d logits against fp64; fused against unfused within twice the bound."""
    c = R.make_case(name)
    kind, eps = _HY_W[wk]
    w = _hy_weight(kind, c["C"], 17 + c["C"])
    tag = f"{name}/{wk}"
    y, m, sei = c["y"].to(DEV), c["mask"].to(DEV), c["sei"].to(DEV).contiguous()
    kw = dict(weight=_wdev(w), label_smoothing=eps)

    def leaves():
        return c["logits"].to(DEV).requires_grad_(True), c["w"].to(DEV).requires_grad_(True)
    ld, wd = leaves()
    loss_p, out_p = ops.hybrid_loss(ld, y, m, wd, sei, c["c1"], c["c2"])
    _, gw_p = torch.autograd.grad(loss_p * R.G, (ld, wd))
    ld, wd = leaves()
    loss, out = ops.hybrid_loss(ld, y, m, wd, sei, c["c1"], c["c2"], **kw)
    gl, gw = torch.autograd.grad(loss * R.G, (ld, wd))
    assert torch.equal(_bits(out[:5]), _bits(out_p[:5])) and torch.equal(_bits(gw), _bits(gw_p))          # the regularisers do not see the criterion
    assert torch.equal(_bits(loss.reshape(1)), _bits(out[6:7]))
    # fp64 / fp32 closed forms: the regularisers' share from loss_ref (the case with an empty mask has no cross-entropy share in d logits)
    wc = dict(logits=c["logits"], y=c["y"], mask=c["mask"], w=w, eps=eps)
    ref = {}
    for dt in (torch.float64, torch.float32):
        full, reg_only, ce = R.closed_form(c, dt), R.closed_form(dict(c, mask=torch.zeros_like(c["mask"])), dt), W.closed_form(wc, dt)
        ref[dt] = dict(ce=ce["loss"], loss=ce["loss"] + full["out7"][4], dlogits=reg_only["dlogits"] + ce["dlogits"])
    r64, r32 = ref[torch.float64], ref[torch.float32]
    bd = {k: R.bound(r64[k], r32[k]) for k in r64}
    _check(tag, "hy_ce", out[5], r64["ce"], bd["ce"])
    _check(tag, "hy_loss", out[6], r64["loss"], bd["loss"])
    _check(tag, "hy_dlogits", gl, r64["dlogits"], bd["dlogits"])
    # unfused: masked_cross_entropy(keywords) + edge_regularizers
    ld, wd = leaves()
    ce_u = ops.masked_cross_entropy(ld, y, m, **kw)
    reg, terms = ops.edge_regularizers(wd, ld, sei, y, m, c["c1"], c["c2"])
    gl_u, gw_u = torch.autograd.grad((ce_u + reg) * R.G, (ld, wd), allow_unused=True)
    assert torch.equal(_bits(out[:5]), _bits(terms))
    _check(tag, "hy_fused_vs_unfused_ce", out[5], ce_u.detach().double().cpu(), 2 * bd["ce"])
    _check(tag, "hy_fused_vs_unfused_loss", out[6], (ce_u + reg).detach().double().cpu(), 2 * bd["loss"])
    _check(tag, "hy_fused_vs_unfused_dlogits", gl, gl_u.double().cpu(), 2 * bd["dlogits"])
    _check(tag, "hy_fused_vs_unfused_dw", gw, gw_u.double().cpu(), 2 * R.bounds(name)["dw"])


def test_hybrid_loss_neutral_keywords_are_the_plain_call_bitwise(ops):
    c = R.make_case("N257_C41_q5000")
    y, m, sei = c["y"].to(DEV), c["mask"].to(DEV), c["sei"].to(DEV).contiguous()
    res = []
    for kw in ({}, dict(weight=None, label_smoothing=0.0)):
        ld, wd = c["logits"].to(DEV).requires_grad_(True), c["w"].to(DEV).requires_grad_(True)
        loss, out = ops.hybrid_loss(ld, y, m, wd, sei, c["c1"], c["c2"], **kw)
        res.append((out, *torch.autograd.grad(loss * R.G, (ld, wd))))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- through train / captured graphs
def _args(**kw):
    a = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", edge_mlp_type="GCN", conditional=True, sparse_edge_mlp=True, t_init=0.7,
                           t_min=0.5, degree_bias_coef=0.3, reg1=True, reg2=True, regularizer1_coef=1.0, consist_reg_coef=0.5,
                           hybrid_checkpoint=False, drop_rate=0.0, lr=1e-2)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _partition(S):
    return S.synthetic_graph(300, 21000, 16, 5, seed=3, train_frac=0.5, device=DEV)


def _model(S, p_drop=0.0):
    torch.manual_seed(3)
    S.fix_seeds(3)
    m = S.GNNModel(16, 32, 5, dropout_prob=p_drop, edge_mlp_type="GCN").to(DEV)
    og = torch.optim.Adam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-2)
    oe = torch.optim.Adam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-2)
    return m, og, oe


_W5 = (0.2, 5.0, 1.0, 0.3, 3.0)


def test_train_replays_captured_steps_under_a_weighted_smoothed_criterion():
    import sgs_gnn_amd as S
    b = _partition(S)
    q = b.edge_index.shape[1] // 5
    m, og, oe = _model(S)
    w = torch.tensor(_W5, device=DEV)
    crit = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)
    a = _args(sgs_hipgraph=True)
    losses = [S.train(a, ep, 10, m, og, oe, None, crit, [b], q=q)[0] for ep in range(4)]
    sg = getattr(m, "_sgs_stepgraphs", None)
    assert sg is not None, "the weighted criterion fell back to eager steps"
    # the RNG epoch starts at 1 with the first capture and every replayed backward ticks it: all four steps were replays
    assert sg.captures >= 1 and sg.host_epoch == 5 and int(sg.epoch_word.item()) == 5
    assert all(torch.isfinite(torch.tensor(v)) for v in losses), losses
    caps = sg.captures
    w.mul_(2)                                                             # in place: read through the same pointer, nothing is captured again
    assert torch.isfinite(torch.tensor(S.train(a, 4, 10, m, og, oe, None, crit, [b], q=q)[0]))
    assert m._sgs_stepgraphs is sg and sg.captures == caps and sg.host_epoch == 6
    crit2 = torch.nn.CrossEntropyLoss(weight=w.clone(), label_smoothing=0.1)          # another weight tensor: the captures are rebuilt
    S.train(a, 5, 10, m, og, oe, None, crit2, [b], q=q)
    sg2 = m._sgs_stepgraphs
    assert sg2 is not sg and sg2.captures >= 1
    crit3 = torch.nn.CrossEntropyLoss(weight=crit2.weight, label_smoothing=0.2)       # the same tensor, another smoothing: rebuilt as well
    S.train(a, 6, 10, m, og, oe, None, crit3, [b], q=q)
    assert m._sgs_stepgraphs is not sg2


def test_captured_step_equals_its_eager_and_fp64_recomputation_and_follows_the_weight_in_place(ops):
    import sgs_gnn_amd as S
    from sgs_gnn_amd.stepgraph import StepGraphs
    from test_gpu_stepgraph import _check_sampled_replay, _kept
    b = _partition(S)
    q = b.edge_index.shape[1] // 5
    m, og, oe = _model(S)
    w = torch.tensor(_W5, device=DEV)
    eps = 0.1
    crit = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps)
    a = _args()
    sg = StepGraphs.attach(m, "hybrid", a, crit, q, False, loader=[b])
    sg.debug_keep = True
    y, mask = b.y.cpu(), b.train_mask.cpu()
    try:
        sg.step(b, 0)
        for p in m.parameters():
            p.grad = None
        c = next(s_ for s_ in sg.slots[True] if s_.live is b)
        caps = sg.captures

        def replay(tag):
            sg.replay_g1(c)
            k = _kept(c, b)
            cnt = c.cbuf.tolist()
            c.g2l.replay()
            gl, ll = {i: g.clone() for i, g in c.grads_l.items()}, c.loss_l.clone()
            c.g2r.replay()
            gr, lr_ = {i: g.clone() for i, g in c.grads_r.items()}, c.loss_r.clone()
            torch.cuda.synchronize()
            assert sg.captures == caps
            wc = w.cpu()
            hc = dict(logits=k["learned_out"].cpu(), w=k["w"].cpu(), y=y, mask=mask, sei=k["sampled_edge_index"].cpu(), c1=1.0, c2=0.5)
            tot, rnd, old = {}, {}, {}
            for dt in (torch.float64, torch.float32):
                reg = R.closed_form(hc, dt)["out7"][4]
                tot[dt] = W.closed_form(dict(logits=hc["logits"], y=y, mask=mask, w=wc, eps=eps), dt)["loss"] + reg
                old[dt] = W.closed_form(dict(logits=hc["logits"], y=y, mask=mask, w=torch.tensor(_W5), eps=eps), dt)["loss"] + reg
                rnd[dt] = W.closed_form(dict(logits=k["random_out"].cpu(), y=y, mask=mask, w=wc, eps=eps), dt)["loss"]
            bd = R.bound(tot[torch.float64], tot[torch.float32])
            _check(tag, "replayed_learned_loss", ll, tot[torch.float64], bd)
            _check(tag, "replayed_random_loss", lr_, rnd[torch.float64], R.bound(rnd[torch.float64], rnd[torch.float32]))
            eager = ops.hybrid_loss(k["learned_out"], b.y, b.train_mask, k["w"], k["sampled_edge_index"], 1.0, 0.5, weight=w, label_smoothing=eps)[0]
            _check(tag, "replayed_vs_eager_loss", ll, eager.double().cpu(), bd)
            print(f"BITWISE replayed_vs_eager_loss {tag} {bool(torch.equal(_bits(ll.reshape(1)), _bits(eager.reshape(1))))}")
            eager_r = ops.masked_cross_entropy(k["random_out"], b.y, b.train_mask, weight=w, label_smoothing=eps)
            _check(tag, "replayed_vs_eager_random_loss", lr_, eager_r.double().cpu(), R.bound(rnd[torch.float64], rnd[torch.float32]))
            # the whole step -- outputs, both losses, every parameter gradient of both branches -- recomputed eagerly from the replay's draws
            _check_sampled_replay(S, m, a, crit, b, q, "hybrid", k, cnt, gl, ll, gr, lr_)
            for p in m.parameters():
                p.grad = None
            return abs(float(tot[torch.float64] - old[torch.float64])), bd
        replay("as captured")
        w.mul_(2)                                      # a weighted mean: the value does not move, the replay must still agree
        replay("w doubled in place")
        w.mul_(torch.tensor([4.0, 0.25, 1.0, 3.0, 0.5], device=DEV))
        moved, bd = replay("w reshaped in place")
        assert moved > 100 * bd, (moved, bd)           # the stale weight would miss the bound by far
    finally:
        sg.release()


# ---------------------------------------------------------------------------------------------------- sharded trainers (world size 1)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_SH_EPS = 0.1


def _sharded_worker(rank, world, port, q_out):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from importlib import import_module
        import sgs_gnn_amd as S
        sh = import_module("sgs_gnn_amd.sharded")
        b = S.synthetic_graph(300, 21000, 16, 5, seed=3, train_frac=0.5, device=DEV)
        torch.manual_seed(0)
        m = S.GNNModel(16, 64, 5, dropout_prob=0.3, edge_mlp_type="GCN").to(DEV)
        # a fresh model's logits are near zero, where every row's loss is ln C whatever its class and a weighted mean equals the plain one:
        # a class-dependent output bias makes the row losses differ by class, so that the class weights move the mean
        m.gcn2.bias.data.copy_(torch.tensor([2.0, -2.0, 1.0, -1.0, 0.0]))
        og = torch.optim.Adam([p for n, p in m.named_parameters() if "gcn" in n], lr=1e-3)
        oe = torch.optim.Adam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-3)
        # no gate and no regulariser: the step's loss IS the criterion on learned_out
        args = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", conditional=False, sparse_edge_mlp=True, t_init=0.7, t_min=0.5,
                                  degree_bias_coef=0.3, reg1=False, reg2=False, regularizer1_coef=1.0, consist_reg_coef=0.5, hybrid_checkpoint=False)
        crit = torch.nn.CrossEntropyLoss(weight=torch.tensor(_W5, device=DEV), label_smoothing=_SH_EPS)
        shard = sh.EdgeShard(b, rank, world)
        q = b.edge_index.shape[1] // 5
        S.fix_seeds(5)
        out = dict(y=b.y.cpu().numpy(), mask=b.train_mask.cpu().numpy())
        for name, fn in (("edge", sh.train_step_sharded), ("block", sh.train_step_blocksharded)):
            tr = fn(args, m, shard, og, oe, crit, q)
            out[name] = dict(loss=float(tr["loss"]), logits=tr["learned_out"].cpu().numpy(), upd=bool(tr["update_edge_mlp"]))
        refused = []
        for fn in (sh.train_step_sharded, sh.train_step_blocksharded):
            try:
                fn(args, m, shard, og, oe, torch.nn.NLLLoss(), q)
            except NotImplementedError as e:
                refused.append(str(e))
        out["refused"] = refused
        q_out.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_sharded_trainers_train_on_the_weighted_loss():
    ctx = mp.get_context("spawn")
    qq = ctx.Queue()
    p = ctx.Process(target=_sharded_worker, args=(0, 1, _free_port(), qq))
    p.start()
    _, got = qq.get(timeout=300)
    p.join(120)
    assert p.exitcode == 0
    y, mask = torch.from_numpy(got["y"]), torch.from_numpy(got["mask"])
    for name in ("edge", "block"):
        o = got[name]
        assert o["upd"]
        base = dict(logits=torch.from_numpy(o["logits"]), y=y, mask=mask)
        wc = dict(base, w=torch.tensor(_W5), eps=_SH_EPS)
        r64, r32 = W.closed_form(wc)["loss"], W.closed_form(wc, torch.float32)["loss"]
        plain = W.closed_form(dict(base, w=None, eps=0.0))["loss"]
        bd = R.bound(r64, r32)
        assert abs(float(r64 - plain)) > 100 * bd, (float(r64), float(plain), bd)          # the unweighted loss is far outside the bound
        _check(name, "sharded_step_loss", torch.tensor(o["loss"]), r64, bd)
    assert len(got["refused"]) == 2 and "train_step_sharded" in got["refused"][0] and "train_step_blocksharded" in got["refused"][1]
    assert all("NLLLoss" in s for s in got["refused"])
