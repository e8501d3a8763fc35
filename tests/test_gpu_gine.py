"""GPU: the GINE head (GINModel(gin_edge_weight=True): PyG 2.3.1 GIN built from GINEConv(edge_dim=1) with the sampled edge weight as the
attribute) on the gathering kernels of csrc/gine.hip, against tests/gine_ref.py (fp64, edge-list form, torch autograd).  Tolerances are
tests/test_gpu_gat_heads.py's: forward < 1e-5, every gradient < 1e-4, max-abs error over max-abs reference.  The seeded inputs come from
gine_ref.layer_case / head_case, whose pre-activations are all further than 1e-4 from zero in fp64 (tests/test_gine_cpu.py checks it):
the kernels and the reference then take the same ReLU branch everywhere, and the gradients are comparable at all.  Third-party layer
restated from its published algorithm: parity with PyG itself unpinned."""
import argparse
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gine_ref as R  # noqa: E402
from test_gine_cpu import head_keeps  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 0.25                                   # a diagonal other than 1


def rel(a, r):
    a, r = a.detach().double().cpu(), r.detach().double().cpu()
    if r.numel() == 0:
        return 0.0 if a.shape == r.shape else float("inf")
    den = float(r.abs().max())
    err = float((a - r).abs().max())
    return err / den if den > 0 else err


class _Data:
    pass


@functools.lru_cache(maxsize=None)
def _layer_ref(case, weights):
    """The fp64 reference of one layer case, computed once and shared: (z, out, gradients by name)."""
    c = R.layer_case(case)
    names = ["x", "a", "b", "W0", "b0", "W1", "b1"] + (["w"] if weights else [])
    L = {k: c[k].double().clone().requires_grad_(True) for k in names}
    z = R.gine_aggregate(L["x"], c["ei"], L.get("w"), L["a"], L["b"], 1.0 + EPS)
    out = R.gine_layer(L["x"], c["ei"], L.get("w"), L["a"], L["b"], L["W0"], L["b0"], L["W1"], L["b1"], diag=1.0 + EPS)
    out.backward(c["gy"].double())
    return z.detach(), out.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in L.items()}


def _conv(c, eps=EPS):
    from sgs_gnn_amd.model import GINEConv
    conv = GINEConv(c["D"], c["O"], eps=eps)
    with torch.no_grad():
        conv.lin.weight.copy_(c["a"][:, None])
        conv.lin.bias.copy_(c["b"])
        for lin, W, b in ((conv.nn.lins[0], c["W0"], c["b0"]), (conv.nn.lins[1], c["W1"], c["b1"])):
            lin.weight.copy_(W)
            lin.bias.copy_(b)
    return conv.to(DEV)


def _run_layer(conv, c, w, need_x=True):
    """One forward + backward -> (out, {name: gradient})."""
    for p in conv.parameters():
        p.grad = None
    xd = c["x"].to(DEV).requires_grad_(need_x)
    wd = None if w is None else w.to(DEV).requires_grad_(True)
    out = conv(xd, c["ei"].to(DEV), wd)
    out.backward(c["gy"].to(DEV))
    l0, l1 = conv.nn.lins
    g = {"a": conv.lin.weight.grad[:, 0], "b": conv.lin.bias.grad, "W0": l0.weight.grad, "b0": l0.bias.grad, "W1": l1.weight.grad,
         "b1": l1.bias.grad}
    if need_x:
        g["x"] = xd.grad
    if wd is not None:
        g["w"] = wd.grad
    return out.detach(), g


@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("case", R.LAYER_CASES, ids=R.case_id)
def test_layer_forward_backward(case, weights):
    import sgs_gnn_amd as S
    c = R.layer_case(case)
    z_ref, out_ref, g_ref = _layer_ref(case, weights)
    conv = _conv(c)
    ei = c["ei"].to(DEV)
    attr = S.ops.edge_attr(S.ops.get_graph(ei, c["N"]), c["w"].to(DEV) if weights else None)
    z = S.ops.gine_aggregate(c["x"].to(DEV), attr, conv.lin.weight, conv.lin.bias, 1.0 + EPS)
    out, g = _run_layer(conv, c, c["w"] if weights else None)
    assert tuple(out.shape) == (c["N"], c["O"]) and tuple(z.shape) == (c["N"], c["D"])
    errs = {"z": rel(z, z_ref), "out": rel(out, out_ref)}
    for k, v in g.items():
        if k == "w" and c["E"] == 0:
            assert v is None or v.numel() == 0
            continue
        errs["d " + k] = rel(v, g_ref[k])
    print("gine_layer", R.case_id(case), weights, errs)
    if weights and c["E"] > 8:
        assert float(g["w"].abs().max()) > 0
    assert errs.pop("z") < 1e-5 and errs.pop("out") < 1e-5
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


def test_first_layer_variant_writes_no_input_gradient():
    """x without requires_grad (the head's first layer): the backward is asked for no d x, and every other gradient is unchanged bitwise."""
    c = R.layer_case((120, 2500, 41, 16))
    conv = _conv(c)
    o1, g1 = _run_layer(conv, c, c["w"], need_x=True)
    o2, g2 = _run_layer(conv, c, c["w"], need_x=False)
    assert torch.equal(o1, o2) and "x" not in g2
    for k in g2:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("case", [(50, 400, 7, 6), (64, 3000, 602, 32), "star"], ids=R.case_id)
def test_zero_lin_and_nonnegative_x_is_the_plain_gin_layer(case):
    from sgs_gnn_amd.model import GINConv
    c = R.layer_case(case)
    c["x"] = c["x"].abs()
    c["a"], c["b"] = torch.zeros_like(c["a"]), torch.zeros_like(c["b"])
    conv = _conv(c)
    plain = GINConv(c["D"], c["O"], eps=EPS).to(DEV)
    plain.nn.load_state_dict(conv.nn.state_dict())
    xd, ei = c["x"].to(DEV), c["ei"].to(DEV)
    with torch.no_grad():
        want = plain(xd, ei)
        for w in (None, c["w"].to(DEV)):
            assert rel(conv(xd, ei, w), want) < 1e-5


@pytest.mark.parametrize("case", [(50, 400, 7, 6), (64, 3000, 602, 32), (300, 6000, 256, 5), "star", (8, 4000, 70, 9)], ids=R.case_id)
def test_no_weights_equal_unit_weights_bitwise(case):
    c = R.layer_case(case)
    conv = _conv(c)
    o1, g1 = _run_layer(conv, c, None)
    o2, g2 = _run_layer(conv, c, torch.ones(c["E"]))
    assert torch.equal(o1, o2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("case", [(50, 400, 7, 6), (64, 3000, 602, 32), (300, 6000, 256, 5), "star", (8, 4000, 70, 9)], ids=R.case_id)
def test_two_identical_passes_are_bitwise_equal(case):
    c = R.layer_case(case)
    conv = _conv(c)
    o1, g1 = _run_layer(conv, c, c["w"])
    g1 = {k: v.clone() for k, v in g1.items()}
    o2, g2 = _run_layer(conv, c, c["w"])
    assert torch.equal(o1, o2) and set(g1) == set(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


# ---------------------------------------------------------------------------------------------------- the two-layer head
def _head(S, c, p=0.0, flag=True):
    m = S.GINModel(R.HEAD["F"], R.HEAD["H"], R.HEAD["C"], dropout_prob=p, edge_mlp_type="GCN", gin_edge_weight=flag)
    if flag:
        missing = m.load_state_dict(c["P"], strict=False)
        assert not missing.unexpected_keys and all(not k.startswith("GIN.") or k.endswith("eps") for k in missing.missing_keys)
    data = _Data()
    data.x = c["x"].to(DEV)
    return m.to(DEV), data


def _head_ref(c, keep, weights=True):
    P = {k: v.double().clone().requires_grad_(True) for k, v in c["P"].items()}
    w = c["w"].double().requires_grad_(True) if weights else None
    out = R.gine_model(P, c["x"].double(), c["ei"], w, keep=keep, p=R.DROPOUT_P)
    out.square().sum().backward()
    return out.detach(), (w.grad if weights else None), {k: v.grad for k, v in P.items()}


def _check_head(m, data, c, ref, tag):
    out_ref, gw_ref, gp_ref = ref
    for p in m.parameters():
        p.grad = None
    wd = c["w"].to(DEV).requires_grad_(True)
    logits = m(data, c["ei"].to(DEV), wd)
    logits.square().sum().backward()
    params = dict(m.named_parameters())
    errs = {"logits": rel(logits, out_ref), "edge_weight": rel(wd.grad, gw_ref)}
    for n in gp_ref:
        errs[n] = rel(params[n].grad, gp_ref[n])
    print("gine_head", tag, errs)
    assert len(gp_ref) == 12 and float(wd.grad.abs().max()) > 0
    assert errs.pop("logits") < 1e-5
    for k, v in errs.items():
        assert v < 1e-4, (k, v)
    return wd.grad


@pytest.mark.parametrize("mode", ["train", "eval", "dropout"])
def test_two_layer_head_logits_and_gradients(mode):
    """Both layers consume the same edge weights: edge_weight.grad is the reference's sum over both layers (the second layer to finish
    adds the first one's d w on its way out).  dropout: the drawn mask is ops.dropout_keep's at the same seed, restated on the host."""
    import sgs_gnn_amd as S
    from sgs_gnn_amd import model as M
    keeps = head_keeps()
    c = R.head_case(keeps)
    m, data = _head(S, c, p=R.DROPOUT_P if mode == "dropout" else 0.0)
    m.train(mode != "eval")
    M.set_dropout_seed(R.DROPOUT_SEED)
    if mode == "dropout":
        seed = M._DropoutClock.next_seed()
        M.set_dropout_seed(R.DROPOUT_SEED)
        dev_keep = S.ops.dropout_keep(seed, M.SITE_GIN, R.HEAD["N"], R.HEAD["H"], R.DROPOUT_P, torch.device(DEV))
        assert torch.equal(dev_keep.cpu(), keeps[1])                  # the host restatement IS the mask the model draws
    _check_head(m, data, c, _head_ref(c, keeps[1] if mode == "dropout" else None), mode)
    assert M._DropoutClock.tick == (1 if mode == "dropout" else 0)    # GIN's seed accounting: one seed per training forward with p > 0


def test_first_layers_share_of_the_edge_weight_gradient():
    """With the first layer's lin zeroed and x > 0 its messages do not depend on the weights: d w is the second layer's share alone, in
    the reference and here -- and differs from the two-layer sum of the full model."""
    import sgs_gnn_amd as S
    keeps = head_keeps()
    c = R.head_case(keeps, first_lin_zero=True)
    m, data = _head(S, c)
    m.train()
    gw = _check_head(m, data, c, _head_ref(c, None), "first_lin_zero")
    # the second layer alone, by hand: its input from the model's own first layer, detached
    with torch.no_grad():
        h = torch.relu(m.GIN.convs[0](data.x, c["ei"].to(DEV), c["w"].to(DEV)))
    wd = c["w"].to(DEV).requires_grad_(True)
    m.GIN.convs[1](h, c["ei"].to(DEV), wd).square().sum().backward()
    assert rel(gw, wd.grad) < 1e-6


def test_weight_gradients_join_the_grouped_launch():
    """Under ops.deferred_weight_grads the head's four Linear weight gradients run as ONE grouped launch (N = 1000 nodes: the grouped
    kernel takes the partition-sized products, from 128 up to 1023 rows to reduce over), with the same values as the four single launches."""
    import sgs_gnn_amd as S
    ops = S.ops
    g = torch.Generator().manual_seed(8)
    N, E = 1000, 4000
    ei = torch.randint(0, N, (2, E), generator=g).to(DEV)
    torch.manual_seed(8)
    m = S.GINModel(12, 64, 5, dropout_prob=0.0, edge_mlp_type="GCN", gin_edge_weight=True).to(DEV).train()
    data = _Data()
    data.x = torch.randn(N, 12, generator=g).to(DEV)
    w = torch.rand(E, generator=g)
    L = S._lib.lib()
    assert all(L.sgs_gemm_tn_group_supported(N, *c.nn.lins[k].weight.shape) > 0 for c in m.GIN.convs for k in (0, 1))
    got = []
    for defer in (False, True):
        for p in m.parameters():
            p.grad = None
        wd = w.to(DEV).requires_grad_(True)
        loss = m(data, ei, wd).square().sum()
        before = dict(ops.GEMM_TN_LAUNCHES)
        if defer:
            with ops.deferred_weight_grads(loss):
                loss.backward()
        else:
            loss.backward()
        torch.cuda.synchronize()
        d = {k: ops.GEMM_TN_LAUNCHES[k] - before[k] for k in before}
        got.append(({n: p.grad.clone() for n, p in m.named_parameters() if n.startswith("GIN.")}, wd.grad.clone()))
        assert d == ({"single": 0, "group": 1} if defer else {"single": 4, "group": 0}), d
    for n in got[0][0]:
        assert rel(got[1][0][n], got[0][0][n]) < 1e-6, n
    assert torch.equal(got[0][1], got[1][1])


# ---------------------------------------------------------------------------------------------------- the point of the feature
def _st_args(**kw):
    a = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", conditional=True, sparse_edge_mlp=False, t_init=0.7, t_min=0.5,
                           degree_bias_coef=0.3, reg1=False, reg2=False, regularizer1_coef=1.0, consist_reg_coef=0.5)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("flag", [True, False])
def test_the_cross_entropy_reaches_the_edge_weights_only_with_the_flag(flag):
    """One learned-branch loss with both regularisers off (the loss is the cross entropy alone) on a small partition: with
    gin_edge_weight=True the sampled weights get the reference's gradient and the scorer a non-zero one; without it (today's model) the
    weights get none."""
    import sgs_gnn_amd as S
    from sgs_gnn_amd.training import learned_loss, sampled_forward
    b = S.synthetic_graph(100, 2000, 12, 5, seed=1, train_frac=0.5).to(DEV)
    q = 400
    torch.manual_seed(11)
    S.fix_seeds(0)
    m = S.GINModel(12, 16, 5, 0.0, edge_mlp_type="GCN", gin_edge_weight=flag).to(DEV).train()
    args = _st_args()
    S.ops.new_memo_scope()
    S.ops.get_pairs(b.edge_index, b.x.shape[0], build=True)
    st = sampled_forward("hybrid", args, m, b, q)
    w = st.edge_probs_for_loss
    w.retain_grad()
    loss = learned_loss(args, torch.nn.CrossEntropyLoss(), st, b)
    loss.backward()
    g = m.edge_prob_mlp.fc1.weight.grad
    assert bool(torch.isfinite(loss)) and w.numel() == q
    if not flag:
        assert w.grad is None or float(w.grad.abs().max()) == 0.0
        assert g is None or float(g.abs().max()) == 0.0
        return
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    P = {k: v.detach().cpu().double() for k, v in m.state_dict().items() if k.startswith("GIN.")}
    w64 = w.detach().cpu().double().requires_grad_(True)
    ei = st.sampled_edge_index.cpu()
    hs = []
    out = R.gine_model(P, b.x.cpu().double(), ei, w64, hidden_out=hs)
    mask = b.train_mask.cpu()
    torch.nn.functional.cross_entropy(out[mask], b.y.cpu()[mask]).backward()
    margin = min(R.min_abs_preact(b.x.cpu().double(), ei, w64.detach(), P["GIN.convs.0.lin.weight"][:, 0], P["GIN.convs.0.lin.bias"]),
                 R.min_abs_preact(hs[0], ei, w64.detach(), P["GIN.convs.1.lin.weight"][:, 0], P["GIN.convs.1.lin.bias"]))
    errs = {"logits": rel(st.learned_out, out), "loss": abs(float(loss) - float(torch.nn.functional.cross_entropy(out[mask], b.y.cpu()[mask]))),
            "edge_weight": rel(w.grad, w64.grad)}
    print("gine_learned_branch", errs, "min |pre-activation| of this draw:", margin)
    assert float(w.grad.abs().max()) > 0
    assert errs["logits"] < 1e-5 and errs["edge_weight"] < 1e-4, (errs, margin)


def test_default_is_the_model_without_the_keyword_bitwise():
    import sgs_gnn_amd as S
    from sgs_gnn_amd import model as M
    c = R.head_case()
    outs = []
    for kw in ({}, {"gin_edge_weight": False}):
        torch.manual_seed(3)
        m = S.GINModel(R.HEAD["F"], R.HEAD["H"], R.HEAD["C"], dropout_prob=0.3, edge_mlp_type="GCN", **kw).to(DEV).train()
        data = _Data()
        data.x = c["x"].to(DEV)
        M.set_dropout_seed(9)
        outs.append(m(data, c["ei"].to(DEV), c["w"].to(DEV)).detach().clone())
        assert M._DropoutClock.tick == 1
    assert torch.equal(outs[0], outs[1])


def test_training_loop_eager_and_replayed():
    """The learned step is captured as for the other heads (the model is called through model(batch, edge_index, w); every buffer of the
    layer comes from torch's allocator or ops.workspace, nothing is read back)."""
    import sgs_gnn_amd as S
    torch.manual_seed(5)
    S.fix_seeds(5)
    crit = torch.nn.CrossEntropyLoss()
    bs = [S.synthetic_graph(150, E, 24, 5, seed=11 + i, device=DEV) for i, E in enumerate([5000, 900, 4000])]
    m = S.GINModel(24, 32, 5, dropout_prob=0.3, edge_mlp_type="GCN", gin_edge_weight=True).to(DEV)
    og = S.FusedAdam([p for n, p in m.named_parameters() if "GIN" in n or "gcn" in n], lr=1e-2)
    oe = S.FusedAdam([p for n, p in m.named_parameters() if "edge_prob_mlp" in n], lr=1e-2)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    for hip in (False, True):
        a = _st_args(reg1=True, reg2=True, edge_mlp_type="GCN", sparse_edge_mlp=True, hybrid_checkpoint=False, drop_rate=0.0, lr=1e-2,
                     sgs_hipgraph=hip)
        for ep in range(3):
            loss, _, cond, tot = S.train(a, ep, 3, m, og, oe, None, crit, bs, q=1000)
            assert tot == 3 and loss == loss and abs(loss) != float("inf")
    for n, p in m.named_parameters():
        assert torch.isfinite(p).all(), n
    assert all(not torch.equal(p, before[n]) for n, p in m.named_parameters() if n.startswith("GIN."))
    assert m._sgs_stepgraphs.captures <= 4


def test_ensemble_evaluation_takes_the_serial_loop():
    import sgs_gnn_amd as S
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    torch.manual_seed(4)
    m = S.GINModel(12, 16, 5, dropout_prob=0.3, edge_mlp_type="GCN", gin_edge_weight=True).to(DEV)
    bs = [S.synthetic_graph(200, E, 12, 5, seed=21 + i, train_frac=0.4) for i, E in enumerate([4000, 1500])]
    got = {}
    for engine in (False, True):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=5)
        if engine:
            args.sgs_eval_batch, args.sgs_eval_batch_heads, args.sgs_eval_batch_variants = True, "all", True
        S.manual_seed(7)
        before = dict(ev.PATH_COUNTS)
        got[engine] = S.ensemble_evaluate(args, m, bs, DEV, q=2000, mode="learned")
        assert ev.PATH_COUNTS["serial"] == before["serial"] + 1 and ev.PATH_COUNTS["batched"] == before["batched"]
    assert len(got[True]) == 3 and got[True] == got[False]
    assert all(v == v and 0.0 <= v <= 1.0 for v in got[True])
