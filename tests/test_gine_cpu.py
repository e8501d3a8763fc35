"""CPU: the GINE head (GINModel(..., gin_edge_weight=True) = PyG 2.3.1 GIN built from GINEConv(edge_dim=1)) -- the two fp64 restatements of
tests/gine_ref.py against each other on every case tests/test_gpu_gine.py runs, the input condition of those cases, construction and
state_dict keys, the unchanged default, the new C-ABI entries (variant and workspace queries, argument validation: no GPU needed) and the
routing (serial ensemble evaluation, no sharded trainers)."""
import argparse
import os
import sys
from importlib import import_module

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gine_ref as R  # noqa: E402


def _rel(a, r):
    if r.numel() == 0:
        return 0.0 if a.shape == r.shape else float("inf")
    return float((a - r).abs().max()) / (float(r.abs().max()) + 1e-300)


def head_keeps():
    """The hidden dropout masks of the head cases: none, and the first training forward's after set_dropout_seed(R.DROPOUT_SEED)."""
    from sgs_gnn_amd import model as M
    M.set_dropout_seed(R.DROPOUT_SEED)
    seed = M._DropoutClock.next_seed()
    M.set_dropout_seed(R.DROPOUT_SEED)
    return (None, R.dropout_keep_host(seed, M.SITE_GIN, R.HEAD["N"], R.HEAD["H"], R.DROPOUT_P))


@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("case", R.LAYER_CASES, ids=R.case_id)
def test_edge_list_and_dense_restatements_agree(case, weights):
    c = R.layer_case(case)
    res = []
    for agg in (R.gine_aggregate, R.gine_aggregate_dense):
        names = ["x", "a", "b", "W0", "b0", "W1", "b1"] + (["w"] if weights else [])
        L = {k: c[k].double().clone().requires_grad_(True) for k in names}
        out = R.gine_layer(L["x"], c["ei"], L.get("w"), L["a"], L["b"], L["W0"], L["b0"], L["W1"], L["b1"], diag=1.25, aggregate=agg)
        out.backward(c["gy"].double())
        res.append([out.detach()] + [torch.zeros_like(t) if t.grad is None else t.grad for t in L.values()])
    for u, v in zip(*res):
        assert _rel(u, v) < 1e-10 or float(u.abs().max()) == 0.0 == float(v.abs().max())
    if weights and c["E"] > 8:
        assert float(res[0][-1].abs().max()) > 0


def test_two_layer_restatements_agree():
    keeps = head_keeps()
    c = R.head_case(keeps)
    res = []
    for agg in (R.gine_aggregate, R.gine_aggregate_dense):
        P = {k: v.double().clone().requires_grad_(True) for k, v in c["P"].items()}
        w = c["w"].double().requires_grad_(True)
        out = R.gine_model(P, c["x"].double(), c["ei"], w, keep=keeps[1], p=R.DROPOUT_P, aggregate=agg)
        out.square().sum().backward()
        res.append([out.detach(), w.grad] + [P[k].grad for k in sorted(P)])
    for u, v in zip(*res):
        assert _rel(u, v) < 1e-10


def test_reference_on_a_hand_sized_graph():
    """3 nodes, one column: edges 0->2 (w 0.5), 1->2 (w 2), 1->2 again (w 0), 2->2 (w 1); a = 1, b = -1, diag = 1.5."""
    ei = torch.tensor([[0, 1, 1, 2], [2, 2, 2, 2]])
    w = torch.tensor([0.5, 2.0, 0.0, 1.0], dtype=torch.float64)
    x = torch.tensor([[1.0], [-0.5], [0.25]], dtype=torch.float64)
    one = torch.ones(1, dtype=torch.float64)
    want2 = 1.5 * 0.25 + max(1.0 + 0.5 - 1, 0) + max(-0.5 + 2 - 1, 0) + max(-0.5 + 0 - 1, 0) + max(0.25 + 1 - 1, 0)
    for agg in (R.gine_aggregate, R.gine_aggregate_dense):
        z = agg(x, ei, w, one, -one, 1.5)
        assert abs(float(z[2, 0]) - want2) < 1e-12 and abs(float(z[0, 0]) - 1.5) < 1e-12 and abs(float(z[1, 0]) + 0.75) < 1e-12
        z1 = agg(x, ei, None, one, -one, 1.0)                         # w None = ones: every message is relu(x_j)
        assert abs(float(z1[2, 0]) - (0.25 + 1.0 + 0.0 + 0.0 + 0.25)) < 1e-12
    assert abs(R.min_abs_preact(x, ei, w, one, -one) - 0.25) < 1e-12


@pytest.mark.parametrize("case", R.LAYER_CASES, ids=R.case_id)
def test_input_condition_of_the_layer_cases(case):
    """No pre-activation of a seeded GPU case lies within 1e-4 of zero in fp64, with the weights as given and as ones: an fp32 kernel and
    the fp64 reference then take the same ReLU branch everywhere (a flipped branch would move a gradient term by a whole dZ)."""
    c = R.layer_case(case)
    x, a, b = c["x"].double(), c["a"].double(), c["b"].double()
    assert R.min_abs_preact(x, c["ei"], c["w"].double(), a, b) > R.MARGIN
    assert R.min_abs_preact(x, c["ei"], None, a, b) > R.MARGIN
    if c["E"] >= 8:
        ei = c["ei"]
        assert bool((ei[0] == ei[1]).any()) and torch.unique(ei, dim=1).shape[1] < ei.shape[1]      # (i, i) and duplicate edges present
    if case == "star":
        assert int(torch.bincount(ei[1]).max()) >= 700 and int(torch.bincount(ei[0]).max()) >= 700


@pytest.mark.parametrize("first_lin_zero", [False, True])
def test_input_condition_of_the_head_cases_both_layers(first_lin_zero):
    keeps = head_keeps()
    assert 0.6 < float(keeps[1].float().mean()) < 0.8
    c = R.head_case(keeps, first_lin_zero=first_lin_zero)
    P = {k: v.double() for k, v in c["P"].items()}
    x = c["x"].double()
    for keep in keeps:
        for w in (c["w"].double(), None):
            hs = []
            R.gine_model(P, x, c["ei"], w, keep=keep, p=R.DROPOUT_P, hidden_out=hs)
            if not first_lin_zero:
                assert R.min_abs_preact(x, c["ei"], w, P["GIN.convs.0.lin.weight"][:, 0], P["GIN.convs.0.lin.bias"]) > R.MARGIN
            else:
                assert float(x.min()) > R.MARGIN and float(P["GIN.convs.0.lin.weight"].abs().max()) == 0.0
            assert R.min_abs_preact(hs[0], c["ei"], w, P["GIN.convs.1.lin.weight"][:, 0], P["GIN.convs.1.lin.bias"]) > R.MARGIN


def test_layer_cases_reach_every_kernel_shape():
    """sgs_gine_variant is a pure host function: the cases take the wave-per-row kernels and both workgroup-per-row ones, at every
    vector width."""
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()
    got = set()
    for case in R.LAYER_CASES:
        c = R.layer_case(case)
        if c["N"]:
            got.add(L.sgs_gine_variant(c["N"], c["D"], c["E"], 16))
    assert {v // 1000 for v in got} == {0, 1} and {v % 100 for v in got} == {64, 4, 16}
    assert {(v // 100) % 10 for v in got} == {1, 2, 4}
    assert L.sgs_gine_variant(1013, 602, 70200, 16) == 1204 and L.sgs_gine_variant(1013, 256, 70200, 16) == 1404      # bench S3's partition
    assert L.sgs_gine_variant(33869, 128, 100000, 16) == 264 and L.sgs_gine_variant(33869, 256, 100000, 16) == 464    # bench S4's
    assert L.sgs_gine_variant(100, 256, 500, 8) == 264 and L.sgs_gine_variant(100, 256, 500, 4) == 164               # alignment
    assert L.sgs_gine_variant(100, 602, 500, 16) == 264 and L.sgs_gine_variant(100, 33, 500, 16) == 164


GIN_KEYS = ("nn.lins.0.weight", "nn.lins.0.bias", "nn.lins.1.weight", "nn.lins.1.bias", "eps")


def test_state_dict_keys_and_init():
    import sgs_gnn_amd as S
    from sgs_gnn_amd.model import GIN, GINConv, GINEConv
    keys = lambda m: {k for k in m.state_dict() if k.startswith("GIN.")}
    today = {f"GIN.convs.{l}.{k}" for l in (0, 1) for k in GIN_KEYS}
    d, f, t = S.GINModel(12, 16, 5), S.GINModel(12, 16, 5, gin_edge_weight=False), S.GINModel(12, 16, 5, gin_edge_weight=True)
    assert keys(d) == keys(f) == today
    assert keys(t) - today == {f"GIN.convs.{l}.lin.{k}" for l in (0, 1) for k in ("weight", "bias")} and today <= keys(t)
    assert set(d.state_dict()) - keys(d) == set(t.state_dict()) - keys(t)                   # the scorer's keys are untouched
    assert d.gin_edge_weight is False and t.gin_edge_weight is True
    assert all(isinstance(c, GINConv) for c in d.GIN.convs) and all(isinstance(c, GINEConv) for c in t.GIN.convs)
    sd = t.state_dict()
    for l, width in ((0, 12), (1, 16)):
        wt, bs = sd[f"GIN.convs.{l}.lin.weight"], sd[f"GIN.convs.{l}.lin.bias"]
        assert tuple(wt.shape) == (width, 1) and tuple(bs.shape) == (width,)
        assert 0 < float(wt.abs().max()) <= 1.0 and 0 < float(bs.abs().max()) <= 1.0      # torch.nn.Linear(1, width)'s default range
    with pytest.raises(TypeError):
        S.GINModel(12, 16, 5, 0.3, "MLP", True)                                            # keyword-only
    for bad in (0, 2):
        with pytest.raises(ValueError):
            GIN(12, 16, 2, 5, edge_dim=bad)
        with pytest.raises(ValueError):
            GINEConv(12, 16, edge_dim=bad)


def test_default_model_draws_the_same_parameters():
    import sgs_gnn_amd as S
    torch.manual_seed(11)
    a = S.GINModel(12, 16, 5).state_dict()
    torch.manual_seed(11)
    b = S.GINModel(12, 16, 5, gin_edge_weight=False).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_edge_weight_model_takes_the_serial_evaluation_loop_whatever_the_opt_ins():
    import sgs_gnn_amd as S
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    plain, edge = S.GINModel(12, 16, 5), S.GINModel(12, 16, 5, gin_edge_weight=True)
    for flag in (True, 3):
        for heads in (None, "all", ("GIN",), ("GCN", "GIN")):
            for variants in (None, False, True):
                args = argparse.Namespace(sgs_eval_batch=flag, sgs_eval_batch_heads=heads, sgs_eval_batch_variants=variants)
                assert ev._batched_ok(args, edge, 11) is False
                assert ev._batched_ok(args, plain, 11) is (heads is not None)              # unchanged: GIN takes the engine when selected
    assert ev._batched_ok(argparse.Namespace(), edge, 11) is False and ev._batched_ok(argparse.Namespace(), plain, 11) is False


def test_sharded_trainers_refuse_the_head():
    import sgs_gnn_amd as S
    sh = import_module("sgs_gnn_amd.sharded")
    m = S.GINModel(6, 8, 3, edge_mlp_type="GCN", gin_edge_weight=True)
    for fn in (sh.train_step_sharded, sh.train_step_blocksharded):
        with pytest.raises(NotImplementedError, match="gin_edge_weight"):
            fn(None, m, None, None, None, None, 5)
    with pytest.raises(NotImplementedError, match="gin_edge_weight"):
        sh.sharded_evaluate_forward(None, m, None, 5)


def test_no_cpu_fallback_for_the_layer():
    import sgs_gnn_amd as S
    ei = torch.randint(0, 10, (2, 40))
    m = S.GINModel(6, 8, 3, gin_edge_weight=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(S.Batch(x=torch.randn(10, 6), edge_index=ei), ei, torch.rand(40))


def test_header_declares_the_entry_points_and_the_workspace_query_runs_on_the_cpu():
    import sgs_gnn_amd
    protos = sgs_gnn_amd._lib.parse_header()
    L = sgs_gnn_amd._lib.lib()
    for name in ("sgs_gine_variant", "sgs_gine_aggregate_fwd", "sgs_gine_aggregate_bwd_workspace_bytes", "sgs_gine_aggregate_bwd"):
        assert name in protos and hasattr(L, name), name
    assert {"x", "edge_w", "a", "b", "diag", "in_ptr", "in_src", "in_eid", "z"} <= set(protos["sgs_gine_aggregate_fwd"][2])
    assert {"dz", "out_ptr", "out_dst", "out_eid", "dw_add", "d_x", "d_edge_w", "d_a", "d_b", "ws", "ws_bytes"} <= set(
        protos["sgs_gine_aggregate_bwd"][2])
    q = L.sgs_gine_aggregate_bwd_workspace_bytes
    for N, D in ((1013, 602), (33869, 128), (1, 1), (7, 5)):
        assert q(N, D) >= 2 * D * 4 * min(N, 4)
    assert q(10 ** 6, 602) == q(33869, 602) < 16 << 20            # partials per workgroup, not per row
    assert q(0, 4) > 0 and q(-5, 4) > 0 and q(4, 0) > 0          # bad sizes: a harmless size, the launch entry reports them


def test_argument_validation_reports_through_the_error_channel():
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()
    fwd = lambda N, D: L.sgs_gine_aggregate_fwd(None, None, None, None, 1.0, N, D, 0, None, None, None, None, None)
    bwd = lambda N, D: L.sgs_gine_aggregate_bwd(None, None, None, None, None, 1.0, N, D, 0, None, None, None, None, None, None, None, None,
                                                None, 0, None)
    for f in (fwd, bwd):
        assert f(-1, 4) == -1 and b"bad sizes" in L.sgs_last_error()
        assert f(10, 0) == -1 and b"bad sizes" in L.sgs_last_error()
        assert f(0, 4) == 0                                        # N = 0 without outputs: validates and returns
        assert f(10, 4) == -1 and b"null" in L.sgs_last_error()
