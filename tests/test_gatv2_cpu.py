"""CPU: the GATv2 head (GATModel(..., gat_v2=True) = PyG 2.3.1 GAT(..., v2=True)) -- the two fp64 restatements of tests/gatv2_ref.py against
each other, construction and validation, state_dict keys, the unchanged default, the new C-ABI entries (workspace query and argument
validation run without a GPU) and the routing (serial ensemble evaluation, no sharded trainers)."""
import argparse
import os
import sys
from importlib import import_module

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gatv2_ref as R  # noqa: E402
from test_gpu_gat_edge import _weights  # noqa: E402
from test_gpu_gat_heads import CASES, _graph  # noqa: E402

pytestmark = []          # the imported modules' gpu mark does not apply here

V2_CASES = CASES + R.EXTRA_CASES


def _rel(a, r):
    if r.numel() == 0:
        return 0.0 if a.shape == r.shape else float("inf")
    return float((a - r).abs().max()) / (float(r.abs().max()) + 1e-300)


@pytest.mark.parametrize("variant", ["plain", "weights", "weights_masks"])
@pytest.mark.parametrize("N,E,Fin,K,C,concat", V2_CASES)
def test_edge_list_and_dense_restatements_agree(N, E, Fin, K, C, concat, variant):
    ei, g = _graph(N, E, N + K * C)
    dt = torch.float64
    x = torch.randn(N, Fin, generator=g, dtype=dt)
    w = _weights(E, g).double() if variant != "plain" else None
    D = K * C
    P = [torch.randn(D, Fin, generator=g, dtype=dt) * 0.4, torch.randn(D, generator=g, dtype=dt) * 0.2,
         torch.randn(D, Fin, generator=g, dtype=dt) * 0.4, torch.randn(D, generator=g, dtype=dt) * 0.2,
         torch.randn(K, C, generator=g, dtype=dt), torch.randn(D if concat else C, generator=g, dtype=dt) * 0.3,
         torch.randn(D, 1, generator=g, dtype=dt)]
    kw = {}
    if variant == "weights_masks":
        kw = dict(keep_e=torch.rand(E, K, generator=g) > 0.3, keep_l=torch.rand(N, K, generator=g) > 0.3, p=0.3)
    gy = torch.randn(N, D if concat else C, generator=g, dtype=dt)
    res = []
    for layer in (R.gatv2_layer, R.gatv2_layer_dense):
        leaves = [t.clone().requires_grad_(True) for t in [x] + ([w] if w is not None else []) + P]
        xx = leaves[0]
        ww = leaves[1] if w is not None else None
        out = layer(xx, ei, ww, *leaves[-7:], K, C, concat, **kw)
        out.backward(gy)
        grads = [torch.zeros_like(t) if t.grad is None else t.grad for t in leaves]
        if w is None:
            assert leaves[-1].grad is None or float(leaves[-1].grad.abs().max()) == 0.0      # lin_edge is unused without weights
        res.append([out.detach()] + grads)
    assert len(res[0]) == len(res[1])
    for a, b in zip(*res):
        assert _rel(a, b) < 1e-10 or float(b.abs().max()) == 0.0 == float(a.abs().max())
    if w is not None and E > 8:
        gw = res[0][2]
        loops = ei[0] == ei[1]
        assert bool(loops.any()) and float(gw[loops].abs().max()) == 0.0 and float(gw.abs().max()) > 0


def test_constructor_validation_and_keyword_only_argument():
    import sgs_gnn_amd as S
    from sgs_gnn_amd.model import GAT, GATv2Conv
    for bad in (0, 17, -1):
        with pytest.raises(ValueError):
            GATv2Conv(7, 4, heads=bad)
    for bad in (17, -1):
        with pytest.raises(ValueError):
            S.GATModel(12, 16 * 17, 5, gat_heads=bad, gat_v2=True)
    for bad in (0, 2, 3):
        with pytest.raises(ValueError):
            GATv2Conv(7, 4, heads=2, edge_dim=bad)
    with pytest.raises(ValueError, match="divisible"):
        S.GATModel(12, 30, 5, gat_heads=4, gat_v2=True)
    with pytest.raises(ValueError, match="divisible"):
        GAT(12, 30, 2, 5, heads=4, v2=True)
    with pytest.raises(TypeError):
        S.GATModel(12, 16, 5, 0.3, 8, "MLP", 4, True, True)               # the head's options are keyword-only
    m = S.GATModel(12, 16, 5, gat_heads=4, gat_edge_weight=True, gat_v2=True)
    assert m.gat_v2 is True and m.GAT.v2 is True and all(isinstance(c, GATv2Conv) and c.edge_dim == 1 for c in m.GAT.convs)
    c0, c1 = m.GAT.convs
    assert (c0.heads, c0.out_channels, c0.concat) == (4, 4, True) and (c1.heads, c1.out_channels, c1.concat) == (4, 5, False)
    d = S.GATModel(12, 16, 5)
    assert d.gat_v2 is False and not any(isinstance(c, GATv2Conv) for c in d.GAT.convs)


V2_KEYS = ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")


@pytest.mark.parametrize("K", [1, 4, 16])
def test_state_dict_keys_shapes_and_init(K):
    import sgs_gnn_amd as S
    torch.manual_seed(0)
    keys = lambda m: {k for k in m.state_dict() if k.startswith("GAT.")}
    m = S.GATModel(12, 32, 5, gat_heads=K, gat_v2=True)
    assert keys(m) == {f"GAT.convs.{l}.{k}" for l in (0, 1) for k in V2_KEYS} and len(keys(m)) == 12
    e = S.GATModel(12, 32, 5, gat_heads=K, gat_v2=True, gat_edge_weight=True)
    assert keys(e) == keys(m) | {f"GAT.convs.{l}.lin_edge.weight" for l in (0, 1)} and len(keys(e)) == 14
    sd = e.state_dict()
    for l, Fin, C, width in ((0, 12, 32 // K, 32), (1, 32, 5, 5)):
        g = lambda k: sd[f"GAT.convs.{l}.{k}"]
        for side in ("lin_l", "lin_r"):
            assert tuple(g(f"{side}.weight").shape) == (K * C, Fin) and tuple(g(f"{side}.bias").shape) == (K * C,)
            assert 0 < float(g(f"{side}.weight").abs().max()) <= (6.0 / (Fin + K * C)) ** 0.5            # glorot
            assert float(g(f"{side}.bias").abs().max()) == 0.0
        assert not torch.equal(g("lin_l.weight"), g("lin_r.weight"))                                  # share_weights = False
        assert tuple(g("att").shape) == (1, K, C) and 0 < float(g("att").abs().max()) <= (6.0 / (K + C)) ** 0.5
        assert tuple(g("bias").shape) == (width,) and float(g("bias").abs().max()) == 0.0
        assert tuple(g("lin_edge.weight").shape) == (K * C, 1) and 0 < float(g("lin_edge.weight").abs().max()) <= (6.0 / (1 + K * C)) ** 0.5
        assert e.GAT.convs[l].lin_edge.bias is None


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("edge", [False, True])
def test_default_model_is_the_model_without_the_keyword(K, edge):
    import sgs_gnn_amd as S
    torch.manual_seed(11)
    a = S.GATModel(12, 16, 5, gat_heads=K, gat_edge_weight=edge).state_dict()
    torch.manual_seed(11)
    b = S.GATModel(12, 16, 5, gat_heads=K, gat_edge_weight=edge, gat_v2=False).state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not any("lin_l" in k or "lin_r" in k for k in b)


V2_EXPORTS = ("sgs_gatv2_alpha_heads_fwd", "sgs_gatv2_alpha_heads_bwd_workspace_bytes", "sgs_gatv2_alpha_heads_bwd", "sgs_gatv2_dxl_heads")


def test_header_declares_the_entry_points_and_the_workspace_query_runs_on_the_cpu():
    import sgs_gnn_amd
    protos = sgs_gnn_amd._lib.parse_header()
    L = sgs_gnn_amd._lib.lib()
    for name in V2_EXPORTS:
        assert name in protos and hasattr(L, name), name
    assert {"xl", "xr", "att", "edge_w", "lin_edge", "loop_w", "loop_inv_cnt"} <= set(protos["sgs_gatv2_alpha_heads_fwd"][2])
    assert {"dw_add", "g_logit", "g_loop", "d_xr", "d_att", "d_lin_edge", "d_edge_w", "ws", "ws_bytes"} <= set(protos["sgs_gatv2_alpha_heads_bwd"][2])
    assert {"g_logit", "g_loop", "accumulate", "d_xl"} <= set(protos["sgs_gatv2_dxl_heads"][2])
    q = L.sgs_gatv2_alpha_heads_bwd_workspace_bytes
    for N, K, C in ((1013, 8, 32), (33869, 8, 32), (33869, 1, 256), (40, 16, 65), (1, 1, 1), (0, 4, 4)):
        assert q(N, K, C) >= 2 * K * C * 4                    # at least one workgroup's partial rows of d att and d lin_edge
    assert q(10 ** 6, 8, 32) >= q(1013, 8, 32)
    assert q(33869, 8, 32) < 64 << 20                         # partials per workgroup, not per row
    assert q(10, 0, 4) > 0 and q(-5, 4, 4) > 0                # bad sizes: a harmless size, the launch entry reports them


def test_argument_validation_reports_through_the_error_channel():
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()

    def fwd(N, K, C, p=0.0):
        return L.sgs_gatv2_alpha_heads_fwd(None, None, None, None, None, N, K, C, 0, None, None, None, 0.2, p, 0, 0, None, None, None, None, None,
                                           None, None)

    def bwd(N, K, C, p=0.0):
        return L.sgs_gatv2_alpha_heads_bwd(None, None, None, None, None, None, None, N, K, C, 0, None, None, None, 0.2, p, 0, 0, None, None, None,
                                           None, None, None, None, None, None, None, None, None, 0, None)

    def dxl(N, K, C, p=0.0):
        return L.sgs_gatv2_dxl_heads(None, None, None, None, None, None, None, None, N, K, C, 0, None, None, None, 0.2, 0, None, None)

    for f in (fwd, bwd, dxl):
        for K in (0, 17):
            assert f(10, K, 4) == -1 and b"unsupported heads" in L.sgs_last_error()
        assert f(10, 4, 0) == -1 and b"unsupported heads" in L.sgs_last_error()
        assert f(-1, 4, 4) == -1 and b"bad arguments" in L.sgs_last_error()
        assert f(0, 8, 4) == 0 and f(0, 1, 3) == 0                                  # N = 0: validates and returns
        assert f(10, 8, 4) == -1 and b"null" in L.sgs_last_error() and b"pointer" in L.sgs_last_error()
    for f in (fwd, bwd):
        assert f(10, 4, 4, p=1.0) == -1 and b"bad arguments" in L.sgs_last_error()


def test_v2_model_takes_the_serial_evaluation_loop_whatever_the_opt_ins():
    import sgs_gnn_amd as S
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    args = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True)
    for kw in ({}, {"gat_heads": 8}, {"gat_edge_weight": True}, {"gat_heads": 4, "gat_edge_weight": True}):
        assert ev._batched_ok(args, S.GATModel(12, 16, 5, gat_v2=True, **kw), 11) is False
        assert ev._batched_ok(args, S.GATModel(12, 16, 5, gat_v2=False, **kw), 11) is True


def test_sharded_trainers_refuse_the_v2_head():
    import sgs_gnn_amd as S
    sh = import_module("sgs_gnn_amd.sharded")
    m = S.GATModel(6, 8, 3, edge_mlp_type="GCN", gat_heads=2, gat_v2=True)
    for fn in (sh.train_step_sharded, sh.train_step_blocksharded):
        with pytest.raises(NotImplementedError, match="gat_v2"):
            fn(None, m, None, None, None, None, 5)
    with pytest.raises(NotImplementedError, match="gat_v2"):
        sh.sharded_evaluate_forward(None, m, None, 5)


def test_no_cpu_fallback_for_the_v2_layer():
    import sgs_gnn_amd as S
    ei = torch.randint(0, 10, (2, 40))
    m = S.GATModel(6, 8, 3, gat_heads=2, gat_edge_weight=True, gat_v2=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(S.Batch(x=torch.randn(10, 6), edge_index=ei), ei, torch.rand(40))


def test_reference_on_a_hand_sized_graph():
    """gatv2_layer against the definition written out by hand: 3 nodes, edges 0->2 (w 0.5), 1->2 (w 0), 1->2 again (w 1), 2->2 (removed),
    one head of one channel, lin_l = 1 (bias 0.1), lin_r = -0.5 (bias 0): node 2's loop carries the mean 0.5 of its three remaining
    in-edges, nodes 0 and 1 (no in-edges) carry 0 and return their own x_l."""
    ei = torch.tensor([[0, 1, 1, 2], [2, 2, 2, 2]])
    w = torch.tensor([0.5, 0.0, 1.0, 9.0], dtype=torch.float64)
    xs = (1.0, 2.0, -1.0)
    x = torch.tensor([[v] for v in xs], dtype=torch.float64)
    one = torch.ones(1, 1, dtype=torch.float64)
    t = lambda v: torch.tensor([v], dtype=torch.float64)
    le, a = 0.7, -1.3
    out = R.gatv2_layer(x, ei, w, one, t(0.1), -0.5 * one, t(0.0), a * one, t(0.0), le * one, 1, 1, True)
    lr = lambda v: v if v > 0 else 0.2 * v
    xl, xr = [v + 0.1 for v in xs], [-0.5 * v for v in xs]
    lg = [a * lr(xl[0] + xr[2] + 0.5 * le), a * lr(xl[1] + xr[2] + 0.0), a * lr(xl[1] + xr[2] + 1.0 * le), a * lr(xl[2] + xr[2] + 0.5 * le)]
    e = torch.tensor(lg, dtype=torch.float64).exp()
    al = e / e.sum()
    want2 = float(al[0] * xl[0] + al[1] * xl[1] + al[2] * xl[1] + al[3] * xl[2])
    assert abs(float(out[2, 0]) - want2) < 1e-12
    assert abs(float(out[0, 0]) - xl[0]) < 1e-12 and abs(float(out[1, 0]) - xl[1]) < 1e-12       # only their loops
    dense = R.gatv2_layer_dense(x, ei, w, one, t(0.1), -0.5 * one, t(0.0), a * one, t(0.0), le * one, 1, 1, True)
    assert float((dense - out).abs().max()) < 1e-12
