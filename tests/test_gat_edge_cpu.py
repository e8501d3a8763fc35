"""CPU: the edge-weighted GAT head (GATModel(..., gat_edge_weight=True) = PyG 2.3.1 GAT(..., edge_dim=1) with the edge weight as the
attribute) -- construction, state_dict keys with and without the flag, the unchanged default, the new C-ABI declarations and their error
channel, and the routing (serial ensemble evaluation, no sharded trainers).  tests/gat_edge_ref.py is checked here against its own
definition on a hand-sized graph."""
import argparse
import os
import sys
from importlib import import_module

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_edge_ref as R  # noqa: E402

TODAY_KEYS = {f"GAT.convs.{l}.{k}" for l in (0, 1) for k in ("lin_src.weight", "lin_dst.weight", "att_src", "att_dst", "bias")}
EDGE_KEYS = {f"GAT.convs.{l}.{k}" for l in (0, 1) for k in ("lin_edge.weight", "att_edge")}


def _head_keys(m):
    return {k for k in m.state_dict() if not k.startswith("edge_prob_mlp.")}


def test_constructor_and_keyword_only_argument():
    import sgs_gnn_amd as S
    m = S.GATModel(12, 16, 5, gat_heads=4, gat_edge_weight=True)
    assert m.gat_edge_weight is True and m.GAT.edge_dim == 1 and all(c.edge_dim == 1 for c in m.GAT.convs)
    d = S.GATModel(12, 16, 5)
    assert d.gat_edge_weight is False and d.GAT.edge_dim is None and not hasattr(d.GAT.convs[0], "lin_edge")
    with pytest.raises(TypeError):
        S.GATModel(12, 16, 5, 0.3, 8, "MLP", 4, True)                   # gat_heads / gat_edge_weight are keyword-only
    from sgs_gnn_amd.model import GAT, GATConv
    for bad in (0, 2, 3):
        with pytest.raises(ValueError):
            GATConv(7, 4, heads=2, edge_dim=bad)
    assert GAT(12, 16, 2, 5, heads=2, edge_dim=1).convs[1].edge_dim == 1


@pytest.mark.parametrize("K", [1, 4, 16])
def test_state_dict_keys_shapes_and_init(K):
    import sgs_gnn_amd as S
    torch.manual_seed(0)
    m = S.GATModel(12, 32, 5, gat_heads=K, gat_edge_weight=True)
    assert _head_keys(m) == TODAY_KEYS | EDGE_KEYS
    sd = m.state_dict()
    for l, C in ((0, 32 // K), (1, 5)):
        le, ae = sd[f"GAT.convs.{l}.lin_edge.weight"], sd[f"GAT.convs.{l}.att_edge"]
        assert tuple(le.shape) == (K * C, 1) and tuple(ae.shape) == (1, K, C)
        assert 0 < float(le.abs().max()) <= (6.0 / (1 + K * C)) ** 0.5      # glorot on its own shape
        assert 0 < float(ae.abs().max()) <= (6.0 / (K + C)) ** 0.5          # glorot as att_src
        assert m.GAT.convs[l].lin_edge.bias is None
    assert _head_keys(S.GATModel(12, 32, 5, gat_heads=K)) == TODAY_KEYS
    assert _head_keys(S.GATModel(12, 32, 5, gat_heads=K, gat_edge_weight=False)) == TODAY_KEYS


def test_strict_load_fails_both_ways_and_round_trips():
    import sgs_gnn_amd as S
    on, off = S.GATModel(12, 16, 5, gat_heads=2, gat_edge_weight=True), S.GATModel(12, 16, 5, gat_heads=2)
    with pytest.raises(RuntimeError):
        off.load_state_dict(on.state_dict())            # unexpected lin_edge / att_edge
    with pytest.raises(RuntimeError):
        on.load_state_dict(off.state_dict())            # missing lin_edge / att_edge
    fresh = S.GATModel(12, 16, 5, gat_heads=2, gat_edge_weight=True)
    fresh.load_state_dict(on.state_dict())
    assert all(torch.equal(v, on.state_dict()[k]) for k, v in fresh.state_dict().items())


@pytest.mark.parametrize("K", [1, 8])
def test_default_model_draws_the_same_initial_weights_as_before_the_keyword(K):
    """The edge parameters are created after today's: a model without the flag consumes the generator exactly as before."""
    import sgs_gnn_amd as S
    torch.manual_seed(11)
    a = S.GATModel(12, 16, 5, gat_heads=K).state_dict()
    torch.manual_seed(11)
    b = S.GATModel(12, 16, 5, gat_heads=K, gat_edge_weight=False).state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # and, layer by layer, today's draw order: lin_src, att_src, att_dst (the first layer of the flag-on model starts the same way)
    from sgs_gnn_amd.model import GATConv
    torch.manual_seed(5)
    c0 = GATConv(7, 4, heads=K)
    torch.manual_seed(5)
    c1 = GATConv(7, 4, heads=K, edge_dim=1)
    for k in ("lin_src.weight", "att_src", "att_dst", "bias"):
        assert torch.equal(c0.state_dict()[k], c1.state_dict()[k])


def test_edge_coef_is_the_collapsed_edge_term():
    from sgs_gnn_amd.model import GATConv
    torch.manual_seed(2)
    c = GATConv(7, 5, heads=3, edge_dim=1)
    w = torch.rand(11)
    full = (c.lin_edge(w.view(-1, 1)).view(-1, 3, 5) * c.att_edge).sum(-1)           # PyG's expression
    assert torch.allclose(full, w[:, None] * c.edge_coef()[None, :], rtol=1e-6, atol=1e-7)


EDGE_EXPORTS = ("sgs_gat_alpha_heads_edge_fwd", "sgs_gat_alpha_heads_edge_bwd_workspace_bytes", "sgs_gat_alpha_heads_edge_bwd")


def test_header_declares_the_edge_entry_points():
    import sgs_gnn_amd
    protos = sgs_gnn_amd._lib.parse_header()
    for name in EDGE_EXPORTS:
        assert name in protos, name
    assert {"edge_w", "edge_coef", "loop_w", "loop_inv_cnt"} <= set(protos["sgs_gat_alpha_heads_edge_fwd"][2])
    assert {"edge_w", "edge_coef", "dw_add", "d_edge_w", "d_edge_coef", "ws", "ws_bytes"} <= set(protos["sgs_gat_alpha_heads_edge_bwd"][2])
    L = sgs_gnn_amd._lib.lib()
    for name in EDGE_EXPORTS:
        assert hasattr(L, name)


def test_argument_validation_reports_through_the_error_channel():
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()

    def fwd(N, K):
        return L.sgs_gat_alpha_heads_edge_fwd(None, None, None, None, N, K, 0, None, None, None, 0.2, 0.0, 0, 0, None, None, None, None, None,
                                              None, None)

    def bwd(N, K):
        return L.sgs_gat_alpha_heads_edge_bwd(None, None, None, None, None, None, N, K, 0, None, None, None, 0.2, 0.0, 0, 0, None, None, None,
                                              None, None, None, None, None, None, None, None, 0, None)

    for f in (fwd, bwd):
        for K in (0, 17):
            assert f(10, K) == -1 and b"unsupported heads" in L.sgs_last_error()
        assert f(0, 8) == 0 and f(0, 1) == 0                                       # N = 0: validates and returns
        assert f(10, 8) == -1 and b"null pointer" in L.sgs_last_error()
    assert L.sgs_gat_alpha_heads_edge_bwd_workspace_bytes(1013, 8) >= 4 * 8 * ((1013 + 3) // 4)


def test_edge_weighted_model_takes_the_serial_evaluation_loop():
    import sgs_gnn_amd as S
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    args = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all")
    assert ev._batched_ok(args, S.GATModel(12, 16, 5, gat_edge_weight=True), 11) is False
    assert ev._batched_ok(args, S.GATModel(12, 16, 5, gat_edge_weight=False), 11) is True
    assert ev._batched_ok(args, S.GATModel(12, 16, 5), 11) is True


def test_sharded_trainers_refuse_the_edge_weighted_head():
    import sgs_gnn_amd as S
    sh = import_module("sgs_gnn_amd.sharded")
    m = S.GATModel(6, 8, 3, edge_mlp_type="GCN", gat_heads=2, gat_edge_weight=True)
    for fn in (sh.train_step_sharded, sh.train_step_blocksharded):
        with pytest.raises(NotImplementedError, match="gat_edge_weight"):
            fn(None, m, None, None, None, None, 5)
    with pytest.raises(NotImplementedError, match="gat_edge_weight"):
        sh.sharded_evaluate_forward(None, m, None, 5)


def test_no_cpu_fallback_for_the_edge_weighted_layer():
    import sgs_gnn_amd as S
    ei = torch.randint(0, 10, (2, 40))
    m = S.GATModel(6, 8, 3, gat_heads=2, gat_edge_weight=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(S.Batch(x=torch.randn(10, 6), edge_index=ei), ei, torch.rand(40))


def test_reference_on_a_hand_sized_graph():
    """The helper against the definition written out by hand: 3 nodes, edges 0->2 (w 0.5), 1->2 (w 0), 1->2 again (w 1), 2->2 (removed),
    one head, x' = x: node 2's loop carries the mean 0.5 of its three remaining in-edges, nodes 0 and 1 (no in-edges) carry 0."""
    ei = torch.tensor([[0, 1, 1, 2], [2, 2, 2, 2]])
    w = torch.tensor([0.5, 0.0, 1.0, 9.0], dtype=torch.float64)
    x = torch.tensor([[1.0], [2.0], [-1.0]], dtype=torch.float64)
    one = torch.ones(1, 1, dtype=torch.float64)
    c = 0.7 * 0.3
    out = R.gat_edge_layer(x, ei, w, one, 0.4 * one, -0.2 * one, torch.zeros(1, dtype=torch.float64), 0.7 * one, 0.3 * one, 1, 1, True)
    lr = lambda v: v if v > 0 else 0.2 * v
    a_s, a_d = [0.4 * v for v in (1.0, 2.0, -1.0)], [-0.2 * v for v in (1.0, 2.0, -1.0)]
    lg = [lr(a_s[0] + a_d[2] + 0.5 * c), lr(a_s[1] + a_d[2] + 0.0), lr(a_s[1] + a_d[2] + 1.0 * c), lr(a_s[2] + a_d[2] + 0.5 * c)]
    e = torch.tensor(lg, dtype=torch.float64).exp()
    al = e / e.sum()
    want2 = float(al[0] * 1.0 + al[1] * 2.0 + al[2] * 2.0 + al[3] * -1.0)
    assert abs(float(out[2, 0]) - want2) < 1e-12
    assert abs(float(out[0, 0]) - 1.0) < 1e-12 and abs(float(out[1, 0]) - 2.0) < 1e-12       # only their loops
    # w = None: the edge term is absent
    o2 = R.gat_edge_layer(x, ei, None, one, 0.4 * one, -0.2 * one, torch.zeros(1, dtype=torch.float64), None, None, 1, 1, True)
    e2 = torch.tensor([lr(a_s[0] + a_d[2]), lr(a_s[1] + a_d[2]), lr(a_s[1] + a_d[2]), lr(a_s[2] + a_d[2])], dtype=torch.float64).exp()
    al2 = e2 / e2.sum()
    assert abs(float(o2[2, 0]) - float(al2[0] * 1.0 + al2[1] * 2.0 + al2[2] * 2.0 - al2[3])) < 1e-12
