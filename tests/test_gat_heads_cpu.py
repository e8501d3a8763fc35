"""CPU: the multi-head GAT head's construction (GATConv / GAT / GATModel shapes and state_dict keys, PyG 2.3.1's layout), the new C-ABI
declarations with the host-only predicate sgs_gat_heads_supported, and the evaluation routing (the batched ensemble engine is one-head:
a gat_heads > 1 model takes the serial loop)."""
import argparse
import sys

import pytest


def test_gatconv_heads_parameter_shapes_and_keys():
    from sgs_gnn_amd.model import GATConv
    for concat in (True, False):
        c = GATConv(7, 4, heads=3, concat=concat)
        sd = c.state_dict()
        assert set(sd) == {"lin_src.weight", "lin_dst.weight", "att_src", "att_dst", "bias"}
        assert c.lin_dst is c.lin_src
        assert tuple(sd["lin_src.weight"].shape) == (12, 7)
        assert tuple(sd["att_src"].shape) == (1, 3, 4) and tuple(sd["att_dst"].shape) == (1, 3, 4)
        assert tuple(sd["bias"].shape) == ((12,) if concat else (4,))
        assert c.heads == 3 and c.concat is concat and c.out_channels == 4
        # glorot bounds on the parameters' own shapes
        assert float(sd["lin_src.weight"].abs().max()) <= (6.0 / (7 + 12)) ** 0.5
        assert float(sd["att_src"].abs().max()) <= (6.0 / (3 + 4)) ** 0.5


def test_gatconv_rejects_unsupported_head_counts():
    from sgs_gnn_amd.model import GATConv
    for heads in (0, 17):
        with pytest.raises(ValueError):
            GATConv(7, 4, heads=heads)


def test_gat_layers_follow_init_conv():
    from sgs_gnn_amd.model import GAT
    g = GAT(12, 64, 2, 5, heads=8)
    c0, c1 = g.convs
    assert c0.out_channels == 8 and c0.heads == 8 and c0.concat
    assert c1.out_channels == 5 and c1.heads == 8 and not c1.concat
    assert tuple(c0.lin_src.weight.shape) == (64, 12) and tuple(c0.bias.shape) == (64,)
    assert tuple(c1.lin_src.weight.shape) == (40, 64) and tuple(c1.bias.shape) == (5,)
    with pytest.raises(ValueError):
        GAT(12, 60, 2, 5, heads=8)


def test_gatmodel_heads_argument_stays_unused_and_gat_heads_reaches_gat():
    import sgs_gnn_amd as S
    m = S.GATModel(12, 16, 5, heads=8)
    assert tuple(m.state_dict()["GAT.convs.0.att_src"].shape) == (1, 1, 16)
    assert m.gat_heads == 1
    m4 = S.GATModel(12, 16, 5, gat_heads=4)
    assert tuple(m4.state_dict()["GAT.convs.0.att_src"].shape) == (1, 4, 4)
    assert tuple(m4.state_dict()["GAT.convs.1.att_src"].shape) == (1, 4, 5)
    assert set(m4.state_dict()) == set(m.state_dict())
    with pytest.raises(TypeError):
        S.GATModel(12, 16, 5, 0.3, 8, "MLP", 4)          # gat_heads is keyword-only


HEAD_EXPORTS = ("sgs_gat_heads_supported", "sgs_gat_scores_heads_fwd", "sgs_gat_scores_heads_bwd_workspace_bytes", "sgs_gat_scores_heads_bwd",
                "sgs_gat_alpha_heads_fwd", "sgs_gat_alpha_heads_bwd", "sgs_edge_sum_by_row_heads", "sgs_spmm_csr_heads", "sgs_sddmm_csr_heads")


def test_header_declares_the_multi_head_entry_points():
    import sgs_gnn_amd
    protos = sgs_gnn_amd._lib.parse_header()
    for name in HEAD_EXPORTS:
        assert name in protos, name
    _, argtypes, argnames = protos["sgs_gat_heads_supported"]
    assert len(argtypes) == 2 and argnames == ["K", "C"]


@pytest.mark.parametrize("K,C,ok", [(1, 1, 1), (8, 32, 1), (8, 5, 1), (16, 64, 1), (0, 8, 0), (17, 4, 0), (4, 0, 0)])
def test_heads_supported_table(K, C, ok):
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()
    assert L.sgs_gat_heads_supported(K, C) == ok
    assert sgs_gnn_amd.ops.gat_heads_supported(K, C) is bool(ok)


def test_unsupported_heads_report_through_the_error_channel():
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()
    rc = L.sgs_spmm_csr_heads(None, 10, 17, 4, 0, None, None, None, None, None, 0, None, 0, 0.0, 0, 0, None, None)
    assert rc == -1 and b"unsupported heads" in L.sgs_last_error()
    rc = L.sgs_gat_alpha_heads_fwd(None, None, 10, 0, 0, None, None, None, 0.2, 0.0, 0, 0, None, None, None, None, None)
    assert rc == -1 and b"unsupported heads" in L.sgs_last_error()
    assert L.sgs_gat_scores_heads_fwd(None, 0, 8, 32, None, None, None, None, None) == 0          # N = 0: validates and returns


def test_multi_head_model_takes_the_serial_evaluation_loop():
    import sgs_gnn_amd as S
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    args = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all")
    assert ev._batched_ok(args, S.GATModel(12, 16, 5, gat_heads=4), 11) is False
    assert ev._batched_ok(args, S.GATModel(12, 16, 5, gat_heads=1), 11) is True
    assert ev._batched_ok(args, S.GATModel(12, 16, 5), 11) is True
