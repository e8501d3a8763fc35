"""CPU: the Chebyshev head of order K > 1 -- construction (ChebConv / ChebModel shapes and state_dict keys, PyG 2.3.1's layout), the new
C-ABI declarations with the host-only predicate sgs_cheb_supported, the error channel, and the evaluation routing (the batched ensemble
engine's Chebyshev branch is K = 1 only: a cheb_k > 1 model takes the serial loop)."""
import argparse
import sys

import pytest
import torch

TODAY_KEYS = {"gcn1.lins.0.weight", "gcn1.bias", "gcn2.lins.0.weight", "gcn2.bias"}


def _head_keys(m):
    return {k for k in m.state_dict() if not k.startswith("edge_prob_mlp.")}


def test_chebconv_parameter_shapes_keys_and_init():
    from sgs_gnn_amd.model import ChebConv
    torch.manual_seed(0)
    c = ChebConv(7, 4, K=3)
    sd = c.state_dict()
    assert set(sd) == {"lins.0.weight", "lins.1.weight", "lins.2.weight", "bias"}
    for k in range(3):
        assert tuple(sd[f"lins.{k}.weight"].shape) == (4, 7)
        assert float(sd[f"lins.{k}.weight"].abs().max()) <= (6.0 / (7 + 4)) ** 0.5        # glorot bound
        assert float(sd[f"lins.{k}.weight"].abs().max()) > 0
    assert not torch.equal(sd["lins.0.weight"], sd["lins.1.weight"])
    assert tuple(sd["bias"].shape) == (4,) and float(sd["bias"].abs().max()) == 0.0
    assert c.K == 3


def test_chebconv_rejects_unsupported_orders_and_normalisations():
    from sgs_gnn_amd.model import ChebConv
    for K in (0, 9):
        with pytest.raises(ValueError):
            ChebConv(7, 4, K=K)
    with pytest.raises(NotImplementedError):
        ChebConv(7, 4, K=2, normalization='rw')
    with pytest.raises(NotImplementedError):
        ChebConv(7, 4, K=1, normalization=None)


def test_chebmodel_keys_with_and_without_the_keyword():
    import sgs_gnn_amd as S
    m3 = S.ChebModel(12, 16, 5, cheb_k=3)
    assert _head_keys(m3) == {f"gcn{l}.lins.{k}.weight" for l in (1, 2) for k in range(3)} | {"gcn1.bias", "gcn2.bias"}
    assert tuple(m3.state_dict()["gcn1.lins.2.weight"].shape) == (16, 12) and tuple(m3.state_dict()["gcn2.lins.2.weight"].shape) == (5, 16)
    assert m3.cheb_k == 3
    m1 = S.ChebModel(12, 16, 5)
    assert _head_keys(m1) == TODAY_KEYS and m1.cheb_k == 1
    assert _head_keys(S.ChebModel(12, 16, 5, 0.3, "GCN")) == TODAY_KEYS
    with pytest.raises(TypeError):
        S.ChebModel(12, 16, 5, 0.3, "MLP", 3)                       # cheb_k is keyword-only
    with pytest.raises(ValueError):
        S.ChebModel(12, 16, 5, cheb_k=9)


def test_default_model_draws_the_same_initial_weights_as_before_the_keyword():
    """K = 1 constructs one Linear per layer and initialises it exactly as before: same generator consumption, same weights."""
    import sgs_gnn_amd as S
    torch.manual_seed(11)
    a = S.ChebModel(12, 16, 5).state_dict()
    torch.manual_seed(11)
    b = S.ChebModel(12, 16, 5, cheb_k=1).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_state_dict_round_trip_and_strict_mismatch():
    import sgs_gnn_amd as S
    m3 = S.ChebModel(12, 16, 5, cheb_k=3)
    sd = {k: v.clone() for k, v in m3.state_dict().items()}
    fresh = S.ChebModel(12, 16, 5, cheb_k=3)
    fresh.load_state_dict(sd)
    assert all(torch.equal(fresh.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        S.ChebModel(12, 16, 5, cheb_k=1).load_state_dict(sd)       # strict: unexpected lins.1 / lins.2


CHEB_EXPORTS = ("sgs_cheb_supported", "sgs_cheb_norm_fwd", "sgs_cheb_norm_bwd_workspace_bytes", "sgs_cheb_norm_bwd", "sgs_cheb_spmm")


def test_header_declares_the_chebyshev_entry_points():
    import sgs_gnn_amd
    protos = sgs_gnn_amd._lib.parse_header()
    for name in CHEB_EXPORTS:
        assert name in protos, name
    _, argtypes, argnames = protos["sgs_cheb_supported"]
    assert len(argtypes) == 1 and argnames == ["K"]
    names = protos["sgs_cheb_spmm"][2]
    assert {"ldx", "ldadd", "ldsub", "ldy"} <= set(names)            # a leading dimension per dense operand


@pytest.mark.parametrize("K,ok", [(1, 1), (8, 1), (2, 1), (0, 0), (9, 0), (-1, 0)])
def test_cheb_supported_table(K, ok):
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()
    assert L.sgs_cheb_supported(K) == ok
    assert sgs_gnn_amd.ops.cheb_supported(K) is bool(ok)


def test_unsupported_order_reports_through_the_error_channel():
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()

    def spmm(K, N):
        return L.sgs_cheb_spmm(K, None, 4, N, 4, 0, None, None, None, 1.0, None, 0, None, 0, None, 0, 0.0, 0, 0, None, 4, None, 0, 1.0, None)

    for K in (0, 9):
        assert spmm(K, 10) == -1 and b"unsupported" in L.sgs_last_error()
    assert spmm(3, 0) == 0                                            # N = 0: validates and returns
    assert L.sgs_cheb_norm_fwd(None, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0
    assert L.sgs_cheb_norm_bwd(None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None, 0, None) == 0
    assert L.sgs_cheb_norm_bwd_workspace_bytes(1013) >= 4 * 1013


def test_higher_order_model_takes_the_serial_evaluation_loop():
    import sgs_gnn_amd as S
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    args = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all")
    assert ev._batched_ok(args, S.ChebModel(12, 16, 5, cheb_k=3), 11) is False
    assert ev._batched_ok(args, S.ChebModel(12, 16, 5, cheb_k=1), 11) is True
    assert ev._batched_ok(args, S.ChebModel(12, 16, 5), 11) is True


def test_no_cpu_fallback_for_the_chebyshev_ops():
    import sgs_gnn_amd as S
    ei = torch.randint(0, 10, (2, 40))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.cheb_norm(S.ops.get_graph(ei, 10))
    g = S.ops.Graph.__new__(S.ops.Graph)                             # a graph object that exists: the weights are refused on their own
    g.edge_index, g.n_edges, g.N = ei, 40, 10
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.cheb_norm(g, torch.rand(40))
    nm = S.ops.Norm()                                               # (never reached: the tensors are checked first)
    nm.graph, nm.what_loop, nm.dis = None, None, torch.ones(10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.cheb_conv(torch.randn(10, 6), torch.randn(8, 6), torch.zeros(4), nm, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ChebModel(6, 8, 3, cheb_k=2)(S.Batch(x=torch.randn(10, 6), edge_index=ei), ei, torch.rand(40))


def test_sharded_trainers_refuse_a_higher_order_head():
    from importlib import import_module
    import sgs_gnn_amd as S
    sh = import_module("sgs_gnn_amd.sharded")
    m = S.ChebModel(6, 8, 3, edge_mlp_type="GCN", cheb_k=2)
    for fn in (sh.train_step_sharded, sh.train_step_blocksharded):
        with pytest.raises(NotImplementedError, match="cheb_k"):
            fn(None, m, None, None, None, None, 5)
    with pytest.raises(NotImplementedError, match="cheb_k"):
        sh.sharded_evaluate_forward(None, m, None, 5)
