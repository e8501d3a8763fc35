"""GPU: the backward prologue of every layer op (ops._grad_through_act: dZ = dY * act'(Y) and the bias gradient) and the edge-weight
gradient hand-over of the two edge-term attention ops, on one tiny graph.

The expected dZ and dbias are built by hand through the C ABI with the three entry points the prologue chooses between
(sgs_act_bwd_colsum, sgs_act_bwd, sgs_colsum) from the op's own output and the upstream gradient, and compared bitwise.  What the op
itself formed is read off a recording wrapper around the prologue (dZ is internal to every backward) and off bias.grad.

The two families differ on purpose for a bias that exists but does not require a gradient: the GCN / Chebyshev layers then do no bias
work at all, the attention layers still compute the sum and autograd discards it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, E, FIN = 37, 150, 7
SEED, SITE = 5, 2


def _edges():
    """150 directed edges over 37 nodes: one self-loop (3, 3), one duplicated edge (1 -> 2 twice), node 36 without in-edges."""
    g = torch.Generator().manual_seed(1234)
    src = torch.randint(0, N, (E,), generator=g)
    dst = torch.randint(0, N - 1, (E,), generator=g)                # nothing points at node 36
    clash = src == dst
    src[clash] = (src[clash] + 1) % N                               # no accidental loops ...
    src[0], dst[0] = 3, 3                                           # ... one deliberate
    src[1], dst[1], src[2], dst[2] = 1, 2, 1, 2
    ei = torch.stack([src, dst])
    assert int((ei[0] == ei[1]).sum()) == 1 and not bool((ei[1] == N - 1).any())
    return ei


@pytest.fixture(scope="module")
def env():
    import sgs_gnn_amd as S
    ops = S.ops
    ei = _edges().to(DEV)
    return S, ops, ops.get_graph(ei, N)


ACTS = {"none": (0, 0.0), "relu": (1, 0.0), "relu_dropout": (2, 0.3)}
BIASES = ("absent", "trainable", "frozen")
GCN_FAMILY = ("gcn_propagate", "gcn_layer", "cheb_conv")
OPS = GCN_FAMILY + ("gat_h1", "gat_h3", "gat_h3_edge", "gatv2_h3", "gatv2_h3_edge")


def _leaf(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV).requires_grad_(True)


def _run(ops, gr, op, C, act, p, bias_mode, spy):
    """Forward + backward of `op` at `C` output channels (per head); returns (Y, gy, bias, the other leaves by name)."""
    g = torch.Generator().manual_seed(77)
    K = 3 if "_h3" in op else 1
    width = K * C
    w = (torch.rand(E, generator=g) + 0.1).to(DEV).requires_grad_(True)
    bias = None
    if bias_mode != "absent":
        bias = (torch.randn(width, generator=g) * 0.3).to(DEV).requires_grad_(bias_mode == "trainable")
    leaves = {"w": w} if (op in GCN_FAMILY or op.endswith("_edge")) else {}      # (the plain attention ops take no edge weights)
    kw = dict(act=act, p=p, seed=SEED, site=SITE)
    if op == "gcn_propagate":
        leaves["X"] = _leaf(g, N, C)
        Y = ops.gcn_propagate(leaves["X"], ops.gcn_norm(gr, w), bias, **kw)
    elif op == "gcn_layer":
        leaves["x"], leaves["W"] = _leaf(g, N, FIN), _leaf(g, C, FIN, scale=0.4)
        Y, _ = ops.gcn_layer(leaves["x"], leaves["W"], bias, ops.gcn_norm(gr, w), **kw)
    elif op == "cheb_conv":
        leaves["x"], leaves["W"] = _leaf(g, N, FIN), _leaf(g, 3 * C, FIN, scale=0.4)
        Y = ops.cheb_conv(leaves["x"], leaves["W"], bias, ops.cheb_norm(gr, w), 3, **kw)
    else:
        akw = dict(act=act, p_act=p, seed_act=SEED, site_act=SITE, heads=K, concat=True)
        leaves["xl"] = _leaf(g, N, width)
        if op.startswith("gatv2"):
            leaves["xr"], leaves["att"] = _leaf(g, N, width), _leaf(g, width, scale=0.5)
            if op.endswith("_edge"):
                leaves["lin_edge"] = _leaf(g, width, scale=0.5)
                akw.update(edge_weight=w, lin_edge=leaves["lin_edge"])
            Y = ops.gatv2_aggregate(leaves["xl"], leaves["xr"], leaves["att"], bias, gr, **akw)
        else:
            shape = (N,) if K == 1 else (N, K)
            leaves["a_s"], leaves["a_d"] = _leaf(g, *shape), _leaf(g, *shape)
            if op.endswith("_edge"):
                leaves["coef"] = _leaf(g, K, scale=0.5)
                akw.update(edge_weight=w, edge_coef=leaves["coef"])
            Y = ops.gat_aggregate(leaves["xl"], leaves["a_s"], leaves["a_d"], bias, gr, **akw)
    gy = torch.randn(N, Y.shape[1], generator=g).to(DEV)
    spy.clear()
    Y.backward(gy)
    return Y.detach(), gy, bias, leaves


def _expected(ops, gy, Y, act, p, want_db):
    """(dZ, dbias) by hand through the C ABI, with the entry point the prologue is to choose."""
    L = ops._lib.lib()
    n, D = gy.shape
    ws = ops.workspace(L.sgs_colsum_workspace_bytes(n, D), gy.device)
    db = torch.empty(D, dtype=torch.float32, device=gy.device) if want_db else None
    if act == 0:
        if want_db:
            ops._lib.check(L.sgs_colsum(gy.data_ptr(), n, D, db.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "sgs_colsum")
        return gy, db
    dZ = torch.empty_like(gy)
    if want_db:
        ops._lib.check(L.sgs_act_bwd_colsum(gy.data_ptr(), Y.data_ptr(), n, D, act, p, dZ.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                            ops._stream()), "sgs_act_bwd_colsum")
    else:
        ops._lib.check(L.sgs_act_bwd(gy.data_ptr(), Y.data_ptr(), gy.numel(), act, p, dZ.data_ptr(), ops._stream()), "sgs_act_bwd")
    return dZ, db


@pytest.fixture()
def spy(env, monkeypatch):
    """Records every prologue call of a backward: (want_db, dZ, dbias as returned); counts the bias-sum launches beside it."""
    _, ops, _ = env
    calls = []
    real, real_colsum = ops._grad_through_act, ops._colsum

    def prologue(dY, Y, act, p, want_db, colsum_now=True):
        out = real(dY, Y, act, p, want_db, colsum_now)
        calls.append(("prologue", bool(want_db), out[0], out[1]))
        return out

    def colsum(A):
        calls.append(("colsum", A))
        return real_colsum(A)

    monkeypatch.setattr(ops, "_grad_through_act", prologue)
    monkeypatch.setattr(ops, "_colsum", colsum)
    return calls


@pytest.mark.parametrize("act_name", list(ACTS))
@pytest.mark.parametrize("op", OPS)
def test_prologue_dz_and_dbias_bitwise(env, spy, op, act_name):
    _, ops, gr = env
    act, p = ACTS[act_name]
    gcn_family = op in GCN_FAMILY
    for C in (5, 8):                                                # odd rows (the scalar kernels) and 16-byte aligned rows
        grads = {}
        for bias_mode in BIASES:
            Y, gy, bias, leaves = _run(ops, gr, op, C, act, p, bias_mode, spy)
            pro = [c for c in spy if c[0] == "prologue"]
            late = [c for c in spy if c[0] == "colsum"]
            assert len(pro) == 1, (op, C, bias_mode, len(pro))
            _, want_db, dZ, _ = pro[0]
            # what each family asks for: the GCN / Chebyshev layers has_bias AND needs_input_grad, the attention layers has_bias alone
            assert want_db == ((bias_mode == "trainable") if gcn_family else (bias_mode != "absent")), (op, C, bias_mode)
            exp_dZ, exp_db = _expected(ops, gy, Y, act, p, want_db)
            assert torch.equal(dZ, exp_dZ), (op, C, bias_mode)
            if bias_mode == "trainable":
                assert bias.grad is not None and torch.equal(bias.grad, exp_db), (op, C, bias_mode)
            elif bias_mode == "frozen":
                assert bias.grad is None
                if gcn_family:                                      # no bias work at all: neither the fused pass nor a column sum
                    assert pro[0][3] is None and not late, (op, C)
                else:                                               # computed (bitwise the trainable run's) and discarded by autograd
                    assert pro[0][3] is not None and torch.equal(pro[0][3], exp_db), (op, C)
            else:
                assert pro[0][3] is None and not late, (op, C)
            grads[bias_mode] = {k: v.grad.clone() for k, v in leaves.items() if v.grad is not None}
            assert set(grads[bias_mode]) == set(leaves), (op, C, bias_mode, sorted(grads[bias_mode]))
        # a bias that is frozen changes nothing else: every other gradient is bitwise the trainable run's
        for k, v in grads["trainable"].items():
            assert torch.equal(grads["frozen"][k], v), (op, C, k)


def _edge_layer(ops, gr, op, xl, P, ea_or_w):
    akw = dict(act=1, p_act=0.0, heads=3, concat=True)
    if op == "gatv2_h3_edge":
        return ops.gatv2_aggregate(xl, P["xr"], P["att"], P["bias"], gr, edge_weight=ea_or_w, lin_edge=P["le"], **akw)
    return ops.gat_aggregate(xl, P["a_s"], P["a_d"], P["bias"], gr, edge_weight=ea_or_w, edge_coef=P["coef"], **akw)


@pytest.mark.parametrize("op", ["gat_h3_edge", "gatv2_h3_edge"])
def test_two_layers_sharing_one_edge_attr_hand_their_dw_over(env, op):
    """Two layers over ONE EdgeAttr: the edge weights' gradient is the sum of the two layers' d w taken one layer at a time (the second
    layer to finish adds the first one's inside its kernel: one fp32 add per edge either way), and the side band is neutral afterwards."""
    _, ops, gr = env
    C, K = 5, 3
    width = K * C
    g = torch.Generator().manual_seed(99)
    w0 = torch.rand(E, generator=g) + 0.1
    x0 = torch.randn(N, width, generator=g)
    gy = torch.randn(N, width, generator=g).to(DEV)

    def params():
        gp = torch.Generator().manual_seed(7)
        mk = lambda *s: (torch.randn(*s, generator=gp) * 0.5).to(DEV)
        return [dict(xr=mk(N, width), att=mk(width), le=mk(width), a_s=mk(N, K), a_d=mk(N, K), coef=mk(K), bias=mk(width)) for _ in range(2)]

    # both layers in one backward, sharing the wrapper
    P1, P2 = params()
    w = w0.to(DEV).requires_grad_(True)
    ea = ops.gat_edge_attr(gr, w)
    Y1 = _edge_layer(ops, gr, op, x0.to(DEV), P1, ea)
    Y2 = _edge_layer(ops, gr, op, Y1, P2, ea)
    Y2.backward(gy)
    assert ea._g_first is None and ea._g_extra is None and ea._dw_first is None and ea._extra_total is False
    # one layer at a time: layer 2 over layer 1's output, then layer 1 under layer 2's input gradient, each with a wrapper of its own
    wa = w0.to(DEV).requires_grad_(True)
    h = Y1.detach().clone().requires_grad_(True)
    _edge_layer(ops, gr, op, h, P2, ops.gat_edge_attr(gr, wa)).backward(gy)
    wb = w0.to(DEV).requires_grad_(True)
    _edge_layer(ops, gr, op, x0.to(DEV), P1, ops.gat_edge_attr(gr, wb)).backward(h.grad)
    assert float(wa.grad.abs().max()) > 0 and float(wb.grad.abs().max()) > 0
    assert torch.equal(w.grad, wa.grad + wb.grad)
