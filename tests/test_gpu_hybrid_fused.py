"""The hybrid loss in three launches (sgs_hybrid_loss_fused_fwd / sgs_hybrid_loss_fused_bwd) against the chain it replaces, through the C
ABI, bit for bit (`view(int32)`), every output pre-filled with nan so that an entry nobody wrote shows:

    forward    sgs_hybrid_loss_fwd (_w_fwd)                                       out[7], row_lse, rowloss, n_rows / den
    backward   sgs_edge_reg_bwd -> sgs_endpoint_reduce -> sgs_masked_ce_bwd_acc (_w_bwd_acc)      dlogits, dw

Shapes: N = 37 with q = 150 (nnz < 8 N: a wave per node), 600 (8 N <= nnz < 64 N: four waves per node) and 2 400 (>= 64 N: sixteen),
each with C = 5 (fewer columns than a 16-lane group), 41 (three ragged segments) and 64 (a multiple of 4: the reference reduction
takes its float4 form).  Every case has a hub node on ~40 % of the edges, a node with no incident edge, ~5 % self-loops and repeated
columns (loss_ref._edges), a zero logits row and a 1e-10 row (the cosine's clamp is active on their edges).  Variants at q = 600, C = 41
and at the sixteen-wave size: masks all / none, coef1 = 0, a label sum <= 1 (reg1 off), the weighted / smoothed criterion."""
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 37
QS = (150, 600, 2400)
CS = (5, 41, 64)


def _case(q, C, variant="base"):
    g = torch.Generator().manual_seed(7000 + 10 * q + C)
    L = torch.randn(N, C, generator=g)
    L[1] = 0.0
    L[2] = 0.0
    L[2, 0] = 1e-10
    y = torch.randint(0, C, (N,), generator=g)
    m = torch.rand(N, generator=g) < 0.6
    m[0] = True
    sei = R._edges(N - 1, q, g)                                    # node N - 1 has no incident edge
    hub = torch.rand(q, generator=g) < 0.4                         # node 0 on ~40 % of the edges, either end
    side = (torch.rand(q, generator=g) < 0.5).long()
    sei[side[hub], hub.nonzero().flatten()] = 0
    w = torch.rand(q, generator=g) * 0.98 + 0.01
    c1, c2, weight, eps = 1.0, 0.5, None, 0.0
    if variant == "mask_all":
        m[:] = True
    elif variant == "mask_none":
        m[:] = False
    elif variant == "coef1_0":
        c1 = 0.0
    elif variant == "labelsum_le1":                                # distinct labels, no self-loop: at most one same-label valid edge
        assert C >= N
        y = torch.arange(N)
        loop = sei[0] == sei[1]
        sei[1, loop] = (sei[0, loop] + 1) % (N - 1)
        m[:] = True
    elif variant == "weighted":
        weight, eps = torch.rand(C, generator=g) + 0.5, 0.1
    elif variant == "smoothed":
        eps = 0.2
    else:
        assert variant == "base"
    return dict(q=q, C=C, logits=L.contiguous(), y=y, mask=m, sei=sei.contiguous(), w=w, c1=c1, c2=c2, weight=weight, eps=eps,
                weighted=variant in ("weighted", "smoothed"))


def _nan(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -(2 ** 31), dtype=dtype, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _run(c):
    """-> (reference outputs, fused outputs), each a dict of device tensors."""
    import sgs_gnn_amd as S
    ops, lib = S.ops, S._lib
    Lh = lib.lib()
    p, st = ops._ptr, ops._stream
    q, C = c["q"], c["C"]
    lg, y, mk = c["logits"].to(DEV), c["y"].to(DEV), ops._u8(c["mask"].to(DEV))
    w, sei = c["w"].to(DEV), c["sei"].to(DEV)
    wt = None if c["weight"] is None else c["weight"].to(DEV)
    eps, wd = c["eps"], c["weighted"]
    gl = torch.tensor([R.G], dtype=torch.float32, device=DEV)
    gr = ops.get_graph(sei, N)
    assert gr.n_edges == q and gr.N == N
    ws = ops.workspace(Lh.sgs_edge_reg_workspace_bytes(q), lg.device)
    ndt = torch.float32 if wd else torch.int32

    ref = dict(out=_nan(7), row_lse=_nan(N), rowloss=_nan(N), norm=_nan(1, dtype=ndt), dw=_nan(q), Gs=_nan(q, C), Gd=_nan(q, C), dlogits=_nan(N, C))
    if wd:
        lib.check(Lh.sgs_hybrid_loss_w_fwd(p(lg), N, C, p(y), p(mk), p(w), p(sei), q, c["c1"], c["c2"], p(wt), eps, p(ref["out"]), p(ref["row_lse"]),
                                           p(ref["rowloss"]), p(ref["norm"]), ws.data_ptr(), ws.numel(), st()), "sgs_hybrid_loss_w_fwd")
    else:
        lib.check(Lh.sgs_hybrid_loss_fwd(p(lg), N, C, p(y), p(mk), p(w), p(sei), q, c["c1"], c["c2"], p(ref["out"]), p(ref["row_lse"]),
                                         p(ref["rowloss"]), p(ref["norm"]), ws.data_ptr(), ws.numel(), st()), "sgs_hybrid_loss_fwd")
    lib.check(Lh.sgs_edge_reg_bwd(p(w), p(sei), q, q, p(lg), N, C, p(y), p(mk), p(ref["out"]), c["c1"], c["c2"], p(gl), p(ref["dw"]), p(ref["Gs"]),
                                  p(ref["Gd"]), st()), "sgs_edge_reg_bwd")
    lib.check(Lh.sgs_endpoint_reduce(p(ref["Gs"]), p(ref["Gd"]), None, N, C, q, p(gr.in_ptr), p(gr.in_src), p(gr.in_eid), p(gr.out_ptr),
                                     p(gr.out_dst), p(gr.out_eid), 1.0, 1.0, p(ref["dlogits"]), st()), "sgs_endpoint_reduce")
    if wd:
        lib.check(Lh.sgs_masked_ce_w_bwd_acc(p(lg), N, C, p(y), p(mk), p(wt), eps, p(ref["row_lse"]), p(ref["norm"]), p(gl), p(ref["dlogits"]),
                                             st()), "sgs_masked_ce_w_bwd_acc")
    else:
        lib.check(Lh.sgs_masked_ce_bwd_acc(p(lg), N, C, p(y), p(mk), p(ref["row_lse"]), p(ref["norm"]), p(gl), p(ref["dlogits"]), st()),
                  "sgs_masked_ce_bwd_acc")

    def fwd(stash):
        o = dict(out=_nan(7), row_lse=_nan(N), rowloss=_nan(N), norm=_nan(1, dtype=ndt))
        lib.check(Lh.sgs_hybrid_loss_fused_fwd(p(lg), N, C, p(y), p(mk), p(w), p(sei), q, c["c1"], c["c2"], int(wd), p(wt), eps, p(o["out"]),
                                               p(o["row_lse"]), p(o["rowloss"]), p(o["norm"]), p(stash), ws.data_ptr(), ws.numel(), st()),
                  "sgs_hybrid_loss_fused_fwd")
        return o

    stash = _nan(q, 4)
    new = fwd(stash)
    new.update(stash=stash, dw=_nan(q), dlogits=_nan(N, C), nostash=fwd(None))
    lib.check(Lh.sgs_hybrid_loss_fused_bwd(p(lg), N, C, p(y), p(mk), p(w), q, p(stash), p(new["out"]), c["c1"], int(wd), p(wt), eps, p(new["row_lse"]),
                                           p(new["norm"]), p(gl), p(gr.in_ptr), p(gr.in_src), p(gr.in_eid), p(gr.out_ptr), p(gr.out_dst),
                                           p(gr.out_eid), p(new["dw"]), p(new["dlogits"]), st()), "sgs_hybrid_loss_fused_bwd")
    torch.cuda.synchronize()
    return ref, new


def _compare(c):
    ref, new = _run(c)
    for k in ("out", "row_lse", "rowloss", "norm"):
        assert torch.equal(_bits(new[k]), _bits(ref[k])), k
        assert torch.equal(_bits(new["nostash"][k]), _bits(ref[k])), ("no stash", k)
    assert not bool(torch.isnan(new["stash"]).any())                       # every sampled edge's four words were written
    for k in ("dw", "dlogits"):
        assert not bool(torch.isnan(ref[k]).any()), k                      # (the inputs keep every value finite)
        bad = (_bits(new[k]) != _bits(ref[k])).nonzero()
        assert bad.numel() == 0, (k, bad[:8].tolist(), new[k].cpu()[tuple(bad[0])], ref[k].cpu()[tuple(bad[0])])
    return ref, new


def _preconditions(c):
    s, d = c["sei"]
    deg = torch.bincount(torch.cat([s, d]), minlength=N)
    assert int(deg[N - 1]) == 0 and int(deg[0]) >= 0.35 * c["q"]
    L = c["logits"].double()
    nx, ny = (L[s] ** 2).sum(1), (L[d] ** 2).sum(1)
    assert int((nx * ny < 1e-16).sum()) >= 2                                # the cosine's clamp is active
    assert bool((s == d).any()) or c["y"].unique().numel() == N


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("q", QS)
def test_fused_chain_bitwise(q, C):
    c = _case(q, C)
    _preconditions(c)
    assert (q < 8 * N, q >= 64 * N) == {150: (True, False), 600: (False, False), 2400: (False, True)}[q]
    ref, new = _compare(c)
    lone = new["dlogits"][N - 1].cpu()                                       # the node without an edge: the cross entropy's term alone
    if not bool(c["mask"][N - 1]):
        assert bool((lone == 0).all())
    else:
        assert bool((lone != 0).any())


@pytest.mark.parametrize("variant", ["mask_all", "mask_none", "coef1_0", "labelsum_le1", "weighted", "smoothed"])
@pytest.mark.parametrize("q", (600, 2400))
def test_fused_chain_variants_bitwise(q, variant):
    c = _case(q, 41, variant)
    _preconditions(c)
    ref, new = _compare(c)
    o = new["out"].cpu()
    if variant == "mask_none":
        assert float(o[2]) == 0.0 and bool(torch.isnan(o[5]))
        assert bool((new["dlogits"][N - 1].cpu() == 0).all())
    if variant == "labelsum_le1":
        assert float(o[3]) <= 1.0 and float(o[0]) == 0.0 and float(o[2]) > 0.0


def test_lone_train_node_gets_the_cross_entropy_alone():
    """The node without an edge, on the mask: its row is exactly what sgs_masked_ce_bwd writes."""
    import sgs_gnn_amd as S
    ops, lib = S.ops, S._lib
    c = _case(600, 41)
    c["mask"] = c["mask"].clone()
    c["mask"][N - 1] = True
    ref, new = _compare(c)
    lg, y, mk = c["logits"].to(DEV), c["y"].to(DEV), ops._u8(c["mask"].to(DEV))
    gl = torch.tensor([R.G], dtype=torch.float32, device=DEV)
    ce = _nan(N, 41)
    lib.check(lib.lib().sgs_masked_ce_bwd(ops._ptr(lg), N, 41, ops._ptr(y), ops._ptr(mk), ops._ptr(new["row_lse"]), ops._ptr(new["norm"]),
                                          ops._ptr(gl), ops._ptr(ce), ops._stream()), "sgs_masked_ce_bwd")
    assert torch.equal(_bits(new["dlogits"][N - 1]), _bits(ce[N - 1]))


def test_ops_hybrid_loss_takes_the_fused_chain_and_keeps_no_stash_without_grad():
    """ops.hybrid_loss: the same seven outputs with and without a gradient wanted; its gradients are the C-ABI chain's."""
    import sgs_gnn_amd as S
    ops = S.ops
    c = _case(2400, 41)
    ref, new = _compare(c)
    d = dict(y=c["y"].to(DEV), mask=c["mask"].to(DEV), sei=c["sei"].to(DEV))
    ld, wd = c["logits"].to(DEV).requires_grad_(True), c["w"].to(DEV).requires_grad_(True)
    loss, out = ops.hybrid_loss(ld, d["y"], d["mask"], wd, d["sei"], c["c1"], c["c2"])
    gl, gw = torch.autograd.grad(loss * R.G, (ld, wd))
    assert torch.equal(_bits(out), _bits(ref["out"]))
    assert torch.equal(_bits(gl), _bits(ref["dlogits"])) and torch.equal(_bits(gw), _bits(ref["dw"]))
    with torch.no_grad():
        _, out2 = ops.hybrid_loss(ld, d["y"], d["mask"], wd, d["sei"], c["c1"], c["c2"])
    assert torch.equal(_bits(out2), _bits(ref["out"]))
