"""GPU: the batched ensemble-evaluation engine of the GATv2 head (GATModel(gat_v2=True), args.sgs_eval_batch_gatv2).

Kernel level: block d of ops.gatv2_alpha_heads_multi (sgs_gatv2_alpha_heads_fwd_multi) is BITWISE what sgs_gatv2_alpha_heads_fwd (C ABI,
p_drop = 0) writes to alpha / alpha_loop on draw d's Graph, in all four (VEC, ONE) instantiations, for a shared x_l / x_r pair and for
dense per-draw blocks, with and without the edge term; one case is held element by element to gatv2_kernels_ref.alpha_fwd in fp64 under
that module's own a-priori bound.

Engine level: against the serial loop from the same clocks -- drawn edge sets torch.equal, F1 equal, both clocks equal, PATH_COUNTS on
the right path, per-draw logits and mean within 1e-5 x max|logits| (tests/test_gpu_ensemble_batched_heads.py's own tolerance, for its
reason: layer 2's product runs as one library GEMM over D N rows, which need not be bitwise the per-draw GEMM; the softmax and the
aggregation are pinned bitwise at kernel level.  The logits are NOT asserted bitwise here) -- against the fp64 model under
test_gpu_gatv2.py's forward bound, under node-covering draws, determinism, and the dropout seed training sees afterwards."""
import argparse
import sys

import pytest
import torch

import gatv2_kernels_ref as KR
import gatv2_ref
from conftest import load_golden
from test_gpu_ensemble_batched_variants import _draws

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOPE = 0.2
FWD_BOUND = 1e-5          # max-abs error over max-abs reference: test_gpu_gatv2.py::test_two_layer_head_logits_and_gradients' logits bound
SERIAL_TOL = 1e-5         # x max|logits|: test_gpu_ensemble_batched_heads.py's serial-vs-batched tolerance
KC = [(1, 16), (2, 5), (16, 20), (3, 41), (8, 8)]


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


# ------------------------------------------------------------------ kernel level
def _single(S, xl, xr, att, gd, K, C, w=None, le=None):
    """sgs_gatv2_alpha_heads_fwd through the C ABI on one draw's Graph, p_drop = 0 -> (alpha [n, K], alpha_loop [N, K], loop_w [N] or None)."""
    L, ops = S._lib.lib(), S.ops
    N, n = gd.N, gd.n_edges
    f32 = dict(dtype=torch.float32, device=DEV)
    soft, alpha = torch.empty(max(n, 1), K, **f32), torch.empty(max(n, 1), K, **f32)
    soft_loop, alpha_loop = torch.empty(N, K, **f32), torch.empty(N, K, **f32)
    edge = w is not None and n > 0
    loop = torch.empty(2, N, **f32) if edge else None
    S._lib.check(L.sgs_gatv2_alpha_heads_fwd(xl.data_ptr(), xr.data_ptr(), att.data_ptr(), w.data_ptr() if edge else None,
                                             le.data_ptr() if edge else None, N, K, C, n, ops._ptr(gd.in_ptr), ops._ptr(gd.in_src),
                                             ops._ptr(gd.in_eid), SLOPE, 0.0, 0, 16, ops._ptr(soft), ops._ptr(soft_loop), ops._ptr(alpha),
                                             ops._ptr(alpha_loop), loop[0].data_ptr() if edge else None, loop[1].data_ptr() if edge else None,
                                             ops._stream()), "sgs_gatv2_alpha_heads_fwd")
    assert torch.equal(soft, alpha) or n == 0                 # p = 0: alpha is soft
    return alpha[:n], alpha_loop, (loop[0] if edge else None)


def _x_of(kind, D, N, W, g):
    """-> (xl, xr, x_stride, [draw d's (xl, xr) blocks, views into the buffers]) for a shared pair or dense per-draw blocks."""
    if kind == "shared":
        xl, xr = torch.randn(N, W, generator=g).to(DEV), torch.randn(N, W, generator=g).to(DEV)
        return xl, xr, 0, [(xl, xr)] * D
    xl, xr = torch.randn(D, N, W, generator=g).to(DEV), torch.randn(D, N, W, generator=g).to(DEV)
    return xl, xr, N * W, [(xl[d], xr[d]) for d in range(D)]


def _aligned16(*ts):
    return int(all(t.data_ptr() % 16 == 0 for t in ts))


def _check_blocks(S, graph, D, K, C, kind, edge):
    ops = S.ops
    L = S._lib.lib()
    N, q, smp, csr, gds, _, g = _draws(S, graph, D)
    W = K * C
    att = (torch.rand(W, generator=g) * 2 - 1).to(DEV)
    le = (torch.rand(W, generator=g) * 2 - 1).to(DEV)
    xl, xr, stride, blocks = _x_of(kind, D, N, W, g)
    w = None
    if edge:
        w = smp.w if smp is not None else torch.zeros(D, 0, device=DEV)
    alpha, alpha_loop = ops.gatv2_alpha_heads_multi(xl, xr, stride, att, csr, q, N, K, SLOPE, **(dict(edge_w=w, lin_edge=le) if edge else {}))
    assert alpha.shape == (D, max(q, 1), K) and alpha_loop.shape == (D, N, K)
    code = L.sgs_gatv2_variant(0, N, K, C, _aligned16(xl, xr, att, le))
    singles = []
    for d in range(D):
        bl, br = blocks[d]
        # every block takes the variant of the base pointers: the single-draw call on the block itself (a view, not a copy)
        assert L.sgs_gatv2_variant(0, N, K, C, _aligned16(bl, br, att, le)) == code, (graph, D, K, C, kind, d)
        wd = w[d].contiguous() if (edge and q > 0) else None
        one, one_loop, loop_w = _single(S, bl, br, att, gds[d], K, C, wd, le)
        assert torch.equal(alpha[d, :q], one), (graph, D, K, C, kind, edge, d)
        assert torch.equal(alpha_loop[d], one_loop), (graph, D, K, C, kind, edge, d)
        singles.append((one, one_loop, loop_w))
    return N, q, smp, csr, gds, dict(xl=xl, xr=xr, stride=stride, blocks=blocks, w=w, att=att, le=le, alpha=alpha, alpha_loop=alpha_loop,
                                     singles=singles, code=code)


def test_the_shapes_reach_all_four_instantiations():
    import sgs_gnn_amd as S
    L = S._lib.lib()
    seen = {}
    for K, C in KC:
        for N in (300, 24, 6, 25):
            code = L.sgs_gatv2_variant(0, N, K, C, 1)
            assert code // 1000000 == 1
            seen.setdefault((code // 100000 % 10, code // 100 % 10), []).append((K, C))
    assert set(seen) == {(4, 1), (1, 1), (4, 0), (1, 0)}, seen
    assert (1, 16) in seen[(4, 1)] and (2, 5) in seen[(1, 1)] and (16, 20) in seen[(4, 0)] and (3, 41) in seen[(1, 0)] and (8, 8) in seen[(4, 1)]


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("graph", ["hub", "dense", "very_dense", "empty"])
@pytest.mark.parametrize("K,C", KC)
def test_every_block_is_bitwise_the_single_draw_softmax(D, graph, K, C):
    import sgs_gnn_amd as S
    want_vec = 4 if C % 4 == 0 else 1
    for kind in ("shared", "blocks"):
        for edge in (False, True):
            N, q, smp, csr, gds, r = _check_blocks(S, graph, D, K, C, kind, edge)
            assert r["code"] // 100000 % 10 == want_vec                                   # float4 on every draw's block whenever C % 4 == 0
            if graph == "hub":
                deg = csr[0][0, 1:] - csr[0][0, :-1]
                assert int(deg[0]) > 64 and int((deg[250:] != 0).sum()) == 0              # a row of many gathers, and rows without in-edges
                for d in range(D):
                    ei = smp.edge_index[d]
                    diag = (ei[0] == ei[1]).nonzero().flatten()
                    assert diag.numel() > 0 and bool((r["alpha"][d, diag] == 0).all())    # drawn (i, i) entries: exactly 0
                    # a row without in-edges: the loop alone, exp(0) / (1 + 1e-16), which is the single-draw value
                    assert bool((r["alpha_loop"][d, 250:] == 1.0).all()) and torch.equal(r["alpha_loop"][d, 250:], r["singles"][d][1][250:])


def test_one_case_against_the_fp64_kernel_reference_element_by_element():
    """dense graph, K = 3, C = 41 (VEC 1, chunks walked in a loop) with the edge term, per-draw blocks.  The loop's pre-activation takes the
    kernel's own fp32 mean weight, as tests/test_gpu_gatv2_gine_kernels.py hands it to the reference: the single-draw call's loop_w, whose
    alpha the block equals bit for bit."""
    import sgs_gnn_amd as S
    D, K, C = 3, 3, 41
    N, q, smp, csr, gds, r = _check_blocks(S, "dense", D, K, C, "blocks", True)
    for d in range(D):
        bl, br = r["blocks"][d]
        ref = KR.alpha_fwd(bl.cpu(), br.cpu(), r["att"].cpu(), csr[0][d].cpu(), csr[1][d].cpu(), csr[2][d].cpu(), K, C, SLOPE,
                           edge_w=r["w"][d].cpu(), lin_edge=r["le"].cpu(), loop_w=r["singles"][d][2].cpu(), bounds=True)
        for name, got, want, bound in (("alpha", r["alpha"][d, :q], ref["soft"], ref["soft_bound"]),
                                       ("alpha_loop", r["alpha_loop"][d], ref["soft_loop"], ref["soft_loop_bound"])):
            err = (got.double().cpu() - want).abs()
            print(f"draw {d} {name}: max |err| = {float(err.max()):.3e}, max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert not bool(KR.outside(got.cpu(), want, bound).any()), (d, name)


def test_the_weights_count_and_launches_repeat():
    import sgs_gnn_amd as S
    ops = S.ops
    for graph, (K, C) in (("hub", (8, 8)), ("dense", (3, 41)), ("very_dense", (16, 20))):
        N, q, smp, csr, gds, _, g = _draws(S, graph, 3)
        W = K * C
        att, le = (torch.rand(W, generator=g) * 2 - 1).to(DEV), (torch.rand(W, generator=g) * 2 - 1).to(DEV)
        xl, xr = torch.randn(3, N, W, generator=g).to(DEV), torch.randn(3, N, W, generator=g).to(DEV)
        run = lambda **kw: ops.gatv2_alpha_heads_multi(xl, xr, N * W, att, csr, q, N, K, SLOPE, **kw)
        none = run()
        w1, w2 = run(edge_w=smp.w, lin_edge=le), run(edge_w=smp.w, lin_edge=le)
        assert torch.equal(w1[0], w2[0]) and torch.equal(w1[1], w2[1])                     # two identical launches: identical bits
        assert not torch.equal(w1[0], none[0]) and not torch.equal(w1[1], none[1])         # lin_edge != 0: the weights change alpha
        # zero weights: fmaf(0, le, xl + xr) is xl + xr, and the loop's mean weight is 0 -- here the reference's formula says "equal"
        z = run(edge_w=torch.zeros_like(smp.w), lin_edge=le)
        assert torch.equal(z[0], none[0]) and torch.equal(z[1], none[1])
        # and a zero lin_edge with real weights likewise
        z = run(edge_w=smp.w, lin_edge=torch.zeros_like(le))
        assert torch.equal(z[0], none[0]) and torch.equal(z[1], none[1])
        # out= reuses the pair
        again = run(edge_w=smp.w, lin_edge=le, out=none)
        assert again[0] is none[0] and again[1] is none[1] and torch.equal(again[0], w1[0]) and torch.equal(again[1], w1[1])


def test_wrapper_refuses_wrong_arguments():
    import sgs_gnn_amd as S
    ops = S.ops
    N, q, smp, csr, gds, _, g = _draws(S, "hub", 2)
    K, C = 2, 4
    att = torch.zeros(K * C, device=DEV)
    x = torch.zeros(N, K * C, device=DEV)
    xb = torch.zeros(2, N, K * C, device=DEV)
    with pytest.raises(RuntimeError, match="edge_w must be"):
        ops.gatv2_alpha_heads_multi(x, x, 0, att, csr, q, N, K, SLOPE, edge_w=torch.zeros(2, q + 1, device=DEV), lin_edge=att)
    with pytest.raises(RuntimeError, match="edge_w needs lin_edge"):
        ops.gatv2_alpha_heads_multi(x, x, 0, att, csr, q, N, K, SLOPE, edge_w=smp.w)
    with pytest.raises(RuntimeError, match="lin_edge must be"):
        ops.gatv2_alpha_heads_multi(x, x, 0, att, csr, q, N, K, SLOPE, edge_w=smp.w, lin_edge=att[:4])
    for stride in (1, N * K * C + 4, 2 * N * K * C, -N * K * C):
        with pytest.raises(RuntimeError, match="x_stride"):
            ops.gatv2_alpha_heads_multi(xb, xb, stride, att, csr, q, N, K, SLOPE)
    with pytest.raises(RuntimeError, match="xl must be"):
        ops.gatv2_alpha_heads_multi(x, x, N * K * C, att, csr, q, N, K, SLOPE)           # per-draw stride, one block of data
    with pytest.raises(RuntimeError, match="xr must be"):
        ops.gatv2_alpha_heads_multi(x, xb, 0, att, csr, q, N, K, SLOPE)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.gatv2_alpha_heads_multi(x, x, 0, att, csr, q, N, K, SLOPE, out=(torch.zeros(2, q, K + 1, device=DEV), torch.zeros(2, N, K, device=DEV)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gatv2_alpha_heads_multi(x.cpu(), x, 0, att, csr, q, N, K, SLOPE)
    # the C entry point itself refuses a padded stride
    L = S._lib.lib()
    rc = L.sgs_gatv2_alpha_heads_fwd_multi(xb.data_ptr(), xb.data_ptr(), N * K * C + 4, att.data_ptr(), None, None, N, K, C, 2, q, ops._ptr(csr[0]),
                                           ops._ptr(csr[1]), ops._ptr(csr[2]), SLOPE, xb.data_ptr(), xb.data_ptr(), None)
    assert rc == -1 and b"x_stride" in L.sgs_last_error()


@pytest.mark.parametrize("graph", ["hub", "dense", "empty"])
def test_the_aggregation_over_the_new_alphas_equals_the_single_draw_aggregation(graph):
    import sgs_gnn_amd as S
    ops = S.ops
    D, K, C = 3, 8, 8
    N, q, smp, csr, gds, r = _check_blocks(S, graph, D, K, C, "blocks", graph != "empty")
    bias_c, bias_m = torch.randn(K * C).to(DEV), torch.randn(C).to(DEV)
    xl = r["xl"]
    for mode, bias, act in ((ops.HEADS_CONCAT, bias_c, ops.ACT_RELU), (ops.HEADS_MEAN, bias_m, ops.ACT_NONE)):
        Y = ops._spmm_heads_multi(xl, N * K * C, csr, r["alpha"], r["alpha_loop"], mode, bias, act, q, N, K, C)
        for d in range(D):
            gd = gds[d]
            a, al = r["alpha"][d].contiguous(), r["alpha_loop"][d].contiguous()          # (bitwise the single-draw softmax's: _check_blocks)
            one = ops._spmm_heads(xl[d].contiguous(), gd.in_ptr, gd.in_src, gd.in_eid, a, al, mode, bias, act, 0.0, 0, 0, N, K, C, q)
            assert torch.equal(Y[d], one), (graph, mode, d)


# ------------------------------------------------------------------ the engine
def _model(S, fin, hid, ncls, K, edge, scorer_state=None, seed=0):
    torch.manual_seed(seed)
    m = S.GATModel(fin, hid, ncls, dropout_prob=0.3, edge_mlp_type="GCN", gat_heads=K, gat_edge_weight=edge, gat_v2=True)
    if scorer_state is not None:
        m.load_state_dict({k: v for k, v in scorer_state.items() if k.startswith("edge_prob_mlp.")}, strict=False)
    with torch.no_grad():                                        # biases and the edge Linears: make them count
        for n_, p_ in m.named_parameters():
            if n_.startswith("edge_prob_mlp."):
                continue
            if n_.endswith("bias"):
                p_.copy_(torch.randn(p_.shape) * 0.1)
            elif "lin_edge" in n_:
                p_.copy_(torch.rand(p_.shape) * 2 - 1)
    return m.to(DEV)


_FIXTURE = {}
MODELS = [(1, False), (1, True), (4, False), (4, True)]


def _fixture(K=4, edge=True):
    """-> (fx, model, sampled partition (E > q), whole partition (E <= q: the shortcut), generator); partitions and models built once."""
    import sgs_gnn_amd as S
    if "data" not in _FIXTURE:
        fx = load_golden("pipeline_hybrid_gcn.pt")
        n = fx["x"].shape[0]
        g = torch.Generator().manual_seed(1)
        val = torch.rand(n, generator=g) < 0.5
        masks = dict(y=fx["y"], train_mask=fx["train_mask"], val_mask=val & ~fx["train_mask"], test_mask=~val & ~fx["train_mask"])
        b = S.Batch(x=fx["x"], edge_index=fx["edge_index"], prob=fx["prob"], **masks)
        q = fx["q"]
        keep = torch.randperm(fx["edge_index"].shape[1], generator=g)[:q // 2].sort().values
        pr = fx["prob"][keep]
        small = S.Batch(x=fx["x"], edge_index=fx["edge_index"][:, keep].contiguous(), prob=pr / pr.sum(), **masks)
        assert b.edge_index.shape[1] > q and small.edge_index.shape[1] <= q      # both branches of the engine are taken
        _FIXTURE["data"] = (fx, b, small)
    fx, b, small = _FIXTURE["data"]
    if (K, edge) not in _FIXTURE:
        _FIXTURE[(K, edge)] = _model(S, fx["x"].shape[1], 16, 5, K, edge, fx["state0"])
    return fx, _FIXTURE[(K, edge)], b, small, torch.Generator().manual_seed(2)


ON = dict(sgs_eval_batch_heads="all", sgs_eval_batch_gatv2=True)


def _run(S, m, batches, q, mode, draws, flag, seed=7, extra=None):
    """One ensemble_evaluate from fixed clocks; flag None = the serial loop.  -> (f1, traces, (noise tick, dropout tick))."""
    path = "serial" if flag is None else "batched"
    args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws, **(extra or {}))
    if flag is not None:
        args.sgs_eval_batch = flag
        for k, v in ON.items():
            setattr(args, k, v)
        if extra and extra.get("sgs_cover_nodes"):
            args.sgs_eval_batch_cover = True
    S.manual_seed(seed)
    before = dict(_ev().PATH_COUNTS)
    traces = []
    args._sgs_trace_eval = {}
    f1 = S.ensemble_evaluate(args, m, batches, DEV, q=q, mode=mode)
    after = dict(_ev().PATH_COUNTS)
    other = "serial" if path == "batched" else "batched"
    assert after[path] == before[path] + 1 and after[other] == before[other]
    traces.append(dict(args._sgs_trace_eval))
    if len(batches) > 1:
        args._sgs_trace_eval = {}
        S.ensemble_evaluate(args, m, batches[:1], DEV, q=q, mode=mode)
        traces.append(dict(args._sgs_trace_eval))
    return f1, traces, (S.sampling._NoiseClock.tick, S.model._DropoutClock.tick)


def _assert_same(serial, batched):
    (f_s, ts, k_s), (f_b, tb, k_b) = serial, batched
    assert k_s == k_b                     # both clocks: the noise clock and the dropout clock
    assert f_s == f_b
    for t_s, t_b in zip(ts, tb):
        assert set(t_b) == set(t_s) == {"logits", "mean", "edges"}
        assert torch.equal(t_s["edges"], t_b["edges"])
        assert t_b["logits"].shape == t_s["logits"].shape
        scale = float(t_s["logits"].abs().max())
        dl, dm = float((t_b["logits"] - t_s["logits"]).abs().max()), float((t_b["mean"] - t_s["mean"]).abs().max())
        print(f"max|logits| = {scale:.4e}: per-draw diff {dl:.3e}, mean diff {dm:.3e} (tolerance {SERIAL_TOL * scale:.3e})")
        assert dl <= SERIAL_TOL * scale and dm <= SERIAL_TOL * scale


@pytest.mark.parametrize("mode", ["learned", "edge", "random", "full"])
@pytest.mark.parametrize("K,edge", MODELS)
def test_batched_gatv2_equals_the_serial_loop(mode, K, edge):
    """[sampled, whole] partitions, sgs_eval_batch True and 3 against one serial run: the first trace is the whole partition's (E <= q
    shortcut), the second call's the sampled one's.  Logits within SERIAL_TOL x max|logits|, not bitwise (layer 2's GEMM over D N rows)."""
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture(K, edge)
    serial = _run(S, m, [b, small], fx["q"], mode, 5, None)
    for flag in (True, 3):
        batched = _run(S, m, [b, small], fx["q"], mode, 5, flag)
        _assert_same(serial, batched)
        sampled, whole = batched[1][1], batched[1][0]
        assert whole["edges"].shape[2] == small.edge_index.shape[1]
        if mode != "full":
            assert sampled["edges"].shape[2] == fx["q"] and not torch.equal(sampled["edges"][0], sampled["edges"][1])      # draws really happen
            assert not torch.equal(sampled["logits"][0], sampled["logits"][1])                                             # and reach the logits


def _learned_draws(S, m, b, q, noises):
    ops = S.ops
    bd = b.to(DEV)
    m.eval()
    with torch.no_grad():
        ops.get_pairs(bd.edge_index, bd.x.shape[0], build=True)
        p = m.edge_prob_mlp(bd.x, bd.edge_index).squeeze().contiguous()
    smp = ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.0, q, bd.edge_index, len(noises), noise=torch.stack(noises), want_edge_index=True,
                                want_w=True)
    return bd, smp


def _v2_inputs(m, x):
    c = m.GAT.convs[0]
    W = c.heads * c.out_channels
    return c.lin_l(x).contiguous(), c.lin_r(x).contiguous(), W


@pytest.mark.parametrize("K,edge", MODELS)
def test_batched_gatv2_matches_fp64_with_explicit_noise(K, edge):
    """Per-draw logits against gatv2_ref.gatv2_model in fp64 under FWD_BOUND (test_gpu_gatv2.py's logits bound, as a max-abs error over the
    max-abs reference); with gat_edge_weight the same draws without weights give other logits."""
    import sgs_gnn_amd as S
    ops = S.ops
    fx, m, b, small, g = _fixture(K, edge)
    E, q, draws = fx["edge_index"].shape[1], fx["q"], 4
    noises = [torch.empty(E).exponential_(1, generator=g).to(DEV) for _ in range(draws)]
    args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws, sgs_eval_batch=True, _sgs_noise_eval=list(noises), _sgs_trace_eval={},
                              **ON)
    before = _ev().PATH_COUNTS["batched"]
    S.ensemble_evaluate(args, m, [b], DEV, q=q, mode="learned")
    assert _ev().PATH_COUNTS["batched"] == before + 1
    got, edges = args._sgs_trace_eval["logits"], args._sgs_trace_eval["edges"]
    bd, smp = _learned_draws(S, m, b, q, noises)
    assert torch.equal(smp.edge_index, edges)
    P = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    x = fx["x"].double()
    for d in range(draws):
        ref = gatv2_ref.gatv2_model(P, x, edges[d].cpu(), smp.w[d].double().cpu() if edge else None, K, 16, 5)
        err = float((got[d].double().cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)
        print(f"K={K} edge={edge} draw {d}: max-abs error / max-abs reference = {err:.3e}")
        assert err <= FWD_BOUND, (d, err)
    if edge:
        # the same draws without weights give other logits: the weights reach the attention
        parent = ops.get_graph(bd.edge_index, bd.x.shape[0])
        with torch.no_grad():
            xl1, xr1, _ = _v2_inputs(m, bd.x)
            unit = S.eval_batch._drawn_gatv2_logits(parent, smp, tuple(m.GAT.convs), xl1, xr1, None)
            again = S.eval_batch._drawn_gatv2_logits(parent, smp, tuple(m.GAT.convs), xl1, xr1, smp.w)
        assert float((again - got).abs().max()) <= SERIAL_TOL * float(got.abs().max())
        assert float((unit - got).abs().max()) > 100 * SERIAL_TOL * float(got.abs().max())


@pytest.mark.parametrize("mode", ["learned", "edge", "random"])
def test_under_node_covering_draws_the_engine_equals_the_serial_covering_loop(mode):
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture()
    extra = dict(sgs_cover_nodes=True)
    _assert_same(_run(S, m, [b, small], fx["q"], mode, 5, None, extra=extra), _run(S, m, [b, small], fx["q"], mode, 5, True, extra=extra))


def test_two_identical_batched_evaluations_are_bitwise_equal():
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture()
    a = _run(S, m, [b, small], fx["q"], "learned", 11, True)
    c = _run(S, m, [b, small], fx["q"], "learned", 11, True)
    assert a[0] == c[0] and a[2] == c[2]
    for ta, tc in zip(a[1], c[1]):
        assert torch.equal(ta["logits"], tc["logits"]) and torch.equal(ta["mean"], tc["mean"]) and torch.equal(ta["edges"], tc["edges"])
    # the split into passes does not change a draw: 11 in one pass against passes of 3 (softmax and aggregation bitwise per draw; layer 2's
    # GEMM sees other row counts, hence the tolerance)
    k3 = _run(S, m, [b, small], fx["q"], "learned", 11, 3)
    assert k3[0] == a[0] and k3[2] == a[2] and torch.equal(k3[1][1]["edges"], a[1][1]["edges"])
    scale = float(a[1][1]["logits"].abs().max())
    assert float((k3[1][1]["logits"] - a[1][1]["logits"]).abs().max()) <= SERIAL_TOL * scale


def test_training_after_batched_evaluation_draws_the_same_dropout_seed_and_masks():
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture()
    bd = b.to(DEV)
    state, seeds, outs = [], [], []
    for path in ("serial", "batched"):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=4)
        if path == "batched":
            args.sgs_eval_batch = True
            for k, v in ON.items():
                setattr(args, k, v)
        S.manual_seed(3)
        S.ensemble_evaluate(args, m, [b, small, b], DEV, q=fx["q"], mode="learned")
        state.append((S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
        m.train()
        with torch.no_grad():
            outs.append(m(bd, bd.edge_index))                    # a training forward: dropout on
        m.eval()
        seeds.append(S.model._DropoutClock.next_seed())
    assert state[0] == state[1] and state[0][0] > 0 and state[0][1] > 0
    assert seeds[0] == seeds[1]
    assert torch.equal(outs[0], outs[1])


def test_without_the_new_opt_in_every_other_opt_in_keeps_the_serial_loop():
    import sgs_gnn_amd as S
    ev = _ev()
    fx, m, b, small, _ = _fixture()
    old = dict(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True)
    runs = []
    for kw in ({}, dict(old, sgs_eval_batch_cover=True), dict(old, sgs_eval_batch_gine=True), dict(old, sgs_eval_batch_gatv2=False),
               dict(old, sgs_eval_batch_gine=True, sgs_eval_batch_cover=True, sgs_eval_batch_gatv2=None),
               dict(sgs_eval_batch=3, sgs_eval_batch_heads=["GAT"])):
        a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, _sgs_trace_eval={}, **kw)
        S.manual_seed(7)
        before = dict(ev.PATH_COUNTS)
        f1 = S.ensemble_evaluate(a, m, [b], DEV, q=fx["q"], mode="learned")
        assert ev.PATH_COUNTS["serial"] == before["serial"] + 1 and ev.PATH_COUNTS["batched"] == before["batched"], kw
        runs.append((f1, a._sgs_trace_eval["logits"]))
    for f1, logits in runs[1:]:
        assert f1 == runs[0][0] and torch.equal(logits, runs[0][1])


def test_partition_shaped_case_eight_heads_with_the_edge_term():
    """N = 1013, F = 602, hidden 64, C = 41, E ~ 60 000, q = 20 000, 11 draws, learned mode, 8 heads with the edge term: layer 1 (8 heads
    of 8 channels) takes VEC 4 / ONE, layer 2 (8 heads of 41 channels, 8 lanes per head) VEC 1 / !ONE."""
    import sgs_gnn_amd as S
    N, F, H, C, q = 1013, 602, 64, 41, 20_000
    b = S.synthetic_graph(N, 60_000, F, C, seed=41, train_frac=0.3, power=0.6, device=DEV)
    E = b.edge_index.shape[1]
    assert 55_000 <= E <= 60_000
    L = S._lib.lib()
    v1, v2 = L.sgs_gatv2_variant(0, N, 8, H // 8, 1), L.sgs_gatv2_variant(0, N, 8, C, 1)
    assert (v1 // 100000 % 10, v1 // 100 % 10) == (4, 1) and (v2 // 100000 % 10, v2 // 100 % 10) == (1, 0)
    assert v2 == L.sgs_gatv2_variant(0, N, 8, C, 0)                                      # C % 4 != 0: the alignment plays no part
    m = _model(S, F, H, C, 8, True, seed=5)
    serial = _run(S, m, [b], q, "learned", 11, None)
    batched = _run(S, m, [b], q, "learned", 11, True)
    _assert_same(serial, batched)
    t = batched[1][0]
    assert t["logits"].shape == (11, N, C) and not torch.equal(t["edges"][0], t["edges"][1]) and not torch.equal(t["logits"][0], t["logits"][1])
