"""GPU: the batched ensemble-evaluation engine for multi-head / edge-weighted GAT and Chebyshev K > 1 (args.sgs_eval_batch_variants).
Kernel level: every multi-draw kernel's block d is bitwise the single-draw kernel on draw d's arrays.  Engine level: against the serial
loop (drawn edge sets, F1, clocks, per-draw logits -- bitwise: the engine's kernels run the single-draw device code per draw, and the
Chebyshev degree is summed in the serial order), against the fp64 references, determinism, and the dropout seed
training sees afterwards."""
import argparse
import sys

import pytest
import torch

import cheb_ref
import gat_edge_ref
from conftest import load_golden
from test_gpu_gat_heads import _two_layer_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_BOUND = 1e-5          # max-abs error over max-abs reference: test_gpu_gat_heads.py / test_gpu_gat_edge.py / test_gpu_cheb.py forward bound


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


# ------------------------------------------------------------------ kernel level
def _hub_graph():
    """300 nodes: 50 isolated (250..299), self loops on nodes 5..39, a duplicated edge, node 0 with 200 in-edges and node 1 with 200
    out-edges (in- and out-degree >> 64 after a draw of 700 of ~1080)."""
    g = torch.Generator().manual_seed(5)
    hub_in = torch.stack([torch.arange(1, 201), torch.zeros(200, dtype=torch.int64)])
    hub_out = torch.stack([torch.ones(200, dtype=torch.int64), torch.arange(2, 202)])
    rnd = torch.randint(1, 250, (2, 600), generator=g)
    loops = torch.arange(5, 40).repeat(2, 1)
    ei = torch.cat([hub_in, hub_out, rnd, loops, rnd[:, :3]], dim=1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous(), 300, 700


def _dense_graph():
    """24 nodes, 3000 edges (duplicates and self loops included): q = 2000 >= 16 N, the row-per-workgroup form of the Chebyshev step."""
    g = torch.Generator().manual_seed(6)
    return torch.randint(0, 24, (2, 3000), generator=g), 24, 2000


def _very_dense_graph():
    """6 nodes, 4000 edges: q = 3000 >= 256 N, the 16-wave row form."""
    g = torch.Generator().manual_seed(7)
    return torch.randint(0, 6, (2, 4000), generator=g), 6, 3000


GRAPHS = {"hub": _hub_graph, "dense": _dense_graph, "very_dense": _very_dense_graph}


def _draws(S, name, D):
    """-> (N, q, smp, csr, [single-draw Graph per draw], parent Graph, generator); "empty": E = 0, CSRs made by hand."""
    ops = S.ops
    g = torch.Generator().manual_seed(D)
    if name == "empty":
        N = 25
        i32 = dict(dtype=torch.int32, device=DEV)
        csr = (torch.zeros(D, N + 1, **i32), torch.zeros(D, 1, **i32), torch.zeros(D, 1, **i32), torch.full((D, N), -1, **i32))
        gd = ops.Graph(torch.zeros(2, 0, dtype=torch.int64, device=DEV), N)
        return N, 0, None, csr, [gd] * D, gd, g
    ei, N, q = GRAPHS[name]()
    ei = ei.to(DEV)
    p = torch.rand(ei.shape[1], generator=g).to(DEV)
    smp = ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.0, q, ei, D, seed=9, stream_id0=1, want_edge_index=True, want_w=True)
    parent = ops.get_graph(ei, N)
    csr = ops.graph_filter_multi(parent, smp)
    gds = []
    for d in range(D):
        gd = ops.Graph(smp.edge_index[d].contiguous(), N)
        assert torch.equal(gd.in_ptr, csr[0][d]) and torch.equal(gd.in_src[:q], csr[1][d, :q]) and torch.equal(gd.in_eid[:q], csr[2][d, :q])
        gds.append(gd)
    return N, q, smp, csr, gds, parent, g


def _single_alpha_heads(S, a_s, a_d, gd, K, w=None, coef=None):
    L, ops = S._lib.lib(), S.ops
    N, n = gd.N, gd.n_edges
    f32 = dict(dtype=torch.float32, device=DEV)
    soft, alpha = torch.empty(max(n, 1), K, **f32), torch.empty(max(n, 1), K, **f32)
    soft_loop, alpha_loop = torch.empty(N, K, **f32), torch.empty(N, K, **f32)
    if w is None:
        S._lib.check(L.sgs_gat_alpha_heads_fwd(ops._ptr(a_s), ops._ptr(a_d), N, K, n, ops._ptr(gd.in_ptr), ops._ptr(gd.in_src), ops._ptr(gd.in_eid),
                                               0.2, 0.0, 0, 16, ops._ptr(soft), ops._ptr(soft_loop), ops._ptr(alpha), ops._ptr(alpha_loop),
                                               ops._stream()), "sgs_gat_alpha_heads_fwd")
    else:
        loop = torch.empty(2, N, **f32)
        S._lib.check(L.sgs_gat_alpha_heads_edge_fwd(ops._ptr(a_s), ops._ptr(a_d), ops._ptr(w), ops._ptr(coef), N, K, n, ops._ptr(gd.in_ptr),
                                                    ops._ptr(gd.in_src), ops._ptr(gd.in_eid), 0.2, 0.0, 0, 16, ops._ptr(soft), ops._ptr(soft_loop),
                                                    ops._ptr(alpha), ops._ptr(alpha_loop), loop[0].data_ptr(), loop[1].data_ptr(), ops._stream()),
                     "sgs_gat_alpha_heads_edge_fwd")
    return alpha[:n], alpha_loop


HEAD_CASES = [(1, True), (2, False), (2, True), (8, False), (8, True), (16, False), (16, True)]      # (heads, edge term); one head: edge term only


@pytest.mark.parametrize("D", [1, 3, 11])
@pytest.mark.parametrize("graph", ["hub", "dense", "empty"])
@pytest.mark.parametrize("K,edge", HEAD_CASES)
def test_alpha_heads_and_spmm_heads_multi_equal_the_single_draw_kernels(D, graph, K, edge):
    import sgs_gnn_amd as S
    ops = S.ops
    N, q, smp, csr, gds, _, g = _draws(S, graph, D)
    coef = torch.randn(K, generator=g).to(DEV) if edge else None
    w = (smp.w if smp is not None else torch.zeros(D, 0, device=DEV)) if edge else None
    if smp is not None:
        deg = csr[0][0, 1:] - csr[0][0, :-1]
        assert graph != "hub" or (int(deg[0]) > 64 and int((deg[250:] != 0).sum()) == 0)
    for C in (8, 5):                                             # 16-byte rows and column-by-column rows
        Xs = torch.randn(N, K * C, generator=g).to(DEV)          # layer 1: shared
        Xd = torch.randn(D, N, K * C, generator=g).to(DEV)       # layer 2: per draw
        bias_c, bias_m = torch.randn(K * C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
        for shared in (True, False):
            if shared:
                a_s, a_d, stride = torch.randn(N, K, generator=g).to(DEV), torch.randn(N, K, generator=g).to(DEV), 0
            else:
                a_s, a_d, stride = torch.randn(D, N, K, generator=g).to(DEV), torch.randn(D, N, K, generator=g).to(DEV), N * K
            kw = dict(edge_w=w, edge_coef=coef) if edge else {}
            alpha, alpha_loop = ops.gat_alpha_heads_multi(a_s, a_d, stride, csr, q, N, K, 0.2, **kw)
            X, xs = (Xs, 0) if shared else (Xd, N * K * C)
            Yc = ops._spmm_heads_multi(X, xs, csr, alpha, alpha_loop, ops.HEADS_CONCAT, bias_c, ops.ACT_RELU, q, N, K, C)
            Ym = ops._spmm_heads_multi(X, xs, csr, alpha, alpha_loop, ops.HEADS_MEAN, bias_m, ops.ACT_NONE, q, N, K, C)
            for d in range(D):
                gd = gds[d]
                sa, sd = (a_s, a_d) if shared else (a_s[d].contiguous(), a_d[d].contiguous())
                wd = w[d].contiguous() if edge else None
                want, want_loop = _single_alpha_heads(S, sa, sd, gd, K, wd, coef)
                assert torch.equal(alpha[d, :q], want), (d, C, shared)
                assert torch.equal(alpha_loop[d], want_loop), (d, C, shared)
                Xone = Xs if shared else Xd[d].contiguous()
                al, lo = alpha[d].contiguous(), alpha_loop[d].contiguous()
                for mode, Y, b, act in ((ops.HEADS_CONCAT, Yc, bias_c, ops.ACT_RELU), (ops.HEADS_MEAN, Ym, bias_m, ops.ACT_NONE)):
                    one = ops._spmm_heads(Xone, gd.in_ptr, gd.in_src, gd.in_eid, al, lo, mode, b, act, 0.0, 0, 0, N, K, C, q)
                    assert torch.equal(Y[d], one), (d, C, shared, mode)


def test_spmm_heads_multi_wide_mean_rows_keep_the_non_lds_form():
    """K C > 1024 floats: the head mean whose lanes walk the heads (a different summation order from the LDS form: the choice must agree)."""
    import sgs_gnn_amd as S
    ops = S.ops
    D, K, C = 3, 16, 72
    N, q, smp, csr, gds, _, g = _draws(S, "hub", D)
    a_s, a_d = torch.randn(N, K, generator=g).to(DEV), torch.randn(N, K, generator=g).to(DEV)
    alpha, alpha_loop = ops.gat_alpha_heads_multi(a_s, a_d, 0, csr, q, N, K, 0.2)
    X = torch.randn(D, N, K * C, generator=g).to(DEV)
    b = torch.randn(C, generator=g).to(DEV)
    Y = ops._spmm_heads_multi(X, N * K * C, csr, alpha, alpha_loop, ops.HEADS_MEAN, b, ops.ACT_NONE, q, N, K, C)
    for d in range(D):
        one = ops._spmm_heads(X[d].contiguous(), gds[d].in_ptr, gds[d].in_src, gds[d].in_eid, alpha[d].contiguous(), alpha_loop[d].contiguous(),
                              ops.HEADS_MEAN, b, ops.ACT_NONE, 0.0, 0, 0, N, K, C, q)
        assert torch.equal(Y[d], one)


@pytest.mark.parametrize("K", [2, 8, 16])
def test_gat_scores_heads_over_stacked_draws_is_per_row(K):
    import sgs_gnn_amd as S
    g = torch.Generator().manual_seed(3)
    D, N, C = 5, 777, 5
    z = torch.randn(D * N, K * C, generator=g).to(DEV)
    att_s, att_d = torch.randn(1, K, C, generator=g).to(DEV), torch.randn(1, K, C, generator=g).to(DEV)
    a_s, a_d = S.ops.gat_scores(z, att_s, att_d, heads=K)
    for d in range(D):
        s1, d1 = S.ops.gat_scores(z[d * N:(d + 1) * N].contiguous(), att_s, att_d, heads=K)
        assert torch.equal(a_s[d * N:(d + 1) * N], s1) and torch.equal(a_d[d * N:(d + 1) * N], d1)


@pytest.mark.parametrize("D", [1, 3, 11])
@pytest.mark.parametrize("graph", ["hub", "dense", "very_dense"])
@pytest.mark.parametrize("weighted", [True, False])
def test_cheb_norm_and_step_multi_equal_the_single_draw_kernels(D, graph, weighted):
    import sgs_gnn_amd as S
    ops = S.ops
    N, q, smp, csr, gds, parent, g = _draws(S, graph, D)
    w = smp.w if weighted else None
    dis, l_in = ops.cheb_norm_multi(parent, smp, csr, w)
    for d in range(D):
        nm = ops._cheb_norm_forward(gds[d], w[d].contiguous() if weighted else None)
        assert torch.equal(dis[d], nm.dis), d                    # the by-source degree: same values in the same order
        assert torch.equal(l_in[d, :q], nm.what_in[:q]), d
    if graph == "hub":
        out_deg = torch.bincount(smp.edge_index[0, 0], minlength=N)
        assert int(out_deg[1]) > 64                              # a row the wave walks more than once
    for W in (8, 5):
        ld = 3 * W                                               # operands are column blocks of wider buffers
        for shared in (True, False):
            Xb = torch.randn(*((N, ld) if shared else (D, N, ld)), generator=g).to(DEV)
            Ab = torch.randn(*((N, ld) if shared else (D, N, ld)), generator=g).to(DEV)
            st = 0 if shared else N * ld
            bias = torch.randn(W, generator=g).to(DEV)
            Y = torch.empty(D, N, W, device=DEV)
            ops._cheb_step_multi(3, Xb.data_ptr() + 4 * W, ld, st, N, W, q, D, csr, l_in, 2.0, Ab.data_ptr(), ld, st, Ab.data_ptr() + 8 * W, ld, st,
                                 bias, ops.ACT_RELU, Y.data_ptr(), W, N * W)
            for d in range(D):
                xb, ab = (Xb, Ab) if shared else (Xb[d], Ab[d])
                one = torch.empty(N, W, device=DEV)
                ops._cheb_step(3, xb.data_ptr() + 4 * W, ld, N, W, gds[d].in_ptr, gds[d].in_src, l_in[d].contiguous(), q, 2.0, ab.data_ptr(), ld,
                               ab.data_ptr() + 8 * W, ld, bias, ops.ACT_RELU, 0.0, 0, 0, one.data_ptr(), W)
                assert torch.equal(Y[d], one), (d, W, shared)


# ------------------------------------------------------------------ the engine
MODELS = {"gat_heads4": ("GAT", dict(gat_heads=4)), "gat_edge": ("GAT", dict(gat_edge_weight=True)),
          "gat_heads4_edge": ("GAT", dict(gat_heads=4, gat_edge_weight=True)), "cheb_k3": ("Cheb", dict(cheb_k=3)),
          "gat_heads16": ("GAT", dict(gat_heads=16)), "cheb_k8": ("Cheb", dict(cheb_k=8))}
NAMES = tuple(MODELS)


def _model(S, name, fin, hid, ncls, scorer_state=None, seed=0):
    torch.manual_seed(seed)
    head, kw = MODELS[name]
    m = (S.GATModel if head == "GAT" else S.ChebModel)(fin, hid, ncls, dropout_prob=0.3, edge_mlp_type="GCN", **kw)
    if scorer_state is not None:
        m.load_state_dict({k: v for k, v in scorer_state.items() if k.startswith("edge_prob_mlp.")}, strict=False)
    with torch.no_grad():                                        # biases are zero-initialised: make them count
        for n_, p_ in m.named_parameters():
            if n_.endswith("bias") and not n_.startswith("edge_prob_mlp."):
                p_.copy_(torch.randn(p_.shape) * 0.1)
    return m.to(DEV)


def _fixture(name):
    """-> (fx, model, sampled partition (E > q), whole partition (E <= q: the shortcut), generator)."""
    import sgs_gnn_amd as S
    fx = load_golden("pipeline_hybrid_gcn.pt")
    m = _model(S, name, fx["x"].shape[1], 16, 5, fx["state0"])
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
    return fx, m, b, small, g


def _both(S, m, batches, q, mode, draws, flag, seed=7):
    res = {}
    for path in ("serial", "batched"):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws)
        if path == "batched":
            args.sgs_eval_batch, args.sgs_eval_batch_heads, args.sgs_eval_batch_variants = flag, "all", True
        S.manual_seed(seed)
        before = dict(_ev().PATH_COUNTS)
        f1, traces = None, []
        # one call per partition list keeps the last partition's trace; evaluate each prefix's last partition through a list of its own
        args._sgs_trace_eval = {}
        f1 = S.ensemble_evaluate(args, m, batches, DEV, q=q, mode=mode)
        assert _ev().PATH_COUNTS[path] == before[path] + 1
        traces.append(dict(args._sgs_trace_eval))
        args._sgs_trace_eval = {}
        S.ensemble_evaluate(args, m, batches[:1], DEV, q=q, mode=mode)
        traces.append(dict(args._sgs_trace_eval))
        res[path] = (f1, traces, (S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
    return res


def _assert_same(res, bitwise=True):
    (f_s, ts, k_s), (f_b, tb, k_b) = res["serial"], res["batched"]
    assert k_s == k_b                     # both clocks: the noise clock and the dropout clock
    assert f_s == f_b
    for t_s, t_b in zip(ts, tb):
        assert set(t_b) == set(t_s) == {"logits", "mean", "edges"}
        assert torch.equal(t_s["edges"], t_b["edges"])
        assert t_b["logits"].shape == t_s["logits"].shape
        assert torch.equal(t_b["logits"], t_s["logits"])
        assert torch.equal(t_b["mean"], t_s["mean"])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ["learned", "edge", "random", "full"])
@pytest.mark.parametrize("flag", [True, 3])
def test_batched_variants_equal_the_serial_loop_bitwise(name, mode, flag):
    """[sampled, whole] partitions: the last trace is the whole partition's (E <= q shortcut), the second call's the sampled one's."""
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture(name)
    res = _both(S, m, [b, small], fx["q"], mode, 5, flag)
    _assert_same(res)
    sampled, whole = res["batched"][1][1], res["batched"][1][0]
    assert whole["edges"].shape[2] == small.edge_index.shape[1]
    if mode != "full":
        assert sampled["edges"].shape[2] == fx["q"] and not torch.equal(sampled["edges"][0], sampled["edges"][1])      # draws really happen
        assert not torch.equal(sampled["logits"][0], sampled["logits"][1])                                             # and reach the logits


@pytest.mark.parametrize("name", NAMES)
def test_batched_variants_match_fp64_with_explicit_noise(name):
    import sgs_gnn_amd as S
    ops = S.ops
    fx, m, b, small, g = _fixture(name)
    E, q, draws = fx["edge_index"].shape[1], fx["q"], 4
    noises = [torch.empty(E).exponential_(1, generator=g).to(DEV) for _ in range(draws)]
    args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws, sgs_eval_batch=True, sgs_eval_batch_heads="all",
                              sgs_eval_batch_variants=True, _sgs_noise_eval=list(noises), _sgs_trace_eval={})
    before = _ev().PATH_COUNTS["batched"]
    S.ensemble_evaluate(args, m, [b], DEV, q=q, mode="learned")
    assert _ev().PATH_COUNTS["batched"] == before + 1
    got, edges = args._sgs_trace_eval["logits"], args._sgs_trace_eval["edges"]
    # the same draws and their straight-through weights, for the references
    bd = b.to(DEV)
    m.eval()
    with torch.no_grad():
        ops.get_pairs(bd.edge_index, bd.x.shape[0], build=True)
        p = m.edge_prob_mlp(bd.x, bd.edge_index).squeeze().contiguous()
    smp = ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.0, q, bd.edge_index, draws, noise=torch.stack(noises), want_edge_index=True, want_w=True)
    assert torch.equal(smp.edge_index, edges)
    P = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    x = fx["x"].double()
    head, kw = MODELS[name]
    for d in range(draws):
        ei, w = edges[d].cpu(), smp.w[d].double().cpu()
        if head == "Cheb":
            ref = cheb_ref.model(P, x, ei, w, kw["cheb_k"])
        elif kw.get("gat_edge_weight"):
            ref = gat_edge_ref.gat_edge_model(P, x, ei, w, kw.get("gat_heads", 1), 16, 5)
        else:
            ref = _two_layer_ref(P, x, ei, kw["gat_heads"], 16, 5)
        err = float((got[d].double().cpu() - ref).abs().max()) / float(ref.abs().max())
        print(f"{name} draw {d}: max-abs error / max-abs reference = {err:.3e}")
        assert err <= FWD_BOUND, (name, d, err)


@pytest.mark.parametrize("name", ["gat_heads4_edge", "cheb_k3"])
def test_two_identical_batched_passes_are_bitwise_equal(name):
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture(name)
    a = _both(S, m, [b, small], fx["q"], "learned", 11, True)["batched"]
    c = _both(S, m, [b, small], fx["q"], "learned", 11, True)["batched"]
    assert a[0] == c[0] and a[2] == c[2]
    for ta, tc in zip(a[1], c[1]):
        assert torch.equal(ta["logits"], tc["logits"]) and torch.equal(ta["mean"], tc["mean"]) and torch.equal(ta["edges"], tc["edges"])


@pytest.mark.parametrize("name", ["gat_heads4_edge", "cheb_k3"])
def test_training_after_batched_variant_evaluation_draws_the_same_dropout_seed(name):
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture(name)
    bd = b.to(DEV)
    state, seeds, outs = [], [], []
    for path in ("serial", "batched"):
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=4)
        if path == "batched":
            args.sgs_eval_batch, args.sgs_eval_batch_heads, args.sgs_eval_batch_variants = True, "all", True
        S.manual_seed(3)
        S.ensemble_evaluate(args, m, [b, small, b], DEV, q=fx["q"], mode="learned")
        state.append((S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
        m.train()
        with torch.no_grad():
            outs.append(m(bd, bd.edge_index))                    # a training forward: dropout on
        m.eval()
        seeds.append(S.model._DropoutClock.next_seed())
    assert state[0] == state[1] and state[0][0] > 0
    assert seeds[0] == seeds[1]
    assert torch.equal(outs[0], outs[1])
