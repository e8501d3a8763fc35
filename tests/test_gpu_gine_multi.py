"""GPU: the batched ensemble-evaluation engine of the GINE head (GINModel(gin_edge_weight=True), args.sgs_eval_batch_gine).

Kernel level: block d of ops.gine_aggregate_multi (sgs_gine_aggregate_fwd_multi) is BITWISE ops.gine_aggregate on draw d's Graph, in every
row form (one wave per row, 4 / 16 waves per row), at VEC 1 / 2 / 4, for a shared x, per-draw blocks and a stride that is not a multiple
of the vector width, with and without weights.

Engine level: against the serial loop from the same clocks -- drawn edge sets torch.equal, F1 equal, both clocks equal, PATH_COUNTS on
the right path, per-draw logits and mean within 1e-5 x max|logits| (tests/test_gpu_ensemble_batched_heads.py's own tolerance, for its
reason: the MLP Linears run as one library GEMM over D N rows, which need not be bitwise the per-draw GEMM; the aggregation itself is
pinned bitwise at kernel level.  The logits are NOT asserted bitwise here) -- against the fp64 model under test_gpu_gine.py's forward
bound, under node-covering draws, determinism, and the dropout seed training sees afterwards."""
import argparse
import sys

import pytest
import torch

import gine_kernels_ref as KR
import gine_ref
from conftest import load_golden
from test_gpu_ensemble_batched_variants import _draws

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_BOUND = 1e-5          # max-abs error over max-abs reference: test_gpu_gine.py's forward bound
SERIAL_TOL = 1e-5         # x max|logits|: test_gpu_ensemble_batched_heads.py's serial-vs-batched tolerance


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


# ------------------------------------------------------------------ kernel level
def _x_of(kind, D, N, Dc, g):
    """-> (x, x_stride, [draw d's [N, Dc] block]) for a shared block, per-draw blocks, or blocks one float further apart than N Dc."""
    if kind == "shared":
        x = torch.randn(N, Dc, generator=g).to(DEV)
        return x, 0, [x] * D
    stride = N * Dc + (1 if kind == "unaligned" else 0)
    flat = torch.randn((D - 1) * stride + N * Dc, generator=g).to(DEV)
    return flat, stride, [flat[d * stride:d * stride + N * Dc].view(N, Dc) for d in range(D)]


def _check_blocks(S, graph, D, Dc, kind, weighted):
    ops = S.ops
    N, q, smp, csr, gds, _, g = _draws(S, graph, D)
    a, b = (torch.rand(Dc, generator=g) * 2 - 1).to(DEV), (torch.rand(Dc, generator=g) * 2 - 1).to(DEV)
    x, stride, blocks = _x_of(kind, D, N, Dc, g)
    w = None
    if weighted:
        w = smp.w if smp is not None else torch.zeros(D, 0, device=DEV)
    z = ops.gine_aggregate_multi(x, stride, csr, w, a, b, KR.DIAG, q, N, Dc)
    assert z.shape == (D, N, Dc)
    for d in range(D):
        wd = w[d].contiguous() if (weighted and q > 0) else None
        one = ops.gine_aggregate(blocks[d].contiguous(), ops.edge_attr(gds[d], wd), a, b, KR.DIAG)
        assert torch.equal(z[d], one), (graph, D, Dc, kind, weighted, d)
    return N, q, smp, csr, gds, (x, stride, blocks, w, a, b, z)


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("graph", ["hub", "dense", "very_dense", "empty"])
@pytest.mark.parametrize("Dc", [5, 70, 132, 602])
def test_every_block_is_bitwise_the_single_draw_aggregate(D, graph, Dc):
    import sgs_gnn_amd as S
    L = S._lib.lib()
    want = {"hub": 0, "dense": 1004, "very_dense": 1016, "empty": 0}[graph]
    N, q = {"hub": (300, 700), "dense": (24, 2000), "very_dense": (6, 3000), "empty": (25, 0)}[graph]
    var = L.sgs_gine_variant(N, Dc, q, 16)
    assert var // 1000 * 1000 + (var % 100 if var >= 1000 else 0) == want                 # the row form the graph is meant to reach
    assert var // 100 % 10 == {5: 1, 70: 2, 132: 4, 602: 2}[Dc]                           # and the vector width of the width
    for kind in ("shared", "blocks") + (("unaligned",) if Dc == 132 else ()):
        for weighted in (False, True):
            n_, q_, smp, csr, _, _ = _check_blocks(S, graph, D, Dc, kind, weighted)
            assert (n_, q_) == (N, q)
    if graph == "hub":
        deg = csr[0][0, 1:] - csr[0][0, :-1]
        assert int(deg[0]) > 64 and int((deg[250:] != 0).sum()) == 0                      # a row of many gathers, and empty rows


def test_null_weights_are_bitwise_a_tensor_of_ones_and_launches_repeat():
    import sgs_gnn_amd as S
    ops = S.ops
    for graph, Dc in (("hub", 70), ("dense", 132), ("very_dense", 5)):
        N, q, smp, csr, gds, g = _draws(S, graph, 3)[:5] + (torch.Generator().manual_seed(2),)
        a, b = (torch.rand(Dc, generator=g) * 2 - 1).to(DEV), (torch.rand(Dc, generator=g) * 2 - 1).to(DEV)
        x = torch.randn(3, N, Dc, generator=g).to(DEV)
        none = ops.gine_aggregate_multi(x, N * Dc, csr, None, a, b, 1.0, q, N, Dc)
        ones = ops.gine_aggregate_multi(x, N * Dc, csr, torch.ones(3, q, device=DEV), a, b, 1.0, q, N, Dc)
        assert torch.equal(none, ones)
        w1 = ops.gine_aggregate_multi(x, N * Dc, csr, smp.w, a, b, 1.0, q, N, Dc)
        w2 = ops.gine_aggregate_multi(x, N * Dc, csr, smp.w, a, b, 1.0, q, N, Dc)
        assert torch.equal(w1, w2) and not torch.equal(w1, none)                           # deterministic, and the weights count


def test_one_case_against_the_fp64_kernel_reference_element_by_element():
    import sgs_gnn_amd as S
    D, Dc = 3, 70
    N, q, smp, csr, gds, (x, stride, blocks, w, a, b, z) = _check_blocks(S, "dense", D, Dc, "blocks", True)
    for d in range(D):
        ref, bound = KR.fwd(blocks[d].cpu(), csr[0][d].cpu(), csr[1][d].cpu(), csr[2][d].cpu(), w[d].cpu(), a.cpu(), b.cpu(), KR.DIAG, bound=True)
        err = (z[d].double().cpu() - ref).abs()
        print(f"draw {d}: max |err| = {float(err.max()):.3e}, max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), d


def test_wrapper_refuses_wrong_shapes():
    import sgs_gnn_amd as S
    ops = S.ops
    N, q, smp, csr, gds, _, g = _draws(S, "hub", 2)
    a = torch.zeros(8, device=DEV)
    x = torch.zeros(N, 8, device=DEV)
    with pytest.raises(RuntimeError, match="x must be"):
        ops.gine_aggregate_multi(x, N * 8, csr, None, a, a, 1.0, q, N, 8)                  # per-draw stride, one block of data
    with pytest.raises(RuntimeError, match="w must be"):
        ops.gine_aggregate_multi(x, 0, csr, torch.zeros(2, q + 1, device=DEV), a, a, 1.0, q, N, 8)
    with pytest.raises(RuntimeError, match="a and b"):
        ops.gine_aggregate_multi(x, 0, csr, None, a[:4], a, 1.0, q, N, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gine_aggregate_multi(x.cpu(), 0, csr, None, a, a, 1.0, q, N, 8)


# ------------------------------------------------------------------ the engine
def _model(S, fin, hid, ncls, scorer_state=None, seed=0):
    torch.manual_seed(seed)
    m = S.GINModel(fin, hid, ncls, dropout_prob=0.3, edge_mlp_type="GCN", gin_edge_weight=True)
    if scorer_state is not None:
        m.load_state_dict({k: v for k, v in scorer_state.items() if k.startswith("edge_prob_mlp.")}, strict=False)
    with torch.no_grad():                                        # biases and the edge Linears: make them count
        for n_, p_ in m.named_parameters():
            if n_.startswith("edge_prob_mlp."):
                continue
            if n_.endswith("bias"):
                p_.copy_(torch.randn(p_.shape) * 0.1)
            elif ".lin." in n_:
                p_.copy_(torch.rand(p_.shape) * 2 - 1)
    return m.to(DEV)


_FIXTURE = {}


def _fixture():
    """-> (fx, model, sampled partition (E > q), whole partition (E <= q: the shortcut), generator); built once."""
    import sgs_gnn_amd as S
    if not _FIXTURE:
        fx = load_golden("pipeline_hybrid_gcn.pt")
        m = _model(S, fx["x"].shape[1], 16, 5, fx["state0"])
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
        _FIXTURE["v"] = (fx, m, b, small)
    return _FIXTURE["v"] + (torch.Generator().manual_seed(2),)


ON = dict(sgs_eval_batch_heads="all", sgs_eval_batch_gine=True)


def _both(S, m, batches, q, mode, draws, flag, seed=7, extra=None, paths=("serial", "batched")):
    res = {}
    for path in paths:
        args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws, **(extra or {}))
        if path == "batched":
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
        res[path] = (f1, traces, (S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
    return res


def _assert_same(res):
    (f_s, ts, k_s), (f_b, tb, k_b) = res["serial"], res["batched"]
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
@pytest.mark.parametrize("flag", [True, 3])
def test_batched_gine_equals_the_serial_loop(mode, flag):
    """[sampled, whole] partitions: the first trace is the whole partition's (E <= q shortcut), the second call's the sampled one's."""
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture()
    res = _both(S, m, [b, small], fx["q"], mode, 5, flag)
    _assert_same(res)
    sampled, whole = res["batched"][1][1], res["batched"][1][0]
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


def test_batched_gine_matches_fp64_with_explicit_noise_and_the_weights_reach_the_messages():
    import sgs_gnn_amd as S
    ops = S.ops
    fx, m, b, small, g = _fixture()
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
        ref = gine_ref.gine_model(P, x, edges[d].cpu(), smp.w[d].double().cpu())
        err = float((got[d].double().cpu() - ref).abs().max()) / float(ref.abs().max())
        print(f"draw {d}: max-abs error / max-abs reference = {err:.3e}")
        assert err <= FWD_BOUND, (d, err)
    # the same draws with unit weights give other logits: the weights reach the messages
    with torch.no_grad():
        unit = S.eval_batch._drawn_gine_logits(ops.get_graph(bd.edge_index, bd.x.shape[0]), smp, None, tuple(m.GIN.convs), bd.x.contiguous())
        again = S.eval_batch._drawn_gine_logits(ops.get_graph(bd.edge_index, bd.x.shape[0]), smp, smp.w, tuple(m.GIN.convs), bd.x.contiguous())
    assert torch.equal(again, got)
    assert not torch.equal(unit, got)


@pytest.mark.parametrize("mode", ["learned", "edge", "random"])
def test_under_node_covering_draws_the_engine_equals_the_serial_covering_loop(mode):
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture()
    res = _both(S, m, [b, small], fx["q"], mode, 5, True, extra=dict(sgs_cover_nodes=True))
    _assert_same(res)


def test_two_identical_batched_evaluations_are_bitwise_equal():
    import sgs_gnn_amd as S
    fx, m, b, small, _ = _fixture()
    a = _both(S, m, [b, small], fx["q"], "learned", 11, True, paths=("batched",))["batched"]
    c = _both(S, m, [b, small], fx["q"], "learned", 11, True, paths=("batched",))["batched"]
    assert a[0] == c[0] and a[2] == c[2]
    for ta, tc in zip(a[1], c[1]):
        assert torch.equal(ta["logits"], tc["logits"]) and torch.equal(ta["mean"], tc["mean"]) and torch.equal(ta["edges"], tc["edges"])
    # the split into passes does not change a draw: 11 in one pass against passes of 3 (per-draw aggregation bitwise; the GEMMs see
    # other row counts, hence the tolerance)
    k3 = _both(S, m, [b, small], fx["q"], "learned", 11, 3, paths=("batched",))["batched"]
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
    assert state[0] == state[1] and state[0][0] > 0
    assert seeds[0] == seeds[1]
    assert torch.equal(outs[0], outs[1])


def test_without_the_new_opt_in_every_other_opt_in_keeps_the_serial_loop():
    import sgs_gnn_amd as S
    ev = _ev()
    fx, m, b, small, _ = _fixture()
    runs = []
    for kw in ({}, dict(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True, sgs_eval_batch_cover=True),
               dict(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True, sgs_eval_batch_gine=False)):
        a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=3, _sgs_trace_eval={}, **kw)
        S.manual_seed(7)
        before = dict(ev.PATH_COUNTS)
        f1 = S.ensemble_evaluate(a, m, [b], DEV, q=fx["q"], mode="learned")
        assert ev.PATH_COUNTS["serial"] == before["serial"] + 1 and ev.PATH_COUNTS["batched"] == before["batched"]
        runs.append((f1, a._sgs_trace_eval["logits"]))
    assert runs[0][0] == runs[1][0] == runs[2][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], runs[2][1])


def test_partition_shaped_case_runs_the_four_wave_row_form_in_both_layers():
    """N = 1013, F = 602, H = 64, C = 41, E ~ 60 000, q = 20 000 >= 16 N, 11 draws, learned mode: 4 waves per row in both layers, VEC 2
    at the input width (variant 1204) and VEC 1 at the hidden width (1104: sgs_gine_variant halves VEC while D <= 32 VEC, 64 -> 2 -> 1)."""
    import sgs_gnn_amd as S
    N, F, H, C, q = 1013, 602, 64, 41, 20_000
    b = S.synthetic_graph(N, 60_000, F, C, seed=41, train_frac=0.3, power=0.6, device=DEV)
    E = b.edge_index.shape[1]
    assert 55_000 <= E <= 60_000 and q >= 16 * N
    L = S._lib.lib()
    assert L.sgs_gine_variant(N, F, q, 16) == 1204 and L.sgs_gine_variant(N, H, q, 16) == 1104
    m = _model(S, F, H, C, seed=5)
    res = _both(S, m, [b], q, "learned", 11, True)
    _assert_same(res)
    t = res["batched"][1][0]
    assert t["logits"].shape == (11, N, C) and not torch.equal(t["edges"][0], t["edges"][1]) and not torch.equal(t["logits"][0], t["logits"][1])
