"""CPU: the batched engine of the GINE head (GINModel(gin_edge_weight=True)) -- the routing opt-in `args.sgs_eval_batch_gine`, the
planner's `gine_in` term, the C entry point sgs_gine_aggregate_fwd_multi (declaration, export, every guard through the error channel) and
an fp64 restatement of eval_batch._drawn_gine_logits' per-draw mathematics held to gine_ref.gine_model.  Nothing here needs a GPU."""
import argparse
import ctypes
import itertools

import pytest
import torch

import gine_ref
from test_eval_batch_cover_cpu import OPTINS, _ABSENT, _Untouchable, _ev, _models


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _ns(base, **extra):
    return argparse.Namespace(**base, **{k: v for k, v in extra.items() if v is not _ABSENT})


# ------------------------------------------------------------------ routing
def _gine_rule(kw):
    """The issue's rule, restated: flag truthy, "GIN" among the selected heads, the new opt-in True; under the cover flag also the cover
    opt-in True."""
    if not kw.get("sgs_eval_batch"):
        return False
    heads = kw.get("sgs_eval_batch_heads")
    if not (heads == "all" or (isinstance(heads, (list, tuple, set)) and "GIN" in heads)):
        return False
    if kw.get("sgs_eval_batch_gine") is not True:
        return False
    return kw.get("sgs_cover_nodes") is not True or kw.get("sgs_eval_batch_cover") is True


def test_truth_table(pkg):
    ev = _ev()
    seen = {True: 0, False: 0}
    optins = OPTINS + [dict(sgs_eval_batch=3, sgs_eval_batch_heads=["GIN"])]
    for (name, (m, _)), base in itertools.product(_models(pkg).items(), optins):
        for cover_flag, cover_optin in ((_ABSENT, _ABSENT), (True, _ABSENT), (True, False), (True, True), (False, True)):
            absent = ev._batched_ok(_ns(base, sgs_cover_nodes=cover_flag, sgs_eval_batch_cover=cover_optin), m, 11)
            for gine in (_ABSENT, None, False, True):
                a = _ns(base, sgs_cover_nodes=cover_flag, sgs_eval_batch_cover=cover_optin, sgs_eval_batch_gine=gine)
                got = ev._batched_ok(a, m, 11)
                if name == "GINE":
                    assert got is _gine_rule(vars(a)), (name, vars(a))
                    seen[got] += 1
                else:
                    assert got is absent, (name, vars(a))                             # every other model: its value with the opt-in absent
            if name in ("GINE", "GATv2"):
                assert absent is False, (name, base)                                  # without the opt-in: never, as before it existed
    assert seen[True] > 0 and seen[False] > 0


def test_the_table_is_not_trivial(pkg):
    """GINE reaches the engine with and without the cover pair; with any one opt-in removed it does not; gat_v2 never does."""
    ev = _ev()
    models = _models(pkg)
    gine, v2 = models["GINE"][0], models["GATv2"][0]
    plain = dict(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_gine=True)
    cover = dict(plain, sgs_cover_nodes=True, sgs_eval_batch_cover=True)
    for full in (plain, cover, dict(plain, sgs_eval_batch=4), dict(plain, sgs_eval_batch_heads=("GIN",)), dict(cover, sgs_eval_batch_variants=True)):
        assert ev._batched_ok(argparse.Namespace(**full), gine, 11) is True, full
        assert ev._batched_ok(argparse.Namespace(**full), v2, 11) is False, full
        for k in full:
            if k == "sgs_cover_nodes" or k == "sgs_eval_batch_variants":
                continue                                                              # (not opt-ins of this head)
            fewer = {a: b for a, b in full.items() if a != k}
            assert ev._batched_ok(argparse.Namespace(**fewer), gine, 11) is False, fewer
    assert ev._batched_ok(argparse.Namespace(**dict(plain, sgs_eval_batch_heads=["GAT", "Cheb"])), gine, 11) is False
    assert ev._batched_ok(argparse.Namespace(**plain), gine, 0) is False
    # the plain GIN model does not need the new opt-in, and is not disturbed by it
    gin = models["GIN"][0]
    for v in (_ABSENT, None, False, True):
        assert ev._batched_ok(_ns(dict(sgs_eval_batch=True, sgs_eval_batch_heads="all"), sgs_eval_batch_gine=v), gin, 11) is True


def test_invalid_values_raise_before_a_loader_is_touched(pkg):
    ev = _ev()
    models = _models(pkg)
    for bad in (1, 0, "yes", [True], 1.0):
        for name in ("GCN", "GINE"):
            m = models[name][0]
            a = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_gine=bad, device="cpu", num_samples_eval=3)
            with pytest.raises(ValueError, match="sgs_eval_batch_gine"):
                ev._batched_ok(a, m, 3)
            before = dict(ev.PATH_COUNTS)
            for mode in ("learned", "random", "edge", "full"):
                with pytest.raises(ValueError, match="sgs_eval_batch_gine"):
                    ev.ensemble_evaluate(a, m, _Untouchable(), "cpu", q=10, mode=mode)
            assert ev.PATH_COUNTS == before
            # consulted only when sgs_eval_batch is truthy, as the other opt-ins
            for off in (False, None, 0):
                assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=off, sgs_eval_batch_gine=bad), m, 3) is False
            assert ev._batched_ok(argparse.Namespace(sgs_eval_batch_gine=bad), m, 3) is False
            # under the cover flag without its opt-in nothing else is consulted (the routing from before the opt-ins existed)
            assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_cover_nodes=True, sgs_eval_batch_gine=bad), m, 3) is False
            with pytest.raises(ValueError, match="sgs_eval_batch_gine"):
                ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_cover_nodes=True, sgs_eval_batch_cover=True, sgs_eval_batch_gine=bad), m, 3)


# ------------------------------------------------------------------ the planner
SHAPES = [(4097, 2000, 900, 16, 5), (100_003, 20_000, 20_000, 64, 7), (463_000, 90_000, 33_869, 256, 40), (351_000, 70_200, 1_013, 256, 41)]
HEAD_KW = [("GCN", {}), ("GAT", {}), ("GIN", {}), ("Cheb", {}), ("GAT", dict(gat_heads=4, gat_edge=True)), ("Cheb", dict(cheb_k=3)),
           ("GIN", dict(cover=True))]
BUDGETS = [True, 1, 4, 100] + [("bytes", n) for n in (1, 1 << 20, 8 << 20, 64 << 20, 1 << 30)]


def _per_today(E, q, N, H, C, head, gat_heads=1, gat_edge=False, cheb_k=1, cover=False):
    """plan_draws' per-draw bytes as its docstring states them for the heads that existed before gine_in."""
    per = 4 * ((E + 63) & ~63) + 5 * E + 40 * q + 36 * (N + 1) + 4 * N * H + 8 * N * C + 3 * 2048 * 4 + 64
    if head == "GAT":
        per += 4 * q * gat_heads + 12 * N * gat_heads + 4 * N * C * (gat_heads - 1) + (8 * N if gat_edge else 0)
    elif head == "GIN":
        per += 4 * N * H + 8 * N * C + 4 * q + 4 * N
    elif head == "Cheb" and cheb_k > 1:
        per += 4 * N * (cheb_k - 1) * (H + C) + 4 * q + 4 * N + 4 * E
    return per + (4 * 1024 + 8 if cover else 0)


def _split(D, k):
    k = max(1, min(D, k))
    return [k] * (D // k) + ([D % k] if D % k else [])


def test_plan_draws_gine_in_zero_is_todays_list(pkg):
    ev = _ev()
    for (E, q, N, H, C), (head, kw), D, budget in itertools.product(SHAPES, HEAD_KW, (1, 3, 11, 64), BUDGETS):
        got = ev.plan_draws(E, q, N, H, C, D, budget, head=head, gine_in=0, **kw)
        assert got == ev.plan_draws(E, q, N, H, C, D, budget, head=head, **kw)
        if budget is True or isinstance(budget, tuple):                               # today's numbers, restated from the docstring
            nbytes = ev.EVAL_BATCH_BUDGET if budget is True else budget[1]
            assert got == _split(D, nbytes // _per_today(E, q, N, H, C, head, **kw)), (head, kw, budget)
        else:
            assert got == _split(D, budget)


def test_plan_draws_gine_term(pkg):
    ev = _ev()
    E, q, N, H, C, D = 351_000, 70_200, 1_013, 256, 41, 11                           # S3's partition shape
    gin = ev.plan_draws(E, q, N, H, C, D, True, head="GIN")
    gine = ev.plan_draws(E, q, N, H, C, D, True, head="GIN", gine_in=602)
    assert sum(gine) == D and min(gine) >= 1 and max(gine) <= max(gin)               # no larger than plain GIN's pass
    for shape, budget in itertools.product(SHAPES, [True] + [("bytes", n) for n in (1 << 20, 8 << 20, 64 << 20, 1 << 30)]):
        e, q_, n, h, c = shape
        last = None
        for F in (1, 2, 12, 128, 602, 4096, 100_000):                                # non-increasing in F
            pl = ev.plan_draws(e, q_, n, h, c, 64, budget, head="GIN", gine_in=F)
            assert sum(pl) == 64 and min(pl) >= 1
            assert last is None or max(pl) <= last, (shape, budget, F)
            last = max(pl)
            for k in (1, 4, 100):                                                    # "at most k": no byte model
                assert ev.plan_draws(e, q_, n, h, c, 64, k, head="GIN", gine_in=F) == ev.plan_draws(e, q_, n, h, c, 64, k, head="GIN")
    # the term is the documented one: base + 4 N F + 8 N H replaces GIN's
    e, q_, n, h, c = SHAPES[0]
    F = 12
    per = _per_today(e, q_, n, h, c, "GCN") + 4 * n * F + 8 * n * h
    assert ev.plan_draws(e, q_, n, h, c, 11, ("bytes", 11 * per), head="GIN", gine_in=F) == [11]
    assert ev.plan_draws(e, q_, n, h, c, 11, ("bytes", 11 * per - 1), head="GIN", gine_in=F) == [10, 1]
    assert ev.plan_draws(e, q_, n, h, c, 11, ("bytes", 11 * per), head="GIN", gine_in=F, cover=True) == [10, 1]
    for head in ("GCN", "GAT", "Cheb"):
        with pytest.raises(ValueError, match="gine_in"):
            ev.plan_draws(e, q_, n, h, c, 11, True, head=head, gine_in=12)
    with pytest.raises(ValueError, match="gine_in"):
        ev.plan_draws(e, q_, n, h, c, 11, True, head="GIN", gine_in=-1)
    with pytest.raises(TypeError):
        ev.plan_draws(e, q_, n, h, c, 11, True, "GIN", 1, False, 1, False, 12)       # keyword-only


# ------------------------------------------------------------------ header and library
def test_the_entry_point_is_declared_exported_and_guarded(pkg):
    L = pkg._lib.lib()
    protos = pkg._lib.parse_header()
    assert "sgs_gine_aggregate_fwd_multi" in protos and hasattr(L, "sgs_gine_aggregate_fwd_multi")
    assert protos["sgs_gine_aggregate_fwd_multi"][2] == ["x", "x_stride", "edge_w", "a", "b", "diag", "N", "Dc", "nnz", "D", "in_ptr", "in_src",
                                                         "in_eid", "z", "stream"]
    assert L.sgs_abi_version() == 1
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    err = L.sgs_last_error

    def call(N=10, Dc=4, nnz=5, D=3, x_stride=0, x=p, a=p, b=p, ptr=p, src=p, eid=p, z=p):
        return L.sgs_gine_aggregate_fwd_multi(x, x_stride, None, a, b, 1.0, N, Dc, nnz, D, ptr, src, eid, z, None)

    for kw in (dict(N=-1), dict(Dc=0), dict(D=0), dict(D=65536), dict(nnz=-1), dict(x_stride=1), dict(x_stride=39), dict(x_stride=-40)):
        assert call(**kw) == -1 and err().startswith(b"sgs_gine_aggregate_fwd_multi") and b"bad sizes" in err(), kw
    assert call(N=0) == 0                                                            # nothing launched (no GPU here)
    assert call(N=0, x=None, a=None, b=None, ptr=None, src=None, eid=None, z=None) == 0
    for kw in (dict(x=None), dict(a=None), dict(b=None), dict(ptr=None), dict(z=None), dict(src=None), dict(eid=None),
               dict(x=None, a=None, b=None, ptr=None, src=None, eid=None, z=None)):
        assert call(**kw) == -1 and err().startswith(b"sgs_gine_aggregate_fwd_multi") and b"null" in err(), kw
    # x and z must not overlap: the shared block, and the last draw's block of a strided x
    assert call(z=p) == -1 and b"overlap" in err()
    assert call(z=p + 4 * 39) == -1 and b"overlap" in err()
    assert call(x_stride=40, z=p + 4 * 119) == -1 and b"overlap" in err()


# ------------------------------------------------------------------ the composition, in fp64
def _hand_draws():
    """Three draws over 7 nodes (edge lists [2, 6], one weight per drawn edge).  Draw 0: a self loop (2, 2), a duplicated edge (0 -> 1
    twice) and node 6 isolated; draw 1: node 0 with three in-edges; draw 2: every node but 3 isolated."""
    e0 = torch.tensor([[0, 0, 2, 3, 4, 5], [1, 1, 2, 4, 5, 3]])
    e1 = torch.tensor([[1, 2, 3, 0, 6, 5], [0, 0, 0, 6, 5, 4]])
    e2 = torch.tensor([[3, 3, 3, 3, 3, 3], [3, 3, 3, 3, 3, 3]])
    g = torch.Generator().manual_seed(11)
    return [e0, e1, e2], torch.rand(3, 6, generator=g, dtype=torch.float64) * 0.9 + 0.05


def _drawn_gine_logits_fp64(P, x, edges, w):
    """eval_batch._drawn_gine_logits, restated: per layer the aggregate of every draw (layer 1 over the shared x, layer 2 over the draw's own
    block of the stacked hidden rows), then the MLP's two Linears over the stacked [D N, .] rows, ReLU between the layers."""
    D, N = len(edges), x.shape[0]
    h = x
    for l in range(2):
        g = lambda k: P[f"GIN.convs.{l}.{k}"]
        blocks = [h if l == 0 else h.view(D, N, -1)[d] for d in range(D)]
        z = torch.stack([gine_ref.gine_aggregate(blocks[d], edges[d], None if w is None else w[d], g("lin.weight")[:, 0], g("lin.bias"), 1.0)
                         for d in range(D)])
        h = torch.relu(z.view(D * N, -1) @ g("nn.lins.0.weight").t() + g("nn.lins.0.bias"))
        h = h @ g("nn.lins.1.weight").t() + g("nn.lins.1.bias")
        if l == 0:
            h = torch.relu(h)
    return h.view(D, N, -1)


def test_the_engines_mathematics_is_the_models_in_fp64(pkg):
    torch.manual_seed(4)
    m = pkg.GINModel(9, 8, 4, gin_edge_weight=True)
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if n_.startswith("GIN."):
                p_.copy_(torch.randn(p_.shape) * 0.5)
    assert m.GIN.convs[0]._eps == 0.0 and m.GIN.convs[0].in_channels == 9 and m.GIN.convs[1].in_channels == 8
    P = {k: v.detach().double() for k, v in m.state_dict().items()}
    edges, w = _hand_draws()
    deg0 = torch.bincount(edges[0][1], minlength=7)
    assert int(deg0[6]) == 0 and int(deg0[1]) == 2 and bool((edges[0][0] == edges[0][1]).any())
    x = torch.randn(7, 9, dtype=torch.float64)
    for ww in (w, None):
        got = _drawn_gine_logits_fp64(P, x, edges, ww)
        assert got.shape == (3, 7, 4)
        for d in range(3):
            ref = gine_ref.gine_model(P, x, edges[d], None if ww is None else ww[d])
            assert float((got[d] - ref).abs().max()) <= 1e-10, d
        assert not torch.equal(got[0], got[1])
    assert not torch.allclose(_drawn_gine_logits_fp64(P, x, edges, w), _drawn_gine_logits_fp64(P, x, edges, None))


def test_ops_signatures(pkg):
    import inspect
    ops = pkg.ops
    assert list(inspect.signature(ops.gine_aggregate_multi).parameters) == ["x", "x_stride", "csr", "w", "a", "b", "diag", "q", "N", "Dc"]
    assert list(inspect.signature(pkg.eval_batch._drawn_gine_logits).parameters)[:4] == ["parent", "smp", "w", "convs"]
    prm = inspect.signature(_ev().plan_draws).parameters["gine_in"]
    assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default == 0
