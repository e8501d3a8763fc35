"""CPU: the batched engine of the GATv2 head (GATModel(gat_v2=True)) -- the routing opt-in `args.sgs_eval_batch_gatv2`, the planner's
`gat_v2` term, and the C entry point sgs_gatv2_alpha_heads_fwd_multi (declaration, export, every guard through the error channel).
Nothing here needs a GPU."""
import argparse
import ctypes
import inspect
import itertools

import pytest
import torch

from test_eval_batch_cover_cpu import OPTINS, _ABSENT, _Untouchable, _ev, _models


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _ns(base, **extra):
    return argparse.Namespace(**base, **{k: v for k, v in extra.items() if v is not _ABSENT})


def _v2_models(S):
    """GATv2 models: heads 1 and 8, with and without the edge term."""
    return {f"GATv2 K={K} edge={e}": S.GATModel(12, 16, 5, gat_heads=K, gat_edge_weight=e, gat_v2=True) for K in (1, 8) for e in (False, True)}


# ------------------------------------------------------------------ routing
def _v2_rule(kw, n_draws=11):
    """The issue's rule, restated: flag truthy, the new opt-in True, "GAT" among the selected heads, n_draws >= 1; under the cover flag
    also the cover opt-in True.  sgs_eval_batch_variants and sgs_eval_batch_gine play no part."""
    if not kw.get("sgs_eval_batch"):
        return False
    if kw.get("sgs_eval_batch_gatv2") is not True:
        return False
    heads = kw.get("sgs_eval_batch_heads")
    if not (heads == "all" or (isinstance(heads, (list, tuple, set)) and "GAT" in heads)):
        return False
    if n_draws < 1:
        return False
    return kw.get("sgs_cover_nodes") is not True or kw.get("sgs_eval_batch_cover") is True


COVER_PAIRS = ((_ABSENT, _ABSENT), (True, _ABSENT), (True, False), (True, True), (False, True))


def _bases():
    """Every combination of the opt-ins that existed before this one: the cover file's list, a GIN-only and a GAT-only selection, each
    with sgs_eval_batch_gine absent and True."""
    more = [dict(sgs_eval_batch=3, sgs_eval_batch_heads=["GIN"]), dict(sgs_eval_batch=3, sgs_eval_batch_heads=("GAT",))]
    for base in OPTINS + more:
        yield base
        yield dict(base, sgs_eval_batch_gine=True)


def test_truth_table(pkg):
    ev = _ev()
    models = {name: m for name, (m, _) in _models(pkg).items()}
    v2 = _v2_models(pkg)
    seen = {True: 0, False: 0}
    for base, (cover_flag, cover_optin) in itertools.product(_bases(), COVER_PAIRS):
        cov = dict(sgs_cover_nodes=cover_flag, sgs_eval_batch_cover=cover_optin)
        for name, m in models.items():
            absent = ev._batched_ok(_ns(base, **cov), m, 11)
            for val in (_ABSENT, None, False, True):
                a = _ns(base, **cov, sgs_eval_batch_gatv2=val)
                got = ev._batched_ok(a, m, 11)
                if name == "GATv2":
                    assert got is _v2_rule(vars(a)), (name, vars(a))
                else:
                    assert got is absent, (name, vars(a))                             # every non-v2 model: its value with the opt-in absent
            if name == "GATv2":
                assert absent is False, base                                          # without the opt-in: never, as before it existed
        for name, m in v2.items():
            for val in (_ABSENT, None, False, True):
                a = _ns(base, **cov, sgs_eval_batch_gatv2=val)
                got = ev._batched_ok(a, m, 11)
                assert got is _v2_rule(vars(a)), (name, vars(a))
                assert ev._batched_ok(a, m, 0) is False
                seen[got] += 1
    assert seen[True] > 0 and seen[False] > 0


def test_the_table_is_not_trivial(pkg):
    """Every v2 model reaches the engine with and without the cover pair, with and without the variants opt-in; with any single required
    opt-in removed it does not."""
    ev = _ev()
    plain = dict(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_gatv2=True)
    cover = dict(plain, sgs_cover_nodes=True, sgs_eval_batch_cover=True)
    for name, m in _v2_models(pkg).items():
        for full in (plain, cover, dict(plain, sgs_eval_batch=4), dict(plain, sgs_eval_batch_heads=("GAT",)),
                     dict(cover, sgs_eval_batch_variants=True), dict(plain, sgs_eval_batch_variants=False)):
            assert ev._batched_ok(argparse.Namespace(**full), m, 11) is True, (name, full)
            for k in full:
                if k in ("sgs_cover_nodes", "sgs_eval_batch_variants"):
                    continue                                                          # (not opt-ins of this head)
                fewer = {a: b for a, b in full.items() if a != k}
                assert ev._batched_ok(argparse.Namespace(**fewer), m, 11) is False, (name, fewer)
        assert ev._batched_ok(argparse.Namespace(**dict(plain, sgs_eval_batch_heads=["GIN", "Cheb", "GCN"])), m, 11) is False
        assert ev._batched_ok(argparse.Namespace(**plain), m, 0) is False
    # the v1 models do not need the new opt-in and are not disturbed by it
    models = _models(pkg)
    for v in (_ABSENT, None, False, True):
        a = _ns(dict(sgs_eval_batch=True, sgs_eval_batch_heads="all"), sgs_eval_batch_gatv2=v)
        assert ev._batched_ok(a, models["GAT"][0], 11) is True
        assert ev._batched_ok(a, models["GAT heads=8"][0], 11) is False


def test_invalid_values_raise_before_a_loader_is_touched(pkg):
    ev = _ev()
    models = dict({"GCN": _models(pkg)["GCN"][0]}, **_v2_models(pkg))
    for bad in (1, 0, "yes", [True], 1.0):
        for name in ("GCN", "GATv2 K=8 edge=True"):
            m = models[name]
            a = argparse.Namespace(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_gatv2=bad, device="cpu", num_samples_eval=3)
            with pytest.raises(ValueError, match="sgs_eval_batch_gatv2"):
                ev._batched_ok(a, m, 3)
            before = dict(ev.PATH_COUNTS)
            for mode in ("learned", "random", "edge", "full"):
                with pytest.raises(ValueError, match="sgs_eval_batch_gatv2"):
                    ev.ensemble_evaluate(a, m, _Untouchable(), "cpu", q=10, mode=mode)
            assert ev.PATH_COUNTS == before
            # consulted only when sgs_eval_batch is truthy, as the other opt-ins
            for off in (False, None, 0):
                assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=off, sgs_eval_batch_gatv2=bad), m, 3) is False
            assert ev._batched_ok(argparse.Namespace(sgs_eval_batch_gatv2=bad), m, 3) is False
            # under the cover flag without its opt-in nothing else is consulted (the routing from before the opt-ins existed)
            assert ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_cover_nodes=True, sgs_eval_batch_gatv2=bad), m, 3) is False
            with pytest.raises(ValueError, match="sgs_eval_batch_gatv2"):
                ev._batched_ok(argparse.Namespace(sgs_eval_batch=True, sgs_cover_nodes=True, sgs_eval_batch_cover=True, sgs_eval_batch_gatv2=bad),
                               m, 3)


# ------------------------------------------------------------------ the planner
SHAPES = [(4097, 2000, 900, 16, 5), (100_003, 20_000, 20_000, 64, 7), (463_000, 90_000, 33_869, 256, 40), (351_000, 70_200, 1_013, 256, 41)]
HEAD_KW = [("GCN", {}), ("GAT", {}), ("GIN", {}), ("Cheb", {}), ("GAT", dict(gat_heads=4, gat_edge=True)), ("GAT", dict(gat_heads=8)),
           ("GAT", dict(gat_edge=True, cover=True)), ("Cheb", dict(cheb_k=3)), ("GIN", dict(cover=True)), ("GIN", dict(gine_in=602))]
BUDGETS = [True, 1, 4, 100] + [("bytes", n) for n in (1, 1 << 20, 8 << 20, 64 << 20, 1 << 30)]


def _base(E, q, N, H, C):
    return 4 * ((E + 63) & ~63) + 5 * E + 40 * q + 36 * (N + 1) + 4 * N * H + 8 * N * C + 3 * 2048 * 4 + 64


def _per_today(E, q, N, H, C, head, gat_heads=1, gat_edge=False, cheb_k=1, cover=False, gine_in=0):
    """A frozen copy of plan_draws' per-draw bytes from before the gat_v2 keyword."""
    per = _base(E, q, N, H, C)
    if head == "GAT":
        per += 4 * q * gat_heads + 12 * N * gat_heads + 4 * N * C * (gat_heads - 1) + (8 * N if gat_edge else 0)
    elif head == "GIN" and gine_in:
        per += 4 * N * gine_in + 8 * N * H
    elif head == "GIN":
        per += 4 * N * H + 8 * N * C + 4 * q + 4 * N
    elif head == "Cheb" and cheb_k > 1:
        per += 4 * N * (cheb_k - 1) * (H + C) + 4 * q + 4 * N + 4 * E
    return per + (4 * 1024 + 8 if cover else 0)


def _v2_allocations(q, N, C, K):
    """What eval_batch._drawn_gatv2_logits allocates per draw beside the hidden block, the logits and the drawn edge's weight, as plan_draws'
    docstring lists it: attention values [q, K], loop attentions [N, K], the layer-2 product [N, 2 K C], its halves x_l, x_r [N, K C]."""
    return 4 * q * K + 4 * N * K + 4 * N * 2 * K * C + 2 * 4 * N * K * C


def _split(D, k):
    k = max(1, min(D, k))
    return [k] * (D // k) + ([D % k] if D % k else [])


def test_plan_draws_default_is_todays_list(pkg):
    ev = _ev()
    for (E, q, N, H, C), (head, kw), D, budget in itertools.product(SHAPES, HEAD_KW, (1, 3, 11, 64), BUDGETS):
        got = ev.plan_draws(E, q, N, H, C, D, budget, head=head, gat_v2=False, **kw)
        assert got == ev.plan_draws(E, q, N, H, C, D, budget, head=head, **kw)
        if budget is True or isinstance(budget, tuple):
            nbytes = ev.EVAL_BATCH_BUDGET if budget is True else budget[1]
            assert got == _split(D, nbytes // _per_today(E, q, N, H, C, head, **kw)), (head, kw, budget)
        else:
            assert got == _split(D, budget)


def test_plan_draws_gatv2_term(pkg):
    ev = _ev()
    for (E, q, N, H, C), K, edge, cover, D, budget in itertools.product(SHAPES, (1, 4, 8, 16), (False, True), (False, True), (1, 11, 64), BUDGETS):
        kw = dict(head="GAT", gat_heads=K, gat_edge=edge, cover=cover)
        v2 = ev.plan_draws(E, q, N, H, C, D, budget, gat_v2=True, **kw)
        v1 = ev.plan_draws(E, q, N, H, C, D, budget, **kw)
        assert sum(v2) == D and min(v2) >= 1
        assert max(v2) <= max(v1), (kw, budget)                                       # never a larger pass than the v1 term's
        if budget is True or isinstance(budget, tuple):
            nbytes = ev.EVAL_BATCH_BUDGET if budget is True else budget[1]
            floor = _base(E, q, N, H, C) + _v2_allocations(q, N, C, K) + (4 * 1024 + 8 if cover else 0)
            assert max(v2) <= max(1, nbytes // floor), (kw, budget)                   # per-draw bytes >= the listed allocations
        else:
            assert v2 == _split(D, budget)                                            # "at most k": no byte model
    # the term is the documented one, to the byte
    E, q, N, H, C = SHAPES[0]
    per = _base(E, q, N, H, C) + _v2_allocations(q, N, C, 8)
    assert per == _base(E, q, N, H, C) + 4 * q * 8 + 4 * N * 8 + 16 * N * 8 * C
    assert ev.plan_draws(E, q, N, H, C, 11, ("bytes", 11 * per), head="GAT", gat_heads=8, gat_v2=True) == [11]
    assert ev.plan_draws(E, q, N, H, C, 11, ("bytes", 11 * per - 1), head="GAT", gat_heads=8, gat_v2=True) == [10, 1]
    assert ev.plan_draws(E, q, N, H, C, 11, ("bytes", 11 * per), head="GAT", gat_heads=8, gat_v2=True, gat_edge=True) == [11]   # eval: no loop weights
    assert ev.plan_draws(E, q, N, H, C, 11, ("bytes", 11 * per), head="GAT", gat_heads=8, gat_v2=True, cover=True) == [10, 1]
    for head in ("GCN", "GIN", "Cheb"):
        with pytest.raises(ValueError, match="gat_v2"):
            ev.plan_draws(E, q, N, H, C, 11, True, head=head, gat_v2=True)
    with pytest.raises(ValueError, match="gat_v2"):
        ev.plan_draws(E, q, N, H, C, 11, True, head="GAT", gat_v2=1)
    with pytest.raises(TypeError):
        ev.plan_draws(E, q, N, H, C, 11, True, "GAT", 1, False, 1, False, 0, True)   # keyword-only
    prm = inspect.signature(ev.plan_draws).parameters["gat_v2"]
    assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is False


# ------------------------------------------------------------------ header and library
def test_the_entry_point_is_declared_exported_and_guarded(pkg):
    L = pkg._lib.lib()
    protos = pkg._lib.parse_header()
    name = "sgs_gatv2_alpha_heads_fwd_multi"
    assert name in protos and hasattr(L, name)
    assert protos[name][2] == ["xl", "xr", "x_stride", "att", "edge_w", "lin_edge", "N", "K", "C", "D", "nnz", "in_ptr", "in_src", "in_eid",
                               "negative_slope", "alpha", "alpha_loop", "stream"]
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    err = L.sgs_last_error

    def call(N=10, K=2, C=4, D=3, nnz=5, x_stride=0, xl=p, xr=p, att=p, w=None, le=None, ptr=p, src=p, eid=p, alpha=p, loop=p):
        return L.sgs_gatv2_alpha_heads_fwd_multi(xl, xr, x_stride, att, w, le, N, K, C, D, nnz, ptr, src, eid, 0.2, alpha, loop, None)

    for kw in (dict(N=-1), dict(nnz=-1), dict(D=0), dict(D=65536), dict(N=1 << 31), dict(nnz=1 << 31)):
        assert call(**kw) == -1 and err().startswith(name.encode()) and b"bad sizes" in err(), kw
    for kw in (dict(K=0), dict(K=17), dict(C=0)):
        assert call(**kw) == -1 and err().startswith(name.encode()) and b"heads" in err(), kw
    for s in (1, 79, 81, 84, 160, -80, 40):                                          # N K C = 80: 0 and 80 only, a padded stride included
        assert call(x_stride=s) == -1 and err().startswith(name.encode()) and b"x_stride" in err(), s
    assert call(w=p) == -1 and b"edge_w needs lin_edge" in err()
    assert call(N=0) == 0                                                            # nothing launched (no GPU here)
    assert call(N=0, xl=None, xr=None, att=None, ptr=None, src=None, eid=None, alpha=None, loop=None) == 0
    for kw in (dict(xl=None), dict(xr=None), dict(att=None), dict(ptr=None), dict(loop=None), dict(src=None), dict(eid=None), dict(alpha=None)):
        assert call(**kw) == -1 and err().startswith(name.encode()) and b"null" in err(), kw
        assert call(x_stride=80, **kw) == -1 and b"null" in err(), kw


def test_ops_signatures(pkg):
    ops = pkg.ops
    assert list(inspect.signature(ops.gatv2_alpha_heads_multi).parameters) == ["xl", "xr", "x_stride", "att", "csr", "q", "N", "K", "negative_slope",
                                                                               "edge_w", "lin_edge", "out"]
    assert list(inspect.signature(pkg.eval_batch._drawn_gatv2_logits).parameters) == ["parent", "smp", "convs", "xl1", "xr1", "w"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gatv2_alpha_heads_multi(torch.zeros(4, 8), torch.zeros(4, 8), 0, torch.zeros(8), (torch.zeros(1, 5, dtype=torch.int32),) * 3, 0, 4, 2, 0.2)
