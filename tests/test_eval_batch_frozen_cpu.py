"""CPU: the engine table of eval_batch.py routes and plans exactly as the code it replaced (tests/eval_routing_ref.py, a frozen copy),
over full products of models, flags and shapes; the pass-splitting function; the table itself; the import layering.  Nothing here needs a
GPU."""
import argparse
import itertools
import os
import re
import subprocess
import sys

import pytest
import torch

import eval_routing_ref as REF
from test_eval_batch_cover_cpu import _ABSENT, _ev, _models
from test_eval_batch_gatv2_cpu import BUDGETS, HEAD_KW, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd


def _ten_models(S):
    ms = {name: m for name, (m, _) in _models(S).items()}
    ms["GATv2 heads=8 edge"] = S.GATModel(12, 16, 5, gat_heads=8, gat_v2=True, gat_edge_weight=True)
    assert len(ms) == 10
    return ms


def _outcome(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except Exception as e:                     # compared too: the same type with the same message
        return type(e), str(e)


# ------------------------------------------------------------------ routing
FLAG = (_ABSENT, False, 0, True, 4, -1, "4")
HEADSEL = (_ABSENT, None, "all", ["GAT", "Cheb"], "GATX")
BOOL = (_ABSENT, False, True, 1)           # (None, the fifth value, makes the product 2 million calls; the per-flag truth tables cover it)
COVER = (_ABSENT, False, True)


def test_routing_equals_the_frozen_copy_over_the_full_product(pkg):
    ev = _ev()
    models = list(_ten_models(pkg).values())
    seen = {True: 0, False: 0, "raised": 0}
    for flag, heads, var, cov, gine, v2, cover in itertools.product(FLAG, HEADSEL, BOOL, BOOL, BOOL, BOOL, COVER):
        kw = dict(sgs_eval_batch=flag, sgs_eval_batch_heads=heads, sgs_eval_batch_variants=var, sgs_eval_batch_cover=cov,
                  sgs_eval_batch_gine=gine, sgs_eval_batch_gatv2=v2, sgs_cover_nodes=cover)
        a = argparse.Namespace(**{k: v for k, v in kw.items() if v is not _ABSENT})
        for m in models:
            for n_draws in (0, 1, 11):
                want = _outcome(REF._batched_ok, a, m, n_draws)
                got = _outcome(ev._batched_ok, a, m, n_draws)
                assert type(got) is type(want) and got == want, (vars(a), type(m).__name__, n_draws, got, want)
                seen[want if isinstance(want, bool) else "raised"] += 1
    assert min(seen.values()) > 0, seen


# ------------------------------------------------------------------ the planner
V2_KW = [("GAT", dict(gat_v2=True)), ("GAT", dict(gat_v2=True, gat_heads=8, gat_edge=True)), ("GAT", dict(gat_v2=True, gat_heads=4, cover=True))]
ODD_KW = [("GCN", dict(gat_v2=True)), ("GAT", dict(gat_v2=1)), ("GAT", dict(gine_in=5)), ("GIN", dict(gine_in=-1)), ("SAGE", {}),
          ("GAT", dict(gat_heads=17)), ("Cheb", dict(cheb_k=9)), ("GAT", dict(cheb_k=3)), ("Cheb", dict(gat_heads=8, gat_edge=True))]


def test_planner_equals_the_frozen_copy(pkg):
    ev = _ev()
    raised = 0
    for (E, q, N, H, C), (head, kw), D, budget in itertools.product(SHAPES, HEAD_KW + V2_KW + ODD_KW, (0, 1, 3, 11, 64),
                                                                    BUDGETS + [0, -1, ("bytes", 0)]):
        want = _outcome(REF.plan_draws, E, q, N, H, C, D, budget, head=head, **kw)
        got = _outcome(ev.plan_draws, E, q, N, H, C, D, budget, head=head, **kw)
        assert type(got) is type(want) and got == want, (E, q, N, H, C, head, kw, D, budget, got, want)
        raised += isinstance(want, tuple)
    assert raised > 0
    assert ev.plan_draws(*SHAPES[0], 11, True) == REF.plan_draws(*SHAPES[0], 11, True)             # the default head


# ------------------------------------------------------------------ pass splitting
def _givens(D):
    t = lambda d: torch.full((6,), float(d), dtype=torch.float64)      # (converted to float32; its value names the draw)
    return {"clock": [None] * D, "explicit": [t(d) for d in range(D)], "alternating": [t(d) if d % 2 == 0 else None for d in range(D)],
            "explicit 0-4, then clock": [t(d) if d < 5 else None for d in range(D)]}


@pytest.mark.parametrize("plan", [[4, 4, 3], [11], [1] * 11])
def test_split_passes(pkg, plan):
    D, seed, tick = sum(plan), 1234, 77
    for name, given in _givens(D).items():
        snapshot = list(given)
        passes, used = pkg.eval_batch.split_passes(plan, given, seed, tick)
        assert len(given) == D and all(a is b for a, b in zip(given, snapshot))      # its arguments are left as they were
        assert sum(n for n, *_ in passes) == D, name
        assert used == sum(g is None for g in given), name
        d = clock_before = 0
        bounds = list(itertools.accumulate(plan))                                    # a pass lies within one plan entry
        for n, noise, s, sid0 in passes:
            entry = next(i for i, b in enumerate(bounds) if d < b)
            assert n >= 1 and d + n <= bounds[entry], (name, d, n)
            kinds = {g is None for g in given[d:d + n]}
            assert len(kinds) == 1, (name, d, n)                                     # never both kinds in one pass
            if kinds == {True}:
                assert noise is None and (s, sid0) == (seed, tick + 1 + clock_before), (name, d)
                clock_before += n
            else:
                assert (s, sid0) == (0, 0) and noise.dtype == torch.float32 and noise.is_contiguous() and tuple(noise.shape) == (n, 6)
                assert noise[:, 0].tolist() == [float(k) for k in range(d, d + n)], (name, d)    # draws keep their order
            d += n
        assert d == D


# ------------------------------------------------------------------ the table
EXPECT = {"GCN": ("GCN", "GCN", 1), "GAT": ("GAT, one head", "GAT", 1), "GIN": ("GIN", "GIN", 0), "Cheb": ("Chebyshev K = 1", "Cheb", 0),
          "GAT heads=8": ("GAT, per-head kernels", "GAT", 1), "GAT edge": ("GAT, per-head kernels", "GAT", 1),
          "Cheb K=3": ("Chebyshev K >= 2", "Cheb", 0), "GATv2": ("GATv2", "GAT", 1), "GINE": ("GINE", "GIN", 0),
          "GATv2 heads=8 edge": ("GATv2", "GAT", 1)}


def test_every_model_has_exactly_one_row(pkg):
    ev, eb = _ev(), pkg.eval_batch
    assert len(eb.ENGINES) == 8 and len({e.name for e in eb.ENGINES}) == 8
    assert {e.head for e in eb.ENGINES} == set(ev.HEADS) and {e.optin for e in eb.ENGINES} <= {None, *eb.OPTINS}
    for name, m in _ten_models(pkg).items():
        rows = [e for e in eb.ENGINES if e.serves(m)]
        assert len(rows) == 1, name
        assert (rows[0].name, rows[0].head, rows[0].ticks) == EXPECT[name], name
        assert eb.engine_of(m) is rows[0]
        assert ev._head_of(m) == EXPECT[name][1]
        assert ev._head_dims(m, ev._head_of(m)) == (16, 5), name                     # hidden 16 (heads x 16 // heads for GAT), 5 classes
    wide = pkg.GATModel(12, 48, 7, gat_heads=8)
    assert ev._head_dims(wide, "GAT") == (48, 7) and ev._head_dims(pkg.GINModel(12, 32, 3), "GIN") == (32, 3)
    assert ev._head_dims(pkg.ChebModel(12, 24, 4, cheb_k=2), "Cheb") == (24, 4) and ev._head_dims(pkg.GNNModel(12, 8, 2), "GCN") == (8, 2)
    for other in (torch.nn.Linear(3, 3), torch.nn.ReLU(), object()):
        assert not any(e.serves(other) for e in eb.ENGINES) and eb.engine_of(other) is None and ev._head_of(other) is None
        with pytest.raises(TypeError, match="no batched engine"):
            eb.ensemble_partition_head(None, other, 10, 0, None, [], None)


# ------------------------------------------------------------------ layering
def test_ops_does_not_import_the_models_and_eval_batch_imports_first():
    src = open(os.path.join(ROOT, "sgs-gnn_amd", "ops.py")).read()
    assert not re.search(r"^\s*from\s+\.model\s+import|^\s*from\s+\.\s+import\s+.*\bmodel\b|^\s*import\s+.*\bmodel\b", src, re.M)
    assert "ensemble_partition" not in src and "_drawn_" not in src                  # no alias left behind
    r = subprocess.run([sys.executable, "-c", "import sgs_gnn_amd.eval_batch"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
