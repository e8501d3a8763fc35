"""CPU: the host half of the edge scorer's C entry points -- what the size functions return and what every entry point answers to
arguments it must reject (or accept as empty) before it launches anything.  The expected answers, return code and full sgs_last_error()
text, were recorded from the library BEFORE the launchers were given one args builder / workspace layout / dispatcher
(tests/golden/gen_scorer_entry_table.py -> tests/golden/scorer_entry_table.json), so they pin order and wording of every check."""
import importlib.util
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_scorer_entry_table", os.path.join(GOLDEN, "gen_scorer_entry_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()


@pytest.fixture(scope="module")
def L():
    import sgs_gnn_amd
    return sgs_gnn_amd._lib.lib()


@pytest.fixture(scope="module")
def table():
    with open(GEN.TABLE) as f:
        return json.load(f)


def r(nbytes):
    return (max(nbytes, 0) + 255) // 256 * 256


def test_workspace_bytes_formula(L):
    for N, H, E in itertools.product((-1, 0, 1, 300), (-4, 0, 4, 100, 128, 256, 512), (-1, 0, 1, 1000)):
        n, h, e = max(N, 0), max(H, 0), max(E, 0)
        want = r(4 * h * h) + r(4 * n * h) + r(8 * e) + 256 + r(8 * h * h) + 256
        assert L.sgs_edge_score_workspace_bytes(N, H, E) == want, (N, H, E)


def test_epd_workspace_bytes_formula(L):
    for H in (-4, 0, 4, 16, 100, 128, 256, 320, 1024):
        h = max(H, 0)
        assert L.sgs_edge_score_epd_workspace_bytes(H) == r(8 * h * h) + 256, H


def test_fused_opart_rows_formula(L):
    for n, N in itertools.product((-1, 0, 1, 31, 32, 33, 700), (-1, 0, 1, 300)):
        assert L.sgs_edge_score_bwd_fused_opart_rows(n, N) == (max(n, 0) + 31) // 32 + max(N, 0), (n, N)


def test_table_covers_the_cases(table):
    assert sorted(table) == sorted(cid for cid, _, _, _ in GEN.cases())
    assert all(rc != GEN.SGS_EHIP for rc, _ in table.values())          # nothing recorded got as far as the HIP runtime


@pytest.mark.parametrize("fn", sorted(GEN.SPEC))
def test_entry_point_validation(L, table, fn):
    import sgs_gnn_amd
    protos = sgs_gnn_amd._lib.parse_header()
    mine = [(cid, a) for cid, f, a, _ in GEN.cases() if f == fn]
    assert mine
    for cid, a in mine:
        assert GEN.run_case(L, protos, fn, a) == table[cid], cid
