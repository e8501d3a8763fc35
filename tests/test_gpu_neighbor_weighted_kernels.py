"""GPU: sgs_nbr_select_weighted through the C ABI, outputs and the exactly sized workspace between red zones, against
tests/neighbor_weighted_ref.py by exact equality.  Case table: neighbor_ref.kernel_case (in-rows of 0, 1, f - 1, f, f + 1, 63, 64, 65, 255, 256,
257, hub and hub + 1 entries, N = 131), every fan-out of FANOUTS, frontiers of 0, 1, 3 and N rows, and five weight patterns: uniform random,
all equal, 70 % zeros, whole rows zero (the hub rows among them) and only {1, 2^24 - 1}."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ref as R  # noqa: E402
import neighbor_weighted_ref as W  # noqa: E402
from zoned import DEV, Zoned  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = -77777


@pytest.fixture(scope="module")
def lib():
    import sgs_gnn_amd as S
    return S._lib.lib()


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _select(lib, g, wq, rows, f, K, cap=None):
    """one call between red zones, compared with the reference; the inputs must come back untouched"""
    want_offs, want = W.select(g.in_ptr, g.in_eid, wq, g.N, rows, f, K)
    total = int(want_offs[-1])
    cap = total if cap is None else cap
    host = [g.in_ptr, g.in_eid, wq, np.asarray(rows, dtype=np.int32)]
    d = [_dev(a) for a in host]
    chosen, tot = Zoned(cap, torch.int32, FILL), Zoned(1, torch.int64, FILL)
    nbytes = lib.sgs_nbr_select_workspace_bytes(len(rows))
    assert nbytes % 8 == 0
    ws = Zoned(nbytes // 8, torch.int64, FILL)
    rc = lib.sgs_nbr_select_weighted(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), g.N, g.E, d[3].data_ptr(), len(rows), f, K, chosen.ptr, cap,
                                     tot.ptr, ws.ptr, nbytes, None)
    assert rc == 0, lib.sgs_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(ws.get()[:len(rows) + 1], want_offs) and int(tot.get()[0]) == total
    got = chosen.get().copy()                                               # (get() checks both red zones: nothing at or beyond cap)
    assert np.array_equal(got, want[:cap])
    for a, b in zip(host, d):
        assert np.array_equal(a, b.cpu().numpy())
    return got


@pytest.fixture(scope="module")
def cases(lib):
    hub = lib.sgs_nbr_select_hub_row()
    cache = {}

    def get(f):
        if f not in cache:
            ei, N = R.kernel_case(f, hub, seed=abs(f))
            g = R.Graph(ei, N)
            deg = np.diff(g.in_ptr)
            ff = f if f > 0 else 7
            assert N % 4 == 3 and set(R.ROW_LENGTHS + (max(ff - 1, 0), ff, ff + 1, hub, hub + 1)) <= set(deg.tolist())
            cache[f] = (g, [int(np.nonzero(deg == hub)[0][0]), int(np.nonzero(deg == hub + 1)[0][0])])
        return cache[f]
    return get


@pytest.mark.parametrize("pattern", W.WEIGHT_PATTERNS)
@pytest.mark.parametrize("f", R.FANOUTS)
def test_kernel_case_table(lib, cases, f, pattern):
    g, hubs = cases(f)
    wq = W.weight_pattern(pattern, g, seed=abs(f) + 11, zero_rows=hubs)
    if pattern == "zero_rows":
        assert all(not wq[g.in_ptr[v]:g.in_ptr[v + 1]].any() for v in hubs)
    K = R.stream_key(3, 1, 4, 1)
    differs = False
    for rows in R.kernel_frontiers(g.N, seed=f + 5):
        first = _select(lib, g, wq, rows, f, K)
        assert np.array_equal(_select(lib, g, wq, rows, f, K), first)        # the same bits on a second call
        differs |= not np.array_equal(first, R.select(g.in_ptr, g.in_eid, g.N, rows, f, K)[1])
    assert differs == (f > 0)                                                # another key, another draw wherever a row is cut


def test_hub_rows_and_ties_in_the_workgroup_form(lib, cases):
    """rows of hub and hub + 1 entries side by side in one tile, fan-outs below, at and above the hub length; weights of two values and 70 %
    zeros make the threshold key a tie (the zero weights share one key) in both row forms"""
    hub = lib.sgs_nbr_select_hub_row()
    g, (a, b) = cases(25)
    deg = np.diff(g.in_ptr)
    small = int(np.nonzero(deg == 65)[0][0])
    for pattern in ("mostly_zero", "two_values", "zero_rows"):
        wq = W.weight_pattern(pattern, g, seed=4, zero_rows=[b])
        for f in (1, 25, 300, hub - 1, hub, hub + 1, hub + 2):
            for rows in ([b], [a, b, small, b], [small, b, a]):
                got = _select(lib, g, wq, rows, f, 0xDEADBEEF)
                assert got.shape[0] == sum(min(f, int(deg[r])) for r in rows)
    # the zeros of a row are taken only after its positive weights, first come first
    wq = W.weight_pattern("mostly_zero", g, seed=4)
    for v in (a, b, small):
        lo, hi = int(g.in_ptr[v]), int(g.in_ptr[v + 1])
        pos = int((wq[lo:hi] > 0).sum())
        got = _select(lib, g, wq, [v], pos + 5, 77)
        zeros = g.in_eid[lo:hi][wq[lo:hi] == 0]
        assert np.array_equal(np.sort(got), np.sort(np.concatenate([g.in_eid[lo:hi][wq[lo:hi] > 0], zeros[:5]])))


def test_caps_bound_every_write(lib, cases):
    g, _ = cases(25)
    wq = W.weight_pattern("random", g, seed=1)
    rows = np.arange(g.N, dtype=np.int32)
    for cap in (0, 1, 100):
        _select(lib, g, wq, rows, 25, 5, cap=cap)


def test_argument_errors(lib, cases):
    g, _ = cases(2)
    d = [_dev(g.in_ptr), _dev(g.in_eid), _dev(W.weight_pattern("random", g, 0)), _dev(np.arange(4))]
    buf = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()
    names = (("ptr", d[0].data_ptr()), ("eid", d[1].data_ptr()), ("wq", d[2].data_ptr()), ("N", g.N), ("nnz", g.E), ("rows", d[3].data_ptr()),
             ("n_rows", 4), ("f", 2), ("key", 1), ("chosen", p), ("cap", 8), ("total", None), ("ws", p + 1024), ("ws_bytes", 1024), ("stream", None))
    sel = lambda **kw: lib.sgs_nbr_select_weighted(*[kw.get(k, v) for k, v in names])  # noqa: E731
    assert sel() == 0
    for kw, msg in ((dict(wq=None), b"null"), (dict(f=0), b"fanout"), (dict(f=-2), b"fanout"), (dict(N=0), b"bad sizes"), (dict(nnz=-1), b"bad sizes"),
                    (dict(n_rows=-1), b"n_rows"), (dict(ptr=None), b"null"), (dict(chosen=None), b"null"), (dict(ws=p + 1028), b"aligned")):
        assert sel(**kw) == -1 and msg in lib.sgs_last_error() and b"sgs_nbr_select_weighted" in lib.sgs_last_error(), kw
    assert sel(ws_bytes=8) == -2
    torch.cuda.synchronize()


def test_ops_wrapper_dispatches_on_the_weights(cases):
    import sgs_gnn_amd as S
    g, _ = cases(25)
    wq = W.weight_pattern("random", g, seed=2)
    rows = np.arange(g.N, dtype=np.int32)
    K = R.stream_key(1, 2, 3, 4)
    d = [_dev(g.in_ptr), _dev(g.in_eid), _dev(rows), _dev(wq)]
    offs, want = W.select(g.in_ptr, g.in_eid, wq, g.N, rows, 25, K)
    got = S.ops.nbr_select(d[0], d[1], g.N, d[2], 25, K, int(offs[-1]), wq=d[3])
    assert np.array_equal(got.cpu().numpy(), want)
    plain = S.ops.nbr_select(d[0], d[1], g.N, d[2], 25, K, int(offs[-1]))
    assert np.array_equal(plain.cpu().numpy(), R.select(g.in_ptr, g.in_eid, g.N, rows, 25, K)[1])
    with pytest.raises(ValueError, match="weights for"):
        S.ops.nbr_select(d[0], d[1], g.N, d[2], 25, K, int(offs[-1]), wq=d[3][:-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.nbr_select(d[0], d[1], g.N, d[2], 25, K, int(offs[-1]), wq=d[3].cpu())
