"""GPU: sgs_consensus_accum, sgs_consensus_select and sgs_edge_class_counts through the C ABI against tests/consensus_ref.py, by exact
equality (integers, bits, edge sets).  Every output sits between red zones that must stay untouched.  Shapes (consensus_ref's tables): both
sides of the 16-byte tile, more than one workgroup, aligned and unaligned mask rows and bases, the fused small-E path and one size just
above its limit for the large-E path, both forms of the class-pair kernel on both sides of the LDS limit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consensus_ref as R  # noqa: E402
from zoned import DEV, Zoned  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import sgs_gnn_amd as S
    return S._lib.lib(), S.ops._stream


def _dev_bytes(buf, shift):
    """The mask buffer on the device, its first byte `shift` bytes past a 16-byte boundary."""
    t = torch.full((buf.size + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 16 == 0
    t[shift:shift + buf.size].copy_(torch.from_numpy(buf).to(DEV))
    return t, t.data_ptr() + shift


# ------------------------------------------------------------------ sgs_consensus_accum
@pytest.mark.parametrize("E", R.ACCUM_E)
def test_consensus_accum_exact(lib, E):
    L, stream = lib
    for Dc in R.ACCUM_DC:
        for pad in R.ACCUM_PAD:
            buf, rows = R.make_masks(E, Dc, pad, 31 * E + Dc + pad)
            shift = 0 if pad == 0 else 5                                        # unaligned rows AND an unaligned base
            keep, mptr = _dev_bytes(buf, shift)
            stride = E + pad
            base = np.arange(128, dtype=np.int64) * 1000003 + (1 << 33)
            want, want_h = R.accum_ref(rows, hist=base.copy())
            # one pass
            cnt = Zoned(E, torch.int32, -7777, shift=0 if pad == 0 else 1)
            hist = Zoned(128, torch.int64, -5)
            hist.set(base)
            assert L.sgs_consensus_accum(mptr, stride, Dc, E, 1, cnt.ptr if E else None, hist.ptr, stream()) == 0, L.sgs_last_error()
            assert np.array_equal(cnt.get(), want), (E, Dc, pad)
            assert np.array_equal(hist.get(), want_h if E else base), (E, Dc, pad)          # accumulated, not cleared
            if E:
                assert int((want_h - base).sum()) == E
                assert int(want.max()) <= Dc                                    # bytes of value 2 and 255 count once
            # two passes (first, then accumulate; the histogram only on the second) against the one
            if Dc >= 2 and E:
                k = Dc // 3 + 1
                cnt2 = Zoned(E, torch.int32, -7777, shift=0 if pad == 0 else 1)
                hist2 = Zoned(128, torch.int64, -5)
                hist2.set(base)
                assert L.sgs_consensus_accum(mptr, stride, k, E, 1, cnt2.ptr, None, stream()) == 0
                assert np.array_equal(cnt2.get(), R.accum_ref(rows[:k])[0])
                assert L.sgs_consensus_accum(mptr + k * stride, stride, Dc - k, E, 0, cnt2.ptr, hist2.ptr, stream()) == 0
                assert np.array_equal(cnt2.get(), want) and np.array_equal(hist2.get(), want_h), (E, Dc, pad)
            del keep


def test_consensus_accum_no_draws_and_validation(lib):
    L, stream = lib
    E = 4097
    cnt = Zoned(E, torch.int32, -7777)
    hist = Zoned(128, torch.int64, 0)
    assert L.sgs_consensus_accum(None, E, 0, E, 1, cnt.ptr, hist.ptr, stream()) == 0          # Dc = 0 with first: the counts are zeroed
    assert not cnt.get().any() and int(hist.get()[0]) == E and int(hist.get().sum()) == E
    cnt.set(np.full(E, 3, dtype=np.int32))
    assert L.sgs_consensus_accum(None, E, 0, E, 0, cnt.ptr, None, stream()) == 0               # Dc = 0 without: untouched
    assert bool((cnt.get() == 3).all())
    assert L.sgs_consensus_accum(None, E, 128, E, 1, cnt.ptr, None, stream()) == -1 and b"Dc=128" in L.sgs_last_error()
    assert bool((cnt.get() == 3).all())


# ------------------------------------------------------------------ sgs_consensus_select
def _select_case(L, stream, E, q, count, p, tag):
    g = np.random.default_rng(E + q)
    ei = g.integers(0, 1 << 40, size=(2, E), dtype=np.int64)
    want = R.select_ref(count, p, q, ei)
    d_count = torch.from_numpy(count).to(DEV)
    d_p = torch.from_numpy(p).to(DEV) if p is not None else None
    d_ei = torch.from_numpy(ei).to(DEV)
    mask = Zoned(E, torch.uint8, 0xAB)
    eid = Zoned(q, torch.int64, -9)
    eo = Zoned(2 * q, torch.int64, -9)
    co = Zoned(q, torch.int32, -9)
    po = Zoned(q, torch.float32, -9.0)
    ko = Zoned(E, torch.int32, -9)
    nb = L.sgs_consensus_select_workspace_bytes(E)
    ws = torch.full((nb + 512,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = L.sgs_consensus_select(d_count.data_ptr() if E else None, d_p.data_ptr() if d_p is not None and E else None, E, q,
                                d_ei.data_ptr() if E else None, mask.ptr if E else None, eid.ptr, eo.ptr, co.ptr, po.ptr, ko.ptr,
                                ws.data_ptr(), nb, stream())
    assert rc == 0, L.sgs_last_error()
    torch.cuda.synchronize()
    assert bool((ws[nb:] == 0xFF).all()), "the workspace was overrun"
    assert np.array_equal(ko.get().view(np.uint32), want["keys"]), tag
    assert np.array_equal(mask.get(), want["mask"]), tag
    assert np.array_equal(eid.get(), want["eid"]), tag
    assert np.array_equal(eo.get().reshape(2, q), want["edge_index"]), tag
    assert np.array_equal(co.get(), want["count"]), tag
    assert np.array_equal(po.get().view(np.uint32), want["p"].view(np.uint32)), tag          # bits: the NaN score too
    return want


@pytest.mark.parametrize("E", R.SELECT_E)
def test_consensus_select_exact(lib, E):
    L, stream = lib
    D = 11
    for with_p in (True, False):
        count, p = R.make_counts_scores(E, D, 17 * E + with_p, with_p)
        if E >= 16 and with_p:
            assert np.isnan(p[3]) and p[7] < 0
        for q in R.select_qs(E):
            want = _select_case(L, stream, E, q, count, p, (E, q, with_p))
            assert int(want["mask"].sum()) == q
    if E >= 16:                                                                  # counts outside [0, 127] are clamped, never an index
        count, p = R.make_counts_scores(E, D, 5 * E)
        count[0], count[1] = -5, 100000
        _select_case(L, stream, E, E // 5, count, p, (E, "clamped"))


def test_consensus_select_large_path(lib):
    L, stream = lib
    E = R.SELECT_LARGE_E
    count, p = R.make_counts_scores(E, 11, 99)
    _select_case(L, stream, E, E // 5, count, p, "large path")


def test_consensus_select_optional_outputs_and_refusal(lib):
    L, stream = lib
    E, q = 4097, 800
    count, p = R.make_counts_scores(E, 11, 3)
    want = R.select_ref(count, p, q)
    d_count, d_p = torch.from_numpy(count).to(DEV), torch.from_numpy(p).to(DEV)
    nb = L.sgs_consensus_select_workspace_bytes(E)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    mask = Zoned(E, torch.uint8, 0xAB)
    co = Zoned(q, torch.int32, -9)
    assert L.sgs_consensus_select(d_count.data_ptr(), d_p.data_ptr(), E, q, None, mask.ptr, None, None, co.ptr, None, None, ws.data_ptr(), nb,
                                  stream()) == 0                                 # count_out without eid: ids from the workspace
    assert np.array_equal(mask.get(), want["mask"]) and np.array_equal(co.get(), want["count"])
    assert L.sgs_consensus_select(d_count.data_ptr(), d_p.data_ptr(), E, E + 1, None, mask.ptr, None, None, None, None, None, ws.data_ptr(), nb,
                                  stream()) == -1 and b"without replacement" in L.sgs_last_error()
    assert L.sgs_consensus_select(d_count.data_ptr(), d_p.data_ptr(), E, q, None, mask.ptr, None, None, None, None, None, ws.data_ptr(), nb - 256,
                                  stream()) == -2 and b"workspace too small" in L.sgs_last_error()
    assert np.array_equal(mask.get(), want["mask"])                              # refused calls wrote nothing


# ------------------------------------------------------------------ sgs_edge_class_counts
@pytest.mark.parametrize("form,C", [(2, c) for c in R.PAIR_PRIVATE_C] + [(1, c) for c in R.PAIR_DIRECT_C])
def test_edge_class_counts_exact(lib, form, C):
    L, stream = lib
    N = 300
    try:
        assert L.sgs_edge_class_variant_set(form) == 0
        for n in R.PAIR_N_EDGES:
            for with_mask in (False, True):
                ei, y, m = R.make_pairs_case(n, N, C, 13 * n + C + with_mask, with_mask)
                if n >= 8:
                    assert (y == -100).any() and (y == C).any() and (ei == N).any()
                want = R.edge_class_ref(ei, y, N, C, m)
                assert L.sgs_edge_class_variant(n, C) == (form if n else 0)
                d_ei, d_y = torch.from_numpy(ei).to(DEV), torch.from_numpy(y).to(DEV)
                d_m = torch.from_numpy(m).to(DEV) if m is not None else None
                base = np.arange(C * C, dtype=np.int64) * 1000003 + (1 << 33)
                out = Zoned(C * C, torch.int64, -5)
                out.set(base)
                for rep in (1, 2):                                               # accumulated over two calls
                    rc = L.sgs_edge_class_counts(d_ei.data_ptr() if n else None, n, d_m.data_ptr() if d_m is not None and n else None,
                                                 d_y.data_ptr(), N, C, out.ptr, stream())
                    assert rc == 0, L.sgs_last_error()
                    assert np.array_equal(out.get().reshape(C, C), base.reshape(C, C) + rep * want), (form, C, n, with_mask, rep)
        if C > 128:                                                              # the privatised form beyond its LDS limit: refused, nothing launched
            L.sgs_edge_class_variant_set(2)
            out = Zoned(C * C, torch.int64, -5)
            assert L.sgs_edge_class_counts(d_ei.data_ptr(), 70003, None, d_y.data_ptr(), N, C, out.ptr, stream()) == -1
            assert b"privatised" in L.sgs_last_error() and bool((out.get() == -5).all())
    finally:
        L.sgs_edge_class_variant_set(0)


def test_edge_class_counts_forms_agree_and_wrapper(lib):
    import sgs_gnn_amd as S
    ops = S.ops
    N, C, n = 300, 5, 70003
    ei, y, m = R.make_pairs_case(n, N, C, 77, True)
    want = torch.from_numpy(R.edge_class_ref(ei, y, N, C, m))
    d_ei, d_y, d_m = torch.from_numpy(ei).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(m).to(DEV)
    try:
        got = {}
        for code in (0, 1, 2):
            ops.edge_class_variant_set(code)
            got[code] = ops.edge_class_counts(d_ei, d_y, N, C, mask=d_m).cpu()
            assert torch.equal(got[code], want), code
        assert ops.edge_class_variant(n, C) == 2
        ops.edge_class_variant_set(0)
        assert ops.edge_class_variant(n, C) == 2 and ops.edge_class_variant(n, 129) == 1
        full = ops.edge_class_counts(d_ei, d_y, N, C, mask=d_m != 0)             # a bool mask
        assert torch.equal(full.cpu(), want)
        acc = ops.edge_class_counts(d_ei, d_y, N, C, mask=d_m, out=full)
        assert acc is full and torch.equal(full.cpu(), 2 * want)
        with pytest.raises(RuntimeError, match="out must be"):
            ops.edge_class_counts(d_ei, d_y, N, C, out=torch.zeros(C, C + 1, dtype=torch.int64, device=DEV))
        with pytest.raises(RuntimeError, match="y must be"):
            ops.edge_class_counts(d_ei, d_y.int(), N, C)
        with pytest.raises(RuntimeError, match="edge_index must be"):
            ops.edge_class_counts(d_ei.int(), d_y, N, C)
    finally:
        ops.edge_class_variant_set(0)


# ------------------------------------------------------------------ the ops wrappers over the same kernels
def test_ops_wrappers_compose(lib):
    import sgs_gnn_amd as S
    ops = S.ops
    E, D, q = 4097, 11, 800
    _, rows = R.make_masks(E, D, 0, 5)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    hist = torch.zeros(128, dtype=torch.int64, device=DEV)
    count = ops.consensus_accum(d_rows[:4])
    count = ops.consensus_accum(d_rows[4:], count, first=False, hist=hist)
    want, want_h = R.accum_ref(rows, hist=np.zeros(128, dtype=np.int64))
    assert np.array_equal(count.cpu().numpy(), want) and np.array_equal(hist.cpu().numpy(), want_h)
    _, p = R.make_counts_scores(E, D, 9)
    ei = np.random.default_rng(1).integers(0, 1000, size=(2, E), dtype=np.int64)
    r = ops.consensus_select(count, torch.from_numpy(p).to(DEV), q, torch.from_numpy(ei).to(DEV), want_keys=True)
    ref = R.select_ref(want, p, q, ei)
    assert (r.E, r.q) == (E, q) and r.mask.dtype == torch.bool
    assert np.array_equal(r.mask.cpu().numpy().astype(np.uint8), ref["mask"]) and np.array_equal(r.eid.cpu().numpy(), ref["eid"])
    assert np.array_equal(r.edge_index.cpu().numpy(), ref["edge_index"]) and np.array_equal(r.count.cpu().numpy(), ref["count"])
    assert np.array_equal(r.keys.cpu().numpy().astype(np.uint32), ref["keys"])
    assert np.array_equal(r.p.cpu().numpy().view(np.uint32), ref["p"].view(np.uint32))
    r0 = ops.consensus_select(count, None, q, None)
    assert r0.edge_index is None and r0.keys is None
    assert np.array_equal(r0.eid.cpu().numpy(), R.select_ref(want, None, q)["eid"]) and bool((r0.p == 1).all())
    with pytest.raises(RuntimeError, match="without replacement"):
        ops.consensus_select(count, None, E + 1, None)
    with pytest.raises(RuntimeError, match="count must be"):
        ops.consensus_select(count.long(), None, q, None)
    with pytest.raises(RuntimeError, match="p must be"):
        ops.consensus_select(count, torch.zeros(E, dtype=torch.float64, device=DEV), q, None)
    with pytest.raises(RuntimeError, match="count is required"):
        ops.consensus_accum(d_rows, None, first=False)
    with pytest.raises(RuntimeError, match="hist must be"):
        ops.consensus_accum(d_rows, hist=torch.zeros(64, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="bool or uint8"):
        ops.consensus_accum(d_rows.float())
