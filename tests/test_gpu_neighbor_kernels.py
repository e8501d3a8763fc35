"""GPU: every sgs_nbr_* entry point through the C ABI, outputs, state and the exactly sized workspaces between red zones, against
tests/neighbor_ref.py by exact equality.  Case table (neighbor_ref.kernel_case): in-rows of 0, 1, f - 1, f, f + 1, 63, 64, 65, 255, 256, 257,
hub and hub + 1 entries, N = 131 nodes (no multiple of the four waves of a workgroup), frontiers of 0, 1, 3 and N rows, f in
{1, 2, 25, 64, 65, -1}; a whole batch stage by stage for both subgraph types; ids, rows and columns outside their range; SGS_EINVAL."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ref as R  # noqa: E402
from zoned import DEV, Zoned  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = -77777


@pytest.fixture(scope="module")
def lib():
    import sgs_gnn_amd as S
    return S._lib.lib()


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ok(lib, rc):
    assert rc == 0, lib.sgs_last_error()
    torch.cuda.synchronize()


def _select(lib, ptr, eid, N, rows, f, K, cap=None):
    want_offs, want = R.select(ptr, eid, N, rows, f, K)
    total = int(want_offs[-1])
    cap = total if cap is None else cap
    d = [_dev(ptr), _dev(eid), _dev(rows)]
    chosen, tot = Zoned(cap, torch.int32, FILL), Zoned(1, torch.int64, FILL)
    nbytes = lib.sgs_nbr_select_workspace_bytes(len(rows))
    assert nbytes % 8 == 0
    ws = Zoned(nbytes // 8, torch.int64, FILL)
    _ok(lib, lib.sgs_nbr_select(d[0].data_ptr(), d[1].data_ptr(), N, eid.shape[0], d[2].data_ptr(), len(rows), f, K, chosen.ptr, cap, tot.ptr,
                                 ws.ptr, nbytes, None))
    offs = ws.get()[:len(rows) + 1]
    assert np.array_equal(offs, want_offs) and int(tot.get()[0]) == total
    got = chosen.get().copy()
    assert np.array_equal(got, want[:cap])
    return got


class State:
    def __init__(self, lib, N):
        self.lib, self.N = lib, N
        self.bytes = lib.sgs_nbr_state_bytes(N)
        assert self.bytes % 4 == 0
        self.z = Zoned(self.bytes // 4, torch.int32, FILL)
        self.W = (N + 31) // 32

    def begin(self, seeds):
        d = _dev(seeds)
        _ok(self.lib, self.lib.sgs_nbr_begin(d.data_ptr(), len(seeds), self.N, self.z.ptr, self.bytes, None))

    def bitmaps(self):
        """-> (members, reached, seeds) as bool [N]"""
        words = self.z.get().view(np.uint32)
        stride = ((self.W + 1) * 4 + 255) // 256 * 64
        out = []
        for j in range(3):
            w = words[j * stride:j * stride + self.W]
            out.append(np.unpackbits(w.view(np.uint8), bitorder="little")[:self.N].astype(bool))
        return out


def _frontier(lib, st, chosen, ei_dev, E, in_ptr, next_f, member, src_ref, cap=None):
    """runs sgs_nbr_frontier and the reference from the same state; `member` (the reference's) is updated"""
    N = st.N
    want = R.frontier(chosen, src_ref, E, N, member)
    want_next = R.next_total(in_ptr, want, next_f) if next_f != 0 else 0
    cap = want.shape[0] if cap is None else cap
    d = [_dev(chosen), _dev(in_ptr)]
    out, sizes = Zoned(cap, torch.int32, FILL), Zoned(2, torch.int64, FILL)
    _ok(lib, lib.sgs_nbr_frontier(d[0].data_ptr(), len(chosen), ei_dev.data_ptr(), E, N, d[1].data_ptr(), next_f, st.z.ptr, st.bytes, out.ptr, cap,
                                   sizes.ptr, None))
    assert sizes.get().tolist() == [want.shape[0], want_next]
    assert np.array_equal(out.get(), want[:cap])
    got_member, reached, _ = st.bitmaps()
    assert np.array_equal(got_member, member) and not reached.any()
    return want


def _collate(lib, st, g, data, member, seeds, chosen, ei_dev, sub):
    """sgs_nbr_nodes, the edges of `sub`, sgs_nbr_gather -> compared with the reference's batch"""
    N, E, n = g.N, g.E, int(member.sum())
    wpre, nodes, mism = Zoned(st.W, torch.int32, FILL), Zoned(n, torch.int64, FILL), Zoned(1, torch.int32, 0)
    _ok(lib, lib.sgs_nbr_nodes(st.z.ptr, st.bytes, N, n, wpre.ptr, nodes.ptr, mism.ptr, None))
    node_ids = nodes.get().copy()
    assert np.array_equal(node_ids, np.nonzero(member)[0]) and int(mism.get()[0]) == 0
    words = np.packbits(np.pad(member, (0, st.W * 32 - N)), bitorder="little").view(np.uint32)
    pop = np.asarray([bin(int(w)).count("1") for w in words])
    assert np.array_equal(wpre.get(), np.cumsum(pop) - pop)
    prob = _dev(data["prob"], np.float32)
    if sub == "induced":
        want_ei, want_eid = R.induced(g.out_ptr, g.out_dst, g.out_eid, N, E, member)
        d = [_dev(g.out_ptr), _dev(g.out_dst), _dev(g.out_eid)]
        rowptr, tot = Zoned(n + 1, torch.int64, FILL), Zoned(1, torch.int64, FILL)
        _ok(lib, lib.sgs_nbr_induced_count(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), N, E, st.z.ptr, st.bytes, wpre.ptr, nodes.ptr, n,
                                            rowptr.ptr, tot.ptr, None))
        E_b = int(tot.get()[0])
        assert E_b == want_eid.shape[0]
        cnt = np.bincount(want_ei[0], minlength=n)
        assert np.array_equal(rowptr.get(), np.concatenate([[0], np.cumsum(cnt)]))
        ei, pr, eid = Zoned(2 * E_b, torch.int64, FILL), Zoned(E_b, torch.float32, -7.0), Zoned(E_b, torch.int64, FILL)
        _ok(lib, lib.sgs_nbr_induced_fill(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), prob.data_ptr(), N, E, st.z.ptr, st.bytes, wpre.ptr,
                                           nodes.ptr, n, rowptr.ptr, E_b, ei.ptr, pr.ptr, eid.ptr, None))
        got_ei = ei.get().reshape(2, E_b)
    else:
        want_ei, want_eid = R.directional(np.concatenate(chosen) if chosen else np.zeros(0, np.int32), g.ei, E, N, member)
        segs = [_dev(c) for c in chosen if c.shape[0]]
        m = sum(s.numel() for s in segs)
        table = (ctypes.c_int64 * (2 * max(len(segs), 1)))(*([v for s in segs for v in (s.data_ptr(), s.numel())] or [0, 0]))
        nbytes = lib.sgs_nbr_directional_workspace_bytes(m)
        assert nbytes % 8 == 0
        ws = Zoned(nbytes // 8, torch.int64, FILL)
        ei, pr, eid, tot = Zoned(2 * m, torch.int64, FILL), Zoned(m, torch.float32, -7.0), Zoned(m, torch.int64, FILL), Zoned(1, torch.int64, FILL)
        _ok(lib, lib.sgs_nbr_directional(table, max(len(segs), 1), m, ei_dev.data_ptr(), E, N, prob.data_ptr(), st.z.ptr, st.bytes, wpre.ptr, ei.ptr,
                                          pr.ptr, eid.ptr, tot.ptr, ws.ptr, nbytes, None))
        ws.get()
        E_b = int(tot.get()[0])
        assert E_b == want_eid.shape[0]
        got_ei = ei.get().reshape(2, m)[:, :E_b]
        assert (ei.get().reshape(2, m)[:, E_b:] == FILL).all() and (eid.get()[E_b:] == FILL).all()       # dropped ids leave the tail alone
    assert np.array_equal(got_ei, want_ei) and np.array_equal(eid.get()[:E_b], want_eid)
    assert np.array_equal(pr.get()[:E_b], data["prob"][want_eid])
    F = data["x"].shape[1]
    x, y = Zoned(n * F, torch.float32, -7.0), Zoned(n, torch.int64, FILL)
    mo, so = Zoned(3 * n, torch.uint8, 9), Zoned(n, torch.uint8, 9)
    dx, dy, dm = _dev(data["x"], np.float32), _dev(data["y"], np.int64), _dev(data["masks"], np.uint8)
    _ok(lib, lib.sgs_nbr_gather(nodes.ptr, n, N, dx.data_ptr(), F * 4, x.ptr, dy.data_ptr(), y.ptr, dm.data_ptr(), st.z.ptr, st.bytes, mo.ptr, so.ptr,
                                 None))
    is_seed = np.zeros(N, dtype=bool)
    is_seed[np.asarray(seeds)] = True
    assert np.array_equal(x.get().reshape(n, F), data["x"][node_ids]) and np.array_equal(y.get(), data["y"][node_ids])
    assert np.array_equal(so.get().astype(bool), is_seed[node_ids])
    assert np.array_equal(mo.get().reshape(3, n).astype(bool), data["masks"][:, node_ids] & is_seed[node_ids][None, :])


def _batch(lib, g, data, seeds, fans, keys):
    """one batch through the C ABI, every stage against the reference, both subgraph types at the end"""
    st = State(lib, g.N)
    st.begin(seeds)
    member = np.zeros(g.N, dtype=bool)
    member[np.asarray(seeds, dtype=np.int64)] = True
    got_m, _, got_s = st.bitmaps()
    assert np.array_equal(got_m, member) and np.array_equal(got_s, member)
    ei_dev = _dev(g.ei, np.int64)
    front, chosen = np.asarray(seeds, dtype=np.int32), []
    for h, (f, K) in enumerate(zip(fans, keys)):
        c = _select(lib, g.in_ptr, g.in_eid, g.N, front, f, K)
        chosen.append(c)
        front = _frontier(lib, st, c, ei_dev, g.E, g.in_ptr, fans[h + 1] if h + 1 < len(fans) else 0, member, g.ei[0]).astype(np.int32)
    for sub in R.SUBGRAPH_TYPES:
        _collate(lib, st, g, data, member, seeds, chosen, ei_dev, sub)
    return int(member.sum())


@pytest.mark.parametrize("f", R.FANOUTS)
def test_kernel_case_table(lib, f):
    hub = lib.sgs_nbr_select_hub_row()
    ei, N = R.kernel_case(f, hub, seed=abs(f))
    g = R.Graph(ei, N)
    deg = np.diff(g.in_ptr).tolist()
    ff = f if f > 0 else 7
    assert N % 4 == 3 and set(R.ROW_LENGTHS + (max(ff - 1, 0), ff, ff + 1, hub, hub + 1)) <= set(deg)
    K = R.stream_key(3, 1, 4, 1)
    for rows in R.kernel_frontiers(N, seed=f + 5):
        first = _select(lib, g.in_ptr, g.in_eid, N, rows, f, K)
        assert np.array_equal(_select(lib, g.in_ptr, g.in_eid, N, rows, f, K), first)            # the same bits on a second call
    data = R.node_data(g, 5, 3, 1)
    seeds = np.random.default_rng(f + 9).permutation(N)[:3]
    n = _batch(lib, g, data, seeds, [f, f], [K, R.stream_key(3, 1, 4, 2)])
    assert n > 3


def test_hub_row_goes_through_the_workgroup_form(lib):
    """rows of hub and hub + 1 entries side by side in one tile: the longer one is above sgs_nbr_select_hub_row(), so its workgroup's four
    waves select it together; fan-outs below, at and above the hub length, and the plain copy"""
    hub = lib.sgs_nbr_select_hub_row()
    ei, N = R.kernel_case(25, hub, seed=2)
    g = R.Graph(ei, N)
    deg = np.diff(g.in_ptr)
    a, b = int(np.nonzero(deg == hub)[0][0]), int(np.nonzero(deg == hub + 1)[0][0])
    small = int(np.nonzero(deg == 3)[0][0]) if (deg == 3).any() else int(np.argmin(deg))
    for f in (1, 25, 300, hub, hub + 1, hub + 2, -1):
        for rows in ([b], [a, b, small, b], [small, b, a]):
            got = _select(lib, g.in_ptr, g.in_eid, N, np.asarray(rows, dtype=np.int32), f, 0xDEADBEEF)
            assert got.shape[0] == sum(int(deg[r]) if f < 0 else min(f, int(deg[r])) for r in rows)


def test_out_of_range_ids_rows_and_columns_are_skipped(lib):
    ei, N = R.kernel_case(2, 70, seed=6)
    g = R.Graph(ei, N)
    data = R.node_data(g, 3, 2, 0)
    rng = np.random.default_rng(1)
    # rows outside [0, N) are empty rows; ids pass through the selection unread
    rows = np.asarray([5, -1, N, 17, N + 5, 2 ** 31 - 1, 40], dtype=np.int32)
    bad_eid = g.in_eid.copy()
    hit = rng.random(g.E) < 0.2
    bad_eid[hit] = rng.choice(np.asarray([-1, g.E, g.E + 7, -2 ** 31, 2 ** 31 - 1], dtype=np.int64), int(hit.sum())).astype(np.int32)
    for f in (2, -1):
        _select(lib, g.in_ptr, bad_eid, N, rows, f, 99)
    # the frontier skips ids outside [0, E) and sources outside [0, N)
    st = State(lib, N)
    seeds = [3, 9]
    st.begin(seeds + [-4, N + 1])                                                              # a seed outside the range is skipped
    member = np.zeros(N, dtype=bool)
    member[seeds] = True
    assert np.array_equal(st.bitmaps()[0], member)
    src = g.ei[0].copy()
    src[rng.random(g.E) < 0.2] = N + 3
    src[rng.random(g.E) < 0.1] = -1
    bad_ei = _dev(np.stack([src, g.ei[1]]), np.int64)
    chosen = bad_eid[rng.permutation(g.E)[:200]]
    _frontier(lib, st, chosen, bad_ei, g.E, g.in_ptr, -1, member, src)
    # the collate skips columns / ids outside their range (induced) and ids whose ends are no members (directional)
    gb = R.Graph(ei, N)
    gb.out_dst = g.out_dst.copy()
    gb.out_dst[rng.random(g.E) < 0.1] = N
    gb.out_dst[rng.random(g.E) < 0.1] = -5
    gb.out_eid = g.out_eid.copy()
    gb.out_eid[rng.random(g.E) < 0.1] = g.E
    good_ei = _dev(g.ei, np.int64)
    _collate(lib, st, gb, data, member, seeds, [], good_ei, "induced")
    _collate(lib, st, g, data, member, seeds, [chosen[:120], chosen[120:]], good_ei, "directional")


def test_caps_bound_every_write(lib):
    ei, N = R.kernel_case(25, 70, seed=8)
    g = R.Graph(ei, N)
    rows = np.arange(N, dtype=np.int32)
    _select(lib, g.in_ptr, g.in_eid, N, rows, 25, 5, cap=100)
    st = State(lib, N)
    st.begin([0])
    member = np.zeros(N, dtype=bool)
    member[0] = True
    _frontier(lib, st, np.arange(g.E, dtype=np.int32), _dev(g.ei, np.int64), g.E, g.in_ptr, 3, member, g.ei[0], cap=10)


def test_argument_errors(lib):
    ei, N = R.kernel_case(2, 70, seed=6)
    g = R.Graph(ei, N)
    d = [_dev(g.in_ptr), _dev(g.in_eid), _dev(np.arange(4))]
    buf = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()
    sel = lambda **kw: lib.sgs_nbr_select(*[kw.get(k, v) for k, v in (("ptr", d[0].data_ptr()), ("eid", d[1].data_ptr()), ("N", N), ("nnz", g.E),  # noqa: E731
                                                                      ("rows", d[2].data_ptr()), ("n_rows", 4), ("f", 2), ("key", 1), ("chosen", p),
                                                                      ("cap", 8), ("total", None), ("ws", p + 1024), ("ws_bytes", 1024), ("stream", None))])
    assert sel() == 0
    for kw, msg in ((dict(f=0), b"fanout"), (dict(f=-2), b"fanout"), (dict(N=0), b"bad sizes"), (dict(N=2 ** 31), b"bad sizes"), (dict(nnz=-1), b"bad sizes"),
                    (dict(n_rows=-1), b"n_rows"), (dict(ptr=None), b"null"), (dict(rows=None), b"null"), (dict(chosen=None), b"null"),
                    (dict(ws=None), b"null"), (dict(ws=p + 1028), b"aligned")):
        assert sel(**kw) == -1 and msg in lib.sgs_last_error(), kw
    assert sel(ws_bytes=8) == -2
    sb = lib.sgs_nbr_state_bytes(N)
    assert lib.sgs_nbr_begin(d[2].data_ptr(), 4, N, p, sb - 4, None) == -2
    assert lib.sgs_nbr_begin(d[2].data_ptr(), 4, 0, p, sb, None) == -1 and lib.sgs_nbr_begin(None, 4, N, p, sb, None) == -1
    assert lib.sgs_nbr_begin(d[2].data_ptr(), 4, N, p + 2, sb, None) == -1 and lib.sgs_nbr_begin(d[2].data_ptr(), 4, N, None, sb, None) == -1
    assert lib.sgs_nbr_begin(d[2].data_ptr(), 4, N, p, sb, None) == 0
    fr = lambda nf=0, sizes=p + 2048, E=g.E: lib.sgs_nbr_frontier(d[1].data_ptr(), 4, p + 4096, E, N, d[0].data_ptr(), nf, p, sb, p + 8192, 4, sizes, None)  # noqa: E731
    assert fr(nf=-2) == -1 and fr(sizes=None) == -1 and fr(E=2 ** 31) == -1
    assert lib.sgs_nbr_nodes(p, sb, N, N + 1, p + 2048, p + 4096, None, None) == -1 and lib.sgs_nbr_nodes(p, sb, N, 1, None, p + 4096, None, None) == -1
    assert lib.sgs_nbr_induced_count(d[0].data_ptr(), d[1].data_ptr(), d[1].data_ptr(), N, g.E, p, sb, p + 2048, p + 4096, N + 1, p + 8192, None, None) == -1
    assert lib.sgs_nbr_induced_fill(d[0].data_ptr(), d[1].data_ptr(), d[1].data_ptr(), None, N, g.E, p, sb, p + 2048, p + 4096, 1, p + 8192, 1, p + 9000,
                                    p + 9100, None, None) == -1 and b"prob_out without prob" in lib.sgs_last_error()
    seg = (ctypes.c_int64 * 2)(d[1].data_ptr(), 4)
    wb = lib.sgs_nbr_directional_workspace_bytes(4)
    big = torch.zeros(wb // 8 + 1, dtype=torch.int64, device=DEV)
    dr = lambda n_seg=1, m=4, ws_bytes=wb: lib.sgs_nbr_directional(seg, n_seg, m, p + 4096, g.E, N, None, p, sb, p + 2048, p + 8192, None, None, p + 9000,  # noqa: E731
                                                                  big.data_ptr(), ws_bytes, None)
    assert dr(n_seg=0) == -1 and dr(n_seg=lib.sgs_nbr_max_hops() + 1) == -1 and dr(ws_bytes=64) == -2
    assert dr(m=5) == -1 and b"segments hold" in lib.sgs_last_error()
    assert lib.sgs_nbr_gather(p + 4096, 1, N, p, 6, p + 8192, p, p, p, p, sb, p, p, None) == -1 and b"4-byte" in lib.sgs_last_error()
    assert lib.sgs_nbr_gather(p + 4096, N + 1, N, p, 8, p + 8192, p, p, p, p, sb, p, p, None) == -1
    torch.cuda.synchronize()


def test_ops_wrappers_refuse_cpu_tensors():
    import sgs_gnn_amd as S
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.nbr_select(torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 2, torch.zeros(1, dtype=torch.int32), 2, 0, 1)
    assert S.ops.nbr_select_hub_row() >= 256 and S.ops.nbr_max_hops() >= 3
