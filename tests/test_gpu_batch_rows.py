"""GPU: the paths of csrc/batch_rows.h that the two builders' own kernel tests do not reach, through the C ABI with red zones around every
output and workspace, against tests/neighbor_ref.py and tests/cluster_collate_ref.py by exact equality.
  - the induced collate's hub form: out-rows of 0, 1, 63, 64, 65, 255, 256, 257, hub and hub + 1 entries (hub = sgs_nbr_select_hub_row()),
    the two hub rows in one 4-row tile, as rows and as columns only, and a fill whose E_b is one too small;
  - the cluster collate with TWO hub rows in one 16-row tile (two slots of the slice-count table), rows of exactly 1024 and 1025 entries
    on either side of its threshold, groups of 1, 2 and 3 partitions;
  - the shared scan's second tile: 4095, 4096, 4097 and 8193 items, as sgs_nbr_select's offsets and as sgs_cluster_collate_count's rowptr."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ref as R  # noqa: E402
from cluster_collate_ref import collate_ref, full_csr_ref  # noqa: E402
from zoned import DEV, Zoned  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = -77777
SCAN_SIZES = (4095, 4096, 4097, 8193)


@pytest.fixture(scope="module")
def lib():
    import sgs_gnn_amd as S
    return S._lib.lib()


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ok(lib, rc):
    assert rc == 0, lib.sgs_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- induced collate: hub rows
@pytest.fixture(scope="module")
def hub_graph(lib):
    """neighbor_ref.kernel_case with source and destination swapped: the OUT-rows carry the case table's lengths"""
    hub = int(lib.sgs_nbr_select_hub_row())
    ei, N = R.kernel_case(25, hub, seed=7)
    g = R.Graph(ei[::-1], N)
    deg = np.diff(g.out_ptr)
    assert N == 131 and set(R.ROW_LENGTHS + (hub, hub + 1)) <= set(deg.tolist())
    a, b = int(np.nonzero(deg == hub)[0][0]), int(np.nonzero(deg == hub + 1)[0][0])
    prob = (np.random.default_rng(5).random(g.E).astype(np.float32) + np.float32(0.5)) / np.float32(g.E)
    d = dict(ptr=_dev(g.out_ptr), dst=_dev(g.out_dst), eid=_dev(g.out_eid), prob=_dev(prob, np.float32))
    return dict(g=g, hubs=(a, b), prob=prob, d=d)


def _member_sets(N, hubs):
    a, b = hubs
    rest = [v for v in range(N) if v not in hubs]
    return {"all": list(range(N)), "hubs_and_three": [a, b, rest[1], rest[-2], rest[-1]], "hubs_as_columns_only": rest}


@pytest.mark.parametrize("which", ["all", "hubs_and_three", "hubs_as_columns_only"])
def test_induced_collate_hub_rows(lib, hub_graph, which):
    g, d, prob, (a, b) = hub_graph["g"], hub_graph["d"], hub_graph["prob"], hub_graph["hubs"]
    N, E = g.N, g.E
    nodes_in = _member_sets(N, (a, b))[which]
    member = np.zeros(N, dtype=bool)
    member[nodes_in] = True
    n = int(member.sum())
    if which != "hubs_as_columns_only":                  # both hub rows in one tile of four local rows: two slots of the slice-count table
        rank = np.cumsum(member) - 1
        assert member[a] and member[b] and rank[a] // 4 == rank[b] // 4
    else:
        assert not member[a] and not member[b]
    want_ei, want_eid = R.induced(g.out_ptr, g.out_dst, g.out_eid, N, E, member)
    E_b = int(want_eid.shape[0])
    assert E_b > 0
    sb = lib.sgs_nbr_state_bytes(N)
    assert sb % 4 == 0
    st = Zoned(sb // 4, torch.int32, FILL)
    seeds = _dev(nodes_in)
    _ok(lib, lib.sgs_nbr_begin(seeds.data_ptr(), len(nodes_in), N, st.ptr, sb, None))
    wpre, nodes, mism = Zoned((N + 31) // 32, torch.int32, FILL), Zoned(n, torch.int64, FILL), Zoned(1, torch.int32, 0)
    _ok(lib, lib.sgs_nbr_nodes(st.ptr, sb, N, n, wpre.ptr, nodes.ptr, mism.ptr, None))
    assert np.array_equal(nodes.get(), np.nonzero(member)[0]) and int(mism.get()[0]) == 0
    csr = (d["ptr"].data_ptr(), d["dst"].data_ptr(), d["eid"].data_ptr())
    rowptr, tot = Zoned(n + 1, torch.int64, FILL), Zoned(1, torch.int64, FILL)
    _ok(lib, lib.sgs_nbr_induced_count(*csr, N, E, st.ptr, sb, wpre.ptr, nodes.ptr, n, rowptr.ptr, tot.ptr, None))
    assert int(tot.get()[0]) == E_b
    assert np.array_equal(rowptr.get(), np.concatenate([[0], np.cumsum(np.bincount(want_ei[0], minlength=n))]))
    for short in (0, 1):                                  # the exact E_b, then one below the count
        m = E_b - short
        ei, pr, eid = Zoned(2 * m, torch.int64, FILL), Zoned(m, torch.float32, -7.0), Zoned(m, torch.int64, FILL)
        _ok(lib, lib.sgs_nbr_induced_fill(*csr, d["prob"].data_ptr(), N, E, st.ptr, sb, wpre.ptr, nodes.ptr, n, rowptr.ptr, m, ei.ptr, pr.ptr,
                                           eid.ptr, None))
        assert np.array_equal(ei.get().reshape(2, m), want_ei[:, :m])                       # (get() also checks the red zones)
        assert np.array_equal(eid.get(), want_eid[:m])
        assert np.array_equal(pr.get().view(np.uint32), prob[want_eid[:m]].view(np.uint32))
    for z in (st, wpre, nodes, rowptr, tot):
        z.get()


# ---------------------------------------------------------------- cluster collate: two hub rows in one tile
CN, CP = 1100, 3
C_SIZES = [400, 300, 400]
C_GROUPS = [(0,), (0, 2), (0, 1, 2)]


@pytest.fixture(scope="module")
def two_hub_graph():
    """1100 nodes in 3 partitions.  In the permuted order the nodes 18 and 19 (one 16-row tile of every group that holds partition 0) have
    rows of 1060 and 1090 entries, node 40 one of exactly 1024 (the longest a wave walks alone) and a node of partition 2 one of exactly
    1025 (the shortest hub); every other row has 0 to 20."""
    rng = np.random.default_rng(23)
    part = np.repeat(np.arange(CP), C_SIZES)[rng.permutation(CN)]
    perm = np.argsort(part, kind="stable")
    lens = rng.integers(0, 21, CN)
    lens[perm[18]], lens[perm[19]], lens[perm[40]], lens[perm[C_SIZES[0] + C_SIZES[1] + 7]] = 1060, 1090, 1024, 1025
    src = np.repeat(np.arange(CN), lens)
    dst = np.concatenate([rng.permutation(CN)[:k] for k in lens])                              # distinct columns inside a row
    ei = np.stack([src, dst]).astype(np.int64)
    c = full_csr_ref(ei, part, CP)
    deg = np.diff(c["full_ptr"])
    assert deg[18] > 1024 and deg[19] > 1024 and 18 // 16 == 19 // 16 and deg[40] == 1024 and (deg == 1025).sum() == 1
    g = dict(c, ei=ei, part=part, prob=rng.random(ei.shape[1], dtype=np.float32), masks=rng.integers(0, 2, (3, CN)).astype(np.uint8))
    g["new_ei"] = np.stack([np.repeat(np.arange(CN), deg), c["full_col"]])
    g["csr_prob"], g["csr_masks"] = g["prob"][c["order"]], np.ascontiguousarray(g["masks"][:, c["perm"]])
    g["d"] = {k: torch.from_numpy(np.ascontiguousarray(g[k])).to(DEV) for k in ("full_ptr", "full_col", "csr_prob", "csr_masks")}
    return g


def _cluster_outputs(n_b, E_b):
    return dict(ei=Zoned(2 * E_b, torch.int64, -7), prob=Zoned(E_b, torch.float32, -1.0), eid=Zoned(E_b, torch.int64, -7),
                attr=Zoned(3 * n_b, torch.uint8, 9), mis=Zoned(1, torch.int32, 0))


def _cluster_collate(lib, g, arr, k, n_b, E_b, N):
    d = g["d"]
    nbytes = lib.sgs_cluster_collate_workspace_bytes(n_b)
    assert nbytes % 8 == 0
    ws, out = Zoned(nbytes // 8, torch.int64, FILL), _cluster_outputs(n_b, E_b)
    _ok(lib, lib.sgs_cluster_collate(d["full_ptr"].data_ptr(), d["full_col"].data_ptr(), d["csr_prob"].data_ptr(), arr, k, n_b, E_b, out["ei"].ptr,
                                      out["prob"].ptr, out["eid"].ptr, d["csr_masks"].data_ptr(), out["attr"].ptr, 3, N, out["mis"].ptr, ws.ptr,
                                      nbytes, None))
    ws.get()
    return {name: z.get() for name, z in out.items()}


@pytest.mark.parametrize("group", C_GROUPS, ids=str)
def test_cluster_collate_two_hub_rows_in_one_tile(lib, two_hub_graph, group):
    g, d = two_hub_graph, two_hub_graph["d"]
    nptr = g["node_ptr"]
    ranges = [(int(nptr[p]), int(nptr[p + 1])) for p in group]
    pseudo = np.full(CN, len(ranges), dtype=np.int64)
    for j, (lo, hi) in enumerate(ranges):
        pseudo[lo:hi] = j
    ref = collate_ref(g["new_ei"], pseudo, range(len(ranges)), g["csr_prob"])
    n_b, E_b = int(ref["node_ids"].shape[0]), int(ref["edge_index"].shape[1])
    assert n_b == sum(C_SIZES[p] for p in group) and E_b > 1024
    arr = (ctypes.c_int64 * (2 * len(ranges)))(*[v for r in ranges for v in r])
    nbytes = lib.sgs_cluster_collate_workspace_bytes(n_b)
    ws, tot = Zoned(nbytes // 8, torch.int64, FILL), Zoned(1, torch.int64, FILL)
    _ok(lib, lib.sgs_cluster_collate_count(d["full_ptr"].data_ptr(), d["full_col"].data_ptr(), arr, len(ranges), n_b, tot.ptr, ws.ptr, nbytes, None))
    assert int(tot.get()[0]) == E_b
    assert np.array_equal(ws.get()[:n_b + 1], np.concatenate([[0], np.cumsum(np.bincount(ref["edge_index"][0], minlength=n_b))]))
    got = _cluster_collate(lib, g, arr, len(ranges), n_b, E_b, CN)
    assert int(got["mis"][0]) == 0
    assert np.array_equal(got["ei"].reshape(2, E_b), ref["edge_index"]) and np.array_equal(got["eid"], ref["eid"])
    assert np.array_equal(got["prob"].view(np.uint32), ref["prob"].view(np.uint32))
    assert np.array_equal(got["attr"].reshape(3, n_b), g["csr_masks"][:, ref["node_ids"]])
    short = _cluster_collate(lib, g, arr, len(ranges), n_b, E_b - 1, CN)                       # E_b one too small: reported, nothing leaves [0, E_b)
    assert int(short["mis"][0]) == 1
    assert np.array_equal(short["ei"].reshape(2, E_b - 1), ref["edge_index"][:, :E_b - 1]) and np.array_equal(short["eid"], ref["eid"][:E_b - 1])
    assert np.array_equal(short["prob"].view(np.uint32), ref["prob"][:E_b - 1].view(np.uint32))


# ---------------------------------------------------------------- the scan across tile borders
@pytest.fixture(scope="module")
def wide_graph():
    """8193 nodes with in-degrees 0 to 3: more rows than two tiles of the scan (4096 items each)"""
    rng = np.random.default_rng(31)
    N = SCAN_SIZES[-1]
    dst = np.repeat(np.arange(N), rng.integers(0, 4, N))
    g = R.Graph(np.stack([rng.integers(0, N, dst.shape[0]), dst]).astype(np.int64), N)
    assert set(np.diff(g.in_ptr).tolist()) == {0, 1, 2, 3}
    return g, rng.permutation(N).astype(np.int32)


@pytest.mark.parametrize("n_rows", SCAN_SIZES)
def test_scan_second_tile_as_select_offsets(lib, wide_graph, n_rows):
    g, order = wide_graph
    rows = order[:n_rows]
    want_offs, want = R.select(g.in_ptr, g.in_eid, g.N, rows, -1, 0)
    total = int(want_offs[-1])
    d = [_dev(g.in_ptr), _dev(g.in_eid), _dev(rows)]
    chosen, tot = Zoned(total, torch.int32, FILL), Zoned(1, torch.int64, FILL)
    nbytes = lib.sgs_nbr_select_workspace_bytes(n_rows)
    assert nbytes % 8 == 0
    ws = Zoned(nbytes // 8, torch.int64, FILL)
    _ok(lib, lib.sgs_nbr_select(d[0].data_ptr(), d[1].data_ptr(), g.N, g.E, d[2].data_ptr(), n_rows, -1, 0, chosen.ptr, total, tot.ptr, ws.ptr,
                                 nbytes, None))
    assert np.array_equal(ws.get()[:n_rows + 1], want_offs) and int(tot.get()[0]) == total
    assert np.array_equal(chosen.get(), want)


@pytest.mark.parametrize("n_b", SCAN_SIZES)
def test_scan_second_tile_as_cluster_rowptr(lib, wide_graph, n_b):
    g, _ = wide_graph
    ptr, col = _dev(g.out_ptr, np.int64), _dev(g.out_dst, np.int64)
    ref = collate_ref(g.ei, (np.arange(g.N) >= n_b).astype(np.int64), [0])                       # one partition range [0, n_b)
    arr = (ctypes.c_int64 * 2)(0, n_b)
    nbytes = lib.sgs_cluster_collate_workspace_bytes(n_b)
    assert nbytes % 8 == 0
    ws, tot = Zoned(nbytes // 8, torch.int64, FILL), Zoned(1, torch.int64, FILL)
    _ok(lib, lib.sgs_cluster_collate_count(ptr.data_ptr(), col.data_ptr(), arr, 1, n_b, tot.ptr, ws.ptr, nbytes, None))
    assert int(tot.get()[0]) == ref["edge_index"].shape[1]
    assert np.array_equal(ws.get()[:n_b + 1], np.concatenate([[0], np.cumsum(np.bincount(ref["edge_index"][0], minlength=n_b))]))
