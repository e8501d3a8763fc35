"""GPU: sgs_cluster_collate through the C ABI (outputs between red zones) and ops.cluster_collate, against the loop restatement of
tests/cluster_collate_ref.py.  The graph is the smallest at which the kernels can still go wrong: ~2 600 nodes, ~31 000 directed
edges, 7 partitions of which one has no node, one has one node and one has no edge inside it, a hub joined to (almost) every node --
its row is longer than the 1024 columns one wave walks alone, so the workgroup-wide hub path runs --, 20 rows of degree 0, groups
whose batch has no edge, and k in {1, 2, 3, cap}."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cluster_collate_ref import collate_ref, full_csr_ref  # noqa: E402

pytestmark = pytest.mark.gpu
P, N = 7, 2600
SIZES = [700, 0, 1, 600, 50, 649, 600]          # partition 1: no node; 2: one node; 4: no edge inside it
GROUPS = [(0,), (4,), (1,), (2,), (0, 3), (1, 2), (0, 4), (0, 2, 5), (3, 4, 6), (1, 2, 4)]
NO_EDGE = {(4,), (1,), (2,), (1, 2), (1, 2, 4)}


def _graph():
    rng = np.random.default_rng(11)
    part = np.repeat(np.arange(P), SIZES)[rng.permutation(N)]
    hub = int(np.nonzero(part == 0)[0][12])               # new id 12: inside the second of the 32 ranges of the k = cap case
    lonely = np.nonzero(part == 5)[0][:20]                       # rows of degree 0
    quiet = np.zeros(N, dtype=bool)
    quiet[lonely] = True
    busy = np.nonzero(~quiet & (part != 4) & (np.arange(N) != hub))[0]
    a, b = rng.choice(busy, 14000), rng.choice(busy, 14000)
    others = np.nonzero(~quiet & (np.arange(N) != hub))[0]
    a, b = np.concatenate([a, np.full(others.shape, hub)]), np.concatenate([b, others])
    ok = a != b
    lo, hi = np.minimum(a[ok], b[ok]), np.maximum(a[ok], b[ok])
    keys = np.unique(np.concatenate([lo * N + hi, hi * N + lo]))
    ei = np.stack([keys // N, keys % N]).astype(np.int64)
    prob = rng.random(ei.shape[1], dtype=np.float32)
    masks = rng.integers(0, 2, (3, N)).astype(np.uint8)
    return dict(ei=ei, part=part, prob=prob, masks=masks, hub=hub, lonely=lonely)


@pytest.fixture(scope="module")
def G():
    """The graph, its partition-grouped CSR (numpy and device) and -- computed once, shared, never modified -- the reference batch of
    every range list the tests use, in the CSR's own numbering (eid = position in full_col)."""
    g = _graph()
    c = full_csr_ref(g["ei"], g["part"], P)
    assert g["ei"].shape[1] > 30000 and int(np.diff(c["full_ptr"]).max()) > 2500 and int((np.diff(c["full_ptr"]) == 0).sum()) == 20
    new_src = np.repeat(np.arange(N), np.diff(c["full_ptr"]))
    g.update(c, new_ei=np.stack([new_src, c["full_col"]]), csr_prob=g["prob"][c["order"]], csr_masks=np.ascontiguousarray(g["masks"][:, c["perm"]]))
    dev = "cuda:0"
    g["d"] = {k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("full_ptr", "full_col", "csr_prob", "csr_masks")}
    nptr = g["node_ptr"]
    cases = {grp: [(int(nptr[p]), int(nptr[p + 1])) for p in grp] for grp in GROUPS}
    # k = cap: 32 ascending ranges of 3 .. 80 nodes with gaps between them, across partition borders, the hub's node among them
    hub_new = int(np.nonzero(c["perm"] == g["hub"])[0][0])
    cap, at = 32, 0
    wide = []
    for j in range(cap):
        at += (7 * j) % 23
        wide.append((at, at + 3 + (11 * j) % 78))
        at = wide[-1][1]
    assert at <= N and any(lo <= hub_new < hi for lo, hi in wide)
    cases["cap"] = wide
    g["cases"], g["refs"] = cases, {}
    for name, ranges in cases.items():
        pseudo = np.full(N, len(ranges), dtype=np.int64)
        for j, (lo, hi) in enumerate(ranges):
            pseudo[lo:hi] = j
        g["refs"][name] = collate_ref(g["new_ei"], pseudo, range(len(ranges)), g["csr_prob"])
    return g


def _call(S, G, ranges, n_b, E_b, out, ws, prob=True, k=None):
    L = S._lib.lib()
    d = G["d"]
    flat = [v for r in ranges for v in r]
    arr = (ctypes.c_int64 * max(len(flat), 1))(*flat)
    return L.sgs_cluster_collate(d["full_ptr"].data_ptr(), d["full_col"].data_ptr(), d["csr_prob"].data_ptr() if prob else None, arr,
                                 len(ranges) if k is None else k, n_b, E_b, out["ei"].ptr, out["prob"].ptr if prob else None, out["eid"].ptr,
                                 d["csr_masks"].data_ptr(), out["attr"].ptr, 3, N, out["mis"].ptr, ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream)


def _outputs(n_b, E_b, shift=0):
    from zoned import Zoned
    return dict(ei=Zoned(2 * E_b, torch.int64, -7, shift), prob=Zoned(E_b, torch.float32, -1.0, shift), eid=Zoned(E_b, torch.int64, -7, shift),
                attr=Zoned(3 * n_b, torch.uint8, 9, shift), mis=Zoned(1, torch.int32, 0))


def _relabel(ranges, ids):
    out = np.full(ids.shape, -1, dtype=np.int64)
    at = 0
    for lo, hi in ranges:
        m = (ids >= lo) & (ids < hi)
        out[m] = ids[m] - lo + at
        at += hi - lo
    return out


@pytest.fixture(scope="module")
def S():
    import sgs_gnn_amd
    return sgs_gnn_amd


@pytest.mark.parametrize("name", GROUPS + ["cap"], ids=str)
def test_collate_matches_the_reference_between_red_zones(S, G, name):
    ranges, ref = G["cases"][name], G["refs"][name]
    n_b, E_b = int(ref["node_ids"].shape[0]), int(ref["edge_index"].shape[1])
    assert (E_b == 0) == (name in NO_EDGE)
    L = S._lib.lib()
    assert len(ranges) <= L.sgs_cluster_collate_max_parts()
    ws = torch.full((int(L.sgs_cluster_collate_workspace_bytes(n_b)),), 0xFF, dtype=torch.uint8, device="cuda:0")
    out = _outputs(n_b, E_b, shift=1 if name == "cap" else 0)
    assert _call(S, G, ranges, n_b, E_b, out, ws) == 0, L.sgs_last_error()
    torch.cuda.synchronize()
    got = {k: v.get().copy() for k, v in out.items()}                               # (get() also checks the red zones)
    assert int(got["mis"][0]) == 0
    assert np.array_equal(got["ei"].reshape(2, E_b), ref["edge_index"])
    assert np.array_equal(got["eid"], ref["eid"])
    assert np.array_equal(got["prob"].view(np.uint32), ref["prob"].view(np.uint32))
    assert np.array_equal(got["attr"].reshape(3, n_b), G["csr_masks"][:, ref["node_ids"]])
    # full_col[eid] relabelled reproduces the edge list, and so does the row that owns each position
    assert np.array_equal(_relabel(ranges, G["full_col"][got["eid"]]), got["ei"].reshape(2, E_b)[1])
    assert np.array_equal(_relabel(ranges, np.searchsorted(G["full_ptr"], got["eid"], side="right") - 1), got["ei"].reshape(2, E_b)[0])
    # a second call on the same (now used) workspace gives identical bytes
    out2 = _outputs(n_b, E_b, shift=1 if name == "cap" else 0)
    assert _call(S, G, ranges, n_b, E_b, out2, ws) == 0
    torch.cuda.synchronize()
    for k in out:
        assert np.array_equal(out2[k].get(), got[k]), k


def test_optional_outputs_and_the_count_entry(S, G):
    ranges, ref = G["cases"][(0, 3)], G["refs"][(0, 3)]
    n_b, E_b = int(ref["node_ids"].shape[0]), int(ref["edge_index"].shape[1])
    L = S._lib.lib()
    ws = torch.zeros(int(L.sgs_cluster_collate_workspace_bytes(n_b)), dtype=torch.uint8, device="cuda:0")
    d = G["d"]
    arr = (ctypes.c_int64 * (2 * len(ranges)))(*[v for r in ranges for v in r])
    ei = torch.full((2, E_b), -7, dtype=torch.int64, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    assert L.sgs_cluster_collate(d["full_ptr"].data_ptr(), d["full_col"].data_ptr(), None, arr, len(ranges), n_b, E_b, ei.data_ptr(), None, None,
                                 None, None, 0, N, None, ws.data_ptr(), ws.numel(), st) == 0, L.sgs_last_error()
    total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    assert L.sgs_cluster_collate_count(d["full_ptr"].data_ptr(), d["full_col"].data_ptr(), arr, len(ranges), n_b, total.data_ptr(), ws.data_ptr(),
                                       ws.numel(), st) == 0, L.sgs_last_error()
    assert np.array_equal(ei.cpu().numpy(), ref["edge_index"]) and int(total.item()) == E_b


def test_mismatch_word_and_red_zones_when_E_b_is_one_too_small(S, G):
    for name in [(0, 3), "cap"]:                                                   # a hub row written by the workgroup path in both
        ranges, ref = G["cases"][name], G["refs"][name]
        n_b, E_b = int(ref["node_ids"].shape[0]), int(ref["edge_index"].shape[1]) - 1
        L = S._lib.lib()
        ws = torch.zeros(int(L.sgs_cluster_collate_workspace_bytes(n_b)), dtype=torch.uint8, device="cuda:0")
        out = _outputs(n_b, E_b)
        assert _call(S, G, ranges, n_b, E_b, out, ws) == 0, L.sgs_last_error()
        torch.cuda.synchronize()
        got = {k: v.get() for k, v in out.items()}                                  # red zones intact
        assert int(got["mis"][0]) == 1
        assert np.array_equal(got["ei"].reshape(2, E_b), ref["edge_index"][:, :E_b]) and np.array_equal(got["eid"], ref["eid"][:E_b])


def test_error_channel(S, G):
    L = S._lib.lib()
    cap = L.sgs_cluster_collate_max_parts()
    assert cap >= 16
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    small = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    out = _outputs(32, 8)
    bad = [([], 0, ws, b"k = 0"), ([(0, 1)] * (cap + 1), cap + 1, ws, b"must be in"), ([(10, 20), (0, 5)], 15, ws, b"ascending"),
           ([(0, 10), (9, 20)], 21, ws, b"overlap"), ([(0, 10), (10, 20)], 19, ws, b"n_b"), ([(0, 10), (10, 20)], 20, small, b"workspace too small")]
    for ranges, n_b, w, msg in bad:
        assert _call(S, G, ranges, n_b, 8, out, w) == -1 and msg in L.sgs_last_error(), msg
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((torch.from_numpy(v.get()) == v.fill).all()), k                  # a refused call writes nothing


def test_op_builds_the_reference_batch(S, G):
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((N, 6)).astype(np.float32))
    y = torch.arange(N) % 5
    m = torch.from_numpy(G["masks"]).bool()
    rp = S.ResidentPartitions(x, torch.from_numpy(G["ei"]), y, m[0], m[1], m[2], torch.from_numpy(G["part"]), num_parts=P, device="cuda:0",
                              prob=torch.from_numpy(G["prob"]), keep_cut_edges=True)
    assert rp.size_path == "table"
    for grp in [(0, 3), (1, 2), (4,), (0, 2, 5)]:
        bt = S.ops.cluster_collate(rp, grp[::-1], want_eid=True)                    # (drawn in any order: taken ascending)
        ref = collate_ref(G["ei"], G["part"], grp, G["prob"])
        ids = torch.from_numpy(ref["node_ids"])
        assert bt.parts == grp and torch.equal(bt.node_ids.cpu(), ids)
        assert np.array_equal(bt.edge_index.cpu().numpy(), ref["edge_index"])
        assert np.array_equal(bt.prob.cpu().numpy().view(np.uint32), ref["prob"].view(np.uint32))
        assert np.array_equal(G["order"][bt.eid.cpu().numpy()], ref["eid"])
        assert torch.equal(bt.x.cpu(), x[ids]) and torch.equal(bt.y.cpu(), y[ids]) and bt.restored_edges == ref["restored"]
        for i, k in enumerate(("train_mask", "val_mask", "test_mask")):
            assert getattr(bt, k).dtype == torch.bool and torch.equal(getattr(bt, k).cpu(), m[i][ids])
    assert int(rp.collate_mismatch.item()) == 0
    cpu = S.ResidentPartitions(x, torch.from_numpy(G["ei"]), y, m[0], m[1], m[2], torch.from_numpy(G["part"]), num_parts=P, device="cpu",
                               keep_cut_edges=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.cluster_collate(cpu, (0, 3))
