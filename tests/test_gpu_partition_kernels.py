"""GPU: sgs_lp_propose, sgs_lp_commit and sgs_partition_stats through the C ABI, outputs and the exactly sized workspace between red zones,
against tests/partition_ref.py by exact equality; then partition_graph end to end, phase by phase.  Kernel case table
(partition_ref.kernel_case): rows of 0, 1, 63, 64, 65, 256, 257, 512, 513 and 1025 entries, one hub row for the workgroup form, a row whose
neighbours all lie in one part, N = 259 / 4099 nodes (no multiple of the four waves of a workgroup), P in {1, 2, 64, 65, 4096}, both
eligibility rules, and every hand-made case of tests/test_partition_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_ref as R  # noqa: E402
from zoned import DEV, Zoned  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = -77777


@pytest.fixture(scope="module")
def lib():
    import sgs_gnn_amd as S
    return S._lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _propose(lib, ptr, col, part, P, mode, key, mingain):
    N = part.shape[0]
    d = [_dev(ptr), _dev(col), _dev(part)]
    best, gain = Zoned(N, torch.int32, FILL), Zoned(N, torch.int32, FILL)
    rc = lib.sgs_lp_propose(d[0].data_ptr(), d[1].data_ptr(), N, col.shape[0], P, d[2].data_ptr(), mode, key, mingain, best.ptr, gain.ptr, None)
    assert rc == 0, lib.sgs_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d[2].cpu().numpy(), part)                                  # inputs untouched
    return best.get().copy(), gain.get().copy()


def _commit(lib, best, gain, part, size, cap, lo):
    N, P = part.shape[0], size.shape[0]
    d = [_dev(best), _dev(gain)]
    zp, zs, zm = Zoned(N, torch.int32, FILL), Zoned(P, torch.int32, FILL), Zoned(1, torch.int32, FILL)
    zp.set(part.astype(np.int32))
    zs.set(size.astype(np.int32))
    nbytes = lib.sgs_lp_commit_workspace_bytes(N, P)
    assert nbytes % 8 == 0
    ws = Zoned(nbytes // 8, torch.int64, FILL)
    rc = lib.sgs_lp_commit(d[0].data_ptr(), d[1].data_ptr(), N, P, cap, lo, zp.ptr, zs.ptr, zm.ptr, ws.ptr, nbytes, None)
    assert rc == 0, lib.sgs_last_error()
    torch.cuda.synchronize()
    ws.get()                                                                         # the red zones around the workspace
    return zp.get().copy(), zs.get().copy(), int(zm.get()[0])


def _stats(lib, ptr, col, part, P):
    d = [_dev(ptr), _dev(col), _dev(part)]
    size, cut = Zoned(P, torch.int32, FILL), Zoned(1, torch.int64, FILL)
    rc = lib.sgs_partition_stats(d[0].data_ptr(), d[1].data_ptr(), part.shape[0], col.shape[0], P, d[2].data_ptr(), size.ptr, cut.ptr, None)
    assert rc == 0, lib.sgs_last_error()
    torch.cuda.synchronize()
    return size.get().copy(), int(cut.get()[0])


def _sweep_both(lib, ptr, col, part, P, mode, key, mingain, cap, lo):
    """one sweep on the device and in the reference from the same state -> the part vector after it"""
    elig = R.eligible(part, mode, key)
    want_b, want_g = R.propose(ptr, col, part, P, elig, mingain)
    best, gain = _propose(lib, ptr, col, part, P, mode, key, mingain)
    assert np.array_equal(best, want_b) and np.array_equal(gain, want_g)
    b2, g2 = _propose(lib, ptr, col, part, P, mode, key, mingain)                     # the same bits on a second call
    assert np.array_equal(b2, best) and np.array_equal(g2, gain)
    size = np.bincount(part[part >= 0], minlength=P).astype(np.int32)
    want_p, want_s = part.copy(), size.copy()
    want_m = R.commit(best, gain, want_p, want_s, cap, lo)
    got_p, got_s, got_m = _commit(lib, best, gain, part, size, cap, lo)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_s, want_s) and got_m == want_m
    return got_p, int((best >= 0).sum()), got_m


@pytest.mark.parametrize("P", R.PARTS)
def test_kernel_case_table(lib, P):
    hub = lib.sgs_lp_propose_hub_row()
    ptr, col, part = R.kernel_case(P, hub, seed=P)
    N = part.shape[0]
    assert N % 4 == 3 and int(np.diff(ptr).max()) > hub and set(R.ROW_LENGTHS + R.HELD_LENGTHS) <= set(np.diff(ptr).tolist())
    size = np.bincount(part[part >= 0], minlength=P)
    cap, lo = int(size.max()) + (1 if P <= 2 else 0), int(np.median(size))            # both sides of the commit bind
    proposals = moved = 0
    for mode, key, mingain, lo_s in ((R.ELIG_UNASSIGNED, 0, 1, 0), (R.ELIG_HASH, 5, 0, lo), (R.ELIG_HASH, 6, 1, lo), (R.ELIG_HASH, 2 ** 32 - 1, -3, 0)):
        after, np_, nm = _sweep_both(lib, ptr, col, part, P, mode, key, mingain, cap, lo_s)
        proposals, moved = proposals + np_, moved + nm
        got_size, got_cut = _stats(lib, ptr, col, after, P)
        want_size, want_cut = R.stats(ptr, col, after, P)
        assert np.array_equal(got_size, want_size) and got_cut == want_cut
    assert proposals > moved > 0                                                     # the limits did bind, and not everywhere


def test_hub_row_proposes_through_the_workgroup_form(lib):
    """the hub row of the case table is eligible under the key used, has a best part, and the one-wave rows beside it in its tile too"""
    hub = lib.sgs_lp_propose_hub_row()
    ptr, col, part = R.kernel_case(64, hub, seed=64)
    part = part.copy()
    part[4:8] = [3, -1, 7, 9]                                                        # tile 1 = rows 4-7: the hub (row 6) has a part of its own
    key = R.key_for([4, 5, 6, 7], part.shape[0])
    best, gain = _propose(lib, ptr, col, part, 64, R.ELIG_HASH, key, -10 ** 6)
    want_b, want_g = R.propose(ptr, col, part, 64, R.eligible(part, R.ELIG_HASH, key), -10 ** 6)
    assert np.array_equal(best, want_b) and np.array_equal(gain, want_g) and (best[4:8] >= 0).all() and best[6] != 7


@pytest.mark.parametrize("case", R.propose_cases(), ids=lambda c: c[0])
def test_propose_hand_cases(lib, case):
    _, ptr, col, part, P, mingain, node, want = case
    N = part.shape[0]
    modes = [(R.ELIG_HASH, R.key_for([node], N))] + ([(R.ELIG_UNASSIGNED, 0)] if part[node] < 0 else [])
    for mode, key in modes:
        best, gain = _propose(lib, ptr, col, part, P, mode, key, mingain)
        want_b, want_g = R.propose(ptr, col, part, P, R.eligible(part, mode, key), mingain)
        assert np.array_equal(best, want_b) and np.array_equal(gain, want_g)
        assert (int(best[node]), int(gain[node])) == want


@pytest.mark.parametrize("case", R.commit_cases(), ids=lambda c: c[0])
def test_commit_hand_cases(lib, case):
    _, best, gain, part, size, cap, lo, want = case
    got_p, got_s, got_m = _commit(lib, best, gain, part, size, cap, lo)
    assert np.array_equal(got_p, want) and got_m == int((want != part).sum())
    assert np.array_equal(got_s, np.bincount(want[want >= 0], minlength=size.shape[0]))


def test_gain_clamp_on_two_rows_of_a_million_entries(lib):
    ptr, col, part, size, cap, want = R.clamp_case()
    best, gain = _propose(lib, ptr, col, part, 2, R.ELIG_UNASSIGNED, 0, 1)
    assert list(best) == [-1, -1, 1, 1] and list(gain) == [0, 0, R.GMAX, R.GMAX + 6]
    got_p, got_s, got_m = _commit(lib, best, gain, part, size, cap, 0)
    assert np.array_equal(got_p, want) and list(got_s) == [1, 2] and got_m == 1


# ---------------------------------------------------------------- partition_graph, phase by phase
def _shapes():
    ei, N = R.grid_graph(64, 100)
    yield "grid", ei, N, 16
    ei, N, _ = R.planted_graph(4096, 8, 12, 3, 5)
    yield "planted", ei, N, 8
    ei, _ = R.grid_graph(9, 2)
    yield "N = 70, P = 64", ei[:, (ei < 70).all(0)], 70, 64


def _run_both(ei, N, P, **kw):
    import sgs_gnn_amd as S
    ptr, col = R.csr(ei, N)
    want_trace = []
    want, wrep = R.partition(ptr, col, P, trace=lambda phase, p: want_trace.append((phase, p.copy())), **kw)
    rep = {"trace": []}
    got = S.partition_graph(torch.from_numpy(ei).to(DEV), N, P, report=rep, **kw)
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == (N,)
    assert len(rep["trace"]) == len(want_trace)
    for (gp, gt), (wp, wt) in zip(rep["trace"], want_trace):
        assert gp == wp and np.array_equal(gt.cpu().numpy(), wt), gp                 # after grow, after fill, after every refinement sweep
    assert np.array_equal(got.cpu().numpy(), want)
    for k in ("cap", "grow_sweeps", "filled", "moved", "cut_edges", "cut_edges_initial"):
        assert rep[k] == wrep[k], k
    assert np.array_equal(rep["sizes"].cpu().numpy(), wrep["sizes"]) and rep["imbalance"] == wrep["imbalance"]
    return got, rep


@pytest.mark.parametrize("name,ei,N,P", list(_shapes()), ids=lambda v: v if isinstance(v, str) else "")
def test_partition_graph_equals_the_reference_after_every_phase(name, ei, N, P):
    _run_both(ei, N, P, hot=3, cold=2, seed=1)


def test_partition_graph_at_the_defaults_on_the_grid():
    ei, N = R.grid_graph(64, 100)
    _, rep = _run_both(ei, N, 16)
    assert rep["cut_edges"] <= 0.15 * ei.shape[1] and len(rep["moved"]) == 60


def test_init_refines_a_given_partition_and_is_validated():
    import sgs_gnn_amd as S
    ei, N = R.grid_graph(16, 7)
    init = R.hash_partition(N, 4, 9)
    ptr, col = R.csr(ei, N)
    want, wrep = R.partition(ptr, col, 4, hot=4, cold=2, seed=2, init=init)
    rep = {}
    d_ei = torch.from_numpy(ei).to(DEV)
    got = S.partition_graph(d_ei, N, 4, hot=4, cold=2, seed=2, init=torch.from_numpy(init).to(DEV), report=rep)
    assert np.array_equal(got.cpu().numpy(), want) and rep["cut_edges"] == wrep["cut_edges"] < wrep["cut_edges_initial"] == rep["cut_edges_initial"]
    for bad in (torch.full((N,), 4), torch.full((N,), -1), torch.zeros(N, dtype=torch.int64)):
        with pytest.raises(ValueError, match="init"):
            S.partition_graph(d_ei, N, 4, init=bad.to(DEV))
    with pytest.raises(ValueError, match="both ways"):
        S.partition_graph(d_ei[:, : ei.shape[1] // 2].contiguous(), N, 4)
    with pytest.raises(ValueError, match="num_parts"):
        S.partition_graph(d_ei, N, N + 1)


def test_ops_wrappers():
    import sgs_gnn_amd as S
    ptr, col, part = R.kernel_case(65, S._lib.lib().sgs_lp_propose_hub_row(), seed=3)
    d_ptr, d_col, d_part = _dev(ptr), _dev(col), _dev(part)
    best, gain = S.ops.lp_propose(d_ptr, d_col, d_part, 65, S.ops.LP_HASH, 12, 0)
    want_b, want_g = R.propose(ptr, col, part, 65, R.eligible(part, R.ELIG_HASH, 12), 0)
    assert np.array_equal(best.cpu().numpy(), want_b) and np.array_equal(gain.cpu().numpy(), want_g)
    size = np.bincount(part[part >= 0], minlength=65).astype(np.int32)
    d_size = _dev(size)
    moved = S.ops.lp_commit(best, gain, d_part, d_size, int(size.max()), 2)
    want_m = R.commit(want_b, want_g, part, size, int(size.max()), 2)
    assert int(moved.item()) == want_m > 0 and np.array_equal(d_part.cpu().numpy(), part) and np.array_equal(d_size.cpu().numpy(), size)
    got_size, got_cut = S.ops.partition_stats(d_ptr, d_col, d_part, 65)
    want_size, want_cut = R.stats(ptr, col, part, 65)
    assert np.array_equal(got_size.cpu().numpy(), want_size) and int(got_cut.item()) == want_cut
    with pytest.raises(RuntimeError, match="sgs_lp_propose"):
        S.ops.lp_propose(d_ptr, d_col, d_part, 5000, S.ops.LP_HASH)
