"""CPU: the partitioner's numpy reference (tests/partition_ref.py) rule by rule on hand-made cases, its invariants, the quality it reaches
on two small graphs -- the device path is held to the same figures by equality (tests/test_gpu_partition_kernels.py) -- and the C ABI's
host-only side: workspace query and argument errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_ref as R  # noqa: E402

SEEDS = (0, 1, 2, 3)


def test_hash_is_murmur3_finaliser():
    assert [int(x) for x in R.fmix32(np.asarray([0, 1, 0xFFFFFFFF]))] == [0, 0x514E28B7, 0x81F16F39]
    assert int(R.H(5, 9)) == int(R.fmix32(5 ^ int(R.fmix32(9))))


@pytest.mark.parametrize("case", R.propose_cases(), ids=lambda c: c[0])
def test_propose_rules(case):
    _, ptr, col, part, P, mingain, node, want = case
    best, gain = R.propose(ptr, col, part, P, np.ones(part.shape[0], dtype=bool), mingain)
    assert (int(best[node]), int(gain[node])) == want
    none, zero = R.propose(ptr, col, part, P, np.zeros(part.shape[0], dtype=bool), mingain)
    assert (none == -1).all() and (zero == 0).all()                      # nobody eligible, nothing proposed


@pytest.mark.parametrize("case", R.commit_cases(), ids=lambda c: c[0])
def test_commit_rules(case):
    _, best, gain, part, size, cap, lo, want = case
    part, size = part.copy(), size.copy()
    moved = R.commit(best, gain, part, size, cap, lo)
    assert np.array_equal(part, want) and moved == int((want != case[3]).sum())
    assert np.array_equal(size, np.bincount(want[want >= 0], minlength=size.shape[0]))


def test_gain_is_clamped_to_twenty_bits():
    ptr, col, part, size, cap, want = R.clamp_case()
    best, gain = R.propose(ptr, col, part, 2, part < 0, 1)
    assert list(best) == [-1, -1, 1, 1] and list(gain) == [0, 0, R.GMAX, R.GMAX + 6]
    assert R.commit(best, gain, part, size, cap, 0) == 1 and np.array_equal(part, want)


def test_fill_order_and_seeding_of_isolated_nodes():
    ptr, col = np.zeros(8, dtype=np.int32), np.zeros(0, dtype=np.int32)            # seven nodes, no edge
    part, rep = R.partition(ptr, col, 2, eps=0.0, hot=2, cold=1, seed=3)
    order = np.lexsort((np.arange(7), R.H(np.arange(7), 3)))
    want = np.full(7, -1)
    want[order[:2]] = [0, 1]
    left = np.nonzero(want < 0)[0]
    want[left] = [0, 0, 0, 1, 1]                                                    # base = 4: three more for part 0, then part 1's (one slot unused)
    assert np.array_equal(part, want) and rep["filled"] == 5 and rep["grow_sweeps"] == 1 and rep["cut_edges"] == 0
    # isolated nodes seed last: with one edge in the graph its two ends are the seeds whatever their hashes
    ei = R.both_ways([5], [2])
    ptr, col = R.csr(ei, 7)
    assert sorted(R.seed_nodes(ptr, col, 2, 11)) == [2, 5]


def test_one_part():
    ei, N = R.grid_graph(5, 1)
    ptr, col = R.csr(ei, N)
    part, rep = R.partition(ptr, col, 1, hot=2, cold=1)
    assert (part == 0).all() and rep["cut_edges"] == 0 and rep["moved"] == [0, 0, 0] and rep["cap"] >= N


def test_init_validation():
    ei, N = R.grid_graph(4, 1)
    ptr, col = R.csr(ei, N)
    for bad in (np.full(N, 2), np.full(N, -1), np.zeros(N, dtype=np.int64)):        # out of range twice; every node in part 0 of 2
        with pytest.raises(ValueError):
            R.partition(ptr, col, 2, init=bad)
    init = np.arange(N) % 2
    part, rep = R.partition(ptr, col, 2, hot=3, cold=2, init=init)
    assert rep["cut_edges"] <= rep["cut_edges_initial"] and rep["grow_sweeps"] == 0


def _graphs():
    ei, N = R.grid_graph(16, 7)
    yield "grid", ei, N, 5
    ei, N, _ = R.planted_graph(512, 4, 6, 2, 3)
    yield "planted", ei, N, 4
    ei, N = R.grid_graph(9, 2)
    yield "N = 70ish, many parts", ei[:, (ei < 70).all(0)], 70, 64


@pytest.mark.parametrize("name,ei,N,P", list(_graphs()), ids=lambda v: v if isinstance(v, str) else "")
def test_invariants(name, ei, N, P):
    ptr, col = R.csr(ei, N)
    cap = R.bounds(N, P, 0.05)[0]
    seen = []

    def trace(phase, part):
        size = np.bincount(part[part >= 0], minlength=P)
        assert size.max() <= cap, phase
        assert phase == "grow" or (part >= 0).all()
        seen.append(part.copy())
    part, rep = R.partition(ptr, col, P, hot=6, cold=3, seed=1, trace=trace)
    assert len(seen) == 2 + 9 and (part >= 0).all() and (part < P).all() and np.array_equal(seen[-1], part)
    again, _ = R.partition(ptr, col, P, hot=6, cold=3, seed=1)
    other, _ = R.partition(ptr, col, P, hot=6, cold=3, seed=2)
    assert np.array_equal(again, part) and not np.array_equal(other, part)
    assert rep["imbalance"] <= cap * P / N and rep["sizes"].sum() == N


@pytest.fixture(scope="module")
def grid64():
    ei, N = R.grid_graph(64, 100)
    return R.csr(ei, N), ei.shape[1], N


@pytest.mark.parametrize("seed", SEEDS)
def test_quality_grid(grid64, seed):
    """Shuffled-id 64 x 64 grid, P = 16, eps = 0.05, defaults: the cut is at most 0.15 E (a hash partition: 0.94 E)."""
    (ptr, col), E, N = grid64
    part, rep = R.partition(ptr, col, 16, seed=seed)
    print(f"grid seed {seed}: cut {rep['cut_edges'] / E:.4f} E after refinement, {rep['cut_edges_initial'] / E:.4f} E before")
    assert rep["cut_edges"] <= 0.15 * E
    assert R.stats(ptr, col, R.hash_partition(N, 16, seed), 16)[1] > 0.9 * E


@pytest.fixture(scope="module")
def planted():
    ei, N, truth = R.planted_graph(4096, 8, 12, 3, 5)
    return R.csr(ei, N), ei.shape[1], N, truth


@pytest.mark.parametrize("seed", SEEDS)
def test_quality_planted(planted, seed):
    """Planted partition, N = 4096, 8 communities, 12 intra and 3 random inter edges per node: the cut never rises from grow + fill to the
    end and ends below 0.5 E (planted: 0.18 E, hash partition: 0.87 E)."""
    (ptr, col), E, N, truth = planted
    cuts = []
    part, rep = R.partition(ptr, col, 8, seed=seed, trace=lambda phase, p: cuts.append(R.stats(ptr, col, p, 8)[1]))
    cuts = cuts[1:]                                                                 # from "fill" on
    print(f"planted seed {seed}: cut {cuts[0] / E:.4f} E -> {cuts[-1] / E:.4f} E")
    assert cuts[0] == rep["cut_edges_initial"] and cuts[-1] == rep["cut_edges"]
    assert all(b <= a for a, b in zip(cuts, cuts[1:]))
    assert rep["cut_edges"] < 0.5 * E
    assert 0.17 * E < R.stats(ptr, col, truth, 8)[1] < 0.19 * E and R.stats(ptr, col, R.hash_partition(N, 8, seed), 8)[1] > 0.85 * E


# ---------------------------------------------------------------- C ABI, host-only side
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    return sgs_gnn_amd._lib.lib()


def test_workspace_query_runs_without_a_gpu(lib):
    small, big = lib.sgs_lp_commit_workspace_bytes(1000, 16), lib.sgs_lp_commit_workspace_bytes(1 << 20, 4096)
    assert small >= 3 * 8 * 1000 + 1000 and big >= 3 * 8 * (1 << 20) + (1 << 20) and big > small
    assert lib.sgs_lp_commit_workspace_bytes(-1, 16) == lib.sgs_lp_commit_workspace_bytes(1000, 0) == 256
    assert lib.sgs_lp_propose_hub_row() >= 1025                                      # the GPU case table's rows up to 1025 stay one-wave rows


@pytest.mark.parametrize("N,nnz,P,word", [(100, 50, 0, b"outside [1, 4096]"), (10000, 50, 4097, b"outside [1, 4096]"), (3, 2, 5, b"P <= N"),
                                          (-1, 0, 1, b"bad sizes"), (10, -4, 2, b"bad sizes")])
def test_argument_errors_report_through_the_error_channel(lib, N, nnz, P, word):
    assert lib.sgs_lp_propose(None, None, N, nnz, P, None, 0, 0, 1, None, None, None) == -1
    assert b"sgs_lp_propose" in lib.sgs_last_error() and word in lib.sgs_last_error()
    assert lib.sgs_partition_stats(None, None, N, nnz, P, None, None, None, None) == -1
    assert b"sgs_partition_stats" in lib.sgs_last_error() and word in lib.sgs_last_error()
    if nnz >= 0:
        assert lib.sgs_lp_commit(None, None, N, P, 10, 1, None, None, None, None, 0, None) == -1
        assert b"sgs_lp_commit" in lib.sgs_last_error() and word in lib.sgs_last_error()


def test_wrappers_have_no_cpu_fallback(lib):
    import torch
    import sgs_gnn_amd as S
    ptr, col, part = torch.zeros(5, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.lp_propose(ptr, col, part, 2, S.ops.LP_HASH)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.lp_commit(part, part, part, torch.zeros(2, dtype=torch.int32), 4, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.partition_stats(ptr, col, part, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.partition_graph(torch.zeros(2, 0, dtype=torch.int64), 4, 2)
