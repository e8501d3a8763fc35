"""CPU: the node-block arithmetic of the sharded trainers (`sharded.block_layout`: empty shards, empty blocks behind a hub, halo owner,
halo users) -- equal to the frozen copy of the code it was lifted from (tests/sharded_layout_ref.py) on every rank, and four invariants
checked by brute force, over a seeded sweep of source-sorted edge lists cut by `shard_bounds`.  No process group, no GPU."""
import functools
import random
from importlib import import_module

import pytest

import sharded_layout_ref as REF

LISTS = 5000


@pytest.fixture(scope="module")
def sh():
    import __graft_entry__ as ge
    ge.build()
    return import_module("sgs_gnn_amd.sharded")


@functools.lru_cache(maxsize=None)
def _sweep(shard_bounds):
    """(N, world, src, bounds, firsts) per list: N 1-12, E 0-40, world 1-5, chunk 1, 2 or 4; half of the lists (N > 1) get a hub source
    with up to E out-edges of its own."""
    rnd = random.Random(1)
    cases = []
    for _ in range(LISTS):
        N, world, chunk, E = rnd.randint(1, 12), rnd.randint(1, 5), rnd.choice([1, 2, 4]), rnd.randint(0, 40)
        src = [rnd.randrange(N) for _ in range(E)]
        if rnd.random() < 0.5 and N > 1 and E:
            src = ([rnd.randrange(N)] * rnd.randint(0, E) + src)[:E]
        src.sort()
        b = shard_bounds(E, world, chunk)
        firsts = [src[b[r]] if b[r + 1] > b[r] else N for r in range(world)]         # what NodeBlocks all-gathers: N for a shard without edges
        cases.append((N, world, src, b, firsts))
    return cases


def test_block_layout_equals_the_frozen_copy_on_every_rank(sh):
    seen = dict(empty_shard=0, empty_block=0, halo=0)
    for N, world, src, b, firsts in _sweep(sh.shard_bounds):
        for rank in range(world):
            got = sh.block_layout(list(firsts), N, rank, world)
            want = REF.node_blocks_frozen(list(firsts), N, rank, world)
            assert tuple(got) == tuple(want), (N, world, src, b, rank)
            nb, lo, hi, _, halo, _ = want
            if b[rank + 1] == b[rank]:
                seen["empty_shard"] += 1
            elif hi == lo:
                seen["empty_block"] += 1                 # a shard with edges, all of them inside a hub's row that an earlier rank owns
            seen["halo"] += halo
    # the sweep reaches every corner the arithmetic has (a sweep of this shape holds thousands of each)
    assert min(seen.values()) >= 1000, seen


def test_block_layout_invariants_by_brute_force(sh):
    for N, world, src, b, firsts in _sweep(sh.shard_bounds):
        L = [sh.block_layout(list(firsts), N, r, world) for r in range(world)]
        nb = L[0][0]
        why = (N, world, src, b)
        # 1. nb is non-decreasing from 0 to N, and every rank sees the same one
        assert nb[0] == 0 and nb[-1] == N and len(nb) == world + 1 and all(nb[i] <= nb[i + 1] for i in range(world)), why
        assert all(l[0] == nb for l in L), why
        for r in range(world):
            _, lo, hi, owner, halo, users = L[r]
            assert (lo, hi) == (nb[r], nb[r + 1]) and halo == (0 if owner is None else 1), why
            # 2. every source in the rank's shard lies in [lo, hi), or equals hi with halo == 1
            assert all(lo <= s < hi or (halo == 1 and s == hi) for s in src[b[r]:b[r + 1]]), (why, r)
            # 3. a halo owner's block starts at that hi and is non-empty
            if halo:
                assert L[owner][1] == hi and L[owner][2] > L[owner][1], (why, r)
            # 4. r in halo_users of rank k exactly when rank r has halo == 1 and halo_owner == k
            for k in range(world):
                assert (r in L[k][5]) == (halo == 1 and owner == k), (why, r, k)
