"""A frozen copy of the node-block arithmetic as it stood inside `sharded.NodeBlocks.__init__` before it became the pure function
`sharded.block_layout`.  Kept verbatim apart from reading `firsts` / `N` from arguments instead of the all-gathered tensors and the
shard; `block_layout` is held to it over a sweep of source-sorted edge lists (tests/test_sharded_layout_cpu.py).  Do not edit."""


def node_blocks_frozen(firsts, N, rank, world):
    nb = [int(f) for f in firsts]
    nb[0] = 0
    for r in range(len(nb) - 2, -1, -1):              # an empty shard owns nothing: its block collapses onto the next one's start
        nb[r] = min(nb[r], nb[r + 1])
    nb[0] = 0
    nb = nb + [N]
    lo, hi = nb[rank], nb[rank + 1]
    size = [nb[r + 1] - nb[r] for r in range(world)]
    # owner of node `hi` = the next rank with a non-empty block (a hub whose edges fill whole shards leaves empty blocks between)
    halo_owner = next((r for r in range(rank + 1, world) if size[r] > 0), None) if hi < N else None
    halo = 0 if halo_owner is None else 1
    halo_users = [r for r in range(rank) if size[rank] > 0 and nb[r + 1] == lo
                  and next((k for k in range(r + 1, world) if size[k] > 0), None) == rank]
    return nb, lo, hi, halo_owner, halo, halo_users
