"""numpy reference of the neighbour-sampled batches (sgs_gnn_amd/data.py: ResidentGraph / NeighborLoader; csrc/neighbor.hip).  Everything is
integer arithmetic, so the device result is compared with this one by equality.  The kernel contracts (`select`, `frontier`, `induced`,
`directional`) and the batch built from them (`sample`, `make_batch`, `epoch_batches`) are restated here independently of the product; the
case tables at the end are shared by the CPU and the GPU tests."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_ref as PR  # noqa: E402

M32 = PR.M32
fmix32 = PR.fmix32
grid_graph, planted_graph = PR.grid_graph, PR.planted_graph
SUBGRAPH_TYPES = ("induced", "directional")
FANOUTS = (1, 2, 25, 64, 65, -1)
ROW_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257)
FRONTIER_SIZES = (0, 1, 3)            # and N


def stream_key(seed, epoch, batch, hop):
    """K(seed, epoch, batch, hop) = fmix32(hop + fmix32(batch + fmix32(epoch + fmix32(seed)))), additions modulo 2^32"""
    k = int(fmix32(np.uint64(int(seed) & 0xFFFFFFFF)))
    for t in (epoch, batch, hop):
        k = int(fmix32(np.uint64((int(t) + k) & 0xFFFFFFFF)))
    return k


def edge_keys(eid, K):
    return fmix32((np.asarray(eid).astype(np.int64).astype(np.uint64) & M32) ^ np.uint64(K))


# ---------------------------------------------------------------- the graph
def sort_edges(edge_index):
    """-> (the edge list sorted by (src, dst), stable; the order applied)"""
    ei = np.asarray(edge_index, dtype=np.int64)
    order = np.lexsort((ei[1], ei[0]))
    return np.ascontiguousarray(ei[:, order]), order


def csr_by(rows, other, N):
    """rows of `rows`, entries in ascending edge id -> (ptr int32 [N + 1], other int32 [E], eid int32 [E])"""
    order = np.argsort(rows, kind="stable")
    ptr = np.zeros(N + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    return ptr.astype(np.int32), other[order].astype(np.int32), order.astype(np.int32)


class Graph:
    """the sorted edge list and both CSRs, as ResidentGraph keeps them"""

    def __init__(self, edge_index, N):
        self.ei, self.order = sort_edges(edge_index)
        self.N, self.E = int(N), int(self.ei.shape[1])
        self.in_ptr, self.in_src, self.in_eid = csr_by(self.ei[1], self.ei[0], N)
        self.out_ptr, self.out_dst, self.out_eid = csr_by(self.ei[0], self.ei[1], N)


# ---------------------------------------------------------------- kernel contracts
def select(ptr, eid, N, rows, f, K):
    """-> (offs int64 [n_rows + 1], chosen int32): per frontier row min(f, deg) ids, the f smallest keys of a longer row, in row order"""
    out, offs = [], [0]
    for v in np.asarray(rows).tolist():
        ids = eid[ptr[v]:ptr[v + 1]] if 0 <= v < N else eid[:0]
        if f >= 0 and ids.shape[0] > f:
            keys = edge_keys(ids, K)
            ids = ids[keys <= np.sort(keys)[f - 1]][:f]
        out.append(ids)
        offs.append(offs[-1] + ids.shape[0])
    return np.asarray(offs, dtype=np.int64), (np.concatenate(out) if out else eid[:0]).astype(np.int32)


def frontier(chosen, src, E, N, member):
    """the sources of the chosen ids that are not members, ascending; `member` (bool [N]) is updated in place"""
    c = np.asarray(chosen, dtype=np.int64)
    c = c[(c >= 0) & (c < E)]
    u = np.asarray(src, dtype=np.int64)[c]
    u = u[(u >= 0) & (u < N)]
    new = np.unique(u[~member[u]])
    member[new] = True
    return new


def next_total(in_ptr, nodes, f):
    deg = np.diff(in_ptr.astype(np.int64))[nodes]
    return int(deg.sum() if f < 0 else np.minimum(deg, f).sum())


def induced(out_ptr, out_dst, out_eid, N, E, member):
    """-> (local edge_index [2, E_b], eid [E_b]): the out-CSR rows of the members ascending, entries with a member column kept in order"""
    nodes = np.nonzero(member)[0]
    loc = np.cumsum(member) - 1
    s, d, ids = [], [], []
    for r, v in enumerate(nodes.tolist()):
        c, e = out_dst[out_ptr[v]:out_ptr[v + 1]].astype(np.int64), out_eid[out_ptr[v]:out_ptr[v + 1]].astype(np.int64)
        ok = (c >= 0) & (c < N) & (e >= 0) & (e < E)
        ok[ok] = member[c[ok]]
        s.append(np.full(int(ok.sum()), r, dtype=np.int64))
        d.append(loc[c[ok]])
        ids.append(e[ok])
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, dtype=np.int64)  # noqa: E731
    return np.stack([cat(s), cat(d)]).astype(np.int64), cat(ids).astype(np.int64)


def directional(chosen_all, ei, E, N, member):
    """-> (local edge_index [2, m'], eid [m']): the chosen ids ascending; an id outside [0, E) or with an end outside the members is dropped"""
    c = np.sort(np.asarray(chosen_all, dtype=np.int64))
    c = c[(c >= 0) & (c < E)]
    a, b = ei[0][c], ei[1][c]
    ok = (a >= 0) & (a < N) & (b >= 0) & (b < N)
    ok[ok] = member[a[ok]] & member[b[ok]]
    c = c[ok]
    loc = np.cumsum(member) - 1
    return np.stack([loc[ei[0][c]], loc[ei[1][c]]]).astype(np.int64), c


# ---------------------------------------------------------------- one batch
def sample(g, seeds, fanouts, keys):
    """-> (member bool [N], hop_nodes, the chosen ids of every hop)"""
    seeds = np.asarray(seeds, dtype=np.int64)
    assert np.unique(seeds).shape[0] == seeds.shape[0]
    member = np.zeros(g.N, dtype=bool)
    member[seeds] = True
    front, hop_nodes, chosen = seeds, [int(seeds.shape[0])], []
    for f, K in zip(fanouts, keys):
        _, c = select(g.in_ptr, g.in_eid, g.N, front, f, K)
        chosen.append(c)
        front = frontier(c, g.ei[0], g.E, g.N, member)
        hop_nodes.append(int(front.shape[0]))
    return member, hop_nodes, chosen


def make_batch(g, data, seeds, fanouts, keys, subgraph_type="induced"):
    """`data`: dict(x, y, masks [3, N] bool, prob [E] in the SORTED edge order) -> the fields of the Batch as numpy arrays"""
    member, hop_nodes, chosen = sample(g, seeds, fanouts, keys)
    node_ids = np.nonzero(member)[0].astype(np.int64)
    if subgraph_type == "induced":
        ei, eid = induced(g.out_ptr, g.out_dst, g.out_eid, g.N, g.E, member)
    elif subgraph_type == "directional":
        ei, eid = directional(np.concatenate(chosen), g.ei, g.E, g.N, member)
    else:
        raise ValueError(subgraph_type)
    seed_mask = np.zeros(g.N, dtype=bool)
    seed_mask[np.asarray(seeds, dtype=np.int64)] = True
    seed_mask = seed_mask[node_ids]
    m = data["masks"][:, node_ids] & seed_mask[None, :]
    return dict(x=data["x"][node_ids], y=data["y"][node_ids], edge_index=ei, prob=data["prob"][eid], eid=eid, node_ids=node_ids,
                seed_mask=seed_mask, n_seeds=int(len(seeds)), hop_nodes=hop_nodes, train_mask=m[0], val_mask=m[1], test_mask=m[2])


def shuffle_seed(seed, epoch):
    return (int(seed) * 0x9E3779B1 + int(epoch)) % (1 << 63)


def epoch_seeds(input_ids, batch_size, shuffle, seed, epoch, drop_last=False):
    """the seed lists of one epoch: consecutive chunks of the (shuffled) input list"""
    import torch
    ids = np.asarray(input_ids, dtype=np.int64)
    if shuffle:
        ids = ids[torch.randperm(ids.shape[0], generator=torch.Generator().manual_seed(shuffle_seed(seed, epoch))).numpy()]
    out = [ids[i:i + batch_size] for i in range(0, ids.shape[0], batch_size)]
    if drop_last and out and out[-1].shape[0] < batch_size:
        out.pop()
    return out


def epoch_batches(g, data, input_ids, fanouts, batch_size, shuffle, seed, epoch, subgraph_type="induced", drop_last=False):
    return [make_batch(g, data, s, fanouts, [stream_key(seed, epoch, b, h) for h in range(len(fanouts))], subgraph_type)
            for b, s in enumerate(epoch_seeds(input_ids, batch_size, shuffle, seed, epoch, drop_last))]


# ---------------------------------------------------------------- data of the tests
def node_data(g, nfeat, ncls, seed):
    rng = np.random.default_rng(seed)
    r = rng.random(g.N)
    masks = np.stack([r < 0.5, (r >= 0.5) & (r < 0.75), r >= 0.75])
    return dict(x=rng.standard_normal((g.N, nfeat)).astype(np.float32), y=rng.integers(0, ncls, g.N).astype(np.int64), masks=masks,
                prob=(rng.random(g.E).astype(np.float32) + np.float32(0.5)) / np.float32(max(g.E, 1)))


def directed_graph(N, E, seed):
    """a directed multigraph with self loops: E uniform (src, dst) pairs as drawn"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N, E), rng.integers(0, N, E)]).astype(np.int64), N


def kernel_case(f, hub_row, seed):
    """A graph made for the kernels alone (directed, multi-edges and loops as they fall): node v has ROW_LENGTHS / f - 1, f, f + 1 / hub_row,
    hub_row + 1 / 0-20 in-edges from uniform sources; N = 131 is no multiple of the four waves of a workgroup.  -> (edge_index, N)"""
    rng = np.random.default_rng(seed)
    N = 131
    ff = f if f > 0 else 7
    lens = list(ROW_LENGTHS) + [max(ff - 1, 0), ff, ff + 1, hub_row, hub_row + 1]
    lens = np.asarray(lens + list(rng.integers(0, 21, N - len(lens))))[rng.permutation(N)]
    dst = np.repeat(np.arange(N), lens)
    return np.stack([rng.integers(0, N, dst.shape[0]), dst]).astype(np.int64), N


def kernel_frontiers(N, seed):
    rng = np.random.default_rng(seed)
    return [rng.permutation(N)[:k].astype(np.int32) for k in FRONTIER_SIZES] + [rng.permutation(N).astype(np.int32)]
