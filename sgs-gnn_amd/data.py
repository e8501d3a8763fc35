"""Batch duck-type of the reference's loaders (PyG `Data` as ClusterLoader yields it: .x, .edge_index,
.y, .train_mask/.val_mask/.test_mask, .prob, .to(device)) and seeded synthetic look-alikes of the
benchmark graphs: real datasets cannot be fetched offline."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


class Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def num_nodes(self):
        return self.x.shape[0]

    def to(self, device):
        dev = torch.device(device)
        if self.x.device == dev or (dev.type == "cuda" and self.x.is_cuda and dev.index in (None, self.x.device.index)):
            return self
        out = Batch(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in self.__dict__.items() if not k.startswith("_sgs")})
        return out


def degree_prior(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """`data.prob` of datasets.py:141-156 (add_degree) for a row-sorted edge_index:
    softmax_e( E^-1/2 / (colcount[row_e] + rowcount[col_e] + 1e-10) )."""
    row, col = edge_index[0], edge_index[1]
    E = edge_index.shape[1]
    rowcount = torch.bincount(row, minlength=num_nodes).to(torch.float32)
    colcount = torch.bincount(col, minlength=num_nodes).to(torch.float32)
    prob = 1.0 / ((colcount[row] + rowcount[col]) + 1e-10)
    return F.softmax(prob * E ** -0.5, dim=0)


def batch_prior(global_prob, index, edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """The `prob` of a batch with the row-sorted local edge list `edge_index`: `global_prob[index]` where a whole-graph prior exists
    (prior="global"), else the degree prior of the batch's own edge list (prior="local") -- ops.degree_prior on a HIP device, the torch
    composition above on the CPU and for an empty edge list."""
    if global_prob is not None:
        return global_prob[index].contiguous()
    if edge_index.is_cuda and edge_index.shape[1] > 0:
        from . import ops
        return ops.degree_prior(edge_index, num_nodes)
    return degree_prior(edge_index, num_nodes)


def synthetic_graph(n: int, n_edges_target: int, nfeat: int, ncls: int, seed: int, train_frac: float = 0.66,
                    power: float = 0.8, device="cpu") -> Batch:
    """Undirected, loop-free, coalesced, row-sorted degree-corrected random graph with power-law
    expected degrees (both directions stored), N(0,1) features with a weak class signal, uniform
    labels, Bernoulli masks and the reference's degree prior."""
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed)
    kw = dict(generator=g, device=dev)
    wts = (torch.arange(1, n + 1, dtype=torch.float32, device=dev) ** (-power))
    wts = wts[torch.randperm(n, **kw)]
    m = n_edges_target // 2
    max_pairs = n * (n - 1) // 2
    m = min(m, int(max_pairs * 0.9))
    keys = torch.zeros(0, dtype=torch.int64, device=dev)
    while keys.numel() < m:                       # draw endpoint pairs ~ w_i w_j, dedupe, repeat
        need = int((m - keys.numel()) * 1.3) + 16
        a = torch.multinomial(wts, need, replacement=True, generator=g)
        b = torch.multinomial(wts, need, replacement=True, generator=g)
        a, b = a.to(torch.int64), b.to(torch.int64)
        ok = a != b
        lo, hi = torch.minimum(a[ok], b[ok]), torch.maximum(a[ok], b[ok])
        keys = torch.unique(torch.cat([keys, lo * n + hi]))
    keys = keys[torch.randperm(keys.numel(), **kw)[:m]]
    lo, hi = keys // n, keys % n
    both = torch.unique(torch.cat([lo * n + hi, hi * n + lo]))       # sorted -> row-sorted, coalesced
    ei = torch.stack([both // n, both % n])
    y = torch.randint(0, ncls, (n,), **kw)
    x = torch.randn(n, nfeat, **kw)
    x[torch.arange(n, device=dev), y % nfeat] += 1.5
    r = torch.rand(n, **kw)
    tm = r < train_frac
    vm = (r >= train_frac) & (r < train_frac + (1 - train_frac) * 0.3)
    return Batch(x=x, edge_index=ei, y=y, train_mask=tm, val_mask=vm, test_mask=~(tm | vm), prob=degree_prior(ei, n))


def reddit_partition_stream(num_parts: int = 230, seed: int = 42, nfeat: int = 602, ncls: int = 41, n: int = 1013,
                            e_lo: int = 60_000, e_hi: int = 500_000, frac_above_q: float = 0.52, q: int = 100_000,
                            device="cpu", only=None):
    """S3 of SURVEY.md section 8d: a Reddit-like METIS partition stream -- `num_parts` batches of
    ~1013 nodes whose intra-partition edge counts mirror the reference run (119 of 230 partitions
    exceed q = 100 000; logs/pipeline_hybrid.log:8).  `only` (a set of indices): build just those partitions, None elsewhere."""
    sizes = reddit_partition_sizes(num_parts, seed, e_lo, e_hi, frac_above_q, q)
    return [synthetic_graph(n, E, nfeat, ncls, seed * 1000 + i, device=device) if only is None or i in only else None
            for i, E in enumerate(sizes)]


def reddit_partition_sizes(num_parts: int = 230, seed: int = 42, e_lo: int = 60_000, e_hi: int = 500_000, frac_above_q: float = 0.52,
                           q: int = 100_000):
    """Edge counts of `reddit_partition_stream`'s partitions (same seed -> same list), without building them."""
    g = torch.Generator().manual_seed(seed)
    sizes = []
    for i in range(num_parts):
        # deterministic interleave: every prefix of the stream has ~frac_above_q of its partitions above q
        above = int((i + 1) * frac_above_q) > int(i * frac_above_q)
        lo, hi = (int(q * 1.02), e_hi) if above else (e_lo, int(q * 0.98))
        sizes.append(int(lo + (hi - lo) * float(torch.rand(1, generator=g))))
    return sizes


class ResidentPartitions:
    """All partitions of one graph resident in HBM: the device-side counterpart of the reference's
    `ClusterData(data, num_parts)` + `ClusterLoader(cluster_data, batch_size=1, shuffle=True)` (main.py:63-65; SURVEY.md
    section 8f item 2).  The reference re-slices every batch on the CPU and copies it to the GPU each time it is visited;
    here the partitioning is applied ONCE on the device and iteration yields `Batch` objects whose tensors never move again --
    which is also what the HIP-graph replay of the step needs (captures are keyed on the batch tensors' addresses).  The node ->
    partition vector `part_id` is the caller's (METIS run on the host, or any other partitioner) or the project's own:
    `ResidentPartitions.from_graph` computes it on the device with `partition_graph` (partition.py: balanced k-way label
    propagation; single level, so its cuts are honest but not METIS-grade).

    Semantics follow ClusterData: partition p holds the nodes with part_id == p (in ascending original id), the edges with
    BOTH endpoints in p (relabelled, row-sorted), the node attributes x / y / masks, and the edge attribute `prob` sliced
    from the full graph's prior (`prior="global"`, what the reference does: add_degree runs before partitioning,
    datasets.py:141-156) or recomputed on the partition (`prior="local"`)."""

    CUT_TABLE_MAX_PARTS = 2048       # the P x P block edge-count table is kept up to here (32 MiB of int64 on the host)

    def __init__(self, x, edge_index, y, train_mask, val_mask, test_mask, part_id, num_parts=None, device="cuda:0", prior="global",
                 prob=None, shuffle=False, seed=0, *, keep_cut_edges=False):
        """`keep_cut_edges=True` additionally keeps the WHOLE graph in the permuted node order (a row-sorted CSR `full_ptr` /
        `full_col` over all E edges, `full_prob`, the node attributes) and the host-side tables `ResidentClusterLoader` needs to
        build batches of several partitions with the edges between them restored."""
        dev = torch.device(device)
        part_id = part_id.to(dev).to(torch.int64)
        N = x.shape[0]
        if part_id.numel() != N:
            raise ValueError("part_id must have one entry per node")
        P = int(num_parts) if num_parts is not None else int(part_id.max()) + 1
        ei = edge_index.to(dev)
        E = ei.shape[1]
        if prob is None and prior == "global":
            if dev.type == "cuda":
                from . import ops
                # the device op wants a row-sorted edge list (CSR build); sort a copy and scatter the prior back
                order = torch.argsort(ei[0] * N + ei[1])
                p_sorted = ops.degree_prior(ei[:, order].contiguous(), N)
                prob = torch.empty_like(p_sorted)
                prob[order] = p_sorted
            else:
                prob = degree_prior(ei, N)
        elif prob is not None:
            prob = prob.to(dev)
        # nodes grouped by partition (stable: ascending original id inside a partition)
        perm = torch.argsort(part_id, stable=True)
        counts = torch.bincount(part_id, minlength=P)
        nptr = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        nptr[1:] = torch.cumsum(counts, 0)
        new_id = torch.empty(N, dtype=torch.int64, device=dev)
        new_id[perm] = torch.arange(N, device=dev)
        # intra-partition edges, relabelled, sorted by (partition, new src, new dst)
        ps, pd = part_id[ei[0]], part_id[ei[1]]
        keep = ps == pd
        src, dst, pe = new_id[ei[0][keep]], new_id[ei[1][keep]], ps[keep]
        order = torch.argsort(src * N + dst)            # new ids are grouped by partition, so this sorts by (p, src, dst)
        src, dst, pe = src[order], dst[order], pe[order]
        eprob = prob[keep][order] if prob is not None else None
        ecounts = torch.bincount(pe, minlength=P)
        eptr = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        eptr[1:] = torch.cumsum(ecounts, 0)
        xs, ys = x.to(dev)[perm], y.to(dev)[perm]
        tm, vm, sm = train_mask.to(dev)[perm], val_mask.to(dev)[perm], test_mask.to(dev)[perm]
        nptr_h, eptr_h = nptr.tolist(), eptr.tolist()    # one read-back at construction time
        self.num_parts, self.perm, self.node_ptr, self.edge_ptr = P, perm, nptr, eptr
        self.dropped_edges = int(E - int(keep.sum()))    # inter-partition edges (ClusterLoader with batch_size=1 drops them too)
        self.batches = []
        for p in range(P):
            a, b, ea, eb = nptr_h[p], nptr_h[p + 1], eptr_h[p], eptr_h[p + 1]
            lei = torch.stack([src[ea:eb] - a, dst[ea:eb] - a]).contiguous()
            bp = batch_prior(eprob, slice(ea, eb), lei, b - a)
            self.batches.append(Batch(x=xs[a:b].contiguous(), edge_index=lei, y=ys[a:b].contiguous(), train_mask=tm[a:b].contiguous(),
                                      val_mask=vm[a:b].contiguous(), test_mask=sm[a:b].contiguous(), prob=bp, part=p,
                                      node_ids=perm[a:b]))
        self.shuffle = shuffle
        self._gen = torch.Generator().manual_seed(seed)
        self.keep_cut_edges = bool(keep_cut_edges)
        if keep_cut_edges:
            fs, fd = new_id[ei[0]], new_id[ei[1]]
            forder = torch.argsort(fs * N + fd)
            fptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
            fptr[1:] = torch.cumsum(torch.bincount(fs, minlength=N), 0)
            self.full_ptr, self.full_col = fptr, fd[forder].contiguous()
            self.full_prob = prob[forder].contiguous() if prob is not None else None      # None: prior="local", recomputed per batch
            self.x_all, self.y_all = xs.contiguous(), ys.contiguous()
            self.masks_all = torch.stack([tm, vm, sm]).to(torch.uint8).contiguous()       # [3, N] bytes: train / val / test
            self.num_nodes, self.num_edges = N, E
            self.node_ptr_host, self.edge_ptr_host = nptr_h, eptr_h
            # E_b of any group without a read-back: edges between every pair of partitions, counted once (one read-back here)
            self.size_path = "table" if P <= self.CUT_TABLE_MAX_PARTS else "readback"
            self.block_edges = torch.bincount(ps * P + pd, minlength=P * P).view(P, P).cpu() if self.size_path == "table" else None
            self.collate_mismatch = torch.zeros(1, dtype=torch.int32, device=dev)         # set by the device collate if its count != E_b

    @classmethod
    def from_graph(cls, x, edge_index, y, train_mask, val_mask, test_mask, num_parts, *, partition=None, **kw):
        """`partition_graph(edge_index, N, num_parts, **partition)` on the constructor's device, then the constructor with its result:
        a raw undirected `edge_index` (stored both ways) in, resident partitions out.  `partition`: keyword arguments of
        `partition_graph` (eps, hot, cold, seed, init, report); `kw`: the constructor's.  The vector is kept as `part_id`."""
        from .partition import partition_graph
        dev = torch.device(kw.get("device", "cuda:0"))
        part_id = partition_graph(edge_index.to(dev), x.shape[0], num_parts, **dict(partition or {}))
        self = cls(x, edge_index, y, train_mask, val_mask, test_mask, part_id, num_parts=num_parts, **kw)
        self.part_id = part_id
        return self

    def batch_sizes(self, group):
        """(n_b, E_b) of the union of the partitions in `group` from host tables alone; E_b is None when P is above the block
        table's limit (`size_path == "readback"`: the collate counts on the device and reads 8 bytes back)."""
        if not self.keep_cut_edges:
            raise ValueError("ResidentPartitions was built without keep_cut_edges=True: the edges between partitions are gone")
        n_b = sum(self.node_ptr_host[p + 1] - self.node_ptr_host[p] for p in group)
        E_b = None
        if self.block_edges is not None:
            g = torch.as_tensor(list(group), dtype=torch.int64)
            E_b = int(self.block_edges[g][:, g].sum())
        if n_b >= 2 ** 31 or (E_b is not None and E_b >= 2 ** 31):
            raise ValueError(f"a batch of {n_b} nodes / {E_b} edges does not fit the int32 graph kernels (limit 2^31)")
        return n_b, E_b

    def loader(self, batch_size, regroup="fixed", shuffle=False, seed=0) -> "ResidentClusterLoader":
        return ResidentClusterLoader(self, batch_size, regroup=regroup, shuffle=shuffle, seed=seed)

    def __len__(self):
        return self.num_parts

    def __getitem__(self, i):
        return self.batches[i]

    # ------------------------------------------------------------------ on-disk partition cache
    # The reference caches the METIS result through ClusterData(save_dir=...) (main.py:59-63; PyG 2.3.1 writes
    # `save_dir/partition_<P>.pt` = (adj, partptr, perm)) and re-slices every batch from it on the CPU.  Here the cache holds the
    # result of that slicing too, as ONE tensor-only safetensors file `save_dir/sgs_partitions_<P>.safetensors`:
    #   perm [N] i64        original node id of new node i (nodes grouped by partition; PyG's `perm`)
    #   node_ptr [P+1] i64  partition p owns new nodes node_ptr[p]:node_ptr[p+1]          (PyG's `partptr`)
    #   edge_ptr [P+1] i64  ... and intra-partition edges edge_ptr[p]:edge_ptr[p+1]
    #   x [N,F] f32, y [N] i64, train_mask / val_mask / test_mask [N] u8     node attributes in new order
    #   edge_index [2,E'] i64   intra-partition edges, partition-LOCAL node ids, row-sorted inside each partition
    #   prob [E'] f32           the edge prior sliced like edge_index (add_degree / add_ER output)
    # metadata: format = "sgs-partitions-v1", num_parts, dropped_edges.  Nothing in the file is executable.
    FORMAT = "sgs-partitions-v1"

    @staticmethod
    def cache_path(save_dir: str, num_parts: int) -> str:
        import os
        return os.path.join(save_dir, f"sgs_partitions_{int(num_parts)}.safetensors")

    def save(self, save_dir: str) -> str:
        import os
        from safetensors.torch import save_file
        os.makedirs(save_dir, exist_ok=True)
        cat = lambda k, dim=0: torch.cat([getattr(b, k) for b in self.batches], dim=dim).contiguous().cpu()      # noqa: E731
        t = dict(perm=self.perm.cpu(), node_ptr=self.node_ptr.cpu(), edge_ptr=self.edge_ptr.cpu(), x=cat("x"), y=cat("y"),
                 train_mask=cat("train_mask").to(torch.uint8), val_mask=cat("val_mask").to(torch.uint8),
                 test_mask=cat("test_mask").to(torch.uint8), edge_index=cat("edge_index", 1), prob=cat("prob"))
        path = self.cache_path(save_dir, self.num_parts)
        save_file(t, path, metadata={"format": self.FORMAT, "num_parts": str(self.num_parts), "dropped_edges": str(self.dropped_edges)})
        return path

    @classmethod
    def load(cls, save_dir: str, num_parts: int, device="cuda:0", shuffle=False, seed=0, *, keep_cut_edges=False) -> "ResidentPartitions":
        """Rebuild the resident partition tables from `save()`'s file: memory-mapped read, one host-to-device copy per tensor,
        then per-partition views (no re-partitioning, no prior recomputation)."""
        if keep_cut_edges:
            raise ValueError(f"the {cls.FORMAT} cache holds intra-partition edges only: keep_cut_edges=True needs the whole graph, "
                             "build ResidentPartitions(..., keep_cut_edges=True) from it instead")
        from safetensors import safe_open
        dev = torch.device(device)
        path = cls.cache_path(save_dir, num_parts)
        with safe_open(path, framework="pt", device="cpu") as f:
            meta = f.metadata() or {}
            if meta.get("format") != cls.FORMAT or int(meta.get("num_parts", -1)) != int(num_parts):
                raise ValueError(f"{path}: not a {cls.FORMAT} cache for {num_parts} partitions")
            t = {k: f.get_tensor(k).to(dev) for k in f.keys()}
        self = cls.__new__(cls)
        P = int(num_parts)
        self.num_parts, self.perm, self.node_ptr, self.edge_ptr = P, t["perm"], t["node_ptr"], t["edge_ptr"]
        self.dropped_edges = int(meta.get("dropped_edges", 0))
        nptr, eptr = t["node_ptr"].tolist(), t["edge_ptr"].tolist()
        if len(nptr) != P + 1 or len(eptr) != P + 1 or nptr[-1] != t["x"].shape[0] or eptr[-1] != t["edge_index"].shape[1]:
            raise ValueError(f"{path}: inconsistent partition pointers")
        tm, vm, sm = t["train_mask"].bool(), t["val_mask"].bool(), t["test_mask"].bool()
        self.batches = []
        for p in range(P):
            a, b, ea, eb = nptr[p], nptr[p + 1], eptr[p], eptr[p + 1]
            self.batches.append(Batch(x=t["x"][a:b], edge_index=t["edge_index"][:, ea:eb].contiguous(), y=t["y"][a:b], train_mask=tm[a:b],
                                      val_mask=vm[a:b], test_mask=sm[a:b], prob=t["prob"][ea:eb], part=p, node_ids=t["perm"][a:b]))
        self.shuffle = shuffle
        self._gen = torch.Generator().manual_seed(seed)
        self.keep_cut_edges = False
        return self

    def __iter__(self):
        order = torch.randperm(self.num_parts, generator=self._gen).tolist() if self.shuffle else range(self.num_parts)
        for i in order:
            yield self.batches[i]


# ---------------------------------------------------------------------------------------------------- multi-partition batches
def collate_torch(parts: ResidentPartitions, group) -> Batch:
    """The union of the partitions in `group` (ascending) with the cut edges between them restored, as a plain torch composition
    over `parts`' whole-graph CSR.  It defines the batch (nodes = the partitions' node lists concatenated, edges relabelled and
    ordered by (local src, local dst), `prob` gathered or -- prior="local" -- recomputed) and is what runs on a CPU device; on a HIP
    device the loader calls `ops.cluster_collate` instead and this composition only serves as the yardstick of
    tools/cluster_batch_probe.py."""
    group = _check_group(parts, group)
    dev = parts.full_ptr.device
    nptr = parts.node_ptr_host
    rows = torch.cat([torch.arange(nptr[p], nptr[p + 1], device=dev) for p in group])
    n_b = rows.numel()
    loc = torch.full((parts.num_nodes,), -1, dtype=torch.int64, device=dev)
    loc[rows] = torch.arange(n_b, device=dev)
    src, eid = _expand_rows(parts.full_ptr, rows)
    dst = loc[parts.full_col[eid]]
    keep = dst >= 0
    ei = torch.stack([src[keep], dst[keep]]).contiguous()           # rows ascending; a row's columns keep their order (monotone relabelling)
    prob = batch_prior(parts.full_prob, eid[keep], ei, n_b)
    m = parts.masks_all[:, rows].bool()
    return Batch(x=parts.x_all[rows], edge_index=ei, y=parts.y_all[rows], train_mask=m[0].contiguous(), val_mask=m[1].contiguous(),
                 test_mask=m[2].contiguous(), prob=prob, node_ids=parts.perm[rows], parts=group,
                 restored_edges=int(ei.shape[1]) - _intra_edges(parts, group))


def _check_group(parts, group):
    if not getattr(parts, "keep_cut_edges", False):
        raise ValueError("ResidentPartitions was built without keep_cut_edges=True: the edges between partitions are gone")
    g = tuple(sorted(int(p) for p in group))
    if len(g) < 1 or len(set(g)) != len(g) or g[0] < 0 or g[-1] >= parts.num_parts:
        raise ValueError(f"a group is a non-empty set of distinct partition ids below {parts.num_parts}, got {tuple(group)}")
    return g


def _intra_edges(parts, group) -> int:
    return sum(parts.edge_ptr_host[p + 1] - parts.edge_ptr_host[p] for p in group)


class ResidentClusterLoader:
    """`ClusterLoader(cluster_data, batch_size=k, shuffle=...)` over a resident graph: every step trains on the union of k partitions
    with the edges between those k partitions put back (Cluster-GCN's stochastic multiple partitions).  Groups are the consecutive
    chunks of k of `randperm(P)` (or of `range(P)`), each taken in ascending partition id.

    regroup="fixed": the order is drawn once; the merged batches are built once and stay resident in `self.batches`, so everything
    downstream (captured replay included) sees ordinary resident batches.  regroup="epoch": a fresh order at every `__iter__`, a fresh
    batch every step -- on a HIP device each one is built by `ops.cluster_collate` (four launches), never by a torch composition.
    `dropped_edges`: edges of the graph that no batch holds (fixed), or that the last completed epoch did not see (epoch)."""

    def __init__(self, parts: ResidentPartitions, batch_size: int, regroup: str = "fixed", shuffle: bool = False, seed: int = 0):
        if not getattr(parts, "keep_cut_edges", False):
            raise ValueError("ResidentClusterLoader needs ResidentPartitions(..., keep_cut_edges=True)")
        if regroup not in ("fixed", "epoch"):
            raise ValueError(f"regroup must be 'fixed' or 'epoch', got {regroup!r}")
        k = int(batch_size)
        if k < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        self._on_device = parts.full_ptr.is_cuda
        if self._on_device:
            from . import ops
            cap = ops.cluster_collate_max_parts()
            if k > cap:
                raise ValueError(f"batch_size {k} is above the device collate's limit of {cap} partitions per batch")
        self.parts, self.batch_size, self.regroup, self.shuffle = parts, k, regroup, bool(shuffle)
        self.size_path = parts.size_path
        self._gen = torch.Generator().manual_seed(seed)
        self.groups, self.batches, self.dropped_edges = None, None, None
        if regroup == "fixed":
            self.groups = self._draw()
            self.batches = [self._collate(g) for g in self.groups]
            self.dropped_edges = parts.num_edges - sum(int(b.edge_index.shape[1]) for b in self.batches)

    def _draw(self):
        P, k = self.parts.num_parts, self.batch_size
        order = torch.randperm(P, generator=self._gen).tolist() if self.shuffle else list(range(P))
        return [tuple(sorted(order[i:i + k])) for i in range(0, P, k)]

    def _collate(self, group) -> Batch:
        if self._on_device:
            from . import ops
            return ops.cluster_collate(self.parts, group)
        return collate_torch(self.parts, group)

    def __len__(self):
        return -(-self.parts.num_parts // self.batch_size)

    def __iter__(self):
        if self.regroup == "fixed":
            yield from self.batches
            return
        self.groups = self._draw()
        seen = 0
        for g in self.groups:
            b = self._collate(g)
            seen += int(b.edge_index.shape[1])
            yield b
        self.dropped_edges = self.parts.num_edges - seen


# ---------------------------------------------------------------------------------------------------- neighbour-sampled batches
_M32 = 0xFFFFFFFF
SUBGRAPH_TYPES = ("induced", "directional")


def fmix32(h: int) -> int:
    """murmur3's 32-bit finaliser (partition.py's hash)"""
    h &= _M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def neighbor_stream_key(seed: int, epoch: int, batch: int, hop: int) -> int:
    """K(seed, epoch, batch, hop) = fmix32(hop + fmix32(batch + fmix32(epoch + fmix32(seed)))), additions modulo 2^32: the key under which
    hop `hop` of batch `batch` of epoch `epoch` ranks edge id e by fmix32(e ^ K)."""
    k = fmix32(int(seed))
    for t in (epoch, batch, hop):
        k = fmix32(int(t) + k)
    return k


def fmix32_tensor(h):
    """`fmix32` on an int64 tensor of 32-bit values (partition.py's parity hash, the neighbour sampler's keys)"""
    h = h & _M32
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def _log2_table():
    """T[i] = floor(2^24 log2(1 + i / 256)), i = 0 .. 256, by repeated squaring with Python integers at 200 fractional bits (the table of
    csrc/neighbor.hip, which builds it at compile time)"""
    bits, out = 200, []
    for i in range(256):
        y, t = (256 + i) << (bits - 8), 0
        for _ in range(24):
            y = (y * y) >> bits
            t <<= 1
            if y >> (bits + 1):
                t, y = t | 1, y >> 1
        out.append(t)
    return out + [1 << 24]


_LOG2_TABLE = {}


def _log2q_tensor(x):
    """LOG2Q of include/sgs_hip.h on an int64 tensor of values in [1, 2^32), integer ops only"""
    T = _LOG2_TABLE.get(x.device)
    if T is None:
        T = _LOG2_TABLE[x.device] = torch.tensor(_log2_table(), dtype=torch.int64, device=x.device)
    n, t = torch.zeros_like(x), x
    for sh in (16, 8, 4, 2, 1):
        big = (t >> sh) > 0
        n = n + big * sh
        t = torch.where(big, t >> sh, t)
    m = (x << (32 - n)) & _M32
    i, r = m >> 24, (m >> 8) & 0xFFFF
    return (n << 24) + T[i] + (((T[i + 1] - T[i]) * r) >> 16)


def _weighted_key_tensor(h, wq):
    """sgs_nbr_weighted_key on int64 tensors: the hash h of an edge id and its quantised weight -> the key (2^32 - 1 where wq == 0)"""
    nl = (32 << 24) - _log2q_tensor(h.clamp(min=1))
    key = _log2q_tensor(nl) - _log2q_tensor(wq.clamp(min=1)) + (24 << 24)
    return torch.where(wq >= 1, key, torch.full_like(key, _M32))


def _expand_rows(ptr, rows):
    """-> (row number, position in the CSR arrays) of every entry of the CSR rows `rows`, rows back to back"""
    dev = ptr.device
    beg = ptr[rows].to(torch.int64)
    deg = ptr[rows + 1].to(torch.int64) - beg
    rid = torch.repeat_interleave(torch.arange(rows.numel(), device=dev), deg)
    pos = torch.repeat_interleave(beg - (torch.cumsum(deg, 0) - deg), deg) + torch.arange(int(rid.numel()), device=dev)
    return rid, pos


def check_fanouts(num_neighbors):
    fan = [int(f) for f in num_neighbors]
    if len(fan) < 1:
        raise ValueError("num_neighbors must name at least one hop")
    if any(f == 0 or f < -1 for f in fan):
        raise ValueError(f"a fan-out is >= 1, or -1 for every neighbour; got {fan}")
    return fan


def check_subgraph_type(subgraph_type):
    if subgraph_type == "bidirectional":
        raise ValueError("subgraph_type='bidirectional' is not supported: use 'induced' (every stored edge among the batch's nodes) "
                         "or 'directional' (the sampled edges)")
    if subgraph_type not in SUBGRAPH_TYPES:
        raise ValueError(f"subgraph_type must be one of {SUBGRAPH_TYPES}, got {subgraph_type!r}")
    return subgraph_type


class ResidentGraph:
    """One whole graph resident on `device`, for batches that are SAMPLED from it rather than cut out of it (`neighbor_loader`): the edge
    list sorted by (src, dst) -- an edge's id is its position there; `edge_order` maps it back to the caller's list --, both CSR orientations
    (ops.get_graph's on a HIP device), the full-graph prior `prob` in sorted order (`prior="global"`: ops.degree_prior unless given;
    `prior="local"`: none, every batch computes the prior of its own edge list), x, y and the three masks as [3, N] bytes.  The graph may be
    directed and may hold self loops and repeated edges."""

    def __init__(self, x, edge_index, y, train_mask, val_mask, test_mask, device="cuda:0", prior="global", prob=None):
        if prior not in ("global", "local"):
            raise ValueError(f"prior must be 'global' or 'local', got {prior!r}")
        dev = torch.device(device)
        N, E = int(x.shape[0]), int(edge_index.shape[1])
        if not 1 <= N < 2 ** 31 or E >= 2 ** 31:
            raise ValueError(f"a graph of {N} nodes / {E} edges does not fit the int32 graph kernels (need 1 <= N < 2^31, E < 2^31)")
        ei = edge_index.to(dev).to(torch.int64)
        if E and (int(ei.min()) < 0 or int(ei.max()) >= N):
            raise ValueError("edge_index holds a node id outside [0, N)")
        order = torch.argsort(ei[0] * N + ei[1], stable=True)
        ei = ei[:, order].contiguous()
        self.num_nodes, self.num_edges, self.edge_index, self.edge_order = N, E, ei, order
        self.on_device = dev.type == "cuda"
        if self.on_device:
            from . import ops
            g = ops.get_graph(ei, N)
            self.in_ptr, self.in_eid, self.out_ptr, self.out_dst, self.out_eid = g.in_ptr, g.in_eid, g.out_ptr, g.out_dst, g.out_eid
            self._nbr_state = ops.nbr_state(N, dev)
            self.collate_mismatch = torch.zeros(1, dtype=torch.int32, device=dev)       # set if a batch's members are not the nodes counted
        else:
            by_dst = torch.argsort(ei[1], stable=True)                                  # rows in ascending edge id, like sgs_graph_build's
            ptr_of = lambda r: torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(r, minlength=N), 0)]).to(torch.int32)  # noqa: E731
            self.in_ptr, self.in_eid = ptr_of(ei[1]), by_dst.to(torch.int32)
            self.out_ptr, self.out_dst, self.out_eid = ptr_of(ei[0]), ei[1].to(torch.int32), torch.arange(E, dtype=torch.int32)
        if prob is not None:
            prob = prob.to(dev)[order].contiguous()
        elif prior == "global":
            prob = batch_prior(None, None, ei, N)
        self.prob, self.prior = prob, prior
        self.x, self.y = x.to(dev).contiguous(), y.to(dev).to(torch.int64).contiguous()
        self.masks = torch.stack([train_mask, val_mask, test_mask]).to(dev).to(torch.uint8).contiguous()
        ip = self.in_ptr.cpu().to(torch.int64)                                          # one read-back at construction: the seeds' rows are sized on the host
        self.in_deg_host = ip[1:] - ip[:-1]

    def neighbor_loader(self, num_neighbors, batch_size, input_nodes="train", shuffle=True, seed=0, subgraph_type="induced", resample="epoch",
                        drop_last=False, weight=None) -> "NeighborLoader":
        return NeighborLoader(self, num_neighbors, batch_size, input_nodes=input_nodes, shuffle=shuffle, seed=seed, subgraph_type=subgraph_type,
                              resample=resample, drop_last=drop_last, weight=weight)

    def neighbor_weights(self, weight):
        """The `weight_q` of `batch` for a loader's `weight`: None -> None (the uniform draw); "prob" -> the full-graph prior; a float tensor
        [E] of weights >= 0 in the CALLER's edge order (learned edge scores, an effective-resistance prior, ...).  -> int32 [E] on the graph's
        device, quantised (ops.nbr_quantize_weights) and in in-CSR order, aligned with `in_eid`."""
        if weight is None:
            return None
        from . import ops
        if isinstance(weight, str):
            if weight != "prob":
                raise ValueError(f"weight must be None, 'prob' or a tensor of one weight per edge, got {weight!r}")
            if self.prob is None:
                raise ValueError("weight='prob' needs the full-graph prior: this graph was built with prior='local'")
            w = self.prob
        else:
            w = torch.as_tensor(weight)
            if w.dim() != 1 or w.numel() != self.num_edges or not w.is_floating_point():
                raise ValueError(f"a weight tensor holds one floating-point weight per edge ({self.num_edges}), in the order of the edge list given")
            w = w.to(self.edge_index.device)[self.edge_order]
        return ops.nbr_quantize_weights(w)[self.in_eid.to(torch.int64)].contiguous()

    def check_seeds(self, seeds):
        s = torch.as_tensor(seeds, dtype=torch.int64).cpu().reshape(-1)
        if s.numel() and (int(s.min()) < 0 or int(s.max()) >= self.num_nodes):
            raise ValueError(f"a seed node id lies outside [0, {self.num_nodes})")
        if torch.unique(s).numel() != s.numel():
            raise ValueError("the seed nodes must be distinct")
        return s

    def batch(self, seeds, num_neighbors, keys, subgraph_type="induced", weight_q=None) -> Batch:
        """One batch: distinct `seeds`, one fan-out and one 32-bit stream key per hop.  On a HIP device it is built by the kernels of
        csrc/neighbor.hip (ops.neighbor_batch), never by a torch composition; on the CPU by `neighbor_collate_torch`.  `weight_q`
        (`neighbor_weights`): quantised weights in in-CSR order for a weighted draw; None: the uniform one."""
        fan, subgraph_type, seeds = check_fanouts(num_neighbors), check_subgraph_type(subgraph_type), self.check_seeds(seeds)
        if len(keys) != len(fan):
            raise ValueError("one stream key per hop")
        if weight_q is not None and (weight_q.dtype != torch.int32 or weight_q.numel() != self.num_edges or weight_q.device != self.in_eid.device):
            raise ValueError("weight_q: int32, one entry per in-CSR entry, on the graph's device (ResidentGraph.neighbor_weights)")
        if self.on_device:
            from . import ops
            if len(fan) > ops.nbr_max_hops():
                raise ValueError(f"{len(fan)} hops, the device builder's limit is {ops.nbr_max_hops()}")
            return ops.neighbor_batch(self, seeds, fan, keys, subgraph_type, weight_q)
        return neighbor_collate_torch(self, seeds, fan, keys, subgraph_type, weight_q)


def neighbor_collate_torch(graph: ResidentGraph, seeds, num_neighbors, keys, subgraph_type="induced", weight_q=None) -> Batch:
    """The neighbour-sampled batch as a plain torch composition over `graph`'s tensors, wherever they live.  It is what runs when the graph is
    on the CPU and the yardstick of tools/neighbor_probe.py; on a HIP device the loader calls ops.neighbor_batch instead.  Rules
    ("Neighbour-sampled batches"): hop h takes, for every frontier node, all its in-edges if there are at most f_h (or
    f_h = -1), else the f_h whose keys fmix32(edge id ^ K_h) are smallest; the sources not yet in the batch form the next frontier;
    node_ids ascending; `induced` = every stored edge among them, `directional` = the chosen edges, both in ascending edge id.
    `weight_q` (int32 [E] in in-CSR order): the keys are sgs_nbr_weighted_key's, computed with torch integer ops; they can tie, and a stable
    sort by (row, key) then takes the earliest ties in row order ("Weighted neighbour sampling" in the same section)."""
    fan, subgraph_type = check_fanouts(num_neighbors), check_subgraph_type(subgraph_type)
    dev, N = graph.edge_index.device, graph.num_nodes
    seeds = torch.as_tensor(seeds, dtype=torch.int64).to(dev)
    member = torch.zeros(N, dtype=torch.bool, device=dev)
    member[seeds] = True
    front, hop_nodes, chosen = seeds, [int(seeds.numel())], []
    for f, K in zip(fan, keys):
        rid, pos = _expand_rows(graph.in_ptr, front)
        ids = graph.in_eid[pos].to(torch.int64)
        if f >= 0:
            key = fmix32_tensor(ids ^ int(K))
            if weight_q is None:
                order = torch.argsort((rid << 32) | key)                 # by row, then by key: distinct ids have distinct keys
            else:
                order = torch.argsort((rid << 32) | _weighted_key_tensor(key, weight_q[pos].to(torch.int64)), stable=True)
            deg = torch.bincount(rid, minlength=front.numel())
            start = torch.cumsum(deg, 0) - deg
            keep = torch.zeros(ids.numel(), dtype=torch.bool, device=dev)
            keep[order] = (torch.arange(ids.numel(), device=dev) - start[rid[order]]) < f
            ids = ids[keep]
        chosen.append(ids)
        u = graph.edge_index[0][ids]
        front = torch.unique(u[~member[u]])
        member[front] = True
        hop_nodes.append(int(front.numel()))
    node_ids = torch.nonzero(member).reshape(-1)
    loc = torch.cumsum(member, 0) - 1
    if subgraph_type == "induced":
        rid, pos = _expand_rows(graph.out_ptr, node_ids)
        eid = graph.out_eid[pos].to(torch.int64)
        keep = member[graph.edge_index[1][eid]]
        eid = eid[keep]
        ei = torch.stack([rid[keep], loc[graph.edge_index[1][eid]]]).contiguous()
    else:
        eid = torch.sort(torch.cat(chosen)).values
        ei = torch.stack([loc[graph.edge_index[0][eid]], loc[graph.edge_index[1][eid]]]).contiguous()
    n = int(node_ids.numel())
    prob = batch_prior(graph.prob, eid, ei, n)
    is_seed = torch.zeros(N, dtype=torch.bool, device=dev)
    is_seed[seeds] = True
    seed_mask = is_seed[node_ids]
    m = graph.masks[:, node_ids].bool() & seed_mask[None, :]
    return Batch(x=graph.x[node_ids], edge_index=ei, y=graph.y[node_ids], train_mask=m[0].contiguous(), val_mask=m[1].contiguous(),
                 test_mask=m[2].contiguous(), prob=prob, eid=eid, node_ids=node_ids, seed_mask=seed_mask, n_seeds=int(seeds.numel()),
                 hop_nodes=hop_nodes)


class NeighborLoader:
    """GraphSAGE-style mini-batches over a `ResidentGraph` (PyG's `NeighborLoader`): batch b of an epoch is the b-th chunk of `batch_size`
    seed nodes of the (shuffled) input list plus their sampled len(num_neighbors)-hop in-neighbourhood.  The shuffle is drawn on the host by a
    generator seeded with (seed, epoch); the neighbours by the integer stream keys `neighbor_stream_key(seed, epoch, b, hop)`, so a
    (seed, epoch) pair names its batches exactly.  `epoch` advances at every `__iter__`; `set_epoch(e)` pins it (None: advance again).

    Only the seeds of a batch have a sampled receptive field: its train / val / test masks are the graph's ANDed with `seed_mask`, so loss,
    gate and metrics count seeds only, and a pass with `input_nodes` covering every node once counts every node exactly once.
    resample="epoch": a fresh batch every step (eager training only).  resample="fixed": the batches of epoch 0 are built once and stay
    resident in `self.batches` -- ordinary resident batches, which replay under args.sgs_hipgraph.  `q` stays per step, the caller's to scale.

    weight=None: every hop draws uniformly.  weight="prob" (the graph's full-graph prior) or a float tensor [E] in the caller's edge order:
    a frontier node with more than f in-edges draws f of them without replacement, each draw proportional to the weight among those left
    (`ResidentGraph.neighbor_weights`; zero-weight edges only when fewer than f positive ones exist).  Still a pure integer function of
    (seed, epoch, batch, hop) and the quantised weights.  `set_weight` swaps the weights between epochs, e.g. for the scorer's latest edge
    probabilities."""

    def __init__(self, graph: ResidentGraph, num_neighbors, batch_size: int, input_nodes="train", shuffle: bool = True, seed: int = 0,
                 subgraph_type: str = "induced", resample: str = "epoch", drop_last: bool = False, weight=None):
        self.num_neighbors, self.subgraph_type = check_fanouts(num_neighbors), check_subgraph_type(subgraph_type)
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        if resample not in ("fixed", "epoch"):
            raise ValueError(f"resample must be 'fixed' or 'epoch', got {resample!r}")
        if graph.on_device:
            from . import ops
            if len(self.num_neighbors) > ops.nbr_max_hops():
                raise ValueError(f"{len(self.num_neighbors)} hops, the device builder's limit is {ops.nbr_max_hops()}")
        if isinstance(input_nodes, str):
            if input_nodes not in ("train", "val", "test", "all"):
                raise ValueError(f"input_nodes must be 'train', 'val', 'test', 'all', a bool mask or a list of node ids, got {input_nodes!r}")
            ids = (torch.arange(graph.num_nodes) if input_nodes == "all"
                   else torch.nonzero(graph.masks[("train", "val", "test").index(input_nodes)]).reshape(-1).cpu())
        else:
            t = torch.as_tensor(input_nodes)
            if t.dtype == torch.bool:
                if t.numel() != graph.num_nodes:
                    raise ValueError("a bool input_nodes mask needs one entry per node")
                ids = torch.nonzero(t).reshape(-1).cpu()
            else:
                ids = graph.check_seeds(t)
        self.graph, self.batch_size, self.shuffle, self.seed = graph, int(batch_size), bool(shuffle), int(seed)
        self.resample, self.drop_last, self.input_ids = resample, bool(drop_last), ids.to(torch.int64)
        self.epoch, self._pinned, self.batches = 0, None, None
        self.weight_q = graph.neighbor_weights(weight)
        if resample == "fixed":
            self.batches = list(self._build(0))

    def set_epoch(self, epoch) -> None:
        self._pinned = None if epoch is None else int(epoch)

    def set_weight(self, weight) -> None:
        """Replaces the fan-out weights (None, "prob" or a tensor, as at construction); the next `__iter__` draws with them."""
        if self.batches is not None:
            raise ValueError("set_weight: the batches of a resample='fixed' loader are already built; make a new loader")
        self.weight_q = self.graph.neighbor_weights(weight)

    def seed_lists(self, epoch: int):
        ids = self.input_ids
        if self.shuffle:
            g = torch.Generator().manual_seed((self.seed * 0x9E3779B1 + int(epoch)) % (1 << 63))
            ids = ids[torch.randperm(ids.numel(), generator=g)]
        out = [ids[i:i + self.batch_size] for i in range(0, ids.numel(), self.batch_size)]
        if self.drop_last and out and out[-1].numel() < self.batch_size:
            out.pop()
        return out

    def _build(self, epoch: int):
        L = len(self.num_neighbors)
        for b, seeds in enumerate(self.seed_lists(epoch)):
            keys = [neighbor_stream_key(self.seed, epoch, b, h) for h in range(L)]
            yield self.graph.batch(seeds, self.num_neighbors, keys, self.subgraph_type, self.weight_q)

    def __len__(self):
        n = self.input_ids.numel()
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        if self.resample == "fixed":
            yield from self.batches
            return
        epoch = self.epoch if self._pinned is None else self._pinned
        self.epoch = epoch + 1
        yield from self._build(epoch)


def synthetic_partitioned_graph(num_parts: int, n_per_part: int, e_intra, cut_frac: float, nfeat: int, ncls: int, seed: int, device="cpu"):
    """-> (Batch, part_id): `num_parts` graphs of `synthetic_graph(n_per_part, e_intra, ...)` (`e_intra`: one stored-edge target or one per
    partition) on disjoint node ranges, plus cut_frac * (undirected intra-partition edges) further undirected edges between uniformly drawn
    nodes of DIFFERENT partitions (drawn until that many distinct pairs exist), coalesced, row-sorted, stored both ways, with the degree
    prior of the whole graph.  Node ids are then shuffled, so a partition is not a contiguous id range.  `reddit_partition_stream` makes
    independent partitions with no edge between them; this is the same material with a cut structure -- a synthetic one."""
    dev = torch.device(device)
    P, n = int(num_parts), int(n_per_part)
    N = P * n
    targets = [int(e_intra)] * P if not hasattr(e_intra, "__len__") else [int(e) for e in e_intra]
    if len(targets) != P:
        raise ValueError("e_intra must be one number or one per partition")
    g = torch.Generator(device=dev).manual_seed(seed)
    kw = dict(generator=g, device=dev)
    subs = [synthetic_graph(n, targets[p], nfeat, ncls, seed * 1000 + p, device=dev) for p in range(P)]
    intra = torch.cat([(b.edge_index[0] + p * n) * N + (b.edge_index[1] + p * n) for p, b in enumerate(subs)])
    m_cut = int(cut_frac * (intra.numel() // 2)) if P > 1 else 0
    cut = torch.zeros(0, dtype=torch.int64, device=dev)
    while cut.numel() < m_cut:
        need = int((m_cut - cut.numel()) * 1.3) + 16
        a, b = torch.randint(0, N, (need,), **kw), torch.randint(0, N, (need,), **kw)
        ok = (a // n) != (b // n)
        lo, hi = torch.minimum(a[ok], b[ok]), torch.maximum(a[ok], b[ok])
        cut = torch.unique(torch.cat([cut, lo * N + hi]))
    cut = cut[torch.randperm(cut.numel(), **kw)[:m_cut]]
    lo, hi = cut // N, cut % N
    keys = torch.cat([intra, lo * N + hi, hi * N + lo])
    sigma = torch.randperm(N, **kw)                                   # contiguous id -> shuffled id
    keys = torch.unique(sigma[keys // N] * N + sigma[keys % N])       # sorted -> row-sorted, coalesced
    ei = torch.stack([keys // N, keys % N])
    cat = lambda k: torch.cat([getattr(b, k) for b in subs])          # noqa: E731
    scat = lambda t: torch.empty_like(t).index_copy_(0, sigma, t)     # noqa: E731
    part_id = scat(torch.arange(N, device=dev) // n)
    return Batch(x=scat(cat("x")), edge_index=ei, y=scat(cat("y")), train_mask=scat(cat("train_mask")), val_mask=scat(cat("val_mask")),
                 test_mask=scat(cat("test_mask")), prob=degree_prior(ei, N)), part_id
