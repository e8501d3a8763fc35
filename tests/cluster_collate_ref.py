"""Loop / numpy restatement of a multi-partition batch ("Multi-partition batches"), independent of the product.

A group G = {p_1 < ... < p_k} (always ascending).  Nodes of the batch: the partitions' node lists (each in ascending original id)
concatenated in that order; a node's local id is its position.  Edges: every input edge with both endpoints in G, relabelled,
ordered by (local src, local dst).  prob: the given per-edge values, gathered."""
import numpy as np


def collate_ref(edge_index, part_id, group, prob=None):
    """edge_index [2, E] int64, part_id [N] -> dict(node_ids [n_b], edge_index [2, E_b], eid [E_b] (index into the INPUT edge list),
    prob [E_b] or None, restored (edges of the batch whose endpoints lie in different partitions))."""
    edge_index, part_id = np.asarray(edge_index), np.asarray(part_id)
    group = sorted(int(p) for p in group)
    node_ids = np.concatenate([np.nonzero(part_id == p)[0] for p in group] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    local = {int(v): i for i, v in enumerate(node_ids)}
    rows = []
    restored = 0
    for e in range(edge_index.shape[1]):
        s, d = int(edge_index[0, e]), int(edge_index[1, e])
        if s in local and d in local:
            rows.append((local[s], local[d], e))
            restored += int(part_id[s] != part_id[d])
    rows.sort()
    arr = np.array(rows, dtype=np.int64).reshape(-1, 3)
    out = dict(node_ids=node_ids, edge_index=np.ascontiguousarray(arr[:, :2].T), eid=arr[:, 2].copy(), restored=restored, prob=None)
    if prob is not None:
        out["prob"] = np.asarray(prob)[arr[:, 2]]
    return out


def full_csr_ref(edge_index, part_id, num_parts):
    """The whole graph in partition-grouped node order: perm [N] (original id of new node i), node_ptr [P+1], full_ptr [N+1],
    full_col [E] (new ids, rows ascending, columns ascending inside a row), order [E] (input edge stored at each CSR position)."""
    edge_index, part_id = np.asarray(edge_index), np.asarray(part_id)
    N = part_id.shape[0]
    perm = np.argsort(part_id, kind="stable").astype(np.int64)
    new_id = np.empty(N, dtype=np.int64)
    new_id[perm] = np.arange(N)
    node_ptr = np.zeros(num_parts + 1, dtype=np.int64)
    node_ptr[1:] = np.cumsum(np.bincount(part_id, minlength=num_parts))
    s, d = new_id[edge_index[0]], new_id[edge_index[1]]
    order = np.lexsort((d, s)).astype(np.int64)
    full_ptr = np.zeros(N + 1, dtype=np.int64)
    full_ptr[1:] = np.cumsum(np.bincount(s, minlength=N))
    return dict(perm=perm, node_ptr=node_ptr, full_ptr=full_ptr, full_col=d[order].copy(), order=order)


def groups_ref(order, k):
    return [tuple(sorted(order[i:i + k])) for i in range(0, len(order), k)]
