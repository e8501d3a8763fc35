"""The node-covering draw (sgs_sample_topq_cover) restated on integers.

Input: the fp32 keys of the draw (the device's own `keys_out`, or any non-negative fp32 vector), the candidate edge list, N and q.
Everything below is integer logic on the keys' bit patterns, vectorised with numpy (no loop over edges), so it does not depend on
floating-point arithmetic:

  1. forced edge of node i: among the edges with dst == i and src != i, the largest key, ties to the lowest edge id;
  2. boosted key: the key's bits with bit 31 set when the edge is forced;
  3. selected: the q largest boosted keys, ties to the lowest edge id.

`cover_ref_loop` is the same rule as a per-node Python loop, for checking this file against itself on small graphs."""
import numpy as np
import torch


def key_bits(keys) -> np.ndarray:
    """fp32 keys (tensor or array) -> their bit patterns as int64 (keys are >= 0: bit 31 is clear)."""
    k = keys.detach().cpu().numpy() if isinstance(keys, torch.Tensor) else np.asarray(keys)
    return np.ascontiguousarray(k, dtype=np.float32).view(np.uint32).astype(np.int64)


def _ei(edge_index) -> np.ndarray:
    return edge_index.detach().cpu().numpy() if isinstance(edge_index, torch.Tensor) else np.asarray(edge_index)


def forced_edges(bits: np.ndarray, edge_index, N: int) -> np.ndarray:
    """bool [E]: the forced edges (step 1)."""
    ei = _ei(edge_index)
    E = bits.shape[0]
    forced = np.zeros(E, dtype=bool)
    cand = np.nonzero(ei[0] != ei[1])[0]
    if cand.size == 0:
        return forced
    dst = ei[1][cand]
    order = np.lexsort((cand, -bits[cand], dst))          # by dst, then key descending, then edge id ascending
    ds = dst[order]
    first = np.ones(ds.size, dtype=bool)
    first[1:] = ds[1:] != ds[:-1]
    forced[cand[order[first]]] = True
    return forced


def top_q(bits: np.ndarray, q: int) -> np.ndarray:
    """bool [E]: the q largest entries of `bits`, ties to the lowest index."""
    E = bits.shape[0]
    mask = np.zeros(E, dtype=bool)
    if q > 0:
        mask[np.lexsort((np.arange(E), -bits))[:q]] = True
    return mask


def cover_ref(keys, edge_index, N: int, q: int) -> dict:
    """-> dict(mask bool [E], eid int64 [q] ascending, forced bool [E], M, n_forced_selected, threshold_bits (unboosted, of the q-th
    largest boosted key; 0 when q == 0), ties (number of selected edges whose boosted key equals the q-th largest))."""
    bits = key_bits(keys)
    forced = forced_edges(bits, edge_index, N)
    boosted = bits | (forced.astype(np.int64) << 31)
    mask = top_q(boosted, q)
    M = int(forced.sum())
    out = dict(mask=mask, eid=np.nonzero(mask)[0].astype(np.int64), forced=forced, M=M, n_forced_selected=int((forced & mask).sum()),
               threshold_bits=0, ties=0)
    if q > 0:
        T = int(boosted[mask].min())
        out["threshold_bits"] = T & 0x7FFFFFFF
        out["ties"] = int((boosted[mask] == T).sum())
    return out


def plain_ref(keys, q: int) -> np.ndarray:
    """The plain draw's mask for the same keys."""
    return top_q(key_bits(keys), q)


def cover_ref_loop(keys, edge_index, N: int, q: int) -> dict:
    """The rule as a per-node loop (small graphs only)."""
    bits = key_bits(keys)
    ei = _ei(edge_index)
    E = bits.shape[0]
    forced = np.zeros(E, dtype=bool)
    for i in range(N):
        best = -1
        for e in range(E):
            if ei[1][e] == i and ei[0][e] != i and (best < 0 or bits[e] > bits[best]):
                best = e
        if best >= 0:
            forced[best] = True
    boosted = [int(bits[e]) | (int(forced[e]) << 31) for e in range(E)]
    order = sorted(range(E), key=lambda e: (-boosted[e], e))
    mask = np.zeros(E, dtype=bool)
    mask[order[:q]] = True
    return dict(mask=mask, forced=forced, M=int(forced.sum()))


def uncovered_nodes(mask, edge_index, N: int) -> int:
    """Nodes that have a non-loop in-edge among the candidates but none among the selected edges."""
    ei = _ei(edge_index)
    m = np.asarray(mask, dtype=bool)
    real = ei[0] != ei[1]
    has = np.zeros(N, dtype=bool)
    has[ei[1][real]] = True
    got = np.zeros(N, dtype=bool)
    got[ei[1][real & m]] = True
    return int((has & ~got).sum())
