"""fp64 dense restatement of the Chebyshev head's contract (PyG 2.3.1 ChebConv, normalization='sym', lambda_max = 2, restated from
memory: parity with PyG is unpinned).  L_hat is a dense [N, N] matrix and the layer runs the DIRECT T_k recurrence, so nothing here shares
the product's algebra (which is Clenshaw's recurrence at the output width); torch autograd gives every gradient."""
import torch


def laplacian(edge_index, w, N):
    """-> (L_hat [N, N], dis [N], l [n_edges]); `w` None = unit weights.  (i, i) edges carry weight 0, the degree is summed by SOURCE,
    dis = deg^-1/2 with 0 where deg = 0, l_e = -dis[s] w_e dis[d], (L_hat)[d, s] += l_e (duplicates add up), diagonal 0."""
    s, d = edge_index[0], edge_index[1]
    if w is None:
        w = torch.ones(s.numel(), dtype=torch.float64)
    wz = torch.where(s != d, w, torch.zeros_like(w))
    deg = torch.zeros(N, dtype=torch.float64).index_add(0, s, wz)
    pos = deg > 0
    dis = torch.where(pos, torch.where(pos, deg, torch.ones_like(deg)).pow(-0.5), torch.zeros_like(deg))
    l = -dis[s] * wz * dis[d]
    Lh = torch.zeros(N, N, dtype=torch.float64).index_put((d, s), l, accumulate=True)
    return Lh, dis, l


def conv(x, Ws, bias, Lh):
    """sum_k T_k(L_hat) x W_k^T + bias with T_0 = x, T_1 = L_hat x, T_k = 2 L_hat T_{k-1} - T_{k-2}."""
    t0 = x
    out = t0 @ Ws[0].t()
    if len(Ws) > 1:
        t1 = Lh @ x
        out = out + t1 @ Ws[1].t()
        for W in Ws[2:]:
            t2 = 2.0 * (Lh @ t1) - t0
            out = out + t2 @ W.t()
            t0, t1 = t1, t2
    return out + bias


def model(P, x, edge_index, w, K, keep=None, p=0.0):
    """ChebModel: gcn1 -> ReLU -> dropout (`keep` [N, H] in {0, 1}, scaled by 1 / (1 - p)) -> gcn2 on one L_hat.  `P`: the head's
    state_dict entries as fp64 tensors."""
    Lh, _, _ = laplacian(edge_index, w, x.shape[0])
    h = torch.relu(conv(x, [P[f"gcn1.lins.{k}.weight"] for k in range(K)], P["gcn1.bias"], Lh))
    if keep is not None:
        h = h * keep / (1.0 - p)
    return conv(h, [P[f"gcn2.lins.{k}.weight"] for k in range(K)], P["gcn2.bias"], Lh)
