"""GPU: sgs_graph_filter_multi / sgs_gcn_norm_fwd_multi give, for every draw, the in-CSR arrays of sgs_graph_filter (ops.get_subgraph)
and the in-direction outputs of sgs_gcn_norm_fwd -- on both scan forms of the filter: rows scanned by each wave (N <= 4096) and the
separate per-draw scan launch (N > 4096)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n,e_target", [(1013, 60_000), (6_000, 90_000)])
@pytest.mark.parametrize("weighted", [False, True])
def test_filter_and_norm_multi_equal_single_draw_kernels(n, e_target, weighted):
    import sgs_gnn_amd as S
    ops = S.ops
    b = S.synthetic_graph(n, e_target, 8, 3, seed=n, device=DEV)
    ei = b.edge_index
    E = ei.shape[1]
    q = E // 5
    D = 5
    g = torch.Generator().manual_seed(9)
    p = torch.rand(E, generator=g).to(DEV)
    parent = ops.get_graph(ei, n)
    smp = ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.3, q, ei, D, seed=5, stream_id0=40, want_w=weighted)
    csr = ops.graph_filter_multi(parent, smp)
    norm = ops.gcn_norm_multi(csr, smp.w if weighted else None, q, n)
    for d in range(D):
        r = ops.sample_topq(ops.SAMPLE_LEARNED, p, None, 0.3, q, ei, seed=5, stream_id=40 + d)
        assert torch.equal(r.eid, smp.eid[d])
        sub = ops.get_subgraph(ei, n, r)
        assert torch.equal(csr[0][d], sub.in_ptr)
        assert torch.equal(csr[1][d, :q], sub.in_src[:q])
        assert torch.equal(csr[2][d, :q], sub.in_eid[:q])
        assert torch.equal(csr[3][d], sub.loop_eid[:n])
        w = ops.st_weights(p, None, 0.3, r.stats, r.eid) if weighted else None
        nm = ops._norm_forward(sub, w)
        for got, want in ((norm[0][d], nm.dis), (norm[1][d], nm.loopw), (norm[2][d, :q], nm.what_in[:q]), (norm[3][d], nm.what_loop)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
