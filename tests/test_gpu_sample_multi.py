"""GPU: sgs_sample_topq_multi's draw d is bitwise what sgs_sample_topq returns for stream id s0 + d (or noise row d), on the small-E
(fused) and the large-E path, for the learned (istest), prior and uniform draws, with the straight-through weights folded in."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, S0 = 1234, 77


def _inputs(kind, E, g):
    import sgs_gnn_amd as S
    if kind == "learned":
        return S.ops.SAMPLE_LEARNED, torch.rand(E, generator=g).to(DEV)
    if kind == "prior":
        return S.ops.SAMPLE_PRIOR, torch.randn(E, generator=g).to(DEV)
    return S.ops.SAMPLE_LEARNED, None


def _check(kind, E, q, D, explicit):
    import sgs_gnn_amd as S
    g = torch.Generator().manual_seed(E + D)
    mode, p = _inputs(kind, E, g)
    ei = torch.randint(0, 5000, (2, E), generator=g).to(DEV)
    noise = torch.empty(D, E).exponential_(1, generator=g).to(DEV) if explicit else None
    want_w = kind == "learned"
    m = S.ops.sample_topq_multi(mode, p, None, 0.3, q, ei, D, noise=noise, seed=SEED, stream_id0=S0, want_w=want_w)
    for d in range(D):
        r = S.ops.sample_topq(mode, p, None, 0.3, q, ei, noise=None if noise is None else noise[d].contiguous(), seed=SEED, stream_id=S0 + d)
        assert torch.equal(m.mask[d], r.mask), (kind, E, D, d)
        assert torch.equal(m.eid[d], r.eid)
        assert torch.equal(m.edge_index[d], r.edge_index)
        assert torch.equal(m.stats[d].view(torch.int32), r.stats.view(torch.int32))
        if want_w:
            w = S.ops.st_weights(p, None, 0.3, r.stats, r.eid)
            assert torch.equal(m.w[d].view(torch.int32), w.view(torch.int32))
    if D > 1:
        assert not torch.equal(m.mask[0], m.mask[1])          # different streams, different draws


@pytest.mark.parametrize("kind", ["learned", "prior", "uniform"])
@pytest.mark.parametrize("D", [1, 2, 11])
@pytest.mark.parametrize("explicit", [False, True])
def test_small_path_bitwise(kind, D, explicit):
    _check(kind, 40_000, 10_000, D, explicit)


@pytest.mark.parametrize("kind", ["learned", "prior", "uniform"])
@pytest.mark.parametrize("D", [1, 2, 11])
@pytest.mark.parametrize("explicit", [False, True])
def test_large_path_bitwise(kind, D, explicit):
    _check(kind, (1 << 21) + 5_003, 400_000, D, explicit)


@pytest.mark.parametrize("E,q", [(40_000, 10_000), ((1 << 21) + 5_003, 400_000)])
def test_ties_take_lowest_ids(E, q):
    import sgs_gnn_amd as S
    p = torch.full((E,), 0.5, device=DEV)
    ei = torch.arange(2 * E, device=DEV).view(2, E)
    noise = torch.ones(3, E, device=DEV)
    m = S.ops.sample_topq_multi(S.ops.SAMPLE_LEARNED, p, None, 0.3, q, ei, 3, noise=noise)
    ar = torch.arange(q, device=DEV)
    for d in range(3):
        assert torch.equal(m.eid[d], ar)
        assert int(m.mask[d].sum()) == q and bool(m.mask[d, :q].all())


def test_degenerate_q_equals_E_and_zero():
    import sgs_gnn_amd as S
    E = 5000
    p = torch.rand(E, device=DEV)
    ei = torch.randint(0, 100, (2, E), device=DEV)
    for q in (0, E):
        m = S.ops.sample_topq_multi(S.ops.SAMPLE_LEARNED, p, None, 0.3, q, ei, 3, seed=SEED, stream_id0=S0, want_w=q > 0)
        for d in range(3):
            r = S.ops.sample_topq(S.ops.SAMPLE_LEARNED, p, None, 0.3, q, ei, seed=SEED, stream_id=S0 + d)
            assert torch.equal(m.mask[d], r.mask) and torch.equal(m.eid[d], r.eid) and torch.equal(m.edge_index[d], r.edge_index)
            assert torch.equal(m.stats[d], r.stats)


@pytest.mark.parametrize("E,q", [(40_000, 10_000), ((1 << 21) + 5_003, 400_000)])
def test_chunked_4_4_3_equals_one_pass(E, q):
    import sgs_gnn_amd as S
    g = torch.Generator().manual_seed(5)
    p = torch.rand(E, generator=g).to(DEV)
    ei = torch.randint(0, 5000, (2, E), generator=g).to(DEV)
    one = S.ops.sample_topq_multi(S.ops.SAMPLE_LEARNED, p, None, 0.3, q, ei, 11, seed=SEED, stream_id0=S0, want_w=True)
    parts = [S.ops.sample_topq_multi(S.ops.SAMPLE_LEARNED, p, None, 0.3, q, ei, k, seed=SEED, stream_id0=S0 + o, want_w=True)
             for o, k in ((0, 4), (4, 4), (8, 3))]
    for name in ("mask", "eid", "edge_index", "stats", "w"):
        assert torch.equal(getattr(one, name), torch.cat([getattr(r, name) for r in parts])), name
