"""GPU parity: the edge scorer at wide hidden sizes (256 < H <= 1024, H % 32 == 0; the chunked kernel edge_score_wide_kernel) against
the fp64 `_edge_score` of the oracle fed the same dropout masks (ops.dropout_keep), with the bounds of test_gpu_edge_score.py."""
import pytest
import torch

from oracle import sgs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()
    L.sgs_edge_score_set_variant(-1)
    L.sgs_edge_score_set_bwd_variant(-1)
    return sgs_gnn_amd.ops


def _case(N, H, E, seed):
    g = torch.Generator().manual_seed(seed)
    codes = torch.relu(torch.randn(N, H, generator=g))
    ei = torch.randint(0, N, (2, E), generator=g)
    if E > 5:
        ei[:, 2] = ei[0, 2]                                       # a self loop among the scored edges
    b = 1.0 / (2 * H) ** 0.5
    W1 = (torch.rand(H, 2 * H, generator=g) * 2 - 1) * b
    b1 = (torch.rand(H, generator=g) * 2 - 1) * b
    W2 = (torch.rand(1, H, generator=g) * 2 - 1) / H ** 0.5
    b2 = (torch.rand(1, generator=g) * 2 - 1) / H ** 0.5
    return codes, ei, W1, b1, W2, b2, g


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / (float(b.double().abs().max()) + 1e-30)


def _near_kink(codes, ei, W1, b1):
    """Edges with a hidden pre-activation within fp32 rounding of ReLU's kink: fp32 and fp64 may disagree on that unit's ReLU', so
    such edges carry no gradient in the comparisons (as in test_gpu_edge_score.py's endpoint-dropout test)."""
    c = codes.to(DEV).double()
    out = []
    for a in range(0, ei.shape[1], 16384):
        s, d = ei[0, a:a + 16384].to(DEV), ei[1, a:a + 16384].to(DEV)
        v = torch.cat([c[s] * c[d], c[s] - c[d]], 1) @ W1.to(DEV).double().t() + b1.to(DEV).double()
        out.append((v.abs() < 1e-5).any(1).cpu())
    return torch.cat(out)


def _oracle(codes, ei, W1, b1, W2, b2, p, keep, gp):
    """fp64 forward (all edges) and backward (upstream gradient gp) on the device."""
    leaves = [t.clone().to(DEV).double().requires_grad_(True) for t in (codes, W1, b1, W2, b2)]
    co, W1o, b1o, W2o, b2o = leaves
    eid = ei.to(DEV)
    po = O.edge_score(co[eid[0]], co[eid[1]], W1o, b1o, W2o, b2o, p, None if keep is None else keep.to(DEV)).squeeze(1)
    po.backward(gp.to(DEV).double())
    return po.detach().cpu(), [t.grad.cpu() for t in leaves]


@pytest.mark.parametrize("N,H,E", [(300, 288, 66_001), (257, 384, 3_001), (500, 512, 5_003), (200, 1024, 1_999)])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_wide_forward_and_dense_backward_vs_fp64(ops, N, H, E, p):
    """Forward over every edge and the dense backward (sgs_edge_score_bwd_core's dv form, the library dfeat GEMM, the weight-gradient
    GEMM and the endpoint reduce).  Ragged E; the 66 001-row case is past every size threshold of the H <= 256 kernels."""
    codes, ei, W1, b1, W2, b2, g = _case(N, H, E, N + H + E)
    seed, site = 4242, 2
    keep = ops.dropout_keep(seed, site, E, H, p, DEV).cpu() if p > 0 else None
    gp = torch.randn(E, generator=g)
    gp[_near_kink(codes, ei, W1, b1)] = 0.0
    po, go = _oracle(codes, ei, W1, b1, W2, b2, p, keep, gp)
    dl = [t.clone().to(DEV).requires_grad_(True) for t in (codes, W1, b1, W2, b2)]
    n0 = ops.PRECISION_COUNTS["fwd_fp32"]
    pd = ops.edge_score(*dl, ei.to(DEV), active=None, p=p, seed=seed, site=site, precision="bf16")   # bf16 falls back to fp32 here
    assert ops.PRECISION_COUNTS["fwd_fp32"] == n0 + 1
    assert float((pd.detach().cpu().double() - po).abs().max()) < 2e-6
    pd.backward(gp.to(DEV))
    for name, a, b in zip(["dcodes", "dW1", "db1", "dW2", "db2"], [t.grad for t in dl], go):
        assert bool(torch.isfinite(a).all()), name
        if name == "db2":
            assert abs(float(a) - float(b)) < 2e-6 * float(gp.abs().sum()) / 4, name
        else:
            assert _rel(a, b.reshape(a.shape)) < 2e-5, (name, _rel(a, b.reshape(a.shape)))


def test_wide_active_subset_in_shuffled_order_equals_masked_dense(ops):
    """The backward core over an active set in arbitrary order gives the dense backward's gradients with the other rows' upstream
    gradient zeroed."""
    N, H, E, q = 400, 512, 6_000, 1_500
    codes, ei, W1, b1, W2, b2, g = _case(N, H, E, 9)
    eid = torch.randperm(E, generator=g)[:q]                      # NOT sorted
    gq = torch.randn(q, generator=g)
    gp = torch.zeros(E)
    gp[eid] = gq
    res = []
    for use_active in (False, True):
        dl = [t.clone().to(DEV).requires_grad_(True) for t in (codes, W1, b1, W2, b2)]
        act = ops.ActiveSet()
        pd = ops.edge_score(*dl, ei.to(DEV), active=act, p=0.3, seed=5, site=2, pairs=None)
        if use_active:
            act.set(eid.to(DEV), ops.Graph(ei[:, eid].to(DEV), N))
        pd.backward(gp.to(DEV))
        res.append([t.grad.cpu() for t in dl])
    for a, b in zip(*res):
        assert _rel(a, b) < 1e-5


def test_wide_paired_forward_equals_plain_forward_bitwise(ops):
    """At H = 512, p = 0.3: the paired forward (canonical edges only run the contraction) gives sgs_edge_score_fwd's bits for every
    edge, on an undirected graph with one-directional extras, self loops and duplicates (unmated or mated one to one)."""
    import sgs_gnn_amd as S
    L = S._lib.lib()
    H, N = 512, 700
    assert L.sgs_edge_score_paired_supported(H) == 1
    b = S.synthetic_graph(N, 90_000, 8, 3, seed=4, device=DEV)
    g = torch.Generator().manual_seed(8)
    extra = torch.randint(0, N, (2, 3000), generator=g)
    loops = torch.arange(0, 50).repeat(2, 1)
    dup = b.edge_index[:, :500].cpu()
    ei = torch.cat([b.edge_index.cpu(), extra, loops, dup], dim=1)
    ei = ei[:, torch.argsort(ei[0] * N + ei[1], stable=True)].contiguous().to(DEV)
    E = ei.shape[1]
    codes, _, W1, b1, W2, b2, _ = _case(N, H, 10, 5)
    canon, mate = ops.get_pairs(ei, N, build=True)
    assert 0 < canon.numel() < E and int((mate[:E] < 0).sum()) > 0
    d = [t.to(DEV) for t in (codes, W1, b1, W2, b2)]
    with torch.no_grad():
        plain = ops.edge_score(*d, ei, p=0.3, seed=31, site=2, pairs=None)
        paired = ops.edge_score(*d, ei, p=0.3, seed=31, site=2, pairs=(canon, mate))
    assert torch.equal(plain, paired)
    keep = ops.dropout_keep(31, 2, E, H, 0.3, DEV)
    eic = ei
    with torch.no_grad():
        po = torch.cat([O.edge_score(d[0][eic[0, a:a + 16384]].double(), d[0][eic[1, a:a + 16384]].double(), d[1].double(), d[2].double(),
                                     d[3].double(), d[4].double(), 0.3, keep[a:a + 16384]).squeeze(1) for a in range(0, E, 16384)])
    assert float((paired.double() - po).abs().max()) < 2e-6


def test_wide_edge_id_offset_slice_equals_full_launch_bitwise(ops):
    """Dropout rows are global edge ids: scoring a slice with its offset gives the same bits as that slice of the full launch."""
    N, H, E = 300, 384, 9_001
    codes, ei, W1, b1, W2, b2, _ = _case(N, H, E, 77)
    d = [t.to(DEV) for t in (codes, W1, b1, W2, b2)]
    eid = ei.to(DEV)
    with torch.no_grad():
        full = ops.edge_score(*d, eid, p=0.3, seed=12, site=2, pairs=None)
        a, z = 2_345, 7_001
        part = ops.edge_score(*d, eid[:, a:z].contiguous(), p=0.3, seed=12, site=2, edge_id_offset=a, pairs=None)
    assert torch.equal(full[a:z], part)


def test_wide_endpoint_dropout_scorer_vs_fp64(ops):
    """EdgeProbMLP's scorer with endpoint dropout (sgs_edge_score_epd_fwd / _bwd_core, K = 2H) at H = 512, p = 0.3, backward over an
    active subset."""
    from sgs_gnn_amd.model import SITE_MLP_X, SITE_MLP_Y, SITE_SCORE
    N, H, E, q, p = 300, 512, 4_001, 1_500, 0.3
    codes, ei, W1, b1, W2, b2, g = _case(N, H, E, 200 + H)
    sx, sy, ss = 11, 12, 13
    kx, ky, kh = (ops.dropout_keep(sd, site, E, H, p, DEV) for sd, site in ((sx, SITE_MLP_X), (sy, SITE_MLP_Y), (ss, SITE_SCORE)))
    Ao = codes.clone().to(DEV).double().requires_grad_(True)
    Po = [t.clone().to(DEV).double().requires_grad_(True) for t in (W1, b1, W2, b2)]
    eo = ei.to(DEV)
    xm = Ao[eo[0]] * kx / (1 - p)
    ym = Ao[eo[1]] * ky / (1 - p)
    po = O.edge_score(xm, ym, Po[0], Po[1], Po[2], Po[3], p, kh).squeeze(1)
    dl = [t.clone().to(DEV).requires_grad_(True) for t in (codes, W1, b1, W2, b2)]
    act = ops.ActiveSet()
    pd = ops.edge_score_epd(*dl, eo, active=act, p=p, seed=ss, site=SITE_SCORE, p_ep=p, seed_x=sx, site_x=SITE_MLP_X, seed_y=sy,
                            site_y=SITE_MLP_Y)
    assert float((pd.detach().double() - po.detach()).abs().max()) < 2e-6
    eid = torch.sort(torch.randperm(E, generator=g)[:q]).values
    gp = torch.zeros(E)
    gp[eid] = torch.randn(q, generator=g)
    act.set(eid.to(DEV), ops.Graph(ei[:, eid].to(DEV), N))
    with torch.no_grad():
        vpre = torch.cat([xm * ym, xm - ym], 1) @ Po[0].t() + Po[1]
        gp[(vpre.abs() < 1e-5).any(1).cpu()] = 0.0
    po.backward(gp.to(DEV).double())
    pd.backward(gp.to(DEV))
    for name, a, b in zip(["dA", "dW1", "db1", "dW2", "db2"], [t.grad for t in dl], [Ao.grad, Po[0].grad, Po[1].grad, Po[2].grad, Po[3].grad]):
        assert bool(torch.isfinite(a).all()), name
        assert _rel(a, b.reshape(a.shape)) < 2e-5, (name, _rel(a, b.reshape(a.shape)))


def test_wide_forward_is_run_to_run_deterministic(ops):
    """Three launches at E ~ 150 000, H = 512 (plain and paired) give the same bits: the fc2 partials are summed in a fixed order."""
    import sgs_gnn_amd as S
    N, H = 5_000, 512
    b = S.synthetic_graph(N, 150_000, 8, 3, seed=21, device=DEV)
    codes, _, W1, b1, W2, b2, _ = _case(N, H, 10, 33)
    d = [t.to(DEV) for t in (codes, W1, b1, W2, b2)]
    pairs = ops.get_pairs(b.edge_index, N, build=True)
    for pr in (None, pairs):
        with torch.no_grad():
            outs = [ops.edge_score(*d, b.edge_index, p=0.3, seed=3, site=2, pairs=pr).clone() for _ in range(3)]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
