"""GPU: the fused scorer backward with the MODE 5 operand packed by the prep launch (sgs_edge_score_bwd_prep_sd_pack +
sgs_edge_score_bwd_dfeat_fused_packed) -- against the entry points it replaces bit for bit, against the unfused form through autograd, run to
run, and replayed from a captured graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    import sgs_gnn_amd
    return sgs_gnn_amd


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-30)


def _inputs(N, H, q, p, seed=71):
    """A row-sorted edge list with a hub source, q active rows drawn from it in edge order, and what the forward kept."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    E = 3 * q + 7
    ei = torch.randint(0, N, (2, E), device=DEV, generator=g)
    ei[0, : E // 20] = 3
    ei = ei[:, torch.argsort(ei[0] * N + ei[1], stable=True)].contiguous()
    eid = torch.sort(torch.randperm(E, device=DEV, generator=g)[:q]).values
    t = dict(
        N=N, H=H, q=q, p=p, E=E, ei=ei, eid=eid,
        codes=torch.relu(torch.randn(N, H, device=DEV, generator=g)),
        W1=torch.randn(H, 2 * H, device=DEV, generator=g) / (2 * H) ** 0.5,
        b1=torch.randn(H, device=DEV, generator=g) / H ** 0.5,
        w2=torch.randn(H, device=DEV, generator=g) / H ** 0.5,
        U=torch.randn(N, H, device=DEV, generator=g),
        gp=torch.randn(q, device=DEV, generator=g),
        p_out=torch.rand(E, device=DEV, generator=g),
        maskbits=torch.randint(-2**31, 2**31 - 1, (E, H // 32), device=DEV, generator=g, dtype=torch.int64).to(torch.int32),
    )
    return t


class _Chain:
    """The five launches of the chain through the C ABI, into buffers allocated once (so that a captured graph can replay them)."""

    def __init__(self, S, t):
        self.S, self.L, self.t = S, S._lib.lib(), t
        L, N, H, q = self.L, t["N"], t["H"], t["q"]
        f32 = dict(dtype=torch.float32, device=DEV)
        self.graph = S.ops.Graph(t["ei"][:, t["eid"]].contiguous(), N)
        self.dz, self.bits = torch.empty(q, **f32), torch.empty(q, H // 32, dtype=torch.int32, device=DEV)
        self.sd = torch.empty(q, 2, dtype=torch.int32, device=DEV)
        self.G, self.opart = torch.empty(q, H, **f32), torch.empty(L.sgs_edge_score_bwd_fused_opart_rows(q, N), H, **f32)
        self.dW1, self.db1, self.db2 = torch.empty(H, 2 * H, **f32), torch.empty(H, **f32), torch.empty(1, **f32)
        self.Traw, self.craw = torch.empty(H, H, **f32), torch.empty(H, **f32)
        self.dcodes, self.dU, self.Rraw, self.dw2 = torch.empty(N, H, **f32), torch.empty(N, H, **f32), torch.empty(N, H, **f32), torch.empty(H, **f32)
        self.wsd = torch.empty(L.sgs_edge_score_workspace_bytes(0, H, 0), dtype=torch.uint8, device=DEV)
        self.wsg = torch.empty(L.sgs_gemm_tn_workspace_bytes(q, H, H), dtype=torch.uint8, device=DEV)

    def outputs(self):
        H = self.t["H"]                                # (d W1's right half is the node-level tail's, not the chain's)
        return [x.clone() for x in (self.dz, self.bits, self.sd, self.G, self.dW1[:, :H], self.db1, self.db2, self.Traw, self.craw, self.dcodes,
                                    self.dU, self.Rraw, self.dw2)]

    def run(self, full=True):
        """full = False: the two launches of the fused pair only (prep + dfeat; the weight-gradient GEMM serves tall shapes alone)."""
        S, L, t = self.S, self.L, self.t
        ck, st = S._lib.check, S.ops._stream()
        N, H, q, p, E = t["N"], t["H"], t["q"], t["p"], t["E"]
        ck(L.sgs_edge_score_bwd_prep_sd_pack(t["codes"].data_ptr(), N, H, t["ei"].data_ptr(), E, t["eid"].data_ptr(), q, t["gp"].data_ptr(),
                                             t["p_out"].data_ptr(), t["maskbits"].data_ptr(), self.dz.data_ptr(), self.bits.data_ptr(),
                                             self.sd.data_ptr(), t["W1"].data_ptr(), t["w2"].data_ptr(), p, self.wsd.data_ptr(), self.wsd.numel(), st),
           "prep_sd_pack")
        ck(L.sgs_edge_score_bwd_dfeat_fused_packed(self.bits.data_ptr(), self.dz.data_ptr(), self.sd.data_ptr(), t["codes"].data_ptr(), q, N, H,
                                                   self.G.data_ptr(), self.opart.data_ptr(), self.wsd.data_ptr(), self.wsd.numel(), st),
           "dfeat_fused_packed")
        if not full:
            return
        scale = 1.0 / (1.0 - p)
        ck(L.sgs_gemm_tn_mask_gather(self.bits.data_ptr(), self.dz.data_ptr(), t["w2"].data_ptr(), scale, t["codes"].data_ptr(), N, self.sd.data_ptr(),
                                     q, H, H, self.dW1.data_ptr(), 2 * H, self.db1.data_ptr(), self.db2.data_ptr(), self.Traw.data_ptr(),
                                     self.craw.data_ptr(), self.wsg.data_ptr(), self.wsg.numel(), st), "gemm_tn_mask_gather")
        gr = self.graph
        ck(L.sgs_edge_score_bwd_reduce_fused(self.G.data_ptr(), self.opart.data_ptr(), self.bits.data_ptr(), self.dz.data_ptr(), t["w2"].data_ptr(), p,
                                             N, H, q, gr.in_ptr.data_ptr(), gr.in_eid.data_ptr(), gr.out_ptr.data_ptr(), self.dcodes.data_ptr(),
                                             self.dU.data_ptr(), self.Rraw.data_ptr(), st), "reduce_fused")
        ck(L.sgs_edge_score_dw2_from_parts(t["W1"].data_ptr(), self.Traw.data_ptr(), t["U"].data_ptr(), self.Rraw.data_ptr(), t["b1"].data_ptr(),
                                           self.craw.data_ptr(), N, H, p, self.dw2.data_ptr(), st), "dw2_from_parts")


@pytest.mark.parametrize("H,p,q", [(256, 0.3, 100_000), (128, 0.0, 70_001), (256, 0.0, 95)])
def test_packed_chain_equals_separate_pack_bit_for_bit(S, H, p, q):
    """prep_sd_pack == prep_sd (dz, mask rows, endpoints) and dfeat_fused_packed == dfeat_fused (G, opart's run-end rows), bit for bit: the pack
    made inside the prep launch is the separate pack.  (Both dfeat entry points run the same MODE 5 kernel; its epilogue -- the slice-ahead
    endpoint gathers -- is pinned by test_gpu_edge_score.py::test_fused_dfeat_entry_point_by_source_partials_and_G, G == dfeat * codes[src] bit
    for bit against the unfused dfeat, and by the comparison with the unfused backward below.)"""
    N = 1013
    t = _inputs(N, H, q, p)
    ch = _Chain(S, t)
    ch.run(full=False)
    L, ck, st = ch.L, S._lib.check, S.ops._stream()
    f32 = dict(dtype=torch.float32, device=DEV)
    dz, bits, sd = torch.empty(q, **f32), torch.empty(q, H // 32, dtype=torch.int32, device=DEV), torch.empty(q, 2, dtype=torch.int32, device=DEV)
    ck(L.sgs_edge_score_bwd_prep_sd(t["codes"].data_ptr(), N, H, t["ei"].data_ptr(), t["E"], t["eid"].data_ptr(), q, t["gp"].data_ptr(),
                                    t["p_out"].data_ptr(), t["maskbits"].data_ptr(), dz.data_ptr(), bits.data_ptr(), sd.data_ptr(), st), "prep_sd")
    dz2, bits2, feat = torch.empty(q, **f32), torch.empty(q, H // 32, dtype=torch.int32, device=DEV), torch.empty(q, H, **f32)
    ck(L.sgs_edge_score_bwd_prep(t["codes"].data_ptr(), N, H, t["ei"].data_ptr(), t["E"], t["eid"].data_ptr(), q, t["gp"].data_ptr(),
                                 t["p_out"].data_ptr(), t["maskbits"].data_ptr(), dz2.data_ptr(), bits2.data_ptr(), feat.data_ptr(), st), "prep")
    G = torch.full((q, H), float("nan"), **f32)
    opart = torch.full_like(ch.opart, float("nan"))
    ws = torch.empty(L.sgs_edge_score_workspace_bytes(0, H, 0), dtype=torch.uint8, device=DEV)
    ck(L.sgs_edge_score_bwd_dfeat_fused(ch.bits.data_ptr(), ch.dz.data_ptr(), ch.sd.data_ptr(), t["codes"].data_ptr(), q, N, H, t["W1"].data_ptr(),
                                        t["w2"].data_ptr(), p, G.data_ptr(), opart.data_ptr(), ws.data_ptr(), ws.numel(), st), "dfeat_fused")
    torch.cuda.synchronize()
    src, dst = t["ei"][0, t["eid"]], t["ei"][1, t["eid"]]
    assert torch.equal(ch.sd[:, 0].long(), src) and torch.equal(ch.sd[:, 1].long(), dst) and torch.equal(ch.sd, sd)
    assert torch.equal(ch.bits, t["maskbits"][t["eid"]]) and torch.equal(ch.bits, bits) and torch.equal(bits, bits2)
    assert torch.equal(ch.dz, dz) and torch.equal(dz, dz2)
    assert torch.equal(ch.G, G)
    r = torch.arange(q, device=DEV)
    is_end = torch.ones(q, dtype=torch.bool, device=DEV)
    is_end[:-1] = (src[1:] != src[:-1]) | (r[:-1] % 32 == 31)
    slots = (r[is_end] >> 5) + src[is_end]
    assert bool(torch.isfinite(opart[slots]).all())
    assert torch.equal(ch.opart[slots], opart[slots])


@pytest.mark.parametrize("H,p", [(256, 0.0), (256, 0.3), (128, 0.0), (128, 0.3)])
def test_chain_is_run_to_run_deterministic_and_replays_from_a_graph(S, H, p):
    """Two eager calls give bitwise equal results; the chain captured in a CUDA graph and replayed three times gives them again."""
    t = _inputs(1013, H, 100_000, p)
    ch = _Chain(S, t)
    ch.run()
    torch.cuda.synchronize()
    first = ch.outputs()
    ch.run()
    torch.cuda.synchronize()
    second = ch.outputs()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    for x in (ch.dz, ch.G, ch.dW1, ch.dcodes, ch.dU, ch.dw2):
        x.fill_(float("nan"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # (warm-up off the legacy stream, as torch.cuda.graph wants)
        ch.run()
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ch.run()
    for _ in range(3):
        for x in (ch.dz, ch.G, ch.dW1, ch.dcodes, ch.dU, ch.dw2):
            x.fill_(float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, ch.outputs()):
            assert torch.equal(a, b)


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_fused_chain_equals_unfused_backward_at_partition_size(S, H, p):
    """The scorer's backward through autograd at a Reddit partition's shape (N = 1 013, q = 100 000): the fused chain against the unfused
    mask form (feat / dfeat as [n, H] arrays) on the same inputs; and two fused backwards are bitwise equal."""
    ops = S.ops
    N, q = 1013, 100_000
    t = _inputs(N, H, q, p, seed=5)
    E, ei, eid = t["E"], t["ei"], t["eid"]
    g = torch.Generator(device=DEV).manual_seed(9)
    gp = torch.zeros(E, device=DEV)
    gp[eid] = torch.randn(q, device=DEV, generator=g)
    b2 = torch.randn(1, device=DEV, generator=g)
    assert ops.src_sorted(ei)
    grads = {}
    for form, fused in (("fused", True), ("fused_again", True), ("unfused", False)):
        ops._fused_backward = fused
        try:
            dl = [x.clone().requires_grad_(True) for x in (t["codes"], t["W1"], t["b1"], t["w2"].reshape(1, -1), b2)]
            act = ops.ActiveSet()
            pd = ops.edge_score(dl[0], dl[1], dl[2], dl[3], dl[4], ei, active=act, p=p, seed=5, site=2)
            act.set(eid, ops.Graph(ei[:, eid].contiguous(), N))
            pd.backward(gp)
            torch.cuda.synchronize()
            grads[form] = [x.grad.detach().clone() for x in dl]
        finally:
            ops._fused_backward = True
    for a, b in zip(grads["fused"], grads["fused_again"]):
        assert torch.equal(a, b)
    for name, a, b in zip(["dcodes", "dW1", "db1", "dw2", "db2"], grads["fused"], grads["unfused"]):
        assert bool(torch.isfinite(a).all()), name
        assert _rel(a, b) < (2e-5 if name in ("dw2", "db2") else 3e-6), (name, _rel(a, b))
    assert _rel(grads["fused"][1][:, :H], grads["unfused"][1][:, :H]) < 2e-6
    assert _rel(grads["fused"][2], grads["unfused"][2]) < 2e-6
