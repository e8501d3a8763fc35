"""GPU: every form of the edge scorer, run-to-run bit-identical and against fp64, at a size where the codes table is not L2-resident.

Config 4's partition shape (n = 33 869, E ~ 463 k; the codes table is 34 MB at H = 256) with q = 100 000 drawn active rows.  Each form
runs 20 times and must give the same bits every time; its first run is held once to an fp64 reference evaluated on the device (for the
bf16 mode: the fp64 evaluation of the bf16-ROUNDED operands, as tests/test_gpu_scorer_bf16.py) at the existing tests' tolerances.  Mask
words are compared bit for bit with the fp64-derived ReLU x dropout mask, excluding only units whose pre-activation lies within an
fp32-rounding margin of 0.  A last case repeats the forms while another stream runs large device-to-device copies (uneven memory
timing) and asks for the same bits again.

Forms: forward unpaired (MODE 0), paired (MODE 3), mask-keeping (unpaired and paired), fp32 and bf16; backward core variants 0 / 3 / 4
(pinned through sgs_edge_score_set_bwd_variant) and the mask-form core; sgs_edge_score_bwd_dfeat_fused_packed(_bf16); the shared-operand
weight gradient sgs_gemm_tn_mask_gather(_bf16).  H in {128, 256}, p in {0, 0.3}."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUNS = 20
N_NODES, E_TARGET, Q = 33_869, 463_000, 100_000
SEED, SITE = 3, 2


@pytest.fixture(scope="module")
def S():
    import sgs_gnn_amd
    yield sgs_gnn_amd
    _CASES.clear()                                   # the fp64 tables (~3 GB) do not outlive the module


def _bf(t):
    """RNE to bf16 and back, in fp64 (as pk_bf16)."""
    return t.float().to(torch.bfloat16).to(torch.float64)


def _unpack(bits, H):
    """int32 [R, H / 32] mask words -> bool [R, H] (bit h of row r in word h / 32)."""
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits.unsqueeze(2) >> sh) & 1).reshape(bits.shape[0], H).bool()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-30)


def _repeat(fn, outs):
    """fn() writes `outs` (a list of tensors); run it RUNS times and return the first run's values after checking every later run
    gives the same bits."""
    fn()
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    for it in range(1, RUNS):
        fn()
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(outs, first)):
            if not torch.equal(a, b):
                raise AssertionError(f"run {it}, output {k}: {int((a != b).sum())} of {a.numel()} elements differ from run 0")
    return first


_CASES = {}


def _case(S, H):
    """Inputs and the two fp64 pre-activation tables (fp32 function; bf16 mode) of every scored edge, built once per H."""
    if H in _CASES:
        return _CASES[H]
    ops = S.ops
    b = S.synthetic_graph(N_NODES, E_TARGET, 8, 5, seed=300, train_frac=0.2, power=0.6, device=DEV)
    ei = b.edge_index.contiguous()
    E = ei.shape[1]
    assert ops.src_sorted(ei) and E > 400_000
    g = torch.Generator(device=DEV).manual_seed(H)
    c = dict(H=H, ei=ei, E=E)
    c["codes"] = torch.relu(torch.randn(N_NODES, H, device=DEV, generator=g))
    c["W1"] = torch.randn(H, 2 * H, device=DEV, generator=g) / (2 * H) ** 0.5
    c["b1"] = torch.randn(H, device=DEV, generator=g) * 0.05
    c["w2"] = torch.randn(H, device=DEV, generator=g) / H ** 0.5
    c["b2"] = torch.randn(1, device=DEV, generator=g) * 0.1
    c["U"] = torch.mm(c["codes"], c["W1"][:, H:].t()).contiguous()                 # the fp32 library GEMM, as ops.edge_score
    c["pairs"] = ops.get_pairs(ei, N_NODES, build=True)
    c["eid"] = torch.sort(torch.randperm(E, device=DEV, generator=g)[:Q]).values
    c["gq"] = torch.randn(Q, device=DEV, generator=g)
    c32, W1a = c["codes"], c["W1"][:, :H]
    c64 = c32.double()
    U64 = c64 @ c["W1"][:, H:].double().t()
    Ws, Wb = W1a.double().t(), _bf(W1a).t()
    v64, vbf = torch.empty(E, H, dtype=torch.float64, device=DEV), torch.empty(E, H, dtype=torch.float64, device=DEV)
    for a in range(0, E, 65536):
        s, d = ei[0, a:a + 65536], ei[1, a:a + 65536]
        v64[a:a + 65536] = (c64[s] * c64[d]) @ Ws + (U64[s] - U64[d]) + c["b1"].double()
        vbf[a:a + 65536] = _bf(c32[s] * c32[d]) @ Wb + (c["U"][s] - c["U"][d]).double() + c["b1"].double()
    c["v"] = {"fp32": v64, "bf16": vbf}
    _CASES[H] = c
    return c


def _want(c, prec, p):
    """(probabilities [E], mask [E, H], clear [E, H]) of the fp64 reference: clear = |v| outside the rounding margin of 0."""
    v = c["v"][prec]
    keep = c["_keep"] if p > 0 else None
    on = v > 0
    if keep is not None:
        on &= keep
    scale = 1.0 / (1.0 - p)
    z = (torch.where(on, v, torch.zeros((), dtype=torch.float64, device=DEV)) * scale) @ c["w2"].double() + float(c["b2"])
    clear = v.abs() > (1e-5 if prec == "fp32" else 2e-6)
    return torch.sigmoid(z), on, clear


def _ws(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=DEV)


# ----------------------------------------------------------------------------------------------------------------------------------
# forward

def _forward_forms(S, c, p, prec):
    """{form: (fn, outputs)} for the four forward forms of one precision."""
    L, ops = S._lib.lib(), S.ops
    H, E, ei = c["H"], c["E"], c["ei"]
    canon, mate = c["pairs"]
    P = ops._ptr
    sfx = "_bf16" if prec == "bf16" else ""
    ws = _ws(L.sgs_edge_score_workspace_bytes(N_NODES, H, E))
    common = (P(c["W1"]), P(c["b1"]), P(c["w2"]), P(c["b2"]), float(p), SEED, SITE)
    head = (P(c["codes"]), P(c["U"]), N_NODES, H, P(ei), E, 0)
    forms = {}
    o = torch.empty(E, device=DEV)
    forms["plain"] = (lambda o=o: S._lib.check(getattr(L, "sgs_edge_score_fwd" + sfx)(*head, *common, P(o), ws.data_ptr(), ws.numel(), ops._stream()),
                                               "fwd"), [o])
    o = torch.empty(E, device=DEV)
    forms["paired"] = (lambda o=o: S._lib.check(getattr(L, "sgs_edge_score_fwd_paired" + sfx)(*head, P(canon), canon.numel(), P(mate), *common, P(o),
                                                                                                ws.data_ptr(), ws.numel(), ops._stream()), "fwd_paired"), [o])
    for name, pr in (("mask", None), ("mask_paired", (canon, mate))):
        o, bits = torch.empty(E, device=DEV), torch.empty(E, H // 32, dtype=torch.int32, device=DEV)
        cn, mt = pr if pr is not None else (None, None)
        forms[name] = (lambda o=o, bits=bits, cn=cn, mt=mt: S._lib.check(getattr(L, "sgs_edge_score_fwd_mask" + sfx)(
            *head, P(cn), 0 if cn is None else cn.numel(), P(mt), *common, P(o), P(bits), ws.data_ptr(), ws.numel(), ops._stream()), "fwd_mask"),
            [o, bits])
    return forms, ws


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_forms_deterministic_and_exact(S, H, p, prec):
    L = S._lib.lib()
    L.sgs_edge_score_set_variant(4)                 # the bf16x6 loop (the production forward at this size), pinned
    try:
        c = _case(S, H)
        c["_keep"] = S.ops.dropout_keep(SEED, SITE, c["E"], H, p, DEV) if p > 0 else None
        want, on, clear = _want(c, prec, p)
        assert float(clear.double().mean()) > 0.999
        forms, _ = _forward_forms(S, c, p, prec)
        res = {name: _repeat(fn, outs) for name, (fn, outs) in forms.items()}
    finally:
        L.sgs_edge_score_set_variant(-1)
    for name, outs in res.items():
        err = float((outs[0].double() - want).abs().max())
        assert err < 2e-6, (name, err)
        if len(outs) > 1:
            got = _unpack(outs[1], H)
            bad = int(((got != on) & clear).sum())
            assert bad == 0, f"{name}: {bad} mask bits differ from the fp64 ReLU x dropout mask"
    assert torch.equal(res["plain"][0], res["paired"][0]) and torch.equal(res["plain"][0], res["mask_paired"][0])
    assert torch.equal(res["mask"][0], res["plain"][0]) and torch.equal(res["mask"][1], res["mask_paired"][1])


# ----------------------------------------------------------------------------------------------------------------------------------
# backward core (recompute), every selectable variant, and the mask-form core

@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_backward_core_variants_deterministic_and_exact(S, H, p):
    L, ops = S._lib.lib(), S.ops
    c = _case(S, H)
    c["_keep"] = ops.dropout_keep(SEED, SITE, c["E"], H, p, DEV) if p > 0 else None
    want, on, clear = _want(c, "fp32", p)
    eid, gq, ei = c["eid"], c["gq"], c["ei"]
    P = ops._ptr
    f32 = dict(dtype=torch.float32, device=DEV)
    tile = L.sgs_edge_score_bwd_tile()
    ws = _ws(L.sgs_edge_score_workspace_bytes(N_NODES, H, 0))
    args = (P(c["codes"]), P(c["U"]), N_NODES, H, P(ei), c["E"], 0, P(eid), Q, P(gq), P(c["W1"]), P(c["b1"]), P(c["w2"]), P(c["b2"]), float(p),
            SEED, SITE)
    res = {}
    try:
        for variant in (0, 3, 4):
            L.sgs_edge_score_set_bwd_variant(variant)
            assert L.sgs_edge_score_get_bwd_variant() == variant
            dv, hdz, dz, feat = torch.empty(Q, H, **f32), torch.empty((Q + tile - 1) // tile, H, **f32), torch.empty(Q, **f32), torch.empty(Q, H, **f32)
            fn = (lambda dv=dv, hdz=hdz, dz=dz, feat=feat: S._lib.check(L.sgs_edge_score_bwd_core(
                *args, P(dv), P(hdz), P(dz), P(feat), ws.data_ptr(), ws.numel(), ops._stream()), "bwd_core"))
            res[variant] = _repeat(fn, [dv, hdz, dz, feat])
        L.sgs_edge_score_set_bwd_variant(-1)
        bits, hdz, dz, feat = torch.empty(Q, H // 32, dtype=torch.int32, device=DEV), torch.empty((Q + tile - 1) // tile, H, **f32), torch.empty(Q, **f32), torch.empty(Q, H, **f32)
        fn = (lambda: S._lib.check(L.sgs_edge_score_bwd_core_bits(*args, P(bits), P(hdz), P(dz), P(feat), ws.data_ptr(), ws.numel(), ops._stream()),
                                   "bwd_core_bits"))
        res["bits"] = _repeat(fn, [bits, hdz, dz, feat])
    finally:
        L.sgs_edge_score_set_bwd_variant(-1)
    s, d = ei[0, eid], ei[1, eid]
    pe = want[eid]
    dz64 = gq.double() * pe * (1 - pe)
    v, m, cl = c["v"]["fp32"][eid], on[eid], clear[eid]
    scale = 1.0 / (1.0 - p)
    dv64 = dz64[:, None] * m.double() * (c["w2"].double() * scale)
    dw2_64 = (dz64[:, None] * torch.where(m, v, torch.zeros((), dtype=torch.float64, device=DEV)) * scale).sum(0)
    feat32 = c["codes"][s] * c["codes"][d]
    for form, outs in res.items():
        rdv, rhdz, rdz, rfeat = outs
        assert torch.equal(rfeat, feat32), form
        assert _rel(rdz, dz64) < 2e-5, (form, _rel(rdz, dz64))
        assert _rel(rhdz.double().sum(0), dw2_64) < 2e-5, (form, _rel(rhdz.double().sum(0), dw2_64))
        if form == "bits":
            bad = int(((_unpack(rdv, H) != m) & cl).sum())
            assert bad == 0, f"mask-form core: {bad} dv bits differ from the fp64 mask"
        else:
            err = float(((rdv.double() - dv64).abs() * cl).max()) / float(dv64.abs().max())
            assert err < 2e-5, (form, err)


# ----------------------------------------------------------------------------------------------------------------------------------
# the fused backward's dfeat contraction and the shared-operand weight gradient, fp32 and bf16

def _prep(S, c, p, prec):
    """The forward that keeps the mask (paired), then sgs_edge_score_bwd_prep_sd_pack(_bf16): (bits, dz, sd, ws holding the operand)."""
    L, ops = S._lib.lib(), S.ops
    P = ops._ptr
    H, E, ei = c["H"], c["E"], c["ei"]
    sfx = "_bf16" if prec == "bf16" else ""
    canon, mate = c["pairs"]
    pout, maskbits = torch.empty(E, device=DEV), torch.empty(E, H // 32, dtype=torch.int32, device=DEV)
    wsf = _ws(L.sgs_edge_score_workspace_bytes(N_NODES, H, E))
    S._lib.check(getattr(L, "sgs_edge_score_fwd_mask" + sfx)(P(c["codes"]), P(c["U"]), N_NODES, H, P(ei), E, 0, P(canon), canon.numel(), P(mate),
                                                             P(c["W1"]), P(c["b1"]), P(c["w2"]), P(c["b2"]), float(p), SEED, SITE, P(pout),
                                                             P(maskbits), wsf.data_ptr(), wsf.numel(), ops._stream()), "fwd_mask")
    bits, dz = torch.empty(Q, H // 32, dtype=torch.int32, device=DEV), torch.empty(Q, device=DEV)
    sd = torch.empty(Q, 2, dtype=torch.int32, device=DEV)
    wsd = _ws(L.sgs_edge_score_workspace_bytes(0, H, 0))
    S._lib.check(getattr(L, "sgs_edge_score_bwd_prep_sd_pack" + sfx)(P(c["codes"]), N_NODES, H, P(ei), E, P(c["eid"]), Q, P(c["gq"]), P(pout),
                                                                     P(maskbits), P(dz), P(bits), P(sd), P(c["W1"]), P(c["w2"]), float(p),
                                                                     wsd.data_ptr(), wsd.numel(), ops._stream()), "prep_sd_pack")
    torch.cuda.synchronize()
    return bits, dz, sd, wsd, pout


def _fused_forms(S, c, p, prec, prep):
    L, ops = S._lib.lib(), S.ops
    P = ops._ptr
    H = c["H"]
    sfx = "_bf16" if prec == "bf16" else ""
    bits, dz, sd, wsd, _ = prep
    G = torch.empty(Q, H, device=DEV)
    opart = torch.zeros(L.sgs_edge_score_bwd_fused_opart_rows(Q, N_NODES), H, device=DEV)
    f_dfeat = (lambda: S._lib.check(getattr(L, "sgs_edge_score_bwd_dfeat_fused_packed" + sfx)(
        P(bits), P(dz), P(sd), P(c["codes"]), Q, N_NODES, H, P(G), P(opart), wsd.data_ptr(), wsd.numel(), ops._stream()), "dfeat_fused_packed"))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    C = torch.full((H, 2 * H), 7.0, device=DEV)
    cs, dzs, Craw, csraw = torch.empty(H, device=DEV), torch.empty(1, device=DEV), torch.empty(H, H, device=DEV), torch.empty(H, device=DEV)
    wsg = _ws(L.sgs_gemm_tn_workspace_bytes(Q, H, H))
    assert L.sgs_gemm_tn_mask_supported(Q, H, H)
    f_gemm = (lambda: S._lib.check(getattr(L, "sgs_gemm_tn_mask_gather" + sfx)(
        P(bits), P(dz), P(c["w2"]), scale, P(c["codes"]), N_NODES, P(sd), Q, H, H, P(C), 2 * H, P(cs), P(dzs), P(Craw), P(csraw), wsg.data_ptr(),
        wsg.numel(), ops._stream()), "gather"))
    return {"dfeat": (f_dfeat, [G, opart]), "gemm": (f_gemm, [C, cs, dzs, Craw, csraw])}


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fused_dfeat_and_gather_gradient_deterministic_and_exact(S, H, p, prec):
    L, ops = S._lib.lib(), S.ops
    c = _case(S, H)
    c["_keep"] = ops.dropout_keep(SEED, SITE, c["E"], H, p, DEV) if p > 0 else None
    want, on, clear = _want(c, prec, p)
    prep = _prep(S, c, p, prec)
    bits, dz, sd, _, pout = prep
    eid, ei = c["eid"], c["ei"]
    s, d = ei[0, eid], ei[1, eid]
    # the prep: the active rows' endpoints and mask, dz from the forward's own p
    assert torch.equal(sd.long(), torch.stack([s, d], 1)) and torch.equal(dz, c["gq"] * pout[eid] * (1.0 - pout[eid]))
    m = _unpack(bits, H)
    assert int(((m != on[eid]) & clear[eid]).sum()) == 0
    L.sgs_gemm_tn_set_gather_variant(1, 0)                          # the shared-operand kernel (the default), pinned
    res = {name: _repeat(fn, outs) for name, (fn, outs) in _fused_forms(S, c, p, prec, prep).items()}
    # fp64 references on the kernels' own mask and dz (the backward is defined given what the forward kept)
    rnd = _bf if prec == "bf16" else (lambda t: t.double())
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    w2 = c["w2"]
    md, dz64 = m.double(), dz.double()
    Wd32 = c["W1"][:, :H] * (w2 * np.float32(scale)).reshape(-1, 1)          # diag(w2 / (1 - p)) W1a, formed in fp32 as the pack forms it
    dfeat = dz64[:, None] * (md @ rnd(Wd32))
    c64 = c["codes"].double()
    G, opart = res["dfeat"]
    assert _rel(G, dfeat * c64[s]) < 3e-6, _rel(G, dfeat * c64[s])
    r = torch.arange(Q, device=DEV)
    is_end = torch.ones(Q, dtype=torch.bool, device=DEV)
    is_end[:-1] = (s[1:] != s[:-1]) | (r[:-1] % 32 == 31)
    slots = (r[is_end] >> 5) + s[is_end]
    got = torch.zeros(N_NODES, H, dtype=torch.float64, device=DEV).index_add_(0, s[is_end], opart[slots].double())
    ref = torch.zeros(N_NODES, H, dtype=torch.float64, device=DEV).index_add_(0, s, dfeat * c64[d])
    assert _rel(got, ref) < 3e-6, _rel(got, ref)
    B32 = (c["codes"][s] * c["codes"][d]) * dz[:, None]                        # dz * feat, formed in fp32 as the GEMM forms it
    T = md.t() @ rnd(B32)
    csr = (md * dz64[:, None]).sum(0)
    C, cs, dzs, Craw, csraw = res["gemm"]
    assert torch.all(C[:, H:] == 7.0)
    tol = 3e-6 if prec == "bf16" else 2e-6
    for name, a, b in (("C", C[:, :H], (w2.double() * scale)[:, None] * T), ("colsum", cs, csr * w2.double() * scale), ("Craw", Craw, T),
                       ("colsum_raw", csraw, csr)):
        assert _rel(a, b) < tol, (name, _rel(a, b))
    assert abs(float(dzs) - float(dz64.sum())) < 2e-6 * float(dz64.abs().sum())


# ----------------------------------------------------------------------------------------------------------------------------------
# uneven memory timing: the same forms beside a stream of large device-to-device copies

def test_forms_are_bit_identical_beside_a_copy_stream(S):
    L, ops = S._lib.lib(), S.ops
    H, p = 256, 0.3
    c = _case(S, H)
    outs = {}
    side = torch.cuda.Stream()
    src = torch.empty(1 << 29, dtype=torch.float32, device=DEV).fill_(1.0)    # 2 GiB each way: far more than the L2 and the MALL
    dst = torch.empty_like(src)
    L.sgs_edge_score_set_variant(4)
    try:
        for prec in ("fp32", "bf16"):
            prep = _prep(S, c, p, prec)
            forms = dict(_forward_forms(S, c, p, prec)[0])
            forms.update(_fused_forms(S, c, p, prec, prep))
            for name, (fn, o) in forms.items():
                fn()
                torch.cuda.synchronize()
                base = [t.clone() for t in o]
                for it in range(RUNS // 2):
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        dst.copy_(src)
                        dst.copy_(src)
                    fn()                                                     # launched while the copies are running
                    torch.cuda.current_stream().wait_stream(side)
                    torch.cuda.synchronize()
                    for k, (a, b) in enumerate(zip(o, base)):
                        if not torch.equal(a, b):
                            raise AssertionError(f"{prec} {name}, loaded run {it}, output {k}: {int((a != b).sum())} of {a.numel()} elements differ")
                outs[(prec, name)] = True
    finally:
        L.sgs_edge_score_set_variant(-1)
    assert len(outs) == 12
