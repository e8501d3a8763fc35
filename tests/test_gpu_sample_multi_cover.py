"""GPU: sgs_sample_topq_multi_cover through the C ABI and through ops.sample_topq_multi(..., cover=).

Two independent checks per draw d of a call:
  * row d of every output is torch.equal to the single covering call (ops.sample_topq(..., cover=), then ops.st_weights) for stream id
    SID0 + d or noise row d: mask, eid, edge_index, stats as int32 bits, w as int32 bits, cover_info;
  * row d equals tests/cover_ref.py applied to the PLAIN single call's keys_out for that stream (integer logic, so exact).
The single calls and the references of a configuration are computed once for 11 streams and shared by every D (rows 0 .. D-1)."""
import functools

import numpy as np
import pytest
import torch

import cover_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, SID0, C = 4321, 55, 0.3
DMAX = 11
DS = (1, 2, 5, 11)                                  # 5 and 11 leave a partial last group of 4


@pytest.fixture(scope="module")
def S():
    import sgs_gnn_amd
    return sgs_gnn_amd


@pytest.fixture(scope="module")
def ops(S):
    return S.ops


# ------------------------------------------------------------------ inputs (the recipe of tests/test_gpu_cover.py, copied)
def _graph(E, N, M, seed):
    """E edges over N nodes of which exactly M have a non-loop in-edge (M <= min(N, E); M >= 1 needs N >= 2): every edge points at
    one of M destination nodes, each of which is guaranteed one edge from another node; about a tenth of the rest are self-loops."""
    g = np.random.default_rng(seed)
    if M == 0:
        d = g.integers(0, N, E)
        return torch.from_numpy(np.stack([d, d]))
    D = g.permutation(N)[:M]
    dst = np.concatenate([D, D[g.integers(0, M, E - M)]])
    src = g.integers(0, N, E)
    src[:M] = (D + 1 + g.integers(0, N - 1, M)) % N                  # != dst
    loop = g.random(E) < 0.1
    loop[:M] = False
    src[loop] = dst[loop]
    perm = g.permutation(E)
    return torch.from_numpy(np.stack([src[perm], dst[perm]]))


KINDS = ("M<q", "M=q", "M>q")


def _target_M(E, q, N, kind):
    """The M that makes the case, or None where the shape cannot have it (M <= min(N, E))."""
    top = min(N, E)
    M = {"M<q": min(q // 2, top), "M=q": q, "M>q": min(top, 2 * q + 1)}[kind]
    ok = {"M<q": M < q, "M=q": M == q, "M>q": M > q}[kind] and M <= top
    return M if ok else None


SMALL = [(7, 3, 5), (2049, 1, 300), (4097, 2000, 4097), (100_003, 20_000, 20_000)]
LARGE = (2_097_153, 400_000, 50_000)                # the one shape on the large-E path, at D = 3 only
CASES = [(E, q, N, k) for E, q, N in SMALL + [LARGE] for k in KINDS if _target_M(E, q, N, k) is not None]


def test_the_cases_cover_every_kind_and_both_paths(S):
    assert {k for *_, k in CASES} == set(KINDS)
    assert {(E, q, N) for E, q, N, _ in CASES} == set(SMALL + [LARGE])
    assert [E > 1024 * 2048 for E, _, _ in SMALL + [LARGE]] == [False] * 4 + [True]
    assert 100_003 % 64 != 0                                          # the padded key stride differs from E there


def _scores(mode, E, seed):
    g = torch.Generator().manual_seed(seed)
    if mode == "learned":
        return torch.sigmoid(torch.randn(E, generator=g))
    if mode == "prior":
        return torch.randn(E, generator=g)
    return None


def _kind(ops, mode):
    return ops.SAMPLE_PRIOR if mode == "prior" else ops.SAMPLE_LEARNED


class _Cfg:
    """One configuration's inputs on the device, its single covering calls and its references for streams SID0 .. SID0 + n - 1."""


def _singles(ops, ei, N, q, mode, p, noise, n):
    """-> _Cfg: r[d] (single covering call + w), ref[d] (cover_ref over the PLAIN call's keys), for d < n."""
    c = _Cfg()
    E = ei.shape[1]
    c.E, c.N, c.q, c.mode, c.n = E, N, q, mode, n
    c.ei_cpu = ei
    c.ei = ei.to(DEV).contiguous()
    c.p = None if p is None else p.to(DEV)
    c.noise = None if noise is None else noise.to(DEV).contiguous()
    c.graph = ops.get_graph(c.ei, N)
    c.r, c.w, c.ref = [], [], []
    kind = _kind(ops, mode)
    for d in range(n):
        kw = dict(noise=None if c.noise is None else c.noise[d].contiguous(), seed=SEED, stream_id=SID0 + d)
        r = ops.sample_topq(kind, c.p, None, C, q, c.ei, cover=c.graph, want_p=False, **kw)
        plain = ops.sample_topq(kind, c.p, None, C, q, c.ei, want_keys=True, want_p=False, **kw)
        c.r.append(r)
        c.w.append(ops.st_weights(c.p, None, C, r.stats, r.eid) if mode == "learned" and q > 0 else None)
        keys = plain.keys if 0 < q < E else torch.zeros(E)            # degenerate draws compute no keys; M does not depend on them
        c.ref.append(CR.cover_ref(keys, ei, N, q))
    torch.cuda.synchronize()
    return c


@functools.lru_cache(maxsize=None)
def _config(E, q, N, kind, mode, explicit):
    import sgs_gnn_amd as S
    M = _target_M(E, q, N, kind)
    n = 3 if E == LARGE[0] else DMAX
    ei = _graph(E, N, M, seed=E + q)
    noise = torch.empty(n, E).exponential_(1, generator=torch.Generator().manual_seed(E + 7)) if explicit else None
    c = _singles(S.ops, ei, N, q, mode, _scores(mode, E, seed=E), noise, n)
    for ref in c.ref:                                                 # M from the reference, not from the recipe
        assert ref["M"] == M and {"M<q": M < q, "M=q": M == q, "M>q": M > q}[kind]
        if M <= q:
            assert CR.uncovered_nodes(ref["mask"], ei, N) == 0
    return c


# ------------------------------------------------------------------ the two ways to call
class _Out:
    pass


def _via_abi(S, c, D, want_info=True):
    """D covering draws through the C entry point itself; outputs prefilled so that an unwritten row shows."""
    L = S._lib.lib()
    ptr = lambda t: None if t is None else t.data_ptr()
    E, q, N = c.E, c.q, c.N
    o = _Out()
    mask = torch.full((D, E), 7, dtype=torch.uint8, device=DEV)
    o.eid = torch.full((D, q), -1, dtype=torch.int64, device=DEV)
    o.edge_index = torch.full((D, 2, q), -1, dtype=torch.int64, device=DEV)
    o.stats = torch.full((D, 4), -3.0, dtype=torch.float32, device=DEV)
    o.w = torch.full((D, q), -3.0, dtype=torch.float32, device=DEV) if c.mode == "learned" else None
    o.cover_info = torch.full((D, 2), -7, dtype=torch.int32, device=DEV) if want_info else None
    nws = L.sgs_sample_topq_multi_cover_workspace_bytes(E, N, D)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    noise = None if c.noise is None else c.noise[:D].contiguous()
    g = c.graph
    rc = L.sgs_sample_topq_multi_cover(_kind(S.ops, c.mode), ptr(c.p), None, C, ptr(noise), SEED, SID0, D, E, q, ptr(c.ei), N, ptr(g.in_ptr),
                                       ptr(g.in_src), ptr(g.in_eid), ptr(mask), ptr(o.eid), ptr(o.edge_index), ptr(o.stats), ptr(o.w),
                                       ptr(o.cover_info), ptr(ws), nws, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.sgs_last_error()
    torch.cuda.synchronize()
    assert int(mask.max()) <= 1
    o.mask = mask.bool()
    return o


def _via_ops(S, c, D):
    noise = None if c.noise is None else c.noise[:D].contiguous()
    return S.ops.sample_topq_multi(_kind(S.ops, c.mode), c.p, None, C, c.q, c.ei, D, noise=noise, seed=SEED, stream_id0=SID0,
                                   want_w=c.mode == "learned", cover=c.graph)


def _bits(t):
    return t.view(torch.int32)


def _check_rows(c, m, D):
    E, q = c.E, c.q
    assert tuple(m.mask.shape) == (D, E) and tuple(m.eid.shape) == (D, q) and tuple(m.cover_info.shape) == (D, 2)
    for d in range(D):
        r, ref = c.r[d], c.ref[d]
        # the single covering call
        assert torch.equal(m.mask[d], r.mask), d
        assert torch.equal(m.eid[d], r.eid), d
        assert torch.equal(m.edge_index[d], r.edge_index), d
        assert torch.equal(_bits(m.stats[d]), _bits(r.stats)), d
        assert torch.equal(m.cover_info[d], r.cover_info), d
        if c.w[d] is not None:
            assert torch.equal(_bits(m.w[d]), _bits(c.w[d])), d
        # the integer reference over the plain call's keys
        assert np.array_equal(m.mask[d].cpu().numpy(), ref["mask"]), d
        eid = torch.from_numpy(ref["eid"])
        assert torch.equal(m.eid[d].cpu(), eid), d
        assert torch.equal(m.edge_index[d].cpu(), c.ei_cpu[:, eid]), d
        assert m.cover_info[d].tolist() == [ref["M"], min(ref["M"], q)] == [ref["M"], ref["n_forced_selected"]], d
        if 0 < q < E:
            st = m.stats[d].cpu()
            assert int(st[2:3].view(torch.int32)) == ref["threshold_bits"] and int(st[3]) == ref["ties"], d


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("explicit", [False, True], ids=["clock", "noise"])
@pytest.mark.parametrize("mode", ["learned", "prior", "uniform"])
@pytest.mark.parametrize("E,q,N,kind", CASES)
def test_rows_equal_the_single_calls_and_the_reference(S, E, q, N, kind, mode, explicit):
    c = _config(E, q, N, kind, mode, explicit)
    for D in ((3,) if E == LARGE[0] else DS):
        _check_rows(c, _via_abi(S, c, D), D)
        _check_rows(c, _via_ops(S, c, D), D)
    if c.n > 1 and 0 < q < E and E > 7:
        assert not torch.equal(c.r[0].mask, c.r[1].mask)              # different streams, different draws


def test_cover_info_may_be_null_and_two_calls_give_identical_bits(S):
    c = _config(100_003, 20_000, 20_000, "M<q", "learned", False)
    a, b, n = _via_abi(S, c, 11), _via_abi(S, c, 11), _via_abi(S, c, 11, want_info=False)
    for name in ("mask", "eid", "edge_index", "cover_info"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("stats", "w"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    for name in ("mask", "eid", "edge_index"):
        assert torch.equal(getattr(a, name), getattr(n, name)), name
    assert torch.equal(_bits(a.stats), _bits(n.stats)) and torch.equal(_bits(a.w), _bits(n.w))


@pytest.mark.parametrize("E,q,N,kind", [(4097, 2000, 4097, "M>q"), (100_003, 20_000, 20_000, "M=q"), LARGE + ("M<q",)])
def test_the_group_size_does_not_change_a_bit(S, E, q, N, kind):
    c = _config(E, q, N, kind, "learned", False)
    D = c.n
    L = S._lib.lib()
    try:
        outs = []
        for G in (1, 2, 4):
            assert L.sgs_sample_topq_multi_cover_group_set(G) == 0
            outs.append(_via_abi(S, c, D))
    finally:
        assert L.sgs_sample_topq_multi_cover_group_set(0) == 0
    for o in outs:
        _check_rows(c, o, D)


def test_a_plain_multi_call_is_unchanged_by_covering_calls_around_it(S, ops):
    c = _config(100_003, 20_000, 20_000, "M<q", "learned", False)
    plain = lambda: ops.sample_topq_multi(ops.SAMPLE_LEARNED, c.p, None, C, c.q, c.ei, 5, seed=SEED, stream_id0=SID0, want_w=True)
    before = plain()
    cov = _via_ops(S, c, 5)
    after = plain()
    assert before.cover_info is None and after.cover_info is None
    for name in ("mask", "eid", "edge_index"):
        assert torch.equal(getattr(before, name), getattr(after, name)), name
    assert torch.equal(_bits(before.stats), _bits(after.stats)) and torch.equal(_bits(before.w), _bits(after.w))
    assert not torch.equal(before.mask, cov.mask)                     # (and the covering call is another draw)
    for d in range(5):                                                # the plain call is still the plain single draw
        r = ops.sample_topq(ops.SAMPLE_LEARNED, c.p, None, C, c.q, c.ei, seed=SEED, stream_id=SID0 + d)
        assert torch.equal(after.mask[d], r.mask) and torch.equal(_bits(after.stats[d]), _bits(r.stats))


# ------------------------------------------------------------------ degree classes
@pytest.mark.parametrize("n_src,lanes", [(20_000, 4), (1000, 16), (100, 64)])
def test_degree_classes(S, ops, n_src, lanes):
    """Rows of in-degree 0 .. 20 000 (the graph of tests/test_gpu_cover.py): a sub-wave group, its last partial sweep and both sides of
    the hand-over to the whole workgroup (above 128 / 512 / 2048 entries) for each lanes-per-row variant, at D = 5 (a partial group)."""
    degs = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 20_000, 128, 129, 512, 513]
    N = len(degs) + n_src
    src = torch.cat([len(degs) + torch.arange(d) % n_src for d in degs])
    dst = torch.cat([torch.full((d,), i, dtype=torch.int64) for i, d in enumerate(degs)])
    E = src.numel()
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(1))
    ei = torch.stack([src[perm], dst[perm]])
    assert S._lib.lib().sgs_sample_topq_cover_variant(N, E) == lanes
    p = _scores("learned", E, seed=3)
    for q in (5, 13, 5000):                           # M = 13: below, at and above
        c = _singles(ops, ei, N, q, "learned", p, None, 5)
        assert all(ref["M"] == 13 for ref in c.ref)
        _check_rows(c, _via_abi(S, c, 5), 5)


# ------------------------------------------------------------------ ties
def test_ties_go_to_the_lowest_ids_differently_per_draw(S, ops):
    """Constant p and explicit noise from a few repeated values, another pattern in every row: in each draw most comparisons are ties,
    both among a node's in-edges (the forced edge is the lowest id of its best level) and at the threshold."""
    for E, N, q in ((500, 40, 100), (5000, 300, 300), (5000, 3000, 1000)):
        ei = _graph(E, N, min(N, E) // 2, seed=E + N)
        p = torch.full((E,), 0.25)
        e = torch.arange(E)
        noise = torch.stack([torch.full((E,), 2.0)] + [1.0 + ((e // (d + 1) + d) % 3).float() for d in range(1, 5)])
        c = _singles(ops, ei, N, q, "learned", p, noise, 5)
        for d, ref in enumerate(c.ref):
            bits = CR.key_bits(ops.sample_topq(ops.SAMPLE_LEARNED, c.p, None, C, q, c.ei, noise=c.noise[d].contiguous(), want_keys=True).keys)
            assert len(set(bits.tolist())) == (1 if d == 0 else 3)
            assert ref["ties"] > 1
        # draw 0: every key equal, so the forced edge of a node is its lowest-id non-loop in-edge and the rest the lowest ids
        real = ei[0] != ei[1]
        first = {}
        for k in range(E):
            if bool(real[k]):
                first.setdefault(int(ei[1, k]), k)
        assert sorted(first.values()) == list(np.nonzero(c.ref[0]["forced"])[0])
        assert len({tuple(ref["eid"]) for ref in c.ref}) == 5                     # the draws differ
        for D in (2, 5):
            _check_rows(c, _via_abi(S, c, D), D)
        _check_rows(c, _via_ops(S, c, 5), 5)


# ------------------------------------------------------------------ degenerate draws
@pytest.mark.parametrize("E,N,M", [(7, 5, 3), (5000, 300, 120), (100_003, 20_000, 9000)])
def test_q_zero_and_q_equals_E(S, ops, E, N, M):
    ei = _graph(E, N, M, seed=E)
    for mode in ("learned", "uniform"):
        for q in (0, E):
            c = _singles(ops, ei, N, q, mode, _scores(mode, E, seed=2), None, 3)
            assert all(ref["M"] == M for ref in c.ref)
            for m in (_via_abi(S, c, 3), _via_ops(S, c, 3)):
                _check_rows(c, m, 3)
                assert m.cover_info.tolist() == [[M, min(M, q)]] * 3
                assert int(m.mask.sum()) == 3 * q


def test_ops_refuses_a_graph_of_another_edge_list(ops):
    ei = _graph(100, 10, 5, seed=1).to(DEV)
    p = torch.rand(100, device=DEV)
    with pytest.raises(RuntimeError, match="cover"):
        ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.3, 10, ei, 3, cover=ops.Graph(ei[:, :50].contiguous(), 10))
    with pytest.raises(RuntimeError, match="cover"):
        ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.3, 10, ei, 3, cover=object())
    assert ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.3, 10, ei, 3).cover_info is None
    r = ops.sample_topq_multi(ops.SAMPLE_LEARNED, p, None, 0.3, 10, ei, 3, cover=ops.get_graph(ei, 10))
    assert tuple(r.cover_info.shape) == (3, 2)
