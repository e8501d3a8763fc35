"""GPU: node-covering draws (sgs_sample_topq_cover) through the C ABI, through ops and through the pipelines.

In every case three things must hold: keys_out is bitwise the plain call's; mask, sampled_eid, sampled_edge_index and sampled_p are
tests/cover_ref.py applied to the device's OWN keys (integer logic, so exact); cover_info == (M, min(M, q))."""
import argparse

import numpy as np
import pytest
import torch

import cover_ref as CR
import sampler_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    import sgs_gnn_amd
    return sgs_gnn_amd


@pytest.fixture(scope="module")
def ops(S):
    return S.ops


# ------------------------------------------------------------------ inputs
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


def _scores(E, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.sigmoid(torch.randn(E, generator=g))
    prior = torch.rand(E, generator=g)
    return p, prior / prior.sum()


def _check(ops, r, plain, p, ei, N, q):
    """The three properties, plus the reported threshold / ties and the CSR-free outputs' consistency."""
    E = ei.shape[1]
    torch.cuda.synchronize()
    if 0 < q < E:
        assert torch.equal(r.keys.view(torch.int32), plain.keys.view(torch.int32))          # bitwise the plain call's
        keys = r.keys
    else:
        keys = torch.zeros(E)                       # degenerate draws compute no keys (as the plain call); M does not depend on them
    ref = CR.cover_ref(keys, ei, N, q)
    assert np.array_equal(r.mask.cpu().numpy(), ref["mask"])
    eid = torch.from_numpy(ref["eid"])
    assert torch.equal(r.eid.cpu(), eid)
    assert torch.equal(r.edge_index.cpu(), ei[:, eid])
    if r.p is not None:
        assert torch.equal(r.p.cpu(), p[eid])
    assert r.cover_info.tolist() == [ref["M"], min(ref["M"], q)] == [ref["M"], ref["n_forced_selected"]]
    if 0 < q < E:
        st = r.stats.cpu()
        assert int(st[2:3].view(torch.int32)) == ref["threshold_bits"] and int(st[3]) == ref["ties"]
        assert torch.equal(st[:2], plain.stats.cpu()[:2])
    return ref


def _both(ops, mode, p, prior, q, ei, N, noise=None, seed=5, sid=9, c=0.3):
    d = lambda t: None if t is None else t.to(DEV)
    eid_ = ei.to(DEV).contiguous()
    kw = dict(noise=d(noise), seed=seed, stream_id=sid, want_keys=True)
    plain = ops.sample_topq(mode, d(p), d(prior), c, q, eid_, **kw)
    r = ops.sample_topq(mode, d(p), d(prior), c, q, eid_, cover=ops.get_graph(eid_, N), **kw)
    return r, plain


# ------------------------------------------------------------------ the (E, q, N) grid, through the C ABI
GRID = [(1, 1, 2), (7, 3, 5), (64, 63, 9), (2048, 400, 300), (2049, 1, 300), (4097, 2000, 4097), (100_003, 20_000, 20_000),
        (2_097_153, 400_000, 50_000)]
KINDS = ("M<q", "M=q", "M>q")


def _target_M(E, q, N, kind):
    """The M that makes the case, or None where the shape cannot have it (M <= min(N, E))."""
    top = min(N, E)
    M = {"M<q": min(q // 2, top), "M=q": q, "M>q": min(top, 2 * q + 1)}[kind]
    ok = {"M<q": M < q, "M=q": M == q, "M>q": M > q}[kind] and M <= top
    return M if ok else None


def test_the_grid_has_every_kind_of_case():
    kinds = {k for E, q, N in GRID for k in KINDS if _target_M(E, q, N, k) is not None}
    assert kinds == set(KINDS)
    assert all(any(_target_M(E, q, N, k) is not None for k in KINDS) for E, q, N in GRID)


def _abi_draw(S, mode, p, prior, c, noise, seed, sid, E, q, ei, N, g):
    """One covering draw through the C entry point itself."""
    L = S._lib.lib()
    ptr = lambda t: None if t is None else t.data_ptr()
    mask = torch.empty(E, dtype=torch.uint8, device=DEV)
    eid = torch.empty(q, dtype=torch.int64, device=DEV)
    sei = torch.empty(2, q, dtype=torch.int64, device=DEV)
    sp = torch.empty(q, dtype=torch.float32, device=DEV)
    stats = torch.empty(4, dtype=torch.float32, device=DEV)
    keys = torch.empty(E, dtype=torch.float32, device=DEV)
    info = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    nws = L.sgs_sample_topq_cover_workspace_bytes(E, N)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    rc = L.sgs_sample_topq_cover(mode, ptr(p), ptr(prior), c, ptr(noise), seed, sid, E, q, ptr(ei), N, ptr(g.in_ptr), ptr(g.in_src),
                                 ptr(g.in_eid), ptr(mask), ptr(eid), ptr(sei), ptr(sp), ptr(stats), ptr(keys), ptr(info), ptr(ws), nws,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.sgs_last_error()
    r = S.ops.SampleResult()
    r.mask, r.eid, r.edge_index, r.p, r.stats, r.keys, r.cover_info, r.E, r.q = mask.bool(), eid, sei, sp, stats, keys, info, E, q
    return r


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E,q,N", GRID)
def test_grid_through_the_c_abi(S, ops, E, q, N, kind):
    M = _target_M(E, q, N, kind)
    if M is None:
        return                                      # (which shapes cannot have which kind is pinned by the test above)
    ei = _graph(E, N, M, seed=E + q)
    p, prior = _scores(E, seed=E)
    d_ei, d_p, d_prior = ei.to(DEV).contiguous(), p.to(DEV), prior.to(DEV)
    g = ops.Graph(d_ei, N)
    r = _abi_draw(S, ops.SAMPLE_LEARNED, d_p, d_prior, 0.3, None, 11, 4, E, q, d_ei, N, g)
    plain = ops.sample_topq(ops.SAMPLE_LEARNED, d_p, d_prior, 0.3, q, d_ei, seed=11, stream_id=4, want_keys=True)
    ref = _check(ops, r, plain, p, ei, N, q)
    assert ref["M"] == M and {"M<q": M < q, "M=q": M == q, "M>q": M > q}[kind]           # from the reference, not assumed
    if M <= q:
        assert CR.uncovered_nodes(ref["mask"], ei, N) == 0
    L = S._lib.lib()
    assert (E > 1024 * 2048) == (E == GRID[-1][0])                                        # only the last shape takes the large-E path
    assert L.sgs_sample_topq_cover_variant(N, E) in (4, 16, 64)


# ------------------------------------------------------------------ a covering draw under sgs_dyn_edges_set
@pytest.mark.parametrize("live", SR.DYN_LIVE)
def test_dyn_edges_covering_draw_with_a_long_row(S, ops, live):
    """Capacity 6151 edges over 1000 nodes (4 lanes per row: a row above 128 entries goes to the whole workgroup), live 4097 and 1.  The
    call gets the capacity as E and the CSR of the live prefix in capacity-sized arrays, as a replayed step does: the pointers of the
    rows past the live nodes are the live E, the entries past it are stale.  Node 7 has 700 in-edges or more in the capacity graph, at least
    400 of them among the first 4097 edges.  Mask, edge ids, columns, M, threshold and ties against cover_ref of the live prefix, exactly, with
    the keys replayed by sampler_ref (which the call's own keys must equal bit for bit)."""
    cap, N, c = SR.DYN_CAPACITY, 1000, SR.C_COEF
    q = 800 if live > 1 else 1
    L = S._lib.lib()
    assert L.sgs_sample_topq_cover_variant(N, cap) == 4
    p, prior, noise, _ = SR.make_inputs(cap, "learned_prior", 71 + live)
    g = np.random.default_rng(73 + live)
    dst = g.integers(0, N, cap)
    hub = np.concatenate([g.permutation(4097)[:400], 4097 + g.permutation(cap - 4097)[:300]])
    dst[hub] = 7
    src = np.where(g.random(cap) < 0.1, dst, g.integers(0, N, cap))
    ei = np.stack([src, dst]).astype(np.int64)
    if live > 1:
        assert int((dst[:live] == 7).sum()) >= 400 > 32 * 4
    n_live = int(dst[:live].max()) + 1                                                # the live partition's nodes
    order = np.argsort(dst[:live], kind="stable")
    in_ptr = np.full(N + 1, live, dtype=np.int32)
    in_ptr[:n_live + 1] = np.concatenate([[0], np.cumsum(np.bincount(dst[:live], minlength=n_live))])
    in_src, in_eid = g.integers(0, N, cap).astype(np.int32), g.integers(0, cap, cap).astype(np.int32)      # stale past the live E
    in_src[:live], in_eid[:live] = src[:live][order], order
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    csr = argparse.Namespace(in_ptr=d(in_ptr), in_src=d(in_src), in_eid=d(in_eid))
    word = torch.tensor([live], dtype=torch.int64, device=DEV)
    try:
        assert L.sgs_dyn_edges_set(word.data_ptr()) == 0
        r = _abi_draw(S, ops.SAMPLE_LEARNED, d(p), d(prior), c, d(noise), 0, 0, cap, q, d(ei), N, csr)
        torch.cuda.synchronize()
    finally:
        assert L.sgs_dyn_edges_set(None) == 0
    Z, _ = SR.tree_sum(p[:live])
    kbits = SR.keys(SR.LEARNED, p[:live], prior[:live], c, noise[:live], Z, n=live)
    assert np.array_equal(r.keys.cpu().numpy()[:live].view(np.uint32), kbits)
    ref = CR.cover_ref(kbits.view(np.float32), ei[:, :live], N, q)
    assert np.array_equal(r.mask.cpu().numpy()[:live], ref["mask"])
    assert np.array_equal(r.eid.cpu().numpy(), ref["eid"]) and np.array_equal(r.edge_index.cpu().numpy(), ei[:, ref["eid"]])
    assert np.array_equal(r.p.cpu().numpy().view(np.uint32), p[ref["eid"]].view(np.uint32))
    assert r.cover_info.tolist() == [ref["M"], min(ref["M"], q)] == [ref["M"], ref["n_forced_selected"]]
    st = r.stats.cpu()
    assert int(st[2:3].view(torch.int32)) == ref["threshold_bits"] and int(st[3]) == ref["ties"]
    assert st[:1].numpy().view(np.uint32)[0] == np.array([Z], dtype=np.float32).view(np.uint32)[0]
    if live > 1:
        assert ref["forced"][dst[:live] == 7].sum() == 1                              # the long row forced its one best edge


# ------------------------------------------------------------------ degree classes
@pytest.mark.parametrize("n_src,lanes", [(20_000, 4), (1000, 16), (100, 64)])
def test_degree_classes(S, ops, n_src, lanes):
    """Rows of in-degree 0, 1, 2, 63, 64, 65, 2047, 2048, 2049 and 20 000, and 128, 129, 512, 513 beside them (the sources folded onto
    n_src nodes, which sets the mean degree and with it the lanes per row), so that every row-length path of each variant runs: a
    sub-wave group, its last partial sweep, and both sides of the hand-over to the whole workgroup (above 128 / 512 / 2048 entries)."""
    degs = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 20_000, 128, 129, 512, 513]
    N = len(degs) + n_src
    src = torch.cat([len(degs) + torch.arange(d) % n_src for d in degs])
    dst = torch.cat([torch.full((d,), i, dtype=torch.int64) for i, d in enumerate(degs)])
    E = src.numel()
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(1))
    ei = torch.stack([src[perm], dst[perm]])
    assert S._lib.lib().sgs_sample_topq_cover_variant(N, E) == lanes
    p, prior = _scores(E, seed=3)
    for q in (5, 13, 5000):                           # M = 13: below, at and above
        r, plain = _both(ops, ops.SAMPLE_LEARNED, p, prior, q, ei, N)
        ref = _check(ops, r, plain, p, ei, N, q)
        assert ref["M"] == 13


def test_star_self_loops_and_a_row_of_loops_plus_one_real_edge(ops):
    # a star, both directions: the hub's best in-edge and every leaf's only one
    n = 3000
    leaves = torch.arange(1, n + 1)
    ei = torch.cat([torch.stack([leaves, torch.zeros_like(leaves)]), torch.stack([torch.zeros_like(leaves), leaves])], dim=1)
    p, prior = _scores(2 * n, seed=8)
    for q in (700, n + 1, n + 500):
        r, plain = _both(ops, ops.SAMPLE_LEARNED, p, prior, q, ei, n + 1)
        assert _check(ops, r, plain, p, ei, n + 1, q)["M"] == n + 1
    # self-loops only: M = 0 and the draw IS the plain draw
    d = torch.randint(0, 50, (5000,), generator=torch.Generator().manual_seed(2))
    ei = torch.stack([d, d])
    p, prior = _scores(5000, seed=9)
    r, plain = _both(ops, ops.SAMPLE_LEARNED, p, prior, 1000, ei, 50)
    assert _check(ops, r, plain, p, ei, 50, 1000)["M"] == 0
    assert torch.equal(r.mask, plain.mask) and torch.equal(r.eid, plain.eid) and torch.equal(r.stats, plain.stats)
    # node 3: five self-loops with large scores and one real in-edge with a tiny one; the real edge is the forced one
    ei = torch.tensor([[3, 3, 1, 3, 3, 3, 0, 2], [3, 3, 3, 3, 3, 3, 2, 0]])
    p = torch.tensor([0.9, 0.9, 1e-6, 0.9, 0.9, 0.9, 0.5, 0.5])
    noise = torch.ones(8)
    r, plain = _both(ops, ops.SAMPLE_LEARNED, p, None, 3, ei, 4, noise=noise)
    ref = _check(ops, r, plain, p, ei, 4, 3)
    assert list(np.nonzero(ref["forced"])[0]) == [2, 6, 7] and r.eid.tolist() == [2, 6, 7]
    assert plain.eid.tolist() == [0, 1, 3]


def test_ties_go_to_the_lowest_ids_in_both_places(ops):
    """Constant p and constant noise: every key is equal, so the forced edge of a node is its lowest-id non-loop in-edge and the
    threshold tie takes the lowest ids."""
    for E, N, q in ((500, 40, 100), (5000, 300, 300), (5000, 3000, 1000)):
        ei = _graph(E, N, min(N, E) // 2, seed=E + N)
        p = torch.full((E,), 0.25)
        noise = torch.full((E,), 2.0)
        r, plain = _both(ops, ops.SAMPLE_LEARNED, p, None, q, ei, N, noise=noise)
        ref = _check(ops, r, plain, p, ei, N, q)
        assert len(set(r.keys.cpu().tolist())) == 1
        real = ei[0] != ei[1]
        first = {}
        for e in range(E):
            if bool(real[e]):
                first.setdefault(int(ei[1, e]), e)
        assert sorted(first.values()) == list(np.nonzero(ref["forced"])[0])
        M = ref["M"]
        if M <= q:
            rest = [e for e in range(E) if not ref["forced"][e]][:q - M]
            assert r.eid.tolist() == sorted(list(first.values()) + rest)
        else:
            assert r.eid.tolist() == sorted(first.values())[:q]


# ------------------------------------------------------------------ modes, noise, determinism
@pytest.mark.parametrize("mode", ["learned", "istest", "prior", "uniform"])
@pytest.mark.parametrize("E,q,N", [(4097, 2000, 900), (100_003, 20_000, 20_000)])
def test_modes_noise_and_determinism(ops, mode, E, q, N):
    ei = _graph(E, N, N // 2, seed=E)
    p, prior = _scores(E, seed=E + 1)
    kind = ops.SAMPLE_PRIOR if mode == "prior" else ops.SAMPLE_LEARNED
    pp = None if mode == "uniform" else (torch.randn(E, generator=torch.Generator().manual_seed(4)) if mode == "prior" else p)
    pr = prior if mode == "learned" else None
    r, plain = _both(ops, kind, pp, pr, q, ei, N, seed=21, sid=3)
    ref = _check(ops, r, plain, pp, ei, N, q)
    assert ref["M"] == N // 2
    # noise=None gives the selection the explicit sgs_exp_noise vector gives
    noise = ops.exp_noise(21, 3, E, DEV)
    r2, plain2 = _both(ops, kind, pp, pr, q, ei, N, noise=noise.cpu())
    _check(ops, r2, plain2, pp, ei, N, q)
    assert torch.equal(r2.mask, r.mask) and torch.equal(r2.eid, r.eid) and torch.equal(r2.keys, r.keys)
    # two calls are bitwise equal
    r3, _ = _both(ops, kind, pp, pr, q, ei, N, seed=21, sid=3)
    torch.cuda.synchronize()
    for a, b in ((r3.mask, r.mask), (r3.eid, r.eid), (r3.edge_index, r.edge_index), (r3.stats, r.stats), (r3.keys, r.keys),
                 (r3.cover_info, r.cover_info)):
        assert torch.equal(a, b)


def test_ops_refuses_a_graph_of_another_edge_list(ops):
    ei = _graph(100, 10, 5, seed=1).to(DEV)
    p = torch.rand(100, device=DEV)
    with pytest.raises(RuntimeError, match="cover"):
        ops.sample_topq(ops.SAMPLE_LEARNED, p, None, 0.3, 10, ei, cover=ops.Graph(ei[:, :50].contiguous(), 10))
    assert ops.sample_topq(ops.SAMPLE_LEARNED, p, None, 0.3, 10, ei).cover_info is None
    r = ops.sample_topq(ops.SAMPLE_LEARNED, p, None, 0.3, 10, ei, cover=ops.get_graph(ei, 10))
    r.check()


# ------------------------------------------------------------------ what is done with the result
def test_subgraph_and_active_set_of_a_covering_draw(ops):
    E, N, q = 30_000, 4000, 6000
    ei = _graph(E, N, 3000, seed=6)
    p, prior = _scores(E, seed=7)
    r, plain = _both(ops, ops.SAMPLE_LEARNED, p, prior, q, ei, N)
    ref = _check(ops, r, plain, p, ei, N, q)
    d_ei = ei.to(DEV).contiguous()
    parent = ops.get_graph(d_ei, N)
    assert parent.n_edges == E
    sub = ops.get_subgraph(d_ei, N, r)
    want = ops.Graph(d_ei[:, torch.from_numpy(ref["eid"]).to(DEV)].contiguous(), N)
    torch.cuda.synchronize()
    for name in ("in_ptr", "in_src", "in_eid", "out_ptr", "out_dst", "out_eid"):
        assert torch.equal(getattr(sub, name), getattr(want, name)), name
    a = ops.ActiveSet()
    a.set(r.eid, sub)                               # checked with a read-back: the compaction is in edge order
    assert a.ascending is True and bool((r.eid[1:] > r.eid[:-1]).all())


# ------------------------------------------------------------------ pipelines
def _args(**kw):
    a = argparse.Namespace(device=DEV, mode="learned", pipeline="hybrid", edge_mlp_type="GCN", conditional=True,
                           sparse_edge_mlp=True, t_init=0.7, t_min=0.5, degree_bias_coef=0.3, reg1=True, reg2=True,
                           regularizer1_coef=1.0, consist_reg_coef=0.5, hybrid_checkpoint=False, drop_rate=0.0, lr=1e-2)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _model(S, seed=3, hid=32):
    torch.manual_seed(seed)
    S.fix_seeds(seed)
    return S.GNNModel(24, hid, 5, dropout_prob=0.0, edge_mlp_type="GCN").to(DEV)


def _needs_cover(ei, N):
    """(M, bool [N]: nodes with a non-loop in-edge) of a partition."""
    e = ei.cpu().numpy()
    has = np.zeros(N, dtype=bool)
    has[e[1][e[0] != e[1]]] = True
    return int(has.sum()), has


@pytest.mark.parametrize("pipeline", ["hybrid", "straight_through", "two_pass"])
def test_every_draw_of_a_step_covers_and_flag_off_is_todays_draw(S, ops, pipeline):
    from sgs_gnn_amd.training import sampled_forward
    b = S.synthetic_graph(300, 1800, 24, 5, seed=17, device=DEV)                  # mean degree about 6
    E, N = b.edge_index.shape[1], b.x.shape[0]
    q = 400
    M, _ = _needs_cover(b.edge_index, N)
    assert M <= q < E

    def step(**kw):
        m = _model(S)                               # same parameters and the same noise / dropout clocks for every run
        st = sampled_forward(pipeline, _args(pipeline=pipeline, **kw), m, b, q)
        torch.cuda.synchronize()
        return st

    on = step(sgs_cover_nodes=True)
    for smp in (on.rs, on.smp):                     # the prior draw and the learned draw
        assert smp.cover_info.tolist() == [M, M]
        assert CR.uncovered_nodes(smp.mask.cpu().numpy(), b.edge_index, N) == 0
        assert int(smp.mask.sum()) == q and torch.equal(smp.edge_index, b.edge_index[:, smp.eid])
    off, absent, none = step(sgs_cover_nodes=False), step(), step(sgs_cover_nodes=None)
    for st in (off, none):
        assert st.rs.cover_info is None and st.smp.cover_info is None
        assert torch.equal(st.rs.eid, absent.rs.eid) and torch.equal(st.smp.eid, absent.smp.eid)
        assert torch.equal(st.learned_out, absent.learned_out)
    # today's draw for the same seeds, made by hand: the prior draw is the first tick of the noise clock
    S.fix_seeds(3)
    from sgs_gnn_amd.sampling import _NoiseClock
    hand = ops.sample_topq(ops.SAMPLE_PRIOR, b.prob, None, 0.0, q, b.edge_index, seed=_NoiseClock.seed, stream_id=1, want_p=False)
    assert torch.equal(hand.eid, absent.rs.eid)
    # the plain draws leave nodes without an in-edge at this degree; that is what the flag is for
    assert CR.uncovered_nodes(absent.smp.mask.cpu().numpy(), b.edge_index, N) > 0


def test_replayed_step_draws_cover_on_partitions_of_different_size(S, ops):
    """One capture per slot serves three partitions of different size; every replay's two draws equal their eager recomputation
    from the replay's own scores and noise (same seed, stream id and RNG epoch) over the partition's own CSR, and they cover."""
    from sgs_gnn_amd.sampling import _NoiseClock
    from sgs_gnn_amd.stepgraph import StepGraphs
    crit = torch.nn.CrossEntropyLoss()
    shapes = [(300, 1800), (220, 1300), (260, 1500)]
    bs = [S.synthetic_graph(n, E, 24, 5, seed=60 + i, device=DEV) for i, (n, E) in enumerate(shapes)]
    q = 400
    m = _model(S)
    a = _args(sgs_cover_nodes=True)
    sg = StepGraphs.attach(m, "hybrid", a, crit, q, False, loader=bs)
    sg.debug_keep = True
    try:
        assert sg._config_key()[-1] is True                        # the flag is part of what the captures bake in
        for rnd in range(2):
            for b in bs:
                E, N = b.edge_index.shape[1], b.x.shape[0]
                M, _ = _needs_cover(b.edge_index, N)
                assert M <= q < E
                h = sg.forward(b)
                c = h.c
                assert h.sampled and c.live is b and int(c.dims[0]) == E
                h.gate_counts()
                k = {n_: (None if t is None else t.clone()) for n_, t in c.keep.items()}
                c.g2l.replay()
                c.g2r.replay()
                torch.cuda.synchronize()
                epoch_now = int(sg.epoch_word.item())
                sg.epoch_word.fill_(epoch_now - 2)                  # the epoch the replay's draws saw (each backward graph ticked once)
                try:
                    tick0 = sg.seed_state[True][0]
                    cover = ops.get_graph(b.edge_index, N)
                    n1 = ops.exp_noise(_NoiseClock.seed, tick0 + 1, E, DEV)
                    r0 = ops.sample_topq(ops.SAMPLE_PRIOR, b.prob, None, 0.0, q, b.edge_index, noise=n1, want_keys=True, cover=cover)
                    n2 = ops.exp_noise(_NoiseClock.seed, tick0 + 2, E, DEV)
                    r1 = ops.sample_topq(ops.SAMPLE_LEARNED, k["edge_probs_full"][:E].contiguous(), b.prob, a.degree_bias_coef, q,
                                         b.edge_index, noise=n2, want_keys=True, cover=cover)
                    torch.cuda.synchronize()
                finally:
                    sg.epoch_word.fill_(epoch_now)
                sg.host_epoch += 2
                assert torch.equal(r0.edge_index, k["rsei"]) and torch.equal(r1.eid, k["eid"])
                assert torch.equal(k["sampled_edge_index"], b.edge_index[:, k["eid"]])
                for r in (r0, r1):
                    ref = CR.cover_ref(r.keys, b.edge_index, N, q)
                    assert np.array_equal(r.mask.cpu().numpy(), ref["mask"]) and r.cover_info.tolist() == [M, M]
                    assert CR.uncovered_nodes(ref["mask"], b.edge_index, N) == 0
                for p_ in m.parameters():
                    p_.grad = None
        assert sg.captures <= 2                                     # two sampled slots, three sizes: a capture served more than one
    finally:
        sg.release()


def test_ensemble_evaluate_takes_the_serial_loop_and_its_draws_cover(S, ops):
    import sys
    ev = sys.modules["sgs_gnn_amd.evaluate"]
    b = S.synthetic_graph(300, 1800, 24, 5, seed=23, device=DEV)
    E, N = b.edge_index.shape[1], b.x.shape[0]
    q = 400
    M, has = _needs_cover(b.edge_index, N)
    assert M <= q < E
    m = _model(S)
    for mode in ("learned", "random", "edge"):
        trace = {}
        a = _args(sgs_cover_nodes=True, sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True, num_samples_eval=3,
                  _sgs_trace_eval=trace)
        before = dict(ev.PATH_COUNTS)
        ev.ensemble_evaluate(a, m, [b], DEV, q=q, mode=mode)
        assert ev.PATH_COUNTS == dict(serial=before["serial"] + 1, batched=before["batched"])
        edges = trace["edges"].cpu().numpy()
        assert edges.shape == (3, 2, q)
        for d in range(3):
            got = np.zeros(N, dtype=bool)
            s_, d_ = edges[d]
            got[d_[s_ != d_]] = True
            assert not (has & ~got).any(), (mode, d)
        assert not np.array_equal(edges[0], edges[1])
        # and the same call without the flag takes the batched engine, as before
        a2 = _args(sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True, num_samples_eval=3)
        before = dict(ev.PATH_COUNTS)
        ev.ensemble_evaluate(a2, m, [b], DEV, q=q, mode=mode)
        assert ev.PATH_COUNTS == dict(serial=before["serial"], batched=before["batched"] + 1)
