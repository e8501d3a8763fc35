"""CPU: tests/sampler_ref.py held against oracle/ (keys, selection, straight-through backward), against float64 (the fixed reduction
tree) and against its own invariants (select states and histograms, shard additivity, the tie hand-out).  No GPU, no product kernels:
this file keeps the reference of tests/test_gpu_sampler_kernels.py honest."""
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import sgs_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


# ------------------------------------------------------------------ against the oracle
def _learned_against_oracle(p, prior, noise, q, istest, Z):
    pr = None if istest else prior
    samples, _ = O.sampler_keys(p, prior, R.C_COEF, istest, Z=Z)
    bits = R.keys(R.LEARNED, p.numpy(), None if pr is None else pr.numpy(), R.C_COEF, noise.numpy(), float(Z))
    assert np.array_equal(bits, _bits(samples / noise))
    sel = R.select(bits, q)
    mask, _ = O.gumbel_softmax_sampling(prior, p, q, R.C_COEF, istest, noise, Z=Z)
    assert np.array_equal(sel["mask"].astype(bool), mask.numpy())
    assert np.array_equal(sel["eid"], np.flatnonzero(mask.numpy()))
    return sel


def test_keys_and_select_equal_the_oracle_on_the_golden_learned_cases():
    for c in load_golden("sampler.pt")["learned"]:
        sel = _learned_against_oracle(c["p"], c["prior"], c["noise"], c["q"], c["istest"], c["Z"])
        assert np.array_equal(sel["mask"].astype(bool), c["mask"].numpy())            # what the reference itself drew
        bits = R.keys(R.LEARNED, c["p"].numpy(), None if c["istest"] else c["prior"].numpy(), R.C_COEF, c["noise"].numpy(), float(c["Z"]))
        assert np.array_equal(bits, _bits(c["samples"] / c["noise"]))


def test_keys_and_select_against_the_oracle_on_the_golden_prior_cases():
    for c in load_golden("sampler.pt")["prior"]:
        E, q = c["E"], c["q"]
        okeys = F.softmax(c["prob"], dim=-1) / c["noise"]
        sel = R.select(_bits(okeys), q)                                                 # the selection, given the oracle's own keys
        want = np.zeros(E, dtype=bool)
        want[O.prior_draw(c["prob"], c["noise"], q).numpy()] = True
        assert np.array_equal(sel["mask"].astype(bool), want)
        prob = c["prob"].numpy()
        mx, _ = R.tree_max(prob)
        assert mx == prob.max()
        Z, _ = R.tree_sum(R.softmax_terms(prob, mx))
        mine = R.keys(R.PRIOR, prob, None, 0.0, c["noise"].numpy(), Z, mx).view(np.float32)
        assert np.allclose(mine, okeys.numpy(), rtol=2e-6, atol=0)                      # numpy's exp and torch's softmax: a few ulp


@pytest.mark.parametrize("E,q", [(1, 1), (7, 3), (2049, 1), (4097, 2000), (100003, 20000)])
@pytest.mark.parametrize("istest", [False, True])
def test_keys_and_select_equal_the_oracle_on_random_cases(E, q, istest):
    g = torch.Generator().manual_seed(E * 7 + q)
    p = torch.sigmoid(torch.randn(E, generator=g))
    prior = F.softmax(torch.rand(E, generator=g) * 3, dim=0)
    noise = torch.empty(E).exponential_(1, generator=g)
    Z = torch.tensor(R.tree_sum(p.numpy())[0])
    _learned_against_oracle(p, prior, noise, q, istest, Z)


def test_uniform_keys_are_one_over_z_over_noise():
    noise = np.array([0.5, 1.0, 4.0], dtype=np.float32)
    Z, part = R.tree_sum(np.ones(3, dtype=np.float32))
    assert Z == 3.0 and part.tolist() == [3.0]
    want = (np.float32(1.0) / (np.float32(3.0) + np.float32(1e-12))) / noise
    assert np.array_equal(R.keys(R.LEARNED, None, None, 0.0, noise, Z), want.view(np.uint32))


# ------------------------------------------------------------------ the fixed tree
@pytest.mark.parametrize("n", [1, 255, 2047, 2048, 2049, 6151, 257 * 2048 + 3, 2049 * 2048 + 1])
def test_tree_sum_within_its_bound_of_float64(n):
    g = np.random.default_rng(n)
    x = g.random(n, dtype=np.float32)
    t0 = time.perf_counter()
    s, part = R.tree_sum(x)
    dt = time.perf_counter() - t0
    assert s.dtype == np.float32 and part.dtype == np.float32 and part.size == (n + 2047) // 2048
    assert R.tree_depth(n) == 8 + 6 + 4 + -(-part.size // 256) + 6 + 4
    err, bound = abs(float(s) - float(x.astype(np.float64).sum())), R.tree_bound(x)
    assert err <= bound, (n, err, bound)
    assert dt < 1.0, dt                                                                # vectorised over the chunks
    m, mpart = R.tree_max(x)
    assert m == x.max() and np.array_equal(mpart, np.array([x[i:i + 2048].max() for i in range(0, n, 2048)], dtype=np.float32))


def test_tree_sum_is_the_written_order_on_a_case_where_order_shows():
    """One chunk, hand-replayed with Python loops from the description in the issue / the kernel source."""
    g = np.random.default_rng(5)
    x = (g.random(2048, dtype=np.float32) * np.float32(1e4)).astype(np.float32)
    acc = [np.float32(0.0)] * 256
    for t in range(256):
        for i in range(8):
            acc[t] = np.float32(acc[t] + x[i * 256 + t])
    waves = []
    for w in range(4):
        v = acc[64 * w:64 * w + 64]
        for o in (32, 16, 8, 4, 2, 1):
            v = [np.float32(v[l] + v[l + o]) if l + o < len(v) else v[l] for l in range(o)]
        waves.append(v[0])
    r = np.float32(0.0)
    for w in waves:
        r = np.float32(r + w)
    s, part = R.tree_sum(x)
    assert part[0].tobytes() == r.tobytes() and s.tobytes() == r.tobytes()
    assert np.float32(x.sum()).tobytes() != r.tobytes() or np.float32(np.cumsum(x)[-1]).tobytes() != r.tobytes()     # the order matters here


def test_tree_sum_is_additive_over_shards_cut_at_chunk_multiples():
    g = np.random.default_rng(11)
    x = g.random(R.SHARD_E, dtype=np.float32)
    whole, part = R.tree_sum(x)
    for bounds in R.SHARD_LAYOUTS.values():
        parts = [R.tree_sum(x[lo:hi])[1] for lo, hi in zip(bounds[:-1], bounds[1:])]
        cat = np.concatenate(parts)
        assert np.array_equal(cat.view(np.uint32), part.view(np.uint32))
        assert R.finish(cat).tobytes() == whole.tobytes()
        mparts = np.concatenate([R.tree_max(x[lo:hi])[1] for lo, hi in zip(bounds[:-1], bounds[1:])])
        assert R.finish_max(mparts) == x.max()
    assert R.tree_sum(x[:0])[1].size == 0 and R.tree_sum(x[:0])[0] == 0.0


# ------------------------------------------------------------------ select internals
def _tie_heavy_bits(E, seed):
    g = np.random.default_rng(seed)
    vals = np.array([0.0, 0.125, 0.3, 0.30000004, 0.9, 7.5], dtype=np.float32).view(np.uint32)
    bits = g.choice(vals, size=E).astype(np.uint32)
    rnd = g.random(E, dtype=np.float32).view(np.uint32)
    return np.where(g.random(E) < 0.5, bits, rnd).astype(np.uint32)


@pytest.mark.parametrize("E", [1, 7, 2049, 6151, 70003])
def test_select_states_and_histograms_are_consistent(E):
    bits = _tie_heavy_bits(E, E)
    order = np.argsort(~bits, kind="stable")                                            # descending by bits, lowest id first among equals
    for q in sorted({1, E // 5, E // 2, E - 1, E} & set(range(1, E + 1))):
        s = R.select(bits, q)
        assert int(s["mask"].sum()) == q and np.array_equal(s["eid"], np.sort(order[:q]))
        T = int(bits[order[q - 1]])
        assert s["T"] == T and int(s["states"][2][0]) == T                              # the final prefix: the q-th largest key's bits
        assert s["n_gt"] + s["ties"] == q and int(s["states"][2][2]) + int(s["states"][2][1]) == q
        assert s["n_gt"] == int((bits > T).sum()) and s["ties"] == int(s["states"][2][1])
        assert int(s["hists"][0].sum()) == E
        k_prev = q
        for d in range(3):
            h, (prefix, k_rem, n_gt, pad) = s["hists"][d], (int(v) for v in s["states"][d])
            digit = (T >> R.SHIFTS[d]) & R.DIGIT_MASKS[d]
            assert prefix == (T >> R.SHIFTS[d]) << R.SHIFTS[d] and pad == 0
            above = int(h[digit + 1:].sum())                                            # what the kernel's descending walk passes over
            assert above < k_prev <= above + int(h[digit]) and k_rem == k_prev - above
            if d + 1 < 3:
                assert int(s["hists"][d + 1].sum()) == int(h[digit])                    # the next histogram holds exactly this bin's keys
                assert n_gt == 0
            k_prev = k_rem


def test_select_orders_by_bit_pattern():
    f = np.array([1.0, -0.0, 0.0, -2.0, np.inf], dtype=np.float32)
    s = R.select(f.view(np.uint32), 2)
    assert s["eid"].tolist() == [1, 3] and s["T"] == 0x80000000                         # negatives rank above every positive key


def test_shard_counts():
    bits = np.array([5, 9, 5, 1, 5, 9, 0, 5], dtype=np.uint32)
    assert R.shard_counts(bits, 5, (0, 3, 3, 8)) == [(1, 2), (0, 0), (1, 2)]


# ------------------------------------------------------------------ the tie hand-out
def test_tie_quotas_hand_written_and_the_product_helper():
    from sgs_gnn_amd import sharded
    for k_rem, counts, want in R.TIE_QUOTA_CASES:
        assert R.tie_quotas(k_rem, counts) == list(want), (k_rem, counts)
        assert sharded.tie_quotas(k_rem, [list(c) for c in counts]) == list(want), (k_rem, counts)
    g = np.random.default_rng(3)
    for _ in range(200):
        counts = [(int(a), int(b)) for a, b in g.integers(0, 6, size=(int(g.integers(1, 6)), 2))]
        k = int(g.integers(0, sum(b for _, b in counts) + 1))
        got = sharded.tie_quotas(k, counts)
        assert got == R.tie_quotas(k, counts) and sum(got) == k and all(0 <= t <= b for t, (_, b) in zip(got, counts))


# ------------------------------------------------------------------ the one workspace layout (the library loads without a device)
WS_E = (0, 1, 2047, 2048, 2049, 1025 * 2048 + 1)
WS_D = (1, 2, 11)


def test_workspace_sizes_come_from_one_layout():
    import sgs_gnn_amd
    L = sgs_gnn_amd._lib.lib()
    N = 1013                                                                            # the node count does not enter a size
    sizes = {
        "topq": lambda E, D: L.sgs_sample_topq_workspace_bytes(E),
        "cover": lambda E, D: L.sgs_sample_topq_cover_workspace_bytes(E, N),
        "multi": lambda E, D: L.sgs_sample_topq_multi_workspace_bytes(E, D),
        "multi_cover": lambda E, D: L.sgs_sample_topq_multi_cover_workspace_bytes(E, N, D),
        "consensus": lambda E, D: L.sgs_consensus_select_workspace_bytes(E),
        "shard": lambda E, D: L.sgs_sampler_shard_workspace_bytes(E),
    }
    for name, f in sizes.items():
        tab = np.array([[f(E, D) for D in WS_D] for E in WS_E], dtype=np.int64)
        assert (tab % 256 == 0).all() and (tab > 0).all(), name
        assert (np.diff(tab, axis=0) >= 0).all() and (np.diff(tab, axis=1) >= 0).all(), name   # non-decreasing in E and in D
        assert f(-5, 1) == f(0, 1) and f(2049, 0) == f(2049, 1) == f(2049, -3), name            # E < 0 is 0, D < 1 is 1
    for D in WS_D:
        extra = {sizes["multi_cover"](E, D) - sizes["multi"](E, D) for E in WS_E}
        assert len(extra) == 1 and extra.pop() >= 4 * 1024 * D, D                       # per-workgroup counts: no function of E
    assert len({sizes["cover"](E, 1) - sizes["topq"](E, 1) for E in WS_E}) == 1
    for E in WS_E:
        assert sizes["multi"](E, 1) == sizes["topq"](E, 1) and sizes["multi_cover"](E, 1) == sizes["cover"](E, 1)
        assert sizes["consensus"](E, 1) >= sizes["topq"](E, 1) + 8 * E
        assert sizes["topq"](E, 1) >= 4 * E and sizes["multi"](E, 11) >= 11 * 4 * E     # the key rows


# ------------------------------------------------------------------ straight-through weights
@pytest.mark.parametrize("with_prior", [False, True])
def test_st_closed_form_against_autograd_of_the_oracle(with_prior):
    """Inputs on a 2^-10 grid and c = 0.25, so that Z and the mix coefficients are the same numbers in float32 and in float64."""
    E, q, c = 500, 120, 0.25
    g = np.random.default_rng(17 + with_prior)
    p = (g.integers(0, 1025, size=E) / 1024.0).astype(np.float32)
    p[:6] = [0.0, 1.0, 1.5, 0.0, 1.0, 1.5]                                               # the clamp's edges and beyond: h = g, g, 0
    prior = (g.integers(1, 9, size=E) / 4096.0).astype(np.float32) if with_prior else None
    eid = np.sort(np.concatenate([np.arange(3), 3 + g.choice(E - 3, size=q - 3, replace=False)])).astype(np.int64)
    gw = g.standard_normal(q).astype(np.float32)
    Z = float(p.astype(np.float64).sum())
    assert np.float32(Z) == Z
    ref = R.st_closed_form(p, prior, c, Z, eid, gw, np.float64)
    pt = torch.tensor(p.astype(np.float64), requires_grad=True)
    mask = torch.zeros(E, dtype=torch.bool)
    mask[torch.from_numpy(eid)] = True
    _, w = O.gumbel_softmax_sampling(None if prior is None else torch.tensor(prior.astype(np.float64)), pt, q, c, not with_prior,
                                     force_mask=mask)
    (w * torch.tensor(gw.astype(np.float64))).sum().backward()
    assert np.allclose(ref["w"], w.detach().numpy(), rtol=1e-12, atol=0)
    assert np.allclose(ref["dp"], pt.grad.numpy(), rtol=1e-10, atol=1e-15)
    assert float(ref["dp"][eid[2]]) == float(ref["dense"])                               # p = 1.5: outside the clamp, no own term
    # float32: the forward restatement agrees with the closed form to rounding, and is what st_fwd returns
    w32 = R.st_fwd(p, prior, c, Z, eid)
    assert w32.dtype == np.float32 and np.allclose(w32, ref["w"], rtol=3e-7, atol=0)
    r32 = R.st_closed_form(p, prior, c, Z, eid, gw, np.float32)
    assert r32["dp"].dtype == np.float32 and np.array_equal(r32["w"], w32)
