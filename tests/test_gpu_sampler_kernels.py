"""GPU: the top-q sampler's general (large-E) path, its phase API, the byte-wise branches of the compaction, the degenerate draws,
sgs_dyn_edges_set and the straight-through weights, through the C ABI against tests/sampler_ref.py.

Everything that is integers or bits is compared with array_equal on integers or bit views: the normaliser Z (the fixed reduction tree
replayed in numpy), the keys (learned and uniform modes), the digit histograms, the 16-byte select state, the per-shard counts, mask,
edge ids, columns, probabilities, threshold and ties, the straight-through forward.  The only tolerances:
    prior-mode keys             2e-6 relative (the device's expf against numpy's exp; tests/test_gpu_sampler.py uses the same), after which
                                the selection is checked exactly given the kernel's own key bits
    prior-mode Z, d p           loss_ref.bound(ref64, ref32): 8 x the deviation of the float32 evaluation from the float64 one + 4 ulp
    Z against the float64 sum   sampler_ref.tree_bound: depth x 2^-24 x sum |x|
and each prints `RATIO <quantity> <case> <error / bound>` before it asserts.  Every output sits between red zones; every workspace has
exactly the size its *_workspace_bytes function reports, is filled with 0xFF beforehand and is followed by guard bytes that must come back
untouched.

Sections: A the phase API with one shard (= the general path's kernels at any E), B with R shards emulated in one process (the host does
the collectives) against the reference AND bit for bit against one sgs_sample_topq call on the small path, C sgs_sample_topq across the
path boundary (1024 / 1025 / 1026 / 2050 chunks; the last is the only size at which the histogram grid strides), D the byte-wise
branches, E q == 0 / q == E and the identity of Z across the paths, F sgs_dyn_edges_set, G the straight-through weights, H every entry
that takes a workspace (single, covering, batched, batched covering, consensus) with a buffer of exactly the reported size between red
zones, against sampler_ref / cover_ref / consensus_ref, and refused with one byte less.

Largest error / bound per quantity measured on an MI355X over all cases of this file (plain and with SGS_POISON=1: the same figures; the
module prints them as WORST lines): Z against the float64 sum 0.05 of the tree bound, prior-mode Z 0.11, prior-mode keys 0.06 of the
2e-6, d p dense term 0.28 (the cancelling sum; 0.06 otherwise), d p on the selected entries 0.09.  Every exact comparison held: the fixed-tree
replay gives the device's Z bit for bit on the small path, the general path and the phase API at every size here, and no check exposed
a defect in csrc/sampler.hip or sharded.py.

That the checks bite was tried on three deliberately wrong builds of csrc/sampler.hip: `be <= k_rem` for `be < k_rem` in compact_body
fails sections A (the case with exact zeros), B (both tie layouts) and C (both tie layouts, two random cases); hist_next_body without
its `chunk += gridDim.x` stride fails the 2050-chunk size only; the four wave sums of block_sum added in reverse fail the Z bit checks
of A, B, C and D."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as LR  # noqa: E402
import sampler_ref as R  # noqa: E402
from zoned import DEV, Zoned  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 512
C = R.C_COEF
U32, F32 = np.uint32, np.float32
_WORST = {}


@pytest.fixture(scope="module")
def lib():
    import sgs_gnn_amd as S
    yield S._lib.lib(), S.ops._stream
    print("\n" + "\n".join(f"WORST {k} {v[0]:.3f} ({v[1]})" for k, v in sorted(_WORST.items())))


# ------------------------------------------------------------------ helpers
def _ratio(quantity, tag, err, bd):
    ratio = err / bd if bd > 0 else (0.0 if err == 0 else float("inf"))
    print(f"RATIO {quantity} {tag} {ratio:.4f} err={err:.3e} bound={bd:.3e}")
    if ratio >= _WORST.get(quantity, (-1.0, ""))[0]:
        _WORST[quantity] = (ratio, tag)
    assert err <= bd, (tag, quantity, err, bd)


def _d(arr):
    return None if arr is None else torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a).view(U32)


class Ws:
    """A workspace of exactly `nb` bytes, 0xFF-filled, followed by guard bytes."""

    def __init__(self, nb):
        self.nb = int(nb)
        self.t = torch.full((self.nb + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        assert self.t.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.t[self.nb:] == 0xFF).all()), "the workspace was overrun"


def _zeroed(n, dtype):
    z = Zoned(n, dtype, -9)
    z.t.zero_()
    return z


@functools.lru_cache(maxsize=4)
def _inputs(E, mode, seed, zeros=False):
    return R.make_inputs(E, mode, seed, zeros)          # shared among the tests that need them and never modified


def _take(z, dropped):
    """An output's payload, or None for one passed as NULL (its buffer must then be untouched)."""
    a = z.get()
    if dropped:
        assert bool((a == z.fill).all()), "a buffer that was not passed was written"
        return None
    return a


OUTPUTS = ("eid", "sei", "sp", "stats", "keys")


def _topq(lib, mode, inp, q, noise="explicit", seed=0, sid=0, mask_shift=0, ei_shift=0, drop=(), out_len=None, E=None):
    """One sgs_sample_topq call -> dict of numpy outputs (None where an output was passed as NULL).  E: the size argument when it is not
    the arrays' length (the capacity under sgs_dyn_edges_set is the arrays' length; a plain call on a prefix passes less)."""
    L, stream = lib
    p, prior, noise_h, ei = inp
    abi_mode, _, _ = R.mode_args(mode)
    n = noise_h.size
    E = n if E is None else E
    m = q if out_len is None else out_len
    d_p, d_prior = _d(p), _d(prior)
    d_noise = _d(noise_h) if noise == "explicit" else None
    eiz = Zoned(2 * n, torch.int64, -3, shift=ei_shift)
    eiz.set(ei.reshape(-1))
    mask = Zoned(n, torch.uint8, 0xAB, shift=mask_shift)
    z = dict(eid=Zoned(m, torch.int64, -9), sei=Zoned(2 * m, torch.int64, -9), sp=Zoned(m, torch.float32, -9.0),
             stats=Zoned(4, torch.float32, -9.0), keys=Zoned(n, torch.float32, -9.0))
    ws = Ws(L.sgs_sample_topq_workspace_bytes(E))
    ptr = {k: (None if k in drop else v.ptr) for k, v in z.items()}
    rc = L.sgs_sample_topq(abi_mode, _p(d_p), _p(d_prior), C, _p(d_noise), seed, sid, E, q, eiz.ptr, mask.ptr, ptr["eid"], ptr["sei"],
                           ptr["sp"], ptr["stats"], ptr["keys"], ws.ptr, ws.nb, stream())
    assert rc == 0, L.sgs_last_error()
    ws.check()
    out = {k: _take(v, k in drop) for k, v in z.items()}
    out["mask"] = mask.get()
    if out["sei"] is not None:
        out["sei"] = out["sei"].reshape(2, m)
    assert np.array_equal(eiz.get(), ei.reshape(-1))
    return out


def _phase(lib, mode, inp, q, bounds, noise="explicit", seed=0, sid=0, tag=""):
    """The phases of an edge-sharded draw up to the counts, with the shards of `bounds` emulated in one process and the collectives on the
    host.  Every intermediate the phases expose is compared with the reference on the way: per-chunk partials, digit histograms before
    each select, the state after it, the zeroed histogram, the stored keys, the counts.  -> the state sgs_sampler_shard_compact needs."""
    from sgs_gnn_amd import sharded
    L, stream = lib
    p, prior, noise_h, ei = inp
    abi_mode, _, _ = R.mode_args(mode)
    chunk = int(L.sgs_sampler_chunk())
    assert chunk == R.CHUNK and all(b % chunk == 0 for b in bounds[:-1])
    sh = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        n = hi - lo
        s = SimpleNamespace(lo=lo, n=n, nblk=(n + chunk - 1) // chunk, p_h=p[lo:hi], ei_h=np.ascontiguousarray(ei[:, lo:hi]))
        s.p, s.prior = _d(p[lo:hi]), (_d(prior[lo:hi]) if prior is not None else None)
        s.noise = _d(noise_h[lo:hi]) if noise == "explicit" else None
        s.ws = Ws(L.sgs_sampler_shard_workspace_bytes(n))
        s.scal, s.hist, s.state = _zeroed(4, torch.float32), _zeroed(R.BINS, torch.int32), _zeroed(4, torch.int32)
        s.part = Zoned(s.nblk, torch.float32, -9.0)
        s.keys_out, s.counts = Zoned(n, torch.float32, -9.0), Zoned(2, torch.int32, -9)
        sh.append(s)

    def reduce_stage(stage):
        for s in sh:
            assert L.sgs_sampler_shard_partials(stage, _p(s.p), s.n, s.scal.ptr, s.part.ptr, stream()) == 0, L.sgs_last_error()
        allp = np.concatenate([s.part.get() for s in sh])
        d_all = _d(allp)
        for s in sh:
            assert L.sgs_sampler_shard_finalize(stage, _p(d_all), allp.size, s.scal.ptr, stream()) == 0, L.sgs_last_error()
        return allp

    if abi_mode == R.LEARNED:
        assert np.array_equal(_bits(reduce_stage(0)), _bits(R.tree_sum(p)[1])), tag
    else:
        assert np.array_equal(_bits(reduce_stage(1)), _bits(R.tree_max(p)[1])), tag
        reduce_stage(2)
    scal = sh[0].scal.get().copy()
    assert all(np.array_equal(_bits(s.scal.get()), _bits(scal)) for s in sh), tag
    for s in sh:
        rc = L.sgs_sampler_shard_keys(abi_mode, _p(s.p), _p(s.prior), C, _p(s.noise), seed, sid, s.lo, s.n, s.scal.ptr, s.ws.ptr, s.keys_out.ptr,
                                      s.hist.ptr, stream())
        assert rc == 0, L.sgs_last_error()
    keys = np.concatenate([s.keys_out.get() for s in sh])
    kbits = _bits(keys)
    for s in sh:                                                                         # the keys buffer: the first region of the workspace
        assert np.array_equal(s.ws.t[:4 * s.n].cpu().numpy().view(U32), kbits[s.lo:s.lo + s.n]), tag
    sel = R.select(kbits, q)
    for ps in range(3):
        if ps > 0:
            for s in sh:
                assert L.sgs_sampler_shard_hist(s.ws.ptr, s.n, ps, s.state.ptr, s.hist.ptr, stream()) == 0, L.sgs_last_error()
        tot = sum(s.hist.get().astype(np.int64) for s in sh)                             # the all-reduce
        assert np.array_equal(tot, sel["hists"][ps]), (tag, "histogram", ps)
        for s in sh:
            s.hist.set(tot.astype(np.int32))
            assert L.sgs_sampler_select(s.hist.ptr, ps, q, s.state.ptr, stream()) == 0, L.sgs_last_error()
        for s in sh:
            assert np.array_equal(s.state.get().view(U32), sel["states"][ps]), (tag, "state", ps, s.state.get(), sel["states"][ps])
            assert not s.hist.get().any(), (tag, "sgs_sampler_select leaves the histogram zeroed", ps)
    for s in sh:
        assert L.sgs_sampler_shard_count(s.ws.ptr, s.n, s.state.ptr, s.counts.ptr, s.ws.ptr, s.ws.nb, stream()) == 0, L.sgs_last_error()
    allc = [tuple(int(v) for v in s.counts.get()) for s in sh]
    assert allc == R.shard_counts(kbits, sel["T"], bounds), tag
    k_rem = int(sel["states"][2][1])
    ties = sharded.tie_quotas(k_rem, allc)
    assert ties == R.tie_quotas(k_rem, allc) and sum(ties) == k_rem
    stats = np.array([scal[0], scal[1], np.array([sel["T"]], dtype=U32).view(F32)[0], F32(k_rem)], dtype=F32)
    return SimpleNamespace(sh=sh, keys=keys, counts=allc, ties=ties, stats=stats, sel=sel)


def _phase_compact(lib, ph, mask_shift=0, ei_shift=0, drop=()):
    """sgs_sampler_shard_compact on every shard of a _phase, the outputs concatenated in rank order (the all-gather)."""
    L, stream = lib
    outs = []
    for s, (g, _), t in zip(ph.sh, ph.counts, ph.ties):
        ql = g + t
        eiz = Zoned(2 * s.n, torch.int64, -3, shift=ei_shift)
        eiz.set(s.ei_h.reshape(-1))
        mask = Zoned(s.n, torch.uint8, 0xAB, shift=mask_shift)
        z = dict(eid=Zoned(ql, torch.int64, -9), sei=Zoned(2 * ql, torch.int64, -9), sp=Zoned(ql, torch.float32, -9.0))
        ptr = {k: (None if k in drop else v.ptr) for k, v in z.items()}
        rc = L.sgs_sampler_shard_compact(s.ws.ptr, s.n, s.state.ptr, t, ql, s.lo, _p(s.p), eiz.ptr, mask.ptr, ptr["eid"], ptr["sei"], ptr["sp"],
                                         s.ws.ptr, s.ws.nb, stream())
        assert rc == 0, L.sgs_last_error()
        s.ws.check()
        o = {k: _take(v, k in drop) for k, v in z.items()}
        o["mask"] = mask.get()
        if o["sei"] is not None:
            o["sei"] = o["sei"].reshape(2, ql)
        outs.append(o)
    cat = lambda k, ax=0: None if k in drop else np.concatenate([o[k] for o in outs], axis=ax)       # noqa: E731
    return dict(mask=cat("mask"), eid=cat("eid"), sei=cat("sei", 1), sp=cat("sp"), stats=ph.stats, keys=ph.keys)


_REFS = {}


def _learned_ref(p, prior, noise, q, ref_key):
    """(Z, float64 sum, tree bound, key bits, selection) of a learned / uniform draw; computed once per `ref_key` where one is given."""
    if ref_key is not None and ref_key in _REFS:
        return _REFS[ref_key]
    x = p if p is not None else np.ones(noise.size, dtype=F32)
    Zref, _ = R.tree_sum(x)
    kref = R.keys(R.LEARNED, p, prior, C, noise, Zref, n=noise.size)
    ref = (Zref, float(x.astype(np.float64).sum()), R.tree_bound(x), kref, R.select(kref, q))
    if ref_key is not None:
        _REFS.clear()                                                                    # one at a time: they are large
        _REFS[ref_key] = ref
    return ref


def _check_draw(tag, mode, inp, q, got, noise=None, ref_key=None):
    """The common checks of a draw: Z, max, keys, selection, compacted outputs, threshold and ties against the reference.  Outputs that
    are None (passed as NULL) are skipped; without stats the keys are replayed with the reference's own Z (learned modes only).
    ref_key: names the (inputs, q) of a learned-mode reference that several calls share."""
    p, prior, noise_h, ei = inp
    noise = noise_h if noise is None else noise
    abi_mode, _, _ = R.mode_args(mode)
    stats = got["stats"]
    sel = None
    if abi_mode == R.LEARNED:
        Zref, sum64, bd, kref, sel = _learned_ref(p, prior, noise, q, ref_key)
        if stats is not None:
            assert _bits(stats[:1])[0] == _bits(np.array([Zref]))[0], (tag, "Z", float(stats[0]), float(Zref))
            _ratio("Z_vs_fp64", tag, abs(float(stats[0]) - sum64), bd)
        if got["keys"] is not None:
            assert np.array_equal(_bits(got["keys"]), kref), (tag, "keys")
    else:
        assert stats is not None and got["keys"] is not None
        Z, mx = stats[0], stats[1]
        assert _bits(stats[1:2])[0] == _bits(np.array([p.max()], dtype=F32))[0], (tag, "max")
        ref64 = float(np.exp(p.astype(np.float64) - float(mx)).sum())
        ref32 = float(R.tree_sum(R.softmax_terms(p, mx))[0])
        _ratio("Z_prior", tag, abs(float(Z) - ref64), LR.bound(ref64, ref32))
        kref = R.keys(R.PRIOR, p, None, 0.0, noise, Z, mx).view(F32).astype(np.float64)
        err = np.abs(got["keys"].astype(np.float64) - kref)
        bd = 2e-6 * np.abs(kref)
        worst = int(np.argmax(err - bd))
        _ratio("keys_prior", tag, float(err[worst]), float(bd[worst]))
        assert bool((err <= bd).all()), (tag, "prior-mode keys")
        sel = R.select(_bits(got["keys"]), q)                                            # the selection: exact, given the kernel's own keys
    assert np.array_equal(got["mask"], sel["mask"]), (tag, "mask")
    if got["eid"] is not None:
        assert np.array_equal(got["eid"], sel["eid"]), (tag, "eid")
    if got["sei"] is not None:
        assert np.array_equal(got["sei"], ei[:, sel["eid"]]), (tag, "edge_index")
    if got["sp"] is not None:
        want = p[sel["eid"]] if p is not None else np.ones(q, dtype=F32)
        assert np.array_equal(_bits(got["sp"]), _bits(want)), (tag, "sampled_p")
    if stats is not None:
        assert _bits(stats[2:3])[0] == sel["T"], (tag, "threshold")
        assert float(stats[3]) == float(sel["ties"]), (tag, "ties")
    return sel


def _same_draw(a, b, tag, keys=True):
    for k in ("mask", "eid", "sei", "sp", "stats") + (("keys",) if keys else ()):
        if a[k] is None or b[k] is None:
            continue
        x, y = (_bits(a[k]), _bits(b[k])) if a[k].dtype == F32 else (a[k], b[k])
        assert np.array_equal(x, y), (tag, k)


def _exp_noise(lib, seed, sid, E):
    L, stream = lib
    z = Zoned(E, torch.float32, -9.0)
    assert L.sgs_exp_noise(seed, sid, E, z.ptr, stream()) == 0, L.sgs_last_error()
    return z.get().copy()


# ------------------------------------------------------------------ A. the phase API with one shard: the general path at small E
@pytest.mark.parametrize("E", R.PHASE_ONE_SHARD_E)
def test_phase_api_one_shard(lib, E):
    cases = [(m, False) for m in R.PHASE_MODES] + ([("learned", True), ("learned_prior", True)] if E == 6151 else [])
    ran = 0
    for mode, zeros in cases:
        inp = _inputs(E, mode, 3 * E + len(mode), zeros)
        if zeros:
            assert (inp[0] == 0).sum() > 100
        for q in R.phase_qs(E):
            tag = f"A_E{E}_q{q}_{mode}{'_zeros' if zeros else ''}"
            ph = _phase(lib, mode, inp, q, (0, E), tag=tag)
            _check_draw(tag, mode, inp, q, _phase_compact(lib, ph))
            ran += 1
    if E == 1:                                                                           # 0 < q < E has no member: the phases still reduce
        L, stream = lib
        inp = _inputs(E, "learned", 5)
        part, scal, d_p = Zoned(1, torch.float32, -9.0), _zeroed(4, torch.float32), _d(inp[0])
        assert L.sgs_sampler_shard_partials(0, _p(d_p), 1, scal.ptr, part.ptr, stream()) == 0
        assert L.sgs_sampler_shard_finalize(0, part.ptr, 1, scal.ptr, stream()) == 0
        assert _bits(scal.get())[0] == _bits(inp[0])[0] and _bits(part.get())[0] == _bits(inp[0])[0]
    else:
        assert ran >= 3


def test_phase_api_keys_refuses_uniform_weights(lib):
    L, stream = lib
    E = 7
    inp = _inputs(E, "learned", 1)
    ws, scal, hist = Ws(L.sgs_sampler_shard_workspace_bytes(E)), _zeroed(4, torch.float32), _zeroed(R.BINS, torch.int32)
    ko = Zoned(E, torch.float32, -9.0)
    rc = L.sgs_sampler_shard_keys(R.LEARNED, None, None, C, _p(_d(inp[2])), 0, 0, 0, E, scal.ptr, ws.ptr, ko.ptr, hist.ptr, stream())
    assert rc == -1 and b"sgs_sampler_shard_keys: null pointer" in L.sgs_last_error()
    ws.check()
    assert bool((ko.get() == -9.0).all()) and not hist.get().any() and bool((ws.t == 0xFF).all())


# ------------------------------------------------------------------ B. R shards emulated in one process
@pytest.mark.parametrize("layout", list(R.SHARD_LAYOUTS))
@pytest.mark.parametrize("mode", R.PHASE_MODES)
def test_phase_api_shards_against_reference_and_small_path(lib, layout, mode):
    E, bounds = R.SHARD_E, R.SHARD_LAYOUTS[layout]
    q = E // 5
    inp = _inputs(E, mode, 41 + len(mode))
    seed, sid = 0x1234567 + len(layout), 9
    dev_noise = _exp_noise(lib, seed, sid, E)
    for noise in ("explicit", "in-register"):
        tag = f"B_{layout}_{mode}_{noise}"
        ph = _phase(lib, mode, inp, q, bounds, noise=noise, seed=seed, sid=sid, tag=tag)
        got = _phase_compact(lib, ph)
        # (in-register: the keys of shard r equal the reference's with the slice of sgs_exp_noise at the shard's GLOBAL offset)
        _check_draw(tag, mode, inp, q, got, noise=None if noise == "explicit" else dev_noise)
        one = _topq(lib, mode, inp, q, noise=noise, seed=seed, sid=sid)                 # the fused small-E path on the whole array
        _same_draw(got, one, tag)                                                        # Z, max, keys, selection, threshold: bit for bit


def _tie_inputs(E, noise):
    e = np.arange(E, dtype=np.int64)
    return np.full(E, 0.5, dtype=F32), None, noise.astype(F32), np.stack([e ^ 0x5555, 3 * e + (1 << 35)])


def test_phase_api_tie_class_across_shards(lib):
    """The threshold's tie class starts in shard 0 and ends in shard 2; the last tie taken lies inside shard 1."""
    E, bounds = R.SHARD_E, R.SHARD_LAYOUTS["R3"]
    e = np.arange(E)
    eq = (e >= 5000) & (e < 15000) & (e % 2 == 0)
    gt = (e % 5 == 1) & ~eq
    noise = np.where(eq, 1.0, np.where(gt, 0.5, 2.0))
    in0 = int(eq[:bounds[1]].sum())
    q = int(gt.sum()) + in0 + 1500
    inp = _tie_inputs(E, noise)
    ph = _phase(lib, "learned", inp, q, bounds, tag="B_ties_across")
    assert [c[1] for c in ph.counts] == [in0, int(eq[bounds[1]:bounds[2]].sum()), int(eq[bounds[2]:].sum())] and in0 > 0
    assert ph.ties == [in0, 1500, 0] and ph.counts[1][1] > 1500 and ph.counts[2][1] > 0
    got = _phase_compact(lib, ph)
    sel = _check_draw("B_ties_across", "learned", inp, q, got)
    assert sel["ties"] == in0 + 1500 and sel["n_gt"] == int(gt.sum())
    _same_draw(got, _topq(lib, "learned", inp, q), "B_ties_across")


def test_phase_api_fewer_positive_weights_than_q(lib):
    """Fewer edges than q have a positive weight: the threshold key is +0 and the zeros are taken by lowest id across the shards."""
    E, bounds = R.SHARD_E, R.SHARD_LAYOUTS["R3"]
    g = np.random.default_rng(8)
    _, _, noise, ei = R.make_inputs(E, "learned", 77)
    p = np.zeros(E, dtype=F32)
    pos = g.choice(E, size=300, replace=False)
    p[pos] = np.maximum(g.random(300, dtype=F32), F32(2.0 ** -20))
    q = 300 + 7000
    inp = (p, None, noise, ei)
    ph = _phase(lib, "learned", inp, q, bounds, tag="B_zero_threshold")
    got = _phase_compact(lib, ph)
    sel = _check_draw("B_zero_threshold", "learned", inp, q, got)
    assert sel["T"] == 0 and sel["n_gt"] == 300 and ph.ties[0] == ph.counts[0][1] and 0 < ph.ties[1] < ph.counts[1][1] and ph.ties[2] == 0
    _same_draw(got, _topq(lib, "learned", inp, q), "B_zero_threshold")


# ------------------------------------------------------------------ C. sgs_sample_topq across the path boundary
@pytest.mark.parametrize("E", R.BOUNDARY_E)
@pytest.mark.parametrize("mode", R.MODES)
def test_sample_topq_across_the_path_boundary(lib, E, mode):
    q = E // 5
    inp = _inputs(E, mode, 7 * (E % 1000) + len(mode))
    tag = f"C_E{E}_{mode}"
    got = _topq(lib, mode, inp, q)
    _check_draw(tag, mode, inp, q, got)
    if mode == "learned":                                                                # in-register noise, once per size
        seed, sid = 99 + E, 3
        dev_noise = _exp_noise(lib, seed, sid, E)
        reg = _topq(lib, mode, inp, q, noise="in-register", seed=seed, sid=sid)
        _check_draw(tag + "_in_register", mode, inp, q, reg, noise=dev_noise)
        exp = _topq(lib, mode, (inp[0], inp[1], dev_noise, inp[3]), q)
        _same_draw(reg, exp, tag + "_in_register")


def test_sample_topq_general_path_interleaved_ties(lib):
    """Greater, equal and smaller keys interleave in every thread's eight items (e % 3); the ties taken spread over hundreds of chunks
    and end in the middle of one."""
    E = R.TIES_E
    e = np.arange(E)
    noise = np.choose(e % 3, [0.5, 1.0, 2.0])
    n_gt = int((e % 3 == 0).sum())
    q = n_gt + 400000
    inp = _tie_inputs(E, noise)
    sel = _check_draw("C_ties_interleaved", "learned", inp, q, _topq(lib, "learned", inp, q))
    assert sel["ties"] == 400000 and sel["n_gt"] == n_gt
    last_tie = int(np.flatnonzero((e % 3 == 1) & (sel["mask"] == 1))[-1])
    assert last_tie // R.CHUNK > 500 and 8 < last_tie % R.CHUNK < R.CHUNK - 8


def test_sample_topq_general_path_scattered_greater_over_equal(lib):
    E = R.TIES_E
    g = np.random.default_rng(12)
    noise = np.ones(E)
    hot = g.choice(E, size=3000, replace=False)
    noise[hot] = 0.5
    q = 3000 + 123457
    inp = _tie_inputs(E, noise)
    sel = _check_draw("C_ties_scattered", "learned", inp, q, _topq(lib, "learned", inp, q))
    assert sel["ties"] == 123457 and sel["n_gt"] == 3000


# ------------------------------------------------------------------ D. the byte-wise branches of compact_body
def _bytewise_variants():
    v = [dict(mask_shift=s) for s in (1, 3, 7)] + [dict(ei_shift=1), dict(mask_shift=3, ei_shift=1)]
    return v + [dict(drop=(k,)) for k in OUTPUTS] + [dict(drop=("eid", "sei", "sp"))]


@pytest.mark.parametrize("E", R.BYTEWISE_E)
@pytest.mark.parametrize("api", ["sample_topq", "shard_compact"])
def test_bytewise_branches_and_optional_outputs(lib, E, api):
    """mask 1, 3 and 7 bytes past an 8-byte boundary (mask_aligned == 0), edge_index 8 bytes past a 16-byte boundary and odd E
    (whole == false), an even E on aligned bases (the vector path), every optional output NULL in turn."""
    mode = "learned_prior"
    for n in (E, E - 1):                                                                 # odd, then even: the 16-byte column loads
        inp = _inputs(n, mode, 13 + n % 1000)
        q = n // 5
        tag = f"D_{api}_E{n}"
        ph = _phase(lib, mode, inp, q, (0, n), tag=tag) if api == "shard_compact" else None
        variants = [dict()] + (_bytewise_variants() if n == E else [dict(mask_shift=7), dict(ei_shift=1)])
        for kw in variants:
            if api == "sample_topq":
                got = _topq(lib, mode, inp, q, **kw)
            else:
                if set(kw.get("drop", ())) & {"stats", "keys"}:
                    continue                                                             # not outputs of sgs_sampler_shard_compact
                got = _phase_compact(lib, ph, **kw)
            name = "_".join(f"{k}-{'+'.join(v) if isinstance(v, tuple) else v}" for k, v in kw.items()) or "plain"
            _check_draw(f"{tag}_{name}", mode, inp, q, got, ref_key=(n, mode, q))


# ------------------------------------------------------------------ E. degenerate draws and the Z identity
@pytest.mark.parametrize("E", R.DEGENERATE_E)
@pytest.mark.parametrize("mode", R.MODES)
def test_degenerate_draws_and_z_identity(lib, E, mode):
    """q == E and q == 0 take the general path at any E; their Z (and max) must be, bit for bit, the fused small-E path's (q == E - 1)."""
    inp = _inputs(E, mode, 23 + E)
    p, _, _, ei = inp
    base = _topq(lib, mode, inp, E - 1)
    _check_draw(f"E_E{E}_{mode}_base", mode, inp, E - 1, base)
    full = _topq(lib, mode, inp, E)
    assert bool((full["mask"] == 1).all()) and np.array_equal(full["eid"], np.arange(E)) and np.array_equal(full["sei"], ei)
    assert np.array_equal(_bits(full["sp"]), _bits(p if p is not None else np.ones(E, dtype=F32)))
    none = _topq(lib, mode, inp, 0, out_len=E)
    assert not none["mask"].any()
    assert bool((none["eid"] == -9).all()) and bool((none["sei"] == -9).all()) and bool((none["sp"] == -9.0).all())      # untouched
    for d in (full, none):
        assert np.array_equal(_bits(d["stats"][:2]), _bits(base["stats"][:2])), (E, mode, d["stats"], base["stats"])
        assert np.array_equal(_bits(d["stats"][2:]), np.zeros(2, dtype=U32))            # no threshold, no ties
        assert bool((d["keys"] == -9.0).all())                                           # no keys are computed


# ------------------------------------------------------------------ F. sgs_dyn_edges_set on the sampler
@pytest.mark.parametrize("live", R.DYN_LIVE)
@pytest.mark.parametrize("mode", R.MODES)
def test_dyn_edges_sampler(lib, live, mode):
    """Capacity 6151.  The live count 1 admits q = 1 only (0 < q is required, q <= live): the plain call with E = 1 is then a degenerate
    draw that reports no threshold, so stats[2..3] are held against the reference there."""
    L, stream = lib
    cap = R.DYN_CAPACITY
    q = 800 if live > 1 else 1
    inp = _inputs(cap, mode, 31 + live)
    head = tuple(None if a is None else np.ascontiguousarray(a[..., :live]) for a in inp)
    word = torch.tensor([live], dtype=torch.int64, device=DEV)
    try:
        assert L.sgs_dyn_edges_set(word.data_ptr()) == 0
        got = _topq(lib, mode, inp, q)                                                   # edge_index keeps the capacity as its row stride
    finally:
        assert L.sgs_dyn_edges_set(None) == 0
    plain = _topq(lib, mode, head, q)
    assert bool((got["mask"][live:] == 0xAB).all()) and bool((got["keys"][live:] == -9.0).all())    # past the live count: untouched
    got = dict(got, mask=got["mask"][:live], keys=got["keys"][:live])
    _check_draw(f"F_live{live}_{mode}", mode, head, q, got)
    if live > 1:
        _same_draw(got, plain, (live, mode))
    else:
        _same_draw(dict(got, stats=got["stats"][:2]), dict(plain, stats=plain["stats"][:2]), (live, mode), keys=False)


def test_dyn_edges_sampler_refusals(lib):
    L, stream = lib
    word = torch.tensor([100], dtype=torch.int64, device=DEV)
    msg = b"a dynamic edge count (sgs_dyn_edges_set) needs 0 < q < capacity <= 2097152"
    try:
        assert L.sgs_dyn_edges_set(word.data_ptr()) == 0
        for E, q in ((R.SMALL_LIMIT + 1, 10), (6151, 0), (6151, 6151)):
            p = torch.rand(E, device=DEV)
            mask = Zoned(E, torch.uint8, 0xAB)
            ws = Ws(L.sgs_sample_topq_workspace_bytes(E))
            rc = L.sgs_sample_topq(R.LEARNED, p.data_ptr(), None, C, None, 0, 0, E, q, None, mask.ptr, None, None, None, None, None, ws.ptr,
                                   ws.nb, stream())
            assert rc == -1 and msg in L.sgs_last_error(), L.sgs_last_error()
            ws.check()
            assert bool((mask.get() == 0xAB).all()) and bool((ws.t == 0xFF).all())     # refused: nothing launched
    finally:
        assert L.sgs_dyn_edges_set(None) == 0


# ------------------------------------------------------------------ G. the straight-through weights
def _st_case(E, q, with_prior, seed, cancel=False):
    g = np.random.default_rng(seed)
    if cancel:
        p = (F32(0.25) + F32(0.75) * g.random(E, dtype=F32)).astype(F32)
    else:
        p = np.maximum(g.random(E, dtype=F32), F32(2.0 ** -20))
        p[:9] = [0.0, 1.0, 1.5, 0.0, 1.0, 1.5, 0.0, 1.0, 1.5]                           # ids 0..5 are selected, 6..8 are not
    prior = ((F32(0.5) + g.random(E, dtype=F32)) / F32(E)).astype(F32) if with_prior else None
    eid = np.sort(np.concatenate([np.arange(6), 9 + g.choice(E - 9, size=q - 6, replace=False)])).astype(np.int64)
    gw = g.standard_normal(q).astype(F32)
    if cancel:                                                                           # S = sum g p^2 cancels pairwise to rounding
        pe = p[eid].astype(np.float64)
        gw[1::2] = (-gw[0:q - 1:2].astype(np.float64) * pe[0:q - 1:2] ** 2 / pe[1::2] ** 2).astype(F32)[:gw[1::2].size]
    return p, prior, eid, gw, R.tree_sum(p)[0]


def _st_run(lib, p, prior, eid, gw, Z, tag, live=None):
    L, stream = lib
    E, q = p.size, eid.size
    d_p, d_prior, d_eid, d_gw = _d(p), _d(prior), _d(eid), _d(gw)
    d_stats = _d(np.array([Z, 0, 0, 0], dtype=F32))
    w = Zoned(q, torch.float32, -9.0)
    assert L.sgs_st_weights_fwd(_p(d_p), _p(d_prior), C, _p(d_stats), _p(d_eid), E, q, w.ptr, stream()) == 0, L.sgs_last_error()
    assert np.array_equal(_bits(w.get()), _bits(R.st_fwd(p, prior, C, Z, eid))), (tag, "forward")
    ws = Ws(L.sgs_st_weights_bwd_workspace_bytes(E, q))
    dp = Zoned(E, torch.float32, -9.0)
    rc = L.sgs_st_weights_bwd(_p(d_p), _p(d_prior), C, _p(d_stats), _p(d_eid), _p(d_gw), E, q, dp.ptr, ws.ptr, ws.nb, stream())
    assert rc == 0, L.sgs_last_error()
    ws.check()
    got = dp.get()
    n = E if live is None else live
    r64, r32 = (R.st_closed_form(p[:n], None if prior is None else prior[:n], C, Z, eid, gw, dt) for dt in (np.float64, np.float32))
    rest = np.ones(n, dtype=bool)
    rest[eid] = False
    dense = got[:n][rest]
    assert dense.size and bool((_bits(dense) == _bits(dense[:1])[0]).all()), (tag, "the dense term is one value")
    _ratio("st_dense", tag, abs(float(dense[0]) - float(r64["dense"])), LR.bound(float(r64["dense"]), float(r32["dense"])))
    _ratio("st_selected", tag, float(np.abs(got[eid].astype(np.float64) - r64["sel"]).max()), LR.bound(r64["sel"], r32["sel"]))
    if live is not None:
        assert not _bits(got[live:]).any(), (tag, "entries at or past the live count are exactly +0")
    return r64


@pytest.mark.parametrize("E,q", R.ST_SHAPES)
@pytest.mark.parametrize("with_prior", [False, True])
def test_st_weights_fwd_bwd(lib, E, q, with_prior):
    p, prior, eid, gw, Z = _st_case(E, q, with_prior, E + q + with_prior)
    r64 = _st_run(lib, p, prior, eid, gw, Z, f"G_E{E}_q{q}_{'prior' if with_prior else 'plain'}")
    assert float(r64["dp"][2]) == float(r64["dense"]) and float(r64["dp"][0]) != float(r64["dense"])      # p = 1.5 has no own term; p = 0 has


def test_st_weights_bwd_cancelling_sum(lib):
    """grad_w makes S = sum h p^2 cancel to rounding: the bound is the quantity's own (the fp32 error model's deviation + 4 ulp), not a
    multiple of the tiny value."""
    E, q = 3000, 700
    p, prior, eid, gw, Z = _st_case(E, q, True, 5, cancel=True)
    r64 = _st_run(lib, p, prior, eid, gw, Z, "G_cancel")
    terms = np.abs(gw.astype(np.float64) * p[eid].astype(np.float64) ** 2)
    assert abs(float(r64["S"])) < 1e-5 * float(terms.sum())


def test_st_weights_bwd_dyn_edges(lib):
    L, stream = lib
    E, q, live = 3000, 700, 2000
    p, prior, eid, gw, _ = _st_case(live, q, True, 6)
    g = np.random.default_rng(1)
    p = np.concatenate([p, g.random(E - live, dtype=F32)])
    prior = np.concatenate([prior, g.random(E - live, dtype=F32)])
    Z = R.tree_sum(p[:live])[0]
    word = torch.tensor([live], dtype=torch.int64, device=DEV)
    try:
        assert L.sgs_dyn_edges_set(word.data_ptr()) == 0
        _st_run(lib, p, prior, eid, gw, Z, "G_dyn", live=live)
    finally:
        assert L.sgs_dyn_edges_set(None) == 0


# ------------------------------------------------------------------ H. every entry that takes a workspace, at exactly the reported size
WS_ENTRIES = ("topq", "cover", "multi", "multi_cover", "consensus")
WS_CASES = ((2049, 700), (1025 * R.CHUNK + 1, 400_000), (2049, 0), (2049, 2049))     # two chunks (small path), the large path, nothing, everything
WS_D, WS_N = 3, 300


@functools.lru_cache(maxsize=2)
def _ws_inputs(E):
    """What the five entries read at one E (shared, never modified): scores, a noise row per draw, a graph over WS_N nodes (a tenth of
    its edges self-loops) with its destination CSR, consensus counts and scores; plus the key bits of every draw from the reference."""
    import consensus_ref as CoR
    p, prior, _, _ = R.make_inputs(E, "learned_prior", 41 + E)
    g = np.random.default_rng(43 + E)
    noise = np.clip(g.standard_exponential((WS_D, E), dtype=F32), F32(2.0 ** -20), F32(32.0)).astype(F32)
    dst = g.integers(0, WS_N, E)
    src = np.where(g.random(E) < 0.1, dst, g.integers(0, WS_N, E))
    ei = np.stack([src, dst]).astype(np.int64)
    order = np.argsort(dst, kind="stable")
    in_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=WS_N))]).astype(np.int32)
    count, score = CoR.make_counts_scores(E, 11, 47 + E)
    Z, _ = R.tree_sum(p)
    kbits = [R.keys(R.LEARNED, p, prior, C, noise[d], Z, n=E) for d in range(WS_D)]
    dev = SimpleNamespace(p=_d(p), prior=_d(prior), noise=_d(noise), ei=_d(ei), in_ptr=_d(in_ptr), in_src=_d(src[order].astype(np.int32)),
                          in_eid=_d(order.astype(np.int32)), count=_d(count), score=_d(score))
    return SimpleNamespace(E=E, p=p, ei=ei, count=count, score=score, Z=Z, kbits=kbits, dev=dev, CoR=CoR)


def _ws_call(lib, entry, c, q, short):
    """One call of `entry` with a workspace of (reported size - short) bytes between red zones -> (rc, outputs, D).  Every buffer is
    read back through Zoned.get, which asserts its zones."""
    L, stream = lib
    E, d = c.E, c.dev
    D = WS_D if entry.startswith("multi") else 1
    nb = {"topq": lambda: L.sgs_sample_topq_workspace_bytes(E), "cover": lambda: L.sgs_sample_topq_cover_workspace_bytes(E, WS_N),
          "multi": lambda: L.sgs_sample_topq_multi_workspace_bytes(E, D), "multi_cover": lambda: L.sgs_sample_topq_multi_cover_workspace_bytes(E, WS_N, D),
          "consensus": lambda: L.sgs_consensus_select_workspace_bytes(E)}[entry]()
    assert nb % 256 == 0
    ws = Zoned(nb, torch.uint8, 0xFF, shift=192)                                         # 64 + 192 zone bytes: the payload is 256-B aligned
    assert ws.ptr % 256 == 0
    z = dict(mask=Zoned(D * E, torch.uint8, 0xAB), eid=Zoned(D * q, torch.int64, -9), sei=Zoned(D * 2 * q, torch.int64, -9),
             sp=Zoned(q, torch.float32, -9.0), stats=Zoned(4 * D, torch.float32, -9.0), info=Zoned(2 * D, torch.int32, -7),
             cnt=Zoned(q, torch.int32, -9), keys=Zoned(E, torch.int32, -9))
    P = {k: v.ptr for k, v in z.items()}
    race = (R.LEARNED, _p(d.p), _p(d.prior), C, _p(d.noise), 0, 0)
    csr = (WS_N, _p(d.in_ptr), _p(d.in_src), _p(d.in_eid))
    tail = (ws.ptr, nb - short, stream())
    if entry == "topq":
        rc = L.sgs_sample_topq(*race, E, q, _p(d.ei), P["mask"], P["eid"], P["sei"], P["sp"], P["stats"], None, *tail)
    elif entry == "cover":
        rc = L.sgs_sample_topq_cover(*race, E, q, _p(d.ei), *csr, P["mask"], P["eid"], P["sei"], P["sp"], P["stats"], None, P["info"], *tail)
    elif entry == "multi":
        rc = L.sgs_sample_topq_multi(*race, D, E, q, _p(d.ei), P["mask"], P["eid"], P["sei"], P["stats"], None, *tail)
    elif entry == "multi_cover":
        rc = L.sgs_sample_topq_multi_cover(*race, D, E, q, _p(d.ei), *csr, P["mask"], P["eid"], P["sei"], P["stats"], None, P["info"], *tail)
    else:
        rc = L.sgs_consensus_select(_p(d.count), _p(d.score), E, q, _p(d.ei), P["mask"], P["eid"], P["sei"], P["cnt"], P["sp"], P["keys"], *tail)
    torch.cuda.synchronize()
    out = {k: v.get() for k, v in z.items()}
    out["ws"] = ws.get()
    return rc, out, D


@pytest.mark.parametrize("E,q", WS_CASES)
@pytest.mark.parametrize("entry", WS_ENTRIES)
def test_exact_size_workspace_between_guard_zones(lib, entry, E, q):
    import cover_ref as CR
    L, _ = lib
    c = _ws_inputs(E)
    fills = dict(mask=0xAB, eid=-9, sei=-9, sp=-9.0, stats=-9.0, info=-7, cnt=-9, keys=-9, ws=0xFF)
    rc, out, D = _ws_call(lib, entry, c, q, short=1)                                     # one byte short: refused, nothing written
    assert rc == -2 and b"workspace too small" in L.sgs_last_error(), (rc, L.sgs_last_error())
    for k, v in out.items():
        assert bool((v == fills[k]).all()), (entry, k, "written by a refused call")
    rc, out, D = _ws_call(lib, entry, c, q, short=0)
    assert rc == 0, L.sgs_last_error()
    mask, eid, sei = out["mask"].reshape(D, E), out["eid"].reshape(D, q), out["sei"].reshape(D, 2, q)
    stats, info = out["stats"].reshape(D, 4), out["info"].reshape(D, 2)
    if entry == "consensus":
        ref = c.CoR.select_ref(c.count, c.score, q, c.ei)
        assert np.array_equal(mask[0], ref["mask"]) and np.array_equal(eid[0], ref["eid"]) and np.array_equal(sei[0], ref["edge_index"])
        assert np.array_equal(out["cnt"], ref["count"]) and np.array_equal(_bits(out["sp"]), _bits(ref["p"]))
        assert np.array_equal(out["keys"].view(U32), ref["keys"])
        return
    covering = entry.endswith("cover")
    for d in range(D):
        tag = (entry, E, q, d)
        if covering:
            ref = CR.cover_ref(c.kbits[d].view(F32), c.ei, WS_N, q)
            want_mask, want_eid, T, ties = ref["mask"].astype(np.uint8), ref["eid"], ref["threshold_bits"], ref["ties"]
            assert info[d].tolist() == [ref["M"], min(ref["M"], q)] == [ref["M"], ref["n_forced_selected"]], tag
        else:
            sel = R.select(c.kbits[d], q) if 0 < q < E else None
            want_mask = sel["mask"] if sel else np.full(E, q == E, dtype=np.uint8)
            want_eid = sel["eid"] if sel else np.arange(q, dtype=np.int64)
            T, ties = (sel["T"], sel["ties"]) if sel else (0, 0)
            assert bool((info[d] == -7).all()), tag
        assert np.array_equal(mask[d], want_mask), tag
        assert np.array_equal(eid[d], want_eid) and np.array_equal(sei[d], c.ei[:, want_eid]), tag
        if D == 1:
            assert np.array_equal(_bits(out["sp"]), _bits(c.p[want_eid])), tag
        assert _bits(stats[d, :1])[0] == _bits(np.array([c.Z]))[0] and stats[d, 1] == 0.0, tag
        if 0 < q < E:
            assert _bits(stats[d, 2:3])[0] == T and float(stats[d, 3]) == float(ties), tag
        else:
            assert np.array_equal(_bits(stats[d, 2:]), np.zeros(2, dtype=U32)), tag     # no threshold, no ties

