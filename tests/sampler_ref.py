"""numpy restatement of the top-q sampler (csrc/sampler.hip) for the exact pins of tests/test_gpu_sampler_kernels.py, with the shape and
case tables that file and tests/test_sampler_ref_cpu.py share.  numpy only: no torch, no GPU, nothing of the product.

What is replayed bit for bit from the source (float32 op by op, one rounding per op):
    tree_sum / tree_max   reduce_partial<0|1|2> + block_sum + wave_sum + reduce_final: the fixed reduction tree of the normaliser
    keys                  sample_prob + keys_hist0_body: p / (Z + 1e-12f), the prior mix, the divide by the noise
    st_fwd                st_fwd_body: the straight-through weights
What is the CONTRACT of include/sgs_hip.h, written independently of the kernels' radix select:
    select                the q largest keys, ties to the lowest edge id, plus the digit histograms and select states that contract implies
    shard_counts, tie_quotas   the per-shard counts and the tie hand-out of the edge-sharded draw
    st_closed_form        the weights and their full backward from the comment above st_bwd_partial, in any dtype (float64: the reference,
                          float32: its error model)

Floating-point corner that is NOT part of any of this: what the device's divide does with denormal operands or results.  The case
builders keep every s and every key a normal float or an exact zero."""
import math

import numpy as np

F32 = np.float32
CHUNK = 2048                     # edges per workgroup: sgs_sampler_chunk()
THREADS = 256
ITEMS = CHUNK // THREADS         # 8
WAVE = 64
BINS = 2048
SHIFTS = (21, 10, 0)             # the three radix digits: 11 + 11 + 10 bits
DIGIT_MASKS = (0x7FF, 0x7FF, 0x3FF)
SMALL_LIMIT = 1024 * CHUNK       # the fused small-E path serves 0 < q < E <= SMALL_LIMIT; everything else is the general path
EPS = F32(1e-12)                 # the literal 1e-12f
LEARNED, PRIOR = 0, 1

# ------------------------------------------------------------------ case tables
MODES = ("learned_prior", "learned", "prior", "uniform")           # uniform: p == NULL (mode LEARNED, no prior)
PHASE_MODES = MODES[:3]                                             # sgs_sampler_shard_keys refuses p == NULL
C_COEF = 0.3
PHASE_ONE_SHARD_E = (1, 7, 2047, 2048, 2049, 4097, 6151, 257 * CHUNK + 3)     # the last: scan_blocks / reduce_final give threads two items
SHARD_E = 9 * CHUNK + 5
SHARD_LAYOUTS = {                                                   # bounds at multiples of the chunk; "empty": E_local == 0 on rank 1
    "R2": (0, 4 * CHUNK, SHARD_E),
    "R3": (0, 3 * CHUNK, 6 * CHUNK, SHARD_E),
    "R3_empty_middle": (0, 4 * CHUNK, 4 * CHUNK, SHARD_E),
}
BOUNDARY_E = (SMALL_LIMIT, SMALL_LIMIT + 1, 1025 * CHUNK + 1, 2049 * CHUNK + 1)   # 1024, 1025, 1026 and 2050 chunks
TIES_E = 1025 * CHUNK + 1
BYTEWISE_E = (6151, 1025 * CHUNK + 1)
DEGENERATE_E = (300, 6151)
DYN_CAPACITY, DYN_LIVE = 6151, (4097, 1)
ST_SHAPES = ((3000, 700), (50000, 2049), (700000, 600000))          # (E, q); 600 000 -> 293 partials: st_bwd_final's second item
TIE_QUOTA_CASES = (
    # (k_rem, per-shard (greater, equal), quotas)
    (0, ((3, 5), (1, 2)), (0, 0)),
    (4, ((3, 5), (1, 2)), (4, 0)),
    (5, ((3, 5), (1, 2)), (5, 0)),
    (6, ((3, 5), (1, 2)), (5, 1)),
    (7, ((3, 5), (1, 2)), (5, 2)),
    (3, ((9, 0), (0, 2), (4, 8)), (0, 2, 1)),                       # a shard with no equal keys
    (3, ((2, 2), (0, 0), (0, 4)), (2, 0, 1)),                       # a shard with zero edges
    (1, ((0, 0), (0, 0), (7, 1)), (0, 0, 1)),
)


def phase_qs(E):
    return sorted({q for q in (1, E // 5, E - 1) if 0 < q < E})


def mode_args(mode):
    """(C ABI mode, has p, has prior) of a MODES name."""
    return {"learned_prior": (LEARNED, True, True), "learned": (LEARNED, True, False), "prior": (PRIOR, True, False),
            "uniform": (LEARNED, False, False)}[mode]


# ------------------------------------------------------------------ inputs
def make_inputs(E, mode, seed, zeros=False):
    """(p, prior, noise, edge_index) of a draw in `mode`; p / prior are None where the mode has none.
    learned p: exact 0 (zeros=True: about a tenth of the entries) or in [2^-20, 1); prior p: N(0, 1) logits; the prior: positive, of order
    1 / E, not constant; noise in [2^-20, 32].  Hence every s and every key is a normal float or an exact zero.  The endpoint columns
    are distinct 64-bit values per row and column, so any misplaced column shows."""
    g = np.random.default_rng(seed)
    _, has_p, has_prior = mode_args(mode)
    p = prior = None
    if mode == "prior":
        p = g.standard_normal(E).astype(F32)
    elif has_p:
        p = np.maximum(g.random(E, dtype=F32), F32(2.0 ** -20))
        if zeros:
            p[g.random(E) < 0.1] = 0.0
    if has_prior:
        prior = ((F32(0.5) + g.random(E, dtype=F32)) / F32(E)).astype(F32)
    noise = np.clip(g.standard_exponential(E, dtype=F32), F32(2.0 ** -20), F32(32.0)).astype(F32)
    e = np.arange(E, dtype=np.int64)
    ei = np.stack([e ^ 0x5555, 3 * e + (1 << 35)])
    return p, prior, noise, ei


# ------------------------------------------------------------------ the fixed reduction tree
def _wave_fold(v, op):
    """wave_sum: v[l] = op(v[l], v[l + o]) for o = 32, 16, ..., 1; lane 0 holds the result.  v: [..., 64]."""
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v[..., :o], v[..., o:2 * o])
    return v[..., 0]


def _block(acc, op, ident):
    """block_sum of `acc` [n, 256]: four wave folds, then the four wave results taken in order starting from the identity."""
    w = _wave_fold(acc.reshape(acc.shape[0], THREADS // WAVE, WAVE), op)
    r = np.full(acc.shape[0], ident, dtype=F32)
    for i in range(THREADS // WAVE):
        r = op(r, w[:, i])
    return r


def _tree(x, op, ident):
    x = np.ascontiguousarray(x, dtype=F32)
    n = x.size
    nblk = (n + CHUNK - 1) // CHUNK
    xp = np.full(nblk * CHUNK, ident, dtype=F32)       # an absent element leaves the accumulator as it is; so does the identity (the
    xp[:n] = x                                         # accumulators start at +0 / -inf and never become -0)
    xp = xp.reshape(nblk, ITEMS, THREADS)              # thread t of chunk b takes elements b * 2048 + i * 256 + t, i = 0..7 in order
    acc = np.full((nblk, THREADS), ident, dtype=F32)
    for i in range(ITEMS):
        acc = op(acc, xp[:, i, :])
    part = _block(acc, op, ident)
    return finish(part, op, ident), part


def finish(part, op=np.add, ident=0.0):
    """reduce_final over per-chunk partials (of one array or the concatenation of several shards'): thread t takes partials t, t + 256, ...
    in order, then the block tree."""
    part = np.ascontiguousarray(part, dtype=F32)
    n = part.size
    rows = max((n + THREADS - 1) // THREADS, 1)
    pp = np.full(rows * THREADS, ident, dtype=F32)
    pp[:n] = part
    pp = pp.reshape(rows, THREADS)
    acc = np.full(THREADS, ident, dtype=F32)
    for r in range(rows):
        acc = op(acc, pp[r])
    return F32(_block(acc[None, :], op, ident)[0])


def tree_sum(x):
    """(sum, per-chunk partials) of float32 `x` in the sampler's fixed order, bit for bit (no NaN handling: a + NaN is NaN)."""
    return _tree(x, np.add, 0.0)


def tree_max(x):
    """(max, per-chunk partials): the same tree with fmaxf and identity -inf.  (max is exact in any order; a NaN input would differ:
    fmaxf drops it, np.maximum keeps it.  The sampler's inputs hold none.)"""
    return _tree(x, np.maximum, -np.inf)


def finish_max(part):
    return finish(part, np.maximum, -np.inf)


def tree_depth(n):
    """Terms the fixed tree adds one after another on its longest path for n elements: per-thread items, wave fold, four wave sums,
    partials per thread, wave fold, four wave sums.  |tree_sum(x) - sum(x)| <= tree_depth * 2^-24 * sum|x| to first order."""
    nblk = (n + CHUNK - 1) // CHUNK
    return ITEMS + 6 + 4 + int(math.ceil(nblk / THREADS)) + 6 + 4


def tree_bound(x):
    return tree_depth(len(x)) * 2.0 ** -24 * float(np.abs(np.asarray(x, dtype=np.float64)).sum())


def softmax_terms(p, mx):
    """exp(p - mx) in float32 with numpy's exp (within an ulp or two of the device's expf, not bit-equal)."""
    return np.exp(np.asarray(p, dtype=F32) - F32(mx)).astype(F32)


# ------------------------------------------------------------------ keys
def mix_coefs(c):
    """(1 - c) and c as the kernels hold them: computed in double, then cast to float32."""
    return F32(1.0 - float(c)), F32(float(c))


def keys(mode, p, prior, c, noise, Z, mx=0.0, n=None):
    """uint32 bits of key_e = s_e / noise_e, every op rounded to float32 as sample_prob / keys_hist0_body do:
         learned: Zeps = fl(Z + 1e-12f); s = fl(p / Zeps); with a prior s = fl(fl((1 - c) s) + fl(c prior))
         prior:   s = fl(fl(exp(p - mx)) / Z)             (numpy's exp: not bit-exact against the device's expf)
       p None: weights of 1.f (n = the number of edges, default len(noise))."""
    noise = np.asarray(noise, dtype=F32)
    n = noise.size if n is None else n
    Z = F32(Z)
    if mode == PRIOR:
        s = softmax_terms(p, mx) / Z
    else:
        pv = np.ones(n, dtype=F32) if p is None else np.asarray(p, dtype=F32)
        s = pv / (Z + EPS)
        if prior is not None:
            omc, cc = mix_coefs(c)
            s = (omc * s) + (cc * np.asarray(prior, dtype=F32))
    assert s.dtype == F32
    return np.ascontiguousarray((s / noise).astype(F32)).view(np.uint32)


# ------------------------------------------------------------------ selection
def select(bits, q):
    """The header's contract for 0 < q <= E: the q largest keys win, ties at the threshold go to the lowest edge ids.

    ORDER IS BY THE uint32 BIT PATTERN of the key, not by its float value.  For the keys the sampler produces (>= +0, finite) the two
    agree.  Otherwise: a negative key (bit 31 set, -0 included) ranks ABOVE every positive one, more negative = larger; a NaN ranks by
    its bits (a positive NaN above +inf); -0 and +0 are different keys.

    Returns a dict: mask [E] u8, eid [q] ascending int64, T (threshold bits), ties (keys == T taken), n_gt (keys > T),
    hists (three int64 [2048] digit histograms: shift 21 of all keys, shift 10 of the keys sharing T's top digit, shift 0 of the keys
    sharing T's top two digits) and states (three uint32 [4] = (prefix, k_rem, n_gt, 0) after each of the three digit selections; n_gt
    is written by the last one only)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    E = bits.size
    assert 0 < q <= E
    T = np.partition(bits, E - q)[E - q]                              # the q-th largest
    gt = bits > T
    n_gt = int(gt.sum())
    ties = q - n_gt
    eq_ids = np.flatnonzero(bits == T)
    assert 0 < ties <= eq_ids.size
    mask = gt.astype(np.uint8)
    mask[eq_ids[:ties]] = 1
    eid = np.flatnonzero(mask).astype(np.int64)
    T = int(T)
    hists, states = [], []
    for d, (sh, dm) in enumerate(zip(SHIFTS, DIGIT_MASKS)):
        if d == 0:
            among = bits
        else:
            among = bits[(bits >> np.uint32(SHIFTS[d - 1])) == np.uint32(T >> SHIFTS[d - 1])]
        hists.append(np.bincount((among >> np.uint32(sh)) & np.uint32(dm), minlength=BINS).astype(np.int64))
        prefix = (T >> sh) << sh
        k_rem = q - int((bits >> np.uint32(sh) > np.uint32(T >> sh)).sum())      # still to take among the keys that share the prefix
        states.append(np.array([prefix, k_rem, n_gt if sh == 0 else 0, 0], dtype=np.uint32))
    return dict(mask=mask, eid=eid, T=T, ties=ties, n_gt=n_gt, hists=hists, states=states)


def shard_counts(bits, T, bounds):
    """Per shard [bounds[r], bounds[r + 1]): (#keys > T, #keys == T)."""
    bits = np.asarray(bits, dtype=np.uint32)
    return [(int((bits[lo:hi] > np.uint32(T)).sum()), int((bits[lo:hi] == np.uint32(T)).sum())) for lo, hi in zip(bounds[:-1], bounds[1:])]


def tie_quotas(k_rem, counts):
    """The k_rem ties go to the lowest global ids: the lowest ranks first, each taking min(what is left, its #equal)."""
    out, left = [], int(k_rem)
    for _, eq in counts:
        t = min(left, int(eq))
        out.append(t)
        left -= t
    return out


# ------------------------------------------------------------------ straight-through weights
def st_fwd(p, prior, c, Z, eid):
    """w_j = clamp(fl(p_e fl(fl(1 - s_e) + s_e)), 0, 1), e = eid[j], s as in keys(): st_fwd_body, bit for bit."""
    pv = np.asarray(p, dtype=F32)[eid]
    s = pv / (F32(Z) + EPS)
    if prior is not None:
        omc, cc = mix_coefs(c)
        s = (omc * s) + (cc * np.asarray(prior, dtype=F32)[eid])
    st = (F32(1.0) - s) + s
    v = pv * st
    assert v.dtype == F32
    return np.minimum(np.maximum(v, F32(0.0)), F32(1.0))


def st_closed_form(p, prior, c, Z, eid, grad_w, dtype):
    """The straight-through weights and their backward wrt p with every intermediate in `dtype` (the comment above st_bwd_partial):
         Z' = Z + 1e-12f,  s_e = p_e / Z' (mixed with the prior),  st_e = (1 - s_e) + s_e,  w_j = clamp(p_e st_e, 0, 1)
         h_j = g_j [0 <= p_e st_e <= 1],  S = sum_j h_j p_e^2,  a = (1 - c) with a prior, else 1
         dp_k = -(a / Z'^2) S  for every k  +  [k = eid[j]] h_j (st_e + a p_e / Z')
       Z is an INPUT (stats[0], a float32 value); (1 - c), c and 1e-12f are the kernels' float32 constants: their values are the
       function's.  The float32 evaluation sums S one term after the other, the order with the largest rounding error of any: it is the
       error model, and the device's tree must do no worse.
       Returns dict(w, S, dense (the scalar first term), sel (dp at eid), dp [E])."""
    dt = np.dtype(dtype).type
    pa = np.asarray(p, dtype=F32).astype(dt)
    pe = pa[eid]
    g = np.asarray(grad_w, dtype=F32).astype(dt)
    Zp = dt(F32(Z)) + dt(EPS)
    s = pe / Zp
    a = dt(1.0)
    if prior is not None:
        omc, cc = mix_coefs(c)
        a = dt(omc)
        s = a * s + dt(cc) * np.asarray(prior, dtype=F32).astype(dt)[eid]
    st = (dt(1.0) - s) + s
    v = pe * st
    w = np.minimum(np.maximum(v, dt(0.0)), dt(1.0))
    h = np.where((v >= 0) & (v <= 1), g, dt(0.0))
    terms = h * pe * pe
    if terms.size == 0:
        S = dt(0.0)
    elif dt is np.float64:
        S = dt(math.fsum(terms.tolist()))
    else:
        S = np.cumsum(terms, dtype=dt)[-1]
    dense = -(a / (Zp * Zp)) * S
    sel = dense + h * (st + a * pe / Zp)
    dp = np.full(pa.size, dense, dtype=dt)
    dp[eid] = sel
    return dict(w=w, S=S, dense=dt(dense), sel=sel.astype(dt), dp=dp)
