// K0 / K2 / K3: exponential-race top-q edge sampler with stable compaction (gfx950).
//
// Reference: sampling.py:91-155 (`gumbel_softmax_sampling`), training_hybrid.py:46-48 (prior
// draw), :83/:86 (boolean-mask compaction).  torch.multinomial(s, q, replacement=False) is
// topk(s / Exp(1)); we compute the fp32 keys with the reference's expression order (IEEE
// div/mul/add, no contraction), find the q-th largest key EXACTLY with a 3-digit radix select
// over the key bit patterns (keys >= 0, so uint order == float order), break ties towards the
// lowest edge id, and emit mask + compacted columns in original edge order.
//
// HBM-bound: per candidate edge 8 B read (+4 B noise if supplied) + 4 B key write/3x4 B re-read
// (L2/Infinity-Cache resident at partition scale) + 1 B mask; per selected edge 16 B index
// read + 28 B written.  All counting is integer => run-to-run and rank-count invariant.
#include "sgs_common.h"

namespace sgs {
namespace {

constexpr int kThreads = 256;
constexpr int kItems = 8;                    // consecutive elements per thread
constexpr int kChunk = kThreads * kItems;    // 2048 elements per block
constexpr int kBins = 2048;                  // 11-bit digits
constexpr int kShift0 = 21, kShift1 = 10, kShift2 = 0;
constexpr uint32_t kMask1 = 0x7FFu, kMask2 = 0x3FFu;

struct SelectState {
    uint32_t prefix;   // key bits decided so far (high digits)
    uint32_t k_rem;    // how many keys still to take among those matching `prefix`
    uint32_t n_gt;     // (final) number of keys strictly greater than the threshold
    uint32_t pad;
};
struct SelPart { uint32_t prefix, k_rem; };   // fused small-E path: the state after digit 0 and after digit 1

// D draws over one candidate set, by value to every kernel of the selection chain; a kernel's draw is d = blockIdx.y.  A single
// draw is D == 1 on a one-row grid: d == 0, so every stride multiplies by zero.
struct DrawSet {
    uint32_t* keys; int64_t ks;     // key row of draw d at keys + d * ks
    uint32_t* hist; int64_t hs;     // digit histograms of draw d at hist + d * hs (3 * kBins on the small path, kBins on the large)
    SelectState* st;                // st[d]
    SelPart* sel;                   // sel[2 d], sel[2 d + 1]
    uint2* cnt; int64_t cs;         // per-chunk (gt, eq) counts of draw d at cnt + d * cs
    int D;
};
// the output rows of draw d: mask + d * E, eid / p + d * q, sei + d * 2 q, stats + 4 d (any but the mask may be null)
struct DrawOut {
    uint8_t* mask;
    int64_t *eid, *sei;
    float *p, *stats;
};
// row `off` of an optional output: null stays null.  The OFFSET is selected, not the pointer: straight-line scalar code, so a kernel's
// argument loads stay in one batch ahead of its first wait (a branch here split them into two dependent round trips).
template <typename T>
__device__ __forceinline__ T* opt_row(T* p, int64_t off) { return p + (p ? off : int64_t(0)); }
__device__ __forceinline__ DrawOut out_row(const DrawOut& o, int64_t d, int64_t E, int64_t q) {
    return DrawOut{o.mask + d * E, opt_row(o.eid, d * q), opt_row(o.sei, d * 2 * q), opt_row(o.p, d * q), opt_row(o.stats, 4 * d)};
}

// ---------------------------------------------------------------- reductions (deterministic tree)
// MODE 0: sum(p)   MODE 1: max(p)   MODE 2: sum(exp(p - max))
template <int MODE>
__global__ void __launch_bounds__(kThreads) reduce_partial(const float* __restrict__ p, int64_t E,
                                                          const float* __restrict__ scal, float* __restrict__ part) {
    __shared__ float red[kThreads / 64];
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kChunk;
    float mx = 0.f;
    if (MODE == 2) mx = scal[1];
    float acc = (MODE == 1) ? -INFINITY : 0.f;
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
        if (e < E) {
            const float v = p ? p[e] : 1.f;          // p == nullptr: uniform weights (sgs_sample_topq, random_edge_sampling)
            if (MODE == 0) acc += v;
            else if (MODE == 1) acc = fmaxf(acc, v);
            else acc += expf(v - mx);
        }
    }
    if (MODE == 1) {
        const float r = block_max(acc, red);
        if (threadIdx.x == 0) part[blockIdx.x] = r;
    } else {
        const float r = block_sum(acc, red);
        if (threadIdx.x == 0) part[blockIdx.x] = r;
    }
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) reduce_final(const float* __restrict__ part, int64_t n,
                                                        float* __restrict__ scal) {
    __shared__ float red[kThreads / 64];
    float acc = (MODE == 1) ? -INFINITY : 0.f;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) {
        const float v = part[i];
        if (MODE == 1) acc = fmaxf(acc, v);
        else acc += v;
    }
    if (MODE == 1) {
        const float r = block_max(acc, red);
        if (threadIdx.x == 0) scal[1] = r;
    } else {
        const float r = block_sum(acc, red);
        if (threadIdx.x == 0) scal[0] = r;
    }
}

// ---------------------------------------------------------------- key computation
// The reference's fp32 expression order, op by op (sampling.py:93-96):
//   samples = edge_probs / (edge_probs.sum() + eps)
//   samples = (1 - c) * samples + c * batch.prob          (python doubles -> fp32 scalars)
//   keys    = samples / Exp(1)
template <int MODE>
__device__ __forceinline__ float sample_prob(float pv, float Zeps, float mx, float priorv, bool has_prior,
                                             float one_minus_c, float c) {
    if (MODE == SGS_SAMPLE_LEARNED) {
        float s = __fdiv_rn(pv, Zeps);
        if (has_prior) s = __fadd_rn(__fmul_rn(one_minus_c, s), __fmul_rn(c, priorv));
        return s;
    } else {
        return __fdiv_rn(expf(pv - mx), Zeps);
    }
}

template <int MODE>
__device__ __forceinline__ void keys_hist0_body(const float* __restrict__ p, const float* __restrict__ prior,
                                                const float* __restrict__ noise, uint64_t seed,
                                                uint64_t stream_id, const uint64_t* __restrict__ epoch, int64_t edge_offset, int64_t E, float one_minus_c, float c,
                                                const float* __restrict__ scal, uint32_t* __restrict__ keys,
                                                float* __restrict__ keys_out, uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[kBins];
    for (int i = threadIdx.x; i < kBins; i += kThreads) lh[i] = 0;
    __syncthreads();
    seed = fold_epoch(seed, epoch);
    const float Z = scal[0];
    const float Zeps = (MODE == SGS_SAMPLE_LEARNED) ? __fadd_rn(Z, 1e-12f) : Z;
    const float mx = (MODE == SGS_SAMPLE_PRIOR) ? scal[1] : 0.f;
    const bool has_prior = prior != nullptr;
    // grid-stride over the 2048-edge chunks: at full-graph scale (56 k chunks) a workgroup per chunk would flush 56 k
    // private histograms into the 2048 global bins; a capped grid flushes a few thousand
    const int64_t nchunk = (E + kChunk - 1) / kChunk;
    for (int64_t chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {
        const int64_t base = chunk * kChunk;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
            if (e < E) {
                const float s = sample_prob<MODE>(p ? p[e] : 1.f, Zeps, mx, has_prior ? prior[e] : 0.f, has_prior, one_minus_c, c);
                const float nz = noise ? noise[e] : exp_noise_at(seed, stream_id, static_cast<uint64_t>(edge_offset + e));
                const float key = __fdiv_rn(s, nz);
                const uint32_t bits = __float_as_uint(key);
                keys[e] = bits;
                if (keys_out) keys_out[e] = key;
                atomicAdd(&lh[bits >> kShift0], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kThreads) {
        const uint32_t v = lh[i];
        if (v) atomicAdd(&hist[i], v);
    }
}
// large-E path and phase API: draw d reads noise row d (or stream stream_id0 + d)
template <int MODE>
__global__ void __launch_bounds__(kThreads) keys_hist0(const float* __restrict__ p, const float* __restrict__ prior,
                                                      const float* __restrict__ noise, uint64_t seed, uint64_t stream_id0,
                                                      const uint64_t* __restrict__ epoch, int64_t edge_offset, int64_t E, float one_minus_c,
                                                      float c, const float* __restrict__ scal, DrawSet ds, float* __restrict__ keys_out) {
    const int64_t d = blockIdx.y;
    keys_hist0_body<MODE>(p, prior, noise ? noise + d * E : nullptr, seed, stream_id0 + d, epoch, edge_offset, E, one_minus_c, c, scal,
                          ds.keys + d * ds.ks, opt_row(keys_out, d * E), ds.hist + d * ds.hs);
}

// Histogram of the next digit among keys whose higher digits equal state->prefix.
__device__ __forceinline__ void hist_next_body(const uint32_t* __restrict__ keys, int64_t E, int shift,
                                               uint32_t digit_mask, int prev_shift,
                                               const SelectState* __restrict__ st, uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[kBins];
    for (int i = threadIdx.x; i < kBins; i += kThreads) lh[i] = 0;
    __syncthreads();
    const uint32_t want = st->prefix >> prev_shift;
    const int64_t nchunk = (E + kChunk - 1) / kChunk;
    for (int64_t chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {
        const int64_t base = chunk * kChunk;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
            if (e < E) {
                const uint32_t bits = keys[e];
                if ((bits >> prev_shift) == want) atomicAdd(&lh[(bits >> shift) & digit_mask], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kThreads) {
        const uint32_t v = lh[i];
        if (v) atomicAdd(&hist[i], v);
    }
}
__global__ void __launch_bounds__(kThreads) hist_next(DrawSet ds, int64_t E, int shift, uint32_t digit_mask, int prev_shift) {
    const int64_t d = blockIdx.y;
    hist_next_body(ds.keys + d * ds.ks, E, shift, digit_mask, prev_shift, ds.st + d, ds.hist + d * ds.hs);
}

// One block: locate the digit bin holding the k_rem-th largest key of the current prefix.
__device__ __forceinline__ uint32_t load_coherent(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ void select_digit_body(uint32_t* __restrict__ hist, int shift, int first, uint32_t q, SelectState* __restrict__ st) {
    __shared__ uint32_t tsum[kThreads];
    __shared__ uint32_t found_bin, found_above;
    constexpr int per = kBins / kThreads;  // 8 bins per thread, descending order
    const uint32_t k = first ? q : st->k_rem;
    uint32_t loc[per];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < per; ++j) {
        const int bin = kBins - 1 - (threadIdx.x * per + j);
        loc[j] = load_coherent(hist + bin);
        s += loc[j];
    }
    tsum[threadIdx.x] = s;
    __syncthreads();
    // exclusive prefix over threads (descending bins): Hillis-Steele in LDS
    for (int off = 1; off < kThreads; off <<= 1) {
        uint32_t v = (threadIdx.x >= off) ? tsum[threadIdx.x - off] : 0u;
        __syncthreads();
        tsum[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t before = tsum[threadIdx.x] - s;  // keys in strictly higher bins than this thread's range
    if (before < k && before + s >= k) {
        uint32_t run = before;
#pragma unroll
        for (int j = 0; j < per; ++j) {
            if (run < k && run + loc[j] >= k) {
                found_bin = kBins - 1 - (threadIdx.x * per + j);
                found_above = run;
            }
            run += loc[j];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t pre = first ? 0u : st->prefix;
        st->prefix = pre | (found_bin << shift);
        st->k_rem = k - found_above;
        if (shift == 0) st->n_gt = q - (k - found_above);
    }
    // clear the histogram for the next pass
    for (int i = threadIdx.x; i < kBins; i += kThreads) hist[i] = 0;
    __syncthreads();
}
__global__ void __launch_bounds__(kThreads) select_digit(DrawSet ds, int shift, int first, uint32_t q) {
    select_digit_body(ds.hist + static_cast<int64_t>(blockIdx.y) * ds.hs, shift, first, q, ds.st + blockIdx.y);
}

// ---------------------------------------------------------------- counting + scan + compaction
__device__ __forceinline__ void load_keys8(const uint32_t* __restrict__ keys, int64_t e0, int64_t E, uint32_t (&k)[kItems]) {
    if (e0 + kItems <= E) {
        const uint4 a = *reinterpret_cast<const uint4*>(keys + e0);
        const uint4 b = *reinterpret_cast<const uint4*>(keys + e0 + 4);
        k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
        k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < kItems; ++j) k[j] = (e0 + j < E) ? keys[e0 + j] : 0u;
    }
}

__device__ __forceinline__ void count_blocks_body(const uint32_t* __restrict__ keys, int64_t E,
                                                  const SelectState* __restrict__ st, uint2* __restrict__ cnt) {
    __shared__ int red[2 * (kThreads / 64)];
    const uint32_t T = st->prefix;
    const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kItems;
    uint32_t k[kItems];
    load_keys8(keys, e0, E, k);
    int gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const bool in = e0 + j < E;
        gt += (in && k[j] > T);
        eq += (in && k[j] == T);
    }
    gt = wave_sum_int_all(gt);
    eq = wave_sum_int_all(eq);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[2 * wid] = gt; red[2 * wid + 1] = eq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int g = 0, q_ = 0;
        for (int w = 0; w < kThreads / 64; ++w) { g += red[2 * w]; q_ += red[2 * w + 1]; }
        cnt[blockIdx.x] = make_uint2(static_cast<uint32_t>(g), static_cast<uint32_t>(q_));
    }
}
__global__ void __launch_bounds__(kThreads) count_blocks(DrawSet ds, int64_t E) {
    const int64_t d = blockIdx.y;
    count_blocks_body(ds.keys + d * ds.ks, E, ds.st + d, ds.cnt + d * ds.cs);
}

// One block: exclusive scan of the per-block (gt, eq) counts, in place.
__device__ void scan_blocks_body(uint2* __restrict__ cnt, int64_t nblk) {
    __shared__ uint32_t sg[kThreads], se[kThreads];
    const int64_t per = (nblk + kThreads - 1) / kThreads;
    const int64_t lo = static_cast<int64_t>(threadIdx.x) * per;
    const int64_t hi = (lo + per < nblk) ? lo + per : nblk;
    uint32_t g = 0, e = 0;
    for (int64_t i = lo; i < hi; ++i) { g += cnt[i].x; e += cnt[i].y; }
    sg[threadIdx.x] = g; se[threadIdx.x] = e;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        uint32_t vg = 0, ve = 0;
        if (threadIdx.x >= off) { vg = sg[threadIdx.x - off]; ve = se[threadIdx.x - off]; }
        __syncthreads();
        sg[threadIdx.x] += vg; se[threadIdx.x] += ve;
        __syncthreads();
    }
    uint32_t rg = sg[threadIdx.x] - g, re = se[threadIdx.x] - e;
    for (int64_t i = lo; i < hi; ++i) {
        const uint2 c = cnt[i];
        cnt[i] = make_uint2(rg, re);
        rg += c.x; re += c.y;
    }
}
__global__ void __launch_bounds__(kThreads) scan_blocks(DrawSet ds, int64_t nblk) {
    scan_blocks_body(ds.cnt + static_cast<int64_t>(blockIdx.y) * ds.cs, nblk);
}

// blk_gt / blk_eq: number of keys > T / == T in all chunks before this workgroup's
__device__ __forceinline__ void compact_body(uint32_t blk_gt, uint32_t blk_eq, const uint32_t* __restrict__ keys, int64_t E, int64_t Ecap, int64_t q,
                                             int64_t ties_override, int64_t eid_offset, const SelectState* __restrict__ st,
                                             const float* __restrict__ p, const int64_t* __restrict__ edge_index,
                                             uint8_t* __restrict__ mask, int mask_aligned,
                                             int64_t* __restrict__ sampled_eid, int64_t* __restrict__ sei,
                                             float* __restrict__ sampled_p) {
    __shared__ uint32_t wg[kThreads / 64], we[kThreads / 64];
    const uint32_t T = st->prefix, k_rem = ties_override >= 0 ? static_cast<uint32_t>(ties_override) : st->k_rem;
    const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kItems;
    uint32_t k[kItems];
    load_keys8(keys, e0, E, k);
    uint32_t gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const bool in = e0 + j < E;
        gt += (in && k[j] > T);
        eq += (in && k[j] == T);
    }
    // exclusive prefix of (gt, eq) over the block's threads: wave scan + wave totals
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t ig = gt, ie = eq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t vg = __shfl_up(ig, o, 64), ve = __shfl_up(ie, o, 64);
        if (lane >= o) { ig += vg; ie += ve; }
    }
    if (lane == 63) { wg[wid] = ig; we[wid] = ie; }
    __syncthreads();
    uint32_t bg = blk_gt, be = blk_eq;
    for (int w = 0; w < wid; ++w) { bg += wg[w]; be += we[w]; }
    bg += ig - gt;   // #gt with lower id (global)
    be += ie - eq;   // #eq with lower id (global)
    uint64_t mbits = 0;
    // The endpoint columns of this thread's 8 candidates are loaded UNCONDITIONALLY as four 16-byte vectors per row of
    // edge_index when the tile is whole: at the usual 20 % keep rate a predicated 8-byte gather touches nearly every cache
    // line anyway, and at full-graph scale (E = 114.6 M) the streaming form is what HBM delivers at speed.
    const bool whole = e0 + kItems <= E && sei != nullptr && ((reinterpret_cast<uintptr_t>(edge_index) | (static_cast<uint64_t>(Ecap) * 8)) & 15) == 0;
    int64_t sv[kItems], dv[kItems];
    if (whole) {
#pragma unroll
        for (int j = 0; j < kItems; j += 2) {
            const longlong2 a = *reinterpret_cast<const longlong2*>(edge_index + e0 + j);
            const longlong2 b = *reinterpret_cast<const longlong2*>(edge_index + Ecap + e0 + j);
            sv[j] = a.x; sv[j + 1] = a.y; dv[j] = b.x; dv[j + 1] = b.y;
        }
    }
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const int64_t e = e0 + j;
        if (e < E) {
            const bool isgt = k[j] > T, iseq = k[j] == T;
            const bool sel = isgt || (iseq && be < k_rem);
            if (sel) {
                mbits |= (uint64_t(1) << (8 * j));
                const int64_t pos = static_cast<int64_t>(bg) + static_cast<int64_t>(be < k_rem ? be : k_rem);
                if (sampled_eid) sampled_eid[pos] = eid_offset + e;
                if (sei) {
                    sei[pos] = whole ? sv[j] : edge_index[e];
                    sei[q + pos] = whole ? dv[j] : edge_index[Ecap + e];
                }
                if (sampled_p) sampled_p[pos] = p ? p[e] : 1.f;
            }
            bg += isgt;
            be += iseq;
        }
    }
    if (mask_aligned && e0 + kItems <= E) {
        *reinterpret_cast<uint64_t*>(mask + e0) = mbits;
    } else {
#pragma unroll
        for (int j = 0; j < kItems; ++j)
            if (e0 + j < E) mask[e0 + j] = static_cast<uint8_t>((mbits >> (8 * j)) & 1u);
    }
}
// ties_override / eid_offset: the phase API's share of the ties and its shard's first global edge id (-1 / 0 otherwise)
__global__ void __launch_bounds__(kThreads) compact(DrawSet ds, int64_t E, int64_t q, int64_t ties_override, int64_t eid_offset,
                                                   const float* __restrict__ p, const int64_t* __restrict__ edge_index, DrawOut out) {
    const int64_t d = blockIdx.y;
    const DrawOut o = out_row(out, d, E, q);
    const uint2 c = ds.cnt[d * ds.cs + blockIdx.x];
    compact_body(c.x, c.y, ds.keys + d * ds.ks, E, E, q, ties_override, eid_offset, ds.st + d, p, edge_index, o.mask,
                 (reinterpret_cast<uintptr_t>(o.mask) & 7) == 0, o.eid, o.sei, o.p);
}

// ---------------------------------------------------------------- fused small-E path (partition scale)
// At partition scale (E <= ~2 M) a draw is launch-latency bound, so sgs_sample_topq runs the same algorithm in
// 6 (learned) / 7 (prior) launches instead of 13 / 15.  The one-workgroup steps between the passes (final reductions,
// digit selection, block scan) are RECOMPUTED BY EVERY WORKGROUP of the next pass from the complete per-chunk partials /
// histograms / counts the previous launch left in memory -- a few KB of L2 reads per workgroup, the same arithmetic in
// the same order (bit-identical Z, max, threshold), no inter-workgroup synchronisation.  (A "last workgroup done"
// variant with tickets was measured slower on MI355X: the device-scope fences write back / invalidate the per-XCD L2s.)
constexpr int kSmallBlocks = 1024;
constexpr int kHistGrid = 2048;        // workgroups of the histogram passes on the large-E path (grid-stride over chunks)     // small path when E <= 1024 chunks (2 M candidate edges)

// sgs_dyn_edges_set: the live candidate count comes from a device word; the launch was sized for the capacity.  Returns false
// for a workgroup that has no chunk of the live range (it leaves at once: it has no part in the recomputed reductions either).
__device__ __forceinline__ bool dyn_range(const int64_t* __restrict__ dynE, int64_t& E, int64_t& nblk) {
    if (dynE) {
        const int64_t live = *dynE;               // never more than the capacity the launch was sized for
        if (live < E) E = live;
        nblk = (E + kChunk - 1) / kChunk;
        return static_cast<int64_t>(blockIdx.x) < nblk;
    }
    return true;
}

template <int MODE>   // 1: max, otherwise sum (fixed tree, as reduce_final); result in every thread
__device__ __forceinline__ float final_reduce_all(const float* __restrict__ part, int64_t n, float* red) {
    float acc = (MODE == 1) ? -INFINITY : 0.f;
    // (the first kThreads threads only: a wider workgroup -- small_keys_hist0 -- reduces in exactly the order of a kThreads-wide one; the
    //  other waves contribute the identity to the fixed tree)
    if (threadIdx.x < kThreads)
        for (int64_t i = threadIdx.x; i < n; i += kThreads) {
            const float v = part[i];
            if (MODE == 1) acc = fmaxf(acc, v);
            else acc += v;
        }
    if (MODE == 1) return block_max(acc, red);
    const float r = block_sum(acc, red);
    __shared__ float bc;
    if (threadIdx.x == 0) bc = r;
    __syncthreads();
    const float out = bc;
    __syncthreads();
    return out;
}

// select_digit's search without its side effects: (bin, #keys in higher bins) of the k-th largest key; every thread
// gets the result.  `hist` is complete (previous launch).
__device__ __forceinline__ uint2 select_digit_local(const uint32_t* __restrict__ hist, uint32_t k) {
    __shared__ uint32_t tsum[kThreads];
    __shared__ uint32_t found_bin, found_above;
    constexpr int per = kBins / kThreads;
    uint32_t loc[per];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < per; ++j) {
        loc[j] = hist[kBins - 1 - (threadIdx.x * per + j)];
        s += loc[j];
    }
    tsum[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        uint32_t v = (threadIdx.x >= off) ? tsum[threadIdx.x - off] : 0u;
        __syncthreads();
        tsum[threadIdx.x] += v;
        __syncthreads();
    }
    const uint32_t before = tsum[threadIdx.x] - s;
    if (before < k && before + s >= k) {
        uint32_t run = before;
#pragma unroll
        for (int j = 0; j < per; ++j) {
            if (run < k && run + loc[j] >= k) {
                found_bin = kBins - 1 - (threadIdx.x * per + j);
                found_above = run;
            }
            run += loc[j];
        }
    }
    __syncthreads();
    const uint2 r = make_uint2(found_bin, found_above);
    __syncthreads();
    return r;
}

// first kernel of a draw: per-chunk partial (sum for LEARNED, max for PRIOR) + clears the three digit histograms
template <int MODE>
__global__ void __launch_bounds__(kThreads) small_reduce_first(const float* __restrict__ p, int64_t E, float* __restrict__ part,
                                                              uint32_t* __restrict__ hist3, const int64_t* __restrict__ dynE) {
    __shared__ float red[kThreads / 64];
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < 3 * kBins; i += gridDim.x * kThreads) hist3[i] = 0;
    int64_t nblk_ = 0;
    if (!dyn_range(dynE, E, nblk_)) return;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kChunk;
    float acc = (MODE == 1) ? -INFINITY : 0.f;
    // (loads first, unconditional on clamped indices, then the arithmetic: a load under `if (e < E)` with its use inside the branch is
    //  waited for inside the branch -- the unrolled items went through memory one after the other)
    float pv[kItems];
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
        pv[i] = p ? p[e < E ? e : E - 1] : 1.f;
    }
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
        if (e < E) {
            if (MODE == 1) acc = fmaxf(acc, pv[i]);
            else acc += pv[i];
        }
    }
    if (MODE == 1) {
        const float r = block_max(acc, red);
        if (threadIdx.x == 0) part[blockIdx.x] = r;
    } else {
        const float r = block_sum(acc, red);
        if (threadIdx.x == 0) part[blockIdx.x] = r;
    }
}

// PRIOR only: per-chunk partial of sum(exp(p - max)); the max is re-reduced by every workgroup from part_max
__global__ void __launch_bounds__(kThreads) small_reduce_sumexp(const float* __restrict__ p, int64_t E, const float* __restrict__ part_max,
                                                               int64_t nblk, float* __restrict__ part_sum, const int64_t* __restrict__ dynE) {
    __shared__ float red[kThreads / 64];
    if (!dyn_range(dynE, E, nblk)) return;
    const float mx = final_reduce_all<1>(part_max, nblk, red);
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kChunk;
    float acc = 0.f;
    float pv[kItems];
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
        pv[i] = p[e < E ? e : E - 1];
    }
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
        if (e < E) acc += expf(pv[i] - mx);
    }
    const float r = block_sum(acc, red);
    if (threadIdx.x == 0) part_sum[blockIdx.x] = r;
}

// The key pass: 2 048 edges per workgroup as everywhere (one histogram flush and one redundant reduction per 2 048 keys), but 1 024 threads
// with TWO edges each.  With 256 threads x 8 edges (rounds 1-2) a partition's 172-242 workgroups put one wave on a SIMD, each running eight
// Philox draws back to back behind the reductions' round trips: 19 us under the counters, 65 % of it waiting (r03 PMC).  Sixteen waves per
// workgroup overlap those latencies.  (512-edge workgroups were tried in round 2: slower, four times the flushes and reductions.)
constexpr int kKeyThreads = 1024;
constexpr int kKeyItems = kChunk / kKeyThreads;
template <int MODE>
__global__ void __launch_bounds__(kKeyThreads) small_keys_hist0(const float* __restrict__ p, const float* __restrict__ prior,
                                                               const float* __restrict__ noise, uint64_t seed, uint64_t stream_id,
                                                               const uint64_t* __restrict__ epoch, int64_t E, float one_minus_c, float c,
                                                               const float* __restrict__ part_sum, const float* __restrict__ part_max,
                                                               int64_t nblk, float* __restrict__ scal, uint32_t* __restrict__ keys,
                                                               float* __restrict__ keys_out, uint32_t* __restrict__ hist0,
                                                               const int64_t* __restrict__ dynE) {
    __shared__ uint32_t lh[kBins];
    __shared__ float red[kKeyThreads / 64];
    if (!dyn_range(dynE, E, nblk)) return;
    for (int i = threadIdx.x; i < kBins; i += kKeyThreads) lh[i] = 0;
    seed = fold_epoch(seed, epoch);
    const bool has_prior = prior != nullptr;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kChunk;
    // every load of the thread in flight before the reductions' barriers and before the first use
    float pv[kKeyItems], qv[kKeyItems], nv[kKeyItems];
#pragma unroll
    for (int i = 0; i < kKeyItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kKeyThreads + threadIdx.x;
        const int64_t ec = e < E ? e : E - 1;
        pv[i] = p ? p[ec] : 1.f;
        qv[i] = has_prior ? prior[ec] : 0.f;
        nv[i] = noise ? noise[ec] : 0.f;
    }
    const float mx = (MODE == SGS_SAMPLE_PRIOR) ? final_reduce_all<1>(part_max, nblk, red) : 0.f;
    const float Z = final_reduce_all<0>(part_sum, nblk, red);          // (syncs: lh is cleared for everyone)
    if (blockIdx.x == 0 && threadIdx.x == 0) { scal[0] = Z; scal[1] = mx; }
    const float Zeps = (MODE == SGS_SAMPLE_LEARNED) ? __fadd_rn(Z, 1e-12f) : Z;
    // all keys in registers BEFORE the first store: vmcnt counts stores too on this target, and behind per-item branches the compiler's
    // wait for an item's (long finished) loads was vmcnt(0) -- i.e. for the previous item's key store
    float kf[kKeyItems];
#pragma unroll
    for (int i = 0; i < kKeyItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kKeyThreads + threadIdx.x;
        kf[i] = 0.f;
        if (e < E) {
            const float s = sample_prob<MODE>(pv[i], Zeps, mx, qv[i], has_prior, one_minus_c, c);
            const float nz = noise ? nv[i] : exp_noise_at(seed, stream_id, static_cast<uint64_t>(e));
            kf[i] = __fdiv_rn(s, nz);
        }
    }
#pragma unroll
    for (int i = 0; i < kKeyItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kKeyThreads + threadIdx.x;
        if (e < E) {
            const uint32_t bits = __float_as_uint(kf[i]);
            keys[e] = bits;
            if (keys_out) keys_out[e] = kf[i];
            atomicAdd(&lh[bits >> kShift0], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kKeyThreads) {
        const uint32_t v = lh[i];
        if (v) atomicAdd(&hist0[i], v);
    }
}

// pass d (1 or 2): every workgroup first finishes digit d-1 from the complete hist_prev (+ the state workgroup 0 of the
// previous pass published), then histograms digit d of the keys matching the prefix; workgroup 0 publishes the state.
__device__ __forceinline__ void small_hist_next_body(const uint32_t* __restrict__ keys, int64_t E, int shift, uint32_t digit_mask,
                                                     int prev_shift, int first, uint32_t q, const uint32_t* __restrict__ hist_prev,
                                                     const SelPart* __restrict__ sel_in, SelPart* __restrict__ sel_out,
                                                     uint32_t* __restrict__ hist, const int64_t* __restrict__ dynE) {
    __shared__ uint32_t lh[kBins];
    int64_t nblk_ = 0;
    if (!dyn_range(dynE, E, nblk_)) return;
    for (int i = threadIdx.x; i < kBins; i += kThreads) lh[i] = 0;
    const uint32_t k = first ? q : sel_in->k_rem;
    const uint32_t pre = first ? 0u : sel_in->prefix;
    const uint2 f = select_digit_local(hist_prev, k);                  // (syncs: lh is cleared for everyone)
    const uint32_t prefix = pre | (f.x << prev_shift);
    if (blockIdx.x == 0 && threadIdx.x == 0) { sel_out->prefix = prefix; sel_out->k_rem = k - f.y; }
    const uint32_t want = prefix >> prev_shift;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kChunk;
    uint32_t kv[kItems];
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
        kv[i] = keys[e < E ? e : E - 1];
    }
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
        if (e < E && (kv[i] >> prev_shift) == want) atomicAdd(&lh[(kv[i] >> shift) & digit_mask], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kThreads) {
        const uint32_t v = lh[i];
        if (v) atomicAdd(&hist[i], v);
    }
}
// pass 1 (first = 1) or 2: the draw's three digit histograms are consecutive at ds.hist + d * ds.hs
__global__ void __launch_bounds__(kThreads) small_hist_next(DrawSet ds, int64_t E, int shift, uint32_t digit_mask, int prev_shift, int first,
                                                           uint32_t q, const int64_t* __restrict__ dynE) {
    const int64_t d = blockIdx.y;
    uint32_t* h = ds.hist + d * ds.hs;
    const int pass = first ? 1 : 2;
    small_hist_next_body(ds.keys + d * ds.ks, E, shift, digit_mask, prev_shift, first, q, h + (pass - 1) * kBins,
                         first ? nullptr : ds.sel + 2 * d, ds.sel + 2 * d + (first ? 0 : 1), h + pass * kBins, dynE);
}

// every workgroup finishes the last digit (threshold T, ties to take), counts its chunk; workgroup 0 publishes the final
// SelectState and the stats
__device__ __forceinline__ void small_count_body(const uint32_t* __restrict__ keys, int64_t E, uint32_t q,
                                                 const uint32_t* __restrict__ hist2, const SelPart* __restrict__ sel_in,
                                                 SelectState* __restrict__ st, uint2* __restrict__ cnt, const float* __restrict__ scal,
                                                 float* __restrict__ stats, const int64_t* __restrict__ dynE) {
    __shared__ int red[2 * (kThreads / 64)];
    int64_t nblk_ = 0;
    if (!dyn_range(dynE, E, nblk_)) return;
    const uint32_t k = sel_in->k_rem;
    const uint2 f = select_digit_local(hist2, k);
    const uint32_t T = sel_in->prefix | (f.x << kShift2);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->prefix = T;
        st->k_rem = k - f.y;
        st->n_gt = q - (k - f.y);
        st->pad = 0;
        if (stats) {
            stats[0] = scal[0];
            stats[1] = scal[1];
            stats[2] = __uint_as_float(T);
            stats[3] = static_cast<float>(k - f.y);
        }
    }
    const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kItems;
    uint32_t kk[kItems];
    load_keys8(keys, e0, E, kk);
    int gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const bool in = e0 + j < E;
        gt += (in && kk[j] > T);
        eq += (in && kk[j] == T);
    }
    gt = wave_sum_int_all(gt);
    eq = wave_sum_int_all(eq);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[2 * wid] = gt; red[2 * wid + 1] = eq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int g = 0, q_ = 0;
        for (int w = 0; w < kThreads / 64; ++w) { g += red[2 * w]; q_ += red[2 * w + 1]; }
        cnt[blockIdx.x] = make_uint2(static_cast<uint32_t>(g), static_cast<uint32_t>(q_));
    }
}
__global__ void __launch_bounds__(kThreads) small_count(DrawSet ds, int64_t E, uint32_t q, const float* __restrict__ scal,
                                                       float* __restrict__ stats, const int64_t* __restrict__ dynE) {
    const int64_t d = blockIdx.y;
    small_count_body(ds.keys + d * ds.ks, E, q, ds.hist + d * ds.hs + 2 * kBins, ds.sel + 2 * d + 1, ds.st + d, ds.cnt + d * ds.cs, scal,
                     opt_row(stats, 4 * d), dynE);
}

// compaction with the exclusive prefix over the preceding chunks' (gt, eq) counts recomputed by each workgroup
__device__ __forceinline__ void small_compact_body(const uint32_t* __restrict__ keys, int64_t E, int64_t q, const SelectState* __restrict__ st,
                                                   const uint2* __restrict__ cnt, const float* __restrict__ p,
                                                   const int64_t* __restrict__ edge_index, uint8_t* __restrict__ mask, int mask_aligned,
                                                   int64_t* __restrict__ sampled_eid, int64_t* __restrict__ sei,
                                                   float* __restrict__ sampled_p, const int64_t* __restrict__ dynE) {
    __shared__ int red[2 * (kThreads / 64)];
    __shared__ uint32_t pre[2];
    const int64_t Ecap = E;                       // row stride of edge_index (the capacity under sgs_dyn_edges_set)
    int64_t nblk_ = 0;
    if (!dyn_range(dynE, E, nblk_)) return;
    int g = 0, e = 0;
    for (int i = threadIdx.x; i < static_cast<int>(blockIdx.x); i += kThreads) { g += static_cast<int>(cnt[i].x); e += static_cast<int>(cnt[i].y); }
    g = wave_sum_int_all(g);
    e = wave_sum_int_all(e);
    if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = g; red[2 * (threadIdx.x >> 6) + 1] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int G = 0, Q = 0;
        for (int w = 0; w < kThreads / 64; ++w) { G += red[2 * w]; Q += red[2 * w + 1]; }
        pre[0] = static_cast<uint32_t>(G);
        pre[1] = static_cast<uint32_t>(Q);
    }
    __syncthreads();
    compact_body(pre[0], pre[1], keys, E, Ecap, q, int64_t(-1), int64_t(0), st, p, edge_index, mask, mask_aligned, sampled_eid, sei, sampled_p);
}
__global__ void __launch_bounds__(kThreads) small_compact(DrawSet ds, int64_t E, int64_t q, const float* __restrict__ p,
                                                         const int64_t* __restrict__ edge_index, DrawOut out,
                                                         const int64_t* __restrict__ dynE) {
    const int64_t d = blockIdx.y;
    const DrawOut o = out_row(out, d, E, q);
    small_compact_body(ds.keys + d * ds.ks, E, q, ds.st + d, ds.cnt + d * ds.cs, p, edge_index, o.mask,
                       (reinterpret_cast<uintptr_t>(o.mask) & 7) == 0, o.eid, o.sei, o.p, dynE);
}

// ---------------------------------------------------------------- node-covering draws (sgs_sample_topq_cover)
// After the key pass: every node's best non-loop in-edge (largest key, ties to the lowest edge id) gets bit 31 of its key set
// (keys >= 0, so the bit is free and the top radix digit already spans it); the radix select, count and compaction then run
// over the boosted keys unchanged.  The rows of the destination CSR partition the edges, so a row reads and writes only its
// own keys: no ordering between rows is needed.  LPR lanes share a row (sgs_sample_topq_cover_variant: 4 / 16 / 64 from the
// mean in-degree); a row of more than kCoverLongPerLane entries per lane (128 / 512 / 2048) is handed to the whole workgroup
// instead, so neither a 20 000-entry row serialises behind four lanes nor 64 lanes idle on degree-3 rows.  The digit-0 histogram the key pass accumulated is
// corrected by MOVING one count per forced edge from bin b to bin b + 1024 (integer atomics, first aggregated per workgroup
// in LDS): all counting stays integer, so the draw does not depend on the launch geometry or on the order of the atomics.
constexpr int kCoverThreads = 256;
constexpr int kCoverGrid = 1024;       // workgroups at most (grid-stride over the rows); also the length of the per-workgroup counts
constexpr int kCoverLongPerLane = 32;  // entries per lane of a row's group above which the whole workgroup takes the row

// (key bits << 32 | ~edge id) of CSR entry j of `row`, 0 for a self-loop: a 64-bit max is "largest key, then lowest edge id".
// keys == nullptr (degenerate draws, M only): any non-loop entry counts.
__device__ __forceinline__ unsigned long long cover_cand(const uint32_t* __restrict__ keys, uint32_t E, const int32_t* __restrict__ in_src,
                                                         const int32_t* __restrict__ in_eid, int64_t j, int64_t row) {
    const uint32_t eid = static_cast<uint32_t>(in_eid[j]);
    if (static_cast<int64_t>(in_src[j]) == row || eid >= E) return 0ull;
    const uint32_t bits = keys ? keys[eid] : 0u;
    return (static_cast<unsigned long long>(bits) << 32) | static_cast<uint32_t>(~eid);      // ~eid != 0: eid < E <= 2^31 - 1
}
__device__ __forceinline__ void cover_boost(unsigned long long best, uint32_t* __restrict__ keys, uint32_t* moved, uint32_t* nforced) {
    const uint32_t eid = ~static_cast<uint32_t>(best), bits = static_cast<uint32_t>(best >> 32);
    if (keys) {
        keys[eid] = bits | 0x80000000u;
        atomicAdd(&moved[(bits >> kShift0) & (kBins / 2 - 1)], 1u);
    }
    atomicAdd(nforced, 1u);
}
template <int LPR>
__global__ void __launch_bounds__(kCoverThreads) cover_rows(uint32_t* __restrict__ keys, int64_t E, int64_t N, const int32_t* __restrict__ in_ptr,
                                                           const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                           uint32_t* __restrict__ hist0, uint32_t* __restrict__ mcnt,
                                                           const int64_t* __restrict__ dynE) {
    constexpr int RPB = kCoverThreads / LPR;          // rows per workgroup and sweep
    constexpr int kLong = kCoverLongPerLane * LPR;    // a group walks at most 32 dependent gathers per lane
    __shared__ uint32_t moved[kBins / 2];             // forced keys per (unboosted) top digit
    __shared__ uint32_t longrow[RPB];
    __shared__ uint32_t nlong, nforced;
    __shared__ unsigned long long wbest[kCoverThreads / 64];
    if (dynE) {
        const int64_t live = *dynE;                   // rows past the live nodes are empty: their pointers are padded with the live E
        if (live < E) E = live;
    }
    for (int i = threadIdx.x; i < kBins / 2; i += kCoverThreads) moved[i] = 0;
    if (threadIdx.x == 0) { nlong = 0; nforced = 0; }
    __syncthreads();
    const uint32_t E32 = static_cast<uint32_t>(E);
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * RPB; base < N; base += static_cast<int64_t>(gridDim.x) * RPB) {
        const int64_t row = base + grp;
        unsigned long long best = 0ull;
        if (row < N) {
            int64_t s = in_ptr[row], t = in_ptr[row + 1];
            if (s < 0) s = 0;
            if (t > E) t = E;
            if (t - s > kLong) {
                if (sub == 0) longrow[atomicAdd(&nlong, 1u)] = static_cast<uint32_t>(row);
            } else {
                for (int64_t j = s + sub; j < t; j += LPR) {
                    const unsigned long long c = cover_cand(keys, E32, in_src, in_eid, j, row);
                    best = c > best ? c : best;
                }
            }
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) {
            const unsigned long long c = __shfl_xor(best, o, 64);
            best = c > best ? c : best;
        }
        if (sub == 0 && best) cover_boost(best, keys, moved, &nforced);
        __syncthreads();
        const uint32_t nl = nlong;
        for (uint32_t l = 0; l < nl; ++l) {           // (uniform: every thread reads the same nlong)
            const int64_t lrow = longrow[l];
            int64_t s = in_ptr[lrow], t = in_ptr[lrow + 1];
            if (s < 0) s = 0;
            if (t > E) t = E;
            unsigned long long b = 0ull;
            for (int64_t j = s + threadIdx.x; j < t; j += kCoverThreads) {
                const unsigned long long c = cover_cand(keys, E32, in_src, in_eid, j, lrow);
                b = c > b ? c : b;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long c = __shfl_xor(b, o, 64);
                b = c > b ? c : b;
            }
            if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = b;
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int w = 1; w < kCoverThreads / 64; ++w) b = wbest[w] > b ? wbest[w] : b;
                if (b) cover_boost(b, keys, moved, &nforced);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) nlong = 0;
        __syncthreads();
    }
    if (hist0)
        for (int i = threadIdx.x; i < kBins / 2; i += kCoverThreads) {
            const uint32_t v = moved[i];
            if (v) { atomicSub(&hist0[i], v); atomicAdd(&hist0[i + kBins / 2], v); }
        }
    if (threadIdx.x == 0) mcnt[blockIdx.x] = nforced;
}

// One workgroup, last launch of a covering draw: M from the per-workgroup counts, the flag bit off the reported threshold.
__device__ __forceinline__ void cover_finish_body(const uint32_t* __restrict__ mcnt, int nb, int64_t q, float* __restrict__ stats,
                                                  int32_t* __restrict__ cover_info) {
    __shared__ int red[kThreads / 64];
    int m = 0;
    for (int i = threadIdx.x; i < nb; i += kThreads) m += static_cast<int>(mcnt[i]);
    m = wave_sum_int_all(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        int M = 0;
        for (int w = 0; w < kThreads / 64; ++w) M += red[w];
        if (cover_info) {
            cover_info[0] = M;
            cover_info[1] = static_cast<int64_t>(M) < q ? M : static_cast<int32_t>(q);
        }
        if (stats) stats[2] = __uint_as_float(__float_as_uint(stats[2]) & 0x7FFFFFFFu);
    }
}
// ms = kCoverGrid, or 0 when one key-less cover_rows counted M for all draws (degenerate q)
__global__ void __launch_bounds__(kThreads) cover_finish(const uint32_t* __restrict__ mcnt, int64_t ms, int nb, int64_t q,
                                                        float* __restrict__ stats, int32_t* __restrict__ cover_info) {
    const int64_t d = blockIdx.y;
    cover_finish_body(mcnt + d * ms, nb, q, opt_row(stats, 4 * d), opt_row(cover_info, 2 * d));
}

// counts[0] = #keys > threshold, counts[1] = #keys == threshold in this shard (before the scan).
__global__ void __launch_bounds__(kThreads) total_counts(const uint2* __restrict__ cnt, int64_t nblk, uint32_t* __restrict__ counts) {
    __shared__ int red[2 * (kThreads / 64)];
    int g = 0, e = 0;
    for (int64_t i = threadIdx.x; i < nblk; i += kThreads) { g += static_cast<int>(cnt[i].x); e += static_cast<int>(cnt[i].y); }
    g = wave_sum_int_all(g);
    e = wave_sum_int_all(e);
    if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = g; red[2 * (threadIdx.x >> 6) + 1] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int G = 0, Q = 0;
        for (int w = 0; w < kThreads / 64; ++w) { G += red[2 * w]; Q += red[2 * w + 1]; }
        counts[0] = static_cast<uint32_t>(G);
        counts[1] = static_cast<uint32_t>(Q);
    }
}

__global__ void write_stats(const float* __restrict__ scal, const SelectState* __restrict__ st, float* __restrict__ stats) {
    const int d = blockIdx.y;
    stats[4 * d + 0] = scal[0];
    stats[4 * d + 1] = scal[1];
    stats[4 * d + 2] = __uint_as_float(st[d].prefix);
    stats[4 * d + 3] = static_cast<float>(st[d].k_rem);
}

// degenerate draws: nothing (value 0) or everything (value 1, q == E)
__global__ void select_all(int64_t E, const float* __restrict__ p, const int64_t* __restrict__ edge_index, DrawOut out, uint8_t value) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const DrawOut o = out_row(out, blockIdx.y, E, E);
    o.mask[e] = value;
    if (value) {
        if (o.eid) o.eid[e] = e;
        if (o.sei) { o.sei[e] = edge_index[e]; o.sei[E + e] = edge_index[E + e]; }
        if (o.p) o.p[e] = p ? p[e] : 1.f;
    }
}

// out[0, j] = edge_index[0, idx[j]], out[1, j] = edge_index[1, idx[j]]  (sampling.py:161-163: edge_index[:, sampled_indices])
__global__ void gather_columns_kernel(const int64_t* __restrict__ edge_index, int64_t E, const int64_t* __restrict__ idx, int64_t q,
                                      int64_t* __restrict__ out) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j >= q) return;
    const int64_t e = idx[j];
    const bool ok = e >= 0 && e < E;                  // out-of-range indices give (-1, -1) columns instead of a fault
    out[j] = ok ? edge_index[e] : int64_t(-1);
    out[q + j] = ok ? edge_index[E + e] : int64_t(-1);
}

__global__ void exp_noise_kernel(uint64_t seed, uint64_t stream_id, const uint64_t* __restrict__ epoch, int64_t E, float* __restrict__ noise) {
    seed = fold_epoch(seed, epoch);
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e < E) noise[e] = exp_noise_at(seed, stream_id, static_cast<uint64_t>(e));
}

__global__ void dropout_keep_kernel(uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch, int64_t rows, int64_t cols,
                                    uint32_t thresh, uint8_t* __restrict__ keep) {
    seed = fold_epoch(seed, epoch);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < rows * cols) {
        const int64_t r = i / cols;
        const uint32_t c = static_cast<uint32_t>(i - r * cols);
        keep[i] = dropout_keep_at(seed, site, static_cast<uint64_t>(r), c, thresh) ? 1 : 0;
    }
}

// ---------------------------------------------------------------- straight-through weights
// sampling.py:137-138,155:  w = clamp(p * ((one_hot - s).detach() + s), 0, 1)[mask]
template <bool HAS_PRIOR>
__device__ __forceinline__ void st_fwd_body(const float* __restrict__ p, const float* __restrict__ prior, float one_minus_c, float c,
                                            const float* __restrict__ stats, const int64_t* __restrict__ eid, int64_t q,
                                            float* __restrict__ w) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j >= q) return;
    const int64_t e = eid[j];
    const float Zeps = __fadd_rn(stats[0], 1e-12f);
    const float pv = p[e];
    float s = __fdiv_rn(pv, Zeps);
    if (HAS_PRIOR) s = __fadd_rn(__fmul_rn(one_minus_c, s), __fmul_rn(c, prior[e]));
    const float st = __fadd_rn(__fsub_rn(1.0f, s), s);
    const float v = __fmul_rn(pv, st);
    w[j] = fminf(fmaxf(v, 0.f), 1.f);
}
template <bool HAS_PRIOR>
__global__ void st_fwd(const float* __restrict__ p, const float* __restrict__ prior, float one_minus_c, float c,
                       const float* __restrict__ stats, const int64_t* __restrict__ eid, int64_t q, float* __restrict__ w) {
    const int64_t d = blockIdx.y;
    st_fwd_body<HAS_PRIOR>(p, prior, one_minus_c, c, stats + 4 * d, eid + d * q, q, w + d * q);
}

// backward: h_e = g_e [0 <= p_e st_e <= 1];  S = sum_sel h_e p_e^2
//   dp_k = -(a/Z'^2) S  (all k)  +  [k sel] h_k (st_k + a p_k / Z'),  a = (1-c) or 1 (istest)
template <bool HAS_PRIOR>
__global__ void __launch_bounds__(kThreads) st_bwd_partial(const float* __restrict__ p, const float* __restrict__ prior,
                                                          float one_minus_c, float c, const float* __restrict__ stats,
                                                          const int64_t* __restrict__ eid, const float* __restrict__ gw,
                                                          int64_t q, float* __restrict__ part) {
    __shared__ float red[kThreads / 64];
    float acc = 0.f;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kChunk;
    const float Zeps = stats[0] + 1e-12f;
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const int64_t j = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
        if (j < q) {
            const int64_t e = eid[j];
            const float pv = p[e];
            float s = pv / Zeps;
            if (HAS_PRIOR) s = one_minus_c * s + c * prior[e];
            const float v = pv * ((1.0f - s) + s);
            const float h = (v >= 0.f && v <= 1.f) ? gw[j] : 0.f;
            acc += h * pv * pv;
        }
    }
    const float r = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ void __launch_bounds__(kThreads) st_bwd_final(const float* __restrict__ part, int64_t n, float* __restrict__ S) {
    __shared__ float red[kThreads / 64];
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) acc += part[i];
    const float r = block_sum(acc, red);
    if (threadIdx.x == 0) S[0] = r;
}

__global__ void st_bwd_dense(const float* __restrict__ S, const float* __restrict__ stats, float a, int64_t E,
                             float* __restrict__ dp, const int64_t* __restrict__ dynE) {
    const int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= E) return;
    const float Zeps = stats[0] + 1e-12f;
    // under sgs_dyn_edges_set the entries between the live count and the capacity are not edges: exactly zero gradient
    dp[k] = (dynE && k >= *dynE) ? 0.f : -(a / (Zeps * Zeps)) * S[0];

}

template <bool HAS_PRIOR>
__global__ void st_bwd_sparse(const float* __restrict__ p, const float* __restrict__ prior, float one_minus_c, float c,
                              float a, const float* __restrict__ stats, const int64_t* __restrict__ eid,
                              const float* __restrict__ gw, int64_t q, float* __restrict__ dp) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j >= q) return;
    const int64_t e = eid[j];
    const float Zeps = stats[0] + 1e-12f;
    const float pv = p[e];
    float s = pv / Zeps;
    if (HAS_PRIOR) s = one_minus_c * s + c * prior[e];
    const float st = (1.0f - s) + s;
    const float v = pv * st;
    const float h = (v >= 0.f && v <= 1.f) ? gw[j] : 0.f;
    dp[e] += h * (st + a * pv / Zeps);   // eids are unique: no race
}


// ---------------------------------------------------------------- D draws of one candidate set in one pass (ensemble evaluation)
// sgs_sample_topq_multi: draw d is sgs_sample_topq with stream id stream_id0 + d (or noise row d), bit for bit -- the same bodies run
// with a draw index in the grid (blockIdx.y), so every radix-select stage is ONE launch for all D draws.  The normaliser (Z, or max and
// sum of exp) does not depend on the noise: it is reduced once.  The key pass loads p / prior once per edge and loops over a group of
// kMultiG draws with one LDS histogram each; it STORES the D key arrays (rows padded to 64 keys, so load_keys8's 16-byte loads stay
// aligned) rather than recomputing them from the hash in the three later passes: at partition scale the D x 4E bytes stay in the
// Infinity Cache, and a recompute would put three more Philox evaluations per key and draw on passes that are otherwise pure loads.
constexpr int kMultiG = 4;                   // draws per key-pass workgroup: 4 x 8 KiB of LDS histograms beside 16 waves
constexpr int kMultiCoverG = 2;              // draws per workgroup of a batched pass's cover_rows (1, 2 or 4; measured: DESIGN.md section 5)

__host__ __device__ inline int64_t multi_key_stride(int64_t E) { return (E + 63) & ~int64_t(63); }

template <int MODE>
__global__ void __launch_bounds__(kKeyThreads) multi_keys_hist0(const float* __restrict__ p, const float* __restrict__ prior,
                                                               const float* __restrict__ noise, uint64_t seed, uint64_t stream_id0,
                                                               const uint64_t* __restrict__ epoch, int64_t E, int D, float one_minus_c, float c,
                                                               const float* __restrict__ part_sum, const float* __restrict__ part_max,
                                                               int64_t nblk, float* __restrict__ scal, uint32_t* __restrict__ keys,
                                                               int64_t ks, uint32_t* __restrict__ hist3) {
    __shared__ uint32_t lh[kMultiG][kBins];
    __shared__ float red[kKeyThreads / 64];
    const int d0 = blockIdx.y * kMultiG;
    const int G = (D - d0) < kMultiG ? (D - d0) : kMultiG;
    for (int i = threadIdx.x; i < kMultiG * kBins; i += kKeyThreads) (&lh[0][0])[i] = 0;
    seed = fold_epoch(seed, epoch);
    const bool has_prior = prior != nullptr;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kChunk;
    float pv[kKeyItems], qv[kKeyItems];
#pragma unroll
    for (int i = 0; i < kKeyItems; ++i) {
        const int64_t e = base + static_cast<int64_t>(i) * kKeyThreads + threadIdx.x;
        const int64_t ec = e < E ? e : E - 1;
        pv[i] = p ? p[ec] : 1.f;
        qv[i] = has_prior ? prior[ec] : 0.f;
    }
    const float mx = (MODE == SGS_SAMPLE_PRIOR) ? final_reduce_all<1>(part_max, nblk, red) : 0.f;
    const float Z = final_reduce_all<0>(part_sum, nblk, red);          // (syncs: lh is cleared for everyone)
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { scal[0] = Z; scal[1] = mx; }
    const float Zeps = (MODE == SGS_SAMPLE_LEARNED) ? __fadd_rn(Z, 1e-12f) : Z;
    float sv[kKeyItems];
#pragma unroll
    for (int i = 0; i < kKeyItems; ++i) sv[i] = sample_prob<MODE>(pv[i], Zeps, mx, qv[i], has_prior, one_minus_c, c);
    for (int g = 0; g < G; ++g) {
        const int d = d0 + g;
        float kf[kKeyItems];
#pragma unroll
        for (int i = 0; i < kKeyItems; ++i) {
            const int64_t e = base + static_cast<int64_t>(i) * kKeyThreads + threadIdx.x;
            kf[i] = 0.f;
            if (e < E) {
                const float nz = noise ? noise[static_cast<int64_t>(d) * E + e] : exp_noise_at(seed, stream_id0 + d, static_cast<uint64_t>(e));
                kf[i] = __fdiv_rn(sv[i], nz);
            }
        }
#pragma unroll
        for (int i = 0; i < kKeyItems; ++i) {
            const int64_t e = base + static_cast<int64_t>(i) * kKeyThreads + threadIdx.x;
            if (e < E) {
                const uint32_t bits = __float_as_uint(kf[i]);
                keys[static_cast<int64_t>(d) * ks + e] = bits;
                atomicAdd(&lh[g][bits >> kShift0], 1u);
            }
        }
    }
    __syncthreads();
    for (int g = 0; g < G; ++g)
        for (int i = threadIdx.x; i < kBins; i += kKeyThreads) {
            const uint32_t v = lh[g][i];
            if (v) atomicAdd(&hist3[static_cast<int64_t>(d0 + g) * 3 * kBins + i], v);
        }
}

// ---------------------------------------------------------------- node-covering draws of the batched pass (sgs_sample_topq_multi_cover)
// cover_rows for a GROUP of G draws (blockIdx.y): the key rows keys + d * ks share one candidate graph, so a lane reads a CSR entry
// (in_src[j], in_eid[j]) once and gathers that edge's key from each of the group's rows -- G independent gathers in flight per entry
// where the single-draw kernel has one -- with one 64-bit (bits << 32 | ~eid) running maximum per draw in registers.  The winner of
// draw d gets bit 31 in d's own key row and moves one count of d's digit-0 histogram (hist + d * hs) from bin b to bin b + 1024, first
// aggregated per (workgroup, draw) in LDS (4 KiB per draw of the group), flushed as integer atomicSub / atomicAdd pairs.  Rows, lanes
// per row, the hand-over of long rows to the whole workgroup, the bounds checks and the grid-stride are cover_rows'; per draw the
// comparisons are the same integers, so row d of the keys and histograms is bitwise what cover_rows leaves for that draw, whatever G.
// The last group is partial: its spare slots re-read the group's last row (no branch around the gathers) and force nothing.
// (A single covering draw does NOT run this kernel with G = 1: measured on an MI355X that form takes 0.4 to 0.7 us longer than
// cover_rows<LPR> at a partition's size -- 10.3 to 10.6 against 9.9 us -- for a reason that was not found; DESIGN.md.)
template <int G>
__device__ __forceinline__ void cover_cand_group(uint32_t* const (&krow)[G], uint32_t E, const int32_t* __restrict__ in_src,
                                                 const int32_t* __restrict__ in_eid, int64_t j, int64_t row, unsigned long long (&best)[G]) {
    const uint32_t eid = static_cast<uint32_t>(in_eid[j]);
    if (static_cast<int64_t>(in_src[j]) == row || eid >= E) return;
    uint32_t bits[G];
#pragma unroll
    for (int g = 0; g < G; ++g) bits[g] = krow[g][eid];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const unsigned long long c = (static_cast<unsigned long long>(bits[g]) << 32) | static_cast<uint32_t>(~eid);
        best[g] = c > best[g] ? c : best[g];
    }
}
template <int LPR, int G>
__global__ void __launch_bounds__(kCoverThreads) cover_rows_group(DrawSet ds, int64_t E, int64_t N, const int32_t* __restrict__ in_ptr,
                                                                 const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                                 uint32_t* __restrict__ mcnt) {
    constexpr int RPB = kCoverThreads / LPR;
    constexpr int kLong = kCoverLongPerLane * LPR;
    __shared__ uint32_t moved[G][kBins / 2];
    __shared__ uint32_t longrow[RPB];
    __shared__ uint32_t nlong, nforced[G];
    __shared__ unsigned long long wbest[G][kCoverThreads / 64];
    const int d0 = blockIdx.y * G;
    const int gn = (ds.D - d0) < G ? (ds.D - d0) : G;     // draws of this group (>= 1: the grid has ceil(D / G) groups)
    uint32_t* krow[G];
#pragma unroll
    for (int g = 0; g < G; ++g) krow[g] = ds.keys + static_cast<int64_t>(d0 + (g < gn ? g : gn - 1)) * ds.ks;
    for (int i = threadIdx.x; i < G * (kBins / 2); i += kCoverThreads) (&moved[0][0])[i] = 0;
    if (threadIdx.x < G) nforced[threadIdx.x] = 0;
    if (threadIdx.x == 0) nlong = 0;
    __syncthreads();
    const uint32_t E32 = static_cast<uint32_t>(E);
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * RPB; base < N; base += static_cast<int64_t>(gridDim.x) * RPB) {
        const int64_t row = base + grp;
        unsigned long long best[G];
#pragma unroll
        for (int g = 0; g < G; ++g) best[g] = 0ull;
        if (row < N) {
            int64_t s = in_ptr[row], t = in_ptr[row + 1];
            if (s < 0) s = 0;
            if (t > E) t = E;
            if (t - s > kLong) {
                if (sub == 0) longrow[atomicAdd(&nlong, 1u)] = static_cast<uint32_t>(row);
            } else {
                for (int64_t j = s + sub; j < t; j += LPR) cover_cand_group<G>(krow, E32, in_src, in_eid, j, row, best);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) {
                const unsigned long long c = __shfl_xor(best[g], o, 64);
                best[g] = c > best[g] ? c : best[g];
            }
        }
        if (sub == 0) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < gn && best[g]) cover_boost(best[g], krow[g], moved[g], &nforced[g]);
        }
        __syncthreads();
        const uint32_t nl = nlong;
        for (uint32_t l = 0; l < nl; ++l) {           // (uniform: every thread reads the same nlong)
            const int64_t lrow = longrow[l];
            int64_t s = in_ptr[lrow], t = in_ptr[lrow + 1];
            if (s < 0) s = 0;
            if (t > E) t = E;
            unsigned long long b[G];
#pragma unroll
            for (int g = 0; g < G; ++g) b[g] = 0ull;
            for (int64_t j = s + threadIdx.x; j < t; j += kCoverThreads) cover_cand_group<G>(krow, E32, in_src, in_eid, j, lrow, b);
#pragma unroll
            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned long long c = __shfl_xor(b[g], o, 64);
                    b[g] = c > b[g] ? c : b[g];
                }
                if ((threadIdx.x & 63) == 0) wbest[g][threadIdx.x >> 6] = b[g];
            }
            __syncthreads();
            if (threadIdx.x == 0) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    unsigned long long v = b[g];
                    for (int w = 1; w < kCoverThreads / 64; ++w) v = wbest[g][w] > v ? wbest[g][w] : v;
                    if (g < gn && v) cover_boost(v, krow[g], moved[g], &nforced[g]);
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) nlong = 0;
        __syncthreads();
    }
    for (int g = 0; g < gn; ++g) {
        uint32_t* h = ds.hist + static_cast<int64_t>(d0 + g) * ds.hs;
        for (int i = threadIdx.x; i < kBins / 2; i += kCoverThreads) {
            const uint32_t v = moved[g][i];
            if (v) { atomicSub(&h[i], v); atomicAdd(&h[i + kBins / 2], v); }
        }
    }
    if (static_cast<int>(threadIdx.x) < gn) mcnt[static_cast<int64_t>(d0 + threadIdx.x) * kCoverGrid + blockIdx.x] = nforced[threadIdx.x];
}

// ---------------------------------------------------------------- consensus of D draws (sgs_consensus_accum / sgs_consensus_select)
// The fold: count[e] (+)= #{d < Dc : mask[d, e] != 0}.  A thread owns 16 consecutive edges and keeps their 16 counts as packed bytes in two
// 64-bit words (Dc <= 127, so a byte never carries).  Row d's 16 bytes at mask + d * stride + e0 are rarely 16-byte aligned (the stride is E),
// so the thread loads the one or two ALIGNED 16-byte granules that hold them and shifts the bytes into place; a granule that is not wholly
// inside the mask block [mask, mask + (Dc - 1) * stride + E) -- the head of the first row, the tail of the last -- is read byte by byte, the
// bytes outside as 0, so nothing outside the block is ever touched.  The count histogram is privatised in LDS.
constexpr int kAccItems = 16;
constexpr int kAccChunk = kThreads * kAccItems;       // 4096 edges per workgroup
constexpr int kCountBins = 128;                       // counts 0..127
constexpr int kCountMax = kCountBins - 1;

__device__ __forceinline__ void load_granule(const uint8_t* g, const uint8_t* lo, const uint8_t* hi, uint64_t& a, uint64_t& b) {
    if (g >= lo && g + 16 <= hi) {
        const uint4 v = *reinterpret_cast<const uint4*>(g);
        a = (static_cast<uint64_t>(v.y) << 32) | v.x;
        b = (static_cast<uint64_t>(v.w) << 32) | v.z;
    } else {
        a = b = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (g + j >= lo && g + j < hi) a |= static_cast<uint64_t>(g[j]) << (8 * j);
            if (g + 8 + j >= lo && g + 8 + j < hi) b |= static_cast<uint64_t>(g[8 + j]) << (8 * j);
        }
    }
}
// 0x01 in every byte of x that is not 0
__device__ __forceinline__ uint64_t nonzero_bytes(uint64_t x) {
    constexpr uint64_t k7f = 0x7F7F7F7F7F7F7F7FULL;
    return ((((x & k7f) + k7f) | x) >> 7) & 0x0101010101010101ULL;
}
__device__ __forceinline__ int clamp_count(int c) { return c < 0 ? 0 : (c > kCountMax ? kCountMax : c); }

__global__ void __launch_bounds__(kThreads) consensus_accum_kernel(const uint8_t* __restrict__ mask, int64_t stride, int Dc, int64_t E, int first,
                                                                  int32_t* __restrict__ count, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t lh[kCountBins];
    if (hist) {
        if (threadIdx.x < kCountBins) lh[threadIdx.x] = 0;
        __syncthreads();
    }
    const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kAccChunk + static_cast<int64_t>(threadIdx.x) * kAccItems;
    if (e0 < E) {
        const uint8_t* lo = mask;
        const uint8_t* hi = Dc > 0 ? mask + static_cast<int64_t>(Dc - 1) * stride + E : mask;
        uint64_t acc0 = 0, acc1 = 0;
        for (int d = 0; d < Dc; ++d) {
            const uint8_t* a = mask + static_cast<int64_t>(d) * stride + e0;
            const int sh = static_cast<int>(reinterpret_cast<uintptr_t>(a) & 15);
            const uint8_t* g = a - sh;
            uint64_t w0, w1, w2 = 0, w3 = 0;
            load_granule(g, lo, hi, w0, w1);
            if (sh) load_granule(g + 16, lo, hi, w2, w3);
            if (sh >= 8) { w0 = w1; w1 = w2; w2 = w3; }
            const int s = 8 * (sh & 7);
            if (s) {
                w0 = (w0 >> s) | (w1 << (64 - s));
                w1 = (w1 >> s) | (w2 << (64 - s));
            }
            acc0 += nonzero_bytes(w0);
            acc1 += nonzero_bytes(w1);
        }
        // (bytes past the row's end were counted from the next row or as 0: they are never stored)
        const bool whole = e0 + kAccItems <= E && (reinterpret_cast<uintptr_t>(count + e0) & 15) == 0;
        int c[kAccItems];
        if (first) {
#pragma unroll
            for (int j = 0; j < kAccItems; ++j) c[j] = 0;
        } else if (whole) {
#pragma unroll
            for (int j = 0; j < kAccItems; j += 4) {
                const int4 v = *reinterpret_cast<const int4*>(count + e0 + j);
                c[j] = v.x; c[j + 1] = v.y; c[j + 2] = v.z; c[j + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kAccItems; ++j) c[j] = e0 + j < E ? count[e0 + j] : 0;
        }
#pragma unroll
        for (int j = 0; j < kAccItems; ++j) c[j] += static_cast<int>(((j < 8 ? acc0 : acc1) >> (8 * (j & 7))) & 0xFF);
        if (whole) {
#pragma unroll
            for (int j = 0; j < kAccItems; j += 4) *reinterpret_cast<int4*>(count + e0 + j) = make_int4(c[j], c[j + 1], c[j + 2], c[j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < kAccItems; ++j)
                if (e0 + j < E) count[e0 + j] = c[j];
        }
        if (hist) {
#pragma unroll
            for (int j = 0; j < kAccItems; ++j)
                if (e0 + j < E) atomicAdd(&lh[clamp_count(c[j])], 1u);
        }
    }
    if (hist) {
        __syncthreads();
        if (threadIdx.x < kCountBins) {
            const uint32_t v = lh[threadIdx.x];
            if (v) atomicAdd(&hist[threadIdx.x], static_cast<unsigned long long>(v));
        }
    }
}

// key_e = (count_e << 25) | (bits(p_e) >> 6): the count is the primary key, the score breaks ties among equal counts.  p == nullptr, or a
// score that is not >= 0 (negative, -0, NaN): low part 0.  A non-negative float's bits are below 2^31, so the low part is below 2^25.
__device__ __forceinline__ uint32_t consensus_key(int c, const float* __restrict__ p, int64_t e) {
    uint32_t low = 0;
    if (p) {
        const float v = p[e];
        const uint32_t b = __float_as_uint(v);
        if (v >= 0.f && !(b >> 31)) low = b >> 6;
    }
    return (static_cast<uint32_t>(clamp_count(c)) << 25) | low;
}
// The key pass with the first digit's histogram fused in, as keys_hist0 (grid-stride over the 2048-edge chunks; hist0 zeroed by the caller).
__global__ void __launch_bounds__(kThreads) consensus_keys_hist0(const int32_t* __restrict__ count, const float* __restrict__ p, int64_t E,
                                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ keys_out,
                                                                uint32_t* __restrict__ hist0) {
    __shared__ uint32_t lh[kBins];
    for (int i = threadIdx.x; i < kBins; i += kThreads) lh[i] = 0;
    __syncthreads();
    const int64_t nchunk = (E + kChunk - 1) / kChunk;
    for (int64_t chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {
        const int64_t base = chunk * kChunk;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const int64_t e = base + static_cast<int64_t>(i) * kThreads + threadIdx.x;
            if (e < E) {
                const uint32_t bits = consensus_key(count[e], p, e);
                keys[e] = bits;
                if (keys_out) keys_out[e] = bits;
                atomicAdd(&lh[bits >> kShift0], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kThreads) {
        const uint32_t v = lh[i];
        if (v) atomicAdd(&hist0[i], v);
    }
}
// count_out[i] = count[eid[i]] (clamped as the key clamps it) for the q selected edges
__global__ void consensus_gather_count(const int32_t* __restrict__ count, const int64_t* __restrict__ eid, int64_t q, int64_t E,
                                       int32_t* __restrict__ count_out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= q) return;
    const int64_t e = eid[i];
    count_out[i] = (e >= 0 && e < E) ? clamp_count(count[e]) : 0;
}

}  // namespace
}  // namespace sgs

using namespace sgs;

extern "C" {

int sgs_exp_noise(uint64_t seed, uint64_t stream_id, int64_t E, float* noise, sgs_stream_t stream) {
    SGS_REQUIRE(E >= 0 && (E == 0 || noise), SGS_EINVAL, "sgs_exp_noise: bad arguments");
    if (E == 0) return SGS_OK;
    hipLaunchKernelGGL(exp_noise_kernel, dim3(cdiv(E, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), seed,
                       stream_id, epoch_ptr(), E, noise);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_dropout_keep(uint64_t seed, uint32_t site, int64_t rows, int64_t cols, float p, uint8_t* keep,
                     sgs_stream_t stream) {
    SGS_REQUIRE(rows >= 0 && cols >= 0 && cols < (int64_t(1) << 32) && p >= 0.f && p < 1.f, SGS_EINVAL,
                "sgs_dropout_keep: bad arguments");
    if (rows * cols == 0) return SGS_OK;
    SGS_REQUIRE(keep, SGS_EINVAL, "sgs_dropout_keep: null output");
    hipLaunchKernelGGL(dropout_keep_kernel, dim3(cdiv(rows * cols, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), seed, site, epoch_ptr(), rows, cols, dropout_thresh(p), keep);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- one workspace layout
// Every carving of a draw's workspace for (E, D, covering?, consensus?); on a null base only `bytes`, the size, means anything.  scal, st
// and hist are adjacent, in that order: the large path clears them, through the one histogram per draw it uses, in one zero_async.  The
// key rows are padded to 64 keys (multi_key_stride) for load_keys8's 16-byte loads.
struct SamplerWs {
    uint32_t* keys; int64_t ks;
    float *part, *part2, *scal;     // per-chunk partials (sum or max; sum of exp); the scalars Z and max
    SelectState* st;
    uint32_t* hist;                 // 3 * kBins per draw: a draw's three digits on the small path; the first kBins * D as one row per draw on the large
    uint2* cnt; int64_t cs;
    SelPart* sel;
    uint32_t* mcnt;                 // covering draws: forced edges per (draw, workgroup of cover_rows)
    int64_t* eid;                   // consensus: edge ids for count_out when the caller asks for none
    size_t bytes;
};
static SamplerWs sampler_ws(void* base, int64_t E, int64_t D, bool cover, bool consensus) {
    if (E < 0) E = 0;
    if (D < 1) D = 1;
    SamplerWs w{};
    w.ks = multi_key_stride(E);
    w.cs = cdiv(E, kChunk) + 1;
    Carver cv(base);
    w.keys = cv.take<uint32_t>(w.ks * D);
    w.part = cv.take<float>(w.cs);
    w.part2 = cv.take<float>(w.cs);
    w.scal = cv.take<float>(4);
    w.st = cv.take<SelectState>(D);
    w.hist = cv.take<uint32_t>(3 * kBins * D);
    w.cnt = cv.take<uint2>(w.cs * D);
    w.sel = cv.take<SelPart>(2 * D);
    if (cover) w.mcnt = cv.take<uint32_t>(kCoverGrid * D);
    if (consensus) w.eid = cv.take<int64_t>(E);
    w.bytes = cv.off;
    return w;
}
static int check_ws(const char* fn, const void* ws, size_t ws_bytes, size_t ws_need) {
    SGS_REQUIRE(ws && ws_bytes >= ws_need, SGS_EWORKSPACE, "%s: workspace too small (%zu < %zu)", fn, ws_bytes, ws_need);
    SGS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, SGS_EINVAL, "%s: workspace must be 256-B aligned", fn);
    return SGS_OK;
}

// ---------------------------------------------------------------- one selection chain
// what a covering draw adds to the plain one (sgs_sample_topq[_multi]_cover); nullptr = the plain draw
struct CoverArgs {
    int64_t N;
    const int32_t *in_ptr, *in_src, *in_eid;
    int32_t* info;
    int lanes, grid, group;      // sgs_sample_topq_cover_variant of the shape; workgroups of cover_rows; draws per workgroup of it
    bool batched;                // sgs_sample_topq_multi_cover: a degenerate pass counts M before it writes the stats, a single draw after
};
// draws per workgroup of a batched pass's cover_rows (sgs_sample_topq_multi_cover_group_set); the result does not depend on it
static int g_multi_cover_group = kMultiCoverG;
static CoverArgs cover_args(int64_t N, int64_t E, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, int32_t* info, int group,
                            bool batched) {
    CoverArgs c{N, in_ptr, in_src, in_eid, info, sgs_sample_topq_cover_variant(N, E), 1, group, batched};
    if (N > 0) {
        const int64_t nb = cdiv(N, kCoverThreads / c.lanes);
        c.grid = static_cast<int>(nb < kCoverGrid ? nb : kCoverGrid);
    }
    return c;
}
// a single draw's forced-edge kernel.  keys == nullptr: count M only (degenerate draws); hist0 == nullptr: no histogram to correct
static void launch_cover_rows(const CoverArgs& c, uint32_t* keys, int64_t E, uint32_t* hist0, uint32_t* mcnt, const int64_t* dynE,
                              hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(c.grid)), blk(kCoverThreads);
    if (c.lanes == 4)
        hipLaunchKernelGGL(cover_rows<4>, grid, blk, 0, stream, keys, E, c.N, c.in_ptr, c.in_src, c.in_eid, hist0, mcnt, dynE);
    else if (c.lanes == 16)
        hipLaunchKernelGGL(cover_rows<16>, grid, blk, 0, stream, keys, E, c.N, c.in_ptr, c.in_src, c.in_eid, hist0, mcnt, dynE);
    else
        hipLaunchKernelGGL(cover_rows<64>, grid, blk, 0, stream, keys, E, c.N, c.in_ptr, c.in_src, c.in_eid, hist0, mcnt, dynE);
}
// a batched pass's: c.group draws per workgroup
template <int G>
static void launch_cover_rows_group_g(const CoverArgs& c, const DrawSet& ds, int64_t E, uint32_t* mcnt, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(c.grid), static_cast<unsigned>(cdiv(ds.D, G))), blk(kCoverThreads);
    if (c.lanes == 4)
        hipLaunchKernelGGL((cover_rows_group<4, G>), grid, blk, 0, stream, ds, E, c.N, c.in_ptr, c.in_src, c.in_eid, mcnt);
    else if (c.lanes == 16)
        hipLaunchKernelGGL((cover_rows_group<16, G>), grid, blk, 0, stream, ds, E, c.N, c.in_ptr, c.in_src, c.in_eid, mcnt);
    else
        hipLaunchKernelGGL((cover_rows_group<64, G>), grid, blk, 0, stream, ds, E, c.N, c.in_ptr, c.in_src, c.in_eid, mcnt);
}
static void launch_cover_rows_group(const CoverArgs& c, const DrawSet& ds, int64_t E, uint32_t* mcnt, hipStream_t stream) {
    if (c.group == 1) launch_cover_rows_group_g<1>(c, ds, E, mcnt, stream);
    else if (c.group == 2) launch_cover_rows_group_g<2>(c, ds, E, mcnt, stream);
    else launch_cover_rows_group_g<4>(c, ds, E, mcnt, stream);
}

enum SelPath { kSelAll, kSelSmall, kSelLarge };   // q == 0 or q == E; at most kSmallBlocks chunks (2 M candidate edges); more

// Everything of a draw set but its keys, once for sgs_sample_topq[_multi][_cover] and sgs_consensus_select.  key_pass(path, ds) launches
// the caller's zeroing, normalisers and key pass for the path chosen here (no keys on kSelAll).  The forced-edge kernel runs between it
// and the first selection pass; cover_finish after the stats are written, so before a caller's st_fwd.
//   kSelSmall: 4 launches, the one-workgroup steps between the passes recomputed by every workgroup (see "fused small-E path" above)
//   kSelLarge: 9 launches + the stats
template <class KeyPass>
static int select_chain(const SamplerWs& w, int64_t D, int64_t E, int64_t q, const float* p, const int64_t* edge_index, const DrawOut& out,
                        const CoverArgs* cover, const int64_t* dynE, hipStream_t stream, KeyPass key_pass) {
    const int64_t nblk = cdiv(E, kChunk);
    const SelPath path = (q == 0 || q == E) ? kSelAll : nblk <= kSmallBlocks ? kSelSmall : kSelLarge;
    // a draw's three digit histograms on the small path; one per draw, packed, on the large
    const DrawSet ds{w.keys, w.ks, w.hist, path == kSelSmall ? 3 * kBins : kBins, w.st, w.sel, w.cnt, w.cs, static_cast<int>(D)};
    const float* scal = w.scal;
    uint32_t* mcnt = w.mcnt;
    const unsigned Du = static_cast<unsigned>(ds.D), nb = static_cast<unsigned>(nblk);
    const dim3 blk(kThreads), grid(nb, Du), hgrid(nblk < kHistGrid ? nb : kHistGrid, Du), one(1, Du);
    const uint32_t q32 = static_cast<uint32_t>(q);
    if (int rc = key_pass(path, ds)) return rc;
    if (cover && path != kSelAll) {
        if (cover->batched) launch_cover_rows_group(*cover, ds, E, mcnt, stream);
        else launch_cover_rows(*cover, ds.keys, E, ds.hist, mcnt, dynE, stream);
    }
    if (path == kSelAll) {
        hipLaunchKernelGGL(select_all, dim3(static_cast<unsigned>(cdiv(E, 256)), Du), dim3(256), 0, stream, E, p, edge_index, out,
                           static_cast<uint8_t>(q == E ? 1 : 0));
    } else if (path == kSelSmall) {
        hipLaunchKernelGGL(small_hist_next, grid, blk, 0, stream, ds, E, kShift1, kMask1, kShift0, 1, q32, dynE);
        hipLaunchKernelGGL(small_hist_next, grid, blk, 0, stream, ds, E, kShift2, kMask2, kShift1, 0, q32, dynE);
        hipLaunchKernelGGL(small_count, grid, blk, 0, stream, ds, E, q32, scal, out.stats, dynE);
        hipLaunchKernelGGL(small_compact, grid, blk, 0, stream, ds, E, q, p, edge_index, out, dynE);
    } else {
        hipLaunchKernelGGL(select_digit, one, blk, 0, stream, ds, kShift0, 1, q32);
        hipLaunchKernelGGL(hist_next, hgrid, blk, 0, stream, ds, E, kShift1, kMask1, kShift0);
        hipLaunchKernelGGL(select_digit, one, blk, 0, stream, ds, kShift1, 0, q32);
        hipLaunchKernelGGL(hist_next, hgrid, blk, 0, stream, ds, E, kShift2, kMask2, kShift1);
        hipLaunchKernelGGL(select_digit, one, blk, 0, stream, ds, kShift2, 0, q32);
        hipLaunchKernelGGL(count_blocks, grid, blk, 0, stream, ds, E);
        hipLaunchKernelGGL(scan_blocks, one, blk, 0, stream, ds, nblk);
        hipLaunchKernelGGL(compact, grid, blk, 0, stream, ds, E, q, int64_t(-1), int64_t(0), p, edge_index, out);
    }
    // degenerate draws: M does not depend on the keys or on the draw -- one key-less launch counts the rows that have a non-loop entry,
    // and every draw's finishing workgroup reads those counts
    if (cover && path == kSelAll && cover->batched) launch_cover_rows(*cover, nullptr, E, nullptr, mcnt, dynE, stream);
    if (path != kSelSmall && out.stats) hipLaunchKernelGGL(write_stats, one, dim3(1), 0, stream, scal, ds.st, out.stats);
    if (cover) {
        if (path == kSelAll && !cover->batched) launch_cover_rows(*cover, nullptr, E, nullptr, mcnt, dynE, stream);
        hipLaunchKernelGGL(cover_finish, one, blk, 0, stream, mcnt, path == kSelAll ? int64_t(0) : int64_t(kCoverGrid), cover->grid, q,
                           out.stats, cover->info);
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}

// ---------------------------------------------------------------- the exponential race's draws
struct RaceArgs {
    int mode;
    const float *p, *prior, *noise;
    uint64_t seed, stream_id0;      // draw d: noise row d, or stream stream_id0 + d
    float one_minus_c, c;           // python: (1 - c) and c are doubles, cast to fp32 when they meet the fp32 tensor
    float* keys_out;                // single draws only
};
static RaceArgs race_args(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise, uint64_t seed,
                          uint64_t stream_id0, float* keys_out) {
    return RaceArgs{mode, p, prior, noise, seed, stream_id0, static_cast<float>(1.0 - degree_bias_coef), static_cast<float>(degree_bias_coef),
                    keys_out};
}

// select_chain's key pass for the race.  The normaliser (Z, or max and sum of exp) does not depend on the noise: one reduction for all
// draws.  A batched pass differs from a single draw on the small path alone: its key kernel, and the zeroing of the histograms that
// small_reduce_first clears for one draw only.
static int race_key_pass(SelPath path, const DrawSet& ds, const RaceArgs& a, const SamplerWs& w, int64_t E, bool multi, const int64_t* dynE,
                         hipStream_t stream) {
    const int64_t nblk = cdiv(E, kChunk);
    const unsigned nb = static_cast<unsigned>(nblk), Du = static_cast<unsigned>(ds.D);
    const dim3 blk(kThreads), grid(nb);
    const bool learned = a.mode == SGS_SAMPLE_LEARNED;
    const float* prior = learned ? a.prior : nullptr;
    if (path == kSelSmall) {
        if (multi)
            if (int rc = zero_async(ds.hist, static_cast<size_t>(3 * kBins) * ds.D * 4, stream)) return rc;
        const dim3 kgrid(nb, multi ? static_cast<unsigned>(cdiv(ds.D, kMultiG)) : 1u), kblk(kKeyThreads);
        const float *part_sum = learned ? w.part : w.part2, *part_max = learned ? nullptr : w.part;
        if (learned) {
            hipLaunchKernelGGL(small_reduce_first<0>, grid, blk, 0, stream, a.p, E, w.part, ds.hist, dynE);
        } else {
            hipLaunchKernelGGL(small_reduce_first<1>, grid, blk, 0, stream, a.p, E, w.part, ds.hist, dynE);
            hipLaunchKernelGGL(small_reduce_sumexp, grid, blk, 0, stream, a.p, E, w.part, nblk, w.part2, dynE);
        }
        if (multi && learned)
            hipLaunchKernelGGL(multi_keys_hist0<SGS_SAMPLE_LEARNED>, kgrid, kblk, 0, stream, a.p, prior, a.noise, a.seed, a.stream_id0, epoch_ptr(),
                               E, ds.D, a.one_minus_c, a.c, part_sum, part_max, nblk, w.scal, ds.keys, ds.ks, ds.hist);
        else if (multi)
            hipLaunchKernelGGL(multi_keys_hist0<SGS_SAMPLE_PRIOR>, kgrid, kblk, 0, stream, a.p, prior, a.noise, a.seed, a.stream_id0, epoch_ptr(),
                               E, ds.D, a.one_minus_c, a.c, part_sum, part_max, nblk, w.scal, ds.keys, ds.ks, ds.hist);
        else if (learned)
            hipLaunchKernelGGL(small_keys_hist0<SGS_SAMPLE_LEARNED>, kgrid, kblk, 0, stream, a.p, prior, a.noise, a.seed, a.stream_id0, epoch_ptr(),
                               E, a.one_minus_c, a.c, part_sum, part_max, nblk, w.scal, ds.keys, a.keys_out, ds.hist, dynE);
        else
            hipLaunchKernelGGL(small_keys_hist0<SGS_SAMPLE_PRIOR>, kgrid, kblk, 0, stream, a.p, prior, a.noise, a.seed, a.stream_id0, epoch_ptr(),
                               E, a.one_minus_c, a.c, part_sum, part_max, nblk, w.scal, ds.keys, a.keys_out, ds.hist, dynE);
        return SGS_OK;
    }
    // scal, st and the histograms are adjacent carvings: one zeroing launch (a kernel, not a memset node: see zero_async).  A single draw
    // clears the one histogram it uses; a batched pass all three per draw, as it always has
    if (int rc = zero_async(w.scal, static_cast<size_t>(reinterpret_cast<char*>(ds.hist + (multi ? 3 : 1) * kBins * ds.D) - reinterpret_cast<char*>(w.scal)), stream))
        return rc;
    if (learned) {
        hipLaunchKernelGGL(reduce_partial<0>, grid, blk, 0, stream, a.p, E, w.scal, w.part);
        hipLaunchKernelGGL(reduce_final<0>, dim3(1), blk, 0, stream, w.part, nblk, w.scal);
    } else {
        hipLaunchKernelGGL(reduce_partial<1>, grid, blk, 0, stream, a.p, E, w.scal, w.part);
        hipLaunchKernelGGL(reduce_final<1>, dim3(1), blk, 0, stream, w.part, nblk, w.scal);
        hipLaunchKernelGGL(reduce_partial<2>, grid, blk, 0, stream, a.p, E, w.scal, w.part);
        hipLaunchKernelGGL(reduce_final<2>, dim3(1), blk, 0, stream, w.part, nblk, w.scal);
    }
    if (path == kSelLarge) {
        const dim3 hgrid(nblk < kHistGrid ? nb : kHistGrid, Du);
        if (learned)
            hipLaunchKernelGGL(keys_hist0<SGS_SAMPLE_LEARNED>, hgrid, blk, 0, stream, a.p, prior, a.noise, a.seed, a.stream_id0, epoch_ptr(),
                               int64_t(0), E, a.one_minus_c, a.c, w.scal, ds, a.keys_out);
        else
            hipLaunchKernelGGL(keys_hist0<SGS_SAMPLE_PRIOR>, hgrid, blk, 0, stream, a.p, prior, a.noise, a.seed, a.stream_id0, epoch_ptr(),
                               int64_t(0), E, a.one_minus_c, a.c, w.scal, ds, a.keys_out);
    }
    return SGS_OK;
}

// sgs_sample_topq[_cover] (multi == false: D == 1) and sgs_sample_topq_multi[_cover]
static int sample_draws(const char* fn, bool multi, const CoverArgs* cover, const RaceArgs& a, int64_t D, int64_t E, int64_t q,
                        const int64_t* edge_index, const DrawOut& out, float* st_weights, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(a.mode == SGS_SAMPLE_LEARNED || a.mode == SGS_SAMPLE_PRIOR, SGS_EINVAL, "%s: bad mode %d", fn, a.mode);
    SGS_REQUIRE(D >= 1 && D <= 65535, SGS_EINVAL, "%s: D=%lld draws (need 1 <= D <= 65535)", fn, (long long)D);
    SGS_REQUIRE(E >= 0 && q >= 0, SGS_EINVAL, "%s: negative size (E=%lld q=%lld)", fn, (long long)E, (long long)q);
    SGS_REQUIRE(q <= E, SGS_EINVAL, "%s: cannot sample q=%lld > E=%lld edges without replacement", fn, (long long)q, (long long)E);
    SGS_REQUIRE(E < (int64_t(1) << 32), SGS_EINVAL, "%s: E=%lld exceeds 2^32-1", fn, (long long)E);
    if (cover) {
        SGS_REQUIRE(cover->N >= 0, SGS_EINVAL, "%s: negative node count (N=%lld)", fn, (long long)cover->N);
        SGS_REQUIRE(E == 0 || (cover->in_ptr && cover->in_src && cover->in_eid), SGS_EINVAL,
                    "%s: null destination CSR (in_ptr / in_src / in_eid) with E=%lld", fn, (long long)E);
        SGS_REQUIRE(E < (int64_t(1) << 31) && cover->N < (int64_t(1) << 31), SGS_EINVAL,
                    "%s: E=%lld, N=%lld exceed the int32 CSR", fn, (long long)E, (long long)cover->N);
    }
    if (E == 0) return SGS_OK;
    SGS_REQUIRE(out.mask, SGS_EINVAL, "%s: null mask", fn);
    SGS_REQUIRE(a.p || (a.mode == SGS_SAMPLE_LEARNED && !a.prior), SGS_EINVAL, "%s: p == NULL (uniform weights) needs mode LEARNED and no prior", fn);
    SGS_REQUIRE(!out.sei || edge_index, SGS_EINVAL, "%s: edge_index required for sampled_edge_index", fn);
    SGS_REQUIRE(!st_weights || (a.p && out.eid && out.stats && a.mode == SGS_SAMPLE_LEARNED), SGS_EINVAL,
                "%s: st_weights needs p, sampled_eid, stats and mode LEARNED", fn);
    const int64_t* dynE = dyn_edges_ptr();
    SGS_REQUIRE(!multi || !dynE, SGS_EINVAL, "%s: not available under a dynamic edge count (sgs_dyn_edges_set)", fn);
    if (int rc = check_ws(fn, ws, ws_bytes, sampler_ws(nullptr, E, D, cover != nullptr, false).bytes)) return rc;
    SGS_REQUIRE(!dynE || (cdiv(E, kChunk) <= kSmallBlocks && q > 0 && q < E), SGS_EINVAL,
                "%s: a dynamic edge count (sgs_dyn_edges_set) needs 0 < q < capacity <= %lld", fn, (long long)kSmallBlocks * kChunk);

    const SamplerWs w = sampler_ws(ws, E, D, cover != nullptr, false);
    if (int rc = select_chain(w, D, E, q, a.p, edge_index, out, cover, dynE, stream,
                              [&](SelPath path, const DrawSet& ds) { return race_key_pass(path, ds, a, w, E, multi, dynE, stream); }))
        return rc;
    if (st_weights && q > 0) {   // (after cover_finish: the straight-through weights read the threshold the single call reports, flag bit off)
        const dim3 g(static_cast<unsigned>(cdiv(q, 256)), static_cast<unsigned>(D));
        if (a.prior)
            hipLaunchKernelGGL(st_fwd<true>, g, dim3(256), 0, stream, a.p, a.prior, a.one_minus_c, a.c, out.stats, out.eid, q, st_weights);
        else
            hipLaunchKernelGGL(st_fwd<false>, g, dim3(256), 0, stream, a.p, a.prior, a.one_minus_c, a.c, out.stats, out.eid, q, st_weights);
        SGS_LAUNCH_OK();
    }
    return SGS_OK;
}

extern "C" {

size_t sgs_sample_topq_workspace_bytes(int64_t E) { return sampler_ws(nullptr, E, 1, false, false).bytes; }
// (N: the forced-edge kernel's per-workgroup counts have a fixed length, its grid is capped at kCoverGrid)
size_t sgs_sample_topq_cover_workspace_bytes(int64_t E, int64_t N) { (void)N; return sampler_ws(nullptr, E, 1, true, false).bytes; }
size_t sgs_sample_topq_multi_workspace_bytes(int64_t E, int64_t D) { return sampler_ws(nullptr, E, D, false, false).bytes; }
size_t sgs_sample_topq_multi_cover_workspace_bytes(int64_t E, int64_t N, int64_t D) { (void)N; return sampler_ws(nullptr, E, D, true, false).bytes; }
size_t sgs_consensus_select_workspace_bytes(int64_t E) { return sampler_ws(nullptr, E, 1, false, true).bytes; }

int sgs_sample_topq_cover_variant(int64_t N, int64_t E) {
    if (N <= 0 || E < 8 * N) return 4;
    return E < 64 * N ? 16 : 64;
}

int sgs_sample_topq_multi_cover_group_set(int G) {
    SGS_REQUIRE(G == 0 || G == 1 || G == 2 || G == 4, SGS_EINVAL, "sgs_sample_topq_multi_cover_group_set: G=%d (need 1, 2 or 4, or 0 for the default)", G);
    g_multi_cover_group = G ? G : kMultiCoverG;
    return SGS_OK;
}

int sgs_sample_topq(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise,
                    uint64_t seed, uint64_t stream_id, int64_t E, int64_t q, const int64_t* edge_index,
                    uint8_t* mask, int64_t* sampled_eid, int64_t* sampled_edge_index, float* sampled_p, float* stats,
                    float* keys_out, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    return sample_draws("sgs_sample_topq", false, nullptr, race_args(mode, p, prior, degree_bias_coef, noise, seed, stream_id, keys_out), 1, E, q,
                        edge_index, DrawOut{mask, sampled_eid, sampled_edge_index, sampled_p, stats}, nullptr, ws, ws_bytes, stream_);
}

int sgs_sample_topq_cover(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise,
                          uint64_t seed, uint64_t stream_id, int64_t E, int64_t q, const int64_t* edge_index,
                          int64_t N, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                          uint8_t* mask, int64_t* sampled_eid, int64_t* sampled_edge_index, float* sampled_p,
                          float* stats, float* keys_out, int32_t* cover_info, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    const CoverArgs c = cover_args(N, E, in_ptr, in_src, in_eid, cover_info, 1, false);
    return sample_draws("sgs_sample_topq_cover", false, &c, race_args(mode, p, prior, degree_bias_coef, noise, seed, stream_id, keys_out), 1, E, q,
                        edge_index, DrawOut{mask, sampled_eid, sampled_edge_index, sampled_p, stats}, nullptr, ws, ws_bytes, stream_);
}

int sgs_sample_topq_multi(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise, uint64_t seed,
                          uint64_t stream_id0, int64_t D, int64_t E, int64_t q, const int64_t* edge_index, uint8_t* mask, int64_t* sampled_eid,
                          int64_t* sampled_edge_index, float* stats, float* st_weights, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    return sample_draws("sgs_sample_topq_multi", true, nullptr, race_args(mode, p, prior, degree_bias_coef, noise, seed, stream_id0, nullptr), D, E,
                        q, edge_index, DrawOut{mask, sampled_eid, sampled_edge_index, nullptr, stats}, st_weights, ws, ws_bytes, stream_);
}

int sgs_sample_topq_multi_cover(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise, uint64_t seed,
                                uint64_t stream_id0, int64_t D, int64_t E, int64_t q, const int64_t* edge_index, int64_t N,
                                const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, uint8_t* mask, int64_t* sampled_eid,
                                int64_t* sampled_edge_index, float* stats, float* st_weights, int32_t* cover_info, void* ws, size_t ws_bytes,
                                sgs_stream_t stream_) {
    const CoverArgs c = cover_args(N, E, in_ptr, in_src, in_eid, cover_info, g_multi_cover_group, true);
    return sample_draws("sgs_sample_topq_multi_cover", true, &c, race_args(mode, p, prior, degree_bias_coef, noise, seed, stream_id0, nullptr), D,
                        E, q, edge_index, DrawOut{mask, sampled_eid, sampled_edge_index, nullptr, stats}, st_weights, ws, ws_bytes, stream_);
}

/* ---------------------------------------------------------------- consensus of D draws (the sparsifier export)
 * sgs_consensus_accum folds a pass's masks into per-edge keep counts; sgs_consensus_select builds one uint32 key per edge from
 * (count, score) and hands it to the sampler's own select / count / compact chain (small- and large-E path). */
int sgs_consensus_accum(const uint8_t* mask, int64_t mask_stride, int64_t Dc, int64_t E, int first, int32_t* count, int64_t* hist,
                        sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(Dc >= 0 && E >= 0, SGS_EINVAL, "sgs_consensus_accum: negative size (Dc=%lld E=%lld)", (long long)Dc, (long long)E);
    SGS_REQUIRE(Dc <= kCountMax, SGS_EINVAL, "sgs_consensus_accum: Dc=%lld draws in a pass, at most %d (a count is kept below %d)",
                (long long)Dc, kCountMax, kCountBins);
    SGS_REQUIRE(E < (int64_t(1) << 32), SGS_EINVAL, "sgs_consensus_accum: E=%lld exceeds 2^32-1", (long long)E);
    SGS_REQUIRE(Dc <= 1 || mask_stride >= E, SGS_EINVAL, "sgs_consensus_accum: mask_stride=%lld below E=%lld", (long long)mask_stride, (long long)E);
    if (E == 0) return SGS_OK;
    SGS_REQUIRE(count && (Dc == 0 || mask), SGS_EINVAL, "sgs_consensus_accum: null pointer");
    if (Dc == 0 && !first && !hist) return SGS_OK;
    hipLaunchKernelGGL(consensus_accum_kernel, dim3(static_cast<unsigned>(cdiv(E, kAccChunk))), dim3(kThreads), 0, stream, mask, mask_stride,
                       static_cast<int>(Dc), E, first, count, reinterpret_cast<unsigned long long*>(hist));
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_consensus_select(const int32_t* count, const float* p, int64_t E, int64_t q, const int64_t* edge_index, uint8_t* mask, int64_t* eid,
                         int64_t* edge_index_out, int32_t* count_out, float* p_out, uint32_t* keys_out, void* ws, size_t ws_bytes,
                         sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const char* fn = "sgs_consensus_select";
    SGS_REQUIRE(E >= 0 && q >= 0, SGS_EINVAL, "%s: negative size (E=%lld q=%lld)", fn, (long long)E, (long long)q);
    SGS_REQUIRE(q <= E, SGS_EINVAL, "%s: cannot select q=%lld > E=%lld edges without replacement", fn, (long long)q, (long long)E);
    SGS_REQUIRE(E < (int64_t(1) << 32), SGS_EINVAL, "%s: E=%lld exceeds 2^32-1", fn, (long long)E);
    if (E == 0) return SGS_OK;
    SGS_REQUIRE(count && mask, SGS_EINVAL, "%s: null count or mask", fn);
    SGS_REQUIRE(!edge_index_out || edge_index, SGS_EINVAL, "%s: edge_index required for edge_index_out", fn);
    if (int rc = check_ws(fn, ws, ws_bytes, sgs_consensus_select_workspace_bytes(E))) return rc;

    const SamplerWs w = sampler_ws(ws, E, 1, false, true);
    if (count_out && !eid) eid = w.eid;
    // the key pass with the histograms it needs cleared first; nothing / everything needs the keys only for keys_out.  No dynamic edge
    // count: the consensus is not a captured path, sizes are taken as given.
    auto key_pass = [&](SelPath path, const DrawSet& ds) -> int {
        if (path == kSelAll && !keys_out) return SGS_OK;
        const int64_t nblk = cdiv(E, kChunk);
        const unsigned nb = static_cast<unsigned>(nblk);
        int rc;
        if (path == kSelLarge) rc = zero_async(w.scal, static_cast<size_t>(reinterpret_cast<char*>(ds.hist + kBins) - reinterpret_cast<char*>(w.scal)), stream);
        else rc = zero_async(ds.hist, (path == kSelSmall ? 3 : 1) * kBins * sizeof(uint32_t), stream);
        if (rc) return rc;
        hipLaunchKernelGGL(consensus_keys_hist0, dim3(nblk < kHistGrid ? nb : kHistGrid), dim3(kThreads), 0, stream, count, p,
                           E, ds.keys, keys_out, ds.hist);
        return SGS_OK;
    };
    if (int rc = select_chain(w, 1, E, q, p, edge_index, DrawOut{mask, eid, edge_index_out, p_out, nullptr}, nullptr, nullptr, stream, key_pass))
        return rc;
    if (count_out && q > 0)
        hipLaunchKernelGGL(consensus_gather_count, dim3(cdiv(q, 256)), dim3(256), 0, stream, count, eid, q, E, count_out);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

/* ---------------------------------------------------------------- phase API (edge-sharded draws)
 * The same kernels as sgs_sample_topq, exposed per phase so that R ranks holding contiguous,
 * 2048-aligned shards of the edge list can run ONE exact global draw: per-chunk partial sums are
 * all-gathered and reduced in the single-GPU order (bit-identical Z), digit histograms are
 * all-reduced (integers), every rank runs the same digit selection, ties at the threshold go to the
 * lowest GLOBAL edge ids, and compaction is local.  Noise is keyed by the global edge id. */
size_t sgs_sampler_shard_workspace_bytes(int64_t E_local) {
    if (E_local < 0) E_local = 0;
    return carve_bytes(E_local, 4) + carve_bytes(cdiv(E_local, kChunk) + 1, sizeof(uint2)) + 256;
}
int64_t sgs_sampler_chunk(void) { return kChunk; }
// a phase's one draw over the caller's own buffers (those a phase does not touch are null)
static DrawSet shard_draw(const uint32_t* keys, uint32_t* hist, const void* state, uint2* cnt) {
    return DrawSet{const_cast<uint32_t*>(keys), 0, hist, 0, static_cast<SelectState*>(const_cast<void*>(state)), nullptr, cnt, 0, 1};
}

int sgs_sampler_shard_partials(int stage, const float* p, int64_t E, const float* scal, float* part, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(stage >= 0 && stage <= 2 && E >= 0, SGS_EINVAL, "sgs_sampler_shard_partials: bad arguments");
    if (E == 0) return SGS_OK;
    SGS_REQUIRE(p && part && (stage != 2 || scal), SGS_EINVAL, "sgs_sampler_shard_partials: null pointer");
    const dim3 grid(static_cast<unsigned>(cdiv(E, kChunk))), blk(kThreads);
    if (stage == 0) hipLaunchKernelGGL(reduce_partial<0>, grid, blk, 0, stream, p, E, scal, part);
    else if (stage == 1) hipLaunchKernelGGL(reduce_partial<1>, grid, blk, 0, stream, p, E, scal, part);
    else hipLaunchKernelGGL(reduce_partial<2>, grid, blk, 0, stream, p, E, scal, part);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_sampler_shard_finalize(int stage, const float* part_all, int64_t nblk_all, float* scal, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(stage >= 0 && stage <= 2 && nblk_all >= 0 && scal && (nblk_all == 0 || part_all), SGS_EINVAL,
                "sgs_sampler_shard_finalize: bad arguments");
    if (stage == 1) hipLaunchKernelGGL(reduce_final<1>, dim3(1), dim3(kThreads), 0, stream, part_all, nblk_all, scal);
    else hipLaunchKernelGGL(reduce_final<0>, dim3(1), dim3(kThreads), 0, stream, part_all, nblk_all, scal);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_sampler_shard_keys(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise,
                           uint64_t seed, uint64_t stream_id, int64_t edge_offset, int64_t E, const float* scal, uint32_t* keys,
                           float* keys_out, uint32_t* hist, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE((mode == SGS_SAMPLE_LEARNED || mode == SGS_SAMPLE_PRIOR) && E >= 0 && edge_offset >= 0, SGS_EINVAL,
                "sgs_sampler_shard_keys: bad arguments");
    if (E == 0) return SGS_OK;
    SGS_REQUIRE(p && scal && keys && hist, SGS_EINVAL, "sgs_sampler_shard_keys: null pointer");
    const float one_minus_c = static_cast<float>(1.0 - degree_bias_coef), c = static_cast<float>(degree_bias_coef);
    const int64_t nb_ = cdiv(E, kChunk);
    const dim3 hgrid(static_cast<unsigned>(nb_ < kHistGrid ? nb_ : kHistGrid)), blk(kThreads);
    if (mode == SGS_SAMPLE_LEARNED)
        hipLaunchKernelGGL(keys_hist0<SGS_SAMPLE_LEARNED>, hgrid, blk, 0, stream, p, prior, noise, seed, stream_id, epoch_ptr(), edge_offset, E,
                           one_minus_c, c, scal, shard_draw(keys, hist, nullptr, nullptr), keys_out);
    else
        hipLaunchKernelGGL(keys_hist0<SGS_SAMPLE_PRIOR>, hgrid, blk, 0, stream, p, nullptr, noise, seed, stream_id, epoch_ptr(), edge_offset, E,
                           one_minus_c, c, scal, shard_draw(keys, hist, nullptr, nullptr), keys_out);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_sampler_shard_hist(const uint32_t* keys, int64_t E, int pass, const void* state, uint32_t* hist, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE((pass == 1 || pass == 2) && E >= 0 && state && hist, SGS_EINVAL, "sgs_sampler_shard_hist: bad arguments");
    if (E == 0) return SGS_OK;
    const int64_t nb_ = cdiv(E, kChunk);
    const dim3 hgrid(static_cast<unsigned>(nb_ < kHistGrid ? nb_ : kHistGrid)), blk(kThreads);
    const DrawSet ds = shard_draw(keys, hist, state, nullptr);
    if (pass == 1) hipLaunchKernelGGL(hist_next, hgrid, blk, 0, stream, ds, E, kShift1, kMask1, kShift0);
    else hipLaunchKernelGGL(hist_next, hgrid, blk, 0, stream, ds, E, kShift2, kMask2, kShift1);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_sampler_select(uint32_t* hist, int pass, int64_t q, void* state, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(pass >= 0 && pass <= 2 && q > 0 && hist && state, SGS_EINVAL, "sgs_sampler_select: bad arguments");
    const int shift = pass == 0 ? kShift0 : pass == 1 ? kShift1 : kShift2;
    hipLaunchKernelGGL(select_digit, dim3(1), dim3(kThreads), 0, stream, shard_draw(nullptr, hist, state, nullptr), shift, pass == 0 ? 1 : 0,
                       static_cast<uint32_t>(q));
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_sampler_shard_count(const uint32_t* keys, int64_t E, const void* state, uint32_t* counts, void* ws, size_t ws_bytes,
                            sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(E >= 0 && state && counts, SGS_EINVAL, "sgs_sampler_shard_count: bad arguments");
    SGS_REQUIRE(ws && ws_bytes >= sgs_sampler_shard_workspace_bytes(E), SGS_EWORKSPACE, "sgs_sampler_shard_count: workspace too small");
    Carver cv(ws);
    cv.take<uint32_t>(E);                                  // keys live in the caller's copy of this region
    uint2* cnt = cv.take<uint2>(cdiv(E, kChunk) + 1);
    const int64_t nblk = cdiv(E, kChunk);
    const DrawSet ds = shard_draw(keys, nullptr, state, cnt);
    if (nblk > 0) hipLaunchKernelGGL(count_blocks, dim3(nblk), dim3(kThreads), 0, stream, ds, E);
    hipLaunchKernelGGL(total_counts, dim3(1), dim3(kThreads), 0, stream, cnt, nblk, counts);
    if (nblk > 0) hipLaunchKernelGGL(scan_blocks, dim3(1), dim3(kThreads), 0, stream, ds, nblk);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_sampler_shard_compact(const uint32_t* keys, int64_t E, const void* state, int64_t ties_local, int64_t q_local,
                              int64_t edge_offset, const float* p, const int64_t* edge_index_local, uint8_t* mask,
                              int64_t* sampled_eid, int64_t* sampled_edge_index, float* sampled_p, void* ws, size_t ws_bytes,
                              sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(E >= 0 && ties_local >= 0 && q_local >= 0 && state, SGS_EINVAL, "sgs_sampler_shard_compact: bad arguments");
    if (E == 0) return SGS_OK;
    SGS_REQUIRE(keys && mask && p, SGS_EINVAL, "sgs_sampler_shard_compact: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_sampler_shard_workspace_bytes(E), SGS_EWORKSPACE, "sgs_sampler_shard_compact: workspace too small");
    Carver cv(ws);
    cv.take<uint32_t>(E);
    uint2* cnt = cv.take<uint2>(cdiv(E, kChunk) + 1);      // scanned by sgs_sampler_shard_count
    hipLaunchKernelGGL(compact, dim3(cdiv(E, kChunk)), dim3(kThreads), 0, stream, shard_draw(keys, nullptr, state, cnt), E, q_local, ties_local,
                       edge_offset, p, edge_index_local, DrawOut{mask, sampled_eid, sampled_edge_index, sampled_p, nullptr});
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gather_columns(const int64_t* edge_index, int64_t E, const int64_t* idx, int64_t q, int64_t* out, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(E >= 0 && q >= 0, SGS_EINVAL, "sgs_gather_columns: bad sizes");
    if (q == 0) return SGS_OK;
    SGS_REQUIRE(edge_index && idx && out, SGS_EINVAL, "sgs_gather_columns: null pointer");
    hipLaunchKernelGGL(gather_columns_kernel, dim3(cdiv(q, 256)), dim3(256), 0, stream, edge_index, E, idx, q, out);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_st_weights_fwd(const float* p, const float* prior, double degree_bias_coef, const float* stats,
                       const int64_t* sampled_eid, int64_t E, int64_t q, float* w, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(E >= 0 && q >= 0 && q <= E, SGS_EINVAL, "sgs_st_weights_fwd: bad sizes");
    if (q == 0) return SGS_OK;
    SGS_REQUIRE(p && stats && sampled_eid && w, SGS_EINVAL, "sgs_st_weights_fwd: null pointer");
    const float one_minus_c = static_cast<float>(1.0 - degree_bias_coef), c = static_cast<float>(degree_bias_coef);
    if (prior)
        hipLaunchKernelGGL(st_fwd<true>, dim3(cdiv(q, 256)), dim3(256), 0, stream, p, prior, one_minus_c, c, stats,
                           sampled_eid, q, w);
    else
        hipLaunchKernelGGL(st_fwd<false>, dim3(cdiv(q, 256)), dim3(256), 0, stream, p, prior, one_minus_c, c, stats,
                           sampled_eid, q, w);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_st_weights_bwd_workspace_bytes(int64_t E, int64_t q) {
    (void)E;
    if (q < 0) q = 0;
    return carve_bytes(cdiv(q, kChunk) + 1, 4) + carve_bytes(4, 4) + 256;
}

int sgs_st_weights_bwd(const float* p, const float* prior, double degree_bias_coef, const float* stats,
                       const int64_t* sampled_eid, const float* grad_w, int64_t E, int64_t q, float* grad_p, void* ws,
                       size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(E >= 0 && q >= 0 && q <= E, SGS_EINVAL, "sgs_st_weights_bwd: bad sizes");
    if (E == 0) return SGS_OK;
    SGS_REQUIRE(p && stats && grad_p && (q == 0 || (sampled_eid && grad_w)), SGS_EINVAL, "sgs_st_weights_bwd: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_st_weights_bwd_workspace_bytes(E, q), SGS_EWORKSPACE,
                "sgs_st_weights_bwd: workspace too small");
    Carver cv(ws);
    const int64_t nblk = cdiv(q, kChunk);
    float* part = cv.take<float>(nblk + 1);
    float* S = cv.take<float>(4);
    const float one_minus_c = static_cast<float>(1.0 - degree_bias_coef), c = static_cast<float>(degree_bias_coef);
    const float a = prior ? one_minus_c : 1.0f;
    if (int rc = zero_async(S, 16, stream)) return rc;
    if (q > 0) {
        if (prior)
            hipLaunchKernelGGL(st_bwd_partial<true>, dim3(nblk), dim3(kThreads), 0, stream, p, prior, one_minus_c, c, stats,
                               sampled_eid, grad_w, q, part);
        else
            hipLaunchKernelGGL(st_bwd_partial<false>, dim3(nblk), dim3(kThreads), 0, stream, p, prior, one_minus_c, c, stats,
                               sampled_eid, grad_w, q, part);
        hipLaunchKernelGGL(st_bwd_final, dim3(1), dim3(kThreads), 0, stream, part, nblk, S);
    }
    hipLaunchKernelGGL(st_bwd_dense, dim3(cdiv(E, 256)), dim3(256), 0, stream, S, stats, a, E, grad_p, dyn_edges_ptr());
    if (q > 0) {
        if (prior)
            hipLaunchKernelGGL(st_bwd_sparse<true>, dim3(cdiv(q, 256)), dim3(256), 0, stream, p, prior, one_minus_c, c, a,
                               stats, sampled_eid, grad_w, q, grad_p);
        else
            hipLaunchKernelGGL(st_bwd_sparse<false>, dim3(cdiv(q, 256)), dim3(256), 0, stream, p, prior, one_minus_c, c, a,
                               stats, sampled_eid, grad_w, q, grad_p);
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}

}  // extern "C"
