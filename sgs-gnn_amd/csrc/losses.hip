// K6: gate and losses of the hybrid / straight-through / two-pass step (gfx950).
//
// Reference: training_hybrid.py:92-133 and utils.py:163-169 (`calculate_f1`), 187-211
// (`consistency_loss`).  The reference copies logits to the host for sklearn's micro-F1, runs
// two sort-based torch.isin calls and one .item() sync for reg1; here everything stays on the
// device and every reduction uses a fixed tree (deterministic).
#include <algorithm>
#include <atomic>

#include "sgs_common.h"
#include "endpoint_reduce.h"

namespace sgs {
namespace {

constexpr int kT = 256;

// ---------------------------------------------------------------- gate: #correct argmax on train rows
// One lane's share of a row scan: columns lane, lane + 64, ... in increasing order, so a later equal value never replaces an earlier one.
// The lane's first column is taken unconditionally, outside the loop: with the "no column yet" sentinel tested inside the loop
// (`v > best || (v == best && c < bi) || bi == sentinel`) the compiled loop updated `best` but left `bi` at the sentinel whenever
// `v > best` was false, so a row of -inf (nothing exceeds the initial -inf) had no argmax at all and never counted as correct; torch.argmax
// gives 0 there (tests/test_gpu_loss_chain.py::test_gate_counts_exact plants such rows).
__device__ __forceinline__ void lane_argmax(const float* __restrict__ row, int64_t C, int lane, float& best, int& bi) {
    if (lane >= C) return;
    best = row[lane];
    bi = lane;
    for (int64_t c = lane + 64; c < C; c += 64) {
        const float v = row[c];
        if (v > best) { best = v; bi = static_cast<int>(c); }
    }
}

// One wave per row; torch.argmax semantics (first maximum wins).
__global__ void __launch_bounds__(kT) masked_correct(const float* __restrict__ logits, int64_t N, int64_t C,
                                                    const int64_t* __restrict__ y, const uint8_t* __restrict__ mask,
                                                    int* __restrict__ correct) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N || !mask[i]) return;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    lane_argmax(logits + i * C, C, lane, best, bi);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
    }
    if (lane == 0) {
        atomicAdd(&correct[1], 1);
        if (static_cast<int64_t>(bi) == y[i]) atomicAdd(&correct[0], 1);
    }
}

// The gate's two counts in one launch: waves [0, N) score logits_a into correct[0:2], waves [N, 2N) logits_b into
// correct[2:4].  `correct` must be zero on entry (the caller's allocation clears it: one fill for both).
__global__ void __launch_bounds__(1024) masked_correct_pair(const float* __restrict__ logits_a, const float* __restrict__ logits_b, int64_t N,
                                                           int64_t C, const int64_t* __restrict__ y, const uint8_t* __restrict__ mask,
                                                           int* __restrict__ correct) {
    // 16 waves = 16 rows of ONE of the two logit matrices per workgroup (blockIdx.y selects it): the counts are reduced in LDS
    // and each workgroup issues two atomics instead of every row issuing two
    __shared__ int red[2 * 16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 16 + wid;
    const float* __restrict__ logits = blockIdx.y ? logits_b : logits_a;
    int ok = 0, row = 0;
    if (i < N && mask[i]) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        lane_argmax(logits + i * C, C, lane, best, bi);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
        }
        row = 1;
        ok = (static_cast<int64_t>(bi) == y[i]) ? 1 : 0;
    }
    if (lane == 0) { red[2 * wid] = ok; red[2 * wid + 1] = row; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a_ = 0, b_ = 0;
        for (int w = 0; w < 16; ++w) { a_ += red[2 * w]; b_ += red[2 * w + 1]; }
        int* out = correct + (blockIdx.y ? 2 : 0);
        if (b_) atomicAdd(&out[1], b_);
        if (a_) atomicAdd(&out[0], a_);
    }
}

// The gate in two launches with no zero fill and no atomics: gate_counts_partial = masked_correct_pair's row scan, but every workgroup
// writes its own (#correct, #rows) pair; gate_counts_finish (one wave) adds them in order, writes out[0..3] = (#correct_a, #train,
// #correct_b, #train), out[4] = 0 and -- with `dst` -- hands the four counts to the polling host exactly as publish_words does.
__global__ void __launch_bounds__(1024) gate_counts_partial(const float* __restrict__ logits_a, const float* __restrict__ logits_b, int64_t N,
                                                           int64_t C, const int64_t* __restrict__ y, const uint8_t* __restrict__ mask,
                                                           int2* __restrict__ part) {
    __shared__ int red[2 * 16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 16 + wid;
    const float* __restrict__ logits = blockIdx.y ? logits_b : logits_a;
    int ok = 0, row = 0;
    if (i < N && mask[i]) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        lane_argmax(logits + i * C, C, lane, best, bi);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
        }
        row = 1;
        ok = (static_cast<int64_t>(bi) == y[i]) ? 1 : 0;
    }
    if (lane == 0) { red[2 * wid] = ok; red[2 * wid + 1] = row; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a_ = 0, b_ = 0;
        for (int w = 0; w < 16; ++w) { a_ += red[2 * w]; b_ += red[2 * w + 1]; }
        part[static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x] = make_int2(a_, b_);
    }
}
__global__ void __launch_bounds__(64) gate_counts_finish(const int2* __restrict__ part, int nblk, int* __restrict__ out,
                                                        const uint64_t* __restrict__ seq, int32_t* __restrict__ dst) {
    int a0 = 0, r0 = 0, a1 = 0, r1 = 0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
        const int2 pa = part[b], pb = part[nblk + b];
        a0 += pa.x; r0 += pa.y; a1 += pb.x; r1 += pb.y;
    }
    a0 = wave_sum_int_all(a0); r0 = wave_sum_int_all(r0); a1 = wave_sum_int_all(a1); r1 = wave_sum_int_all(r1);
    if (threadIdx.x == 0) {
        out[0] = a0; out[1] = r0; out[2] = a1; out[3] = r1; out[4] = 0;
        if (dst) {
            __hip_atomic_store(dst + 0, a0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(dst + 1, r0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(dst + 2, a1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(dst + 3, r1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __atomic_thread_fence(__ATOMIC_RELEASE);
            __hip_atomic_store(dst + 4, static_cast<int32_t>(seq ? seq[0] : 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// End of a replayed step in one launch: running loss += this step's loss, RNG epoch += 1 (the next replay draws fresh noise).
__global__ void loss_tick(float* __restrict__ sum, const float* __restrict__ loss, uint64_t* __restrict__ epoch) {
    if (threadIdx.x == 0) {
        if (sum && loss) sum[0] += loss[0];
        if (epoch) epoch[0] += 1;
    }
}

// Hands a few device words to the HOST without a copy engine round trip: `dst` is pinned, device-mapped host memory; the
// payload is written first, then the sequence word (the RNG epoch, which changes on every graph replay) with release
// semantics at system scope, so a host thread that polls the sequence word sees the payload.  Used for the gate.
__global__ void publish_words(const int32_t* __restrict__ src, int n, const uint64_t* __restrict__ seq, int32_t* dst) {
    if (threadIdx.x < n) __hip_atomic_store(dst + threadIdx.x, src[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    if (threadIdx.x == 0) {
        __atomic_thread_fence(__ATOMIC_RELEASE);
        __hip_atomic_store(dst + n, static_cast<int32_t>(seq ? seq[0] : 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---------------------------------------------------------------- masked cross entropy, plain (kW = false) and class-weighted / label-smoothed (kW = true)
// F.cross_entropy(logits[mask], y[mask], weight = w, label_smoothing = eps, reduction = "mean"); w == nullptr: all ones.
//   row_i = (1 - eps) w[y_i] (lse_i - x_i[y_i]) + (eps / C) sum_c w_c (lse_i - x_ic)        on train rows, 0 elsewhere; row_lse kept for backward
//   den   = sum over train rows of w[y_i];   loss = sum_i row_i / den, nan when den == 0 (torch: the hard term's own 0 / 0)
//   dx_ic = g / den [ (1 - eps) w[y_i] (softmax_ic - [c == y_i]) + (eps / C) (W softmax_ic - w_c) ],  W = sum_c w_c;  nan on train rows when den == 0
// The plain criterion is w = 1, eps = 0 with the terms that vanish never formed: row_i = lse_i - x_i[y_i], den = #train rows (an int32
// word; 0 / 0 = nan, as torch's mean over an empty selection), dx_ic = g / #train (softmax_ic - [c == y_i]).
// The smoothing sum is taken as sum_c w_c (lse - x_c) -- one wave reduction more than the plain row -- and not as W lse - sum_c w_c x_c, which
// needs two and W.  eps == 0 skips it.  A label outside [0, C) on a train row is outside the contract; only the weighted criterion indexes
// by it (`class_weight`), and it reads nothing out of bounds there (weight 0, no label term).
//
// CeNorm<kW>: the divisor of the mean and what the weighted criterion alone reads.  A kernel takes it by value as its LAST argument: the
// plain one is empty, so the plain instantiations keep the plain kernels' argument layout.
template <bool kW>
struct CeNorm;
template <>
struct CeNorm<false> {
    using Word = int;                                   // the stored divisor: n_rows, the number of train rows
    static __host__ __device__ CeNorm make(const float*, float, const int64_t*, int64_t) { return CeNorm{}; }
    __device__ __forceinline__ int row(int64_t) const { return 1; }                          // what a train row adds to the divisor
    static __device__ __forceinline__ float mean(float sum, float n) { return sum / n; }     // 0/0 = nan, as torch's mean over an empty selection
    static __device__ __forceinline__ float scale(float gl, const int* n_rows) { return gl / static_cast<float>(n_rows[0]); }
};
template <>
struct CeNorm<true> {
    using Word = float;                                 // den, the sum of the train rows' class weights
    const float* __restrict__ weight;
    float eps;
    const int64_t* __restrict__ y;
    int64_t C;
    static __host__ __device__ CeNorm make(const float* weight, float eps, const int64_t* y, int64_t C) { return CeNorm{weight, eps, y, C}; }
    __device__ __forceinline__ float of_label(int64_t yi) const {
        if (yi < 0 || yi >= C) return 0.f;
        return weight ? weight[yi] : 1.f;
    }
    __device__ __forceinline__ float of_class(int64_t c) const { return weight ? weight[c] : 1.f; }
    __device__ __forceinline__ float row(int64_t i) const { return of_label(y[i]); }
    static __device__ __forceinline__ float mean(float sum, float den) { return (den == 0.f) ? NAN : sum / den; }
    static __device__ __forceinline__ float scale(float gl, const float* den) {
        const float d = den[0];
        return (d == 0.f) ? NAN : gl / d;
    }
};

// rowloss[i] and row_lse[i] of one wave's row (i, all 64 lanes); ce_rows and the merged forward launch (hybrid_fwd_pair) share it.
template <bool kW>
__device__ __forceinline__ void ce_row(int64_t i, int lane, const float* __restrict__ logits, int64_t N, int64_t C, const int64_t* __restrict__ y,
                                       const uint8_t* __restrict__ mask, const CeNorm<kW>& cn, float* __restrict__ row_lse,
                                       float* __restrict__ rowloss) {
    if (i >= N) return;
    if (!mask[i]) {
        if (lane == 0) { rowloss[i] = 0.f; row_lse[i] = 0.f; }
        return;
    }
    float mx = -INFINITY;
    for (int64_t c = lane; c < C; c += 64) mx = fmaxf(mx, logits[i * C + c]);
    mx = wave_max_all(mx);
    float s = 0.f;
    for (int64_t c = lane; c < C; c += 64) s += expf(logits[i * C + c] - mx);
    s = wave_sum_all(s);
    const float lse = mx + logf(s);
    if constexpr (!kW) {
        if (lane == 0) {
            row_lse[i] = lse;
            rowloss[i] = lse - logits[i * C + y[i]];
        }
    } else {
        const float eps = cn.eps;
        float sm = 0.f;
        if (eps != 0.f) {
            for (int64_t c = lane; c < C; c += 64) sm += cn.of_class(c) * (lse - logits[i * C + c]);
            sm = wave_sum_all(sm);
        }
        if (lane == 0) {
            const int64_t yi = y[i];
            const float hard = (yi >= 0 && yi < C) ? cn.of_label(yi) * (lse - logits[i * C + yi]) : 0.f;
            row_lse[i] = lse;
            rowloss[i] = (eps != 0.f) ? (1.f - eps) * hard + (eps / static_cast<float>(C)) * sm : hard;
        }
    }
}
template <bool kW>
__global__ void __launch_bounds__(kT) ce_rows(const float* __restrict__ logits, int64_t N, int64_t C, const int64_t* __restrict__ y,
                                             const uint8_t* __restrict__ mask, float* __restrict__ row_lse, float* __restrict__ rowloss,
                                             const CeNorm<kW> cn) {
    ce_row<kW>((static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6, threadIdx.x & 63, logits, N, C, y, mask, cn, row_lse, rowloss);
}

// One block of 1024: norm[0] = the divisor (recomputed from the mask, and from w and y when weighted: no [N] buffer), loss = sum(rowloss) / norm[0].
template <bool kW>
__global__ void __launch_bounds__(1024) ce_final(const float* __restrict__ rowloss, const uint8_t* __restrict__ mask, int64_t N,
                                                float* __restrict__ loss, typename CeNorm<kW>::Word* __restrict__ norm, const CeNorm<kW> cn) {
    __shared__ float red[16];
    float acc = 0.f;
    typename CeNorm<kW>::Word dn = 0;
    for (int64_t i = threadIdx.x; i < N; i += 1024) {
        acc += rowloss[i];
        dn += mask[i] ? cn.row(i) : 0;
    }
    const float r = block_sum(acc, red);
    if constexpr (kW) {
        dn = block_sum(dn, red);
    } else {                                            // the count stays an integer: no N < 2^24 limit on the plain entry
        __shared__ int redi[16];
        dn = wave_sum_int_all(dn);
        if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = dn;
        __syncthreads();
        dn = 0;
        if (threadIdx.x == 0)
            for (int w = 0; w < 16; ++w) dn += redi[w];
    }
    if (threadIdx.x == 0) {
        norm[0] = dn;
        loss[0] = CeNorm<kW>::mean(r, static_cast<float>(dn));
    }
}

// W = sum_c w_c in every thread of the block, in a fixed order (the same value in every block).  Every thread of the block must call it;
// the first kThreads (a multiple of 64) form the sum.
template <int kThreads>
__device__ __forceinline__ float block_weight_sum(const float* __restrict__ weight, int64_t C, float* red) {
    if (threadIdx.x < kThreads) {
        float v = 0.f;
        for (int64_t c = threadIdx.x; c < C; c += kThreads) v += weight[c];
        v = wave_sum_all(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    }
    __syncthreads();
    float r = 0.f;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) r += red[k];
    return r;
}

// One entry of the gradient above (a train row's), scaled by CeNorm<kW>::scale(grad_loss[0], norm); W = sum_c w_c (read when weighted and
// eps != 0).
template <bool kW>
__device__ __forceinline__ float ce_grad(const CeNorm<kW>& cn, float x, float lse, int64_t yi, int64_t c, int64_t C, float W,
                                         const float* __restrict__ grad_loss, const typename CeNorm<kW>::Word* __restrict__ norm) {
    if constexpr (!kW) {
        const float sm = expf(x - lse);
        return (sm - (yi == c ? 1.f : 0.f)) * CeNorm<kW>::scale(grad_loss[0], norm);
    } else {
        const float sc = CeNorm<kW>::scale(grad_loss[0], norm);
        const float sm = expf(x - lse);
        const float hard = cn.of_label(yi) * (sm - (yi == c ? 1.f : 0.f));
        if (cn.eps == 0.f) return hard * sc;
        return ((1.f - cn.eps) * hard + (cn.eps * (1.f / static_cast<float>(C))) * (W * sm - cn.of_class(c))) * sc;
    }
}

// dlogits = (kAcc: +=) the gradient above.  Off the train rows the plain writing form stores a computed 0, the weighted one stores 0 and
// leaves, the accumulating forms leave without touching memory.
template <bool kW, bool kAcc>
__global__ void __launch_bounds__(kT) ce_bwd(const float* __restrict__ logits, int64_t N, int64_t C, const int64_t* __restrict__ y,
                                            const uint8_t* __restrict__ mask, const float* __restrict__ row_lse,
                                            const typename CeNorm<kW>::Word* __restrict__ norm, const float* __restrict__ grad_loss,
                                            float* __restrict__ dlogits, const CeNorm<kW> cn) {
    float W = static_cast<float>(C);
    if constexpr (kW) {
        __shared__ float red[kT / 64];
        if (cn.eps != 0.f && cn.weight) W = block_weight_sum<kT>(cn.weight, C, red);        // (uniform branch: every thread of every block takes it or none)
    }
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (idx >= N * C) return;
    const int64_t i = idx / C, c = idx - i * C;
    float g = 0.f;
    if (mask[i]) {
        g = ce_grad<kW>(cn, logits[idx], row_lse[i], y[i], c, C, W, grad_loss, norm);
    } else if (kW || kAcc) {
        if (!kAcc) dlogits[idx] = 0.f;
        return;
    }
    if (kAcc) dlogits[idx] += g;
    else dlogits[idx] = g;
}

// ---------------------------------------------------------------- edge regularisers
struct EdgeTerms {
    float dot, nx, ny;   // <x,y>, |x|^2, |y|^2
};
__device__ __forceinline__ EdgeTerms edge_dot(const float* __restrict__ x, const float* __restrict__ y, int64_t C) {
    EdgeTerms t{0.f, 0.f, 0.f};
    for (int64_t c = 0; c < C; ++c) {
        const float a = x[c], b = y[c];
        t.dot = fmaf(a, b, t.dot); t.nx = fmaf(a, a, t.nx); t.ny = fmaf(b, b, t.ny);
    }
    return t;
}
// F.cosine_similarity(x, y, eps=1e-8) = <x,y> / sqrt(max(|x|^2 |y|^2, eps^2))
__device__ __forceinline__ float cos_from(const EdgeTerms& t) { return t.dot / sqrtf(fmaxf(t.nx * t.ny, 1e-16f)); }

// edges per workgroup of the forward pass: kRegRounds rounds of one edge per 16-lane group (16 rounds measured 28 us at q = 100 000
// against 19 for the thread-per-edge form: too few workgroups, each a serial chain; 4 rounds: 1 563 workgroups)
constexpr int kRegRounds = 4;
constexpr int kRegEdges = kRegRounds * (kT / 16);
// per block partials: [0]=sum bce, [1]=sum (w-cos)^2, [2]=#valid, [3]=sum labels
__global__ void __launch_bounds__(kT) reg_fwd_partial(const float* __restrict__ w, const int64_t* __restrict__ sei, int64_t q,
                                                     const float* __restrict__ logits, int64_t C, const int64_t* __restrict__ y,
                                                     const uint8_t* __restrict__ tm, float* __restrict__ cos_out,
                                                     float* __restrict__ part) {
    __shared__ float red[kT / 64];
    // 16 lanes per edge (a logits row is C = 41 floats: three 64-byte segments instead of 41 strided scalar loads by one thread), the
    // workgroup's kRegEdges edges in kRegRounds rounds of kT / 16; lane 0 of a group keeps the group's terms
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    float bce = 0.f, sq = 0.f, nv = 0.f, nl = 0.f;
#pragma unroll
    for (int r = 0; r < kRegRounds; ++r) {
        const int64_t j = static_cast<int64_t>(blockIdx.x) * kRegEdges + r * (kT / 16) + grp;
        const bool live = j < q;
        const int64_t jj = live ? j : 0;
        const int64_t s = sei[jj], d = sei[q + jj];
        const float* x = logits + s * C;
        const float* yv = logits + d * C;
        float dot = 0.f, nx = 0.f, ny = 0.f;
        for (int64_t c = sub; c < C; c += 16) {
            const float a = x[c], b = yv[c];
            dot = fmaf(a, b, dot); nx = fmaf(a, a, nx); ny = fmaf(b, b, ny);
        }
        dot = row16_sum_all_dpp(dot); nx = row16_sum_all_dpp(nx); ny = row16_sum_all_dpp(ny);
        if (live && sub == 0) {
            const float wj = w[j];
            const float cs = cos_from(EdgeTerms{dot, nx, ny});
            if (cos_out) cos_out[j] = cs;
            const float df = wj - cs;
            sq += df * df;
            if (tm[s] && tm[d]) {
                nv += 1.f;
                const bool same = y[s] == y[d];
                nl += same ? 1.f : 0.f;
                // F.binary_cross_entropy clamps each log at -100
                bce += same ? -fmaxf(logf(wj), -100.f) : -fmaxf(logf(1.f - wj), -100.f);
            }
        }
    }
    const float r0 = block_sum(bce, red);
    const float r1 = block_sum(sq, red);
    const float r2 = block_sum(nv, red);
    const float r3 = block_sum(nl, red);
    if (threadIdx.x == 0) {
        part[4 * blockIdx.x + 0] = r0; part[4 * blockIdx.x + 1] = r1;
        part[4 * blockIdx.x + 2] = r2; part[4 * blockIdx.x + 3] = r3;
    }
}

// The four column sums of the per-block partials part[4 b + k], for one finishing block of kT threads: `gather` is a thread's share
// (blocks threadIdx.x, threadIdx.x + kT, ...), `reduce` the block's four sums, taken in column order (valid in thread 0).
struct RegSums {
    float bce = 0.f, sq = 0.f, nv = 0.f, nl = 0.f;
    __device__ __forceinline__ void gather(const float* __restrict__ part, int64_t nblk) {
        for (int64_t b = threadIdx.x; b < nblk; b += kT) {
            bce += part[4 * b]; sq += part[4 * b + 1]; nv += part[4 * b + 2]; nl += part[4 * b + 3];
        }
    }
    __device__ __forceinline__ void reduce(float* red) {
        bce = block_sum(bce, red); sq = block_sum(sq, red); nv = block_sum(nv, red); nl = block_sum(nl, red);
    }
    // out[0] = reg1 (0 unless sum(labels) > 1), out[1] = reg2, out[2] = #valid, out[3] = sum labels, out[4] = coef1 * reg1 + coef2 * reg2
    __device__ __forceinline__ void store(int64_t q, float coef1, float coef2, float* __restrict__ out) const {
        const float reg1 = (nl > 1.f) ? bce / nv : 0.f;             // training_hybrid.py:125-128
        const float reg2 = sq / static_cast<float>(q);
        out[0] = reg1; out[1] = reg2; out[2] = nv; out[3] = nl;
        out[4] = coef1 * reg1 + coef2 * reg2;
    }
};

__global__ void __launch_bounds__(kT) reg_fwd_final(const float* __restrict__ part, int64_t nblk, int64_t q, float coef1, float coef2,
                                                   float* __restrict__ out) {
    __shared__ float red[kT / 64];
    RegSums s;
    s.gather(part, nblk);
    s.reduce(red);
    if (threadIdx.x == 0) s.store(q, coef1, coef2, out);
}

// The learned branch's whole loss in one finishing launch (training_hybrid.py:105-133): the cross entropy's mean over the train rows
// (as ce_final<kW>, in a block of kT) and the two regularisers (as reg_fwd_final: same partials, same order);  out[0..4] as reg_fwd_final,
// out[5] = cross entropy, out[6] = out[5] + out[4] = the loss, norm[0] = the cross entropy's divisor.
template <bool kW>
__global__ void __launch_bounds__(kT) hybrid_loss_final(const float* __restrict__ part, int64_t nblk, int64_t q, float coef1, float coef2,
                                                       const float* __restrict__ rowloss, const uint8_t* __restrict__ mask, int64_t N,
                                                       float* __restrict__ out, typename CeNorm<kW>::Word* __restrict__ norm,
                                                       const CeNorm<kW> cn) {
    __shared__ float red[kT / 64];
    RegSums s;
    float ce = 0.f, dn = 0.f;
    s.gather(part, nblk);
    for (int64_t i = threadIdx.x; i < N; i += kT) {
        ce += rowloss[i];
        dn += mask[i] ? static_cast<float>(cn.row(i)) : 0.f;        // (plain: counts < 2^24, exact in fp32)
    }
    s.reduce(red);
    const float rc = block_sum(ce, red), rn = block_sum(dn, red);
    if (threadIdx.x == 0) {
        s.store(q, coef1, coef2, out);
        out[5] = CeNorm<kW>::mean(rc, rn);
        out[6] = out[5] + out[4];
        norm[0] = static_cast<typename CeNorm<kW>::Word>(rn);
    }
}

// raw[0..3] = {sum bce, sum (w-cos)^2, #valid, sum labels} of this rank's edges (edge-sharded losses: the
// ranks all-reduce these four sums and finish the formulas with the global q).
__global__ void __launch_bounds__(kT) reg_raw_final(const float* __restrict__ part, int64_t nblk, float* __restrict__ raw) {
    __shared__ float red[kT / 64];
    RegSums s;
    s.gather(part, nblk);
    s.reduce(red);
    if (threadIdx.x == 0) { raw[0] = s.bce; raw[1] = s.sq; raw[2] = s.nv; raw[3] = s.nl; }
}

// What the backward needs of a sampled edge's three dot products: {inv, cx, cy, r0}.  cos = dot inv; r0 = (2 (w - cos) / q_norm) coef2, so
// that dL/d(w - cos) = r0 * grad_loss (q_norm = global #sampled edges); d cos / d x = y inv - cx x, d cos / d y = x inv - cy y, cx = cos /
// |x|^2 and cy = cos / |y|^2 while F.cosine_similarity's eps clamp is inactive and 0 under it, as autograd.
struct EdgeBwdScalars {
    float inv, cx, cy, r0;
    __device__ __forceinline__ EdgeBwdScalars(float dot, float nx, float ny, float wj, float q_norm, float coef2) {
        const float den2 = fmaxf(nx * ny, 1e-16f);
        inv = 1.0f / sqrtf(den2);
        const float cs = dot * inv;
        r0 = 2.0f * (wj - cs) / q_norm * coef2;
        const bool clamped = nx * ny < 1e-16f;
        cx = clamped ? 0.f : cs / nx;
        cy = clamped ? 0.f : cs / ny;
    }
};

// Per sampled edge: dw[j] and the gradient rows wrt logits[src] (Gs) and logits[dst] (Gd).
// One 16-lane group per sampled edge (16 edges per workgroup): the group's lanes stride the C logit columns, so the two
// [q, C] gradient-row arrays are written as contiguous segments (a thread-per-edge loop writes them with a stride of C
// floats: 69 us at q = 100 000, C = 41).  The three dot products are reduced inside the group in a fixed order.
__global__ void __launch_bounds__(kT) reg_bwd_edges(const float* __restrict__ w, const int64_t* __restrict__ sei, int64_t q,
                                                   const float* __restrict__ logits, int64_t C, const int64_t* __restrict__ y,
                                                   const uint8_t* __restrict__ tm, const float* __restrict__ out, float coef1,
                                                   float coef2, float q_norm, const float* __restrict__ grad_loss,
                                                   float* __restrict__ dw, float* __restrict__ Gs, float* __restrict__ Gd) {
    const int sub = threadIdx.x & 15;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * (kT / 16) + (threadIdx.x >> 4);
    const bool live = j < q;
    const int64_t jj = live ? j : 0;
    const float gl = grad_loss[0];
    const int64_t s = sei[jj], d = sei[q + jj];
    const float* x = logits + s * C;
    const float* yv = logits + d * C;
    float dot = 0.f, nx = 0.f, ny = 0.f;
    for (int64_t c = sub; c < C; c += 16) {
        const float a = x[c], b = yv[c];
        dot = fmaf(a, b, dot); nx = fmaf(a, a, nx); ny = fmaf(b, b, ny);
    }
    dot = row16_sum_all_dpp(dot); nx = row16_sum_all_dpp(nx); ny = row16_sum_all_dpp(ny);      // all 16 lanes of a group end with the same sums
    if (!live) return;
    const float wj = w[j];
    const EdgeBwdScalars st(dot, nx, ny, wj, q_norm, coef2);
    const float inv = st.inv, cx = st.cx, cy = st.cy;
    const float r = st.r0 * gl;                                                    // dL/d(w - cos) = ((2 (w - cos) / q_norm) coef2) gl
    if (sub == 0) {
        float g = r;
        if (coef1 != 0.f && out[3] > 1.f && tm[s] && tm[d]) {
            const float tgt = (y[s] == y[d]) ? 1.f : 0.f;
            g += coef1 * gl * (wj - tgt) / fmaxf((1.f - wj) * wj, 1e-12f) / out[2];   // torch's BCE backward
        }
        dw[j] = g;
    }
    for (int64_t c = sub; c < C; c += 16) {
        const float a = x[c], b = yv[c];
        Gs[j * C + c] = -r * (b * inv - cx * a);
        Gd[j * C + c] = -r * (a * inv - cy * b);
    }
}

// ---------------------------------------------------------------- the hybrid loss in three launches (sgs_hybrid_loss_fused_fwd / _bwd)
// Forward, one launch for two jobs (as spmm_rowgroup_pair_dual): the first nce workgroups do ce_rows<kW>'s work, the
// rest reg_fwd_partial's.  Partials, block-sum order and the per-thread accumulation order over the four rounds are reg_fwd_partial's, so
// hybrid_loss_final reads the same bits.  What differs is the order of the LOADS: reg_fwd_partial reads w, tm[s], tm[d], y[s], y[d] under
// `if (live && sub == 0)` inside each round, so its four rounds go through memory one after another (index -> rows -> scalars, four
// times); here the indices of all four rounds are read first, then every row segment and every scalar, unconditionally on clamped
// indices, and the arithmetic follows.  The row loop runs column-outer / round-inner: each round's three sums still take their columns
// in increasing order.
// `stash` (may be null: no gradient wanted) keeps per sampled edge what the backward needs of the three dot products:
// EdgeBwdScalars' {inv, cx, cy, r0} with r = r0 * grad_loss -- 16 bytes per edge in place of two gradient rows.
template <bool kW>
__global__ void __launch_bounds__(kT) hybrid_fwd_pair(const float* __restrict__ w, const int64_t* __restrict__ sei, int64_t q,
                                                     const float* __restrict__ logits, int64_t N, int64_t C, const int64_t* __restrict__ y,
                                                     const uint8_t* __restrict__ tm, int64_t nce, float coef2, float q_norm,
                                                     const float* __restrict__ weight, float eps, float* __restrict__ part,
                                                     float4* __restrict__ stash, float* __restrict__ row_lse, float* __restrict__ rowloss) {
    const int64_t blk = static_cast<int64_t>(blockIdx.x) - nce;         // the row-loss workgroups come first: short, and not the launch's tail
    if (blk < 0) {
        const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
        ce_row<kW>(i, threadIdx.x & 63, logits, N, C, y, tm, CeNorm<kW>::make(weight, eps, y, C), row_lse, rowloss);
        return;
    }
    __shared__ float red[4][kT / 64];
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    int64_t jj[kRegRounds], s[kRegRounds], d[kRegRounds];
    bool live[kRegRounds];
#pragma unroll
    for (int r = 0; r < kRegRounds; ++r) {
        const int64_t j = blk * kRegEdges + r * (kT / 16) + grp;
        live[r] = j < q;
        jj[r] = live[r] ? j : 0;
    }
#pragma unroll
    for (int r = 0; r < kRegRounds; ++r) { s[r] = sei[jj[r]]; d[r] = sei[q + jj[r]]; }
    float wj[kRegRounds];
    uint8_t ts[kRegRounds], td[kRegRounds];
    int64_t ys[kRegRounds], yd[kRegRounds];
#pragma unroll
    for (int r = 0; r < kRegRounds; ++r) { wj[r] = w[jj[r]]; ts[r] = tm[s[r]]; td[r] = tm[d[r]]; ys[r] = y[s[r]]; yd[r] = y[d[r]]; }
    float dot[kRegRounds], nx[kRegRounds], ny[kRegRounds];
#pragma unroll
    for (int r = 0; r < kRegRounds; ++r) { dot[r] = 0.f; nx[r] = 0.f; ny[r] = 0.f; }
    for (int64_t c = sub; c < C; c += 16) {
        float a[kRegRounds], b[kRegRounds];
#pragma unroll
        for (int r = 0; r < kRegRounds; ++r) { a[r] = logits[s[r] * C + c]; b[r] = logits[d[r] * C + c]; }
#pragma unroll
        for (int r = 0; r < kRegRounds; ++r) {
            dot[r] = fmaf(a[r], b[r], dot[r]); nx[r] = fmaf(a[r], a[r], nx[r]); ny[r] = fmaf(b[r], b[r], ny[r]);
        }
    }
    // Every lane of a group holds every round's three sums: lane r of the group takes round r, so the per-edge arithmetic (a logarithm,
    // a square root, five divisions with the stash) runs once per workgroup and not once per round in lane 0 alone.
#pragma unroll
    for (int r = 0; r < kRegRounds; ++r) { dot[r] = row16_sum_all_dpp(dot[r]); nx[r] = row16_sum_all_dpp(nx[r]); ny[r] = row16_sum_all_dpp(ny[r]); }
    float dt = dot[0], sx = nx[0], sy = ny[0], wr = wj[0];
    bool on = live[0], valid = ts[0] && td[0], same = ys[0] == yd[0];
    int64_t je = jj[0];
#pragma unroll
    for (int r = 1; r < kRegRounds; ++r)
        if (sub == r) {
            dt = dot[r]; sx = nx[r]; sy = ny[r]; wr = wj[r];
            on = live[r]; valid = ts[r] && td[r]; same = ys[r] == yd[r];
            je = jj[r];
        }
    on = on && sub < kRegRounds;
    float t_bce = 0.f, t_sq = 0.f, t_nv = 0.f, t_nl = 0.f;
    if (on) {
        const float cs = cos_from(EdgeTerms{dt, sx, sy});
        const float df = wr - cs;
        t_sq = df * df;
        if (valid) {
            t_nv = 1.f;
            t_nl = same ? 1.f : 0.f;
            // F.binary_cross_entropy clamps each log at -100
            t_bce = same ? -fmaxf(logf(wr), -100.f) : -fmaxf(logf(1.f - wr), -100.f);
        }
        if (stash) {
            const EdgeBwdScalars st(dt, sx, sy, wr, q_norm, coef2);
            stash[je] = make_float4(st.inv, st.cx, st.cy, st.r0);
        }
    }
    // lane 0 of the group adds the four rounds' terms in round order, as reg_fwd_partial's lane 0 does (a round that adds nothing there
    // adds +0 here: the sums start at +0 and are never -0, so the bits are the same)
    float bce = 0.f, sq = 0.f, nv = 0.f, nl = 0.f;
    const int g0 = threadIdx.x & 48;                   // the group's first lane within the wave
#pragma unroll
    for (int r = 0; r < kRegRounds; ++r) {
        bce += __shfl(t_bce, g0 + r, 64); sq += __shfl(t_sq, g0 + r, 64); nv += __shfl(t_nv, g0 + r, 64); nl += __shfl(t_nl, g0 + r, 64);
    }
    if (sub != 0) { bce = 0.f; sq = 0.f; nv = 0.f; nl = 0.f; }
    // block_sum's tree for the four sums at once (one barrier in place of eight): wave sums, then thread 0 adds them in wave order
    bce = wave_sum(bce); sq = wave_sum(sq); nv = wave_sum(nv); nl = wave_sum(nl);
    if ((threadIdx.x & 63) == 0) {
        const int wid = threadIdx.x >> 6;
        red[0][wid] = bce; red[1][wid] = sq; red[2][wid] = nv; red[3][wid] = nl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r[k] = 0.f;
            for (int i = 0; i < kT / 64; ++i) r[k] += red[k][i];
        }
        part[4 * blk + 0] = r[0]; part[4 * blk + 1] = r[1];
        part[4 * blk + 2] = r[2]; part[4 * blk + 3] = r[3];
    }
}

// Backward, one launch: the endpoint reduction's traversal (csrc/endpoint_reduce.h) with the terms FORMED where they are added, in
// place of reg_bwd_edges -> endpoint_reduce -> ce_bwd<kW, true> and their two [q, C] arrays.  For a sampled edge e = (s, d) with the forward's
// {inv, cx, cy, r0} and r = r0 * grad_loss, the entry of e in s's out-row is reg_bwd_edges' Gs[e, c] = -r (b inv - cx a) and the entry in
// d's in-row its Gd[e, c] = -r (a inv - cy b), a = logits[s, c], b = logits[d, c]: the node's own row is read once, the neighbour's per
// entry (the table is cache resident).  Every sampled edge is in exactly one out-row (self-loops included), whose visitor writes dw[e]
// by reg_bwd_edges' formula; the writer of dlogits[v, c] adds the cross entropy's term, ce_bwd<kW, true>'s.
template <bool kW>
struct EpHybridTerms {
    static constexpr bool kCol = true, kVisit = true;
    const float* __restrict__ logits;
    int64_t C;
    const float4* __restrict__ stash;
    const float* __restrict__ w;
    const int64_t* __restrict__ y;
    const uint8_t* __restrict__ tm;
    const float* __restrict__ out7;
    float coef1;
    const float* __restrict__ grad_loss;
    float* __restrict__ dw;
    const float* __restrict__ weight;
    float eps;
    const float* __restrict__ row_lse;
    const typename CeNorm<kW>::Word* __restrict__ norm;          // n_rows (int32) of the plain criterion, den (float) of the weighted one
    // What every entry of a workgroup needs is read once: W, grad_loss and whether reg1 is on (coef1 != 0 and a label sum above 1)
    // with its divisor out[2].
    struct Blk { float W, gl, nvalid; bool reg1; };
    struct Own { float x; };
    struct Raw { float4 st; float nb; };
    // A value that is the same in every lane and that this kernel never writes goes through the scalar cache (one request per wave, no
    // work for the vector memory pipe, which the row loads of a hub node's workgroup keep busy).
    template <class T>
    static __device__ __forceinline__ T uniform_load(const T* ptr) {
        return *(const __attribute__((address_space(4))) T*)(ptr);
    }
    __device__ __forceinline__ Blk block_init() const {
        Blk b;
        b.W = static_cast<float>(C);
        b.gl = uniform_load(grad_loss);
        b.nvalid = uniform_load(out7 + 2);
        b.reg1 = coef1 != 0.f && uniform_load(out7 + 3) > 1.f;
        if constexpr (kW) {                                 // W = sum_c w_c as ce_bwd<true, *> has it: the workgroup's first kT threads form it
            __shared__ float red[kT / 64];
            if (eps != 0.f && weight) b.W = block_weight_sum<kT>(weight, C, red);         // (uniform branch)
        }
        return b;
    }
    __device__ __forceinline__ Own own(int64_t v, int64_t, int64_t c0) const { return Own{logits[v * C + c0]}; }
    // The four stash words of the four entries in flight are ONE load: lane l reads word (l >> 2) & 3 of entry l & 3's edge, and
    // v_readlane hands entry u its words from lanes u, 4 + u, 8 + u, 12 + u.  (As four 64-lane loads of one address each, and as scalar
    // loads -- a stream of misses in the scalar cache --, the same words set the kernel's time.)
    struct Pre { float word; };
    __device__ __forceinline__ Pre preload(int e_lane, int lane) const {
        return Pre{reinterpret_cast<const float*>(stash)[static_cast<int64_t>(e_lane) * 4 + ((lane >> 2) & 3)]};
    }
    __device__ __forceinline__ Raw load(const Pre& pre, int u, bool, int, int col, int64_t, int64_t c0) const {
        const int wd = __float_as_int(pre.word);
        Raw r;
        r.st = make_float4(__int_as_float(__builtin_amdgcn_readlane(wd, u)), __int_as_float(__builtin_amdgcn_readlane(wd, 4 + u)),
                           __int_as_float(__builtin_amdgcn_readlane(wd, 8 + u)), __int_as_float(__builtin_amdgcn_readlane(wd, 12 + u)));
        r.nb = logits[static_cast<int64_t>(col) * C + c0];
        return r;
    }
    __device__ __forceinline__ void term(const Blk& blk, const Raw& rw, const Own& o, bool isout, float (&m)[1], float (&t)[1]) const {
        const float inv = rw.st.x, cx = rw.st.y, cy = rw.st.z;
        const float r = rw.st.w * blk.gl;
        const float a = isout ? o.x : rw.nb, b = isout ? rw.nb : o.x;
        m[0] = isout ? -r * (b * inv - cx * a) : -r * (a * inv - cy * b);
        t[0] = 1.f;
    }
    // d w of the out entry (v, col) = edge e, one entry per thread (as a visitor inside the sums it ran in one lane, entry after entry,
    // and its two divisions set the kernel's time).
    __device__ __forceinline__ void visit(const Blk& blk, int64_t v, int e, int col) const {
        const float gl = blk.gl;
        const float wj = w[e];
        const float r = stash[e].w * gl;
        float g = r;
        if (blk.reg1 && tm[v] && tm[col]) {
            const float tgt = (y[v] == y[col]) ? 1.f : 0.f;
            g += coef1 * gl * (wj - tgt) / fmaxf((1.f - wj) * wj, 1e-12f) / blk.nvalid;   // torch's BCE backward
        }
        dw[e] = g;
    }
    __device__ __forceinline__ float finish(const Blk& blk, int64_t v, int64_t c, float sum) const {
        if (!tm[v]) return sum;
        return sum + ce_grad<kW>(CeNorm<kW>::make(weight, eps, y, C), logits[v * C + c], row_lse[v], y[v], c, C, blk.W, grad_loss, norm);
    }
};


// ---------------------------------------------------------------- ensemble mean + the three split counts (evaluate.py, ensemble_evaluate)
// One wave per row.  acc = ((o_0 + o_1) + o_2) + ... in draw order (fp32, as the serial loop's `out = out + o`), carried across passes in
// `acc`; the last pass multiplies by 1/D when D > 1 -- torch's true division by a Python scalar is a multiply by the fp32 reciprocal on the
// device -- and counts the argmax (first maximum wins, as masked_correct) against y on the three masks into counts[6] (int64, accumulated).
__global__ void __launch_bounds__(kT) ensemble_mean_correct(const float* __restrict__ logits, int64_t xs, int Dc, int64_t N, int64_t C,
                                                           float* __restrict__ acc, int first, int last, int D_total, float inv,
                                                           const int64_t* __restrict__ y, const uint8_t* __restrict__ m0,
                                                           const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2,
                                                           unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int64_t c = lane; c < C; c += 64) {
        float v = first ? logits[i * C + c] : acc[i * C + c];
        for (int d = first ? 1 : 0; d < Dc; ++d) v = __fadd_rn(v, logits[static_cast<int64_t>(d) * xs + i * C + c]);
        if (last && D_total > 1) v = __fmul_rn(v, inv);
        acc[i * C + c] = v;
        if (v > best || (v == best && static_cast<int>(c) < bi) || bi == 0x7fffffff) { best = v; bi = static_cast<int>(c); }
    }
    if (!last) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
    }
    if (lane == 0) {
        const bool ok = static_cast<int64_t>(bi) == y[i];
        const uint8_t* ms[3] = {m0, m1, m2};
#pragma unroll
        for (int s = 0; s < 3; ++s)
            if (ms[s][i]) {
                atomicAdd(&counts[2 * s + 1], 1ull);
                if (ok) atomicAdd(&counts[2 * s], 1ull);
            }
    }
}

// ---------------------------------------------------------------- per-split confusion counts (evaluate.py: macro / weighted F1, per-class report)
// conf[s][y_i][argmax_c logits[i, c]] += 1 for every row i and split s with m_s[i] != 0; conf is int64 [3, C, C], accumulated.  Integer
// atomics only, so the matrix does not depend on arrival order.  A row outside every mask is left before its label is read; a masked row
// whose label is outside [0, C) breaks the contract and is skipped, never used as an index.
__device__ __forceinline__ int wave_row_argmax(const float* __restrict__ row, int64_t C, int lane) {      // valid in every lane (C >= 1)
    float best = -INFINITY;
    int bi = 0x7fffffff;
    lane_argmax(row, C, lane, best, bi);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
    }
    return bi;
}

// Direct form: one wave per row, lane 0 issues up to three non-returning 64-bit global adds.
__global__ void __launch_bounds__(kT) confusion_direct(const float* __restrict__ logits, int64_t N, int64_t C, const int64_t* __restrict__ y,
                                                      const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1,
                                                      const uint8_t* __restrict__ m2, unsigned long long* __restrict__ conf) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    const bool in0 = m0[i] != 0, in1 = m1[i] != 0, in2 = m2[i] != 0;
    if (!(in0 || in1 || in2)) return;
    const int bi = wave_row_argmax(logits + i * C, C, lane);
    if (lane != 0) return;
    const int64_t t = y[i];
    if (t < 0 || t >= C) return;
    const int64_t cell = t * C + bi;
    if (in0) atomicAdd(&conf[cell], 1ull);
    if (in1) atomicAdd(&conf[C * C + cell], 1ull);
    if (in2) atomicAdd(&conf[2 * C * C + cell], 1ull);
}

// Privatised form (12 C^2 <= 65536 bytes of LDS, N < 2^31): a workgroup of 16 waves keeps an int32 [3, C, C] histogram in LDS, walks rows
// in a grid-stride loop and adds only its non-zero cells to conf at the end: the hot cells (the diagonal of a trained model) take one
// global add per workgroup instead of one per row.
constexpr int kConfT = 1024;
__global__ void __launch_bounds__(kConfT) confusion_private(const float* __restrict__ logits, int64_t N, int64_t C, const int64_t* __restrict__ y,
                                                           const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1,
                                                           const uint8_t* __restrict__ m2, unsigned long long* __restrict__ conf) {
    extern __shared__ int hist[];
    const int cells = 3 * static_cast<int>(C * C);
    for (int k = threadIdx.x; k < cells; k += kConfT) hist[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int cc = static_cast<int>(C * C);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * (kConfT / 64) + wid; i < N; i += static_cast<int64_t>(gridDim.x) * (kConfT / 64)) {
        const bool in0 = m0[i] != 0, in1 = m1[i] != 0, in2 = m2[i] != 0;
        if (!(in0 || in1 || in2)) continue;
        const int bi = wave_row_argmax(logits + i * C, C, lane);
        if (lane != 0) continue;
        const int64_t t = y[i];
        if (t < 0 || t >= C) continue;
        const int cell = static_cast<int>(t * C) + bi;
        if (in0) atomicAdd(&hist[cell], 1);
        if (in1) atomicAdd(&hist[cc + cell], 1);
        if (in2) atomicAdd(&hist[2 * cc + cell], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += kConfT) {
        const int v = hist[k];
        if (v) atomicAdd(&conf[k], static_cast<unsigned long long>(v));
    }
}

constexpr int64_t kConfPrivMaxC = 73;             // 12 * 73^2 = 63 948 <= 65 536 bytes of LDS; 74 needs 65 712
// The automatic rule (include/sgs_hip.h; measurements in DESIGN.md section 5, "Per-class evaluation metrics"): the direct form's adds
// queue up per 128-byte line of conf, 3 C^2 / 16 lines in all, so it loses only at few classes and many rows.
constexpr int64_t kConfAutoMaxC = 12;
constexpr int64_t kConfAutoMinRows = 4096;
std::atomic<int> g_conf_variant{0};

// ---------------------------------------------------------------- class-pair edge counts (sparsify.py: the export's quality report)
// pairs[y[src_e]][y[dst_e]] += 1 for every edge e with mask == nullptr or mask[e] != 0; pairs is int64 [C, C], accumulated.  Integer
// atomics only.  An edge with an endpoint outside [0, N) or a label outside [0, C) is skipped, never used as an index.
__device__ __forceinline__ int64_t edge_class_cell(const int64_t* __restrict__ edge_index, int64_t n, const uint8_t* __restrict__ mask,
                                                   const int64_t* __restrict__ y, int64_t N, int64_t C, int64_t e) {      // -1: skipped
    if (mask && mask[e] == 0) return -1;
    const int64_t s = edge_index[e], d = edge_index[n + e];
    if (s < 0 || s >= N || d < 0 || d >= N) return -1;
    const int64_t a = y[s], b = y[d];
    if (a < 0 || a >= C || b < 0 || b >= C) return -1;
    return a * C + b;
}
// Direct form: one thread per edge, one non-returning 64-bit global add.
__global__ void __launch_bounds__(kT) edge_class_direct(const int64_t* __restrict__ edge_index, int64_t n, const uint8_t* __restrict__ mask,
                                                       const int64_t* __restrict__ y, int64_t N, int64_t C, unsigned long long* __restrict__ pairs) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (e >= n) return;
    const int64_t cell = edge_class_cell(edge_index, n, mask, y, N, C, e);
    if (cell >= 0) atomicAdd(&pairs[cell], 1ull);
}
// Privatised form (4 C^2 <= 65536 bytes of LDS, n < 2^31): an int32 [C, C] table per workgroup over a grid-stride loop, the non-zero cells
// added to pairs at the end.  With few classes nearly every edge of a homophilous graph hits one of the C diagonal cells: those take one
// global add per workgroup instead of one per edge.
__global__ void __launch_bounds__(kConfT) edge_class_private(const int64_t* __restrict__ edge_index, int64_t n, const uint8_t* __restrict__ mask,
                                                            const int64_t* __restrict__ y, int64_t N, int64_t C,
                                                            unsigned long long* __restrict__ pairs) {
    extern __shared__ int hist[];
    const int cells = static_cast<int>(C * C);
    for (int k = threadIdx.x; k < cells; k += kConfT) hist[k] = 0;
    __syncthreads();
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kConfT + threadIdx.x; e < n; e += static_cast<int64_t>(gridDim.x) * kConfT) {
        const int64_t cell = edge_class_cell(edge_index, n, mask, y, N, C, e);
        if (cell >= 0) atomicAdd(&hist[static_cast<int>(cell)], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += kConfT) {
        const int v = hist[k];
        if (v) atomicAdd(&pairs[k], static_cast<unsigned long long>(v));
    }
}
constexpr int64_t kPairPrivMaxC = 128;            // 4 * 128^2 = 65 536 bytes of LDS
std::atomic<int> g_pair_variant{0};

}  // namespace
}  // namespace sgs

using namespace sgs;

namespace {

// The cross entropy entries' argument checks: `ok` is the entry's own condition; the plain entries count a null n_rows among the bad
// arguments, the weighted ones name the smoothing and `den` on their own.
template <bool kW>
int ce_check(const char* fn, bool ok, const void* norm, float eps) {
    SGS_REQUIRE(ok && (kW || norm), SGS_EINVAL, "%s: bad arguments", fn);
    if (kW) {
        SGS_REQUIRE(eps >= 0.f && eps <= 1.f, SGS_EINVAL, "%s: label_smoothing outside [0, 1]", fn);
        SGS_REQUIRE(norm, SGS_EINVAL, "%s: den is NULL", fn);
    }
    return SGS_OK;
}

template <bool kW>
int masked_ce_fwd(const char* fn, const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* weight,
                  float eps, float* loss, float* row_lse, float* rowloss, typename CeNorm<kW>::Word* norm, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // (the weighted divisor is summed in fp32 by one block: N < 2^24 as in the hybrid forwards)
    if (int rc = ce_check<kW>(fn, N > 0 && (!kW || N < (int64_t(1) << 24)) && C > 0 && logits && y && train_mask && loss && row_lse && rowloss, norm, eps))
        return rc;
    const CeNorm<kW> cn = CeNorm<kW>::make(weight, eps, y, C);
    hipLaunchKernelGGL(ce_rows<kW>, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, logits, N, C, y, train_mask, row_lse, rowloss, cn);
    hipLaunchKernelGGL(ce_final<kW>, dim3(1), dim3(1024), 0, stream, static_cast<const float*>(rowloss), train_mask, N, loss, norm, cn);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

template <bool kW, bool kAcc>
int masked_ce_bwd(const char* fn, const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* weight,
                  float eps, const float* row_lse, const typename CeNorm<kW>::Word* norm, const float* grad_loss, float* dlogits,
                  sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = ce_check<kW>(fn, N > 0 && C > 0 && logits && y && train_mask && row_lse && grad_loss && dlogits, norm, eps)) return rc;
    hipLaunchKernelGGL((ce_bwd<kW, kAcc>), dim3(cdiv(N * C, kT)), dim3(kT), 0, stream, logits, N, C, y, train_mask, row_lse, norm, grad_loss, dlogits,
                       CeNorm<kW>::make(weight, eps, y, C));
    SGS_LAUNCH_OK();
    return SGS_OK;
}

// The launches of the three hybrid forwards, after their checks: row losses and per-edge partials (`fused`: in one launch, with the
// backward's stash), then the finishing block.
template <bool kW>
int hybrid_loss_launch(bool fused, const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w,
                       const int64_t* sei, int64_t q, float coef1, float coef2, const float* weight, float eps, float* out, float* row_lse,
                       float* rowloss, void* norm, float* stash, void* ws, hipStream_t stream) {
    Carver cv(ws);
    const int64_t nblk = cdiv(q, kRegEdges);
    float* part = cv.take<float>(4 * (nblk + 1));
    const int64_t nce = cdiv(N * 64, kT);
    const CeNorm<kW> cn = CeNorm<kW>::make(weight, eps, y, C);
    if (fused) {
        hipLaunchKernelGGL(hybrid_fwd_pair<kW>, dim3(static_cast<unsigned>(nce + nblk)), dim3(kT), 0, stream, w, sei, q, logits, N, C, y, train_mask, nce,
                           coef2, static_cast<float>(q), weight, eps, part, reinterpret_cast<float4*>(stash), row_lse, rowloss);
    } else {
        hipLaunchKernelGGL(ce_rows<kW>, dim3(nce), dim3(kT), 0, stream, logits, N, C, y, train_mask, row_lse, rowloss, cn);
        hipLaunchKernelGGL(reg_fwd_partial, dim3(nblk), dim3(kT), 0, stream, w, sei, q, logits, C, y, train_mask, static_cast<float*>(nullptr), part);
    }
    hipLaunchKernelGGL(hybrid_loss_final<kW>, dim3(1), dim3(kT), 0, stream, static_cast<const float*>(part), nblk, q, coef1, coef2,
                       static_cast<const float*>(rowloss), train_mask, N, out, static_cast<typename CeNorm<kW>::Word*>(norm), cn);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

template <bool kW>
int hybrid_loss_fwd(const char* fn, const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w,
                    const int64_t* sei, int64_t q, float coef1, float coef2, const float* weight, float eps, float* out, float* row_lse,
                    float* rowloss, typename CeNorm<kW>::Word* norm, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    if (int rc = ce_check<kW>(fn, q > 0 && N > 0 && N < (int64_t(1) << 24) && C > 0 && logits && y && train_mask && w && sei && out && row_lse && rowloss,
                              norm, eps))
        return rc;
    SGS_REQUIRE(ws && ws_bytes >= sgs_edge_reg_workspace_bytes(q), SGS_EWORKSPACE, "%s: workspace too small", fn);
    return hybrid_loss_launch<kW>(false, logits, N, C, y, train_mask, w, sei, q, coef1, coef2, weight, eps, out, row_lse, rowloss, norm, nullptr, ws,
                                  static_cast<hipStream_t>(stream_));
}

}  // namespace

extern "C" {

int sgs_masked_correct(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask,
                       int32_t* correct, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && C > 0 && correct, SGS_EINVAL, "sgs_masked_correct: bad arguments");
    if (int rc = zero_async(correct, 8, stream)) return rc;
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(logits && y && train_mask, SGS_EINVAL, "sgs_masked_correct: null pointer");
    hipLaunchKernelGGL(masked_correct, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, logits, N, C, y, train_mask, correct);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_masked_correct_pair(const float* logits_a, const float* logits_b, int64_t N, int64_t C, const int64_t* y,
                            const uint8_t* train_mask, int32_t* correct4, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && C > 0 && correct4, SGS_EINVAL, "sgs_masked_correct_pair: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(logits_a && logits_b && y && train_mask, SGS_EINVAL, "sgs_masked_correct_pair: null pointer");
    hipLaunchKernelGGL(masked_correct_pair, dim3(static_cast<unsigned>(cdiv(N, 16)), 2), dim3(1024), 0, stream, logits_a, logits_b, N, C, y, train_mask,
                       correct4);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_gate_counts_workspace_bytes(int64_t N) { return carve_bytes(static_cast<size_t>(2 * (cdiv(N < 0 ? 0 : N, 16) + 1)), 8) + 256; }

int sgs_gate_counts(const float* logits_a, const float* logits_b, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask,
                    int32_t* out5, const uint64_t* seq_dev, int32_t* dst_host_mapped, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && N < (int64_t(1) << 30) && C > 0 && out5, SGS_EINVAL, "sgs_gate_counts: bad arguments");
    SGS_REQUIRE(N == 0 || (logits_a && logits_b && y && train_mask), SGS_EINVAL, "sgs_gate_counts: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_gate_counts_workspace_bytes(N), SGS_EWORKSPACE, "sgs_gate_counts: workspace too small");
    Carver cv(ws);
    const int nblk = static_cast<int>(cdiv(N, 16));
    int2* part = reinterpret_cast<int2*>(cv.take<int64_t>(static_cast<size_t>(2 * (nblk + 1))));
    if (nblk > 0)
        hipLaunchKernelGGL(gate_counts_partial, dim3(static_cast<unsigned>(nblk), 2), dim3(1024), 0, stream, logits_a, logits_b, N, C, y, train_mask,
                           part);
    hipLaunchKernelGGL(gate_counts_finish, dim3(1), dim3(64), 0, stream, static_cast<const int2*>(part), nblk, out5, seq_dev, dst_host_mapped);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_loss_tick(float* loss_sum, const float* loss, uint64_t* epoch, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(loss_tick, dim3(1), dim3(64), 0, stream, loss_sum, loss, epoch);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_publish_to_host(const int32_t* src_dev, int64_t n, const uint64_t* seq_dev, int32_t* dst_host_mapped, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n > 0 && n <= 63 && src_dev && dst_host_mapped, SGS_EINVAL, "sgs_publish_to_host: bad arguments");
    hipLaunchKernelGGL(publish_words, dim3(1), dim3(64), 0, stream, src_dev, static_cast<int>(n), seq_dev, dst_host_mapped);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_masked_ce_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, float* loss,
                      float* row_lse, float* rowloss, int32_t* n_rows, sgs_stream_t stream_) {
    return masked_ce_fwd<false>("sgs_masked_ce_fwd", logits, N, C, y, train_mask, nullptr, 0.f, loss, row_lse, rowloss, n_rows, stream_);
}

int sgs_masked_ce_bwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask,
                      const float* row_lse, const int32_t* n_rows, const float* grad_loss, float* dlogits,
                      sgs_stream_t stream_) {
    return masked_ce_bwd<false, false>("sgs_masked_ce_bwd", logits, N, C, y, train_mask, nullptr, 0.f, row_lse, n_rows, grad_loss, dlogits, stream_);
}

int sgs_masked_ce_bwd_acc(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* row_lse,
                          const int32_t* n_rows, const float* grad_loss, float* dlogits, sgs_stream_t stream_) {
    return masked_ce_bwd<false, true>("sgs_masked_ce_bwd_acc", logits, N, C, y, train_mask, nullptr, 0.f, row_lse, n_rows, grad_loss, dlogits, stream_);
}

int sgs_masked_ce_w_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* weight,
                        float label_smoothing, float* loss, float* row_lse, float* rowloss, float* den, sgs_stream_t stream_) {
    return masked_ce_fwd<true>("sgs_masked_ce_w_fwd", logits, N, C, y, train_mask, weight, label_smoothing, loss, row_lse, rowloss, den, stream_);
}

int sgs_masked_ce_w_bwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* weight,
                        float label_smoothing, const float* row_lse, const float* den, const float* grad_loss, float* dlogits,
                        sgs_stream_t stream_) {
    return masked_ce_bwd<true, false>("sgs_masked_ce_w_bwd", logits, N, C, y, train_mask, weight, label_smoothing, row_lse, den, grad_loss, dlogits,
                                      stream_);
}

int sgs_masked_ce_w_bwd_acc(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* weight,
                            float label_smoothing, const float* row_lse, const float* den, const float* grad_loss, float* dlogits,
                            sgs_stream_t stream_) {
    return masked_ce_bwd<true, true>("sgs_masked_ce_w_bwd_acc", logits, N, C, y, train_mask, weight, label_smoothing, row_lse, den, grad_loss, dlogits,
                                     stream_);
}

int sgs_hybrid_loss_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w,
                        const int64_t* sampled_edge_index, int64_t q, float coef1, float coef2, float* out, float* row_lse, float* rowloss,
                        int32_t* n_rows, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    return hybrid_loss_fwd<false>("sgs_hybrid_loss_fwd", logits, N, C, y, train_mask, w, sampled_edge_index, q, coef1, coef2, nullptr, 0.f, out, row_lse,
                                  rowloss, n_rows, ws, ws_bytes, stream_);
}

int sgs_hybrid_loss_w_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w,
                          const int64_t* sampled_edge_index, int64_t q, float coef1, float coef2, const float* weight, float label_smoothing,
                          float* out, float* row_lse, float* rowloss, float* den, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    return hybrid_loss_fwd<true>("sgs_hybrid_loss_w_fwd", logits, N, C, y, train_mask, w, sampled_edge_index, q, coef1, coef2, weight, label_smoothing,
                                 out, row_lse, rowloss, den, ws, ws_bytes, stream_);
}

size_t sgs_edge_reg_workspace_bytes(int64_t q) { return carve_bytes(4 * (cdiv(q < 0 ? 0 : q, kRegEdges) + 1), 4) + 256; }

int sgs_edge_reg_fwd(const float* w, const int64_t* sampled_edge_index, int64_t q, const float* logits, int64_t N, int64_t C,
                     const int64_t* y, const uint8_t* train_mask, float coef1, float coef2, float* out, float* cos_out,
                     void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(q > 0 && N > 0 && C > 0 && w && sampled_edge_index && logits && y && train_mask && out, SGS_EINVAL,
                "sgs_edge_reg_fwd: bad arguments");
    SGS_REQUIRE(ws && ws_bytes >= sgs_edge_reg_workspace_bytes(q), SGS_EWORKSPACE, "sgs_edge_reg_fwd: workspace too small");
    Carver cv(ws);
    const int64_t nblk = cdiv(q, kRegEdges);
    float* part = cv.take<float>(4 * (nblk + 1));
    hipLaunchKernelGGL(reg_fwd_partial, dim3(nblk), dim3(kT), 0, stream, w, sampled_edge_index, q, logits, C, y, train_mask, cos_out,
                       part);
    hipLaunchKernelGGL(reg_fwd_final, dim3(1), dim3(kT), 0, stream, part, nblk, q, coef1, coef2, out);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_edge_reg_partial(const float* w, const int64_t* sampled_edge_index, int64_t q, const float* logits, int64_t N, int64_t C,
                         const int64_t* y, const uint8_t* train_mask, float* raw, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(q >= 0 && N > 0 && C > 0 && raw, SGS_EINVAL, "sgs_edge_reg_partial: bad arguments");
    SGS_REQUIRE(ws && ws_bytes >= sgs_edge_reg_workspace_bytes(q), SGS_EWORKSPACE, "sgs_edge_reg_partial: workspace too small");
    Carver cv(ws);
    const int64_t nblk = cdiv(q, kRegEdges);
    float* part = cv.take<float>(4 * (nblk + 1));
    if (q > 0) {
        SGS_REQUIRE(w && sampled_edge_index && logits && y && train_mask, SGS_EINVAL, "sgs_edge_reg_partial: null pointer");
        hipLaunchKernelGGL(reg_fwd_partial, dim3(nblk), dim3(kT), 0, stream, w, sampled_edge_index, q, logits, C, y, train_mask,
                           static_cast<float*>(nullptr), part);
    }
    hipLaunchKernelGGL(reg_raw_final, dim3(1), dim3(kT), 0, stream, part, nblk, raw);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_edge_reg_bwd(const float* w, const int64_t* sampled_edge_index, int64_t q, int64_t q_global, const float* logits, int64_t N,
                     int64_t C, const int64_t* y, const uint8_t* train_mask, const float* out, float coef1, float coef2,
                     const float* grad_loss, float* dw, float* Gs, float* Gd, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(q >= 0 && q_global >= q && N > 0 && C > 0, SGS_EINVAL, "sgs_edge_reg_bwd: bad arguments");
    if (q == 0) return SGS_OK;
    SGS_REQUIRE(w && sampled_edge_index && logits && y && train_mask && out && grad_loss && dw && Gs && Gd, SGS_EINVAL,
                "sgs_edge_reg_bwd: null pointer");
    hipLaunchKernelGGL(reg_bwd_edges, dim3(cdiv(q, kT / 16)), dim3(kT), 0, stream, w, sampled_edge_index, q, logits, C, y, train_mask, out,
                       coef1, coef2, static_cast<float>(q_global), grad_loss, dw, Gs, Gd);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_hybrid_loss_fused_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w,
                              const int64_t* sampled_edge_index, int64_t q, float coef1, float coef2, int weighted, const float* weight,
                              float label_smoothing, float* out, float* row_lse, float* rowloss, void* norm, float* stash, void* ws,
                              size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(q > 0 && N > 0 && N < (int64_t(1) << 24) && C > 0 && logits && y && train_mask && w && sampled_edge_index && out && row_lse &&
                    rowloss && norm,
                SGS_EINVAL, "sgs_hybrid_loss_fused_fwd: bad arguments");
    SGS_REQUIRE(weighted ? (label_smoothing >= 0.f && label_smoothing <= 1.f) : (!weight && label_smoothing == 0.f), SGS_EINVAL,
                "sgs_hybrid_loss_fused_fwd: label_smoothing outside [0, 1], or a weight / smoothing without `weighted`");
    SGS_REQUIRE((reinterpret_cast<uintptr_t>(stash) & 15) == 0, SGS_EINVAL, "sgs_hybrid_loss_fused_fwd: stash must be 16-byte aligned");
    SGS_REQUIRE(ws && ws_bytes >= sgs_edge_reg_workspace_bytes(q), SGS_EWORKSPACE, "sgs_hybrid_loss_fused_fwd: workspace too small");
    return (weighted ? hybrid_loss_launch<true> : hybrid_loss_launch<false>)(true, logits, N, C, y, train_mask, w, sampled_edge_index, q, coef1, coef2,
                                                                             weight, label_smoothing, out, row_lse, rowloss, norm, stash, ws, stream);
}

int sgs_hybrid_loss_fused_bwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w, int64_t q,
                              const float* stash, const float* out, float coef1, int weighted, const float* weight, float label_smoothing,
                              const float* row_lse, const void* norm, const float* grad_loss, const int32_t* in_ptr, const int32_t* in_src,
                              const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* dw,
                              float* dlogits, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(q > 0 && N > 0 && N < (int64_t(1) << 31) && C > 0 && logits && y && train_mask && w && stash && out && row_lse && norm && grad_loss &&
                    in_ptr && in_src && in_eid && out_ptr && out_dst && out_eid && dw && dlogits,
                SGS_EINVAL, "sgs_hybrid_loss_fused_bwd: bad arguments");
    SGS_REQUIRE(weighted ? (label_smoothing >= 0.f && label_smoothing <= 1.f) : (!weight && label_smoothing == 0.f), SGS_EINVAL,
                "sgs_hybrid_loss_fused_bwd: label_smoothing outside [0, 1], or a weight / smoothing without `weighted`");
    SGS_REQUIRE((reinterpret_cast<uintptr_t>(stash) & 15) == 0, SGS_EINVAL, "sgs_hybrid_loss_fused_bwd: stash must be 16-byte aligned");
    const int nw = ep_traversal(q, N);                  // the traversal sgs_endpoint_reduce takes for this (nnz, N)
#define SGS_HYB(KW_)                                                                                                                              \
    do {                                                                                                                                          \
        const EpHybridTerms<KW_> terms{logits, C, reinterpret_cast<const float4*>(stash), w, y, train_mask, out, coef1, grad_loss, dw, weight,    \
                                       label_smoothing, row_lse, static_cast<const CeNorm<KW_>::Word*>(norm)};                                    \
        if (nw == 16)     hipLaunchKernelGGL((endpoint_reduce_rowblock<1, 16, EpHybridTerms<KW_>>), dim3(static_cast<unsigned>(N)), dim3(1024), 0, stream, \
                                             terms, N, C, in_ptr, in_src, in_eid, out_ptr, out_dst, out_eid, 1.0f, 1.0f, dlogits);               \
        else if (nw == 4) hipLaunchKernelGGL((endpoint_reduce_rowblock<1, 4, EpHybridTerms<KW_>>), dim3(static_cast<unsigned>(N)), dim3(256), 0, stream,   \
                                             terms, N, C, in_ptr, in_src, in_eid, out_ptr, out_dst, out_eid, 1.0f, 1.0f, dlogits);               \
        else              hipLaunchKernelGGL((endpoint_reduce<1, EpHybridTerms<KW_>>), dim3(static_cast<unsigned>(cdiv(N * 64, kEpT))), dim3(kEpT), 0,     \
                                             stream, terms, N, C, in_ptr, in_src, in_eid, out_ptr, out_dst, out_eid, 1.0f, 1.0f, dlogits);       \
    } while (0)
    if (weighted) SGS_HYB(true); else SGS_HYB(false);
#undef SGS_HYB
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_ensemble_mean_correct(const float* logits, int64_t x_stride, int64_t Dc, int64_t N, int64_t C, float* acc, int first, int last,
                              int64_t D_total, const int64_t* y, const uint8_t* mask0, const uint8_t* mask1, const uint8_t* mask2, int64_t* counts,
                              sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(Dc >= 1 && N >= 0 && C > 0 && D_total >= Dc && x_stride >= 0 && (Dc == 1 || x_stride == 0 || x_stride >= N * C), SGS_EINVAL,
                "sgs_ensemble_mean_correct: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(logits && acc && (!last || (y && mask0 && mask1 && mask2 && counts)), SGS_EINVAL, "sgs_ensemble_mean_correct: null pointer");
    const float inv = 1.0f / static_cast<float>(D_total);
    hipLaunchKernelGGL(ensemble_mean_correct, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, logits, x_stride, static_cast<int>(Dc), N, C, acc,
                       first, last, static_cast<int>(D_total), inv, y, mask0, mask1, mask2, reinterpret_cast<unsigned long long*>(counts));
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_confusion_variant_set(int code) {
    SGS_REQUIRE(code >= 0 && code <= 2, SGS_EINVAL, "sgs_confusion_variant_set: code %d, need 0 (automatic), 1 (direct) or 2 (privatised)", code);
    g_conf_variant.store(code);
    return SGS_OK;
}

int sgs_confusion_variant(int64_t N, int64_t C) {
    if (N < 0 || C < 1) return -1;
    if (N == 0) return 0;
    const bool priv_ok = C <= kConfPrivMaxC && N < (int64_t(1) << 31);
    switch (g_conf_variant.load()) {
        case 1: return 1;
        case 2: return priv_ok ? 2 : -1;
        default: return priv_ok && C <= kConfAutoMaxC && N >= kConfAutoMinRows ? 2 : 1;
    }
}

int sgs_confusion_counts(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* m0, const uint8_t* m1, const uint8_t* m2,
                         int64_t* conf, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && N < (int64_t(1) << 32) && C >= 1 && C < (int64_t(1) << 24) && conf, SGS_EINVAL, "sgs_confusion_counts: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(logits && y && m0 && m1 && m2, SGS_EINVAL, "sgs_confusion_counts: null pointer");
    const int var = sgs_confusion_variant(N, C);
    SGS_REQUIRE(var > 0, SGS_EINVAL, "sgs_confusion_counts: the privatised form (forced by sgs_confusion_variant_set(2)) needs C <= 73 and N < 2^31");
    unsigned long long* out = reinterpret_cast<unsigned long long*>(conf);
    if (var == 1) {
        hipLaunchKernelGGL(confusion_direct, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, logits, N, C, y, m0, m1, m2, out);
    } else {
        static const int cus = [] {
            int dev = 0, n = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
            return n;
        }();
        const int64_t grid = std::min<int64_t>(cdiv(N, kConfT / 64), cus);
        hipLaunchKernelGGL(confusion_private, dim3(static_cast<unsigned>(grid)), dim3(kConfT), static_cast<size_t>(12 * C * C), stream, logits, N, C, y,
                           m0, m1, m2, out);
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_edge_class_variant_set(int code) {
    SGS_REQUIRE(code >= 0 && code <= 2, SGS_EINVAL, "sgs_edge_class_variant_set: code %d, need 0 (automatic), 1 (direct) or 2 (privatised)", code);
    g_pair_variant.store(code);
    return SGS_OK;
}

int sgs_edge_class_variant(int64_t n, int64_t C) {
    if (n < 0 || C < 1) return -1;
    if (n == 0) return 0;
    const bool priv_ok = C <= kPairPrivMaxC && n < (int64_t(1) << 31);
    switch (g_pair_variant.load()) {
        case 1: return 1;
        case 2: return priv_ok ? 2 : -1;
        default: return priv_ok ? 2 : 1;          // by capability alone
    }
}

int sgs_edge_class_counts(const int64_t* edge_index, int64_t n, const uint8_t* mask, const int64_t* y, int64_t N, int64_t C, int64_t* pairs,
                          sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n >= 0 && N >= 0 && C >= 1 && C < (int64_t(1) << 24), SGS_EINVAL, "sgs_edge_class_counts: bad sizes (n=%lld N=%lld C=%lld)",
                (long long)n, (long long)N, (long long)C);
    const int var = sgs_edge_class_variant(n, C);
    SGS_REQUIRE(var >= 0, SGS_EINVAL, "sgs_edge_class_counts: the privatised form (forced by sgs_edge_class_variant_set(2)) needs C <= 128 and n < 2^31");
    if (n == 0) return SGS_OK;
    SGS_REQUIRE(edge_index && pairs && (N == 0 || y), SGS_EINVAL, "sgs_edge_class_counts: null pointer");
    unsigned long long* out = reinterpret_cast<unsigned long long*>(pairs);
    if (var == 1) {
        hipLaunchKernelGGL(edge_class_direct, dim3(static_cast<unsigned>(cdiv(n, kT))), dim3(kT), 0, stream, edge_index, n, mask, y, N, C, out);
    } else {
        static const int cus = [] {
            int dev = 0, k = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&k, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || k < 1) k = 256;
            return k;
        }();
        const int64_t grid = std::min<int64_t>(cdiv(n, kConfT), cus);
        hipLaunchKernelGGL(edge_class_private, dim3(static_cast<unsigned>(grid)), dim3(kConfT), static_cast<size_t>(4 * C * C), stream, edge_index, n,
                           mask, y, N, C, out);
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}

}  // extern "C"
