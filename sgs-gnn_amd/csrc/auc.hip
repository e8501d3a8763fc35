// Exact ROC-AUC counts on the device (evaluate.py: args.sgs_eval_auc / args.sgs_eval_auc_report; contract: include/sgs_hip.h).
//
// sgs_auc_pack turns a score matrix [N, S] into one 64-bit key per (row, column) item:
//     bits 0-2 the three split masks | bit 3 positive | bits 4-35 the order-preserving image of the fp32 score | bits 36.. the column
// sgs_auc_counts sorts any concatenation of such keys on bits [4, 36 + ceil(log2 S)) (the library radix sort, csrc/graph_sort.hip: stable,
// the flag bits ride along) and then makes ONE streaming pass over the sorted keys in tiles of kTile items.  With G_s(k) the number of
// split-s negatives among sorted positions 0..k, a positive item i of split s and column c whose tie run (equal column and score) spans
// positions [b, e] has   2 #{negatives below} + #{negatives tied} = (G_s(e) - base_s(c)) + (G_s(b - 1) - base_s(c)),
// base_s(c) = G_s(first position of column c - 1) = the sum of Nn over the columns before c.  So the pass is
//     auc_tile_counts : per tile, the negatives per split                                   (one read of the keys)
//     auc_scan3       : exclusive scan over the tiles, per split                            (in place; entry n_tiles = the total)
//     auc_rank        : per tile the inclusive in-tile prefix, every positive item's run [b, e] and  A += G(e) + G(b - 1), P += 1,
//                       Nn += 1 per negative, into out[s][c]                                 (second read of the keys)
//     auc_finish      : base_s(c) by a scan of Nn over the columns;  twoU = A - 2 P base
// A run that reaches a tile edge is closed by ONE lookup per tile edge, never per item: a search in the sorted keys for where the run
// really starts (ends; block_bound), then the scanned count of that position's tile plus one partial-tile count by the whole workgroup.  Its
// cost is O(log n + kTile) whatever the run's length (confident predictions give runs of 1e5 and more equal scores at log p = -0.0).
// Everything is integer arithmetic (unsigned 64-bit, wrap allowed in A: the result fits); sums across workgroups are integer atomic adds,
// so the result does not depend on arrival order and two calls give the same bits.
#include "sgs_common.h"

namespace sgs {
namespace {
constexpr int kT = 256;                 // threads per workgroup
constexpr int kI = 8;                   // consecutive sorted items per thread
constexpr int kTile = kT * kI;          // items per workgroup of the rank-sum pass (sgs_auc_block_items)
constexpr int kScoreShift = 4, kColShift = 36;
constexpr int kMaxS = 65536;
constexpr int kF = 21;                  // three per-split counts of at most kTile packed into one 64-bit word, 21 bits each
constexpr uint64_t kFMask = (uint64_t(1) << kF) - 1;
using u64 = unsigned long long;

int col_bits(int64_t S) {
    int b = 0;
    while ((int64_t(1) << b) < S) ++b;
    return b;
}

// ---------------------------------------------------------------- pack
__device__ __forceinline__ uint32_t order_image(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;                                      // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(kT) auc_pack(const float* __restrict__ scores, int64_t n, int64_t S, int64_t C, const int64_t* __restrict__ y,
                                               const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2,
                                               uint64_t* __restrict__ keys) {
    for (int64_t idx = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x; idx < n; idx += static_cast<int64_t>(gridDim.x) * kT) {
        const int64_t i = idx / S, c = idx - i * S;
        const float x = scores[idx];
        const int64_t yi = y[i];                                       // compared only, never an index
        const int64_t target = (S == 1) ? 1 : c;
        uint64_t m = (m0[i] != 0 ? 1u : 0u) | (m1[i] != 0 ? 2u : 0u) | (m2[i] != 0 ? 4u : 0u);
        if (yi < 0 || yi >= C || x != x) m = 0;                        // label outside [0, C) or a NaN score: the item is in no split
        const uint64_t pos = (yi == target) ? 8u : 0u;
        keys[idx] = (static_cast<uint64_t>(c) << kColShift) | (static_cast<uint64_t>(order_image(x)) << kScoreShift) | pos | m;
    }
}

// ---------------------------------------------------------------- rank sum
// one word holding, per split, whether the item is a NEGATIVE of that split
__device__ __forceinline__ uint64_t neg_word(uint64_t key) {
    if (key & 8u) return 0;
    return (key & 1u) | (((key >> 1) & 1u) << kF) | (((key >> 2) & 1u) << (2 * kF));
}
__device__ __forceinline__ uint64_t field(uint64_t w, int s) { return (w >> (s * kF)) & kFMask; }

// Exclusive scan of one 64-bit value per thread over the workgroup (kT threads); *total = the sum over all threads.  `ws` needs kT / 64 + 1
// words.  Every thread must call it.
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* ws, uint64_t* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) ws[wid] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int w = 0; w < kT / 64; ++w) {
            const uint64_t t = ws[w];
            ws[w] = run;
            run += t;
        }
        ws[kT / 64] = run;
    }
    __syncthreads();
    const uint64_t r = ws[wid] + inc - v;
    *total = ws[kT / 64];
    __syncthreads();                                                   // ws may be reused at once
    return r;
}

// tile_cnt [3][nt1] (split-major, nt1 = n_tiles + 1): the negatives of every tile; entry n_tiles = 0 (auc_scan3 turns it into the total)
__global__ void __launch_bounds__(kT) auc_tile_counts(const uint64_t* __restrict__ keys, int64_t n, int64_t nt1, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint64_t ws[kT / 64 + 1];
    const int64_t start = static_cast<int64_t>(blockIdx.x) * kTile;
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < kI; ++j) {
        const int64_t p = start + j * kT + threadIdx.x;
        if (p < n) w += neg_word(keys[p]);
    }
    uint64_t total;
    block_excl_scan(w, ws, &total);
    if (threadIdx.x < 3) {
        tile_cnt[threadIdx.x * nt1 + blockIdx.x] = static_cast<uint32_t>(field(total, threadIdx.x));
        if (blockIdx.x == 0) tile_cnt[threadIdx.x * nt1 + (nt1 - 1)] = 0u;
    }
}

// blockIdx.x = split: exclusive scan of tile_cnt[split][0 .. nt1) in place (a chunk of consecutive entries per thread)
__global__ void __launch_bounds__(kT) auc_scan3(uint32_t* __restrict__ tile_cnt, int64_t nt1) {
    __shared__ uint64_t ws[kT / 64 + 1];
    uint32_t* a = tile_cnt + static_cast<int64_t>(blockIdx.x) * nt1;
    const int64_t chunk = (nt1 + kT - 1) / kT, lo = chunk * threadIdx.x, hi = (lo + chunk < nt1) ? lo + chunk : nt1;
    uint64_t sum = 0;
    for (int64_t k = lo; k < hi; ++k) sum += a[k];
    uint64_t total;
    uint64_t run = block_excl_scan(sum, ws, &total);
    for (int64_t k = lo; k < hi; ++k) {
        const uint32_t t = a[k];
        a[k] = static_cast<uint32_t>(run);
        run += t;
    }
}

// LDS index of tile item k: one pad word per kI items, so that the kI consecutive items a thread owns start on different banks
__device__ __forceinline__ int ph(int k) { return k + (k >> 3); }
static_assert(kI == 8, "ph() pads once per 8 items");

// negatives per split among sorted positions [0, x), 0 <= x <= n, by the whole workgroup: the scanned count of x's tile plus a partial count
__device__ __forceinline__ void prefix_at(const uint64_t* __restrict__ keys, int64_t x, const uint32_t* __restrict__ tile_base, int64_t nt1,
                                          uint64_t* ws, uint64_t out[3]) {
    const int64_t tq = x / kTile, lo = tq * kTile;                     // tq <= n_tiles = nt1 - 1; [lo, x) has fewer than kTile items
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < kI; ++j) {
        const int64_t p = lo + j * kT + threadIdx.x;
        if (p < x) w += neg_word(keys[p]);
    }
    uint64_t total;
    block_excl_scan(w, ws, &total);
#pragma unroll
    for (int s = 0; s < 3; ++s) out[s] = tile_base[s * nt1 + tq] + field(total, s);
}

// First position p in [lo, hi) of the sorted keys whose sort bits are >= v (UPPER: > v), or hi if there is none -- by the whole workgroup:
// every round all kT threads probe evenly spaced positions at once and the range shrinks kT-fold, so a search over 2^31 keys is four
// dependent loads deep where one thread's bisection would be thirty-one.  Every thread must call it with the same arguments.
template <bool UPPER>
__device__ __forceinline__ int64_t block_bound(const uint64_t* __restrict__ keys, int64_t lo, int64_t hi, uint64_t v) {
    while (lo < hi) {
        const int64_t step = (hi - lo + kT - 1) / kT, p = lo + step * threadIdx.x;
        int before = 0;                                                // is the bound beyond p?  true for the probes up to some thread, false after
        if (p < hi) {
            const uint64_t k = keys[p] >> kScoreShift;
            before = UPPER ? (k <= v) : (k < v);
        }
        const int64_t nb = __syncthreads_count(before);                // probes 0 .. nb - 1 lie before the bound, probe nb (if in range) does not
        if (nb == 0) return lo;
        const int64_t top = lo + nb * step;
        lo += (nb - 1) * step + 1;
        hi = (top < hi) ? top : hi;
    }
    return lo;
}

__device__ __forceinline__ void add_cell(u64* __restrict__ out, int64_t S, int s, int64_t c, uint64_t A, uint64_t P, uint64_t Nn) {
    u64* cell = out + (static_cast<int64_t>(s) * S + c) * 3;
    if (A) atomicAdd(cell, static_cast<u64>(A));
    if (P) atomicAdd(cell + 1, static_cast<u64>(P));
    if (Nn) atomicAdd(cell + 2, static_cast<u64>(Nn));
}

// out [3][S][3] (zero on entry): {A, P, Nn} per (split, column); auc_finish turns A into twoU
__global__ void __launch_bounds__(kT) auc_rank(const uint64_t* __restrict__ keys, int64_t n, int64_t S, const uint32_t* __restrict__ tile_base,
                                               int64_t nt1, u64* __restrict__ out) {
    __shared__ uint64_t sk[kTile + kTile / 8];                         // the tile's keys
    __shared__ uint64_t pre[kTile + kTile / 8];                        // inclusive in-tile count of negatives, three packed fields
    __shared__ uint64_t ws[kT / 64 + 1];
    __shared__ int edge[2];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x, start = t * kTile;
    const int cnt = static_cast<int>((n - start < kTile) ? n - start : kTile);        // >= 1: the grid has cdiv(n, kTile) workgroups
    constexpr uint64_t kPad = ~uint64_t(0) << kScoreShift;             // past the end: above every key, in no split
#pragma unroll
    for (int j = 0; j < kI; ++j) {
        const int k = j * kT + tid;
        sk[ph(k)] = (k < cnt) ? keys[start + k] : kPad;
    }
    __syncthreads();
    uint64_t mine[kI];
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < kI; ++j) {
        mine[j] = sk[ph(tid * kI + j)];
        w += neg_word(mine[j]);
    }
    uint64_t tile_total;
    uint64_t run = block_excl_scan(w, ws, &tile_total);
#pragma unroll
    for (int j = 0; j < kI; ++j) {
        run += neg_word(mine[j]);
        pre[ph(tid * kI + j)] = run;
    }
    // the two tile edges: does the first (last) item's run go on in the neighbouring tile, and if so where does it start (end)
    const uint64_t first = sk[ph(0)] >> kScoreShift, last = sk[ph(cnt - 1)] >> kScoreShift;
    const int64_t end = start + cnt;
    if (tid == 0) {
        edge[0] = (start > 0 && (keys[start - 1] >> kScoreShift) == first) ? 1 : 0;
        edge[1] = (end < n && (keys[end] >> kScoreShift) == last) ? 1 : 0;
    }
    __syncthreads();
    uint64_t base[3], GL[3], GR[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        base[s] = tile_base[s * nt1 + t];
        GL[s] = base[s];                                               // G(start - 1)
        GR[s] = base[s] + field(tile_total, s);                        // G(start + cnt - 1)
    }
    const bool cross_left = edge[0] != 0, cross_right = edge[1] != 0;  // the same in every thread: both branches are workgroup-uniform
    if (cross_left)                                                    // G(run start - 1) of the run that enters from the left; keys[start - 1] is in it
        prefix_at(keys, block_bound<false>(keys, 0, start - 1, first), tile_base, nt1, ws, GL);
    if (cross_right)                                                   // G(run end) of the run that leaves to the right; keys[end] is in it
        prefix_at(keys, block_bound<true>(keys, end + 1, n, last), tile_base, nt1, ws, GR);

    const int64_t col_first = static_cast<int64_t>(sk[ph(0)] >> kColShift), col_last = static_cast<int64_t>(sk[ph(cnt - 1)] >> kColShift);
    const bool one_column = col_first == col_last;
    uint64_t A[3] = {0, 0, 0}, Pn = 0, Nn = 0;                          // Pn, Nn: three packed fields
    int64_t cur = col_first;
#pragma unroll
    for (int j = 0; j < kI; ++j) {                                     // (unrolled: mine[] stays in registers)
        const int k = tid * kI + j;
        if (k >= cnt) break;
        const uint64_t key = mine[j];
        const int64_t c = static_cast<int64_t>(key >> kColShift);
        if (c != cur) {                                                // only in a tile that holds several columns
            if (cur < S)
                for (int s = 0; s < 3; ++s) add_cell(out, S, s, cur, A[s], field(Pn, s), field(Nn, s));
            A[0] = A[1] = A[2] = Pn = Nn = 0;
            cur = c;
        }
        const uint32_t m = static_cast<uint32_t>(key & 7u);
        if (m == 0) continue;
        if (!(key & 8u)) {
            Nn += neg_word(key);
            continue;
        }
        const uint64_t v = key >> kScoreShift;
        int lo = 0, hi = k;                                            // b: first item of the tile whose (column, score) equals mine
        if (k > 0 && (sk[ph(k - 1)] >> kScoreShift) != v) lo = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((sk[ph(mid)] >> kScoreShift) < v) lo = mid + 1; else hi = mid;
        }
        const int b = lo;
        lo = k + 1;
        hi = cnt;                                                      // e + 1: first item after mine with a larger one, or cnt
        if (k + 1 < cnt && (sk[ph(k + 1)] >> kScoreShift) != v) hi = k + 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((sk[ph(mid)] >> kScoreShift) <= v) lo = mid + 1; else hi = mid;
        }
        const int e = lo - 1;
        const uint64_t pb = (b > 0) ? pre[ph(b - 1)] : 0, pe = pre[ph(e)];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (!((m >> s) & 1u)) continue;
            const uint64_t Gb = (b == 0) ? GL[s] : base[s] + field(pb, s);
            const uint64_t Ge = (e == cnt - 1) ? GR[s] : base[s] + field(pe, s);
            A[s] += Ge + Gb;
            Pn += uint64_t(1) << (s * kF);
        }
    }
    if (!one_column) {
        if (cur < S)
            for (int s = 0; s < 3; ++s) add_cell(out, S, s, cur, A[s], field(Pn, s), field(Nn, s));
        return;                                                        // (workgroup-uniform: no barrier follows for anyone)
    }
    // the usual tile, all of one column: one set of adds per workgroup
    uint64_t tA[3], tP, tN;
    block_excl_scan(A[0], ws, &tA[0]);
    block_excl_scan(A[1], ws, &tA[1]);
    block_excl_scan(A[2], ws, &tA[2]);
    block_excl_scan(Pn, ws, &tP);
    block_excl_scan(Nn, ws, &tN);
    if (tid < 3 && col_first < S) add_cell(out, S, tid, col_first, tA[tid], field(tP, tid), field(tN, tid));
}

// blockIdx.x = split: base(c) = the negatives of the columns before c;  out[s][c][0] = A - 2 P base(c)
__global__ void __launch_bounds__(kT) auc_finish(u64* __restrict__ out, int64_t S) {
    __shared__ uint64_t ws[kT / 64 + 1];
    u64* a = out + static_cast<int64_t>(blockIdx.x) * S * 3;
    const int64_t chunk = (S + kT - 1) / kT, lo = chunk * threadIdx.x, hi = (lo + chunk < S) ? lo + chunk : S;
    uint64_t sum = 0;
    for (int64_t c = lo; c < hi; ++c) sum += a[3 * c + 2];
    uint64_t total;
    uint64_t base = block_excl_scan(sum, ws, &total);
    for (int64_t c = lo; c < hi; ++c) {
        a[3 * c] -= 2 * a[3 * c + 1] * base;
        base += a[3 * c + 2];
    }
}

struct CountsLayout {
    size_t sorted, temp, tiles, total;
    int64_t nt1;
    size_t temp_bytes;
};
CountsLayout counts_layout(int64_t n, int64_t S) {
    CountsLayout L{};
    L.nt1 = cdiv(n, kTile) + 1;
    L.temp_bytes = auc_sort_temp_bytes(n, kScoreShift, kColShift + col_bits(S));
    L.sorted = carve_bytes(static_cast<size_t>(n) + 1, 8);
    L.temp = carve_bytes(L.temp_bytes + 256, 1);
    L.tiles = carve_bytes(3 * static_cast<size_t>(L.nt1), 4);
    L.total = L.sorted + L.temp + L.tiles + 256;
    return L;
}
}  // namespace
}  // namespace sgs

extern "C" {
int64_t sgs_auc_block_items(void) { return sgs::kTile; }

int sgs_auc_pack(const float* scores, int64_t N, int64_t S, int64_t C, const int64_t* y, const uint8_t* m0, const uint8_t* m1, const uint8_t* m2,
                 uint64_t* keys, sgs_stream_t stream) {
    using namespace sgs;
    SGS_REQUIRE(N >= 0 && S >= 1 && S <= kMaxS && ((C == 2 && S == 1) || (C > 2 && S == C)), SGS_EINVAL,
                "sgs_auc_pack: bad arguments (N = %lld, S = %lld, C = %lld): need N >= 0 and S = 1 with C = 2, or S = C with 2 < C <= %d",
                (long long)N, (long long)S, (long long)C, kMaxS);
    SGS_REQUIRE(N < (int64_t(1) << 31) / S, SGS_EINVAL, "sgs_auc_pack: N * S = %lld * %lld, need fewer than 2^31 items", (long long)N, (long long)S);
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(scores && y && m0 && m1 && m2 && keys, SGS_EINVAL, "sgs_auc_pack: null pointer");
    const int64_t n = N * S;
    const int64_t grid = cdiv(n, kT) < 16384 ? cdiv(n, kT) : 16384;
    hipLaunchKernelGGL(auc_pack, dim3(static_cast<unsigned>(grid)), dim3(kT), 0, static_cast<hipStream_t>(stream), scores, n, S, C, y, m0, m1, m2, keys);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_auc_counts_workspace_bytes(int64_t n, int64_t S) {
    using namespace sgs;
    if (n <= 0 || n >= (int64_t(1) << 31) || S < 1 || S > kMaxS) return 256;
    return counts_layout(n, S).total;
}

int sgs_auc_counts(const uint64_t* keys, int64_t n, int64_t S, int64_t* out, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    using namespace sgs;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && S >= 1 && S <= kMaxS, SGS_EINVAL,
                "sgs_auc_counts: bad arguments (n = %lld, S = %lld): need 0 <= n < 2^31 and 1 <= S <= %d", (long long)n, (long long)S, kMaxS);
    SGS_REQUIRE(out, SGS_EINVAL, "sgs_auc_counts: null pointer (out)");
    if (int rc = zero_async(out, static_cast<size_t>(S) * 9 * 8, stream)) return rc;
    if (n == 0) {
        SGS_LAUNCH_OK();
        return SGS_OK;
    }
    SGS_REQUIRE(keys && ws, SGS_EINVAL, "sgs_auc_counts: null pointer");
    const CountsLayout L = counts_layout(n, S);
    SGS_REQUIRE(ws_bytes >= L.total, SGS_EWORKSPACE, "sgs_auc_counts: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    Carver cv(ws);
    uint64_t* sorted = cv.take<uint64_t>(static_cast<size_t>(n) + 1);
    void* temp = cv.take<char>(L.temp_bytes + 256);
    uint32_t* tiles = cv.take<uint32_t>(3 * static_cast<size_t>(L.nt1));
    if (int rc = auc_sort_keys(keys, sorted, n, kScoreShift, kColShift + col_bits(S), temp, L.temp_bytes, stream)) return rc;
    const dim3 gt(static_cast<unsigned>(L.nt1 - 1)), blk(kT);
    hipLaunchKernelGGL(auc_tile_counts, gt, blk, 0, stream, sorted, n, L.nt1, tiles);
    hipLaunchKernelGGL(auc_scan3, dim3(3), blk, 0, stream, tiles, L.nt1);
    hipLaunchKernelGGL(auc_rank, gt, blk, 0, stream, sorted, n, S, tiles, L.nt1, reinterpret_cast<u64*>(out));
    hipLaunchKernelGGL(auc_finish, dim3(3), blk, 0, stream, reinterpret_cast<u64*>(out), S);
    SGS_LAUNCH_OK();
    return SGS_OK;
}
}
