// Device partitioner kernels (partition.py: partition_graph; contract: include/sgs_hip.h): the sweep of a balanced k-way label
// propagation -- every node tallies the parts of its neighbours and proposes the best other part (sgs_lp_propose), a two-sided
// capacity-constrained commit accepts a deterministic subset of the proposals (sgs_lp_commit) -- and the cut / size statistics
// (sgs_partition_stats).  Everything is integer arithmetic: the tally is a count, the commit an order on 64-bit keys, the sums across
// workgroups integer atomic adds, so the result does not depend on arrival order and equals tests/partition_ref.py element for element.
//
// sgs_lp_propose: one WAVE per row with a private slab of P 32-bit counters in LDS (kWaves slabs per workgroup, dynamic LDS = kWaves * 4 P
// bytes: 64 KiB at P = 4096, i.e. two workgroups = eight waves per CU there, and up to the wave limit below P = 1024).  Lanes stride the row and
// do a RETURNING LDS add on counter[part[col]]; every returned old + 1 is a candidate (count, p) for the lane's running maximum under (count
// descending, p ascending).  The final count of every part is among the candidates and no candidate exceeds it, so a wave reduction gives the
// exact argmax whatever order the adds landed in.  The node's own part is counted but never a candidate; its count is read back after the
// pass.  Afterwards the touched counters alone are zeroed, so nothing of size P is cleared per row (the slabs are zeroed once per workgroup,
// which then walks row tiles in a grid-stride loop): a lane keeps kHeld entries in registers -- their column loads and then their part
// gathers are all in flight before the first add -- so a row of up to kHeld * 64 entries is zeroed from the registers, and only a longer
// one is read a second time.  The kernel is latency-bound (a wave's rows are dependent chains walked one after the other; DESIGN.md
// section 5 "Partitioner" has the measured share of the bandwidth floor).  A row longer than kHubRow entries is left to the END of its tile, where all
// kWaves waves walk it together on slab 0 (a hub of 3e5 entries would otherwise hold one wave for 2 x 4700 iterations while its
// workgroup's other waves idle).
#include "sgs_common.h"

namespace sgs {
namespace {
constexpr int kT = 256;
constexpr int kWaves = kT / kWave;          // rows per tile of sgs_lp_propose
constexpr int kHeld = 8;                    // entries per lane the one-wave form keeps in registers (rows up to 512 entries are read once)
constexpr int kHubRow = 2048;              // a row with more stored entries than this is walked by the whole workgroup
constexpr int kMaxParts = 4096;
constexpr int kGainBits = 20, kNodeBits = 31, kPartShift = kGainBits + kNodeBits;      // key = part << 51 | (2^20 - 1 - gain) << 31 | v
constexpr uint32_t kGainMax = (1u << kGainBits) - 1;
constexpr uint64_t kLowMask = (uint64_t(1) << kPartShift) - 1;
using u64 = unsigned long long;

// (count, part) candidates packed so that "better" is "larger": count in the high word, ~part in the low one; 0 = no candidate
__device__ __forceinline__ u64 cand(uint32_t count, uint32_t p) { return (static_cast<u64>(count) << 32) | (0xFFFFFFFFu - p); }
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// tally the entries [beg + first, end) of row v with stride `step` into `cnt`; -> the thread's best candidate
// (a column outside [0, N) or a part outside [0, P) is skipped, never used as an index)
__device__ __forceinline__ u64 tally(const int* __restrict__ col, const int* __restrict__ part, int64_t beg, int64_t end, int first, int step,
                                     int v, int pv, uint32_t* cnt, int64_t N, int P) {
    u64 mine = 0;
    for (int64_t e = beg + first; e < end; e += step) {
        const int u = col[e];
        if (u == v || u < 0 || u >= N) continue;
        const int p = part[u];
        if (p < 0 || p >= P) continue;
        const uint32_t c = atomicAdd(&cnt[p], 1u) + 1u;
        if (p != pv) {
            const u64 k = cand(c, static_cast<uint32_t>(p));
            mine = k > mine ? k : mine;
        }
    }
    return mine;
}
__device__ __forceinline__ void untally(const int* __restrict__ col, const int* __restrict__ part, int64_t beg, int64_t end, int first, int step,
                                        int v, uint32_t* cnt, int64_t N, int P) {
    for (int64_t e = beg + first; e < end; e += step) {
        const int u = col[e];
        if (u == v || u < 0 || u >= N) continue;
        const int p = part[u];
        if (p >= 0 && p < P) cnt[p] = 0u;
    }
}
// the one-wave form's tally of entries first, first + 64, ... (kHeld of them); p[j] = the part counted for entry j, or -1
__device__ __forceinline__ u64 tally_held(const int* __restrict__ col, const int* __restrict__ part, int64_t first, int64_t end, int v, int pv,
                                          uint32_t* cnt, int64_t N, int P, int (&p)[kHeld]) {
    int u[kHeld];
#pragma unroll
    for (int j = 0; j < kHeld; ++j) {
        const int64_t e = first + j * kWave;
        u[j] = e < end ? col[e] : -1;
    }
#pragma unroll
    for (int j = 0; j < kHeld; ++j) p[j] = (u[j] >= 0 && u[j] < N && u[j] != v) ? part[u[j]] : -1;
    u64 mine = 0;
#pragma unroll
    for (int j = 0; j < kHeld; ++j) {
        if (p[j] < 0 || p[j] >= P) {
            p[j] = -1;
            continue;
        }
        const uint32_t c = atomicAdd(&cnt[p[j]], 1u) + 1u;
        if (p[j] != pv) {
            const u64 k = cand(c, static_cast<uint32_t>(p[j]));
            mine = k > mine ? k : mine;
        }
    }
    return mine;
}
__device__ __forceinline__ void emit(u64 top, uint32_t own, int mingain, int v, int* __restrict__ best, int* __restrict__ gain) {
    int b = -1, g = 0;
    if (top != 0) {
        const int64_t d = static_cast<int64_t>(top >> 32) - static_cast<int64_t>(own);
        if (d >= mingain) {
            b = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(top));
            g = static_cast<int>(d);
        }
    }
    best[v] = b;
    gain[v] = g;
}
__device__ __forceinline__ bool is_eligible(int mode, uint32_t hk, int v, int pv) {
    return mode == 0 ? pv < 0 : (fmix32(static_cast<uint32_t>(v) ^ hk) & 1u) != 0u;
}

__global__ void __launch_bounds__(kT) lp_propose(const int* __restrict__ ptr, const int* __restrict__ col, int64_t N, int P,
                                                 const int* __restrict__ part, int mode, uint32_t hk, int mingain, int* __restrict__ best,
                                                 int* __restrict__ gain) {
    extern __shared__ uint32_t slabs[];                                 // [kWaves][P]
    __shared__ u64 wtop[kWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t* cnt = slabs + static_cast<size_t>(wid) * P;
    for (int i = threadIdx.x; i < kWaves * P; i += kT) slabs[i] = 0u;
    __syncthreads();
    const int64_t tiles = (N + kWaves - 1) / kWaves;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {           // the trip count is the same for every wave: barriers below are safe
        const int64_t v64 = t * kWaves + wid;
        if (v64 < N) {
            const int v = static_cast<int>(v64), pv = part[v];
            const int64_t beg = ptr[v], end = ptr[v + 1];
            if (!is_eligible(mode, hk, v, pv)) {
                if (lane == 0) {
                    best[v] = -1;
                    gain[v] = 0;
                }
            } else if (end - beg <= kHubRow) {
                // kHeld entries per lane at a time: their column loads, then their part gathers, are all in flight before the first add
                int p[kHeld];
#pragma unroll
                for (int j = 0; j < kHeld; ++j) p[j] = -1;              // (an empty row runs no pass)
                u64 mine = 0;
                for (int64_t base = beg; base < end; base += kHeld * kWave) {
                    const u64 k = tally_held(col, part, base + lane, end, v, pv, cnt, N, P, p);
                    mine = k > mine ? k : mine;
                }
                const u64 top = wave_max_u64(mine);
                const uint32_t own = (pv >= 0 && pv < P) ? *static_cast<volatile uint32_t*>(cnt + pv) : 0u;      // after every add of this wave
                if (end - beg <= kHeld * kWave) {                       // the whole row is still in registers: no second read of it
#pragma unroll
                    for (int j = 0; j < kHeld; ++j)
                        if (p[j] >= 0) cnt[p[j]] = 0u;
                } else {
                    untally(col, part, beg, end, lane, kWave, v, cnt, N, P);
                }
                if (lane == 0) emit(top, own, mingain, v, best, gain);
            }
        }
        // the tile's hub rows, one after the other, by all waves on slab 0 (every slab is all zero between rows)
        for (int w = 0; w < kWaves; ++w) {
            const int64_t h64 = t * kWaves + w;
            if (h64 >= N) break;
            const int h = static_cast<int>(h64);
            const int64_t beg = ptr[h], end = ptr[h + 1];
            if (end - beg <= kHubRow) continue;
            const int ph = part[h];
            if (!is_eligible(mode, hk, h, ph)) continue;                // (written above by wave w)
            __syncthreads();                                            // wave 0 is done with slab 0; wtop is free
            const u64 top = wave_max_u64(tally(col, part, beg, end, threadIdx.x, kT, h, ph, slabs, N, P));
            if (lane == 0) wtop[wid] = top;
            __syncthreads();
            const uint32_t own = (ph >= 0 && ph < P) ? *static_cast<volatile uint32_t*>(slabs + ph) : 0u;
            __syncthreads();
            untally(col, part, beg, end, threadIdx.x, kT, h, slabs, N, P);
            if (threadIdx.x == 0) {
                u64 all = wtop[0];
                for (int k = 1; k < kWaves; ++k) all = wtop[k] > all ? wtop[k] : all;
                emit(all, own, mingain, h, best, gain);
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- commit
__device__ __forceinline__ uint64_t low_bits(int gain, int v) {
    const uint32_t g = gain < 0 ? 0u : (static_cast<uint32_t>(gain) > kGainMax ? kGainMax : static_cast<uint32_t>(gain));
    return (static_cast<uint64_t>(kGainMax - g) << kNodeBits) | static_cast<uint32_t>(v);
}

// keys_t[v] = the target key of v's proposal, or part field = P (sorts behind every real key); keys_s[v] = the same filler; accept = 0
__global__ void __launch_bounds__(kT) lp_keys(const int* __restrict__ best, const int* __restrict__ gain, int64_t N, int P,
                                              uint64_t* __restrict__ keys_t, uint64_t* __restrict__ keys_s, uint8_t* __restrict__ accept,
                                              int* __restrict__ moved) {
    const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (v == 0) *moved = 0;
    if (v >= N) return;
    const int b = best[v];
    const uint64_t none = (static_cast<uint64_t>(P) << kPartShift) | static_cast<uint32_t>(v);
    keys_t[v] = (b >= 0 && b < P) ? (static_cast<uint64_t>(b) << kPartShift) | low_bits(gain[v], static_cast<int>(v)) : none;
    keys_s[v] = none;
    accept[v] = 0;
}

// rank of sorted position i within its part's run = i - (first position whose part field is >= the part's)
__device__ __forceinline__ int64_t run_rank(const uint64_t* __restrict__ sorted, int64_t N, int64_t i, uint64_t p) {
    int64_t lo = 0, hi = i;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((sorted[mid] >> kPartShift) < p) lo = mid + 1; else hi = mid;
    }
    return i - lo;
}

// by TARGET: the first max(cap - size[t], 0) proposals of every target survive; a survivor with a source part gets a source key, one without
// is accepted at once
__global__ void __launch_bounds__(kT) lp_rank_target(const uint64_t* __restrict__ sorted, int64_t N, int P, const int* __restrict__ size,
                                                     int64_t cap, const int* __restrict__ part, uint64_t* __restrict__ keys_s,
                                                     uint8_t* __restrict__ accept) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (i >= N) return;
    const uint64_t key = sorted[i], t = key >> kPartShift;
    if (t >= static_cast<uint64_t>(P)) return;
    const int64_t room = cap - size[t];
    if (run_rank(sorted, N, i, t) >= room) return;
    const int64_t v = static_cast<int64_t>(key & ((uint64_t(1) << kNodeBits) - 1));
    if (v >= N) return;
    const int s = part[v];
    if (s < 0 || s >= P) accept[v] = 1;
    else keys_s[v] = (static_cast<uint64_t>(s) << kPartShift) | (key & kLowMask);
}
// by SOURCE: the first max(size[s] - lo, 0) survivors of every source are accepted
__global__ void __launch_bounds__(kT) lp_rank_source(const uint64_t* __restrict__ sorted, int64_t N, int P, const int* __restrict__ size,
                                                     int64_t lo, uint8_t* __restrict__ accept) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (i >= N) return;
    const uint64_t key = sorted[i], s = key >> kPartShift;
    if (s >= static_cast<uint64_t>(P)) return;
    const int64_t spare = static_cast<int64_t>(size[s]) - lo;
    if (run_rank(sorted, N, i, s) >= spare) return;
    const int64_t v = static_cast<int64_t>(key & ((uint64_t(1) << kNodeBits) - 1));
    if (v < N) accept[v] = 1;
}
__global__ void __launch_bounds__(kT) lp_apply(const int* __restrict__ best, const uint8_t* __restrict__ accept, int64_t N, int P,
                                               int* __restrict__ part, int* __restrict__ size, int* __restrict__ moved) {
    const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    int m = 0;
    if (v < N && accept[v]) {
        const int s = part[v], b = best[v];
        part[v] = b;
        atomicAdd(&size[b], 1);
        if (s >= 0 && s < P) atomicSub(&size[s], 1);
        m = 1;
    }
    m = wave_sum_int_all(m);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(moved, m);
}

int part_bits(int64_t P) {                                              // bits that hold the values 0 .. P
    int b = 1;
    while ((int64_t(1) << b) <= P) ++b;
    return b;
}

struct CommitLayout {
    size_t keys, accept, temp, total, temp_bytes;
};
CommitLayout commit_layout(int64_t N, int64_t P) {
    CommitLayout L{};
    L.temp_bytes = auc_sort_temp_bytes(N, 0, kPartShift + part_bits(P));
    L.keys = carve_bytes(static_cast<size_t>(N) + 1, 8);
    L.accept = carve_bytes(static_cast<size_t>(N) + 4, 1);
    L.temp = carve_bytes(L.temp_bytes + 256, 1);
    L.total = 3 * L.keys + L.accept + L.temp + 256;
    return L;
}

// ---------------------------------------------------------------- statistics
// one wave per row over a grid-stride loop; sizes in an LDS table per workgroup, non-zero cells flushed at the end
__global__ void __launch_bounds__(kT) partition_stats(const int* __restrict__ ptr, const int* __restrict__ col, int64_t N, int P,
                                                      const int* __restrict__ part, int* __restrict__ size, u64* __restrict__ cut) {
    extern __shared__ uint32_t hist[];                                  // [P]
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < P; i += kT) hist[i] = 0u;
    __syncthreads();
    u64 mine = 0;
    for (int64_t v = static_cast<int64_t>(blockIdx.x) * kWaves + wid; v < N; v += static_cast<int64_t>(gridDim.x) * kWaves) {
        const int pv = part[v];
        if (lane == 0 && pv >= 0 && pv < P) atomicAdd(&hist[pv], 1u);
        const int64_t end = ptr[v + 1];
        for (int64_t e = ptr[v] + lane; e < end; e += kWave) {
            const int u = col[e];
            if (u != v && u >= 0 && u < N && part[u] != pv) ++mine;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(cut, mine);
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += kT)
        if (hist[i]) atomicAdd(&size[i], static_cast<int>(hist[i]));
}

int check_shape(const char* who, int64_t N, int64_t nnz, int64_t P) {
    SGS_REQUIRE(N >= 0 && nnz >= 0 && N < (int64_t(1) << 31) && nnz < (int64_t(1) << 31), SGS_EINVAL,
                "%s: bad sizes (N = %lld, nnz = %lld): need 0 <= N, nnz < 2^31", who, (long long)N, (long long)nnz);
    SGS_REQUIRE(P >= 1 && P <= kMaxParts, SGS_EINVAL, "%s: P = %lld outside [1, %d]", who, (long long)P, kMaxParts);
    SGS_REQUIRE(P <= N, SGS_EINVAL, "%s: P = %lld parts for N = %lld nodes (need P <= N)", who, (long long)P, (long long)N);
    return SGS_OK;
}
int64_t grid_for(int64_t tiles) { return tiles < 2048 ? (tiles < 1 ? 1 : tiles) : 2048; }    // 256 CUs x 8 resident workgroups at small P
}  // namespace
}  // namespace sgs

extern "C" {
int64_t sgs_lp_propose_hub_row(void) { return sgs::kHubRow; }

int sgs_lp_propose(const int32_t* ptr, const int32_t* col, int64_t N, int64_t nnz, int64_t P, const int32_t* part, int eligible, uint32_t hash_key,
                   int mingain, int32_t* best, int32_t* gain, sgs_stream_t stream) {
    using namespace sgs;
    if (int rc = check_shape("sgs_lp_propose", N, nnz, P)) return rc;
    SGS_REQUIRE(eligible == 0 || eligible == 1, SGS_EINVAL, "sgs_lp_propose: eligible = %d, need 0 (unassigned nodes) or 1 (hash bit)", eligible);
    SGS_REQUIRE(ptr && part && best && gain && (col || nnz == 0), SGS_EINVAL, "sgs_lp_propose: null pointer");
    const size_t lds = static_cast<size_t>(kWaves) * static_cast<size_t>(P) * 4;
    if (lds > 32768)                                                    // up to 64 KiB of dynamic LDS on top of the static words
        SGS_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(lp_propose), hipFuncAttributeMaxDynamicSharedMemorySize, kWaves * kMaxParts * 4));
    hipLaunchKernelGGL(lp_propose, dim3(static_cast<unsigned>(grid_for(cdiv(N, kWaves)))), dim3(kT), lds, static_cast<hipStream_t>(stream), ptr, col, N,
                       static_cast<int>(P), part, eligible, fmix32(hash_key), mingain, best, gain);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_lp_commit_workspace_bytes(int64_t N, int64_t P) {
    using namespace sgs;
    if (N <= 0 || N >= (int64_t(1) << 31) || P < 1 || P > kMaxParts) return 256;
    return commit_layout(N, P).total;
}

int sgs_lp_commit(const int32_t* best, const int32_t* gain, int64_t N, int64_t P, int64_t cap, int64_t lo, int32_t* part, int32_t* size,
                  int32_t* moved, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    using namespace sgs;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = check_shape("sgs_lp_commit", N, 0, P)) return rc;
    SGS_REQUIRE(cap >= 0 && lo >= 0, SGS_EINVAL, "sgs_lp_commit: negative bound (cap = %lld, lo = %lld)", (long long)cap, (long long)lo);
    SGS_REQUIRE(best && gain && part && size && moved && ws, SGS_EINVAL, "sgs_lp_commit: null pointer");
    const CommitLayout L = commit_layout(N, P);
    SGS_REQUIRE(ws_bytes >= L.total, SGS_EWORKSPACE, "sgs_lp_commit: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    Carver cv(ws);
    uint64_t* keys_t = cv.take<uint64_t>(static_cast<size_t>(N) + 1);
    uint64_t* keys_s = cv.take<uint64_t>(static_cast<size_t>(N) + 1);
    uint64_t* sorted = cv.take<uint64_t>(static_cast<size_t>(N) + 1);
    uint8_t* accept = cv.take<uint8_t>(static_cast<size_t>(N) + 4);
    void* temp = cv.take<char>(L.temp_bytes + 256);
    const int end_bit = kPartShift + part_bits(P);
    const dim3 grid(static_cast<unsigned>(cdiv(N, kT))), blk(kT);
    hipLaunchKernelGGL(lp_keys, grid, blk, 0, stream, best, gain, N, static_cast<int>(P), keys_t, keys_s, accept, moved);
    // The sorts run over ALL bits from 0 up, although the keys are written in ascending v and a stable sort on the bits above v's would do:
    // below its merge-sort limit the library compares through a mask built as (1 << end_bit) - 1, which is wrong for end_bit = 64 with a
    // begin_bit above 0 (P = 4096 puts the filler's part field in bit 63); from bit 0 it compares whole keys, and they are distinct.
    if (int rc = auc_sort_keys(keys_t, sorted, N, 0, end_bit, temp, L.temp_bytes, stream)) return rc;
    hipLaunchKernelGGL(lp_rank_target, grid, blk, 0, stream, sorted, N, static_cast<int>(P), size, cap, part, keys_s, accept);
    if (int rc = auc_sort_keys(keys_s, sorted, N, 0, end_bit, temp, L.temp_bytes, stream)) return rc;
    hipLaunchKernelGGL(lp_rank_source, grid, blk, 0, stream, sorted, N, static_cast<int>(P), size, lo, accept);
    hipLaunchKernelGGL(lp_apply, grid, blk, 0, stream, best, accept, N, static_cast<int>(P), part, size, moved);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_partition_stats(const int32_t* ptr, const int32_t* col, int64_t N, int64_t nnz, int64_t P, const int32_t* part, int32_t* size,
                        int64_t* cut, sgs_stream_t stream_) {
    using namespace sgs;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = check_shape("sgs_partition_stats", N, nnz, P)) return rc;
    SGS_REQUIRE(ptr && part && size && cut && (col || nnz == 0), SGS_EINVAL, "sgs_partition_stats: null pointer");
    if (int rc = fill2_async(size, static_cast<size_t>(P) * 4, 0u, cut, 8, 0u, stream)) return rc;
    int64_t grid = cdiv(N, kWaves * 8);                                // eight rows per wave: one flush of the size table per 32 rows at least
    grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
    hipLaunchKernelGGL(partition_stats, dim3(static_cast<unsigned>(grid)), dim3(kT), static_cast<size_t>(P) * 4, stream, ptr, col, N,
                       static_cast<int>(P), part, size, reinterpret_cast<u64*>(cut));
    SGS_LAUNCH_OK();
    return SGS_OK;
}
}
