// Neighbour-sampled batches (data.py: ResidentGraph / NeighborLoader; contract: include/sgs_hip.h; numpy restatement:
// tests/neighbor_ref.py): seeds plus a sampled k-hop in-neighbourhood, built on the device from the whole graph's two CSRs.  Everything is
// integer arithmetic and no result depends on the order in which atomics land, so the batch equals the reference element for element.
//
// SELECTION (sgs_nbr_select): one WAVE per frontier row of the in-CSR.  A row of deg <= f entries (or f = -1) copies its edge ids.  A longer
// row finds the f-th smallest 32-bit key fmix32(edge id ^ K) by a radix select -- four passes of 8-bit digits from the top, a 256-bin histogram
// per wave in LDS, the keys recomputed from the ids in every pass and never stored -- and then emits the ids whose key is not above it in row
// order (ballot + prefix popcount).  Distinct ids have distinct keys (fmix32 is a bijection), so exactly f ids pass.  A row of more than
// kHubRow entries is left to the end of its tile, where the workgroup's four waves walk it together on histogram 0.  A row's output offset is
// the exclusive scan of min(f, deg) over the frontier, from ptr alone (one single-workgroup scan launch before the row kernel).
// WEIGHTED SELECTION (sgs_nbr_select_weighted): the same kernel template with another key.  Edge e with quantised weight wq in [1, 2^24) gets
// key = LOG2Q(-log2 u) - LOG2Q(wq) + 24 * 2^24, u = max(fmix32(e ^ K), 1) / 2^32: the order of -ln(u) / w, an exponential clock, so the f
// smallest keys are f successive draws proportional to the weight, without replacement.  LOG2Q is a 24-bit fixed-point log2 from a 257-word
// table (built at compile time by integer squaring, copied to LDS by every workgroup) with linear interpolation: integers only, the same
// bits as tests/neighbor_weighted_ref.py.  wq = 0 has the key 2^32 - 1.  These keys CAN tie, so the compaction has two parts: every id with
// a key below the f-th smallest, plus the first `k` ids with that key in row order, k = the rank the last radix pass leaves (two ballots per
// step; in the hub form two count rows).  A one-wave row (at most kHubRow keys) computes its keys once, in the first pass, and keeps them in
// LDS for the other three passes and the compaction (8 KiB per wave; measured 17-24 % faster than recomputing them); a hub row recomputes.
// FRONTIER (sgs_nbr_begin / sgs_nbr_frontier): three node bitmaps of ceil(N / 32) words (batch members, reached this hop, seeds).  The sources
// of the chosen edges are OR-ed into `reached` unless already members; one single-workgroup popcount scan over the words then emits the new
// nodes ascending, merges them into the members and clears `reached`.  Nothing is proportional to E, and to N only through the words.
// COLLATE (sgs_nbr_nodes, sgs_nbr_induced_count / _fill, sgs_nbr_directional, sgs_nbr_gather): a node's local id is its rank among the
// members = the popcount prefix of its word + the popcount of the lower bits of that word.  induced: count -> scan -> fill over the out-CSR
// rows of the members -- the row squeeze and the scan of csrc/batch_rows.h, which the cluster collate runs too: one wave per row, a row of
// more than kHubRow entries walked by the workgroup's four waves in slices; here only the policy `InducedRows`.  directional: the chosen ids of all hops sorted (library radix sort) and gathered.
#include "batch_rows.h"

namespace sgs {
namespace {
constexpr int kT = 256;
constexpr int kWaves = kT / kWave;          // frontier rows per tile of nbr_select
constexpr int kHubRow = 2048;               // a row with more entries than this is walked by the whole workgroup
constexpr int kMaxHops = 8;
constexpr int kSortBits = 33;               // edge ids below 2^31, the marker of a skipped id at 2^32
using u64 = unsigned long long;

// ---------------------------------------------------------------- the weighted key
// T[i] = floor(2^24 log2(1 + i / 256)), i = 0 .. 256, by integer squaring: y in [1, 2) as a 2.62 fixed-point number; 24 times y <- y^2 and
// one bit of the logarithm (y >= 2: the bit is set and y is halved).  Every step truncates, so y only ever errs low, by less than 2^-36
// after 24 doublings: a bit would be wrong only where a true y came that close to 2.  tests/neighbor_weighted_ref.py brackets y from both
// sides at 200 bits and finds the same 257 words.
constexpr uint32_t kWqMax = (1u << 24) - 1u, kNoKey = 0xFFFFFFFFu;
struct Log2Table {
    int32_t t[257];
};
constexpr uint64_t square_q62(uint64_t y) {          // y < 2^63 -> floor(y^2 / 2^62) from 32-bit halves
    const uint64_t a = y >> 32, b = y & 0xFFFFFFFFull;
    const uint64_t ab = a * b, mid = ab << 33;
    const uint64_t lo = b * b + mid;
    const uint64_t hi = a * a + (ab >> 31) + (lo < mid ? 1u : 0u);
    return (hi << 2) | (lo >> 62);
}
constexpr Log2Table make_log2_table() {
    Log2Table tab{};
    for (int i = 0; i < 256; ++i) {
        uint64_t y = static_cast<uint64_t>(256 + i) << 54;
        int32_t t = 0;
        for (int b = 0; b < 24; ++b) {
            y = square_q62(y);
            t <<= 1;
            if (y >> 63) {
                t |= 1;
                y >>= 1;
            }
        }
        tab.t[i] = t;
    }
    tab.t[256] = 1 << 24;
    return tab;
}
constexpr Log2Table kLog2Host = make_log2_table();
__device__ const Log2Table kLog2Dev = make_log2_table();

// LOG2Q(x), 1 <= x < 2^32: 2^24 log2(x) in [-2.9e-6 * 2^24, 0] of the true value, monotone.  T: the table (LDS on the device).
__host__ __device__ __forceinline__ uint32_t log2q(uint32_t x, const int32_t* T) {
    const int n = 31 - __builtin_clz(x);
    const uint32_t m = (x << (31 - n)) << 1;         // the 32 bits below the leading one
    const uint32_t i = m >> 24, r = (m >> 8) & 0xFFFFu;
    const uint32_t lo = static_cast<uint32_t>(T[i]), d = static_cast<uint32_t>(T[i + 1]) - lo;
    return (static_cast<uint32_t>(n) << 24) + lo + static_cast<uint32_t>((static_cast<uint64_t>(d) * r) >> 16);
}
// the key of an edge whose id hashes to h, under the quantised weight wq (read as unsigned; above 2^24 - 1 it counts as 2^24 - 1)
__host__ __device__ __forceinline__ uint32_t weighted_key(uint32_t h, uint32_t wq, const int32_t* T) {
    if (wq == 0u) return kNoKey;
    const uint32_t nl = (32u << 24) - log2q(h ? h : 1u, T);               // -log2 of a uniform variate, in [1, 2^29]
    return log2q(nl, T) - log2q(wq > kWqMax ? kWqMax : wq, T) + (24u << 24);
}

// LDS traffic of ONE wave: its lanes' atomics / stores are visible to its lanes' later loads
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int64_t row_deg(const int* __restrict__ ptr, int64_t N, int v) {
    return (v < 0 || v >= N) ? 0 : static_cast<int64_t>(ptr[v + 1]) - static_cast<int64_t>(ptr[v]);
}
__device__ __forceinline__ int64_t row_take(int64_t deg, int64_t f) { return (f < 0 || deg <= f) ? deg : f; }

// ---------------------------------------------------------------- the per-item actions of the scans (scan_one: csrc/batch_rows.h)
struct OffsOp {                                     // offs[r] = sum of min(f, deg) over the frontier rows before r
    const int* ptr;
    const int* rows;
    int64_t N, f;
    int64_t* offs;
    int64_t n_rows;
    int64_t* total;
    __device__ int load(int64_t i) const { return static_cast<int>(row_take(row_deg(ptr, N, rows[i]), f)); }
    __device__ void store(int64_t i, int64_t before, int) const { offs[i] = before; }
    __device__ void finish(int64_t t) const {
        offs[n_rows] = t;
        if (total) *total = t;
    }
};

struct EmitOp {                                     // the new nodes of a hop, ascending; members |= new; reached = 0
    uint32_t* member;
    uint32_t* reached;
    int* frontier;
    int64_t cap, N;
    const int* ptr;
    int64_t f_next;
    int64_t* sizes;                                 // [0] = new nodes, [1] = sum of min(f_next, deg) over them (zeroed by the marking launch)
    __device__ int load(int64_t w) const { return __popc(reached[w] & ~member[w]); }
    __device__ void store(int64_t w, int64_t before, int) const {
        uint32_t fresh = reached[w] & ~member[w];
        reached[w] = 0u;
        if (!fresh) return;
        member[w] |= fresh;
        int64_t take = 0;
        while (fresh) {
            const int b = __ffs(fresh) - 1;
            fresh &= fresh - 1;
            const int64_t v = w * 32 + b;
            if (v < N) {
                if (before < cap) frontier[before] = static_cast<int>(v);
                if (f_next != 0) take += row_take(row_deg(ptr, N, static_cast<int>(v)), f_next);
            }
            ++before;
        }
        if (take) atomicAdd(reinterpret_cast<u64*>(sizes + 1), static_cast<u64>(take));
    }
    __device__ void finish(int64_t t) const { sizes[0] = t; }
};

struct RankOp {                                     // wpre[w] = members below word w; node_ids = the members ascending
    const uint32_t* member;
    int* wpre;
    int64_t* node_ids;
    int64_t n;
    int* mismatch;
    __device__ int load(int64_t w) const { return __popc(member[w]); }
    __device__ void store(int64_t w, int64_t before, int) const {
        wpre[w] = static_cast<int>(before);
        uint32_t m = member[w];
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            if (before < n) node_ids[before] = w * 32 + b;
            ++before;
        }
    }
    __device__ void finish(int64_t t) const {
        if (mismatch && t != n) *mismatch = 1;
    }
};

// ---------------------------------------------------------------- selection
// the digit of the k-th smallest (k >= 1) among the keys counted in hist[256]; k becomes its rank inside that bin.  Same result in every lane.
__device__ __forceinline__ uint32_t find_digit(const uint32_t* hist, uint32_t& k) {
    const int lane = threadIdx.x & 63;
    uint32_t h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = hist[lane * 4 + j];
    const uint32_t s = (h[0] + h[1]) + (h[2] + h[3]);
    uint32_t inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    const uint32_t exc = inc - s;
    const bool here = exc < k && k <= inc;          // exactly one lane (the bins hold at least k keys)
    uint32_t d = 0, kk = 0;
    if (here) {
        uint32_t run = exc;
        int j = 0;
        while (j < 3 && run + h[j] < k) {
            run += h[j];
            ++j;
        }
        d = static_cast<uint32_t>(lane * 4 + j);
        kk = k - run;
    }
    const u64 m = __ballot(here);
    const int src = m ? __ffsll(static_cast<long long>(m)) - 1 : 0;
    k = __shfl(kk, src, 64);
    return __shfl(d, src, 64);
}

// the key of entry e of the in-CSR under id `id`: the hash, or the weighted key from wq[e] and the table T
template <bool kWeighted>
__device__ __forceinline__ uint32_t entry_key(int id, const int* __restrict__ wq, int64_t e, uint32_t K, const int32_t* T) {
    const uint32_t h = fmix32(static_cast<uint32_t>(id) ^ K);
    if constexpr (kWeighted) return weighted_key(h, static_cast<uint32_t>(wq[e]), T);
    else return h;
}

// `who` of `team` threads walk the entries [beg, end) of a row: the keys that agree with `prefix` on the bits of `mask` go into hist
template <bool kWeighted>
__device__ __forceinline__ void tally_keys(const int* __restrict__ eid, const int* __restrict__ wq, const int32_t* T, int64_t beg, int64_t end,
                                           int who, int team, uint32_t K, uint32_t prefix, uint32_t mask, int shift, uint32_t* hist) {
    for (int64_t e = beg + who; e < end; e += team) {
        const uint32_t key = entry_key<kWeighted>(eid[e], wq, e, K, T);
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
}

// kWeighted = false: keys fmix32(id ^ K), distinct, one-part compaction (key <= threshold).  kWeighted = true: keys from wq (aligned with eid)
// through the LDS copy of the log2 table, two-part compaction (key < threshold, then the first k ties in row order).
template <bool kWeighted>
__global__ void __launch_bounds__(kT) nbr_select(const int* __restrict__ ptr, const int* __restrict__ eid, int64_t N, const int* __restrict__ rows,
                                                 int64_t n_rows, int64_t f, uint32_t K, const int64_t* __restrict__ offs, int* __restrict__ chosen,
                                                 int64_t cap, const int* __restrict__ wq) {
    __shared__ uint32_t hist[kWaves][256];
    __shared__ int wcnt[2][kWaves];
    const int32_t* T = nullptr;
    uint32_t* skey = nullptr;
    if constexpr (kWeighted) {
        __shared__ int32_t tab[257];
        __shared__ uint32_t staged[kWaves][kHubRow];                    // a one-wave row's keys, computed once (32 KiB per workgroup)
        skey = staged[threadIdx.x >> 6];
        for (int i = threadIdx.x; i < 257; i += kT) tab[i] = kLog2Dev.t[i];
        __syncthreads();
        T = tab;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t tiles = (n_rows + kWaves - 1) / kWaves;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {           // the trip count is the same for every wave: barriers below are safe
        const int64_t r = t * kWaves + wid;
        if (r < n_rows) {
            const int v = rows[r];
            const int64_t deg = row_deg(ptr, N, v);
            if (deg > 0 && deg <= kHubRow) {
                const int64_t beg = ptr[v], end = beg + deg, out = offs[r];
                if (f < 0 || deg <= f) {
                    for (int64_t i = lane; i < deg; i += kWave)
                        if (out + i < cap) chosen[out + i] = eid[beg + i];
                } else {
                    uint32_t* hs = hist[wid];
                    uint32_t prefix = 0, mask = 0, k = static_cast<uint32_t>(f);
                    for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) hs[lane * 4 + j] = 0u;
                        wave_sync();
                        if constexpr (kWeighted) {                           // first pass: the keys go to LDS; a lane re-reads its own
                            for (int64_t e = beg + lane; e < end; e += kWave) {
                                uint32_t key;
                                if (shift == 24) {
                                    key = entry_key<true>(eid[e], wq, e, K, T);
                                    skey[e - beg] = key;
                                } else {
                                    key = skey[e - beg];
                                }
                                if ((key & mask) == prefix) atomicAdd(&hs[(key >> shift) & 255u], 1u);
                            }
                        } else {
                            tally_keys<false>(eid, wq, T, beg, end, lane, kWave, K, prefix, mask, shift, hs);
                        }
                        wave_sync();
                        const uint32_t d = find_digit(hs, k);
                        wave_sync();
                        prefix |= d << shift;
                        mask |= 255u << shift;
                    }
                    int64_t run = 0;                                     // prefix is now the f-th smallest key itself
                    int64_t ties = 0;                                    // (weighted) and k how many ids with exactly that key are taken
                    for (int64_t b = beg; b < end; b += kWave) {
                        const int64_t e = b + lane;
                        int id = 0;
                        bool in = false, tie = false;
                        if (e < end) {
                            id = eid[e];
                            if constexpr (kWeighted) {
                                const uint32_t key = skey[e - beg];
                                in = key < prefix;
                                tie = key == prefix;
                            } else {
                                in = entry_key<false>(id, wq, e, K, T) <= prefix;
                            }
                        }
                        const u64 m = __ballot(in);
                        int64_t pos = run + __popcll(m & ((1ull << lane) - 1ull));
                        if constexpr (kWeighted) {                           // the ties before this lane that are taken: the first k of them
                            const u64 mt = __ballot(tie);
                            const int64_t before = ties + __popcll(mt & ((1ull << lane) - 1ull));
                            pos += before < k ? before : k;
                            in = in || (tie && before < k);
                            ties += __popcll(mt);
                        }
                        if (in && pos < f && out + pos < cap) chosen[out + pos] = id;       // (pos < f: repeated ids would tie)
                        run += __popcll(m);
                    }
                }
            }
        }
        // the tile's hub rows, one after the other, by all waves on histogram 0
        for (int w = 0; w < kWaves; ++w) {
            const int64_t hr = t * kWaves + w;
            if (hr >= n_rows) break;
            const int hv = rows[hr];
            const int64_t deg = row_deg(ptr, N, hv);
            if (deg <= kHubRow) continue;                               // (uniform over the workgroup: read from global memory by all)
            const int64_t beg = ptr[hv], end = beg + deg, out = offs[hr];
            if (f < 0 || deg <= f) {
                for (int64_t i = threadIdx.x; i < deg; i += kT)
                    if (out + i < cap) chosen[out + i] = eid[beg + i];
                continue;
            }
            uint32_t prefix = 0, mask = 0, k = static_cast<uint32_t>(f);
            for (int shift = 24; shift >= 0; shift -= 8) {
                __syncthreads();                                        // wave 0 is done with histogram 0; the last find is over
                hist[0][threadIdx.x] = 0u;
                __syncthreads();
                tally_keys<kWeighted>(eid, wq, T, beg, end, threadIdx.x, kT, K, prefix, mask, shift, hist[0]);
                __syncthreads();
                const uint32_t d = find_digit(hist[0], k);              // every wave finds the same digit
                prefix |= d << shift;
                mask |= 255u << shift;
            }
            int64_t run = 0, ties = 0;
            int buf = 0;
            for (int64_t b = beg; b < end; b += kT, buf ^= 1) {
                const int64_t e = b + threadIdx.x;
                int id = 0;
                bool in = false, tie = false;
                if (e < end) {
                    id = eid[e];
                    const uint32_t key = entry_key<kWeighted>(id, wq, e, K, T);
                    if constexpr (kWeighted) {
                        in = key < prefix;
                        tie = key == prefix;
                    } else {
                        in = key <= prefix;
                    }
                }
                const u64 m = __ballot(in);
                if (lane == 0) wcnt[buf][wid] = __popcll(m);
                int64_t taken_ties = 0;                                 // (weighted) the ties before this thread that are taken
                if constexpr (kWeighted) {                               // a second row of counts: the ties of every wave
                    __shared__ int wties[2][kWaves];
                    const u64 mt = __ballot(tie);
                    if (lane == 0) wties[buf][wid] = __popcll(mt);
                    __syncthreads();
                    int tbefore = 0, ttotal = 0;
#pragma unroll
                    for (int x = 0; x < kWaves; ++x) {
                        const int c = wties[buf][x];
                        tbefore += x < wid ? c : 0;
                        ttotal += c;
                    }
                    const int64_t tb = ties + tbefore + __popcll(mt & ((1ull << lane) - 1ull));
                    ties += ttotal;
                    taken_ties = tb < k ? tb : k;
                    in = in || (tie && tb < k);
                } else {
                    __syncthreads();                                    // (two rows of counts alternate: one barrier per step)
                }
                int before = 0, total = 0;
#pragma unroll
                for (int x = 0; x < kWaves; ++x) {
                    const int c = wcnt[buf][x];
                    before += x < wid ? c : 0;
                    total += c;
                }
                const int64_t pos = run + before + __popcll(m & ((1ull << lane) - 1ull)) + taken_ties;
                if (in && pos < f && out + pos < cap) chosen[out + pos] = id;
                run += total;
            }
            __syncthreads();
        }
        __syncthreads();                                                // the next tile's one-wave rows reuse the histograms
    }
}

// ---------------------------------------------------------------- frontier
__global__ void __launch_bounds__(kT) nbr_seed(const int* __restrict__ seeds, int64_t n, int64_t N, uint32_t* __restrict__ member,
                                               uint32_t* __restrict__ seedbits) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (i >= n) return;
    const int v = seeds[i];
    if (v < 0 || v >= N) return;
    atomicOr(&member[v >> 5], 1u << (v & 31));
    atomicOr(&seedbits[v >> 5], 1u << (v & 31));
}

__global__ void __launch_bounds__(kT) nbr_reach(const int* __restrict__ chosen, int64_t n, const int64_t* __restrict__ src, int64_t E, int64_t N,
                                                const uint32_t* __restrict__ member, uint32_t* __restrict__ reached, int64_t* __restrict__ sizes) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (i == 0) sizes[0] = sizes[1] = 0;
    if (i >= n) return;
    const int e = chosen[i];
    if (e < 0 || e >= E) return;
    const int64_t u = src[e];
    if (u < 0 || u >= N) return;
    const uint32_t bit = 1u << (u & 31);
    if (!(member[u >> 5] & bit)) atomicOr(&reached[u >> 5], bit);
}

// ---------------------------------------------------------------- collate
__device__ __forceinline__ bool is_member(const uint32_t* __restrict__ member, int64_t v) { return (member[v >> 5] >> (v & 31)) & 1u; }
__device__ __forceinline__ int64_t local_id(const uint32_t* __restrict__ member, const int* __restrict__ wpre, int64_t v) {
    return static_cast<int64_t>(wpre[v >> 5]) + __popc(member[v >> 5] & ((1u << (v & 31)) - 1u));
}

// The squeeze's policy (csrc/batch_rows.h): local row r is the out-CSR row of member node_ids[r]; an entry is kept when its column is a
// member (and column and id are in range); its local column is the column's rank among the members, its id the stored edge id.
struct InducedRows {
    static constexpr bool kStaged = false;
    struct Lds {};
    const int* optr;
    const int* odst;
    const int* oeid;
    int64_t N, E;
    const uint32_t* member;
    const int* wpre;
    const int64_t* node_ids;
    __device__ void stage(Lds&) const {}
    __device__ RowSpan row(const Lds&, int64_t r) const {
        const int64_t v = node_ids[r];
        if (v < 0 || v >= N) return RowSpan{0, 0, v};
        return RowSpan{optr[v], optr[v + 1], v};
    }
    __device__ void side_work(int64_t, int64_t, int) const {}
    __device__ bool keep(const Lds&, int64_t e, int64_t& lc, int64_t& id) const {
        const int64_t c = odst[e];
        id = oeid[e];
        if (!(c >= 0 && c < N && id >= 0 && id < E && is_member(member, c))) return false;
        lc = local_id(member, wpre, c);
        return true;
    }
};
template <bool kWrite>
void launch_induced(const InducedRows& rows, int64_t n, int64_t E_b, int64_t* rowptr, const float* prob, int64_t* ei_out, float* prob_out,
                    int64_t* eid_out, hipStream_t stream) {
    hipLaunchKernelGGL((squeeze_rows<InducedRows, kT, kHubRow, kWrite>), dim3(static_cast<unsigned>(cdiv(n, kWaves))), dim3(kT), 0, stream, rows, n,
                       E_b, rowptr, prob, ei_out, prob_out, eid_out);
}

struct Segments {
    const int* ptr[kMaxHops];
    int64_t pre[kMaxHops + 1];
    int n;
};
// the chosen ids of every hop as 64-bit sort keys; an id outside [0, E) or with an end outside the members sorts behind every real one
__global__ void __launch_bounds__(kT) nbr_keys(const Segments s, int64_t m, const int64_t* __restrict__ edge_index, int64_t E, int64_t N,
                                               const uint32_t* __restrict__ member, uint64_t* __restrict__ keys, int64_t* __restrict__ total) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (i == 0) *total = 0;
    if (i >= m) return;
    int j = 0;
    while (j + 1 < s.n && i >= s.pre[j + 1]) ++j;
    const int e = s.ptr[j][i - s.pre[j]];
    bool ok = e >= 0 && e < E;
    if (ok) {
        const int64_t a = edge_index[e], b = edge_index[E + e];
        ok = a >= 0 && a < N && b >= 0 && b < N && is_member(member, a) && is_member(member, b);
    }
    keys[i] = ok ? static_cast<uint64_t>(e) : (uint64_t(1) << 32);
}
__global__ void __launch_bounds__(kT) nbr_directional(const uint64_t* __restrict__ sorted, int64_t m, const int64_t* __restrict__ edge_index,
                                                      int64_t E, const uint32_t* __restrict__ member, const int* __restrict__ wpre,
                                                      const float* __restrict__ prob, int64_t* __restrict__ ei_out, float* __restrict__ prob_out,
                                                      int64_t* __restrict__ eid_out, int64_t* __restrict__ total) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    bool ok = false;
    if (i < m) {
        const uint64_t key = sorted[i];
        ok = key < static_cast<uint64_t>(E);
        if (ok) {                                                       // the real ids are the first of the sorted list: position = rank
            const int64_t e = static_cast<int64_t>(key);
            ei_out[i] = local_id(member, wpre, edge_index[e]);
            ei_out[m + i] = local_id(member, wpre, edge_index[E + e]);
            if (prob_out) prob_out[i] = prob[e];
            if (eid_out) eid_out[i] = e;
        }
    }
    const int c = __popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(reinterpret_cast<u64*>(total), static_cast<u64>(c));
}

// one wave per member: its x row (whole 4-byte words), y, the three masks ANDed with "is a seed", and the seed flag
__global__ void __launch_bounds__(kT) nbr_gather(const int64_t* __restrict__ node_ids, int64_t n, int64_t N, const uint32_t* __restrict__ x,
                                                 int64_t row_words, uint32_t* __restrict__ x_out, const int64_t* __restrict__ y,
                                                 int64_t* __restrict__ y_out, const uint8_t* __restrict__ masks, const uint32_t* __restrict__ seedbits,
                                                 uint8_t* __restrict__ masks_out, uint8_t* __restrict__ seed_out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    if (r >= n) return;
    const int64_t v = node_ids[r];
    if (v < 0 || v >= N) return;
    const uint32_t* src = x + v * row_words;
    uint32_t* dst = x_out + r * row_words;
    for (int64_t i = lane; i < row_words; i += kWave) dst[i] = src[i];
    const bool seed = is_member(seedbits, v);
    if (lane < 3) masks_out[lane * n + r] = (seed && masks[lane * N + v]) ? 1 : 0;
    if (lane == 3) seed_out[r] = seed ? 1 : 0;
    if (lane == 4) y_out[r] = y[v];
}

int64_t words_of(int64_t N) { return (N + 31) / 32; }
size_t state_bytes_for(int64_t N) { return 3 * carve_bytes(static_cast<size_t>(words_of(N)) + 1, 4); }
struct State {
    uint32_t *member, *reached, *seedbits;
};
int open_state(const char* who, int64_t N, void* state, size_t state_bytes, State& s) {
    SGS_REQUIRE(N >= 1 && N < (int64_t(1) << 31), SGS_EINVAL, "%s: N = %lld outside [1, 2^31)", who, (long long)N);
    SGS_REQUIRE(state != nullptr && (reinterpret_cast<uintptr_t>(state) & 3) == 0, SGS_EINVAL, "%s: null or misaligned state", who);
    SGS_REQUIRE(state_bytes >= state_bytes_for(N), SGS_EWORKSPACE, "%s: state too small (%zu < %zu bytes)", who, state_bytes, state_bytes_for(N));
    Carver c(state);
    const size_t w = static_cast<size_t>(words_of(N)) + 1;
    s.member = c.take<uint32_t>(w);
    s.reached = c.take<uint32_t>(w);
    s.seedbits = c.take<uint32_t>(w);
    return SGS_OK;
}
int64_t grid_rows(int64_t rows) {
    const int64_t tiles = cdiv(rows, kWaves);
    return tiles < 1 ? 1 : (tiles > 4096 ? 4096 : tiles);
}
struct DirLayout {
    size_t keys, temp, total, temp_bytes;
};
DirLayout dir_layout(int64_t m) {
    DirLayout L{};
    L.temp_bytes = m > 0 ? auc_sort_temp_bytes(m, 0, kSortBits) : 0;
    L.keys = carve_bytes(static_cast<size_t>(m) + 1, 8);
    L.temp = carve_bytes(L.temp_bytes + 256, 1);
    L.total = 2 * L.keys + L.temp + 256;
    return L;
}
}  // namespace
}  // namespace sgs

extern "C" {
int64_t sgs_nbr_select_hub_row(void) { return sgs::kHubRow; }
int sgs_nbr_max_hops(void) { return sgs::kMaxHops; }

size_t sgs_nbr_select_workspace_bytes(int64_t n_rows) { return sgs::carve_bytes(static_cast<size_t>(n_rows > 0 ? n_rows : 0) + 1, 8); }

}  // extern "C"

namespace sgs {
namespace {
// both selection entry points: the same checks, the same scan, the row kernel with or without weights
template <bool kWeighted>
int select_rows(const char* who, const int32_t* in_ptr, const int32_t* in_eid, const int32_t* in_wq, int64_t N, int64_t nnz, const int32_t* rows,
                int64_t n_rows, int64_t fanout, uint32_t key, int32_t* chosen, int64_t cap, int64_t* total_dev, void* ws, size_t ws_bytes,
                hipStream_t stream) {
    SGS_REQUIRE(N >= 1 && nnz >= 0 && N < (int64_t(1) << 31) && nnz < (int64_t(1) << 31), SGS_EINVAL,
                "%s: bad sizes (N = %lld, nnz = %lld): need 1 <= N < 2^31, 0 <= nnz < 2^31", who, (long long)N, (long long)nnz);
    SGS_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31) && cap >= 0, SGS_EINVAL, "%s: bad n_rows or cap", who);
    SGS_REQUIRE(fanout == -1 || (fanout >= 1 && fanout < (int64_t(1) << 31)), SGS_EINVAL, "%s: fanout = %lld, need >= 1 or -1 (every neighbour)", who,
                (long long)fanout);
    SGS_REQUIRE(in_ptr && (in_eid || nnz == 0) && (!kWeighted || in_wq || nnz == 0) && (rows || n_rows == 0) && (chosen || cap == 0) && ws, SGS_EINVAL,
                "%s: null pointer", who);
    SGS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, SGS_EINVAL, "%s: workspace must be 8-byte aligned", who);
    SGS_REQUIRE(ws_bytes >= sgs_nbr_select_workspace_bytes(n_rows), SGS_EWORKSPACE, "%s: workspace too small", who);
    int64_t* offs = static_cast<int64_t*>(ws);
    hipLaunchKernelGGL(scan_one<OffsOp>, dim3(1), dim3(kST), 0, stream, OffsOp{in_ptr, rows, N, fanout, offs, n_rows, total_dev}, n_rows);
    SGS_LAUNCH_OK();
    if (n_rows > 0 && cap > 0) {
        hipLaunchKernelGGL(nbr_select<kWeighted>, dim3(static_cast<unsigned>(grid_rows(n_rows))), dim3(kT), 0, stream, in_ptr, in_eid, N, rows, n_rows,
                           fanout, key, offs, chosen, cap, in_wq);
        SGS_LAUNCH_OK();
    }
    return SGS_OK;
}
}  // namespace
}  // namespace sgs

extern "C" {
int sgs_nbr_select(const int32_t* in_ptr, const int32_t* in_eid, int64_t N, int64_t nnz, const int32_t* rows, int64_t n_rows, int64_t fanout,
                   uint32_t key, int32_t* chosen, int64_t cap, int64_t* total_dev, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    return sgs::select_rows<false>("sgs_nbr_select", in_ptr, in_eid, nullptr, N, nnz, rows, n_rows, fanout, key, chosen, cap, total_dev, ws, ws_bytes,
                                   static_cast<hipStream_t>(stream_));
}

int sgs_nbr_select_weighted(const int32_t* in_ptr, const int32_t* in_eid, const int32_t* in_wq, int64_t N, int64_t nnz, const int32_t* rows,
                            int64_t n_rows, int64_t fanout, uint32_t key, int32_t* chosen, int64_t cap, int64_t* total_dev, void* ws,
                            size_t ws_bytes, sgs_stream_t stream_) {
    return sgs::select_rows<true>("sgs_nbr_select_weighted", in_ptr, in_eid, in_wq, N, nnz, rows, n_rows, fanout, key, chosen, cap, total_dev, ws,
                                  ws_bytes, static_cast<hipStream_t>(stream_));
}

void sgs_nbr_log2_table(int32_t* out) {
    for (int i = 0; i < 257; ++i) out[i] = sgs::kLog2Host.t[i];
}

uint32_t sgs_nbr_weighted_key(uint32_t hash, uint32_t wq) { return sgs::weighted_key(hash, wq, sgs::kLog2Host.t); }

size_t sgs_nbr_state_bytes(int64_t N) { return (N < 1 || N >= (int64_t(1) << 31)) ? 256 : sgs::state_bytes_for(N); }

int sgs_nbr_begin(const int32_t* seeds, int64_t n_seeds, int64_t N, void* state, size_t state_bytes, sgs_stream_t stream_) {
    using namespace sgs;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    State s;
    if (int rc = open_state("sgs_nbr_begin", N, state, state_bytes, s)) return rc;
    SGS_REQUIRE(n_seeds >= 0 && n_seeds < (int64_t(1) << 31) && (seeds || n_seeds == 0), SGS_EINVAL, "sgs_nbr_begin: bad seed list");
    if (int rc = zero_async(state, state_bytes_for(N), stream)) return rc;
    if (n_seeds > 0) {
        hipLaunchKernelGGL(nbr_seed, dim3(static_cast<unsigned>(cdiv(n_seeds, kT))), dim3(kT), 0, stream, seeds, n_seeds, N, s.member, s.seedbits);
        SGS_LAUNCH_OK();
    }
    return SGS_OK;
}

int sgs_nbr_frontier(const int32_t* chosen, int64_t n_chosen, const int64_t* edge_index, int64_t E, int64_t N, const int32_t* in_ptr,
                     int64_t next_fanout, void* state, size_t state_bytes, int32_t* frontier_out, int64_t cap, int64_t* sizes_dev,
                     sgs_stream_t stream_) {
    using namespace sgs;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    State s;
    if (int rc = open_state("sgs_nbr_frontier", N, state, state_bytes, s)) return rc;
    SGS_REQUIRE(E >= 0 && E < (int64_t(1) << 31) && n_chosen >= 0 && n_chosen < (int64_t(1) << 31) && cap >= 0, SGS_EINVAL,
                "sgs_nbr_frontier: bad sizes");
    SGS_REQUIRE(next_fanout >= -1 && next_fanout < (int64_t(1) << 31), SGS_EINVAL, "sgs_nbr_frontier: next_fanout = %lld (0: no next hop)",
                (long long)next_fanout);
    SGS_REQUIRE((chosen || n_chosen == 0) && (edge_index || E == 0) && in_ptr && sizes_dev && (frontier_out || cap == 0), SGS_EINVAL,
                "sgs_nbr_frontier: null pointer");
    hipLaunchKernelGGL(nbr_reach, dim3(static_cast<unsigned>(n_chosen > 0 ? cdiv(n_chosen, kT) : 1)), dim3(kT), 0, stream, chosen, n_chosen,
                       edge_index, E, N, s.member, s.reached, sizes_dev);
    hipLaunchKernelGGL(scan_one<EmitOp>, dim3(1), dim3(kST), 0, stream, EmitOp{s.member, s.reached, frontier_out, cap, N, in_ptr, next_fanout, sizes_dev},
                       words_of(N));
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_nbr_nodes(const void* state, size_t state_bytes, int64_t N, int64_t n, int32_t* wpre, int64_t* node_ids, int32_t* mismatch_dev,
                  sgs_stream_t stream_) {
    using namespace sgs;
    State s;
    if (int rc = open_state("sgs_nbr_nodes", N, const_cast<void*>(state), state_bytes, s)) return rc;
    SGS_REQUIRE(n >= 0 && n <= N && wpre && (node_ids || n == 0), SGS_EINVAL, "sgs_nbr_nodes: bad n or null pointer");
    hipLaunchKernelGGL(scan_one<RankOp>, dim3(1), dim3(kST), 0, static_cast<hipStream_t>(stream_), RankOp{s.member, wpre, node_ids, n, mismatch_dev},
                       words_of(N));
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_nbr_induced_count(const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, int64_t N, int64_t E, const void* state,
                          size_t state_bytes, const int32_t* wpre, const int64_t* node_ids, int64_t n, int64_t* rowptr, int64_t* total_dev,
                          sgs_stream_t stream_) {
    using namespace sgs;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    State s;
    if (int rc = open_state("sgs_nbr_induced_count", N, const_cast<void*>(state), state_bytes, s)) return rc;
    SGS_REQUIRE(E >= 0 && E < (int64_t(1) << 31) && n >= 0 && n <= N, SGS_EINVAL, "sgs_nbr_induced_count: bad sizes");
    SGS_REQUIRE(out_ptr && (E == 0 || (out_dst && out_eid)) && wpre && (node_ids || n == 0) && rowptr, SGS_EINVAL,
                "sgs_nbr_induced_count: null pointer");
    if (n > 0) {
        launch_induced<false>(InducedRows{out_ptr, out_dst, out_eid, N, E, s.member, wpre, node_ids}, n, 0, rowptr, nullptr, nullptr, nullptr, nullptr,
                              stream);
        SGS_LAUNCH_OK();
    }
    hipLaunchKernelGGL(scan_one<RowptrOp>, dim3(1), dim3(kST), 0, stream, RowptrOp{rowptr, n, total_dev, 0, nullptr}, n);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_nbr_induced_fill(const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, const float* prob, int64_t N, int64_t E,
                         const void* state, size_t state_bytes, const int32_t* wpre, const int64_t* node_ids, int64_t n, const int64_t* rowptr,
                         int64_t E_b, int64_t* edge_index_out, float* prob_out, int64_t* eid_out, sgs_stream_t stream_) {
    using namespace sgs;
    State s;
    if (int rc = open_state("sgs_nbr_induced_fill", N, const_cast<void*>(state), state_bytes, s)) return rc;
    SGS_REQUIRE(E >= 0 && E < (int64_t(1) << 31) && n >= 0 && n <= N && E_b >= 0 && E_b <= E, SGS_EINVAL, "sgs_nbr_induced_fill: bad sizes");
    SGS_REQUIRE(out_ptr && (E == 0 || (out_dst && out_eid)) && wpre && (node_ids || n == 0) && rowptr && (edge_index_out || E_b == 0), SGS_EINVAL,
                "sgs_nbr_induced_fill: null pointer");
    SGS_REQUIRE(prob_out == nullptr || prob != nullptr, SGS_EINVAL, "sgs_nbr_induced_fill: prob_out without prob");
    if (n > 0 && E_b > 0) {
        launch_induced<true>(InducedRows{out_ptr, out_dst, out_eid, N, E, s.member, wpre, node_ids}, n, E_b, const_cast<int64_t*>(rowptr), prob,
                             edge_index_out, prob_out, eid_out, static_cast<hipStream_t>(stream_));
        SGS_LAUNCH_OK();
    }
    return SGS_OK;
}

size_t sgs_nbr_directional_workspace_bytes(int64_t m) { return (m < 0 || m >= (int64_t(1) << 31)) ? 256 : sgs::dir_layout(m).total; }

int sgs_nbr_directional(const int64_t* segments_host, int64_t n_segments, int64_t m, const int64_t* edge_index, int64_t E, int64_t N,
                        const float* prob, const void* state, size_t state_bytes, const int32_t* wpre, int64_t* edge_index_out, float* prob_out,
                        int64_t* eid_out, int64_t* total_dev, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    using namespace sgs;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    State s;
    if (int rc = open_state("sgs_nbr_directional", N, const_cast<void*>(state), state_bytes, s)) return rc;
    SGS_REQUIRE(n_segments >= 1 && n_segments <= kMaxHops && segments_host, SGS_EINVAL, "sgs_nbr_directional: %lld segments, need 1 to %d",
                (long long)n_segments, kMaxHops);
    SGS_REQUIRE(E >= 0 && E < (int64_t(1) << 31) && m >= 0 && m < (int64_t(1) << 31), SGS_EINVAL, "sgs_nbr_directional: bad sizes");
    Segments sg{};
    int64_t pre = 0;
    for (int64_t j = 0; j < n_segments; ++j) {
        const int64_t cnt = segments_host[2 * j + 1];
        SGS_REQUIRE(cnt >= 0 && (cnt == 0 || segments_host[2 * j] != 0), SGS_EINVAL, "sgs_nbr_directional: segment %lld: bad count or null address",
                    (long long)j);
        sg.ptr[j] = reinterpret_cast<const int*>(static_cast<uintptr_t>(segments_host[2 * j]));
        sg.pre[j] = pre;
        pre += cnt;
    }
    sg.pre[n_segments] = pre;
    sg.n = static_cast<int>(n_segments);
    SGS_REQUIRE(pre == m, SGS_EINVAL, "sgs_nbr_directional: the segments hold %lld ids, m = %lld", (long long)pre, (long long)m);
    SGS_REQUIRE((edge_index || E == 0) && wpre && total_dev && (edge_index_out || m == 0) && ws, SGS_EINVAL, "sgs_nbr_directional: null pointer");
    SGS_REQUIRE(prob_out == nullptr || prob != nullptr, SGS_EINVAL, "sgs_nbr_directional: prob_out without prob");
    SGS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, SGS_EINVAL, "sgs_nbr_directional: workspace must be 8-byte aligned");
    const DirLayout L = dir_layout(m);
    SGS_REQUIRE(ws_bytes >= L.total, SGS_EWORKSPACE, "sgs_nbr_directional: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    Carver cv(ws);
    uint64_t* keys = cv.take<uint64_t>(static_cast<size_t>(m) + 1);
    uint64_t* sorted = cv.take<uint64_t>(static_cast<size_t>(m) + 1);
    void* temp = cv.take<char>(L.temp_bytes + 256);
    const dim3 grid(static_cast<unsigned>(m > 0 ? cdiv(m, kT) : 1)), blk(kT);
    hipLaunchKernelGGL(nbr_keys, grid, blk, 0, stream, sg, m, edge_index, E, N, s.member, keys, total_dev);
    SGS_LAUNCH_OK();
    if (m == 0) return SGS_OK;
    if (int rc = auc_sort_keys(keys, sorted, m, 0, kSortBits, temp, L.temp_bytes, stream)) return rc;
    hipLaunchKernelGGL(nbr_directional, grid, blk, 0, stream, sorted, m, edge_index, E, s.member, wpre, prob, edge_index_out, prob_out, eid_out,
                       total_dev);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_nbr_gather(const int64_t* node_ids, int64_t n, int64_t N, const void* x, int64_t row_bytes, void* x_out, const int64_t* y, int64_t* y_out,
                   const uint8_t* masks, const void* state, size_t state_bytes, uint8_t* masks_out, uint8_t* seed_mask_out, sgs_stream_t stream_) {
    using namespace sgs;
    State s;
    if (int rc = open_state("sgs_nbr_gather", N, const_cast<void*>(state), state_bytes, s)) return rc;
    SGS_REQUIRE(n >= 0 && n <= N, SGS_EINVAL, "sgs_nbr_gather: n = %lld outside [0, N]", (long long)n);
    SGS_REQUIRE(row_bytes >= 0 && row_bytes % 4 == 0, SGS_EINVAL, "sgs_nbr_gather: a row of x must be whole 4-byte words (row_bytes = %lld)",
                (long long)row_bytes);
    SGS_REQUIRE(n == 0 || (node_ids && (row_bytes == 0 || (x && x_out)) && y && y_out && masks && masks_out && seed_mask_out), SGS_EINVAL,
                "sgs_nbr_gather: null pointer");
    if (n > 0) {
        hipLaunchKernelGGL(nbr_gather, dim3(static_cast<unsigned>(cdiv(n, kWaves))), dim3(kT), 0, static_cast<hipStream_t>(stream_), node_ids, n, N,
                           static_cast<const uint32_t*>(x), row_bytes / 4, static_cast<uint32_t*>(x_out), y, y_out, masks, s.seedbits, masks_out,
                           seed_mask_out);
        SGS_LAUNCH_OK();
    }
    return SGS_OK;
}
}
