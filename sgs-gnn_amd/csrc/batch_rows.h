// What the device-side batch builders share (users: csrc/cluster.hip, csrc/neighbor.hip): ONE single-workgroup exclusive scan and ONE
// squeeze of CSR rows (count -> scan -> fill).  Integer work only, no atomics: both builders' outputs are exact.
//
// SCAN (scan_one<Op>): one workgroup of kST threads walks tiles of kST * kSPer items -- kSPer per thread, a wave scan, the 16 wave totals
// through two alternating LDS rows (one barrier per tile), a running carry.  An Op provides
//   int  load(i)                   the item's count
//   void store(i, before, count)   what to do with the item's exclusive prefix
//   void finish(total)             by thread 0, after the last tile
//
// SQUEEZE (squeeze_rows<P, kThreads, kHub, kWrite>): one WAVE per local row, 64 entries per step; a ballot and a prefix popcount give the
// kept count and the output positions, so a row's kept entries keep their order.  kWrite = false: rowptr[r] = kept entries of row r
// (counted in place; scan_one<RowptrOp> turns them into offsets).  kWrite = true: they go to [rowptr[r], rowptr[r + 1]) of edge_index_out
// [2, E_b] (local row, local column), prob_out (prob[id]) and eid_out (id); every write is guarded by pos < E_b.  HUB ROWS: a row of
// more than kHub entries is not walked by its own wave; after the short rows of a workgroup are done, all its waves walk each hub row
// together in contiguous 64-aligned slices.  The slice counts go through an LDS table [hub row of the tile][wave]; the fill counts the
// slices first and offsets each by the kept counts before it.  A hub therefore costs len / kThreads steps of one workgroup, twice,
// instead of len / 64 steps of one wave.  A policy P (passed by value) answers three questions:
//   RowSpan row(lds, r)            which entries [beg, end) of the CSR arrays are local row r (empty when its node is out of range), and
//                                  its source node
//   bool keep(lds, e, lc, id)      is entry e kept; if so its local column and its edge id
//   void side_work(r, src, lane)   per-row work of the COUNT pass, by the row's wave (the cluster collate gathers byte attributes here)
// and may own an LDS block: P::Lds, filled by stage(lds) (every thread, before a barrier) when P::kStaged.
#pragma once
#include "sgs_common.h"

namespace sgs {
namespace {

constexpr int kST = 1024;                   // threads of the single-workgroup scans
constexpr int kSPer = 4;                    // items per thread and tile there

template <class Op>
__global__ void __launch_bounds__(kST) scan_one(Op op, int64_t n) {
    __shared__ int wtot[2][kST / kWave];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int64_t carry = 0;
    int buf = 0;
    for (int64_t base = 0; base < n; base += kST * kSPer, buf ^= 1) {
        const int64_t i = base + static_cast<int64_t>(threadIdx.x) * kSPer;
        int v[kSPer];
        int mine = 0;
#pragma unroll
        for (int j = 0; j < kSPer; ++j) {
            v[j] = i + j < n ? op.load(i + j) : 0;
            mine += v[j];
        }
        int inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wtot[buf][wid] = inc;
        __syncthreads();                            // (two LDS rows alternate: one barrier per tile)
        int64_t run = carry + (inc - mine);
        int64_t total = 0;
#pragma unroll
        for (int w = 0; w < kST / kWave; ++w) {
            const int t = wtot[buf][w];
            run += w < wid ? t : 0;
            total += t;
        }
#pragma unroll
        for (int j = 0; j < kSPer; ++j) {
            if (i + j < n) op.store(i + j, run, v[j]);
            run += v[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0) op.finish(carry);
}

struct RowptrOp {                                   // counts -> exclusive prefix, in place
    int64_t* rowptr;
    int64_t n;
    int64_t* total;
    int64_t E_b;                                    // the host's edge count, compared with the total when `mismatch` is given
    int* mismatch;
    __device__ int load(int64_t i) const { return static_cast<int>(rowptr[i]); }
    __device__ void store(int64_t i, int64_t before, int) const { rowptr[i] = before; }
    __device__ void finish(int64_t t) const {
        rowptr[n] = t;
        if (total) *total = t;
        if (mismatch && t != E_b) *mismatch = 1;
    }
};

struct RowSpan {
    int64_t beg, end, src;
};

// One wave walks the entries [beg, end) of a source row.  kWrite: the kept ones go to positions out_base, out_base + 1, ...
// Returns the kept count (the same in every lane).
template <bool kWrite, class P>
__device__ __forceinline__ int squeeze_span(const P& p, const typename P::Lds& lds, int64_t beg, int64_t end, int64_t out_base, int64_t local_row,
                                            int64_t E_b, const float* __restrict__ prob, int64_t* __restrict__ ei_out,
                                            float* __restrict__ prob_out, int64_t* __restrict__ eid_out) {
    const int lane = threadIdx.x & 63;
    int run = 0;
    for (int64_t b = beg; b < end; b += kWave) {
        const int64_t e = b + lane;
        int64_t lc = 0, id = 0;
        const bool in = e < end && p.keep(lds, e, lc, id);
        const unsigned long long m = __ballot(in);
        if (kWrite && in) {
            const int64_t pos = out_base + run + __popcll(m & ((1ull << lane) - 1ull));
            // (a host E_b that disagrees with the device count is reported by the caller's mismatch word; nothing leaves [0, E_b))
            if (static_cast<uint64_t>(pos) < static_cast<uint64_t>(E_b)) {
                ei_out[pos] = local_row;
                ei_out[E_b + pos] = lc;
                if (prob_out) prob_out[pos] = prob[id];
                if (eid_out) eid_out[pos] = id;
            }
        }
        run += __popcll(m);
    }
    return run;
}

template <class P, int kThreads, int kHub, bool kWrite>
__global__ void __launch_bounds__(kThreads) squeeze_rows(const P p, int64_t n, int64_t E_b, int64_t* __restrict__ rowptr,
                                                         const float* __restrict__ prob, int64_t* __restrict__ ei_out,
                                                         float* __restrict__ prob_out, int64_t* __restrict__ eid_out) {
    constexpr int kW = kThreads / kWave;            // local rows per workgroup (one wave each)
    __shared__ typename P::Lds lds;
    __shared__ int64_t s_beg[kW], s_end[kW];
    __shared__ int s_part[kW][kW];                  // [hub row of the workgroup][wave]: kept count of that wave's slice
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if constexpr (P::kStaged) {
        p.stage(lds);
        __syncthreads();
    }
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kW + wid;
    int64_t beg = 0, end = 0;
    if (r < n) {
        const RowSpan s = p.row(lds, r);
        beg = s.beg;
        end = s.end;
        if (!kWrite) p.side_work(r, s.src, lane);
    }
    if (lane == 0) { s_beg[wid] = beg; s_end[wid] = end; }
    if (r < n && end - beg <= kHub) {
        const int c = squeeze_span<kWrite>(p, lds, beg, end, kWrite ? rowptr[r] : 0, r, E_b, prob, ei_out, prob_out, eid_out);
        if (!kWrite && lane == 0) rowptr[r] = c;
    }
    __syncthreads();
    // hub rows of this workgroup (the conditions below read LDS only: uniform over the workgroup, so every barrier is met by all)
    bool any_hub = false;
    for (int h = 0; h < kW; ++h) any_hub = any_hub || (s_end[h] - s_beg[h] > kHub);
    if (!any_hub) return;
    for (int h = 0; h < kW; ++h) {
        const int64_t hb = s_beg[h], he = s_end[h];
        if (he - hb <= kHub) continue;
        const int64_t slice = ((he - hb + kW - 1) / kW + kWave - 1) / kWave * kWave;
        const int64_t b0 = hb + slice * wid < he ? hb + slice * wid : he;
        const int64_t b1 = b0 + slice < he ? b0 + slice : he;
        const int64_t hr = static_cast<int64_t>(blockIdx.x) * kW + h;
        const int c = squeeze_span<false>(p, lds, b0, b1, 0, hr, E_b, prob, ei_out, prob_out, eid_out);
        if (lane == 0) s_part[h][wid] = c;
    }
    __syncthreads();
    for (int h = 0; h < kW; ++h) {
        const int64_t hb = s_beg[h], he = s_end[h];
        if (he - hb <= kHub) continue;
        const int64_t hr = static_cast<int64_t>(blockIdx.x) * kW + h;
        int before = 0, total = 0;
        for (int w = 0; w < kW; ++w) {
            const int t = s_part[h][w];
            before += w < wid ? t : 0;
            total += t;
        }
        if (!kWrite) {
            if (wid == h && lane == 0) rowptr[hr] = total;
        } else {
            const int64_t slice = ((he - hb + kW - 1) / kW + kWave - 1) / kWave * kWave;
            const int64_t b0 = hb + slice * wid < he ? hb + slice * wid : he;
            const int64_t b1 = b0 + slice < he ? b0 + slice : he;
            squeeze_span<true>(p, lds, b0, b1, rowptr[hr] + before, hr, E_b, prob, ei_out, prob_out, eid_out);
        }
    }
}

}  // namespace
}  // namespace sgs
