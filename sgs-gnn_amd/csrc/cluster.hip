// Multi-partition batches (Cluster-GCN's "stochastic multiple partitions"): the edge list of the union of k partitions, cut edges
// between them restored, squeezed out of the whole graph's row-sorted CSR (gfx950).
//
// Reference: ClusterLoader(cluster_data, batch_size=k) (main.py:63-65 builds it with batch_size=1): its collate concatenates the k
// partitions' node ranges, keeps every edge with both endpoints in them and relabels.  The nodes are stored grouped by partition, so
// partition p owns the node range [node_ptr[p], node_ptr[p+1]) and a group {p_1 < ... < p_k} is k sorted, disjoint ranges.  They
// travel BY VALUE in the kernel arguments (no device-side table to refill per batch); membership of a column and its local id are
// one binary search over the k range starts, the source row of a local row is the same search over the k prefix sums.  The group is
// ascending, so relabelling is monotone: the kept columns of a row keep their order and the output is row-sorted without a sort.
//
// Three launches: count per row -> scan -> fill.  One wave per local row, 64 columns per step, a ballot gives the kept count / the
// output positions (the sgs_graph_filter pattern).  HUB ROWS: a row longer than kHubDeg is not walked by its own wave; after the
// short rows of a workgroup are done, its 16 waves walk each hub row together (16 contiguous slices; the fill counts the slices
// first and offsets each by the kept counts before it).  A hub therefore costs deg / 1024 steps of one workgroup instead of
// deg / 64 steps of one wave.  Integer work only: prob_out is a gather.  No atomics.
#include "sgs_common.h"

namespace sgs {
namespace {

constexpr int kMaxParts = 32;
constexpr int kCT = 1024;               // threads per workgroup of the row kernels
constexpr int kRows = kCT / kWave;      // local rows per workgroup (one wave each)
constexpr int kHubDeg = 1024;           // rows longer than this are walked by the whole workgroup
constexpr int kMaxBytesAttr = 4;        // per-node byte attributes gathered beside the edges (the three masks)

struct ClusterArgs {
    int64_t lo[kMaxParts];              // node range of part j in the whole graph's (partition-grouped) numbering
    int64_t hi[kMaxParts];
    int64_t pre[kMaxParts + 1];         // local id of part j's first node; pre[k] = n_b
    int k;
};

// largest j in [0, k) with a[j] <= v, or -1
__device__ __forceinline__ int last_le(const int64_t* a, int k, int64_t v) {
    int l = 0, h = k;
    while (l < h) {
        const int m = (l + h) >> 1;
        if (a[m] <= v) l = m + 1;
        else h = m;
    }
    return l - 1;
}

// One wave walks the columns [beg, end) of a source row.  kWrite: the kept ones go to positions out_base, out_base + 1, ...
// Returns the kept count (the same in every lane).
template <bool kWrite>
__device__ __forceinline__ int walk_span(const int64_t* __restrict__ col, const float* __restrict__ prob, int64_t beg, int64_t end,
                                         const int64_t* s_lo, const int64_t* s_hi, const int64_t* s_pre, int k, int64_t out_base,
                                         int64_t local_row, int64_t E_b, int64_t* __restrict__ ei_out, float* __restrict__ prob_out,
                                         int64_t* __restrict__ eid_out) {
    const int lane = threadIdx.x & 63;
    int run = 0;
    for (int64_t b = beg; b < end; b += kWave) {
        const int64_t e = b + lane;
        bool in = false;
        int64_t lc = 0;
        if (e < end) {
            const int64_t c = col[e];
            const int j = last_le(s_lo, k, c);
            if (j >= 0 && c < s_hi[j]) {
                in = true;
                lc = s_pre[j] + (c - s_lo[j]);
            }
        }
        const unsigned long long m = __ballot(in);
        if (kWrite && in) {
            const int64_t pos = out_base + run + __popcll(m & ((1ull << lane) - 1ull));
            // (a host E_b that disagrees with the device count is reported through the mismatch word; nothing leaves [0, E_b))
            if (static_cast<uint64_t>(pos) < static_cast<uint64_t>(E_b)) {
                ei_out[pos] = local_row;
                ei_out[E_b + pos] = lc;
                if (prob_out) prob_out[pos] = prob[e];
                if (eid_out) eid_out[pos] = e;
            }
        }
        run += __popcll(m);
    }
    return run;
}

// kWrite = false: cnt[r] = kept columns of local row r (+ the per-node byte attributes, gathered by the row's wave).
// kWrite = true : the kept columns of row r go to [rowptr[r], rowptr[r + 1]).
template <bool kWrite>
__global__ void __launch_bounds__(kCT) cluster_rows(const ClusterArgs a, const int64_t* __restrict__ full_ptr, const int64_t* __restrict__ full_col,
                                                    const float* __restrict__ full_prob, int64_t n_b, int64_t E_b, int* __restrict__ cnt,
                                                    const int64_t* __restrict__ rowptr, int64_t* __restrict__ ei_out,
                                                    float* __restrict__ prob_out, int64_t* __restrict__ eid_out,
                                                    const uint8_t* __restrict__ attr_in, uint8_t* __restrict__ attr_out, int n_attr,
                                                    int64_t N) {
    __shared__ int64_t s_lo[kMaxParts], s_hi[kMaxParts], s_pre[kMaxParts + 1];
    __shared__ int64_t s_beg[kRows], s_end[kRows];
    __shared__ int s_part[kRows][kRows];            // [hub row of the workgroup][wave]: kept count of that wave's slice
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int k = a.k;
    if (threadIdx.x < kMaxParts) {
        s_lo[threadIdx.x] = a.lo[threadIdx.x];
        s_hi[threadIdx.x] = a.hi[threadIdx.x];
    }
    if (threadIdx.x <= kMaxParts) s_pre[threadIdx.x] = a.pre[threadIdx.x];
    __syncthreads();
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kRows + wid;
    int64_t beg = 0, end = 0;
    if (r < n_b) {
        const int j = last_le(s_pre, k, r);
        const int64_t src = s_lo[j] + (r - s_pre[j]);
        beg = full_ptr[src];
        end = full_ptr[src + 1];
        if (!kWrite && lane < n_attr) attr_out[static_cast<int64_t>(lane) * n_b + r] = attr_in[static_cast<int64_t>(lane) * N + src];
    }
    if (lane == 0) { s_beg[wid] = beg; s_end[wid] = end; }
    if (r < n_b && end - beg <= kHubDeg) {
        const int n = walk_span<kWrite>(full_col, full_prob, beg, end, s_lo, s_hi, s_pre, k, kWrite ? rowptr[r] : 0, r, E_b, ei_out,
                                        prob_out, eid_out);
        if (!kWrite && lane == 0) cnt[r] = n;
    }
    __syncthreads();
    // hub rows of this workgroup (the conditions below read LDS only: uniform over the workgroup, so every barrier is met by all)
    bool any_hub = false;
    for (int h = 0; h < kRows; ++h) any_hub = any_hub || (s_end[h] - s_beg[h] > kHubDeg);
    if (!any_hub) return;
    for (int h = 0; h < kRows; ++h) {
        const int64_t hb = s_beg[h], he = s_end[h];
        if (he - hb <= kHubDeg) continue;
        const int64_t slice = ((he - hb + kRows - 1) / kRows + kWave - 1) / kWave * kWave;
        const int64_t b0 = hb + slice * wid < he ? hb + slice * wid : he;
        const int64_t b1 = b0 + slice < he ? b0 + slice : he;
        const int64_t hr = static_cast<int64_t>(blockIdx.x) * kRows + h;
        const int n = walk_span<false>(full_col, full_prob, b0, b1, s_lo, s_hi, s_pre, k, 0, hr, E_b, ei_out, prob_out, eid_out);
        if (lane == 0) s_part[h][wid] = n;
    }
    __syncthreads();
    for (int h = 0; h < kRows; ++h) {
        const int64_t hb = s_beg[h], he = s_end[h];
        if (he - hb <= kHubDeg) continue;
        const int64_t hr = static_cast<int64_t>(blockIdx.x) * kRows + h;
        int before = 0, total = 0;
        for (int w = 0; w < kRows; ++w) {
            const int t = s_part[h][w];
            before += w < wid ? t : 0;
            total += t;
        }
        if (!kWrite) {
            if (wid == h && lane == 0) cnt[hr] = total;
        } else {
            const int64_t slice = ((he - hb + kRows - 1) / kRows + kWave - 1) / kWave * kWave;
            const int64_t b0 = hb + slice * wid < he ? hb + slice * wid : he;
            const int64_t b1 = b0 + slice < he ? b0 + slice : he;
            walk_span<true>(full_col, full_prob, b0, b1, s_lo, s_hi, s_pre, k, rowptr[hr] + before, hr, E_b, ei_out, prob_out, eid_out);
        }
    }
}

// Exclusive scan of the n_b row counts -> rowptr[n_b + 1] (int64), one workgroup: tiles of 4096 counts, four per thread, wave scan +
// the 16 wave totals through LDS, a running carry (the scan of gcn.hip's CSR build).  Thread 0 compares the total with the host's
// E_b and publishes it.
__global__ void __launch_bounds__(kCT) cluster_scan(const int* __restrict__ cnt, int64_t n_b, int64_t* __restrict__ rowptr, int64_t E_b,
                                                    int* __restrict__ mismatch, int64_t* __restrict__ total_out) {
    __shared__ int wtot[2][16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int64_t carry = 0;
    int buf = 0;
    for (int64_t base = 0; base < n_b; base += 4096, buf ^= 1) {
        const int64_t i = base + static_cast<int64_t>(threadIdx.x) * 4;
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < n_b ? cnt[i + j] : 0;
        const int mine = (v[0] + v[1]) + (v[2] + v[3]);
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
        for (int w = 0; w < 16; ++w) {
            const int t = wtot[buf][w];
            run += w < wid ? t : 0;
            total += t;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < n_b) rowptr[i + j] = run;
            run += v[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        rowptr[n_b] = carry;
        if (total_out) *total_out = carry;
        if (mismatch && carry != E_b) *mismatch = 1;
    }
}

struct Plan {
    ClusterArgs a;
    int* cnt;
    int64_t* rowptr;
};

size_t ws_bytes_for(int64_t n_b) {
    const size_t n = static_cast<size_t>(n_b > 0 ? n_b : 0);
    return carve_bytes(n + 1, sizeof(int)) + carve_bytes(n + 1, sizeof(int64_t));
}

// Checks the host descriptors and carves the workspace.  ranges_host [k][2] = {lo, hi} of each part, ascending and disjoint.
int make_plan(const char* who, const int64_t* ranges_host, int64_t k, int64_t n_b, void* ws, size_t ws_bytes, Plan& p) {
    SGS_REQUIRE(k >= 1 && k <= kMaxParts, SGS_EINVAL, "%s: k = %lld parts, must be in [1, %d]", who, (long long)k, kMaxParts);
    SGS_REQUIRE(ranges_host != nullptr, SGS_EINVAL, "%s: null range table", who);
    SGS_REQUIRE(n_b >= 0 && n_b < (int64_t(1) << 31), SGS_EINVAL, "%s: n_b out of range", who);
    p.a = ClusterArgs{};
    int64_t pre = 0, last_hi = 0;
    for (int64_t j = 0; j < k; ++j) {
        const int64_t lo = ranges_host[2 * j], hi = ranges_host[2 * j + 1];
        SGS_REQUIRE(lo >= 0 && hi >= lo, SGS_EINVAL, "%s: part %lld: bad node range [%lld, %lld)", who, (long long)j, (long long)lo, (long long)hi);
        SGS_REQUIRE(j == 0 || lo >= last_hi, SGS_EINVAL, "%s: part %lld: node ranges must be ascending and must not overlap (unsorted group?)", who,
                    (long long)j);
        p.a.lo[j] = lo; p.a.hi[j] = hi; p.a.pre[j] = pre;
        pre += hi - lo;
        last_hi = hi;
    }
    p.a.pre[k] = pre;
    // unused tail: empty ranges past every node, so that a search over all kMaxParts entries would still be well defined
    for (int64_t j = k; j < kMaxParts; ++j) { p.a.lo[j] = last_hi; p.a.hi[j] = last_hi; p.a.pre[j + 1] = pre; }
    p.a.k = static_cast<int>(k);
    SGS_REQUIRE(pre == n_b, SGS_EINVAL, "%s: the ranges hold %lld nodes, n_b = %lld", who, (long long)pre, (long long)n_b);
    SGS_REQUIRE(ws && ws_bytes >= ws_bytes_for(n_b), SGS_EINVAL, "%s: workspace too small", who);
    SGS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, SGS_EINVAL, "%s: workspace must be 8-byte aligned", who);
    Carver c(ws);
    p.cnt = c.take<int>(static_cast<size_t>(n_b) + 1);
    p.rowptr = c.take<int64_t>(static_cast<size_t>(n_b) + 1);
    return SGS_OK;
}

}  // namespace
}  // namespace sgs

extern "C" {

int sgs_cluster_collate_max_parts(void) { return sgs::kMaxParts; }

size_t sgs_cluster_collate_workspace_bytes(int64_t n_b) { return sgs::ws_bytes_for(n_b); }

int sgs_cluster_collate_count(const int64_t* full_ptr, const int64_t* full_col, const int64_t* ranges_host, int64_t k, int64_t n_b,
                              int64_t* total_dev, void* ws, size_t ws_bytes, sgs_stream_t stream) {
    using namespace sgs;
    Plan p;
    const int rc = make_plan("sgs_cluster_collate_count", ranges_host, k, n_b, ws, ws_bytes, p);
    if (rc != SGS_OK) return rc;
    SGS_REQUIRE(full_ptr && full_col && total_dev, SGS_EINVAL, "sgs_cluster_collate_count: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_b > 0) {
        hipLaunchKernelGGL(cluster_rows<false>, dim3(static_cast<unsigned>(cdiv(n_b, kRows))), dim3(kCT), 0, st, p.a, full_ptr, full_col,
                           static_cast<const float*>(nullptr), n_b, int64_t(0), p.cnt, static_cast<const int64_t*>(nullptr),
                           static_cast<int64_t*>(nullptr), static_cast<float*>(nullptr), static_cast<int64_t*>(nullptr),
                           static_cast<const uint8_t*>(nullptr), static_cast<uint8_t*>(nullptr), 0, int64_t(0));
        SGS_LAUNCH_OK();
    }
    hipLaunchKernelGGL(cluster_scan, dim3(1), dim3(kCT), 0, st, p.cnt, n_b, p.rowptr, int64_t(0), static_cast<int*>(nullptr), total_dev);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_cluster_collate(const int64_t* full_ptr, const int64_t* full_col, const float* full_prob, const int64_t* ranges_host, int64_t k,
                        int64_t n_b, int64_t E_b, int64_t* edge_index_out, float* prob_out, int64_t* eid_out, const uint8_t* attr_in,
                        uint8_t* attr_out, int64_t n_attr, int64_t N, int32_t* mismatch_dev, void* ws, size_t ws_bytes,
                        sgs_stream_t stream) {
    using namespace sgs;
    Plan p;
    const int rc = make_plan("sgs_cluster_collate", ranges_host, k, n_b, ws, ws_bytes, p);
    if (rc != SGS_OK) return rc;
    SGS_REQUIRE(E_b >= 0 && E_b < (int64_t(1) << 31), SGS_EINVAL, "sgs_cluster_collate: E_b out of range");
    SGS_REQUIRE(full_ptr && full_col && (E_b == 0 || edge_index_out), SGS_EINVAL, "sgs_cluster_collate: null pointer");
    SGS_REQUIRE(prob_out == nullptr || full_prob != nullptr, SGS_EINVAL, "sgs_cluster_collate: prob_out without full_prob");
    SGS_REQUIRE(n_attr >= 0 && n_attr <= kMaxBytesAttr && (n_attr == 0 || (attr_in && attr_out && N >= p.a.hi[k - 1])), SGS_EINVAL,
                "sgs_cluster_collate: bad node attribute arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_b > 0) {
        hipLaunchKernelGGL(cluster_rows<false>, dim3(static_cast<unsigned>(cdiv(n_b, kRows))), dim3(kCT), 0, st, p.a, full_ptr, full_col,
                           full_prob, n_b, E_b, p.cnt, static_cast<const int64_t*>(nullptr), static_cast<int64_t*>(nullptr),
                           static_cast<float*>(nullptr), static_cast<int64_t*>(nullptr), attr_in, attr_out, static_cast<int>(n_attr), N);
        SGS_LAUNCH_OK();
    }
    hipLaunchKernelGGL(cluster_scan, dim3(1), dim3(kCT), 0, st, p.cnt, n_b, p.rowptr, E_b, mismatch_dev, static_cast<int64_t*>(nullptr));
    SGS_LAUNCH_OK();
    if (n_b > 0 && E_b > 0) {
        hipLaunchKernelGGL(cluster_rows<true>, dim3(static_cast<unsigned>(cdiv(n_b, kRows))), dim3(kCT), 0, st, p.a, full_ptr, full_col,
                           full_prob, n_b, E_b, static_cast<int*>(nullptr), p.rowptr, edge_index_out, prob_out, eid_out,
                           static_cast<const uint8_t*>(nullptr), static_cast<uint8_t*>(nullptr), 0, N);
        SGS_LAUNCH_OK();
    }
    return SGS_OK;
}

}  // extern "C"
