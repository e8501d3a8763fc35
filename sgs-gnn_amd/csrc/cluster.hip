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
// Three launches: count per row -> scan -> fill, all three the shared kernels of csrc/batch_rows.h (the row squeeze with its hub
// form, the single-workgroup scan; the neighbour loader's induced collate runs the same two).  This file holds what is the cluster
// collate's own: the policy `ClusterRows` (the range searches and the byte-attribute gather of the count pass), the launch shape --
// kCT = 1024 threads, 16 rows per workgroup, a row longer than kHubDeg = 1024 walked by all 16 waves --, the checks of the host's
// range table and the entry points.  The workspace is the int64 rowptr alone: the count pass writes the counts into it and the scan
// turns them into offsets in place, compares the total with the host's E_b and sets the mismatch word.  Integer work only: prob_out
// is a gather.  No atomics.
#include "batch_rows.h"

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

// The squeeze's policy (csrc/batch_rows.h): the three range tables live in LDS; local row r and a column's membership / local id are
// one binary search each; an entry's id is its position in full_col; the count pass gathers the node's byte attributes.
struct ClusterRows {
    static constexpr bool kStaged = true;
    struct Lds {
        int64_t lo[kMaxParts], hi[kMaxParts], pre[kMaxParts + 1];
    };
    ClusterArgs a;
    const int64_t* full_ptr;
    const int64_t* full_col;
    const uint8_t* attr_in;
    uint8_t* attr_out;
    int n_attr;
    int64_t n_b, N;
    __device__ void stage(Lds& s) const {
        if (threadIdx.x < kMaxParts) {
            s.lo[threadIdx.x] = a.lo[threadIdx.x];
            s.hi[threadIdx.x] = a.hi[threadIdx.x];
        }
        if (threadIdx.x <= kMaxParts) s.pre[threadIdx.x] = a.pre[threadIdx.x];
    }
    __device__ RowSpan row(const Lds& s, int64_t r) const {
        const int j = last_le(s.pre, a.k, r);
        const int64_t src = s.lo[j] + (r - s.pre[j]);
        return RowSpan{full_ptr[src], full_ptr[src + 1], src};
    }
    __device__ void side_work(int64_t r, int64_t src, int lane) const {
        if (lane < n_attr) attr_out[static_cast<int64_t>(lane) * n_b + r] = attr_in[static_cast<int64_t>(lane) * N + src];
    }
    __device__ bool keep(const Lds& s, int64_t e, int64_t& lc, int64_t& id) const {
        const int64_t c = full_col[e];
        const int j = last_le(s.lo, a.k, c);
        if (j < 0 || c >= s.hi[j]) return false;
        lc = s.pre[j] + (c - s.lo[j]);
        id = e;
        return true;
    }
};

struct Plan {
    ClusterArgs a;
    int64_t* rowptr;
};

size_t ws_bytes_for(int64_t n_b) { return carve_bytes(static_cast<size_t>(n_b > 0 ? n_b : 0) + 1, sizeof(int64_t)); }

// count (kWrite = false: into rowptr, in place) or fill of the n_b local rows
template <bool kWrite>
void launch_rows(const ClusterRows& rows, int64_t E_b, int64_t* rowptr, const float* full_prob, int64_t* ei_out, float* prob_out, int64_t* eid_out,
                 hipStream_t st) {
    hipLaunchKernelGGL((squeeze_rows<ClusterRows, kCT, kHubDeg, kWrite>), dim3(static_cast<unsigned>(cdiv(rows.n_b, kRows))), dim3(kCT), 0, st, rows,
                       rows.n_b, E_b, rowptr, full_prob, ei_out, prob_out, eid_out);
}

// Checks the host descriptors and the workspace (rowptr[n_b + 1], counted and scanned in place).  ranges_host [k][2] = {lo, hi} of each part, ascending and disjoint.
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
    p.rowptr = static_cast<int64_t*>(ws);
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
        launch_rows<false>(ClusterRows{p.a, full_ptr, full_col, nullptr, nullptr, 0, n_b, 0}, 0, p.rowptr, nullptr, nullptr, nullptr, nullptr, st);
        SGS_LAUNCH_OK();
    }
    hipLaunchKernelGGL(scan_one<RowptrOp>, dim3(1), dim3(kST), 0, st, RowptrOp{p.rowptr, n_b, total_dev, 0, nullptr}, n_b);
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
    const ClusterRows rows{p.a, full_ptr, full_col, attr_in, attr_out, static_cast<int>(n_attr), n_b, N};
    if (n_b > 0) {
        launch_rows<false>(rows, E_b, p.rowptr, full_prob, nullptr, nullptr, nullptr, st);
        SGS_LAUNCH_OK();
    }
    hipLaunchKernelGGL(scan_one<RowptrOp>, dim3(1), dim3(kST), 0, st, RowptrOp{p.rowptr, n_b, nullptr, E_b, mismatch_dev}, n_b);
    SGS_LAUNCH_OK();
    if (n_b > 0 && E_b > 0) {
        launch_rows<true>(rows, E_b, p.rowptr, full_prob, edge_index_out, prob_out, eid_out, st);
        SGS_LAUNCH_OK();
    }
    return SGS_OK;
}

}  // extern "C"
