// K4 / K5: graph preparation, gcn_norm and weighted CSR SpMM / SDDMM for the GCN layers (gfx950).
//
// Reference: PyG 2.3.1 GCNConv as called at model.py:94-95,107-111 (scorer encoder) and
// model.py:151-153,159-161 (GNNModel): add_remaining_self_loops -> deg = scatter_add(w, dst)
// -> w_hat = deg^-1/2[src] w deg^-1/2[dst] -> out[dst] += w_hat x'[src] -> + bias.
// The reference materialises [nnz, D] messages and scatter-adds them (atomics on GPU); here
// the aggregation is a gather over a dst-sorted CSR (no float atomics, deterministic), and
// the transposed pass of backward is the same kernel over the src-sorted CSR.
//
// All kernels are HBM/L2-bandwidth bound gathers: per nnz 4 B col + 4 B weight + 4*D B row.
#include "sgs_common.h"
#include "spmm_plan.h"

namespace sgs {
size_t graph_sort_workspace_bytes(int64_t n, int64_t N);
size_t graph_src_sorted_workspace_bytes(int64_t n, int64_t N);
int graph_build_src_sorted(const int64_t* ei, int64_t n, int64_t N, int32_t* in_ptr, int32_t* in_src, int32_t* in_eid, int32_t* out_ptr,
                           int32_t* out_dst, int32_t* out_eid, int32_t* loop_eid, int32_t* unsorted_flag, void* ws, size_t ws_bytes,
                           hipStream_t stream);
int graph_build_by_sort(const int64_t* ei, int64_t n, int64_t N, int32_t* in_ptr, int32_t* in_src, int32_t* in_eid, int32_t* out_ptr,
                        int32_t* out_dst, int32_t* out_eid, int32_t* loop_eid, void* ws, size_t ws_bytes, hipStream_t stream);
}

namespace sgs {
namespace {

constexpr int kT = 256;
constexpr int kMaxLdsRow = 8192;   // longest row sorted in LDS (32 KiB)

// ---------------------------------------------------------------- CSR build
__global__ void __launch_bounds__(kT) count_degrees(const int64_t* __restrict__ ei, int64_t n_edges, int* __restrict__ cnt_in,
                                                   int* __restrict__ cnt_out, int* __restrict__ loop_eid) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (e >= n_edges) return;
    const int s = static_cast<int>(ei[e]), d = static_cast<int>(ei[n_edges + e]);
    atomicAdd(&cnt_in[d], 1);
    atomicAdd(&cnt_out[s], 1);
    if (s == d) atomicMax(&loop_eid[s], static_cast<int>(e));   // PyG: the last existing loop wins
}

// blockIdx.x = 0: in-direction, 1: out-direction.  Exclusive scan of N counts -> ptr[N+1]; also initialises the fill cursors.
// Tiles of 4096 consecutive counts, four per thread (coalesced), wave scan + the 16 wave totals through LDS, a running carry; the next
// tile's counts are loaded before this tile's barrier.  (Each thread scanning its own N / 1024 consecutive counts -- every access of a
// wave a different cache line -- took 70 us at N = 33 869.)
__device__ __forceinline__ void scan_counts_body(const int* __restrict__ cnt, int64_t N, int* __restrict__ ptr, int* __restrict__ cur) {
    __shared__ int wtot[2][16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    auto load4 = [&](int64_t i, int (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < N ? cnt[i + j] : 0;
    };
    int carry = 0, buf = 0;
    int v[4], vn[4];
    load4(static_cast<int64_t>(threadIdx.x) * 4, v);
    for (int64_t base = 0; base < N; base += 4096, buf ^= 1) {
        const int64_t i = base + static_cast<int64_t>(threadIdx.x) * 4;
        load4(i + 4096, vn);
        const int mine = (v[0] + v[1]) + (v[2] + v[3]);
        int inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wtot[buf][wid] = inc;
        __syncthreads();                            // (two LDS rows alternate: one barrier per tile)
        int run = carry + inc - mine, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int t = wtot[buf][w];
            run += w < wid ? t : 0;
            total += t;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < N) { ptr[i + j] = run; cur[i + j] = run; }
            run += v[j];
            v[j] = vn[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0) ptr[N] = carry;
}
__global__ void __launch_bounds__(1024) scan_counts(const int* __restrict__ cnt_in, const int* __restrict__ cnt_out,
                                                   int64_t N, int* __restrict__ in_ptr, int* __restrict__ out_ptr,
                                                   int* __restrict__ cur_in, int* __restrict__ cur_out) {
    if (blockIdx.x == 0) scan_counts_body(cnt_in, N, in_ptr, cur_in);
    else scan_counts_body(cnt_out, N, out_ptr, cur_out);
}

__global__ void __launch_bounds__(kT) fill_rows(const int64_t* __restrict__ ei, int64_t n_edges, int* __restrict__ cur_in,
                                               int* __restrict__ cur_out, int* __restrict__ tmp_in, int* __restrict__ tmp_out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (e >= n_edges) return;
    const int s = static_cast<int>(ei[e]), d = static_cast<int>(ei[n_edges + e]);
    tmp_in[atomicAdd(&cur_in[d], 1)] = static_cast<int>(e);
    tmp_out[atomicAdd(&cur_out[s], 1)] = static_cast<int>(e);
}

// Small-N variants (N <= kLdsNodes, e.g. METIS partitions): every edge hammering ~1k global counters
// is contention-bound, so a workgroup first counts / ranks its chunk of edges in LDS and touches each
// global counter at most once per chunk.
constexpr int kLdsNodes = 4096;
constexpr int kEdgesPerBlock = 4096;      // 16 per thread
__global__ void __launch_bounds__(kT) count_degrees_lds(const int64_t* __restrict__ ei, int64_t n_edges, int N, int* __restrict__ cnt_in,
                                                       int* __restrict__ cnt_out, int* __restrict__ loop_eid) {
    __shared__ int lin[kLdsNodes], lout[kLdsNodes];
    for (int i = threadIdx.x; i < N; i += kT) { lin[i] = 0; lout[i] = 0; }
    __syncthreads();
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kEdgesPerBlock;
    for (int it = 0; it < kEdgesPerBlock / kT; ++it) {
        const int64_t e = base + it * kT + threadIdx.x;
        if (e < n_edges) {
            const int s = static_cast<int>(ei[e]), d = static_cast<int>(ei[n_edges + e]);
            atomicAdd(&lin[d], 1);
            atomicAdd(&lout[s], 1);
            if (s == d) atomicMax(&loop_eid[s], static_cast<int>(e));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += kT) {
        if (lin[i]) atomicAdd(&cnt_in[i], lin[i]);
        if (lout[i]) atomicAdd(&cnt_out[i], lout[i]);
    }
}

__global__ void __launch_bounds__(kT) fill_rows_lds(const int64_t* __restrict__ ei, int64_t n_edges, int N, int* __restrict__ cur_in,
                                                   int* __restrict__ cur_out, int* __restrict__ tmp_in, int* __restrict__ tmp_out) {
    __shared__ int lin[kLdsNodes], lout[kLdsNodes];
    for (int i = threadIdx.x; i < N; i += kT) { lin[i] = 0; lout[i] = 0; }
    __syncthreads();
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kEdgesPerBlock;
    int rs[kEdgesPerBlock / kT], rd[kEdgesPerBlock / kT], ss[kEdgesPerBlock / kT], dd[kEdgesPerBlock / kT];
#pragma unroll
    for (int it = 0; it < kEdgesPerBlock / kT; ++it) {
        const int64_t e = base + it * kT + threadIdx.x;
        ss[it] = -1;
        if (e < n_edges) {
            ss[it] = static_cast<int>(ei[e]);
            dd[it] = static_cast<int>(ei[n_edges + e]);
            rd[it] = atomicAdd(&lin[dd[it]], 1);      // rank inside this chunk
            rs[it] = atomicAdd(&lout[ss[it]], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += kT) {       // reserve this chunk's slots: one global atomic per touched node
        const int ci = lin[i], co = lout[i];
        lin[i] = ci ? atomicAdd(&cur_in[i], ci) : 0;
        lout[i] = co ? atomicAdd(&cur_out[i], co) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kEdgesPerBlock / kT; ++it) {
        if (ss[it] >= 0) {
            const int e = static_cast<int>(base + it * kT + threadIdx.x);
            tmp_in[lin[dd[it]] + rd[it]] = e;
            tmp_out[lout[ss[it]] + rs[it]] = e;
        }
    }
}

// The atomic fill leaves each row's edge ids in arrival order; sorting them (unique ints) makes
// the CSR -- and every floating-point sum over a row -- deterministic.
// Rows of <= 64 entries: one wave, bitonic network through lane shuffles.
__device__ __forceinline__ void sort_rows_wave_body(int64_t block, const int* __restrict__ in_ptr, const int* __restrict__ out_ptr, int64_t N,
                                                    const int* __restrict__ tmp_in, const int* __restrict__ tmp_out,
                                                    const int64_t* __restrict__ ei, int64_t n_edges, int* __restrict__ in_eid,
                                                    int* __restrict__ in_src, int* __restrict__ out_eid,
                                                    int* __restrict__ out_dst) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (block * kT + threadIdx.x) >> 6;
    if (r >= 2 * N) return;
    const bool out = r >= N;
    const int64_t row = out ? r - N : r;
    const int* ptr = out ? out_ptr : in_ptr;
    const int base = ptr[row], d = ptr[row + 1] - base;
    if (d == 0 || d > 64) return;
    const int* tmp = out ? tmp_out : tmp_in;
    int v = lane < d ? tmp[base + lane] : 0x7fffffff;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = __shfl_xor(v, j, 64);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            v = keep_min ? min(v, o) : max(v, o);
        }
    }
    if (lane < d) {
        if (out) { out_eid[base + lane] = v; out_dst[base + lane] = static_cast<int>(ei[n_edges + v]); }
        else     { in_eid[base + lane] = v;  in_src[base + lane] = static_cast<int>(ei[v]); }
    }
}

// Rows of > 64 entries: one block per row; bitonic sort in LDS up to kMaxLdsRow entries,
// rank-by-counting straight from L2 beyond that (hub rows).
__device__ __forceinline__ void sort_rows_block_body(int64_t r, int* a, const int* __restrict__ in_ptr, const int* __restrict__ out_ptr, int64_t N,
                                                     const int* __restrict__ tmp_in, const int* __restrict__ tmp_out,
                                                     const int64_t* __restrict__ ei, int64_t n_edges, int* __restrict__ in_eid,
                                                     int* __restrict__ in_src, int* __restrict__ out_eid,
                                                     int* __restrict__ out_dst) {
    const bool out = r >= N;
    const int64_t row = out ? r - N : r;
    const int* ptr = out ? out_ptr : in_ptr;
    const int base = ptr[row], d = ptr[row + 1] - base;
    if (d <= 64) return;
    const int* tmp = (out ? tmp_out : tmp_in) + base;
    int* eid_o = (out ? out_eid : in_eid) + base;
    int* col_o = (out ? out_dst : in_src) + base;
    const int64_t* colsrc = out ? ei + n_edges : ei;
    if (d <= kMaxLdsRow) {
        int n2 = 128;
        while (n2 < d) n2 <<= 1;
        for (int i = threadIdx.x; i < n2; i += kT) a[i] = i < d ? tmp[i] : 0x7fffffff;
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int idx = threadIdx.x; idx < (n2 >> 1); idx += kT) {
                    const int i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1));
                    const int p = i | j;
                    const int x = a[i], y = a[p];
                    const bool asc = (i & k) == 0;
                    if ((x > y) == asc) { a[i] = y; a[p] = x; }
                }
                __syncthreads();
            }
        }
        for (int i = threadIdx.x; i < d; i += kT) {
            const int v = a[i];
            eid_o[i] = v;
            col_o[i] = static_cast<int>(colsrc[v]);
        }
    } else {
        for (int i = threadIdx.x; i < d; i += kT) {
            const int v = tmp[i];
            int rank = 0;
            for (int j = 0; j < d; ++j) rank += (tmp[j] < v);
            eid_o[rank] = v;
            col_o[rank] = static_cast<int>(colsrc[v]);
        }
    }
}

// One launch for both row classes: the first `n_wave_blocks` workgroups sort the short rows (one wave each), the
// remaining 2N workgroups the long ones (one workgroup each; short rows return at once).
__global__ void __launch_bounds__(kT) sort_rows(int64_t n_wave_blocks, const int* __restrict__ in_ptr, const int* __restrict__ out_ptr, int64_t N,
                                               const int* __restrict__ tmp_in, const int* __restrict__ tmp_out,
                                               const int64_t* __restrict__ ei, int64_t n_edges, int* __restrict__ in_eid,
                                               int* __restrict__ in_src, int* __restrict__ out_eid, int* __restrict__ out_dst) {
    __shared__ int a[kMaxLdsRow];
    if (static_cast<int64_t>(blockIdx.x) < n_wave_blocks)
        sort_rows_wave_body(blockIdx.x, in_ptr, out_ptr, N, tmp_in, tmp_out, ei, n_edges, in_eid, in_src, out_eid, out_dst);
    else
        sort_rows_block_body(static_cast<int64_t>(blockIdx.x) - n_wave_blocks, a, in_ptr, out_ptr, N, tmp_in, tmp_out, ei, n_edges, in_eid,
                             in_src, out_eid, out_dst);
}

// ---------------------------------------------------------------- CSR of a SAMPLED subgraph from its parent's CSR
// A drawn subgraph keeps a subset of the parent's edges in their original order, so its CSR (both orientations, rows
// sorted by edge id) is the parent's CSR with the unselected entries squeezed out and the edge ids renumbered by rank:
// no atomics, no per-row sort.  Three launches instead of the five of sgs_graph_build, and none of them is the row sort
// (19 us at partition scale):  (1) one wave per parent row counts its selected entries; spare workgroups scatter
// pos[sampled_eid[j]] = j;  (2) scan_counts;  (3) one wave per parent row compacts its entries with a ballot prefix.
// Large parents (>= 8 M edges): the byte mask (E bytes) is first packed into a bit mask (E/8 bytes) so that the random
// `mask[eid]` lookups along the in-rows hit a 14 MB table (L2 / Infinity Cache resident) instead of a 114 MB one.
__global__ void __launch_bounds__(kT) pack_mask_bits(const uint8_t* __restrict__ mask, int64_t E, uint32_t* __restrict__ bits) {
    const int64_t w = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;        // one 32-edge word per thread
    if (w * 32 >= E) return;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int64_t e = w * 32 + j;
        if (e < E && mask[e]) v |= 1u << j;
    }
    bits[w] = v;
}
template <bool BITS>
__device__ __forceinline__ bool mask_at(const uint8_t* __restrict__ mask, int e) {
    if (BITS) return (reinterpret_cast<const uint32_t*>(mask)[e >> 5] >> (e & 31)) & 1u;
    return mask[e] != 0;
}

// nrows = 2N: in- and out-rows; N: in-rows only (the forward-only CSRs of sgs_graph_filter_multi)
template <bool BITS>
__device__ __forceinline__ void filter_count_scatter_body(const int* __restrict__ in_ptr, const int* __restrict__ in_eid,
                                                          const int* __restrict__ out_ptr, const int* __restrict__ out_eid, int64_t N,
                                                          const uint8_t* __restrict__ mask, const int64_t* __restrict__ sampled_eid,
                                                          int64_t q, int64_t n_row_blocks, int* __restrict__ cnt_in,
                                                          int* __restrict__ cnt_out, int* __restrict__ pos, int64_t nrows) {
    if (static_cast<int64_t>(blockIdx.x) >= n_row_blocks) {
        const int64_t j = (static_cast<int64_t>(blockIdx.x) - n_row_blocks) * kT + threadIdx.x;
        if (j < q) pos[sampled_eid[j]] = static_cast<int>(j);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int64_t r = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (r >= nrows) return;
    const bool out = r >= N;
    const int64_t row = out ? r - N : r;
    const int* ptr = out ? out_ptr : in_ptr;
    const int* eid = out ? out_eid : in_eid;
    int c = 0;
    const int b = ptr[row], e = ptr[row + 1];
    for (int k = b + lane; k < e; k += 256) {          // four entries per lane in flight: ids first, then their mask words
        int id[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) id[u] = eid[min(k + 64 * u, e - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool m = mask_at<BITS>(mask, id[u]);
            c += (k + 64 * u < e && m) ? 1 : 0;
        }
    }
    c = wave_sum_int_all(c);
    if (lane == 0) (out ? cnt_out : cnt_in)[row] = c;
}
template <bool BITS>
__global__ void __launch_bounds__(kT) filter_count_scatter(const int* __restrict__ in_ptr, const int* __restrict__ in_eid,
                                                          const int* __restrict__ out_ptr, const int* __restrict__ out_eid, int64_t N,
                                                          const uint8_t* __restrict__ mask, const int64_t* __restrict__ sampled_eid,
                                                          int64_t q, int64_t n_row_blocks, int* __restrict__ cnt_in,
                                                          int* __restrict__ cnt_out, int* __restrict__ pos) {
    filter_count_scatter_body<BITS>(in_ptr, in_eid, out_ptr, out_eid, N, mask, sampled_eid, q, n_row_blocks, cnt_in, cnt_out, pos, 2 * N);
}

// SCAN: the child row pointers are not there yet -- every wave sums the counts of the rows before its own (N <= kSelfScanRows: a few
// cached loads per lane) and writes its entry of the pointer array (the last row also the total): the scan launch between the count and
// the fill pass goes away (partition scale: one launch = ~5 us of a ~90 us draw-to-normalisation chain).
constexpr int64_t kSelfScanRows = 4096;
template <bool BITS, bool SCAN>
__device__ __forceinline__ void filter_fill_body(int64_t nrows, const int* __restrict__ pin_ptr, const int* __restrict__ pin_src, const int* __restrict__ pin_eid,
                                                 const int* __restrict__ pout_ptr, const int* __restrict__ pout_dst,
                                                 const int* __restrict__ pout_eid, int64_t N, const uint8_t* __restrict__ mask,
                                                 const int* __restrict__ pos, int* __restrict__ in_ptr, int* __restrict__ in_src,
                                                 int* __restrict__ in_eid, int* __restrict__ out_ptr, int* __restrict__ out_dst,
                                                 int* __restrict__ out_eid, int* __restrict__ loop_eid, const int* __restrict__ cnt_in,
                                                 const int* __restrict__ cnt_out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (r >= nrows) return;
    const bool out = r >= N;
    const int64_t row = out ? r - N : r;
    const int* pptr = out ? pout_ptr : pin_ptr;
    const int* pcol = out ? pout_dst : pin_src;
    const int* peid = out ? pout_eid : pin_eid;
    int* ccol = out ? out_dst : in_src;
    int* ceid = out ? out_eid : in_eid;
    int w;                                            // write cursor of the child row
    if constexpr (SCAN) {
        const int* cnt = out ? cnt_out : cnt_in;
        int acc = 0;
        for (int64_t i = lane; i < row; i += 64) acc += cnt[i];
        w = wave_sum_int_all(acc);
        if (lane == 0) {
            int* cptr = out ? out_ptr : in_ptr;
            cptr[row] = w;
            if (row == N - 1) cptr[N] = w + cnt[row];
        }
    } else {
        w = (out ? out_ptr : in_ptr)[row];
    }
    int loop = -1;
    const int b = pptr[row], e = pptr[row + 1];
    // the next 64 entries' (edge id, column) are loaded while this step's mask / position lookups are in flight, and the id / column / mask
    // loads are unconditional (clamped): as `if (k < e) { pe = ..; sel = mask[pe]; if (sel) { col = ..; ne = pos[pe]; } }` a step was three
    // dependent memory round trips
    int pe_c = 0, col_c = 0;
    if (e > b) { const int kc = min(b + lane, e - 1); pe_c = peid[kc]; col_c = pcol[kc]; }
    for (int k0 = b; k0 < e; k0 += 64) {
        const int k = k0 + lane;
        const int kn = min(k + 64, e - 1);
        const int pe_n = peid[kn], col_n = pcol[kn];
        const bool m_c = mask_at<BITS>(mask, pe_c);
        const bool sel = k < e && m_c;
        const int ne = sel ? pos[pe_c] : 0;             // selected entries only: on a whole graph `pos` is hundreds of MB of random 4-byte reads
        const int col = col_c;
        pe_c = pe_n; col_c = col_n;
        const unsigned long long bal = __ballot(sel);
        if (sel) {
            const int o = w + __popcll(bal & ((1ull << lane) - 1ull));
            ccol[o] = col;
            ceid[o] = ne;
        }
        if (!out) {                                     // PyG: the last existing self loop of a node carries its loop weight
            const unsigned long long lb = __ballot(sel && col == static_cast<int>(row));
            if (lb) loop = __shfl(ne, 63 - __clzll(lb), 64);
        }
        w += __popcll(bal);
    }
    if (!out && lane == 0) loop_eid[row] = loop;
}
template <bool BITS, bool SCAN = false>
__global__ void __launch_bounds__(kT) filter_fill(const int* __restrict__ pin_ptr, const int* __restrict__ pin_src, const int* __restrict__ pin_eid,
                                                 const int* __restrict__ pout_ptr, const int* __restrict__ pout_dst,
                                                 const int* __restrict__ pout_eid, int64_t N, const uint8_t* __restrict__ mask,
                                                 const int* __restrict__ pos, int* __restrict__ in_ptr, int* __restrict__ in_src,
                                                 int* __restrict__ in_eid, int* __restrict__ out_ptr, int* __restrict__ out_dst,
                                                 int* __restrict__ out_eid, int* __restrict__ loop_eid, const int* __restrict__ cnt_in = nullptr,
                                                 const int* __restrict__ cnt_out = nullptr) {
    filter_fill_body<BITS, SCAN>(2 * N, pin_ptr, pin_src, pin_eid, pout_ptr, pout_dst, pout_eid, N, mask, pos, in_ptr, in_src, in_eid, out_ptr,
                                 out_dst, out_eid, loop_eid, cnt_in, cnt_out);
}

// ---------------------------------------------------------------- gcn_norm forward
// One wave per node: deg_i = loopw_i + sum_{k in in-row i, src != i} w[eid_k]; dis = deg^-1/2.
__device__ __forceinline__ void norm_deg_body(const float* __restrict__ w, int64_t N, const int* __restrict__ in_ptr,
                                              const int* __restrict__ in_src, const int* __restrict__ in_eid,
                                              const int* __restrict__ loop_eid, float* __restrict__ dis,
                                              float* __restrict__ loopw) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    const int b = in_ptr[i], e = in_ptr[i + 1];
    float acc = 0.f;
    for (int k = b + lane; k < e; k += 64) {
        if (in_src[k] != static_cast<int>(i)) acc += w ? w[in_eid[k]] : 1.0f;
    }
    acc = wave_sum_all(acc);
    const int le = loop_eid[i];
    const float lw = (le >= 0 && w) ? w[le] : 1.0f;
    const float deg = lw + acc;
    float di = 1.0f / sqrtf(deg);           // deg.pow(-0.5)
    if (isinf(di)) di = 0.f;                // masked_fill(inf -> 0)
    if (lane == 0) { dis[i] = di; loopw[i] = lw; }
}
__global__ void __launch_bounds__(kT) norm_deg(const float* __restrict__ w, int64_t N, const int* __restrict__ in_ptr,
                                              const int* __restrict__ in_src, const int* __restrict__ in_eid,
                                              const int* __restrict__ loop_eid, float* __restrict__ dis,
                                              float* __restrict__ loopw) {
    norm_deg_body(w, N, in_ptr, in_src, in_eid, loop_eid, dis, loopw);
}

// Edge-sharded graphs: each rank sums the weights of ITS in-edges (degpart), the ranks all-reduce, and
// the normalisation continues from the global degree (the added self loop counts once: + 1).
__global__ void __launch_bounds__(kT) deg_partial(const float* __restrict__ w, int64_t N, const int* __restrict__ in_ptr,
                                                 const int* __restrict__ in_src, const int* __restrict__ in_eid,
                                                 float* __restrict__ degpart) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    float acc = 0.f;
    for (int k = in_ptr[i] + lane; k < in_ptr[i + 1]; k += 64)
        if (in_src[k] != static_cast<int>(i)) acc += w ? w[in_eid[k]] : 1.0f;
    acc = wave_sum_all(acc);
    if (lane == 0) degpart[i] = acc;
}
__global__ void __launch_bounds__(kT) dis_from_degree(const float* __restrict__ degsum, int64_t N, float* __restrict__ dis,
                                                     float* __restrict__ loopw) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (i >= N) return;
    float di = 1.0f / sqrtf(1.0f + degsum[i]);
    if (isinf(di)) di = 0.f;
    dis[i] = di;
    loopw[i] = 1.0f;
}
// Y = act(X + bias) with the same fused ReLU / counter-based dropout as the SpMM epilogue.
__global__ void __launch_bounds__(kT) bias_act(const float* __restrict__ X, const float* __restrict__ bias, int64_t N, int64_t D, int act,
                                              float drop_scale, uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                              const uint64_t* __restrict__ epoch, float* __restrict__ Y, int64_t row_offset) {
    seed = fold_epoch(seed, epoch);
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (idx >= N * D) return;
    const int64_t i = idx / D;
    const uint32_t c = static_cast<uint32_t>(idx - i * D);
    float y = X[idx];
    if (bias) y += bias[c];
    if (act != SGS_ACT_NONE) y = fmaxf(y, 0.f);
    if (act == SGS_ACT_RELU_DROPOUT) y = dropout_keep_at(seed, site, static_cast<uint64_t>(row_offset + i), c, drop_thresh) ? y * drop_scale : 0.f;
    Y[idx] = y;
}

// GraphSAGE mean aggregation (PyG SAGEConv aggr='mean': mean over in-edges, duplicates and (i,i) edges
// counted, no loops added): entry weight 1 / indeg(dst) in both CSR orders.
__global__ void __launch_bounds__(kT) mean_weights(int64_t N, const int* __restrict__ in_ptr, const int* __restrict__ out_ptr,
                                                  const int* __restrict__ out_dst, float* __restrict__ what_in,
                                                  float* __restrict__ what_out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (r >= 2 * N) return;
    if (r < N) {
        const int b = in_ptr[r], e = in_ptr[r + 1];
        const float w = e > b ? 1.0f / static_cast<float>(e - b) : 0.f;
        for (int k = b + lane; k < e; k += 64) what_in[k] = w;
    } else {
        const int64_t i = r - N;
        for (int k = out_ptr[i] + lane; k < out_ptr[i + 1]; k += 64) {
            const int t = out_dst[k];
            what_out[k] = 1.0f / static_cast<float>(in_ptr[t + 1] - in_ptr[t]);
        }
    }
}

// datasets.py:141-156 `add_degree` (before its softmax): logit_e = E^-1/2 / (colcount[row_e] + rowcount[col_e] + 1e-10),
// colcount = in-degree, rowcount = out-degree, read off the two CSR pointer arrays.
__global__ void __launch_bounds__(kT) degree_prior_logits(const int64_t* __restrict__ ei, int64_t E, const int* __restrict__ in_ptr,
                                                         const int* __restrict__ out_ptr, float scale, float* __restrict__ logit) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (e >= E) return;
    const int r = static_cast<int>(ei[e]), c = static_cast<int>(ei[E + e]);
    const float colcount_r = static_cast<float>(in_ptr[r + 1] - in_ptr[r]);
    const float rowcount_c = static_cast<float>(out_ptr[c + 1] - out_ptr[c]);
    const float prob = 1.0f / ((colcount_r + rowcount_c) + 1e-10f);
    logit[e] = prob * scale;
}

// Normalised weights in both CSR orders (0 for loop entries, which the loop term replaces).
__device__ __forceinline__ void norm_weights_body(int64_t nrows, const float* __restrict__ w, int64_t N, int64_t n_edges,
                                                  const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                  const int* __restrict__ in_eid, const int* __restrict__ out_ptr,
                                                  const int* __restrict__ out_dst, const int* __restrict__ out_eid,
                                                  const float* __restrict__ dis, const float* __restrict__ loopw,
                                                  float* __restrict__ what_in, float* __restrict__ what_out,
                                                  float* __restrict__ what_loop) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (r >= nrows) return;
    const bool out = r >= N;
    const int i = static_cast<int>(out ? r - N : r);
    const float di = dis[i];
    if (!out) {
        const int b = in_ptr[i], e = in_ptr[i + 1];
        for (int k = b + lane; k < e; k += 64) {
            const int s = in_src[k];
            const float we = w ? w[in_eid[k]] : 1.0f;
            what_in[k] = (s == i) ? 0.f : (dis[s] * we) * di;     // dis[row] * w * dis[col]
        }
        if (lane == 0) what_loop[i] = (di * loopw[i]) * di;
    } else {
        const int b = out_ptr[i], e = out_ptr[i + 1];
        for (int k = b + lane; k < e; k += 64) {
            const int t = out_dst[k];
            const float we = w ? w[out_eid[k]] : 1.0f;
            what_out[k] = (t == i) ? 0.f : (di * we) * dis[t];
        }
    }
}
__global__ void __launch_bounds__(kT) norm_weights(const float* __restrict__ w, int64_t N, int64_t n_edges,
                                                  const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                  const int* __restrict__ in_eid, const int* __restrict__ out_ptr,
                                                  const int* __restrict__ out_dst, const int* __restrict__ out_eid,
                                                  const float* __restrict__ dis, const float* __restrict__ loopw,
                                                  float* __restrict__ what_in, float* __restrict__ what_out,
                                                  float* __restrict__ what_loop) {
    norm_weights_body(2 * N, w, N, n_edges, in_ptr, in_src, in_eid, out_ptr, out_dst, out_eid, dis, loopw, what_in, what_out, what_loop);
}

// ---------------------------------------------------------------- gcn_norm backward
__global__ void __launch_bounds__(kT) norm_bwd_node(const float* __restrict__ w, const float* __restrict__ gw,
                                                   const float* __restrict__ gloop, int64_t N, const int* __restrict__ in_ptr,
                                                   const int* __restrict__ in_src, const int* __restrict__ in_eid,
                                                   const int* __restrict__ out_ptr, const int* __restrict__ out_dst,
                                                   const int* __restrict__ out_eid, const float* __restrict__ dis,
                                                   const float* __restrict__ loopw, float* __restrict__ Hn,
                                                   const float* __restrict__ gw2 = nullptr, const float* __restrict__ gloop2 = nullptr) {
    // gw2 / gloop2 (optional): a second layer's gradient wrt the same normalised weights, summed on read (both GCN layers of a model
    // share one normalisation: autograd's add kernel between the two SDDMMs and this pass is not needed)
    const int lane = threadIdx.x & 63;
    const int64_t t = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (t >= N) return;
    float acc = 0.f;
    // (unconditional clamped loads, the condition applied to the finished product: index pair, then the three gathers, per step)
    auto side = [&](const int* __restrict__ ptr, const int* __restrict__ col, const int* __restrict__ eid) {
        const int b = ptr[t], e_ = ptr[t + 1];
        for (int k0 = b; k0 < e_; k0 += 64) {
            const int k = k0 + lane, kc = min(k, e_ - 1);
            const int s = col[kc], e = eid[kc];
            const float ge = gw2 ? gw[e] + gw2[e] : gw[e];
            const float v = ge * w[e] * dis[s];
            if (k < e_ && s != static_cast<int>(t)) acc += v;
        }
    };
    side(in_ptr, in_src, in_eid);
    side(out_ptr, out_dst, out_eid);
    acc = wave_sum_all(acc);
    if (lane == 0) {
        const float a = dis[t];
        const float gl = gloop2 ? gloop[t] + gloop2[t] : gloop[t];
        const float G = acc + 2.0f * gl * loopw[t] * a;
        Hn[t] = -0.5f * a * a * a * G;
    }
}

__global__ void __launch_bounds__(kT) norm_bwd_edge(const float* __restrict__ gw, const float* __restrict__ gloop,
                                                   const int64_t* __restrict__ ei, int64_t n_edges,
                                                   const int* __restrict__ loop_eid, const float* __restrict__ dis,
                                                   const float* __restrict__ Hn, float* __restrict__ dw,
                                                   const float* __restrict__ gw2 = nullptr, const float* __restrict__ gloop2 = nullptr,
                                                   const float* __restrict__ dw_add = nullptr) {
    // dw_add (optional, may alias dw): another consumer's gradient wrt the same edge weights, added on the way out
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (e >= n_edges) return;
    const int s = static_cast<int>(ei[e]), t = static_cast<int>(ei[n_edges + e]);
    float g;
    if (s != t) g = (gw2 ? gw[e] + gw2[e] : gw[e]) * dis[s] * dis[t] + Hn[t];
    else g = (gloop2 ? gloop[s] + gloop2[s] : gloop[s]) * dis[s] * dis[s] + Hn[s];   // every existing (i,i) edge: PyG's index_put backward hands
                                                                                     // the loop gradient to overwritten duplicates too
    dw[e] = dw_add ? g + dw_add[e] : g;
}

// ---------------------------------------------------------------- CSR SpMM:  Y[i,:] = act( sum_k val[k] X[col[k],:] + diag[i] X[i,:] + bias )
// A group of LPR lanes owns one output row and walks its CSR row; each lane holds VEC
// consecutive columns per column chunk.  Gathered X rows come from L2/Infinity Cache at
// partition scale; the per-row (col, val) stream is a wave-uniform broadcast read.
template <int VEC> struct VecT;
template <> struct VecT<1> { using type = float; };
template <> struct VecT<4> { using type = float4; };

__device__ __forceinline__ void fma_vec(float& a, float w, float x) { a = fmaf(w, x, a); }
__device__ __forceinline__ void fma_vec(float4& a, float w, const float4& x) {
    a.x = fmaf(w, x.x, a.x); a.y = fmaf(w, x.y, a.y); a.z = fmaf(w, x.z, a.z); a.w = fmaf(w, x.w, a.w);
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ---------------------------------------------------------------------------------------------
// Mates: mate[e] = id of the reverse edge (dst_e -> src_e) of edge e, or -1 -- the pairing behind the paired scorer forward
// (edge_score.hip MODE 3).  rev[e]: binary search for src_e in the out-row of dst_e (rows of a coalesced, row-sorted edge list are
// ascending in dst; on any other list the search may simply miss and the edge stays unmated, which only costs speed); a mate
// is kept only when the relation is mutual, so duplicates pair off one to one and self loops stay alone.
__global__ void __launch_bounds__(kT) edge_reverse(const int64_t* __restrict__ ei, int64_t n, const int* __restrict__ out_ptr,
                                                  const int* __restrict__ out_dst, const int* __restrict__ out_eid, int* __restrict__ rev) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (e >= n) return;
    const int s = static_cast<int>(ei[e]), d = static_cast<int>(ei[n + e]);
    int lo = out_ptr[d], hi = out_ptr[d + 1];
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (out_dst[mid] < s) lo = mid + 1; else hi = mid;
    }
    rev[e] = (lo < end && out_dst[lo] == s) ? out_eid[lo] : -1;
}
__global__ void __launch_bounds__(kT) edge_mate(const int* __restrict__ rev, int64_t n, int* __restrict__ mate) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (e >= n) return;
    const int m = rev[e];
    mate[e] = (m >= 0 && m != e && rev[m] == static_cast<int>(e)) ? m : -1;
}

template <int VEC, int LPR>
__device__ __forceinline__ void spmm_csr_body(const float* __restrict__ X, int64_t N, int64_t D, const int* __restrict__ ptr,
                                              const int* __restrict__ col, const float* __restrict__ val,
                                              const float* __restrict__ diag, const float* __restrict__ bias, int act,
                                              float drop_scale, uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                              const uint64_t* __restrict__ epoch, float* __restrict__ Y) {
    using V = typename VecT<VEC>::type;
    constexpr int RPB = kT / LPR;   // rows per block
    seed = fold_epoch(seed, epoch);
    const int sub = threadIdx.x % LPR;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / LPR;
    if (i >= N) return;
    const int b = ptr[i], e = ptr[i + 1];
    const float dg = diag ? diag[i] : 0.f;
    for (int64_t c0 = static_cast<int64_t>(sub) * VEC; c0 < D; c0 += static_cast<int64_t>(LPR) * VEC) {
        V acc;
        if (VEC == 4) *reinterpret_cast<float4*>(&acc) = zero4(); else *reinterpret_cast<float*>(&acc) = 0.f;
        int k = b;
        for (; k + 4 <= e; k += 4) {          // 4 independent row gathers in flight
            const int j0 = col[k], j1 = col[k + 1], j2 = col[k + 2], j3 = col[k + 3];
            const float w0 = val[k], w1 = val[k + 1], w2 = val[k + 2], w3 = val[k + 3];
            const V x0 = *reinterpret_cast<const V*>(X + static_cast<int64_t>(j0) * D + c0);
            const V x1 = *reinterpret_cast<const V*>(X + static_cast<int64_t>(j1) * D + c0);
            const V x2 = *reinterpret_cast<const V*>(X + static_cast<int64_t>(j2) * D + c0);
            const V x3 = *reinterpret_cast<const V*>(X + static_cast<int64_t>(j3) * D + c0);
            fma_vec(acc, w0, x0); fma_vec(acc, w1, x1); fma_vec(acc, w2, x2); fma_vec(acc, w3, x3);
        }
        for (; k < e; ++k) {
            const V x0 = *reinterpret_cast<const V*>(X + static_cast<int64_t>(col[k]) * D + c0);
            fma_vec(acc, val[k], x0);
        }
        if (diag) {
            const V xi = *reinterpret_cast<const V*>(X + i * D + c0);
            fma_vec(acc, dg, xi);
        }
        float o[VEC];
        *reinterpret_cast<V*>(o) = acc;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float y = o[v];
            if (bias) y += bias[c0 + v];
            if (act != SGS_ACT_NONE) y = fmaxf(y, 0.f);
            if (act == SGS_ACT_RELU_DROPOUT)
                y = dropout_keep_at(seed, site, static_cast<uint64_t>(i), static_cast<uint32_t>(c0 + v), drop_thresh)
                        ? y * drop_scale : 0.f;
            o[v] = y;
        }
        *reinterpret_cast<V*>(Y + i * D + c0) = *reinterpret_cast<V*>(o);
    }
}
template <int VEC, int LPR>
__global__ void __launch_bounds__(kT) spmm_csr(const float* __restrict__ X, int64_t N, int64_t D, const int* __restrict__ ptr,
                                              const int* __restrict__ col, const float* __restrict__ val,
                                              const float* __restrict__ diag, const float* __restrict__ bias, int act,
                                              float drop_scale, uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                              const uint64_t* __restrict__ epoch, float* __restrict__ Y) {
    spmm_csr_body<VEC, LPR>(X, N, D, ptr, col, val, diag, bias, act, drop_scale, drop_thresh, seed, site, epoch, Y);
}

// Small-N variant (METIS partitions: ~1k rows of ~100-1000 nnz): one wave per row leaves the chip
// mostly empty and hub rows serialise, so a 4-wave workgroup owns a row, each wave gathers a strided
// quarter of its nnz (8 rows in flight per wave) and the four partial sums are combined through LDS
// in a fixed order (deterministic).
// Long rows (sgs_spmm_long_rows_set, on by default): a row of kSpmmLongRow entries or more takes spmm_long_row_gather instead of the
// loop in the bodies below.  The four (or sixteen) waves that own a hub row of ~1000 entries finish long after every other row of a
// partition-sized launch, and what they are short of is instruction issue: that loop spends ~18 instructions per entry and wave (two
// per-lane loads of a wave-uniform (col, val) pair, a 64-bit multiply and add per row address), and its time per entry does not
// depend on the row width between 256 B and 1 KiB ("Long rows").  Here a wave loads its share of the row's
// (col, val) 64 entries at a time, one per lane (the next 64 already in flight), turns the column into a 32-bit byte offset once per
// lane, and walks the 64 entries in unrolled batches of GU: per entry one v_readlane (the row offset, a scalar), one add, one load
// off the scalar base X, one v_readlane (the weight) and the fmas; two batches are in flight (PIPE) where registers allow.
// Only loads move: wave w still sums entries b + w, b + w + NW, ... in that order as one fma chain per column, so the partials, and
// with them Y, are bitwise the short loop's.
// Lanes past the row's last column (c0 >= D) gather column 0 and their sums are never read: control flow stays wave-uniform.
constexpr int kSpmmLongRow = 256;
template <int VEC, int NW, int GU, bool PIPE>
__device__ __forceinline__ void spmm_long_row_gather(const float* __restrict__ X, int64_t D, const int* __restrict__ col,
                                                     const float* __restrict__ val, int b, int e, int wave, int lane, int64_t cl,
                                                     float (&acc)[VEC]) {
    using V = typename VecT<VEC>::type;
    const int k0 = __builtin_amdgcn_readfirstlane(b) + __builtin_amdgcn_readfirstlane(wave);
    const int cnt = (__builtin_amdgcn_readfirstlane(e) - k0 + NW - 1) / NW;      // this wave's entries: k0 + NW m, m < cnt
    const uint32_t cb = static_cast<uint32_t>(cl) * 4u;     // byte offset of this lane's columns in a row
    const uint32_t rowb = static_cast<uint32_t>(D) * 4u;    // (the launchers take this path only while N * D * 4 fits 32 bits)
    const char* __restrict__ Xb = reinterpret_cast<const char*>(X);
    constexpr int NG = 64 / GU;
    int jn = 0;
    float wn = 0.f;
    if (lane < cnt) { jn = col[k0 + NW * lane]; wn = val[k0 + NW * lane]; }
    for (int m0 = 0; m0 < cnt; m0 += 64) {
        const uint32_t ol = static_cast<uint32_t>(jn) * rowb;       // this lane's entry: byte offset of its X row
        const float wl = wn;
        const int mn = m0 + 64 + lane;
        if (mn < cnt) { jn = col[k0 + NW * mn]; wn = val[k0 + NW * mn]; }
        const int nb = cnt - m0 < 64 ? cnt - m0 : 64;
        const int ng = nb / GU;
        // entry m of the chunk: a scalar row offset (v_readlane) + the lane's column offset beside the scalar base X; m is a
        // constant in the unrolled batches below
        const auto ld = [&](int m) {
            const uint32_t off = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(ol), m)) + cb;
            return *reinterpret_cast<const V*>(Xb + off);
        };
        const auto fm = [&](const V& x, int m) {
            const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wl), m));
            float xv[VEC];
            *reinterpret_cast<V*>(xv) = x;
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, xv[v], acc[v]);
        };
        V x[PIPE ? 2 : 1][GU];
        if (PIPE && ng > 0) {
#pragma unroll
            for (int u = 0; u < GU; ++u) x[0][u] = ld(u);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g < ng) {
                constexpr int one = PIPE ? 1 : 0;
                if (PIPE) {
                    if (g + 1 < ng) {
#pragma unroll
                        for (int u = 0; u < GU; ++u) x[(g + 1) & one][u] = ld((g + 1) * GU + u);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < GU; ++u) x[0][u] = ld(g * GU + u);
                }
#pragma unroll
                for (int u = 0; u < GU; ++u) fm(x[g & one][u], g * GU + u);
            }
        }
        const int t0 = ng * GU, rem = nb - t0;      // < GU left: one batch, as far as it goes
#pragma unroll
        for (int u = 0; u < GU - 1; ++u) if (u < rem) x[0][u] = ld(t0 + u);
#pragma unroll
        for (int u = 0; u < GU - 1; ++u) if (u < rem) fm(x[0][u], t0 + u);
    }
}

// The row gather of every waves-per-row kernel: wave `wave` of the NW that own row [b, e) sums entries b + wave, b + wave + NW, ... in
// that order, one fma chain per column, into acc (zero on entry) -- the row's partial for the lane's VEC columns from c0 (in: c0 < D).
// GU: gathers in flight in the main loop (the entries are taken in the same order whatever GU is).
// LONG: rows of kSpmmLongRow entries or more take spmm_long_row_gather<VEC, NW, LGU, LPIPE>: batches of LGU rows, two of them in flight
// (LPIPE) or one, as the kernel's register budget allows (the batch size does not enter the sums).  b, e are wave-uniform.
template <int VEC, int NW, bool LONG, int GU, int LGU, bool LPIPE>
__device__ __forceinline__ void spmm_row_gather(const float* __restrict__ X, int64_t D, const int* __restrict__ col,
                                                const float* __restrict__ val, int b, int e, int wave, int lane, int64_t c0, bool in,
                                                float (&acc)[VEC]) {
    using V = typename VecT<VEC>::type;
    if (LONG && e - b >= kSpmmLongRow) {
        spmm_long_row_gather<VEC, NW, LGU, LPIPE>(X, D, col, val, b, e, wave, lane, in ? c0 : 0, acc);
    } else if (in) {
        int k = b + wave;
        for (; k + (GU - 1) * NW < e; k += GU * NW) {    // GU independent gathers (k, k+NW, ..., k+(GU-1)NW)
            int j[GU]; float w[GU]; V x[GU];
#pragma unroll
            for (int u = 0; u < GU; ++u) { j[u] = col[k + NW * u]; w[u] = val[k + NW * u]; }
#pragma unroll
            for (int u = 0; u < GU; ++u) x[u] = *reinterpret_cast<const V*>(X + static_cast<int64_t>(j[u]) * D + c0);
#pragma unroll
            for (int u = 0; u < GU; ++u) {
                float xv[VEC];
                *reinterpret_cast<V*>(xv) = x[u];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], xv[v], acc[v]);
            }
        }
        for (; k < e; k += NW) {
            float xv[VEC];
            *reinterpret_cast<V*>(xv) = *reinterpret_cast<const V*>(X + static_cast<int64_t>(col[k]) * D + c0);
            const float w = val[k];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, xv[v], acc[v]);
        }
    }
}
// Column c of row i, finished by thread t of the row's waves: the NW wave partials in a fixed order (deterministic), then the diagonal
// term, bias, ReLU and the dropout hash.  Returns Y[i, c].
template <int VEC, int NW>
__device__ __forceinline__ float spmm_row_finish(const float (*part)[64 * VEC], int t, const float* __restrict__ X, int64_t D, int64_t i,
                                                 int64_t c, const float* __restrict__ diag, float dg, const float* __restrict__ bias,
                                                 int act, float drop_scale, uint32_t drop_thresh, uint32_t rkey) {
    float y = 0.f;
#pragma unroll
    for (int g = 0; g < NW; g += 4) y += (part[g][t] + part[g + 1][t]) + (part[g + 2][t] + part[g + 3][t]);
    if (diag) y = fmaf(dg, X[i * D + c], y);
    if (bias) y += bias[c];
    if (act != SGS_ACT_NONE) y = fmaxf(y, 0.f);
    if (act == SGS_ACT_RELU_DROPOUT) y = dropout_keep_col(rkey, static_cast<uint32_t>(c), drop_thresh) ? y * drop_scale : 0.f;
    return y;
}

// NW waves per row: 4, or 16 when rows are long (power-law partitions: the hub rows set the kernel's duration)
template <int VEC, int NW, bool LONG>
__device__ __forceinline__ void spmm_csr_rowblock_body(const float* __restrict__ X, int64_t N, int64_t D, const int* __restrict__ ptr,
                                                       const int* __restrict__ col, const float* __restrict__ val,
                                                       const float* __restrict__ diag, const float* __restrict__ bias, int act,
                                                       float drop_scale, uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                                       const uint64_t* __restrict__ epoch, float* __restrict__ Y) {
    __shared__ float part[NW][64 * VEC];
    seed = fold_epoch(seed, epoch);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const int b = ptr[i], e = ptr[i + 1];
    const float dg = diag ? diag[i] : 0.f;
    const uint32_t rkey = dropout_row_key(seed, site, static_cast<uint64_t>(i));
    for (int64_t cbase = 0; cbase < D; cbase += 64 * VEC) {
        const int64_t c0 = cbase + static_cast<int64_t>(lane) * VEC;
        const bool in = c0 < D;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        spmm_row_gather<VEC, NW, LONG, 8, 8, true>(X, D, col, val, b, e, wave, lane, c0, in, acc);
#pragma unroll
        for (int v = 0; v < VEC; ++v) part[wave][lane * VEC + v] = acc[v];
        __syncthreads();
        // 64*VEC columns finished by the first 64*VEC threads
        const int t = threadIdx.x;
        if (t < 64 * VEC && cbase + t < D) {
            const int64_t c = cbase + t;
            Y[i * D + c] = spmm_row_finish<VEC, NW>(part, t, X, D, i, c, diag, dg, bias, act, drop_scale, drop_thresh, rkey);
        }
        __syncthreads();
    }
}
template <int VEC, int NW, bool LONG>
__global__ void __launch_bounds__(64 * NW) spmm_csr_rowblock(const float* __restrict__ X, int64_t N, int64_t D, const int* __restrict__ ptr,
                                                       const int* __restrict__ col, const float* __restrict__ val,
                                                       const float* __restrict__ diag, const float* __restrict__ bias, int act,
                                                       float drop_scale, uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                                       const uint64_t* __restrict__ epoch, float* __restrict__ Y) {
    spmm_csr_rowblock_body<VEC, NW, LONG>(X, N, D, ptr, col, val, diag, bias, act, drop_scale, drop_thresh, seed, site, epoch, Y);
}

// SDDMM over the CSR: g[eid[k]] = <A[i,:], B[col[k],:]> for k in row i ; gdiag[i] = <A[i,:], B[i,:]>.
template <int VEC, int LPR>
__global__ void __launch_bounds__(kT) sddmm_csr(const float* __restrict__ A, const float* __restrict__ B, int64_t N, int64_t D,
                                               const int* __restrict__ ptr, const int* __restrict__ col,
                                               const int* __restrict__ eid, float* __restrict__ g, float* __restrict__ gdiag) {
    using V = typename VecT<VEC>::type;
    constexpr int RPB = kT / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / LPR;
    const bool live = i < N;            // keep every lane in the shuffles
    const int b = live ? ptr[i] : 0, e = live ? ptr[i + 1] : 0;
    // rows of one LPR-group advance together; groups in a wave may have different trip counts,
    // so the loop bound is made wave-uniform (max over the wave) and dead lanes contribute 0.
    int trips = e - b + 1;             // +1: the diagonal term
    for (int o = 32; o > 0; o >>= 1) trips = max(trips, __shfl_xor(trips, o, 64));
    for (int t = 0; t < trips; ++t) {
        const int k = b + t;
        const bool is_edge = live && k < e;
        const bool is_diag = live && k == e;
        const int64_t j = is_edge ? col[k] : i;
        float acc = 0.f;
        if (is_edge || is_diag) {
            for (int64_t c0 = static_cast<int64_t>(sub) * VEC; c0 < D; c0 += static_cast<int64_t>(LPR) * VEC) {
                float a[VEC], x[VEC];
                *reinterpret_cast<V*>(a) = *reinterpret_cast<const V*>(A + i * D + c0);
                *reinterpret_cast<V*>(x) = *reinterpret_cast<const V*>(B + j * D + c0);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc = fmaf(a[v], x[v], acc);
            }
        }
#pragma unroll
        for (int o = LPR >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (sub == 0) {
            if (is_edge) g[eid[k]] = acc;
            else if (is_diag && gdiag) gdiag[i] = acc;
        }
    }
}

// Small-N variant of sddmm_csr: a 4-wave workgroup per row, waves stride the row's entries, two
// independent dot products in flight per wave.
template <int VEC, int NW>
__global__ void __launch_bounds__(64 * NW) sddmm_csr_rowblock(const float* __restrict__ A, const float* __restrict__ B, int64_t N, int64_t D,
                                                        const int* __restrict__ ptr, const int* __restrict__ col,
                                                        const int* __restrict__ eid, float* __restrict__ g, float* __restrict__ gdiag) {
    using V = typename VecT<VEC>::type;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const int b = ptr[i], e = ptr[i + 1];
    const float* Ai = A + i * D;
    auto dot = [&](int64_t j) {
        float acc = 0.f;
        for (int64_t c0 = static_cast<int64_t>(lane) * VEC; c0 < D; c0 += 64 * VEC) {
            float a[VEC], x[VEC];
            *reinterpret_cast<V*>(a) = *reinterpret_cast<const V*>(Ai + c0);
            *reinterpret_cast<V*>(x) = *reinterpret_cast<const V*>(B + j * D + c0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc = fmaf(a[v], x[v], acc);
        }
        return acc;
    };
    if (D <= 64 * VEC) {
        // the usual case (a row fits one pass of the wave): row i's slice stays in registers, FOUR entries per step with their indices
        // loaded first and the four row gathers issued together (unconditional: entries past the row are clamped and not stored)
        const int64_t c0 = static_cast<int64_t>(lane) * VEC;
        const bool in = c0 < D;
        float a[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) a[v] = 0.f;
        if (in) *reinterpret_cast<V*>(a) = *reinterpret_cast<const V*>(Ai + c0);
        const int64_t cl = in ? c0 : 0;
        for (int k = b + wave; k < e; k += 4 * NW) {
            int jc[4], ev[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = k + NW * u;
                const int kc = kk < e ? kk : e - 1;
                jc[u] = col[kc];
                ev[u] = eid[kc];
            }
            float x[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<V*>(x[u]) = *reinterpret_cast<const V*>(B + static_cast<int64_t>(jc[u]) * D + cl);
            float d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float acc = 0.f;
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc = fmaf(a[v], in ? x[u][v] : 0.f, acc);
                d[u] = acc;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) d[u] = wave_sum_hi_dpp(d[u]);       // (DPP path; the total lands in lane 63)
            if (lane == 63) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + NW * u < e) g[ev[u]] = d[u];
            }
        }
        if (wave == 0 && gdiag) {
            const float d0 = wave_sum_all(dot(i));
            if (lane == 0) gdiag[i] = d0;
        }
        return;
    }
    int k = b + wave;
    for (; k + NW < e; k += 2 * NW) {
        float d0 = dot(col[k]), d1 = dot(col[k + NW]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { d0 += __shfl_xor(d0, o, 64); d1 += __shfl_xor(d1, o, 64); }
        if (lane == 0) { g[eid[k]] = d0; g[eid[k + NW]] = d1; }
    }
    for (; k < e; k += NW) {
        const float d0 = wave_sum_all(dot(col[k]));
        if (lane == 0) g[eid[k]] = d0;
    }
    if (wave == 0 && gdiag) {
        const float d0 = wave_sum_all(dot(i));
        if (lane == 0) gdiag[i] = d0;
    }
}

// dZ = dY * act'(Y):  ReLU -> [Y > 0];  ReLU+dropout -> [Y > 0] / (1 - p)  (Y > 0 iff kept and positive).
__global__ void __launch_bounds__(kT) act_bwd(const float* __restrict__ dY, const float* __restrict__ Y, int64_t n, int act,
                                             float drop_scale, float* __restrict__ dZ) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (i >= n) return;
    float g = dY[i];
    if (act != SGS_ACT_NONE) g = (Y[i] > 0.f) ? (act == SGS_ACT_RELU_DROPOUT ? g * drop_scale : g) : 0.f;
    dZ[i] = g;
}

// Column sums of a [N, D] matrix (bias / fc2 gradients), two fixed-order stages so the result is
// deterministic and the first stage fills the chip: block (cx, ry) sums kColRows rows of 64 columns.
constexpr int kColRows = 256;
// rows per first-stage workgroup: 256 for tall matrices, down to 32 for partition-sized ones so that the first stage
// still spreads over the chip (N = 1013: 32 row chunks x D/64 column groups instead of 4 x D/64)
inline int colsum_rows(int64_t N) { return N >= 16384 ? kColRows : (N >= 4096 ? 128 : 32); }
__global__ void __launch_bounds__(kT) colsum_partial(const float* __restrict__ A, int64_t N, int64_t D, int rows, float* __restrict__ part) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rgrp = threadIdx.x >> 6;
    const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows;
    const int64_t r1 = (r0 + rows < N) ? r0 + rows : N;
    float acc = 0.f;
    if (c < D)
        for (int64_t r = r0 + rgrp; r < r1; r += 4) acc += A[r * D + c];
    red[rgrp][threadIdx.x & 63] = acc;
    __syncthreads();
    if (rgrp == 0 && c < D)
        part[static_cast<int64_t>(blockIdx.y) * D + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
template <int RG>    // RG row groups of 64 columns per workgroup (RG * 64 threads): 4 for a handful of partials, 16 for tall inputs
__global__ void __launch_bounds__(RG * 64) colsum_final(const float* __restrict__ part, int64_t nchunk, int64_t D, float* __restrict__ out) {
    __shared__ float red[RG][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rgrp = threadIdx.x >> 6;
    float acc = 0.f;
    if (c < D)
        for (int64_t r = rgrp; r < nchunk; r += RG) acc += part[r * D + c];
    red[rgrp][threadIdx.x & 63] = acc;
    __syncthreads();
    if (rgrp == 0 && c < D) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < RG; g += 4) s += (red[g][threadIdx.x] + red[g + 1][threadIdx.x]) + (red[g + 2][threadIdx.x] + red[g + 3][threadIdx.x]);
        out[c] = s;
    }
}

// Partition-sized inputs (N <= kColSmallRows rows): the column sums in ONE launch -- a workgroup owns 16 columns, its 64 row lanes
// stride the rows and meet in LDS in a fixed tree (deterministic).  ACT: the activation backward rides along, dZ = dY * act'(Y) is
// written and summed in the same pass (a layer's backward then holds one launch where it held act_bwd + the two colsum stages).
constexpr int kColSmallRows = 2048;
template <bool ACT>
__device__ __forceinline__ void colsum_small_body(const float* __restrict__ A, const float* __restrict__ Y, int64_t N, int64_t D, int act,
                                                  float drop_scale, float* __restrict__ dZ, float* __restrict__ out, int64_t blk) {
    __shared__ float red[64][17];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int64_t c = blk * 16 + cl;
    float acc = 0.f;
    if (c < D) {
#pragma unroll 16
        for (int64_t r = rl; r < N; r += 64) {        // (N ~ 1 000: all 16 loads of a thread in flight at once)
            float g = A[r * D + c];
            if (ACT) {
                if (act != SGS_ACT_NONE) g = (Y[r * D + c] > 0.f) ? (act == SGS_ACT_RELU_DROPOUT ? g * drop_scale : g) : 0.f;
                dZ[r * D + c] = g;
            }
            acc += g;
        }
    }
    red[rl][cl] = acc;
    __syncthreads();
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        if (rl < h) red[rl][cl] += red[rl + h][cl];
        __syncthreads();
    }
    if (rl == 0 && c < D && out) out[c] = red[0][cl];
}
template <bool ACT>
__global__ void __launch_bounds__(1024) colsum_small(const float* __restrict__ A, const float* __restrict__ Y, int64_t N, int64_t D, int act,
                                                    float drop_scale, float* __restrict__ dZ, float* __restrict__ out) {
    colsum_small_body<ACT>(A, Y, N, D, act, drop_scale, dZ, out, blockIdx.x);
}

// D % 4 == 0: the same pass on 16-byte words -- a thread owns four columns and N/256 rows, so every load of a thread is in flight at
// once and the 16-column row segments stay whole 64-byte reads.
template <bool ACT>
__device__ __forceinline__ void colsum_small_v4_body(const float* __restrict__ A, const float* __restrict__ Y, int64_t N, int64_t D, int act,
                                                     float drop_scale, float* __restrict__ dZ, float* __restrict__ out, int64_t blk) {
    __shared__ float4 red[256][4];
    const int cg = threadIdx.x & 3, rl = threadIdx.x >> 2;
    const int64_t c = blk * 16 + 4 * cg;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < D) {
#pragma unroll 8
        for (int64_t r = rl; r < N; r += 256) {
            float4 g = *reinterpret_cast<const float4*>(A + r * D + c);
            if (ACT) {
                if (act != SGS_ACT_NONE) {
                    const float4 y = *reinterpret_cast<const float4*>(Y + r * D + c);
                    const float sc = act == SGS_ACT_RELU_DROPOUT ? drop_scale : 1.f;
                    g.x = y.x > 0.f ? g.x * sc : 0.f; g.y = y.y > 0.f ? g.y * sc : 0.f;
                    g.z = y.z > 0.f ? g.z * sc : 0.f; g.w = y.w > 0.f ? g.w * sc : 0.f;
                }
                *reinterpret_cast<float4*>(dZ + r * D + c) = g;
            }
            acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
        }
    }
    red[rl][cg] = acc;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
        if (rl < h) {
            const float4 o = red[rl + h][cg];
            float4 m = red[rl][cg];
            m.x += o.x; m.y += o.y; m.z += o.z; m.w += o.w;
            red[rl][cg] = m;
        }
        __syncthreads();
    }
    if (rl == 0 && c < D && out) *reinterpret_cast<float4*>(out + c) = red[0][cg];
}
template <bool ACT>
__global__ void __launch_bounds__(1024) colsum_small_v4(const float* __restrict__ A, const float* __restrict__ Y, int64_t N, int64_t D, int act,
                                                       float drop_scale, float* __restrict__ dZ, float* __restrict__ out) {
    colsum_small_v4_body<ACT>(A, Y, N, D, act, drop_scale, dZ, out, blockIdx.x);
}

// A vector's sum (D = 1, e.g. d fc2.bias = sum of dz over the q active edges) in one workgroup: the two-stage kernels above would spend
// a 64-column workgroup on every row chunk of a one-column matrix.
constexpr int64_t kVecSumMax = int64_t(1) << 20;
__global__ void __launch_bounds__(1024) vecsum_small(const float* __restrict__ A, int64_t N, float* __restrict__ out) {
    __shared__ float red[16];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int64_t i = threadIdx.x;
    for (; i + 3 * 1024 < N; i += 4 * 1024) { a0 += A[i]; a1 += A[i + 1024]; a2 += A[i + 2048]; a3 += A[i + 3072]; }
    for (; i < N; i += 1024) a0 += A[i];
    const float r = block_sum((a0 + a1) + (a2 + a3), red);
    if (threadIdx.x == 0) out[0] = r;
}


// ---------------------------------------------------------------- D drawn subgraphs of one partition (ensemble evaluation)
// blockIdx.y = draw.  The bodies above run unchanged on draw d's slices, so every array equals what sgs_graph_filter /
// sgs_gcn_norm_fwd / sgs_spmm_csr produce for that draw alone.  Forward only: in-rows (nrows = N), no out-CSR.
__global__ void __launch_bounds__(kT) multi_filter_count(const int* __restrict__ pin_ptr, const int* __restrict__ pin_eid, int64_t N, int64_t E,
                                                        const uint8_t* __restrict__ mask, const int64_t* __restrict__ sampled_eid, int64_t q,
                                                        int64_t n_row_blocks, int* __restrict__ cnt, int* __restrict__ pos) {
    const int64_t d = blockIdx.y;
    filter_count_scatter_body<false>(pin_ptr, pin_eid, nullptr, nullptr, N, mask + d * E, sampled_eid + d * q, q, n_row_blocks, cnt + d * (N + 1),
                                     nullptr, pos + d * E, N);
}
__global__ void __launch_bounds__(1024) multi_scan_counts(const int* __restrict__ cnt, int64_t N, int* __restrict__ in_ptr, int* __restrict__ cur) {
    const int64_t d = blockIdx.y;
    scan_counts_body(cnt + d * (N + 1), N, in_ptr + d * (N + 1), cur + d * (N + 1));
}
template <bool SCAN>
__global__ void __launch_bounds__(kT) multi_filter_fill(const int* __restrict__ pin_ptr, const int* __restrict__ pin_src, const int* __restrict__ pin_eid,
                                                       int64_t N, int64_t E, int64_t q, const uint8_t* __restrict__ mask, const int* __restrict__ pos,
                                                       int* __restrict__ in_ptr, int* __restrict__ in_src, int* __restrict__ in_eid,
                                                       int* __restrict__ loop_eid, const int* __restrict__ cnt) {
    const int64_t d = blockIdx.y;
    filter_fill_body<false, SCAN>(N, pin_ptr, pin_src, pin_eid, nullptr, nullptr, nullptr, N, mask + d * E, pos + d * E, in_ptr + d * (N + 1),
                                  in_src + d * q, in_eid + d * q, nullptr, nullptr, nullptr, loop_eid + d * N, cnt + d * (N + 1), nullptr);
}
__global__ void __launch_bounds__(kT) multi_norm_deg(const float* __restrict__ w, int64_t q, int64_t N, const int* __restrict__ in_ptr,
                                                    const int* __restrict__ in_src, const int* __restrict__ in_eid, const int* __restrict__ loop_eid,
                                                    float* __restrict__ dis, float* __restrict__ loopw) {
    const int64_t d = blockIdx.y;
    norm_deg_body(w ? w + d * q : nullptr, N, in_ptr + d * (N + 1), in_src + d * q, in_eid + d * q, loop_eid + d * N, dis + d * N, loopw + d * N);
}
__global__ void __launch_bounds__(kT) multi_norm_weights(const float* __restrict__ w, int64_t q, int64_t N, const int* __restrict__ in_ptr,
                                                        const int* __restrict__ in_src, const int* __restrict__ in_eid, const float* __restrict__ dis,
                                                        const float* __restrict__ loopw, float* __restrict__ what_in, float* __restrict__ what_loop) {
    const int64_t d = blockIdx.y;
    norm_weights_body(N, w ? w + d * q : nullptr, N, q, in_ptr + d * (N + 1), in_src + d * q, in_eid + d * q, nullptr, nullptr, nullptr, dis + d * N,
                      loopw + d * N, what_in + d * q, nullptr, what_loop + d * N);
}
template <int VEC, int LPR>
__global__ void __launch_bounds__(kT) multi_spmm_csr(const float* __restrict__ X, int64_t xs, int64_t N, int64_t D, int64_t nnz,
                                                    const int* __restrict__ ptr, const int* __restrict__ col, const float* __restrict__ val,
                                                    const float* __restrict__ diag, const float* __restrict__ bias, int act, float* __restrict__ Y) {
    const int64_t d = blockIdx.y;
    spmm_csr_body<VEC, LPR>(X + d * xs, N, D, ptr + d * (N + 1), col + d * nnz, val + d * nnz, diag ? diag + d * N : nullptr, bias, act, 1.0f, 0u,
                            uint64_t(0), 0u, nullptr, Y + d * N * D);
}
template <int VEC, int NW, bool LONG>
__global__ void __launch_bounds__(64 * NW) multi_spmm_csr_rowblock(const float* __restrict__ X, int64_t xs, int64_t N, int64_t D, int64_t nnz,
                                                                 const int* __restrict__ ptr, const int* __restrict__ col,
                                                                 const float* __restrict__ val, const float* __restrict__ diag,
                                                                 const float* __restrict__ bias, int act, float* __restrict__ Y) {
    const int64_t d = blockIdx.y;
    spmm_csr_rowblock_body<VEC, NW, LONG>(X + d * xs, N, D, ptr + d * (N + 1), col + d * nnz, val + d * nnz, diag ? diag + d * N : nullptr, bias, act,
                                    1.0f, 0u, uint64_t(0), 0u, nullptr, Y + d * N * D);
}

// GCN layer pairs (partition scale, the row-block path): the SpMM of one layer with the neighbouring layer's row-local work in its
// epilogue, so the dense product / activation backward / bias sums between two SpMMs lose their launches.  A workgroup is 16 waves:
// RG = 16 / NW rows side by side, each gathered by NW waves exactly as spmm_csr_rowblock_body does (same entry order, same fixed-order
// combination of the wave partials, same dropout hash), so Y is bitwise sgs_spmm_csr's.  The RG finished rows stay in LDS for:
//   kPairFwd:  Z[i, o] = sum_d Y[i, d] Wn[o, d]   (Wn [Dn, D], the next layer's weight): a thread per (row, o).
//   kPairBwd:  dZp[i, e] = act'(Yp[i, e]) * sum_c Y[i, c] Wn[c, e]   (Wn [D, Dn], Yp [N, Dn]: the previous layer's product and activation
//              backward, act' as colsum_small<true>): a thread per (row, e).
//   Both products are fp32 fma chains in lib_gemm_dot's order, the order in which the library GEMMs they replace (hipBLASLt's fp32
//   kernels for these shapes: v_mfma_f32_16x16x4_f32, which accumulates its four products in turn) sum: Z and dZp are bitwise the
//   GEMMs' results, so a training run with the pairs is bitwise the run without them.  (Checked by tests/test_gpu_gcn_fused.py.)
//   kPairCol:  neither.
// kPairBwd / kPairCol also sum the columns of X (the bias gradient of the layer whose dZ X is): the first ncs workgroups run
// colsum_small(_v4)<false>'s pass over X -- bitwise sgs_colsum at N <= kColSmallRows -- and the row groups follow.
enum { kPairCol = 0, kPairFwd = 1, kPairBwd = 2 };
constexpr int kPairMaxD = 512;      // widest Y row kept in LDS
constexpr int kPairWlds = 12288;    // kPairFwd: Wn (transposed) is staged in LDS when Dn * D fits (48 KiB; the GNN head's W2: 41 x 256)
constexpr int kPairWpre = kPairWlds / 1024;
// Position t of the library's summation over k = 0..K-1: 16-deep steps of two 8-element halves, each half its even k, then its odd k
// (two k per lane per LDS read feed two MFMAs); the K % 16 tail in plain order.
// lib_gemm_dot: sum_k y(k) w(k) as one fp32 fma chain in that order; the operands of the next 8-element half are loaded while the
// current half's fmas run (the chain itself is the latency: a thread per output, the order fixes it).
template <class FY, class FW>
__device__ __forceinline__ float lib_gemm_dot(int K, FY y, FW w) {
    const int Kmain = K / 16 * 16;
    float z = 0.f;
    if (Kmain > 0) {
        float ya[8], wa[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = 2 * (u & 3) + (u >> 2); ya[u] = y(k); wa[u] = w(k); }
        for (int b = 0; b < Kmain; b += 8) {
            const int nb = b + 8 < Kmain ? b + 8 : b;
            float yn[8], wn[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int k = nb + 2 * (u & 3) + (u >> 2); yn[u] = y(k); wn[u] = w(k); }
#pragma unroll
            for (int u = 0; u < 8; ++u) z = fmaf(ya[u], wa[u], z);
#pragma unroll
            for (int u = 0; u < 8; ++u) { ya[u] = yn[u]; wa[u] = wn[u]; }
        }
    }
    for (int k = Kmain; k < K; ++k) z = fmaf(y(k), w(k), z);
    return z;
}
// GU, LGU, LPIPE: spmm_row_gather's (the row-block body's values unless a kernel's register budget asks for less)
template <int VEC, int NW, int MODE, bool LONG, int GU = 8, int LGU = GU, bool LPIPE = true>
__device__ __forceinline__ void spmm_rowgroup_pair_body(const float* __restrict__ X, int64_t N, int64_t D, const int* __restrict__ ptr,
                                                        const int* __restrict__ col, const float* __restrict__ val,
                                                        const float* __restrict__ diag, const float* __restrict__ bias, int act,
                                                        float drop_scale, uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                                        const uint64_t* __restrict__ epoch, float* __restrict__ Y,
                                                        const float* __restrict__ Wn, int64_t Dn, const float* __restrict__ Yp,
                                                        float* __restrict__ Zn, int ncs, float* __restrict__ colsum) {
    constexpr int RG = 16 / NW;
    __shared__ float part[RG][NW][64 * VEC];
    __shared__ __align__(16) float ys[RG * kPairMaxD];
    __shared__ float wl[MODE == kPairFwd ? kPairWlds : 1];
    if (MODE != kPairFwd && static_cast<int>(blockIdx.x) < ncs) {
        if (D % 4 == 0) colsum_small_v4_body<false>(X, nullptr, N, D, SGS_ACT_NONE, 1.f, nullptr, colsum, blockIdx.x);
        else            colsum_small_body<false>(X, nullptr, N, D, SGS_ACT_NONE, 1.f, nullptr, colsum, blockIdx.x);
        return;
    }
    seed = fold_epoch(seed, epoch);
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) % NW, grp = threadIdx.x / (64 * NW);
    const int64_t row0 = static_cast<int64_t>(blockIdx.x - ncs) * RG;
    const int64_t i = row0 + grp;
    const bool live = i < N;
    int b = 0, e = 0;
    float dg = 0.f;
    uint32_t rkey = 0;
    const int yact = MODE == kPairBwd ? SGS_ACT_NONE : act;     // kPairBwd: act / drop_scale are the previous layer's
    if (live) {
        b = ptr[i];
        e = ptr[i + 1];
        dg = diag ? diag[i] : 0.f;
        rkey = dropout_row_key(seed, site, static_cast<uint64_t>(i));
    }
    // kPairFwd with Wn staged: its elements are loaded now (coalesced, kPairWpre per thread) and written to LDS after the gathers, so
    // their latency hides behind the rows'
    const bool wlds = MODE == kPairFwd && Dn * D <= kPairWlds;
    float wpre[MODE == kPairFwd ? kPairWpre : 1];
    if (MODE == kPairFwd && wlds) {
#pragma unroll
        for (int u = 0; u < kPairWpre; ++u) {
            const int64_t idx = threadIdx.x + 1024 * u;
            wpre[u] = idx < Dn * D ? Wn[idx] : 0.f;
        }
    }
    // ---- spmm_csr_rowblock_body, one row per group of NW waves
    for (int64_t cbase = 0; cbase < D; cbase += 64 * VEC) {
        const int64_t c0 = cbase + static_cast<int64_t>(lane) * VEC;
        const bool in = c0 < D;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        spmm_row_gather<VEC, NW, LONG, GU, LGU, LPIPE>(X, D, col, val, b, e, wave, lane, c0, in, acc);   // (a dead row: b = e = 0)
#pragma unroll
        for (int v = 0; v < VEC; ++v) part[grp][wave][lane * VEC + v] = acc[v];
        __syncthreads();
        const int t = threadIdx.x % (64 * NW);
        if (live && t < 64 * VEC && cbase + t < D) {
            const int64_t c = cbase + t;
            const float y = spmm_row_finish<VEC, NW>(part[grp], t, X, D, i, c, diag, dg, bias, yact, drop_scale, drop_thresh, rkey);
            Y[i * D + c] = y;
            ys[grp * D + c] = y;
        }
        __syncthreads();
    }
    if (MODE == kPairFwd) {
        if (wlds) {
#pragma unroll
            for (int u = 0; u < kPairWpre; ++u) {
                const int64_t idx = threadIdx.x + 1024 * u;
                if (idx < Dn * D) {
                    const int64_t o = idx / D, k = idx - o * D;
                    wl[k * Dn + o] = wpre[u];           // [k][o]: the lanes of a wave read consecutive o
                }
            }
            __syncthreads();
        }
        for (int64_t idx = threadIdx.x; idx < RG * Dn; idx += 1024) {
            const int r = static_cast<int>(idx / Dn);
            const int64_t o = idx - r * Dn, ir = row0 + r;
            if (ir >= N) break;
            const float* yr = ys + r * D;
            const auto yk = [&](int k) { return yr[k]; };
            Zn[ir * Dn + o] = wlds ? lib_gemm_dot(static_cast<int>(D), yk, [&](int k) { return wl[k * Dn + o]; })
                                   : lib_gemm_dot(static_cast<int>(D), yk, [&](int k) { return Wn[o * D + k]; });
        }
    } else if (MODE == kPairBwd) {
        for (int64_t idx = threadIdx.x; idx < RG * Dn; idx += 1024) {
            const int r = static_cast<int>(idx / Dn);
            const int64_t ep = idx - r * Dn, ir = row0 + r;
            if (ir >= N) break;
            const float* yr = ys + r * D;
            float a = lib_gemm_dot(static_cast<int>(D), [&](int c) { return yr[c]; }, [&](int c) { return Wn[c * Dn + ep]; });
            if (act != SGS_ACT_NONE) a = (Yp[ir * Dn + ep] > 0.f) ? (act == SGS_ACT_RELU_DROPOUT ? a * drop_scale : a) : 0.f;
            Zn[ir * Dn + ep] = a;
        }
    }
}
// (1024-thread workgroups: 128 VGPRs at most; the long-row path's two batches of 8 float4 rows fit: 96 to 112)
template <int VEC, int NW, int MODE, bool LONG>
__global__ void __launch_bounds__(1024) spmm_rowgroup_pair(const float* __restrict__ X, int64_t N, int64_t D, const int* __restrict__ ptr,
                                                           const int* __restrict__ col, const float* __restrict__ val,
                                                           const float* __restrict__ diag, const float* __restrict__ bias, int act,
                                                           float drop_scale, uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                                           const uint64_t* __restrict__ epoch, float* __restrict__ Y,
                                                           const float* __restrict__ Wn, int64_t Dn, const float* __restrict__ Yp,
                                                           float* __restrict__ Zn, int ncs, float* __restrict__ colsum) {
    spmm_rowgroup_pair_body<VEC, NW, MODE, LONG>(X, N, D, ptr, col, val, diag, bias, act, drop_scale, drop_thresh, seed, site, epoch, Y, Wn, Dn, Yp, Zn,
                                           ncs, colsum);
}

// Two jobs per launch (the GNN head's learned and random forward: the same layers and weights over two graphs of N rows): gridDim.y = 2,
// workgroup (x, y) runs the single-job body of workgroup x on job y's graph and outputs (workgroup-uniform look-up: scalar loads), so each
// job's results are bitwise the single launch's.  Neither job reads what the other writes.
struct SpmmDualJob {
    const float* X;
    const int* ptr;
    const int* col;
    const float* val;
    const float* diag;
    float* Y;
    float* Z;               // layer pair only: Y Wn^T
    int64_t nnz;
    uint64_t seed;
};
struct SpmmDualArgs {
    SpmmDualJob job[2];
};
template <int VEC, int NW, bool LONG>
__global__ void __launch_bounds__(64 * NW) spmm_csr_rowblock_dual(SpmmDualArgs a, int64_t N, int64_t D, const float* __restrict__ bias, int act,
                                                                  float drop_scale, uint32_t drop_thresh, uint32_t site,
                                                                  const uint64_t* __restrict__ epoch) {
    const SpmmDualJob& j = a.job[blockIdx.y];
    spmm_csr_rowblock_body<VEC, NW, LONG>(j.X, N, D, j.ptr, j.col, j.val, j.diag, bias, act, drop_scale, drop_thresh, j.seed, site, epoch, j.Y);
}
// The pair kernel's 16-wave workgroups are 4 waves on every SIMD: two of them share a CU (what lets the two jobs' gathers overlap) only
// within 512 / 8 = 64 VGPRs.  The single-job <4, 4> kernel has 78, and the bound alone spills; with 4 float4 gathers in flight instead
// of 8 the kernel fits without scratch (60 VGPRs).  LDS: 2 x 72 KiB of the CU's 160.  -DSGS_DUAL_PAIR_CAPPED=0 builds the uncapped
// form (the single-job kernel's registers and unroll: one workgroup per CU) for A/B timing.
#ifndef SGS_DUAL_PAIR_CAPPED
#define SGS_DUAL_PAIR_CAPPED 1
#endif
constexpr int kDualPairWaves = SGS_DUAL_PAIR_CAPPED ? 8 : 4;
constexpr int dual_pair_gu(int vec) { return SGS_DUAL_PAIR_CAPPED && vec == 4 ? 4 : 8; }
// the long-row path under the same cap: at VEC = 4 it does not fit (one batch of 4 in flight: 64 VGPRs and 8 bytes of scratch), so
// that kernel keeps the short loop whatever the switch says; at VEC = 1 two batches of 4 fit (two of 8 spill)
constexpr bool dual_pair_long(int vec) { return !(SGS_DUAL_PAIR_CAPPED && vec == 4); }
constexpr int dual_pair_long_gu(int vec) { return SGS_DUAL_PAIR_CAPPED ? 4 : 8; }
template <int VEC, int NW, bool LONG>
__global__ void __launch_bounds__(1024, kDualPairWaves) spmm_rowgroup_pair_dual(SpmmDualArgs a, int64_t N, int64_t D,
                                                                                const float* __restrict__ bias, int act, float drop_scale,
                                                                                uint32_t drop_thresh, uint32_t site,
                                                                                const uint64_t* __restrict__ epoch,
                                                                                const float* __restrict__ Wn, int64_t Dn) {
    const SpmmDualJob& j = a.job[blockIdx.y];
    spmm_rowgroup_pair_body<VEC, NW, kPairFwd, LONG && dual_pair_long(VEC), dual_pair_gu(VEC), dual_pair_long_gu(VEC)>(j.X, N, D, j.ptr, j.col, j.val, j.diag, bias, act, drop_scale,
                                                                                  drop_thresh, j.seed, site, epoch, j.Y, Wn, Dn, nullptr, j.Z, 0,
                                                                                  nullptr);
}

}  // namespace
}  // namespace sgs

using namespace sgs;

// sgs_spmm_long_rows_set: read by the SpMM launchers at launch time; it selects the kernel (a captured graph keeps what it launched).
// On, a graph of at most kSpmmLongMaxRows rows launches the <..., LONG = true> kernels.  Their two batches of rows in flight cost
// 20 - 34 VGPRs at VEC = 4 (DESIGN.md section 5 has the table), which only pays where hub rows set the launch's duration: a grid of about one
// resident round of workgroups (partitions, N ~ 1000).  A larger grid hides its hubs behind its other workgroups and is bound by
// how many waves a CU holds, so it keeps the short loop's kernels and their occupancy.
static int g_spmm_long_rows = 1;
constexpr int64_t kSpmmLongMaxRows = 4096;
static inline bool spmm_long_rows_on(int64_t N, int64_t D) {       // (D: the long path keeps byte offsets into X in 32 bits)
    return g_spmm_long_rows && N <= kSpmmLongMaxRows && D <= (int64_t(1) << 18);
}
// The one kernel choice of every GCN SpMM entry point (so a pair, a two-job launch and every draw of a multi launch equal sgs_spmm_csr)
static inline SpmmPlan gcn_spmm_plan(int64_t N, int64_t D, int64_t nnz, bool al16) {
    return spmm_plan(N, D, nnz, al16, spmm_long_rows_on(N, D));
}
// a pair kernel's grid: the column-sum workgroups, then 16 / NW rows per 16-wave workgroup
static inline dim3 pair_grid(const SpmmPlan& p, int64_t N, int ncs = 0, unsigned jobs = 1) {
    return dim3(static_cast<unsigned>(ncs + cdiv(N, 16 / p.w)), jobs);
}

// The activation / dropout arguments of entry point `who`, checked and normalised (p = 0: RELU_DROPOUT is plain RELU)
struct ActDrop { int act; float scale; uint32_t thresh; };
static int act_drop(const char* who, int act, float p_drop, ActDrop* o) {
    SGS_REQUIRE(act >= SGS_ACT_NONE && act <= SGS_ACT_RELU_DROPOUT && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL, "%s: bad activation / dropout", who);
    *o = ActDrop{(act == SGS_ACT_RELU_DROPOUT && p_drop == 0.f) ? SGS_ACT_RELU : act, 1.0f / (1.0f - p_drop), dropout_thresh(p_drop)};
    return SGS_OK;
}

extern "C" {

// large edge lists: two stable radix sorts instead of atomics + per-row sorts (csrc/graph_sort.hip)
constexpr int64_t kSortEdges = int64_t(1) << 22;

size_t sgs_graph_build_workspace_bytes(int64_t n_edges, int64_t N) {
    if (n_edges < 0) n_edges = 0;
    if (N < 0) N = 0;
    if (n_edges >= kSortEdges) return graph_sort_workspace_bytes(n_edges, N);
    return 4 * carve_bytes(N + 1, 4) + 2 * carve_bytes(n_edges + 1, 4) + 512;
}

int sgs_graph_build(const int64_t* edge_index, int64_t n_edges, int64_t N, int32_t* in_ptr, int32_t* in_src,
                    int32_t* in_eid, int32_t* out_ptr, int32_t* out_dst, int32_t* out_eid, int32_t* loop_eid, void* ws,
                    size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n_edges >= 0 && N >= 0 && n_edges < (int64_t(1) << 31) && N < (int64_t(1) << 31), SGS_EINVAL,
                "sgs_graph_build: sizes out of range (n_edges=%lld N=%lld)", (long long)n_edges, (long long)N);
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(in_ptr && out_ptr && loop_eid && (n_edges == 0 || (edge_index && in_src && in_eid && out_dst && out_eid)),
                SGS_EINVAL, "sgs_graph_build: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_graph_build_workspace_bytes(n_edges, N), SGS_EWORKSPACE,
                "sgs_graph_build: workspace too small");
    if (n_edges >= kSortEdges)
        return graph_build_by_sort(edge_index, n_edges, N, in_ptr, in_src, in_eid, out_ptr, out_dst, out_eid, loop_eid, ws, ws_bytes, stream);
    Carver cv(ws);
    int* cnt_in = cv.take<int>(N + 1);
    int* cnt_out = cv.take<int>(N + 1);
    int* cur_in = cv.take<int>(N + 1);
    int* cur_out = cv.take<int>(N + 1);
    int* tmp_in = cv.take<int>(n_edges + 1);
    int* tmp_out = cv.take<int>(n_edges + 1);
    // cnt_in + cnt_out are adjacent -> 0; loop_eid -> -1 (one kernel launch, not memset nodes: see zero_async)
    if (int rc = fill2_async(cnt_in, 2 * carve_bytes(N + 1, 4), 0u, loop_eid, static_cast<size_t>(N) * 4, 0xFFFFFFFFu, stream)) return rc;
    const bool small_n = N <= kLdsNodes;
    if (n_edges > 0) {
        if (small_n)
            hipLaunchKernelGGL(count_degrees_lds, dim3(cdiv(n_edges, kEdgesPerBlock)), dim3(kT), 0, stream, edge_index, n_edges,
                               static_cast<int>(N), cnt_in, cnt_out, loop_eid);
        else
            hipLaunchKernelGGL(count_degrees, dim3(cdiv(n_edges, kT)), dim3(kT), 0, stream, edge_index, n_edges, cnt_in, cnt_out,
                               loop_eid);
    }
    // (a "last workgroup scans" variant of the count kernel was tried and is slower on MI355X: the device-scope fences it
    //  needs write back / invalidate the per-XCD L2s)
    hipLaunchKernelGGL(scan_counts, dim3(2), dim3(1024), 0, stream, cnt_in, cnt_out, N, in_ptr, out_ptr, cur_in, cur_out);
    if (n_edges > 0) {
        if (small_n)
            hipLaunchKernelGGL(fill_rows_lds, dim3(cdiv(n_edges, kEdgesPerBlock)), dim3(kT), 0, stream, edge_index, n_edges,
                               static_cast<int>(N), cur_in, cur_out, tmp_in, tmp_out);
        else
            hipLaunchKernelGGL(fill_rows, dim3(cdiv(n_edges, kT)), dim3(kT), 0, stream, edge_index, n_edges, cur_in, cur_out,
                               tmp_in, tmp_out);
        const int64_t n_wave_blocks = cdiv(2 * N * 64, kT);
        hipLaunchKernelGGL(sort_rows, dim3(static_cast<unsigned>(n_wave_blocks + 2 * N)), dim3(kT), 0, stream, n_wave_blocks, in_ptr, out_ptr, N,
                           tmp_in, tmp_out, edge_index, n_edges, in_eid, in_src, out_eid, out_dst);
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_graph_build_src_sorted_workspace_bytes(int64_t n_edges, int64_t N) {
    return graph_src_sorted_workspace_bytes(n_edges < 0 ? 0 : n_edges, N < 0 ? 0 : N);
}

int sgs_graph_build_src_sorted(const int64_t* edge_index, int64_t n_edges, int64_t N, int32_t* in_ptr, int32_t* in_src, int32_t* in_eid,
                               int32_t* out_ptr, int32_t* out_dst, int32_t* out_eid, int32_t* loop_eid, int32_t* unsorted, void* ws,
                               size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n_edges >= 0 && N >= 0 && n_edges < (int64_t(1) << 31) && N < (int64_t(1) << 31), SGS_EINVAL,
                "sgs_graph_build_src_sorted: sizes out of range (n_edges=%lld N=%lld)", (long long)n_edges, (long long)N);
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(in_ptr && out_ptr && loop_eid && (n_edges == 0 || (edge_index && in_src && in_eid && out_dst && out_eid)), SGS_EINVAL,
                "sgs_graph_build_src_sorted: null pointer");
    SGS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0, SGS_EINVAL, "sgs_graph_build_src_sorted: workspace must be 256-B aligned");
    return graph_build_src_sorted(edge_index, n_edges, N, in_ptr, in_src, in_eid, out_ptr, out_dst, out_eid, loop_eid, unsorted, ws, ws_bytes, stream);
}

size_t sgs_graph_filter_workspace_bytes(int64_t E_parent, int64_t N) {
    if (E_parent < 0) E_parent = 0;
    if (N < 0) N = 0;
    return 4 * carve_bytes(N + 1, 4) + carve_bytes(E_parent + 1, 4) + carve_bytes(E_parent / 32 + 2, 4) + 256;
}

int sgs_graph_filter(const int32_t* pin_ptr, const int32_t* pin_src, const int32_t* pin_eid, const int32_t* pout_ptr,
                     const int32_t* pout_dst, const int32_t* pout_eid, int64_t E_parent, int64_t N, const uint8_t* mask,
                     const int64_t* sampled_eid, int64_t q, int32_t* in_ptr, int32_t* in_src, int32_t* in_eid, int32_t* out_ptr,
                     int32_t* out_dst, int32_t* out_eid, int32_t* loop_eid, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(E_parent >= 0 && N >= 0 && q >= 0 && q <= E_parent && E_parent < (int64_t(1) << 31) && N < (int64_t(1) << 30), SGS_EINVAL,
                "sgs_graph_filter: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(pin_ptr && pout_ptr && in_ptr && out_ptr && loop_eid && (E_parent == 0 || (pin_src && pin_eid && pout_dst && pout_eid && mask)) &&
                    (q == 0 || (sampled_eid && in_src && in_eid && out_dst && out_eid)), SGS_EINVAL, "sgs_graph_filter: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_graph_filter_workspace_bytes(E_parent, N), SGS_EWORKSPACE, "sgs_graph_filter: workspace too small");
    Carver cv(ws);
    int* cnt_in = cv.take<int>(N + 1);
    int* cnt_out = cv.take<int>(N + 1);
    int* cur_in = cv.take<int>(N + 1);       // scan_counts also initialises fill cursors; unused here
    int* cur_out = cv.take<int>(N + 1);
    int* pos = cv.take<int>(E_parent + 1);
    uint32_t* bits = cv.take<uint32_t>(E_parent / 32 + 2);
    const int64_t n_row_blocks = cdiv(2 * N * 64, kT);
    const dim3 g1(static_cast<unsigned>(n_row_blocks + cdiv(q, kT))), g3(static_cast<unsigned>(n_row_blocks)), blk(kT);
    if (E_parent >= (int64_t(1) << 23)) {
        hipLaunchKernelGGL(pack_mask_bits, dim3(static_cast<unsigned>(cdiv(cdiv(E_parent, 32), kT))), blk, 0, stream, mask, E_parent, bits);
        const uint8_t* bm = reinterpret_cast<const uint8_t*>(bits);
        hipLaunchKernelGGL(filter_count_scatter<true>, g1, blk, 0, stream, pin_ptr, pin_eid, pout_ptr, pout_eid, N, bm, sampled_eid, q, n_row_blocks,
                           cnt_in, cnt_out, pos);
        hipLaunchKernelGGL(scan_counts, dim3(2), dim3(1024), 0, stream, cnt_in, cnt_out, N, in_ptr, out_ptr, cur_in, cur_out);
        hipLaunchKernelGGL(filter_fill<true>, g3, blk, 0, stream, pin_ptr, pin_src, pin_eid, pout_ptr, pout_dst, pout_eid, N, bm, pos, in_ptr, in_src,
                           in_eid, out_ptr, out_dst, out_eid, loop_eid);
    } else if (N <= kSelfScanRows) {
        hipLaunchKernelGGL(filter_count_scatter<false>, g1, blk, 0, stream, pin_ptr, pin_eid, pout_ptr, pout_eid, N, mask, sampled_eid, q,
                           n_row_blocks, cnt_in, cnt_out, pos);
        hipLaunchKernelGGL((filter_fill<false, true>), g3, blk, 0, stream, pin_ptr, pin_src, pin_eid, pout_ptr, pout_dst, pout_eid, N, mask, pos,
                           in_ptr, in_src, in_eid, out_ptr, out_dst, out_eid, loop_eid, static_cast<const int*>(cnt_in),
                           static_cast<const int*>(cnt_out));
    } else {
        hipLaunchKernelGGL(filter_count_scatter<false>, g1, blk, 0, stream, pin_ptr, pin_eid, pout_ptr, pout_eid, N, mask, sampled_eid, q,
                           n_row_blocks, cnt_in, cnt_out, pos);
        hipLaunchKernelGGL(scan_counts, dim3(2), dim3(1024), 0, stream, cnt_in, cnt_out, N, in_ptr, out_ptr, cur_in, cur_out);
        hipLaunchKernelGGL(filter_fill<false>, g3, blk, 0, stream, pin_ptr, pin_src, pin_eid, pout_ptr, pout_dst, pout_eid, N, mask, pos, in_ptr,
                           in_src, in_eid, out_ptr, out_dst, out_eid, loop_eid);
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_edge_mates_workspace_bytes(int64_t n_edges) { return carve_bytes(n_edges < 0 ? 0 : n_edges, 4) + 256; }

int sgs_edge_mates(const int64_t* edge_index, int64_t n_edges, int64_t N, const int32_t* out_ptr, const int32_t* out_dst,
                   const int32_t* out_eid, int32_t* mate, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n_edges >= 0 && N >= 0 && n_edges < (int64_t(1) << 31), SGS_EINVAL, "sgs_edge_mates: bad sizes");
    if (n_edges == 0) return SGS_OK;
    SGS_REQUIRE(edge_index && out_ptr && out_dst && out_eid && mate, SGS_EINVAL, "sgs_edge_mates: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_edge_mates_workspace_bytes(n_edges), SGS_EWORKSPACE, "sgs_edge_mates: workspace too small");
    Carver cv(ws);
    int* rev = cv.take<int>(n_edges);
    const dim3 g(static_cast<unsigned>(cdiv(n_edges, kT))), blk(kT);
    hipLaunchKernelGGL(edge_reverse, g, blk, 0, stream, edge_index, n_edges, out_ptr, out_dst, out_eid, rev);
    hipLaunchKernelGGL(edge_mate, g, blk, 0, stream, rev, n_edges, mate);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gcn_norm_fwd(const float* w, int64_t n_edges, int64_t N, const int32_t* in_ptr, const int32_t* in_src,
                     const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                     const int32_t* loop_eid, float* dis, float* loopw, float* what_in, float* what_out, float* what_loop,
                     sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_gcn_norm_fwd: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(in_ptr && out_ptr && loop_eid && dis && loopw && what_loop, SGS_EINVAL, "sgs_gcn_norm_fwd: null pointer");
    hipLaunchKernelGGL(norm_deg, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, w, N, in_ptr, in_src, in_eid, loop_eid, dis, loopw);
    hipLaunchKernelGGL(norm_weights, dim3(cdiv(2 * N * 64, kT)), dim3(kT), 0, stream, w, N, n_edges, in_ptr, in_src, in_eid,
                       out_ptr, out_dst, out_eid, dis, loopw, what_in, what_out, what_loop);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gcn_degree_partial(const float* w, int64_t n_edges, int64_t N, const int32_t* in_ptr, const int32_t* in_src,
                           const int32_t* in_eid, float* degpart, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_gcn_degree_partial: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(in_ptr && degpart, SGS_EINVAL, "sgs_gcn_degree_partial: null pointer");
    hipLaunchKernelGGL(deg_partial, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, w, N, in_ptr, in_src, in_eid, degpart);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gcn_norm_from_degree(const float* w, const float* degsum, int64_t n_edges, int64_t N, const int32_t* in_ptr,
                             const int32_t* in_src, const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst,
                             const int32_t* out_eid, float* dis, float* loopw, float* what_in, float* what_out,
                             float* what_loop, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_gcn_norm_from_degree: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(degsum && in_ptr && out_ptr && dis && loopw && what_loop, SGS_EINVAL, "sgs_gcn_norm_from_degree: null pointer");
    hipLaunchKernelGGL(dis_from_degree, dim3(cdiv(N, kT)), dim3(kT), 0, stream, degsum, N, dis, loopw);
    hipLaunchKernelGGL(norm_weights, dim3(cdiv(2 * N * 64, kT)), dim3(kT), 0, stream, w, N, n_edges, in_ptr, in_src, in_eid,
                       out_ptr, out_dst, out_eid, dis, loopw, what_in, what_out, what_loop);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_bias_act(const float* X, const float* bias, int64_t N, int64_t D, int act, float p_drop, uint64_t seed, uint32_t site,
                 float* Y, sgs_stream_t stream_) {
    return sgs_bias_act_rows(X, bias, N, D, 0, act, p_drop, seed, site, Y, stream_);
}

int sgs_bias_act_rows(const float* X, const float* bias, int64_t N, int64_t D, int64_t row_offset, int act, float p_drop, uint64_t seed,
                      uint32_t site, float* Y, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D >= 0 && D < (int64_t(1) << 32), SGS_EINVAL, "sgs_bias_act: bad arguments");
    ActDrop ad;
    if (int rc = act_drop("sgs_bias_act", act, p_drop, &ad)) return rc;
    if (N * D == 0) return SGS_OK;
    SGS_REQUIRE(X && Y, SGS_EINVAL, "sgs_bias_act: null pointer");
    hipLaunchKernelGGL(bias_act, dim3(cdiv(N * D, kT)), dim3(kT), 0, stream, X, bias, N, D, ad.act, ad.scale, ad.thresh, seed, site, epoch_ptr(), Y,
                       row_offset);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_mean_weights(int64_t n_edges, int64_t N, const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* out_dst,
                     float* what_in, float* what_out, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_mean_weights: bad sizes");
    if (N == 0 || n_edges == 0) return SGS_OK;
    SGS_REQUIRE(in_ptr && out_ptr && out_dst && what_in && what_out, SGS_EINVAL, "sgs_mean_weights: null pointer");
    hipLaunchKernelGGL(mean_weights, dim3(cdiv(2 * N * 64, kT)), dim3(kT), 0, stream, N, in_ptr, out_ptr, out_dst, what_in, what_out);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_degree_prior_logits(const int64_t* edge_index, int64_t E, int64_t N, const int32_t* in_ptr, const int32_t* out_ptr,
                            float* logits, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && E >= 0, SGS_EINVAL, "sgs_degree_prior_logits: bad sizes");
    if (E == 0) return SGS_OK;
    SGS_REQUIRE(edge_index && in_ptr && out_ptr && logits, SGS_EINVAL, "sgs_degree_prior_logits: null pointer");
    const float scale = static_cast<float>(1.0 / sqrt(static_cast<double>(E)));          // len(prob) ** -0.5
    hipLaunchKernelGGL(degree_prior_logits, dim3(cdiv(E, kT)), dim3(kT), 0, stream, edge_index, E, in_ptr, out_ptr, scale, logits);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_gcn_norm_bwd_workspace_bytes(int64_t N) { return carve_bytes(N < 0 ? 0 : N, 4) + 256; }

int sgs_gcn_norm_bwd(const float* w, const float* gw_hat, const float* gloop, int64_t n_edges, int64_t N,
                     const float* dis, const float* loopw, const int32_t* in_ptr, const int32_t* in_src,
                     const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                     const int32_t* loop_eid, const int64_t* edge_index, float* dw, void* ws, size_t ws_bytes,
                     sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_gcn_norm_bwd: bad sizes");
    if (N == 0 || n_edges == 0) return SGS_OK;
    SGS_REQUIRE(w && gw_hat && gloop && dis && loopw && dw && edge_index, SGS_EINVAL, "sgs_gcn_norm_bwd: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_gcn_norm_bwd_workspace_bytes(N), SGS_EWORKSPACE, "sgs_gcn_norm_bwd: workspace too small");
    Carver cv(ws);
    float* Hn = cv.take<float>(N);
    hipLaunchKernelGGL(norm_bwd_node, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, w, gw_hat, gloop, N, in_ptr, in_src, in_eid,
                       out_ptr, out_dst, out_eid, dis, loopw, Hn);
    hipLaunchKernelGGL(norm_bwd_edge, dim3(cdiv(n_edges, kT)), dim3(kT), 0, stream, gw_hat, gloop, edge_index, n_edges, loop_eid,
                       dis, Hn, dw);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

/* The same with up to two upstream gradients summed on read (gw_hat2 / gloop2: the second GCN layer over the same normalisation) and
 * another consumer's d w added on the way out (dw_add, may be dw itself: in-place accumulation) -- the adds autograd would launch. */
int sgs_gcn_norm_bwd_sum(const float* w, const float* gw_hat, const float* gloop, const float* gw_hat2, const float* gloop2, const float* dw_add,
                         int64_t n_edges, int64_t N, const float* dis, const float* loopw, const int32_t* in_ptr, const int32_t* in_src,
                         const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                         const int32_t* loop_eid, const int64_t* edge_index, float* dw, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_gcn_norm_bwd_sum: bad sizes");
    if (N == 0 || n_edges == 0) return SGS_OK;
    SGS_REQUIRE(w && gw_hat && gloop && dis && loopw && dw && edge_index && ((gw_hat2 != nullptr) == (gloop2 != nullptr)), SGS_EINVAL,
                "sgs_gcn_norm_bwd_sum: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_gcn_norm_bwd_workspace_bytes(N), SGS_EWORKSPACE, "sgs_gcn_norm_bwd_sum: workspace too small");
    Carver cv(ws);
    float* Hn = cv.take<float>(N);
    hipLaunchKernelGGL(norm_bwd_node, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, w, gw_hat, gloop, N, in_ptr, in_src, in_eid,
                       out_ptr, out_dst, out_eid, dis, loopw, Hn, gw_hat2, gloop2);
    hipLaunchKernelGGL(norm_bwd_edge, dim3(cdiv(n_edges, kT)), dim3(kT), 0, stream, gw_hat, gloop, edge_index, n_edges, loop_eid,
                       dis, Hn, dw, gw_hat2, gloop2, dw_add);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

/* Edge-sharded gcn_norm backward: the per-node term Hn is linear in its edge contributions, so each rank
 * computes its partial (gloop only on the rank that owns the self-loop term), the host all-reduces Hn, and
 * the per-edge pass finishes locally. */
int sgs_gcn_norm_bwd_node(const float* w, const float* gw_hat, const float* gloop, int64_t n_edges, int64_t N, const float* dis,
                          const float* loopw, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                          const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* Hn,
                          sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_gcn_norm_bwd_node: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(w && gw_hat && gloop && dis && loopw && Hn, SGS_EINVAL, "sgs_gcn_norm_bwd_node: null pointer");
    hipLaunchKernelGGL(norm_bwd_node, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, w, gw_hat, gloop, N, in_ptr, in_src, in_eid, out_ptr,
                       out_dst, out_eid, dis, loopw, Hn);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gcn_norm_bwd_edge(const float* gw_hat, const float* gloop, int64_t n_edges, int64_t N, const float* dis,
                          const int32_t* loop_eid, const int64_t* edge_index, const float* Hn, float* dw, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_gcn_norm_bwd_edge: bad sizes");
    if (n_edges == 0) return SGS_OK;
    SGS_REQUIRE(gw_hat && gloop && dis && loop_eid && edge_index && Hn && dw, SGS_EINVAL, "sgs_gcn_norm_bwd_edge: null pointer");
    hipLaunchKernelGGL(norm_bwd_edge, dim3(cdiv(n_edges, kT)), dim3(kT), 0, stream, gw_hat, gloop, edge_index, n_edges, loop_eid, dis, Hn, dw);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

/* Which kernel the launchers below pick -- pure host functions of the shape: the code of the launchers' own plan (spmm_plan.h).
 * sgs_spmm_csr_variant / sgs_sddmm_csr_variant:  kind * 1000 + VEC * 100 + W
 *   kind 0: a group of W = LPR lanes per row (spmm_csr<VEC, LPR> / sddmm_csr<VEC, LPR>), LPR = the power of two >= ceil(D / VEC), at most 64
 *   kind 1: a workgroup of W = NW waves per row (spmm_csr_rowblock<VEC, NW> / sddmm_csr_rowblock<VEC, NW>)
 *   VEC = 4 iff D % 4 == 0 and both dense operands are 16-byte aligned (aligned16 != 0), else 1. */
int sgs_spmm_csr_variant(int64_t N, int64_t D, int64_t nnz, int al16) { return spmm_plan(N, D, nnz, al16 != 0).code(); }

int sgs_spmm_long_rows_set(int on) {
    const int prev = g_spmm_long_rows;
    g_spmm_long_rows = on ? 1 : 0;
    return prev;
}
int sgs_spmm_long_rows_threshold(void) { return kSpmmLongRow; }
int sgs_spmm_long_rows_active(int64_t N, int64_t D) { return spmm_long_rows_on(N, D) ? 1 : 0; }

// long rows (partitions; whole graphs of average degree >= 16) at any N: a workgroup per row, 16 waves from 64 entries a row
int sgs_sddmm_csr_variant(int64_t N, int64_t D, int64_t nnz, int al16) {
    return spmm_row_form(N, D, nnz, (D % 4 == 0 && al16) ? 4 : 1, INT64_MAX, 64).code();
}

int sgs_spmm_csr(const float* X, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col, const float* val,
                 const float* diag, const float* bias, int act, float p_drop, uint64_t seed, uint32_t site, float* Y,
                 sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D >= 0, SGS_EINVAL, "sgs_spmm_csr: bad sizes");
    ActDrop ad;
    if (int rc = act_drop("sgs_spmm_csr", act, p_drop, &ad)) return rc;
    if (N == 0 || D == 0) return SGS_OK;
    SGS_REQUIRE(X && ptr && Y && X != Y, SGS_EINVAL, "sgs_spmm_csr: null or aliased pointer");
    const SpmmPlan p = gcn_spmm_plan(N, D, nnz, aligned16(X) && aligned16(Y));
    const dim3 g_(p.blocks(N)), b_(p.block());
    if (p.kind)
        dispatch_waves_long(p, [&](auto V, auto W, auto L) {
            hipLaunchKernelGGL((spmm_csr_rowblock<V(), W(), L()>), g_, b_, 0, stream, X, N, D, ptr, col, val, diag, bias, ad.act, ad.scale, ad.thresh,
                               seed, site, epoch_ptr(), Y);
        });
    else
        dispatch_lanes(p, [&](auto V, auto W) {
            hipLaunchKernelGGL((spmm_csr<V(), W()>), g_, b_, 0, stream, X, N, D, ptr, col, val, diag, bias, ad.act, ad.scale, ad.thresh, seed, site,
                               epoch_ptr(), Y);
        });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_sddmm_csr(const float* A, const float* B, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col,
                  const int32_t* eid, float* g, float* gdiag, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D >= 0, SGS_EINVAL, "sgs_sddmm_csr: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(A && B && ptr, SGS_EINVAL, "sgs_sddmm_csr: null pointer");
    const SpmmPlan p = SpmmPlan::of_code(sgs_sddmm_csr_variant(N, D, nnz, aligned16(A) && aligned16(B)));
    const dim3 g_(p.blocks(N)), b_(p.block());
    dispatch_plan(p, [&](auto V, auto W) { hipLaunchKernelGGL((sddmm_csr<V(), W()>), g_, b_, 0, stream, A, B, N, D, ptr, col, eid, g, gdiag); },
                  [&](auto V, auto W) { hipLaunchKernelGGL((sddmm_csr_rowblock<V(), W()>), g_, b_, 0, stream, A, B, N, D, ptr, col, eid, g, gdiag); });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_act_bwd(const float* dY, const float* Y, int64_t n, int act, float p_drop, float* dZ, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n >= 0, SGS_EINVAL, "sgs_act_bwd: bad arguments");
    ActDrop ad;
    if (int rc = act_drop("sgs_act_bwd", act, p_drop, &ad)) return rc;
    if (n == 0) return SGS_OK;
    SGS_REQUIRE(dY && dZ && (act == SGS_ACT_NONE || Y), SGS_EINVAL, "sgs_act_bwd: null pointer");
    hipLaunchKernelGGL(act_bwd, dim3(cdiv(n, kT)), dim3(kT), 0, stream, dY, Y, n, ad.act, ad.scale, dZ);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_colsum_workspace_bytes(int64_t N, int64_t D) {
    if (N < 0) N = 0;
    if (D < 0) D = 0;
    return carve_bytes(static_cast<size_t>(cdiv(N, colsum_rows(N)) + 1) * D, 4) + 256;
}

/* Which kernels sgs_colsum (fused_act = 0) / sgs_act_bwd_colsum (fused_act != 0) launch:  kind * 1000000 + F * 100000 + rows * 100 + RG
 *   kind 1: colsum_small<F>      (0 < N <= 2048, D % 4 != 0)        kind 2: colsum_small_v4<F>   (0 < N <= 2048, D % 4 == 0)
 *   kind 3: vecsum_small         (D == 1, 2048 < N <= 2^20)         kind 4: colsum_partial over `rows` rows per chunk (32 | 128 | 256),
 *                                                                           then colsum_final<RG> (16 when there are more than 64 chunks, else 4)
 *   F = 1: the activation backward rides along -- inside the kernel for kinds 1 and 2, as an act_bwd launch in front of kinds 3 and 4;
 *   rows = RG = 0 for kinds 1 to 3. */
int sgs_colsum_variant(int64_t N, int64_t D, int fused_act) {
    const int f = fused_act ? 100000 : 0;
    if (N > 0 && N <= kColSmallRows) return (D % 4 == 0 ? 2000000 : 1000000) + f;
    if (D == 1 && N > 0 && N <= kVecSumMax) return 3000000 + f;
    const int rows = colsum_rows(N);
    return 4000000 + f + rows * 100 + (cdiv(N, rows) > 64 ? 16 : 4);
}

int sgs_colsum(const float* A, int64_t N, int64_t D, float* out, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D >= 0, SGS_EINVAL, "sgs_colsum: bad sizes");
    if (D == 0) return SGS_OK;
    SGS_REQUIRE(out && (N == 0 || A), SGS_EINVAL, "sgs_colsum: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_colsum_workspace_bytes(N, D), SGS_EWORKSPACE, "sgs_colsum: workspace too small");
    const int var = sgs_colsum_variant(N, D, 0);
    switch (var / 1000000) {
        case 1:
            // (round 1 tried a single launch with 64-column workgroups, N/16 rows per thread: slower than the two stages by 12 us per
            //  backward; with 16-column workgroups a thread walks N/64 rows and all of its loads are in flight together)
            hipLaunchKernelGGL(colsum_small<false>, dim3(cdiv(D, 16)), dim3(1024), 0, stream, A, static_cast<const float*>(nullptr), N, D, SGS_ACT_NONE, 1.f,
                               static_cast<float*>(nullptr), out);
            break;
        case 2:
            hipLaunchKernelGGL(colsum_small_v4<false>, dim3(cdiv(D, 16)), dim3(1024), 0, stream, A, static_cast<const float*>(nullptr), N, D, SGS_ACT_NONE,
                               1.f, static_cast<float*>(nullptr), out);
            break;
        case 3:
            hipLaunchKernelGGL(vecsum_small, dim3(1), dim3(1024), 0, stream, A, N, out);
            break;
        default: {
            Carver cv(ws);
            const int rows = var / 100 % 1000;
            const int64_t nchunk = cdiv(N, rows);
            float* part = cv.take<float>(static_cast<size_t>(nchunk + 1) * D);
            if (nchunk > 0)
                hipLaunchKernelGGL(colsum_partial, dim3(cdiv(D, 64), nchunk), dim3(kT), 0, stream, A, N, D, rows, part);
            if (var % 100 == 16) hipLaunchKernelGGL(colsum_final<16>, dim3(cdiv(D, 64)), dim3(1024), 0, stream, part, nchunk, D, out);
            else                 hipLaunchKernelGGL(colsum_final<4>, dim3(cdiv(D, 64)), dim3(kT), 0, stream, part, nchunk, D, out);
        }
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}


int sgs_act_bwd_colsum(const float* dY, const float* Y, int64_t N, int64_t D, int act, float p_drop, float* dZ, float* colsum, void* ws,
                       size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D >= 0, SGS_EINVAL, "sgs_act_bwd_colsum: bad arguments");
    ActDrop ad;
    if (int rc = act_drop("sgs_act_bwd_colsum", act, p_drop, &ad)) return rc;
    if (D == 0) return SGS_OK;
    SGS_REQUIRE(colsum && (N == 0 || (dZ && dY && (act == SGS_ACT_NONE || Y))), SGS_EINVAL, "sgs_act_bwd_colsum: null pointer");   // (an empty dZ has no address)
    switch (sgs_colsum_variant(N, D, 1) / 1000000) {
        case 1:
            hipLaunchKernelGGL(colsum_small<true>, dim3(cdiv(D, 16)), dim3(1024), 0, stream, dY, Y, N, D, ad.act, ad.scale, dZ, colsum);
            break;
        case 2:
            hipLaunchKernelGGL(colsum_small_v4<true>, dim3(cdiv(D, 16)), dim3(1024), 0, stream, dY, Y, N, D, ad.act, ad.scale, dZ, colsum);
            break;
        default:
            if (int rc = sgs_act_bwd(dY, Y, N * D, act, p_drop, dZ, stream_)) return rc;
            return sgs_colsum(dZ, N, D, colsum, ws, ws_bytes, stream_);
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}

// ---- GCN layer pairs (spmm_rowgroup_pair): only where sgs_spmm_csr takes its row-block path
int sgs_gcn_pair_ok(int64_t N, int64_t nnz, int64_t D) {
    return (N > 0 && D > 0 && D <= kPairMaxD && spmm_plan(N, D, nnz, false).kind == 1) ? 1 : 0;
}

int sgs_spmm_csr_next(const float* X, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col, const float* val,
                      const float* diag, const float* bias, int act, float p_drop, uint64_t seed, uint32_t site, const float* Wn, int64_t Dn,
                      float* Y, float* Z, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(sgs_gcn_pair_ok(N, nnz, D) && Dn > 0, SGS_EINVAL, "sgs_spmm_csr_next: not a row-block shape (see sgs_gcn_pair_ok)");
    ActDrop ad;
    if (int rc = act_drop("sgs_spmm_csr_next", act, p_drop, &ad)) return rc;
    SGS_REQUIRE(X && ptr && Y && Wn && Z && X != Y && Z != Y && Z != X, SGS_EINVAL, "sgs_spmm_csr_next: null or aliased pointer");
    const SpmmPlan p = gcn_spmm_plan(N, D, nnz, aligned16(X) && aligned16(Y));      // (as sgs_spmm_csr: Y is bitwise its result)
    dispatch_waves_long(p, [&](auto V, auto W, auto L) {
        hipLaunchKernelGGL((spmm_rowgroup_pair<V(), W(), kPairFwd, L()>), pair_grid(p, N), dim3(1024), 0, stream, X, N, D, ptr, col, val, diag, bias,
                           ad.act, ad.scale, ad.thresh, seed, site, epoch_ptr(), Y, Wn, Dn, static_cast<const float*>(nullptr), Z, 0,
                           static_cast<float*>(nullptr));
    });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_spmm_csr_bwd_prev(const float* dZ, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col, const float* val,
                          const float* diag, const float* W, int64_t Dp, const float* Yp, int act, float p_drop, float* dX, float* dZp,
                          float* colsum, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(sgs_gcn_pair_ok(N, nnz, D), SGS_EINVAL, "sgs_spmm_csr_bwd_prev: not a row-block shape (see sgs_gcn_pair_ok)");
    ActDrop ad;
    if (int rc = act_drop("sgs_spmm_csr_bwd_prev", act, p_drop, &ad)) return rc;
    SGS_REQUIRE(dZ && ptr && dX && dZ != dX, SGS_EINVAL, "sgs_spmm_csr_bwd_prev: null or aliased pointer");
    SGS_REQUIRE(!W || (Dp > 0 && dZp && (act == SGS_ACT_NONE || Yp) && dZp != dX && dZp != dZ), SGS_EINVAL,
                "sgs_spmm_csr_bwd_prev: W needs Dp > 0, dZp and (with an activation) Yp");
    const SpmmPlan p = gcn_spmm_plan(N, D, nnz, aligned16(dZ) && aligned16(dX));
    const int ncs = colsum ? static_cast<int>(cdiv(D, 16)) : 0;
    dispatch_waves_long(p, [&](auto V, auto W_, auto L) {
        const float* const no_bias = nullptr;
        const uint64_t* const no_epoch = nullptr;
        if (W)
            hipLaunchKernelGGL((spmm_rowgroup_pair<V(), W_(), kPairBwd, L()>), pair_grid(p, N, ncs), dim3(1024), 0, stream, dZ, N, D, ptr, col, val, diag,
                               no_bias, ad.act, ad.scale, 0u, uint64_t(0), 0u, no_epoch, dX, W, Dp, Yp, dZp, ncs, colsum);
        else
            hipLaunchKernelGGL((spmm_rowgroup_pair<V(), W_(), kPairCol, L()>), pair_grid(p, N, ncs), dim3(1024), 0, stream, dZ, N, D, ptr, col, val, diag,
                               no_bias, int(SGS_ACT_NONE), 1.f, 0u, uint64_t(0), 0u, no_epoch, dX, no_bias, int64_t(0), no_bias,
                               static_cast<float*>(nullptr), ncs, colsum);
    });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

// ---- two-job forms of the GNN head's two forward launches (spmm_rowgroup_pair_dual, spmm_csr_rowblock_dual)
int sgs_gcn_dual_ok(int64_t N, int64_t nnz_a, int64_t nnz_b, int64_t D, int64_t Dn) {
    return (sgs_gcn_pair_ok(N, nnz_a, D) && sgs_gcn_pair_ok(N, nnz_b, D) && Dn > 0 &&
            spmm_plan(N, D, nnz_a, false).w == spmm_plan(N, D, nnz_b, false).w) ? 1 : 0;
}

int sgs_spmm_csr_next_dual(const float* X, int64_t N, int64_t D, const float* bias, int act, float p_drop, uint32_t site, const float* Wn,
                           int64_t Dn, int64_t nnz_a, const int32_t* ptr_a, const int32_t* col_a, const float* val_a, const float* diag_a,
                           uint64_t seed_a, float* Y_a, float* Z_a, int64_t nnz_b, const int32_t* ptr_b, const int32_t* col_b,
                           const float* val_b, const float* diag_b, uint64_t seed_b, float* Y_b, float* Z_b, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(sgs_gcn_dual_ok(N, nnz_a, nnz_b, D, Dn), SGS_EINVAL, "sgs_spmm_csr_next_dual: not two row-block shapes of one variant (see sgs_gcn_dual_ok)");
    ActDrop ad;
    if (int rc = act_drop("sgs_spmm_csr_next_dual", act, p_drop, &ad)) return rc;
    SGS_REQUIRE(X && ptr_a && ptr_b && Y_a && Y_b && Wn && Z_a && Z_b && X != Y_a && X != Y_b && X != Z_a && X != Z_b && Y_a != Y_b &&
                    Z_a != Z_b && Y_a != Z_a && Y_a != Z_b && Y_b != Z_a && Y_b != Z_b,
                SGS_EINVAL, "sgs_spmm_csr_next_dual: null or aliased pointer");
    const SpmmPlan p = gcn_spmm_plan(N, D, nnz_a, aligned16(X) && aligned16(Y_a));      // (per job as sgs_spmm_csr_next picks it)
    SGS_REQUIRE(p.vec == gcn_spmm_plan(N, D, nnz_b, aligned16(X) && aligned16(Y_b)).vec, SGS_EINVAL,
                "sgs_spmm_csr_next_dual: the two jobs select different kernel variants (alignment)");
    SpmmDualArgs a;
    a.job[0] = SpmmDualJob{X, ptr_a, col_a, val_a, diag_a, Y_a, Z_a, nnz_a, seed_a};
    a.job[1] = SpmmDualJob{X, ptr_b, col_b, val_b, diag_b, Y_b, Z_b, nnz_b, seed_b};
    dispatch_waves_long(p, [&](auto V, auto W, auto L) {
        hipLaunchKernelGGL((spmm_rowgroup_pair_dual<V(), W(), L()>), pair_grid(p, N, 0, 2), dim3(1024), 0, stream, a, N, D, bias, ad.act, ad.scale,
                           ad.thresh, site, epoch_ptr(), Wn, Dn);
    });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_spmm_csr_dual(const float* X_a, const float* X_b, int64_t N, int64_t D, const float* bias, int act, float p_drop, uint32_t site,
                      int64_t nnz_a, const int32_t* ptr_a, const int32_t* col_a, const float* val_a, const float* diag_a, uint64_t seed_a,
                      float* Y_a, int64_t nnz_b, const int32_t* ptr_b, const int32_t* col_b, const float* val_b, const float* diag_b,
                      uint64_t seed_b, float* Y_b, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N > 0 && D > 0, SGS_EINVAL, "sgs_spmm_csr_dual: bad sizes");
    ActDrop ad;
    if (int rc = act_drop("sgs_spmm_csr_dual", act, p_drop, &ad)) return rc;
    SGS_REQUIRE(X_a && X_b && ptr_a && ptr_b && Y_a && Y_b && Y_a != Y_b && X_a != Y_a && X_a != Y_b && X_b != Y_a && X_b != Y_b, SGS_EINVAL,
                "sgs_spmm_csr_dual: null or aliased pointer");
    const SpmmPlan p = gcn_spmm_plan(N, D, nnz_a, aligned16(X_a) && aligned16(Y_a));
    SGS_REQUIRE(p.kind == 1 && p.code() == gcn_spmm_plan(N, D, nnz_b, aligned16(X_b) && aligned16(Y_b)).code(), SGS_EINVAL,
                "sgs_spmm_csr_dual: not two row-block shapes of one variant (see sgs_spmm_csr_variant)");
    SpmmDualArgs a;
    a.job[0] = SpmmDualJob{X_a, ptr_a, col_a, val_a, diag_a, Y_a, nullptr, nnz_a, seed_a};
    a.job[1] = SpmmDualJob{X_b, ptr_b, col_b, val_b, diag_b, Y_b, nullptr, nnz_b, seed_b};
    dispatch_waves_long(p, [&](auto V, auto W, auto L) {
        hipLaunchKernelGGL((spmm_csr_rowblock_dual<V(), W(), L()>), dim3(p.blocks(N), 2), dim3(p.block()), 0, stream, a, N, D, bias, ad.act, ad.scale,
                           ad.thresh, site, epoch_ptr());
    });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

}  // extern "C"

extern "C" {

size_t sgs_graph_filter_multi_workspace_bytes(int64_t E_parent, int64_t N, int64_t D) {
    if (E_parent < 0) E_parent = 0;
    if (N < 0) N = 0;
    if (D < 1) D = 1;
    return 2 * carve_bytes(static_cast<size_t>(D * (N + 1)), 4) + carve_bytes(static_cast<size_t>(D * E_parent + 1), 4) + 256;
}

int sgs_graph_filter_multi(const int32_t* pin_ptr, const int32_t* pin_src, const int32_t* pin_eid, int64_t E_parent, int64_t N, int64_t D,
                           const uint8_t* mask, const int64_t* sampled_eid, int64_t q, int32_t* in_ptr, int32_t* in_src, int32_t* in_eid,
                           int32_t* loop_eid, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(E_parent >= 0 && N >= 0 && q >= 0 && q <= E_parent && E_parent < (int64_t(1) << 31) && N < (int64_t(1) << 30) && D >= 1 &&
                    D <= 65535, SGS_EINVAL, "sgs_graph_filter_multi: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(pin_ptr && in_ptr && loop_eid && (E_parent == 0 || (pin_src && pin_eid && mask)) &&
                    (q == 0 || (sampled_eid && in_src && in_eid)), SGS_EINVAL, "sgs_graph_filter_multi: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_graph_filter_multi_workspace_bytes(E_parent, N, D), SGS_EWORKSPACE,
                "sgs_graph_filter_multi: workspace too small");
    Carver cv(ws);
    int* cnt = cv.take<int>(D * (N + 1));
    int* cur = cv.take<int>(D * (N + 1));
    int* pos = cv.take<int>(D * E_parent + 1);
    const unsigned Du = static_cast<unsigned>(D);
    const int64_t n_row_blocks = cdiv(N * 64, kT);
    const dim3 g1(static_cast<unsigned>(n_row_blocks + cdiv(q, kT)), Du), g3(static_cast<unsigned>(n_row_blocks), Du), blk(kT);
    hipLaunchKernelGGL(multi_filter_count, g1, blk, 0, stream, pin_ptr, pin_eid, N, E_parent, mask, sampled_eid, q, n_row_blocks, cnt, pos);
    if (N <= kSelfScanRows) {
        hipLaunchKernelGGL(multi_filter_fill<true>, g3, blk, 0, stream, pin_ptr, pin_src, pin_eid, N, E_parent, q, mask, pos, in_ptr, in_src, in_eid,
                           loop_eid, static_cast<const int*>(cnt));
    } else {
        hipLaunchKernelGGL(multi_scan_counts, dim3(1, Du), dim3(1024), 0, stream, cnt, N, in_ptr, cur);
        hipLaunchKernelGGL(multi_filter_fill<false>, g3, blk, 0, stream, pin_ptr, pin_src, pin_eid, N, E_parent, q, mask, pos, in_ptr, in_src, in_eid,
                           loop_eid, static_cast<const int*>(cnt));
    }
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gcn_norm_fwd_multi(const float* w, int64_t q, int64_t N, int64_t D, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                           const int32_t* loop_eid, float* dis, float* loopw, float* what_in, float* what_loop, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && q >= 0 && D >= 1 && D <= 65535, SGS_EINVAL, "sgs_gcn_norm_fwd_multi: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(in_ptr && loop_eid && dis && loopw && what_loop && (q == 0 || (in_src && in_eid && what_in)), SGS_EINVAL,
                "sgs_gcn_norm_fwd_multi: null pointer");
    const dim3 g(static_cast<unsigned>(cdiv(N * 64, kT)), static_cast<unsigned>(D));
    hipLaunchKernelGGL(multi_norm_deg, g, dim3(kT), 0, stream, w, q, N, in_ptr, in_src, in_eid, loop_eid, dis, loopw);
    hipLaunchKernelGGL(multi_norm_weights, g, dim3(kT), 0, stream, w, q, N, in_ptr, in_src, in_eid, dis, loopw, what_in, what_loop);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_spmm_csr_multi(const float* X, int64_t x_stride, int64_t N, int64_t Dc, int64_t nnz, int64_t D, const int32_t* ptr, const int32_t* col,
                       const float* val, const float* diag, const float* bias, int act, float* Y, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && Dc >= 0 && nnz >= 0 && D >= 1 && D <= 65535 && x_stride >= 0, SGS_EINVAL, "sgs_spmm_csr_multi: bad sizes");
    SGS_REQUIRE(act == SGS_ACT_NONE || act == SGS_ACT_RELU, SGS_EINVAL, "sgs_spmm_csr_multi: act must be NONE or RELU (forward only)");
    if (N == 0 || Dc == 0) return SGS_OK;
    SGS_REQUIRE(X && ptr && Y && (nnz == 0 || (col && val)), SGS_EINVAL, "sgs_spmm_csr_multi: null pointer");
    SGS_REQUIRE(x_stride == 0 || x_stride >= N * Dc, SGS_EINVAL, "sgs_spmm_csr_multi: x_stride must be 0 (shared X) or >= N * Dc");
    SGS_REQUIRE(X + (D - 1) * x_stride + N * Dc <= Y || Y + D * N * Dc <= X, SGS_EINVAL, "sgs_spmm_csr_multi: X and Y overlap");
    // sgs_spmm_csr's plan on the per-draw entry count, so every draw equals it (16-byte gathers: every draw's block of X aligned as well)
    const SpmmPlan p = gcn_spmm_plan(N, Dc, nnz, x_stride % 4 == 0 && aligned16(X) && aligned16(Y));
    const dim3 g_(p.blocks(N), static_cast<unsigned>(D)), b_(p.block());
    if (p.kind)
        dispatch_waves_long(p, [&](auto V, auto W, auto L) {
            hipLaunchKernelGGL((multi_spmm_csr_rowblock<V(), W(), L()>), g_, b_, 0, stream, X, x_stride, N, Dc, nnz, ptr, col, val, diag, bias, act, Y);
        });
    else
        dispatch_lanes(p, [&](auto V, auto W) {
            hipLaunchKernelGGL((multi_spmm_csr<V(), W()>), g_, b_, 0, stream, X, x_stride, N, Dc, nnz, ptr, col, val, diag, bias, act, Y);
        });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

}  // extern "C"
