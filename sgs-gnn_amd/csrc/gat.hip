// K8: GAT attention (PyG 2.3.1 GATConv) over the dst-sorted CSR (gfx950): the one-head kernels first (what the reference's GATModel runs),
// the fused multi-head ones (2 <= heads <= 16; their own SpMM / SDDMM, since the weights are per head) in the second half of the file.
//
// Reference: model.py:189-208 builds torch_geometric.nn.models.GAT(num_layers=2, act='relu',
// dropout=p); each GATConv layer is
//   x' = lin(x);  a_s = <x', att_src>, a_d = <x', att_dst>                  (node level, host side)
//   existing self loops removed, one loop per node added
//   e_k = leaky_relu(a_s[src_k] + a_d[dst_k], 0.2);  alpha = softmax over each node's in-edges
//   alpha = dropout(alpha, p)  (training);  out[i] = sum_k alpha_k x'[src_k] + bias
// `edge_weight` is ignored by PyG's GAT (supports_edge_weight = False) unless the layers are built with edge_dim = 1:
// the gat_alpha_heads_edge_* kernels below then add the edge term to the logit.
// The aggregation itself reuses sgs_spmm_csr (val = alpha, diag = loop alpha); this file holds the
// segment softmax and its backward.  One wave per destination node; rows are walked three times
// (max, sum, normalise) from L2.
#include <type_traits>

#include "sgs_common.h"

namespace sgs {
namespace {

constexpr int kT = 256;

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : slope * v; }

// alpha_in[k] (dst-CSR order; 0 for (i,i) entries), alpha_loop[i]: post-softmax, post-dropout weights;
// soft_in / soft_loop: the pre-dropout softmax values kept for backward (SOFT = false: not written).  One wave per row i.
template <bool SOFT>
__device__ __forceinline__ void gat_alpha_fwd_body(int64_t i, int lane, const float* __restrict__ a_s, const float* __restrict__ a_d,
                                                   const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                   const int* __restrict__ in_eid, float slope, float drop_scale, uint32_t drop_thresh,
                                                   int use_drop, uint64_t seed, uint32_t site, float* __restrict__ soft_in,
                                                   float* __restrict__ soft_loop, float* __restrict__ alpha_in, float* __restrict__ alpha_loop) {
    const int b = in_ptr[i], e = in_ptr[i + 1];
    const float ad = a_d[i];
    const float eloop = lrelu(a_s[i] + ad, slope);
    float mx = eloop;
    for (int k = b + lane; k < e; k += 64) {
        const int s = in_src[k];
        if (s != static_cast<int>(i)) mx = fmaxf(mx, lrelu(a_s[s] + ad, slope));
    }
    mx = wave_max_all(mx);
    float sum = 0.f;
    for (int k = b + lane; k < e; k += 64) {
        const int s = in_src[k];
        if (s != static_cast<int>(i)) sum += expf(lrelu(a_s[s] + ad, slope) - mx);
    }
    sum = wave_sum_all(sum) + expf(eloop - mx);
    const float inv = 1.0f / (sum + 1e-16f);                  // torch_geometric.utils.softmax: / (sum + 1e-16)
    // attention dropout is keyed by (site, row = edge id) for edges and (site + 1, row = node) for loops
    for (int k = b + lane; k < e; k += 64) {
        const int s = in_src[k];
        float sm = 0.f, al = 0.f;
        if (s != static_cast<int>(i)) {
            sm = expf(lrelu(a_s[s] + ad, slope) - mx) * inv;
            al = sm;
            if (use_drop) al = dropout_keep_at(seed, site, static_cast<uint64_t>(in_eid[k]), 0u, drop_thresh) ? sm * drop_scale : 0.f;
        }
        if (SOFT) soft_in[k] = sm;
        alpha_in[k] = al;
    }
    if (lane == 0) {
        const float sm = expf(eloop - mx) * inv;
        float al = sm;
        if (use_drop) al = dropout_keep_at(seed, site + 1u, static_cast<uint64_t>(i), 0u, drop_thresh) ? sm * drop_scale : 0.f;
        if (SOFT) soft_loop[i] = sm;
        alpha_loop[i] = al;
    }
}

__global__ void __launch_bounds__(kT) gat_alpha_fwd(const float* __restrict__ a_s, const float* __restrict__ a_d, int64_t N,
                                                   const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                   const int* __restrict__ in_eid, float slope, float drop_scale,
                                                   uint32_t drop_thresh, int use_drop, uint64_t seed, uint32_t site,
                                                   const uint64_t* __restrict__ epoch, float* __restrict__ soft_in,
                                                   float* __restrict__ soft_loop, float* __restrict__ alpha_in,
                                                   float* __restrict__ alpha_loop) {
    seed = fold_epoch(seed, epoch);
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    gat_alpha_fwd_body<true>(i, lane, a_s, a_d, in_ptr, in_src, in_eid, slope, drop_scale, drop_thresh, use_drop, seed, site, soft_in, soft_loop,
                             alpha_in, alpha_loop);
}

// D drawn graphs of one partition (ensemble evaluation, no attention dropout): blockIdx.y = draw d, which reads the node scores at
// a_s + d * as, a_d + d * as (as = 0: shared by every draw) and its CSR slices ptr [N+1], src [nnz]; the body above runs unchanged on
// them, so row d of alpha_in [D, nnz] / alpha_loop [D, N] is bitwise what gat_alpha_fwd (p = 0) writes for draw d alone.
__global__ void __launch_bounds__(kT) gat_alpha_fwd_multi(const float* __restrict__ a_s, const float* __restrict__ a_d, int64_t as, int64_t N,
                                                         int64_t nnz, const int* __restrict__ in_ptr, const int* __restrict__ in_src, float slope,
                                                         float* __restrict__ alpha_in, float* __restrict__ alpha_loop) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    const int64_t d = blockIdx.y;
    gat_alpha_fwd_body<false>(i, lane, a_s + d * as, a_d + d * as, in_ptr + d * (N + 1), in_src + d * nnz, nullptr, slope, 1.0f, 0u, 0,
                              uint64_t(0), 0u, nullptr, nullptr, alpha_in + d * nnz, alpha_loop + d * N);
}

// Backward of dropout + softmax + leaky_relu for one destination row:
//   dal_k  = galpha[eid_k] (gradient wrt the dropped alpha; from sgs_sddmm_csr) , dloop = gloop[i]
//   dsm_k  = dal_k * keep_k * scale ;  dot = sum_k sm_k dsm_k (incl. loop)
//   de_k   = sm_k (dsm_k - dot) ;  dpre_k = de_k * (pre_k > 0 ? 1 : slope)
//   ge[eid_k] = dpre_k (-> d a_s[src_k], summed per source by the caller) ; d a_d[i] = sum_k dpre_k ;
//   gsl[i] = dpre_loop  (the loop's contribution to d a_s[i])
__global__ void __launch_bounds__(kT) gat_alpha_bwd(const float* __restrict__ a_s, const float* __restrict__ a_d, int64_t N,
                                                   const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                   const int* __restrict__ in_eid, float slope, float drop_scale,
                                                   uint32_t drop_thresh, int use_drop, uint64_t seed, uint32_t site,
                                                   const uint64_t* __restrict__ epoch,
                                                   const float* __restrict__ soft_in, const float* __restrict__ soft_loop,
                                                   const float* __restrict__ galpha, const float* __restrict__ gloop,
                                                   float* __restrict__ ge, float* __restrict__ gsl, float* __restrict__ d_ad) {
    seed = fold_epoch(seed, epoch);
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    const int b = in_ptr[i], e = in_ptr[i + 1];
    const float ad = a_d[i];
    auto dsm_edge = [&](int k) {
        float g = galpha[in_eid[k]];
        if (use_drop) g = dropout_keep_at(seed, site, static_cast<uint64_t>(in_eid[k]), 0u, drop_thresh) ? g * drop_scale : 0.f;
        return g;
    };
    float gl = gloop[i];
    if (use_drop) gl = dropout_keep_at(seed, site + 1u, static_cast<uint64_t>(i), 0u, drop_thresh) ? gl * drop_scale : 0.f;
    float dot = 0.f;
    for (int k = b + lane; k < e; k += 64)
        if (in_src[k] != static_cast<int>(i)) dot += soft_in[k] * dsm_edge(k);
    dot = wave_sum_all(dot) + soft_loop[i] * gl;
    float dad = 0.f;
    for (int k = b + lane; k < e; k += 64) {
        const int s = in_src[k];
        float dpre = 0.f;
        if (s != static_cast<int>(i)) {
            const float pre = a_s[s] + ad;
            dpre = soft_in[k] * (dsm_edge(k) - dot) * (pre > 0.f ? 1.f : slope);
        }
        ge[in_eid[k]] = dpre;
        dad += dpre;
    }
    dad = wave_sum_all(dad);
    if (lane == 0) {
        const float pre = a_s[i] + ad;
        const float dl = soft_loop[i] * (gl - dot) * (pre > 0.f ? 1.f : slope);
        gsl[i] = dl;
        d_ad[i] = dad + dl;
    }
}

// out_order[k] = by_eid[eid[k]]  (re-order a per-edge array into a CSR's entry order)
// `dyn` (sgs_dyn_edges_set): the entries of a staged parent CSR past the live edge count are stale -- n = min(n, *dyn).  (A drawn
// subgraph has q < live edges, so its re-orderings are untouched.)
__global__ void __launch_bounds__(kT) gather_by_eid(const float* __restrict__ by_eid, const int* __restrict__ eid, int64_t n,
                                                   float* __restrict__ out_order, const int64_t* __restrict__ dyn) {
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (dyn && *dyn < n) n = *dyn;
    if (k < n) out_order[k] = by_eid[eid[k]];
}
__global__ void __launch_bounds__(kT) scatter_by_eid(const float* __restrict__ in_order, const int* __restrict__ eid, int64_t n,
                                                    float* __restrict__ by_eid, const int64_t* __restrict__ dyn) {
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (dyn && *dyn < n) n = *dyn;
    if (k < n) by_eid[eid[k]] = in_order[k];
}

// Node-level attention scores a_s = <x', att_src>, a_d = <x', att_dst> in ONE pass over x' (one wave per row, 16-byte loads).  The library
// GEMV the host used for these ran at 280 us per call on [33 869 x 256] (rocprofv3, config 4: 4 calls per step, a fifth of the step).
__global__ void __launch_bounds__(kT) gat_scores_fwd(const float* __restrict__ xl, int64_t N, int64_t D, const float* __restrict__ att_s,
                                                    const float* __restrict__ att_d, float* __restrict__ a_s, float* __restrict__ a_d) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    float s = 0.f, d = 0.f;
    if ((D & 3) == 0) {
        for (int64_t c = 4 * lane; c < D; c += 256) {
            const float4 x = *reinterpret_cast<const float4*>(xl + i * D + c);
            const float4 u = *reinterpret_cast<const float4*>(att_s + c);
            const float4 v = *reinterpret_cast<const float4*>(att_d + c);
            s = fmaf(x.x, u.x, fmaf(x.y, u.y, fmaf(x.z, u.z, fmaf(x.w, u.w, s))));
            d = fmaf(x.x, v.x, fmaf(x.y, v.y, fmaf(x.z, v.z, fmaf(x.w, v.w, d))));
        }
    } else {
        for (int64_t c = lane; c < D; c += 64) {
            const float x = xl[i * D + c];
            s = fmaf(x, att_s[c], s);
            d = fmaf(x, att_d[c], d);
        }
    }
    s = wave_sum_all(s);
    d = wave_sum_all(d);
    if (lane == 0) { a_s[i] = s; a_d[i] = d; }
}

// backward: dxl[i, :] (+)= g_s[i] att_s + g_d[i] att_d  (ACC: added to an existing gradient);  per-workgroup partial sums of
// d att_s = sum_i g_s[i] x'[i, :], d att_d likewise (part [gridDim.x][2][D]; a second tiny launch adds them in order)
template <bool ACC>
__global__ void __launch_bounds__(kT) gat_scores_bwd(const float* __restrict__ xl, int64_t N, int64_t D, const float* __restrict__ att_s,
                                                    const float* __restrict__ att_d, const float* __restrict__ g_s, const float* __restrict__ g_d,
                                                    float* __restrict__ dxl, float* __restrict__ part, int rows_per_wg) {
    // thread t owns column t (D <= 256 per pass); a workgroup walks rows_per_wg rows
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_wg;
    const int64_t r1 = r0 + rows_per_wg < N ? r0 + rows_per_wg : N;
    for (int64_t cb = 0; cb < D; cb += kT) {
        const int64_t c = cb + threadIdx.x;
        const bool in = c < D;
        const float us = in ? att_s[c] : 0.f, ud = in ? att_d[c] : 0.f;
        float ps = 0.f, pd = 0.f;
        for (int64_t i = r0; i < r1; ++i) {
            const float gs = g_s[i], gd = g_d[i];
            if (in) {
                const float x = xl[i * D + c];
                ps = fmaf(gs, x, ps);
                pd = fmaf(gd, x, pd);
                const float v = fmaf(gs, us, gd * ud);
                dxl[i * D + c] = ACC ? dxl[i * D + c] + v : v;
            }
        }
        if (in) {
            part[(static_cast<int64_t>(blockIdx.x) * 2) * D + c] = ps;
            part[(static_cast<int64_t>(blockIdx.x) * 2 + 1) * D + c] = pd;
        }
    }
}

// d att = sum over the workgroups' partial rows, fixed order: 64 columns x 16 row groups per workgroup (row group g takes partials g, g + 16,
// ... with four independent running sums; the groups are then added in order).  One thread per column walking all `nwg` rows was a chain of
// 530 dependent loads at arxiv-year's size: 89 us for 1 MB.
__global__ void __launch_bounds__(1024) gat_scores_bwd_finish(const float* __restrict__ part, int nwg, int64_t D, float* __restrict__ datt_s,
                                                             float* __restrict__ datt_d) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * 64 + lane;             // column of the concatenated [2 D] vector
    const bool ok = c < 2 * D;
    const int which = c >= D ? 1 : 0;
    const int64_t cc = which ? c - D : c;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (ok) {
        const float* col = part + static_cast<int64_t>(which) * D + cc;
        int w = g;
        for (; w + 48 < nwg; w += 64) {
            a0 += col[static_cast<int64_t>(w) * 2 * D];
            a1 += col[static_cast<int64_t>(w + 16) * 2 * D];
            a2 += col[static_cast<int64_t>(w + 32) * 2 * D];
            a3 += col[static_cast<int64_t>(w + 48) * 2 * D];
        }
        for (; w < nwg; w += 16) a0 += col[static_cast<int64_t>(w) * 2 * D];
    }
    red[g][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (g == 0 && ok) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc += red[k][lane];
        (which ? datt_d : datt_s)[cc] = acc;
    }
}


// =====================================================================================================================
// Multi-head GATConv (1 <= K <= 16 heads of C channels; x' is [N, K C] with head-major columns).  heads = 1 keeps the kernels above.
//
// Per-edge arrays are EDGE-MAJOR and indexed by EDGE ID: v[eid * K + h] (a row's K weights are contiguous: 32 B at K = 8), per-node
// arrays are [N, K].  Keeping them by edge id means the forward aggregation (dst-CSR), the transposed one (src-CSR) and the softmax
// backward all address the same array through their CSR's eid column, so the one-head path's scatter / gather re-orderings between
// entry orders do not exist here.
//
// Lane layout of the per-row kernels (softmax forward / backward, by-source sum): one wave per row, KP = K rounded up to a power of
// two, lane = sub * KP + h: 64 / KP entries of the row per step, each entry's CSR indices loaded once (one address for the KP lanes
// of an entry: a broadcast) and its K values by K adjacent lanes.  Reductions over a head are xor-shuffles over the lane bits above
// KP, a fixed tree: no float atomics anywhere, results are run-to-run identical.  Lanes with h >= K (K not a power of two) read
// head 0 and store nothing.
constexpr int kMaxHeads = 16;

template <int KP>
__device__ __forceinline__ float head_sum_all(float v) {
#pragma unroll
    for (int o = 32; o >= KP; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int KP>
__device__ __forceinline__ float head_max_all(float v) {
#pragma unroll
    for (int o = 32; o >= KP; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// soft / alpha [n, K] by edge id (0 for (i, i) entries), soft_loop / alpha_loop [N, K].  Attention dropout is keyed (site, row = edge id,
// col = head) and (site + 1, row = node, col = head): sgs_dropout_keep(seed, site, E, K, p) is the mask used, column 0 at K = 1 the
// one-head kernel's.
// The *_body function below is the only copy of the row code: the single-draw kernel after it (SOFT = true) and the multi-draw kernel
// (SOFT = false) are its two callers, and the other *_body functions of this file follow the same rule.  Each caller gets an
// instantiation of its own (SOFT here, SINGLE on the SpMM bodies, which have no option to tell the two apart): the multi-draw kernels pass
// constants for the dropout arguments, the compiler folds the constants of an internal function's only caller into it before it inlines,
// and an instantiation shared with a caller that passes variables loses that and came out with another register allocation in the
// multi-draw kernels.  With one instantiation per caller their ISA is the one they had when they were the bodies' only users
// ("The bodies").
template <int KP, bool SOFT>
__device__ __forceinline__ void gat_alpha_heads_fwd_body(int64_t i, int lane, const float* __restrict__ a_s, const float* __restrict__ a_d, int K,
                                                         const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                         const int* __restrict__ in_eid, float slope, float drop_scale, uint32_t drop_thresh,
                                                         int use_drop, uint64_t seed, uint32_t site, float* __restrict__ soft,
                                                         float* __restrict__ soft_loop, float* __restrict__ alpha, float* __restrict__ alpha_loop) {
    constexpr int EPW = 64 / KP;
    const int h = lane & (KP - 1), sub = lane / KP;
    const bool hv = h < K;
    const int hc = hv ? h : 0;
    const int b = in_ptr[i], e = in_ptr[i + 1];
    const float ad = a_d[i * K + hc];
    const float eloop = lrelu(a_s[i * K + hc] + ad, slope);
    float mx = eloop;
    for (int k = b + sub; k < e; k += EPW) {
        const int s = in_src[k];
        if (s != static_cast<int>(i)) mx = fmaxf(mx, lrelu(a_s[static_cast<int64_t>(s) * K + hc] + ad, slope));
    }
    mx = head_max_all<KP>(mx);
    float sum = 0.f;
    for (int k = b + sub; k < e; k += EPW) {
        const int s = in_src[k];
        if (s != static_cast<int>(i)) sum += expf(lrelu(a_s[static_cast<int64_t>(s) * K + hc] + ad, slope) - mx);
    }
    sum = head_sum_all<KP>(sum) + expf(eloop - mx);
    const float inv = 1.0f / (sum + 1e-16f);                  // torch_geometric.utils.softmax: / (sum + 1e-16)
    for (int k = b + sub; k < e; k += EPW) {
        const int s = in_src[k];
        const int64_t ed = in_eid[k];
        float sm = 0.f, al = 0.f;
        if (s != static_cast<int>(i)) {
            sm = expf(lrelu(a_s[static_cast<int64_t>(s) * K + hc] + ad, slope) - mx) * inv;
            al = sm;
            if (use_drop) al = dropout_keep_at(seed, site, static_cast<uint64_t>(ed), static_cast<uint32_t>(hc), drop_thresh) ? sm * drop_scale : 0.f;
        }
        if (hv) {
            if (SOFT) soft[ed * K + h] = sm;
            alpha[ed * K + h] = al;
        }
    }
    if (sub == 0 && hv) {
        const float sm = expf(eloop - mx) * inv;
        float al = sm;
        if (use_drop) al = dropout_keep_at(seed, site + 1u, static_cast<uint64_t>(i), static_cast<uint32_t>(h), drop_thresh) ? sm * drop_scale : 0.f;
        if (SOFT) soft_loop[i * K + h] = sm;
        alpha_loop[i * K + h] = al;
    }
}


template <int KP>
__global__ void __launch_bounds__(kT) gat_alpha_heads_fwd(const float* __restrict__ a_s, const float* __restrict__ a_d, int64_t N, int K,
                                                         const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                         const int* __restrict__ in_eid, float slope, float drop_scale, uint32_t drop_thresh,
                                                         int use_drop, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                         float* __restrict__ soft, float* __restrict__ soft_loop, float* __restrict__ alpha,
                                                         float* __restrict__ alpha_loop) {
    seed = fold_epoch(seed, epoch);
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;                                       // wave-uniform
    gat_alpha_heads_fwd_body<KP, true>(i, lane, a_s, a_d, K, in_ptr, in_src, in_eid, slope, drop_scale, drop_thresh, use_drop, seed, site, soft,
                                       soft_loop, alpha, alpha_loop);
}

// D drawn graphs of one partition (ensemble evaluation: no attention dropout, no kept softmax): blockIdx.y = draw d, which reads the node
// scores at a_s + d * as, a_d + d * as (as = 0: one [N, K] pair shared by every draw) and its CSR slices ptr [N+1], src / eid [nnz]; the
// body above runs unchanged on them, so row d of alpha [D, nnz, K] (by the draw's edge id) / alpha_loop [D, N, K] is bitwise what
// gat_alpha_heads_fwd (p = 0) writes for draw d alone.
template <int KP>
__global__ void __launch_bounds__(kT) gat_alpha_heads_fwd_multi(const float* __restrict__ a_s, const float* __restrict__ a_d, int64_t as, int64_t N,
                                                               int K, int64_t nnz, const int* __restrict__ in_ptr,
                                                               const int* __restrict__ in_src, const int* __restrict__ in_eid, float slope,
                                                               float* __restrict__ alpha, float* __restrict__ alpha_loop) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    const int64_t d = blockIdx.y;
    gat_alpha_heads_fwd_body<KP, false>(i, lane, a_s + d * as, a_d + d * as, K, in_ptr + d * (N + 1), in_src + d * nnz, in_eid + d * nnz, slope,
                                        1.0f, 0u, 0, uint64_t(0), 0u, nullptr, nullptr, alpha + d * nnz * K, alpha_loop + d * N * K);
}

// Backward of dropout + softmax + leaky_relu per (destination row, head); the formulas of gat_alpha_bwd above with galpha / soft / ge [n, K]
// by edge id and gloop / soft_loop / gsl / d_ad [N, K].
template <int KP>
__global__ void __launch_bounds__(kT) gat_alpha_heads_bwd(const float* __restrict__ a_s, const float* __restrict__ a_d, int64_t N, int K,
                                                         const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                         const int* __restrict__ in_eid, float slope, float drop_scale, uint32_t drop_thresh,
                                                         int use_drop, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                         const float* __restrict__ soft, const float* __restrict__ soft_loop,
                                                         const float* __restrict__ galpha, const float* __restrict__ gloop,
                                                         float* __restrict__ ge, float* __restrict__ gsl, float* __restrict__ d_ad) {
    constexpr int EPW = 64 / KP;
    seed = fold_epoch(seed, epoch);
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    const int h = lane & (KP - 1), sub = lane / KP;
    const bool hv = h < K;
    const int hc = hv ? h : 0;
    const int b = in_ptr[i], e = in_ptr[i + 1];
    const float ad = a_d[i * K + hc];
    auto dsm_edge = [&](int64_t ed) {
        float g = galpha[ed * K + hc];
        if (use_drop) g = dropout_keep_at(seed, site, static_cast<uint64_t>(ed), static_cast<uint32_t>(hc), drop_thresh) ? g * drop_scale : 0.f;
        return g;
    };
    float gl = gloop[i * K + hc];
    if (use_drop) gl = dropout_keep_at(seed, site + 1u, static_cast<uint64_t>(i), static_cast<uint32_t>(hc), drop_thresh) ? gl * drop_scale : 0.f;
    const float sl = soft_loop[i * K + hc];
    float dot = 0.f;
    for (int k = b + sub; k < e; k += EPW)
        if (in_src[k] != static_cast<int>(i)) {
            const int64_t ed = in_eid[k];
            dot += soft[ed * K + hc] * dsm_edge(ed);
        }
    dot = head_sum_all<KP>(dot) + sl * gl;
    float dad = 0.f;
    for (int k = b + sub; k < e; k += EPW) {
        const int s = in_src[k];
        const int64_t ed = in_eid[k];
        float dpre = 0.f;
        if (s != static_cast<int>(i)) {
            const float pre = a_s[static_cast<int64_t>(s) * K + hc] + ad;
            dpre = soft[ed * K + hc] * (dsm_edge(ed) - dot) * (pre > 0.f ? 1.f : slope);
        }
        if (hv) ge[ed * K + h] = dpre;
        dad += dpre;
    }
    dad = head_sum_all<KP>(dad);
    if (sub == 0 && hv) {
        const float pre = a_s[i * K + h] + ad;
        const float dl = sl * (gl - dot) * (pre > 0.f ? 1.f : slope);
        gsl[i * K + h] = dl;
        d_ad[i * K + h] = dad + dl;
    }
}

// ---- edge-weighted attention (GATConv edge_dim = 1 with the edge weight as the attribute): the logit of edge e = (s -> i), head h is
//   leaky_relu(a_s[s, h] + a_d[i, h] + w_e c_h),   c_h = <lin_edge.weight[h, :], att_edge[h, :]>  (host side, [K]),
// and the added loop of node i carries the mean weight of i's non-self in-edges (fill_value = 'mean'; 0 without any):
//   leaky_relu(a_s[i, h] + a_d[i, h] + wbar_i c_h).
// `w` is [n] by edge id.  The kernels are variants of gat_alpha_heads_fwd / _bwd of their own (the unweighted kernels' code is untouched);
// K = 1 runs their KP = 1 instantiation.  The first walk of the forward (the row maximum) also sums the row's weights, so wbar_i and
// 1 / cnt_i cost no launch; both are kept for the backward ([N] each).
__device__ __forceinline__ float edge_logit(float as, float ad, float w, float c, float slope) { return lrelu(fmaf(w, c, as + ad), slope); }

// SOFT = false (the multi-draw kernel): neither the kept softmax nor wbar / inv_cnt (the backward's inputs) are written.
template <int KP, bool SOFT>
__device__ __forceinline__ void gat_alpha_heads_edge_fwd_body(int64_t i, int lane, const float* __restrict__ a_s, const float* __restrict__ a_d,
                                                              const float* __restrict__ w, const float* __restrict__ coef, int K,
                                                              const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                              const int* __restrict__ in_eid, float slope, float drop_scale,
                                                              uint32_t drop_thresh, int use_drop, uint64_t seed, uint32_t site,
                                                              float* __restrict__ soft, float* __restrict__ soft_loop, float* __restrict__ alpha,
                                                              float* __restrict__ alpha_loop, float* __restrict__ wbar,
                                                              float* __restrict__ inv_cnt) {
    constexpr int EPW = 64 / KP;
    const int h = lane & (KP - 1), sub = lane / KP;
    const bool hv = h < K;
    const int hc = hv ? h : 0;
    const int b = in_ptr[i], e = in_ptr[i + 1];
    const float ad = a_d[i * K + hc];
    const float c = coef[hc];
    float mx = -INFINITY, wsum = 0.f, cnt = 0.f;
    for (int k = b + sub; k < e; k += EPW) {
        const int s = in_src[k];
        if (s != static_cast<int>(i)) {
            const float we = w[in_eid[k]];
            mx = fmaxf(mx, edge_logit(a_s[static_cast<int64_t>(s) * K + hc], ad, we, c, slope));
            wsum += we;
            cnt += 1.f;
        }
    }
    wsum = head_sum_all<KP>(wsum);                            // over the entries (the KP lanes of an entry hold the same weight)
    cnt = head_sum_all<KP>(cnt);
    const float icnt = cnt > 0.f ? 1.0f / cnt : 0.f;
    const float wb = wsum * icnt;
    const float eloop = edge_logit(a_s[i * K + hc], ad, wb, c, slope);
    mx = fmaxf(head_max_all<KP>(mx), eloop);
    float sum = 0.f;
    for (int k = b + sub; k < e; k += EPW) {
        const int s = in_src[k];
        if (s != static_cast<int>(i)) sum += expf(edge_logit(a_s[static_cast<int64_t>(s) * K + hc], ad, w[in_eid[k]], c, slope) - mx);
    }
    sum = head_sum_all<KP>(sum) + expf(eloop - mx);
    const float inv = 1.0f / (sum + 1e-16f);                  // torch_geometric.utils.softmax: / (sum + 1e-16)
    for (int k = b + sub; k < e; k += EPW) {
        const int s = in_src[k];
        const int64_t ed = in_eid[k];
        float sm = 0.f, al = 0.f;
        if (s != static_cast<int>(i)) {
            sm = expf(edge_logit(a_s[static_cast<int64_t>(s) * K + hc], ad, w[ed], c, slope) - mx) * inv;
            al = sm;
            if (use_drop) al = dropout_keep_at(seed, site, static_cast<uint64_t>(ed), static_cast<uint32_t>(hc), drop_thresh) ? sm * drop_scale : 0.f;
        }
        if (hv) {
            if (SOFT) soft[ed * K + h] = sm;
            alpha[ed * K + h] = al;
        }
    }
    if (sub == 0 && hv) {
        const float sm = expf(eloop - mx) * inv;
        float al = sm;
        if (use_drop) al = dropout_keep_at(seed, site + 1u, static_cast<uint64_t>(i), static_cast<uint32_t>(h), drop_thresh) ? sm * drop_scale : 0.f;
        if (SOFT) soft_loop[i * K + h] = sm;
        alpha_loop[i * K + h] = al;
    }
    if (SOFT && lane == 0) { wbar[i] = wb; inv_cnt[i] = icnt; }
}


template <int KP>
__global__ void __launch_bounds__(kT) gat_alpha_heads_edge_fwd(const float* __restrict__ a_s, const float* __restrict__ a_d,
                                                              const float* __restrict__ w, const float* __restrict__ coef, int64_t N, int K,
                                                              const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                              const int* __restrict__ in_eid, float slope, float drop_scale, uint32_t drop_thresh,
                                                              int use_drop, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                              float* __restrict__ soft, float* __restrict__ soft_loop, float* __restrict__ alpha,
                                                              float* __restrict__ alpha_loop, float* __restrict__ wbar, float* __restrict__ inv_cnt) {
    seed = fold_epoch(seed, epoch);
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;                                       // wave-uniform
    gat_alpha_heads_edge_fwd_body<KP, true>(i, lane, a_s, a_d, w, coef, K, in_ptr, in_src, in_eid, slope, drop_scale, drop_thresh, use_drop, seed,
                                            site, soft, soft_loop, alpha, alpha_loop, wbar, inv_cnt);
}

// The multi-draw form of the above (see gat_alpha_heads_fwd_multi): draw d's weights are w + d * nnz (by the draw's edge id), coef [K] is
// shared.  Row d is bitwise gat_alpha_heads_edge_fwd's (p = 0) alpha / alpha_loop for draw d alone.
template <int KP>
__global__ void __launch_bounds__(kT) gat_alpha_heads_edge_fwd_multi(const float* __restrict__ a_s, const float* __restrict__ a_d, int64_t as,
                                                                    const float* __restrict__ w, const float* __restrict__ coef, int64_t N, int K,
                                                                    int64_t nnz, const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                                    const int* __restrict__ in_eid, float slope, float* __restrict__ alpha,
                                                                    float* __restrict__ alpha_loop) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    const int64_t d = blockIdx.y;
    gat_alpha_heads_edge_fwd_body<KP, false>(i, lane, a_s + d * as, a_d + d * as, w + d * nnz, coef, K, in_ptr + d * (N + 1), in_src + d * nnz,
                                             in_eid + d * nnz, slope, 1.0f, 0u, 0, uint64_t(0), 0u, nullptr, nullptr, alpha + d * nnz * K,
                                             alpha_loop + d * N * K, nullptr, nullptr);
}

// gat_alpha_heads_bwd with the edge term: ge / gsl / d_ad as there, plus
//   dw[e]  = sum_h c_h (ge[e, h] + gsl[i, h] / cnt_i)  (+ dw_add[e])   for e into i, 0 for (i, i) entries -- the K lanes of an entry are
//            added by xor-shuffles below KP, one lane stores; `dw_add` [n] or NULL: the other layer's d w, summed on the way out;
//   dc[h]  = sum_e w_e ge[e, h] + sum_i wbar_i gsl[i, h]: the workgroup's rows are added in wave order into part[blockIdx.x, h]
//            ([gridDim.x, K]; gat_edge_dc_finish adds the workgroups in a fixed order).
// The second walk runs wave-uniform trips (every lane takes part in the shuffles of its entry).
template <int KP>
__global__ void __launch_bounds__(kT) gat_alpha_heads_edge_bwd(const float* __restrict__ a_s, const float* __restrict__ a_d,
                                                              const float* __restrict__ w, const float* __restrict__ coef,
                                                              const float* __restrict__ wbar, const float* __restrict__ inv_cnt, int64_t N, int K,
                                                              const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                              const int* __restrict__ in_eid, float slope, float drop_scale, uint32_t drop_thresh,
                                                              int use_drop, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                              const float* __restrict__ soft, const float* __restrict__ soft_loop,
                                                              const float* __restrict__ galpha, const float* __restrict__ gloop,
                                                              const float* __restrict__ dw_add, float* __restrict__ ge, float* __restrict__ gsl,
                                                              float* __restrict__ d_ad, float* __restrict__ dw, float* __restrict__ part) {
    constexpr int EPW = 64 / KP;
    __shared__ float red[kT / 64][kMaxHeads];
    seed = fold_epoch(seed, epoch);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    const int h = lane & (KP - 1), sub = lane / KP;
    const bool hv = h < K;
    const int hc = hv ? h : 0;
    float dc = 0.f;
    if (i < N) {                                              // wave-uniform; every wave reaches the barrier below
        const int b = in_ptr[i], e = in_ptr[i + 1];
        const float ad = a_d[i * K + hc];
        const float c = coef[hc];
        const float wb = wbar[i], icnt = inv_cnt[i];
        auto dsm_edge = [&](int64_t ed) {
            float g = galpha[ed * K + hc];
            if (use_drop) g = dropout_keep_at(seed, site, static_cast<uint64_t>(ed), static_cast<uint32_t>(hc), drop_thresh) ? g * drop_scale : 0.f;
            return g;
        };
        float gl = gloop[i * K + hc];
        if (use_drop) gl = dropout_keep_at(seed, site + 1u, static_cast<uint64_t>(i), static_cast<uint32_t>(hc), drop_thresh) ? gl * drop_scale : 0.f;
        const float sl = soft_loop[i * K + hc];
        float dot = 0.f;
        for (int k = b + sub; k < e; k += EPW)
            if (in_src[k] != static_cast<int>(i)) {
                const int64_t ed = in_eid[k];
                dot += soft[ed * K + hc] * dsm_edge(ed);
            }
        dot = head_sum_all<KP>(dot) + sl * gl;
        const float prel = fmaf(wb, c, a_s[i * K + hc] + ad);
        const float dl = sl * (gl - dot) * (prel > 0.f ? 1.f : slope);
        const float cm = hv ? c : 0.f;                        // lanes past K add nothing to an entry's d w
        const float loop_term = dl * icnt;
        float dad = 0.f;
        for (int k0 = b; k0 < e; k0 += EPW) {
            const int k = k0 + sub;
            const bool in = k < e;
            const int s = in ? in_src[k] : static_cast<int>(i);
            const int64_t ed = in ? in_eid[k] : 0;
            const bool edge = in && s != static_cast<int>(i);
            float dpre = 0.f, t = 0.f;
            if (edge) {
                const float we = w[ed];
                const float pre = fmaf(we, c, a_s[static_cast<int64_t>(s) * K + hc] + ad);
                dpre = soft[ed * K + hc] * (dsm_edge(ed) - dot) * (pre > 0.f ? 1.f : slope);
                dc = fmaf(we, dpre, dc);
                t = cm * (dpre + loop_term);
            }
            if (in && hv) ge[ed * K + h] = dpre;
            dad += dpre;
#pragma unroll
            for (int o = KP >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
            if (in && h == 0) dw[ed] = dw_add ? dw_add[ed] + t : t;
        }
        dad = head_sum_all<KP>(dad);
        dc = fmaf(wb, dl, head_sum_all<KP>(dc));
        if (sub == 0 && hv) {
            gsl[i * K + h] = dl;
            d_ad[i * K + h] = dad + dl;
        }
    }
    if (sub == 0 && hv) red[wave][h] = dc;
    __syncthreads();
    if (threadIdx.x < K) {
        float acc = 0.f;
#pragma unroll
        for (int v = 0; v < kT / 64; ++v) acc += red[v][threadIdx.x];
        part[static_cast<int64_t>(blockIdx.x) * K + threadIdx.x] = acc;
    }
}

// dc[h] = sum over the workgroups' partial rows part[nwg, K], fixed order: thread (g, h) adds rows g, g + 64, ... and the 64 groups are then
// added in order.
__global__ void __launch_bounds__(1024) gat_edge_dc_finish(const float* __restrict__ part, int nwg, int K, float* __restrict__ dc) {
    __shared__ float red[64][kMaxHeads];
    const int h = threadIdx.x & (kMaxHeads - 1), g = threadIdx.x >> 4;
    float acc = 0.f;
    if (h < K)
        for (int r = g; r < nwg; r += 64) acc += part[static_cast<int64_t>(r) * K + h];
    red[g][h] = acc;
    __syncthreads();
    if (threadIdx.x < K) {
        float s = 0.f;
        for (int v = 0; v < 64; ++v) s += red[v][threadIdx.x];
        dc[threadIdx.x] = s;
    }
}

// out[j, h] = sum over j's out-edges (src-CSR order) of ge[eid, h] + gsl[j, h]: d a_src of the layer (the one-head path runs an SpMM
// over a column of ones for this, after a gather into src-CSR order).
template <int KP>
__global__ void __launch_bounds__(kT) edge_sum_by_row_heads(const float* __restrict__ ge, const float* __restrict__ gsl, int64_t N, int K,
                                                           const int* __restrict__ ptr, const int* __restrict__ eid, float* __restrict__ out) {
    constexpr int EPW = 64 / KP;
    const int lane = threadIdx.x & 63;
    const int64_t j = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (j >= N) return;
    const int h = lane & (KP - 1), sub = lane / KP;
    const bool hv = h < K;
    const int hc = hv ? h : 0;
    const int b = ptr[j], e = ptr[j + 1];
    float acc = 0.f;
    for (int k = b + sub; k < e; k += EPW) acc += ge[static_cast<int64_t>(eid[k]) * K + hc];
    acc = head_sum_all<KP>(acc);
    if (sub == 0 && hv) out[j * K + h] = acc + (gsl ? gsl[j * K + h] : 0.f);
}

// Node scores for K heads in one pass over x': x' viewed as [N K, C] (head-major columns make a (node, head) slice contiguous), unit
// u = i K + h owned by G = 2^lg lanes (VEC floats per lane and step): a_s[u] = <x'[u, :], att_s[h, :]>, a_d likewise.
template <int VEC>
__global__ void __launch_bounds__(kT) gat_scores_heads_fwd(const float* __restrict__ xl, int64_t NU, int K, int64_t C,
                                                          const float* __restrict__ att_s, const float* __restrict__ att_d,
                                                          float* __restrict__ a_s, float* __restrict__ a_d, int lg) {
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    const int G = 1 << lg;
    const int64_t u = t >> lg;
    const int g = static_cast<int>(t & (G - 1));
    const bool live = u < NU;                                 // every lane stays for the shuffles
    float s = 0.f, d = 0.f;
    if (live) {
        const int h = static_cast<int>(u % K);
        const float* x = xl + u * C;
        const float* us = att_s + h * C;
        const float* ud = att_d + h * C;
        for (int64_t c = static_cast<int64_t>(g) * VEC; c < C; c += static_cast<int64_t>(G) * VEC) {
            float xv[VEC], sv[VEC], dv[VEC];
            *reinterpret_cast<V*>(xv) = *reinterpret_cast<const V*>(x + c);
            *reinterpret_cast<V*>(sv) = *reinterpret_cast<const V*>(us + c);
            *reinterpret_cast<V*>(dv) = *reinterpret_cast<const V*>(ud + c);
#pragma unroll
            for (int v = 0; v < VEC; ++v) { s = fmaf(xv[v], sv[v], s); d = fmaf(xv[v], dv[v], d); }
        }
    }
    for (int o = G >> 1; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); d += __shfl_xor(d, o, 64); }
    if (live && g == 0) { a_s[u] = s; a_d[u] = d; }
}

// backward of the above, gat_scores_bwd's scheme over D = K C columns: thread owns column j = h C + c, dxl[i, j] (+)= g_s[i, h] att_s[j] +
// g_d[i, h] att_d[j]; per-workgroup partials of d att (flat [K C]) finished by gat_scores_bwd_finish in a fixed order.
template <bool ACC>
__global__ void __launch_bounds__(kT) gat_scores_heads_bwd(const float* __restrict__ xl, int64_t N, int K, int64_t C,
                                                          const float* __restrict__ att_s, const float* __restrict__ att_d,
                                                          const float* __restrict__ g_s, const float* __restrict__ g_d, float* __restrict__ dxl,
                                                          float* __restrict__ part, int rows_per_wg) {
    const int64_t D = static_cast<int64_t>(K) * C;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_wg;
    const int64_t r1 = r0 + rows_per_wg < N ? r0 + rows_per_wg : N;
    for (int64_t cb = 0; cb < D; cb += kT) {
        const int64_t c = cb + threadIdx.x;
        const bool in = c < D;
        const int h = in ? static_cast<int>(c / C) : 0;
        const float us = in ? att_s[c] : 0.f, ud = in ? att_d[c] : 0.f;
        float ps = 0.f, pd = 0.f;
        if (in) {
            for (int64_t i = r0; i < r1; ++i) {
                const float gs = g_s[i * K + h], gd = g_d[i * K + h];
                const float x = xl[i * D + c];
                ps = fmaf(gs, x, ps);
                pd = fmaf(gd, x, pd);
                const float v = fmaf(gs, us, gd * ud);
                dxl[i * D + c] = ACC ? dxl[i * D + c] + v : v;
            }
            part[(static_cast<int64_t>(blockIdx.x) * 2) * D + c] = ps;
            part[(static_cast<int64_t>(blockIdx.x) * 2 + 1) * D + c] = pd;
        }
    }
}

// acc[0 .. VEC) = sum_k val[eid_k, h] X[col_k, xc ..] + diag[i, h] X[i, xc ..] over row i = [b, e) of the CSR, entries in order
template <int VEC>
__device__ __forceinline__ void spmm_heads_acc(const float* __restrict__ X, int64_t XD, int64_t xc, int K, int h, int64_t i, int b, int e,
                                               const int* __restrict__ col, const int* __restrict__ eid, const float* __restrict__ val,
                                               const float* __restrict__ diag, float (&acc)[VEC]) {
    using V = typename std::conditional<VEC == 4, float4, float>::type;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    int k = b;
    for (; k + 4 <= e; k += 4) {          // 4 independent row gathers in flight
        int j[4]; float w[4]; float x[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) { j[u] = col[k + u]; w[u] = val[static_cast<int64_t>(eid[k + u]) * K + h]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) *reinterpret_cast<V*>(x[u]) = *reinterpret_cast<const V*>(X + static_cast<int64_t>(j[u]) * XD + xc);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
    }
    for (; k < e; ++k) {
        float x[VEC];
        *reinterpret_cast<V*>(x) = *reinterpret_cast<const V*>(X + static_cast<int64_t>(col[k]) * XD + xc);
        const float w = val[static_cast<int64_t>(eid[k]) * K + h];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[v], acc[v]);
    }
    if (diag) {
        float x[VEC];
        *reinterpret_cast<V*>(x) = *reinterpret_cast<const V*>(X + i * XD + xc);
        const float w = diag[i * K + h];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[v], acc[v]);
    }
}

// Per-head CSR SpMM, output [N, K C]:  Y[i, h C + c] = sum_k val[eid_k, h] X[col_k, h C + c] + diag[i, h] X[i, h C + c], then the bias / ReLU /
// dropout epilogue of spmm_csr.  LPR = 2^lg lanes own a row, VEC consecutive columns each (VEC = 4 only when C % 4 == 0, so a lane's
// columns belong to one head; with VEC = 1 any C is correct): at K C = 256 a wave gathers the same 1 KB row as the one-head layer and
// the K weights of an entry arrive as one 4 K-byte read.  BCAST (backward of the head mean): X is [N, C], shared by the heads, and the
// result is scaled by 1 / K:  Y[i, h C + c] = (1 / K) (sum_k val[eid_k, h] X[col_k, c] + diag[i, h] X[i, c]).
// SINGLE (here and on the two head-mean bodies) selects no code: it is true from the single-draw kernel and gives each caller its own
// instantiation (see the note at gat_alpha_heads_fwd_body).
template <int VEC, bool BCAST, bool SINGLE = false>
__device__ __forceinline__ void spmm_csr_heads_body(const float* __restrict__ X, int64_t N, int K, int64_t C, const int* __restrict__ ptr,
                                                    const int* __restrict__ col, const int* __restrict__ eid, const float* __restrict__ val,
                                                    const float* __restrict__ diag, const float* __restrict__ bias, int act, float drop_scale,
                                                    uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                                    float* __restrict__ Y, int lg) {
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const int LPR = 1 << lg;
    const int sub = threadIdx.x & (LPR - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kT >> lg) + (threadIdx.x >> lg);
    if (i >= N) return;
    const int64_t D = static_cast<int64_t>(K) * C;
    const int64_t XD = BCAST ? C : D;
    const float post = BCAST ? 1.0f / static_cast<float>(K) : 1.0f;
    const int b = ptr[i], e = ptr[i + 1];
    for (int64_t c0 = static_cast<int64_t>(sub) * VEC; c0 < D; c0 += static_cast<int64_t>(LPR) * VEC) {
        const int h = static_cast<int>(c0 / C);
        const int64_t xc = BCAST ? c0 - h * C : c0;
        float acc[VEC];
        spmm_heads_acc<VEC>(X, XD, xc, K, h, i, b, e, col, eid, val, diag, acc);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float y = BCAST ? acc[v] * post : acc[v];
            if (bias) y += bias[c0 + v];
            if (act != SGS_ACT_NONE) y = fmaxf(y, 0.f);
            if (act == SGS_ACT_RELU_DROPOUT)
                y = dropout_keep_at(seed, site, static_cast<uint64_t>(i), static_cast<uint32_t>(c0 + v), drop_thresh) ? y * drop_scale : 0.f;
            acc[v] = y;
        }
        *reinterpret_cast<V*>(Y + i * D + c0) = *reinterpret_cast<V*>(acc);
    }
}
template <int VEC, bool BCAST>
__global__ void __launch_bounds__(kT) spmm_csr_heads(const float* __restrict__ X, int64_t N, int K, int64_t C, const int* __restrict__ ptr,
                                                    const int* __restrict__ col, const int* __restrict__ eid, const float* __restrict__ val,
                                                    const float* __restrict__ diag, const float* __restrict__ bias, int act, float drop_scale,
                                                    uint32_t drop_thresh, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                    float* __restrict__ Y, int lg) {
    seed = fold_epoch(seed, epoch);
    spmm_csr_heads_body<VEC, BCAST, true>(X, N, K, C, ptr, col, eid, val, diag, bias, act, drop_scale, drop_thresh, seed, site, Y, lg);
}

// The head-mean form (GATConv concat = False), fused: Y[i, c] = (1 / K) sum_h (sum_k val[eid_k, h] X[col_k, h C + c] + diag[i, h] X[i, h C + c])
// + bias[c].  A lane owns VEC output columns and walks the K heads of each gathered row itself (heads in order 0 .. K - 1 per entry, entries
// in CSR order), so the [N, K C] per-head result is never written and no second launch averages it.
template <int VEC, bool SINGLE = false>
__device__ __forceinline__ void spmm_csr_heads_mean_body(const float* __restrict__ X, int64_t N, int K, int64_t C, const int* __restrict__ ptr,
                                                         const int* __restrict__ col, const int* __restrict__ eid, const float* __restrict__ val,
                                                         const float* __restrict__ diag, const float* __restrict__ bias, int act, float drop_scale,
                                                         uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                                         float* __restrict__ Y, int lg) {
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const int LPR = 1 << lg;
    const int sub = threadIdx.x & (LPR - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kT >> lg) + (threadIdx.x >> lg);
    if (i >= N) return;
    const int64_t D = static_cast<int64_t>(K) * C;
    const float invK = 1.0f / static_cast<float>(K);
    const int b = ptr[i], e = ptr[i + 1];
    for (int64_t c0 = static_cast<int64_t>(sub) * VEC; c0 < C; c0 += static_cast<int64_t>(LPR) * VEC) {
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int k = b; k <= e; ++k) {                        // k == e: the loop term
            const bool loop = k == e;
            if (loop && !diag) break;
            const float* xr = X + (loop ? i : static_cast<int64_t>(col[k])) * D + c0;
            const float* wr = loop ? diag + i * K : val + static_cast<int64_t>(eid[k]) * K;
            for (int h = 0; h < K; ++h) {
                float x[VEC];
                *reinterpret_cast<V*>(x) = *reinterpret_cast<const V*>(xr + h * C);
                const float w = wr[h];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[v], acc[v]);
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float y = acc[v] * invK;
            if (bias) y += bias[c0 + v];
            if (act != SGS_ACT_NONE) y = fmaxf(y, 0.f);
            if (act == SGS_ACT_RELU_DROPOUT)
                y = dropout_keep_at(seed, site, static_cast<uint64_t>(i), static_cast<uint32_t>(c0 + v), drop_thresh) ? y * drop_scale : 0.f;
            acc[v] = y;
        }
        *reinterpret_cast<V*>(Y + i * C + c0) = *reinterpret_cast<V*>(acc);
    }
}
template <int VEC>
__global__ void __launch_bounds__(kT) spmm_csr_heads_mean(const float* __restrict__ X, int64_t N, int K, int64_t C, const int* __restrict__ ptr,
                                                         const int* __restrict__ col, const int* __restrict__ eid, const float* __restrict__ val,
                                                         const float* __restrict__ diag, const float* __restrict__ bias, int act, float drop_scale,
                                                         uint32_t drop_thresh, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                         float* __restrict__ Y, int lg) {
    seed = fold_epoch(seed, epoch);
    spmm_csr_heads_mean_body<VEC, true>(X, N, K, C, ptr, col, eid, val, diag, bias, act, drop_scale, drop_thresh, seed, site, Y, lg);
}

// The same head mean with the concat kernel's lane layout (a lane owns VEC columns of the [K C] per-head row, so a wave gathers whole rows and
// long rows are walked with four gathers in flight): the per-head sums go to LDS ([rows of the workgroup][K C] floats, at most 16 KB) and
// lanes c < C add the K heads of column c in order 0 .. K - 1.  Used when K C rows fit (kMeanLdsFloats); the kernel above walks the heads in
// each lane with C / VEC lanes per row and was 6x slower at K = 8, C = 5 on a power-law graph, where 8 lanes served a hub row alone.
constexpr int kMeanLdsFloats = 4096;
template <int VEC, bool SINGLE = false>
__device__ __forceinline__ void spmm_csr_heads_mean_lds_body(const float* __restrict__ X, int64_t N, int K, int64_t C, const int* __restrict__ ptr,
                                                             const int* __restrict__ col, const int* __restrict__ eid, const float* __restrict__ val,
                                                             const float* __restrict__ diag, const float* __restrict__ bias, int act, float drop_scale,
                                                             uint32_t drop_thresh, uint64_t seed, uint32_t site,
                                                             float* __restrict__ Y, int lg, float* __restrict__ part) {
    const int LPR = 1 << lg;
    const int sub = threadIdx.x & (LPR - 1), r = threadIdx.x >> lg;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kT >> lg) + r;
    const bool live = i < N;                                  // every thread reaches the barrier
    const int64_t D = static_cast<int64_t>(K) * C;
    float* mine = part + r * D;
    if (live) {
        const int b = ptr[i], e = ptr[i + 1];
        for (int64_t c0 = static_cast<int64_t>(sub) * VEC; c0 < D; c0 += static_cast<int64_t>(LPR) * VEC) {
            const int h = static_cast<int>(c0 / C);
            float acc[VEC];
            spmm_heads_acc<VEC>(X, D, c0, K, h, i, b, e, col, eid, val, diag, acc);
#pragma unroll
            for (int v = 0; v < VEC; ++v) mine[c0 + v] = acc[v];
        }
    }
    __syncthreads();
    if (!live) return;
    const float invK = 1.0f / static_cast<float>(K);
    for (int64_t c = sub; c < C; c += LPR) {
        float y = 0.f;
        for (int h = 0; h < K; ++h) y += mine[h * C + c];
        y *= invK;
        if (bias) y += bias[c];
        if (act != SGS_ACT_NONE) y = fmaxf(y, 0.f);
        if (act == SGS_ACT_RELU_DROPOUT)
            y = dropout_keep_at(seed, site, static_cast<uint64_t>(i), static_cast<uint32_t>(c), drop_thresh) ? y * drop_scale : 0.f;
        Y[i * C + c] = y;
    }
}
template <int VEC>
__global__ void __launch_bounds__(kT) spmm_csr_heads_mean_lds(const float* __restrict__ X, int64_t N, int K, int64_t C, const int* __restrict__ ptr,
                                                             const int* __restrict__ col, const int* __restrict__ eid, const float* __restrict__ val,
                                                             const float* __restrict__ diag, const float* __restrict__ bias, int act, float drop_scale,
                                                             uint32_t drop_thresh, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                             float* __restrict__ Y, int lg) {
    __shared__ float part[kMeanLdsFloats];
    seed = fold_epoch(seed, epoch);
    spmm_csr_heads_mean_lds_body<VEC, true>(X, N, K, C, ptr, col, eid, val, diag, bias, act, drop_scale, drop_thresh, seed, site, Y, lg, part);
}

// D drawn graphs of one partition (ensemble evaluation: ReLU / bias only, no dropout): blockIdx.y = draw d, which reads X + d * xs (xs = 0:
// one X shared by every draw), its CSR slices ptr [N+1], col / eid [nnz], its weights val [nnz, K] / diag [N, K] and writes its block of
// Y [D, N, W] (W = K C, or C for the head mean).  The bodies above run unchanged, so block d is bitwise sgs_spmm_csr_heads' for draw d.
// MODE: 0 concat, 1 the LDS head mean, 2 the head mean with lanes owning output columns (rows of more than 1024 floats).
template <int VEC, int MODE>
__global__ void __launch_bounds__(kT) spmm_csr_heads_multi(const float* __restrict__ X, int64_t xs, int64_t N, int K, int64_t C, int64_t nnz,
                                                          const int* __restrict__ ptr, const int* __restrict__ col, const int* __restrict__ eid,
                                                          const float* __restrict__ val, const float* __restrict__ diag,
                                                          const float* __restrict__ bias, int act, float* __restrict__ Y, int lg) {
    const int64_t d = blockIdx.y;
    const int64_t W = MODE == 0 ? static_cast<int64_t>(K) * C : C;
    X += d * xs; ptr += d * (N + 1); col += d * nnz; eid += d * nnz; val += d * nnz * K; Y += d * N * W;
    if (diag) diag += d * N * K;
    if constexpr (MODE == 0) {
        spmm_csr_heads_body<VEC, false>(X, N, K, C, ptr, col, eid, val, diag, bias, act, 1.0f, 0u, uint64_t(0), 0u, Y, lg);
    } else if constexpr (MODE == 1) {
        __shared__ float part[kMeanLdsFloats];
        spmm_csr_heads_mean_lds_body<VEC>(X, N, K, C, ptr, col, eid, val, diag, bias, act, 1.0f, 0u, uint64_t(0), 0u, Y, lg, part);
    } else {
        spmm_csr_heads_mean_body<VEC>(X, N, K, C, ptr, col, eid, val, diag, bias, act, 1.0f, 0u, uint64_t(0), 0u, Y, lg);
    }
}

// Per-head SDDMM over the CSR: g[eid_k, h] = <A[i, h, :], B[col_k, h, :]>, gdiag[i, h] = <A[i, h, :], B[i, h, :]>.  LPR = KP G lanes per row:
// lane (h, g) walks columns g VEC, (g + G) VEC, ... of head h's slice and the G lanes of a head are summed by xor-shuffles.  BCAST: A is
// [N, C], shared by the heads, and the products are scaled by 1 / K (the head mean's backward).
template <int VEC, bool BCAST>
__global__ void __launch_bounds__(kT) sddmm_csr_heads(const float* __restrict__ A, const float* __restrict__ B, int64_t N, int K, int64_t C,
                                                     const int* __restrict__ ptr, const int* __restrict__ col, const int* __restrict__ eid,
                                                     float* __restrict__ g, float* __restrict__ gdiag, int lg, int lgG) {
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const int LPR = 1 << lg, G = 1 << lgG;
    const int sub = threadIdx.x & (LPR - 1);
    const int h = sub >> lgG, gl = sub & (G - 1);
    const bool hv = h < K;
    const int hc = hv ? h : 0;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kT >> lg) + (threadIdx.x >> lg);
    const bool live = i < N;            // keep every lane in the shuffles
    const int64_t D = static_cast<int64_t>(K) * C;
    const float post = BCAST ? 1.0f / static_cast<float>(K) : 1.0f;
    const int b = live ? ptr[i] : 0, e = live ? ptr[i + 1] : 0;
    const float* Ai = A + (live ? i : 0) * (BCAST ? C : D) + (BCAST ? 0 : hc * C);
    int trips = e - b + 1;             // +1: the loop term; made wave-uniform, dead lanes contribute 0
    for (int o = 32; o > 0; o >>= 1) trips = max(trips, __shfl_xor(trips, o, 64));
    for (int t = 0; t < trips; ++t) {
        const int k = b + t;
        const bool is_edge = live && k < e;
        const bool is_diag = live && k == e;
        const int64_t j = is_edge ? col[k] : i;
        float acc = 0.f;
        if (is_edge || is_diag) {
            const float* Bj = B + j * D + hc * C;
            for (int64_t c0 = static_cast<int64_t>(gl) * VEC; c0 < C; c0 += static_cast<int64_t>(G) * VEC) {
                float a[VEC], x[VEC];
                *reinterpret_cast<V*>(a) = *reinterpret_cast<const V*>(Ai + c0);
                *reinterpret_cast<V*>(x) = *reinterpret_cast<const V*>(Bj + c0);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc = fmaf(a[v], x[v], acc);
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (gl == 0 && hv) {
            if (is_edge) g[static_cast<int64_t>(eid[k]) * K + h] = acc * post;
            else if (is_diag) gdiag[i * K + h] = acc * post;
        }
    }
}

inline int log2_ceil(int64_t v) {
    int l = 0;
    while ((int64_t(1) << l) < v) ++l;
    return l;
}
inline bool heads_ok(int64_t K, int64_t C) { return K >= 1 && K <= kMaxHeads && C >= 1 && C <= (int64_t(1) << 24); }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// KP = K rounded up to a power of two selects the per-row kernels' instantiation
#define SGS_DISPATCH_KPV(KERNEL, KP, GRID, STREAM, ...)                                                                 \
    do {                                                                                                                \
        switch (KP) {                                                                                                   \
            case 1: hipLaunchKernelGGL((KERNEL<1>), GRID, dim3(kT), 0, STREAM, __VA_ARGS__); break;                     \
            case 2: hipLaunchKernelGGL((KERNEL<2>), GRID, dim3(kT), 0, STREAM, __VA_ARGS__); break;                     \
            case 4: hipLaunchKernelGGL((KERNEL<4>), GRID, dim3(kT), 0, STREAM, __VA_ARGS__); break;                     \
            case 8: hipLaunchKernelGGL((KERNEL<8>), GRID, dim3(kT), 0, STREAM, __VA_ARGS__); break;                     \
            default: hipLaunchKernelGGL((KERNEL<16>), GRID, dim3(kT), 0, STREAM, __VA_ARGS__); break;                   \
        }                                                                                                               \
    } while (0)
#define SGS_DISPATCH_KP(KERNEL, K, GRID, STREAM, ...) SGS_DISPATCH_KPV(KERNEL, 1 << log2_ceil(K), GRID, STREAM, __VA_ARGS__)

// The launch choice of every multi-head entry point (sgs_gat_heads_variant's code, see include/sgs_hip.h), taken apart again
struct HeadsChoice {
    int kind, vec, lg, lgG, w;
    explicit HeadsChoice(int code)
        : kind(code / 1000000), vec(code / 100000 % 10), lg(code / 10000 % 10), lgG(code / 1000 % 10), w(code % 1000) {}
};
inline int heads_code(int kind, int vec, int lg, int lgG, int w) { return kind * 1000000 + vec * 100000 + lg * 10000 + lgG * 1000 + w; }
inline int min6(int lg) { return lg > 6 ? 6 : lg; }
inline int heads_kp(int64_t N, int64_t K) { return HeadsChoice(sgs_gat_heads_variant(SGS_GAT_OP_ROW, N, K, 1, 0)).w; }   // the per-row family's KP

}  // namespace
}  // namespace sgs

using namespace sgs;

extern "C" {

int sgs_gat_alpha_fwd(const float* a_src, const float* a_dst, int64_t N, int64_t n_edges, const int32_t* in_ptr,
                      const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed,
                      uint32_t site, float* soft_in, float* soft_loop, float* alpha_in, float* alpha_loop,
                      sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0 && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL, "sgs_gat_alpha_fwd: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(a_src && a_dst && in_ptr && soft_loop && alpha_loop && (n_edges == 0 || (in_src && in_eid && soft_in && alpha_in)),
                SGS_EINVAL, "sgs_gat_alpha_fwd: null pointer");
    hipLaunchKernelGGL(gat_alpha_fwd, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, a_src, a_dst, N, in_ptr, in_src, in_eid,
                       negative_slope, 1.0f / (1.0f - p_drop), dropout_thresh(p_drop), p_drop > 0.f ? 1 : 0, seed, site, epoch_ptr(), soft_in,
                       soft_loop, alpha_in, alpha_loop);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gat_alpha_fwd_multi(const float* a_src, const float* a_dst, int64_t a_stride, int64_t N, int64_t D, int64_t nnz,
                            const int32_t* in_ptr, const int32_t* in_src, float negative_slope, float* alpha_in, float* alpha_loop,
                            sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && nnz >= 0 && D >= 1 && D <= 65535 && (a_stride == 0 || a_stride >= N), SGS_EINVAL,
                "sgs_gat_alpha_fwd_multi: bad sizes (1 <= D <= 65535; a_stride 0 or >= N)");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(a_src && a_dst && in_ptr && alpha_loop && (nnz == 0 || (in_src && alpha_in)), SGS_EINVAL, "sgs_gat_alpha_fwd_multi: null pointer");
    hipLaunchKernelGGL(gat_alpha_fwd_multi, dim3(static_cast<unsigned>(cdiv(N * 64, kT)), static_cast<unsigned>(D)), dim3(kT), 0, stream, a_src, a_dst,
                       a_stride, N, nnz, in_ptr, in_src, negative_slope, alpha_in, alpha_loop);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gat_alpha_bwd(const float* a_src, const float* a_dst, int64_t N, int64_t n_edges, const int32_t* in_ptr,
                      const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed,
                      uint32_t site, const float* soft_in, const float* soft_loop, const float* galpha, const float* gloop,
                      float* g_edge, float* g_selfloop, float* d_a_dst, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0 && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL, "sgs_gat_alpha_bwd: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(a_src && a_dst && in_ptr && soft_loop && gloop && g_selfloop && d_a_dst, SGS_EINVAL, "sgs_gat_alpha_bwd: null pointer");
    hipLaunchKernelGGL(gat_alpha_bwd, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, a_src, a_dst, N, in_ptr, in_src, in_eid,
                       negative_slope, 1.0f / (1.0f - p_drop), dropout_thresh(p_drop), p_drop > 0.f ? 1 : 0, seed, site, epoch_ptr(), soft_in,
                       soft_loop, galpha, gloop, g_edge, g_selfloop, d_a_dst);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gather_by_eid(const float* by_eid, const int32_t* eid, int64_t n, float* out_order, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n >= 0, SGS_EINVAL, "sgs_gather_by_eid: bad size");
    if (n == 0) return SGS_OK;
    SGS_REQUIRE(by_eid && eid && out_order, SGS_EINVAL, "sgs_gather_by_eid: null pointer");
    hipLaunchKernelGGL(gather_by_eid, dim3(cdiv(n, kT)), dim3(kT), 0, stream, by_eid, eid, n, out_order, dyn_edges_ptr());
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_scatter_by_eid(const float* in_order, const int32_t* eid, int64_t n, float* by_eid, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(n >= 0, SGS_EINVAL, "sgs_scatter_by_eid: bad size");
    if (n == 0) return SGS_OK;
    SGS_REQUIRE(in_order && eid && by_eid, SGS_EINVAL, "sgs_scatter_by_eid: null pointer");
    hipLaunchKernelGGL(scatter_by_eid, dim3(cdiv(n, kT)), dim3(kT), 0, stream, in_order, eid, n, by_eid, dyn_edges_ptr());
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gat_scores_fwd(const float* xl, int64_t N, int64_t D, const float* att_src, const float* att_dst, float* a_src, float* a_dst,
                       sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D > 0, SGS_EINVAL, "sgs_gat_scores_fwd: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(xl && att_src && att_dst && a_src && a_dst, SGS_EINVAL, "sgs_gat_scores_fwd: null pointer");
    hipLaunchKernelGGL(gat_scores_fwd, dim3(static_cast<unsigned>((N * 64 + kT - 1) / kT)), dim3(kT), 0, stream, xl, N, D, att_src, att_dst, a_src, a_dst);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

static inline int gat_scores_rows_per_wg(int64_t N) { return N >= 65536 ? 256 : (N >= 4096 ? 64 : 16); }
size_t sgs_gat_scores_bwd_workspace_bytes(int64_t N, int64_t D) {
    if (N < 0) N = 0;
    if (D < 0) D = 0;
    const int64_t rp = gat_scores_rows_per_wg(N);
    return static_cast<size_t>((N + rp - 1) / rp) * 2 * D * 4 + 256;
}

int sgs_gat_scores_bwd(const float* xl, int64_t N, int64_t D, const float* att_src, const float* att_dst, const float* g_src, const float* g_dst,
                       int accumulate, float* dxl, float* datt_src, float* datt_dst, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D > 0, SGS_EINVAL, "sgs_gat_scores_bwd: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(xl && att_src && att_dst && g_src && g_dst && dxl && datt_src && datt_dst, SGS_EINVAL, "sgs_gat_scores_bwd: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_gat_scores_bwd_workspace_bytes(N, D), SGS_EWORKSPACE, "sgs_gat_scores_bwd: workspace too small");
    const int rp = gat_scores_rows_per_wg(N);
    const int nwg = static_cast<int>((N + rp - 1) / rp);
    float* part = static_cast<float*>(ws);
    if (accumulate)
        hipLaunchKernelGGL((gat_scores_bwd<true>), dim3(nwg), dim3(kT), 0, stream, xl, N, D, att_src, att_dst, g_src, g_dst, dxl, part, rp);
    else
        hipLaunchKernelGGL((gat_scores_bwd<false>), dim3(nwg), dim3(kT), 0, stream, xl, N, D, att_src, att_dst, g_src, g_dst, dxl, part, rp);
    hipLaunchKernelGGL(gat_scores_bwd_finish, dim3(static_cast<unsigned>((2 * D + 63) / 64)), dim3(1024), 0, stream, part, nwg, D, datt_src, datt_dst);
    SGS_LAUNCH_OK();
    return SGS_OK;
}


// ---------------------------------------------------------------- multi-head entry points
int sgs_gat_heads_supported(int64_t K, int64_t C) { return heads_ok(K, C) ? 1 : 0; }

int sgs_gat_heads_variant(int op, int64_t N, int64_t K, int64_t C, int aligned16) {
    if (op == SGS_GAT_OP_ROW) C = 1;                          // the per-row family has no channel axis
    if (!heads_ok(K, C) || N < 0) return -1;
    const int vec = (C % 4 == 0 && aligned16) ? 4 : 1;
    switch (op) {
        case SGS_GAT_OP_SCORES_FWD: return heads_code(1, vec, min6(log2_ceil(cdiv(C, vec))), 0, 0);
        case SGS_GAT_OP_SCORES_BWD: return heads_code(2, 1, 0, 0, gat_scores_rows_per_wg(N));
        case SGS_GAT_OP_SPMM_CONCAT: return heads_code(3, vec, min6(log2_ceil(cdiv(K * C, vec))), 0, 0);
        case SGS_GAT_OP_SPMM_MEAN: {
            const int lg = min6(log2_ceil(cdiv(K * C, vec)));
            if ((kT >> lg) * K * C <= kMeanLdsFloats) return heads_code(4, vec, lg, 0, 0);
            return heads_code(5, vec, min6(log2_ceil(cdiv(C, vec))), 0, 0);      // rows of more than 1024 floats: lanes own output columns and walk the heads
        }
        case SGS_GAT_OP_SPMM_BROADCAST: return heads_code(6, vec, min6(log2_ceil(cdiv(K * C, vec))), 0, 0);
        case SGS_GAT_OP_SDDMM:
        case SGS_GAT_OP_SDDMM_BROADCAST: {
            const int lgK = log2_ceil(K);
            int lgG = log2_ceil(cdiv(C, vec));
            if (lgG > 6 - lgK) lgG = 6 - lgK;
            return heads_code(op == SGS_GAT_OP_SDDMM ? 7 : 8, vec, lgK + lgG, lgG, 0);
        }
        case SGS_GAT_OP_ROW: return heads_code(9, 1, 0, 0, 1 << log2_ceil(K));
        default: return -1;
    }
}

#define SGS_REQUIRE_HEADS(name)                                                                                         \
    SGS_REQUIRE(heads_ok(K, C), SGS_EINVAL, name ": unsupported heads = %lld x channels = %lld (1 <= heads <= 16, channels >= 1)", \
                static_cast<long long>(K), static_cast<long long>(C))

int sgs_gat_scores_heads_fwd(const float* xl, int64_t N, int64_t K, int64_t C, const float* att_src, const float* att_dst, float* a_src,
                             float* a_dst, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_gat_scores_heads_fwd");
    SGS_REQUIRE(N >= 0 && N * K * 64 < (int64_t(1) << 40), SGS_EINVAL, "sgs_gat_scores_heads_fwd: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(xl && att_src && att_dst && a_src && a_dst, SGS_EINVAL, "sgs_gat_scores_heads_fwd: null pointer");
    const HeadsChoice ch(sgs_gat_heads_variant(SGS_GAT_OP_SCORES_FWD, N, K, C, al16(xl) && al16(att_src) && al16(att_dst)));
    const int lg = ch.lg;
    const dim3 grid(static_cast<unsigned>(cdiv((N * K) << lg, kT)));
    if (ch.vec == 4)
        hipLaunchKernelGGL((gat_scores_heads_fwd<4>), grid, dim3(kT), 0, stream, xl, N * K, static_cast<int>(K), C, att_src, att_dst, a_src, a_dst, lg);
    else
        hipLaunchKernelGGL((gat_scores_heads_fwd<1>), grid, dim3(kT), 0, stream, xl, N * K, static_cast<int>(K), C, att_src, att_dst, a_src, a_dst, lg);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_gat_scores_heads_bwd_workspace_bytes(int64_t N, int64_t K, int64_t C) {
    if (K < 0) K = 0;
    if (C < 0) C = 0;
    return sgs_gat_scores_bwd_workspace_bytes(N, K * C);
}

int sgs_gat_scores_heads_bwd(const float* xl, int64_t N, int64_t K, int64_t C, const float* att_src, const float* att_dst, const float* g_src,
                             const float* g_dst, int accumulate, float* dxl, float* datt_src, float* datt_dst, void* ws, size_t ws_bytes,
                             sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_gat_scores_heads_bwd");
    SGS_REQUIRE(N >= 0, SGS_EINVAL, "sgs_gat_scores_heads_bwd: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(xl && att_src && att_dst && g_src && g_dst && dxl && datt_src && datt_dst, SGS_EINVAL, "sgs_gat_scores_heads_bwd: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_gat_scores_heads_bwd_workspace_bytes(N, K, C), SGS_EWORKSPACE, "sgs_gat_scores_heads_bwd: workspace too small");
    const int64_t D = K * C;
    const int rp = HeadsChoice(sgs_gat_heads_variant(SGS_GAT_OP_SCORES_BWD, N, K, C, 0)).w;
    const int nwg = static_cast<int>((N + rp - 1) / rp);
    float* part = static_cast<float*>(ws);
    if (accumulate)
        hipLaunchKernelGGL((gat_scores_heads_bwd<true>), dim3(nwg), dim3(kT), 0, stream, xl, N, static_cast<int>(K), C, att_src, att_dst, g_src, g_dst,
                           dxl, part, rp);
    else
        hipLaunchKernelGGL((gat_scores_heads_bwd<false>), dim3(nwg), dim3(kT), 0, stream, xl, N, static_cast<int>(K), C, att_src, att_dst, g_src, g_dst,
                           dxl, part, rp);
    hipLaunchKernelGGL(gat_scores_bwd_finish, dim3(static_cast<unsigned>((2 * D + 63) / 64)), dim3(1024), 0, stream, part, nwg, D, datt_src, datt_dst);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gat_alpha_heads_fwd(const float* a_src, const float* a_dst, int64_t N, int64_t K, int64_t n_edges, const int32_t* in_ptr,
                            const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed, uint32_t site,
                            float* soft, float* soft_loop, float* alpha, float* alpha_loop, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t C = 1;
    SGS_REQUIRE_HEADS("sgs_gat_alpha_heads_fwd");
    SGS_REQUIRE(N >= 0 && n_edges >= 0 && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL, "sgs_gat_alpha_heads_fwd: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(a_src && a_dst && in_ptr && soft_loop && alpha_loop && (n_edges == 0 || (in_src && in_eid && soft && alpha)), SGS_EINVAL,
                "sgs_gat_alpha_heads_fwd: null pointer");
    SGS_DISPATCH_KPV(gat_alpha_heads_fwd, heads_kp(N, K), dim3(static_cast<unsigned>(cdiv(N * 64, kT))), stream, a_src, a_dst, N, static_cast<int>(K),
                     in_ptr, in_src, in_eid, negative_slope, 1.0f / (1.0f - p_drop), dropout_thresh(p_drop), p_drop > 0.f ? 1 : 0, seed, site, epoch_ptr(), soft,
                    soft_loop, alpha, alpha_loop);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gat_alpha_heads_bwd(const float* a_src, const float* a_dst, int64_t N, int64_t K, int64_t n_edges, const int32_t* in_ptr,
                            const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed, uint32_t site,
                            const float* soft, const float* soft_loop, const float* galpha, const float* gloop, float* g_edge, float* g_selfloop,
                            float* d_a_dst, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t C = 1;
    SGS_REQUIRE_HEADS("sgs_gat_alpha_heads_bwd");
    SGS_REQUIRE(N >= 0 && n_edges >= 0 && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL, "sgs_gat_alpha_heads_bwd: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(a_src && a_dst && in_ptr && soft_loop && gloop && g_selfloop && d_a_dst &&
                    (n_edges == 0 || (in_src && in_eid && soft && galpha && g_edge)),
                SGS_EINVAL, "sgs_gat_alpha_heads_bwd: null pointer");
    SGS_DISPATCH_KPV(gat_alpha_heads_bwd, heads_kp(N, K), dim3(static_cast<unsigned>(cdiv(N * 64, kT))), stream, a_src, a_dst, N, static_cast<int>(K),
                     in_ptr, in_src, in_eid, negative_slope, 1.0f / (1.0f - p_drop), dropout_thresh(p_drop), p_drop > 0.f ? 1 : 0, seed, site, epoch_ptr(), soft,
                    soft_loop, galpha, gloop, g_edge, g_selfloop, d_a_dst);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gat_alpha_heads_edge_fwd(const float* a_src, const float* a_dst, const float* edge_w, const float* edge_coef, int64_t N, int64_t K,
                                 int64_t n_edges, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, float negative_slope,
                                 float p_drop, uint64_t seed, uint32_t site, float* soft, float* soft_loop, float* alpha, float* alpha_loop,
                                 float* loop_w, float* loop_inv_cnt, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t C = 1;
    SGS_REQUIRE_HEADS("sgs_gat_alpha_heads_edge_fwd");
    SGS_REQUIRE(N >= 0 && n_edges >= 0 && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL, "sgs_gat_alpha_heads_edge_fwd: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(a_src && a_dst && edge_coef && in_ptr && soft_loop && alpha_loop && loop_w && loop_inv_cnt &&
                    (n_edges == 0 || (edge_w && in_src && in_eid && soft && alpha)),
                SGS_EINVAL, "sgs_gat_alpha_heads_edge_fwd: null pointer");
    SGS_DISPATCH_KPV(gat_alpha_heads_edge_fwd, heads_kp(N, K), dim3(static_cast<unsigned>(cdiv(N * 64, kT))), stream, a_src, a_dst, edge_w, edge_coef, N,
                    static_cast<int>(K), in_ptr, in_src, in_eid, negative_slope, 1.0f / (1.0f - p_drop), dropout_thresh(p_drop), p_drop > 0.f ? 1 : 0,
                    seed, site, epoch_ptr(), soft, soft_loop, alpha, alpha_loop, loop_w, loop_inv_cnt);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_gat_alpha_heads_edge_bwd_workspace_bytes(int64_t N, int64_t K) {
    if (N < 0) N = 0;
    if (K < 0) K = 0;
    return static_cast<size_t>(cdiv(N * 64, kT)) * static_cast<size_t>(K) * 4 + 256;
}

int sgs_gat_alpha_heads_edge_bwd(const float* a_src, const float* a_dst, const float* edge_w, const float* edge_coef, const float* loop_w,
                                 const float* loop_inv_cnt, int64_t N, int64_t K, int64_t n_edges, const int32_t* in_ptr, const int32_t* in_src,
                                 const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed, uint32_t site, const float* soft,
                                 const float* soft_loop, const float* galpha, const float* gloop, const float* dw_add, float* g_edge,
                                 float* g_selfloop, float* d_a_dst, float* d_edge_w, float* d_edge_coef, void* ws, size_t ws_bytes,
                                 sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t C = 1;
    SGS_REQUIRE_HEADS("sgs_gat_alpha_heads_edge_bwd");
    SGS_REQUIRE(N >= 0 && n_edges >= 0 && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL, "sgs_gat_alpha_heads_edge_bwd: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(a_src && a_dst && edge_coef && loop_w && loop_inv_cnt && in_ptr && soft_loop && gloop && g_selfloop && d_a_dst && d_edge_coef &&
                    (n_edges == 0 || (edge_w && in_src && in_eid && soft && galpha && g_edge && d_edge_w)),
                SGS_EINVAL, "sgs_gat_alpha_heads_edge_bwd: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_gat_alpha_heads_edge_bwd_workspace_bytes(N, K), SGS_EWORKSPACE,
                "sgs_gat_alpha_heads_edge_bwd: workspace too small");
    const int nwg = static_cast<int>(cdiv(N * 64, kT));
    float* part = static_cast<float*>(ws);
    SGS_DISPATCH_KPV(gat_alpha_heads_edge_bwd, heads_kp(N, K), dim3(static_cast<unsigned>(nwg)), stream, a_src, a_dst, edge_w, edge_coef, loop_w, loop_inv_cnt, N,
                    static_cast<int>(K), in_ptr, in_src, in_eid, negative_slope, 1.0f / (1.0f - p_drop), dropout_thresh(p_drop), p_drop > 0.f ? 1 : 0,
                    seed, site, epoch_ptr(), soft, soft_loop, galpha, gloop, dw_add, g_edge, g_selfloop, d_a_dst, d_edge_w, part);
    hipLaunchKernelGGL(gat_edge_dc_finish, dim3(1), dim3(1024), 0, stream, part, nwg, static_cast<int>(K), d_edge_coef);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_edge_sum_by_row_heads(const float* g_edge, const float* g_self, int64_t N, int64_t K, int64_t nnz, const int32_t* ptr, const int32_t* eid,
                              float* out, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t C = 1;
    SGS_REQUIRE_HEADS("sgs_edge_sum_by_row_heads");
    SGS_REQUIRE(N >= 0 && nnz >= 0, SGS_EINVAL, "sgs_edge_sum_by_row_heads: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(ptr && out && (nnz == 0 || (g_edge && eid)), SGS_EINVAL, "sgs_edge_sum_by_row_heads: null pointer");
    SGS_DISPATCH_KPV(edge_sum_by_row_heads, heads_kp(N, K), dim3(static_cast<unsigned>(cdiv(N * 64, kT))), stream, g_edge, g_self, N, static_cast<int>(K), ptr, eid,
                    out);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_spmm_csr_heads(const float* X, int64_t N, int64_t K, int64_t C, int64_t nnz, const int32_t* ptr, const int32_t* col, const int32_t* eid,
                       const float* val, const float* diag, int mode, const float* bias, int act, float p_drop, uint64_t seed, uint32_t site,
                       float* Y, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_spmm_csr_heads");
    SGS_REQUIRE(N >= 0 && nnz >= 0 && mode >= SGS_HEADS_CONCAT && mode <= SGS_HEADS_BROADCAST, SGS_EINVAL, "sgs_spmm_csr_heads: bad sizes / mode");
    SGS_REQUIRE(act >= SGS_ACT_NONE && act <= SGS_ACT_RELU_DROPOUT && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL,
                "sgs_spmm_csr_heads: bad activation / dropout");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(X && ptr && Y && X != Y && (nnz == 0 || (col && eid && val)), SGS_EINVAL, "sgs_spmm_csr_heads: null or aliased pointer");
    const int op = mode == SGS_HEADS_MEAN ? SGS_GAT_OP_SPMM_MEAN : (mode == SGS_HEADS_BROADCAST ? SGS_GAT_OP_SPMM_BROADCAST : SGS_GAT_OP_SPMM_CONCAT);
    const HeadsChoice ch(sgs_gat_heads_variant(op, N, K, C, al16(X) && al16(Y)));
    const int vec = ch.vec, lg = ch.lg;
    const bool mean_lds = ch.kind == 4;
    const float scale = 1.0f / (1.0f - p_drop);
    const uint32_t th = dropout_thresh(p_drop);
    if (act == SGS_ACT_RELU_DROPOUT && p_drop == 0.f) act = SGS_ACT_RELU;
    const int Ki = static_cast<int>(K);
    const dim3 grid(static_cast<unsigned>(cdiv(N, kT >> lg)));
#define SGS_SPMM_HEADS_ARGS X, N, Ki, C, ptr, col, eid, val, diag, bias, act, scale, th, seed, site, epoch_ptr(), Y, lg
    if (mean_lds) {
        if (vec == 4) hipLaunchKernelGGL((spmm_csr_heads_mean_lds<4>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_ARGS);
        else          hipLaunchKernelGGL((spmm_csr_heads_mean_lds<1>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_ARGS);
    } else if (mode == SGS_HEADS_MEAN) {
        if (vec == 4) hipLaunchKernelGGL((spmm_csr_heads_mean<4>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_ARGS);
        else          hipLaunchKernelGGL((spmm_csr_heads_mean<1>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_ARGS);
    } else if (mode == SGS_HEADS_BROADCAST) {
        if (vec == 4) hipLaunchKernelGGL((spmm_csr_heads<4, true>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_ARGS);
        else          hipLaunchKernelGGL((spmm_csr_heads<1, true>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_ARGS);
    } else {
        if (vec == 4) hipLaunchKernelGGL((spmm_csr_heads<4, false>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_ARGS);
        else          hipLaunchKernelGGL((spmm_csr_heads<1, false>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_ARGS);
    }
#undef SGS_SPMM_HEADS_ARGS
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_sddmm_csr_heads(const float* A, const float* B, int64_t N, int64_t K, int64_t C, int64_t nnz, const int32_t* ptr, const int32_t* col,
                        const int32_t* eid, int broadcast, float* g, float* gdiag, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_sddmm_csr_heads");
    SGS_REQUIRE(N >= 0 && nnz >= 0, SGS_EINVAL, "sgs_sddmm_csr_heads: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(A && B && ptr && gdiag && (nnz == 0 || (col && eid && g)), SGS_EINVAL, "sgs_sddmm_csr_heads: null pointer");
    const HeadsChoice ch(sgs_gat_heads_variant(broadcast ? SGS_GAT_OP_SDDMM_BROADCAST : SGS_GAT_OP_SDDMM, N, K, C, al16(A) && al16(B)));
    const int vec = ch.vec, lg = ch.lg, lgG = ch.lgG;
    const int Ki = static_cast<int>(K);
    const dim3 grid(static_cast<unsigned>(cdiv(N, kT >> lg)));
#define SGS_SDDMM_HEADS_ARGS A, B, N, Ki, C, ptr, col, eid, g, gdiag, lg, lgG
    if (broadcast) {
        if (vec == 4) hipLaunchKernelGGL((sddmm_csr_heads<4, true>), grid, dim3(kT), 0, stream, SGS_SDDMM_HEADS_ARGS);
        else          hipLaunchKernelGGL((sddmm_csr_heads<1, true>), grid, dim3(kT), 0, stream, SGS_SDDMM_HEADS_ARGS);
    } else {
        if (vec == 4) hipLaunchKernelGGL((sddmm_csr_heads<4, false>), grid, dim3(kT), 0, stream, SGS_SDDMM_HEADS_ARGS);
        else          hipLaunchKernelGGL((sddmm_csr_heads<1, false>), grid, dim3(kT), 0, stream, SGS_SDDMM_HEADS_ARGS);
    }
#undef SGS_SDDMM_HEADS_ARGS
    SGS_LAUNCH_OK();
    return SGS_OK;
}

// ---------------------------------------------------------------- multi-draw entry points (ensemble evaluation, forward only)
int sgs_gat_alpha_heads_fwd_multi(const float* a_src, const float* a_dst, int64_t a_stride, const float* edge_w, const float* edge_coef,
                                  int64_t N, int64_t K, int64_t D, int64_t nnz, const int32_t* in_ptr, const int32_t* in_src,
                                  const int32_t* in_eid, float negative_slope, float* alpha, float* alpha_loop, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t C = 1;
    SGS_REQUIRE_HEADS("sgs_gat_alpha_heads_fwd_multi");
    SGS_REQUIRE(N >= 0 && nnz >= 0 && D >= 1 && D <= 65535 && (a_stride == 0 || a_stride >= N * K), SGS_EINVAL,
                "sgs_gat_alpha_heads_fwd_multi: bad sizes (1 <= D <= 65535; a_stride 0 or >= N K)");
    SGS_REQUIRE((edge_w == nullptr) == (edge_coef == nullptr) || nnz == 0, SGS_EINVAL,
                "sgs_gat_alpha_heads_fwd_multi: edge_w and edge_coef come together");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(a_src && a_dst && in_ptr && alpha_loop && (nnz == 0 || (in_src && in_eid && alpha)), SGS_EINVAL,
                "sgs_gat_alpha_heads_fwd_multi: null pointer");
    const dim3 grid(static_cast<unsigned>(cdiv(N * 64, kT)), static_cast<unsigned>(D));
    if (edge_coef)
        SGS_DISPATCH_KP(gat_alpha_heads_edge_fwd_multi, K, grid, stream, a_src, a_dst, a_stride, edge_w, edge_coef, N, static_cast<int>(K), nnz, in_ptr,
                        in_src, in_eid, negative_slope, alpha, alpha_loop);
    else
        SGS_DISPATCH_KP(gat_alpha_heads_fwd_multi, K, grid, stream, a_src, a_dst, a_stride, N, static_cast<int>(K), nnz, in_ptr, in_src, in_eid,
                        negative_slope, alpha, alpha_loop);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_spmm_csr_heads_multi(const float* X, int64_t x_stride, int64_t N, int64_t K, int64_t C, int64_t nnz, int64_t D, const int32_t* ptr,
                             const int32_t* col, const int32_t* eid, const float* val, const float* diag, int mode, const float* bias, int act,
                             float* Y, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_spmm_csr_heads_multi");
    SGS_REQUIRE(N >= 0 && nnz >= 0 && D >= 1 && D <= 65535 && (x_stride == 0 || x_stride >= N * K * C) &&
                    (mode == SGS_HEADS_CONCAT || mode == SGS_HEADS_MEAN),
                SGS_EINVAL, "sgs_spmm_csr_heads_multi: bad sizes / mode (1 <= D <= 65535; x_stride 0 or >= N K C; CONCAT or MEAN)");
    SGS_REQUIRE(act == SGS_ACT_NONE || act == SGS_ACT_RELU, SGS_EINVAL, "sgs_spmm_csr_heads_multi: act must be NONE or RELU");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(X && ptr && Y && X != Y && (nnz == 0 || (col && eid && val)), SGS_EINVAL, "sgs_spmm_csr_heads_multi: null or aliased pointer");
    // the single-draw choice of vector width, made for every draw's block at once (their starts differ by multiples of 4 floats when C % 4 == 0)
    const int vec = (C % 4 == 0 && al16(X) && al16(Y) && x_stride % 4 == 0) ? 4 : 1;
    const int Ki = static_cast<int>(K);
    int lg = log2_ceil(cdiv(K * C, vec));
    if (lg > 6) lg = 6;
    const bool mean_lds = mode == SGS_HEADS_MEAN && (kT >> lg) * K * C <= kMeanLdsFloats;
    if (mode == SGS_HEADS_MEAN && !mean_lds) {
        lg = log2_ceil(cdiv(C, vec));
        if (lg > 6) lg = 6;
    }
    const dim3 grid(static_cast<unsigned>(cdiv(N, kT >> lg)), static_cast<unsigned>(D));
#define SGS_SPMM_HEADS_MULTI_ARGS X, x_stride, N, Ki, C, nnz, ptr, col, eid, val, diag, bias, act, Y, lg
    if (mean_lds) {
        if (vec == 4) hipLaunchKernelGGL((spmm_csr_heads_multi<4, 1>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_MULTI_ARGS);
        else          hipLaunchKernelGGL((spmm_csr_heads_multi<1, 1>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_MULTI_ARGS);
    } else if (mode == SGS_HEADS_MEAN) {
        if (vec == 4) hipLaunchKernelGGL((spmm_csr_heads_multi<4, 2>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_MULTI_ARGS);
        else          hipLaunchKernelGGL((spmm_csr_heads_multi<1, 2>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_MULTI_ARGS);
    } else {
        if (vec == 4) hipLaunchKernelGGL((spmm_csr_heads_multi<4, 0>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_MULTI_ARGS);
        else          hipLaunchKernelGGL((spmm_csr_heads_multi<1, 0>), grid, dim3(kT), 0, stream, SGS_SPMM_HEADS_MULTI_ARGS);
    }
#undef SGS_SPMM_HEADS_MULTI_ARGS
    SGS_LAUNCH_OK();
    return SGS_OK;
}

}  // extern "C"
