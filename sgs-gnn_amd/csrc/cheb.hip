// Chebyshev head, K > 1 (PyG ChebConv, normalization = 'sym', lambda_max = 2): the scaled-Laplacian normalisation of an edge list and
// the fused three-term recurrence step.  L_hat = 2 L / lambda_max - I has the off-diagonal entries l_e = -dis[s_e] w_e dis[d_e] and a zero
// diagonal (1 - 1), so unlike the GCN normalisation (gcn.hip) there is no loop term, the degree is summed BY SOURCE, and existing
// (i, i) edges carry weight 0 everywhere.  Nothing here assumes a symmetric edge list: the forward aggregates over the dst-CSR, the
// backward over the src-CSR.
//
// The layer runs Clenshaw's recurrence at the OUTPUT width (the host forms Y = X [W_0 | ... | W_{K-1}]^T with library GEMMs):
//     b_k = Y_k + 2 L_hat b_{k+1} - b_{k+2}   (k = K-1 ... 1),      out = act(Y_0 + L_hat b_1 - b_2 + bias)
// and its backward the direct recurrence U_k = 2 L_hat^T U_{k-1} - U_{k-2} over the src-CSR.  Every step is ONE launch of cheb_spmm:
//     Y[i, :] = act(add[i, :] + alpha * sum_k val[k] X[col[k], :] - sub[i, :] + bias)
// with a leading dimension per dense operand, so the steps read and write column blocks of the concatenated buffers in place.
//
// No float atomics: every per-row sum runs in CSR order over a fixed tree (run-to-run identical).  No host synchronisation.
#include "sgs_common.h"
#include "spmm_plan.h"

namespace sgs {
namespace {

constexpr int kT = 256;
constexpr int kMaxK = 8;      // a choice, not a hardware limit (include/sgs_hip.h)

inline bool cheb_ok(int64_t K) { return K >= 1 && K <= kMaxK; }

// ---------------------------------------------------------------- normalisation
// deg_n = sum of w over the OUT-edges of n (self loops excluded), dis = deg^-1/2 (inf -> 0).  One wave per node.
__global__ void __launch_bounds__(kT) cheb_deg(const float* __restrict__ w, int64_t N, const int* __restrict__ out_ptr,
                                              const int* __restrict__ out_dst, const int* __restrict__ out_eid, float* __restrict__ dis) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;
    float acc = 0.f;
    for (int k = out_ptr[i] + lane; k < out_ptr[i + 1]; k += 64)
        if (out_dst[k] != static_cast<int>(i)) acc += w ? w[out_eid[k]] : 1.0f;
    acc = wave_sum_all(acc);
    float di = 1.0f / sqrtf(acc);           // deg.pow(-0.5)
    if (isinf(di)) di = 0.f;                // masked_fill(inf -> 0): nodes without out-edges
    if (lane == 0) dis[i] = di;
}

// l = -(dis[src] * w) * dis[dst] in both CSR orders (the same product order, so the two copies are bitwise equal); 0 on (i, i) entries.
__global__ void __launch_bounds__(kT) cheb_weights(const float* __restrict__ w, int64_t N, const int* __restrict__ in_ptr,
                                                  const int* __restrict__ in_src, const int* __restrict__ in_eid,
                                                  const int* __restrict__ out_ptr, const int* __restrict__ out_dst,
                                                  const int* __restrict__ out_eid, const float* __restrict__ dis,
                                                  float* __restrict__ l_in, float* __restrict__ l_out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (r >= 2 * N) return;
    const bool out = r >= N;
    const int i = static_cast<int>(out ? r - N : r);
    const float di = dis[i];
    if (!out) {
        for (int k = in_ptr[i] + lane; k < in_ptr[i + 1]; k += 64) {
            const int s = in_src[k];
            const float we = w ? w[in_eid[k]] : 1.0f;
            l_in[k] = (s == i) ? 0.f : -((dis[s] * we) * di);
        }
    } else {
        for (int k = out_ptr[i] + lane; k < out_ptr[i + 1]; k += 64) {
            const int t = out_dst[k];
            const float we = w ? w[out_eid[k]] : 1.0f;
            l_out[k] = (t == i) ? 0.f : -((di * we) * dis[t]);
        }
    }
}

// ---- D drawn subgraphs of one partition (ensemble evaluation, forward only): blockIdx.y = draw d.
// The engine has the drawn subgraphs' in-CSRs only (sgs_graph_filter_multi), and the degree is summed by SOURCE.  cheb_deg_multi walks the
// PARENT's out-row of node i under draw d's mask instead of a filtered out-CSR: the filter keeps the parent's entry order, so the selected
// entries of the row, in order, are the drawn subgraph's out-row, and entry number r of that row belongs to lane r % 64 of cheb_deg.  Each
// step of 64 parent entries hands its selected values to those lanes with one ds_permute (the unselected lanes fill the other lanes with
// +0, which changes no partial sum), so every lane adds the same values in the same order as cheb_deg over the filtered out-CSR and the
// wave sum is the same tree: dis [D, N] is bitwise the single-draw result.  Weights are read by PARENT edge id (wE [D, E], scattered by
// cheb_scatter_w_multi; only selected edges are read, so the rest of wE stays unwritten); wE == NULL = unit weights.
__global__ void __launch_bounds__(kT) cheb_scatter_w_multi(const float* __restrict__ w, const int64_t* __restrict__ sampled_eid, int64_t q, int64_t E,
                                                          float* __restrict__ wE) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (j >= q) return;
    const int64_t d = blockIdx.y;
    wE[d * E + sampled_eid[d * q + j]] = w[d * q + j];
}

__global__ void __launch_bounds__(kT) cheb_deg_multi(const float* __restrict__ wE, int64_t N, int64_t E, const int* __restrict__ pout_ptr,
                                                    const int* __restrict__ pout_dst, const int* __restrict__ pout_eid,
                                                    const uint8_t* __restrict__ mask, float* __restrict__ dis) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (i >= N) return;                                       // wave-uniform
    const int64_t d = blockIdx.y;
    const uint8_t* __restrict__ m = mask + d * E;
    const float* __restrict__ w = wE ? wE + d * E : nullptr;
    const unsigned long long below = (1ull << lane) - 1ull;
    float acc = 0.f;
    int base = 0;                                             // selected entries of the row so far
    const int b = pout_ptr[i], e = pout_ptr[i + 1];
    for (int k0 = b; k0 < e; k0 += 64) {                      // wave-uniform trips: every lane takes part in the permute
        const int k = k0 + lane;
        bool sel = false;
        float v = 0.f;
        if (k < e) {
            const int pe = pout_eid[k];
            sel = m[pe] != 0;
            if (sel && pout_dst[k] != static_cast<int>(i)) v = w ? w[pe] : 1.0f;
        }
        const unsigned long long bal = __ballot(sel);
        const int cnt = __popcll(bal);
        const int r = sel ? __popcll(bal & below) : cnt + __popcll(~bal & below);      // a permutation of 0 .. 63
        acc += __int_as_float(__builtin_amdgcn_ds_permute(((base + r) & 63) << 2, __float_as_int(v)));
        base += cnt;
    }
    acc = wave_sum_all(acc);
    float di = 1.0f / sqrtf(acc);
    if (isinf(di)) di = 0.f;
    if (lane == 0) dis[d * N + i] = di;
}

// cheb_weights' in-rows for draw d: l_in [D, nnz] over the draw's in-CSR, w [D, nnz] by the draw's edge id (NULL: unit).
__global__ void __launch_bounds__(kT) cheb_weights_multi(const float* __restrict__ w, int64_t N, int64_t nnz, const int* __restrict__ in_ptr,
                                                        const int* __restrict__ in_src, const int* __restrict__ in_eid,
                                                        const float* __restrict__ dis, float* __restrict__ l_in) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (r >= N) return;
    const int64_t d = blockIdx.y;
    in_ptr += d * (N + 1); in_src += d * nnz; in_eid += d * nnz; dis += d * N; l_in += d * nnz;
    if (w) w += d * nnz;
    const int i = static_cast<int>(r);
    const float di = dis[i];
    for (int k = in_ptr[i] + lane; k < in_ptr[i + 1]; k += 64) {
        const int s = in_src[k];
        const float we = w ? w[in_eid[k]] : 1.0f;
        l_in[k] = (s == i) ? 0.f : -((dis[s] * we) * di);
    }
}

// c_n = -1/2 dis_n^3 (sum_{e: s_e = n} -w_e dis[d_e] g_e + sum_{e: d_e = n} -dis[s_e] w_e g_e): what the degree of n passes back to
// each of its out-edges' weights.  g2 (optional): a second layer's gradient over the same normalisation, summed on read.
__global__ void __launch_bounds__(kT) cheb_norm_bwd_node(const float* __restrict__ w, const float* __restrict__ g, const float* __restrict__ g2,
                                                        int64_t N, const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                        const int* __restrict__ in_eid, const int* __restrict__ out_ptr,
                                                        const int* __restrict__ out_dst, const int* __restrict__ out_eid,
                                                        const float* __restrict__ dis, float* __restrict__ cn) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x) >> 6;
    if (t >= N) return;
    float acc = 0.f;
    auto side = [&](const int* __restrict__ ptr, const int* __restrict__ col, const int* __restrict__ eid) {
        const int e_ = ptr[t + 1];
        for (int k = ptr[t] + lane; k < e_; k += 64) {
            const int s = col[k], e = eid[k];
            const float ge = g2 ? g[e] + g2[e] : g[e];
            if (s != static_cast<int>(t)) acc -= ge * w[e] * dis[s];
        }
    };
    side(out_ptr, out_dst, out_eid);
    side(in_ptr, in_src, in_eid);
    acc = wave_sum_all(acc);
    if (lane == 0) {
        const float a = dis[t];
        cn[t] = -0.5f * a * a * a * acc;
    }
}

__global__ void __launch_bounds__(kT) cheb_norm_bwd_edge(const float* __restrict__ g, const float* __restrict__ g2,
                                                        const int64_t* __restrict__ ei, int64_t n_edges, const float* __restrict__ dis,
                                                        const float* __restrict__ cn, float* __restrict__ dw) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
    if (e >= n_edges) return;
    const int s = static_cast<int>(ei[e]), t = static_cast<int>(ei[n_edges + e]);
    float r = 0.f;                                        // (i, i) edges are removed: their weight reaches nothing
    if (s != t) r = cn[s] - (g2 ? g[e] + g2[e] : g[e]) * dis[s] * dis[t];
    dw[e] = r;
}

// ---------------------------------------------------------------- the recurrence step
template <int VEC> struct VecT;
template <> struct VecT<1> { using type = float; };
template <> struct VecT<4> { using type = float4; };

struct StepArgs {
    const float* X;   int64_t ldx;       // gathered operand
    const float* add; int64_t ldadd;     // may be NULL; may be Y itself (in place: each element is read and written by one thread)
    const float* sub; int64_t ldsub;     // may be NULL
    const float* bias;                   // may be NULL
    float* Y;         int64_t ldy;
    float* Y2;        int64_t ldy2;      // may be NULL: a second copy of the result scaled by scale2
    float alpha, scale2;
    int act;
    float drop_scale;
    uint32_t drop_thresh;
    uint64_t seed;
    uint32_t site;
    const uint64_t* epoch;
};

// everything after the row sum, for one element (row i, column c)
__device__ __forceinline__ void finish(const StepArgs& a, int64_t i, int64_t c, float s, uint32_t rkey) {
    float y = a.alpha * s;
    if (a.add) y = a.add[i * a.ldadd + c] + y;
    if (a.sub) y -= a.sub[i * a.ldsub + c];
    if (a.bias) y += a.bias[c];
    if (a.act != SGS_ACT_NONE) y = fmaxf(y, 0.f);
    if (a.act == SGS_ACT_RELU_DROPOUT) y = dropout_keep_col(rkey, static_cast<uint32_t>(c), a.drop_thresh) ? y * a.drop_scale : 0.f;
    a.Y[i * a.ldy + c] = y;
    if (a.Y2) a.Y2[i * a.ldy2 + c] = a.scale2 * y;
}

// Short rows (whole graphs of low degree): a group of LPR lanes owns one output row, each lane VEC consecutive columns per chunk,
// four independent row gathers in flight (the load order sgs_spmm_csr settled on).
// The *_body function below is the only copy of the row code: the single-draw kernel after it and the multi-draw kernel both call it, as
// do the two callers of cheb_spmm_rowblock_body ("The bodies").
template <int VEC, int LPR>
__device__ __forceinline__ void cheb_spmm_rows_body(const StepArgs& a, int64_t N, int64_t D, const int* __restrict__ ptr,
                                                    const int* __restrict__ col, const float* __restrict__ val) {
    using V = typename VecT<VEC>::type;
    constexpr int RPB = kT / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / LPR;
    if (i >= N) return;
    const uint32_t rkey = dropout_row_key(fold_epoch(a.seed, a.epoch), a.site, static_cast<uint64_t>(i));
    const int b = ptr[i], e = ptr[i + 1];
    const float* __restrict__ X = a.X;
    const int64_t ldx = a.ldx;
    for (int64_t c0 = static_cast<int64_t>(sub) * VEC; c0 < D; c0 += static_cast<int64_t>(LPR) * VEC) {
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        int k = b;
        for (; k + 4 <= e; k += 4) {
            int j[4]; float w[4]; float x[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; ++u) { j[u] = col[k + u]; w[u] = val[k + u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<V*>(x[u]) = *reinterpret_cast<const V*>(X + static_cast<int64_t>(j[u]) * ldx + c0);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
        }
        for (; k < e; ++k) {
            float x[VEC];
            *reinterpret_cast<V*>(x) = *reinterpret_cast<const V*>(X + static_cast<int64_t>(col[k]) * ldx + c0);
            const float w = val[k];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[v], acc[v]);
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) finish(a, i, c0 + v, acc[v], rkey);
    }
}
template <int VEC, int LPR>
__global__ void __launch_bounds__(kT) cheb_spmm_rows(StepArgs a, int64_t N, int64_t D, const int* __restrict__ ptr,
                                                    const int* __restrict__ col, const float* __restrict__ val) {
    cheb_spmm_rows_body<VEC, LPR>(a, N, D, ptr, col, val);
}

// Long rows (partitions: ~1k rows of tens to hundreds of entries): a workgroup of NW waves owns a row, each wave gathers a strided
// share of its entries (8 in flight) and the partial sums meet in LDS in a fixed order.  NW = 16 for very long rows.
// SINGLE selects no code: it is true from the single-draw kernel, so that each caller has an instantiation of its own.  The multi-draw
// kernel's LDS array reaches the body as a constant only while that kernel is the instantiation's one caller; sharing it changed the
// multi-draw kernel's instruction order.  (cheb_spmm_rows_body takes no such argument and is shared as it is.)
template <int VEC, int NW, bool SINGLE = false>
__device__ __forceinline__ void cheb_spmm_rowblock_body(const StepArgs& a, int64_t N, int64_t D, const int* __restrict__ ptr,
                                                             const int* __restrict__ col, const float* __restrict__ val, float (*part)[64 * VEC]) {
    using V = typename VecT<VEC>::type;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const int b = ptr[i], e = ptr[i + 1];
    const uint32_t rkey = dropout_row_key(fold_epoch(a.seed, a.epoch), a.site, static_cast<uint64_t>(i));
    const float* __restrict__ X = a.X;
    const int64_t ldx = a.ldx;
    for (int64_t cbase = 0; cbase < D; cbase += 64 * VEC) {
        const int64_t c0 = cbase + static_cast<int64_t>(lane) * VEC;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        if (c0 < D) {
            int k = b + wave;
            for (; k + 7 * NW < e; k += 8 * NW) {
                int j[8]; float w[8]; V x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { j[u] = col[k + NW * u]; w[u] = val[k + NW * u]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const V*>(X + static_cast<int64_t>(j[u]) * ldx + c0);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float xv[VEC];
                    *reinterpret_cast<V*>(xv) = x[u];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], xv[v], acc[v]);
                }
            }
            for (; k < e; k += NW) {
                float xv[VEC];
                *reinterpret_cast<V*>(xv) = *reinterpret_cast<const V*>(X + static_cast<int64_t>(col[k]) * ldx + c0);
                const float w = val[k];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, xv[v], acc[v]);
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) part[wave][lane * VEC + v] = acc[v];
        __syncthreads();
        const int t = threadIdx.x;                 // 64 * VEC columns finished by the first 64 * VEC threads
        if (t < 64 * VEC && cbase + t < D) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < NW; g += 4) s += (part[g][t] + part[g + 1][t]) + (part[g + 2][t] + part[g + 3][t]);
            finish(a, i, cbase + t, s, rkey);
        }
        __syncthreads();
    }
}
template <int VEC, int NW>
__global__ void __launch_bounds__(64 * NW) cheb_spmm_rowblock(StepArgs a, int64_t N, int64_t D, const int* __restrict__ ptr,
                                                             const int* __restrict__ col, const float* __restrict__ val) {
    __shared__ float part[NW][64 * VEC];
    cheb_spmm_rowblock_body<VEC, NW, true>(a, N, D, ptr, col, val, part);
}

// One recurrence step for the D drawn subgraphs of a partition (ensemble evaluation: forward only, bias / ReLU, no dropout, no Y2):
// blockIdx.y = draw d.  Each dense operand keeps its leading dimension and has a draw stride of its own (0: shared by every draw -- the
// layer-1 products Y_0 and, at K = 2, Y_1, which no step overwrites); ptr [D, N+1], col / val [D, nnz].  The bodies above run unchanged
// on draw d's operands, and the host picks the row form and the vector width by sgs_cheb_spmm's rules, so block d is bitwise that call's.
struct StepStrides { int64_t x, add, sub, y; };
__device__ __forceinline__ StepArgs step_of_draw(StepArgs a, const StepStrides& st, int64_t d) {
    a.X += d * st.x;
    if (a.add) a.add += d * st.add;
    if (a.sub) a.sub += d * st.sub;
    a.Y += d * st.y;
    return a;
}
template <int VEC, int LPR>
__global__ void __launch_bounds__(kT) cheb_spmm_rows_multi(StepArgs a, StepStrides st, int64_t N, int64_t D, int64_t nnz,
                                                          const int* __restrict__ ptr, const int* __restrict__ col,
                                                          const float* __restrict__ val) {
    const int64_t d = blockIdx.y;
    cheb_spmm_rows_body<VEC, LPR>(step_of_draw(a, st, d), N, D, ptr + d * (N + 1), col + d * nnz, val + d * nnz);
}
template <int VEC, int NW>
__global__ void __launch_bounds__(64 * NW) cheb_spmm_rowblock_multi(StepArgs a, StepStrides st, int64_t N, int64_t D, int64_t nnz,
                                                                   const int* __restrict__ ptr, const int* __restrict__ col,
                                                                   const float* __restrict__ val) {
    __shared__ float part[NW][64 * VEC];
    const int64_t d = blockIdx.y;
    cheb_spmm_rowblock_body<VEC, NW>(step_of_draw(a, st, d), N, D, ptr + d * (N + 1), col + d * nnz, val + d * nnz, part);
}

}  // namespace
}  // namespace sgs

using namespace sgs;

extern "C" {

int sgs_cheb_supported(int64_t K) { return cheb_ok(K) ? 1 : 0; }

#define SGS_REQUIRE_CHEB(name) \
    SGS_REQUIRE(cheb_ok(K), SGS_EINVAL, name ": unsupported Chebyshev order K = %lld (1 <= K <= 8)", static_cast<long long>(K))

int sgs_cheb_norm_fwd(const float* w, int64_t n_edges, int64_t N, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                      const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* dis, float* l_in, float* l_out,
                      sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_cheb_norm_fwd: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(in_ptr && out_ptr && dis && (n_edges == 0 || (in_src && in_eid && out_dst && out_eid && l_in && l_out)), SGS_EINVAL,
                "sgs_cheb_norm_fwd: null pointer");
    hipLaunchKernelGGL(cheb_deg, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, w, N, out_ptr, out_dst, out_eid, dis);
    if (n_edges > 0)
        hipLaunchKernelGGL(cheb_weights, dim3(cdiv(2 * N * 64, kT)), dim3(kT), 0, stream, w, N, in_ptr, in_src, in_eid, out_ptr, out_dst,
                           out_eid, dis, l_in, l_out);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_cheb_norm_bwd_workspace_bytes(int64_t N) { return carve_bytes(N < 0 ? 0 : N, 4) + 256; }

int sgs_cheb_norm_bwd(const float* w, const float* g, const float* g2, int64_t n_edges, int64_t N, const float* dis, const int32_t* in_ptr,
                      const int32_t* in_src, const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                      const int64_t* edge_index, float* dw, void* ws, size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && n_edges >= 0, SGS_EINVAL, "sgs_cheb_norm_bwd: bad sizes");
    if (N == 0 || n_edges == 0) return SGS_OK;
    SGS_REQUIRE(w && g && dis && in_ptr && in_src && in_eid && out_ptr && out_dst && out_eid && edge_index && dw, SGS_EINVAL,
                "sgs_cheb_norm_bwd: null pointer");
    SGS_REQUIRE(ws && ws_bytes >= sgs_cheb_norm_bwd_workspace_bytes(N), SGS_EWORKSPACE, "sgs_cheb_norm_bwd: workspace too small");
    Carver cv(ws);
    float* cn = cv.take<float>(N);
    hipLaunchKernelGGL(cheb_norm_bwd_node, dim3(cdiv(N * 64, kT)), dim3(kT), 0, stream, w, g, g2, N, in_ptr, in_src, in_eid, out_ptr, out_dst,
                       out_eid, dis, cn);
    hipLaunchKernelGGL(cheb_norm_bwd_edge, dim3(cdiv(n_edges, kT)), dim3(kT), 0, stream, g, g2, edge_index, n_edges, dis, cn, dw);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

/* Which kernel sgs_cheb_spmm / sgs_cheb_spmm_multi launch -- a pure host function of the shape, and both launchers switch on its result.
 * The encoding of sgs_spmm_csr_variant:  VEC * 100 + LPR for cheb_spmm_rows<VEC, LPR> (LPR = the power of two >= ceil(D / VEC), at most 64),
 * 1000 + VEC * 100 + NW for cheb_spmm_rowblock<VEC, NW> (N <= 65536 and nnz >= 16 N; NW = 16 from nnz >= 256 N).  VEC = 4 iff D % 4 == 0,
 * ldx % 4 == 0 and X is 16-byte aligned (aligned16 != 0; X only: the other operands are touched per element), else 1.  0 when nothing is
 * launched (N == 0 or D == 0), -1 for negative sizes. */
int sgs_cheb_spmm_variant(int64_t N, int64_t D, int64_t nnz, int64_t ldx, int al16) {
    if (N < 0 || D < 0 || nnz < 0 || ldx < 0) return -1;
    if (N == 0 || D == 0) return 0;
    return spmm_plan(N, D, nnz, ldx % 4 == 0 && al16).code();      // sgs_spmm_csr's plan; the gathered rows' pitch enters VEC
}

int sgs_cheb_spmm(int64_t K, const float* X, int64_t ldx, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col,
                  const float* val, float alpha, const float* add, int64_t ldadd, const float* sub, int64_t ldsub, const float* bias, int act,
                  float p_drop, uint64_t seed, uint32_t site, float* Y, int64_t ldy, float* Y2, int64_t ldy2, float scale2,
                  sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_CHEB("sgs_cheb_spmm");
    SGS_REQUIRE(N >= 0 && D >= 0 && nnz >= 0, SGS_EINVAL, "sgs_cheb_spmm: bad sizes");
    SGS_REQUIRE(act >= SGS_ACT_NONE && act <= SGS_ACT_RELU_DROPOUT && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL,
                "sgs_cheb_spmm: bad activation / dropout");
    if (N == 0 || D == 0) return SGS_OK;
    SGS_REQUIRE(X && ptr && Y && X != Y && X != Y2 && (nnz == 0 || (col && val)), SGS_EINVAL, "sgs_cheb_spmm: null or aliased pointer");
    SGS_REQUIRE(ldx >= D && ldy >= D && (!add || ldadd >= D) && (!sub || ldsub >= D) && (!Y2 || ldy2 >= D), SGS_EINVAL,
                "sgs_cheb_spmm: a leading dimension is smaller than D");
    // 16-byte gathers need the gathered operand's block start and row pitch aligned (the other operands are touched per element)
    const SpmmPlan p = SpmmPlan::of_code(sgs_cheb_spmm_variant(N, D, nnz, ldx, aligned16(X)));
    if (act == SGS_ACT_RELU_DROPOUT && p_drop == 0.f) act = SGS_ACT_RELU;
    StepArgs a;
    a.X = X; a.ldx = ldx; a.add = add; a.ldadd = ldadd; a.sub = sub; a.ldsub = ldsub; a.bias = bias; a.Y = Y; a.ldy = ldy;
    a.Y2 = Y2; a.ldy2 = ldy2; a.alpha = alpha; a.scale2 = scale2; a.act = act; a.drop_scale = 1.0f / (1.0f - p_drop);
    a.drop_thresh = dropout_thresh(p_drop); a.seed = seed; a.site = site; a.epoch = epoch_ptr();
    const dim3 g_(p.blocks(N)), b_(p.block());
    dispatch_plan(p, [&](auto V, auto W) { hipLaunchKernelGGL((cheb_spmm_rows<V(), W()>), g_, b_, 0, stream, a, N, D, ptr, col, val); },
                  [&](auto V, auto W) { hipLaunchKernelGGL((cheb_spmm_rowblock<V(), W()>), g_, b_, 0, stream, a, N, D, ptr, col, val); });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

// ---------------------------------------------------------------- multi-draw entry points (ensemble evaluation, forward only)
size_t sgs_cheb_norm_fwd_multi_workspace_bytes(int64_t E_parent, int64_t D) {
    if (E_parent < 0) E_parent = 0;
    if (D < 0) D = 0;
    return carve_bytes(static_cast<size_t>(E_parent) * static_cast<size_t>(D), 4) + 256;
}

int sgs_cheb_norm_fwd_multi(const float* w, const int64_t* sampled_eid, const uint8_t* mask, int64_t q, int64_t N, int64_t E_parent, int64_t D,
                            const int32_t* pout_ptr, const int32_t* pout_dst, const int32_t* pout_eid, const int32_t* in_ptr,
                            const int32_t* in_src, const int32_t* in_eid, float* dis, float* l_in, void* ws, size_t ws_bytes,
                            sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && q >= 0 && E_parent >= 0 && q <= E_parent && D >= 1 && D <= 65535, SGS_EINVAL,
                "sgs_cheb_norm_fwd_multi: bad sizes (q <= E_parent; 1 <= D <= 65535)");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(pout_ptr && in_ptr && dis && (E_parent == 0 || (pout_dst && pout_eid && mask)) &&
                    (q == 0 || (in_src && in_eid && l_in && (!w || sampled_eid))),
                SGS_EINVAL, "sgs_cheb_norm_fwd_multi: null pointer");
    float* wE = nullptr;
    if (w && q > 0) {
        SGS_REQUIRE(ws && ws_bytes >= sgs_cheb_norm_fwd_multi_workspace_bytes(E_parent, D), SGS_EWORKSPACE,
                    "sgs_cheb_norm_fwd_multi: workspace too small");
        Carver cv(ws);
        wE = cv.take<float>(static_cast<size_t>(E_parent) * static_cast<size_t>(D));
        hipLaunchKernelGGL(cheb_scatter_w_multi, dim3(static_cast<unsigned>(cdiv(q, kT)), static_cast<unsigned>(D)), dim3(kT), 0, stream, w,
                           sampled_eid, q, E_parent, wE);
    }
    const dim3 grid(static_cast<unsigned>(cdiv(N * 64, kT)), static_cast<unsigned>(D));
    hipLaunchKernelGGL(cheb_deg_multi, grid, dim3(kT), 0, stream, wE, N, E_parent, pout_ptr, pout_dst, pout_eid, mask, dis);
    if (q > 0) hipLaunchKernelGGL(cheb_weights_multi, grid, dim3(kT), 0, stream, w, N, q, in_ptr, in_src, in_eid, dis, l_in);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_cheb_spmm_multi(int64_t K, const float* X, int64_t ldx, int64_t x_stride, int64_t N, int64_t D, int64_t nnz, int64_t n_draws,
                        const int32_t* ptr, const int32_t* col, const float* val, float alpha, const float* add, int64_t ldadd,
                        int64_t add_stride, const float* sub, int64_t ldsub, int64_t sub_stride, const float* bias, int act, float* Y, int64_t ldy,
                        int64_t y_stride, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_CHEB("sgs_cheb_spmm_multi");
    SGS_REQUIRE(N >= 0 && D >= 0 && nnz >= 0 && n_draws >= 1 && n_draws <= 65535, SGS_EINVAL, "sgs_cheb_spmm_multi: bad sizes (1 <= draws <= 65535)");
    SGS_REQUIRE(act == SGS_ACT_NONE || act == SGS_ACT_RELU, SGS_EINVAL, "sgs_cheb_spmm_multi: act must be NONE or RELU");
    if (N == 0 || D == 0) return SGS_OK;
    SGS_REQUIRE(X && ptr && Y && X != Y && (nnz == 0 || (col && val)), SGS_EINVAL, "sgs_cheb_spmm_multi: null or aliased pointer");
    SGS_REQUIRE(ldx >= D && ldy >= D && (!add || ldadd >= D) && (!sub || ldsub >= D), SGS_EINVAL,
                "sgs_cheb_spmm_multi: a leading dimension is smaller than D");
    SGS_REQUIRE(x_stride >= 0 && add_stride >= 0 && sub_stride >= 0 && (n_draws == 1 || y_stride >= (N - 1) * ldy + D), SGS_EINVAL,
                "sgs_cheb_spmm_multi: bad draw stride (every draw writes a block of its own)");
    // sgs_cheb_spmm's rule, for every draw's block and on the per-draw entry count
    const SpmmPlan p = SpmmPlan::of_code(sgs_cheb_spmm_variant(N, D, nnz, ldx, x_stride % 4 == 0 && aligned16(X)));
    StepArgs a;
    a.X = X; a.ldx = ldx; a.add = add; a.ldadd = ldadd; a.sub = sub; a.ldsub = ldsub; a.bias = bias; a.Y = Y; a.ldy = ldy;
    a.Y2 = nullptr; a.ldy2 = 0; a.alpha = alpha; a.scale2 = 1.0f; a.act = act; a.drop_scale = 1.0f;
    a.drop_thresh = 0u; a.seed = 0; a.site = 0u; a.epoch = nullptr;
    StepStrides st;
    st.x = x_stride; st.add = add_stride; st.sub = sub_stride; st.y = y_stride;
    const dim3 g_(p.blocks(N), static_cast<unsigned>(n_draws)), b_(p.block());
    dispatch_plan(p, [&](auto V, auto W) { hipLaunchKernelGGL((cheb_spmm_rows_multi<V(), W()>), g_, b_, 0, stream, a, st, N, D, nnz, ptr, col, val); },
                  [&](auto V, auto W) { hipLaunchKernelGGL((cheb_spmm_rowblock_multi<V(), W()>), g_, b_, 0, stream, a, st, N, D, nnz, ptr, col, val); });
    SGS_LAUNCH_OK();
    return SGS_OK;
}

}  // extern "C"
