// GINE aggregation (PyG 2.3.1 GINEConv with edge_dim = 1 and the edge weight as the attribute, restated from its published algorithm):
//
//   t_e[c] = w_e a[c] + b[c]                                        a = lin.weight[:, 0], b = lin.bias (lin = Linear(1, D))
//   Z[i, c] = diag x[i, c] + sum_{e: j -> i} relu(x[j, c] + t_e[c])   diag = 1 + eps; (i, i) and duplicate entries are ordinary entries
//
// The ReLU sits inside the sum, so neither the layer's first Linear nor sgs_spmm_csr can take the aggregation's place: the kernels here
// gather rows at the INPUT width D and apply the edge term and the ReLU per gathered element.  Per entry they move 12 + 4 D bytes (column
// index, edge id, weight, one row) against 3 D flops: gather-bound, so the shapes are spmm_csr's -- one wave per row with 4 row gathers in
// flight (short rows), or a workgroup of NW = 4 / 16 waves per row, each wave gathering a strided share of the entries 4 at a time, the
// wave partials combined through LDS in a fixed order (few long rows: the partition shape).  A lane owns VEC = 4 / 2 / 1 consecutive
// columns per chunk of 64 VEC columns; VEC is the widest the alignment and D allow that still fills the wave (D = 602 -> 2, 256 -> 4).
//
// Mask-recompute contract: the forward stores no mask.  The backward recomputes the pre-activation with the SAME explicit expression,
// gine_pre() = x + (w a + b), from the same fp32 inputs; the library is built with -ffp-contract=off, so no multiply-add is fused on
// either side and the two values agree bit for bit: an element passes the ReLU in the backward iff it did in the forward.  w == NULL
// (unit weights) evaluates the same expression with w = 1.0f, so it is bitwise the result of a vector of ones.
//
// Backward (src-CSR; row j holds x_j, gathers dZ of its destinations; m = dZ[dst_e, c] where the recomputed pre-activation is > 0, else 0):
//   dX[j, c] = diag dZ[j, c] + sum_e m          (optional)
//   dw[e]    = sum_c a[c] m (+ dw_add[e])        a reduction across the wave per entry and column chunk; lane 63 adds the chunks up in
//                                               dw[e] itself (one thread owns an entry for the whole launch: program order, no atomics)
//   da[c]    = sum_e w_e m,  db[c] = sum_e m     lane-private over the rows of a workgroup, per-workgroup partials in the workspace, summed
//                                               in a fixed order by a second small launch
// No float atomics, no memset nodes, no host synchronisation: two identical launches give identical bits.
#include "sgs_common.h"

namespace sgs {
namespace {

constexpr int kT = 256;
constexpr int kMaxParts = 2048;      // most workgroups (= partial rows of d a / d b) a backward launch uses

// the pre-activation, written once: forward and backward agree on its sign bit for bit (see the contract above)
__device__ __forceinline__ float gine_pre(float x, float w, float a, float b) { return x + (w * a + b); }

template <int VEC> struct GV;
template <> struct GV<1> { using T = float; };
template <> struct GV<2> { using T = float2; };
template <> struct GV<4> { using T = float4; };

template <int VEC>
__device__ __forceinline__ void ldv(float (&dst)[VEC], const float* __restrict__ p) {
    using V = typename GV<VEC>::T;
    const V t = *reinterpret_cast<const V*>(p);
    __builtin_memcpy(dst, &t, sizeof(V));
}
template <int VEC>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&src)[VEC]) {
    using V = typename GV<VEC>::T;
    V t;
    __builtin_memcpy(&t, src, sizeof(V));
    *reinterpret_cast<V*>(p) = t;
}
template <int VEC>
__device__ __forceinline__ void zerov(float (&dst)[VEC]) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) dst[v] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// acc += relu(x_src + t_e) over entries k = k0, k0 + step, ... < end of one row, 4 gathers in flight
template <int VEC>
__device__ __forceinline__ void gine_gather(float (&acc)[VEC], const float* __restrict__ X, const float* __restrict__ w, int64_t D, int64_t c0,
                                            const int* __restrict__ src, const int* __restrict__ eid, int k0, int end, int step,
                                            const float (&av)[VEC], const float (&bv)[VEC]) {
    int k = k0;
    for (; k + 3 * step < end; k += 4 * step) {
        int j[4];
        float we[4], x[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            j[u] = src[k + u * step];
            we[u] = w ? w[eid[k + u * step]] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) ldv<VEC>(x[u], X + static_cast<int64_t>(j[u]) * D + c0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] += fmaxf(gine_pre(x[u][v], we[u], av[v], bv[v]), 0.f);
    }
    for (; k < end; k += step) {
        float x[VEC];
        const float we = w ? w[eid[k]] : 1.0f;
        ldv<VEC>(x, X + static_cast<int64_t>(src[k]) * D + c0);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += fmaxf(gine_pre(x[v], we, av[v], bv[v]), 0.f);
    }
}

// one wave per row, kT / 64 rows per workgroup: the body of a workgroup, shared by the single-draw and the multi-draw kernel
template <int VEC>
__device__ __forceinline__ void gine_fwd_wave_body(const float* __restrict__ X, const float* __restrict__ w, const float* __restrict__ a,
                                                   const float* __restrict__ b, float diag, int64_t N, int64_t D,
                                                   const int* __restrict__ ptr, const int* __restrict__ src, const int* __restrict__ eid,
                                                   float* __restrict__ Z) {
    const int lane = threadIdx.x & 63;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kT / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const int bgn = ptr[i], end = ptr[i + 1];
    for (int64_t c0 = static_cast<int64_t>(lane) * VEC; c0 < D; c0 += 64 * VEC) {
        float av[VEC], bv[VEC], acc[VEC], xi[VEC], o[VEC];
        ldv<VEC>(av, a + c0);
        ldv<VEC>(bv, b + c0);
        zerov<VEC>(acc);
        gine_gather<VEC>(acc, X, w, D, c0, src, eid, bgn, end, 1, av, bv);
        ldv<VEC>(xi, X + i * D + c0);
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = diag * xi[v] + acc[v];
        stv<VEC>(Z + i * D + c0, o);
    }
}

template <int VEC>
__global__ void __launch_bounds__(kT) gine_fwd_wave(const float* __restrict__ X, const float* __restrict__ w, const float* __restrict__ a,
                                                   const float* __restrict__ b, float diag, int64_t N, int64_t D,
                                                   const int* __restrict__ ptr, const int* __restrict__ src, const int* __restrict__ eid,
                                                   float* __restrict__ Z) {
    gine_fwd_wave_body<VEC>(X, w, a, b, diag, N, D, ptr, src, eid, Z);
}

// a workgroup of NW waves per row (row blockIdx.x)
template <int VEC, int NW>
__device__ __forceinline__ void gine_fwd_block_body(float (&part)[NW][64 * VEC], const float* __restrict__ X, const float* __restrict__ w,
                                                    const float* __restrict__ a, const float* __restrict__ b, float diag, int64_t D,
                                                    const int* __restrict__ ptr, const int* __restrict__ src, const int* __restrict__ eid,
                                                    float* __restrict__ Z) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const int bgn = ptr[i], end = ptr[i + 1];
    for (int64_t cbase = 0; cbase < D; cbase += 64 * VEC) {
        const int64_t c0 = cbase + static_cast<int64_t>(lane) * VEC;
        float acc[VEC];
        zerov<VEC>(acc);
        if (c0 < D) {
            float av[VEC], bv[VEC];
            ldv<VEC>(av, a + c0);
            ldv<VEC>(bv, b + c0);
            gine_gather<VEC>(acc, X, w, D, c0, src, eid, bgn + wave, end, NW, av, bv);
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) part[wave][lane * VEC + v] = acc[v];
        __syncthreads();
        const int t = threadIdx.x;
        if (t < 64 * VEC && cbase + t < D) {
            const int64_t c = cbase + t;
            float y = 0.f;
#pragma unroll
            for (int g = 0; g < NW; g += 4) y += (part[g][t] + part[g + 1][t]) + (part[g + 2][t] + part[g + 3][t]);
            Z[i * D + c] = diag * X[i * D + c] + y;
        }
        __syncthreads();
    }
}

template <int VEC, int NW>
__global__ void __launch_bounds__(64 * NW) gine_fwd_block(const float* __restrict__ X, const float* __restrict__ w, const float* __restrict__ a,
                                                         const float* __restrict__ b, float diag, int64_t N, int64_t D,
                                                         const int* __restrict__ ptr, const int* __restrict__ src,
                                                         const int* __restrict__ eid, float* __restrict__ Z) {
    __shared__ float part[NW][64 * VEC];
    gine_fwd_block_body<VEC, NW>(part, X, w, a, b, diag, D, ptr, src, eid, Z);
}

// Multi-draw forms (batched ensemble evaluation): draw d = blockIdx.y runs the single-draw workgroup body on its own arrays --
// X + d x_stride (0: one block shared by all draws), w + d nnz1, ptr + d (N + 1), src / eid + d nnz1 (nnz1 = max(nnz, 1), the row pitch of
// graph_filter_multi's arrays), Z + d N D.  Same body, same order of every column's additions: block d is bitwise the single-draw result.
template <int VEC>
__global__ void __launch_bounds__(kT) gine_fwd_wave_multi(const float* __restrict__ X, int64_t x_stride, const float* __restrict__ w,
                                                         const float* __restrict__ a, const float* __restrict__ b, float diag, int64_t N,
                                                         int64_t D, int64_t nnz1, const int* __restrict__ ptr, const int* __restrict__ src,
                                                         const int* __restrict__ eid, float* __restrict__ Z) {
    const int64_t d = blockIdx.y;
    gine_fwd_wave_body<VEC>(X + d * x_stride, w ? w + d * nnz1 : nullptr, a, b, diag, N, D, ptr + d * (N + 1), src + d * nnz1, eid + d * nnz1,
                            Z + d * N * D);
}

template <int VEC, int NW>
__global__ void __launch_bounds__(64 * NW) gine_fwd_block_multi(const float* __restrict__ X, int64_t x_stride, const float* __restrict__ w,
                                                               const float* __restrict__ a, const float* __restrict__ b, float diag,
                                                               int64_t N, int64_t D, int64_t nnz1, const int* __restrict__ ptr,
                                                               const int* __restrict__ src, const int* __restrict__ eid,
                                                               float* __restrict__ Z) {
    __shared__ float part[NW][64 * VEC];
    const int64_t d = blockIdx.y;
    gine_fwd_block_body<VEC, NW>(part, X + d * x_stride, w ? w + d * nnz1 : nullptr, a, b, diag, D, ptr + d * (N + 1), src + d * nnz1,
                                 eid + d * nnz1, Z + d * N * D);
}

// ---------------------------------------------------------------------------------------------------------------- backward
// One wave's share (entries k0, k0 + step, ... < end) of row j's chunk: acc += m, da += w m, db += m, dw[e] (+)= sum_c a m.
// Wave-uniform control flow: every lane (also one past D: in == false, all its values 0) takes part in the wave reductions.
template <int VEC>
__device__ __forceinline__ void gine_scatter(float (&acc)[VEC], float (&da)[VEC], float (&db)[VEC], const float* __restrict__ dZ,
                                             const float* __restrict__ w, const float* __restrict__ dw_add, float* dw, int64_t D, int64_t c0,
                                             bool in, bool first_chunk, const int* __restrict__ dst, const int* __restrict__ eid, int k0,
                                             int end, int step, const float (&xj)[VEC], const float (&av)[VEC], const float (&bv)[VEC]) {
    const int lane = threadIdx.x & 63;
    for (int k = k0; k < end; k += 4 * step) {
        int e[4];
        float we[4], g[4][VEC];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kk = k + u * step;
            ok[u] = kk < end;
            e[u] = ok[u] ? eid[kk] : 0;
            we[u] = (ok[u] && w) ? w[e[u]] : 1.0f;
            zerov<VEC>(g[u]);
            if (ok[u] && in) ldv<VEC>(g[u], dZ + static_cast<int64_t>(dst[kk]) * D + c0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!ok[u]) break;                      // (wave-uniform)
            float s = 0.f;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float m = gine_pre(xj[v], we[u], av[v], bv[v]) > 0.f ? g[u][v] : 0.f;
                acc[v] += m;
                db[v] += m;
                da[v] += we[u] * m;
                s += av[v] * m;
            }
            if (dw) {
                s = wave_sum_hi_dpp(s);
                if (lane == 63) dw[e[u]] = first_chunk ? (dw_add ? s + dw_add[e[u]] : s) : dw[e[u]] + s;
            }
        }
    }
}

// one wave per row; workgroup `blockIdx.x` owns rows [blockIdx.x * rows_per_block, ...) and writes one partial row of d a / d b
template <int VEC>
__global__ void __launch_bounds__(kT) gine_bwd_wave(const float* __restrict__ X, const float* __restrict__ dZ, const float* __restrict__ w,
                                                   const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ dw_add,
                                                   float diag, int64_t N, int64_t D, int64_t rows_per_block, const int* __restrict__ ptr,
                                                   const int* __restrict__ dst, const int* __restrict__ eid, float* __restrict__ dX, float* dw,
                                                   float* __restrict__ part) {
    constexpr int NWV = kT / 64;
    __shared__ float red[2][NWV][64 * VEC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
    const int64_t row1 = row0 + rows_per_block < N ? row0 + rows_per_block : N;
    for (int64_t cbase = 0; cbase < D; cbase += 64 * VEC) {
        const int64_t c0 = cbase + static_cast<int64_t>(lane) * VEC;
        const bool in = c0 < D;
        float av[VEC], bv[VEC], da[VEC], db[VEC];
        zerov<VEC>(av); zerov<VEC>(bv); zerov<VEC>(da); zerov<VEC>(db);
        if (in) { ldv<VEC>(av, a + c0); ldv<VEC>(bv, b + c0); }
        for (int64_t j = row0 + wave; j < row1; j += NWV) {
            float xj[VEC], acc[VEC];
            zerov<VEC>(xj); zerov<VEC>(acc);
            if (in) ldv<VEC>(xj, X + j * D + c0);
            gine_scatter<VEC>(acc, da, db, dZ, w, dw_add, dw, D, c0, in, cbase == 0, dst, eid, ptr[j], ptr[j + 1], 1, xj, av, bv);
            if (dX && in) {
                float gj[VEC], o[VEC];
                ldv<VEC>(gj, dZ + j * D + c0);
#pragma unroll
                for (int v = 0; v < VEC; ++v) o[v] = diag * gj[v] + acc[v];
                stv<VEC>(dX + j * D + c0, o);
            }
        }
        if (part) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) { red[0][wave][lane * VEC + v] = da[v]; red[1][wave][lane * VEC + v] = db[v]; }
            __syncthreads();
            const int t = threadIdx.x;
            if (t < 64 * VEC && cbase + t < D) {
                float* prow = part + static_cast<int64_t>(blockIdx.x) * 2 * D + cbase + t;
                prow[0] = (red[0][0][t] + red[0][1][t]) + (red[0][2][t] + red[0][3][t]);
                prow[D] = (red[1][0][t] + red[1][1][t]) + (red[1][2][t] + red[1][3][t]);
            }
            __syncthreads();
        }
    }
}

// a workgroup of NW waves per row; workgroup `blockIdx.x` owns rows blockIdx.x, blockIdx.x + gridDim.x, ...
template <int VEC, int NW>
__global__ void __launch_bounds__(64 * NW) gine_bwd_block(const float* __restrict__ X, const float* __restrict__ dZ, const float* __restrict__ w,
                                                         const float* __restrict__ a, const float* __restrict__ b,
                                                         const float* __restrict__ dw_add, float diag, int64_t N, int64_t D,
                                                         const int* __restrict__ ptr, const int* __restrict__ dst, const int* __restrict__ eid,
                                                         float* __restrict__ dX, float* dw, float* __restrict__ part) {
    __shared__ float red[NW][64 * VEC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = threadIdx.x;
    for (int64_t cbase = 0; cbase < D; cbase += 64 * VEC) {
        const int64_t c0 = cbase + static_cast<int64_t>(lane) * VEC;
        const bool in = c0 < D;
        float av[VEC], bv[VEC], da[VEC], db[VEC];
        zerov<VEC>(av); zerov<VEC>(bv); zerov<VEC>(da); zerov<VEC>(db);
        if (in) { ldv<VEC>(av, a + c0); ldv<VEC>(bv, b + c0); }
        for (int64_t j = blockIdx.x; j < N; j += gridDim.x) {
            float xj[VEC], acc[VEC];
            zerov<VEC>(xj); zerov<VEC>(acc);
            if (in) ldv<VEC>(xj, X + j * D + c0);
            gine_scatter<VEC>(acc, da, db, dZ, w, dw_add, dw, D, c0, in, cbase == 0, dst, eid, ptr[j] + wave, ptr[j + 1], NW, xj, av, bv);
            if (dX) {                               // (kernel-uniform)
#pragma unroll
                for (int v = 0; v < VEC; ++v) red[wave][lane * VEC + v] = acc[v];
                __syncthreads();
                if (t < 64 * VEC && cbase + t < D) {
                    float y = 0.f;
#pragma unroll
                    for (int g = 0; g < NW; g += 4) y += (red[g][t] + red[g + 1][t]) + (red[g + 2][t] + red[g + 3][t]);
                    dX[j * D + cbase + t] = diag * dZ[j * D + cbase + t] + y;
                }
                __syncthreads();
            }
        }
        if (part) {
            float* prow = part + static_cast<int64_t>(blockIdx.x) * 2 * D + cbase + t;
#pragma unroll
            for (int which = 0; which < 2; ++which) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) red[wave][lane * VEC + v] = which ? db[v] : da[v];
                __syncthreads();
                if (t < 64 * VEC && cbase + t < D) {
                    float y = 0.f;
#pragma unroll
                    for (int g = 0; g < NW; g += 4) y += (red[g][t] + red[g + 1][t]) + (red[g + 2][t] + red[g + 3][t]);
                    prow[which * D] = y;
                }
                __syncthreads();
            }
        }
    }
}

// d a | d b [2 D] = the sum of `nparts` partial rows, in a fixed order: 16 groups of 64 columns, group g adds rows g, g + 16, ..., then
// the 16 group sums are added as a fixed tree.  nparts == 0 writes zeros.
__global__ void __launch_bounds__(1024) gine_dab_final(const float* __restrict__ part, int64_t nparts, int64_t D, float* __restrict__ da,
                                                      float* __restrict__ db) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * 64 + lane;
    float s = 0.f;
    if (c < 2 * D)
        for (int64_t p = grp; p < nparts; p += 16) s += part[p * 2 * D + c];
    red[grp][lane] = s;
    __syncthreads();
    if (grp == 0 && c < 2 * D) {
        float y = 0.f;
#pragma unroll
        for (int g = 0; g < 16; g += 4) y += (red[g][lane] + red[g + 1][lane]) + (red[g + 2][lane] + red[g + 3][lane]);
        if (c < D) da[c] = y; else db[c - D] = y;
    }
}

inline bool aligned_to(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & static_cast<uintptr_t>(bytes - 1)) == 0; }

}  // namespace
}  // namespace sgs

using namespace sgs;

extern "C" {

/* kind * 1000 + VEC * 100 + W.  kind 0: one wave per row (W = 64 lanes); kind 1: a workgroup of W = 4 / 16 waves per row (few long rows:
 * N <= 65536 and nnz >= 16 N; 16 waves from nnz >= 256 N).  VEC: the widest of 4 / 2 / 1 with D % VEC == 0 and every dense operand
 * 4 VEC-byte aligned (`align_bytes`: what all of them are aligned to), halved while half the wave would stay idle (D <= 32 VEC). */
int sgs_gine_variant(int64_t N, int64_t D, int64_t nnz, int align_bytes) {
    int vec = (D % 4 == 0 && align_bytes >= 16) ? 4 : (D % 2 == 0 && align_bytes >= 8) ? 2 : 1;
    while (vec > 1 && D <= 32 * vec) vec /= 2;
    if (N <= 65536 && nnz >= 16 * N) return 1000 + vec * 100 + (nnz >= 256 * N ? 16 : 4);
    return vec * 100 + 64;
}

#define GINE_DISPATCH(var, WAVE_LAUNCH, BLOCK_LAUNCH)                                                    \
    switch (var) {                                                                                     \
        case 164: WAVE_LAUNCH(1); break;                                                               \
        case 264: WAVE_LAUNCH(2); break;                                                               \
        case 464: WAVE_LAUNCH(4); break;                                                               \
        case 1104: BLOCK_LAUNCH(1, 4); break;                                                          \
        case 1204: BLOCK_LAUNCH(2, 4); break;                                                          \
        case 1404: BLOCK_LAUNCH(4, 4); break;                                                          \
        case 1116: BLOCK_LAUNCH(1, 16); break;                                                         \
        case 1216: BLOCK_LAUNCH(2, 16); break;                                                         \
        case 1416: BLOCK_LAUNCH(4, 16); break;                                                         \
        default: SGS_REQUIRE(false, SGS_EINVAL, "sgs_gine_aggregate: no kernel for variant %d", var);  \
    }

static int gine_align(const void* p0, const void* p1, const void* p2, const void* p3, const void* p4) {
    const void* ps[5] = {p0, p1, p2, p3, p4};
    int al = 16;
    for (const void* p : ps)
        if (p) al = aligned_to(p, 16) ? al : (aligned_to(p, 8) ? (al < 8 ? al : 8) : 4);
    return al;
}

int sgs_gine_aggregate_fwd(const float* x, const float* edge_w, const float* a, const float* b, float diag, int64_t N, int64_t D,
                           int64_t n_edges, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, float* z,
                           sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D >= 1 && n_edges >= 0 && N <= 0x7FFFFFFF, SGS_EINVAL, "sgs_gine_aggregate_fwd: bad sizes");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(x && a && b && in_ptr && z && x != z && (n_edges == 0 || (in_src && in_eid)), SGS_EINVAL,
                "sgs_gine_aggregate_fwd: null or aliased pointer");
    const int var = sgs_gine_variant(N, D, n_edges, gine_align(x, z, a, b, nullptr));
#define FWD_WAVE(V) hipLaunchKernelGGL((gine_fwd_wave<V>), dim3(static_cast<unsigned>(cdiv(N, kT / 64))), dim3(kT), 0, stream, x, edge_w, a, b, \
                                       diag, N, D, in_ptr, in_src, in_eid, z)
#define FWD_BLOCK(V, W) hipLaunchKernelGGL((gine_fwd_block<V, W>), dim3(static_cast<unsigned>(N)), dim3(64 * W), 0, stream, x, edge_w, a, b, diag, \
                                           N, D, in_ptr, in_src, in_eid, z)
    GINE_DISPATCH(var, FWD_WAVE, FWD_BLOCK)
#undef FWD_WAVE
#undef FWD_BLOCK
    SGS_LAUNCH_OK();
    return SGS_OK;
}

/* All D draws of a pass in one launch (draw = blockIdx.y) over graph_filter_multi's draw-strided in-CSRs.  The kind / NW choice is
 * sgs_gine_variant's for (N, Dc, nnz), as a single-draw call on one draw makes it.  VEC only decides which lane owns a column, never the
 * order of a column's additions, so it may differ from a single-draw call's without changing a bit: here every draw's base address has
 * to be 4 VEC-byte aligned, i.e. the pointers AND the element strides between draws (x_stride, N Dc; the latter follows from Dc % VEC == 0
 * and is checked all the same).  An unaligned stride drops to the next narrower VEC. */
int sgs_gine_aggregate_fwd_multi(const float* x, int64_t x_stride, const float* edge_w, const float* a, const float* b, float diag, int64_t N,
                                 int64_t Dc, int64_t nnz, int64_t D, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                                 float* z, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && Dc >= 1 && nnz >= 0 && N <= 0x7FFFFFFF && nnz <= 0x7FFFFFFF && D >= 1 && D <= 65535 &&
                    (x_stride == 0 || x_stride >= N * Dc), SGS_EINVAL,
                "sgs_gine_aggregate_fwd_multi: bad sizes (need N >= 0, Dc >= 1, nnz >= 0, 1 <= D <= 65535, x_stride 0 or >= N * Dc)");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(x && a && b && in_ptr && z && (nnz == 0 || (in_src && in_eid)), SGS_EINVAL, "sgs_gine_aggregate_fwd_multi: null pointer");
    SGS_REQUIRE(x + (D - 1) * x_stride + N * Dc <= z || z + D * N * Dc <= x, SGS_EINVAL, "sgs_gine_aggregate_fwd_multi: x and z overlap");
    int al = gine_align(x, z, a, b, nullptr);
    if (D > 1)
        while (al > 4 && ((x_stride * 4) % al != 0 || (N * Dc * 4) % al != 0)) al /= 2;
    const int var = sgs_gine_variant(N, Dc, nnz, al);
    const int64_t nnz1 = nnz > 0 ? nnz : 1;
    const unsigned Du = static_cast<unsigned>(D);
#define FWD_WAVE(V) hipLaunchKernelGGL((gine_fwd_wave_multi<V>), dim3(static_cast<unsigned>(cdiv(N, kT / 64)), Du), dim3(kT), 0, stream, x, \
                                       x_stride, edge_w, a, b, diag, N, Dc, nnz1, in_ptr, in_src, in_eid, z)
#define FWD_BLOCK(V, W) hipLaunchKernelGGL((gine_fwd_block_multi<V, W>), dim3(static_cast<unsigned>(N), Du), dim3(64 * W), 0, stream, x, x_stride, \
                                           edge_w, a, b, diag, N, Dc, nnz1, in_ptr, in_src, in_eid, z)
    GINE_DISPATCH(var, FWD_WAVE, FWD_BLOCK)
#undef FWD_WAVE
#undef FWD_BLOCK
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_gine_aggregate_bwd_workspace_bytes(int64_t N, int64_t D) {
    if (N <= 0 || D <= 0) return 256;
    const int64_t parts = N < kMaxParts ? N : kMaxParts;
    return carve_bytes(static_cast<size_t>(parts) * 2 * static_cast<size_t>(D), sizeof(float));
}

int sgs_gine_aggregate_bwd(const float* x, const float* dz, const float* edge_w, const float* a, const float* b, float diag, int64_t N,
                           int64_t D, int64_t n_edges, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                           const float* dw_add, float* d_x, float* d_edge_w, float* d_a, float* d_b, void* ws, size_t ws_bytes,
                           sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE(N >= 0 && D >= 1 && n_edges >= 0 && N <= 0x7FFFFFFF, SGS_EINVAL, "sgs_gine_aggregate_bwd: bad sizes");
    SGS_REQUIRE((d_a == nullptr) == (d_b == nullptr), SGS_EINVAL, "sgs_gine_aggregate_bwd: d_a and d_b come together");
    SGS_REQUIRE(!d_a || (ws && ws_bytes >= sgs_gine_aggregate_bwd_workspace_bytes(N, D)), SGS_EINVAL,
                "sgs_gine_aggregate_bwd: workspace too small (sgs_gine_aggregate_bwd_workspace_bytes)");
    SGS_REQUIRE(!dw_add || (d_edge_w && dw_add != d_edge_w), SGS_EINVAL, "sgs_gine_aggregate_bwd: dw_add needs d_edge_w and must not alias it");
    float* part = d_a ? static_cast<float*>(ws) : nullptr;
    int64_t nparts = 0;
    if (N > 0) {
        SGS_REQUIRE(x && dz && a && b && out_ptr && (n_edges == 0 || (out_dst && out_eid)) && d_x != dz && d_x != x, SGS_EINVAL,
                    "sgs_gine_aggregate_bwd: null or aliased pointer");
        const int var = sgs_gine_variant(N, D, n_edges, gine_align(x, dz, a, b, d_x));
        if (var >= 1000) {
            const int64_t cap = (var % 100 == 16) ? kMaxParts / 4 : kMaxParts;
            nparts = N < cap ? N : cap;
#define BWD_WAVE(V) SGS_REQUIRE(false, SGS_EINVAL, "sgs_gine_aggregate_bwd: variant %d", var)
#define BWD_BLOCK(V, W) hipLaunchKernelGGL((gine_bwd_block<V, W>), dim3(static_cast<unsigned>(nparts)), dim3(64 * W), 0, stream, x, dz, edge_w, a, \
                                           b, dw_add, diag, N, D, out_ptr, out_dst, out_eid, d_x, d_edge_w, part)
            GINE_DISPATCH(var, BWD_WAVE, BWD_BLOCK)
#undef BWD_WAVE
#undef BWD_BLOCK
        } else {
            constexpr int64_t RW = kT / 64;
            const int64_t rows_per_block = cdiv(cdiv(N, RW), kMaxParts) * RW;
            nparts = cdiv(N, rows_per_block);
#define BWD_WAVE(V) hipLaunchKernelGGL((gine_bwd_wave<V>), dim3(static_cast<unsigned>(nparts)), dim3(kT), 0, stream, x, dz, edge_w, a, b, dw_add, \
                                       diag, N, D, rows_per_block, out_ptr, out_dst, out_eid, d_x, d_edge_w, part)
#define BWD_BLOCK(V, W) SGS_REQUIRE(false, SGS_EINVAL, "sgs_gine_aggregate_bwd: variant %d", var)
            GINE_DISPATCH(var, BWD_WAVE, BWD_BLOCK)
#undef BWD_WAVE
#undef BWD_BLOCK
        }
        SGS_LAUNCH_OK();
    }
    if (d_a) {
        hipLaunchKernelGGL(gine_dab_final, dim3(static_cast<unsigned>(cdiv(2 * D, 64))), dim3(1024), 0, stream, part, nparts, D, d_a, d_b);
        SGS_LAUNCH_OK();
    }
    return SGS_OK;
}

}  // extern "C"
