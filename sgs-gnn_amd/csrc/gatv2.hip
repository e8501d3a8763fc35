// GATv2 attention (PyG 2.3.1 GATv2Conv, share_weights = False, restated from its published algorithm) for 1 <= K <= 16 heads of C channels.
//
//   x_l = lin_l(x), x_r = lin_r(x), both [N, K C] with head-major columns; for an entry j -> i and head h
//     s[c]     = x_l[j, h, c] + x_r[i, h, c] (+ w_e le[h, c])          le = lin_edge.weight viewed [K, C], w_e the edge weight
//     logit_h  = sum_c att[h, c] leaky_relu(s[c])
//   softmax per (destination, head) over the in-entries plus one added loop (existing (i, i) entries are removed; the loop carries the mean
//   weight of its node's remaining in-edges, 0 without any), / (sum + 1e-16), attention dropout keyed as the GATConv kernels' (site, edge id,
//   head) / (site + 1, node, head).  The aggregation out_i = sum alpha x_l[j] and the SDDMM behind d alpha are sgs_spmm_csr_heads /
//   sgs_sddmm_csr_heads of gat.hip, unchanged.
//
// Unlike GATConv's logit (two node-level scalars) this one is a reduction over C channels of two gathered rows per (entry, head), so the
// softmax kernels here gather rows.  Lane layout of the two by-destination kernels = sddmm_csr_heads': LPR = KP G lanes own a row (KP = K
// rounded up to a power of two, G = a power of two <= 64 / KP lanes per head), lane (h, g) owns VEC consecutive channels of head h per chunk
// of G VEC channels, float4 when C % 4 == 0 and the pointers are 16-byte aligned.  ONE = a head's C channels fit one chunk (C <= G VEC: every
// shape the two-layer head meets up to hidden 256): x_r[i], att[h] and le[h] then stay in registers for the whole row walk.  Otherwise the
// channel chunks are walked in a loop and re-read (cache-hot) per entry.  The entries of a row are walked one per trip by the row's LPR
// lanes; the trip count is made wave-uniform so that every lane takes part in the xor-shuffles that add a head's G partial sums.
// No float atomics: every sum has a fixed order, two identical launches give identical bits.
#include <math.h>

#include <type_traits>

#include "sgs_common.h"

namespace sgs {
namespace {

constexpr int kT = 256;
constexpr int kMaxHeads = 16;
constexpr int kMaxIters = 16;       // row passes per workgroup of the backward (bounds the per-workgroup partials of d att / d le)

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : slope * v; }
// the pre-activation, written once so that forward, backward and the by-source kernel agree on its sign bit for bit
__device__ __forceinline__ float v2_pre(float xl, float xr, float w, float le) { return fmaf(w, le, xl + xr); }

template <int VEC>
__device__ __forceinline__ void ldv(float (&dst)[VEC], const float* __restrict__ p) {
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    *reinterpret_cast<V*>(dst) = *reinterpret_cast<const V*>(p);
}
template <int VEC>
__device__ __forceinline__ void zerov(float (&dst)[VEC]) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) dst[v] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// Sweep 1 (trip t = entry t of the row, the added loop as the extra trip): raw logit -> soft[eid, h] (written by lane g = t mod G of the
// head), running max and sum kept by every lane of the head; with the edge term the row's weights are summed on the way, so the loop's
// mean weight is known when its trip comes.  Sweep 2: each lane re-reads the raw logits it wrote itself, normalises, applies the dropout
// mask and writes soft / alpha; (i, i) entries get 0.
// The row walk is one body, shared by the single-draw kernel and the multi-draw eval kernel below (EVAL: no dropout, no separate soft /
// soft_loop copies, no wbar / inv_cnt outputs -- `soft` IS the alpha block then: the raw logits wait in it between the sweeps and sweep 2
// overwrites them in place; `alpha`, `soft_loop`, `wbar`, `inv_cnt` are not touched).  Everything that decides a bit of the result is
// common to both: v2_pre / lrelu, the trip order, the online max / sum, the shuffle order, 1 / (sum + 1e-16).  `soft` is read back, so
// it is not restrict here or in either kernel; a caller must never hand one buffer in as both `soft` and `alpha`.
template <int VEC, bool ONE, bool EVAL>
__device__ __forceinline__ void v2_alpha_fwd_rows(const float* xl, const float* xr, const float* att, const float* w, const float* le, int64_t N,
                                                  int K, int64_t C, const int* in_ptr, const int* in_src, const int* in_eid, float slope,
                                                  float drop_scale, uint32_t drop_thresh, int use_drop, uint64_t seed, uint32_t site, float* soft,
                                                  float* soft_loop, float* alpha, float* alpha_loop, float* wbar, float* inv_cnt, int lg, int lgG) {
    const int LPR = 1 << lg, G = 1 << lgG;
    const int sub = threadIdx.x & (LPR - 1);
    const int h = sub >> lgG, gl = sub & (G - 1);
    const bool hv = h < K;
    const int hc = hv ? h : 0;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kT >> lg) + (threadIdx.x >> lg);
    const bool live = i < N;                                  // dead rows keep their lanes in the shuffles
    const int64_t ir = live ? i : 0;
    const int64_t D = static_cast<int64_t>(K) * C;
    const bool has_w = w != nullptr;
    const bool drop = !EVAL && use_drop != 0;
    const int b = live ? in_ptr[i] : 0, deg = live ? in_ptr[i + 1] - b : 0;
    int trips = deg + 1;
    for (int o = 32; o > 0; o >>= 1) trips = max(trips, __shfl_xor(trips, o, 64));
    const float* xri = xr + ir * D + static_cast<int64_t>(hc) * C;
    const float* ah = att + static_cast<int64_t>(hc) * C;
    const float* leh = has_w ? le + static_cast<int64_t>(hc) * C : nullptr;
    const int64_t c1 = static_cast<int64_t>(gl) * VEC;
    const int64_t cstep = static_cast<int64_t>(G) * VEC;
    float r[VEC], a[VEC], l[VEC];
    zerov<VEC>(r); zerov<VEC>(a); zerov<VEC>(l);
    if (ONE && c1 < C) {
        ldv<VEC>(r, xri + c1);
        ldv<VEC>(a, ah + c1);
        if (has_w) ldv<VEC>(l, leh + c1);
    }
    float m = -INFINITY, ssum = 0.f, wsum = 0.f, cnt = 0.f, lraw = 0.f, wb = 0.f, icnt = 0.f;
    for (int t = 0; t < trips; ++t) {
        const int k = b + t;
        const bool in = live && t < deg;
        const bool is_diag = live && t == deg;
        const int s = in ? in_src[k] : static_cast<int>(ir);
        const int64_t ed = in ? in_eid[k] : 0;
        const bool is_edge = in && s != static_cast<int>(i);
        float we = 0.f;
        if (has_w) {
            if (is_edge) {
                we = w[ed];
                wsum += we;
                cnt += 1.f;
            } else if (is_diag) {
                icnt = cnt > 0.f ? 1.0f / cnt : 0.f;
                wb = wsum * icnt;
                we = wb;
            }
        }
        float acc = 0.f;
        if (is_edge || is_diag) {
            const float* xj = xl + static_cast<int64_t>(s) * D + static_cast<int64_t>(hc) * C;
            if (ONE) {
                if (c1 < C) {
                    float x[VEC];
                    ldv<VEC>(x, xj + c1);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc = fmaf(a[v], lrelu(v2_pre(x[v], r[v], we, l[v]), slope), acc);
                }
            } else {
                for (int64_t c0 = c1; c0 < C; c0 += cstep) {
                    float x[VEC], rr[VEC], aa[VEC], ll[VEC];
                    ldv<VEC>(x, xj + c0);
                    ldv<VEC>(rr, xri + c0);
                    ldv<VEC>(aa, ah + c0);
                    zerov<VEC>(ll);
                    if (has_w) ldv<VEC>(ll, leh + c0);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc = fmaf(aa[v], lrelu(v2_pre(x[v], rr[v], we, ll[v]), slope), acc);
                }
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (is_edge || is_diag) {
            const float mn = fmaxf(m, acc);
            ssum = ssum * expf(m - mn) + expf(acc - mn);
            m = mn;
        }
        if (is_edge && hv && gl == (t & (G - 1))) soft[ed * K + h] = acc;
        if (is_diag) lraw = acc;
    }
    if (live && hv) {
        const float inv = 1.0f / (ssum + 1e-16f);             // torch_geometric.utils.softmax: / (sum + 1e-16)
        for (int t = gl; t < deg; t += G) {
            const int k = b + t;
            const int s = in_src[k];
            const int64_t ed = in_eid[k];
            float sm = 0.f, al = 0.f;
            if (s != static_cast<int>(i)) {
                sm = expf(soft[ed * K + h] - m) * inv;
                al = sm;
                if (drop) al = dropout_keep_at(seed, site, static_cast<uint64_t>(ed), static_cast<uint32_t>(h), drop_thresh) ? sm * drop_scale : 0.f;
            }
            soft[ed * K + h] = sm;
            if (!EVAL) alpha[ed * K + h] = al;
        }
        if (gl == 0) {
            const float sm = expf(lraw - m) * inv;
            float al = sm;
            if (drop) al = dropout_keep_at(seed, site + 1u, static_cast<uint64_t>(i), static_cast<uint32_t>(h), drop_thresh) ? sm * drop_scale : 0.f;
            if (!EVAL) soft_loop[i * K + h] = sm;
            alpha_loop[i * K + h] = al;
        }
    }
    if (!EVAL && live && has_w && sub == 0) { wbar[i] = wb; inv_cnt[i] = icnt; }
}

template <int VEC, bool ONE>
__global__ void __launch_bounds__(kT) gatv2_alpha_heads_fwd(const float* __restrict__ xl, const float* __restrict__ xr,
                                                           const float* __restrict__ att, const float* __restrict__ w,
                                                           const float* __restrict__ le, int64_t N, int K, int64_t C,
                                                           const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                           const int* __restrict__ in_eid, float slope, float drop_scale, uint32_t drop_thresh,
                                                           int use_drop, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                           float* soft, float* __restrict__ soft_loop, float* __restrict__ alpha,
                                                           float* __restrict__ alpha_loop, float* __restrict__ wbar, float* __restrict__ inv_cnt,
                                                           int lg, int lgG) {
    seed = fold_epoch(seed, epoch);
    v2_alpha_fwd_rows<VEC, ONE, false>(xl, xr, att, w, le, N, K, C, in_ptr, in_src, in_eid, slope, drop_scale, drop_thresh, use_drop, seed, site,
                                       soft, soft_loop, alpha, alpha_loop, wbar, inv_cnt, lg, lgG);
}

// All D draws of a pass (ensemble evaluation: p = 0, forward only), draw = blockIdx.y, over graph_filter_multi's draw-strided in-CSRs
// (in_ptr [D, N + 1], in_src / in_eid [D, nnz1]).  Draw d reads xl / xr + d * xs (0: one pair shared by all draws), w + d * nnz1 by the
// draw's edge id, and writes block d of alpha [D, nnz1, K] and alpha_loop [D, N, K].  `alpha` holds the raw logits between the sweeps
// (each lane re-reads only what it wrote itself), so it is NOT restrict; no soft / soft_loop / wbar / inv_cnt exist here.
template <int VEC, bool ONE>
__global__ void __launch_bounds__(kT) gatv2_alpha_heads_fwd_multi(const float* __restrict__ xl, const float* __restrict__ xr, int64_t xs,
                                                                 const float* __restrict__ att, const float* __restrict__ w,
                                                                 const float* __restrict__ le, int64_t N, int K, int64_t C, int64_t nnz1,
                                                                 const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                                 const int* __restrict__ in_eid, float slope, float* alpha,
                                                                 float* __restrict__ alpha_loop, int lg, int lgG) {
    const int64_t d = blockIdx.y;
    v2_alpha_fwd_rows<VEC, ONE, true>(xl + d * xs, xr + d * xs, att, w ? w + d * nnz1 : nullptr, le, N, K, C, in_ptr + d * (N + 1),
                                      in_src + d * nnz1, in_eid + d * nnz1, slope, 1.0f, 0u, 0, 0, 0u, alpha + d * nnz1 * K, nullptr, nullptr,
                                      alpha_loop + d * N * K, nullptr, nullptr, lg, lgG);
}

// ---------------------------------------------------------------------------------------------------------------- backward, by destination
// Per row i and head h: the softmax / dropout backward gives g[e, h] (-> g_logit, by edge id, 0 for (i, i) entries) and the loop's g (->
// g_loop [N, K]); in the same walk s is recomputed from the gathered x_l[j] and, per channel, t = g att leaky_relu'(s):
//   d x_r[i]     = sum over the row's entries and its loop of t          (registers, stored once)
//   d att[h, c]  = sum g leaky_relu(s),   d le[h, c] = sum t w           (registers over the workgroup's `iters` row passes, the rows of a pass
//                  added through LDS in row order -> part[blockIdx.x, 2, K C]; gatv2_param_finish adds the workgroups in a fixed order)
//   d w[e]       = sum_{h, c} t le  (+ the loop's share, its own sum / cnt_i, + dw_add[e])      xor-shuffles over the row's LPR lanes
// The loop entry is taken first (its mean weight is kept from the forward), so its share of d w is known when the edges are walked.
// !ONE: the chunks of C are the outer loop (one register set per chunk) and d w, which needs all chunks of an entry, is a second walk.
template <int VEC, bool ONE>
__global__ void __launch_bounds__(kT) gatv2_alpha_heads_bwd(const float* __restrict__ xl, const float* __restrict__ xr,
                                                           const float* __restrict__ att, const float* __restrict__ w,
                                                           const float* __restrict__ le, const float* __restrict__ wbar,
                                                           const float* __restrict__ inv_cnt, int64_t N, int K, int64_t C,
                                                           const int* __restrict__ in_ptr, const int* __restrict__ in_src,
                                                           const int* __restrict__ in_eid, float slope, float drop_scale, uint32_t drop_thresh,
                                                           int use_drop, uint64_t seed, uint32_t site, const uint64_t* __restrict__ epoch,
                                                           const float* __restrict__ soft, const float* __restrict__ soft_loop,
                                                           const float* __restrict__ galpha, const float* __restrict__ gloop,
                                                           const float* __restrict__ dw_add, float* __restrict__ g_logit,
                                                           float* __restrict__ g_loop, float* __restrict__ dxr, float* __restrict__ dw,
                                                           float* __restrict__ part, int lg, int lgG, int iters) {
    __shared__ float red[2][kT * VEC];
    seed = fold_epoch(seed, epoch);
    const int LPR = 1 << lg, G = 1 << lgG;
    const int sub = threadIdx.x & (LPR - 1);
    const int h = sub >> lgG, gl = sub & (G - 1);
    const bool hv = h < K;
    const int hc = hv ? h : 0;
    const int rpp = kT >> lg, row_in_wg = threadIdx.x >> lg;
    const int64_t D = static_cast<int64_t>(K) * C;
    const bool has_w = w != nullptr;
    const float* ah = att + static_cast<int64_t>(hc) * C;
    const float* leh = has_w ? le + static_cast<int64_t>(hc) * C : nullptr;
    const int64_t c1 = static_cast<int64_t>(gl) * VEC;
    const int64_t cstep = static_cast<int64_t>(G) * VEC;
    const int nchunks = ONE ? 1 : static_cast<int>((C + cstep - 1) / cstep);

    auto dsm_edge = [&](int64_t ed) {
        float g = galpha[ed * K + hc];
        if (use_drop) g = dropout_keep_at(seed, site, static_cast<uint64_t>(ed), static_cast<uint32_t>(hc), drop_thresh) ? g * drop_scale : 0.f;
        return g;
    };
    // sum_e soft dsoft over the row's entries and its loop (every lane of the head ends with it); gL = the loop's g
    auto row_dot = [&](bool live, int64_t i, int b, int deg, float& gL) {
        float dot = 0.f;
        if (live)
            for (int t = gl; t < deg; t += G)
                if (in_src[b + t] != static_cast<int>(i)) {
                    const int64_t ed = in_eid[b + t];
                    dot += soft[ed * K + hc] * dsm_edge(ed);
                }
        for (int o = G >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
        gL = 0.f;
        if (live) {
            float gd = gloop[i * K + hc];
            if (use_drop) gd = dropout_keep_at(seed, site + 1u, static_cast<uint64_t>(i), static_cast<uint32_t>(hc), drop_thresh) ? gd * drop_scale : 0.f;
            const float sl = soft_loop[i * K + hc];
            dot += sl * gd;
            gL = hv ? sl * (gd - dot) : 0.f;                  // lanes past K add nothing anywhere
        }
        return dot;
    };
    auto row_sum = [&](float v) {                             // over the row's LPR lanes
        for (int o = LPR >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    };

    for (int chunk = 0; chunk < nchunks; ++chunk) {           // block-uniform
        const int64_t c0 = c1 + chunk * cstep;
        const bool cin = c0 < C;
        float a[VEC], l[VEC], datt[VEC], dle[VEC];
        zerov<VEC>(a); zerov<VEC>(l); zerov<VEC>(datt); zerov<VEC>(dle);
        if (cin) {
            ldv<VEC>(a, ah + c0);
            if (has_w) ldv<VEC>(l, leh + c0);
        }
        for (int it = 0; it < iters; ++it) {                  // block-uniform
            const int64_t i = (static_cast<int64_t>(blockIdx.x) * iters + it) * rpp + row_in_wg;
            const bool live = i < N;
            const int64_t ir = live ? i : 0;
            const int b = live ? in_ptr[i] : 0, deg = live ? in_ptr[i + 1] - b : 0;
            int trips = deg;
            for (int o = 32; o > 0; o >>= 1) trips = max(trips, __shfl_xor(trips, o, 64));
            float r[VEC], dr[VEC];
            zerov<VEC>(r); zerov<VEC>(dr);
            if (cin) ldv<VEC>(r, xr + ir * D + static_cast<int64_t>(hc) * C + c0);
            // one entry: gathers x_l[j]'s chunk, adds into dr / datt / dle, returns this lane's part of sum_c t le
            auto entry = [&](int64_t j, float we, float g) {
                float tl = 0.f;
                if (cin) {
                    float x[VEC];
                    ldv<VEC>(x, xl + j * D + static_cast<int64_t>(hc) * C + c0);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float s = v2_pre(x[v], r[v], we, l[v]);
                        const bool pos = s > 0.f;
                        const float t = g * a[v] * (pos ? 1.f : slope);
                        dr[v] += t;
                        datt[v] = fmaf(g, pos ? s : slope * s, datt[v]);
                        dle[v] = fmaf(t, we, dle[v]);
                        tl = fmaf(t, l[v], tl);
                    }
                }
                return tl;
            };
            float gL;
            const float dot = row_dot(live, i, b, deg, gL);
            const float wb = (has_w && live) ? wbar[i] : 0.f, icnt = (has_w && live) ? inv_cnt[i] : 0.f;
            float tloop = live ? entry(ir, wb, gL) : 0.f;
            float loop_term = 0.f;
            if (ONE && has_w) loop_term = row_sum(tloop) * icnt;
            if (live && hv && gl == 0 && chunk == 0) g_loop[i * K + h] = gL;
            for (int t = 0; t < trips; ++t) {
                const int k = b + t;
                const bool in = live && t < deg;
                const int s = in ? in_src[k] : static_cast<int>(ir);
                const int64_t ed = in ? in_eid[k] : 0;
                const bool is_edge = in && s != static_cast<int>(i);
                float g = 0.f, tl = 0.f;
                if (is_edge) {
                    if (hv) g = soft[ed * K + hc] * (dsm_edge(ed) - dot);
                    tl = entry(s, has_w ? w[ed] : 0.f, g);
                }
                if (in && hv && gl == 0 && chunk == 0) g_logit[ed * K + h] = g;
                if (ONE && has_w) {
                    tl = row_sum(tl);
                    if (in && sub == 0) {
                        const float v = is_edge ? tl + loop_term : 0.f;
                        dw[ed] = dw_add ? dw_add[ed] + v : v;
                    }
                }
            }
            if (live && hv && cin) {
                using V = typename std::conditional<VEC == 4, float4, float>::type;
                *reinterpret_cast<V*>(dxr + i * D + static_cast<int64_t>(h) * C + c0) = *reinterpret_cast<V*>(dr);
            }
        }
        // the workgroup's rows, added in row order
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            red[0][threadIdx.x * VEC + v] = datt[v];
            red[1][threadIdx.x * VEC + v] = dle[v];
        }
        __syncthreads();
        if (threadIdx.x < LPR && hv && cin) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float sa = 0.f, sl = 0.f;
                for (int rr = 0; rr < rpp; ++rr) {
                    sa += red[0][(rr * LPR + sub) * VEC + v];
                    sl += red[1][(rr * LPR + sub) * VEC + v];
                }
                float* p = part + static_cast<int64_t>(blockIdx.x) * 2 * D + static_cast<int64_t>(h) * C + c0 + v;
                p[0] = sa;
                p[D] = sl;
            }
        }
        __syncthreads();
    }

    if (!ONE && has_w) {                                      // d w needs all chunks of an entry: a walk of its own
        auto tl_full = [&](int64_t j, int64_t i, float we, float g) {
            float tl = 0.f;
            for (int64_t c0 = c1; c0 < C; c0 += cstep) {
                float x[VEC], rr[VEC], aa[VEC], ll[VEC];
                ldv<VEC>(x, xl + j * D + static_cast<int64_t>(hc) * C + c0);
                ldv<VEC>(rr, xr + i * D + static_cast<int64_t>(hc) * C + c0);
                ldv<VEC>(aa, ah + c0);
                ldv<VEC>(ll, leh + c0);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float s = v2_pre(x[v], rr[v], we, ll[v]);
                    tl = fmaf(g * aa[v] * (s > 0.f ? 1.f : slope), ll[v], tl);
                }
            }
            return tl;
        };
        for (int it = 0; it < iters; ++it) {
            const int64_t i = (static_cast<int64_t>(blockIdx.x) * iters + it) * rpp + row_in_wg;
            const bool live = i < N;
            const int64_t ir = live ? i : 0;
            const int b = live ? in_ptr[i] : 0, deg = live ? in_ptr[i + 1] - b : 0;
            int trips = deg;
            for (int o = 32; o > 0; o >>= 1) trips = max(trips, __shfl_xor(trips, o, 64));
            float gL;
            const float dot = row_dot(live, i, b, deg, gL);
            const float wb = live ? wbar[i] : 0.f, icnt = live ? inv_cnt[i] : 0.f;
            const float loop_term = row_sum(live ? tl_full(ir, ir, wb, gL) : 0.f) * icnt;
            for (int t = 0; t < trips; ++t) {
                const int k = b + t;
                const bool in = live && t < deg;
                const int s = in ? in_src[k] : static_cast<int>(ir);
                const int64_t ed = in ? in_eid[k] : 0;
                const bool is_edge = in && s != static_cast<int>(i);
                float tl = 0.f;
                if (is_edge && hv) tl = tl_full(s, ir, w[ed], soft[ed * K + hc] * (dsm_edge(ed) - dot));
                tl = row_sum(tl);
                if (in && sub == 0) {
                    const float v = is_edge ? tl + loop_term : 0.f;
                    dw[ed] = dw_add ? dw_add[ed] + v : v;
                }
            }
        }
    }
}

// d att [D] = columns 0 .. D - 1, d le [D] = columns D .. 2 D - 1 of part [nwg, 2 D], workgroups added in a fixed order: thread (g, lane)
// adds rows g, g + 16, ... of its column and the 16 groups are then added in order.
__global__ void __launch_bounds__(1024) gatv2_param_finish(const float* __restrict__ part, int nwg, int64_t D, float* __restrict__ datt,
                                                          float* __restrict__ dle) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * 64 + lane;
    const bool ok = c < 2 * D;
    float acc = 0.f;
    if (ok)
        for (int r = g; r < nwg; r += 16) acc += part[static_cast<int64_t>(r) * 2 * D + c];
    red[g][lane] = acc;
    __syncthreads();
    if (g == 0 && ok) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[k][lane];
        if (c < D) datt[c] = s;
        else if (dle) dle[c - D] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward, by source
// d x_l[j, h, c] (+)= sum over j's out-entries (j -> i, src-CSR order; (j, j) entries skipped) of g_logit[e, h] att[h, c] leaky_relu'(s)
//                     + the loop's term, s recomputed from the lane's own x_l[j] columns and the gathered x_r[i].  Lane layout of
// spmm_csr_heads: LPR lanes own a row, VEC consecutive columns each; nothing is reduced across lanes.
template <int VEC>
__global__ void __launch_bounds__(kT) gatv2_dxl_heads(const float* __restrict__ xl, const float* __restrict__ xr, const float* __restrict__ att,
                                                     const float* __restrict__ w, const float* __restrict__ le, const float* __restrict__ wbar,
                                                     const float* __restrict__ g_logit, const float* __restrict__ g_loop, int64_t N, int K,
                                                     int64_t C, const int* __restrict__ ptr, const int* __restrict__ dst,
                                                     const int* __restrict__ eid, float slope, int accumulate, float* dxl, int lg) {
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const int LPR = 1 << lg;
    const int sub = threadIdx.x & (LPR - 1);
    const int64_t j = static_cast<int64_t>(blockIdx.x) * (kT >> lg) + (threadIdx.x >> lg);
    if (j >= N) return;
    const int64_t D = static_cast<int64_t>(K) * C;
    const bool has_w = w != nullptr;
    const int b = ptr[j], e = ptr[j + 1];
    const float wb = has_w ? wbar[j] : 0.f;
    for (int64_t c0 = static_cast<int64_t>(sub) * VEC; c0 < D; c0 += static_cast<int64_t>(LPR) * VEC) {
        const int h = static_cast<int>(c0 / C);
        float x[VEC], a[VEC], l[VEC], acc[VEC];
        ldv<VEC>(x, xl + j * D + c0);
        ldv<VEC>(a, att + c0);
        zerov<VEC>(l);
        if (has_w) ldv<VEC>(l, le + c0);
        zerov<VEC>(acc);
        for (int k = b; k < e; ++k) {
            const int i = dst[k];
            if (i == static_cast<int>(j)) continue;
            const int64_t ed = eid[k];
            const float g = g_logit[ed * K + h];
            const float we = has_w ? w[ed] : 0.f;
            float r[VEC];
            ldv<VEC>(r, xr + static_cast<int64_t>(i) * D + c0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] += g * a[v] * (v2_pre(x[v], r[v], we, l[v]) > 0.f ? 1.f : slope);
        }
        {
            const float g = g_loop[j * K + h];
            float r[VEC];
            ldv<VEC>(r, xr + j * D + c0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] += g * a[v] * (v2_pre(x[v], r[v], wb, l[v]) > 0.f ? 1.f : slope);
        }
        if (accumulate) {
            float o[VEC];
            *reinterpret_cast<V*>(o) = *reinterpret_cast<const V*>(dxl + j * D + c0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] += o[v];
        }
        *reinterpret_cast<V*>(dxl + j * D + c0) = *reinterpret_cast<V*>(acc);
    }
}

inline int log2_ceil(int64_t v) {
    int l = 0;
    while ((int64_t(1) << l) < v) ++l;
    return l;
}
inline bool heads_ok(int64_t K, int64_t C) { return K >= 1 && K <= kMaxHeads && C >= 1 && C <= (int64_t(1) << 24); }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// lane geometry of the by-destination kernels for (K, C) and a vector width
struct Geom {
    int vec, lgG, lg, iters;
    bool one;
};
inline Geom geom(int64_t N, int64_t K, int64_t C, int vec) {
    Geom g;
    g.vec = vec;
    const int lgK = log2_ceil(K);
    g.lgG = log2_ceil(cdiv(C, vec));
    if (g.lgG > 6 - lgK) g.lgG = 6 - lgK;
    g.lg = lgK + g.lgG;
    g.one = (static_cast<int64_t>(vec) << g.lgG) >= C;
    const int64_t passes = cdiv(N > 0 ? N : 1, kT >> g.lg);
    int64_t it = passes / 2048;                               // about 2048 workgroups once there are rows enough
    g.iters = static_cast<int>(it < 1 ? 1 : (it > kMaxIters ? kMaxIters : it));
    return g;
}

// The launch choice of every entry point (sgs_gatv2_variant's code, see include/sgs_hip.h), taken apart again: the launchers and the
// workspace query decode the query's result instead of deciding anything themselves.
struct V2Choice {
    int kind, vec, lg, lgG, iters;
    bool one;
    explicit V2Choice(int code)
        : kind(code / 1000000), vec(code / 100000 % 10), lg(code / 10000 % 10), lgG(code / 1000 % 10), iters(code % 100), one(code / 100 % 10 != 0) {}
    int64_t passes(int64_t N) const { return cdiv(N > 0 ? N : 1, kT >> lg); }            // row passes of kT >> lg rows each
    int64_t nwg(int64_t N) const { return cdiv(passes(N), iters > 0 ? iters : 1); }     // workgroups of the backward
};

}  // namespace
}  // namespace sgs

using namespace sgs;

extern "C" {

int sgs_gatv2_variant(int op, int64_t N, int64_t K, int64_t C, int aligned16) {
    if (op < SGS_GATV2_OP_ALPHA_FWD || op > SGS_GATV2_OP_DXL || N < 0 || !heads_ok(K, C)) return -1;
    const int vec = (C % 4 == 0 && aligned16) ? 4 : 1;
    if (op == SGS_GATV2_OP_DXL) {
        int lg = log2_ceil(cdiv(K * C, vec));
        if (lg > 6) lg = 6;
        return 3000000 + vec * 100000 + lg * 10000;
    }
    const Geom g = geom(N, K, C, vec);
    return (op + 1) * 1000000 + vec * 100000 + g.lg * 10000 + g.lgG * 1000 + (g.one ? 100 : 0) + (op == SGS_GATV2_OP_ALPHA_BWD ? g.iters : 0);
}

#define SGS_REQUIRE_HEADS(name)                                                                                         \
    SGS_REQUIRE(heads_ok(K, C), SGS_EINVAL, name ": unsupported heads = %lld x channels = %lld (1 <= heads <= 16, channels >= 1)", \
                static_cast<long long>(K), static_cast<long long>(C))

int sgs_gatv2_alpha_heads_fwd(const float* xl, const float* xr, const float* att, const float* edge_w, const float* lin_edge, int64_t N,
                              int64_t K, int64_t C, int64_t n_edges, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                              float negative_slope, float p_drop, uint64_t seed, uint32_t site, float* soft, float* soft_loop, float* alpha,
                              float* alpha_loop, float* loop_w, float* loop_inv_cnt, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_gatv2_alpha_heads_fwd");
    SGS_REQUIRE(N >= 0 && N < (int64_t(1) << 31) && n_edges >= 0 && n_edges < (int64_t(1) << 31) && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL,
                "sgs_gatv2_alpha_heads_fwd: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(xl && xr && att && in_ptr && soft_loop && alpha_loop && (n_edges == 0 || (in_src && in_eid && soft && alpha)), SGS_EINVAL,
                "sgs_gatv2_alpha_heads_fwd: null pointer");
    SGS_REQUIRE(!edge_w || (lin_edge && loop_w && loop_inv_cnt), SGS_EINVAL,
                "sgs_gatv2_alpha_heads_fwd: null pointer (edge_w needs lin_edge, loop_w and loop_inv_cnt)");
    const V2Choice g(sgs_gatv2_variant(SGS_GATV2_OP_ALPHA_FWD, N, K, C, al16(xl) && al16(xr) && al16(att) && (!edge_w || al16(lin_edge))));
    const bool v4 = g.vec == 4;
    const dim3 grid(static_cast<unsigned>(g.passes(N)));
#define SGS_V2_FWD_ARGS                                                                                                              \
    xl, xr, att, edge_w, lin_edge, N, static_cast<int>(K), C, in_ptr, in_src, in_eid, negative_slope, 1.0f / (1.0f - p_drop),       \
        dropout_thresh(p_drop), p_drop > 0.f ? 1 : 0, seed, site, epoch_ptr(), soft, soft_loop, alpha, alpha_loop, loop_w, loop_inv_cnt, g.lg, g.lgG
    if (v4) {
        if (g.one) hipLaunchKernelGGL((gatv2_alpha_heads_fwd<4, true>), grid, dim3(kT), 0, stream, SGS_V2_FWD_ARGS);
        else       hipLaunchKernelGGL((gatv2_alpha_heads_fwd<4, false>), grid, dim3(kT), 0, stream, SGS_V2_FWD_ARGS);
    } else {
        if (g.one) hipLaunchKernelGGL((gatv2_alpha_heads_fwd<1, true>), grid, dim3(kT), 0, stream, SGS_V2_FWD_ARGS);
        else       hipLaunchKernelGGL((gatv2_alpha_heads_fwd<1, false>), grid, dim3(kT), 0, stream, SGS_V2_FWD_ARGS);
    }
#undef SGS_V2_FWD_ARGS
    SGS_LAUNCH_OK();
    return SGS_OK;
}

// The vector width (float4 / scalar) changes which channels a lane sums and so the bits of a logit: block d has to take the variant a
// single-draw call on that block takes.  Hence x_stride is 0 or exactly N K C: with C % 4 == 0 every draw's block then starts at the
// base pointer's alignment (N K C floats are a multiple of 16 bytes), so one al16() of the bases decides for all draws, as it does for
// the single-draw launcher; any other stride is refused rather than silently given another variant.
int sgs_gatv2_alpha_heads_fwd_multi(const float* xl, const float* xr, int64_t x_stride, const float* att, const float* edge_w,
                                    const float* lin_edge, int64_t N, int64_t K, int64_t C, int64_t D, int64_t nnz, const int32_t* in_ptr,
                                    const int32_t* in_src, const int32_t* in_eid, float negative_slope, float* alpha, float* alpha_loop,
                                    sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_gatv2_alpha_heads_fwd_multi");
    SGS_REQUIRE(N >= 0 && N < (int64_t(1) << 31) && nnz >= 0 && nnz < (int64_t(1) << 31) && D >= 1 && D <= 65535, SGS_EINVAL,
                "sgs_gatv2_alpha_heads_fwd_multi: bad sizes (need 0 <= N, nnz < 2^31 and 1 <= D <= 65535)");
    SGS_REQUIRE(x_stride == 0 || x_stride == N * K * C, SGS_EINVAL,
                "sgs_gatv2_alpha_heads_fwd_multi: x_stride = %lld: need 0 (one shared [N, K C] pair) or N K C = %lld (dense per-draw blocks)",
                static_cast<long long>(x_stride), static_cast<long long>(N * K * C));
    SGS_REQUIRE(!edge_w || lin_edge, SGS_EINVAL, "sgs_gatv2_alpha_heads_fwd_multi: null pointer (edge_w needs lin_edge)");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(xl && xr && att && in_ptr && alpha_loop && (nnz == 0 || (in_src && in_eid && alpha)), SGS_EINVAL,
                "sgs_gatv2_alpha_heads_fwd_multi: null pointer");
    const V2Choice g(sgs_gatv2_variant(SGS_GATV2_OP_ALPHA_FWD, N, K, C, al16(xl) && al16(xr) && al16(att) && (!edge_w || al16(lin_edge))));
    const dim3 grid(static_cast<unsigned>(g.passes(N)), static_cast<unsigned>(D));
    const int64_t nnz1 = nnz > 0 ? nnz : 1;
#define SGS_V2_FWD_MULTI_ARGS                                                                                                        \
    xl, xr, x_stride, att, edge_w, lin_edge, N, static_cast<int>(K), C, nnz1, in_ptr, in_src, in_eid, negative_slope, alpha, alpha_loop, g.lg, g.lgG
    if (g.vec == 4) {
        if (g.one) hipLaunchKernelGGL((gatv2_alpha_heads_fwd_multi<4, true>), grid, dim3(kT), 0, stream, SGS_V2_FWD_MULTI_ARGS);
        else       hipLaunchKernelGGL((gatv2_alpha_heads_fwd_multi<4, false>), grid, dim3(kT), 0, stream, SGS_V2_FWD_MULTI_ARGS);
    } else {
        if (g.one) hipLaunchKernelGGL((gatv2_alpha_heads_fwd_multi<1, true>), grid, dim3(kT), 0, stream, SGS_V2_FWD_MULTI_ARGS);
        else       hipLaunchKernelGGL((gatv2_alpha_heads_fwd_multi<1, false>), grid, dim3(kT), 0, stream, SGS_V2_FWD_MULTI_ARGS);
    }
#undef SGS_V2_FWD_MULTI_ARGS
    SGS_LAUNCH_OK();
    return SGS_OK;
}

size_t sgs_gatv2_alpha_heads_bwd_workspace_bytes(int64_t N, int64_t K, int64_t C) {
    if (N < 0) N = 0;
    if (!heads_ok(K, C)) return 256;
    // the vector width is chosen from the pointers at launch: room for either
    int64_t nwg = V2Choice(sgs_gatv2_variant(SGS_GATV2_OP_ALPHA_BWD, N, K, C, 0)).nwg(N);
    const int64_t n4 = V2Choice(sgs_gatv2_variant(SGS_GATV2_OP_ALPHA_BWD, N, K, C, 1)).nwg(N);
    if (n4 > nwg) nwg = n4;
    return static_cast<size_t>(nwg) * 2 * static_cast<size_t>(K * C) * 4 + 256;
}

int sgs_gatv2_alpha_heads_bwd(const float* xl, const float* xr, const float* att, const float* edge_w, const float* lin_edge, const float* loop_w,
                              const float* loop_inv_cnt, int64_t N, int64_t K, int64_t C, int64_t n_edges, const int32_t* in_ptr,
                              const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed, uint32_t site,
                              const float* soft, const float* soft_loop, const float* galpha, const float* gloop, const float* dw_add,
                              float* g_logit, float* g_loop, float* d_xr, float* d_att, float* d_lin_edge, float* d_edge_w, void* ws,
                              size_t ws_bytes, sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_gatv2_alpha_heads_bwd");
    SGS_REQUIRE(N >= 0 && N < (int64_t(1) << 31) && n_edges >= 0 && n_edges < (int64_t(1) << 31) && p_drop >= 0.f && p_drop < 1.f, SGS_EINVAL,
                "sgs_gatv2_alpha_heads_bwd: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(xl && xr && att && in_ptr && soft_loop && gloop && g_loop && d_xr && d_att &&
                    (n_edges == 0 || (in_src && in_eid && soft && galpha && g_logit)),
                SGS_EINVAL, "sgs_gatv2_alpha_heads_bwd: null pointer");
    SGS_REQUIRE(!edge_w || (lin_edge && loop_w && loop_inv_cnt && d_lin_edge && d_edge_w), SGS_EINVAL,
                "sgs_gatv2_alpha_heads_bwd: null pointer (edge_w needs lin_edge, loop_w, loop_inv_cnt, d_lin_edge and d_edge_w)");
    SGS_REQUIRE(ws && ws_bytes >= sgs_gatv2_alpha_heads_bwd_workspace_bytes(N, K, C), SGS_EWORKSPACE,
                "sgs_gatv2_alpha_heads_bwd: workspace too small");
    const V2Choice g(sgs_gatv2_variant(SGS_GATV2_OP_ALPHA_BWD, N, K, C,
                                       al16(xl) && al16(xr) && al16(att) && al16(d_xr) && (!edge_w || al16(lin_edge))));
    const bool v4 = g.vec == 4;
    const int64_t nwg = g.nwg(N);
    const dim3 grid(static_cast<unsigned>(nwg));
    float* part = static_cast<float*>(ws);
#define SGS_V2_BWD_ARGS                                                                                                              \
    xl, xr, att, edge_w, lin_edge, loop_w, loop_inv_cnt, N, static_cast<int>(K), C, in_ptr, in_src, in_eid, negative_slope,         \
        1.0f / (1.0f - p_drop), dropout_thresh(p_drop), p_drop > 0.f ? 1 : 0, seed, site, epoch_ptr(), soft, soft_loop, galpha, gloop, dw_add,  \
        g_logit, g_loop, d_xr, d_edge_w, part, g.lg, g.lgG, g.iters
    if (v4) {
        if (g.one) hipLaunchKernelGGL((gatv2_alpha_heads_bwd<4, true>), grid, dim3(kT), 0, stream, SGS_V2_BWD_ARGS);
        else       hipLaunchKernelGGL((gatv2_alpha_heads_bwd<4, false>), grid, dim3(kT), 0, stream, SGS_V2_BWD_ARGS);
    } else {
        if (g.one) hipLaunchKernelGGL((gatv2_alpha_heads_bwd<1, true>), grid, dim3(kT), 0, stream, SGS_V2_BWD_ARGS);
        else       hipLaunchKernelGGL((gatv2_alpha_heads_bwd<1, false>), grid, dim3(kT), 0, stream, SGS_V2_BWD_ARGS);
    }
#undef SGS_V2_BWD_ARGS
    const int64_t D = K * C;
    hipLaunchKernelGGL(gatv2_param_finish, dim3(static_cast<unsigned>(cdiv(2 * D, 64))), dim3(1024), 0, stream, part, static_cast<int>(nwg), D,
                       d_att, edge_w ? d_lin_edge : nullptr);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

int sgs_gatv2_dxl_heads(const float* xl, const float* xr, const float* att, const float* edge_w, const float* lin_edge, const float* loop_w,
                        const float* g_logit, const float* g_loop, int64_t N, int64_t K, int64_t C, int64_t nnz, const int32_t* out_ptr,
                        const int32_t* out_dst, const int32_t* out_eid, float negative_slope, int accumulate, float* d_xl,
                        sgs_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SGS_REQUIRE_HEADS("sgs_gatv2_dxl_heads");
    SGS_REQUIRE(N >= 0 && N < (int64_t(1) << 31) && nnz >= 0 && nnz < (int64_t(1) << 31), SGS_EINVAL, "sgs_gatv2_dxl_heads: bad arguments");
    if (N == 0) return SGS_OK;
    SGS_REQUIRE(xl && xr && att && g_loop && out_ptr && d_xl && d_xl != xl && d_xl != xr && (nnz == 0 || (out_dst && out_eid && g_logit)),
                SGS_EINVAL, "sgs_gatv2_dxl_heads: null or aliased pointer");
    SGS_REQUIRE(!edge_w || (lin_edge && loop_w), SGS_EINVAL, "sgs_gatv2_dxl_heads: null pointer (edge_w needs lin_edge and loop_w)");
    const V2Choice ch(sgs_gatv2_variant(SGS_GATV2_OP_DXL, N, K, C,
                                        al16(xl) && al16(xr) && al16(att) && al16(d_xl) && (!edge_w || al16(lin_edge))));
    const bool v4 = ch.vec == 4;
    const int lg = ch.lg;
    const dim3 grid(static_cast<unsigned>(cdiv(N, kT >> lg)));
    if (v4)
        hipLaunchKernelGGL((gatv2_dxl_heads<4>), grid, dim3(kT), 0, stream, xl, xr, att, edge_w, lin_edge, loop_w, g_logit, g_loop, N,
                           static_cast<int>(K), C, out_ptr, out_dst, out_eid, negative_slope, accumulate, d_xl, lg);
    else
        hipLaunchKernelGGL((gatv2_dxl_heads<1>), grid, dim3(kT), 0, stream, xl, xr, att, edge_w, lin_edge, loop_w, g_logit, g_loop, N,
                           static_cast<int>(K), C, out_ptr, out_dst, out_eid, negative_slope, accumulate, d_xl, lg);
    SGS_LAUNCH_OK();
    return SGS_OK;
}

}  // extern "C"
