// The endpoint reduction's three traversals as templates over a "term" policy (users: csrc/edge_score.hip, csrc/losses.hip).
//
//   out[v,:] = finish( sum_{k in out-row v} sgn_out * term(out entry k)  +  sum_{k in in-row v} sgn_in * term(in entry k) )
//
// Scatter of per-edge gradient rows to both endpoints as a deterministic gather over the two CSR orientations of the active edge list
// (no float atomics).  The policy decides what a term IS: EpLoadRows reads it from a materialised [nnz, H] array (sgs_endpoint_reduce);
// the hybrid loss's policy (csrc/losses.hip) forms it from two rows of the logits table and four per-edge scalars and adds the cross
// entropy's gradient in `finish` (sgs_hybrid_loss_fused_bwd).  Entry order, the four-in-flight grouping and the part[g] tree belong to
// the templates, so two policies that produce the same terms produce the same sums, bit for bit.
//
// A policy P provides
//   kCol, kVisit            does a term need the entry's other endpoint / is `visit` more than a no-op
//   Blk  block_init()       once per workgroup, by EVERY thread, before any thread leaves (may synchronise)
//   Own  own(v, H, c0)      what the node itself contributes to its terms at columns c0 .. c0 + VEC - 1
//   Pre  preload(e_lane, lane)             loads shared among the lanes: lane l holds the edge id of the entry in flight l & 3
//   Raw  load(pre, u, isout, e, col, H, c0)   every other global load of entry u in flight (all issued before the first use)
//   void term(blk, raw, own, isout, m, t)  the entry's factors: the sum takes fmaf(sgn * m[j], t[j], acc[j])
//   void visit(blk, v, e, col)             once per OUT entry of v, one entry per thread, before the sums (every edge is in one out-row)
//   float finish(blk, v, c, sum)           the value stored at out[v, c]
#pragma once
#include <type_traits>

#include "sgs_common.h"

namespace sgs {
namespace {

constexpr int kEpT = 256;

// Which traversal a (nnz, N) takes: 0 = a wave per node (nnz < 8 N), 4 / 16 = a workgroup of that many waves per node -- long rows
// (partitions, and whole graphs of average degree >= 8); a power-law partition has hub nodes with thousands of incident sampled edges,
// and with 4 waves those few workgroups set the kernel's duration, hence 16 from nnz >= 64 N on.
inline int ep_traversal(int64_t nnz, int64_t N) { return nnz >= 64 * N ? 16 : (nnz >= 8 * N ? 4 : 0); }

// term = Mo[eid,:] (out entries) / Mi[eid,:] (in entries), times T[other endpoint,:] with HAS_T
template <int VEC, bool HAS_T>
struct EpLoadRows {
    static constexpr bool kCol = HAS_T, kVisit = false;
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const float* __restrict__ Mo;
    const float* __restrict__ Mi;
    const float* __restrict__ T;
    struct Blk {};
    struct Own {};
    struct Pre {};
    struct Raw { float m[VEC], t[VEC]; };
    __device__ __forceinline__ Blk block_init() const { return Blk{}; }
    __device__ __forceinline__ Own own(int64_t, int64_t, int64_t) const { return Own{}; }
    __device__ __forceinline__ Pre preload(int, int) const { return Pre{}; }
    __device__ __forceinline__ Raw load(const Pre&, int, bool isout, int e, int col, int64_t H, int64_t c0) const {
        Raw r;
        *reinterpret_cast<V*>(r.m) = *reinterpret_cast<const V*>((isout ? Mo : Mi) + static_cast<int64_t>(e) * H + c0);
        if (HAS_T) *reinterpret_cast<V*>(r.t) = *reinterpret_cast<const V*>(T + static_cast<int64_t>(col) * H + c0);
        else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) r.t[j] = 1.f;
        }
        return r;
    }
    __device__ __forceinline__ void term(const Blk&, const Raw& r, const Own&, bool, float (&m)[VEC], float (&t)[VEC]) const {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { m[j] = r.m[j]; t[j] = r.t[j]; }
    }
    __device__ __forceinline__ void visit(const Blk&, int64_t, int, int) const {}
    __device__ __forceinline__ float finish(const Blk&, int64_t, int64_t, float sum) const { return sum; }
};

// One wave per node: out-row then in-row, one entry at a time.
template <int VEC, class P>
__global__ void __launch_bounds__(kEpT) endpoint_reduce(const P p, int64_t N, int64_t H, const int* __restrict__ in_ptr,
                                                       const int* __restrict__ in_src, const int* __restrict__ in_eid,
                                                       const int* __restrict__ out_ptr, const int* __restrict__ out_dst,
                                                       const int* __restrict__ out_eid, float sgn_out, float sgn_in, float* __restrict__ out) {
    const typename P::Blk blk = p.block_init();
    const int lane = threadIdx.x & 63;
    const int64_t v = (static_cast<int64_t>(blockIdx.x) * kEpT + threadIdx.x) >> 6;   // one wave per node
    if (v >= N) return;
    if (P::kVisit)
        for (int k = out_ptr[v] + lane; k < out_ptr[v + 1]; k += 64) p.visit(blk, v, out_eid[k], out_dst[k]);
    for (int64_t cbase = 0; cbase < H; cbase += 64 * VEC) {
        // every lane walks the rows (a lane past the last column on the block's first column, its sums unused): `preload` may share an
        // entry's words among the lanes of the wave
        const int64_t c0 = cbase + static_cast<int64_t>(lane) * VEC;
        const int64_t cl = c0 < H ? c0 : cbase;
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
        const typename P::Own own = p.own(v, H, cl);
        for (int dir = 0; dir < 2; ++dir) {
            const int* ptr = dir == 0 ? out_ptr : in_ptr;
            const int* col = dir == 0 ? out_dst : in_src;
            const int* eid = dir == 0 ? out_eid : in_eid;
            const float sg = dir == 0 ? sgn_out : sgn_in;
            const int b = ptr[v], e = ptr[v + 1];
            for (int k = b; k < e; ++k) {
                const int ek = eid[k], ck = P::kCol ? col[k] : 0;
                const typename P::Pre pre = p.preload(ek, lane);
                const typename P::Raw raw = p.load(pre, 0, dir == 0, ek, ck, H, cl);
                float m[VEC], t[VEC];
                p.term(blk, raw, own, dir == 0, m, t);
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[j] = fmaf(sg * m[j], t[j], acc[j]);
            }
        }
        if (c0 < H) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] = p.finish(blk, v, c0 + j, acc[j]);
            if (VEC == 4) *reinterpret_cast<float4*>(out + v * H + c0) = *reinterpret_cast<float4*>(acc);
            else out[v * H + c0] = acc[0];
        }
    }
}

// Small-N variant: a workgroup of NW waves per node; the node's out-row then in-row entries form one list that the waves stride with
// four independent entries in flight each; partial sums meet in LDS in a fixed order (deterministic).  NW: ep_traversal.
// The four entries' indices are ONE load (lane l reads entry l & 3's) handed round with v_readlane, not four loads of one address each;
// `preload` gets the per-lane edge id so that a policy can fetch per-edge words the same way.
template <int VEC, int NW, class P>
__global__ void __launch_bounds__(64 * NW) endpoint_reduce_rowblock(const P p, int64_t N, int64_t H, const int* __restrict__ in_ptr,
                                                                   const int* __restrict__ in_src, const int* __restrict__ in_eid,
                                                                   const int* __restrict__ out_ptr, const int* __restrict__ out_dst,
                                                                   const int* __restrict__ out_eid, float sgn_out, float sgn_in,
                                                                   float* __restrict__ out) {
    __shared__ float part[NW][64 * VEC];
    const typename P::Blk blk = p.block_init();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t v = blockIdx.x;
    const int ob = out_ptr[v], no = out_ptr[v + 1] - ob;
    const int ib = in_ptr[v], ni = in_ptr[v + 1] - ib;
    const int total = no + ni;
    if (P::kVisit)
        for (int k = threadIdx.x; k < no; k += 64 * NW) p.visit(blk, v, out_eid[ob + k], out_dst[ob + k]);
    for (int64_t cbase = 0; cbase < H; cbase += 64 * VEC) {
        // every lane walks the rows (a lane past the last column on the block's first column, its sums unused)
        const int64_t c0 = cbase + static_cast<int64_t>(lane) * VEC;
        const int64_t cl = c0 < H ? c0 : cbase;
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
        const typename P::Own own = p.own(v, H, cl);
        for (int k0 = wave; k0 < total; k0 += 4 * NW) {
            // indices first, then every entry's loads, all unconditional (entries past the row: clamped to its last entry, sign 0) --
            // under `if (k < total)` each entry's index wait (vmcnt(0)) also waited for the previous entry's rows
            float sg[4];
            int er[4], cr[4];
            bool io[4];
            typename P::Raw raw[4];
            const int kl = k0 + NW * (lane & 3);
            const int kcl = kl < total ? kl : total - 1;
            const bool iol = kcl < no;
            const int idl = iol ? ob + kcl : ib + (kcl - no);
            const int el = (iol ? out_eid : in_eid)[idl];
            const int cll = P::kCol ? (iol ? out_dst : in_src)[idl] : 0;
            const typename P::Pre pre = p.preload(el, lane);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + NW * u;
                const int kc = k < total ? k : total - 1;
                const bool isout = kc < no;
                er[u] = __builtin_amdgcn_readlane(el, u);
                cr[u] = P::kCol ? __builtin_amdgcn_readlane(cll, u) : 0;
                io[u] = isout;
                sg[u] = k < total ? (isout ? sgn_out : sgn_in) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) raw[u] = p.load(pre, u, io[u], er[u], cr[u], H, cl);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float m[VEC], t[VEC];
                p.term(blk, raw[u], own, io[u], m, t);
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[j] = fmaf(sg[u] * m[j], t[j], acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) part[wave][lane * VEC + j] = acc[j];
        __syncthreads();
        const int tt = threadIdx.x;
        if (tt < 64 * VEC && cbase + tt < H) {
            float sum = 0.f;
#pragma unroll
            for (int g = 0; g < NW; g += 4) sum += (part[g][tt] + part[g + 1][tt]) + (part[g + 2][tt] + part[g + 3][tt]);
            out[v * H + cbase + tt] = p.finish(blk, v, cbase + tt, sum);
        }
        __syncthreads();
    }
}

}  // namespace
}  // namespace sgs
