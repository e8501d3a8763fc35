// Host side of the CSR SpMM / SDDMM launchers (gcn.hip, cheb.hip): which kernel a shape gets, as one plan, the variant code the
// sgs_*_variant queries report, and the dispatch that turns the plan into template arguments.  Host only: no kernel lives here.
#pragma once
#include <cstdint>
#include <type_traits>

namespace sgs {

inline int pick_lpr(int64_t D, int vec) {       // the power of two >= ceil(D / vec), at most 64
    const int64_t need = (D + vec - 1) / vec;
    int lpr = 1;
    while (lpr < need && lpr < 64) lpr <<= 1;
    return lpr;
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// kind 0: a group of w lanes per row, 256-thread workgroups (w = pick_lpr).  kind 1: a workgroup of w waves per row (4 | 16).
// vec 4: 16-byte gathers.  long_rows: the <..., LONG = true> kernels (kind 1, where the kernel family has them).
struct SpmmPlan {
    int kind, vec, w;
    bool long_rows;
    int code() const { return kind * 1000 + vec * 100 + w; }      // what sgs_spmm_csr_variant and its kin return
    static SpmmPlan of_code(int code) { return SpmmPlan{code / 1000, code / 100 % 10, code % 100, false}; }
    unsigned block() const { return kind ? 64u * w : 256u; }
    unsigned blocks(int64_t N) const { return static_cast<unsigned>(kind ? N : (N + 256 / w - 1) / (256 / w)); }
};

// The row form: waves per row from 16 entries a row on average (at most max_rows rows: the grid is a workgroup per row), 16 waves
// from wide_per_row entries a row; lanes per row otherwise.
inline SpmmPlan spmm_row_form(int64_t N, int64_t D, int64_t nnz, int vec, int64_t max_rows, int64_t wide_per_row) {
    if (N <= max_rows && nnz >= 16 * N) return SpmmPlan{1, vec, nnz >= wide_per_row * N ? 16 : 4, false};
    return SpmmPlan{0, vec, pick_lpr(D, vec), false};
}
// sgs_spmm_csr's plan, shared by every GCN SpMM entry point and by the Chebyshev step: few, long rows get a workgroup each; 16 waves
// for very long rows only (at ~100 entries per row the 16-wave form measured 5 % slower).  VEC = 4 iff D % 4 == 0 and al16: both dense
// operands 16-byte aligned, with whatever pitch or stride condition the caller adds.  long_on: the long-row switch and its size
// limits, as the caller evaluated them.
constexpr int64_t kSpmmRowblockMaxRows = 65536;
inline SpmmPlan spmm_plan(int64_t N, int64_t D, int64_t nnz, bool al16, bool long_on = false) {
    SpmmPlan p = spmm_row_form(N, D, nnz, (D % 4 == 0 && al16) ? 4 : 1, kSpmmRowblockMaxRows, 256);
    p.long_rows = p.kind == 1 && long_on;
    return p;
}

// Run-time (vec, w) -> compile-time arguments: f(integral_constant<int, VEC>, integral_constant<int, W>), W from the list Ws.
template <int V> using int_c = std::integral_constant<int, V>;
template <int... Ws, class F>
inline void dispatch_vec_w(int vec, int w, F&& f) {
    const auto on_w = [&](auto V) { (void)((w == Ws && (f(V, int_c<Ws>{}), true)) || ...); };
    if (vec == 4) on_w(int_c<4>{});
    else          on_w(int_c<1>{});
}
// f(VEC, LPR) for a lanes-per-row plan; f(VEC, NW) for a waves-per-row plan; f(VEC, NW, LONG) where the kernel takes the long-row flag
template <class F> inline void dispatch_lanes(const SpmmPlan& p, F&& f) { dispatch_vec_w<1, 2, 4, 8, 16, 32, 64>(p.vec, p.w, f); }
template <class F> inline void dispatch_waves(const SpmmPlan& p, F&& f) { dispatch_vec_w<4, 16>(p.vec, p.w, f); }
template <class FR, class FB> inline void dispatch_plan(const SpmmPlan& p, FR&& rows, FB&& block) {      // whichever form p has
    if (p.kind) dispatch_waves(p, block);
    else        dispatch_lanes(p, rows);
}
template <class F> inline void dispatch_waves_long(const SpmmPlan& p, F&& f) {
    dispatch_waves(p, [&](auto V, auto W) {
        if (p.long_rows) f(V, W, std::true_type{});
        else             f(V, W, std::false_type{});
    });
}

}  // namespace sgs
