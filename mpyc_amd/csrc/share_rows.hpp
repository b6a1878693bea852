// share_rows.hpp -- the sub-share rows of the "apply" end of a secure round.  Included by kernels.hpp before sort.hpp.
//
// A round re-shares a local product; what a party receives are nrows sub-share rows in the compact index of the round.  The
// apply kernel of the round (k_cx_apply, k_carry_apply, k_tour_select, k_tour_unit_expand, k_find_leaf_apply,
// k_trunc_finish, k_norm_apply) recombines them with the Lagrange vector,  v = sum_j lam[j] rows[j][c],  in registers and
// folds v into its own output: the recombination never goes to memory.  The rows are read once: non-temporal loads.
//
// Here: the kernel argument, the recombination of the K packs a kernel has loaded, and the element path.  Two things stay
// written out in the kernels, because every other spelling that was tried changed their code for the worse
// (profiles/r20_share_rows.md):
//   * the K loads in flight of the pack path (rows issued with ldgw_issue<true> into rx[K], the kernel's own
//     ldgw_issue<false> loads next, rows finished first), in all seven;
//   * the recombination itself in k_cx_apply and k_carry_apply, the same DotAcc / F::acc loops as below, inline.
#pragma once

namespace ffgpu {

// the sub-share rows a party received and their Lagrange vector (prepared: f.prep)
template <class F, int K>
struct ShareRows {
    const typename F::elem* rows[K];
    typename F::word lam[K];
};

// v = sum_j lam[j] x[j], word by word, for the packs x[j] a kernel has loaded from one unit of the rows
template <class F, int K>
__device__ __forceinline__ Pack<typename F::word> share_rows_pack(const F& f, const ShareRows<F, K>& ra, const Pack<typename F::word> (&x)[K]) {
    typedef Pack<typename F::word> P;
    P v;
#pragma unroll
    for (int q = 0; q < P::N; ++q) {
        DotAcc<F> s;
        s.zero(f);
#pragma unroll
        for (int j = 0; j < K; ++j) s.mac(f, ra.lam[j], x[j].w[q]);
        v.w[q] = s.reduce(f);
    }
    return v;
}

// v for the element at compact index c
template <class F, int K>
__device__ __forceinline__ typename F::word share_rows_elem(const F& f, const ShareRows<F, K>& ra, size_t c) {
    typename F::acc s;
    f.acc_zero(s);
#pragma unroll
    for (int j = 0; j < K; ++j) f.acc_mac(s, ra.lam[j], ld_elem<F>(ra.rows[j], c));
    return f.acc_reduce(s);
}

}  // namespace ffgpu
