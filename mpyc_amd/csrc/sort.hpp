// sort.hpp -- the two data-movement ends of a compare-exchange stage of runtime.np_sort (runtime.py:1764-1770; Batcher's
// merge-exchange network) for one party's shares over a prime field.  Included by kernels.hpp after sgn.hpp.  The stage in
// closed form, the plan and every index: sort_geom.hpp.
//
//   k_cx_diff    out[o, j, i] = a[o, I_j + d, i] - a[o, I_j, i]                       compact (outer, P, inner)
//   k_cx_apply   h = sum_s lam[s] rows[s][o, j, i];  a[o, I_j, i] += h;  a[o, I_j + d, i] -= h        in place
// Between the two the caller compares the differences with zero and multiplies the bit by the difference; the rows of
// k_cx_apply are the sub-shares of that product a party received (share_rows.hpp).
//
// Both are streaming kernels over the compact index: one unit per thread, all loads of a unit issued before the first use.
// A unit is a pack (16 bytes; one 12- or 24-byte element) when runs, compact rows and row pitch are whole packs and the
// pointers are aligned (CxPlan::vec), a single element otherwise.  The 24-byte pack path is wave-contiguous (ldgw / stgw):
// the plan admits it only for runs and compact rows of whole waves, so every wave of the loop is entirely in or out and
// lane L is at first + L; the branch that selects the path is a kernel argument (wave-uniform).
// I and I + d are disjoint: the thread that owns a pair reads and writes both members, nothing synchronises.
//
// Memory policy: `a` is read by k_cx_diff, read and written by k_cx_apply and read again by the next stage, the differences
// feed the comparison at once: default policy.  The sub-share rows: share_rows.hpp.
#pragma once
#include "sort_geom.hpp"

namespace ffgpu {

static_assert((int)GEOM_THREADS == (int)BLOCK && (int)CX_THREADS == (int)BLOCK, "geom.hpp is laid out for the library's workgroup");

template <class F>
__global__ __launch_bounds__(BLOCK) void k_cx_diff(F f, const typename F::elem* __restrict__ a, typename F::elem* __restrict__ out,
                                                    CxPlan pl) {
    typedef Pack<typename F::word> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* av = reinterpret_cast<const MP*>(a);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const CxAt at = cx_at(pl, g);
            const auto r0 = ldgw_issue<false>(av + at.lo), r1 = ldgw_issue<false>(av + at.hi);
            const P x0 = ldgw_finish(r0), x1 = ldgw_finish(r1);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = f.sub(x1.w[q], x0.w[q]);
            stgw<false>(ov + at.c, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const CxAt at = cx_at(pl, g);
            st_elem<F>(out, at.c, f.sub(ld_elem<F>(a, at.hi), ld_elem<F>(a, at.lo)));
        }
    }
}

template <class F, int K>
__global__ __launch_bounds__(BLOCK) void k_cx_apply(F f, ShareRows<F, K> ra, typename F::elem* __restrict__ a, CxPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        MP* av = reinterpret_cast<MP*>(a);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const CxAt at = cx_at(pl, g);
            P x[K], x0, x1;
            {
                decltype(ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[0]))) rx[K];
#pragma unroll
                for (int j = 0; j < K; ++j) rx[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[j]) + at.c);
                const auto r0 = ldgw_issue<false>(const_cast<const MP*>(av) + at.lo), r1 = ldgw_issue<false>(const_cast<const MP*>(av) + at.hi);
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = ldgw_finish(rx[j]);
                x0 = ldgw_finish(r0);
                x1 = ldgw_finish(r1);
            }
            P y0, y1;
#pragma unroll
            for (int q = 0; q < P::N; ++q) {
                DotAcc<F> s;
                s.zero(f);
#pragma unroll
                for (int j = 0; j < K; ++j) s.mac(f, ra.lam[j], x[j].w[q]);
                const W h = s.reduce(f);
                y0.w[q] = f.add(x0.w[q], h);
                y1.w[q] = f.sub(x1.w[q], h);
            }
            stgw<false>(av + at.lo, y0);
            stgw<false>(av + at.hi, y1);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const CxAt at = cx_at(pl, g);
            typename F::acc s;
            f.acc_zero(s);
#pragma unroll
            for (int j = 0; j < K; ++j) f.acc_mac(s, ra.lam[j], ld_elem<F>(ra.rows[j], at.c));
            const W h = f.acc_reduce(s);
            const W x0 = ld_elem<F>(a, at.lo), x1 = ld_elem<F>(a, at.hi);
            st_elem<F>(a, at.lo, f.add(x0, h));
            st_elem<F>(a, at.hi, f.sub(x1, h));
        }
    }
}

}  // namespace ffgpu
