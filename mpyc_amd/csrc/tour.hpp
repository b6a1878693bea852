// tour.hpp -- the data-movement ends of a tournament round for one party's shares over a prime field: the maximum / minimum
// along an axis (runtime.np_amax / np_amin, runtime.py:3413-3419, 3462-3468) and the argmax / argmin with unit vectors
// (runtime._np_argmax / _np_argmin, runtime.py:3806-3820, 3934-3948).  Included by kernels.hpp after bits.hpp.  The two
// pairings in closed form, the plan and every index: tour_geom.hpp.
//
//   k_tour_diff         out[o, j, i] = a[o, second_j, i] - a[o, first_j, i]  (neg: the other way round)   compact (outer, h, inner)
//   k_tour_select       v = sum_s lam[s] rows[s][o, j, i];  out[o, n0 + j, i] = a[o, first_j, i] + v  (neg: - v);
//                       out[o, 0, i] = a[o, 0, i] when n0                                                   half level (outer, kc, inner)
//   k_tour_unit_prod    out[o, j, i] = u[o, n0 + j, i] * c[o, j, i]                                          compact
//   k_tour_unit_expand  v as above;  out[o, n0 + 2j, i] = u[o, n0 + j, i] - v;  out[o, n0 + 2j + 1, i] = v;
//                       out[o, 0, i] = u[o, 0, i] when n0                                                   full level (outer, k, inner)
// Between diff and select the caller compares the differences with zero and multiplies the bit by the difference; between
// unit_prod and unit_expand it re-shares the product.  The rows are the sub-shares a party received (share_rows.hpp).
//
// All four are streaming kernels over the compact index: one unit per thread, all loads of a unit issued before the first
// use.  A unit is a pack (16 bytes; one 12- or 24-byte element) when runs, compact rows and the bye are whole packs and the
// pointers are aligned (TourPlan::vec), a single element otherwise.  The 24-byte pack path is wave-contiguous (ldgw / stgw):
// the plan admits it only for runs, compact rows and byes of whole waves, so every wave of the loop is entirely in or out,
// lane L is at first + L, and a wave carries a piece of the bye with all its lanes or with none; the branch that selects the
// path is a kernel argument (wave-uniform).  The units that carry the bye are the first of a compact row.
//
// Memory policy: the levels and the compact outputs are read by the next call: default policy.  The sub-share rows:
// share_rows.hpp.
#pragma once
#include "tour_geom.hpp"

namespace ffgpu {

template <class F>
__global__ __launch_bounds__(BLOCK) void k_tour_diff(F f, const typename F::elem* __restrict__ a, typename F::elem* __restrict__ out,
                                                      TourPlan pl, int neg) {
    typedef Pack<typename F::word> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* av = reinterpret_cast<const MP*>(a);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const TourAt at = tour_at(pl, g);
            const auto r0 = ldgw_issue<false>(av + (neg ? at.second : at.first)), r1 = ldgw_issue<false>(av + (neg ? at.first : at.second));
            const P x0 = ldgw_finish(r0), x1 = ldgw_finish(r1);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = f.sub(x1.w[q], x0.w[q]);
            stgw<false>(ov + at.c, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const TourAt at = tour_at(pl, g);
            const typename F::word x0 = ld_elem<F>(a, neg ? at.second : at.first), x1 = ld_elem<F>(a, neg ? at.first : at.second);
            st_elem<F>(out, at.c, f.sub(x1, x0));
        }
    }
}

template <class F, int K>
__global__ __launch_bounds__(BLOCK) void k_tour_select(F f, ShareRows<F, K> ra, const typename F::elem* __restrict__ a,
                                                        typename F::elem* __restrict__ out, TourPlan pl, int neg) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* av = reinterpret_cast<const MP*>(a);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const TourAt at = tour_at(pl, g);
            P x[K], x0;
            {
                decltype(ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[0]))) rx[K];
#pragma unroll
                for (int j = 0; j < K; ++j) rx[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[j]) + at.c);
                const auto r0 = ldgw_issue<false>(av + at.first);
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = ldgw_finish(rx[j]);
                x0 = ldgw_finish(r0);
            }
            const P v = share_rows_pack<F, K>(f, ra, x);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = neg ? f.sub(x0.w[q], v.w[q]) : f.add(x0.w[q], v.w[q]);
            stgw<false>(ov + at.half, y);
            if (at.bye) {                                   // (24-byte elements: the whole wave or none of it)
                const P z = ldgw_finish(ldgw_issue<false>(av + at.bye_full));
                stgw<false>(ov + at.bye_half, z);
            }
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const TourAt at = tour_at(pl, g);
            const W v = share_rows_elem<F, K>(f, ra, at.c);
            const W x0 = ld_elem<F>(a, at.first);
            st_elem<F>(out, at.half, neg ? f.sub(x0, v) : f.add(x0, v));
            if (at.bye) st_elem<F>(out, at.bye_half, ld_elem<F>(a, at.bye_full));
        }
    }
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_tour_unit_prod(F f, const typename F::elem* __restrict__ u, const typename F::elem* __restrict__ c,
                                                           typename F::elem* __restrict__ out, TourPlan pl) {
    typedef Pack<typename F::word> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* uv = reinterpret_cast<const MP*>(u);
        const MP* cv = reinterpret_cast<const MP*>(c);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const TourAt at = tour_at(pl, g);
            const auto r0 = ldgw_issue<false>(uv + at.half), r1 = ldgw_issue<false>(cv + at.c);
            const P x0 = ldgw_finish(r0), x1 = ldgw_finish(r1);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = f.mul(x0.w[q], x1.w[q]);
            stgw<false>(ov + at.c, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const TourAt at = tour_at(pl, g);
            st_elem<F>(out, at.c, f.mul(ld_elem<F>(u, at.half), ld_elem<F>(c, at.c)));
        }
    }
}

template <class F, int K>
__global__ __launch_bounds__(BLOCK) void k_tour_unit_expand(F f, ShareRows<F, K> ra, const typename F::elem* __restrict__ u,
                                                             typename F::elem* __restrict__ out, TourPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* uv = reinterpret_cast<const MP*>(u);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const TourAt at = tour_at(pl, g);
            P x[K], x0;
            {
                decltype(ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[0]))) rx[K];
#pragma unroll
                for (int j = 0; j < K; ++j) rx[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[j]) + at.c);
                const auto r0 = ldgw_issue<false>(uv + at.half);
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = ldgw_finish(rx[j]);
                x0 = ldgw_finish(r0);
            }
            const P v = share_rows_pack<F, K>(f, ra, x);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = f.sub(x0.w[q], v.w[q]);
            stgw<false>(ov + at.first, y);
            stgw<false>(ov + at.second, v);
            if (at.bye) {                                   // (24-byte elements: the whole wave or none of it)
                const P z = ldgw_finish(ldgw_issue<false>(uv + at.bye_half));
                stgw<false>(ov + at.bye_full, z);
            }
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const TourAt at = tour_at(pl, g);
            const W v = share_rows_elem<F, K>(f, ra, at.c);
            const W x0 = ld_elem<F>(u, at.half);
            st_elem<F>(out, at.first, f.sub(x0, v));
            st_elem<F>(out, at.second, v);
            if (at.bye) st_elem<F>(out, at.bye_full, ld_elem<F>(u, at.bye_half));
        }
    }
}

}  // namespace ffgpu
