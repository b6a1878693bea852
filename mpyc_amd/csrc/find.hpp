// find.hpp -- the data-movement ends of a round of the first-occurrence search along an axis for one party's shares over a
// prime field (runtime.np_find, runtime.py:4603-4698).  Included by kernels.hpp after tour.hpp.  The pairing, the plans and
// every index: find_geom.hpp.
//
// A level is component-major (C, outer, kk, inner), component 0 = nf, components 1..F the running values of cs_f.  The leaf
// level is never stored: leaf j is (b', tab[q,0,j] + b' tab[q,1,j]) with b' = b or 1 - b (flip) from the bits (outer, k,
// inner), and the public leaf (1, tab[q,0,k] + tab[q,1,k]) at position k when virt.
//
//   k_find_leaf_prod    out[q, o, j, i] = leaf_0(first_j) * (leaf_q(second_j) - leaf_q(first_j))          compact (C, outer, h, inner)
//   k_find_leaf_apply   v = sum_s lam[s] rows[s][q, o, j, i];  out[q, o, n0 + j, i] = leaf_q(first_j) + v;
//                       out[q, o, 0, i] = leaf_q(0) when n0                                                 next level (C, outer, kc, inner)
//   k_find_prod         out[q, o, j, i] = lv[0, o, first_j, i] * (lv[q, o, second_j, i] - lv[q, o, first_j, i])   compact
// The apply of a later round, out[q, o, n0 + j, i] = lv[q, o, first_j, i] + v with the bye copied, is k_tour_select
// (tour.hpp) on (C * outer, kk, inner) with TOUR_ODD_EVEN and neg = 0: the components are just more rows of the same round,
// so there is no copy of it here.
//
// The three follow the tournament kernels: one flat grid-stride loop over the compact units of ONE component, a unit a pack
// (16 bytes; one 12- or 24-byte element) when FindPlan::t.vec, a single element otherwise, the 24-byte pack path
// wave-contiguous (runs, compact rows and byes of whole waves; the public leaf is then the partner of whole waves); the
// path is a kernel argument (wave-uniform).  A thread walks the C components of its unit: the bits and nf are loaded once
// per unit and serve every component, and a position is uniform over a pack, so a table entry is read once per pack.  The
// loads of a unit's bits are issued before the first use; so are the two (prod) or nrows (apply) loads of each component,
// and apply issues the rows of component q + 1 before it computes component q.  The public leaf's bit is not loaded: the
// plan gives it the first member's address (issued, not used) and the kernel selects the public 1.
//
// Memory policy: bits, levels and compact outputs are read again by the next call: default policy.  The sub-share rows:
// share_rows.hpp.  The table is F * 2 * kv elements, read through the cache with default policy; with inner
// == 1 the position differs lane by lane (a gather over 2 * 64 adjacent entries per wave), with inner > 1 it is uniform over
// a run.  With inner == 1 a pair is two adjacent elements: one 16-byte load per lane for 8-byte elements instead of two
// element loads was built and measured at (10^6, 31, 1) and changed nothing (profiles/find_kernels.md), so the element path
// loads the two members as it does for every other inner.
#pragma once
#include "find_geom.hpp"

namespace ffgpu {

// b' of a loaded bit: b, 1 - b when flip, and the public 1 for the virtual leaf (never flipped)
template <class F>
__device__ __forceinline__ typename F::word find_bit(const F& f, const typename F::word& b, const typename F::word& one, int flip, int pub) {
    return ff_pick(pub != 0, one, ff_pick(flip != 0, f.sub(one, b), b));
}
// the two table entries of value component q >= 1 at position pos: tab is (F, 2, kv)
template <class F>
struct FindTab {
    typename F::word t0, t1;
};
template <class F>
__device__ __forceinline__ FindTab<F> find_tab(const typename F::elem* __restrict__ tab, size_t kv, int q, size_t pos) {
    FindTab<F> e;
    const size_t at = (size_t)(q - 1) * 2 * kv + pos;
    e.t0 = ld_elem<F>(tab, at);
    e.t1 = ld_elem<F>(tab, at + kv);
    return e;
}
template <class F>
__device__ __forceinline__ typename F::word find_leaf(const F& f, const FindTab<F>& e, const typename F::word& bp) {
    return f.add(e.t0, f.mul(bp, e.t1));
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_find_leaf_prod(F f, const typename F::elem* __restrict__ bits, const typename F::elem* __restrict__ tab,
                                                           typename F::elem* __restrict__ out, FindPlan pl, int ncomp, int flip) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    const W one = ff_one_elem(f);
    if (pl.t.vec) {
        const MP* bv = reinterpret_cast<const MP*>(bits);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.t.total; g += gsz) {
            const FindAt at = find_leaf_at(pl, g);
            const auto r0 = ldgw_issue<false>(bv + at.first), r1 = ldgw_issue<false>(bv + at.second);
            P b1 = ldgw_finish(r0), b2 = ldgw_finish(r1), y;
#pragma unroll
            for (int w = 0; w < P::N; ++w) {
                b1.w[w] = find_bit(f, b1.w[w], one, flip, 0);
                b2.w[w] = find_bit(f, b2.w[w], one, flip, at.virt2);
                y.w[w] = f.mul(b1.w[w], f.sub(b2.w[w], b1.w[w]));
            }
            stgw<false>(ov + at.c, y);
            for (int q = 1; q < ncomp; ++q) {
                const FindTab<F> e1 = find_tab<F>(tab, pl.kv, q, at.pos), e2 = find_tab<F>(tab, pl.kv, q, at.pos + 1);
#pragma unroll
                for (int w = 0; w < P::N; ++w) y.w[w] = f.mul(b1.w[w], f.sub(find_leaf(f, e2, b2.w[w]), find_leaf(f, e1, b1.w[w])));
                stgw<false>(ov + (size_t)q * pl.plane_c + at.c, y);
            }
        }
    } else {
        for (size_t g = gid; g < pl.t.total; g += gsz) {
            const FindAt at = find_leaf_at(pl, g);
            const W x1 = ld_elem<F>(bits, at.first), x2 = ld_elem<F>(bits, at.second);
            const W b1 = find_bit(f, x1, one, flip, 0), b2 = find_bit(f, x2, one, flip, at.virt2);
            st_elem<F>(out, at.c, f.mul(b1, f.sub(b2, b1)));
            for (int q = 1; q < ncomp; ++q) {
                const FindTab<F> e1 = find_tab<F>(tab, pl.kv, q, at.pos), e2 = find_tab<F>(tab, pl.kv, q, at.pos + 1);
                st_elem<F>(out, (size_t)q * pl.plane_c + at.c, f.mul(b1, f.sub(find_leaf(f, e2, b2), find_leaf(f, e1, b1))));
            }
        }
    }
}

template <class F, int K>
__global__ __launch_bounds__(BLOCK) void k_find_leaf_apply(F f, ShareRows<F, K> ra, const typename F::elem* __restrict__ bits,
                                                            const typename F::elem* __restrict__ tab, typename F::elem* __restrict__ out,
                                                            FindPlan pl, int ncomp, int flip) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    const W one = ff_one_elem(f);
    if (pl.t.vec) {
        const MP* bv = reinterpret_cast<const MP*>(bits);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.t.total; g += gsz) {
            const FindAt at = find_leaf_at(pl, g);
            decltype(ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[0]))) rx[K];
            const auto r0 = ldgw_issue<false>(bv + at.first);
#pragma unroll
            for (int j = 0; j < K; ++j) rx[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[j]) + at.c);
            P b1 = ldgw_finish(r0);
#pragma unroll
            for (int w = 0; w < P::N; ++w) b1.w[w] = find_bit(f, b1.w[w], one, flip, 0);
            for (int q = 0; q < ncomp; ++q) {
                P x[K];
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = ldgw_finish(rx[j]);
                if (q + 1 < ncomp) {                        // the next component's rows fly while this one is computed
#pragma unroll
                    for (int j = 0; j < K; ++j)
                        rx[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[j]) + (size_t)(q + 1) * pl.plane_c + at.c);
                }
                const P v = share_rows_pack<F, K>(f, ra, x);
                P y;
                if (q == 0) {
#pragma unroll
                    for (int w = 0; w < P::N; ++w) y.w[w] = f.add(b1.w[w], v.w[w]);
                } else {
                    const FindTab<F> e = find_tab<F>(tab, pl.kv, q, at.pos);
#pragma unroll
                    for (int w = 0; w < P::N; ++w) y.w[w] = f.add(find_leaf(f, e, b1.w[w]), v.w[w]);
                }
                stgw<false>(ov + (size_t)q * pl.plane_half + at.half, y);
            }
            if (at.bye) {                                   // (24-byte elements: the whole wave or none of it)
                P z = ldgw_finish(ldgw_issue<false>(bv + at.bye_full));
#pragma unroll
                for (int w = 0; w < P::N; ++w) z.w[w] = find_bit(f, z.w[w], one, flip, 0);
                stgw<false>(ov + at.bye_half, z);
                for (int q = 1; q < ncomp; ++q) {
                    const FindTab<F> e = find_tab<F>(tab, pl.kv, q, 0);
                    P y;
#pragma unroll
                    for (int w = 0; w < P::N; ++w) y.w[w] = find_leaf(f, e, z.w[w]);
                    stgw<false>(ov + (size_t)q * pl.plane_half + at.bye_half, y);
                }
            }
        }
    } else {
        for (size_t g = gid; g < pl.t.total; g += gsz) {
            const FindAt at = find_leaf_at(pl, g);
            const W b1 = find_bit(f, ld_elem<F>(bits, at.first), one, flip, 0);
            for (int q = 0; q < ncomp; ++q) {
                const W v = share_rows_elem<F, K>(f, ra, (size_t)q * pl.plane_c + at.c);
                const W leaf = q == 0 ? b1 : find_leaf(f, find_tab<F>(tab, pl.kv, q, at.pos), b1);
                st_elem<F>(out, (size_t)q * pl.plane_half + at.half, f.add(leaf, v));
            }
            if (at.bye) {
                const W z = find_bit(f, ld_elem<F>(bits, at.bye_full), one, flip, 0);
                st_elem<F>(out, at.bye_half, z);
                for (int q = 1; q < ncomp; ++q)
                    st_elem<F>(out, (size_t)q * pl.plane_half + at.bye_half, find_leaf(f, find_tab<F>(tab, pl.kv, q, 0), z));
            }
        }
    }
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_find_prod(F f, const typename F::elem* __restrict__ lv, typename F::elem* __restrict__ out,
                                                      FindPlan pl, int ncomp) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.t.vec) {
        const MP* av = reinterpret_cast<const MP*>(lv);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.t.total; g += gsz) {
            const TourAt at = tour_at(pl.t, g);
            const auto r0 = ldgw_issue<false>(av + at.first), r1 = ldgw_issue<false>(av + at.second);
            const P nf = ldgw_finish(r0);
            P x0 = nf, x1 = ldgw_finish(r1);
            for (int q = 0;;) {
                P y;
#pragma unroll
                for (int w = 0; w < P::N; ++w) y.w[w] = f.mul(nf.w[w], f.sub(x1.w[w], x0.w[w]));
                stgw<false>(ov + (size_t)q * pl.plane_c + at.c, y);
                if (++q == ncomp) break;
                const auto s0 = ldgw_issue<false>(av + (size_t)q * pl.plane_full + at.first),
                           s1 = ldgw_issue<false>(av + (size_t)q * pl.plane_full + at.second);
                x0 = ldgw_finish(s0);
                x1 = ldgw_finish(s1);
            }
        }
    } else {
        for (size_t g = gid; g < pl.t.total; g += gsz) {
            const TourAt at = tour_at(pl.t, g);
            const W nf = ld_elem<F>(lv, at.first);
            W x0 = nf, x1 = ld_elem<F>(lv, at.second);
            for (int q = 0;;) {
                st_elem<F>(out, (size_t)q * pl.plane_c + at.c, f.mul(nf, f.sub(x1, x0)));
                if (++q == ncomp) break;
                x0 = ld_elem<F>(lv, (size_t)q * pl.plane_full + at.first);
                x1 = ld_elem<F>(lv, (size_t)q * pl.plane_full + at.second);
            }
        }
    }
}

}  // namespace ffgpu
