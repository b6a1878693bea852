// explog.hpp -- the local steps under the secure logarithm and exponential of fixed-point numbers over a prime field
// (runtime.np_log, np_exp2, runtime.py:4853-4945) that no other kernel serves: the doubling step of the power ladder
// (runtime.np_vander, runtime.py:4947-4977), the Taylor sum, the fixed-base power with per-element exponents
// (runtime._np_pow_public_int_base_secret_integral_exponent, runtime.py:1389-1425) and np_flip along the bit axis.  Included
// by kernels.hpp after fxp.hpp.  Index arithmetic and plans: explog_geom.hpp.
//
//   k_powers_prod   out[j n + e] = P[(h-1) stride + e] * P[j stride + e], j < w      the top power times the w lowest: dense (w, n)
//   k_poly_dot      out[e] = c0 + sum_{j<theta} tab[j] P[j stride + e]               one lazy accumulator, one reduction
//   k_pow_base      out[e] = prod_i T[15 i + d_i(e) - 1] over the windows d_i != 0   T = g^(d 16^i) staged in LDS
//   k_bits_reverse  out[h l + j] = bits[h l + l-1-j]                                 the reversed-row walk of geom.hpp
//
// The first two and the last are streaming kernels as the fixed-point kernels are: one flat grid-stride loop, a unit a pack
// (16 bytes; one 12- or 24-byte element) when the plan's vec, a single element otherwise, the 24-byte pack path
// wave-contiguous (ldgw / stgw: arrays of whole waves); the path is a kernel argument (wave-uniform).  k_powers_prod keeps
// the top power of its unit in registers across the w products: w + 1 loads per element where a materialised broadcast
// costs 2 w.  k_poly_dot stages the theta <= 64 prepared coefficients in LDS once per workgroup and accumulates without
// reducing, as k_recombine_any does for up to 64 rows.  k_bits_reverse moves its output as packs and reads by element,
// as k_norm_prod does.
//
// k_pow_base is bound by its products, not by memory: one element per thread and iteration, the table staged in LDS once
// per workgroup (the launcher caps the grid so that a workgroup serves many elements per staging), a window that is zero
// costs nothing, the first non-zero window is a copy.  The lookups are divergent LDS reads: lanes of a wave read up to 64
// different entries of one window's 15.
//
// Memory policy: the powers are read again by the next round and by the Taylor sum, every output by the next call:
// default policy throughout.
#pragma once
#include "explog_geom.hpp"

namespace ffgpu {

template <class F>
__global__ __launch_bounds__(BLOCK) void k_powers_prod(F f, const typename F::elem* P, int h, int w, typename F::elem* out,
                                                        RowsPlan pl, size_t n) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* pv = reinterpret_cast<const MP*>(P);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const PK top = ldgw_finish(ldgw_issue<false>(pv + rows_unit(pl, (size_t)h - 1, g)));
            for (int j = 0; j < w; ++j) {
                const PK x = ldgw_finish(ldgw_issue<false>(pv + rows_unit(pl, (size_t)j, g)));
                PK y;
#pragma unroll
                for (int q = 0; q < PK::N; ++q) y.w[q] = f.mul(top.w[q], x.w[q]);
                stgw<false>(ov + (size_t)j * pl.total + g, y);
            }
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const W top = ld_elem<F>(P, rows_unit(pl, (size_t)h - 1, g));
            for (int j = 0; j < w; ++j)
                st_elem<F>(out, (size_t)j * n + g, f.mul(top, ld_elem<F>(P, rows_unit(pl, (size_t)j, g))));
        }
    }
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_poly_dot(F f, const typename F::elem* __restrict__ P, int theta,
                                                     const typename F::elem* __restrict__ tab, typename F::word c0,
                                                     typename F::elem* __restrict__ out, RowsPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    __shared__ W coef[POLY_MAX_TERMS];
    if ((int)threadIdx.x < theta) coef[threadIdx.x] = f.prep(ld_elem<F>(tab, threadIdx.x));
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* pv = reinterpret_cast<const MP*>(P);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            typename F::acc s[PK::N];
#pragma unroll
            for (int q = 0; q < PK::N; ++q) f.acc_zero(s[q]);
            for (int j = 0; j < theta; ++j) {
                const PK x = ldgw_finish(ldgw_issue<false>(pv + rows_unit(pl, (size_t)j, g)));
                const W c = coef[j];
#pragma unroll
                for (int q = 0; q < PK::N; ++q) f.acc_mac(s[q], c, x.w[q]);
            }
            PK y;
#pragma unroll
            for (int q = 0; q < PK::N; ++q) y.w[q] = f.add(f.acc_reduce(s[q]), c0);
            stgw<false>(ov + g, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            typename F::acc s;
            f.acc_zero(s);
            for (int j = 0; j < theta; ++j) f.acc_mac(s, coef[j], ld_elem<F>(P, rows_unit(pl, (size_t)j, g)));
            st_elem<F>(out, g, f.add(f.acc_reduce(s), c0));
        }
    }
}

// limb q of a canonical word as an integer of 64-bit limbs (limbs the word does not have are zero)
template <class W>
__device__ __forceinline__ uint64_t explog_limb(const W& w, int q) {
    if constexpr (sizeof(W) == 24) return q == 0 ? w.lo : q == 1 ? w.mid : w.hi;
    else if constexpr (sizeof(W) == 16) return q == 0 ? w.lo : q == 1 ? w.hi : 0;
    else return q == 0 ? (uint64_t)w : 0;
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_pow_base(F f, const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ tab,
                                                     typename F::elem* __restrict__ out, PowBasePlan pl, size_t n) {
    typedef typename F::word W;
    __shared__ W T[POW_WIN_DIGITS * pow_base_max_windows(sizeof(typename F::elem))];
    for (int i = threadIdx.x; i < pl.tab_elems; i += BLOCK) T[i] = ld_elem<F>(tab, (size_t)i);
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    const W one = ff_one_elem(f);
    for (size_t e = gid; e < n; e += gsz) {
        const W v = ld_elem<F>(x, e);
        const uint64_t l0 = explog_limb(v, 0), l1 = explog_limb(v, 1), l2 = explog_limb(v, 2);
        W acc = one;
        bool have = false;
        for (int i = 0; i < pl.nwin; ++i) {
            const unsigned d = pow_base_digit(pl, l0, l1, l2, i);
            if (d) {
                const W t = T[pow_base_slot(i, d)];
                acc = have ? f.mul(acc, t) : t;
                have = true;
            }
        }
        st_elem<F>(out, e, acc);
    }
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_bits_reverse(F f, const typename F::elem* __restrict__ bits, typename F::elem* __restrict__ out,
                                                         RevPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            RevAt at = rev_at(pl, g * PK::N);
            PK y;
#pragma unroll
            for (int q = 0; q < PK::N; ++q) {
                y.w[q] = ld_elem<F>(bits, at.src);
                rev_next(pl, at);
            }
            stgw<false>(ov + g, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) st_elem<F>(out, g, ld_elem<F>(bits, rev_at(pl, g).src));
    }
}

}  // namespace ffgpu
