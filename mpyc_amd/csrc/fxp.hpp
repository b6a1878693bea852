// fxp.hpp -- the local steps of fixed-point arithmetic for one party's shares over a prime field: the secure truncation
// runtime.np_trunc (runtime.py:839-873) and the gate in front of the search of runtime._norm (runtime.py:4718-4727), on which
// protocols.py builds the fixed-point product, _norm, _rec (runtime.py:4737-4745) and np_divide.  Included by kernels.hpp after
// find.hpp.  Index arithmetic and plans: fxp_geom.hpp; the tile of the mask: sgn_geom.hpp.
//
//   k_trunc_mask    ar[h] = a[h] + sum_k rbits[h f + k] 2^k;  masked[h] = ar[h] + offset + rdivf[h] 2^f     the value that is opened
//   k_trunc_finish  c = sum_s lam[s] rows[s][h] as its canonical integer;  out[h] = (ar[h] - (c mod 2^f)) 2^-f
//   k_norm_prod     out[h (l-1) + j] = (2 x_top - 1) bits[h l + l-2-j];  sign[h] = 1 - 2 x_top               compact (n, l - 1)
//   k_norm_apply    v = sum_s lam[s] rows[s][h (l-1) + j];  out[h (l-1) + j] = 1 - x_top + v                 dense (n, l - 1, 1)
// x_top = bits[h l + l-1], bit index k least significant first.
//
// k_trunc_mask is k_bits_mask with the other sign of the bit sum and a second store: the same tile, chunks, Horner walk and
// occupancy (bits_mask_sum, bits.hpp).  ar is stored so that the finish reads one element per value instead of the f bit
// shares again.  The other three are streaming kernels as the tournament kernels are: one flat grid-stride loop, a unit a
// pack (16 bytes; one 12- or 24-byte element) when the plan's vec, a single element otherwise, the 24-byte pack path
// wave-contiguous (ldgw / stgw: arrays of whole waves); the path is a kernel argument (wave-uniform).  The two norm kernels
// move the compact side as packs and read the bits by element: consecutive lanes read a row backwards, which falls into the
// same cache lines as reading it forwards, and x_top is one line per row.
//
// The opened value c of the finish exists in registers only.  Elements are canonical in memory for every policy (the
// Montgomery policies convert inside a product), so the canonical integer of c is the recombined word itself and c mod 2^f
// the low limb under a mask (sgn_low64, as k_sgn_expand takes c mod 2^l); the mask is built on the host, so f = 64 shifts
// nothing by 64.
//
// Memory policy: bit shares are read once: non-temporal loads.  ar, the bits and every output are read by the next call:
// default policy.  The sub-share rows of the finish and of the apply: share_rows.hpp.
#pragma once
#include "fxp_geom.hpp"
#include "sgn_geom.hpp"

namespace ffgpu {

template <class F>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_trunc_mask(F f, const typename F::elem* __restrict__ a, const typename F::elem* __restrict__ rbits,
                                                       const typename F::elem* __restrict__ rdivf, int fb, typename F::word two_f,
                                                       typename F::word offset, typename F::elem* __restrict__ ar_out,
                                                       typename F::elem* __restrict__ out, size_t n) {
    typedef typename F::word W;
    __shared__ uint32_t lds[sgn_lds_words(sizeof(typename F::elem))];
    const BitsMaskSum<F> m = bits_mask_sum<F>(f, lds, a, rbits, rdivf, fb, n);
    const W ar = f.add(m.av, m.acc);
    const W hi = f.mul(m.rd, two_f);
    sgn_store<F>(ar_out, m.h, ar, m.live, m.wave_full);
    sgn_store<F>(out, m.h, f.add(f.add(ar, offset), hi), m.live, m.wave_full);
}

// (ar - (c mod 2^f)) 2^-f for a recombined c
template <class F>
__device__ __forceinline__ typename F::word trunc_value(const F& f, const typename F::word& ar, const typename F::word& c, uint64_t cmask,
                                                        const typename F::word& inv) {
    return f.mul(f.sub(ar, sgn_word64<typename F::word>(sgn_low64(c) & cmask)), inv);
}

template <class F, int K>
__global__ __launch_bounds__(BLOCK) void k_trunc_finish(F f, ShareRows<F, K> ra, const typename F::elem* __restrict__ ar, uint64_t cmask,
                                                         typename F::word inv, typename F::elem* __restrict__ out, FlatPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* av = reinterpret_cast<const MP*>(ar);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            P x[K], x0;
            {
                decltype(ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[0]))) rx[K];
#pragma unroll
                for (int j = 0; j < K; ++j) rx[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[j]) + g);
                const auto r0 = ldgw_issue<false>(av + g);
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = ldgw_finish(rx[j]);
                x0 = ldgw_finish(r0);
            }
            const P c = share_rows_pack<F, K>(f, ra, x);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = trunc_value<F>(f, x0.w[q], c.w[q], cmask, inv);
            stgw<false>(ov + g, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const W c = share_rows_elem<F, K>(f, ra, g);
            st_elem<F>(out, g, trunc_value<F>(f, ld_elem<F>(ar, g), c, cmask, inv));
        }
    }
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_norm_prod(F f, const typename F::elem* __restrict__ bits, typename F::elem* __restrict__ out,
                                                      typename F::elem* __restrict__ sign_out, RevPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    const W one = ff_one_elem(f);
    if (pl.vec) {
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            RevAt at = rev_at(pl, g * P::N);
            W xb[P::N], xt[P::N];
            size_t sg_at[P::N];
#pragma unroll
            for (int q = 0; q < P::N; ++q) {
                xb[q] = ld_elem<F>(bits, at.src);
                xt[q] = ld_elem<F>(bits, at.top);
                sg_at[q] = at.j == 0 ? at.h : (size_t)-1;
                rev_next(pl, at);
            }
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) {
                const W s = f.sub(f.add(xt[q], xt[q]), one);
                y.w[q] = f.mul(s, xb[q]);
                if (sign_out && sg_at[q] != (size_t)-1) st_elem<F>(sign_out, sg_at[q], f.neg(s));
            }
            stgw<false>(ov + g, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const RevAt at = rev_at(pl, g);
            const W xb = ld_elem<F>(bits, at.src), xt = ld_elem<F>(bits, at.top);
            const W s = f.sub(f.add(xt, xt), one);
            st_elem<F>(out, g, f.mul(s, xb));
            if (sign_out && at.j == 0) st_elem<F>(sign_out, at.h, f.neg(s));
        }
    }
}

template <class F, int K>
__global__ __launch_bounds__(BLOCK) void k_norm_apply(F f, ShareRows<F, K> ra, const typename F::elem* __restrict__ bits,
                                                       typename F::elem* __restrict__ out, RevPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    const W one = ff_one_elem(f);
    if (pl.vec) {
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            P x[K];
            W xt[P::N];
            {
                decltype(ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[0]))) rx[K];
#pragma unroll
                for (int j = 0; j < K; ++j) rx[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[j]) + g);
                RevAt at = rev_at(pl, g * P::N);
#pragma unroll
                for (int q = 0; q < P::N; ++q) {
                    xt[q] = ld_elem<F>(bits, at.top);
                    rev_next(pl, at);
                }
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = ldgw_finish(rx[j]);
            }
            const P v = share_rows_pack<F, K>(f, ra, x);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = f.add(f.sub(one, xt[q]), v.w[q]);
            stgw<false>(ov + g, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const RevAt at = rev_at(pl, g);
            const W v = share_rows_elem<F, K>(f, ra, g);
            st_elem<F>(out, g, f.add(f.sub(one, ld_elem<F>(bits, at.top)), v));
        }
    }
}

}  // namespace ffgpu
