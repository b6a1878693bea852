// bsgn.hpp -- the two local steps of the secure binary sign by Legendre symbols over a Blum prime (p = 3 mod 4), the
// activation of the binarized network demo (demos/np_bnnmnist.py:44-156): for a prime p chosen so that (2a + 1 | p) is the sign
// of a over a range of a, one masked opening and one Legendre symbol per element give the sign; the demo's variants take
// w = 1, 3 or 5 symbols of 2a + 1 + 2j.  Included by kernels.hpp after rbits.hpp.  Index arithmetic and plans: bsgn_geom.hpp.
//
//   k_bsgn_mask        out[i n + e] = z[i n + e] (alpha a[e] + beta[i]), i < w                      the value that is opened
//   k_bsgn_finish      h = (c[i n + e] | p);  out_q[i n + e] = h s_q[i n + e], q < m                 rows mode
//   k_bsgn_finish_sum  out_q[e] = sum_{i < w} (c[i n + e] | p) s_q[i n + e], q < m                   sum mode
// with host scalars alpha and beta[i] (2 and 1 + 2j for the sign; 1 and 0 for the second stage of the five-symbol variant),
// z a sharing of s r^2 (s a random sign, r a random element) and (0 | p) = 0.  The arrays are row-major (w, n).
//
// k_bsgn_mask is a streaming kernel of the shape of k_iszero_mask: one flat grid-stride loop, a unit a pack when the plan's
// vec, a single element otherwise, the 24-byte pack path wave-contiguous (ldgw / stgw); the path is a kernel argument.  A
// thread forms alpha a once (a reduced product) and keeps it in registers across the w rows; per row one addition, one lazy
// product and one reduction: (2 w + 1) n elements of traffic where a materialised broadcast costs 3 w n + n.  The row loop is
// unrolled under a wave-uniform exit so that beta[i] is a kernel-argument register, never an indexed array.
//
// k_bsgn_finish is the exponentiation of k_pow with other ends (pow_stream, kernels.hpp), as k_legendre_code and
// k_rbits_finish are: the same chain for the exponent (p - 1) / 2, the same plan, grid and launch bounds, over the w n opened
// values.  The symbol of a PUBLIC value is formed once and serves every party's row: per row one load, one select between s,
// p - s and 0, one store behind some hundred products (ldg / stg by the lane, as k_rbits_finish); no code bytes are written.
// k_bsgn_finish_sum cannot be a put functor of pow_stream, which hands over one entry at a time: a thread owns a unit of the n
// elements, runs the same chain (ff_pow_digits on packs, ff_pow on single elements, as pow_stream does) on its unit of every
// row, keeps the w symbols as 2-bit codes in one 64-bit word, and then walks the parties: w loads, w - 1 additions or
// subtractions, one store each.
//
// Memory policy: the masked values are read by the opening, the opened values were written by it, every output is read by the
// next call: default-policy stores; the parties' shares are streamed: nt loads.
#pragma once
#include "bsgn_geom.hpp"

namespace ffgpu {

template <class F>
struct BsgnMaskArgs {
    typename F::word alpha;                     // canonical
    typename F::word beta[BSGN_MAX_ROWS];       // canonical; entries from w on repeat beta[0]
};

// z (ap + beta) with ap = alpha a: one addition, one lazy product, one reduction
template <class F>
__device__ __forceinline__ typename F::word bsgn_mask_value(const F& f, const typename F::word& ap, const typename F::word& beta,
                                                            const typename F::word& z) {
    typename F::acc s;
    f.acc_zero(s);
    f.acc_mac(s, f.prep(f.add(ap, beta)), z);
    return f.acc_reduce(s);
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_bsgn_mask(F f, const typename F::elem* __restrict__ a, const typename F::elem* __restrict__ z,
                                                      BsgnMaskArgs<F> ma, int w, typename F::elem* __restrict__ out, RowsPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* av = reinterpret_cast<const MP*>(a);
        const MP* zv = reinterpret_cast<const MP*>(z);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            PK ap = ldgw_finish(ldgw_issue<false>(av + g));
#pragma unroll
            for (int q = 0; q < PK::N; ++q) ap.w[q] = f.mul(ap.w[q], ma.alpha);
#pragma unroll
            for (int i = 0; i < BSGN_MAX_ROWS; ++i) {
                if (i >= w) break;
                const size_t u = rows_unit(pl, (size_t)i, g);
                const PK xz = ldgw_finish(ldgw_issue<false>(zv + u));
                PK y;
#pragma unroll
                for (int q = 0; q < PK::N; ++q) y.w[q] = bsgn_mask_value<F>(f, ap.w[q], ma.beta[i], xz.w[q]);
                stgw<false>(ov + u, y);
            }
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const W ap = f.mul(ld_elem<F>(a, g), ma.alpha);
#pragma unroll
            for (int i = 0; i < BSGN_MAX_ROWS; ++i) {
                if (i >= w) break;
                const size_t u = rows_unit(pl, (size_t)i, g);
                st_elem<F>(out, u, bsgn_mask_value<F>(f, ap, ma.beta[i], ld_elem<F>(z, u)));
            }
        }
    }
}

// the parties' rows of shares and outputs ((w, n) arrays; an output in sum mode has n entries)
template <class F>
struct BsgnFinishArgs {
    const typename F::elem* s[BSGN_MAX_PARTIES];
    typename F::elem* out[BSGN_MAX_PARTIES];
    int m;
};

// h s for the symbol h of code: s, p - s or 0
template <class F>
__device__ __forceinline__ typename F::word bsgn_signed(const F& f, unsigned code, const typename F::word& s) {
    typedef typename F::word W;
    return code == LEGENDRE_RESIDUE ? s : code == LEGENDRE_NONRESIDUE ? f.neg(s) : W();
}

template <class F>
struct PowPutBsgn {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const F& f;
    const BsgnFinishArgs<F>& fa;
    __device__ __forceinline__ void pack(size_t i, const P& x, const P& r) const {
        unsigned code[P::N];
#pragma unroll
        for (int q = 0; q < P::N; ++q) code[q] = legendre_code_of(x.w[q], r.w[q]);
        for (int j = 0; j < fa.m; ++j) {
            const P s = ldg<true>(reinterpret_cast<const MP*>(fa.s[j]) + i);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = bsgn_signed<F>(f, code[q], s.w[q]);
            stg<false>(reinterpret_cast<MP*>(fa.out[j]) + i, y);
        }
    }
    __device__ __forceinline__ void elem(size_t e, const W& x, const W& r) const {
        const unsigned code = legendre_code_of(x, r);
        for (int j = 0; j < fa.m; ++j) st_elem<F>(fa.out[j], e, bsgn_signed<F>(f, code, ld_elem<F>(fa.s[j], e)));
    }
};
template <class F>
__global__ __launch_bounds__(BLOCK) void k_bsgn_finish(F f, const typename F::elem* __restrict__ c, ExpArgs ex, BsgnFinishArgs<F> fa,
                                                        size_t nvec, size_t n) {
    pow_stream<F, false>(f, c, ex, nvec, n, PowPutBsgn<F>{f, fa});
}

// acc + h s
template <class F>
__device__ __forceinline__ typename F::word bsgn_accumulate(const F& f, unsigned code, const typename F::word& acc,
                                                            const typename F::word& s) {
    return code == LEGENDRE_RESIDUE ? f.add(acc, s) : code == LEGENDRE_NONRESIDUE ? f.sub(acc, s) : acc;
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_bsgn_finish_sum(F f, const typename F::elem* __restrict__ c, ExpArgs ex, BsgnFinishArgs<F> fa,
                                                            int w, RowsPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* cv = reinterpret_cast<const MP*>(c);
        for (size_t g = gid; g < pl.total; g += gsz) {
            uint64_t codes = 0;
            for (int i = 0; i < w; ++i) {
                const P x = ldg<false>(cv + rows_unit(pl, (size_t)i, g));
#pragma unroll
                for (int q = 0; q < P::N; ++q) codes = bsgn_sym_put(codes, i, q, legendre_code_of(x.w[q], ff_pow_digits(f, x.w[q], ex)));
            }
            for (int j = 0; j < fa.m; ++j) {
                const MP* sv = reinterpret_cast<const MP*>(fa.s[j]);
                P y;
#pragma unroll
                for (int q = 0; q < P::N; ++q) y.w[q] = W();
                for (int i = 0; i < w; ++i) {
                    const P s = ldg<true>(sv + rows_unit(pl, (size_t)i, g));
#pragma unroll
                    for (int q = 0; q < P::N; ++q) y.w[q] = bsgn_accumulate<F>(f, bsgn_sym_of(codes, i, q), y.w[q], s.w[q]);
                }
                stg<false>(reinterpret_cast<MP*>(fa.out[j]) + g, y);
            }
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            uint64_t codes = 0;
            for (int i = 0; i < w; ++i) {
                const W x = ld_elem<F>(c, rows_unit(pl, (size_t)i, g));
                codes = bsgn_sym_put(codes, i, 0, legendre_code_of(x, ff_pow(f, x, ex)));
            }
            for (int j = 0; j < fa.m; ++j) {
                W y = W();
                for (int i = 0; i < w; ++i)
                    y = bsgn_accumulate<F>(f, bsgn_sym_of(codes, i, 0), y, ld_elem<F>(fa.s[j], rows_unit(pl, (size_t)i, g)));
                st_elem<F>(fa.out[j], g, y);
            }
        }
    }
}

}  // namespace ffgpu
