// iszero.hpp -- the local steps of the probabilistic zero test over a Blum prime (p = 3 mod 4), runtime._np_is_zero
// (runtime.py:3581-3620), which runtime.np_equal takes for the default fields (runtime.py:3569-3579): k masked copies of every
// element, one opening, one Legendre symbol per opened value, a selection, a product over the k rows.  Included by
// kernels.hpp after explog.hpp.  Index arithmetic and plans: iszero_geom.hpp.
//
//   k_iszero_mask    c[i n + e] = a[e] r[i n + e] + (1 - 2 z[i n + e]) u2[i n + e], i < k        the value that is opened
//   k_legendre_code  code[j] = 2 if c[j] == 0, else 1 if c[j]^((p-1)/2) == 1, else 0              one byte per entry
//   k_iszero_finish  out[j] = z[j] if code[j] == 0, 1 - z[j] if code[j] == 1, 1 if code[j] == 2   0 counts as a square
// The arrays are row-major (k, n): row i holds the i-th masked copy of the n elements.
//
// k_iszero_mask and k_iszero_finish are streaming kernels as the fixed-point kernels are: one flat grid-stride loop, a unit a
// pack (16 bytes; one 12- or 24-byte element) when the plan's vec, a single element otherwise, the 24-byte pack path
// wave-contiguous (ldgw / stgw: arrays of whole waves); the path is a kernel argument (wave-uniform).  The mask keeps its unit
// of `a` in registers across the k rows, prepared once as the first operand of a lazy product, as k_powers_prod keeps the top
// power: (4 k + 1) n elements of traffic where a materialised broadcast costs 5 k n.  z holds SHARES of bits, arbitrary field
// elements, so both terms are full products: two lazy products into one accumulator and one reduction per entry.
//
// k_legendre_code is the exponentiation of k_pow with other ends (pow_stream, kernels.hpp): the same chain for the exponent
// (p - 1) / 2 (ff_pow_chain, in digits where the policy has them), the same plan, grid and launch bounds; a canonical element
// in, a compare against one and zero, a byte out.  It is bound by its products.  The codes of a pack leave as one ordinary
// 1-, 2- or 4-byte vector store.
//
// Memory policy: the masked values are read by the opening, the opened values were written by it, the codes and every output
// are read by the next call: default policy throughout.
#pragma once
#include "iszero_geom.hpp"

namespace ffgpu {

// the codes of a pack of N elements: N consecutive bytes as one access (N = 1, 2, 4; the plan guarantees the alignment)
template <int N>
__device__ __forceinline__ uint32_t ld_codes(const uint8_t* p) {
    if constexpr (N == 4) return *reinterpret_cast<const uint32_t*>(p);
    else if constexpr (N == 2) return *reinterpret_cast<const uint16_t*>(p);
    else return *p;
}
template <int N>
__device__ __forceinline__ void st_codes(uint8_t* p, uint32_t v) {
    if constexpr (N == 4) *reinterpret_cast<uint32_t*>(p) = v;
    else if constexpr (N == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
    else *p = (uint8_t)v;
}

// a r + (1 - 2 z) u2 with ap = prep(a): two lazy products, one reduction
template <class F>
__device__ __forceinline__ typename F::word iszero_mask_value(const F& f, const typename F::word& ap, const typename F::word& r,
                                                              const typename F::word& z, const typename F::word& u2,
                                                              const typename F::word& one) {
    typename F::acc s;
    f.acc_zero(s);
    f.acc_mac(s, ap, r);
    f.acc_mac(s, f.prep(f.sub(one, f.add(z, z))), u2);
    return f.acc_reduce(s);
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_iszero_mask(F f, const typename F::elem* __restrict__ a, const typename F::elem* __restrict__ r,
                                                        const typename F::elem* __restrict__ z, const typename F::elem* __restrict__ u2, int k,
                                                        typename F::elem* __restrict__ out, RowsPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    const W one = ff_one_elem(f);
    if (pl.vec) {
        const MP* av = reinterpret_cast<const MP*>(a);
        const MP* rv = reinterpret_cast<const MP*>(r);
        const MP* zv = reinterpret_cast<const MP*>(z);
        const MP* uv = reinterpret_cast<const MP*>(u2);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            PK ap = ldgw_finish(ldgw_issue<false>(av + g));
#pragma unroll
            for (int q = 0; q < PK::N; ++q) ap.w[q] = f.prep(ap.w[q]);
            for (int i = 0; i < k; ++i) {
                const size_t u = rows_unit(pl, (size_t)i, g);
                const auto r0 = ldgw_issue<false>(rv + u), r1 = ldgw_issue<false>(zv + u), r2 = ldgw_issue<false>(uv + u);
                const PK xr = ldgw_finish(r0), xz = ldgw_finish(r1), xu = ldgw_finish(r2);
                PK y;
#pragma unroll
                for (int q = 0; q < PK::N; ++q) y.w[q] = iszero_mask_value<F>(f, ap.w[q], xr.w[q], xz.w[q], xu.w[q], one);
                stgw<false>(ov + u, y);
            }
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const W ap = f.prep(ld_elem<F>(a, g));
            for (int i = 0; i < k; ++i) {
                const size_t u = rows_unit(pl, (size_t)i, g);
                st_elem<F>(out, u, iszero_mask_value<F>(f, ap, ld_elem<F>(r, u), ld_elem<F>(z, u), ld_elem<F>(u2, u), one));
            }
        }
    }
}

// the symbol of c from r = c^((p-1)/2), both canonical
template <class W>
__device__ __forceinline__ unsigned legendre_code_of(const W& c, const W& r) {
    const bool zero = (explog_limb(c, 0) | explog_limb(c, 1) | explog_limb(c, 2)) == 0;
    const bool is_one = explog_limb(r, 0) == 1 && (explog_limb(r, 1) | explog_limb(r, 2)) == 0;
    return zero ? (unsigned)LEGENDRE_ZERO : is_one ? (unsigned)LEGENDRE_RESIDUE : (unsigned)LEGENDRE_NONRESIDUE;
}
template <class F>
struct PowPutLegendre {
    typedef Pack<typename F::word> P;
    uint8_t* __restrict__ code;
    __device__ __forceinline__ void pack(size_t i, const P& x, const P& r) const {
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < P::N; ++q) v = iszero_code_put(v, q, legendre_code_of(x.w[q], r.w[q]));
        st_codes<P::N>(code + iszero_code_at(P::N, i), v);
    }
    __device__ __forceinline__ void elem(size_t e, const typename F::word& x, const typename F::word& r) const {
        code[e] = (uint8_t)legendre_code_of(x, r);
    }
};
template <class F>
__global__ __launch_bounds__(BLOCK) void k_legendre_code(F f, const typename F::elem* __restrict__ c, ExpArgs ex, uint8_t* __restrict__ code,
                                                          size_t nvec, size_t n) {
    pow_stream<F, false>(f, c, ex, nvec, n, PowPutLegendre<F>{code});
}

template <class F>
__device__ __forceinline__ typename F::word iszero_finish_value(const F& f, unsigned code, const typename F::word& z,
                                                                const typename F::word& one) {
    const typename F::word nz = f.sub(one, z);
    return code == LEGENDRE_NONRESIDUE ? z : code == LEGENDRE_RESIDUE ? nz : one;
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_iszero_finish(F f, const uint8_t* __restrict__ code, const typename F::elem* __restrict__ z,
                                                          typename F::elem* __restrict__ out, FlatPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    const W one = ff_one_elem(f);
    if (pl.vec) {
        const MP* zv = reinterpret_cast<const MP*>(z);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const auto r0 = ldgw_issue<false>(zv + g);
            const uint32_t cv = ld_codes<PK::N>(code + iszero_code_at(PK::N, g));
            const PK xz = ldgw_finish(r0);
            PK y;
#pragma unroll
            for (int q = 0; q < PK::N; ++q) y.w[q] = iszero_finish_value<F>(f, iszero_code_of(cv, q), xz.w[q], one);
            stgw<false>(ov + g, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) st_elem<F>(out, g, iszero_finish_value<F>(f, code[g], ld_elem<F>(z, g), one));
    }
}

}  // namespace ffgpu
