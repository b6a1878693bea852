// rbits.hpp -- the two local steps of secure random bits over a prime field, the PRSS branch of runtime.np_random_bits
// (runtime.py:4243-4272): with r a random sharing and z a degree-2t sharing of zero, r^2 + z is opened at threshold 2t, and
// r (r^2)^(-1/2) is a uniform +-1 wherever the square is not 0.  Included by kernels.hpp after iszero.hpp.  Index
// arithmetic and plans: rbits_geom.hpp.
//
//   k_rbits_open     c[h] = sum_i lam[i] (r_i[h]^2 + z_i[h]), i < k; *zeros += #{h : c[h] == 0}        the value that is opened
//   k_rbits_finish   s = c[h]^((3p - 5) / 4);  b_i[h] = r_i[h] (s A) + B, i < m;  0 in every row where c[h] == 0
// with host scalars A = 2^f, B = 0 for signed bits (+-1 2^f) and A = B = (p + 1) / 2 2^f for bits in {0, 1} 2^f:
// (r s + 1) (p + 1) / 2 2^f = r (s A) + A.  The rows are separate arrays of n entries, one pointer each.
//
// k_rbits_open is the recombination with other operands: the accumulator and its flush are DotAcc / F::acc of k_recombine /
// k_recombine_any, the row count a template parameter up to rbits_fused_rows() with all 2 k loads of a pack in flight (MAXK
// rows; 5 for 24-byte elements, whose 2 k raw wave loads no longer fit the registers beyond that: 255 VGPRs at k = 7, AGPR
// copies at k = 9), a run-time count by elements above that.  A term lam r^2 has three factors, so the square is a reduced
// product; r^2 + z is one modular addition, and the Lagrange sum is k lazy products into one accumulator with ONE reduction
// per entry: 2 k rows read, one written, where the composed calls (k muladd, one recombination) move 3 k + k + 1.  A thread
// counts its zeros in a register; the wave adds them up by shuffles and lane 0 issues one vector atomic on the int32
// counter -- only when the wave saw a zero at all, which has probability 64 / p.
//
// k_rbits_finish is the exponentiation of k_pow with other ends (pow_stream, kernels.hpp): the same chain for the exponent
// (3p - 5) / 4 -- which ffgpu_pow hands over as ((p - 3) / 4, post) --, the same plan, grid and launch bounds.  The power of
// the PUBLIC value is formed once and serves every party's row: per row one load, one product, one addition, one store
// behind some hundred products, moved by the lane as k_pow moves its operand and its power (ldg / stg: bound by its products,
// the kernel gains nothing from wave-contiguous accesses of 24-byte elements).  A row is read before it is written by the
// same thread and by no other, so b_i may be r_i.
//
// Memory policy: c is read by the finish, the bits by the next protocol step: default-policy stores; streamed loads nt.
#pragma once
#include "rbits_geom.hpp"

namespace ffgpu {

static_assert(RBITS_FUSED_ROWS == MAXK && RBITS_FUSED_ROWS_24 <= MAXK && RBITS_MAX_ROWS == MAXK_ANY,
              "rbits_geom.hpp restates the row limits of the recombination");

template <class W>
__device__ __forceinline__ bool rbits_is_zero(const W& c) {
    return (explog_limb(c, 0) | explog_limb(c, 1) | explog_limb(c, 2)) == 0;
}

// the zeros a thread counted, summed over the wave (every lane arrives here: the streaming loops have ended), added once
__device__ __forceinline__ void rbits_count_add(int cnt, int* zeros) {
#pragma unroll
    for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (zeros && cnt && __lane_id() == 0) atomicAdd(zeros, cnt);
}

template <class F, int K>
struct RbitsOpenArgs {
    const typename F::elem* r[K];
    const typename F::elem* z[K];
    typename F::word lam[K];            // prepared constants
};

template <class F, int K>
__global__ __launch_bounds__(BLOCK) void k_rbits_open(F f, RbitsOpenArgs<F, K> ra, typename F::elem* __restrict__ out, int* zeros,
                                                       size_t nvec, size_t n) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    int cnt = 0;
    for (size_t i = gid; i < nvec; i += gsz) {
        P xr[K], xz[K];
        {
            decltype(ldgw_issue<true>(reinterpret_cast<const MP*>(ra.r[0]))) rr[K], rz[K];
#pragma unroll
            for (int j = 0; j < K; ++j) rr[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.r[j]) + i);
#pragma unroll
            for (int j = 0; j < K; ++j) rz[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.z[j]) + i);
#pragma unroll
            for (int j = 0; j < K; ++j) xr[j] = ldgw_finish(rr[j]);
#pragma unroll
            for (int j = 0; j < K; ++j) xz[j] = ldgw_finish(rz[j]);
        }
        P y;
#pragma unroll
        for (int q = 0; q < P::N; ++q) {
            DotAcc<F> s;
            s.zero(f);
#pragma unroll
            for (int j = 0; j < K; ++j) s.mac(f, ra.lam[j], f.add(f.mul(xr[j].w[q], xr[j].w[q]), xz[j].w[q]));
            y.w[q] = s.reduce(f);
            cnt += rbits_is_zero(y.w[q]) ? 1 : 0;
        }
        stgw<false>(reinterpret_cast<MP*>(out) + i, y);
    }
    const size_t done = nvec * (size_t)(P::N * F::EPW);
    for (size_t e = done + gid; e < n; e += gsz) {
        typename F::acc s;
        f.acc_zero(s);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const W x = ld_elem<F>(ra.r[j], e);
            f.acc_mac(s, ra.lam[j], f.add(f.mul(x, x), ld_elem<F>(ra.z[j], e)));
        }
        const W y = f.acc_reduce(s);
        cnt += rbits_is_zero(y) ? 1 : 0;
        st_elem<F>(out, e, y);
    }
    rbits_count_add(cnt, zeros);
}

template <class F>
struct RbitsOpenArgsAny {
    const typename F::elem* r[MAXK_ANY];
    const typename F::elem* z[MAXK_ANY];
    typename F::word lam[MAXK_ANY];
};

template <class F>
__global__ __launch_bounds__(BLOCK) void k_rbits_open_any(F f, RbitsOpenArgsAny<F> ra, int k, typename F::elem* __restrict__ out, int* zeros,
                                                           size_t n) {
    typedef typename F::word W;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    int cnt = 0;
    for (size_t e = gid; e < n; e += gsz) {
        typename F::acc s;
        f.acc_zero(s);
        for (int j = 0; j < k; ++j) {
            const W x = ld_elem<F>(ra.r[j], e);
            f.acc_mac(s, ra.lam[j], f.add(f.mul(x, x), ld_elem<F>(ra.z[j], e)));
        }
        const W y = f.acc_reduce(s);
        cnt += rbits_is_zero(y) ? 1 : 0;
        st_elem<F>(out, e, y);
    }
    rbits_count_add(cnt, zeros);
}

// (no __restrict__ on the rows: b[i] may be r[i])
template <class F>
struct RbitsFinishArgs {
    const typename F::elem* r[MAXK_ANY];
    typename F::elem* b[MAXK_ANY];
    typename F::word A, B;
    int m;
};

template <class F>
__device__ __forceinline__ typename F::word rbits_bit_value(const F& f, bool zero, const typename F::word& r, const typename F::word& u,
                                                            const typename F::word& B) {
    typedef typename F::word W;
    const W v = f.add(f.mul(r, u), B);
    return zero ? W() : v;
}

template <class F>
struct PowPutRbits {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const F& f;
    const RbitsFinishArgs<F>& fa;
    __device__ __forceinline__ void pack(size_t i, const P& x, const P& s) const {
        P u;
        bool zero[P::N];
#pragma unroll
        for (int q = 0; q < P::N; ++q) {
            u.w[q] = f.mul(s.w[q], fa.A);
            zero[q] = rbits_is_zero(x.w[q]);
        }
        for (int j = 0; j < fa.m; ++j) {
            const P r = ldg<true>(reinterpret_cast<const MP*>(fa.r[j]) + i);
            P y;
#pragma unroll
            for (int q = 0; q < P::N; ++q) y.w[q] = rbits_bit_value<F>(f, zero[q], r.w[q], u.w[q], fa.B);
            stg<false>(reinterpret_cast<MP*>(fa.b[j]) + i, y);
        }
    }
    __device__ __forceinline__ void elem(size_t e, const W& x, const W& s) const {
        const W u = f.mul(s, fa.A);
        const bool zero = rbits_is_zero(x);
        for (int j = 0; j < fa.m; ++j) st_elem<F>(fa.b[j], e, rbits_bit_value<F>(f, zero, ld_elem<F>(fa.r[j], e), u, fa.B));
    }
};
template <class F>
__global__ __launch_bounds__(BLOCK) void k_rbits_finish(F f, const typename F::elem* __restrict__ c, ExpArgs ex, RbitsFinishArgs<F> fa,
                                                         size_t nvec, size_t n) {
    pow_stream<F, false>(f, c, ex, nvec, n, PowPutRbits<F>{f, fa});
}

}  // namespace ffgpu
