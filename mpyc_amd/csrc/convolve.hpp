// convolve.hpp -- full convolution of two field arrays in one kernel (np.convolve on field arrays: finfields.py:796-801,
// the local part of runtime.np_convolve, runtime.py:2627).  Included by kernels.hpp after matmul.hpp.
#pragma once
#include "convolve_geom.hpp"

namespace ffgpu {

// c[k] = sum_j a[k - j] v[j] over the field, na >= nv >= 1.  Geometry and index arithmetic: convolve_geom.hpp.  The inner
// operation is k_matmul's: the lazily reduced multiply-accumulate of the policy (acc_mac, or 28-bit digit columns for the
// multi-limb 2^k - c primes, whose operands are staged in LDS as digits), reduced every DotAcc<F>::FLUSH terms.  The
// lanes of a tap group read ONE tap per step (same address: LDS broadcast; the wide shape's group is the whole wave) and
// consecutive window elements (digit-major for the digit policies), the groups of a wave neighbouring taps and
// overlapping windows, so no access conflicts on a bank.  The taps are the constant operand: f.prep, as for A in k_matmul.
// The next chunk's element is fetched into a register before this chunk is multiplied, so the load's latency hides
// behind the arithmetic even with one workgroup per compute unit.  Memory: reads a and v (a about TV / TO + 1 times,
// from cache), writes out once; no scratch.  Outputs are stored with the default cache policy (not a tracked hand-off
// producer, like ffgpu_matmul).
template <class F, class S>
__global__ __launch_bounds__(BLOCK) void k_convolve(F f, const typename F::elem* __restrict__ a, size_t na,
                                                     const typename F::elem* __restrict__ v, size_t nv,
                                                     typename F::elem* __restrict__ out) {
    typedef typename F::word W;
    constexpr int R = S::R;
    static_assert((int)S::THREADS == (int)BLOCK, "ConvShape is laid out for the library's workgroup");
    constexpr bool LZ = DotAcc<F>::lazy;
    constexpr int NL = DotAcc<F>::NL;
    constexpr int FLUSH = DotAcc<F>::FLUSH;
    static_assert(FLUSH % S::PER == 0, "the flush test follows whole chunks");
    using Acc = typename DotAcc<F>::type;
    __shared__ W Ws[LZ ? 1 : S::WIN];
    __shared__ W Ts[LZ ? 1 : S::TV];
    __shared__ uint32_t Wd[NL][LZ ? S::WIN : 1];
    __shared__ uint32_t Td[LZ ? S::TV : 1][NL];
    __shared__ W red[S::G][S::TO];
    const int tid = threadIdx.x, o = tid % S::OL, g = tid / S::OL;
    const size_t nout = na + nv - 1;
    const size_t k0 = (size_t)blockIdx.x * S::TO;
    size_t jlo, jhi;
    conv_tap_range(k0, S::TO, na, nv, jlo, jhi);
    // staging duty: threads 0 .. WIN-1 one window slot each, the last TV threads one tap each
    const bool is_win = tid < S::WIN, is_tap = tid >= BLOCK - S::TV;
    const int ti = tid - (BLOCK - S::TV);
    auto fetch = [&](size_t j0) -> W {
        if (is_win) {
            const int64_t idx = conv_win_index(k0, j0, S::TV, tid);
            const bool ok = idx >= 0 && idx < (int64_t)na;          // out-of-range: read element 0, then zero it
            return ff_keep_if<W>(ld_elem<F>(a, ok ? (size_t)idx : 0), ok);
        }
        if (is_tap) {
            const size_t j = j0 + (size_t)ti;
            const bool ok = j < jhi;
            return ff_keep_if<W>(f.prep(ld_elem<F>(v, ok ? j : 0)), ok);
        }
        return W();
    };
    Acc acc[R];
    W tot[R];
    bool have = false;
    auto zero = [&](Acc& a_) {
        if constexpr (LZ) f.lacc_zero(a_); else f.acc_zero(a_);
    };
    auto reduce = [&](const Acc& a_) -> W {
        if constexpr (LZ) return f.lacc_reduce(a_); else return f.acc_reduce(a_);
    };
#pragma unroll
    for (int r = 0; r < R; ++r) zero(acc[r]);
    int since = 0;
    W nxt = fetch(jlo);
    for (size_t j0 = jlo; j0 < jhi; j0 += S::TV) {
        if (is_win || is_tap) {
            if constexpr (LZ) {
                uint32_t d[NL];
                f.lacc_digits(nxt, d);
#pragma unroll
                for (int t_ = 0; t_ < NL; ++t_) {
                    if (is_win) Wd[t_][tid] = d[t_]; else Td[ti][t_] = d[t_];
                }
            } else {
                if (is_win) Ws[tid] = nxt; else Ts[ti] = nxt;
            }
        }
        __syncthreads();
        if (j0 + S::TV < jhi) nxt = fetch(j0 + S::TV);
        const int tv = jhi - j0 < (size_t)S::TV ? (int)(jhi - j0) : (int)S::TV;
        for (int jj = g; jj < tv; jj += S::G) {
            if constexpr (LZ) {
                uint32_t t[NL];
#pragma unroll
                for (int t_ = 0; t_ < NL; ++t_) t[t_] = Td[jj][t_];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    uint32_t x[NL];
                    const int slot = conv_win_slot(o + S::OL * r, jj, S::TV);
#pragma unroll
                    for (int t_ = 0; t_ < NL; ++t_) x[t_] = Wd[t_][slot];
                    f.lacc_mac_digits(acc[r], t, x);
                }
            } else {
                const W t = Ts[jj];
#pragma unroll
                for (int r = 0; r < R; ++r) f.acc_mac(acc[r], t, Ws[conv_win_slot(o + S::OL * r, jj, S::TV)]);
            }
        }
        __syncthreads();
        since += S::PER;
        if (conv_flush_due(since, S::PER, FLUSH)) {   // keep the unreduced accumulators inside their headroom
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const W part = reduce(acc[r]);
                tot[r] = have ? f.add(tot[r], part) : part;
                zero(acc[r]);
            }
            have = true;
            since = 0;
        }
    }
    // add the G partial sums of every output
#pragma unroll
    for (int r = 0; r < R; ++r) {
        W part = reduce(acc[r]);
        if (have) part = f.add(tot[r], part);
        red[g][o + S::OL * r] = part;
    }
    __syncthreads();
    for (int i = tid; i < S::TO; i += BLOCK) {
        W s = red[0][i];
#pragma unroll
        for (int q = 1; q < S::G; ++q) s = f.add(s, red[q][i]);
        if (k0 + (size_t)i < nout) st_elem<F>(out, k0 + (size_t)i, s);
    }
}

}  // namespace ffgpu
