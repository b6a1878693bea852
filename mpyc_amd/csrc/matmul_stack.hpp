// matmul_stack.hpp -- a stack of matrix products in one launch: C[b] = A[b] @ B[b], b < batch (NumPy's matmul on
// stacks of matrices: finfields.py:1126-1135 hands them to the object matmul, the local product of runtime.np_matmul,
// runtime.py:2481-2541).  Shapes and ownership: matmul_stack_geom.hpp.  Included by kernels.hpp after matmul.hpp.
#pragma once
#include "matmul_stack_geom.hpp"

namespace ffgpu {

// what both kernels take besides the three pointers; strides and leading dimensions in elements, stride 0 = one matrix
// shared by the whole stack
struct StackArgs {
    size_t lda, sa, ldb, sb, ldc, sc, batch;
    int M, K, N;
    int P, KC, rows_a, rows_b;    // packed shape (StackPlan)
    int vec_a, vec_b;             // packed shape: the operand's P matrices are one aligned contiguous run -> 16-byte loads
    int bm, bn;                   // tiled shape
    size_t tiles_m, tiles_n;
};

// ---- packed shape: M N <= BLOCK, P matrices per workgroup, one output per thread --------------------------------
// The inner operation is k_matmul's: the policy's lazily reduced multiply-accumulate (acc_mac, or 28-bit digit columns
// for the multi-limb 2^k - c primes, staged in LDS as digits), flushed every DotAcc<F>::FLUSH terms (DotSum,
// kernels.hpp); the packed-byte fields multiply four terms per SWAR word (k_matmul_bytes).  Results are canonical, so
// they equal k_matmul's bit for bit.
// Staging: the P matrices of a contiguous stack are ONE run in memory, read by consecutive threads (16 bytes per lane
// for elements of up to 8 bytes when the run is aligned; wider elements are 12 to 24 bytes per lane as they are).
// LDS layout: operand X as [term][digit][row], row = (matrix in the workgroup) * M + i for A, * N + j for B.  For a fixed
// term the threads of a wave read consecutive rows of B and a few broadcast rows of A: no read conflicts on a bank.  The
// staging writes of A are a transpose (consecutive threads hold consecutive terms of a row) and do conflict, up to
// min(K, 32) ways; every element is written once and read N times, and B's writes are consecutive.
template <class F>
__global__ __launch_bounds__(BLOCK) void k_matmul_stack_packed(F f, const typename F::elem* __restrict__ A,
                                                                const typename F::elem* __restrict__ B,
                                                                typename F::elem* __restrict__ C, StackArgs s) {
    typedef typename F::word W;
    typedef typename F::elem E;
    constexpr bool BY = F::EPW > 1;                    // one element per byte
    constexpr bool LZ = !BY && DotAcc<F>::lazy;
    constexpr int NL = DotAcc<F>::NL;
    constexpr int FLUSH = DotAcc<F>::FLUSH;
    extern __shared__ __attribute__((aligned(16))) unsigned char stack_smem[];
    const int M = s.M, K = s.K, N = s.N, P = s.P, tid = threadIdx.x;
    const size_t b0 = (size_t)blockIdx.x * (size_t)P;
    const int np = s.batch - b0 < (size_t)P ? (int)(s.batch - b0) : P;      // matrices of this workgroup
    size_t b;
    int pl, i, j;
    const bool active = stack_packed_owner(P, M, N, s.batch, blockIdx.x, tid, b, pl, i, j);
    const int ra = s.sa ? pl * M + i : i, rb = s.sb ? pl * N + j : j;
    const int rows_a = s.rows_a, rows_b = s.rows_b;
    unsigned char* const sA = stack_smem;
    unsigned char* const sB = stack_smem + (size_t)rows_a * s.KC * (BY ? 1 : LZ ? 4 * NL : (int)sizeof(W));

    auto put = [&](unsigned char* base, int rows, int kk, int row, const W& v) {
        if constexpr (BY) {
            base[kk * rows + row] = (uint8_t)v;
        } else if constexpr (LZ) {
            uint32_t d[NL];
            DotAcc<F>::digits(f, v, d);
            uint32_t* q = reinterpret_cast<uint32_t*>(base);
#pragma unroll
            for (int t_ = 0; t_ < NL; ++t_) q[(kk * NL + t_) * rows + row] = d[t_];
        } else {
            reinterpret_cast<W*>(base)[kk * rows + row] = v;
        }
    };
    // element (p, u, v) of an operand chunk, v fastest.  A: u = row i, v = term; B: u = term, v = column j.
    auto stage = [&](auto is_a, const E* __restrict__ X, size_t ld, size_t stride, int U, int V, int k0, int vec,
                     unsigned char* dst, int rows) {
        constexpr bool ISA = decltype(is_a)::value;
        const int nmat = stride ? np : 1, uv = U * V, cnt = nmat * uv;
        const E* __restrict__ base = X + b0 * stride;
        auto place = [&](int e, W w) {
            const int p = e / uv, r = e - p * uv, u = r / V, v = r - u * V;
            if constexpr (ISA) {
                if constexpr (!BY) w = f.prep(w);
                put(dst, rows, v, p * U + u, w);
            } else {
                put(dst, rows, u, p * V + v, w);
            }
        };
        int done = 0;
        if constexpr (sizeof(E) <= 8) {
            if (vec) {                                  // the whole chunk is one aligned run (KC == K)
                constexpr int EPL = 16 / (int)sizeof(E);
                const int nv = cnt / EPL;
                for (int idx = tid; idx < nv; idx += BLOCK) {
                    const ff_u32x4 raw = *reinterpret_cast<const ff_u32x4*>(base + (size_t)idx * EPL);
                    E tmp[EPL];
                    __builtin_memcpy(tmp, &raw, 16);
#pragma unroll
                    for (int q = 0; q < EPL; ++q) place(idx * EPL + q, (W)tmp[q]);
                }
                done = nv * EPL;
            }
        }
        for (int e = done + tid; e < cnt; e += BLOCK) {
            const int p = e / uv, r = e - p * uv, u = r / V, v = r - u * V;
            const size_t g = ISA ? (size_t)p * stride + (size_t)u * ld + (size_t)(k0 + v)
                                 : (size_t)p * stride + (size_t)(k0 + u) * ld + (size_t)v;
            place(e, ld_elem<F>(base, g));
        }
    };

    DotSum<F> sum;
    uint32_t bacc = 0;
    bool have = false;
    int since = 0;
    if constexpr (!BY) sum.zero(f);
    for (int k0 = 0; k0 < K; k0 += s.KC) {
        const int kc = K - k0 < s.KC ? K - k0 : s.KC;
        stage(std::true_type(), A, s.lda, s.sa, M, kc, k0, s.vec_a, sA, rows_a);
        stage(std::false_type(), B, s.ldb, s.sb, kc, N, k0, s.vec_b, sB, rows_b);
        __syncthreads();
        if (active) {
            if constexpr (BY) {
                for (int kk = 0; kk < kc; kk += 4) {    // four terms per SWAR product; bytes past the chunk are zero terms
                    uint32_t av = 0, bv = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (kk + q < kc) {
                            av |= (uint32_t)sA[(kk + q) * rows_a + ra] << (8 * q);
                            bv |= (uint32_t)sB[(kk + q) * rows_b + rb] << (8 * q);
                        }
                    bacc ^= f.mul(av, bv);
                }
            } else {
                for (int kk = 0; kk < kc; ++kk) {
                    if constexpr (LZ) {
                        const uint32_t* qa = reinterpret_cast<const uint32_t*>(sA);
                        const uint32_t* qb = reinterpret_cast<const uint32_t*>(sB);
                        uint32_t a[NL], x[NL];
#pragma unroll
                        for (int t_ = 0; t_ < NL; ++t_) {
                            a[t_] = qa[(kk * NL + t_) * rows_a + ra];
                            x[t_] = qb[(kk * NL + t_) * rows_b + rb];
                        }
                        sum.mac_digits(f, a, x);
                    } else {
                        sum.mac(f, reinterpret_cast<const W*>(sA)[kk * rows_a + ra], reinterpret_cast<const W*>(sB)[kk * rows_b + rb]);
                    }
                    if (++since == FLUSH) {             // keep the unreduced accumulator inside its headroom
                        sum.flush(f, have);
                        have = true;
                        since = 0;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    E* __restrict__ out = C + b * s.sc + (size_t)i * s.ldc + (size_t)j;
    if constexpr (BY) {
        bacc ^= bacc >> 16;
        bacc ^= bacc >> 8;
        out[0] = (uint8_t)(bacc & 0xffu);
    } else {
        st_elem<F>(out, 0, sum.result(f, have));
    }
}

// ---- tiled shape: k_matmul's tile body, the matrix index folded into a flat tile index --------------------------
// The second expansion of matmul_tile_body.hpp.  It sits in a function of its own, not in the kernel, for the
// __restrict__ of the per-matrix pointers: expanded in the kernel, where only the stack's base pointers are parameters,
// k_matmul_stack_tiled<MONT128, 2, 2> ran 4 to 17 % slower (profiles/r13_matmul_one_body.md).
template <class F, int TM, int TN>
__device__ __forceinline__ void stack_tile(const F& f, const typename F::elem* __restrict__ A, size_t lda,
                                           const typename F::elem* __restrict__ B, size_t ldb,
                                           typename F::elem* __restrict__ C, size_t ldc, int M, int K, int N,
                                           const int m0, const int n0) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#include "matmul_tile_body.hpp"
}
template <class F, int TM, int TN>
__global__ __launch_bounds__(BLOCK) void k_matmul_stack_tiled(F f, const typename F::elem* __restrict__ A,
                                                               const typename F::elem* __restrict__ B,
                                                               typename F::elem* __restrict__ C, StackArgs s) {
    size_t b;
    int m0, n0;
    stack_tile_of(blockIdx.x, s.tiles_m, s.tiles_n, 16 * TM, 16 * TN, b, m0, n0);
    stack_tile<F, TM, TN>(f, A + b * s.sa, s.lda, B + b * s.sb, s.ldb, C + b * s.sc, s.ldc, s.M, s.K, s.N, m0, n0);
}
template <class F>
__global__ __launch_bounds__(BLOCK) void k_matmul_stack_tiled_bytes(F f, const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                                     uint8_t* __restrict__ C, StackArgs s) {
    size_t b;
    int m0, n0;
    stack_tile_of(blockIdx.x, s.tiles_m, s.tiles_n, 32, 32, b, m0, n0);
    matmul_bytes_tile<F>(f, A + b * s.sa, s.lda, B + b * s.sb, s.ldb, C + b * s.sc, s.ldc, s.M, s.K, s.N, m0, n0);
}

}  // namespace ffgpu
