// matmul_tile_body.hpp -- the tile body of the dense VALU product: the statements of one workgroup that computes one
// BM x BN tile of C = A @ B.  NO include guard and no namespace: this text is included INSIDE the braces of k_matmul
// (matmul.hpp) and of k_matmul_stack_tiled (matmul_stack.hpp), after each has defined
//     F, TM, TN          the policy and the outputs per thread (template parameters)
//     f                  the policy object
//     A, B, C            the three matrices (const elem*, const elem*, elem*), lda, ldb, ldc their leading dimensions
//     M, K, N            the shape; K may already be one split-K slice
//     tx, ty             threadIdx.x & 15, threadIdx.x >> 4: the thread's place in the 16 x 16 workgroup
//     m0, n0             the origin of this workgroup's tile
// As a __device__ function called from both kernels the same statements took up to 60 more registers inside k_matmul
// (profiles/r12_matmul_stack.md; profiles/r13_matmul_one_body.md has its timings), so the text is shared and expanded
// twice instead.  The running sums keep their hand-written form here: with DotSum (kernels.hpp) one instantiation gained
// scratch (profiles/r13_matmul_one_body.md).
// Thread ownership inside a tile (ty + 16 i, tx + 16 j) is restated as stack_tile_row / stack_tile_col in
// matmul_stack_geom.hpp for the host walk.
    typedef typename F::word W;
    static_assert(F::EPW == 1, "packed fields use the byte-wise instantiation");
    // multi-limb 2^k - c primes (round 6): the tiles are staged as 28-bit DIGITS and every term is NL^2 multiply-adds into
    // column sums (fields.hpp LazyDot), reduced every 32 terms -- ~100 instructions per term with the 128-bit limb arithmetic
    constexpr bool LZ = DotAcc<F>::lazy;
    constexpr int NL = DotAcc<F>::NL;
    constexpr int BK = 16, BM = 16 * TM, BN = 16 * TN, FLUSH = DotAcc<F>::FLUSH;
    static_assert(FLUSH % BK == 0, "the flush test follows whole k-steps");
    using Acc = typename DotAcc<F>::type;
    __shared__ W As[LZ ? 1 : BK][LZ ? 1 : BM + 1];
    __shared__ W Bs[LZ ? 1 : BK][LZ ? 1 : BN + 1];
    __shared__ uint32_t Ad[LZ ? BK : 1][LZ ? BM + 1 : 1][NL];
    __shared__ uint32_t Bd[LZ ? BK : 1][LZ ? BN + 1 : 1][NL];
    Acc acc[TM][TN];
    W tot[TM][TN];
    bool have = false;
    auto zero = [&](Acc& a_) {
        if constexpr (LZ) f.lacc_zero(a_); else f.acc_zero(a_);
    };
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) zero(acc[i][j]);
    int since = 0;
    for (int k0 = 0; k0 < K; k0 += BK) {
        // stage A (BM x BK) transposed and B (BK x BN)
        for (int idx = threadIdx.x; idx < BM * BK; idx += BLOCK) {
            int mm = idx / BK, kk = idx % BK;
            int gm = m0 + mm, gk = k0 + kk;
            const bool ok = gm < M && gk < K;      // out-of-range: read element 0, then zero it
            const W v = ff_keep_if<W>(f.prep(ld_elem<F>(A, ok ? (size_t)gm * lda + gk : 0)), ok);
            if constexpr (LZ) {
                uint32_t d[NL];
                f.lacc_digits(v, d);
#pragma unroll
                for (int t_ = 0; t_ < NL; ++t_) Ad[kk][mm][t_] = d[t_];
            } else {
                As[kk][mm] = v;
            }
        }
        for (int idx = threadIdx.x; idx < BK * BN; idx += BLOCK) {
            int kk = idx / BN, nn = idx % BN;
            int gk = k0 + kk, gn = n0 + nn;
            const bool ok = gk < K && gn < N;
            const W v = ff_keep_if<W>(ld_elem<F>(B, ok ? (size_t)gk * ldb + gn : 0), ok);
            if constexpr (LZ) {
                uint32_t d[NL];
                f.lacc_digits(v, d);
#pragma unroll
                for (int t_ = 0; t_ < NL; ++t_) Bd[kk][nn][t_] = d[t_];
            } else {
                Bs[kk][nn] = v;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < BK; ++kk) {
            if constexpr (LZ) {
                uint32_t a[TM][NL], b[TN][NL];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int t_ = 0; t_ < NL; ++t_) a[i][t_] = Ad[kk][ty + 16 * i][t_];
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int t_ = 0; t_ < NL; ++t_) b[j][t_] = Bd[kk][tx + 16 * j][t_];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) f.lacc_mac_digits(acc[i][j], a[i], b[j]);
            } else {
                W a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = As[kk][ty + 16 * i];
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = Bs[kk][tx + 16 * j];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) f.acc_mac(acc[i][j], a[i], b[j]);
            }
        }
        __syncthreads();
        since += BK;
        if (since >= FLUSH) {   // keep the unreduced accumulators inside their headroom (2^8 products; digit columns: 32)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    W part;
                    if constexpr (LZ) part = f.lacc_reduce(acc[i][j]); else part = f.acc_reduce(acc[i][j]);
                    tot[i][j] = have ? f.add(tot[i][j], part) : part;
                    zero(acc[i][j]);
                }
            have = true;
            since = 0;
        }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            int gm = m0 + ty + 16 * i, gn = n0 + tx + 16 * j;
            if (gm < M && gn < N) {
                W r;
                if constexpr (LZ) r = f.lacc_reduce(acc[i][j]); else r = f.acc_reduce(acc[i][j]);
                if (have) r = f.add(tot[i][j], r);
                st_elem<F>(C, (size_t)gm * ldc + gn, r);
            }
        }
