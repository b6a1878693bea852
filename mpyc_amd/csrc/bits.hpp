// bits.hpp -- the local steps of bit decomposition over a prime field, runtime.np_to_bits (runtime.py:4391-4456) with the
// prefix-carry network of np_add_bits (runtime.py:4301-4334), for one party's shares.  Included by kernels.hpp after
// sort.hpp.  The network as rounds and the plan of the level kernels: bits_geom.hpp; tiles, chunks and LDS layout of the
// element-major bit shares: sgn_geom.hpp (the functions of the secure comparison, reused as they are).
//
//   k_bits_mask     masked[h] = a[h] + offset + rdivl[h] 2^l - sum_k rbits[h l + k] 2^k                   the value that is opened
//   k_bits_expand   g[k n + h] = cb_k ? r : 0,  p[k n + h] = cb_k ? 1 - r : r                            leaves of the network, public c
//   k_carry_prod    out[j n + h] = (j < Rc ? G : P)[q_j n + h] * P[k_j n + h]                            a round's local products
//   k_carry_apply   v = sum_s lam[s] rows[s][j n + h];  G[k_j n + h] += v (j < Rc),  P[k_j n + h] = v     in place
//   k_bits_finish   out[h l + k] = rbits[h l + k] + cb_k - 2 G[k n + h] + G[(k-1) n + h]                  element-major
// Bit index k runs least significant first.  G, P and the compact products are bit-major (row k at k n), rbits and the
// result element-major.
//
// mask, expand and finish own a tile of SGN_TILE elements per workgroup and stage its bit shares through LDS a chunk of
// columns at a time (sgn_stage); finish writes its results back into the staged tile and moves it out with the same
// units, so both its element-major sides are coalesced.  The two level kernels are streaming kernels, one unit per thread
// (BitsPlan): workgroup row y is product row y, so the (k, q) entry of the table is uniform over a workgroup.
//
// Memory policy: the bit shares are read once: non-temporal loads.  G and P are read and written round after round, the
// products feed the re-sharing at once: default policy.  The sub-share rows of k_carry_apply: share_rows.hpp.
#pragma once
#include "bits_geom.hpp"
#include "sgn_geom.hpp"

namespace ffgpu {

// the inverse of sgn_lds_elem: the element that starts at LDS word p
template <class F>
__device__ __forceinline__ void bits_lds_put(uint32_t* p, const typename F::word& w) {
    constexpr int EW = sizeof(typename F::elem) / 4;
    if constexpr (EW == 1) {
        p[0] = (uint32_t)w;
    } else if constexpr (EW == 2) {
        p[0] = (uint32_t)w;
        p[1] = (uint32_t)((uint64_t)w >> 32);
    } else if constexpr (EW == 3) {
        p[0] = (uint32_t)w.lo;
        p[1] = (uint32_t)(w.lo >> 32);
        p[2] = (uint32_t)w.hi;
    } else if constexpr (EW == 4) {
        p[0] = (uint32_t)w.lo;
        p[1] = (uint32_t)(w.lo >> 32);
        p[2] = (uint32_t)w.hi;
        p[3] = (uint32_t)(w.hi >> 32);
    } else {
        static_assert(EW == 6, "element sizes: 4, 8, 12, 16, 24 bytes");
        p[0] = (uint32_t)w.lo;
        p[1] = (uint32_t)(w.lo >> 32);
        p[2] = (uint32_t)w.mid;
        p[3] = (uint32_t)(w.mid >> 32);
        p[4] = (uint32_t)w.hi;
        p[5] = (uint32_t)(w.hi >> 32);
    }
}

// Columns i0 .. i0 + cols - 1 of the tile, LDS -> global: sgn_stage backwards, the same units at the same addresses.
template <class F>
__device__ __forceinline__ void bits_unstage(const uint32_t* lds, typename F::elem* __restrict__ out, size_t h0, unsigned rows, int l,
                                             int i0, int cols) {
    constexpr size_t EB = sizeof(typename F::elem);
    constexpr int UW = sgn_unit_words(EB);
    uint32_t* g = reinterpret_cast<uint32_t*>(out);
    SgnCursor c = sgn_cursor(threadIdx.x, sgn_units_per_row(cols, EB));
    while (c.row < rows) {
        const unsigned at = sgn_unit_lds_word(c.row, c.u, EB);
        uint32_t* dst = g + sgn_unit_src_word(h0, c.row, l, i0, c.u, EB);
        if constexpr (UW == 2) {
            ff_u32x2 x;
            x.x = lds[at];
            x.y = lds[at + 1];
            *reinterpret_cast<ff_u32x2*>(dst) = x;
        } else {
            dst[0] = lds[at];
        }
        sgn_cursor_next(c);
    }
}

// Occupancy: as sgn.hpp states for mask and expand -- a workgroup is four waves, LDS admits four workgroups per compute
// unit, and the registers are held to the same four waves per SIMD.
// ---- mask ------------------------------------------------------------------------------------------------------------------
// (runtime.py:4414-4415, 4446: r_modl = np.sum(r_bits << shifts, axis=1); a + offset + (r_divl << l) - r_modl.)  The
// weighted row sum by Horner from the most significant bit down, acc = 2 acc + r_k: the chunks are staged last to first
// and every thread walks its columns backwards.  One product, rdivl 2^l.
// What a thread of the mask kernels holds for its element h once the tile is walked: a[h], rdivl[h] and
// acc = sum_k rbits[h l + k] 2^k.  The body of k_bits_mask and of k_trunc_mask (fxp.hpp): the two differ in the sign of acc and
// in what they store.  lds: the workgroup's sgn_lds_words(EB) words.
template <class F>
struct BitsMaskSum {
    typename F::word av, rd, acc;
    size_t h;
    bool live, wave_full;
};
template <class F>
__device__ __forceinline__ BitsMaskSum<F> bits_mask_sum(const F& f, uint32_t* lds, const typename F::elem* __restrict__ a,
                                                         const typename F::elem* __restrict__ rbits,
                                                         const typename F::elem* __restrict__ rdivl, int l, size_t n) {
    typedef typename F::word W;
    constexpr size_t EB = sizeof(typename F::elem);
    const size_t h0 = sgn_tile_base(blockIdx.x);
    const unsigned rows = sgn_tile_rows(n, h0), t = threadIdx.x;
    BitsMaskSum<F> m;
    m.h = h0 + t;
    m.live = t < rows;
    m.wave_full = h0 + (t | 63u) < n;
    m.av = sgn_load<F>(a, m.h, m.live, m.wave_full);
    m.rd = sgn_load<F>(rdivl, m.h, m.live, m.wave_full);
    W acc = W();
    for (int i0 = (l - 1) / sgn_chunk(EB) * sgn_chunk(EB); i0 >= 0; i0 -= sgn_chunk(EB)) {
        const int cols = sgn_chunk_cols(l, i0, EB);
        sgn_stage<F>(lds, rbits, h0, rows, l, i0, cols);
        __syncthreads();
        if (m.live) {
            for (int j = cols - 1; j >= 0; --j) acc = f.add(f.add(acc, acc), sgn_lds_elem<F>(lds + sgn_walk_lds_word(t, j, EB)));
        }
        __syncthreads();
    }
    m.acc = acc;
    return m;
}

template <class F>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_bits_mask(F f, const typename F::elem* __restrict__ a, const typename F::elem* __restrict__ rbits,
                                                      const typename F::elem* __restrict__ rdivl, int l, typename F::word two_l,
                                                      typename F::word offset, typename F::elem* __restrict__ out, size_t n) {
    typedef typename F::word W;
    __shared__ uint32_t lds[sgn_lds_words(sizeof(typename F::elem))];
    const BitsMaskSum<F> m = bits_mask_sum<F>(f, lds, a, rbits, rdivl, l, n);
    const W hi = f.mul(m.rd, two_l);
    sgn_store<F>(out, m.h, f.sub(f.add(f.add(m.av, offset), hi), m.acc), m.live, m.wave_full);
}

// ---- expand: the leaves a_i b_i and a_i + b_i - 2 a_i b_i of np_add_bits for a public b (runtime.py:4309-4314, 4447-4448) --
// cb_k = bit k of the canonical integer c[h] mod 2^l.  Public bits select, they never multiply.
template <class F>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_bits_expand(F f, const typename F::elem* __restrict__ c, const typename F::elem* __restrict__ rbits,
                                                        int l, typename F::elem* __restrict__ g, typename F::elem* __restrict__ p, size_t n) {
    typedef typename F::word W;
    constexpr size_t EB = sizeof(typename F::elem);
    __shared__ uint32_t lds[sgn_lds_words(EB)];
    const size_t h0 = sgn_tile_base(blockIdx.x);
    const unsigned rows = sgn_tile_rows(n, h0), t = threadIdx.x;
    const size_t h = h0 + t;
    const bool live = t < rows, wave_full = h0 + (t | 63u) < n;
    const W one = ff_one_elem(f);
    const uint64_t cl = sgn_low64(sgn_load<F>(c, h, live, wave_full));      // (bits l and up are never looked at)
    for (int i0 = 0; i0 < l; i0 += sgn_chunk(EB)) {
        const int cols = sgn_chunk_cols(l, i0, EB);
        sgn_stage<F>(lds, rbits, h0, rows, l, i0, cols);
        __syncthreads();
        for (int j = 0; j < cols; ++j) {
            const int k = i0 + j;
            const W r = live ? sgn_lds_elem<F>(lds + sgn_walk_lds_word(t, j, EB)) : W();
            const bool cb = (cl >> k) & 1u;
            sgn_store<F>(g, sgn_out_index(k, n, h), ff_pick(cb, r, W()), live, wave_full);
            sgn_store<F>(p, sgn_out_index(k, n, h), ff_pick(cb, f.sub(one, r), r), live, wave_full);
        }
        __syncthreads();
    }
}

// ---- the two ends of a round of the carry network ---------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(BLOCK) void k_carry_prod(F f, const typename F::elem* __restrict__ g, const typename F::elem* __restrict__ p,
                                                       typename F::elem* __restrict__ out, BitsLevel lv, BitsPlan pl) {
    typedef Pack<typename F::word> P;
    typedef typename MemPack<F>::type MP;
    const int y = blockIdx.y;
    const int k = lv.k[y], q = lv.q[y];
    const typename F::elem* left = y < lv.rc ? g : p;     // uniform over the workgroup
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* lf = reinterpret_cast<const MP*>(left);
        const MP* pv = reinterpret_cast<const MP*>(p);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t u = gid; u < pl.row_units; u += gsz) {
            const auto r0 = ldgw_issue<false>(lf + bits_unit(pl, q, u)), r1 = ldgw_issue<false>(pv + bits_unit(pl, k, u));
            const P x0 = ldgw_finish(r0), x1 = ldgw_finish(r1);
            P z;
#pragma unroll
            for (int e = 0; e < P::N; ++e) z.w[e] = f.mul(x0.w[e], x1.w[e]);
            stgw<false>(ov + bits_unit(pl, y, u), z);
        }
    } else {
        for (size_t u = gid; u < pl.row_units; u += gsz)
            st_elem<F>(out, bits_unit(pl, y, u), f.mul(ld_elem<F>(left, bits_unit(pl, q, u)), ld_elem<F>(p, bits_unit(pl, k, u))));
    }
}

template <class F, int K>
__global__ __launch_bounds__(BLOCK) void k_carry_apply(F f, ShareRows<F, K> ra, typename F::elem* __restrict__ g, typename F::elem* __restrict__ p,
                                                        BitsLevel lv, BitsPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    const int y = blockIdx.y;
    const int k = lv.k[y];
    const bool cprod = y < lv.rc;                        // uniform over the workgroup
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        MP* tv = reinterpret_cast<MP*>(cprod ? g : p);
        for (size_t u = gid; u < pl.row_units; u += gsz) {
            const size_t at = bits_unit(pl, k, u), c = bits_unit(pl, y, u);
            P x[K], x0 = P();
            {
                decltype(ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[0]))) rx[K];
#pragma unroll
                for (int j = 0; j < K; ++j) rx[j] = ldgw_issue<true>(reinterpret_cast<const MP*>(ra.rows[j]) + c);
                if (cprod) {
                    const auto r0 = ldgw_issue<false>(const_cast<const MP*>(tv) + at);
#pragma unroll
                    for (int j = 0; j < K; ++j) x[j] = ldgw_finish(rx[j]);
                    x0 = ldgw_finish(r0);
                } else {
#pragma unroll
                    for (int j = 0; j < K; ++j) x[j] = ldgw_finish(rx[j]);
                }
            }
            P z;
#pragma unroll
            for (int e = 0; e < P::N; ++e) {
                DotAcc<F> s;
                s.zero(f);
#pragma unroll
                for (int j = 0; j < K; ++j) s.mac(f, ra.lam[j], x[j].w[e]);
                const W v = s.reduce(f);
                z.w[e] = cprod ? f.add(x0.w[e], v) : v;
            }
            stgw<false>(tv + at, z);
        }
    } else {
        typename F::elem* t = cprod ? g : p;
        for (size_t u = gid; u < pl.row_units; u += gsz) {
            const size_t at = bits_unit(pl, k, u), c = bits_unit(pl, y, u);
            typename F::acc s;
            f.acc_zero(s);
#pragma unroll
            for (int j = 0; j < K; ++j) f.acc_mac(s, ra.lam[j], ld_elem<F>(ra.rows[j], c));
            const W v = f.acc_reduce(s);
            st_elem<F>(t, at, cprod ? f.add(ld_elem<F>(t, at), v) : v);
        }
    }
}

// ---- finish: the sum bits a_k + b_k - 2 c_k + c_(k-1) (runtime.py:4332-4334) with a = r, b = the public bits of c ---------------
// The chunk of rbits is staged as in mask and expand; every thread walks the columns of its own element, reads row k of G
// (consecutive lanes at consecutive elements), keeps G[k] for the next column, and puts the result where the bit share was;
// the tile then leaves LDS by the units it came in with.
template <class F>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_bits_finish(F f, const typename F::elem* __restrict__ c, const typename F::elem* __restrict__ rbits,
                                                        const typename F::elem* __restrict__ g, int l, typename F::elem* __restrict__ out,
                                                        size_t n) {
    typedef typename F::word W;
    constexpr size_t EB = sizeof(typename F::elem);
    __shared__ uint32_t lds[sgn_lds_words(EB)];
    const size_t h0 = sgn_tile_base(blockIdx.x);
    const unsigned rows = sgn_tile_rows(n, h0), t = threadIdx.x;
    const size_t h = h0 + t;
    const bool live = t < rows, wave_full = h0 + (t | 63u) < n;
    const W one = ff_one_elem(f);
    const uint64_t cl = sgn_low64(sgn_load<F>(c, h, live, wave_full));
    W prev = W();                                        // G[k-1], 0 for k == 0
    for (int i0 = 0; i0 < l; i0 += sgn_chunk(EB)) {
        const int cols = sgn_chunk_cols(l, i0, EB);
        sgn_stage<F>(lds, rbits, h0, rows, l, i0, cols);
        __syncthreads();
        for (int j = 0; j < cols; ++j) {
            const int k = i0 + j;
            const W gk = sgn_load<F>(g, sgn_out_index(k, n, h), live, wave_full);
            if (live) {
                uint32_t* at = lds + sgn_walk_lds_word(t, j, EB);
                const W r = sgn_lds_elem<F>(at);
                const bool cb = (cl >> k) & 1u;
                const W s = f.add(ff_pick(cb, f.add(r, one), r), prev);
                bits_lds_put<F>(at, f.sub(s, f.add(gk, gk)));
            }
            prev = gk;
        }
        __syncthreads();
        bits_unstage<F>(lds, out, h0, rows, l, i0, cols);
        __syncthreads();
    }
}

}  // namespace ffgpu
