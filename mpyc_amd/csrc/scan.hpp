// scan.hpp -- prefix scans and reductions of a field array along one axis (np.cumsum / np.cumprod / np.cumulative_sum /
// np.cumulative_prod and ufunc.accumulate on field arrays: finfields.py:801, 807; FiniteFieldArray.sum / .prod along an
// axis: finfields.py:1332-1349; runtime.np_cumsum, runtime.py:3510-3549, and the cumsum of runtime.np_sgn, runtime.py:3668).
// Included by kernels.hpp after convolve.hpp.  Geometry and index arithmetic: scan_geom.hpp.
//
// Field addition and multiplication are exact, associative and commutative on canonical values, so every kernel here works
// with the policy's add / mul (canonical in, canonical out) and any evaluation order gives the same bytes.  (The
// Montgomery policies keep values canonical in memory and pay two reductions per product inside mul; a running product
// kept in Montgomery form would need the second one as well to emit the canonical prefix, so a scan saves nothing by it.
// A REDUCTION emits nothing until the end and could halve its reductions that way -- one Montgomery product per element
// with the run in prepared form; that is not built and the two Montgomery policies are not among the measured fields
// (profiles/r09_scan.md), so it stays an open item rather than a claim.)
//
// Memory policy: the column walk streams its input once (non-temporal loads on the pack path).  The row kernels read
// with the default policy: pass (A) of a multi-tile line is read again by pass (C), and an 80 MB array stays in the
// Infinity Cache between the two.  Outputs of every kernel here take the default policy: a scan's result is consumed by the
// next operation of its caller (np_sgn slices it at once) and these launches are not producers the hand-off tracker
// follows (handoff.hpp), exactly as ffgpu_matmul and ffgpu_convolve.
#pragma once
#include "scan_geom.hpp"

namespace ffgpu {

static_assert((int)SCAN_THREADS == (int)BLOCK, "scan_geom.hpp is laid out for the library's workgroup");

template <class F, bool MUL>
struct ScanOp {
    typedef typename F::word W;
    // identity of a word whose every element lane is live (packs of the column walk)
    static __device__ __forceinline__ W id(const F& f) {
        if constexpr (MUL) return ff_one(f); else return W();
    }
    // identity of a word that holds ONE element (scalar paths; differs for the packed GF(2^n <= 8) policy only)
    static __device__ __forceinline__ W id_elem(const F& f) {
        if constexpr (MUL) return ff_one_elem(f); else return W();
    }
    static __device__ __forceinline__ W ap(const F& f, const W& a, const W& b) {
        if constexpr (MUL) return f.mul(a, b); else return f.add(a, b);
    }
};

// ---- columns ---------------------------------------------------------------------------------------------------------
// One column: `run` walks j = 0 .. k-1; U loads are issued before the first of them is used, so a wave keeps U coalesced
// requests in flight.  ld(j) / st(j, v) address step j (st is called for positions 0 .. k-1 [+ 1 with the initial]).
enum { SCAN_COL_U = 4 };
template <class V, bool RED, class Ap, class Ld, class St>
__device__ __forceinline__ void scan_walk(size_t k, int wi, const V& ident, Ap&& ap, Ld&& ld, St&& st) {
    V run = ident;
    if (!RED && wi) st((size_t)0, run);
    size_t j = 0;
    for (; j + SCAN_COL_U <= k; j += SCAN_COL_U) {
        V x[SCAN_COL_U];
#pragma unroll
        for (int u = 0; u < SCAN_COL_U; ++u) x[u] = ld(j + u);
#pragma unroll
        for (int u = 0; u < SCAN_COL_U; ++u) {
            run = ap(run, x[u]);
            if (!RED) st(j + u + (size_t)wi, run);
        }
    }
    for (; j < k; ++j) {
        run = ap(run, ld(j));
        if (!RED) st(j + (size_t)wi, run);
    }
    if (RED) st((size_t)0, run);
}

// a and out may be the same array (in place, wi == 0): a thread reads step j of its own column before it writes it and no
// other thread touches that column -- hence no __restrict__ here.
template <class F, bool MUL, bool RED>
__global__ __launch_bounds__(BLOCK) void k_scan_cols(F f, const typename F::elem* a, typename F::elem* out, size_t k, size_t inner,
                                                      size_t per, size_t units, int vec, int wi) {
    typedef typename F::word W;
    typedef Pack<W> P;
    typedef typename MemPack<F>::type MP;
    typedef ScanOp<F, MUL> Op;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    const size_t kk = RED ? 1 : k + (size_t)wi;         // entries of `out` along the axis
    if (vec) {
        const MP* av = reinterpret_cast<const MP*>(a);
        MP* ov = reinterpret_cast<MP*>(out);
        P ident;
#pragma unroll
        for (int q = 0; q < P::N; ++q) ident.w[q] = Op::id(f);
        for (size_t u = gid; u < units; u += gsz) {
            size_t o, c;
            scan_col_of(u, per, o, c);
            scan_walk<P, RED>(
                k, wi, ident,
                [&](const P& r, const P& x) {
                    P y;
#pragma unroll
                    for (int q = 0; q < P::N; ++q) y.w[q] = Op::ap(f, r.w[q], x.w[q]);
                    return y;
                },
                [&](size_t j) { return ldg<true>(av + scan_col_index(o, c, j, k, per)); },
                [&](size_t j, const P& v) { stg<false>(ov + scan_col_index(o, c, j, kk, per), v); });
        }
    } else {
        const W ident = Op::id_elem(f);
        for (size_t u = gid; u < units; u += gsz) {
            size_t o, c;
            scan_col_of(u, inner, o, c);
            scan_walk<W, RED>(
                k, wi, ident, [&](const W& r, const W& x) { return Op::ap(f, r, x); },
                [&](size_t j) { return ld_elem<F>(a, scan_col_index(o, c, j, k, inner)); },
                [&](size_t j, const W& v) { st_elem<F>(out, scan_col_index(o, c, j, kk, inner), v); });
        }
    }
}

// ---- rows ------------------------------------------------------------------------------------------------------------
// cross-lane move of a field word within a wave, 32 bits at a time (the value of lane - delta; lanes below delta get their own)
template <class W>
__device__ __forceinline__ W wave_shfl_up(const W& v, int delta) {
    static_assert(sizeof(W) % 4 == 0, "word size");
    union {
        W w;
        int d[sizeof(W) / 4];
    } in, outv;
    in.w = v;
#pragma unroll
    for (int q = 0; q < (int)(sizeof(W) / 4); ++q) outv.d[q] = __shfl_up(in.d[q], delta, 64);
    return outv.w;
}

// Exclusive scan of one value per thread over the workgroup, in thread order; `total` is the fold of all of them.  Wave
// scan by cross-lane moves (6 steps), then the BLOCK / 64 wave totals through LDS (3 more operations).  sm: BLOCK / 64 words; the caller puts a
// barrier between two calls that share it.
template <class F, bool MUL>
__device__ __forceinline__ typename F::word scan_block_excl(const F& f, typename F::word v, typename F::word* sm,
                                                            typename F::word& total) {
    typedef typename F::word W;
    typedef ScanOp<F, MUL> Op;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    W incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const W y = wave_shfl_up(incl, d);
        if (lane >= d) incl = Op::ap(f, y, incl);
    }
    if (lane == 63) sm[wave] = incl;
    W excl = wave_shfl_up(incl, 1);
    if (lane == 0) excl = Op::id_elem(f);
    __syncthreads();
    // prefixes of the wave totals: the same three operations on every thread, then a select -- not one chain per wave
    W pre[BLOCK / 64];
    pre[0] = sm[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) pre[w] = Op::ap(f, pre[w - 1], sm[w]);
    total = pre[BLOCK / 64 - 1];
    W before = Op::id_elem(f);
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w)
        if (wave == w) before = pre[w - 1];
    return Op::ap(f, before, excl);
}

// Fold of one value per thread over the workgroup (valid on thread 0): butterfly within the wave, wave totals through LDS.
template <class F, bool MUL>
__device__ __forceinline__ typename F::word scan_block_total(const F& f, typename F::word v, typename F::word* sm) {
    typedef typename F::word W;
    typedef ScanOp<F, MUL> Op;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = Op::ap(f, v, wave_shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    W r = sm[0];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < BLOCK / 64; ++w) r = Op::ap(f, r, sm[w]);
    }
    return r;
}

template <class F>
struct ScanItems {
    enum { N = sizeof(typename F::elem) <= 8 ? 16 : 8 };        // = scan_items(sizeof(elem))
};

// The ITEMS elements of thread `tid` of tile t: j0 + q, identity where the thread holds nothing (tid >= tt) or the line has
// ended.  UNIT (inner == 1): a thread's elements are consecutive in memory and a thread that is wholly inside the line
// loads them without a test per element, so that the compiler merges the loads into 16-byte accesses.
template <class F, bool MUL, bool UNIT>
__device__ __forceinline__ void scan_tile_load(const F& f, const typename F::elem* a, size_t base, size_t inner, size_t j0,
                                               size_t k, bool live, typename F::word (&x)[ScanItems<F>::N]) {
    typedef ScanOp<F, MUL> Op;
    constexpr int IT = ScanItems<F>::N;
    if (live && j0 + IT <= k) {
#pragma unroll
        for (int q = 0; q < IT; ++q) x[q] = ld_elem<F>(a, base + (j0 + q) * (UNIT ? (size_t)1 : inner));
    } else {
#pragma unroll
        for (int q = 0; q < IT; ++q) {
            const bool ok = live && j0 + q < k;
            x[q] = ok ? ld_elem<F>(a, base + (j0 + q) * (UNIT ? (size_t)1 : inner)) : Op::id_elem(f);
        }
    }
}

// (A) aggregate of every tile -> dst[line * ntiles + tile] (elements, not words: with one tile per line dst is the output of
// a reduction itself)
template <class F, bool MUL, bool UNIT>
__global__ __launch_bounds__(BLOCK) void k_scan_tile_reduce(F f, const typename F::elem* __restrict__ a,
                                                             typename F::elem* __restrict__ dst, size_t k, size_t inner,
                                                             size_t ntiles, int tt) {
    typedef typename F::word W;
    typedef ScanOp<F, MUL> Op;
    constexpr int IT = ScanItems<F>::N;
    static_assert(IT == 16 || IT == 8, "scan_items");
    __shared__ W sm[BLOCK / 64];
    size_t line, t;
    scan_tile_of((size_t)blockIdx.x, ntiles, line, t);
    const size_t base = scan_line_base(line, k, inner);
    const int tid = threadIdx.x;
    W x[IT];
    scan_tile_load<F, MUL, UNIT>(f, a, base, inner, scan_item_j(t, (size_t)tt * IT, tid, IT, 0), k, tid < tt, x);
    W v = x[0];
    // (compile-time loops: `#pragma unroll` gives up on the largest products -- GF(2^128) -- and x[] would move to scratch)
    ff_static_for<1, IT, 1>([&](auto q) { v = Op::ap(f, v, x[q]); });
    const W total = scan_block_total<F, MUL>(f, v, sm);
    if (tid == 0) st_elem<F>(dst, (size_t)blockIdx.x, total);
}

// (B) one workgroup per line: exclusive scan of the line's tile aggregates in place (FINAL: their fold -> out[line]), chunk
// after chunk in order with the running carry in registers
template <class F, bool MUL, bool FINAL>
__global__ __launch_bounds__(BLOCK) void k_scan_tile_carry(F f, typename F::elem* ws, typename F::elem* out, size_t ntiles) {
    typedef typename F::word W;
    typedef ScanOp<F, MUL> Op;
    __shared__ W sm[BLOCK / 64];
    const size_t line = blockIdx.x;
    W carry = Op::id_elem(f);
    for (size_t c0 = 0; c0 < ntiles; c0 += BLOCK) {
        const size_t t = c0 + threadIdx.x;
        const bool ok = t < ntiles;
        const W v = ok ? ld_elem<F>(ws, scan_ws_index(line, t, ntiles)) : Op::id_elem(f);
        W total;
        const W excl = scan_block_excl<F, MUL>(f, v, sm, total);
        if (!FINAL && ok) st_elem<F>(ws, scan_ws_index(line, t, ntiles), Op::ap(f, carry, excl));
        carry = Op::ap(f, carry, total);
        __syncthreads();                                   // sm is written again by the next chunk
    }
    if (FINAL && threadIdx.x == 0) st_elem<F>(out, line, carry);
}

// (C) scan of every tile with its carry-in (ws == nullptr: one tile per line, no carry).  a and out may be the same
// array (wi == 0): a workgroup has read its whole tile before its first store, and no other workgroup touches it.
template <class F, bool MUL, bool UNIT>
__global__ __launch_bounds__(BLOCK) void k_scan_tile(F f, const typename F::elem* a, typename F::elem* out,
                                                      const typename F::elem* ws, size_t k, size_t inner, size_t ntiles, int tt,
                                                      int wi) {
    typedef typename F::word W;
    typedef ScanOp<F, MUL> Op;
    constexpr int IT = ScanItems<F>::N;
    __shared__ W sm[BLOCK / 64];
    size_t line, t;
    scan_tile_of((size_t)blockIdx.x, ntiles, line, t);
    const size_t base = scan_line_base(line, k, inner);
    const size_t obase = scan_line_base(line, k + (size_t)wi, inner);
    const int tid = threadIdx.x;
    const size_t j0 = scan_item_j(t, (size_t)tt * IT, tid, IT, 0);
    const bool live = tid < tt;
    W x[IT];
    scan_tile_load<F, MUL, UNIT>(f, a, base, inner, j0, k, live, x);
    ff_static_for<1, IT, 1>([&](auto q) { x[q] = Op::ap(f, x[q - 1], x[q]); });
    W total;
    W pre = scan_block_excl<F, MUL>(f, x[IT - 1], sm, total);
    if (ws) pre = Op::ap(f, ld_elem<F>(ws, (size_t)blockIdx.x), pre);
    if (wi && t == 0 && tid == 0) st_elem<F>(out, obase, Op::id_elem(f));
    const size_t step = UNIT ? (size_t)1 : inner;
    if (live && j0 + IT <= k) {
        ff_static_for<0, IT, 1>([&](auto q) { st_elem<F>(out, obase + (j0 + q + (size_t)wi) * step, Op::ap(f, pre, x[q])); });
    } else {
        ff_static_for<0, IT, 1>([&](auto q) {
            if (live && j0 + q < k) st_elem<F>(out, obase + (j0 + q + (size_t)wi) * step, Op::ap(f, pre, x[q]));
        });
    }
}

}  // namespace ffgpu
