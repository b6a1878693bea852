// unitvec.hpp -- the three local steps under secure unit vectors and table lookup at secret indices over a prime field
// (runtime.np_unit_vector, runtime.py:5002-5029; runtime.unit_vector, runtime.py:4979-5000; mpyc.random.np_random_unit_vector,
// random.py:123-152) that no other kernel serves.  The interleave of a demultiplexer round is k_tour_unit_expand as it is.
// Included by kernels.hpp after bsgn.hpp.  Index arithmetic and plans: unitvec_geom.hpp.
//
//   k_unit_prod   out[j n + e] = x[e xstride] U[j n + e], j < h                      the broadcast product of a round: dense (h, n)
//   k_unit_roll   out[j n + e] = U[((j - c[e]) mod K2) n + e], j < K <= K2            random unit vectors rotated by the opened offset
//   k_unit_dot    out[e] = sum_{j < rows} tab[(j + c[e]) mod K2] U[j n + e]           the table read through them, never rotated
// with U position-major (rows, n), c the opened public canonical values (their low kbits bits count), tab zero from tlen up.
//
// All three are streaming kernels of the shape of k_powers_prod and k_poly_dot: one flat grid-stride loop over the units of a
// row, a unit a pack (16 bytes; one 12- or 24-byte element) when the plan's vec, a single element otherwise, the 24-byte pack
// path wave-contiguous (ldgw / stgw: rows of whole waves); the path is a kernel argument (wave-uniform).
//
// k_unit_prod keeps its unit of x in registers across the h rows: h + 1 loads per element where a materialised broadcast
// costs 2 h, as k_powers_prod keeps its top power.  The row loads of k_unit_prod and k_unit_dot go out in groups of four
// (gate_load's chunks): the loop is as long as the table, and one load in flight per thread left it bound by latency.
// With xstride == 1 (rows of random bits) the unit of x is a pack; with the element-major (n, l) bits of k_bits_finish
// (xstride = l) the pack path gathers its x values by element.
//
// k_unit_roll is a gather: a thread owns a column unit of `out` and walks the K output rows; its source row walks
// (j - c) mod K2, so every LANE reads its own column top to bottom with a wrap, while the 64 lanes of a wave read 64 different
// rows at one instant: one line per lane and access, of which the access uses one element.  The rest of the line is used by
// the neighbouring lanes when their own rotation reaches that row, within K2 iterations: the reuse is left to L2, not staged
// in LDS -- and counters show that L2 does not deliver it at n = 10^5 (6-10 % hits, 14-16 times the algorithmic bytes fetched:
// profiles/unitvec_kernels.md); this kernel is bound by that traffic.  A column tile in LDS would need all
// K2 rows of its columns at once (the rotation differs per column, so no row chunk serves a whole tile): K2 eb bytes per
// column, two columns of 24-byte elements at kbits = 10 -- no tile worth a coalesced load.  The stores are whole packs.
// Scattering the stores instead (coalesced loads of row i, stores to row (i + c) mod K2) would write part lines, and read
// K2 rows where K serve.
//
// k_unit_dot stages the prepared table, zero from tlen up, in DYNAMICALLY sized LDS once per workgroup (the launcher caps
// the grid so that a workgroup serves many elements per staging): a 16-entry table costs 16 words, not the occupancy of
// 64 KiB.  The lookups are divergent LDS reads, as in k_pow_base: lanes of a wave read up to 64 different entries.  Without c
// the entry is j for every lane: one broadcast read.  The sum is lazy, flushed every DotAcc<F>::FLUSH terms (DotSum); one
// store per element.  The table takes one WORD per entry: at most 64 KiB, kbits <= 14, 13, 12, 12, 11 for elements of 4, 8,
// 12, 16, 24 bytes (unit_dot_max_kbits); beyond that the launcher refuses (FFGPU_ENOTSUP).
//
// Memory policy: U is read again by the next round or the next call, every output by the next call: default policy throughout.
#pragma once
#include "unitvec_geom.hpp"

namespace ffgpu {

enum { UNIT_GROUP = 4 };            // row loads a thread of k_unit_prod / k_unit_dot has in flight

template <class F>
__global__ __launch_bounds__(BLOCK) void k_unit_prod(F f, const typename F::elem* __restrict__ x, size_t xstride,
                                                      const typename F::elem* __restrict__ U, size_t h,
                                                      typename F::elem* __restrict__ out, RowsPlan pl, int xvec) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* xv = reinterpret_cast<const MP*>(x);
        const MP* uv = reinterpret_cast<const MP*>(U);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            PK xs;
            if (xvec) {
                xs = ldgw_finish(ldgw_issue<false>(xv + g));
            } else {
#pragma unroll
                for (int q = 0; q < PK::N; ++q) xs.w[q] = ld_elem<F>(x, unit_x_at(unit_elem(pl, g, (unsigned)q), xstride));
            }
            // rows in groups of UNIT_GROUP: the loads of a group are issued together and waited for once (h is wave-uniform, the
            // guards are scalar branches), as gate_load does -- one load, one product, one store per row would expose h latencies
            for (size_t j0 = 0; j0 < h; j0 += UNIT_GROUP) {
                decltype(ldgw_issue<false>(uv)) raw[UNIT_GROUP];
#pragma unroll
                for (int r = 0; r < UNIT_GROUP; ++r)
                    if (j0 + r < h) raw[r] = ldgw_issue<false>(uv + rows_unit(pl, j0 + r, g));
#pragma unroll
                for (int r = 0; r < UNIT_GROUP; ++r)
                    if (j0 + r < h) {
                        const PK uj = ldgw_finish(raw[r]);
                        PK y;
#pragma unroll
                        for (int q = 0; q < PK::N; ++q) y.w[q] = f.mul(xs.w[q], uj.w[q]);
                        stgw<false>(ov + rows_unit(pl, j0 + r, g), y);
                    }
            }
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const W xs = ld_elem<F>(x, unit_x_at(g, xstride));
            for (size_t j0 = 0; j0 < h; j0 += UNIT_GROUP) {
                W uj[UNIT_GROUP];
#pragma unroll
                for (int r = 0; r < UNIT_GROUP; ++r)
                    if (j0 + r < h) uj[r] = ld_elem<F>(U, rows_unit(pl, j0 + r, g));
#pragma unroll
                for (int r = 0; r < UNIT_GROUP; ++r)
                    if (j0 + r < h) st_elem<F>(out, rows_unit(pl, j0 + r, g), f.mul(xs, uj[r]));
            }
        }
    }
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_unit_roll(F f, const typename F::elem* __restrict__ U, const typename F::elem* __restrict__ c,
                                                      uint64_t cmask, size_t K, typename F::elem* __restrict__ out, RowsPlan pl,
                                                      size_t n) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    (void)f;
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* cv = reinterpret_cast<const MP*>(c);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            const PK cs = ldgw_finish(ldgw_issue<false>(cv + g));
            size_t off[PK::N];
#pragma unroll
            for (int q = 0; q < PK::N; ++q) off[q] = unit_offset(explog_limb(cs.w[q], 0), cmask);
#pragma unroll 4
            for (size_t j = 0; j < K; ++j) {
                PK y;
#pragma unroll
                for (int q = 0; q < PK::N; ++q) y.w[q] = ld_elem<F>(U, unit_roll_src(j, off[q], cmask) * n + unit_elem(pl, g, (unsigned)q));
                stgw<false>(ov + rows_unit(pl, j, g), y);
            }
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const size_t off = unit_offset(explog_limb(ld_elem<F>(c, g), 0), cmask);
#pragma unroll 4
            for (size_t j = 0; j < K; ++j) st_elem<F>(out, j * n + g, ld_elem<F>(U, unit_roll_src(j, off, cmask) * n + g));
        }
    }
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_unit_dot(F f, const typename F::elem* __restrict__ U, size_t rows,
                                                     const typename F::elem* __restrict__ c, uint64_t cmask,
                                                     const typename F::elem* __restrict__ tab, size_t tlen, size_t entries,
                                                     typename F::elem* __restrict__ out, RowsPlan pl) {
    typedef typename F::word W;
    typedef Pack<W> PK;
    typedef typename MemPack<F>::type MP;
    constexpr int FLUSH = DotAcc<F>::FLUSH;
    static_assert(FLUSH % UNIT_GROUP == 0, "the flush test follows whole groups of rows");
    extern __shared__ __attribute__((aligned(16))) unsigned char unit_smem[];
    W* T = reinterpret_cast<W*>(unit_smem);
    for (size_t i = threadIdx.x; i < entries; i += BLOCK) T[i] = i < tlen ? f.prep(ld_elem<F>(tab, i)) : W();
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t gsz = (size_t)gridDim.x * BLOCK;
    if (pl.vec) {
        const MP* uv = reinterpret_cast<const MP*>(U);
        const MP* cv = reinterpret_cast<const MP*>(c);
        MP* ov = reinterpret_cast<MP*>(out);
        for (size_t g = gid; g < pl.total; g += gsz) {
            size_t off[PK::N];
#pragma unroll
            for (int q = 0; q < PK::N; ++q) off[q] = 0;
            if (c) {
                const PK cs = ldgw_finish(ldgw_issue<false>(cv + g));
#pragma unroll
                for (int q = 0; q < PK::N; ++q) off[q] = unit_offset(explog_limb(cs.w[q], 0), cmask);
            }
            DotSum<F> s[PK::N];
#pragma unroll
            for (int q = 0; q < PK::N; ++q) s[q].zero(f);
            bool have = false;
            int since = 0;
            for (size_t j0 = 0; j0 < rows; j0 += UNIT_GROUP) {          // groups of loads, as in k_unit_prod
                decltype(ldgw_issue<false>(uv)) raw[UNIT_GROUP];
#pragma unroll
                for (int r = 0; r < UNIT_GROUP; ++r)
                    if (j0 + r < rows) raw[r] = ldgw_issue<false>(uv + rows_unit(pl, j0 + r, g));
#pragma unroll
                for (int r = 0; r < UNIT_GROUP; ++r)
                    if (j0 + r < rows) {
                        const PK uj = ldgw_finish(raw[r]);
#pragma unroll
                        for (int q = 0; q < PK::N; ++q) s[q].mac(f, T[unit_dot_tab(j0 + r, off[q], cmask)], uj.w[q]);
                        ++since;
                    }
                if (since == FLUSH) {               // (whole groups: FLUSH is a multiple of UNIT_GROUP) keep the unreduced accumulators inside their headroom
#pragma unroll
                    for (int q = 0; q < PK::N; ++q) s[q].flush(f, have);
                    have = true;
                    since = 0;
                }
            }
            PK y;
#pragma unroll
            for (int q = 0; q < PK::N; ++q) y.w[q] = s[q].result(f, have);
            stgw<false>(ov + g, y);
        }
    } else {
        for (size_t g = gid; g < pl.total; g += gsz) {
            const size_t off = c ? unit_offset(explog_limb(ld_elem<F>(c, g), 0), cmask) : 0;
            DotSum<F> s;
            s.zero(f);
            bool have = false;
            int since = 0;
            for (size_t j0 = 0; j0 < rows; j0 += UNIT_GROUP) {
                W uj[UNIT_GROUP];
#pragma unroll
                for (int r = 0; r < UNIT_GROUP; ++r)
                    if (j0 + r < rows) uj[r] = ld_elem<F>(U, rows_unit(pl, j0 + r, g));
#pragma unroll
                for (int r = 0; r < UNIT_GROUP; ++r)
                    if (j0 + r < rows) {
                        s.mac(f, T[unit_dot_tab(j0 + r, off, cmask)], uj[r]);
                        ++since;
                    }
                if (since == FLUSH) {
                    s.flush(f, have);
                    have = true;
                    since = 0;
                }
            }
            st_elem<F>(out, g, s.result(f, have));
        }
    }
}

}  // namespace ffgpu
