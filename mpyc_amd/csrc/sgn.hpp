// sgn.hpp -- the local steps of the secure comparison runtime.np_sgn (runtime.py:3622-3693) between its openings, for one
// party's shares over a prime field: mask (:3649-3657), expand (:3658-3671, :3679) and finish (:3674-3676).  Included by
// kernels.hpp after scan.hpp.  Geometry and index arithmetic: sgn_geom.hpp.
//
// Every step is affine in the shares given public data, so each is one pass.  The random bit shares are element-major
// (n, l), the operands of the product tree bit-major (l + 1, n): mask and expand stage a tile's bit shares through LDS with
// coalesced loads, a chunk of bit columns at a time, and every thread then walks the columns of its own element with the
// prefix count of the XORs, the weighted sum and c mod 2^l in registers (sgn_geom.hpp).  finish is element-wise
// (stream_map).
//
// Memory policy: the bit shares are read once (non-temporal loads); outputs take the default policy -- e and nx feed the
// product tree of the caller at once.  Public bits select, they never multiply: x_i = c_i ? 1 - r_i : r_i.
#pragma once
#include "sgn_geom.hpp"

namespace ffgpu {

static_assert((int)GEOM_THREADS == (int)BLOCK && (int)SGN_TILE == (int)BLOCK, "sgn_geom.hpp is laid out for the library's workgroup");
static_assert((int)SGN_X24_BYTES == (BLOCK / 64) * 96 * 16, "sgn_geom.hpp counts the staging region of ldgw / stgw");

template <class W>
__device__ __forceinline__ W sgn_word64(uint64_t v) {
    if constexpr (sizeof(W) == 24) {
        W w;
        w.lo = v;
        w.mid = 0;
        w.hi = 0;
        return w;
    } else if constexpr (sizeof(W) == 16) {
        W w;
        w.lo = v;
        w.hi = 0;
        return w;
    } else {
        return (W)v;
    }
}
template <class W>
__device__ __forceinline__ uint64_t sgn_low64(const W& w) {
    if constexpr (sizeof(W) >= 16) return w.lo; else return (uint64_t)w;
}
template <class W>
__device__ __forceinline__ bool sgn_is_zero(const W& w) {
    if constexpr (sizeof(W) == 24) return (w.lo | w.mid | w.hi) == 0;
    else if constexpr (sizeof(W) == 16) return (w.lo | w.hi) == 0;
    else return w == 0;
}

// the element that starts at LDS word p (rows start at odd word offsets: 4-byte reads, 64 lanes in 64 banks each)
template <class F>
__device__ __forceinline__ typename F::word sgn_lds_elem(const uint32_t* p) {
    typedef typename F::word W;
    constexpr int EW = sizeof(typename F::elem) / 4;
    if constexpr (EW == 1) {
        return (W)p[0];
    } else if constexpr (EW == 2) {
        return (W)((uint64_t)p[0] | ((uint64_t)p[1] << 32));
    } else if constexpr (EW == 3) {
        W w;
        w.lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);
        w.hi = p[2];
        return w;
    } else if constexpr (EW == 4) {
        W w;
        w.lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);
        w.hi = (uint64_t)p[2] | ((uint64_t)p[3] << 32);
        return w;
    } else {
        static_assert(EW == 6, "element sizes: 4, 8, 12, 16, 24 bytes");
        W w;
        w.lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);
        w.mid = (uint64_t)p[2] | ((uint64_t)p[3] << 32);
        w.hi = (uint64_t)p[4] | ((uint64_t)p[5] << 32);
        return w;
    }
}

// N units of a thread: all loads first, then the LDS stores.  PRED: the thread may run out of rows (last tile).
template <class F, int N, bool PRED>
__device__ __forceinline__ void sgn_stage_group(uint32_t* lds, const uint32_t* __restrict__ g, size_t h0, unsigned rows, int l, int i0,
                                                SgnCursor& c) {
    constexpr size_t EB = sizeof(typename F::elem);
    constexpr int UW = sgn_unit_words(EB);
    uint32_t v[N][UW];
    SgnCursor d = c;                                 // the stores replay the cursor: no LDS address is held across the loads
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (!PRED || c.row < rows) {
            const uint32_t* src = g + sgn_unit_src_word(h0, c.row, l, i0, c.u, EB);
            if constexpr (UW == 2) {
                const ff_u32x2 x = __builtin_nontemporal_load(reinterpret_cast<const ff_u32x2*>(src));
                v[k][0] = x.x;
                v[k][1] = x.y;
            } else {
                v[k][0] = __builtin_nontemporal_load(src);
            }
        }
        sgn_cursor_next(c);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (!PRED || d.row < rows) {
            const unsigned at = sgn_unit_lds_word(d.row, d.u, EB);
#pragma unroll
            for (int w = 0; w < UW; ++w) lds[at + w] = v[k][w];
        }
        sgn_cursor_next(d);
    }
}

// Columns i0 .. i0 + cols - 1 of the tile's bit shares -> LDS.  Consecutive threads move consecutive 4- or 8-byte units of a
// row (sgn_geom.hpp).  A full tile gives every thread the same number of units (the units of one row): they go in groups of
// INFL (15 or 16) loads issued back to back with no test between them -- a full chunk is one or two such groups, 32 KiB in
// flight per workgroup -- and the last tile of the array takes the tested form.
template <class F>
__device__ __forceinline__ void sgn_stage(uint32_t* lds, const typename F::elem* __restrict__ rbits, size_t h0, unsigned rows, int l,
                                          int i0, int cols) {
    constexpr size_t EB = sizeof(typename F::elem);
    constexpr int INFL = (EB / 4) % 3 ? 16 : 15;      // divides the units of a thread in a full chunk: 32, 16, 30, 16, 15
    static_assert((sgn_chunk(EB) * sgn_elem_words(EB) / sgn_unit_words(EB)) % INFL == 0, "groups of a full chunk");
    const uint32_t* g = reinterpret_cast<const uint32_t*>(rbits);
    const unsigned upr = sgn_units_per_row(cols, EB);
    SgnCursor c = sgn_cursor(threadIdx.x, upr);
    if (rows == (unsigned)SGN_TILE) {
        unsigned left = upr;
        for (; left >= (unsigned)INFL; left -= INFL) sgn_stage_group<F, INFL, false>(lds, g, h0, rows, l, i0, c);
        for (; left >= 4; left -= 4) sgn_stage_group<F, 4, false>(lds, g, h0, rows, l, i0, c);
        for (; left > 0; --left) sgn_stage_group<F, 1, false>(lds, g, h0, rows, l, i0, c);
    } else {
        while (c.row < rows) sgn_stage_group<F, 4, true>(lds, g, h0, rows, l, i0, c);
    }
}

// Element idx of an n-element array, one element per lane, lanes at consecutive elements.  12-byte elements: dwordx3.
// 24-byte elements: the wave-contiguous ldgw / stgw when the whole wave is inside the array and its 1536 bytes start
// 16-byte aligned (wave-uniform conditions), three dwordx2 per lane otherwise.
template <class F>
__device__ __forceinline__ bool sgn_wave_ok(const typename F::elem* p, size_t idx, bool wave_full) {
    return wave_full && (((uintptr_t)(p + idx) - (uintptr_t)__lane_id() * 24) & 15u) == 0;
}
template <class F>
__device__ __forceinline__ typename F::word sgn_load(const typename F::elem* p, size_t idx, bool live, bool wave_full) {
    typedef typename F::word W;
    if constexpr (sizeof(typename F::elem) == 24) {
        if (sgn_wave_ok<F>(p, idx, wave_full)) return ldgw_finish(ldgw_issue<false>(p + idx)).w[0];
        return live ? ldg<false>(p + idx).w[0] : W();
    } else if constexpr (sizeof(typename F::elem) == 12) {
        return live ? ldg<false>(p + idx).w[0] : W();
    } else {
        return live ? ld_elem<F>(p, idx) : W();
    }
}
template <class F>
__device__ __forceinline__ void sgn_store(typename F::elem* p, size_t idx, const typename F::word& v, bool live, bool wave_full) {
    if constexpr (sizeof(typename F::elem) == 24) {
        Pack<u192e> x;
        x.w[0] = v;
        if (sgn_wave_ok<F>(p, idx, wave_full)) stgw<false>(p + idx, x);
        else if (live) stg<false>(p + idx, x);
    } else if constexpr (sizeof(typename F::elem) == 12) {
        Pack<u128e> x;
        x.w[0] = v;
        if (live) stg<false>(p + idx, x);
    } else {
        if (live) st_elem<F>(p, idx, v);
    }
}

// Occupancy: a workgroup is four waves, one per SIMD, and LDS admits four workgroups per compute unit (sgn_geom.hpp).  The
// loads in flight cost registers (a chunk's data plus the addresses the compiler forms up front: 112-138 VGPRs for 8- to
// 24-byte elements left alone, three waves per SIMD for the widest), so mask and expand ask for at least four waves per
// SIMD; the 24-byte expand then spills 11 VGPRs and times the same (profiles/r15_sgn.md).
// ---- mask: masked[h] = a[h] + 2^l + sum_i rbits[h l + i] 2^(l-1-i) + rdivl[h] 2^l ----------------------------------------
// (runtime.py:3649-3657: r_modl = np.sum(r_bits << shifts, axis=1); a_r = a + (1 << l) + r_modl; a_r + (r_divl << l).)
// The weighted row sum by Horner in the field, acc = 2 acc + r_i; one product, (rdivl + 1) 2^l.
template <class F>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_sgn_mask(F f, const typename F::elem* __restrict__ a, const typename F::elem* __restrict__ rbits,
                                                     const typename F::elem* __restrict__ rdivl, int l, typename F::word two_l,
                                                     typename F::elem* __restrict__ out, size_t n) {
    typedef typename F::word W;
    constexpr size_t EB = sizeof(typename F::elem);
    __shared__ uint32_t lds[sgn_lds_words(EB)];
    const size_t h0 = sgn_tile_base(blockIdx.x);
    const unsigned rows = sgn_tile_rows(n, h0), t = threadIdx.x;
    const size_t h = h0 + t;
    const bool live = t < rows, wave_full = h0 + (t | 63u) < n;
    const W av = sgn_load<F>(a, h, live, wave_full);
    const W rd = sgn_load<F>(rdivl, h, live, wave_full);
    W acc = W();
    for (int i0 = 0; i0 < l; i0 += sgn_chunk(EB)) {
        const int cols = sgn_chunk_cols(l, i0, EB);
        sgn_stage<F>(lds, rbits, h0, rows, l, i0, cols);
        __syncthreads();
        if (live) {
            for (int j = 0; j < cols; ++j) acc = f.add(f.add(acc, acc), sgn_lds_elem<F>(lds + sgn_walk_lds_word(t, j, EB)));
        }
        __syncthreads();
    }
    const W hi = f.mul(f.add(rd, ff_one_elem(f)), two_l);
    sgn_store<F>(out, h, f.add(f.add(av, acc), hi), live, wave_full);
}

// ---- expand ----------------------------------------------------------------------------------------------------------------
// With cl = c[h] mod 2^l (the canonical integer), cb_i = bit l-1-i of cl, r_i = rbits[h l + i], s = 2 sbit[h] - 1:
//   x_i = cb_i ? 1 - r_i : r_i                         (Xor = c_bits + r_bits - 2 c_bits r_bits, runtime.py:3661-3663)
//   S_0 = 0, S_{i+1} = S_i + x_i                       (SumXors, :3666-3668)
//   e[i n + h] = s - cb_i + r_i + 3 S_i, i < l; e[l n + h] = s - 1 + 3 S_l      (:3671)
//   nx[i n + h] = 1 - x_i                              (:3679)
//   z[h] = cl - a[h] - 2^l - sum_i r_i 2^(l-1-i)       (:3658-3659, a_r recomputed from the inputs already being read)
// e, nx, z: each may be null; sbit only when e is.
template <class F>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_sgn_expand(F f, const typename F::elem* __restrict__ c, const typename F::elem* __restrict__ a,
                                                       const typename F::elem* __restrict__ rbits, const typename F::elem* __restrict__ sbit,
                                                       int l, typename F::word two_l, typename F::elem* __restrict__ e,
                                                       typename F::elem* __restrict__ nx, typename F::elem* __restrict__ z, size_t n) {
    typedef typename F::word W;
    constexpr size_t EB = sizeof(typename F::elem);
    __shared__ uint32_t lds[sgn_lds_words(EB)];
    const size_t h0 = sgn_tile_base(blockIdx.x);
    const unsigned rows = sgn_tile_rows(n, h0), t = threadIdx.x;
    const size_t h = h0 + t;
    const bool live = t < rows, wave_full = h0 + (t | 63u) < n;
    const W one = ff_one_elem(f);
    const uint64_t cl = sgn_low64(sgn_load<F>(c, h, live, wave_full)) & (l == 64 ? ~0ull : ((1ull << l) - 1));
    W s = W();
    if (e) {
        const W sb = sgn_load<F>(sbit, h, live, wave_full);
        s = f.sub(f.add(sb, sb), one);
    }
    const W sm1 = f.sub(s, one);
    W S = W(), acc = W();
    for (int i0 = 0; i0 < l; i0 += sgn_chunk(EB)) {
        const int cols = sgn_chunk_cols(l, i0, EB);
        sgn_stage<F>(lds, rbits, h0, rows, l, i0, cols);
        __syncthreads();
        for (int j = 0; j < cols; ++j) {
            const int i = i0 + j;
            const W r = live ? sgn_lds_elem<F>(lds + sgn_walk_lds_word(t, j, EB)) : W();
            const bool cb = (cl >> (l - 1 - i)) & 1u;
            const W omr = f.sub(one, r);
            if (e) {
                const W s3 = f.add(f.add(S, S), S);
                sgn_store<F>(e, sgn_out_index(i, n, h), f.add(f.add(ff_pick(cb, sm1, s), r), s3), live, wave_full);
            }
            if (nx) sgn_store<F>(nx, sgn_out_index(i, n, h), ff_pick(cb, r, omr), live, wave_full);
            S = f.add(S, ff_pick(cb, omr, r));
            acc = f.add(f.add(acc, acc), r);
        }
        __syncthreads();
    }
    if (e) sgn_store<F>(e, sgn_out_index(l, n, h), f.add(sm1, f.add(f.add(S, S), S)), live, wave_full);
    if (z) {
        const W av = sgn_load<F>(a, h, live, wave_full);
        sgn_store<F>(z, h, f.sub(f.sub(f.sub(sgn_word64<W>(cl), av), two_l), acc), live, wave_full);
    }
}

// ---- finish: lt[h] = (z[h] + ((1 - 2 g) s + 3) 2^(l-1)) 2^-l, g = (w[h] == 0), s = 2 sbit[h] - 1 ---------------------------
// (runtime.py:3674-3676: h = (1 - (g << 1)) * s_sign + 3; z = Zp.array(z + (h << l-1)) >> l.)
template <class F, bool NT>
__global__ __launch_bounds__(BLOCK) void k_sgn_finish(F f, const typename F::elem* __restrict__ w, const typename F::elem* __restrict__ sbit,
                                                       const typename F::elem* __restrict__ z, typename F::word half, typename F::word inv,
                                                       typename F::elem* __restrict__ o, size_t nvec, size_t n, int pol) {
    typedef typename F::word W;
    const W one = ff_one_elem(f);
    const W three = f.add(f.add(one, one), one);
    stream_map<F, NT>(o, nvec, n, pol, [=](W wv, W sb, W zv) -> W {
        const W s = f.sub(f.add(sb, sb), one);
        const W v = f.add(ff_pick(sgn_is_zero(wv), f.neg(s), s), three);
        return f.mul(f.add(zv, f.mul(v, half)), inv);
    }, w, sbit, z);
}

}  // namespace ffgpu
