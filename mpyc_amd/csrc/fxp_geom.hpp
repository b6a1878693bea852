// fxp_geom.hpp -- index arithmetic and launch plans of the fixed-point kernels (fxp.hpp): the finish of the secure truncation
// (runtime.np_trunc, runtime.py:839-873) and the gate in front of the search of runtime._norm (runtime.py:4718-4727).  Plain C++
// (no HIP): the kernels, their launcher and the C ABI take every index from here, and tests/fxp_check.cpp walks the same
// functions with g++.  (The mask of the truncation owns a tile per workgroup: its geometry is sgn_geom.hpp, as it is.)
//
// trunc_finish is flat over the n elements.  The two norm kernels are flat over the COMPACT array (n, l - 1): the bits of an
// element below its sign bit, most significant first.  bits is what ffgpu_bits_finish writes, element-major (n, l), least
// significant first, so compact element c = h (l - 1) + j takes
//   src = h l + (l - 2 - j)     the bit of weight 2^(l-2-j): the row of element h read backwards from below the sign bit
//   top = h l + (l - 1)         the sign bit x_top of element h
// A thread owns a unit: a pack of cx_pack(eb) consecutive compact elements where whole packs apply (sort_geom.hpp: the
// pointers aligned and the array a whole number of cx_gran(eb) elements -- whole waves for 24-byte elements), a single
// element otherwise.  The compact side (the output; the sub-share rows of norm_apply) moves as packs; the reversed reads and
// x_top are element loads -- a pack of compact elements may straddle two rows, and its sources run backwards.
#pragma once
#include "sort_geom.hpp"

namespace ffgpu {

enum { FXP_MAX_BITS = 64 };

// ---- trunc_finish: one flat loop over n --------------------------------------------------------------------------------------
struct FxpFlatPlan {
    int ok;                 // 0: sizes overflow -- nothing may be launched
    int vec;                // whole packs apply
    size_t total;           // units of the flat loop
};
FFCX_HD FxpFlatPlan fxp_flat_plan(size_t n, size_t eb, bool aligned) {
    FxpFlatPlan pl = FxpFlatPlan();
    size_t bytes;
    if (eb < 4 || eb % 4) return pl;
    if (!cx_mul_ok(n, eb, bytes) || bytes > ((size_t)1 << 62)) return pl;
    pl.ok = 1;
    pl.vec = aligned && n != 0 && n % cx_gran(eb) == 0;
    pl.total = n / (pl.vec ? cx_pack(eb) : 1);
    return pl;
}

// ---- norm_prod / norm_apply: one flat loop over the compact (n, l - 1) array ------------------------------------------------------
FFCX_HD bool fxp_norm_l_valid(int l) { return l >= 2 && l <= FXP_MAX_BITS; }

struct FxpNormPlan {
    int ok;                 // 0: l out of range, sizes overflow -- nothing may be launched
    int vec;                // whole packs apply
    unsigned pack;          // compact elements of a unit: cx_pack(eb) when vec, else 1
    size_t l, l1;           // bits of an element, and l - 1: the length of a compact row
    size_t elems;           // n * (l - 1): compact elements
    size_t total;           // units of the flat loop
    int shift;              // log2(l1) when a power of two, else -1
    int narrow;             // every compact index fits 32 bits
};
FFCX_HD FxpNormPlan fxp_norm_plan(size_t n, int l, size_t eb, bool aligned) {
    FxpNormPlan pl = FxpNormPlan();
    size_t nl, bytes;
    if (!fxp_norm_l_valid(l) || eb < 4 || eb % 4) return pl;
    if (!cx_mul_ok(n, (size_t)l, nl) || !cx_mul_ok(nl, eb, bytes) || bytes > ((size_t)1 << 62)) return pl;
    pl.ok = 1;
    pl.l = (size_t)l;
    pl.l1 = (size_t)l - 1;
    pl.elems = n * pl.l1;
    pl.vec = aligned && pl.elems != 0 && pl.elems % cx_gran(eb) == 0;
    pl.pack = pl.vec ? cx_pack(eb) : 1u;
    pl.total = pl.elems / pl.pack;
    pl.shift = cx_pow2(pl.l1) ? cx_log2(pl.l1) : -1;
    pl.narrow = pl.elems <= 0xffffffffu;
    return pl;
}

// ---- what a lane does with compact element c (the kernels call exactly these) ---------------------------------------------------------
struct FxpNormAt {
    size_t h, j;            // element and position below the sign bit, most significant first: c = h (l - 1) + j
    size_t src, top;        // elements of bits: the bit of weight 2^(l-2-j) and the sign bit of element h
};
FFCX_HD FxpNormAt fxp_norm_at(const FxpNormPlan& pl, size_t c) {
    FxpNormAt at;
    at.h = cx_div(c, pl.l1, pl.shift, pl.narrow);
    at.j = c - at.h * pl.l1;
    at.top = at.h * pl.l + pl.l1;
    at.src = at.top - 1 - at.j;
    return at;
}
// compact element c + 1 from compact element c, without a division: the next unit member of a pack
FFCX_HD void fxp_norm_next(const FxpNormPlan& pl, FxpNormAt& at) {
    ++at.j;
    --at.src;
    if (at.j == pl.l1) {
        at.j = 0;
        ++at.h;
        at.top += pl.l;
        at.src = at.top - 1;
    }
}

}  // namespace ffgpu
