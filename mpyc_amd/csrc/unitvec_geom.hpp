// unitvec_geom.hpp -- index arithmetic and launch plans of the three kernels under secure unit vectors and table lookup at
// secret indices (unitvec.hpp): the broadcast product of a demultiplexer round, the rotation of random unit vectors by an
// opened offset (runtime.np_unit_vector, runtime.py:5002-5029) and the table read through them.
// Plain C++ (no HIP): the kernels, their launcher and the C ABI take every index from here, and tests/unitvec_check.cpp walks
// the same functions with g++.
//
// Unit vectors are POSITION-MAJOR (rows, n): row j holds position j for the n indices, rows n elements apart.  All three
// kernels are flat over the n elements of a row: a thread owns a unit of every row it touches, which is the rows plan of
// geom.hpp with stride n.  Unit g of row j is unit  rows_unit(pl, j, g)  of the array.
//   * unit_prod: element q of unit g takes x[(g pack + q) xstride]: a pack of x itself when xstride == 1, gathered by
//     element otherwise (the element-major (n, l) bits of bits_finish: xstride = l);
//   * unit_roll: out row j < K of element e is source row  (j - c[e]) mod K2,  K2 = 2^kbits;
//   * unit_dot:  term j < rows of element e takes table entry  (j + c[e]) mod K2;  without c the entry j.
// c[e] mod K2 is the low kbits bits of the canonical integer: the low limb under the mask K2 - 1 (the high limbs are
// arbitrary), as the masked opening of the truncation (fxp.hpp) is cut.
//
// The table of unit_dot lives in dynamically sized LDS, one prepared WORD per entry (4, 8, 16, 16, 24 bytes for elements of
// 4, 8, 12, 16, 24 bytes), zero from tlen up; 64 KiB at the most: kbits <= 14, 13, 12, 12, 11.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { UNIT_MAX_KBITS = 30 };               // of a rotation: K2 = 2^kbits rows
enum { UNIT_LDS_BYTES = 65536 };            // the table of unit_dot

FFG_HD bool unit_kbits_valid(int kbits) { return kbits >= 0 && kbits <= UNIT_MAX_KBITS; }
FFG_HD uint64_t unit_mask(int kbits) { return ((uint64_t)1 << kbits) - 1; }

// ---- the rows plan of all three: `rows` dense rows of n elements; pl.span == rows * n --------------------------------------
FFG_HD RowsPlan unit_rows_plan(size_t n, size_t rows, size_t eb, bool aligned) {
    return rows_plan(n, rows, n, eb, aligned);
}
// element q of unit g, as an element of its row
FFG_HD size_t unit_elem(const RowsPlan& pl, size_t g, unsigned q) { return g * pl.pack + q; }

// ---- unit_prod: where the factor of element e sits in x; the elements x spans ----------------------------------------------
FFG_HD size_t unit_x_at(size_t e, size_t xstride) { return e * xstride; }
FFG_HD bool unit_x_span(size_t n, size_t xstride, size_t eb, size_t& span) {
    size_t above;
    span = 0;
    if (xstride < 1) return false;
    if (n == 0) return true;
    if (!geom_mul_ok(n - 1, xstride, above) || above + 1 < above) return false;
    span = above + 1;
    return geom_bytes_ok(span, eb);
}
// a pack of x serves a unit as it is: consecutive factors (and x aligned, which the launcher knows)
FFG_HD bool unit_x_packs(const RowsPlan& pl, size_t xstride) { return pl.vec && xstride == 1; }

// ---- unit_roll / unit_dot: the rotation ---------------------------------------------------------------------------------------
// the offset of an element from the low limb of its canonical opened value
FFG_HD size_t unit_offset(uint64_t low_limb, uint64_t mask) { return (size_t)(low_limb & mask); }
// source row of out row j:  (j - off) mod K2,  off <= mask = K2 - 1
FFG_HD size_t unit_roll_src(size_t j, size_t off, uint64_t mask) { return (j + ((size_t)mask + 1 - off)) & (size_t)mask; }
// table entry of term j:  (j + off) mod K2;  without a rotation off == 0 and mask == ~0
FFG_HD size_t unit_dot_tab(size_t j, size_t off, uint64_t mask) { return (j + off) & (size_t)mask; }
FFG_HD bool unit_roll_valid(int kbits, size_t K) { return unit_kbits_valid(kbits) && K >= 1 && K <= ((size_t)1 << kbits); }

// ---- unit_dot: the table in LDS ---------------------------------------------------------------------------------------------------
FFG_CX size_t unit_word_bytes(size_t eb) { return eb == 4 ? 4u : eb == 8 ? 8u : eb == 24 ? 24u : 16u; }
FFG_CX int unit_dot_max_kbits(size_t eb) {
    int k = 0;
    while (((size_t)2 << k) * unit_word_bytes(eb) <= (size_t)UNIT_LDS_BYTES) ++k;
    return k;
}
struct UnitDotPlan {
    int ok;                 // 0: counts out of range -- FFGPU_EINVAL
    int fits;               // 0: the table does not fit LDS -- FFGPU_ENOTSUP
    size_t entries;         // entries of the table in LDS: K2 with a rotation, rows without
    size_t lds_bytes;
    uint64_t mask;          // K2 - 1 with a rotation, all ones without
};
FFG_HD UnitDotPlan unit_dot_plan(size_t rows, bool rotated, int kbits, size_t tlen, size_t eb) {
    UnitDotPlan pl = UnitDotPlan();
    if (rows < 1 || tlen < 1) return pl;
    if (rotated) {
        if (!unit_kbits_valid(kbits) || rows != ((size_t)1 << kbits) || tlen > rows) return pl;
        pl.mask = unit_mask(kbits);
    } else {
        if (tlen != rows) return pl;
        pl.mask = ~(uint64_t)0;
    }
    pl.ok = 1;
    pl.entries = rows;
    pl.fits = rows <= (size_t)UNIT_LDS_BYTES / unit_word_bytes(eb);
    pl.lds_bytes = pl.fits ? rows * unit_word_bytes(eb) : 0;
    return pl;
}

}  // namespace ffgpu
