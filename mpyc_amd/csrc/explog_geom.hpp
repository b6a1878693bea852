// explog_geom.hpp -- index arithmetic and launch plans of the kernels under the secure logarithm and exponential (explog.hpp):
// the doubling step of the power ladder (runtime.np_vander, runtime.py:4947-4977), the Taylor sum (runtime.py:4887, 4934),
// the fixed-base power with per-element exponents (runtime.py:1408, 1422) and np_flip along the bit axis (runtime.py:4876).
// Plain C++ (no HIP): the kernels, their launcher and the C ABI take every index from here, and tests/explog_check.cpp
// walks the same functions with g++.
//
// powers_prod and poly_dot are flat over the n elements of a row of the POWER-MAJOR block P: row j holds y^(j+1), n elements,
// rows `stride` elements apart.  A thread owns a unit of every row it touches: a pack of cx_pack(eb) consecutive elements
// where whole packs apply (sort_geom.hpp: pointers and row pitch aligned, n a whole number of cx_gran(eb) elements -- whole
// waves for 24-byte elements), a single element otherwise.  Unit g of row j is unit  j * pitch + g  of the block.
//
// bits_reverse is the compact reversed index of fxp_geom.hpp with nothing left out: a plan whose compact row is the whole
// row (l1 == l), walked with fxp_norm_at / fxp_norm_next as they are -- element c = h l + j reads bits[h l + l-1-j].
//
// pow_base reads its exponent in 4-bit windows: window i of element e is bits shift + 4 i .. shift + 4 i + 3 of the
// canonical integer, cut off at bit shift + ebits; the table holds g^(d 16^i) at  15 i + d - 1  for d = 1..15.
#pragma once
#include "fxp_geom.hpp"

namespace ffgpu {

enum { POLY_MAX_TERMS = 64 };               // = MAXK_ANY (kernels.hpp): products one lazy accumulator takes
enum { POW_WIN_BITS = 4, POW_WIN_DIGITS = 15 };

// ---- powers_prod / poly_dot: one flat loop over the n elements of a row -------------------------------------------------------
struct ExplogRowsPlan {
    int ok;                 // 0: row count out of range, stride < n, sizes overflow -- nothing may be launched
    int vec;                // whole packs apply
    unsigned pack;          // elements of a unit: cx_pack(eb) when vec, else 1
    size_t total;           // units of the flat loop = units of a row
    size_t pitch;           // units between two rows of the block
    size_t span;            // elements from the block's first to one past its last: (rows - 1) * stride + n
};
FFCX_HD ExplogRowsPlan explog_rows_plan(size_t n, size_t rows, size_t stride, size_t eb, bool aligned) {
    ExplogRowsPlan pl = ExplogRowsPlan();
    size_t above, bytes;
    if (eb < 4 || eb % 4 || rows < 1 || stride < n) return pl;
    if (!cx_mul_ok(rows - 1, stride, above) || above + n < above) return pl;
    if (!cx_mul_ok(above + n, eb, bytes) || bytes > ((size_t)1 << 62)) return pl;
    pl.ok = 1;
    pl.span = above + n;
    pl.vec = aligned && n != 0 && n % cx_gran(eb) == 0 && (rows == 1 || (stride * eb) % cx_align(eb) == 0);
    pl.pack = pl.vec ? cx_pack(eb) : 1u;
    pl.vec = pl.vec && (rows == 1 || stride % pl.pack == 0);
    if (!pl.vec) pl.pack = 1u;
    pl.total = n / pl.pack;
    pl.pitch = stride / pl.pack;
    return pl;
}
// unit g of row j, in units of the block
FFCX_HD size_t explog_row_unit(const ExplogRowsPlan& pl, size_t j, size_t g) { return j * pl.pitch + g; }

FFCX_HD bool explog_prod_valid(int h, int w) { return h >= 1 && w >= 1 && w <= h; }
FFCX_HD bool explog_poly_valid(int theta) { return theta >= 1 && theta <= POLY_MAX_TERMS; }

// ---- bits_reverse: the reversed index of fxp_geom.hpp over whole rows -----------------------------------------------------
FFCX_HD bool explog_rev_l_valid(int l) { return l >= 1 && l <= FXP_MAX_BITS; }
FFCX_HD FxpNormPlan explog_rev_plan(size_t n, int l, size_t eb, bool aligned) {
    FxpNormPlan pl = FxpNormPlan();
    size_t nl, bytes;
    if (!explog_rev_l_valid(l) || eb < 4 || eb % 4) return pl;
    if (!cx_mul_ok(n, (size_t)l, nl) || !cx_mul_ok(nl, eb, bytes) || bytes > ((size_t)1 << 62)) return pl;
    pl.ok = 1;
    pl.l = pl.l1 = (size_t)l;               // the compact row is the whole row: src = h l + l-1-j (top = h l + l is never read)
    pl.elems = nl;
    pl.vec = aligned && pl.elems != 0 && pl.elems % cx_gran(eb) == 0;
    pl.pack = pl.vec ? cx_pack(eb) : 1u;
    pl.total = pl.elems / pl.pack;
    pl.shift = cx_pow2(pl.l1) ? cx_log2(pl.l1) : -1;
    pl.narrow = pl.elems <= 0xffffffffu;
    return pl;
}

// ---- pow_base: 4-bit windows of a canonical integer of up to three 64-bit limbs ---------------------------------------------
struct PowBasePlan {
    int ok;                 // 0: ebits or shift out of range, sizes overflow -- nothing may be launched
    int shift, ebits;
    int nwin;               // windows: ceil(ebits / 4)
    int tab_elems;          // elements of the table: 15 * nwin
};
FFCX_CX int pow_base_max_windows(size_t eb) { return (int)(eb * 8 / POW_WIN_BITS); }
FFCX_HD PowBasePlan pow_base_plan(size_t n, int shift, int ebits, int pbits, size_t eb) {
    PowBasePlan pl = PowBasePlan();
    size_t bytes;
    if (eb < 4 || eb % 4 || pbits < 1 || (size_t)pbits > eb * 8) return pl;
    if (ebits < 1 || ebits > pbits || shift < 0 || shift >= 192) return pl;
    if (!cx_mul_ok(n, eb, bytes) || bytes > ((size_t)1 << 62)) return pl;
    pl.ok = 1;
    pl.shift = shift;
    pl.ebits = ebits;
    pl.nwin = (ebits + POW_WIN_BITS - 1) / POW_WIN_BITS;
    pl.tab_elems = POW_WIN_DIGITS * pl.nwin;
    return pl;
}
// window i < nwin of the integer limb[0] + limb[1] 2^64 + limb[2] 2^128 (limbs the word does not have are zero): 0..15
FFCX_HD unsigned pow_base_digit(const PowBasePlan& pl, uint64_t l0, uint64_t l1, uint64_t l2, int i) {
    const int b = pl.shift + POW_WIN_BITS * i;              // < 192 + 192
    const int q = b >> 6, r = b & 63;
    const uint64_t cur = q == 0 ? l0 : q == 1 ? l1 : q == 2 ? l2 : 0;
    const uint64_t nxt = q == 0 ? l1 : q == 1 ? l2 : 0;
    uint64_t d = cur >> r;
    if (r > 64 - POW_WIN_BITS) d |= nxt << (64 - r);
    const int left = pl.ebits - POW_WIN_BITS * i;           // bits of the exponent from this window on: >= 1
    const unsigned mask = left >= POW_WIN_BITS ? 15u : (1u << left) - 1u;
    return (unsigned)d & mask;
}
// where g^(d 16^i) sits, d in 1..15
FFCX_HD int pow_base_slot(int i, unsigned d) { return POW_WIN_DIGITS * i + (int)d - 1; }

}  // namespace ffgpu
