// explog_geom.hpp -- index arithmetic and launch plans of the kernels under the secure logarithm and exponential (explog.hpp):
// the doubling step of the power ladder (runtime.np_vander, runtime.py:4947-4977), the Taylor sum (runtime.py:4887, 4934),
// the fixed-base power with per-element exponents (runtime.py:1408, 1422) and np_flip along the bit axis (runtime.py:4876).
// Plain C++ (no HIP): the kernels, their launcher and the C ABI take every index from here, and tests/explog_check.cpp
// walks the same functions with g++.
//
// powers_prod and poly_dot are flat over the n elements of a row of the POWER-MAJOR block P: row j holds y^(j+1), n elements,
// rows `stride` elements apart: rows_plan / rows_unit (geom.hpp) as they are.
//
// bits_reverse is the reversed-row walk of geom.hpp with nothing left out: the compact row is the whole row, element
// c = h l + j reads bits[h l + l-1-j].
//
// pow_base reads its exponent in 4-bit windows: window i of element e is bits shift + 4 i .. shift + 4 i + 3 of the
// canonical integer, cut off at bit shift + ebits; the table holds g^(d 16^i) at  15 i + d - 1  for d = 1..15.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { POLY_MAX_TERMS = 64 };               // = MAXK_ANY (kernels.hpp): products one lazy accumulator takes
enum { POW_WIN_BITS = 4, POW_WIN_DIGITS = 15 };
enum { EXPLOG_REV_MAX_BITS = 64 };          // of a row of bits_reverse

// ---- powers_prod / poly_dot: the row counts the rows plan is asked for ---------------------------------------------------------
FFG_HD bool explog_prod_valid(int h, int w) { return h >= 1 && w >= 1 && w <= h; }
FFG_HD bool explog_poly_valid(int theta) { return theta >= 1 && theta <= POLY_MAX_TERMS; }

// ---- bits_reverse: whole rows backwards -------------------------------------------------------------------------------------
FFG_HD bool explog_rev_l_valid(int l) { return l >= 1 && l <= EXPLOG_REV_MAX_BITS; }
FFG_HD RevPlan explog_rev_plan(size_t n, int l, size_t eb, bool aligned) {
    if (!explog_rev_l_valid(l)) return RevPlan();
    return rev_plan(n, (size_t)l, false, eb, aligned);
}

// ---- pow_base: 4-bit windows of a canonical integer of up to three 64-bit limbs ---------------------------------------------
struct PowBasePlan {
    int ok;                 // 0: ebits or shift out of range, sizes overflow -- nothing may be launched
    int shift, ebits;
    int nwin;               // windows: ceil(ebits / 4)
    int tab_elems;          // elements of the table: 15 * nwin
};
FFG_CX int pow_base_max_windows(size_t eb) { return (int)(eb * 8 / POW_WIN_BITS); }
FFG_HD PowBasePlan pow_base_plan(size_t n, int shift, int ebits, int pbits, size_t eb) {
    PowBasePlan pl = PowBasePlan();
    if (!geom_size_ok(n, eb) || pbits < 1 || (size_t)pbits > eb * 8) return pl;
    if (ebits < 1 || ebits > pbits || shift < 0 || shift >= 192) return pl;
    pl.ok = 1;
    pl.shift = shift;
    pl.ebits = ebits;
    pl.nwin = (ebits + POW_WIN_BITS - 1) / POW_WIN_BITS;
    pl.tab_elems = POW_WIN_DIGITS * pl.nwin;
    return pl;
}
// window i < nwin of the integer limb[0] + limb[1] 2^64 + limb[2] 2^128 (limbs the word does not have are zero): 0..15
FFG_HD unsigned pow_base_digit(const PowBasePlan& pl, uint64_t l0, uint64_t l1, uint64_t l2, int i) {
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
FFG_HD int pow_base_slot(int i, unsigned d) { return POW_WIN_DIGITS * i + (int)d - 1; }

}  // namespace ffgpu
