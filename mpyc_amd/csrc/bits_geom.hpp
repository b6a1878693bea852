// bits_geom.hpp -- the prefix-carry network of runtime.np_add_bits (runtime.py:4301-4334) as rounds of independent
// products, and the plan of the two level kernels (bits.hpp).  Plain C++ (no HIP): the kernels, their launcher and the C ABI
// take every index from here, and tests/bits_check.cpp walks the same functions with g++.
//
// The reference's recursion f(i, j, high) over bit positions [i, j) splits at h = i + (j - i) / 2 and merges with
//   c2 += c1[-1] * d2                  G[k] += G[h-1] * P[k]   for h <= k < j
//   d2 *= d1[-1]     when high         P[k]  = P[h-1] * P[k]   for h <= k < j
// (c: generate / carry, d: propagate).  The root is not high, a left child inherits `high`, a right child is always high;
// high <=> i > 0.  A merge over j - i positions runs in ROUND rho = ceil(log2(j - i)), rho = 1 .. ceil(log2 l): the
// children of a merge are shorter than it by at least a half, so they lie in earlier rounds; the merges of one round
// cover disjoint positions; and the only values a round reads that it also writes are G[k] / P[k] of the product's own k
// (q = h - 1 lies in the left half, which the round does not write).  So within a round every product reads values from
// before the round: the products of a round are formed first (compact rows), re-shared, and applied afterwards.
//
// Round rho is a list of c-products  G[q] * P[k]  for every k of the right half of every merge of the round, q = h - 1, k
// ascending, followed by the d-products  P[q] * P[k]  for the same (k, q) of the merges with i > 0, k ascending:
// R = Rc + Rd product rows, at most 63 for l <= 64 (l = 64, round 1: 32 + 31; R may reach or pass l, as for l = 6, round 2:
// 4 + 2).  G, P and the compact products are bit-major: row k is n contiguous elements at k * n.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { BITS_MAX_L = 64 };
enum { BITS_MAX_ROWS = 63 };                // the widest round of any l <= 64 (tests/bits_check.cpp walks them all)

// rounds of the network: ceil(log2 l); 0 for l == 1, -1 for an l out of range
FFG_HD int bits_rounds(int l) {
    if (l < 1 || l > BITS_MAX_L) return -1;
    int r = 0;
    while (((size_t)1 << r) < (size_t)l) ++r;
    return r;
}
// ceil(log2 n), n >= 1
FFG_HD int bits_height(int n) {
    int r = 0;
    while ((1 << r) < n) ++r;
    return r;
}

// One round: rows 0 .. rc-1 are the c-products, rows rc .. rc+rd-1 the d-products; row j multiplies row q[j] (of G for a
// c-product, of P for a d-product) with row k[j] of P, and its recombined value goes to row k[j] (added to G / stored to P).
// The table travels to the kernels by value, in the kernel arguments.
struct BitsLevel {
    uint8_t rc, rd;
    uint8_t k[BITS_MAX_ROWS], q[BITS_MAX_ROWS];
};

// the merges of round `round` below [i, j), left to right (so k ascends): c-rows appended at lv.rc, d-rows collected in dk / dq
inline void bits_collect(int i, int j, int round, BitsLevel& lv, uint8_t* dk, uint8_t* dq) {
    const int n = j - i;
    if (n < 2) return;
    const int ht = bits_height(n);
    if (ht < round) return;                  // every merge below is in an earlier round
    const int h = i + n / 2;
    if (ht > round) {
        bits_collect(i, h, round, lv, dk, dq);
        bits_collect(h, j, round, lv, dk, dq);
        return;
    }
    for (int k = h; k < j; ++k) {
        lv.k[lv.rc] = (uint8_t)k;
        lv.q[lv.rc] = (uint8_t)(h - 1);
        ++lv.rc;
        if (i > 0) {
            dk[lv.rd] = (uint8_t)k;
            dq[lv.rd] = (uint8_t)(h - 1);
            ++lv.rd;
        }
    }
}
// false: l or round out of range (1 <= l <= 64, 1 <= round <= bits_rounds(l))
inline bool bits_level(int l, int round, BitsLevel& lv) {
    lv = BitsLevel();
    const int rounds = bits_rounds(l);
    if (rounds < 0 || round < 1 || round > rounds) return false;
    uint8_t dk[BITS_MAX_ROWS], dq[BITS_MAX_ROWS];
    bits_collect(0, l, round, lv, dk, dq);
    for (int j = 0; j < lv.rd; ++j) {
        lv.k[lv.rc + j] = dk[j];
        lv.q[lv.rc + j] = dq[j];
    }
    return true;
}

// ---- the plan of a level launch -------------------------------------------------------------------------------------------
// Both level kernels run grid (gx, R): workgroup row y serves product row y (the table entry is then uniform over the
// workgroup), and the gx workgroups of a row stream its n elements in UNITS: packs of geom_pack(eb) elements when vec, single
// elements otherwise.  Whole packs apply when every row starts aligned: n a multiple of geom_gran(eb) (24-byte elements:
// whole waves, kernels.hpp ldgw / stgw), the byte pitch n * eb of a row a multiple of geom_align(eb), and aligned pointers.
// Unit u of product row y: the compact arrays at unit y * row_units + u, G / P row r at unit r * row_units + u.
struct BitsPlan {
    int ok;                 // 0: l or round out of range, sizes overflow -- nothing may be launched
    int rows;               // R
    int vec;                // whole packs apply
    size_t row_units;       // units of a row
    unsigned gx;            // workgroups per product row
};
FFG_HD BitsPlan bits_plan(size_t n, int l, int rows, size_t eb, bool aligned, size_t max_blocks) {
    BitsPlan pl = BitsPlan();
    size_t nl;
    if (l < 1 || l > BITS_MAX_L || rows < 0 || rows > BITS_MAX_ROWS) return pl;
    if (!geom_mul_ok(n, (size_t)l, nl) || !geom_size_ok(nl, eb)) return pl;
    pl.ok = 1;
    pl.rows = rows;
    if (rows == 0 || n == 0) return pl;
    pl.vec = aligned && n % geom_gran(eb) == 0 && (n * eb) % geom_align(eb) == 0;
    pl.row_units = pl.vec ? n / geom_pack(eb) : n;
    size_t want = (pl.row_units + GEOM_THREADS - 1) / GEOM_THREADS;
    size_t cap = max_blocks / (size_t)rows;
    if (cap < 1) cap = 1;
    if (cap > (size_t)GEOM_MAX_GRID) cap = (size_t)GEOM_MAX_GRID;
    pl.gx = (unsigned)(want < cap ? want : cap);
    return pl;
}
// the unit of row r that belongs with unit u of a row
FFG_HD size_t bits_unit(const BitsPlan& pl, int r, size_t u) { return (size_t)r * pl.row_units + u; }

}  // namespace ffgpu
