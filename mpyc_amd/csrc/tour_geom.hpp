// tour_geom.hpp -- a round of the tournament behind runtime.np_amax / np_amin (runtime.py:3413-3419, 3462-3468) and
// runtime._np_argmax / _np_argmin (runtime.py:3806-3820, 3934-3948) in closed form, and the plan of the four kernels of
// tour.hpp.  Plain C++ (no HIP): the kernels, their launcher and the C ABI take every index from here, and
// tests/tour_check.cpp walks the same functions with g++.
//
// The array is contiguous row-major (outer, k, inner), element (o, j, i) at (o * k + j) * inner + i; the round runs along
// k >= 2.  n0 = k % 2, h = k / 2 pairs, kc = h + n0 survivors; position 0 is the bye when n0.  Pair j < h is
//   TOUR_HALVES     first_j = n0 + j,    second_j = kc + j            a[n0:(k+1)/2] against a[(k+1)/2:]
//   TOUR_ODD_EVEN   first_j = n0 + 2j,   second_j = n0 + 2j + 1       a[n0::2] against a[n0+1::2]: the first occurrence wins
// The pairs are disjoint and, with the bye, cover 0..k-1 once.  Three arrays meet in a round: the FULL level (outer, k,
// inner), the next (HALF) level (outer, kc, inner) whose position n0 + j belongs to pair j, and the COMPACT (outer, h,
// inner) arrays of differences, comparison bits and products.  A RUN is a stretch of compact elements whose two members are
// contiguous in the full level: h * inner elements for HALVES (the whole compact row), inner elements for ODD_EVEN.  With c
// the index of an element of a compact row (c < h * inner), b = c / run and w = c % run:
//   first member   o * k * inner + n0 * inner + b * 2 run + w       (b == 0 throughout for HALVES)
//   second member  run elements further on
//   half level     o * kc * inner + n0 * inner + c
// and the bye's `inner` elements at the start of a row go with the first `inner` compact elements of that row.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { TOUR_HALVES = 0, TOUR_ODD_EVEN = 1 };        // = FFGPU_TOUR_HALVES / FFGPU_TOUR_ODD_EVEN (include/ffgpu.h)

FFG_HD bool tour_mode_valid(int mode) { return mode == TOUR_HALVES || mode == TOUR_ODD_EVEN; }
FFG_HD size_t tour_pairs(size_t k) { return k / 2; }
FFG_HD size_t tour_next(size_t k) { return k / 2 + k % 2; }
FFG_HD size_t tour_first(size_t k, int mode, size_t j) { return mode == TOUR_HALVES ? k % 2 + j : k % 2 + 2 * j; }
FFG_HD size_t tour_second(size_t k, int mode, size_t j) { return mode == TOUR_HALVES ? tour_next(k) + j : k % 2 + 2 * j + 1; }

// ---- the plan of a launch ------------------------------------------------------------------------------------------------------
// Everything below `vec` counts UNITS: packs of geom_pack(eb) elements when vec, single elements otherwise (geom.hpp).
// Whole packs apply when a run, a compact row and the bye are multiples of geom_gran(eb) elements (24-byte elements: whole
// waves) and the pointers are aligned; every row of the three arrays then starts on a pack, and a wave on a wave.  The
// flat loop is the pair walk of geom.hpp.
struct TourPlan {
    int ok;                 // 0: k < 2, unknown mode, sizes overflow -- nothing may be launched
    size_t pairs, next;     // h, kc
    size_t row_elems;       // h * inner: elements of a compact row
    int vec;                // whole packs apply
    size_t row_units;       // units of a compact row
    size_t run;             // units of a run
    size_t pitch_full;      // units between two rows of the full level: k * inner elements
    size_t pitch_half;      // ... of the half level: kc * inner elements
    size_t bye;             // units of the bye at the start of a row: n0 * inner elements (= where pair 0 starts)
    size_t total;           // outer * row_units: the flat loop
    int run_shift, row_shift;   // log2 of run / row_units when a power of two, else -1
    int narrow;             // every flat index and divisor fits 32 bits
};
FFG_HD TourPlan tour_plan(size_t outer, size_t k, size_t inner, int mode, size_t eb, bool aligned) {
    TourPlan pl = TourPlan();
    size_t rowa, n;
    if (k < 2 || !tour_mode_valid(mode)) return pl;
    if (!geom_mul_ok(k, inner, rowa) || !geom_mul_ok(outer, rowa, n) || !geom_size_ok(n, eb)) return pl;
    pl.ok = 1;
    pl.pairs = tour_pairs(k);
    pl.next = tour_next(k);
    pl.row_elems = pl.pairs * inner;        // (h <= k: the products below stay under n)
    if (outer == 0 || inner == 0) return pl;
    const size_t run = mode == TOUR_HALVES ? pl.row_elems : inner;
    const size_t bye = (k % 2) * inner;
    const unsigned g = geom_gran(eb);
    pl.vec = aligned && run % g == 0 && pl.row_elems % g == 0 && bye % g == 0;     // (g * eb is a multiple of geom_align(eb))
    const size_t u = pl.vec ? geom_pack(eb) : 1;
    pair_fill(pl, outer, pl.row_elems, run, u);
    pl.pitch_full = rowa / u;
    pl.pitch_half = pl.next * inner / u;
    pl.bye = bye / u;
    return pl;
}

// ---- what a lane does with flat unit g (the kernels call exactly this) ---------------------------------------------------------
struct TourAt {
    size_t c;               // unit of the compact arrays
    size_t first, second;   // the pair's members in the full level
    size_t half;            // the pair's position in the half level
    int bye;                // this unit also carries a unit of the bye:
    size_t bye_full, bye_half;      // where it lies in the full and in the half level
};
FFG_HD TourAt tour_at(const TourPlan& pl, size_t g) {
    const PairAt w = pair_split(pl, g);
    TourAt at;
    at.c = g;
    at.first = w.o * pl.pitch_full + pl.bye + w.b * pl.run + w.c;   // b * 2 run + (c - b * run)
    at.second = at.first + pl.run;
    at.half = w.o * pl.pitch_half + pl.bye + w.c;
    at.bye = w.c < pl.bye;
    at.bye_full = w.o * pl.pitch_full + w.c;
    at.bye_half = w.o * pl.pitch_half + w.c;
    return at;
}

}  // namespace ffgpu
