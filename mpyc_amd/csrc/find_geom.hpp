// find_geom.hpp -- a round of the first-occurrence search behind runtime.np_find (runtime.py:4603-4698) in closed form, and
// the plan of the three kernels of find.hpp.  Plain C++ (no HIP): the kernels, their launcher and the C ABI take every index
// from here, and tests/find_check.cpp walks the same functions with g++.
//
// A node of the search tree is the stack (nf, v_1 .. v_F): C = 1 + F components, nf = 1 for "no 0 in my interval".  The
// combine of two neighbouring intervals, combine(L, R) = L + nf_L (R - L) (np_where(nf[0], R, L), runtime.py:4684), is
// associative and keeps order, so the tree may pair neighbours: the ODD_EVEN pairing of tour_geom.hpp over kk positions,
// n0 = kk % 2, h = kk / 2 pairs (n0 + 2j, n0 + 2j + 1), kc = h + n0 survivors, position 0 the bye when n0.
//
// A stored LEVEL is component-major (C, outer, kk, inner): component q is the contiguous (outer, kk, inner) array at
// q * outer * kk * inner, so a round over it is a round of tour_geom.hpp per component (TourPlan / tour_at as they are) plus
// the three distances between components: of the full level, of the next (half) level and of the compact products.
//
// The LEAF level is never stored.  The bits are (outer, k, inner) and the pairing runs over kv = k + virt positions: with
// virt, position k is the public leaf (1, f(e)); it is the second member of the last pair, always, and has no memory behind
// it.  The leaf round is therefore the ODD_EVEN plan over kv whose full-level pitch is the bits' k * inner, and whose last
// pair's second member is flagged and given the address of its first member (a load that is issued and not used), so that
// the virtual position never becomes a bit address.  position(first) = n0 + 2b indexes the leaf table (F, 2, kv).
#pragma once
#include "tour_geom.hpp"

namespace ffgpu {

enum { FIND_MIN_COMP = 2, FIND_MAX_COMP = 5 };      // C = 1 + F, 1 <= F <= 4

FFG_HD bool find_comp_valid(int ncomp) { return ncomp >= FIND_MIN_COMP && ncomp <= FIND_MAX_COMP; }

// ---- the plan of a launch -----------------------------------------------------------------------------------------------------
// t counts units as TourPlan does (packs when t.vec, else elements); so do the three plane distances.  Whole packs need what
// tour_plan() needs; `inner` a multiple of geom_gran(eb) then makes every component plane, every row of the bits and the
// position of a unit whole as well (a pack never straddles two positions).
struct FindPlan {
    TourPlan t;             // the ODD_EVEN round over kk (a stored level) or kv (the leaf round, pitch_full = k * inner)
    int virt;               // the leaf round has the public leaf at position k
    size_t kv;              // positions of the leaf round: the row length of the leaf table
    size_t plane_full;      // units between two components of a stored full level: outer * kk * inner elements
    size_t plane_half;      // ... of the next level: outer * kc * inner
    size_t plane_c;         // ... of the compact products: outer * h * inner
};

// a stored level (C, outer, k, inner), k >= 2
FFG_HD FindPlan find_plan(size_t outer, size_t k, size_t inner, int ncomp, size_t eb, bool aligned) {
    FindPlan pl = FindPlan();
    size_t n, all;
    if (!find_comp_valid(ncomp)) return pl;
    pl.t = tour_plan(outer, k, inner, TOUR_ODD_EVEN, eb, aligned);
    if (!pl.t.ok) return pl;
    n = outer * k * inner;                      // (tour_plan() has checked this product)
    if (!geom_mul_ok(n, (size_t)ncomp, all) || !geom_size_ok(all, eb)) {
        pl.t.ok = 0;
        return pl;
    }
    pl.kv = k;
    const size_t u = pl.t.vec ? geom_pack(eb) : 1;
    pl.plane_full = n / u;
    pl.plane_half = outer * pl.t.next * inner / u;
    pl.plane_c = outer * pl.t.row_elems / u;
    return pl;
}

// the leaf round: bits (outer, k, inner), k >= 1, kv = k + virt >= 2 positions
FFG_HD FindPlan find_leaf_plan(size_t outer, size_t k, size_t inner, int ncomp, int virt, size_t eb, bool aligned) {
    FindPlan pl = FindPlan();
    if (k < 1 || (virt != 0 && virt != 1)) return pl;
    pl = find_plan(outer, k + (size_t)virt, inner, ncomp, eb, aligned);
    if (!pl.t.ok) return pl;
    pl.virt = virt;
    pl.plane_full = 0;                          // (no stored full level)
    if (outer == 0 || inner == 0) return pl;
    pl.t.pitch_full = k * inner / (pl.t.vec ? geom_pack(eb) : 1);
    return pl;
}

// ---- what a lane does with flat unit g of the leaf round (the kernels call exactly this) -------------------------------------------
struct FindAt {
    size_t c;               // unit of a compact component
    size_t first, second;   // the pair's members in the bits; second == first when virt2
    int virt2;              // the second member is the public leaf: its bit is the public 1 and is not loaded
    size_t pos;             // the position of the first member (the second's is pos + 1): the column of the leaf table
    size_t half;            // the pair's position in a component of the next level
    int bye;                // this unit also carries a unit of the bye (position 0):
    size_t bye_full, bye_half;      // where it lies in the bits and in a component of the next level
};
FFG_HD FindAt find_leaf_at(const FindPlan& pl, size_t g) {
    const TourPlan& t = pl.t;
    const PairAt w = pair_split(t, g);
    FindAt at;
    at.c = g;
    at.first = w.o * t.pitch_full + t.bye + w.b * t.run + w.c;      // b * 2 run + (c - b * run)
    at.virt2 = pl.virt && w.b + 1 == t.pairs;
    at.second = at.virt2 ? at.first : at.first + t.run;
    at.pos = (pl.kv & 1) + 2 * w.b;
    at.half = w.o * t.pitch_half + t.bye + w.c;
    at.bye = w.c < t.bye;
    at.bye_full = w.o * t.pitch_full + w.c;
    at.bye_half = w.o * t.pitch_half + w.c;
    return at;
}

}  // namespace ffgpu
