// sort_geom.hpp -- the stages of Batcher's merge-exchange network (runtime.np_sort, runtime.py:1738-1774; Knuth 5.2.2M) in
// closed form, and the plan of the two compare-exchange kernels (sort.hpp).  Plain C++ (no HIP): the kernels, their
// launcher and the C ABI take every index from here, and tests/sort_check.cpp walks the same functions with g++.
//
// The array is contiguous row-major (outer, k, inner), element (o, j, i) at (o * k + j) * inner + i; the network runs
// along k.  A stage is (p, d, r): p a power of two, and either r == 0 with d == p, or r == p with d + p a larger power of
// two.  Its index set is I = { i < k - d : i & p == r }; every i in I is paired with i + d.
//   I_j = (j / p) * 2p + (j % p) + r                                  the j-th member of I, ascending
//   P   = (k - d) / 2p * p + min(max((k - d) % 2p - r, 0), p)         pairs of the stage
//   I and I + d are disjoint, so whoever owns pair j owns both of its members.
// p consecutive j are p consecutive positions of both members and of the compact pair array (outer, P, inner): a RUN of
// p * inner contiguous elements.  With c the index of an element of a compact row (c < P * inner), b = c / run and
// w = c % run, the pair's members are at  b * 2 run + w + r * inner  and  d * inner  further on in the row of `a`.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { CX_THREADS = 256 };                  // = GEOM_THREADS; tests/test_gpu_rbits.py reads the workgroup size off this line
static_assert((int)CX_THREADS == (int)GEOM_THREADS, "the compare-exchange kernels run the library's workgroup");

// ---- the stage list: the reference's loop over (p, d, q, r) ------------------------------------------------------------------
//   t = (k-1).bit_length(); p = 1 << t-1
//   while p: d, q, r = p, 1 << t-1, 0
//            while d: <stage (p, d, r)>; d, q, r = q - p, q >> 1, p
//            p >>= 1
struct CxStageIter {
    size_t p, d, q, r, top;                 // top = 1 << t-1; p == 0: past the last stage
};
FFG_HD CxStageIter cx_stages_begin(size_t k) {
    CxStageIter it = CxStageIter();
    if (k < 2) return it;
    size_t top = 1;
    while (top <= (k - 1) / 2) top <<= 1;                     // the highest power of two <= k - 1
    it.p = it.d = it.q = it.top = top;
    return it;
}
FFG_HD bool cx_stages_done(const CxStageIter& it) { return it.p == 0; }
FFG_HD void cx_stages_next(CxStageIter& it) {
    it.d = it.q - it.p;
    it.q >>= 1;
    it.r = it.p;
    if (it.d == 0) {
        it.p >>= 1;
        it.d = it.p;
        it.q = it.top;
        it.r = 0;
    }
}

// ---- one stage ---------------------------------------------------------------------------------------------------------------
FFG_HD bool cx_stage_valid(size_t k, size_t p, size_t d, size_t r) {
    if (k < 2 || !geom_pow2(p)) return false;
    if (r == 0) return d == p;
    if (r != p) return false;
    const size_t q = d + p;
    return q > d && q > p && geom_pow2(q);    // (q > d: no wrap-around)
}
// pairs of the stage; 0 for an invalid stage
FFG_HD size_t cx_pairs(size_t k, size_t p, size_t d, size_t r) {
    if (!cx_stage_valid(k, p, d, r) || d >= k || p >= k) return 0;
    const int lg = geom_log2(p);
    const size_t m = k - d;
    const size_t full = (m >> lg) >> 1;                      // m / 2p
    const size_t rem = m - ((full << lg) << 1);              // m % 2p
    const size_t tail = rem > r ? (rem - r < p ? rem - r : p) : 0;
    return (full << lg) + tail;
}
// the j-th member of I (lg = log2 p)
FFG_HD size_t cx_index_lg(size_t j, int lg, size_t r) { return ((j >> lg) << (lg + 1)) + (j & (((size_t)1 << lg) - 1)) + r; }
FFG_HD size_t cx_index(size_t j, size_t p, size_t r) { return cx_index_lg(j, geom_log2(p), r); }

// ---- the plan of a launch ------------------------------------------------------------------------------------------------------
// Everything below `vec` counts UNITS: packs of geom_pack(eb) elements when vec, single elements otherwise.  Whole packs apply
// when a run, a compact row and the byte pitch of a row of `a` are whole numbers of geom_gran(eb) elements / geom_align(eb)
// bytes and the pointers are aligned.  The flat loop is the pair walk of geom.hpp (always a shift, for run, when inner is one).
struct CxPlan {
    int ok;                 // 0: invalid stage, sizes overflow -- nothing may be launched
    size_t pairs;           // P
    size_t row_elems;       // P * inner: elements of a compact row
    int vec;                // whole packs apply
    size_t row_units;       // units of a compact row
    size_t run;             // units of a run: p * inner elements
    size_t pitch;           // units between two rows of `a`: k * inner elements
    size_t off_r, off_d;    // units from the start of a run pair to its first member, and from there to the second
    size_t total;           // outer * row_units: the flat loop
    int run_shift, row_shift;   // log2 of run / row_units when a power of two, else -1
    int narrow;             // every flat index and divisor fits 32 bits
};
FFG_HD CxPlan cx_plan(size_t outer, size_t k, size_t inner, size_t p, size_t d, size_t r, size_t eb, bool aligned) {
    CxPlan pl = CxPlan();
    size_t rowa, n;
    if (!cx_stage_valid(k, p, d, r)) return pl;
    if (!geom_mul_ok(k, inner, rowa) || !geom_mul_ok(outer, rowa, n) || !geom_size_ok(n, eb)) return pl;
    pl.ok = 1;
    pl.pairs = cx_pairs(k, p, d, r);
    pl.row_elems = pl.pairs * inner;        // (P <= k / 2 and d < k when P > 0: the products below stay under n)
    if (pl.pairs == 0 || outer == 0 || inner == 0) return pl;
    const size_t run = p * inner;
    const unsigned g = geom_gran(eb);
    pl.vec = aligned && run % g == 0 && pl.row_elems % g == 0 && (rowa * eb) % geom_align(eb) == 0;
    const size_t u = pl.vec ? geom_pack(eb) : 1;
    pair_fill(pl, outer, pl.row_elems, run, u);
    pl.pitch = rowa / u;
    pl.off_r = r * inner / u;
    pl.off_d = d * inner / u;
    return pl;
}

// ---- what a lane does with flat unit g (the kernels call exactly this) ---------------------------------------------------------------
struct CxAt {
    size_t lo, hi, c;       // units: first and second member in `a`, and the unit of the compact array
};
FFG_HD CxAt cx_at(const CxPlan& pl, size_t g) {
    const PairAt w = pair_split(pl, g);
    CxAt at;
    at.lo = w.o * pl.pitch + w.b * pl.run + w.c + pl.off_r;        // b * 2 run + (c - b * run)
    at.hi = at.lo + pl.off_d;
    at.c = g;
    return at;
}

}  // namespace ffgpu
