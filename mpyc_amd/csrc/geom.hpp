// geom.hpp -- what the geometry headers (*_geom.hpp) share: the host/device macro pair, the checked product, the pack of an
// element size, the size guard of every plan, the four plans that are flat over units, and the pair walk of the sorting
// network, the tournament and the search.  Plain C++ (no HIP), and it includes none of the project's headers: the kernels,
// their launchers, the C ABI and the tests/*_check.cpp programs (g++) all take these from here; tests/geom_check.cpp walks
// them by brute force.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FFG_HD __host__ __device__ __forceinline__
#define FFG_CX __host__ __device__ constexpr
#else
#define FFG_HD inline
#define FFG_CX constexpr
#endif

namespace ffgpu {

enum { GEOM_THREADS = 256 };                // threads of a workgroup = BLOCK (kernels.hpp)
enum { GEOM_MAX_GRID = 0x7fffffff };        // workgroups of a grid dimension

FFG_HD bool geom_pow2(size_t x) { return x != 0 && (x & (x - 1)) == 0; }
FFG_HD int geom_log2(size_t x) {            // x a power of two
    int s = 0;
    while ((x >> s) > 1) ++s;
    return s;
}
// a * b, false on overflow
FFG_HD bool geom_mul_ok(size_t a, size_t b, size_t& r) {
    r = a * b;
    return a == 0 || r / a == b;
}
// x / y: a shift where y is a power of two (shift = log2 y, else -1), a 32-bit division where both fit (narrow)
FFG_HD size_t geom_div(size_t x, size_t y, int shift, int narrow) {
    if (shift >= 0) return x >> shift;
    if (narrow) return (size_t)((uint32_t)x / (uint32_t)y);
    return x / y;
}

// ---- packs ---------------------------------------------------------------------------------------------------------------------
// What one lane moves per access (elements), what a stretch of elements must be a multiple of for whole packs to apply, and
// the byte alignment of a pack, per element size (bytes): 4 -> four elements in 16 bytes, 8 -> two, 12 -> one (dwordx3,
// dword aligned), 16 -> one, 24 -> one per lane, but the WAVE moves its 64 elements as one 16-byte aligned span
// (kernels.hpp, ldgw / stgw): whole waves.  (1 -> sixteen: the bytes of GF(2^8), four to a word; no plan below takes them.)
FFG_CX unsigned geom_pack(size_t eb) { return eb == 1 ? 16u : eb == 4 ? 4u : eb == 8 ? 2u : 1u; }
FFG_CX unsigned geom_gran(size_t eb) { return eb == 24 ? 64u : geom_pack(eb); }
FFG_CX unsigned geom_align(size_t eb) { return eb == 12 ? 4u : 16u; }

// ---- the size guard of every plan ------------------------------------------------------------------------------------------------
// count * eb neither wraps nor exceeds 2^62
FFG_HD bool geom_bytes_ok(size_t count, size_t eb) {
    size_t bytes;
    return geom_mul_ok(count, eb, bytes) && bytes <= ((size_t)1 << 62);
}
// ... and eb is the size of a prime field's element: 4, 8, 12, 16 or 24
FFG_HD bool geom_size_ok(size_t count, size_t eb) {
    return (eb == 4 || eb == 8 || eb == 12 || eb == 16 || eb == 24) && geom_bytes_ok(count, eb);
}

// A thread owns a UNIT: a pack of geom_pack(eb) consecutive elements where whole packs apply (`vec`: the pointers aligned and
// every stretch a whole number of geom_gran(eb) elements), a single element otherwise.

// ---- flat: one loop over n elements -------------------------------------------------------------------------------------------------
struct FlatPlan {
    int ok;                 // 0: sizes refused -- nothing may be launched
    int vec;                // whole packs apply
    unsigned pack;          // elements of a unit: geom_pack(eb) when vec, else 1
    size_t total;           // units of the flat loop
};
FFG_HD FlatPlan flat_plan(size_t n, size_t eb, bool aligned) {
    FlatPlan pl = FlatPlan();
    if (!geom_size_ok(n, eb)) return pl;
    pl.ok = 1;
    pl.vec = aligned && n != 0 && n % geom_gran(eb) == 0;
    pl.pack = pl.vec ? geom_pack(eb) : 1u;
    pl.total = n / pl.pack;
    return pl;
}

// ---- rows: one loop over the n elements of a row, `rows` rows `stride` elements apart -------------------------------------------
// A thread owns the same unit of every row it touches; whole packs also need every row to start on one.
struct RowsPlan {
    int ok;                 // 0: rows < 1, stride < n, sizes refused -- nothing may be launched
    int vec;                // whole packs apply
    unsigned pack;          // elements of a unit: geom_pack(eb) when vec, else 1
    size_t total;           // units of the flat loop = units of a row
    size_t pitch;           // units between two rows
    size_t span;            // elements from the first row's first to one past the last row's last: (rows - 1) * stride + n
};
FFG_HD RowsPlan rows_plan(size_t n, size_t rows, size_t stride, size_t eb, bool aligned) {
    RowsPlan pl = RowsPlan();
    size_t above;
    if (rows < 1 || stride < n) return pl;
    if (!geom_mul_ok(rows - 1, stride, above) || above + n < above || !geom_size_ok(above + n, eb)) return pl;
    pl.ok = 1;
    pl.span = above + n;
    pl.vec = aligned && n != 0 && n % geom_gran(eb) == 0 && (rows == 1 || (stride * eb) % geom_align(eb) == 0);
    pl.pack = pl.vec ? geom_pack(eb) : 1u;
    pl.vec = pl.vec && (rows == 1 || stride % pl.pack == 0);
    if (!pl.vec) pl.pack = 1u;
    pl.total = n / pl.pack;
    pl.pitch = stride / pl.pack;
    return pl;
}
// unit g of row j
FFG_HD size_t rows_unit(const RowsPlan& pl, size_t j, size_t g) { return j * pl.pitch + g; }

// ---- stream: packs through a vector loop, the rest through an element tail -----------------------------------------------------
// packs of n elements that go through the vector loop of a streaming kernel.  24-byte elements: whole waves only -- in
// `for (i = gid; i < nvec; i += gsz)` every wave is then entirely in or entirely out, which ldgw / stgw rely on
FFG_HD size_t stream_nvec(size_t n, size_t eb, bool vec) { return !vec ? 0 : eb == 24 ? (n & ~(size_t)63) : n / geom_pack(eb); }
struct StreamPlan {
    int ok;                 // 0: sizes refused -- nothing may be launched
    unsigned pack;          // elements of a pack: geom_pack(eb)
    size_t nvec;            // packs through the vector loop; 0: elements throughout
    size_t tail;            // first element of the tail: nvec * pack
    size_t threads;         // what the grid is sized for: nvec, or count when there are no packs
};
FFG_HD StreamPlan stream_plan(size_t count, size_t eb, bool aligned) {
    StreamPlan pl = StreamPlan();
    if (!geom_size_ok(count, eb)) return pl;
    pl.ok = 1;
    pl.pack = geom_pack(eb);
    pl.nvec = stream_nvec(count, eb, aligned);
    pl.tail = pl.nvec * pl.pack;
    pl.threads = pl.nvec ? pl.nvec : count;
    return pl;
}

// ---- reversed rows: one loop over a compact array whose rows are rows of an (n, l) array read backwards ---------------------------
// The source is element-major (n, l); the COMPACT array is (n, l1) with l1 = l, or l1 = l - 1 when the top element of every
// row is left out (skip_top).  Compact element c = h l1 + j takes
//   src = h l + (l1 - 1 - j)    row h read backwards from below its top
//   top = h l + l1              with skip_top the top element of row h (without, one past the row: never read)
// The compact side moves as packs; the reversed reads are element loads -- a pack of compact elements may straddle two rows,
// and its sources run backwards.
struct RevPlan {
    int ok;                 // 0: sizes refused -- nothing may be launched
    int vec;                // whole packs apply
    unsigned pack;          // compact elements of a unit: geom_pack(eb) when vec, else 1
    size_t l, l1;           // length of a source row and of a compact row
    size_t elems;           // n * l1: compact elements
    size_t total;           // units of the flat loop
    int shift;              // log2(l1) when a power of two, else -1
    int narrow;             // every compact index fits 32 bits
};
// (a family's range check of l comes before this call: fxp_norm_plan, explog_rev_plan)
FFG_HD RevPlan rev_plan(size_t n, size_t l, bool skip_top, size_t eb, bool aligned) {
    RevPlan pl = RevPlan();
    size_t nl;
    if (l < 1 || !geom_mul_ok(n, l, nl) || !geom_size_ok(nl, eb)) return pl;
    pl.ok = 1;
    pl.l = l;
    pl.l1 = skip_top ? l - 1 : l;
    pl.elems = n * pl.l1;
    pl.vec = aligned && pl.elems != 0 && pl.elems % geom_gran(eb) == 0;
    pl.pack = pl.vec ? geom_pack(eb) : 1u;
    pl.total = pl.elems / pl.pack;
    pl.shift = geom_pow2(pl.l1) ? geom_log2(pl.l1) : -1;
    pl.narrow = pl.elems <= 0xffffffffu;
    return pl;
}
// what a lane does with compact element c (the kernels call exactly these)
struct RevAt {
    size_t h, j;            // row and position in the compact row: c = h l1 + j
    size_t src, top;        // elements of the source
};
FFG_HD RevAt rev_at(const RevPlan& pl, size_t c) {
    RevAt at;
    at.h = geom_div(c, pl.l1, pl.shift, pl.narrow);
    at.j = c - at.h * pl.l1;
    at.top = at.h * pl.l + pl.l1;
    at.src = at.top - 1 - at.j;
    return at;
}
// compact element c + 1 from compact element c, without a division: the next member of a pack
FFG_HD void rev_next(const RevPlan& pl, RevAt& at) {
    ++at.j;
    --at.src;
    if (at.j == pl.l1) {
        at.j = 0;
        ++at.h;
        at.top += pl.l;
        at.src = at.top - 1;
    }
}

// ---- the pair walk: CxPlan (sort_geom.hpp), TourPlan (tour_geom.hpp) and, through its t, FindPlan (find_geom.hpp) -------------
// A compact array (outer, row_elems) whose rows fall into RUNS; the kernels run one flat loop over outer * row_units units,
// g -> (o, c) = (g / row_units, g % row_units), c -> b = c / run; a shift replaces a division wherever the divisor is a power
// of two.  u: elements of a unit.  The plan type brings the fields row_units, run, total, run_shift, row_shift, narrow.
template <class Plan>
FFG_HD void pair_fill(Plan& pl, size_t outer, size_t row_elems, size_t run_elems, size_t u) {
    pl.row_units = row_elems / u;
    pl.run = run_elems / u;
    pl.total = outer * pl.row_units;
    pl.run_shift = geom_pow2(pl.run) ? geom_log2(pl.run) : -1;
    pl.row_shift = geom_pow2(pl.row_units) ? geom_log2(pl.row_units) : -1;
    pl.narrow = pl.total <= 0xffffffffu && pl.run <= 0xffffffffu;
}
struct PairAt {
    size_t o, c, b;         // row, unit of the compact row, run of the row
};
template <class Plan>
FFG_HD PairAt pair_split(const Plan& pl, size_t g) {
    PairAt at;
    at.o = geom_div(g, pl.row_units, pl.row_shift, pl.narrow);
    at.c = g - at.o * pl.row_units;
    at.b = geom_div(at.c, pl.run, pl.run_shift, pl.narrow);
    return at;
}

}  // namespace ffgpu
