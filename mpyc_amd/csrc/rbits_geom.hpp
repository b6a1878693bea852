// rbits_geom.hpp -- index arithmetic and launch plans of the two kernels under secure random bits over a prime field
// (rbits.hpp): the opened masked squares of runtime.np_random_bits (runtime.py:4251-4252) and the bits that follow from
// them (runtime.py:4265-4272).  Plain C++ (no HIP): the kernels, their launcher and the C ABI take every index from here,
// and tests/rbits_check.cpp walks the same functions with g++.
//
// Both kernels are flat over the n entries of a row and read or write up to RBITS_MAX_ROWS separate rows of n entries each
// (one pointer per row, no pitch): entry e of every row is element e of that row's array.  Both take the streaming plan of
// the exponentiation (legendre_plan, iszero_geom.hpp: nvec packs of cx_pack(eb) elements through the vector loop -- whole
// waves for 24-byte elements --, the rest through the element tail).  Pack i of the vector loop is elements
// i * pack .. i * pack + pack - 1 of every row.
//   * the opening: packs for up to rbits_fused_rows(eb) rows (the row count is a template parameter there, as in
//     k_recombine); more rows go by elements throughout (k_recombine_any's loop).
//   * the finish: packs whatever the row count; the rows are walked one after the other behind one exponentiation.
#pragma once
#include "iszero_geom.hpp"

namespace ffgpu {

enum { RBITS_FUSED_ROWS = 9 };              // = MAXK (kernels.hpp): rows of the opening that keep whole packs
enum { RBITS_FUSED_ROWS_24 = 5 };           // ... of 24-byte elements: a row in flight is two raw wave loads of 8 registers
FFCX_CX int rbits_fused_rows(size_t eb) { return eb == 24 ? (int)RBITS_FUSED_ROWS_24 : (int)RBITS_FUSED_ROWS; }
enum { RBITS_MAX_ROWS = 64 };               // = MAXK_ANY (kernels.hpp): the row limit of ffgpu_recombine

FFCX_HD bool rbits_rows_valid(int rows) { return rows >= 1 && rows <= RBITS_MAX_ROWS; }

struct RbitsPlan {
    int ok;                 // 0: the row count or the sizes are refused -- nothing may be launched
    int fused;              // the opening: the row count is a template parameter (rows <= rbits_fused_rows(eb))
    unsigned pack;          // elements of a pack: cx_pack(eb)
    size_t nvec;            // packs through the vector loop (whole waves for 24-byte elements); 0: elements throughout
    size_t tail;            // first entry of the element tail: nvec * pack
    size_t threads;         // what the grid is sized for: nvec, or n when there are no packs
};
FFCX_HD RbitsPlan rbits_plan_(size_t n, int rows, size_t eb, bool packs) {
    RbitsPlan pl = RbitsPlan();
    if (!rbits_rows_valid(rows)) return pl;
    const LegendrePlan lp = legendre_plan(n, eb, packs);
    if (!lp.ok) return pl;
    pl.ok = 1;
    pl.fused = rows <= rbits_fused_rows(eb);
    pl.pack = lp.pack;
    pl.nvec = lp.nvec;
    pl.tail = lp.tail;
    pl.threads = lp.threads;
    return pl;
}
// aligned: every row pointer (and the output) admits packs
FFCX_HD RbitsPlan rbits_open_plan(size_t n, int k, size_t eb, bool aligned) {
    return rbits_plan_(n, k, eb, aligned && k <= rbits_fused_rows(eb));
}
FFCX_HD RbitsPlan rbits_finish_plan(size_t n, int m, size_t eb, bool aligned) { return rbits_plan_(n, m, eb, aligned); }

// first element of pack i of a row
FFCX_HD size_t rbits_pack_at(unsigned pack, size_t i) { return i * pack; }

// entries that `blocks` workgroups take at one pack per thread: a grid capped at that many blocks is saturated from here on
// (every thread owns a pack; one entry more and the loop of thread 0 iterates, or the tail begins)
FFCX_HD size_t rbits_grid_entries(size_t blocks, size_t eb) { return blocks * (size_t)CX_THREADS * cx_pack(eb); }

}  // namespace ffgpu
