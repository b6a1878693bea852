// rbits_geom.hpp -- index arithmetic and launch plans of the two kernels under secure random bits over a prime field
// (rbits.hpp): the opened masked squares of runtime.np_random_bits (runtime.py:4251-4252) and the bits that follow from
// them (runtime.py:4265-4272).  Plain C++ (no HIP): the kernels, their launcher and the C ABI take every index from here,
// and tests/rbits_check.cpp walks the same functions with g++.
//
// Both kernels are flat over the n entries of a row and read or write up to RBITS_MAX_ROWS separate rows of n entries each
// (one pointer per row, no pitch): entry e of every row is element e of that row's array.  Both take the stream plan of
// geom.hpp (nvec packs of geom_pack(eb) elements through the vector loop -- whole waves for 24-byte elements --, the rest
// through the element tail).  Pack i of the vector loop is elements i * pack .. i * pack + pack - 1 of every row.
//   * the opening: packs for up to rbits_fused_rows(eb) rows (the row count is a template parameter there, as in
//     k_recombine); more rows go by elements throughout (k_recombine_any's loop).
//   * the finish: packs whatever the row count; the rows are walked one after the other behind one exponentiation.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { RBITS_FUSED_ROWS = 9 };              // = MAXK (kernels.hpp): rows of the opening that keep whole packs
enum { RBITS_FUSED_ROWS_24 = 5 };           // ... of 24-byte elements: a row in flight is two raw wave loads of 8 registers
FFG_CX int rbits_fused_rows(size_t eb) { return eb == 24 ? (int)RBITS_FUSED_ROWS_24 : (int)RBITS_FUSED_ROWS; }
enum { RBITS_MAX_ROWS = 64 };               // = MAXK_ANY (kernels.hpp): the row limit of ffgpu_recombine

FFG_HD bool rbits_rows_valid(int rows) { return rows >= 1 && rows <= RBITS_MAX_ROWS; }

// aligned: every row pointer (and the output) admits packs.  The opening is FUSED (the row count a template parameter) for
// k <= rbits_fused_rows(eb); beyond that it has no packs.
FFG_HD StreamPlan rbits_open_plan(size_t n, int k, size_t eb, bool aligned) {
    if (!rbits_rows_valid(k)) return StreamPlan();
    return stream_plan(n, eb, aligned && k <= rbits_fused_rows(eb));
}
FFG_HD StreamPlan rbits_finish_plan(size_t n, int m, size_t eb, bool aligned) {
    if (!rbits_rows_valid(m)) return StreamPlan();
    return stream_plan(n, eb, aligned);
}

// first element of pack i of a row
FFG_HD size_t rbits_pack_at(unsigned pack, size_t i) { return i * pack; }

// entries that `blocks` workgroups take at one pack per thread: a grid capped at that many blocks is saturated from here on
// (every thread owns a pack; one entry more and the loop of thread 0 iterates, or the tail begins)
FFG_HD size_t rbits_grid_entries(size_t blocks, size_t eb) { return blocks * (size_t)GEOM_THREADS * geom_pack(eb); }

}  // namespace ffgpu
