// bsgn_geom.hpp -- index arithmetic and launch plans of the two kernels under the secure binary sign by Legendre symbols
// (bsgn.hpp): the masked values (2a + 1 + 2j) z_j that are opened and the shares h s of the symbols that follow from them.
// Plain C++ (no HIP): the kernels, their launcher and the C ABI take every index from here, and tests/bsgn_check.cpp walks
// the same functions with g++.
//
// The arrays are ROW-MAJOR (w, n), 1 <= w <= BSGN_MAX_ROWS: row i holds the i-th symbol's entry of the n elements, rows n
// elements apart -- the layout prod_rows consumes.
//   * the mask is flat over the n elements of a row: a thread owns a unit of `a` and the same unit of every row, which is the
//     mask of the zero test as it is (iszero_mask_plan: the rows plan of geom.hpp with stride n);
//   * the finish in rows mode is flat over count = w n entries with the stream plan of geom.hpp (nvec packs through the vector
//     loop, the rest through the element tail), every party's row of shares walked behind one exponentiation;
//   * the finish in sum mode is flat over the n elements of a row as the mask is: a thread forms the w symbols of its unit,
//     keeps them as 2-bit codes (LEGENDRE_*, iszero_geom.hpp) in one 64-bit word and walks the parties.
#pragma once
#include "iszero_geom.hpp"

namespace ffgpu {

enum { BSGN_MAX_ROWS = 8 };                 // symbols per element: the demo takes 1, 3 or 5
enum { BSGN_MAX_PARTIES = 64 };             // rows of shares behind one exponentiation (= MAXK_ANY, kernels.hpp)

FFG_HD bool bsgn_w_valid(int w) { return w >= 1 && w <= BSGN_MAX_ROWS; }
FFG_HD bool bsgn_m_valid(int m) { return m >= 1 && m <= BSGN_MAX_PARTIES; }

// ---- mask, and the finish in sum mode: one flat loop over the n elements of a row; pl.span == w * n --------------------------
FFG_HD RowsPlan bsgn_rows_plan(size_t n, int w, size_t eb, bool aligned) {
    if (!bsgn_w_valid(w)) return RowsPlan();
    return iszero_mask_plan(n, w, eb, aligned);
}
// unit g of row i is rows_unit(pl, i, g); unit g of `a` (of a sum-mode output) is g itself

// ---- the finish in rows mode: the stream plan over count = w * n entries ----------------------------------------------------
FFG_HD StreamPlan bsgn_flat_plan(size_t n, int w, size_t eb, bool aligned) {
    size_t count;
    if (!bsgn_w_valid(w) || !geom_mul_ok(n, (size_t)w, count)) return StreamPlan();
    return stream_plan(count, eb, aligned);
}

// ---- the symbols of a unit in sum mode: code (LEGENDRE_*) of row i, element q of the pack, two bits each ----------------------
static_assert(BSGN_MAX_ROWS * 4 * 2 <= 64, "the codes of a unit fit one 64-bit word (a pack holds four elements at the most)");
FFG_HD unsigned bsgn_sym_shift(int i, int q) { return 2u * (unsigned)(4 * i + q); }
FFG_HD uint64_t bsgn_sym_put(uint64_t codes, int i, int q, unsigned code) { return codes | ((uint64_t)(code & 3u) << bsgn_sym_shift(i, q)); }
FFG_HD unsigned bsgn_sym_of(uint64_t codes, int i, int q) { return (unsigned)(codes >> bsgn_sym_shift(i, q)) & 3u; }

}  // namespace ffgpu
