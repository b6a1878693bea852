// iszero_geom.hpp -- index arithmetic and launch plans of the kernels under the probabilistic zero test over a Blum prime
// (iszero.hpp): the mask of runtime._np_is_zero (runtime.py:3608), the Legendre symbols of the opened values
// (finfields.py:1464-1470) and the selection that follows them (runtime.py:3614-3615).  Plain C++ (no HIP): the kernels, their
// launcher and the C ABI take every index from here, and tests/iszero_check.cpp walks the same functions with g++.
//
// The masked copies are ROW-MAJOR (k, n): row i holds the i-th copy of the n elements, rows n elements apart -- the layout
// prod_rows consumes.  The mask is flat over the n elements of a row: a thread owns a unit of `a` and the same unit of every
// row, which is the rows plan of geom.hpp with stride n.  Unit g of row i is unit  rows_unit(pl, i, g)  of the (k, n) arrays
// and unit g of `a`.
//
// The symbols and the finish are flat over count = k n entries with one code BYTE per entry: the codes of a unit of `pack`
// elements are the `pack` consecutive bytes from  g * pack  on, moved as one 1-, 2- or 4-byte access -- so whole packs also
// need the byte array aligned to `pack` bytes.  The symbols take the stream plan of the exponentiation (stream_plan: nvec packs
// through the vector loop, the rest through the element tail); the finish has no tail: flat_plan, packs or elements throughout.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { LEGENDRE_NONRESIDUE = 0, LEGENDRE_RESIDUE = 1, LEGENDRE_ZERO = 2 };

FFG_HD bool iszero_k_valid(int k) { return k >= 1; }

// ---- mask: one flat loop over the n elements of a row; pl.span == k * n, the entries of every (k, n) array -----------------
FFG_HD RowsPlan iszero_mask_plan(size_t n, int k, size_t eb, bool aligned) {
    if (!iszero_k_valid(k)) return RowsPlan();
    return rows_plan(n, (size_t)k, n, eb, aligned);
}

// ---- the code bytes of a unit ------------------------------------------------------------------------------------------------
// is a byte array at address `addr` aligned for the one access that moves a pack's codes?
FFG_HD bool iszero_codes_aligned(uintptr_t addr, size_t eb) { return addr % geom_pack(eb) == 0; }
// the first code byte of unit g of `pack` elements
FFG_HD size_t iszero_code_at(unsigned pack, size_t g) { return g * pack; }
// byte q of the word that holds a pack's codes
FFG_HD unsigned iszero_code_of(uint32_t codes, int q) { return (codes >> (8 * q)) & 0xffu; }
FFG_HD uint32_t iszero_code_put(uint32_t codes, int q, unsigned code) { return codes | ((uint32_t)code << (8 * q)); }

}  // namespace ffgpu
