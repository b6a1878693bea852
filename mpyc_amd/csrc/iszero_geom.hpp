// iszero_geom.hpp -- index arithmetic and launch plans of the kernels under the probabilistic zero test over a Blum prime
// (iszero.hpp): the mask of runtime._np_is_zero (runtime.py:3608), the Legendre symbols of the opened values
// (finfields.py:1464-1470) and the selection that follows them (runtime.py:3614-3615).  Plain C++ (no HIP): the kernels, their
// launcher and the C ABI take every index from here, and tests/iszero_check.cpp walks the same functions with g++.
//
// The masked copies are ROW-MAJOR (k, n): row i holds the i-th copy of the n elements, rows n elements apart -- the layout
// prod_rows consumes.  The mask is flat over the n elements of a row: a thread owns a unit of `a` and the same unit of every
// row, which is the row plan of a power-major block with stride n (explog_geom.hpp) as it is: a pack of cx_pack(eb)
// consecutive elements where whole packs apply (sort_geom.hpp: pointers and row pitch aligned, n a whole number of
// cx_gran(eb) elements -- whole waves for 24-byte elements), a single element otherwise.  Unit g of row i is unit
// i * pitch + g  of the (k, n) arrays and unit g of `a`.
//
// The symbols and the finish are flat over count = k n entries with one code BYTE per entry: the codes of a unit of `pack`
// elements are the `pack` consecutive bytes from  g * pack  on, moved as one 1-, 2- or 4-byte access -- so whole packs also
// need the byte array aligned to `pack` bytes.  The symbols take the streaming plan of the exponentiation (nvec packs through
// the vector loop, the rest through the element tail); the finish has no tail: packs or elements throughout.
#pragma once
#include "explog_geom.hpp"

namespace ffgpu {

enum { LEGENDRE_NONRESIDUE = 0, LEGENDRE_RESIDUE = 1, LEGENDRE_ZERO = 2 };

FFCX_HD bool iszero_k_valid(int k) { return k >= 1; }

// ---- mask: one flat loop over the n elements of a row; pl.span == k * n, the entries of every (k, n) array -----------------
FFCX_HD ExplogRowsPlan iszero_mask_plan(size_t n, int k, size_t eb, bool aligned) {
    if (!iszero_k_valid(k)) return ExplogRowsPlan();
    return explog_rows_plan(n, (size_t)k, n, eb, aligned);
}
// unit g of row i, in units of a (k, n) array; unit g of `a` is g itself
FFCX_HD size_t iszero_mask_unit(const ExplogRowsPlan& pl, size_t i, size_t g) { return explog_row_unit(pl, i, g); }

// ---- the code bytes of a unit ------------------------------------------------------------------------------------------------
// is a byte array at address `addr` aligned for the one access that moves a pack's codes?
FFCX_HD bool iszero_codes_aligned(uintptr_t addr, size_t eb) { return addr % cx_pack(eb) == 0; }
// the first code byte of unit g of `pack` elements
FFCX_HD size_t iszero_code_at(unsigned pack, size_t g) { return g * pack; }
// byte q of the word that holds a pack's codes
FFCX_HD unsigned iszero_code_of(uint32_t codes, int q) { return (codes >> (8 * q)) & 0xffu; }
FFCX_HD uint32_t iszero_code_put(uint32_t codes, int q, unsigned code) { return codes | ((uint32_t)code << (8 * q)); }

// ---- symbols: the plan of the exponentiation -- packs of the vector loop, then an element tail -------------------------------
struct LegendrePlan {
    int ok;                 // 0: sizes overflow -- nothing may be launched
    unsigned pack;          // elements of a pack: cx_pack(eb)
    size_t nvec;            // packs through the vector loop (whole waves for 24-byte elements); 0: elements throughout
    size_t tail;            // first entry of the element tail: nvec * pack
    size_t threads;         // what the grid is sized for: nvec, or count when there are no packs
};
FFCX_HD LegendrePlan legendre_plan(size_t count, size_t eb, bool aligned) {
    LegendrePlan pl = LegendrePlan();
    size_t bytes;
    if (eb < 4 || eb % 4) return pl;
    if (!cx_mul_ok(count, eb, bytes) || bytes > ((size_t)1 << 62)) return pl;
    pl.ok = 1;
    pl.pack = cx_pack(eb);
    pl.nvec = !aligned ? 0 : eb == 24 ? (count & ~(size_t)63) : count / pl.pack;
    pl.tail = pl.nvec * pl.pack;
    pl.threads = pl.nvec ? pl.nvec : count;
    return pl;
}

// ---- finish: one flat loop over count, packs or elements throughout -----------------------------------------------------------
struct IszeroFlatPlan {
    int ok;                 // 0: sizes overflow -- nothing may be launched
    int vec;                // whole packs apply
    unsigned pack;          // elements of a unit: cx_pack(eb) when vec, else 1
    size_t total;           // units of the flat loop
};
FFCX_HD IszeroFlatPlan iszero_flat_plan(size_t count, size_t eb, bool aligned) {
    IszeroFlatPlan pl = IszeroFlatPlan();
    const FxpFlatPlan fp = fxp_flat_plan(count, eb, aligned);
    if (!fp.ok) return pl;
    pl.ok = 1;
    pl.vec = fp.vec;
    pl.pack = fp.vec ? cx_pack(eb) : 1u;
    pl.total = fp.total;
    return pl;
}

}  // namespace ffgpu
