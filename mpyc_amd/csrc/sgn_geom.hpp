// sgn_geom.hpp -- geometry and index arithmetic of the secure-comparison kernels (sgn.hpp).  Plain C++ (no HIP): the
// kernels and their launcher take every index from here, and tests/sgn_check.cpp walks the same functions with g++.
//
// n values of bit length l.  The random bit shares arrive element-major, rbits[h * l + i]; the product tree consumes its
// operands bit-major, e[i * n + h].  A workgroup owns a TILE of SGN_TILE consecutive elements, thread t the element
// h0 + t.  The tile's bit shares are staged through LDS a CHUNK of bit columns at a time:
//   load   the chunk of row r is cols * EW consecutive 4-byte words of global memory (EW = words of an element); the
//          workgroup moves the chunk in UNITS of 4 or 8 bytes, unit q = row q / upr, unit q % upr of that row, consecutive
//          threads at consecutive units: consecutive addresses within a row, rows l elements apart (the whole tile is one
//          contiguous span when the chunk holds all l columns);
//   LDS    row r starts at word r * stride, stride = the words of a full chunk of one row rounded up to the next ODD
//          number: thread t walking column j reads words t * stride + j * EW + w, and 64 consecutive t at an odd
//          word stride fall into 64 different 4-byte banks;
//   walk   thread t walks the columns of its own row with the running values in registers and writes row i of the outputs
//          at i * n + h0 + t: consecutive lanes at consecutive elements.
// The running values are carried across chunks, so LDS per workgroup does not grow with l.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { SGN_TILE = 256 };                    // elements of a workgroup's tile: one per thread
enum { SGN_ROW_WORDS = 32 };                // 4-byte words of payload of an LDS row, at most
enum { SGN_MAX_L = 64 };
// per-wave staging of the 24-byte wave-contiguous accesses (kernels.hpp, x24_region): 4 waves x 96 x 16 bytes
enum { SGN_X24_BYTES = 4 * 96 * 16 };
// bound on the LDS of a workgroup, all element sizes: a quarter of the compute unit's 160 KiB, so LDS admits four
// workgroups (sixteen waves) per compute unit; sgn.hpp holds the kernels' registers to the same four waves per SIMD
enum { SGN_LDS_BOUND = 40 * 1024 };

FFG_CX int sgn_elem_words(size_t eb) { return (int)(eb / 4); }                          // 1, 2, 3, 4, 6
// bit columns of a chunk: 32, 16, 10, 8, 5
FFG_CX int sgn_chunk(size_t eb) { return SGN_ROW_WORDS / sgn_elem_words(eb); }
// words between two LDS rows: odd (33, 33, 31, 33, 31)
FFG_CX int sgn_stride(size_t eb) { return (sgn_chunk(eb) * sgn_elem_words(eb)) | 1; }
// words of a load unit: 8-byte units where an element is a whole number of them (its rows then start 8-byte aligned)
FFG_CX int sgn_unit_words(size_t eb) { return sgn_elem_words(eb) % 2 == 0 ? 2 : 1; }
FFG_CX size_t sgn_lds_words(size_t eb) { return (size_t)SGN_TILE * (size_t)sgn_stride(eb); }
FFG_CX size_t sgn_lds_bytes(size_t eb) { return sgn_lds_words(eb) * 4 + (eb == 24 ? (size_t)SGN_X24_BYTES : 0); }

struct SgnPlan {
    int ok;             // 0: l out of range, sizes overflow or more tiles than a grid holds -- nothing may be launched
    size_t tiles;       // workgroups
    size_t nl;          // n * l: elements of rbits, of nx; e has nl + n
};
FFG_HD SgnPlan sgn_plan(size_t n, int l, size_t eb) {
    SgnPlan p = SgnPlan();
    size_t ne;
    if (l < 1 || l > SGN_MAX_L) return p;
    if (!geom_mul_ok(n, (size_t)l + 1, ne) || !geom_size_ok(ne, eb)) return p;
    p.nl = n * (size_t)l;
    p.tiles = (n + SGN_TILE - 1) / SGN_TILE;
    if (p.tiles > (size_t)GEOM_MAX_GRID) return p;
    p.ok = 1;
    return p;
}

// ---- tiles and chunks ----------------------------------------------------------------------------------------------------
FFG_HD size_t sgn_tile_base(size_t tile) { return tile * (size_t)SGN_TILE; }
// live rows of the tile that starts at h0
FFG_HD unsigned sgn_tile_rows(size_t n, size_t h0) { return n - h0 < (size_t)SGN_TILE ? (unsigned)(n - h0) : (unsigned)SGN_TILE; }
// columns of the chunk that starts at bit column i0
FFG_HD int sgn_chunk_cols(int l, int i0, size_t eb) { return l - i0 < sgn_chunk(eb) ? l - i0 : sgn_chunk(eb); }
// load units of one row of a chunk of `cols` columns
FFG_HD unsigned sgn_units_per_row(int cols, size_t eb) { return (unsigned)(cols * sgn_elem_words(eb) / sgn_unit_words(eb)); }

// ---- load: the units a thread moves, in order ------------------------------------------------------------------------------
// thread tid takes units tid, tid + GEOM_THREADS, ...; the cursor keeps (row, unit of the row) without a division per step
struct SgnCursor {
    unsigned row, u, drow, du, upr;
};
FFG_HD SgnCursor sgn_cursor(unsigned tid, unsigned upr) {
    SgnCursor c;
    c.upr = upr;
    c.row = tid / upr;
    c.u = tid % upr;
    c.drow = (unsigned)GEOM_THREADS / upr;
    c.du = (unsigned)GEOM_THREADS % upr;
    return c;
}
FFG_HD void sgn_cursor_next(SgnCursor& c) {
    c.row += c.drow;
    c.u += c.du;
    if (c.u >= c.upr) {
        c.u -= c.upr;
        ++c.row;
    }
}
// 4-byte word of rbits (from its first byte) where the unit starts: element (h0 + row) * l + i0, plus the unit's offset
FFG_HD size_t sgn_unit_src_word(size_t h0, unsigned row, int l, int i0, unsigned u, size_t eb) {
    return ((h0 + row) * (size_t)l + (size_t)i0) * (size_t)sgn_elem_words(eb) + (size_t)u * (size_t)sgn_unit_words(eb);
}
// LDS word where the unit goes
FFG_HD unsigned sgn_unit_lds_word(unsigned row, unsigned u, size_t eb) {
    return row * (unsigned)sgn_stride(eb) + u * (unsigned)sgn_unit_words(eb);
}

// ---- walk ------------------------------------------------------------------------------------------------------------------
// first LDS word of column j of the chunk in row t
FFG_HD unsigned sgn_walk_lds_word(unsigned t, int j, size_t eb) {
    return t * (unsigned)sgn_stride(eb) + (unsigned)j * (unsigned)sgn_elem_words(eb);
}
// element of a bit-major (rows, n) output: row i (i <= l), element h
FFG_HD size_t sgn_out_index(int i, size_t n, size_t h) { return (size_t)i * n + h; }

}  // namespace ffgpu
