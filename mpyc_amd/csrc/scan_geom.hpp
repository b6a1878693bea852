// scan_geom.hpp -- geometry and index arithmetic of the prefix-scan / axis-reduction kernels (scan.hpp).  Plain C++ (no
// HIP): the kernels, their launcher and ffgpu_scan_workspace_bytes take every index from here, and tests/scan_check.cpp
// walks the same functions with g++.
//
// An array is contiguous row-major (outer, k, inner): element (o, j, i) at (o k + j) inner + i, scanned or reduced along
// j.  A LINE is one (o, i): k elements, `inner` elements apart; there are outer * inner lines.  Two geometries:
//   columns  a thread owns one line, or -- when inner is a multiple of the 16-byte pack and the pointers are aligned -- one
//            pack of consecutive i at one o, and walks j = 0 .. k-1 with the running value in registers.  Neighbouring
//            threads are neighbouring i: every step of a wave is one coalesced access.  One launch, no workspace.
//   rows     a workgroup owns a TILE of T = threads * ITEMS consecutive j of one line; thread t holds the ITEMS
//            elements j0 + t ITEMS .. of it.  A line of one tile is scanned in one launch.  A line of several tiles is
//            reduce-then-scan: (A) every tile writes its aggregate to workspace[line * ntiles + tile], (B) one workgroup
//            per line scans that line's aggregates exclusively, in place, chunk after chunk in order, (C) every tile is
//            read again and scanned with its carry-in.  No workgroup waits for another inside a launch.  A reduction is
//            (A) and then one workgroup per line folding the aggregates.  With inner > 1 the tile's elements are `inner`
//            apart in memory (strided, uncoalesced: the geometry of few long lines only).
// The launcher chooses by line count, line length and stride (scan_choose).
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { SCAN_THREADS = 256 };                    // = BLOCK (kernels.hpp)
enum { SCAN_COLS = 1, SCAN_ROWS = 2 };
enum { SCAN_MAX_GRID = 0x7fffffff };

// elements a thread of the row geometry holds (by element size in bytes: the arithmetic word is 4 or 8 bytes up to 8-byte
// elements, 16 or 24 bytes above)
FFG_HD int scan_items(size_t eb) { return eb <= 8 ? 16 : 8; }
// elements of one 16-byte pack (one lane's access) in the column geometry; 12-, 16- and 24-byte elements go one per lane
FFG_HD int scan_epv(size_t eb) { return eb <= 8 ? (int)(16 / eb) : 1; }

struct ScanPlan {
    int ok;             // 0: sizes overflow or the grid would be too large -- nothing may be launched
    int geom;           // SCAN_COLS / SCAN_ROWS
    size_t lines;       // outer * inner
    // columns
    size_t per;         // threads per o: inner / EPV (packs) or inner (single elements)
    size_t units;       // outer * per: threads that own a column
    int vec;            // packs
    // rows
    int tt;             // threads of a workgroup that hold elements (the rest idle): the tile-size switch
    size_t tile;        // T = tt * ITEMS
    size_t ntiles;      // tiles per line
    size_t ws_elems;    // workspace elements: lines * ntiles when ntiles > 1
};

// geom_cfg: 0 = choose, SCAN_COLS / SCAN_ROWS = forced.  tile_threads: 1 .. SCAN_THREADS.
// Strided lines (inner > 1): columns when they give every compute unit a workgroup's worth of threads, and also when a line
// is shorter than a tile -- a workgroup per strided line would then idle most of its threads and read uncoalesced, which
// measured nine times slower than even a thin column walk ((64, 65536) bytes of GF(2^8), profiles/r09_scan.md); row tiles
// only for few long strided lines.  Contiguous lines (inner == 1): row tiles, except many short lines (a quarter tile at
// most), which take one thread per line.
FFG_HD int scan_choose(size_t units, size_t k, size_t inner, size_t tile, int num_cu, int geom_cfg) {
    if (geom_cfg == SCAN_COLS || geom_cfg == SCAN_ROWS) return geom_cfg;
    const bool fills = units >= (size_t)num_cu * 64;
    if (inner > 1) return fills || k < tile ? SCAN_COLS : SCAN_ROWS;
    return fills && k * 4 <= tile ? SCAN_COLS : SCAN_ROWS;
}

// aligned: every pointer of the call is 16-byte aligned (4-byte for 12-byte elements).  with_initial counts for the
// output size check only.
FFG_HD ScanPlan scan_plan(size_t outer, size_t k, size_t inner, size_t eb, bool aligned, int num_cu, int geom_cfg,
                             int tile_threads, int with_initial = 0) {
    ScanPlan p = ScanPlan();
    size_t n, nout;
    if (k == 0 || outer == 0 || inner == 0 || eb == 0) return p;
    if (!geom_mul_ok(outer, inner, p.lines) || !geom_mul_ok(p.lines, k, n)) return p;
    if (k + 1 == 0 || !geom_mul_ok(p.lines, k + (with_initial ? 1 : 0), nout) || !geom_bytes_ok(nout, eb)) return p;
    const int epv = scan_epv(eb);
    p.vec = aligned && inner % (size_t)epv == 0;
    p.per = p.vec ? inner / (size_t)epv : inner;
    p.units = outer * p.per;
    p.tt = tile_threads < 1 ? 1 : tile_threads > SCAN_THREADS ? (int)SCAN_THREADS : tile_threads;
    p.tile = (size_t)p.tt * (size_t)scan_items(eb);
    p.ntiles = (k + p.tile - 1) / p.tile;
    p.geom = scan_choose(p.units, k, inner, p.tile, num_cu, geom_cfg);
    size_t blocks;
    if (p.geom == SCAN_ROWS) {
        if (!geom_mul_ok(p.lines, p.ntiles, blocks) || blocks > (size_t)SCAN_MAX_GRID) return p;
        p.ws_elems = p.ntiles > 1 ? blocks : 0;
    } else {
        if ((p.units + SCAN_THREADS - 1) / SCAN_THREADS > (size_t)SCAN_MAX_GRID) return p;
        p.ws_elems = 0;
    }
    p.ok = 1;
    return p;
}

// ---- columns -----------------------------------------------------------------------------------------------------------
// thread `u` of p.units: its o and its column c (pack or element) within o
FFG_HD void scan_col_of(size_t u, size_t per, size_t& o, size_t& c) {
    o = u / per;
    c = u % per;
}
// index (in packs or elements, whichever `per` counts) of step j of that column in an array with kk entries along the axis
FFG_HD size_t scan_col_index(size_t o, size_t c, size_t j, size_t kk, size_t per) { return (o * kk + j) * per + c; }

// ---- rows --------------------------------------------------------------------------------------------------------------
// workgroup b: its line and its tile
FFG_HD void scan_tile_of(size_t b, size_t ntiles, size_t& line, size_t& t) {
    line = b / ntiles;
    t = b % ntiles;
}
// first element (j = 0) of a line in an array with kk entries along the axis
FFG_HD size_t scan_line_base(size_t line, size_t kk, size_t inner) { return (line / inner) * kk * inner + line % inner; }
// axis position of item q of thread `tid` in tile t (valid when tid < tt and the result is < k)
FFG_HD size_t scan_item_j(size_t t, size_t tile, int tid, int items, int q) {
    return t * tile + (size_t)tid * (size_t)items + (size_t)q;
}
// workspace slot of a tile's aggregate / carry-in
FFG_HD size_t scan_ws_index(size_t line, size_t t, size_t ntiles) { return line * ntiles + t; }

}  // namespace ffgpu
