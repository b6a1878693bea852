// conv2d_geom.hpp -- tile / window / tap index arithmetic, flush schedule, LDS bytes and launch plan of k_conv2d
// (conv2d.hpp).  Plain C++ (no HIP): the kernel and its launcher take every index from here, and tests/conv2d_check.cpp
// walks the same functions with g++ against the plain seven-deep loop.
//
// Y[i, j, I, J] = b[j] + sum_{l<r} sum_{di<s} sum_{dj<s} x[i, l, I + di - (s-1)/2, J + dj - s/2] W[j, l, di, dj], terms
// whose x index falls outside [0, m) x [0, n) are 0 (the demo's convolvetensor, np_cnnmnist.py:69-80: the row offset is
// its s2, the column offset what np.correlate(mode='same') takes).  x: (k, r, m, n), W: (v, r, s, s), Y: (k, v, m, n),
// row-major, 1 <= s <= 16.
//
// Output-stationary: a workgroup owns one image, one tile of TH x TW output pixels and one block of VB output channels.
// Its BLOCK threads are G channel groups of PL = TH TW pixel lanes; a lane owns pixel (py, px) of the tile for the VR
// channels g VR .. g VR + VR - 1 of the block, so that every output has exactly one owner (workgroup, thread, register)
// and no partial sums leave the thread.  Two shapes:
//   wide    16 x 16 pixels, G = 1, VR = 4 (VB = 4): one window element feeds four accumulators;
//   narrow   8 x 16 pixels, G = 2, VR = 1 (VB = 2): four times the workgroups for the same tensors, each with a quarter of
//           the products per thread -- the launcher takes it while the wide tiles would not fill the chip (a 14 x 14
//           image is ONE wide tile: 16 workgroups per sender for 64 output channels, 64 narrow ones).
// The workgroup walks the input channels in steps of CH.  Per step it stages in LDS, per channel, the zero-padded window
// (TH + s - 1) x (TW + s - 1) -- window slot (wy, wx) holds x[I0 + wy - (s-1)/2, J0 + wx - s/2], zero outside the image
// -- and the s x s taps of that channel for the VB output channels of the block, zero for channels from v up.  The lanes
// of a wave read ONE tap per step (the same address: a broadcast) and consecutive window elements of a row.
//
// Flush schedule: an accumulator takes s terms per filter row and holds `flush` of them, so it is reduced after every
// flush / s filter rows, counted on across the input channels: inside a channel once s^2 > flush (s >= 6 at 32 terms).
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum {
    CONV2D_MAX_S = 16,              // the flush test follows whole filter rows: a row must fit an accumulator twice over
    CONV2D_MAX_SENDERS = 64,        // the senders of one launch (the limit of ffgpu_recombine)
    CONV2D_MAX_CH = 8,              // input channels per staging step at the most
    CONV2D_LDS_STEP = 32768,        // LDS bytes a staging step of more than one channel may take: four workgroups per CU
    CONV2D_LDS_LIMIT = 65536,       // LDS bytes of a workgroup at the most
    CONV2D_MAX_GRID = 0x7fffffff    // HIP's limit for gridDim.x
};

template <int TH_, int TW_, int VR_>
struct Conv2dShape {
    enum {
        THREADS = 256,              // = BLOCK (kernels.hpp)
        TH = TH_, TW = TW_,         // output pixels of a tile
        PL = TH * TW,               // pixel lanes of a channel group
        G = THREADS / PL,           // channel groups
        VR = VR_,                   // output channels a lane keeps in registers
        VB = G * VR                 // output channels of a workgroup
    };
    static_assert(PL * G == THREADS && PL % 64 == 0, "a channel group is whole waves");
};
typedef Conv2dShape<16, 16, 4> Conv2dWide;
typedef Conv2dShape<8, 16, 1> Conv2dNarrow;

FFG_HD int conv2d_row_off(int s) { return (s - 1) / 2; }
FFG_HD int conv2d_col_off(int s) { return s / 2; }

// filter rows between two reductions of an accumulator that holds `flush` terms: at least 2 for s <= CONV2D_MAX_S
FFG_HD int conv2d_flush_rows(int s, int flush) { return flush / s; }

// the launch: everything the kernel needs beside the pointers.  Filled by conv2d_plan().
struct Conv2dGeom {
    size_t r, m, n, v;              // input channels, rows, columns, output channels
    int s, WH, WW;                  // filter size; window rows and columns: TH + s - 1, TW + s - 1
    int CH;                         // input channels per staging step
    int TH, TW, VB, VR;             // the shape taken
    unsigned tiles_y, tiles_x, vblocks;   // tiles and channel blocks of one image
};

struct Conv2dPlan {
    bool ok;                        // the sizes are valid (conv2d_plan states what that means)
    bool grid_ok;                   // the grid is within HIP's limits
    bool empty;                     // k v m n == 0: nothing to do
    int wide;                       // 1: the wide shape
    int flush_rows;                 // conv2d_flush_rows(s, flush)
    uint64_t grid_x;                // k tiles_y tiles_x vblocks
    unsigned grid_y;                // the senders
    size_t lds_bytes;
    Conv2dGeom g;
};

// elements of the three tensors; false when one of them, times elem_bytes, overflows size_t (or passes 2^62)
FFG_HD bool conv2d_sizes(size_t k, size_t r, size_t m, size_t n, size_t v, int s, size_t elem_bytes, size_t* nx, size_t* nw,
                           size_t* ny) {
    size_t t;
    if (!geom_mul_ok(k, r, t) || !geom_mul_ok(t, m, t) || !geom_mul_ok(t, n, *nx)) return false;
    if (!geom_mul_ok(v, r, t) || !geom_mul_ok(t, (size_t)s * (size_t)s, *nw)) return false;
    if (!geom_mul_ok(k, v, t) || !geom_mul_ok(t, m, t) || !geom_mul_ok(t, n, *ny)) return false;
    return geom_bytes_ok(*nx, elem_bytes) && geom_bytes_ok(*nw, elem_bytes) && geom_bytes_ok(*ny, elem_bytes);
}

// window and tap slots of one input channel
FFG_HD int conv2d_win_slots(int TH, int TW, int s) { return (TH + s - 1) * (TW + s - 1); }
FFG_HD int conv2d_tap_slots(int VB, int s) { return VB * s * s; }
// LDS bytes of a staging step of CH channels; slot_bytes: a staged operand (a word, or its 28-bit digits)
FFG_HD size_t conv2d_lds_bytes(int TH, int TW, int VB, int s, int CH, size_t slot_bytes) {
    return (size_t)CH * (size_t)(conv2d_win_slots(TH, TW, s) + conv2d_tap_slots(VB, s)) * slot_bytes;
}
// input channels per step: as many as CONV2D_LDS_STEP holds, at most CONV2D_MAX_CH and r, at least one
FFG_HD int conv2d_channels_per_step(int TH, int TW, int VB, int s, size_t r, size_t slot_bytes) {
    const size_t one = conv2d_lds_bytes(TH, TW, VB, s, 1, slot_bytes);
    size_t ch = (size_t)CONV2D_LDS_STEP / one;
    if (ch > (size_t)CONV2D_MAX_CH) ch = CONV2D_MAX_CH;
    if (ch > r) ch = r;
    return ch < 1 ? 1 : (int)ch;
}

FFG_HD size_t conv2d_ceil_div(size_t a, size_t b) { return a / b + (a % b != 0); }

// workgroups of a shape for the whole call; false on overflow
FFG_HD bool conv2d_blocks(size_t k, size_t m, size_t n, size_t v, int TH, int TW, int VB, size_t* blocks) {
    size_t t, all;
    if (!geom_mul_ok(k, conv2d_ceil_div(m, (size_t)TH), t) || !geom_mul_ok(t, conv2d_ceil_div(n, (size_t)TW), t) ||
        !geom_mul_ok(t, conv2d_ceil_div(v, (size_t)VB), all))
        return false;
    *blocks = all;                  // (untouched on overflow)
    return true;
}

// the wide shape once its workgroups, over all senders, give every compute unit `per_cu` of them, the narrow one below
FFG_HD bool conv2d_use_wide(size_t wide_blocks, int nsend, int num_cu, int per_cu) {
    size_t all;
    if (!geom_mul_ok(wide_blocks, (size_t)nsend, all)) return true;
    return all >= (size_t)(num_cu > 0 ? num_cu : 1) * (size_t)per_cu;
}

// The launch plan.  ok: 1 <= s <= CONV2D_MAX_S, s <= n, nsend >= 1, no size overflowing, and r, m, n, v >= 1 unless
// k v m n == 0 (empty: nothing is launched).  slot_bytes, flush: of the field policy (conv2d.hpp).
FFG_HD Conv2dPlan conv2d_plan(size_t k, size_t r, size_t m, size_t n, size_t v, int s, int nsend, int num_cu, int wide_per_cu,
                                size_t elem_bytes, size_t slot_bytes, int flush) {
    Conv2dPlan p = Conv2dPlan();
    size_t nx, nw, ny;
    if (s < 1 || s > (int)CONV2D_MAX_S || nsend < 1 || !conv2d_sizes(k, r, m, n, v, s, elem_bytes, &nx, &nw, &ny)) return p;
    p.empty = ny == 0;
    if ((size_t)s > n && !(p.empty && n == 0)) return p;
    if (!p.empty && r < 1) return p;
    p.ok = true;
    p.flush_rows = conv2d_flush_rows(s, flush);
    p.grid_y = (unsigned)nsend;
    size_t wb = 0;
    const bool wide = p.empty || !conv2d_blocks(k, m, n, v, Conv2dWide::TH, Conv2dWide::TW, Conv2dWide::VB, &wb) ||
                      conv2d_use_wide(wb, nsend, num_cu, wide_per_cu);
    p.wide = wide ? 1 : 0;
    Conv2dGeom& g = p.g;
    g.r = r; g.m = m; g.n = n; g.v = v; g.s = s;
    g.TH = wide ? (int)Conv2dWide::TH : (int)Conv2dNarrow::TH;
    g.TW = wide ? (int)Conv2dWide::TW : (int)Conv2dNarrow::TW;
    g.VB = wide ? (int)Conv2dWide::VB : (int)Conv2dNarrow::VB;
    g.VR = wide ? (int)Conv2dWide::VR : (int)Conv2dNarrow::VR;
    g.WH = g.TH + s - 1;
    g.WW = g.TW + s - 1;
    g.CH = conv2d_channels_per_step(g.TH, g.TW, g.VB, s, r, slot_bytes);
    p.lds_bytes = conv2d_lds_bytes(g.TH, g.TW, g.VB, s, g.CH, slot_bytes);
    size_t blocks = 0;
    const size_t ty = conv2d_ceil_div(m, (size_t)g.TH), tx = conv2d_ceil_div(n, (size_t)g.TW), vb = conv2d_ceil_div(v, (size_t)g.VB);
    p.grid_ok = conv2d_blocks(k, m, n, v, g.TH, g.TW, g.VB, &blocks) && blocks <= (size_t)CONV2D_MAX_GRID &&
                nsend <= 65535 && p.lds_bytes <= (size_t)CONV2D_LDS_LIMIT;
    p.grid_x = blocks;
    if (p.grid_ok) {
        g.tiles_y = (unsigned)ty;
        g.tiles_x = (unsigned)tx;
        g.vblocks = (unsigned)vb;
    }
    return p;
}

// what workgroup b of the grid's x dimension owns: channel blocks fastest (the workgroups that share a window are neighbours)
struct Conv2dBlock {
    size_t img;                     // the image
    size_t I0, J0;                  // first output row and column of the tile
    size_t j0;                      // first output channel of the block
};
FFG_HD Conv2dBlock conv2d_block(const Conv2dGeom& g, unsigned b) {
    Conv2dBlock o;
    o.j0 = (size_t)(b % g.vblocks) * (size_t)g.VB;
    b /= g.vblocks;
    o.J0 = (size_t)(b % g.tiles_x) * (size_t)g.TW;
    b /= g.tiles_x;
    o.I0 = (size_t)(b % g.tiles_y) * (size_t)g.TH;
    o.img = b / g.tiles_y;
    return o;
}

// what thread tid of a workgroup owns: pixel (py, px) of the tile, channels c0 .. c0 + VR - 1 of the block
struct Conv2dLane {
    int py, px, c0;
};
FFG_HD Conv2dLane conv2d_lane(const Conv2dGeom& g, int tid) {
    const int pl = g.TH * g.TW, p = tid % pl;
    Conv2dLane o;
    o.py = p / g.TW;
    o.px = p % g.TW;
    o.c0 = (tid / pl) * g.VR;
    return o;
}

// image row / column that window slot row wy / column wx holds for the tile at I0 / J0 (negative or past the image: zero)
FFG_HD int64_t conv2d_win_row(size_t I0, int wy, int s) { return (int64_t)I0 + wy - conv2d_row_off(s); }
FFG_HD int64_t conv2d_win_col(size_t J0, int wx, int s) { return (int64_t)J0 + wx - conv2d_col_off(s); }
// the halo test
FFG_HD bool conv2d_in_image(int64_t row, int64_t col, size_t m, size_t n) {
    return row >= 0 && col >= 0 && (uint64_t)row < (uint64_t)m && (uint64_t)col < (uint64_t)n;
}
// staged slot of window element (wy, wx) of the step's channel cl, and of tap (di, dj) of channel cl for channel c of the block
FFG_HD int conv2d_win_slot(const Conv2dGeom& g, int cl, int wy, int wx) { return (cl * g.WH + wy) * g.WW + wx; }
FFG_HD int conv2d_tap_slot(const Conv2dGeom& g, int cl, int c, int di, int dj) { return ((cl * g.VB + c) * g.s + di) * g.s + dj; }
// the inverse maps the staging loops use: slot -> (cl, wy, wx) and slot -> (cl, c, di * s + dj)
FFG_HD void conv2d_win_of(const Conv2dGeom& g, int slot, int& cl, int& wy, int& wx) {
    const int per = g.WH * g.WW;
    cl = slot / per;
    const int rem = slot - cl * per;
    wy = rem / g.WW;
    wx = rem - wy * g.WW;
}
FFG_HD void conv2d_tap_of(const Conv2dGeom& g, int slot, int& cl, int& c, int& tap) {
    const int ss = g.s * g.s, per = g.VB * ss;
    cl = slot / per;
    const int rem = slot - cl * per;
    c = rem / ss;
    tap = rem - c * ss;
}
// indices into the row-major tensors
FFG_HD size_t conv2d_x_index(const Conv2dGeom& g, size_t img, size_t l, size_t row, size_t col) {
    return ((img * g.r + l) * g.m + row) * g.n + col;
}
FFG_HD size_t conv2d_w_index(const Conv2dGeom& g, size_t j, size_t l, int tap) {
    return (j * g.r + l) * (size_t)(g.s * g.s) + (size_t)tap;
}
FFG_HD size_t conv2d_y_index(const Conv2dGeom& g, size_t img, size_t j, size_t row, size_t col) {
    return ((img * g.v + j) * g.m + row) * g.n + col;
}

}  // namespace ffgpu
