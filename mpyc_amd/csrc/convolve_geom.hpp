// convolve_geom.hpp -- tile / window index arithmetic of k_convolve (convolve.hpp).  Plain C++ (no HIP): the kernel and its
// launcher take every index from here, and tests/convolve_check.cpp walks the same functions with g++ against the plain
// double loop.
//
// c[k] = sum_j a[k - j] v[j], 0 <= k < na + nv - 1, a the longer operand (na >= nv), v the taps.  Output-stationary:
// a workgroup owns TO consecutive outputs k0 .. k0 + TO and walks the taps that can reach them in chunks of TV.  Its
// BLOCK threads are G tap groups of OL output lanes; a lane owns the R outputs k0 + o + OL r and group g takes taps
// g, g + G, ... of a chunk, so that an output's terms are spread over G accumulators which the workgroup adds at the
// end.  No partial sums ever leave the workgroup: the kernel needs no scratch memory.  Two shapes:
//   wide    OL = 64 (a group is a wave: one tap per wave and step), G = 4, TO = 128 -- many outputs, e.g. few taps
//           over a long array, where a tile's window is fetched once for 128 outputs;
//   narrow  OL = 16, G = 16, TO = 32 -- few outputs and many taps (4096 x 4096 is 64 wide tiles on 256 compute units,
//           but 256 narrow ones): the launcher takes it while the wide tiles would not fill the chip.
// Per chunk the workgroup stages the TV taps and the WIN = TO + TV - 1 elements of `a` they meet, one element per thread
// (WIN + TV <= BLOCK): window slot i holds a[k0 - j0 - (TV - 1) + i], zero outside [0, na).
#pragma once
#include "geom.hpp"

namespace ffgpu {

template <int R_, int OL_>
struct ConvShape {
    enum {
        THREADS = 256,          // = BLOCK (kernels.hpp)
        OL = OL_,               // output lanes of a tap group
        G = THREADS / OL,       // tap groups
        R = R_,                 // outputs per lane
        TO = OL * R,            // outputs per workgroup
        TV = 64,                // taps per chunk
        WIN = TO + TV - 1,      // window elements per chunk
        PER = TV / G            // most terms one accumulator takes per chunk
    };
    static_assert(WIN + TV <= THREADS, "one staged element per thread");
    static_assert(TV % G == 0, "tap groups share a chunk evenly");
};
enum { CONV_R = 2 };                            // outputs per lane of both shapes
typedef ConvShape<CONV_R, 64> ConvWide;
typedef ConvShape<CONV_R, 16> ConvNarrow;

// the wide shape once it gives every compute unit `per_cu` tiles, the narrow one below that
FFG_HD bool conv_use_wide(size_t nout, int num_cu, int per_cu) {
    return (nout + ConvWide::TO - 1) / ConvWide::TO >= (size_t)num_cu * (size_t)per_cu;
}

FFG_HD size_t conv_tiles(size_t nout, int TO) { return (nout + (size_t)TO - 1) / (size_t)TO; }

// taps that reach the outputs [k0, k0 + TO): lo <= j < hi needs 0 <= k - j < na for some k of the tile.  Never empty for
// k0 < na + nv - 1.
FFG_HD void conv_tap_range(size_t k0, int TO, size_t na, size_t nv, size_t& lo, size_t& hi) {
    lo = k0 + 1 > na ? k0 + 1 - na : 0;
    hi = k0 + (size_t)TO < nv ? k0 + (size_t)TO : nv;
}

// index into `a` of window slot i for the chunk of taps starting at j0 (negative or >= na: the slot holds zero)
FFG_HD int64_t conv_win_index(size_t k0, size_t j0, int TV, int slot) {
    return (int64_t)k0 - (int64_t)j0 - (int64_t)(TV - 1) + (int64_t)slot;
}
// window slot that tap jj of the chunk (0 <= jj < TV) meets at local output o (0 <= o < TO)
FFG_HD int conv_win_slot(int o, int jj, int TV) { return o - jj + (TV - 1); }

// unreduced accumulation: `since` terms (at most) sit in an accumulator that holds `flush` of them; after a chunk added up to
// PER more, reduce before the next chunk could pass the bound
FFG_HD bool conv_flush_due(int since, int PER, int flush) { return since + PER > flush; }

}  // namespace ffgpu
