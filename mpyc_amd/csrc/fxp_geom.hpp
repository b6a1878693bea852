// fxp_geom.hpp -- index arithmetic and launch plans of the fixed-point kernels (fxp.hpp): the finish of the secure truncation
// (runtime.np_trunc, runtime.py:839-873) and the gate in front of the search of runtime._norm (runtime.py:4718-4727).  Plain C++
// (no HIP): the kernels, their launcher and the C ABI take every index from here, and tests/fxp_check.cpp walks the same
// functions with g++.  (The mask of the truncation owns a tile per workgroup: its geometry is sgn_geom.hpp, as it is.)
//
// trunc_finish is flat over the n elements: flat_plan (geom.hpp) as it is.  The two norm kernels are flat over the COMPACT
// array (n, l - 1): the bits of an element below its sign bit, most significant first.  bits is what ffgpu_bits_finish writes,
// element-major (n, l), least significant first, so compact element c = h (l - 1) + j takes
//   src = h l + (l - 2 - j)     the bit of weight 2^(l-2-j): the row of element h read backwards from below the sign bit
//   top = h l + (l - 1)         the sign bit x_top of element h
// which is the reversed-row walk of geom.hpp with the top of every row left out (RevPlan, rev_at / rev_next).
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { FXP_MAX_BITS = 64 };

// ---- norm_prod / norm_apply: one flat loop over the compact (n, l - 1) array ------------------------------------------------------
FFG_HD bool fxp_norm_l_valid(int l) { return l >= 2 && l <= FXP_MAX_BITS; }
FFG_HD RevPlan fxp_norm_plan(size_t n, int l, size_t eb, bool aligned) {
    if (!fxp_norm_l_valid(l)) return RevPlan();
    return rev_plan(n, (size_t)l, true, eb, aligned);
}

}  // namespace ffgpu
