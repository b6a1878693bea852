// matmul_stack_geom.hpp -- which shape a stack of matrix products takes and who owns which output (matmul_stack.hpp).
// Plain C++ (no HIP): the kernels and their launcher take every index from here, and tests/matmul_stack_check.cpp
// walks the same functions with g++.
//
// C[b] = A[b] @ B[b], b < batch, every matrix M x K times K x N.  Two shapes:
//   packed  M * N <= 256: a workgroup takes P consecutive matrices and computes one output per thread -- thread t owns
//           output (i, j) = ((t % (M N)) / N, t % N) of matrix P * workgroup + t / (M N).  Both operands of the P pairs
//           are staged in LDS, K in chunks of KC terms so that the pairs stay inside STACK_LDS_BUDGET; an operand that
//           the whole stack shares (batch stride 0) is staged once, not P times.
//   tiled   everything else: k_matmul's 32 x 32 / 64 x 32 output tiles, the matrix index folded into a FLAT tile index
//           (blockIdx.x: grid.z stops at 65 535 and the batch must not).
// Neither shape needs scratch memory or a workspace, and any batch is one launch.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum {
    STACK_THREADS = 256,          // = BLOCK (kernels.hpp)
    STACK_LDS_BUDGET = 16384,     // bytes of staged operands per workgroup: eight workgroups still fit a compute unit's 160 KiB
    STACK_KC_WANT = 8,            // a chunk shorter than this (and than K) halves P instead
    STACK_MAX_GRID = 0x7fffffff
};
enum StackShape { STACK_PACKED = 0, STACK_TILED = 1 };

struct StackPlan {
    int ok;                       // 0: sizes the kernels are not built for (more workgroups than a grid holds)
    int shape;                    // StackShape
    int P;                        // packed: matrices per workgroup
    int KC;                       // packed: terms per staged chunk (0 only for K == 0)
    int rows_a, rows_b;           // packed: rows of A / columns of B staged per term (P M and P N; M, N when shared)
    size_t lds_bytes;             // packed: dynamic LDS of the launch, at most STACK_LDS_BUDGET
    int bm, bn;                   // tiled: output tile
    size_t tiles_m, tiles_n;      // tiled: tiles per matrix
    size_t grid;                  // workgroups
};

// LDS bytes of one staged element: its word, or 4 bytes per 28-bit digit for the digit-column policies (lazy_nl > 0)
FFG_HD int stack_slot_bytes(int word_bytes, int lazy_nl) { return lazy_nl > 0 ? 4 * lazy_nl : word_bytes; }

// elem_bytes: storage of an element (1: the packed-byte fields, >= 12: words of two or three limbs); slot_bytes:
// stack_slot_bytes of the policy; shared_a / shared_b: the operand has batch stride 0.
FFG_HD StackPlan stack_plan(size_t M, size_t K, size_t N, size_t batch, int elem_bytes, int num_cu, int slot_bytes,
                                bool shared_a, bool shared_b) {
    StackPlan p = {};
    if (M == 0 || N == 0 || batch == 0 || M >= ((size_t)1 << 30) || N >= ((size_t)1 << 30) || K >= ((size_t)1 << 30) ||
        slot_bytes < 1 || num_cu < 1)
        return p;
    if (M * N <= (size_t)STACK_THREADS) {
        p.shape = STACK_PACKED;
        int P = (int)((size_t)STACK_THREADS / (M * N));
        for (;;) {
            p.rows_a = (int)(shared_a ? M : (size_t)P * M);
            p.rows_b = (int)(shared_b ? N : (size_t)P * N);
            const size_t per = (size_t)(p.rows_a + p.rows_b) * (size_t)slot_bytes;        // bytes per term
            const size_t fit = (size_t)STACK_LDS_BUDGET / per;
            p.KC = (int)(K < fit ? K : fit);
            const size_t want = K < (size_t)STACK_KC_WANT ? K : (size_t)STACK_KC_WANT;
            if ((size_t)p.KC >= want || P == 1) break;
            P = (P + 1) / 2;
        }
        if (K > 0 && p.KC < 1) return p;              // (cannot happen: M + N <= 257 and a slot has at most 28 bytes)
        p.P = P;
        p.lds_bytes = (size_t)(p.rows_a + p.rows_b) * (size_t)slot_bytes * (size_t)p.KC;
        p.grid = (batch + (size_t)P - 1) / (size_t)P;
    } else {
        p.shape = STACK_TILED;
        p.bn = 32;
        // 64 x 32 tiles (4 x 2 outputs per thread) for one-limb words once the stack gives every fourth compute unit a
        // tile; words of two or three limbs, packed bytes and small stacks take 32 x 32 (k_matmul's rule, per stack)
        const size_t t64 = ((M + 63) / 64) * ((N + 31) / 32);
        const size_t q = (size_t)num_cu / 4;
        const bool small_out = t64 < q && batch < q && batch * t64 < q;
        p.bm = (elem_bytes >= 12 || elem_bytes == 1 || small_out) ? 32 : 64;
        p.tiles_m = (M + (size_t)p.bm - 1) / (size_t)p.bm;
        p.tiles_n = (N + (size_t)p.bn - 1) / (size_t)p.bn;
        const size_t per = p.tiles_m * p.tiles_n;     // < 2^50
        if (batch > (size_t)STACK_MAX_GRID / per) return p;
        p.grid = batch * per;
    }
    if (p.grid > (size_t)STACK_MAX_GRID) return p;
    p.ok = 1;
    return p;
}

// packed: the output thread t of workgroup wg owns; false: the thread owns none (past the P matrices or the batch)
FFG_HD bool stack_packed_owner(int P, int M, int N, size_t batch, size_t wg, int t, size_t& b, int& pl, int& i, int& j) {
    const int mn = M * N;
    pl = t / mn;
    const int rem = t - pl * mn;
    i = rem / N;
    j = rem - i * N;
    b = wg * (size_t)P + (size_t)pl;
    return pl < P && b < batch;
}

// tiled: flat tile index -> matrix and tile origin
FFG_HD void stack_tile_of(size_t flat, size_t tiles_m, size_t tiles_n, int bm, int bn, size_t& b, int& m0, int& n0) {
    const size_t per = tiles_m * tiles_n;
    b = flat / per;
    const size_t r = flat - b * per;
    m0 = (int)(r / tiles_n) * bm;
    n0 = (int)(r % tiles_n) * bn;
}
// tiled: thread t of a tile owns rows m0 + t / 16 + 16 u (u < bm / 16) and columns n0 + t % 16 + 16 v (v < bn / 16).
// A RESTATEMENT for the host walk of what the tile body (matmul_tile_body.hpp) computes inline as ty + 16 i, tx + 16 j: the kernel
// does not call these two.
FFG_HD int stack_tile_row(int m0, int t, int u) { return m0 + (t >> 4) + 16 * u; }
FFG_HD int stack_tile_col(int n0, int t, int v) { return n0 + (t & 15) + 16 * v; }

}  // namespace ffgpu
