// matmul_stack_check.cpp -- host walk of the stacked-product geometry (mpyc_amd/csrc/matmul_stack_geom.hpp), built with
// g++ by tests/test_matmul_stack_host.py.  For every (M, K, N) up to 41 in each dimension, every element width with the
// LDS slot sizes of its policies, shared and per-matrix operands and several CU counts it checks that
//   * the packed shape is never chosen with M N > 256, and P M N <= 256;
//   * the staged operands stay inside STACK_LDS_BUDGET, the chunk is at least one term and the rows are what the kernel
//     indexes (P M, P N; M, N for a shared operand);
//   * grids stay within limits (and a batch that does not fit is refused);
// and, for batches around every P boundary, that every (matrix, row, column) is owned by exactly one thread of one
// workgroup -- by replaying the index functions the kernels call (stack_packed_owner, stack_tile_of); thread ownership
// inside a tile is walked through stack_tile_row / stack_tile_col, which restate matmul_tile's inline ty + 16 i, tx + 16 j.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "../mpyc_amd/csrc/matmul_stack_geom.hpp"

using namespace ffgpu;

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::printf("FAIL %s line %d: M %zu K %zu N %zu batch %zu eb %d slot %d cu %d sa %d sb %d\n", #cond, __LINE__, \
                        M, K, N, batch, eb, slot, cu, (int)sa, (int)sb);                                               \
            return false;                                                                                              \
        }                                                                                                              \
    } while (0)

// every output of the stack exactly once
static bool own(const StackPlan& p, size_t M, size_t K, size_t N, size_t batch, int eb, int slot, int cu, bool sa, bool sb) {
    std::vector<int> seen(batch * M * N, 0);
    if (p.shape == STACK_PACKED) {
        for (size_t wg = 0; wg < p.grid; ++wg)
            for (int t = 0; t < STACK_THREADS; ++t) {
                size_t b;
                int pl, i, j;
                if (!stack_packed_owner(p.P, (int)M, (int)N, batch, wg, t, b, pl, i, j)) continue;
                CHECK(b < batch && i >= 0 && (size_t)i < M && j >= 0 && (size_t)j < N && pl >= 0 && pl < p.P);
                CHECK(b / (size_t)p.P == wg);
                // the rows the thread reads lie inside what was staged
                CHECK((sa ? i : pl * (int)M + i) < p.rows_a && (sb ? j : pl * (int)N + j) < p.rows_b);
                ++seen[(b * M + (size_t)i) * N + (size_t)j];
            }
    } else {
        for (size_t flat = 0; flat < p.grid; ++flat) {
            size_t b;
            int m0, n0;
            stack_tile_of(flat, p.tiles_m, p.tiles_n, p.bm, p.bn, b, m0, n0);
            CHECK(b < batch && m0 >= 0 && (size_t)m0 < M && n0 >= 0 && (size_t)n0 < N);
            for (int t = 0; t < STACK_THREADS; ++t)
                for (int u = 0; u < p.bm / 16; ++u)
                    for (int v = 0; v < p.bn / 16; ++v) {
                        const int r = stack_tile_row(m0, t, u), c = stack_tile_col(n0, t, v);
                        CHECK(r >= m0 && r < m0 + p.bm && c >= n0 && c < n0 + p.bn);
                        if ((size_t)r < M && (size_t)c < N) ++seen[(b * M + (size_t)r) * N + (size_t)c];
                    }
        }
    }
    for (int s : seen) CHECK(s == 1);
    return true;
}

static bool plan_ok(size_t M, size_t K, size_t N, int eb, int slot, int cu, bool sa, bool sb, std::set<std::tuple<size_t, size_t, int, int, int, int>>& walked) {
    size_t batch = 1;
    const StackPlan p1 = stack_plan(M, K, N, 1, eb, cu, slot, sa, sb);
    CHECK(p1.ok);
    std::vector<size_t> batches = {1, 2, 3};
    if (p1.shape == STACK_PACKED) {
        CHECK(M * N <= (size_t)STACK_THREADS);
        const size_t P = (size_t)p1.P;
        for (size_t bb : {P - 1, P, P + 1, 2 * P + 1, 3 * P})
            if (bb >= 1) batches.push_back(bb);
    } else {
        CHECK(M * N > (size_t)STACK_THREADS);
    }
    for (size_t bt : batches) {
        batch = bt;
        const StackPlan p = stack_plan(M, K, N, batch, eb, cu, slot, sa, sb);
        CHECK(p.ok && p.shape == p1.shape);
        CHECK(p.grid >= 1 && p.grid <= (size_t)STACK_MAX_GRID);
        if (p.shape == STACK_PACKED) {
            CHECK(p.P == p1.P && p.P >= 1 && (size_t)p.P * M * N <= (size_t)STACK_THREADS);
            CHECK(p.rows_a == (int)(sa ? M : (size_t)p.P * M) && p.rows_b == (int)(sb ? N : (size_t)p.P * N));
            CHECK(p.KC >= 1 && (size_t)p.KC <= K);
            CHECK(p.lds_bytes == (size_t)(p.rows_a + p.rows_b) * (size_t)slot * (size_t)p.KC);
            CHECK(p.lds_bytes <= (size_t)STACK_LDS_BUDGET);
            CHECK(p.grid == (batch + (size_t)p.P - 1) / (size_t)p.P);
        } else {
            CHECK(p.bn == 32 && (p.bm == 32 || p.bm == 64));
            CHECK(!(eb >= 12 || eb == 1) || p.bm == 32);
            CHECK(p.tiles_m * (size_t)p.bm >= M && (p.tiles_m - 1) * (size_t)p.bm < M);
            CHECK(p.tiles_n * (size_t)p.bn >= N && (p.tiles_n - 1) * (size_t)p.bn < N);
            CHECK(p.grid == batch * p.tiles_m * p.tiles_n);
        }
        // ownership depends on (M, N, batch) and on P or the tile only: walk each such case once
        const auto key = std::make_tuple(M, N, p.shape == STACK_PACKED ? p.P : p.bm, (int)batch, (int)sa, (int)sb);
        if (walked.insert(key).second && !own(p, M, K, N, batch, eb, slot, cu, sa, sb)) return false;
    }
    return true;
}

int main() {
    // element widths and the LDS slot of their policies: the word, or 4 bytes per 28-bit digit (4, 5 and 7 digits)
    const int widths[][2] = {{1, 1}, {4, 4}, {8, 8}, {12, 16 /* the word, and PM96's 4 digits */}, {16, 16}, {16, 20}, {24, 24}, {24, 28}};
    const int cus[] = {1, 64, 256, 304};
    std::set<std::tuple<size_t, size_t, int, int, int, int>> walked;
    size_t plans = 0;
    for (size_t M = 1; M <= 41; ++M)
        for (size_t N = 1; N <= 41; ++N)
            for (size_t K = 1; K <= 41; ++K)
                for (const auto& w : widths)
                    for (int cu : cus)
                        for (int sh = 0; sh < 3; ++sh) {     // no shared operand, A shared, B shared
                            if (!plan_ok(M, K, N, w[0], w[1], cu, sh == 1, sh == 2, walked)) return 1;
                            ++plans;
                        }
    // long K: chunks, and P gives way before the chunk drops under STACK_KC_WANT terms
    for (size_t K : {(size_t)97, (size_t)577, (size_t)4096, (size_t)100000})
        for (size_t M : {(size_t)1, (size_t)4, (size_t)8, (size_t)16, (size_t)256})
            for (size_t N : {(size_t)1, (size_t)4, (size_t)8, (size_t)16})
                for (const auto& w : widths) {
                    if (!plan_ok(M, K, N, w[0], w[1], 256, false, false, walked)) return 1;
                    const StackPlan p = stack_plan(M, K, N, 7, w[0], 256, w[1], false, false);
                    if (p.shape == STACK_PACKED && p.P > 1 && p.KC < STACK_KC_WANT) {
                        std::printf("FAIL short chunk with P > 1: M %zu K %zu N %zu slot %d\n", M, K, N, w[1]);
                        return 1;
                    }
                    ++plans;
                }
    {   // grids: a tiled batch past the limit is refused, the largest that fits is not; a packed one likewise; no batch, no plan
        const size_t big = (size_t)STACK_MAX_GRID;
        if (stack_plan(64, 8, 64, big / 2 + 1, 8, 256, 8, false, false).ok || !stack_plan(64, 8, 64, big / 2, 8, 256, 8, false, false).ok ||
            stack_plan(16, 8, 16, big + 1, 8, 256, 8, false, false).ok || !stack_plan(16, 8, 16, big, 8, 256, 8, false, false).ok ||
            stack_plan(16, 8, 16, 0, 8, 256, 8, false, false).ok || stack_plan(0, 8, 16, 1, 8, 256, 8, false, false).ok ||
            stack_plan((size_t)1 << 30, 8, 16, 1, 8, 256, 8, false, false).ok ||
            stack_plan(1000, 8, 1000, ~(size_t)0 / 2, 8, 256, 8, false, false).ok) {
            std::printf("FAIL grid limits\n");
            return 1;
        }
        const StackPlan z = stack_plan(4, 0, 4, 5, 8, 256, 8, false, false);          // K == 0: zeros, nothing staged
        if (!z.ok || z.shape != STACK_PACKED || z.KC != 0 || z.lds_bytes != 0) {
            std::printf("FAIL K == 0\n");
            return 1;
        }
    }
    std::printf("matmul_stack ok: %zu plans, %zu ownership walks\n", plans, walked.size());
    return 0;
}
