// rbits_check.cpp -- walks mpyc_amd/csrc/rbits_geom.hpp on the host (g++, no HIP) against brute-force enumeration, for five
// element sizes and both alignments:
//   * the opening (rbits_open_plan) and the finish (rbits_finish_plan): for every n at an edge of the launch plan -- 1, one
//     pack - 1 / pack / pack + 1, a wave of packs +- 1, one block of packs +- 1 and one entry past a grid of 3 blocks
//     (rbits_grid_entries) -- and every row count in {1, 3, 5, 7, 9, 10, 64}, the packs of the vector loop and the element
//     tail cover the n entries of a row once; pack i is elements i pack .. i pack + pack - 1; whole waves for 24-byte
//     elements; the grid is sized for the packs (or for the entries when there are none): the plan of the exponentiation
//     (stream_plan) restated;
//   * the opening keeps packs only for up to rbits_fused_rows(eb) rows (9; 5 for 24-byte elements), the finish for every row
//     count; no packs on unaligned pointers;
//   * row counts below 1 and above RBITS_MAX_ROWS and overflowing sizes are refused; n = 0 is a plan of nothing.
// Prints "rbits ok <plans>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/rbits_geom.hpp"

using namespace ffgpu;

#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAIL %s: ", #cond);   \
            printf(__VA_ARGS__);          \
            printf("\n");                 \
            exit(1);                      \
        }                                 \
    } while (0)

static size_t nplans = 0;

static void check_plan(const StreamPlan& pl, size_t n, int rows, size_t eb, bool packs, bool open) {
    CHECK(pl.ok && pl.pack == geom_pack(eb), "n=%zu rows=%d eb=%zu", n, rows, eb);
    const StreamPlan lp = stream_plan(n, eb, packs);
    CHECK(pl.nvec == lp.nvec && pl.tail == lp.tail && pl.threads == lp.threads, "the plan of the exponentiation");
    if (!packs) CHECK(pl.nvec == 0, "packs where none apply");
    else if (eb == 24) CHECK(pl.nvec % 64 == 0 && n - pl.nvec < 64, "24-byte packs: whole waves, a tail below one");
    else CHECK(pl.nvec == n / pl.pack, "every whole pack goes through the vector loop");
    CHECK(pl.tail == pl.nvec * pl.pack && pl.tail <= n, "the tail starts after the packs");
    CHECK(pl.threads == (pl.nvec ? pl.nvec : n), "the grid is sized for the packs");
    if (open && rows > rbits_fused_rows(eb)) CHECK(pl.nvec == 0, "packs beyond the fused rows");
    std::vector<int> seen(n, 0);
    for (size_t i = 0; i < pl.nvec; ++i)
        for (unsigned q = 0; q < pl.pack; ++q) {
            const size_t e = rbits_pack_at(pl.pack, i) + q;
            CHECK(e == i * pl.pack + q && e < pl.tail, "element of pack %zu", i);
            ++seen[e];
        }
    for (size_t e = pl.tail; e < n; ++e) ++seen[e];
    for (size_t e = 0; e < n; ++e) CHECK(seen[e] == 1, "entry %zu hit %d times", e, seen[e]);
    ++nplans;
}

int main() {
    const size_t ebs[5] = {4, 8, 12, 16, 24};
    const int rows[7] = {1, 3, 5, 7, 9, 10, 64};
    CHECK(RBITS_FUSED_ROWS == 9 && RBITS_FUSED_ROWS_24 == 5 && RBITS_MAX_ROWS == 64, "the row limits of the header");
    for (size_t eb : ebs) {
        const size_t pack = geom_pack(eb), wave = 64 * pack, block = rbits_grid_entries(1, eb), grid = rbits_grid_entries(3, eb);
        CHECK(block == (size_t)GEOM_THREADS * pack && grid == 3 * block, "entries of a grid");
        const size_t ns[] = {1, pack - 1, pack, pack + 1, wave - 1, wave, wave + 1, block - 1, block, block + 1, grid, grid + 1, 5003};
        CHECK(rbits_fused_rows(eb) == (eb == 24 ? 5 : 9), "fused rows per element size");
        for (int al = 0; al < 2; ++al) {
            for (size_t n : ns)
                for (int k : rows) {
                    check_plan(rbits_open_plan(n, k, eb, al != 0), n, k, eb, al != 0 && k <= rbits_fused_rows(eb), true);
                    check_plan(rbits_finish_plan(n, k, eb, al != 0), n, k, eb, al != 0, false);
                }
            CHECK(rbits_open_plan(0, 3, eb, al != 0).ok && rbits_open_plan(0, 3, eb, al != 0).threads == 0, "n = 0 is a plan of nothing");
            CHECK(rbits_finish_plan(0, 3, eb, al != 0).ok && rbits_finish_plan(0, 3, eb, al != 0).nvec == 0, "n = 0 is a plan of nothing");
            for (int bad : {0, -1, 65, 1 << 20}) {
                CHECK(!rbits_open_plan(5, bad, eb, al != 0).ok && !rbits_finish_plan(5, bad, eb, al != 0).ok, "rows=%d", bad);
                CHECK(!rbits_open_plan(0, bad, eb, al != 0).ok && !rbits_rows_valid(bad), "rows=%d at n = 0", bad);
            }
            CHECK(!rbits_open_plan((size_t)1 << 62, 3, eb, al != 0).ok && !rbits_finish_plan((size_t)1 << 62, 3, eb, al != 0).ok,
                  "n eb overflows");
        }
    }
    CHECK(!rbits_open_plan(4, 3, 6, true).ok && !rbits_finish_plan(4, 3, 2, true).ok && !rbits_finish_plan(4, 3, 0, true).ok, "element size");
    printf("rbits ok %zu\n", nplans);
    return 0;
}
