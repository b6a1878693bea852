// bsgn_check.cpp -- walks mpyc_amd/csrc/bsgn_geom.hpp on the host (g++, no HIP) against brute-force enumeration, for five
// element sizes and both alignments:
//   * the rows plan of the mask and of the finish in sum mode (bsgn_rows_plan / rows_unit): for n in {1, 2, 63, 64, 65,
//     128, 255, 256, 257, 5003} and w in 1..8, the units of every row cover its n elements once, every element a unit touches
//     lies inside row i of the (w, n) array, unit g of row i and unit g of `a` (of a sum-mode output) are the same elements of
//     their rows; packs only on aligned pointers, whole waves for 24-byte elements;
//   * the flat plan of the finish in rows mode (bsgn_flat_plan): the packs of the vector loop and the element tail cover the
//     w n entries once and it is the plan of the exponentiation over w n entries;
//   * the 2-bit codes of a unit (bsgn_sym_put / bsgn_sym_of): every (row, element) slot of a 64-bit word holds its own code;
//   * w outside 1..8, m outside 1..64 and overflowing sizes are refused.
// Prints "bsgn ok <plans>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/bsgn_geom.hpp"
#include "../mpyc_amd/csrc/rbits_geom.hpp"     // RBITS_MAX_ROWS: the row limit the parties are held to

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

static void check_rows(size_t n, int w, size_t eb, bool aligned) {
    const RowsPlan pl = bsgn_rows_plan(n, w, eb, aligned);
    const size_t W = (size_t)w, gran = geom_gran(eb);
    CHECK(pl.ok && pl.span == W * n, "n=%zu w=%d", n, w);
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    else CHECK(pl.vec == (n % gran == 0), "pack decision n=%zu w=%d eb=%zu", n, w, eb);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == n, "loop length");
    CHECK(pl.pack <= 4, "the codes of a unit: four elements at the most");
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs: whole waves");
    if (pl.vec) CHECK((n * eb) % geom_align(eb) == 0, "rows of packs start aligned");
    std::vector<int> seen(W * n, 0);
    for (size_t i = 0; i < W; ++i)
        for (size_t g = 0; g < pl.total; ++g) {
            const size_t u = rows_unit(pl, i, g);
            for (unsigned q = 0; q < pl.pack; ++q) {
                const size_t e = u * pl.pack + q, ea = g * pl.pack + q;      // entry of the (w, n) array, element of `a`
                CHECK(e < W * n && ea < n && e == i * n + ea, "unit (%zu, %zu) is not its element of row %zu", i, g, i);
                ++seen[e];
            }
        }
    for (size_t j = 0; j < W * n; ++j) CHECK(seen[j] == 1, "(row, element) %zu hit %d times", j, seen[j]);
    ++nplans;
}

static void check_flat(size_t n, int w, size_t eb, bool aligned) {
    const StreamPlan pl = bsgn_flat_plan(n, w, eb, aligned), want = stream_plan((size_t)w * n, eb, aligned);
    const size_t count = (size_t)w * n;
    CHECK(pl.ok && want.ok, "n=%zu w=%d eb=%zu", n, w, eb);
    CHECK(pl.pack == want.pack && pl.nvec == want.nvec && pl.tail == want.tail && pl.threads == want.threads,
          "the plan of the exponentiation over w n entries");
    if (!aligned) CHECK(pl.nvec == 0, "packs on unaligned pointers");
    else if (eb == 24) CHECK(pl.nvec % 64 == 0 && count - pl.nvec < 64, "24-byte packs: whole waves, a tail below one");
    else CHECK(pl.nvec == count / pl.pack, "every whole pack goes through the vector loop");
    std::vector<int> seen(count, 0);
    for (size_t i = 0; i < pl.nvec; ++i)
        for (unsigned q = 0; q < pl.pack; ++q) {
            CHECK(i * pl.pack + q < pl.tail, "pack %zu", i);
            ++seen[i * pl.pack + q];
        }
    for (size_t e = pl.tail; e < count; ++e) ++seen[e];
    for (size_t e = 0; e < count; ++e) CHECK(seen[e] == 1, "entry %zu hit %d times", e, seen[e]);
    ++nplans;
}

int main() {
    const size_t ebs[5] = {4, 8, 12, 16, 24};
    const size_t ns[10] = {1, 2, 63, 64, 65, 128, 255, 256, 257, 5003};
    for (size_t eb : ebs)
        for (int al = 0; al < 2; ++al) {
            for (size_t n : ns)
                for (int w = 1; w <= BSGN_MAX_ROWS; ++w) {
                    check_rows(n, w, eb, al != 0);
                    check_flat(n, w, eb, al != 0);
                }
            CHECK(bsgn_rows_plan(0, 3, eb, al != 0).ok && bsgn_rows_plan(0, 3, eb, al != 0).total == 0, "n = 0 is a plan of nothing");
            CHECK(bsgn_flat_plan(0, 3, eb, al != 0).ok && bsgn_flat_plan(0, 3, eb, al != 0).threads == 0, "n = 0 is a plan of nothing");
            // refusals: the row count, overflowing sizes
            CHECK(!bsgn_rows_plan(5, 0, eb, al != 0).ok && !bsgn_rows_plan(5, -1, eb, al != 0).ok && !bsgn_rows_plan(5, 9, eb, al != 0).ok, "w");
            CHECK(!bsgn_flat_plan(5, 0, eb, al != 0).ok && !bsgn_flat_plan(5, 9, eb, al != 0).ok, "w");
            CHECK(!bsgn_rows_plan((size_t)1 << 62, 8, eb, al != 0).ok && !bsgn_flat_plan((size_t)1 << 62, 8, eb, al != 0).ok, "w n overflows");
            CHECK(!bsgn_rows_plan(((size_t)1 << 61) / eb, 8, eb, al != 0).ok && !bsgn_flat_plan(((size_t)1 << 61) / eb, 8, eb, al != 0).ok,
                  "w n eb overflows");
        }
    CHECK(!bsgn_rows_plan(4, 2, 6, true).ok && !bsgn_flat_plan(4, 2, 2, true).ok, "element size");
    CHECK(bsgn_w_valid(1) && bsgn_w_valid(8) && !bsgn_w_valid(0) && !bsgn_w_valid(9), "1 <= w <= 8");
    CHECK(bsgn_m_valid(1) && bsgn_m_valid(64) && !bsgn_m_valid(0) && !bsgn_m_valid(65), "1 <= m <= 64");
    CHECK((int)BSGN_MAX_PARTIES == (int)RBITS_MAX_ROWS, "the parties of one exponentiation");
    // the codes of a unit: slot (i, q) holds its own two bits and no other slot's
    for (int i = 0; i < BSGN_MAX_ROWS; ++i)
        for (int q = 0; q < 4; ++q)
            for (unsigned c = 0; c < 3; ++c) {
                const uint64_t v = bsgn_sym_put(0, i, q, c);
                for (int i2 = 0; i2 < BSGN_MAX_ROWS; ++i2)
                    for (int q2 = 0; q2 < 4; ++q2)
                        CHECK(bsgn_sym_of(v, i2, q2) == (i2 == i && q2 == q ? c : 0u), "slot (%d, %d)", i, q);
                const uint64_t full = bsgn_sym_put(~(uint64_t)0 & ~((uint64_t)3 << bsgn_sym_shift(i, q)), i, q, c);
                CHECK(bsgn_sym_of(full, i, q) == c, "slot (%d, %d) among set neighbours", i, q);
            }
    CHECK(bsgn_sym_shift(BSGN_MAX_ROWS - 1, 3) == 62, "the last slot ends the word");
    printf("bsgn ok %zu\n", nplans);
    return 0;
}
