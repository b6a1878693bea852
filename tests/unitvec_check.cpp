// unitvec_check.cpp -- walks mpyc_amd/csrc/unitvec_geom.hpp on the host (g++, no HIP) against brute-force enumeration, for five
// element sizes and both alignments:
//   * the rows plan of the three kernels (unit_rows_plan / rows_unit / unit_elem): for n in {1, 2, 63, 64, 65, 128, 255,
//     256, 257, 5003} and rows in {1, 2, 3, 5, 8, 64}, the units of every row cover its n elements once and lie inside the row;
//     packs only on aligned pointers, whole waves for 24-byte elements; the factor of unit_prod for xstride in {1, 3, 16} is
//     the element's own (unit_x_at), its span (unit_x_span) the last factor plus one, a pack of x only for xstride 1;
//   * the rotation: for every kbits in 1..13, every c in [0, K2) and every j, the rolled source row (unit_roll_src) is
//     (j - c) mod K2 and the rotated table index (unit_dot_tab) (j + c) mod K2, the two are inverse to each other, and the
//     offset of an element (unit_offset) is the low kbits bits of its low limb whatever lies above them;
//   * the table of unit_dot (unit_dot_plan): entries, LDS bytes and the kbits limit per element size (14, 13, 12, 12, 11);
//   * counts out of range and overflowing sizes are refused.
// Prints "unitvec ok <plans>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/unitvec_geom.hpp"

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

static void check_rows(size_t n, size_t rows, size_t eb, bool aligned) {
    const RowsPlan pl = unit_rows_plan(n, rows, eb, aligned);
    const size_t gran = geom_gran(eb);
    CHECK(pl.ok && pl.span == rows * n, "n=%zu rows=%zu", n, rows);
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    else CHECK(pl.vec == (n % gran == 0 && (rows == 1 || (n * eb) % geom_align(eb) == 0)), "pack decision n=%zu rows=%zu eb=%zu", n, rows, eb);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == n, "loop length");
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs: whole waves");
    std::vector<int> seen(rows * n, 0);
    for (size_t j = 0; j < rows; ++j)
        for (size_t g = 0; g < pl.total; ++g) {
            const size_t u = rows_unit(pl, j, g);
            for (unsigned q = 0; q < pl.pack; ++q) {
                const size_t e = u * pl.pack + q, er = unit_elem(pl, g, q);
                CHECK(e < rows * n && er < n && e == j * n + er, "unit (%zu, %zu) is not its element of row %zu", j, g, j);
                ++seen[e];
            }
        }
    for (size_t e = 0; e < rows * n; ++e) CHECK(seen[e] == 1, "(row, element) %zu hit %d times", e, seen[e]);
    const size_t xs[3] = {1, 3, 16};
    for (size_t xstride : xs) {
        size_t span;
        CHECK(unit_x_span(n, xstride, eb, span) && span == (n - 1) * xstride + 1, "span of x");
        for (size_t e = 0; e < n; ++e) CHECK(unit_x_at(e, xstride) == e * xstride && unit_x_at(e, xstride) < span, "factor of element %zu", e);
        CHECK(unit_x_packs(pl, xstride) == (pl.vec && xstride == 1), "a pack of x only for consecutive factors");
    }
    ++nplans;
}

static void check_rotation(int kbits) {
    const size_t K2 = (size_t)1 << kbits;
    const uint64_t mask = unit_mask(kbits);
    CHECK(mask == K2 - 1, "mask");
    for (size_t c = 0; c < K2; ++c) {
        // the low kbits bits of the low limb, whatever lies above them
        CHECK(unit_offset((uint64_t)c, mask) == c && unit_offset((uint64_t)c | ~mask, mask) == c &&
                  unit_offset((uint64_t)c + ((uint64_t)0x9e3779b97f4a7c15ull << kbits), mask) == c,
              "offset of c=%zu", c);
        for (size_t j = 0; j < K2; ++j) {
            const size_t src = unit_roll_src(j, c, mask), tab = unit_dot_tab(j, c, mask);
            CHECK(src == (j + K2 - c) % K2, "source row kbits=%d c=%zu j=%zu", kbits, c, j);
            CHECK(tab == (j + c) % K2, "table index kbits=%d c=%zu j=%zu", kbits, c, j);
            CHECK(unit_roll_src(tab, c, mask) == j && unit_dot_tab(src, c, mask) == j, "the two are inverse");
        }
    }
    ++nplans;
}

int main() {
    const size_t ebs[5] = {4, 8, 12, 16, 24};
    const int maxk[5] = {14, 13, 12, 12, 11};
    const size_t ns[10] = {1, 2, 63, 64, 65, 128, 255, 256, 257, 5003};
    const size_t rs[6] = {1, 2, 3, 5, 8, 64};
    for (int i = 0; i < 5; ++i) {
        const size_t eb = ebs[i];
        for (int al = 0; al < 2; ++al) {
            for (size_t n : ns)
                for (size_t rows : rs) check_rows(n, rows, eb, al != 0);
            CHECK(unit_rows_plan(0, 3, eb, al != 0).ok && unit_rows_plan(0, 3, eb, al != 0).total == 0, "n = 0 is a plan of nothing");
            CHECK(!unit_rows_plan(5, 0, eb, al != 0).ok, "no rows");
            CHECK(!unit_rows_plan((size_t)1 << 62, 8, eb, al != 0).ok, "rows n overflows");
            CHECK(!unit_rows_plan(((size_t)1 << 61) / eb, 8, eb, al != 0).ok, "rows n eb overflows");
        }
        size_t span;
        CHECK(unit_x_span(0, 1, eb, span) && span == 0 && !unit_x_span(5, 0, eb, span), "x: nothing, and no stride");
        CHECK(!unit_x_span((size_t)1 << 62, 8, eb, span) && !unit_x_span(((size_t)1 << 61) / eb, 8, eb, span), "x overflows");
        // the table of unit_dot
        CHECK(unit_dot_max_kbits(eb) == maxk[i], "kbits limit of %zu-byte elements", eb);
        const size_t wb = unit_word_bytes(eb);
        CHECK(wb >= eb && (wb == eb || eb == 12), "one word per entry");
        for (int kbits = 0; kbits <= 16; ++kbits) {
            const size_t K2 = (size_t)1 << kbits;
            const UnitDotPlan a = unit_dot_plan(K2, true, kbits, K2, eb), b = unit_dot_plan(K2, true, kbits, 1, eb);
            CHECK(a.ok && b.ok && a.fits == (kbits <= maxk[i]) && a.entries == K2 && a.mask == K2 - 1, "rotated table kbits=%d", kbits);
            if (a.fits) CHECK(a.lds_bytes == K2 * wb && a.lds_bytes <= (size_t)UNIT_LDS_BYTES, "LDS bytes");
            CHECK(!unit_dot_plan(K2 + 1, true, kbits, 1, eb).ok && !unit_dot_plan(K2, true, kbits, K2 + 1, eb).ok &&
                      !unit_dot_plan(K2, true, kbits, 0, eb).ok,
                  "rows == K2, 1 <= tlen <= K2");
        }
        const UnitDotPlan p = unit_dot_plan(193, false, 7, 193, eb);
        CHECK(p.ok && p.fits && p.entries == 193 && p.mask == ~(uint64_t)0 && unit_dot_tab(150, 0, p.mask) == 150, "without a rotation");
        CHECK(!unit_dot_plan(193, false, 0, 192, eb).ok && !unit_dot_plan(0, false, 0, 0, eb).ok, "tlen == rows >= 1");
        CHECK(!unit_dot_plan(2, true, -1, 1, eb).ok && !unit_dot_plan(2, true, 31, 1, eb).ok, "kbits");
    }
    for (int kbits = 1; kbits <= 13; ++kbits) check_rotation(kbits);
    CHECK(unit_roll_valid(0, 1) && unit_roll_valid(3, 5) && unit_roll_valid(3, 8) && unit_roll_valid(30, (size_t)1 << 30), "K <= K2");
    CHECK(!unit_roll_valid(3, 9) && !unit_roll_valid(3, 0) && !unit_roll_valid(-1, 1) && !unit_roll_valid(31, 1), "K, kbits");
    CHECK(!unit_rows_plan(4, 2, 6, true).ok, "element size");
    printf("unitvec ok %zu\n", nplans);
    return 0;
}
