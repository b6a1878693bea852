// iszero_check.cpp -- walks mpyc_amd/csrc/iszero_geom.hpp on the host (g++, no HIP) against brute-force enumeration, for five
// element sizes and both alignments:
//   * the mask (iszero_mask_plan / rows_unit): for n in {1, 2, 63, 64, 65, 128, 255, 256, 257, 5003} and k in
//     {1, 2, 8, 9, 30}, the units of every row cover its n elements once, every element a unit touches lies inside row i of
//     the (k, n) array and below k n, unit g of row i and unit g of `a` are the same elements of their rows, and (row,
//     element) pairs are hit exactly once; packs only on aligned pointers, whole waves for 24-byte elements;
//   * the symbols (stream_plan): the packs of the vector loop and the element tail cover the count entries once, the code
//     bytes of pack i are bytes i pack .. i pack + pack - 1, whole waves for 24-byte elements, the grid is sized for the packs
//     (or for the entries when there are none) -- the plan of the exponentiation restated;
//   * the finish (flat_plan / iszero_code_at): every entry and every code byte is owned once;
//   * the code word of a pack (iszero_code_put / iszero_code_of) and the alignment rule of the byte array;
//   * k < 1 and overflowing sizes are refused.
// Prints "iszero ok <plans>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/iszero_geom.hpp"

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

static void check_mask(size_t n, int k, size_t eb, bool aligned) {
    const RowsPlan pl = iszero_mask_plan(n, k, eb, aligned);
    const size_t K = (size_t)k, gran = geom_gran(eb);
    CHECK(pl.ok && pl.span == K * n, "n=%zu k=%d", n, k);
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    else CHECK(pl.vec == (n % gran == 0), "pack decision n=%zu k=%d eb=%zu", n, k, eb);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == n, "loop length");
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs: whole waves");
    if (pl.vec) CHECK((n * eb) % geom_align(eb) == 0, "rows of packs start aligned");
    std::vector<int> seen(K * n, 0);
    for (size_t i = 0; i < K; ++i)
        for (size_t g = 0; g < pl.total; ++g) {
            const size_t u = rows_unit(pl, i, g);
            for (unsigned q = 0; q < pl.pack; ++q) {
                const size_t e = u * pl.pack + q, ea = g * pl.pack + q;      // entry of the (k, n) array, element of `a`
                CHECK(e < K * n && ea < n && e == i * n + ea, "unit (%zu, %zu) is not its element of row %zu", i, g, i);
                ++seen[e];
            }
        }
    for (size_t j = 0; j < K * n; ++j) CHECK(seen[j] == 1, "(row, element) %zu hit %d times", j, seen[j]);
    ++nplans;
}

static void check_legendre(size_t count, size_t eb, bool aligned) {
    const StreamPlan pl = stream_plan(count, eb, aligned);
    CHECK(pl.ok && pl.pack == geom_pack(eb), "count=%zu eb=%zu", count, eb);
    if (!aligned) CHECK(pl.nvec == 0, "packs on unaligned pointers");
    else if (eb == 24) CHECK(pl.nvec % 64 == 0 && count - pl.nvec < 64, "24-byte packs: whole waves, a tail below one");
    else CHECK(pl.nvec == count / pl.pack, "every whole pack goes through the vector loop");
    CHECK(pl.tail == pl.nvec * pl.pack && pl.tail <= count, "the tail starts after the packs");
    CHECK(pl.threads == (pl.nvec ? pl.nvec : count), "the grid is sized for the packs");
    std::vector<int> seen(count, 0);
    for (size_t i = 0; i < pl.nvec; ++i)
        for (unsigned q = 0; q < pl.pack; ++q) {
            const size_t b = iszero_code_at(pl.pack, i) + q;
            CHECK(b == i * pl.pack + q && b < pl.tail, "code byte of pack %zu", i);
            ++seen[b];
        }
    for (size_t e = pl.tail; e < count; ++e) ++seen[e];
    for (size_t e = 0; e < count; ++e) CHECK(seen[e] == 1, "entry %zu hit %d times", e, seen[e]);
    ++nplans;
}

static void check_finish(size_t count, size_t eb, bool aligned) {
    const FlatPlan pl = flat_plan(count, eb, aligned);
    CHECK(pl.ok, "count=%zu eb=%zu", count, eb);
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    else CHECK(pl.vec == (count != 0 && count % geom_gran(eb) == 0), "pack decision count=%zu eb=%zu", count, eb);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == count, "loop length");
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs: whole waves");
    std::vector<int> seen(count, 0);
    for (size_t g = 0; g < pl.total; ++g) {
        const size_t b = iszero_code_at(pl.pack, g);
        CHECK(b % pl.pack == 0, "the codes of a unit start on a multiple of the pack");
        for (unsigned q = 0; q < pl.pack; ++q) {
            CHECK(b + q < count, "code byte of unit %zu", g);
            ++seen[b + q];
        }
    }
    for (size_t e = 0; e < count; ++e) CHECK(seen[e] == 1, "entry %zu hit %d times", e, seen[e]);
    ++nplans;
}

int main() {
    const size_t ebs[5] = {4, 8, 12, 16, 24};
    const size_t ns[10] = {1, 2, 63, 64, 65, 128, 255, 256, 257, 5003};
    const int ks[5] = {1, 2, 8, 9, 30};
    for (size_t eb : ebs)
        for (int al = 0; al < 2; ++al) {
            for (size_t n : ns)
                for (int k : ks) {
                    check_mask(n, k, eb, al != 0);
                    check_legendre((size_t)k * n, eb, al != 0);
                    check_finish((size_t)k * n, eb, al != 0);
                }
            check_legendre(0, eb, al != 0);
            check_finish(0, eb, al != 0);
            CHECK(iszero_mask_plan(0, 3, eb, al != 0).ok && iszero_mask_plan(0, 3, eb, al != 0).total == 0, "n = 0 is a plan of nothing");
            // refusals: the row count, overflowing sizes
            CHECK(!iszero_mask_plan(5, 0, eb, al != 0).ok && !iszero_mask_plan(5, -1, eb, al != 0).ok, "k < 1");
            CHECK(!iszero_mask_plan((size_t)1 << 62, 8, eb, al != 0).ok, "k n overflows");
            CHECK(!iszero_mask_plan(((size_t)1 << 61) / eb, 30, eb, al != 0).ok, "k n eb overflows");
            CHECK(!stream_plan((size_t)1 << 62, eb, al != 0).ok && !flat_plan((size_t)1 << 62, eb, al != 0).ok, "count eb overflows");
        }
    CHECK(!iszero_mask_plan(4, 2, 6, true).ok && !stream_plan(4, 2, true).ok && !flat_plan(4, 0, true).ok, "element size");
    // the code word of a pack, and the alignment of the byte array for the one access that moves it
    for (unsigned c0 = 0; c0 < 3; ++c0)
        for (unsigned c1 = 0; c1 < 3; ++c1)
            for (unsigned c3 = 0; c3 < 3; ++c3) {
                uint32_t v = iszero_code_put(iszero_code_put(iszero_code_put(0, 0, c0), 1, c1), 3, c3);
                CHECK(iszero_code_of(v, 0) == c0 && iszero_code_of(v, 1) == c1 && iszero_code_of(v, 2) == 0 && iszero_code_of(v, 3) == c3,
                      "code word");
                CHECK(v == (c0 | (c1 << 8) | (c3 << 24)), "byte q of the word is the code of element q (little-endian)");
            }
    for (uintptr_t a = 0; a < 16; ++a) {
        CHECK(iszero_codes_aligned(a, 4) == (a % 4 == 0) && iszero_codes_aligned(a, 8) == (a % 2 == 0), "alignment of a pack's codes");
        CHECK(iszero_codes_aligned(a, 12) && iszero_codes_aligned(a, 16) && iszero_codes_aligned(a, 24), "one byte needs none");
    }
    CHECK(LEGENDRE_NONRESIDUE == 0 && LEGENDRE_RESIDUE == 1 && LEGENDRE_ZERO == 2, "the codes of the header");
    printf("iszero ok %zu\n", nplans);
    return 0;
}
