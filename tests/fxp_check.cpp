// fxp_check.cpp -- walks mpyc_amd/csrc/fxp_geom.hpp on the host (g++, no HIP) against brute-force enumeration, for l in 2..64,
// n in {1, 2, 63, 64, 65, 257}, five element sizes and both alignments:
//   * the norm kernels (fxp_norm_plan / rev_at / rev_next): every unit of the flat loop maps to the elements the
//     maps of include/ffgpu.h name -- compact element c = h (l-1) + j reads bits[h l + l-2-j] and the sign bit
//     bits[h l + l-1]; every (h, j) is owned exactly once, the sign bit is never a source, every bit below it is a source
//     once, no index falls outside n * l; stepping through a pack with rev_next gives what rev_at gives;
//   * the flat plan of trunc_finish (flat_plan): the units cover n once;
//   * the pack decision agrees with alignment and size: never on unaligned pointers, always when the array is a whole number
//     of geom_gran(eb) elements on aligned ones, whole waves for 24-byte elements;
//   * bit counts out of range and overflowing sizes are refused.
// Prints "fxp ok <plans>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/fxp_geom.hpp"

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

static void check_norm(size_t n, int l, size_t eb, bool aligned) {
    const RevPlan pl = fxp_norm_plan(n, l, eb, aligned);
    const size_t l1 = (size_t)l - 1, elems = n * l1, gran = geom_gran(eb);
    CHECK(pl.ok && pl.l == (size_t)l && pl.l1 == l1 && pl.elems == elems, "n=%zu l=%d", n, l);
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    else CHECK(pl.vec == (elems % gran == 0), "pack decision n=%zu l=%d eb=%zu", n, l, eb);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == elems, "loop length");
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs: whole waves");
    if (pl.vec) CHECK((pl.pack * eb) % geom_align(eb) == 0 || pl.pack == 1, "a pack is a whole aligned access");
    std::vector<int> seen_c(elems, 0), seen_src(n * (size_t)l, 0);
    for (size_t g = 0; g < pl.total; ++g) {
        RevAt at = rev_at(pl, g * pl.pack);
        for (unsigned q = 0; q < pl.pack; ++q) {
            const size_t c = g * pl.pack + q;
            const RevAt ref = rev_at(pl, c);
            CHECK(at.h == ref.h && at.j == ref.j && at.src == ref.src && at.top == ref.top, "next() and at() differ at c=%zu", c);
            CHECK(at.h == c / l1 && at.j == c % l1, "c=%zu -> (h, j)", c);
            CHECK(at.h < n && at.j < l1, "(h, j) out of range");
            CHECK(at.top == at.h * (size_t)l + l1 && at.src == at.h * (size_t)l + (l1 - 1 - at.j), "sources of c=%zu", c);
            CHECK(at.src < n * (size_t)l && at.top < n * (size_t)l && at.src != at.top, "source out of range");
            ++seen_c[at.h * l1 + at.j];
            ++seen_src[at.src];
            rev_next(pl, at);
        }
    }
    for (size_t c = 0; c < elems; ++c) CHECK(seen_c[c] == 1, "compact element %zu owned %d times", c, seen_c[c]);
    for (size_t e = 0; e < n * (size_t)l; ++e) CHECK(seen_src[e] == (e % (size_t)l == l1 ? 0 : 1), "bit %zu read %d times", e, seen_src[e]);
    ++nplans;
}

static void check_flat(size_t n, size_t eb, bool aligned) {
    const FlatPlan pl = flat_plan(n, eb, aligned);
    const size_t gran = geom_gran(eb);
    CHECK(pl.ok, "n=%zu", n);
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    else CHECK(pl.vec == (n % gran == 0), "pack decision n=%zu eb=%zu", n, eb);
    CHECK(pl.total * (pl.vec ? geom_pack(eb) : 1) == n, "the units cover n");
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs: whole waves");
    ++nplans;
}

int main() {
    const size_t ebs[] = {4, 8, 12, 16, 24}, ns[] = {1, 2, 63, 64, 65, 257};
    for (size_t eb : ebs)
        for (int al = 0; al < 2; ++al) {
            for (size_t n : ns) {
                for (int l = 2; l <= 64; ++l) check_norm(n, l, eb, al != 0);
                check_flat(n, eb, al != 0);
            }
            for (size_t n : {(size_t)128, (size_t)2048, (size_t)5003}) check_flat(n, eb, al != 0);
        }
    // refused
    CHECK(!fxp_norm_plan(5, 1, 8, true).ok && !fxp_norm_plan(5, 65, 8, true).ok && !fxp_norm_plan(5, 0, 8, true).ok, "l out of range");
    CHECK(!fxp_norm_plan(5, 16, 6, true).ok && !flat_plan(5, 2, true).ok, "element size");
    CHECK(!fxp_norm_plan((size_t)1 << 62, 16, 8, true).ok && !fxp_norm_plan((size_t)1 << 57, 64, 8, true).ok, "n * l overflows");
    CHECK(!flat_plan((size_t)1 << 61, 24, true).ok && !flat_plan((size_t)1 << 60, 8, true).ok, "n * eb overflows");
    CHECK(fxp_norm_plan(0, 16, 8, true).ok && fxp_norm_plan(0, 16, 8, true).total == 0 && flat_plan(0, 8, true).total == 0, "empty");
    // a large array: wide indices, no 32-bit division
    {
        const size_t n = ((size_t)1 << 33) + 3;
        const RevPlan pl = fxp_norm_plan(n, 33, 8, false);
        CHECK(pl.ok && !pl.narrow && pl.shift == 5, "wide plan");
        const RevAt at = rev_at(pl, pl.elems - 1);
        CHECK(at.h == n - 1 && at.j == 31 && at.src == (n - 1) * 33 && at.top == n * 33 - 1, "last element of a wide plan");
    }
    printf("fxp ok %zu\n", nplans);
    return 0;
}
