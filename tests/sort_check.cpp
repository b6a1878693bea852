// sort_check.cpp -- walks mpyc_amd/csrc/sort_geom.hpp on the host (g++, no HIP) against brute-force enumeration:
//   * the stage list of every k in 2..300 equals the reference's loop restated here, every listed stage is valid;
//   * cx_pairs equals |{ i < k - d : i & p == r }|, cx_index(j) is its j-th member, I and I + d are disjoint and in range;
//   * near misses of a stage are refused (p not a power of two, d of neither form, r not in {0, p}) and count 0 pairs;
//   * cx_plan / cx_at: for several (outer, inner), element sizes and alignments every unit of the flat loop maps to the
//     elements the maps of include/ffgpu.h name, every compact element and every member is owned exactly once, nothing
//     outside I and I + d is touched, packs are whole, contiguous and aligned, and the 24-byte path sees whole waves.
// Prints "sort ok <stages>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/sort_geom.hpp"

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

struct Stage {
    size_t p, d, r;
};

static std::vector<Stage> reference_stages(size_t k) {
    std::vector<Stage> out;
    int t = 0;
    while (((k - 1) >> t) != 0) ++t;                 // (k-1).bit_length()
    size_t p = (size_t)1 << (t - 1);
    while (p) {
        size_t d = p, q = (size_t)1 << (t - 1), r = 0;
        while (d) {
            out.push_back({p, d, r});
            d = q - p;
            q >>= 1;
            r = p;
        }
        p >>= 1;
    }
    return out;
}

static std::vector<size_t> brute(size_t k, size_t p, size_t d, size_t r) {
    std::vector<size_t> I;
    if (d >= k) return I;
    for (size_t i = 0; i < k - d; ++i)
        if ((i & p) == r) I.push_back(i);
    return I;
}

static void check_plan(size_t outer, size_t k, size_t inner, const Stage& s, size_t eb, bool aligned) {
    const CxPlan pl = cx_plan(outer, k, inner, s.p, s.d, s.r, eb, aligned);
    const std::vector<size_t> I = brute(k, s.p, s.d, s.r);
    CHECK(pl.ok && pl.pairs == I.size() && pl.row_elems == I.size() * inner, "k=%zu p=%zu d=%zu r=%zu", k, s.p, s.d, s.r);
    if (I.empty()) {
        CHECK(pl.total == 0, "empty stage with work");
        return;
    }
    const size_t u = pl.vec ? geom_pack(eb) : 1;
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    if (pl.vec) {
        CHECK((s.p * inner) % geom_gran(eb) == 0 && pl.row_elems % geom_gran(eb) == 0 && (k * inner * eb) % geom_align(eb) == 0, "pack conditions");
        CHECK(pl.total % (geom_gran(eb) / u) == 0, "whole waves");
    }
    CHECK(pl.total == outer * pl.row_elems / u, "loop length");
    std::vector<int> seen_a(outer * k * inner, 0), seen_c(outer * pl.row_elems, 0);
    for (size_t g = 0; g < pl.total; ++g) {
        const CxAt at = cx_at(pl, g);
        if (eb == 24 && pl.vec && g % 64 != 0) {     // lane L of a wave at first + L, in all three arrays
            const CxAt prev = cx_at(pl, g - 1);
            CHECK(at.lo == prev.lo + 1 && at.hi == prev.hi + 1 && at.c == prev.c + 1, "wave not contiguous at g=%zu", g);
        }
        if (pl.vec && (eb != 24 || g % 64 == 0)) CHECK((at.lo * u * eb) % geom_align(eb) == 0 && (at.hi * u * eb) % geom_align(eb) == 0 && (at.c * u * eb) % geom_align(eb) == 0, "alignment");
        for (size_t e = 0; e < u; ++e) {
            const size_t c = at.c * u + e, lo = at.lo * u + e, hi = at.hi * u + e;
            CHECK(c < seen_c.size() && hi < seen_a.size() && lo < hi, "out of range: k=%zu inner=%zu g=%zu", k, inner, g);
            const size_t o = c / pl.row_elems, j = (c % pl.row_elems) / inner, i = c % inner;
            CHECK(lo == (o * k + I[j]) * inner + i && hi == (o * k + I[j] + s.d) * inner + i,
                  "map: k=%zu inner=%zu p=%zu d=%zu r=%zu eb=%zu g=%zu", k, inner, s.p, s.d, s.r, eb, g);
            ++seen_c[c];
            ++seen_a[lo];
            ++seen_a[hi];
        }
    }
    for (size_t c = 0; c < seen_c.size(); ++c) CHECK(seen_c[c] == 1, "compact element %zu owned %d times", c, seen_c[c]);
    std::vector<int> member(k, 0);
    for (size_t x : I) {
        ++member[x];
        ++member[x + s.d];
    }
    for (size_t e = 0; e < seen_a.size(); ++e)
        CHECK(seen_a[e] == member[(e / inner) % k], "element %zu of a touched %d times", e, seen_a[e]);
}

int main() {
    size_t nstages = 0;
    for (size_t k = 2; k <= 300; ++k) {
        const std::vector<Stage> ref = reference_stages(k);
        size_t n = 0;
        for (CxStageIter it = cx_stages_begin(k); !cx_stages_done(it); cx_stages_next(it), ++n) {
            CHECK(n < ref.size() && it.p == ref[n].p && it.d == ref[n].d && it.r == ref[n].r, "stage %zu of k=%zu", n, k);
            CHECK(cx_stage_valid(k, it.p, it.d, it.r), "a listed stage is refused: k=%zu", k);
        }
        CHECK(n == ref.size(), "k=%zu: %zu stages, the reference has %zu", k, n, ref.size());
        nstages += n;
        for (const Stage& s : ref) {
            const std::vector<size_t> I = brute(k, s.p, s.d, s.r);
            CHECK(cx_pairs(k, s.p, s.d, s.r) == I.size(), "pairs: k=%zu p=%zu d=%zu r=%zu", k, s.p, s.d, s.r);
            std::vector<int> hit(k, 0);
            for (size_t j = 0; j < I.size(); ++j) {
                CHECK(cx_index(j, s.p, s.r) == I[j], "index: k=%zu p=%zu d=%zu r=%zu j=%zu", k, s.p, s.d, s.r, j);
                CHECK(I[j] + s.d < k, "second member out of range");
                ++hit[I[j]];
                ++hit[I[j] + s.d];
            }
            for (size_t i = 0; i < k; ++i) CHECK(hit[i] <= 1, "I and I + d meet at %zu: k=%zu p=%zu d=%zu r=%zu", i, k, s.p, s.d, s.r);
            // near misses
            CHECK(!cx_stage_valid(k, s.p * 3, s.d, s.r) && cx_pairs(k, s.p * 3, s.d, s.r) == 0, "p not a power of two");
            CHECK(!cx_stage_valid(k, s.p, s.d + 1, s.r) && cx_pairs(k, s.p, s.d + 1, s.r) == 0, "d of neither form");
            CHECK(!cx_stage_valid(k, s.p, s.d, s.r + 1 + s.p) && cx_pairs(k, s.p, s.d, s.r + 1 + s.p) == 0, "r not in {0, p}");
            if (k <= 70 || k == 96 || k == 128 || k == 257 || k == 300) {
                static const size_t shapes[][2] = {{1, 1}, {3, 1}, {1, 3}, {2, 64}, {2, 4}};
                static const size_t ebs[] = {4, 8, 12, 16, 24};
                for (const auto& sh : shapes)
                    for (size_t eb : ebs)
                        for (int aligned = 0; aligned < 2; ++aligned) check_plan(sh[0], k, sh[1], s, eb, aligned != 0);
            }
        }
    }
    // valid stages with no pair, stages past the array, invalid sizes
    CHECK(cx_stage_valid(4, 2, 2, 2) && cx_pairs(4, 2, 2, 2) == 0, "an empty stage");
    CHECK(cx_stage_valid(3, 2, 6, 2) && cx_pairs(3, 2, 6, 2) == 0, "d past the array");
    CHECK(!cx_stage_valid(1, 1, 1, 0) && !cx_stage_valid(8, 0, 0, 0) && !cx_stage_valid(8, 2, 0, 2), "degenerate stages");
    CHECK(!cx_stage_valid(8, (size_t)1 << 63, (size_t)1 << 63, (size_t)1 << 63), "d + p wraps");
    CHECK(!cx_plan((size_t)1 << 40, (size_t)1 << 30, 1, 1, 1, 0, 8, true).ok, "byte count overflows");
    CHECK(!cx_plan(1, (size_t)1 << 62, 4, 1, 1, 0, 8, true).ok, "element count overflows");
    CHECK(cx_plan(0, 8, 1, 1, 1, 0, 8, true).ok && cx_plan(0, 8, 1, 1, 1, 0, 8, true).total == 0, "outer == 0");
    // a large stage: the flat loop leaves 32 bits
    {
        const size_t k = (size_t)1 << 34;
        const CxPlan pl = cx_plan(1, k, 1, 4, 4, 0, 8, false);
        CHECK(pl.ok && !pl.narrow && pl.pairs == k / 2 && pl.total == k / 2, "wide plan");
        const CxAt at = cx_at(pl, pl.total - 1);
        CHECK(at.lo == k - 5 && at.hi == k - 1, "last pair of a wide stage");
    }
    printf("sort ok %zu\n", nstages);
    return 0;
}
