// tour_check.cpp -- walks mpyc_amd/csrc/tour_geom.hpp on the host (g++, no HIP) against brute-force enumeration:
//   * for every k in 2..300 and both pairings, tour_first / tour_second equal the reference's slices enumerated here
//     (a[n0:(k+1)/2] against a[(k+1)/2:], and a[n0::2] against a[n0+1::2]), the pairs are disjoint and, with the bye,
//     cover 0..k-1 exactly once;
//   * tour_plan / tour_at: for a grid of (outer, inner), five element sizes and both alignments every unit of the flat loop
//     maps to the elements the maps of include/ffgpu.h name in the full, the half and the compact arrays; every compact
//     element, every member, every position of the half level and every bye element is owned exactly once; packs are
//     whole, contiguous and aligned, and the 24-byte path sees whole waves, the bye included;
//   * invalid rounds and overflowing sizes are refused.
// Prints "tour ok <plans>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/tour_geom.hpp"

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

// the reference's slices by enumeration
static void brute(size_t k, int mode, std::vector<size_t>& a1, std::vector<size_t>& a2) {
    const size_t n0 = k % 2;
    a1.clear();
    a2.clear();
    if (mode == TOUR_HALVES) {
        for (size_t x = n0; x < (k + 1) / 2; ++x) a1.push_back(x);
        for (size_t x = (k + 1) / 2; x < k; ++x) a2.push_back(x);
    } else {
        for (size_t x = n0; x < k; x += 2) a1.push_back(x);
        for (size_t x = n0 + 1; x < k; x += 2) a2.push_back(x);
    }
}

static size_t nplans = 0;

static void check_plan(size_t outer, size_t k, size_t inner, int mode, size_t eb, bool aligned) {
    const TourPlan pl = tour_plan(outer, k, inner, mode, eb, aligned);
    std::vector<size_t> a1, a2;
    brute(k, mode, a1, a2);
    const size_t n0 = k % 2, h = k / 2, kc = h + n0;
    CHECK(pl.ok && pl.pairs == h && pl.next == kc && pl.row_elems == h * inner, "k=%zu mode=%d", k, mode);
    const size_t u = pl.vec ? geom_pack(eb) : 1;
    const size_t run = mode == TOUR_HALVES ? h * inner : inner;
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    if (pl.vec) {
        CHECK(run % geom_gran(eb) == 0 && pl.row_elems % geom_gran(eb) == 0 && (n0 * inner) % geom_gran(eb) == 0, "pack conditions");
        CHECK(pl.total % (geom_gran(eb) / u) == 0 && pl.bye % (geom_gran(eb) / u) == 0, "whole waves");
    } else if (aligned) {
        CHECK(run % geom_gran(eb) != 0 || pl.row_elems % geom_gran(eb) != 0 || (n0 * inner) % geom_gran(eb) != 0, "packs apply and are not taken");
    }
    CHECK(pl.total == outer * pl.row_elems / u, "loop length");
    const size_t nfull = outer * k * inner, nhalf = outer * kc * inner, ncomp = outer * h * inner;
    std::vector<int> seen_full(nfull, 0), seen_half(nhalf, 0), seen_c(ncomp, 0), bye_full(nfull, 0), bye_half(nhalf, 0);
    for (size_t g = 0; g < pl.total; ++g) {
        const TourAt at = tour_at(pl, g);
        if (eb == 24 && pl.vec && g % 64 != 0) {     // lane L of a wave at first + L, in every array
            const TourAt prev = tour_at(pl, g - 1);
            CHECK(at.first == prev.first + 1 && at.second == prev.second + 1 && at.c == prev.c + 1 && at.half == prev.half + 1,
                  "wave not contiguous at g=%zu", g);
            CHECK(at.bye == prev.bye && (!at.bye || (at.bye_full == prev.bye_full + 1 && at.bye_half == prev.bye_half + 1)),
                  "bye splits a wave at g=%zu", g);
        }
        if (pl.vec && (eb != 24 || g % 64 == 0)) {
            const size_t al = geom_align(eb), ub = u * eb;
            CHECK((at.first * ub) % al == 0 && (at.second * ub) % al == 0 && (at.c * ub) % al == 0 && (at.half * ub) % al == 0, "alignment");
            if (at.bye) CHECK((at.bye_full * ub) % al == 0 && (at.bye_half * ub) % al == 0, "alignment of the bye");
        }
        for (size_t e = 0; e < u; ++e) {
            const size_t c = at.c * u + e, lo = at.first * u + e, hi = at.second * u + e, hf = at.half * u + e;
            CHECK(c < ncomp && lo < nfull && hi < nfull && hf < nhalf, "out of range: k=%zu inner=%zu g=%zu", k, inner, g);
            const size_t o = c / pl.row_elems, j = (c % pl.row_elems) / inner, i = c % inner;
            CHECK(lo == (o * k + a1[j]) * inner + i && hi == (o * k + a2[j]) * inner + i,
                  "members: k=%zu inner=%zu mode=%d eb=%zu g=%zu", k, inner, mode, eb, g);
            CHECK(hf == (o * kc + n0 + j) * inner + i, "half level: k=%zu inner=%zu mode=%d eb=%zu g=%zu", k, inner, mode, eb, g);
            ++seen_c[c];
            ++seen_full[lo];
            ++seen_full[hi];
            ++seen_half[hf];
            if (at.bye) {
                const size_t bf = at.bye_full * u + e, bh = at.bye_half * u + e;
                CHECK(n0 == 1 && j == 0 && bf < nfull && bh < nhalf, "bye out of range");
                CHECK(bf == o * k * inner + i && bh == o * kc * inner + i, "bye: k=%zu inner=%zu g=%zu", k, inner, g);
                ++bye_full[bf];
                ++bye_half[bh];
            }
        }
    }
    for (size_t c = 0; c < ncomp; ++c) CHECK(seen_c[c] == 1, "compact element %zu owned %d times", c, seen_c[c]);
    for (size_t e = 0; e < nfull; ++e) {
        const bool is_bye = n0 && (e / inner) % k == 0;
        CHECK(seen_full[e] == (is_bye ? 0 : 1) && bye_full[e] == (is_bye ? 1 : 0), "element %zu of the full level: %d / %d", e,
              seen_full[e], bye_full[e]);
    }
    for (size_t e = 0; e < nhalf; ++e) {
        const bool is_bye = n0 && (e / inner) % kc == 0;
        CHECK(seen_half[e] == (is_bye ? 0 : 1) && bye_half[e] == (is_bye ? 1 : 0), "element %zu of the half level: %d / %d", e,
              seen_half[e], bye_half[e]);
    }
    ++nplans;
}

int main() {
    for (size_t k = 2; k <= 300; ++k) {
        for (int mode = 0; mode < 2; ++mode) {
            std::vector<size_t> a1, a2;
            brute(k, mode, a1, a2);
            const size_t n0 = k % 2;
            CHECK(a1.size() == tour_pairs(k) && a2.size() == tour_pairs(k) && tour_next(k) == tour_pairs(k) + n0, "k=%zu mode=%d: pair count", k, mode);
            std::vector<int> hit(k, 0);
            for (size_t j = 0; j < a1.size(); ++j) {
                CHECK(tour_first(k, mode, j) == a1[j] && tour_second(k, mode, j) == a2[j], "k=%zu mode=%d j=%zu", k, mode, j);
                CHECK(a1[j] < k && a2[j] < k, "member out of range");
                ++hit[a1[j]];
                ++hit[a2[j]];
            }
            if (n0) ++hit[0];
            for (size_t i = 0; i < k; ++i) CHECK(hit[i] == 1, "k=%zu mode=%d: position %zu covered %d times", k, mode, i, hit[i]);
            if (k <= 40 || k == 63 || k == 64 || k == 65 || k == 128 || k == 129 || k == 257 || k == 300) {
                static const size_t outers[] = {1, 3};
                static const size_t inners[] = {1, 2, 3, 4, 64, 65};
                static const size_t ebs[] = {4, 8, 12, 16, 24};
                for (size_t outer : outers)
                    for (size_t inner : inners)
                        for (size_t eb : ebs)
                            for (int aligned = 0; aligned < 2; ++aligned) check_plan(outer, k, inner, mode, eb, aligned != 0);
            }
        }
    }
    // whole waves of 24-byte elements, the bye included
    CHECK(tour_plan(2, 5, 128, TOUR_HALVES, 24, true).vec && tour_plan(2, 5, 128, TOUR_ODD_EVEN, 24, true).vec, "waves");
    CHECK(tour_plan(2, 4, 32, TOUR_HALVES, 24, true).vec && !tour_plan(2, 4, 32, TOUR_ODD_EVEN, 24, true).vec, "runs of a mode");
    CHECK(!tour_plan(2, 5, 32, TOUR_HALVES, 24, true).vec, "a bye that is no whole wave");
    check_plan(2, 5, 128, TOUR_HALVES, 24, true);
    check_plan(2, 5, 128, TOUR_ODD_EVEN, 24, true);
    check_plan(1, 4, 32, TOUR_HALVES, 24, true);
    // invalid rounds, invalid sizes
    CHECK(!tour_plan(1, 1, 1, TOUR_HALVES, 8, true).ok && !tour_plan(1, 0, 1, TOUR_ODD_EVEN, 8, true).ok, "k < 2");
    CHECK(!tour_plan(1, 8, 1, 2, 8, true).ok && !tour_plan(1, 8, 1, -1, 8, true).ok, "unknown pairing");
    CHECK(!tour_mode_valid(2) && tour_mode_valid(TOUR_HALVES) && tour_mode_valid(TOUR_ODD_EVEN), "modes");
    CHECK(!tour_plan((size_t)1 << 40, (size_t)1 << 30, 1, TOUR_HALVES, 8, true).ok, "byte count overflows");
    CHECK(!tour_plan(1, (size_t)1 << 62, 4, TOUR_ODD_EVEN, 8, true).ok, "element count overflows");
    CHECK(tour_plan(0, 8, 1, TOUR_HALVES, 8, true).ok && tour_plan(0, 8, 1, TOUR_HALVES, 8, true).total == 0, "outer == 0");
    CHECK(tour_plan(3, 8, 0, TOUR_HALVES, 8, true).ok && tour_plan(3, 8, 0, TOUR_HALVES, 8, true).total == 0, "inner == 0");
    // a large round: the flat loop leaves 32 bits
    {
        const size_t k = ((size_t)1 << 34) + 1;
        const TourPlan pl = tour_plan(1, k, 1, TOUR_ODD_EVEN, 8, false);
        CHECK(pl.ok && !pl.narrow && pl.pairs == k / 2 && pl.total == k / 2, "wide plan");
        const TourAt at = tour_at(pl, pl.total - 1);
        CHECK(at.first == k - 2 && at.second == k - 1 && at.half == k / 2 && !at.bye, "last pair of a wide round");
        const TourPlan ph = tour_plan(1, k, 1, TOUR_HALVES, 8, false);
        const TourAt ah = tour_at(ph, 0);
        CHECK(ah.first == 1 && ah.second == k / 2 + 1 && ah.bye && ah.bye_full == 0 && ah.bye_half == 0, "first pair of a wide round");
    }
    printf("tour ok %zu\n", nplans);
    return 0;
}
