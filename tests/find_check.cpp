// find_check.cpp -- walks mpyc_amd/csrc/find_geom.hpp on the host (g++, no HIP) against brute-force enumeration, for k in
// 1..300, virt in {0, 1}, five element sizes, inner in {1, 3, 64, 65, 128}, both alignments and 2..3 components:
//   * the leaf round (find_leaf_plan / find_leaf_at): every unit of the flat loop maps to the elements the maps of
//     include/ffgpu.h name -- pair j = (n0 + 2j, n0 + 2j + 1) over kv = k + virt positions, the bits at pitch k * inner, the
//     next level at pitch kc * inner; every compact element, every real pair member, every position of the next level and
//     the bye is owned exactly once; the virtual position k is flagged, is always the second member of the last pair and is
//     never turned into a bit address; no address falls outside outer * k * inner; packs are whole, contiguous, aligned
//     and lie within one position; the 24-byte path sees whole waves, the bye and the virtual partner included;
//   * a stored level (find_plan + tour_at): the plane distances are those of (C, outer, kk, inner) and its companions, and
//     whole packs keep every plane aligned;
//   * invalid rounds and overflowing sizes are refused.
// Prints "find ok <plans>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/find_geom.hpp"

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

static void check_leaf(size_t outer, size_t k, size_t inner, int virt, int ncomp, size_t eb, bool aligned) {
    const size_t kv = k + (size_t)virt;
    const FindPlan pl = find_leaf_plan(outer, k, inner, ncomp, virt, eb, aligned);
    if (kv < 2) {
        CHECK(!pl.t.ok, "a round over one position");
        return;
    }
    const size_t n0 = kv % 2, h = kv / 2, kc = h + n0;
    CHECK(pl.t.ok && pl.t.pairs == h && pl.t.next == kc && pl.t.row_elems == h * inner && pl.kv == kv && pl.virt == virt, "k=%zu virt=%d", k, virt);
    const size_t u = pl.t.vec ? geom_pack(eb) : 1, gran = geom_gran(eb);
    if (!aligned) CHECK(!pl.t.vec, "packs on unaligned pointers");
    if (pl.t.vec) CHECK(inner % gran == 0, "pack conditions");
    else if (aligned) CHECK(inner % gran != 0, "packs apply and are not taken");
    CHECK(pl.t.total == outer * h * inner / u && pl.t.pitch_full == k * inner / u && pl.t.pitch_half == kc * inner / u, "loop length and pitches");
    CHECK(pl.plane_c == outer * h * inner / u && pl.plane_half == outer * kc * inner / u, "plane distances");
    if (pl.t.vec) CHECK((pl.plane_c * u * eb) % geom_align(eb) == 0 && (pl.plane_half * u * eb) % geom_align(eb) == 0 && pl.plane_c % (gran / u) == 0 && pl.plane_half % (gran / u) == 0, "planes stay aligned");
    const size_t nbits = outer * k * inner, nhalf = outer * kc * inner, nc = outer * h * inner;
    std::vector<int> seen_bits(nbits, 0), seen_half(nhalf, 0), seen_c(nc, 0), bye_bits(nbits, 0), bye_half(nhalf, 0);
    size_t virtual_pairs = 0;
    for (size_t g = 0; g < pl.t.total; ++g) {
        const FindAt at = find_leaf_at(pl, g);
        if (eb == 24 && pl.t.vec && g % 64 != 0) {     // lane L of a wave at first + L, in every array; flags wave-uniform
            const FindAt prev = find_leaf_at(pl, g - 1);
            CHECK(at.first == prev.first + 1 && at.second == prev.second + 1 && at.c == prev.c + 1 && at.half == prev.half + 1, "wave not contiguous at g=%zu", g);
            CHECK(at.virt2 == prev.virt2 && at.pos == prev.pos, "the public leaf or a position splits a wave at g=%zu", g);
            CHECK(at.bye == prev.bye && (!at.bye || (at.bye_full == prev.bye_full + 1 && at.bye_half == prev.bye_half + 1)), "bye splits a wave at g=%zu", g);
        }
        if (pl.t.vec && (eb != 24 || g % 64 == 0)) {
            const size_t al = geom_align(eb), ub = u * eb;
            CHECK((at.first * ub) % al == 0 && (at.second * ub) % al == 0 && (at.c * ub) % al == 0 && (at.half * ub) % al == 0, "alignment");
            if (at.bye) CHECK((at.bye_full * ub) % al == 0 && (at.bye_half * ub) % al == 0, "alignment of the bye");
        }
        for (size_t e = 0; e < u; ++e) {
            const size_t c = at.c * u + e, lo = at.first * u + e, hi = at.second * u + e, hf = at.half * u + e;
            CHECK(c < nc && lo < nbits && hi < nbits && hf < nhalf, "out of range: k=%zu virt=%d inner=%zu g=%zu", k, virt, inner, g);
            const size_t o = c / (h * inner), j = (c % (h * inner)) / inner, i = c % inner;
            const size_t p1 = n0 + 2 * j, p2 = p1 + 1;
            CHECK(at.pos == p1 && p2 < kv, "position: k=%zu virt=%d inner=%zu g=%zu", k, virt, inner, g);
            CHECK(p1 < k && lo == (o * k + p1) * inner + i, "first member: k=%zu virt=%d inner=%zu eb=%zu g=%zu", k, virt, inner, eb, g);
            CHECK(hf == (o * kc + n0 + j) * inner + i, "next level: k=%zu virt=%d inner=%zu eb=%zu g=%zu", k, virt, inner, eb, g);
            ++seen_c[c];
            ++seen_bits[lo];
            ++seen_half[hf];
            if (p2 == k) {                              // the public leaf: flagged, no address of its own
                CHECK(virt && at.virt2 && j == h - 1 && hi == lo, "virtual position turned into an address: k=%zu inner=%zu g=%zu", k, inner, g);
                ++virtual_pairs;
            } else {
                CHECK(!at.virt2 && hi == (o * k + p2) * inner + i, "second member: k=%zu virt=%d inner=%zu eb=%zu g=%zu", k, virt, inner, eb, g);
                ++seen_bits[hi];
            }
            if (at.bye) {
                const size_t bf = at.bye_full * u + e, bh = at.bye_half * u + e;
                CHECK(n0 == 1 && j == 0 && bf < nbits && bh < nhalf, "bye out of range");
                CHECK(bf == o * k * inner + i && bh == o * kc * inner + i, "bye: k=%zu inner=%zu g=%zu", k, inner, g);
                ++bye_bits[bf];
                ++bye_half[bh];
            }
        }
    }
    CHECK(virtual_pairs == (virt ? outer * inner : 0), "the public leaf is the partner of %zu elements", virtual_pairs);
    for (size_t c = 0; c < nc; ++c) CHECK(seen_c[c] == 1, "compact element %zu owned %d times", c, seen_c[c]);
    for (size_t e = 0; e < nbits; ++e) {
        const bool is_bye = n0 && (e / inner) % k == 0;
        CHECK(seen_bits[e] == (is_bye ? 0 : 1) && bye_bits[e] == (is_bye ? 1 : 0), "bit %zu: %d / %d (k=%zu virt=%d inner=%zu)", e, seen_bits[e], bye_bits[e], k, virt, inner);
    }
    for (size_t e = 0; e < nhalf; ++e) {
        const bool is_bye = n0 && (e / inner) % kc == 0;
        CHECK(seen_half[e] == (is_bye ? 0 : 1) && bye_half[e] == (is_bye ? 1 : 0), "element %zu of the next level: %d / %d", e, seen_half[e], bye_half[e]);
    }
    ++nplans;
}

static void check_level(size_t outer, size_t k, size_t inner, int ncomp, size_t eb, bool aligned) {
    const FindPlan pl = find_plan(outer, k, inner, ncomp, eb, aligned);
    const TourPlan t = tour_plan(outer, k, inner, TOUR_ODD_EVEN, eb, aligned);
    CHECK(pl.t.ok && t.ok && pl.t.vec == t.vec && pl.t.total == t.total && pl.t.pitch_full == t.pitch_full && pl.t.pitch_half == t.pitch_half &&
              pl.t.run == t.run && pl.t.bye == t.bye && pl.t.row_units == t.row_units, "a stored level is a tournament round per component");
    const size_t u = pl.t.vec ? geom_pack(eb) : 1, h = k / 2, kc = h + k % 2;
    CHECK(pl.plane_full * u == outer * k * inner && pl.plane_half * u == outer * kc * inner && pl.plane_c * u == outer * h * inner && pl.kv == k && !pl.virt, "plane distances");
    if (pl.t.vec)
        CHECK((pl.plane_full * u * eb) % geom_align(eb) == 0 && pl.plane_full % (geom_gran(eb) / u) == 0 && pl.plane_c % (geom_gran(eb) / u) == 0, "planes stay aligned");
    // the last unit of the last component stays inside (C, outer, k, inner) and (C, outer, h, inner)
    if (pl.t.total) {
        const TourAt at = tour_at(pl.t, pl.t.total - 1);
        CHECK(((size_t)(ncomp - 1) * pl.plane_full + at.second) * u + u <= (size_t)ncomp * outer * k * inner, "level out of range");
        CHECK(((size_t)(ncomp - 1) * pl.plane_c + at.c) * u + u <= (size_t)ncomp * outer * h * inner, "compact out of range");
    }
    ++nplans;
}

int main() {
    static const size_t outers[] = {1, 3};
    static const size_t inners[] = {1, 3, 64, 65, 128};
    static const size_t ebs[] = {4, 8, 12, 16, 24};
    for (size_t k = 1; k <= 300; ++k) {
        for (size_t inner : inners) {
            for (size_t eb : ebs)
                for (int virt = 0; virt < 2; ++virt)
                    for (int aligned = 0; aligned < 2; ++aligned) {
                        const size_t outer = inner > 3 && k > 12 ? 1 : outers[(k + inner + (size_t)virt) % 2];     // (long rows: one of them)
                        const int ncomp = 2 + (int)((k + eb / 4) % 2);
                        check_leaf(outer, k, inner, virt, ncomp, eb, aligned != 0);
                        if (k >= 2 && !virt) check_level(outer, k, inner, ncomp, eb, aligned != 0);
                    }
        }
    }
    // whole waves of 24-byte elements with the public leaf as the partner of a wave run, and as the only partner
    CHECK(find_leaf_plan(2, 5, 128, 3, 1, 24, true).t.vec && find_leaf_plan(1, 1, 64, 2, 1, 24, true).t.vec, "waves");
    CHECK(!find_leaf_plan(2, 5, 65, 3, 1, 24, true).t.vec && find_leaf_plan(2, 5, 65, 3, 1, 16, true).t.vec, "runs that are no whole waves");
    check_leaf(1, 1, 5003, 1, 2, 8, true);
    check_leaf(1, 1, 5003, 1, 2, 8, false);
    // invalid rounds, invalid sizes
    CHECK(!find_leaf_plan(1, 0, 1, 2, 1, 8, true).t.ok && !find_leaf_plan(1, 1, 1, 2, 0, 8, true).t.ok && find_leaf_plan(1, 1, 1, 2, 1, 8, true).t.ok, "k < 1, kv < 2");
    CHECK(!find_leaf_plan(1, 4, 1, 2, 2, 8, true).t.ok && !find_leaf_plan(1, 4, 1, 2, -1, 8, true).t.ok, "virt outside {0, 1}");
    CHECK(!find_plan(1, 1, 1, 2, 8, true).t.ok && !find_plan(1, 0, 1, 2, 8, true).t.ok, "a stored level with k < 2");
    for (int ncomp : {-1, 0, 1, 6, 7})
        CHECK(!find_comp_valid(ncomp) && !find_plan(1, 4, 1, ncomp, 8, true).t.ok && !find_leaf_plan(1, 4, 1, ncomp, 1, 8, true).t.ok, "ncomp=%d", ncomp);
    for (int ncomp : {2, 3, 4, 5}) CHECK(find_comp_valid(ncomp) && find_plan(1, 4, 1, ncomp, 8, true).t.ok, "ncomp=%d", ncomp);
    CHECK(!find_plan((size_t)1 << 40, (size_t)1 << 30, 1, 2, 8, true).t.ok && !find_leaf_plan(1, (size_t)1 << 62, 4, 2, 0, 8, true).t.ok, "sizes overflow");
    CHECK(find_plan((size_t)1 << 55, 8, 1, 2, 8, true).t.ok && !find_plan((size_t)1 << 55, 8, 1, 5, 8, true).t.ok, "the components overflow the byte count");
    CHECK(!find_leaf_plan(1, ~(size_t)0, 1, 2, 1, 8, true).t.ok, "k + virt wraps");
    CHECK(find_leaf_plan(0, 8, 1, 2, 1, 8, true).t.ok && find_leaf_plan(0, 8, 1, 2, 1, 8, true).t.total == 0, "outer == 0");
    CHECK(find_plan(3, 8, 0, 2, 8, true).t.ok && find_plan(3, 8, 0, 2, 8, true).t.total == 0, "inner == 0");
    // a large round: the flat loop leaves 32 bits; the public leaf closes the last pair
    {
        const size_t k = ((size_t)1 << 34) + 1;
        const FindPlan pl = find_leaf_plan(1, k, 1, 2, 1, 8, false);
        CHECK(pl.t.ok && !pl.t.narrow && pl.t.pairs == (k + 1) / 2 && pl.t.total == (k + 1) / 2, "wide plan");
        const FindAt at = find_leaf_at(pl, pl.t.total - 1);
        CHECK(at.first == k - 1 && at.second == k - 1 && at.virt2 && at.pos == k - 1 && at.half == k / 2 && !at.bye, "last pair of a wide round");
    }
    printf("find ok %zu\n", nplans);
    return 0;
}
