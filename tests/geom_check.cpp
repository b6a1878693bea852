// geom_check.cpp -- walks mpyc_amd/csrc/geom.hpp on the host (g++, no HIP) against brute-force enumeration, for the five
// element sizes and both alignments:
//   * the size guard refuses element sizes 0, 2, 6 and 10, a wrapping product and count * eb above 2^62; accepts count = 0;
//   * the flat plan, n in 0..200: packs exactly when aligned, n != 0 and n a whole number of granules; total * pack == n; every
//     element in exactly one unit; whole waves for 24-byte packs;
//   * the rows plan, n in 0..200, rows 1..4, stride n..n+5: the span; packs exactly when the flat condition holds and every row
//     starts aligned; unit (j, g) covers element j * stride + g * pack + q exactly once; rows < 1 and stride < n refused;
//   * the stream plan, count in 0..200: nvec by the stated rule, tail, threads, whole waves for 24-byte elements, and
//     stream_nvec agrees;
//   * the reversed-row walk, n in 0..9, l in 1..64, with and without the top: rev_at is the closed form, rev_next applied q
//     times is rev_at(c + q), and the shift path, the 32-bit division and the 64-bit division agree;
//   * the pair split, row_units and run each of powers of two and non-powers, totals below and above 2^32 (synthetic sizes, no
//     memory): (o, c, b) == (g / row_units, g % row_units, c / run).
// Prints "geom ok <checks>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/geom.hpp"

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

static size_t nchecks = 0;
static const size_t EBS[5] = {4, 8, 12, 16, 24};
static const size_t TWO62 = (size_t)1 << 62;

static bool flat_packs(size_t n, size_t eb, bool aligned) { return aligned && n != 0 && n % (eb == 24 ? 64 : geom_pack(eb)) == 0; }

static void check_basics() {
    CHECK(GEOM_THREADS == 256 && GEOM_MAX_GRID == 0x7fffffff, "the workgroup and the grid limit");
    CHECK(geom_pack(4) == 4 && geom_pack(8) == 2 && geom_pack(12) == 1 && geom_pack(16) == 1 && geom_pack(24) == 1, "packs");
    CHECK(geom_gran(4) == 4 && geom_gran(8) == 2 && geom_gran(12) == 1 && geom_gran(16) == 1 && geom_gran(24) == 64, "granules");
    CHECK(geom_align(4) == 16 && geom_align(8) == 16 && geom_align(12) == 4 && geom_align(16) == 16 && geom_align(24) == 16, "alignment");
    for (size_t eb : EBS) CHECK(geom_pack(eb) * eb % geom_align(eb) == 0 || eb == 24, "a pack keeps the alignment: eb=%zu", eb);
    CHECK(64 * 24 % geom_align(24) == 0, "a wave of 24-byte elements keeps the alignment");
    size_t r;
    CHECK(geom_mul_ok(0, ~(size_t)0, r) && r == 0 && geom_mul_ok(~(size_t)0, 1, r) && r == ~(size_t)0, "products that fit");
    CHECK(geom_mul_ok((size_t)1 << 32, ((size_t)1 << 32) - 1, r) && !geom_mul_ok((size_t)1 << 32, (size_t)1 << 32, r), "2^64 wraps");
    CHECK(!geom_mul_ok(~(size_t)0, 2, r) && !geom_mul_ok(3, ~(size_t)0 / 3 + 1, r), "wrapping products");
    for (int s = 0; s < 64; ++s) {
        const size_t x = (size_t)1 << s;
        CHECK(geom_pow2(x) && geom_log2(x) == s, "2^%d", s);
        if (s >= 2) CHECK(!geom_pow2(x + 1) && !geom_pow2(x - 1), "neighbours of 2^%d", s);
    }
    CHECK(!geom_pow2(0), "zero is no power of two");
    ++nchecks;
}

static void check_guard() {
    for (size_t eb : {(size_t)0, (size_t)2, (size_t)6, (size_t)10})
        CHECK(!geom_size_ok(0, eb) && !geom_size_ok(5, eb) && !flat_plan(5, eb, true).ok && !rows_plan(5, 1, 5, eb, true).ok &&
                  !stream_plan(5, eb, true).ok && !rev_plan(5, 3, false, eb, true).ok,
              "element size %zu", eb);
    for (size_t eb : EBS) {
        CHECK(geom_size_ok(0, eb) && geom_size_ok(1, eb), "count = 0 and 1: eb=%zu", eb);
        CHECK(geom_size_ok(TWO62 / eb, eb) && !geom_size_ok(TWO62 / eb + 1, eb), "count * eb at and above 2^62: eb=%zu", eb);
        CHECK(!geom_size_ok(~(size_t)0 / eb + 1, eb) && !geom_size_ok(~(size_t)0, eb), "a wrapping product: eb=%zu", eb);
        CHECK(geom_bytes_ok(TWO62 / eb, eb) && !geom_bytes_ok(TWO62 / eb + 1, eb) && !geom_bytes_ok(~(size_t)0 / eb + 1, eb), "bytes: eb=%zu", eb);
        for (int al = 0; al < 2; ++al) {
            CHECK(flat_plan(TWO62 / eb, eb, al).ok && !flat_plan(TWO62 / eb + 1, eb, al).ok, "flat at the limit");
            CHECK(stream_plan(TWO62 / eb, eb, al).ok && !stream_plan(TWO62 / eb + 1, eb, al).ok, "stream at the limit");
            CHECK(!rows_plan(8, ~(size_t)0 / 4, 8, eb, al).ok && !rows_plan(8, 2, ~(size_t)0 - 3, eb, al).ok, "rows that wrap");
            CHECK(!rev_plan(~(size_t)0 / 3, 64, false, eb, al).ok && !rev_plan(TWO62 / eb, 2, true, eb, al).ok, "reversed rows that wrap");
        }
        ++nchecks;
    }
}

static void check_flat(size_t n, size_t eb, bool aligned) {
    const FlatPlan pl = flat_plan(n, eb, aligned);
    CHECK(pl.ok, "n=%zu eb=%zu", n, eb);
    CHECK((pl.vec != 0) == flat_packs(n, eb, aligned), "the pack decision: n=%zu eb=%zu aligned=%d", n, eb, (int)aligned);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == n, "units: n=%zu eb=%zu", n, eb);
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs go in whole waves: n=%zu", n);
    std::vector<int> seen(n, 0);
    for (size_t g = 0; g < pl.total; ++g)
        for (unsigned q = 0; q < pl.pack; ++q) ++seen[g * pl.pack + q];
    for (size_t e = 0; e < n; ++e) CHECK(seen[e] == 1, "element %zu in %d units", e, seen[e]);
    ++nchecks;
}

static void check_rows(size_t n, size_t rows, size_t stride, size_t eb, bool aligned) {
    const RowsPlan pl = rows_plan(n, rows, stride, eb, aligned);
    CHECK(pl.ok, "n=%zu rows=%zu stride=%zu eb=%zu", n, rows, stride, eb);
    CHECK(pl.span == (rows - 1) * stride + n, "span: n=%zu rows=%zu stride=%zu", n, rows, stride);
    bool rows_aligned = true;                   // every row starts where a pack may start, on a whole pack of the block
    for (size_t j = 0; j < rows; ++j) rows_aligned = rows_aligned && (j * stride * eb) % geom_align(eb) == 0 && (j * stride) % geom_pack(eb) == 0;
    CHECK((pl.vec != 0) == (flat_packs(n, eb, aligned) && rows_aligned), "the pack decision: n=%zu rows=%zu stride=%zu eb=%zu aligned=%d", n, rows,
          stride, eb, (int)aligned);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == n, "units: n=%zu stride=%zu", n, stride);
    CHECK(rows == 1 || pl.pitch * pl.pack == stride, "the pitch of more than one row: n=%zu stride=%zu", n, stride);
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs go in whole waves: n=%zu", n);
    std::vector<int> seen(pl.span, 0);
    for (size_t j = 0; j < rows; ++j)
        for (size_t g = 0; g < pl.total; ++g)
            for (unsigned q = 0; q < pl.pack; ++q) {
                const size_t e = rows_unit(pl, j, g) * pl.pack + q;
                CHECK(e == j * stride + g * pl.pack + q && e < pl.span, "unit (%zu, %zu)", j, g);
                ++seen[e];
            }
    for (size_t j = 0; j < rows; ++j)
        for (size_t i = 0; i < n; ++i) CHECK(seen[j * stride + i] == 1, "element (%zu, %zu) in %d units", j, i, seen[j * stride + i]);
    size_t hits = 0;
    for (int s : seen) hits += (size_t)s;
    CHECK(hits == rows * n, "nothing between the rows is touched");
    ++nchecks;
}

static void check_stream(size_t count, size_t eb, bool aligned) {
    const StreamPlan pl = stream_plan(count, eb, aligned);
    CHECK(pl.ok && pl.pack == geom_pack(eb), "count=%zu eb=%zu", count, eb);
    const size_t want = !aligned ? 0 : eb == 24 ? count / 64 * 64 : count / geom_pack(eb);
    CHECK(pl.nvec == want && stream_nvec(count, eb, aligned) == pl.nvec, "nvec: count=%zu eb=%zu aligned=%d", count, eb, (int)aligned);
    CHECK(pl.tail == pl.nvec * pl.pack && pl.tail <= count, "tail: count=%zu eb=%zu", count, eb);
    CHECK(pl.threads == (pl.nvec ? pl.nvec : count), "threads: count=%zu eb=%zu", count, eb);
    if (aligned && eb == 24) CHECK(pl.nvec % 64 == 0 && count - pl.nvec < 64, "24-byte packs: whole waves, a tail below one");
    if (aligned && eb != 24) CHECK(count - pl.tail < pl.pack, "every whole pack goes through the vector loop");
    ++nchecks;
}

static void check_rev(size_t n, size_t l, bool skip_top, size_t eb, bool aligned) {
    const RevPlan pl = rev_plan(n, l, skip_top, eb, aligned);
    const size_t l1 = skip_top ? l - 1 : l;
    CHECK(pl.ok && pl.l == l && pl.l1 == l1 && pl.elems == n * l1, "n=%zu l=%zu skip_top=%d eb=%zu", n, l, (int)skip_top, eb);
    CHECK((pl.vec != 0) == flat_packs(pl.elems, eb, aligned), "the pack decision: n=%zu l=%zu eb=%zu aligned=%d", n, l, eb, (int)aligned);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == pl.elems, "units: n=%zu l=%zu", n, l);
    CHECK(pl.shift == (geom_pow2(l1) ? geom_log2(l1) : -1) && pl.narrow == 1, "shift and narrow: l1=%zu", l1);
    RevPlan by32 = pl, by64 = pl;               // the same walk by the 32-bit and by the 64-bit division
    by32.shift = -1;
    by64.shift = -1;
    by64.narrow = 0;
    std::vector<int> seen(n * l, 0);
    for (size_t c = 0; c < pl.elems; ++c) {
        const RevAt at = rev_at(pl, c);
        const size_t h = c / l1, j = c % l1;
        CHECK(at.h == h && at.j == j && at.src == h * l + (l1 - 1 - j) && at.top == h * l + l1, "compact element %zu: n=%zu l=%zu", c, n, l);
        const RevAt a32 = rev_at(by32, c), a64 = rev_at(by64, c);
        CHECK(a32.h == h && a32.j == j && a32.src == at.src && a32.top == at.top, "the 32-bit division: c=%zu l1=%zu", c, l1);
        CHECK(a64.h == h && a64.j == j && a64.src == at.src && a64.top == at.top, "the 64-bit division: c=%zu l1=%zu", c, l1);
        RevAt walk = at;
        for (size_t q = 1; q <= 4 && c + q < pl.elems; ++q) {
            rev_next(pl, walk);
            const RevAt there = rev_at(pl, c + q);
            CHECK(walk.h == there.h && walk.j == there.j && walk.src == there.src && walk.top == there.top, "next x %zu from %zu: l=%zu", q, c, l);
        }
        ++seen[at.src];
        if (skip_top) CHECK(at.top == h * l + l - 1, "the top of row %zu", h);
    }
    for (size_t h = 0; h < n; ++h)
        for (size_t i = 0; i < l; ++i) CHECK(seen[h * l + i] == (i < l1 ? 1 : 0), "source (%zu, %zu) read %d times", h, i, seen[h * l + i]);
    ++nchecks;
}

struct SynthPlan {                              // what pair_fill / pair_split ask of a plan type
    size_t row_units, run, total;
    int run_shift, row_shift, narrow;
};
static void check_pair(size_t outer, size_t row_elems, size_t run_elems, size_t u) {
    SynthPlan pl = SynthPlan();
    pair_fill(pl, outer, row_elems, run_elems, u);
    CHECK(pl.row_units == row_elems / u && pl.run == run_elems / u && pl.total == outer * pl.row_units, "units: %zu %zu %zu %zu", outer, row_elems,
          run_elems, u);
    CHECK(pl.run_shift == (geom_pow2(pl.run) ? geom_log2(pl.run) : -1) && pl.row_shift == (geom_pow2(pl.row_units) ? geom_log2(pl.row_units) : -1),
          "shifts: row_units=%zu run=%zu", pl.row_units, pl.run);
    CHECK(pl.narrow == (pl.total <= 0xffffffffu && pl.run <= 0xffffffffu), "narrow: total=%zu", pl.total);
    SynthPlan by_div = pl;                      // the same split with no shift: the division the plan's `narrow` selects
    by_div.run_shift = by_div.row_shift = -1;
    const size_t gs[] = {0, 1, pl.run - 1, pl.run, pl.run + 1, pl.row_units - 1, pl.row_units, pl.row_units + 1, pl.total / 3, pl.total / 2,
                         0xffffffffu, (size_t)1 << 32, ((size_t)1 << 32) + 12345, pl.total - 2, pl.total - 1};
    for (size_t g : gs) {
        if (g >= pl.total) continue;
        const PairAt at = pair_split(pl, g), ad = pair_split(by_div, g);
        const size_t o = g / pl.row_units, c = g % pl.row_units, b = c / pl.run;
        CHECK(at.o == o && at.c == c && at.b == b, "g=%zu row_units=%zu run=%zu", g, pl.row_units, pl.run);
        CHECK(ad.o == o && ad.c == c && ad.b == b, "g=%zu row_units=%zu run=%zu by division", g, pl.row_units, pl.run);
    }
    for (size_t g = 0; g < pl.total && g < 4096; ++g) {
        const PairAt at = pair_split(pl, g);
        CHECK(at.o == g / pl.row_units && at.c == g % pl.row_units && at.b == at.c / pl.run, "g=%zu row_units=%zu run=%zu", g, pl.row_units, pl.run);
    }
    ++nchecks;
}

int main() {
    check_basics();
    check_guard();
    for (size_t eb : EBS)
        for (int al = 0; al < 2; ++al) {
            for (size_t n = 0; n <= 200; ++n) {
                check_flat(n, eb, al != 0);
                check_stream(n, eb, al != 0);
                for (size_t rows = 1; rows <= 4; ++rows)
                    for (size_t stride = n; stride <= n + 5; ++stride) check_rows(n, rows, stride, eb, al != 0);
                CHECK(!rows_plan(n, 0, n, eb, al != 0).ok, "rows < 1");
                if (n > 0) CHECK(!rows_plan(n, 1, n - 1, eb, al != 0).ok && !rows_plan(n, 3, 0, eb, al != 0).ok, "stride < n");
            }
            for (size_t n = 0; n <= 9; ++n)
                for (size_t l = 1; l <= 64; ++l)
                    for (int skip = 0; skip < 2; ++skip) check_rev(n, l, skip != 0, eb, al != 0);
            CHECK(!rev_plan(4, 0, false, eb, al != 0).ok && !rev_plan(4, 0, true, eb, al != 0).ok, "l < 1");
            // a compact array past 2^32 elements: the 64-bit division, and the shift
            for (size_t l : {(size_t)33, (size_t)32}) {
                const size_t n = ((size_t)1 << 32) / l + 7;
                const RevPlan pl = rev_plan(n, l, false, eb, al != 0);
                CHECK(pl.ok && !pl.narrow && pl.elems == n * l, "a wide plan: l=%zu", l);
                for (size_t c : {(size_t)0, (size_t)0xffffffffu, (size_t)1 << 32, pl.elems - 1}) {
                    const RevAt at = rev_at(pl, c);
                    CHECK(at.h == c / l && at.j == c % l && at.src == at.h * l + (l - 1 - at.j), "c=%zu of a wide plan", c);
                }
            }
        }
    // the pair split: row_units and run each a power of two and not, units of 1, 2 and 4 elements, totals on both sides of 2^32
    for (size_t u : {(size_t)1, (size_t)2, (size_t)4})
        for (size_t run_units : {(size_t)1, (size_t)4, (size_t)5, (size_t)64, (size_t)96, (size_t)1 << 20, ((size_t)1 << 20) + 3})
            for (size_t runs : {(size_t)1, (size_t)2, (size_t)3, (size_t)8, (size_t)13})
                for (size_t outer : {(size_t)1, (size_t)3, (size_t)1 << 10, ((size_t)1 << 32) / (run_units * runs) + 5, (size_t)1 << 33}) {
                    size_t t1, t2;
                    if (!geom_mul_ok(run_units * runs * u, outer, t1) || !geom_mul_ok(t1, 24, t2) || t2 > TWO62) continue;
                    check_pair(outer, run_units * runs * u, run_units * u, u);
                }
    {   // both sides of 2^32 were met
        SynthPlan lo = SynthPlan(), hi = SynthPlan();
        pair_fill(lo, 3, 96 * 13, 96, 1);
        pair_fill(hi, (size_t)1 << 33, 5 * 3, 5, 1);
        CHECK(lo.narrow && lo.run_shift < 0 && lo.row_shift < 0 && !hi.narrow && hi.total > 0xffffffffu, "narrow and wide synthetic plans");
    }
    printf("geom ok %zu\n", nchecks);
    return 0;
}
