// explog_check.cpp -- walks mpyc_amd/csrc/explog_geom.hpp on the host (g++, no HIP) against brute-force enumeration, for five
// element sizes and both alignments:
//   * the row plan of powers_prod / poly_dot (rows_plan / rows_unit): for n in {1, 2, 63, 64, 65, 257, 5003}, rows
//     in {1, 2, 3, 21, 64} and strides n, n + 3 and n + 64, the units of every row cover its n elements once, every element a
//     unit touches lies inside row j of the block, and (row, element) pairs are hit exactly once; packs only on aligned
//     pointers with an aligned pitch, whole waves for 24-byte elements;
//   * the reversed index of bits_reverse (explog_rev_plan with rev_at / rev_next): l in 1..64, every (h, j) is owned
//     once and reads bits[h l + l-1-j], no source falls outside n * l;
//   * the windows of pow_base (pow_base_plan / pow_base_digit / pow_base_slot): for random three-limb integers, shifts and bit
//     counts, the digits are those of ((x >> shift) mod 2^ebits) in base 16, every window index and every table slot is in
//     range;
//   * counts out of range and overflowing sizes are refused.
// Prints "explog ok <plans>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mpyc_amd/csrc/explog_geom.hpp"

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

static void check_rows(size_t n, size_t rows, size_t stride, size_t eb, bool aligned) {
    const RowsPlan pl = rows_plan(n, rows, stride, eb, aligned);
    const size_t gran = geom_gran(eb);
    CHECK(pl.ok && pl.span == (rows - 1) * stride + n, "n=%zu rows=%zu stride=%zu", n, rows, stride);
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    const bool pitch_ok = rows == 1 || ((stride * eb) % geom_align(eb) == 0 && stride % geom_pack(eb) == 0);
    if (aligned) CHECK(pl.vec == (n % gran == 0 && pitch_ok), "pack decision n=%zu stride=%zu eb=%zu", n, stride, eb);
    CHECK(pl.pack == (pl.vec ? geom_pack(eb) : 1u) && pl.total * pl.pack == n, "loop length");
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs: whole waves");
    if (pl.vec && rows > 1) CHECK(pl.pitch * pl.pack == stride, "the pitch is the stride in units");
    std::vector<int> seen(rows * n, 0);
    for (size_t j = 0; j < rows; ++j)
        for (size_t g = 0; g < pl.total; ++g) {
            const size_t u = rows_unit(pl, j, g);
            for (unsigned q = 0; q < pl.pack; ++q) {
                const size_t e = u * pl.pack + q;                          // element of the block
                CHECK(e >= j * stride && e < j * stride + n && e < pl.span, "unit (%zu, %zu) leaves its row", j, g);
                ++seen[j * n + (e - j * stride)];
            }
        }
    for (size_t i = 0; i < rows * n; ++i) CHECK(seen[i] == 1, "(row, element) %zu hit %d times", i, seen[i]);
    ++nplans;
}

static void check_rev(size_t n, int l, size_t eb, bool aligned) {
    const RevPlan pl = explog_rev_plan(n, l, eb, aligned);
    const size_t L = (size_t)l, elems = n * L, gran = geom_gran(eb);
    CHECK(pl.ok && pl.l == L && pl.l1 == L && pl.elems == elems, "n=%zu l=%d", n, l);
    if (!aligned) CHECK(!pl.vec, "packs on unaligned pointers");
    else CHECK(pl.vec == (elems % gran == 0), "pack decision n=%zu l=%d eb=%zu", n, l, eb);
    CHECK(pl.total * pl.pack == elems, "loop length");
    if (pl.vec && eb == 24) CHECK(pl.total % 64 == 0, "24-byte packs: whole waves");
    std::vector<int> seen_c(elems, 0), seen_src(elems, 0);
    for (size_t g = 0; g < pl.total; ++g) {
        RevAt at = rev_at(pl, g * pl.pack);
        for (unsigned q = 0; q < pl.pack; ++q) {
            const size_t c = g * pl.pack + q;
            CHECK(at.h == c / L && at.j == c % L && at.h < n, "c=%zu -> (h, j)", c);
            CHECK(at.src == at.h * L + (L - 1 - at.j) && at.src < elems, "source of c=%zu", c);
            ++seen_c[c];
            ++seen_src[at.src];
            rev_next(pl, at);
        }
    }
    for (size_t c = 0; c < elems; ++c) CHECK(seen_c[c] == 1 && seen_src[c] == 1, "element %zu written %d, read %d times", c, seen_c[c], seen_src[c]);
    ++nplans;
}

static uint64_t rnd_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rnd_state ^= rnd_state << 13;
    rnd_state ^= rnd_state >> 7;
    rnd_state ^= rnd_state << 17;
    return rnd_state;
}

// bit b of the three-limb integer
static unsigned bit_of(const uint64_t x[3], int b) { return b < 192 ? (unsigned)((x[b >> 6] >> (b & 63)) & 1u) : 0u; }

static void check_pow(int shift, int ebits, int pbits, size_t eb) {
    const PowBasePlan pl = pow_base_plan(7, shift, ebits, pbits, eb);
    CHECK(pl.ok && pl.nwin == (ebits + 3) / 4 && pl.tab_elems == 15 * pl.nwin, "shift=%d ebits=%d", shift, ebits);
    CHECK(pl.nwin >= 1 && pl.nwin <= pow_base_max_windows(eb), "windows fit the LDS table of the element size");
    for (int rep = 0; rep < 24; ++rep) {
        uint64_t x[3] = {rnd(), eb > 8 ? rnd() : 0, eb > 16 ? rnd() : 0};
        if (eb == 4) x[0] &= 0xffffffffu;
        if (eb == 12) x[1] &= 0xffffffffu;
        if (rep == 0) x[0] = x[1] = x[2] = 0;
        if (rep == 1) { x[0] = ~0ull; x[1] = eb > 8 ? ~0ull : 0; x[2] = eb > 16 ? ~0ull : 0; }
        for (int i = 0; i < pl.nwin; ++i) {
            const unsigned d = pow_base_digit(pl, x[0], x[1], x[2], i);
            unsigned want = 0;
            for (int k = 0; k < 4; ++k)
                if (4 * i + k < ebits) want |= bit_of(x, shift + 4 * i + k) << k;
            CHECK(d == want && d <= 15, "digit %d of shift=%d ebits=%d: %u, expected %u", i, shift, ebits, d, want);
            if (d) CHECK(pow_base_slot(i, d) >= 0 && pow_base_slot(i, d) < pl.tab_elems, "slot out of the table");
        }
    }
    CHECK(pow_base_slot(0, 1) == 0 && pow_base_slot(pl.nwin - 1, 15) == pl.tab_elems - 1, "first and last slot");
    ++nplans;
}

int main() {
    const size_t ebs[] = {4, 8, 12, 16, 24}, ns[] = {1, 2, 63, 64, 65, 257, 5003}, rws[] = {1, 2, 3, 21, 64};
    const int pbits_of[] = {31, 61, 80, 127, 192};
    for (int k = 0; k < 5; ++k) {
        const size_t eb = ebs[k];
        for (int al = 0; al < 2; ++al) {
            for (size_t n : ns) {
                for (size_t rows : rws)
                    for (size_t pad : {(size_t)0, (size_t)3, (size_t)64}) check_rows(n, rows, n + pad, eb, al != 0);
                if (n <= 257)
                    for (int l = 1; l <= 64; ++l) check_rev(n, l, eb, al != 0);
            }
            check_rev(5003, 33, eb, al != 0);
        }
        const int pb = pbits_of[k];
        for (int ebits = 1; ebits <= pb; ++ebits)
            for (int shift : {0, 1, 3, 16, 60, 61, 63, 64, 127, 191}) check_pow(shift, ebits, pb, eb);
        CHECK(!pow_base_plan(5, 0, 0, pb, eb).ok && !pow_base_plan(5, 0, pb + 1, pb, eb).ok, "ebits out of range");
        CHECK(!pow_base_plan(5, -1, 4, pb, eb).ok && !pow_base_plan(5, 192, 4, pb, eb).ok, "shift out of range");
    }
    // refused
    CHECK(!explog_prod_valid(0, 1) && !explog_prod_valid(3, 0) && !explog_prod_valid(3, 4) && explog_prod_valid(3, 3), "h, w");
    CHECK(!explog_poly_valid(0) && !explog_poly_valid(65) && explog_poly_valid(1) && explog_poly_valid(64), "theta");
    CHECK(!rows_plan(5, 0, 5, 8, true).ok && !rows_plan(5, 2, 4, 8, true).ok && !rows_plan(5, 2, 5, 6, true).ok, "rows, stride, element size");
    CHECK(!rows_plan((size_t)1 << 60, 64, (size_t)1 << 60, 8, true).ok && !rows_plan((size_t)1 << 61, 1, (size_t)1 << 61, 24, true).ok, "sizes overflow");
    CHECK(!explog_rev_plan(5, 0, 8, true).ok && !explog_rev_plan(5, 65, 8, true).ok && !explog_rev_plan((size_t)1 << 58, 64, 8, true).ok, "l, n * l");
    CHECK(!pow_base_plan((size_t)1 << 61, 0, 4, 61, 8).ok && !pow_base_plan(5, 0, 4, 65, 8).ok, "n * eb, modulus wider than the element");
    CHECK(rows_plan(0, 3, 0, 8, true).ok && rows_plan(0, 3, 0, 8, true).total == 0 && explog_rev_plan(0, 7, 8, true).total == 0, "empty");
    printf("explog ok %zu\n", nplans);
    return 0;
}
