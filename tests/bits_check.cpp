// bits_check.cpp -- host walk of mpyc_amd/csrc/bits_geom.hpp (g++ -Wall -Wextra -Werror, no HIP): for l = 1..64 the rounds
// of the prefix-carry network against the reference's recursion restated here and against true carries of random bit
// vectors; the k of a round distinct, no q among them, every merge's inputs final before its round; and the launch plan
// of the two level kernels owning every compact element and every touched row element exactly once, for the five element
// sizes with n odd, even and a multiple of 64.  Prints "bits ok <total product rows>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mpyc_amd/csrc/bits_geom.hpp"

using namespace ffgpu;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

struct Merge {
    int i, h, j, high;
};
static int height(int n) {
    int r = 0;
    while ((1 << r) < n) ++r;
    return r;
}
// runtime.py:4307-4327, the merges only
static void recurse(int i, int j, int high, std::vector<Merge>& out) {
    const int n = j - i;
    if (n == 1) return;
    const int h = i + n / 2;
    recurse(i, h, high, out);
    recurse(h, j, 1, out);
    out.push_back({i, h, j, high});
}
// the reference's recursion on integers: prefix carries c (and propagates d when high)
static void ref_carries(const std::vector<int>& a, const std::vector<int>& b, int i, int j, bool high, std::vector<long>& c,
                        std::vector<long>& d) {
    const int n = j - i;
    if (n == 1) {
        c[i] = a[i] * b[i];
        if (high) d[i] = a[i] + b[i] - 2 * c[i];
        return;
    }
    const int h = i + n / 2;
    ref_carries(a, b, i, h, high, c, d);
    ref_carries(a, b, h, j, true, c, d);
    for (int k = h; k < j; ++k) c[k] += c[h - 1] * d[k];
    if (high)
        for (int k = h; k < j; ++k) d[k] *= d[h - 1];
}

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 20);
}

static long check_network(int l) {
    std::vector<Merge> ms;
    recurse(0, l, 0, ms);
    const int rounds = bits_rounds(l);
    CHECK(rounds == height(l));
    BitsLevel lv;
    CHECK(!bits_level(l, 0, lv) && !bits_level(l, rounds + 1, lv) && !bits_level(l, -1, lv));
    long total = 0;
    std::vector<BitsLevel> levels;
    for (int rho = 1; rho <= rounds; ++rho) {
        CHECK(bits_level(l, rho, lv));
        levels.push_back(lv);
        // the expected rows from the restated recursion, left to right
        std::vector<int> ck, cq, dk, dq;
        for (int pos = 0; pos < l; ++pos)                 // merges of a round are disjoint: order them by i
            for (const Merge& m : ms)
                if (m.i == pos && height(m.j - m.i) == rho) {
                    // every merge's inputs are final before its round: both children are merged in earlier rounds
                    CHECK(height(m.h - m.i) < rho && height(m.j - m.h) < rho);
                    for (int k = m.h; k < m.j; ++k) {
                        ck.push_back(k), cq.push_back(m.h - 1);
                        if (m.high) dk.push_back(k), dq.push_back(m.h - 1);
                    }
                }
        CHECK((size_t)lv.rc == ck.size() && (size_t)lv.rd == dk.size());
        CHECK(lv.rc >= 1 && lv.rd <= lv.rc && lv.rc + lv.rd <= BITS_MAX_ROWS);
        for (int j = 0; j < lv.rc; ++j) CHECK(lv.k[j] == ck[j] && lv.q[j] == cq[j]);
        for (int j = 0; j < lv.rd; ++j) CHECK(lv.k[lv.rc + j] == dk[j] && lv.q[lv.rc + j] == dq[j]);
        // k distinct (within the c-rows and within the d-rows) and ascending, no q among the k
        std::vector<int> is_k(l, 0);
        for (int j = 0; j < lv.rc; ++j) {
            CHECK(!is_k[lv.k[j]] && (j == 0 || lv.k[j] > lv.k[j - 1]));
            is_k[lv.k[j]] = 1;
        }
        for (int j = 0; j < lv.rd; ++j) {
            CHECK(is_k[lv.k[lv.rc + j]] && (j == 0 || lv.k[lv.rc + j] > lv.k[lv.rc + j - 1]));
        }
        for (int j = 0; j < lv.rc + lv.rd; ++j) CHECK(lv.q[j] < l && lv.k[j] < l && !is_k[lv.q[j]]);
        total += lv.rc + lv.rd;
    }
    // the schedule computes the reference's carries, and those are the true carries
    for (int rep = 0; rep < 20; ++rep) {
        std::vector<int> a(l), b(l);
        for (int k = 0; k < l; ++k) a[k] = rnd() & 1, b[k] = rnd() & 1;
        if (rep == 0)
            for (int k = 0; k < l; ++k) a[k] = 1, b[k] = k == 0;       // one carry through every position
        std::vector<long> G(l), P(l), c(l), d(l);
        for (int k = 0; k < l; ++k) G[k] = a[k] * b[k], P[k] = a[k] + b[k] - 2 * a[k] * b[k];
        for (const BitsLevel& v : levels) {
            std::vector<long> prod(v.rc + v.rd);
            for (int j = 0; j < v.rc; ++j) prod[j] = G[v.q[j]] * P[v.k[j]];
            for (int j = 0; j < v.rd; ++j) prod[v.rc + j] = P[v.q[v.rc + j]] * P[v.k[v.rc + j]];
            for (int j = 0; j < v.rc; ++j) G[v.k[j]] += prod[j];
            for (int j = 0; j < v.rd; ++j) P[v.k[v.rc + j]] = prod[v.rc + j];
        }
        ref_carries(a, b, 0, l, false, c, d);
        int cy = 0;
        for (int k = 0; k < l; ++k) {
            cy = (a[k] + b[k] + cy) >> 1;
            CHECK(G[k] == c[k] && G[k] == cy);
        }
    }
    return total;
}

// the two level kernels' loops, walked for every workgroup and thread of the grid
static void check_plan(size_t n, int l, const BitsLevel& lv, size_t eb, bool aligned, size_t max_blocks) {
    const int R = lv.rc + lv.rd;
    const BitsPlan pl = bits_plan(n, l, R, eb, aligned, max_blocks);
    CHECK(pl.ok && pl.rows == R);
    if (R == 0 || n == 0) return;
    const size_t u = pl.vec ? geom_pack(eb) : 1;
    CHECK(pl.gx >= 1 && (size_t)pl.gx * (size_t)R <= (max_blocks > (size_t)R ? max_blocks : (size_t)R));
    if (pl.vec) {
        CHECK(aligned && n % geom_gran(eb) == 0 && (n * eb) % geom_align(eb) == 0 && pl.row_units * u == n);
        if (eb == 24) CHECK(pl.row_units % 64 == 0);      // every wave of the loop entirely in or out
    } else {
        CHECK(pl.row_units == n);
    }
    std::vector<int> compact((size_t)R * n, 0), g((size_t)l * n, 0), p((size_t)l * n, 0), rdg((size_t)l * n, 0), rdp((size_t)l * n, 0);
    for (int y = 0; y < R; ++y)
        for (unsigned bx = 0; bx < pl.gx; ++bx)
            for (unsigned t = 0; t < (unsigned)GEOM_THREADS; ++t)
                for (size_t x = (size_t)bx * GEOM_THREADS + t; x < pl.row_units; x += (size_t)pl.gx * GEOM_THREADS) {
                    const size_t c = bits_unit(pl, y, x), at = bits_unit(pl, lv.k[y], x), qa = bits_unit(pl, lv.q[y], x);
                    if (pl.vec && (eb != 24 || x % 64 == 0))      // (24 bytes: the wave's 64 elements start aligned)
                        CHECK((c * u * eb) % geom_align(eb) == 0 && (at * u * eb) % geom_align(eb) == 0 && (qa * u * eb) % geom_align(eb) == 0);
                    for (size_t e = 0; e < u; ++e) {
                        CHECK(c * u + e < (size_t)R * n && at * u + e < (size_t)l * n && qa * u + e < (size_t)l * n);
                        ++compact[c * u + e];
                        ++(y < lv.rc ? g : p)[at * u + e];                 // what carry_apply writes
                        ++(y < lv.rc ? rdg : rdp)[qa * u + e];             // what carry_prod reads on the left
                        CHECK(at * u + e == (size_t)lv.k[y] * n + (x * u + e) && c * u + e == (size_t)y * n + (x * u + e));
                    }
                }
    for (int v : compact) CHECK(v == 1);
    std::vector<int> kc(l, 0), kd(l, 0), qc(l, 0), qd(l, 0);
    for (int y = 0; y < R; ++y) ++(y < lv.rc ? kc : kd)[lv.k[y]], ++(y < lv.rc ? qc : qd)[lv.q[y]];
    for (int r = 0; r < l; ++r)
        for (size_t h = 0; h < n; ++h) {
            CHECK(g[(size_t)r * n + h] == kc[r] && p[(size_t)r * n + h] == kd[r] && kc[r] <= 1 && kd[r] <= 1);
            CHECK(rdg[(size_t)r * n + h] == qc[r] && rdp[(size_t)r * n + h] == qd[r]);
        }
}

int main() {
    static const int want[][4] = {{2, 1, 1, 0}, {3, 2, 3, 1}, {7, 3, 11, 5}, {8, 3, 12, 5}, {16, 4, 32, 17}, {32, 5, 80, 49},
                                  {33, 6, 86, 54}, {64, 6, 192, 129}};
    long total = 0;
    for (int l = 1; l <= 64; ++l) total += check_network(l);
    for (const auto& w : want) {
        int rc = 0, rd = 0, widest = 0;
        CHECK(bits_rounds(w[0]) == w[1]);
        for (int rho = 1; rho <= w[1]; ++rho) {
            BitsLevel lv;
            CHECK(bits_level(w[0], rho, lv));
            rc += lv.rc, rd += lv.rd;
            if (lv.rc + lv.rd > widest) widest = lv.rc + lv.rd;
        }
        CHECK(rc == w[2] && rd == w[3] && widest == (w[0] == 33 ? 31 : w[0] - 1));
    }
    CHECK(bits_rounds(1) == 0 && bits_rounds(0) == -1 && bits_rounds(65) == -1 && bits_rounds(-3) == -1);
    static const size_t ebs[] = {4, 8, 12, 16, 24}, ns[] = {1, 2, 7, 63, 64, 66, 128, 257, 1000, 1024 + 64};
    for (size_t eb : ebs)
        for (int l : {2, 3, 7, 16, 33, 64})
            for (int rho = 1; rho <= bits_rounds(l); ++rho) {
                BitsLevel lv;
                CHECK(bits_level(l, rho, lv));
                for (size_t n : ns) {
                    check_plan(n, l, lv, eb, true, (size_t)GEOM_MAX_GRID);
                    check_plan(n, l, lv, eb, false, (size_t)GEOM_MAX_GRID);
                    check_plan(n, l, lv, eb, true, 70);                    // a capped grid: threads take several units
                    check_plan(n, l, lv, eb, true, 1);
                }
            }
    // sizes that overflow, and arguments out of range
    CHECK(!bits_plan((size_t)1 << 62, 16, 3, 8, true, 100).ok && !bits_plan((size_t)1 << 58, 64, 3, 24, true, 100).ok);
    CHECK(!bits_plan(10, 0, 1, 8, true, 100).ok && !bits_plan(10, 65, 1, 8, true, 100).ok && !bits_plan(10, 8, 64, 8, true, 100).ok);
    CHECK(!bits_plan(10, 8, 1, 6, true, 100).ok && bits_plan(0, 8, 3, 8, true, 100).ok && bits_plan(10, 8, 0, 8, true, 100).ok);
    std::printf("bits ok %ld\n", total);
    return 0;
}
