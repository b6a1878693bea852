// conv2d_check.cpp -- walks mpyc_amd/csrc/conv2d_geom.hpp on the host exactly as k_conv2d does (block -> tile, thread ->
// pixel and channels, staging loops, term loops, flush schedule) on small integers modulo a small prime, against the plain
// seven-deep loop.  Checks: every output has exactly one owner (workgroup, thread, register); every (output, term) pair is
// visited exactly once; halo slots hold zero and only they; an accumulator never holds more than FLUSH unreduced terms,
// for FLUSH = 32 and 192 and every s in 1..16; the staged slots lie inside the LDS bytes the plan reports, which lie inside
// the limit; both tile shapes.  Prints "conv2d ok <launches walked>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mpyc_amd/csrc/conv2d_geom.hpp"

using namespace ffgpu;

static const long P = 251;
static long fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (fails++ < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
        }                                                               \
    } while (0)

static unsigned long long rs = 88172645463325252ull;
static long rnd(long n) {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return (long)(rs % (unsigned long long)n);
}

struct Case {
    size_t k, r, m, n, v;
    int s;
};

// one launch, as the kernel runs it; returns false if the plan refuses
static bool walk(const Case& c, int nsend, int wide_per_cu, size_t slot_bytes, int flush, bool bias) {
    const Conv2dPlan pl = conv2d_plan(c.k, c.r, c.m, c.n, c.v, c.s, nsend, 256, wide_per_cu, 8, slot_bytes, flush);
    if (!pl.ok || pl.empty || !pl.grid_ok) return false;
    const Conv2dGeom& g = pl.g;
    const int s = c.s, ss = s * s;
    CHECK(pl.wide == (wide_per_cu == 0 ? 1 : 0) || wide_per_cu == 2);
    CHECK(g.TH == (pl.wide ? 16 : 8) && g.TW == 16 && g.VB == (pl.wide ? 4 : 2) && g.VR == (pl.wide ? 4 : 1));
    CHECK(g.TH * g.TW * (g.VB / g.VR) == 256);
    CHECK(g.WH == g.TH + s - 1 && g.WW == g.TW + s - 1 && g.CH >= 1 && (size_t)g.CH <= c.r && g.CH <= (int)CONV2D_MAX_CH);
    CHECK(pl.lds_bytes == conv2d_lds_bytes(g.TH, g.TW, g.VB, s, g.CH, slot_bytes) && pl.lds_bytes <= (size_t)CONV2D_LDS_LIMIT);
    CHECK(g.CH == 1 || pl.lds_bytes <= (size_t)CONV2D_LDS_STEP);
    CHECK(pl.flush_rows == flush / s && pl.flush_rows >= 1 && pl.flush_rows * s <= flush);
    CHECK(pl.grid_x == (uint64_t)c.k * g.tiles_y * g.tiles_x * g.vblocks && pl.grid_y == (unsigned)nsend);
    const size_t nx = c.k * c.r * c.m * c.n, nw = c.v * c.r * (size_t)ss, ny = c.k * c.v * c.m * c.n;
    std::vector<long> x(nx), w(nw), b(c.v), want(ny), got(ny, -1);
    for (auto& e : x) e = 1 + rnd(P - 1);                                   // nonzero: a zero slot is a halo slot
    for (auto& e : w) e = rnd(P);
    for (auto& e : b) e = rnd(P);
    const int ro = (s - 1) / 2, co = s / 2;
    for (size_t i = 0; i < c.k; ++i)
        for (size_t j = 0; j < c.v; ++j)
            for (size_t I = 0; I < c.m; ++I)
                for (size_t J = 0; J < c.n; ++J) {
                    long acc = bias ? b[j] : 0;
                    for (size_t l = 0; l < c.r; ++l)
                        for (int di = 0; di < s; ++di)
                            for (int dj = 0; dj < s; ++dj) {
                                const long row = (long)I + di - ro, col = (long)J + dj - co;
                                if (row >= 0 && row < (long)c.m && col >= 0 && col < (long)c.n)
                                    acc += x[((i * c.r + l) * c.m + (size_t)row) * c.n + (size_t)col] * w[(j * c.r + l) * ss + di * s + dj];
                            }
                    want[((i * c.v + j) * c.m + I) * c.n + J] = acc % P;
                }
    std::vector<int> owners(ny, 0);
    std::vector<unsigned char> seen(ny * c.r * (size_t)ss, 0);
    const size_t slots = pl.lds_bytes / slot_bytes;
    const int win_one = g.WH * g.WW, tap_one = g.VB * ss, win_all = g.CH * win_one;
    std::vector<long> lds(slots);
    const int VR = g.VR, period = conv2d_flush_rows(s, flush);
    for (unsigned blk = 0; blk < (unsigned)pl.grid_x; ++blk) {
        const Conv2dBlock bl = conv2d_block(g, blk);
        CHECK(bl.img < c.k && bl.I0 < c.m && bl.J0 < c.n && bl.j0 < c.v);
        std::vector<long> acc(256 * VR, 0), tot(256 * VR, 0);
        std::vector<int> unreduced(256, 0), rows_since(256, 0);
        for (size_t l0 = 0; l0 < c.r; l0 += (size_t)g.CH) {
            const int nch = c.r - l0 < (size_t)g.CH ? (int)(c.r - l0) : g.CH;
            for (auto& e : lds) e = -7;                                     // poison: a slot read must have been staged
            for (int i = 0; i < nch * win_one; ++i) {
                int cl, wy, wx;
                conv2d_win_of(g, i, cl, wy, wx);
                CHECK(conv2d_win_slot(g, cl, wy, wx) == i && (size_t)i < slots);
                const int64_t row = conv2d_win_row(bl.I0, wy, s), col = conv2d_win_col(bl.J0, wx, s);
                const bool ok = conv2d_in_image(row, col, c.m, c.n);
                CHECK(ok == (row >= 0 && row < (int64_t)c.m && col >= 0 && col < (int64_t)c.n));
                lds[i] = ok ? x[conv2d_x_index(g, bl.img, l0 + cl, (size_t)row, (size_t)col)] : 0;
                CHECK((lds[i] == 0) == !ok);
            }
            for (int i = 0; i < nch * tap_one; ++i) {
                int cl, ch, tap;
                conv2d_tap_of(g, i, cl, ch, tap);
                CHECK(conv2d_tap_slot(g, cl, ch, tap / s, tap % s) == i && (size_t)(win_all + i) < slots);
                const size_t j = bl.j0 + ch;
                lds[win_all + i] = j < c.v ? w[conv2d_w_index(g, j, l0 + cl, tap)] : 0;
            }
            for (int tid = 0; tid < 256; ++tid) {
                const Conv2dLane ln = conv2d_lane(g, tid);
                CHECK(ln.py >= 0 && ln.py < g.TH && ln.px >= 0 && ln.px < g.TW && ln.c0 >= 0 && ln.c0 + VR <= g.VB);
                const size_t I = bl.I0 + ln.py, J = bl.J0 + ln.px;
                for (int cl = 0; cl < nch; ++cl)
                    for (int di = 0; di < s; ++di) {
                        const int wrow = conv2d_win_slot(g, cl, ln.py + di, ln.px), trow = conv2d_tap_slot(g, cl, ln.c0, di, 0);
                        for (int dj = 0; dj < s; ++dj) {
                            CHECK(wrow + dj < nch * win_one && lds[wrow + dj] >= 0);
                            for (int u = 0; u < VR; ++u) {
                                const int ts = trow + u * ss + dj;
                                CHECK(ts < nch * tap_one && lds[win_all + ts] >= 0);
                                acc[tid * VR + u] += lds[win_all + ts] * lds[wrow + dj];
                                const size_t j = bl.j0 + ln.c0 + u;
                                if (I < c.m && J < c.n && j < c.v)
                                    ++seen[(conv2d_y_index(g, bl.img, j, I, J) * c.r + l0 + cl) * ss + di * s + dj];
                            }
                            ++unreduced[tid];
                            CHECK(unreduced[tid] <= flush);
                        }
                        if (++rows_since[tid] == period) {
                            for (int u = 0; u < VR; ++u) {
                                tot[tid * VR + u] = (tot[tid * VR + u] + acc[tid * VR + u]) % P;
                                acc[tid * VR + u] = 0;
                            }
                            unreduced[tid] = rows_since[tid] = 0;
                        }
                    }
            }
        }
        for (int tid = 0; tid < 256; ++tid) {
            const Conv2dLane ln = conv2d_lane(g, tid);
            const size_t I = bl.I0 + ln.py, J = bl.J0 + ln.px;
            for (int u = 0; u < VR; ++u) {
                const size_t j = bl.j0 + ln.c0 + u;
                if (I < c.m && J < c.n && j < c.v) {
                    const size_t o = conv2d_y_index(g, bl.img, j, I, J);
                    CHECK(o < ny);
                    ++owners[o];
                    got[o] = (tot[tid * VR + u] + acc[tid * VR + u] + (bias ? b[j] : 0)) % P;
                }
            }
        }
    }
    for (size_t o = 0; o < ny; ++o) CHECK(owners[o] == 1 && got[o] == want[o]);
    for (auto e : seen) CHECK(e == 1);
    return true;
}

int main() {
    long launches = 0;
    // the flush schedule alone: every s, both bounds
    for (int flush : {32, 192})
        for (int s = 1; s <= (int)CONV2D_MAX_S; ++s) {
            const int period = conv2d_flush_rows(s, flush);
            CHECK(period >= 1 && period * s <= flush && (period + 1) * s > flush);
            CHECK(s * s <= flush || period < s);                        // the flush fires inside a channel
        }
    // refusals of the plan
    CHECK(!conv2d_plan(1, 1, 4, 4, 1, 0, 1, 256, 2, 8, 8, 192).ok && !conv2d_plan(1, 1, 4, 4, 1, 17, 1, 256, 2, 8, 8, 192).ok);
    CHECK(!conv2d_plan(1, 1, 4, 4, 1, 5, 1, 256, 2, 8, 8, 192).ok && conv2d_plan(1, 1, 2, 5, 1, 5, 1, 256, 2, 8, 8, 192).ok);
    CHECK(!conv2d_plan(1, 0, 4, 4, 1, 3, 1, 256, 2, 8, 8, 192).ok && !conv2d_plan(1, 1, 4, 4, 1, 3, 0, 256, 2, 8, 8, 192).ok);
    CHECK(conv2d_plan(0, 1, 4, 4, 1, 3, 1, 256, 2, 8, 8, 192).empty && conv2d_plan(1, 0, 4, 4, 0, 3, 1, 256, 2, 8, 8, 192).ok);
    CHECK(!conv2d_plan((size_t)1 << 62, 4, 4, 4, 1, 3, 1, 256, 2, 8, 8, 192).ok);
    CHECK(!conv2d_plan((size_t)1 << 40, 1, 16, 16, 4, 1, 1, 256, 2, 1, 8, 192).grid_ok);
    // the shape switch: wide from num_cu * per_cu workgroups of the wide shape
    CHECK(!conv2d_plan(1, 1, 14, 14, 64, 5, 3, 256, 2, 8, 8, 192).wide && conv2d_plan(64, 1, 28, 28, 32, 5, 3, 256, 2, 8, 8, 192).wide);
    CHECK(conv2d_use_wide(512, 1, 256, 2) && !conv2d_use_wide(511, 1, 256, 2) && conv2d_use_wide(171, 3, 256, 2));
    // the largest staging step fits for every slot size
    for (size_t slot : {4u, 8u, 16u, 24u, 28u})
        for (int wide = 0; wide < 2; ++wide)
            CHECK(conv2d_lds_bytes(wide ? 16 : 8, 16, wide ? 4 : 2, 16, 1, slot) <= (size_t)CONV2D_LDS_LIMIT);
    const Case cases[] = {
        {1, 1, 1, 1, 1, 1},   {2, 3, 5, 6, 2, 3},  {1, 2, 4, 5, 3, 4},  {1, 1, 3, 7, 1, 5},  {1, 2, 2, 6, 2, 6},
        {1, 1, 7, 15, 1, 2},  {1, 2, 8, 16, 4, 3}, {2, 1, 9, 17, 5, 3}, {1, 1, 15, 16, 1, 6}, {1, 1, 16, 17, 4, 16},
        {1, 2, 17, 33, 5, 1}, {1, 9, 3, 16, 2, 16}, {1, 11, 5, 5, 9, 5}, {1, 40, 2, 3, 1, 1},  {1, 3, 1, 16, 2, 16},
        {3, 5, 10, 9, 6, 4},
    };
    for (const Case& c : cases)
        for (int wide_per_cu : {0, 1 << 30})
            for (int flush : {32, 192})
                for (size_t slot : {8u, 28u}) launches += walk(c, 1 + (int)(c.k % 3), wide_per_cu, slot, flush, (c.s & 1) != 0);
    CHECK(launches == 16 * 2 * 2 * 2);
    if (fails) {
        printf("conv2d FAILED: %ld\n", fails);
        return 1;
    }
    printf("conv2d ok %ld\n", launches);
    return 0;
}
