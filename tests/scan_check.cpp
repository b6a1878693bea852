// scan_check.cpp -- host walk of the scan / axis-reduction geometry (mpyc_amd/csrc/scan_geom.hpp), built with g++ by
// tests/test_scan_host.py.  For many (outer, k, inner), every element size, both geometries (packs and single elements
// for the column walk) and several tile sizes it replays the index arithmetic the kernels use and checks that
//   * every input element is owned by exactly one thread slot, and that slot decodes to the element's own (o, j, i);
//   * every output element (k + 1 entries along the axis with the initial, one for a reduction) is written exactly once;
//   * row tiles of a line follow each other in order (tile t starts where tiles 0 .. t-1 end), their workspace slots are
//     distinct and inside the plan's ws_elems, and ws_elems is what ffgpu_scan_workspace_bytes reports (the plan's);
//   * the three passes (tile aggregates, exclusive scan of the aggregates in chunks of a workgroup, tile scan with the
//     carry-in) and the column walk give the prefix sums of a plain loop, on 64-bit wrap-around sums of random values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mpyc_amd/csrc/scan_geom.hpp"

using namespace ffgpu;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            std::printf("FAIL %s line %d: outer %zu k %zu inner %zu eb %zu geom %d tt %d aligned %d\n", #cond, __LINE__, \
                        outer, k, inner, eb, geom, tt, (int)aligned);                                            \
            return false;                                                                                        \
        }                                                                                                        \
    } while (0)

static bool walk(size_t outer, size_t k, size_t inner, size_t eb, int geom, int tt, bool aligned, int wi) {
    const ScanPlan p = scan_plan(outer, k, inner, eb, aligned, 256, geom, tt, wi);
    CHECK(p.ok && p.geom == geom);
    const size_t n = outer * k * inner, kk = k + (size_t)wi, nout = outer * kk * inner;
    CHECK(p.lines == outer * inner);
    std::vector<uint64_t> a(n), want(nout), got(nout, 0), red(outer * inner, 0);
    std::vector<int> seen(n, 0), wrote(nout, 0), wrote_red(outer * inner, 0);
    for (auto& x : a) x = rnd();
    for (size_t o = 0; o < outer; ++o)
        for (size_t i = 0; i < inner; ++i) {
            uint64_t run = 0;
            if (wi) want[(o * kk) * inner + i] = 0;
            for (size_t j = 0; j < k; ++j) {
                run += a[(o * k + j) * inner + i];
                want[(o * kk + j + wi) * inner + i] = run;
            }
        }
    if (geom == SCAN_COLS) {
        CHECK(p.ws_elems == 0);
        const size_t epv = p.vec ? (size_t)scan_epv(eb) : 1;
        CHECK(p.per * epv == inner && p.units == outer * p.per);
        CHECK(!p.vec || (aligned && inner % epv == 0));
        for (size_t u = 0; u < p.units; ++u) {
            size_t o, c;
            scan_col_of(u, p.per, o, c);
            CHECK(o < outer && c < p.per);
            for (size_t q = 0; q < epv; ++q) {
                uint64_t run = 0;
                if (wi) {
                    const size_t e = scan_col_index(o, c, 0, kk, p.per) * epv + q;
                    CHECK(e < nout);
                    wrote[e]++;
                    got[e] = 0;
                }
                for (size_t j = 0; j < k; ++j) {
                    const size_t e = scan_col_index(o, c, j, k, p.per) * epv + q;
                    CHECK(e < n && e == (o * k + j) * inner + c * epv + q);
                    seen[e]++;
                    run += a[e];
                    const size_t w = scan_col_index(o, c, j + wi, kk, p.per) * epv + q;
                    CHECK(w < nout);
                    wrote[w]++;
                    got[w] = run;
                }
                const size_t r = scan_col_index(o, c, 0, 1, p.per) * epv + q;
                CHECK(r < outer * inner && r == o * inner + c * epv + q);
                wrote_red[r]++;
                red[r] = run;
            }
        }
    } else {
        const int items = scan_items(eb);
        CHECK(p.tile == (size_t)p.tt * items && p.ntiles == (k + p.tile - 1) / p.tile);
        CHECK(p.ws_elems == (p.ntiles > 1 ? p.lines * p.ntiles : 0));
        const size_t blocks = p.lines * p.ntiles;
        std::vector<uint64_t> ws(blocks, 0);
        std::vector<int> ws_hit(blocks, 0);
        // (A) tile aggregates
        for (size_t b = 0; b < blocks; ++b) {
            size_t line, t;
            scan_tile_of(b, p.ntiles, line, t);
            CHECK(line < p.lines && t < p.ntiles);
            const size_t base = scan_line_base(line, k, inner);
            size_t expect_j = t * p.tile;                       // tiles chain: tile t starts where t-1 ended
            uint64_t agg = 0;
            for (int tid = 0; tid < p.tt; ++tid) {              // (threads tt .. 255 of a workgroup hold nothing)
                if (scan_item_j(t, p.tile, tid, items, 0) >= k) break;   // (and so do those past the end of the line)
                for (int q = 0; q < items; ++q) {
                    const size_t j = scan_item_j(t, p.tile, tid, items, q);
                    if (j >= k) continue;
                    CHECK(j == expect_j);
                    ++expect_j;
                    const size_t e = base + j * inner;
                    CHECK(e < n && e == ((line / inner) * k + j) * inner + line % inner);
                    seen[e]++;
                    agg += a[e];
                }
            }
            CHECK(expect_j == (t + 1 < p.ntiles ? (t + 1) * p.tile : k));
            const size_t s = scan_ws_index(line, t, p.ntiles);
            CHECK(s < blocks && s == b && (p.ntiles == 1 || s < p.ws_elems));
            ws_hit[s]++;
            ws[s] = agg;
        }
        for (size_t s = 0; s < blocks; ++s) CHECK(ws_hit[s] == 1);
        // reduction: the fold of a line's aggregates; (B) exclusive scan of them, chunk after chunk
        for (size_t line = 0; line < p.lines; ++line) {
            uint64_t carry = 0;
            for (size_t c0 = 0; c0 < p.ntiles; c0 += SCAN_THREADS) {
                uint64_t excl = 0;
                for (size_t t = c0; t < c0 + SCAN_THREADS && t < p.ntiles; ++t) {
                    const size_t s = scan_ws_index(line, t, p.ntiles);
                    const uint64_t v = ws[s];
                    ws[s] = carry + excl;
                    excl += v;
                }
                carry += excl;
            }
            wrote_red[line]++;
            red[line] = carry;
        }
        // (C) tiles with their carry-in
        for (size_t b = 0; b < blocks; ++b) {
            size_t line, t;
            scan_tile_of(b, p.ntiles, line, t);
            const size_t obase = scan_line_base(line, kk, inner);
            uint64_t run = p.ntiles > 1 ? ws[b] : 0;
            if (wi && t == 0) {
                CHECK(obase < nout);
                wrote[obase]++;
                got[obase] = 0;
            }
            for (int tid = 0; tid < p.tt; ++tid) {
                if (scan_item_j(t, p.tile, tid, items, 0) >= k) break;
                for (int q = 0; q < items; ++q) {
                    const size_t j = scan_item_j(t, p.tile, tid, items, q);
                    if (j >= k) continue;
                    run += a[scan_line_base(line, k, inner) + j * inner];
                    const size_t w = obase + (j + wi) * inner;
                    CHECK(w < nout);
                    wrote[w]++;
                    got[w] = run;
                }
            }
        }
    }
    for (size_t e = 0; e < n; ++e) CHECK(seen[e] == 1);
    for (size_t e = 0; e < nout; ++e) CHECK(wrote[e] == 1 && got[e] == want[e]);
    for (size_t o = 0; o < outer; ++o)
        for (size_t i = 0; i < inner; ++i) {
            const size_t r = o * inner + i;
            CHECK(wrote_red[r] == 1 && red[r] == want[(o * kk + k - 1 + wi) * inner + i]);
        }
    return true;
}

int main() {
    const size_t outers[] = {1, 2, 3, 40};
    const size_t inners[] = {1, 2, 3, 4, 5, 15, 16, 17, 32, 33, 40};
    const size_t ebs[] = {1, 4, 8, 12, 24};
    const int tts[] = {1, 2, 3, 16, 64, 256};
    std::vector<size_t> ks;
    for (size_t k = 1; k <= 70; ++k) ks.push_back(k);
    for (size_t k : {127, 128, 129, 255, 256, 257, 300}) ks.push_back(k);
    size_t cases = 0;
    for (size_t outer : outers)
        for (size_t inner : inners)
            for (size_t k : ks)
                for (size_t eb : ebs) {
                    const int wi = (int)((outer + inner + k) & 1);
                    for (int aligned = 0; aligned < 2; ++aligned, ++cases)
                        if (!walk(outer, k, inner, eb, SCAN_COLS, 256, aligned != 0, wi)) return 1;
                    if (eb == 4 || eb == 12) continue;            // (row tiles know two element classes: <= 8 bytes, above)
                    for (int tt : tts) {
                        ++cases;
                        if (!walk(outer, k, inner, eb, SCAN_ROWS, tt, true, wi)) return 1;
                    }
                }
    // the chooser: forced settings are obeyed; left alone it takes columns only when they fill the device
    {
        const ScanPlan a = scan_plan(33, 1, 1000000, 12, true, 256, 0, 256), b = scan_plan(1, 10000000, 1, 8, true, 256, 0, 256),
                       c = scan_plan(1000000, 16, 1, 8, true, 256, 0, 256), d = scan_plan(4, 2500000, 1, 8, true, 256, 0, 256);
        // strided lines: few long ones take row tiles, lines shorter than a tile the column walk even when they are few
        const ScanPlan e = scan_plan(1, 64, 65536, 1, true, 256, 0, 256), g = scan_plan(1000000, 1, 3, 8, true, 256, 0, 256),
                       h = scan_plan(1, 1000000, 3, 8, true, 256, 0, 256);
        if (!(e.ok && e.geom == SCAN_COLS && g.ok && g.geom == SCAN_COLS && h.ok && h.geom == SCAN_ROWS && h.ws_elems == 3 * 245)) {
            std::printf("FAIL chooser (strided)\n");
            return 1;
        }
        if (!(a.ok && a.geom == SCAN_COLS && b.ok && b.geom == SCAN_ROWS && b.ws_elems == (10000000 + 4095) / 4096 &&
              c.ok && c.geom == SCAN_COLS && d.ok && d.geom == SCAN_ROWS && d.ws_elems * 256 <= 10000000)) {
            std::printf("FAIL chooser\n");
            return 1;
        }
        // refused: zero sizes, overflowing products, more tiles than a grid
        const size_t big = (size_t)1 << 40;
        if (scan_plan(0, 1, 1, 8, true, 256, 0, 256).ok || scan_plan(1, 0, 1, 8, true, 256, 0, 256).ok ||
            scan_plan(1, 1, 0, 8, true, 256, 0, 256).ok || scan_plan(big, big, 2, 8, true, 256, 0, 256).ok ||
            scan_plan(big, 3, big, 8, true, 256, 0, 256).ok || scan_plan(1, ~(size_t)0, 1, 8, true, 256, 0, 256, 1).ok ||
            scan_plan((size_t)1 << 32, 2, 1, 8, true, 256, SCAN_ROWS, 256).ok) {
            std::printf("FAIL refusals\n");
            return 1;
        }
    }
    std::printf("scan ok: %zu cases\n", cases);
    return 0;
}
