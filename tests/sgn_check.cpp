// Host walk of mpyc_amd/csrc/sgn_geom.hpp, the index arithmetic of the secure-comparison kernels (sgn.hpp), with g++:
// for every element size, l = 1 .. 64 and n = 1 .. 700 it replays what the workgroups do -- stage a chunk of bit columns
// of a tile through LDS (every thread's cursor), walk the columns, write the bit-major outputs -- and checks that
//   * every 4-byte word of rbits is loaded exactly once, and the walker of element h finds exactly the words of
//     (h, i) at column i (so every (element, bit) is owned exactly once);
//   * every LDS index stays inside the declared LDS size, which stays within the bound the header states;
//   * every element of the (l + 1, n) output is written exactly once;
//   * the 64 lanes of a wave read 64 different LDS banks at every step of the column walk, and the staging stores of a
//     full tile put at most two lanes of a 32-lane group on one bank (up to six in a shorter last chunk).
// A full tile does the same whatever n is (its calls do not see n), so full tiles are replayed when they are the last
// tile of an n (n a multiple of the tile) and skipped as inner tiles of larger n; the last tile is replayed for every n.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mpyc_amd/csrc/sgn_geom.hpp"

using namespace ffgpu;

static int fail(const char* what, size_t eb, int l, size_t n) {
    std::printf("FAIL %s: eb=%zu l=%d n=%zu\n", what, eb, l, n);
    return 1;
}

int main() {
    const size_t ebs[5] = {4, 8, 12, 16, 24};
    const size_t NMAX = 700;
    std::vector<unsigned char> seen(NMAX * 64 * 6), outs((64 + 1) * NMAX);
    std::vector<uint32_t> lds;
    for (size_t eb : ebs) {
        const int ew = sgn_elem_words(eb), uw = sgn_unit_words(eb), ch = sgn_chunk(eb), stride = sgn_stride(eb);
        if (sgn_lds_bytes(eb) > (size_t)SGN_LDS_BOUND) return fail("lds bound", eb, 0, 0);
        if (sgn_lds_words(eb) != (size_t)SGN_TILE * (size_t)stride || !(stride & 1) || stride < ch * ew) return fail("stride", eb, 0, 0);
        if (ew % uw || (size_t)ew * 4 != eb || ch < 1) return fail("units", eb, 0, 0);
        // banks: lanes t0 .. t0 + 63 at column j, word w
        for (unsigned t0 = 0; t0 < (unsigned)SGN_TILE; t0 += 64)
            for (int j = 0; j < ch; ++j)
                for (int w = 0; w < ew; ++w) {
                    // 64 lanes in 64 different banks of 4 bytes, and each half wave (the lane group of a 4-byte read) in 32
                    // different banks modulo 32
                    unsigned long long banks = 0, half[2] = {0, 0};
                    for (unsigned t = t0; t < t0 + 64; ++t) {
                        const unsigned a = sgn_walk_lds_word(t, j, eb) + (unsigned)w;
                        banks |= 1ull << (a % 64);
                        half[(t - t0) / 32] |= 1ull << (a % 32);
                    }
                    if (banks != ~0ull || half[0] != 0xffffffffull || half[1] != 0xffffffffull) return fail("bank conflict", eb, j, t0);
                }
        lds.assign(sgn_lds_words(eb), 0xffffffffu);
        for (int l = 1; l <= SGN_MAX_L; ++l) {
            for (size_t n = 1; n <= NMAX; ++n) {
                const SgnPlan p = sgn_plan(n, l, eb);
                if (!p.ok || p.nl != n * (size_t)l || p.tiles != (n + SGN_TILE - 1) / SGN_TILE) return fail("plan", eb, l, n);
                const size_t tile = p.tiles - 1, h0 = sgn_tile_base(tile);
                const unsigned rows = sgn_tile_rows(n, h0);
                if (h0 >= n || h0 + rows != n || rows > (unsigned)SGN_TILE) return fail("tile", eb, l, n);
                const size_t first = h0 * (size_t)l * (size_t)ew, words = (size_t)rows * (size_t)l * (size_t)ew;
                std::memset(seen.data(), 0, words);
                int ncols = 0;
                for (int i0 = 0; i0 < l; i0 += ch) {
                    const int cols = sgn_chunk_cols(l, i0, eb);
                    if (cols < 1 || cols > ch || i0 + cols > l) return fail("chunk", eb, l, n);
                    ncols += cols;
                    const unsigned upr = sgn_units_per_row(cols, eb);
                    if (upr * (unsigned)uw != (unsigned)(cols * ew)) return fail("units per row", eb, l, n);
                    for (unsigned tid = 0; tid < (unsigned)GEOM_THREADS; ++tid) {
                        unsigned q = tid;
                        for (SgnCursor c = sgn_cursor(tid, upr); c.row < rows; sgn_cursor_next(c), q += GEOM_THREADS) {
                            if (c.row != q / upr || c.u != q % upr) return fail("cursor", eb, l, n);
                            const size_t src = sgn_unit_src_word(h0, c.row, l, i0, c.u, eb);
                            const unsigned at = sgn_unit_lds_word(c.row, c.u, eb);
                            for (int w = 0; w < uw; ++w) {
                                if (src + w < first || src + w >= first + words) return fail("load outside the tile", eb, l, n);
                                if ((size_t)at + w >= lds.size()) return fail("lds index (load)", eb, l, n);
                                if (seen[src + w - first]++) return fail("word loaded twice", eb, l, n);
                                lds[at + w] = (uint32_t)(src + w);
                            }
                        }
                    }
                    // staging stores of a full tile: step k of the 32 lanes of a store's lane group (threads g .. g + 31,
                    // units g + k * threads ..), 4 bytes at a time.  A 4-byte store spends 4 cycles moving its registers and 2 LDS cycles per
                    // lane on the busiest bank of a group, so two lanes on a bank cost nothing and four cost twice: a full chunk
                    // (the case every l >= chunk spends its time in) stays at two.  In a shorter last chunk rows start one bank apart (the stride is 33 or 31: +-1 modulo 32), so a bank
                    // is shared by at most as many lanes as a row has words, and by no more than the rows the group spans plus
                    // one: the smaller of the two (at most 6, for rows of 5 or 6 words) bounds it.  (A model of the address pattern, not a measurement.)
                    if (rows == (unsigned)SGN_TILE) {
                        const unsigned wpr = (unsigned)(cols * ew), span = (32 * (unsigned)uw + wpr - 1) / wpr + 1;
                        const unsigned shortmax = wpr < span ? wpr : span;
                        for (unsigned k = 0; k < upr; ++k)
                            for (unsigned g = 0; g < (unsigned)GEOM_THREADS; g += 32)
                                for (int w = 0; w < uw; ++w) {
                                    unsigned char cnt[32] = {0};
                                    for (unsigned t = g; t < g + 32; ++t) {
                                        const unsigned q = t + k * (unsigned)GEOM_THREADS;
                                        if (++cnt[(sgn_unit_lds_word(q / upr, q % upr, eb) + (unsigned)w) % 32] > (cols == ch ? 2u : shortmax))
                                            return fail("staging store: more than two lanes on a bank", eb, l, n);
                                    }
                                }
                    }
                    for (unsigned t = 0; t < rows; ++t)
                        for (int j = 0; j < cols; ++j) {
                            const unsigned at = sgn_walk_lds_word(t, j, eb);
                            const size_t want = ((h0 + t) * (size_t)l + (size_t)(i0 + j)) * (size_t)ew;
                            for (int w = 0; w < ew; ++w) {
                                if ((size_t)at + w >= lds.size()) return fail("lds index (walk)", eb, l, n);
                                if (lds[at + w] != (uint32_t)(want + w)) return fail("walker reads another element", eb, l, n);
                            }
                        }
                }
                if (ncols != l) return fail("columns", eb, l, n);
                for (size_t k = 0; k < words; ++k)
                    if (seen[k] != 1) return fail("word not loaded", eb, l, n);
                // outputs: all tiles, rows 0 .. l (element size does not enter)
                if (eb == 4) {
                    const size_t total = ((size_t)l + 1) * n;
                    std::memset(outs.data(), 0, total);
                    for (size_t tl = 0; tl < p.tiles; ++tl) {
                        const size_t b = sgn_tile_base(tl);
                        for (unsigned t = 0; t < sgn_tile_rows(n, b); ++t)
                            for (int i = 0; i <= l; ++i) {
                                const size_t o = sgn_out_index(i, n, b + t);
                                if (o >= total || outs[o]++) return fail("output index", eb, l, n);
                            }
                    }
                    for (size_t k = 0; k < total; ++k)
                        if (outs[k] != 1) return fail("output not written", eb, l, n);
                }
            }
        }
    }
    // sizes that must be refused
    if (sgn_plan(10, 0, 8).ok || sgn_plan(10, 65, 8).ok || sgn_plan(~(size_t)0 / 8, 64, 8).ok || sgn_plan((size_t)1 << 60, 2, 8).ok)
        return fail("plan accepts", 8, 0, 0);
    std::printf("sgn ok\n");
    return 0;
}
