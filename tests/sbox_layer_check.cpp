// sbox_layer_check.cpp -- walks mpyc_amd/csrc/sbox_layer_geom.hpp on the host (g++, no HIP): the launch plan of the fused
// GF(2^8) S-box layer and the ChaCha block counters its threads use, as k_gf8_sbox_layer (misc.hip) takes them from the header.
//
// For num_cu in {1, 2, 3}, all nine (m, t) and n on both sides of every threshold (one word, one workgroup, the capped grid,
// steps = 1 .. 5 where the continued stream begins at 4, steps 16 / 17 and 32 / 33 where a thread takes its next spare block,
// each with 0 .. 3 ragged bytes and one word less or more) every (thread, step) is enumerated the way the kernel loops:
//   * every word below nthreads_full is taken once, by thread i % gsz in step i / gsz, and no thread takes more than `steps`;
//   * fresh stream per step: word i DRAWS from blocks i NBLK .. i NBLK + NBLK - 1 (NBLK blocks hold the 11 K T words of a
//     step, the last one in part); SblKeystream<10> also keeps block i NBLK + NBLK IN PROGRESS when the step ends -- the
//     first block of word i + 1, worked on and thrown away, no word of it is handed out by this step;
//   * continued stream (t = 1, steps >= 4): thread g draws two blocks per step from g bpt on and keeps g bpt + 2 (its
//     steps) in progress behind its last step: all inside [g bpt, (g + 1) bpt), which no other thread enters; the 33rd
//     word of step j comes from spare block 2^62 + g spt + j / 16, inside [2^62 + g spt, 2^62 + (g + 1) spt);
//   * the ragged end draws NBLK blocks from 2^61 on.
// All blocks DRAWN FROM are pairwise distinct; the blocks in progress of the continued stream are distinct from every drawn
// block and from each other; streams stay below 2^61, the ragged end in [2^61, 2^61 + 15], spare blocks in [2^62, 2^62 + 2^61),
// everything below 2^63.  `ok` is the launcher's refusal: it is restated with 128-bit integers (the uint64 expression it is
// written in may wrap only where an earlier clause already refuses) and probed at huge n.
// Prints "sbox_layer ok <plans> <blocks>" and exits 0, or the first failure and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../mpyc_amd/csrc/sbox_layer_geom.hpp"

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

typedef unsigned __int128 u128;
static size_t nplans = 0, nblocks = 0;
static const int MT[9][2] = {{3, 1}, {4, 1}, {5, 1}, {5, 2}, {6, 1}, {6, 2}, {7, 1}, {7, 2}, {7, 3}};

// the launcher's arithmetic, restated from its description with integers that cannot wrap
struct Restated {
    u128 nthreads_full, grid, gsz, steps;
    int rest, per_cu, nblk, cont, ok;
};
static Restated restate(size_t n, int t, int m, int num_cu) {
    Restated r;
    r.nthreads_full = n / 4;
    r.rest = (int)(n % 4);
    r.per_cu = t == 1 ? (m <= 4 ? 4 : 3) : (t == 2 ? 3 : 2);
    u128 want = (r.nthreads_full + 255) / 256;
    if (want < 1) want = 1;
    r.grid = std::min<u128>(want, (u128)num_cu * r.per_cu);
    r.gsz = r.grid * 256;
    r.steps = (r.nthreads_full + r.gsz - 1) / r.gsz;
    r.nblk = t == 1 ? 3 : (t == 2 ? 7 : 15);
    r.cont = t == 1 && r.steps >= 4;
    const u128 lim = (u128)1 << 61;
    r.ok = r.gsz * (2 * r.steps + 2) < lim && r.gsz * (r.steps / 16 + 1) < lim && r.nthreads_full * 16 < lim;
    return r;
}

static void check_header(const SblPlan& pl, size_t n, int t, int m, int num_cu) {
    const Restated r = restate(n, t, m, num_cu);
    CHECK(pl.ok == r.ok, "n=%zu t=%d m=%d cu=%d: ok=%d", n, t, m, num_cu, pl.ok);
    CHECK((u128)pl.nthreads_full == r.nthreads_full && pl.rest_bytes == r.rest && (u128)pl.grid == r.grid, "n=%zu t=%d m=%d", n, t, m);
    CHECK((u128)pl.steps == r.steps && pl.cont == r.cont && pl.NBLK == r.nblk, "n=%zu t=%d m=%d: steps", n, t, m);
    CHECK((u128)pl.bpt == 2 * r.steps + 2 && (u128)pl.spt == r.steps / 16 + 1, "n=%zu: bpt / spt", n);
    CHECK(pl.NBLK == sbl_nblk(t, SBL_W) && pl.NBLK * 16 >= sbl_step_words(t, SBL_W) && (pl.NBLK - 1) * 16 < sbl_step_words(t, SBL_W),
          "NBLK holds the words of a step");
    CHECK(sbl_step_words(t, SBL_W) == 11 * (2 * t + 1) * t, "words of a step");
    CHECK(!pl.cont || sbl_step_words(t, SBL_W) == 33, "the continued stream: two whole blocks and one spare word");
    CHECK(pl.grid >= 1 && pl.grid <= (unsigned)(num_cu * sbl_resident_per_cu(t, m)), "the capped grid");
}

static void walk(size_t n, int t, int m, int num_cu) {
    const SblPlan pl = sbl_plan(n, t, m, num_cu);
    check_header(pl, n, t, m, num_cu);
    CHECK(pl.ok, "a small shape is refused: n=%zu", n);
    CHECK(pl.nthreads_full * 4 + (size_t)pl.rest_bytes == n && pl.rest_bytes >= 0 && pl.rest_bytes < 4, "words and ragged bytes");
    const size_t gsz = (size_t)pl.grid * SBL_THREADS;
    // what the kernel derives from (nthreads_full, gsz) is what the launcher planned with
    const uint64_t ksteps = sbl_nsteps(pl.nthreads_full, gsz);
    CHECK(ksteps == pl.steps && sbl_bpt(ksteps) == pl.bpt && sbl_spt(ksteps) == pl.spt && (int)sbl_cont(t, SBL_W, ksteps) == pl.cont,
          "kernel and launcher disagree");
    std::vector<uint64_t> drawn, progress;
    std::vector<int> seen(pl.nthreads_full, 0);
    const uint64_t lim = SBL_CTR_LIMIT;
    for (size_t g = 0; g < gsz; ++g) {
        uint64_t j = 0;
        const uint64_t base = sbl_ctr_thread(g, pl.bpt);
        for (size_t i = g; i < pl.nthreads_full; i += gsz, ++j) {
            ++seen[i];
            CHECK(i % gsz == g && i / gsz == j, "word %zu", i);
            if (pl.cont) {
                for (int b = 0; b < 2; ++b) {
                    const uint64_t c = base + 2 * j + b;
                    CHECK(c >= base && c < base + pl.bpt && c < lim, "thread %zu step %llu leaves its blocks", g, (unsigned long long)j);
                    drawn.push_back(c);
                }
                const uint64_t sc = sbl_ctr_spare(g, pl.spt, j);
                CHECK(sc >= SBL_CTR_SPARE + g * pl.spt && sc < SBL_CTR_SPARE + (g + 1) * pl.spt && sc < SBL_CTR_SPARE + lim,
                      "spare block of thread %zu step %llu", g, (unsigned long long)j);
                if ((j & 15) == 0) drawn.push_back(sc);                       // computed once, serves 16 steps
                else CHECK(sc == sbl_ctr_spare(g, pl.spt, j & ~15ull), "steps of one spare block");
            } else {
                const uint64_t c0 = sbl_ctr_step(i, pl.NBLK);
                CHECK(c0 == (uint64_t)i * (uint64_t)pl.NBLK, "fresh stream of word %zu", i);
                for (int b = 0; b < pl.NBLK; ++b) {
                    CHECK(c0 + b < lim, "word %zu leaves the stream range", i);
                    drawn.push_back(c0 + b);
                }
                // in progress when the step ends (SblKeystream<10>): the next word's first block, never handed out here
                CHECK(c0 + pl.NBLK == sbl_ctr_step(i + 1, pl.NBLK) && c0 + pl.NBLK < lim, "block in progress of word %zu", i);
            }
        }
        CHECK(j <= pl.steps, "thread %zu takes %llu steps", g, (unsigned long long)j);
        if (g == 0) CHECK(j == pl.steps, "thread 0 takes every step");
        if (pl.cont && g < pl.nthreads_full) {                                 // begin() ran; after j steps block base + 2 j is in progress
            const uint64_t c = base + 2 * j;
            CHECK(c >= base && c < base + pl.bpt && c < lim, "block in progress of thread %zu", g);
            progress.push_back(c);
        }
    }
    for (size_t i = 0; i < pl.nthreads_full; ++i) CHECK(seen[i] == 1, "word %zu taken %d times", i, seen[i]);
    if (pl.rest_bytes)
        for (int b = 0; b < pl.NBLK; ++b) {
            const uint64_t c = SBL_CTR_RAGGED + b;
            CHECK(c >= lim && c < SBL_CTR_SPARE, "ragged end");
            drawn.push_back(c);
        }
    const size_t ndrawn = drawn.size();
    std::vector<uint64_t> all(drawn);
    all.insert(all.end(), progress.begin(), progress.end());
    std::sort(all.begin(), all.end());
    for (size_t q = 1; q < all.size(); ++q) CHECK(all[q] != all[q - 1], "block %llu used twice (n=%zu t=%d m=%d cu=%d)", (unsigned long long)all[q], n, t, m, num_cu);
    if (!all.empty()) CHECK(all.back() < (1ull << 63), "a block in the range of the re-draws");
    nblocks += ndrawn;
    ++nplans;
}

int main() {
    CHECK(SBL_THREADS == 256 && SBL_W == 1 && SBL_CTR_LIMIT == (1ull << 61) && SBL_CTR_RAGGED == (1ull << 61) && SBL_CTR_SPARE == (1ull << 62),
          "the constants of the header");
    CHECK(sbl_nblk(1, 1) == 3 && sbl_nblk(2, 1) == 7 && sbl_nblk(3, 1) == 15 && sbl_can_cont(1, 1) && !sbl_can_cont(2, 1) && !sbl_can_cont(1, 2),
          "blocks of a step");
    for (int cu = 1; cu <= 3; ++cu)
        for (const auto& mt : MT) {
            const int m = mt[0], t = mt[1];
            const size_t gmax = (size_t)cu * sbl_resident_per_cu(t, m) * 256;      // threads of the capped grid
            std::vector<size_t> ns = {1, 2, 3, 4, 5, 7, 8, 4 * 255, 4 * 256, 4 * 256 + 1, 4 * 257, 4 * 257 + 3};
            for (size_t steps : {1, 2, 3, 4, 5, 16, 17, 32, 33})
                for (int d = -1; d <= 1; ++d)
                    for (size_t rest = 0; rest < (d ? 1u : 4u); ++rest) ns.push_back(4 * (gmax * steps + d) + rest);
            for (size_t n : ns) walk(n, t, m, cu);
            // the thresholds themselves
            CHECK(sbl_plan(4 * gmax * 3, t, m, cu).cont == 0 && sbl_plan(4 * gmax * 3 + 3, t, m, cu).cont == 0, "three steps: fresh streams");
            CHECK(sbl_plan(4 * gmax * 3 + 4, t, m, cu).cont == (t == 1) && sbl_plan(4 * gmax * 3 + 4, t, m, cu).steps == 4, "four steps: continued at t = 1");
            CHECK(sbl_plan(0, t, m, cu).ok && sbl_plan(0, t, m, cu).grid == 1 && sbl_plan(0, t, m, cu).steps == 0, "n = 0 is a plan of nothing");
        }
    // the refusal, at sizes nobody can enumerate: on both sides of each clause, and where the uint64 expressions wrap
    size_t nrefused = 0, naccepted = 0;
    for (int cu : {1, 3, 256, 304})
        for (const auto& mt : MT) {
            const int m = mt[0], t = mt[1];
            const uint64_t gsz = (uint64_t)cu * sbl_resident_per_cu(t, m) * 256;
            std::vector<uint64_t> ns;
            for (int e = 40; e < 64; ++e)
                for (int64_t d : {-5, -4, -1, 0, 1, 4, 5}) ns.push_back((1ull << e) + (uint64_t)d);
            // 2 gsz (steps + 1) = 2^61 exactly when nthreads_full = 2^60 - gsz (gsz a power of two times 1, 3 ...): walk around it
            for (int64_t d = -3; d <= 3; ++d) {
                ns.push_back(4 * ((1ull << 60) - gsz + (uint64_t)d));
                ns.push_back(4 * ((1ull << 60) - 2 * gsz + (uint64_t)d));
                ns.push_back(4 * ((1ull << 60) + (uint64_t)d));
                ns.push_back(4 * ((1ull << 57) + (uint64_t)d));                // nthreads_full * 16 = 2^61
            }
            ns.push_back(~0ull);
            ns.push_back(~0ull - 3);
            for (uint64_t n : ns) {
                const SblPlan pl = sbl_plan((size_t)n, t, m, cu);
                check_header(pl, (size_t)n, t, m, cu);
                if (pl.ok) {
                    ++naccepted;
                    // the last thread's last block and spare block are inside their ranges
                    const u128 g = (u128)pl.grid * 256 - 1;
                    CHECK(g * pl.bpt + pl.bpt <= (u128)SBL_CTR_LIMIT && (u128)pl.nthreads_full * pl.NBLK <= (u128)SBL_CTR_LIMIT, "accepted, and a stream leaves its range");
                    CHECK((u128)SBL_CTR_SPARE + g * pl.spt + pl.spt <= ((u128)1 << 63), "accepted, and a spare block reaches the re-draws");
                } else {
                    ++nrefused;
                }
            }
        }
    CHECK(nrefused > 500 && naccepted > 500, "both sides of the refusal: %zu refused, %zu accepted", nrefused, naccepted);
    printf("sbox_layer ok %zu %zu\n", nplans, nblocks);
    return 0;
}
