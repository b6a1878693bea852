// sbox_layer_geom.hpp -- launch arithmetic and keystream counters of the fused GF(2^8) S-box layer (misc.hip,
// k_gf8_sbox_layer).  Plain C++ (no HIP): the kernel and its launcher take the grid, the steps of a thread and every block
// counter from here, and tests/sbox_layer_check.cpp walks the same functions with g++.
//
// n secure bytes, one SWAR word (four bytes) per thread and step: nthreads_full = n / 4 words go through the grid-stride
// loop (word i in step i / gsz of thread i % gsz), the n % 4 bytes after them through thread 0 with byte accesses.  The
// grid is capped at the resident workgroups, so a thread walks through `steps` words at the most.
//
// The keystream (ChaCha, 64-bit block counter, one key and nonce per launch) is drawn from four disjoint counter ranges:
//   fresh stream per step  word i draws its 11 K T coefficient words from blocks i * NBLK .. i * NBLK + NBLK - 1
//                          (K = 2t + 1, NBLK = ceil(11 K T / 16): 3, 7, 15 for t = 1, 2, 3);
//   continued stream       (t = 1 and steps >= 4) thread g draws 32 words per step from its own blocks
//                          g * bpt .. g * bpt + bpt - 1, bpt = 2 steps + 2: two per step, and the one that SblKeystream<DR>
//                          (rng.hpp) holds in progress behind the last step;
//   ragged end             a fresh stream at 2^61;
//   spare blocks           the 33rd word of the steps 16 q .. 16 q + 15 of thread g of the continued stream comes from
//                          block 2^62 + g * spt + q, spt = steps / 16 + 1.
// The first two lie below 2^61, everything below 2^63 (from where the re-draws of the samplers count, rng.hpp): a shape
// that would leave a range is refused (ok = 0).
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { SBL_THREADS = 256 };                 // = BLOCK (kernels.hpp)
enum { SBL_W = 1 };                         // SWAR words of a thread per step
enum { SBL_MAX_M = 7, SBL_MAX_T = 3 };

static constexpr uint64_t SBL_CTR_LIMIT = 1ull << 61;        // the two stream ranges end here
static constexpr uint64_t SBL_CTR_RAGGED = 1ull << 61;       // first block of the ragged end
static constexpr uint64_t SBL_CTR_SPARE = 1ull << 62;        // first spare block

// keystream words of a step, and the blocks that hold them
FFG_CX int sbl_step_words(int t, int w) { return 11 * (2 * t + 1) * t * w; }
FFG_CX int sbl_nblk(int t, int w) { return (sbl_step_words(t, w) + 15) / 16; }
// the continued stream exists for one word per thread at t = 1: 33 = 2 x 16 + 1 words per step
FFG_CX bool sbl_can_cont(int t, int w) { return t == 1 && w == 1; }

// resident workgroups per compute unit (4 per CU at t = 1, m <= 4: 119-128 VGPRs; 3 for m >= 5; 2-3 per CU for t >= 2)
FFG_CX int sbl_resident_per_cu(int t, int m) { return t == 1 ? (m <= 4 ? 4 : 3) : (t == 2 ? 3 : 2); }

// what a thread of a grid of gsz threads does with nthreads_full words
FFG_HD uint64_t sbl_nsteps(size_t nthreads_full, size_t gsz) { return (nthreads_full + gsz - 1) / gsz; }   // words of thread 0
FFG_HD uint64_t sbl_bpt(uint64_t steps) { return 2 * steps + 2; }         // blocks of a thread's continued stream
FFG_HD uint64_t sbl_spt(uint64_t steps) { return steps / 16 + 1; }        // its spare blocks
// the keystream continues from step to step
FFG_HD bool sbl_cont(int t, int w, uint64_t steps) { return sbl_can_cont(t, w) && steps >= 4; }

// block counters
FFG_HD uint64_t sbl_ctr_step(size_t i, int nblk) { return (uint64_t)i * nblk; }                  // fresh stream of word i
FFG_HD uint64_t sbl_ctr_thread(size_t g, uint64_t bpt) { return (uint64_t)g * bpt; }             // continued stream of thread g
FFG_HD uint64_t sbl_ctr_spare(size_t g, uint64_t spt, uint64_t j) {                              // spare block of step j
    return SBL_CTR_SPARE + (uint64_t)g * spt + (j >> 4);
}

struct SblPlan {
    int ok;                 // 0: a counter range would be left (n > ~10^17 bytes) -- nothing may be launched
    size_t nthreads_full;   // whole words of a row
    int rest_bytes;         // the n % 4 bytes after them: thread 0, byte accesses
    unsigned grid;          // workgroups: one word per thread, capped at the resident ones
    uint64_t steps;
    int cont;
    int NBLK;
    uint64_t bpt, spt;
};
// (m, t) as the launcher dispatches them: 2t + 1 <= m <= 7, 1 <= t <= 3
FFG_HD SblPlan sbl_plan(size_t n, int t, int m, int num_cu) {
    SblPlan pl = SblPlan();
    constexpr int W = SBL_W;
    pl.nthreads_full = n / (4 * (size_t)W);
    pl.rest_bytes = (int)(n - pl.nthreads_full * 4 * W);
    size_t want = (pl.nthreads_full + SBL_THREADS - 1) / SBL_THREADS;
    if (want < 1) want = 1;
    const size_t resident = (size_t)num_cu * sbl_resident_per_cu(t, m);
    if (want > resident) want = resident;
    pl.grid = (unsigned)want;
    const uint64_t gsz = (uint64_t)pl.grid * SBL_THREADS;
    pl.steps = sbl_nsteps(pl.nthreads_full, gsz);
    pl.cont = sbl_cont(t, W, pl.steps);
    pl.NBLK = sbl_nblk(t, W);
    pl.bpt = sbl_bpt(pl.steps);
    pl.spt = sbl_spt(pl.steps);
    pl.ok = !(gsz * pl.bpt >= SBL_CTR_LIMIT || gsz * pl.spt >= SBL_CTR_LIMIT ||
              pl.nthreads_full * 16ull >= SBL_CTR_LIMIT);
    return pl;
}

}  // namespace ffgpu
