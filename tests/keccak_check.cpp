// keccak_check.cpp -- mpyc_amd/csrc/keccak_geom.hpp walked with g++ (tests/test_keccak_host.py):
//   * the rho offsets and the pi map against the iterative walk x, y = y, (2x + 3y) % 5 with triangular numbers;
//   * the per-output source (plane, rotation), split into lanes and bytes, against brute force over all 1600 positions;
//   * the 24 x 7 iota bits against the LFSR of FIPS 202 and against the 24 published round constants, and the SWAR word of
//     every lane group;
//   * the launch plan for every nstates from 1 to 2 x (states per workgroup) + 1: every (state, plane, z) owned exactly once,
//     tails masked, keystream counters pairwise distinct; the refusals of the plan and of (m, t).
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <vector>
#include "../mpyc_amd/csrc/keccak_geom.hpp"

using namespace ffgpu;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #c);             \
            return 1;                                                 \
        }                                                             \
    } while (0)

static const uint64_t PUBLISHED[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull,
    0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull,
    0x0000000080008009ull, 0x000000008000000Aull, 0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
    0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// FIPS 202 algorithm 5, as written there: an 8-bit register R, R[0] the result
static int rc_fips(int t) {
    if (t % 255 == 0) return 1;
    int R[9] = {1, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 1; i <= t % 255; ++i) {
        for (int q = 8; q > 0; --q) R[q] = R[q - 1];
        R[0] = 0;
        R[0] ^= R[8];
        R[4] ^= R[8];
        R[5] ^= R[8];
        R[6] ^= R[8];
    }
    return R[0];
}

int main() {
    long checks = 0;
    // rho and pi against the walk
    {
        int seen[25] = {0};
        int x = 1, y = 0;
        CHECK(kk_rho(0, 0) == 0);
        seen[0] = 1;
        for (int t = 0; t < 24; ++t) {
            CHECK(kk_rho(x, y) == (t + 1) * (t + 2) / 2 % 64);
            const int nx = y, ny = (2 * x + 3 * y) % 5;
            CHECK(kk_pi_x(x, y) == nx && kk_pi_y(x, y) == ny);
            CHECK(kk_src_x(nx, ny) == x && kk_src_y(nx, ny) == y);
            CHECK(!seen[5 * y + x]);
            seen[5 * y + x] = 1;
            x = nx;
            y = ny;
            ++checks;
        }
        CHECK(x == 1 && y == 0);
        CHECK(kk_pi_x(0, 0) == 0 && kk_pi_y(0, 0) == 0 && kk_src_plane(0) == 0 && kk_src_rot(0) == 0);
    }
    // the source table against brute force: move 1600 distinct labels by the walk, then read them back through the table
    // the way the kernel does (lanes of four z, a rotation by q lanes and c bytes)
    {
        std::vector<int> a(1600), b(1600, -1);
        for (int i = 0; i < 1600; ++i) a[i] = i;
        for (int z = 0; z < 64; ++z) b[z] = a[z];
        int x = 1, y = 0;
        for (int t = 0; t < 24; ++t) {
            const int shift = (t + 1) * (t + 2) / 2 % 64;
            const int nx = y, ny = (2 * x + 3 * y) % 5;
            for (int z = 0; z < 64; ++z) b[64 * (5 * ny + nx) + (z + shift) % 64] = a[64 * (5 * y + x) + z];
            x = nx;
            y = ny;
        }
        for (int P = 0; P < 25; ++P) {
            const int sp = kk_src_plane(P), r = kk_src_rot(P), q = kk_rot_lanes(r), c = kk_rot_bytes(r);
            CHECK(sp >= 0 && sp < 25 && r >= 0 && r < 64 && 4 * q + c == r && c >= 0 && c < 4 && q >= 0 && q < 16);
            for (int g = 0; g < 16; ++g)
                for (int i = 0; i < 4; ++i) {
                    // byte i of (hi << 8c) | (lo >> 8(4 - c)): byte i - c of the word of lane g - q, or byte 4 + i - c of lane g - q - 1
                    const int lane = i >= c ? (g - q) & 15 : (g - q - 1) & 15;
                    const int byte = i >= c ? i - c : 4 + i - c;
                    CHECK(b[64 * P + 4 * g + i] == a[64 * sp + 4 * lane + byte]);
                    ++checks;
                }
        }
    }
    // iota
    {
        const KkRoundConstants tab = kk_round_constants();
        for (int r = 0; r < 24; ++r) {
            uint64_t rc = 0;
            for (int j = 0; j < 7; ++j) {
                CHECK(kk_iota_bit(r, j) == rc_fips(7 * r + j));
                if (rc_fips(7 * r + j)) rc |= 1ull << ((1 << j) - 1);
                ++checks;
            }
            CHECK(rc == PUBLISHED[r] && kk_round_constant(r) == PUBLISHED[r] && tab.rc[r] == PUBLISHED[r]);
            for (int g = 0; g < 16; ++g) {
                const uint32_t w = kk_iota_word(PUBLISHED[r], g);
                for (int i = 0; i < 4; ++i) CHECK(((w >> (8 * i)) & 0xffu) == ((PUBLISHED[r] >> (4 * g + i)) & 1u));
            }
        }
        CHECK(kk_iota_word(0, 3) == 0);
    }
    // the plan
    CHECK(KK_STATES_PER_WG == 16 && KK_THREADS == 256 && KK_LANES_PER_STATE == 16);
    CHECK(kk_nblk(1) == 2 && kk_nblk(2) == 4 && kk_nblk(3) == 5);
    for (size_t nstates = 1; nstates <= 2 * KK_STATES_PER_WG + 1; ++nstates) {
        const KkPlan pl = kk_plan(nstates);
        CHECK(pl.ok && pl.grid == (nstates + 15) / 16 && pl.tail_states >= 1 && pl.tail_states <= 16);
        CHECK((size_t)(pl.grid - 1) * 16 + pl.tail_states == nstates);
        std::vector<int> owned(nstates * 1600, 0);
        for (int t = 1; t <= 3; ++t) {
            std::set<uint64_t> ctrs;
            size_t live = 0;
            for (unsigned blk = 0; blk < pl.grid; ++blk)
                for (int th = 0; th < KK_THREADS; ++th) {
                    const uint64_t s = kk_state_of(blk, th);
                    const int g = kk_group_of(th);
                    CHECK(g >= 0 && g < 16 && g == (th & 15) && (th >> 4) + 16 * blk == s);      // 16 consecutive lanes a state
                    if (s >= nstates) continue;                                                   // masked tail
                    ++live;
                    for (int b = 0; b < kk_nblk(t); ++b) CHECK(ctrs.insert(kk_ctr(s, g, kk_nblk(t)) + b).second);
                    if (t == 1)
                        for (int p = 0; p < 25; ++p) {
                            const size_t off = kk_offset(s, p, g);
                            CHECK(off % 4 == 0 && off + 4 <= nstates * 1600);
                            for (int i = 0; i < 4; ++i) ++owned[off + i];
                        }
                }
            CHECK(live == nstates * 16 && ctrs.size() == live * (size_t)kk_nblk(t));
            CHECK(*ctrs.rbegin() == nstates * 16 * (uint64_t)kk_nblk(t) - 1 && *ctrs.rbegin() < KK_CTR_LIMIT);
            // the counters of a state do not depend on nstates
            CHECK(kk_ctr(0, 0, kk_nblk(t)) == 0 && kk_ctr(nstates - 1, 15, kk_nblk(t)) == ((nstates - 1) * 16 + 15) * kk_nblk(t));
        }
        for (size_t i = 0; i < owned.size(); ++i) CHECK(owned[i] == 1);
        checks += (long)owned.size();
    }
    CHECK(!kk_plan(0).ok && kk_plan(KK_MAX_GRID * 16).ok && !kk_plan(KK_MAX_GRID * 16 + 1).ok);
    CHECK(kk_plan(KK_MAX_GRID * 16).grid == KK_MAX_GRID && (uint64_t)KK_MAX_GRID * KK_THREADS <= 0xffffffffull);
    {
        int pairs = 0;
        for (int m = 0; m <= 9; ++m)
            for (int t = -1; t <= 5; ++t) pairs += kk_pair_ok(m, t) ? 1 : 0;
        CHECK(pairs == 10 && kk_pair_ok(1, 0) && kk_pair_ok(3, 1) && kk_pair_ok(7, 3) && kk_pair_ok(5, 2) && !kk_pair_ok(2, 0) &&
              !kk_pair_ok(4, 2) && !kk_pair_ok(8, 1) && !kk_pair_ok(6, 3));
    }
    printf("keccak ok %ld\n", checks);
    return 0;
}
