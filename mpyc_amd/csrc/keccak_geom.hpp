// keccak_geom.hpp -- the rho / pi / iota tables of Keccak-f[1600] and the launch arithmetic of the secure Keccak round
// kernels (keccak.hpp: k_keccak).  Plain C++ (no HIP): the kernels and their launcher take every table entry, the state
// and lane a thread owns and every keystream counter from here, and tests/keccak_check.cpp walks the same functions with
// g++.
//
// Layout.  A party's share of a batch of states is nstates x 1600 bytes, state-major: position i = 64 (5 y + x) + z of
// state b (S[i] of demos/sha3.py:43, A[x, y, z]) is byte 1600 b + i, one GF(2^n) element per byte.  "Plane" p = 5 y + x
// names the 64 positions of one (x, y); they are 16 dwords.
//
// Threads.  A wave holds FOUR states; lane l owns z = 4 (l & 15) .. 4 (l & 15) + 3 of state (l >> 4) of its wave, as 25 SWAR
// words (one per plane, GF2P8::word: byte i of the word = z = 4 (l & 15) + i).  A plane of a state is then 16 consecutive
// dwords read by 16 consecutive lanes, and a rotation along z by r = 4 q + c is a rotation by q lanes within the 16-lane
// group and a funnel shift by c bytes.  A workgroup of 256 threads holds 16 states; the grid is ceil(nstates / 16)
// workgroups by the senders of the launch, NOT capped: what a thread does depends on its state alone.
//
// Keystream (ChaCha, one key and nonce per launch, the sender in bits 8..15 of nonce word 1 as in the batched chain gate):
// the thread of (state b, lane group g = z / 4) draws its 25 t coefficient words -- word (plane p, coefficient q) is draw
// number p t + q -- from blocks (16 b + g) NBLK .. + NBLK - 1, NBLK = ceil(25 t / 16).  So the keystream a position
// receives depends on (key, nonce, sender, b, position) only.  The counters stay below 2^61 (the ranges above it belong to
// other kernels, sbox_layer_geom.hpp and rng.hpp), which every nstates that a grid admits does.
#pragma once
#include "geom.hpp"

namespace ffgpu {

enum { KK_STATE_BYTES = 1600, KK_PLANES = 25, KK_ROUNDS = 24 };
enum { KK_THREADS = 256 };                        // = BLOCK (kernels.hpp)
enum { KK_LANES_PER_STATE = 16 };                 // 64 z / 4 bytes of a word
enum { KK_STATES_PER_WG = KK_THREADS / KK_LANES_PER_STATE };   // 16
enum { KK_MAX_K = 7, KK_MAX_M = 7, KK_MAX_T = 3 };

// ---- rho, pi ----------------------------------------------------------------------------------------------------
// rho offset of plane (x, y): the triangular numbers (t + 1)(t + 2) / 2 mod 64 along the walk (x, y) <- (y, 2x + 3y) from
// (1, 0) (FIPS 202 section 3.2.2; demos/sha3.py:29, 91-95), 0 for (0, 0) -- as the published table, index 5 y + x
FFG_CX int kk_rho(int x, int y) {
    constexpr int R[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    return R[5 * y + x];
}
// pi: plane (x, y) moves to (y, 2x + 3y)
FFG_CX int kk_pi_x(int, int y) { return y; }
FFG_CX int kk_pi_y(int x, int y) { return (2 * x + 3 * y) % 5; }
// the inverse, per OUTPUT plane (X, Y) of rho-pi: b[X, Y, z] = a[x, y, z - rho(x, y)] with y = X, x = (X + 3 Y) mod 5
// (2 x = Y - 3 X, 1 / 2 = 3 mod 5)
FFG_CX int kk_src_x(int X, int Y) { return (X + 3 * Y) % 5; }
FFG_CX int kk_src_y(int X, int) { return X; }
FFG_CX int kk_src_plane(int P) { return 5 * kk_src_y(P % 5, P / 5) + kk_src_x(P % 5, P / 5); }
FFG_CX int kk_src_rot(int P) { return kk_rho(kk_src_x(P % 5, P / 5), kk_src_y(P % 5, P / 5)); }
// a rotation along z by r on the words of a 16-lane group: out(g) = (w(g - q) << 8 c) | (w(g - q - 1) >> 8 (4 - c))
FFG_CX int kk_rot_lanes(int r) { return r >> 2; }
FFG_CX int kk_rot_bytes(int r) { return r & 3; }

// ---- iota ---------------------------------------------------------------------------------------------------------
// bit j of round r: the coefficient of x^0 of x^(7 r + j) mod x^8 + x^6 + x^5 + x^4 + 1 (FIPS 202 algorithm 5;
// demos/sha3.py:31-33), added at z = 2^j - 1 of plane (0, 0)
FFG_CX int kk_rc_bit(int t) {
    unsigned v = 1;                               // x^0
    for (int i = 0; i < t % 255; ++i) {
        v <<= 1;
        if (v & 0x100u) v ^= 0x171u;              // x^8 = x^6 + x^5 + x^4 + 1
    }
    return (int)(v & 1u);
}
FFG_CX int kk_iota_bit(int round, int j) { return kk_rc_bit(7 * round + j); }
// the round constant as the 64-bit lane word of the standard
FFG_CX uint64_t kk_round_constant(int round) {
    uint64_t rc = 0;
    for (int j = 0; j < 7; ++j)
        if (kk_iota_bit(round, j)) rc |= 1ull << ((1 << j) - 1);
    return rc;
}
struct KkRoundConstants {
    uint64_t rc[KK_ROUNDS];
};
FFG_CX KkRoundConstants kk_round_constants() {
    KkRoundConstants t = KkRoundConstants();
    for (int r = 0; r < KK_ROUNDS; ++r) t.rc[r] = kk_round_constant(r);
    return t;
}
// the SWAR word lane group g adds to plane 0: the field's 1 in byte i where bit 4 g + i of the round constant is set
FFG_HD uint32_t kk_iota_word(uint64_t rc, int g) {
    const uint32_t nib = (uint32_t)(rc >> (4 * g)) & 0xfu;
    return (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
}

// ---- threads and keystream ---------------------------------------------------------------------------------------
FFG_CX int kk_nblk(int t) { return (KK_PLANES * t + 15) / 16; }              // keystream blocks of a thread: 2, 4, 5
FFG_HD uint64_t kk_state_of(uint64_t block, int thread) { return block * KK_STATES_PER_WG + (uint64_t)(thread / KK_LANES_PER_STATE); }
FFG_HD int kk_group_of(int thread) { return thread % KK_LANES_PER_STATE; }
// first keystream block of the thread of (state, lane group)
FFG_HD uint64_t kk_ctr(uint64_t state, int group, int nblk) { return (state * KK_LANES_PER_STATE + (uint64_t)group) * (uint64_t)nblk; }
// byte offset of the thread's word of plane p within a row
FFG_HD size_t kk_offset(uint64_t state, int plane, int group) {
    return (size_t)state * KK_STATE_BYTES + (size_t)(64 * plane + 4 * group);
}

static constexpr uint64_t KK_CTR_LIMIT = 1ull << 61;
static constexpr uint64_t KK_MAX_GRID = 0xffffffffull / KK_THREADS;     // a grid dimension times the workgroup size stays below 2^32

struct KkPlan {
    int ok;              // 0: nstates needs more workgroups than a grid has (2.7 * 10^8 states, 429 GB a row) -- nothing may be launched
    unsigned grid;       // workgroups per sender
    int tail_states;     // states of the last workgroup (1..16)
};
FFG_HD KkPlan kk_plan(size_t nstates) {
    KkPlan pl = KkPlan();
    const uint64_t want = ((uint64_t)nstates + KK_STATES_PER_WG - 1) / KK_STATES_PER_WG;
    pl.ok = nstates >= 1 && want <= KK_MAX_GRID &&
            (uint64_t)nstates * KK_LANES_PER_STATE * (uint64_t)kk_nblk(KK_MAX_T) < KK_CTR_LIMIT;
    pl.grid = pl.ok ? (unsigned)want : 0u;
    pl.tail_states = pl.ok ? (int)(nstates - (size_t)(want - 1) * KK_STATES_PER_WG) : 0;
    return pl;
}
// the (m, t) the round kernel is built for: no re-sharing for one party, and the pairs of the S-box layer
FFG_CX bool kk_pair_ok(int m, int t) {
    return (m == 1 && t == 0) || (t >= 1 && t <= KK_MAX_T && m >= 2 * t + 1 && m <= KK_MAX_M);
}

}  // namespace ffgpu
