// keccak.hpp -- one secure round of Keccak-f[1600] on shares over GF(2^n <= 8) (demos/sha3.py:72-106), for a batch of
// states and all senders of a re-sharing round in one launch.  Included by misc.hip; geometry, tables and keystream
// counters: keccak_geom.hpp.
//
// The map, for one sender's share a of one state (planes a[x, y] of 64 positions z):
//   1. a = sum_s lam_s rows[s] (the recombination of the previous round's sub-shares; k = 1, lam = 1: a plain share),
//      then iota of the PREVIOUS round: the field's 1 added at z = 2^j - 1 of plane (0, 0) where the constant has a bit
//      (every party adds a public constant to its share);
//   2. theta: C[x] = sum_y a[x, y], D[x] = C[x - 1] + rot(C[x + 1], 1), a[x, y] += D[x];
//   3. rho, pi: b[y, 2x + 3y] = rot(a[x, y], rho(x, y));
//   4. chi, local: out[x, y] = b[x, y] + (b[x + 1, y] + 1) b[x + 2, y] -- a degree-2t sharing held by the senders;
//   5. (k_keccak<M, T>, M >= 1) every element of out is dealt to the M parties with a fresh degree-T polynomial whose
//      coefficients come from the ChaCha keystream: share_j = out + sum_q c_q (j + 1)^(q + 1), Horner with muladd_small.
// apply_round = 0 stops after step 1 (the tail after round 23, and the plain recombination).
//
// A lane holds 4 consecutive z of the 25 planes of one state as 25 SWAR words (GF2P8::word), 16 lanes a state, 4 states a
// wave: every load and store is a dword, 64 consecutive bytes per state and plane; a rotation along z by r is one or two
// cross-lane reads within the 16-lane group (ds_bpermute) and a funnel shift by r % 4 bytes.  The arithmetic is GF2P8's
// own (acc_mac, mul, muladd_small).
#pragma once
#include "keccak_geom.hpp"

namespace ffgpu {

struct KeccakArgs {
    const uint8_t* rows[KK_MAX_K];   // the k rows sender 0 recombines; sender y reads them in_batch bytes further on
    uint32_t lam[KK_MAX_K];
    int k;
    int apply_round;
    size_t in_batch;
    uint8_t* out;                    // M == 0: sender y's state at out + y * out_batch;
    size_t out_batch, share_stride;  // M >= 1: the share of party j + 1 from sender y at out + j * share_stride + y * out_batch
    uint64_t rc;                     // round constant of the iota in front (0: none)
    uint64_t nstates;
};

// rot(v, r) along z on the words of a 16-lane group: out(g) = (v(g - q) << 8 c) | (v(g - q - 1) >> 8 (4 - c)), r = 4 q + c.
// r is a compile-time constant wherever this is called (unrolled loops over constexpr tables).
__device__ __forceinline__ uint32_t kk_rot(uint32_t v, int r, int group) {
    const int q = kk_rot_lanes(r), c = kk_rot_bytes(r);
    const uint32_t hi = q ? (uint32_t)__shfl((int)v, (group - q) & 15, KK_LANES_PER_STATE) : v;
    if (c == 0) return hi;
    const uint32_t lo = (uint32_t)__shfl((int)v, (group - q - 1) & 15, KK_LANES_PER_STATE);
    return (hi << (8 * c)) | (lo >> (32 - 8 * c));
}

// M == 0: the deterministic map only (ffgm_gf2_keccak_local)
template <int M, int T>
__global__ __launch_bounds__(KK_THREADS) void k_keccak(GF2P8 f, KeccakArgs a, RngArgs ra) {
    constexpr bool SHARE = M > 0;
    if constexpr (SHARE) rng_load_state(ra);
    const int g = kk_group_of((int)threadIdx.x);
    const uint64_t state = kk_state_of(blockIdx.x, (int)threadIdx.x);
    const bool live = state < a.nstates;
    const unsigned y = blockIdx.y;
    // lanes past the last state read the last state and store nothing: every lane takes part in every cross-lane read
    const size_t off = kk_offset(live ? state : a.nstates - 1, 0, g);
    uint32_t w[KK_PLANES];
#pragma unroll
    for (int p = 0; p < KK_PLANES; ++p) w[p] = 0;
    for (int s = 0; s < a.k; ++s) {                                       // k, lam, rows: wave-uniform
        const uint32_t* row = reinterpret_cast<const uint32_t*>(a.rows[s] + (size_t)y * a.in_batch + off);
        const uint32_t lam = a.lam[s];
        uint32_t v[KK_PLANES];
#pragma unroll
        for (int p = 0; p < KK_PLANES; ++p) v[p] = row[16 * p];           // 25 loads in flight, one wait
#pragma unroll
        for (int p = 0; p < KK_PLANES; ++p) {
            GF2P8::acc acc;
            acc.a = w[p];
            f.acc_mac(acc, lam, v[p]);
            w[p] = f.acc_reduce(acc);
        }
    }
    w[0] = f.add(w[0], kk_iota_word(a.rc, g));
    uint32_t o[KK_PLANES];
    if (a.apply_round) {
        uint32_t C[5];
#pragma unroll
        for (int x = 0; x < 5; ++x) C[x] = f.add(f.add(f.add(w[x], w[5 + x]), f.add(w[10 + x], w[15 + x])), w[20 + x]);
        uint32_t C1[5];
#pragma unroll
        for (int x = 0; x < 5; ++x) C1[x] = kk_rot(C[x], 1, g);
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const uint32_t D = f.add(C[(x + 4) % 5], C1[(x + 1) % 5]);
#pragma unroll
            for (int yy = 0; yy < 5; ++yy) w[5 * yy + x] = f.add(w[5 * yy + x], D);
        }
        uint32_t b[KK_PLANES];
#pragma unroll
        for (int P = 0; P < KK_PLANES; ++P) b[P] = kk_rot(w[kk_src_plane(P)], kk_src_rot(P), g);
        const uint32_t one = 0x01010101u;
#pragma unroll
        for (int yy = 0; yy < 5; ++yy)
#pragma unroll
            for (int x = 0; x < 5; ++x)
                o[5 * yy + x] = f.add(b[5 * yy + x], f.mul(f.add(b[5 * yy + (x + 1) % 5], one), b[5 * yy + (x + 2) % 5]));
    } else {
#pragma unroll
        for (int p = 0; p < KK_PLANES; ++p) o[p] = w[p];
    }
    const size_t ooff = kk_offset(live ? state : 0, 0, g) + (size_t)y * a.out_batch;
    if constexpr (!SHARE) {
        if (live) {
            uint32_t* orow = reinterpret_cast<uint32_t*>(a.out + ooff);
#pragma unroll
            for (int p = 0; p < KK_PLANES; ++p) orow[16 * p] = o[p];
        }
    } else {
        ra.rk.nonce[1] += (uint32_t)y << 8;
        constexpr int NBLK = kk_nblk(T);
        const uint64_t ctr0 = kk_ctr(state, g, NBLK);
        uint32_t ks[16];
#pragma unroll
        for (int p = 0; p < KK_PLANES; ++p) {
            uint32_t c[T];
#pragma unroll
            for (int q = 0; q < T; ++q) {
                const int d = p * T + q;                                  // draw number: block d / 16, word d % 16
                if ((d & 15) == 0) {
                    const uint64_t ctr = ctr0 + (uint64_t)(d >> 4);
                    chacha_block(ra.rk.key, (uint32_t)ctr, (uint32_t)(ctr >> 32), ra.rk.nonce[0], ra.rk.nonce[1], (int)ra.rk.rounds, ks);
                }
                c[q] = ks[d & 15] & f.emask;
            }
#pragma unroll
            for (int j = 0; j < M; ++j) {
                uint32_t h = c[T - 1];
#pragma unroll
                for (int q = T - 2; q >= 0; --q) h = f.muladd_small(h, (uint32_t)(j + 1), c[q]);
                const uint32_t share = f.muladd_small(h, (uint32_t)(j + 1), o[p]);
                if (live) reinterpret_cast<uint32_t*>(a.out + (size_t)j * a.share_stride + ooff)[16 * p] = share;
            }
        }
        rng_state_release(ra);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------
inline bool kk_fill_args(const GF2P8& f, KeccakArgs& a, const void* const* rows, const uint64_t* lam2, int k, size_t in_batch,
                         int iota_round, int apply_round, void* out, size_t nstates) {
    if (f.n < 1 || f.n > 8 || k < 1 || k > KK_MAX_K || iota_round < -1 || iota_round >= KK_ROUNDS) return false;
    memset(&a, 0, sizeof(a));
    uintptr_t bits = (uintptr_t)out | in_batch;
    for (int s = 0; s < k; ++s) {
        a.rows[s] = (const uint8_t*)rows[s];
        a.lam[s] = (uint32_t)(lam2[2 * s] & 0xffu);
        bits |= (uintptr_t)rows[s];
    }
    if (bits & 3) return false;
    a.k = k;
    a.apply_round = apply_round ? 1 : 0;
    a.in_batch = in_batch;
    a.out = (uint8_t*)out;
    a.rc = iota_round >= 0 ? kk_round_constant(iota_round) : 0;
    a.nstates = nstates;
    return true;
}

inline LaunchStatus ffgpu_launch_keccak_local_impl(const void* policy, const void* const* rows, const uint64_t* lam2, int k, size_t in_batch,
                                                   int nbatch, int iota_round, int apply_round, void* out, size_t out_batch,
                                                   size_t nstates, hipStream_t st) {
    const GF2P8& f = *reinterpret_cast<const GF2P8*>(policy);
    KeccakArgs a;
    if (!kk_fill_args(f, a, rows, lam2, k, in_batch, iota_round, apply_round, out, nstates) || (out_batch & 3) || nbatch < 1 || nbatch > 255)
        return L_NOT_SUPPORTED;
    const KkPlan pl = kk_plan(nstates);
    if (!pl.ok) return L_NOT_SUPPORTED;
    a.out_batch = out_batch;
    RngArgs ra;
    memset(&ra, 0, sizeof(ra));
    hipLaunchKernelGGL((k_keccak<0, 0>), dim3(pl.grid, (unsigned)nbatch), dim3(KK_THREADS), 0, st, f, a, ra);
    return launched();
}

inline LaunchStatus ffgpu_launch_keccak_round_impl(const void* policy, const void* const* rows, const uint64_t* lam2, int k, size_t in_batch,
                                                   int iota_round, int t, int m, void* shares, size_t share_stride, size_t out_batch,
                                                   size_t nstates, hipStream_t st, const RngArgs* rng) {
    const GF2P8& f = *reinterpret_cast<const GF2P8*>(policy);
    if (!kk_pair_ok(m, t)) return L_NOT_SUPPORTED;
    if (t == 0)                                     // one party: no re-sharing, the round's output is its new share
        return ffgpu_launch_keccak_local_impl(policy, rows, lam2, k, in_batch, 1, iota_round, 1, shares, out_batch, nstates, st);
    if ((1u << f.n) <= (unsigned)m) return L_NOT_SUPPORTED;               // the parties' points 1..m must be field elements
    KeccakArgs a;
    if (!kk_fill_args(f, a, rows, lam2, k, in_batch, iota_round, 1, shares, nstates) || ((share_stride | out_batch) & 3)) return L_NOT_SUPPORTED;
    const KkPlan pl = kk_plan(nstates);
    if (!pl.ok) return L_NOT_SUPPORTED;
    a.out_batch = out_batch;
    a.share_stride = share_stride;
    const unsigned senders = (unsigned)(2 * t + 1);
    RngArgs ra = *rng;
    ra.release = (ra.dev_key && !ra.no_advance && (uint64_t)pl.grid * senders <= (uint64_t)RNG_RELEASE_MAX_GRID) ? 1 : 0;
#define KK_CASE(MM, TT)                                                                                                \
    if (m == MM && t == TT) {                                                                                          \
        hipLaunchKernelGGL((k_keccak<MM, TT>), dim3(pl.grid, senders), dim3(KK_THREADS), 0, st, f, a, ra);             \
        FFGPU_CHECK_LAUNCH();                                                                                          \
        if (ra.dev_key && !ra.release && !ra.no_advance)                                                               \
            hipLaunchKernelGGL((k_rng_advance<0>), dim3(1), dim3(1), 0, st, const_cast<RngKey*>(ra.dev_key), 1u);      \
        return launched();                                                                                             \
    }
    KK_CASE(3, 1) KK_CASE(4, 1) KK_CASE(5, 1) KK_CASE(5, 2) KK_CASE(6, 1) KK_CASE(6, 2) KK_CASE(7, 1) KK_CASE(7, 2) KK_CASE(7, 3)
#undef KK_CASE
    return L_NOT_SUPPORTED;
}

}  // namespace ffgpu
