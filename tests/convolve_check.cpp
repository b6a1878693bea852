// g++ check of the convolution kernel's index arithmetic (mpyc_amd/csrc/convolve_geom.hpp): a host walk of k_convolve's
// loops -- tiles, tap range, chunks, one staged element per thread, tap groups, flush cadence, the final sum over the
// groups, for both tile shapes -- with the PM64 Mersenne policy of fields.hpp, for every (na, nv) up to 300 x 300, against
// the plain double loop.
// Prints "convolve ok" and exits 0, or names the first mismatch and exits 1.  Driven by tests/test_convolve_host.py.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include "../mpyc_amd/csrc/fields.hpp"
#include "../mpyc_amd/csrc/convolve_geom.hpp"

using namespace ffgpu;

typedef PM64<false, true> F;            // p = 2^61 - 1
enum { FLUSH = 192 };                   // DotAcc<F>::FLUSH for a policy without digit accumulators (kernels.hpp)

static F make_field() {
    F f;
    f.k = 61;
    f.c = 1;
    f.mask = (1ull << 61) - 1;
    f.p = f.mask;
    return f;
}

// what one workgroup of k_convolve<F, S> does for the tile starting at k0; flush: terms an accumulator may hold
template <class S>
static void tile(const F& f, const std::vector<uint64_t>& a, const std::vector<uint64_t>& v, size_t k0, int flush,
                 std::vector<uint64_t>& out, long& flushes, int& worst) {
    const size_t na = a.size(), nv = v.size(), nout = na + nv - 1;
    size_t jlo, jhi;
    conv_tap_range(k0, S::TO, na, nv, jlo, jhi);
    static F::acc acc[S::THREADS][S::R];
    static uint64_t tot[S::THREADS][S::R];
    static int terms[S::THREADS][S::R];
    uint64_t Ws[S::WIN], Ts[S::TV];
    for (int t = 0; t < S::THREADS; ++t)
        for (int r = 0; r < S::R; ++r) {
            f.acc_zero(acc[t][r]);
            terms[t][r] = 0;
        }
    bool have = false;
    int since = 0;
    for (size_t j0 = jlo; j0 < jhi; j0 += S::TV) {
        for (int t = 0; t < S::THREADS; ++t) {             // staging: one element per thread
            if (t < S::WIN) {
                const int64_t idx = conv_win_index(k0, j0, S::TV, t);
                Ws[t] = idx >= 0 && idx < (int64_t)na ? a[(size_t)idx] : 0;
            } else if (t >= S::THREADS - S::TV) {
                const size_t j = j0 + (size_t)(t - (S::THREADS - S::TV));
                Ts[t - (S::THREADS - S::TV)] = j < jhi ? v[j] : 0;
            }
        }
        const int tv = jhi - j0 < (size_t)S::TV ? (int)(jhi - j0) : (int)S::TV;
        for (int t = 0; t < S::THREADS; ++t) {
            const int o = t % S::OL, g = t / S::OL;
            for (int jj = g; jj < tv; jj += S::G)
                for (int r = 0; r < S::R; ++r) {
                    const int slot = conv_win_slot(o + S::OL * r, jj, S::TV);
                    if (slot < 0 || slot >= S::WIN) {
                        printf("FAILED: window slot %d out of range\n", slot);
                        exit(1);
                    }
                    f.acc_mac(acc[t][r], Ts[jj], Ws[slot]);
                    if (++terms[t][r] > worst) worst = terms[t][r];
                }
        }
        since += S::PER;
        if (conv_flush_due(since, S::PER, flush)) {
            for (int t = 0; t < S::THREADS; ++t)
                for (int r = 0; r < S::R; ++r) {
                    const uint64_t part = f.acc_reduce(acc[t][r]);
                    tot[t][r] = have ? f.add(tot[t][r], part) : part;
                    f.acc_zero(acc[t][r]);
                    terms[t][r] = 0;
                }
            have = true;
            since = 0;
            ++flushes;
        }
    }
    static uint64_t red[S::G][S::TO];
    for (int t = 0; t < S::THREADS; ++t)
        for (int r = 0; r < S::R; ++r) {
            uint64_t part = f.acc_reduce(acc[t][r]);
            if (have) part = f.add(tot[t][r], part);
            red[t / S::OL][t % S::OL + S::OL * r] = part;
        }
    for (int i = 0; i < S::TO; ++i) {
        uint64_t s = red[0][i];
        for (int q = 1; q < S::G; ++q) s = f.add(s, red[q][i]);
        if (k0 + (size_t)i < nout) out[k0 + (size_t)i] = s;
    }
}

static uint64_t next_value(uint64_t& state, uint64_t p) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t x = state >> 3;
    return (state >> 61) == 0 ? p - 1 : x % p;             // one value in eight is p - 1
}

template <class S>
static int run(const F& f, size_t na, size_t nv, int flush, uint64_t& state, long& flushes, int& worst) {
    std::vector<uint64_t> a(na), v(nv), out(na + nv - 1, ~0ull);
    for (auto& x : a) x = next_value(state, f.p);
    for (auto& x : v) x = next_value(state, f.p);
    const size_t tiles = conv_tiles(na + nv - 1, S::TO);
    for (size_t b = 0; b < tiles; ++b) tile<S>(f, a, v, b * S::TO, flush, out, flushes, worst);
    for (size_t k = 0; k < na + nv - 1; ++k) {
        unsigned __int128 s = 0;
        for (size_t j = 0; j < nv; ++j)
            if (k >= j && k - j < na) {
                s += (unsigned __int128)a[k - j] * v[j];              // a product is below 2^122
                if (s >> 127) s %= f.p;
            }
        if ((uint64_t)(s % f.p) != out[k]) {
            printf("FAILED: OL=%d na=%zu nv=%zu flush=%d k=%zu\n", (int)S::OL, na, nv, flush, k);
            return 1;
        }
    }
    return 0;
}

template <class S>
static int walk(const F& f, uint64_t& state) {
    long flushes = 0;
    int worst = 0;
    // the kernel's cadence: every (na, nv) with na >= nv (the C entry swaps the operands)
    for (size_t na = 1; na <= 300; ++na)
        for (size_t nv = 1; nv <= na; ++nv)
            if (run<S>(f, na, nv, FLUSH, state, flushes, worst)) return 1;
    if (worst > FLUSH) {
        printf("FAILED: %d terms in an accumulator that holds %d\n", worst, (int)FLUSH);
        return 1;
    }
    // 300 taps give an accumulator at most 75 terms, so the bound of 192 never forces a flush above: walk the same sizes
    // with accumulators that hold only 32 terms (the digit accumulators' bound) and 2 PER terms (the tightest the
    // cadence allows) to cover the flush path itself
    for (int flush : {32, 2 * (int)S::PER}) {
        const long before = flushes;
        worst = 0;
        for (size_t na = 1; na <= 300; na += 13)
            for (size_t nv = 1; nv <= na; ++nv)
                if (run<S>(f, na, nv, flush, state, flushes, worst)) return 1;
        if ((flushes == before && flush == 2 * (int)S::PER) || worst > flush) {
            printf("FAILED: flush path (bound %d, flushes %ld, worst %d)\n", flush, flushes - before, worst);
            return 1;
        }
    }
    return 0;
}

int main() {
    const F f = make_field();
    uint64_t state = 20261016;
    if (walk<ConvWide>(f, state) || walk<ConvNarrow>(f, state)) return 1;
    // shape choice: wide from per_cu tiles per compute unit on
    if (!conv_use_wide(256 * 2 * 128 - 127, 256, 2) || conv_use_wide(256 * 2 * 128 - 128, 256, 2) || !conv_use_wide(1, 256, 0) ||
        conv_use_wide((size_t)1 << 40, 256, 1 << 30)) {
        printf("FAILED: shape choice\n");
        return 1;
    }
    printf("convolve ok\n");
    return 0;
}
