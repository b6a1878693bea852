// hostint.hpp -- one unsigned 192-bit host integer: the arithmetic api.hip does on a context's modulus (bit length, the
// exponents p - 2, (p - 1) / 2, (p + 1) / 2 and (3p - 5) / 4, the scalars 2^l, 2^-l and ((p + 1) / 2) 2^f mod p, the
// quotient by 3 of an exponent).  Plain C++ (no HIP): tests/api_args_check.cpp drives it with g++ against Python integers.
// The modulus limbs of a context are zero-padded to three, so every field goes through this one three-limb path.
// No operation allocates; none is on a path that runs per element.
#pragma once
#include <stdint.h>

namespace ffgpu {

struct U192 {
    uint64_t w[3];     // little-endian limbs

    U192(uint64_t lo = 0) : w{lo, 0, 0} {}
    U192(const uint64_t* limbs, int n) : w{limbs[0], n > 1 ? limbs[1] : 0, n > 2 ? limbs[2] : 0} {}
    static U192 pow2(int k) {                                  // 2^k, 0 <= k < 192
        U192 r;
        r.w[k >> 6] = 1ull << (k & 63);
        return r;
    }

    int bits() const {                                         // bit length; 0 for 0
        for (int i = 2; i >= 0; --i)
            if (w[i]) return 64 * i + 64 - __builtin_clzll(w[i]);
        return 0;
    }
    bool bit(int i) const { return (w[i >> 6] >> (i & 63)) & 1; }
    bool operator>=(const U192& o) const {
        for (int i = 2; i > 0; --i)
            if (w[i] != o.w[i]) return w[i] > o.w[i];
        return w[0] >= o.w[0];
    }

    // x + y; *carry (if given) gets bit 192 of the sum
    U192 add(const U192& y, unsigned* carry = nullptr) const {
        U192 r;
        unsigned __int128 c = 0;
        for (int i = 0; i < 3; ++i) {
            c += (unsigned __int128)w[i] + y.w[i];
            r.w[i] = (uint64_t)c;
            c >>= 64;
        }
        if (carry) *carry = (unsigned)c;
        return r;
    }
    U192 sub(const U192& y) const {                            // x - y, x >= y
        U192 r;
        uint64_t borrow = 0;
        for (int i = 0; i < 3; ++i) {
            const unsigned __int128 d = (unsigned __int128)w[i] - y.w[i] - borrow;
            r.w[i] = (uint64_t)d;
            borrow = (uint64_t)(d >> 64) & 1;
        }
        return r;
    }
    U192 shr(int k, unsigned top = 0) const {                  // x >> k, 0 <= k < 64; `top` (0 or 1) comes in as bit 192
        if (k == 0) return *this;
        U192 r;
        r.w[0] = (w[0] >> k) | (w[1] << (64 - k));
        r.w[1] = (w[1] >> k) | (w[2] << (64 - k));
        r.w[2] = (w[2] >> k) | ((uint64_t)top << (64 - k));
        return r;
    }
    U192 div3(unsigned* rem) const {                           // x / 3 and x % 3
        U192 q;
        unsigned __int128 r = 0;
        for (int i = 2; i >= 0; --i) {
            const unsigned __int128 cur = (r << 64) | w[i];
            q.w[i] = (uint64_t)(cur / 3);
            r = cur % 3;
        }
        *rem = (unsigned)r;
        return q;
    }

    // modulo an odd p, for x < p
    U192 halve_mod(const U192& p) const {                      // x / 2 mod p: (x + p) / 2 when x is odd
        if (!(w[0] & 1)) return shr(1);
        unsigned carry;
        const U192 s = add(p, &carry);
        return s.shr(1, carry);
    }
    U192 double_mod(const U192& p) const {                     // 2 x mod p
        unsigned carry;
        const U192 d = add(*this, &carry);
        return carry || d >= p ? d.sub(p) : d;                 // (with the carry the wrapped difference is the right one)
    }
    U192 times_pow2_mod(int k, const U192& p) const {          // x 2^k mod p, k >= 0
        U192 r = *this;
        for (int i = 0; i < k; ++i) r = r.double_mod(p);
        return r;
    }
    static U192 inv_pow2_mod(int k, const U192& p) {           // 2^-k mod p, k >= 0
        U192 r(1);
        for (int i = 0; i < k; ++i) r = r.halve_mod(p);
        return r;
    }

    // a host scalar of `limbs` limbs, as the launchers read a packed array of them (the value fits)
    void store(uint64_t* out, int limbs) const {
        for (int i = 0; i < limbs; ++i) out[i] = w[i];
    }
};

// 2^l, 2^(l-1) and 2^-l mod p as three host scalars of `limbs` limbs each, packed (the rest of out[9] is zero); false
// unless 1 <= l <= bit_length(p) - 2: the three are then field elements, 2^l < p / 2
inline bool pow2_consts(const U192& p, int l, int limbs, uint64_t out[9]) {
    if (l < 1 || l > p.bits() - 2) return false;
    for (int i = 0; i < 9; ++i) out[i] = 0;
    U192::pow2(l).store(out, limbs);
    U192::pow2(l - 1).store(out + limbs, limbs);
    U192::inv_pow2_mod(l, p).store(out + 2 * limbs, limbs);
    return true;
}

// the exponents the entries derive from an odd prime p (p_minus_2 also from a group order q >= 2)
inline U192 p_minus_2(const U192& p) { return p.sub(2); }
inline U192 half_below(const U192& p) { return p.sub(1).shr(1); }            // (p - 1) / 2, the Legendre exponent
inline U192 half_above(const U192& p) { return p.shr(1).add(1); }            // (p + 1) / 2
inline U192 three_p_minus_5_over_4(const U192& p) { return p.sub(2).sub(p.sub(3).shr(2)); }   // p = 3 mod 4: p - 2 - (p - 3) / 4

}  // namespace ffgpu
