// Host check of the two plain headers under the C boundary (mpyc_amd/csrc/api.hip), with g++:
//   * hostint.hpp: for every modulus on the command line (hexadecimal) it prints what api.hip derives from it -- the bit
//     length, the packed scalars 2^l, 2^(l-1), 2^-l, the exponents p - 2, (p - 1) / 2, (p + 1) / 2, (3p - 5) / 4 with
//     their quotient and remainder by 3, and 2^f, ((p + 1) / 2) 2^f mod p -- for tests/test_api_args_host.py to compare
//     against Python integers.  An even modulus stands for a group order 2^deg: bit length and q - 2 only.
//   * operands.hpp: the frame's answers on synthetic addresses (nothing is dereferenced); "operands ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../mpyc_amd/csrc/hostint.hpp"
#include "../mpyc_amd/csrc/operands.hpp"

using namespace ffgpu;

static U192 parse_hex(const char* s) {
    U192 v;
    const size_t len = std::strlen(s);
    for (size_t i = 0; i < len && i < 48; ++i) {
        const char c = s[len - 1 - i];
        const uint64_t d = c >= '0' && c <= '9' ? c - '0' : 10 + ((c | 32) - 'a');
        v.w[i / 16] |= d << (4 * (i % 16));
    }
    return v;
}
static void put(const U192& v) { std::printf(" %016llx%016llx%016llx", (unsigned long long)v.w[2], (unsigned long long)v.w[1], (unsigned long long)v.w[0]); }
static void put_exp(const char* name, const U192& e) {
    unsigned rem;
    const U192 q = e.div3(&rem);
    std::printf("%s", name);
    put(e);
    put(q);
    std::printf(" %u\n", rem);
}

static void integers(const U192& p) {
    std::printf("modulus");
    put(p);
    std::printf("\nbits %d\n", p.bits());
    int ones = 0;
    for (int i = 0; i < 192; ++i) ones += p.bit(i);
    std::printf("ones %d\n", ones);
    put_exp("pm2", p_minus_2(p));
    if (!p.bit(0)) return;
    const int limbs = p.bits() > 128 ? 3 : 2;              // (ffgpu_ctx_scalar_limbs)
    const int ls[4] = {1, 2, 63, 64};
    for (int l : ls) {
        uint64_t c[9];
        if (!pow2_consts(p, l, limbs, c)) {
            std::printf("l %d refused\n", l);
            continue;
        }
        std::printf("l %d", l);
        for (int s = 0; s < 3; ++s) put(U192(c + s * limbs, limbs));
        uint64_t rest = 0;
        for (int i = 3 * limbs; i < 9; ++i) rest |= c[i];
        std::printf(" %d\n", rest == 0);
    }
    put_exp("hb", half_below(p));
    put_exp("ha", half_above(p));
    if ((p.w[0] & 3) == 3) put_exp("e34", three_p_minus_5_over_4(p));
    const int fs[4] = {0, 1, 64, 191};
    for (int f : fs) {
        std::printf("f %d", f);
        put(U192(1).times_pow2_mod(f, p));
        put(half_above(p).times_pow2_mod(f, p));
        std::printf("\n");
    }
}

static const void* at(uintptr_t a) { return (const void*)a; }
static void* wr(uintptr_t a) { return (void*)a; }

#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                 \
        }                                                             \
    } while (0)

static int operands() {
    {   // an output touching the last byte of an input; next to it
        Operands o;
        o.in(at(0x1000), 16);
        o.out(wr(0x100f), 8);
        EXPECT(!o.ok());
        Operands q;
        q.in(at(0x1000), 16);
        q.out(wr(0x1010), 8);
        q.out(wr(0xff8), 8);
        EXPECT(q.ok());
    }
    {   // two outputs sharing one byte; an array updated in place is an output
        Operands o;
        o.out(wr(0x2000), 8);
        o.out(wr(0x2007), 8);
        EXPECT(!o.ok());
        Operands q;
        q.inout(wr(0x2000), 8);
        q.inout(wr(0x2008), 8);
        EXPECT(q.ok());
        q.in(at(0x2004), 1);
        EXPECT(!q.ok());
    }
    {   // empty ranges never overlap
        Operands o;
        o.in(at(0x3000), 64);
        o.in(at(0x3100), 0);
        o.out(wr(0x3010), 0);
        o.out(wr(0x3100), 16);
        o.out(wr(0x3108), 0);
        EXPECT(o.ok());
    }
    {   // a null required pointer, of every kind
        Operands a, b, c, d, e, f;
        a.in(nullptr, 8);
        b.out(nullptr, 8);
        c.inout(nullptr, 8);
        d.host(nullptr);
        e.in_rows(nullptr, 2, 8);
        f.out_rows(nullptr, 2, 8);
        EXPECT(!a.ok() && !b.ok() && !c.ok() && !d.ok() && !e.ok() && !f.ok());
        Operands g;
        g.in(nullptr, 0);                                   // (also when nothing lies behind it)
        EXPECT(!g.ok());
    }
    {   // a skipped optional pointer; one that is given takes part
        Operands o;
        o.in(at(0x4000), 8);
        o.in_opt(nullptr, 8);
        o.out_opt(nullptr, 8);
        o.out(wr(0x4008), 8);
        o.host(at(0x10));
        EXPECT(o.ok() && o.nin == 1 && o.nout == 1);
        o.in_opt(at(0x400c), 8);
        EXPECT(!o.ok());
        Operands q;
        q.in(at(0x4000), 8);
        q.out_opt(wr(0x4004), 8);
        EXPECT(!q.ok());
    }
    {   // a null inside a pointer array; none counted when the count is not positive
        const void* rows[3] = {at(0x5000), nullptr, at(0x5100)};
        Operands o;
        o.in_rows(rows, 3, 8);
        EXPECT(!o.ok());
        Operands q;
        q.in_rows(rows, 1, 8);
        q.in_rows(rows, 0, 8);
        q.in_rows(rows, -1, 8);
        EXPECT(q.ok() && q.nin == 1);
        void* outs[2] = {wr(0x5200), nullptr};
        Operands r;
        r.out_rows(outs, 2, 8);
        EXPECT(!r.ok());
    }
    {   // the exact alias: the same address accepted, one element further refused, another row refused
        const void* r[2] = {at(0x6000), at(0x6100)};
        void* same[2] = {wr(0x6000), wr(0x6100)};
        void* apart[2] = {wr(0x6200), wr(0x6100)};
        void* shifted[2] = {wr(0x6008), wr(0x6100)};
        void* swapped[2] = {wr(0x6100), wr(0x6000)};
        void* twice[2] = {wr(0x6000), wr(0x6000)};
        void* const* tries[5] = {same, apart, shifted, swapped, twice};
        const bool want[5] = {true, true, false, false, false};
        for (int t = 0; t < 5; ++t) {
            Operands o;
            o.in(at(0x6800), 64);
            int first = -1;
            o.in_rows(r, 2, 64, &first);
            EXPECT(first == 1);
            o.out_rows(tries[t], 2, 64, first);
            EXPECT(o.ok() == want[t]);
        }
        Operands o;                                         // without the allowance the same address is an overlap
        o.in_rows(r, 2, 64);
        o.out_rows(same, 2, 64);
        EXPECT(!o.ok());
        Operands q;                                         // and the allowance names one input, not the address
        q.in(at(0x6000), 64);
        int first = -1;
        q.in_rows(r + 1, 1, 64, &first).out(wr(0x6000), 64, first);
        EXPECT(!q.ok());
    }
    {   // capacity: the last array that fits, one more of either kind
        Operands o;
        for (int i = 0; i < Operands::MAX_IN; ++i) o.in(at(0x100000 + 16 * (uintptr_t)i), 16);
        for (int i = 0; i < Operands::MAX_OUT; ++i) o.out(wr(0x200000 + 16 * (uintptr_t)i), 16);
        EXPECT(o.ok() && o.nin == Operands::MAX_IN && o.nout == Operands::MAX_OUT);
        Operands a = o, b = o, c = o;
        a.in(at(0x300000), 16);
        b.out(wr(0x300000), 16);
        c.in_opt(at(0x300000), 16);
        EXPECT(!a.ok() && !b.ok() && !c.ok());
        EXPECT(a.nin == Operands::MAX_IN && b.nout == Operands::MAX_OUT);
        static const void* many[Operands::MAX_IN + 5];
        for (int i = 0; i < Operands::MAX_IN + 5; ++i) many[i] = at(0x400000 + 16 * (uintptr_t)i);
        Operands d;
        d.in_rows(many, Operands::MAX_IN + 5, 16);
        EXPECT(!d.ok());
        Operands e;
        e.out_rows((void* const*)many, Operands::MAX_OUT + 1, 16);
        EXPECT(!e.ok());
    }
    std::printf("operands ok\n");
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) integers(parse_hex(argv[i]));
    return operands();
}
