// launch.hpp -- host side of the kernels: per-policy launcher table (FieldOps) behind the C ABI of api.hip.
// Included by kernels.hpp.  The launchers of the secure protocols' local steps are in launch_secure.hpp, included at the end.
#pragma once

namespace ffgpu {

// ---- launch plumbing -------------------------------------------------------
// The library's launch shape and run-time switches (one table: INTEGRATION.md section 6).  Filled ONCE per context, when it
// is created (ffgpu_ctx_create), and carried by it: no getenv and no device query on any call path.
struct LaunchCfg {
    int num_cu;             // compute units of the context's device
    int blocks_per_cu;      // FFGPU_BLOCKS_PER_CU: cap of the streaming grids; 0 = uncapped: one 16-byte pack per thread (default, measured best)
    int mm_mfma;            // FFGPU_MM_MFMA=0: dense products stay on the VALU kernel (cross-checks of the matrix-core path)
    double mm_mfma_min;     // FFGPU_MM_MFMA_MIN: smallest M*N*K that goes to the matrix cores (default 8e7)
    int gf2w_bitsliced;     // FFGPU_GF2W_BITSLICED=0: GF(2^64) products through the multiplier kernel only
    int conv_wide_per_cu;   // FFGPU_CONV_WIDE_PER_CU: 128-output tiles per compute unit from which ffgpu_convolve takes its wide shape
                            // (default 2; 0: always wide, a huge value: always narrow -- tests drive both shapes at small sizes)
    int scan_geom;          // FFGPU_SCAN_GEOM: 0 = ffgpu_scan / ffgpu_axis_reduce choose their geometry (scan_geom.hpp), 1 = always the
                            // column walk, 2 = always row tiles (tests drive both at small sizes; never changes a result)
    int scan_tile_threads;  // FFGPU_SCAN_TILE_THREADS: threads of a row-tile workgroup that hold elements (default: all 256; tests
                            // lower it so that small arrays span many tiles)
    int mm_stack_loop_min;  // FFGPU_MM_STACK_LOOP_MIN: ffgpu_matmul_stack loops over the single-product launcher from this M*N*K per
                            // matrix on (0: always); below it the whole stack is one launch of the stack kernels (matmul_stack.hpp)
    int handoff;            // FFGPU_HANDOFF=0: every streamed output non-temporal (no hand-off tracking, handoff.hpp)
    int policy;             // PER LAUNCH, never set in the context's copy: the launch's cache policy word (CachePolicy, kernels.hpp) --
                            // how to store outputs that feed the next launch on the stream (handoff.hpp; api.hip hands the
                            // launcher a copy); 0: every access nt
};

// What a launcher reports.  One value per meaning; api.hip maps them to FFGPU_* in one place (status_of).
enum LaunchCode {
    L_OK = 0,
    L_BAD_ARG,         // an argument the entry point should have refused
    L_NOT_SUPPORTED,   // sizes outside what the kernels are built for
    L_DECLINED,        // this route does not serve the call: the caller takes another one (never leaves the library)
    L_PLAN_REFUSED,    // scan_plan() refuses the sizes
    L_WS_TOO_SMALL,    // the caller's workspace is smaller than the plan needs
    L_HIP_ERROR        // a launch failed: `hip` says how
};
struct LaunchStatus {
    LaunchCode code;
    hipError_t hip;
    LaunchStatus(LaunchCode c = L_OK, hipError_t e = hipSuccess) : code(c), hip(e) {}
    bool ok() const { return code == L_OK; }
};
// the status of the launches enqueued so far by this call
inline LaunchStatus launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LaunchStatus() : LaunchStatus(L_HIP_ERROR, e);
}
#define FFGPU_CHECK_LAUNCH()                      \
    do {                                          \
        const LaunchStatus s__ = launched();      \
        if (!s__.ok()) return s__;                \
    } while (0)

inline unsigned grid_for(size_t iters, const LaunchCfg& lc) {
    size_t want = (iters + BLOCK - 1) / BLOCK;
    size_t cap = lc.blocks_per_cu > 0 ? (size_t)lc.blocks_per_cu * (size_t)lc.num_cu : (size_t)0x7fffffff;
    if (want < 1) want = 1;
    return (unsigned)(want < cap ? want : cap);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the launchers of the secure protocols' local steps have a table and a header of their own (launch_secure.hpp)
struct SecureOps;
template <class F>
const SecureOps* secure_ops();

// host-side table of launchers for one policy type; the context stores the
// policy blob and a pointer to this table.
struct FieldOps {
    LaunchStatus (*ew2)(const void* F, const LaunchCfg& lc, int op, const void* a, const void* b, void* o, size_t n,
               hipStream_t st);
    LaunchStatus (*ew1)(const void* F, const LaunchCfg& lc, int op, const void* a, const uint64_t* scalar2, void* o,
               size_t n, hipStream_t st);
    LaunchStatus (*muladd)(const void* F, const LaunchCfg& lc, const void* a, const void* b, const void* c, void* o,
                  size_t n, hipStream_t st);
    // coef == nullptr && rng != nullptr: coefficients are drawn in-kernel from the keystream
    LaunchStatus (*split)(const void* F, const LaunchCfg& lc, const void* a, const void* b, const void* coef,
                 size_t cstride, int t, int m, void* out, size_t ostride, size_t n, hipStream_t st,
                 const RngArgs* rng);
    LaunchStatus (*rng_coeffs)(const void* F, const LaunchCfg& lc, void* coef, size_t cstride, int t, size_t n, hipStream_t st,
                      const RngArgs* rng);
    LaunchStatus (*recombine)(const void* F, const LaunchCfg& lc, const void* const* rows, const uint64_t* lam2, int k,
                     int w, void* out, size_t ostride, size_t n, hipStream_t st);
    LaunchStatus (*pow)(const void* F, const LaunchCfg& lc, const void* a, const ExpArgs* ex, void* out, size_t n, hipStream_t st);
    LaunchStatus (*inv)(const void* F, const LaunchCfg& lc, const void* a, const ExpArgs* ex, void* out, size_t n, int* flag,
               hipStream_t st);
    LaunchStatus (*matmul)(const void* F, const LaunchCfg& lc, const void* A, size_t lda, const void* B, size_t ldb, void* C,
                  size_t ldc, int M, int K, int N, void* workspace, size_t workspace_bytes, hipStream_t st);
    LaunchStatus (*dot)(const void* F, const LaunchCfg& lc, const void* a, const void* b, void* out, void* workspace, size_t n,
               hipStream_t st);
    // nbatch > 1: gridDim.y independent gates in one launch, operands / outputs of gate y at element offsets y*yA, y*yB, y*yO
    LaunchStatus (*gate)(const void* F, const LaunchCfg& lc, const void* const* rowsA, const uint64_t* lamA2, int kA,
                const void* const* rowsB, const uint64_t* lamB2, int kB, int t, int m, void* out, size_t ostride,
                size_t n, hipStream_t st, const RngArgs* rng, int nbatch, size_t yA, size_t yB, size_t yO);
    LaunchStatus (*sqrt_cl)(const void* F, const LaunchCfg& lc, const void* a, const ExpArgs* eleg, const ExpArgs* elad, void* out, size_t n,
                   hipStream_t st);
    LaunchStatus (*gauss)(const void* F, const LaunchCfg& lc, void* A, int n, int ncols, size_t batch, int det_mode, const ExpArgs* ex,
                 void* det, int* sing, hipStream_t st);
    LaunchStatus (*group_matvec)(const void* F, const LaunchCfg& lc, const uint64_t* m2, const uint64_t* bias2, int r, int g,
                        const void* in, void* out, size_t ngroups, hipStream_t st);
    LaunchStatus (*beaver)(const void* F, const LaunchCfg& lc, const void* z, const void* x, const void* y, const void* d, const void* e,
                  void* out, int add_de, size_t n, hipStream_t st);
    LaunchStatus (*prss)(const void* F, const LaunchCfg& lc, const void* const* streams, int ks, int d, int l, int mask_bits,
                const uint64_t* weights2, const uint64_t* r2, int accumulate, void* out, size_t n, hipStream_t st);
    // keys40: ks x (32-byte ChaCha key + 8-byte nonce)
    LaunchStatus (*prss_chacha)(const void* F, const LaunchCfg& lc, const uint8_t* keys40, int ks, int d, int l, int mask_bits, int rounds,
                       const uint64_t* weights2, const uint64_t* r2, int accumulate, void* out, size_t n, hipStream_t st);
    // C[b] = A[b] @ B[b], b < batch, in one launch without workspace; strides in elements, 0 = one matrix shared by the stack
    // (L_PLAN_REFUSED: stack_plan() refuses the sizes)
    LaunchStatus (*matmul_stack)(const void* F, const LaunchCfg& lc, const void* A, size_t lda, size_t sa, const void* B, size_t ldb,
                        size_t sb, void* C, size_t ldc, size_t sc, int M, int K, int N, size_t batch, hipStream_t st);
    int stack_slot;         // LDS bytes of one staged element of the stack kernels (stack_plan's slot_bytes)
    // full convolution, na >= nv >= 1, out: na + nv - 1 elements
    LaunchStatus (*convolve)(const void* F, const LaunchCfg& lc, const void* a, size_t na, const void* v, size_t nv, void* out,
                    hipStream_t st);
    // inclusive scan / reduction along k of a contiguous (outer, k, inner) array with field addition (mul = 0) or
    // multiplication; workspace: scan_plan().ws_elems elements (L_PLAN_REFUSED, L_WS_TOO_SMALL)
    LaunchStatus (*scan)(const void* F, const LaunchCfg& lc, int mul, const void* a, void* out, size_t outer, size_t k, size_t inner,
                int with_initial, void* workspace, size_t workspace_bytes, hipStream_t st);
    LaunchStatus (*axis_reduce)(const void* F, const LaunchCfg& lc, int mul, const void* a, void* out, size_t outer, size_t k,
                       size_t inner, void* workspace, size_t workspace_bytes, hipStream_t st);
    // local steps of the secure protocols (launch_secure.hpp); nullptr for a GF(2^n) policy
    const SecureOps* secure;
};

// Host scalars (Lagrange coefficients, constants, matrix entries) cross the C ABI as little-endian 64-bit limbs:
// 2 per scalar, 3 for the three-limb prime fields (ffgpu_ctx_scalar_limbs).
template <class F>
constexpr int scalar_limbs() {
    return sizeof(typename F::word) == 24 ? 3 : 2;
}
// scalar number idx of a host array -> policy word (broadcast for packed fields)
template <class F>
inline typename F::word word_at(const F& f, const uint64_t* base, size_t idx);
template <class F>
inline typename F::word word_from_limbs(const F& f, uint64_t lo, uint64_t hi) {
    if constexpr (sizeof(typename F::word) == 24) {
        typename F::word w;
        w.lo = lo;
        w.mid = hi;
        w.hi = 0;
        return w;
    } else if constexpr (sizeof(typename F::word) == 16) {
        typename F::word w;
        w.lo = lo;
        w.hi = hi;
        return w;
    } else if constexpr (F::EPW == 4) {
        uint32_t b = (uint32_t)(lo & 0xffu);
        return b * 0x01010101u;
    } else {
        return (typename F::word)lo;
    }
}
template <class F>
inline typename F::word word_at(const F& f, const uint64_t* base, size_t idx) {
    constexpr int SL = scalar_limbs<F>();
    const uint64_t* l = base + idx * SL;
    if constexpr (SL == 3) {
        typename F::word w;
        w.lo = l[0];
        w.mid = l[1];
        w.hi = l[2];
        return w;
    } else {
        return word_from_limbs<F>(f, l[0], l[1]);
    }
}

// Run-time integer -> template parameter: calls fn(std::integral_constant<int, V>()) for the V of the list that equals v;
// false when none does.  Only the listed values are instantiated.  (Kernels are launched from named member functions
// that fn calls, see the note at launch_glds.)
template <int LO, int... I>
constexpr auto int_range_(std::integer_sequence<int, I...>) { return std::integer_sequence<int, LO + I...>(); }
template <int LO, int HI>
using IntRange = decltype(int_range_<LO>(std::make_integer_sequence<int, HI - LO + 1>()));
template <int... V, class Fn>
inline bool dispatch_int(std::integer_sequence<int, V...>, int v, Fn&& fn) {
    return ((v == V ? (fn(std::integral_constant<int, V>()), true) : false) || ...);
}

// Does an M x K x N product over a prime field go to the matrix cores, and with how many bytes of digit planes
// (`digits` int8 planes per operand, padded to whole tiles)?  0: it stays on the vector ALUs.  The one copy of this
// decision: ffgpu_matmul sizes the scratch with it, Launchers::matmul takes the route with it.
// (from 9 rows / columns on: the tiles are padded to 64 -- a batch of 9..63 rows against 4096 x 4096 takes the 88 us of
// 64 rows instead of 670-690 us on the vector ALUs)
// (restated in tests/matmul_contract.py -- move the two together)
inline size_t mfma_plane_bytes(const LaunchCfg& lc, size_t digits, size_t M, size_t K, size_t N) {
    if (!lc.mm_mfma || M <= SKINNY_MAX || N <= SKINNY_MAX || K < 64 || (double)M * N * K < lc.mm_mfma_min) return 0;
    const size_t Mp = (M + 63) / 64 * 64, Np = (N + 63) / 64 * 64, Kp = (K + 31) / 32 * 32;
    return digits * (Mp + Np) * Kp;
}

template <class F>
struct Launchers {
    typedef typename F::elem E;
    typedef typename F::word W;
    enum { EPV = Pack<W>::N * F::EPW };  // elements per pack (one lane's access)
    // dwordx3 needs dword alignment only; three-limb (24-byte) elements are moved by the WAVE as dwordx4 (kernels.hpp, ldgw)
    enum { PACK_ALIGN = sizeof(E) == 12 ? 4 : 16 };
    static bool al(const void* p) { return ((uintptr_t)p & (PACK_ALIGN - 1)) == 0; }
    static_assert(geom_pack(sizeof(E)) == (unsigned)EPV, "geom.hpp counts this field's pack");
    static_assert(geom_align(sizeof(E)) == (unsigned)PACK_ALIGN, "geom.hpp states this field's pack alignment");
    // packs that go through the vector loop of a kernel (the rest: its scalar tail): the rule of geom.hpp, 24-byte elements in
    // whole waves only
    static size_t nvec_of(size_t n, bool vec) { return stream_nvec(n, sizeof(E), vec); }
    // The streaming plan of a launch: nvec packs through the vector loop, one pack per thread up to the grid cap (one element
    // per thread when the operands do not allow packs).  The one place where nvec_of and grid_for meet: every launcher takes
    // its nvec from here, so 24-byte fields get whole waves whatever grid it then picks.
    // pol: the cache policy word of the launch (LaunchCfg::policy), which the vector loop obeys.
    struct Plan {
        size_t nvec;
        unsigned grid;
        int pol;
    };
    static Plan plan(size_t n, bool vec, const LaunchCfg& lc) {
        const size_t nvec = nvec_of(n, vec);
        return {nvec, grid_for(nvec ? nvec : n, lc), lc.policy};
    }
    // share generation with in-kernel coefficients (k_split RNG, the gate): the grouped loop serves up to 4 packs per thread
    // (RngLayout::G) on half as many threads as packs, a slightly larger grid is harmless; below ~2.6e5 packs it cannot
    // fill the chip and every thread takes one pack instead (ra.spread).  Small grids let the kernel's last workgroup
    // advance the device-resident nonce (ra.release, gy gates per launch counted); otherwise rng_advance follows.
    // (The 262144 packs at which the spread loop ends are named by tests/test_gpu_share_contract.py, SPREAD_MAX_PACKS: its
    // grouped-loop cases sit just above it.  Move the two together.)
    static Plan plan_rng(size_t n, bool vec, const LaunchCfg& lc, RngArgs& ra, unsigned gy = 1) {
        Plan p = plan(n, vec, lc);
        const bool spread = p.nvec > 0 && p.nvec < 262144;
        ra.spread = spread ? 1 : 0;
        if (p.nvec && !spread) p.grid = grid_for((n / EPV + 2) / 2, lc);
        ra.release = !ra.no_advance && (size_t)p.grid * gy <= RNG_RELEASE_MAX_GRID;
        return p;
    }
    // after an RNG launch: advance the device-resident nonce unless the kernel did (ra.release) or the caller will
    static void rng_advance(const RngArgs& ra, hipStream_t st) {
        if (ra.dev_key && !ra.release && !ra.no_advance)
            hipLaunchKernelGGL((k_rng_advance<0>), dim3(1), dim3(1), 0, st, const_cast<RngKey*>(ra.dev_key), 1u);
    }
    // (a member function, not a lambda inside `matmul`: clang does not emit the host stub of a kernel specialisation
    // that is only named inside a generic lambda's discarded-branch neighbourhood)
    template <bool BRAW>
    static void launch_glds(const F& f, dim3 grid, hipStream_t st, const int8_t* Ap, const int8_t* Bp, E* out, size_t out_ld, int M, int N,
                            int Kp, int kb, int ke, int acc_, int kslice, size_t zs, const E* Braw, size_t ldb, uint64_t pmod) {
        if constexpr (F::EPW == 1 && !F::BINARY && sizeof(E) == 8) {
            const size_t lds = (size_t)(BRAW ? 8 : 6) * GLDS_TILE;
            static bool attr_done = false;
            if (!attr_done) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_limb_gemm_glds<F, BRAW>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                attr_done = true;
            }
            hipLaunchKernelGGL((k_limb_gemm_glds<F, BRAW>), grid, dim3(BLOCK), lds, st, f, Ap, Bp, out, out_ld, M, N, Kp, kb, ke, acc_,
                               kslice, zs, Braw, ldb, pmod);
        }
    }
    // the policy blob of the context (FieldOps entries take it untyped)
    static const F& policy(const void* Fp) { return *reinterpret_cast<const F*>(Fp); }
    static bool stride_ok(size_t stride) { return (stride * sizeof(E)) % PACK_ALIGN == 0; }

    template <int OP>
    static void go_ew2(const F& f, const LaunchCfg& lc, const E* a, const E* b, E* o, size_t n, hipStream_t st) {
        const Plan p = plan(n, al(a) && al(b) && al(o), lc);
        constexpr int OCC = EwOccupancy<F, OP>::waves;
        // (streamed loads and stores carry the non-temporal hint: +4-8 %, profiles/r01_tuning.md; the un-hinted instantiations
        // that rounds 1-5 kept behind FFGPU_NT=0 for A/B runs are gone)
        if constexpr (OCC > 0)
            hipLaunchKernelGGL((k_ew2_occ<F, OP, true, OCC>), dim3(p.grid), dim3(BLOCK), 0, st, f, a, b, o, p.nvec, n, p.pol);
        else
            hipLaunchKernelGGL((k_ew2<F, OP, true>), dim3(p.grid), dim3(BLOCK), 0, st, f, a, b, o, p.nvec, n, p.pol);
    }
    static LaunchStatus ew2(const void* Fp, const LaunchCfg& lc, int op, const void* a, const void* b, void* o, size_t n,
                   hipStream_t st) {
        const F& f = policy(Fp);
        const E* A = (const E*)a;
        const E* B = (const E*)b;
        E* O = (E*)o;
        const bool known = dispatch_int(std::integer_sequence<int, OP_ADD, OP_SUB, OP_MUL>(), op,
                                        [&](auto o_) { go_ew2<decltype(o_)::value>(f, lc, A, B, O, n, st); });
        return known ? launched() : LaunchStatus(L_BAD_ARG);
    }

    template <int OP>
    static void go_ew1(const F& f, const LaunchCfg& lc, const E* a, W s, E* o, size_t n, hipStream_t st) {
        const Plan p = plan(n, al(a) && al(o), lc);
        hipLaunchKernelGGL((k_ew1<F, OP, true>), dim3(p.grid), dim3(BLOCK), 0, st, f, a, s, o, p.nvec, n, p.pol);
    }
    static LaunchStatus ew1(const void* Fp, const LaunchCfg& lc, int op, const void* a, const uint64_t* scalar2, void* o,
                   size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        W s = scalar2 ? word_at<F>(f, scalar2, 0) : word_from_limbs<F>(f, 0, 0);
        const E* A = (const E*)a;
        E* O = (E*)o;
        const bool known = dispatch_int(std::integer_sequence<int, OP_ADD, OP_RSUB, OP_MUL, OP_NEG, OP_REDUCE>(), op,
                                        [&](auto o_) { go_ew1<decltype(o_)::value>(f, lc, A, s, O, n, st); });
        return known ? launched() : LaunchStatus(L_BAD_ARG);
    }

    static LaunchStatus muladd(const void* Fp, const LaunchCfg& lc, const void* a, const void* b, const void* c, void* o,
                      size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const Plan p = plan(n, al(a) && al(b) && al(c) && al(o), lc);
        hipLaunchKernelGGL((k_muladd<F, true>), dim3(p.grid), dim3(BLOCK), 0, st, f, (const E*)a,
                           (const E*)b, (const E*)c, (E*)o, p.nvec, n, p.pol);
        return launched();
    }

    template <int T, bool FUSE, bool RNG, bool REC = false>
    static void go_split(const F& f, const Plan& p, const E* a, const E* b, const E* coef, size_t cstride, int m, E* out,
                         size_t ostride, size_t n, hipStream_t st, const RngArgs& ra, const GateSrc<F>& gs, unsigned gy = 1) {
        hipLaunchKernelGGL((k_split<F, T, FUSE, true, RNG, REC>), dim3(p.grid, gy), dim3(BLOCK), 0, st, f, a, b,
                           coef, cstride, m, out, ostride, p.nvec, n, ra, gs, p.pol);
    }
    template <bool FUSE, bool RNG>
    static LaunchStatus split_t(const F& f, const LaunchCfg& lc, const E* a, const E* b, const E* coef, size_t cstride,
                       int t, int m, E* out, size_t ostride, size_t n, hipStream_t st, const RngArgs& ra_in) {
        RngArgs ra = ra_in;
        if (t > MAXT) {
            const Plan p = RNG ? plan_rng(n, false, lc, ra) : plan(n, false, lc);
            hipLaunchKernelGGL((k_split_any<F, FUSE, RNG>), dim3(p.grid), dim3(BLOCK), 0, st, f, a, b, coef, cstride,
                               t, m, out, ostride, n, ra);
        } else {
            const bool vec = al(a) && (!FUSE || al(b)) && al(out) &&
                             (stride_ok(ostride) || m <= 1) &&
                             (RNG || t == 0 || (al(coef) && (stride_ok(cstride) || t <= 1)));
            const Plan p = RNG ? plan_rng(n, vec, lc, ra) : plan(n, vec, lc);
            GateSrc<F> gs;
            memset(&gs, 0, sizeof(gs));
            const bool known = dispatch_int(IntRange<0, MAXT>(), t, [&](auto t_) {     // (t = 0 draws nothing: one kernel for both)
                constexpr int T = decltype(t_)::value;
                go_split<T, FUSE, (T > 0 && RNG)>(f, p, a, b, coef, cstride, m, out, ostride, n, st, ra, gs);
            });
            if (!known) return L_BAD_ARG;
        }
        if (RNG && t > 0) rng_advance(ra, st);
        return L_OK;
    }
    // fused chain gate: both factors given as recombinations (GateSrc), product re-shared with the device CSPRNG
    static LaunchStatus gate(const void* Fp, const LaunchCfg& lc, const void* const* rowsA, const uint64_t* lamA2, int kA,
                    const void* const* rowsB, const uint64_t* lamB2, int kB, int t, int m, void* out, size_t ostride,
                    size_t n, hipStream_t st, const RngArgs* rng, int nbatch, size_t yA, size_t yB, size_t yO) {
        const F& f = policy(Fp);
        if (t < 1 || t > 3 || kA < 1 || kA > GATE_MAXK || kB < 0 || kB > GATE_MAXK || !rng) return L_NOT_SUPPORTED;
        if (nbatch < 1 || nbatch > 255) return L_NOT_SUPPORTED;
        GateSrc<F> gs;
        memset(&gs, 0, sizeof(gs));
        bool vec = al(out) && (stride_ok(ostride) || m <= 1);
        if (nbatch > 1) {
            gs.yA = yA;
            gs.yB = yB;
            gs.yO = yO;
            vec = vec && stride_ok(yA) && stride_ok(yO) && (kB == 0 || stride_ok(yB));
        }
        for (int j = 0; j < kA; ++j) {
            gs.rowsA[j] = (const E*)rowsA[j];
            gs.lamA[j] = f.prep(word_at<F>(f, lamA2, j));
            vec = vec && al(rowsA[j]);
        }
        for (int j = 0; j < kB; ++j) {
            gs.rowsB[j] = (const E*)rowsB[j];
            gs.lamB[j] = f.prep(word_at<F>(f, lamB2, j));
            vec = vec && al(rowsB[j]);
        }
        gs.kA = kA;
        gs.kB = kB;
        gs.square = kB == 0;
        constexpr int SLG = scalar_limbs<F>();
        gs.plainA = kA == 1 && lamA2[0] == 1 && lamA2[1] == 0 && (SLG < 3 || lamA2[SLG - 1] == 0);
        gs.plainB = kB == 1 && lamB2[0] == 1 && lamB2[1] == 0 && (SLG < 3 || lamB2[SLG - 1] == 0);
        RngArgs ra = *rng;
        const unsigned gy = (unsigned)nbatch;
        const Plan p = plan_rng(n, vec, lc, ra, gy);
        E* o = (E*)out;
        dispatch_int(IntRange<1, 3>(), t, [&](auto t_) {
            go_split<decltype(t_)::value, true, true, true>(f, p, nullptr, nullptr, nullptr, 0, m, o, ostride, n, st, ra, gs, gy);
        });
        rng_advance(ra, st);
        return launched();
    }
    static LaunchStatus split(const void* Fp, const LaunchCfg& lc, const void* a, const void* b, const void* coef,
                     size_t cstride, int t, int m, void* out, size_t ostride, size_t n, hipStream_t st,
                     const RngArgs* rng) {
        const F& f = policy(Fp);
        RngArgs ra;
        memset(&ra, 0, sizeof(ra));
        LaunchStatus rc;
        if (rng) {
            ra = *rng;
            rc = b ? split_t<true, true>(f, lc, (const E*)a, (const E*)b, nullptr, 0, t, m, (E*)out, ostride, n, st, ra)
                   : split_t<false, true>(f, lc, (const E*)a, nullptr, nullptr, 0, t, m, (E*)out, ostride, n, st, ra);
        } else {
            rc = b ? split_t<true, false>(f, lc, (const E*)a, (const E*)b, (const E*)coef, cstride, t, m, (E*)out,
                                          ostride, n, st, ra)
                   : split_t<false, false>(f, lc, (const E*)a, nullptr, (const E*)coef, cstride, t, m, (E*)out,
                                           ostride, n, st, ra);
        }
        return rc.ok() ? launched() : rc;
    }
    static LaunchStatus rng_coeffs(const void* Fp, const LaunchCfg& lc, void* coef, size_t cstride, int t, size_t n, hipStream_t st,
                          const RngArgs* rng) {
        const F& f = policy(Fp);
        E* C = (E*)coef;
        size_t npacks = (n + EPV - 1) / EPV;
        unsigned grid = grid_for(npacks, lc);
        if (t > MAXT) {
            hipLaunchKernelGGL((k_rng_coeffs_any<F>), dim3(grid), dim3(BLOCK), 0, st, f, C, cstride, t, n, *rng);
            return launched();
        }
        const size_t nvec = plan(n, al(coef) && (stride_ok(cstride) || t <= 1), lc).nvec;
        const bool known = dispatch_int(IntRange<1, MAXT>(), t, [&](auto t_) {
            hipLaunchKernelGGL((k_rng_coeffs<F, decltype(t_)::value>), dim3(grid), dim3(BLOCK), 0, st, f, C, cstride, nvec, n, *rng);
        });
        return known ? launched() : LaunchStatus(L_BAD_ARG);
    }

    template <int K>
    static void go_rec(const F& f, const LaunchCfg& lc, const void* const* rows, const uint64_t* lam2, int w,
                       E* out, size_t ostride, size_t n, hipStream_t st) {
        RecArgs<F, K> ra;
        bool vec = al(out) && (stride_ok(ostride) || w <= 1);
        for (int j = 0; j < K; ++j) {
            ra.rows[j] = (const E*)rows[j];
            vec = vec && al(rows[j]);
        }
        for (int r = 0; r < w; ++r)
            for (int j = 0; j < K; ++j) {
                ra.lam[r * K + j] = f.prep(word_at<F>(f, lam2, (size_t)r * K + j));
            }
        for (int i = w * K; i < MAXW * K; ++i) ra.lam[i] = ra.lam[0];
        const Plan p = plan(n, vec, lc);
        hipLaunchKernelGGL((k_recombine<F, K, true>), dim3(p.grid), dim3(BLOCK), 0, st, f, ra, w, out, ostride,
                           p.nvec, n, p.pol);
    }
    static LaunchStatus recombine(const void* Fp, const LaunchCfg& lc, const void* const* rows, const uint64_t* lam2, int k,
                         int w, void* out, size_t ostride, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        E* O = (E*)out;
        if (k > MAXK) {
            if (k > MAXK_ANY) return L_NOT_SUPPORTED;
            for (int r = 0; r < w; ++r) {
                RecArgsAny<F> ra;
                for (int j = 0; j < k; ++j) {
                    ra.rows[j] = (const E*)rows[j];
                    ra.lam[j] = f.prep(word_at<F>(f, lam2, (size_t)r * k + j));
                }
                for (int j = k; j < MAXK_ANY; ++j) {
                    ra.rows[j] = ra.rows[0];
                    ra.lam[j] = ra.lam[0];
                }
                unsigned grid = grid_for(n, lc);
                hipLaunchKernelGGL((k_recombine_any<F>), dim3(grid), dim3(BLOCK), 0, st, f, ra, k,
                                   O + (size_t)r * ostride, n);
            }
            return launched();
        }
        for (int r0 = 0; r0 < w; r0 += MAXW) {
            int wc = (w - r0) < MAXW ? (w - r0) : MAXW;
            const uint64_t* l = lam2 + scalar_limbs<F>() * (size_t)r0 * k;
            E* o = O + (size_t)r0 * ostride;
            if (!dispatch_int(IntRange<1, MAXK>(), k, [&](auto k_) { go_rec<decltype(k_)::value>(f, lc, rows, l, wc, o, ostride, n, st); }))
                return L_BAD_ARG;
        }
        return launched();
    }

    static LaunchStatus pow(const void* Fp, const LaunchCfg& lc, const void* a, const ExpArgs* ex, void* out, size_t n,
                   hipStream_t st) {
        const F& f = policy(Fp);
        const Plan p = plan(n, al(a) && al(out), lc);
        hipLaunchKernelGGL((k_pow<F, true>), dim3(p.grid), dim3(BLOCK), 0, st, f, (const E*)a, *ex, (E*)out, p.nvec, n);
        return launched();
    }
    static LaunchStatus inv(const void* Fp, const LaunchCfg& lc, const void* a, const ExpArgs* ex, void* out, size_t n, int* flag,
                   hipStream_t st) {
        const F& f = policy(Fp);
        const size_t nvec = plan(n, al(a) && al(out), lc).nvec;
        // packs per thread: ONE exponentiation (70 products for 2^61 - 1) is shared by G x CH packs, and the
        // G x CH x N prefix words stay in registers (two waves per SIMD at CH = 8..12 for one-word fields)
        if constexpr (F::EPW == 1 && sizeof(W) == 8) {
            // One exponentiation (70 products for 2^61 - 1) is shared by the CH x G packs of a thread: k_inv_fast (full batches
            // without predicates, second reads in a window, exponentiation without its window table when the exponent allows
            // it) at 8 x 2 packs = 32 elements per thread and three waves per SIMD for arrays of at least 32768 elements
            // (profiles/r04_alu.md: thirteen shapes measured; more packs per thread spill or fall to two waves, fewer pay more
            // exponentiations); k_inv_batch below that and for GF(2^n).
            // (prime fields only: the GF(2^n) product has run-time loops, its prefix array lives in scratch memory either way,
            // and the round-3 kernel needs less of it -- 272-336 B against 528-624 B per thread)
            if (!F::BINARY && nvec >= (size_t)BLOCK * 64) {
                if (pow_lean_ok(*ex)) return launch_inv_fast<8, 2, 6, 3, true>(f, a, ex, out, nvec, n, flag, st);
                return launch_inv_fast<8, 2, 3, 1, false>(f, a, ex, out, nvec, n, flag, st);
            }
            // All waves of the launch take the same time and two fit on a SIMD, so the launch runs in ROUNDS of
            // 2 x 4 x num_cu waves: 10^7 elements at CH = 8 are 4883 waves = 2.4 rounds -- three rounds of time for
            // 2.4 of work (measured: 56 us).  More packs per thread amortise the exponentiation better AND change the
            // number of rounds; pick the CH with the least rounds x (products per thread).
            const size_t slots = (size_t)lc.num_cu * 4 * 2;
            int best = 8;
            double best_cost = 0;
            for (int ch : {8, 10}) {                    // (CH = 12: 296 VGPRs, one wave per SIMD)
                const size_t waves = (nvec / (size_t)(ch * 2) + 63) / 64 + 1;
                const size_t rounds = (waves + slots - 1) / slots;
                const double cost = (double)rounds * (3.0 * ch * 2 * (double)EPV + 73.0);
                if (ch == 8 || cost < best_cost * 0.97) {
                    best = ch;
                    best_cost = ch == 8 ? cost : (cost < best_cost ? cost : best_cost);
                }
            }
            if (best == 10) return launch_inv<10, 2>(f, lc, a, ex, out, nvec, n, flag, st);
            return launch_inv<8, 2>(f, lc, a, ex, out, nvec, n, flag, st);
        } else {
            if constexpr (HasDigitChain<F>::value) {
                // multi-limb 2^k - c primes: the whole batch in digits (k_inv_digits), NL = ceil(k / 28) registers per value
                if (nvec >= 4096) {
                    const LaunchStatus rc = launch_inv_digits_from<F::CHAIN_MIN_NL>(f, lc, a, ex, out, nvec, n, flag, st);
                    if (rc.code != L_DECLINED) return rc;
                }
            }
            constexpr int CH = F::EPW > 1 ? 2 : 8;          // packed bytes: 8 words per batch (zero mask)
            return launch_inv<CH, 1>(f, lc, a, ex, out, nvec, n, flag, st);
        }
    }
    // L_DECLINED: the modulus has no digit form at this NL (DigitChain::setup: c too large) -> the word kernel
    template <int NL>
    static LaunchStatus launch_inv_digits_from(const F& f, const LaunchCfg& lc, const void* a, const ExpArgs* ex, void* out, size_t nvec,
                                      size_t n, int* flag, hipStream_t st) {
        if constexpr (!HasDigitChain<F>::value) {
            return L_DECLINED;
        } else if constexpr (NL > F::CHAIN_MAX_NL) {
            return L_DECLINED;
        } else {
            if (f.k > 28u * NL) return launch_inv_digits_from<NL + 1>(f, lc, a, ex, out, nvec, n, flag, st);
            DigitChain<NL> dc;
            if (!f.template chain_setup<NL>(dc)) return L_DECLINED;
            constexpr int CH = NL <= 3 ? 32 : NL == 4 ? 24 : NL <= 6 ? 16 : 12;      // ~96 registers of prefix products
            unsigned grid = grid_for((nvec + CH - 1) / CH, lc);
            hipLaunchKernelGGL((k_inv_digits<F, NL, CH, true>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, *ex, (E*)out, nvec, n,
                               flag);
            return launched();
        }
    }
    // square-and-multiply after the leading run costs popcount(tail) products, the window table 8 up front and one per
    // window: lean when the tail holds few set bits (q - 2 of every 2^k - c prime: a run of ones and a short tail)
    static bool pow_lean_ok(const ExpArgs& ex) {
        int i = ex.nbits - 1;
        auto bit = [&](int b) { return (int)((ex.e[b >> 6] >> (b & 63)) & 1u); };
        while (i >= 0 && bit(i)) --i;                 // the leading run
        if (ex.nbits - 1 - i < 12) i = ex.nbits - 2;  // (short runs are not raised by doubling: everything is tail)
        int ones = 0;
        for (int b = i; b >= 0; --b) ones += bit(b);
        return ones <= 6;
    }
    template <int CH, int G, int WIN, int WAVES, bool LEAN, int WIN1 = 0>
    static LaunchStatus launch_inv_fast(const F& f, const void* a, const ExpArgs* ex, void* out, size_t nvec, size_t n, int* flag,
                               hipStream_t st) {
        if constexpr (F::EPW == 1 && sizeof(W) == 8) {
            const size_t per_block = (size_t)BLOCK * CH * G;
            const size_t nfull = nvec / per_block;
            const size_t rest = nvec % per_block;
            const unsigned grid = (unsigned)nfull + (unsigned)((rest + BLOCK - 1) / BLOCK) + ((rest == 0 && n > nvec * EPV) ? 1u : 0u);
            hipLaunchKernelGGL((k_inv_fast<F, CH, G, WIN, WAVES, LEAN, WIN1>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, *ex, (E*)out,
                               nvec, n, (unsigned)nfull, flag);
        }
        return launched();
    }
    template <int CH, int G>
    static LaunchStatus launch_inv(const F& f, const LaunchCfg& lc, const void* a, const ExpArgs* ex, void* out, size_t nvec, size_t n,
                          int* flag, hipStream_t st) {
        size_t iters = nvec ? (nvec + CH * G - 1) / (CH * G) : n;
        unsigned grid = grid_for(iters, lc);
        hipLaunchKernelGGL((k_inv_batch<F, CH, G, true>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, *ex, (E*)out,
                           nvec, n, flag);
        return launched();
    }

    // skinny shapes (one output dimension <= 8): HBM-bound kernels that read the big operand once
    // (every choice from here to Launchers::matmul is restated in tests/matmul_contract.py, plan() -- move the two together)
    template <int NN>
    static void go_matvec(const F& f, const E* A, size_t lda, const E* B, size_t ldb, E* C, size_t ldc, int M, int K,
                          int N, hipStream_t st) {
        if (K <= 32 && M >= 1024) {               // short rows: one thread per row
            unsigned grid = (unsigned)(((size_t)M + BLOCK - 1) / BLOCK);
            hipLaunchKernelGGL((k_matvec_short_rows<F, NN>), dim3(grid), dim3(BLOCK), 0, st, f, A, lda, B, ldb, C, ldc, M, K, N);
            return;
        }
        const int vec = al(A) && stride_ok(lda);
        const int bvec = al(B) && stride_ok(ldb) && (N % (int)Pack<W>::N == 0) && sizeof(E) != 12;
        if constexpr (NN <= 2) {              // (12-byte elements too since round 6: one element per pack, dwordx3 accesses)
            // long rows, one or two columns: R = 2 rows per workgroup share every load of B (measured at 4096^2 / 8192^2:
            // R = 1 32.5 / 117 us, R = 2 27.4 / 85 us, R = 4 28.3 / 99 us, R = 8 35.8 / 112 us)
            constexpr int R = 2;
            if (vec && K >= 1024 && M >= 1024 * R) {
                const int bpack = (N == 1 && ldb == 1 && al(B)) ? 1 : 0;
                hipLaunchKernelGGL((k_matvec_rows_r<F, NN, R>), dim3((unsigned)((M + R - 1) / R)), dim3(BLOCK), 0, st, f, A, lda, B,
                                   ldb, C, ldc, M, K, N, vec, bpack);
                return;
            }
        }
        hipLaunchKernelGGL((k_matvec_rows<F, NN>), dim3((unsigned)M), dim3(BLOCK), 0, st, f, A, lda, B, ldb, C, ldc, K, N, vec,
                           bvec);
    }
    // one-word primes, 2..8 columns: column sums, one instantiation per N; two rows of A per workgroup up to 4 columns
    template <int NN>
    static void go_matvec_col(const F& f, const LaunchCfg& lc, const E* A, size_t lda, const E* B, size_t ldb, E* C, size_t ldc, int M,
                              int K, hipStream_t st) {
        if constexpr (col_mac_ok<F>::value) {
            constexpr int R = NN <= 4 ? 2 : 1;
            const int vec = al(A) && stride_ok(lda);
            const int bvec = al(B) && stride_ok(ldb) && (NN % (int)Pack<W>::N == 0);
            // B contiguous and 16-byte aligned, rows of A aligned: sixteen lanes per row (a wave per row when 16 rows per
            // workgroup would leave CUs without one), the rows of B through LDS
            if (vec && ldb == (size_t)NN && al(B) && K >= 64) {
                if ((M + 15) / 16 >= 2 * lc.num_cu)
                    hipLaunchKernelGGL((k_matvec_sub_col<F, NN, 16>), dim3((unsigned)((M + 15) / 16)), dim3(BLOCK), 0, st, f, A, lda, B, C, ldc, M, K);
                else
                    hipLaunchKernelGGL((k_matvec_sub_col<F, NN, 64>), dim3((unsigned)((M + 3) / 4)), dim3(BLOCK), 0, st, f, A, lda, B, C, ldc, M, K);
            } else {
                hipLaunchKernelGGL((k_matvec_rows_col<F, NN, R>), dim3((unsigned)((M + R - 1) / R)), dim3(BLOCK), 0, st, f, A, lda, B, ldb,
                                   C, ldc, M, K, vec, bvec);
            }
        }
    }
    template <int MM>
    static void go_vecmat(const F& f, const E* A, size_t lda, const E* B, size_t ldb, W* part, int M, int K, int N,
                          int ks, int kchunk, hipStream_t st) {
        constexpr int CW = Pack<W>::N;
        const bool vec = sizeof(E) != 12 && CW > 1 && al(B) && stride_ok(ldb) && N % CW == 0;
        if (vec) {
            dim3 grid((N / CW + BLOCK - 1) / BLOCK, ks);
            hipLaunchKernelGGL((k_vecmat_partial<F, MM, true, (MM > 1)>), grid, dim3(BLOCK), 0, st, f, A, lda, B, ldb, part, M, K, N, kchunk);
        } else {
            dim3 grid((N + BLOCK - 1) / BLOCK, ks);
            hipLaunchKernelGGL((k_vecmat_partial<F, MM, false, (MM > 1)>), grid, dim3(BLOCK), 0, st, f, A, lda, B, ldb, part, M, K, N, kchunk);
        }
    }
    // one-word prime fields: column accumulators, one instantiation per M, one column per thread.  Rows of B per group (two
    // groups in registers) and resident workgroups per CU follow the registers of the column sums, 12 per row of A (measured,
    // 4096 x 4096 over 2^61 - 1, profiles/HISTORY.md): up to 4 rows four workgroups and groups of 8; 5..7 rows three
    // workgroups and groups of 4; 8 rows two workgroups and groups of 16
    template <int MM>
    struct VecmatCol {
        static constexpr int UNR = MM <= 4 ? 8 : MM < 8 ? 4 : 16;
        static constexpr int MINB = MM <= 4 ? 4 : MM < 8 ? 3 : 2;
    };
    static int vecmat_col_per_cu(int M) { return M <= 4 ? 4 : M < 8 ? 3 : 2; }
    template <int MM>
    static void go_vecmat_col(const F& f, const E* A, size_t lda, const E* B, size_t ldb, W* part, int K, int N, int ks,
                              int kchunk, hipStream_t st) {
        if constexpr (col_mac_ok<F>::value) {
            typedef VecmatCol<MM> C;
            dim3 grid((N + BLOCK - 1) / BLOCK, ks);
            hipLaunchKernelGGL((k_vecmat_partial_col<F, MM, C::UNR, C::MINB>), grid, dim3(BLOCK), 0, st, f, A, lda, B, ldb, part, K, N, kchunk);
        }
    }
    // ---- dense products: five routes, tried in this order; each says whether it took the product -----------------
    struct Mat {
        const E* A; size_t lda;
        const E* B; size_t ldb;
        E* C; size_t ldc;
        int M, K, N;
        void* ws; size_t ws_bytes;      // scratch of the call (api.hip, ScratchSlots), may be absent
        hipStream_t st;
    };
    // at most 8 columns (4 for three-limb words: the eight-column kernel would spill, N in 5..8 takes the tiled product)
    static bool mm_skinny_n(const F& f, const LaunchCfg& lc, const Mat& m) {
        if constexpr (F::EPW == 1) {
            if (m.N > (sizeof(W) > 16 ? 4 : SKINNY_MAX) || m.M < 64 || m.K < 1) return false;
            if constexpr (col_mac_ok<F>::value) {
                if (m.N >= 2 && m.K > 32) {               // (short rows keep the one-thread-per-row kernel)
                    dispatch_int(IntRange<2, SKINNY_MAX>(), m.N, [&](auto n_) {
                        go_matvec_col<decltype(n_)::value>(f, lc, m.A, m.lda, m.B, m.ldb, m.C, m.ldc, m.M, m.K, m.st);
                    });
                    return true;
                }
            }
            if (m.N == 1) go_matvec<1>(f, m.A, m.lda, m.B, m.ldb, m.C, m.ldc, m.M, m.K, m.N, m.st);
            else if (m.N == 2) go_matvec<2>(f, m.A, m.lda, m.B, m.ldb, m.C, m.ldc, m.M, m.K, m.N, m.st);
            else if (m.N <= 4) go_matvec<4>(f, m.A, m.lda, m.B, m.ldb, m.C, m.ldc, m.M, m.K, m.N, m.st);
            else go_matvec<8>(f, m.A, m.lda, m.B, m.ldb, m.C, m.ldc, m.M, m.K, m.N, m.st);
            return true;
        }
        return false;
    }
    // at most 8 rows: partial sums over chunks of K in the scratch, then k_vecmat_final
    static bool mm_skinny_m(const F& f, const LaunchCfg& lc, const Mat& m) {
        if constexpr (F::EPW == 1) {
            const int M = m.M, K = m.K, N = m.N;
            if (M > SKINNY_MAX || N < 64 || K < 1 || !m.ws) return false;
            // split K so that one round of workgroups fills the chip; each chunk at least 8 rows.  One-word primes: one
            // column per thread, as many workgroups as are resident at once (registers of the column sums)
            int cpt = (int)Pack<W>::N, target = 1024;        // columns per thread, workgroups
            if constexpr (col_mac_ok<F>::value) {
                cpt = 1;
                target = lc.num_cu * vecmat_col_per_cu(M);
            }
            const int cols_blocks = (N / cpt + BLOCK - 1) / BLOCK;
            int ks = (target + cols_blocks - 1) / cols_blocks;
            if (ks > (K + 7) / 8) ks = (K + 7) / 8;
            if (ks < 1) ks = 1;
            while (ks > 1 && (size_t)ks * M * N * sizeof(W) > m.ws_bytes) ks /= 2;
            if ((size_t)ks * M * N * sizeof(W) > m.ws_bytes) return false;
            const int kchunk = (K + ks - 1) / ks;
            ks = (K + kchunk - 1) / kchunk;
            W* part = (W*)m.ws;
            if constexpr (col_mac_ok<F>::value) {
                dispatch_int(IntRange<1, SKINNY_MAX>(), M, [&](auto m_) {
                    go_vecmat_col<decltype(m_)::value>(f, m.A, m.lda, m.B, m.ldb, part, K, N, ks, kchunk, m.st);
                });
            } else if (M == 1) go_vecmat<1>(f, m.A, m.lda, m.B, m.ldb, part, M, K, N, ks, kchunk, m.st);
            else if (M == 2) go_vecmat<2>(f, m.A, m.lda, m.B, m.ldb, part, M, K, N, ks, kchunk, m.st);
            else if (M <= 4) go_vecmat<4>(f, m.A, m.lda, m.B, m.ldb, part, M, K, N, ks, kchunk, m.st);
            else go_vecmat<8>(f, m.A, m.lda, m.B, m.ldb, part, M, K, N, ks, kchunk, m.st);
            constexpr int CO = BLOCK / VECMAT_FINAL_G;
            hipLaunchKernelGGL((k_vecmat_final<F>), dim3((unsigned)(((size_t)M * N + CO - 1) / CO)), dim3(BLOCK), 0,
                               m.st, f, (const W*)part, ks, M, N, m.C, m.ldc);
            return true;
        }
        return false;
    }
    // large dense products over primes of up to 64 bits: int8 matrix cores, 8 signed base-256 digits per operand
    // (k_limb_gemm_glds), 4 for 32-bit storage (k_limb_gemm_l4)
    static bool mm_mfma(const F& f, const LaunchCfg& lc, const Mat& m) {
        if constexpr (F::EPW == 1 && !F::BINARY && sizeof(W) <= 8) {
            const int M = m.M, K = m.K, N = m.N;
            const int L = sizeof(W) == 4 ? 4 : 8;
            const uint64_t pmod = (uint64_t)f.p;
            const int Mp = (M + 63) / 64 * 64, Np = (N + 63) / 64 * 64, Kp = (K + 31) / 32 * 32;
            const size_t need = mfma_plane_bytes(lc, L, M, K, N);
            if (!need || !m.ws || need > m.ws_bytes) return false;
            int8_t* Ap = (int8_t*)m.ws;
            int8_t* Bp = Ap + (size_t)L * Mp * Kp;
            const unsigned ga = (unsigned)(((size_t)Mp * Kp + BLOCK - 1) / BLOCK);
            dim3 gb(Np / 32, Kp / 32), gg(Np / 64, Mp / 64);
            auto go = [&](auto lc_) {
                constexpr int LL = decltype(lc_)::value;
                hipLaunchKernelGGL((k_limb_split_a<F, LL>), dim3(ga), dim3(BLOCK), 0, m.st, m.A, m.lda, pmod, Ap, M, K, Mp, Kp);
                // up to 128 rows of 64-bit elements: the product kernel converts B itself (BRAW), no digit planes of B --
                // for whole tiles and 16-byte aligned rows of B; ragged shapes go through the planes
                constexpr bool CAN_RAW = LL == 8 && sizeof(E) == 8;
                const bool braw = CAN_RAW && gg.y <= 2 && K % 32 == 0 && N % 64 == 0 && m.ldb % 2 == 0 && (((uintptr_t)m.B) & 15) == 0;
                if (!braw)
                    hipLaunchKernelGGL((k_limb_split_bt<F, LL>), gb, dim3(BLOCK), 0, m.st, m.B, m.ldb, pmod, Bp, K, N, Np, Kp);
                auto product = [&](dim3 grid, E* out, size_t out_ld, int kb, int ke, int acc_, int kslice, size_t zs) {
                    if constexpr (CAN_RAW) {
                        if (braw) launch_glds<true>(f, grid, m.st, Ap, (const int8_t*)nullptr, out, out_ld, M, N, Kp, kb, ke, acc_, kslice, zs, m.B, m.ldb, pmod);
                        else launch_glds<false>(f, grid, m.st, Ap, Bp, out, out_ld, M, N, Kp, kb, ke, acc_, kslice, zs, (const E*)nullptr, (size_t)0, (uint64_t)0);
                    } else {
                        hipLaunchKernelGGL((k_limb_gemm_l4<F>), grid, dim3(BLOCK), 0, m.st, f, (const int8_t*)Ap, (const int8_t*)Bp, out,
                                           out_ld, M, N, Kp, kb, ke, acc_, kslice, zs);
                    }
                };
                // few output tiles (a batch of 64..256 rows against a big matrix): split K over blockIdx.z into
                // slabs behind the planes, summed by k_splitk_sum
                const size_t tiles = (size_t)gg.x * gg.y;
                int ks = 1;
                if (tiles <= 128 && Kp >= 512) {
                    // ONE round of workgroups (a workgroup holds a CU: 512 registers per lane): tiles x slabs ~ CUs.
                    // Measured (round 4, 64 x 4096 x 4096): 256 workgroups 94 us, 384: 127, 512: 107, 768: 117, 1536: 121
                    // -- every extra slab repeats the epilogue and the pipeline fill.
                    ks = (int)((lc.num_cu + tiles - 1) / tiles);
                    if (ks > Kp / 256) ks = Kp / 256;
                    while (ks > 1 && need + 256 + (size_t)ks * M * N * sizeof(E) > m.ws_bytes) --ks;
                }
                if (ks > 1 && Kp <= LIMB_KCHUNK) {
                    const int kslice = ((Kp + ks - 1) / ks + 31) / 32 * 32;
                    ks = (Kp + kslice - 1) / kslice;
                    E* slabs = (E*)((char*)m.ws + ((need + 255) / 256) * 256);
                    dim3 g3(gg.x, gg.y, ks);
                    product(g3, slabs, (size_t)N, 0, Kp, 0, kslice, (size_t)M * N);
                    hipLaunchKernelGGL((k_splitk_sum<F>), dim3((unsigned)(((size_t)M * N + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, m.st, f,
                                       (const E*)slabs, ks, M, N, m.C, m.ldc);
                    return;
                }
                for (int kb = 0; kb < Kp; kb += LIMB_KCHUNK) {
                    const int ke = kb + LIMB_KCHUNK < Kp ? kb + LIMB_KCHUNK : Kp;
                    product(gg, m.C, m.ldc, kb, ke, kb > 0 ? 1 : 0, 0, (size_t)0);
                }
            };
            if (L == 4) go(std::integral_constant<int, 4>());
            else go(std::integral_constant<int, 8>());
            return true;
        }
        return false;
    }
    // primes of 65..128 bits: the matrix-core product in passes over the diagonals (k_limb_gemm_wide)
    static bool mm_mfma_wide(const F& f, const LaunchCfg& lc, const Mat& m) {
        if constexpr (F::EPW == 1 && !F::BINARY && sizeof(W) == 16) {
            const int M = m.M, K = m.K, N = m.N;
            constexpr int LW = sizeof(E) == 12 ? 12 : 16;
            const int Mp = (M + 63) / 64 * 64, Np = (N + 63) / 64 * 64, Kp = (K + 31) / 32 * 32;
            const size_t need = mfma_plane_bytes(lc, LW, M, K, N);
            if (!need || !m.ws || need > m.ws_bytes) return false;
            int8_t* Ap = (int8_t*)m.ws;
            int8_t* Bp = Ap + (size_t)LW * Mp * Kp;
            const unsigned ga = (unsigned)(((size_t)Mp * Kp + BLOCK - 1) / BLOCK);
            dim3 gb(Np / 32, Kp / 32), gg(Np / 64, Mp / 64);
            hipLaunchKernelGGL((k_limb_split_a_wide<F, LW>), dim3(ga), dim3(BLOCK), 0, m.st, m.A, m.lda, f.p_lo, f.p_hi, Ap, M,
                               K, Mp, Kp);
            hipLaunchKernelGGL((k_limb_split_bt_wide<F, LW>), gb, dim3(BLOCK), 0, m.st, m.B, m.ldb, f.p_lo, f.p_hi, Bp, K, N,
                               Np, Kp);
            // 256^D0 mod p by repeated doubling of the canonical 1 (host, canonical arithmetic of the policy)
            auto pow256 = [&](int d0) {
                W v;
                v.lo = 1;
                v.hi = 0;
                for (int i = 0; i < 8 * d0; ++i) v = f.add(v, v);
                return v;
            };
            bool first = true;
            for (int kb = 0; kb < Kp; kb += LIMB_KCHUNK_WIDE) {
                const int ke = kb + LIMB_KCHUNK_WIDE < Kp ? kb + LIMB_KCHUNK_WIDE : Kp;
                auto pass = [&](auto d0_, auto ndp_) {
                    constexpr int D0 = decltype(d0_)::value, NDP = decltype(ndp_)::value;
                    hipLaunchKernelGGL((k_limb_gemm_wide<F, LW, D0, NDP>), gg, dim3(BLOCK), 0, m.st, f, (const int8_t*)Ap,
                                       (const int8_t*)Bp, m.C, m.ldc, M, N, Mp, Np, Kp, kb, ke, first ? 0 : 1, pow256(D0));
                    first = false;
                };
                if constexpr (LW == 12) {            // 23 diagonals: 12 + 11
                    pass(std::integral_constant<int, 0>(), std::integral_constant<int, 12>());
                    pass(std::integral_constant<int, 12>(), std::integral_constant<int, 11>());
                } else {                              // 31 diagonals: 11 + 10 + 10
                    pass(std::integral_constant<int, 0>(), std::integral_constant<int, 11>());
                    pass(std::integral_constant<int, 11>(), std::integral_constant<int, 10>());
                    pass(std::integral_constant<int, 21>(), std::integral_constant<int, 10>());
                }
            }
            return true;
        }
        return false;
    }
    // every other product: tiles on the vector ALUs
    static void mm_valu(const F& f, const Mat& m) {
        const int M = m.M, K = m.K, N = m.N;
        if constexpr (F::EPW > 1) {
            dim3 grid((N + 31) / 32, (M + 31) / 32);
            hipLaunchKernelGGL((k_matmul_bytes<F>), grid, dim3(BLOCK), 0, m.st, f, (const uint8_t*)m.A, m.lda,
                               (const uint8_t*)m.B, m.ldb, (uint8_t*)m.C, m.ldc, M, K, N);
        } else {
            // 4 x 2 outputs per thread: measured best (1.93 T MAC/s at 4096^3 over GF(2^61-1))
            // small outputs (a 64 x 64 product is two 64 x 32 tiles): 32 x 32 tiles give four times as many workgroups
            const bool small_out = ((M + 63) / 64) * ((N + 31) / 32) < 64;
            const bool t42 = !(sizeof(W) >= 16 || small_out);   // two- and three-limb words: 2x2 keeps two waves per SIMD
            const int bm = t42 ? 64 : 32;
            const int bn = 32;
            dim3 grid((N + bn - 1) / bn, (M + bm - 1) / bm);
            // too few output tiles to fill 256 CUs: split K over blockIdx.z into slabs of the workspace
            int ks = 1, kchunk = 0;
            const size_t tiles = (size_t)grid.x * grid.y;
            E* out = m.C;
            size_t out_ld = m.ldc, zstride = 0;
            if (tiles < 512 && K >= 64 && m.ws) {
                ks = (int)((1024 + tiles - 1) / tiles);
                if (ks > K / 32) ks = K / 32;
                while (ks > 1 && (size_t)ks * M * N * sizeof(E) > m.ws_bytes) ks /= 2;
                if (ks > 1) {
                    kchunk = ((K + ks - 1) / ks + 15) / 16 * 16;
                    ks = (K + kchunk - 1) / kchunk;
                    grid.z = ks;
                    out = (E*)m.ws;
                    out_ld = N;
                    zstride = (size_t)M * N;
                }
            }
            if (ks <= 1) kchunk = 0;
            if (t42)
                hipLaunchKernelGGL((k_matmul<F, 4, 2>), grid, dim3(BLOCK), 0, m.st, f, m.A, m.lda, m.B, m.ldb, out, out_ld, M, K, N, kchunk, zstride);
            else
                hipLaunchKernelGGL((k_matmul<F, 2, 2>), grid, dim3(BLOCK), 0, m.st, f, m.A, m.lda, m.B, m.ldb, out, out_ld, M, K, N, kchunk, zstride);
            if (ks > 1)
                hipLaunchKernelGGL((k_splitk_sum<F>), dim3((unsigned)(((size_t)M * N + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, m.st, f,
                                   (const E*)m.ws, ks, M, N, m.C, m.ldc);
        }
    }
    static LaunchStatus matmul(const void* Fp, const LaunchCfg& lc, const void* A, size_t lda, const void* B, size_t ldb, void* C,
                               size_t ldc, int M, int K, int N, void* workspace, size_t workspace_bytes, hipStream_t st) {
        const F& f = policy(Fp);
        const Mat m = {(const E*)A, lda, (const E*)B, ldb, (E*)C, ldc, M, K, N, workspace, workspace_bytes, st};
        if (!mm_skinny_n(f, lc, m) && !mm_skinny_m(f, lc, m) && !mm_mfma(f, lc, m) && !mm_mfma_wide(f, lc, m)) mm_valu(f, m);
        return launched();
    }
    // ---- stacks of products: one launch, the shape from stack_plan (matmul_stack_geom.hpp), no workspace -------------
    enum { STACK_SLOT = F::EPW > 1 ? 1 : (DotAcc<F>::lazy ? 4 * (int)DotAcc<F>::NL : (int)sizeof(W)) };
    // (named member functions launch the kernels, see the note at launch_glds)
    static void launch_stack_packed(const F& f, const StackPlan& p, const StackArgs& s, const E* A, const E* B, E* C, hipStream_t st) {
        hipLaunchKernelGGL((k_matmul_stack_packed<F>), dim3((unsigned)p.grid), dim3(BLOCK), p.lds_bytes, st, f, A, B, C, s);
    }
    static void launch_stack_tiled(const F& f, const StackPlan& p, const StackArgs& s, const E* A, const E* B, E* C, hipStream_t st) {
        if constexpr (F::EPW > 1) {
            hipLaunchKernelGGL((k_matmul_stack_tiled_bytes<F>), dim3((unsigned)p.grid), dim3(BLOCK), 0, st, f, (const uint8_t*)A,
                               (const uint8_t*)B, (uint8_t*)C, s);
        } else {
            if constexpr (sizeof(W) < 16) {             // (two- and three-limb words: the plan never asks for 64-row tiles)
                if (p.bm == 64) {
                    hipLaunchKernelGGL((k_matmul_stack_tiled<F, 4, 2>), dim3((unsigned)p.grid), dim3(BLOCK), 0, st, f, A, B, C, s);
                    return;
                }
            }
            hipLaunchKernelGGL((k_matmul_stack_tiled<F, 2, 2>), dim3((unsigned)p.grid), dim3(BLOCK), 0, st, f, A, B, C, s);
        }
    }
    static LaunchStatus matmul_stack(const void* Fp, const LaunchCfg& lc, const void* A, size_t lda, size_t sa, const void* B, size_t ldb,
                                     size_t sb, void* C, size_t ldc, size_t sc, int M, int K, int N, size_t batch, hipStream_t st) {
        const F& f = policy(Fp);
        const StackPlan p = stack_plan((size_t)M, (size_t)K, (size_t)N, batch, (int)sizeof(E), lc.num_cu, STACK_SLOT, sa == 0, sb == 0);
        if (!p.ok) return L_PLAN_REFUSED;
        StackArgs s = {};
        s.lda = lda; s.sa = sa; s.ldb = ldb; s.sb = sb; s.ldc = ldc; s.sc = sc; s.batch = batch;
        s.M = M; s.K = K; s.N = N;
        if (p.shape == STACK_PACKED) {
            s.P = p.P; s.KC = p.KC > 0 ? p.KC : 1; s.rows_a = p.rows_a; s.rows_b = p.rows_b;
            // 16-byte loads: the operand's matrices of every workgroup are one aligned run, staged whole (KC == K)
            const bool whole = K > 0 && p.KC == K && sizeof(E) <= 8;
            auto run_ok = [&](const void* X, size_t ld, size_t cols, size_t stride, size_t per) {
                return whole && aligned16(X) && ld == cols && (stride == 0 || (stride == per && ((size_t)p.P * per * sizeof(E)) % 16 == 0));
            };
            s.vec_a = run_ok(A, lda, (size_t)K, sa, (size_t)M * K) ? 1 : 0;
            s.vec_b = run_ok(B, ldb, (size_t)N, sb, (size_t)K * N) ? 1 : 0;
            launch_stack_packed(f, p, s, (const E*)A, (const E*)B, (E*)C, st);
        } else {
            s.bm = p.bm; s.bn = p.bn; s.tiles_m = p.tiles_m; s.tiles_n = p.tiles_n;
            launch_stack_tiled(f, p, s, (const E*)A, (const E*)B, (E*)C, st);
        }
        return launched();
    }
    // Shape by output count (convolve_geom.hpp): wide tiles once they give every compute unit lc.conv_wide_per_cu of them,
    // narrow ones below that, so that few outputs with many taps still fill the chip.  Neither needs scratch.
    template <class S>
    static LaunchStatus go_convolve(const F& f, const E* a, size_t na, const E* v, size_t nv, E* out, hipStream_t st) {
        const size_t tiles = conv_tiles(na + nv - 1, S::TO);
        if (tiles > 0x7fffffffu) return L_BAD_ARG;
        hipLaunchKernelGGL((k_convolve<F, S>), dim3((unsigned)tiles), dim3(BLOCK), 0, st, f, a, na, v, nv, out);
        return launched();
    }
    static LaunchStatus convolve(const void* Fp, const LaunchCfg& lc, const void* a, size_t na, const void* v, size_t nv, void* out,
                        hipStream_t st) {
        const F& f = policy(Fp);
        if (conv_use_wide(na + nv - 1, lc.num_cu, lc.conv_wide_per_cu))
            return go_convolve<ConvWide>(f, (const E*)a, na, (const E*)v, nv, (E*)out, st);
        return go_convolve<ConvNarrow>(f, (const E*)a, na, (const E*)v, nv, (E*)out, st);
    }
    // Scans and axis reductions (scan.hpp).  The column walk follows the streaming plan of the other launchers: one column
    // (pack) per thread up to the grid cap, packs only where every pointer allows them (al).  24-byte elements move per
    // lane (three dwordx2) in both geometries: consecutive j of a column are a whole row apart, so the wave-contiguous
    // ldgw / stgw contract would hold only for rows of whole waves, and the per-lane form serves every shape.
    template <bool MUL, bool RED, bool UNIT>
    static void go_scan_rows(const F& f, const ScanPlan& p, const E* a, E* out, size_t k, size_t inner, int wi, E* ws,
                             hipStream_t st, unsigned blocks, unsigned lines) {
        if constexpr (RED) {
            hipLaunchKernelGGL((k_scan_tile_reduce<F, MUL, UNIT>), dim3(blocks), dim3(BLOCK), 0, st, f, a, p.ntiles > 1 ? ws : out,
                               k, inner, p.ntiles, p.tt);
            if (p.ntiles > 1)
                hipLaunchKernelGGL((k_scan_tile_carry<F, MUL, true>), dim3(lines), dim3(BLOCK), 0, st, f, ws, out, p.ntiles);
        } else {
            if (p.ntiles > 1) {
                hipLaunchKernelGGL((k_scan_tile_reduce<F, MUL, UNIT>), dim3(blocks), dim3(BLOCK), 0, st, f, a, ws, k, inner,
                                   p.ntiles, p.tt);
                hipLaunchKernelGGL((k_scan_tile_carry<F, MUL, false>), dim3(lines), dim3(BLOCK), 0, st, f, ws, (E*)nullptr,
                                   p.ntiles);
            }
            hipLaunchKernelGGL((k_scan_tile<F, MUL, UNIT>), dim3(blocks), dim3(BLOCK), 0, st, f, a, out,
                               p.ntiles > 1 ? (const E*)ws : (const E*)nullptr, k, inner, p.ntiles, p.tt, wi);
        }
    }
    template <bool MUL, bool RED>
    static LaunchStatus go_scan(const F& f, const LaunchCfg& lc, const E* a, E* out, size_t outer, size_t k, size_t inner, int wi,
                       E* ws, size_t ws_bytes, hipStream_t st) {
        static_assert((int)EPV == (int)(sizeof(E) <= 8 ? 16 / sizeof(E) : 1), "scan_epv mirrors the pack size");
        const ScanPlan p = scan_plan(outer, k, inner, sizeof(E), al(a) && al(out), lc.num_cu, lc.scan_geom,
                                     lc.scan_tile_threads, wi);
        if (!p.ok) return L_PLAN_REFUSED;
        if (p.geom == SCAN_COLS) {
            hipLaunchKernelGGL((k_scan_cols<F, MUL, RED>), dim3(grid_for(p.units, lc)), dim3(BLOCK), 0, st, f, a, out, k, inner,
                               p.per, p.units, p.vec, wi);
            return launched();
        }
        const unsigned blocks = (unsigned)(p.lines * p.ntiles), lines = (unsigned)p.lines;
        if (p.ntiles > 1 && (!ws || ws_bytes / sizeof(E) < p.ws_elems)) return L_WS_TOO_SMALL;
        if (inner == 1) go_scan_rows<MUL, RED, true>(f, p, a, out, k, inner, wi, ws, st, blocks, lines);
        else go_scan_rows<MUL, RED, false>(f, p, a, out, k, inner, wi, ws, st, blocks, lines);
        return launched();
    }
    static LaunchStatus scan(const void* Fp, const LaunchCfg& lc, int mul, const void* a, void* out, size_t outer, size_t k, size_t inner,
                    int with_initial, void* workspace, size_t workspace_bytes, hipStream_t st) {
        const F& f = policy(Fp);
        const int wi = with_initial ? 1 : 0;
        if (mul) return go_scan<true, false>(f, lc, (const E*)a, (E*)out, outer, k, inner, wi, (E*)workspace, workspace_bytes, st);
        return go_scan<false, false>(f, lc, (const E*)a, (E*)out, outer, k, inner, wi, (E*)workspace, workspace_bytes, st);
    }
    static LaunchStatus axis_reduce(const void* Fp, const LaunchCfg& lc, int mul, const void* a, void* out, size_t outer, size_t k,
                           size_t inner, void* workspace, size_t workspace_bytes, hipStream_t st) {
        const F& f = policy(Fp);
        if (mul) return go_scan<true, true>(f, lc, (const E*)a, (E*)out, outer, k, inner, 0, (E*)workspace, workspace_bytes, st);
        return go_scan<false, true>(f, lc, (const E*)a, (E*)out, outer, k, inner, 0, (E*)workspace, workspace_bytes, st);
    }
    static LaunchStatus dot(const void* Fp, const LaunchCfg& lc, const void* a, const void* b, void* out, void* workspace, size_t n,
                   hipStream_t st) {
        const F& f = policy(Fp);
        const size_t nvec = plan(n, al(a) && (!b || al(b)), lc).nvec;
        size_t iters = nvec ? nvec : n;
        size_t want = (iters + (size_t)BLOCK * 8 - 1) / ((size_t)BLOCK * 8);     // >= 8 packs per thread
        // the grid is bounded by what the workspace holds: 1024 workgroups of words up to 16 bytes, 682 of the 24-byte words
        constexpr size_t max_blocks = dot_max_blocks<W>();
        static_assert(max_blocks >= 1 && max_blocks <= DOT_MAX_BLOCKS && max_blocks * sizeof(W) <= DOT_WORKSPACE_BYTES,
                      "the partial sums of dot / sum must fit the workspace that include/ffgpu.h promises");
        unsigned grid = (unsigned)(want < 1 ? 1 : want > max_blocks ? max_blocks : want);
        W* part = (W*)workspace;
        if (b)
            hipLaunchKernelGGL((k_dot_partial<F, true>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, (const E*)b,
                               part, nvec, n);
        else
            hipLaunchKernelGGL((k_dot_partial<F, false>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, (const E*)a,
                               part, nvec, n);
        hipLaunchKernelGGL((k_dot_final<F>), dim3(1), dim3(BLOCK), 0, st, f, (const W*)part, (int)grid, (E*)out);
        return launched();
    }
    static LaunchStatus sqrt_cl(const void* Fp, const LaunchCfg& lc, const void* a, const ExpArgs* eleg, const ExpArgs* elad, void* out,
                       size_t n, hipStream_t st) {
        if constexpr (F::BINARY) {
            return L_NOT_SUPPORTED;
        } else {
            const F& f = policy(Fp);
                unsigned grid = grid_for(n, lc);
            hipLaunchKernelGGL((k_sqrt_cl<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, *eleg, *elad, (E*)out, n);
            return launched();
        }
    }
    static LaunchStatus gauss(const void* Fp, const LaunchCfg& lc, void* A, int n, int ncols, size_t batch, int det_mode,
                     const ExpArgs* ex, void* det, int* sing, hipStream_t st) {
        const F& f = policy(Fp);
        constexpr int TI = 4;
        constexpr size_t ZMAX = 32768;                    // grid.z limit: larger batches go in chunks
        for (size_t b0 = 0; b0 < batch; b0 += ZMAX) {
            unsigned nb = (unsigned)(batch - b0 < ZMAX ? batch - b0 : ZMAX);
            E* Ab = (E*)A + b0 * (size_t)n * ncols;
            E* db = det ? (E*)det + b0 : nullptr;
            for (int k = 0; k < n; ++k) {
                hipLaunchKernelGGL((k_gauss_pivot<F>), dim3(nb), dim3(BLOCK), 0, st, f, Ab, n, ncols, k, *ex, db,
                                   sing + b0);
                int cols = ncols - k - 1;
                int rows = det_mode ? n - k - 1 : n;
                if (cols > 0 && rows > 0) {
                    dim3 grid((cols + BLOCK - 1) / BLOCK, (rows + TI - 1) / TI, nb);
                    hipLaunchKernelGGL((k_gauss_elim<F, TI>), grid, dim3(BLOCK), 0, st, f, Ab, n, ncols, k, det_mode,
                                       sing + b0);
                }
            }
        }
        return launched();
    }
    static LaunchStatus group_matvec(const void* Fp, const LaunchCfg& lc, const uint64_t* m2, const uint64_t* bias2, int r, int g,
                            const void* in, void* out, size_t ngroups, hipStream_t st) {
        const F& f = policy(Fp);
        if (r < 1 || g < 1 || r > GM_MAX || g > GM_MAX) return L_NOT_SUPPORTED;
        GroupMatArgs<F> ga;
        memset(&ga, 0, sizeof(ga));
        for (int i = 0; i < r * g; ++i) ga.m[i] = f.prep(word_at<F>(f, m2, i));
        for (int a = 0; a < r; ++a) {
            W b = bias2 ? word_at<F>(f, bias2, a) : word_from_limbs<F>(f, 0, 0);
            if constexpr (F::EPW > 1) b &= 0xffu;     // one element per word on this (element-wise) path
            ga.bias[a] = b;
        }
        ga.r = r;
        ga.g = g;
        unsigned grid = grid_for(ngroups, lc);
        if constexpr (F::EPW == 4) {
            const bool al8 = (((uintptr_t)in) & 7u) == 0;
            if (g == 8 && r == 8 && al8 && (((uintptr_t)out) & 7u) == 0) {
                hipLaunchKernelGGL((k_group8_bytes<F, 8>), dim3(grid), dim3(BLOCK), 0, st, f, ga, (const uint8_t*)in,
                                   (uint8_t*)out, ngroups);
                return launched();
            }
            if (g == 8 && r == 1 && al8) {
                hipLaunchKernelGGL((k_group8_bytes<F, 1>), dim3(grid), dim3(BLOCK), 0, st, f, ga, (const uint8_t*)in,
                                   (uint8_t*)out, ngroups);
                return launched();
            }
        }
        hipLaunchKernelGGL((k_group_matvec<F>), dim3(grid), dim3(BLOCK), 0, st, f, ga, (const E*)in, (E*)out, ngroups);
        return launched();
    }
    static LaunchStatus beaver(const void* Fp, const LaunchCfg& lc, const void* z, const void* x, const void* y, const void* d,
                      const void* e, void* out, int add_de, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const Plan p = plan(n, al(z) && al(x) && al(y) && al(d) && al(e) && al(out), lc);
        hipLaunchKernelGGL((k_beaver<F, true>), dim3(p.grid), dim3(BLOCK), 0, st, f, (const E*)z, (const E*)x, (const E*)y,
                           (const E*)d, (const E*)e, (E*)out, add_de, p.nvec, n);
        return launched();
    }
    static LaunchStatus prss(const void* Fp, const LaunchCfg& lc, const void* const* streams, int ks, int d, int l, int mask_bits,
                    const uint64_t* weights2, const uint64_t* r2, int accumulate, void* out, size_t n,
                    hipStream_t st) {
        const F& f = policy(Fp);
        if (ks < 1 || d < 1 || l < 1 || ks > PRSS_MAXS || ks * d > PRSS_MAXW) return L_NOT_SUPPORTED;
        PrssArgs<F> pa;
        memset(&pa, 0, sizeof(pa));
        for (int s = 0; s < ks; ++s) pa.streams[s] = (const uint8_t*)streams[s];
        for (int i = 0; i < ks * d; ++i)
            pa.w[i] = f.prep(word_at<F>(f, weights2, i));
        pa.r0 = r2[0];
        pa.r1 = r2[1];
        pa.ks = ks; pa.d = d; pa.l = l; pa.mask_bits = mask_bits; pa.accumulate = accumulate;
        unsigned grid = grid_for(n, lc);
        hipLaunchKernelGGL((k_prss<F>), dim3(grid), dim3(BLOCK), 0, st, f, pa, (E*)out, n);
        return launched();
    }

    static LaunchStatus prss_chacha(const void* Fp, const LaunchCfg& lc, const uint8_t* keys40, int ks, int d, int l, int mask_bits, int rounds,
                           const uint64_t* weights2, const uint64_t* r2, int accumulate, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        if (ks < 1 || d < 1 || l < 1 || l > 64 || ks > PRSS_CC_MAXS || ks * d > PRSS_CC_MAXW) return L_NOT_SUPPORTED;
        PrssCcArgs<F> pa;
        memset(&pa, 0, sizeof(pa));
        for (int s = 0; s < ks; ++s) {
            memcpy(pa.key[s], keys40 + 40 * s, 32);
            memcpy(pa.nonce[s], keys40 + 40 * s + 32, 8);
        }
        for (int i = 0; i < ks * d; ++i) pa.w[i] = f.prep(word_at<F>(f, weights2, i));
        pa.r0 = r2[0];
        pa.r1 = r2[1];
        pa.ks = ks; pa.d = d; pa.l = l; pa.mask_bits = mask_bits; pa.accumulate = accumulate; pa.rounds = rounds;
        prss_cc_layout(l, &pa.tb, &pa.dpt);
        const size_t tiles = (n + (size_t)pa.dpt - 1) / (size_t)pa.dpt;
        const unsigned grid = (unsigned)((tiles + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL((k_prss_chacha<F>), dim3(grid), dim3(BLOCK), 0, st, f, pa, (E*)out, n);
        return launched();
    }

    static const FieldOps* table() {
        static const FieldOps ops = {
            .ew2 = &ew2, .ew1 = &ew1, .muladd = &muladd, .split = &split, .rng_coeffs = &rng_coeffs,
            .recombine = &recombine, .pow = &pow, .inv = &inv, .matmul = &matmul, .dot = &dot,
            .gate = &gate, .sqrt_cl = &sqrt_cl, .gauss = &gauss, .group_matvec = &group_matvec, .beaver = &beaver,
            .prss = &prss, .prss_chacha = &prss_chacha, .matmul_stack = &matmul_stack, .stack_slot = STACK_SLOT, .convolve = &convolve, .scan = &scan, .axis_reduce = &axis_reduce,
            .secure = secure_ops<F>()};
        return &ops;
    }
};

}  // namespace ffgpu

#include "launch_secure.hpp"   // SecureOps + the launchers of the secure protocols' local steps

// ---- misc.hip: kernels outside the per-policy tables (GF(2^8) S-box steps, GF(2^n) table products, copy, probes) ----
// Declared here, once, for misc.hip and api.hip.
int ffgpu_sbox_build_lut(const void* gf2p8_policy, const uint8_t* rows8, uint8_t b, uint8_t* lut256);
bool ffgpu_gf8_build_tables(const void* policy, void* tables_out);     // false: no generator found, no tables
int ffgpu_gf2w_build_rtable(const void* policy, int limbs, void* rtable_out);
void ffgpu_gf8_sbox_layer_tables(const void* policy, const void* mul_tables, const uint64_t* m2, const uint64_t* bias2,
                                 unsigned char* out);
ffgpu::LaunchStatus ffgpu_launch_sbox(const uint8_t* lut256, const ffgpu::LaunchCfg& lc, const void* in, void* out, size_t n, hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_gf8_to_bits(const ffgpu::LaunchCfg& lc, const void* in, const void* addend, void* out, size_t n, hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_gf8_mask_open(const void* policy, const ffgpu::LaunchCfg& lc, const void* const* rows, const uint64_t* coef2,
                                               int nrows, const void* const* rbits, const uint64_t* mu2, int np, void* out, size_t n,
                                               hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_gf8_bits_affine_fold(const void* policy, const ffgpu::LaunchCfg& lc, const uint64_t* m2, const uint64_t* bias2,
                                                      const void* c, const void* rbits, size_t ybr, void* out, size_t ybo, size_t n,
                                                      int nbatch, hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_gf8_group8(const void* policy, const ffgpu::LaunchCfg& lc, const uint64_t* m2, const uint64_t* bias2, int fold,
                                            const void* in, void* out, size_t ngroups, hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_gf8_sbox_layer(const void* policy, const ffgpu::LaunchCfg& lc, const void* x, size_t xs, const void* r, size_t rs,
                                                void* out, size_t os, const void* tables_dev, const uint64_t* lam2, const uint64_t* mu2,
                                                int t, int m, size_t n, hipStream_t st, const ffgpu::RngArgs* rng);
ffgpu::LaunchStatus ffgpu_launch_keccak_local(const void* policy, const void* const* rows, const uint64_t* lam2, int k, size_t in_batch,
                                              int nbatch, int iota_round, int apply_round, void* out, size_t out_batch, size_t nstates,
                                              hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_keccak_round(const void* policy, const void* const* rows, const uint64_t* lam2, int k, size_t in_batch,
                                              int iota_round, int t, int m, void* shares, size_t share_stride, size_t out_batch,
                                              size_t nstates, hipStream_t st, const ffgpu::RngArgs* rng);
ffgpu::LaunchStatus ffgpu_launch_gf8_mul_tab(const void* tables, const ffgpu::LaunchCfg& lc, const void* a, const void* b, void* out, size_t n,
                                             hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_gf2w_mul_win(const void* policy, int limbs, const void* rtable, const ffgpu::LaunchCfg& lc, const void* a,
                                              const void* b, void* out, size_t n, hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_gf2w64_mul_bitsliced(const void* policy, const ffgpu::LaunchCfg& lc, const void* a, const void* b, void* out,
                                                      size_t n, hipStream_t st, size_t* done);
ffgpu::LaunchStatus ffgpu_launch_gf2w_recombine(const void* policy, int limbs, const ffgpu::LaunchCfg& lc, const void* const* rows,
                                                const uint64_t* lam2, int k, void* out, size_t n, hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_copy(const ffgpu::LaunchCfg& lc, const void* src, void* dst, size_t bytes, hipStream_t st);
ffgpu::LaunchStatus ffgpu_launch_valu_probe(const ffgpu::LaunchCfg& lc, int op, int iters, int waves_per_simd, void* scratch32, double* out,
                                            hipStream_t st);
