// launch_secure.hpp -- host side of the secure protocols' local steps: their launcher table (SecureOps) and one short launcher
// per kernel.  Included by launch.hpp, after Launchers<F>.
//
// Prime fields only: the entries of api.hip that end here begin with PRIME_CTX, and a GF(2^n) policy has no such table
// (secure_ops).  A new family adds its kernels' launchers below and their lines in SecureOps and table().
#pragma once

namespace ffgpu {

struct SecureOps {
    // local steps of the secure comparison (sgn.hpp); consts: the host scalars 2^l, 2^(l-1), 2^-l
    // (L_PLAN_REFUSED: sgn_plan() refuses the sizes)
    LaunchStatus (*sgn_mask)(const void* F, const LaunchCfg& lc, const void* a, const void* rbits, const void* rdivl, int l,
                    const uint64_t* consts, void* out, size_t n, hipStream_t st);
    LaunchStatus (*sgn_expand)(const void* F, const LaunchCfg& lc, const void* c, const void* a, const void* rbits, const void* sbit,
                      int l, const uint64_t* consts, void* e, void* nx, void* z, size_t n, hipStream_t st);
    LaunchStatus (*sgn_finish)(const void* F, const LaunchCfg& lc, const void* w, const void* sbit, const void* z, int l,
                      const uint64_t* consts, void* out, size_t n, hipStream_t st);
    // the two ends of a compare-exchange stage of the sorting network (sort.hpp) (L_PLAN_REFUSED: cx_plan() refuses the
    // stage or the sizes; L_NOT_SUPPORTED: more than MAXK rows)
    LaunchStatus (*cx_diff)(const void* F, const LaunchCfg& lc, const void* a, void* out, size_t outer, size_t k, size_t inner,
                   size_t p, size_t d, size_t r, hipStream_t st);
    LaunchStatus (*cx_apply)(const void* F, const LaunchCfg& lc, void* a, const void* const* rows, const uint64_t* lam2, int nrows,
                    size_t outer, size_t k, size_t inner, size_t p, size_t d, size_t r, hipStream_t st);
    // local steps of bit decomposition (bits.hpp); consts: the host scalars 2^l and offset; lv: the round's table
    // (bits_level) (L_PLAN_REFUSED: sgn_plan() / bits_plan() refuses the sizes; L_NOT_SUPPORTED: more than MAXK rows)
    LaunchStatus (*bits_mask)(const void* F, const LaunchCfg& lc, const void* a, const void* rbits, const void* rdivl, int l,
                     const uint64_t* consts, void* out, size_t n, hipStream_t st);
    LaunchStatus (*bits_expand)(const void* F, const LaunchCfg& lc, const void* c, const void* rbits, int l, void* g, void* p, size_t n,
                       hipStream_t st);
    LaunchStatus (*carry_prod)(const void* F, const LaunchCfg& lc, const void* g, const void* p, int l, const BitsLevel& lv, void* out,
                      size_t n, hipStream_t st);
    LaunchStatus (*carry_apply)(const void* F, const LaunchCfg& lc, void* g, void* p, const void* const* rows, const uint64_t* lam2,
                       int nrows, int l, const BitsLevel& lv, size_t n, hipStream_t st);
    LaunchStatus (*bits_finish)(const void* F, const LaunchCfg& lc, const void* c, const void* rbits, const void* g, int l, void* out,
                       size_t n, hipStream_t st);
    // the ends of a tournament round (tour.hpp) (L_PLAN_REFUSED: tour_plan() refuses the round or the sizes;
    // L_NOT_SUPPORTED: more than MAXK rows)
    LaunchStatus (*tour_diff)(const void* F, const LaunchCfg& lc, const void* a, void* out, size_t outer, size_t k, size_t inner, int mode,
                     int neg, hipStream_t st);
    LaunchStatus (*tour_select)(const void* F, const LaunchCfg& lc, const void* a, const void* const* rows, const uint64_t* lam2,
                       int nrows, void* out, size_t outer, size_t k, size_t inner, int mode, int neg, hipStream_t st);
    LaunchStatus (*tour_unit_prod)(const void* F, const LaunchCfg& lc, const void* u, const void* c, void* out, size_t outer, size_t k,
                          size_t inner, hipStream_t st);
    LaunchStatus (*tour_unit_expand)(const void* F, const LaunchCfg& lc, const void* u, const void* const* rows, const uint64_t* lam2,
                            int nrows, void* out, size_t outer, size_t k, size_t inner, hipStream_t st);
    // the ends of a round of the first-occurrence search (find.hpp) (L_PLAN_REFUSED: find_plan() / find_leaf_plan() refuses
    // the round or the sizes; L_NOT_SUPPORTED: fewer than one or more than MAXK rows)
    LaunchStatus (*find_leaf_prod)(const void* F, const LaunchCfg& lc, const void* bits, const void* tab, void* out, size_t outer,
                          size_t k, size_t inner, int ncomp, int flip, int virt, hipStream_t st);
    LaunchStatus (*find_leaf_apply)(const void* F, const LaunchCfg& lc, const void* bits, const void* tab, const void* const* rows,
                           const uint64_t* lam2, int nrows, void* out, size_t outer, size_t k, size_t inner, int ncomp, int flip,
                           int virt, hipStream_t st);
    LaunchStatus (*find_prod)(const void* F, const LaunchCfg& lc, const void* level, void* out, size_t outer, size_t k, size_t inner,
                     int ncomp, hipStream_t st);
    // local steps of fixed-point truncation and normalisation (fxp.hpp); consts of trunc_mask: the host scalars 2^f and
    // offset, of trunc_finish: 2^-f (L_PLAN_REFUSED: sgn_plan() / flat_plan() / fxp_norm_plan() refuses the sizes;
    // L_NOT_SUPPORTED: fewer than one or more than MAXK rows)
    LaunchStatus (*trunc_mask)(const void* F, const LaunchCfg& lc, const void* a, const void* rbits, const void* rdivf, int f,
                      const uint64_t* consts, void* ar, void* masked, size_t n, hipStream_t st);
    LaunchStatus (*trunc_finish)(const void* F, const LaunchCfg& lc, const void* const* rows, const uint64_t* lam2, int nrows,
                        const void* ar, int f, const uint64_t* consts, void* out, size_t n, hipStream_t st);
    LaunchStatus (*norm_prod)(const void* F, const LaunchCfg& lc, const void* bits, int l, void* out, void* sign_out, size_t n,
                     hipStream_t st);
    LaunchStatus (*norm_apply)(const void* F, const LaunchCfg& lc, const void* bits, const void* const* rows, const uint64_t* lam2,
                      int nrows, int l, void* out, size_t n, hipStream_t st);
    // local steps under the secure logarithm and exponential (explog.hpp); c0 of poly_dot: one host scalar; pbits of
    // pow_base: the bit length of the modulus (L_PLAN_REFUSED: rows_plan() / pow_base_plan() / explog_rev_plan()
    // refuses the sizes or the counts)
    LaunchStatus (*powers_prod)(const void* F, const LaunchCfg& lc, const void* P, size_t stride, int h, int w, void* out, size_t n,
                       hipStream_t st);
    LaunchStatus (*poly_dot)(const void* F, const LaunchCfg& lc, const void* P, size_t stride, int theta, const void* tab,
                    const uint64_t* c0, void* out, size_t n, hipStream_t st);
    LaunchStatus (*pow_base)(const void* F, const LaunchCfg& lc, const void* x, int shift, int ebits, int pbits, const void* tab, void* out,
                    size_t n, hipStream_t st);
    LaunchStatus (*bits_reverse)(const void* F, const LaunchCfg& lc, const void* bits, int l, void* out, size_t n, hipStream_t st);
    // local steps of the Legendre zero test (iszero.hpp); the (k, n) arrays are row-major; ex of legendre_code: the exponent
    // (p - 1) / 2 as ffgpu_pow hands it to pow (L_PLAN_REFUSED: iszero_mask_plan() / stream_plan() / flat_plan()
    // refuses the sizes or the count)
    LaunchStatus (*iszero_mask)(const void* F, const LaunchCfg& lc, const void* a, const void* r, const void* z, const void* u2, int k,
                       void* out, size_t n, hipStream_t st);
    LaunchStatus (*legendre_code)(const void* F, const LaunchCfg& lc, const void* c, const ExpArgs* ex, uint8_t* code, size_t count,
                         hipStream_t st);
    LaunchStatus (*iszero_finish)(const void* F, const LaunchCfg& lc, const uint8_t* code, const void* z, void* out, size_t count,
                         hipStream_t st);
    // local steps of secure random bits (rbits.hpp); rows of n entries, one pointer each; lam2, A2, B2: host scalars; ex of
    // rbits_finish: the exponent (3p - 5) / 4 as ffgpu_pow hands it to pow (L_PLAN_REFUSED: rbits_open_plan() /
    // rbits_finish_plan() refuses the row count or the sizes)
    LaunchStatus (*rbits_open)(const void* F, const LaunchCfg& lc, const void* const* r, const void* const* z, const uint64_t* lam2, int k,
                      void* out, int* zeros, size_t n, hipStream_t st);
    LaunchStatus (*rbits_finish)(const void* F, const LaunchCfg& lc, const void* c, const ExpArgs* ex, const void* const* r, void* const* b,
                        int m, const uint64_t* A2, const uint64_t* B2, size_t n, hipStream_t st);
    // local steps of the secure binary sign by Legendre symbols (bsgn.hpp); the (w, n) arrays are row-major; alpha2, beta2:
    // one and w host scalars; ex of bsgn_finish: the exponent (p - 1) / 2 as ffgpu_pow hands it to pow; s, out: m rows of
    // shares and outputs, an output of n entries when sum (L_PLAN_REFUSED: bsgn_rows_plan() / bsgn_flat_plan() refuses the
    // counts or the sizes)
    LaunchStatus (*bsgn_mask)(const void* F, const LaunchCfg& lc, const void* a, const void* z, const uint64_t* alpha2,
                     const uint64_t* beta2, int w, void* out, size_t n, hipStream_t st);
    LaunchStatus (*bsgn_finish)(const void* F, const LaunchCfg& lc, const void* c, const ExpArgs* ex, const void* const* s, void* const* out,
                       int m, int w, int sum, size_t n, hipStream_t st);
    // local steps under secure unit vectors and table lookup (unitvec.hpp); the arrays are position-major (rows, n); c of
    // unit_dot may be null: no rotation (L_PLAN_REFUSED: unit_rows_plan() / unit_dot_plan() refuses the counts or the sizes;
    // L_NOT_SUPPORTED: the table of unit_dot does not fit LDS)
    LaunchStatus (*unit_prod)(const void* F, const LaunchCfg& lc, const void* x, size_t xstride, const void* U, size_t h, void* out,
                     size_t n, hipStream_t st);
    LaunchStatus (*unit_roll)(const void* F, const LaunchCfg& lc, const void* U, const void* c, int kbits, size_t K, void* out, size_t n,
                     hipStream_t st);
    LaunchStatus (*unit_dot)(const void* F, const LaunchCfg& lc, const void* U, size_t rows, const void* c, int kbits, const void* tab,
                    size_t tlen, void* out, size_t n, hipStream_t st);
    // the 2-D correlation of a secure convolution layer (conv2d.hpp): x, w, b (null: no bias; else nsend entries, all set)
    // and out are HOST arrays of nsend device pointers, one launch for all senders.  conv2d_plan is host-only: the plan
    // this policy's launcher takes for the sizes (conv2d_geom.hpp) (L_PLAN_REFUSED: conv2d_plan() refuses the sizes;
    // L_NOT_SUPPORTED: more than CONV2D_MAX_SENDERS senders, or a grid beyond HIP's limits)
    LaunchStatus (*conv2d)(const void* F, const LaunchCfg& lc, const void* const* x, const void* const* w, const void* const* b,
                  void* const* out, int nsend, size_t k, size_t r, size_t m, size_t n, size_t v, int s, hipStream_t st);
    Conv2dPlan (*conv2d_plan)(const LaunchCfg& lc, size_t k, size_t r, size_t m, size_t n, size_t v, int s, int nsend);
};

template <class F>
struct SecureLaunchers : Launchers<F> {
    static_assert(!F::BINARY, "the secure steps are built for prime fields only (secure_ops)");
    typedef Launchers<F> Base;
    using typename Base::E;
    using typename Base::Plan;
    using Base::al;
    using Base::EPV;
    using Base::PACK_ALIGN;
    using Base::plan;
    using Base::policy;

    // ---- the three frames.  Each takes the plan's answer and a callable that launches; the callables are plain (non-generic)
    // lambdas or, for the kernels with the row count as a template parameter, call a named go_*<K> (the note at launch_glds).
    // flat: one streaming loop over `units` (a pack where the plan admits packs, else an element) per thread up to the grid
    // cap.  In this order: refused, nothing to do, go(grid).
    template <class Go>
    static LaunchStatus flat(bool plan_ok, size_t units, const LaunchCfg& lc, Go&& go) {
        if (!plan_ok) return L_PLAN_REFUSED;
        if (units == 0) return L_OK;
        go(grid_for(units, lc));
        return launched();
    }
    // tiled: a workgroup per tile of SGN_TILE elements, go(p) launches on p.tiles of them.  sgn_plan, refused, nothing to do, go.
    template <class Go>
    static LaunchStatus tiled(size_t n, int l, Go&& go) {
        const SgnPlan p = sgn_plan(n, l, sizeof(E));
        if (!p.ok) return L_PLAN_REFUSED;
        if (n == 0) return L_OK;
        go(p);
        return launched();
    }
    // The launchers that take the sub-share rows of a round (share_rows.hpp) share the staging of the rows and their frame.
    // stage_rows: the rows and the prepared Lagrange vector as a kernel argument; *vec stays true only if every row is aligned
    // for packs.  The go_*<K> below are: stage, plan with vec, launch.
    template <int K>
    static ShareRows<F, K> stage_rows(const F& f, const void* const* rows, const uint64_t* lam2, bool* vec) {
        ShareRows<F, K> ra;
        for (int j = 0; j < K; ++j) {
            ra.rows[j] = (const E*)rows[j];
            ra.lam[j] = f.prep(word_at<F>(f, lam2, (size_t)j));
            *vec = *vec && al(rows[j]);
        }
        return ra;
    }
    // launch_rows: more than MAXK rows are L_NOT_SUPPORTED; then the plan's answer (refused, nothing to do); then go(k_) with
    // nrows as an integral_constant.  Fewer than one row matches no K: L_BAD_ARG (the entry point should have refused it),
    // unless the launcher documents L_NOT_SUPPORTED for it (SecureOps: find_leaf_apply, trunc_finish, norm_apply).
    enum RowsBelowOne { BELOW_ONE_BAD_ARG, BELOW_ONE_NOT_SUPPORTED };
    template <class Go>
    static LaunchStatus launch_rows(int nrows, RowsBelowOne below, bool plan_ok, bool empty, Go&& go) {
        if (nrows > MAXK || (below == BELOW_ONE_NOT_SUPPORTED && nrows < 1)) return L_NOT_SUPPORTED;
        if (!plan_ok) return L_PLAN_REFUSED;
        if (empty) return L_OK;
        if (!dispatch_int(IntRange<1, MAXK>(), nrows, go)) return L_BAD_ARG;
        return launched();
    }

    // The local steps of the secure comparison (sgn.hpp): a workgroup per tile of SGN_TILE elements for mask and expand,
    // the streaming plan for finish.  Constants (2^l, 2^(l-1), 2^-l) travel as kernel arguments.
    static LaunchStatus sgn_mask(const void* Fp, const LaunchCfg& lc, const void* a, const void* rbits, const void* rdivl, int l,
                        const uint64_t* consts, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        return tiled(n, l, [&](const SgnPlan& p) {
            hipLaunchKernelGGL((k_sgn_mask<F>), dim3((unsigned)p.tiles), dim3(BLOCK), 0, st, f, (const E*)a, (const E*)rbits,
                               (const E*)rdivl, l, word_at<F>(f, consts, 0), (E*)out, n);
        });
    }
    static LaunchStatus sgn_expand(const void* Fp, const LaunchCfg& lc, const void* c, const void* a, const void* rbits,
                          const void* sbit, int l, const uint64_t* consts, void* e, void* nx, void* z, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        return tiled(n, l, [&](const SgnPlan& p) {
            hipLaunchKernelGGL((k_sgn_expand<F>), dim3((unsigned)p.tiles), dim3(BLOCK), 0, st, f, (const E*)c, (const E*)a,
                               (const E*)rbits, (const E*)sbit, l, word_at<F>(f, consts, 0), (E*)e, (E*)nx, (E*)z, n);
        });
    }
    static LaunchStatus sgn_finish(const void* Fp, const LaunchCfg& lc, const void* w, const void* sbit, const void* z, int l,
                          const uint64_t* consts, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const Plan p = plan(n, al(w) && al(sbit) && al(z) && al(out), lc);
        hipLaunchKernelGGL((k_sgn_finish<F, true>), dim3(p.grid), dim3(BLOCK), 0, st, f, (const E*)w, (const E*)sbit, (const E*)z,
                           word_at<F>(f, consts, 1), word_at<F>(f, consts, 2), (E*)out, p.nvec, n, p.pol);
        return launched();
    }
    // The two ends of a compare-exchange stage (sort.hpp): one flat streaming loop over the compact pair array.
    static LaunchStatus cx_diff(const void* Fp, const LaunchCfg& lc, const void* a, void* out, size_t outer, size_t k, size_t inner,
                       size_t p, size_t d, size_t r, hipStream_t st) {
        const F& f = policy(Fp);
        const CxPlan pl = cx_plan(outer, k, inner, p, d, r, sizeof(E), al(a) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_cx_diff<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, (E*)out, pl);
        });
    }
    template <int K>
    static void go_cx_apply(const F& f, const LaunchCfg& lc, E* a, const void* const* rows, const uint64_t* lam2, size_t outer,
                            size_t k, size_t inner, size_t p, size_t d, size_t r, hipStream_t st) {
        bool vec = al(a);
        const ShareRows<F, K> ra = stage_rows<K>(f, rows, lam2, &vec);
        const CxPlan pl = cx_plan(outer, k, inner, p, d, r, sizeof(E), vec);
        hipLaunchKernelGGL((k_cx_apply<F, K>), dim3(grid_for(pl.total, lc)), dim3(BLOCK), 0, st, f, ra, a, pl);
    }
    static LaunchStatus cx_apply(const void* Fp, const LaunchCfg& lc, void* a, const void* const* rows, const uint64_t* lam2, int nrows,
                        size_t outer, size_t k, size_t inner, size_t p, size_t d, size_t r, hipStream_t st) {
        const F& f = policy(Fp);
        const CxPlan pl = cx_plan(outer, k, inner, p, d, r, sizeof(E), false);
        return launch_rows(nrows, BELOW_ONE_BAD_ARG, pl.ok, pl.total == 0, [&](auto k_) {
            go_cx_apply<decltype(k_)::value>(f, lc, (E*)a, rows, lam2, outer, k, inner, p, d, r, st);
        });
    }
    // The local steps of bit decomposition (bits.hpp): a workgroup per tile of SGN_TILE elements for mask, expand and finish;
    // grid (gx, R) for the two ends of a round, a unit (a pack where bits_plan() admits packs, else an element) per thread up
    // to the grid cap.
    static LaunchStatus bits_mask(const void* Fp, const LaunchCfg& lc, const void* a, const void* rbits, const void* rdivl, int l,
                         const uint64_t* consts, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        return tiled(n, l, [&](const SgnPlan& p) {
            hipLaunchKernelGGL((k_bits_mask<F>), dim3((unsigned)p.tiles), dim3(BLOCK), 0, st, f, (const E*)a, (const E*)rbits,
                               (const E*)rdivl, l, word_at<F>(f, consts, 0), word_at<F>(f, consts, 1), (E*)out, n);
        });
    }
    static LaunchStatus bits_expand(const void* Fp, const LaunchCfg& lc, const void* c, const void* rbits, int l, void* g, void* p,
                           size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        return tiled(n, l, [&](const SgnPlan& pl) {
            hipLaunchKernelGGL((k_bits_expand<F>), dim3((unsigned)pl.tiles), dim3(BLOCK), 0, st, f, (const E*)c, (const E*)rbits, l,
                               (E*)g, (E*)p, n);
        });
    }
    static LaunchStatus bits_finish(const void* Fp, const LaunchCfg& lc, const void* c, const void* rbits, const void* g, int l,
                           void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        return tiled(n, l, [&](const SgnPlan& pl) {
            hipLaunchKernelGGL((k_bits_finish<F>), dim3((unsigned)pl.tiles), dim3(BLOCK), 0, st, f, (const E*)c, (const E*)rbits,
                               (const E*)g, l, (E*)out, n);
        });
    }
    static size_t bits_max_blocks(const LaunchCfg& lc) {
        return lc.blocks_per_cu > 0 ? (size_t)lc.blocks_per_cu * (size_t)lc.num_cu : (size_t)GEOM_MAX_GRID;
    }
    static LaunchStatus carry_prod(const void* Fp, const LaunchCfg& lc, const void* g, const void* p, int l, const BitsLevel& lv,
                          void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const BitsPlan pl = bits_plan(n, l, lv.rc + lv.rd, sizeof(E), al(g) && al(p) && al(out), bits_max_blocks(lc));
        if (!pl.ok) return L_PLAN_REFUSED;
        if (pl.rows == 0 || n == 0) return L_OK;
        hipLaunchKernelGGL((k_carry_prod<F>), dim3(pl.gx, (unsigned)pl.rows), dim3(BLOCK), 0, st, f, (const E*)g, (const E*)p,
                           (E*)out, lv, pl);
        return launched();
    }
    template <int K>
    static void go_carry_apply(const F& f, const LaunchCfg& lc, E* g, E* p, const void* const* rows, const uint64_t* lam2, int l,
                               const BitsLevel& lv, size_t n, hipStream_t st) {
        bool vec = al(g) && al(p);
        const ShareRows<F, K> ra = stage_rows<K>(f, rows, lam2, &vec);
        const BitsPlan pl = bits_plan(n, l, lv.rc + lv.rd, sizeof(E), vec, bits_max_blocks(lc));
        hipLaunchKernelGGL((k_carry_apply<F, K>), dim3(pl.gx, (unsigned)pl.rows), dim3(BLOCK), 0, st, f, ra, g, p, lv, pl);
    }
    static LaunchStatus carry_apply(const void* Fp, const LaunchCfg& lc, void* g, void* p, const void* const* rows, const uint64_t* lam2,
                           int nrows, int l, const BitsLevel& lv, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const BitsPlan pl = bits_plan(n, l, lv.rc + lv.rd, sizeof(E), false, bits_max_blocks(lc));
        return launch_rows(nrows, BELOW_ONE_BAD_ARG, pl.ok, pl.rows == 0 || n == 0, [&](auto k_) {
            go_carry_apply<decltype(k_)::value>(f, lc, (E*)g, (E*)p, rows, lam2, l, lv, n, st);
        });
    }
    // The ends of a tournament round (tour.hpp): one flat streaming loop over the compact pair array.  unit_prod touches the
    // half level and the compact arrays only, which lie as in a HALVES round; unit_expand interleaves: an ODD_EVEN round.
    static LaunchStatus tour_diff(const void* Fp, const LaunchCfg& lc, const void* a, void* out, size_t outer, size_t k, size_t inner,
                         int mode, int neg, hipStream_t st) {
        const F& f = policy(Fp);
        const TourPlan pl = tour_plan(outer, k, inner, mode, sizeof(E), al(a) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_tour_diff<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, (E*)out, pl, neg ? 1 : 0);
        });
    }
    static LaunchStatus tour_unit_prod(const void* Fp, const LaunchCfg& lc, const void* u, const void* c, void* out, size_t outer,
                              size_t k, size_t inner, hipStream_t st) {
        const F& f = policy(Fp);
        const TourPlan pl = tour_plan(outer, k, inner, TOUR_HALVES, sizeof(E), al(u) && al(c) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_tour_unit_prod<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)u, (const E*)c, (E*)out, pl);
        });
    }
    // select (expand == false) and unit_expand share everything but the kernel
    template <int K>
    static void go_tour_rows(const F& f, const LaunchCfg& lc, bool expand, const E* a, const void* const* rows, const uint64_t* lam2,
                             E* out, size_t outer, size_t k, size_t inner, int mode, int neg, hipStream_t st) {
        bool vec = al(a) && al(out);
        const ShareRows<F, K> ra = stage_rows<K>(f, rows, lam2, &vec);
        const TourPlan pl = tour_plan(outer, k, inner, mode, sizeof(E), vec);
        if (expand) hipLaunchKernelGGL((k_tour_unit_expand<F, K>), dim3(grid_for(pl.total, lc)), dim3(BLOCK), 0, st, f, ra, a, out, pl);
        else hipLaunchKernelGGL((k_tour_select<F, K>), dim3(grid_for(pl.total, lc)), dim3(BLOCK), 0, st, f, ra, a, out, pl, neg ? 1 : 0);
    }
    static LaunchStatus tour_rows(const void* Fp, const LaunchCfg& lc, bool expand, const void* a, const void* const* rows,
                         const uint64_t* lam2, int nrows, void* out, size_t outer, size_t k, size_t inner, int mode, int neg,
                         hipStream_t st) {
        const F& f = policy(Fp);
        const TourPlan pl = tour_plan(outer, k, inner, mode, sizeof(E), false);
        return launch_rows(nrows, BELOW_ONE_BAD_ARG, pl.ok, pl.total == 0, [&](auto k_) {
            go_tour_rows<decltype(k_)::value>(f, lc, expand, (const E*)a, rows, lam2, (E*)out, outer, k, inner, mode, neg, st);
        });
    }
    static LaunchStatus tour_select(const void* Fp, const LaunchCfg& lc, const void* a, const void* const* rows, const uint64_t* lam2,
                           int nrows, void* out, size_t outer, size_t k, size_t inner, int mode, int neg, hipStream_t st) {
        return tour_rows(Fp, lc, false, a, rows, lam2, nrows, out, outer, k, inner, mode, neg, st);
    }
    static LaunchStatus tour_unit_expand(const void* Fp, const LaunchCfg& lc, const void* u, const void* const* rows,
                                const uint64_t* lam2, int nrows, void* out, size_t outer, size_t k, size_t inner, hipStream_t st) {
        return tour_rows(Fp, lc, true, u, rows, lam2, nrows, out, outer, k, inner, TOUR_ODD_EVEN, 0, st);
    }
    // The ends of a round of the first-occurrence search (find.hpp): one flat streaming loop over the compact units of one
    // component; a thread walks the components of its unit.
    static LaunchStatus find_leaf_prod(const void* Fp, const LaunchCfg& lc, const void* bits, const void* tab, void* out, size_t outer,
                              size_t k, size_t inner, int ncomp, int flip, int virt, hipStream_t st) {
        const F& f = policy(Fp);
        const FindPlan pl = find_leaf_plan(outer, k, inner, ncomp, virt, sizeof(E), al(bits) && al(out));
        return flat(pl.t.ok, pl.t.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_find_leaf_prod<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)bits, (const E*)tab, (E*)out, pl,
                               ncomp, flip ? 1 : 0);
        });
    }
    template <int K>
    static void go_find_leaf_apply(const F& f, const LaunchCfg& lc, const E* bits, const E* tab, const void* const* rows,
                                   const uint64_t* lam2, E* out, size_t outer, size_t k, size_t inner, int ncomp, int flip, int virt,
                                   hipStream_t st) {
        bool vec = al(bits) && al(out);
        const ShareRows<F, K> ra = stage_rows<K>(f, rows, lam2, &vec);
        const FindPlan pl = find_leaf_plan(outer, k, inner, ncomp, virt, sizeof(E), vec);
        hipLaunchKernelGGL((k_find_leaf_apply<F, K>), dim3(grid_for(pl.t.total, lc)), dim3(BLOCK), 0, st, f, ra, bits, tab, out, pl,
                           ncomp, flip ? 1 : 0);
    }
    static LaunchStatus find_leaf_apply(const void* Fp, const LaunchCfg& lc, const void* bits, const void* tab, const void* const* rows,
                               const uint64_t* lam2, int nrows, void* out, size_t outer, size_t k, size_t inner, int ncomp,
                               int flip, int virt, hipStream_t st) {
        const F& f = policy(Fp);
        const FindPlan pl = find_leaf_plan(outer, k, inner, ncomp, virt, sizeof(E), false);
        return launch_rows(nrows, BELOW_ONE_NOT_SUPPORTED, pl.t.ok, pl.t.total == 0, [&](auto k_) {
            go_find_leaf_apply<decltype(k_)::value>(f, lc, (const E*)bits, (const E*)tab, rows, lam2, (E*)out, outer, k, inner,
                                                    ncomp, flip, virt, st);
        });
    }
    static LaunchStatus find_prod(const void* Fp, const LaunchCfg& lc, const void* level, void* out, size_t outer, size_t k,
                         size_t inner, int ncomp, hipStream_t st) {
        const F& f = policy(Fp);
        const FindPlan pl = find_plan(outer, k, inner, ncomp, sizeof(E), al(level) && al(out));
        return flat(pl.t.ok, pl.t.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_find_prod<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)level, (E*)out, pl, ncomp);
        });
    }
    // The local steps of fixed-point truncation and normalisation (fxp.hpp): a workgroup per tile of SGN_TILE elements for
    // the mask, as for bits_mask; one flat streaming loop for the other three.
    static LaunchStatus trunc_mask(const void* Fp, const LaunchCfg& lc, const void* a, const void* rbits, const void* rdivf, int fb,
                          const uint64_t* consts, void* ar, void* masked, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        return tiled(n, fb, [&](const SgnPlan& p) {
            hipLaunchKernelGGL((k_trunc_mask<F>), dim3((unsigned)p.tiles), dim3(BLOCK), 0, st, f, (const E*)a, (const E*)rbits,
                               (const E*)rdivf, fb, word_at<F>(f, consts, 0), word_at<F>(f, consts, 1), (E*)ar, (E*)masked, n);
        });
    }
    template <int K>
    static void go_trunc_finish(const F& f, const LaunchCfg& lc, const void* const* rows, const uint64_t* lam2, const E* ar, int fb,
                                const uint64_t* consts, E* out, size_t n, hipStream_t st) {
        bool vec = al(ar) && al(out);
        const ShareRows<F, K> ra = stage_rows<K>(f, rows, lam2, &vec);
        const FlatPlan pl = flat_plan(n, sizeof(E), vec);
        const uint64_t cmask = fb >= 64 ? ~0ull : (1ull << fb) - 1;         // (no shift by 64)
        hipLaunchKernelGGL((k_trunc_finish<F, K>), dim3(grid_for(pl.total, lc)), dim3(BLOCK), 0, st, f, ra, ar, cmask,
                           word_at<F>(f, consts, 0), out, pl);
    }
    static LaunchStatus trunc_finish(const void* Fp, const LaunchCfg& lc, const void* const* rows, const uint64_t* lam2, int nrows,
                            const void* ar, int fb, const uint64_t* consts, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const bool plan_ok = fb >= 1 && fb <= FXP_MAX_BITS && flat_plan(n, sizeof(E), false).ok;
        return launch_rows(nrows, BELOW_ONE_NOT_SUPPORTED, plan_ok, n == 0, [&](auto k_) {
            go_trunc_finish<decltype(k_)::value>(f, lc, rows, lam2, (const E*)ar, fb, consts, (E*)out, n, st);
        });
    }
    static LaunchStatus norm_prod(const void* Fp, const LaunchCfg& lc, const void* bits, int l, void* out, void* sign_out, size_t n,
                         hipStream_t st) {
        const F& f = policy(Fp);
        const RevPlan pl = fxp_norm_plan(n, l, sizeof(E), al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_norm_prod<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)bits, (E*)out, (E*)sign_out, pl);
        });
    }
    template <int K>
    static void go_norm_apply(const F& f, const LaunchCfg& lc, const E* bits, const void* const* rows, const uint64_t* lam2, int l,
                              E* out, size_t n, hipStream_t st) {
        bool vec = al(out);
        const ShareRows<F, K> ra = stage_rows<K>(f, rows, lam2, &vec);
        const RevPlan pl = fxp_norm_plan(n, l, sizeof(E), vec);
        hipLaunchKernelGGL((k_norm_apply<F, K>), dim3(grid_for(pl.total, lc)), dim3(BLOCK), 0, st, f, ra, bits, out, pl);
    }
    static LaunchStatus norm_apply(const void* Fp, const LaunchCfg& lc, const void* bits, const void* const* rows, const uint64_t* lam2,
                          int nrows, int l, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const RevPlan pl = fxp_norm_plan(n, l, sizeof(E), false);
        return launch_rows(nrows, BELOW_ONE_NOT_SUPPORTED, pl.ok, pl.total == 0, [&](auto k_) {
            go_norm_apply<decltype(k_)::value>(f, lc, (const E*)bits, rows, lam2, l, (E*)out, n, st);
        });
    }
    // The local steps under the secure logarithm and exponential (explog.hpp): one flat streaming loop; pow_base is bound by
    // its products and stages its table per workgroup: eight workgroups per compute unit at the most, each over many elements.
    static LaunchStatus powers_prod(const void* Fp, const LaunchCfg& lc, const void* P, size_t stride, int h, int w, void* out, size_t n,
                           hipStream_t st) {
        const F& f = policy(Fp);
        if (!explog_prod_valid(h, w)) return L_PLAN_REFUSED;
        const RowsPlan pl = rows_plan(n, (size_t)h, stride, sizeof(E), al(P) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_powers_prod<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)P, h, w, (E*)out, pl, n);
        });
    }
    static LaunchStatus poly_dot(const void* Fp, const LaunchCfg& lc, const void* P, size_t stride, int theta, const void* tab,
                        const uint64_t* c0, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        if (!explog_poly_valid(theta)) return L_PLAN_REFUSED;
        const RowsPlan pl = rows_plan(n, (size_t)theta, stride, sizeof(E), al(P) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_poly_dot<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)P, theta, (const E*)tab,
                               word_at<F>(f, c0, 0), (E*)out, pl);
        });
    }
    static LaunchStatus pow_base(const void* Fp, const LaunchCfg& lc, const void* x, int shift, int ebits, int pbits, const void* tab,
                        void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const PowBasePlan pl = pow_base_plan(n, shift, ebits, pbits, sizeof(E));
        return flat(pl.ok && pl.nwin <= pow_base_max_windows(sizeof(E)), n, lc, [&](unsigned want) {
            const unsigned cap = (unsigned)(lc.num_cu > 0 ? lc.num_cu : 1) * 8u;
            hipLaunchKernelGGL((k_pow_base<F>), dim3(want < cap ? want : cap), dim3(BLOCK), 0, st, f, (const E*)x, (const E*)tab, (E*)out,
                               pl, n);
        });
    }
    static LaunchStatus bits_reverse(const void* Fp, const LaunchCfg& lc, const void* bits, int l, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const RevPlan pl = explog_rev_plan(n, l, sizeof(E), al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_bits_reverse<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)bits, (E*)out, pl);
        });
    }
    // The local steps of the Legendre zero test (iszero.hpp).  mask and finish: one flat streaming loop; whole packs also need
    // the code bytes aligned to the one access that moves a pack's codes.  legendre_code is the launch of pow with a byte
    // array for an output: the same packs through the vector loop and the same grid (stream_plan takes its nvec where plan()
    // does: stream_nvec, geom.hpp); its pl.threads is 0 for count == 0 only.
    static bool codes_al(const void* code) { return iszero_codes_aligned((uintptr_t)code, sizeof(E)); }
    static LaunchStatus iszero_mask(const void* Fp, const LaunchCfg& lc, const void* a, const void* r, const void* z, const void* u2, int k,
                           void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const RowsPlan pl = iszero_mask_plan(n, k, sizeof(E), al(a) && al(r) && al(z) && al(u2) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_iszero_mask<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, (const E*)r, (const E*)z,
                               (const E*)u2, k, (E*)out, pl);
        });
    }
    static LaunchStatus legendre_code(const void* Fp, const LaunchCfg& lc, const void* c, const ExpArgs* ex, uint8_t* code, size_t count,
                             hipStream_t st) {
        const F& f = policy(Fp);
        const StreamPlan pl = stream_plan(count, sizeof(E), al(c) && codes_al(code));
        return flat(pl.ok, pl.threads, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_legendre_code<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)c, *ex, code, pl.nvec, count);
        });
    }
    static LaunchStatus iszero_finish(const void* Fp, const LaunchCfg& lc, const uint8_t* code, const void* z, void* out, size_t count,
                             hipStream_t st) {
        const F& f = policy(Fp);
        const FlatPlan pl = flat_plan(count, sizeof(E), al(z) && al(out) && codes_al(code));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_iszero_finish<F>), dim3(grid), dim3(BLOCK), 0, st, f, code, (const E*)z, (E*)out, pl);
        });
    }
    // The local steps of secure random bits (rbits.hpp): the plan, grid and launch bounds of pow (rbits_open_plan /
    // rbits_finish_plan are stream_plan: tests/rbits_check.cpp).  The opening keeps whole packs for up to rbits_fused_rows()
    // rows, with the row count a template parameter as in recombine; more rows (up to MAXK_ANY) go by elements.
    template <int K>
    static void go_rbits_open(const F& f, const LaunchCfg& lc, const void* const* r, const void* const* z, const uint64_t* lam2, E* out,
                              int* zeros, size_t n, hipStream_t st) {
        RbitsOpenArgs<F, K> ra;
        bool vec = al(out);
        for (int j = 0; j < K; ++j) {
            ra.r[j] = (const E*)r[j];
            ra.z[j] = (const E*)z[j];
            ra.lam[j] = f.prep(word_at<F>(f, lam2, (size_t)j));
            vec = vec && al(r[j]) && al(z[j]);
        }
        const StreamPlan pl = rbits_open_plan(n, K, sizeof(E), vec);
        hipLaunchKernelGGL((k_rbits_open<F, K>), dim3(grid_for(pl.threads, lc)), dim3(BLOCK), 0, st, f, ra, out, zeros, pl.nvec, n);
    }
    static LaunchStatus rbits_open(const void* Fp, const LaunchCfg& lc, const void* const* r, const void* const* z, const uint64_t* lam2,
                          int k, void* out, int* zeros, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const StreamPlan pl = rbits_open_plan(n, k, sizeof(E), false);
        if (!pl.ok) return L_PLAN_REFUSED;
        if (n == 0) return L_OK;
        if (k > rbits_fused_rows(sizeof(E))) {
            static_assert(sizeof(RbitsOpenArgsAny<F>) + sizeof(F) + 64 <= 4096, "kernel arguments");
            RbitsOpenArgsAny<F> ra;
            for (int j = 0; j < MAXK_ANY; ++j) {
                const int s = j < k ? j : 0;
                ra.r[j] = (const E*)r[s];
                ra.z[j] = (const E*)z[s];
                ra.lam[j] = f.prep(word_at<F>(f, lam2, (size_t)s));
            }
            hipLaunchKernelGGL((k_rbits_open_any<F>), dim3(grid_for(pl.threads, lc)), dim3(BLOCK), 0, st, f, ra, k, (E*)out, zeros, n);
            return launched();
        }
        if (!dispatch_int(IntRange<1, rbits_fused_rows(sizeof(E))>(), k,
                          [&](auto k_) { go_rbits_open<decltype(k_)::value>(f, lc, r, z, lam2, (E*)out, zeros, n, st); }))
            return L_BAD_ARG;
        return launched();
    }
    static LaunchStatus rbits_finish(const void* Fp, const LaunchCfg& lc, const void* c, const ExpArgs* ex, const void* const* r,
                            void* const* b, int m, const uint64_t* A2, const uint64_t* B2, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        static_assert(sizeof(RbitsFinishArgs<F>) + sizeof(F) + sizeof(ExpArgs) + 64 <= 4096, "kernel arguments");
        if (!rbits_rows_valid(m)) return L_PLAN_REFUSED;
        RbitsFinishArgs<F> fa;
        bool vec = al(c);
        for (int j = 0; j < MAXK_ANY; ++j) {
            const int s = j < m ? j : 0;
            fa.r[j] = (const E*)r[s];
            fa.b[j] = (E*)b[s];
            vec = vec && al(r[s]) && al(b[s]);
        }
        fa.A = word_at<F>(f, A2, 0);
        fa.B = word_at<F>(f, B2, 0);
        fa.m = m;
        const StreamPlan pl = rbits_finish_plan(n, m, sizeof(E), vec);
        if (!pl.ok) return L_PLAN_REFUSED;
        if (n == 0) return L_OK;
        hipLaunchKernelGGL((k_rbits_finish<F>), dim3(grid_for(pl.threads, lc)), dim3(BLOCK), 0, st, f, (const E*)c, *ex, fa, pl.nvec, n);
        return launched();
    }
    // The local steps of the secure binary sign (bsgn.hpp).  mask: one flat streaming loop over the units of a row, the
    // launch of iszero_mask.  finish in rows mode: the launch of pow over the w n opened values, as legendre_code and
    // rbits_finish (bsgn_flat_plan is stream_plan over w n); in sum mode: a flat loop over the units of a row, bound by the w
    // exponentiations of a unit.
    static LaunchStatus bsgn_mask(const void* Fp, const LaunchCfg& lc, const void* a, const void* z, const uint64_t* alpha2,
                         const uint64_t* beta2, int w, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const RowsPlan pl = bsgn_rows_plan(n, w, sizeof(E), al(a) && al(z) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            BsgnMaskArgs<F> ma;
            ma.alpha = word_at<F>(f, alpha2, 0);
            for (int i = 0; i < BSGN_MAX_ROWS; ++i) ma.beta[i] = word_at<F>(f, beta2, (size_t)(i < w ? i : 0));
            hipLaunchKernelGGL((k_bsgn_mask<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)a, (const E*)z, ma, w, (E*)out, pl);
        });
    }
    static LaunchStatus bsgn_finish(const void* Fp, const LaunchCfg& lc, const void* c, const ExpArgs* ex, const void* const* s,
                           void* const* out, int m, int w, int sum, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        static_assert(sizeof(BsgnFinishArgs<F>) + sizeof(F) + sizeof(ExpArgs) + sizeof(RowsPlan) + 64 <= 4096, "kernel arguments");
        if (!bsgn_m_valid(m) || !bsgn_w_valid(w)) return L_PLAN_REFUSED;
        BsgnFinishArgs<F> fa;
        bool vec = al(c);
        for (int j = 0; j < BSGN_MAX_PARTIES; ++j) {
            const int q = j < m ? j : 0;
            fa.s[j] = (const E*)s[q];
            fa.out[j] = (E*)out[q];
            vec = vec && al(s[q]) && al(out[q]);
        }
        fa.m = m;
        if (sum) {
            const RowsPlan pl = bsgn_rows_plan(n, w, sizeof(E), vec);
            return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
                hipLaunchKernelGGL((k_bsgn_finish_sum<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)c, *ex, fa, w, pl);
            });
        }
        const StreamPlan pl = bsgn_flat_plan(n, w, sizeof(E), vec);
        return flat(pl.ok, pl.threads, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_bsgn_finish<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)c, *ex, fa, pl.nvec, (size_t)w * n);
        });
    }
    // The local steps under secure unit vectors and table lookup (unitvec.hpp): one flat streaming loop over the units of a
    // row.  unit_roll reads U by element: only c and the output decide on packs.  unit_dot stages its table per workgroup, as
    // pow_base does: eight workgroups per compute unit at the most, each over many elements; the table's bytes are the
    // launch's dynamic LDS.
    static LaunchStatus unit_prod(const void* Fp, const LaunchCfg& lc, const void* x, size_t xstride, const void* U, size_t h, void* out,
                         size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        size_t xspan;
        if (h < 1 || !unit_x_span(n, xstride, sizeof(E), xspan)) return L_PLAN_REFUSED;
        const RowsPlan pl = unit_rows_plan(n, h, sizeof(E), al(U) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_unit_prod<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)x, xstride, (const E*)U, h, (E*)out, pl,
                               unit_x_packs(pl, xstride) && al(x) ? 1 : 0);
        });
    }
    static LaunchStatus unit_roll(const void* Fp, const LaunchCfg& lc, const void* U, const void* c, int kbits, size_t K, void* out,
                         size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        if (!unit_roll_valid(kbits, K)) return L_PLAN_REFUSED;
        const RowsPlan pl = unit_rows_plan(n, (size_t)1 << kbits, sizeof(E), al(c) && al(out));
        return flat(pl.ok, pl.total, lc, [&](unsigned grid) {
            hipLaunchKernelGGL((k_unit_roll<F>), dim3(grid), dim3(BLOCK), 0, st, f, (const E*)U, (const E*)c, unit_mask(kbits), K, (E*)out,
                               pl, n);
        });
    }
    static_assert(unit_word_bytes(sizeof(E)) == sizeof(typename F::word), "unitvec_geom.hpp states this field's word");
    static LaunchStatus unit_dot(const void* Fp, const LaunchCfg& lc, const void* U, size_t rows, const void* c, int kbits,
                        const void* tab, size_t tlen, void* out, size_t n, hipStream_t st) {
        const F& f = policy(Fp);
        const UnitDotPlan dp = unit_dot_plan(rows, c != nullptr, kbits, tlen, sizeof(E));
        if (!dp.ok) return L_PLAN_REFUSED;
        if (!dp.fits) return L_NOT_SUPPORTED;
        const RowsPlan pl = unit_rows_plan(n, rows, sizeof(E), al(U) && al(out) && (!c || al(c)));
        return flat(pl.ok, pl.total, lc, [&](unsigned want) {
            const unsigned cap = (unsigned)(lc.num_cu > 0 ? lc.num_cu : 1) * 8u;
            hipLaunchKernelGGL((k_unit_dot<F>), dim3(want < cap ? want : cap), dim3(BLOCK), (unsigned)dp.lds_bytes, st, f, (const E*)U, rows,
                               (const E*)c, dp.mask, (const E*)tab, tlen, dp.entries, (E*)out, pl);
        });
    }
    // The 2-D correlation (conv2d.hpp): grid (k tiles channel-blocks, senders), the shape by conv2d_plan(): wide once its
    // workgroups give every compute unit lc.conv_wide_per_cu of them, as for ffgpu_convolve; the staged channels are the
    // launch's dynamic LDS.
    static Conv2dPlan conv2d_plan_of(const LaunchCfg& lc, size_t k, size_t r, size_t m, size_t n, size_t v, int s, int nsend) {
        return conv2d_plan(k, r, m, n, v, s, nsend, lc.num_cu, lc.conv_wide_per_cu, sizeof(E), conv2d_slot_bytes<F>(), DotAcc<F>::FLUSH);
    }
    static LaunchStatus conv2d(const void* Fp, const LaunchCfg& lc, const void* const* x, const void* const* w, const void* const* b,
                      void* const* out, int nsend, size_t k, size_t r, size_t m, size_t n, size_t v, int s, hipStream_t st) {
        const F& f = policy(Fp);
        static_assert(sizeof(Conv2dArgs<F>) + sizeof(F) + sizeof(Conv2dGeom) + 64 <= 4096, "kernel arguments");
        if (nsend > (int)CONV2D_MAX_SENDERS) return L_NOT_SUPPORTED;
        const Conv2dPlan pl = conv2d_plan_of(lc, k, r, m, n, v, s, nsend);
        if (!pl.ok) return L_PLAN_REFUSED;
        if (pl.empty) return L_OK;
        if (!pl.grid_ok) return L_NOT_SUPPORTED;
        Conv2dArgs<F> ca;
        for (int j = 0; j < (int)CONV2D_MAX_SENDERS; ++j) {
            const int q = j < nsend ? j : 0;
            ca.x[j] = (const E*)x[q];
            ca.w[j] = (const E*)w[q];
            ca.b[j] = b ? (const E*)b[q] : nullptr;
            ca.out[j] = (E*)out[q];
        }
        const dim3 grid((unsigned)pl.grid_x, pl.grid_y);
        if (pl.wide) hipLaunchKernelGGL((k_conv2d<F, Conv2dWide>), grid, dim3(BLOCK), (unsigned)pl.lds_bytes, st, f, ca, pl.g);
        else hipLaunchKernelGGL((k_conv2d<F, Conv2dNarrow>), grid, dim3(BLOCK), (unsigned)pl.lds_bytes, st, f, ca, pl.g);
        return launched();
    }

    static const SecureOps* table() {
        static const SecureOps ops = {
            .sgn_mask = &sgn_mask, .sgn_expand = &sgn_expand, .sgn_finish = &sgn_finish,
            .cx_diff = &cx_diff, .cx_apply = &cx_apply,
            .bits_mask = &bits_mask, .bits_expand = &bits_expand, .carry_prod = &carry_prod, .carry_apply = &carry_apply,
            .bits_finish = &bits_finish,
            .tour_diff = &tour_diff, .tour_select = &tour_select, .tour_unit_prod = &tour_unit_prod,
            .tour_unit_expand = &tour_unit_expand,
            .find_leaf_prod = &find_leaf_prod, .find_leaf_apply = &find_leaf_apply, .find_prod = &find_prod,
            .trunc_mask = &trunc_mask, .trunc_finish = &trunc_finish, .norm_prod = &norm_prod, .norm_apply = &norm_apply,
            .powers_prod = &powers_prod, .poly_dot = &poly_dot, .pow_base = &pow_base, .bits_reverse = &bits_reverse,
            .iszero_mask = &iszero_mask, .legendre_code = &legendre_code, .iszero_finish = &iszero_finish,
            .rbits_open = &rbits_open, .rbits_finish = &rbits_finish,
            .bsgn_mask = &bsgn_mask, .bsgn_finish = &bsgn_finish,
            .unit_prod = &unit_prod, .unit_roll = &unit_roll, .unit_dot = &unit_dot,
            .conv2d = &conv2d, .conv2d_plan = &conv2d_plan_of};
        return &ops;
    }
};

// the secure steps of a policy: the table of its launchers over a prime field, none over GF(2^n) (whose contexts the entries
// turn away before they look: PRIME_CTX, and ffgpu_ctx_create checks that the table matches the kind)
template <class F>
const SecureOps* secure_ops() {
    if constexpr (F::BINARY) return nullptr;
    else return SecureLaunchers<F>::table();
}

}  // namespace ffgpu
