"""TEST INFRASTRUCTURE ONLY: the driver of the contract tests of ffgpu_matmul (include/ffgpu.h) on every route of its
dispatcher, Launchers::matmul (mpyc_amd/csrc/launch.hpp) behind matmul_one (api.hip).

plan() restates that dispatcher in plain Python: which kernel a call takes, with which flags, how K is split, and how
many terms one thread accumulates at most -- the number every flush test follows from.  The case generators derive
their shapes from the constants of that plan (thresholds, tile sizes, the CU count) and name the route and the flags
they mean to reach; Driver.run asserts both against plan() before it makes the call, so a case that is routed
elsewhere fails instead of passing on another kernel.

One case = one call on views into ONE backing tensor  guard | A | guard | B | guard | C | guard,  guards of 0xA5, a
view 16-byte aligned or one element in, C pre-filled with canonical noise.  After the call the whole tensor is
compared byte for byte with an image: C's M x N block holds the reference, the ldc - N pads, A, B and every guard are
what was uploaded.  Violations carry the kinds 'out', 'pad', 'input', 'guard'.

Data: 'max' -- every element q - 1, the most an accumulator holds between two flushes, expectation K (q - 1)^2 in
closed form; 'per' -- rows of A repeat with period PA = 7, columns of B with period PB = 5 (odd: no factor in common
with a tile of 2, 16, 64 or 256), edge values first, so the reference is computed for one period (oracle/fforacle.c
through coracle.matmul up to 128 bits, Python integers for 24-byte fields) and tiled, and large operands are assembled
on the device from the uploaded period.  Expected values never come from the library.

Nothing here imports the GPU at module level: tests/test_matmul_contract_host.py drives the same code against
tests/cpuctx.CpuFieldContext and against deliberately wrong adapters."""
import functools
import math
import os
import random
from types import SimpleNamespace

import numpy as np

from ew_contract import ContractViolation, GUARD_BYTE, ints_to_bytes
from oracle import pyoracle as po
from oracle.coracle import elem_bytes
from second_tier_contract import word_bytes, _hex

OK, EINVAL = 0, 1                       # include/ffgpu.h: FFGPU_OK, FFGPU_EINVAL

# ---- the dispatcher's constants, restated (each with the place it lives; those places name this file) ------------------------
BLOCK = 256                             # kernels.hpp: enum { BLOCK = 256 }
SKINNY_MAX = 8                          # matmul.hpp: enum { SKINNY_MAX = 8, SKINNY_FLUSH = 192 }
SKINNY_FLUSH = 192                      # matmul.hpp, the same line: the flush bound of the column-sum kernels
DOT_FLUSH = 192                         # kernels.hpp DotAcc: enum { NL = 1, FLUSH = 192 }
LAZY_FLUSH = 32                         # fields.hpp: enum { FF_D28_MAX_TERMS = 32 }, DotAcc<F>::FLUSH of the digit accumulators
MATVEC_SUB_KT = 512                     # matmul.hpp: constexpr int MATVEC_SUB_KT = 512, MATVEC_SUB_U = 4
VECMAT_KT = 32                          # matmul.hpp: constexpr int VECMAT_KT = 32
VECMAT_COL_KT = 128                     # matmul.hpp: constexpr int VECMAT_COL_KT = 128
VECMAT_FINAL_G = 8                      # matmul.hpp: constexpr int VECMAT_FINAL_G = 8
LIMB_KCHUNK = 8192                      # matmul.hpp: enum { LIMB_KCHUNK = 8192 }
LIMB_KCHUNK_WIDE = 4096                 # matmul.hpp: enum { LIMB_KCHUNK_WIDE = 4096 }
SCRATCH_BYTES = 64 << 20                # api.hip matmul_one: 64 MiB of split-K slabs / partial sums
SCRATCH_MAX = 8 << 30                   # api.hip matmul_one: plane requests above 8 GiB fall back to the vector ALUs
SCRATCH_TILES = 2048                    # api.hip matmul_one: scratch without planes only below 2048 tiles of 32 x 32 ...
SCRATCH_MIN_K = 64                      # ... and from K = 64 on
SHORT_ROWS_MAX_K = 32                   # launch.hpp go_matvec: K <= 32 && M >= 1024 -> k_matvec_short_rows
SHORT_ROWS_MIN_M = 1024
ROWS_R_MIN_K = 1024                     # launch.hpp go_matvec: vec && K >= 1024 && M >= 1024 * R, R = 2
ROWS_R_MIN_M = 2048
SKINNY_N_MIN_M = 64                     # launch.hpp mm_skinny_n: m.M < 64 -> not skinny
SKINNY_M_MIN_N = 64                     # launch.hpp mm_skinny_m: N < 64 -> not skinny
SUB_COL_MIN_K = 64                      # launch.hpp go_matvec_col: ... && K >= 64
VECMAT_TARGET = 1024                    # launch.hpp mm_skinny_m: target = 1024 workgroups
VECMAT_MIN_CHUNK = 8                    # launch.hpp mm_skinny_m: ks <= (K + 7) / 8
MFMA_MIN_K = 64                         # launch.hpp mfma_plane_bytes: K < 64 -> 0
MFMA_MIN_DEFAULT = 8e7                  # api.hip SWITCHES: FFGPU_MM_MFMA_MIN
MFMA_SPLIT_TILES = 128                  # launch.hpp mm_mfma: tiles <= 128 && Kp >= 512
MFMA_SPLIT_KP = 512
MFMA_SLAB = 256                         # launch.hpp mm_mfma: ks <= Kp / 256
BRAW_MAX_ROW_TILES = 2                  # launch.hpp mm_mfma: gg.y <= 2 (up to 128 rows)
VALU_SMALL_TILES = 64                   # launch.hpp mm_valu: small_out = tiles of 64 x 32 < 64
VALU_SPLIT_TILES = 512                  # launch.hpp mm_valu: tiles < 512 && K >= 64
VALU_SPLIT_MIN_K = 64
VALU_SPLIT_TARGET = 1024                # launch.hpp mm_valu: ks = ceil(1024 / tiles), at most K / 32
VALU_BK = 16                            # matmul_tile_body.hpp: BK = 16; slabs are whole k-steps

PA, PB = 7, 5                           # the periods of the rows of A and of the columns of B
NOISE = 101                             # elements of the noise C is pre-filled with
GUARD = 1024                            # bytes of guard between the operands (>= 42 elements of any field)

ROUTES = ('short_rows', 'rows_r', 'rows', 'sub_col16', 'sub_col64', 'rows_col', 'vecmat', 'vecmat_col', 'mfma_glds',
          'mfma_l4', 'mfma_wide', 'valu_4x2', 'valu_2x2', 'valu_bytes')


def cdiv(a, b):
    return -(-a // b)


# ---- what the dispatcher knows of a field ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def traits(modulus, binary):
    """everything Launchers<F>::matmul reads off its policy F, from the modulus alone (policy_build.hpp picks F)"""
    eb = elem_bytes(modulus, binary)
    wb = word_bytes(eb)
    k = modulus.bit_length()
    pm = (not binary) and (1 << k) - modulus < (1 << 31)           # 2^k - c with a small c
    t = SimpleNamespace(modulus=modulus, binary=binary, eb=eb, wb=wb)
    t.q = (1 << (k - 1)) if binary else modulus
    t.epw = 4 if eb == 1 else 1                                     # F::EPW
    t.pack = 1 if wb > 16 else 16 // wb                             # Pack<W>::N
    t.pack_align = 4 if eb == 12 else 16                            # Launchers::PACK_ALIGN
    t.col_mac = (not binary) and eb == 8                            # fields.hpp col_mac_ok: PM64<*>, RC64
    t.lazy = pm and eb in (12, 16, 24)                              # DotAcc<F>::lazy: PM96, PM128<*>, PM192 have F::lacc
    t.flush = LAZY_FLUSH if t.lazy else DOT_FLUSH                   # DotAcc<F>::FLUSH
    t.mfma = 0 if binary or eb > 16 else (4 if eb == 4 else 8 if eb == 8 else 12 if eb == 12 else 16)   # digits per operand
    t.skinny_n_max = 4 if wb > 16 else SKINNY_MAX                   # launch.hpp mm_skinny_n
    t.ld_unit = t.pack_align // math.gcd(t.pack_align, eb)          # stride_ok(ld) <=> ld % ld_unit == 0
    t.one_in_unaligned = eb % t.pack_align != 0                     # a view one element in fails Launchers::al
    return t


def env_of(num_cu=256, mfma_min=None, mfma_on=None):
    """the run-time inputs of the plan: LaunchCfg::num_cu, FFGPU_MM_MFMA_MIN and FFGPU_MM_MFMA as api.hip reads them"""
    if mfma_min is None:
        mfma_min = float(os.environ.get('FFGPU_MM_MFMA_MIN', MFMA_MIN_DEFAULT))
    if mfma_on is None:
        mfma_on = int(os.environ.get('FFGPU_MM_MFMA', '1'))
    return SimpleNamespace(num_cu=int(num_cu), mfma_min=float(mfma_min), mfma_on=int(mfma_on))


def ld_up(t, x):
    """the smallest leading dimension >= x with stride_ok"""
    return cdiv(x, t.ld_unit) * t.ld_unit


def ld_bad(t, x):
    """the smallest leading dimension >= x without stride_ok (fields with ld_unit > 1 only)"""
    assert t.ld_unit > 1
    return x if x % t.ld_unit else x + 1


def vecmat_col_unr(M):
    return 8 if M <= 4 else 4 if M < 8 else 16                     # launch.hpp VecmatCol<MM>::UNR


def vecmat_col_per_cu(M):
    return 4 if M <= 4 else 3 if M < 8 else 2                      # launch.hpp vecmat_col_per_cu


def mfma_plane_bytes(env, digits, M, K, N):
    """launch.hpp mfma_plane_bytes"""
    if not env.mfma_on or M <= SKINNY_MAX or N <= SKINNY_MAX or K < MFMA_MIN_K or float(M) * N * K < env.mfma_min:
        return 0
    return digits * (cdiv(M, 64) * 64 + cdiv(N, 64) * 64) * (cdiv(K, 32) * 32)


def _stream_terms(K, epv, vec):
    """the terms of thread 0 of a workgroup that walks a row of K elements: packs of epv, then a scalar tail"""
    nvec = K // epv if vec else 0
    return cdiv(nvec, BLOCK) * epv + cdiv(K - nvec * epv, BLOCK)


def plan(t, M, K, N, lda, ldb, a_aligned=True, b_aligned=True, env=None):
    """Launchers::matmul and matmul_one restated.  a_aligned, b_aligned: the pointer is 16-byte aligned (else it is one
    element in).  Returns route, the flags vec / bvec / bpack / braw, ks, kchunk, kchunks (launches of the matrix-core
    product kernel), stage, and terms: the most one thread accumulates in one launch"""
    env = env or env_of()
    al_a = a_aligned or not t.one_in_unaligned
    al_b = b_aligned or not t.one_in_unaligned
    ok = lambda ld: ld % t.ld_unit == 0
    p = SimpleNamespace(route=None, vec=0, bvec=0, bpack=0, braw=0, ks=1, kchunk=0, kchunks=0, stage=0, terms=K, unr=0)
    # api.hip matmul_one: the scratch of the call
    prime = not t.binary
    want = mfma_plane_bytes(env, 8 if t.eb <= 8 else 16, M, K, N) if prime else 0
    if want:
        want += SCRATCH_BYTES
    if want > SCRATCH_MAX:
        want = 0
    planes = want != 0
    if not want and K >= SCRATCH_MIN_K and cdiv(M, 32) * cdiv(N, 32) < SCRATCH_TILES:
        want = SCRATCH_BYTES
    ws = want                                                       # (grow-only: at least this; no plan below is bound by more)
    # mm_skinny_n
    if t.epw == 1 and N <= t.skinny_n_max and M >= SKINNY_N_MIN_M and K >= 1:
        if t.col_mac and N >= 2 and K > SHORT_ROWS_MAX_K:           # go_matvec_col
            p.vec = int(al_a and ok(lda))
            p.bvec = int(al_b and ok(ldb) and N % t.pack == 0)
            if p.vec and ldb == N and b_aligned and K >= SUB_COL_MIN_K:
                lw = 16 if cdiv(M, 16) >= 2 * env.num_cu else 64
                p.route = 'sub_col%d' % lw
                p.bvec = 0
                keven, terms = K & ~1, 0
                for kt0 in range(0, keven, MATVEC_SUB_KT):
                    terms += 2 * cdiv(min(keven - kt0, MATVEC_SUB_KT) // 2, lw)
                p.terms = terms + (K & 1)
            else:
                p.route = 'rows_col'
                p.terms = _stream_terms(K, t.pack, p.vec)
            return p
        if K <= SHORT_ROWS_MAX_K and M >= SHORT_ROWS_MIN_M:         # go_matvec
            p.route = 'short_rows'
            return p
        p.vec = int(al_a and ok(lda))
        p.bvec = int(al_b and ok(ldb) and N % t.pack == 0 and t.eb != 12)
        if N <= 2 and p.vec and K >= ROWS_R_MIN_K and M >= ROWS_R_MIN_M:
            p.route = 'rows_r'
            p.bpack = int(N == 1 and ldb == 1 and al_b)
            p.bvec = 0
        else:
            p.route = 'rows'
        p.terms = _stream_terms(K, t.pack, p.vec)
        return p
    # mm_skinny_m
    if t.epw == 1 and M <= SKINNY_MAX and N >= SKINNY_M_MIN_N and K >= 1 and ws:
        cpt, target = (1, env.num_cu * vecmat_col_per_cu(M)) if t.col_mac else (t.pack, VECMAT_TARGET)
        cols_blocks = cdiv(N // cpt, BLOCK)
        ks = max(1, min(cdiv(target, cols_blocks), (K + VECMAT_MIN_CHUNK - 1) // VECMAT_MIN_CHUNK))
        while ks > 1 and ks * M * N * t.wb > ws:
            ks //= 2                                                # (never taken: see scratch_halving_unreachable)
        if ks * M * N * t.wb <= ws:
            p.kchunk = cdiv(K, ks)
            p.ks = cdiv(K, p.kchunk)
            p.terms = p.kchunk
            if t.col_mac:
                p.route, p.stage, p.unr = 'vecmat_col', 1, vecmat_col_unr(M)
            else:
                p.route, p.stage, p.unr = 'vecmat', int(M > 1), 4
                p.vec = int(t.eb != 12 and t.pack > 1 and al_b and ok(ldb) and N % t.pack == 0)
            return p
    # mm_mfma, mm_mfma_wide
    if t.epw == 1 and t.mfma and planes:
        Mp, Np, Kp = cdiv(M, 64) * 64, cdiv(N, 64) * 64, cdiv(K, 32) * 32
        if t.wb == 16:
            p.route = 'mfma_wide'
            p.kchunks = cdiv(Kp, LIMB_KCHUNK_WIDE)
            return p
        p.route = 'mfma_glds' if t.eb == 8 else 'mfma_l4'
        p.braw = int(t.eb == 8 and Mp // 64 <= BRAW_MAX_ROW_TILES and K % 32 == 0 and N % 64 == 0 and ldb % 2 == 0 and b_aligned)
        tiles, ks = (Np // 64) * (Mp // 64), 1
        if tiles <= MFMA_SPLIT_TILES and Kp >= MFMA_SPLIT_KP:
            ks = min(cdiv(env.num_cu, tiles), Kp // MFMA_SLAB)      # (the scratch bound never binds: at most 12.6 MB of slabs)
        if ks > 1 and Kp <= LIMB_KCHUNK:
            p.kchunk = cdiv(cdiv(Kp, ks), 32) * 32
            p.ks = cdiv(Kp, p.kchunk)
            p.kchunks = 1
        else:
            p.kchunks = cdiv(Kp, LIMB_KCHUNK)
        return p
    # mm_valu
    if t.epw > 1:
        p.route = 'valu_bytes'
        return p
    small_out = cdiv(M, 64) * cdiv(N, 32) < VALU_SMALL_TILES
    t42 = not (t.wb >= 16 or small_out)
    p.route = 'valu_4x2' if t42 else 'valu_2x2'
    tiles = cdiv(N, 32) * cdiv(M, 64 if t42 else 32)
    p.tiles = tiles
    if tiles < VALU_SPLIT_TILES and K >= VALU_SPLIT_MIN_K and ws:
        ks = min(cdiv(VALU_SPLIT_TARGET, tiles), K // 32)
        while ks > 1 and ks * M * N * t.eb > ws:
            ks //= 2                                                # (never taken: ks * tiles < 1536 tiles of at most 48 KiB)
        if ks > 1:
            p.kchunk = cdiv(cdiv(K, ks), VALU_BK) * VALU_BK
            p.ks = cdiv(K, p.kchunk)
            p.terms = p.kchunk
    return p


def scratch_halving_unreachable(t, num_cu=256):
    """the `while (... > ws_bytes) ks /= 2` loop of mm_skinny_m: the largest ks M N sizeof(W) any admissible call asks for,
    against the 64 MiB the call is granted.  ks <= ceil(target / cols_blocks) and N <= 256 cpt cols_blocks, so
    ks N <= (target + cols_blocks) 256 cpt; cols_blocks <= 256 because 32-column tiles stay below 2048"""
    worst = 0
    for M in range(1, SKINNY_MAX + 1):
        cpt, target = (1, num_cu * vecmat_col_per_cu(M)) if t.col_mac else (t.pack, VECMAT_TARGET)
        for cb in range(1, SCRATCH_TILES * 32 // (BLOCK * cpt) + 2):
            N = min(cb * BLOCK * cpt + cpt - 1, SCRATCH_TILES * 32 - 1)
            worst = max(worst, cdiv(target, cdiv(N // cpt, BLOCK)) * M * N * t.wb)
    return worst, SCRATCH_BYTES


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case:
    """one call.  route, flags: what plan() must say; min_terms / max_terms: bounds on plan().terms; edges: the names this
    case adds to Driver.seen once it has passed.  *_in: the view starts one element in.  ldc: default N + 3"""

    def __init__(self, label, M, K, N, route, lda=None, ldb=None, ldc=None, a_in=False, b_in=False, c_in=False, data='per',
                 edges=(), min_terms=None, max_terms=None, null_ab=False, **flags):
        self.label, self.M, self.K, self.N, self.route = label, M, K, N, route
        self.lda = K if lda is None else lda
        self.ldb = N if ldb is None else ldb
        self.ldc = N + 3 if ldc is None else ldc
        self.a_in, self.b_in, self.c_in, self.data = a_in, b_in, c_in, data
        self.edges, self.min_terms, self.max_terms, self.null_ab, self.flags = tuple(edges), min_terms, max_terms, null_ab, flags

    def plan(self, t, env):
        return plan(t, self.M, self.K, self.N, self.lda, self.ldb, not self.a_in, not self.b_in, env)

    def check_plan(self, t, env):
        p = self.plan(t, env)
        where = (self.label, self.M, self.K, self.N, self.lda, self.ldb, vars(p))
        assert p.route == self.route, where
        for name, v in self.flags.items():
            assert getattr(p, name) == v, (name, v) + where
        assert self.min_terms is None or p.terms >= self.min_terms, where
        assert self.max_terms is None or p.terms <= self.max_terms, where
        return p

    def macs(self):
        return self.M * self.K * self.N

    def __repr__(self):
        return 'Case(%s: %d x %d x %d, ld %d %d %d, in %d%d%d, %s)' % (self.label, self.M, self.K, self.N, self.lda, self.ldb,
                                                                        self.ldc, self.a_in, self.b_in, self.c_in, self.data)


def _both(case_args, **kw):
    """the same call on periodic data and on all q - 1"""
    label = case_args[0]
    return [Case(label + '/' + d, *case_args[1:], data=d, **kw) for d in ('per', 'max')]


def skinny_n_columns(t):
    return range(1, t.skinny_n_max + 1)


def cases_short_rows(t, env):
    """k_matvec_short_rows: K <= 32 and M >= 1024, any field with one element per word; its neighbours take other routes"""
    if t.epw > 1:
        return []
    out = []
    for N in skinny_n_columns(t):                                   # every N; ldb > N on the even ones
        out.append(Case('short_rows/N=%d' % N, SHORT_ROWS_MIN_M + 1, SHORT_ROWS_MAX_K, N, 'short_rows',
                        ldb=N + (N % 2 == 0), edges=('short_rows/N', 'short_rows/ldb>N') if N % 2 == 0 else ('short_rows/N',)))
    nmax = t.skinny_n_max
    for M in (SHORT_ROWS_MIN_M, SHORT_ROWS_MIN_M + 1, SHORT_ROWS_MIN_M + BLOCK - 1):
        for K in (1, SHORT_ROWS_MAX_K):
            out.append(Case('short_rows/M=%d,K=%d' % (M, K), M, K, nmax, 'short_rows', ldb=nmax + 2, lda=K + 1, a_in=True,
                            edges=('short_rows/M-edges', 'short_rows/K=1' if K == 1 else 'short_rows/K=32')))
    out.append(Case('short_rows/M-1', SHORT_ROWS_MIN_M - 1, SHORT_ROWS_MAX_K, nmax, 'rows', edges=('short_rows/M=1023:other',)))
    out.append(Case('short_rows/K+1', SHORT_ROWS_MIN_M, SHORT_ROWS_MAX_K + 1, 2, 'rows_col' if t.col_mac else 'rows',
                    edges=('short_rows/K=33:other',)))
    out.append(Case('short_rows/max', SHORT_ROWS_MIN_M + 1, SHORT_ROWS_MAX_K, nmax, 'short_rows', data='max',
                    edges=('short_rows/max',)))
    return out


def rows_r_columns(t):
    return (1,) if t.col_mac else (1, 2)


def cases_rows_r(t, env):
    """k_matvec_rows_r<F, NN, 2>: N <= 2 (column-sum fields: N = 1), A in packs, K >= 1024, M >= 2048"""
    if t.epw > 1:
        return []
    out = []
    M0, K0 = ROWS_R_MIN_M, ROWS_R_MIN_K
    ks = [ld_up(t, K0), ld_up(t, K0) + 1, ld_up(t, K0) + t.pack + 1]
    for N in rows_r_columns(t):
        for i, K in enumerate(ks):
            M = (M0, M0 + 1)[i % 2]                                 # an odd M: the second row of the last workgroup is past M
            out.append(Case('rows_r/N=%d,K=%d' % (N, K), M, K, N, 'rows_r', lda=ld_up(t, K), bpack=int(N == 1),
                            edges=('rows_r/N=%d' % N, 'rows_r/K-edges', 'rows_r/odd-M' if M % 2 else 'rows_r/even-M',
                                   'rows_r/bpack' if N == 1 else 'rows_r/bpack-off:N=2')))
        out.append(Case('rows_r/M-1,N=%d' % N, M0 - 1, ks[0], N, 'rows', lda=ks[0], vec=1, edges=('rows_r/M=2047:other',)))
        out.append(Case('rows_r/K-1,N=%d' % N, M0, K0 - 1, N, 'rows', lda=ld_up(t, K0 - 1), vec=1, edges=('rows_r/K=1023:other',)))
    out.append(Case('rows_r/ldb=3', M0 + 1, ks[1], 1, 'rows_r', lda=ld_up(t, ks[1]), ldb=3, bpack=0, edges=('rows_r/bpack-off:ldb',)))
    if t.one_in_unaligned:
        out.append(Case('rows_r/B-in', M0 + 1, ks[2], 1, 'rows_r', lda=ld_up(t, ks[2]), b_in=True, bpack=0,
                        edges=('rows_r/bpack-off:B-in',)))
    if t.lazy and t.pack == 1:                                      # UN = 4: packs in fours, 4 x 256 per round of the workgroup
        for d in (-1, 0, 1):                                        # (one round less one is K = 1023, below ROWS_R_MIN_K: two rounds)
            K = 2 * 4 * BLOCK + d
            out.append(Case('rows_r/4pack%+d' % d, M0 + 1, K, 1, 'rows_r', lda=ld_up(t, K), bpack=1, edges=('rows_r/4-pack',)))
    return out


def flush_k(t):
    """a row of K elements walked by 256 threads in packs: every thread flushes (FLUSH terms), accumulates one more pack,
    and thread 0 takes the odd element behind the packs"""
    return BLOCK * (t.flush + t.pack) + 1


def cases_rows_r_flush(t, env):
    if t.epw > 1:
        return []
    K = ld_up(t, flush_k(t)) + 1
    return _both(('rows_r/flush', ROWS_R_MIN_M + 1, K, 1, 'rows_r'), lda=ld_up(t, K), bpack=1, min_terms=t.flush + t.pack + 1,
                 edges=('rows_r/flush',))


def cases_rows(t, env):
    """k_matvec_rows<F, NN>: what is left of matrix x few columns (column-sum fields: N = 1)"""
    if t.epw > 1:
        return []
    out = []
    M = SKINNY_N_MIN_M + 3
    K0 = 2 * BLOCK * t.pack                                         # two packs per thread, no scalar tail
    ns = (1,) if t.col_mac else tuple(skinny_n_columns(t))
    for N in ns:
        for tail in (0, 1):
            K = K0 + tail
            bvec = int(N % t.pack == 0 and t.eb != 12)
            out.append(Case('rows/N=%d,K=%d' % (N, K), M, K, N, 'rows', lda=ld_up(t, K), ldb=ld_up(t, N) if bvec else N, vec=1, bvec=bvec,
                            edges=('rows/vec', 'rows/N', 'rows/tail' if tail else 'rows/no-tail',
                                   'rows/bvec' if bvec else 'rows/bvec-off:N' if t.eb != 12 else 'rows/12-byte')))
    N = ns[-1]
    out.append(Case('rows/M-1', SKINNY_N_MIN_M - 1, K0, N, None, edges=('rows/M=63:other',)))
    if t.ld_unit > 1:
        out.append(Case('rows/odd-lda', M, K0 + 1, N, 'rows', lda=ld_bad(t, K0 + 1), vec=0, edges=('rows/vec-off:lda',)))
        out.append(Case('rows/odd-ldb', M, K0 + 1, N, 'rows', lda=ld_up(t, K0 + 1), ldb=ld_bad(t, N), vec=1, bvec=0,
                        edges=('rows/bvec-off:ldb',)))
    if t.one_in_unaligned:
        out.append(Case('rows/A-in', M, K0 + 1, N, 'rows', lda=ld_up(t, K0 + 1), a_in=True, vec=0, edges=('rows/vec-off:A-in',)))
        out.append(Case('rows/B-in', M, K0 + 1, N, 'rows', lda=ld_up(t, K0 + 1), b_in=True, vec=1, bvec=0, edges=('rows/bvec-off:B-in',)))
    return out


def cases_rows_flush(t, env):
    if t.epw > 1:
        return []
    K = ld_up(t, flush_k(t)) + 1
    N = 1 if t.col_mac else t.skinny_n_max
    out = _both(('rows/flush', SKINNY_N_MIN_M + 1, K, N, 'rows'), lda=ld_up(t, K), vec=1, min_terms=t.flush + t.pack + 1,
                edges=('rows/flush',))
    if t.one_in_unaligned:                                          # the scalar loop: `++cnt >= FLUSH`
        K = BLOCK * (t.flush + 1) + 1
        out += _both(('rows/flush-scalar', SKINNY_N_MIN_M + 1, K, N, 'rows'), a_in=True, vec=0, min_terms=t.flush + 2,
                     edges=('rows/flush-scalar',))
    return out


SUB_COL_KS = (SUB_COL_MIN_K, SUB_COL_MIN_K + 1, MATVEC_SUB_KT - 1, MATVEC_SUB_KT, MATVEC_SUB_KT + 1, 2 * MATVEC_SUB_KT + 2)


def sub_col16_min_m(env):
    """(M + 15) / 16 >= 2 num_cu"""
    return 16 * 2 * env.num_cu - 15


def cases_sub_col(t, env, lw):
    """k_matvec_sub_col<F, NN, LW>: column-sum fields, 2 <= N <= 8, A in packs, B contiguous and aligned, K >= 64"""
    if not t.col_mac:
        return []
    m16 = sub_col16_min_m(env)
    ms = (m16, m16 + 1, m16 + 17) if lw == 16 else (SKINNY_N_MIN_M, SKINNY_N_MIN_M + 1, SKINNY_N_MIN_M + 3)
    route = 'sub_col%d' % lw
    out = []
    for N in range(2, SKINNY_MAX + 1):
        for i, K in enumerate(SUB_COL_KS):
            M = ms[(i + N) % 3]
            out.append(Case('%s/N=%d,K=%d' % (route, N, K), M, K, N, route, lda=ld_up(t, K), ldc=N + 1 + i % 2, vec=1,
                            edges=(route + '/N', route + '/K-edges', route + '/M-edges', route + '/ldc>N')))
    if lw == 16:
        out.append(Case('sub_col16/M-1', m16 - 1, SUB_COL_KS[1], 3, 'sub_col64', edges=('sub_col16/M-1:sub_col64',), lda=ld_up(t, SUB_COL_KS[1])))
    return out


def cases_sub_col_flush(t, env, lw):
    """a lane takes K / lw terms, two at a time: past lw x 192 every lane has flushed; three more steps, then the odd last
    column on top of a count that the flush left odd (the SKINNY_FLUSH + 2 bound of the kernel's static_assert)"""
    if not t.col_mac:
        return []
    M = sub_col16_min_m(env) if lw == 16 else SKINNY_N_MIN_M + 1
    K = 2 * lw * SKINNY_FLUSH + 2 * lw * 3 + 1
    route = 'sub_col%d' % lw
    out = []
    for N in (3, 8):
        out += _both((route + '/flush,N=%d' % N, M, K, N, route), lda=ld_up(t, K), min_terms=2 * SKINNY_FLUSH + 7, edges=(route + '/flush',))
    return out


def cases_rows_col(t, env):
    """k_matvec_rows_col<F, NN, R>: column-sum fields leave sub_col one condition at a time"""
    if not t.col_mac:
        return []
    out = []
    M = SKINNY_N_MIN_M + 3                                          # odd: two rows per workgroup up to N = 4, the last one alone
    Kc = 2 * BLOCK * t.pack + 1
    for N in range(2, SKINNY_MAX + 1):
        even = N % 2 == 0
        for K in (SHORT_ROWS_MAX_K + 1, SUB_COL_MIN_K - 1):         # short K: everything else as sub_col wants it
            out.append(Case('rows_col/N=%d,K=%d' % (N, K), M, K, N, 'rows_col', lda=ld_up(t, K), vec=1, bvec=int(even),
                            edges=('rows_col/N', 'rows_col/K<64', 'rows_col/vec', 'rows_col/bvec' if even else 'rows_col/bvec-off:N')))
        out.append(Case('rows_col/ldb+1,N=%d' % N, M, Kc, N, 'rows_col', lda=ld_up(t, Kc), ldb=N + 1, vec=1, bvec=0,
                        edges=('rows_col/ldb=N+1',)))
        out.append(Case('rows_col/ldb+2,N=%d' % N, M, Kc, N, 'rows_col', lda=ld_up(t, Kc), ldb=N + 2, vec=1, bvec=int(even),
                        edges=('rows_col/ldb=N+2', 'rows_col/odd-M')))
        out.append(Case('rows_col/B-in,N=%d' % N, M, Kc, N, 'rows_col', lda=ld_up(t, Kc), b_in=True, vec=1, bvec=0,
                        edges=('rows_col/B-in',)))
        out.append(Case('rows_col/A-in,N=%d' % N, M + 1, Kc, N, 'rows_col', lda=ld_up(t, Kc), a_in=True, vec=0, bvec=int(even),
                        edges=('rows_col/A-in',)))
    return out


def cases_rows_col_flush(t, env):
    if not t.col_mac:
        return []
    K = BLOCK * (SKINNY_FLUSH + t.pack) + 1
    out = []
    for N in (2, 5):
        out += _both(('rows_col/flush,N=%d' % N, SKINNY_N_MIN_M + 1, K, N, 'rows_col'), lda=ld_up(t, K), ldb=N + 2, vec=1,
                     min_terms=SKINNY_FLUSH + t.pack + 1, edges=('rows_col/flush',))
    return out


def vecmat_ks0(t, env, M, N):
    cpt, target = (1, env.num_cu * vecmat_col_per_cu(M)) if t.col_mac else (t.pack, VECMAT_TARGET)
    return cdiv(target, cdiv(N // cpt, BLOCK))


def vecmat_k(t, env, M, N, kchunk, ragged=True):
    """the K at which mm_skinny_m cuts chunks of `kchunk` rows (>= 8), the last one a row short if ragged"""
    assert kchunk >= VECMAT_MIN_CHUNK
    ks0 = vecmat_ks0(t, env, M, N)
    K = kchunk * ks0 - (1 if ragged and ks0 > 1 else 0)
    if K < SCRATCH_MIN_K:                                           # (a device of very few CUs: whole chunks)
        K = kchunk * ks0
    assert K >= SCRATCH_MIN_K, (M, N, kchunk, ks0)
    return K


def vecmat_final_shape(t, env, M, ks):
    """(N, K) of a small B at which M rows of A are cut into exactly ks chunks, or None.  From ks = 8 on the bound of 8 rows
    per chunk does it at N = 64; below, the target itself must be that small: ceil(target / cols_blocks) <= ks, with
    K >= 64 (the scratch) and N < 65536 (fewer than 2048 tiles of 32 columns)"""
    if ks >= SCRATCH_MIN_K // VECMAT_MIN_CHUNK:
        N, K = SKINNY_M_MIN_N, VECMAT_MIN_CHUNK * ks
        return (N, K) if plan(t, M, K, N, K, N, env=env).ks == ks else None
    cpt, target = (1, env.num_cu * vecmat_col_per_cu(M)) if t.col_mac else (t.pack, VECMAT_TARGET)
    for cb in range(cdiv(target, max(ks, 1)), SCRATCH_TILES * 32 // (BLOCK * cpt) + 1):
        N = max(SKINNY_M_MIN_N, (cb - 1) * BLOCK * cpt + cpt)
        if N >= SCRATCH_TILES * 32:
            break
        for K in range(SCRATCH_MIN_K, SCRATCH_MIN_K + 2 * VECMAT_MIN_CHUNK * max(ks, 1)):
            if plan(t, M, K, N, K, N, env=env).ks == ks:
                return N, K
    return None


VECMAT_FINAL_KS = (1, 7, 8, 9, 39, 40, 41)
VECMAT_NS = (SKINNY_M_MIN_N, BLOCK - 1, BLOCK, BLOCK + 1)


def cases_vecmat_col(t, env):
    """k_vecmat_partial_col<F, MM, UNR, MINB> + k_vecmat_final: column-sum fields, M <= 8, N >= 64, K >= 64"""
    if not t.col_mac:
        return []
    out = []
    for M in range(1, SKINNY_MAX + 1):
        unr = vecmat_col_unr(M)
        # (a chunk is at least 8 rows: below UNR only where UNR = 16, and never equal to UNR = 4)
        chunks = sorted({VECMAT_MIN_CHUNK, max(unr, VECMAT_MIN_CHUNK), 2 * unr + 1})
        for i, kc in enumerate(chunks):
            N = VECMAT_NS[(i + M) % 4]
            K = vecmat_k(t, env, M, N, kc)
            e = 'vecmat_col/kchunk<UNR' if kc < unr else 'vecmat_col/kchunk=UNR' if kc == unr else \
                'vecmat_col/kchunk=2UNR+1' if kc == 2 * unr + 1 else 'vecmat_col/kchunk=2UNR'
            out.append(Case('vecmat_col/M=%d,kc=%d' % (M, kc), M, K, N, 'vecmat_col', kchunk=kc, lda=K + M % 2, ldb=N + (i % 2) * 3,
                            b_in=(i == 2), edges=('vecmat_col/M', 'vecmat_col/N-edges', e, 'vecmat_col/ragged-K') +
                            (('vecmat_col/ldb>N',) if i % 2 else ()) + (('vecmat_col/B-in',) if i == 2 else ())))
    return out


def cases_vecmat_col_tiles(t, env):
    """the second staged tile (128 and 129 rows of a chunk) at N = 257, where the dead lanes of the second workgroup pass the
    barriers; the flush (192 + UNR rows and more)"""
    if not t.col_mac:
        return []
    out = []
    N = BLOCK + 1
    for M in (1, 5, 8):
        unr = vecmat_col_unr(M)
        for kc in (VECMAT_COL_KT, VECMAT_COL_KT + 1):
            out.append(Case('vecmat_col/M=%d,kc=%d' % (M, kc), M, vecmat_k(t, env, M, N, kc), N, 'vecmat_col', kchunk=kc,
                            edges=('vecmat_col/tile=%d' % kc,)))
        kc = SKINNY_FLUSH + unr + 3
        out += _both(('vecmat_col/flush,M=%d' % M, M, vecmat_k(t, env, M, N, kc), N, 'vecmat_col'), kchunk=kc,
                     min_terms=SKINNY_FLUSH + unr, edges=('vecmat_col/flush',))
    return out


def cases_vecmat(t, env):
    """k_vecmat_partial<F, MM, VEC, STAGE>: every other field with one element per word, M <= 8, N >= 64, K >= 64"""
    if t.epw > 1 or t.col_mac:
        return []
    out = []
    can_vec = t.eb != 12 and t.pack > 1
    for M in range(1, SKINNY_MAX + 1):
        for i, kc in enumerate((VECMAT_MIN_CHUNK + 1, VECMAT_KT, VECMAT_KT + 1)):
            N = (BLOCK * t.pack, SKINNY_M_MIN_N + t.pack, BLOCK * t.pack + 1)[(i + M) % 3]     # the last: N % pack != 0
            vec = int(can_vec and N % t.pack == 0)
            K = vecmat_k(t, env, M, N, kc)
            e = ('vecmat/VEC',) if vec else ('vecmat/VEC-off:N',) if can_vec else ('vecmat/VEC-off:field',)
            out.append(Case('vecmat/M=%d,kc=%d' % (M, kc), M, K, N, 'vecmat', kchunk=kc, vec=vec, stage=int(M > 1), lda=K + M % 2,
                            edges=e + ('vecmat/M', 'vecmat/STAGE' if M > 1 else 'vecmat/no-STAGE', 'vecmat/kchunk=%d' % kc)))
    if can_vec and t.one_in_unaligned:
        N = BLOCK * t.pack
        out.append(Case('vecmat/B-in', 3, vecmat_k(t, env, 3, N, VECMAT_KT + 1), N, 'vecmat', b_in=True, vec=0, edges=('vecmat/VEC-off:B-in',)))
    return out


def cases_vecmat_flush(t, env):
    if t.epw > 1 or t.col_mac:
        return []
    out = []
    N = SKINNY_M_MIN_N + t.pack
    for M in (1, 3, 6):                                             # unstaged; the 4- and the 8-row instantiation with mi < M
        for kc in (t.flush, t.flush + 1):
            out += _both(('vecmat/flush,M=%d,kc=%d' % (M, kc), M, vecmat_k(t, env, M, N, kc), N, 'vecmat'), kchunk=kc, stage=int(M > 1),
                         min_terms=t.flush, edges=('vecmat/flush' if kc == t.flush else 'vecmat/flush+1',))
    return out


def cases_vecmat_final(t, env):
    """k_vecmat_final with ks partial rows: eight groups, the four-deep loop and its tail"""
    if t.epw > 1:
        return []
    out = []
    for ks in VECMAT_FINAL_KS:
        shape = vecmat_final_shape(t, env, 3, ks)
        if shape is None:
            continue                                                # (final_ks_unreachable says which, the tests assert that list)
        N, K = shape
        out.append(Case('vecmat_final/ks=%d' % ks, 3, K, N, 'vecmat_col' if t.col_mac else 'vecmat', ks=ks, edges=('vecmat_final/ks=%d' % ks,)))
    return out


def final_ks_unreachable(t, env):
    return () if t.epw > 1 else tuple(ks for ks in VECMAT_FINAL_KS if vecmat_final_shape(t, env, 3, ks) is None)


def mfma_route(t):
    return {4: 'mfma_l4', 8: 'mfma_glds', 12: 'mfma_wide', 16: 'mfma_wide'}[t.mfma]


def valu_route(t, M, N):
    if t.epw > 1:
        return 'valu_bytes'
    return 'valu_2x2' if t.wb >= 16 or cdiv(M, 64) * cdiv(N, 32) < VALU_SMALL_TILES else 'valu_4x2'


def cases_mfma(t, env):
    """the int8 matrix-core products of the prime fields up to 128 bits and the decision that leads to them"""
    if not t.mfma or not env.mfma_on:
        return []
    out = []
    r = mfma_route(t)
    S = 256
    kmin = max(MFMA_MIN_K, cdiv(int(env.mfma_min), S * S))          # M N K on both sides of mfma_min
    if kmin > MFMA_MIN_K:
        out.append(Case('mfma/MNK>=min', S, kmin, S, r, edges=('mfma/MNK>=min',)))
        out.append(Case('mfma/MNK<min', S, kmin - 1, S, valu_route(t, S, S), edges=('mfma/MNK<min',)))
    big = cdiv(int(env.mfma_min), 9 * MFMA_MIN_K)                    # 9 x 64 x big >= mfma_min
    out.append(Case('mfma/M=9', 9, MFMA_MIN_K, big, r, edges=('mfma/M=9', 'mfma/K=64')))
    out.append(Case('mfma/N=9', big, MFMA_MIN_K, 9, r, lda=MFMA_MIN_K + 1, edges=('mfma/N=9',)))
    out.append(Case('mfma/N=8', max(big, SKINNY_N_MIN_M), MFMA_MIN_K, 8 if t.skinny_n_max == 8 else 4, None, edges=('mfma/N=8:skinny',)))
    out.append(Case('mfma/M=8', 8, MFMA_MIN_K, max(big, SKINNY_M_MIN_N), 'vecmat_col' if t.col_mac else 'vecmat', edges=('mfma/M=8:skinny',)))
    out.append(Case('mfma/K=63', 9, MFMA_MIN_K - 1, cdiv(int(env.mfma_min), 9 * (MFMA_MIN_K - 1)) + 1, valu_route(t, 9, big), edges=('mfma/K=63:valu',)))
    # ragged everything, more than one chunk of K
    kc = LIMB_KCHUNK_WIDE if t.wb == 16 else LIMB_KCHUNK
    m = 70
    while m * m * (kc + 33) < env.mfma_min:
        m += 64
    out.append(Case('mfma/chunks', m, kc + 33, m + 3, r, kchunks=2, lda=kc + 34, ldb=m + 4, a_in=True, b_in=True, c_in=True,
                    edges=('mfma/K-chunks', 'mfma/ragged')))
    out.append(Case('mfma/max', 65, 2 * S + 1, max(SKINNY_MAX + 1, cdiv(int(env.mfma_min), 65 * (2 * S + 1)) + 1), r, data='max', edges=('mfma/max',)))
    if t.wb <= 8:
        # split-K slabs: 128 against 129 tiles, Kp 480 against 512
        N128 = MFMA_SPLIT_TILES * 64
        out.append(Case('mfma/tiles=128', 64, MFMA_SPLIT_KP, N128, r, ks=min(cdiv(env.num_cu, 128), 2), edges=('mfma/split:128-tiles',)))
        out.append(Case('mfma/tiles=129', 64, MFMA_SPLIT_KP, N128 + 1, r, ks=1, edges=('mfma/no-split:129-tiles',)))
        n = cdiv(cdiv(int(env.mfma_min), 64 * (MFMA_SPLIT_KP - 32)), 64) * 64
        out.append(Case('mfma/Kp=480', 64, MFMA_SPLIT_KP - 32, n, r, ks=1, edges=('mfma/no-split:Kp=480',)))
        out.append(Case('mfma/Kp=512', 64, MFMA_SPLIT_KP - 31, n, r, ks=2, ldb=n + 1, edges=('mfma/split:Kp=512',)))
        out.append(Case('mfma/short-slab', 70, 5 * MFMA_SLAB + 40, 200, r, ks=min(cdiv(env.num_cu, 8), 5), edges=('mfma/split:ragged',)))
    if t.eb == 8:
        # the product kernel converts B itself (braw): one condition at a time
        Kb = 256
        Nb = cdiv(cdiv(int(env.mfma_min), 128 * Kb), 64) * 64
        out.append(Case('mfma/braw', 128, Kb, Nb, r, braw=1, edges=('mfma/braw',)))
        out.append(Case('mfma/braw,ldb', 128, Kb, Nb, r, braw=1, ldb=Nb + 2, edges=('mfma/braw:ldb-even',)))
        out.append(Case('mfma/braw-off:M', 129, Kb, Nb, r, braw=0, edges=('mfma/braw-off:M=129',)))
        out.append(Case('mfma/braw-off:K', 128, Kb + 1, Nb, r, braw=0, lda=Kb + 2, edges=('mfma/braw-off:K%32',)))
        out.append(Case('mfma/braw-off:N', 128, Kb, Nb + 1, r, braw=0, ldb=Nb + 2, edges=('mfma/braw-off:N%64',)))
        out.append(Case('mfma/braw-off:ldb', 128, Kb, Nb, r, braw=0, ldb=Nb + 1, edges=('mfma/braw-off:ldb-odd',)))
        out.append(Case('mfma/braw-off:B-in', 128, Kb, Nb, r, braw=0, ldb=Nb + 2, b_in=True, edges=('mfma/braw-off:B-in',)))
        out.append(Case('mfma/braw,split', 128, 4 * MFMA_SLAB, 512, r, braw=1, edges=('mfma/braw:split',), data='max'))
    return out


def cases_valu(t, env):
    """k_matmul<F, 4, 2> / <F, 2, 2> (+ k_splitk_sum) and k_matmul_bytes: what no other route takes"""
    out = []
    if t.epw > 1:
        for M, K, N in ((33, 70, 45), (1, 1, 1), (64, 33, 64), (65, 300, 31)):
            out.append(Case('valu_bytes/%dx%dx%d' % (M, K, N), M, K, N, 'valu_bytes', lda=K + 3, ldb=N + 5, a_in=M % 2 == 1, b_in=N % 2 == 1,
                            c_in=K % 2 == 1, edges=('valu_bytes',)))
        out.append(Case('valu_bytes/max', 40, 777, 35, 'valu_bytes', data='max', edges=('valu_bytes/max',)))
        return out
    Ks = VALU_SPLIT_MIN_K - 1
    if t.wb < 16:
        # 63 against 64 tiles of 64 x 32 (K below 64: no split, below the matrix cores)
        out.append(Case('valu/tiles=63', 7 * 64, Ks, 9 * 32, 'valu_2x2', ks=1, edges=('valu/2x2:63-tiles',)))
        out.append(Case('valu/tiles=64', 8 * 64, Ks, 8 * 32, 'valu_4x2', ks=1, edges=('valu/4x2:64-tiles',)))
        out.append(Case('valu/4x2,ragged', 8 * 64 + 1, 17, 8 * 32 - 1, 'valu_4x2', ks=1, lda=18, a_in=True, b_in=True, edges=('valu/4x2:ragged',)))
    out.append(Case('valu/2x2,ragged', 33, 17, 45, 'valu_2x2', ks=1, lda=18, ldb=46, a_in=True, b_in=True, c_in=True, edges=('valu/2x2:ragged',)))
    # the split: K 63 against 64, a short last slab
    out.append(Case('valu/K=63', 40, Ks, 45, 'valu_2x2', ks=1, edges=('valu/no-split:K=63',)))
    out.append(Case('valu/K=64', 40, Ks + 1, 45, 'valu_2x2', ks=2, kchunk=32, edges=('valu/split:K=64',)))
    out.append(Case('valu/short-slab', 40, 5 * 48 + 7, 45, 'valu_2x2', edges=('valu/split:short-slab',), ks=6, kchunk=48))
    if not t.mfma:
        # 511 against 512 tiles at K = 64 (fields with matrix-core products take those from 1.6e7 multiply-adds on)
        bm = 64 if t.wb < 16 else 32
        r = 'valu_4x2' if t.wb < 16 else 'valu_2x2'
        out.append(Case('valu/tiles=511', 7 * bm, VALU_SPLIT_MIN_K, 73 * 32, r, ks=2, edges=('valu/split:511-tiles',)))
        out.append(Case('valu/tiles=512', 8 * bm, VALU_SPLIT_MIN_K, 64 * 32, r, ks=1, edges=('valu/no-split:512-tiles',)))
    return out


def cases_valu_flush(t, env):
    """M <= 8 and N = 63: no skinny route, no matrix cores; two tiles, so K is cut into ks slabs -- each past FLUSH terms"""
    if t.epw > 1:
        return []
    M, N = 5, SKINNY_M_MIN_N - 1
    ks = cdiv(VALU_SPLIT_TARGET, 2)
    slab = cdiv(t.flush + VALU_BK + 1, VALU_BK) * VALU_BK
    K = ks * slab - 3
    return _both(('valu/flush', M, K, N, 'valu_2x2'), ks=ks, kchunk=slab, min_terms=t.flush + VALU_BK, edges=('valu/flush',))


def cases_degenerate(t, env):
    """K == 0: zeros in C's block, the pads untouched, NULL A and B -- on a shape of every route family"""
    shapes = [('short_rows', SHORT_ROWS_MIN_M, 1), ('rows', SKINNY_N_MIN_M + 1, 2), ('vecmat', 3, BLOCK + 1), ('mfma', 300, 300),
              ('valu', 33, 45), ('one', 1, 1)]
    return [Case('K=0/' + name, M, 0, N, 'valu_bytes' if t.epw > 1 else valu_route(t, M, N), lda=0, ldb=N, null_ab=True,
                 edges=('K=0/' + name,)) for name, M, N in shapes]


FAMILIES = {
    'short_rows': cases_short_rows, 'rows_r': cases_rows_r, 'rows': cases_rows, 'sub_col16': lambda t, e: cases_sub_col(t, e, 16),
    'sub_col64': lambda t, e: cases_sub_col(t, e, 64), 'rows_col': cases_rows_col, 'vecmat_col': cases_vecmat_col,
    'vecmat_col_tiles': cases_vecmat_col_tiles, 'vecmat': cases_vecmat, 'vecmat_final': cases_vecmat_final, 'mfma': cases_mfma,
    'valu': cases_valu, 'degenerate': cases_degenerate,
}
FLUSH_FAMILIES = {
    'rows_r_flush': cases_rows_r_flush, 'rows_flush': cases_rows_flush, 'sub_col16_flush': lambda t, e: cases_sub_col_flush(t, e, 16),
    'sub_col64_flush': lambda t, e: cases_sub_col_flush(t, e, 64), 'rows_col_flush': cases_rows_col_flush,
    'vecmat_flush': cases_vecmat_flush, 'valu_flush': cases_valu_flush,
}


def resolve(t, env, cases):
    """cases whose route is None take the one the plan gives -- they are the 'goes elsewhere' neighbours, which assert only
    that it is NOT the family's own route (the generator says which in the edge name)"""
    for c in cases:
        if c.route is None:
            c.route = c.plan(t, env).route
    return cases


def family(name, modulus, binary, env):
    t = traits(modulus, binary)
    gen = FAMILIES.get(name) or FLUSH_FAMILIES[name]
    return resolve(t, env, gen(t, env))


# the edges the issue lists, per class of field; the closing test of tests/test_gpu_matmul_contract.py compares Driver.seen
def required_edges(t, env):
    """every edge name the generators of this field produce: what the closing test holds Driver.seen against"""
    out = set()
    for name in list(FAMILIES) + list(FLUSH_FAMILIES):
        for c in family(name, t.modulus, t.binary, env):
            out.update(c.edges)
            out.add(c.route)
    return out


# the edges that must exist on SOME field, typed out: a generator that stops producing one fails the host test
REQUIRED = {
    'short_rows/N', 'short_rows/ldb>N', 'short_rows/M-edges', 'short_rows/K=1', 'short_rows/K=32', 'short_rows/M=1023:other',
    'short_rows/K=33:other', 'short_rows/max',
    'rows_r/N=1', 'rows_r/N=2', 'rows_r/K-edges', 'rows_r/odd-M', 'rows_r/even-M', 'rows_r/bpack', 'rows_r/bpack-off:N=2',
    'rows_r/bpack-off:ldb', 'rows_r/bpack-off:B-in', 'rows_r/4-pack', 'rows_r/flush', 'rows_r/M=2047:other', 'rows_r/K=1023:other',
    'rows/vec', 'rows/N', 'rows/tail', 'rows/no-tail', 'rows/bvec', 'rows/bvec-off:N', 'rows/12-byte', 'rows/vec-off:lda',
    'rows/vec-off:A-in', 'rows/bvec-off:ldb', 'rows/bvec-off:B-in', 'rows/flush', 'rows/flush-scalar', 'rows/M=63:other',
    'sub_col16/N', 'sub_col16/K-edges', 'sub_col16/M-edges', 'sub_col16/ldc>N', 'sub_col16/flush', 'sub_col16/M-1:sub_col64',
    'sub_col64/N', 'sub_col64/K-edges', 'sub_col64/M-edges', 'sub_col64/ldc>N', 'sub_col64/flush',
    'rows_col/N', 'rows_col/K<64', 'rows_col/vec', 'rows_col/bvec', 'rows_col/bvec-off:N', 'rows_col/ldb=N+1', 'rows_col/ldb=N+2',
    'rows_col/odd-M', 'rows_col/B-in', 'rows_col/A-in', 'rows_col/flush',
    'vecmat_col/M', 'vecmat_col/N-edges', 'vecmat_col/kchunk<UNR', 'vecmat_col/kchunk=UNR', 'vecmat_col/kchunk=2UNR+1', 'vecmat_col/kchunk=2UNR',
    'vecmat_col/ragged-K', 'vecmat_col/ldb>N', 'vecmat_col/B-in', 'vecmat_col/tile=128', 'vecmat_col/tile=129', 'vecmat_col/flush',
    'vecmat/VEC', 'vecmat/VEC-off:N', 'vecmat/VEC-off:field', 'vecmat/VEC-off:B-in', 'vecmat/M', 'vecmat/STAGE', 'vecmat/no-STAGE',
    'vecmat/kchunk=9', 'vecmat/kchunk=32', 'vecmat/kchunk=33', 'vecmat/flush', 'vecmat/flush+1',
    'vecmat_final/ks=7', 'vecmat_final/ks=8', 'vecmat_final/ks=9', 'vecmat_final/ks=39', 'vecmat_final/ks=40', 'vecmat_final/ks=41',
    'mfma/MNK>=min', 'mfma/MNK<min', 'mfma/M=9', 'mfma/N=9', 'mfma/K=64', 'mfma/K=63:valu', 'mfma/M=8:skinny', 'mfma/N=8:skinny',
    'mfma/K-chunks', 'mfma/ragged', 'mfma/max', 'mfma/split:128-tiles', 'mfma/no-split:129-tiles', 'mfma/no-split:Kp=480',
    'mfma/split:Kp=512', 'mfma/split:ragged', 'mfma/braw', 'mfma/braw:ldb-even', 'mfma/braw-off:M=129', 'mfma/braw-off:K%32',
    'mfma/braw-off:N%64', 'mfma/braw-off:ldb-odd', 'mfma/braw-off:B-in', 'mfma/braw:split',
    'valu/2x2:63-tiles', 'valu/4x2:64-tiles', 'valu/4x2:ragged', 'valu/2x2:ragged', 'valu/no-split:K=63', 'valu/split:K=64',
    'valu/split:short-slab', 'valu/split:511-tiles', 'valu/no-split:512-tiles', 'valu/flush', 'valu_bytes', 'valu_bytes/max',
    'K=0/short_rows', 'K=0/rows', 'K=0/vecmat', 'K=0/mfma', 'K=0/valu', 'K=0/one',
    'refused/M=0', 'refused/N=0', 'refused/lda<K', 'refused/ldb<N', 'refused/ldc<N', 'refused/C=NULL',
} | set(ROUTES)


# ---- data and references -----------------------------------------------------------------------------------------------------
def _np_dtype(eb):
    return {1: np.uint8, 4: np.uint32, 8: np.uint64, 12: np.uint32, 16: np.uint64}[eb]


def edge_elems(t):
    """0, 1, q - 1, q - 2, q // 2 and, where they are elements, the representative switch of the digit split 0x7f...7f with
    its neighbours"""
    q = t.q
    sw = int.from_bytes(b'\x7f' * min(t.eb, 8), 'little')
    vals = [0, 1, q - 1, q - 2, q // 2] + [v for v in (sw - 1, sw, sw + 1, q - sw) if 0 <= v < q]
    return [v % q for v in vals]


def rand_bytes(t, rng, n):
    """n canonical elements as bytes: uniform up to 64 bits; wider, uniform k-bit values (k the bit length of q) with the
    top bit cleared wherever the top limb does not already show the value to be below q"""
    eb = t.eb
    if t.q < 1 << 64:
        return rng.integers(0, t.q, size=n, dtype=np.uint64, endpoint=False).astype({1: '<u1', 4: '<u4', 8: '<u8'}[eb]).view(np.uint8).copy()
    if t.q == 1 << 64:
        return rng.integers(0, 256, size=n * eb, dtype=np.uint8)
    bits = (t.q - 1).bit_length()
    raw = rng.integers(0, 256, size=(n, eb), dtype=np.uint8)
    top = (bits - 1) // 8                                           # the byte that holds the top bit
    raw[:, top + 1:] = 0
    raw[:, top] &= (1 << ((bits - 1) % 8 + 1)) - 1
    if not t.binary:
        lw = 4 if eb == 12 else 8                                   # compare the top limb with q's
        limb = raw[:, eb - lw:].copy().view('<u4' if lw == 4 else '<u8').reshape(n)
        clear = limb >= (t.q >> (8 * (eb - lw)))
        raw[clear, top] &= (1 << ((bits - 1) % 8)) - 1
    return raw.reshape(-1)


def ref_product(t, co, a, b, pa, K, pb):
    """(pa x K) @ (K x pb) from the byte images, as bytes.  Never the library: oracle/fforacle.c, or Python integers"""
    eb = t.eb
    if K == 0:
        return np.zeros(pa * pb * eb, dtype=np.uint8)
    if eb == 24:
        def obj(raw, r, c):
            v = np.empty(r * c, dtype=object)
            bts = raw.tobytes()
            v[:] = [int.from_bytes(bts[i:i + 24], 'little') for i in range(0, len(bts), 24)]
            return v.reshape(r, c)
        C = np.dot(obj(a, pa, K), obj(b, K, pb)) % t.q
        return ints_to_bytes([int(v) for v in C.reshape(-1)], 24)
    cf = _cfield(co, t.modulus, t.binary)
    dt = _np_dtype(eb)
    shape = lambda n: (n, 2) if eb == 16 else (n, 3) if eb == 12 else (n,)
    A = np.ascontiguousarray(a).view(dt).reshape(shape(pa * K))
    B = np.ascontiguousarray(b).view(dt).reshape(shape(K * pb))
    co.set_threads(co.max_threads())
    try:
        C = co.matmul(cf, A, B, pa, K, pb)
    finally:
        co.set_threads(1)
    return np.ascontiguousarray(C).view(np.uint8).reshape(-1).copy()


_cfields = {}


def _cfield(co, modulus, binary):
    if (modulus, binary) not in _cfields:
        _cfields[modulus, binary] = co.CField(modulus, binary)
    return _cfields[modulus, binary]


def max_expected(t, K):
    """every element q - 1: K (q - 1)^2 -- K mod q over a prime, by the parity of K over GF(2^n)"""
    if not t.binary:
        return K % t.q
    F = po.Field(t.modulus, True)
    e = t.q - 1
    return po.mul(F, e, e) if K & 1 else 0


_periods = {}


def period_data(t, co, K, kind):
    """(A period (pa, K eb), B period (K, pb eb), C period (pa, pb eb)) as uint8 arrays, cached per field, K and kind"""
    key = (t.modulus, t.binary, K, kind)
    if key in _periods:
        return _periods[key]
    eb = t.eb
    if kind == 'max':
        e = ints_to_bytes([t.q - 1], eb)
        a, b, pa, pb = np.tile(e, K).reshape(1, K * eb), np.tile(e, K).reshape(K, eb), 1, 1
        c = ints_to_bytes([max_expected(t, K)], eb).reshape(1, eb)
    else:
        rng = np.random.default_rng([t.modulus % (1 << 63), K, 17])
        pa, pb = (3, 3) if eb == 24 and K > 1 << 14 else (PA, PB)    # (Python integers: a shorter odd period on long rows)
        a = rand_bytes(t, rng, pa * K).reshape(pa, K * eb)
        b = rand_bytes(t, rng, K * pb).reshape(K, pb * eb)
        edges = edge_elems(t)
        for r in range(pa):                                         # edge values first (and last), rotated from row to row
            vals = (edges[r % len(edges):] + edges[:r % len(edges)])[:K]
            a[r, :len(vals) * eb] = ints_to_bytes(vals, eb)
            if K > 2 * len(edges):                                  # (the last term of a row is never zero)
                a[r, (K - len(vals)) * eb:] = ints_to_bytes(vals[:0:-1] + [t.q - 1 - r % (t.q - 1)], eb)
        for cidx in range(pb):
            vals = (edges[(2 * cidx + 1) % len(edges):] + edges[:(2 * cidx + 1) % len(edges)])[:K]
            for k, v in enumerate(vals):
                b[k, cidx * eb:(cidx + 1) * eb] = ints_to_bytes([v], eb)
        c = ref_product(t, co, a.reshape(-1), b.reshape(-1), pa, K, pb).reshape(pa, pb * eb)
    if len(_periods) > 64:
        _periods.clear()
    _periods[key] = (a, b, c)
    return _periods[key]


# ---- adapters ----------------------------------------------------------------------------------------------------------------
def api_status(K, M, N, lda, ldb, ldc, a, b, c):
    """the argument checks of ffgpu_matmul (api.hip): None when the call goes ahead"""
    if M == 0 or N == 0:
        return OK
    if c is None or ldc < N:
        return EINVAL
    if K and (a is None or b is None or lda < K or ldb < N):
        return EINVAL
    return None


class CpuAdapter:
    """an engine-style context on CPU tensors behind the signature of the C ABI: the argument checks of api.hip, operands
    read through their leading dimensions, the product by ctx.matmul, the result written through ldc"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.eb, self.device = torch, ctx, ctx.elem_bytes, torch.device('cpu')
        self.num_cu = None

    def _gather(self, buf, off, rows, ld, cols):
        eb, torch = self.eb, self.torch
        if rows == 0 or cols == 0:
            raw = torch.empty(0, dtype=torch.uint8)
        else:
            raw = torch.as_strided(buf, (rows, cols * eb), (ld * eb, 1), off).contiguous().reshape(-1)
        from mpyc_amd import engine
        t = raw.view(engine._torch_dtype(eb))
        limbs = engine.limbs_of(eb)
        return engine.DevArray(self.ctx, t.reshape(rows * cols, limbs) if limbs else t, rows * cols)

    def _scatter(self, buf, off, rows, ld, cols, arr):
        raw = arr.t.contiguous().view(self.torch.uint8).reshape(rows, cols * self.eb)
        self.torch.as_strided(buf, (rows, cols * self.eb), (ld * self.eb, 1), off).copy_(raw)

    def product(self, buf, a, lda, b, ldb, M, K, N):
        return self.ctx.matmul(self._gather(buf, a or 0, M if K else 0, lda, K), self._gather(buf, b or 0, K, ldb, N if K else 0), M, K, N)

    def matmul(self, buf, a, lda, b, ldb, c, ldc, M, K, N):
        rc = api_status(K, M, N, lda, ldb, ldc, a, b, c)
        if rc is not None:
            return rc
        self._scatter(buf, c, M, ldc, N, self.product(buf, a, lda, b, ldb, M, K, N))
        return OK

    def sync(self):
        pass


class GpuAdapter:
    """the C ABI itself on base pointer + byte offset"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.eb, self.device = torch, ctx, ctx.elem_bytes, ctx.torch_device
        self.num_cu = torch.cuda.get_device_properties(self.device).multi_processor_count

    def matmul(self, buf, a, lda, b, ldb, c, ldc, M, K, N):
        p = lambda off: None if off is None else buf.data_ptr() + off
        cx = self.ctx
        return cx._L.ffgpu_matmul(cx._h, p(a), lda, p(b), ldb, p(c), ldc, M, K, N, cx._stream())

    def sync(self):
        self.torch.cuda.synchronize(self.device)


# ---- the driver --------------------------------------------------------------------------------------------------------------
def _align16(x):
    return cdiv(x, 16) * 16


class Driver:
    def __init__(self, adapter, co, modulus, binary, env=None):
        self.ad, self.co, self.t = adapter, co, traits(int(modulus), bool(binary))
        assert adapter.eb == self.t.eb
        self.env = env or env_of(num_cu=adapter.num_cu or 256)
        self.cases = 0              # calls compared with the reference
        self.seen = set()           # routes and edges of the cases that passed
        self.max_bytes = 0          # the largest backing tensor

    # ---- buffers ----
    def _place(self, buf, off, rows, ld, cols, per):
        """rows x cols elements at byte offset off, leading dimension ld: element (i, j) is per[i % pr, j % pc]; per: a
        uint8 tensor (pr, pc, eb) on the device.  In slices of at most 256 MiB"""
        torch, eb = self.ad.torch, self.t.eb
        if rows == 0 or cols == 0:
            return
        pr, pc = per.shape[0], per.shape[1]
        if pc != cols:
            per = per[:, torch.arange(cols, device=per.device) % pc]
        flat = per.reshape(pr, cols * eb)
        step = max(pr, (1 << 28) // (cols * eb) // pr * pr)
        dst = torch.as_strided(buf, (rows, cols * eb), (ld * eb, 1), off)
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            dst[r0:r1].copy_(flat[torch.arange(r0, r1, device=per.device) % pr])

    def layout(self, case):
        """byte offsets of A, B, C and the size of the tensor: GUARD bytes of guard at least before, between and after"""
        eb = self.t.eb
        span = lambda rows, ld, cols: ((rows - 1) * ld + cols) * eb if rows and cols else 0
        sizes = {'A': span(case.M, case.lda, case.K), 'B': span(case.K, case.ldb, case.N), 'C': span(case.M, case.ldc, case.N)}
        off, cur = {}, 0
        for s, one_in in (('A', case.a_in), ('B', case.b_in), ('C', case.c_in)):
            off[s] = _align16(cur + GUARD) + (eb if one_in else 0)
            cur = off[s] + sizes[s]
        return off, sizes, _align16(cur + GUARD)

    def _noise(self):
        rng = np.random.default_rng([self.t.modulus % (1 << 63), 23])
        return self.ad.torch.from_numpy(rand_bytes(self.t, rng, NOISE)).to(self.ad.device)

    def _prepare(self, case):
        torch, eb, t = self.ad.torch, self.t.eb, self.t
        off, sizes, total = self.layout(case)
        self.max_bytes = max(self.max_bytes, total)
        buf = torch.full((total,), GUARD_BYTE, dtype=torch.uint8, device=self.ad.device)
        a, b, c = period_data(t, self.co, case.K, case.data)
        dev = lambda x, r, cc: torch.from_numpy(np.ascontiguousarray(x)).to(self.ad.device).reshape(r, cc, eb)
        if case.K:
            self._place(buf, off['A'], case.M, case.lda, case.K, dev(a, a.shape[0], case.K))
            self._place(buf, off['B'], case.K, case.ldb, case.N, dev(b, case.K, b.shape[1] // eb))
        noise = self._noise()                                       # C and its pads: canonical noise
        n = sizes['C']
        reps = cdiv(n, noise.numel())
        buf[off['C']:off['C'] + n] = noise.repeat(reps)[:n]
        return buf, off, sizes, dev(c, c.shape[0], c.shape[1] // eb)

    def _check(self, got, want, case, off, sizes):
        torch, eb = self.ad.torch, self.t.eb
        if torch.equal(got, want):
            return
        kinds, notes = set(), []
        pos = torch.nonzero(got != want).reshape(-1)
        for name in ('A', 'B', 'C'):
            lo, hi = off[name], off[name] + sizes[name]
            inside = pos[(pos >= lo) & (pos < hi)]
            if not inside.numel():
                continue
            if name == 'C':
                col = (inside - lo) % (case.ldc * eb)
                for kind, sel in (('out', inside[col < case.N * eb]), ('pad', inside[col >= case.N * eb])):
                    if sel.numel():
                        p = int(sel[0])
                        e = lo + (p - lo) // eb * eb
                        i, j = divmod((e - lo) // eb, case.ldc)
                        kinds.add(kind)
                        notes.append('%s: C[%d, %d] got %s, want %s (%d bytes differ)' % (
                            kind, i, j, _hex(got[e:e + eb].cpu().numpy()), _hex(want[e:e + eb].cpu().numpy()), sel.numel()))
            else:
                kinds.add('input')
                notes.append('input %s changed at byte %d' % (name, int(inside[0]) - lo))
        outside = pos
        for name in ('A', 'B', 'C'):
            outside = outside[(outside < off[name]) | (outside >= off[name] + sizes[name])]
        if outside.numel():
            kinds.add('guard')
            p = int(outside[0])
            near = min(('A', 'B', 'C'), key=lambda s: min(abs(p - off[s]), abs(p - off[s] - sizes[s])))
            notes.append('guard byte %d changed (%d bytes before %s, %d past its end)' % (p, off[near] - p, near, p - off[near] - sizes[near]))
        raise ContractViolation(kinds, '%r: %s' % (case, '; '.join(notes)))

    # ---- one call ----
    def run(self, case):
        """assert the plan the case claims, make the call, compare the whole tensor"""
        torch, t = self.ad.torch, self.t
        p = case.check_plan(t, self.env)
        buf, off, sizes, cper = self._prepare(case)
        want = buf.clone()
        a, b = (None, None) if case.null_ab else (off['A'], off['B'])
        rc = self.ad.matmul(buf, a, case.lda, b, case.ldb, off['C'], case.ldc, case.M, case.K, case.N)
        assert rc == OK, (case, rc)
        self.ad.sync()
        self._place(want, off['C'], case.M, case.ldc, case.N, cper)
        self._check(buf, want, case, off, sizes)
        self.cases += 1
        self.seen.add(p.route)
        self.seen.update(case.edges)
        del buf, want
        return p

    def run_all(self, cases):
        for c in cases:
            self.run(c)
        return len(cases)

    def run_family(self, name):
        return self.run_all(family(name, self.t.modulus, self.t.binary, self.env))

    def run_refused(self):
        """M == 0 or N == 0: FFGPU_OK; lda < K, ldb < N, ldc < N, C == NULL: FFGPU_EINVAL; not a byte changes either way"""
        torch = self.ad.torch
        M, K, N = 5, 70, 9
        base = Case('refused', M, K, N, None, lda=K + 1, ldb=N + 1, ldc=N + 1)
        calls = [('M=0', OK, dict(M=0)), ('N=0', OK, dict(N=0)), ('lda<K', EINVAL, dict(lda=K - 1)), ('ldb<N', EINVAL, dict(ldb=N - 1)),
                 ('ldc<N', EINVAL, dict(ldc=N - 1)), ('C=NULL', EINVAL, dict(c=None))]
        for name, status, change in calls:
            buf, off, sizes, _ = self._prepare(base)
            want = buf.clone()
            args = dict(a=off['A'], lda=base.lda, b=off['B'], ldb=base.ldb, c=off['C'], ldc=base.ldc, M=M, K=K, N=N)
            args.update(change)
            rc = self.ad.matmul(buf, args['a'], args['lda'], args['b'], args['ldb'], args['c'], args['ldc'], args['M'], args['K'], args['N'])
            assert rc == status, (name, rc)
            self.ad.sync()
            base.label = 'refused/' + name
            self._check(buf, want, base, off, sizes)
            self.cases += 1
            self.seen.add('refused/' + name)
        return len(calls)
