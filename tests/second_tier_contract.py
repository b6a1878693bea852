"""TEST INFRASTRUCTURE ONLY: the driver of the contract tests of the "second-tier" entry points of include/ffgpu.h --
ffgpu_dot / ffgpu_sum, ffgpu_gauss and ffgpu_group_matvec -- at the sizes where their launch plans change.

One case = one call (dot: the three calls dot(a, b), sum(a), dot(a, a)) on views into ONE backing tensor
guard | operand | guard | ... | guard, guards of 0xA5.  After the call the whole tensor is compared, byte for byte, with
an image built from the reference: an output holds the expected value, what the header leaves unspecified (the workspace
of dot / sum, the left n columns of a solved system, a singular matrix) is taken over from the result, and every other
byte -- operands and guards -- is what was uploaded.  The workspace of dot / sum is a view of exactly
FFGPU_REDUCE_WORKSPACE_BYTES bytes with WS_GUARD bytes of guard on each side inside the same tensor, so a launcher that
writes more partial sums than the workspace holds fails on the guard and never writes outside the allocation.

Expected values never come from the code under test: Python integers and oracle/pyoracle (po.add, po.mul, po._dot,
po.gauss_solve, po.gauss_det, pinned to the goldens by tests/test_oracle_golden.py), or construction: a dot over a
periodic array is (n // L) * D + prefix[n % L]; a matrix A = P U with U upper triangular and P a cyclic row shift has one
candidate pivot per column, determinant prod U[k][k], and A X = B has the chosen X as its solution.

Nothing here imports the GPU at module level: tests/test_second_tier_contract_host.py drives the same code against
tests/cpuctx.CpuFieldContext and against deliberately wrong contexts."""
import functools
import random

import numpy as np

from ew_contract import ContractViolation, GUARD_BYTE, ints_to_bytes
from fieldutil import edge_values
from oracle import pyoracle as po
from oracle.coracle import elem_bytes

OK, EINVAL, ENOTSUP = 0, 1, 2           # include/ffgpu.h: FFGPU_OK, FFGPU_EINVAL, FFGPU_ENOTSUP

# ---- the launch geometry, restated (each constant with the place it lives) ---------------------------------------------
BLOCK = 256                             # mpyc_amd/csrc/kernels.hpp: enum { BLOCK = 256 }, threads of a workgroup
DOT_PACKS_PER_THREAD = 8                # launch.hpp Launchers::dot: want = ceil(iters / (BLOCK * 8)) workgroups
DOT_MAX_BLOCKS = 1024                   # kernels.hpp: enum { DOT_MAX_BLOCKS = 1024 }
DOT_FLUSH = 192                         # kernels.hpp k_dot_partial: `cnt >= 192` -- words in the pack loop, elements in the scalar one
PACK_BYTES = 16                         # kernels.hpp Pack<W>: what one lane moves per access
WAVE = 64                               # launch.hpp Launchers::nvec_of: 24-byte elements go in whole waves, nvec = n & ~63
REDUCE_WORKSPACE_BYTES = 1024 * 16      # include/ffgpu.h: FFGPU_REDUCE_WORKSPACE_BYTES
GAUSS_ZMAX = 32768                      # launch.hpp Launchers::gauss: matrices per chunk (grid.z)
GM_MAX = 16                             # kernels.hpp: enum { GM_MAX = 16 }, the largest r and g of group_matvec

DOT_BLOCK_ITERS = BLOCK * DOT_PACKS_PER_THREAD          # 2048 iterations (packs, or elements on unaligned views) per workgroup
DOT_GRIDS = (1, 2, 682, 683, 1023, 1024, 1025)          # 682 = 16384 // 24: the last grid whose 24-byte partials fit the workspace
DOT_SMALL = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4099)
PERIOD = 4099                           # elements of the block that is tiled to length n
WS_GUARD = 16384                        # >= the 8192 bytes that 1024 partials of 24 bytes overrun the workspace by
GUARD = 1024                            # bytes of guard between the other operands (>= 42 elements of any field)

GAUSS_SMALL_N = (1, 2, 3, 4, 5, 8, 17)
GAUSS_KINDS = ('rand', 'swap', 'swap2', 'singular', 'zero')     # tests/golden/make_golden.py linalg_cases
GAUSS_WIDE_N = (2, 5)
GAUSS_TALL_N = (257, 260, 513)
GAUSS_BATCHES = ((2, (0,)), (2, (1,)), (7, (0, 3, 6)), (64, (0, 32, 63)))       # (batch, positions of singular matrices)
GAUSS_BIG_BATCHES = (GAUSS_ZMAX - 1, GAUSS_ZMAX, GAUSS_ZMAX + 1, 2 * GAUSS_ZMAX + 1)
GM_DIMS = (1, 2, 7, 8, 15, 16)
GM_NGROUPS = (0, 1, 2, 63, 64, 65, 1025)


def word_bytes(eb):
    """sizeof(F::word), fields.hpp: GF(2^n <= 8) packs four bytes in a 32-bit word, 12-byte elements compute in 16-byte words"""
    return {1: 4, 4: 4, 8: 8, 12: 16, 16: 16, 24: 24}[eb]


def elems_per_word(eb):
    return 4 if eb == 1 else 1                      # F::EPW


def elems_per_pack(eb):
    """Launchers::EPV = Pack<W>::N * EPW; 12-, 16- and 24-byte elements go one per lane"""
    return PACK_BYTES // eb if eb <= 8 else 1


def has_unaligned_views(eb):
    """Launchers::al: 16-byte alignment (12-byte elements: 4).  A view one element in is unaligned for 1-, 4-, 8- and 24-byte
    elements only"""
    return eb in (1, 4, 8, 24)


def dot_iters(eb, n, aligned):
    """what Launchers::dot sizes its grid by: packs through the pack loop, elements when there is none"""
    if not aligned:
        nvec = 0
    elif eb == 24:
        nvec = n & ~(WAVE - 1)
    else:
        nvec = n // elems_per_pack(eb)
    return nvec or n


def dot_max_grid(eb):
    """the bound of the grid: DOT_MAX_BLOCKS, and no more partial words than the workspace holds"""
    return min(DOT_MAX_BLOCKS, REDUCE_WORKSPACE_BYTES // word_bytes(eb))


def dot_grid(eb, n, aligned):
    want = -(-dot_iters(eb, n, aligned) // DOT_BLOCK_ITERS)
    return max(1, min(want, dot_max_grid(eb)))


def _dot_n(eb, iters, aligned, tail):
    """the n whose plan has `iters` iterations, plus a scalar tail (aligned views only: the largest one, or none)"""
    if not aligned:
        return iters
    if eb == 24:
        assert iters % WAVE == 0
        return iters + (WAVE - 1 if tail else 0)
    epp = elems_per_pack(eb)
    return iters * epp + (epp - 1 if tail else 0)


def dot_grid_edge_sizes(eb, aligned):
    """(g, delta, n): iters = 2048 g + delta for g in DOT_GRIDS, delta in -1, 0, 1 (24-byte elements on aligned views move
    in waves: delta in -64, 0, 64); off the edge with the largest scalar tail, on it with none"""
    step = WAVE if (eb == 24 and aligned) else 1
    return [(g, d, _dot_n(eb, DOT_BLOCK_ITERS * g + d * step, aligned, d != 0)) for g in DOT_GRIDS for d in (-1, 0, 1)]


def dot_loop_size(eb, aligned):
    """3 x DOT_MAX_BLOCKS x 2048 iterations plus an odd tail: every thread of the saturated grid loops"""
    n = _dot_n(eb, 3 * DOT_MAX_BLOCKS * DOT_BLOCK_ITERS, aligned, True)
    return n if n % 2 else n + 1


def dot_flush_size(eb, aligned):
    """the smallest n at which every thread of the saturated grid flushes once and accumulates again: DOT_FLUSH words
    (elements in the scalar loop) per thread, one more round, an odd tail"""
    words_per_iter = (PACK_BYTES // word_bytes(eb) if eb != 24 else 1) if aligned else 1
    rounds = -(-DOT_FLUSH // words_per_iter) + 1
    n = _dot_n(eb, dot_max_grid(eb) * BLOCK * rounds, aligned, True)
    return n if n % 2 else n + 1


def _align16(x):
    return -(-x // 16) * 16


def _hex(raw):
    return bytes(raw)[::-1].hex()


# ---- references ------------------------------------------------------------------------------------------------------------
def _mult(F, k, v):
    """k * v in the field, k a count"""
    return (v if k & 1 else 0) if F.binary else k * v % F.modulus


def _rand_elems(F, rng, n):
    return [rng.randrange(F.order) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def dot_blocks(modulus, binary):
    """the two blocks of PERIOD elements -- edge values first, then uniform random -- with the prefix tables of a . b, a . a and
    sum a (entry i: over the first i elements), computed once per field with po.add / po.mul"""
    F = po.Field(modulus, binary)
    eb = elem_bytes(modulus, binary)
    rng = random.Random(modulus % 100003 + 7)
    edges = edge_values(F)
    a = (edges + _rand_elems(F, rng, PERIOD))[:PERIOD]
    b = (edges[::-1] + _rand_elems(F, rng, PERIOD))[:PERIOD]
    pab, paa, psa = [0], [0], [0]
    for x, y in zip(a, b):
        pab.append(po.add(F, pab[-1], po.mul(F, x, y)))
        paa.append(po.add(F, paa[-1], po.mul(F, x, x)))
        psa.append(po.add(F, psa[-1], x))
    return {'a': ints_to_bytes(a, eb), 'b': ints_to_bytes(b, eb), 'ab': pab, 'aa': paa, 'sa': psa, 'ints': (a, b)}


def dot_expected(F, n, data):
    """(dot(a, b), sum(a), dot(a, a)) of the arrays of length n: 'tiled' the blocks of dot_blocks repeated, 'max' every
    element q - 1 (primes: (-1)^2 = 1, so dot = n and sum = -n; GF(2^n): the all-ones element, by parity)"""
    if data == 'max':
        e = F.order - 1
        sq = po.mul(F, e, e)
        return _mult(F, n, sq), _mult(F, n, e), _mult(F, n, sq)
    blk = dot_blocks(F.modulus, F.binary)
    k, r = divmod(n, PERIOD)
    return tuple(po.add(F, _mult(F, k, blk[t][PERIOD]), blk[t][r]) for t in ('ab', 'sa', 'aa'))


def gauss_kind_matrix(F, rng, n, kind):
    """the matrix kinds of tests/golden/make_golden.py: random; a zero pivot (from n = 3 on the first usable pivot is two rows
    down); the same with a second zero pivot further down; a dependent last row; all zero"""
    q = F.order
    A = [_rand_elems(F, rng, n) for _ in range(n)]
    if kind.startswith('swap'):
        A[0][0] = 0
        if n > 2:
            A[1][0] = 0
        if kind == 'swap2' and n > 3:
            A[3][3] = 0
    elif kind == 'singular':
        if n > 2:
            A[n - 1] = [po.add(F, x, y) for x, y in zip(A[0], A[1])]
        else:                                                # n = 2: three times the first row; n = 1: zero
            A[n - 1] = [po.mul(F, 3, x) for x in A[0]] if n == 2 else [0]
    elif kind == 'zero':
        A = [[0] * n for _ in range(n)]
    return A


def ref_solve(F, A, B):
    """po.gauss_solve, None for a singular matrix"""
    try:
        return po.gauss_solve(F, A, B)
    except ZeroDivisionError:
        return None


class GaussCase:
    """a batch of (n x ncols) systems with what the header specifies about the result"""

    def __init__(self, F, n, ncols, mats, sols, dets, label):
        # mats: batch lists of n rows of ncols ints; sols: per matrix n rows of ncols - n ints, or None (singular);
        # dets: per matrix the determinant (det mode) or None
        self.F, self.n, self.ncols, self.label = F, n, ncols, label
        self.mats, self.sols, self.dets = mats, sols, dets
        self.batch = len(mats)


@functools.lru_cache(maxsize=None)
def gauss_small_cases(modulus, binary):
    """n in GAUSS_SMALL_N: one batch of the five kinds per n with two right-hand sides, solved and with determinants"""
    F = po.Field(modulus, binary)
    rng = random.Random(modulus % 100003 + 11)
    out = []
    for n in GAUSS_SMALL_N:
        As = [gauss_kind_matrix(F, rng, n, kind) for kind in GAUSS_KINDS]
        Bs = [[_rand_elems(F, rng, 2) for _ in range(n)] for _ in As]
        mats = [[ra + rb for ra, rb in zip(A, B)] for A, B in zip(As, Bs)]
        out.append(GaussCase(F, n, n + 2, mats, [ref_solve(F, A, B) for A, B in zip(As, Bs)],
                             [po.gauss_det(F, A) for A in As], 'small n=%d' % n))
    return out


def _nonsingular(F, rng, n):
    while True:
        A = [_rand_elems(F, rng, n) for _ in range(n)]
        if po.gauss_det(F, A):
            return A


def gauss_wide_ncols(n):
    """ncols - k - 1, the columns k_gauss_elim covers, crosses BLOCK and 2 BLOCK at k = 0 for ncols = 257 | 258 and 513 | 514, at
    the last k = n - 1 for ncols = n + BLOCK | + 1 and n + 2 BLOCK | + 1; n and n + 1: no and one right-hand side"""
    return sorted({n, n + 1, BLOCK, BLOCK + 1, BLOCK + 2, 2 * BLOCK + 1, 2 * BLOCK + 2, n + BLOCK, n + BLOCK + 1,
                   n + 2 * BLOCK, n + 2 * BLOCK + 1})


@functools.lru_cache(maxsize=None)
def gauss_wide_cases(modulus, binary):
    """n in GAUSS_WIDE_N x gauss_wide_ncols, solve mode against po.gauss_solve.  Fields whose Python arithmetic is slow
    (GF(2^n), n > 8) repeat their right-hand sides with period 11 -- coprime to BLOCK --, the solution repeats with them"""
    F = po.Field(modulus, binary)
    rng = random.Random(modulus % 100003 + 13)
    slow = binary and F.order > 256
    out = []
    for n in GAUSS_WIDE_N:
        A = _nonsingular(F, rng, n)
        if n > 2:
            A[0][0] = 0                                      # a row swap in the first column
            if not po.gauss_det(F, A):
                A = _nonsingular(F, rng, n)
        for ncols in gauss_wide_ncols(n):
            rhs = ncols - n
            per = min(rhs, 11) if slow else rhs
            B = [_rand_elems(F, rng, per) for _ in range(n)]
            X = po.gauss_solve(F, A, B) if per else [[] for _ in range(n)]
            B = [[row[j % per] for j in range(rhs)] for row in B]
            X = [[row[j % per] for j in range(rhs)] for row in X]
            out.append(GaussCase(F, n, ncols, [[ra + rb for ra, rb in zip(A, B)]], [X], None, 'wide n=%d ncols=%d' % (n, ncols)))
    return out


def tall_system(F, n, rhs, seed, zero_row=None):
    """A = P U: U upper triangular with a nonzero diagonal, otherwise random, P the cyclic row shift by one (row i of A is row
    i + 1 of U, the last row of A is row 0 of U).  In column k the only nonzero entry at or below the diagonal sits in row n - 1,
    n - 1 - k rows down, so the pivot rule has no choice: det = prod U[k][k].  B = A X for a chosen X.  zero_row: that row of U
    is zero, so A is singular.  Returns (A, B, X, det)."""
    rng = random.Random(seed)
    q = F.order
    U = [[0] * r + [rng.randrange(1, q)] + _rand_elems(F, rng, n - r - 1) for r in range(n)]
    if zero_row is not None:
        U[zero_row] = [0] * n
    X = [_rand_elems(F, rng, rhs) for _ in range(n)]
    cols = [[X[c][j] for c in range(n)] for j in range(rhs)]
    UX = [[po._dot(F, U[r][r:], col[r:]) for col in cols] for r in range(n)]
    det = 1
    for r in range(n):
        det = po.mul(F, det, U[r][r])
    shift = lambda rows: rows[1:] + rows[:1]
    return shift(U), shift(UX), X, det


@functools.lru_cache(maxsize=None)
def gauss_tall_cases(modulus, binary, sizes=GAUSS_TALL_N):
    """per n a batch of two: the singular variant (row n // 2 of U zero) first, then the regular system; one right-hand side"""
    F = po.Field(modulus, binary)
    out = []
    for n in sizes:
        A0, B0, _, _ = tall_system(F, n, 1, modulus % 100003 + n, zero_row=n // 2)
        A1, B1, X1, d1 = tall_system(F, n, 1, modulus % 100003 + n + 1)
        mats = [[ra + rb for ra, rb in zip(A, B)] for A, B in ((A0, B0), (A1, B1))]
        out.append(GaussCase(F, n, n + 1, mats, [None, X1], [0, d1], 'tall n=%d' % n))
    return out


class GaussPool:
    """POOL small systems solved once with po; a batch of any size takes them in turn (period POOL - 2, coprime to the chunk
    size), with the two singular ones -- a dependent row; all zero -- planted where the case wants them"""
    POOL = 13

    def __init__(self, F, n, rhs, seed):
        rng = random.Random(seed)
        eb = elem_bytes(F.modulus, F.binary)
        kinds = ['singular' if n > 1 else 'zero', 'zero'] + ['rand', 'swap'] * ((self.POOL - 2) // 2) + ['rand']
        self.F, self.n, self.ncols, self.eb = F, n, n + rhs, eb
        As = [gauss_kind_matrix(F, rng, n, k) for k in kinds]
        self.dets = [po.gauss_det(F, A) for A in As]
        for i in range(2, self.POOL):
            while not self.dets[i]:                                  # (tiny fields: draw again)
                As[i] = gauss_kind_matrix(F, rng, n, kinds[i])
                self.dets[i] = po.gauss_det(F, As[i])
        Bs = [[_rand_elems(F, rng, rhs) for _ in range(n)] for _ in As]
        self.mats = [[ra + rb for ra, rb in zip(A, B)] for A, B in zip(As, Bs)]
        # (without a right-hand side there is nothing to solve: singular is what has determinant 0)
        self.sols = [(ref_solve(F, A, B) if rhs else [[] for _ in range(n)]) if d else None for A, B, d in zip(As, Bs, self.dets)]
        assert self.sols[0] is None and self.sols[1] is None and all(s is not None for s in self.sols[2:])
        flat = lambda rows: [v for row in rows for v in row]
        self.mat_bytes = np.stack([ints_to_bytes(flat(m), eb) for m in self.mats])
        zero = [[0] * rhs] * n
        self.sol_bytes = np.stack([ints_to_bytes(flat(s if s is not None else zero), eb).reshape(n, rhs * eb)
                                   for s in self.sols]) if rhs else None
        self.det_bytes = np.stack([ints_to_bytes([d], eb) for d in self.dets])

    def indices(self, batch, singular_at):
        idx = 2 + np.arange(batch) % (self.POOL - 2)
        for j, pos in enumerate(sorted(singular_at)):
            idx[pos] = j % 2
        return idx


@functools.lru_cache(maxsize=None)
def gauss_pool(modulus, binary, n, rhs):
    return GaussPool(po.Field(modulus, binary), n, rhs, modulus % 100003 + 17 * n + rhs)


def big_batch_singular_at(batch):
    """the first and the last matrix, the last of chunk one and the first of chunk two"""
    return sorted({p for p in (0, GAUSS_ZMAX - 1, GAUSS_ZMAX, batch - 1) if 0 <= p < batch})


class GroupPool:
    """one (r, g): a random matrix with a random bias, and PG input groups -- all zero, all q - 1, then random -- with their
    outputs from po._dot / po.add, computed once; group i of a call is pool group i mod PG.  PG = 67 > 65, so up to 65 groups
    are all different; fields whose Python arithmetic is slow (GF(2^n), n > 8) take 13"""

    def __init__(self, F, r, g, seed):
        rng = random.Random(seed)
        eb = elem_bytes(F.modulus, F.binary)
        q = F.order
        self.PG = 13 if F.binary and q > 256 else 67
        self.F, self.r, self.g, self.eb = F, r, g, eb
        self.M = [_rand_elems(F, rng, g) for _ in range(r)]
        self.bias = _rand_elems(F, rng, r)
        groups = [[0] * g, [q - 1] * g] + [_rand_elems(F, rng, g) for _ in range(self.PG - 2)]
        outs = [[po.add(F, po._dot(F, row, grp), b) for row, b in zip(self.M, self.bias)] for grp in groups]
        self.in_bytes = np.stack([ints_to_bytes(grp, eb) for grp in groups])
        self.out_bytes = np.stack([ints_to_bytes(o, eb) for o in outs])

    def data(self, ngroups):
        idx = np.arange(ngroups) % self.PG
        return self.in_bytes[idx].reshape(-1), self.out_bytes[idx].reshape(-1)


@functools.lru_cache(maxsize=None)
def group_pool(modulus, binary, r, g):
    return GroupPool(po.Field(modulus, binary), r, g, modulus % 100003 + 31 * r + g)


def group_max_case(F, r, g, ngroups, with_bias):
    """every matrix entry and every input element q - 1, the worst case of the g-term lazy accumulator: a term is (q - 1)^2
    (1 for a prime), a row g of them, plus the bias q - 1 or none"""
    eb = elem_bytes(F.modulus, F.binary)
    e = F.order - 1
    v = _mult(F, g, po.mul(F, e, e))
    if with_bias:
        v = po.add(F, v, e)
    M, bias = [[e] * g for _ in range(r)], ([e] * r if with_bias else None)
    return M, bias, np.tile(ints_to_bytes([e], eb), g * ngroups), np.tile(ints_to_bytes([v], eb), r * ngroups)


# ---- adapters --------------------------------------------------------------------------------------------------------------
class CpuAdapter:
    """an engine-style context on CPU tensors (tests/cpuctx.CpuFieldContext and the wrong contexts of the host test) behind the
    signature of the C ABI: the same argument checks as api.hip, results copied into the slots the caller names"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.eb, self.device = torch, ctx, ctx.elem_bytes, torch.device('cpu')

    def _view(self, buf, off, n):
        from mpyc_amd import engine
        t = buf[off:off + n * self.eb].view(engine._torch_dtype(self.eb))
        limbs = engine.limbs_of(self.eb)
        return engine.DevArray(self.ctx, t.reshape(n, limbs) if limbs else t, n)

    def _store(self, buf, off, arr):
        raw = arr.t.contiguous().view(self.torch.uint8).reshape(-1)
        buf[off:off + raw.numel()] = raw

    def dot(self, buf, a, b, out, ws, n):
        A = self._view(buf, a, n)
        self._store(buf, out, self.ctx.sum(A) if b is None else self.ctx.dot(A, A if b == a else self._view(buf, b, n)))
        return OK

    def gauss(self, buf, a, n, ncols, batch, mode, det, sing):
        if n < 0 or ncols < n or mode not in (0, 1):
            return EINVAL
        if batch == 0:
            return OK
        if sing is None or (mode == 1 and det is None):
            return EINVAL
        if n == 0:
            return OK
        d, flags = self.ctx.gauss(self._view(buf, a, batch * n * ncols), n, ncols, batch, det=bool(mode))
        if mode:
            self._store(buf, det, d)
        buf[sing:sing + 4 * batch] = flags[:batch].contiguous().view(self.torch.uint8).reshape(-1)
        return OK

    def group_matvec(self, buf, M, bias, r, g, src, dst, ngroups):
        if r < 1 or g < 1:
            return EINVAL
        if r > GM_MAX or g > GM_MAX:
            return ENOTSUP
        self._store(buf, dst, self.ctx.group_matvec(self._view(buf, src, g * ngroups), [list(row) for row in M], bias))
        return OK

    def sync(self):
        pass


class GpuAdapter:
    """the C ABI itself on base pointer + byte offset (the engine wrappers own their workspace, flags and outputs)"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.eb, self.device = torch, ctx, ctx.elem_bytes, ctx.torch_device

    @staticmethod
    def _p(buf, off):
        return None if off is None else buf.data_ptr() + off

    def dot(self, buf, a, b, out, ws, n):
        c = self.ctx
        if b is None:
            return c._L.ffgpu_sum(c._h, self._p(buf, a), self._p(buf, out), self._p(buf, ws), n, c._stream())
        return c._L.ffgpu_dot(c._h, self._p(buf, a), self._p(buf, b), self._p(buf, out), self._p(buf, ws), n, c._stream())

    def gauss(self, buf, a, n, ncols, batch, mode, det, sing):
        c = self.ctx
        return c._L.ffgpu_gauss(c._h, self._p(buf, a), n, ncols, batch, mode, self._p(buf, det), self._p(buf, sing), c._stream())

    def group_matvec(self, buf, M, bias, r, g, src, dst, ngroups):
        c = self.ctx
        m = c._scalars([v for row in M for v in row])
        b = c._scalars(bias) if bias is not None else None
        return c._L.ffgpu_group_matvec(c._h, m, b, r, g, self._p(buf, src), self._p(buf, dst), ngroups, c._stream())

    def sync(self):
        self.torch.cuda.synchronize()


# ---- the driver ------------------------------------------------------------------------------------------------------------
class Driver:
    def __init__(self, adapter, modulus, binary):
        self.ad, self.F = adapter, po.Field(modulus, binary)
        self.modulus, self.binary = int(modulus), bool(binary)
        self.eb = elem_bytes(modulus, binary)
        assert adapter.eb == self.eb
        self.q = self.F.order
        self.cases = 0              # calls compared with the reference
        self.seen = set()
        self.max_bytes = 0          # the largest backing tensor

    # ---- buffers ----
    def _alloc(self, total):
        torch = self.ad.torch
        self.max_bytes = max(self.max_bytes, total)
        return torch.full((total,), GUARD_BYTE, dtype=torch.uint8, device=self.ad.device)

    def _upload(self, img):
        self.max_bytes = max(self.max_bytes, img.size)
        return self.ad.torch.from_numpy(img.copy()).to(self.ad.device)

    def _tile(self, buf, off, block, nbytes):
        """buf[off : off + nbytes] = block repeated (block: a uint8 tensor on the device)"""
        lb = block.numel()
        k, rem = divmod(nbytes, lb)
        if k:
            buf[off:off + k * lb].view(k, lb).copy_(block.expand(k, lb))
        if rem:
            buf[off + k * lb:off + nbytes] = block[:rem]

    def _check(self, got, want, regions, where):
        """got, want: uint8 tensors of the whole backing tensor; regions: (name, lo, hi, kind) of every operand, kind 'out' or
        'input'; everything between them is guard"""
        torch = self.ad.torch
        if torch.equal(got, want):
            return
        kinds, notes, cur = set(), [], 0

        def first_diff(lo, hi):
            for c in range(lo, hi, 1 << 26):
                d = torch.nonzero(got[c:min(hi, c + (1 << 26))] != want[c:min(hi, c + (1 << 26))])
                if d.numel():
                    return c + int(d[0])
            return None
        for name, lo, hi, kind in sorted(regions, key=lambda r: r[1]) + [('', got.numel(), got.numel(), '')]:
            if lo > cur:
                p = first_diff(cur, lo)
                if p is not None:
                    kinds.add('guard')
                    notes.append('guard byte %d changed (before %r at %d)' % (p, name or 'the end', lo))
            if hi > lo:
                p = first_diff(lo, hi)
                if p is not None:
                    kinds.add(kind)
                    e = lo + (p - lo) // self.eb * self.eb
                    notes.append('%s %r differs at byte %d of %d: got %s, want %s' % (
                        kind, name, p - lo, hi - lo, _hex(got[e:e + self.eb].cpu().numpy()), _hex(want[e:e + self.eb].cpu().numpy())))
            cur = max(cur, hi)
        raise ContractViolation(kinds, '%r: %s' % (where, '; '.join(notes)))

    # ---- dot / sum ----
    def run_dot(self, n, aligned=True, data='tiled', same_pointer=True):
        """dot(a, b), sum(a) and, with same_pointer, dot(a, a) on arrays of n elements; aligned=False: a and b start one element
        past a 16-byte boundary.  data: see dot_expected."""
        torch, eb, F = self.ad.torch, self.eb, self.F
        assert aligned or has_unaligned_views(eb)
        shift = 0 if aligned else eb
        off, cur = {}, 0
        for s in ('a', 'b'):
            off[s] = _align16(cur + GUARD) + shift
            cur = off[s] + n * eb
        outs = ('dot', 'sum') + (('dot_aa',) if same_pointer else ())
        for s in outs:
            off[s] = _align16(cur + GUARD)
            cur = off[s] + eb
        off['ws'] = _align16(cur + WS_GUARD)
        total = off['ws'] + REDUCE_WORKSPACE_BYTES + WS_GUARD
        buf = self._alloc(total)
        if data == 'max':
            blocks = {s: torch.from_numpy(ints_to_bytes([self.q - 1], eb)).to(self.ad.device) for s in 'ab'}
        else:
            blk = dot_blocks(self.modulus, self.binary)
            blocks = {s: torch.from_numpy(blk[s]).to(self.ad.device) for s in 'ab'}
        for s in 'ab':
            self._tile(buf, off[s], blocks[s], n * eb)
        want = buf.clone()
        ws = off['ws']
        calls = {'dot': (off['a'], off['b']), 'sum': (off['a'], None), 'dot_aa': (off['a'], off['a'])}
        for s in outs:
            rc = self.ad.dot(buf, calls[s][0], calls[s][1], off[s], ws, n)
            assert rc == OK, (s, n, rc)
        self.ad.sync()
        exp = dict(zip(('dot', 'sum', 'dot_aa'), dot_expected(F, n, data)))
        for s in outs:
            want[off[s]:off[s] + eb] = torch.from_numpy(ints_to_bytes([exp[s]], eb)).to(self.ad.device)
        if n:                                   # the contents of the workspace are the library's; n = 0 leaves it alone
            want[ws:ws + REDUCE_WORKSPACE_BYTES] = buf[ws:ws + REDUCE_WORKSPACE_BYTES]
        regions = [(s, off[s], off[s] + n * eb, 'input') for s in 'ab'] + [(s, off[s], off[s] + eb, 'out') for s in outs]
        regions.append(('workspace', ws, ws + REDUCE_WORKSPACE_BYTES, 'out'))
        self._check(buf, want, regions, ('dot/sum', n, 'aligned' if aligned else 'one-in', data))
        self.cases += len(outs)
        self.seen.add(('dot', n, aligned, data))
        del buf, want

    # ---- gauss ----
    def run_gauss(self, case, mode, idx=None, pool=None):
        """one call on a GaussCase, or -- idx given -- on the batch that takes pool system idx[i] as matrix i.  mode 0: the
        right-hand columns of the non-singular systems and the flags are compared, det_out must stay untouched; mode 1:
        det_out and the flags.  What a mode leaves unspecified -- the left n columns, singular systems, in mode 1 all matrices
        -- is taken over from the result.  Every guard is compared."""
        eb = self.eb
        flat = lambda rows: [v for row in rows for v in row]
        if pool is not None:
            n, ncols, batch = pool.n, pool.ncols, len(idx)
            mats = pool.mat_bytes[idx].reshape(-1)
            singular = idx < 2
            sol = pool.sol_bytes[idx] if pool.sol_bytes is not None else None          # (batch, n, rhs * eb)
            det = pool.det_bytes[idx].reshape(-1)
            label = 'pool n=%d ncols=%d batch=%d' % (n, ncols, batch)
        else:
            n, ncols, batch, label = case.n, case.ncols, case.batch, case.label
            rhs = ncols - n
            mats = ints_to_bytes([v for m in case.mats for v in flat(m)], eb)
            if mode == 0:
                singular = np.array([s is None for s in case.sols])
                sol = np.stack([ints_to_bytes(flat(s if s is not None else [[0] * rhs] * n), eb).reshape(n, rhs * eb)
                                for s in case.sols]) if rhs else None
            else:
                singular = np.array([d == 0 for d in case.dets])
                det = ints_to_bytes(case.dets, eb)
        off_a = _align16(GUARD)
        off_d = _align16(off_a + mats.size + GUARD)
        off_s = _align16(off_d + batch * eb + GUARD)
        total = _align16(off_s + 4 * batch + GUARD)
        img = np.full(total, GUARD_BYTE, dtype=np.uint8)            # det_out and the flags start as 0xA5 too
        img[off_a:off_a + mats.size] = mats
        buf = self._upload(img)
        rc = self.ad.gauss(buf, off_a, n, ncols, batch, mode, off_d, off_s)
        assert rc == OK, (label, mode, rc)
        self.ad.sync()
        got = buf.cpu().numpy()
        want = img.copy()
        want[off_s:off_s + 4 * batch] = singular.astype('<i4').view(np.uint8)
        want[off_a:off_a + mats.size] = got[off_a:off_a + mats.size]
        if mode == 1:
            want[off_d:off_d + batch * eb] = det
        elif ncols > n:
            w = want[off_a:off_a + mats.size].reshape(batch, n, ncols * eb)
            w[~singular, :, n * eb:] = sol[~singular]
        regions = [('matrices', off_a, off_a + mats.size, 'out'), ('det_out', off_d, off_d + batch * eb, 'out'),
                   ('dev_singular', off_s, off_s + 4 * batch, 'out')]
        t = self.ad.torch
        self._check(t.from_numpy(got), t.from_numpy(want), regions, ('gauss', label, 'det' if mode else 'solve'))
        self.cases += 1
        self.seen.add(('gauss', label, mode))

    def run_gauss_untouched(self, n, ncols, batch, mode, room=3):
        """batch = 0 or n = 0: FFGPU_OK, and not a byte changes -- matrices, det_out and flags (room for `room` matrices of
        max(n, 1) x max(ncols, 1)) included"""
        eb = self.eb
        rng = np.random.default_rng(n * 131 + ncols * 17 + batch)
        msize = room * max(n, 1) * max(ncols, 1) * eb
        off_a = _align16(GUARD)
        off_d = _align16(off_a + msize + GUARD)
        off_s = _align16(off_d + room * eb + GUARD)
        total = _align16(off_s + 4 * room + GUARD)
        img = np.full(total, GUARD_BYTE, dtype=np.uint8)
        img[off_a:off_a + msize] = rng.integers(0, 256, size=msize, dtype=np.uint8)
        buf = self._upload(img)
        rc = self.ad.gauss(buf, off_a, n, ncols, batch, mode, off_d, off_s)
        assert rc == OK, (n, ncols, batch, mode, rc)
        self.ad.sync()
        t = self.ad.torch
        regions = [('matrices', off_a, off_a + msize, 'out'), ('det_out', off_d, off_d + room * eb, 'out'),
                   ('dev_singular', off_s, off_s + 4 * room, 'out')]
        self._check(buf.cpu(), t.from_numpy(img), regions, ('gauss untouched', n, ncols, batch, mode))
        self.cases += 1

    def run_gauss_matrix(self, tall=False, tall_sizes=GAUSS_TALL_N, big=GAUSS_BIG_BATCHES):
        """small (both modes), wide (solve), the batches with singular systems planted, the large batches, the edges; tall on
        request (one field per element width)"""
        for case in gauss_small_cases(self.modulus, self.binary):
            for mode in (0, 1):
                self.run_gauss(case, mode)
        for case in gauss_wide_cases(self.modulus, self.binary):
            self.run_gauss(case, 0)
        if tall:
            for case in gauss_tall_cases(self.modulus, self.binary, tuple(tall_sizes)):
                for mode in (0, 1):
                    self.run_gauss(case, mode)
        solve3, det3 = gauss_pool(self.modulus, self.binary, 3, 2), gauss_pool(self.modulus, self.binary, 3, 0)
        for batch, at in GAUSS_BATCHES:
            self.run_gauss(None, 0, solve3.indices(batch, at), solve3)
            self.run_gauss(None, 1, det3.indices(batch, at), det3)
        solve2, det2 = gauss_pool(self.modulus, self.binary, 2, 1), gauss_pool(self.modulus, self.binary, 2, 0)
        for batch in big:
            at = big_batch_singular_at(batch)
            self.run_gauss(None, 0, solve2.indices(batch, at), solve2)
            self.run_gauss(None, 1, det2.indices(batch, at), det2)
        self.run_gauss(None, 0, det3.indices(7, (0, 3, 6)), det3)           # solve mode without a right-hand side: the flags
        for n, ncols, batch, mode in ((3, 5, 0, 0), (3, 3, 0, 1), (0, 0, 3, 0), (0, 2, 3, 0), (0, 0, 3, 1)):
            self.run_gauss_untouched(n, ncols, batch, mode)

    # ---- group_matvec ----
    def run_group(self, M, bias, in_bytes, out_bytes, ngroups, in_shift=0, out_shift=0, status=OK, label=''):
        """out[i r + a] = bias[a] + sum_c M[a][c] in[i g + c]; in / out start in_shift / out_shift bytes past a 16-byte
        boundary.  status != OK: that status, and not a byte changes."""
        r, g, eb = len(M), len(M[0]), self.eb
        off_i = _align16(GUARD) + in_shift
        off_o = _align16(off_i + g * ngroups * eb + GUARD) + out_shift
        total = _align16(off_o + r * ngroups * eb + GUARD)
        img = np.full(total, GUARD_BYTE, dtype=np.uint8)
        img[off_i:off_i + in_bytes.size] = in_bytes
        buf = self._upload(img)
        rc = self.ad.group_matvec(buf, M, bias, r, g, off_i, off_o, ngroups)
        assert rc == status, (label, r, g, ngroups, rc)
        self.ad.sync()
        want = img.copy()
        if status == OK:
            want[off_o:off_o + out_bytes.size] = out_bytes
        regions = [('in', off_i, off_i + g * ngroups * eb, 'input'), ('out', off_o, off_o + r * ngroups * eb, 'out')]
        t = self.ad.torch
        self._check(buf.cpu(), t.from_numpy(want), regions, ('group_matvec', label, r, g, ngroups, in_shift, out_shift))
        self.cases += 1
        self.seen.add(('group', label, r, g, ngroups, in_shift, out_shift))

    def run_group_matrix(self, dims=GM_DIMS, ngroups=GM_NGROUPS):
        """(r, g) in dims^2 x ngroups x {random matrix and bias; all q - 1 with bias q - 1; all q - 1 without bias}"""
        for r in dims:
            for g in dims:
                pool = group_pool(self.modulus, self.binary, r, g)
                for ng in ngroups:
                    src, dst = pool.data(ng)
                    self.run_group(pool.M, pool.bias, src, dst, ng, label='random')
                    for with_bias in (True, False):
                        M, bias, src, dst = group_max_case(self.F, r, g, ng, with_bias)
                        self.run_group(M, bias, src, dst, ng, label='max+bias' if with_bias else 'max')

    def run_group_byte_offsets(self, ngroups=65):
        """GF(2^n <= 8): (8, 8) and (1, 8) with in and out at every byte offset 0..7 -- the 8-byte fast paths at the offsets
        that allow them, the general kernel at the others -- for a random matrix, the all-ones case and, (1, 8), the powers of
        two of np_from_bits, which have a route of their own"""
        assert self.eb == 1
        F = self.F
        for r in (8, 1):
            pool = group_pool(self.modulus, self.binary, r, 8)
            src, dst = pool.data(ngroups)
            variants = [('random', pool.M, pool.bias, src, dst), ('max+bias',) + group_max_case(F, r, 8, ngroups, True)]
            if r == 1:
                pw = [[po.reduce(F, 1 << c) for c in range(8)]]
                outs = [po._dot(F, pw[0], [int(v) for v in src[8 * i:8 * i + 8]]) for i in range(ngroups)]
                variants.append(('from_bits', pw, None, src, ints_to_bytes(outs, 1)))
            for label, M, bias, s, d in variants:
                for i in range(8):
                    for o in range(8):
                        self.run_group(M, bias, s, d, ngroups, in_shift=i, out_shift=o, label=label)

    def run_group_too_large(self):
        """r = 17 or g = 17: FFGPU_ENOTSUP, nothing written"""
        eb = self.eb
        for r, g in ((GM_MAX + 1, 3), (3, GM_MAX + 1), (GM_MAX + 1, GM_MAX + 1)):
            M = [[1] * g for _ in range(r)]
            src = np.tile(ints_to_bytes([1], eb), g * 8)
            self.run_group(M, None, src, None, 8, status=ENOTSUP, label='too large')
