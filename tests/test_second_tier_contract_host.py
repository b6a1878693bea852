"""The driver of the dot / sum, gauss and group_matvec contract tests (tests/second_tier_contract.py) without a GPU: the sizes
it derives from the launch geometry are the ones meant, it passes on the Python-integer context of tests/cpuctx.py, and it
fails -- in the check meant for it, with the right kind of violation -- on contexts that are wrong the way a kernel or a
launcher could be.  A driver that cannot see these would not see the kernel bugs it exists for."""
import pytest

torch = pytest.importorskip('torch')

import second_tier_contract as st
from cpuctx import CpuFieldContext
from ew_contract import ContractViolation
from mpyc_amd.engine import DevArray
from oracle import pyoracle as po

P61, P96, P136, GF256 = (2**61 - 1, False), (2**96 - 17, False), (2**136 - 113, False), (0x11b, True)
FIELDS = [P61, P96, P136, GF256]
IDS = [hex(m) for m, _ in FIELDS]
DOT_SIZES = (0, 1, 2, 3, 17, 63, 64, 65, 255, 2047, 2048, 2049, 4099, 8200)       # thinned: Python integers


def driver(cls, modulus, binary, adapter=st.CpuAdapter):
    return st.Driver(adapter(cls(modulus, binary)), modulus, binary)


# ---- the derived sizes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eb', [1, 4, 8, 12, 16, 24])
def test_sizes_follow_the_launch_geometry(eb):
    for aligned in (True, False) if st.has_unaligned_views(eb) else (True,):
        cap = st.dot_max_grid(eb)
        for g, d, n in st.dot_grid_edge_sizes(eb, aligned):
            assert st.dot_grid(eb, n, aligned) == min(g + (d > 0), cap), (g, d, n)
            step = st.WAVE if eb == 24 and aligned else 1
            assert st.dot_iters(eb, n, aligned) == 2048 * g + d * step
        loop = st.dot_loop_size(eb, aligned)
        assert 0 <= st.dot_iters(eb, loop, aligned) - 3 * 1024 * 2048 <= 1 and loop % 2
        n = st.dot_flush_size(eb, aligned)
        # every thread of the saturated grid takes the words of one flush and one more iteration
        words = {1: 4, 4: 4, 8: 2}.get(eb, 1) if aligned else 1
        per_thread = st.dot_iters(eb, n, aligned) // (cap * st.BLOCK)
        assert (per_thread - 1) * words >= st.DOT_FLUSH > (per_thread - 2) * words and n % 2
    assert st.dot_max_grid(eb) == (682 if eb == 24 else 1024)
    assert st.dot_max_grid(eb) * st.word_bytes(eb) <= st.REDUCE_WORKSPACE_BYTES


def test_the_numbers_of_the_workspace_overrun():
    """an uncapped launcher writes 24 bytes per workgroup: past the 16384 bytes of the workspace from grid 683 on, that is from
    682 x 2048 = 1 396 736 iterations, and 8192 bytes past it on the full grid; the guards hold that"""
    assert 682 * 24 <= st.REDUCE_WORKSPACE_BYTES < 683 * 24
    first = min(n for g, d, n in st.dot_grid_edge_sizes(24, False) if n > 682 * 2048)
    assert first == 1396737 and -(-first // 2048) == 683
    assert 1024 * 24 - st.REDUCE_WORKSPACE_BYTES == 8192 <= st.WS_GUARD
    assert st.dot_flush_size(8, True) == 2 * 1024 * 256 * 97 + 1 and st.dot_flush_size(1, True) == 16 * 1024 * 256 * 49 + 15


def test_tall_construction():
    """A = P U at n = 257: in every column one nonzero entry at or below the diagonal, in the last row -- 256 rows down in the
    first column.  (po.gauss_solve and po.gauss_det agree with the construction: the integer context, which computes with them,
    passes these cases in test_gauss_passes_on_the_integer_context.)"""
    case = st.gauss_tall_cases(2**61 - 1, False, (257,))[0]
    sing, reg = case.mats
    for k in range(257):
        assert [i for i in range(k, 257) if reg[i][k]] == [256] if k < 256 else reg[256][256] != 0
    assert case.sols[0] is None and case.dets[0] == 0 and not any(sing[127]) and case.dets[1] != 0


# ---- the honest context passes ---------------------------------------------------------------------------------------------
def run_dot_matrix(drv, sizes=DOT_SIZES):
    for aligned in (True, False) if st.has_unaligned_views(drv.eb) else (True,):
        for n in sizes:
            drv.run_dot(n, aligned, 'tiled')
            drv.run_dot(n, aligned, 'max', same_pointer=False)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_dot_and_sum_pass_on_the_integer_context(modulus, binary):
    drv = driver(CpuFieldContext, modulus, binary)
    run_dot_matrix(drv)
    classes = 2 if st.has_unaligned_views(drv.eb) else 1
    assert drv.cases == classes * len(DOT_SIZES) * (3 + 2)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_gauss_passes_on_the_integer_context(modulus, binary):
    drv = driver(CpuFieldContext, modulus, binary)
    drv.run_gauss_matrix(tall=(modulus, binary) == P61, tall_sizes=(257,), big=(st.GAUSS_ZMAX + 1,))
    wide = sum(len(st.gauss_wide_ncols(n)) for n in st.GAUSS_WIDE_N)
    assert wide == 9 + 11                  # (n = 2: two of the eleven coincide twice)
    assert drv.cases == 7 * 2 + wide + (2 if (modulus, binary) == P61 else 0) + 4 * 2 + 2 + 1 + 5


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_group_matvec_passes_on_the_integer_context(modulus, binary):
    drv = driver(CpuFieldContext, modulus, binary)
    drv.run_group_matrix(dims=(1, 7, 8, 16), ngroups=(0, 1, 2, 65))
    assert drv.cases == 16 * 4 * 3
    drv.run_group_too_large()
    if drv.eb == 1:
        drv.run_group_byte_offsets(ngroups=9)
        assert drv.cases == 16 * 4 * 3 + 3 + 64 * 5


# ---- wrong contexts --------------------------------------------------------------------------------------------------------
class DotIgnoresTheLastPartialBlock(CpuFieldContext):
    """(1) reduces whole workgroups' worth of elements only"""

    def _cut(self, a):
        n = a.n - a.n % st.DOT_BLOCK_ITERS if a.n >= st.DOT_BLOCK_ITERS else a.n
        return DevArray(self, a.t[:n], n)

    def dot(self, a, b):
        return super().dot(self._cut(a), self._cut(b))

    def sum(self, a):
        return super().sum(self._cut(a))


class DotDropsTheScalarTail(DotIgnoresTheLastPartialBlock):
    """(2) the pack loop without the scalar loop behind it"""

    def _cut(self, a):
        per = st.WAVE if self.elem_bytes == 24 else st.elems_per_pack(self.elem_bytes)
        return DevArray(self, a.t[:a.n - a.n % per], a.n - a.n % per)


def kernel_like_gauss(ctx, a, n, ncols, batch, det, pivot_rows=None, col_limit=None):
    """Gauss-Jordan in the kernels' order on Python integers; pivot_rows: the pivot search looks at that many rows only;
    col_limit: the elimination covers that many columns right of the pivot only"""
    F = ctx.F
    vals = a.to_ints()
    flags = torch.zeros(max(batch, 1), dtype=torch.int32)
    dets = []
    for b in range(batch):
        M = [vals[(b * n + i) * ncols:(b * n + i + 1) * ncols] for i in range(n)]
        d = 1
        for k in range(n):
            x = next((i for i in range(k, n if pivot_rows is None else min(n, k + pivot_rows)) if M[i][k]), None)
            if x is None:
                flags[b], d = 1, 0
                break
            M[k], M[x] = M[x], M[k]
            d = po.mul(F, d, M[k][k])
            inv = po.inv(F, M[k][k])
            M[k] = [po.mul(F, v, inv) for v in M[k]]
            hi = ncols if col_limit is None else min(ncols, k + 1 + col_limit)
            for i in range(k + 1 if det else 0, n):
                if i != k and M[i][k]:
                    m = M[i][k]
                    M[i][k + 1:hi] = [po.sub(F, v, po.mul(F, m, r)) for v, r in zip(M[i][k + 1:hi], M[k][k + 1:hi])]
        dets.append(d)
        vals[b * n * ncols:(b + 1) * n * ncols] = [v for row in M for v in row]
    ctx._put(a, vals)
    return (ctx._put(ctx.empty(batch), dets) if det else None), flags


class GaussPivotSearchStopsAfter256Rows(CpuFieldContext):
    """(3) k_gauss_pivot without its stride loop"""

    def gauss(self, a, n, ncols, batch=1, det=False):
        return kernel_like_gauss(self, a, n, ncols, batch, det, pivot_rows=st.BLOCK)


class GaussIgnoresColumnsBeyond256(CpuFieldContext):
    """(4) k_gauss_elim with one column block"""

    def gauss(self, a, n, ncols, batch=1, det=False):
        return kernel_like_gauss(self, a, n, ncols, batch, det, col_limit=st.BLOCK)


class GaussWritesChunkTwoAtOffsetZero(CpuFieldContext):
    """(5) the determinants and flags of the second chunk of 32768 matrices land at the start of det_out / dev_singular"""

    def gauss(self, a, n, ncols, batch=1, det=False):
        d, flags = super().gauss(a, n, ncols, batch, det)
        if batch > st.GAUSS_ZMAX:
            m = batch - st.GAUSS_ZMAX
            flags[:m] = flags[st.GAUSS_ZMAX:batch].clone()
            flags[st.GAUSS_ZMAX:] = 0
            if det:
                d.t[:m] = d.t[st.GAUSS_ZMAX:batch].clone()
                d.t[st.GAUSS_ZMAX:] = 0
        return d, flags


class GaussLeavesFlagsUnsetInSolveMode(CpuFieldContext):
    """(6)"""

    def gauss(self, a, n, ncols, batch=1, det=False):
        d, flags = super().gauss(a, n, ncols, batch, det)
        if not det:
            flags.zero_()
        return d, flags


class GroupMatvecUsesEightColumns(CpuFieldContext):
    """(7) the 8-byte fast path taken for every g"""

    def group_matvec(self, x, matrix, bias=None, out=None):
        return super().group_matvec(x, [[v if c < 8 else 0 for c, v in enumerate(row)] for row in matrix], bias, out)


class WritesPastTheWorkspace(st.CpuAdapter):
    """(8) one partial sum more than FFGPU_REDUCE_WORKSPACE_BYTES holds (the launcher before its grid was bounded by the
    workspace, on 24-byte fields)"""

    def dot(self, buf, a, b, out, ws, n):
        rc = super().dot(buf, a, b, out, ws, n)
        if n:
            buf[ws + st.REDUCE_WORKSPACE_BYTES:ws + st.REDUCE_WORKSPACE_BYTES + 24] = 0
        return rc


class WritesTheWorkspaceOfAnEmptySum(st.CpuAdapter):
    """(9) n = 0 must leave the workspace alone"""

    def dot(self, buf, a, b, out, ws, n):
        buf[ws:ws + 8] = 0
        return super().dot(buf, a, b, out, ws, n)


def dot_sizes(*sizes):
    def run(drv):
        run_dot_matrix(drv, sizes)
    return run


def wide(drv):
    for case in st.gauss_wide_cases(drv.modulus, drv.binary):
        drv.run_gauss(case, 0)


def tall(drv):
    for case in st.gauss_tall_cases(drv.modulus, drv.binary, (257,)):
        drv.run_gauss(case, 0)


def chunked(mode):
    def run(drv):
        pool = st.gauss_pool(drv.modulus, drv.binary, 2, 0 if mode else 1)
        batch = st.GAUSS_ZMAX + 3               # three matrices in chunk two, the first of them singular
        drv.run_gauss(None, mode, pool.indices(batch, st.big_batch_singular_at(batch)), pool)
    return run


def batches(drv):
    pool = st.gauss_pool(drv.modulus, drv.binary, 3, 2)
    for batch, at in st.GAUSS_BATCHES:
        drv.run_gauss(None, 0, pool.indices(batch, at), pool)


def groups(drv):
    drv.run_group_matrix(dims=(7, 8, 15), ngroups=(2, 65))


# (context, adapter, the part of the matrix meant to catch it, kind of violation, words of its message, fields)
WRONG = [
    (DotIgnoresTheLastPartialBlock, st.CpuAdapter, dot_sizes(2047, 2048), None, '', FIELDS),           # whole blocks: it passes
    (DotIgnoresTheLastPartialBlock, st.CpuAdapter, dot_sizes(2047, 2048, 2049), 'out', '2049', FIELDS),
    (DotDropsTheScalarTail, st.CpuAdapter, dot_sizes(0, 64, 2048), None, '', [P61, P136, GF256]),          # no tail: it passes
    (DotDropsTheScalarTail, st.CpuAdapter, dot_sizes(64, 65), 'out', '65', [P61, P136, GF256]),
    (GaussPivotSearchStopsAfter256Rows, st.CpuAdapter, tall, 'out', 'tall n=257', [P61]),
    (GaussIgnoresColumnsBeyond256, st.CpuAdapter, wide, 'out', 'ncols=258', [P61, GF256]),
    (GaussWritesChunkTwoAtOffsetZero, st.CpuAdapter, chunked(0), 'out', 'dev_singular', [P61]),
    (GaussWritesChunkTwoAtOffsetZero, st.CpuAdapter, chunked(1), 'out', 'det_out', [P61]),
    (GaussLeavesFlagsUnsetInSolveMode, st.CpuAdapter, batches, 'out', 'dev_singular', [P61, GF256]),
    (GroupMatvecUsesEightColumns, st.CpuAdapter, groups, 'out', '15', [P61, P136, GF256]),
    (CpuFieldContext, WritesPastTheWorkspace, dot_sizes(0, 1), 'guard', 'guard byte', [P136]),
    (CpuFieldContext, WritesTheWorkspaceOfAnEmptySum, dot_sizes(0), 'out', 'workspace', [P61]),
]


@pytest.mark.parametrize('cls,adapter,part,kind,words,fields', WRONG,
                         ids=['%s-%s-%s' % (c.__name__, a.__name__, k) for c, a, _, k, _, _ in WRONG])
def test_driver_fails_on_a_wrong_context(cls, adapter, part, kind, words, fields):
    for modulus, binary in fields:
        drv = driver(cls, modulus, binary, adapter)
        if kind is None:
            part(drv)
            continue
        with pytest.raises(ContractViolation) as err:
            part(drv)
        assert kind in err.value.kinds and words in str(err.value), (cls.__name__, hex(modulus), str(err.value))
        good = driver(CpuFieldContext, modulus, binary)          # and the same part passes on the honest context
        part(good)
        assert good.cases > drv.cases
