"""ffgpu_dot / ffgpu_sum, ffgpu_gauss and ffgpu_group_matvec at the sizes where their launchers change shape, on every field
policy, byte for byte against Python integers and oracle/pyoracle, through the C ABI on views between guards.

dot / sum: the small sizes; iters = 2048 g + delta around every grid g in 1, 2, 682, 683, 1023, 1024, 1025 (2048 = BLOCK x 8
iterations per workgroup; 682 = FFGPU_REDUCE_WORKSPACE_BYTES // 24, 1024 = DOT_MAX_BLOCKS), on aligned views (iterations are
packs) and on views one element in (iterations are elements); 3 x 1024 x 2048 iterations, where every thread loops; and, on
one modulus per accumulator type, the flush edge: grid x BLOCK x (192 words + one iteration) -- 5.0e7 elements of 8 to 16
bytes, 2.0e8 of GF(2^8), 3.4e7 of 24 bytes.  Periodic data with edge values and the all-(q - 1) worst case of the lazy
accumulator; dot(a, a) on one pointer; the workspace a view of exactly FFGPU_REDUCE_WORKSPACE_BYTES between guards; n = 0.

gauss: the matrix kinds of the goldens at n up to 17 in both modes; two and three column blocks of k_gauss_elim; pivots 256
and more rows below the diagonal (k_gauss_pivot's stride loop); batches in solve mode with singular systems first, in the
middle and last; the 32768-matrix chunks of the launcher with singular systems on both sides of the seam; batch = 0, n = 0,
no right-hand side; guards around the matrices, det_out and dev_singular.

group_matvec: (r, g) in {1, 2, 7, 8, 15, 16}^2, 0 to 1025 groups, random and all-(q - 1) matrices; GF(2^8) at every byte
offset of `in` and `out`; r or g = 17.

The case logic, the references and the layouts are tests/second_tier_contract.py; tests/test_second_tier_contract_host.py shows
that driver fails when it should.  Expected values never come from the library."""
import numpy as np
import pytest

import ew_contract as ew
import second_tier_contract as st
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def ids_of(fields):
    return [('gf2:' if b else '') + hex(m) for m, b in fields]


FIELDS = ew.contract_fields()
MONT192 = (2**135 + 4823, False)                # a 24-byte prime of no special shape: the second policy with 24-byte words
DOT_FIELDS = FIELDS + [MONT192]
# one modulus per accumulator type (F::acc, fields.hpp): PM64, RC64, RC32, PM128, MONT128, PM192, MONT192, GF2P8, GF2W32,
# GF2W64, GF2W128
FLUSH_FIELDS = [(2**61 - 1, False), (6616326157076047771, False), (2**31 - 1, False), (2**128 - 173, False),
                (2**127 + 2**100 + 0x101, False), (2**136 - 113, False), MONT192, (0x11b, True), (0x10000008d, True),
                (0x1000000000000001b, True), (0x100000000000000000000000000000087, True)]
# one prime per element width (8, 12, 16, 24 bytes) and GF(2^8), GF(2^32): the tall systems are built on the host
TALL_FIELDS = [(2**61 - 1, False), (2**96 - 17, False), (2**128 - 173, False), (2**136 - 113, False), (0x11b, True)]
TALL_257_ONLY = [(0x10000008d, True)]

_ctxs = {}


def default_ctx(modulus, binary):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from mpyc_amd import engine
    if (modulus, binary) not in _ctxs:
        _ctxs[modulus, binary] = engine.FieldContext(modulus, binary, device=0)
    return _ctxs[modulus, binary]


def driver(modulus, binary):
    ctx = default_ctx(modulus, binary)
    assert ctx.order == po.Field(modulus, binary).order
    return st.Driver(st.GpuAdapter(ctx), modulus, binary)


def alignments(eb):
    return (True, False) if st.has_unaligned_views(eb) else (True,)


def test_constants_restated():
    """what the driver restates, against what the library and the engine say"""
    from mpyc_amd import engine
    ctx = default_ctx(2**61 - 1, False)
    assert engine.FieldContext._workspace(ctx).numel() == st.REDUCE_WORKSPACE_BYTES
    assert sorted({st.elem_bytes(m, b) for m, b in DOT_FIELDS}) == [1, 4, 8, 12, 16, 24]
    assert {default_ctx(m, b).reduction for m, b in ((2**136 - 113, False), MONT192)} == {'pseudo-mersenne', 'montgomery'}


# ---- dot / sum ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', DOT_FIELDS, ids=ids_of(DOT_FIELDS))
def test_dot_and_sum_small_sizes(modulus, binary):
    drv = driver(modulus, binary)
    for aligned in alignments(drv.eb):
        for n in st.DOT_SMALL:
            drv.run_dot(n, aligned, 'tiled')
            drv.run_dot(n, aligned, 'max', same_pointer=False)
    assert drv.cases == len(alignments(drv.eb)) * len(st.DOT_SMALL) * 5
    print('largest tensor: %d bytes' % drv.max_bytes)


@pytest.mark.parametrize('modulus,binary', DOT_FIELDS, ids=ids_of(DOT_FIELDS))
def test_dot_and_sum_at_the_grid_edges(modulus, binary):
    """also the test of the workspace bound: on 24-byte fields the grids 683 to 1024 would write up to 8192 bytes past the
    workspace, into the guard behind it"""
    drv = driver(modulus, binary)
    eb = drv.eb
    for aligned in alignments(eb):
        sizes = st.dot_grid_edge_sizes(eb, aligned)
        assert [g for g, d, n in sizes if d == 0] == list(st.DOT_GRIDS)
        for g, d, n in sizes:
            assert st.dot_grid(eb, n, aligned) == min(g + (d > 0), st.dot_max_grid(eb))
            drv.run_dot(n, aligned, 'tiled')                       # dot(a, b), sum(a), dot(a, a)
            drv.run_dot(n, aligned, 'max', same_pointer=False)
        drv.run_dot(st.dot_loop_size(eb, aligned), aligned, 'tiled')
    assert drv.cases == len(alignments(eb)) * (21 * 5 + 3)
    print('largest tensor: %d bytes; sizes %r' % (drv.max_bytes, [n for _, _, n in st.dot_grid_edge_sizes(eb, True)]))


@pytest.mark.parametrize('modulus,binary', FLUSH_FIELDS, ids=ids_of(FLUSH_FIELDS))
def test_dot_and_sum_at_the_flush_edge(modulus, binary):
    """every thread of the saturated grid flushes its lazy accumulator once and accumulates again -- in the pack loop on
    aligned views, in the scalar loop (`++cnt >= 192`) on views one element in; all elements q - 1 is the most the accumulator
    holds between two flushes"""
    drv = driver(modulus, binary)
    for aligned in alignments(drv.eb):
        n = st.dot_flush_size(drv.eb, aligned)
        drv.run_dot(n, aligned, 'tiled', same_pointer=False)
        drv.run_dot(n, aligned, 'max', same_pointer=False)
        print('n = %d (%s)' % (n, 'aligned' if aligned else 'one element in'))
    assert drv.cases == len(alignments(drv.eb)) * 4
    print('largest tensor: %d bytes' % drv.max_bytes)


# ---- gauss -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_gauss_small_wide_and_batched(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_gauss_matrix()
    wide = sum(len(st.gauss_wide_ncols(n)) for n in st.GAUSS_WIDE_N)
    assert drv.cases == 7 * 2 + wide + 4 * 2 + 4 * 2 + 1 + 5
    assert all(('gauss', 'pool n=2 ncols=%d batch=%d' % (2 + (1 - mode), b), mode) in drv.seen
               for b in (32767, 32768, 32769, 65537) for mode in (0, 1))
    print('largest tensor: %d bytes' % drv.max_bytes)


@pytest.mark.parametrize('modulus,binary', TALL_FIELDS + TALL_257_ONLY, ids=ids_of(TALL_FIELDS + TALL_257_ONLY))
def test_gauss_pivots_far_below_the_diagonal(modulus, binary):
    """A = P U (second_tier_contract.tall_system): in column k the pivot sits n - 1 - k rows down, 256 and more for the first
    columns; a singular variant rides in the same batch"""
    drv = driver(modulus, binary)
    sizes = (257,) if (modulus, binary) in TALL_257_ONLY else st.GAUSS_TALL_N
    for case in st.gauss_tall_cases(modulus, binary, sizes):
        for mode in (0, 1):
            drv.run_gauss(case, mode)
    assert drv.cases == 2 * len(sizes)
    print('largest tensor: %d bytes' % drv.max_bytes)


def test_gauss_argument_checks():
    """det_out = NULL in det mode stays FFGPU_EINVAL, and writes nothing"""
    ctx = default_ctx(2**61 - 1, False)
    buf = torch.full((4096,), st.GUARD_BYTE, dtype=torch.uint8, device=ctx.torch_device)
    ad = st.GpuAdapter(ctx)
    assert ad.gauss(buf, 1024, 2, 2, 1, 1, None, 2048) == st.EINVAL
    assert ad.gauss(buf, 1024, 2, 2, 1, 0, None, None) == st.EINVAL
    assert ad.gauss(buf, 1024, 3, 2, 1, 0, None, 2048) == st.EINVAL
    torch.cuda.synchronize()
    assert bool((buf == st.GUARD_BYTE).all())


def test_gauss_through_the_mirror():
    """np.linalg.det of a stack of more than 32768 matrices and np.linalg.solve with 300 right-hand sides, against the same
    references"""
    assert torch.cuda.is_available()
    from mpyc_amd import finfields
    p = 2**61 - 1
    F, G = po.Field(p, False), finfields.GF(p)
    pool = st.gauss_pool(p, False, 2, 0)
    batch = st.GAUSS_ZMAX + 5
    idx = pool.indices(batch, st.big_batch_singular_at(batch))
    dets = np.linalg.det(G.array([pool.mats[i] for i in idx]))
    assert dets.shape == (batch,) and [int(v) for v in dets.value] == [pool.dets[i] for i in idx]
    case = [c for c in st.gauss_wide_cases(p, False) if c.n == 5 and c.ncols == 5 + 2 * st.BLOCK][0]
    A, B = [r[:5] for r in case.mats[0]], [r[5:] for r in case.mats[0]]
    B = [row[:300] for row in B]
    x = np.linalg.solve(G.array(A), G.array(B))
    assert x.shape == (5, 300) and [[int(v) for v in row] for row in x.value] == [row[:300] for row in case.sols[0]]


# ---- group_matvec ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_group_matvec_every_shape(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_group_matrix()
    assert drv.cases == 36 * 7 * 3
    assert all(('group', 'max+bias', 16, 16, n, 0, 0) in drv.seen for n in st.GM_NGROUPS)
    drv.run_group_too_large()
    assert drv.cases == 36 * 7 * 3 + 3
    print('largest tensor: %d bytes' % drv.max_bytes)


def test_group_matvec_at_every_byte_offset():
    """GF(2^8): the two 8-byte fast paths and the general kernel must agree with the reference wherever `in` and `out` start"""
    drv = driver(0x11b, True)
    drv.run_group_byte_offsets()
    assert drv.cases == 64 * 5
