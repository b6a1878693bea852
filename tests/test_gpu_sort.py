"""The two ends of a compare-exchange stage of the sorting network on the device (ffgpu_cx_diff / ffgpu_cx_apply,
mpyc_amd/csrc/sort.hpp) against Python integers computed here from the maps include/ffgpu.h states, over every prime
policy, every stage of several k and four (outer, inner); shapes that reach the pack paths, views at odd element offsets
and a capped grid; guard bytes around the outputs and the positions cx_apply must not touch; status codes; the same bytes
as index_select / sub / recombine / add / sub / index_copy_ composed; protocols.sort end to end for all parties on one GPU;
one stage replayed from a captured HIP graph; two and nine rows, the edges of the launcher's row dispatch, on both paths."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_sgn import FIELDS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

KS = (2, 3, 5, 8, 13, 64, 65, 257)
SHAPES = ((1, 1), (3, 1), (1, 3), (2, 64))             # (outer, inner)
NROWS = (1, 3, 7)


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def stages(k):
    """the reference's loop (runtime.py:1759-1772) with the index set of every stage, by enumeration"""
    out = []
    t = (k - 1).bit_length()
    p = 1 << t - 1
    while p:
        d, q, r = p, 1 << t - 1, 0
        while d:
            i = np.arange(k - d)
            out.append((p, d, r, i[(i & p) == r]))
            d, q, r = q - p, q >> 1, p
        p >>= 1
    return out


def draw(rng, p, count):
    """uniform field elements (200 random bits mod p) as an object array, built inside NumPy's loops"""
    w = rng.integers(0, 2**64, size=(3, count), dtype=np.uint64).astype(object)
    return ((w[0] << 136) ^ (w[1] << 64) ^ w[2]) % p


def diff_ref(p, A, I, d):
    """A: (outer, k, inner) objects -> compact (outer, P, inner)"""
    return (A[:, I + d, :] - A[:, I, :]) % p


def apply_ref(p, A, I, d, rows, lam):
    """rows: nrows flat compact arrays; the new A"""
    outer, _, inner = A.shape
    h = sum(l * r for l, r in zip(lam, rows)) % p
    h = h.reshape(outer, len(I), inner)
    B = A.copy()
    B[:, I, :] = (A[:, I, :] + h) % p
    B[:, I + d, :] = (A[:, I + d, :] - h) % p
    return B


def view(engine, ctx, x, lo, n):
    return engine.DevArray(ctx, x.t[lo:lo + n], n)


def same(x, want):
    return bool(torch.equal(x.t.reshape(-1), want.t.reshape(-1)))


def edges(A, p):
    flat = A.reshape(-1)
    e = [0, p - 1, 1, p - 2]
    flat[:min(len(e), len(flat))] = e[:len(flat)]
    return A


def run_shape(engine, ctx, p, rng, outer, k, inner, stage_list, offset=0, nrows_of=lambda s: NROWS[s % 3]):
    """every listed stage of one (outer, k, inner): expectations from Python integers, uploaded once for the whole
    list; `a`, the rows and `out` are views `offset` elements into their buffers"""
    n = outer * k * inner
    A = edges(draw(rng, p, n), p).reshape(outer, k, inner)
    pmax = max(len(I) for _, _, _, I in stage_list) * outer * inner
    row_counts = [nrows_of(s) for s in range(len(stage_list))]
    R = [edges(draw(rng, p, pmax), p) for _ in range(max(NROWS + tuple(row_counts)))]
    want_d, want_a, lams = [], [], []
    for s, (_, d, _, I) in enumerate(stage_list):
        c = outer * len(I) * inner
        nr = row_counts[s]
        lam = [int(v) for v in draw(rng, p, nr)]
        lams.append(lam)
        want_d.append(diff_ref(p, A, I, d).reshape(-1))
        want_a.append(apply_ref(p, A, I, d, [r[:c] for r in R[:nr]], lam).reshape(-1))
    WD, WA = ctx.from_ints(np.concatenate(want_d)), ctx.from_ints(np.concatenate(want_a))
    a0 = ctx.from_ints(A.reshape(-1))
    buf = ctx.empty(n + offset)
    a = view(engine, ctx, buf, offset, n)
    rbuf = [ctx.empty(pmax + offset) for _ in R]
    for b, r in zip(rbuf, R):
        b.t[offset:].copy_(ctx.from_ints(r).t)
    obuf = ctx.empty(pmax + offset)
    at = 0
    for s, (ps, d, r, I) in enumerate(stage_list):
        c = outer * len(I) * inner
        assert ctx.cx_pairs(k, ps, d, r) == len(I)
        a.t.copy_(a0.t)
        out = ctx.cx_diff(a, outer, k, inner, ps, d, r, out=view(engine, ctx, obuf, offset, c))
        assert same(out, view(engine, ctx, WD, at, c)), ('diff', outer, k, inner, ps, d, r)
        assert same(a, a0), ('diff wrote a', outer, k, inner, ps, d, r)
        nr = len(lams[s])
        got = ctx.cx_apply(a, [view(engine, ctx, b, offset, c) for b in rbuf[:nr]], lams[s], outer, k, inner, ps, d, r)
        assert got is a and same(a, view(engine, ctx, WA, s * n, n)), ('apply', outer, k, inner, ps, d, r, nr)
        at += c
    for b, r in zip(rbuf, R):
        assert same(view(engine, ctx, b, offset, pmax), ctx.from_ints(r)), 'a row was written'
    return len(stage_list)


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(len(name) * 1000 + p % 997)
    ran = 0
    for k in KS:
        for outer, inner in SHAPES:
            ran += run_shape(engine, ctx, p, rng, outer, k, inner, stages(k))
    assert ran == 4 * sum(len(stages(k)) for k in KS)


@pytest.mark.parametrize('name', list(FIELDS))
def test_shapes_that_reach_the_pack_paths(mods, name):
    """k = 4096, inner = 1: runs from 1 to 2048 elements, so every stage class of every pack size (and whole waves of
    24-byte elements from p = 64 on); (2, 96, 64): runs of whole waves with a k that is no power of two"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(7 + p % 997)
    assert run_shape(engine, ctx, p, rng, 1, 4096, 1, stages(4096)) == 78
    assert run_shape(engine, ctx, p, rng, 2, 96, 64, stages(96)) == len(stages(96))


def pick_stages(k):
    """a long run, a short run with d == p and a short run with a large d"""
    st = stages(k)
    return [st[0], [s for s in st if s[0] == 1 and s[2] == 0][0], max((s for s in st if s[0] == 1), key=lambda s: s[1]),
            [s for s in st if s[0] == 64 and s[2] == 64][0]]


@pytest.mark.parametrize('name', ['pm64-k64', 'pm96', 'pm192'])
def test_views_at_odd_element_offsets_and_capped_grid(mods, monkeypatch, name):
    """8-, 12- and 24-byte storage: `a`, the rows and `out` one element into their buffers (8- and 24-byte elements are
    then not 16-byte aligned: the element path), and the same with FFGPU_BLOCKS_PER_CU=1, where every thread of the
    loop takes several units -- aligned (packs, whole waves) and at the odd offset"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    rng = np.random.default_rng(11 + p % 997)
    ctx = engine.FieldContext(p, device=0)
    for outer, k, inner in ((3, 13, 1), (2, 96, 64), (1, 257, 3)):
        run_shape(engine, ctx, p, rng, outer, k, inner, stages(k), offset=1)
    monkeypatch.setenv('FFGPU_BLOCKS_PER_CU', '1')
    capped = engine.FieldContext(p, device=0)
    monkeypatch.delenv('FFGPU_BLOCKS_PER_CU')
    outer, k, inner = 5, 1024, 64
    threads = torch.cuda.get_device_properties(0).multi_processor_count * 256
    assert outer * (k // 2) * inner // 2 > threads           # more packs of 8-byte elements than threads in the grid
    for offset in (0, 1):
        run_shape(engine, capped, p, rng, outer, k, inner, pick_stages(k), offset=offset, nrows_of=lambda s: (3, 7, 1, 3)[s])


@pytest.mark.parametrize('name', ['pm64-k64', 'pm128', 'pm192'])
def test_two_and_nine_rows_on_both_paths(mods, name):
    """NROWS stops at seven; the launcher dispatches over 1 .. 9 rows, so both edges next to the ends: every stage of
    k = 3 with two and with nine rows over 8-, 16- and 24-byte storage.  (2, 3, 64): the pack path (whole waves of 24-byte
    elements); (1, 3, 3) and (2, 3, 64) one element into the buffers: the element path of 8- and 24-byte elements (a pack
    of 16-byte elements is one element, aligned at every element offset: they stay on the pack path)"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(29 + p % 997)
    for outer, k, inner, offset in ((2, 3, 64, 0), (1, 3, 3, 0), (2, 3, 64, 1)):
        for nr in (2, 9):
            assert run_shape(engine, ctx, p, rng, outer, k, inner, stages(k), offset=offset, nrows_of=lambda s: nr) == 3


@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
def test_nothing_is_written_outside_the_outputs(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    pad = 240                                              # a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    eb = ctx.elem_bytes
    rng = np.random.default_rng(13 + p % 997)
    L, h, st = ctx._L, ctx._h, ctx._stream()

    def guarded(x):
        """a copy of x between two pads of 0xa5: (buffer, pointer of the copy)"""
        raw = x.t.contiguous().view(torch.uint8).reshape(-1)
        buf = torch.full((pad + raw.numel() + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        buf[pad:pad + raw.numel()] = raw
        return buf, buf.data_ptr() + pad

    def check(buf, want):
        raw = want.t.contiguous().view(torch.uint8).reshape(-1)
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + raw.numel():] == 0xa5).all()), 'guard bytes written'
        assert torch.equal(buf[pad:pad + raw.numel()], raw)

    for outer, k, inner in ((3, 13, 1), (2, 96, 64), (1, 130, 2)):
        n = outer * k * inner
        A = draw(rng, p, n).reshape(outer, k, inner)
        a0 = ctx.from_ints(A.reshape(-1))
        for ps, d, r, I in stages(k):
            c = outer * len(I) * inner
            rows = [draw(rng, p, c) for _ in range(3)]
            lam = [int(v) for v in draw(rng, p, 3)]
            drows = [ctx.from_ints(x) for x in rows]
            keep = [x.t.clone() for x in drows]
            bo, po = guarded(ctx.from_ints([0] * c))
            assert L.ffgpu_cx_diff(h, a0.ptr, po, outer, k, inner, ps, d, r, st) == _ffi.OK
            check(bo, ctx.from_ints(diff_ref(p, A, I, d).reshape(-1)))
            ba, pa = guarded(a0)
            ptrs = (ctypes.c_void_p * 3)(*[x.ptr for x in drows])
            assert L.ffgpu_cx_apply(h, pa, ptrs, ctx._scalars(lam), 3, outer, k, inner, ps, d, r, st) == _ffi.OK
            # the whole array: positions outside I and I + d keep their bytes
            check(ba, ctx.from_ints(apply_ref(p, A, I, d, rows, lam).reshape(-1)))
            for x, t in zip(drows, keep):
                assert torch.equal(x.t, t), 'a row was written'
        assert same(a0, ctx.from_ints(A.reshape(-1))), 'cx_diff wrote its input'
    assert eb in (4, 8, 12, 16, 24)


def test_status_codes(mods):
    import ctypes
    _ffi, engine, _, _ = mods
    p = 2**61 - 1
    ctx = engine.FieldContext(p, device=0)
    L, h, st = ctx._L, ctx._h, ctx._stream()
    outer, k, inner = 2, 13, 3
    n = outer * k * inner
    pat = lambda cnt, v: torch.full((cnt * ctx.elem_bytes,), v, dtype=torch.uint8, device='cuda')
    A, O, R = pat(n, 0x5a), pat(n, 0x3c), pat(n, 0x77)
    a, o, rw = A.data_ptr(), O.data_ptr(), R.data_ptr()
    rows = (ctypes.c_void_p * 12)(*([rw] * 12))
    lam = ctx._scalars([1] * 12)
    EINVAL, OK = _ffi.EINVAL, _ffi.OK
    diff = lambda *s, a_=a, o_=o, shape=(outer, k, inner): L.ffgpu_cx_diff(h, a_, o_, *shape, *s, st)
    appl = lambda *s, a_=a, rows_=rows, lam_=lam, nr=3, shape=(outer, k, inner): L.ffgpu_cx_apply(h, a_, rows_, lam_, nr, *shape, *s, st)
    assert diff(4, 4, 0) == OK and appl(4, 4, 0) == OK                      # (a valid call, for contrast)
    torch.cuda.synchronize()
    A.fill_(0x5a), O.fill_(0x3c)
    # a null context or pointer
    assert L.ffgpu_cx_diff(None, a, o, outer, k, inner, 4, 4, 0, st) == EINVAL
    assert L.ffgpu_cx_apply(None, a, rows, lam, 3, outer, k, inner, 4, 4, 0, st) == EINVAL
    assert diff(4, 4, 0, a_=None) == EINVAL and diff(4, 4, 0, o_=None) == EINVAL
    assert appl(4, 4, 0, a_=None) == EINVAL and appl(4, 4, 0, rows_=None) == EINVAL and appl(4, 4, 0, lam_=None) == EINVAL
    assert appl(4, 4, 0, rows_=(ctypes.c_void_p * 3)(rw, None, rw)) == EINVAL
    # k < 2
    assert diff(1, 1, 0, shape=(outer, 1, inner)) == EINVAL and appl(1, 1, 0, shape=(outer, 1, inner)) == EINVAL
    assert diff(1, 1, 0, shape=(outer, 0, inner)) == EINVAL
    # not a stage: p not a power of two, d of neither form, r not in {0, p}
    for bad in ((3, 3, 0), (0, 0, 0), (6, 2, 6), (4, 3, 0), (4, 8, 0), (2, 4, 2), (2, 2 ** 64 - 2, 2), (2, 0, 2), (4, 4, 1),
                (4, 4, 2), (2, 6, 4), (2, 2, 1)):
        assert diff(*bad) == EINVAL and appl(*bad) == EINVAL, bad
    # nrows
    assert appl(4, 4, 0, nr=0) == EINVAL and appl(4, 4, 0, nr=-1) == EINVAL
    assert appl(4, 4, 0, nr=9) == OK
    assert appl(4, 4, 0, nr=10) == _ffi.ENOTSUP and appl(4, 4, 0, nr=12) == _ffi.ENOTSUP
    big = (ctypes.c_void_p * 65)(*([rw] * 65))                              # what ffgpu_recombine says to too many rows
    assert L.ffgpu_recombine(h, big, ctx._scalars([1] * 65), 65, 1, o, n, n, st) == _ffi.ENOTSUP
    torch.cuda.synchronize()
    A.fill_(0x5a)
    # sizes whose byte count overflows
    assert diff(4, 4, 0, shape=(1 << 40, 13, 1 << 21)) == EINVAL and appl(4, 4, 0, shape=(1 << 40, 13, 1 << 21)) == EINVAL
    assert diff(4, 4, 0, shape=(1 << 62, 13, 4)) == EINVAL and diff(4, 4, 0, shape=(1, 1 << 61, 1)) == EINVAL
    # overlap: out inside a, a row inside a, a row that ends where a starts (allowed)
    eb = ctx.elem_bytes
    assert diff(4, 4, 0, o_=a) == EINVAL and diff(4, 4, 0, o_=a + (n - 1) * eb) == EINVAL
    assert appl(4, 4, 0, rows_=(ctypes.c_void_p * 3)(rw, a + 8, rw)) == EINVAL
    assert appl(4, 4, 0, rows_=(ctypes.c_void_p * 3)(a, rw, rw)) == EINVAL
    torch.cuda.synchronize()
    assert bool((A == 0x5a).all()) and bool((O == 0x3c).all()) and bool((R == 0x77).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    assert diff(4, 4, 0, shape=(0, k, inner), a_=None, o_=None) == OK and diff(4, 4, 0, shape=(outer, k, 0)) == OK
    assert appl(4, 4, 0, shape=(0, k, inner), a_=None, rows_=None) == OK and appl(4, 4, 0, shape=(outer, k, 0)) == OK
    assert L.ffgpu_cx_pairs(4, 2, 2, 2) == 0 and L.ffgpu_cx_pairs(13, 8, 24, 8) == 0
    assert diff(2, 2, 2, shape=(outer, 4, inner), a_=None, o_=None) == OK                 # a stage with no pair
    assert appl(8, 24, 8, a_=None, rows_=None) == OK                                        # d past the array
    torch.cuda.synchronize()
    assert bool((A == 0x5a).all()) and bool((O == 0x3c).all())
    # the pair count against brute force, valid stages and near misses
    for kk in (2, 3, 5, 8, 13, 64, 65, 257, 4096):
        for ps, d, r, I in stages(kk):
            assert L.ffgpu_cx_pairs(kk, ps, d, r) == len(I) == ctx.cx_pairs(kk, ps, d, r)
            assert L.ffgpu_cx_pairs(kk, ps * 3, d, r) == 0 and L.ffgpu_cx_pairs(kk, ps, d + 1, r) == 0
    # binary fields
    for mod in (0x11b, (1 << 64) | 0x1b):
        bctx = engine.FieldContext(mod, True, device=0)
        g = torch.zeros(4096, dtype=torch.uint8, device='cuda').data_ptr()
        assert bctx._L.ffgpu_cx_diff(bctx._h, g, g + 2048, 1, 8, 1, 4, 4, 0, st) == _ffi.ENOTSUP
        assert bctx._L.ffgpu_cx_apply(bctx._h, g, (ctypes.c_void_p * 1)(g + 2048), bctx._scalars([1]), 1, 1, 8, 1, 4, 4, 0,
                                      st) == _ffi.ENOTSUP
    # the engine's own checks
    x = ctx.from_ints(list(range(n)))
    with pytest.raises(ValueError):
        ctx.cx_diff(x, outer, k + 1, inner, 4, 4, 0)
    with pytest.raises(ValueError):
        ctx.cx_diff(x, outer, k, inner, 4, 4, 0, out=ctx.empty(5))
    with pytest.raises(ValueError):
        ctx.cx_diff(x, outer, k, inner, 3, 3, 0)
    with pytest.raises(ValueError):
        ctx.cx_apply(x, [ctx.empty(5)], [1], outer, k, inner, 4, 4, 0)
    with pytest.raises(ValueError):
        ctx.cx_apply(x, [], [], outer, k, inner, 4, 4, 0)
    with pytest.raises(ValueError):
        ctx.cx_diff(x, 0, k, inner, 4, 4, 0)


@pytest.mark.parametrize('modulus', [2**61 - 1, 2**80 - 65, 2**136 - 113], ids=['2^61-1', '2^80-65', '2^136-113'])
@pytest.mark.parametrize('k,inner', [(257, 1), (64, 5)])
def test_same_bytes_as_the_composition_of_existing_calls(mods, modulus, k, inner):
    """every stage: the gathers, the difference, the recombination, b0 + h, b1 - h and the scatters from index_select,
    ffgpu_sub, ffgpu_recombine, ffgpu_add, ffgpu_sub and index_copy_ give the bytes of the two kernels"""
    _ffi, engine, _, _ = mods
    ctx = engine.FieldContext(modulus, device=0)
    rng = np.random.default_rng(k + inner)
    outer, nr = 2, 3
    n = outer * k * inner
    a0 = ctx.from_ints(draw(rng, modulus, n))
    lam = [int(v) for v in draw(rng, modulus, nr)]
    rowbuf = [ctx.from_ints(draw(rng, modulus, outer * (k // 2) * inner)) for _ in range(nr)]
    tail = tuple(a0.t.shape[1:])
    for ps, d, r, I in stages(k):
        c = outer * len(I) * inner
        lo = torch.as_tensor(I, device='cuda')
        cube = lambda x: x.t.reshape((outer, k, inner) + tail)
        flat = lambda t: engine.DevArray(ctx, t.contiguous().reshape((c,) + tail), c)
        b0, b1 = flat(cube(a0).index_select(1, lo)), flat(cube(a0).index_select(1, lo + d))
        want_diff = ctx.sub(b1, b0)
        rows = [view(engine, ctx, x, 0, c) for x in rowbuf]
        hh = ctx.recombine(rows, lam)
        n0, n1 = ctx.add(b0, hh), ctx.sub(b1, hh)
        want = a0.clone()
        wc = cube(want)
        wc.index_copy_(1, lo, n0.t.reshape((outer, len(I), inner) + tail))
        wc.index_copy_(1, lo + d, n1.t.reshape((outer, len(I), inner) + tail))
        a = a0.clone()
        assert same(ctx.cx_diff(a, outer, k, inner, ps, d, r), want_diff), (ps, d, r)
        assert same(ctx.cx_apply(a, rows, lam, outer, k, inner, ps, d, r), want), (ps, d, r)


@pytest.mark.parametrize('modulus,l', [(2**61 - 1, 16), (2**64 - 189, 32)], ids=['2^61-1', '2^64-189'])
@pytest.mark.parametrize('m,t', [(3, 1), (7, 3)])
@pytest.mark.parametrize('shape', [(1, 65, 1), (2, 13, 3)], ids=['1x65x1', '2x13x3'])
def test_sort_end_to_end(mods, modulus, l, m, t, shape):
    _ffi, engine, finfields, protocols = mods
    from oracle import pyoracle as po
    F = finfields.GF(modulus)
    ctx = engine.FieldContext(modulus, device=0)
    rng = random.Random(l * 100 + m + shape[1])
    outer, k, inner = shape
    n = outer * k * inner
    lo, hi = -(1 << (l - 2)), (1 << (l - 2)) - 1           # l-1 signed bits: every difference fits l
    vals = [lo, hi, 0, hi, lo, -1, 0, 1] + [rng.randint(lo, hi) for _ in range(n - 8)]
    rng.shuffle(vals)
    plain = np.array(vals, dtype=np.int64).reshape(shape)
    sh = lambda v: protocols.share(ctx, ctx.from_ints([x % modulus for x in v]), t, m)
    xs = sh(vals)
    before = [x.t.clone() for x in xs]

    def rand(count):
        return (sh([rng.randrange(2) for _ in range(count * l)]), sh([rng.randrange(2) for _ in range(count)]),
                sh([rng.randrange(1 << 24) for _ in range(count)]), sh([rng.randrange(1, modulus) for _ in range(count)]))

    out = protocols.sort(ctx, F, xs, outer, k, inner, t, l, rand)
    assert len(out) == m and all(torch.equal(x.t, b) for x, b in zip(xs, before))
    want = np.sort(plain, axis=1).reshape(-1).tolist()
    signed = lambda v: v - modulus if v > modulus // 2 else v
    for pick in (list(range(t + 1)), sorted(rng.sample(range(m), t + 1)), list(range(m - t - 1, m))):
        lam = [int(v) for v in po.recombination_vector(po.Field(modulus, False), [i + 1 for i in pick], 0)]
        assert [signed(v) for v in ctx.recombine([out[i] for i in pick], lam).to_ints()] == want, pick
    with pytest.raises(ValueError):
        protocols.sort(ctx, F, xs[:2 * t], outer, k, inner, t, l, rand)
    with pytest.raises(ValueError):
        protocols.sort(ctx, F, xs, outer, k + 1, inner, t, l, rand)


def test_graph_capture_replays_one_stage(mods):
    _ffi, engine, _, _ = mods
    p = 2**64 - 189
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(21)
    outer, k, inner = 2, 96, 64
    ps, d, r, I = stages(k)[3]
    n, c = outer * k * inner, outer * len(I) * inner
    a = ctx.empty(n)
    rows = [ctx.empty(c) for _ in range(2)]
    lam = [int(v) for v in draw(rng, p, 3)]

    def stage():
        diff = ctx.cx_diff(a, outer, k, inner, ps, d, r)
        ctx.cx_apply(a, [diff] + rows, lam, outer, k, inner, ps, d, r)
        return diff

    cg = engine.CapturedLaunches(stage)
    for _ in range(2):
        A = draw(rng, p, n).reshape(outer, k, inner)
        R = [draw(rng, p, c) for _ in rows]
        a.t.copy_(ctx.from_ints(A.reshape(-1)).t)
        for x, v in zip(rows, R):
            x.t.copy_(ctx.from_ints(v).t)
        D = diff_ref(p, A, I, d).reshape(-1)
        want = ctx.from_ints(apply_ref(p, A, I, d, [D] + R, lam).reshape(-1))
        # uncaptured, on a copy
        b = a.clone()
        assert same(ctx.cx_apply(b, [ctx.cx_diff(b, outer, k, inner, ps, d, r)] + rows, lam, outer, k, inner, ps, d, r), want)
        cg.result.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        assert same(cg.result, ctx.from_ints(D)) and same(a, want)
