"""The four ends of a tournament round on the device (ffgpu_tour_diff / _select / _unit_prod / _unit_expand,
mpyc_amd/csrc/tour.hpp) against Python integers computed here from the maps include/ffgpu.h states, over every prime
policy and both pairings; views at odd element offsets and a capped grid; guard bytes around every output; status codes;
protocols.amax / amin / argmax / argmin / arg_index / maximum / minimum end to end for all parties on one GPU, the
reference's own values included; the same bytes as index_select / sub / mul / recombine / add / cat and the Fortran-order
interleave composed; a round trip through the four calls replayed from a captured HIP graph; two and nine rows, the edges of the launcher's
row dispatch, on both paths."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_sgn import FIELDS, draw, same, sizes, view
from test_tour_host import L as GOLDEN_L, _golden_cases, _one_hot, _values

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

HALVES, ODD_EVEN = 0, 1
# odd and even k, inner of 1, inner below a pack, whole packs, whole waves of 24-byte elements (with and without a bye)
SHAPES = ((1, 2, 5003), (1, 1025, 1), (257, 6, 1), (5, 7, 1), (3, 8, 64), (2, 5, 128), (2, 9, 3), (1, 3, 65))
NROWS = (1, 3, 7)


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def test_the_shapes_cross_the_unit_boundaries():
    assert max(sizes()) == 5003 and all(o * (k // 2) * i <= 5003 for o, k, i in SHAPES)
    assert {k % 2 for _, k, _ in SHAPES} == {0, 1} and {i for _, _, i in SHAPES} >= {1, 3, 64, 65, 128}


# ---- the maps on Python integers (object arrays) --------------------------------------------------------------------------
def pairs(k, mode):
    n0, pos = k % 2, np.arange(k)
    return (pos[n0:(k + 1) // 2], pos[(k + 1) // 2:]) if mode == HALVES else (pos[n0::2], pos[n0 + 1::2])


def diff_ref(p, A, mode, neg):
    a1, a2 = pairs(A.shape[1], mode)
    return ((A[:, a1, :] - A[:, a2, :]) if neg else (A[:, a2, :] - A[:, a1, :])) % p


def recombine_ref(p, rows, lam, shape):
    return (sum(l * r for l, r in zip(lam, rows)) % p).reshape(shape)


def select_ref(p, A, v, mode, neg):
    a1, _ = pairs(A.shape[1], mode)
    m = ((A[:, a1, :] - v) if neg else (A[:, a1, :] + v)) % p
    return np.concatenate((A[:, :1, :], m), axis=1) if A.shape[1] % 2 else m


def prod_ref(p, U, C, k):
    return U[:, k % 2:, :] * C % p


def expand_ref(p, U, v, k):
    outer, kc, inner = U.shape
    n0 = k % 2
    out = np.empty((outer, k, inner), dtype=object)
    out[:, n0::2, :] = (U[:, n0:, :] - v) % p
    out[:, n0 + 1::2, :] = v
    if n0:
        out[:, 0, :] = U[:, 0, :]
    return out


class Data:
    """the inputs of one field, uploaded once `offset` elements into their buffers: a level of NA elements and seven
    sub-share rows of NC; every shape takes prefixes"""

    def __init__(self, engine, ctx, p, seed, na=2 * 5003, nc=5003, offset=0, rows=max(NROWS)):
        rng = np.random.default_rng(seed)
        self.engine, self.ctx, self.p, self.offset, self.nc = engine, ctx, p, offset, nc
        self.A = draw(rng, p, na)
        self.A[:4] = [0, p - 1, 1, p - 2]
        self.R = [draw(rng, p, nc) for _ in range(rows)]
        for r in self.R:
            r[:4] = [p - 1, 0, p - 2, 1]
        self.lam = [int(v) for v in draw(rng, p, rows)]
        self.lam[0] = 1
        self.dA = self._up(self.A)
        self.dR = [self._up(r) for r in self.R]
        self.keep = [x.t.clone() for x in [self.dA] + self.dR]
        self.obuf = ctx.empty(na + offset)

    def _up(self, vals):
        buf = self.ctx.empty(len(vals) + self.offset)
        buf.t[self.offset:].copy_(self.ctx.from_ints(vals).t)
        return buf

    def a(self, n):
        return view(self.engine, self.ctx, self.dA, self.offset, self.offset + n)

    def rows(self, nr, c):
        return [view(self.engine, self.ctx, x, self.offset, self.offset + c) for x in self.dR[:nr]]

    def out(self, n):
        return view(self.engine, self.ctx, self.obuf, self.offset, self.offset + n)

    def untouched(self):
        return all(torch.equal(x.t, k) for x, k in zip([self.dA] + self.dR, self.keep))


def run_shape(d, outer, k, inner, nrows=NROWS):
    """the four kernels on one (outer, k, inner): both pairings, neg 0 and 1, every row count; expectations from Python
    integers, uploaded once; returns the number of calls checked"""
    ctx, p = d.ctx, d.p
    h, kc = k // 2, k // 2 + k % 2
    n, nh, c = outer * k * inner, outer * kc * inner, outer * h * inner
    assert c <= d.nc
    A, U = d.A[:n].reshape(outer, k, inner), d.A[:nh].reshape(outer, kc, inner)
    V = {nr: recombine_ref(p, [r[:c] for r in d.R[:nr]], d.lam[:nr] if nr > 1 else [1], (outer, h, inner)) for nr in nrows}
    lam = lambda nr: d.lam[:nr] if nr > 1 else [1]
    calls = []                                           # (what, expected, call)
    for mode in (HALVES, ODD_EVEN):
        for neg in (0, 1):
            calls.append((('diff', mode, neg), diff_ref(p, A, mode, neg),
                          lambda mode=mode, neg=neg: ctx.tour_diff(d.a(n), outer, k, inner, mode, neg, out=d.out(c))))
            for nr in nrows:
                calls.append((('select', mode, neg, nr), select_ref(p, A, V[nr], mode, neg),
                              lambda mode=mode, neg=neg, nr=nr: ctx.tour_select(d.a(n), d.rows(nr, c), lam(nr), outer, k, inner, mode, neg,
                                                                                  out=d.out(nh))))
    calls.append((('unit_prod',), prod_ref(p, U, d.R[0][:c].reshape(outer, h, inner), k),
                  lambda: ctx.tour_unit_prod(d.a(nh), d.rows(1, c)[0], outer, k, inner, out=d.out(c))))
    for nr in nrows:
        calls.append((('unit_expand', nr), expand_ref(p, U, V[nr], k),
                      lambda nr=nr: ctx.tour_unit_expand(d.a(nh), d.rows(nr, c), lam(nr), outer, k, inner, out=d.out(n))))
    W = ctx.from_ints(np.concatenate([w.reshape(-1) for _, w, _ in calls]))
    at = 0
    for what, w, call in calls:
        got = call()
        assert got.n == w.size and same(got, W.t[at:at + w.size]), (what, outer, k, inner, d.offset)
        at += w.size
    assert d.untouched(), ('an input was written', outer, k, inner)
    return len(calls)


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    d = Data(engine, ctx, p, seed=len(name) * 1000 + p % 997)
    ran = sum(run_shape(d, *shape) for shape in SHAPES)
    assert ran == len(SHAPES) * (2 * 2 * (1 + len(NROWS)) + 1 + len(NROWS))


@pytest.mark.parametrize('name', ['pm64-k64', 'pm96', 'pm192'])
def test_views_at_odd_element_offsets_and_capped_grid(mods, monkeypatch, name):
    """8-, 12- and 24-byte storage: the level, the rows and the output one element into their buffers (8- and 24-byte
    elements are then not 16-byte aligned: the element path), and the same with FFGPU_BLOCKS_PER_CU=1 on three times
    64 * 1024 compact elements (64 * 1024 is the number of threads of the capped grid when the device has 256 compute
    units), where every thread of the loop takes several units -- aligned (packs, whole waves) and at the odd offset"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    d = Data(engine, ctx, p, seed=11 + p % 997, offset=1)
    for shape in SHAPES:
        run_shape(d, *shape)
    monkeypatch.setenv('FFGPU_BLOCKS_PER_CU', '1')
    capped = engine.FieldContext(p, device=0)
    monkeypatch.delenv('FFGPU_BLOCKS_PER_CU')
    outer, k, inner = 3, 129, 1024
    c = outer * (k // 2) * inner
    threads = torch.cuda.get_device_properties(0).multi_processor_count * 256
    assert c == 3 * 64 * 1024 and c // 2 > threads            # more packs of 8-byte elements than threads in the grid
    for offset in (0, 1):
        big = Data(engine, capped, p, seed=17 + offset, na=outer * k * inner, nc=c, offset=offset)
        run_shape(big, outer, k, inner, nrows=(3,))


@pytest.mark.parametrize('name', ['pm64-k64', 'pm128', 'pm192'])
def test_two_and_nine_rows_on_both_paths(mods, name):
    """NROWS stops at seven; the launcher of select and unit_expand dispatches over 1 .. 9 rows, so both edges next to the
    ends, over 8-, 16- and 24-byte storage.  (3, 8, 64): the pack path (whole waves of 24-byte elements); (2, 9, 3) and
    (3, 8, 64) one element into the buffers: the element path of 8- and 24-byte elements (a pack of 16-byte elements is one
    element, aligned at every element offset: they stay on the pack path)"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    for offset, shapes in ((0, ((3, 8, 64), (2, 9, 3))), (1, ((3, 8, 64),))):
        d = Data(engine, ctx, p, seed=23 + offset + p % 997, na=3 * 8 * 64, nc=3 * 4 * 64, offset=offset, rows=9)
        for shape in shapes:
            assert run_shape(d, *shape, nrows=(2, 9)) == 2 * 2 * 3 + 1 + 2


@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
def test_nothing_is_written_outside_the_outputs(mods, name):
    """0xa5 on both sides of every output; the whole output is compared, so the bye row of the next level and every slot of
    unit_expand's (outer, k, inner) output are; inputs and rows keep their bytes"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    pad = 240                                              # a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    d = Data(engine, ctx, p, seed=13 + p % 997)
    Lb, hd, st = ctx._L, ctx._h, ctx._stream()

    def guarded(count):
        return torch.full((pad + count * ctx.elem_bytes + pad,), 0xa5, dtype=torch.uint8, device='cuda')

    def check(buf, want, what):
        raw = ctx.from_ints(want.reshape(-1)).t.contiguous().view(torch.uint8).reshape(-1)
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + raw.numel():] == 0xa5).all()), ('guard bytes written', what)
        assert torch.equal(buf[pad:pad + raw.numel()], raw), what

    nr = 3
    lam, lam2 = d.lam[:nr], ctx._scalars(d.lam[:nr])
    for outer, k, inner in ((5, 7, 1), (3, 8, 64), (2, 5, 128), (2, 9, 3), (1, 3, 65), (1, 2, 131)):
        h, kc = k // 2, k // 2 + k % 2
        n, nh, c = outer * k * inner, outer * kc * inner, outer * h * inner
        A, U = d.A[:n].reshape(outer, k, inner), d.A[:nh].reshape(outer, kc, inner)
        v = recombine_ref(p, [r[:c] for r in d.R[:nr]], lam, (outer, h, inner))
        ptrs = (ctypes.c_void_p * nr)(*[x.ptr for x in d.dR[:nr]])
        for mode in (HALVES, ODD_EVEN):
            for neg in (0, 1):
                b = guarded(c)
                assert Lb.ffgpu_tour_diff(hd, d.dA.ptr, b.data_ptr() + pad, outer, k, inner, mode, neg, st) == _ffi.OK
                check(b, diff_ref(p, A, mode, neg), ('diff', outer, k, inner, mode, neg))
                b = guarded(nh)
                assert Lb.ffgpu_tour_select(hd, d.dA.ptr, ptrs, lam2, nr, b.data_ptr() + pad, outer, k, inner, mode, neg, st) == _ffi.OK
                check(b, select_ref(p, A, v, mode, neg), ('select', outer, k, inner, mode, neg))
        b = guarded(c)
        assert Lb.ffgpu_tour_unit_prod(hd, d.dA.ptr, d.dR[0].ptr, b.data_ptr() + pad, outer, k, inner, st) == _ffi.OK
        check(b, prod_ref(p, U, d.R[0][:c].reshape(outer, h, inner), k), ('unit_prod', outer, k, inner))
        b = guarded(n)
        assert Lb.ffgpu_tour_unit_expand(hd, d.dA.ptr, ptrs, lam2, nr, b.data_ptr() + pad, outer, k, inner, st) == _ffi.OK
        check(b, expand_ref(p, U, v, k), ('unit_expand', outer, k, inner))
        assert d.untouched(), 'an input or a row was written'


def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p = 2**61 - 1
    ctx = engine.FieldContext(p, device=0)
    Lb, h, st = ctx._L, ctx._h, ctx._stream()
    shape = (2, 13, 3)
    outer, k, inner = shape
    n = outer * k * inner
    eb = ctx.elem_bytes
    pat = lambda cnt, v: torch.full((cnt * eb,), v, dtype=torch.uint8, device='cuda')
    A, O, R = pat(n, 0x5a), pat(n, 0x3c), pat(n, 0x77)
    a, o, rw = A.data_ptr(), O.data_ptr(), R.data_ptr()
    rows = (ctypes.c_void_p * 12)(*([rw] * 12))
    lam = ctx._scalars([1] * 12)
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    diff = lambda a_=a, o_=o, shape=shape, mode=HALVES: Lb.ffgpu_tour_diff(h, a_, o_, *shape, mode, 0, st)
    sel = lambda a_=a, rows_=rows, lam_=lam, nr=3, o_=o, shape=shape, mode=ODD_EVEN: Lb.ffgpu_tour_select(h, a_, rows_, lam_, nr, o_, *shape, mode, 1, st)
    prod = lambda u_=a, c_=rw, o_=o, shape=shape: Lb.ffgpu_tour_unit_prod(h, u_, c_, o_, *shape, st)
    exp = lambda u_=a, rows_=rows, lam_=lam, nr=3, o_=o, shape=shape: Lb.ffgpu_tour_unit_expand(h, u_, rows_, lam_, nr, o_, *shape, st)
    assert diff() == OK and sel() == OK and prod() == OK and exp() == OK        # (valid calls, for contrast)
    assert sel(nr=9) == OK and exp(nr=9) == OK
    torch.cuda.synchronize()
    assert not bool((O == 0x3c).all())
    O.fill_(0x3c)
    # a null context or pointer
    assert Lb.ffgpu_tour_diff(None, a, o, *shape, 0, 0, st) == EINVAL
    assert Lb.ffgpu_tour_select(None, a, rows, lam, 3, o, *shape, 0, 0, st) == EINVAL
    assert Lb.ffgpu_tour_unit_prod(None, a, rw, o, *shape, st) == EINVAL
    assert Lb.ffgpu_tour_unit_expand(None, a, rows, lam, 3, o, *shape, st) == EINVAL
    assert diff(a_=None) == EINVAL and diff(o_=None) == EINVAL
    assert prod(u_=None) == EINVAL and prod(c_=None) == EINVAL and prod(o_=None) == EINVAL
    holed = (ctypes.c_void_p * 3)(rw, None, rw)
    for fn in (sel, exp):
        assert fn(None) == EINVAL and fn(rows_=None) == EINVAL and fn(lam_=None) == EINVAL and fn(o_=None) == EINVAL
        assert fn(rows_=holed) == EINVAL
    # k < 2
    for kk in (1, 0):
        bad = (outer, kk, inner)
        assert diff(shape=bad) == EINVAL and sel(shape=bad) == EINVAL and prod(shape=bad) == EINVAL and exp(shape=bad) == EINVAL
    # an unknown mode
    for mode in (2, -1, 7):
        assert diff(mode=mode) == EINVAL and sel(mode=mode) == EINVAL
    # nrows
    for fn in (sel, exp):
        assert fn(nr=0) == EINVAL and fn(nr=-1) == EINVAL
        assert fn(nr=10) == ENOTSUP and fn(nr=12) == ENOTSUP
    # sizes whose element or byte count overflows
    for bad in ((1 << 40, 13, 1 << 21), (1 << 62, 13, 4), (1, 1 << 61, 1)):
        assert diff(shape=bad) == EINVAL and sel(shape=bad) == EINVAL and prod(shape=bad) == EINVAL and exp(shape=bad) == EINVAL
    # overlap: an output inside an input, a row inside an output
    last = (n - 1) * eb
    assert diff(o_=a) == EINVAL and diff(o_=a + last) == EINVAL
    assert sel(o_=a) == EINVAL and sel(o_=a + last) == EINVAL
    assert exp(o_=a) == EINVAL and exp(o_=a + (outer * (k // 2 + 1) * inner - 1) * eb) == EINVAL     # (u is (outer, kc, inner))
    assert prod(o_=a) == EINVAL and prod(o_=rw) == EINVAL and prod(o_=rw + (outer * (k // 2) * inner - 1) * eb) == EINVAL
    for fn in (sel, exp):
        assert fn(rows_=(ctypes.c_void_p * 3)(rw, o + 8, rw)) == EINVAL and fn(rows_=(ctypes.c_void_p * 3)(o, rw, rw)) == EINVAL
    torch.cuda.synchronize()
    assert bool((A == 0x5a).all()) and bool((O == 0x3c).all()) and bool((R == 0x77).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    for empty in ((0, k, inner), (outer, k, 0)):
        assert diff(a_=None, o_=None, shape=empty) == OK and sel(a_=None, rows_=None, o_=None, shape=empty) == OK
        assert prod(u_=None, c_=None, o_=None, shape=empty) == OK and exp(u_=None, rows_=None, o_=None, shape=empty) == OK
    torch.cuda.synchronize()
    assert bool((A == 0x5a).all()) and bool((O == 0x3c).all())
    # binary fields
    for mod in (0x11b, (1 << 64) | 0x1b, (1 << 128) | 0x87):
        bctx = engine.FieldContext(mod, True, device=0)
        G = torch.full((8192,), 0x42, dtype=torch.uint8, device='cuda')
        g = G.data_ptr()
        brow, one = (ctypes.c_void_p * 1)(g + 2048), bctx._scalars([1])
        bL, bh = bctx._L, bctx._h
        assert bL.ffgpu_tour_diff(bh, g, g + 4096, 1, 8, 1, 0, 0, st) == ENOTSUP
        assert bL.ffgpu_tour_select(bh, g, brow, one, 1, g + 4096, 1, 8, 1, 0, 0, st) == ENOTSUP
        assert bL.ffgpu_tour_unit_prod(bh, g, g + 2048, g + 4096, 1, 8, 1, st) == ENOTSUP
        assert bL.ffgpu_tour_unit_expand(bh, g, brow, one, 1, g + 4096, 1, 8, 1, st) == ENOTSUP
        torch.cuda.synchronize()
        assert bool((G == 0x42).all())
    # the engine's own checks
    x = ctx.from_ints(list(range(n)))
    half = ctx.from_ints(list(range(outer * 7 * inner)))
    comp = ctx.from_ints(list(range(outer * 6 * inner)))
    for bad in (lambda: ctx.tour_diff(x, outer, k + 1, inner, HALVES),
                lambda: ctx.tour_diff(x, outer, k, inner, 2),
                lambda: ctx.tour_diff(x, outer, k, inner, HALVES, out=ctx.empty(5)),
                lambda: ctx.tour_diff(x, 0, k, inner, HALVES),
                lambda: ctx.tour_diff(x, n, 1, 1, HALVES),
                lambda: ctx.tour_select(x, [ctx.empty(5)], [1], outer, k, inner, HALVES),
                lambda: ctx.tour_select(x, [], [], outer, k, inner, HALVES),
                lambda: ctx.tour_select(x, [comp], [1, 1], outer, k, inner, HALVES),
                lambda: ctx.tour_select(x, [comp], [1], outer, k, inner, HALVES, out=comp),
                lambda: ctx.tour_unit_prod(x, comp, outer, k, inner),
                lambda: ctx.tour_unit_prod(half, half, outer, k, inner),
                lambda: ctx.tour_unit_expand(x, [comp], [1], outer, k, inner),
                lambda: ctx.tour_unit_expand(half, [comp], [1], outer, k, inner, out=half)):
        with pytest.raises(ValueError):
            bad()
    assert ctx.tour_unit_expand(half, [comp], [1], outer, k, inner).n == n and ctx.tour_unit_prod(half, comp, outer, k, inner).n == comp.n


# ---- the protocols ----------------------------------------------------------------------------------------------------------
E2E_SHAPES = [(1, 2, 31), (7, 3, 1), (64, 10, 1), (2, 33, 5), (1, 257, 1)]


def _plain_arrays(l, seed):
    """the end-to-end shapes with values of l-2 signed bits (every difference has l-1), and the reference's arrays"""
    rng = random.Random(seed)
    out = []
    for shape in E2E_SHAPES:
        a = _values(rng, shape).astype(object)
        if l > GOLDEN_L:                                  # stretch to the bit length: order, ties and extremes stay
            a = a * (1 << (l - GOLDEN_L))
        out.append((a, None))
    for case in _golden_cases():
        out.append((np.array(case['values'], dtype=object).reshape(case['shape']), case))
    return out


@pytest.mark.parametrize('modulus,l', [(2**61 - 1, 16), (2**64 - 189, 32)], ids=['2^61-1', '2^64-189'])
@pytest.mark.parametrize('m,t', [(3, 1), (7, 3)])
def test_tournaments_end_to_end(mods, modulus, l, m, t):
    _ffi, engine, finfields, protocols = mods
    from oracle import pyoracle as po
    F = finfields.GF(modulus)
    ctx = engine.FieldContext(modulus, device=0)
    rng = random.Random(l * 100 + m)
    sh = lambda v: protocols.share(ctx, ctx.from_ints([int(x) % modulus for x in v]), t, m)
    signed = lambda v: v - modulus if v > modulus // 2 else v
    picks = (list(range(t + 1)), sorted(rng.sample(range(m), t + 1)), list(range(m - t - 1, m)))
    lams = [[int(v) for v in po.recombination_vector(po.Field(modulus, False), [i + 1 for i in pick], 0)] for pick in picks]

    def rand(count):
        return (sh([rng.randrange(2) for _ in range(count * l)]), sh([rng.randrange(2) for _ in range(count)]),
                sh([rng.randrange(1 << 24) for _ in range(count)]), sh([rng.randrange(1, modulus) for _ in range(count)]))

    def opens_to(shares, want, what):
        """any t+1 shares recombine to `want`"""
        want = [int(v) for v in np.asarray(want).reshape(-1)]
        assert len(shares) == m and all(s.n == len(want) for s in shares), what
        for pick, lam in zip(picks, lams):
            assert [signed(v) for v in ctx.recombine([shares[i] for i in pick], lam).to_ints()] == want, (what, pick)

    for plain, case in _plain_arrays(l, seed=l + m):
        outer, k, inner = plain.shape
        ints = plain.astype(np.int64)
        xs = sh(plain.reshape(-1))
        before = [x.t.clone() for x in xs]
        args = (outer, k, inner, t, l, rand)
        opens_to(protocols.amax(ctx, F, xs, *args), ints.max(axis=1), ('amax', plain.shape))
        opens_to(protocols.amin(ctx, F, xs, *args), ints.min(axis=1), ('amin', plain.shape))
        for name, fn, npfn, ext in (('argmax', protocols.argmax, np.argmax, np.max), ('argmin', protocols.argmin, np.argmin, np.min)):
            unit, value = fn(ctx, F, xs, *args)
            opens_to(unit, _one_hot(npfn(ints, axis=1), k), (name, 'unit', plain.shape))
            opens_to(value, ext(ints, axis=1), (name, 'value', plain.shape))
            opens_to(protocols.arg_index(ctx, unit, outer, k, inner), npfn(ints, axis=1), (name, 'index', plain.shape))
            if case is not None:                          # what the reference itself returned
                opens_to(unit, case[name + '_unit'], (name, 'reference unit', plain.shape))
                opens_to(value, case[name + '_value'], (name, 'reference value', plain.shape))
        assert all(torch.equal(x.t, b) for x, b in zip(xs, before)), 'a protocol wrote its input'
    for fn in (protocols.amax, protocols.amin, protocols.argmax, protocols.argmin):
        with pytest.raises(ValueError):
            fn(ctx, F, xs[:2 * t], *args)
        with pytest.raises(ValueError):
            fn(ctx, F, xs, outer, k + 1, inner, t, l, rand)
    # the element-wise pair
    n = 1031
    lo, hi = -(1 << (l - 3)), (1 << (l - 3)) - 1
    x = [hi, lo, 0, 5, lo, hi] + [rng.randint(lo, hi) for _ in range(n - 6)]
    y = [lo, hi, 0, 5, lo, hi] + [rng.randint(lo, hi) for _ in range(n - 6)]
    xs, ys = sh(x), sh(y)
    before = [v.t.clone() for v in xs + ys]
    opens_to(protocols.maximum(ctx, F, xs, ys, t, l, rand), np.maximum(x, y), 'maximum')
    opens_to(protocols.minimum(ctx, F, xs, ys, t, l, rand), np.minimum(x, y), 'minimum')
    assert all(torch.equal(v.t, b) for v, b in zip(xs + ys, before))
    with pytest.raises(ValueError):
        protocols.maximum(ctx, F, xs[:2 * t], ys[:2 * t], t, l, rand)


@pytest.mark.parametrize('modulus', [2**64 - 189, 2**80 - 65], ids=['2^64-189', '2^80-65'])
@pytest.mark.parametrize('shape', [(2, 257, 1), (3, 12, 5), (2, 9, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_same_bytes_as_the_composition_of_existing_calls(mods, modulus, shape):
    """one downward and one upward round per pairing: the gathers, the difference, the recombination, a1 +- v and the
    concatenation with the bye from index_select, ffgpu_sub, ffgpu_recombine, ffgpu_add / _sub and cat; u[:, n0:] * c from
    a slice and ffgpu_mul; (u - v, v) concatenated and reshaped in Fortran order, as the reference writes it
    (runtime.py:3945-3948), give the bytes of the four kernels"""
    _ffi, engine, _, _ = mods
    ctx = engine.FieldContext(modulus, device=0)
    outer, k, inner = shape
    rng = np.random.default_rng(k + inner)
    n0, h = k % 2, k // 2
    kc = h + n0
    n, nh, c, nr = outer * k * inner, outer * kc * inner, outer * h * inner, 3
    a = ctx.from_ints(draw(rng, modulus, n))
    u = ctx.from_ints(draw(rng, modulus, nh))
    lam = [int(v) for v in draw(rng, modulus, nr)]
    rows = [ctx.from_ints(draw(rng, modulus, c)) for _ in range(nr)]
    tail = tuple(a.t.shape[1:])
    cube = lambda x, kk: x.t.reshape((outer, kk, inner) + tail)
    flat = lambda t: engine.DevArray(ctx, t.contiguous().reshape((-1,) + tail), t.numel() // (int(np.prod(tail)) if tail else 1))
    v = ctx.recombine(rows, lam)
    for mode in (HALVES, ODD_EVEN):
        i1, i2 = (torch.as_tensor(x, device='cuda') for x in pairs(k, mode))
        a1, a2 = flat(cube(a, k).index_select(1, i1)), flat(cube(a, k).index_select(1, i2))
        for neg in (0, 1):
            assert same(ctx.tour_diff(a, outer, k, inner, mode, neg), (ctx.sub(a1, a2) if neg else ctx.sub(a2, a1)).t), (mode, neg)
            m_ = cube(ctx.sub(a1, v) if neg else ctx.add(a1, v), h)
            want = torch.cat((cube(a, k)[:, :1], m_), dim=1) if n0 else m_
            assert same(ctx.tour_select(a, rows, lam, outer, k, inner, mode, neg), want.contiguous()), (mode, neg)
    # upward: u2 = u[:, n0:] * c; (u - u2, u2) concatenated along the leading axis, reshaped in Fortran order; u0 re-attached
    ubody = flat(cube(u, kc)[:, n0:])
    assert same(ctx.tour_unit_prod(u, rows[0], outer, k, inner), ctx.mul(ubody, rows[0]).t)
    lead = (outer * inner,)                               # the reference's rows: one per (o, i), the axis last
    rowsfirst = lambda x: cube(x, h).movedim(1, 2).reshape(lead + (h,) + tail)
    stacked = torch.cat((rowsfirst(ctx.sub(ubody, v)), rowsfirst(v)), dim=0)                    # (2 * rows, h)
    # reshape((rows, 2h), order='F') of the (2 rows, h) array: element (r, 2j + s) = stacked[s * rows + r, j]
    inter = stacked.reshape((2,) + lead + (h,) + tail).movedim(0, 2).reshape(lead + (2 * h,) + tail)
    if n0:
        u0 = cube(u, kc)[:, :1].movedim(1, 2).reshape(lead + (1,) + tail)
        inter = torch.cat((u0, inter), dim=1)
    want = inter.reshape((outer, inner, k) + tail).movedim(2, 1).contiguous()
    assert same(ctx.tour_unit_expand(u, rows, lam, outer, k, inner), want)


def test_graph_capture_replays_a_round_trip(mods):
    """diff -> select (the difference itself as one of the rows) -> unit_prod -> unit_expand, captured once, replayed on
    inputs changed in between"""
    _ffi, engine, _, _ = mods
    p = 2**64 - 189
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(21)
    outer, k, inner = 2, 9, 64
    h, kc = k // 2, k // 2 + k % 2
    n, nh, c = outer * k * inner, outer * kc * inner, outer * h * inner
    a = ctx.empty(n)
    rows = [ctx.empty(c) for _ in range(2)]
    lam = [int(v) for v in draw(rng, p, 3)]

    def trip():
        diff = ctx.tour_diff(a, outer, k, inner, ODD_EVEN, True)
        nxt = ctx.tour_select(a, [diff] + rows, lam, outer, k, inner, ODD_EVEN, True)
        prod = ctx.tour_unit_prod(nxt, diff, outer, k, inner)
        return ctx.tour_unit_expand(nxt, [prod] + rows, lam, outer, k, inner)

    cg = engine.CapturedLaunches(trip)
    for _ in range(2):
        A = draw(rng, p, n).reshape(outer, k, inner)
        R = [draw(rng, p, c) for _ in rows]
        a.t.copy_(ctx.from_ints(A.reshape(-1)).t)
        for x, v in zip(rows, R):
            x.t.copy_(ctx.from_ints(v).t)
        D = diff_ref(p, A, ODD_EVEN, 1)
        N = select_ref(p, A, recombine_ref(p, [D.reshape(-1)] + R, lam, D.shape), ODD_EVEN, 1)
        P = prod_ref(p, N, D, k)
        want = ctx.from_ints(expand_ref(p, N, recombine_ref(p, [P.reshape(-1)] + R, lam, D.shape), k).reshape(-1))
        assert same(trip(), want.t)                       # uncaptured
        cg.result.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        assert same(cg.result, want.t) and same(a, ctx.from_ints(A.reshape(-1)).t)
