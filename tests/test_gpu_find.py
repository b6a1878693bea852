"""The three ends of a round of the first-occurrence search on the device (ffgpu_find_leaf_prod / _leaf_apply / _prod,
mpyc_amd/csrc/find.hpp) against Python integers computed here from the maps include/ffgpu.h states, over every prime policy,
with and without the public leaf, flipped and not, two and three components; views at odd element offsets and a capped grid;
guard bytes around every output; inputs and table untouched; status codes; the later rounds' apply through ffgpu_tour_select
on the components as rows; protocols.find end to end for all parties on one GPU, the reference's own values included; a
round trip through the calls replayed from a captured HIP graph; two and nine rows, the edges of the launcher's row
dispatch, on both paths."""
import ctypes
import random

import numpy as np
import pytest

from test_find_host import first_index, golden_cases, random_bits, recorded, variants
from test_gpu_sgn import FIELDS, draw, same, view

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ODD_EVEN = 1
# (outer, k, inner, which virt): odd and even k + virt, inner of 1, inner below a pack, whole packs, whole waves of 24-byte
# elements; the public leaf as the only partner (k = 1) and as the partner of a pack or wave run
SHAPES = ((1, 1, 5003, (1,)), (1, 2, 5003, (0, 1)), (1, 1025, 1, (0, 1)), (257, 6, 1, (0, 1)), (5, 7, 1, (0, 1)), (3, 8, 64, (0, 1)),
          (2, 5, 128, (0, 1)), (2, 9, 3, (0, 1)), (1, 3, 65, (0, 1)))
NROWS = (1, 3, 7)
NA = 3 * 2 * 5003                                           # a level (3, 1, 2, 5003); the bits are a prefix
NC = 3 * 5003                                               # a compact array of three components
NT = 2 * 2 * 1026                                           # a table (2, 2, 1026)
SMALL = 2000                                                # shapes up to this many bits take every (flip, C) combination


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def test_the_shapes_cross_the_unit_boundaries():
    assert all(o * k * i <= 2 * 5003 and o * ((k + 1) // 2) * i <= 5003 for o, k, i, _ in SHAPES)
    assert {(k + v) % 2 for _, k, _, vs in SHAPES for v in vs} == {0, 1} and {i for _, _, i, _ in SHAPES} >= {1, 3, 64, 65, 128, 5003}
    assert (1, 1, 5003, (1,)) in SHAPES and max(k for _, k, _, _ in SHAPES) + 1 <= NT // 4


# ---- the maps on Python integers (object arrays) --------------------------------------------------------------------------
def pairs(kk):
    n0, pos = kk % 2, np.arange(kk)
    return pos[n0::2], pos[n0 + 1::2]


def leaves_ref(p, B, T, flip, virt):
    """the leaf level (C, outer, k + virt, inner) that is never stored: leaf j = (b', T[q, 0, j] + b' T[q, 1, j])"""
    outer, k, inner = B.shape
    b = (1 - B) % p if flip else B
    if virt:
        b = np.concatenate((b, np.ones((outer, 1, inner), dtype=object)), axis=1)      # the public leaf: b' = 1, not flipped
    return np.stack([b] + [(T[q, 0][None, :, None] + b * T[q, 1][None, :, None]) % p for q in range(T.shape[0])])


def prod_ref(p, LV):
    a1, a2 = pairs(LV.shape[2])
    return LV[0][None][:, :, a1, :] * (LV[:, :, a2, :] - LV[:, :, a1, :]) % p


def apply_ref(p, LV, V):
    a1, _ = pairs(LV.shape[2])
    m = (LV[:, :, a1, :] + V) % p
    return np.concatenate((LV[:, :, :1, :], m), axis=2) if LV.shape[2] % 2 else m


def recombine_ref(p, rows, lam, shape):
    return (sum(l * r for l, r in zip(lam, rows)) % p).reshape(shape)


class Data:
    """the inputs of one field, uploaded once `offset` elements into their buffers: a level of `na` elements (the bits are a
    prefix), seven sub-share rows of `nc` and a table pool; every shape takes prefixes"""

    def __init__(self, engine, ctx, p, seed, na=NA, nc=NC, offset=0, nrows=max(NROWS), nout=None):
        rng = np.random.default_rng(seed)
        self.engine, self.ctx, self.p, self.offset, self.nc = engine, ctx, p, offset, nc
        self.A = draw(rng, p, na)
        self.A[:4] = [0, p - 1, 1, p - 2]
        self.R = [draw(rng, p, nc) for _ in range(nrows)]
        for r in self.R:
            r[:4] = [p - 1, 0, p - 2, 1]
        self.T = draw(rng, p, NT)
        self.T[:3] = [p - 1, 0, 1]
        self.lam = [int(v) for v in draw(rng, p, max(nrows, max(NROWS)))]
        self.lam[0] = 1
        self.dA, self.dT = self._up(self.A), self._up(self.T)
        self.dR = [self._up(r) for r in self.R]
        self.keep = [x.t.clone() for x in [self.dA, self.dT] + self.dR]
        self.obuf = ctx.empty((nout or na) + offset)

    def _up(self, vals):
        buf = self.ctx.empty(len(vals) + self.offset)
        buf.t[self.offset:].copy_(self.ctx.from_ints(vals).t)
        return buf

    def a(self, n):
        return view(self.engine, self.ctx, self.dA, self.offset, self.offset + n)

    def tab(self, n):
        return view(self.engine, self.ctx, self.dT, self.offset, self.offset + n)

    def rows(self, nr, c):
        return [view(self.engine, self.ctx, x, self.offset, self.offset + c) for x in self.dR[:nr]]

    def out(self, n):
        return view(self.engine, self.ctx, self.obuf, self.offset, self.offset + n)

    def untouched(self):
        return all(torch.equal(x.t, k) for x, k in zip([self.dA, self.dT] + self.dR, self.keep))


def run_shape(d, outer, k, inner, virts, combos, nrows=NROWS, levels=(2, 3)):
    """the three kernels and the later rounds' apply on one (outer, k, inner); combos: the (flip, C) of the leaf calls, per
    virt; expectations from Python integers, uploaded once; returns the number of calls checked"""
    ctx, p = d.ctx, d.p
    lam = lambda nr: d.lam[:nr] if nr > 1 else [1]
    calls = []                                           # (what, expected, call)
    B = d.A[:outer * k * inner].reshape(outer, k, inner)
    for virt in virts:
        kv = k + virt
        h, kc = kv // 2, kv // 2 + kv % 2
        for flip, C in combos[virt]:
            T = d.T[:(C - 1) * 2 * kv].reshape(C - 1, 2, kv)
            LV = leaves_ref(p, B, T, flip, virt)
            c = C * outer * h * inner
            assert c <= d.nc
            args = (outer, k, inner, C, flip, virt)
            calls.append((('leaf_prod',) + args, prod_ref(p, LV),
                          lambda args=args, T=T, c=c: ctx.find_leaf_prod(d.a(B.size), d.tab(T.size), *args, out=d.out(c))))
            for nr in nrows:
                V = recombine_ref(p, [r[:c] for r in d.R[:nr]], lam(nr), (C, outer, h, inner))
                calls.append((('leaf_apply', nr) + args, apply_ref(p, LV, V),
                              lambda args=args, T=T, c=c, nr=nr, n=C * outer * kc * inner: ctx.find_leaf_apply(
                                  d.a(B.size), d.tab(T.size), d.rows(nr, c), lam(nr), *args, out=d.out(n))))
    if k >= 2:                                           # a stored level, and its apply through tour_select
        h, kc = k // 2, k // 2 + k % 2
        for C in levels:
            LV = d.A[:C * B.size].reshape(C, outer, k, inner)
            c = C * outer * h * inner
            calls.append((('prod', outer, k, inner, C), prod_ref(p, LV),
                          lambda C=C, c=c: ctx.find_prod(d.a(C * B.size), outer, k, inner, C, out=d.out(c))))
            V = recombine_ref(p, [r[:c] for r in d.R[:3]], lam(3), (C, outer, h, inner))
            calls.append((('tour_select as the apply', outer, k, inner, C), apply_ref(p, LV, V),
                          lambda C=C, c=c: ctx.tour_select(d.a(C * B.size), d.rows(3, c), lam(3), C * outer, k, inner, ODD_EVEN,
                                                           out=d.out(C * outer * kc * inner))))
    W = ctx.from_ints(np.concatenate([w.reshape(-1) for _, w, _ in calls]))
    at = 0
    for what, w, call in calls:
        got = call()
        assert got.n == w.size and same(got, W.t[at:at + w.size]), (what, d.offset)
        at += w.size
    assert d.untouched(), ('an input, a row or the table was written', outer, k, inner)
    return len(calls)


ALL_COMBOS = [(flip, C) for flip in (0, 1) for C in (2, 3)]


def run_all(d):
    """every shape; the small ones with every (flip, C), the large ones with one each, cycling per virt"""
    ran, turn, seen = 0, {0: 0, 1: 0}, set()
    for outer, k, inner, virts in SHAPES:
        combos = {}
        for virt in virts:
            if outer * k * inner <= SMALL:
                combos[virt] = ALL_COMBOS
            else:
                combos[virt] = [ALL_COMBOS[turn[virt] % 4]]
                turn[virt] += 1
            seen |= {(virt,) + fc for fc in combos[virt]}
        ran += run_shape(d, outer, k, inner, virts, combos)
    assert len(seen) == 8
    return ran


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    assert run_all(Data(engine, ctx, p, seed=len(name) * 1000 + p % 997)) > 150


@pytest.mark.parametrize('name', ['pm64-k64', 'pm96', 'pm192'])
def test_views_at_odd_element_offsets(mods, name):
    """8-, 12- and 24-byte storage: the bits, the level, the table, the rows and the output one element into their buffers
    (8- and 24-byte elements are then not 16-byte aligned: the element path)"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    run_all(Data(engine, ctx, p, seed=11 + p % 997, offset=1))


@pytest.mark.parametrize('name', ['pm64-k64', 'pm128', 'pm192'])
def test_two_and_nine_rows_on_both_paths(mods, name):
    """NROWS stops at seven; the launcher of leaf_apply dispatches over 1 .. 9 rows, so both edges next to the ends, over
    8-, 16- and 24-byte storage, with and without the public leaf.  (3, 8, 64): the pack path (whole waves of 24-byte
    elements); (2, 9, 3) and (3, 8, 64) one element into the buffers: the element path of 8- and 24-byte elements (a pack of
    16-byte elements is one element, aligned at every element offset: they stay on the pack path)"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    combos = {0: [(0, 3)], 1: [(1, 2)]}
    for offset, shapes in ((0, ((3, 8, 64), (2, 9, 3))), (1, ((3, 8, 64),))):
        d = Data(engine, ctx, p, seed=23 + offset + p % 997, na=3 * 8 * 64, nc=3 * 3 * 4 * 64, offset=offset, nrows=9,
                 nout=3 * 3 * 5 * 64)
        for outer, k, inner in shapes:
            assert run_shape(d, outer, k, inner, (0, 1), combos, nrows=(2, 9), levels=()) == 2 * 3


@pytest.mark.parametrize('name', ['pm64-k64', 'pm192'])
def test_capped_grid(mods, monkeypatch, name):
    """FFGPU_BLOCKS_PER_CU=1 on three times 64 * 1024 compact elements per component (64 * 1024 is the number of threads of
    the capped grid when the device has 256 compute units): every thread of the loop takes several units, with a bye and the
    public leaf as the partner of the last run -- aligned (packs, whole waves) and at an odd offset"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    monkeypatch.setenv('FFGPU_BLOCKS_PER_CU', '1')
    capped = engine.FieldContext(p, device=0)
    monkeypatch.delenv('FFGPU_BLOCKS_PER_CU')
    outer, k, inner = 3, 128, 1024
    c = outer * ((k + 1) // 2) * inner
    threads = torch.cuda.get_device_properties(0).multi_processor_count * 256
    assert c == 3 * 64 * 1024 and c // 2 > threads            # more packs of 8-byte elements than threads in the grid
    for offset in (0, 1):
        big = Data(engine, capped, p, seed=17 + offset, na=outer * k * inner, nc=2 * c, offset=offset, nrows=3, nout=2 * outer * (k + 2) // 2 * inner)
        run_shape(big, outer, k, inner, (1,), {1: [(1, 2)]}, nrows=(3,), levels=())


@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
def test_nothing_is_written_outside_the_outputs(mods, name):
    """0xa5 on both sides of every output; the whole output is compared, so the bye of every component of the next level
    is; bits, level, table and rows keep their bytes"""
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

    nr, C = 3, 3
    lam, lam2 = d.lam[:nr], ctx._scalars(d.lam[:nr])
    ptrs = (ctypes.c_void_p * nr)(*[x.ptr for x in d.dR[:nr]])
    for outer, k, inner in ((5, 7, 1), (3, 8, 64), (2, 5, 128), (2, 9, 3), (1, 3, 65), (1, 2, 131), (4, 1, 64)):
        B = d.A[:outer * k * inner].reshape(outer, k, inner)
        for virt, flip in ((0, 1), (1, 0)):
            kv = k + virt
            if kv < 2:
                continue
            h, kc = kv // 2, kv // 2 + kv % 2
            T = d.T[:(C - 1) * 2 * kv].reshape(C - 1, 2, kv)
            LV = leaves_ref(p, B, T, flip, virt)
            v = recombine_ref(p, [r[:C * outer * h * inner] for r in d.R[:nr]], lam, (C, outer, h, inner))
            b = guarded(C * outer * h * inner)
            assert Lb.ffgpu_find_leaf_prod(hd, d.dA.ptr, d.dT.ptr, b.data_ptr() + pad, outer, k, inner, C, flip, virt, st) == _ffi.OK
            check(b, prod_ref(p, LV), ('leaf_prod', outer, k, inner, virt))
            b = guarded(C * outer * kc * inner)
            assert Lb.ffgpu_find_leaf_apply(hd, d.dA.ptr, d.dT.ptr, ptrs, lam2, nr, b.data_ptr() + pad, outer, k, inner, C, flip, virt,
                                            st) == _ffi.OK
            check(b, apply_ref(p, LV, v), ('leaf_apply', outer, k, inner, virt))
        if k >= 2:
            b = guarded(C * outer * (k // 2) * inner)
            assert Lb.ffgpu_find_prod(hd, d.dA.ptr, b.data_ptr() + pad, outer, k, inner, C, st) == _ffi.OK
            check(b, prod_ref(p, d.A[:C * B.size].reshape(C, outer, k, inner)), ('prod', outer, k, inner))
        assert d.untouched(), 'an input, a row or the table was written'


def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p = 2**61 - 1
    ctx = engine.FieldContext(p, device=0)
    Lb, h, st = ctx._L, ctx._h, ctx._stream()
    shape = (2, 13, 3)
    outer, k, inner = shape
    C = 3
    n = 5 * outer * (k + 1) * inner                        # room for five components of k + 1 positions
    eb = ctx.elem_bytes
    pat = lambda cnt, v: torch.full((cnt * eb,), v, dtype=torch.uint8, device='cuda')
    A, O, R, T = pat(n, 0x5a), pat(n, 0x3c), pat(n, 0x77), pat(n, 0x11)
    a, o, rw, tb = A.data_ptr(), O.data_ptr(), R.data_ptr(), T.data_ptr()
    rows = (ctypes.c_void_p * 12)(*([rw] * 12))
    lam = ctx._scalars([1] * 12)
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    lp = lambda b_=a, t_=tb, o_=o, shape=shape, C=C, flip=1, virt=1: Lb.ffgpu_find_leaf_prod(h, b_, t_, o_, *shape, C, flip, virt, st)
    la = lambda b_=a, t_=tb, rows_=rows, lam_=lam, nr=3, o_=o, shape=shape, C=C, flip=1, virt=1: Lb.ffgpu_find_leaf_apply(
        h, b_, t_, rows_, lam_, nr, o_, *shape, C, flip, virt, st)
    pr = lambda l_=a, o_=o, shape=shape, C=C: Lb.ffgpu_find_prod(h, l_, o_, *shape, C, st)
    assert lp() == OK and la() == OK and pr() == OK and la(nr=9) == OK and la(nr=1) == OK        # (valid calls, for contrast)
    assert lp(shape=(4, 1, 2)) == OK and la(shape=(4, 1, 2)) == OK                               # k = 1 with the public leaf
    assert lp(C=2, virt=0, flip=0) == OK and lp(C=5) == OK and pr(C=5) == OK
    torch.cuda.synchronize()
    assert not bool((O == 0x3c).all())
    O.fill_(0x3c)
    # a null context or pointer
    assert Lb.ffgpu_find_leaf_prod(None, a, tb, o, *shape, C, 0, 1, st) == EINVAL
    assert Lb.ffgpu_find_leaf_apply(None, a, tb, rows, lam, 3, o, *shape, C, 0, 1, st) == EINVAL
    assert Lb.ffgpu_find_prod(None, a, o, *shape, C, st) == EINVAL
    assert lp(b_=None) == EINVAL and lp(t_=None) == EINVAL and lp(o_=None) == EINVAL
    assert la(b_=None) == EINVAL and la(t_=None) == EINVAL and la(rows_=None) == EINVAL and la(lam_=None) == EINVAL and la(o_=None) == EINVAL
    assert la(rows_=(ctypes.c_void_p * 3)(rw, None, rw)) == EINVAL
    assert pr(l_=None) == EINVAL and pr(o_=None) == EINVAL
    # k < 1; k < 2 for a stored level; fewer than two positions for the leaf calls
    assert lp(shape=(outer, 0, inner)) == EINVAL and la(shape=(outer, 0, inner)) == EINVAL and pr(shape=(outer, 0, inner)) == EINVAL
    assert pr(shape=(outer, 1, inner)) == EINVAL
    assert lp(shape=(outer, 1, inner), virt=0) == EINVAL and la(shape=(outer, 1, inner), virt=0) == EINVAL
    # the number of components, flip, virt
    for bad in (1, 0, -1, 6, 9):
        assert lp(C=bad) == EINVAL and la(C=bad) == EINVAL and pr(C=bad) == EINVAL
    for bad in (2, -1):
        assert lp(flip=bad) == EINVAL and la(flip=bad) == EINVAL and lp(virt=bad) == EINVAL and la(virt=bad) == EINVAL
    # nrows
    for nr in (0, -1, 10, 12):
        assert la(nr=nr) == ENOTSUP
    # sizes whose element or byte count overflows
    for bad in ((1 << 40, 13, 1 << 21), (1 << 62, 13, 4), (1, 1 << 61, 1), (1, (1 << 64) - 1, 1)):
        assert lp(shape=bad) == EINVAL and la(shape=bad) == EINVAL and pr(shape=bad) == EINVAL
    assert pr(shape=(1 << 55, 8, 1), C=5) == EINVAL
    # overlap: an output inside the bits or the level, inside the table, a row inside an output
    nb, kv = outer * k * inner, k + 1
    assert lp(o_=a) == EINVAL and lp(o_=a + (nb - 1) * eb) == EINVAL and lp(o_=tb) == EINVAL and lp(o_=tb + ((C - 1) * 2 * kv - 1) * eb) == EINVAL
    assert la(o_=a) == EINVAL and la(o_=a + (nb - 1) * eb) == EINVAL and la(o_=tb + ((C - 1) * 2 * kv - 1) * eb) == EINVAL
    assert la(o_=rw) == EINVAL and la(o_=rw + (C * outer * (kv // 2) * inner - 1) * eb) == EINVAL
    assert la(rows_=(ctypes.c_void_p * 3)(rw, o + 8, rw)) == EINVAL and la(rows_=(ctypes.c_void_p * 3)(o, rw, rw)) == EINVAL
    assert pr(o_=a) == EINVAL and pr(o_=a + (C * nb - 1) * eb) == EINVAL
    torch.cuda.synchronize()
    assert bool((A == 0x5a).all()) and bool((O == 0x3c).all()) and bool((R == 0x77).all()) and bool((T == 0x11).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    for empty in ((0, k, inner), (outer, k, 0)):
        assert lp(b_=None, t_=None, o_=None, shape=empty) == OK and la(b_=None, t_=None, rows_=None, o_=None, shape=empty) == OK
        assert pr(l_=None, o_=None, shape=empty) == OK
    torch.cuda.synchronize()
    assert bool((A == 0x5a).all()) and bool((O == 0x3c).all())
    # binary fields
    for mod in (0x11b, (1 << 64) | 0x1b, (1 << 128) | 0x87):
        bctx = engine.FieldContext(mod, True, device=0)
        G = torch.full((8192,), 0x42, dtype=torch.uint8, device='cuda')
        g = G.data_ptr()
        brow, one = (ctypes.c_void_p * 1)(g + 2048), bctx._scalars([1])
        bL, bh = bctx._L, bctx._h
        assert bL.ffgpu_find_leaf_prod(bh, g, g + 1024, g + 4096, 1, 8, 1, 2, 0, 1, st) == ENOTSUP
        assert bL.ffgpu_find_leaf_apply(bh, g, g + 1024, brow, one, 1, g + 4096, 1, 8, 1, 2, 0, 1, st) == ENOTSUP
        assert bL.ffgpu_find_prod(bh, g, g + 4096, 1, 8, 1, 2, st) == ENOTSUP
        torch.cuda.synchronize()
        assert bool((G == 0x42).all())
        with pytest.raises(ValueError):
            bctx.find_table(2, [0, 1], [1, 2])
    # the engine's own checks
    x = ctx.from_ints(list(range(outer * k * inner)))
    tab = ctx.find_table(k, list(range(k)), list(range(1, k + 1)), -1)
    assert tab.to_ints() == list(range(k)) + [p - 1] + [1] * k + [0]
    comp = ctx.from_ints(list(range(2 * outer * 7 * inner)))
    for bad in (lambda: ctx.find_leaf_prod(x, tab, outer, k + 1, inner, 2, 0, 1),
                lambda: ctx.find_leaf_prod(x, tab, outer, k, inner, 2, 0, 0),                  # (the table has k + 1 columns)
                lambda: ctx.find_leaf_prod(x, tab, outer, k, inner, 3, 0, 1),
                lambda: ctx.find_leaf_prod(x, tab, outer, k, inner, 6, 0, 1),
                lambda: ctx.find_leaf_prod(x, tab, outer, k, inner, 2, 2, 1),
                lambda: ctx.find_leaf_prod(x, tab, 0, k, inner, 2, 0, 1),
                lambda: ctx.find_leaf_prod(x, tab, outer, k, inner, 2, 0, 1, out=ctx.empty(5)),
                lambda: ctx.find_leaf_apply(x, tab, [ctx.empty(5)], [1], outer, k, inner, 2, 0, 1),
                lambda: ctx.find_leaf_apply(x, tab, [], [], outer, k, inner, 2, 0, 1),
                lambda: ctx.find_leaf_apply(x, tab, [comp], [1, 1], outer, k, inner, 2, 0, 1),
                lambda: ctx.find_prod(x, outer, k, inner, 2),
                lambda: ctx.find_prod(comp, outer, 7, inner, 2, out=ctx.empty(5)),
                lambda: ctx.find_prod(comp, 2 * outer * 7 * inner, 1, 1, 2)):
        with pytest.raises(ValueError):
            bad()
    assert ctx.find_leaf_prod(x, tab, outer, k, inner, 2, 0, 1).n == comp.n == ctx.find_leaf_apply(x, tab, [comp], [1], outer, k, inner, 2, 0, 1).n
    assert ctx.find_prod(comp, outer, 7, inner, 2).n == 2 * outer * 3 * inner


# ---- the protocol -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus', [2**61 - 1, 2**136 - 113], ids=['2^61-1', '2^136-113'])
@pytest.mark.parametrize('m,t', [(3, 1), (7, 3)])
def test_find_end_to_end(mods, modulus, m, t):
    """the recorded cases (bits and integers) and (1000, 31, 1): every variant opens, from any t + 1 parties, to numpy's values
    and to what the reference returned"""
    _ffi, engine, finfields, protocols = mods
    from oracle import pyoracle as po
    F = finfields.GF(modulus)
    ctx = engine.FieldContext(modulus, device=0)
    rng = random.Random(100 + m)
    l = 16
    sh = lambda v: protocols.share(ctx, ctx.from_ints([int(x) % modulus for x in v]), t, m)
    signed = lambda v: v - modulus if v > modulus // 2 else v
    picks = (list(range(t + 1)), sorted(rng.sample(range(m), t + 1)), list(range(m - t - 1, m)))
    lams = [[int(v) for v in po.recombination_vector(po.Field(modulus, False), [i + 1 for i in pick], 0)] for pick in picks]

    def rand(count):
        return (sh([rng.randrange(2) for _ in range(count * l)]), None, sh([rng.randrange(1 << 24) for _ in range(count)]), None)

    def opens_to(shares, want, what):
        """any t+1 shares recombine to `want`"""
        want = [int(v) for v in np.asarray(want).reshape(-1)]
        assert len(shares) == m and all(s.n == len(want) for s in shares), what
        for pick, lam in zip(picks, lams):
            assert [signed(v) for v in ctx.recombine([shares[i] for i in pick], lam).to_ints()] == want, (what, pick)

    arrays = [(np.array(c['bits'], dtype=np.int64).reshape(c['shape']), c) for c in golden_cases()]
    arrays.append((random_bits(rng, (1000, 31, 1)), None))
    for plain, case in arrays:
        outer, k, inner = plain.shape
        xs = sh(plain.reshape(-1))
        before = [x.t.clone() for x in xs]
        for s in (0, 1):
            ix, found = first_index(plain, s)
            for key, kw, want in variants(k):
                res = protocols.find(ctx, F, xs, outer, k, inner, t, s=s, **kw)
                flat = []
                for x in (res if isinstance(res, tuple) else (res,)):
                    flat += list(x) if isinstance(x, tuple) else [x]
                exp = [want(int(i), bool(f)) for i, f in zip(ix.reshape(-1), found.reshape(-1))]
                exp = [list(v) for v in zip(*exp)] if isinstance(exp[0], tuple) else [exp]
                assert len(flat) == len(exp), (key, plain.shape)
                if case is not None:
                    assert exp == recorded(case, s, key), (key, plain.shape, 'numpy and the reference disagree')
                for shares, e in zip(flat, exp):
                    opens_to(shares, e, (key, s, plain.shape))
        assert all(torch.equal(x.t, b) for x, b in zip(xs, before)), 'find wrote its input'
        if case is not None:                              # bits=False: the first 2 among integers in -3..3
            ints = np.array(case['ints'], dtype=np.int64).reshape(case['shape'])
            ys = sh(ints.reshape(-1))
            got = protocols.find(ctx, F, ys, outer, k, inner, t, s=case['ints_s'], e=-1, bits=False, l=l, rand=rand)
            ix, found = first_index(ints, case['ints_s'])
            assert np.where(found, ix, -1).reshape(-1).tolist() == case['ints_e_minus1']
            opens_to(got, case['ints_e_minus1'], ('bits=False', plain.shape))
    with pytest.raises(ValueError):
        protocols.find(ctx, F, xs[:2 * t], outer, k, inner, t)
    with pytest.raises(ValueError):
        protocols.find(ctx, F, xs, outer, k + 1, inner, t)


def test_graph_capture_replays_a_round_trip(mods):
    """leaf_prod -> split_rng -> leaf_apply -> find_prod for three parties, the products opened (degree 2t, so the bytes do not
    depend on the coefficients drawn): captured once, replayed on inputs changed in between, the same bytes as the eager run
    and as the integer model"""
    _ffi, engine, finfields, protocols = mods
    from oracle import pyoracle as po
    p = 2**64 - 189
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(21)
    outer, k, inner, C, flip, virt, m, t = 2, 8, 64, 3, 1, 1, 3, 1
    kv = k + virt
    kc = kv // 2 + kv % 2
    lam = [int(v) for v in po.recombination_vector(po.Field(p, False), [1, 2, 3], 0)]
    bits = [ctx.empty(outer * k * inner) for _ in range(m)]
    for b in bits:
        b.t.zero_()
    tab = ctx.empty((C - 1) * 2 * kv)
    tab.t.zero_()
    state = ctx.rng_state()

    def trip():
        prod = [ctx.find_leaf_prod(b, tab, outer, k, inner, C, flip, virt) for b in bits]
        sub = [ctx.split_rng(x, t, m, state=state) for x in prod]
        level = [ctx.find_leaf_apply(bits[j], tab, [sub[i].row(j) for i in range(m)], lam, outer, k, inner, C, flip, virt) for j in range(m)]
        return ctx.recombine([ctx.find_prod(x, outer, kc, inner, C) for x in level], lam)

    cg = engine.CapturedLaunches(trip)
    for _ in range(2):
        B = rng.integers(0, 2, size=(outer, k, inner)).astype(object)
        T = draw(rng, p, (C - 1) * 2 * kv).reshape(C - 1, 2, kv)
        for b, x in zip(bits, protocols.share(ctx, ctx.from_ints(B.reshape(-1)), t, m)):
            b.t.copy_(x.t)
        tab.t.copy_(ctx.from_ints(T.reshape(-1)).t)
        kept = [b.t.clone() for b in bits]
        LV = leaves_ref(p, B, T, flip, virt)
        N = apply_ref(p, LV, prod_ref(p, LV))
        want = ctx.from_ints(prod_ref(p, N).reshape(-1))
        assert same(trip(), want.t)                       # uncaptured
        cg.result.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        assert same(cg.result, want.t) and all(torch.equal(b.t, x) for b, x in zip(bits, kept))
