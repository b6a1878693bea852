"""Fixed-point truncation and the gate of the normalisation on the device (ffgpu_trunc_mask / _trunc_finish, ffgpu_norm_prod /
_norm_apply, mpyc_amd/csrc/fxp.hpp) against Python integers computed here from the maps include/ffgpu.h states, over every
prime policy; guard bytes around every output, inputs unchanged, views at odd element offsets, status codes, bits_mask after
sharing its body with trunc_mask, protocols.trunc / fxp_multiply / norm / reciprocal / divide end to end for all parties on one
GPU against the same calls on the Python-integer stand-in with the same randomness (the reference's _norm values of
tests/golden/fxp/fxp.json included), and one truncation replayed from a captured HIP graph."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_sgn import FIELDS, draw, obj, same, sizes, view
from test_fxp_host import Run, golden, norm_model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

# (these cross the 32-, 16-, 10-, 8- and 5-column chunks of the five element sizes)
ALL_F = (1, 2, 3, 7, 10, 11, 16, 32, 33, 64)
MASK_N = (1, 63, 64, 255, 256, 257, 5003)                 # the tile of 256 and a partial wave
FINISH_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5003)
FINISH_F = (1, 31, 32, 33, 63, 64)
NROWS = (1, 2, 3, 4, 7, 9)
NORM_L = (2, 3, 4, 5, 17, 32, 33, 64)
NORM_N = (1, 2, 63, 64, 65, 257, 5003)
NMAX = 5003


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def test_sizes_cover_the_tile():
    assert set(sizes()) <= set(MASK_N) | {1, 63, 257, NMAX}


def up(ctx, vals):
    return ctx.from_ints(np.asarray(vals, dtype=object).reshape(-1))


# ---- the maps of include/ffgpu.h on Python integers ----------------------------------------------------------------------------
def trunc_mask_ref(p, f, a, R, rd, offset):
    acc = obj([0] * len(a))
    for k in range(f):
        acc = acc + (R[:, k] << k)
    ar = (a + acc) % p
    return ar, (ar + offset + (rd << f)) % p


def recombine_ref(p, rows, lam):
    return sum(int(x) * r for x, r in zip(lam, rows)) % p


def trunc_finish_ref(p, f, c, ar):
    return (ar - (c & ((1 << f) - 1))) * pow(1 << f, -1, p) % p


def norm_prod_ref(p, l, bits):
    B = bits.reshape(-1, l)
    top = B[:, l - 1]
    out = ((2 * top - 1)[:, None] * B[:, :l - 1][:, ::-1]) % p
    return out.reshape(-1), (1 - 2 * top) % p


def norm_apply_ref(p, l, bits, v):
    top = bits.reshape(-1, l)[:, l - 1]
    return ((1 - top)[:, None] + v.reshape(-1, l - 1)) % p


def edge(p, x):
    """field elements with both extremes in front"""
    x[:4] = [0, p - 1, 1, p - 2][:len(x)]
    return x


# ---- trunc_mask ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FIELDS))
def test_trunc_mask_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    ran = 0
    for f in ALL_F:
        if f > p.bit_length() - 2:
            with pytest.raises(ValueError):
                ctx.trunc_mask(ctx.empty(1), ctx.empty(f), ctx.empty(1), f, 0)
            continue
        rng = np.random.default_rng(3000 + f)
        a, rd, rb = edge(p, draw(rng, p, NMAX)), edge(p, draw(rng, p, NMAX))[::-1].copy(), draw(rng, p, NMAX * f)
        rb[:3] = [p - 1, 0, 1][:len(rb)]
        offset = int(draw(rng, p, 1)[0]) if f % 2 else (1 << (f + 7)) % p
        ar, masked = trunc_mask_ref(p, f, a, rb.reshape(NMAX, f), rd, offset)
        d = {k: up(ctx, v) for k, v in (('a', a), ('rd', rd), ('rb', rb), ('ar', ar), ('masked', masked))}
        keep = {k: d[k].t.clone() for k in ('a', 'rd', 'rb')}
        for n in MASK_N:
            v = lambda k, per=1: view(engine, ctx, d[k], 0, n * per)
            got_ar, got = ctx.trunc_mask(v('a'), v('rb', f), v('rd'), f, offset)
            assert same(got_ar, d['ar'].t[:n]), ('ar', name, f, n)
            assert same(got, d['masked'].t[:n]), ('masked', name, f, n)
            ran += 1
        assert all(torch.equal(d[k].t, keep[k]) for k in keep), 'trunc_mask wrote an input'
    assert ran >= 3 * len(MASK_N)


# ---- trunc_finish ------------------------------------------------------------------------------------------------------------------
class FinishData:
    """nine rows of NMAX elements, ar, and per (f, nrows) the expected output; the first elements of row 0 are solved so that
    the recombined c has its low f bits all ones, all zeros, and is p - 1"""

    def __init__(self, ctx, p, seed):
        rng = np.random.default_rng(seed)
        self.p, self.ctx = p, ctx
        self.rows = [draw(rng, p, NMAX) for _ in range(max(NROWS))]
        self.ar = edge(p, draw(rng, p, NMAX))
        self.lam = [int(v) for v in draw(rng, p, max(NROWS))]
        self.lam[0] = p - 1
        self.dar = up(ctx, self.ar)
        self.drows = [up(ctx, r) for r in self.rows]

    def case(self, f, nrows):
        """(device row 0 for this case, lambdas, expected output on the device)"""
        p = self.p
        lam = [1] if nrows == 1 else self.lam[:nrows]
        row0 = self.rows[0].copy()
        targets = [(1 << f) - 1, ((p - 1) >> f) << f, p - 1, 0, (1 << f) % p, ((1 << f) - 1) ^ 1]
        inv0 = pow(lam[0], -1, p)
        for h, tgt in enumerate(targets):
            for at in (1 + h, 257 + h):                # (element 0 stays random: n = 1; the second tile too)
                rst = recombine_ref(p, [r[at:at + 1] for r in self.rows[1:nrows]], lam[1:])[0] if nrows > 1 else 0
                row0[at] = (tgt - rst) * inv0 % p
        c = recombine_ref(p, [row0] + self.rows[1:nrows], lam)
        assert [int(c[1 + h]) for h in range(len(targets))] == [t % p for t in targets]
        return up(self.ctx, row0), lam, up(self.ctx, trunc_finish_ref(p, f, c, self.ar))


@pytest.mark.parametrize('name', list(FIELDS))
def test_trunc_finish_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    D = FinishData(ctx, p, seed=41 + p % 1009)
    keep = [r.t.clone() for r in D.drows] + [D.dar.t.clone()]
    ran = 0
    for i, f in enumerate(FINISH_F):
        if f > p.bit_length() - 2:
            continue
        for nrows in (NROWS if i % 2 == 0 else NROWS[i % 3::3]):
            row0, lam, want = D.case(f, nrows)
            for n in FINISH_N:
                rows = [view(engine, ctx, r, 0, n) for r in [row0] + D.drows[1:nrows]]
                got = ctx.trunc_finish(rows, lam, view(engine, ctx, D.dar, 0, n), f)
                assert same(got, want.t[:n]), (name, f, nrows, n)
                ran += 1
            # views one element into their buffers: 8- and 24-byte elements are then not 16-byte aligned (the element path)
            n = 2048
            rows = [view(engine, ctx, r, 1, 1 + n) for r in [row0] + D.drows[1:nrows]]
            out = view(engine, ctx, ctx.empty(n + 1), 1, 1 + n)
            ctx.trunc_finish(rows, lam, view(engine, ctx, D.dar, 1, 1 + n), f, out=out)
            assert same(out, want.t[1:1 + n]), ('offset view', name, f, nrows)
    assert ran >= len(FINISH_N) * 4
    assert all(torch.equal(x.t, k) for x, k in zip(D.drows + [D.dar], keep)), 'trunc_finish wrote an input'
    with pytest.raises(NotImplementedError):
        ctx.trunc_finish([D.drows[0]] * 10, [1] * 10, D.dar, 1)


# ---- norm_prod / norm_apply ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FIELDS))
def test_norm_kernels_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    lam_all = [int(v) for v in draw(np.random.default_rng(5), p, max(NROWS))]
    lam_all[0] = p - 1
    for i, l in enumerate(NORM_L):
        rng = np.random.default_rng(4000 + l)
        bits = draw(rng, p, NMAX * l)                    # shares of bits are arbitrary field elements
        bits[:4] = [0, p - 1, 1, p - 2][:4]
        bits[l - 1] = p - 1
        prod, sign = norm_prod_ref(p, l, bits)
        nrows = NROWS[i % len(NROWS)]
        lam = [1] if nrows == 1 else lam_all[:nrows]
        rows = [draw(rng, p, NMAX * (l - 1)) for _ in range(nrows)]
        applied = norm_apply_ref(p, l, bits, recombine_ref(p, rows, lam)).reshape(-1)
        dbits, dprod, dsign, dapp = up(ctx, bits), up(ctx, prod), up(ctx, sign), up(ctx, applied)
        drows = [up(ctx, r) for r in rows]
        keep = [x.t.clone() for x in [dbits] + drows]
        for n in NORM_N:
            b = view(engine, ctx, dbits, 0, n * l)
            out, sg = ctx.norm_prod(b, l)
            assert same(out, dprod.t[:n * (l - 1)]) and same(sg, dsign.t[:n]), ('prod', name, l, n)
            out2, none = ctx.norm_prod(b, l, want_sign=False)                # sign_out NULL
            assert none is None and same(out2, dprod.t[:n * (l - 1)]), ('prod without sign', name, l, n)
            got = ctx.norm_apply(b, [view(engine, ctx, r, 0, n * (l - 1)) for r in drows], lam, l)
            assert same(got, dapp.t[:n * (l - 1)]), ('apply', name, l, nrows, n)
        # one element into the buffers: the element path for 8- and 24-byte elements
        n = 257
        out = view(engine, ctx, ctx.empty(n * (l - 1) + 1), 1, 1 + n * (l - 1))
        ctx.norm_prod(view(engine, ctx, dbits, 0, n * l), l, want_sign=False, out=out)
        assert same(out, dprod.t[:n * (l - 1)]), ('prod at an odd offset', name, l)
        shifted = []
        for r in drows:
            buf = ctx.empty(n * (l - 1) + 1)
            buf.t[1:].copy_(r.t[:n * (l - 1)])
            shifted.append(view(engine, ctx, buf, 1, 1 + n * (l - 1)))
        ctx.norm_apply(view(engine, ctx, dbits, 0, n * l), shifted, lam, l, out=out)
        assert same(out, dapp.t[:n * (l - 1)]), ('apply at an odd offset', name, l)
        assert all(torch.equal(x.t, k) for x, k in zip([dbits] + drows, keep)), 'a norm kernel wrote an input'
    with pytest.raises(NotImplementedError):
        ctx.norm_apply(ctx.empty(4), [ctx.empty(2)] * 10, [1] * 10, 2)


# ---- guard bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
def test_nothing_is_written_outside_the_outputs(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    f, l, n, pad = min(16, p.bit_length() - 2), 17, 300, 240     # 240: a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    eb = ctx.elem_bytes
    rng = np.random.default_rng(77)
    a, rd, rb, bits = draw(rng, p, n), draw(rng, p, n), draw(rng, p, n * f), draw(rng, p, n * l)
    rows = [draw(rng, p, n * (l - 1)) for _ in range(3)]
    lam = [int(v) for v in draw(rng, p, 3)]
    offset = int(draw(rng, p, 1)[0])
    ar, masked = trunc_mask_ref(p, f, a, rb.reshape(n, f), rd, offset)
    c = recombine_ref(p, [r[:n] for r in rows], lam)
    prod, sign = norm_prod_ref(p, l, bits)
    applied = norm_apply_ref(p, l, bits, recombine_ref(p, rows, lam)).reshape(-1)
    da, drd, drb, dbits, dar = (up(ctx, v) for v in (a, rd, rb, bits, ar))
    drows = [up(ctx, r) for r in rows]
    inputs = [da, drd, drb, dbits, dar] + drows
    keep = [x.t.clone() for x in inputs]

    def guarded(nelem):
        buf = torch.full((pad + nelem * eb + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        return buf, buf.data_ptr() + pad

    def check(buf, nelem, want):
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + nelem * eb:] == 0xa5).all()), 'guard bytes written'
        assert torch.equal(buf[pad:pad + nelem * eb], up(ctx, want).t.contiguous().view(torch.uint8).reshape(-1))

    L, h, st = ctx._L, ctx._h, ctx._stream()
    ptrs = lambda xs: (ctypes.c_void_p * len(xs))(*[x.ptr for x in xs])
    (b1, p1), (b2, p2) = guarded(n), guarded(n)
    assert L.ffgpu_trunc_mask(h, da.ptr, drb.ptr, drd.ptr, ctx._scalars([offset]), f, p1, p2, n, st) == _ffi.OK
    check(b1, n, ar), check(b2, n, masked)
    b3, p3 = guarded(n)
    short = [view(engine, ctx, r, 0, n) for r in drows]
    assert L.ffgpu_trunc_finish(h, ptrs(short), ctx._scalars(lam), 3, dar.ptr, f, p3, n, st) == _ffi.OK
    check(b3, n, trunc_finish_ref(p, f, c, ar))
    (b4, p4), (b5, p5) = guarded(n * (l - 1)), guarded(n)
    assert L.ffgpu_norm_prod(h, dbits.ptr, l, p4, p5, n, st) == _ffi.OK
    check(b4, n * (l - 1), prod), check(b5, n, sign)
    b6, p6 = guarded(n * (l - 1))
    assert L.ffgpu_norm_prod(h, dbits.ptr, l, p6, None, n, st) == _ffi.OK
    check(b6, n * (l - 1), prod)
    b7, p7 = guarded(n * (l - 1))
    assert L.ffgpu_norm_apply(h, dbits.ptr, ptrs(drows), ctx._scalars(lam), 3, l, p7, n, st) == _ffi.OK
    check(b7, n * (l - 1), applied)
    assert all(torch.equal(x.t, k) for x, k in zip(inputs, keep)), 'an input was written'


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p, f, l, n = 2**61 - 1, 16, 16, 300
    ctx = engine.FieldContext(p, device=0)
    L, h, st = ctx._L, ctx._h, ctx._stream()
    eb = ctx.elem_bytes
    pat = lambda k: torch.full((k * eb,), 0x5a, dtype=torch.uint8, device='cuda')
    IN, RB, O1, O2, RW = pat(n), pat(64 * n), pat(64 * n), pat(64 * n), pat(64 * n)
    a, rb, o1, o2, rw = (x.data_ptr() for x in (IN, RB, O1, O2, RW))
    off, lam = ctx._scalars([1 << 31]), ctx._scalars([1] * 12)
    rows = (ctypes.c_void_p * 12)(*([rw] * 12))
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    mask = lambda f_=f, n_=n, a_=a, rb_=rb, rd_=a, off_=off, ar_=o1, o_=o2: L.ffgpu_trunc_mask(h, a_, rb_, rd_, off_, f_, ar_, o_, n_, st)
    fin = lambda f_=f, n_=n, rows_=rows, lam_=lam, nr=3, ar_=a, o_=o1: L.ffgpu_trunc_finish(h, rows_, lam_, nr, ar_, f_, o_, n_, st)
    prod = lambda l_=l, n_=n, b_=rb, o_=o1, s_=o2: L.ffgpu_norm_prod(h, b_, l_, o_, s_, n_, st)
    appl = lambda l_=l, n_=n, b_=rb, rows_=rows, lam_=lam, nr=3, o_=o1: L.ffgpu_norm_apply(h, b_, rows_, lam_, nr, l_, o_, n_, st)
    # a bit count out of range
    for bad in (0, 65, p.bit_length() - 1, -1):
        assert mask(f_=bad) == EINVAL and fin(f_=bad) == EINVAL
    for bad in (1, 0, 65, -1):
        assert prod(l_=bad) == EINVAL and appl(l_=bad) == EINVAL
    # a null context or required pointer
    assert L.ffgpu_trunc_mask(None, a, rb, a, off, f, o1, o2, n, st) == EINVAL
    assert L.ffgpu_trunc_finish(None, rows, lam, 3, a, f, o1, n, st) == EINVAL
    assert L.ffgpu_norm_prod(None, rb, l, o1, o2, n, st) == EINVAL
    assert L.ffgpu_norm_apply(None, rb, rows, lam, 3, l, o1, n, st) == EINVAL
    assert mask(a_=None) == EINVAL and mask(rb_=None) == EINVAL and mask(rd_=None) == EINVAL and mask(off_=None) == EINVAL
    assert mask(ar_=None) == EINVAL and mask(o_=None) == EINVAL                      # both outputs are required
    assert fin(rows_=None) == EINVAL and fin(lam_=None) == EINVAL and fin(ar_=None) == EINVAL and fin(o_=None) == EINVAL
    assert fin(rows_=(ctypes.c_void_p * 3)(rw, None, rw)) == EINVAL
    assert prod(b_=None) == EINVAL and prod(o_=None) == EINVAL
    assert appl(b_=None) == EINVAL and appl(rows_=None) == EINVAL and appl(lam_=None) == EINVAL and appl(o_=None) == EINVAL
    assert appl(rows_=(ctypes.c_void_p * 3)(rw, rw, None)) == EINVAL
    # nrows
    assert fin(nr=0) == EINVAL and fin(nr=-1) == EINVAL and appl(nr=0) == EINVAL and appl(nr=-1) == EINVAL
    assert fin(nr=10) == ENOTSUP and fin(nr=12) == ENOTSUP and appl(nr=10) == ENOTSUP and appl(nr=12) == ENOTSUP
    # n * f / n * l or its byte size overflowing
    for big in (1 << 62, 1 << 58):
        assert mask(n_=big) == EINVAL and fin(n_=big) == EINVAL and prod(n_=big) == EINVAL and appl(n_=big) == EINVAL
    # overlaps: an output on an input, a row or another output
    assert mask(ar_=a) == EINVAL and mask(o_=rb + eb * (n * f - 1)) == EINVAL and mask(o_=o1) == EINVAL and mask(ar_=o2 + eb * (n - 1)) == EINVAL
    assert fin(o_=a) == EINVAL and fin(o_=rw + eb * (n - 1)) == EINVAL
    assert prod(o_=rb) == EINVAL and prod(o_=rb + eb * (n * l - 1)) == EINVAL and prod(s_=rb) == EINVAL and prod(s_=o1 + eb * (n * (l - 1) - 1)) == EINVAL
    assert appl(o_=rb) == EINVAL and appl(o_=rw + eb * (n * (l - 1) - 1)) == EINVAL
    torch.cuda.synchronize()
    for buf in (IN, RB, O1, O2, RW):
        assert bool((buf == 0x5a).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    assert mask(n_=0, a_=None, o_=None) == OK and fin(n_=0, rows_=None, o_=None) == OK
    assert prod(n_=0, b_=None, o_=None) == OK and appl(n_=0, rows_=None, o_=None) == OK
    assert mask(f_=p.bit_length() - 2, n_=0) == OK and prod(l_=64, n_=0) == OK       # the largest bit counts
    torch.cuda.synchronize()
    for buf in (IN, RB, O1, O2, RW):
        assert bool((buf == 0x5a).all())
    # valid calls, for contrast (nine rows are served, sign_out may be NULL)
    assert mask() == OK and fin() == OK and fin(nr=9) == OK and fin(nr=1) == OK
    assert prod() == OK and prod(s_=None) == OK and appl() == OK and appl(nr=9) == OK and prod(l_=2) == OK and appl(l_=64, n_=4) == OK
    torch.cuda.synchronize()
    # binary fields
    for mod in (0x11b, (1 << 64) | 0x1b):
        bctx = engine.FieldContext(mod, True, device=0)
        g = torch.zeros(8192, dtype=torch.uint8, device='cuda').data_ptr()
        bl, bh = bctx._L, bctx._h
        one, r1 = bctx._scalars([1]), (ctypes.c_void_p * 1)(g + 2048)
        assert bl.ffgpu_trunc_mask(bh, g, g + 512, g + 1024, one, 4, g + 2048, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgpu_trunc_finish(bh, r1, one, 1, g, 4, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgpu_norm_prod(bh, g, 4, g + 2048, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgpu_norm_apply(bh, g, r1, one, 1, 4, g + 4096, 4, st) == ENOTSUP
    # the engine's own checks
    x, bits = ctx.empty(n), ctx.empty(n * l)
    for bad in (lambda: ctx.trunc_mask(x, bits, x, f + 1, 0), lambda: ctx.trunc_mask(x, bits, ctx.empty(5), f, 0),
                lambda: ctx.trunc_finish([], [], x, f), lambda: ctx.trunc_finish([ctx.empty(5)], [1], x, f),
                lambda: ctx.trunc_finish([x], [1], x, f, out=ctx.empty(5)), lambda: ctx.norm_prod(bits, 7),
                lambda: ctx.norm_prod(bits, 1), lambda: ctx.norm_prod(bits, l, out=ctx.empty(5)),
                lambda: ctx.norm_apply(bits, [x], [1], l), lambda: ctx.norm_apply(bits, [], [], l)):
        with pytest.raises(ValueError):
            bad()


# ---- bits_mask shares its body with trunc_mask ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rc32', 'pm64-mersenne', 'pm96', 'mont128', 'pm192'])
def test_bits_mask_gives_what_it_gave(mods, name):
    """one case per element size: masked = a + offset + rdivl 2^l - sum_k rbits 2^k, and ar + (that) = 2 a + offset + rdivl 2^l
    ties the two kernels to each other"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    l, n = min(11, p.bit_length() - 2), 1031
    rng = np.random.default_rng(9)
    a, rd, rb = edge(p, draw(rng, p, n)), draw(rng, p, n), draw(rng, p, n * l)
    offset = int(draw(rng, p, 1)[0])
    acc = obj([0] * n)
    for k in range(l):
        acc = acc + (rb.reshape(n, l)[:, k] << k)
    da, drd, drb = up(ctx, a), up(ctx, rd), up(ctx, rb)
    got = ctx.bits_mask(da, drb, drd, l, offset)
    assert same(got, up(ctx, (a + offset + (rd << l) - acc) % p).t)
    ar, _ = ctx.trunc_mask(da, drb, drd, l, offset)
    assert same(ctx.add(ar, got), up(ctx, (2 * a + offset + (rd << l)) % p).t)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
E2E = [('pm96', 32, 16, 3, 1), ('pm64-mersenne', 16, 8, 3, 1), ('pm64-mersenne', 16, 8, 7, 3), ('pm128', 32, 16, 3, 1),
       ('pm192', 32, 16, 3, 1)]


def e2e_values(l, f, n):
    """the golden denominators and numerators first, then random ones with representable reciprocals"""
    case = next(c for c in golden() if (c['l'], c['f']) == (l, f))
    rng = random.Random(l)
    den, num = list(case['den']), list(case['num'])
    lo = 1 << (2 * f - l + 1)
    while len(den) < n:
        v = rng.randrange(lo + 1, 1 << (l - 1)) * rng.choice((1, -1))
        den.append(v)
        num.append(rng.randrange(-(abs(v) << max(l - f - 3, 0)), (abs(v) << max(l - f - 3, 0)) + 1) >> 1)
    return case, den[:n], [max(-(1 << (l - 2)), min(1 << (l - 2), v)) for v in num[:n]]


@pytest.mark.parametrize('name,l,f,m,t', E2E, ids=[f'{e[0]}-{e[1]}.{e[2]}-m{e[3]}' for e in E2E])
def test_protocols_end_to_end_against_the_stand_in(mods, name, l, f, m, t):
    """trunc, fxp_multiply, norm, reciprocal and divide on the device and on the Python-integer stand-in, the same plain
    randomness fed to both: the opened values agree bit for bit (the sharing polynomials differ, the values cannot)"""
    _ffi, engine, finfields, protocols = mods
    from fxp_cpuctx import FxpCpuFieldContext
    p, n = FIELDS[name], 300
    case, den, num = e2e_values(l, f, n)
    dev, cpu = engine.FieldContext(p, device=0), FxpCpuFieldContext(p)
    lim, vr = 1 << ((l + f - 2) // 2), random.Random(f)                    # factors whose product has l + f - 1 signed bits
    u, w = [[vr.randint(-lim, lim) for _ in range(n)] for _ in range(2)]
    results = []
    for ctx in (dev, cpu):
        run = Run(ctx, m, t, seed=l * 100 + m)
        xs, ys = run.share(den), run.share(num)
        before = [x.to_ints() for x in xs]
        rbits, rdivf = run.rand_trunc(n, f)
        out = {'trunc': run.open(protocols.trunc(ctx, run.F, xs, rbits, rdivf, t, f, l)),
               'mul': run.open(protocols.fxp_multiply(ctx, run.F, run.share(u), run.share(w), t, f, l, run.rand_trunc)),
               'norm': run.open(protocols.norm(ctx, run.F, xs, t, l, f, run.rand_bits)),
               'rec': run.open(protocols.reciprocal(ctx, run.F, xs, t, l, f, run.rand_bits, run.rand_trunc)),
               'div': run.open(protocols.divide(ctx, run.F, ys, xs, t, l, f, run.rand_bits, run.rand_trunc))}
        assert [x.to_ints() for x in xs] == before, 'an input was written'
        results.append(out)
    got, want = results
    for key in want:
        assert got[key] == want[key], (key, [h for h, (x, y) in enumerate(zip(got[key], want[key])) if x != y][:5])
    assert got['norm'] == [norm_model(a, l, f) for a in den] and got['norm'][:len(case['den'])] == case['den_norm']
    assert all(y in (a >> f, (a >> f) + 1) for a, y in zip(den, got['trunc']))


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_one_truncation(mods):
    """mask -> finish for one party (its own masked share and one received row), captured once, replayed on changed inputs"""
    _ffi, engine, _, _ = mods
    p, f, n = 2**80 - 65, 16, 5003
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(12)
    a, rb, rd, other = (ctx.empty(k) for k in (n, n * f, n, n))
    lam = [int(v) for v in draw(rng, p, 2)]
    offset = 1 << 47

    def steps():
        ar, masked = ctx.trunc_mask(a, rb, rd, f, offset)
        return ar, masked, ctx.trunc_finish([masked, other], lam, ar, f)

    for x, k in ((a, n), (rb, n * f), (rd, n), (other, n)):
        x.t.copy_(up(ctx, draw(rng, p, k)).t)
    cg = engine.CapturedLaunches(steps)
    for _ in range(2):
        A, RB, RD, OT = draw(rng, p, n), draw(rng, p, n * f), draw(rng, p, n), draw(rng, p, n)
        for x, v in ((a, A), (rb, RB), (rd, RD), (other, OT)):
            x.t.copy_(up(ctx, v).t)
        ar, masked = trunc_mask_ref(p, f, A, RB.reshape(n, f), RD, offset)
        want = (ar, masked, trunc_finish_ref(p, f, recombine_ref(p, [masked, OT], lam), ar))
        for out in cg.result:
            out.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        for out, w in zip(cg.result, want):
            assert same(out, up(ctx, w).t)
