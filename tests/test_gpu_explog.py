"""The local steps under the secure logarithm and exponential on the device (ffgm_powers_prod / _poly_dot / _pow_base /
_bits_reverse, mpyc_amd/csrc/explog.hpp) against Python integers computed here from the maps include/ffgpu_math.h states, over
every prime policy; guard bytes around every output, inputs unchanged, views at odd element offsets, status codes,
protocols.powers / log / exp2 / pow_public_base end to end for all parties on one GPU against the same calls on the
Python-integer stand-in with the same randomness and against the reference's values (tests/golden/explog/explog.json), and
one ladder round with the Taylor sum replayed from a captured HIP graph."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_sgn import FIELDS, draw, same, view
from test_gpu_fxp import E2E, edge, recombine_ref, up
from test_explog_host import ExpRun, golden, ladder_model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ALL_N = (1, 63, 64, 65, 255, 256, 257, 5003)
PAD_N = (1, 64, 257, 5003)                                  # also with rows n + 3 elements apart
NMAX = 5003
PROD_HW = ((1, 1), (2, 2), (3, 2), (4, 4), (5, 4), (8, 8), (21, 10))
THETAS = (1, 2, 3, 9, 10, 21, 64)
REV_L = (1, 2, 3, 17, 32, 33, 64)
EBITS = (1, 3, 4, 5, 31, 32, 33, 64, 65)
SHIFTS = (0, 1, 16)


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


class Rows:
    """64 rows of NMAX field elements on the device, row-major at pitch NMAX, with their Python integers"""

    def __init__(self, ctx, p, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.p = ctx, p
        self.host = [edge(p, draw(rng, p, NMAX)) if j % 3 == 0 else draw(rng, p, NMAX) for j in range(64)]
        self.dev = up(ctx, np.concatenate(self.host))

    def block(self, engine, rows, n, stride, extra=0, lead=0):
        """a fresh block: `lead` unused elements, then rows 0..rows-1 cut to n elements, `stride` apart, then room for `extra`
        more rows; everything that is not a row holds row 63's values.  Returns (the view past `lead`, the whole buffer)"""
        ctx = self.ctx
        total = lead + (rows + extra) * stride
        buf = ctx.empty(total)
        fill = self.dev.t[63 * NMAX:64 * NMAX]
        for at in range(0, total, NMAX):
            k = min(NMAX, total - at)
            buf.t[at:at + k].copy_(fill[:k])
        for j in range(rows):
            buf.t[lead + j * stride:lead + j * stride + n].copy_(self.dev.t[j * NMAX:j * NMAX + n])
        return view(engine, ctx, buf, lead, total), buf


# ---- powers_prod -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FIELDS))
def test_powers_prod_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    R = Rows(ctx, p, seed=11 + p % 997)
    ran = 0
    for h, w in PROD_HW:
        want = up(ctx, np.concatenate([R.host[h - 1] * R.host[j] % p for j in range(w)]))
        want_rows = lambda n: torch.cat([want.t[j * NMAX:j * NMAX + n] for j in range(w)])
        for n in ALL_N:
            for stride in ((n, n + 3) if n in PAD_N else (n,)):
                P, buf = R.block(engine, h, n, stride)
                keep = buf.t.clone()
                got = ctx.powers_prod(P, n, h, w, stride=stride)
                assert same(got, want_rows(n)), (name, h, w, n, stride)
                assert torch.equal(buf.t, keep), 'powers_prod wrote its input'
                ran += 1
            # the output in rows h.. of the same block
            P, buf = R.block(engine, h, n, n, extra=w)
            out = view(engine, ctx, P, h * n, (h + w) * n)
            assert ctx.powers_prod(P, n, h, w, out=out) is out
            assert same(out, want_rows(n)), ('in the block', name, h, w, n)
            assert all(torch.equal(P.t[j * n:(j + 1) * n], R.dev.t[j * NMAX:j * NMAX + n]) for j in range(h)), 'the rows read were written'
        # one element into the buffers: the element path for 8- and 24-byte elements
        n = 2048
        P, buf = R.block(engine, h, n, n, lead=1)
        out = view(engine, ctx, ctx.empty(w * n + 1), 1, 1 + w * n)
        ctx.powers_prod(P, n, h, w, out=out)
        assert same(out, want_rows(n)), ('offset view', name, h, w)
    assert ran == len(PROD_HW) * (len(ALL_N) + len(PAD_N))


# ---- poly_dot ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FIELDS))
def test_poly_dot_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    R = Rows(ctx, p, seed=13 + p % 997)
    rng = np.random.default_rng(14)
    for i, theta in enumerate(THETAS):
        coefs = [int(v) for v in draw(rng, p, theta)]
        for at, v in zip(range(theta - 1, -1, -1), (p - 1, 1, 0)):             # planted from the last coefficient down
            coefs[at] = v
        c0 = (0, p - 1, int(draw(rng, p, 1)[0]))[i % 3]
        tab = ctx.poly_table(coefs)
        acc = sum(c * R.host[j] for j, c in enumerate(coefs))
        want = up(ctx, (acc + c0) % p)
        for n in ALL_N:
            for stride in ((n, n + 3) if n in PAD_N else (n,)):
                P, buf = R.block(engine, theta, n, stride)
                keep = buf.t.clone()
                got = ctx.poly_dot(P, n, tab, c0, stride=stride)
                assert same(got, want.t[:n]), (name, theta, n, stride)
                assert torch.equal(buf.t, keep) and tab.to_ints() == coefs, 'poly_dot wrote an input'
        n = 2048
        P, buf = R.block(engine, theta, n, n, lead=1)
        out = view(engine, ctx, ctx.empty(n + 1), 1, 1 + n)
        ctx.poly_dot(P, n, tab, c0, out=out)
        assert same(out, want.t[:n]), ('offset view', name, theta)
    for c0 in (0, p - 1):                                                       # both constants at the largest sum
        coefs = [p - 1] * 64
        got = ctx.poly_dot(R.dev, NMAX, ctx.poly_table(coefs), c0)
        assert same(got, up(ctx, (c0 - sum(R.host)) % p).t), (name, 'p - 1 everywhere', c0)


# ---- pow_base ------------------------------------------------------------------------------------------------------------------
def planted_exponents(p, ebits, shift):
    nwin = (ebits + 3) // 4
    vals = [0, 1, (1 << ebits) - 1, 1 << (ebits - 1), int('f' * max(nwin - 1, 1), 16) & ((1 << ebits) - 1), 15 & ((1 << ebits) - 1)]
    out = []
    for v in vals:
        for low in (0, (1 << shift) - 1):
            x = (v << shift) | low
            if x < p:
                out.append(x)
    return out


@pytest.mark.parametrize('name', list(FIELDS))
def test_pow_base_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(15 + p % 997)
    bases = (2, 3, p - 1)
    ebits_all = sorted({e for e in EBITS if e <= p.bit_length()} | {p.bit_length()})
    seen = set()
    for i, ebits in enumerate(ebits_all):
        for k in range(2 if i % 2 == 0 else 1):
            shift, g = SHIFTS[(i + k) % 3], bases[(i // 2 + 2 * k) % 3]
            seen.add(('s', shift)), seen.add(('g', g))
            x = draw(rng, p, NMAX)
            plant = planted_exponents(p, ebits, shift)
            x[:len(plant)] = plant
            x[300:300 + len(plant)] = plant                                     # beyond the first workgroup too
            mask = (1 << ebits) - 1
            want = up(ctx, np.array([pow(g, (int(v) >> shift) & mask, p) for v in x], dtype=object))
            dx, tab = up(ctx, x), ctx.pow_table(g, ebits)
            assert tab.n == 15 * ((ebits + 3) // 4) and tab.to_ints()[:2] == [g % p, g * g % p]
            keep = (dx.t.clone(), tab.t.clone())
            for n in ALL_N:
                got = ctx.pow_base(view(engine, ctx, dx, 0, n), tab, ebits, shift=shift)
                assert same(got, want.t[:n]), (name, ebits, shift, g, n)
            n = 2048
            out = view(engine, ctx, ctx.empty(n + 1), 1, 1 + n)
            ctx.pow_base(view(engine, ctx, dx, 1, 1 + n), tab, ebits, shift=shift, out=out)
            assert same(out, want.t[1:1 + n]), ('offset view', name, ebits, shift, g)
            assert torch.equal(dx.t, keep[0]) and torch.equal(tab.t, keep[1]), 'pow_base wrote an input'
    assert seen == {('s', s) for s in SHIFTS} | {('g', g) for g in bases}
    for bad in (0, p.bit_length() + 1):
        with pytest.raises(ValueError):
            ctx.pow_table(2, bad)


# ---- bits_reverse ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FIELDS))
def test_bits_reverse_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    for l in REV_L:
        rng = np.random.default_rng(5000 + l)
        bits = edge(p, draw(rng, p, NMAX * l))                                   # shares of bits are arbitrary field elements
        dbits, want = up(ctx, bits), up(ctx, bits.reshape(NMAX, l)[:, ::-1].reshape(-1))
        keep = dbits.t.clone()
        for n in ALL_N:
            got = ctx.bits_reverse(view(engine, ctx, dbits, 0, n * l), l)
            assert same(got, want.t[:n * l]), (name, l, n)
        n = 257
        out = view(engine, ctx, ctx.empty(n * l + 1), 1, 1 + n * l)
        ctx.bits_reverse(view(engine, ctx, dbits, l, (n + 1) * l), l, out=out)
        assert same(out, want.t[l:(n + 1) * l]), ('offset view', name, l)
        assert torch.equal(dbits.t, keep), 'bits_reverse wrote its input'


# ---- guard bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
def test_nothing_is_written_outside_the_outputs(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    h, w, theta, l, n, pad = 5, 4, 9, 17, 300, 240               # 240: a multiple of every element size and of 16
    ebits, shift = min(33, p.bit_length()), 1
    ctx = engine.FieldContext(p, device=0)
    eb = ctx.elem_bytes
    rng = np.random.default_rng(78)
    rows = [draw(rng, p, n) for _ in range(theta)]
    coefs, c0 = [int(v) for v in draw(rng, p, theta)], int(draw(rng, p, 1)[0])
    x, bits = draw(rng, p, n), draw(rng, p, n * l)
    dP, dx, dbits, tab, ptab = up(ctx, np.concatenate(rows)), up(ctx, x), up(ctx, bits), ctx.poly_table(coefs), ctx.pow_table(3, ebits)
    inputs = [dP, dx, dbits, tab, ptab]
    keep = [v.t.clone() for v in inputs]

    def guarded(nelem):
        buf = torch.full((pad + nelem * eb + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        return buf, buf.data_ptr() + pad

    def check(buf, nelem, want):
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + nelem * eb:] == 0xa5).all()), 'guard bytes written'
        assert torch.equal(buf[pad:pad + nelem * eb], up(ctx, want).t.contiguous().view(torch.uint8).reshape(-1))

    L, hd, st = ctx._L, ctx._h, ctx._stream()
    b1, p1 = guarded(w * n)
    assert L.ffgm_powers_prod(hd, dP.ptr, n, h, w, p1, n, st) == _ffi.OK
    check(b1, w * n, np.concatenate([rows[h - 1] * rows[j] % p for j in range(w)]))
    b2, p2 = guarded(n)
    assert L.ffgm_poly_dot(hd, dP.ptr, n, theta, tab.ptr, ctx._scalars([c0]), p2, n, st) == _ffi.OK
    check(b2, n, (sum(c * r for c, r in zip(coefs, rows)) + c0) % p)
    b3, p3 = guarded(n)
    assert L.ffgm_pow_base(hd, dx.ptr, shift, ebits, ptab.ptr, p3, n, st) == _ffi.OK
    check(b3, n, np.array([pow(3, (int(v) >> shift) & ((1 << ebits) - 1), p) for v in x], dtype=object))
    b4, p4 = guarded(n * l)
    assert L.ffgm_bits_reverse(hd, dbits.ptr, l, p4, n, st) == _ffi.OK
    check(b4, n * l, bits.reshape(n, l)[:, ::-1].reshape(-1))
    assert all(torch.equal(v.t, k) for v, k in zip(inputs, keep)), 'an input was written'


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p, n, hh, l = 2**61 - 1, 300, 4, 16
    ctx = engine.FieldContext(p, device=0)
    L, h, st = ctx._L, ctx._h, ctx._stream()
    eb = ctx.elem_bytes
    pat = lambda k: torch.full((k * eb,), 0x5a, dtype=torch.uint8, device='cuda')
    BLK, TAB, O1, X = pat(64 * n), pat(15 * 16), pat(64 * n), pat(n)
    blk, tab, o1, x = (b.data_ptr() for b in (BLK, TAB, O1, X))
    c0 = ctx._scalars([5])
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    prod = lambda P_=blk, s_=n, h_=hh, w_=2, o_=o1, n_=n: L.ffgm_powers_prod(h, P_, s_, h_, w_, o_, n_, st)
    dot = lambda P_=blk, s_=n, th=9, t_=tab, c_=c0, o_=o1, n_=n: L.ffgm_poly_dot(h, P_, s_, th, t_, c_, o_, n_, st)
    pw = lambda x_=x, sh=0, eb_=16, t_=tab, o_=o1, n_=n: L.ffgm_pow_base(h, x_, sh, eb_, t_, o_, n_, st)
    rev = lambda b_=blk, l_=l, o_=o1, n_=n: L.ffgm_bits_reverse(h, b_, l_, o_, n_, st)
    # counts out of range
    assert prod(h_=0, w_=0) == EINVAL and prod(w_=0) == EINVAL and prod(w_=hh + 1) == EINVAL and prod(h_=-1, w_=-1) == EINVAL
    assert dot(th=0) == EINVAL and dot(th=65) == EINVAL and dot(th=-1) == EINVAL
    assert pw(eb_=0) == EINVAL and pw(eb_=62) == EINVAL and pw(sh=-1) == EINVAL and pw(sh=192) == EINVAL
    assert rev(l_=0) == EINVAL and rev(l_=65) == EINVAL and rev(l_=-1) == EINVAL
    assert prod(s_=n - 1) == EINVAL and dot(s_=n - 1) == EINVAL                      # rows closer than n elements
    # a null context or required pointer
    assert L.ffgm_powers_prod(None, blk, n, hh, 2, o1, n, st) == EINVAL and L.ffgm_poly_dot(None, blk, n, 9, tab, c0, o1, n, st) == EINVAL
    assert L.ffgm_pow_base(None, x, 0, 16, tab, o1, n, st) == EINVAL and L.ffgm_bits_reverse(None, blk, l, o1, n, st) == EINVAL
    assert prod(P_=None) == EINVAL and prod(o_=None) == EINVAL
    assert dot(P_=None) == EINVAL and dot(t_=None) == EINVAL and dot(c_=None) == EINVAL and dot(o_=None) == EINVAL
    assert pw(x_=None) == EINVAL and pw(t_=None) == EINVAL and pw(o_=None) == EINVAL
    assert rev(b_=None) == EINVAL and rev(o_=None) == EINVAL
    # sizes overflowing
    for big in (1 << 62, 1 << 60):
        assert prod(n_=big, s_=big) == EINVAL and dot(n_=big, s_=big) == EINVAL and pw(n_=big) == EINVAL and rev(n_=big) == EINVAL
    assert prod(s_=1 << 62) == EINVAL and dot(s_=1 << 62) == EINVAL
    # overlaps: an output on an input
    assert prod(o_=blk) == EINVAL and prod(o_=blk + eb * (hh * n - 1)) == EINVAL and prod(o_=blk + eb * ((hh - 1) * n + 5)) == EINVAL
    assert dot(o_=blk + eb * (9 * n - 1)) == EINVAL and dot(o_=tab) == EINVAL and dot(o_=blk) == EINVAL
    assert pw(o_=x) == EINVAL and pw(o_=tab) == EINVAL and pw(o_=x + eb * (n - 1)) == EINVAL
    assert rev(o_=blk) == EINVAL and rev(o_=blk + eb * (n * l - 1)) == EINVAL
    torch.cuda.synchronize()
    for buf in (BLK, TAB, O1, X):
        assert bool((buf == 0x5a).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    assert prod(n_=0, s_=0, P_=None, o_=None) == OK and dot(n_=0, s_=0, P_=None, t_=None, o_=None) == OK
    assert pw(n_=0, x_=None, t_=None, o_=None) == OK and rev(n_=0, b_=None, o_=None) == OK
    assert pw(n_=0, eb_=61) == OK and rev(n_=0, l_=64) == OK and dot(n_=0, th=64) == OK      # the largest counts
    torch.cuda.synchronize()
    for buf in (BLK, TAB, O1, X):
        assert bool((buf == 0x5a).all())
    # valid calls, for contrast; the output of powers_prod may start right after the rows read
    TAB.zero_(), X.zero_()
    assert prod() == OK and prod(o_=blk + eb * hh * n) == OK and prod(w_=hh) == OK and prod(h_=1, w_=1) == OK
    assert dot() == OK and dot(th=1) == OK and dot(th=64, n_=4, s_=4) == OK and pw() == OK and pw(eb_=1) == OK and pw(sh=191) == OK
    assert rev() == OK and rev(l_=1) == OK and rev(l_=64, n_=4) == OK
    torch.cuda.synchronize()
    # binary fields
    for mod in (0x11b, (1 << 64) | 0x1b):
        bctx = engine.FieldContext(mod, True, device=0)
        g = torch.zeros(8192, dtype=torch.uint8, device='cuda').data_ptr()
        bl, bh = bctx._L, bctx._h
        one = bctx._scalars([1])
        assert bl.ffgm_powers_prod(bh, g, 4, 2, 2, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgm_poly_dot(bh, g, 4, 2, g + 2048, one, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgm_pow_base(bh, g, 0, 4, g + 2048, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgm_bits_reverse(bh, g, 4, g + 4096, 4, st) == ENOTSUP
    # the engine's own checks
    P, t9 = ctx.empty(hh * n), ctx.empty(9)
    for bad in (lambda: ctx.powers_prod(P, n, hh, hh + 1), lambda: ctx.powers_prod(P, n, hh + 1, 1), lambda: ctx.powers_prod(P, n, 0, 0),
                lambda: ctx.powers_prod(P, n, hh, 2, stride=n - 1), lambda: ctx.powers_prod(P, n, hh, 2, out=ctx.empty(5)),
                lambda: ctx.poly_dot(P, n, t9, 0), lambda: ctx.poly_dot(P, n, ctx.empty(0), 0), lambda: ctx.poly_dot(P, n, ctx.empty(65), 0),
                lambda: ctx.poly_dot(P, n, ctx.empty(3), 0, out=ctx.empty(5)), lambda: ctx.poly_table([]), lambda: ctx.poly_table([1] * 65),
                lambda: ctx.pow_base(P, ctx.empty(15), 5), lambda: ctx.pow_base(P, ctx.empty(30), 5, shift=192),
                lambda: ctx.pow_base(P, ctx.empty(30), 5, out=ctx.empty(5)), lambda: ctx.pow_base(P, ctx.empty(15 * 16), 62),
                lambda: ctx.bits_reverse(P, 7), lambda: ctx.bits_reverse(P, 0), lambda: ctx.bits_reverse(ctx.empty(130), 65),
                lambda: ctx.bits_reverse(P, 4, out=ctx.empty(5))):
        with pytest.raises(ValueError):
            bad()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def e2e_inputs(l, f, n):
    """the fixture's inputs first, then random ones of the same domains"""
    case = next(c for c in golden() if (c['l'], c['f']) == (l, f))
    rng = random.Random(l)
    log_in, exp2_in = list(case['log_in']), list(case['exp2_in'])
    while len(log_in) < n:
        bits = rng.randint(1, l - 1)
        log_in.append(rng.randrange(1 << (bits - 1), 1 << bits))
        exp2_in.append(rng.randrange((-f) << f, (l - 1 - f) << f))
    return case, log_in[:n], exp2_in[:n]


@pytest.mark.parametrize('name,l,f,m,t', E2E, ids=[f'{e[0]}-{e[1]}.{e[2]}-m{e[3]}' for e in E2E])
def test_protocols_end_to_end_against_the_stand_in(mods, name, l, f, m, t):
    """powers, log, exp2 and pow_public_base on the device and on the Python-integer stand-in, the same plain randomness fed to
    both: the opened values agree bit for bit (the sharing polynomials differ, the values cannot)"""
    _ffi, engine, finfields, protocols = mods
    from explog_cpuctx import ExplogCpuFieldContext
    p, n = FIELDS[name], 300
    case, log_in, exp2_in = e2e_inputs(l, f, n)
    vr = random.Random(f)
    ys = [vr.randint(-(3 << (f - 1)), 3 << (f - 1)) for _ in range(n)]
    bexp = [vr.randrange(0, l - 1 - f) << f for _ in range(n)]
    results = []
    for ctx in (engine.FieldContext(p, device=0), ExplogCpuFieldContext(p)):
        run = ExpRun(ctx, m, t, seed=l * 100 + m)
        xs = run.share(log_in)
        before = [x.to_ints() for x in xs]
        out = {'powers': run.open(protocols.powers(ctx, run.F, run.share(ys), 10, t, f, l, run.rand_trunc)),
               'log': run.open(protocols.log(ctx, run.F, xs, t, l, f, run.rand_bits, run.rand_trunc)),
               'exp2': run.open(protocols.exp2(ctx, run.F, run.share(exp2_in), t, l, f, run.rand_trunc, run.rand_exp)),
               'pow': run.open(protocols.pow_public_base(ctx, run.F, 2, run.share(bexp), t, l, f, run.rand_exp))}
        assert [x.to_ints() for x in xs] == before, 'an input was written'
        results.append(out)
    got, want = results
    for key in want:
        assert got[key] == want[key], (key, [h for h, (x, y) in enumerate(zip(got[key], want[key])) if x != y][:5])
    assert got['pow'] == [2**(b >> f) << f for b in bexp]


@pytest.mark.parametrize('name,l,f,m,t', E2E[:3], ids=[f'{e[0]}-{e[1]}.{e[2]}-m{e[3]}' for e in E2E[:3]])
def test_nearest_draws_on_the_device_equal_the_reference(mods, name, l, f, m, t):
    """the fixture's inputs with the nearest draw in every truncation: the device opens the reference's values bit for bit"""
    _ffi, engine, finfields, protocols = mods
    case = next(c for c in golden() if (c['l'], c['f']) == (l, f))
    ctx = engine.FieldContext(FIELDS[name], device=0)
    run = ExpRun(ctx, m, t, seed=l + m, nearest=True)
    assert run.open(protocols.log(ctx, run.F, run.share(case['log_in']), t, l, f, run.rand_bits, run.rand_trunc)) == case['log_nearest']
    assert run.open(protocols.exp2(ctx, run.F, run.share(case['exp2_in']), t, l, f, run.rand_trunc, run.rand_exp)) == case['exp2_nearest']
    vr = random.Random(f)
    ys = [0, 1, -1, 1 << f, -(1 << f)] + [vr.randint(-(1 << f), 1 << f) for _ in range(35)]      # |y| <= 1: every power is in range
    got = run.open(protocols.powers(ctx, run.F, run.share(ys), 21, t, f, l, run.rand_trunc))
    assert [[got[j * len(ys) + e] for j in range(21)] for e in range(len(ys))] == [ladder_model(y, 21, f) for y in ys]


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_a_ladder_round_and_the_taylor_sum(mods):
    """powers_prod -> the recombination of two received rows into rows h.. of the block -> poly_dot over all h + w rows, for
    one party, captured once, replayed on changed inputs"""
    _ffi, engine, _, _ = mods
    p, n, h, w = 2**80 - 65, 5003, 3, 2
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(21)
    block, other = ctx.empty((h + w) * n), ctx.empty(w * n)
    lam = [int(v) for v in draw(rng, p, 2)]
    coefs, c0 = [int(v) for v in draw(rng, p, h + w)], int(draw(rng, p, 1)[0])
    tab = ctx.poly_table(coefs)
    new = view(engine, ctx, block, h * n, (h + w) * n)

    def steps():
        prods = ctx.powers_prod(block, n, h, w)
        ctx.recombine([prods, other], lam, out=new)
        return prods, ctx.poly_dot(block, n, tab, c0)

    block.t.copy_(up(ctx, draw(rng, p, (h + w) * n)).t)
    other.t.copy_(up(ctx, draw(rng, p, w * n)).t)
    cg = engine.CapturedLaunches(steps)
    for _ in range(2):
        B, OT = draw(rng, p, (h + w) * n), draw(rng, p, w * n)
        block.t.copy_(up(ctx, B).t)
        other.t.copy_(up(ctx, OT).t)
        rows = [B[j * n:(j + 1) * n] for j in range(h)]
        prods = np.concatenate([rows[h - 1] * rows[j] % p for j in range(w)])
        fresh = recombine_ref(p, [prods, OT], lam)
        rows += [fresh[j * n:(j + 1) * n] for j in range(w)]
        for out in cg.result:
            out.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        assert same(cg.result[0], up(ctx, prods).t) and same(new, up(ctx, fresh).t)
        assert same(cg.result[1], up(ctx, (sum(c * r for c, r in zip(coefs, rows)) + c0) % p).t)
