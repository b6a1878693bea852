"""Bit decomposition over a prime field on the device (ffgpu_bits_mask / _expand / _finish, ffgpu_carry_prod / _apply,
mpyc_amd/csrc/bits.hpp) against Python integers computed here from the maps include/ffgpu.h states, over every prime
policy; guard bytes around every output and the rows of G and P a round does not name, status codes, protocols.to_bits
end to end for all parties on one GPU (the values and bits of tests/golden/bits/to_bits.json included), the same bytes from the
calls the engine had before (row copies, mul, recombine, add), one round trip replayed from a captured HIP graph, and two
and nine rows, the edges of the launcher's row dispatch, on both paths of carry_apply."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_sgn import FIELDS, draw, obj, same, sizes, view
from test_bits_host import golden, signed_values

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

# (these cross the 32-, 16-, 10-, 8- and 5-column chunks of the five element sizes)
ALL_L = (1, 2, 3, 7, 10, 11, 16, 32, 33, 64)
NMAX = 5003
NROWS = (1, 3, 7)
STEP = 4096


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def merges(l):
    """np_add_bits' recursion f(i, j, high) (runtime.py:4307-4327): its merges (i, h, j, high), left to right"""
    out = []

    def f(i, j, high):
        n = j - i
        if n == 1:
            return
        h = i + n // 2
        f(i, h, high)
        f(h, j, True)
        out.append((i, h, j, high))
    f(0, l, False)
    return sorted(out)


def level(l, rho):
    """(c-rows, d-rows) of round rho as lists of (k, q)"""
    c, d = [], []
    for i, h, j, high in merges(l):
        if (j - i - 1).bit_length() == rho:
            c += [(k, h - 1) for k in range(h, j)]
            d += [(k, h - 1) for k in range(h, j)] if high else []
    return c, d


def rounds(l):
    return (l - 1).bit_length()


def mask_ref(p, l, a, R, rd, offset):
    acc = obj([0] * len(a))
    for k in range(l):
        acc = acc + (R[:, k] << k)
    return (a + offset + (rd << l) - acc) % p


def expand_ref(p, l, c, R):
    cl = c & ((1 << l) - 1)
    n = len(c)
    G, P = np.empty((l, n), dtype=object), np.empty((l, n), dtype=object)
    for k in range(l):
        cb, r = (cl >> k) & 1, R[:, k]
        G[k] = np.where(cb == 1, r, 0)
        P[k] = np.where(cb == 1, (1 - r) % p, r)
    return G, P


def prod_ref(p, G, P, rows_c, rows_d):
    out = [G[q] * P[k] % p for k, q in rows_c] + [P[q] * P[k] % p for k, q in rows_d]
    return np.stack(out) if out else np.empty((0, G.shape[1]), dtype=object)


def apply_ref(p, G, P, rows, lam, rows_c, rows_d):
    """rows: nrows arrays (R, n); the new (G, P)"""
    v = sum(int(x) * r for x, r in zip(lam, rows)) % p
    G, P = G.copy(), P.copy()
    for j, (k, _) in enumerate(rows_c):
        G[k] = (G[k] + v[j]) % p
    for j, (k, _) in enumerate(rows_d):
        P[k] = v[len(rows_c) + j]
    return G, P


def finish_ref(p, l, c, R, G):
    cl = c & ((1 << l) - 1)
    out = np.empty(R.shape, dtype=object)
    for k in range(l):
        out[:, k] = (R[:, k] + ((cl >> k) & 1) - 2 * G[k] + (G[k - 1] if k else 0)) % p
    return out


class Data:
    """inputs of NMAX elements for one (field, l) with their expected outputs on the device; every smaller n is a prefix
    (rbits and the bits are element-major, G, P and the compact products column prefixes of bit-major matrices)"""

    def __init__(self, ctx, p, l, seed):
        rng = np.random.default_rng(seed)
        n = NMAX
        self.p, self.l, self.n = p, l, n
        self.a, self.rd, self.c = draw(rng, p, n), draw(rng, p, n), draw(rng, p, n)
        self.rb = draw(rng, p, n * l)
        edge = [0, p - 1, (1 << l) - 1, 1 << l, (1 << l) + 1, p - 2]
        self.c[1:1 + len(edge)] = edge                 # (c[0] stays random: n = 1)
        self.c[256:256 + len(edge)] = edge
        self.a[:3], self.rd[:3], self.rb[:3] = [0, p - 1, 1], [p - 1, 0, 1], [p - 1, 0, 1]
        self.offset = int(draw(rng, p, 1)[0]) if seed % 2 else (1 << l)
        R = self.rb.reshape(n, l)
        self.masked = mask_ref(p, l, self.a, R, self.rd, self.offset)
        self.G, self.P = expand_ref(p, l, self.c, R)
        # the level kernels and finish run on arbitrary field elements (shares are): G0 / P0, not the leaves
        self.G0, self.P0 = draw(rng, p, n * l).reshape(l, n), draw(rng, p, n * l).reshape(l, n)
        self.G0[0, :4], self.P0[0, :4] = [0, p - 1, 1, p - 2], [p - 1, p - 1, 0, 1]
        self.bits = finish_ref(p, l, self.c, R, self.G0)
        self.lam = [int(v) for v in draw(rng, p, max(NROWS))]
        self.lam[0] = p - 1
        # the sub-share rows of every round are windows of one pool, STEP elements apart (a multiple of every pack)
        self.levels = [level(l, rho) + (NROWS[rho % 3],) for rho in range(1, rounds(l) + 1)]
        maxr = max([len(c_) + len(d_) for c_, d_, _ in self.levels] or [0])
        pool = draw(rng, p, maxr * n + max(NROWS) * STEP)
        prods, self.changed = [], []
        for rc_, rd_, nr in self.levels:
            R = len(rc_) + len(rd_)
            v = sum(x * pool[s * STEP:s * STEP + R * n] for s, x in enumerate(self.lam[:nr])) % p
            v = v.reshape(R, n)
            prods.append(prod_ref(p, self.G0, self.P0, rc_, rd_))
            new = [(self.G0[k] + v[j]) % p for j, (k, _) in enumerate(rc_)] + [v[len(rc_) + j] for j in range(len(rd_))]
            self.changed.append(np.stack(new))
        up = lambda v: ctx.from_ints(np.asarray(v, dtype=object).reshape(-1))
        self.d = {k: up(getattr(self, k)) for k in ('a', 'rd', 'rb', 'c', 'masked', 'G', 'P', 'G0', 'P0', 'bits')}
        self.dpool = up(pool)
        self.dprod = [up(x) for x in prods]
        # what carry_apply leaves: G0 / P0 with the round's rows replaced (copies of uploaded rows, no device arithmetic)
        self.dg, self.dp = [], []
        for (rc_, rd_, _), new in zip(self.levels, self.changed):
            g2, p2, dn = self.d['G0'].clone(), self.d['P0'].clone(), up(new)
            shape = lambda x, rows: x.t.reshape((rows, n) + tuple(x.t.shape[1:]))
            for j, (k, _) in enumerate(rc_):
                shape(g2, l)[k] = shape(dn, len(rc_) + len(rd_))[j]
            for j, (k, _) in enumerate(rd_):
                shape(p2, l)[k] = shape(dn, len(rc_) + len(rd_))[len(rc_) + j]
            self.dg.append(g2), self.dp.append(p2)

    def rows(self, engine, ctx, rho, n):
        """the nr sub-share rows of round rho for the first n columns: contiguous compact (R, n) arrays"""
        rc_, rd_, nr = self.levels[rho - 1]
        R = len(rc_) + len(rd_)
        return [flat(engine, ctx, self.cols(view(engine, ctx, self.dpool, s * STEP, s * STEP + R * NMAX), R, n)) for s in range(nr)]

    @staticmethod
    def cols(x, nrows, n):
        """columns 0 .. n-1 of a device bit-major (nrows, NMAX) matrix, contiguous"""
        t = x.t
        return t.reshape((nrows, NMAX) + tuple(t.shape[1:]))[:, :n].contiguous()


def flat(engine, ctx, t2):
    """a contiguous (rows, n[, limbs]) tensor as a DevArray of rows * n elements"""
    tail = tuple(t2.shape[2:])
    t = t2.contiguous().reshape((t2.shape[0] * t2.shape[1],) + tail)
    return engine.DevArray(ctx, t, t.shape[0])


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    ran = 0
    for l in ALL_L:
        if l > p.bit_length() - 2:
            continue
        D = Data(ctx, p, l, seed=2000 + l)
        d = D.d
        for n in sizes():
            v = lambda k, per=1: view(engine, ctx, d[k], 0, n * per)
            tag = (name, l, n)
            assert same(ctx.bits_mask(v('a'), v('rb', l), v('rd'), l, D.offset), d['masked'].t[:n]), ('mask',) + tag
            g, pp = ctx.bits_expand(v('c'), v('rb', l), l)
            assert same(g, D.cols(d['G'], l, n)), ('expand g',) + tag
            assert same(pp, D.cols(d['P'], l, n)), ('expand p',) + tag
            g0, p0 = flat(engine, ctx, D.cols(d['G0'], l, n)), flat(engine, ctx, D.cols(d['P0'], l, n))
            assert same(ctx.bits_finish(v('c'), v('rb', l), g0, l), d['bits'].t[:n * l]), ('finish',) + tag
            assert ctx.carry_rounds(l) == rounds(l)
            for rho in range(1, rounds(l) + 1):
                rc_, rd_, nr = D.levels[rho - 1]
                R = len(rc_) + len(rd_)
                assert ctx.carry_level(l, rho) == (len(rc_), len(rd_), rc_ + rd_)
                assert same(ctx.carry_prod(g0, p0, l, rho), D.cols(D.dprod[rho - 1], R, n)), ('prod', rho) + tag
                g1, p1 = g0.clone(), p0.clone()
                rows = D.rows(engine, ctx, rho, n)
                got = ctx.carry_apply(g1, p1, rows, D.lam[:nr], l, rho)
                assert got[0] is g1 and got[1] is p1
                assert same(g1, D.cols(D.dg[rho - 1], l, n)), ('apply g', rho, nr) + tag
                assert same(p1, D.cols(D.dp[rho - 1], l, n)), ('apply p', rho, nr) + tag
            ran += 1
    assert ran >= 3 * len(sizes())


@pytest.mark.parametrize('name', ['pm64-k64', 'pm96', 'pm192'])
def test_views_at_odd_element_offsets_and_capped_grid(mods, monkeypatch, name):
    """G, P, the rows and the compact output one element into their buffers (8- and 24-byte elements are then not
    16-byte aligned: the element path), and FFGPU_BLOCKS_PER_CU=1 with n = 64 * 1024, where every thread of a level kernel
    takes several units -- aligned (packs, whole waves) and at the odd offset"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    rng = np.random.default_rng(31 + p % 997)
    monkeypatch.setenv('FFGPU_BLOCKS_PER_CU', '1')
    capped = engine.FieldContext(p, device=0)
    monkeypatch.delenv('FFGPU_BLOCKS_PER_CU')
    for ctx, l, n in ((engine.FieldContext(p, device=0), 7, 320), (capped, 3, 64 * 1024)):
        G, P = draw(rng, p, l * n).reshape(l, n), draw(rng, p, l * n).reshape(l, n)
        lam = [int(x) for x in draw(rng, p, 3)]
        for rho in range(1, rounds(l) + 1):
            rc_, rd_ = level(l, rho)
            R = len(rc_) + len(rd_)
            rows = [draw(rng, p, R * n).reshape(R, n) for _ in range(3)]
            want_prod = ctx.from_ints(prod_ref(p, G, P, rc_, rd_).reshape(-1))
            g2, p2 = apply_ref(p, G, P, rows, lam, rc_, rd_)
            want_g, want_p = ctx.from_ints(g2.reshape(-1)), ctx.from_ints(p2.reshape(-1))
            for offset in (0, 1):
                def put(vals, count):
                    buf = ctx.empty(count + offset)
                    buf.t[offset:].copy_(ctx.from_ints(vals.reshape(-1)).t)
                    return view(engine, ctx, buf, offset, offset + count)
                g, pp = put(G, l * n), put(P, l * n)
                out = view(engine, ctx, ctx.empty(R * n + offset), offset, offset + R * n)
                assert same(ctx.carry_prod(g, pp, l, rho, out=out), want_prod.t), (name, l, n, rho, offset)
                ctx.carry_apply(g, pp, [put(r, R * n) for r in rows], lam, l, rho)
                assert same(g, want_g.t) and same(pp, want_p.t), (name, l, n, rho, offset)


@pytest.mark.parametrize('name', ['pm64-k64', 'pm128', 'pm192'])
def test_two_and_nine_rows_on_both_paths(mods, name):
    """NROWS stops at seven; the launcher of carry_apply dispatches over 1 .. 9 rows, so both edges next to the ends: every
    round of l = 7 with two and with nine rows over 8-, 16- and 24-byte storage.  n = 64: the pack path (whole waves of
    24-byte elements); n = 65, and n = 64 one element into the buffers: the element path of 8- and 24-byte elements (a pack
    of 16-byte elements is one element, aligned at every element offset: they stay on the pack path)"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(37 + p % 997)
    l = 7
    for n, offset in ((64, 0), (65, 0), (64, 1)):
        def put(vals, count):
            buf = ctx.empty(count + offset)
            buf.t[offset:].copy_(ctx.from_ints(vals.reshape(-1)).t)
            return view(engine, ctx, buf, offset, offset + count)
        G, P = draw(rng, p, l * n).reshape(l, n), draw(rng, p, l * n).reshape(l, n)
        lam = [int(x) for x in draw(rng, p, 9)]
        for rho in range(1, rounds(l) + 1):
            rc_, rd_ = level(l, rho)
            R = len(rc_) + len(rd_)
            rows = [draw(rng, p, R * n).reshape(R, n) for _ in range(9)]
            drows = [put(r, R * n) for r in rows]
            keep = [x.t.clone() for x in drows]
            for nr in (2, 9):
                g2, p2 = apply_ref(p, G, P, rows[:nr], lam[:nr], rc_, rd_)
                g, pp = put(G, l * n), put(P, l * n)
                ctx.carry_apply(g, pp, drows[:nr], lam[:nr], l, rho)
                assert same(g, ctx.from_ints(g2.reshape(-1)).t) and same(pp, ctx.from_ints(p2.reshape(-1)).t), (name, n, offset, rho, nr)
            assert all(torch.equal(x.t, t) for x, t in zip(drows, keep)), 'a row was written'


@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
def test_nothing_is_written_outside_the_outputs(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    l, n, pad = min(16, p.bit_length() - 2), 300, 240          # 240: a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    eb = ctx.elem_bytes
    D = Data(ctx, p, l, seed=6)
    d = D.d
    before = {k: d[k].t.clone() for k in ('a', 'rd', 'rb', 'c')}

    def guarded(nelem, init=None):
        buf = torch.full((pad + nelem * eb + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        if init is not None:
            buf[pad:pad + nelem * eb] = init.contiguous().view(torch.uint8).reshape(-1)
        return buf, buf.data_ptr() + pad

    def check(buf, nelem, want_t):
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + nelem * eb:] == 0xa5).all()), 'guard bytes written'
        assert torch.equal(buf[pad:pad + nelem * eb], want_t.contiguous().view(torch.uint8).reshape(-1))

    L, h, st = ctx._L, ctx._h, ctx._stream()
    bm, pm = guarded(n)
    assert L.ffgpu_bits_mask(h, d['a'].ptr, d['rb'].ptr, d['rd'].ptr, ctx._scalars([D.offset]), l, pm, n, st) == _ffi.OK
    check(bm, n, d['masked'].t[:n])
    (bg, pg), (bp, pp) = guarded(l * n), guarded(l * n)
    assert L.ffgpu_bits_expand(h, d['c'].ptr, d['rb'].ptr, l, pg, pp, n, st) == _ffi.OK
    check(bg, l * n, D.cols(d['G'], l, n))
    check(bp, l * n, D.cols(d['P'], l, n))
    g0, p0 = flat(engine, ctx, D.cols(d['G0'], l, n)), flat(engine, ctx, D.cols(d['P0'], l, n))
    keep_g, keep_p = g0.t.clone(), p0.t.clone()
    bo, po = guarded(n * l)
    assert L.ffgpu_bits_finish(h, d['c'].ptr, d['rb'].ptr, g0.ptr, l, po, n, st) == _ffi.OK
    check(bo, n * l, d['bits'].t[:n * l])
    for rho in range(1, rounds(l) + 1):
        rc_, rd_, nr = D.levels[rho - 1]
        R = len(rc_) + len(rd_)
        bc, pc = guarded(R * n)
        assert L.ffgpu_carry_prod(h, g0.ptr, p0.ptr, l, rho, pc, n, st) == _ffi.OK
        check(bc, R * n, D.cols(D.dprod[rho - 1], R, n))
        assert torch.equal(g0.t, keep_g) and torch.equal(p0.t, keep_p), 'carry_prod wrote an operand'
        rows = D.rows(engine, ctx, rho, n)
        keep = [r.t.clone() for r in rows]
        (b1, q1), (b2, q2) = guarded(l * n, g0.t), guarded(l * n, p0.t)
        ptrs = (ctypes.c_void_p * nr)(*[r.ptr for r in rows])
        assert L.ffgpu_carry_apply(h, q1, q2, ptrs, ctx._scalars(D.lam[:nr]), nr, l, rho, n, st) == _ffi.OK
        # the whole arrays: the rows of G and P the round does not name keep their bytes
        check(b1, l * n, D.cols(D.dg[rho - 1], l, n))
        check(b2, l * n, D.cols(D.dp[rho - 1], l, n))
        untouched_g = [k for k in range(l) if k not in {k for k, _ in rc_}]
        untouched_p = [k for k in range(l) if k not in {k for k, _ in rd_}]
        gw, pw = D.cols(D.dg[rho - 1], l, n), D.cols(D.dp[rho - 1], l, n)
        g_in, p_in = D.cols(d['G0'], l, n), D.cols(d['P0'], l, n)
        assert all(torch.equal(gw[k], g_in[k]) for k in untouched_g) and all(torch.equal(pw[k], p_in[k]) for k in untouched_p)
        for r, t in zip(rows, keep):
            assert torch.equal(r.t, t), 'a row was written'
    for k, t in before.items():
        assert torch.equal(d[k].t, t), f'input {k} was written'


def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p, l, n = 2**61 - 1, 16, 300
    ctx = engine.FieldContext(p, device=0)
    D = Data(ctx, p, l, seed=7)
    d = D.d
    L, h, st = ctx._L, ctx._h, ctx._stream()
    eb = ctx.elem_bytes
    pat = lambda k: torch.full((k * eb,), 0x5a, dtype=torch.uint8, device='cuda')
    GB, PB, OB, MB, RB = pat(64 * n), pat(64 * n), pat(64 * n), pat(n), pat(64 * n)
    gp, pp, op, mp, rw = (x.data_ptr() for x in (GB, PB, OB, MB, RB))
    a, rb, rd, c = (d[k].ptr for k in ('a', 'rb', 'rd', 'c'))
    off = ctx._scalars([1 << l])
    rows = (ctypes.c_void_p * 12)(*([rw] * 12))
    lam = ctx._scalars([1] * 12)
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    mask = lambda l_=l, n_=n, a_=a, rb_=rb, rd_=rd, off_=off, o_=mp: L.ffgpu_bits_mask(h, a_, rb_, rd_, off_, l_, o_, n_, st)
    expand = lambda l_=l, n_=n, c_=c, rb_=rb, g_=gp, p_=pp: L.ffgpu_bits_expand(h, c_, rb_, l_, g_, p_, n_, st)
    finish = lambda l_=l, n_=n, c_=c, rb_=rb, g_=gp, o_=op: L.ffgpu_bits_finish(h, c_, rb_, g_, l_, o_, n_, st)
    prod = lambda l_=l, rho=1, n_=n, g_=gp, p_=pp, o_=op: L.ffgpu_carry_prod(h, g_, p_, l_, rho, o_, n_, st)
    appl = lambda l_=l, rho=1, n_=n, g_=gp, p_=pp, rows_=rows, lam_=lam, nr=3: L.ffgpu_carry_apply(h, g_, p_, rows_, lam_, nr, l_, rho,
                                                                                                   n_, st)
    # l out of range
    for bad in (0, 65, p.bit_length() - 1, -1):
        assert mask(l_=bad) == EINVAL and expand(l_=bad) == EINVAL and finish(l_=bad) == EINVAL
        assert prod(l_=bad) == EINVAL and appl(l_=bad) == EINVAL
    # round out of range
    for bad in (0, 5, -1, 64):
        assert prod(rho=bad) == EINVAL and appl(rho=bad) == EINVAL
    assert prod(l_=1, rho=1) == EINVAL and appl(l_=1, rho=1) == EINVAL                # l = 1 has no round
    # a null context or required pointer
    assert L.ffgpu_bits_mask(None, a, rb, rd, off, l, mp, n, st) == EINVAL
    assert L.ffgpu_bits_expand(None, c, rb, l, gp, pp, n, st) == EINVAL
    assert L.ffgpu_bits_finish(None, c, rb, gp, l, op, n, st) == EINVAL
    assert L.ffgpu_carry_prod(None, gp, pp, l, 1, op, n, st) == EINVAL
    assert L.ffgpu_carry_apply(None, gp, pp, rows, lam, 3, l, 1, n, st) == EINVAL
    assert mask(a_=None) == EINVAL and mask(rb_=None) == EINVAL and mask(rd_=None) == EINVAL and mask(o_=None) == EINVAL
    assert mask(off_=None) == EINVAL
    assert expand(c_=None) == EINVAL and expand(rb_=None) == EINVAL and expand(g_=None) == EINVAL and expand(p_=None) == EINVAL
    assert finish(c_=None) == EINVAL and finish(rb_=None) == EINVAL and finish(g_=None) == EINVAL and finish(o_=None) == EINVAL
    assert prod(g_=None) == EINVAL and prod(p_=None) == EINVAL and prod(o_=None) == EINVAL
    assert appl(g_=None) == EINVAL and appl(p_=None) == EINVAL and appl(rows_=None) == EINVAL and appl(lam_=None) == EINVAL
    assert appl(rows_=(ctypes.c_void_p * 3)(rw, None, rw)) == EINVAL
    # nrows
    assert appl(nr=0) == EINVAL and appl(nr=-1) == EINVAL
    assert appl(nr=10) == ENOTSUP and appl(nr=12) == ENOTSUP
    # n * l or its byte size overflowing
    for big in (1 << 62, 1 << 58):
        assert mask(n_=big) == EINVAL and expand(n_=big) == EINVAL and finish(n_=big) == EINVAL
        assert prod(n_=big) == EINVAL and appl(n_=big) == EINVAL
    # overlaps: an output on an input or on another output, a row on g or p, g on p
    assert mask(o_=a) == EINVAL and mask(o_=rb + eb * (n * l - 1)) == EINVAL and mask(o_=rd) == EINVAL
    assert expand(g_=rb) == EINVAL and expand(p_=c) == EINVAL and expand(p_=gp + eb * (n * l - 1)) == EINVAL and expand(g_=pp) == EINVAL
    assert finish(o_=rb) == EINVAL and finish(o_=gp) == EINVAL and finish(o_=c) == EINVAL
    assert prod(o_=gp) == EINVAL and prod(o_=pp + eb * (n * l - 1)) == EINVAL
    assert appl(rows_=(ctypes.c_void_p * 3)(rw, gp + 8, rw)) == EINVAL and appl(rows_=(ctypes.c_void_p * 3)(pp, rw, rw)) == EINVAL
    assert appl(p_=gp) == EINVAL and appl(p_=gp + eb * (n * l - 1)) == EINVAL
    torch.cuda.synchronize()
    for buf in (GB, PB, OB, MB, RB):
        assert bool((buf == 0x5a).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    assert mask(n_=0, a_=None, o_=None) == OK and expand(n_=0, g_=None) == OK and finish(n_=0, o_=None) == OK
    assert prod(n_=0, g_=None, o_=None) == OK and appl(n_=0, g_=None, rows_=None) == OK
    assert mask(l_=p.bit_length() - 2, n_=0) == OK                                  # the largest l
    torch.cuda.synchronize()
    for buf in (GB, PB, OB, MB, RB):
        assert bool((buf == 0x5a).all())
    # valid calls, for contrast (nine rows are served)
    assert mask() == OK and expand() == OK and finish() == OK and prod() == OK and appl() == OK and appl(nr=9) == OK
    assert prod(rho=4) == OK and appl(rho=4) == OK
    torch.cuda.synchronize()
    # binary fields
    for mod in (0x11b, (1 << 64) | 0x1b, (1 << 128) | 0x87):
        bctx = engine.FieldContext(mod, True, device=0)
        g = torch.zeros(8192, dtype=torch.uint8, device='cuda').data_ptr()
        bl, bh = bctx._L, bctx._h
        assert bl.ffgpu_bits_mask(bh, g, g + 512, g + 1024, bctx._scalars([1]), 4, g + 2048, 4, st) == ENOTSUP
        assert bl.ffgpu_bits_expand(bh, g, g + 512, 4, g + 2048, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgpu_bits_finish(bh, g, g + 512, g + 1024, 4, g + 2048, 4, st) == ENOTSUP
        assert bl.ffgpu_carry_prod(bh, g, g + 1024, 4, 1, g + 2048, 4, st) == ENOTSUP
        assert bl.ffgpu_carry_apply(bh, g, g + 1024, (ctypes.c_void_p * 1)(g + 2048), bctx._scalars([1]), 1, 4, 1, 4, st) == ENOTSUP
    # the engine's own checks
    with pytest.raises(ValueError):
        ctx.bits_mask(d['a'], d['rb'], d['rd'], l + 1, 1 << l)
    with pytest.raises(ValueError):
        ctx.bits_expand(d['c'], d['rb'], l - 1)
    with pytest.raises(ValueError):
        ctx.carry_prod(d['G0'], d['P0'], l, 5)
    with pytest.raises(ValueError):
        ctx.carry_prod(d['G0'], d['P0'], l, 1, out=ctx.empty(5))
    with pytest.raises(ValueError):
        ctx.carry_apply(d['G0'], d['P0'], [ctx.empty(5)], [1], l, 1)
    with pytest.raises(ValueError):
        ctx.carry_apply(d['G0'], d['P0'], [], [], l, 1)
    with pytest.raises(ValueError):
        ctx.bits_finish(d['c'], d['rb'], ctx.empty(5), l)
    with pytest.raises(ValueError):
        ctx.carry_rounds(65)


@pytest.mark.parametrize('modulus,l', [(2**61 - 1, 16), (2**64 - 189, 32)], ids=['2^61-1', '2^64-189'])
@pytest.mark.parametrize('m,t', [(3, 1), (7, 3)])
def test_to_bits_end_to_end(mods, modulus, l, m, t):
    """rdivl in [1, 2^24) and offset 2^l: a + 2^l + 2^l rdivl - r lies in (2^l rdivl - 2^l / 2, 2^l rdivl + 2^l 3/2), inside
    (0, p) for both fields: the opened value does not wrap"""
    _ffi, engine, finfields, protocols = mods
    from oracle import pyoracle as po
    F = finfields.GF(modulus)
    ctx = engine.FieldContext(modulus, device=0)
    rng = random.Random(l * 100 + m)
    n = 1031
    gold = golden()[l]
    a = signed_values(rng, l, n - len(gold['values'])) + gold['values']
    want = [[(v >> k) & 1 for k in range(l)] for v in a]
    assert want[n - len(gold['values']):] == gold['bits']
    want = [b for row in want for b in row]
    sh = lambda vals: protocols.share(ctx, ctx.from_ints([v % modulus for v in vals]), t, m)
    xs, rbits = sh(a), sh([rng.randrange(2) for _ in range(n * l)])
    rdivl = sh([rng.randrange(1, 1 << 24) for _ in range(n)])
    before = [x.t.clone() for x in xs + rbits + rdivl]
    out = protocols.to_bits(ctx, F, xs, rbits, rdivl, t, l)
    assert len(out) == m and all(o.n == n * l for o in out)
    assert all(torch.equal(x.t, b) for x, b in zip(xs + rbits + rdivl, before)), 'to_bits wrote its inputs'
    assert protocols.open_(ctx, F, out, t).to_ints() == want                               # bit k of a mod 2^l
    for pick in (sorted(rng.sample(range(m), t + 1)), list(range(m - t - 1, m))):          # any t+1 shares
        lam = [int(v) for v in po.recombination_vector(po.Field(modulus, False), [i + 1 for i in pick], 0)]
        assert ctx.recombine([out[i] for i in pick], lam).to_ints() == want, pick
    assert protocols.open_(ctx, F, protocols.from_bits(ctx, out, l), t).to_ints() == [v % (1 << l) for v in a]
    with pytest.raises(ValueError):
        protocols.to_bits(ctx, F, xs[:2 * t], rbits[:2 * t], rdivl[:2 * t], t, l)


def composed_round(engine, ctx, g, p, l, n, rho, rows, lam):
    """one round from the calls the engine had before: row copies for the gather, mul, recombine + add"""
    rc_, rd_ = level(l, rho)
    row = lambda x, k: engine.DevArray(ctx, x.t[k * n:(k + 1) * n], n)

    def cat(ts):
        t = torch.cat([x.t for x in ts])
        return engine.DevArray(ctx, t, t.shape[0])
    left = cat([row(g, q) for _, q in rc_] + [row(p, q) for _, q in rd_])
    right = cat([row(p, k) for k, _ in rc_ + rd_])
    prod = ctx.mul(left, right)
    v = ctx.recombine(rows, lam)
    g2, p2 = g.clone(), p.clone()
    for j, (k, _) in enumerate(rc_):
        ctx.add(row(g, k), row(v, j), out=row(g2, k))
    for j, (k, _) in enumerate(rd_):
        row(p2, k).t.copy_(row(v, len(rc_) + j).t)
    return prod, g2, p2


@pytest.mark.parametrize('modulus,l', [(2**64 - 189, 32), (2**80 - 65, 33)], ids=['2^64-189', '2^80-65'])
def test_same_bytes_as_the_composition_of_existing_calls(mods, modulus, l):
    """every step equals, bit for bit, what the calls of the engine that existed before compute for the same inputs; the
    public c_bits are built on the host and uploaded, as the reference's np_to_bits does"""
    _ffi, engine, finfields, protocols = mods
    ctx = engine.FieldContext(modulus, device=0)
    F = finfields.GF(modulus)
    rng = random.Random(l)
    n, t, m = 1031, 1, 3
    p = modulus
    sh = lambda vals: protocols.share(ctx, ctx.from_ints([v % modulus for v in vals]), t, m)
    xs, rbits = sh(signed_values(rng, l, n)), sh([rng.randrange(2) for _ in range(n * l)])
    rdivl = sh([rng.randrange(1, 1 << 24) for _ in range(n)])
    lam = [int(v) for v in protocols._lagrange(F, range(1, 2 * t + 2))]
    pw = ctx.from_ints([1 << k for k in range(l)])
    masked = [ctx.bits_mask(xs[i], rbits[i], rdivl[i], l, 1 << l) for i in range(m)]
    c = protocols.open_(ctx, F, masked, t)
    cl = [v & ((1 << l) - 1) for v in c.to_ints()]
    CB = ctx.from_ints([(v >> k) & 1 for k in range(l) for v in cl])                    # bit-major
    CBe = ctx.from_ints([(v >> k) & 1 for v in cl for k in range(l)])                   # element-major
    for i in range(m):
        r_modl = ctx.matmul(rbits[i], pw, n, l, 1)
        want = ctx.sub(ctx.add(ctx.add_scalar(xs[i], 1 << l), ctx.mul_scalar(rdivl[i], (1 << l) % p)), r_modl)
        assert same(masked[i], want.t)
        rt = rbits[i].t.reshape((n, l) + tuple(rbits[i].t.shape[1:])).transpose(0, 1).contiguous()
        rT = engine.DevArray(ctx, rt.reshape((n * l,) + tuple(rbits[i].t.shape[1:])), n * l)
        g_want = ctx.mul(CB, rT)
        p_want = ctx.sub(ctx.add(CB, rT), ctx.mul_scalar(g_want, 2))
        g, pp = ctx.bits_expand(c, rbits[i], l)
        assert same(g, g_want.t) and same(pp, p_want.t)
        for rho in range(1, rounds(l) + 1):
            R = ctx.carry_rows(l, rho)
            rows = [ctx.from_ints([rng.randrange(p) for _ in range(R * n)]) for _ in range(2 * t + 1)]
            prod, g2, p2 = composed_round(engine, ctx, g, pp, l, n, rho, rows, lam)
            assert same(ctx.carry_prod(g, pp, l, rho), prod.t), rho
            ctx.carry_apply(g, pp, rows, lam, l, rho)
            assert same(g, g2.t) and same(pp, p2.t), rho
        # a + b - 2c + c_shifted, element-major: the transposes of the reference's layout
        tail = tuple(g.t.shape[1:])
        gT = g.t.reshape((l, n) + tail).transpose(0, 1).contiguous()
        sT = torch.zeros_like(gT)
        sT[:, 1:] = gT[:, :-1]
        el = lambda x: engine.DevArray(ctx, x.reshape((n * l,) + tail), n * l)
        want = ctx.add(ctx.sub(ctx.add(rbits[i], CBe), ctx.mul_scalar(el(gT), 2)), el(sT))
        assert same(ctx.bits_finish(c, rbits[i], g, l), want.t)


def test_graph_capture_replays_one_round_trip(mods):
    _ffi, engine, _, _ = mods
    p, l, n = 2**64 - 189, 32, 5003
    ctx = engine.FieldContext(p, device=0)
    D = Data(ctx, p, l, seed=9)
    d = D.d
    rho = 2
    rc_, rd_, nr = D.levels[rho - 1]
    R = len(rc_) + len(rd_)
    rows = [ctx.empty(R * n) for _ in range(nr - 1)]
    lam = D.lam[:nr]
    c, rb = d['c'].clone(), d['rb'].clone()

    def steps():
        masked = ctx.bits_mask(d['a'], rb, d['rd'], l, D.offset)
        g, pp = ctx.bits_expand(c, rb, l)
        prod = ctx.carry_prod(g, pp, l, rho)
        ctx.carry_apply(g, pp, [prod] + rows, lam, l, rho)
        return masked, g, pp, prod, ctx.bits_finish(c, rb, g, l)

    cg = engine.CapturedLaunches(steps)
    rng = np.random.default_rng(4)
    for _ in range(2):
        C, RB = draw(rng, p, n), draw(rng, p, n * l)
        Rw = [draw(rng, p, R * n).reshape(R, n) for _ in rows]
        c.t.copy_(ctx.from_ints(C).t)
        rb.t.copy_(ctx.from_ints(RB).t)
        for x, v in zip(rows, Rw):
            x.t.copy_(ctx.from_ints(v.reshape(-1)).t)
        Rm = RB.reshape(n, l)
        G, P = expand_ref(p, l, C, Rm)
        prod = prod_ref(p, G, P, rc_, rd_)
        G2, P2 = apply_ref(p, G, P, [prod] + Rw, lam, rc_, rd_)
        want = (mask_ref(p, l, D.a, Rm, D.rd, D.offset), G2, P2, prod, finish_ref(p, l, C, Rm, G2))
        for out in cg.result:
            out.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        for out, w in zip(cg.result, want):
            assert same(out, ctx.from_ints(np.asarray(w, dtype=object).reshape(-1)).t)
