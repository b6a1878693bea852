"""The local steps under secure unit vectors and table lookup at secret indices on the device (ffgm_unit_prod / ffgm_unit_roll /
ffgm_unit_dot, mpyc_amd/csrc/unitvec.hpp) against Python integers computed here from the maps include/ffgpu_math.h states, over
every prime policy and element size; outputs and U at aligned pointers and one element off; guard bytes around every output,
inputs unchanged; status codes with nothing written on refusal; the three calls replayed from one captured HIP graph; and
protocols.unit_vectors / unit_vectors_from_bits (behind to_bits) / lookup for all parties on one GPU, on every index value and on
the inputs of the fixture recorded from the reference (tests/golden/unit/unit.json).

The operands of a case are drawn from a pool of Python-integer field elements by index, so that a large array costs one
device gather, not one conversion per element: the expected products of unit_prod are a table of Python-integer products of
the two pools, placed by the same indices; the expected output of unit_roll is the pool at indices moved by Python-integer
index arithmetic on the Python integers c; the sums of unit_dot are formed in Python integers outright."""
import random

import numpy as np
import pytest

from test_gpu_sgn import draw, same, view
from test_gpu_fxp import up
from test_gpu_bsgn import FIELDS
from test_unitvec_host import KS, UnitDraws, check_fixture, columns, golden
from test_rbits_host import gf, open_two_ways
from test_sort_host import _share

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

POOL, XPOOL = 509, 8
LAZY32 = ('pm96', 'pm128', 'pm192')                       # DotAcc<F>::FLUSH == 32: the multi-limb 2^k - c primes; 192 elsewhere
BY_SIZE = ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192']  # one field per element size: 4, 8, 12, 16, 24 bytes


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def flush_of(name):
    return 32 if name in LAZY32 else 192


class Pool:
    """POOL field elements as Python integers and on the device; arrays of them by index"""

    def __init__(self, engine, ctx, p, seed):
        self.engine, self.ctx, self.p = engine, ctx, p
        self.rng = np.random.default_rng(seed)
        self.vals = draw(self.rng, p, POOL)
        self.vals[:4] = [0, 1, p - 1, p - 2]
        self.dev = up(ctx, self.vals)

    def pick(self, count):
        """(indices, DevArray) of `count` elements of the pool"""
        idx = self.rng.integers(0, POOL, size=count)
        return idx, self.at(idx)

    def at(self, idx):
        idx = np.asarray(idx).reshape(-1)
        t = self.dev.t[torch.from_numpy(idx).to(self.dev.t.device)]
        return self.engine.DevArray(self.ctx, t.contiguous(), len(idx))


def lead(engine, ctx, x):
    """x behind one unused element, in a fresh buffer: a view one element in"""
    buf = ctx.empty(x.n + 1)
    buf.t[1:].copy_(x.t)
    buf.t[:1].copy_(x.t[:1])
    return view(engine, ctx, buf, 1, 1 + x.n)


# ---- unit_prod ---------------------------------------------------------------------------------------------------------------------
PROD_H, PROD_N, PROD_XS = (1, 2, 5, 64), (1, 63, 64, 65, 257, 1031), (1, 3, 16)


@pytest.mark.parametrize('name', list(FIELDS))
def test_unit_prod_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    P = Pool(engine, ctx, p, seed=11 + p % 977)
    H, N, XS = max(PROD_H), max(PROD_N), max(PROD_XS)
    xvals = np.array([0, 1, p - 1] + [int(v) for v in draw(P.rng, p, XPOOL - 3)], dtype=object)
    table = up(ctx, (xvals[:, None] * P.vals[None, :] % p).reshape(-1))                 # every product, in Python integers
    xi = P.rng.integers(0, XPOOL, size=N * XS)
    x = engine.DevArray(ctx, up(ctx, xvals).t[torch.from_numpy(xi).cuda()].contiguous(), N * XS)
    ui, U = P.pick(H * N)
    ui = ui.reshape(H, N)
    keep_x, keep_U = x.t.clone(), U.t.clone()
    ran = 0
    for n in PROD_N:
        for h in PROD_H:
            sub_i = ui[:h, :n]
            Uhn = P.at(sub_i)
            for xs in PROD_XS:
                want = table.t[torch.from_numpy(xi[:n * xs:xs][None, :] * POOL + sub_i).reshape(-1).cuda()]
                got = ctx.unit_prod(x, Uhn, h, xstride=xs)
                assert got.n == h * n and same(got, want), ('aligned', name, n, h, xs)
                out = view(engine, ctx, ctx.empty(h * n + 1), 1, 1 + h * n)
                assert ctx.unit_prod(x, lead(engine, ctx, Uhn), h, xstride=xs, out=out) is out
                assert same(out, want), ('one element off', name, n, h, xs)
                ran += 1
    assert ran == len(PROD_N) * len(PROD_H) * len(PROD_XS)
    # x itself one element off (xstride 1: no pack of x), and at an offset with a stride: bit 2 of (n, 5) bits
    n, h = 256, 5
    Uhn, want = P.at(ui[:h, :n]), lambda off, xs: table.t[torch.from_numpy(xi[off:off + n * xs:xs][None, :] * POOL + ui[:h, :n]).reshape(-1).cuda()]
    assert same(ctx.unit_prod(x, Uhn, h, xoffset=1), want(1, 1)) and same(ctx.unit_prod(x, Uhn, h, xstride=5, xoffset=2), want(2, 5))
    # operands all p - 1: every product is 1
    ones = ctx.empty(h * 257)
    for xs in (1, 3):
        full = lambda count: engine.DevArray(ctx, P.dev.t[2:3].expand((count,) + tuple(P.dev.t.shape[1:])).contiguous(), count)
        got = ctx.unit_prod(full(257 * xs), full(h * 257), h, xstride=xs, out=ones)
        assert got.to_ints() == [1] * (h * 257), (name, xs)
    assert torch.equal(x.t, keep_x) and torch.equal(U.t, keep_U), 'an input was written'


# ---- unit_roll ---------------------------------------------------------------------------------------------------------------------
# (320: whole packs, and whole waves of 24-byte elements, with the wrap at every K2; 1, 65 and 257 are the element path)
ROLL_CASES, ROLL_N = ((1, 2), (3, 5), (3, 8), (8, 129), (8, 256), (10, 1024)), (1, 65, 257, 320)


def offsets(p, kbits, n, high):
    """n canonical values with every residue mod K2 present when n >= K2, else K2 - 1 downwards and 0 last; high: the largest
    value below p with that residue (high limbs all ones for the 2^k - c primes)"""
    K2 = 1 << kbits
    res = [(K2 - 1 - e) % K2 for e in range(n)]
    if 2 <= n < K2:
        res[-1] = 0
    assert set(res) == set(range(K2)) if n >= K2 else (res[0] == K2 - 1 and (n < 2 or 0 in res))
    return [(p - 1) - ((p - 1 - r) % K2) if high else r + K2 * (e % 3) for e, r in enumerate(res)], res


@pytest.mark.parametrize('name', list(FIELDS))
def test_unit_roll_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    P = Pool(engine, ctx, p, seed=23 + p % 971)
    ran = 0
    for kbits, K in ROLL_CASES:
        K2 = 1 << kbits
        for n in ROLL_N:
            ui, U = P.pick(K2 * n)
            ui = ui.reshape(K2, n)
            keep = U.t.clone()
            for high in (False, True):
                cvals, res = offsets(p, kbits, n, high)
                assert all(0 <= v < p and v % K2 == r for v, r in zip(cvals, res)) and (not high or cvals[0] > p - 1 - K2)
                c = up(ctx, cvals)
                off = np.array([v % K2 for v in cvals], dtype=np.int64)                     # Python integers: c mod K2
                src = (np.arange(K, dtype=np.int64)[:, None] - off[None, :]) % K2           # (j - c) mod K2
                want = P.at(ui[src, np.arange(n)[None, :]]).t
                got = ctx.unit_roll(U, c, kbits, K)
                assert got.n == K * n and same(got, want), ('aligned', name, kbits, K, n, high)
                out = view(engine, ctx, ctx.empty(K * n + 1), 1, 1 + K * n)
                assert ctx.unit_roll(lead(engine, ctx, U), lead(engine, ctx, c), kbits, K, out=out) is out
                assert same(out, want), ('one element off', name, kbits, K, n, high)
                ran += 1
            assert torch.equal(U.t, keep), 'an input was written'
    assert ran == len(ROLL_CASES) * len(ROLL_N) * 2
    # kbits = 0: one row, whatever c holds
    U = P.pick(70)[1]
    assert same(ctx.unit_roll(U, up(ctx, [p - 1] * 70), 0, 1), U.t)


# ---- unit_dot ----------------------------------------------------------------------------------------------------------------------
def dot_ref(p, tab, U, rows, n, c, K2):
    """sum_j tab[(j + c[e]) mod K2] U[j n + e] in Python integers, tab zero from len(tab) up; c None: tab[j]"""
    T = np.array(list(tab) + [0] * (max(rows, K2) - len(tab)), dtype=object)
    Um = np.asarray(U, dtype=object).reshape(rows, n)
    if c is None:
        return [int(v) for v in (T[:rows, None] * Um).sum(axis=0) % p]
    idx = (np.arange(rows)[:, None] + np.array([v % K2 for v in c], dtype=np.int64)[None, :]) % K2
    return [int(v) for v in (T[idx] * Um).sum(axis=0) % p]


@pytest.mark.parametrize('name', list(FIELDS))
def test_unit_dot_without_rotation_at_the_flush_edges(mods, name):
    """table and U all p - 1: every term is 1, the sum is the row count -- at FLUSH - 1, FLUSH, FLUSH + 1 and 2 FLUSH + 1 terms"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    F = flush_of(name)
    top = up(ctx, [p - 1])
    full = lambda count: engine.DevArray(ctx, top.t[0:1].expand((count,) + tuple(top.t.shape[1:])).contiguous(), count)
    for rows in (1, F - 1, F, F + 1, 2 * F + 1):
        for n in (64, 65):
            U, tab = full(rows * n), full(rows)
            assert ctx.unit_dot(U, tab, rows).to_ints() == [rows % p] * n, (name, rows, n)
            assert ctx.unit_dot(lead(engine, ctx, U), tab, rows).to_ints() == [rows % p] * n, ('one element off', name, rows, n)
    # a table of its own per row, random U: the plain dot product
    P = Pool(engine, ctx, p, seed=5)
    rows, n = 2 * F + 1, 65
    (ui, U), (ti, tab) = P.pick(rows * n), P.pick(rows)
    assert ctx.unit_dot(U, tab, rows).to_ints() == dot_ref(p, P.vals[ti], P.vals[ui], rows, n, None, 0)


@pytest.mark.parametrize('name', list(FIELDS))
def test_unit_dot_with_rotation(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    P = Pool(engine, ctx, p, seed=41 + p % 967)
    kmax = ctx.unit_dot_max_kbits()
    assert kmax == {4: 14, 8: 13, 12: 12, 16: 12, 24: 11}[ctx.elem_bytes]
    rng = random.Random(3)
    for kbits in (1, 5, 8, kmax):
        K2 = 1 << kbits
        for n in (1, 65, 130):
            if kbits < kmax:
                ui, U = P.pick(K2 * n)
                Uvals = P.vals[ui]
            else:
                # the largest table: U is zero but for six rows per column, rows 0 and K2 - 1 among them, so that the sums
                # in Python integers stay small; the kernel walks every row all the same
                ui = np.zeros((K2, n), dtype=np.int64)
                for e in range(n):
                    for j in [0, K2 - 1] + [rng.randrange(K2) for _ in range(4)]:
                        ui[j, e] = rng.randrange(1, POOL)
                U, Uvals = P.at(ui), None
            keep = U.t.clone()
            cvals, _ = offsets(p, kbits, n, high=(n == 65))
            c = up(ctx, cvals)
            for tlen in (1, K2 // 2 + 1, K2):
                ti, tab = P.pick(tlen)
                tvals = P.vals[ti]
                if Uvals is not None:
                    want = dot_ref(p, tvals, Uvals, K2, n, cvals, K2)
                else:
                    want = []
                    for e in range(n):
                        at = lambda i: int(tvals[i]) if i < tlen else 0
                        want.append(sum(at((j + cvals[e]) % K2) * int(P.vals[ui[j, e]]) for j in np.nonzero(ui[:, e])[0].tolist()) % p)
                got = ctx.unit_dot(U, tab, K2, c=c, kbits=kbits)
                assert got.to_ints() == want, ('aligned', name, kbits, n, tlen)
                out = view(engine, ctx, ctx.empty(n + 1), 1, 1 + n)
                assert ctx.unit_dot(lead(engine, ctx, U), tab, K2, c=lead(engine, ctx, c), kbits=kbits, out=out) is out
                assert out.to_ints() == want, ('one element off', name, kbits, n, tlen)
            assert torch.equal(U.t, keep), 'an input was written'
    # one kbits above the bound: FFGPU_ENOTSUP, and nothing written
    kbits, n = kmax + 1, 2
    K2 = 1 << kbits
    U = ctx.empty(K2 * n)
    U.t.zero_()
    out = ctx.empty(n)
    out.t.fill_(0x5a)
    with pytest.raises(NotImplementedError):
        ctx.unit_dot(U, P.pick(3)[1], K2, c=up(ctx, [1, 2]), kbits=kbits, out=out)
    assert ctx._L.ffgm_unit_dot(ctx._h, U.ptr, K2, None, 0, U.ptr, K2, out.ptr, n, ctx._stream()) == _ffi.ENOTSUP    # ... without c too
    torch.cuda.synchronize()
    assert bool((out.t == 0x5a).all()), 'a refused call wrote'


# ---- guard bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', BY_SIZE)
@pytest.mark.parametrize('n', [320, 301])
def test_nothing_is_written_outside_the_outputs(mods, name, n):
    """n = 320: whole packs (and whole waves of 24-byte elements) in all three kernels; n = 301: the element paths"""
    _ffi, engine, _, _ = mods
    p, pad, kbits, K, h = FIELDS[name], 240, 3, 5, 3            # 240: a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    eb, K2 = ctx.elem_bytes, 1 << kbits
    rng = np.random.default_rng(83)
    x, U, tab = draw(rng, p, n), draw(rng, p, K2 * n), draw(rng, p, K)
    cvals, _ = offsets(p, kbits, n, True)
    dx, dU, dtab, dc = up(ctx, x), up(ctx, U), up(ctx, tab), up(ctx, cvals)
    keep = [v.t.clone() for v in (dx, dU, dtab, dc)]

    def guarded(nbytes):
        buf = torch.full((pad + nbytes + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        return buf, buf.data_ptr() + pad

    def check(buf, nbytes, vals):
        want = up(ctx, vals).t.contiguous().view(torch.uint8).reshape(-1)
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + nbytes:] == 0xa5).all()), 'guard bytes written'
        assert torch.equal(buf[pad:pad + nbytes], want)

    L, hd, st = ctx._L, ctx._h, ctx._stream()
    Um = U.reshape(K2, n)
    b, q = guarded(h * n * eb)
    assert L.ffgm_unit_prod(hd, dx.ptr, 1, dU.ptr, h, q, n, st) == _ffi.OK
    check(b, h * n * eb, (x[None, :] * Um[:h] % p).reshape(-1))
    b, q = guarded(K * n * eb)
    assert L.ffgm_unit_roll(hd, dU.ptr, dc.ptr, kbits, K, q, n, st) == _ffi.OK
    check(b, K * n * eb, np.array([[Um[(j - v) % K2, e] for e, v in enumerate(cvals)] for j in range(K)], dtype=object).reshape(-1))
    b, q = guarded(n * eb)
    assert L.ffgm_unit_dot(hd, dU.ptr, K2, dc.ptr, kbits, dtab.ptr, K, q, n, st) == _ffi.OK
    check(b, n * eb, dot_ref(p, tab, U, K2, n, cvals, K2))
    b, q = guarded(n * eb)
    assert L.ffgm_unit_dot(hd, dU.ptr, K, None, 0, dtab.ptr, K, q, n, st) == _ffi.OK
    check(b, n * eb, dot_ref(p, tab, U[:K * n], K, n, None, 0))
    assert all(torch.equal(v.t, k_) for v, k_ in zip((dx, dU, dtab, dc), keep)), 'an input was written'


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p, n, kbits, K, h = 2**61 - 1, 300, 3, 5, 4
    ctx = engine.FieldContext(p, device=0)
    L, hd, st = ctx._L, ctx._h, ctx._stream()
    eb, K2 = ctx.elem_bytes, 8
    pat = lambda count: torch.full((count,), 0x5a, dtype=torch.uint8, device='cuda')
    X, UU, C, T, O = pat(3 * n * eb), pat(K2 * n * eb), pat(n * eb), pat(K2 * eb), pat(K2 * n * eb)
    x, U, c, tab, o = (b.data_ptr() for b in (X, UU, C, T, O))
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    prod = lambda x_=x, xs_=1, U_=U, h_=h, o_=o, n_=n: L.ffgm_unit_prod(hd, x_, xs_, U_, h_, o_, n_, st)
    roll = lambda U_=U, c_=c, kb_=kbits, K_=K, o_=o, n_=n: L.ffgm_unit_roll(hd, U_, c_, kb_, K_, o_, n_, st)
    dot = lambda U_=U, rows_=K2, c_=c, kb_=kbits, t_=tab, tl_=K, o_=o, n_=n: L.ffgm_unit_dot(hd, U_, rows_, c_, kb_, t_, tl_, o_, n_, st)
    # the counts, also with nothing to do
    assert prod(h_=0) == EINVAL and prod(h_=0, n_=0) == EINVAL and prod(xs_=0) == EINVAL and prod(xs_=0, n_=0) == EINVAL
    for kb, K_ in ((3, 0), (3, 9), (-1, 1), (31, 1)):
        assert roll(kb_=kb, K_=K_) == EINVAL and roll(kb_=kb, K_=K_, n_=0) == EINVAL
    assert dot(rows_=7) == EINVAL and dot(rows_=9) == EINVAL and dot(rows_=7, n_=0) == EINVAL, 'rows != 2^kbits with c'
    assert dot(tl_=K2 + 1) == EINVAL and dot(tl_=0) == EINVAL and dot(tl_=K2 + 1, n_=0) == EINVAL, 'tlen > K2'
    assert dot(c_=None, rows_=5, tl_=4) == EINVAL and dot(c_=None, rows_=0, tl_=0) == EINVAL, 'tlen == rows without c'
    assert dot(kb_=-1) == EINVAL and dot(kb_=31, rows_=1 << 31) == EINVAL
    # a null context or required pointer
    assert L.ffgm_unit_prod(None, x, 1, U, h, o, n, st) == EINVAL and L.ffgm_unit_roll(None, U, c, kbits, K, o, n, st) == EINVAL
    assert L.ffgm_unit_dot(None, U, K2, c, kbits, tab, K, o, n, st) == EINVAL
    assert prod(x_=None) == EINVAL and prod(U_=None) == EINVAL and prod(o_=None) == EINVAL
    assert roll(U_=None) == EINVAL and roll(c_=None) == EINVAL and roll(o_=None) == EINVAL
    assert dot(U_=None) == EINVAL and dot(t_=None) == EINVAL and dot(o_=None) == EINVAL
    # sizes overflowing: rows n, rows n eb, the span of x
    assert prod(n_=1 << 62) == EINVAL and prod(n_=1 << 60) == EINVAL and prod(h_=3, n_=(1 << 64) // 3 + 1) == EINVAL
    assert prod(xs_=1 << 40, n_=1 << 30) == EINVAL and prod(h_=1, xs_=1 << 63, n_=3) == EINVAL
    assert roll(n_=1 << 62) == EINVAL and roll(n_=1 << 60) == EINVAL and roll(kb_=30, K_=1, n_=1 << 34) == EINVAL
    assert dot(n_=1 << 62) == EINVAL and dot(n_=1 << 60) == EINVAL
    # overlaps: an output on an input
    last = lambda base, count: base + eb * (count - 1)
    assert prod(o_=U) == EINVAL and prod(o_=x) == EINVAL and prod(o_=last(U, h * n)) == EINVAL and prod(U_=last(o, h * n)) == EINVAL
    assert prod(xs_=3, o_=last(x, 3 * n - 2)) == EINVAL
    assert roll(o_=U) == EINVAL and roll(o_=c) == EINVAL and roll(o_=last(U, K2 * n)) == EINVAL and roll(c_=last(o, K * n)) == EINVAL
    assert dot(o_=U) == EINVAL and dot(o_=c) == EINVAL and dot(o_=tab) == EINVAL and dot(o_=last(tab, K)) == EINVAL
    assert dot(t_=last(o, n)) == EINVAL and dot(c_=None, rows_=K, o_=last(U, K * n)) == EINVAL
    torch.cuda.synchronize()
    for buf in (X, UU, C, T, O):
        assert bool((buf == 0x5a).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    assert prod(n_=0, x_=None, U_=None, o_=None) == OK and roll(n_=0, U_=None, c_=None, o_=None) == OK
    assert dot(n_=0, U_=None, c_=None, rows_=4, tl_=4, t_=None, o_=None) == OK
    torch.cuda.synchronize()
    for buf in (X, UU, C, T, O):
        assert bool((buf == 0x5a).all())
    # valid calls, for contrast (inputs may alias each other; the operands are canonical)
    for buf in (X, UU, C, T):
        buf.zero_()
    assert prod() == OK and prod(xs_=3) == OK and prod(x_=U) == OK and roll() == OK and roll(c_=U) == OK and roll(kb_=0, K_=1) == OK
    assert dot() == OK and dot(c_=None, rows_=K) == OK and dot(c_=U, t_=U, tl_=K2) == OK and dot(o_=last(o, n + 1)) == OK
    torch.cuda.synchronize()
    assert bool((O[:K * n * eb] == 0).all())
    # binary fields
    for mod in (0x11b, (1 << 64) | 0x1b):
        bctx = engine.FieldContext(mod, True, device=0)
        G = torch.zeros(16384, dtype=torch.uint8, device='cuda')
        g = G.data_ptr()
        bl, bh = bctx._L, bctx._h
        assert bl.ffgm_unit_prod(bh, g, 1, g + 1024, 2, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgm_unit_roll(bh, g, g + 1024, 1, 2, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgm_unit_dot(bh, g, 2, g + 1024, 1, g + 2048, 2, g + 4096, 4, st) == ENOTSUP
        e2, e4 = bctx.empty(2), bctx.empty(4)
        for bad in (lambda: bctx.unit_prod(e2, e4, 2), lambda: bctx.unit_roll(e4, e2, 1, 2), lambda: bctx.unit_dot(e4, e2, 2, c=e2, kbits=1)):
            with pytest.raises(NotImplementedError):
                bad()
    # the engine's own checks
    e2, e3, e6, e8 = ctx.empty(2), ctx.empty(3), ctx.empty(6), ctx.empty(8)
    for bad in (lambda: ctx.unit_prod(e6, e8, 3), lambda: ctx.unit_prod(e6, e8, 4, xstride=0), lambda: ctx.unit_prod(e6, e8, 4, xstride=6),
                lambda: ctx.unit_prod(e6, e8, 4, xoffset=5), lambda: ctx.unit_prod(e6, e8, 4, out=e2), lambda: ctx.unit_roll(e8, e2, 2, 5),
                lambda: ctx.unit_roll(e8, e2, 3, 8), lambda: ctx.unit_roll(e8, e6, 2, 4), lambda: ctx.unit_roll(e8, e2, 2, 3, out=e8),
                lambda: ctx.unit_dot(e8, e3, 4), lambda: ctx.unit_dot(e8, e3, 8, c=e2, kbits=3), lambda: ctx.unit_dot(e8, e3, 4, c=e6, kbits=2),
                lambda: ctx.unit_dot(e8, e8, 4, c=e2, kbits=2), lambda: ctx.unit_dot(e8, e3, 4, c=e2, kbits=2, out=e8)):
        with pytest.raises(ValueError):
            bad()


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_prod_roll_dot(mods):
    """the three calls captured once on one stream, replayed on changed inputs, equal to Python integers and to the eager result"""
    _ffi, engine, _, _ = mods
    p, n, kbits, K = 2**80 - 65, 1031, 4, 13
    K2 = 1 << kbits
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(29)
    x, U, c, tab = ctx.empty(n), ctx.empty(K2 * n), ctx.empty(n), ctx.empty(K)

    def steps():
        v = ctx.unit_prod(x, U, K2)
        return [v, ctx.unit_roll(v, c, kbits, K), ctx.unit_dot(v, tab, K2, c=c, kbits=kbits)]

    def load():
        vals = [draw(rng, p, n), draw(rng, p, K2 * n), draw(rng, p, n), draw(rng, p, K)]
        for dst, v in zip((x, U, c, tab), vals):
            dst.t.copy_(up(ctx, v).t)
        return vals

    load()
    cg = engine.CapturedLaunches(steps)
    for _ in range(2):
        vx, vU, vc, vt = load()
        prod = (vx[None, :] * vU.reshape(K2, n) % p)
        rolled = np.array([[prod[(j - int(v)) % K2, e] for e, v in enumerate(vc)] for j in range(K)], dtype=object)
        for out in cg.result:
            out.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        eager = steps()
        torch.cuda.synchronize()
        assert same(cg.result[0], up(ctx, prod.reshape(-1)).t) and same(cg.result[1], up(ctx, rolled.reshape(-1)).t)
        assert cg.result[2].to_ints() == dot_ref(p, vt, prod.reshape(-1), K2, n, [int(v) for v in vc], K2)
        assert all(same(a, b.t) for a, b in zip(cg.result, eager))


# ---- the compositions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [2, 3, 5, 13, 256])
def test_end_to_end_on_every_index(mods, K):
    """(m, t) = (3, 1), batches of n = 67 indices that together hold every index value (one batch but for K = 256), on the
    shipped supplier's draws: unit_vectors and unit_vectors_from_bits (behind to_bits) open to one-hot rows, lookup to
    table[a] for a public and for a shared table; the inputs are not written"""
    _ffi, engine, finfields, protocols = mods
    p, m, t, n = 2**61 - 1, 3, 1, 67
    ctx, F = engine.FieldContext(p, device=0), gf(p)
    R = protocols.Randomness(ctx, F, t, m, b'unit vectors on the device')
    rng = random.Random(K)
    table = [rng.randrange(p) for _ in range(K)]
    pub, sh = ctx.from_ints(table), _share(ctx, rng, table, t, m)
    l = max(1, (K - 1).bit_length())
    seen = set()
    for lo in range(0, K, n):
        a = [(lo + e) % K for e in range(n)]
        rng.shuffle(a)
        seen |= set(a)
        xs = _share(ctx, rng, a, t, m)
        before = [x.t.clone() for x in xs]
        onehot = [[int(j == v) for j in range(K)] for v in a]
        assert columns(open_two_ways(ctx, protocols.unit_vectors(ctx, F, xs, K, t, R.rand_unit), t), K, n) == onehot
        assert open_two_ways(ctx, protocols.lookup(ctx, F, xs, pub, K, t, R.rand_unit), t) == [table[v] for v in a]
        assert open_two_ways(ctx, protocols.lookup(ctx, F, xs, sh, K, t, R.rand_unit), t) == [table[v] for v in a]
        rbits, rdivl = R.rand_bits(n, l)
        bits = protocols.to_bits(ctx, F, xs, rbits, rdivl, t, l)
        assert columns(open_two_ways(ctx, protocols.unit_vectors_from_bits(ctx, F, bits, l, K, t), t), K, n) == onehot
        assert all(torch.equal(x.t, b) for x, b in zip(xs, before)), 'an input was written'
    assert seen == set(range(K))
    assert open_two_ways(ctx, sh, t) == table and pub.to_ints() == table


def test_the_compositions_open_to_the_fixture(mods):
    """what the reference's np_unit_vector, unit_vector and T @ np_unit_vector opened, on the fixture's inputs and modulus"""
    _ffi, engine, _, _ = mods
    assert tuple(e['K'] for e in golden()['unit']) == KS
    check_fixture(lambda p: engine.FieldContext(p, device=0), 3, 1)
