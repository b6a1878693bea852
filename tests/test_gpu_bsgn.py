"""The local steps of the secure binary sign by Legendre symbols on the device (ffgm_bsgn_mask / ffgm_bsgn_finish,
mpyc_amd/csrc/bsgn.hpp) against Python integers computed here from the maps include/ffgpu_math.h states, over every prime
policy; guard bytes around every output, inputs unchanged, views one element into their buffers, status codes with nothing
written on refusal, protocols.bsgn for all parties on one GPU -- its results against what the reference demo opened
(tests/golden/bsgn/bsgn.json), its local steps share for share against the Python-integer stand-in over the demo's three
primes -- and mask -> open -> finish replayed from a captured HIP graph."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_sgn import FIELDS as SGN_FIELDS, draw, same, view
from test_gpu_fxp import up
from test_bsgn_host import DEMO_PRIMES, Draws, golden
from test_rbits_host import gf, open_two_ways
from test_sort_host import _share, _signed

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

BLUM40 = 2**40 - 213
FIELDS = dict(SGN_FIELDS, **{'pm64-gen-blum': BLUM40})
ALL_N = (1, 63, 64, 65, 255, 256, 257, 5003)
ALL_W = (1, 2, 3, 5, 8)
ALL_M = (1, 3, 7)
NMAX, WMAX, MMAX = 5003, 8, 7


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def symbols(p, c):
    """(c | p) as 1, -1, 0, entry by entry"""
    half = (p - 1) // 2
    return np.array([0 if v == 0 else 1 if pow(int(v), half, p) == 1 else -1 for v in c.reshape(-1)], dtype=object).reshape(c.shape)


def nonresidue(p):
    return next(v for v in range(2, 100) if pow(v, (p - 1) // 2, p) == p - 1)


class Data:
    """(WMAX, NMAX) operands of both kernels with their expected outputs on the device, computed once; a (w, n) case is rows < w
    and columns < n of the matrices (a sum over the rows < w: row w - 1 of the running sums)"""

    def __init__(self, ctx, p, seed):
        rng = np.random.default_rng(seed)
        W, N, M = WMAX, NMAX, MMAX
        self.p = p
        self.alpha = int(draw(rng, p, 1)[0]) % (p - 2) + 2
        self.betas = [p - 1, 0, 1] + [int(v) for v in draw(rng, p, W - 3)]
        a = draw(rng, p, N)
        a[:3] = [0, 1, p - 1]
        a[3] = (p - self.betas[0]) * pow(self.alpha, -1, p) % p           # alpha a + beta[0] = 0
        a[N - 1] = (p - self.betas[W - 1]) * pow(self.alpha, -1, p) % p   # ... and in the last row at the last element
        z = draw(rng, p, W * N).reshape(W, N)
        z[0, :3], z[1, :3], z[W - 1, N - 3:] = [0, 1, p - 1], [p - 1, p - 1, 0], [p - 1, 1, p - 1]
        z[2] = p - 1
        beta = np.array(self.betas, dtype=object)[:, None]
        self.mask = z * ((self.alpha * a)[None, :] % p + beta) % p
        assert self.mask[0, 3] == 0 and self.mask[W - 1, N - 1] == 0 and z[0, 3] != 0
        # the opened values: 0, 1, p - 1, residues and non-residues in the first columns of every row and in every last column
        c = draw(rng, p, W * N).reshape(W, N)
        nr = nonresidue(p)
        plant = [0, 1, p - 1, 4, nr, nr * 4 % p, pow(nr, 2, p), p - 4]
        for i in range(W):
            c[i, :len(plant)] = plant[i:] + plant[:i]
            for j, n in enumerate(ALL_N):
                c[i, n - 1] = plant[(i + j) % len(plant)]
        h = symbols(p, c)
        assert h[0, :5].tolist() == [0, 1, 1 if p % 4 == 1 else -1, 1, -1] and (h == 0).sum() >= W
        s = [draw(rng, p, W * N).reshape(W, N) for _ in range(M)]
        for q in range(M):
            s[q][:, :3] = [0, 1, p - 1]
        s[0][:] = 1 + rng.integers(0, 2, size=(W, N)).astype(object) * (p - 2)      # party 0: signs themselves, 1 or p - 1
        self.rows = [h * sq % p for sq in s]
        self.sums = [np.cumsum(r, axis=0) % p for r in self.rows]
        self.host = {'a': a, 'z': z, 'c': c, **{f's{q}': s[q] for q in range(M)}}
        self.d = {k_: up(ctx, v) for k_, v in self.host.items()}
        self.d['mask'] = up(ctx, self.mask)
        for q in range(M):
            self.d[f'rows{q}'], self.d[f'sums{q}'] = up(ctx, self.rows[q]), up(ctx, self.sums[q])

    def sub(self, ctx, engine, key, w, n, row0=0):
        """rows row0 .. w-1, columns < n of a (WMAX, NMAX) matrix on the device, as a fresh contiguous array"""
        t = self.d[key].t
        t = t.reshape((WMAX, NMAX) + tuple(t.shape[1:]))[row0:w, :n].contiguous()
        cnt = (w - row0) * n
        return engine.DevArray(ctx, t.reshape((cnt,) + tuple(t.shape[2:])), cnt)


def lead(engine, ctx, x):
    """x behind one unused element, in a fresh buffer: a view one element in"""
    buf = ctx.empty(x.n + 1)
    buf.t[1:].copy_(x.t)
    buf.t[:1].copy_(x.t[:1])
    return view(engine, ctx, buf, 1, 1 + x.n)


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    D = Data(ctx, p, seed=57 + p % 991)
    keep = {k_: v.t.clone() for k_, v in D.d.items()}
    ran = 0
    for n in ALL_N:
        a = view(engine, ctx, D.d['a'], 0, n)
        for w in ALL_W:
            got = ctx.bsgn_mask(a, D.sub(ctx, engine, 'z', w, n), D.alpha, D.betas[:w])
            assert got.n == w * n and same(got, D.sub(ctx, engine, 'mask', w, n).t), ('mask', name, n, w)
            c = D.sub(ctx, engine, 'c', w, n)
            for m in ALL_M:
                ss = [D.sub(ctx, engine, f's{q}', w, n) for q in range(m)]
                rows = ctx.bsgn_finish(c, ss, w)
                assert len(rows) == m and all(same(rows[q], D.sub(ctx, engine, f'rows{q}', w, n).t) for q in range(m)), ('rows', name, n, w, m)
                sums = ctx.bsgn_finish(c, ss, w, sum=True)
                assert len(sums) == m and all(x.n == n for x in sums)
                assert all(same(sums[q], D.sub(ctx, engine, f'sums{q}', w, n, row0=w - 1).t) for q in range(m)), ('sum', name, n, w, m)
                ran += 1
    assert ran == len(ALL_N) * len(ALL_W) * len(ALL_M)
    # one element into their buffers: the element paths
    n, w, m = 2048, 3, 3
    out = view(engine, ctx, ctx.empty(w * n + 1), 1, 1 + w * n)
    assert ctx.bsgn_mask(lead(engine, ctx, view(engine, ctx, D.d['a'], 0, n)), lead(engine, ctx, D.sub(ctx, engine, 'z', w, n)), D.alpha,
                         D.betas[:w], out=out) is out
    assert same(out, D.sub(ctx, engine, 'mask', w, n).t), ('mask, offset views', name)
    c = lead(engine, ctx, D.sub(ctx, engine, 'c', w, n))
    ss = [lead(engine, ctx, D.sub(ctx, engine, f's{q}', w, n)) for q in range(m)]
    for sum_ in (False, True):
        on = n if sum_ else w * n
        outs = [view(engine, ctx, ctx.empty(on + 1), 1, 1 + on) for _ in range(m)]
        res = ctx.bsgn_finish(c, ss, w, sum=sum_, outs=outs)
        assert all(r is o for r, o in zip(res, outs))
        want = [D.sub(ctx, engine, f'sums{q}', w, n, row0=w - 1) if sum_ else D.sub(ctx, engine, f'rows{q}', w, n) for q in range(m)]
        assert all(same(o, x.t) for o, x in zip(outs, want)), ('finish, offset views', name, sum_)
    # aligned operands, one party's row off its alignment: packs are refused for all
    ss[1:] = [D.sub(ctx, engine, f's{q}', w, n) for q in range(1, m)]
    c = D.sub(ctx, engine, 'c', w, n)
    assert all(same(o, D.sub(ctx, engine, f'rows{q}', w, n).t) for q, o in enumerate(ctx.bsgn_finish(c, ss, w)))
    assert all(torch.equal(D.d[k_].t, keep[k_]) for k_ in keep), 'an input was written'


# ---- guard bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
@pytest.mark.parametrize('n,w', [(320, 3), (301, 2)])
def test_nothing_is_written_outside_the_outputs(mods, name, n, w):
    """n = 320: whole packs (and whole waves of 24-byte elements) in all three kernels; n = 301: the element paths and the tail"""
    _ffi, engine, _, _ = mods
    p, pad, m = FIELDS[name], 240, 3                            # 240: a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    eb, cnt = ctx.elem_bytes, w * n
    rng = np.random.default_rng(83)
    a, z, c = draw(rng, p, n), draw(rng, p, cnt), draw(rng, p, cnt)
    s = [draw(rng, p, cnt) for _ in range(m)]
    c[:3], c[-1] = [0, 1, p - 1], 0
    alpha, betas = 2, [1 + 2 * j for j in range(w)]
    inputs = [up(ctx, v) for v in [a, z, c] + s]
    da, dz, dc = inputs[:3]
    ds = inputs[3:]
    keep = [v.t.clone() for v in inputs]
    h = symbols(p, c)

    def guarded(nbytes):
        buf = torch.full((pad + nbytes + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        return buf, buf.data_ptr() + pad

    def check(buf, nbytes, want_bytes):
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + nbytes:] == 0xa5).all()), 'guard bytes written'
        assert torch.equal(buf[pad:pad + nbytes], want_bytes)

    as_bytes = lambda vals: up(ctx, vals).t.contiguous().view(torch.uint8).reshape(-1)
    L, hd, st = ctx._L, ctx._h, ctx._stream()
    b1, p1 = guarded(cnt * eb)
    assert L.ffgm_bsgn_mask(hd, da.ptr, dz.ptr, ctx._scalars([alpha]), ctx._scalars(betas), w, p1, n, st) == _ffi.OK
    check(b1, cnt * eb, as_bytes(z * (np.tile(alpha * a, w) + np.repeat(np.array(betas, dtype=object), n)) % p))
    sp = (ctypes.c_void_p * m)(*[x.ptr for x in ds])
    for sum_ in (0, 1):
        on = n if sum_ else cnt
        bufs = [guarded(on * eb) for _ in range(m)]
        op = (ctypes.c_void_p * m)(*[b[1] for b in bufs])
        assert L.ffgm_bsgn_finish(hd, dc.ptr, sp, op, m, w, sum_, n, st) == _ffi.OK
        for q in range(m):
            full = h * s[q] % p
            check(bufs[q][0], on * eb, as_bytes(full.reshape(w, n).sum(axis=0) % p if sum_ else full))
    assert all(torch.equal(v.t, k_) for v, k_ in zip(inputs, keep)), 'an input was written'


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p, n, w, m = 2**61 - 1, 300, 4, 3
    ctx = engine.FieldContext(p, device=0)
    L, h, st = ctx._L, ctx._h, ctx._stream()
    eb, cnt = ctx.elem_bytes, w * n
    pat = lambda count: torch.full((count,), 0x5a, dtype=torch.uint8, device='cuda')
    A, Z, O, C = pat(n * eb), pat(cnt * eb), pat(cnt * eb), pat(cnt * eb)
    S, OUT = [pat(cnt * eb) for _ in range(m)], [pat(cnt * eb) for _ in range(m)]
    a, z, o, c = (b.data_ptr() for b in (A, Z, O, C))
    sp, op = [b.data_ptr() for b in S], [b.data_ptr() for b in OUT]
    al, be = ctx._scalars([2]), ctx._scalars([1, 3, 5, 7])
    arr = lambda ptrs: (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    mask = lambda a_=a, z_=z, al_=al, be_=be, w_=w, o_=o, n_=n: L.ffgm_bsgn_mask(h, a_, z_, al_, be_, w_, o_, n_, st)
    fin = lambda c_=c, s_=sp, o_=op, m_=m, w_=w, sum_=0, n_=n: L.ffgm_bsgn_finish(h, c_, None if s_ is None else arr(s_),
                                                                                None if o_ is None else arr(o_), m_, w_, sum_, n_, st)
    # the counts, also with nothing to do
    for bad in (0, -1, 9):
        assert mask(w_=bad) == EINVAL and mask(w_=bad, n_=0) == EINVAL and fin(w_=bad) == EINVAL and fin(w_=bad, n_=0) == EINVAL
    assert fin(m_=0) == EINVAL and fin(m_=-1) == EINVAL and fin(m_=0, n_=0) == EINVAL and fin(sum_=2) == EINVAL and fin(sum_=-1) == EINVAL
    assert fin(m_=65, s_=sp * 22, o_=op * 22) == ENOTSUP and fin(m_=65, n_=0) == ENOTSUP
    # a null context or required pointer
    assert L.ffgm_bsgn_mask(None, a, z, al, be, w, o, n, st) == EINVAL and L.ffgm_bsgn_finish(None, c, arr(sp), arr(op), m, w, 0, n, st) == EINVAL
    assert mask(a_=None) == EINVAL and mask(z_=None) == EINVAL and mask(al_=None) == EINVAL and mask(be_=None) == EINVAL and mask(o_=None) == EINVAL
    assert fin(c_=None) == EINVAL and fin(s_=None) == EINVAL and fin(o_=None) == EINVAL
    assert fin(s_=[sp[0], None, sp[2]]) == EINVAL and fin(o_=[op[0], op[1], None]) == EINVAL
    # sizes overflowing: w n, w n eb
    assert mask(n_=1 << 62) == EINVAL and mask(n_=1 << 60) == EINVAL and mask(w_=3, n_=(1 << 64) // 3 + 1) == EINVAL
    assert fin(n_=1 << 62) == EINVAL and fin(n_=1 << 60) == EINVAL and fin(w_=3, n_=(1 << 64) // 3 + 1) == EINVAL and fin(sum_=1, n_=1 << 60) == EINVAL
    # overlaps: an output on an input or on another output
    assert mask(o_=a) == EINVAL and mask(o_=z) == EINVAL and mask(o_=z + eb * (cnt - 1)) == EINVAL and mask(a_=o + eb * (cnt - 1)) == EINVAL
    assert fin(o_=[c, op[1], op[2]]) == EINVAL and fin(o_=[op[0], op[1], c + eb * (cnt - 1)]) == EINVAL
    assert fin(o_=[sp[0], op[1], op[2]]) == EINVAL and fin(o_=[op[0], sp[2], op[2]]) == EINVAL and fin(o_=[op[0], op[0], op[2]]) == EINVAL
    assert fin(o_=[op[0], op[1], op[1] + eb * (cnt - 1)]) == EINVAL and fin(sum_=1, o_=[op[0], op[1], op[1] + eb * (n - 1)]) == EINVAL
    assert fin(sum_=1, o_=[op[0], op[1], sp[0] + eb * (cnt - 1)]) == EINVAL
    torch.cuda.synchronize()
    for buf in [A, Z, O, C] + S + OUT:
        assert bool((buf == 0x5a).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    assert mask(n_=0, a_=None, z_=None, al_=None, be_=None, o_=None) == OK and fin(n_=0, c_=None, s_=None, o_=None) == OK
    assert fin(n_=0, sum_=1, m_=64, c_=None, s_=None, o_=None) == OK
    torch.cuda.synchronize()
    for buf in [A, Z, O, C] + S + OUT:
        assert bool((buf == 0x5a).all())
    # valid calls, for contrast (inputs may alias each other; the operands are canonical)
    for buf in [A, Z, C] + S:
        buf.zero_()
    S[0].view(torch.int64).fill_(1)
    assert mask() == OK and mask(w_=1) == OK and mask(a_=z) == OK and fin() == OK and fin(s_=[sp[0]] * 3) == OK
    assert fin(sum_=1, o_=[op[0], op[0] + eb * n, op[0] + 2 * eb * n]) == OK
    torch.cuda.synchronize()
    assert bool((O == 0).all()) and bool((OUT[1] == 0).all()), 'zeros everywhere: (0 | p) = 0'
    C.view(torch.int64).fill_(4)
    assert fin() == OK and fin(sum_=1, o_=[op[1], op[2], op[2] + eb * n]) == OK
    torch.cuda.synchronize()
    assert bool((OUT[0].view(torch.int64) == 1).all()) and bool((OUT[1].view(torch.int64)[:n] == w).all()), 'a residue: s itself, w of them'
    # binary fields, and the field of two elements
    for mod in (0x11b, (1 << 64) | 0x1b):
        bctx = engine.FieldContext(mod, True, device=0)
        G = torch.zeros(16384, dtype=torch.uint8, device='cuda')
        g = G.data_ptr()
        bl, bh = bctx._L, bctx._h
        assert bl.ffgm_bsgn_mask(bh, g, g + 1024, al, be, 2, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgm_bsgn_finish(bh, g, arr([g + 1024]), arr([g + 4096]), 1, 2, 0, 4, st) == ENOTSUP
        for bad in (lambda: bctx.bsgn_mask(bctx.empty(2), bctx.empty(4), 2, [1, 3]), lambda: bctx.bsgn_finish(bctx.empty(4), [bctx.empty(4)], 2)):
            with pytest.raises(NotImplementedError):
                bad()
    two = engine.FieldContext(2, device=0)
    G = torch.zeros(16384, dtype=torch.uint8, device='cuda')
    g = G.data_ptr()
    assert two._L.ffgm_bsgn_finish(two._h, g, arr([g + 1024]), arr([g + 4096]), 1, 2, 0, 4, st) == ENOTSUP
    torch.cuda.synchronize()
    assert bool((G == 0).all())
    with pytest.raises(NotImplementedError):
        two.bsgn_finish(two.empty(4), [two.empty(4)], 2)
    # the engine's own checks
    e2, e8 = ctx.empty(2), ctx.empty(8)
    for bad in (lambda: ctx.bsgn_mask(e2, e8, 2, []), lambda: ctx.bsgn_mask(e2, e8, 2, [1] * 9), lambda: ctx.bsgn_mask(e2, e8, 2, [1, 3, 5]),
                lambda: ctx.bsgn_mask(e2, e8, 2, [1, 3, 5, 7], out=e2), lambda: ctx.bsgn_finish(e8, [], 4), lambda: ctx.bsgn_finish(e8, [e8], 3),
                lambda: ctx.bsgn_finish(e8, [e2], 4), lambda: ctx.bsgn_finish(e8, [e8], 0), lambda: ctx.bsgn_finish(e8, [e8], 4, outs=[e8, e8]),
                lambda: ctx.bsgn_finish(e8, [e8], 4, sum=True, outs=[e8]), lambda: ctx.bsgn_finish(e8, [e8], 4, outs=[e2])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        ctx.bsgn_finish(e8, [e8] * 65, 4)


# ---- the protocol ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [0, 1, 2])
def test_bsgn_opens_to_the_fixture(mods, d):
    """(m, t) = (3, 1) on the device over the prime the demo pairs with d, on every input of the fixture: what the reference's
    own bsgn_d opened, the wrong signs beyond the range included; the inputs are not written"""
    _ffi, engine, finfields, protocols = mods
    e = golden()[d]
    p, m, t = e['p'], 3, 1
    assert p == DEMO_PRIMES[d]
    ctx = engine.FieldContext(p, device=0)
    rng = random.Random(70 + d)
    xs = _share(ctx, rng, e['a'], t, m)
    before = [x.t.clone() for x in xs]
    draws = Draws(ctx, m, t, seed=80 + d)
    got = protocols.bsgn(ctx, gf(p), xs, t, d, draws)
    assert [_signed(v, p) for v in open_two_ways(ctx, got, t)] == e['bsgn']
    assert all(torch.equal(x.t, b) for x, b in zip(xs, before)) and draws.unwritten(), 'an input of bsgn was written'
    # ... and on nothing but the shipped supplier's draws
    R = protocols.Randomness(ctx, gf(p), t, m, b'bsgn on the device')
    got = protocols.bsgn(ctx, gf(p), xs, t, d, R.rand_bsgn)
    assert [_signed(v, p) for v in open_two_ways(ctx, got, t)] == e['bsgn']


@pytest.mark.parametrize('p', DEMO_PRIMES)
def test_local_steps_share_for_share(mods, p):
    """the same shares into the device and into the Python-integer stand-in, for every variant's row count and both modes"""
    _ffi, engine, finfields, protocols = mods
    from bsgn_cpuctx import BsgnCpuFieldContext
    m, t, n = 3, 1, 1027
    dev, cpu = engine.FieldContext(p, device=0), BsgnCpuFieldContext(p)
    rng = random.Random(p % 1009)
    a = [rng.randrange(-700, 700) for _ in range(n - 2)] + [(p - 1) // 2, (p - 3) // 2]         # zeros of 2a + 1 and of 2a + 3
    xs_cpu = _share(cpu, rng, a, t, m)
    s_cpu, r_cpu = Draws(cpu, m, t, seed=5, plant={0: 0, 6 * n - 1: 0})(6 * n)
    to_dev = lambda v: [dev.from_ints(x.to_ints()) for x in v]
    xs, s, r = to_dev(xs_cpu), to_dev(s_cpu), to_dev(r_cpu)
    F = gf(p)
    z = protocols.multiply(dev, F, s, protocols.multiply(dev, F, r, r, t), t)
    z_cpu = [cpu.from_ints(x.to_ints()) for x in z]
    rows = lambda ctx, v, lo, hi: [protocols._rows(ctx, x, lo, hi, n) for x in v]
    for d in (0, 1, 2):
        w = protocols.bsgn_rows(d)
        betas = [1 + 2 * j for j in range(-(w // 2), w // 2 + 1)]
        masked = [[ctx.bsgn_mask(x_[i], rows(ctx, z_, 0, w)[i], 2, betas) for i in range(m)]
                  for ctx, x_, z_ in ((dev, xs, z), (cpu, xs_cpu, z_cpu))]
        assert [v.to_ints() for v in masked[0]] == [v.to_ints() for v in masked[1]], ('mask: a share differs', d)
        cs = [protocols.open_(ctx, F, mk, t, degree=2 * t) for ctx, mk in zip((dev, cpu), masked)]
        assert cs[0].to_ints() == cs[1].to_ints() and 0 in cs[0].to_ints()
        for sum_ in (False, True):
            fins = [ctx.bsgn_finish(c, rows(ctx, s_, 0, w), w, sum=sum_) for ctx, c, s_ in ((dev, cs[0], s), (cpu, cs[1], s_cpu))]
            assert [v.to_ints() for v in fins[0]] == [v.to_ints() for v in fins[1]], ('finish: a share differs', d, sum_)
    # the second stage of d = 2: alpha = 1, beta = 0 on the sixth row
    T = dev.bsgn_finish(cs[0], rows(dev, s, 0, 5), 5, sum=True)
    T_cpu = [cpu.from_ints(x.to_ints()) for x in T]
    m2 = [[ctx.bsgn_mask(T_[i], rows(ctx, z_, 5, 6)[i], 1, [0]) for i in range(m)] for ctx, T_, z_ in ((dev, T, z), (cpu, T_cpu, z_cpu))]
    assert [v.to_ints() for v in m2[0]] == [v.to_ints() for v in m2[1]]


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_mask_open_finish(mods):
    """three senders' masks, the opening of their degree-2 values, the finish of three parties in both modes on the opened
    values, captured once on one stream, replayed on changed inputs, equal to Python integers and to the eager result"""
    _ffi, engine, _, protocols = mods
    p, n, w, m, t = 2**80 - 65, 5003, 5, 3, 1
    ctx = engine.FieldContext(p, device=0)
    F = gf(p)
    rng = np.random.default_rng(29)
    xs, zs = [ctx.empty(n) for _ in range(m)], [ctx.empty(w * n) for _ in range(m)]
    ss = [ctx.empty(w * n) for _ in range(m)]
    betas = [p - 3, p - 1, 1, 3, 5]
    lam = [3, p - 3, 1]                                                        # the Lagrange vector of x = 1, 2, 3 at 0

    def steps():
        c = protocols.open_(ctx, F, [ctx.bsgn_mask(xs[i], zs[i], 2, betas) for i in range(m)], t, degree=2 * t)
        return [c] + ctx.bsgn_finish(c, ss, w) + ctx.bsgn_finish(c, ss, w, sum=True)

    def load():
        vals = [draw(rng, p, n) for _ in range(m)] + [draw(rng, p, w * n) for _ in range(2 * m)]
        for i in range(m):
            vals[m + i][:2] = 0                                                 # zeros among the opened values
        for dst, v in zip(xs + zs + ss, vals):
            dst.t.copy_(up(ctx, v).t)
        return vals

    load()
    cg = engine.CapturedLaunches(steps)
    for _ in range(2):
        vals = load()
        vx, vz, vs = vals[:m], vals[m:2 * m], vals[2 * m:]
        beta = np.repeat(np.array(betas, dtype=object), n)
        c = sum(lam[i] * (vz[i] * (np.tile(2 * vx[i], w) + beta) % p) for i in range(m)) % p
        h = symbols(p, c)
        for out in cg.result:
            out.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        eager = steps()
        torch.cuda.synchronize()
        assert h[0] == 0 and set(h.tolist()) == {0, 1, -1} and same(cg.result[0], up(ctx, c).t)
        for q in range(m):
            full = h * vs[q] % p
            assert same(cg.result[1 + q], up(ctx, full).t) and same(cg.result[1 + m + q], up(ctx, full.reshape(w, n).sum(axis=0) % p).t)
        assert all(same(x, y.t) for x, y in zip(cg.result, eager))
