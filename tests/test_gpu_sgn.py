"""The local steps of the secure comparison on the device (ffgpu_sgn_mask / _expand / _finish, mpyc_amd/csrc/sgn.hpp)
against Python integers computed here from the maps include/ffgpu.h states, over every prime policy; NULL output
combinations, guard bytes around every output, status codes, protocols.compare_zero end to end for all parties on one
GPU, the same values from the calls the engine had before (matmul with the power vector, element-wise calls, scan),
and the three calls replayed from a captured HIP graph."""
import os
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one field per prime policy of the launcher table (and the third PM64 variant)
FIELDS = {
    'rc32': 2**31 - 1, 'pm64-mersenne': 2**61 - 1, 'pm64-k64': 2**64 - 189, 'pm64-gen': 2**40 - 87,
    'rc64': 6616326157076047771, 'pm96': 2**80 - 65, 'pm128': 2**128 - 173, 'pm192': 2**136 - 113,
    'mont128': 258797994007609146293811961253269568351, 'mont192': 2**135 + 4823,
}
# (10 and 20: whole chunks of the 12- and 24-byte geometries, 10 and 5 columns)
ALL_L = (1, 2, 7, 10, 16, 20, 31, 32, 33, 64)
NMAX = 5003


def tile_size():
    src = open(os.path.join(ROOT, 'mpyc_amd', 'csrc', 'sgn_geom.hpp')).read()
    return int(re.search(r'SGN_TILE\s*=\s*(\d+)', src).group(1))


def sizes():
    t = tile_size()
    return sorted({1, 63, 257, NMAX, t - 1, t, t + 1})


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def obj(vals):
    a = np.empty(len(vals), dtype=object)
    a[:] = vals
    return a


def draw(rng, p, count):
    """uniform field elements (200 random bits mod p) as an object array, built inside NumPy's loops"""
    w = rng.integers(0, 2**64, size=(3, count), dtype=np.uint64).astype(object)
    return ((w[0] << 136) ^ (w[1] << 64) ^ w[2]) % p


def mask_ref(p, l, a, R, rd):
    acc = obj([0] * len(a))
    for i in range(l):
        acc = (acc * 2 + R[:, i]) % p
    return (a + (1 << l) + acc + (rd << l)) % p, acc


def expand_ref(p, l, c, a, R, sb, acc):
    n = len(a)
    cl = c & ((1 << l) - 1)
    s = (2 * sb - 1) % p
    S = obj([0] * n)
    e, nx = np.empty((l + 1, n), dtype=object), np.empty((l, n), dtype=object)
    for i in range(l):
        cb, r = (cl >> (l - 1 - i)) & 1, R[:, i]
        x = np.where(cb == 1, (1 - r) % p, r)
        e[i] = (s - cb + r + 3 * S) % p
        nx[i] = (1 - x) % p
        S = (S + x) % p
    e[l] = (s - 1 + 3 * S) % p
    return e, nx, (cl - a - (1 << l) - acc) % p


def finish_ref(p, l, w, sb, z):
    s = 2 * sb - 1
    h = np.where(w == 0, -s, s) + 3
    return (z + h * (1 << (l - 1))) * pow(1 << l, -1, p) % p


def view(engine, ctx, x, lo, hi):
    return engine.DevArray(ctx, x.t[lo:hi], hi - lo)


def same(x, want_t):
    return bool(torch.equal(x.t.reshape(-1), want_t.reshape(-1)))


class Data:
    """inputs of NMAX elements for one (field, l) with their expected outputs on the device; every smaller n is a
    prefix (rbits is element-major, the outputs are column prefixes of the bit-major matrices)"""

    def __init__(self, engine, ctx, p, l, seed):
        rng = np.random.default_rng(seed)
        n = NMAX
        self.l, self.n = l, n
        self.a, self.sb, self.rd = draw(rng, p, n), draw(rng, p, n), draw(rng, p, n)
        self.rb = draw(rng, p, n * l)
        self.c, self.w = draw(rng, p, n), draw(rng, p, n)
        edge = [0, p - 1, (1 << l) - 1, 1 << l, (1 << l) + 1, p - 2]
        self.c[1:1 + len(edge)] = edge                 # (c[0] stays random: n = 1)
        self.c[256:256 + len(edge)] = edge
        self.w[::3] = 0
        self.a[:3], self.sb[:3], self.rb[:3] = [0, p - 1, 1], [p - 1, 0, 1], [p - 1, 0, 1]
        R = self.rb.reshape(n, l)
        self.masked, acc = mask_ref(p, l, self.a, R, self.rd)
        self.e, self.nx, self.z = expand_ref(p, l, self.c, self.a, R, self.sb, acc)
        self.lt = finish_ref(p, l, self.w, self.sb, self.z)
        up = lambda v: ctx.from_ints(v.reshape(-1))
        self.d = {k: up(getattr(self, k)) for k in ('a', 'sb', 'rd', 'rb', 'c', 'w', 'masked', 'e', 'nx', 'z', 'lt')}

    def rows(self, key, nrows, n):
        """columns 0 .. n-1 of the expected bit-major (nrows, NMAX) matrix"""
        t = self.d[key].t
        return t.reshape((nrows, self.n) + tuple(t.shape[1:]))[:, :n].contiguous()


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    ran = 0
    for l in ALL_L:
        if l > p.bit_length() - 2:
            continue
        D = Data(engine, ctx, p, l, seed=1000 + l)
        d = D.d
        for n in sizes():
            v = lambda k, per=1: view(engine, ctx, d[k], 0, n * per)
            masked = ctx.sgn_mask(v('a'), v('rb', l), v('rd'), l)
            e, nx, z = ctx.sgn_expand(v('c'), v('a'), v('rb', l), v('sb'), l, want_e=True, want_nx=True)
            lt = ctx.sgn_finish(v('w'), v('sb'), v('z'), l)
            tag = (name, l, n)
            assert same(masked, d['masked'].t[:n]), ('mask',) + tag
            assert same(e, D.rows('e', l + 1, n)), ('e',) + tag
            assert same(nx, D.rows('nx', l, n)), ('nx',) + tag
            assert same(z, d['z'].t[:n]), ('z',) + tag
            assert same(lt, d['lt'].t[:n]), ('finish',) + tag
            ran += 1
    assert ran >= 3 * len(sizes())


def _call_expand(ctx, d, l, n, e, nx, z, sbit=True):
    P = lambda x: x.ptr if x is not None else None
    return ctx._L.ffgpu_sgn_expand(ctx._h, d['c'].ptr, d['a'].ptr, d['rb'].ptr, d['sb'].ptr if sbit else None, l, P(e), P(nx),
                                   P(z), n, ctx._stream())


@pytest.mark.parametrize('name', ['pm64-mersenne', 'pm96', 'pm192'])
def test_null_output_combinations(mods, name):
    _ffi, engine, _, _ = mods
    p, l, n = FIELDS[name], 7, 777
    ctx = engine.FieldContext(p, device=0)
    D = Data(engine, ctx, p, l, seed=5)
    want = {'e': D.rows('e', l + 1, n), 'nx': D.rows('nx', l, n), 'z': D.d['z'].t[:n]}
    size = {'e': (l + 1) * n, 'nx': l * n, 'z': n}
    for keys in (('e',), ('nx',), ('z',), ('e', 'nx'), ('e', 'z'), ('nx', 'z'), ('e', 'nx', 'z')):
        out = {k: ctx.empty(size[k]) if k in keys else None for k in size}
        rc = _call_expand(ctx, D.d, l, n, out['e'], out['nx'], out['z'], sbit='e' in keys)
        assert rc == _ffi.OK, keys
        for k in keys:
            assert same(out[k], want[k]), (keys, k)


@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
def test_nothing_is_written_outside_the_outputs(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    l, n, pad = min(16, p.bit_length() - 2), 300, 240          # 240: a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    eb = ctx.elem_bytes
    D = Data(engine, ctx, p, l, seed=6)
    d = D.d
    before = {k: d[k].t.clone() for k in ('a', 'sb', 'rd', 'rb', 'c', 'w', 'z')}

    def guarded(nelem):
        buf = torch.full((pad + nelem * eb + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        return buf, buf.data_ptr() + pad

    def check(buf, nelem, want_t):
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + nelem * eb:] == 0xa5).all())
        got = buf[pad:pad + nelem * eb]
        assert torch.equal(got, want_t.contiguous().view(torch.uint8).reshape(-1))

    L, h, st = ctx._L, ctx._h, ctx._stream()
    bm, pm = guarded(n)
    assert L.ffgpu_sgn_mask(h, d['a'].ptr, d['rb'].ptr, d['rd'].ptr, l, pm, n, st) == _ffi.OK
    check(bm, n, d['masked'].t[:n])
    (be, pe), (bx, px), (bz, pz) = guarded((l + 1) * n), guarded(l * n), guarded(n)
    assert L.ffgpu_sgn_expand(h, d['c'].ptr, d['a'].ptr, d['rb'].ptr, d['sb'].ptr, l, pe, px, pz, n, st) == _ffi.OK
    check(be, (l + 1) * n, D.rows('e', l + 1, n))
    check(bx, l * n, D.rows('nx', l, n))
    check(bz, n, d['z'].t[:n])
    bl, pl = guarded(n)
    assert L.ffgpu_sgn_finish(h, d['w'].ptr, d['sb'].ptr, d['z'].ptr, l, pl, n, st) == _ffi.OK
    check(bl, n, d['lt'].t[:n])
    for k, t in before.items():
        assert torch.equal(d[k].t, t), f'input {k} was written'


def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p, l, n = 2**61 - 1, 16, 300
    ctx = engine.FieldContext(p, device=0)
    D = Data(engine, ctx, p, l, seed=7)
    d = D.d
    L, h, st = ctx._L, ctx._h, ctx._stream()
    pat = lambda k: torch.full((k * ctx.elem_bytes,), 0x5a, dtype=torch.uint8, device='cuda')
    E, X, Z, M = pat((l + 1) * n + 64 * n), pat(64 * n), pat(n), pat(n)
    ep, xp, zp, mp = E.data_ptr(), X.data_ptr(), Z.data_ptr(), M.data_ptr()
    a, rb, sb, rd, c, w, z = (d[k].ptr for k in ('a', 'rb', 'sb', 'rd', 'c', 'w', 'z'))
    EINVAL = _ffi.EINVAL
    for bad in (0, 65, p.bit_length() - 1, -1):
        assert L.ffgpu_sgn_mask(h, a, rb, rd, bad, mp, n, st) == EINVAL
        assert L.ffgpu_sgn_expand(h, c, a, rb, sb, bad, ep, xp, zp, n, st) == EINVAL
        assert L.ffgpu_sgn_finish(h, w, sb, z, bad, mp, n, st) == EINVAL
    assert L.ffgpu_sgn_mask(h, a, rb, rd, p.bit_length() - 2, mp, 0, st) == _ffi.OK           # the largest l; n == 0
    assert L.ffgpu_sgn_expand(h, c, a, rb, sb, l, ep, xp, zp, 0, st) == _ffi.OK
    assert L.ffgpu_sgn_finish(h, w, sb, z, l, mp, 0, st) == _ffi.OK
    assert L.ffgpu_sgn_expand(h, c, a, rb, None, l, ep, xp, zp, n, st) == EINVAL               # e needs the sign bit
    assert L.ffgpu_sgn_expand(h, c, a, rb, sb, l, None, None, None, n, st) == EINVAL           # no output at all
    assert L.ffgpu_sgn_expand(h, c, None, rb, sb, l, ep, xp, zp, n, st) == EINVAL
    assert L.ffgpu_sgn_expand(h, c, a, rb, sb, l, rb + 8, xp, zp, n, st) == EINVAL             # e inside rbits
    assert L.ffgpu_sgn_expand(h, c, a, rb, sb, l, ep, rb, zp, n, st) == EINVAL                 # nx is rbits
    assert L.ffgpu_sgn_expand(h, c, a, rb, sb, l, ep, ep + 8 * n, zp, n, st) == EINVAL         # nx inside e
    assert L.ffgpu_sgn_expand(h, c, a, rb, sb, l, ep, xp, a, n, st) == EINVAL                  # z is a
    assert L.ffgpu_sgn_mask(h, a, rb, rd, l, a, n, st) == EINVAL
    assert L.ffgpu_sgn_mask(h, a, rb, rd, l, rb + 8 * (n * l - 1), n, st) == EINVAL
    assert L.ffgpu_sgn_mask(h, a, None, rd, l, mp, n, st) == EINVAL
    assert L.ffgpu_sgn_finish(h, w, sb, z, l, z, n, st) == EINVAL
    assert L.ffgpu_sgn_finish(h, w, sb, None, l, mp, n, st) == EINVAL
    assert L.ffgpu_sgn_expand(h, c, a, rb, sb, 64, ep, xp, zp, (1 << 63), st) == EINVAL        # (l itself is too large here)
    assert L.ffgpu_sgn_expand(h, c, a, rb, sb, l, ep, xp, zp, (1 << 62), st) == EINVAL         # n * l overflows
    torch.cuda.synchronize()
    for buf, val in ((E, 0x5a), (X, 0x5a), (Z, 0x5a), (M, 0x5a)):
        assert bool((buf == val).all()), 'a refused call wrote'
    # binary fields
    for mod in (0x11b, (1 << 64) | 0x1b, (1 << 128) | 0x87):
        bctx = engine.FieldContext(mod, True, device=0)
        g = torch.zeros(4096, dtype=torch.uint8, device='cuda').data_ptr()
        assert bctx._L.ffgpu_sgn_mask(bctx._h, g, g + 512, g + 1024, 4, g + 2048, 4, st) == _ffi.ENOTSUP
        assert bctx._L.ffgpu_sgn_expand(bctx._h, g, g + 256, g + 512, g + 1024, 4, g + 2048, None, None, 4, st) == _ffi.ENOTSUP
        assert bctx._L.ffgpu_sgn_finish(bctx._h, g, g + 512, g + 1024, 4, g + 2048, 4, st) == _ffi.ENOTSUP
    with pytest.raises(ValueError):
        ctx.sgn_mask(d['a'], d['rb'], d['rd'], l + 1)
    with pytest.raises(ValueError):
        ctx.sgn_expand(d['c'], d['a'], d['rb'], None, l)


def signed_values(rng, l, n):
    lo, hi = -(1 << (l - 1)), (1 << (l - 1)) - 1
    vals = [lo, hi, 0, -1, 1, lo + 1, hi - 1, 0]
    return vals + [rng.randint(lo, hi) for _ in range(n - len(vals))]


@pytest.mark.parametrize('modulus,l', [(2**61 - 1, 16), (2**64 - 189, 32)], ids=['2^61-1', '2^64-189'])
@pytest.mark.parametrize('m,t', [(3, 1), (7, 3)])
def test_compare_zero_end_to_end(mods, modulus, l, m, t):
    _ffi, engine, finfields, protocols = mods
    from oracle import pyoracle as po
    F = finfields.GF(modulus)
    ctx = engine.FieldContext(modulus, device=0)
    rng = random.Random(l * 100 + m)
    n = 1031
    a = signed_values(rng, l, n)
    sh = lambda vals: protocols.share(ctx, ctx.from_ints([v % modulus for v in vals]), t, m)
    xs = sh(a)
    rbits, sbits = sh([rng.randrange(2) for _ in range(n * l)]), sh([rng.randrange(2) for _ in range(n)])
    rdivl, rzero = sh([rng.randrange(1 << 24) for _ in range(n)]), sh([rng.randrange(1, modulus) for _ in range(n)])
    pick = sorted(rng.sample(range(m), t + 1))
    lam = [int(v) for v in po.recombination_vector(po.Field(modulus, False), [i + 1 for i in pick], 0)]
    signed = lambda v: v - modulus if v > modulus // 2 else v
    for mode, want in (('lt', [int(v < 0) for v in a]), ('eq', [int(v == 0) for v in a]),
                       ('sgn', [(v > 0) - (v < 0) for v in a])):
        eq_mode = mode == 'eq'
        out = protocols.compare_zero(ctx, F, xs, rbits, None if eq_mode else sbits, rdivl, None if eq_mode else rzero, t, l,
                                     mode=mode)
        assert len(out) == m
        assert [signed(v) for v in protocols.open_(ctx, F, out, t).to_ints()] == want, mode
        assert [signed(v) for v in ctx.recombine([out[i] for i in pick], lam).to_ints()] == want, mode   # any t+1 shares


def composed_steps(engine, ctx, p, l, a, rbits, sbit, rdivl, c, w):
    """the three local steps from the calls the engine had before: matmul with the power vector, element-wise calls, scan;
    the public c_bits, c mod 2^l and (1 - 2g) are built on the host and uploaded, as the reference's np_sgn does"""
    n = a.n
    def cat(ts):
        t = torch.cat([x.t for x in ts])
        return engine.DevArray(ctx, t, t.shape[0])
    pw = ctx.from_ints([1 << (l - 1 - i) for i in range(l)])
    a_r = ctx.add_scalar(ctx.add(a, ctx.matmul(rbits, pw, n, l, 1)), 1 << l)
    masked = ctx.add(a_r, ctx.mul_scalar(rdivl, (1 << l) % p))
    cl = [v & ((1 << l) - 1) for v in c.to_ints()]
    z = ctx.sub(ctx.from_ints(cl), a_r)
    CB = ctx.from_ints([(v >> (l - 1 - i)) & 1 for i in range(l) for v in cl])
    rt = rbits.t.reshape((n, l) + tuple(rbits.t.shape[1:])).transpose(0, 1).contiguous()
    rT = engine.DevArray(ctx, rt.reshape((n * l,) + tuple(rbits.t.shape[1:])), n * l)
    xor = ctx.sub(ctx.add(CB, rT), ctx.mul_scalar(ctx.mul(CB, rT), 2))
    sums = ctx.scan(xor, 1, l, n, with_initial=True)
    s = ctx.add_scalar(ctx.mul_scalar(sbit, 2), p - 1)
    e = ctx.add(ctx.sub(cat([s] * (l + 1)), cat([ctx.sub(CB, rT), ctx.from_ints([1] * n)])), ctx.mul_scalar(sums, 3))
    nx = ctx.rsub_scalar(xor, 1)
    gm = ctx.from_ints([(p - 1) if v == 0 else 1 for v in w.to_ints()])
    h = ctx.add_scalar(ctx.mul(gm, s), 3)
    lt = ctx.mul_scalar(ctx.add(z, ctx.mul_scalar(h, 1 << (l - 1))), pow(1 << l, -1, p))
    return masked, e, nx, z, lt


@pytest.mark.parametrize('modulus,l', [(2**61 - 1, 16), (2**64 - 189, 32), (2**80 - 65, 33)], ids=['2^61-1', '2^64-189', '2^80-65'])
def test_same_bytes_as_the_composition_of_existing_calls(mods, modulus, l):
    """every local step equals, bit for bit, what the calls of the engine that existed before compute for the same
    inputs -- so with the same openings (c, w) the share of [a < 0] is the same share"""
    _ffi, engine, finfields, protocols = mods
    ctx = engine.FieldContext(modulus, device=0)
    F = finfields.GF(modulus)
    rng = random.Random(l)
    n, t, m = 1031, 1, 3
    sh = lambda vals: protocols.share(ctx, ctx.from_ints([v % modulus for v in vals]), t, m)
    a = signed_values(rng, l, n)
    xs, rbits, sbits = sh(a), sh([rng.randrange(2) for _ in range(n * l)]), sh([rng.randrange(2) for _ in range(n)])
    rdivl = sh([rng.randrange(1 << 24) for _ in range(n)])
    c = protocols.open_(ctx, F, [ctx.sgn_mask(xs[i], rbits[i], rdivl[i], l) for i in range(m)], t)
    w = ctx.from_ints([0 if i % 2 else rng.randrange(1, modulus) for i in range(n)])
    for i in range(m):
        masked, e, nx, z, lt = composed_steps(engine, ctx, modulus, l, xs[i], rbits[i], sbits[i], rdivl[i], c, w)
        assert same(ctx.sgn_mask(xs[i], rbits[i], rdivl[i], l), masked.t)
        e2, nx2, z2 = ctx.sgn_expand(c, xs[i], rbits[i], sbits[i], l, want_e=True, want_nx=True)
        assert same(e2, e.t) and same(nx2, nx.t) and same(z2, z.t)
        assert same(ctx.sgn_finish(w, sbits[i], z2, l), lt.t)


def test_graph_capture_replays_the_three_calls(mods):
    _ffi, engine, _, _ = mods
    p, l, n = 2**64 - 189, 32, 5003
    ctx = engine.FieldContext(p, device=0)
    D = Data(engine, ctx, p, l, seed=8)
    d = D.d

    def steps():
        masked = ctx.sgn_mask(d['a'], d['rb'], d['rd'], l)
        e, nx, z = ctx.sgn_expand(d['c'], d['a'], d['rb'], d['sb'], l, want_e=True, want_nx=True)
        return masked, e, nx, z, ctx.sgn_finish(d['w'], d['sb'], z, l)

    cg = engine.CapturedLaunches(steps)
    want = (d['masked'].t, d['e'].t, d['nx'].t, d['z'].t, d['lt'].t)
    for _ in range(2):
        for out in cg.result:
            out.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        for out, wt in zip(cg.result, want):
            assert same(out, wt)
