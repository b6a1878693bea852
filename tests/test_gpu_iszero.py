"""The local steps of the Legendre zero test on the device (ffgm_iszero_mask / _legendre_code / _iszero_finish,
mpyc_amd/csrc/iszero.hpp) against Python integers computed here from the maps include/ffgpu_math.h states, over every prime
policy; guard bytes around every output (the byte array included), inputs unchanged, views one element into their buffers,
status codes, protocols.is_zero end to end for all parties on one GPU -- its local steps share for share against the
Python-integer stand-in, the whole against a model on the same draws and, at k = 30, against the truth and the reference's
recorded results (tests/golden/iszero/iszero.json) -- and mask -> code -> finish replayed from a captured HIP graph."""
import random

import numpy as np
import pytest

from test_gpu_sgn import FIELDS as SGN_FIELDS, draw, same, view
from test_gpu_fxp import up
from test_iszero_host import ZeroRun, golden, model, run_zero

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

BLUM40 = 2**40 - 213                                        # the Blum prime of the pm64-gen policy (2^40 - 87 is 1 mod 4)
FIELDS = dict(SGN_FIELDS, **{'pm64-gen-blum': BLUM40})
ALL_N = (1, 63, 64, 65, 255, 256, 257, 5003)
ALL_K = (1, 2, 8, 9, 30)
NMAX, KMAX = 5003, 30
COUNTS = sorted({k * n for k in ALL_K for n in ALL_N})


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def is_prime(n):
    """Miller-Rabin with the first twelve primes as bases: deterministic below 3.3 10^24"""
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for q in small:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_the_fields(mods):
    """nine of the ten primes of the comparison tests are Blum; 2^40 - 213 is prime, Blum, and takes the policy of 2^40 - 87 by
    the rule of policy_build.hpp: 33..64 bits, c = 2^k - p below 2^min((k-1)/2, 31), neither c == 1 nor k == 64"""
    _ffi, engine, _, _ = mods
    assert sorted(name for name, p in SGN_FIELDS.items() if p % 4 != 3) == ['pm64-gen'] and len(SGN_FIELDS) == 10
    assert is_prime(BLUM40) and BLUM40 % 4 == 3 and is_prime(2**40 - 87) and not is_prime(2**40 - 211)
    for p in (BLUM40, SGN_FIELDS['pm64-gen']):
        k = p.bit_length()
        c = (1 << k) - p
        assert 32 < k < 64 and 1 < c < (1 << min((k - 1) // 2, 31))
        ctx = engine.FieldContext(p, device=0)
        assert ctx.elem_bytes == 8 and ctx.reduction == engine.FieldContext(SGN_FIELDS['pm64-gen'], device=0).reduction


def code_ref(p, c):
    half = (p - 1) // 2
    return np.array([2 if v == 0 else 1 if pow(int(v), half, p) == 1 else 0 for v in c], dtype=np.uint8)


def nonresidue(p):
    return next(v for v in range(2, 100) if pow(v, (p - 1) // 2, p) == p - 1)


class Data:
    """(KMAX, NMAX) operands of the three kernels with their expected outputs on the device, computed once; a (k, n) case is
    rows < k and columns < n of the mask's matrices, and the first k n entries of the flat arrays of the symbols and the finish"""

    def __init__(self, ctx, p, seed):
        rng = np.random.default_rng(seed)
        K, N = KMAX, NMAX
        self.p = p
        a = draw(rng, p, N)
        a[:6] = [0, 1, p - 1, p - 1, 2, p - 2]
        a[::5] = p - 1
        r, z, u2 = (draw(rng, p, K * N).reshape(K, N) for _ in range(3))
        z[2:] = z[2:] % 2                                       # bits below, shares of bits (any element) in rows 0 and 1
        r[0, :64], z[0, :64], u2[0, :64] = p - 1, 1, p - 1      # both products (p - 1)^2: the bound of the lazy accumulator
        r[1], z[1], u2[1] = p - 1, 1, p - 1                     # ... over a whole row
        r[2, :4], z[2, :4], u2[2, :4] = [0, 1, 0, p - 1], [0, 1, p - 1, 0], [0, 0, 1, p - 1]
        r[K - 1, N - 3:], z[K - 1, N - 3:], u2[K - 1, N - 3:] = [0, 1, p - 1], [1, 0, 1], [p - 1, 0, 1]
        self.mask = (a[None, :] * r + (1 - 2 * z) * u2) % p
        # the symbols: public values with planted 0, 1, p - 1, a residue and a non-residue at the first and at every last index
        c = draw(rng, p, K * N)
        nr = nonresidue(p)
        plant = [0, 1, p - 1, 4, nr, nr * 4 % p, pow(nr, 2, p), p - 4]
        c[:len(plant)] = plant
        for i, cnt in enumerate(COUNTS):
            c[cnt - 1] = plant[i % len(plant)]
        self.code = code_ref(p, c)
        assert self.code[:5].tolist() == [2, 1, 1 if p % 4 == 1 else 0, 1, 0] and self.code[6] == 1
        zf = draw(rng, p, K * N)
        zf[:4] = [0, 1, p - 1, 2]
        self.fin = np.where(self.code == 0, zf, np.where(self.code == 1, (1 - zf) % p, 1))
        self.host = {'a': a, 'r': r, 'z': z, 'u2': u2, 'c': c, 'zf': zf}
        self.d = {k_: up(ctx, v) for k_, v in self.host.items()}
        self.d.update(mask=up(ctx, self.mask), fin=up(ctx, self.fin))
        self.dcode = torch.from_numpy(self.code).cuda()

    def sub(self, ctx, engine, key, k, n):
        """rows < k, columns < n of a (KMAX, NMAX) matrix on the device, as a fresh contiguous array"""
        t = self.d[key].t
        t = t.reshape((KMAX, NMAX) + tuple(t.shape[1:]))[:k, :n].contiguous()
        return engine.DevArray(ctx, t.reshape((k * n,) + tuple(t.shape[2:])), k * n)


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    D = Data(ctx, p, seed=31 + p % 997)
    keep = {k_: v.t.clone() for k_, v in D.d.items()}
    ran = 0
    for n in ALL_N:
        a = view(engine, ctx, D.d['a'], 0, n)
        for k in ALL_K:
            r, z, u2 = (D.sub(ctx, engine, key, k, n) for key in ('r', 'z', 'u2'))
            got = ctx.iszero_mask(a, r, z, u2, k)
            assert got.n == k * n and same(got, D.sub(ctx, engine, 'mask', k, n).t), ('mask', name, n, k)
            cnt = k * n
            code = ctx.legendre_code(view(engine, ctx, D.d['c'], 0, cnt))
            assert code.dtype == torch.uint8 and code.shape == (cnt,) and torch.equal(code, D.dcode[:cnt]), ('code', name, n, k)
            fin = ctx.iszero_finish(D.dcode[:cnt], view(engine, ctx, D.d['zf'], 0, cnt))
            assert same(fin, D.d['fin'].t[:cnt]), ('finish', name, n, k)
            ran += 1
    assert ran == 40
    # one element (one byte) into their buffers: the element path, and the codes off their alignment
    n, k = 2048, 3
    cnt = k * n
    lead = lambda x, count: view(engine, ctx, torch_cat_lead(engine, ctx, x, count), 1, 1 + count)
    r, z, u2, want = (D.sub(ctx, engine, key, k, n) for key in ('r', 'z', 'u2', 'mask'))
    out = view(engine, ctx, ctx.empty(cnt + 1), 1, 1 + cnt)
    assert ctx.iszero_mask(lead(view(engine, ctx, D.d['a'], 0, n), n), lead(r, cnt), lead(z, cnt), lead(u2, cnt), k, out=out) is out
    assert same(out, want.t), ('mask, offset views', name)
    cbuf = torch.full((cnt + 2,), 0xa5, dtype=torch.uint8, device='cuda')
    assert ctx.legendre_code(view(engine, ctx, D.d['c'], 1, 1 + cnt), out=cbuf[1:1 + cnt]).data_ptr() == cbuf.data_ptr() + 1
    assert torch.equal(cbuf[1:1 + cnt], D.dcode[1:1 + cnt]) and cbuf[0] == 0xa5 and cbuf[-1] == 0xa5, ('code, offset views', name)
    out = view(engine, ctx, ctx.empty(cnt + 1), 1, 1 + cnt)
    ctx.iszero_finish(D.dcode[1:1 + cnt], view(engine, ctx, D.d['zf'], 1, 1 + cnt), out=out)
    assert same(out, D.d['fin'].t[1:1 + cnt]), ('finish, offset views', name)
    # aligned elements, codes one byte off: packs are refused for the codes alone
    cnt = 4096
    ctx.legendre_code(view(engine, ctx, D.d['c'], 0, cnt), out=cbuf[1:1 + cnt])
    assert torch.equal(cbuf[1:1 + cnt], D.dcode[:cnt]) and cbuf[0] == 0xa5
    shifted = torch.cat([cbuf[:1], D.dcode[:cnt]])[1:]
    assert same(ctx.iszero_finish(shifted, view(engine, ctx, D.d['zf'], 0, cnt)), D.d['fin'].t[:cnt])
    assert all(torch.equal(D.d[k_].t, keep[k_]) for k_ in keep) and torch.equal(D.dcode.cpu(), torch.from_numpy(D.code)), 'an input was written'
    if p % 4 != 3:
        _, _, finfields, protocols = mods
        run = ZeroRun(ctx, 3, 1, seed=1)
        with pytest.raises(ValueError):
            protocols.is_zero(ctx, run.F, run.share([0, 5]), 1, 8, lambda count: pytest.fail('no randomness may be drawn'))


def torch_cat_lead(engine, ctx, x, count):
    """x behind one unused element, in a fresh buffer"""
    buf = ctx.empty(count + 1)
    buf.t[1:].copy_(x.t)
    buf.t[:1].copy_(x.t[:1])
    return buf


# ---- guard bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
@pytest.mark.parametrize('n,k', [(320, 3), (301, 2)])
def test_nothing_is_written_outside_the_outputs(mods, name, n, k):
    """n = 320: whole packs (and whole waves of 24-byte elements) in all three kernels; n = 301: the element paths and the tail"""
    _ffi, engine, _, _ = mods
    p, pad = FIELDS[name], 240                                  # 240: a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    eb, cnt = ctx.elem_bytes, k * n
    rng = np.random.default_rng(79)
    a, r, z, u2, c, zf = draw(rng, p, n), draw(rng, p, cnt), draw(rng, p, cnt), draw(rng, p, cnt), draw(rng, p, cnt), draw(rng, p, cnt)
    c[:3], c[-1] = [0, 1, p - 1], 0
    inputs = [up(ctx, v) for v in (a, r, z, u2, c, zf)]
    da, dr, dz, du, dc, dzf = inputs
    keep = [v.t.clone() for v in inputs]
    code = code_ref(p, c)
    dcode = torch.from_numpy(code).cuda()

    def guarded(nbytes):
        buf = torch.full((pad + nbytes + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        return buf, buf.data_ptr() + pad

    def check(buf, nbytes, want_bytes):
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + nbytes:] == 0xa5).all()), 'guard bytes written'
        assert torch.equal(buf[pad:pad + nbytes], want_bytes)

    as_bytes = lambda vals: up(ctx, vals).t.contiguous().view(torch.uint8).reshape(-1)
    L, hd, st = ctx._L, ctx._h, ctx._stream()
    b1, p1 = guarded(cnt * eb)
    assert L.ffgm_iszero_mask(hd, da.ptr, dr.ptr, dz.ptr, du.ptr, k, p1, n, st) == _ffi.OK
    check(b1, cnt * eb, as_bytes((np.tile(a, k) * r + (1 - 2 * z) * u2) % p))
    b2, p2 = guarded(cnt)
    assert L.ffgm_legendre_code(hd, dc.ptr, p2, cnt, st) == _ffi.OK
    check(b2, cnt, dcode)
    b3, p3 = guarded(cnt * eb)
    assert L.ffgm_iszero_finish(hd, dcode.data_ptr(), dzf.ptr, p3, cnt, st) == _ffi.OK
    check(b3, cnt * eb, as_bytes(np.where(code == 0, zf, np.where(code == 1, (1 - zf) % p, 1))))
    assert all(torch.equal(v.t, k_) for v, k_ in zip(inputs, keep)) and torch.equal(dcode.cpu(), torch.from_numpy(code)), 'an input was written'


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
def test_status_codes(mods):
    _ffi, engine, _, _ = mods
    p, n, k = 2**61 - 1, 300, 4
    ctx = engine.FieldContext(p, device=0)
    L, h, st = ctx._L, ctx._h, ctx._stream()
    eb, cnt = ctx.elem_bytes, k * n
    pat = lambda count: torch.full((count,), 0x5a, dtype=torch.uint8, device='cuda')
    A, R, Z, U, O, C = pat(n * eb), pat(cnt * eb), pat(cnt * eb), pat(cnt * eb), pat(cnt * eb), pat(cnt)
    a, r, z, u, o, c = (b.data_ptr() for b in (A, R, Z, U, O, C))
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    mask = lambda a_=a, r_=r, z_=z, u_=u, k_=k, o_=o, n_=n: L.ffgm_iszero_mask(h, a_, r_, z_, u_, k_, o_, n_, st)
    code = lambda c_=r, o_=c, n_=cnt: L.ffgm_legendre_code(h, c_, o_, n_, st)
    fin = lambda c_=c, z_=z, o_=o, n_=cnt: L.ffgm_iszero_finish(h, c_, z_, o_, n_, st)
    # the row count
    assert mask(k_=0) == EINVAL and mask(k_=-1) == EINVAL and mask(k_=0, n_=0) == EINVAL
    # a null context or required pointer
    assert L.ffgm_iszero_mask(None, a, r, z, u, k, o, n, st) == EINVAL and L.ffgm_legendre_code(None, r, c, cnt, st) == EINVAL
    assert L.ffgm_iszero_finish(None, c, z, o, cnt, st) == EINVAL
    assert mask(a_=None) == EINVAL and mask(r_=None) == EINVAL and mask(z_=None) == EINVAL and mask(u_=None) == EINVAL and mask(o_=None) == EINVAL
    assert code(c_=None) == EINVAL and code(o_=None) == EINVAL
    assert fin(c_=None) == EINVAL and fin(z_=None) == EINVAL and fin(o_=None) == EINVAL
    # sizes overflowing: k n, k n eb, count eb
    assert mask(n_=1 << 62) == EINVAL and mask(n_=1 << 60) == EINVAL and mask(k_=1 << 30, n_=1 << 40) == EINVAL
    assert mask(k_=3, n_=(1 << 64) // 3 + 1) == EINVAL
    for big in (1 << 62, 1 << 60):
        assert code(n_=big) == EINVAL and fin(n_=big) == EINVAL
    # overlaps: an output on an input
    assert mask(o_=a) == EINVAL and mask(o_=r) == EINVAL and mask(o_=z + eb * (cnt - 1)) == EINVAL and mask(o_=u) == EINVAL
    assert mask(a_=o + eb * (cnt - 1)) == EINVAL
    assert code(o_=r) == EINVAL and code(o_=r + eb * cnt - 1) == EINVAL
    assert fin(o_=z) == EINVAL and fin(c_=o + 5) == EINVAL and fin(o_=z + eb * (cnt - 1)) == EINVAL
    torch.cuda.synchronize()
    for buf in (A, R, Z, U, O, C):
        assert bool((buf == 0x5a).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    assert mask(n_=0, a_=None, r_=None, z_=None, u_=None, o_=None) == OK and mask(n_=0, k_=1 << 30) == OK
    assert code(n_=0, c_=None, o_=None) == OK and fin(n_=0, c_=None, z_=None, o_=None) == OK
    torch.cuda.synchronize()
    for buf in (A, R, Z, U, O, C):
        assert bool((buf == 0x5a).all())
    # valid calls, for contrast (inputs may alias each other; the operands are canonical)
    for buf in (A, R, Z, U):
        buf.zero_()
    assert mask() == OK and mask(k_=1) == OK and mask(r_=u, z_=u) == OK and code() == OK and fin() == OK and code(n_=1) == OK
    torch.cuda.synchronize()
    assert bool((C == 2).all()) and bool((O.view(torch.int64) == 1).all()), 'zeros everywhere: code 2, result 1'
    # binary fields, and the field of two elements
    for mod in (0x11b, (1 << 64) | 0x1b):
        bctx = engine.FieldContext(mod, True, device=0)
        g = torch.zeros(8192, dtype=torch.uint8, device='cuda').data_ptr()
        bl, bh = bctx._L, bctx._h
        assert bl.ffgm_iszero_mask(bh, g, g + 1024, g + 2048, g + 3072, 2, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgm_legendre_code(bh, g, g + 4096, 4, st) == ENOTSUP
        assert bl.ffgm_iszero_finish(bh, g, g + 1024, g + 4096, 4, st) == ENOTSUP
        for bad in (lambda: bctx.iszero_mask(bctx.empty(2), bctx.empty(4), bctx.empty(4), bctx.empty(4), 2),
                    lambda: bctx.legendre_code(bctx.empty(4)), lambda: bctx.iszero_finish(torch.zeros(4, dtype=torch.uint8, device='cuda'), bctx.empty(4))):
            with pytest.raises(NotImplementedError):
                bad()
    two = engine.FieldContext(2, device=0)
    g = torch.zeros(8192, dtype=torch.uint8, device='cuda')
    assert two._L.ffgm_legendre_code(two._h, g.data_ptr(), g.data_ptr() + 4096, 4, st) == ENOTSUP
    torch.cuda.synchronize()
    assert bool((g == 0).all())
    with pytest.raises(NotImplementedError):
        two.legendre_code(two.empty(4))
    # the engine's own checks
    e2, e8 = ctx.empty(2), ctx.empty(8)
    codes = torch.zeros(8, dtype=torch.uint8, device='cuda')
    for bad in (lambda: ctx.iszero_mask(e2, e8, e8, e8, 0), lambda: ctx.iszero_mask(e2, e8, e8, e8, 3), lambda: ctx.iszero_mask(e2, e8, e8, e2, 4),
                lambda: ctx.iszero_mask(e2, e8, e8, e8, 4, out=e2), lambda: ctx.legendre_code(e8, out=codes[:7]),
                lambda: ctx.legendre_code(e8, out=codes.to(torch.int8)), lambda: ctx.legendre_code(e8, out=codes.cpu()),
                lambda: ctx.legendre_code(e8, out=torch.zeros(16, dtype=torch.uint8, device='cuda')[::2]),
                lambda: ctx.iszero_finish(codes[:7], e8), lambda: ctx.iszero_finish(codes, e8, out=e2),
                lambda: ctx.iszero_finish(codes.to(torch.int32), e8)):
        with pytest.raises(ValueError):
            bad()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
E2E_FIELDS = ('pm64-mersenne', 'pm96', 'pm192')                 # 2^61 - 1, 2^80 - 65, 2^136 - 113
N_E2E = 257


def e2e_pairs(p):
    """the fixture's pairs that fit the field (64-bit operands need more than 2^61 - 1) first, then equal and unequal random
    ones; with the reference's recorded results"""
    e = golden()['equal'][1 if p.bit_length() < 70 else 0]
    a, b, want = list(e['a']), list(e['b']), list(e['equal'])
    assert all(abs(v) < p // 4 for v in a + b)
    rng = random.Random(p % 1000)
    while len(a) < N_E2E:
        x = rng.randrange(-(p // 4), p // 4)
        y = x if rng.randrange(2) else rng.randrange(-(p // 4), p // 4)
        a.append(x), b.append(y), want.append(int(x == y))
    return a[:N_E2E], b[:N_E2E], want[:N_E2E]


@pytest.mark.parametrize('m,t', [(3, 1), (7, 3)])
@pytest.mark.parametrize('k', (8, 30))
@pytest.mark.parametrize('name', E2E_FIELDS)
def test_is_zero_end_to_end(mods, name, k, m, t):
    _ffi, engine, finfields, protocols = mods
    from iszero_cpuctx import IszeroCpuFieldContext
    p = FIELDS[name]
    a, b, recorded = e2e_pairs(p)
    n = len(a)
    # the whole protocol on the device against the model on the same draws: the public values, the codes, the result
    res, want = run_zero(p, a, b, m, t, k, seed=8000 + 10 * k + m, ctx=engine.FieldContext(p, device=0))
    assert res == want
    if k == 30:
        assert want == [int(x == y) for x, y in zip(a, b)] == recorded, 'the model has a false positive: pick another seed'
    # the local steps share for share against the stand-in: the same shares in, the device's u2 handed to both
    dev, cpu = engine.FieldContext(p, device=0), IszeroCpuFieldContext(p)
    runs = [ZeroRun(ctx, m, t, seed=9000 + k + m) for ctx in (dev, cpu)]
    d = [(x - y) % p for x, y in zip(a, b)]
    xs = [run.share(d) for run in runs]
    for run in runs:
        run.n = n
    zrs = [run.rand_zero(k * n) for run in runs]
    assert all([v.to_ints() for v in w0] == [v.to_ints() for v in w1] for w0, w1 in zip(zrs[0], zrs[1]))
    u2_dev = protocols.multiply(dev, runs[0].F, zrs[0][2], zrs[0][2], t)
    u2 = [u2_dev, [cpu.from_ints(u.to_ints()) for u in u2_dev]]
    masked = [[ctx.iszero_mask(xs[j][i], zrs[j][1][i], zrs[j][0][i], u2[j][i], k) for i in range(m)] for j, ctx in enumerate((dev, cpu))]
    assert [v.to_ints() for v in masked[0]] == [v.to_ints() for v in masked[1]], 'mask: a share differs'
    cs = [protocols.open_(ctx, runs[j].F, masked[j], t, degree=2 * t) for j, ctx in enumerate((dev, cpu))]
    assert cs[0].to_ints() == cs[1].to_ints()
    codes = [ctx.legendre_code(c) for ctx, c in zip((dev, cpu), cs)]
    assert codes[0].tolist() == codes[1].tolist() and set(codes[0].tolist()) <= {0, 1, 2}
    fins = [[ctx.iszero_finish(codes[j], zrs[j][0][i]) for i in range(m)] for j, ctx in enumerate((dev, cpu))]
    assert [v.to_ints() for v in fins[0]] == [v.to_ints() for v in fins[1]], 'finish: a share differs'
    z, r, s = runs[0].draws[0]
    u2_plain = runs[0].open(u2_dev)
    assert [v % p for v in u2_plain] == [v * v % p for v in s]
    assert cs[0].to_ints() == model(p, d, k, z, r, s)[0]


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_mask_code_finish(mods):
    """one party's mask, the symbols of its masked values (standing in for the opened ones) and its finish, captured once on one
    stream, replayed on changed inputs, equal to the eager result"""
    _ffi, engine, _, _ = mods
    p, n, k = 2**80 - 65, 5003, 9
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(23)
    a, r, z, u2 = ctx.empty(n), ctx.empty(k * n), ctx.empty(k * n), ctx.empty(k * n)

    def steps():
        c = ctx.iszero_mask(a, r, z, u2, k)
        code = ctx.legendre_code(c)
        return c, code, ctx.iszero_finish(code, z)

    def load():
        vals = [draw(rng, p, n)] + [draw(rng, p, k * n) for _ in range(3)]
        vals[0][:2], vals[3][:2] = 0, 0                                        # zeros among the masked values
        for dst, v in zip((a, r, z, u2), vals):
            dst.t.copy_(up(ctx, v).t)
        return vals

    load()
    cg = engine.CapturedLaunches(steps)
    for _ in range(2):
        va, vr, vz, vu = load()
        c = (np.tile(va, k) * vr + (1 - 2 * vz) * vu) % p
        code = code_ref(p, c)
        for out in cg.result:
            (out if isinstance(out, torch.Tensor) else out.t).zero_()
        cg.replay()
        torch.cuda.synchronize()
        eager = steps()
        torch.cuda.synchronize()
        assert same(cg.result[0], up(ctx, c).t) and same(cg.result[0], eager[0].t)
        assert torch.equal(cg.result[1].cpu(), torch.from_numpy(code)) and torch.equal(cg.result[1], eager[1]) and code[0] == 2
        assert same(cg.result[2], up(ctx, np.where(code == 0, vz, np.where(code == 1, (1 - vz) % p, 1))).t) and same(cg.result[2], eager[2].t)
