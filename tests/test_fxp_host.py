"""CPU checks of fixed-point truncation, product, normalisation, reciprocal and division: the four C ABI entries exist in
header, library and binding; the compact index of the norm kernels and the launch plans (mpyc_amd/csrc/fxp_geom.hpp) walked by
tests/fxp_check.cpp with g++ against brute-force enumeration; protocols.trunc / fxp_multiply / norm / reciprocal / divide
composed over a Python-integer context (tests/fxp_cpuctx.py) open to the closed forms, to an independent integer model of the
whole chain fed the same randomness, and to the reference's values (tests/golden/fxp/fxp.json), and do not with a context
whose mask weighs the bits most significant first, whose finish forgets `mod 2^f`, whose norm_prod does not reverse or whose
norm_apply adds x_top.  No GPU needed."""
import json
import math
import os
import random
import re
import shutil
import subprocess

import pytest

from test_sort_host import _lagrange, _share, _signed

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, 'golden', 'fxp', 'fxp.json')
P61, P80, P127 = 2**61 - 1, 2**80 - 65, 2**127 - 1
CASES = [(3, 1), (7, 3)]


def test_fxp_entries_in_header_library_and_binding():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    for name, nparams in (('ffgpu_trunc_mask', 10), ('ffgpu_trunc_finish', 9), ('ffgpu_norm_prod', 7), ('ffgpu_norm_apply', 9)):
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, f'{name} is not declared in include/ffgpu.h'
        params = [p.strip() for p in m.group(1).split(',')]
        assert len(params) == nparams, params
        assert re.search(r' T ' + name + r'\b', out), f'{name} is not exported by libffgpu.so'
        assert name in _ffi.EXPORTED and len(_ffi._SIGS[name]) == nparams
    assert len(re.findall(r' T ffgpu_\w+', out)) == 104 == len(set(re.findall(r'\b(ffgpu_\w+)\s*\(', hdr)))
    L_ = _ffi.lib()
    # no context: refused before anything is touched
    assert L_.ffgpu_trunc_mask(None, None, None, None, None, 8, None, None, 1, None) == _ffi.EINVAL
    assert L_.ffgpu_trunc_finish(None, None, None, 1, None, 8, None, 1, None) == _ffi.EINVAL
    assert L_.ffgpu_norm_prod(None, None, 16, None, None, 1, None) == _ffi.EINVAL
    assert L_.ffgpu_norm_apply(None, None, None, None, 1, 16, None, 1, None) == _ffi.EINVAL


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_fxp_geometry_on_the_host(tmp_path):
    """l in 2..64, n in {1, 2, 63, 64, 65, 257}, five element sizes, both alignments: every compact index maps to in-range
    sources, every (h, j) is hit once, the pack decision agrees with alignment"""
    exe = str(tmp_path / 'fxp_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'fxp_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'fxp ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) > 3000


# ---- the protocols over Python integers -----------------------------------------------------------------------------------
class Run:
    """one protocol run over the stand-in: sharings, the two randomness callbacks (which record what they drew, as plain
    integers, in the order of the calls) and the opening"""

    def __init__(self, ctx, m, t, seed, rbound=1 << 16, nearest=False):
        import mpyc_amd.finfields as gff
        self.ctx, self.m, self.t, self.p = ctx, m, t, ctx.modulus
        self.F = gff.GF(self.p)
        self.rng = random.Random(seed)
        self.rbound = rbound
        self.nearest = nearest          # rand_trunc hands out the bits of 2^(f-1) for every element: see nearest_chains()
        self.truncs = []                # (f, r, R) per call of rand_trunc: the values of the random bits and of the high masks
        self.decomps = []               # (count, l) per call of rand_bits

    def share(self, vals):
        return _share(self.ctx, self.rng, [int(v) for v in vals], self.t, self.m)

    def rand_trunc(self, count, f):
        bits = ([0] * (f - 1) + [1]) * count if self.nearest else [self.rng.randrange(2) for _ in range(count * f)]
        R = [self.rng.randrange(self.rbound) for _ in range(count)]
        self.truncs.append((f, [sum(bits[h * f + k] << k for k in range(f)) for h in range(count)], R))
        return self.share(bits), self.share(R)

    def rand_bits(self, count, l):
        self.decomps.append((count, l))
        return self.share([self.rng.randrange(2) for _ in range(count * l)]), self.share([self.rng.randrange(self.rbound) for _ in range(count)])

    def open(self, shares):
        """the value from the first and from the last t+1 parties: both must agree"""
        res = []
        for pick in (list(range(self.t + 1)), list(range(self.m - self.t - 1, self.m))):
            lam = _lagrange(self.p, [i + 1 for i in pick])
            res.append([_signed(v, self.p) for v in self.ctx.recombine([shares[i] for i in pick], lam).to_ints()])
        assert res[0] == res[1], 'the sharing has degree above t'
        return res[0]


# ---- the independent integer model: no context, no protocols, only the closed forms of the issue -----------------------------
def trunc_model(a, r, R, f, L):
    """the integer np_trunc returns for the drawn randomness"""
    c = a + (1 << (L - 1)) + r + (R << f)
    y, rem = divmod(a + r - (c & ((1 << f) - 1)), 1 << f)
    assert rem == 0
    return y


def norm_model(a, l, f):
    """(2s - 1) 2^(i + 2f - l + 1): s the inverted sign bit, i the leading bits below the sign bit that differ from s"""
    s = 0 if a < 0 else 1
    i = 0
    while i < l - 1 and ((a >> (l - 2 - i)) & 1) != s:
        i += 1
    return (2 * s - 1) << (i + 2 * f - l + 1)


class Model:
    """the chain on plain integers; consumes the recorded truncation randomness in order"""

    def __init__(self, truncs, l, f):
        self.truncs, self.l, self.f, self.at = truncs, l, f, 0

    def mul(self, xs, ys):
        f, r, R = self.truncs[self.at]
        self.at += 1
        assert f == self.f and len(r) == len(xs)
        return [trunc_model(x * y, r[h], R[h], f, self.l + f) for h, (x, y) in enumerate(zip(xs, ys))]

    def reciprocal(self, a):
        f = self.f
        v = [norm_model(x, self.l, f) for x in a]
        b = self.mul(a, v)
        c = [round(2.9142135623731 * 2**f) - 2 * x for x in b]
        for _ in range(int(math.ceil(math.log2((f + 1) / 3.54)))):
            cb = self.mul(c, b)
            c = self.mul(c, [(1 << (f + 1)) - x for x in cb])
        return self.mul(c, v)

    def divide(self, num, den):
        return self.mul(self.reciprocal(den), num)


def golden():
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    assert [(c['l'], c['f']) for c in doc['cases']] == [(32, 16), (16, 8), (24, 12)] and doc['repeats'] == 8
    return doc['cases']


def modulus_for(l):
    return P61 if l <= 16 else P80


# ---- trunc ------------------------------------------------------------------------------------------------------------------
def trunc_inputs(rng, f, L):
    """negative values, multiples of 2^f, the range ends, random values"""
    hi = (1 << (L - 1)) - 1
    vals = [0, 1, -1, 1 << f, -(1 << f), 3 << f, -(5 << f), (1 << f) - 1, -((1 << f) - 1), (1 << f) + 1, hi, -hi, hi >> f << f, -(hi >> f << f)]
    return vals + [rng.randint(-hi, hi) for _ in range(26)]


def check_trunc(ctx, m, t, f, L, seed):
    """returns the elements where the opened value differs from the closed form or leaves {floor, floor + 1}"""
    from mpyc_amd import protocols
    run = Run(ctx, m, t, seed)
    vals = trunc_inputs(run.rng, f, L)
    xs = run.share(vals)
    before = [x.to_ints() for x in xs]
    rbits, rdivf = run.rand_trunc(len(vals), f)
    got = run.open(protocols.trunc(ctx, run.F, xs, rbits, rdivf, t, f, L))
    assert [x.to_ints() for x in xs] == before, 'trunc wrote its input'
    _, r, R = run.truncs[0]
    return [h for h, a in enumerate(vals) if got[h] != trunc_model(a, r[h], R[h], f, L) or got[h] not in (a >> f, (a >> f) + 1)]


@pytest.mark.parametrize('m,t', CASES)
@pytest.mark.parametrize('f', (1, 8, 16, 33, 64))
def test_trunc_opens_to_the_closed_form(m, t, f):
    from fxp_cpuctx import FxpCpuFieldContext
    L = f + 24
    assert check_trunc(FxpCpuFieldContext(P127), m, t, f, L, seed=100 * m + f) == []
    if f <= 16:
        assert check_trunc(FxpCpuFieldContext(P61), m, t, f, f + 16, seed=200 * m + f) == []


def test_trunc_against_the_reference():
    """the recorded np_trunc: the protocol's value lies in {floor, floor + 1} as every recorded one does, and wherever the
    reference's eight draws gave one value only because the low bits are zero, so does the protocol"""
    from fxp_cpuctx import FxpCpuFieldContext
    from mpyc_amd import protocols
    for i, case in enumerate(golden()):
        l, f = case['l'], case['f']
        ctx = FxpCpuFieldContext(modulus_for(l))
        run = Run(ctx, 3, 1, seed=300 + i)
        a = case['trunc_in']
        rbits, rdivf = run.rand_trunc(len(a), f)
        got = run.open(protocols.trunc(ctx, run.F, run.share(a), rbits, rdivf, 1, f, l + f))
        for x, y, lo, hi in zip(a, got, case['trunc_min'], case['trunc_max']):
            assert x >> f <= lo <= hi <= (x >> f) + 1 and y in (x >> f, (x >> f) + 1)
            if x % (1 << f) == 0:
                assert lo == hi == y == x >> f


# ---- norm --------------------------------------------------------------------------------------------------------------------
def norm_inputs(rng, l):
    vals = [1, -1, 1 << (l - 2), -(1 << (l - 2)), -(1 << (l - 1)), (1 << (l - 1)) - 1]
    vals += [1 << k for k in range(l - 1)] + [-(1 << k) for k in range(l - 1)]
    return vals + [rng.randint(-(1 << (l - 1)), (1 << (l - 1)) - 1) for _ in range(20)]


def check_norm(ctx, m, t, l, f, vals, seed):
    from mpyc_amd import protocols
    run = Run(ctx, m, t, seed)
    xs = run.share(vals)
    before = [x.to_ints() for x in xs]
    got = run.open(protocols.norm(ctx, run.F, xs, t, l, f, run.rand_bits))
    assert [x.to_ints() for x in xs] == before and run.decomps == [(len(vals), l)]
    return got


@pytest.mark.parametrize('m,t', CASES)
@pytest.mark.parametrize('l,f', [(16, 8), (32, 16), (24, 12), (17, 8), (9, 9), (2, 1)])
def test_norm_opens_to_the_closed_form(m, t, l, f):
    from fxp_cpuctx import FxpCpuFieldContext
    vals = norm_inputs(random.Random(l), l)
    got = check_norm(FxpCpuFieldContext(modulus_for(l)), m, t, l, f, vals, seed=10 * m + l)
    assert got == [norm_model(a, l, f) for a in vals]
    assert norm_model(-1, l, f) == -(1 << (2 * f)) and norm_model(1, l, f) == 1 << (l - 2 + 2 * f - l + 1)


@pytest.mark.parametrize('m,t', CASES)
def test_norm_opens_to_the_reference(m, t):
    from fxp_cpuctx import FxpCpuFieldContext
    for i, case in enumerate(golden()):
        l, f = case['l'], case['f']
        for key_in, key in (('norm_in', 'norm'), ('den', 'den_norm')):
            assert [norm_model(a, l, f) for a in case[key_in]] == case[key]
            if m == 3 or key == 'norm':
                assert check_norm(FxpCpuFieldContext(modulus_for(l)), m, t, l, f, case[key_in], seed=400 + i) == case[key]


def test_norm_refuses_bit_lengths_outside_f_to_2f_plus_1():
    from fxp_cpuctx import FxpCpuFieldContext
    from mpyc_amd import protocols
    ctx = FxpCpuFieldContext(P61)
    run = Run(ctx, 3, 1, seed=1)
    xs = run.share([5, -5])
    for l, f in ((7, 8), (18, 8), (1, 1)):
        with pytest.raises(ValueError):
            protocols.norm(ctx, run.F, xs, 1, l, f, run.rand_bits)
    with pytest.raises(ValueError):
        protocols.norm(ctx, run.F, xs[:2], 1, 16, 8, run.rand_bits)


# ---- the party-count and the axis-shape check, one each for all protocols ---------------------------------------------------
def _no_draw(*_):
    raise AssertionError('no randomness may be drawn')


def _compare_zero(P, c, F, xs, ys, mode):
    """three values of l = 4 bits: the first rows of xs as values and masks, ys as the 12 bit shares"""
    three = [P._rows(c, x, 0, 1, 3) for x in xs]
    return P.compare_zero(c, F, three, ys, three, three, three, 1, 4, mode=mode)


# every protocol function that multiplies, as call(protocols, ctx, F, xs, ys) on sharings of 12 values; t = 1, l = 10
MULTIPLYING = {
    'multiply': lambda P, c, F, xs, ys: P.multiply(c, F, xs, ys, 1),
    'multiply_pending': lambda P, c, F, xs, ys: P.multiply_pending(c, F, xs, ys, 1),
    'multiply_pending_square': lambda P, c, F, xs, ys: P.multiply_pending(c, F, P.Pending.of(xs), P.Pending.of(xs), 1),
    'reshare': lambda P, c, F, xs, ys: P.reshare(c, F, xs, 1, len(xs)),
    'pow254': lambda P, c, F, xs, ys: P.pow254(c, F, xs, 1),
    'pow254_fused': lambda P, c, F, xs, ys: P.pow254_fused(c, F, xs, 1),
    'matmul': lambda P, c, F, xs, ys: P.matmul(c, F, xs, ys, 3, 4, 3, 1),
    'prod_rows': lambda P, c, F, xs, ys: P.prod_rows(c, F, xs, 4, 1),
    'is_zero_public': lambda P, c, F, xs, ys: P.is_zero_public(c, F, xs, ys, 1),
    'compare_zero_lt': lambda P, c, F, xs, ys: _compare_zero(P, c, F, xs, ys, 'lt'),
    'compare_zero_eq': lambda P, c, F, xs, ys: _compare_zero(P, c, F, xs, ys, 'eq'),
    'sort': lambda P, c, F, xs, ys: P.sort(c, F, xs, 1, 12, 1, 1, 10, _no_draw),
    'carry_prefix': lambda P, c, F, xs, ys: P.carry_prefix(c, F, xs, ys, 4, 3, 1),
    'carry_prefix_P_short': lambda P, c, F, xs, ys: P.carry_prefix(c, F, xs + xs[:1], ys, 4, 3, 1),
    'to_bits': lambda P, c, F, xs, ys: P.to_bits(c, F, [P._rows(c, x, 0, 1, 3) for x in xs], ys, [P._rows(c, x, 0, 1, 3) for x in xs], 1, 4),
    'amax': lambda P, c, F, xs, ys: P.amax(c, F, xs, 1, 12, 1, 1, 10, _no_draw),
    'amin': lambda P, c, F, xs, ys: P.amin(c, F, xs, 2, 3, 2, 1, 10, _no_draw),
    'argmax': lambda P, c, F, xs, ys: P.argmax(c, F, xs, 1, 12, 1, 1, 10, _no_draw),
    'argmin': lambda P, c, F, xs, ys: P.argmin(c, F, xs, 2, 3, 2, 1, 10, _no_draw),
    'maximum': lambda P, c, F, xs, ys: P.maximum(c, F, xs, ys, 1, 10, _no_draw),
    'minimum': lambda P, c, F, xs, ys: P.minimum(c, F, xs, ys, 1, 10, _no_draw),
    'minimum_y_short': lambda P, c, F, xs, ys: P.minimum(c, F, xs + xs[:1], ys, 1, 10, _no_draw),
    'find': lambda P, c, F, xs, ys: P.find(c, F, xs, 1, 12, 1, 1),
    'find_integers': lambda P, c, F, xs, ys: P.find(c, F, xs, 1, 12, 1, 1, s=5, bits=False, l=10, rand=_no_draw),
    'fxp_multiply': lambda P, c, F, xs, ys: P.fxp_multiply(c, F, xs, ys, 1, 4, 8, _no_draw),
    'norm': lambda P, c, F, xs, ys: P.norm(c, F, xs, 1, 8, 4, _no_draw),
    'reciprocal': lambda P, c, F, xs, ys: P.reciprocal(c, F, xs, 1, 8, 4, _no_draw, _no_draw),
    'divide': lambda P, c, F, xs, ys: P.divide(c, F, xs, ys, 1, 8, 4, _no_draw, _no_draw),
    'sbox_layer_all': lambda P, c, F, xs, ys: P.sbox_layer_all(c, F, xs, [P._cat(c, [y] * 8) for y in ys], 1, [[0] * 8] * 8, [0] * 8, fused=False),
}


@pytest.mark.parametrize('name', sorted(MULTIPLYING))
def test_every_multiplying_protocol_refuses_2t_parties(name):
    """m = 2t: the first 2t+1 parties re-share a product, so two parties at t = 1 are refused -- before any randomness is
    drawn"""
    from fxp_cpuctx import FxpCpuFieldContext
    from mpyc_amd import protocols
    ctx = FxpCpuFieldContext(P61)
    run = Run(ctx, 3, 1, seed=2)
    xs, ys = run.share(range(12)), run.share(range(1, 13))
    with pytest.raises(ValueError):
        MULTIPLYING[name](protocols, ctx, run.F, xs[:2], ys[:2])


# every function that takes (outer, k, inner), as call(protocols, ctx, F, xs, outer, k, inner); t = 1, l = 10
ALONG_AN_AXIS = {
    'sort': lambda P, c, F, xs, o, k, i: P.sort(c, F, xs, o, k, i, 1, 10, _no_draw),
    'amax': lambda P, c, F, xs, o, k, i: P.amax(c, F, xs, o, k, i, 1, 10, _no_draw),
    'amin': lambda P, c, F, xs, o, k, i: P.amin(c, F, xs, o, k, i, 1, 10, _no_draw),
    'argmax': lambda P, c, F, xs, o, k, i: P.argmax(c, F, xs, o, k, i, 1, 10, _no_draw),
    'argmin': lambda P, c, F, xs, o, k, i: P.argmin(c, F, xs, o, k, i, 1, 10, _no_draw),
    'arg_index': lambda P, c, F, xs, o, k, i: P.arg_index(c, xs, o, k, i),
    'find': lambda P, c, F, xs, o, k, i: P.find(c, F, xs, o, k, i, 1),
    'find_integers': lambda P, c, F, xs, o, k, i: P.find(c, F, xs, o, k, i, 1, s=5, bits=False, l=10, rand=_no_draw),
}


@pytest.mark.parametrize('name', sorted(ALONG_AN_AXIS))
def test_every_protocol_along_an_axis_refuses_a_share_of_the_wrong_length(name):
    """the LAST party's share one element short or long, every share of another length than outer * k * inner, and an extent
    below 1"""
    from fxp_cpuctx import FxpCpuFieldContext
    from mpyc_amd import protocols
    ctx = FxpCpuFieldContext(P61)
    run = Run(ctx, 3, 1, seed=3)
    xs = run.share(range(12))
    call = lambda shares, *shape: ALONG_AN_AXIS[name](protocols, ctx, run.F, shares, *shape)
    for last in (run.share(range(11))[2], run.share(range(13))[2]):
        with pytest.raises(ValueError):
            call(xs[:2] + [last], 2, 3, 2)
    for shape in ((1, 13, 1), (2, 3, 3), (1, 11, 1), (0, 12, 1), (12, 0, 1), (1, 12, 0)):
        with pytest.raises(ValueError):
            call(xs, *shape)


# ---- fxp_multiply, reciprocal, divide ----------------------------------------------------------------------------------------
def within(y, lo, hi):
    """the tolerance of the issue: [min, max] of the reference's eight draws, widened on each side by its own width and by at
    least one unit"""
    w = max(hi - lo, 1)
    return lo - w <= y <= hi + w, max(lo - y, y - hi, 0)


@pytest.mark.parametrize('m,t', CASES)
def test_fxp_multiply_matches_the_integer_model(m, t):
    from fxp_cpuctx import FxpCpuFieldContext
    from mpyc_amd import protocols
    for l, f in ((16, 8), (32, 16)):
        ctx = FxpCpuFieldContext(modulus_for(l))
        run = Run(ctx, m, t, seed=l + m)
        lim = 1 << ((l + f - 2) // 2)
        xs = [0, 1, -1, 1 << f, -(1 << f), lim - 1, -(lim - 1)] + [run.rng.randint(-lim, lim) for _ in range(25)]
        ys = [run.rng.randint(-lim, lim) for _ in xs]
        got = run.open(protocols.fxp_multiply(ctx, run.F, run.share(xs), run.share(ys), t, f, l, run.rand_trunc))
        want = Model(run.truncs, l, f).mul(xs, ys)
        assert got == want and all(y in (x * z >> f, (x * z >> f) + 1) for x, z, y in zip(xs, ys, got))


_CHAINS = {}


def chains(m, t, i):
    """reciprocal(den) and divide(num, den) of golden case i on the stand-in, once per (m, t, i): the opened values and the
    truncation randomness each run drew"""
    if (m, t, i) not in _CHAINS:
        from fxp_cpuctx import FxpCpuFieldContext
        from mpyc_amd import protocols
        case = golden()[i]
        l, f, den, num = case['l'], case['f'], case['den'], case['num']
        ctx = FxpCpuFieldContext(modulus_for(l))
        run = Run(ctx, m, t, seed=500 + i)
        rec = run.open(protocols.reciprocal(ctx, run.F, run.share(den), t, l, f, run.rand_bits, run.rand_trunc))
        run2 = Run(ctx, m, t, seed=600 + i)
        div = run2.open(protocols.divide(ctx, run2.F, run2.share(num), run2.share(den), t, l, f, run2.rand_bits, run2.rand_trunc))
        assert len(run.decomps) == 1 == len(run2.decomps)
        _CHAINS[(m, t, i)] = (rec, run.truncs, div, run2.truncs)
    return _CHAINS[(m, t, i)]


def nearest_chains(m, t, i):
    """chains() with ONE particular draw of the rounding bits, r = 2^(f-1) in every truncation (the high masks stay random: they
    do not reach the result).  np_trunc returns floor(a / 2^f) + 1 with probability (a mod 2^f) / 2^f, and for this draw
    floor((a + 2^(f-1)) / 2^f), the nearer of the two: of every truncation of the chain the likelier outcome"""
    key = (m, t, i, 'nearest')
    if key not in _CHAINS:
        from fxp_cpuctx import FxpCpuFieldContext
        from mpyc_amd import protocols
        case = golden()[i]
        l, f, den, num = case['l'], case['f'], case['den'], case['num']
        ctx = FxpCpuFieldContext(modulus_for(l))
        run = Run(ctx, m, t, seed=700 + i, nearest=True)
        rec = run.open(protocols.reciprocal(ctx, run.F, run.share(den), t, l, f, run.rand_bits, run.rand_trunc))
        run2 = Run(ctx, m, t, seed=800 + i, nearest=True)
        div = run2.open(protocols.divide(ctx, run2.F, run2.share(num), run2.share(den), t, l, f, run2.rand_bits, run2.rand_trunc))
        assert all(r == [1 << (f - 1)] * len(den) for _, r, _ in run.truncs + run2.truncs)
        assert rec == Model(run.truncs, l, f).reciprocal(den) and div == Model(run2.truncs, l, f).divide(num, den)
        _CHAINS[key] = (rec, div)
    return _CHAINS[key]


def chain_cases(m):
    """(m = 7 runs the 16-bit case only: the protocol is the same, the shares cost more)"""
    return [i for i, c in enumerate(golden()) if m == 3 or c['l'] == 16]


@pytest.mark.parametrize('m,t', CASES)
def test_reciprocal_and_divide_match_the_integer_model(m, t):
    """bit for bit against the model of the whole chain with the same randomness"""
    for i in chain_cases(m):
        case = golden()[i]
        l, f = case['l'], case['f']
        rec, truncs, div, truncs2 = chains(m, t, i)
        theta = int(math.ceil(math.log2((f + 1) / 3.54)))
        assert len(truncs) == 2 + 2 * theta and len(truncs2) == 3 + 2 * theta
        assert rec == Model(truncs, l, f).reciprocal(case['den'])
        assert div == Model(truncs2, l, f).divide(case['num'], case['den'])


def test_the_nearest_draw_is_the_likelier_outcome_of_a_truncation():
    for f, L in ((8, 24), (16, 48)):
        for a in (0, 1, -1, (1 << (f - 1)) - 1, 1 << (f - 1), (1 << (f - 1)) + 1, -(1 << (f - 1)), 12345, -12345, (3 << f) - 1):
            frac = a % (1 << f)
            likelier = (a >> f) + (1 if 2 * frac >= (1 << f) else 0)         # floor + 1 has probability frac / 2^f
            assert trunc_model(a, 1 << (f - 1), 977, f, L) == likelier == (a + (1 << (f - 1))) >> f


@pytest.mark.parametrize('m,t', CASES)
def test_reciprocal_and_divide_lie_within_the_reference_interval(m, t):
    """Every result within the recorded [min, max] of the reference's eight draws for that element, widened on each side by
    the interval's own width and by at least one unit.

    The protocol's run and a run of the reference are two draws of the same rounding bits, and the fixture holds eight of
    the reference's.  Which draw the protocol gets here is fixed by reasoning, not by a seed: r = 2^(f-1) in every
    truncation, which rounds to nearest and so takes the likelier of the two outcomes of every truncation of the chain
    (nearest_chains()).  A uniformly random draw is the wrong thing to hold against eight samples: the last Newton iterate c
    takes one of two neighbouring values and c v with v = 2^k >> 2^f spreads them 2^(k-f) units apart, and where one of the
    two is rare the reference's eight draws record only the common one.  With the random draws of chains() 3 of the 720
    results lie outside this tolerance ((32, 16) div element 77 by 4178 units, (24, 12) rec element 19 by 256, and for
    m = 7 (16, 8) div element 51 by 64) although the integer model is exact on those very runs; for that element 77
    (den = 6, num = 33426, recorded [365099663, 365099664]) 300 further draws of the reference's own np_divide span
    [365095485, 365108020], and 300 draws of the model span the same.  A protocol difference -- another constant, a Newton step
    more or less, another bit length in a truncation -- moves the likelier outcome as it moves every other."""
    report, bad = {}, {}
    for i in chain_cases(m):
        case = golden()[i]
        rec, div = nearest_chains(m, t, i)
        for key, got in (('rec', rec), ('div', div)):
            res = [within(y, lo, hi) for y, lo, hi in zip(got, case[key + '_min'], case[key + '_max'])]
            report[(case['l'], case['f'], key)] = (sum(not ok for ok, _ in res), max(d for _, d in res))
            if not all(ok for ok, _ in res):
                bad[(case['l'], case['f'], key)] = [h for h, (ok, _) in enumerate(res) if not ok]
    print('(elements outside the tolerance, largest distance from the recorded [min, max]):', report)
    assert not bad, bad


@pytest.mark.parametrize('wrong', ['one Newton step less', 'another constant', 'the normalisation one bit short'])
def test_the_reference_interval_catches_a_different_protocol(wrong):
    """the same check on the integer model with one thing changed must find elements outside"""
    bad = 0
    for case in golden():
        l, f, den = case['l'], case['f'], case['den']
        theta = int(math.ceil(math.log2((f + 1) / 3.54)))
        mdl = Model([(f, [1 << (f - 1)] * len(den), [0] * len(den))] * (2 + 2 * theta), l, f)
        v = [norm_model(x, l, f) >> (1 if wrong == 'the normalisation one bit short' else 0) for x in den]
        b = mdl.mul(den, v)
        c = [round((2.9142135623731 if wrong != 'another constant' else 2.5) * 2**f) - 2 * x for x in b]
        for _ in range(theta - (1 if wrong == 'one Newton step less' else 0)):
            c = mdl.mul(c, [(1 << (f + 1)) - x for x in mdl.mul(c, b)])
        rec = mdl.mul(c, v)
        bad += sum(not within(y, lo, hi)[0] for y, lo, hi in zip(rec, case['rec_min'], case['rec_max']))
    assert bad > 0


# ---- the deliberately wrong stand-ins ------------------------------------------------------------------------------------------
def test_a_mask_that_weighs_most_significant_first_is_caught():
    from fxp_cpuctx import FxpCpuFieldContext
    ctx = FxpCpuFieldContext(P127)
    ctx.mask_msb_first = True
    assert check_trunc(ctx, 3, 1, 8, 32, seed=7) != []
    ctx = FxpCpuFieldContext(P127)
    assert check_trunc(ctx, 3, 1, 8, 32, seed=7) == []


def test_a_finish_without_mod_is_caught():
    from fxp_cpuctx import FxpCpuFieldContext
    ctx = FxpCpuFieldContext(P127)
    ctx.finish_no_mod = True
    assert len(check_trunc(ctx, 3, 1, 8, 32, seed=8)) > 30


def test_a_norm_prod_without_the_reversal_is_caught():
    from fxp_cpuctx import FxpCpuFieldContext
    ctx = FxpCpuFieldContext(P61)
    ctx.prod_no_reversal = True
    vals = norm_inputs(random.Random(3), 16)
    got = check_norm(ctx, 3, 1, 16, 8, vals, seed=9)
    assert got != [norm_model(a, 16, 8) for a in vals]
    assert got[1] == norm_model(-1, 16, 8)              # (all bits alike: the order does not show)


def test_a_norm_apply_that_adds_the_sign_bit_is_caught():
    from fxp_cpuctx import FxpCpuFieldContext
    ctx = FxpCpuFieldContext(P61)
    ctx.apply_adds_top = True
    vals = norm_inputs(random.Random(4), 16)
    assert check_norm(ctx, 3, 1, 16, 8, vals, seed=10) != [norm_model(a, 16, 8) for a in vals]


def test_the_stand_in_refuses_what_the_engine_refuses():
    from fxp_cpuctx import FxpCpuFieldContext
    ctx = FxpCpuFieldContext(P61)
    run = Run(ctx, 3, 1, seed=2)
    a, bits = run.share([1, 2, 3])[0], run.share([0, 1] * 24)[0]
    for bad in (lambda: ctx.trunc_mask(a, bits, a, 0, 0), lambda: ctx.trunc_mask(a, bits, a, 60, 0), lambda: ctx.trunc_mask(a, bits, a, 8, 0),
                lambda: ctx.trunc_finish([], [], a, 8), lambda: ctx.trunc_finish([bits], [1], a, 8),
                lambda: ctx.norm_prod(bits, 1), lambda: ctx.norm_prod(bits, 5), lambda: ctx.norm_apply(bits, [a], [1], 16)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        ctx.trunc_finish([a] * 10, [1] * 10, a, 8)
    out, sign = ctx.norm_prod(bits, 16, want_sign=False)
    assert sign is None and out.n == 45
    assert FxpCpuFieldContext(0x11b, binary=True).binary
    with pytest.raises(NotImplementedError):
        gf = FxpCpuFieldContext(0x11b, binary=True)
        gf.norm_prod(gf.from_ints([0, 1]), 2)
