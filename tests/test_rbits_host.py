"""CPU checks of secure random bits and of the supplier of the protocols' randomness: the two C ABI entries of
include/ffgpu_math.h exist in header, library and binding; the launch plans (mpyc_amd/csrc/rbits_geom.hpp) walked by
tests/rbits_check.cpp with g++ against brute-force enumeration; protocols.random_bits composed over a Python-integer context
(tests/rbits_cpuctx.py) on the draws the reference was fed (tests/golden/rbits/rbits.json) -- at one party element for element
the reference's opened squares and bits, at (m, t) = (3, 1) and (5, 2) opening to them from the first and from the last t+1
parties --; protocols.Randomness: every sharing opens to one value from two party sets, bits are bits, zeros are zeros of
degree 2t, bounded elements stay below their bound, no common input is used twice, 4096 bits of a fixed key are balanced, and
compare_zero, fxp_multiply and is_zero run end to end on nothing but its draws; and they do not with an opening that counts no
zeros, kept entries in the wrong order, the 1 added after the halving, z left out or a bound that is not rounded.  No GPU
needed."""
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
GOLDEN = os.path.join(TESTS, 'golden', 'rbits', 'rbits.json')
ENTRIES = (('ffgm_rbits_open', 9), ('ffgm_rbits_finish', 9))
P61, P80, P127 = 2**61 - 1, 2**80 - 65, 2**127 - 1
PARTIES = [(1, 0), (3, 1), (5, 2)]
CASES = ('none', 'first_last', 'adjacent', 'all_first', 'second_again')
# The key of the balance check: with it Randomness(m = 3, t = 1).bits(4096) over 2^61 - 1 has BALANCE_ONES ones, which is
# within 3 sqrt(4096) = 192 of 2048 (six standard deviations); found on the stand-in, used unchanged on the device
# (tests/test_gpu_rbits.py), where the PRF is the same.
BALANCE_KEY = b'mpyc_amd rbits balance check 00'
BALANCE_ONES = 2066


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_rbits_entries_in_header_library_and_binding():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu_math.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    for name, nparams in ENTRIES:
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, f'{name} is not declared in include/ffgpu_math.h'
        assert len([p.strip() for p in m.group(1).split(',')]) == nparams
        assert re.search(r' T ' + name + r'\b', out), f'{name} is not exported by libffgpu.so'
        assert name in _ffi.EXPORTED_MATH and name not in _ffi.EXPORTED and len(_ffi._SIGS_MATH[name]) == nparams
    assert set(re.findall(r'\b(ffgm_\w+)\s*\(', hdr)) == set(_ffi.EXPORTED_MATH) == set(re.findall(r' T (ffgm_\w+)', out))
    L_ = _ffi.lib()
    # no context: refused before anything is touched
    assert L_.ffgm_rbits_open(None, None, None, None, 3, None, None, 4, None) == _ffi.EINVAL
    assert L_.ffgm_rbits_finish(None, None, None, None, 3, 0, 0, 4, None) == _ffi.EINVAL


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_rbits_geometry_on_the_host(tmp_path):
    """every entry of a row is covered once by the packs and the tail of both plans, at every edge of the launch plan, for five
    element sizes, both alignments and row counts on both sides of the fused limit"""
    exe = str(tmp_path / 'rbits_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'rbits_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'rbits ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) > 1500


def test_the_fixture_is_what_the_issue_asks_for():
    doc = golden()
    assert [(e['name'], e['p'] % 4) for e in doc['fields']] == [('pm64-mersenne', 3), ('pm64-k64', 3), ('pm96', 3), ('pm64-gen', 1)]
    assert [e['p'] for e in doc['fields']] == [P61, 2**64 - 189, P80, 2**40 - 87] and doc['count'] == 12
    for e in doc['fields']:
        p = e['p']
        assert tuple(c['case'] for c in e['cases']) == CASES
        for c in e['cases']:
            assert [(b['signed'], b['f']) for b in c['bits']] == [(False, 0), (False, 16), (True, 0), (True, 16)]
            opened = [[(r * r + z) % p for r, z in zip(rd['r'], rd['z'])] for rd in c['rounds']]
            assert opened == c['opened']
            zeros = [[i for i, v in enumerate(o) if v == 0] for o in opened]
            assert [len(o) for o in opened] == [12] + [len(z) for z in zeros[:-1]] and zeros[-1] == []
            want = {'none': [[]], 'first_last': [[0, 11], []], 'adjacent': [[4, 5], []], 'all_first': [list(range(12)), []],
                    'second_again': [[2, 7, 9], [1], []]}[c['case']]
            assert zeros == want


# ---- the protocol on the recorded draws ------------------------------------------------------------------------------------------
class GoldenDraw:
    """draw(h) of protocols.random_bits from the recorded rounds: r shared at degree t, z at degree 2t (its recorded value is 0
    except where it plants a zero square), the polynomials from a seeded generator"""

    def __init__(self, ctx, rounds, m, t, seed):
        self.ctx, self.rounds, self.m, self.t, self.rng, self.at = ctx, rounds, m, t, random.Random(seed), 0
        self.handed = []

    def __call__(self, h):
        rd = self.rounds[self.at]
        self.at += 1
        assert len(rd['r']) == h, 'the redraw has as many entries as the last draw had zero squares'
        r, z = _share(self.ctx, self.rng, rd['r'], self.t, self.m), _share(self.ctx, self.rng, rd['z'], 2 * self.t, self.m)
        self.handed.append(([x.to_ints() for x in r], [x.to_ints() for x in z], r, z))
        return r, z


def open_two_ways(ctx, shares, degree):
    """the value from the first and from the last degree+1 parties: both must agree"""
    p, m, res = ctx.modulus, len(shares), []
    for pick in (list(range(degree + 1)), list(range(m - degree - 1, m))):
        lam = _lagrange(p, [i + 1 for i in pick])
        res.append(ctx.recombine([shares[i] for i in pick], lam).to_ints())
    assert res[0] == res[1], 'the sharing has a higher degree'
    return res[0]


def run_golden(ctx, protocols, field, e, c, m, t, seed=1):
    """random_bits on the draws of one recorded case, every (signed, f): the opened squares of every round and the bits"""
    count = len(c['rounds'][0]['r'])
    for b in c['bits']:
        draw = GoldenDraw(ctx, c['rounds'], m, t, seed)
        opened, real = [], ctx.rbits_open

        def recording(rs, zs, lambdas, zeros=None, out=None):
            assert len(rs) == len(zs) == 2 * t + 1, 'the opening takes the first 2t+1 parties'
            res = real(rs, zs, lambdas, zeros=zeros, out=out)
            opened.append(res.to_ints())
            return res

        ctx.rbits_open = recording
        try:
            got = protocols.random_bits(ctx, field, count, t, draw, signed=b['signed'], f=b['f'])
        finally:
            del ctx.rbits_open
        assert draw.at == len(c['rounds']) and opened == c['opened'], 'the opened squares differ from the recording'
        assert len(got) == m and all(g.n == count for g in got)
        assert open_two_ways(ctx, got, t) == b['values'], (e['name'], c['case'], b['signed'], b['f'], m, t)
        for r0, z0, r, z in draw.handed:                                 # what draw() returned is not written
            assert [x.to_ints() for x in r] == r0 and [x.to_ints() for x in z] == z0, 'an input of random_bits was written'


def gf(p):
    import mpyc_amd.finfields as gff
    return gff.GF(p)


@pytest.mark.parametrize('m,t', PARTIES)
def test_random_bits_is_the_reference_on_the_same_draws(m, t):
    """m = 1: a share is the value, so this is element for element the reference's run; m = 3, 5: the same values opened from
    the first and from the last t+1 parties, the squares opened from the first 2t+1"""
    from mpyc_amd import protocols
    from rbits_cpuctx import RbitsCpuFieldContext
    for e in golden()['fields']:
        ctx = RbitsCpuFieldContext(e['p'])
        for c in e['cases']:
            run_golden(ctx, protocols, gf(e['p']), e, c, m, t, seed=100 * m + t)


def test_random_bits_edges():
    from mpyc_amd import protocols
    from rbits_cpuctx import RbitsCpuFieldContext
    ctx = RbitsCpuFieldContext(P61)
    F = gf(P61)
    rng = random.Random(5)
    calls = []

    def draw(h):
        calls.append(h)
        return _share(ctx, rng, [rng.randrange(1, P61) for _ in range(h)], 1, 3), _share(ctx, rng, [0] * h, 2, 3)

    got = protocols.random_bits(ctx, F, 0, 1, draw)
    assert len(got) == 3 and all(g.n == 0 for g in got) and calls == [0], 'count == 0: empty rows for every party'
    bits = open_two_ways(ctx, protocols.random_bits(ctx, F, 33, 1, draw, signed=True), 1)
    assert set(bits) <= {1, P61 - 1} and len(bits) == 33 and calls == [0, 33]
    with pytest.raises(ValueError):
        protocols.random_bits(ctx, F, 4, 1, lambda h: (draw(h)[0][:2], draw(h)[1][:2]))        # fewer than 2t+1 parties
    with pytest.raises(ValueError):
        protocols.random_bits(ctx, F, 4, 1, lambda h: (draw(h)[0], draw(h - 1)[1]))            # a short sharing
    with pytest.raises(ValueError):
        protocols.random_bits(ctx, F, -1, 1, draw)
    from iszero_cpuctx import IszeroCpuFieldContext
    with pytest.raises(ValueError):
        protocols.random_bits(IszeroCpuFieldContext(0x11b, True), None, 4, 1, draw)
    # the stand-in refuses what the engine refuses
    a = ctx.from_ints([1, 2])
    for call in (lambda: ctx.rbits_open([a], [a, a], [1]), lambda: ctx.rbits_open([a], [a], [1, 1]), lambda: ctx.rbits_open([], [], []),
                 lambda: ctx.rbits_open([a], [ctx.from_ints([1])], [1]), lambda: ctx.rbits_open([a] * 65, [a] * 65, [1] * 65),
                 lambda: ctx.rbits_finish(a, []), lambda: ctx.rbits_finish(a, [a], f=192), lambda: ctx.rbits_finish(a, [a], outs=[a, a]),
                 lambda: ctx.rbits_finish(a, [ctx.from_ints([1])])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError):
        RbitsCpuFieldContext(2**40 - 87).rbits_finish(a, [a])
    cnt = ctx.zero_counter()
    c = ctx.rbits_open([ctx.from_ints([0, 3, 5])], [ctx.from_ints([0, P61 - 9, 1])], [1], zeros=cnt)
    c = ctx.rbits_open([ctx.from_ints([0, 3, 5])], [ctx.from_ints([0, P61 - 9, 1])], [2], zeros=cnt, out=c)
    assert c.to_ints() == [0, 0, 52] and int(cnt.item()) == 4, 'the counter is added to'
    assert [x.to_ints() for x in ctx.rbits_finish(ctx.from_ints([0, 4, 4]), [ctx.from_ints([7, 2, P61 - 2])], signed=True, f=3)] == \
        [[0, 8, P61 - 8]]
    assert [x.to_ints() for x in ctx.rbits_finish(ctx.from_ints([0, 4, 4]), [ctx.from_ints([7, 2, P61 - 2])])] == [[0, 1, 0]]


# ---- the supplier ---------------------------------------------------------------------------------------------------------------
def supplier(p, m, t, key=b'k' * 16, ctx=None, **kw):
    from mpyc_amd import protocols
    from rbits_cpuctx import RbitsCpuFieldContext
    ctx = RbitsCpuFieldContext(p) if ctx is None else ctx
    return ctx, protocols.Randomness(ctx, gf(p), t, m, key, **kw)


def rounded(bound, m, t):
    """runtime.py:4074-4075"""
    return 1 << max(0, (bound // math.comb(m, t)).bit_length() - 1)


def check_supplier(ctx, R, count=40):
    """the model checks on one supplier; returns the common inputs it used"""
    p, m, t = ctx.modulus, R.m, R.t
    used, real = [], R._uci

    def recording():
        used.append(real())
        return used[-1]

    R._uci = recording
    el = open_two_ways(ctx, R.elements(count), t)
    assert len(el) == count and len(set(el)) > count // 2 and all(0 <= v < p for v in el)
    assert el != open_two_ways(ctx, R.elements(count), t), 'two calls, two common inputs'
    zs = R.zeros(count)
    assert open_two_ways(ctx, zs, 2 * t) == [0] * count, 'zeros: a sharing of zero of degree 2t'
    if t:
        assert any(x.to_ints() != [0] * count for x in zs), 'zeros: a RANDOM sharing of zero'
        with pytest.raises(AssertionError):
            open_two_ways(ctx, zs, t)                                    # ... and not one of degree t
    for bound in (1 << 30, 1 << 7, 1000, 3, 1):
        v = open_two_ways(ctx, R.elements(count, bound), t)
        rb = rounded(bound, m, t)
        assert all(0 <= x < rb * math.comb(m, t) <= bound or (x == 0 and rb == 1) for x in v), ('elements(bound)', bound, max(v))
        assert R.rounded_bound(bound) == rb
        if rb > 4:
            assert max(v) >= rb // 2 or count < 8, 'the draws use their range'
    for signed, f in ((False, 0), (True, 0), (False, 16), (True, 5)):
        unit = (1 << f) % p
        b = open_two_ways(ctx, R.bits(count, signed=signed, f=f), t)
        assert len(b) == count and set(b) == ({unit, p - unit} if signed else {0, unit}), ('bits', signed, f)
    rb, rdivl = R.rand_bits(5, 7)
    assert set(open_two_ways(ctx, rb, t)) <= {0, 1} and rb[0].n == 35 and all(v < 1 << R.sec_param for v in open_two_ways(ctx, rdivl, t))
    rb, rdivf = R.rand_trunc(5, 4, l=8)
    assert set(open_two_ways(ctx, rb, t)) <= {0, 1} and rb[0].n == 20
    assert all(v < 1 << (R.sec_param + 8 - 4) for v in open_two_ways(ctx, rdivf, t)) and rdivf[0].n == 5
    z, r, s = R.rand_zero(6)
    assert set(open_two_ways(ctx, z, t)) <= {0, 1} and all(len(open_two_ways(ctx, x, t)) == 6 for x in (r, s))
    rbits, sbits, rdivl, rzero = R.rand_compare(9)(4)
    assert (rbits[0].n, sbits[0].n, rdivl[0].n, rzero[0].n) == (36, 4, 4, 4)
    assert set(open_two_ways(ctx, rbits, t) + open_two_ways(ctx, sbits, t)) <= {0, 1}
    ex = R.rand_exp(9, 1 << 12)
    assert len(ex) == t + 1 and all(x.n == 9 and max(x.to_ints()) < 1 << 12 for x in ex) and len({tuple(x.to_ints()) for x in ex}) == t + 1
    assert R.rand_exp(3, 1)[0].to_ints() == [0, 0, 0]
    assert len(used) == len(set(used)) == R.counter, 'a common input was used twice'
    del R._uci
    return used


@pytest.mark.parametrize('p', [P61, P80, 2**40 - 87])
@pytest.mark.parametrize('m,t', [(3, 1), (4, 1), (6, 2)])
def test_randomness_model(p, m, t):
    ctx, R = supplier(p, m, t)
    used = check_supplier(ctx, R)
    # the same key: the same values; another key, or more rounds: other values
    a = [x.to_ints() for x in supplier(p, m, t)[1].elements(8)]
    assert a == [x.to_ints() for x in supplier(p, m, t)[1].elements(8)]
    assert a != [x.to_ints() for x in supplier(p, m, t, key=b'K' * 16)[1].elements(8)]
    assert a != [x.to_ints() for x in supplier(p, m, t, rounds=12)[1].elements(8)]
    assert len(used) > 20


def test_randomness_refusals():
    from mpyc_amd import protocols
    from iszero_cpuctx import IszeroCpuFieldContext
    ctx, R = supplier(P61, 3, 1)
    with pytest.raises(ValueError):
        protocols.Randomness(ctx, gf(P61), 1, 2, b'k')                   # fewer than 2t+1 parties
    with pytest.raises(ValueError):
        protocols.Randomness(IszeroCpuFieldContext(0x11b, True), None, 1, 3, b'k')
    with pytest.raises(ValueError):
        R.rand_exp(4, 1000)
    with pytest.raises(ValueError):
        R.rand_trunc(4, 40, l=30)
    assert [x.n for x in R.bits(0)] == [0, 0, 0] and [x.n for x in R.elements(0, 8)] == [0, 0, 0]
    ctx0, R0 = supplier(P61, 1, 0)                                        # one party: a share is the value
    assert R0.zeros(3)[0].to_ints() == [0, 0, 0] and set(R0.bits(20)[0].to_ints()) == {0, 1}


def test_bits_of_a_fixed_key_are_balanced():
    """4096 bits: the number of ones within 3 sqrt(4096) = 192 of 2048 (six standard deviations); the key is recorded above"""
    ctx, R = supplier(P61, 3, 1, key=BALANCE_KEY)
    ones = sum(open_two_ways(ctx, R.bits(4096), 1))
    print('ones among 4096 bits:', ones)
    assert abs(ones - 2048) <= 192
    assert ones == BALANCE_ONES


# ---- end to end: nothing but the supplier's draws --------------------------------------------------------------------------------
VALUES = [0, 1, -1, 2, -2, 255, -256, 12345, -12345, (1 << 15) - 1, -(1 << 15), 77]


def run_end_to_end(ctx, protocols, which, m=3, t=1, key=b'end to end key 01', n=None):
    """one of compare_zero('lt'), fxp_multiply, is_zero on a dozen values (repeated to n entries) with Randomness as the only
    source of randomness; returns (opened result, expected)"""
    vals = VALUES if n is None else [VALUES[i % len(VALUES)] for i in range(n)]
    p = ctx.modulus
    F = gf(p)
    R = protocols.Randomness(ctx, F, t, m, key)
    rng = random.Random(7)
    xs = _share(ctx, rng, vals, t, m)
    if which == 'lt':
        l = 17
        rbits, sbits, rdivl, rzero = R.rand_compare(l)(len(vals))
        got = protocols.compare_zero(ctx, F, xs, rbits, sbits, rdivl, rzero, t, l, mode='lt')
        return open_two_ways(ctx, got, t), [int(v < 0) for v in vals]
    if which == 'fxp':                                                    # |x|, |y| <= 2^12: |x y| < 2^(l+f-1), l + f = 26 <= 29, the
        f, l = 8, 18                                                      # bit length rand_trunc assumes over 2^61 - 1
        small = [v >> 3 for v in vals]
        xs, ys = _share(ctx, rng, small, t, m), _share(ctx, rng, small[::-1], t, m)
        got = [_signed(v, p) for v in open_two_ways(ctx, protocols.fxp_multiply(ctx, F, xs, ys, t, f, l, R.rand_trunc), t)]
        return got, [x * y for x, y in zip(small, small[::-1])]
    assert which == 'zero'
    got = protocols.is_zero(ctx, F, xs, t, R.sec_param, R.rand_zero)
    return open_two_ways(ctx, got, t), [int(v == 0) for v in vals]


def check_end_to_end(which, got, want):
    if which == 'fxp':                                                    # floor(x y / 2^f) or that plus one
        assert all(w >> 8 <= g <= (w >> 8) + 1 for g, w in zip(got, want)), (got, want)
    else:
        assert got == want, which


def zero_test_prime(protocols, sec_param=30):
    """the field is_zero runs over: the first of the candidates that runtime.np_equal sends down the Legendre route"""
    cands = [(P61, 16), (2**40 - 87, 64), (P127, 64), (P80, 32)]
    picked = [p for p, l in cands if protocols.equal_route(p, l, sec_param) == 'legendre']
    assert picked == [P127]
    return picked[0]


@pytest.mark.parametrize('which', ['lt', 'fxp', 'zero'])
def test_protocols_run_on_the_supplier_alone(which):
    from mpyc_amd import protocols
    from rbits_cpuctx import RbitsCpuFieldContext
    p = zero_test_prime(protocols) if which == 'zero' else P61
    got, want = run_end_to_end(RbitsCpuFieldContext(p), protocols, which)
    check_end_to_end(which, got, want)
    assert len(got) == 12


# ---- wrong variants must fail, driven by the same checks --------------------------------------------------------------------------
class ReversedCat:
    """torch with a cat that puts the last piece first: the kept entries behind the last draw"""

    def __getattr__(self, name):
        import torch
        if name == 'cat':
            return lambda parts, *a, **kw: torch.cat(list(parts)[::-1], *a, **kw)
        return getattr(torch, name)


WRONG = ('no_zero_drop', 'kept_order', 'one_after_half', 'without_z', 'bound_not_rounded')


@pytest.mark.parametrize('wrong', WRONG)
def test_a_wrong_step_is_caught(wrong, monkeypatch):
    from mpyc_amd import protocols
    from rbits_cpuctx import RbitsCpuFieldContext
    e = golden()['fields'][0]
    p = e['p']
    ctx = RbitsCpuFieldContext(p)
    case = {c['case']: c for c in e['cases']}
    if wrong == 'bound_not_rounded':
        _, R = supplier(p, 3, 1, ctx=ctx)
        check_supplier(ctx, R)                                           # the right supplier passes
        monkeypatch.setattr(protocols.Randomness, 'rounded_bound', lambda self, bound: bound)
        _, R = supplier(p, 3, 1, ctx=ctx)
        with pytest.raises(AssertionError):
            check_supplier(ctx, R)
        return
    c = case['second_again']
    run_golden(ctx, protocols, gf(p), e, c, 3, 1)                        # the right steps pass on these very draws
    if wrong == 'no_zero_drop':                                          # the opening counts nothing: no entry is dropped or redrawn
        real = ctx.rbits_open
        ctx_open = lambda rs, zs, lambdas, zeros=None, out=None: real(rs, zs, lambdas, zeros=None, out=out)
        monkeypatch.setattr(ctx, 'rbits_open', ctx_open, raising=False)
        ctx.finish_keeps_zero = True
    elif wrong == 'kept_order':
        monkeypatch.setattr(protocols, '_torch', lambda: ReversedCat())
    elif wrong == 'one_after_half':
        ctx.finish_one_after_half = True
    elif wrong == 'without_z':
        ctx.open_without_z = True
    with pytest.raises(AssertionError):
        if wrong == 'no_zero_drop':
            c = dict(c, rounds=c['rounds'][:1], opened=c['opened'][:1])  # (it never asks for the second draw)
            got = protocols.random_bits(ctx, gf(p), 12, 1, GoldenDraw(ctx, c['rounds'], 3, 1, 1))
            assert open_two_ways(ctx, got, 1) == c['bits'][0]['values']
        else:
            run_golden(ctx, protocols, gf(p), e, c, 3, 1)


# ---- p = 1 mod 4: the bits composed from sqrt_cl, inv, mul and the scalar forms -------------------------------------------------
ONE_MOD_FOUR = [2**80 - 143, 2**136 - 243, 2**127 + 2**100 + 0x101]          # 12-, 24- and 16-byte (Montgomery) storage
COMPOSED = [(m, t, signed, f) for m, t in ((3, 1), (5, 2)) for signed in (False, True) for f in (0, 2)]


def run_one_mod_four(ctx, protocols, m, t, signed, f, count=257, seed=1):
    """random_bits over a prime = 1 mod 4 on draws made here: uniform non-zero r, z a sharing of zero but for three entries
    (the first, the last, one inside), where z = -r^2 makes the opened square 0, so that the entries are compacted and three
    are drawn again.  The opened result is r (r^2)^(-1/2) with the root of oracle.pyoracle.sqrt_prime -- the root the reference
    takes, which decides the sign of every bit -- mapped to a bit and scaled by 2^f."""
    from oracle import pyoracle as po
    p = ctx.modulus
    assert p % 4 == 1
    rng = random.Random(seed)
    planted = [0, count // 3, count - 1]
    r1 = [rng.randrange(1, p) for _ in range(count)]
    z1 = [(-r1[h] * r1[h]) % p if h in planted else 0 for h in range(count)]
    r2 = [rng.randrange(1, p) for _ in planted]
    rounds = [{'r': r1, 'z': z1}, {'r': r2, 'z': [0] * len(r2)}]
    draw = GoldenDraw(ctx, rounds, m, t, seed)
    got = protocols.random_bits(ctx, gf(p), count, t, draw, signed=signed, f=f)
    assert draw.at == 2 and len(got) == m and all(g.n == count for g in got)
    r = [v for h, v in enumerate(r1) if h not in planted] + r2                   # the kept entries, then the last draw whole
    F, want = po.Field(p, False), []
    for v in r:
        b = v * pow(po.sqrt_prime(F, v * v % p), -1, p) % p
        assert b in (1, p - 1)
        want.append(((b if signed else (b + 1) * ((p + 1) >> 1)) << f) % p)
    assert open_two_ways(ctx, got, t) == want, (hex(p), m, t, signed, f)
    assert len({w for w in want}) == 2, 'both bits occur'
    for r0, z0, rs, zs in draw.handed:
        assert [x.to_ints() for x in rs] == r0 and [x.to_ints() for x in zs] == z0, 'an input of random_bits was written'


@pytest.mark.parametrize('m,t,signed,f', COMPOSED)
@pytest.mark.parametrize('p', ONE_MOD_FOUR, ids=hex)
def test_random_bits_over_primes_one_mod_four(p, m, t, signed, f):
    from mpyc_amd import protocols
    from rbits_cpuctx import RbitsCpuFieldContext
    run_one_mod_four(RbitsCpuFieldContext(p), protocols, m, t, signed, f, seed=10 * m + f)
