"""CPU checks of the secure binary sign by Legendre symbols: the two C ABI entries of include/ffgpu_math.h exist in header,
library and binding; the launch plans (mpyc_amd/csrc/bsgn_geom.hpp) walked by tests/bsgn_check.cpp with g++ against
brute-force enumeration; protocols.bsgn_value / bsgn_range against what the reference demo's own bsgn_0 / bsgn_1 / bsgn_2
opened (tests/golden/bsgn/bsgn.json, wrong signs beyond the range included); protocols.bsgn composed over a Python-integer
context (tests/bsgn_cpuctx.py) for (m, t) = (1, 0), (3, 1), (7, 3) and every variant: it opens to the fixture on the fixture's
inputs and to bsgn_value on random field elements over a 31-bit Blum prime; d = 0 share for share against a model on the
replayed draws; planted zeros give 0; every deliberately wrong switch of the stand-in is caught; the refusals; and the
protocol on nothing but protocols.Randomness.  No GPU needed."""
import json
import os
import random
import re
import shutil
import subprocess

import pytest

from test_rbits_host import gf, open_two_ways
from test_sort_host import _share, _signed

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, 'golden', 'bsgn', 'bsgn.json')
ENTRIES = (('ffgm_bsgn_mask', 9), ('ffgm_bsgn_finish', 9))
DEMO_PRIMES = (3546374752298322551, 9409569905028393239, 15569949805843283171)
DEMO_RANGES = (134, 383, 594)
P31 = 2**31 - 1                                                          # a Blum prime: 3 mod 4
PARTIES = [(1, 0), (3, 1), (7, 3)]


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)['bsgn']


def test_bsgn_entries_in_header_library_and_binding():
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
    assert L_.ffgm_bsgn_mask(None, None, None, None, None, 3, None, 4, None) == _ffi.EINVAL
    assert L_.ffgm_bsgn_finish(None, None, None, None, 3, 3, 0, 4, None) == _ffi.EINVAL
    assert L_.ffgpu_abi_version() == 1


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_bsgn_geometry_on_the_host(tmp_path):
    """every (row, element) pair is covered once by the rows plan and by the packs and the tail of the flat plan, for five
    element sizes, both alignments and every row count; the 2-bit codes of a unit keep to their slots"""
    exe = str(tmp_path / 'bsgn_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'bsgn_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'bsgn ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) == 5 * 2 * 10 * 8 * 2


# ---- the function itself against the reference demo ---------------------------------------------------------------------------
def test_the_fixture_is_what_the_issue_asks_for():
    doc = golden()
    assert [e['d'] for e in doc] == [0, 1, 2] and tuple(e['p'] for e in doc) == DEMO_PRIMES and tuple(e['B'] for e in doc) == DEMO_RANGES
    for e in doc:
        B = e['B']
        assert e['p'] % 4 == 3 and e['a'] == list(range(-B - 8, B + 9)) and len(e['bsgn']) == len(e['a'])
        sign = {a: v for a, v in zip(e['a'], e['bsgn'])}
        assert all(sign[a] == (1 if a >= 0 else -1) for a in range(-B, B + 1))
        assert sign[B + 1] != 1 or sign[-B - 1] != -1, 'the sign is first wrong at |a| = B + 1'


def test_bsgn_value_and_range_are_the_reference():
    from mpyc_amd import protocols
    assert [protocols.bsgn_rows(d) for d in range(3)] == [1, 3, 5] and [protocols.bsgn_draws(d) for d in range(3)] == [1, 3, 6]
    for e in golden():
        p, d = e['p'], e['d']
        assert [protocols.bsgn_value(p, d, a) for a in e['a']] == e['bsgn'], d
        assert protocols.bsgn_range(p, d) == e['B']
        assert protocols.bsgn_range(p, d, limit=100) == 100
    # a zero symbol is 0 in its term
    p = DEMO_PRIMES[0]
    assert protocols.bsgn_value(p, 0, (p - 1) // 2) == 0
    assert protocols.bsgn_value(P31, 2, (P31 - 1) // 2) == protocols._legendre(P31, sum(protocols._legendre(P31, v) for v in (-4, -2, 2, 4)))
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            protocols.bsgn_value(p, bad, 1)


# ---- the protocol on the stand-in -------------------------------------------------------------------------------------------------
class Draws:
    """rand_bsgn(count) from a seeded generator: signs and elements shared at degree t; `plant` maps entries of r to values"""

    def __init__(self, ctx, m, t, seed, plant=None):
        self.ctx, self.m, self.t, self.rng, self.plant, self.handed = ctx, m, t, random.Random(seed), plant or {}, []

    def __call__(self, count):
        p = self.ctx.modulus
        s = [self.rng.choice((1, p - 1)) for _ in range(count)]
        r = [self.plant.get(i, self.rng.randrange(1, p)) for i in range(count)]
        ss, rs = _share(self.ctx, self.rng, s, self.t, self.m), _share(self.ctx, self.rng, r, self.t, self.m)
        self.handed.append((s, r, ss, rs, [x.to_ints() for x in ss], [x.to_ints() for x in rs]))
        return ss, rs

    def unwritten(self):
        return all([x.to_ints() for x in ss] == s0 and [x.to_ints() for x in rs] == r0 for _, _, ss, rs, s0, r0 in self.handed)


def run_bsgn(ctx, a, m, t, d, seed=1, plant=None):
    """protocols.bsgn on the values a: (opened result as signed integers, the shares, the draws)"""
    from mpyc_amd import protocols
    p = ctx.modulus
    rng = random.Random(1000 + seed)
    xs = _share(ctx, rng, a, t, m)
    before = [x.to_ints() for x in xs]
    draws = Draws(ctx, m, t, seed, plant)
    got = protocols.bsgn(ctx, gf(p), xs, t, d, draws)
    assert len(got) == m and all(g.n == len(a) for g in got)
    assert [x.to_ints() for x in xs] == before and draws.unwritten(), 'an input of bsgn was written'
    assert len(draws.handed) == 1 and len(draws.handed[0][0]) == protocols.bsgn_draws(d) * len(a)
    return [_signed(v, p) for v in open_two_ways(ctx, got, t)], got, draws


def check_fixture(make_ctx, m, t, ds=(0, 1, 2)):
    for e in golden():
        if e['d'] in ds:
            got, _, _ = run_bsgn(make_ctx(e['p']), e['a'], m, t, e['d'], seed=10 * m + e['d'])
            assert got == e['bsgn'], (e['d'], m, t)


def check_zeros(make_ctx, m=3, t=1):
    """a planted r = 0 gives 0 in its term (the result, for d = 0 and d = 2's last stage); so does 2a + 1 = 0 mod p"""
    from mpyc_amd import protocols
    p = DEMO_PRIMES[0]
    a = [0, 5, -5, (p - 1) // 2, 7, -7]
    got, _, _ = run_bsgn(make_ctx(p), a, m, t, 0, seed=3, plant={1: 0, 5: 0})
    assert got == [1, 0, -1, 0, 1, 0]
    p = DEMO_PRIMES[2]
    n = 4
    got, _, _ = run_bsgn(make_ctx(p), [3, -3, 9, -9], m, t, 2, seed=4, plant={5 * n + 1: 0, 2 * n + 2: 0})
    # entry 1: r5 = 0, the whole result; entry 2: the middle symbol (of 19) drops out of the sum of five
    L = protocols._legendre
    assert got == [1, 0, L(p, sum(L(p, v) for v in (15, 17, 21, 23))), -1]
    assert protocols.bsgn_value(p, 2, 9) == 1


@pytest.mark.parametrize('m,t', PARTIES)
@pytest.mark.parametrize('d', [0, 1, 2])
def test_bsgn_opens_to_the_fixture(m, t, d):
    from bsgn_cpuctx import BsgnCpuFieldContext
    check_fixture(BsgnCpuFieldContext, m, t, ds=(d,))


@pytest.mark.parametrize('m,t', PARTIES)
@pytest.mark.parametrize('d', [0, 1, 2])
def test_bsgn_is_bsgn_value_on_random_elements(m, t, d):
    from mpyc_amd import protocols
    from bsgn_cpuctx import BsgnCpuFieldContext
    rng = random.Random(31 * m + d)
    a = [0, 1, P31 - 1, 2, P31 - 2, (P31 - 1) // 2, (P31 + 1) // 2] + [rng.randrange(P31) for _ in range(90)]
    got, _, _ = run_bsgn(BsgnCpuFieldContext(P31), a, m, t, d, seed=5)
    assert got == [protocols.bsgn_value(P31, d, v) for v in a]
    assert d != 0 or got[5] == 0                                          # (2a + 1 = 0 mod p is among the inputs)


@pytest.mark.parametrize('m,t', PARTIES)
def test_bsgn_0_share_for_share(m, t):
    """the opened value is (2a + 1) s r^2 whatever the re-sharing rounds drew, so party q's share is its share of s times the
    symbol of that value"""
    from mpyc_amd import protocols
    from bsgn_cpuctx import BsgnCpuFieldContext
    p = DEMO_PRIMES[0]
    a = list(range(-140, 141, 7)) + [(p - 1) // 2]
    _, got, draws = run_bsgn(BsgnCpuFieldContext(p), a, m, t, 0, seed=8, plant={2: 0})
    s, r, _, _, s_shares, _ = draws.handed[0]
    h = [protocols._legendre(p, (2 * x + 1) * sv * rv * rv) for x, sv, rv in zip(a, s, r)]
    assert h[2] == 0 and h[-1] == 0 and set(h) == {1, -1, 0}
    for q in range(m):
        assert got[q].to_ints() == [hv * sv % p for hv, sv in zip(h, s_shares[q])], q


def test_planted_zeros_give_zero():
    from bsgn_cpuctx import BsgnCpuFieldContext
    check_zeros(BsgnCpuFieldContext)


WRONG = ('mask_without_beta', 'symbol_swapped', 'finish_zero_residue', 'sum_is_row0')


@pytest.mark.parametrize('wrong', WRONG)
def test_a_wrong_step_is_caught(wrong):
    from bsgn_cpuctx import BsgnCpuFieldContext

    def make(p):
        ctx = BsgnCpuFieldContext(p)
        assert getattr(ctx, wrong) is False
        setattr(ctx, wrong, True)
        return ctx

    # every check alone: which of them sees this switch
    seen = []
    for name, chk in (('fixture', lambda: check_fixture(make, 3, 1)), ('zeros', lambda: check_zeros(make))):
        try:
            chk()
        except AssertionError:
            seen.append(name)
    assert seen, 'the wrong step went unnoticed'
    # the fixture holds no zero symbol: only the planted zeros tell 0 from a residue
    assert ('fixture' in seen) == (wrong != 'finish_zero_residue') and (wrong != 'finish_zero_residue' or seen == ['zeros'])


def test_bsgn_refusals():
    from mpyc_amd import protocols
    from bsgn_cpuctx import BsgnCpuFieldContext
    p = DEMO_PRIMES[0]
    ctx = BsgnCpuFieldContext(p)
    F = gf(p)
    rng = random.Random(2)
    xs = _share(ctx, rng, [1, -1, 2], 1, 3)
    draws = Draws(ctx, 3, 1, 1)
    assert [_signed(v, p) for v in open_two_ways(ctx, protocols.bsgn(ctx, F, xs, 1, 0, draws), 1)] == [1, -1, 1]
    with pytest.raises(ValueError):
        protocols.bsgn(ctx, F, xs, 1, 3, draws)                           # d
    with pytest.raises(ValueError):
        protocols.bsgn(ctx, F, xs[:2], 1, 0, Draws(ctx, 2, 1, 1))         # m = 2t
    p1 = 2**40 - 87                                                       # 1 mod 4
    ctx1 = BsgnCpuFieldContext(p1)
    with pytest.raises(ValueError):
        protocols.bsgn(ctx1, gf(p1), _share(ctx1, rng, [1], 1, 3), 1, 0, Draws(ctx1, 3, 1, 1))
    ctxb = BsgnCpuFieldContext(0x11b, True)
    with pytest.raises(ValueError):
        protocols.bsgn(ctxb, None, [ctxb.from_ints([1])] * 3, 1, 0, draws)
    for bad in (lambda c: (draws(c)[0], draws(c - 1)[1]),                 # a short sharing
                lambda c: (draws(c)[0][:2], draws(c)[1]),                 # a party missing
                lambda c: draws(c)[0],                                    # one sharing
                lambda c: (draws(c + 1))):                                # too many entries
        with pytest.raises(ValueError):
            protocols.bsgn(ctx, F, xs, 1, 1, bad)
    # the stand-in refuses what the engine refuses
    a, z = ctx.from_ints([1, 2]), ctx.from_ints([1, 2, 3, 4])
    for call in (lambda: ctx.bsgn_mask(a, z, 2, []), lambda: ctx.bsgn_mask(a, z, 2, [1] * 9), lambda: ctx.bsgn_mask(a, z, 2, [1]),
                 lambda: ctx.bsgn_mask(a, z, 2, [1, 3], out=a), lambda: ctx.bsgn_finish(z, [], 2), lambda: ctx.bsgn_finish(z, [z], 3),
                 lambda: ctx.bsgn_finish(z, [a], 2), lambda: ctx.bsgn_finish(z, [z], 9), lambda: ctx.bsgn_finish(z, [z], 2, outs=[z, z]),
                 lambda: ctx.bsgn_finish(z, [z], 2, sum=True, outs=[z])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: ctxb.bsgn_mask(a, z, 2, [1, 3]), lambda: ctxb.bsgn_finish(z, [z], 2), lambda: ctx.bsgn_finish(z, [z] * 65, 2)):
        with pytest.raises(NotImplementedError):
            call()
    assert ctx.bsgn_mask(a, z, 2, [1, p - 1]).to_ints() == [3, 10, 3, 12]
    assert [x.to_ints() for x in ctx.bsgn_finish(ctx.from_ints([4, 0, p - 4, 9]), [ctx.from_ints([5, 6, 7, 8])], 2, sum=True)] == \
        [[(5 - 7) % p, 8]]


@pytest.mark.parametrize('d', [0, 1, 2])
def test_bsgn_runs_on_the_supplier_alone(d):
    from mpyc_amd import protocols
    from bsgn_cpuctx import BsgnCpuFieldContext
    e = golden()[d]
    p, B = e['p'], e['B']
    ctx = BsgnCpuFieldContext(p)
    F = gf(p)
    R = protocols.Randomness(ctx, F, 1, 3, b'bsgn end to end 1')
    a = [0, 1, -1, B, -B, B + 1, -B - 1, B - 1, 1 - B, 17, -17, 100]
    before = R.counter
    got = protocols.bsgn(ctx, F, _share(ctx, random.Random(d), a, 1, 3), 1, d, R.rand_bsgn)
    assert [_signed(v, p) for v in open_two_ways(ctx, got, 1)] == [e['bsgn'][e['a'].index(v)] for v in a]
    assert R.counter > before
    s, r = R.rand_bsgn(10)
    assert set(open_two_ways(ctx, s, 1)) <= {1, p - 1} and len(set(open_two_ways(ctx, r, 1))) == 10
