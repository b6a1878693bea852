"""CPU checks of the Legendre zero test: the three C ABI entries of include/ffgpu_math.h exist in header, library and binding
(and leave the 104 names of include/ffgpu.h alone); the unit / row index of the mask, the code bytes of a pack and the plans
(mpyc_amd/csrc/iszero_geom.hpp) walked by tests/iszero_check.cpp with g++ against brute-force enumeration;
protocols.equal_route against the reference's recorded dispatch; protocols.is_zero / equal composed over a Python-integer
context (tests/iszero_cpuctx.py) against a model on plain integers fed the same draws -- the opened values c, the codes and the
result -- and, at k = 30, against [a == b] and the reference's recorded results (tests/golden/iszero/iszero.json); and they do
not with a mask without its factor 2, a finish that ignores a zero, a code that takes p - 1 for a residue, an opening from
t + 1 parties or a product over k - 1 rows.  No GPU needed."""
import json
import os
import random
import re
import shutil
import subprocess

import pytest

from test_fxp_host import Run

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, 'golden', 'iszero', 'iszero.json')
CASES = [(3, 1), (7, 3)]
KS = (8, 9, 30)
ENTRIES = (('ffgm_iszero_mask', 9), ('ffgm_legendre_code', 5), ('ffgm_iszero_finish', 6))


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_iszero_entries_in_header_library_and_binding():
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
    ffgpu_hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ffgpu.h')).read(), flags=re.S)
    assert len(re.findall(r' T ffgpu_\w+', out)) == 104 == len(set(re.findall(r'\b(ffgpu_\w+)\s*\(', ffgpu_hdr))) == len(_ffi.EXPORTED)
    L_ = _ffi.lib()
    # no context: refused before anything is touched
    assert L_.ffgm_iszero_mask(None, None, None, None, None, 8, None, 4, None) == _ffi.EINVAL
    assert L_.ffgm_legendre_code(None, None, None, 4, None) == _ffi.EINVAL
    assert L_.ffgm_iszero_finish(None, None, None, None, 4, None) == _ffi.EINVAL


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_iszero_geometry_on_the_host(tmp_path):
    """every (row, element) of the masked copies is hit once and is its element of `a`, every entry and code byte of the
    symbols and of the finish is owned once, for five element sizes and both alignments"""
    exe = str(tmp_path / 'iszero_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'iszero_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'iszero ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) > 1500


def test_equal_route_is_the_reference_dispatch_cell_for_cell():
    from mpyc_amd import protocols
    rows = golden()['routes']
    assert sorted({r['l'] for r in rows}) == [16, 31, 32, 61, 62, 64, 128] and sorted({r['sec_param'] for r in rows}) == [7, 8, 30, 40]
    assert len(rows) == 28
    seen = set()
    for r in rows:
        assert sorted(r['calls'].values()) == [0, 1], 'the reference entered exactly one of the two'
        want = 'legendre' if r['calls']['_np_is_zero'] else 'bits'
        assert protocols.equal_route(r['p'], r['l'], r['sec_param']) == want, (r['l'], r['sec_param'])
        seen.add(want)
    assert seen == {'legendre', 'bits'}
    # the Blum condition, which no default field of the table fails
    assert protocols.equal_route(2**127 - 1, 64, 30) == 'legendre' and protocols.equal_route(2**107 - 1, 64, 30) == 'legendre'
    assert protocols.equal_route(2**130 - 5, 64, 30) == 'legendre' and protocols.equal_route(2**40 - 87, 64, 30) == 'bits'
    assert (2**130 - 5) % 4 == 3 and (2**40 - 87) % 4 == 1
    for e in golden()['equal']:
        want = 'legendre' if e['calls']['_np_is_zero'] else 'bits'
        assert protocols.equal_route(e['p'], e['l'], golden()['sec_param']) == want


def test_recorded_symbols_are_euler_s_criterion():
    """the fixture's is_sqr against pow(c, (p-1)/2, p), which both the stand-in and the device compute; 0 counts as a square"""
    from iszero_cpuctx import legendre_code_ref
    rows = golden()['is_sqr']
    assert len(rows) == 11
    for r in rows:
        p, vals = r['p'], r['values']
        assert len(vals) == 64 and vals[:3] == [0, 1, p - 1]
        assert [int(c != 0) for c in legendre_code_ref(p, vals)] == r['is_sqr'], r['name']
        assert legendre_code_ref(p, vals)[0] == 2 and r['is_sqr'][2] == (0 if p % 4 == 3 else 1)


# ---- the protocol over Python integers ----------------------------------------------------------------------------------------
class ZeroRun(Run):
    """Run plus the randomness of the zero test, recorded as plain integers.  plant: entries (row, element) whose s is 0 and
    whose z is 1 -- the masked value is then a r alone, zero where a is"""

    def __init__(self, *args, plant=(), **kw):
        super().__init__(*args, **kw)
        self.plant, self.draws, self.n = plant, [], None

    def rand_zero(self, count):
        p = self.p
        z = [self.rng.randrange(2) for _ in range(count)]
        r = [self.rng.randrange(p) for _ in range(count)]
        s = [self.rng.randrange(p) for _ in range(count)]
        for i, e in self.plant:
            z[i * self.n + e], s[i * self.n + e] = 1, 0
        self.draws.append((z, r, s))
        return self.share(z), self.share(r), self.share(s)


def model(p, a, k, z, r, s):
    """_np_is_zero on plain integers for the drawn randomness: the opened values, the codes and the result"""
    n = len(a)
    c = [(a[e] * r[i * n + e] + (1 - 2 * z[i * n + e]) * s[i * n + e] ** 2) % p for i in range(k) for e in range(n)]
    code = [2 if v == 0 else 1 if pow(v, (p - 1) // 2, p) == 1 else 0 for v in c]
    rows = [zz if cd == 0 else 1 - zz if cd == 1 else 1 for cd, zz in zip(code, z)]
    res = [1] * n
    for i in range(k):
        for e in range(n):
            res[e] *= rows[i * n + e]
    return c, code, res


def run_zero(p, a, b, m, t, k, seed, plant=(), ctx=None, **flags):
    """protocols.is_zero (b is None) or equal on plain operands over the stand-in (or the context given), checked against the
    model on the same draws: the public values, the codes, the result; returns (result, model result)"""
    from iszero_cpuctx import IszeroCpuFieldContext
    from mpyc_amd import protocols

    seen = {}
    ctx = IszeroCpuFieldContext(p) if ctx is None else ctx
    real = ctx.legendre_code

    def recording(c, out=None):
        assert 'c' not in seen, 'ONE legendre_code on the public values'
        code = real(c, out)
        seen['c'], seen['code'] = c.to_ints(), code.tolist()
        return code

    ctx.legendre_code = recording
    for name, v in flags.items():
        assert hasattr(ctx, name)
        setattr(ctx, name, v)
    run = ZeroRun(ctx, m, t, seed, plant=plant)
    run.n = len(a)
    xs = run.share(a)
    ys = None if b is None else run.share(b)
    before = [x.to_ints() for x in xs + (ys or [])]
    if b is None:
        got = protocols.is_zero(ctx, run.F, xs, t, k, run.rand_zero)
    else:
        got = protocols.equal(ctx, run.F, xs, ys, t, k, run.rand_zero)
    assert [x.to_ints() for x in xs + (ys or [])] == before, 'the inputs were written'
    assert len(got) == m and all(g.n == len(a) for g in got)
    del ctx.legendre_code
    res = run.open(got)                                                  # (first and last t+1 parties agree: degree <= t)
    (z, r, s), = run.draws
    d = [(x - y) % p for x, y in zip(a, b or [0] * len(a))]
    c, code, want = model(p, d, k, z, r, s)
    assert seen['c'] == c, 'the opened values are not a r + (1 - 2 z) u^2'
    assert seen['code'] == code, 'the codes'
    assert res == want, 'the result differs from the model on the same draws'
    return res, want


@pytest.mark.parametrize('m,t', CASES)
@pytest.mark.parametrize('k', KS)
def test_equal_opens_to_the_model_and_at_k_30_to_the_truth(m, t, k):
    """k = 8, 9: only the model on the same draws (a false positive has probability 2^-k per unequal element); k = 30: the
    model has no false positive with these seeds, so the result is [a == b], the reference's recorded values"""
    for i, e in enumerate(golden()['equal']):
        p, a, b = e['p'], e['a'], e['b']
        assert p % 4 == 3 and len(a) == len(b) == 90
        if k != 30:                                                      # a third of the pairs: every kind, the extremes included
            a, b = a[:30], b[:30]
        res, want = run_zero(p, a, b, m, t, k, seed=5000 + 100 * k + 10 * m + i)
        if k == 30:
            assert want == [int(x == y) for x, y in zip(a, b)], 'the model has a false positive: pick another seed'
            assert res == e['equal'], (e['type'], e['l'])
    assert 1 in e['equal'] and 0 in e['equal']


@pytest.mark.parametrize('m,t', CASES)
def test_planted_zero_masks(m, t):
    """s = 0 (and z = 1) planted on entries with a = 0 and with a != 0: the opened value is 0 where a is, code 2, and the row
    counts as 1"""
    p = 2**80 - 65
    a = [0, 7, 0, p - 1, 1, 0, 123456789]
    for k in (1, 2, 9):
        plant = [(0, 0), (0, 1), (k - 1, 2), (k - 1, 3), (0, 5), (k - 1, 5)]
        res, want = run_zero(p, a, None, m, t, k, seed=6000 + k, plant=plant)
        if k == 9:
            assert res == [1, 0, 1, 0, 0, 1, 0]
        assert [res[e] for e in (0, 2, 5)] == [1, 1, 1], 'a zero is never missed'


WRONG = ('mask_without_two', 'finish_ignores_zero', 'code_minus_one', 'open_t_plus_1', 'prod_k_minus_1', 'prod_drops_last_row')


@pytest.mark.parametrize('wrong', WRONG)
def test_a_wrong_step_is_caught(wrong, monkeypatch):
    """prod_k_minus_1: prod_rows told k - 1 rows of the same array (the shapes no longer fit); prod_drops_last_row: the product of
    rows 0 .. k-2 only -- at k = 2 a nonzero element passes when its first row alone is 1, which the model on the same draws
    tells apart (24 nonzero elements: it happens for several of them with this seed)"""
    from mpyc_amd import protocols
    p = 2**80 - 65
    a = [0, 7, 0, p - 1, 1, 0, 123456789] + list(range(2, 22))
    k = 2 if wrong == 'prod_drops_last_row' else 9
    plant, flags = [(0, 0), (0, 1), (k - 1, 2), (k - 1, 3)], {}
    run_zero(p, a, None, 3, 1, k, seed=7000, plant=plant)                # the right steps pass on these very draws
    if wrong == 'open_t_plus_1':
        real = protocols.open_
        monkeypatch.setattr(protocols, 'open_', lambda ctx, field, xs, t, degree=None: real(ctx, field, xs, t))
    elif wrong == 'prod_k_minus_1':
        real = protocols.prod_rows
        monkeypatch.setattr(protocols, 'prod_rows', lambda ctx, field, xs, rows, t, rng=None: real(ctx, field, xs, rows - 1, t, rng))
    elif wrong == 'prod_drops_last_row':
        real = protocols.prod_rows
        monkeypatch.setattr(protocols, 'prod_rows', lambda ctx, field, xs, rows, t, rng=None: real(ctx, field, [
            protocols._rows(ctx, x, 0, rows - 1, x.n // rows) for x in xs], rows - 1, t, rng))
    else:
        flags[wrong] = True
    with pytest.raises((AssertionError, ValueError) if wrong == 'prod_k_minus_1' else AssertionError):
        run_zero(p, a, None, 3, 1, k, seed=7000, plant=plant, **flags)


def test_a_finish_that_ignores_a_zero_misses_a_zero():
    """the planted entry (a = 0, s = 0, z = 1) opens to 0; taken for a residue its row is 1 - z = 0 and the zero is lost"""
    from iszero_cpuctx import iszero_finish_ref
    p = 2**61 - 1
    assert iszero_finish_ref(p, [2, 2, 1, 1, 0, 0], [1, 0, 1, 0, 1, 0]) == [1, 1, 0, 1, 1, 0]
    assert iszero_finish_ref(p, [2, 2], [1, 0], ignore_zero=True) == [0, 1]
    assert iszero_finish_ref(p, [1, 0], [5, 5]) == [p - 4, 5], 'z is a share: any field element'


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _no_draw(*_):
    raise AssertionError('no randomness may be drawn')


def test_refusals():
    from iszero_cpuctx import IszeroCpuFieldContext
    from mpyc_amd import protocols
    ctx = IszeroCpuFieldContext(2**80 - 65)
    run = ZeroRun(ctx, 3, 1, seed=1)
    run.n = 2
    xs = run.share([5, 0])
    with pytest.raises(ValueError):
        protocols.is_zero(ctx, run.F, xs, 1, 0, _no_draw)                    # k < 1
    with pytest.raises(ValueError):
        protocols.is_zero(ctx, run.F, xs[:2], 1, 8, _no_draw)                # fewer than 2t+1 parties
    with pytest.raises(ValueError):
        protocols.equal(ctx, run.F, xs, xs[:2], 1, 8, _no_draw)
    with pytest.raises(ValueError):
        protocols.is_zero(ctx, run.F, xs, 1, 8, lambda count: (run.share([0] * count),) * 2 + (run.share([0] * (count - 1)),))
    ctx1 = IszeroCpuFieldContext(2**40 - 87)                                 # p = 1 mod 4: -1 is a residue
    run1 = ZeroRun(ctx1, 3, 1, seed=2)
    with pytest.raises(ValueError):
        protocols.is_zero(ctx1, run1.F, run1.share([5, 0]), 1, 8, _no_draw)
    # the stand-in refuses what the engine refuses
    a, kn = ctx.from_ints([1, 2]), ctx.from_ints([1, 2, 3, 4])
    for call in (lambda: ctx.iszero_mask(a, kn, kn, kn, 0), lambda: ctx.iszero_mask(a, kn, kn, a, 2),
                 lambda: ctx.iszero_mask(a, kn, kn, kn, 2, out=a), lambda: ctx.iszero_finish(ctx.legendre_code(a), kn),
                 lambda: ctx.iszero_finish(ctx.legendre_code(kn), kn, out=a)):
        with pytest.raises(ValueError):
            call()
    assert ctx.iszero_mask(a, kn, ctx.from_ints([0, 1, 5, 0]), ctx.from_ints([10, 20, 30, 40]), 2).to_ints() == \
        [1 + 10, (4 - 20) % ctx.modulus, (3 - 9 * 30) % ctx.modulus, 8 + 40]
    assert ctx.legendre_code(ctx.from_ints([0, 1, 4, ctx.modulus - 1, ctx.modulus - 4])).tolist() == [2, 1, 1, 0, 0]
