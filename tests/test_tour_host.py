"""CPU checks of the tournament feature: the four C ABI entries exist in header, library and binding; the two pairings in
closed form and the launch plan of the kernels (mpyc_amd/csrc/tour_geom.hpp) walked by tests/tour_check.cpp with g++
against brute-force enumeration of the reference's slices; protocols.amax / amin / argmax / argmin / arg_index / maximum /
minimum composed over a Python-integer context (tests/tour_cpuctx.py) open to numpy's results and to the reference's
(tests/golden/tour/tournament.json), and do not with a context whose tour_select swaps the sign or whose tour_unit_expand
writes v to the even slot.  No GPU needed."""
import json
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_sort_host import _lagrange, _share, _signed

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, 'golden', 'tour', 'tournament.json')


def test_tour_entries_in_header_library_and_binding():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    for name, nparams in (('ffgpu_tour_diff', 9), ('ffgpu_tour_select', 12), ('ffgpu_tour_unit_prod', 8), ('ffgpu_tour_unit_expand', 10)):
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, f'{name} is not declared in include/ffgpu.h'
        params = [p.strip() for p in m.group(1).split(',')]
        assert len(params) == nparams, params
        assert re.search(r' T ' + name + r'\b', out), f'{name} is not exported by libffgpu.so'
        assert name in _ffi.EXPORTED and len(_ffi._SIGS[name]) == nparams
    assert re.search(r'#define\s+FFGPU_TOUR_HALVES\s+0\b', hdr) and re.search(r'#define\s+FFGPU_TOUR_ODD_EVEN\s+1\b', hdr)
    L = _ffi.lib()
    # no context: refused before anything is touched
    assert L.ffgpu_tour_diff(None, None, None, 1, 8, 1, 0, 0, None) == _ffi.EINVAL
    assert L.ffgpu_tour_select(None, None, None, None, 1, None, 1, 8, 1, 0, 0, None) == _ffi.EINVAL
    assert L.ffgpu_tour_unit_prod(None, None, None, None, 1, 8, 1, None) == _ffi.EINVAL
    assert L.ffgpu_tour_unit_expand(None, None, None, None, 1, None, 1, 8, 1, None) == _ffi.EINVAL


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_tour_geometry_on_the_host(tmp_path):
    """every k in 2..300, both pairings: first / second equal the reference's slices, the pairs are disjoint and cover the
    axis with the bye; the launch plan owns every compact element, every member, every position of the next level and the
    bye once, for five element sizes"""
    exe = str(tmp_path / 'tour_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'tour_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'tour ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) > 10000


def test_the_stand_in_pairs_as_the_closed_forms():
    from tour_cpuctx import HALVES, ODD_EVEN, pair_slices
    for k in range(2, 301):
        n0, h = k % 2, k // 2
        kc = h + n0
        assert pair_slices(k, HALVES) == ([n0 + j for j in range(h)], [kc + j for j in range(h)])
        assert pair_slices(k, ODD_EVEN) == ([n0 + 2 * j for j in range(h)], [n0 + 2 * j + 1 for j in range(h)])


# ---- the protocols over Python integers ---------------------------------------------------------------------------------
MODULUS, L = 2**61 - 1, 16
CASES = [(3, 1), (7, 3)]
SHAPES = [(1, 2, 1), (1, 3, 1), (4, 7, 1), (2, 5, 3), (1, 16, 2), (3, 33, 1)]


def _values(rng, shape):
    """integers of L-2 signed bits (every difference has L-1 signed bits): both extremes, the maximum and the minimum
    twice along k where k > 2, an all-equal row where there are three rows"""
    outer, k, inner = shape
    lo, hi = -(1 << (L - 3)), (1 << (L - 3)) - 1
    a = np.array([rng.randint(lo, hi) for _ in range(outer * k * inner)], dtype=np.int64).reshape(shape)
    a[0, 0, 0], a[-1, -1, -1] = hi, lo
    if k > 2:
        a[0, k - 1, 0] = hi
        a[-1, 1, -1] = lo
    if outer > 2:
        a[1, :, :] = -7
    return a


def _golden_cases():
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    assert doc['l'] == L
    return doc['cases']


class Run:
    """one sharing of `plain` and the randomness source of a protocol run"""

    def __init__(self, ctx, m, t, seed):
        import mpyc_amd.finfields as gff
        self.ctx, self.m, self.t = ctx, m, t
        self.F = gff.GF(MODULUS)
        self.rng = random.Random(seed)
        self.counts = []

    def share(self, vals):
        return _share(self.ctx, self.rng, [int(v) for v in np.asarray(vals).reshape(-1)], self.t, self.m)

    def rand(self, count):
        self.counts.append(count)
        r = self.rng
        return (self.share([r.randrange(2) for _ in range(count * L)]), self.share([r.randrange(2) for _ in range(count)]),
                self.share([r.randrange(1 << 16) for _ in range(count)]), self.share([r.randrange(1, MODULUS) for _ in range(count)]))

    def open(self, shares, shape):
        """the value from the first and from the last t+1 parties: both must agree"""
        res = []
        for pick in (list(range(self.t + 1)), list(range(self.m - self.t - 1, self.m))):
            lam = _lagrange(MODULUS, [i + 1 for i in pick])
            got = self.ctx.recombine([shares[i] for i in pick], lam).to_ints()
            res.append(np.array([_signed(v, MODULUS) for v in got], dtype=np.int64).reshape(shape))
        assert (res[0] == res[1]).all(), 'the sharing has degree above t'
        return res[0]


def _one_hot(idx, k):
    """(outer, inner) positions -> (outer, k, inner) unit vectors"""
    return np.moveaxis(np.eye(k, dtype=np.int64)[idx], -1, 1)


def _rounds(k, inner_count):
    out = []
    while k > 1:
        out.append(k // 2 * inner_count)
        k = k // 2 + k % 2
    return out


def _check_all(ctx, m, t, plain, seed, expect=None):
    """every protocol on one array; returns the list of mismatches (empty: all agree with numpy, and with `expect`, the
    reference's outputs, when given)"""
    from mpyc_amd import protocols
    outer, k, inner = plain.shape
    run = Run(ctx, m, t, seed)
    xs = run.share(plain)
    before = [x.to_ints() for x in xs]
    bad = []

    def cmp(name, got, want):
        if got.shape != want.shape or (got != want).any():
            bad.append(name)

    top = run.open(protocols.amax(ctx, run.F, xs, outer, k, inner, t, L, run.rand), (outer, 1, inner))
    assert run.counts == _rounds(k, outer * inner)
    bot = run.open(protocols.amin(ctx, run.F, xs, outer, k, inner, t, L, run.rand), (outer, 1, inner))
    cmp('amax', top, plain.max(axis=1, keepdims=True))
    cmp('amin', bot, plain.min(axis=1, keepdims=True))
    results = {'amax': top, 'amin': bot}
    for name, fn, npfn, ext in (('argmax', protocols.argmax, np.argmax, np.max), ('argmin', protocols.argmin, np.argmin, np.min)):
        run.counts.clear()
        unit, value = fn(ctx, run.F, xs, outer, k, inner, t, L, run.rand)
        assert run.counts == _rounds(k, outer * inner)
        assert all(u.n == plain.size for u in unit) and all(v.n == outer * inner for v in value)
        u, v = run.open(unit, plain.shape), run.open(value, (outer, 1, inner))
        cmp(name + ' unit', u, _one_hot(npfn(plain, axis=1), k))
        cmp(name + ' value', v, ext(plain, axis=1, keepdims=True))
        cmp(name + ' index', run.open(protocols.arg_index(ctx, unit, outer, k, inner), (outer, inner)), npfn(plain, axis=1))
        results[name + '_unit'], results[name + '_value'] = u, v
    if expect is not None:
        for key, got in results.items():
            cmp('reference ' + key, got.reshape(-1), np.array(expect[key], dtype=np.int64))
    assert [x.to_ints() for x in xs] == before, 'a protocol wrote its input'
    return bad


@pytest.mark.parametrize('m,t', CASES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_tournaments_open_to_numpy(m, t, shape):
    from tour_cpuctx import TourCpuFieldContext
    rng = random.Random(1000 * m + 10 * shape[1] + shape[2])
    assert _check_all(TourCpuFieldContext(MODULUS), m, t, _values(rng, shape), seed=7 * m + shape[1]) == []


def test_tournaments_open_to_the_reference():
    """the reference's own outputs (one party) for arrays with ties"""
    from tour_cpuctx import TourCpuFieldContext
    cases = _golden_cases()
    assert len(cases) >= 4
    for i, case in enumerate(cases):
        plain = np.array(case['values'], dtype=np.int64).reshape(case['shape'])
        assert _check_all(TourCpuFieldContext(MODULUS), 3, 1, plain, seed=50 + i, expect=case) == []


def test_all_equal_rows_and_maximum_minimum():
    from mpyc_amd import protocols
    from tour_cpuctx import TourCpuFieldContext
    ctx = TourCpuFieldContext(MODULUS)
    assert _check_all(ctx, 3, 1, np.full((2, 6, 2), 11, dtype=np.int64), seed=3) == []
    for m, t in CASES:
        run = Run(ctx, m, t, seed=90 + m)
        n = 37
        lo, hi = -(1 << (L - 3)), (1 << (L - 3)) - 1
        x = np.array([hi, lo, 0, 5, lo, hi] + [run.rng.randint(lo, hi) for _ in range(n - 6)], dtype=np.int64)
        y = np.array([lo, hi, 0, 5, lo, hi] + [run.rng.randint(lo, hi) for _ in range(n - 6)], dtype=np.int64)
        xs, ys = run.share(x), run.share(y)
        before = [v.to_ints() for v in xs + ys]
        assert (run.open(protocols.maximum(ctx, run.F, xs, ys, t, L, run.rand), (n,)) == np.maximum(x, y)).all()
        assert (run.open(protocols.minimum(ctx, run.F, xs, ys, t, L, run.rand), (n,)) == np.minimum(x, y)).all()
        assert run.counts == [n, n] and [v.to_ints() for v in xs + ys] == before


WRONG_SHAPES = [(4, 7, 1), (2, 5, 3), (1, 16, 2)]


@pytest.mark.parametrize('shape', WRONG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_a_select_with_the_sign_swapped_is_caught(shape):
    """the deliberately wrong context: tour_select subtracts v where it has to add it and the other way round"""
    from tour_cpuctx import TourCpuFieldContext
    ctx = TourCpuFieldContext(MODULUS)
    ctx.select_sign_swapped = True
    bad = _check_all(ctx, 3, 1, _values(random.Random(5), shape), seed=11)
    assert {'amax', 'amin', 'argmax value', 'argmin value'} <= set(bad)


@pytest.mark.parametrize('shape', WRONG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_an_expand_that_writes_v_to_the_even_slot_is_caught(shape):
    """the deliberately wrong context: tour_unit_expand writes v to n0 + 2j and u - v to n0 + 2j + 1"""
    from tour_cpuctx import TourCpuFieldContext
    ctx = TourCpuFieldContext(MODULUS)
    ctx.expand_even_gets_v = True
    bad = _check_all(ctx, 3, 1, _values(random.Random(6), shape), seed=12)
    assert {'argmax unit', 'argmin unit', 'argmax index', 'argmin index'} <= set(bad)
    assert not {'amax', 'amin', 'argmax value', 'argmin value'} & set(bad)


def test_tournaments_refuse_wrong_shapes_and_too_few_parties():
    from mpyc_amd import protocols
    from tour_cpuctx import TourCpuFieldContext
    ctx = TourCpuFieldContext(MODULUS)
    run = Run(ctx, 3, 1, seed=1)
    xs = run.share(list(range(12)))
    rand = lambda count: (_ for _ in ()).throw(AssertionError('no randomness may be drawn'))
    for fn in (protocols.amax, protocols.amin, protocols.argmax, protocols.argmin):
        with pytest.raises(ValueError):
            fn(ctx, run.F, xs, 1, 13, 1, 1, L, rand)
        with pytest.raises(ValueError):
            fn(ctx, run.F, xs, 0, 12, 1, 1, L, rand)
        with pytest.raises(ValueError):
            fn(ctx, run.F, xs[:2], 1, 12, 1, 1, L, rand)
    with pytest.raises(ValueError):
        protocols.maximum(ctx, run.F, xs[:2], xs[:2], 1, L, rand)
    with pytest.raises(ValueError):
        protocols.maximum(ctx, run.F, xs, run.share(list(range(11))), 1, L, rand)
    with pytest.raises(ValueError):
        protocols.arg_index(ctx, xs, 1, 13, 1)
    # k == 1: nothing to compare; a copy comes back, and the unit vector is the public 1
    out = protocols.amax(ctx, run.F, xs, 12, 1, 1, 1, L, rand)
    assert [o.to_ints() for o in out] == [x.to_ints() for x in xs] and all(o.t.data_ptr() != x.t.data_ptr() for o, x in zip(out, xs))
    unit, value = protocols.argmin(ctx, run.F, xs, 4, 1, 3, 1, L, rand)
    assert all(u.to_ints() == [1] * 12 for u in unit) and [v.to_ints() for v in value] == [x.to_ints() for x in xs]
    # the stand-in refuses what the engine refuses
    with pytest.raises(ValueError):
        ctx.tour_diff(xs[0], 1, 12, 1, 2)
    with pytest.raises(ValueError):
        ctx.tour_diff(xs[0], 12, 1, 1, 0)
    with pytest.raises(ValueError):
        ctx.tour_select(xs[0], [], [], 1, 12, 1, 0)
