"""CPU checks of the first-occurrence search: the three C ABI entries exist in header, library and binding; the pairing over
k + virt positions, the public leaf and the launch plans (mpyc_amd/csrc/find_geom.hpp) walked by tests/find_check.cpp with
g++ against brute-force enumeration; protocols.find composed over a Python-integer context (tests/find_cpuctx.py) opens to
numpy's results and to the reference's (tests/golden/find/find.json) in bit_length(k) rounds, and does not with a context
that ignores flip, whose public leaf has nf = 0, or that pairs (2j, 2j + 1) without the bye shift.  No GPU needed."""
import json
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_tour_host import CASES, L, MODULUS, Run

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, 'golden', 'find', 'find.json')


def test_find_entries_in_header_library_and_binding():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    for name, nparams in (('ffgpu_find_leaf_prod', 11), ('ffgpu_find_leaf_apply', 14), ('ffgpu_find_prod', 8)):
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, f'{name} is not declared in include/ffgpu.h'
        params = [p.strip() for p in m.group(1).split(',')]
        assert len(params) == nparams, params
        assert re.search(r' T ' + name + r'\b', out), f'{name} is not exported by libffgpu.so'
        assert name in _ffi.EXPORTED and len(_ffi._SIGS[name]) == nparams
    L_ = _ffi.lib()
    # no context: refused before anything is touched
    assert L_.ffgpu_find_leaf_prod(None, None, None, None, 1, 8, 1, 2, 0, 1, None) == _ffi.EINVAL
    assert L_.ffgpu_find_leaf_apply(None, None, None, None, None, 1, None, 1, 8, 1, 2, 0, 1, None) == _ffi.EINVAL
    assert L_.ffgpu_find_prod(None, None, None, 1, 8, 1, 2, None) == _ffi.EINVAL


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_find_geometry_on_the_host(tmp_path):
    """k in 1..300, virt 0 and 1, five element sizes, inner in {1, 3, 64, 65, 128}: every compact element, pair member,
    next-level position and the bye is owned once; the public leaf's position never becomes a bit address; no address falls
    outside outer * k * inner"""
    exe = str(tmp_path / 'find_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'find_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'find ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) > 10000


# ---- the protocol over Python integers ------------------------------------------------------------------------------------
def variants(k):
    """(key, keyword arguments of protocols.find, what it opens to for the index ix (k where s does not occur) and the flag
    `found`) -- the calls tests/golden/make_golden_find.py records, under the same keys"""
    return [('e_default', {}, lambda ix, found: ix),
            ('e_minus1', {'e': -1}, lambda ix, found: ix if found else -1),
            ('e_last', {'e': 'k-1'}, lambda ix, found: min(ix, k - 1)),
            ('raw', {'e': None}, lambda ix, found: (0 if found else 1, ix)),
            ('pow', {'cs_f': lambda b, i: (b + 1) << i}, lambda ix, found: 1 << ix),
            ('tuple', {'cs_f': lambda b, i: (i + b, (b + 1) << i)}, lambda ix, found: (ix, 1 << ix)),
            ('f', {'f': lambda i: k - i}, lambda ix, found: k - ix)]


def first_index(plain, s):
    """numpy: (ix, found), ix = k where s does not occur"""
    hit = plain == s
    found = hit.any(axis=1)
    return np.where(found, hit.argmax(axis=1), plain.shape[1]), found


def golden_cases():
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    assert doc['l'] == L
    return doc['cases']


def recorded(case, s, key):
    """the reference's values for a variant, in the layout of `opened()`"""
    r = case['s'][str(s)]
    if key == 'raw':
        return [r['raw_nf'], r['raw_ix']]
    return r[key] if key == 'tuple' else [r[key]]


class Counting:
    """counts the re-sharing rounds of a call: split_rng calls / (2t+1)"""

    def __init__(self, ctx, t):
        self.calls, self.t, inner = 0, t, ctx.split_rng

        def split_rng(*a, **kw):
            self.calls += 1
            return inner(*a, **kw)
        ctx.split_rng = split_rng

    def rounds(self):
        r, self.calls = self.calls / (2 * self.t + 1), 0
        return r


def opened(run, res, shape):
    """a result of protocols.find as a list of (outer, inner) integer arrays: [value], [value_1, ..], or [nf, value ..]"""
    flat = []
    for x in (res if isinstance(res, tuple) else (res,)):
        flat += list(x) if isinstance(x, tuple) else [x]
    return [run.open(x, shape) for x in flat]


def check_bits(ctx, m, t, plain, seed, case=None):
    """every variant for s = 0 and 1 on one sharing of the (outer, k, inner) bits; returns the mismatches as (s, key)"""
    from mpyc_amd import protocols
    outer, k, inner = plain.shape
    run = Run(ctx, m, t, seed)
    xs = run.share(plain)
    before = [x.to_ints() for x in xs]
    count = Counting(ctx, t)
    bad = []
    for s in (0, 1):
        ix, found = first_index(plain, s)
        for key, kw, want in variants(k):
            res = protocols.find(ctx, run.F, xs, outer, k, inner, t, s=s, **kw)
            raw = kw.get('e', 0) is None
            assert count.rounds() == ((k - 1).bit_length() if raw else k.bit_length()), (key, k)
            got = opened(run, res, (outer, inner))
            exp = [[want(int(i), bool(f)) for i, f in zip(ix.reshape(-1), found.reshape(-1))]]
            exp = [list(v) for v in zip(*exp[0])] if isinstance(exp[0][0], tuple) else exp
            ok = len(got) == len(exp) and all(g.reshape(-1).tolist() == e for g, e in zip(got, exp))
            if ok and case is not None:
                ok = [g.reshape(-1).tolist() for g in got] == recorded(case, s, key)
            if not ok:
                bad.append((s, key))
    assert [x.to_ints() for x in xs] == before, 'find wrote its input'
    return bad


def check_ints(ctx, m, t, plain, s, seed, want=None):
    """bits=False: the first s among integers, e=-1"""
    from mpyc_amd import protocols
    outer, k, inner = plain.shape
    run = Run(ctx, m, t, seed)
    xs = run.share(plain)
    before = [x.to_ints() for x in xs]
    got = run.open(protocols.find(ctx, run.F, xs, outer, k, inner, t, s=s, e=-1, bits=False, l=L, rand=run.rand), (outer, inner))
    assert run.counts == [plain.size] and [x.to_ints() for x in xs] == before
    ix, found = first_index(plain, s)
    exp = np.where(found, ix, -1).reshape(-1).tolist()
    return got.reshape(-1).tolist() == exp and (want is None or exp == want)


def random_bits(rng, shape):
    """columns along k: all ones, all zeros, the first 0 at 0 and at k - 1, alternating, then random"""
    outer, k, inner = shape
    a = np.array([rng.randrange(2) for _ in range(outer * k * inner)], dtype=np.int64).reshape(shape)
    planted = [[1] * k, [0] * k, [0] + [1] * (k - 1), [1] * (k - 1) + [0], [(j + 1) % 2 for j in range(k)]]
    for c, col in enumerate(planted[:outer * inner]):
        a[c // inner, :, c % inner] = col
    return a


@pytest.mark.parametrize('m,t', CASES)
def test_find_opens_to_the_reference(m, t):
    """every recorded case: the reference's own outputs (one party) and numpy's"""
    from find_cpuctx import FindCpuFieldContext
    cases = golden_cases()
    assert [tuple(c['shape']) for c in cases] == [(1, 1, 1), (1, 2, 1), (7, 3, 1), (4, 7, 1), (2, 5, 3), (1, 16, 2), (3, 33, 1)]
    for i, case in enumerate(cases):
        ctx = FindCpuFieldContext(MODULUS)
        plain = np.array(case['bits'], dtype=np.int64).reshape(case['shape'])
        assert check_bits(ctx, m, t, plain, seed=40 + i, case=case) == []
        ints = np.array(case['ints'], dtype=np.int64).reshape(case['shape'])
        assert check_ints(ctx, m, t, ints, case['ints_s'], seed=60 + i, want=case['ints_e_minus1'])


RANDOM_SHAPES = [(6, 1, 1), (5, 2, 2), (6, 4, 1), (5, 6, 1), (2, 9, 3), (6, 15, 1), (5, 17, 1), (1, 32, 5), (6, 33, 1)]


@pytest.mark.parametrize('m,t', CASES)
@pytest.mark.parametrize('shape', RANDOM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_find_opens_to_numpy(m, t, shape):
    from find_cpuctx import FindCpuFieldContext
    rng = random.Random(1000 * m + 10 * shape[1] + shape[2])
    ctx = FindCpuFieldContext(MODULUS)
    assert check_bits(ctx, m, t, random_bits(rng, shape), seed=7 * m + shape[1]) == []
    if shape[1] in (1, 6, 17):
        ints = np.array([rng.randint(-3, 3) for _ in range(int(np.prod(shape)))], dtype=np.int64).reshape(shape)
        ints[0, :, 0] = 1                                 # s does not occur
        for s in (2, -3, 0):
            assert check_ints(ctx, m, t, ints, s, seed=3 * m + shape[1])


def test_the_root_keeps_nf_with_the_public_leaf():
    """the public leaf's nf is 1, so the root's nf is [s does not occur] with a default too"""
    from find_cpuctx import FindCpuFieldContext
    from mpyc_amd import protocols
    for wrong, shape in ((False, (5, 6, 1)), (False, (2, 9, 3)), (True, (5, 6, 1)), (True, (2, 9, 3))):
        ctx = FindCpuFieldContext(MODULUS)
        ctx.find_virtual_nf_zero = wrong
        outer, k, inner = shape
        plain = random_bits(random.Random(k), shape)
        run = Run(ctx, 3, 1, seed=k)
        xs = run.share(plain)
        tab = ctx.find_table(k, list(range(k)), list(range(1, k + 1)), k)
        root = protocols._find_root(ctx, run.F, xs, tab, outer, k, inner, 2, 0, 1, 1, None)
        got = run.open(root, (2, outer, inner))
        ix, found = first_index(plain, 0)
        assert (got[1] == ix).all()                       # (the value does not depend on the public leaf's nf)
        assert (got[0] == 1 - found).all() != wrong, 'a public leaf with nf = 0 must be caught'


WRONG_SHAPES = [(5, 6, 1), (2, 9, 3), (6, 15, 1)]


@pytest.mark.parametrize('shape', WRONG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_a_context_that_ignores_flip_is_caught(shape):
    from find_cpuctx import FindCpuFieldContext
    ctx = FindCpuFieldContext(MODULUS)
    ctx.find_ignores_flip = True
    bad = check_bits(ctx, 3, 1, random_bits(random.Random(5), shape), seed=11)
    assert {(1, key) for key, _, _ in variants(shape[1])} <= set(bad) and not [b for b in bad if b[0] == 0]
    ints = np.array([random.Random(6).randint(-3, 3) for _ in range(int(np.prod(shape)))], dtype=np.int64).reshape(shape)
    assert not check_ints(ctx, 3, 1, ints, 2, seed=12)


@pytest.mark.parametrize('shape', WRONG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_a_pairing_without_the_bye_shift_is_caught(shape):
    """(2j, 2j + 1) with the last position carried over instead of the first: wrong wherever k + virt is odd.  (With a default
    the misplaced position is the public leaf, which is harmless in front -- nf = 1 -- but no longer supplies f(e): the
    columns without s open to f(k), so e=-1 shows it and the default e does not.)"""
    from find_cpuctx import FindCpuFieldContext
    ctx = FindCpuFieldContext(MODULUS)
    ctx.find_no_bye_shift = True
    k = shape[1]
    bad = check_bits(ctx, 3, 1, random_bits(random.Random(8), shape), seed=13)
    odd_with_default, odd_raw = (k + 1) % 2 == 1, k % 2 == 1
    for s in (0, 1):
        assert ((s, 'e_minus1') in bad) == odd_with_default and ((s, 'raw') in bad) == odd_raw, bad


def test_find_refuses_wrong_shapes_and_too_few_parties():
    from find_cpuctx import FindCpuFieldContext
    from mpyc_amd import protocols
    ctx = FindCpuFieldContext(MODULUS)
    run = Run(ctx, 3, 1, seed=1)
    xs = run.share([1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0])
    for bad in (lambda: protocols.find(ctx, run.F, xs, 1, 13, 1, 1),
                lambda: protocols.find(ctx, run.F, xs, 0, 12, 1, 1),
                lambda: protocols.find(ctx, run.F, xs[:2], 1, 12, 1, 1),
                lambda: protocols.find(ctx, run.F, xs, 1, 12, 1, 1, s=2),
                lambda: protocols.find(ctx, run.F, xs, 1, 12, 1, 1, s=2, bits=False),
                lambda: protocols.find(ctx, run.F, xs, 1, 12, 1, 1, cs_f=lambda b, i: (i, i, i, i, i))):
        with pytest.raises(ValueError):
            bad()
    # k == 1 raw: no round; the single leaf from element-wise calls
    count = Counting(ctx, 1)
    nf, ix = protocols.find(ctx, run.F, xs, 4, 1, 3, 1, s=1, e=None)
    assert count.rounds() == 0
    plain = np.array([1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0])
    assert run.open(nf, (12,)).tolist() == (1 - plain).tolist() and run.open(ix, (12,)).tolist() == (1 - plain).tolist()
    # four values are served
    four = protocols.find(ctx, run.F, xs, 1, 12, 1, 1, cs_f=lambda b, i: (i + b, 2 * (i + b), -(i + b), 7))
    assert [run.open(v, (1,)).tolist() for v in four] == [[1], [2], [-1], [7]]
    # the stand-in and the table refuse what the engine refuses
    tab = ctx.find_table(12, list(range(12)), list(range(1, 13)), 12)
    assert tab.n == 2 * 13 and ctx.find_table(3, [0, 1, 2], [1, 2, 3]).to_ints() == [0, 1, 2, 1, 1, 1]
    assert ctx.find_table(2, [(0, -1), (1, -2)], [(1, -2), (2, -3)], (5, -5)).to_ints() == \
        [0, 1, 5, 1, 1, 0, MODULUS - 1, MODULUS - 2, MODULUS - 5, MODULUS - 1, MODULUS - 1, 0]
    for bad in (lambda: ctx.find_table(0, [], []), lambda: ctx.find_table(2, [0], [1, 2]), lambda: ctx.find_table(1, [(1, 2)], [(1,)]),
                lambda: ctx.find_table(1, [(1,) * 5], [(1,) * 5]),
                lambda: ctx.find_leaf_prod(xs[0], tab, 1, 12, 1, 6, 0, 1), lambda: ctx.find_leaf_prod(xs[0], tab, 1, 12, 1, 2, 2, 1),
                lambda: ctx.find_leaf_prod(xs[0], tab, 1, 12, 1, 2, 0, 0), lambda: ctx.find_leaf_prod(xs[0], tab, 12, 1, 1, 2, 0, 0),
                lambda: ctx.find_leaf_apply(xs[0], tab, [], [], 1, 12, 1, 2, 0, 1), lambda: ctx.find_prod(xs[0], 1, 12, 1, 2),
                lambda: ctx.find_prod(xs[0], 6, 1, 1, 2)):
        with pytest.raises(ValueError):
            bad()
