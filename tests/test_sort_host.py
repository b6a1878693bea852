"""CPU checks of the sorting feature: the three C ABI entries exist in header, library and binding; the stage list, the
closed forms and the launch plan of the compare-exchange kernels (mpyc_amd/csrc/sort_geom.hpp) walked by
tests/sort_check.cpp with g++ against brute-force enumeration; protocols.sort_stages against the reference's loop restated
here; protocols.sort composed over a Python-integer context (tests/sort_cpuctx.py) opens to numpy.sort, and does not with
a context whose cx_apply swaps the two signs.  No GPU needed."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def reference_stages(n):
    """the loop of runtime._sort / runtime.np_sort, restated: (p, d, r) and the index set of every stage"""
    out = []
    t = (n - 1).bit_length()
    p = 1 << t - 1
    while p:
        d, q, r = p, 1 << t - 1, 0
        while d:
            out.append((p, d, r, [i for i in range(n - d) if i & p == r]))
            d, q, r = q - p, q >> 1, p
        p >>= 1
    return out


def test_sort_entries_in_header_library_and_binding():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    for name, ret, nparams in (('ffgpu_cx_pairs', 'size_t', 4), ('ffgpu_cx_diff', 'int', 10), ('ffgpu_cx_apply', 'int', 12)):
        m = re.search(ret + r'\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, f'{name} is not declared in include/ffgpu.h'
        params = [p.strip() for p in m.group(1).split(',')]
        assert len(params) == nparams, params
        assert re.search(r' T ' + name + r'\b', out), f'{name} is not exported by libffgpu.so'
        assert name in _ffi.EXPORTED and len(_ffi._SIGS[name]) == nparams
    L = _ffi.lib()
    # no context: refused before anything is touched
    assert L.ffgpu_cx_diff(None, None, None, 1, 8, 1, 1, 1, 0, None) == _ffi.EINVAL
    assert L.ffgpu_cx_apply(None, None, None, None, 1, 1, 8, 1, 1, 1, 0, None) == _ffi.EINVAL
    # the pair count needs neither a context nor a device
    for k in (2, 3, 13, 64, 65, 257):
        for p, d, r, I in reference_stages(k):
            assert L.ffgpu_cx_pairs(k, p, d, r) == len(I), (k, p, d, r)
            assert L.ffgpu_cx_pairs(k, 3 * p, d, r) == 0 and L.ffgpu_cx_pairs(k, p, d + 1, r) == 0
            assert L.ffgpu_cx_pairs(k, p, d, r + p + 1) == 0
    assert L.ffgpu_cx_pairs(1, 1, 1, 0) == 0 and L.ffgpu_cx_pairs(0, 1, 1, 0) == 0


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_sort_geometry_on_the_host(tmp_path):
    """every k in 2..300: the stage list equals the reference loop, pair count and index map equal the enumeration, I and
    I + d are disjoint; the launch plan owns every compact element and every member once, for five element sizes"""
    exe = str(tmp_path / 'sort_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'sort_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'sort ok' in r.stdout, r.stdout + r.stderr
    want = sum(len(reference_stages(k)) for k in range(2, 301))
    assert int(r.stdout.split()[-1]) == want


def test_sort_stages_is_the_reference_loop():
    from mpyc_amd import protocols
    from sort_cpuctx import SortCpuFieldContext, stage_indices
    ctx = SortCpuFieldContext(2**61 - 1)
    assert list(protocols.sort_stages(0)) == [] and list(protocols.sort_stages(1)) == []
    for k in range(2, 301):
        ref = reference_stages(k)
        assert list(protocols.sort_stages(k)) == [s[:3] for s in ref]
        for p, d, r, I in ref:
            assert stage_indices(k, p, d, r) == I and ctx.cx_pairs(k, p, d, r) == len(I)
            assert [(j // p) * 2 * p + j % p + r for j in range(len(I))] == I
            assert not set(I) & {i + d for i in I}


def _share(ctx, rng, vals, t, m):
    """Shamir shares of vals (host polynomials): m DevArrays"""
    p = ctx.modulus
    rows = [[] for _ in range(m)]
    for v in vals:
        coef = [v % p] + [rng.randrange(p) for _ in range(t)]
        for i in range(m):
            rows[i].append(sum(c * pow(i + 1, k, p) for k, c in enumerate(coef)) % p)
    return [ctx.from_ints(r) for r in rows]


def _signed(v, p):
    return v - p if v > p // 2 else v


def _lagrange(p, xs):
    lam = []
    for i in xs:
        num = den = 1
        for j in xs:
            if j != i:
                num, den = num * j % p, den * (j - i) % p
        lam.append(num * pow(den, -1, p) % p)
    return lam


def _values(rng, l, shape):
    """integers of l-1 signed bits (so that every difference has l signed bits) with both extremes and duplicates"""
    lo, hi = -(1 << (l - 2)), (1 << (l - 2)) - 1
    n = int(np.prod(shape))
    vals = [lo, hi, 0, hi, lo, -1, 0, 1][:n]
    vals += [rng.randint(lo, hi) for _ in range(n - len(vals))]
    if n > 4:
        vals[-1] = vals[-2]
    rng.shuffle(vals)
    return np.array(vals, dtype=object).reshape(shape)


def _run_sort(ctx, modulus, m, t, shape, l, seed, descending=False):
    import mpyc_amd.finfields as gff
    from mpyc_amd import protocols
    F = gff.GF(modulus)
    rng = random.Random(seed)
    outer, k, inner = shape
    plain = _values(rng, l, shape)
    if descending:                                   # every row needs exchanges
        plain = -np.sort(-plain, axis=1)
    xs = _share(ctx, rng, [int(v) for v in plain.reshape(-1)], t, m)
    before = [x.to_ints() for x in xs]
    counts = []

    def rand(count):
        counts.append(count)
        sh = lambda vals: _share(ctx, rng, vals, t, m)
        return (sh([rng.randrange(2) for _ in range(count * l)]), sh([rng.randrange(2) for _ in range(count)]),
                sh([rng.randrange(1 << 16) for _ in range(count)]), sh([rng.randrange(1, modulus) for _ in range(count)]))

    out = protocols.sort(ctx, F, xs, outer, k, inner, t, l, rand)
    assert len(out) == m and all(o.n == plain.size for o in out)
    assert [x.to_ints() for x in xs] == before, 'sort wrote its input'
    assert counts == [outer * len(I) * inner for _, _, _, I in reference_stages(k) if I]
    opened = []
    for pick in (list(range(t + 1)), list(range(m - t - 1, m))):
        lam = _lagrange(modulus, [i + 1 for i in pick])
        got = ctx.recombine([out[i] for i in pick], lam).to_ints()
        opened.append(np.array([_signed(v, modulus) for v in got], dtype=object).reshape(shape))
    return plain, opened


CASES = [(3, 1), (7, 3)]
SHAPES = [(1, 13, 1), (2, 8, 3), (1, 2, 1)]


@pytest.mark.parametrize('m,t', CASES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sort_opens_to_numpy_sort(m, t, shape):
    from sort_cpuctx import SortCpuFieldContext
    modulus, l = 2**61 - 1, 10
    plain, opened = _run_sort(SortCpuFieldContext(modulus), modulus, m, t, shape, l, seed=100 * m + shape[1])
    want = np.sort(plain.astype(np.int64), axis=1)
    for got in opened:
        assert (got.astype(np.int64) == want).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_a_context_that_swaps_the_signs_is_caught(shape):
    """the deliberately wrong context: cx_apply subtracts h from the first member and adds it to the second"""
    from sort_cpuctx import SortCpuFieldContext
    modulus, l, m, t = 2**61 - 1, 10, 3, 1
    ctx = SortCpuFieldContext(modulus)
    ctx.swap_signs = True
    plain, opened = _run_sort(ctx, modulus, m, t, shape, l, seed=300 + shape[1], descending=True)
    want = np.sort(plain.astype(np.int64), axis=1)
    assert any((got != want).any() for got in opened)


def test_sort_refuses_wrong_shapes_and_too_few_parties():
    from sort_cpuctx import SortCpuFieldContext
    import mpyc_amd.finfields as gff
    from mpyc_amd import protocols
    modulus = 2**61 - 1
    F = gff.GF(modulus)
    ctx = SortCpuFieldContext(modulus)
    rng = random.Random(1)
    xs = _share(ctx, rng, list(range(12)), 1, 3)
    rand = lambda count: (_ for _ in ()).throw(AssertionError('no randomness may be drawn'))
    with pytest.raises(ValueError):
        protocols.sort(ctx, F, xs, 1, 13, 1, 1, 10, rand)
    with pytest.raises(ValueError):
        protocols.sort(ctx, F, xs, 2, 3, 3, 1, 10, rand)
    with pytest.raises(ValueError):
        protocols.sort(ctx, F, xs[:2], 1, 12, 1, 1, 10, rand)
    with pytest.raises(ValueError):
        protocols.sort(ctx, F, xs, 0, 12, 1, 1, 10, rand)
    # k == 1: nothing to sort, a copy comes back
    out = protocols.sort(ctx, F, xs, 12, 1, 1, 1, 10, rand)
    assert [o.to_ints() for o in out] == [x.to_ints() for x in xs] and all(o.t.data_ptr() != x.t.data_ptr() for o, x in zip(out, xs))
