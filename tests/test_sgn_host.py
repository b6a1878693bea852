"""CPU checks of the secure-comparison feature: the three C ABI entries exist in header, library and binding; the
geometry and index arithmetic of the kernels (mpyc_amd/csrc/sgn_geom.hpp) walked by tests/sgn_check.cpp with g++;
protocols.prod_rows / is_zero_public / compare_zero composed over a Python-integer context (tests/sgn_cpuctx.py) open to
the plaintext predicates.  No GPU needed."""
import os
import random
import re
import shutil
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def test_sgn_entries_in_header_library_and_binding():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    for name, nparams in (('ffgpu_sgn_mask', 8), ('ffgpu_sgn_expand', 11), ('ffgpu_sgn_finish', 8)):
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, f'{name} is not declared in include/ffgpu.h'
        params = [p.strip() for p in m.group(1).split(',')]
        assert len(params) == nparams and params[0].startswith('ffgpu_ctx*'), params
        assert re.search(r' T ' + name + r'\b', out), f'{name} is not exported by libffgpu.so'
        assert name in _ffi.EXPORTED and len(_ffi._SIGS[name]) == nparams
    L = _ffi.lib()
    # no context: refused before anything is touched
    assert L.ffgpu_sgn_mask(None, None, None, None, 8, None, 1, None) == _ffi.EINVAL
    assert L.ffgpu_sgn_expand(None, None, None, None, None, 8, None, None, None, 1, None) == _ffi.EINVAL
    assert L.ffgpu_sgn_finish(None, None, None, None, 8, None, 1, None) == _ffi.EINVAL


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_sgn_index_arithmetic_on_the_host(tmp_path):
    """every element size, l = 1 .. 64, n = 1 .. 700: every (element, bit) owned once, LDS indices inside the declared
    size, that size within the header's bound, every output index hit once, no bank shared by two lanes of a wave"""
    exe = str(tmp_path / 'sgn_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'sgn_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'sgn ok' in r.stdout, r.stdout + r.stderr


def _share(ctx, rng, vals, t, m):
    """Shamir shares of vals (host polynomials): m DevArrays"""
    p = ctx.modulus
    rows = [[] for _ in range(m)]
    for v in vals:
        coef = [v % p] + [rng.randrange(p) for _ in range(t)]
        for i in range(m):
            rows[i].append(sum(c * pow(i + 1, k, p) for k, c in enumerate(coef)) % p)
    return [ctx.from_ints(r) for r in rows]


def _open(ctx, field, xs, t):
    from mpyc_amd import protocols
    return protocols.open_(ctx, field, xs, t).to_ints()


def _signed(v, p):
    return v - p if v > p // 2 else v


def _values(rng, l, extra):
    lo, hi = -(1 << (l - 1)), (1 << (l - 1)) - 1
    vals = [v for v in (lo, hi, 0, -1, 1) if lo <= v <= hi]
    return vals + [rng.randint(lo, hi) for _ in range(extra)]


@pytest.mark.parametrize('modulus', [2**61 - 1, 2**80 - 65], ids=['2^61-1', '2^80-65'])
@pytest.mark.parametrize('m,t', [(3, 1), (5, 2)])
@pytest.mark.parametrize('l', [1, 5, 16])
def test_compare_zero_opens_to_the_predicate(modulus, m, t, l):
    from sgn_cpuctx import SgnCpuFieldContext
    import mpyc_amd.finfields as gff
    from mpyc_amd import protocols
    F = gff.GF(modulus)
    ctx = SgnCpuFieldContext(modulus)
    rng = random.Random(1000 * l + 10 * m + t)
    a = _values(rng, l, 4)
    n = len(a)
    xs = _share(ctx, rng, a, t, m)
    rbits = _share(ctx, rng, [rng.randrange(2) for _ in range(n * l)], t, m)
    sbits = _share(ctx, rng, [rng.randrange(2) for _ in range(n)], t, m)
    rdivl = _share(ctx, rng, [rng.randrange(1 << 20) for _ in range(n)], t, m)
    rzero = _share(ctx, rng, [rng.randrange(1, modulus) for _ in range(n)], t, m)
    lt = protocols.compare_zero(ctx, F, xs, rbits, sbits, rdivl, rzero, t, l, mode='lt')
    assert len(lt) == m and _open(ctx, F, lt, t) == [int(v < 0) for v in a]
    eq = protocols.compare_zero(ctx, F, xs, rbits, None, rdivl, None, t, l, mode='eq')
    assert len(eq) == m and _open(ctx, F, eq, t) == [int(v == 0) for v in a]
    sg = protocols.compare_zero(ctx, F, xs, rbits, sbits, rdivl, rzero, t, l, mode='sgn')
    assert [_signed(v, modulus) for v in _open(ctx, F, sg, t)] == [(v > 0) - (v < 0) for v in a]
    with pytest.raises(ValueError):
        protocols.compare_zero(ctx, F, xs, rbits, sbits, rdivl, rzero, t, l, mode='gt')


@pytest.mark.parametrize('rows', range(1, 10))
def test_prod_rows_against_the_plain_product(rows):
    from sgn_cpuctx import SgnCpuFieldContext
    import mpyc_amd.finfields as gff
    from mpyc_amd import protocols
    modulus, m, t, n = 2**61 - 1, 3, 1, 5
    F = gff.GF(modulus)
    ctx = SgnCpuFieldContext(modulus)
    rng = random.Random(rows)
    vals = [rng.randrange(modulus) for _ in range(rows * n)]
    vals[0] = modulus - 1
    xs = _share(ctx, rng, vals, t, m)
    want = [1] * n
    for i in range(rows):
        want = [w * vals[i * n + h] % modulus for h, w in enumerate(want)]
    out = protocols.prod_rows(ctx, F, xs, rows, t)
    assert len(out) == m and all(o.n == n for o in out)
    assert _open(ctx, F, out, t) == want
    with pytest.raises(ValueError):
        protocols.prod_rows(ctx, F, xs, 0, t)


def test_is_zero_public_is_zero_exactly_where_the_value_is():
    from sgn_cpuctx import SgnCpuFieldContext
    import mpyc_amd.finfields as gff
    from mpyc_amd import protocols
    modulus, m, t = 2**80 - 65, 5, 2
    F = gff.GF(modulus)
    ctx = SgnCpuFieldContext(modulus)
    rng = random.Random(9)
    vals = [0, 1, modulus - 1, 0, rng.randrange(modulus)]
    r = [rng.randrange(1, modulus) for _ in vals]
    w = protocols.is_zero_public(ctx, F, _share(ctx, rng, vals, t, m), _share(ctx, rng, r, t, m), t).to_ints()
    assert w == [v * x % modulus for v, x in zip(vals, r)]
    assert [x == 0 for x in w] == [v == 0 for v in vals]
