"""CPU checks of bit decomposition over a prime field: the eight C ABI entries exist in header, library and binding; the
host plan functions (ffgpu_carry_rounds / _rows / _level) against the reference's recursion restated in
tests/bits_cpuctx.py; mpyc_amd/csrc/bits_geom.hpp walked by tests/bits_check.cpp with g++; protocols.to_bits composed
over a Python-integer context (tests/bits_cpuctx.py) opens to the bits of a mod 2^l, including the values and bits the
reference's np_to_bits produced (tests/golden/bits/to_bits.json), and does not with each of three deliberately wrong contexts.
No GPU needed."""
import ctypes
import json
import os
import random
import re
import shutil
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

ENTRIES = (('ffgpu_carry_rounds', 1), ('ffgpu_carry_rows', 4), ('ffgpu_carry_level', 4), ('ffgpu_bits_mask', 9),
           ('ffgpu_bits_expand', 8), ('ffgpu_carry_prod', 8), ('ffgpu_carry_apply', 10), ('ffgpu_bits_finish', 8))
# l: (rounds, Rc total, Rd total, rows of the largest round)
TOTALS = {2: (1, 1, 0, 1), 3: (2, 3, 1, 2), 7: (3, 11, 5, 6), 8: (3, 12, 5, 7), 16: (4, 32, 17, 15), 32: (5, 80, 49, 31),
          33: (6, 86, 54, 31), 64: (6, 192, 129, 63)}


def golden():
    with open(os.path.join(TESTS, 'golden', 'bits', 'to_bits.json')) as fh:
        return {c['l']: c for c in json.load(fh)['cases']}


@pytest.fixture(scope='module')
def L():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi.lib()


def test_bits_entries_in_header_library_and_binding(L):
    from mpyc_amd import _ffi
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    for name, nparams in ENTRIES:
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, f'{name} is not declared in include/ffgpu.h'
        assert len([p for p in m.group(1).split(',')]) == nparams, name
        assert re.search(r' T ' + name + r'\b', out), f'{name} is not exported by libffgpu.so'
        assert name in _ffi.EXPORTED and len(_ffi._SIGS[name]) == nparams
    raw = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    doc = raw[raw.index('bit decomposition over a prime field'):raw.index('int ffgpu_carry_rounds')]
    names = ('ffgpu_bits_mask', 'ffgpu_bits_expand', 'ffgpu_carry_prod', 'ffgpu_carry_apply', 'ffgpu_bits_finish')
    starts = [doc.index(' * ' + name + ':') for name in names] + [len(doc)]
    assert starts == sorted(starts)
    for name, lo, hi in zip(names, starts, starts[1:]):
        assert 'replaces:' in doc[lo:hi], f'{name} does not say what it replaces'
    # no context: refused before anything is touched
    EINVAL = _ffi.EINVAL
    assert L.ffgpu_bits_mask(None, None, None, None, None, 8, None, 4, None) == EINVAL
    assert L.ffgpu_bits_expand(None, None, None, 8, None, None, 4, None) == EINVAL
    assert L.ffgpu_carry_prod(None, None, None, 8, 1, None, 4, None) == EINVAL
    assert L.ffgpu_carry_apply(None, None, None, None, None, 3, 8, 1, 4, None) == EINVAL
    assert L.ffgpu_bits_finish(None, None, None, None, 8, None, 4, None) == EINVAL


def lib_level(L, l, rho):
    from mpyc_amd import _ffi
    rc, rd = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.ffgpu_carry_rows(l, rho, ctypes.byref(rc), ctypes.byref(rd)) == _ffi.OK
    ks, qs = (ctypes.c_uint8 * 63)(*([255] * 63)), (ctypes.c_uint8 * 63)(*([255] * 63))
    assert L.ffgpu_carry_level(l, rho, ks, qs) == _ffi.OK
    R = rc.value + rd.value
    assert all(ks[j] == 255 and qs[j] == 255 for j in range(R, 63)), 'written past the R rows'
    rows = [(ks[j], qs[j]) for j in range(R)]
    return rows[:rc.value], rows[rc.value:]


def test_host_plan_functions_equal_the_reference_recursion(L):
    """the plan needs neither a context nor a device"""
    from mpyc_amd import _ffi
    import bits_cpuctx as bc
    seen = {}
    for l in range(1, 65):
        rounds = L.ffgpu_carry_rounds(l)
        assert rounds == bc.height(l) == (l - 1).bit_length()
        tot_c = tot_d = widest = 0
        by_round = {}
        for i, h, j, high in bc.merges(l):
            by_round.setdefault(bc.height(j - i), []).append((i, h, j, high))
        assert sorted(by_round) == list(range(1, rounds + 1))
        for rho in range(1, rounds + 1):
            c, d = lib_level(L, l, rho)
            want_c = [(k, h - 1) for i, h, j, high in by_round[rho] for k in range(h, j)]
            want_d = [(k, h - 1) for i, h, j, high in by_round[rho] if high for k in range(h, j)]
            assert (c, d) == (want_c, want_d) == bc.level(l, rho), (l, rho)
            assert all(high == (i > 0) for i, _, _, high in by_round[rho])
            ks = [k for k, _ in c]
            assert ks == sorted(set(ks)) and not {q for _, q in c} & set(ks) and set(d) <= set(c)
            tot_c, tot_d, widest = tot_c + len(c), tot_d + len(d), max(widest, len(c) + len(d))
            assert 1 <= len(c) + len(d) <= 63
        seen[l] = (rounds, tot_c, tot_d, widest)
    for l, want in TOTALS.items():
        assert seen[l] == want, l
    assert seen[1] == (0, 0, 0, 0)
    # l and round out of range
    rc, rd = ctypes.c_int(7), ctypes.c_int(7)
    buf = (ctypes.c_uint8 * 63)()
    for l in (0, -1, 65, 1 << 20):
        assert L.ffgpu_carry_rounds(l) == -1
        assert L.ffgpu_carry_rows(l, 1, ctypes.byref(rc), ctypes.byref(rd)) == _ffi.EINVAL
        assert L.ffgpu_carry_level(l, 1, buf, buf) == _ffi.EINVAL
    for l, rho in ((1, 1), (1, 0), (16, 0), (16, 5), (16, -1), (64, 7), (33, 7)):
        assert L.ffgpu_carry_rows(l, rho, ctypes.byref(rc), ctypes.byref(rd)) == _ffi.EINVAL
        assert L.ffgpu_carry_level(l, rho, buf, buf) == _ffi.EINVAL
    assert (rc.value, rd.value) == (7, 7)
    assert L.ffgpu_carry_rows(16, 1, None, ctypes.byref(rd)) == _ffi.EINVAL
    assert L.ffgpu_carry_level(16, 1, None, buf) == _ffi.EINVAL


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_bits_geometry_on_the_host(tmp_path):
    import bits_cpuctx as bc
    exe = str(tmp_path / 'bits_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'bits_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'bits ok' in r.stdout, r.stdout + r.stderr
    want = sum(len(c) + len(d) for l in range(1, 65) for rho in range(1, bc.height(l) + 1) for c, d in [bc.level(l, rho)])
    assert int(r.stdout.split()[-1]) == want


# ---- protocols.to_bits over the Python-integer context ---------------------------------------------------------------
def _share(ctx, rng, vals, t, m):
    """Shamir shares of vals (host polynomials): m DevArrays"""
    p = ctx.modulus
    rows = [[] for _ in range(m)]
    for v in vals:
        coef = [v % p] + [rng.randrange(p) for _ in range(t)]
        for i in range(m):
            rows[i].append(sum(c * pow(i + 1, k, p) for k, c in enumerate(coef)) % p)
    return [ctx.from_ints(r) for r in rows]


def _lagrange(p, xs):
    lam = []
    for i in xs:
        num = den = 1
        for j in xs:
            if j != i:
                num, den = num * j % p, den * (j - i) % p
        lam.append(num * pow(den, -1, p) % p)
    return lam


def signed_values(rng, l, n):
    lo, hi = -(1 << (l - 1)), (1 << (l - 1)) - 1
    vals = [lo, hi, 0, -1, 1, lo + 1, hi - 1, 0]
    return vals + [rng.randint(lo, hi) for _ in range(n - len(vals))]


def run_to_bits(ctx, modulus, m, t, l, seed, count=24):
    """(values, expected bits or None where the fixture has none, [opened bits per choice of t+1 shares], opened
    from_bits)"""
    import mpyc_amd.finfields as gff
    from mpyc_amd import protocols
    F = gff.GF(modulus)
    rng = random.Random(seed)
    vals = signed_values(rng, l, count)
    gold = golden().get(l)
    want = [[(v >> k) & 1 for k in range(l)] for v in vals]
    if gold:
        vals, want = vals + gold['values'], want + gold['bits']
    n = len(vals)
    xs = _share(ctx, rng, vals, t, m)
    rbits = _share(ctx, rng, [rng.randrange(2) for _ in range(n * l)], t, m)
    rdivl = _share(ctx, rng, [rng.randrange(1, 1 << 24) for _ in range(n)], t, m)
    before = [x.to_ints() for x in xs + rbits + rdivl]
    out = protocols.to_bits(ctx, F, xs, rbits, rdivl, t, l)
    assert len(out) == m and all(o.n == n * l for o in out)
    assert [x.to_ints() for x in xs + rbits + rdivl] == before, 'to_bits wrote its inputs'
    opened = []
    for pick in (list(range(t + 1)), sorted(rng.sample(range(m), t + 1)), list(range(m - t - 1, m))):
        lam = _lagrange(modulus, [i + 1 for i in pick])
        flat = ctx.recombine([out[i] for i in pick], lam).to_ints()
        opened.append([flat[h * l:(h + 1) * l] for h in range(n)])
    back = protocols.open_(ctx, F, protocols.from_bits(ctx, out, l), t).to_ints()
    return vals, want, opened, back


CASES = [(3, 1), (7, 3)]
LS = (1, 2, 3, 7, 16)


@pytest.mark.parametrize('m,t', CASES)
@pytest.mark.parametrize('l', LS)
def test_to_bits_opens_to_the_bits(m, t, l):
    """rdivl in [1, 2^24) and offset 2^l: a + 2^l + 2^l rdivl - r lies in (2^l rdivl - 2^l / 2, 2^l rdivl + 2^l 3/2), inside
    (0, 2^61 - 1): the opened value does not wrap"""
    from bits_cpuctx import BitsCpuFieldContext
    modulus = 2**61 - 1
    vals, want, opened, back = run_to_bits(BitsCpuFieldContext(modulus), modulus, m, t, l, seed=100 * m + l)
    assert want == [[(v % (1 << l)) >> k & 1 for k in range(l)] for v in vals]         # (the fixture's bits are those of a mod 2^l)
    for got in opened:
        assert got == want
    assert back == [v % (1 << l) for v in vals]


def test_to_bits_of_32_bits_with_the_golden_values():
    """l = 32: the SecInt(32) values of the fixture; from_bits over more than 16 bits takes the power-vector product"""
    from bits_cpuctx import BitsCpuFieldContext
    modulus, l = 2**61 - 1, 32                         # 2^32 (2^24 + 2) < 2^61 - 1: the opened value does not wrap
    vals, want, opened, back = run_to_bits(BitsCpuFieldContext(modulus), modulus, 3, 1, l, seed=32, count=8)
    assert want[8:] == golden()[l]['bits']
    for got in opened:
        assert got == want
    assert back == [v % (1 << l) for v in vals]


@pytest.mark.skipif(not os.path.isdir('/root/reference/mpyc'), reason='reference checkout not present (build container only)')
def test_committed_bits_fixture_reproduces_from_committed_generator(tmp_path):
    """`committed script => committed fixture`: tests/golden/make_golden_bits.py against the reference, byte for byte"""
    import sys
    env = dict(os.environ, PYTHONPATH='/root/reference', GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(TESTS, 'golden', 'make_golden_bits.py'), '--no-log'], capture_output=True,
                       text=True, cwd='/tmp', env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(tmp_path) == ['to_bits.json']
    with open(os.path.join(TESTS, 'golden', 'bits', 'to_bits.json'), 'rb') as a, open(os.path.join(tmp_path, 'to_bits.json'), 'rb') as b:
        assert a.read() == b.read()


def test_the_golden_values_are_covered():
    g = golden()
    assert sorted(g) == [16, 32]
    for l, case in g.items():
        lo, hi = -(1 << (l - 1)), (1 << (l - 1)) - 1
        assert {lo, hi, -1, 0, 1} <= set(case['values']) and len(case['values']) >= 40
        assert all(len(row) == l and set(row) <= {0, 1} for row in case['bits']) and len(case['bits']) == len(case['values'])


@pytest.mark.parametrize('flag', ['add_into_p', 'drop_d_rows', 'no_carry_in'])
@pytest.mark.parametrize('l', [7, 16])
def test_a_wrong_context_is_caught(flag, l):
    """carry_apply adding into P instead of replacing it; the d-rows of every round dropped; bits_finish without G[k-1]"""
    from bits_cpuctx import BitsCpuFieldContext
    modulus, m, t = 2**61 - 1, 3, 1
    ctx = BitsCpuFieldContext(modulus)
    setattr(ctx, flag, True)
    vals, want, opened, back = run_to_bits(ctx, modulus, m, t, l, seed=300 + l)
    assert any(got != want for got in opened)
    assert back != [v % (1 << l) for v in vals]


def test_to_bits_refuses_wrong_shapes_and_too_few_parties():
    from bits_cpuctx import BitsCpuFieldContext
    import mpyc_amd.finfields as gff
    from mpyc_amd import protocols
    modulus = 2**61 - 1
    F = gff.GF(modulus)
    ctx = BitsCpuFieldContext(modulus)
    rng = random.Random(1)
    xs, rb, rd = _share(ctx, rng, list(range(6)), 1, 3), _share(ctx, rng, [0] * 48, 1, 3), _share(ctx, rng, [1] * 6, 1, 3)
    with pytest.raises(ValueError):
        protocols.to_bits(ctx, F, xs[:2], rb[:2], rd[:2], 1, 8)
    with pytest.raises(ValueError):
        protocols.to_bits(ctx, F, xs, rb, rd, 1, 7)
    with pytest.raises(ValueError):
        protocols.to_bits(ctx, F, xs, rb, rd, 1, 60)                     # l > bit_length(p) - 2
    with pytest.raises(ValueError):
        protocols.carry_prefix(ctx, F, rb, rb[:2], 8, 6, 1)
    with pytest.raises(ValueError):
        protocols.carry_prefix(ctx, F, rb, rb, 7, 6, 1)
