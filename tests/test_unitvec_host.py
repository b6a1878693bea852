"""CPU checks of secure unit vectors and table lookup at secret indices: the three C ABI entries of include/ffgpu_math.h exist
in header, library and binding; the launch plans and the rotation (mpyc_amd/csrc/unitvec_geom.hpp) walked by
tests/unitvec_check.cpp with g++ against brute-force enumeration; protocols.unit_rounds against a brute-force model;
protocols.unit_vectors / unit_vectors_from_bits / lookup composed over a Python-integer context (tests/unitvec_cpuctx.py) for
(m, t) = (1, 0), (3, 1), (7, 3): they open to what the reference's np_unit_vector / unit_vector / T @ np_unit_vector opened
(tests/golden/unit/unit.json); indices beyond K give the documented result; every deliberately wrong switch of the stand-in is
caught; the refusals; and the protocols on nothing but protocols.Randomness.  No GPU needed."""
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
GOLDEN = os.path.join(TESTS, 'golden', 'unit', 'unit.json')
ENTRIES = (('ffgm_unit_prod', 8), ('ffgm_unit_roll', 8), ('ffgm_unit_dot', 10))
KS = (1, 2, 3, 5, 8, 13, 64)
P61 = 2**61 - 1
P31 = 2**31 - 1
PARTIES = [(1, 0), (3, 1), (7, 3)]


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_unit_entries_in_header_library_and_binding():
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
    assert L_.ffgm_unit_prod(None, None, 1, None, 2, None, 4, None) == _ffi.EINVAL
    assert L_.ffgm_unit_roll(None, None, None, 2, 3, None, 4, None) == _ffi.EINVAL
    assert L_.ffgm_unit_dot(None, None, 4, None, 2, None, 3, None, 4, None) == _ffi.EINVAL
    assert L_.ffgpu_abi_version() == 1


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_unit_geometry_on_the_host(tmp_path):
    """every (row, element) unit of each plan is covered once, for five element sizes and both alignments; the rolled source
    row and the rotated table index agree with brute force for every kbits in 1..13, every c and every j"""
    exe = str(tmp_path / 'unitvec_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'unitvec_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'unitvec ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) == 5 * 2 * 10 * 6 + 13


def test_the_fixture_is_what_the_issue_asks_for():
    doc = golden()
    assert doc['p'] == 2**64 - 189 and tuple(e['K'] for e in doc['unit']) == KS
    for e in doc['unit']:
        K = e['K']
        onehot = [[int(j == a) for j in range(K)] for a in range(K)]
        assert e['np_unit'] == onehot and e['unit'] == onehot, K
        assert len(e['table']) == K and e['lookup'] == e['table']
    assert len(set(doc['unit'][-1]['table'])) > 60


def rounds_model(K, full):
    """the rows every level needs, from the last level down: a row needs its parent j >> 1"""
    kbits = (K - 1).bit_length()
    need = set(range(1 << kbits if full else K))
    levels = [need]
    for _ in range(kbits):
        need = {j >> 1 for j in need}
        levels.append(need)
    levels.reverse()
    assert levels[0] == {0}
    for lv in levels:
        assert lv == set(range(len(lv))), 'a level is a prefix of its rows'
    return [(len(levels[s]), len(levels[s + 1])) for s in range(kbits)]


def test_the_engine_states_the_lds_limit_of_the_header():
    """FieldContext.unit_dot_max_kbits (which the stand-in inherits) against unit_dot_max_kbits of unitvec_geom.hpp, whose
    values tests/unitvec_check.cpp pins: the limits quoted in the header comment, per element size"""
    from mpyc_amd import engine
    from unitvec_cpuctx import UnitvecCpuFieldContext
    assert UnitvecCpuFieldContext.unit_dot_max_kbits is engine.FieldContext.unit_dot_max_kbits
    assert UnitvecCpuFieldContext.unit_iota is engine.FieldContext.unit_iota
    src = open(os.path.join(ROOT, 'mpyc_amd', 'csrc', 'unitvec_geom.hpp')).read()
    m = re.search(r'kbits <= ([\d, ]+)\.', src)
    limits = [int(v) for v in m.group(1).split(',')]
    assert limits == [14, 13, 12, 12, 11] and 'UNIT_LDS_BYTES = 65536' in src
    got = [UnitvecCpuFieldContext(p).unit_dot_max_kbits() for p in (2**31 - 1, 2**61 - 1, 2**80 - 65, 2**128 - 173, 2**136 - 113)]
    assert got == limits
    chk = open(os.path.join(TESTS, 'unitvec_check.cpp')).read()
    assert 'maxk[5] = {14, 13, 12, 12, 11}' in chk and 'unit_dot_max_kbits(eb) == maxk[i]' in chk


def test_unit_rounds_is_the_brute_force_plan():
    from mpyc_amd import protocols
    for K in range(1, 301):
        for full in (False, True):
            plan = protocols.unit_rounds(K, full)
            assert plan == rounds_model(K, full), (K, full)
            assert all(keep <= 2 * h for h, keep in plan)
        assert sum(h for h, _ in protocols.unit_rounds(K)) <= K + (K - 1).bit_length()       # about 2K rows written, not 2 K2
    assert protocols.unit_rounds(1) == [] and protocols.unit_rounds(2) == [(1, 2)] and protocols.unit_rounds(5) == [(1, 2), (2, 3), (3, 5)]
    with pytest.raises(ValueError):
        protocols.unit_rounds(0)


# ---- the compositions on the stand-in ----------------------------------------------------------------------------------------------
class UnitDraws:
    """rand_unit(count, kbits, sec_param) from a seeded generator: bits and values in [1, 2^sec_param] shared at degree t"""

    def __init__(self, ctx, m, t, seed):
        self.ctx, self.m, self.t, self.rng, self.handed = ctx, m, t, random.Random(seed), []

    def __call__(self, count, kbits, sec_param):
        bits = [self.rng.randrange(2) for _ in range(count * kbits)]
        R = [self.rng.randrange(1, (1 << sec_param) + 1) for _ in range(count)]
        bs, Rs = _share(self.ctx, self.rng, bits, self.t, self.m), _share(self.ctx, self.rng, R, self.t, self.m)
        self.handed.append((bs + Rs, [x.to_ints() for x in bs + Rs]))
        return bs, Rs

    def unwritten(self):
        return all([x.to_ints() for x in xs] == before for xs, before in self.handed)


def columns(flat, rows, n):
    """the n vectors of a position-major (rows, n) array"""
    assert len(flat) == rows * n
    return [[flat[j * n + e] for j in range(rows)] for e in range(n)]


def run_unit_vectors(ctx, a, K, m, t, seed=1, sec_param=30):
    from mpyc_amd import protocols
    p = ctx.modulus
    xs = _share(ctx, random.Random(1000 + seed), a, t, m)
    before = [x.to_ints() for x in xs]
    draws = UnitDraws(ctx, m, t, seed)
    got = protocols.unit_vectors(ctx, gf(p), xs, K, t, draws, sec_param=sec_param)
    assert len(got) == m and all(g.n == K * len(a) for g in got)
    assert [x.to_ints() for x in xs] == before and draws.unwritten(), 'an input of unit_vectors was written'
    assert len(draws.handed) == (K > 1)
    return columns(open_two_ways(ctx, got, t), K, len(a))


def bits_of(a, l):
    return [(v >> i) & 1 for v in a for i in range(l)]


def run_from_bits(ctx, a, l, K, m, t, seed=1):
    from mpyc_amd import protocols
    p = ctx.modulus
    bs = _share(ctx, random.Random(2000 + seed), bits_of(a, l), t, m)
    before = [x.to_ints() for x in bs]
    got = protocols.unit_vectors_from_bits(ctx, gf(p), bs, l, K, t)
    assert len(got) == m and all(g.n == K * len(a) for g in got)
    assert [x.to_ints() for x in bs] == before, 'the bits were written'
    return columns(open_two_ways(ctx, got, t), K, len(a))


def run_lookup(ctx, a, table, m, t, shared, seed=1, sec_param=30):
    from mpyc_amd import protocols
    p, K = ctx.modulus, len(table)
    rng = random.Random(3000 + seed)
    xs = _share(ctx, rng, a, t, m)
    tab = _share(ctx, rng, table, t, m) if shared else ctx.from_ints([v % p for v in table])
    draws = UnitDraws(ctx, m, t, seed)
    got = protocols.lookup(ctx, gf(p), xs, tab, K, t, draws, sec_param=sec_param)
    assert len(got) == m and all(g.n == len(a) for g in got) and draws.unwritten()
    assert (tab.to_ints() if not shared else open_two_ways(ctx, tab, t)) == [v % p for v in table], 'the table was written'
    return [_signed(v, p) for v in open_two_ways(ctx, got, t)]


def check_fixture(make_ctx, m, t, ks=KS, what=('np_unit', 'unit', 'public', 'shared')):
    """every index of every K of the fixture in one batch: n = K"""
    doc = golden()
    ctx = make_ctx(doc['p'])
    for e in doc['unit']:
        K = e['K']
        if K not in ks:
            continue
        a = list(range(K))
        if 'np_unit' in what:
            assert run_unit_vectors(ctx, a, K, m, t, seed=K) == e['np_unit'], ('np_unit_vector', K, m, t)
        if 'unit' in what:
            l = max(1, (K - 1).bit_length()) + (K % 3)                                  # more bits than the index takes
            assert run_from_bits(ctx, a, l, K, m, t, seed=K) == e['unit'], ('unit_vector', K, m, t)
        for shared in (False, True):
            if ('shared' if shared else 'public') in what:
                assert run_lookup(ctx, a, e['table'], m, t, shared, seed=K + shared) == e['lookup'], ('lookup', K, m, t, shared)


def check_beyond(make_ctx, m=3, t=1):
    """an index a with K <= a < K2 gives the unit vector of a cut to K rows: all zeros; and a table entry of zero"""
    ctx = make_ctx(P61)
    for K in (3, 5, 13):
        K2 = 1 << (K - 1).bit_length()
        a = list(range(K2))
        want = [[int(j == v) for j in range(K)] for v in a]
        assert run_unit_vectors(ctx, a, K, m, t, seed=7) == want
        assert run_from_bits(ctx, a, (K - 1).bit_length(), K, m, t, seed=7) == want
        table = [100 + 7 * j for j in range(K)]
        for shared in (False, True):
            assert run_lookup(ctx, a, table, m, t, shared, seed=9) == [table[v] if v < K else 0 for v in a]


@pytest.mark.parametrize('m,t', PARTIES)
def test_the_compositions_open_to_the_fixture(m, t):
    from unitvec_cpuctx import UnitvecCpuFieldContext
    check_fixture(UnitvecCpuFieldContext, m, t)


def test_indices_beyond_K_give_the_documented_result():
    from unitvec_cpuctx import UnitvecCpuFieldContext
    check_beyond(UnitvecCpuFieldContext)


WRONG = ('bits_lsb_first', 'roll_reversed', 'c_mod_K', 'table_wraps')


@pytest.mark.parametrize('wrong', WRONG)
def test_a_wrong_step_is_caught(wrong):
    from unitvec_cpuctx import UnitvecCpuFieldContext

    def make(p):
        ctx = UnitvecCpuFieldContext(p)
        assert getattr(ctx, wrong) is False
        setattr(ctx, wrong, True)
        return ctx

    seen = []
    for name, chk in (('fixture', lambda: check_fixture(make, 3, 1, ks=(2, 3, 5, 8, 13))), ('beyond', lambda: check_beyond(make))):
        try:
            chk()
        except AssertionError:
            seen.append(name)
    assert seen, 'the wrong step went unnoticed'
    # at a valid index the one term of the sum never reaches beyond K: only indices beyond K see a table that is not zero there
    assert ('fixture' in seen) == (wrong != 'table_wraps') and (wrong != 'table_wraps' or seen == ['beyond'])


@pytest.mark.parametrize('p,sec_param', [(P61, 30), (P31, 20)], ids=['2^61-1', '2^31-1'])
def test_the_compositions_run_on_the_supplier_alone(p, sec_param):
    from mpyc_amd import protocols
    from unitvec_cpuctx import UnitvecCpuFieldContext
    ctx, F, K, m, t = UnitvecCpuFieldContext(p), gf(p), 13, 3, 1
    R = protocols.Randomness(ctx, F, t, m, b'unit vectors end to end', sec_param=sec_param)
    rng = random.Random(p % 1000)
    a = list(range(K)) + [rng.randrange(K) for _ in range(8)]
    n = len(a)
    before = R.counter
    xs = _share(ctx, rng, a, t, m)
    got = columns(open_two_ways(ctx, protocols.unit_vectors(ctx, F, xs, K, t, R.rand_unit, sec_param=sec_param), t), K, n)
    assert got == [[int(j == v) for j in range(K)] for v in a]
    assert R.counter > before
    table = [rng.randrange(p) for _ in range(K)]
    pub = protocols.lookup(ctx, F, xs, ctx.from_ints(table), K, t, R.rand_unit, sec_param=sec_param)
    sh = protocols.lookup(ctx, F, xs, _share(ctx, rng, table, t, m), K, t, R.rand_unit, sec_param=sec_param)
    assert open_two_ways(ctx, pub, t) == open_two_ways(ctx, sh, t) == [table[v] for v in a]
    bits, Rs = R.rand_unit(10, 4, sec_param)
    assert set(open_two_ways(ctx, bits, t)) <= {0, 1} and len(bits[0]) == 40
    assert all(1 <= v <= 1 << sec_param for v in open_two_ways(ctx, Rs, t))
    u = protocols.random_unit_vectors(ctx, F, 10, 4, t, bits)
    cols = columns(open_two_ways(ctx, u, t), 16, 10)
    assert all(sorted(c) == [0] * 15 + [1] for c in cols)
    # the position is the value of the bits, row i the bit of weight 2^i
    b = open_two_ways(ctx, bits, t)
    assert [c.index(1) for c in cols] == [sum(b[i * 10 + e] << i for i in range(4)) for e in range(10)]
    assert open_two_ways(ctx, protocols.arg_index(ctx, u, 1, 16, 10), t) == [c.index(1) for c in cols]
    # too large a sec_param: the opened value would not fit the field
    with pytest.raises(ValueError):
        protocols.unit_vectors(ctx, F, xs, K, t, R.rand_unit, sec_param=p.bit_length() - 5)
    with pytest.raises(ValueError):
        protocols.lookup(ctx, F, xs, ctx.from_ints(table), K, t, R.rand_unit, sec_param=p.bit_length() - 5)
    protocols.unit_vectors(ctx, F, xs, K, t, R.rand_unit, sec_param=p.bit_length() - 6)           # the bound itself is met


def test_unit_refusals():
    from mpyc_amd import protocols
    from unitvec_cpuctx import UnitvecCpuFieldContext
    ctx, F = UnitvecCpuFieldContext(P61), gf(P61)
    rng = random.Random(5)
    xs = _share(ctx, rng, [0, 1, 2], 1, 3)
    draws = UnitDraws(ctx, 3, 1, 1)
    tab = ctx.from_ints([5, 6, 7])
    with pytest.raises(ValueError):
        protocols.unit_vectors(ctx, F, xs[:2], 3, 1, UnitDraws(ctx, 2, 1, 1))                   # m = 2t
    with pytest.raises(ValueError):
        protocols.lookup(ctx, F, xs, ctx.from_ints([5, 6]), 3, 1, draws)                        # a table of another length
    with pytest.raises(ValueError):
        protocols.lookup(ctx, F, xs, _share(ctx, rng, [5, 6, 7], 1, 3)[:2], 3, 1, draws)        # a party's table missing
    for bad in (lambda c, k, s: draws(c, k, s)[0],                                              # one sharing
                lambda c, k, s: (draws(c, k, s)[0], draws(c + 1, k, s)[1]),                     # too many values
                lambda c, k, s: (draws(c, k - 1, s)[0], draws(c, k, s)[1]),                     # too few bits
                lambda c, k, s: (draws(c, k, s)[0][:2], draws(c, k, s)[1])):                    # a party missing
        with pytest.raises(ValueError):
            protocols.unit_vectors(ctx, F, xs, 3, 1, bad)
    bs = _share(ctx, rng, bits_of([0, 1, 2], 2), 1, 3)
    with pytest.raises(ValueError):
        protocols.unit_vectors_from_bits(ctx, F, bs, 2, 5, 1)                                   # l < bit_length(K - 1)
    with pytest.raises(ValueError):
        protocols.demux(ctx, F, bs, 3, 3, 4, 1)                                                 # kbits is not bit_length(K - 1)
    ctxb = UnitvecCpuFieldContext(0x11b, True)
    with pytest.raises((ValueError, NotImplementedError)):
        protocols.unit_vectors(ctxb, None, [ctxb.from_ints([1])] * 3, 2, 1, draws)
    # K == 1: the public 1 and table[0], with no rounds and no draws
    assert run_unit_vectors(ctx, [0, 0, 0], 1, 3, 1) == [[1]] * 3
    assert run_lookup(ctx, [0, 0], [-9], 3, 1, False) == [-9, -9] and run_lookup(ctx, [0, 0], [-9], 3, 1, True) == [-9, -9]
    # the stand-in refuses what the engine refuses
    U, c, x = ctx.from_ints(list(range(8))), ctx.from_ints([1, 2]), ctx.from_ints([1, 0, 1, 1, 0, 1])
    for call in (lambda: ctx.unit_prod(x, U, 3), lambda: ctx.unit_prod(x, U, 4, xstride=0), lambda: ctx.unit_prod(x, U, 4, xstride=6),
                 lambda: ctx.unit_prod(x, U, 4, xoffset=5), lambda: ctx.unit_prod(x, U, 4, out=c), lambda: ctx.unit_roll(U, c, 2, 5),
                 lambda: ctx.unit_roll(U, c, 3, 8), lambda: ctx.unit_roll(U, x, 2, 4), lambda: ctx.unit_roll(U, c, 2, 3, out=U),
                 lambda: ctx.unit_dot(U, tab, 4), lambda: ctx.unit_dot(U, tab, 8, c=c, kbits=3), lambda: ctx.unit_dot(U, tab, 4, c=x, kbits=2),
                 lambda: ctx.unit_dot(U, U, 4, c=c, kbits=2), lambda: ctx.unit_dot(U, tab, 4, c=c, kbits=2, out=U)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: ctxb.unit_prod(x, U, 4), lambda: ctxb.unit_roll(U, c, 2, 3), lambda: ctxb.unit_dot(U, tab, 4, c=c, kbits=2)):
        with pytest.raises(NotImplementedError):
            call()
    big = 1 << (ctx.unit_dot_max_kbits() + 1)
    assert ctx.unit_dot_max_kbits() == 13
    with pytest.raises(NotImplementedError):
        ctx.unit_dot(ctx.from_ints([0] * big), tab, big, c=ctx.from_ints([0]), kbits=ctx.unit_dot_max_kbits() + 1)
    p = P61
    assert ctx.unit_prod(x, U, 4, xstride=2, xoffset=1).to_ints() == [0, 1, 0, 3, 0, 5, 0, 7]
    assert ctx.unit_roll(U, ctx.from_ints([1, p - 1]), 2, 3).to_ints() == [6, 5, 0, 7, 2, 1]    # (j - 1) mod 4; p - 1 = 2 mod 4
    assert ctx.unit_dot(U, tab, 4, c=ctx.from_ints([1, 3]), kbits=2).to_ints() == [(0 * 6 + 2 * 7 + 6 * 5) % p, (3 * 5 + 5 * 6 + 7 * 7) % p]
    assert ctx.unit_dot(U, ctx.from_ints([1, 2, 3, 4]), 4).to_ints() == [2 * 2 + 4 * 3 + 6 * 4, 1 + 3 * 2 + 5 * 3 + 7 * 4]
