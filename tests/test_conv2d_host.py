"""CPU checks of the secure 2-D convolution layers: the two C ABI entries of include/ffgpu_math.h exist in header, library and
binding and answer before any device work; the kernel's geometry (mpyc_amd/csrc/conv2d_geom.hpp) walked by
tests/conv2d_check.cpp with g++ against the plain seven-deep loop; the Python-integer stand-in (tests/conv2d_cpuctx.py) against
what the reference demo's own convolvetensor / maxpool opened (tests/golden/conv2d/conv2d.json); protocols.conv2d /
maxpool2x2 / relu / conv_layer / dense composed over the stand-in for (m, t) = (1, 0), (3, 1), (7, 3), opened two ways; the
deliberately wrong switches of the stand-in are caught; the refusals.  No GPU needed."""
import ctypes
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
GOLDEN = os.path.join(TESTS, 'golden', 'conv2d', 'conv2d.json')
ENTRIES = (('ffgm_conv2d', 13), ('ffgm_conv2d_plan', 9))
P_INT, P_FXP = 2**69 - 93, 2**46 - 21                                     # SecInt(37), SecFxp(10, 4)
INT_SHAPES = [[2, 3, 5, 6, 2, 3], [1, 2, 4, 5, 3, 4], [1, 1, 3, 7, 1, 5], [1, 2, 2, 6, 2, 6], [1, 1, 1, 1, 1, 1]]
PARTIES = [(1, 0), (3, 1), (7, 3)]
L_CMP = 37                                                                # 2^(l+1) + 2^(l+30) < p for both comparisons' fields


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def exact(e):
    """the integer correlation of a recorded case, before any reduction or truncation: Python integers from the formula"""
    k, r, m, n, v, s = e['shape']
    x, W, b = e['x'], e['W'], e['b']
    out = []
    for i in range(k):
        for j in range(v):
            for I in range(m):
                for J in range(n):
                    acc = b[j]
                    for l in range(r):
                        for di in range(s):
                            for dj in range(s):
                                row, col = I + di - (s - 1) // 2, J + dj - s // 2
                                if 0 <= row < m and 0 <= col < n:
                                    acc += x[((i * r + l) * m + row) * n + col] * W[((j * r + l) * s + di) * s + dj]
                    out.append(acc)
    return out


def check_truncated(got, e):
    """the two-part assertion for a probabilistic truncation: floor or floor + 1 of the exact value, and within one unit in the
    last place of what the reference opened"""
    f = e['f']
    for g, a, y in zip(got, exact(e), e['y']):
        assert g in (a >> f, (a >> f) + 1), (g, a)
        assert abs(g - y) <= 1, (g, y)


def test_conv2d_entries_in_header_library_and_binding():
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
    assert len(_ffi.EXPORTED) == 104 and _ffi.lib().ffgpu_abi_version() == 1


def test_statuses_before_device_work():
    """what both entries answer before they touch a device: the refusals of the issue's table that need no launch, the empty
    output, and the plan itself (host-only)"""
    from mpyc_amd import _ffi
    L = _ffi.lib()
    EINVAL, ENOTSUP, OK = _ffi.EINVAL, _ffi.ENOTSUP, _ffi.OK

    def mk(kind, modulus):
        h = ctypes.c_void_p()
        assert L.ffgpu_ctx_create(kind, _ffi.limbs(modulus, 3), 3, 0, ctypes.byref(h)) == 0
        return h
    h, hb = mk(_ffi.PRIME, 2**61 - 1), mk(_ffi.BINARY, 0x11b)
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255
    X, W, B, O = base, base + 8192, base + 16384, base + 32768
    arr = lambda *p: (ctypes.c_void_p * len(p))(*p)
    pl = _ffi.Conv2dPlanStruct()
    # the plan: shapes, grid and LDS of a small call and of the demo's layers
    assert L.ffgm_conv2d_plan(h, 1, 2, 5, 6, 3, 3, 1, ctypes.byref(pl)) == OK
    assert (pl.tile_rows, pl.tile_cols, pl.out_channels, pl.wide, pl.flush_rows) == (8, 16, 2, 0, 64)
    assert pl.in_channels_step == 2 and (pl.grid_x, pl.grid_y) == (2, 1) and pl.lds_bytes == 2 * (10 * 18 + 2 * 9) * 8
    assert L.ffgm_conv2d_plan(h, 64, 1, 28, 28, 32, 5, 3, ctypes.byref(pl)) == OK
    assert (pl.tile_rows, pl.tile_cols, pl.out_channels, pl.wide, pl.grid_x, pl.grid_y) == (16, 16, 4, 1, 64 * 4 * 8, 3)
    assert L.ffgm_conv2d_plan(h, 1, 32, 14, 14, 64, 5, 3, ctypes.byref(pl)) == OK
    assert (pl.tile_rows, pl.wide, pl.grid_x, pl.grid_y, pl.flush_rows) == (8, 0, 2 * 32, 3, 38) and pl.lds_bytes == 8 * (12 * 20 + 2 * 25) * 8
    assert L.ffgm_conv2d_plan(h, 0, 1, 4, 4, 1, 3, 1, ctypes.byref(pl)) == OK and (pl.grid_x, pl.grid_y) == (0, 0)
    for bad in ((1, 1, 4, 4, 1, 0, 1), (1, 1, 4, 4, 1, 17, 1), (1, 1, 4, 4, 1, 5, 1), (1, 0, 4, 4, 1, 3, 1), (1, 1, 4, 4, 1, 3, 0),
                (1 << 62, 4, 4, 4, 1, 3, 1)):
        assert L.ffgm_conv2d_plan(h, *bad, ctypes.byref(pl)) == EINVAL, bad
    assert L.ffgm_conv2d_plan(h, 1, 1, 4, 4, 1, 3, 1, None) == EINVAL and L.ffgm_conv2d_plan(None, 1, 1, 4, 4, 1, 3, 1, ctypes.byref(pl)) == EINVAL
    assert L.ffgm_conv2d_plan(hb, 1, 1, 4, 4, 1, 3, 1, ctypes.byref(pl)) == ENOTSUP
    assert L.ffgm_conv2d_plan(h, 1, 1, 4, 4, 1, 3, 65, ctypes.byref(pl)) == ENOTSUP
    assert L.ffgm_conv2d_plan(h, 1 << 40, 1, 16, 16, 4, 1, 1, ctypes.byref(pl)) == ENOTSUP          # 2^40 workgroups
    # the call
    one = (arr(X), arr(W), arr(B), arr(O))
    assert L.ffgm_conv2d(None, *one, 1, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(hb, *one, 1, 1, 1, 4, 4, 1, 3, None) == ENOTSUP
    assert L.ffgm_conv2d(h, *one, 65, 1, 1, 4, 4, 1, 3, None) == ENOTSUP
    assert L.ffgm_conv2d(h, *one, 0, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, None, None, None, None, 1, 0, 1, 4, 4, 1, 3, None) == OK                # empty: whatever the pointers
    assert L.ffgm_conv2d(h, None, None, None, None, 1, 1, 1, 4, 4, 0, 3, None) == OK
    assert L.ffgm_conv2d(h, None, None, None, None, 1, 0, 1, 4, 4, 1, 17, None) == EINVAL           # the counts are still checked
    for bad in ((1, 1, 4, 4, 1, 0), (1, 1, 4, 4, 1, 17), (1, 1, 4, 4, 1, 5), (1, 0, 4, 4, 1, 3), (1 << 62, 4, 4, 4, 1, 3)):
        assert L.ffgm_conv2d(h, *one, 1, *bad, None) == EINVAL, bad
    assert L.ffgm_conv2d(h, None, arr(W), arr(B), arr(O), 1, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, arr(X), arr(W), arr(B), None, 1, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, arr(X, None), arr(W, W), arr(B, B), arr(O, O + 4096), 2, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, arr(X, X), arr(W, W), arr(B, None), arr(O, O + 4096), 2, 1, 1, 4, 4, 1, 3, None) == EINVAL
    # overlaps: an output with x, W, b, or another sender's output (16 elements of 8 bytes each side)
    assert L.ffgm_conv2d(h, arr(X), arr(W), arr(B), arr(X + 120), 1, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, arr(X), arr(W), arr(B), arr(W - 120), 1, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, arr(X), arr(W), arr(B), arr(B), 1, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, arr(X, X), arr(W, W), arr(B, B), arr(O, O + 120), 2, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, arr(X, X), arr(W, W), arr(B, B), arr(O, X), 2, 1, 1, 4, 4, 1, 3, None) == EINVAL
    assert L.ffgm_conv2d(h, arr(X), arr(W), arr(B), arr(O), 1, 1 << 40, 1, 16, 16, 4, 1, None) == ENOTSUP
    for ctx in (h, hb):
        L.ffgpu_ctx_destroy(ctx)


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_conv2d_geometry_on_the_host(tmp_path):
    """one owner per output, every (output, term) once, zero halo, at most FLUSH unreduced terms for FLUSH = 32 and 192 and
    every s, the staged slots inside the reported LDS bytes, both tile shapes: 16 shapes x 2 tile shapes x 2 bounds x 2 slots"""
    exe = str(tmp_path / 'conv2d_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'conv2d_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'conv2d ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) == 16 * 2 * 2 * 2


# ---- the fixture and the stand-in -------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_issue_asks_for():
    doc = golden()
    ints = [e for e in doc['conv'] if e['f'] == 0]
    fxps = [e for e in doc['conv'] if e['f']]
    assert [e['shape'] for e in ints] == INT_SHAPES and [e['shape'] for e in fxps] == INT_SHAPES[:2]
    assert all(e['p'] == P_INT and e['type'] == 'SecInt37' for e in ints) and all(e['p'] == P_FXP and e['f'] == 4 for e in fxps)
    for e in doc['conv']:
        k, r, m, n, v, s = e['shape']
        assert (len(e['x']), len(e['W']), len(e['b']), len(e['y'])) == (k * r * m * n, v * r * s * s, v, k * v * m * n)
    for e in ints:                                                       # the formula of the issue IS the reference, even s included
        assert exact(e) == e['y'], e['shape']
    for e in fxps:
        check_truncated(e['y'], e)
    lay = doc['layer']
    assert lay['shape'] == [1, 2, 6, 6, 2, 3] and lay['p'] == P_INT and exact({**lay, 'y': None}) == lay['conv']
    c, pool = lay['conv'], []
    ties = 0
    for pl in range(2):
        for I in range(3):
            for J in range(3):
                sq = sorted(c[(pl * 6 + 2 * I + a) * 6 + 2 * J + b] for a in range(2) for b in range(2))
                pool.append(sq[-1])
                ties += sq[-1] == sq[-2]
    assert pool == lay['pool'] and lay['relu'] == [max(q, 0) for q in pool]
    assert ties == lay['ties'] >= 1 and min(pool) < 0 < max(pool), 'both signs and a tie before the ReLU'


def test_stand_in_is_the_reference():
    from conv2d_cpuctx import Conv2dCpuFieldContext
    ctx = Conv2dCpuFieldContext(P_INT)
    for e in golden()['conv']:
        if e['f']:
            continue
        k, r, m, n, v, s = e['shape']
        x, W, b = (ctx.from_ints([q % P_INT for q in e[key]]) for key in 'xWb')
        got = ctx.conv2d([x, x], [W, W], [b, b], k, r, m, n, v, s)
        assert all([_signed(q, P_INT) for q in o.to_ints()] == e['y'] for o in got), e['shape']
        nb = ctx.conv2d([x], [W], None, k, r, m, n, v, s)[0].to_ints()
        assert [_signed(q, P_INT) for q in nb] == [y - e['b'][(i // (m * n)) % v] for i, y in enumerate(e['y'])]


# ---- the protocols on the stand-in ------------------------------------------------------------------------------------------------
def shares_of(ctx, rng, vals, t, m):
    return _share(ctx, rng, [q % ctx.modulus for q in vals], t, m)


def run_conv2d(ctx, protocols, e, m, t, public_w=False, rand_trunc=None, seed=1):
    p = ctx.modulus
    rng = random.Random(seed)
    k, r, mm, n, v, s = e['shape']
    xs = shares_of(ctx, rng, e['x'], t, m)
    ws = ctx.from_ints([q % p for q in e['W']]) if public_w else shares_of(ctx, rng, e['W'], t, m)
    bs = shares_of(ctx, rng, e['b'], t, m)
    before = [a.to_ints() for a in xs]
    got = protocols.conv2d(ctx, gf(p), xs, ws, bs, k, r, mm, n, v, s, t, f=e['f'], rand_trunc=rand_trunc)
    assert len(got) == m and [a.to_ints() for a in xs] == before, 'an input of conv2d was written'
    return [_signed(q, p) for q in open_two_ways(ctx, got, t)]


def check_conv2d(make_ctx, protocols, m, t):
    for e in golden()['conv']:
        ctx = make_ctx(e['p'])
        R = protocols.Randomness(ctx, gf(e['p']), t, m, b'conv2d host %d %d' % (m, t))
        for public_w in (False, True):
            got = run_conv2d(ctx, protocols, e, m, t, public_w, R.rand_trunc, seed=m + 7 * public_w)
            if e['f']:
                check_truncated(got, e)
            else:
                assert got == e['y'], (e['shape'], m, t, public_w)


def check_layer(make_ctx, protocols, m, t):
    """maxpool2x2 and relu on the recorded conv output, and conv_layer as a whole, against the reference's pool and relu"""
    lay = golden()['layer']
    p = lay['p']
    ctx, F = make_ctx(p), gf(p)
    k, r, mm, n, v, s = lay['shape']
    R = protocols.Randomness(ctx, F, t, m, b'conv layer host %d %d' % (m, t))
    rand = R.rand_compare(L_CMP)
    rng = random.Random(3 * m + t)
    pool = protocols.maxpool2x2(ctx, F, shares_of(ctx, rng, lay['conv'], t, m), k * v, mm, n, t, L_CMP, rand)
    assert [_signed(q, p) for q in open_two_ways(ctx, pool, t)] == lay['pool']
    relu = protocols.relu(ctx, F, pool, t, L_CMP, rand)
    assert [_signed(q, p) for q in open_two_ways(ctx, relu, t)] == lay['relu']
    xs, ws, bs = (shares_of(ctx, rng, lay[key], t, m) for key in 'xWb')
    out = protocols.conv_layer(ctx, F, xs, ws, bs, k, r, mm, n, v, s, t, L_CMP, rand)
    assert [_signed(q, p) for q in open_two_ways(ctx, out, t)] == lay['relu']


def check_dense(make_ctx, protocols, m, t):
    """x @ W + b on small integers, shared and public W and b; the fixed-point variant with the two-part assertion"""
    for p, f in ((P_INT, 0), (P_FXP, 4)):
        ctx, F = make_ctx(p), gf(p)
        R = protocols.Randomness(ctx, F, t, m, b'dense host %d %d' % (m, t))
        rng = random.Random(5 * m + f)
        M, K, N = 3, 5, 4
        x, W, b = ([rng.randint(-40, 40) for _ in range(c)] for c in (M * K, K * N, N))
        prod = [sum(x[i * K + q] * W[q * N + j] for q in range(K)) for i in range(M) for j in range(N)]
        for public in (False, True):
            ws = ctx.from_ints([q % p for q in W]) if public else shares_of(ctx, rng, W, t, m)
            bs = ctx.from_ints([q % p for q in b]) if public else shares_of(ctx, rng, b, t, m)
            got = protocols.dense(ctx, F, shares_of(ctx, rng, x, t, m), ws, bs, M, K, N, t, f=f, rand_trunc=R.rand_trunc)
            got = [_signed(q, p) for q in open_two_ways(ctx, got, t)]
            for i, (g, a) in enumerate(zip(got, prod)):
                assert g - b[i % N] in ((a >> f, (a >> f) + 1) if f else (a,)), (i, g, a, public)
        nob = protocols.dense(ctx, F, shares_of(ctx, rng, x, t, m), shares_of(ctx, rng, W, t, m), None, M, K, N, t)
        assert [_signed(q, p) for q in open_two_ways(ctx, nob, t)] == prod


@pytest.mark.parametrize('m,t', PARTIES)
def test_conv2d_opens_to_the_fixture(m, t):
    from mpyc_amd import protocols
    from conv2d_cpuctx import Conv2dCpuFieldContext
    check_conv2d(Conv2dCpuFieldContext, protocols, m, t)


@pytest.mark.parametrize('m,t', PARTIES)
def test_layer_opens_to_the_fixture(m, t):
    from mpyc_amd import protocols
    from conv2d_cpuctx import Conv2dCpuFieldContext
    check_layer(Conv2dCpuFieldContext, protocols, m, t)


@pytest.mark.parametrize('m,t', PARTIES)
def test_dense_is_the_product_plus_the_bias(m, t):
    from mpyc_amd import protocols
    from conv2d_cpuctx import Conv2dCpuFieldContext
    check_dense(Conv2dCpuFieldContext, protocols, m, t)


@pytest.mark.parametrize('wrong', ['col_off_is_row_off', 'without_bias'])
def test_a_wrong_step_is_caught(wrong):
    from mpyc_amd import protocols
    from conv2d_cpuctx import Conv2dCpuFieldContext

    def make(p):
        ctx = Conv2dCpuFieldContext(p)
        assert getattr(ctx, wrong) is False
        setattr(ctx, wrong, True)
        return ctx
    with pytest.raises(AssertionError):
        check_conv2d(make, protocols, 3, 1)
    if wrong == 'col_off_is_row_off':                                    # odd s alone does not tell the two offsets apart
        e = golden()['conv'][0]
        assert e['shape'][5] == 3 and run_conv2d(make(e['p']), protocols, e, 3, 1) == e['y']


def test_refusals():
    from mpyc_amd import protocols
    from conv2d_cpuctx import Conv2dCpuFieldContext
    p = P_INT
    ctx, F = Conv2dCpuFieldContext(p), gf(p)
    rng = random.Random(9)
    x, W, b = shares_of(ctx, rng, range(16), 1, 3), shares_of(ctx, rng, range(9), 1, 3), shares_of(ctx, rng, [1], 1, 3)
    assert len(protocols.conv2d(ctx, F, x, W, b, 1, 1, 4, 4, 1, 3, 1)) == 3
    with pytest.raises(ValueError):
        protocols.conv2d(ctx, F, x[:2], W[:2], b[:2], 1, 1, 4, 4, 1, 3, 1)            # m = 2t
    with pytest.raises(ValueError):
        protocols.conv2d(ctx, F, x, W[:2], b, 1, 1, 4, 4, 1, 3, 1)                    # W for two of three parties
    with pytest.raises(ValueError):
        protocols.conv2d(ctx, F, x, W, b, 1, 1, 4, 4, 1, 3, 1, f=4)                   # a truncation without its randomness
    for bad in ((1, 1, 4, 4, 1, 5), (1, 1, 4, 4, 1, 0), (1, 1, 4, 4, 1, 17), (1, 1, 4, 4, 2, 3), (1, 2, 4, 4, 1, 3), (2, 1, 4, 4, 1, 3)):
        with pytest.raises(ValueError):
            protocols.conv2d(ctx, F, x, W, b, *bad, 1)
    R = protocols.Randomness(ctx, F, 1, 3, b'refusals')
    for mm, n in ((3, 4), (4, 3)):
        with pytest.raises(ValueError):
            protocols.maxpool2x2(ctx, F, shares_of(ctx, rng, range(12), 1, 3), 1, mm, n, 1, L_CMP, R.rand_compare(L_CMP))
    a = [ctx.from_ints(list(range(16)))]
    for call in (lambda: ctx.conv2d([], [], None, 1, 1, 4, 4, 1, 3), lambda: ctx.conv2d(a, a, None, 1, 1, 4, 4, 1, 3),
                 lambda: ctx.conv2d(a, [a[0], a[0]], None, 1, 1, 4, 4, 1, 1), lambda: ctx.conv2d(a, a, None, 1, 1, 4, 4, 1, 1, outs=[a[0], a[0]]),
                 lambda: ctx.conv2d_plan(1, 1, 4, 4, 1, 5), lambda: ctx.conv2d_plan(1, 1, 4, 4, 1, 3, nsend=0)):
        with pytest.raises(ValueError):
            call()
    ctxb = Conv2dCpuFieldContext(0x11b, True)
    for call in (lambda: ctxb.conv2d(a, a, None, 1, 1, 4, 4, 1, 1), lambda: ctx.conv2d(a * 65, a * 65, None, 1, 1, 4, 4, 1, 1),
                 lambda: ctx.conv2d_plan(1, 1, 4, 4, 1, 3, nsend=65)):
        with pytest.raises(NotImplementedError):
            call()
    w1 = [ctx.from_ints([3])]
    assert ctx.conv2d(a, w1, None, 1, 1, 4, 4, 1, 1)[0].to_ints() == [3 * q for q in range(16)]
    assert ctx.conv2d([ctx.empty(0)], a, None, 0, 1, 4, 4, 16, 1)[0].n == 0
