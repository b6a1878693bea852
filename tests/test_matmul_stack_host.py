"""CPU checks of the stacked matrix product: the geometry of the stack kernels (mpyc_amd/csrc/matmul_stack_geom.hpp)
walked by tests/matmul_stack_check.cpp with g++; the C ABI entry in header, library and binding, and every argument
rule it answers before any device work; the mirror's stack branch on contexts without a library handle
(tests/cpuctx.py), against NumPy's object matmul.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_stack_plan_on_the_host(tmp_path):
    """every (M, K, N) up to 41^3, batches around every P boundary, every element width, several CU counts: each output
    owned exactly once, LDS inside the budget, grids inside limits, packed never above 256 outputs"""
    exe = str(tmp_path / 'matmul_stack_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Wno-unknown-pragmas', '-Werror', '-o', exe,
                    os.path.join(TESTS, 'matmul_stack_check.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'matmul_stack ok' in r.stdout, r.stdout + r.stderr


@pytest.fixture(scope='module')
def L():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi.lib()


def test_entry_in_header_library_and_binding(L):
    from mpyc_amd import _ffi
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'int\s+ffgpu_matmul_stack\s*\(([^)]*)\)', hdr)
    assert m, 'ffgpu_matmul_stack is not declared in include/ffgpu.h'
    params = [p.strip() for p in m.group(1).split(',')]
    assert len(params) == 15 and params[0].startswith('ffgpu_ctx*') and params[14].startswith('void*'), params
    assert [p.split()[0] for p in params[1:14]] == ['const', 'size_t', 'size_t', 'const', 'size_t', 'size_t', 'void*',
                                                    'size_t', 'size_t', 'size_t', 'size_t', 'size_t', 'size_t'], params
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r' T ffgpu_matmul_stack\b', out), 'ffgpu_matmul_stack is not exported by libffgpu.so'
    assert 'ffgpu_matmul_stack' in _ffi.EXPORTED and len(_ffi._SIGS['ffgpu_matmul_stack']) == 15
    assert L.ffgpu_abi_version() == 1                                        # the change is additive


def _ctx(L, kind, modulus):
    from mpyc_amd import _ffi
    h = ctypes.c_void_p()
    assert L.ffgpu_ctx_create(kind, _ffi.limbs(modulus, 3), 3, 0, ctypes.byref(h)) == 0
    return h


def test_argument_rules_before_any_device_work(L):
    """every rule of include/ffgpu.h for ffgpu_matmul_stack, answered without a compute call (so without a GPU)"""
    from mpyc_amd import _ffi
    OK, EINVAL = _ffi.OK, _ffi.EINVAL
    f = L.ffgpu_matmul_stack
    assert f(None, None, 0, 0, None, 0, 0, None, 0, 0, 0, 0, 0, 0, None) == EINVAL       # no context
    h = _ctx(L, _ffi.PRIME, 2**61 - 1)
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255
    A, B, C = base, base + 16384, base + 32768
    eb = 8
    # nothing to do: OK before anything is looked at
    assert f(h, None, 0, 0, None, 0, 0, None, 0, 0, 4, 4, 4, 0, None) == OK              # batch == 0
    assert f(h, None, 0, 0, None, 0, 0, None, 0, 0, 0, 4, 4, 8, None) == OK              # M == 0
    assert f(h, None, 0, 0, None, 0, 0, None, 0, 0, 4, 4, 0, 8, None) == OK              # N == 0
    # a correct call for reference: 8 x (4x4 @ 4x4), lda 4, strides 16 -- only the refused variants below are made
    good = dict(A=A, lda=4, sa=16, B=B, ldb=4, sb=16, C=C, ldc=4, sc=16, M=4, K=4, N=4, batch=8)

    def call(**kw):
        a = dict(good, **kw)
        return f(h, a['A'], a['lda'], a['sa'], a['B'], a['ldb'], a['sb'], a['C'], a['ldc'], a['sc'], a['M'], a['K'], a['N'],
                 a['batch'], None)
    assert call(A=None) == EINVAL and call(B=None) == EINVAL and call(C=None) == EINVAL
    assert call(lda=3) == EINVAL and call(ldb=3) == EINVAL and call(ldc=3) == EINVAL    # leading dimension too short
    assert call(sa=15) == EINVAL and call(sb=15) == EINVAL                              # non-zero stride < a matrix
    assert call(lda=6, sa=21) == EINVAL                                                 # a matrix spans 3 * 6 + 4 = 22
    assert call(sc=15) == EINVAL and call(sc=0) == EINVAL                               # stride_c < a matrix; zero, batch > 1
    assert call(ldc=6, sc=21) == EINVAL
    assert call(sc=1, batch=1) == EINVAL                                                # non-zero and too small, any batch
    big = 1 << 62
    assert call(sa=big) == EINVAL and call(sb=big) == EINVAL and call(sc=big) == EINVAL  # byte ranges overflow
    assert call(batch=big, sa=0, sb=0) == EINVAL
    assert call(lda=big) == EINVAL and call(ldc=big) == EINVAL
    assert call(M=1 << 30) == EINVAL and call(N=1 << 30) == EINVAL and call(K=1 << 30) == EINVAL
    # C overlaps A or B: its first byte, its last byte, with strides (the range is the whole stack's)
    assert call(C=A) == EINVAL and call(C=B) == EINVAL
    assert call(C=A + (8 * 16 - 1) * eb) == EINVAL                                      # C starts at A's last element
    assert call(C=A - (8 * 16 - 1) * eb) == EINVAL                                      # C's last element is A's first
    assert call(C=B + 15 * eb, sb=0) == EINVAL                                          # C starts inside the ONE matrix of B
    assert call(C=A + 40 * eb, sa=32) == EINVAL                                         # inside A's strided range
    # more workgroups than a grid holds: 2^31 matrices of 17 x 16 outputs (tiled, one tile each); both operands shared and
    # C far away, so that every other rule is met
    assert call(M=17, N=16, sa=0, sb=0, sc=272, batch=1 << 31, lda=4, ldb=16, ldc=16, C=base + (1 << 50)) == EINVAL
    L.ffgpu_ctx_destroy(h)


MODS = [('P61', 2**61 - 1, False), ('P13', 13, False), ('P128', 2**128 - 173, False), ('GF2_8', 0x11b, True)]


@pytest.mark.parametrize('name,modulus,binary', MODS, ids=[m[0] for m in MODS])
def test_mirror_stack_branch_without_kernels(monkeypatch, name, modulus, binary):
    """tests/cpuctx.py has no library handle: stacks of matrices must keep going through the per-matrix loop
    (_matmul_per_matrix) and give NumPy's object matmul, for every operand form, with today's shapes and errors"""
    from cpuctx import use_cpu_contexts
    import mpyc_amd.finfields as gff
    from mpyc_amd import gfpx
    from oracle import pyoracle as po
    use_cpu_contexts(monkeypatch)
    monkeypatch.setattr(gff, '_ctx_cache', {})
    gff._pGF.cache_clear()
    try:
        F = gff.GF(gfpx.BinaryPolynomial(modulus)) if binary else gff.GF(modulus)
        order = 256 if binary else modulus
        rng = np.random.default_rng(5)
        calls = []
        real = gff._matmul_per_matrix
        monkeypatch.setattr(gff, '_matmul_per_matrix', lambda *a: calls.append(1) or real(*a))
        pf = po.Field(modulus, binary)

        def rand(*shape):
            return np.array([int(rng.integers(0, min(order, 2**62))) ** 2 % order for _ in range(int(np.prod(shape)))],
                            dtype=object).reshape(shape)

        def want(a, b):
            if not binary:
                return np.matmul(a, b) % modulus
            a2 = a.reshape(1, -1) if a.ndim == 1 else a
            b2 = b.reshape(-1, 1) if b.ndim == 1 else b
            batch = np.broadcast_shapes(a2.shape[:-2], b2.shape[:-2])
            ab = np.broadcast_to(a2, batch + a2.shape[-2:]).reshape((-1,) + a2.shape[-2:])
            bb = np.broadcast_to(b2, batch + b2.shape[-2:]).reshape((-1,) + b2.shape[-2:])
            out = np.array([po.matmul(pf, x.tolist(), y.tolist()) for x, y in zip(ab, bb)], dtype=object)
            out = out.reshape(batch + (a2.shape[-2], b2.shape[-1]))
            if a.ndim == 1:
                out = out.reshape(out.shape[:-2] + out.shape[-1:])
            elif b.ndim == 1:
                out = out.reshape(out.shape[:-1])
            return out

        def ints(x):
            return np.array([int(v) for v in np.asarray(x.value).reshape(-1)], dtype=object).reshape(x.shape)

        forms = [((5, 2, 3), (5, 3, 4)), ((2, 3), (5, 3, 4)), ((5, 2, 3), (3, 4)), ((3, 1, 2, 3), (1, 2, 3, 4)),
                 ((3,), (5, 3, 4)), ((5, 2, 3), (3,)), ((2, 5, 2, 3), (5, 3, 4)), ((1, 2, 3), (1, 3, 4))]
        for sa, sb in forms:
            a, b = rand(*sa), rand(*sb)
            fa, fb = F.array(a), F.array(b)
            assert fa.ctx._h is None
            got = fa @ fb
            w = want(a, b)
            assert got.shape == w.shape, (sa, sb)
            assert (ints(got) == w).all(), (sa, sb)
            assert (ints(np.matmul(fa, fb)) == w).all(), (sa, sb)
        a, b = rand(4, 3, 2), rand(4, 3, 5)                  # transposed views of the last two axes
        got = F.array(a).transpose(0, 2, 1) @ F.array(b)
        assert (ints(got) == want(a.transpose(0, 2, 1), b)).all()
        n = len(calls)
        assert n >= len(forms) + 1
        e = F.array(np.zeros((0, 2, 3), dtype=object)) @ F.array(rand(3, 4))          # an empty batch
        assert e.shape == (0, 2, 4)
        z = F.array(np.zeros((5, 2, 0), dtype=object)) @ F.array(np.zeros((5, 0, 4), dtype=object))   # K == 0: zeros
        assert z.shape == (5, 2, 4) and not any(int(v) for v in np.asarray(z.value).reshape(-1))
        with pytest.raises(ValueError):
            F.array(rand(5, 2, 3)) @ F.array(rand(5, 4, 4))
        with pytest.raises(ValueError):
            F.array(rand(5, 2, 3)) @ F.array(rand(4, 3, 4))                           # batches that do not broadcast
    finally:
        gff._pGF.cache_clear()
