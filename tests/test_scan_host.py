"""CPU checks of the scan / axis-reduction feature: the three C ABI entries exist in header, library and binding; the
geometry and index arithmetic of the kernels (mpyc_amd/csrc/scan_geom.hpp) walked by tests/scan_check.cpp with g++; the
mirror on a context without a library handle (tests/cpuctx.py) still takes the composed helpers and agrees with Python
integers, the new prod(initial=, keepdims=) included.  No GPU needed."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def test_scan_entries_in_header_library_and_binding():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    for name, ret, nparams in (('ffgpu_scan', 'int', 11), ('ffgpu_axis_reduce', 'int', 10),
                               ('ffgpu_scan_workspace_bytes', 'size_t', 4)):
        m = re.search(ret + r'\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, f'{name} is not declared in include/ffgpu.h'
        params = [p.strip() for p in m.group(1).split(',')]
        assert len(params) == nparams and params[0].startswith('ffgpu_ctx*'), params
        assert re.search(r' T ' + name + r'\b', out), f'{name} is not exported by libffgpu.so'
        assert name in _ffi.EXPORTED and len(_ffi._SIGS[name]) == nparams
    L = _ffi.lib()
    # no context: refused before anything is touched
    assert L.ffgpu_scan(None, 0, None, None, 1, 1, 1, 0, None, 0, None) == _ffi.EINVAL
    assert L.ffgpu_axis_reduce(None, 0, None, None, 1, 1, 1, None, 0, None) == _ffi.EINVAL
    assert L.ffgpu_scan_workspace_bytes(None, 1, 1, 1) == 0


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_scan_index_arithmetic_on_the_host(tmp_path):
    """(outer, k, inner) up to 40 x 300 x 40, every element size, both geometries, packs and single elements, six tile
    sizes: ownership, tile order, workspace bounds, and the three passes against a plain loop"""
    exe = str(tmp_path / 'scan_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Wno-unknown-pragmas', '-Werror', '-o', exe,
                    os.path.join(TESTS, 'scan_check.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'scan ok' in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize('modulus,binary', [(2**61 - 1, False), (2**127 - 1, False), (0x11b, True)], ids=hex)
def test_mirror_without_kernels_keeps_the_composed_helpers(monkeypatch, modulus, binary):
    """tests/cpuctx.py has no library handle: scans go through _scan_hillis_steele, products through _prod_halving, and give
    what Python integers give"""
    from cpuctx import use_cpu_contexts
    import mpyc_amd.finfields as gff
    from mpyc_amd import gfpx
    from oracle import pyoracle as po
    use_cpu_contexts(monkeypatch)
    monkeypatch.setattr(gff, '_ctx_cache', {})
    gff._pGF.cache_clear()
    try:
        F = gff.GF(gfpx.BinaryPolynomial(modulus)) if binary else gff.GF(modulus)
        order = 1 << (modulus.bit_length() - 1) if binary else modulus
        if binary:
            add, mul = (lambda x, y: x ^ y), (lambda x, y: po.clmod(po.clmul(x, y), modulus))
        else:
            add, mul = (lambda x, y: (x + y) % modulus), (lambda x, y: x * y % modulus)
        rs = np.random.default_rng(5)
        shape = (3, 4, 5)
        vals = [int.from_bytes(rs.bytes(20), 'little') % order for _ in range(60)]
        vals[7], vals[11] = 1, order - 1
        ref = np.array(vals, dtype=object).reshape(shape)
        a = F.array(ref.copy())
        assert a.ctx._h is None
        calls = {'scan': 0, 'prod': 0}
        real_scan, real_prod = gff._scan_hillis_steele, gff.FieldArray._prod_halving
        monkeypatch.setattr(gff, '_scan_hillis_steele', lambda *args: calls.__setitem__('scan', calls['scan'] + 1) or real_scan(*args))
        monkeypatch.setattr(gff.FieldArray, '_prod_halving',
                            lambda self, axis=None: calls.__setitem__('prod', calls['prod'] + 1) or real_prod(self, axis))
        ints = lambda arr: [int(x) for x in np.asarray(arr.value).reshape(-1)]

        def acc(axis, op, wi=None):
            r = np.apply_along_axis(lambda v: np.array(([wi] if wi is not None else []) + list(itertools.accumulate(v, op)),
                                                       dtype=object), axis, ref)
            return [int(v) for v in r.reshape(-1)]

        def red(axis, op):
            r = np.apply_along_axis(lambda v: np.array([list(itertools.accumulate(v, op))[-1]], dtype=object), axis, ref)
            return [int(v) for v in r.reshape(-1)]

        for axis in (0, 1, 2):
            assert ints(np.cumsum(a, axis=axis)) == acc(axis, add)
            assert ints(np.cumprod(a, axis=axis)) == acc(axis, mul)
            assert ints(np.multiply.accumulate(a, axis=axis)) == acc(axis, mul)
            assert ints(np.cumulative_sum(a, axis=axis, include_initial=True)) == acc(axis, add, wi=0)
            assert ints(a.prod(axis=axis)) == red(axis, mul)
            assert ints(a.sum(axis=axis)) == red(axis, add)
            pk = a.prod(axis=axis, keepdims=True, initial=3)                 # used to raise NotImplementedError
            assert pk.shape == tuple(1 if d == axis else s for d, s in enumerate(shape))
            assert ints(pk) == [mul(x, 3) for x in red(axis, mul)]
        assert calls['scan'] == 12 and calls['prod'] == 6
        flat = [int(v) for v in ref.reshape(-1)]
        total = list(itertools.accumulate(flat, mul))[-1]
        sval = lambda x: int(x) if binary else int(x) % modulus
        assert sval(a.prod()) == total and sval(a.prod(initial=7)) == mul(total, 7)
        allp = a.prod(keepdims=True)
        assert allp.shape == (1, 1, 1) and ints(allp) == [total]
        assert ints(np.cumsum(a)) == list(itertools.accumulate(flat, add))
    finally:
        gff._pGF.cache_clear()
