"""CPU checks of the convolution feature: the C ABI entry exists in header, library and binding; the composed route
stays reachable for a context that cannot run the kernel; the kernel's tile / window index arithmetic
(mpyc_amd/csrc/convolve_geom.hpp) walked by tests/convolve_check.cpp with g++.  No GPU needed."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def test_convolve_entry_in_header_library_and_binding():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'int\s+ffgpu_convolve\s*\(([^)]*)\)', hdr)
    assert m, 'ffgpu_convolve is not declared in include/ffgpu.h'
    params = [p.strip() for p in m.group(1).split(',')]
    assert len(params) == 7 and params[0].startswith('ffgpu_ctx*') and params[2].startswith('size_t') \
        and params[4].startswith('size_t') and params[6].startswith('void*'), params
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r' T ffgpu_convolve\b', out), 'ffgpu_convolve is not exported by libffgpu.so'
    assert 'ffgpu_convolve' in _ffi.EXPORTED and len(_ffi._SIGS['ffgpu_convolve']) == 7
    fn = _ffi.lib().ffgpu_convolve
    assert fn(None, None, 0, None, 0, None, None) == _ffi.EINVAL        # no context: refused before anything is touched


@pytest.mark.parametrize('name', ['P61', 'GF2_8'])
def test_convolve_without_kernel_keeps_the_composed_route(monkeypatch, name):
    """tests/cpuctx.py has no library handle and no convolve of its own: np.convolve on its arrays must still give the
    reference's values (tests/golden/npfuncs.json), through the Toeplitz product."""
    from cpuctx import use_cpu_contexts
    import mpyc_amd.finfields as gff
    from mpyc_amd import gfpx
    use_cpu_contexts(monkeypatch)
    monkeypatch.setattr(gff, '_ctx_cache', {})
    gff._pGF.cache_clear()
    try:
        c = json.load(open(os.path.join(TESTS, 'golden', 'npfuncs.json')))[name]
        modulus = int(c['modulus'], 16)
        F = gff.GF(gfpx.BinaryPolynomial(modulus)) if c['binary'] else gff.GF(modulus)
        red = lambda x: int(x, 16) if c['binary'] else int(x, 16) % modulus
        L = lambda key: [red(x) for x in c[key]]
        ints = lambda arr: [int(x) for x in np.asarray(arr.value).reshape(-1)]
        a, v = F.array(L('a')), F.array(L('v'))
        assert a.ctx._h is None
        calls = []
        real = gff._convolve_toeplitz
        monkeypatch.setattr(gff, '_convolve_toeplitz', lambda *args: calls.append(1) or real(*args))
        assert ints(np.convolve(a, v)) == L('conv_full')
        assert ints(np.convolve(a, v, 'same')) == L('conv_same')
        assert ints(np.convolve(a, v, 'valid')) == L('conv_valid')
        assert ints(np.convolve(v, a)) == L('conv_swapped')
        assert len(calls) == 4
        if not c['binary']:
            assert ints(np.polymul(a, v)) == L('conv_full')
        with pytest.raises(ValueError):
            np.convolve(a, v, 'nonsense')
        with pytest.raises(ValueError):
            np.convolve(a, F.array([]))
    finally:
        gff._pGF.cache_clear()


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_convolve_index_arithmetic_on_the_host(tmp_path):
    """every (na, nv) up to 300 x 300 through the kernel's tile / chunk / tap-group walk, flush cadence included"""
    exe = str(tmp_path / 'convolve_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Wno-unknown-pragmas', '-Werror', '-o', exe,
                    os.path.join(TESTS, 'convolve_check.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'convolve ok' in r.stdout, r.stdout + r.stderr
