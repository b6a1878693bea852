"""CPU checks of the base of the geometry headers (mpyc_amd/csrc/geom.hpp): the size guard, the flat, rows, stream and
reversed-row plans and the pair split, walked by tests/geom_check.cpp with g++ against brute-force enumeration -- once plainly,
once stand-alone under the address and undefined-behaviour sanitizers; and the names the header replaced stay gone from the
sources.  No GPU needed."""
import glob
import os
import re
import shutil
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), 'mpyc_amd', 'csrc')


def build_and_run(tmp_path, name, opt, flags):
    exe = str(tmp_path / name)
    cc = subprocess.run(['g++', opt, '-std=c++17', '-Wall', '-Wextra', '-Werror', *flags, '-o', exe, os.path.join(TESTS, 'geom_check.cpp')],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'geom ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ''                                    # (a sanitizer report goes there)
    # 10 plans' worth of cases per element size and alignment: 201 flat, 201 stream, 201 * 24 rows, 10 * 64 * 2 reversed
    assert int(r.stdout.split()[-1]) > 10 * (201 + 201 + 201 * 24 + 1280)


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_geom_on_the_host(tmp_path):
    build_and_run(tmp_path, 'geom_check', '-O2', [])


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_geom_on_the_host_under_sanitizers(tmp_path):
    """the same program, stand-alone, built with the address and undefined-behaviour sanitizers and run as it is"""
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = subprocess.run(['g++', *flags, '-x', 'c++', '-', '-o', str(tmp_path / 'probe')], input='int main() { return 0; }\n',
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip('the sanitizer runtime does not link here')
    build_and_run(tmp_path, 'geom_check_san', '-O1', ['-g', *flags])


def test_one_base_under_the_geometry_headers():
    """every *_geom.hpp takes the macro pair from geom.hpp, and a family's header includes another family's only where it builds
    on it: find on the tournament's round, the binary sign on the symbols of the zero test"""
    headers = sorted(glob.glob(os.path.join(CSRC, '*_geom.hpp')))
    assert len(headers) == 17
    others = {}
    for path in headers:
        src = open(path).read()
        incs = re.findall(r'#include "(\w+\.hpp)"', src)
        assert 'geom.hpp' in incs or any(i.endswith('_geom.hpp') for i in incs), path
        assert not re.search(r'#\s*define\s+FF\w+_(HD|CX)\b', src), path
        others[os.path.basename(path)] = [i for i in incs if i != 'geom.hpp']
    assert {k: v for k, v in others.items() if v} == {'find_geom.hpp': ['tour_geom.hpp'], 'bsgn_geom.hpp': ['iszero_geom.hpp']}
