"""CPU check of the hand-off tracker's second answer (mpyc_amd/csrc/handoff.hpp, plain C++): tests/handoff_fed_check.cpp
compiled with g++ and run -- does a launch read what the last launch on its stream wrote and kept: a fed launch, an unfed
one, a launch on another stream, outputs larger than the cache, lane eviction.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_handoff_tracker_fed_answer(tmp_path):
    exe = str(tmp_path / 'handoff_fed_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe,
                    os.path.join(TESTS, 'handoff_fed_check.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'handoff fed ok' in r.stdout, r.stdout + r.stderr
