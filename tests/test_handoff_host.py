"""CPU check of the hand-off tracker (mpyc_amd/csrc/handoff.hpp, plain C++): tests/handoff_check.cpp compiled with g++ and
run -- the overlap rule, the prediction per stream and per producer kind, the size cap, the lane reuse.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_handoff_tracker_rules(tmp_path):
    exe = str(tmp_path / 'handoff_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe,
                    os.path.join(TESTS, 'handoff_check.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'handoff ok' in r.stdout, r.stdout + r.stderr
