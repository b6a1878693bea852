"""CPU checks of the two plain headers under the C boundary: the 192-bit host integer (mpyc_amd/csrc/hostint.hpp) against
Python integers for every modulus below, and the operand frame (mpyc_amd/csrc/operands.hpp) on synthetic addresses, both
through tests/api_args_check.cpp built with g++ -- once plainly, once with the address and undefined-behaviour sanitizers.
No GPU needed."""
import os
import shutil
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))

# every prime of test_abi.py::test_ctx_classification
PRIMES = [2**61 - 1, 2**64 - 189, 2**128 - 173, 2**127 - 1, 2**96 - 17, 2**80 - 65, 2**97 - 141, 19, 2**31 - 1,
          6616326157076047771, 258797994007609146293811961253269568351, 2**136 - 113, 2**135 + 4823, 2**192 - 237]
# limb-boundary carries and borrows
PRIMES += [3, 7, 2**64 - 59, 2**128 - 159]
ORDERS = [2**deg for deg in (1, 8, 64, 100, 128)]          # the group-order path: q - 2 of GF(2^deg)


def expected_lines(m):
    """what api_args_check prints for modulus m, from Python integers"""
    def h(v):
        assert 0 <= v < 2**192
        return f'{v:048x}'

    def exp(name, e):
        return f'{name} {h(e)} {h(e // 3)} {e % 3}'

    lines = [f'modulus {h(m)}', f'bits {m.bit_length()}', f'ones {bin(m).count("1")}', exp('pm2', m - 2)]
    if m % 2 == 0:
        return lines
    for l in (1, 2, 63, 64):
        if l <= m.bit_length() - 2:
            lines.append(f'l {l} {h(2**l)} {h(2**(l - 1))} {h(pow(2, -l, m))} 1')
        else:
            lines.append(f'l {l} refused')
    lines += [exp('hb', (m - 1) // 2), exp('ha', (m + 1) // 2)]
    if m % 4 == 3:
        assert (3 * m - 5) % 4 == 0
        lines.append(exp('e34', (3 * m - 5) // 4))
    for f in (0, 1, 64, 191):
        lines.append(f'f {f} {h(pow(2, f, m))} {h((m + 1) // 2 * pow(2, f, m) % m)}')
    return lines


def build_and_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cc = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', *flags, '-o', exe,
                         os.path.join(TESTS, 'api_args_check.cpp')], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    moduli = PRIMES + ORDERS
    r = subprocess.run([exe] + [f'{m:x}' for m in moduli], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    want = [line for m in moduli for line in expected_lines(m)] + ['operands ok']
    got = r.stdout.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
    assert r.stderr == ''                                    # (a sanitizer report goes there)


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_integer_and_operand_frame(tmp_path):
    build_and_check(tmp_path, 'api_args_check', [])


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_integer_and_operand_frame_under_sanitizers(tmp_path):
    """the same program, stand-alone, built with the address and undefined-behaviour sanitizers and run as it is"""
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = subprocess.run(['g++', *flags, '-x', 'c++', '-', '-o', str(tmp_path / 'probe')], input='int main() { return 0; }\n',
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip('the sanitizer runtime does not link here')
    build_and_check(tmp_path, 'api_args_check_san', flags)
