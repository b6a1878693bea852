"""The drop-in behind the real MPyC runtime.

mpyc_amd.install() substitutes the device array type (derived from mpyc's own FiniteFieldArray) and the
sharing functions into an importable mpyc; these tests then run the REFERENCE's own unit tests and its
np_aes demo, unmodified, on top of it:

  * build container (reference in /root/reference, no GPU): `-m "not gpu"`, on the Python-integer context of
    tests/cpuctx.py -- checks the HOST logic of the substitution;
  * GPU box: `-m gpu`, on libffgpu's kernels.  The reference does not exist there unless a copy was staged
    into oracle/_ref/ (build() does it where the reference checkout exists, oracle/Makefile `ref`; it is
    git-ignored, never committed, and travels with the working tree); without it these tests skip.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = os.path.join(ROOT, 'oracle', '_ref')
FIPS197 = '69c4e0d86a7b0430d8cdb78070b4c55a'        # docs/demos.rst:611, FIPS-197 appendix C.1


def _ref_root(gpu: bool):
    if gpu:
        return STAGE if os.path.isdir(os.path.join(STAGE, 'mpyc')) else None
    return '/root/reference' if os.path.isdir('/root/reference/mpyc') else None


def _env(ref, cpuctx: bool, site: str):
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([site, os.path.join(ROOT, 'tests'), ROOT, ref])
    env['MPYC_GPU'] = '1'
    env.pop('MPYC_AMD_CPUCTX', None)
    if cpuctx:
        env['MPYC_AMD_CPUCTX'] = '1'
    return env


def _run_reference_tests(ref, cpuctx, files, extra_env=None, k=None):
    env = _env(ref, cpuctx, os.path.join(ROOT, 'tests', 'devsite'))
    env.update(extra_env or {})
    cmd = [sys.executable, '-m', 'pytest', '-p', 'refplugin', '-p', 'no:cacheprovider', '-q', '--tb=short']
    cmd += [os.path.join(ref, 'tests', f) for f in files]
    if k:
        cmd += ['-k', k]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd='/tmp', env=env, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    return r.stdout


def _run_np_aes(ref, cpuctx, args):
    site = os.path.join(ROOT, 'tests', 'devsite') if cpuctx else os.path.join(ROOT, 'mpyc_amd', 'autoinstall')
    env = _env(ref, cpuctx, site)
    env['MPYC_AMD_TRACE_INSTALL'] = '1'
    r = subprocess.run([sys.executable, 'np_aes.py'] + args, capture_output=True, text=True,
                       cwd=os.path.join(ref, 'demos'), env=env, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and FIPS197 in out, out[-3000:]
    assert 'mpyc_amd.install' in out, out[-3000:]          # the substitution really was active in this process
    return out


REF_FILES = ['test_finfields.py', 'test_thresha.py', 'test_gfpx.py', 'test_runtime.py', 'test_secpols.py',
             'test_seclists.py', 'test_mpctools.py', 'test_random.py', 'test_statistics.py']


# ---------------------------------------------------------------------------------------------------
# build container: host logic under the real runtime
# ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(_ref_root(False) is None, reason='reference checkout not present')
def test_install_substitutes_array_type_and_sharing_functions():
    code = '''
import mpyc_amd
names = mpyc_amd.install()
from mpyc import finfields, thresha
import mpyc_amd.finfields as gff
F = finfields.GF(2**61 - 1)                      # created AFTER install -> device array type ...
assert issubclass(F.array, gff.FieldArray) and issubclass(F.array, finfields.FiniteFieldArray), F.array.__mro__
assert F.array.field is F
G = finfields.GF(finfields.find_irreducible(2, 8))
assert issubclass(G.array, gff.FieldArray)
W = finfields.GF(finfields.find_prime_root(200)[0])       # wider than the device path: the reference's own class
assert not issubclass(W.array, gff.FieldArray) and issubclass(W.array, finfields.PrimeFieldArray)
X = finfields.GF(finfields.find_irreducible(3, 2))        # odd-characteristic extension field: reference class
assert not issubclass(X.array, gff.FieldArray)
assert 'thresha.np_random_split' in names and thresha.np_random_split.reference is not thresha.np_random_split
import mpyc_amd.thresha as gth
assert gth._recombination_vector(F, (1, 2, 3), 0) == [3, F.modulus - 3, 1]
ops = gff._fops(G)
assert ops.binary and ops.modulus == 0x11b and ops.mul(57, 67) == 137 and ops.order == 256
print("WIRING_OK", len(names))
'''
    env = _env('/root/reference', False, os.path.join(ROOT, 'tests', 'devsite'))
    env['MPYC_GPU'] = '0'
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd='/tmp', env=env, timeout=300)
    assert r.returncode == 0 and 'WIRING_OK' in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(_ref_root(False) is None, reason='reference checkout not present')
def test_reference_suite_under_install_host_logic():
    """lschoe/mpyc's own tests, unmodified, with install() active (list path routed to the device functions too, and the
    device-resident integer views of `.value` switched on for arrays of any size: MPYC_AMD_LAZY_INTS_MIN=0)."""
    out = _run_reference_tests('/root/reference', True, REF_FILES, {'MPYC_AMD_LIST_MIN': '0', 'MPYC_AMD_LAZY_INTS_MIN': '0'})
    assert ' passed' in out and 'failed' not in out


@pytest.mark.skipif(_ref_root(False) is None, reason='reference checkout not present')
def test_np_aes_demo_under_install_host_logic():
    _run_np_aes('/root/reference', True, ['-1'])
    _run_np_aes('/root/reference', True, ['-1', '-M3'])          # 3 party processes, TCP on localhost


# ---------------------------------------------------------------------------------------------------
# GPU box (needs the staged reference copy)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(_ref_root(True) is None, reason='no staged reference copy (oracle/_ref/, made by build())')
def test_reference_suite_under_install_on_gpu():
    out = _run_reference_tests(STAGE, False, REF_FILES, {'MPYC_AMD_LIST_MIN': '0', 'MPYC_AMD_LAZY_INTS_MIN': '0'})
    assert ' passed' in out and 'failed' not in out


@pytest.mark.gpu
@pytest.mark.skipif(_ref_root(True) is None, reason='no staged reference copy (oracle/_ref/, made by build())')
def test_np_aes_demo_under_install_on_gpu():
    _run_np_aes(STAGE, False, ['-1'])
    _run_np_aes(STAGE, False, ['-1', '-M3'])


@pytest.mark.gpu
@pytest.mark.skipif(_ref_root(True) is None, reason='no staged reference copy (oracle/_ref/, made by build())')
def test_reference_np_demos_under_install_on_gpu():
    """demos/np-run-all.sh of the reference, unmodified, with and without install(): identical printed results
    (tools/run_np_demos.sh; profiles/r02_np_demos.md)."""
    r = subprocess.run(['bash', os.path.join(ROOT, 'tools', 'run_np_demos.sh'), STAGE, 'gpu'], capture_output=True, text=True,
                       cwd=ROOT, timeout=1800)
    assert r.returncode == 0 and 'DIFF' not in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count('SAME') >= 7, r.stdout           # incl. np_lpsolver -i5: 136-bit root-of-unity field (MONT192)


@pytest.mark.skipif(_ref_root(False) is None, reason='reference checkout not present')
def test_reference_np_demos_under_install_host_logic():
    env = dict(os.environ, DEMOS='np_id3gini.py\nnp_lpsolver.py\nnp_aes.py -1\nnp_onewayhashchains.py -k2 --no-random-seed\nsha3.py')
    r = subprocess.run(['bash', os.path.join(ROOT, 'tools', 'run_np_demos.sh'), '/root/reference', 'cpuctx'], capture_output=True,
                       text=True, cwd=ROOT, timeout=1800, env=env)
    assert r.returncode == 0 and 'DIFF' not in r.stdout and r.stdout.count('SAME') == 5, (r.stdout + r.stderr)[-3000:]


_SAME_P_CODE = '''
import pickle
import mpyc_amd
mpyc_amd.install()
import os
if os.environ.get('MPYC_AMD_CPUCTX') == '1':
    from cpuctx import use_cpu_contexts
    use_cpu_contexts()
from mpyc import finfields, thresha
p, n, w = finfields.find_prime_root(40, n=3)
F1 = finfields.GF(p)                    # (p, 2, p-1)
F2 = finfields.GF((p, n, w))            # same modulus, root of unity of order 3: a DIFFERENT cached class
F3 = finfields.GF((p, 1, 1))
assert F1 is not F2 and F1.modulus == F2.modulus == F3.modulus
for F in (F1, F2, F3, F1):              # creation / use order must not matter
    a = F.array([1, 2, 3, p - 1])
    b = pickle.loads(pickle.dumps(a))
    assert type(b) is F.array and b.field is F, (F.nth, type(b).field.nth)
    rows = thresha.np_random_split(F, a, 1, 3)
    back = [pickle.loads(pickle.dumps(rows[i])) for i in range(3)]
    y = thresha.np_recombine(F, [(i + 1, back[i]) for i in range(2)])
    assert (y == a).all()
print('SAME_P_OK')
'''


@pytest.mark.skipif(_ref_root(False) is None, reason='reference checkout not present')
def test_pickled_rows_keep_their_field_class_host_logic():
    """mpyc caches prime fields per (p, n, w); rows pickled over one of them must not come back as arrays
    of a sibling class over the same modulus (np_recombine / field.array would raise)."""
    env = _env('/root/reference', True, os.path.join(ROOT, 'tests', 'devsite'))
    r = subprocess.run([sys.executable, '-c', _SAME_P_CODE], capture_output=True, text=True, cwd='/tmp', env=env, timeout=300)
    assert r.returncode == 0 and 'SAME_P_OK' in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.skipif(_ref_root(True) is None, reason='no staged reference copy (oracle/_ref/, made by build())')
def test_pickled_rows_keep_their_field_class_on_gpu():
    env = _env(STAGE, False, os.path.join(ROOT, 'mpyc_amd', 'autoinstall'))
    r = subprocess.run([sys.executable, '-c', _SAME_P_CODE], capture_output=True, text=True, cwd='/tmp', env=env, timeout=300)
    assert r.returncode == 0 and 'SAME_P_OK' in r.stdout, r.stdout + r.stderr


_RECIPROCAL_CODE = '''
import os, sys
import mpyc_amd
mpyc_amd.install()
if os.environ.get('MPYC_AMD_CPUCTX') == '1':
    from cpuctx import use_cpu_contexts
    use_cpu_contexts()
sys.argv = [sys.argv[0], '--no-log']
from mpyc.runtime import mpc
import mpyc_amd.finfields as gff
import numpy as np

p = 2**61 - 1
secfld = mpc.SecFld(p)
n = 6000
vals = [(7 * i * i + 3 * i + 1) % p or 1 for i in range(n)]
boxed = []                       # arrays whose integers were materialised (FieldArray._host_value)
orig_host = gff.FieldArray._host_value
def counting(self):
    if self._cache is None:
        boxed.append(self.size)
    return orig_host(self)
gff.FieldArray._host_value = counting

async def main():
    async with mpc:
        a = secfld.array(np.array(vals, dtype=object))
        del boxed[:]
        b = mpc.np_reciprocal(a)
        y = await mpc.output(b)
        common = list(boxed)
        del boxed[:]
        assert [int(v) for v in y.value] == [pow(v, -1, p) for v in vals]
        # the branch behind `np.count_nonzero(ar.value) < n`: some mask r is zero (probability n / p in real runs)
        orig = mpc._np_randoms
        calls = []
        def with_zeros(field, m, bound=None):
            r = orig(field, m, bound) if bound is not None else orig(field, m)
            if not calls:
                calls.append(1)
                r = r.copy() if hasattr(r, 'copy') else r
                r[3] = 0
                r[m - 1] = 0
            return r
        mpc._np_randoms = with_zeros
        b2 = mpc.np_reciprocal(a)
        y2 = await mpc.output(b2)
        mpc._np_randoms = orig
        rare = list(boxed)
        assert [int(v) for v in y2.value[:50]] == [pow(v, -1, p) for v in vals[:50]]
        assert [int(v) for v in y2.value] == [pow(v, -1, p) for v in vals]
    return common, rare

common, rare = mpc.run(main())
assert gff.HostView.lazy_lines, 'np_reciprocal was not registered'
assert not any(s >= n for s in common), common          # common path: the opened a*r is counted on the device
assert any(s >= n - 2 for s in rare), rare              # zero branch: real integers for the item assignments
print('RECIPROCAL_OK', common, rare)
'''


@pytest.mark.skipif(_ref_root(False) is None, reason='reference checkout not present')
def test_np_reciprocal_reader_host_logic():
    """runtime.py:1251-1294 under install(): `np.count_nonzero(ar.value)` is answered on the device (no integers are boxed
    on the path every call takes), and the ar == 0 branch -- `b[mask] = x.value`, a C-level assignment -- still gets the real
    integers (HostView.lazy_lines: lazy on the matching source line only)."""
    env = _env('/root/reference', True, os.path.join(ROOT, 'tests', 'devsite'))
    r = subprocess.run([sys.executable, '-c', _RECIPROCAL_CODE], capture_output=True, text=True, cwd='/tmp', env=env, timeout=600)
    assert r.returncode == 0 and 'RECIPROCAL_OK' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
@pytest.mark.skipif(_ref_root(True) is None, reason='no staged reference copy (oracle/_ref/, made by build())')
def test_np_reciprocal_reader_on_gpu():
    env = _env(STAGE, False, os.path.join(ROOT, 'mpyc_amd', 'autoinstall'))
    r = subprocess.run([sys.executable, '-c', _RECIPROCAL_CODE], capture_output=True, text=True, cwd='/tmp', env=env, timeout=600)
    assert r.returncode == 0 and 'RECIPROCAL_OK' in r.stdout, (r.stdout + r.stderr)[-3000:]
