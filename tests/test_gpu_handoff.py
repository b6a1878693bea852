"""Hand-off stores (mpyc_amd/csrc/handoff.hpp): a launch whose outputs the next launch on the stream read last time stores
them with the default cache policy instead of non-temporally.  The policy changes where the bytes sit, never which bytes
are written: the same chains of element-wise products, share generation (plain and fused), recombination (k = 2, 3, 7)
and device copies give bit-identical outputs with FFGPU_HANDOFF=1 (the default) and FFGPU_HANDOFF=0, over four prime
shapes, from one element to 10^7, and under a capped grid (FFGPU_BLOCKS_PER_CU=1).  Each run of the chains goes twice
through the stream, so the second pass runs with the predictions the first one settled.  The switches are read when a
context is created, so every setting runs in a fresh child process (this process does not open the GPU: one child at a
time)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
SIZES = (1, 63, 64 * 256 + 5, 10**6 + 3, 10**7)
CAPPED_SIZES = (1, 63, 64 * 256 + 5, 10**6 + 3)


def fields():
    from mpyc_amd.finfields import find_prime_root
    return {'P61': 2**61 - 1, 'P64': 2**64 - 189, 'P128': 2**128 - 173, 'P192': find_prime_root(192)[0]}


def draw(rs, modulus, eb, *dims):
    """canonical uniform-ish elements as the engine's limb arrays (top limb held below the modulus)"""
    if eb == 8:
        return rs.integers(0, modulus, dims, dtype=np.uint64)
    limbs = eb // 8
    a = rs.integers(0, 2**64, dims + (limbs,), dtype=np.uint64)
    a[..., -1] >>= np.uint64(2 + 64 * limbs - modulus.bit_length())
    return a


def chains(sizes):
    """{field/size: {output: digest}} of two passes of the chains, with whatever switches this process was started with"""
    from mpyc_amd.engine import FieldContext
    from oracle import pyoracle as po
    out = {}
    for name, p in fields().items():
        ctx = FieldContext(p, device=0)
        eb = ctx.elem_bytes
        F = po.Field(p, False)
        lam = {k: po.recombination_vector(F, list(range(1, k + 1)), 0) for k in (2, 3, 7)}
        for n in sizes:
            rs = np.random.default_rng(n + eb)
            a, b = ctx.from_numpy(draw(rs, p, eb, n)), ctx.from_numpy(draw(rs, p, eb, n))
            c1, c3 = ctx.matrix_from_numpy(draw(rs, p, eb, 1, n)), ctx.matrix_from_numpy(draw(rs, p, eb, 3, n))
            zero = ctx.from_numpy(np.zeros_like(draw(rs, p, eb, n)))
            dig = {}
            for rnd in range(2):
                c = ctx.mul(a, b)                                            # element-wise product -> split
                sh = ctx.split(c, c1, 1, 3)                                  # -> recombine from 2 rows
                y2 = ctx.recombine([sh.row(j) for j in range(2)], lam[2])
                sh2 = ctx.split(a, c1, 1, 3, mul_by=b)                       # fused product -> recombine from 3 rows
                y3 = ctx.recombine([sh2.row(j) for j in range(3)], lam[3])
                z = ctx.empty(n)
                if (n * eb) % 16 == 0:
                    ctx.copy(y3.t, z.t)                                      # recombination -> device copy -> ew2
                else:                                                        # (the copy kernel moves 16-byte units)
                    z = ctx.add(y3, zero)
                s = ctx.add(z, y2)
                sh7 = ctx.split(s, c3, 3, 7)                                 # -> recombine from 7 rows
                y7 = ctx.recombine([sh7.row(j) for j in range(7)], lam[7])
                host = {k: v.to_numpy() for k, v in
                        dict(c=c, sh=sh, y2=y2, sh2=sh2, y3=y3, z=z, s=s, sh7=sh7, y7=y7).items()}
                assert (host['y2'] == host['c']).all() and (host['y3'] == host['c']).all(), (name, n, rnd)
                assert (host['y7'] == host['s']).all(), (name, n, rnd)
                for k, v in host.items():
                    dig['%s%d' % (k, rnd)] = hashlib.blake2b(np.ascontiguousarray(v).tobytes(), digest_size=16).hexdigest()
                a = y7                                                       # the next pass starts from this one's end
            out['%s/%d' % (name, n)] = dig
    return out


def run_child(env_extra, sizes):
    child = ('import sys, json; sys.path[:0] = [%r, %r]\n'
             'import test_gpu_handoff as t\n'
             'print("DIGESTS " + json.dumps(t.chains(%r)))\n') % (ROOT, TESTS, tuple(sizes))
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, '-c', child], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('DIGESTS ')]
    assert line, r.stdout[-2000:]
    return json.loads(line[-1][len('DIGESTS '):])


def test_handoff_outputs_bit_identical():
    on = run_child({'FFGPU_HANDOFF': '1', 'FFGPU_BLOCKS_PER_CU': '0'}, SIZES)
    off = run_child({'FFGPU_HANDOFF': '0', 'FFGPU_BLOCKS_PER_CU': '0'}, SIZES)
    assert sorted(on) == sorted(off) and len(on) == 4 * len(SIZES)
    for key in on:
        assert on[key] == off[key], key


def test_handoff_outputs_bit_identical_capped_grid():
    """one workgroup per CU: every thread of the streaming loops takes several packs, stores of both policies in one loop"""
    on = run_child({'FFGPU_HANDOFF': '1', 'FFGPU_BLOCKS_PER_CU': '1'}, CAPPED_SIZES)
    off = run_child({'FFGPU_HANDOFF': '0', 'FFGPU_BLOCKS_PER_CU': '0'}, CAPPED_SIZES)
    for key in on:
        assert on[key] == off[key], key
