"""CPU checks of threshold SHA-3: the two C ABI entries exist in header, library and binding; the rho / pi / iota tables and
the launch plan (mpyc_amd/csrc/keccak_geom.hpp) walked by tests/keccak_check.cpp with g++; protocols.keccak_f1600 / sha3 /
shake composed over the numpy stand-in of the two context methods (tests/keccak_cpuctx.py) for (m, t) = (1, 0) over GF(2),
(3, 1) over GF(4) and (7, 3) over GF(8): the opened digests are what hashlib computes, and for bit lengths hashlib cannot
express what the reference's demos/sha3.py opened (tests/golden/keccak/keccak.json).  No GPU needed."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import keccak_cpuctx as kc
from mpyc_amd import protocols

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

CONFIGS = ((1, 0, 1), (3, 1, 2), (7, 3, 3))            # (m, t, extension degree)
HASHES = {'sha3_224': (224, 1152), 'sha3_256': (256, 1088), 'sha3_384': (384, 832), 'sha3_512': (512, 576),
          'shake_128': (None, 1344), 'shake_256': (None, 1088)}


def golden():
    with open(os.path.join(TESTS, 'golden', 'keccak', 'keccak.json')) as fh:
        return json.load(fh)


def bits_of(s: str) -> np.ndarray:
    return np.array([int(c) for c in s], dtype=np.uint8)


def run_hash(ctx, modulus, name, bits, m, t, d, rng):
    """bits: (nstates, nbits) 0 / 1 -> the opened (nstates, d) digest bits of protocols.sha3 / shake over the stand-in"""
    nstates, nbits = bits.shape
    shares = ctx.matrix_from_numpy(kc.share_bits(modulus, bits, t, m, rng))
    if name.startswith('sha3'):
        out = protocols.sha3(ctx, None if t == 0 else _Field(modulus), shares, nbits, nstates, t, d=d)
    else:
        out = protocols.shake(ctx, None if t == 0 else _Field(modulus), shares, nbits, nstates, t, d, c=256 if name == 'shake_128' else 512)
    assert (out.rows, out.n) == (m, nstates * d)
    rows = out.t.numpy()[:, :out.n]
    opened = kc.open_shares(modulus, rows, t)
    assert (opened <= 1).all()
    for sub in list(kc.subsets(m, t + 1))[:4]:                   # every party's row is a share of the same bits
        T, acc = kc.mul_table(modulus), np.zeros(out.n, dtype=np.uint8)
        for l, j in zip(kc.lagrange_at_zero(modulus, [j + 1 for j in sub]), sub):
            acc ^= T[l][rows[j]]
        assert (acc == opened).all()
    return opened.reshape(nstates, d)


class _Field:
    """what protocols._lagrange asks of a field type: the reference's recombination vector over GF(2^n), by brute force"""

    def __init__(self, modulus):
        self.modulus = modulus


@pytest.fixture(autouse=True)
def _lagrange_by_brute_force(monkeypatch):
    monkeypatch.setattr(protocols, '_lagrange', lambda field, xs: kc.lagrange_at_zero(field.modulus, list(xs)))


def test_entries_exist_in_header_library_and_binding():
    from mpyc_amd import _ffi
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu_math.h')).read()
    for name in ('ffgm_gf2_keccak_local', 'ffgm_gf2_keccak_round'):
        assert f'int {name}(' in hdr and name in _ffi.EXPORTED_MATH
    L_ = _ffi.lib()
    assert L_.ffgm_gf2_keccak_local(None, None, None, 1, 0, 1, -1, 1, None, 0, 1, None) == _ffi.EINVAL
    assert L_.ffgm_gf2_keccak_round(None, None, None, 1, 0, -1, None, 0, 20, None, 0, 1, 3, None, 0, 0, 1, None) == _ffi.EINVAL


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_keccak_geometry_on_the_host(tmp_path):
    """rho, pi, the source table, iota and the launch plan for nstates = 1..33 against walk, brute force and the standard"""
    exe = str(tmp_path / 'keccak_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'keccak_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'keccak ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) > 24 + 1600 + 168 + 33 * 1600


def test_the_fixture_is_what_the_issue_asks_for():
    doc = golden()
    assert [e['nbits'] for e in doc['digests']] == [5, 30, 1605, 1630]
    for e in doc['digests']:
        assert len(e['message']) == e['nbits'] and len(e['sha3_256']) == 256 and len(e['shake128_256']) == 256
    assert len(doc['f1600']) == 2 and doc['f1600'][0]['in'] == '0' * 1600 and '1' in doc['f1600'][1]['in']
    assert all(len(e['in']) == 1600 and len(e['out']) == 1600 for e in doc['f1600'])
    # the zero-state permutation is the published first test vector of Keccak-f[1600]
    lane0 = int(doc['f1600'][0]['out'][:64][::-1], 2)
    assert lane0 == 0xF1258F7940E1DDE7


def test_the_stand_in_round_constants_and_table():
    assert sum(2**((1 << j) - 1) * b for j, b in enumerate(kc.ROUND_BITS[0])) == 1
    assert sum(2**((1 << j) - 1) * b for j, b in enumerate(kc.ROUND_BITS[23])) == 0x8000000080008008
    T = kc.mul_table(0b111)
    assert T[2][2] == 3 and T[2][3] == 1 and T[3][3] == 2 and (T[1] == np.arange(4)).all()
    assert kc.lagrange_at_zero(0b111, [1, 2, 3]) == [1, 1, 1]


@pytest.mark.parametrize('m,t,e', CONFIGS)
def test_keccak_f1600_is_the_reference_permutation(m, t, e):
    """the fixture's two permutations as a batch of two states: 24 rounds and the tail, launches as the issue lists them"""
    modulus, doc = kc.IRREDUCIBLE[e], golden()
    ctx, rng = kc.KeccakCpuContext(modulus, seed=5), np.random.default_rng(7)
    states = np.stack([bits_of(v['in']) for v in doc['f1600']])
    S = ctx.matrix_from_numpy(kc.share_bits(modulus, states, t, m, rng))
    before = S.t.clone()
    out = protocols.keccak_f1600(ctx, None if t == 0 else _Field(modulus), S, 2, t)
    assert (S.t == before).all()
    opened = kc.open_shares(modulus, out.t.numpy()[:, :3200], t).reshape(2, 1600)
    assert (opened == np.stack([bits_of(v['out']) for v in doc['f1600']])).all()
    if t == 0:
        assert ctx.launches == [('local', r - 1, True, m) for r in range(24)] + [('local', 23, False, m)]
    else:
        assert ctx.launches == [('round', r - 1, t, m) for r in range(24)] + [('local', 23, False, m)]


@pytest.mark.parametrize('m,t,e', CONFIGS)
@pytest.mark.parametrize('name', list(HASHES))
def test_hashes_at_the_padding_edges_against_hashlib(m, t, e, name):
    d, r = HASHES[name]
    d_out = d or 256
    modulus = kc.IRREDUCIBLE[e]
    rng = np.random.default_rng(100 * m + len(name))
    lengths = (0, 1, r // 8 - 1, r // 8, r // 8 + 1)
    for nbytes in lengths:
        msg = rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()
        ctx = kc.KeccakCpuContext(modulus, seed=nbytes + 1)
        got = run_hash(ctx, modulus, name, protocols.message_bits([msg]), m, t, d_out, rng)
        h = getattr(hashlib, name)(msg)
        want = h.digest() if d else h.digest(d_out // 8)
        assert protocols.digest_bytes(got) == [want], (name, nbytes)


@pytest.mark.parametrize('m,t,e', CONFIGS)
def test_shake_squeezes_a_second_block(m, t, e):
    modulus, rng = kc.IRREDUCIBLE[e], np.random.default_rng(3)
    msg = b'squeeze past the rate'
    d = 1344 + 8
    got = run_hash(kc.KeccakCpuContext(modulus), modulus, 'shake_128', protocols.message_bits([msg]), m, t, d, rng)
    assert protocols.digest_bytes(got) == [hashlib.shake_128(msg).digest(d // 8)]


@pytest.mark.parametrize('m,t,e', CONFIGS)
def test_a_batch_of_three_messages(m, t, e):
    modulus, rng = kc.IRREDUCIBLE[e], np.random.default_rng(11)
    msgs = [bytes([i]) * 140 for i in (1, 2, 250)]               # 140 bytes: two blocks of SHA3-256
    got = run_hash(kc.KeccakCpuContext(modulus), modulus, 'sha3_256', protocols.message_bits(msgs), m, t, 256, rng)
    assert protocols.digest_bytes(got) == [hashlib.sha3_256(v).digest() for v in msgs]


@pytest.mark.parametrize('m,t,e', CONFIGS)
def test_bit_lengths_hashlib_cannot_express(m, t, e):
    modulus, rng = kc.IRREDUCIBLE[e], np.random.default_rng(13)
    for entry in golden()['digests']:
        bits = bits_of(entry['message']).reshape(1, -1)
        got = run_hash(kc.KeccakCpuContext(modulus), modulus, 'sha3_256', bits, m, t, 256, rng)
        assert (got[0] == bits_of(entry['sha3_256'])).all(), entry['nbits']
        got = run_hash(kc.KeccakCpuContext(modulus), modulus, 'shake_128', bits, m, t, 256, rng)
        assert (got[0] == bits_of(entry['shake128_256'])).all(), entry['nbits']


def test_refusals_of_the_protocols():
    ctx = kc.KeccakCpuContext(0b111)
    S = ctx.empty_matrix(3, 1600)
    with pytest.raises(ValueError):
        protocols.keccak_f1600(ctx, _Field(0b111), S, 2, 1)              # rows are one state, not two
    with pytest.raises(ValueError):
        protocols.keccak_f1600(ctx, _Field(0b111), ctx.empty_matrix(2, 1600), 1, 1)   # fewer than 2t+1 parties
    with pytest.raises(ValueError):
        protocols.sha3(ctx, _Field(0b111), ctx.empty_matrix(3, 8), 8, 1, 1, d=200)
    with pytest.raises(ValueError):
        protocols.shake(ctx, _Field(0b111), ctx.empty_matrix(3, 8), 8, 1, 1, 256, c=300)
    with pytest.raises(ValueError):
        protocols.sha3(ctx, _Field(0b111), ctx.empty_matrix(3, 8), 16, 1, 1)
    with pytest.raises(ValueError):
        protocols.digest_bytes(np.ones((1, 12), dtype=np.uint8))
    with pytest.raises(NotImplementedError):
        ctx.keccak_round([S.row(0)], [1], 1, 1, 4)                       # GF(4) has no point for a fourth party
    assert protocols.message_bits([b'\x01\x80']).tolist() == [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]]
    assert protocols.digest_bytes([[1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]]) == [b'\x01\x80']
