"""CPU checks behind the contract of the ffgpu_gf256_* entry points (tests/gf256_contract.py): the references agree with each
other and with tests/golden/sbox.json before any GPU time is spent on them, and the launch plan and keystream counters of the
fused layer (mpyc_amd/csrc/sbox_layer_geom.hpp) are walked by tests/sbox_layer_check.cpp with g++.  No GPU needed."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import gf256_contract as gc
from oracle import pyoracle as po

TESTS = os.path.dirname(os.path.abspath(__file__))
F8 = gc.field(gc.AES)


def maps():
    A, B = gc.aes_map()
    return {'aes': (A, B), 'identity': (gc.identity(), None), 'general': gc.general_map(F8)}


def test_the_moduli_are_irreducible_and_the_tables_are_the_fields():
    assert [m.bit_length() - 1 for m in gc.BIT_AFFINE_MODULI] == [1, 2, 3, 4, 5, 6, 7, 8, 8]
    assert all(gc.irreducible(m) for m in gc.BIT_AFFINE_MODULI) and not gc.irreducible(0x11a) and not gc.irreducible(0b101)
    for m in gc.BIT_AFFINE_MODULI:
        F = gc.field(m)
        T = gc.mul_table(F)
        assert T.shape == (F.order, F.order) and (T == T.T).all() and (T[1] == np.arange(F.order)).all()
        for a in range(1, F.order):                         # a field: every row of a nonzero element is a permutation
            assert T[a][po.inv(F, a)] == 1 and len(set(T[a].tolist())) == F.order


def test_aes_map_opens_to_the_golden_table():
    g = gc.golden_sbox()
    A, B = gc.aes_map()
    assert int(g['modulus'], 16) == gc.AES and g['b'] == 0x63
    assert g['pow254'] == [po.pow254(F8, v) for v in range(256)]
    assert g['table'] == po.sbox(range(256)) == gc.sbox_lut(g['rows8'], g['b']).tolist()
    assert g['table'] == [gc.fold_py(F8, gc.affine_py(F8, A, B, [(p >> b) & 1 for b in range(8)])) for p in g['pow254']]


@pytest.mark.parametrize('modulus', gc.BIT_AFFINE_MODULI, ids=hex)
def test_array_references_equal_the_integer_ones(modulus):
    F = gc.field(modulus)
    rnd = random.Random(modulus)
    q = F.order
    for M, bias in [(gc.random_matrix(F, rnd, True), None), (gc.random_matrix(F, rnd, False), gc.random_bias(F, rnd)),
                    (gc.shift_matrix(3), gc.random_bias(F, rnd))]:
        x = [rnd.randrange(q) for _ in range(8 * 37)]
        for fb in (0, 1):
            assert gc.bit_affine_np(F, M, bias, fb, x).tolist() == gc.bit_affine_py(F, M, bias, fb, x)
        c = [rnd.randrange(q) for _ in range(37)]
        assert gc.bits_affine_fold_np(F, M, bias, c, x).tolist() == gc.bits_affine_fold_py(F, M, bias, c, x)
    inp, add = [rnd.randrange(q) for _ in range(29)], [rnd.randrange(q) for _ in range(8 * 29)]
    assert gc.to_bits_np(inp, add).tolist() == gc.to_bits_py(inp, add) and gc.to_bits_np(inp, None).tolist() == gc.to_bits_py(inp, None)
    assert gc.to_bits_py([0b10000101], None) == [1, 0, 1, 0, 0, 0, 0, 1]
    rows = [[rnd.randrange(q) for _ in range(29)] for _ in range(9)]
    rb = [[rnd.randrange(q) for _ in range(8 * 29)] for _ in range(3)]
    coef, mu = [rnd.randrange(q) for _ in range(9)], [rnd.randrange(1, q) for _ in range(3)]
    coef[4] = 0
    assert gc.mask_open_np(F, rows, coef, rb, mu, 29).tolist() == gc.mask_open_py(F, rows, coef, rb, mu, 29)
    # from_bits of the identity is the element itself when the "bits" are its bits
    v = list(range(q))
    bits = gc.to_bits_py(v, None)
    assert gc.bit_affine_py(F, gc.identity(), None, 1, bits) == [po.reduce(F, e) for e in v]


@pytest.mark.parametrize('m,t', gc.MT, ids=lambda v: str(v))
def test_layer_reference_opens_to_the_table_from_every_subset(m, t):
    """all 256 bytes through layer_py on shares built from known polynomials: every (t+1)-subset of the parties' output rows
    recombines to the FIPS table (AES map), to pow254 (identity, no bias) and to the general map of pow254; so do the shares"""
    torch = pytest.importorskip('torch')
    g = gc.golden_sbox()
    rnd = random.Random(100 * m + t)
    n = 256
    x = list(range(256))
    rnd.shuffle(x)
    r = [rnd.randrange(2) for _ in range(8 * n)]                     # bits: only then is bits(c) + r the bits of x^254
    cx = [[rnd.randrange(256) for _ in range(n)] for _ in range(t)]
    cr = [[rnd.randrange(256) for _ in range(8 * n)] for _ in range(t)]
    X, R = gc.share_rows_py(F8, x, cx, m), gc.share_rows_py(F8, r, cr, m)
    subs = gc.subsets(m, t + 1)
    for pts in subs:
        assert gc.recombine_py(F8, pts, [X[p - 1] for p in pts]) == x
        assert gc.recombine_py(F8, pts, [R[p - 1] for p in pts]) == r
    assert gc.recombine_py(F8, range(1, t + 1), X[:t]) != x          # t shares do not
    for name, (M, bias) in maps().items():
        out = gc.layer_py(F8, M, bias, x, r, R)
        want = {'aes': [g['table'][v] for v in x], 'identity': [g['pow254'][v] for v in x],
                'general': [gc.fold_py(F8, gc.affine_py(F8, M, bias, [(g['pow254'][v] >> b) & 1 for b in range(8)])) for v in x]}[name]
        for pts in subs:
            assert gc.recombine_py(F8, pts, [out[p - 1] for p in pts]) == want, (name, pts)
        # the table formulation (torch, here on the CPU) is the direct one, byte for byte, rows and opening
        tabs = gc.LayerTables(F8, M, bias)
        dev = tabs.on(torch, 'cpu')
        tt = lambda rows: torch.tensor(rows, dtype=torch.uint8)
        got = gc.layer_expected_torch(torch, dev, tt(x), tt(r), tt(R), n)
        assert got.tolist() == out, name
        assert gc.opened_torch(torch, tabs, dev, [got[p - 1] for p in subs[-1]], subs[-1]).tolist() == want


@pytest.mark.parametrize('m,t', [(3, 1), (5, 2), (7, 3)], ids=lambda v: str(v))
def test_torch_share_builder_is_the_integer_one(m, t):
    torch = pytest.importorskip('torch')
    M, bias = gc.general_map(F8)
    tabs = gc.LayerTables(F8, M, bias)
    dev = tabs.on(torch, 'cpu')
    for n, any_bytes in ((1, True), (3, False), (6, True), (300, True), (300, False)):
        x, r, X, R, cx, cr = gc.layer_inputs_torch(torch, tabs, dev, n, m, t, 7 + n, 'cpu', xs=n + 5, rs=8 * n + 16, any_bytes=any_bytes)
        assert X.shape == (m, n + 5) and R.shape == (m, 8 * n + 16)
        assert (X[:, n:] == gc.GUARD).all() and (R[:, 8 * n:] == gc.GUARD).all()
        assert X[:, :n].tolist() == gc.share_rows_py(F8, x.tolist(), [c.tolist() for c in cx], m)
        assert R[:, :8 * n].tolist() == gc.share_rows_py(F8, r.tolist(), [c.tolist() for c in cr], m)
        if n >= 256:
            assert sorted(set(x.tolist())) == list(range(256))
            assert len(set(r.tolist())) > 200 if any_bytes else set(r.tolist()) == {0, 1}
        assert gc.layer_expected_torch(torch, dev, x, r, R, n).tolist() == gc.layer_py(F8, M, bias, x.tolist(), r.tolist(), R[:, :8 * n].tolist())


def test_capped_sizes_give_three_trips():
    for cus in (1, 64, 256, 304):
        gsz = 256 * cus
        for entry in ('sbox', 'to_bits', 'bit_affine', 'mask_open', 'bits_affine_fold'):
            n = gc.capped_n(entry, gsz)
            assert gc.capped_trips(entry, n, gsz) == 3
            step = {'sbox': 16, 'to_bits': 2}.get(entry, 4)
            assert gc.capped_trips(entry, n - step, gsz) == 2, entry


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_sbox_layer_geometry_and_counters_on_the_host(tmp_path):
    """the launch plan that kernel and launcher share, and every ChaCha block counter of every (thread, step): pairwise distinct,
    inside their ranges, below 2^63; refused exactly where a range would be left"""
    exe = str(tmp_path / 'sbox_layer_check')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(TESTS, 'sbox_layer_check.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'sbox_layer ok' in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[-2]) > 1500 and int(r.stdout.split()[-1]) > 10**7
