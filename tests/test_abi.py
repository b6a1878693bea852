"""C-ABI boundary checks that need no GPU: the library loads, exports exactly what
include/ffgpu.h declares, classifies moduli, and rejects bad arguments with status codes
(no compute calls here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    from mpyc_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi.lib()


def declared_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'ffgpu.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    return sorted(set(re.findall(r'\b(ffgpu_[a-z0-9_]+)\s*\(', hdr)))


def test_header_symbols_exported(L):
    from mpyc_amd import _ffi
    decl = declared_symbols()
    assert len(decl) >= 30
    out = subprocess.run(['nm', '-D', '--defined-only', _ffi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (ffgpu_[a-z0-9_]+)', out))
    missing = [s for s in decl if s not in exported]
    assert not missing, f'declared in include/ffgpu.h but not exported: {missing}'
    assert sorted(_ffi.EXPORTED) == decl, 'python binding and header disagree'
    for s in decl:
        getattr(L, s)


def test_version_and_strerror(L):
    assert L.ffgpu_abi_version() == 1
    assert L.ffgpu_strerror(0) == b'ok'
    assert b'invalid' in L.ffgpu_strerror(1)


def mk(L, kind, modulus, nl=3):
    from mpyc_amd import _ffi
    h = ctypes.c_void_p()
    rc = L.ffgpu_ctx_create(kind, _ffi.limbs(modulus, nl), nl, 0, ctypes.byref(h))
    return rc, h


def test_ctx_classification(L):
    from mpyc_amd import _ffi
    cases = [
        (_ffi.PRIME, 2**61 - 1, 8, 1), (_ffi.PRIME, 2**64 - 189, 8, 1), (_ffi.PRIME, 2**128 - 173, 16, 1),
        (_ffi.PRIME, 2**127 - 1, 16, 1), (_ffi.PRIME, 2**96 - 17, 12, 1), (_ffi.PRIME, 2**80 - 65, 12, 1),
        (_ffi.PRIME, 2**97 - 141, 16, 1), (_ffi.PRIME, 19, 4, 2),
        (_ffi.PRIME, 2**31 - 1, 4, 2), (_ffi.PRIME, 6616326157076047771, 8, 2),
        (_ffi.PRIME, 258797994007609146293811961253269568351, 16, 5),
        (_ffi.PRIME, 2**136 - 113, 24, 1), (_ffi.PRIME, 2**135 + 4823, 24, 5), (_ffi.PRIME, 2**192 - 237, 24, 1),
        (_ffi.BINARY, 0x11b, 1, 3), (_ffi.BINARY, 0b111, 1, 3), (_ffi.BINARY, (1 << 64) | 0x1b, 8, 4),
        (_ffi.BINARY, (1 << 128) | 0x87, 16, 4),
    ]
    for kind, mod, eb, red in cases:
        rc, h = mk(L, kind, mod)
        assert rc == 0, (hex(mod), rc)
        assert L.ffgpu_ctx_elem_bytes(h) == eb, hex(mod)
        assert L.ffgpu_ctx_reduction(h) == red, hex(mod)
        assert L.ffgpu_ctx_device(h) == 0
        L.ffgpu_ctx_destroy(h)


def test_bad_arguments(L):
    from mpyc_amd import _ffi
    assert mk(L, _ffi.PRIME, 0)[0] == _ffi.EMODULUS
    assert mk(L, _ffi.PRIME, 1)[0] == _ffi.EMODULUS
    assert mk(L, _ffi.PRIME, 1 << 128)[0] == _ffi.EMODULUS         # even three-limb modulus
    assert mk(L, _ffi.PRIME, (1 << 192) + 7, nl=4)[0] != 0          # above 192 bits
    assert mk(L, _ffi.PRIME, (1 << 127) + 2**40)[0] == _ffi.EMODULUS  # even two-limb modulus
    assert mk(L, 7, 19)[0] == _ffi.EINVAL
    assert mk(L, _ffi.BINARY, 1)[0] == _ffi.EMODULUS
    rc, h = mk(L, _ffi.PRIME, 2**61 - 1)
    assert rc == 0
    # split: 0 <= t < m (thresha.py:26), null pointers, strides
    assert L.ffgpu_split(h, 16, 16, 8, 3, 3, 16, 8, 8, None) == _ffi.EINVAL
    assert L.ffgpu_split(h, None, 16, 8, 1, 3, 16, 8, 8, None) == _ffi.EINVAL
    assert L.ffgpu_split(h, 16, 16, 8, 1, 3, 16, 4, 8, None) == _ffi.EINVAL      # share_stride < n
    assert L.ffgpu_split(h, 16, None, 0, 0, 1, 16, 0, 0, None) == _ffi.OK        # n == 0 is a no-op
    assert L.ffgpu_mul(h, None, None, None, 0, None) == _ffi.OK
    assert L.ffgpu_mul(h, None, 16, 16, 4, None) == _ffi.EINVAL
    assert L.ffgpu_recombine(h, None, None, 0, 1, 16, 8, 8, None) == _ffi.EINVAL
    rows8 = (ctypes.c_uint8 * 8)()
    assert L.ffgpu_gf256_sbox(h, 16, rows8, 0, 16, 8, None) == _ffi.ENOTSUP    # not GF(2^8)
    L.ffgpu_ctx_destroy(h)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from mpyc_amd import _ffi
    monkeypatch.setattr(_ffi, '_lib', None)
    monkeypatch.setattr(_ffi, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_ffi.FfgpuError):
        _ffi.lib()


def test_empty_inputs_are_ok_everywhere(L):
    """n = 0 (empty arrays, tests/test_thresha.py and finfields edge cases): every compute entry point
    returns FFGPU_OK before touching a device (so this runs without a GPU) and without reading pointers."""
    from mpyc_amd import _ffi
    rc, h = mk(L, _ffi.PRIME, 2**61 - 1)
    assert rc == 0
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    two = (ctypes.c_uint64 * 2)(1, 0)
    rows = (ctypes.c_void_p * 3)(p.value, p.value, p.value)
    lam = (ctypes.c_uint64 * 6)(1, 0, 1, 0, 1, 0)
    key = bytes(32)
    assert L.ffgpu_add(h, p, p, p, 0, None) == 0
    assert L.ffgpu_mul(h, p, p, p, 0, None) == 0
    assert L.ffgpu_neg(h, p, p, 0, None) == 0
    assert L.ffgpu_reduce(h, p, p, 0, None) == 0
    assert L.ffgpu_mul_scalar(h, p, two, p, 0, None) == 0
    assert L.ffgpu_muladd(h, p, p, p, p, 0, None) == 0
    assert L.ffgpu_pow(h, p, two, 1, p, 0, None) == 0
    assert L.ffgpu_inv(h, p, p, 0, p, None) == 0
    assert L.ffgpu_split(h, p, p, 0, 1, 3, p, 0, 0, None) == 0
    assert L.ffgpu_mul_split(h, p, p, p, 0, 1, 3, p, 0, 0, None) == 0
    assert L.ffgpu_split_rng(h, p, key, 0, 20, 1, 3, p, 0, 0, None) == 0
    assert L.ffgpu_recombine(h, rows, lam, 3, 1, p, 0, 0, None) == 0
    assert L.ffgpu_gate_rng(h, rows, lam, 3, None, None, 0, key, 0, 20, None, 1, 3, p, 0, 0, None) == 0
    assert L.ffgpu_group_matvec(h, lam, None, 1, 3, p, p, 0, None) == 0
    assert L.ffgpu_gauss(h, p, 3, 3, 0, 0, None, p, None) == 0
    assert L.ffgpu_shake128_expand(None, None, 0, 10, None, 1) == 0
    # and bad shapes are still rejected when n = 0
    assert L.ffgpu_split(h, p, p, 0, 3, 3, p, 0, 0, None) == _ffi.EINVAL      # t must be < m
    assert L.ffgpu_gate_rng(h, rows, lam, 3, None, None, 0, key, 0, 20, None, 4, 9, p, 0, 0, None) == _ffi.ENOTSUP
    L.ffgpu_ctx_destroy(h)


def test_statuses_before_device_work(L):
    """Calls that every compute entry point answers before any device work (so this runs without a GPU), with the
    status each one gives.  The values are those of the library before its host layer got one launcher status and one
    call scope; they are pinned here so that a change of that layer cannot move them."""
    from mpyc_amd import _ffi
    EINVAL, ENOTSUP = _ffi.EINVAL, _ffi.ENOTSUP
    h = mk(L, _ffi.PRIME, 2**61 - 1)[1]           # 2^61 - 1 = 3 mod 4: no Cipolla-Lehmer square roots
    h13 = mk(L, _ffi.PRIME, 13)[1]                # 13 = 1 mod 4
    hb = mk(L, _ffi.BINARY, 0x11b)[1]
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255
    A, B, C, W = base, base + 8192, base + 16384, base + 32768
    four = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    rows = (ctypes.c_void_p * 3)(A, A, A)
    lam = (ctypes.c_uint64 * 6)(1, 0, 1, 0, 1, 0)
    key = bytes(32)
    keys40 = (ctypes.c_uint8 * 80)()
    m17 = (ctypes.c_uint64 * (2 * 17 * 3))()
    m64 = (ctypes.c_uint64 * 128)()
    rows8 = (ctypes.c_uint8 * 8)()
    out3 = ctypes.cast(C, ctypes.POINTER(ctypes.c_double))
    # scans and axis reductions: k = 0, unknown operation, overlapping ranges, misaligned workspace
    assert L.ffgpu_scan(h, 0, A, B, 1, 0, 1, 0, None, 0, None) == EINVAL
    assert L.ffgpu_scan(h, 7, A, B, 1, 8, 1, 0, None, 0, None) == EINVAL
    assert L.ffgpu_scan(h, 0, A, A + 8, 1, 8, 1, 0, None, 0, None) == EINVAL
    assert L.ffgpu_scan(h, 0, A, B, 1, 8, 1, 0, W + 8, 64, None) == EINVAL
    assert L.ffgpu_scan(h, 0, A, B, 1, 8, 1, 0, A, 64, None) == EINVAL            # workspace inside the input
    assert L.ffgpu_axis_reduce(h, 0, A, B, 1, 0, 1, None, 0, None) == EINVAL
    assert L.ffgpu_axis_reduce(h, 0, A, A, 4, 8, 1, None, 0, None) == EINVAL      # a reduction is never in place
    assert L.ffgpu_axis_reduce(h, 0, A, B, 1, 8, 1, W + 8, 64, None) == EINVAL
    assert L.ffgpu_scan_workspace_bytes(h, 1, 0, 1) == 0
    assert L.ffgpu_scan_workspace_bytes(None, 1, 8, 1) == 0
    # convolution: the output overlaps an operand, an empty operand
    assert L.ffgpu_convolve(h, A, 8, B, 4, A + 16, None) == EINVAL
    assert L.ffgpu_convolve(h, A, 4, B, 8, B + 16, None) == EINVAL
    assert L.ffgpu_convolve(h, A, 8, B, 0, C, None) == EINVAL
    # gates: batch of 256, a host nonce that reaches the batch-row bits, a device-state nonce offset above 32 bits
    assert L.ffgpu_gate_rng_batch(h, rows, lam, 3, 8, None, None, 0, 0, key, 0, 20, None, 0, 1, 3, C, 8, 64, 8, 256, None) == EINVAL
    assert L.ffgpu_gate_rng_batch(h, rows, lam, 3, 8, None, None, 0, 0, key, 1 << 40, 20, None, 0, 1, 3, C, 8, 64, 8, 2, None) == EINVAL
    assert L.ffgpu_gate_rng_batch(h, rows, lam, 3, 8, None, None, 0, 0, None, 1 << 32, 20, W, 0, 1, 3, C, 8, 64, 8, 2, None) == EINVAL
    assert L.ffgpu_gate_rng_batch(h, rows, lam, 3, 8, None, None, 0, 0, key, 0, 20, None, 0, 4, 9, C, 8, 64, 8, 1, None) == ENOTSUP
    assert L.ffgpu_gate_rng_batch(h, rows, lam, 8, 8, None, None, 0, 0, key, 0, 20, None, 0, 1, 3, C, 8, 64, 8, 1, None) == ENOTSUP
    assert L.ffgpu_gate_rng(h, rows, lam, 3, None, None, 0, key, 0, 5, None, 1, 3, C, 8, 8, None) == EINVAL    # 5 rounds
    # pseudo-random secret sharing
    assert L.ffgpu_prss_chacha(h, keys40, 2, 1, 8, 0, 7, lam, 0, C, 8, None) == EINVAL
    assert L.ffgpu_prss_chacha(h, None, 2, 1, 8, 0, 20, lam, 0, C, 8, None) == EINVAL
    assert L.ffgpu_prss_combine(h, rows, 2, 1, 65, 0, lam, 0, C, 8, None) == EINVAL
    assert L.ffgpu_prss_combine(h, None, 2, 1, 8, 0, lam, 0, C, 8, None) == EINVAL
    # linear algebra
    assert L.ffgpu_group_matvec(h, m17, None, 17, 3, A, B, 8, None) == ENOTSUP
    assert L.ffgpu_group_matvec(h, m17, None, 0, 3, A, B, 8, None) == EINVAL
    assert L.ffgpu_matmul(h, A, 4, B, 4, C, 2, 4, 4, 4, None) == EINVAL           # ldc < N
    assert L.ffgpu_matmul(h, A, 2, B, 4, C, 4, 4, 4, 4, None) == EINVAL           # lda < K
    assert L.ffgpu_gauss(h, A, 3, 2, 1, 0, None, B, None) == EINVAL               # fewer columns than rows
    assert L.ffgpu_gauss(h, A, 3, 3, 1, 1, None, B, None) == EINVAL               # determinants wanted, nowhere to put them
    assert L.ffgpu_dot(h, A, None, C, W, 8, None) == EINVAL
    assert L.ffgpu_sum(h, A, None, W, 8, None) == EINVAL
    # powers, inverses, square roots
    assert L.ffgpu_pow(h, A, four, 4, B, 8, None) == EINVAL
    assert L.ffgpu_pow(h, A, None, 1, B, 8, None) == EINVAL
    assert L.ffgpu_inv(h, None, B, 8, None, None) == EINVAL
    assert L.ffgpu_sqrt_cl(h, A, B, 8, None) == ENOTSUP
    assert L.ffgpu_sqrt_cl(hb, A, B, 8, None) == ENOTSUP
    assert L.ffgpu_sqrt_cl(h13, None, B, 8, None) == EINVAL
    # element-wise calls
    assert L.ffgpu_add(h, A, None, C, 8, None) == EINVAL
    assert L.ffgpu_sub(h, A, B, None, 8, None) == EINVAL
    assert L.ffgpu_neg(h, None, B, 8, None) == EINVAL
    assert L.ffgpu_reduce(h, A, None, 8, None) == EINVAL
    assert L.ffgpu_muladd(h, A, B, None, C, 8, None) == EINVAL
    assert L.ffgpu_add_scalar(h, A, None, B, 8, None) == EINVAL
    assert L.ffgpu_mul_scalar(h, A, None, B, 8, None) == EINVAL
    assert L.ffgpu_rsub_scalar(h, A, None, B, 8, None) == EINVAL
    assert L.ffgpu_beaver_combine(h, A, A, A, A, None, 0, B, 8, None) == EINVAL
    assert L.ffgpu_copy(h, None, B, 16, None) == EINVAL
    # share generation with the device generator
    assert L.ffgpu_rng_coeffs(h, key, 0, 20, 0, C, 8, 8, None) == EINVAL          # t = 0
    assert L.ffgpu_rng_coeffs(h, None, 0, 20, 1, C, 8, 8, None) == EINVAL
    assert L.ffgpu_split_rng(h, A, key, 0, 5, 1, 3, C, 8, 8, None) == EINVAL      # 5 rounds
    assert L.ffgpu_mul_split_rng(h, A, None, key, 0, 20, 1, 3, C, 8, 8, None) == EINVAL
    assert L.ffgpu_mul_split(h, A, None, C, 8, 1, 3, C, 8, 8, None) == EINVAL
    assert L.ffgpu_split_rng_state(h, A, None, None, 1, 3, C, 8, 8, None) == EINVAL
    assert L.ffgpu_split_rng_state(h, A, None, W, 3, 3, C, 8, 8, None) == EINVAL
    assert L.ffgpu_rng_state_init(h, None, key, 0, 20, None) == EINVAL
    assert L.ffgpu_rng_state_init(h, W, key, 0, 7, None) == EINVAL
    assert L.ffgpu_rng_state_advance(h, None, 1, None) == EINVAL
    assert L.ffgpu_recombine(h, rows, lam, 3, 2, C, 4, 8, None) == EINVAL         # out_stride < n
    # the GF(2^8) family on a prime context, and its own limits on a GF(2^8) context
    assert L.ffgpu_gf256_to_bits(h, A, None, B, 8, None) == ENOTSUP
    assert L.ffgpu_gf256_bit_affine(h, m64, None, 0, A, B, 8, None) == ENOTSUP
    assert L.ffgpu_gf256_mask_open(h, rows, lam, 3, None, None, 0, C, 8, None) == ENOTSUP
    assert L.ffgpu_gf256_bits_affine_fold(h, m64, None, A, B, 64, C, 8, 8, 1, None) == ENOTSUP
    assert L.ffgpu_gf256_sbox_layer(h, m64, None, lam, lam, 1, 3, A, 8, B, 64, C, 8, 8, key, 0, 20, None, 0, None) == ENOTSUP
    assert L.ffgpu_gf256_sbox(h, A, rows8, 0, B, 8, None) == ENOTSUP
    assert L.ffgpu_gf256_mask_open(hb, rows, lam, 33, None, None, 0, C, 8, None) == ENOTSUP
    assert L.ffgpu_gf256_mask_open(hb, rows, lam, 0, None, None, 0, C, 8, None) == EINVAL
    assert L.ffgpu_gf256_sbox_layer(hb, m64, None, lam, lam, 4, 9, A, 8, B, 64, C, 8, 8, key, 0, 20, None, 0, None) == ENOTSUP
    assert L.ffgpu_gf256_sbox_layer(hb, m64, None, lam, lam, 1, 2, A, 8, B, 64, C, 8, 8, key, 0, 20, None, 0, None) == EINVAL
    assert L.ffgpu_gf256_bit_affine(hb, m64, None, 0, A + 1, B, 8, None) == EINVAL
    assert L.ffgpu_gf256_bits_affine_fold(hb, m64, None, A, B, 64, C, 8, 8, 0, None) == EINVAL
    assert L.ffgpu_gf256_to_bits(hb, None, None, B, 8, None) == EINVAL
    assert L.ffgpu_gf256_sbox(hb, None, rows8, 0, B, 8, None) == EINVAL
    assert L.ffgpu_valu_probe(h, 14, 1, 1, A, out3, None) == EINVAL
    for ctx in (h, h13, hb):
        L.ffgpu_ctx_destroy(ctx)
