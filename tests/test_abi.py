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
    # the entries of the secure rounds: the table below
    got = secure_statuses(L)
    for entry, want in SECURE_STATUS.items():
        for label, status in want.items():
            assert got[entry].get(label) == status, (entry, label)
        assert list(got[entry]) == list(want), entry
    assert list(got) == list(SECURE_STATUS)
    # ffgm_conv2d_plan takes no device array and launches nothing: its refusals, and the plan of a valid call
    plan = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    hp = mk(L, _ffi.PRIME, 2**61 - 1)[1]
    hb = mk(L, _ffi.BINARY, 0x11b)[1]
    assert L.ffgm_conv2d_plan(None, 1, 2, 4, 4, 2, 3, 3, plan) == EINVAL
    assert L.ffgm_conv2d_plan(hb, 1, 2, 4, 4, 2, 3, 3, plan) == ENOTSUP
    assert L.ffgm_conv2d_plan(hb, 1, 2, 4, 4, 2, 3, 0, plan) == ENOTSUP
    assert L.ffgm_conv2d_plan(hp, 1, 2, 4, 4, 2, 3, 3, None) == EINVAL
    assert L.ffgm_conv2d_plan(hp, 1, 2, 4, 4, 2, 3, 0, plan) == EINVAL
    assert L.ffgm_conv2d_plan(hp, 1, 2, 4, 4, 2, 3, 65, plan) == ENOTSUP
    assert L.ffgm_conv2d_plan(hp, 1, 2, 4, 4, 2, 0, 65, plan) == ENOTSUP           # senders above the limit + bad scalar
    assert L.ffgm_conv2d_plan(hp, 1, 2, 4, 4, 2, 3, 65, None) == EINVAL            # ... + null pointer
    assert L.ffgm_conv2d_plan(hp, 1, 2, 4, 4, 2, 0, 3, plan) == EINVAL
    assert L.ffgm_conv2d_plan(hp, 1, 2, 4, 2, 2, 3, 3, plan) == EINVAL             # s > n
    assert L.ffgm_conv2d_plan(hp, 1 << 62, 2, 4, 4, 2, 3, 3, plan) == EINVAL
    assert L.ffgm_conv2d_plan(hp, 1 << 30, 1, 64, 64, 1, 3, 3, plan) == ENOTSUP    # grid refused
    assert L.ffgm_conv2d_plan(hp, 1 << 30, 1, 64, 64, 0, 3, 3, plan) == _ffi.OK    # empty
    assert L.ffgm_conv2d_plan(hp, 1, 2, 4, 4, 2, 3, 3, plan) == _ffi.OK
    L.ffgpu_ctx_destroy(hp)
    L.ffgpu_ctx_destroy(hb)
    h2 = mk(L, _ffi.PRIME, 2)[1]                   # p = 2 has no Legendre symbol: whatever else is wrong with the call
    for entry in ('ffgm_legendre_code', 'ffgm_bsgn_finish'):
        for label, ctx, args in secure_cases(L.ffgpu_ctx_elem_bytes(h2), 2, entry):
            if ctx is None:
                assert getattr(L, entry)(h2, *args) == ENOTSUP, (entry, label)
    L.ffgpu_ctx_destroy(h2)
    assert all(set(status) <= set('IN0') for want in SECURE_STATUS.values() for status in want.values())     # no call is launched
    assert L.ffgpu_last_hip_error() == b''


# ---- the entries of the secure rounds (ffgpu_sgn_* ... ffgm_conv2d): what each one answers before any device work -----------
# An entry is described once: its parameters in ABI order after the context, with the elements each array holds for the
# default scalars (a valid call, which is never made: it would launch).  secure_cases() derives the calls from that, one
# fault at a time and the pairs of faults whose statuses differ, under a label; SECURE_STATUS holds the recorded answers.
#   ('i', name, elems) input, ('o', ..) output, ('io', ..) updated in place, ('i?', ..) / ('o?', ..) optional (null: skipped);
#   ('R', name, count, elems) host array of device pointers read, ('R?', ..) optional, ('W', ..) written; ('h', name) host array of scalars;
#   ('n', name, default) scalar.  elems counts elements of the context; a negative number counts bytes.
SECURE_CONTEXTS = (2**61 - 1, 2**80 - 65, 2**136 - 113, 13)
N, LB, W2 = 8, 2, 2           # elements, bits per element (valid for every context below, also p = 13), rows of a (w, n) array
SECURE = {
    'ffgpu_sgn_mask': dict(p=[('i', 'a', N), ('i', 'rbits', N * LB), ('i', 'rdivl', N), ('n', 'l', LB), ('o', 'masked', N), ('n', 'n', N)],
                           bad=[dict(l=0), dict(l=65)], lbits='l'),
    'ffgpu_sgn_expand': dict(p=[('i', 'c', N), ('i', 'a', N), ('i', 'rbits', N * LB), ('i?', 'sbit', N), ('n', 'l', LB),
                                ('o?', 'e_out', N * LB + N), ('o?', 'nx_out', N * LB), ('o?', 'z_out', N), ('n', 'n', N)],
                             bad=[dict(l=0), dict(l=65), dict(e_out=0, nx_out=0, z_out=0), dict(sbit=0)], lbits='l'),
    'ffgpu_sgn_finish': dict(p=[('i', 'w', N), ('i', 'sbit', N), ('i', 'z', N), ('n', 'l', LB), ('o', 'lt_out', N), ('n', 'n', N)],
                             bad=[dict(l=0), dict(l=65)], lbits='l'),
    # stage (p, d, r) = (1, 1, 0) of k = 4: two pairs
    'ffgpu_cx_diff': dict(p=[('i', 'a', 16), ('o', 'out', 8), ('n', 'outer', 2), ('n', 'k', 4), ('n', 'inner', 2), ('n', 'p', 1), ('n', 'd', 1),
                             ('n', 'r', 0)], bad=[dict(p=3), dict(d=2), dict(r=2), dict(k=1), dict(k=0)], size='outer', empty=dict(inner=0)),
    'ffgpu_cx_apply': dict(p=[('io', 'a', 16), ('R', 'host_rows', 'nrows', 8), ('h', 'host_lambda'), ('n', 'nrows', 3), ('n', 'outer', 2),
                              ('n', 'k', 4), ('n', 'inner', 2), ('n', 'p', 1), ('n', 'd', 1), ('n', 'r', 0)],
                           bad=[dict(p=3), dict(d=2), dict(k=1)], size='outer', empty=dict(outer=0), count=('nrows', 9)),
    # k = 5: two pairs and the bye, three survivors
    'ffgpu_tour_diff': dict(p=[('i', 'a', 20), ('o', 'out', 8), ('n', 'outer', 2), ('n', 'k', 5), ('n', 'inner', 2), ('n', 'mode', 0), ('n', 'neg', 0)],
                            bad=[dict(mode=2), dict(mode=-1), dict(k=1)], size='outer', empty=dict(inner=0)),
    'ffgpu_tour_select': dict(p=[('i', 'a', 20), ('R', 'host_rows', 'nrows', 8), ('h', 'host_lambda'), ('n', 'nrows', 3), ('o', 'out', 12),
                                 ('n', 'outer', 2), ('n', 'k', 5), ('n', 'inner', 2), ('n', 'mode', 1), ('n', 'neg', 1)],
                              bad=[dict(mode=2), dict(k=1)], size='outer', empty=dict(outer=0), count=('nrows', 9)),
    'ffgpu_tour_unit_prod': dict(p=[('i', 'u', 12), ('i', 'c', 8), ('o', 'out', 8), ('n', 'outer', 2), ('n', 'k', 5), ('n', 'inner', 2)],
                                 bad=[dict(k=1), dict(k=0)], size='outer', empty=dict(inner=0)),
    'ffgpu_tour_unit_expand': dict(p=[('i', 'u', 12), ('R', 'host_rows', 'nrows', 8), ('h', 'host_lambda'), ('n', 'nrows', 3), ('o', 'out', 20),
                                      ('n', 'outer', 2), ('n', 'k', 5), ('n', 'inner', 2)],
                                   bad=[dict(k=1)], size='outer', empty=dict(outer=0), count=('nrows', 9)),
    # two components over k = 5 positions: a table of 2 * 5, compact rows of 2 pairs
    'ffgpu_find_leaf_prod': dict(p=[('i', 'bits', 20), ('i', 'tab', 10), ('o', 'out', 16), ('n', 'outer', 2), ('n', 'k', 5), ('n', 'inner', 2),
                                    ('n', 'ncomp', 2), ('n', 'flip', 0), ('n', 'virt', 0)],
                                 bad=[dict(ncomp=1), dict(ncomp=6), dict(flip=2), dict(virt=2), dict(k=1), dict(k=0, virt=1)], size='outer',
                                 empty=dict(inner=0)),
    'ffgpu_find_leaf_apply': dict(p=[('i', 'bits', 20), ('i', 'tab', 10), ('R', 'host_rows', 'nrows', 16), ('h', 'host_lambda'), ('n', 'nrows', 3),
                                     ('o', 'out', 24), ('n', 'outer', 2), ('n', 'k', 5), ('n', 'inner', 2), ('n', 'ncomp', 2), ('n', 'flip', 1),
                                     ('n', 'virt', 0)],
                                  bad=[dict(ncomp=1), dict(flip=-1), dict(virt=2), dict(k=1)], size='outer', empty=dict(outer=0), count=('nrows', 9)),
    'ffgpu_find_prod': dict(p=[('i', 'level', 40), ('o', 'out', 16), ('n', 'outer', 2), ('n', 'k', 5), ('n', 'inner', 2), ('n', 'ncomp', 2)],
                            bad=[dict(ncomp=1), dict(ncomp=6), dict(k=1)], size='outer', empty=dict(inner=0)),
    'ffgpu_bits_mask': dict(p=[('i', 'a', N), ('i', 'rbits', N * LB), ('i', 'rdivl', N), ('h', 'host_offset'), ('n', 'l', LB), ('o', 'masked', N),
                               ('n', 'n', N)], bad=[dict(l=0), dict(l=65), dict(host_offset=0)], lbits='l'),
    'ffgpu_bits_expand': dict(p=[('i', 'c', N), ('i', 'rbits', N * LB), ('n', 'l', LB), ('o', 'g_out', N * LB), ('o', 'p_out', N * LB), ('n', 'n', N)],
                              bad=[dict(l=0), dict(l=65)], lbits='l'),
    # l = 2: one round, of one row
    'ffgpu_carry_prod': dict(p=[('i', 'g', N * LB), ('i', 'p', N * LB), ('n', 'l', LB), ('n', 'round', 1), ('o', 'out', N), ('n', 'n', N)],
                             bad=[dict(l=0), dict(l=65), dict(round=0), dict(round=2)], lbits='l'),
    'ffgpu_carry_apply': dict(p=[('io', 'g', N * LB), ('io', 'p', N * LB), ('R', 'host_rows', 'nrows', N), ('h', 'host_lambda'), ('n', 'nrows', 3),
                                 ('n', 'l', LB), ('n', 'round', 1), ('n', 'n', N)],
                              bad=[dict(l=0), dict(round=0), dict(round=2)], count=('nrows', 9), lbits='l'),
    'ffgpu_bits_finish': dict(p=[('i', 'c', N), ('i', 'rbits', N * LB), ('i', 'g', N * LB), ('n', 'l', LB), ('o', 'out', N * LB), ('n', 'n', N)],
                              bad=[dict(l=0), dict(l=65)], lbits='l'),
    'ffgpu_trunc_mask': dict(p=[('i', 'a', N), ('i', 'rbits', N * LB), ('i', 'rdivf', N), ('h', 'host_offset'), ('n', 'f', LB), ('o', 'ar_out', N),
                                ('o', 'masked_out', N), ('n', 'n', N)], bad=[dict(f=0), dict(f=65), dict(host_offset=0)], lbits='f'),
    'ffgpu_trunc_finish': dict(p=[('R', 'host_rows', 'nrows', N), ('h', 'host_lambda'), ('n', 'nrows', 3), ('i', 'ar', N), ('n', 'f', LB),
                                  ('o', 'out', N), ('n', 'n', N)], bad=[dict(f=0), dict(f=65)], count=('nrows', 9), lbits='f'),
    'ffgpu_norm_prod': dict(p=[('i', 'bits', N * 3), ('n', 'l', 3), ('o', 'out', N * 2), ('o?', 'sign_out', N), ('n', 'n', N)],
                            bad=[dict(l=1), dict(l=65)]),
    'ffgpu_norm_apply': dict(p=[('i', 'bits', N * 3), ('R', 'host_rows', 'nrows', N * 2), ('h', 'host_lambda'), ('n', 'nrows', 3), ('n', 'l', 3),
                                ('o', 'out', N * 2), ('n', 'n', N)], bad=[dict(l=1), dict(l=65)], count=('nrows', 9)),
    'ffgm_powers_prod': dict(p=[('i', 'P', 2 * N), ('n', 'stride', N), ('n', 'h', 2), ('n', 'w', 1), ('o', 'out', N), ('n', 'n', N)],
                             bad=[dict(h=0), dict(w=0), dict(w=3), dict(stride=N - 1)]),
    'ffgm_poly_dot': dict(p=[('i', 'P', 2 * N), ('n', 'stride', N), ('n', 'theta', 2), ('i', 'tab', 2), ('h', 'host_c0'), ('o', 'out', N),
                             ('n', 'n', N)], bad=[dict(theta=0), dict(theta=65), dict(host_c0=0), dict(stride=N - 1)]),
    # three exponent bits: one window of 15 table entries
    'ffgm_pow_base': dict(p=[('i', 'x', N), ('n', 'shift', 1), ('n', 'ebits', 3), ('i', 'tab', 15), ('o', 'out', N), ('n', 'n', N)],
                          bad=[dict(shift=-1), dict(shift=192), dict(ebits=0), dict(ebits=193)], pbits='ebits'),
    'ffgm_bits_reverse': dict(p=[('i', 'bits', N * LB), ('n', 'l', LB), ('o', 'out', N * LB), ('n', 'n', N)], bad=[dict(l=0), dict(l=65)]),
    'ffgm_iszero_mask': dict(p=[('i', 'a', N), ('i', 'r', N * W2), ('i', 'z', N * W2), ('i', 'u2', N * W2), ('n', 'k', W2), ('o', 'out', N * W2),
                                ('n', 'n', N)], bad=[dict(k=0), dict(k=-1)]),
    'ffgm_legendre_code': dict(p=[('i', 'c', N), ('o', 'code', -N), ('n', 'count', N)], bad=[], size='count'),
    'ffgm_iszero_finish': dict(p=[('i', 'code', -N), ('i', 'z', N), ('o', 'out', N), ('n', 'count', N)], bad=[], size='count'),
    'ffgm_rbits_open': dict(p=[('R', 'host_r', 'k', N), ('R', 'host_z', 'k', N), ('h', 'host_lambda'), ('n', 'k', 3), ('o', 'out', N),
                               ('o?', 'zeros', -4), ('n', 'n', N)], bad=[], count=('k', 64)),
    'ffgm_rbits_finish': dict(p=[('i', 'c', N), ('R', 'host_r', 'm', N), ('W', 'host_b', 'm', N), ('n', 'm', 3), ('n', 'is_signed', 0), ('n', 'f', 4),
                                 ('n', 'n', N)], bad=[dict(f=-1), dict(f=192)], count=('m', 64)),
    'ffgm_bsgn_mask': dict(p=[('i', 'a', N), ('i', 'z', N * W2), ('h', 'host_alpha'), ('h', 'host_beta'), ('n', 'w', W2), ('o', 'out', N * W2),
                              ('n', 'n', N)], bad=[dict(w=0), dict(w=9)]),
    'ffgm_bsgn_finish': dict(p=[('i', 'c', N * W2), ('R', 'host_s', 'm', N * W2), ('W', 'host_out', 'm', N * W2), ('n', 'm', 3), ('n', 'w', W2),
                                ('n', 'sum', 0), ('n', 'n', N)], bad=[dict(w=0), dict(w=9), dict(sum=2), dict(sum=-1)], count=('m', 64)),
    'ffgm_unit_prod': dict(p=[('i', 'x', N), ('n', 'xstride', 1), ('i', 'U', 2 * N), ('n', 'h', 2), ('o', 'out', 2 * N), ('n', 'n', N)],
                           bad=[dict(h=0), dict(xstride=0)]),
    'ffgm_unit_roll': dict(p=[('i', 'U', 4 * N), ('i', 'c', N), ('n', 'kbits', 2), ('n', 'K', 3), ('o', 'out', 3 * N), ('n', 'n', N)],
                           bad=[dict(kbits=-1), dict(kbits=31), dict(K=0), dict(K=5)]),
    'ffgm_unit_dot': dict(p=[('i', 'U', 4 * N), ('n', 'rows', 4), ('i?', 'c', N), ('n', 'kbits', 2), ('i', 'tab', 3), ('n', 'tlen', 3), ('o', 'out', N),
                             ('n', 'n', N)], bad=[dict(rows=0), dict(tlen=0), dict(tlen=5), dict(rows=3), dict(kbits=31), dict(c=0)]),
    # one image of 2 channels of 4 x 4, 2 output channels, 3 x 3 taps
    'ffgm_conv2d': dict(p=[('R', 'host_x', 'nsend', 32), ('R', 'host_w', 'nsend', 36), ('R?', 'host_b', 'nsend', 2), ('W', 'host_out', 'nsend', 32),
                           ('n', 'nsend', 3), ('n', 'k', 1), ('n', 'r', 2), ('n', 'm', 4), ('n', 'n', 4), ('n', 'v', 2), ('n', 's', 3)],
                        bad=[dict(s=0), dict(s=5), dict(s=99), dict(r=0)], size='k', empty=dict(k=0), count=('nsend', 64)),
}
# the calls that are not one fault of the description, or one of the pairs secure_cases() forms for every entry
SECURE_EXTRA = {
    'ffgpu_sgn_expand': [('sbit=NULL, only nx and z, empty', dict(sbit=0, e_out=0, n=0))],
    'ffgm_unit_dot': [('table too large', dict(c=0, rows=1 << 20, tlen=1 << 20)),
                      ('table too large + empty', dict(c=0, rows=1 << 20, tlen=1 << 20, n=0)),
                      ('table too large + null pointer', dict(c=0, rows=1 << 20, tlen=1 << 20, U=0)),
                      ('table too large + bad scalar', dict(c=0, rows=1 << 20, tlen=(1 << 20) + 1))],
    'ffgm_conv2d': [('empty + grid refused', dict(k=1 << 30, r=1, m=64, n=64, v=0)), ('grid refused', dict(k=1 << 30, r=1, m=64, n=64, v=1)),
                    ('grid refused + null pointer', dict(k=1 << 30, r=1, m=64, n=64, v=1, host_x=0)),
                    ('no bias, null row of x', dict(host_b=0, host_x='hole')), ('s > n', dict(s=3, n=2))],
    'ffgm_rbits_finish': [('in place but one element apart', dict(host_b='host_r+1'))],
}


def secure_cases(eb, bits, entry):
    """(label, context or None for the prime one, arguments after the context) of every call of the table for `entry`, for a prime
    context of eb-byte elements and a modulus of `bits` bits"""
    spec = SECURE[entry]
    params = spec['p']
    size = spec.get('size', 'n')
    empty = spec.get('empty', {size: 0})
    count, limit = spec.get('count', (None, 0))
    names = [q[1] for q in params]
    default = {q[1]: q[2] for q in params if q[0] == 'n'}
    base = {name: 0x100000000000 + i * 0x100000000 for i, name in enumerate(names)}
    nbytes = {q[1]: (q[-1] * eb if q[-1] > 0 else -q[-1]) for q in params if q[0] != 'n' and q[0] != 'h'}
    unit = {q[1]: (eb if q[-1] > 0 else 1) for q in params if q[0] != 'n' and q[0] != 'h'}
    arrays = [q[1] for q in params if q[0] in ('R', 'R?', 'W')]
    ins = [q[1] for q in params if q[0] in ('i', 'i?', 'R', 'R?')]
    outs = [q[1] for q in params if q[0] in ('o', 'o?', 'io', 'W')]
    required = [q[1] for q in params if q[0] in ('i', 'o', 'io', 'R', 'W', 'h')]

    def build(over):
        """the argument list: defaults, then `over` (a pointer: 0 for null, an address, 'hole' for an array with a null in it)"""
        over = dict(over)
        rows = {}
        for q in params:
            if q[0] in ('R', 'R?', 'W'):
                addr = [base[q[1]] + j * 0x1000000 for j in range(80)]
                rows[q[1]] = addr
        args = []
        for q in params:
            kind, name = q[0], q[1]
            v = over.get(name, None)
            if kind == 'n':
                args.append(q[2] if v is None else v)
            elif kind == 'h':
                args.append(None if v == 0 else (ctypes.c_uint64 * (3 * 80))(*([1, 0, 0] * 80)))
            elif kind in ('R', 'R?', 'W'):
                addr = rows[name]
                if v == 0:
                    args.append(None)
                    continue
                if v == 'hole':
                    addr[over.get(q[2], default[q[2]]) - 1] = None
                elif isinstance(v, str):                    # 'other+1': row i is row i of `other`, one element further
                    addr = [a + eb for a in rows[v.split('+')[0]]]
                elif isinstance(v, dict):                   # {row: address}
                    for j, a in v.items():
                        addr[j] = a
                args.append((ctypes.c_void_p * 80)(*addr))
            else:
                args.append(base[name] if v is None else (v or None))
        return args + [None]

    def first(name):                                        # the address of an array, or of row 0 of an array of pointers
        return base[name]

    def moved(name, to):                                    # `name` (or its row 0) at address `to`
        return {name: {0: to} if name in arrays else to}

    cases = [('gf256', None)]
    for b in spec['bad']:
        cases.append((' '.join(f'{k}={v}' for k, v in b.items()), b))
    nulls = {q[1]: 0 for q in params if q[0] != 'n'}
    cases.append(('empty, every pointer null', dict(empty, **nulls)))
    cases += [(f'{name}=NULL', {name: 0}) for name in required]
    cases += [(f'null inside {name}', {name: 'hole'}) for name in arrays]
    cases += [(f'{size}=2^62', {size: 1 << 62}), (f'{size}=2^58', {size: 1 << 58})]
    overlap = None
    for o in outs:
        for i in ins:
            over = moved(o, first(i) + nbytes[i] - unit[i])
            cases.append((f'{o} at the last element of {i}', over))
            overlap = overlap or over
        for o2 in outs[outs.index(o) + 1:]:
            cases.append((f'{o2} at the last element of {o}', moved(o2, first(o) + nbytes[o] - unit[o])))
    for a in arrays:
        if len([q for q in params if q[1] == a and q[0] == 'W']):
            cases.append((f'row 1 of {a} at the last element of row 0', {a: {1: first(a) + nbytes[a] - unit[a]}}))
    bad = spec['bad'][0] if spec['bad'] else None
    if bad:
        cases.append(('gf256 + bad scalar', ('gf256', bad)))
    if count:
        above, none = {count: limit + 1}, {count: 0}
        cases += [(f'{count}=0', none), (f'{count}=-1', {count: -1}), (f'{count}={limit} + empty', dict(empty, **{count: limit})),
                  (f'{count}={limit + 1}', above), (f'{count}={limit + 1} + empty', dict(empty, **above)), (f'{count}=0 + empty', dict(empty, **none)),
                  (f'{count}={limit + 1} + null pointer', dict(above, **{required[0]: 0})),
                  (f'{count}={limit + 1} + null in row {limit}', dict(above, **{arrays[0]: {limit: None}})),
                  (f'{count}={limit + 1} + null in row 0', dict(above, **{arrays[0]: {0: None}})),
                  (f'{count}={limit + 1} + overlap', dict(above, **overlap))]
        if bad:
            cases += [(f'{count}={limit + 1} + bad scalar', dict(above, **bad)), (f'{count}=0 + bad scalar', dict(none, **bad))]
    if 'lbits' in spec:                                     # 1 <= l <= 64 and l <= bit_length(p) - 2
        l = spec['lbits']
        cases += [(f'{l}=min(bits-2,64) + empty', dict(empty, **{l: min(bits - 2, 64)})), (f'{l}=bits-1 + empty', dict(empty, **{l: bits - 1}))]
    if 'pbits' in spec:                                     # at most the bits of the modulus
        cases += [(f'ebits=bits + empty', dict(empty, ebits=bits)), (f'ebits=bits+1 + empty', dict(empty, ebits=bits + 1))]
    cases += SECURE_EXTRA.get(entry, [])
    for label, over in cases:
        if over is None:
            yield label, 'gf256', build({})
        elif isinstance(over, tuple):
            yield label, 'gf256', build(over[1])
        else:
            yield label, None, build(over)


def secure_statuses(L):
    """{entry: {label: status letters}}: I for FFGPU_EINVAL, N for FFGPU_ENOTSUP, 0 for FFGPU_OK (an empty call), one letter per
    context of SECURE_CONTEXTS, or a single letter when the four agree"""
    from mpyc_amd import _ffi
    letter = {_ffi.OK: '0', _ffi.EINVAL: 'I', _ffi.ENOTSUP: 'N'}
    hb = mk(L, _ffi.BINARY, 0x11b)[1]
    ctxs = [(mk(L, _ffi.PRIME, p)[1], p.bit_length()) for p in SECURE_CONTEXTS]
    got = {}
    for entry in SECURE:
        fn = getattr(L, entry)
        rows = {}
        for h, bits in ctxs:
            eb = L.ffgpu_ctx_elem_bytes(h)
            for label, ctx, args in [('ctx=NULL', 'null', next(secure_cases(eb, bits, entry))[2])] + list(secure_cases(eb, bits, entry)):
                rc = fn({'null': None, 'gf256': hb, None: h}[ctx], *args)
                rows.setdefault(label, []).append(letter.get(rc, f'<{rc}>'))
        got[entry] = {label: (s[0] if len(set(s)) == 1 else ''.join(s)) for label, s in rows.items()}
    for h, _ in ctxs:
        L.ffgpu_ctx_destroy(h)
    L.ffgpu_ctx_destroy(hb)
    return got


# The answers of the library before the entries stated their arrays on one operand type and took their integers from one host
# integer (recorded from a build of that commit), so that such a change of the host layer cannot move them.
SECURE_STATUS = {
    'ffgpu_sgn_mask': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'l=65': 'I', 'empty, every pointer null': '0', 'a=NULL': 'I', 'rbits=NULL': 'I',
        'rdivl=NULL': 'I', 'masked=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'masked at the last element of a': 'I',
        'masked at the last element of rbits': 'I', 'masked at the last element of rdivl': 'I', 'gf256 + bad scalar': 'N',
        'l=min(bits-2,64) + empty': '0', 'l=bits-1 + empty': 'I',
    },
    'ffgpu_sgn_expand': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'l=65': 'I', 'e_out=0 nx_out=0 z_out=0': 'I', 'sbit=0': 'I',
        'empty, every pointer null': 'I', 'c=NULL': 'I', 'a=NULL': 'I', 'rbits=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'e_out at the last element of c': 'I', 'e_out at the last element of a': 'I', 'e_out at the last element of rbits': 'I',
        'e_out at the last element of sbit': 'I', 'nx_out at the last element of e_out': 'I', 'z_out at the last element of e_out': 'I',
        'nx_out at the last element of c': 'I', 'nx_out at the last element of a': 'I', 'nx_out at the last element of rbits': 'I',
        'nx_out at the last element of sbit': 'I', 'z_out at the last element of nx_out': 'I', 'z_out at the last element of c': 'I',
        'z_out at the last element of a': 'I', 'z_out at the last element of rbits': 'I', 'z_out at the last element of sbit': 'I',
        'gf256 + bad scalar': 'N', 'l=min(bits-2,64) + empty': '0', 'l=bits-1 + empty': 'I', 'sbit=NULL, only nx and z, empty': '0',
    },
    'ffgpu_sgn_finish': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'l=65': 'I', 'empty, every pointer null': '0', 'w=NULL': 'I', 'sbit=NULL': 'I',
        'z=NULL': 'I', 'lt_out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'lt_out at the last element of w': 'I',
        'lt_out at the last element of sbit': 'I', 'lt_out at the last element of z': 'I', 'gf256 + bad scalar': 'N',
        'l=min(bits-2,64) + empty': '0', 'l=bits-1 + empty': 'I',
    },
    'ffgpu_cx_diff': {
        'ctx=NULL': 'I', 'gf256': 'N', 'p=3': 'I', 'd=2': 'I', 'r=2': 'I', 'k=1': 'I', 'k=0': 'I', 'empty, every pointer null': '0',
        'a=NULL': 'I', 'out=NULL': 'I', 'outer=2^62': 'I', 'outer=2^58': 'I', 'out at the last element of a': 'I',
        'gf256 + bad scalar': 'N',
    },
    'ffgpu_cx_apply': {
        'ctx=NULL': 'I', 'gf256': 'N', 'p=3': 'I', 'd=2': 'I', 'k=1': 'I', 'empty, every pointer null': '0', 'a=NULL': 'I',
        'host_rows=NULL': 'I', 'host_lambda=NULL': 'I', 'null inside host_rows': 'I', 'outer=2^62': 'I', 'outer=2^58': 'I',
        'a at the last element of host_rows': 'I', 'gf256 + bad scalar': 'N', 'nrows=0': 'I', 'nrows=-1': 'I', 'nrows=9 + empty': '0',
        'nrows=10': 'N', 'nrows=10 + empty': '0', 'nrows=0 + empty': 'I', 'nrows=10 + null pointer': 'I', 'nrows=10 + null in row 9': 'N',
        'nrows=10 + null in row 0': 'I', 'nrows=10 + overlap': 'I', 'nrows=10 + bad scalar': 'I', 'nrows=0 + bad scalar': 'I',
    },
    'ffgpu_tour_diff': {
        'ctx=NULL': 'I', 'gf256': 'N', 'mode=2': 'I', 'mode=-1': 'I', 'k=1': 'I', 'empty, every pointer null': '0', 'a=NULL': 'I',
        'out=NULL': 'I', 'outer=2^62': 'I', 'outer=2^58': 'I', 'out at the last element of a': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgpu_tour_select': {
        'ctx=NULL': 'I', 'gf256': 'N', 'mode=2': 'I', 'k=1': 'I', 'empty, every pointer null': '0', 'a=NULL': 'I', 'host_rows=NULL': 'I',
        'host_lambda=NULL': 'I', 'out=NULL': 'I', 'null inside host_rows': 'I', 'outer=2^62': 'I', 'outer=2^58': 'I',
        'out at the last element of a': 'I', 'out at the last element of host_rows': 'I', 'gf256 + bad scalar': 'N', 'nrows=0': 'I',
        'nrows=-1': 'I', 'nrows=9 + empty': '0', 'nrows=10': 'N', 'nrows=10 + empty': '0', 'nrows=0 + empty': 'I',
        'nrows=10 + null pointer': 'I', 'nrows=10 + null in row 9': 'N', 'nrows=10 + null in row 0': 'I', 'nrows=10 + overlap': 'I',
        'nrows=10 + bad scalar': 'I', 'nrows=0 + bad scalar': 'I',
    },
    'ffgpu_tour_unit_prod': {
        'ctx=NULL': 'I', 'gf256': 'N', 'k=1': 'I', 'k=0': 'I', 'empty, every pointer null': '0', 'u=NULL': 'I', 'c=NULL': 'I',
        'out=NULL': 'I', 'outer=2^62': 'I', 'outer=2^58': 'I', 'out at the last element of u': 'I', 'out at the last element of c': 'I',
        'gf256 + bad scalar': 'N',
    },
    'ffgpu_tour_unit_expand': {
        'ctx=NULL': 'I', 'gf256': 'N', 'k=1': 'I', 'empty, every pointer null': '0', 'u=NULL': 'I', 'host_rows=NULL': 'I',
        'host_lambda=NULL': 'I', 'out=NULL': 'I', 'null inside host_rows': 'I', 'outer=2^62': 'I', 'outer=2^58': 'I',
        'out at the last element of u': 'I', 'out at the last element of host_rows': 'I', 'gf256 + bad scalar': 'N', 'nrows=0': 'I',
        'nrows=-1': 'I', 'nrows=9 + empty': '0', 'nrows=10': 'N', 'nrows=10 + empty': '0', 'nrows=0 + empty': 'I',
        'nrows=10 + null pointer': 'I', 'nrows=10 + null in row 9': 'N', 'nrows=10 + null in row 0': 'I', 'nrows=10 + overlap': 'I',
        'nrows=10 + bad scalar': 'I', 'nrows=0 + bad scalar': 'I',
    },
    'ffgpu_find_leaf_prod': {
        'ctx=NULL': 'I', 'gf256': 'N', 'ncomp=1': 'I', 'ncomp=6': 'I', 'flip=2': 'I', 'virt=2': 'I', 'k=1': 'I', 'k=0 virt=1': 'I',
        'empty, every pointer null': '0', 'bits=NULL': 'I', 'tab=NULL': 'I', 'out=NULL': 'I', 'outer=2^62': 'I', 'outer=2^58': 'I',
        'out at the last element of bits': 'I', 'out at the last element of tab': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgpu_find_leaf_apply': {
        'ctx=NULL': 'I', 'gf256': 'N', 'ncomp=1': 'I', 'flip=-1': 'I', 'virt=2': 'I', 'k=1': 'I', 'empty, every pointer null': '0',
        'bits=NULL': 'I', 'tab=NULL': 'I', 'host_rows=NULL': 'I', 'host_lambda=NULL': 'I', 'out=NULL': 'I', 'null inside host_rows': 'I',
        'outer=2^62': 'I', 'outer=2^58': 'I', 'out at the last element of bits': 'I', 'out at the last element of tab': 'I',
        'out at the last element of host_rows': 'I', 'gf256 + bad scalar': 'N', 'nrows=0': 'N', 'nrows=-1': 'N', 'nrows=9 + empty': '0',
        'nrows=10': 'N', 'nrows=10 + empty': 'N', 'nrows=0 + empty': 'N', 'nrows=10 + null pointer': 'N', 'nrows=10 + null in row 9': 'N',
        'nrows=10 + null in row 0': 'N', 'nrows=10 + overlap': 'N', 'nrows=10 + bad scalar': 'N', 'nrows=0 + bad scalar': 'N',
    },
    'ffgpu_find_prod': {
        'ctx=NULL': 'I', 'gf256': 'N', 'ncomp=1': 'I', 'ncomp=6': 'I', 'k=1': 'I', 'empty, every pointer null': '0', 'level=NULL': 'I',
        'out=NULL': 'I', 'outer=2^62': 'I', 'outer=2^58': 'I', 'out at the last element of level': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgpu_bits_mask': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'l=65': 'I', 'host_offset=0': 'I', 'empty, every pointer null': 'I', 'a=NULL': 'I',
        'rbits=NULL': 'I', 'rdivl=NULL': 'I', 'host_offset=NULL': 'I', 'masked=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'masked at the last element of a': 'I', 'masked at the last element of rbits': 'I', 'masked at the last element of rdivl': 'I',
        'gf256 + bad scalar': 'N', 'l=min(bits-2,64) + empty': '0', 'l=bits-1 + empty': 'I',
    },
    'ffgpu_bits_expand': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'l=65': 'I', 'empty, every pointer null': '0', 'c=NULL': 'I', 'rbits=NULL': 'I',
        'g_out=NULL': 'I', 'p_out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'g_out at the last element of c': 'I',
        'g_out at the last element of rbits': 'I', 'p_out at the last element of g_out': 'I', 'p_out at the last element of c': 'I',
        'p_out at the last element of rbits': 'I', 'gf256 + bad scalar': 'N', 'l=min(bits-2,64) + empty': '0', 'l=bits-1 + empty': 'I',
    },
    'ffgpu_carry_prod': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'l=65': 'I', 'round=0': 'I', 'round=2': 'I', 'empty, every pointer null': '0',
        'g=NULL': 'I', 'p=NULL': 'I', 'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of g': 'I',
        'out at the last element of p': 'I', 'gf256 + bad scalar': 'N', 'l=min(bits-2,64) + empty': '0', 'l=bits-1 + empty': 'I',
    },
    'ffgpu_carry_apply': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'round=0': 'I', 'round=2': 'I', 'empty, every pointer null': '0', 'g=NULL': 'I',
        'p=NULL': 'I', 'host_rows=NULL': 'I', 'host_lambda=NULL': 'I', 'null inside host_rows': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'g at the last element of host_rows': 'I', 'p at the last element of g': 'I', 'p at the last element of host_rows': 'I',
        'gf256 + bad scalar': 'N', 'nrows=0': 'I', 'nrows=-1': 'I', 'nrows=9 + empty': '0', 'nrows=10': 'N', 'nrows=10 + empty': '0',
        'nrows=0 + empty': 'I', 'nrows=10 + null pointer': 'I', 'nrows=10 + null in row 9': 'N', 'nrows=10 + null in row 0': 'I',
        'nrows=10 + overlap': 'I', 'nrows=10 + bad scalar': 'I', 'nrows=0 + bad scalar': 'I', 'l=min(bits-2,64) + empty': '0',
        'l=bits-1 + empty': 'I',
    },
    'ffgpu_bits_finish': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'l=65': 'I', 'empty, every pointer null': '0', 'c=NULL': 'I', 'rbits=NULL': 'I',
        'g=NULL': 'I', 'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of c': 'I',
        'out at the last element of rbits': 'I', 'out at the last element of g': 'I', 'gf256 + bad scalar': 'N',
        'l=min(bits-2,64) + empty': '0', 'l=bits-1 + empty': 'I',
    },
    'ffgpu_trunc_mask': {
        'ctx=NULL': 'I', 'gf256': 'N', 'f=0': 'I', 'f=65': 'I', 'host_offset=0': 'I', 'empty, every pointer null': 'I', 'a=NULL': 'I',
        'rbits=NULL': 'I', 'rdivf=NULL': 'I', 'host_offset=NULL': 'I', 'ar_out=NULL': 'I', 'masked_out=NULL': 'I', 'n=2^62': 'I',
        'n=2^58': 'I', 'ar_out at the last element of a': 'I', 'ar_out at the last element of rbits': 'I',
        'ar_out at the last element of rdivf': 'I', 'masked_out at the last element of ar_out': 'I',
        'masked_out at the last element of a': 'I', 'masked_out at the last element of rbits': 'I',
        'masked_out at the last element of rdivf': 'I', 'gf256 + bad scalar': 'N', 'f=min(bits-2,64) + empty': '0', 'f=bits-1 + empty': 'I',
    },
    'ffgpu_trunc_finish': {
        'ctx=NULL': 'I', 'gf256': 'N', 'f=0': 'I', 'f=65': 'I', 'empty, every pointer null': '0', 'host_rows=NULL': 'I',
        'host_lambda=NULL': 'I', 'ar=NULL': 'I', 'out=NULL': 'I', 'null inside host_rows': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'out at the last element of host_rows': 'I', 'out at the last element of ar': 'I', 'gf256 + bad scalar': 'N', 'nrows=0': 'I',
        'nrows=-1': 'I', 'nrows=9 + empty': '0', 'nrows=10': 'N', 'nrows=10 + empty': 'N', 'nrows=0 + empty': 'I',
        'nrows=10 + null pointer': 'N', 'nrows=10 + null in row 9': 'N', 'nrows=10 + null in row 0': 'N', 'nrows=10 + overlap': 'N',
        'nrows=10 + bad scalar': 'N', 'nrows=0 + bad scalar': 'I', 'f=min(bits-2,64) + empty': '0', 'f=bits-1 + empty': 'I',
    },
    'ffgpu_norm_prod': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=1': 'I', 'l=65': 'I', 'empty, every pointer null': '0', 'bits=NULL': 'I', 'out=NULL': 'I',
        'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of bits': 'I', 'sign_out at the last element of out': 'I',
        'sign_out at the last element of bits': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgpu_norm_apply': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=1': 'I', 'l=65': 'I', 'empty, every pointer null': '0', 'bits=NULL': 'I', 'host_rows=NULL': 'I',
        'host_lambda=NULL': 'I', 'out=NULL': 'I', 'null inside host_rows': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'out at the last element of bits': 'I', 'out at the last element of host_rows': 'I', 'gf256 + bad scalar': 'N', 'nrows=0': 'I',
        'nrows=-1': 'I', 'nrows=9 + empty': '0', 'nrows=10': 'N', 'nrows=10 + empty': 'N', 'nrows=0 + empty': 'I',
        'nrows=10 + null pointer': 'N', 'nrows=10 + null in row 9': 'N', 'nrows=10 + null in row 0': 'N', 'nrows=10 + overlap': 'N',
        'nrows=10 + bad scalar': 'N', 'nrows=0 + bad scalar': 'I',
    },
    'ffgm_powers_prod': {
        'ctx=NULL': 'I', 'gf256': 'N', 'h=0': 'I', 'w=0': 'I', 'w=3': 'I', 'stride=7': 'I', 'empty, every pointer null': '0', 'P=NULL': 'I',
        'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of P': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgm_poly_dot': {
        'ctx=NULL': 'I', 'gf256': 'N', 'theta=0': 'I', 'theta=65': 'I', 'host_c0=0': 'I', 'stride=7': 'I', 'empty, every pointer null': 'I',
        'P=NULL': 'I', 'tab=NULL': 'I', 'host_c0=NULL': 'I', 'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'out at the last element of P': 'I', 'out at the last element of tab': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgm_pow_base': {
        'ctx=NULL': 'I', 'gf256': 'N', 'shift=-1': 'I', 'shift=192': 'I', 'ebits=0': 'I', 'ebits=193': 'I',
        'empty, every pointer null': '0', 'x=NULL': 'I', 'tab=NULL': 'I', 'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'out at the last element of x': 'I', 'out at the last element of tab': 'I', 'gf256 + bad scalar': 'N', 'ebits=bits + empty': '0',
        'ebits=bits+1 + empty': 'I',
    },
    'ffgm_bits_reverse': {
        'ctx=NULL': 'I', 'gf256': 'N', 'l=0': 'I', 'l=65': 'I', 'empty, every pointer null': '0', 'bits=NULL': 'I', 'out=NULL': 'I',
        'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of bits': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgm_iszero_mask': {
        'ctx=NULL': 'I', 'gf256': 'N', 'k=0': 'I', 'k=-1': 'I', 'empty, every pointer null': '0', 'a=NULL': 'I', 'r=NULL': 'I',
        'z=NULL': 'I', 'u2=NULL': 'I', 'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of a': 'I',
        'out at the last element of r': 'I', 'out at the last element of z': 'I', 'out at the last element of u2': 'I',
        'gf256 + bad scalar': 'N',
    },
    'ffgm_legendre_code': {
        'ctx=NULL': 'I', 'gf256': 'N', 'empty, every pointer null': '0', 'c=NULL': 'I', 'code=NULL': 'I', 'count=2^62': 'I',
        'count=2^58': 'I', 'code at the last element of c': 'I',
    },
    'ffgm_iszero_finish': {
        'ctx=NULL': 'I', 'gf256': 'N', 'empty, every pointer null': '0', 'code=NULL': 'I', 'z=NULL': 'I', 'out=NULL': 'I',
        'count=2^62': 'I', 'count=2^58': 'I', 'out at the last element of code': 'I', 'out at the last element of z': 'I',
    },
    'ffgm_rbits_open': {
        'ctx=NULL': 'I', 'gf256': 'N', 'empty, every pointer null': '0', 'host_r=NULL': 'I', 'host_z=NULL': 'I', 'host_lambda=NULL': 'I',
        'out=NULL': 'I', 'null inside host_r': 'I', 'null inside host_z': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'out at the last element of host_r': 'I', 'out at the last element of host_z': 'I', 'zeros at the last element of out': 'I',
        'zeros at the last element of host_r': 'I', 'zeros at the last element of host_z': 'I', 'k=0': 'I', 'k=-1': 'I',
        'k=64 + empty': '0', 'k=65': 'N', 'k=65 + empty': 'N', 'k=0 + empty': 'I', 'k=65 + null pointer': 'N', 'k=65 + null in row 64': 'N',
        'k=65 + null in row 0': 'N', 'k=65 + overlap': 'N',
    },
    'ffgm_rbits_finish': {
        'ctx=NULL': 'I', 'gf256': 'N', 'f=-1': 'IIIN', 'f=192': 'IIIN', 'empty, every pointer null': '000N', 'c=NULL': 'IIIN',
        'host_r=NULL': 'IIIN', 'host_b=NULL': 'IIIN', 'null inside host_r': 'IIIN', 'null inside host_b': 'IIIN', 'n=2^62': 'IIIN',
        'n=2^58': 'IIIN', 'host_b at the last element of c': 'IIIN', 'host_b at the last element of host_r': 'IIIN',
        'row 1 of host_b at the last element of row 0': 'IIIN', 'gf256 + bad scalar': 'N', 'm=0': 'IIIN', 'm=-1': 'IIIN',
        'm=64 + empty': '000N', 'm=65': 'N', 'm=65 + empty': 'N', 'm=0 + empty': 'IIIN', 'm=65 + null pointer': 'N',
        'm=65 + null in row 64': 'N', 'm=65 + null in row 0': 'N', 'm=65 + overlap': 'N', 'm=65 + bad scalar': 'IIIN',
        'm=0 + bad scalar': 'IIIN', 'in place but one element apart': 'IIIN',
    },
    'ffgm_bsgn_mask': {
        'ctx=NULL': 'I', 'gf256': 'N', 'w=0': 'I', 'w=9': 'I', 'empty, every pointer null': '0', 'a=NULL': 'I', 'z=NULL': 'I',
        'host_alpha=NULL': 'I', 'host_beta=NULL': 'I', 'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of a': 'I',
        'out at the last element of z': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgm_bsgn_finish': {
        'ctx=NULL': 'I', 'gf256': 'N', 'w=0': 'I', 'w=9': 'I', 'sum=2': 'I', 'sum=-1': 'I', 'empty, every pointer null': '0', 'c=NULL': 'I',
        'host_s=NULL': 'I', 'host_out=NULL': 'I', 'null inside host_s': 'I', 'null inside host_out': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'host_out at the last element of c': 'I', 'host_out at the last element of host_s': 'I',
        'row 1 of host_out at the last element of row 0': 'I', 'gf256 + bad scalar': 'N', 'm=0': 'I', 'm=-1': 'I', 'm=64 + empty': '0',
        'm=65': 'N', 'm=65 + empty': 'N', 'm=0 + empty': 'I', 'm=65 + null pointer': 'N', 'm=65 + null in row 64': 'N',
        'm=65 + null in row 0': 'N', 'm=65 + overlap': 'N', 'm=65 + bad scalar': 'I', 'm=0 + bad scalar': 'I',
    },
    'ffgm_unit_prod': {
        'ctx=NULL': 'I', 'gf256': 'N', 'h=0': 'I', 'xstride=0': 'I', 'empty, every pointer null': '0', 'x=NULL': 'I', 'U=NULL': 'I',
        'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of x': 'I', 'out at the last element of U': 'I',
        'gf256 + bad scalar': 'N',
    },
    'ffgm_unit_roll': {
        'ctx=NULL': 'I', 'gf256': 'N', 'kbits=-1': 'I', 'kbits=31': 'I', 'K=0': 'I', 'K=5': 'I', 'empty, every pointer null': '0',
        'U=NULL': 'I', 'c=NULL': 'I', 'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I', 'out at the last element of U': 'I',
        'out at the last element of c': 'I', 'gf256 + bad scalar': 'N',
    },
    'ffgm_unit_dot': {
        'ctx=NULL': 'I', 'gf256': 'N', 'rows=0': 'I', 'tlen=0': 'I', 'tlen=5': 'I', 'rows=3': 'I', 'kbits=31': 'I', 'c=0': 'I',
        'empty, every pointer null': 'I', 'U=NULL': 'I', 'tab=NULL': 'I', 'out=NULL': 'I', 'n=2^62': 'I', 'n=2^58': 'I',
        'out at the last element of U': 'I', 'out at the last element of c': 'I', 'out at the last element of tab': 'I',
        'gf256 + bad scalar': 'N', 'table too large': 'N', 'table too large + empty': 'N', 'table too large + null pointer': 'N',
        'table too large + bad scalar': 'I',
    },
    'ffgm_conv2d': {
        'ctx=NULL': 'I', 'gf256': 'N', 's=0': 'I', 's=5': 'I', 's=99': 'I', 'r=0': 'I', 'empty, every pointer null': '0',
        'host_x=NULL': 'I', 'host_w=NULL': 'I', 'host_out=NULL': 'I', 'null inside host_x': 'I', 'null inside host_w': 'I',
        'null inside host_b': 'I', 'null inside host_out': 'I', 'k=2^62': 'I', 'k=2^58': 'I', 'host_out at the last element of host_x': 'I',
        'host_out at the last element of host_w': 'I', 'host_out at the last element of host_b': 'I',
        'row 1 of host_out at the last element of row 0': 'I', 'gf256 + bad scalar': 'N', 'nsend=0': 'I', 'nsend=-1': 'I',
        'nsend=64 + empty': '0', 'nsend=65': 'N', 'nsend=65 + empty': 'N', 'nsend=0 + empty': 'I', 'nsend=65 + null pointer': 'N',
        'nsend=65 + null in row 64': 'N', 'nsend=65 + null in row 0': 'N', 'nsend=65 + overlap': 'N', 'nsend=65 + bad scalar': 'N',
        'nsend=0 + bad scalar': 'I', 'empty + grid refused': '0', 'grid refused': 'N', 'grid refused + null pointer': 'N',
        'no bias, null row of x': 'I', 's > n': 'I',
    },
}
