"""The six ffgpu_gf256_* entry points (include/ffgpu.h; kernels in mpyc_amd/csrc/misc.hip) on every path, byte for byte against
the Python-integer references of tests/gf256_contract.py, through the C ABI (ctx._L) with raw pointers: every output lies inside a
buffer of 0xa5 guards (240 bytes on both sides, and in the padding of strided rows) that is compared whole, inputs keep their
bytes, a refused call leaves a pre-filled output as it was.  Capped grids: a context of its own under FFGPU_BLOCKS_PER_CU=1 and
the smallest n at which thread 0 takes three trips, computed from the device's CU count and asserted.

tests/test_gf256_contract_host.py holds the references against each other and against tests/golden/sbox.json on the CPU.
Expected values never come from the library."""
import ctypes
import random
import time

import numpy as np
import pytest

import gf256_contract as gc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

PAD, GUARD = gc.PAD, gc.GUARD
F8 = gc.field(gc.AES)
KEY = bytes(range(100, 132))
_ctxs = {}
STATS = {'cases': 0, 'max_bytes': 0}


def default_ctx(modulus, binary=True):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from mpyc_amd import engine
    if (modulus, binary) not in _ctxs:
        _ctxs[modulus, binary] = engine.FieldContext(modulus, binary, device=0)
    return _ctxs[modulus, binary]


def capped_ctx(monkeypatch, modulus):
    """a context of its own under FFGPU_BLOCKS_PER_CU=1 (the launch switches are read at creation)"""
    from mpyc_amd import engine
    monkeypatch.setenv('FFGPU_BLOCKS_PER_CU', '1')
    ctx = engine.FieldContext(modulus, True, device=0)
    monkeypatch.delenv('FFGPU_BLOCKS_PER_CU')
    return ctx


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def status():
    from mpyc_amd import _ffi
    return _ffi.OK, _ffi.EINVAL, _ffi.ENOTSUP


class Buf:
    """bytes on the device at a chosen offset from a 256-byte aligned base"""

    def __init__(self, data, off=0):
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1))
        self.off, self.n = off, data.size
        self.t = torch.full((off + data.size + 16,), 0x5a, dtype=torch.uint8, device='cuda')
        assert self.t.data_ptr() % 256 == 0
        self.t[off:off + data.size] = torch.from_numpy(data).to('cuda')
        self.before = self.t.clone()
        STATS['max_bytes'] = max(STATS['max_bytes'], self.t.numel())

    @property
    def ptr(self):
        return self.t.data_ptr() + self.off

    def untouched(self):
        return torch.equal(self.t, self.before)


class Out:
    """`count` output bytes at offset `off` from a 16-byte aligned address, guards all around; rows: (nrows, row bytes, stride)"""

    def __init__(self, count, off=0, fill=GUARD):
        self.off, self.count, self.fill = off, count, fill
        self.t = torch.full((PAD + off + count + PAD,), fill, dtype=torch.uint8, device='cuda')
        assert self.t.data_ptr() % 256 == 0 and PAD % 16 == 0
        STATS['max_bytes'] = max(STATS['max_bytes'], self.t.numel())

    @property
    def ptr(self):
        return self.t.data_ptr() + PAD + self.off

    def check(self, want, what, rows=None):
        """the whole buffer: guards, the output, and with rows = (nrows, nbytes, stride) the padding between rows"""
        exp = torch.full_like(self.t, self.fill)
        want = torch.as_tensor(np.asarray(want, dtype=np.uint8) if not torch.is_tensor(want) else want).to('cuda')
        base = PAD + self.off
        if rows is None:
            exp[base:base + want.numel()] = want.reshape(-1)
        else:
            nrows, nbytes, stride = rows
            want = want.reshape(nrows, nbytes)
            for y in range(nrows):
                exp[base + y * stride:base + y * stride + nbytes] = want[y]
        if not torch.equal(self.t, exp):
            bad = torch.nonzero(self.t != exp).reshape(-1)
            first = int(bad[0])
            raise AssertionError('%r: %d bytes differ, first at %d (output begins at %d): got %d, want %d'
                                 % (what, bad.numel(), first, base, int(self.t[first]), int(exp[first])))
        STATS['cases'] += 1

    def untouched(self):
        return bool((self.t == self.fill).all())


def scalars(ctx, vals):
    return ctx._scalars([int(v) for v in vals])


def matrix_args(ctx, M, bias):
    return scalars(ctx, [v for row in M for v in row]), (scalars(ctx, bias) if bias is not None else None)


def report(name, t0):
    torch.cuda.synchronize()
    print('%s: %d cases so far, %.2f s, largest buffer: %d bytes, %d CUs' % (name, STATS['cases'], time.time() - t0, STATS['max_bytes'], num_cu()))


# ---- ffgpu_gf256_sbox ------------------------------------------------------------------------------------------------------------
def sbox_call(ctx, rows8, b, src, out, n):
    r = (ctypes.c_uint8 * 8)(*rows8)
    return ctx._L.ffgpu_gf256_sbox(ctx._h, src.ptr if src is not None else None, r, ctypes.c_uint8(b), out.ptr if out is not None else None,
                                   n, ctx._stream())


def test_sbox(monkeypatch):
    t0 = time.time()
    OK, EINVAL, ENOTSUP = status()
    g = gc.golden_sbox()
    ctx = default_ctx(gc.AES)
    rnd = np.random.default_rng(1)
    mapA = (g['rows8'], g['b'])
    mapB = ([0x1f, 0x3e, 0x7c, 0xf8, 0xf1, 0xe3, 0xc7, 0x8e][::-1], 0x05)
    lutA, lutB = gc.sbox_lut(*mapA), gc.sbox_lut(*mapB)
    assert lutA.tolist() == g['table'] and lutB.tolist() != g['table']
    for n in (1, 15, 16, 17, 4099):
        data = rnd.integers(0, 256, n, dtype=np.uint8)
        data[:min(n, 256)] = np.arange(min(n, 256))
        for ioff, ooff in ((0, 0), (1, 0), (0, 1)):
            src = Buf(data, ioff)
            # two maps alternated on one context: the cached table follows the (rows8, b) of the call
            for (rows8, b), lut in ((mapA, lutA), (mapB, lutB), (mapA, lutA)):
                out = Out(n, ooff)
                assert sbox_call(ctx, rows8, b, src, out, n) == OK
                out.check(lut[data], ('sbox', n, ioff, ooff, b))
            assert src.untouched()
    # capped grid: thread 0 of CUs x 256 threads takes three 16-byte packs
    cap = capped_ctx(monkeypatch, gc.AES)
    gsz = 256 * num_cu()
    n = gc.capped_n('sbox', gsz) + 5
    assert gc.capped_trips('sbox', n, gsz) == 3 and gc.capped_trips('sbox', n - 16, gsz) == 2
    data = rnd.integers(0, 256, n, dtype=np.uint8)
    src, out = Buf(data), Out(n)
    assert sbox_call(cap, *mapA, src, out, n) == OK
    out.check(lutA[data], ('sbox capped', n))
    assert src.untouched()
    # statuses
    out = Out(16, fill=0x3c)
    src = Buf(np.arange(16))
    assert sbox_call(default_ctx(0x13), *mapA, src, out, 16) == ENOTSUP                     # GF(2^4): x^254 is not the inverse there
    assert sbox_call(default_ctx(2**61 - 1, False), *mapA, src, out, 16) == ENOTSUP
    assert sbox_call(default_ctx(0x1002b, True), *mapA, src, out, 16) == ENOTSUP            # four-byte GF(2^16)
    assert sbox_call(ctx, *mapA, None, out, 16) == EINVAL and sbox_call(ctx, *mapA, src, None, 16) == EINVAL
    assert sbox_call(ctx, *mapA, None, None, 0) == OK
    torch.cuda.synchronize()
    assert out.untouched() and src.untouched()
    report('sbox', t0)


# ---- ffgpu_gf256_to_bits -----------------------------------------------------------------------------------------------------------
def to_bits_call(ctx, src, add, out, n):
    p = lambda b: b.ptr if b is not None else None
    return ctx._L.ffgpu_gf256_to_bits(ctx._h, p(src), p(add), p(out), n, ctx._stream())


@pytest.mark.parametrize('modulus', gc.TO_BITS_MODULI, ids=hex)
def test_to_bits(monkeypatch, modulus):
    t0 = time.time()
    OK, EINVAL, ENOTSUP = status()
    F = gc.field(modulus)
    ctx = default_ctx(modulus)
    rnd = np.random.default_rng(modulus)
    for n in (1, 2, 3, 1025):
        data = rnd.integers(0, F.order, n, dtype=np.uint8)
        data[-1] = F.order - 1
        addv = rnd.integers(0, F.order, 8 * n, dtype=np.uint8)
        for aoff in (None, 0, 8):
            for ioff, ooff in ((0, 0), (1, 0), (0, 8)):
                src, add, out = Buf(data, ioff), (Buf(addv, aoff) if aoff is not None else None), Out(8 * n, ooff)
                assert to_bits_call(ctx, src, add, out, n) == OK
                out.check(gc.to_bits_np(data, addv if add is not None else None), ('to_bits', hex(modulus), n, aoff, ioff, ooff))
                assert src.untouched() and (add is None or add.untouched())
    cap = capped_ctx(monkeypatch, modulus)
    gsz = 256 * num_cu()
    n = gc.capped_n('to_bits', gsz) + 1
    assert gc.capped_trips('to_bits', n, gsz) == 3 and gc.capped_trips('to_bits', n - 2, gsz) == 2
    data, addv = rnd.integers(0, F.order, n, dtype=np.uint8), rnd.integers(0, F.order, 8 * n, dtype=np.uint8)
    src, add, out = Buf(data), Buf(addv), Out(8 * n)
    assert to_bits_call(cap, src, add, out, n) == OK
    out.check(gc.to_bits_np(data, addv), ('to_bits capped', n))
    assert src.untouched() and add.untouched()
    out, src = Out(64, fill=0x3c), Buf(np.arange(8) % F.order)
    assert to_bits_call(default_ctx(2**61 - 1, False), src, None, out, 8) == ENOTSUP
    assert to_bits_call(default_ctx(0x1002b), src, None, out, 8) == ENOTSUP
    assert to_bits_call(ctx, None, None, out, 8) == EINVAL and to_bits_call(ctx, src, None, None, 8) == EINVAL
    assert to_bits_call(ctx, None, None, None, 0) == OK
    torch.cuda.synchronize()
    assert out.untouched() and src.untouched()
    report('to_bits', t0)


# ---- ffgpu_gf256_bit_affine ----------------------------------------------------------------------------------------------------------
def bit_affine_call(ctx, M, bias, fb, src, out, ng):
    mm, bb = matrix_args(ctx, M, bias)
    p = lambda b: b.ptr if b is not None else None
    return ctx._L.ffgpu_gf256_bit_affine(ctx._h, mm, bb, fb, p(src), p(out), ng, ctx._stream())


def bit_affine_matrices(F, rnd):
    """name -> (matrix, general): the AES map (a 0 / 1 matrix; where the field has eight bits), a random 0 / 1 matrix, a random
    matrix over the whole field (every bit plane of the field on some diagonal), the eight single diagonals"""
    ms = {}
    if F.n == 8:
        ms['aes'] = (gc.aes_map()[0], False)
    ms['bits'] = (gc.random_matrix(F, rnd, True), False)
    G = gc.random_matrix(F, rnd, False)
    G[2][5] |= F.order >> 1
    ms['field'] = (G, F.n > 1)
    for d in range(8):
        ms['shift%d' % d] = (gc.shift_matrix(d), False)
    return ms


@pytest.mark.parametrize('modulus', gc.BIT_AFFINE_MODULI, ids=hex)
def test_bit_affine(monkeypatch, modulus):
    t0 = time.time()
    OK, EINVAL, ENOTSUP = status()
    F = gc.field(modulus)
    ctx = default_ctx(modulus)
    rnd = random.Random(modulus)
    nrnd = np.random.default_rng(modulus)
    ms = bit_affine_matrices(F, rnd)
    bias = gc.random_bias(F, rnd)
    bias[7] = F.order - 1
    for ng in (1, 2, 3, 4, 5, 1025):
        x = nrnd.integers(0, F.order, 8 * ng, dtype=np.uint8)
        x[:8] = F.order - 1
        src = Buf(x)
        for name, (M, _) in ms.items():
            for bs in (None, bias):
                for fb in (0, 1):
                    out = Out(ng if fb else 8 * ng)
                    assert bit_affine_call(ctx, M, bs, fb, src, out, ng) == OK
                    out.check(gc.bit_affine_np(F, M, bs, fb, x), ('bit_affine', hex(modulus), name, bs is not None, fb, ng))
        assert src.untouched()
        # 8-byte aligned buffers: the group path; a folded output at an odd address
        M = ms['field'][0]
        for ioff, ooff, fb in ((8, 0, 0), (8, 0, 1), (0, 8, 0), (0, 1, 1), (8, 8, 0)):
            src2, out = Buf(x, ioff), Out(ng if fb else 8 * ng, ooff)
            assert bit_affine_call(ctx, M, bias, fb, src2, out, ng) == OK
            out.check(gc.bit_affine_np(F, M, bias, fb, x), ('bit_affine', hex(modulus), 'offsets', ioff, ooff, fb, ng))
            assert src2.untouched()
    # refused: 4-byte offsets
    x = nrnd.integers(0, F.order, 64, dtype=np.uint8)
    out = Out(64, fill=0x3c)
    assert bit_affine_call(ctx, ms['bits'][0], None, 0, Buf(x, 4), out, 8) == EINVAL
    assert bit_affine_call(ctx, ms['bits'][0], None, 1, Buf(x, 4), out, 8) == EINVAL
    out4 = Out(64, off=4, fill=0x3c)
    assert bit_affine_call(ctx, ms['bits'][0], None, 0, Buf(x), out4, 8) == EINVAL
    assert bit_affine_call(ctx, ms['bits'][0], None, 0, None, out, 8) == EINVAL and bit_affine_call(ctx, ms['bits'][0], None, 0, Buf(x), None, 8) == EINVAL
    assert bit_affine_call(ctx, ms['bits'][0], None, 0, None, None, 0) == OK
    torch.cuda.synchronize()
    assert out.untouched() and out4.untouched()
    # capped grid, one case per (FOLD, GENERAL) instantiation: three trips of the two-packs-per-lane loop
    cap = capped_ctx(monkeypatch, modulus)
    gsz = 256 * num_cu()
    ng = gc.capped_n('bit_affine', gsz) + 1
    assert gc.capped_trips('bit_affine', ng, gsz) == 3 and gc.capped_trips('bit_affine', ng - 4, gsz) == 2
    x = nrnd.integers(0, F.order, 8 * ng, dtype=np.uint8)
    src = Buf(x)
    for name in ('bits', 'field'):
        M, general = ms[name]
        for fb in (0, 1):
            out = Out(ng if fb else 8 * ng)
            assert bit_affine_call(cap, M, bias, fb, src, out, ng) == OK
            out.check(gc.bit_affine_np(F, M, bias, fb, x), ('bit_affine capped', hex(modulus), name, fb, ng))
    assert src.untouched()
    report('bit_affine ' + hex(modulus), t0)


def test_bit_affine_refused_fields():
    OK, EINVAL, ENOTSUP = status()
    out, src = Out(64, fill=0x3c), Buf(np.arange(64) % 2)
    for ctx in (default_ctx(2**61 - 1, False), default_ctx(0x1002b)):
        assert bit_affine_call(ctx, gc.identity(), None, 0, src, out, 8) == ENOTSUP
    torch.cuda.synchronize()
    assert out.untouched() and src.untouched()


# ---- ffgpu_gf256_mask_open -----------------------------------------------------------------------------------------------------------
def mask_open_call(ctx, rows, coef, rbits, mu, out, n, nrows=None, np_=None):
    """rows / rbits: Bufs (or None for a null pointer)"""
    nrows = len(rows) if nrows is None else nrows
    np_ = len(rbits) if np_ is None else np_
    pr = (ctypes.c_void_p * max(1, len(rows)))(*[(b.ptr if b is not None else None) for b in rows])
    pb = (ctypes.c_void_p * max(1, len(rbits)))(*[(b.ptr if b is not None else None) for b in rbits])
    return ctx._L.ffgpu_gf256_mask_open(ctx._h, pr, scalars(ctx, coef) if coef else None, nrows, pb, scalars(ctx, mu) if mu else None, np_,
                                        out.ptr if out is not None else None, n, ctx._stream())


def mask_open_data(F, nrows, np_, n, seed):
    rnd = np.random.default_rng(seed)
    rows = [rnd.integers(0, 256, n, dtype=np.uint8) for _ in range(nrows)]
    rbits = [rnd.integers(0, 256, 8 * n, dtype=np.uint8) for _ in range(np_)]        # any bytes: the sum is linear in them
    coef = [int(v) for v in rnd.integers(1, 256, nrows)]
    if nrows > 1:
        coef[nrows // 2] = 0                                                          # one zero coefficient
    mu = [int(v) for v in rnd.integers(1, 256, np_)]
    return rows, coef, rbits, mu


def test_mask_open(monkeypatch):
    t0 = time.time()
    OK, EINVAL, ENOTSUP = status()
    ctx = default_ctx(gc.AES)
    for nrows, np_ in ((1, 0), (0, 1), (8, 2), (9, 3), (32, 8)):
        for n in (1, 2, 3, 1025):
            rows, coef, rbits, mu = mask_open_data(F8, nrows, np_, n, 1000 * nrows + 10 * np_ + n)
            want = gc.mask_open_np(F8, rows, coef, rbits, mu, n)
            brows, bbits, out = [Buf(r) for r in rows], [Buf(r) for r in rbits], Out(n)
            assert mask_open_call(ctx, brows, coef, bbits, mu, out, n) == OK
            out.check(want, ('mask_open', nrows, np_, n))
            assert all(b.untouched() for b in brows + bbits)
    # each spoiler of the vector path on its own: the output odd, one row odd, one bit row only 8-byte aligned
    for n in (3, 1025):
        rows, coef, rbits, mu = mask_open_data(F8, 9, 3, n, 77 + n)
        want = gc.mask_open_np(F8, rows, coef, rbits, mu, n)
        for spoiler in ('out', 'row', 'bits'):
            brows = [Buf(r, 1 if (spoiler == 'row' and i == 4) else 0) for i, r in enumerate(rows)]
            bbits = [Buf(r, 8 if (spoiler == 'bits' and i == 2) else 0) for i, r in enumerate(rbits)]
            out = Out(n, 1 if spoiler == 'out' else 0)
            assert mask_open_call(ctx, brows, coef, bbits, mu, out, n) == OK
            out.check(want, ('mask_open', spoiler, n))
            assert all(b.untouched() for b in brows + bbits)
    # capped grid with (9, 3): the second pass of the eight-row loop and a party loaded inside the loop, three trips
    cap = capped_ctx(monkeypatch, gc.AES)
    gsz = 256 * num_cu()
    n = gc.capped_n('mask_open', gsz) + 1
    assert gc.capped_trips('mask_open', n, gsz) == 3 and gc.capped_trips('mask_open', n - 4, gsz) == 2
    rows, coef, rbits, mu = mask_open_data(F8, 9, 3, n, 5)
    brows, bbits, out = [Buf(r) for r in rows], [Buf(r) for r in rbits], Out(n)
    assert mask_open_call(cap, brows, coef, bbits, mu, out, n) == OK
    out.check(gc.mask_open_np(F8, rows, coef, rbits, mu, n), ('mask_open capped', n))
    assert all(b.untouched() for b in brows + bbits)
    # two fields alternated on one thread: the launcher's table of 2^b follows the field of the call
    n = 1025
    rows, coef, rbits, mu = mask_open_data(F8, 3, 2, n, 9)
    brows, bbits = [Buf(r) for r in rows], [Buf(r) for r in rbits]
    for modulus in (gc.AES, 0x11d, gc.AES, 0x11d):
        F, out = gc.field(modulus), Out(n)
        assert mask_open_call(default_ctx(modulus), brows, coef, bbits, mu, out, n) == OK
        out.check(gc.mask_open_np(F, rows, coef, rbits, mu, n), ('mask_open', hex(modulus)))
    assert gc.mask_open_np(F8, rows, coef, rbits, mu, n).tolist() != gc.mask_open_np(gc.field(0x11d), rows, coef, rbits, mu, n).tolist()
    # statuses
    out = Out(8, fill=0x3c)
    row, bits = Buf(np.arange(8)), Buf(np.arange(64))
    one = [1] * 40
    assert mask_open_call(ctx, [row] * 33, one[:33], [bits], [1], out, 8) == ENOTSUP
    assert mask_open_call(ctx, [row], [1], [bits] * 9, one[:9], out, 8) == ENOTSUP
    assert mask_open_call(ctx, [], [], [], [], out, 8) == EINVAL
    assert mask_open_call(ctx, [row], [1], [bits], [1], out, 8, nrows=-1) == EINVAL
    assert mask_open_call(ctx, [row, None, row], [1, 1, 1], [bits], [1], out, 8) == EINVAL
    assert mask_open_call(ctx, [row], [1], [None], [1], out, 8) == EINVAL
    assert mask_open_call(ctx, [row], [1], [bits], [1], None, 8) == EINVAL
    for other in (default_ctx(2**61 - 1, False), default_ctx(0x1002b)):
        assert mask_open_call(other, [row], [1], [bits], [1], out, 8) == ENOTSUP
    assert mask_open_call(ctx, [None], [1], [None], [1], None, 0) == OK
    torch.cuda.synchronize()
    assert out.untouched() and row.untouched() and bits.untouched()
    report('mask_open', t0)


# ---- ffgpu_gf256_bits_affine_fold ------------------------------------------------------------------------------------------------------
def fold_call(ctx, M, bias, c, rbits, ybr, out, ybo, n, nbatch):
    mm, bb = matrix_args(ctx, M, bias)
    p = lambda b: b.ptr if b is not None else None
    return ctx._L.ffgpu_gf256_bits_affine_fold(ctx._h, mm, bb, p(c), p(rbits), ybr, p(out), ybo, n, nbatch, ctx._stream())


def fold_strides(n):
    """name -> (rbits stride, out stride); vector path: 16 | rbits stride and 2 | out stride"""
    r16 = (8 * n + 15) // 16 * 16 + 16
    r8 = 8 * n + 8 if (8 * n + 8) % 16 else 8 * n + 16                     # a multiple of 8 that is none of 16: the byte path
    even = n + n % 2 + 2
    odd = n + 1 if (n + 1) % 2 else n + 2
    return {'vector': (r16, even), 'rbits stride': (r8, even), 'out stride': (r16, odd)}


def fold_case(ctx, F, M, bias, n, nbatch, ybr, ybo, seed, what):
    rnd = np.random.default_rng(seed)
    c = rnd.integers(0, 256, n, dtype=np.uint8)
    span = (nbatch - 1) * ybr + 8 * n
    rb = np.full(span, 0x77, dtype=np.uint8)
    want = []
    for y in range(nbatch):
        row = rnd.integers(0, 256, 8 * n, dtype=np.uint8)                  # any bytes
        rb[y * ybr:y * ybr + 8 * n] = row
        want.append(gc.bits_affine_fold_np(F, M, bias, c, row))
    bc, brb, out = Buf(c), Buf(rb), Out((nbatch - 1) * ybo + n)
    OK = status()[0]
    assert fold_call(ctx, M, bias, bc, brb, ybr, out, ybo, n, nbatch) == OK
    out.check(np.stack(want), what, rows=(nbatch, n, ybo))
    assert bc.untouched() and brb.untouched()


def test_bits_affine_fold(monkeypatch):
    t0 = time.time()
    OK, EINVAL, ENOTSUP = status()
    ctx = default_ctx(gc.AES)
    A, B = gc.aes_map()
    G, GB = gc.general_map(F8)
    seed = 0
    for n in (1, 2, 3, 1025):
        for nbatch in (1, 3, 7):
            strides = dict(fold_strides(n))
            if nbatch == 1:
                strides['zero'] = (0, 0)
            for sname, (ybr, ybo) in strides.items():
                for M, bias in ((A, None), (A, B), (G, None), (G, GB)):
                    seed += 1
                    fold_case(ctx, F8, M, bias, n, nbatch, ybr, ybo, seed, ('fold', n, nbatch, sname, M is G, bias is not None))
    cap = capped_ctx(monkeypatch, gc.AES)
    gsz = 256 * num_cu()
    n = gc.capped_n('bits_affine_fold', gsz) + 1
    assert gc.capped_trips('bits_affine_fold', n, gsz) == 3 and gc.capped_trips('bits_affine_fold', n - 4, gsz) == 2
    ybr, ybo = fold_strides(n)['vector']
    fold_case(cap, F8, G, GB, n, 3, ybr, ybo, 99, ('fold capped', n))
    # refused
    n = 8
    c, rb, out = Buf(np.arange(n)), Buf(np.arange(3 * 80) % 256), Out(3 * 16, fill=0x3c)
    for args in ((80, 16, n, 0), (80, 16, n, 65536), (80, 16, n, -1), (8 * n - 1, 16, n, 3), (80, n - 1, n, 3)):
        assert fold_call(ctx, A, B, c, rb, args[0], out, args[1], args[2], args[3]) == EINVAL, args
    assert fold_call(ctx, A, B, None, rb, 80, out, 16, n, 3) == EINVAL and fold_call(ctx, A, B, c, None, 80, out, 16, n, 3) == EINVAL
    assert fold_call(ctx, A, B, c, rb, 80, None, 16, n, 3) == EINVAL
    for other in (default_ctx(2**61 - 1, False), default_ctx(0x1002b)):
        assert fold_call(other, A, B, c, rb, 80, out, 16, n, 3) == ENOTSUP
    assert fold_call(ctx, A, B, None, None, 0, None, 0, 0, 1) == OK
    torch.cuda.synchronize()
    assert out.untouched() and c.untouched() and rb.untouched()
    report('bits_affine_fold', t0)


# ---- ffgpu_gf256_sbox_layer ------------------------------------------------------------------------------------------------------------
_layer_tabs = {}


def layer_maps():
    """(a) AES, (b) the identity with no bias, (c) a general matrix with a bias -> (LayerTables, its device copy)"""
    if not _layer_tabs:
        A, B = gc.aes_map()
        G, GB = gc.general_map(F8)
        for name, (M, bias) in (('a', (A, B)), ('b', (gc.identity(), None)), ('c', (G, GB))):
            tabs = gc.LayerTables(F8, M, bias)
            _layer_tabs[name] = (tabs, tabs.on(torch, 'cuda'))
    return _layer_tabs


def lagrange(points):
    return po.recombination_vector(F8, list(points), 0)


def layer_call(ctx, tabs, m, t, X, xs, R, rs, out, os_, n, rounds=20, nonce=0, key=KEY, state=None, lam=None, mu=None):
    mm, bb = matrix_args(ctx, tabs.M, tabs.bias)
    lam = lagrange(range(1, 2 * t + 2)) if lam is None else lam
    mu = lagrange(range(1, t + 2)) if mu is None else mu
    ptr = lambda v: (v if isinstance(v, int) else (v.data_ptr() if torch.is_tensor(v) else v.ptr)) if v is not None else None
    return ctx._L.ffgpu_gf256_sbox_layer(ctx._h, mm, bb, scalars(ctx, lam), scalars(ctx, mu), t, m, ptr(X), xs, ptr(R), rs, ptr(out), os_, n,
                                         key, nonce, rounds, state, 0, ctx._stream())


def layer_case(ctx, name, m, t, n, rounds, seed, any_bytes, pad_rows, what):
    """one accepted launch: every party's row byte for byte, guards around the rows and in their padding and behind a ragged
    end, the inputs unchanged; with real bits the rows open to the map of x^254 from the first and the last t+1 parties"""
    tabs, dev = layer_maps()[name]
    n4 = (n + 3) // 4 * 4
    xs, rs, os_ = (n4 + 8, (8 * n + 15) // 16 * 16 + 32, n4 + 12) if pad_rows else (n4, (8 * n + 15) // 16 * 16, n4)
    x, r, X, R, _, _ = gc.layer_inputs_torch(torch, tabs, dev, n, m, t, seed, 'cuda', xs=xs, rs=rs, any_bytes=any_bytes)
    assert X.data_ptr() % 16 == 0 and R.data_ptr() % 16 == 0
    Xb, Rb = X.clone(), R.clone()
    want = gc.layer_expected_torch(torch, dev, x, r, R, n)
    out = Out((m - 1) * os_ + n)
    STATS['max_bytes'] = max(STATS['max_bytes'], R.numel())
    assert layer_call(ctx, tabs, m, t, X, xs, R, rs, out, os_, n, rounds=rounds, nonce=seed) == status()[0], what
    out.check(want, what, rows=(m, n, os_))
    assert torch.equal(X, Xb) and torch.equal(R, Rb), ('an input was written', what)
    if not any_bytes:
        g = gc.golden_sbox()
        if name == 'a':
            table = torch.tensor(g['table'], dtype=torch.uint8, device='cuda')
        else:
            table = dev['S'][torch.tensor(g['pow254'], dtype=torch.int64, device='cuda')]       # the map on the bits of x^254
            if name == 'b':
                assert table.tolist() == g['pow254']
        base = PAD
        got = [out.t[base + j * os_:base + j * os_ + n] for j in range(m)]
        for pts in (tuple(range(1, t + 2)), tuple(range(m - t, m + 1))):
            opened = gc.opened_torch(torch, tabs, dev, [got[p - 1] for p in pts], pts)
            assert torch.equal(opened, table[x.to(torch.int64)]), ('opening', what, pts)
    return x


@pytest.mark.parametrize('m,t', gc.MT, ids=lambda v: str(v))
def test_sbox_layer(m, t):
    """all nine (m, t) at every small size, on padded rows; the maps A, C, A (and B) on one context: the cached device tables
    follow the matrix and bias of the call; 20 and 12 rounds, 8 once"""
    t0 = time.time()
    ctx = default_ctx(gc.AES)
    seed = 1000 * m + 100 * t
    for n in (1, 3, 4, 6, 1021, 4099):
        for k, (name, rounds, any_bytes) in enumerate((('a', 20, False), ('c', 12, True), ('a', 12, True), ('b', 20, False), ('c', 20, False))):
            seed += 1
            x = layer_case(ctx, name, m, t, n, rounds, seed, any_bytes, True, ('layer', m, t, n, name, rounds, any_bytes))
            if n >= 256:
                assert sorted(set(x.tolist())) == list(range(256))
    layer_case(ctx, 'a', m, t, 1021, 8, seed + 1, False, False, ('layer', m, t, 1021, 'a', 8))
    report('sbox_layer (%d, %d)' % (m, t), t0)


@pytest.mark.parametrize('m,t', [(3, 1), (4, 1), (5, 1), (7, 1), (5, 2), (7, 3)], ids=lambda v: str(v))
def test_sbox_layer_step_boundary(m, t):
    """n = 12 gsz: three steps per thread, the largest size with a fresh stream per step; n = 12 gsz + 7: four steps and a ragged
    end, the smallest size at which the t = 1 kernels continue their keystream (ChaCha20 interleaved; with 12 rounds the
    block-at-a-time stream)"""
    t0 = time.time()
    ctx = default_ctx(gc.AES)
    gsz = gc.layer_gsz(num_cu(), m, t)
    n3, n4 = 12 * gsz, 12 * gsz + 7
    assert gc.trips(n3 // 4, gsz) == 3 and gc.trips(n4 // 4, gsz) == 4 and n4 % 4 == 3
    layer_case(ctx, 'a', m, t, n3, 20, 31 * m + t, False, False, ('layer three steps', m, t, n3))
    layer_case(ctx, 'c', m, t, n4, 20, 37 * m + t, True, False, ('layer four steps', m, t, n4))
    layer_case(ctx, 'a', m, t, n4, 12, 41 * m + t, False, False, ('layer four steps, 12 rounds', m, t, n4))
    report('sbox_layer steps (%d, %d): n = %d' % (m, t, n4), t0)


def test_sbox_layer_device_state_and_refusals():
    """the device-resident nonce advances by exactly 1 per accepted launch and by 0 per refused one; the status table; a refused
    call writes nothing; protocols.sbox_layer_all still opens to the table where the fused kernel refuses the rows"""
    t0 = time.time()
    OK, EINVAL, ENOTSUP = status()
    from mpyc_amd import engine, finfields, gfpx, protocols
    ctx = default_ctx(gc.AES)
    tabs, dev = layer_maps()['a']
    m, t, n = 3, 1, 1021
    xs, rs, os_ = 1024, 8192, 1024
    x, r, X, R, _, _ = gc.layer_inputs_torch(torch, tabs, dev, n, m, t, 5, 'cuda', xs=xs, rs=rs, any_bytes=False)
    want = gc.layer_expected_torch(torch, dev, x, r, R, n)
    st = ctx.rng_state()
    torch.cuda.synchronize()
    n0 = st.nonce()
    for k in (1, 2, 3):
        out = Out((m - 1) * os_ + n)
        assert layer_call(ctx, tabs, m, t, X, xs, R, rs, out, os_, n, key=None, state=st.ptr) == OK
        out.check(want, ('layer, device state', k), rows=(m, n, os_))
        assert st.nonce() == n0 + k
    out = Out(m * os_, fill=0x3c)
    call = lambda **kw: layer_call(ctx, tabs, kw.pop('m', m), kw.pop('t', t), kw.pop('X', X), kw.pop('xs', xs), kw.pop('R', R),
                                   kw.pop('rs', rs), kw.pop('out', out), kw.pop('os_', os_), kw.pop('n', n), **kw)
    one = [1] * 9
    refused = [
        (dict(t=0, m=3, lam=one[:1], mu=one[:1]), EINVAL), (dict(t=2, m=4, lam=one[:5], mu=one[:3]), EINVAL),
        (dict(t=4, m=9, lam=one[:9], mu=one[:5]), ENOTSUP), (dict(t=1, m=8), ENOTSUP),
        (dict(xs=n - 1), EINVAL), (dict(rs=8 * n - 1), EINVAL), (dict(os_=n - 1), EINVAL),
        (dict(X=None), EINVAL), (dict(R=None), EINVAL), (dict(out=None), EINVAL),
        # rows off their 4- / 16-byte grid
        (dict(X=X.data_ptr() + 1), ENOTSUP), (dict(X=X.data_ptr() + 2), ENOTSUP), (dict(xs=xs + 2), ENOTSUP), (dict(os_=os_ + 1), ENOTSUP),
        (dict(out=out.ptr + 2), ENOTSUP), (dict(R=R.data_ptr() + 8), ENOTSUP), (dict(R=R.data_ptr() + 4), ENOTSUP), (dict(rs=rs + 8), ENOTSUP),
    ]
    for kw, code in refused:
        for state in (None, st.ptr):
            assert call(key=KEY if state is None else None, state=state, **dict(kw)) == code, (kw, state is not None)
    assert call(key=None, state=st.ptr, nonce=2**32) == EINVAL
    ok64 = Out((m - 1) * os_ + n)
    assert call(key=KEY, nonce=2**32, out=ok64) == OK                         # a host nonce has 64 bits
    ok64.check(want, 'layer, 64-bit host nonce', rows=(m, n, os_))
    out2 = Out(m * os_, fill=0x3c)
    for other in (default_ctx(2**61 - 1, False), default_ctx(0x1002b), default_ctx(0x13)):
        assert layer_call(other, tabs, m, t, X, xs, R, rs, out2, os_, n, lam=one[:3], mu=one[:2]) == ENOTSUP
    assert layer_call(ctx, tabs, m, t, None, 0, None, 0, None, 0, 0) == OK
    torch.cuda.synchronize()
    assert st.nonce() == n0 + 3, 'a refused launch advanced the device nonce'
    assert out.untouched() and out2.untouched(), 'a refused call wrote to its output'
    # where the fused kernel refuses the rows, the composition of the per-step kernels serves them
    F = finfields.GF(gfpx.GFpX(2)(gc.AES))
    A, B = gc.aes_map()
    g = gc.golden_sbox()
    table = torch.tensor(g['table'], dtype=torch.uint8, device='cuda')
    n = 1021
    x, r, X, R, _, _ = gc.layer_inputs_torch(torch, tabs, dev, n, m, t, 6, 'cuda', xs=n + 1, rs=8 * n + 8, any_bytes=False)
    assert layer_call(ctx, tabs, m, t, X, n + 1, R, 8 * n + 8, out2, os_, n) == ENOTSUP
    res = protocols.sbox_layer_all(ctx, F, engine.DevMatrix(ctx, X, m, n, n + 1), engine.DevMatrix(ctx, R, m, 8 * n, 8 * n + 8), t, A, B)
    rows = [res.row(j).t for j in range(m)]
    assert torch.equal(gc.opened_torch(torch, tabs, dev, rows[:2], (1, 2)), table[x.to(torch.int64)])
    assert torch.equal(gc.opened_torch(torch, tabs, dev, rows[1:], (2, 3)), table[x.to(torch.int64)])
    assert torch.equal(torch.stack(rows), gc.layer_expected_torch(torch, dev, x, r, R, n))
    assert out2.untouched()
    report('sbox_layer statuses', t0)
