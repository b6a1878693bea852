"""Stacks of matrices through the stack kernels (k_matmul_stack_packed / _tiled, ffgpu_matmul_stack): every field policy,
shapes on both sides of the packed / tiled line, batches around every P boundary, every operand form of `@`, the
accumulator bound, bytes identical to ffgpu_matmul and to the per-matrix loop, one launch, no expanded copy of a
shared operand, 10^5 small and 64 medium matrices, the C ABI.  Every element is compared, nothing is sampled.
Expected values never come from the code under test: prime fields take np.matmul on dtype=object arrays of Python
ints, then % p (what the reference computes, finfields.py:1126-1135); GF(2^n) takes oracle.pyoracle.matmul per matrix."""
import random
import time

import numpy as np
import pytest

from oracle import pyoracle as po
from test_gpu_convolve import P61, P128, binary_moduli, prime_moduli

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

BLOCK, LDS_BUDGET, KC_WANT = 256, 16384, 8          # mpyc_amd/csrc/matmul_stack_geom.hpp
SHAPES = [(1, 1, 1), (2, 3, 4), (4, 4, 4), (8, 8, 8), (16, 16, 16), (17, 5, 16), (33, 70, 31), (64, 16, 32)]


def slot_bytes(modulus, binary):
    """LDS bytes of one staged element: the policy's word, or 4 bytes per 28-bit digit for the 2^k - c primes above 64
    bits (PM96: 4 digits, PM128: 5, PM192: 7)"""
    if binary:
        d = modulus.bit_length() - 1
        return 1 if d <= 8 else 4 if d <= 32 else 8 if d <= 64 else 16
    bits = modulus.bit_length()
    if bits <= 32:
        return 4
    if bits <= 64:
        return 8
    if modulus in (2**80 - 65, 2**96 - 17):
        return 16
    if modulus in (2**127 - 1, P128):
        return 20
    if modulus == 2**136 - 113:
        return 28
    return 16 if bits <= 128 else 24                  # MONT128, MONT192


def plan_p(M, K, N, slot):
    """matrices per workgroup of the packed shape (stack_plan, written out again here); None: the tiled shape"""
    if M * N > BLOCK:
        return None
    P = BLOCK // (M * N)
    while True:
        kc = min(K, LDS_BUDGET // (P * (M + N) * slot))
        if kc >= min(K, KC_WANT) or P == 1:
            return P
        P = (P + 1) // 2


def batches_of(P):
    b = [1, 2, 3]
    if P is not None:
        b += [x for x in (P - 1, P, P + 1, 2 * P + 1) if x >= 1]
    return sorted(set(b))


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    from mpyc_amd import finfields, gfpx
    return finfields, gfpx


def gf(api, modulus, binary=False):
    finfields, gfpx = api
    return finfields.GF(gfpx.BinaryPolynomial(modulus)) if binary else finfields.GF(modulus)


def order_of(modulus, binary):
    return 1 << (modulus.bit_length() - 1) if binary else modulus


def draw(rng, order, *shape):
    n = int(np.prod(shape))
    vals = [rng.randrange(order) for _ in range(n)]
    for i, e in enumerate((order - 1, 0, 1)):          # edge values where there is room
        if 2 * i + 1 < n:
            vals[rng.randrange(n)] = e
    return np.array(vals, dtype=object).reshape(shape)


def expect(modulus, binary, a, b):
    """NumPy's matmul on the Python ints, then % p; GF(2^n): the oracle's product per matrix of the broadcast stack"""
    if not binary:
        return np.matmul(a, b) % modulus
    F = po.Field(modulus, True)
    a2 = a.reshape(1, -1) if a.ndim == 1 else a
    b2 = b.reshape(-1, 1) if b.ndim == 1 else b
    batch = np.broadcast_shapes(a2.shape[:-2], b2.shape[:-2])
    mshape = (a2.shape[-2], b2.shape[-1])
    ab = np.broadcast_to(a2, batch + a2.shape[-2:]).reshape((-1,) + a2.shape[-2:])
    bb = np.broadcast_to(b2, batch + b2.shape[-2:]).reshape((-1,) + b2.shape[-2:])
    out = np.empty((len(ab),) + mshape, dtype=object)
    for i, (x, y) in enumerate(zip(ab, bb)):
        if x.size and y.size:
            out[i] = np.array(po.matmul(F, x.tolist(), y.tolist()), dtype=object).reshape(mshape)
        else:
            out[i] = 0
    out = out.reshape(batch + mshape)
    if a.ndim == 1:
        out = out.reshape(out.shape[:-2] + out.shape[-1:])
    elif b.ndim == 1:
        out = out.reshape(out.shape[:-1])
    return out


def ints(x):
    return np.array([int(v) for v in np.asarray(x.value).reshape(-1)], dtype=object).reshape(x.shape)


def same(got, want, tag):
    assert tuple(got.shape) == tuple(want.shape), (tag, got.shape, want.shape)
    g = ints(got)
    assert (g == want).all(), (tag, np.argwhere(g != want)[:4].tolist())


def raw(dev):
    return dev.to_numpy().tobytes()


ALL = [(p, False) for p in prime_moduli()] + [(m, True) for m in binary_moduli()]


@pytest.mark.parametrize('modulus,binary', ALL, ids=[hex(m) for m, _ in ALL])
def test_every_policy_shapes_and_batches(api, modulus, binary):
    """stack @ stack for every shape and every batch around P; each matrix's BYTES are ffgpu_matmul's on that matrix; one
    batch per shape also byte for byte against the per-matrix loop"""
    from mpyc_amd import finfields
    F = gf(api, modulus, binary)
    order = order_of(modulus, binary)
    rng = random.Random(modulus & 0xffff)
    for M, K, N in SHAPES:
        P = plan_p(M, K, N, slot_bytes(modulus, binary))
        assert (P is None) == (M * N > BLOCK)
        bs = batches_of(P)
        a, b = draw(rng, order, bs[-1], M, K), draw(rng, order, bs[-1], K, N)
        want = expect(modulus, binary, a, b)
        fa, fb = F.array(a), F.array(b)
        ctx = fa.ctx
        for nb in bs:
            tag = (hex(modulus), M, K, N, nb)
            xa, xb = fa[:nb], fb[:nb]
            got = xa @ xb
            same(got, want[:nb], tag)
            if nb <= 3 or nb == bs[-1]:                  # batch == 1 and each matrix of a stack: ffgpu_matmul's bytes;
                gb = raw(got._dev)                       # of the largest batch the first and the last matrix (a later workgroup)
                sz = M * N * ctx.elem_bytes
                for i in (range(nb) if nb <= 3 else (0, nb - 1)):
                    one = ctx.matmul(xa[i]._dev, xb[i]._dev, M, K, N)
                    assert gb[i * sz:(i + 1) * sz] == raw(one), tag + (i,)
        nb = bs[-1] if P is None else min(P + 1, bs[-1])
        loop = finfields._matmul_per_matrix(F.array, fa[:nb], fb[:nb], (nb,))
        assert raw((fa[:nb] @ fb[:nb])._dev) == raw(loop._dev), (hex(modulus), M, K, N, 'per-matrix loop')


@pytest.mark.parametrize('modulus,binary', ALL, ids=[hex(m) for m, _ in ALL])
def test_operand_forms(api, modulus, binary):
    """matrix @ stack, stack @ matrix, partial broadcasts, 1-D on either side, transposed views, an empty batch, K == 0"""
    F = gf(api, modulus, binary)
    order = order_of(modulus, binary)
    rng = random.Random(77 + (modulus & 0xfff))
    for M, K, N in [(2, 3, 4), (4, 4, 4), (17, 5, 16)]:
        forms = [((M, K), (5, K, N)), ((5, M, K), (K, N)), ((5, M, K), (1, K, N)), ((1, M, K), (5, K, N)),
                 ((3, 1, M, K), (1, 2, K, N)), ((2, M, K), (3, 2, K, N)), ((K,), (5, K, N)), ((5, M, K), (K,)),
                 ((1, 1, M, K), (1, K, N))]
        for sa, sb in forms:
            a, b = draw(rng, order, *sa), draw(rng, order, *sb)
            want = expect(modulus, binary, a, b)
            fa, fb = F.array(a), F.array(b)
            same(fa @ fb, want, (hex(modulus), sa, sb))
            same(np.matmul(fa, fb), want, (hex(modulus), sa, sb, 'np.matmul'))
        a, b = draw(rng, order, 5, K, M), draw(rng, order, 5, N, K)          # transposed views of the last two axes
        got = F.array(a).transpose(0, 2, 1) @ F.array(b).transpose(0, 2, 1)
        same(got, expect(modulus, binary, a.transpose(0, 2, 1), b.transpose(0, 2, 1)), (hex(modulus), M, K, N, 'T'))
        e = F.array(np.zeros((0, M, K), dtype=object)) @ F.array(draw(rng, order, K, N))
        assert e.shape == (0, M, N)
        e = F.array(np.zeros((0, M, K), dtype=object)) @ F.array(np.zeros((0, K, N), dtype=object))
        assert e.shape == (0, M, N)
        z = F.array(np.zeros((5, M, 0), dtype=object)) @ F.array(np.zeros((5, 0, N), dtype=object))      # K == 0
        assert z.shape == (5, M, N) and not ints(z).any()
        z = F.array(np.zeros((M, 0), dtype=object)) @ F.array(np.zeros((5, 0, N), dtype=object))
        assert z.shape == (5, M, N) and not ints(z).any()
        with pytest.raises(ValueError):
            F.array(draw(rng, order, 5, M, K)) @ F.array(draw(rng, order, 5, K + 1, N))
        with pytest.raises(ValueError):
            F.array(draw(rng, order, 5, M, K)) @ F.array(draw(rng, order, 4, K, N))


@pytest.mark.parametrize('modulus', prime_moduli(), ids=hex)
def test_accumulator_bound(api, modulus):
    """all entries p - 1, K = 3 x the flush bound + 1 for both accumulator kinds (192 terms for F::acc, 32 for the digit
    columns): every output is K mod p.  Both shapes: 2x2 and 4x4 outputs (packed, K in chunks), 17x16 (tiled)."""
    F = gf(api, modulus)
    for K in (3 * 192 + 1, 3 * 32 + 1):
        for M, N, nb in [(2, 2, 70), (4, 4, 5), (17, 16, 3)]:
            a = F.array(np.full((nb, M, K), modulus - 1, dtype=object))
            b = F.array(np.full((nb, K, N), modulus - 1, dtype=object))
            got = ints(a @ b)
            assert got.shape == (nb, M, N) and (got == K % modulus).all(), (hex(modulus), K, M, N)
            got = ints(a[0] @ b)                                      # the shared operand, staged once
            assert (got == K % modulus).all(), (hex(modulus), K, M, N, 'shared')


def test_one_launch_stack_times_stack(api):
    """4096 x (4x4 @ 4x4) over 2^61 - 1 is ONE compute call of the library (4096 through the per-matrix loop)"""
    F = gf(api, P61)
    rng = random.Random(11)
    a, b = draw(rng, P61, 4096, 4, 4), draw(rng, P61, 4096, 4, 4)
    fa, fb = F.array(a), F.array(b)
    ctx = fa.ctx
    torch.cuda.synchronize()
    ctx.set_timing(True, accumulate=True)
    try:
        ctx.busy_ms()
        got = fa @ fb
        ms, calls = ctx.busy_ms()
    finally:
        ctx.set_timing(False)
    print(f'4096 x (4x4 @ 4x4) over 2^61 - 1: {calls} call(s), {ms * 1e3:.1f} us on the device')
    assert calls == 1
    same(got, expect(P61, False, a, b), 'one launch')


def test_one_launch_matrix_times_stack_without_a_copy(api):
    """matrix @ stack: one call, and no expanded copy of the shared matrix -- the call may allocate the output plus
    SLACK = 64 KiB (torch rounds an allocation up to 512 bytes and may split a cached block of up to 2 MiB only when the
    remainder is at least 1 MiB, so the constant covers rounding, not a second operand: the expanded copy of the 32 x 32
    matrix would be as large as the stack, 8 MiB)."""
    SLACK = 64 << 10
    F = gf(api, P61)
    rng = random.Random(12)
    nb, M = 1024, 32
    a, b = draw(rng, P61, M, M), draw(rng, P61, nb, M, M)
    fa, fb = F.array(a), F.array(b)
    ctx = fa.ctx
    eb = ctx.elem_bytes
    warm = fa @ fb                                       # the same sizes once before: the allocator's state is settled
    del warm
    torch.cuda.synchronize()
    ctx.set_timing(True, accumulate=True)
    try:
        ctx.busy_ms()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        got = fa @ fb
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - before
        ms, calls = ctx.busy_ms()
    finally:
        ctx.set_timing(False)
    out_bytes = nb * M * M * eb
    print(f'matrix @ stack, 1024 x (32x32 @ 32x32): {calls} call(s), extra memory {extra} bytes (output {out_bytes})')
    assert calls == 1
    assert extra <= out_bytes + SLACK, (extra, out_bytes)
    same(got, expect(P61, False, a, b), 'matrix @ stack')
    # and with a 4x4 matrix (packed shape: the shared operand is staged once per workgroup)
    a4, b4 = draw(rng, P61, 4, 4), draw(rng, P61, 4096, 4, 4)
    f4, g4 = F.array(a4), F.array(b4)
    ctx.set_timing(True, accumulate=True)
    try:
        ctx.busy_ms()
        got = f4 @ g4
        ms, calls = ctx.busy_ms()
    finally:
        ctx.set_timing(False)
    assert calls == 1
    same(got, expect(P61, False, a4, b4), 'matrix @ stack 4x4')


@pytest.mark.timeout(300)
@pytest.mark.parametrize('modulus', [P61, P128], ids=hex)
def test_hundred_thousand_small_matrices(api, modulus):
    """10^5 x (4x4 @ 4x4), every output checked"""
    F = gf(api, modulus)
    rs = np.random.default_rng(20261017)
    nb = 10**5
    words = (modulus.bit_length() + 62) // 63

    def big(*shape):
        v = np.zeros(shape, dtype=object)
        for _ in range(words):
            v = v * 2**63 + rs.integers(0, 2**63, shape, dtype=np.uint64).astype(object)
        return v % modulus
    a, b = big(nb, 4, 4), big(nb, 4, 4)
    a[0], b[-1] = modulus - 1, modulus - 1
    fa, fb = F.array(a), F.array(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = fa @ fb
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    want = np.matmul(a, b) % modulus
    print(f'10^5 x (4x4 @ 4x4) over {hex(modulus)}: {(t1 - t0) * 1e3:.2f} ms (host clock), expectation {time.perf_counter() - t1:.2f} s')
    same(got, want, hex(modulus))


@pytest.mark.timeout(300)
def test_sixty_four_medium_matrices(api):
    """64 x (96x80 @ 80x72) over 2^61 - 1 (tiled shape, ragged tiles), every output checked"""
    F = gf(api, P61)
    rs = np.random.default_rng(64)
    a = rs.integers(0, P61, (64, 96, 80), dtype=np.uint64).astype(object)
    b = rs.integers(0, P61, (64, 80, 72), dtype=np.uint64).astype(object)
    a[3, 5], b[7, :, 9] = P61 - 1, P61 - 1
    got = F.array(a) @ F.array(b)
    same(got, np.matmul(a, b) % P61, '64 x 96x80x72')


def test_c_abi(api):
    """ffgpu_matmul_stack directly: strides larger than a matrix, leading dimensions, a side stream synchronised alone,
    refused calls writing nothing"""
    from mpyc_amd import _ffi, engine
    L = _ffi.lib()
    for modulus, (M, K, N) in [(P128, (4, 4, 4)), (P61, (3, 5, 2)), (P61, (20, 9, 17))]:
        ctx = engine.FieldContext(modulus, device=0)
        eb = ctx.elem_bytes
        rng = random.Random(M * 100 + N)
        nb = 37
        lda, ldb, ldc = K + 3, N + 1, N + 2
        sa, sb, sc = M * lda + 5, K * ldb + 2, M * ldc + 7
        abuf, bbuf = draw(rng, modulus, nb * sa), draw(rng, modulus, nb * sb)
        da, db = ctx.from_ints(abuf.tolist()), ctx.from_ints(bbuf.tolist())
        fill = draw(rng, modulus, nb * sc)
        dc = ctx.from_ints(fill.tolist())
        st = torch.cuda.current_stream(0).cuda_stream
        assert L.ffgpu_matmul_stack(ctx._h, da.ptr, lda, sa, db.ptr, ldb, sb, dc.ptr, ldc, sc, M, K, N, nb, st) == _ffi.OK
        torch.cuda.synchronize()
        got = np.array(dc.to_ints(), dtype=object)
        want = fill.copy()                              # what lies between the matrices of C stays as it was
        for i in range(nb):
            a = np.array([[abuf[i * sa + r * lda + k] for k in range(K)] for r in range(M)], dtype=object)
            b = np.array([[bbuf[i * sb + k * ldb + c] for c in range(N)] for k in range(K)], dtype=object)
            c = np.matmul(a, b) % modulus
            for r in range(M):
                want[i * sc + r * ldc:i * sc + r * ldc + N] = c[r]
        assert (got == want).all(), (hex(modulus), M, K, N)
        # stride 0 on either side, through the C ABI
        dc2 = ctx.from_ints(fill.tolist())
        assert L.ffgpu_matmul_stack(ctx._h, da.ptr, lda, 0, db.ptr, ldb, sb, dc2.ptr, ldc, sc, M, K, N, nb, st) == _ffi.OK
        torch.cuda.synchronize()
        got2 = np.array(dc2.to_ints(), dtype=object)
        a0 = np.array([[abuf[r * lda + k] for k in range(K)] for r in range(M)], dtype=object)
        for i in range(nb):
            b = np.array([[bbuf[i * sb + k * ldb + c] for c in range(N)] for k in range(K)], dtype=object)
            c = np.matmul(a0, b) % modulus
            for r in range(M):
                assert (got2[i * sc + r * ldc:i * sc + r * ldc + N] == c[r]).all(), (hex(modulus), 'shared A', i, r)
        # refused calls write nothing
        snap = raw(dc)
        f = L.ffgpu_matmul_stack
        assert f(ctx._h, da.ptr, K - 1, sa, db.ptr, ldb, sb, dc.ptr, ldc, sc, M, K, N, nb, st) == _ffi.EINVAL
        assert f(ctx._h, da.ptr, lda, M * lda - lda, db.ptr, ldb, sb, dc.ptr, ldc, sc, M, K, N, nb, st) == _ffi.EINVAL
        assert f(ctx._h, da.ptr, lda, sa, db.ptr, ldb, sb, dc.ptr, ldc, 0, M, K, N, nb, st) == _ffi.EINVAL
        assert f(ctx._h, da.ptr, lda, sa, db.ptr, ldb, sb, dc.ptr, ldc, (M - 1) * ldc + N - 1, M, K, N, nb, st) == _ffi.EINVAL
        assert f(ctx._h, da.ptr, lda, sa, db.ptr, ldb, sb, da.ptr, ldc, sc, M, K, N, 2, st) == _ffi.EINVAL
        assert f(ctx._h, dc.ptr + eb, lda, sa, db.ptr, ldb, sb, dc.ptr, ldc, sc, M, K, N, 2, st) == _ffi.EINVAL
        assert f(ctx._h, da.ptr, lda, sa, db.ptr, ldb, sb, None, ldc, sc, M, K, N, nb, st) == _ffi.EINVAL
        assert f(ctx._h, da.ptr, lda, sa, db.ptr, ldb, sb, dc.ptr, ldc, sc, M, K, N, 0, st) == _ffi.OK
        torch.cuda.synchronize()
        assert raw(dc) == snap
        # a stream of its own: correct after synchronising that stream only
        side = torch.cuda.Stream(device=0)
        dc3 = ctx.from_ints(fill.tolist())
        torch.cuda.synchronize()
        assert f(ctx._h, da.ptr, lda, sa, db.ptr, ldb, sb, dc3.ptr, ldc, sc, M, K, N, nb, side.cuda_stream) == _ffi.OK
        side.synchronize()
        assert raw(dc3) == snap
        # engine.matmul_stack: sizes and overlap as matmul checks them
        x, y = ctx.from_ints([1] * (nb * M * K)), ctx.from_ints([1] * (nb * K * N))
        with pytest.raises(ValueError):
            ctx.matmul_stack(x, y, nb + 1, M, K, N, M * K, K * N)
        with pytest.raises(ValueError):
            ctx.matmul_stack(x, y, nb, M, K, N, M * K - 1, K * N)
        with pytest.raises(ValueError):
            ctx.matmul_stack(x, y, nb, M, K, N, M * K, K * N, out=ctx.empty(nb * M * N + 1))
        o = ctx.matmul_stack(x, y, nb, M, K, N, M * K, K * N)
        assert o.to_ints() == [K % modulus] * (nb * M * N)


def test_large_matrices_loop_inside_the_call(api, monkeypatch):
    """matrices at or above FFGPU_MM_STACK_LOOP_MIN go through ffgpu_matmul's routes one after the other inside the ONE
    call; a context created with the switch at 0 takes that loop at every size, one with a huge value never does: both
    give the stack kernels' bytes"""
    from mpyc_amd import engine
    rng = random.Random(13)
    nb, M, K, N = 5, 24, 70, 40
    a, b = draw(rng, P61, nb, M, K), draw(rng, P61, nb, K, N)
    want = (np.matmul(a, b) % P61).reshape(-1).tolist()
    outs = []
    for v in ('0', str(2**31 - 1)):
        monkeypatch.setenv('FFGPU_MM_STACK_LOOP_MIN', v)
        ctx = engine.FieldContext(P61, device=0)
        monkeypatch.delenv('FFGPU_MM_STACK_LOOP_MIN')
        da, db = ctx.from_ints(a.reshape(-1).tolist()), ctx.from_ints(b.reshape(-1).tolist())
        ctx.set_timing(True, accumulate=True)
        ctx.busy_ms()
        o = ctx.matmul_stack(da, db, nb, M, K, N, M * K, K * N)
        ms, calls = ctx.busy_ms()
        ctx.set_timing(False)
        assert calls == 1
        assert o.to_ints() == want, v
        outs.append(raw(o))
    assert outs[0] == outs[1]
