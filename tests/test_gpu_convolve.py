"""np.convolve on field arrays through the convolution kernel (k_convolve, ffgpu_convolve): every field policy at the
tile and tap-chunk edges, the accumulator bound, long operands, memory linear in the inputs, sizes the composed route
cannot reach, the C ABI, np.polymul.  Expected values never come from the code under test: prime fields take what the
reference computes (np.convolve on dtype=object arrays of Python ints, then % p -- finfields.py:801, 807), GF(2^n)
the carry-less oracle (oracle.pyoracle.clmul, XOR accumulation, one clmod per output).  Bit-exact."""
import random
import time

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

P61, P128 = 2**61 - 1, 2**128 - 173
# kernel geometry (mpyc_amd/csrc/convolve_geom.hpp): outputs per workgroup of the narrow and the wide shape, taps per
# chunk, tap groups of the two shapes.  Below 2 wide tiles per compute unit (65 536 outputs on 256 of them) the launcher
# takes the narrow shape, so the small cases below run the wide one on a context created with FFGPU_CONV_WIDE_PER_CU=0.
TO_NARROW, TO_WIDE, TV, G_NARROW, G_WIDE = 32, 128, 64, 16, 4


def prime_moduli():
    """one modulus per prime policy: RC32 (two sizes), PM64 Mersenne / k = 64 / 2^k - c, RC64, PM96 (two sizes),
    PM128 k < 128 / k = 128, MONT128 (the first prime above 2^127 + 2^100), PM192, MONT192 (the first prime above
    2^192 - 2^40)"""
    return [2**31 - 1, 19, P61, 2**64 - 189, 2**63 - 25, 6616326157076047771, 2**80 - 65, 2**96 - 17, 2**127 - 1,
            P128, 2**127 + 2**100 + 0x101, 2**136 - 113, 2**192 - 2**40 + 341]


def binary_moduli():
    """GF2P8, GF2W32 (two sizes), GF2W64, GF2W128: the first irreducible polynomial of degree 8, 16, 32, 64, 128"""
    return [0x11b, 0x1002b, 0x10000008d, 0x1000000000000001b, 0x100000000000000000000000000000087]


def test_moduli_are_what_they_claim():
    from mpyc_amd.finfields import is_prime, next_prime
    from mpyc_amd.gfpx import BinaryPolynomial
    assert all(is_prime(p) for p in prime_moduli())
    assert next_prime(2**127 + 2**100) == prime_moduli()[10] and next_prime(2**192 - 2**40) == prime_moduli()[12]
    assert binary_moduli() == [int(BinaryPolynomial.next_irreducible(1 << d)) for d in (8, 16, 32, 64, 128)]


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    from mpyc_amd import finfields, gfpx
    return finfields, gfpx


def gf(api, modulus, binary=False):
    finfields, gfpx = api
    return finfields.GF(gfpx.BinaryPolynomial(modulus)) if binary else finfields.GF(modulus)


def ints(a):
    return [int(x) for x in np.asarray(a.value).reshape(-1)]


def wide_context(monkeypatch, modulus, binary=False):
    """a context of its own whose convolutions take the wide shape at every size (the switch is read at creation)"""
    from mpyc_amd import engine
    monkeypatch.setenv('FFGPU_CONV_WIDE_PER_CU', '0')
    ctx = engine.FieldContext(modulus, binary, device=0)
    monkeypatch.delenv('FFGPU_CONV_WIDE_PER_CU')
    return ctx


def draw(rng, order, n):
    vals = [rng.randrange(order) for _ in range(n)]
    for i, e in enumerate((order - 1, 0, 1)):          # edge values where there is room
        if 2 * i + 1 < n:
            vals[rng.randrange(n)] = e
    return vals


def expect_full(modulus, binary, a, v):
    if not binary:
        c = np.convolve(np.array(a, dtype=object), np.array(v, dtype=object))
        return [int(x) % modulus for x in c]
    out = [0] * (len(a) + len(v) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(v):
            out[i + j] ^= po.clmul(x, y)
    return [po.clmod(c, modulus) for c in out]


def check_all_modes(F, modulus, binary, a, v, tag, wide):
    """both operand orders and all three modes against slices of ONE full expectation, every element; the full
    convolution in both orders through the wide shape as well"""
    na, nv = len(a), len(v)
    full = expect_full(modulus, binary, a, v)
    da, dv = wide.from_ints(a), wide.from_ints(v)
    assert wide.convolve(da, dv).to_ints() == full, ('wide',) + tag
    assert wide.convolve(dv, da).to_ints() == full, ('wide swapped',) + tag
    fa, fv = F.array(a), F.array(v)
    assert ints(np.convolve(fa, fv)) == full, ('full',) + tag
    assert ints(np.convolve(fv, fa)) == full, ('swapped',) + tag
    lo = (min(na, nv) - 1) // 2
    assert ints(np.convolve(fa, fv, 'same')) == full[lo:lo + max(na, nv)], ('same',) + tag
    assert ints(np.convolve(fv, fa, 'same')) == full[lo:lo + max(na, nv)], ('same swapped',) + tag
    assert ints(np.convolve(fa, fv, 'valid')) == full[min(na, nv) - 1:max(na, nv)], ('valid',) + tag


def prime_cases():
    cases = [(na, nv) for na in (1, 2, 63, 64, 65, 700, 2049) for nv in (1, 2, 3, 33, 257) if nv <= na]
    # one below / at / one above the output tile (na + nv - 1 = TO, 2 TO for both shapes) and the tap chunk (nv = TV, 2 TV)
    for TO in (TO_NARROW, TO_WIDE):
        cases += [(TO - 3, 3), (TO - 2, 3), (TO - 1, 3), (2 * TO - 3, 3), (2 * TO - 2, 3), (2 * TO - 1, 3)]
    cases += [(300, TV - 1), (300, TV), (300, TV + 1), (300, 2 * TV - 1), (300, 2 * TV), (300, 2 * TV + 1)]
    return cases


@pytest.mark.parametrize('modulus', prime_moduli(), ids=hex)
def test_every_prime_policy_at_tile_edges(api, monkeypatch, modulus):
    F = gf(api, modulus)
    wide = wide_context(monkeypatch, modulus)
    rng = random.Random(modulus & 0xffff)
    for na, nv in prime_cases():
        check_all_modes(F, modulus, False, draw(rng, modulus, na), draw(rng, modulus, nv), (hex(modulus), na, nv), wide)


@pytest.mark.parametrize('modulus', binary_moduli(), ids=hex)
def test_every_binary_policy_at_tile_edges(api, monkeypatch, modulus):
    F = gf(api, modulus, True)
    wide = wide_context(monkeypatch, modulus, True)
    order = 1 << (modulus.bit_length() - 1)
    rng = random.Random(modulus & 0xffff)
    cases = [(1, 1), (2, 1), (64, 3), (65, 33), (700, 33)]
    for TO in (TO_NARROW, TO_WIDE):                                          # tile and chunk edges
        cases += [(TO - 2, 2), (TO - 1, 2), (TO, 2)]
    cases += [(TV + 2, TV - 1), (TV + 2, TV), (TV + 2, TV + 1)]
    for na, nv in cases:
        assert na * nv <= 25000
        check_all_modes(F, modulus, True, draw(rng, order, na), draw(rng, order, nv), (hex(modulus), na, nv), wide)


@pytest.mark.parametrize('modulus', prime_moduli(), ids=hex)
def test_accumulator_bound(api, monkeypatch, modulus):
    """a = v = [p - 1] * n is the worst case for an unreduced sum: c[k] = min(k, 2n - 2 - k) + 1 (mod p).
    n = 3 x the flush bound + 1 for both accumulator kinds (192 terms for F::acc, 32 for the digit columns), and G times
    that, because the kernel spreads an output's terms over G accumulators (16 in the narrow shape, 4 in the wide one)."""
    F = gf(api, modulus)
    wide = wide_context(monkeypatch, modulus)
    for n in (3 * 32 + 1, 3 * 192 + 1, G_WIDE * 3 * 32 + 1, G_NARROW * 3 * 32 + 1, G_WIDE * 3 * 192 + 1, G_NARROW * 3 * 192 + 1):
        a = F.array([modulus - 1] * n)
        want = [(min(k, 2 * n - 2 - k) + 1) % modulus for k in range(2 * n - 1)]
        assert ints(np.convolve(a, a)) == want, (hex(modulus), n)
        if n <= G_WIDE * 3 * 192 + 1:
            assert wide.convolve(a._dev, a._dev).to_ints() == want, ('wide', hex(modulus), n)


@pytest.mark.parametrize('modulus', [P61, P128], ids=hex)
def test_long_by_long(api, modulus):
    F = gf(api, modulus)
    rng = random.Random(4096)
    a, v = draw(rng, modulus, 4096), draw(rng, modulus, 4096)
    assert ints(np.convolve(F.array(a), F.array(v))) == expect_full(modulus, False, a, v)


@pytest.mark.parametrize('modulus,na,nv', [(P61, 10**6, 64), (2**80 - 65, 10**5, 7)], ids=['p61-1e6x64', 'p80-1e5x7'])
def test_long_by_short(api, modulus, na, nv):
    F = gf(api, modulus)
    rng = random.Random(na)
    a, v = draw(rng, modulus, na), draw(rng, modulus, nv)
    got = ints(np.convolve(F.array(a), F.array(v)))
    assert got == expect_full(modulus, False, a, v)


def test_memory_is_linear_in_the_inputs(api):
    """4096 x 4096 over 2^61 - 1: the call may allocate at most 64 (na + nv) elements + 1 MiB beyond its operands.  The
    kernel needs the output only (it has no scratch, in torch or in the library); the Toeplitz route gathers
    nv = 4096 times the output."""
    F = gf(api, P61)
    na = nv = 4096
    rng = random.Random(5)
    a, v = F.array(draw(rng, P61, na)), F.array(draw(rng, P61, nv))
    eb = a.ctx.elem_bytes
    assert eb == 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    c = np.convolve(a, v)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak extra memory of a 4096 x 4096 convolution: {extra} bytes (output: {(na + nv - 1) * eb})')
    assert extra <= 64 * (na + nv) * eb + (1 << 20), extra
    assert c.shape == (na + nv - 1,)


@pytest.mark.timeout(120)
def test_beyond_the_composed_route(api):
    """131072 x 131072 over 2^61 - 1: the Toeplitz route would need two index tensors of 550 GB; the kernel needs the
    2 MB output.  Checked by direct Python sums at the first and last 64 outputs and 256 seeded positions, and for
    EVERY output by sum c[k] = (sum a)(sum v) and C(r) = A(r) V(r) at a fixed random r (a wrong output escapes the
    second with probability below 2^-43).  Device time on one MI355X: 10.6 ms for the first call (host clock around a
    synchronise, printed below); the whole test about 1 s, the Python sums included."""
    F = gf(api, P61)
    p = P61
    na = nv = 131072
    rs = np.random.default_rng(20261016)
    a = [int(x) % p for x in rs.integers(0, 2**63, na, dtype=np.uint64)]
    v = [int(x) % p for x in rs.integers(0, 2**63, nv, dtype=np.uint64)]
    a[0], a[-1], v[0], v[-1] = p - 1, p - 1, p - 1, 1
    fa, fv = F.array(a), F.array(v)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fc = np.convolve(fa, fv)
    torch.cuda.synchronize()
    print(f'131072 x 131072 convolution: {(time.perf_counter() - t0) * 1e3:.1f} ms (first call, host clock)')
    c = ints(fc)
    nout = na + nv - 1
    assert len(c) == nout and all(0 <= x < p for x in c)
    ar = a[::-1]
    pos = list(range(64)) + list(range(nout - 64, nout)) + sorted(random.Random(6).sample(range(64, nout - 64), 256))
    for k in pos:
        jlo, jhi = max(0, k - na + 1), min(k, nv - 1)            # c[k] = sum_{j = jlo..jhi} a[k - j] v[j]
        s = sum(x * y for x, y in zip(ar[na - 1 - (k - jlo):na - (k - jhi)], v[jlo:jhi + 1]))
        assert c[k] == s % p, k
    assert sum(c) % p == (sum(a) % p) * (sum(v) % p) % p
    r = random.Random(7).randrange(2, p - 1)

    def horner(coeffs):
        acc = 0
        for x in reversed(coeffs):
            acc = (acc * r + x) % p
        return acc
    assert horner(c) == horner(a) * horner(v) % p


def test_c_abi(api):
    """ffgpu_convolve directly: operand order, argument checks, stream"""
    from mpyc_amd import _ffi, engine
    L = _ffi.lib()
    ctx = engine.FieldContext(P128, device=0)
    rng = random.Random(8)
    na, nv = 1000, 77
    a, v = draw(rng, P128, na), draw(rng, P128, nv)
    da, dv = ctx.from_ints(a), ctx.from_ints(v)
    n = na + nv - 1
    o1, o2 = ctx.empty(n), ctx.empty(n)
    st = torch.cuda.current_stream(0).cuda_stream
    assert L.ffgpu_convolve(ctx._h, da.ptr, na, dv.ptr, nv, o1.ptr, st) == _ffi.OK
    assert L.ffgpu_convolve(ctx._h, dv.ptr, nv, da.ptr, na, o2.ptr, st) == _ffi.OK
    torch.cuda.synchronize()
    assert o1.to_numpy().tobytes() == o2.to_numpy().tobytes()
    want = expect_full(P128, False, a, v)
    assert o1.to_ints() == want
    # zero lengths, null pointers
    assert L.ffgpu_convolve(ctx._h, da.ptr, 0, dv.ptr, nv, o1.ptr, st) == _ffi.EINVAL
    assert L.ffgpu_convolve(ctx._h, da.ptr, na, dv.ptr, 0, o1.ptr, st) == _ffi.EINVAL
    assert L.ffgpu_convolve(ctx._h, da.ptr, na, dv.ptr, nv, None, st) == _ffi.EINVAL
    # out overlapping an operand (either one, from either end)
    eb = ctx.elem_bytes
    big = ctx.empty(3 * n)
    big.t.zero_()
    base = big.ptr
    A, V, O = base, base + na * eb, base + (na + nv) * eb                 # a | v | out, back to back: fine
    assert L.ffgpu_convolve(ctx._h, A, na, V, nv, O, st) == _ffi.OK
    assert L.ffgpu_convolve(ctx._h, A, na, V, nv, O - eb, st) == _ffi.EINVAL          # last element of v
    assert L.ffgpu_convolve(ctx._h, A, na, V, nv, A, st) == _ffi.EINVAL
    assert L.ffgpu_convolve(ctx._h, O + (n - 1) * eb, na, V, nv, O, st) == _ffi.EINVAL   # a starts at out's last element
    torch.cuda.synchronize()
    assert o1.to_ints() == want                                            # refused calls wrote nothing
    with pytest.raises(ValueError):
        ctx.convolve(da, dv, out=ctx.empty(n + 1))
    with pytest.raises(ValueError):
        ctx.convolve(da, ctx.empty(0))
    # a stream of its own: correct after synchronising that stream only
    side = torch.cuda.Stream(device=0)
    o3 = ctx.empty(n)
    torch.cuda.synchronize()
    assert L.ffgpu_convolve(ctx._h, da.ptr, na, dv.ptr, nv, o3.ptr, side.cuda_stream) == _ffi.OK
    side.synchronize()
    assert o3.to_ints() == want
    with torch.cuda.stream(side):
        o4 = ctx.convolve(da, dv)
    side.synchronize()
    assert o4.to_ints() == want


def test_polymul_is_the_convolution(api):
    for modulus in (P61, 2**96 - 17):
        F = gf(api, modulus)
        rng = random.Random(1000)
        a, b = draw(rng, modulus, 1001), draw(rng, modulus, 1001)
        a[0] = b[0] = 1                                                     # leading coefficients: degree exactly 1000
        want = expect_full(modulus, False, a, b)
        assert ints(np.polymul(F.array(a), F.array(b))) == want
        assert ints(np.convolve(F.array(a), F.array(b))) == want
