"""The three promises of include/ffgpu.h about the element-wise entry points -- inputs are never written, `out` may alias an
input exactly, elements are canonical on return -- for add, sub, mul, neg, reduce, the scalar forms, muladd, pow, inv and
beaver_combine, on every field policy: every alias pattern at every size at which a path changes, on aligned, one-element-in
and mixed views, with guards around every operand, twice in a row so that the second call reads the first one's output and
stores under the kept-in-cache policy (handoff.hpp), with the hand-off switched off, on a capped grid, on the routes the
launcher picks by size (k_inv_digits, k_inv_fast, k_inv_batch<., 10, 2>, the GF(2^8) table product, the bit-sliced GF(2^64)
product, the window product of dense moduli), and on the limb patterns at which a reduction can go wrong.  The case logic, the
references and the layout are tests/ew_contract.py; tests/test_elementwise_contract_host.py shows that driver fails when it
should.  Expected values never come from the library; every comparison is byte for byte."""
import numpy as np
import pytest

import ew_contract as ew
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

FIELDS = ew.contract_fields()
IDS = [('gf2:' if b else '') + hex(m) for m, b in FIELDS]

# cases per field (a case = entry point x alias pattern x size x alignment class, two chained calls each):
#   27 calls (5 + 3 scalar forms x 4 scalars + muladd + 6 exponents + inv + beaver_combine x 2) in 71 (call, pattern) pairs,
#   54 of them fresh or in place, 50 without the two long exponents
MATRIX_CASES = 71 * 15 + 50 * 4          # every pattern at the 15 sizes up to 129; fresh and in place at the 4 above
ALIGN_CASES = 2 * (54 * 4 + 50)          # two classes; sizes 1, 17, 65, 129 and 1025
REDUCED_CASES = 17 * 15 + 14 * 4         # add, mul, muladd x 3 patterns + mul_scalar x 4 scalars x 2 patterns; 14 fresh / o = a


def test_field_list():
    from test_gpu_scan import ALL_FIELDS
    assert FIELDS[:18] == ALL_FIELDS and len(FIELDS) == 20
    assert all(b and po.Field(m, True).order in (1 << 64, 1 << 128) for m, b in FIELDS[18:])


_ctxs = {}


def default_ctx(modulus, binary):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from mpyc_amd import engine
    if (modulus, binary) not in _ctxs:
        _ctxs[modulus, binary] = engine.FieldContext(modulus, binary, device=0)
    return _ctxs[modulus, binary]


def env_ctx(monkeypatch, modulus, binary, name, value):
    """a context of its own with one launch switch set (they are read at creation)"""
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from mpyc_amd import engine
    monkeypatch.setenv(name, value)
    ctx = engine.FieldContext(modulus, binary, device=0)
    monkeypatch.delenv(name)
    return ctx


def driver(coracle, ctx, modulus, binary, salt=0):
    return ew.Driver(ctx, ew.make_ref(coracle, modulus, binary), seed=modulus % 1009 + salt)


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_alias_patterns_at_every_edge_size(coracle, modulus, binary):
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary)
    drv.run_matrix()
    assert len(drv.seen) == MATRIX_CASES and drv.steps == 2 * MATRIX_CASES
    # every (entry point, pattern) pair at every size up to 129
    pairs = {(e[0], e[1], p) for e in drv.entries for p in drv.patterns_of(e)}
    assert len(pairs) == 71
    assert all((name, label, pat, n, 'aligned') in drv.seen for name, label, pat in pairs for n in ew.SMALL_SIZES)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_alignment_classes(coracle, modulus, binary):
    """all operands one element past a 16-byte boundary (24-byte elements: the 8-byte-aligned path; 12-byte: dwordx3 at an odd
    dword), and one operand so with the rest aligned, which sends the whole call to the scalar loop"""
    ctx = default_ctx(modulus, binary)
    if ctx.elem_bytes == 16:
        return                          # every view of 16-byte elements is 16-byte aligned: no such class
    drv = driver(coracle, ctx, modulus, binary, 1)
    drv.run_alignment()
    assert len(drv.seen) == ALIGN_CASES and drv.steps == 2 * ALIGN_CASES
    assert {k[4] for k in drv.seen} == {'one-in', 'mixed'}


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_chains_without_handoff(coracle, monkeypatch, modulus, binary):
    """the same chains with every store non-temporal (FFGPU_HANDOFF=0)"""
    drv = driver(coracle, env_ctx(monkeypatch, modulus, binary, 'FFGPU_HANDOFF', '0'), modulus, binary, 2)
    drv.run_reduced()
    assert len(drv.seen) == REDUCED_CASES and drv.steps == 2 * REDUCED_CASES


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_capped_grid(coracle, monkeypatch, modulus, binary):
    """FFGPU_BLOCKS_PER_CU=1: G = CUs x 256 threads take more than three packs each, so both loops of stream_map iterate;
    n = 3 G EPV + EPV + 1 (24-byte elements, which move in waves of 64: 3 G + 65)"""
    ctx = env_ctx(monkeypatch, modulus, binary, 'FFGPU_BLOCKS_PER_CU', '1')
    drv = driver(coracle, ctx, modulus, binary, 3)
    eb = ctx.elem_bytes
    G = num_cu() * 256
    epv = 16 // eb if eb <= 8 else 1
    n = 3 * G + 65 if eb == 24 else 3 * G * epv + epv + 1
    ins = {s: drv.draw(drv.entry('add'), n) for s in 'abc'}          # drawn once, shared by the cases
    raw = {'a': drv.draw(drv.entry('reduce'), n)}
    for name, label, pats in (('add', '', ('fresh', 'o=a', 'o=b', 'o=a=b')), ('mul', '', ('fresh', 'o=a', 'o=b', 'o=a=b')),
                              ('muladd', '', ('fresh', 'o=a', 'o=b', 'o=a=b=c')), ('reduce', '', ('fresh', 'o=a')),
                              ('mul_scalar', 'rnd', ('fresh', 'o=a')), ('inv', '', ('fresh', 'o=a'))):
        for pat in pats:
            drv.run(drv.entry(name, label), pat, n, inputs=raw if name == 'reduce' else ins)
    assert len(drv.seen) == 18
    if eb in (4, 8):                    # the capped scalar loop: views one element in
        m = 3 * G + 1
        for name in ('add', 'mul'):
            for pat in ('fresh', 'o=a'):
                drv.run(drv.entry(name), pat, m, 'one-in', inputs={s: v[:m * eb] for s, v in ins.items()})
        assert len(drv.seen) == 22


# ---- routes chosen by size --------------------------------------------------------------------------------------------
def fields_where(pred):
    sel = [(m, b) for m, b in FIELDS if pred(m, b, ew_elem_bytes(m, b))]
    return {'argvalues': sel, 'ids': [('gf2:' if b else '') + hex(m) for m, b in sel]}


def ew_elem_bytes(modulus, binary):
    from oracle.coracle import elem_bytes
    return elem_bytes(modulus, binary)


@pytest.mark.parametrize('modulus,binary', **fields_where(lambda m, b, eb: not b and eb >= 12))
def test_inverse_of_multi_limb_primes(coracle, modulus, binary):
    """4096 + 37 elements: the digit kernel (k_inv_digits) for the 2^k - c primes, fresh and in place"""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 4)
    n = 4096 + 37
    e = drv.entry('inv')
    for pat in ('fresh', 'o=a'):
        drv.run(e, pat, n, inputs={'a': drv.plant(e, n, {0: 0, 4095: 0, 4096: 0, n - 1: 0})})
    assert len(drv.seen) == 2


@pytest.mark.parametrize('modulus,binary', **fields_where(lambda m, b, eb: not b and eb == 8))
def test_inverse_of_one_word_primes_full_batches(coracle, modulus, binary):
    """2 x 32768 + 5 elements: k_inv_fast, zeros at the first and last element and at a block edge (8192 elements a block)"""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 5)
    n = 2 * 32768 + 5
    e = drv.entry('inv')
    for pat in ('fresh', 'o=a'):
        drv.run(e, pat, n, inputs={'a': drv.plant(e, n, {0: 0, 8191: 0, 8192: 0, n - 1: 0})})
    assert len(drv.seen) == 2


def test_gf256_table_product(coracle):
    drv = driver(coracle, default_ctx(0x11b, True), 0x11b, True, 6)
    for pat in ('fresh', 'o=a'):
        drv.run(drv.entry('mul'), pat, 2**18 + 21)
    assert len(drv.seen) == 2


def test_gf256_inverse_sees_a_zero_at_every_byte_of_a_batch(coracle):
    """A thread of k_inv_batch over packed bytes holds 2 packs of 16 bytes; the patch-up of zeros runs only in waves that saw
    one.  One zero per wave, at each of the 32 byte positions of a thread's batch in turn, every other element non-zero (found
    by test_capped_grid: the marks of bytes 1..3 of the last three words were shifted out of the 64-bit mask, so a zero there
    that was alone in its wave was missed: no flag, a non-zero inverse, and zeros in its byte lane of the earlier words).
    n = 32 waves x 64 threads x 32 bytes: thread t of 2048 holds packs t and t + 2048."""
    ctx = default_ctx(0x11b, True)
    drv = driver(coracle, ctx, 0x11b, True, 11)
    n, threads = 32 * 64 * 32, 32 * 64
    e = drv.entry('inv')
    a = drv.draw(e, n)
    a[a == 0] = 0x53
    zeros = [((k // 16) * threads + 64 * k + 1) * 16 + k % 16 for k in range(32)]
    a[zeros] = 0
    for pat in ('fresh', 'o=a'):
        drv.run(e, pat, n, inputs={'a': a})
    assert len(drv.seen) == 2
    for z in zeros:                       # the zero flag: a single zero anywhere raises
        one = np.full(n, 0x53, dtype=np.uint8)
        one[z] = 0
        with pytest.raises(ZeroDivisionError):
            ctx.inv(ctx.from_numpy(one))
    ctx.inv(ctx.from_numpy(np.full(n, 0x53, dtype=np.uint8)))


def test_gf2w64_bitsliced_product(coracle):
    """the bit-sliced kernel and its tail with out = b and out = a = b (out = a: tests/test_gpu_parity.py)"""
    mod = (1 << 64) | 0x1b
    drv = driver(coracle, default_ctx(mod, True), mod, True, 7)
    for pat in ('o=b', 'o=a=b'):
        drv.run(drv.entry('mul'), pat, 2**21 + 2048 * 3 + 5)
    assert len(drv.seen) == 2


@pytest.mark.parametrize('modulus,binary', FIELDS[18:], ids=IDS[18:])
def test_dense_moduli_window_product(coracle, modulus, binary):
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 8)
    for pat in drv.patterns_of(drv.entry('mul')):
        drv.run(drv.entry('mul'), pat, 4099)
    assert len(drv.seen) == 5


def inv_batch_ch(nvec, cus):
    """the rule of launch.hpp (inv, one-word fields outside k_inv_fast): the launch runs in rounds of 2 x 4 x CUs waves;
    CH = 10 is taken when rounds x (12 CH + 73) is 3 % below that of CH = 8"""
    slots = cus * 4 * 2
    cost = {}
    for ch in (8, 10):
        waves = (nvec // (2 * ch) + 63) // 64 + 1
        cost[ch] = -(-waves // slots) * (12 * ch + 73)
    return 10 if cost[10] < cost[8] * 0.97 else 8


@pytest.mark.parametrize('deg', [64, 40])
def test_batched_inverse_ten_packs_per_thread(coracle, deg):
    """k_inv_batch<., 10, 2>, which no other test reaches: GF(2^n), 33 <= n <= 64, at a size where CH = 8 needs two scheduling
    rounds and CH = 10 one.  The rule is recomputed here for this device's CU count, so that a device on which the size
    selects CH = 8 fails instead of testing the wrong kernel."""
    from mpyc_amd.gfpx import BinaryPolynomial
    modulus = int(BinaryPolynomial.next_irreducible(1 << deg))
    slots = num_cu() * 8
    n = 2 * (slots * 1024 + 32768) + 1
    assert inv_batch_ch(n // 2, num_cu()) == 10, 'this size does not select CH = 10 on %d CUs' % num_cu()
    ctx = default_ctx(modulus, True)
    assert ctx.elem_bytes == 8
    drv = driver(coracle, ctx, modulus, True, 9)
    e = drv.entry('inv')
    for pat in ('fresh', 'o=a'):         # (one call each: four million products of the oracle per check)
        drv.run(e, pat, n, inputs={'a': drv.plant(e, n, {0: 0, 5: 0, n // 2: 0, n - 1: 0})}, chain=False)
    assert len(drv.seen) == 2 and drv.steps == 2


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_reduce_of_noncanonical_patterns(coracle, modulus, binary):
    """p, p + 1, 2p - 1, 2p, the largest multiple of p below 2^W and its neighbours, 2^W - 1, 2^(W-1); for GF(2^n) the modulus,
    2^n, 2^n | 1, all ones, a lone top bit -- against % p and pyoracle.clmod, fresh and in place"""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 10)
    planted = ew.run_noncanonical_reduce(drv, po.clmod)
    W = 8 * drv.eb
    assert planted == len(ew.noncanonical_values(modulus, binary, drv.eb)) >= 2
    assert (1 << W) - 1 in ew.noncanonical_values(modulus, binary, drv.eb)
    assert len(drv.seen) == 2
