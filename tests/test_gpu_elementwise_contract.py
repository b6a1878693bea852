"""The three promises of include/ffgpu.h about the element-wise entry points -- inputs are never written, `out` may alias an
input exactly, elements are canonical on return -- for add, sub, mul, neg, reduce, the scalar forms, muladd, pow, inv,
beaver_combine and (primes = 1 mod 4; second half of this file) sqrt_cl, on every field policy: every alias pattern at every size at which a path changes, on aligned, one-element-in
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
    sq_pairs, sq_matrix, _ = ew.sqrt_cases_of(drv.q)       # sqrt_cl joins for the two Montgomery primes, which are = 1 mod 4
    assert (sq_pairs == 2) == (modulus in (2**127 + 2**100 + 0x101, 2**192 - 2**40 + 341))
    assert len(drv.seen) == MATRIX_CASES + sq_matrix and drv.steps == 2 * (MATRIX_CASES + sq_matrix)
    # every (entry point, pattern) pair at every size up to 129
    pairs = {(e[0], e[1], p) for e in drv.entries for p in drv.patterns_of(e)}
    assert len(pairs) == 71 + sq_pairs
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
    sq_align = ew.sqrt_cases_of(drv.q)[2]
    assert len(drv.seen) == ALIGN_CASES + sq_align and drv.steps == 2 * (ALIGN_CASES + sq_align)
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


# ---- sqrt_cl: Cipolla-Lehmer for p = 1 mod 4 (k_sqrt_cl) --------------------------------------------------------------------
# The expectation is oracle.pyoracle.sqrt_prime on Python integers, value by value (tests/golden/sqrt.json pins it to the
# reference's FiniteFieldArray.sqrt() on every modulus below): the root the reference returns, not the other one, and its
# non-root for a non-residue.  The operands come from a pool of 1024 elements per field, so the reference runs once per value.
SQRT_FIELDS = ew.sqrt_fields()
SQRT_IDS = ['%s:%s' % (pol, hex(m)) for m, pol, _ in SQRT_FIELDS]
SQRT_MATRIX = 2 * len(ew.SMALL_SIZES) + 2 * len(ew.LARGE_SIZES)
sqrt_checked = {}                   # policy -> cases of sqrt_cl checked by test_sqrt_cl_alias_patterns_sizes_and_alignment


def test_sqrt_field_list_on_the_device():
    for modulus, policy, eb in SQRT_FIELDS:
        ctx = default_ctx(modulus, False)
        assert ctx.elem_bytes == eb and ctx.reduction == ew.REDUCTION_OF[policy[:2]], (hex(modulus), ctx.reduction, ctx.elem_bytes)
    assert {pol for _, pol, _ in SQRT_FIELDS} == set(ew.SQRT_ROWS)


@pytest.mark.parametrize('modulus,policy,eb', SQRT_FIELDS, ids=SQRT_IDS)
def test_sqrt_cl_alias_patterns_sizes_and_alignment(coracle, modulus, policy, eb):
    """fresh and in place at every size of SMALL_SIZES and LARGE_SIZES, then on aligned, one-element-in and mixed views at
    ALIGN_SIZES; the chained second call takes the roots of the first, residues or not"""
    drv = driver(coracle, default_ctx(modulus, False), modulus, False, 12)
    e = drv.entry('sqrt_cl')
    drv.run_matrix(entries=[e])
    assert len(drv.seen) == SQRT_MATRIX and drv.steps == 2 * SQRT_MATRIX
    drv.run_alignment(entries=[e], aligns=('aligned', 'one-in', 'mixed'))
    # (the aligned cases at these sizes are cases of the matrix, run again on other draws)
    assert drv.steps == 2 * (SQRT_MATRIX + 3 * 2 * len(ew.ALIGN_SIZES))
    assert {k[4] for k in drv.seen} == {'aligned', 'one-in', 'mixed'} and {k[0] for k in drv.seen} == {'sqrt_cl'}
    cases = drv.steps // 2
    sqrt_checked[policy] = sqrt_checked.get(policy, 0) + cases
    print('sqrt_cl: %d cases (%d calls) checked on %s %s' % (cases, drv.steps, policy, hex(modulus)))
    assert cases > 0


def test_sqrt_cl_cases_were_checked_on_every_policy(coracle):
    """(after the test above in file order; on its own it runs the first field of every policy itself)"""
    for policy in ew.SQRT_ROWS:
        if policy not in sqrt_checked:
            modulus = next(m for m, pol, _ in SQRT_FIELDS if pol == policy)
            drv = driver(coracle, default_ctx(modulus, False), modulus, False, 13)
            drv.run_matrix(small=(0, 1, 65), large=(), entries=[drv.entry('sqrt_cl')])
            sqrt_checked[policy] = drv.steps // 2
    print('sqrt_cl cases per policy: %r' % sqrt_checked)
    assert all(sqrt_checked[policy] > 0 for policy in ew.SQRT_ROWS)


@pytest.mark.parametrize('modulus,policy,eb', SQRT_FIELDS, ids=SQRT_IDS)
def test_sqrt_cl_chains_without_handoff(coracle, monkeypatch, modulus, policy, eb):
    drv = driver(coracle, env_ctx(monkeypatch, modulus, False, 'FFGPU_HANDOFF', '0'), modulus, False, 14)
    drv.run_matrix(entries=[drv.entry('sqrt_cl')])
    assert len(drv.seen) == SQRT_MATRIX and drv.steps == 2 * SQRT_MATRIX


def mixed_depth_input(drv, n=5003):
    """n operands laid out by wavefront of 64: all zero | zero and non-zero alternating | depth 1 only | deep only (64 of depth
    >= 6, among them 8 of depth >= 8 and 2 of depth >= 11) | four waves that mix residues, non-residues, 0, 1, p - 1, 4^-1,
    9 * 4^-1, b^2 * 4^-1 for b <= 8 and deep elements | random elements.  GF(13): every element, over and over."""
    p, rng = drv.q, drv.rng
    if p == 13:
        return ew.ints_to_bytes([i % 13 for i in range(n)], drv.eb), {}
    deep = ew.deep_elements(p)
    assert [len(deep[lvl]) for lvl in (6, 8, 11)] == [64, 8, 2], 'the walk over the squares reached its bound for %s' % hex(p)
    rand = ew.bytes_to_ints(drv.ref.random(rng, n + 512), drv.eb)
    nonzero = [v for v in rand if v]
    shallow = [v for v in nonzero[:400] if ew.sqrt_depth(p, v) == 1][:64]
    assert len(shallow) == 64
    deepest = deep[11] + [a for a in deep[8] if a not in deep[11]]
    deep_wave = (deepest + [a for a in deep[6] if a not in deepest])[:64]
    assert len(deep_wave) == 64 and set(deep[11]) | set(deep[8]) <= set(deep_wave)
    inv4 = pow(4, -1, p)
    spice = [0, 1, p - 1, inv4, 9 * inv4 % p] + [b * b * inv4 % p for b in range(1, 9)] + deep[11] + deep[8][:4]
    mixed = []
    for w in range(4):
        wave = [int(v) for v in rand[400 + 64 * w:464 + 64 * w]]
        for s, pos in zip(spice, rng.choice(64, size=len(spice), replace=False)):
            wave[pos] = s
        mixed += wave
    vals = [0] * 64 + [0 if i % 2 == 0 else nonzero[i] for i in range(64)] + shallow + deep_wave + mixed
    vals += rand[512 + len(vals):512 + n]
    assert len(vals) == n
    depth = {'deep wave': min(ew.sqrt_depth(p, a) for a in deep_wave), 'max': max(ew.sqrt_depth(p, a) for a in deep_wave)}
    return ew.ints_to_bytes(vals, drv.eb), depth


@pytest.mark.parametrize('modulus,policy,eb', SQRT_FIELDS, ids=SQRT_IDS)
def test_sqrt_cl_waves_of_mixed_search_depth(coracle, modulus, policy, eb):
    """lanes that skip the search (a = 0), lanes that leave it after one candidate next to lanes that need eleven or more, waves
    of one kind only: every one of the 5003 elements equals the reference, with a fresh output and in place"""
    drv = driver(coracle, default_ctx(modulus, False), modulus, False, 15)
    img, depth = mixed_depth_input(drv)
    if modulus != 13:
        assert depth['deep wave'] >= 6 and depth['max'] >= 11
    e = drv.entry('sqrt_cl')
    for pat in ('fresh', 'o=a'):
        drv.run(e, pat, 5003, inputs={'a': img}, chain=False)
    assert len(drv.seen) == 2 and drv.steps == 2


@pytest.mark.parametrize('modulus', [2**40 - 87, 2**80 - 143, 2**136 - 243], ids=hex)
def test_sqrt_cl_capped_grid(coracle, monkeypatch, modulus):
    """FFGPU_BLOCKS_PER_CU=1: G = CUs x 256 threads, n = 2 G + G / 3 + 7, so every thread takes two elements and a third of
    them a third one.  The operands are drawn from the pool with the special and the deep elements, so the integer reference
    is known for every one of them: ALL n elements are compared (the second and the partial pass, and the whole first one),
    after each of the two chained calls, fresh and in place.  v * v = a is checked through the vectorised reference on every
    residue."""
    assert any(m == modulus for m, _, _ in SQRT_FIELDS)
    ctx = env_ctx(monkeypatch, modulus, False, 'FFGPU_BLOCKS_PER_CU', '1')
    drv = driver(coracle, ctx, modulus, False, 16)
    ref, eb = drv.ref, drv.eb
    G = num_cu() * 256
    n = 2 * G + G // 3 + 7
    deep = ew.deep_elements(modulus)
    extra = np.stack([ref.const(v, 1) for v in ew.sqrt_specials(modulus) + deep[8] + deep[11]])
    values = np.concatenate([drv.sqrt_pool(), extra])
    a = values[drv.rng.integers(0, len(values), size=n)].reshape(-1)
    e = drv.entry('sqrt_cl')
    for pat in ('fresh', 'o=a'):
        drv.run(e, pat, n, inputs={'a': a})
    assert len(drv.seen) == 2 and drv.steps == 4
    # the driver found the device's output equal to ref.sqrt_cl(a), byte for byte: square that
    root = ref.sqrt_cl(a)
    euler = {v: v == 0 or pow(v, (modulus - 1) >> 1, modulus) == 1 for v in ew.bytes_to_ints(values.reshape(-1), eb)}
    residue = np.array([euler[v] for v in ew.bytes_to_ints(a, eb)])
    assert 0.3 * n < residue.sum() < 0.7 * n
    assert not (ref.mul(root, root).reshape(n, eb) != a.reshape(n, eb)).any(axis=1)[residue].any()
    assert (ref.mul(root, root).reshape(n, eb) != a.reshape(n, eb)).any(axis=1)[~residue].all()


@pytest.mark.parametrize('modulus,binary', [(0x11b, True), ((1 << 64) | 0x1b, True), (2**61 - 1, False), (2**136 - 113, False),
                                            (2, False)], ids=['gf2:0x11b', 'gf2:2^64', '2^61-1', '2^136-113', '2'])
def test_sqrt_cl_is_refused_elsewhere(coracle, modulus, binary):
    """binary fields, p = 3 mod 4 and p = 2: not supported, and nothing is written -- the pre-filled output, the operand and the
    guards are byte for byte what was uploaded"""
    ctx = default_ctx(modulus, binary)
    drv = driver(coracle, ctx, modulus, binary, 17)
    assert not any(e[0] == 'sqrt_cl' for e in drv.entries)
    eb = drv.eb
    for n in (1, 65, 1025):
        off, total = ew.layout(eb, n, ['a', 'o'], ())
        img = np.full(total, ew.GUARD_BYTE, dtype=np.uint8)
        img[off['a']:off['a'] + n * eb] = drv.draw(drv.entry('neg'), n)
        img[off['o']:off['o'] + n * eb] = drv.rng.integers(0, 256, size=n * eb, dtype=np.uint8)
        base = torch.from_numpy(img.copy()).to(ctx.torch_device)
        a, o = drv._view(base, off['a'], n), drv._view(base, off['o'], n)
        for out in (o, a):
            with pytest.raises(NotImplementedError):
                ctx.sqrt_cl(a, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(base.cpu().numpy(), img), (hex(modulus), n)
