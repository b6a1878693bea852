"""The driver of the sharing contract (tests/share_contract.py) without a GPU: it passes on the Python-integer adapter, and
it fails -- with the right kind of violation -- on seven adapters that break the contract of include/ffgpu.h the way a kernel
or a launcher could.  A driver that cannot see these would not see the kernel bugs it exists for.  The adapter draws its
coefficients with oracle.pyoracle's ChaCha and the layout restated in share_contract.rng_coeffs_ints, the driver expects the C
oracle's (Python integers and the C oracle's block function for 24-byte elements), so the restatement is checked too."""
import numpy as np
import pytest

import share_contract as sc
from share_contract import PyAdapter

GF256, P61, P128, P136 = (0x11b, True), (2**61 - 1, False), (2**127 + 2**100 + 0x101, False), (2**136 - 113, False)
FIELDS = [GF256, P61, P128, P136]                       # one-byte, 8-byte, 16-byte and 24-byte elements
IDS = [hex(m) for m, _ in FIELDS]
SIZES = (0, 1, 3, 17, 65)            # thinned: Python integers
FULL = (1, 17)


def driver(coracle, cls, modulus, binary, salt=0):
    ref = sc.ShareRef(coracle, modulus, binary)
    return sc.Driver(cls(modulus, binary, ref.eb), ref, seed=modulus % 1009 + salt)


def test_layout_rules():
    assert [sc.pack_unit(eb) for eb in (1, 4, 8, 12, 16, 24)] == [16, 4, 2, 1, 1, 2]
    assert sc.stride_classes(8) == ('tight', 'pack', 'pack+1', 'pitched', 'one-in')
    assert sc.stride_classes(12) == ('tight', 'pack+1', 'pitched', 'one-in')
    assert sc.stride_classes(16) == ('tight', 'pack+1', 'pitched')
    # 'pack+1': the base is aligned and the stride is not a whole pack (24-byte elements: an odd stride)
    for eb in (1, 4, 8, 24):
        for n in sc.SMALL_SIZES + sc.LARGE_SIZES:
            assert (sc.stride_of(eb, n, 'pack') * eb) % 16 == 0 and (sc.stride_of(eb, n, 'pack+1') * eb) % 16 != 0
            assert n <= sc.stride_of(eb, n, 'pack') < n + sc.pack_unit(eb) and (sc.stride_of(eb, n, 'pitched') * eb) % 256 == 0
    assert sc.stride_of(24, 65, 'pack+1') == 67 and sc.stride_of(1, 129, 'pack+1') == 145
    lay = sc.Layout(8)
    a = lay.vec('a', 5, one_in=True)
    o = lay.mat('o', 'out', 3, 7, 5)
    assert a % 16 == 8 and a >= 64 * 8 and o % 16 == 0 and o - (a + 40) >= 64 * 8 and lay.total() - (o + 21 * 8) >= 64 * 8
    assert lay.regions[1]['rows'] == [o, o + 56, o + 112] and lay.regions[1]['bytes'] == 21 * 8


@pytest.mark.parametrize('modulus,binary', [f for f in sc.contract_fields() if f[0].bit_length() <= 129],
                         ids=lambda v: hex(v) if isinstance(v, int) and not isinstance(v, bool) else str(v))
def test_generator_restatement_matches_the_oracle(coracle, modulus, binary):
    """rng_coeffs_ints (with pyoracle's ChaCha) against fforacle.c on every contract field the C oracle covers: the 24-byte
    reference and the integer adapter stand on it"""
    cf = coracle.CField(modulus, binary)
    for t, n, rounds, nonce in ((1, 37, 20, sc.NONCE), (3, 21, 8, sc.NONCE + (2 << 40)), (5, 9, 12, 7)):
        want = np.ascontiguousarray(coracle.rng_coeffs(cf, sc.KEY, nonce, rounds, t, n)).view(np.uint8).reshape(t, n * cf.eb)
        got = sc.rng_coeffs_ints(modulus, binary, cf.eb, sc.KEY, nonce, rounds, t, n, sc.block_from_pyoracle)
        assert [sc.bytes_to_ints(r, cf.eb) for r in want] == got
        assert got == sc.rng_coeffs_ints(modulus, binary, cf.eb, sc.KEY, nonce, rounds, t, n, sc.block_from_coracle(coracle))


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_driver_passes_on_the_integer_adapter(coracle, modulus, binary):
    drv = driver(coracle, PyAdapter, modulus, binary)
    eb, q = drv.eb, drv.q
    drv.run_reduced(SIZES)
    assert len(drv.seen) == drv.cases == sc.count_reduced(eb, q, len(SIZES))
    # two calls per case: the two state entry points of share generation, and the gate on a state
    assert drv.steps == drv.cases + 2 * 2 * len(SIZES) * 2 + len(SIZES) * 2
    z = dict(small=(), full=FULL, large=())
    c = dict(small=0, full=len(FULL), large=0)
    seen = drv.cases
    drv.run_split_matrix(drv.SPLIT_HOST + ('rng_coeffs',), **z)
    assert drv.cases - seen == sc.count_split(eb, q, drv.SPLIT_HOST + ('rng_coeffs',), **c)
    seen = drv.cases
    drv.run_split_matrix(drv.SPLIT_RNG, **z)
    assert drv.cases - seen == sc.count_split(eb, q, drv.SPLIT_RNG, **c)
    seen = drv.cases
    drv.run_recombine_matrix(**z)
    assert drv.cases - seen == sc.count_recombine(eb, **c)
    seen = drv.cases
    drv.run_gate_matrix(**z)
    assert drv.cases - seen == sc.count_gate(eb, **c)
    seen = drv.cases
    drv.run_batch_matrix(**z)
    assert drv.cases - seen == sc.count_batch(eb, **c)
    for cls in ('pack+1', 'tight'):
        drv.run_chain(2, 5, 17, cls)
    steps = drv.steps
    assert drv.run_status() == 22 and drv.steps == steps + 22


# ---- adapters that are wrong the way a kernel or a launcher could be ---------------------------------------------------------
class StoresWholePacks(PyAdapter):
    """rounds every row's tail up to a whole pack (24-byte elements: a whole wave of 64; 16-byte ones: two elements)"""

    def store(self, buf, off, vals, first):
        unit = {24: 64, 16: 2}.get(self.eb, 16 // self.eb)
        super().store(buf, off, list(vals) + [0] * (-len(vals) % unit), first)


class TightRowsAfterTheFirst(PyAdapter):
    """uses n for the stride of rows r > 0"""

    def row(self, base, r, stride, n):
        return base + r * n * self.eb


class PointsFromZero(PyAdapter):
    """evaluates at the points 0..m-1"""

    def point(self, i):
        return i


class BatchStrideOnOutputOnly(PyAdapter):
    """applies the batch stride to the output but not to the operands"""

    def batch(self, which, y, stride):
        return y * stride * self.eb if which == 'o' else 0


class SecondChunkAtRowZero(PyAdapter):
    """writes the second chunk of a w > 8 recombination at row 0"""

    def chunk_row(self, r0):
        return 0


class WritesFactorBack(PyAdapter):
    """writes the recombined factor back into rows_a[0]"""

    def gate_done(self, buf, rows_a, A):
        super().store(buf, rows_a[0], A, False)


class OneElementBefore(PyAdapter):
    """writes one element before the first row"""

    def store(self, buf, off, vals, first):
        super().store(buf, off, vals, first)
        if first and vals:
            buf[off - self.eb:off] = 0


def probe(drv):
    """a slice of the matrix that holds what each wrong adapter gets wrong"""
    for n in (3, 17):
        for cls in ('pack+1', 'tight'):
            drv.run_split('split', 1, 3, n, cls)
            drv.run_split('split_rng', 2, 5, n, cls)
            drv.run_recombine(3, 9, n, cls)
            drv.run_gate('3', '0', 1, n, cls)
            drv.run_gate('1', '3', 1, n, 'aligned', nbatch=3, plus=(1, 0, 1))


WRONG = [(StoresWholePacks, 'pad'), (TightRowsAfterTheFirst, 'out'), (PointsFromZero, 'out'), (BatchStrideOnOutputOnly, 'out'),
         (SecondChunkAtRowZero, 'out'), (WritesFactorBack, 'input'), (OneElementBefore, 'guard')]


@pytest.mark.parametrize('cls,kind', WRONG, ids=[c.__name__ for c, _ in WRONG])
def test_driver_fails_on_a_wrong_adapter(coracle, cls, kind):
    for modulus, binary in FIELDS:
        kinds = set()
        drv = driver(coracle, cls, modulus, binary, 1)
        # every case of the slice on its own, so that one violation does not hide another kind
        for n in (3, 17):
            for c in ('pack+1', 'tight'):
                for run in (lambda: drv.run_split('split', 1, 3, n, c), lambda: drv.run_split('split_rng', 2, 5, n, c),
                            lambda: drv.run_recombine(3, 9, n, c), lambda: drv.run_gate('3', '0', 1, n, c),
                            lambda: drv.run_gate('1', '3', 1, n, 'aligned', nbatch=3, plus=(1, 0, 1))):
                    try:
                        run()
                    except sc.ContractViolation as err:
                        kinds |= err.kinds
        assert kind in kinds, (cls.__name__, hex(modulus), kinds)
        good = driver(coracle, PyAdapter, modulus, binary, 1)
        probe(good)
        assert good.steps == 2 * 2 * 5
