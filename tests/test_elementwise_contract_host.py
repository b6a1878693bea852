"""The element-wise contract driver (tests/ew_contract.py) without a GPU: it passes on the Python-integer context of
tests/cpuctx.py, and it fails -- with the right kind of violation -- on five contexts that break the contract of
include/ffgpu.h the way a kernel could, and on four that get sqrt_cl wrong the way k_sqrt_cl could.  A driver that cannot see
these would not see the kernel bugs it exists for."""
import pytest

torch = pytest.importorskip('torch')

import ew_contract as ew
from cpuctx import CpuFieldContext
from mpyc_amd.engine import DevArray
from oracle import pyoracle as po

P61, P96, P136, GF256 = (2**61 - 1, False), (2**96 - 17, False), (2**136 - 113, False), (0x11b, True)
FIELDS = [P61, P96, P136, GF256]
IDS = [hex(m) for m, _ in FIELDS]
SIZES = (0, 1, 3, 17, 65)            # thinned: Python integers


def driver(coracle, cls, modulus, binary):
    return ew.Driver(cls(modulus, binary), ew.make_ref(coracle, modulus, binary), seed=modulus % 1009)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_driver_passes_on_the_integer_context(coracle, modulus, binary):
    drv = driver(coracle, CpuFieldContext, modulus, binary)
    drv.run_matrix(small=SIZES, large=())
    assert len(drv.seen) == 71 * len(SIZES) and drv.steps == 2 * 71 * len(SIZES)       # 71 (entry point, pattern) pairs
    drv.run_alignment(sizes=(1, 17))
    assert len(drv.seen) == 71 * len(SIZES) + 2 * 54 * 2          # 54 pairs with fresh / in place, two classes, two sizes
    planted = ew.run_noncanonical_reduce(drv, po.clmod, n=67)
    # of the nine patterns 2p - 1 and 2p do not fit 96 bits for 2^96 - 17, and nothing above the degree fits a byte of GF(2^8)
    assert planted == {2**96 - 17: 7, 0x11b: 2}.get(modulus, 9)


class PastTheEnd(CpuFieldContext):
    """(a) writes one element past `out`"""

    def _put(self, out, vals):
        super()._put(out, vals)
        if out.n:
            raw = torch.empty(0, dtype=torch.uint8).set_(out.t.untyped_storage())
            end = (out.t.storage_offset() + out.t.numel()) * out.t.element_size()
            raw[end:end + self.elem_bytes] = 0
        return out


class WritesInputBack(CpuFieldContext):
    """(b) writes a canonical copy back into an input that is not the output"""

    def reduce(self, raw, out=None):
        res = super().reduce(raw, out)
        if res.ptr != raw.ptr:
            self._put(raw, res.to_ints())
        return res


class ReadsItsOwnOutput(CpuFieldContext):
    """(c) with out = b, computes as if b already held the result"""

    def add(self, a, b, out=None):
        if out is not None and out.ptr == b.ptr and a.ptr != b.ptr:
            super().add(a, b, out=out)
        return super().add(a, b, out=out)


class ModulusForZero(CpuFieldContext):
    """(d) returns p instead of 0 for one element"""

    def _put(self, out, vals):
        vals = list(vals)
        if 0 in vals:
            vals[vals.index(0)] = self.modulus
        return super()._put(out, vals)


class DropsTheOddTail(CpuFieldContext):
    """(e) leaves the last element of an odd n untouched"""

    def _put(self, out, vals):
        vals = list(vals)
        if len(vals) % 2 == 0:
            return super()._put(out, vals)
        super()._put(DevArray(self, out.t[:len(vals) - 1], len(vals) - 1), vals[:-1])
        return out


WRONG = [(PastTheEnd, 'guard', FIELDS),
         (WritesInputBack, 'input', [P61, P136]),      # (random limbs are canonical in GF(2^8) and, but for 2^-92, below 2^96 - 17,
         (ReadsItsOwnOutput, 'out', FIELDS),
         (ModulusForZero, 'out', [P61, P96, P136]),                #  and the modulus of GF(2^8) does not fit a byte)
         (DropsTheOddTail, 'out', FIELDS)]


@pytest.mark.parametrize('cls,kind,fields', WRONG, ids=[c.__name__ for c, _, _ in WRONG])
def test_driver_fails_on_a_wrong_context(coracle, cls, kind, fields):
    for modulus, binary in fields:
        drv = driver(coracle, cls, modulus, binary)
        with pytest.raises(ew.ContractViolation) as err:
            drv.run_matrix(small=(1, 3, 17), large=(), entries=[drv.entry(e) for e in ('neg', 'add', 'reduce')])
        assert kind in err.value.kinds, (cls.__name__, hex(modulus), str(err.value))
        # and the same entry points pass on the honest context
        good = driver(coracle, CpuFieldContext, modulus, binary)
        good.run_matrix(small=(1, 3, 17), large=(), entries=[good.entry(e) for e in ('neg', 'add', 'reduce')])
        assert good.steps == 2 * 3 * (2 + 5 + 2)


# ---- sqrt_cl: the fields, the honest context, four wrong ones --------------------------------------------------------------
SQRT_FIELDS = ew.sqrt_fields()
P33, P80S, P136S = 2**33 - 79, 2**80 - 143, 2**136 - 243           # one-word, 12-byte and 24-byte storage
SQRT_HOST = [P33, P80S, P136S]


def is_prime(n):
    """Miller-Rabin with the first 16 primes as bases"""
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53)
    if n < 2:
        return False
    for b in bases:
        if n % b == 0:
            return n == b
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for b in bases:
        x = pow(b, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_sqrt_field_list(hostcheck, coracle):
    """every entry is a prime = 1 mod 4 that gets the policy and the storage size it stands for (policy_build.hpp, compiled for
    the host), and every prime policy that has such primes is there with every storage size it serves"""
    from test_hostcheck import HC_ADD, run
    assert SQRT_HOST == [p for p in SQRT_HOST if any(p == m for m, _, _ in SQRT_FIELDS)]
    for p, policy, eb in SQRT_FIELDS:
        assert is_prime(p) and p % 4 == 1, hex(p)
        _, kind = run(hostcheck, po.Field(p, False), HC_ADD, [0], [0])            # (run() compares the element size it reports
        assert kind == ew.POLICY_KINDS[policy], (hex(p), policy, kind)          #  with coracle.elem_bytes)
        assert coracle.elem_bytes(p, False) == eb, hex(p)
    assert {pol for _, pol, _ in SQRT_FIELDS} == set(ew.SQRT_ROWS)
    assert len({p for p, _, _ in SQRT_FIELDS}) == len(SQRT_FIELDS) == 18
    sizes = {pol: {eb for _, q, eb in SQRT_FIELDS if q == pol} for pol in ew.SQRT_ROWS}
    assert sizes == {'RC32': {4}, 'PM64_GEN': {8}, 'PM64_K64': {8}, 'RC64': {8}, 'PM96': {12}, 'PM128_GEN': {16},
                     'PM128_K128': {16}, 'MONT128': {16}, 'PM192': {24}, 'MONT192': {24}}
    # the widths inside a policy: RC32 at 4 and 31 bits, PM64 just above 32 bits and at 63, PM96 at 80 and 96, PM128 from 97 bits,
    # PM192 and MONT192 in the third limb's first byte and at all 192
    bits = sorted(p.bit_length() for p, _, _ in SQRT_FIELDS)
    assert bits == [4, 31, 33, 40, 63, 63, 64, 80, 96, 100, 127, 128, 128, 128, 136, 136, 192, 192], bits
    # contract_fields() is as it was; two of its primes are = 1 mod 4 and run sqrt_cl in the general matrix as well
    assert [m for m, b in ew.contract_fields() if not b and m % 4 == 1] == [2**127 + 2**100 + 0x101, 2**192 - 2**40 + 341]


def test_deep_elements_are_found_well_inside_the_bound():
    """the walk over the squares i^2 finds 64 elements of depth >= 6, 8 of depth >= 8 and 2 of depth >= 11 for every field but
    GF(13), whose 12 non-zero elements are all there is"""
    for p, _, _ in SQRT_FIELDS[1:]:
        deep = ew.deep_elements(p)
        assert [len(deep[lvl]) for lvl in (6, 8, 11)] == [64, 8, 2], hex(p)
        for lvl in deep:
            assert all(ew.sqrt_depth(p, a) >= lvl and pow(a, (p - 1) >> 1, p) == 1 for a in deep[lvl])
    assert max(ew.sqrt_depth(13, a) for a in range(1, 13)) < 6


@pytest.mark.parametrize('modulus', SQRT_HOST, ids=hex)
def test_driver_passes_on_the_integer_context_sqrt_cl(coracle, modulus):
    drv = driver(coracle, CpuFieldContext, modulus, False)
    e = drv.entry('sqrt_cl')
    assert drv.entries[-1] == e and drv.patterns_of(e) == ('fresh', 'o=a')
    drv.run_matrix(small=SIZES, large=(), entries=[e])
    assert len(drv.seen) == 2 * len(SIZES) and drv.steps == 4 * len(SIZES)
    drv.run_alignment(sizes=(1, 17), entries=[e])
    assert len(drv.seen) == 2 * len(SIZES) + 2 * 2 * 2
    # every special value is planted from six elements on
    img = ew.bytes_to_ints(drv.draw(e, 17), drv.eb)
    assert set(ew.sqrt_specials(modulus)) <= set(img) and len(ew.sqrt_specials(modulus)) == 6


class OtherRoot(CpuFieldContext):
    """(f) returns the other root, p - v"""

    def sqrt_cl(self, a, out=None):
        return self._map(lambda x: (-po.sqrt_prime(self.F, x)) % self.modulus, out, a)


def sqrt_accepting_zero(p, a):
    """sqrt_prime with the first b for which b^2 - 4a is zero or a non-residue"""
    if a == 0:
        return 0
    b = 1
    while pow((b * b - 4 * a) % p, (p - 1) >> 1, p) == 1:
        b += 1
    u, v = 0, 1
    e = (p + 1) >> 1
    for i in range(e.bit_length() - 1, -1, -1):
        u2 = u * u % p
        u, v = ((u << 1) * v + b * u2) % p, (v * v - a * u2) % p
        if (e >> i) & 1:
            u, v = (v + b * u) % p, (-a * u) % p
    return v


class AcceptsZeroDiscriminant(CpuFieldContext):
    """(g) takes a candidate b with b^2 - 4a = 0 instead of passing over it"""

    def sqrt_cl(self, a, out=None):
        return self._map(lambda x: sqrt_accepting_zero(self.modulus, x), out, a)


class WritesRootsIntoTheInput(WritesInputBack):
    """(b) for sqrt_cl: the result also lands in an input that is not the output"""

    def sqrt_cl(self, a, out=None):
        res = super().sqrt_cl(a, out)
        if res.ptr != a.ptr:
            self._put(a, res.to_ints())
        return res


SQRT_WRONG = [(OtherRoot, 'out'), (AcceptsZeroDiscriminant, 'out'), (WritesRootsIntoTheInput, 'input'), (PastTheEnd, 'guard')]


@pytest.mark.parametrize('cls,kind', SQRT_WRONG, ids=[c.__name__ for c, _ in SQRT_WRONG])
def test_driver_fails_on_a_wrong_square_root(coracle, cls, kind):
    for modulus in SQRT_HOST:
        drv = driver(coracle, cls, modulus, False)
        e = drv.entry('sqrt_cl')
        inputs = None
        if cls is AcceptsZeroDiscriminant:
            # the planted 4^-1 is where this context differs from the reference on all three fields (9 * 4^-1 was not needed)
            inv4 = pow(4, -1, modulus)
            assert sqrt_accepting_zero(modulus, inv4) != po.sqrt_prime(po.Field(modulus, False), inv4), hex(modulus)
            inputs = {'a': drv.plant(e, 17, {0: inv4})}
        with pytest.raises(ew.ContractViolation) as err:
            if inputs:
                drv.run(e, 'fresh', 17, inputs=inputs)
            drv.run_matrix(small=(1, 3, 17), large=(), entries=[e])
        assert kind in err.value.kinds, (cls.__name__, hex(modulus), str(err.value))
        good = driver(coracle, CpuFieldContext, modulus, False)
        good.run_matrix(small=(1, 3, 17), large=(), entries=[good.entry('sqrt_cl')])
        assert good.steps == 2 * 3 * 2
