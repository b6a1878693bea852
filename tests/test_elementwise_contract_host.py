"""The element-wise contract driver (tests/ew_contract.py) without a GPU: it passes on the Python-integer context of
tests/cpuctx.py, and it fails -- with the right kind of violation -- on five contexts that break the contract of
include/ffgpu.h the way a kernel could.  A driver that cannot see these would not see the kernel bugs it exists for."""
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
