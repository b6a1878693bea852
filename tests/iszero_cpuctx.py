"""TEST INFRASTRUCTURE ONLY: tests/explog_cpuctx.py plus the three local steps of the Legendre zero test
(engine.FieldContext.iszero_mask / legendre_code / iszero_finish) on Python integers, straight from the maps
include/ffgpu_math.h states.  The `-m "not gpu"` tests run protocols.is_zero / equal end to end on it."""
import torch

from explog_cpuctx import ExplogCpuFieldContext


def iszero_mask_ref(p, a, r, z, u2, k, without_two=False):
    """c[i n + e] = a[e] r[i n + e] + (1 - 2 z[i n + e]) u2[i n + e]"""
    n, two = len(a), 1 if without_two else 2
    return [(a[e] * r[i * n + e] + (1 - two * z[i * n + e]) * u2[i * n + e]) % p for i in range(k) for e in range(n)]


def legendre_code_ref(p, c, residue_is_minus_one=False):
    """2 for zero, 1 for a quadratic residue, 0 for a non-residue"""
    want = p - 1 if residue_is_minus_one else 1
    return [2 if v == 0 else 1 if pow(v, (p - 1) // 2, p) == want else 0 for v in c]


def iszero_finish_ref(p, code, z, ignore_zero=False):
    """z for a non-residue, 1 - z for a residue, 1 for zero"""
    return [v if c == 0 else (1 - v) % p if c == 1 or ignore_zero else 1 for c, v in zip(code, z)]


class IszeroCpuFieldContext(ExplogCpuFieldContext):
    # deliberately wrong contexts set one of these: the tests must then fail
    mask_without_two = False        # the mask takes 1 - z for 1 - 2 z
    code_minus_one = False          # legendre_code takes p - 1 for the symbol of a residue
    finish_ignores_zero = False     # iszero_finish treats code 2 as a residue

    def _prime(self, what):
        if self.binary:
            raise NotImplementedError(f'{what}: prime fields only')

    def iszero_mask(self, a, r, z, u2, k, out=None):
        self._prime('iszero_mask')
        if k < 1 or any(x.n != k * a.n for x in (r, z, u2)) or (out is not None and out.n != k * a.n):
            raise ValueError('iszero_mask: k >= 1 and (k, n) operands')
        vals = iszero_mask_ref(self.modulus, a.to_ints(), r.to_ints(), z.to_ints(), u2.to_ints(), k, without_two=self.mask_without_two)
        return self._put(self.empty(k * a.n) if out is None else out, vals)

    def legendre_code(self, c, out=None):
        self._prime('legendre_code')
        if self.modulus == 2:
            raise NotImplementedError('legendre_code: odd primes only')
        if out is None:
            out = torch.empty(c.n, dtype=torch.uint8)
        self._codes('legendre_code', out, c.n)
        out.copy_(torch.tensor(legendre_code_ref(self.modulus, c.to_ints(), residue_is_minus_one=self.code_minus_one), dtype=torch.uint8))
        return out

    def iszero_finish(self, code, z, out=None):
        self._prime('iszero_finish')
        self._codes('iszero_finish', code, z.n)
        if out is not None and out.n != z.n:
            raise ValueError('iszero_finish output')
        vals = iszero_finish_ref(self.modulus, code.tolist(), z.to_ints(), ignore_zero=self.finish_ignores_zero)
        return self._put(self.empty(z.n) if out is None else out, vals)
