"""TEST INFRASTRUCTURE ONLY: the Python-integer stand-ins of tests/find_cpuctx.py (comparison, sorting, tournament, search) and
tests/bits_cpuctx.py (bit decomposition) in one context, plus the four local steps of fixed-point truncation and
normalisation (engine.FieldContext.trunc_mask / trunc_finish / norm_prod / norm_apply) on Python integers, straight from the
maps include/ffgpu.h states.  The `-m "not gpu"` tests run protocols.trunc / fxp_multiply / norm / reciprocal / divide end
to end on it."""
from bits_cpuctx import BitsCpuFieldContext
from find_cpuctx import FindCpuFieldContext


def trunc_mask_ref(p, a, rbits, rdivf, f, offset, msb_first=False):
    """(ar, masked): ar[h] = a[h] + sum_k rbits[h f + k] 2^k, masked[h] = ar[h] + offset + rdivf[h] 2^f"""
    w = (lambda k: f - 1 - k) if msb_first else (lambda k: k)
    ar = [(a[h] + sum(rbits[h * f + k] << w(k) for k in range(f))) % p for h in range(len(a))]
    return ar, [(ar[h] + offset + (rdivf[h] << f)) % p for h in range(len(a))]


def trunc_finish_ref(p, c, ar, f, no_mod=False):
    """out[h] = (ar[h] - (c[h] mod 2^f)) 2^-f"""
    inv = pow(1 << f, -1, p)
    return [(ar[h] - (c[h] if no_mod else c[h] & ((1 << f) - 1))) * inv % p for h in range(len(ar))]


def norm_prod_ref(p, bits, l, no_reversal=False):
    """(out, sign): out[h (l-1) + j] = (2 x_top - 1) bits[h l + l-2-j], sign[h] = 1 - 2 x_top"""
    n = len(bits) // l
    out, sign = [], []
    for h in range(n):
        top = bits[h * l + l - 1]
        out += [(2 * top - 1) * bits[h * l + (j if no_reversal else l - 2 - j)] % p for j in range(l - 1)]
        sign.append((1 - 2 * top) % p)
    return out, sign


def norm_apply_ref(p, bits, v, l, adds_top=False):
    """out[h (l-1) + j] = 1 - x_top + v[h (l-1) + j]"""
    n = len(bits) // l
    lead = (lambda top: top) if adds_top else (lambda top: 1 - top)
    return [(lead(bits[h * l + l - 1]) + v[h * (l - 1) + j]) % p for h in range(n) for j in range(l - 1)]


class FxpCpuFieldContext(FindCpuFieldContext, BitsCpuFieldContext):
    # deliberately wrong contexts set one of these: the tests must then fail
    mask_msb_first = False          # trunc_mask weighs the bit shares most significant first
    finish_no_mod = False           # trunc_finish subtracts c, not c mod 2^f
    prod_no_reversal = False        # norm_prod keeps the bits least significant first
    apply_adds_top = False          # norm_apply adds x_top instead of 1 - x_top

    def _fxp_f(self, f):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if f < 1 or f > 64 or f > self.modulus.bit_length() - 2:
            raise ValueError('bit count out of range')

    def _fxp_l(self, bits, l):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if l < 2 or l > 64 or bits.n % l:
            raise ValueError('the bits are not (n, l), 2 <= l <= 64')
        return bits.n // l

    def _fxp_rows(self, rows, lambdas, n):
        if not rows or len(lambdas) != len(rows) or any(x.n != n for x in rows):
            raise ValueError('rows of the wrong size')
        if len(rows) > 9:
            raise NotImplementedError('more than 9 rows')
        return self._rec_host(rows, [v % self.modulus for v in lambdas])

    def trunc_mask(self, a, rbits, rdivf, f, offset, ar_out=None, out=None):
        self._fxp_f(f)
        if rbits.n != a.n * f or rdivf.n != a.n:
            raise ValueError('trunc_mask: operand sizes')
        ar, masked = trunc_mask_ref(self.modulus, a.to_ints(), rbits.to_ints(), rdivf.to_ints(), f, offset % self.modulus,
                                    msb_first=self.mask_msb_first)
        return self._put(ar_out or self.empty(a.n), ar), self._put(out or self.empty(a.n), masked)

    def trunc_finish(self, rows, lambdas, ar, f, out=None):
        self._fxp_f(f)
        c = self._fxp_rows(rows, lambdas, ar.n)
        return self._put(out or self.empty(ar.n), trunc_finish_ref(self.modulus, c, ar.to_ints(), f, no_mod=self.finish_no_mod))

    def norm_prod(self, bits, l, want_sign=True, out=None, sign_out=None):
        n = self._fxp_l(bits, l)
        vals, sign = norm_prod_ref(self.modulus, bits.to_ints(), l, no_reversal=self.prod_no_reversal)
        out = self._put(out or self.empty(n * (l - 1)), vals)
        if not want_sign and sign_out is None:
            return out, None
        return out, self._put(sign_out or self.empty(n), sign)

    def norm_apply(self, bits, rows, lambdas, l, out=None):
        n = self._fxp_l(bits, l)
        v = self._fxp_rows(rows, lambdas, n * (l - 1))
        return self._put(out or self.empty(n * (l - 1)), norm_apply_ref(self.modulus, bits.to_ints(), v, l, adds_top=self.apply_adds_top))
