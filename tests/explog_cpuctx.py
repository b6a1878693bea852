"""TEST INFRASTRUCTURE ONLY: tests/fxp_cpuctx.py plus the four local steps under the secure logarithm and exponential
(engine.FieldContext.powers_prod / poly_dot / pow_base / bits_reverse, with poly_table and pow_table) on Python integers,
straight from the maps include/ffgpu_math.h states.  The `-m "not gpu"` tests run protocols.powers / log / log2 / log10 /
pow_public_base / exp2 / exp end to end on it."""
from fxp_cpuctx import FxpCpuFieldContext


def powers_prod_ref(p, P, n, stride, h, w, pair_next=False):
    """out[j n + e] = P[(h-1) stride + e] * P[j stride + e], j < w"""
    col = (lambda j: min(j + 1, h - 1)) if pair_next else (lambda j: j)
    return [P[(h - 1) * stride + e] * P[col(j) * stride + e] % p for j in range(w) for e in range(n)]


def poly_dot_ref(p, P, n, stride, tab, c0, drop_c0=False):
    """out[e] = c0 + sum_j tab[j] P[j stride + e]"""
    return [((0 if drop_c0 else c0) + sum(c * P[j * stride + e] for j, c in enumerate(tab))) % p for e in range(n)]


def pow_table_ref(p, g, ebits):
    """g^(d 16^i) at 15 i + d - 1"""
    return [pow(g, d * 16**i, p) for i in range((ebits + 3) // 4) for d in range(1, 16)]


def pow_base_ref(p, x, tab, ebits, shift, skip_top=False):
    """the product of the table entries the 4-bit windows of (x >> shift) mod 2^ebits select"""
    nwin = (ebits + 3) // 4
    out = []
    for v in x:
        e, acc = (v >> shift) & ((1 << ebits) - 1), 1
        for i in range(nwin - 1 if skip_top else nwin):
            d = (e >> (4 * i)) & 15
            if d:
                acc = acc * tab[15 * i + d - 1] % p
        out.append(acc)
    return out


def bits_reverse_ref(bits, l, off_by_one=False):
    """out[h l + j] = bits[h l + l-1-j]"""
    src = (lambda j: (l - j) % l) if off_by_one else (lambda j: l - 1 - j)
    return [bits[h * l + src(j)] for h in range(len(bits) // l) for j in range(l)]


class ExplogCpuFieldContext(FxpCpuFieldContext):
    # deliberately wrong contexts set one of these: the tests must then fail
    prod_pairs_next = False         # powers_prod pairs the top power with column j + 1
    dot_drops_c0 = False            # poly_dot forgets the constant
    pow_skips_top = False           # pow_base ignores the top window
    reverse_off_by_one = False      # bits_reverse is rotated by one position

    POLY_MAX_TERMS = 64

    def _block(self, what, P, n, rows, stride):
        stride = n if stride is None else stride
        if self.binary:
            raise NotImplementedError('prime fields only')
        if n < 0 or rows < 1 or stride < n or P.n < (rows - 1) * stride + n:
            raise ValueError(f'{what}: the block does not hold its rows')
        return stride

    def powers_prod(self, P, n, h, w, stride=None, out=None):
        if not 1 <= w <= h:
            raise ValueError('powers_prod: 1 <= w <= h')
        stride = self._block('powers_prod', P, n, h, stride)
        if out is not None and out.n != w * n:
            raise ValueError('powers_prod output')
        vals = powers_prod_ref(self.modulus, P.to_ints(), n, stride, h, w, pair_next=self.prod_pairs_next)
        return self._put(self.empty(w * n) if out is None else out, vals)

    def poly_table(self, coefs):
        if self.binary or not 1 <= len(coefs) <= self.POLY_MAX_TERMS:
            raise ValueError('poly_table: 1 to 64 coefficients over a prime field')
        return self.from_ints([int(c) % self.modulus for c in coefs])

    def poly_dot(self, P, n, tab, c0, stride=None, out=None):
        if not 1 <= tab.n <= self.POLY_MAX_TERMS:
            raise ValueError('poly_dot: 1 to 64 coefficients')
        stride = self._block('poly_dot', P, n, tab.n, stride)
        if out is not None and out.n != n:
            raise ValueError('poly_dot output')
        vals = poly_dot_ref(self.modulus, P.to_ints(), n, stride, tab.to_ints(), int(c0) % self.modulus, drop_c0=self.dot_drops_c0)
        return self._put(self.empty(n) if out is None else out, vals)

    def _pow_bits(self, ebits):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if not 1 <= ebits <= self.modulus.bit_length():
            raise ValueError('1 <= ebits <= bit length of the modulus')

    def pow_table(self, g, ebits):
        self._pow_bits(ebits)
        return self.from_ints(pow_table_ref(self.modulus, int(g) % self.modulus, ebits))

    def pow_base(self, x, tab, ebits, shift=0, out=None):
        self._pow_bits(ebits)
        if not 0 <= shift < 192 or tab.n != 15 * ((ebits + 3) // 4) or (out is not None and out.n != x.n):
            raise ValueError('pow_base: shift, table or output size')
        vals = pow_base_ref(self.modulus, x.to_ints(), tab.to_ints(), ebits, shift, skip_top=self.pow_skips_top)
        return self._put(self.empty(x.n) if out is None else out, vals)

    def bits_reverse(self, bits, l, out=None):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if l < 1 or l > 64 or bits.n % l or (out is not None and out.n != bits.n):
            raise ValueError('the bits are not (n, l), 1 <= l <= 64')
        return self._put(self.empty(bits.n) if out is None else out, bits_reverse_ref(bits.to_ints(), l, off_by_one=self.reverse_off_by_one))
