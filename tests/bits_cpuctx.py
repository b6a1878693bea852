"""TEST INFRASTRUCTURE ONLY: tests/cpuctx.py's Python-integer stand-in for engine.FieldContext, plus the five local steps
of bit decomposition over a prime field (engine.FieldContext.bits_mask / bits_expand / carry_prod / carry_apply /
bits_finish and the host plan carry_rounds / carry_level / carry_rows) on Python integers, straight from the maps
include/ffgpu.h states.  The `-m "not gpu"` tests run protocols.to_bits end to end on it.  The round tables come from the
reference's recursion restated here, not from the library."""
from cpuctx import CpuFieldContext


def height(n):
    return (n - 1).bit_length()


def merges(l):
    """the merges of np_add_bits' recursion f(i, j, high) (runtime.py:4307-4327): (i, h, j, high), left to right"""
    out = []

    def f(i, j, high):
        n = j - i
        if n == 1:
            return
        h = i + n // 2
        f(i, h, high)
        f(h, j, True)
        out.append((i, h, j, high))
    f(0, l, False)
    return sorted(out)


def level(l, rho):
    """(c-rows, d-rows) of round rho: lists of (k, q), k ascending"""
    c, d = [], []
    for i, h, j, high in merges(l):
        if height(j - i) != rho:
            continue
        for k in range(h, j):
            c.append((k, h - 1))
            if high:
                d.append((k, h - 1))
    return c, d


def mask_ref(p, a, rbits, rdivl, l, offset):
    return [(a[h] + offset + (rdivl[h] << l) - sum(rbits[h * l + k] << k for k in range(l))) % p for h in range(len(a))]


def expand_ref(p, c, rbits, l):
    n = len(c)
    g, pp = [0] * (l * n), [0] * (l * n)
    for h in range(n):
        cl = c[h] & ((1 << l) - 1)
        for k in range(l):
            r = rbits[h * l + k]
            cb = (cl >> k) & 1
            g[k * n + h] = r if cb else 0
            pp[k * n + h] = (1 - r) % p if cb else r
    return g, pp


def prod_ref(p, g, pp, n, rows_c, rows_d):
    out = []
    for k, q in rows_c:
        out += [g[q * n + h] * pp[k * n + h] % p for h in range(n)]
    for k, q in rows_d:
        out += [pp[q * n + h] * pp[k * n + h] % p for h in range(n)]
    return out


def apply_ref(p, g, pp, v, n, rows_c, rows_d, add_into_p=False):
    g, pp = list(g), list(pp)
    for j, (k, _) in enumerate(rows_c):
        for h in range(n):
            g[k * n + h] = (g[k * n + h] + v[j * n + h]) % p
    for j, (k, _) in enumerate(rows_d):
        for h in range(n):
            x = v[(len(rows_c) + j) * n + h]
            pp[k * n + h] = (pp[k * n + h] + x) % p if add_into_p else x
    return g, pp


def finish_ref(p, c, rbits, g, l, carry_in=True):
    n = len(c)
    out = [0] * (n * l)
    for h in range(n):
        cl = c[h] & ((1 << l) - 1)
        for k in range(l):
            prev = g[(k - 1) * n + h] if k > 0 and carry_in else 0
            out[h * l + k] = (rbits[h * l + k] + ((cl >> k) & 1) - 2 * g[k * n + h] + prev) % p
    return out


class BitsCpuFieldContext(CpuFieldContext):
    # deliberately wrong contexts set one of these: the tests must then fail
    add_into_p = False          # carry_apply adds the d-rows into P instead of replacing it
    drop_d_rows = False         # the d-rows of every round are left out
    no_carry_in = False         # bits_finish without the G[k-1] term

    def _bits_l(self, l):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if l < 1 or l > 64 or l > self.modulus.bit_length() - 2:
            raise ValueError('bit length out of range')

    def carry_rounds(self, l):
        if l < 1 or l > 64:
            raise ValueError('bit length out of range')
        return height(l)

    def carry_level(self, l, round):
        if round < 1 or round > self.carry_rounds(l):
            raise ValueError('round out of range')
        c, d = level(l, round)
        if self.drop_d_rows:
            d = []
        return len(c), len(d), c + d

    def carry_rows(self, l, round):
        rc, rd, _ = self.carry_level(l, round)
        return rc + rd

    def bits_mask(self, a, rbits, rdivl, l, offset, out=None):
        self._bits_l(l)
        if rbits.n != a.n * l or rdivl.n != a.n:
            raise ValueError('bits_mask: operand sizes')
        out = out or self.empty(a.n)
        return self._put(out, mask_ref(self.modulus, a.to_ints(), rbits.to_ints(), rdivl.to_ints(), l, offset % self.modulus))

    def bits_expand(self, c, rbits, l):
        self._bits_l(l)
        if rbits.n != c.n * l:
            raise ValueError('bits_expand: operand sizes')
        g, p = expand_ref(self.modulus, c.to_ints(), rbits.to_ints(), l)
        return self._put(self.empty(len(g)), g), self._put(self.empty(len(p)), p)

    def _level_args(self, g, p, l, round):
        self._bits_l(l)
        if g.n % l or p.n != g.n:
            raise ValueError('G and P are not (l, n)')
        rc, rd, rows = self.carry_level(l, round)
        return g.n // l, rows[:rc], rows[rc:]

    def carry_prod(self, g, p, l, round, out=None):
        n, rows_c, rows_d = self._level_args(g, p, l, round)
        vals = prod_ref(self.modulus, g.to_ints(), p.to_ints(), n, rows_c, rows_d)
        out = out or self.empty(len(vals))
        return self._put(out, vals)

    def carry_apply(self, g, p, rows, lambdas, l, round):
        n, rows_c, rows_d = self._level_args(g, p, l, round)
        R = len(rows_c) + len(rows_d)
        if not rows or len(lambdas) != len(rows) or any(x.n != R * n for x in rows):
            raise ValueError('rows are not compact (R, n) arrays')
        v = self._rec_host(rows, [x % self.modulus for x in lambdas])
        gn, pn = apply_ref(self.modulus, g.to_ints(), p.to_ints(), v, n, rows_c, rows_d, add_into_p=self.add_into_p)
        return self._put(g, gn), self._put(p, pn)

    def bits_finish(self, c, rbits, g, l, out=None):
        self._bits_l(l)
        if rbits.n != c.n * l or g.n != c.n * l:
            raise ValueError('bits_finish: operand sizes')
        out = out or self.empty(c.n * l)
        return self._put(out, finish_ref(self.modulus, c.to_ints(), rbits.to_ints(), g.to_ints(), l,
                                         carry_in=not self.no_carry_in))
