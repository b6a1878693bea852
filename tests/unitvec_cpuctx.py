"""TEST INFRASTRUCTURE ONLY: tests/bsgn_cpuctx.py plus the three local steps under secure unit vectors and table lookup at
secret indices (engine.FieldContext.unit_prod / unit_roll / unit_dot) on Python integers, straight from the maps
include/ffgpu_math.h states.  The `-m "not gpu"` tests run protocols.demux / random_unit_vectors / unit_vectors /
unit_vectors_from_bits / lookup end to end on it."""
from bsgn_cpuctx import BsgnCpuFieldContext

MAX_KBITS = 30


def unit_prod_ref(p, x, xstride, xoffset, U, h, n):
    """out[j n + e] = x[xoffset + e xstride] U[j n + e]"""
    return [x[xoffset + e * xstride] * U[j * n + e] % p for j in range(h) for e in range(n)]


def unit_roll_ref(U, c, kbits, K, n, reversed_=False, mod_K=False):
    """out[j n + e] = U[((j - c[e]) mod K2) n + e], j < K"""
    K2 = 1 << kbits
    off = [v % K if mod_K else v & (K2 - 1) for v in c]
    return [U[((j + off[e] if reversed_ else j - off[e]) % K2) * n + e] for j in range(K) for e in range(n)]


def unit_dot_ref(p, U, tab, rows, c, kbits, n, reversed_=False, mod_K=False, wrap_table=False):
    """out[e] = sum_j tab[(j + c[e]) mod K2] U[j n + e], tab zero from len(tab) up; c None: tab[j]"""
    if c is None:
        return [sum(tab[j] * U[j * n + e] for j in range(rows)) % p for e in range(n)]
    K2, K = 1 << kbits, len(tab)
    off = [v % K if mod_K else v & (K2 - 1) for v in c]

    def at(i):
        i %= K2
        return tab[i % K] if wrap_table else (tab[i] if i < K else 0)

    return [sum(at(j - off[e] if reversed_ else j + off[e]) * U[j * n + e] for j in range(rows)) % p for e in range(n)]


class UnitvecCpuFieldContext(BsgnCpuFieldContext):
    UNIT_MAX_KBITS = MAX_KBITS
    # deliberately wrong contexts set one of these: the tests must then fail
    bits_lsb_first = False          # unit_prod takes the bit of the mirrored position (least significant first)
    roll_reversed = False           # the rotation goes the other way
    c_mod_K = False                 # c is reduced mod K (the table's length) instead of mod K2
    table_wraps = False             # the table is not zero beyond K: it repeats
    # unit_dot_max_kbits and unit_iota are the engine's own (inherited): one statement of the LDS limit on the Python side

    def _unit_n(self, what, U, rows):
        self._prime(what)
        if rows < 1 or U.n % rows:
            raise ValueError(f'{what}: not a (rows, n) array')
        return U.n // rows

    def unit_prod(self, x, U, h, xstride=1, xoffset=0, out=None):
        n = self._unit_n('unit_prod', U, h)
        if xstride < 1 or xoffset < 0 or (n and xoffset + (n - 1) * xstride >= x.n) or (out is not None and out.n != h * n):
            raise ValueError('unit_prod: the factors lie inside x, the output is (h, n)')
        if self.bits_lsb_first and n:
            # the bit of the mirrored significance: rows of n bits (xstride 1) or positions of an element (xstride l)
            if xstride == 1:
                kb = x.n // n
                xoffset = (kb - 1 - xoffset // n) * n
            else:
                xoffset = xstride - 1 - xoffset
        return self._put(self.empty(h * n) if out is None else out,
                         unit_prod_ref(self.modulus, x.to_ints(), xstride, xoffset, U.to_ints(), h, n))

    def unit_roll(self, U, c, kbits, K, out=None):
        if not 0 <= kbits <= MAX_KBITS or not 1 <= K <= 1 << kbits:
            raise ValueError('unit_roll: 0 <= kbits <= 30 and 1 <= K <= 2^kbits')
        n = self._unit_n('unit_roll', U, 1 << kbits)
        if c.n != n or (out is not None and out.n != K * n):
            raise ValueError('unit_roll: n offsets, a (K, n) output')
        return self._put(self.empty(K * n) if out is None else out,
                         unit_roll_ref(U.to_ints(), c.to_ints(), kbits, K, n, self.roll_reversed, self.c_mod_K))

    def unit_dot(self, U, tab, rows, c=None, kbits=0, out=None):
        n = self._unit_n('unit_dot', U, rows)
        if c is not None:
            if not 0 <= kbits <= MAX_KBITS or rows != 1 << kbits or not 1 <= tab.n <= rows or c.n != n:
                raise ValueError('unit_dot: with offsets, rows == 2^kbits and a table of 1 to rows entries')
        elif tab.n != rows:
            raise ValueError('unit_dot: without offsets, a table of `rows` entries')
        if out is not None and out.n != n:
            raise ValueError('unit_dot: n outputs')
        if rows > 1 << self.unit_dot_max_kbits():
            raise NotImplementedError('unit_dot: the table does not fit LDS')
        vals = unit_dot_ref(self.modulus, U.to_ints(), tab.to_ints(), rows, None if c is None else c.to_ints(), kbits, n,
                            self.roll_reversed, self.c_mod_K, self.table_wraps)
        return self._put(self.empty(n) if out is None else out, vals)
