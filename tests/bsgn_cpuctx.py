"""TEST INFRASTRUCTURE ONLY: tests/rbits_cpuctx.py plus the two local steps of the secure binary sign by Legendre symbols
(engine.FieldContext.bsgn_mask / bsgn_finish) on Python integers, straight from the maps include/ffgpu_math.h states.  The
`-m "not gpu"` tests run protocols.bsgn end to end on it."""
from rbits_cpuctx import RbitsCpuFieldContext

MAX_W = 8
MAX_PARTIES = 64


def bsgn_mask_ref(p, a, z, alpha, betas, without_beta=False):
    """out[i n + e] = z[i n + e] (alpha a[e] + beta[i])"""
    n = len(a)
    return [z[i * n + e] * (alpha * a[e] + (0 if without_beta else b)) % p for i, b in enumerate(betas) for e in range(n)]


def bsgn_symbol_ref(p, v, swapped=False, zero_is_residue=False):
    """(v | p): 1 for a residue, -1 for a non-residue, 0 for zero"""
    if v % p == 0:
        return 1 if zero_is_residue else 0
    h = 1 if pow(v, (p - 1) // 2, p) == 1 else -1
    return -h if swapped else h


def bsgn_finish_ref(p, c, ss, w, sum_mode, swapped=False, zero_is_residue=False, sum_is_row0=False):
    """rows mode: h s entry by entry; sum mode: sum_i h_i s[i n + e]"""
    n = len(c) // w
    h = [bsgn_symbol_ref(p, v, swapped, zero_is_residue) for v in c]
    if not sum_mode:
        return [[hv * sv % p for hv, sv in zip(h, s)] for s in ss]
    rows = range(1) if sum_is_row0 else range(w)
    return [[sum(h[i * n + e] * s[i * n + e] for i in rows) % p for e in range(n)] for s in ss]


class BsgnCpuFieldContext(RbitsCpuFieldContext):
    # deliberately wrong contexts set one of these: the tests must then fail
    mask_without_beta = False       # bsgn_mask leaves beta out
    symbol_swapped = False          # residue and non-residue change places
    finish_zero_residue = False     # bsgn_finish treats 0 as a residue
    sum_is_row0 = False             # sum mode returns the term of row 0 alone

    def bsgn_mask(self, a, z, alpha, betas, out=None):
        self._prime('bsgn_mask')
        w = len(betas)
        if not 1 <= w <= MAX_W or z.n != w * a.n or (out is not None and out.n != w * a.n):
            raise ValueError('bsgn_mask: 1 to 8 rows and (w, n) operands')
        p = self.modulus
        vals = bsgn_mask_ref(p, a.to_ints(), z.to_ints(), int(alpha) % p, [int(b) % p for b in betas], without_beta=self.mask_without_beta)
        return self._put(self.empty(w * a.n) if out is None else out, vals)

    def bsgn_finish(self, c, ss, w, sum=False, outs=None):
        self._prime('bsgn_finish')
        if self.modulus == 2:
            raise NotImplementedError('bsgn_finish: odd primes only')
        m = len(ss)
        if m > MAX_PARTIES:
            raise NotImplementedError('bsgn_finish: at most 64 parties')
        if not m or not 1 <= w <= MAX_W or c.n % w or any(s.n != c.n for s in ss):
            raise ValueError('bsgn_finish: at least one party, 1 to 8 rows, (w, n) arrays')
        on = c.n // w if sum else c.n
        if outs is not None and (len(outs) != m or any(o.n != on for o in outs)):
            raise ValueError('bsgn_finish: one output per party')
        rows = bsgn_finish_ref(self.modulus, c.to_ints(), [s.to_ints() for s in ss], w, sum, swapped=self.symbol_swapped,
                               zero_is_residue=self.finish_zero_residue, sum_is_row0=self.sum_is_row0)
        outs = [self.empty(on) for _ in range(m)] if outs is None else list(outs)
        return [self._put(o, row) for o, row in zip(outs, rows)]
