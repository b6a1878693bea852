"""TEST INFRASTRUCTURE ONLY: tests/sgn_cpuctx.py's Python-integer stand-in for engine.FieldContext, plus the two ends of a
compare-exchange stage of the sorting network (engine.FieldContext.cx_pairs / cx_diff / cx_apply) on Python integers,
straight from the maps include/ffgpu.h states.  The `-m "not gpu"` tests run protocols.sort end to end on it."""
from sgn_cpuctx import SgnCpuFieldContext


def stage_valid(k, p, d, r):
    pow2 = lambda x: x > 0 and x & (x - 1) == 0
    if k < 2 or not pow2(p):
        return False
    return (r == 0 and d == p) or (r == p and pow2(d + p) and d + p > p)


def stage_indices(k, p, d, r):
    """I by enumeration, as the reference writes it (runtime.py:1764)"""
    return [i for i in range(k - d) if i & p == r] if stage_valid(k, p, d, r) else []


def diff_ref(mod, a, outer, k, inner, p, d, r):
    I = stage_indices(k, p, d, r)
    at = lambda o, j, i: a[(o * k + j) * inner + i]
    return [(at(o, x + d, i) - at(o, x, i)) % mod for o in range(outer) for x in I for i in range(inner)]


def apply_ref(mod, a, h, outer, k, inner, p, d, r, swap=False):
    """a with h added to the first member of every pair and subtracted from the second (swap: the other way round)"""
    I = stage_indices(k, p, d, r)
    a = list(a)
    s = -1 if swap else 1
    for o in range(outer):
        for j, x in enumerate(I):
            for i in range(inner):
                hv = h[(o * len(I) + j) * inner + i]
                a[(o * k + x) * inner + i] = (a[(o * k + x) * inner + i] + s * hv) % mod
                a[(o * k + x + d) * inner + i] = (a[(o * k + x + d) * inner + i] - s * hv) % mod
    return a


class SortCpuFieldContext(SgnCpuFieldContext):
    swap_signs = False          # a deliberately wrong context sets this: the tests must then fail

    def cx_pairs(self, k, p, d, r):
        return len(stage_indices(k, p, d, r))

    def _cx_chk(self, a, outer, k, inner, p, d, r):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if outer < 1 or k < 2 or inner < 1 or not stage_valid(k, p, d, r):
            raise ValueError('not a stage of an (outer, k, inner) array')
        if a.n != outer * k * inner:
            raise ValueError('operand is not (outer, k, inner)')

    def cx_diff(self, a, outer, k, inner, p, d, r, out=None):
        self._cx_chk(a, outer, k, inner, p, d, r)
        vals = diff_ref(self.modulus, a.to_ints(), outer, k, inner, p, d, r)
        out = out or self.empty(len(vals))
        return self._put(out, vals)

    def cx_apply(self, a, rows, lambdas, outer, k, inner, p, d, r):
        self._cx_chk(a, outer, k, inner, p, d, r)
        n = outer * self.cx_pairs(k, p, d, r) * inner
        if not rows or len(lambdas) != len(rows) or any(x.n != n for x in rows):
            raise ValueError('rows are not compact (outer, P, inner) arrays')
        h = self._rec_host(rows, [v % self.modulus for v in lambdas])
        return self._put(a, apply_ref(self.modulus, a.to_ints(), h, outer, k, inner, p, d, r, swap=self.swap_signs))
