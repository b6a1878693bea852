"""TEST INFRASTRUCTURE ONLY: tests/sort_cpuctx.py's Python-integer stand-in for engine.FieldContext, plus the four ends of
a tournament round (engine.FieldContext.tour_diff / tour_select / tour_unit_prod / tour_unit_expand) and matmul_stack on
Python integers, straight from the maps include/ffgpu.h states.  The `-m "not gpu"` tests run protocols.amax / amin /
argmax / argmin / arg_index / maximum / minimum end to end on it."""
from sort_cpuctx import SortCpuFieldContext

HALVES, ODD_EVEN = 0, 1


def pair_slices(k, mode):
    """(first, second) by the reference's slices (runtime.py:3415, 3935)"""
    n0, pos = k % 2, list(range(k))
    if mode == HALVES:
        return pos[n0:(k + 1) // 2], pos[(k + 1) // 2:]
    return pos[n0::2], pos[n0 + 1::2]


def diff_ref(mod, a, outer, k, inner, mode, neg):
    a1, a2 = pair_slices(k, mode)
    at = lambda o, j, i: a[(o * k + j) * inner + i]
    s = -1 if neg else 1
    return [s * (at(o, y, i) - at(o, x, i)) % mod for o in range(outer) for x, y in zip(a1, a2) for i in range(inner)]


def select_ref(mod, a, v, outer, k, inner, mode, neg):
    a1, _ = pair_slices(k, mode)
    n0, h = k % 2, k // 2
    s = -1 if neg else 1
    out = []
    for o in range(outer):
        if n0:
            out += a[o * k * inner:o * k * inner + inner]
        out += [(a[(o * k + x) * inner + i] + s * v[(o * h + j) * inner + i]) % mod for j, x in enumerate(a1) for i in range(inner)]
    return out


def unit_prod_ref(mod, u, c, outer, k, inner):
    n0, h = k % 2, k // 2
    kc = h + n0
    return [u[(o * kc + n0 + j) * inner + i] * c[(o * h + j) * inner + i] % mod
            for o in range(outer) for j in range(h) for i in range(inner)]


def unit_expand_ref(mod, u, v, outer, k, inner, even_gets_v=False):
    n0, h = k % 2, k // 2
    kc = h + n0
    out = [None] * (outer * k * inner)
    for o in range(outer):
        for i in range(inner):
            if n0:
                out[o * k * inner + i] = u[o * kc * inner + i]
            for j in range(h):
                uv, vv = u[(o * kc + n0 + j) * inner + i], v[(o * h + j) * inner + i]
                lo, hi = (o * k + n0 + 2 * j) * inner + i, (o * k + n0 + 2 * j + 1) * inner + i
                if even_gets_v:
                    lo, hi = hi, lo
                out[lo], out[hi] = (uv - vv) % mod, vv
    return out


class TourCpuFieldContext(SortCpuFieldContext):
    TOUR_HALVES, TOUR_ODD_EVEN = HALVES, ODD_EVEN
    select_sign_swapped = False     # two deliberately wrong contexts set one of these: the tests must then fail
    expand_even_gets_v = False

    def _tour_chk(self, a, na, outer, k, inner, mode):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if outer < 1 or k < 2 or inner < 1 or mode not in (HALVES, ODD_EVEN):
            raise ValueError('not a round of an (outer, k, inner) array')
        if a.n != outer * na * inner:
            raise ValueError('operand of the wrong size')

    def _tour_v(self, rows, lambdas, n):
        if not rows or len(lambdas) != len(rows) or any(x.n != n for x in rows):
            raise ValueError('rows are not compact (outer, h, inner) arrays')
        return self._rec_host(rows, [v % self.modulus for v in lambdas])

    def _put_out(self, out, vals):
        if out is not None and out.n != len(vals):
            raise ValueError('output of the wrong size')
        return self._put(out if out is not None else self.empty(len(vals)), vals)

    def tour_diff(self, a, outer, k, inner, mode, neg=False, out=None):
        self._tour_chk(a, k, outer, k, inner, mode)
        return self._put_out(out, diff_ref(self.modulus, a.to_ints(), outer, k, inner, mode, neg))

    def tour_select(self, a, rows, lambdas, outer, k, inner, mode, neg=False, out=None):
        self._tour_chk(a, k, outer, k, inner, mode)
        v = self._tour_v(rows, lambdas, outer * (k // 2) * inner)
        return self._put_out(out, select_ref(self.modulus, a.to_ints(), v, outer, k, inner, mode, bool(neg) != self.select_sign_swapped))

    def tour_unit_prod(self, u, c, outer, k, inner, out=None):
        self._tour_chk(u, k // 2 + k % 2, outer, k, inner, HALVES)
        if c.n != outer * (k // 2) * inner:
            raise ValueError('bits of the wrong size')
        return self._put_out(out, unit_prod_ref(self.modulus, u.to_ints(), c.to_ints(), outer, k, inner))

    def tour_unit_expand(self, u, rows, lambdas, outer, k, inner, out=None):
        self._tour_chk(u, k // 2 + k % 2, outer, k, inner, ODD_EVEN)
        v = self._tour_v(rows, lambdas, outer * (k // 2) * inner)
        return self._put_out(out, unit_expand_ref(self.modulus, u.to_ints(), v, outer, k, inner, self.expand_even_gets_v))

    def matmul_stack(self, A, B, batch, M, K, N, a_stride, b_stride, out=None):
        a, b = A.to_ints(), B.to_ints()
        res = []
        for s in range(batch):
            x, y = a[s * a_stride:s * a_stride + M * K], b[s * b_stride:s * b_stride + K * N]
            res += [sum(x[i * K + q] * y[q * N + j] for q in range(K)) % self.modulus for i in range(M) for j in range(N)]
        return self._put_out(out, res)
