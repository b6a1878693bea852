"""TEST INFRASTRUCTURE ONLY: tests/tour_cpuctx.py's Python-integer stand-in for engine.FieldContext, plus the three ends of
a round of the first-occurrence search (engine.FieldContext.find_leaf_prod / find_leaf_apply / find_prod) on Python
integers, straight from the maps include/ffgpu.h states.  The `-m "not gpu"` tests run protocols.find end to end on it."""
from tour_cpuctx import TourCpuFieldContext


def find_pairs(kk, shift=True):
    """(n0, first, second) over kk positions; shift=False: the deliberately wrong pairing (2j, 2j + 1) without the bye shift"""
    n0, h = kk % 2, kk // 2
    s = n0 if shift else 0
    return n0, [s + 2 * j for j in range(h)], [s + 2 * j + 1 for j in range(h)]


def leaves_ref(mod, bits, tab, outer, k, inner, ncomp, flip, virt, virt_nf=1):
    """the leaf level the kernels never store, as leaf[q][o][j][i] over kv = k + virt positions"""
    kv = k + virt
    T = lambda q, r, j: tab[((q - 1) * 2 + r) * kv + j]
    lv = [[[[None] * inner for _ in range(kv)] for _ in range(outer)] for _ in range(ncomp)]
    for o in range(outer):
        for j in range(kv):
            for i in range(inner):
                if j == k:                              # the public leaf: b' = 1, never flipped
                    b = virt_nf
                else:
                    b = bits[(o * k + j) * inner + i]
                    b = (1 - b) % mod if flip else b
                lv[0][o][j][i] = b
                for q in range(1, ncomp):
                    lv[q][o][j][i] = (T(q, 0, j) + b * T(q, 1, j)) % mod
    return lv


def level_ref(level, outer, kk, inner, ncomp):
    """a stored level (C, outer, kk, inner) as lv[q][o][j][i]"""
    return [[[[level[((q * outer + o) * kk + j) * inner + i] for i in range(inner)] for j in range(kk)] for o in range(outer)]
            for q in range(ncomp)]


def prod_ref(mod, lv, outer, kk, inner, ncomp, shift=True):
    """out[q, o, j, i] = lv[0][first_j] * (lv[q][second_j] - lv[q][first_j]), compact (C, outer, h, inner)"""
    _, a1, a2 = find_pairs(kk, shift)
    return [lv[0][o][x][i] * (lv[q][o][y][i] - lv[q][o][x][i]) % mod
            for q in range(ncomp) for o in range(outer) for x, y in zip(a1, a2) for i in range(inner)]


def apply_ref(mod, lv, v, outer, kk, inner, ncomp, shift=True):
    """out[q, o, n0 + j, i] = lv[q][first_j] + v[q, o, j, i], out[q, o, 0, i] = lv[q][0] when n0: (C, outer, kc, inner)"""
    n0, a1, _ = find_pairs(kk, shift)
    h = kk // 2
    out = []
    for q in range(ncomp):
        for o in range(outer):
            if n0:
                out += [lv[q][o][0 if shift else kk - 1][i] for i in range(inner)]
            out += [(lv[q][o][x][i] + v[((q * outer + o) * h + j) * inner + i]) % mod for j, x in enumerate(a1) for i in range(inner)]
    return out


class FindCpuFieldContext(TourCpuFieldContext):
    FIND_MAX_VALUES = 4
    find_ignores_flip = False       # three deliberately wrong contexts set one of these: the tests must then fail
    find_virtual_nf_zero = False
    find_no_bye_shift = False

    def _find_chk(self, a, tab, outer, k, inner, ncomp, flip, virt, leaf):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if outer < 1 or k < 1 or inner < 1 or not 2 <= ncomp <= 5 or flip not in (0, 1) or virt not in (0, 1) or k + virt < 2:
            raise ValueError('not a round of the search over an (outer, k, inner) array')
        if a.n != (1 if leaf else ncomp) * outer * k * inner:
            raise ValueError('operand of the wrong size')
        if tab is not None and tab.n != (ncomp - 1) * 2 * (k + virt):
            raise ValueError('table of the wrong size')

    def _leaves(self, bits, tab, outer, k, inner, ncomp, flip, virt):
        return leaves_ref(self.modulus, bits.to_ints(), tab.to_ints(), outer, k, inner, ncomp, 0 if self.find_ignores_flip else flip,
                          virt, 0 if self.find_virtual_nf_zero else 1)

    def find_leaf_prod(self, bits, tab, outer, k, inner, ncomp, flip=0, virt=0, out=None):
        self._find_chk(bits, tab, outer, k, inner, ncomp, flip, virt, True)
        lv = self._leaves(bits, tab, outer, k, inner, ncomp, flip, virt)
        return self._put_out(out, prod_ref(self.modulus, lv, outer, k + virt, inner, ncomp, not self.find_no_bye_shift))

    def find_leaf_apply(self, bits, tab, rows, lambdas, outer, k, inner, ncomp, flip=0, virt=0, out=None):
        self._find_chk(bits, tab, outer, k, inner, ncomp, flip, virt, True)
        kv = k + virt
        v = self._tour_v(rows, lambdas, ncomp * outer * (kv // 2) * inner)
        lv = self._leaves(bits, tab, outer, k, inner, ncomp, flip, virt)
        return self._put_out(out, apply_ref(self.modulus, lv, v, outer, kv, inner, ncomp, not self.find_no_bye_shift))

    def find_prod(self, level, outer, k, inner, ncomp, out=None):
        self._find_chk(level, None, outer, k, inner, ncomp, 0, 0, False)
        lv = level_ref(level.to_ints(), outer, k, inner, ncomp)
        return self._put_out(out, prod_ref(self.modulus, lv, outer, k, inner, ncomp))
