"""TEST INFRASTRUCTURE ONLY: tests/cpuctx.py's Python-integer stand-in for engine.FieldContext, plus the three local
steps of the secure comparison (engine.FieldContext.sgn_mask / sgn_expand / sgn_finish) on Python integers, straight
from the maps include/ffgpu.h states.  mpyc_amd/protocols.py composes whole protocols from a context's methods, so the
`-m "not gpu"` tests run protocols.compare_zero end to end on it."""
from cpuctx import CpuFieldContext


def mask_ref(p, a, rbits, rdivl, l):
    n = len(a)
    return [(a[h] + (1 << l) + sum(rbits[h * l + i] << (l - 1 - i) for i in range(l)) + (rdivl[h] << l)) % p
            for h in range(n)]


def expand_ref(p, c, a, rbits, sbit, l):
    """(e, nx, z) as flat bit-major lists; sbit None: e is None"""
    n = len(a)
    e = [0] * ((l + 1) * n) if sbit is not None else None
    nx, z = [0] * (l * n), [0] * n
    for h in range(n):
        cl = c[h] & ((1 << l) - 1)
        s = (2 * sbit[h] - 1) % p if sbit is not None else 0
        S = 0
        for i in range(l):
            cb, r = (cl >> (l - 1 - i)) & 1, rbits[h * l + i]
            x = (1 - r) % p if cb else r
            if e is not None:
                e[i * n + h] = (s - cb + r + 3 * S) % p
            nx[i * n + h] = (1 - x) % p
            S = (S + x) % p
        if e is not None:
            e[l * n + h] = (s - 1 + 3 * S) % p
        z[h] = (cl - a[h] - (1 << l) - sum(rbits[h * l + i] << (l - 1 - i) for i in range(l))) % p
    return e, nx, z


def finish_ref(p, w, sbit, z, l):
    inv = pow(1 << l, -1, p)
    out = []
    for wv, sb, zv in zip(w, sbit, z):
        s = 2 * sb - 1
        out.append((zv + ((-s if wv == 0 else s) + 3) * (1 << (l - 1))) * inv % p)
    return out


class SgnCpuFieldContext(CpuFieldContext):
    def _sgn_l(self, l):
        if self.binary:
            raise NotImplementedError('prime fields only')
        if l < 1 or l > 64 or l > self.modulus.bit_length() - 2:
            raise ValueError('bit length out of range')

    def sgn_mask(self, a, rbits, rdivl, l, out=None):
        self._sgn_l(l)
        out = out or self.empty(a.n)
        return self._put(out, mask_ref(self.modulus, a.to_ints(), rbits.to_ints(), rdivl.to_ints(), l))

    def sgn_expand(self, c, a, rbits, sbit, l, want_e=True, want_nx=False):
        self._sgn_l(l)
        if want_e and sbit is None:
            raise ValueError('sgn_expand: e needs the sign-mask bit shares')
        n = a.n
        e, nx, z = expand_ref(self.modulus, c.to_ints(), a.to_ints(), rbits.to_ints(), sbit.to_ints() if want_e else None, l)
        return (self._put(self.empty((l + 1) * n), e) if want_e else None,
                self._put(self.empty(l * n), nx) if want_nx else None, self._put(self.empty(n), z))

    def sgn_finish(self, w, sbit, z, l, out=None):
        self._sgn_l(l)
        out = out or self.empty(w.n)
        return self._put(out, finish_ref(self.modulus, w.to_ints(), sbit.to_ints(), z.to_ints(), l))
