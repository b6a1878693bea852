"""TEST INFRASTRUCTURE ONLY: tests/iszero_cpuctx.py plus the two local steps of secure random bits
(engine.FieldContext.rbits_open / rbits_finish) on Python integers, straight from the maps include/ffgpu_math.h states, and
the device PRF of the PRSS through the C oracle (orc_prss_chacha), so that protocols.Randomness draws on the CPU what it draws
on the GPU for the same key.  The `-m "not gpu"` tests run protocols.random_bits / Randomness end to end on it."""
import numpy as np
import torch

from iszero_cpuctx import IszeroCpuFieldContext
from oracle import coracle

MAX_ROWS = 64


def rbits_open_ref(p, rs, zs, lam, without_z=False):
    """c[h] = sum_i lam[i] (r_i[h]^2 + z_i[h])"""
    return [sum(l * (r[h] * r[h] + (0 if without_z else z[h])) for l, r, z in zip(lam, rs, zs)) % p for h in range(len(rs[0]))]


def rbits_finish_ref(p, c, rs, signed, f, keep_zero=False, one_after_half=False):
    """s = c^((3p-5)/4); r s 2^f when signed, else (r s + 1) (p+1)/2 2^f; 0 where c is 0"""
    assert p % 4 == 3
    half, e = (p + 1) >> 1, (3 * p - 5) >> 2
    s = [pow(v, e, p) for v in c]
    out = []
    for r in rs:
        row = []
        for v, sv, rv in zip(c, s, r):
            b = rv * sv % p
            if not signed:
                b = (b * half + 1) % p if one_after_half else (b + 1) * half % p
            row.append(0 if v == 0 and not keep_zero else (b << f) % p)
        out.append(row)
    return out


class RbitsCpuFieldContext(IszeroCpuFieldContext):
    # deliberately wrong contexts set one of these: the tests must then fail
    open_without_z = False          # rbits_open leaves the zero sharing out
    finish_keeps_zero = False       # rbits_finish does not store 0 where the square is 0
    finish_one_after_half = False   # rbits_finish adds the 1 after the halving

    def zero_counter(self):
        return torch.zeros(1, dtype=torch.int32)

    def rbits_open(self, rs, zs, lambdas, zeros=None, out=None):
        self._prime('rbits_open')
        k = len(rs)
        if not 1 <= k <= MAX_ROWS or len(zs) != k or len(lambdas) != k:
            raise ValueError('rbits_open: 1..64 rows of r, as many of z and as many lambdas')
        n = rs[0].n
        if any(x.n != n for x in list(rs) + list(zs)) or (out is not None and out.n != n):
            raise ValueError('rbits_open: rows of one length')
        self._counter('rbits_open', zeros)
        vals = rbits_open_ref(self.modulus, [r.to_ints() for r in rs], [z.to_ints() for z in zs], [int(v) for v in lambdas],
                              without_z=self.open_without_z)
        if zeros is not None:
            zeros += sum(v == 0 for v in vals)
        return self._put(self.empty(n) if out is None else out, vals)

    def rbits_finish(self, c, rs, signed=False, f=0, outs=None):
        self._prime('rbits_finish')
        if self.modulus % 4 != 3:
            raise NotImplementedError('rbits_finish: p = 3 mod 4')
        m = len(rs)
        if not 1 <= m <= MAX_ROWS or f < 0 or f >= 192:
            raise ValueError('rbits_finish: 1..64 rows, 0 <= f < 192')
        if any(r.n != c.n for r in rs) or (outs is not None and (len(outs) != m or any(o.n != c.n for o in outs))):
            raise ValueError('rbits_finish: rows of one length, one output per row')
        rows = rbits_finish_ref(self.modulus, c.to_ints(), [r.to_ints() for r in rs], signed, f, keep_zero=self.finish_keeps_zero,
                                one_after_half=self.finish_one_after_half)
        outs = [self.empty(c.n) for _ in range(m)] if outs is None else list(outs)
        return [self._put(o, row) for o, row in zip(outs, rows)]

    def prss_chacha(self, keys40, d, l, weights, n, mask_bits=0, rounds=20, out=None, accumulate=False):
        """the oracle's C restatement of ffgpu_prss_chacha where it applies (fields of up to 128 bits, draws of up to 32
        bytes), the Python-integer one of tests/cpuctx.py otherwise"""
        if self.elem_bytes > 16 or l > 32 or n == 0:
            return super().prss_chacha(keys40, d, l, weights, n, mask_bits, rounds, out, accumulate)
        out = self.empty(n) if out is None else out
        buf = np.ascontiguousarray(out.to_numpy()) if accumulate else None
        res = coracle.prss_chacha(coracle.CField(self.modulus, self.binary), keys40, d, l, mask_bits, rounds, [int(w) for w in weights], n,
                                  out=buf, accumulate=accumulate)
        out.t.copy_(self.from_numpy(res).t.reshape(out.t.shape))
        return out
