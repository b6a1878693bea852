"""TEST INFRASTRUCTURE ONLY: tests/unitvec_cpuctx.py plus the 2-D correlation of a secure convolution layer
(engine.FieldContext.conv2d / conv2d_plan) on Python integers, straight from the formula include/ffgpu_math.h states -- not
from the kernel.  The `-m "not gpu"` tests run protocols.conv2d / maxpool2x2 / relu / conv_layer / dense end to end on it, and
the GPU tests compare the kernel with conv2d_ref byte for byte."""
import numpy as np

from mpyc_amd.engine import Conv2dPlan
from unitvec_cpuctx import UnitvecCpuFieldContext

MAX_S = 16
MAX_SENDERS = 64


def conv2d_ref(p, x, W, b, k, r, m, n, v, s, row_off=None, col_off=None):
    """Y[i, j, I, J] = b[j] + sum_{l, di, dj} x[i, l, I + di - (s-1)//2, J + dj - s//2] W[j, l, di, dj] mod p on flat row-major
    lists, x outside [0, m) x [0, n) counting as 0; b None: no bias"""
    ro = (s - 1) // 2 if row_off is None else row_off
    co = s // 2 if col_off is None else col_off
    if not k * v * m * n:
        return []
    # the image inside a frame of zeros, so that x[.., I + di - ro, J + dj - co] is xp[.., I + di, J + dj] for every term; one
    # exact Python-integer product per (output, term), summed term by term over whole (k, v, m, n) arrays
    xp = np.zeros((k, r, m + s - 1, n + s - 1), dtype=object)
    xp[:, :, ro:ro + m, co:co + n] = np.array(list(x), dtype=object).reshape(k, r, m, n)
    Wa = np.array(list(W), dtype=object).reshape(v, r, s, s)
    Y = np.zeros((k, v, m, n), dtype=object)
    if b is not None:
        Y += np.array(list(b), dtype=object).reshape(1, v, 1, 1)
    for l in range(r):
        for di in range(s):
            for dj in range(s):
                Y += xp[:, l, di:di + m, dj:dj + n][:, None, :, :] * Wa[:, l, di, dj][None, :, None, None]
    return [int(y) % p for y in Y.reshape(-1)]


class Conv2dCpuFieldContext(UnitvecCpuFieldContext):
    # deliberately wrong contexts set one of these: the tests must then fail
    col_off_is_row_off = False      # both offsets (s-1)//2: wrong for even s
    without_bias = False            # the bias is left out

    def _conv2d_check(self, what, k, r, m, n, v, s, nsend):
        self._prime(what)
        if nsend > MAX_SENDERS:
            raise NotImplementedError(f'{what}: at most 64 senders')
        if nsend < 1 or min(k, r, m, n, v) < 0 or not 1 <= s <= MAX_S:
            raise ValueError(f'{what}: at least one sender, counts >= 0 and 1 <= s <= 16')
        if (k * v * m * n and (s > n or r < 1)) or (not k * v * m * n and n and s > n):
            raise ValueError(f'{what}: s <= n and at least one input channel')

    def conv2d_plan(self, k, r, m, n, v, s, nsend=1):
        """no kernel, no tiles: the whole image is one `tile`"""
        self._conv2d_check('conv2d_plan', k, r, m, n, v, s, nsend)
        return Conv2dPlan(max(m, 1), max(n, 1), max(v, 1), max(r, 1), 1, False, (k, nsend), 0)

    def conv2d(self, xs, ws, bs, k, r, m, n, v, s, outs=None):
        nsend = len(xs)
        self._conv2d_check('conv2d', k, r, m, n, v, s, nsend)
        on = k * v * m * n
        if len(ws) != nsend or (bs is not None and len(bs) != nsend) or any(x.n != k * r * m * n for x in xs) or \
                any(w.n != v * r * s * s for w in ws) or (bs is not None and any(b.n != v for b in bs)) or \
                (outs is not None and (len(outs) != nsend or any(o.n != on for o in outs))):
            raise ValueError('conv2d: one x (k, r, m, n), one W (v, r, s, s), one b (v) and one output (k, v, m, n) per sender')
        outs = [self.empty(on) for _ in range(nsend)] if outs is None else list(outs)
        co = (s - 1) // 2 if self.col_off_is_row_off else None
        for q in range(nsend):
            b = None if bs is None or self.without_bias else bs[q].to_ints()
            self._put(outs[q], conv2d_ref(self.modulus, xs[q].to_ints(), ws[q].to_ints(), b, k, r, m, n, v, s, col_off=co))
        return outs
