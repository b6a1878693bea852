#!/usr/bin/env python3
"""Generate tests/golden/tour/tournament.json from the REAL reference (lschoe/mpyc, pure Python): runtime.np_argmax /
np_argmin (runtime.py:3695-3949) with arg_unary=True, arg_only=False and runtime.np_amax / np_amin (runtime.py:3377-3473)
along axis 1 of small SecInt(16) arrays of shape (outer, k, inner), one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_tour.py --no-log

Per array: the values (row-major; both extremes, duplicates of the maximum and of the minimum, an all-equal row) and what
the reference's protocols return: the unit vectors in the shape of the input, the maxima / minima as (outer, 1, inner).
Data only, a few KB.  The fixture has a directory of its own: tests/golden/*.json are the files make_golden.py writes
(tests/test_wire.py compares the two lists).
"""
import json
import os
import random

import numpy as np

from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tour')     # GOLDEN_OUT: regenerate elsewhere
SHAPES = [(1, 2, 1), (7, 3, 1), (4, 7, 1), (2, 5, 3), (1, 16, 2)]
L = 16


def values(rng, shape):
    """integers of L-2 signed bits (every difference has L-1 signed bits) with ties"""
    outer, k, inner = shape
    lo, hi = -(1 << (L - 3)), (1 << (L - 3)) - 1
    a = np.array([rng.randint(lo, hi) for _ in range(outer * k * inner)]).reshape(shape)
    a[0, 0, 0], a[-1, -1, -1] = hi, lo
    if k > 2:
        a[0, k - 1, 0] = hi                 # the maximum twice: the first occurrence counts
        a[-1, 1, -1] = lo                   # and the minimum
    if outer > 2:
        a[1, :, :] = 5                      # an all-equal row
    return a


def flat(x):
    return [int(v) for v in np.asarray(x).reshape(-1).tolist()]


async def main():
    rng = random.Random(20261019)
    out = {'source': 'mpyc.runtime.np_argmax / np_argmin (arg_unary=True, arg_only=False, keepdims=True), np_amax / np_amin '
                     '(keepdims=True), axis 1, one party', 'l': L, 'cases': []}
    secint = mpc.SecInt(L)
    await mpc.start()
    for shape in SHAPES:
        vals = values(rng, shape)
        a = secint.array(vals)
        umax, vmax = mpc.np_argmax(a, axis=1, keepdims=True, arg_unary=True, arg_only=False)
        umin, vmin = mpc.np_argmin(a, axis=1, keepdims=True, arg_unary=True, arg_only=False)
        case = {'shape': list(shape), 'values': flat(vals),
                'argmax_unit': flat(await mpc.output(umax)), 'argmax_value': flat(await mpc.output(vmax)),
                'argmin_unit': flat(await mpc.output(umin)), 'argmin_value': flat(await mpc.output(vmin)),
                'amax': flat(await mpc.output(mpc.np_amax(a, axis=1, keepdims=True))),
                'amin': flat(await mpc.output(mpc.np_amin(a, axis=1, keepdims=True)))}
        assert case['amax'] == flat(vals.max(axis=1)) == case['argmax_value'] and case['amin'] == flat(vals.min(axis=1)) == case['argmin_value']
        unit = lambda idx: flat(np.moveaxis(np.eye(shape[1], dtype=int)[idx], -1, 1))
        assert case['argmax_unit'] == unit(vals.argmax(axis=1)) and case['argmin_unit'] == unit(vals.argmin(axis=1))
        out['cases'].append(case)
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'tournament.json'), 'w') as fh:
        json.dump(out, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
