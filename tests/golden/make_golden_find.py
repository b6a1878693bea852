#!/usr/bin/env python3
"""Generate tests/golden/find/find.json from the REAL reference (lschoe/mpyc, pure Python): runtime.np_find
(runtime.py:4603-4698) along axis 1 of small SecInt(16) arrays of shape (outer, k, inner), one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_find.py --no-log

Per array: the bits (row-major; columns along k that are all ones, all zeros, have their first 0 at position 0, at k - 1,
and a repeated hit) and, for s = 0 and s = 1, what the reference returns with the default e, e=-1, e='a.shape[axis]-1' and
e=None (nf and ix), with cs_f = (b+1) << i, with the tuple cs_f = (i+b, (b+1) << i) and with f = k - i; and for integers in
-3..3 the first 2 with bits=False and e=-1.  Every result is (outer, inner), row-major.
Data only, a few KB.  The fixture has a directory of its own: tests/golden/*.json are the files make_golden.py writes
(tests/test_wire.py compares the two lists).
"""
import json
import os
import random

import numpy as np

from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'find')     # GOLDEN_OUT: regenerate elsewhere
SHAPES = [(1, 1, 1), (1, 2, 1), (7, 3, 1), (4, 7, 1), (2, 5, 3), (1, 16, 2), (3, 33, 1)]
L = 16


def column(rng, k, which):
    """the planted columns, then random ones"""
    if which == 0:
        return [1] * k
    if which == 1:
        return [0] * k
    if which == 2:
        return [0] + [1] * (k - 1)
    if which == 3:
        return [1] * (k - 1) + [0]
    if which == 4:
        return [(j + 1) % 2 for j in range(k)]
    if which == 5:
        return [0] * (k - 1) + [1]
    return [rng.randrange(2) for _ in range(k)]


def bit_array(rng, shape, first):
    outer, k, inner = shape
    a = np.zeros(shape, dtype=int)
    for c in range(outer * inner):
        a[c // inner, :, c % inner] = column(rng, k, first + c)
    return a


def int_array(rng, shape):
    """integers in -3..3: a column of 2s, a column without a 2, a 2 at the end only, random ones"""
    outer, k, inner = shape
    a = np.array([rng.randint(-3, 3) for _ in range(outer * k * inner)]).reshape(shape)
    cols = [(c // inner, c % inner) for c in range(outer * inner)]
    a[cols[0][0], :, cols[0][1]] = 2
    if len(cols) > 1:
        o, i = cols[1]
        a[o, :, i] = np.where(a[o, :, i] == 2, -2, a[o, :, i])
    if len(cols) > 2:
        o, i = cols[2]
        a[o, :, i] = np.where(a[o, :, i] == 2, 1, a[o, :, i])
        a[o, k - 1, i] = 2
    return a


def flat(x):
    return [int(v) for v in np.asarray(x).reshape(-1).tolist()]


async def main():
    rng = random.Random(20261019)
    out = {'source': 'mpyc.runtime.np_find, axis 1, SecInt(16), one party', 'l': L, 'cases': []}
    secint = mpc.SecInt(L)
    await mpc.start()
    opened = lambda x: mpc.output(x)
    for n, shape in enumerate(SHAPES):
        k = shape[1]
        bits = bit_array(rng, shape, n % 6 if shape[0] * shape[2] == 1 else 0)
        a = secint.array(bits)
        case = {'shape': list(shape), 'bits': flat(bits), 's': {}}
        for s in (0, 1):
            nf, ix = mpc.np_find(a, s, axis=1, e=None)
            both = mpc.np_find(a, s, axis=1, cs_f=lambda b, i: (i + b, (b + 1) << i))
            r = {'e_default': flat(await opened(mpc.np_find(a, s, axis=1))),
                 'e_minus1': flat(await opened(mpc.np_find(a, s, axis=1, e=-1))),
                 'e_last': flat(await opened(mpc.np_find(a, s, axis=1, e='a.shape[axis]-1'))),
                 'raw_nf': flat(await opened(nf)), 'raw_ix': flat(await opened(ix)),
                 'pow': flat(await opened(mpc.np_find(a, s, axis=1, cs_f=lambda b, i: (b + 1) << i))),
                 'tuple': [flat(await opened(c)) for c in both],
                 'f': flat(await opened(mpc.np_find(a, s, axis=1, f=lambda i: k - i)))}
            hit = bits == s
            want = np.where(hit.any(axis=1), hit.argmax(axis=1), k)
            assert r['e_default'] == flat(want) == r['tuple'][0] and r['raw_nf'] == flat(~hit.any(axis=1))
            assert r['pow'] == [1 << v for v in r['e_default']] == r['tuple'][1] and r['f'] == [k - v for v in r['e_default']]
            assert r['e_minus1'] == flat(np.where(hit.any(axis=1), want, -1)) and r['e_last'] == flat(np.minimum(want, k - 1))
            case['s'][str(s)] = r
        ints = int_array(rng, shape)
        case['ints'] = flat(ints)
        case['ints_s'] = 2
        case['ints_e_minus1'] = flat(await opened(mpc.np_find(secint.array(ints), 2, axis=1, bits=False, e=-1)))
        hit = ints == 2
        assert case['ints_e_minus1'] == flat(np.where(hit.any(axis=1), hit.argmax(axis=1), -1))
        out['cases'].append(case)
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'find.json'), 'w') as fh:
        json.dump(out, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
