#!/usr/bin/env python3
"""Generate tests/golden/fxp/fxp.json from the REAL reference (lschoe/mpyc, pure Python): runtime._norm, runtime._rec,
runtime.np_divide and runtime.np_trunc on SecFxp(l, f) arrays, one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_fxp.py --no-log

Everything is recorded as RAW integers a = round(x 2^f).  Per (l, f) in (32, 16), (16, 8), (24, 12):
  norm_in / norm   planted values (+-1, +-2^(l-2), -2^(l-1), 2^(l-1) - 1, every single-bit value and its negative) and the
                   opened _norm of each: exact, _norm draws no rounding bits;
  den / den_norm   about 90 denominators, all nonzero with representable reciprocals (|a| > 2^(2f-l+1)): the planted values
                   that qualify, then random ones of every magnitude; their opened _norm;
  num              a second random array;
  rec, div, trunc  _rec(den), np_divide(num, den) and np_trunc(den) (the raw integer loses its f low bits) each evaluated 8
                   times in this one run and recorded as the per-element minimum and maximum: the probabilistic rounding
                   draws fresh bits per call.  trunc_in is the raw input of np_trunc.
Data only, a few KB.  The fixture has a directory of its own: tests/golden/*.json are the files make_golden.py writes
(tests/test_wire.py compares the two lists).
"""
import json
import os
import random

import numpy as np

from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fxp')     # GOLDEN_OUT: regenerate elsewhere
PARAMS = [(32, 16), (16, 8), (24, 12)]
REPEATS = 8
N_DEN = 90


def planted(l):
    vals = [1, -1, 1 << (l - 2), -(1 << (l - 2)), -(1 << (l - 1)), (1 << (l - 1)) - 1]
    for k in range(l - 1):
        vals += [1 << k, -(1 << k)]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


def denominators(rng, l, f):
    lo = 1 << (2 * f - l + 1)
    out = [v for v in planted(l) if abs(v) > lo]
    out = out[:40]
    while len(out) < N_DEN:
        bits = rng.randint(2 * f - l + 3, l - 1)              # every magnitude, not only the large ones
        v = rng.randrange(1 << (bits - 1), 1 << bits) * rng.choice((1, -1))
        if abs(v) > lo and -(1 << (l - 1)) <= v < (1 << (l - 1)):
            out.append(v)
    return out


async def main():
    rng = random.Random(20261019)
    doc = {'source': 'mpyc.runtime._norm / _rec / np_divide / np_trunc, SecFxp(l, f), one party; raw integers', 'repeats': REPEATS,
           'cases': []}
    await mpc.start()
    for l, f in PARAMS:
        secfxp = mpc.SecFxp(l, f)
        scale = float(1 << f)
        arr = lambda raw: secfxp.array(np.array(raw, dtype=float) / scale)

        async def raw_of(x):
            return [int(v) for v in np.rint(np.asarray(await mpc.output(x), dtype=float).reshape(-1) * scale)]

        async def spread(fn):
            runs = [await raw_of(fn()) for _ in range(REPEATS)]
            return [min(c) for c in zip(*runs)], [max(c) for c in zip(*runs)]

        norm_in = planted(l)
        den = denominators(rng, l, f)
        # numerators small enough that num / den is representable: |num| 2^f / |den| < 2^(l-1)
        num = [rng.randrange(-(abs(d) << max(l - f - 2, 0)) >> 1, ((abs(d) << max(l - f - 2, 0)) >> 1) + 1) for d in den]
        num = [max(-(1 << (l - 2)), min((1 << (l - 2)), v)) for v in num]
        case = {'l': l, 'f': f, 'norm_in': norm_in, 'norm': await raw_of(mpc._norm(arr(norm_in))),
                'den': den, 'den_norm': await raw_of(mpc._norm(arr(den))), 'num': num}
        case['rec_min'], case['rec_max'] = await spread(lambda: mpc._rec(arr(den)))
        case['div_min'], case['div_max'] = await spread(lambda: mpc.np_divide(arr(num), arr(den)))
        case['trunc_in'] = den
        case['trunc_min'], case['trunc_max'] = await spread(lambda: mpc.np_trunc(arr(den)))
        for a, lo, hi in zip(case['trunc_in'], case['trunc_min'], case['trunc_max']):
            assert a >> f <= lo <= hi <= (a >> f) + 1, (a, lo, hi)
        doc['cases'].append(case)
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'fxp.json'), 'w') as fh:
        json.dump(doc, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
