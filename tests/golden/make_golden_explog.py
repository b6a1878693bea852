#!/usr/bin/env python3
"""Generate tests/golden/explog/explog.json from the REAL reference (lschoe/mpyc, pure Python): runtime.np_log, np_log2,
np_exp2, np_exp and np_pow with a public integer base on SecFxp(l, f) arrays, one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_explog.py --no-log

Everything is recorded as RAW integers a = round(x 2^f).  Per (l, f) in (32, 16), (16, 8), (24, 12):
  log_in     about 150 positive values: 1, 2, 3, 2^(l-1) - 1, every single-bit value, then random ones of every magnitude;
  exp2_in    about 150 values: 0, +-1, +-2^f, (-f) 2^f, (l-1-f) 2^f - 1, then random raw values in [(-f) 2^f, (l-1-f) 2^f);
  exp_in     exp2_in scaled into the domain of np_exp (times log 2, rounded towards zero);
  *_nearest  log, log2, exp2 and exp evaluated ONCE with runtime.np_random_bits replaced by a coroutine that hands every
             truncation the bit pattern of 2^(f'-1) for each element (f' the bits that truncation drops): np_trunc then
             returns floor((a + 2^(f'-1)) / 2^f'), whatever the high mask, so the run is deterministic (checked below: two
             such runs agree).  Bit decompositions get zero bits from it; their result does not depend on the bits;
  *_min/_max log and exp2 evaluated 32 times with the reference's own random bits, recorded as the per-element extremes;
  pow3, pow2 np_pow(3, .) and np_pow(2, .) on a few integral exponents (recorded as the plain integers B): exact.
Data only, a few KB.  The fixture has a directory of its own, as tests/golden/fxp has.
"""
import json
import math
import os
import random

import numpy as np

from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'explog')
PARAMS = [(32, 16), (16, 8), (24, 12)]
REPEATS = 32
N_IN = 150


def log_inputs(rng, l):
    vals = [1, 2, 3, (1 << (l - 1)) - 1] + [1 << k for k in range(l - 1)]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    while len(out) < N_IN:
        bits = rng.randint(1, l - 1)
        out.append(rng.randrange(1 << (bits - 1), 1 << bits))
    return out


def exp2_inputs(rng, l, f):
    lo, hi = (-f) << f, (l - 1 - f) << f
    out = [0, 1, -1, 1 << f, -(1 << f), lo, hi - 1]
    while len(out) < N_IN:
        out.append(rng.randrange(lo, hi))
    return out


class NearestBits:
    """np_random_bits for the deterministic run: np_trunc announces the bit count it is about to draw for"""

    def __init__(self):
        self.real_bits, self.real_trunc, self.f = mpc.np_random_bits, mpc.np_trunc, None

    def __enter__(self):
        def np_trunc(a, f=None, l=None):
            self.f = type(a).frac_length if f is None else f
            return self.real_trunc(a, f=f, l=l)

        async def np_random_bits(sftype, n, signed=False):
            f, self.f = self.f, None
            bits = [0] * n if f is None else ([0] * (f - 1) + [1]) * (n // f)
            assert len(bits) == n and not signed
            return sftype.array(np.array(bits, dtype=object))

        mpc.np_trunc, mpc.np_random_bits = np_trunc, np_random_bits
        return self

    def __exit__(self, *exc):
        mpc.np_trunc, mpc.np_random_bits = self.real_trunc, self.real_bits


async def main():
    rng = random.Random(20261019)
    doc = {'source': 'mpyc.runtime.np_log / np_log2 / np_exp2 / np_exp / np_pow, SecFxp(l, f), one party; raw integers',
           'repeats': REPEATS, 'cases': []}
    await mpc.start()
    assert mpc.options.no_async, 'the deterministic run relies on coroutines running to completion in call order'
    for l, f in PARAMS:
        secfxp = mpc.SecFxp(l, f)
        scale = float(1 << f)
        arr = lambda raw: secfxp.array(np.array(raw, dtype=float) / scale)

        async def raw_of(x):
            return [int(v) for v in np.rint(np.asarray(await mpc.output(x), dtype=float).reshape(-1) * scale)]

        async def spread(fn):
            runs = [await raw_of(fn()) for _ in range(REPEATS)]
            return [min(c) for c in zip(*runs)], [max(c) for c in zip(*runs)]

        log_in = log_inputs(rng, l)
        exp2_in = exp2_inputs(rng, l, f)
        exp_in = [int(v * math.log(2)) for v in exp2_in]
        case = {'l': l, 'f': f, 'log_in': log_in, 'exp2_in': exp2_in, 'exp_in': exp_in}
        fns = (('log', mpc.np_log, log_in), ('log2', mpc.np_log2, log_in), ('exp2', mpc.np_exp2, exp2_in), ('exp', mpc.np_exp, exp_in))
        with NearestBits():
            for name, fn, vals in fns:
                case[name + '_nearest'] = await raw_of(fn(arr(vals)))
                assert case[name + '_nearest'] == await raw_of(fn(arr(vals))), name
        for name, fn, vals in (fns[0], fns[2]):
            case[name + '_min'], case[name + '_max'] = await spread(lambda: fn(arr(vals)))
        for a, y in zip(log_in, case['log_nearest']):
            assert abs(y / scale - math.log(a / scale)) < 2.0**(3 - f), (a, y)
        for a, y in zip(exp2_in, case['exp2_nearest']):
            assert abs(y / scale - 2.0**(a / scale)) < 2.0**(3 - f) * max(1.0, 2.0**(a / scale)), (a, y)
        b3 = list(range(0, int((l - 2 - f) / math.log2(3)) + 1))
        b2 = list(range(0, l - 1 - f))
        case['pow3_in'], case['pow2_in'] = b3, b2
        case['pow3'] = await raw_of(mpc.np_pow(3, secfxp.array(np.array(b3))))
        case['pow2'] = await raw_of(mpc.np_pow(2, secfxp.array(np.array(b2))))
        assert case['pow3'] == [3**b << f for b in b3] and case['pow2'] == [2**b << f for b in b2]
        doc['cases'].append(case)
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'explog.json'), 'w') as fh:
        json.dump(doc, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
