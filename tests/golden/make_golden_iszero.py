#!/usr/bin/env python3
"""Generate tests/golden/iszero/iszero.json from the REAL reference (lschoe/mpyc, pure Python): runtime.np_equal on secure
integer and fixed-point arrays, which of its two routes it enters per (bit length, sec_param), and Legendre symbols, one
party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_iszero.py --no-log

  equal    per type SecInt(64), SecInt(32), SecFxp(64): the modulus p of its field, RAW integer operands a and b (for the
           fixed-point type a = round(x 2^f)) with equal and unequal pairs, 0, +-1 and the extremes of the range, the opened
           mpc.np_equal(a, b) as 0 / 1 (for the fixed-point type in units of the output: 1.0 is 1), and which of
           runtime._np_is_zero / np_sgn the call entered (counted);
  routes   per l in (16, 31, 32, 61, 62, 64, 128) and sec_param in (7, 8, 30, 40): the modulus of a fresh SecInt(l) under
           that sec_param and how often np_equal on a 3-element array entered _np_is_zero and np_sgn;
  is_sqr   per test prime 64 values -- 0, 1, p - 1, 2, p - 2, a square and a non-square of small numbers, then random
           ones -- and GF(p).array(values).is_sqr() (finfields.py:1464-1470; 0 counts as a square).
Data only, a few KB.  The fixture has a directory of its own, as tests/golden/explog has.
"""
import json
import os
import random

import numpy as np

from mpyc import finfields, sectypes
from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'iszero')
ROUTE_L = (16, 31, 32, 61, 62, 64, 128)
ROUTE_K = (7, 8, 30, 40)
PRIMES = {'rc32': 2**31 - 1, 'pm64-mersenne': 2**61 - 1, 'pm64-k64': 2**64 - 189, 'pm64-gen': 2**40 - 87, 'pm64-gen-blum': 2**40 - 213,
          'rc64': 6616326157076047771, 'pm96': 2**80 - 65, 'pm128': 2**128 - 173, 'pm192': 2**136 - 113,
          'mont128': 258797994007609146293811961253269568351, 'mont192': 2**135 + 4823}


class Counted:
    """counts the calls of runtime._np_is_zero and runtime.np_sgn while it is entered"""

    def __enter__(self):
        self.real = mpc._np_is_zero, mpc.np_sgn
        self.calls = {'_np_is_zero': 0, 'np_sgn': 0}

        def is_zero(a):
            self.calls['_np_is_zero'] += 1
            return self.real[0](a)

        def sgn(a, **kw):
            self.calls['np_sgn'] += 1
            return self.real[1](a, **kw)

        mpc._np_is_zero, mpc.np_sgn = is_zero, sgn
        return self

    def __exit__(self, *exc):
        mpc._np_is_zero, mpc.np_sgn = self.real


def pairs(rng, l):
    """raw operand pairs of an l-bit type: equal and unequal, 0, +-1, the extremes, neighbours, random ones"""
    lo, hi = -(1 << (l - 1)), (1 << (l - 1)) - 1
    a = [0, 0, 1, -1, 1, hi, lo, hi, lo, hi, 0, 5, -5, hi - 1, lo + 1]
    b = [0, 1, 1, -1, -1, hi, lo, lo, hi, hi - 1, lo, -5, -5, hi, lo]
    for _ in range(25):
        x, y = rng.randrange(lo, hi + 1), rng.randrange(lo, hi + 1)
        a += [x, x, x]
        b += [x, y, x ^ (1 << rng.randrange(l - 1))]
    return a, b


async def main():
    rng = random.Random(20261020)
    doc = {'source': 'mpyc.runtime.np_equal / _np_is_zero / np_sgn and finfields is_sqr, one party; raw integers', 'equal': [],
           'routes': [], 'is_sqr': []}
    await mpc.start()
    doc['sec_param'] = mpc.options.sec_param
    for kind, l in (('SecInt', 64), ('SecInt', 32), ('SecFxp', 64)):
        stype = mpc.SecInt(l) if kind == 'SecInt' else mpc.SecFxp(l)
        f = getattr(stype, 'frac_length', 0)
        p = stype.field.modulus
        a, b = pairs(rng, l)
        raw = lambda v: stype.array(stype.field.array(np.array([x % p for x in v], dtype=object)))
        with Counted() as cnt:
            out = await mpc.output(mpc.np_equal(raw(a), raw(b)))
        got = [int(round(float(v))) for v in np.asarray(out).reshape(-1)]
        assert got == [int(x == y) for x, y in zip(a, b)], kind
        doc['equal'].append({'type': kind, 'l': l, 'f': f, 'p': p, 'a': a, 'b': b, 'equal': got, 'calls': cnt.calls})
    default = mpc.options.sec_param
    for l in ROUTE_L:
        for k in ROUTE_K:
            mpc.options.sec_param = k
            sectypes._SecInt.cache_clear()
            secint = mpc.SecInt(l)
            with Counted() as cnt:
                out = await mpc.output(mpc.np_equal(secint.array(np.array([3, -4, 0])), secint.array(np.array([3, 4, 1]))))
            assert [int(v) for v in out] == [1, 0, 0], (l, k)
            doc['routes'].append({'l': l, 'sec_param': k, 'p': secint.field.modulus, 'calls': cnt.calls})
    mpc.options.sec_param = default
    sectypes._SecInt.cache_clear()
    for name, p in PRIMES.items():
        vals = [0, 1, p - 1, 2, p - 2, 9 * 9 % p, 4, 3, p - 4, p - 9]
        while len(vals) < 64:
            vals.append(rng.randrange(p))
        sq = finfields.GF(p).array(np.array(vals, dtype=object)).is_sqr()
        doc['is_sqr'].append({'name': name, 'p': p, 'values': vals, 'is_sqr': [int(bool(v)) for v in sq]})
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'iszero.json'), 'w') as fh:
        json.dump(doc, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
