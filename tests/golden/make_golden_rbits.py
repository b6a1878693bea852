#!/usr/bin/env python3
"""Generate tests/golden/rbits/rbits.json from the REAL reference (lschoe/mpyc, pure Python): runtime.np_random_bits over
prime fields, the PRSS branch (runtime.py:4243-4267), one party, no logging, with thresha.np_pseudorandom_share and
thresha.np_pseudorandom_share_0 replaced by recorded, partly planted draws -- with one party a share is the value, so the
opened square is r^2 + z for the recorded r and z.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_rbits.py --no-log

Per test prime (2^61 - 1, 2^64 - 189, the 80-bit default of SecFxp(), all 3 mod 4; 2^40 - 87, 1 mod 4) and per planting case
of COUNT = 12 bits:
  none          no zero square: one draw, the fast path;
  first_last    zero squares at the first entry (r = 0) and at the last (z = -r^2);
  adjacent      two adjacent zero squares;
  all_first     a whole first draw of zero squares, then a clean draw: the fast path again;
  second_again  three zero squares, and a second draw that again contains one;
the draws of every round (r and z as the replaced functions handed them out), the opened squares of every round, and for
signed in (False, True) and f in (0, 16) the returned bits as raw field elements (f = 16: through a SecFxp type with
frac_length 16 over the same prime; the same draws for all four).  z is 0 except where it plants a zero square.
Data only, a few tens of KB.  The fixture has a directory of its own, as tests/golden/iszero has.
"""
import json
import os
import random

import numpy as np

from mpyc import thresha
from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rbits')
COUNT = 12
PRIMES = {'pm64-mersenne': 2**61 - 1, 'pm64-k64': 2**64 - 189, 'pm96': None, 'pm64-gen': 2**40 - 87}     # None: SecFxp()'s own
# per case: per round, the entries (of that round's draw) whose square is 0; 'r': by r = 0, 'z': by z = -r^2
CASES = {
    'none': [{}],
    'first_last': [{0: 'r', COUNT - 1: 'z'}, {}],
    'adjacent': [{4: 'z', 5: 'r'}, {}],
    'all_first': [{i: 'rz'[i % 2] for i in range(COUNT)}, {}],
    'second_again': [{2: 'r', 7: 'z', 9: 'z'}, {1: 'z'}, {}],
}


def rounds_of(rng, p, plan):
    """the draws of every round: (r, z) lists; round j has as many entries as round j - 1 had zero squares"""
    out, h = [], COUNT
    for zeros in plan:
        r = [rng.randrange(1, p) for _ in range(h)]
        z = [0] * h
        for i, how in zeros.items():
            if how == 'r':
                r[i] = 0
            else:
                z[i] = -r[i] * r[i] % p
        out.append((r, z))
        h = len(zeros)
    assert h == 0
    return out


class Planted:
    """replaces the two PRSS functions of mpyc.thresha by the recorded draws, in the order np_random_bits calls them"""

    def __init__(self, rounds):
        self.queue = [(kind, vals) for r, z in rounds for kind, vals in (('r', r), ('z', z))]
        self.opened = []

    def __enter__(self):
        self.real = thresha.np_pseudorandom_share, thresha.np_pseudorandom_share_0, mpc.output

        def take(kind):
            def fn(field, m, i, prfs, uci, n):
                k, vals = self.queue.pop(0)
                assert k == kind and len(vals) == n and m == 1 and i == 0, (k, kind, len(vals), n)
                return field.array(np.array(vals, dtype=object))
            return fn

        def output(x, *args, **kw):
            self.opened.append([int(v) for v in x.value])
            return self.real[2](x, *args, **kw)

        thresha.np_pseudorandom_share, thresha.np_pseudorandom_share_0, mpc.output = take('r'), take('z'), output
        return self

    def __exit__(self, *exc):
        thresha.np_pseudorandom_share, thresha.np_pseudorandom_share_0, mpc.output = self.real
        assert exc[0] is not None or not self.queue, 'draws left over'


async def main():
    rng = random.Random(20261020)
    await mpc.start()
    assert len(mpc.parties) == 1 and not mpc.options.no_prss
    doc = {'source': 'mpyc.runtime.np_random_bits, PRSS branch, one party, planted draws; raw field elements', 'count': COUNT,
           'fields': []}
    default = mpc.options.sec_param
    for name, p in PRIMES.items():
        if p is None:
            p = mpc.SecFxp().field.modulus
        assert (p % 4 == 1) == (name == 'pm64-gen')
        mpc.options.sec_param = 8                       # (only so that SecFxp(14, 16) fits the 40-bit prime)
        secfxp = mpc.SecFxp(14, 16, p=p)
        mpc.options.sec_param = default
        field = secfxp.field
        entry = {'name': name, 'p': p, 'cases': []}
        for case, plan in CASES.items():
            rounds = rounds_of(rng, p, plan)
            rec = {'case': case, 'rounds': [{'r': r, 'z': z} for r, z in rounds], 'bits': []}
            for signed in (False, True):
                for f in (0, 16):
                    with Planted(rounds) as pl:
                        x = mpc.np_random_bits(secfxp if f else field, COUNT, signed=signed)
                        vals = await mpc.gather(x)
                    vals = [int(v) % p for v in vals.value]
                    unit = (1 << f) % p
                    assert set(vals) <= ({unit, p - unit} if signed else {0, unit}), (name, case, signed, f)
                    assert pl.opened == [[(a * a + b) % p for a, b in zip(r, z)] for r, z in rounds]
                    rec.setdefault('opened', pl.opened)
                    rec['bits'].append({'signed': signed, 'f': f, 'values': vals})
            entry['cases'].append(rec)
        doc['fields'].append(entry)
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'rbits.json'), 'w') as fh:
        json.dump(doc, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
