#!/usr/bin/env python3
"""Generate tests/golden/unit/unit.json from the REAL reference (lschoe/mpyc, pure Python): unit vectors of secret indices and
a table read through them, one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_unit.py --no-log

Over SecInt(32), for every K in KS and every index a in [0, K):
  np_unit     the opened runtime.np_unit_vector(S(a), K), K entries;
  unit        the opened runtime.unit_vector(S(a), K), K entries;
  lookup      the opened T @ np_unit_vector(S(a), K) for the fixed random table T of the entry (`table`, K signed values).
Data only, 20 KB.  The fixture has a directory of its own, as tests/golden/bsgn has.
"""
import json
import os
import random

import numpy as np

from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'unit')
KS = (1, 2, 3, 5, 8, 13, 64)


async def main():
    secint = mpc.SecInt(32)
    rng = random.Random(20261020)
    doc = {'source': 'runtime.np_unit_vector, runtime.unit_vector and T @ np_unit_vector of the reference, one party, SecInt(32)',
           'p': int(secint.field.modulus), 'unit': []}
    await mpc.start()
    for K in KS:
        table = [rng.randrange(-2**20, 2**20) for _ in range(K)]
        T = np.array(table)
        e = {'K': K, 'table': table, 'np_unit': [], 'unit': [], 'lookup': []}
        for a in range(K):
            u = mpc.np_unit_vector(secint(a), K)
            e['np_unit'].append([int(v) for v in np.asarray(await mpc.output(u)).reshape(-1)])
            e['unit'].append([int(v) for v in await mpc.output(mpc.unit_vector(secint(a), K))])
            e['lookup'].append(int(await mpc.output(mpc.np_sum(u * T))))
        doc['unit'].append(e)
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'unit.json'), 'w') as fh:
        json.dump(doc, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
