#!/usr/bin/env python3
"""Generate tests/golden/bits/to_bits.json from the REAL reference (lschoe/mpyc, pure Python): runtime.np_to_bits
(runtime.py:4391-4456) on SecInt(16) and SecInt(32) arrays, one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_bits.py --no-log

Per bit length l: about 40 input values (both extremes, -1, 0, 1, random values) and the l bits of each that the
reference's protocol returns, least significant first.  Data only, a few KB.  The fixture has a directory of its own:
tests/golden/*.json are the files make_golden.py writes (tests/test_wire.py compares the two lists).
"""
import json
import os
import random

import numpy as np

from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bits')     # GOLDEN_OUT: regenerate elsewhere


def values(rng, l, count=40):
    lo, hi = -(1 << (l - 1)), (1 << (l - 1)) - 1
    vals = [lo, hi, -1, 0, 1, lo + 1, hi - 1, 2, -2]
    return vals + [rng.randint(lo, hi) for _ in range(count - len(vals))]


async def main():
    rng = random.Random(20261018)
    out = {'source': 'mpyc.runtime.np_to_bits, one party', 'cases': []}
    await mpc.start()
    for l in (16, 32):
        secint = mpc.SecInt(l)
        vals = values(rng, l)
        a = secint.array(np.array(vals))
        bits = await mpc.output(mpc.np_to_bits(a))
        bits = [[int(b) for b in row] for row in bits.tolist()]
        assert len(bits) == len(vals) and all(len(row) == l for row in bits)
        for v, row in zip(vals, bits):
            assert sum(b << k for k, b in enumerate(row)) == v % (1 << l)
        out['cases'].append({'l': l, 'values': vals, 'bits': bits})
    await mpc.shutdown()
    with open(os.path.join(OUT, 'to_bits.json'), 'w') as fh:
        json.dump(out, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
