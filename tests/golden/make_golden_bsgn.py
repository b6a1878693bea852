#!/usr/bin/env python3
"""Generate tests/golden/bsgn/bsgn.json from the REAL reference (lschoe/mpyc, pure Python): the binary sign of its binarized
network demo, demos/np_bnnmnist.py, whose own bsgn_0 / bsgn_1 / bsgn_2 are called, one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_bsgn.py --no-log

The demo is loaded from the reference checkout by path (demos/ is no package); nothing of its text is copied.  Per variant
d = 0, 1, 2, over the prime the demo pairs it with (SecInt(14, p=...), np_bnnmnist.py:180-186):
  p      the modulus;
  B      the largest B <= 4096 for which the opened result is the sign (1 for a >= 0, else -1) for every |a| <= B;
  a      every integer in [-B - 8, B + 8], so the first wrong signs at |a| = B + 1 are part of the fixture;
  bsgn   the opened bsgn_d(a) as signed integers.
Data only, a few KB.  The fixture has a directory of its own, as tests/golden/iszero has.
"""
import importlib.util
import json
import os

import numpy as np

import mpyc
from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bsgn')
PRIMES = (3546374752298322551, 9409569905028393239, 15569949805843283171)
LIMIT = 4096
CHUNK = 512


def load_demo():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(mpyc.__file__))), 'demos', 'np_bnnmnist.py')
    spec = importlib.util.spec_from_file_location('np_bnnmnist', path)
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    return demo


async def opened(fn, secint, a):
    out = []
    for i in range(0, len(a), CHUNK):
        res = await mpc.output(fn(secint.array(np.array(a[i:i + CHUNK]))))
        out += [int(v) for v in np.asarray(res).reshape(-1)]
    return out


async def main():
    demo = load_demo()
    doc = {'source': 'demos/np_bnnmnist.py bsgn_0 / bsgn_1 / bsgn_2 of the reference, one party; signed integers', 'bsgn': []}
    await mpc.start()
    for d, p in enumerate(PRIMES):
        secint = mpc.SecInt(14, p=p)
        fn = getattr(demo, f'bsgn_{d}')
        B = -1
        while B < LIMIT:                                                            # the range, from the demo's own outputs
            step = list(range(B + 1, min(B + 1 + CHUNK, LIMIT + 1)))
            pos, neg = await opened(fn, secint, step), await opened(fn, secint, [-v for v in step])
            good = 0
            while good < len(step) and pos[good] == 1 and (step[good] == 0 or neg[good] == -1):
                good += 1
            B += good
            if good < len(step):
                break
        a = list(range(-B - 8, B + 9))
        got = await opened(fn, secint, a)
        assert all(v == (1 if x >= 0 else -1) for x, v in zip(a, got) if abs(x) <= B), d
        doc['bsgn'].append({'d': d, 'p': p, 'B': B, 'a': a, 'bsgn': got})
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'bsgn.json'), 'w') as fh:
        json.dump(doc, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
