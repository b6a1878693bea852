#!/usr/bin/env python3
"""Generate tests/golden/keccak/keccak.json from the REAL reference (lschoe/mpyc, pure Python): its own demos/sha3.py
functions on bit strings whose length is no multiple of 8 (which hashlib cannot express), one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_keccak.py --no-log

  digests   sha3(M, 256, 512) and shake(M, 256, 256) of demos/sha3.py for random messages of 5, 30, 1605 and 1630 bits:
            message and the opened 256 output bits as strings of 0 / 1, in the demo's bit order;
  f1600     the opened keccak_f1600(S) of the zero state and of one random state, 1600 bits each.
Data only, a few KB.  The fixture has a directory of its own, as tests/golden/unit has.
"""
import importlib.util
import json
import os
import random

import numpy as np

import mpyc
from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'keccak')
LENGTHS = (5, 30, 1605, 1630)


def demo():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(mpyc.__file__))), 'demos', 'sha3.py')
    spec = importlib.util.spec_from_file_location('mpyc_demo_sha3', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bitstr(a):
    return ''.join(str(int(v)) for v in np.asarray(a).reshape(-1))


async def main():
    sha3 = demo()
    rng = random.Random(20261021)
    doc = {'source': 'demos/sha3.py of the reference: sha3(M, 256, 512), shake(M, 256, 256) and keccak_f1600(S), one party',
           'digests': [], 'f1600': []}
    await mpc.start()
    for nbits in LENGTHS:
        bits = [rng.randrange(2) for _ in range(nbits)]
        x = sha3.secfld.array(np.array(bits))
        e = {'nbits': nbits, 'message': bitstr(bits),
             'sha3_256': bitstr(await mpc.output(sha3.sha3(x, 256, 512))),
             'shake128_256': bitstr(await mpc.output(sha3.shake(x, 256, 256)))}
        doc['digests'].append(e)
    for state in ([0] * 1600, [rng.randrange(2) for _ in range(1600)]):
        S = sha3.secfld.array(np.array(state))
        doc['f1600'].append({'in': bitstr(state), 'out': bitstr(await mpc.output(sha3.keccak_f1600(S)))})
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'keccak.json'), 'w') as fh:
        json.dump(doc, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
