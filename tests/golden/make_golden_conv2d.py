#!/usr/bin/env python3
"""Generate tests/golden/conv2d/conv2d.json from the REAL reference (lschoe/mpyc, pure Python): the convolution layer of its
convolutional network demo, demos/np_cnnmnist.py, whose own convolvetensor and maxpool are called, one party, no logging.

Run where the reference is importable (it does not travel to the GPU box):

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_conv2d.py --no-log

The demo is loaded from the reference checkout by path (demos/ is no package); nothing of its text is copied.  Recorded, all
as signed RAW integers (a fixed-point number a is round(a 2^f)), tensors flat and row-major:
  conv    per case: the secure type, its prime p and f, (k, r, m, n, v, s), the inputs x (k, r, m, n), W (v, r, s, s), b (v) and
          the opened output y (k, v, m, n) of convolvetensor -- SecInt(37) at five shapes (odd and even s, s = n, m < s, a single
          element), SecFxp(10, 4) at the first two, where the output went through the reference's probabilistic truncation;
  layer   one whole layer under SecInt(37): convolvetensor -> maxpool -> (x >= 0) * x on (1, 2, 6, 6) with v = 2, s = 3: the
          inputs and the opened conv, pool and relu tensors.  The inputs are the first seeded draw for which the pooled tensor
          holds both signs and at least one 2 x 2 square whose maximum occurs twice (a tie).
Data only, a few KB.
"""
import importlib.util
import json
import os
import random

import numpy as np

import mpyc
from mpyc.runtime import mpc

OUT = os.environ.get('GOLDEN_OUT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv2d')
INT_SHAPES = [(2, 3, 5, 6, 2, 3), (1, 2, 4, 5, 3, 4), (1, 1, 3, 7, 1, 5), (1, 2, 2, 6, 2, 6), (1, 1, 1, 1, 1, 1)]
FXP_SHAPES = INT_SHAPES[:2]
LAYER_SHAPE = (1, 2, 6, 6, 2, 3)


def load_demo():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(mpyc.__file__))), 'demos', 'np_cnnmnist.py')
    spec = importlib.util.spec_from_file_location('np_cnnmnist', path)
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    return demo


def draw(rng, shape, bx, bw, bb):
    k, r, m, n, v, s = shape
    x = [rng.randint(-bx, bx) for _ in range(k * r * m * n)]
    W = [rng.randint(-bw, bw) for _ in range(v * r * s * s)]
    b = [rng.randint(-bb, bb) for _ in range(v)]
    return x, W, b


def secure(secnum, f, vals, shape):
    a = np.array(vals, dtype=object).reshape(shape)
    if f:
        return secnum.array(a.astype(float) / (1 << f), integral=False)
    return secnum.array(a)


async def raw(a, f):
    res = np.asarray(await mpc.output(a)).reshape(-1)
    out = [round(float(v) * (1 << f)) for v in res]
    assert all(abs(float(v) * (1 << f) - o) < 1e-9 for v, o in zip(res, out))
    return out


async def convolve(demo, secnum, f, shape, x, W, b):
    k, r, m, n, v, s = shape
    return demo.convolvetensor(secure(secnum, f, x, (k, r, m, n)), secure(secnum, f, W, (v, r, s, s)), secure(secnum, f, b, (v,)))


async def main():
    demo = load_demo()
    doc = {'source': 'demos/np_cnnmnist.py convolvetensor / maxpool of the reference, one party; signed raw integers, flat row-major',
           'conv': [], 'layer': None}
    await mpc.start()
    secint, secfxp = mpc.SecInt(37), mpc.SecFxp(10, 4)
    rng = random.Random(20261021)
    for secnum, f, shapes, bounds in ((secint, 0, INT_SHAPES, (1000, 300, 100000)), (secfxp, 4, FXP_SHAPES, (16, 8, 64))):
        for shape in shapes:
            x, W, b = draw(rng, shape, *bounds)
            y = await raw(await convolve(demo, secnum, f, shape, x, W, b), f)
            doc['conv'].append({'type': secnum.__name__, 'p': int(secnum.field.modulus), 'f': f, 'shape': list(shape), 'x': x, 'W': W,
                                'b': b, 'y': y})
    k, r, m, n, v, s = LAYER_SHAPE
    for seed in range(1000):
        lrng = random.Random(seed)
        x, W, b = draw(lrng, LAYER_SHAPE, 2, 1, 3)
        y = await convolve(demo, secint, 0, LAYER_SHAPE, x, W, b)
        conv = await raw(y, 0)
        pool = await raw(demo.maxpool(y), 0)
        c = np.array(conv).reshape(k * v, m // 2, 2, n // 2, 2)
        ties = sum(1 for pl in range(k * v) for I in range(m // 2) for J in range(n // 2)
                   if sorted(c[pl, I, :, J, :].reshape(-1))[-1] == sorted(c[pl, I, :, J, :].reshape(-1))[-2])
        if min(pool) < 0 < max(pool) and 0 in pool and ties:
            break
    else:
        raise SystemExit('no seed gives both signs and a tie')
    pooled = demo.maxpool(y)
    relu = await raw((pooled >= 0) * pooled, 0)
    assert relu == [max(q, 0) for q in pool]
    doc['layer'] = {'type': secint.__name__, 'p': int(secint.field.modulus), 'f': 0, 'shape': list(LAYER_SHAPE), 'seed': seed, 'x': x,
                    'W': W, 'b': b, 'conv': conv, 'pool': pool, 'relu': relu, 'ties': ties}
    await mpc.shutdown()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'conv2d.json'), 'w') as fh:
        json.dump(doc, fh, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    mpc.run(main())
