#!/usr/bin/env python3
"""Device time of prefix scans and axis reductions on field arrays: the scan kernels (FieldContext.scan / .axis_reduce)
against the composed routes they replace (finfields._scan_hillis_steele, FieldArray._prod_halving,
FieldArray._sum_axis_composed / FieldContext.sum), in alternating runs by device events, with the library's copy kernel
(k_copy16, ffgpu_copy) over the same byte count beside every cell.  Per cell: median time of both routes, their ratio,
peak bytes of both, whether the results are the same bytes, and the fraction of the copy rate the kernels reach against
the cell's floor (2 eb n for the column walk and single-tile rows, 3 eb n for multi-tile rows, (n + n / k) eb for
reductions).
usage: scan_probe.py [--out FILE.json] [--reps N] [--fields p61,p80,p128,p136,gf64,gf8] [--shapes flat,sgn33,...]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

FIELDS = {'p61': (2**61 - 1, False), 'p80': (2**80 - 65, False), 'p128': (2**128 - 173, False),
          'p136': (2**136 - 113, False), 'gf64': (0x1000000000000001b, True), 'gf8': (0x11b, True)}
SHAPES = {'flat': ((10**7,), 0), 'sgn33': ((33, 10**6), 0), 'sgn65': ((65, 10**6), 0), 'rows16': ((10**6, 16), 1),
          'rows4': ((4, 2500000), 1), 'middle': ((1000, 100, 100), 1),
          # many rows reduced along the LAST axis with k > 16 (the composed sum is matrix x ones(k) with no permuted copy)
          'last100': ((10**5, 100), 1), 'last1000': ((10**4, 1000), 1), 'last10k': ((1000, 10**4), 1),
          # three strided lines (row tiles with an element stride of 3), and a 2^22-element column shape
          'strided': ((10**6, 3), 0), 'cols22': ((64, 65536), 0)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def dev_of(r):
    return r._dev if hasattr(r, '_dev') else r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--fields', default=','.join(FIELDS))
    ap.add_argument('--shapes', default=','.join(SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from mpyc_amd import finfields as gff, gfpx
    from mpyc_amd.engine import _torch_dtype
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'cells': []}
    for name in args.fields.split(','):
        modulus, binary = FIELDS[name]
        F = gff.GF(gfpx.BinaryPolynomial(modulus)) if binary else gff.GF(modulus)
        ctx = gff._context(F)
        eb = ctx.elem_bytes
        for sname in args.shapes.split(','):
            shape, axis = SHAPES[sname]
            n = int(np.prod(shape))
            raw = torch.randint(-2**63, 2**63 - 1, ((n * eb + 7) // 8,), dtype=torch.int64, device='cuda')
            raw = raw.view(torch.uint8)[:n * eb].view(_torch_dtype(eb))
            a = F.array(gff.DevArray(ctx, raw.reshape((n, ctx.limbs) if ctx.limbs else (n,)), n)).reshape(shape)   # (the ctor reduces)
            del raw
            outer, k, inner = gff._axis_geometry(shape, axis)
            multi_tile = ctx._L.ffgpu_scan_workspace_bytes(ctx._h, outer, k, inner) > 0
            src = torch.empty(n * eb, dtype=torch.uint8, device='cuda')
            dst = torch.empty_like(src)
            for kind in ('scan', 'reduce'):
                for mul in (False, True):
                    if kind == 'scan':
                        new = lambda: ctx.scan(a._dev, outer, k, inner, mul=mul)
                        old = lambda: gff._scan_hillis_steele(a, axis, mul)
                        floor = (3 if multi_tile else 2) * eb * n
                    else:
                        new = lambda: ctx.axis_reduce(a._dev, outer, k, inner, mul=mul)
                        if mul:
                            old = lambda: a._prod_halving(axis if a.ndim > 1 else None)
                        elif a.ndim > 1:
                            old = lambda: a._sum_axis_composed(axis)
                        else:
                            old = lambda: ctx.sum(a._dev)
                        floor = (n + n // k) * eb
                    new_ms, old_ms, cp_ms, new_peak, old_peak, same = [], [], [], 0, 0, None
                    for rep in range(args.reps + 1):                     # rep 0 warms every route up
                        torch.cuda.synchronize()
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        ms, r_new = timed(new)
                        new_peak = max(new_peak, torch.cuda.max_memory_allocated() - base)
                        if rep:
                            new_ms.append(ms)
                        torch.cuda.reset_peak_memory_stats()
                        try:
                            ms, r_old = timed(old)
                        except (RuntimeError, ValueError, NotImplementedError) as exc:   # the composed route cannot do this cell
                            ms, r_old, same = float('nan'), None, f'composed route failed: {type(exc).__name__}'
                            torch.cuda.empty_cache()
                        old_peak = max(old_peak, torch.cuda.max_memory_allocated() - base)
                        if rep:
                            old_ms.append(ms)
                        elif r_old is None:
                            pass
                        elif isinstance(r_old, (gff.FieldArray, gff.DevArray)):
                            same = bool(torch.equal(dev_of(r_new).t.reshape(-1), dev_of(r_old).t.reshape(-1)))
                        else:                                            # a field element (flat product of the composed route)
                            same = dev_of(r_new).to_ints()[0] == int(r_old) % ((1 << 200) if binary else modulus)
                        del r_new, r_old
                        ms, _ = timed(lambda: ctx.copy(src, dst))
                        if rep:
                            cp_ms.append(ms)
                    nm, om, cm = statistics.median(new_ms), statistics.median(old_ms), statistics.median(cp_ms)
                    copy_rate = 2 * n * eb / cm                          # bytes per ms
                    cell = {'field': name, 'shape': sname, 'geometry': [outer, k, inner], 'kind': kind, 'op': 'mul' if mul else 'add',
                            'new_ms': round(nm, 4), 'composed_ms': round(om, 4), 'ratio': round(om / nm, 2), 'copy_ms': round(cm, 4),
                            'new_peak_bytes': new_peak, 'composed_peak_bytes': old_peak, 'same_bytes': same,
                            'floor_bytes': floor, 'fraction_of_copy_rate': round(floor / copy_rate / nm, 3)}
                    res['cells'].append(cell)
                    print(json.dumps(cell), flush=True)
            del a, src, dst
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
