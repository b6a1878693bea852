#!/usr/bin/env python3
"""The three ends of a round of the first-occurrence search (ffgpu_find_leaf_prod, ffgpu_find_leaf_apply with 3 sub-share rows,
ffgpu_find_prod) for one party over 2^61 - 1 with C = 2 components, the public leaf and flip = 1, at (10^6, 31, 1) and
(10^4, 31, 128); after each kernel's launches the library's copy yardstick (ffgpu_time_copy, k_copy16) moves the bytes the
kernel must move by its map in include/ffgpu.h.  A driver for ONE kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o find -- python tools/find_probe.py
    python tools/find_probe.py --summarize OUT/<...>/find_kernel_trace.csv

--summarize splits the trace into the stretches of one kernel name in launch order (the copy launches separate the three
kernels, the kernels separate the copies) and prints the median duration of every stretch, after its warm-up launches, next
to the bytes and the copy of the same bytes that follows it.  Without a profiler the driver prints the same rows timed by
device events.

--protocol instead times protocols.find (all parties on one GPU, m = 3, t = 1) at (10^6, 31, 1): wall time of a
synchronised run, and the opened indices compared with torch's.
usage: find_probe.py [--launches N] [--shapes 1000000x31x1,10000x31x128] [--protocol] [--summarize kernel_trace.csv]"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODULUS = 2**61 - 1
WARM = 2
C, NR, FLIP, VIRT = 2, 3, 1, 1


def steps_of(outer, k, inner, eb):
    """(label, algorithmic bytes) of the three kernels, by their maps: every bit once and the compact output; the first
    members, the rows and the next level; the stored next level once and its compact output"""
    kv = k + VIRT
    h, kc = kv // 2, kv // 2 + kv % 2
    n, c, nxt = outer * k * inner, outer * h * inner, outer * kc * inner
    c2 = outer * (kc // 2) * inner
    return [('find_leaf_prod', (n + C * c) * eb), ('find_leaf_apply', (c + kv % 2 * outer * inner + NR * C * c + C * nxt) * eb),
            ('find_prod', (C * nxt + C * c2) * eb)]


def drive(args):
    import torch
    from mpyc_amd.engine import FieldContext
    from sort_probe import random_elements, timed
    ctx = FieldContext(MODULUS, device=0)
    eb = ctx.elem_bytes
    for shape in args.shapes.split(','):
        outer, k, inner = (int(v) for v in shape.split('x'))
        kv = k + VIRT
        h, kc = kv // 2, kv // 2 + kv % 2
        bits = random_elements(ctx, outer * k * inner)
        rows = [random_elements(ctx, C * outer * h * inner) for _ in range(NR)]
        lam = [int.from_bytes(os.urandom(32), 'little') % MODULUS for _ in range(NR)]
        tab = ctx.find_table(k, list(range(k)), list(range(1, k + 1)), k)
        out_c, out_l = ctx.empty(C * outer * h * inner), ctx.empty(C * outer * kc * inner)
        out_p = ctx.empty(C * outer * (kc // 2) * inner)
        calls = {'find_leaf_prod': lambda: ctx.find_leaf_prod(bits, tab, outer, k, inner, C, FLIP, VIRT, out=out_c),
                 'find_leaf_apply': lambda: ctx.find_leaf_apply(bits, tab, rows, lam, outer, k, inner, C, FLIP, VIRT, out=out_l),
                 'find_prod': lambda: ctx.find_prod(out_l, outer, kc, inner, C, out=out_p)}
        for label, nbytes in steps_of(outer, k, inner, eb):
            src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')       # a copy reads and writes: same bytes moved
            dst = torch.empty_like(src)
            timed(calls[label], WARM)
            ms, _ = timed(calls[label], args.launches)
            ctx.time_copy(src, dst, WARM)
            cp = ctx.time_copy(src, dst, args.launches)
            print(json.dumps({'shape': shape, 'kernel': label, 'bytes': nbytes, 'event_us': round(ms * 1e3, 1),
                              'event_GBps': round(nbytes / ms / 1e6), 'copy_us': round(cp * 1e3, 1),
                              'fraction_of_copy_rate': round(cp / ms, 3)}), flush=True)
            del src, dst
        del bits, rows, out_c, out_l, out_p
        torch.cuda.empty_cache()


def summarize(args):
    rows = sorted(csv.DictReader(open(args.summarize)), key=lambda r: int(r['Start_Timestamp']))
    name = lambda r: (re.search(r'\bk_\w+', r['Kernel_Name']) or re.match('', '')).group(0)
    rows = [r for r in rows if name(r).startswith('k_find_') or name(r) == 'k_copy16']
    runs = []                                           # stretches of one kernel name
    for r in rows:
        if not runs or runs[-1][0] != name(r):
            runs.append((name(r), []))
        runs[-1][1].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    labels = [(shape, label, nbytes) for shape in args.shapes.split(',')
              for label, nbytes in steps_of(*(int(v) for v in shape.split('x')), 8)]
    assert len(runs) == 2 * len(labels) and all(runs[2 * i][0] == 'k_' + l[1] and runs[2 * i + 1][0] == 'k_copy16' for i, l in enumerate(labels)), \
        [(n, len(d)) for n, d in runs]
    print('| shape | kernel | bytes by the map | kernel us | GB/s | copy of the same bytes us | fraction of the copy rate |')
    print('|---|---|---|---|---|---|---|')
    for i, (shape, label, nbytes) in enumerate(labels):
        k_us, c_us = statistics.median(runs[2 * i][1][WARM:]), statistics.median(runs[2 * i + 1][1][WARM:])
        print(f'| {shape} | `k_{label}` | {nbytes} | {k_us:.1f} | {nbytes / k_us / 1e3:.0f} | {c_us:.1f} | {c_us / k_us:.2f} |')


def protocol(args):
    import torch
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import DevArray, FieldContext
    m, t = 3, 1
    outer, k, inner = 10**6, 31, 1
    ctx = FieldContext(MODULUS, device=0)
    F = finfields.GF(MODULUS)
    g = torch.Generator(device='cuda').manual_seed(31)
    plain = (torch.rand((outer, k), generator=g, device='cuda') < 0.9).to(torch.int64)      # mostly ones: late first zeros
    plain[0], plain[1] = 1, 0
    xs = protocols.share(ctx, DevArray(ctx, plain.reshape(-1).clone(), outer * k), t, m)
    run = lambda: protocols.find(ctx, F, xs, outer, k, inner, t)
    got = protocols.open_(ctx, F, run(), t).t.reshape(-1)                                     # warm-up, and the check
    hit = plain == 0
    want = torch.where(hit.any(dim=1), hit.to(torch.int64).argmax(dim=1), torch.full((outer,), k, device='cuda'))
    ok = bool(torch.equal(got.to(torch.int64), want))
    ms = []
    for _ in range(args.launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({'protocol': 'find', 'shape': [outer, k, inner], 'm': m, 't': t, 'rounds': k.bit_length(), 'correct': ok,
                      'wall_ms_median': round(statistics.median(ms), 2), 'wall_ms_min': round(min(ms), 2)}), flush=True)
    if not ok:
        sys.exit('the opened result is wrong')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=10, help='timed launches per kernel (after 2 warm-up launches)')
    ap.add_argument('--shapes', default='1000000x31x1,10000x31x128')
    ap.add_argument('--protocol', action='store_true')
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    protocol(args) if args.protocol else drive(args)


if __name__ == '__main__':
    main()
