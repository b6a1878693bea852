#!/usr/bin/env python3
"""The four fixed-point kernels (ffgpu_trunc_mask, ffgpu_trunc_finish and ffgpu_norm_apply with 3 rows, ffgpu_norm_prod) for one
party at n = 10^6 over the 80-bit prime 2^80 - 65 (f = 16, l = 32) and over 2^61 - 1 (f = 8, l = 16), with two siblings timed in
the same run on the same shapes (ffgpu_bits_mask on the n*f bit shares, ffgpu_tour_select with the same 3 rows); after each
kernel's launches the library's copy yardstick (ffgpu_time_copy, k_copy16) moves the bytes the kernel must move by its map in
include/ffgpu.h.  A driver for ONE kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o fxp -- python tools/fxp_probe.py
    python tools/fxp_probe.py --summarize OUT/<...>/fxp_kernel_trace.csv

--summarize splits the trace into the stretches of one kernel name in launch order and prints the median duration of every
stretch, after its warm-up launches, next to the bytes and the copy of the same bytes that follows it.  Without a profiler the
driver prints the same rows timed by device events.

--protocol instead times protocols.trunc, fxp_multiply and reciprocal (all parties on one GPU, m = 3, t = 1) at n = 10^6 over
both fields: wall time of a synchronised run with the randomness drawn beforehand, and the opened values checked (the
truncation lies in {floor, floor + 1}; the reciprocal's largest relative error is printed).
usage: fxp_probe.py [--launches N] [--n N] [--protocol] [--summarize kernel_trace.csv]"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = [('2^80-65', 2**80 - 65, 32, 16), ('2^61-1', 2**61 - 1, 16, 8)]
WARM = 2
NR = 3
KERNELS = ('trunc_mask', 'bits_mask', 'trunc_finish', 'tour_select', 'norm_prod', 'norm_apply')


def steps_of(n, l, f, eb):
    """(label, algorithmic bytes) by the maps: the mask reads a, rdivf and the n*f bit shares and writes ar and masked (the
    sibling bits_mask: one output); the finish reads the rows and ar and writes out (tour_select over (n/2, 2, 1): the same rows,
    one more input element per output); norm_prod reads every bit once and writes the compact products and the signs;
    norm_apply reads the sign bits and the rows and writes the dense array"""
    c = n * (l - 1)
    return [('trunc_mask', (n * f + 4 * n) * eb), ('bits_mask', (n * f + 3 * n) * eb), ('trunc_finish', (NR * n + 2 * n) * eb),
            ('tour_select', (NR * n + 2 * n) * eb), ('norm_prod', (n * l + c + n) * eb), ('norm_apply', (n + NR * c + c) * eb)]


def drive(args):
    import torch
    from mpyc_amd.engine import FieldContext
    from sort_probe import random_elements, timed
    n = args.n
    for name, p, l, f in FIELDS:
        ctx = FieldContext(p, device=0)
        eb = ctx.elem_bytes
        a, rd, rb, bits = (random_elements(ctx, k) for k in (n, n, n * f, n * l))
        rows1 = [random_elements(ctx, n) for _ in range(NR)]
        rows2 = [random_elements(ctx, n * (l - 1)) for _ in range(NR)]
        lam = [int.from_bytes(os.urandom(32), 'little') % p for _ in range(NR)]
        o1, o2, oc, half = ctx.empty(n), ctx.empty(n), ctx.empty(n * (l - 1)), ctx.empty(n)
        lvl = random_elements(ctx, 2 * n)                      # tour_select over (n, 2, 1): n pairs, the rows' length
        calls = {'trunc_mask': lambda: ctx.trunc_mask(a, rb, rd, f, 1 << (l + f - 1), ar_out=o1, out=o2),
                 'bits_mask': lambda: ctx.bits_mask(a, rb, rd, f, 1 << f, out=o2),
                 'trunc_finish': lambda: ctx.trunc_finish(rows1, lam, a, f, out=o1),
                 'tour_select': lambda: ctx.tour_select(lvl, rows1, lam, n, 2, 1, ctx.TOUR_ODD_EVEN, out=half),
                 'norm_prod': lambda: ctx.norm_prod(bits, l, out=oc, sign_out=o1),
                 'norm_apply': lambda: ctx.norm_apply(bits, rows2, lam, l, out=oc)}
        for label, nbytes in steps_of(n, l, f, eb):
            src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')       # a copy reads and writes: same bytes moved
            dst = torch.empty_like(src)
            timed(calls[label], WARM)
            ms, _ = timed(calls[label], args.launches)
            ctx.time_copy(src, dst, WARM)
            cp = ctx.time_copy(src, dst, args.launches)
            print(json.dumps({'field': name, 'l': l, 'f': f, 'n': n, 'kernel': label, 'bytes': nbytes, 'event_us': round(ms * 1e3, 1),
                              'event_GBps': round(nbytes / ms / 1e6), 'copy_us': round(cp * 1e3, 1),
                              'fraction_of_copy_rate': round(cp / ms, 3)}), flush=True)
            del src, dst
        del a, rd, rb, bits, rows1, rows2, o1, o2, oc, half, lvl
        torch.cuda.empty_cache()


def summarize(args):
    rows = sorted(csv.DictReader(open(args.summarize)), key=lambda r: int(r['Start_Timestamp']))
    name = lambda r: (re.search(r'\bk_\w+', r['Kernel_Name']) or re.match('', '')).group(0)
    mine = {'k_' + k for k in KERNELS} | {'k_copy16'}
    rows = [r for r in rows if name(r) in mine]
    runs = []                                           # stretches of one kernel name
    for r in rows:
        if not runs or runs[-1][0] != name(r):
            runs.append((name(r), []))
        runs[-1][1].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    labels = [(fname, label, nbytes) for fname, p, l, f in FIELDS
              for label, nbytes in steps_of(args.n, l, f, {80: 12, 61: 8}[p.bit_length()])]
    assert len(runs) == 2 * len(labels) and all(runs[2 * i][0] == 'k_' + l[1] and runs[2 * i + 1][0] == 'k_copy16' for i, l in enumerate(labels)), \
        [(n, len(d)) for n, d in runs]
    print('| field | kernel | bytes by the map | kernel us | GB/s | copy of the same bytes us | fraction of the copy rate |')
    print('|---|---|---|---|---|---|---|')
    for i, (fname, label, nbytes) in enumerate(labels):
        k_us, c_us = statistics.median(runs[2 * i][1][WARM:]), statistics.median(runs[2 * i + 1][1][WARM:])
        print(f'| {fname} | `k_{label}` | {nbytes} | {k_us:.1f} | {nbytes / k_us / 1e3:.0f} | {c_us:.1f} | {c_us / k_us:.2f} |')


def small(ctx, t):
    """non-negative integers below 2^31 (an int64 tensor on the device) as field elements"""
    import torch
    from mpyc_amd.engine import DevArray, _torch_dtype
    n = t.shape[0]
    if not ctx.limbs:
        return DevArray(ctx, t.to(_torch_dtype(ctx.elem_bytes)), n)
    x = torch.zeros((n, ctx.limbs), dtype=_torch_dtype(ctx.elem_bytes), device='cuda')
    x[:, 0] = t.to(x.dtype)
    return DevArray(ctx, x, n)


def low(x):
    """the low limb of opened values that are known to be small and non-negative"""
    t = x.t if x.t.dim() == 1 else x.t[:, 0]
    return t.to('cuda').to(__import__('torch').int64)


def protocol(args):
    import torch
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext
    m, t, n = 3, 1, args.n
    for name, p, l, f in FIELDS:
        ctx = FieldContext(p, device=0)
        F = finfields.GF(p)
        g = torch.Generator(device='cuda').manual_seed(l)
        ri = lambda lo, hi, k: torch.randint(lo, hi, (k,), generator=g, device='cuda', dtype=torch.int64)
        sh = lambda v: protocols.share(ctx, small(ctx, v), t, m)
        theta = 2 if f == 8 else 3                          # ceil(log2((f+1)/3.54))
        pool_t = [(sh(ri(0, 2, n * f)), sh(ri(0, 1 << 16, n))) for _ in range(2 + 2 * theta)]
        pool_b = (sh(ri(0, 2, n * l)), sh(ri(0, 1 << 16, n)))
        den = ri(1 << (2 * f - l + 2), 1 << (l - 2), n)      # positive, representable reciprocals
        oth = ri(0, 1 << ((l + f - 2) // 2), n)
        xs, ys = sh(den), sh(oth)
        it = [iter(())]
        rand_trunc = lambda count, f_: next(it[0])
        rand_bits = lambda count, l_: pool_b

        def run(fn):
            it[0] = iter(pool_t)
            return fn()
        calls = {'trunc': lambda: protocols.trunc(ctx, F, xs, pool_t[0][0], pool_t[0][1], t, f, l),
                 'fxp_multiply': lambda: protocols.fxp_multiply(ctx, F, ys, ys, t, f, l, rand_trunc),
                 'reciprocal': lambda: protocols.reciprocal(ctx, F, xs, t, l, f, rand_bits, rand_trunc)}
        for label, fn in calls.items():
            got = low(protocols.open_(ctx, F, run(fn), t))                                  # warm-up, and the check
            if label == 'trunc':
                ok, note = bool((((got - (den >> f)) >= 0) & ((got - (den >> f)) <= 1)).all()), {}
            elif label == 'fxp_multiply':
                ok, note = bool((((got - ((oth * oth) >> f)) >= 0) & ((got - ((oth * oth) >> f)) <= 1)).all()), {}
            else:
                want = (1 << (2 * f)) / den.double()
                err = (got.double() - want).abs()
                big = want >= (1 << f)                       # (below 1.0 a unit of 2^-f is a large relative step)
                rel = (err[big] / want[big]).max().item()
                ok, note = bool((err <= 2 + want * 2.0 ** -(f - 4)).all()), {'largest_relative_error_of_values_from_1': rel,
                                                                             'largest_error_units': err.max().item()}
            ms = []
            for _ in range(args.launches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(fn)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps(dict({'protocol': label, 'field': name, 'l': l, 'f': f, 'n': n, 'm': m, 't': t, 'correct': ok,
                                   'wall_ms_median': round(statistics.median(ms), 2), 'wall_ms_min': round(min(ms), 2)}, **note)),
                  flush=True)
            if not ok:
                sys.exit('the opened result is wrong')
        del pool_t, pool_b, xs, ys
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=10, help='timed launches per kernel (after 2 warm-up launches)')
    ap.add_argument('--n', type=int, default=10**6)
    ap.add_argument('--protocol', action='store_true')
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    protocol(args) if args.protocol else drive(args)


if __name__ == '__main__':
    main()
