#!/usr/bin/env python3
"""Device time of the two ends of a compare-exchange stage of the sorting network (ffgpu_cx_diff, ffgpu_cx_apply with 3 and
7 sub-share rows) per stage class -- long runs (p >= 64), short runs (p = 1, 2, 4 with d = p), short runs with a large d --
against (a) the same step composed from the calls that existed before (index_select x 2, ffgpu_sub; index_select x 2,
ffgpu_recombine, ffgpu_add, ffgpu_sub, index_copy_ x 2; the index tensors are built before the clock starts, which
favours the composition; both routes issued from Python, `launches` calls per timed interval) and (b) the library's copy yardstick (ffgpu_time_copy) moving the same algorithmic bytes
(diff: 2 P eb read + P eb written; apply: (nrows + 2) P eb read + 2 P eb written), in alternating runs by device events -- the kernel for this
ratio replayed from a captured graph, so that neither side pays a host launch path --,
with a byte comparison of both routes.  --protocol instead times one protocols.sort (all parties on one GPU) and splits
its wall time into the comparison, the multiplication's share generation and the two kernels.

One field per process keeps a step short; run the fields as separate steps, each under its own time limit:
    timeout -k 10 300 python tools/sort_probe.py --fields p64 --out out/sort_p64.json && \\
    timeout -k 10 300 python tools/sort_probe.py --fields p80 --out out/sort_p80.json && \\
    timeout -k 10 300 python tools/sort_probe.py --fields p136 --out out/sort_p136.json && \\
    timeout -k 10 300 python tools/sort_probe.py --protocol --out out/sort_protocol.json
usage: sort_probe.py [--out FILE.json] [--reps N] [--fields p64,p80,p136] [--shapes 1x1048576x1,1x1024x1024]
                     [--launches N] [--classes REGEX] [--protocol [--k K]]"""
import argparse
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch         # noqa: E402

FIELDS = {'p64': 2**64 - 189, 'p80': 2**80 - 65, 'p136': 2**136 - 113}


def timed(fn, launches=1):
    """milliseconds per call of `launches` calls issued back to back between two events (a single call of a few
    microseconds would be timed by the host's launch path, not by the device)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches, r


def random_elements(ctx, count):
    """`count` canonical field elements on the device: random limbs through ffgpu_reduce"""
    from mpyc_amd.engine import DevArray, _torch_dtype
    eb = ctx.elem_bytes
    raw = torch.randint(-2**63, 2**63 - 1, ((count * eb + 7) // 8,), dtype=torch.int64, device='cuda')
    raw = raw.view(torch.uint8)[:count * eb].view(_torch_dtype(eb))
    return ctx.reduce(DevArray(ctx, raw.reshape((count, ctx.limbs) if ctx.limbs else (count,)), count))


def stage_classes(k):
    top = 1 << ((k - 1).bit_length() - 1)
    out = [('long p=%d d=p' % top, top, top, 0), ('long p=64 d=%d' % (top - 64), 64, top - 64, 64)]
    out += [('short p=%d d=p' % p, p, p, 0) for p in (1, 2, 4)]
    out += [('short p=%d d=%d' % (p, top - p), p, top - p, p) for p in (1, 2, 4)]
    return out


class Composed:
    """one stage from the calls that existed before the two kernels"""

    def __init__(self, ctx, outer, k, inner, p, d, r):
        from mpyc_amd.engine import DevArray
        self.ctx, self.DevArray, self.shape = ctx, DevArray, (outer, k, inner)
        i = torch.arange(k - d, device='cuda')
        self.lo = i[(i & p) == r]
        self.hi = self.lo + d
        self.P = int(self.lo.shape[0])

    def cube(self, a):
        return a.t.reshape(self.shape + tuple(a.t.shape[1:]))

    def gather(self, a, idx):
        t = self.cube(a).index_select(1, idx)
        c = self.shape[0] * self.P * self.shape[2]
        return self.DevArray(self.ctx, t.reshape((c,) + tuple(a.t.shape[1:])), c)

    def diff(self, a):
        return self.ctx.sub(self.gather(a, self.hi), self.gather(a, self.lo))

    def apply(self, a, rows, lam):
        ctx = self.ctx
        b0, b1 = self.gather(a, self.lo), self.gather(a, self.hi)
        h = ctx.recombine(rows, lam)
        tail = tuple(a.t.shape[1:])
        shp = (self.shape[0], self.P, self.shape[2]) + tail
        cube = self.cube(a)
        cube.index_copy_(1, self.lo, ctx.add(b0, h).t.reshape(shp))
        cube.index_copy_(1, self.hi, ctx.sub(b1, h).t.reshape(shp))
        return a


def probe_kernels(args):
    from mpyc_amd.engine import CapturedLaunches, FieldContext
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'launches_per_interval': args.launches, 'cells': []}
    for name in args.fields.split(','):
        p_ = FIELDS[name]
        ctx = FieldContext(p_, device=0)
        eb = ctx.elem_bytes
        for shape in args.shapes.split(','):
            outer, k, inner = (int(v) for v in shape.split('x'))
            n = outer * k * inner
            a = random_elements(ctx, n)
            rowbuf = [random_elements(ctx, n // 2) for _ in range(7)]
            lam = [int.from_bytes(os.urandom(32), 'little') % p_ for _ in range(7)]
            for label, p, d, r in stage_classes(k):
                if not re.search(args.classes, label):
                    continue
                comp = Composed(ctx, outer, k, inner, p, d, r)
                c = outer * comp.P * inner
                assert comp.P == ctx.cx_pairs(k, p, d, r)
                from mpyc_amd.engine import DevArray
                rows = [DevArray(ctx, x.t[:c], c) for x in rowbuf]
                steps = {'diff': (lambda: ctx.cx_diff(a, outer, k, inner, p, d, r), lambda: comp.diff(a), 3 * c)}
                for nr in (3, 7):
                    steps['apply nrows=%d' % nr] = (
                        lambda nr=nr: ctx.cx_apply(a, rows[:nr], lam[:nr], outer, k, inner, p, d, r),
                        lambda nr=nr: comp.apply(a, rows[:nr], lam[:nr]), (nr + 4) * c)
                for step, (new, old, elems) in steps.items():
                    nbytes = elems * eb
                    src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')   # a copy reads and writes: same bytes moved
                    dst = torch.empty_like(src)
                    # the same bytes from both routes, each from the same start
                    keep = a.t.clone()
                    r_old = old()
                    got_old = r_old.t.clone()
                    a.t.copy_(keep)
                    r_new = new()
                    same = bool(torch.equal(r_new.t.reshape(-1), got_old.reshape(-1)))
                    a.t.copy_(keep)
                    del r_old, r_new, got_old, keep
                    # the kernel alone: `launches` calls replayed from a captured graph, so that the host's launch path
                    # (about 10 us per call from Python, more than these kernels take) is not what the events see
                    cg = CapturedLaunches(lambda: [new() for _ in range(args.launches)][-1], warmup=1)
                    dev_ms = []
                    new_ms, old_ms, cp_ms = [], [], []
                    for rep in range(args.reps + 1):                                         # rep 0 warms every route up
                        ms, _ = timed(new, args.launches)
                        if rep:
                            new_ms.append(ms)
                        ms, _ = timed(old, args.launches)
                        if rep:
                            old_ms.append(ms)
                        ms, _ = timed(cg.replay)
                        if rep:
                            dev_ms.append(ms / args.launches)
                        ms = ctx.time_copy(src, dst, args.launches)
                        if rep:
                            cp_ms.append(ms)
                    nm, om, cm = statistics.median(new_ms), statistics.median(old_ms), statistics.median(cp_ms)
                    dm = statistics.median(dev_ms)
                    del cg
                    cell = {'field': name, 'elem_bytes': eb, 'shape': shape, 'class': label, 'pairs': comp.P, 'step': step,
                            'us': round(dm * 1e3, 2), 'issued_from_python_us': round(nm * 1e3, 1), 'algorithmic_bytes': nbytes,
                            'GBps': round(nbytes / dm / 1e6, 1), 'copy_us': round(cm * 1e3, 2), 'fraction_of_copy_rate': round(cm / dm, 3),
                            'composed_us': round(om * 1e3, 1), 'composed_over_kernel': round(om / nm, 2), 'same_bytes': same}
                    res['cells'].append(cell)
                    print(json.dumps(cell), flush=True)
                    if not same:
                        sys.exit('the two routes differ')
                    del src, dst
            del a, rowbuf
            torch.cuda.empty_cache()
    return res


def probe_protocol(args):
    """one protocols.sort at k = 1024, m = 3, t = 1, l = 32 over 2^64 - 189: wall time (host clock around a synchronised
    run) split by wrapping the context's methods -- comparison = everything inside compare_zero, multiplication = the
    share generation of [b1 < b0] (b1 - b0) (its recombination is inside cx_apply)"""
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext
    modulus, m, t, l, k = 2**64 - 189, 3, 1, 32, args.k
    ctx = FieldContext(modulus, device=0)
    F = finfields.GF(modulus)
    vals = torch.randint(-2**29, 2**29, (k,), dtype=torch.int64).tolist()
    sh = lambda v: protocols.share(ctx, ctx.from_ints([x % modulus for x in v]), t, m)
    xs = sh(vals)
    pool = {}

    def rand(count):                       # drawn once per size, outside the clock: the caller's randomness is an input
        if count not in pool:
            g = torch.Generator().manual_seed(count)
            bits = lambda c: torch.randint(0, 2, (c,), generator=g).tolist()
            pool[count] = (sh(bits(count * l)), sh(bits(count)), sh(torch.randint(0, 1 << 24, (count,), generator=g).tolist()),
                           sh(torch.randint(1, 1 << 62, (count,), generator=g).tolist()))
        return pool[count]

    spent = {'cx_diff': 0.0, 'cx_apply': 0.0, 'compare_zero': 0.0, 'mul split_rng': 0.0}
    inside = [0]

    def wrap(obj, name, key, outer_only=False):
        fn = getattr(obj, name)

        def w(*a, **kw):
            if inside[0] and not outer_only:
                return fn(*a, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if outer_only:
                inside[0] += 1
            try:
                r = fn(*a, **kw)
                torch.cuda.synchronize()
            finally:
                if outer_only:
                    inside[0] -= 1
            spent[key] += time.perf_counter() - t0
            return r
        setattr(obj, name, w)
        return fn

    res = {'device': torch.cuda.get_device_name(0), 'k': k, 'm': m, 't': t, 'l': l, 'modulus': '2^64-189'}
    for s in protocols.sort_stages(k):
        rand(ctx.cx_pairs(k, *s))
    out = protocols.sort(ctx, F, xs, 1, k, 1, t, l, rand)          # warm-up, and the check
    got = protocols.open_(ctx, F, out, t).to_ints()
    res['sorted'] = [v - modulus if v > modulus // 2 else v for v in got] == sorted(vals)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    protocols.sort(ctx, F, xs, 1, k, 1, t, l, rand)
    torch.cuda.synchronize()
    res['wall_ms_plain'] = round((time.perf_counter() - t0) * 1e3, 2)
    saved = [(ctx, 'cx_diff', wrap(ctx, 'cx_diff', 'cx_diff')), (ctx, 'cx_apply', wrap(ctx, 'cx_apply', 'cx_apply')),
             (ctx, 'split_rng', wrap(ctx, 'split_rng', 'mul split_rng')),
             (protocols, 'compare_zero', wrap(protocols, 'compare_zero', 'compare_zero', outer_only=True))]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    protocols.sort(ctx, F, xs, 1, k, 1, t, l, rand)
    torch.cuda.synchronize()
    res['wall_ms_with_a_sync_around_every_part'] = round((time.perf_counter() - t0) * 1e3, 2)
    for obj, name, fn in saved:
        setattr(obj, name, fn)
    res['parts_ms'] = {key: round(v * 1e3, 2) for key, v in spent.items()}
    res['stages'] = len(list(protocols.sort_stages(k)))
    print(json.dumps(res), flush=True)
    if not res['sorted']:
        sys.exit('the opened result is not sorted')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fields', default=','.join(FIELDS))
    ap.add_argument('--shapes', default='1x1048576x1,1x1024x1024')
    ap.add_argument('--launches', type=int, default=10, help='calls per timed interval')
    ap.add_argument('--classes', default='.', help='regex on the stage class label')
    ap.add_argument('--protocol', action='store_true')
    ap.add_argument('--k', type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    res = probe_protocol(args) if args.protocol else probe_kernels(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
