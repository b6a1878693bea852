#!/usr/bin/env python3
"""Device time of the four ends of a tournament round (ffgpu_tour_diff, ffgpu_tour_select with 3 sub-share rows,
ffgpu_tour_unit_prod, ffgpu_tour_unit_expand with 3 rows) for one party at about 2^20 elements, per pairing and shape class
-- inner = 1 with a small k (argmax over ten classes: 104857 x 10 x 1), a large inner (1 x 1024 x 1024), outer = 1
(1 x 1048576 x 1) -- against (a) the same output composed from the calls the engine had before (diff: index_select x 2,
ffgpu_sub; select: index_select, ffgpu_recombine, ffgpu_add / _sub, cat with the bye; unit_prod: a contiguous copy of
u[:, n0:], ffgpu_mul; unit_expand: ffgpu_recombine, the copy of u[:, n0:], ffgpu_sub, cat and the Fortran-order
interleave, cat with u0; the index tensors are built before the clock starts, which favours the composition; both routes
issued from Python, `launches` calls per timed interval) and (b) the library's copy yardstick (ffgpu_time_copy) moving
the same algorithmic bytes, in alternating runs by device events -- the kernel for this ratio replayed from a captured
graph, so that neither side pays a host launch path --, with a byte comparison of both routes.  --protocol instead times
protocols.argmax and protocols.amax (all parties on one GPU) at (64, 10, 1) and (1, 1024, 1) and splits their wall time
into the comparison, the share generation and the four kernels.

One field per process keeps a step short; run the fields as separate steps, each under its own time limit:
    timeout -k 10 300 python tools/tour_probe.py --fields p61 --out out/tour_p61.json && \\
    timeout -k 10 300 python tools/tour_probe.py --fields p80 --out out/tour_p80.json && \\
    timeout -k 10 300 python tools/tour_probe.py --fields p136 --out out/tour_p136.json && \\
    timeout -k 10 300 python tools/tour_probe.py --protocol --out out/tour_protocol.json
usage: tour_probe.py [--out FILE.json] [--reps N] [--fields p61,p80,p136] [--shapes 104857x10x1,1x1024x1024,1x1048576x1]
                     [--launches N] [--protocol]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch         # noqa: E402

from sort_probe import random_elements, timed     # noqa: E402

FIELDS = {'p61': 2**61 - 1, 'p80': 2**80 - 65, 'p136': 2**136 - 113}
HALVES, ODD_EVEN = 0, 1
MODES = {'halves': HALVES, 'odd_even': ODD_EVEN}


class Composed:
    """one round from the calls that existed before the four kernels"""

    def __init__(self, ctx, outer, k, inner, mode):
        from mpyc_amd.engine import DevArray
        self.ctx, self.DevArray = ctx, DevArray
        self.outer, self.k, self.inner = outer, k, inner
        self.n0, self.h = k % 2, k // 2
        self.kc = self.h + self.n0
        pos = torch.arange(k, device='cuda')
        self.first, self.second = ((pos[self.n0:(k + 1) // 2], pos[(k + 1) // 2:]) if mode == HALVES
                                   else (pos[self.n0::2], pos[self.n0 + 1::2]))

    def cube(self, a, kk):
        return a.t.reshape((self.outer, kk, self.inner) + tuple(a.t.shape[1:]))

    def flat(self, t, count):
        return self.DevArray(self.ctx, t.reshape((count,) + tuple(t.shape[3:])), count)

    def gather(self, a, idx):
        return self.flat(self.cube(a, self.k).index_select(1, idx), self.outer * self.h * self.inner)

    def diff(self, a, neg):
        a1, a2 = self.gather(a, self.first), self.gather(a, self.second)
        return self.ctx.sub(a1, a2) if neg else self.ctx.sub(a2, a1)

    def select(self, a, rows, lam, neg):
        ctx = self.ctx
        a1, v = self.gather(a, self.first), ctx.recombine(rows, lam)
        m = ctx.sub(a1, v) if neg else ctx.add(a1, v)
        if not self.n0:
            return m
        t = torch.cat((self.cube(a, self.k)[:, :1], self.cube(m, self.h)), dim=1)
        return self.flat(t, self.outer * self.kc * self.inner)

    def body(self, u):
        return self.flat(self.cube(u, self.kc)[:, self.n0:].contiguous(), self.outer * self.h * self.inner)

    def unit_prod(self, u, c):
        return self.ctx.mul(self.body(u), c)

    def unit_expand(self, u, rows, lam):
        ctx = self.ctx
        v = ctx.recombine(rows, lam)
        lo = ctx.sub(self.body(u), v)
        # (u - v, v) side by side along a new axis after k: the reference's concatenation and order='F' reshape
        pair = torch.stack((self.cube(lo, self.h), self.cube(v, self.h)), dim=2)
        t = pair.reshape((self.outer, 2 * self.h, self.inner) + tuple(u.t.shape[1:]))
        if self.n0:
            t = torch.cat((self.cube(u, self.kc)[:, :1], t), dim=1)
        return self.flat(t, self.outer * self.k * self.inner)


def probe_kernels(args):
    from mpyc_amd.engine import CapturedLaunches, DevArray, FieldContext
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'launches_per_interval': args.launches, 'cells': []}
    nr = 3
    for name in args.fields.split(','):
        p_ = FIELDS[name]
        ctx = FieldContext(p_, device=0)
        eb = ctx.elem_bytes
        for shape in args.shapes.split(','):
            outer, k, inner = (int(v) for v in shape.split('x'))
            h, kc = k // 2, k // 2 + k % 2
            n, nh, c = outer * k * inner, outer * kc * inner, outer * h * inner
            a = random_elements(ctx, n)
            u = DevArray(ctx, a.t[:nh], nh)
            rows = [random_elements(ctx, c) for _ in range(nr)]
            lam = [int.from_bytes(os.urandom(32), 'little') % p_ for _ in range(nr)]
            bye = (k % 2) * outer * inner
            steps = []                   # (label, mode label, kernel route, composed route, algorithmic elements moved)
            for mlabel, mode in MODES.items():
                comp = Composed(ctx, outer, k, inner, mode)
                steps.append(('diff', mlabel, lambda mode=mode: ctx.tour_diff(a, outer, k, inner, mode, True),
                              lambda comp=comp: comp.diff(a, True), 3 * c))
                steps.append(('select nrows=3', mlabel, lambda mode=mode: ctx.tour_select(a, rows, lam, outer, k, inner, mode, True),
                              lambda comp=comp: comp.select(a, rows, lam, True), (nr + 2) * c + 2 * bye))
            comp = Composed(ctx, outer, k, inner, ODD_EVEN)
            steps.append(('unit_prod', '-', lambda: ctx.tour_unit_prod(u, rows[0], outer, k, inner), lambda: comp.unit_prod(u, rows[0]), 3 * c))
            steps.append(('unit_expand nrows=3', '-', lambda: ctx.tour_unit_expand(u, rows, lam, outer, k, inner),
                          lambda: comp.unit_expand(u, rows, lam), (nr + 3) * c + 2 * bye))
            for step, mlabel, new, old, elems in steps:
                nbytes = elems * eb
                src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')   # a copy reads and writes: same bytes moved
                dst = torch.empty_like(src)
                same = bool(torch.equal(new().t.reshape(-1), old().t.reshape(-1)))
                # the kernel alone: `launches` calls replayed from a captured graph, so that the host's launch path is not
                # what the events see
                cg = CapturedLaunches(lambda: [new() for _ in range(args.launches)][-1], warmup=1)
                new_ms, old_ms, cp_ms, dev_ms = [], [], [], []
                for rep in range(args.reps + 1):                                         # rep 0 warms every route up
                    for fn, sink, launches, per in ((new, new_ms, args.launches, 1), (old, old_ms, args.launches, 1),
                                                    (cg.replay, dev_ms, 1, args.launches)):
                        ms, _ = timed(fn, launches)
                        if rep:
                            sink.append(ms / per)                                        # (a replay is `launches` kernels)
                    ms = ctx.time_copy(src, dst, args.launches)
                    if rep:
                        cp_ms.append(ms)
                nm, om, cm, dm = (statistics.median(x) for x in (new_ms, old_ms, cp_ms, dev_ms))
                del cg
                cell = {'field': name, 'elem_bytes': eb, 'shape': shape, 'mode': mlabel, 'step': step,
                        'us': round(dm * 1e3, 2), 'issued_from_python_us': round(nm * 1e3, 1), 'algorithmic_bytes': nbytes,
                        'GBps': round(nbytes / dm / 1e6, 1), 'copy_us': round(cm * 1e3, 2), 'fraction_of_copy_rate': round(cm / dm, 3),
                        'composed_us': round(om * 1e3, 1), 'composed_over_kernel': round(om / nm, 2),
                        'composed_over_kernel_device': round(om / dm, 2), 'same_bytes': same}
                res['cells'].append(cell)
                print(json.dumps(cell), flush=True)
                if not same:
                    sys.exit('the two routes differ')
                del src, dst
            del a, u, rows
            torch.cuda.empty_cache()
    return res


def probe_protocol(args):
    """protocols.argmax and protocols.amax at (64, 10, 1) and (1, 1024, 1), m = 3, t = 1, l = 32 over 2^64 - 189: wall
    time (host clock around a synchronised run) split by wrapping the context's methods -- comparison = everything inside
    compare_zero, share generation = split_rng outside it (the products' recombination is inside the kernels)"""
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext
    modulus, m, t, l = 2**64 - 189, 3, 1, 32
    ctx = FieldContext(modulus, device=0)
    F = finfields.GF(modulus)
    sh = lambda v: protocols.share(ctx, ctx.from_ints([x % modulus for x in v]), t, m)
    pool = {}

    def rand(count):                       # drawn once per size, outside the clock: the caller's randomness is an input
        if count not in pool:
            g = torch.Generator().manual_seed(count)
            bits = lambda c: torch.randint(0, 2, (c,), generator=g).tolist()
            pool[count] = (sh(bits(count * l)), sh(bits(count)), sh(torch.randint(0, 1 << 24, (count,), generator=g).tolist()),
                           sh(torch.randint(1, 1 << 62, (count,), generator=g).tolist()))
        return pool[count]

    kernels = ('tour_diff', 'tour_select', 'tour_unit_prod', 'tour_unit_expand')
    res = {'device': torch.cuda.get_device_name(0), 'm': m, 't': t, 'l': l, 'modulus': '2^64-189', 'runs': []}
    for outer, k, inner in ((64, 10, 1), (1, 1024, 1)):
        vals = torch.randint(-2**29, 2**29, (outer, k, inner), dtype=torch.int64)
        xs = sh(vals.reshape(-1).tolist())
        signed = lambda v: v - modulus if v > modulus // 2 else v
        for fname in ('argmax', 'amax'):
            fn = getattr(protocols, fname)
            run = lambda: fn(ctx, F, xs, outer, k, inner, t, l, rand)
            out = run()                                   # warm-up, fills the pool, and the check
            if fname == 'argmax':
                idx = [signed(v) for v in protocols.open_(ctx, F, protocols.arg_index(ctx, out[0], outer, k, inner), t).to_ints()]
                ok = idx == vals.argmax(dim=1).reshape(-1).tolist()
            else:
                ok = [signed(v) for v in protocols.open_(ctx, F, out, t).to_ints()] == vals.amax(dim=1).reshape(-1).tolist()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            plain = (time.perf_counter() - t0) * 1e3
            spent = dict.fromkeys(kernels + ('compare_zero', 'split_rng'), 0.0)
            inside = [0]

            def wrap(obj, name, outer_only=False):
                orig = getattr(obj, name)

                def w(*a, **kw):
                    if inside[0] and not outer_only:
                        return orig(*a, **kw)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    inside[0] += outer_only
                    try:
                        r = orig(*a, **kw)
                        torch.cuda.synchronize()
                    finally:
                        inside[0] -= outer_only
                    spent[name] += time.perf_counter() - t1
                    return r
                setattr(obj, name, w)
                return obj, name, orig

            saved = [wrap(ctx, name) for name in kernels + ('split_rng',)] + [wrap(protocols, 'compare_zero', outer_only=True)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            synced = (time.perf_counter() - t0) * 1e3
            for obj, name, orig in saved:
                if obj is ctx:
                    delattr(obj, name)                    # (the wrapper was an instance attribute over the class's method)
                else:
                    setattr(obj, name, orig)
            cell = {'protocol': fname, 'shape': [outer, k, inner], 'correct': ok, 'wall_ms_plain': round(plain, 2),
                    'wall_ms_with_a_sync_around_every_part': round(synced, 2),
                    'parts_ms': {key: round(v * 1e3, 2) for key, v in spent.items()},
                    'comparison_share': round(spent['compare_zero'] * 1e3 / synced, 3)}
            res['runs'].append(cell)
            print(json.dumps(cell), flush=True)
            if not ok:
                sys.exit('the opened result is wrong')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fields', default=','.join(FIELDS))
    ap.add_argument('--shapes', default='104857x10x1,1x1024x1024,1x1048576x1')
    ap.add_argument('--launches', type=int, default=10, help='calls per timed interval')
    ap.add_argument('--protocol', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    res = probe_protocol(args) if args.protocol else probe_kernels(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
