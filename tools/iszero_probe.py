#!/usr/bin/env python3
"""The kernels of the Legendre zero test (include/ffgpu_math.h) on the device, timed by device events:

  ffgm_legendre_code at 3 10^7 symbols (k = 30, n = 10^6) over 2^61 - 1, 2^80 - 65 and 2^128 - 173 next to ffgpu_pow with the
  exponent (p - 1) / 2 at the same count in the same run, five passes each, alternating; the spread of a kernel is the
  largest minus the smallest of its five passes.  --pow-only times ffgpu_pow alone: with --tree DIR, a built copy of the parent
  commit, it gives the parent's number on the same box, which the new kernel is held against;
  ffgm_iszero_mask at k = 30, n = 10^6: time, its algorithmic bytes (4 k + 1) n elements over that time as a fraction of the
  HBM ceiling (8 TB/s) and of the library's copy yardstick moving the same bytes in the same run, and the same rows from the
  element-wise calls that existed before it (materialised broadcast of a, two products, scalar multiply, subtraction from
  one, addition), with a byte comparison of the two results.

--protocol instead times protocols.is_zero end to end at n = 10^6, k = 30, m = 3, t = 1 over 2^80 - 65, all parties on one
GPU, the randomness drawn beforehand: wall time of a synchronised run, its split by stage (device events around each stage of
a hand-staged run of the same calls), the opened result checked against the plain zero test; next to it
protocols.compare_zero(mode='eq') at l = 32 on the same inputs.
usage: iszero_probe.py [--passes N] [--n N] [--k K] [--pow-only [--tree DIR]] [--protocol]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FIELDS = [('2^61-1', 2**61 - 1), ('2^80-65', 2**80 - 65), ('2^128-173', 2**128 - 173)]
HBM_TBPS = 8.0
WARM = 2


def row(**kw):
    print(json.dumps(kw), flush=True)


def passes_of(fn, passes, launches=3):
    """`passes` timings (microseconds per call) of `launches` calls each, after warm-up"""
    from sort_probe import timed
    timed(fn, WARM)
    return [round(timed(fn, launches)[0] * 1e3, 1) for _ in range(passes)]


def stats(us):
    return {'us_median': statistics.median(us), 'us_min': min(us), 'us_max': max(us), 'spread_us': round(max(us) - min(us), 1), 'passes': us}


def drive(args):
    import torch
    from mpyc_amd.engine import DevArray, FieldContext
    from sort_probe import random_elements, timed
    n, k = args.n, args.k
    cnt = k * n
    for name, p in FIELDS:
        ctx = FieldContext(p, device=0)
        eb = ctx.elem_bytes
        x = random_elements(ctx, cnt)
        o = ctx.empty(cnt)
        e = (p - 1) // 2
        plain = lambda: ctx.pow(x, e, out=o)
        if args.pow_only:
            row(field=name, count=cnt, kernel='ffgpu_pow (p-1)/2', **stats(passes_of(plain, args.passes)))
            continue
        codes = torch.empty(cnt, dtype=torch.uint8, device='cuda')
        sym = lambda: ctx.legendre_code(x, out=codes)
        us_p, us_s = [], []
        timed(plain, WARM), timed(sym, WARM)
        for _ in range(args.passes):                                   # alternating
            us_p.append(round(timed(plain, 3)[0] * 1e3, 1))
            us_s.append(round(timed(sym, 3)[0] * 1e3, 1))
        # the same symbols from the powers
        zero = (x.t == 0) if x.t.dim() == 1 else (x.t == 0).all(1)
        one = (o.t == 1) if o.t.dim() == 1 else ((o.t[:, 0] == 1) & (o.t[:, 1:] == 0).all(1))
        want = torch.where(zero, torch.full_like(one, 2, dtype=torch.uint8), one.to(torch.uint8))
        row(field=name, count=cnt, kernel='ffgm_legendre_code', **stats(us_s), same_as_pow=bool(torch.equal(want, codes)),
            residues=int((codes == 1).sum()), ffgpu_pow_same_run=stats(us_p),
            ratio_to_pow_median=round(statistics.median(us_s) / statistics.median(us_p), 4))
        del codes, want
        # the mask against the composed calls
        a = DevArray(ctx, x.t[:n], n)
        r, z, u2 = x, random_elements(ctx, cnt), random_elements(ctx, cnt)
        out = o
        fused = lambda: ctx.iszero_mask(a, r, z, u2, k, out=out)
        t1, t2 = ctx.empty(cnt), ctx.empty(cnt)

        def composed():
            ab = DevArray(ctx, a.t.repeat((k, 1)) if a.t.dim() == 2 else a.t.repeat(k), cnt)      # the materialised broadcast
            ctx.mul(ab, r, out=t1)
            ctx.mul_scalar(z, 2, out=t2)
            ctx.rsub_scalar(t2, 1, out=t2)
            ctx.mul(t2, u2, out=t2)
            return ctx.add(t1, t2, out=t2)

        us_f, us_c = [], []
        timed(fused, WARM), timed(composed, WARM)
        for _ in range(args.passes):
            us_f.append(round(timed(fused, 3)[0] * 1e3, 1))
            us_c.append(round(timed(composed, 3)[0] * 1e3, 1))
        fused()
        same = bool(torch.equal(out.t, composed().t))
        nbytes = (4 * k + 1) * n * eb
        src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        ctx.time_copy(src, dst, WARM)
        cp = ctx.time_copy(src, dst, 5)
        med = statistics.median(us_f)
        row(field=name, n=n, k=k, kernel='ffgm_iszero_mask', algorithmic_bytes=nbytes, **stats(us_f), GBps=round(nbytes / med / 1e3),
            fraction_of_hbm_ceiling=round(nbytes / med / 1e6 / HBM_TBPS, 3), copy_same_bytes_us=round(cp * 1e3, 1),
            fraction_of_copy_rate=round(cp * 1e3 / med, 3), composed=stats(us_c), composed_over_fused=round(statistics.median(us_c) / med, 2),
            same_bytes_as_composed=same)
        del x, o, z, u2, t1, t2, src, dst
        torch.cuda.empty_cache()


def protocol(args):
    import torch
    from fxp_probe import low, small
    from sort_probe import random_elements, timed
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext
    m, t, n, k, l = 3, 1, args.n, args.k, 32
    name, p = FIELDS[1]
    ctx = FieldContext(p, device=0)
    F = finfields.GF(p)
    g = torch.Generator(device='cuda').manual_seed(k)
    ri = lambda lo, hi, count: torch.randint(lo, hi, (count,), generator=g, device='cuda', dtype=torch.int64)
    sh = lambda v: protocols.share(ctx, v, t, m)
    plain = ri(0, 1 << (l - 2), n) * ri(0, 2, n)                               # about half of them zero, below 2^(l-1)
    xs = sh(small(ctx, plain))
    cnt = k * n
    pool = (sh(small(ctx, ri(0, 2, cnt))), sh(random_elements(ctx, cnt)), sh(random_elements(ctx, cnt)))
    rand_zero = lambda count: pool
    rbits, rdivl = sh(small(ctx, ri(0, 2, n * l))), sh(small(ctx, ri(0, 1 << 16, n)))
    routes = {'is_zero k=%d' % k: lambda: protocols.is_zero(ctx, F, xs, t, k, rand_zero),
              'compare_zero eq l=%d' % l: lambda: protocols.compare_zero(ctx, F, xs, rbits, None, rdivl, None, t, l, mode='eq')}
    for label, fn in routes.items():
        got = low(protocols.open_(ctx, F, fn(), t))                            # warm-up, and the check
        wrong = int((got != (plain == 0).to(torch.int64)).sum())
        ms = []
        for _ in range(args.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        row(protocol=label, field=name, n=n, m=m, t=t, wrong_of_n=wrong, wall_ms_median=statistics.median(ms), wall_ms_min=min(ms),
            passes=ms)
        if wrong > 2:
            sys.exit('the opened result is wrong')
    # the stages of is_zero, one device-event window each
    z, r, s = pool
    split = {}

    def stage(label, fn):
        ms, res = timed(fn)
        split[label] = round(split.get(label, 0) + ms, 3)
        return res

    for _ in range(2):                                                         # (the second pass is the one reported)
        split.clear()
        u2 = stage('multiply(s, s): share generation + recombination', lambda: protocols.multiply(ctx, F, s, s, t))
        masked = stage('iszero_mask x 3', lambda: [ctx.iszero_mask(xs[i], r[i], z[i], u2[i], k) for i in range(2 * t + 1)])
        c = stage('open (recombine 3 rows)', lambda: protocols.open_(ctx, F, masked, t, degree=2 * t))
        code = stage('legendre_code x 1', lambda: ctx.legendre_code(c))
        fin = stage('iszero_finish x 3', lambda: [ctx.iszero_finish(code, z[i]) for i in range(m)])
        stage('prod_rows over k rows', lambda: protocols.prod_rows(ctx, F, fin, k, t))
    row(protocol='is_zero k=%d, split by stage (device ms)' % k, field=name, n=n, m=m, t=t, total_ms=round(sum(split.values()), 3), **split)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--n', type=int, default=10**6)
    ap.add_argument('--k', type=int, default=30)
    ap.add_argument('--pow-only', action='store_true')
    ap.add_argument('--protocol', action='store_true')
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the built tree whose mpyc_amd is timed')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    protocol(args) if args.protocol else drive(args)


if __name__ == '__main__':
    main()
