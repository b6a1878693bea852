#!/usr/bin/env python3
"""The kernels of the secure binary sign by Legendre symbols (include/ffgpu_math.h) on the device, timed by device events,
over the 64-bit prime the demo pairs with its five-symbol variant, at n = 2^20 and 2^24:

  ffgm_bsgn_mask for w = 1, 3, 5: time, its algorithmic bytes (2 w + 1) n elements over that time, and the library's copy
  yardstick (ffgpu_time_copy) moving the same bytes in the same run;
  ffgm_bsgn_finish for m = 3, w = 1, 3, 5, in both modes, next to ffgpu_pow with the exponent (p - 1) / 2 on the same w n
  elements in the same run, alternating (the same chain: the difference is the cost of the ends), and the copy yardstick
  moving the extra (2 m w or m w + m) n elements;
  every figure the median of `--passes` passes of three launches each after two warm-up launches; the clocks the driver
  reports are printed first.

--protocol instead runs protocols.bsgn at d = 0, 1, 2 (each over the prime the demo pairs it with) and
protocols.compare_zero(mode='lt', l=10) on the same elements, (m, t) = (3, 1), all parties on one GPU, the randomness drawn
beforehand: GPU-busy time (the summed time of the library's calls, ffgpu_busy_ms) and the number of those calls per run, the
wall time of a synchronised run, the opened result checked against the sign.
usage: bsgn_probe.py [--passes N] [--logn 20,24] [--protocol]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRIMES = (3546374752298322551, 9409569905028393239, 15569949805843283171)
HBM_TBPS = 8.0
WARM = 2


def row(**kw):
    print(json.dumps(kw), flush=True)


def stats(us):
    return {'us_median': statistics.median(us), 'us_min': min(us), 'us_max': max(us), 'passes': us}


def clocks():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if 'GPU[0]' in ln and ('sclk' in ln or 'mclk' in ln or 'fclk' in ln)]
    except (OSError, subprocess.SubprocessError) as e:
        return ['not read: %s' % e]


def alternating(fns, passes):
    """per function, `passes` timings (microseconds per call) of three launches each, the functions taking turns"""
    from sort_probe import timed
    for fn in fns:
        timed(fn, WARM)
    us = [[] for _ in fns]
    for _ in range(passes):
        for i, fn in enumerate(fns):
            us[i].append(round(timed(fn, 3)[0] * 1e3, 1))
    return us


def copy_us(ctx, nbytes):
    import torch
    src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    ctx.time_copy(src, dst, WARM)
    return round(ctx.time_copy(src, dst, 5) * 1e3, 1)


def kernels(args):
    import torch
    from mpyc_amd.engine import DevArray, FieldContext
    from sort_probe import random_elements
    p = PRIMES[2]
    ctx = FieldContext(p, device=0)
    eb, m = ctx.elem_bytes, 3
    row(clocks=clocks(), device=torch.cuda.get_device_name(0), p=p, elem_bytes=eb)
    for logn in args.logn:
        n = 1 << logn
        for w in (1, 3, 5):
            a, z, out = random_elements(ctx, n), random_elements(ctx, w * n), ctx.empty(w * n)
            betas = [1 + 2 * j for j in range(-(w // 2), w // 2 + 1)]
            us, = alternating([lambda: ctx.bsgn_mask(a, z, 2, betas, out=out)], args.passes)
            nbytes = (2 * w + 1) * n * eb
            cp, med = copy_us(ctx, nbytes), statistics.median(us)
            row(kernel='ffgm_bsgn_mask', n=n, w=w, algorithmic_bytes=nbytes, **stats(us), GBps=round(nbytes / med / 1e3),
                fraction_of_hbm_ceiling=round(nbytes / med / 1e6 / HBM_TBPS, 3), copy_same_bytes_us=cp, fraction_of_copy_rate=round(cp / med, 3))
            # the finish on the masked values, next to the plain exponentiation of the same elements
            c, e, po = out, (p - 1) // 2, ctx.empty(w * n)
            ss = [random_elements(ctx, w * n) for _ in range(m)]
            rows_out, sum_out = [ctx.empty(w * n) for _ in range(m)], [ctx.empty(n) for _ in range(m)]
            us_p, us_r, us_s = alternating([lambda: ctx.pow(c, e, out=po), lambda: ctx.bsgn_finish(c, ss, w, outs=rows_out),
                                            lambda: ctx.bsgn_finish(c, ss, w, sum=True, outs=sum_out)], args.passes)
            # the same symbols from the powers: party 0's rows
            one = (po.t == 1) if po.t.dim() == 1 else ((po.t[:, 0] == 1) & (po.t[:, 1:] == 0).all(1))
            neg = ctx.neg(ss[0])
            want = torch.where(one.reshape(-1, *[1] * (ss[0].t.dim() - 1)), ss[0].t, neg.t)
            want = torch.where(((c.t == 0) if c.t.dim() == 1 else (c.t == 0).all(1)).reshape(-1, *[1] * (ss[0].t.dim() - 1)),
                               torch.zeros_like(want), want)
            same = bool(torch.equal(want, rows_out[0].t))
            mp = statistics.median(us_p)
            for label, us_f, extra in (('rows', us_r, 2 * m * w * n), ('sum', us_s, (m * w + m) * n)):
                mf = statistics.median(us_f)
                row(kernel='ffgm_bsgn_finish', mode=label, n=n, w=w, m=m, **stats(us_f), ffgpu_pow_same_run=stats(us_p),
                    over_pow_us=round(mf - mp, 1), extra_elements=extra, copy_of_extra_bytes_us=copy_us(ctx, extra * eb),
                    rows_same_as_pow=same)
            del a, z, out, c, po, ss, rows_out, sum_out, want, neg
            torch.cuda.empty_cache()


def protocol(args):
    import torch
    from fxp_probe import low, small
    from sort_probe import random_elements
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext
    m, t, l = 3, 1, 10
    row(clocks=clocks(), device=torch.cuda.get_device_name(0))
    for logn in args.logn:
        n = 1 << logn
        for d, p in enumerate(PRIMES):
            ctx = FieldContext(p, device=0)
            F = finfields.GF(p)
            B = protocols.bsgn_range(p, d)
            g = torch.Generator(device='cuda').manual_seed(d + logn)
            ri = lambda lo, hi, count: torch.randint(lo, hi, (count,), generator=g, device='cuda', dtype=torch.int64)
            sh = lambda v: protocols.share(ctx, v, t, m)
            plain = ri(-min(B, 1 << (l - 1)), min(B, (1 << (l - 1)) - 1) + 1, n)
            xs = sh(ctx.add_scalar(small(ctx, plain + (1 << l)), p - (1 << l)))
            cnt = protocols.bsgn_draws(d) * n
            signs = ctx.add_scalar(small(ctx, 2 * ri(0, 2, cnt)), p - 1)
            pool = (sh(signs), sh(random_elements(ctx, cnt)))
            rbits, sbits, rdivl, rzero = sh(small(ctx, ri(0, 2, n * l))), sh(small(ctx, ri(0, 2, n))), sh(small(ctx, ri(0, 1 << 16, n))), \
                sh(random_elements(ctx, n))
            routes = {'bsgn d=%d' % d: (lambda: protocols.bsgn(ctx, F, xs, t, d, lambda count: pool),
                                        lambda got: low(ctx.add_scalar(got, 1)) != 2 * (plain >= 0).to(torch.int64)),
                      'compare_zero lt l=%d' % l: (lambda: protocols.compare_zero(ctx, F, xs, rbits, sbits, rdivl, rzero, t, l, mode='lt'),
                                                   lambda got: low(got) != (plain < 0).to(torch.int64))}
            ctx.set_timing(True, accumulate=True)
            for label, (fn, wrong_of) in routes.items():
                wrong = int(wrong_of(protocols.open_(ctx, F, fn(), t)).sum())            # warm-up, and the check
                fn()
                busy, calls, wall = [], [], []
                for _ in range(args.passes):
                    ctx.busy_ms(reset=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    wall.append(round((time.perf_counter() - t0) * 1e3, 3))
                    ms, k = ctx.busy_ms(reset=True)
                    busy.append(round(ms, 3)), calls.append(k)
                row(protocol=label, p=p, n=n, m=m, t=t, range_B=B, wrong_of_n=wrong, gpu_busy_ms_median=statistics.median(busy), busy_passes=busy,
                    library_calls_per_run=calls[0], wall_ms_median=statistics.median(wall), wall_passes=wall)
                if wrong:
                    sys.exit('the opened result is wrong')
            ctx.set_timing(False)
            del xs, pool, rbits, sbits, rdivl, rzero
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--logn', default='20,24')
    ap.add_argument('--protocol', action='store_true')
    args = ap.parse_args()
    args.logn = [int(v) for v in args.logn.split(',')]
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    protocol(args) if args.protocol else kernels(args)


if __name__ == '__main__':
    main()
