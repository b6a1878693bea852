#!/usr/bin/env python3
"""The kernels under the secure logarithm and exponential (include/ffgpu_math.h) for one party at n = 10^6 over 2^61 - 1 and
2^80 - 65, timed by device events:

  ffgm_poly_dot (theta = 11 and 64) and ffgm_powers_prod ((h, w) = (6, 5) and (32, 32)), each followed by the library's copy
  yardstick (ffgpu_time_copy) moving the bytes the kernel must move by its map: (theta + 1) n and (2 w + 1) n elements;
  ffgm_pow_base at ebits = 48 and 80 (61 where the modulus is shorter) next to ffgpu_pow with one host exponent of the same bit
  length in the same run: the fixed-base kernel does at most ceil(ebits/4) - 1 products per element, square-and-multiply
  about ebits + ebits/2; and once more with one exponent in every element, where the table reads are broadcasts and no lane
  diverges -- the difference is what divergent LDS reads and divergent windows cost;
  ffgm_bits_reverse at l = 31.

--protocol instead times protocols.log and protocols.exp2 end to end, SecFxp(32, 16), all parties on one GPU, m = 3, t = 1:
wall time of a synchronised run with the randomness drawn beforehand (one pool of bit shares and high masks, sliced per
call), and the opened values checked against float64 log / exp2 to a few units of 2^-f.
usage: explog_probe.py [--launches N] [--n N] [--protocol]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FIELDS = [('2^61-1', 2**61 - 1), ('2^80-65', 2**80 - 65)]
WARM = 2


def row(**kw):
    print(json.dumps(kw), flush=True)


def drive(args):
    import torch
    from mpyc_amd.engine import DevArray, FieldContext
    from sort_probe import random_elements, timed
    n = args.n
    for name, p in FIELDS:
        ctx = FieldContext(p, device=0)
        eb = ctx.elem_bytes
        P = random_elements(ctx, 64 * n)
        out = ctx.empty(32 * n)

        def against_copy(label, fn, elems):
            nbytes = elems * eb
            src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')       # a copy reads and writes: same bytes moved
            dst = torch.empty_like(src)
            timed(fn, WARM)
            ms, _ = timed(fn, args.launches)
            ctx.time_copy(src, dst, WARM)
            cp = ctx.time_copy(src, dst, args.launches)
            row(field=name, n=n, kernel=label, bytes=nbytes, event_us=round(ms * 1e3, 1), event_GBps=round(nbytes / ms / 1e6),
                copy_us=round(cp * 1e3, 1), fraction_of_copy_rate=round(cp / ms, 3))

        for theta in (11, 64):
            tab = random_elements(ctx, theta)
            o = DevArray(ctx, out.t[:n], n)
            against_copy(f'poly_dot theta={theta}', lambda: ctx.poly_dot(P, n, tab, 12345, out=o), (theta + 1) * n)
        for h, w in ((6, 5), (32, 32)):
            o = DevArray(ctx, out.t[:w * n], w * n)
            against_copy(f'powers_prod h={h} w={w}', lambda: ctx.powers_prod(P, n, h, w, out=o), (2 * w + 1) * n)
        o = DevArray(ctx, out.t[:31 * n], 31 * n)
        bits = DevArray(ctx, P.t[:31 * n], 31 * n)
        against_copy('bits_reverse l=31', lambda: ctx.bits_reverse(bits, 31, out=o), 2 * 31 * n)
        x = DevArray(ctx, P.t[:n], n)
        o = DevArray(ctx, out.t[:n], n)
        for ebits in (48, min(80, p.bit_length())):
            tab = ctx.pow_table(3, ebits)
            shift = p.bit_length() - ebits                     # the top ebits bits of a random element: uniform windows
            fixed = lambda: ctx.pow_base(x, tab, ebits, shift=shift, out=o)
            e = (1 << ebits) - 1 - (0x5a5a5a5a5a5a5a5a5a5a5a & ((1 << (ebits - 1)) - 1))     # ebits bits, about half of them set
            plain = lambda: ctx.pow(x, e, out=o)
            timed(fixed, WARM)
            ms_f, _ = timed(fixed, args.launches)
            timed(plain, WARM)
            ms_p, _ = timed(plain, args.launches)
            same = DevArray(ctx, x.t[:1].expand(*([n] + list(x.t.shape[1:]))).contiguous(), n)    # every lane the same windows:
            uniform = lambda: ctx.pow_base(same, tab, ebits, shift=shift, out=o)                  # broadcast reads, no divergence
            timed(uniform, WARM)
            ms_u, _ = timed(uniform, args.launches)
            row(field=name, n=n, kernel=f'pow_base ebits={ebits}', table_bytes=tab.n * eb, event_us=round(ms_f * 1e3, 1),
                ffgpu_pow_same_bits_us=round(ms_p * 1e3, 1), speedup=round(ms_p / ms_f, 2),
                same_exponent_everywhere_us=round(ms_u * 1e3, 1),
                ps_per_product=round(ms_f * 1e9 / n / ((ebits + 3) // 4 * 15 / 16), 2),
                ffgpu_pow_ps_per_product=round(ms_p * 1e9 / n / (1.5 * ebits), 2))
        del P, out
        torch.cuda.empty_cache()


def protocol(args):
    import torch
    from fxp_probe import low, small
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import DevArray, FieldContext
    m, t, n, l, f = 3, 1, args.n, 32, 16
    for name, p in FIELDS:
        ctx = FieldContext(p, device=0)
        F = finfields.GF(p)
        g = torch.Generator(device='cuda').manual_seed(l)
        ri = lambda lo, hi, k: torch.randint(lo, hi, (k,), generator=g, device='cuda', dtype=torch.int64)
        sh = lambda v: protocols.share(ctx, small(ctx, v), t, m)
        most = max(n * (l - 1), 8 * n * f)                     # the bit decomposition; the widest ladder round of either function
        pool_bits, pool_hi = sh(ri(0, 2, most)), sh(ri(0, 1 << 8, 8 * n))
        cut = lambda xs, k: [DevArray(ctx, x.t[:k], k) for x in xs]
        rand_trunc = lambda count, f_: (cut(pool_bits, count * f_), cut(pool_hi, count))
        rand_bits = lambda count, l_: (cut(pool_bits, count * l_), cut(pool_hi, count))
        masks = [small(ctx, ri(0, 1 << 30, n)) for _ in range(t + 1)]
        rand_exp = lambda count, bound: masks
        a_log = ri(1, 1 << (l - 1), n)
        a_exp = ri(-f << f, (l - 1 - f) << f, n)
        xs_log = sh(a_log)
        xs_exp = [ctx.add_scalar(x, -(f << f) % p) for x in sh(a_exp + (f << f))]          # (small() takes non-negative values)
        calls = {'log': (lambda: protocols.log(ctx, F, xs_log, t, l, f, rand_bits, rand_trunc),
                         lambda: torch.log(a_log.double() / 2**f)),
                 'exp2': (lambda: protocols.exp2(ctx, F, xs_exp, t, l, f, rand_trunc, rand_exp),
                          lambda: torch.exp2(a_exp.double() / 2**f))}
        for label, (fn, ref) in calls.items():
            opened = protocols.open_(ctx, F, [ctx.add_scalar(x, 1 << (l - 1)) for x in fn()], t)     # warm-up, and the check
            got = ((low(opened) & 0xffffffff) - (1 << (l - 1))).double() / 2**f            # (32-bit limbs arrive sign-extended)
            want = ref()
            err = ((got - want).abs() / torch.clamp(want.abs(), min=1.0)).max().item() * 2**f
            ms = []
            for _ in range(args.launches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            ok = err <= 16
            row(protocol=label, field=name, l=l, f=f, n=n, m=m, t=t, correct=ok, largest_error_units_of_2_to_minus_f=round(err, 2),
                wall_ms_median=round(statistics.median(ms), 2), wall_ms_min=round(min(ms), 2))
            if not ok:
                sys.exit('the opened result is wrong')
        del pool_bits, pool_hi, xs_log, xs_exp
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=10, help='timed launches per kernel (after 2 warm-up launches)')
    ap.add_argument('--n', type=int, default=10**6)
    ap.add_argument('--protocol', action='store_true')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    protocol(args) if args.protocol else drive(args)


if __name__ == '__main__':
    main()
