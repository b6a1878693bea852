#!/usr/bin/env python3
"""The two kernels of secure random bits (include/ffgpu_math.h) on the device, timed by device events, over 2^61 - 1,
2^80 - 65 and 2^128 - 173 at m = 3, t = 1 (k = 3 rows in the opening):

  ffgm_rbits_open at 10^7 entries next to the calls it replaces (k x ffgpu_muladd, one ffgpu_recombine), alternating passes:
  time, its algorithmic bytes (2 k + 1) n elements over that time as a fraction of the HBM ceiling (8 TB/s) and of the
  library's copy yardstick moving the same bytes in the same run, a byte comparison of the two results and the zero count;
  ffgm_rbits_finish at 1.6 10^7 entries (the bits of 10^6 fixed-point truncations by 16 bits) next to ffgpu_pow with the
  exponent (3p - 5) / 4 alone and next to ffgpu_pow plus the per-party ffgpu_mul, ffgpu_add_scalar and ffgpu_mul_scalar,
  alternating passes, with a byte comparison.  The spread of a kernel is the largest minus the smallest of its passes.

--protocol instead times protocols.Randomness(...).bits(16 10^6) end to end (wall time of a synchronised run, the draws
included) over the three fields, and over 2^80 - 65 a protocols.fxp_multiply of 10^6 elements of SecFxp(32, 16) fed by
Randomness.rand_trunc, the opened products checked.
usage: rbits_probe.py [--passes N] [--n-open N] [--n-finish N] [--protocol] [--tree DIR]"""
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
M, T = 3, 1


def row(**kw):
    print(json.dumps(kw), flush=True)


def stats(us):
    return {'us_median': statistics.median(us), 'us_min': min(us), 'us_max': max(us), 'spread_us': round(max(us) - min(us), 1), 'passes': us}


def alternating(fns, passes, launches=3):
    """`passes` timings (microseconds per call) of every function, one pass of each in turn, after warm-up"""
    from sort_probe import timed
    for fn in fns:
        timed(fn, WARM)
    out = [[] for _ in fns]
    for _ in range(passes):
        for us, fn in zip(out, fns):
            us.append(round(timed(fn, launches)[0] * 1e3, 1))
    return out


def drive(args):
    import torch
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext
    from sort_probe import random_elements
    k = 2 * T + 1
    for name, p in FIELDS:
        ctx = FieldContext(p, device=0)
        eb = ctx.elem_bytes
        lam = protocols._lagrange(finfields.GF(p), range(1, k + 1))
        # ---- the opening
        n = args.n_open
        rs, zs = [random_elements(ctx, n) for _ in range(k)], [random_elements(ctx, n) for _ in range(k)]
        out, out2, tmp, cnt = ctx.empty(n), ctx.empty(n), [ctx.empty(n) for _ in range(k)], ctx.zero_counter()
        fused = lambda: ctx.rbits_open(rs, zs, lam, zeros=cnt, out=out)

        def composed():
            for i in range(k):
                ctx.muladd(rs[i], rs[i], zs[i], out=tmp[i])
            return ctx.recombine(tmp, lam, out=out2)

        us_f, us_c = alternating((fused, composed), args.passes)
        cnt.zero_()
        fused(), composed()
        nbytes = (2 * k + 1) * n * eb
        src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        ctx.time_copy(src, dst, WARM)
        cp = ctx.time_copy(src, dst, 5)
        med = statistics.median(us_f)
        row(field=name, n=n, k=k, kernel='ffgm_rbits_open', algorithmic_bytes=nbytes, **stats(us_f), GBps=round(nbytes / med / 1e3),
            fraction_of_hbm_ceiling=round(nbytes / med / 1e6 / HBM_TBPS, 3), copy_same_bytes_us=round(cp * 1e3, 1),
            fraction_of_copy_rate=round(cp * 1e3 / med, 3), composed=stats(us_c), composed_over_fused=round(statistics.median(us_c) / med, 2),
            same_bytes_as_composed=bool(torch.equal(out.t, out2.t)), zeros=int(cnt.item()))
        del rs, zs, out, out2, tmp, src, dst
        torch.cuda.empty_cache()
        # ---- the finish: squares of r[0] for the public values, so that the bits are bits
        n = args.n_finish
        rs = [random_elements(ctx, n) for _ in range(M)]
        c = ctx.mul(rs[0], rs[0])
        bits, s, outs = [ctx.empty(n) for _ in range(M)], ctx.empty(n), [ctx.empty(n) for _ in range(M)]
        e, half = (3 * p - 5) >> 2, (p + 1) >> 1
        fused = lambda: ctx.rbits_finish(c, rs, outs=bits)
        plain = lambda: ctx.pow(c, e, out=s)

        def composed():
            ctx.pow(c, e, out=s)
            for i in range(M):
                ctx.mul(rs[i], s, out=outs[i])
                ctx.add_scalar(outs[i], 1, out=outs[i])
                ctx.mul_scalar(outs[i], half, out=outs[i])
            return outs

        us_f, us_p, us_c = alternating((fused, plain, composed), args.passes, launches=2)
        fused(), composed()
        same = all(bool(torch.equal(a.t, b.t)) for a, b in zip(bits, outs))
        first = bits[0].t if bits[0].t.dim() == 1 else bits[0].t[:, 0]
        med = statistics.median(us_f)
        row(field=name, n=n, m=M, kernel='ffgm_rbits_finish', **stats(us_f), ffgpu_pow_same_run=stats(us_p), composed=stats(us_c),
            ratio_to_pow_median=round(med / statistics.median(us_p), 4), composed_over_fused=round(statistics.median(us_c) / med, 3),
            same_bytes_as_composed=same, bits_of_party_1_are_bits=bool(((first == 0) | (first == 1)).all()))
        del rs, c, bits, s, outs
        torch.cuda.empty_cache()


def protocol(args):
    import torch
    from fxp_probe import small
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext

    def wall(fn):
        fn()                                                               # warm-up
        ms = []
        for _ in range(args.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        return ms, res

    count = 16 * 10**6
    for name, p in FIELDS:
        ctx = FieldContext(p, device=0)
        F = finfields.GF(p)
        R = protocols.Randomness(ctx, F, T, M, b'rbits probe key 1')
        ms, bits = wall(lambda: R.bits(count))
        opened = protocols.open_(ctx, F, bits, T)
        low = opened.t if opened.t.dim() == 1 else opened.t[:, 0]
        ones = int((low == 1).sum())
        ok = bool(((low == 0) | (low == 1)).all()) and (opened.t.dim() == 1 or not bool(opened.t[:, 1:].any()))
        row(protocol='Randomness.bits', field=name, count=count, m=M, t=T, wall_ms_median=statistics.median(ms), wall_ms_min=min(ms), passes=ms,
            bits_are_bits=ok, ones=ones, ns_per_bit=round(statistics.median(ms) * 1e6 / count, 2))
        if not ok:
            sys.exit('the opened bits are not bits')
        del bits, opened
        torch.cuda.empty_cache()
    name, p = FIELDS[1]
    ctx = FieldContext(p, device=0)
    F = finfields.GF(p)
    R = protocols.Randomness(ctx, F, T, M, b'rbits probe key 2')
    n, l, f = 10**6, 32, 16
    g = torch.Generator(device='cuda').manual_seed(l)
    a, b = (torch.randint(0, 1 << 20, (n,), generator=g, device='cuda', dtype=torch.int64) for _ in range(2))
    xs, ys = (protocols.share(ctx, small(ctx, v), T, M) for v in (a, b))
    ms, prod = wall(lambda: protocols.fxp_multiply(ctx, F, xs, ys, T, f, l, R.rand_trunc))
    opened = protocols.open_(ctx, F, prod, T)
    got = (opened.t if opened.t.dim() == 1 else opened.t[:, 0]).to(torch.int64)
    want = (a * b) >> f
    wrong = int(((got != want) & (got != want + 1)).sum())
    ms_draw, _ = wall(lambda: R.rand_trunc(n, f))
    row(protocol='fxp_multiply fed by Randomness.rand_trunc', field=name, n=n, l=l, f=f, m=M, t=T, wall_ms_median=statistics.median(ms),
        wall_ms_min=min(ms), passes=ms, of_it_rand_trunc_ms_median=statistics.median(ms_draw), wrong_of_n=wrong)
    if wrong:
        sys.exit('the opened products are wrong')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--n-open', type=int, default=10**7)
    ap.add_argument('--n-finish', type=int, default=16 * 10**6)
    ap.add_argument('--protocol', action='store_true')
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the built tree whose mpyc_amd is timed')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    protocol(args) if args.protocol else drive(args)


if __name__ == '__main__':
    main()
