#!/usr/bin/env python3
"""The kernels under secure unit vectors and table lookup at secret indices (ffgm_unit_prod / ffgm_unit_roll / ffgm_unit_dot,
include/ffgpu_math.h) on the device, timed by device events, over 2^61 - 1, 2^80 - 65 and 2^136 - 113 (8-, 12- and 24-byte
elements), at n = 10^5 indices and K2 = 16, 256, 2048 positions where memory allows (--max-gib):

  per kernel: its time, and the library's copy yardstick (ffgpu_time_copy, k_copy16) moving the kernel's algorithmic bytes in
  the same run -- (h + 1 + h) n elements for unit_prod at h = K2 / 2, (2 K + 1) n for unit_roll at K = K2, (K2 + 2) n + tlen
  for unit_dot at tlen = K2 -- and the copy's time as a fraction of the kernel's;
  against composed calls, each kernel next to the same result from calls the parent commit has, alternating: a materialised
  broadcast of x (torch) plus ffgpu_mul; a torch gather along the rows; unit_roll followed by ffgpu_matmul (1, K) x (K, n);
  the cost of the rotation: unit_dot with one offset for all indices against a random offset per index;
  every figure the median of `--passes` alternating passes of three launches each after two warm-up launches; the clocks the
  driver reports are printed first.

--protocol instead runs one protocols.lookup (public table) and one protocols.unit_vectors at n = 10^5, K = 256,
(m, t) = (3, 1) over 2^61 - 1, all parties on one GPU, the randomness drawn beforehand: GPU-busy time (ffgpu_busy_ms) and the
number of library calls per run, the wall time of a synchronised run, the share of the busy time per step (each step run
again on its own under the same timing), the opened result checked.
--counters is a driver for counter runs (`rocprofv3 --pmc FETCH_SIZE -- python tools/unitvec_probe.py --counters`, and again
with WRITE_SIZE; counters alone, no tracing in the run): the copy yardstick and the three kernels, three launches each.
usage: unitvec_probe.py [--passes N] [--n 100000] [--max-gib 8] [--protocol | --counters]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bsgn_probe import alternating, clocks, copy_us, row, stats  # noqa: E402

PRIMES = (2**61 - 1, 2**80 - 65, 2**136 - 113)
K2S = (16, 256, 2048)


def offsets(ctx, n, K2, same):
    """n canonical elements whose low bits are the offsets: one for all, or one per index"""
    import torch
    from fxp_probe import small
    c = torch.full((n,), K2 // 3, dtype=torch.int64, device='cuda') if same else torch.randint(0, K2, (n,), dtype=torch.int64, device='cuda')
    return small(ctx, c), c


def kernels(args):
    import torch
    from mpyc_amd.engine import DevArray, FieldContext
    from sort_probe import random_elements
    row(clocks=clocks(), device=torch.cuda.get_device_name(0))
    n = args.n
    for p in PRIMES:
        ctx = FieldContext(p, device=0)
        eb = ctx.elem_bytes
        for K2 in K2S:
            kbits = K2.bit_length() - 1
            if 3 * K2 * n * eb > args.max_gib * 2**30 or kbits > ctx.unit_dot_max_kbits():
                row(p=p, K2=K2, skipped='memory')
                continue
            U, x, tab = random_elements(ctx, K2 * n), random_elements(ctx, n), random_elements(ctx, K2)
            c, ci = offsets(ctx, n, K2, same=False)
            c1, _ = offsets(ctx, n, K2, same=True)
            big, out1 = ctx.empty(K2 * n), ctx.empty(n)
            h = K2 // 2
            Uh, oh = DevArray(ctx, U.t[:h * n], h * n), DevArray(ctx, big.t[:h * n], h * n)
            rows = lambda t_: t_.reshape((K2, n) + tuple(t_.shape[1:]))
            # unit_prod against a materialised broadcast plus ffgpu_mul
            xb = ctx.empty(h * n)

            def composed_prod():
                xb.t.reshape((h, n) + tuple(xb.t.shape[1:])).copy_(x.t.unsqueeze(0).expand((h,) + tuple(x.t.shape)))
                return ctx.mul(xb, Uh, out=oh)

            us_k, us_c = alternating([lambda: ctx.unit_prod(x, Uh, h, out=oh), composed_prod], args.passes)
            nbytes = (2 * h + 1) * n * eb
            cp, med = copy_us(ctx, nbytes), statistics.median(us_k)
            row(kernel='ffgm_unit_prod', p=p, n=n, h=h, algorithmic_bytes=nbytes, **stats(us_k), copy_same_bytes_us=cp,
                fraction_of_copy_rate=round(cp / med, 3), composed_broadcast_mul=stats(us_c))
            # unit_roll against a torch gather
            src = ((torch.arange(K2, device='cuda')[:, None] - ci[None, :]) % K2)
            idx = src.reshape((K2, n) + (1,) * (U.t.dim() - 1)).expand((K2, n) + tuple(U.t.shape[1:]))

            def composed_roll():
                return torch.gather(rows(U.t), 0, idx, out=rows(big.t))

            want = composed_roll().clone()
            us_k, us_c = alternating([lambda: ctx.unit_roll(U, c, kbits, K2, out=big), composed_roll], args.passes)
            ctx.unit_roll(U, c, kbits, K2, out=big)
            ok_roll = bool(torch.equal(rows(big.t), want))
            nbytes = (2 * K2 + 1) * n * eb
            cp, med = copy_us(ctx, nbytes), statistics.median(us_k)
            row(kernel='ffgm_unit_roll', p=p, n=n, K=K2, algorithmic_bytes=nbytes, **stats(us_k), copy_same_bytes_us=cp,
                fraction_of_copy_rate=round(cp / med, 3), composed_torch_gather=stats(us_c), same_as_gather=ok_roll)
            # unit_dot against unit_roll + matmul, and with one offset for all indices
            def composed_dot():
                return ctx.matmul(tab, ctx.unit_roll(U, c, kbits, K2, out=big), 1, K2, n, out=out1)

            want = composed_dot().t.clone()
            us_k, us_1, us_c = alternating([lambda: ctx.unit_dot(U, tab, K2, c=c, kbits=kbits, out=out1),
                                            lambda: ctx.unit_dot(U, tab, K2, c=c1, kbits=kbits, out=out1), composed_dot], args.passes)
            ok_dot = bool(torch.equal(ctx.unit_dot(U, tab, K2, c=c, kbits=kbits).t, want))
            nbytes = ((K2 + 2) * n + K2) * eb
            cp, med = copy_us(ctx, nbytes), statistics.median(us_k)
            row(kernel='ffgm_unit_dot', p=p, n=n, K2=K2, tlen=K2, algorithmic_bytes=nbytes, **stats(us_k), copy_same_bytes_us=cp,
                fraction_of_copy_rate=round(cp / med, 3), one_offset_for_all=stats(us_1), composed_roll_matmul=stats(us_c),
                same_as_roll_matmul=ok_dot)
            if not (ok_roll and ok_dot):
                sys.exit('a kernel disagrees with its composed route')
            del U, x, tab, c, c1, big, out1, xb, idx, src, want
            torch.cuda.empty_cache()


def counters(args):
    """a driver for `rocprofv3 --pmc <counter> -- python tools/unitvec_probe.py --counters` (one counter set per run, no
    tracing in it): over 2^61 - 1 at n = 10^5, per K2 in 256, 2048 three launches each of the copy yardstick on 2 K2 n
    elements (it calibrates the counter's unit), unit_prod (h = K2 / 2), unit_roll (K = K2) and unit_dot; the launches of one
    kernel and K2 are told apart by their order in the counter file: copy, prod, roll, dot, per K2"""
    import torch
    from mpyc_amd.engine import DevArray, FieldContext
    from sort_probe import random_elements
    ctx = FieldContext(PRIMES[0], device=0)
    n = args.n
    for K2 in (256, 2048):
        kbits, h = K2.bit_length() - 1, K2 // 2
        U, x, tab = random_elements(ctx, K2 * n), random_elements(ctx, n), random_elements(ctx, K2)
        c, _ = offsets(ctx, n, K2, same=False)
        big, out1 = ctx.empty(K2 * n), ctx.empty(n)
        Uh, oh = DevArray(ctx, U.t[:h * n], h * n), DevArray(ctx, big.t[:h * n], h * n)
        for fn in (lambda: ctx.copy(U.t, big.t), lambda: ctx.unit_prod(x, Uh, h, out=oh), lambda: ctx.unit_roll(U, c, kbits, K2, out=big),
                   lambda: ctx.unit_dot(U, tab, K2, c=c, kbits=kbits, out=out1)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
        del U, x, tab, c, big, out1, Uh, oh
        torch.cuda.empty_cache()
    print('counters driver done')


def protocol(args):
    import torch
    from fxp_probe import low, small
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext
    p, m, t, K, n = PRIMES[0], 3, 1, 256, args.n
    kbits, K2 = 8, 256
    ctx, F = FieldContext(p, device=0), finfields.GF(p)
    row(clocks=clocks(), device=torch.cuda.get_device_name(0), p=p, n=n, K=K, m=m, t=t)
    g = torch.Generator(device='cuda').manual_seed(7)
    ri = lambda lo, hi, count: torch.randint(lo, hi, (count,), generator=g, device='cuda', dtype=torch.int64)
    sh = lambda v: protocols.share(ctx, v, t, m)
    plain = ri(0, K, n)
    xs = sh(small(ctx, plain))
    tvals = ri(0, 1 << 30, K)
    table = small(ctx, tvals)
    pool = (sh(small(ctx, ri(0, 2, kbits * n))), sh(small(ctx, ri(1, (1 << 30) + 1, n))))
    rand_unit = lambda count, kb, sec: pool
    routes = {
        'lookup (public table)': (lambda: protocols.lookup(ctx, F, xs, table, K, t, rand_unit),
                                  lambda got: low(got) != tvals[plain]),
        'unit_vectors': (lambda: protocols.unit_vectors(ctx, F, xs, K, t, rand_unit),
                         lambda got: low(got).reshape(K, n) != (torch.arange(K, device='cuda')[:, None] == plain[None, :]).to(torch.int64)),
    }
    # the steps of the route on their own (the randomised route: demultiplexer, positions, opening, then roll or dot)
    u = protocols.random_unit_vectors(ctx, F, n, kbits, t, pool[0])
    r = protocols.arg_index(ctx, u, 1, K2, n)
    c = protocols.open_(ctx, F, [ctx.add(ctx.sub(xs[i], r[i]), ctx.mul_scalar(pool[1][i], K2)) for i in range(t + 1)], t)
    half = [protocols._rows(ctx, x, 0, K2 // 2, n) for x in u]
    last_bit = [protocols._rows(ctx, b, 0, 1, n) for b in pool[0]]

    def last_round():
        sub = protocols.reshare(ctx, F, [ctx.unit_prod(last_bit[q], half[q], K2 // 2) for q in range(2 * t + 1)], t, m)
        return [ctx.tour_unit_expand(half[j], sub.rows[j], sub.lam, 1, K2, n) for j in range(m)]

    steps = {
        'random_unit_vectors': lambda: protocols.random_unit_vectors(ctx, F, n, kbits, t, pool[0]),
        'its last doubling round alone': last_round,
        'positions (unit_dot on 0 .. K2 - 1)': lambda: protocols._unit_positions(ctx, u, kbits, n),
        'positions by arg_index, for comparison': lambda: protocols.arg_index(ctx, u, 1, K2, n),
        'mask and open': lambda: protocols.open_(ctx, F, [ctx.add(ctx.sub(xs[i], r[i]), ctx.mul_scalar(pool[1][i], K2)) for i in range(t + 1)], t),
        'unit_roll, all parties': lambda: [ctx.unit_roll(x, c, kbits, K) for x in u],
        'unit_dot, all parties': lambda: [ctx.unit_dot(x, table, K2, c=c, kbits=kbits) for x in u],
    }
    ctx.set_timing(True, accumulate=True)

    def measure(fn):
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
        return dict(gpu_busy_ms_median=statistics.median(busy), busy_passes=busy, library_calls_per_run=calls[0],
                    wall_ms_median=statistics.median(wall), wall_passes=wall)

    for label, (fn, wrong_of) in routes.items():
        wrong = int(wrong_of(protocols.open_(ctx, F, fn(), t)).sum())
        row(protocol=label, wrong=wrong, **measure(fn))
        if wrong:
            sys.exit('the opened result is wrong')
    for label, fn in steps.items():
        row(step=label, **measure(fn))
    ctx.set_timing(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--max-gib', type=float, default=8.0)
    ap.add_argument('--protocol', action='store_true')
    ap.add_argument('--counters', action='store_true')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    counters(args) if args.counters else protocol(args) if args.protocol else kernels(args)


if __name__ == '__main__':
    main()
