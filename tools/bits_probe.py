#!/usr/bin/env python3
"""Device time of bit decomposition over a prime field (protocols.to_bits: ffgpu_bits_mask / _expand / _finish and the two
level kernels ffgpu_carry_prod / _apply) at n = 10^6, l = 32, m = 3, t = 1, per kernel and whole, next to the SAME protocol
composed from the calls the engine had before these kernels: matmul with the power vector and element-wise calls for the
mask; the public c_bits built on the host and uploaded, a transposed copy and element-wise calls for the leaves;
index_select gathers, the product inside ffgpu_mul_split_rng, ffgpu_recombine, ffgpu_add and index_copy_ for a round;
transposed copies and element-wise calls for the sum bits.  The comparison partner is always that composed route, never
the new code.  Alternating runs by device events; the whole protocol also by wall clock (host work included).

Per step: median microseconds of both routes for ONE party (the level kernels: summed over the rounds), algorithmic bytes
(what the step must read and write), GB/s, the ratio composed / kernel, and whether both routes gave the same bytes.  Then
the whole protocol for all parties, both routes, and each kernel's share of the fused route's device time (its one-party
time times the number of parties that run it).

One field per process keeps a step short; run the fields as separate steps, each under its own time limit:
    timeout -k 10 300 python tools/bits_probe.py --fields p61 --out out/bits_p61.json --md out/bits_p61.md && \\
    timeout -k 10 300 python tools/bits_probe.py --fields p64 --out out/bits_p64.json --md out/bits_p64.md
usage: bits_probe.py [--out FILE.json] [--md FILE.md] [--reps N] [--fields p61,p64] [--n N] [--l L]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

FIELDS = {'p61': 2**61 - 1, 'p64': 2**64 - 189}
M, T = 3, 1


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def merges(l):
    out = []

    def f(i, j, high):
        if j - i == 1:
            return
        h = i + (j - i) // 2
        f(i, h, high)
        f(h, j, True)
        out.append((i, h, j, high))
    f(0, l, False)
    return sorted(out)


def level(l, rho):
    c, d = [], []
    for i, h, j, high in merges(l):
        if (j - i - 1).bit_length() == rho:
            c += [(k, h - 1) for k in range(h, j)]
            d += [(k, h - 1) for k in range(h, j)] if high else []
    return c, d


class Composed:
    """the protocol's local steps from the calls that existed before the bits kernels (8-byte elements)"""

    def __init__(self, ctx, l, n):
        from mpyc_amd.engine import DevArray
        self.ctx, self.l, self.n, self.DevArray = ctx, l, n, DevArray
        self.pw = ctx.from_ints([1 << k for k in range(l)])
        self.idx = {}
        for rho in range(1, (l - 1).bit_length() + 1):
            c, d = level(l, rho)
            ix = lambda v: torch.as_tensor(v, device='cuda', dtype=torch.int64)
            self.idx[rho] = (ix([q for _, q in c]), ix([k for k, _ in c]), ix([q for _, q in d]), ix([k for k, _ in d]), len(c), len(d))

    def arr(self, t):
        t = t.contiguous().reshape(-1)
        return self.DevArray(self.ctx, t, t.shape[0])

    def mask(self, a, rbits, rdivl):
        ctx, l = self.ctx, self.l
        r_modl = ctx.matmul(rbits, self.pw, self.n, l, 1)
        return ctx.sub(ctx.add(ctx.add_scalar(a, 1 << l), ctx.mul_scalar(rdivl, (1 << l) % ctx.modulus)), r_modl)

    def c_bits(self, c):
        """the public bits of c mod 2^l, built on the host and uploaded (runtime.py:4447-4448): bit-major and element-major"""
        l = self.l
        host = c.t.cpu().numpy().astype(np.uint64) & np.uint64((1 << l) - 1)
        bits = ((host[:, None] >> np.arange(l, dtype=np.uint64)[None, :]) & np.uint64(1))        # (n, l)
        up = lambda x: self.arr(torch.from_numpy(np.ascontiguousarray(x).astype(np.int64)).to('cuda').view(c.t.dtype))
        return up(bits.T), up(bits)

    def expand(self, CB, rbits):
        ctx = self.ctx
        rT = self.arr(rbits.t.reshape(self.n, self.l).transpose(0, 1))
        g = ctx.mul(CB, rT)
        return g, ctx.sub(ctx.add(CB, rT), ctx.mul_scalar(g, 2))

    def gather(self, g, p, rho):
        qc, kc, qd, kd, _, _ = self.idx[rho]
        G, P = g.t.reshape(self.l, self.n), p.t.reshape(self.l, self.n)
        left = self.arr(torch.cat([G.index_select(0, qc), P.index_select(0, qd)]))
        right = self.arr(torch.cat([P.index_select(0, kc), P.index_select(0, kd)]))
        return left, right

    def prod(self, g, p, rho):
        left, right = self.gather(g, p, rho)
        return self.ctx.mul(left, right)

    def apply(self, g, p, rows, lam, rho):
        ctx, n = self.ctx, self.n
        _, kc, _, kd, rc, rd = self.idx[rho]
        v = ctx.recombine(rows, lam)
        G, P = g.t.reshape(self.l, n), p.t.reshape(self.l, n)
        V = v.t.reshape(rc + rd, n)
        new = ctx.add(self.arr(G.index_select(0, kc)), self.arr(V[:rc]))
        G.index_copy_(0, kc, new.t.reshape(rc, n))
        if rd:
            P.index_copy_(0, kd, V[rc:])
        return g, p

    def finish(self, CBe, rbits, g):
        ctx, l, n = self.ctx, self.l, self.n
        gT = g.t.reshape(l, n).transpose(0, 1).contiguous()
        sT = torch.zeros_like(gT)
        sT[:, 1:] = gT[:, :-1]
        return ctx.add(ctx.sub(ctx.add(rbits, CBe), ctx.mul_scalar(self.arr(gT), 2)), self.arr(sT))

    def to_bits(self, field, xs, rbits, rdivl):
        """the whole protocol, all parties (protocols.to_bits with the composed steps)"""
        from mpyc_amd import protocols
        ctx, l = self.ctx, self.l
        m, kk = len(xs), 2 * T + 1
        c = protocols.open_(ctx, field, [self.mask(xs[i], rbits[i], rdivl[i]) for i in range(T + 1)], T)
        CB, CBe = self.c_bits(c)
        gp = [self.expand(CB, rbits[i]) for i in range(m)]
        for rho in sorted(self.idx):
            left, right = zip(*[self.gather(gp[i][0], gp[i][1], rho) for i in range(kk)])
            sub = protocols.reshare(ctx, field, left, T, m, mul_by=right)    # the product inside the share generation
            for j in range(m):
                self.apply(gp[j][0], gp[j][1], sub.rows[j], sub.lam, rho)
        return [self.finish(CBe, rbits[i], gp[i][0]) for i in range(m)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fields', default=','.join(FIELDS))
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--l', type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from mpyc_amd import finfields, protocols
    from mpyc_amd.engine import FieldContext
    n, l = args.n, args.l
    nrounds = (l - 1).bit_length()
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'n': n, 'l': l, 'm': M, 't': T, 'cells': [], 'whole': []}
    for name in args.fields.split(','):
        p = FIELDS[name]
        ctx = FieldContext(p, device=0)
        F = finfields.GF(p)
        eb = ctx.elem_bytes
        assert eb == 8, 'the composed route of this probe handles 8-byte elements'
        gen = torch.Generator(device='cuda').manual_seed(5)
        rnd = lambda count, hi: torch.randint(0, hi, (count,), dtype=torch.int64, device='cuda', generator=gen)
        el = lambda t: ctx.reduce(comp.arr(t.view(ctx.empty(1).t.dtype)))
        comp = Composed(ctx, l, n)
        sh = lambda x: protocols.share(ctx, x, T, M)
        xs = sh(el(rnd(n, 1 << (l - 1))))
        rbits, rdivl = sh(el(rnd(n * l, 2))), sh(el(rnd(n, 1 << 24) + 1))
        lam = protocols._lagrange(F, range(1, 2 * T + 2))
        kk = 2 * T + 1
        c = protocols.open_(ctx, F, [ctx.bits_mask(xs[i], rbits[i], rdivl[i], l, 1 << l) for i in range(T + 1)], T)
        t0 = time.perf_counter()
        CB, CBe = comp.c_bits(c)
        torch.cuda.synchronize()
        cbits_ms = (time.perf_counter() - t0) * 1e3
        g0, p0 = ctx.bits_expand(c, rbits[0], l)
        levels = {rho: level(l, rho) for rho in range(1, nrounds + 1)}
        R = {rho: len(cd[0]) + len(cd[1]) for rho, cd in levels.items()}
        subrows = {rho: [el(rnd(R[rho] * n, 1 << 62)) for _ in range(kk)] for rho in levels}
        sumR, sumRc = sum(R.values()), sum(len(cd[0]) for cd in levels.values())

        def all_rounds(fn):
            out = None
            for rho in levels:
                out = fn(rho)
            return out

        def apply_new():
            g, pp = g0.clone(), p0.clone()
            return timed(lambda: all_rounds(lambda rho: ctx.carry_apply(g, pp, subrows[rho], lam, l, rho)))

        def apply_old():
            g, pp = g0.clone(), p0.clone()
            return timed(lambda: all_rounds(lambda rho: comp.apply(g, pp, subrows[rho], lam, rho)))

        steps = {
            'bits_mask': (lambda: timed(lambda: ctx.bits_mask(xs[0], rbits[0], rdivl[0], l, 1 << l)),
                          lambda: timed(lambda: comp.mask(xs[0], rbits[0], rdivl[0])), (n * l + 2 * n) + n, T + 1),
            'bits_expand': (lambda: timed(lambda: ctx.bits_expand(c, rbits[0], l)), lambda: timed(lambda: comp.expand(CB, rbits[0])),
                            (n * l + n) + 2 * n * l, M),
            'carry_prod (all rounds)': (lambda: timed(lambda: all_rounds(lambda rho: ctx.carry_prod(g0, p0, l, rho))),
                                        lambda: timed(lambda: all_rounds(lambda rho: comp.prod(g0, p0, rho))), 3 * sumR * n, kk),
            'carry_apply (all rounds)': (apply_new, apply_old, (kk * sumR + sumRc + sumR) * n, M),
            'bits_finish': (lambda: timed(lambda: ctx.bits_finish(c, rbits[0], g0, l)), lambda: timed(lambda: comp.finish(CBe, rbits[0], g0)),
                            (2 * n * l + n) + n * l, M),
        }
        per_party = {}
        for step, (new, old, elems, parties) in steps.items():
            nbytes = elems * eb
            new_ms, old_ms, same = [], [], None
            for rep in range(args.reps + 1):                                      # rep 0 warms every route up
                ms, r_new = new()
                if rep:
                    new_ms.append(ms)
                ms, r_old = old()
                if rep:
                    old_ms.append(ms)
                else:
                    pairs = zip(r_new, r_old) if isinstance(r_new, tuple) else [(r_new, r_old)]
                    same = all(bool(torch.equal(x.t.reshape(-1), y.t.reshape(-1))) for x, y in pairs)
                del r_new, r_old
            nm, om = statistics.median(new_ms), statistics.median(old_ms)
            per_party[step] = (nm, parties)
            cell = {'field': name, 'elem_bytes': eb, 'l': l, 'n': n, 'step': step, 'us': round(nm * 1e3, 1),
                    'algorithmic_bytes': nbytes, 'GBps': round(nbytes / nm / 1e6, 1), 'composed_us': round(om * 1e3, 1),
                    'composed_over_kernel': round(om / nm, 2), 'same_bytes': same, 'parties_running_it': parties}
            res['cells'].append(cell)
            print(json.dumps(cell), flush=True)
        del subrows, g0, p0
        torch.cuda.empty_cache()
        # the whole protocol, all parties: device events and wall clock (synchronised), both routes in alternating runs
        dev = {'fused': [], 'composed': []}
        wall = {'fused': [], 'composed': []}
        routes = {'fused': lambda: protocols.to_bits(ctx, F, xs, rbits, rdivl, T, l),
                  'composed': lambda: comp.to_bits(F, xs, rbits, rdivl)}
        same = None
        for rep in range(args.reps + 1):
            outs = {}
            for route, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ms, outs[route] = timed(fn)
                torch.cuda.synchronize()
                if rep:
                    dev[route].append(ms)
                    wall[route].append((time.perf_counter() - t0) * 1e3)
            if not rep:
                # fresh polynomials per run: the shares differ, the opened bits must not
                o1, o2 = (protocols.open_(ctx, F, outs[r], T) for r in ('fused', 'composed'))
                want = ((protocols.open_(ctx, F, xs, T).t.reshape(n, 1) >> torch.arange(l, device='cuda')) & 1).reshape(-1)
                same = bool(torch.equal(o1.t, o2.t)) and bool(torch.equal(o1.t.to(torch.int64), want))
            del outs
        fused_ms = statistics.median(dev['fused'])
        whole = {'field': name, 'fused_device_ms': round(fused_ms, 3), 'composed_device_ms': round(statistics.median(dev['composed']), 3),
                 'fused_wall_ms': round(statistics.median(wall['fused']), 3), 'composed_wall_ms': round(statistics.median(wall['composed']), 3),
                 'composed_c_bits_host_ms': round(cbits_ms, 3), 'opened_bits_equal_and_correct': same,
                 'share_of_fused_device_time': {k: round(v * parties / fused_ms, 3) for k, (v, parties) in per_party.items()}}
        res['whole'].append(whole)
        print(json.dumps(whole), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as fh:
            fh.write('| field | l | n | step (one party) | us | algorithmic bytes | GB/s | composed us | composed / kernel | same bytes | parties |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|---|---|\n')
            for c_ in res['cells']:
                fh.write(f"| {c_['field']} | {c_['l']} | {c_['n']} | {c_['step']} | {c_['us']} | {c_['algorithmic_bytes']} | {c_['GBps']} | "
                         f"{c_['composed_us']} | {c_['composed_over_kernel']} | {c_['same_bytes']} | {c_['parties_running_it']} |\n")
            fh.write('\n| field | fused device ms | composed device ms | fused wall ms | composed wall ms | host c_bits ms | bits equal and correct | share of fused device time |\n')
            fh.write('|---|---|---|---|---|---|---|---|\n')
            for w in res['whole']:
                fh.write(f"| {w['field']} | {w['fused_device_ms']} | {w['composed_device_ms']} | {w['fused_wall_ms']} | {w['composed_wall_ms']} | "
                         f"{w['composed_c_bits_host_ms']} | {w['opened_bits_equal_and_correct']} | {json.dumps(w['share_of_fused_device_time'])} |\n")


if __name__ == '__main__':
    main()
