#!/usr/bin/env python3
"""Device time of the local steps of the secure comparison (ffgpu_sgn_expand with e and nx, with e only, ffgpu_sgn_mask)
against (a) the library's copy yardstick (ffgpu_time_copy) moving the same number of bytes in the same run and (b) the
same outputs composed from the calls the engine had before these kernels (matmul with the power vector, element-wise
calls, a transposed copy, scan), in alternating runs by device events.  The public operands of the composed route
(c mod 2^l, c_bits) are uploaded before the clock starts, which favours it: np_sgn builds them on the host per call.
Per cell: median microseconds of both routes, algorithmic bytes (what the step must read and write), the fraction of the
copy rate the kernel reaches, the ratio to the composed route, and whether both routes gave the same bytes.  The odd n is there for the 24-byte fields: with n odd every other output row
starts off the 16-byte boundary the wave-contiguous stores need and takes three 8-byte stores per lane instead.

One field per process keeps a step short; run the fields as separate steps, each under its own time limit:
    timeout -k 10 300 python tools/sgn_probe.py --fields p64 --out out/sgn_p64.json && \\
    timeout -k 10 300 python tools/sgn_probe.py --fields p80 --out out/sgn_p80.json && \\
    timeout -k 10 300 python tools/sgn_probe.py --fields p136 --out out/sgn_p136.json
usage: sgn_probe.py [--out FILE.json] [--md FILE.md] [--reps N] [--fields p64,p80,p136] [--shapes 32x1000000,64x1000000,32x1000001]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch         # noqa: E402

FIELDS = {'p64': 2**64 - 189, 'p80': 2**80 - 65, 'p136': 2**136 - 113}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def random_elements(ctx, count):
    """`count` canonical field elements on the device: random limbs through ffgpu_reduce"""
    from mpyc_amd.engine import DevArray, _torch_dtype
    eb = ctx.elem_bytes
    raw = torch.randint(-2**63, 2**63 - 1, ((count * eb + 7) // 8,), dtype=torch.int64, device='cuda')
    raw = raw.view(torch.uint8)[:count * eb].view(_torch_dtype(eb))
    return ctx.reduce(DevArray(ctx, raw.reshape((count, ctx.limbs) if ctx.limbs else (count,)), count))


def low64_elements(ctx, v):
    """field elements from an int64 tensor holding values below 2^64 (as bit patterns)"""
    from mpyc_amd.engine import DevArray, _torch_dtype
    eb, n = ctx.elem_bytes, v.shape[0]
    if not ctx.limbs:
        return DevArray(ctx, v.to(_torch_dtype(eb)), n)
    t = torch.zeros((n, ctx.limbs), dtype=_torch_dtype(eb), device=v.device)
    if eb == 12:
        t[:, 0] = (v & 0xffffffff).to(torch.int32)
        t[:, 1] = ((v >> 32) & 0xffffffff).to(torch.int32)
    else:
        t[:, 0] = v
    return DevArray(ctx, t, n)


class Composed:
    """the three local steps from the calls that existed before the sgn kernels"""

    def __init__(self, ctx, l, n, c):
        from mpyc_amd.engine import DevArray
        self.ctx, self.l, self.n, self.DevArray = ctx, l, n, DevArray
        self.pw = ctx.from_ints([1 << (l - 1 - i) for i in range(l)])
        # the public operands, built on the device here (np_sgn builds them on the host and uploads them)
        t = c.t
        if ctx.elem_bytes == 12:
            lo = (t[:, 0].to(torch.int64) & 0xffffffff) | (t[:, 1].to(torch.int64) << 32)
        else:
            lo = t[:, 0] if ctx.limbs else t
        cl = lo if l == 64 else lo & ((1 << l) - 1)
        self.CL = low64_elements(ctx, cl)
        self.CB = low64_elements(ctx, torch.stack([(cl >> (l - 1 - i)) & 1 for i in range(l)]).reshape(-1))
        self.ones = ctx.from_ints([1] * n)

    def cat(self, ts):
        t = torch.cat([x.t for x in ts])
        return self.DevArray(self.ctx, t, t.shape[0])

    def a_r(self, a, rbits):
        ctx, l = self.ctx, self.l
        return ctx.add_scalar(ctx.add(a, ctx.matmul(rbits, self.pw, self.n, l, 1)), 1 << l)

    def mask(self, a, rbits, rdivl):
        ctx = self.ctx
        return ctx.add(self.a_r(a, rbits), ctx.mul_scalar(rdivl, (1 << self.l) % ctx.modulus))

    def expand(self, a, rbits, sbit, want_nx):
        ctx, l, n = self.ctx, self.l, self.n
        z = ctx.sub(self.CL, self.a_r(a, rbits))
        rt = rbits.t.reshape((n, l) + tuple(rbits.t.shape[1:])).transpose(0, 1).contiguous()
        rT = self.DevArray(ctx, rt.reshape((n * l,) + tuple(rbits.t.shape[1:])), n * l)
        xor = ctx.sub(ctx.add(self.CB, rT), ctx.mul_scalar(ctx.mul(self.CB, rT), 2))
        sums = ctx.scan(xor, 1, l, n, with_initial=True)
        s = ctx.add_scalar(ctx.mul_scalar(sbit, 2), ctx.modulus - 1)
        e = ctx.add(ctx.sub(self.cat([s] * (l + 1)), self.cat([ctx.sub(self.CB, rT), self.ones])), ctx.mul_scalar(sums, 3))
        return e, (ctx.rsub_scalar(xor, 1) if want_nx else None), z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fields', default=','.join(FIELDS))
    ap.add_argument('--shapes', default='32x1000000,64x1000000,32x1000001')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from mpyc_amd.engine import FieldContext
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'cells': []}
    for name in args.fields.split(','):
        p = FIELDS[name]
        ctx = FieldContext(p, device=0)
        eb = ctx.elem_bytes
        for shape in args.shapes.split(','):
            l, n = (int(v) for v in shape.split('x'))
            if l > p.bit_length() - 2:
                cell = {'field': name, 'l': l, 'n': n, 'skipped': 'l > bit_length(p) - 2: not a valid call for this field'}
                res['cells'].append(cell)
                print(json.dumps(cell), flush=True)
                continue
            a, sbit, rdivl, c = (random_elements(ctx, n) for _ in range(4))
            rbits = random_elements(ctx, n * l)
            comp = Composed(ctx, l, n, c)
            steps = {
                'expand e+nx': (lambda: ctx.sgn_expand(c, a, rbits, sbit, l, want_e=True, want_nx=True),
                                lambda: comp.expand(a, rbits, sbit, True), (n * l + 3 * n) + ((2 * l + 1) * n + n)),
                'expand e': (lambda: ctx.sgn_expand(c, a, rbits, sbit, l, want_e=True, want_nx=False),
                             lambda: comp.expand(a, rbits, sbit, False), (n * l + 3 * n) + ((l + 1) * n + n)),
                'mask': (lambda: ctx.sgn_mask(a, rbits, rdivl, l), lambda: comp.mask(a, rbits, rdivl), (n * l + 2 * n) + n),
            }
            for step, (new, old, elems) in steps.items():
                nbytes = elems * eb
                src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device='cuda')  # a copy reads and writes: same bytes moved (whole 16-byte packs)
                dst = torch.empty_like(src)
                new_ms, old_ms, cp_ms, same = [], [], [], None
                for rep in range(args.reps + 1):                                      # rep 0 warms every route up
                    ms, r_new = timed(new)
                    if rep:
                        new_ms.append(ms)
                    ms, r_old = timed(old)
                    if rep:
                        old_ms.append(ms)
                    else:
                        pairs = zip(r_new, r_old) if isinstance(r_new, tuple) else [(r_new, r_old)]
                        same = all(bool(torch.equal(x.t.reshape(-1), y.t.reshape(-1))) for x, y in pairs if x is not None)
                    del r_new, r_old
                    ms = ctx.time_copy(src, dst, 3)
                    if rep:
                        cp_ms.append(ms)
                nm, om, cm = statistics.median(new_ms), statistics.median(old_ms), statistics.median(cp_ms)
                cell = {'field': name, 'elem_bytes': eb, 'l': l, 'n': n, 'step': step, 'us': round(nm * 1e3, 1),
                        'algorithmic_bytes': nbytes, 'GBps': round(nbytes / nm / 1e6, 1), 'copy_us': round(cm * 1e3, 1),
                        'fraction_of_copy_rate': round(cm / nm, 3), 'composed_us': round(om * 1e3, 1),
                        'composed_over_kernel': round(om / nm, 2), 'same_bytes': same}
                res['cells'].append(cell)
                print(json.dumps(cell), flush=True)
                del src, dst
            del a, sbit, rdivl, c, rbits, comp
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as fh:
            fh.write('| field | elem B | l | n | step | us | algorithmic bytes | GB/s | copy us | fraction of copy rate | composed us | composed / kernel | same bytes |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|---|---|---|---|\n')
            for c_ in res['cells']:
                if 'skipped' in c_:
                    fh.write(f"| {c_['field']} | | {c_['l']} | {c_['n']} | {c_['skipped']} | | | | | | | | |\n")
                else:
                    fh.write(f"| {c_['field']} | {c_['elem_bytes']} | {c_['l']} | {c_['n']} | {c_['step']} | {c_['us']} | {c_['algorithmic_bytes']} | "
                             f"{c_['GBps']} | {c_['copy_us']} | {c_['fraction_of_copy_rate']} | {c_['composed_us']} | "
                             f"{c_['composed_over_kernel']} | {c_['same_bytes']} |\n")


if __name__ == '__main__':
    main()
