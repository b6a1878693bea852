#!/usr/bin/env python3
"""Time of a stack of matrix products, batch x (M x K @ K x N), in one process and alternating runs:
  stack   the stack kernels (ffgpu_matmul_stack on a context with FFGPU_MM_STACK_LOOP_MIN at its highest value);
  cloop   the loop over the single-product launcher inside the same entry point (a context with the switch at 0);
  python  finfields._matmul_per_matrix, the per-matrix loop that `@` took before the stack kernels existed.
stack and cloop are timed with device events, python with a host clock around a synchronise (it is host-bound).  One
warm-up round and --reps timed rounds; median and range.  The crossover of stack and cloop is the default of
FFGPU_MM_STACK_LOOP_MIN.  Yardsticks of the same run: the HBM copy rate (ffgpu_copy) for the packed shape, k_matmul's
multiply-accumulate rate on ONE matrix of the same total work (FFGPU_MM_MFMA=0) for the tiled one.  Routes whose
estimated time passes --cap-s are not run and reported as "not measured"; cells whose operands pass --cap-gb are left out.
usage: matmul_stack_probe.py [--out FILE.json] [--reps 5] [--cap-s 20] [--cap-gb 3] [--fields p61,...] [--shapes 4x4x4,...]
                             [--batches 100,10000,1000000]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

FIELDS = {'p61': (2**61 - 1, False), 'p80': (2**80 - 65, False), 'p128': (2**128 - 173, False),
          'p136': (2**136 - 113, False), 'gf8': (0x11b, True), 'gf64': (0x1000000000000001b, True)}
SHAPES = [(3, 3, 3), (4, 4, 4), (8, 8, 8), (16, 16, 16), (32, 32, 32), (64, 64, 64), (128, 128, 128), (8, 4096, 8)]
BATCHES = [10**2, 10**4, 10**6]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def context(modulus, binary, **env):
    from mpyc_amd import engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return engine.FieldContext(modulus, binary, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def summary(ms):
    if not ms:
        return None
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'runs': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cap-s', type=float, default=20.0, help='a route estimated to take longer per cell is not measured')
    ap.add_argument('--cap-gb', type=float, default=3.0)
    ap.add_argument('--fields', default=','.join(FIELDS))
    ap.add_argument('--shapes', default=None)
    ap.add_argument('--batches', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from mpyc_amd import finfields as gff, gfpx
    from mpyc_amd.engine import DevArray
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in s.split('x')) for s in args.shapes.split(',')]
    batches = BATCHES if not args.batches else [int(x) for x in args.batches.split(',')]
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'cells': []}
    gen = torch.Generator(device='cuda')
    gen.manual_seed(12)
    for name in args.fields.split(','):
        modulus, binary = FIELDS[name]
        F = gff.GF(gfpx.BinaryPolynomial(modulus)) if binary else gff.GF(modulus)
        cls = F.array
        ctx = gff._context(F)                                       # the default context of `@`
        c_stack = context(modulus, binary, FFGPU_MM_STACK_LOOP_MIN=2**31 - 1)
        c_loop = context(modulus, binary, FFGPU_MM_STACK_LOOP_MIN=0)
        c_valu = context(modulus, binary, FFGPU_MM_MFMA=0)
        eb = ctx.elem_bytes
        src = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        ctx.copy(src, dst)
        copy_ms = min(timed(lambda: ctx.copy(src, dst))[0] for _ in range(5))
        copy_gbs = 2 * src.numel() / copy_ms / 1e6                  # read + write
        del src, dst
        res[name] = {'elem_bytes': eb, 'copy_GBps': copy_gbs}
        print(name, res[name], flush=True)

        def arr(*shape):                                            # random bytes, reduced to canonical elements
            n = int(np.prod(shape))
            lb = ctx.limbs
            raw = torch.randint(0, 256, (n * eb,), dtype=torch.uint8, device='cuda', generator=gen)
            t = raw.view(ctx.empty(0).t.dtype).reshape((n, lb) if lb else (n,))
            return cls._wrap(ctx.reduce(DevArray(ctx, t, n)), (n,)).reshape(shape)

        per_call_s = None                                           # host cost of one per-matrix product, learnt as we go
        for M, K, N in shapes:
            for nb in batches:
                gb = (M * K + K * N + M * N) * eb * nb / 1e9
                if gb > args.cap_gb:
                    continue
                forms = [('stack@stack', (nb, M, K), (nb, K, N))]
                if (M, K, N) in ((4, 4, 4), (32, 32, 32)):
                    forms += [('matrix@stack', (M, K), (nb, K, N)), ('stack@matrix', (nb, M, K), (K, N))]
                for form, sa, sb in forms:
                    A, B = arr(*sa), arr(*sb)
                    a_stride = M * K if len(sa) == 3 else 0
                    routes = {}
                    if form == 'stack@matrix':                      # one 2-D product through `@`
                        routes['stack'] = lambda: (A @ B)._dev
                    else:
                        routes['stack'] = lambda: c_stack.matmul_stack(A._dev, B._dev, nb, M, K, N, a_stride, K * N)
                        if nb <= 10**4:
                            routes['cloop'] = lambda: c_loop.matmul_stack(A._dev, B._dev, nb, M, K, N, a_stride, K * N)
                    A3 = A if len(sa) == 3 else A.reshape(1, M, K)
                    B3 = B if len(sb) == 3 else B.reshape(1, K, N)
                    if per_call_s is None or per_call_s * nb * (args.reps + 1) <= args.cap_s:
                        routes['python'] = lambda: gff._matmul_per_matrix(cls, A3, B3, (nb,))._dev
                    ms = {r: [] for r in routes}
                    same = None
                    for rep in range(args.reps + 1):                # rep 0 warms every route up
                        outs = {}
                        for r, fn in routes.items():
                            t, o = (host_timed if r == 'python' else timed)(fn)
                            if rep:
                                ms[r].append(t)
                            else:
                                outs[r] = o
                                if r == 'python':
                                    per_call_s = max(t / 1e3 / nb, 1e-6)
                        if rep == 0:
                            ref = outs['stack'].t.reshape(-1)
                            same = all(bool(torch.equal(ref, o.t.reshape(-1))) for o in outs.values())
                        del outs
                    macs = M * K * N * nb
                    cell = {'field': name, 'form': form, 'M': M, 'K': K, 'N': N, 'batch': nb, 'packed': M * N <= 256,
                            'same_bytes': same, 'operand_GB': gb}
                    for r in ('stack', 'cloop', 'python'):
                        cell[r] = summary(ms.get(r, [])) or 'not measured'
                    med = cell['stack']['median_ms']
                    cell['stack_GBps'] = gb * 1e3 / med
                    cell['stack_GMACps'] = macs / med / 1e6
                    if M * N > 256 and form == 'stack@stack':       # k_matmul on ONE matrix of the same total work
                        side = max(64, int(round(macs ** (1 / 3) / 64)) * 64)
                        if 3 * side * side * eb <= args.cap_gb * 1e9:
                            X = arr(side, side)._dev
                            c_valu.matmul(X, X, side, side, side)
                            t1 = min(timed(lambda: c_valu.matmul(X, X, side, side, side))[0] for _ in range(3))
                            cell['k_matmul_one_matrix'] = {'side': side, 'GMACps': side**3 / t1 / 1e6}
                            del X
                    res['cells'].append(cell)
                    print(json.dumps(cell), flush=True)
                    del A, B, A3, B3
                    torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
