#!/usr/bin/env python3
"""Device time of np.convolve on field arrays: the convolution kernel (FieldContext.convolve) against the composed
Toeplitz route (finfields._convolve_toeplitz, what np.convolve did before the kernel existed), in alternating runs,
with the yardsticks measured in the same process: the HBM copy rate (ffgpu_copy), the v_mad_u64_u32 issue rate
(ffgpu_valu_probe) and the multiply-accumulate rate of k_matmul for the same field (FFGPU_MM_MFMA=0: the VALU kernel).
The composed route is skipped where its two int64 index tensors plus the gathered matrix pass --parent-cap-gb.
usage: convolve_probe.py [--out FILE.json] [--reps N] [--parent-cap-gb 64] [--fields p61,p128,p136,gf64] [--sizes ...]"""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault('FFGPU_MM_MFMA', '0')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

FIELDS = {'p61': (2**61 - 1, False), 'p128': (2**128 - 173, False), 'p136': (2**136 - 113, False),
          'gf64': (0x1000000000000001b, True)}
SIZES = [(10**7, 4), (10**7, 64), (10**6, 1024), (32768, 32768), (4096, 4096), (700, 33), (9, 4)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent-cap-gb', type=float, default=64.0)
    ap.add_argument('--fields', default=','.join(FIELDS))
    ap.add_argument('--sizes', default=None, help='e.g. 4096x4096,700x33')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from mpyc_amd import finfields as gff, gfpx
    sizes = SIZES if not args.sizes else [tuple(int(x) for x in s.split('x')) for s in args.sizes.split(',')]
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'cells': []}
    rs = np.random.default_rng(8)
    for name in args.fields.split(','):
        modulus, binary = FIELDS[name]
        F = gff.GF(gfpx.BinaryPolynomial(modulus)) if binary else gff.GF(modulus)
        ctx = gff._context(F)
        eb = ctx.elem_bytes
        # yardsticks of this field, now
        src = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        ctx.copy(src, dst)
        copy_ms = min(timed(lambda: ctx.copy(src, dst))[0] for _ in range(5))
        copy_gbs = 2 * src.numel() / copy_ms / 1e6                      # read + write
        del src, dst
        mad_rate = ctx.valu_probe(2)[0]
        def arr(n):                                                     # n random canonical elements
            lb = ctx.limbs
            raw = rs.integers(-2**63, 2**63, (n, lb) if lb else (n,), dtype=np.int64)
            return F.array(gff.DevArray(ctx, torch.from_numpy(raw).to('cuda'), n))          # (the ctor reduces)
        M = 1024
        A = arr(M * M)._dev
        ctx.matmul(A, A, M, M, M)
        mm_ms = min(timed(lambda: ctx.matmul(A, A, M, M, M))[0] for _ in range(3))
        mm_rate = M**3 / mm_ms / 1e6                                    # GMAC/s
        del A
        res[name] = {'elem_bytes': eb, 'copy_GBps': copy_gbs, 'mad_u64_u32_lane_ops_per_s': mad_rate, 'k_matmul_GMACps': mm_rate}
        print(name, res[name], flush=True)
        for na, nv in sizes:
            a, v = arr(na), arr(nv)
            nout = na + nv - 1
            parent_gb = (2 * 8 + eb) * nout * nv / 1e9
            run_parent = parent_gb <= args.parent_cap_gb
            new_ms, par_ms, new_peak, par_peak, same = [], [], 0, 0, None
            reps = args.reps if na * nv < 2e9 else max(2, args.reps // 2)
            for rep in range(reps + 1):                                 # rep 0 warms both routes up
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ms, c_new = timed(lambda: ctx.convolve(a._dev, v._dev))
                new_peak = max(new_peak, torch.cuda.max_memory_allocated() - base)
                if rep:
                    new_ms.append(ms)
                if run_parent:
                    torch.cuda.reset_peak_memory_stats()
                    try:
                        ms, c_par = timed(lambda: gff._convolve_toeplitz(type(a), a, v))
                    except torch.OutOfMemoryError:
                        run_parent, par_ms = False, ['out of memory']
                        torch.cuda.empty_cache()
                        continue
                    par_peak = max(par_peak, torch.cuda.max_memory_allocated() - base)
                    if rep:
                        par_ms.append(ms)
                    elif same is None:
                        same = bool(torch.equal(c_new.t.reshape(-1), c_par._dev.t.reshape(-1)))
                    del c_par
                    torch.cuda.empty_cache()
                del c_new
            cell = {'field': name, 'na': na, 'nv': nv, 'new_ms': new_ms, 'parent_ms': par_ms, 'new_peak_bytes': new_peak,
                    'parent_peak_bytes': par_peak, 'parent_index_plus_gather_GB': parent_gb, 'same_bytes': same,
                    'new_median_ms': statistics.median(new_ms),
                    'stream_floor_ms': (2 * na + nv) * eb / copy_gbs / 1e6,
                    'new_GMACps': na * nv / statistics.median(new_ms) / 1e6}
            if par_ms and not isinstance(par_ms[0], str):
                cell['parent_median_ms'] = statistics.median(par_ms)
            res['cells'].append(cell)
            print(json.dumps(cell), flush=True)
            del a, v
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
