"""Threshold SHA-3 on the device: what a secure Keccak-f[1600] round, a permutation and a SHA3-256 hash cost for a batch of
states, all parties on one GPU.  Device events, medians of five alternating passes.

  round / permutation   ffgm_gf2_keccak_round for all 2t+1 senders (steady state: a pending block in, a block out) and
                        protocols.keccak_f1600 (24 rounds + tail; eager, and replayed from one HIP graph), each as a
                        fraction of the library's device copy of the same algorithmic bytes IN THE SAME PASS: per state and
                        sender k * 1600 bytes in and m * 1600 out;
  ChaCha8 / ChaCha20    the round with a host key and 8 or 20 ChaCha rounds: what the keystream's share of the time is;
  composed              the same permutation from what the library offered before the round kernels: per party the
                        element-wise / roll / strided-copy steps of demos/sha3.py:84-103 as device tensor operations, and
                        chi's product through protocols.multiply (share generation with the fused product + recombination);
  hashes                protocols.sha3 (SHA3-256) of a batch of 32-byte messages per second.

    python tools/keccak_probe.py [--out profiles/keccak_kernels.md] [--composed-max 10000]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpyc_amd import finfields as gff, gfpx as ggx, protocols                     # noqa: E402
from mpyc_amd.engine import CapturedLaunches, DevArray, FieldContext              # noqa: E402

B = 1600
TRI = tuple((i + 1) * (i + 2) // 2 % 64 for i in range(24))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def medians(variants, passes=5):
    """{name: median ms} over `passes` alternating passes through the variants (one untimed pass first)"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(passes):
        for name, fn in variants.items():
            ms[name].append(timed(fn))
    return {name: statistics.median(v) for name, v in ms.items()}


def composed_f1600(ctx, F, parts, t, rng):
    """keccak_f1600 of demos/sha3.py:72-106 per party on (nstates, 5, 5, 64) byte tensors [state, y, x, z]"""
    for r in range(24):
        nxt = []
        for A in parts:
            C = A[:, 0] ^ A[:, 1] ^ A[:, 2] ^ A[:, 3] ^ A[:, 4]
            D = torch.roll(C, 1, 1) ^ torch.roll(torch.roll(C, -1, 1), 1, 2)
            A = A ^ D[:, None]
            Bm = A.clone()
            x, y = 1, 0
            for shift in TRI:
                lane = A[:, y, x]
                x, y = y, (2 * x + 3 * y) % 5
                Bm[:, y, x] = torch.roll(lane, shift, 1)
            nxt.append(Bm)
        n = nxt[0].numel()
        u = [DevArray(ctx, (torch.roll(Bm, -1, 2) ^ 1).reshape(-1), n) for Bm in nxt]
        v = [DevArray(ctx, torch.roll(Bm, -2, 2).reshape(-1), n) for Bm in nxt]
        prod = protocols.multiply(ctx, F, u, v, t, rng)
        parts = []
        for Bm, p in zip(nxt, prod):
            A = Bm ^ p.t.view_as(Bm)
            for j in range(7):
                if (RC[r] >> ((1 << j) - 1)) & 1:
                    A[:, 0, 0, (1 << j) - 1] ^= 1
            parts.append(A)
    return parts


def rc_bit(i):
    v = 1
    for _ in range(i % 255):
        v <<= 1
        if v & 0x100:
            v ^= 0x171
    return v & 1


RC = [sum(rc_bit(7 * r + j) << ((1 << j) - 1) for j in range(7)) for r in range(24)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--composed-max', type=int, default=10**4)
    ap.add_argument('--states', type=int, nargs='*', default=[10**4, 10**5])
    args = ap.parse_args()
    lines = ['| field | (m, t) | states | round us | x copy | ChaCha8 / ChaCha20 round us | permutation ms (eager / graph) | x copy | composed ms | composed / kernels | SHA3-256 hashes/s |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    gen = torch.Generator(device='cuda:0')
    gen.manual_seed(7)
    for modulus, m, t in ((0b111, 3, 1), (0b1011, 7, 3)):
        ctx = FieldContext(modulus, True, device=0)
        F = gff.GF(ggx.GFpX(2)(modulus))
        k = 2 * t + 1
        for nstates in args.states:
            n = B * nstates
            bits = DevArray(ctx, torch.randint(0, 2, (n,), dtype=torch.uint8, device='cuda:0', generator=gen), n)
            S = protocols.as_matrix(ctx, protocols.share(ctx, bits, t, m))
            st = ctx.rng_state()
            blk = ctx.keccak_round([S.row(0)], [1], nstates, t, m, stride_in=S.stride, state=st)
            st.commit()
            lam = protocols._lagrange(F, range(1, k + 1))
            rows = [blk.row(s) for s in range(k)]
            out = ctx.empty_matrix(m * k, n)
            half = k * (k + m) * n // 2 // 16 * 16                      # a copy of X bytes reads X and writes X
            src = torch.randint(0, 255, (half,), dtype=torch.uint8, device='cuda:0', generator=gen)
            dst = torch.empty_like(src)

            def one_round():
                ctx.keccak_round(rows, lam, nstates, t, m, iota_round=3, stride_in=k * blk.stride, out=out, state=st)
                st.pending = 0                                          # the probe re-uses one nonce: no advance kernel in the timing

            def host_key_round(rounds):                                  # the same launch drawing ChaCha8 / ChaCha20 coefficients
                return lambda: ctx.keccak_round(rows, lam, nstates, t, m, iota_round=3, stride_in=k * blk.stride, out=out,
                                                key=bytes(32), nonce=5, rounds=rounds)

            variants = {'round': one_round, 'copy': lambda: ctx.copy(src, dst), 'c8': host_key_round(8), 'c20': host_key_round(20),
                        'perm': lambda: protocols.keccak_f1600(ctx, F, S, nstates, t, rng=st)}
            cg = None
            if nstates <= 10**4:
                cg = CapturedLaunches(lambda: protocols.keccak_f1600(ctx, F, S, nstates, t, rng=st))
                variants['graph'] = cg.replay
            msg = DevArray(ctx, torch.randint(0, 2, (256 * nstates,), dtype=torch.uint8, device='cuda:0', generator=gen), 256 * nstates)
            M = protocols.as_matrix(ctx, protocols.share(ctx, msg, t, m))
            variants['sha3'] = lambda: protocols.sha3(ctx, F, M, 256, nstates, t, rng=st)
            parts = None
            if nstates <= args.composed_max:
                parts = [S.row(j).t.reshape(nstates, 5, 5, 64).clone() for j in range(m)]
                variants['composed'] = lambda: composed_f1600(ctx, F, parts, t, st)
            ms = medians(variants)
            if parts is not None:                                       # both routes open to the same permutation
                a = protocols.open_(ctx, F, [DevArray(ctx, p.reshape(-1), n) for p in composed_f1600(ctx, F, parts, t, st)], t)
                res = protocols.keccak_f1600(ctx, F, S, nstates, t, rng=st)
                b = protocols.open_(ctx, F, [res.row(j) for j in range(m)], t)
                assert torch.equal(a.t, b.t), 'the two routes disagree'
            lines.append('| GF(%d) | (%d, %d) | %d | %.1f | %.2f | %.1f / %.1f | %.2f / %s | %.2f | %s | %s | %.3g |' % (
                1 << (modulus.bit_length() - 1), m, t, nstates, ms['round'] * 1e3, ms['round'] / ms['copy'], ms['c8'] * 1e3, ms['c20'] * 1e3, ms['perm'],
                '%.2f' % ms['graph'] if cg else '-', ms['perm'] / (24 * ms['copy']),
                '%.1f' % ms['composed'] if parts is not None else '-',
                '%.0f' % (ms['composed'] / ms['perm']) if parts is not None else '-', nstates / ms['sha3'] * 1e3))
            print(lines[-1], flush=True)
            del S, blk, out, src, dst, M, parts, cg
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
