#!/usr/bin/env python3
"""Device time of the 2-D correlation of a secure convolution layer: the direct kernel (FieldContext.conv2d, ffgm_conv2d, all
senders in one launch) against the composed route the library offered before it for the same tensors -- per sender an im2col
gather with torch indexing on the limb tensors (a zero element appended for the halo), ctx.matmul with M = k m n, K = r s^2,
N = v, and the bias add --, in alternating runs with a byte comparison of the results, peak memory of both routes, and the
yardstick measured in the same process: the v_mad_u64_u32 issue rate (ffgpu_valu_probe), from which the issue bound of the
kernel's own multiply-add count follows (MADS_PER_TERM: v_mad_u64_u32 per multiply-accumulate in the kernel's inner loop).
Generous to the composed route: its index tensor, the transposed weights and the broadcast bias are built outside the timed
region, and its (k, m, n, v) result is not brought into the (k, v, m, n) layout (only for the comparison).
Then one whole protocols.conv_layer (conv2d -> maxpool2x2 -> relu, three parties, t = 1) per shape at batch 1 and 8, eager
and captured in a HIP graph, on randomness drawn beforehand.
usage: conv2d_probe.py [--out FILE.json] [--reps N] [--fields p69,p46,p61,p80] [--batches 1,8,64] [--no-layer]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

FIELDS = {'p69': 2**69 - 93, 'p46': 2**46 - 21, 'p61': 2**61 - 1, 'p80': 2**80 - 65}    # SecInt(37), SecFxp(10, 4), two more
MADS_PER_TERM = {'p69': 16, 'p46': 4, 'p61': 4, 'p80': 16}       # 4 x 4 digits of 28 bits; a 64 x 64 product in 32-bit halves
LAYERS = {'layer1': (1, 28, 28, 32, 5), 'layer2': (32, 14, 14, 64, 5)}                 # (r, m, n, v, s) of the demo
LAYER_BITS = {'p69': {'layer1': 16, 'layer2': 23}, 'p46': {'layer1': 10, 'layer2': 10}}  # the demo's bit lengths
NSEND = 3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def rand_elems(engine, ctx, rs, count, bound=None):
    """count canonical elements below bound (default: the modulus) on the device"""
    p = ctx.modulus
    w = rs.integers(0, 2**64, size=(3, count), dtype=np.uint64).astype(object)
    vals = ((w[0] << 128) ^ (w[1] << 64) ^ w[2]) % (bound or p)
    return ctx.from_ints(vals)


def im2col_index(k, r, m, n, s, device):
    """(k m n, r s^2) indices into x with one zero element appended at index k r m n: the halo"""
    i, I, J = torch.meshgrid(torch.arange(k), torch.arange(m), torch.arange(n), indexing='ij')
    l, di, dj = torch.meshgrid(torch.arange(r), torch.arange(s), torch.arange(s), indexing='ij')
    row = I.reshape(-1, 1) + di.reshape(1, -1) - (s - 1) // 2
    col = J.reshape(-1, 1) + dj.reshape(1, -1) - s // 2
    idx = ((i.reshape(-1, 1) * r + l.reshape(1, -1)) * m + row) * n + col
    idx[(row < 0) | (row >= m) | (col < 0) | (col >= n)] = k * r * m * n
    return idx.to(device)


class Composed:
    """the composed route for one sender's tensors"""

    def __init__(self, engine, ctx, x, W, b, dims, idx):
        k, r, m, n, v, s = dims
        self.engine, self.ctx, self.dims, self.idx = engine, ctx, dims, idx
        zero = torch.zeros_like(x.t[:1])
        self.xpad = torch.cat([x.t, zero])
        K = r * s * s
        self.Wt = engine.DevArray(ctx, W.t.reshape((v, K) + tuple(W.t.shape[1:])).transpose(0, 1).contiguous().reshape((K * v,) + tuple(W.t.shape[1:])), K * v)
        rows = k * m * n
        self.brow = engine.DevArray(ctx, b.t.reshape((1, v) + tuple(b.t.shape[1:])).expand((rows, v) + tuple(b.t.shape[1:])).contiguous()
                                    .reshape((rows * v,) + tuple(b.t.shape[1:])), rows * v)

    def run(self):
        k, r, m, n, v, s = self.dims
        M, K = k * m * n, r * s * s
        cols = self.xpad[self.idx]                                         # (M, K[, limbs]): s^2 copies of x
        cols = self.engine.DevArray(self.ctx, cols.reshape((M * K,) + tuple(cols.shape[2:])), M * K)
        y = self.ctx.matmul(cols, self.Wt, M, K, v)
        return self.ctx.add(y, self.brow, out=y)

    def in_kernel_layout(self, y):
        k, r, m, n, v, s = self.dims
        t = y.t.reshape((k, m * n, v) + tuple(y.t.shape[1:])).transpose(1, 2).contiguous()
        return t.reshape(-1)


class Replay:
    """a supplier of randomness recorded once (eager) and handed out again in the same order"""

    def __init__(self, fn):
        self.fn, self.tape, self.pos, self.recording = fn, [], 0, True

    def __call__(self, *a):
        if self.recording:
            self.tape.append(self.fn(*a))
            return self.tape[-1]
        self.pos += 1
        return self.tape[self.pos - 1]

    def rewind(self):
        self.recording, self.pos = False, 0


def layer_cells(engine, protocols, gff, name, reps):
    p = FIELDS[name]
    ctx, F = gff._context(gff.GF(p)), gff.GF(p)
    rs = np.random.default_rng(5)
    cells = []
    t, parties = 1, 3
    f = 4 if name == 'p46' else 0
    for lname, (r, m, n, v, s) in LAYERS.items():
        l = LAYER_BITS[name][lname]
        for k in (1, 8):
            R = protocols.Randomness(ctx, F, t, parties, b'conv2d probe')
            rand, rtr = Replay(R.rand_compare(l)), Replay(R.rand_trunc)
            # small inputs (x, W in {0, 1}, b in [0, 16)), every party holding the value itself: a sharing of degree 0
            xs = [rand_elems(engine, ctx, rs, k * r * m * n, 2)] * parties
            ws = [rand_elems(engine, ctx, rs, v * r * s * s, 2)] * parties
            bs = [rand_elems(engine, ctx, rs, v, 16)] * parties
            state = ctx.rng_state()

            def layer():
                rand.pos = rtr.pos = 0
                return protocols.conv_layer(ctx, F, xs, ws, bs, k, r, m, n, v, s, t, l, rand, rng=state, f=f, rand_trunc=rtr)
            layer()                                                        # records the draws
            rand.rewind(), rtr.rewind()
            torch.cuda.synchronize()
            eager = [timed(layer)[0] for _ in range(reps + 1)][1:]
            cg = engine.CapturedLaunches(layer, warmup=1)
            graph = [timed(cg.replay)[0] for _ in range(reps + 1)][1:]
            cell = {'field': name, 'layer': lname, 'k': k, 'l': l, 'f': f, 'eager_ms': eager, 'graph_ms': graph,
                    'eager_median_ms': statistics.median(eager), 'graph_median_ms': statistics.median(graph)}
            cells.append(cell)
            print(json.dumps(cell), flush=True)
            del cg
            torch.cuda.empty_cache()
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fields', default=','.join(FIELDS))
    ap.add_argument('--batches', default='1,8,64')
    ap.add_argument('--no-layer', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from mpyc_amd import engine, finfields as gff, protocols
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'senders': NSEND, 'cells': [], 'layers': []}
    rs = np.random.default_rng(9)
    for name in args.fields.split(','):
        p = FIELDS[name]
        ctx = gff._context(gff.GF(p))
        eb = ctx.elem_bytes
        mad_rate = ctx.valu_probe(2)[0]
        res[name] = {'elem_bytes': eb, 'mad_u64_u32_lane_ops_per_s': mad_rate, 'mads_per_term': MADS_PER_TERM[name]}
        print(name, res[name], flush=True)
        for lname, (r, m, n, v, s) in LAYERS.items():
            for k in (int(q) for q in args.batches.split(',')):
                dims = (k, r, m, n, v, s)
                nx, nw, ny = k * r * m * n, v * r * s * s, k * v * m * n
                xs = [rand_elems(engine, ctx, rs, nx) for _ in range(NSEND)]
                ws = [rand_elems(engine, ctx, rs, nw) for _ in range(NSEND)]
                bs = [rand_elems(engine, ctx, rs, v) for _ in range(NSEND)]
                idx = im2col_index(k, r, m, n, s, 'cuda')
                routes = [Composed(engine, ctx, x, W, b, dims, idx) for x, W, b in zip(xs, ws, bs)]
                pl = ctx.conv2d_plan(*dims, nsend=NSEND)
                new_ms, par_ms, new_peak, par_peak, same = [], [], 0, 0, None
                for rep in range(args.reps + 1):                        # rep 0 warms both routes up
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    ms, y_new = timed(lambda: ctx.conv2d(xs, ws, bs, *dims))
                    new_peak = max(new_peak, torch.cuda.max_memory_allocated() - base)
                    if rep:
                        new_ms.append(ms)
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    ms, y_par = timed(lambda: [c.run() for c in routes])
                    par_peak = max(par_peak, torch.cuda.max_memory_allocated() - base)
                    if rep:
                        par_ms.append(ms)
                    elif same is None:
                        same = all(bool(torch.equal(a.t.reshape(-1), c.in_kernel_layout(y))) for a, y, c in zip(y_new, y_par, routes))
                    del y_new, y_par
                    torch.cuda.empty_cache()
                terms = NSEND * ny * r * s * s
                new_med, par_med = statistics.median(new_ms), statistics.median(par_ms)
                bound_ms = terms * MADS_PER_TERM[name] / mad_rate * 1e3
                cell = {'field': name, 'layer': lname, 'k': k, 'wide': pl.wide, 'grid': list(pl.grid), 'lds_bytes': pl.lds_bytes,
                        'new_ms': new_ms, 'parent_ms': par_ms, 'new_median_ms': new_med, 'parent_median_ms': par_med,
                        'new_peak_bytes': new_peak, 'parent_peak_bytes': par_peak, 'tensor_bytes': NSEND * (nx + nw + v + ny) * eb,
                        'same_bytes': same, 'terms': terms, 'new_GMACps': terms / new_med / 1e6, 'issue_bound_ms': bound_ms,
                        'share_of_issue_bound': bound_ms / new_med}
                res['cells'].append(cell)
                print(json.dumps(cell), flush=True)
                del xs, ws, bs, idx, routes
                torch.cuda.empty_cache()
        if not args.no_layer and name in LAYER_BITS:
            res['layers'] += layer_cells(engine, protocols, gff, name, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
