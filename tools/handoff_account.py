#!/usr/bin/env python3
"""Where the bytes of the headline step go under the cache hand-off (profiles/r19_handoff_account.md).

  handoff_account.py drive
      the library's own pair on four rotating buffer sets, n = 10^7 over 2^61 - 1, m = 3, t = 1: eight device copies
      (k_copy16: exactly 80 MB in, 80 MB out -- the calibration), then 48 steps of fused share generation and recombination
      on one stream with nothing in between.  Run it under
          rocprofv3 --kernel-trace --pmc FETCH_SIZE  (and again with --pmc WRITE_SIZE)
      with FFGPU_HANDOFF=1 and with FFGPU_HANDOFF=0: four runs, one counter each.
  handoff_account.py summarize NAME=counter_collection.csv ...
      per kernel and run: launches, median and mean of the counter over the settled launches (the first eight of a kernel
      are dropped: the tracker settles in the first step, the clocks later), in MB (counter x 1024; FETCH_SIZE NOT doubled:
      the copy line of the same run says what a known 80 MB reads as).
  handoff_account.py summarize-probe PROBE_STDOUT NAME=counter_collection.csv ...
      the same for `tune_handoff counters`: the calibration launches, then per line of the probe (160 launches, writer and
      reader alternating, the last 80 counted) the median counter of the writer and of the reader.
"""
import collections
import csv
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTLE = 8


def drive():
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from mpyc_amd.engine import FieldContext
    from mpyc_amd import finfields as gff, thresha as gth
    torch.cuda.set_device(0)
    n, t, m = 10_000_000, 1, 3
    k = 2 * t + 1
    gen = torch.Generator(device='cuda:0')
    gen.manual_seed(1)
    ctx = FieldContext(bench.P61, device=0)
    sets = [bench.StepData(ctx, n, t, m, gen) for _ in range(4)]
    lam = list(gth._recombination_vector(gff.GF(bench.P61), tuple(range(1, k + 1)), 0))
    for s in sets:
        s.rec = ctx.recombine_plan([s.shares.row(j) for j in range(k)], lam, s.y)
    for rep in range(2):
        for s in sets:
            ctx.copy(s.a.t, s.c.t)
    torch.cuda.synchronize()
    for rep in range(12):
        for s in sets:
            ctx.split(s.a, s.coef, t, m, out=s.shares, mul_by=s.b)
            s.rec()
    torch.cuda.synchronize()
    ctx.mul(sets[0].a, sets[0].b, out=sets[0].c)
    assert torch.equal(sets[0].y.t, sets[0].c.t)
    print('handoff account: drive done, FFGPU_HANDOFF=%s' % os.environ.get('FFGPU_HANDOFF', '(unset: 1)'))


def rows_of(path):
    rows = list(csv.DictReader(open(path)))
    if rows and 'Dispatch_Id' in rows[0]:
        rows.sort(key=lambda r: int(r['Dispatch_Id']))
    for r in rows:
        r['name'] = re.sub(r'\(.*', '', r['Kernel_Name']).replace('void ffgpu::', '').replace('void ', '')
        r['mb'] = float(r['Counter_Value']) * 1024 / 1e6
    return rows


def line(label, v):
    return '| %s | %d | %.1f | %.1f | %.1f..%.1f |' % (label, len(v), statistics.median(v), statistics.fmean(v), min(v), max(v))


HEAD = '| run / kernel | launches counted | median MB | mean MB | min..max MB |\n|---|---|---|---|---|'


def summarize(args):
    print(HEAD)
    for arg in args:
        tag, path = arg.split('=', 1)
        by = collections.OrderedDict()
        for r in rows_of(path):
            by.setdefault((r['Counter_Name'], r['name']), []).append(r['mb'])
        for (cname, kname), v in by.items():
            if not kname.startswith('k_'):
                continue
            v = v[SETTLE:] if len(v) > 2 * SETTLE else v
            print(line('%s %s `%s`' % (tag, cname, kname), v))


def summarize_probe(args):
    names = [ln.split('  writer')[0].strip() for ln in open(args[0]) if '  writer ' in ln]
    print(HEAD)
    for arg in args[1:]:
        tag, path = arg.split('=', 1)
        rows = rows_of(path)
        cname = rows[0]['Counter_Name']
        for r in rows:
            if r['name'].startswith('k_calib'):
                print('| %s %s `%s` grid %s | 1 | %.1f | | |' % (tag, cname, r['name'], r['Grid_Size'], r['mb']))
        pair = [r for r in rows if r['name'].startswith(('k_writer', 'k_reader'))]
        assert len(pair) == 160 * len(names), (len(pair), len(names))
        for i, nm in enumerate(names):
            timed = pair[160 * i + 80:160 * (i + 1)]
            print(line('%s %s %s: writer' % (tag, cname, nm), [r['mb'] for r in timed if r['name'].startswith('k_writer')]))
            print(line('%s %s %s: reader' % (tag, cname, nm), [r['mb'] for r in timed if r['name'].startswith('k_reader')]))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else ''
    if mode == 'drive':
        drive()
    elif mode == 'summarize':
        summarize(sys.argv[2:])
    elif mode == 'summarize-probe':
        summarize_probe(sys.argv[2:])
    else:
        sys.exit(__doc__)
