"""The two local steps of secure random bits on the device (ffgm_rbits_open / ffgm_rbits_finish, mpyc_amd/csrc/rbits.hpp)
against Python integers computed here from the maps include/ffgpu_math.h states, over every prime policy, at every edge of the
launch plan (mpyc_amd/csrc/rbits_geom.hpp) and with 1, 3, 5 and 7 rows (and 10: past the fused rows); the zero counter (planted
zeros, none, all, accumulated over two calls, absent); guard bytes around every output row and the counter; outputs on their
inputs; status codes; protocols.random_bits on the draws the reference was fed (tests/golden/rbits/rbits.json) and, composed
from sqrt_cl, over three primes = 1 mod 4 of 12, 16 and 24 bytes;
protocols.Randomness share for share against the Python-integer stand-in on the same key; compare_zero, fxp_multiply and
is_zero on nothing but its draws; and open -> finish replayed from a captured HIP graph."""
import os
import re

import numpy as np
import pytest

from test_gpu_sgn import draw, same, view
from test_gpu_fxp import up
from test_gpu_iszero import FIELDS, nonresidue
from test_rbits_host import (BALANCE_KEY, BALANCE_ONES, COMPOSED, ONE_MOD_FOUR, P61, P80, check_end_to_end, golden, gf, open_two_ways,
                             run_end_to_end, run_golden, run_one_mod_four, zero_test_prime)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 3, 5, 7)
RMAX = 7


def geom(name, header='rbits_geom.hpp'):
    src = open(os.path.join(ROOT, 'mpyc_amd', 'csrc', header)).read()
    return int(re.search(name + r'\s*=\s*(\d+)', src).group(1))


THREADS = geom('CX_THREADS', 'sort_geom.hpp')
FUSED, FUSED24, MAX_ROWS = geom('RBITS_FUSED_ROWS'), geom('RBITS_FUSED_ROWS_24'), geom('RBITS_MAX_ROWS')


def pack_of(eb):
    """cx_pack (sort_geom.hpp)"""
    return {4: 4, 8: 2}.get(eb, 1)


def grid_entries(blocks, eb):
    """rbits_grid_entries (rbits_geom.hpp)"""
    return blocks * THREADS * pack_of(eb)


def edge_sizes(eb):
    """n = 1; one pack - 1, one pack, one pack + 1; one block of packs - 1, that, + 1 (and for 24-byte elements, whose packs go in
    waves of 64, one wave +- 1)"""
    pack, block = pack_of(eb), grid_entries(1, eb)
    return sorted({1, max(1, pack - 1), pack, pack + 1, 63, 64, 65, block - 1, block, block + 1})


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def test_the_geometry_restated_here():
    assert (THREADS, FUSED, FUSED24, MAX_ROWS) == (256, 9, 5, 64)
    assert edge_sizes(8) == [1, 2, 3, 63, 64, 65, 511, 512, 513] and edge_sizes(24)[-3:] == [255, 256, 257]


def open_ref(p, r, z, lam):
    """c[h] = sum_i lam[i] (r[i][h]^2 + z[i][h]) on object arrays"""
    acc = 0
    for i, l in enumerate(lam):
        acc = acc + l * (r[i] * r[i] + z[i])
    return acc % p


def finish_ref(p, c, r, signed, f):
    assert p % 4 == 3
    e, half = (3 * p - 5) >> 2, (p + 1) >> 1
    s = np.array([pow(int(v), e, p) for v in c], dtype=object)
    nz = np.array([int(v != 0) for v in c], dtype=object)
    rows = []
    for row in r:
        b = row * s % p
        if not signed:
            b = (b + 1) * half % p
        rows.append((b << f) % p * nz)
    return rows


class Data:
    """RMAX rows r and z of n entries with edge values first, then uniform, and per row count k a first row of z that plants
    zero squares at the first entry, at the last entry of every tested size and at two adjacent ones ('some'), nowhere
    ('none': r and z as drawn) or everywhere ('all'); a case (n, k) is the first n entries of the first k rows"""

    def __init__(self, ctx, p, sizes, seed, rows=RMAX, ks=ROWS):
        rng = np.random.default_rng(seed)
        N = max(sizes)
        self.p, self.N = p, N
        nr = nonresidue(p)
        edge = [0, 1, p - 1, nr, p - nr, 2, (p + 1) >> 1, p - 2]
        self.r = [draw(rng, p, N) for _ in range(rows)]
        self.z = [draw(rng, p, N) for _ in range(rows)]
        for i in range(rows):
            for j, v in enumerate(edge[:N]):
                self.r[i][j] = edge[(i + j) % len(edge)]
                self.z[i][j] = edge[(3 * i + j + 1) % len(edge)]
        self.r[0][:min(N, 4)] = [p - 1, 0, p - 1, 1][:N]                 # (p - 1)^2: the bound of a product
        self.lam = {k: [int(v) for v in draw(rng, p, k)] for k in ks}
        for k in ks:
            self.lam[k][0] = p - 1 if k > 1 else 1
        planted = sorted({0, 7, 8} | {n - 1 for n in sizes})
        self.z0, self.c = {}, {}
        for k in ks:
            rest = open_ref(p, self.r[:k], [0 * self.z[0]] + self.z[1:k], self.lam[k])       # the sum without lam[0] z[0]
            fix = (-rest * pow(self.lam[k][0], -1, p)) % p                                  # the z[0] that makes the square 0
            some = self.z[0].copy()
            idx = [h for h in planted if h < N]
            some[idx] = fix[idx]
            self.z0[k] = {'some': some, 'none': self.z[0], 'all': fix}
            self.c[k] = {kind: open_ref(p, self.r[:k], [z0] + self.z[1:k], self.lam[k]) for kind, z0 in self.z0[k].items()}
            assert not self.c[k]['all'].any() and all(self.c[k]['some'][h] == 0 for h in idx)
        self.d = {'r': [up(ctx, v) for v in self.r], 'z': [up(ctx, v) for v in self.z]}
        self.dz0 = {k: {kind: up(ctx, v) for kind, v in self.z0[k].items()} for k in ks}
        self.dc = {k: {kind: up(ctx, v) for kind, v in self.c[k].items()} for k in ks}


@pytest.mark.parametrize('name', list(FIELDS))
def test_open_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    sizes = edge_sizes(ctx.elem_bytes)
    D = Data(ctx, p, sizes, seed=11 + p % 997)
    keep = [x.t.clone() for x in D.d['r'] + D.d['z']]
    ran = 0
    for n in sizes:
        for k in ROWS:
            rs = [view(engine, ctx, x, 0, n) for x in D.d['r'][:k]]
            for kind in ('some', 'none', 'all'):
                zs = [view(engine, ctx, D.dz0[k][kind], 0, n)] + [view(engine, ctx, x, 0, n) for x in D.d['z'][1:k]]
                cnt = ctx.zero_counter()
                got = ctx.rbits_open(rs, zs, D.lam[k], zeros=cnt)
                want = int(sum(1 for v in D.c[k][kind][:n] if v == 0))
                assert got.n == n and same(got, D.dc[k][kind].t[:n]), ('open', name, n, k, kind)
                assert int(cnt.item()) == want and (kind != 'all' or want == n) and (kind != 'some' or want >= 1), ('count', name, n, k, kind)
                if kind == 'some':                                       # added to, not overwritten; and no counter at all
                    out = ctx.empty(n)
                    assert ctx.rbits_open(rs, zs, D.lam[k], zeros=cnt, out=out) is out and int(cnt.item()) == 2 * want
                    assert same(ctx.rbits_open(rs, zs, D.lam[k]), D.dc[k][kind].t[:n])
                ran += 1
    assert ran == 3 * len(sizes) * len(ROWS)
    # one element into their buffers: the element path
    n, k = sizes[-2], 3
    lead = lambda x: view(engine, ctx, x, 1, n)
    cnt = ctx.zero_counter()
    got = ctx.rbits_open([lead(x) for x in D.d['r'][:k]], [lead(D.dz0[k]['some'])] + [lead(x) for x in D.d['z'][1:k]], D.lam[k], zeros=cnt)
    assert same(got, D.dc[k]['some'].t[1:n]) and int(cnt.item()) == sum(1 for v in D.c[k]['some'][1:n] if v == 0)
    assert all(torch.equal(x.t, k_) for x, k_ in zip(D.d['r'] + D.d['z'], keep)), 'an input was written'


def test_open_past_the_fused_rows(mods):
    """10 rows (and 7 of 24-byte elements) take the run-time row count by elements; 64 rows are the limit"""
    _ffi, engine, _, _ = mods
    for name, k in (('pm64-mersenne', 10), ('pm96', 10), ('pm192', 7), ('mont192', 6), ('pm64-mersenne', 64)):
        p = FIELDS[name]
        ctx = engine.FieldContext(p, device=0)
        assert k > (FUSED24 if ctx.elem_bytes == 24 else FUSED)
        n = grid_entries(1, ctx.elem_bytes) + 1
        D = Data(ctx, p, [n], seed=5 + k, rows=k, ks=(k,))
        cnt = ctx.zero_counter()
        got = ctx.rbits_open(D.d['r'], [D.dz0[k]['some']] + D.d['z'][1:], D.lam[k], zeros=cnt)
        assert same(got, D.dc[k]['some'].t) and int(cnt.item()) == sum(1 for v in D.c[k]['some'] if v == 0) >= 3, (name, k)


BLUM = [name for name, p in FIELDS.items() if p % 4 == 3]


@pytest.mark.parametrize('name', BLUM)
def test_finish_against_python_integers(mods, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    sizes = edge_sizes(ctx.elem_bytes)
    D = Data(ctx, p, sizes, seed=17 + p % 997, ks=(3,))
    N = D.N
    c = D.c[3]['some'].copy()                                            # zeros at every edge; then squares and arbitrary values
    sq = np.array([v * v % p for v in D.r[1]], dtype=object)
    c[16::2] = np.where(c[16::2] == 0, 0, sq[16::2])
    nr = nonresidue(p)
    c[1:6] = [1, p - 1, nr, 4, p - 4]
    dc = up(ctx, c)
    keep = [x.t.clone() for x in D.d['r']] + [dc.t.clone()]
    want = {(s, f): [up(ctx, row) for row in finish_ref(p, c, D.r, s, f)] for s, f in ((False, 0), (True, 0), (False, 16), (True, 3))}
    ran = 0
    for n in sizes:
        for m in ROWS:
            for (s, f), rows in want.items():
                rs = [view(engine, ctx, x, 0, n) for x in D.d['r'][:m]]
                got = ctx.rbits_finish(view(engine, ctx, dc, 0, n), rs, signed=s, f=f)
                assert len(got) == m and all(same(g, w.t[:n]) for g, w in zip(got, rows)), ('finish', name, n, m, s, f)
                ran += 1
    assert ran == 4 * len(sizes) * len(ROWS)
    assert all(torch.equal(x.t, k_) for x, k_ in zip(D.d['r'] + [dc], keep)), 'an input was written'
    # the outputs on their inputs, whole packs and one element in; c is never written
    for lo in (0, 1):
        n = sizes[-1] - 1
        mine = [engine.DevArray(ctx, x.t.clone(), N) for x in D.d['r'][:5]]
        rs = [view(engine, ctx, x, lo, lo + n) for x in mine]
        got = ctx.rbits_finish(view(engine, ctx, dc, lo, lo + n), rs, outs=rs)
        assert all(g is r for g, r in zip(got, rs)) and all(same(r, w.t[lo:lo + n]) for r, w in zip(rs, want[False, 0])), ('in place', name, lo)
        assert all(torch.equal(x.t[lo + n:], k_[lo + n:]) and torch.equal(x.t[:lo], k_[:lo]) for x, k_ in zip(mine, keep)), 'past the view'
    assert torch.equal(dc.t, keep[-1])
    # 64 rows: the limit
    rs = [D.d['r'][i % RMAX] for i in range(MAX_ROWS)]
    got = ctx.rbits_finish(dc, rs, signed=True)
    assert all(same(g, want[True, 0][i % RMAX].t) for i, g in enumerate(got))


@pytest.mark.parametrize('name', ['pm64-mersenne', 'pm96', 'pm192'])
def test_one_entry_past_the_saturated_grid(mods, monkeypatch, name):
    """FFGPU_BLOCKS_PER_CU=1: the grid is the CUs; with one entry more than a pack per thread the loop of a thread iterates
    (24-byte elements: one wave more, and an element tail)"""
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    monkeypatch.setenv('FFGPU_BLOCKS_PER_CU', '1')
    ctx = engine.FieldContext(p, device=0)
    monkeypatch.delenv('FFGPU_BLOCKS_PER_CU')
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = grid_entries(cus, ctx.elem_bytes) + (65 if ctx.elem_bytes == 24 else 1)
    k = 3
    D = Data(ctx, p, [n, n // 2], seed=3, rows=k, ks=(k,))
    cnt = ctx.zero_counter()
    got = ctx.rbits_open(D.d['r'], [D.dz0[k]['some']] + D.d['z'][1:], D.lam[k], zeros=cnt)
    assert same(got, D.dc[k]['some'].t) and int(cnt.item()) == sum(1 for v in D.c[k]['some'] if v == 0) >= 4
    c = np.array([v * v % p for v in D.r[1]], dtype=object)
    c[[0, n // 2, n - 1]] = 0
    rows = finish_ref(p, c, D.r[:2], False, 0)
    fin = ctx.rbits_finish(up(ctx, c), D.d['r'][:2])
    assert all(same(g, up(ctx, w).t) for g, w in zip(fin, rows))


# ---- guard bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rc32', 'pm64-k64', 'pm96', 'pm128', 'pm192'])
@pytest.mark.parametrize('n,k', [(320, 3), (301, 5)])
def test_nothing_is_written_outside_the_outputs(mods, name, n, k):
    """n = 320: whole packs (and whole waves of 24-byte elements); n = 301: packs and the tail, or elements throughout"""
    import ctypes
    _ffi, engine, _, _ = mods
    p, pad = FIELDS[name], 240                                          # 240: a multiple of every element size and of 16
    ctx = engine.FieldContext(p, device=0)
    eb = ctx.elem_bytes
    D = Data(ctx, p, [n], seed=79, rows=k, ks=(k,))
    rs, zs = D.d['r'], [D.dz0[k]['some']] + D.d['z'][1:]
    keep = [x.t.clone() for x in rs + zs]

    def guarded(nbytes):
        buf = torch.full((pad + nbytes + pad,), 0xa5, dtype=torch.uint8, device='cuda')
        return buf, buf.data_ptr() + pad

    def check(buf, nbytes, want_bytes):
        assert bool((buf[:pad] == 0xa5).all()) and bool((buf[pad + nbytes:] == 0xa5).all()), 'guard bytes written'
        assert torch.equal(buf[pad:pad + nbytes], want_bytes)

    as_bytes = lambda x: x.t.contiguous().view(torch.uint8).reshape(-1)
    ptrs = lambda xs: (ctypes.c_void_p * len(xs))(*[x if isinstance(x, int) else x.ptr for x in xs])
    L, hd, st = ctx._L, ctx._h, ctx._stream()
    b1, p1 = guarded(n * eb)
    cb = torch.full((pad + 4 + pad,), 0xa5, dtype=torch.uint8, device='cuda')
    cb[pad:pad + 4] = 0
    assert L.ffgm_rbits_open(hd, ptrs(rs), ptrs(zs), ctx._scalars(D.lam[k]), k, p1, cb.data_ptr() + pad, n, st) == _ffi.OK
    check(b1, n * eb, as_bytes(D.dc[k]['some']))
    zeros = sum(1 for v in D.c[k]['some'] if v == 0)
    check(cb, 4, torch.tensor([zeros], dtype=torch.int32, device='cuda').view(torch.uint8))
    c = D.c[k]['some'].copy()
    c[3:] = np.where(c[3:] == 0, 0, np.array([v * v % p for v in D.r[0]], dtype=object)[3:])
    dc = up(ctx, c)
    outs = [guarded(n * eb) for _ in range(k)]
    assert L.ffgm_rbits_finish(hd, dc.ptr, ptrs(rs), ptrs([o[1] for o in outs]), k, 0, 16, n, st) == _ffi.OK
    for (buf, _), row in zip(outs, finish_ref(p, c, D.r, False, 16)):
        check(buf, n * eb, as_bytes(up(ctx, row)))
    assert all(torch.equal(x.t, k_) for x, k_ in zip(rs + zs, keep)) and torch.equal(dc.t, up(ctx, c).t), 'an input was written'


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
def test_status_codes(mods):
    import ctypes
    _ffi, engine, _, _ = mods
    p, n, k = 2**61 - 1, 300, 3
    ctx = engine.FieldContext(p, device=0)
    L, h, st = ctx._L, ctx._h, ctx._stream()
    eb = ctx.elem_bytes
    pat = lambda count: torch.full((count,), 0x5a, dtype=torch.uint8, device='cuda')
    bufs = [pat(n * eb) for _ in range(2 * k + 1 + k)] + [pat(4)]
    R, Z, O, B, C = bufs[:k], bufs[k:2 * k], bufs[2 * k], bufs[2 * k + 1:3 * k + 1], bufs[-1]
    arr = lambda xs: (ctypes.c_void_p * max(1, len(xs)))(*[x if x is None or isinstance(x, int) else x.data_ptr() for x in xs])
    lam = ctx._scalars([1, 2, 3])
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    opn = lambda r=R, z=Z, l=lam, k_=k, o=O.data_ptr(), c=C.data_ptr(), n_=n: L.ffgm_rbits_open(
        h, None if r is None else arr(r), None if z is None else arr(z), l, k_, o, c, n_, st)
    fin = lambda c=O.data_ptr(), r=R, b=B, m=k, s=0, f=0, n_=n: L.ffgm_rbits_finish(
        h, c, None if r is None else arr(r), None if b is None else arr(b), m, s, f, n_, st)
    # the row count: below 1 is an argument error (also at n = 0), above the limit of the recombination not supported
    assert opn(k_=0) == EINVAL and opn(k_=-1) == EINVAL and opn(k_=0, n_=0) == EINVAL and fin(m=0) == EINVAL and fin(m=-3, n_=0) == EINVAL
    many = [R[0]] * (MAX_ROWS + 1)
    assert opn(r=many, z=many, l=ctx._scalars([1] * (MAX_ROWS + 1)), k_=MAX_ROWS + 1) == ENOTSUP
    assert fin(r=many, b=many, m=MAX_ROWS + 1) == ENOTSUP
    # a null context or required pointer, a null row
    assert L.ffgm_rbits_open(None, arr(R), arr(Z), lam, k, O.data_ptr(), None, n, st) == EINVAL
    assert L.ffgm_rbits_finish(None, O.data_ptr(), arr(R), arr(B), k, 0, 0, n, st) == EINVAL
    assert opn(r=None) == EINVAL and opn(z=None) == EINVAL and opn(l=None) == EINVAL and opn(o=None) == EINVAL
    assert opn(r=[R[0], None, R[2]]) == EINVAL and opn(z=[Z[0], Z[1], None]) == EINVAL
    assert fin(c=None) == EINVAL and fin(r=None) == EINVAL and fin(b=None) == EINVAL and fin(b=[B[0], None, B[2]]) == EINVAL
    assert fin(f=-1) == EINVAL and fin(f=192) == EINVAL
    # sizes overflowing
    for big in (1 << 62, 1 << 61):
        assert opn(n_=big) == EINVAL and fin(n_=big) == EINVAL
    # overlaps: an output on an input, the counter on an input or on the output; the bits on c, on another row, on each other
    assert opn(o=R[1].data_ptr()) == EINVAL and opn(o=Z[2].data_ptr() + eb * (n - 1)) == EINVAL and opn(c=R[0].data_ptr() + 8) == EINVAL
    assert opn(c=O.data_ptr() + 4) == EINVAL
    assert fin(b=[B[0], O, B[2]]) == EINVAL and fin(b=[R[1], B[1], B[2]]) == EINVAL and fin(b=[B[0], B[0], B[2]]) == EINVAL
    assert fin(b=[R[0].data_ptr() + eb, B[1], B[2]]) == EINVAL, 'on its own row but not AT it'
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf == 0x5a).all()), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers
    assert opn(n_=0, r=None, z=None, l=None, o=None, c=None) == OK and fin(n_=0, c=None, r=None, b=None) == OK
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf == 0x5a).all())
    # valid calls, for contrast: inputs may alias each other, the bits may be AT their rows, no counter
    for buf in R + Z:
        buf.zero_()
    C.zero_()
    assert opn() == OK and opn(z=R, c=None) == OK and opn(k_=1) == OK
    torch.cuda.synchronize()
    assert bool((O == 0).all()) and int(C.view(torch.int32).item()) == 2 * n, 'zeros everywhere: every entry counted, twice'
    assert fin() == OK and fin(b=R) == OK and fin(b=[R[0], B[1], R[2]], s=1, f=7) == OK
    torch.cuda.synchronize()
    assert all(bool((b == 0).all()) for b in B + R)
    # binary fields; p = 1 mod 4 and p = 2 for the finish
    g = torch.zeros(8192, dtype=torch.uint8, device='cuda')
    gp = g.data_ptr()
    for mod in (0x11b, (1 << 64) | 0x1b):
        bctx = engine.FieldContext(mod, True, device=0)
        assert bctx._L.ffgm_rbits_open(bctx._h, arr([gp]), arr([gp + 1024]), lam, 1, gp + 4096, None, 4, st) == ENOTSUP
        assert bctx._L.ffgm_rbits_finish(bctx._h, gp, arr([gp + 1024]), arr([gp + 4096]), 1, 0, 0, 4, st) == ENOTSUP
        for bad in (lambda: bctx.rbits_open([bctx.empty(4)], [bctx.empty(4)], [1]), lambda: bctx.rbits_finish(bctx.empty(4), [bctx.empty(4)])):
            with pytest.raises(NotImplementedError):
                bad()
    for mod in (2**40 - 87, 2):
        c1 = engine.FieldContext(mod, device=0)
        assert c1._L.ffgm_rbits_finish(c1._h, gp, arr([gp + 1024]), arr([gp + 4096]), 1, 0, 0, 4, st) == ENOTSUP
        with pytest.raises(NotImplementedError):
            c1.rbits_finish(c1.empty(4), [c1.empty(4)])
    torch.cuda.synchronize()
    assert bool((g == 0).all())
    # the engine's own checks
    e2, e8 = ctx.empty(2), ctx.empty(8)
    for bad in (lambda: ctx.rbits_open([e8], [e8, e8], [1]), lambda: ctx.rbits_open([e8], [e2], [1]), lambda: ctx.rbits_open([e8, e8], [e8, e8], [1]),
                lambda: ctx.rbits_open([], [], []), lambda: ctx.rbits_open([e8], [e8], [1], out=e2),
                lambda: ctx.rbits_open([e8], [e8], [1], zeros=torch.zeros(1, dtype=torch.int64, device='cuda')),
                lambda: ctx.rbits_open([e8], [e8], [1], zeros=torch.zeros(1, dtype=torch.int32)),
                lambda: ctx.rbits_finish(e8, []), lambda: ctx.rbits_finish(e8, [e2]), lambda: ctx.rbits_finish(e8, [e8], outs=[e8, e8]),
                lambda: ctx.rbits_finish(e8, [e8], outs=[e2]), lambda: ctx.rbits_finish(e8, [e8], f=192)):
        with pytest.raises(ValueError):
            bad()


# ---- the protocol ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,t', [(1, 0), (3, 1), (5, 2)])
def test_random_bits_on_the_recorded_draws(mods, m, t):
    """every planting case of the fixture, every (signed, f), four primes: the squares the device opens and the bits it returns
    are the reference's"""
    _ffi, engine, _, protocols = mods
    for e in golden()['fields']:
        ctx = engine.FieldContext(e['p'], device=0)
        for c in e['cases']:
            run_golden(ctx, protocols, gf(e['p']), e, c, m, t, seed=100 * m + t)


@pytest.mark.parametrize('p', ONE_MOD_FOUR, ids=hex)
def test_random_bits_over_primes_one_mod_four(mods, p):
    """p = 1 mod 4 on 12-, 24- and 16-byte elements: the bits come from sqrt_cl, inv, mul and the scalar forms, and their
    signs from WHICH root k_sqrt_cl returns; three zero squares planted, so the compaction runs (tests/test_rbits_host.py
    runs the same on Python integers)"""
    _ffi, engine, _, protocols = mods
    ctx = engine.FieldContext(p, device=0)
    for m, t, signed, f in COMPOSED:
        run_one_mod_four(ctx, protocols, m, t, signed, f, seed=10 * m + f)


@pytest.mark.parametrize('p', [P61, P80, 2**40 - 87])
@pytest.mark.parametrize('m,t', [(3, 1), (5, 2)])
def test_randomness_is_the_stand_in_share_for_share(mods, p, m, t):
    """the PRF is pinned (RFC 8439 and the layout the oracle restates), so the same key gives the same shares"""
    _ffi, engine, _, protocols = mods
    from rbits_cpuctx import RbitsCpuFieldContext
    key, n = b'share for share!', 33
    sup = [protocols.Randomness(ctx, gf(p), t, m, key) for ctx in (engine.FieldContext(p, device=0), RbitsCpuFieldContext(p))]
    ints = lambda shares: [x.to_ints() for x in shares]
    for call in (lambda R: R.elements(n), lambda R: R.zeros(n), lambda R: R.elements(n, 1 << 30), lambda R: R.bits(n),
                 lambda R: R.bits(n, signed=True, f=5), lambda R: R.rand_exp(n, 1 << 20), lambda R: R.rand_trunc(3, 5)[1],
                 lambda R: R.rand_zero(4)[0]):
        dev, cpu = (ints(call(R)) for R in sup)
        assert dev == cpu and len(dev[0]) > 0
    assert sup[0].counter == sup[1].counter > 8
    bits = open_two_ways(sup[0].ctx, sup[0].bits(257), t)
    assert set(bits) == {0, 1}


def test_bits_of_the_fixed_key_are_balanced(mods):
    _ffi, engine, _, protocols = mods
    ctx = engine.FieldContext(P61, device=0)
    ones = sum(open_two_ways(ctx, protocols.Randomness(ctx, gf(P61), 1, 3, BALANCE_KEY).bits(4096), 1))
    print('ones among 4096 bits:', ones)
    assert abs(ones - 2048) <= 192 and ones == BALANCE_ONES


@pytest.mark.parametrize('which', ['lt', 'fxp', 'zero'])
def test_protocols_run_on_the_supplier_alone(mods, which):
    _ffi, engine, _, protocols = mods
    p = zero_test_prime(protocols) if which == 'zero' else P61
    got, want = run_end_to_end(engine.FieldContext(p, device=0), protocols, which, n=33)
    check_end_to_end(which, got, want)
    assert len(got) == 33


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_open_finish(mods):
    """the counter zeroed, the squares of three parties opened and counted, five parties' bits: captured once on one stream,
    replayed on changed inputs, equal to the eager result and to Python integers"""
    _ffi, engine, _, _ = mods
    p, n, k, m = 2**80 - 65, 5003, 3, 5
    ctx = engine.FieldContext(p, device=0)
    rng = np.random.default_rng(29)
    rs, zs, cnt = [ctx.empty(n) for _ in range(m)], [ctx.empty(n) for _ in range(k)], ctx.zero_counter()
    lam = [3, p - 3, 1]

    def steps():
        cnt.zero_()
        c = ctx.rbits_open(rs[:k], zs, lam, zeros=cnt)
        return [c] + ctx.rbits_finish(c, rs, signed=True, f=2)

    def load():
        r = [draw(rng, p, n) for _ in range(m)]
        z = [draw(rng, p, n) for _ in range(k)]
        rest = open_ref(p, r[:k], [0 * z[0]] + z[1:], lam)
        z[0][:3] = ((-rest * pow(lam[0], -1, p)) % p)[:3]              # three zero squares
        for dst, v in zip(rs + zs, r + z):
            dst.t.copy_(up(ctx, v).t)
        return r, z

    load()
    cg = engine.CapturedLaunches(steps)
    for _ in range(2):
        r, z = load()
        c = open_ref(p, r[:k], z, lam)
        want = [c] + finish_ref(p, c, r, True, 2)
        for out in cg.result:
            out.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        assert int(cnt.item()) == 3 and not c[:3].any()
        got = [o.t.clone() for o in cg.result]
        eager = steps()
        torch.cuda.synchronize()
        assert int(cnt.item()) == 3
        for g, w, e in zip(got, want, eager):
            assert torch.equal(g, up(ctx, w).t) and torch.equal(g, e.t)
