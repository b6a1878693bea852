"""Secure 2-D convolution layers on the device: the kernel (k_conv2d, ffgm_conv2d) byte for byte against the Python-integer
stand-in (tests/conv2d_cpuctx.py: the formula of include/ffgpu_math.h, not the kernel) on every prime policy, at the tile,
channel-block, filter-size and flush edges that ffgm_conv2d_plan reports, in both tile shapes, for 1, 3 and 7 senders, with
and without bias, between guard bytes; the closed form for all operands p - 1; what the reference's convolvetensor opened
(tests/golden/conv2d/conv2d.json); aliasing and every refusal; graph capture; and protocols.conv2d / maxpool2x2 / relu /
conv_layer / dense for (m, t) = (1, 0), (3, 1), (7, 3) on protocols.Randomness against the same fixture."""
import random

import numpy as np
import pytest

from conv2d_cpuctx import conv2d_ref
from test_conv2d_host import INT_SHAPES, PARTIES, P_FXP, P_INT, check_conv2d, check_dense, check_layer, golden
from test_gpu_bsgn import FIELDS as BSGN_FIELDS
from test_gpu_fxp import up
from test_gpu_sgn import draw, same
from test_sort_host import _signed

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

# the prime list of test_gpu_unitvec.py (one prime per policy: every element size, both 24-byte families) and the demo's two
FIELDS = dict(BSGN_FIELDS, **{'demo-secint37': P_INT, 'demo-secfxp10-4': P_FXP})
LAZY32 = ('pm96', 'pm128', 'pm192', 'demo-secint37')      # DotAcc<F>::FLUSH == 32: the multi-limb 2^k - c primes; 192 elsewhere
MULTI_LIMB = ('pm96', 'pm128', 'pm192', 'mont128', 'mont192', 'demo-secint37')
PAD = 240                                                 # guard bytes: a multiple of every element size and of 16


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import _ffi, engine, finfields, protocols
    return _ffi, engine, finfields, protocols


def flush_of(name):
    return 32 if name in LAZY32 else 192


def contexts(engine, monkeypatch, p):
    """(the context as shipped: narrow tiles at these sizes; one whose convolutions take the wide shape at every size)"""
    narrow = engine.FieldContext(p, device=0)
    monkeypatch.setenv('FFGPU_CONV_WIDE_PER_CU', '0')
    wide = engine.FieldContext(p, device=0)
    monkeypatch.delenv('FFGPU_CONV_WIDE_PER_CU')
    return narrow, wide


def test_the_fields_are_what_they_claim(mods):
    _, engine, finfields, _ = mods
    assert all(finfields.is_prime(p) for p in FIELDS.values()) and len(FIELDS) == 13
    sizes = {name: engine.FieldContext(p, device=0).elem_bytes for name, p in FIELDS.items()}
    assert sorted(set(sizes.values())) == [4, 8, 12, 16, 24] and sizes['pm192'] == sizes['mont192'] == 24
    assert sizes['demo-secint37'] == 12 and sizes['demo-secfxp10-4'] == 8


def run_guarded(_ffi, ctx, xs, ws, bs, dims):
    """ffgm_conv2d into outputs between guard bytes; returns the senders' outputs as uint8 tensors after checking the guards
    and that no input was written"""
    import ctypes
    k, r, m, n, v, s = dims
    nsend, nbytes = len(xs), k * v * m * n * ctx.elem_bytes
    bufs = [torch.full((PAD + nbytes + PAD,), 0xa5, dtype=torch.uint8, device='cuda') for _ in range(nsend)]
    keep = [a.t.clone() for a in list(xs) + list(ws) + list(bs or [])]
    arr = lambda ptrs: (ctypes.c_void_p * nsend)(*ptrs)
    rc = ctx._L.ffgm_conv2d(ctx._h, arr([a.ptr for a in xs]), arr([a.ptr for a in ws]), None if bs is None else arr([a.ptr for a in bs]),
                            arr([b.data_ptr() + PAD for b in bufs]), nsend, k, r, m, n, v, s, ctx._stream())
    assert rc == _ffi.OK, rc
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:PAD] == 0xa5).all()) and bool((b[PAD + nbytes:] == 0xa5).all()), 'guard bytes written'
    assert all(torch.equal(a.t, k_) for a, k_ in zip(list(xs) + list(ws) + list(bs or []), keep)), 'an input was written'
    return [b[PAD:PAD + nbytes] for b in bufs]


def check_case(_ffi, ctx, p, rng, dims, nsend, bias, tag):
    """random tensors per sender (edge values included) through the kernel and through the stand-in's formula: the same bytes"""
    k, r, m, n, v, s = dims
    vals = [[draw(rng, p, c) for c in (k * r * m * n, v * r * s * s, v)] for _ in range(nsend)]
    for x, W, b in vals:
        x[:3], W[:2] = [p - 1, 0, 1], [p - 1, p - 2]                     # (the smallest x here has 3 elements, the smallest W 2)
    xs, ws = [up(ctx, q[0]) for q in vals], [up(ctx, q[1]) for q in vals]
    bs = [up(ctx, q[2]) for q in vals] if bias else None
    got = run_guarded(_ffi, ctx, xs, ws, bs, dims)
    for q, (x, W, b) in enumerate(vals):
        want = up(ctx, conv2d_ref(p, x, W, b if bias else None, *dims)).t.contiguous().view(torch.uint8).reshape(-1)
        assert torch.equal(got[q], want), tag + (dims, nsend, bias, q)


def edge_cases(pl, s=3):
    """(k, r, m, n, v, s) on the edges of the reported tile TH x TW and channel block VB: every listed value of m, n, v and k
    occurs, each next to a different value of the others"""
    TH, TW, VB = pl.tile_rows, pl.tile_cols, pl.out_channels
    return [(1, 1, 1, s, 1, s), (2, 1, TH - 1, TW - 1, VB, s), (1, 2, TH, TW, VB + 1, s), (2, 1, TH + 1, TW + 1, 1, s),
            (1, 1, TH + 1, TW - 1, VB + 1, s), (1, 2, TH - 1, TW + 1, VB, s), (2, 1, 1, TW + 1, VB + 1, s), (1, 1, TH, s, VB, s)]


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernel_at_the_tile_and_channel_edges(mods, monkeypatch, name):
    _ffi, engine, _, _ = mods
    p = FIELDS[name]
    rng = np.random.default_rng(11)
    for which, ctx in zip(('narrow', 'wide'), contexts(engine, monkeypatch, p)):
        pl = ctx.conv2d_plan(1, 1, 8, 16, 4, 3)
        assert pl.wide == (which == 'wide') and (pl.tile_rows, pl.tile_cols, pl.out_channels) == ((16, 16, 4) if pl.wide else (8, 16, 2))
        for i, dims in enumerate(edge_cases(pl)):
            assert ctx.conv2d_plan(*dims, nsend=(1, 3, 7)[i % 3]).wide == pl.wide
            check_case(_ffi, ctx, p, rng, dims, (1, 3, 7)[i % 3], i % 2 == 0, (name, which))


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernel_at_every_filter_size_and_the_flush_bound(mods, monkeypatch, name):
    """s in {1, 2, 3, 6, 16} with n >= s, m < s among them; r s^2 one below, at, one above the policy's flush bound and above
    twice the bound (s = 1), the bound met at a row inside a later channel (s = 2, 3) and inside one channel (s = 6, 16)"""
    _ffi, engine, _, _ = mods
    p, F = FIELDS[name], flush_of(name)
    rng = np.random.default_rng(12)
    narrow, wide = contexts(engine, monkeypatch, p)
    assert narrow.conv2d_plan(1, 1, 4, 4, 1, 1).flush_rows == F and narrow.conv2d_plan(1, 1, 4, 16, 1, 16).flush_rows == F // 16
    cases = [(1, 1, 5, 7, 2, 1), (2, 2, 5, 7, 3, 2), (1, 1, 4, 9, 2, 6), (1, 1, 3, 16, 5, 16), (1, 2, 18, 17, 1, 16),
             (1, F - 1, 3, 5, 2, 1), (1, F, 3, 5, 2, 1), (1, F + 1, 3, 5, 2, 1), (1, 2 * F + 1, 2, 3, 5, 1),
             (1, F // 4, 3, 4, 2, 2), (1, F // 2 + 1, 3, 4, 1, 2), (1, F // 9 + 2, 4, 5, 2, 3), (1, 3, 7, 6, 2, 6)]
    for i, dims in enumerate(cases):
        ctx = (narrow, wide)[i % 2]
        check_case(_ffi, ctx, p, rng, dims, (3, 1, 7, 1)[i % 4], i % 3 != 0, (name, i))
    for dims in cases[5:9]:                                             # the flush edges through the other shape as well
        check_case(_ffi, wide, p, rng, dims, 1, True, (name, 'wide'))


@pytest.mark.parametrize('name', list(FIELDS))
def test_all_operands_p_minus_1(mods, monkeypatch, name):
    """x = W = p - 1, no bias: every product is 1, so an output is r times its count of in-range taps -- the lazy accumulators at
    their largest values, the halo, and flushes inside a channel (s = 6: 36 terms, s = 16: 256) and across channels.  Run over
    every prime, the multi-limb ones among them."""
    _ffi, engine, _, _ = mods
    assert set(MULTI_LIMB) <= set(FIELDS)
    p = FIELDS[name]
    for ctx in contexts(engine, monkeypatch, p):
        for k, r, m, n, v, s in ((1, 7, 7, 9, 5, 6), (1, 2, 5, 17, 5, 16), (2, 3, 17, 18, 1, 16)):
            x, W = up(ctx, [p - 1] * (k * r * m * n)), up(ctx, [p - 1] * (v * r * s * s))
            rows = [sum(0 <= I + di - (s - 1) // 2 < m for di in range(s)) for I in range(m)]
            cols = [sum(0 <= J + dj - s // 2 < n for dj in range(s)) for J in range(n)]
            want = [r * a * b % p for _ in range(k * v) for a in rows for b in cols]
            for got in run_guarded(_ffi, ctx, [x, x, x], [W, W, W], None, (k, r, m, n, v, s)):
                assert torch.equal(got, up(ctx, want).t.contiguous().view(torch.uint8).reshape(-1)), (name, s)


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernel_gives_what_the_reference_opened(mods, name):
    """the demo's own convolvetensor, SecInt(37): the recorded signed integers are far below every prime here"""
    _, engine, _, _ = mods
    p = FIELDS[name]
    ctx = engine.FieldContext(p, device=0)
    doc = golden()
    for e in [c for c in doc['conv'] if c['f'] == 0] + [dict(doc['layer'], y=doc['layer']['conv'])]:
        x, W, b = (up(ctx, [q % p for q in e[key]]) for key in 'xWb')
        got = ctx.conv2d([x], [W], [b], *e['shape'])[0].to_ints()
        assert [_signed(q, p) for q in got] == e['y'], (name, e['shape'])
    assert [c['shape'] for c in doc['conv'][:5]] == INT_SHAPES


def test_aliasing_and_refusals(mods):
    import ctypes
    _ffi, engine, _, _ = mods
    p = 2**61 - 1
    ctx = engine.FieldContext(p, device=0)
    L, hd, st, eb = ctx._L, ctx._h, ctx._stream(), ctx.elem_bytes
    EINVAL, OK, ENOTSUP = _ffi.EINVAL, _ffi.OK, _ffi.ENOTSUP
    k, r, m, n, v, s = 1, 2, 4, 5, 3, 3
    nx, nw, ny = k * r * m * n, v * r * s * s, k * v * m * n
    rng = np.random.default_rng(13)
    xv, wv, bv = draw(rng, p, nx), draw(rng, p, nw), draw(rng, p, v)
    x, W, b = up(ctx, xv), up(ctx, wv), up(ctx, bv)
    pat = lambda count: torch.full((count,), 0x5a, dtype=torch.uint8, device='cuda')
    O = [pat(ny * eb) for _ in range(3)]
    arr = lambda *ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
    o = [q.data_ptr() for q in O]

    NULL = 'null'

    def call(xs=None, ws=None, bs=None, outs=None, nsend=1, dims=(k, r, m, n, v, s), h=hd):
        """the valid call, with the named arguments replaced (NULL: a null pointer)"""
        given = [xs, ws, bs, outs]
        for i, dflt in enumerate(([x.ptr] * nsend, [W.ptr] * nsend, [b.ptr] * nsend, o[:nsend])):
            given[i] = arr(*dflt) if given[i] is None else None if given[i] is NULL else given[i]
        return L.ffgm_conv2d(h, *given, nsend, *dims, st)
    # the counts
    assert call(nsend=0) == EINVAL and call(dims=(k, r, m, n, v, 0)) == EINVAL and call(dims=(k, r, m, n, v, 17)) == EINVAL
    assert call(dims=(k, r, m, 2, v, 3)) == EINVAL, 's > n'
    assert call(dims=(k, 0, m, n, v, s)) == EINVAL, 'no input channel, a non-empty output'
    assert call(dims=(1 << 62, r, m, n, v, s)) == EINVAL and call(dims=(1 << 40, 1 << 30, m, n, v, s)) == EINVAL, 'overflow'
    # a null context or required pointer, any of the senders' entries
    assert call(h=None) == EINVAL and call(xs=NULL) == EINVAL and call(ws=NULL) == EINVAL and call(outs=NULL) == EINVAL
    assert call(xs=arr(x.ptr, None), nsend=2) == EINVAL and call(ws=arr(None, W.ptr), nsend=2) == EINVAL
    assert call(bs=arr(b.ptr, None), nsend=2) == EINVAL and call(outs=arr(o[0], None), nsend=2) == EINVAL
    # any output overlapping any input or another output, from either end
    last = lambda base, count: base + eb * (count - 1)
    assert call(outs=arr(x.ptr)) == EINVAL and call(outs=arr(W.ptr)) == EINVAL and call(outs=arr(b.ptr)) == EINVAL
    assert call(xs=arr(last(o[0], ny))) == EINVAL and call(ws=arr(o[0] - eb * (nw - 1))) == EINVAL and call(bs=arr(last(o[0], ny))) == EINVAL
    assert call(outs=arr(o[0], o[0]), nsend=2) == EINVAL and call(outs=arr(o[0], o[1], last(o[1], ny)), nsend=3) == EINVAL
    assert call(xs=arr(x.ptr, o[0]), nsend=2) == EINVAL, "sender 0's output on sender 1's input"
    # not supported: more than 64 senders, a grid beyond HIP's limit, a GF(2^n) context
    many = arr(*([x.ptr] * 65))
    assert call(xs=many, ws=many, bs=many, outs=many, nsend=65) == ENOTSUP
    assert call(dims=(1 << 40, 1, 16, 16, 4, 1)) == ENOTSUP
    bctx = engine.FieldContext(0x11b, True, device=0)
    assert call(h=bctx._h) == ENOTSUP
    with pytest.raises(NotImplementedError):
        bctx.conv2d([bctx.empty(nx)], [bctx.empty(nw)], None, k, r, m, n, v, s)
    torch.cuda.synchronize()
    assert all(bool((q == 0x5a).all()) for q in O), 'a refused call wrote'
    # nothing to do: FFGPU_OK whatever the pointers, the counts still checked
    assert call(xs=NULL, ws=NULL, bs=NULL, outs=NULL, dims=(0, r, m, n, v, s)) == OK and call(xs=NULL, ws=NULL, bs=NULL, outs=NULL, dims=(k, r, m, n, 0, s)) == OK
    assert call(xs=NULL, ws=NULL, bs=NULL, outs=NULL, dims=(0, r, m, n, v, 17)) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((q == 0x5a).all()) for q in O)
    # inputs may alias each other: the same x, W and b for every sender (public weights), W inside x, b inside W
    want = conv2d_ref(p, xv, wv, bv, k, r, m, n, v, s)
    assert call(nsend=3) == OK
    torch.cuda.synchronize()
    assert all(torch.equal(q, up(ctx, want).t.view(torch.uint8).reshape(-1)) for q in O)
    assert call(ws=arr(x.ptr), bs=arr(W.ptr), dims=(1, 1, 4, 10, 1, 3)) == OK                   # x (1,1,4,10), W = x[:9], b = W[:1]
    torch.cuda.synchronize()
    got = engine.DevArray(ctx, O[0][:40 * eb].view(torch.int64), 40).to_ints()
    assert got == conv2d_ref(p, xv, xv[:9], wv[:1], 1, 1, 4, 10, 1, 3)
    # the engine's own checks
    for bad in (lambda: ctx.conv2d([x], [W], [b], k, r, m, n, v, 4), lambda: ctx.conv2d([x], [W, W], [b], k, r, m, n, v, s),
                lambda: ctx.conv2d([x], [W], [b], k, r, m, n, v, s, outs=[ctx.empty(ny + 1)]), lambda: ctx.conv2d([], [], None, k, r, m, n, v, s),
                lambda: ctx.conv2d([x], [W], [b], k, r, m, n, v, s, outs=[x]), lambda: ctx.conv2d_plan(k, r, m, 2, v, 3)):
        with pytest.raises(ValueError):
            bad()


def test_graph_capture_replays_the_launch(mods):
    """one call for three senders captured once, replayed on changed inputs: the bytes of the eager call and of the formula"""
    _, engine, _, _ = mods
    p = P_INT
    ctx = engine.FieldContext(p, device=0)
    dims = (2, 3, 9, 17, 5, 5)
    k, r, m, n, v, s = dims
    rng = np.random.default_rng(14)
    xs, ws, bs = ([ctx.empty(c) for _ in range(3)] for c in (k * r * m * n, v * r * s * s, v))

    def load():
        vals = [[draw(rng, p, a.n) for a in grp] for grp in (xs, ws, bs)]
        for grp, vv in zip((xs, ws, bs), vals):
            for dst, q in zip(grp, vv):
                dst.t.copy_(up(ctx, q).t)
        return vals

    load()
    cg = engine.CapturedLaunches(lambda: ctx.conv2d(xs, ws, bs, *dims))
    for _ in range(2):
        vx, vw, vb = load()
        for out in cg.result:
            out.t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        eager = ctx.conv2d(xs, ws, bs, *dims)
        torch.cuda.synchronize()
        assert all(same(a, e.t) for a, e in zip(cg.result, eager))
        assert cg.result[1].to_ints() == conv2d_ref(p, vx[1], vw[1], vb[1], *dims)


def test_memory_is_linear_in_the_tensors(mods):
    """the demo's layer 2 at batch 8 for three senders: the call allocates its outputs and nothing else (an im2col route would
    gather s^2 = 25 copies of x)"""
    _, engine, _, _ = mods
    ctx = engine.FieldContext(P_INT, device=0)
    k, r, m, n, v, s = 8, 32, 14, 14, 64, 5
    x, W, b = ctx.empty(k * r * m * n), ctx.empty(v * r * s * s), ctx.empty(v)
    for a in (x, W, b):
        a.t.zero_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    outs = ctx.conv2d([x] * 3, [W] * 3, [b] * 3, k, r, m, n, v, s)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    assert extra <= 3 * k * v * m * n * ctx.elem_bytes + (1 << 20), extra
    assert all(not bool(o.t.any()) for o in outs)


# ---- the protocols on the device, on protocols.Randomness ----------------------------------------------------------------------
def device_ctx(engine):
    return lambda p: engine.FieldContext(p, device=0)


@pytest.mark.parametrize('m,t', PARTIES)
def test_conv2d_opens_to_the_fixture(mods, m, t):
    """shared and public W give the same opened result; the fixed-point cases with the two-part assertion"""
    _, engine, _, protocols = mods
    check_conv2d(device_ctx(engine), protocols, m, t)


@pytest.mark.parametrize('m,t', PARTIES)
def test_maxpool_relu_and_the_whole_layer_open_to_the_fixture(mods, m, t):
    _, engine, _, protocols = mods
    check_layer(device_ctx(engine), protocols, m, t)


@pytest.mark.parametrize('m,t', PARTIES)
def test_dense_is_the_product_plus_the_bias(mods, m, t):
    _, engine, _, protocols = mods
    check_dense(device_ctx(engine), protocols, m, t)


def test_one_launch_for_all_senders(mods, monkeypatch):
    """protocols.conv2d calls the kernel once, for 2t+1 senders"""
    _, engine, finfields, protocols = mods
    ctx = engine.FieldContext(P_INT, device=0)
    calls = []
    real = ctx.conv2d
    monkeypatch.setattr(ctx, 'conv2d', lambda xs, *a, **kw: calls.append(len(xs)) or real(xs, *a, **kw))
    rng = random.Random(1)
    sh = lambda c: [ctx.from_ints([rng.randrange(P_INT) for _ in range(c)]) for _ in range(7)]
    protocols.conv2d(ctx, finfields.GF(P_INT), sh(16), sh(9), sh(1), 1, 1, 4, 4, 1, 3, 2)
    assert calls == [5]
