"""Prefix scans and axis reductions of field arrays through the scan kernels (ffgpu_scan, ffgpu_axis_reduce): every field
policy, both operators, both geometries (column walk, row tiles) at the tile, pack and wave edges, in place, with the
initial element, unaligned views, the full sizes, memory, the C ABI, the NumPy surface, and the comparison with the composed
route the kernels replace.  Expected values never come from the code under test: prime fields take itertools.accumulate
on Python ints with % p (the reference's rule: integer cumsum / cumprod, then one reduction, finfields.py:801, 807), GF(2^n)
XOR and the carry-less oracle (oracle.pyoracle.clmul / clmod); the full-size scans are checked element by element against
the C oracle's element-wise add / mul (out[i] == out[i-1] o a[i]: by induction the whole scan).  Bit-exact throughout.

Row-tile geometry (mpyc_amd/csrc/scan_geom.hpp): a thread holds 16 elements (8 above 8-byte elements), a workgroup tile is
threads x that; a context created with FFGPU_SCAN_TILE_THREADS=2 has tiles of 32 (16) elements, so small arrays span many
tiles.  FFGPU_SCAN_GEOM=1 / 2 forces the column walk / the row tiles."""
import itertools
import random
import statistics

import numpy as np
import pytest

from oracle import coracle, pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

P61, P80, P128 = 2**61 - 1, 2**80 - 65, 2**128 - 173
COLS, ROWS = 1, 2
SMALL_TT = 2


def prime_moduli():
    """the modulus list of tests/test_gpu_convolve.py: one per prime policy"""
    return [2**31 - 1, 19, P61, 2**64 - 189, 2**63 - 25, 6616326157076047771, P80, 2**96 - 17, 2**127 - 1,
            P128, 2**127 + 2**100 + 0x101, 2**136 - 113, 2**192 - 2**40 + 341]


def binary_moduli():
    return [0x11b, 0x1002b, 0x10000008d, 0x1000000000000001b, 0x100000000000000000000000000000087]


ALL_FIELDS = [(p, False) for p in prime_moduli()] + [(m, True) for m in binary_moduli()]
FIELD_IDS = [hex(m) for m, _ in ALL_FIELDS]


def order_of(modulus, binary):
    return 1 << (modulus.bit_length() - 1) if binary else modulus


def field_op(modulus, binary, mul):
    if binary:
        return (lambda x, y: po.clmod(po.clmul(x, y), modulus)) if mul else (lambda x, y: x ^ y)
    return (lambda x, y: x * y % modulus) if mul else (lambda x, y: (x + y) % modulus)


def expect_scan(modulus, binary, vals, outer, k, inner, mul, wi=False):
    """flat list of the (outer, k [+ 1], inner) scan of the flat (outer, k, inner) list vals"""
    op = field_op(modulus, binary, mul)
    kk = k + (1 if wi else 0)
    out = [None] * (outer * kk * inner)
    for o in range(outer):
        for i in range(inner):
            line = list(itertools.accumulate(vals[(o * k) * inner + i:(o * k + k) * inner:inner], op))
            if wi:
                line.insert(0, 1 if mul else 0)
            out[(o * kk) * inner + i:(o * kk + kk) * inner:inner] = line
    return out


def expect_reduce(modulus, binary, vals, outer, k, inner, mul):
    op = field_op(modulus, binary, mul)
    out = []
    for o in range(outer):
        for i in range(inner):
            acc = None
            for x in vals[(o * k) * inner + i:(o * k + k) * inner:inner]:
                acc = x if acc is None else op(acc, x)
            out.append(acc)
    return out


def draw(rng, order, n):
    """seeded draws with order - 1 and 1 planted anywhere and a zero in the last third (a zero must zero every later
    product of its line, and two thirds of a long line still carry non-trivial products)"""
    vals = [rng.randrange(order) for _ in range(n)]
    if n >= 4:
        vals[rng.randrange(n)] = order - 1
        vals[rng.randrange(n)] = 1
        vals[rng.randrange(2 * n // 3, n)] = 0
    return vals


def make_ctx(monkeypatch, modulus, binary, geom=0, tt=256):
    """a context of its own with the geometry / tile switches set (they are read at creation)"""
    from mpyc_amd import engine
    monkeypatch.setenv('FFGPU_SCAN_GEOM', str(geom))
    monkeypatch.setenv('FFGPU_SCAN_TILE_THREADS', str(tt))
    ctx = engine.FieldContext(modulus, binary, device=0)
    monkeypatch.delenv('FFGPU_SCAN_GEOM')
    monkeypatch.delenv('FFGPU_SCAN_TILE_THREADS')
    return ctx


def items_of(eb):
    return 16 if eb <= 8 else 8


def limb_bytes(vals, eb):
    from mpyc_amd.engine import ints_to_np
    return ints_to_np(vals, eb).tobytes()


def check_shape(ctxs, modulus, binary, rng, outer, k, inner, tag):
    """scan and reduction, add and mul, on every context of ctxs (one per geometry / tile setting), byte for byte"""
    order = order_of(modulus, binary)
    vals = draw(rng, order, outer * k * inner)
    eb = ctxs[0][1].elem_bytes
    for mul in (False, True):
        want_scan = limb_bytes(expect_scan(modulus, binary, vals, outer, k, inner, mul), eb)
        want_red = limb_bytes(expect_reduce(modulus, binary, vals, outer, k, inner, mul), eb)
        for name, ctx in ctxs:
            a = ctx.from_ints(vals)
            assert ctx.scan(a, outer, k, inner, mul=mul).to_numpy().tobytes() == want_scan, ('scan', name, mul) + tag
            assert ctx.axis_reduce(a, outer, k, inner, mul=mul).to_numpy().tobytes() == want_red, ('reduce', name, mul) + tag


def check_shape_by_induction(ctxs, modulus, binary, rng, outer, k, inner, tag):
    """the same four results where Python carry-less products would take too long: line by line, out(o, 0, i) == a(o, 0, i)
    and out(o, j, i) == out(o, j-1, i) o a(o, j, i) with the right-hand side computed by the C oracle's element-wise add /
    mul in one call (by induction the whole scan); the reduction must then be the last step of that scan"""
    from mpyc_amd.engine import ints_to_np
    order = order_of(modulus, binary)
    vals = draw(rng, order, outer * k * inner)
    eb = ctxs[0][1].elem_bytes
    cf = coracle.CField(modulus, binary)
    assert cf.eb == eb
    A = ints_to_np(vals, eb)
    A4 = A.reshape((outer, k, inner) + A.shape[1:])
    for mul in (False, True):
        op = coracle.MUL if mul else coracle.ADD
        for name, ctx in ctxs:
            a = ctx.from_ints(vals)
            O = ctx.scan(a, outer, k, inner, mul=mul).to_numpy()
            assert O.shape == A.shape and O.dtype == A.dtype, ('scan', name, mul) + tag
            O4 = O.reshape(A4.shape)
            assert O4[:, 0].tobytes() == A4[:, 0].tobytes(), ('scan first step', name, mul) + tag
            if k > 1:
                step = cf.ew(op, np.ascontiguousarray(O4[:, :-1]), np.ascontiguousarray(A4[:, 1:]))
                assert step.tobytes() == np.ascontiguousarray(O4[:, 1:]).tobytes(), ('scan', name, mul) + tag
            R = ctx.axis_reduce(a, outer, k, inner, mul=mul).to_numpy()
            assert R.tobytes() == np.ascontiguousarray(O4[:, -1]).tobytes(), ('reduce', name, mul) + tag


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    from mpyc_amd import finfields, gfpx
    return finfields, gfpx


def gf(api, modulus, binary=False):
    finfields, gfpx = api
    return finfields.GF(gfpx.BinaryPolynomial(modulus)) if binary else finfields.GF(modulus)


def ints(a):
    return [int(x) for x in np.asarray(a.value).reshape(-1)]


@pytest.mark.parametrize('modulus,binary', ALL_FIELDS, ids=FIELD_IDS)
def test_flat_arrays_at_tile_edges(monkeypatch, modulus, binary):
    """(1, k, 1): one line, from one element to several tiles and a ragged rest, small tiles and the default ones"""
    small = make_ctx(monkeypatch, modulus, binary, ROWS, SMALL_TT)
    default = make_ctx(monkeypatch, modulus, binary)
    cols = make_ctx(monkeypatch, modulus, binary, COLS)
    rng = random.Random(modulus & 0xffff)
    T = SMALL_TT * items_of(small.elem_bytes)
    for k in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 7 * T + 5, 300 * T + 3):     # 300 tiles: two chunks of carries
        # (GF(2^n): Python carry-less products up to 1500 elements, the C oracle step by step above that)
        check = check_shape_by_induction if binary and k > 1500 else check_shape
        check([('small', small), ('cols', cols)], modulus, binary, rng, 1, k, 1, (k,))
    TD = 256 * items_of(small.elem_bytes)
    for k in (TD - 1, TD, TD + 1, 2 * TD + 1) if not binary else (TD + 1,):
        check_shape([('default', default)], modulus, binary, rng, 1, k, 1, (k,))


@pytest.mark.parametrize('modulus,binary', ALL_FIELDS, ids=FIELD_IDS)
def test_many_short_rows_and_few_long_rows(monkeypatch, modulus, binary):
    ctxs = [('auto', make_ctx(monkeypatch, modulus, binary)), ('rows small', make_ctx(monkeypatch, modulus, binary, ROWS, SMALL_TT)),
            ('cols', make_ctx(monkeypatch, modulus, binary, COLS))]
    rng = random.Random(1 + (modulus & 0xffff))
    check_shape(ctxs, modulus, binary, rng, 300, 7, 1, ('short rows',))
    check_shape(ctxs, modulus, binary, rng, 3, 700 if binary else 3000, 1, ('long rows',))


@pytest.mark.parametrize('modulus,binary', ALL_FIELDS, ids=FIELD_IDS)
def test_inner_axis_at_pack_edges(monkeypatch, modulus, binary):
    """(outer, k, inner): inner around the 16-byte pack, k around the load-ahead depth and the tile, both geometries (the
    rows of the row geometry are then `inner` elements apart)"""
    cols = make_ctx(monkeypatch, modulus, binary, COLS)
    rows = make_ctx(monkeypatch, modulus, binary, ROWS, SMALL_TT)
    auto = make_ctx(monkeypatch, modulus, binary)
    eb = cols.elem_bytes
    pack = 16 // eb if eb <= 8 else 1
    rng = random.Random(2 + (modulus & 0xffff))
    inners = sorted({1, 2, 3, 64, 1000} | {x for x in (pack - 1, pack, pack + 1) if x >= 1})
    for inner in inners:
        for k in (1, 2, 33, 257):
            outer = 2 if inner * k <= 40000 else 1
            # (GF(2^n): Python carry-less products for the small cells, the C oracle step by step for the large one)
            check = check_shape_by_induction if binary and inner * k > 40000 else check_shape
            check([('cols', cols), ('rows', rows), ('auto', auto)], modulus, binary, rng, outer, k, inner, (outer, k, inner))


@pytest.mark.parametrize('modulus,binary', [(P61, False), (P80, False), (2**136 - 113, False), (0x11b, True)], ids=hex)
def test_views_in_place_and_initial(api, monkeypatch, modulus, binary):
    """a view at an odd element offset (unaligned base: the single-element paths), in place, with the initial element,
    for both geometries"""
    order = order_of(modulus, binary)
    rng = random.Random(3)
    for geom, tt in ((COLS, 256), (ROWS, SMALL_TT)):
        ctx = make_ctx(monkeypatch, modulus, binary, geom, tt)
        eb = ctx.elem_bytes
        from mpyc_amd.engine import DevArray
        for outer, k, inner in ((1, 331, 1), (2, 33, 8), (3, 5, 32)):
            n = outer * k * inner
            vals = draw(rng, order, n + 1)
            whole = ctx.from_ints(vals)
            view = DevArray(ctx, whole.t[1:], n)                        # starts one element in
            assert view.ptr == whole.ptr + eb
            for mul in (False, True):
                want = expect_scan(modulus, binary, vals[1:], outer, k, inner, mul)
                assert ctx.scan(view, outer, k, inner, mul=mul).to_ints() == want
                assert ctx.axis_reduce(view, outer, k, inner, mul=mul).to_ints() == \
                    expect_reduce(modulus, binary, vals[1:], outer, k, inner, mul)
                wi = ctx.scan(view, outer, k, inner, mul=mul, with_initial=True)
                assert wi.n == outer * (k + 1) * inner
                assert wi.to_ints() == expect_scan(modulus, binary, vals[1:], outer, k, inner, mul, wi=True)
                al = ctx.from_ints(vals[1:])                            # aligned: with_initial through the pack path
                assert ctx.scan(al, outer, k, inner, mul=mul, with_initial=True).to_ints() == \
                    expect_scan(modulus, binary, vals[1:], outer, k, inner, mul, wi=True)
                got = ctx.scan(al, outer, k, inner, mul=mul, out=al)    # in place
                assert got is al and al.to_ints() == want
                again = ctx.from_ints(vals)
                inplace_view = DevArray(ctx, again.t[1:], n)
                ctx.scan(inplace_view, outer, k, inner, mul=mul, out=inplace_view)
                assert again.to_ints() == vals[:1] + want               # and nothing before the view was touched


@pytest.mark.parametrize('modulus,binary', [(P61, False), (2**96 - 17, False), (P128, False), (2**192 - 2**40 + 341, False),
                                            (0x11b, True), (0x1000000000000001b, True)], ids=hex)
def test_through_numpy(api, modulus, binary):
    """np.cumsum, np.cumprod, np.cumulative_sum / _prod with the initial, ufunc.accumulate and .reduce, prod with keepdims and
    initial, sum along an axis of a 3-row array, a middle axis, a transposed view, a slice -- against NumPy on dtype=object
    arrays of Python ints reduced mod p (XOR / carry-less products for GF(2^n))"""
    F = gf(api, modulus, binary)
    order = order_of(modulus, binary)
    rng = random.Random(4)
    add, mulop = field_op(modulus, binary, False), field_op(modulus, binary, True)
    shape = (3, 5, 7)
    vals = draw(rng, order, 3 * 5 * 7)
    ref = np.array(vals, dtype=object).reshape(shape)
    a = F.array(ref.copy())

    def acc(x, axis, op, wi=None):
        r = np.apply_along_axis(lambda v: np.array(([wi] if wi is not None else []) + list(itertools.accumulate(v, op)),
                                                   dtype=object), axis, x)
        return [int(v) for v in r.reshape(-1)]

    def red(x, axis, op):
        r = np.apply_along_axis(lambda v: np.array([list(itertools.accumulate(v, op))[-1]], dtype=object), axis, x)
        return [int(v) for v in r.reshape(-1)]

    for axis in (0, 1, 2, -1):
        assert ints(np.cumsum(a, axis=axis)) == acc(ref, axis, add), axis
        assert ints(np.cumprod(a, axis=axis)) == acc(ref, axis, mulop), axis
        assert ints(np.add.accumulate(a, axis=axis)) == acc(ref, axis, add), axis
        assert ints(np.multiply.accumulate(a, axis=axis)) == acc(ref, axis, mulop), axis
        ci = np.cumulative_sum(a, axis=axis, include_initial=True)
        assert ci.shape == tuple(s + (1 if d == axis % 3 else 0) for d, s in enumerate(shape))
        assert ints(ci) == acc(ref, axis, add, wi=0), axis
        assert ints(np.cumulative_prod(a, axis=axis, include_initial=True)) == acc(ref, axis, mulop, wi=1), axis
        pr = a.prod(axis=axis)
        assert pr.shape == tuple(s for d, s in enumerate(shape) if d != axis % 3) and ints(pr) == red(ref, axis, mulop)
        pk = a.prod(axis=axis, keepdims=True, initial=3)
        assert pk.shape == tuple(1 if d == axis % 3 else s for d, s in enumerate(shape))
        assert ints(pk) == [mulop(x, 3) for x in red(ref, axis, mulop)]
        assert ints(np.multiply.reduce(a, axis=axis)) == red(ref, axis, mulop)
        assert ints(np.add.reduce(a, axis=axis)) == red(ref, axis, add)
        assert ints(a.sum(axis=axis)) == red(ref, axis, add)
    flat = [int(v) for v in ref.reshape(-1)]
    sval = lambda x: int(x) if binary else int(x) % modulus                                # (int() of a prime-field element is signed)
    assert ints(np.cumsum(a)) == list(itertools.accumulate(flat, add))                    # axis=None flattens
    assert ints(np.cumprod(a)) == list(itertools.accumulate(flat, mulop))
    assert sval(a.prod()) == 0 and sval(a.sum()) == list(itertools.accumulate(flat, add))[-1]           # (a zero is planted)
    nz = [v or 1 for v in flat]
    assert sval(F.array(nz).prod()) == list(itertools.accumulate(nz, mulop))[-1] != 0
    allp = a.prod(keepdims=True)
    assert allp.shape == (1, 1, 1) and ints(allp) == [list(itertools.accumulate(flat, mulop))[-1]]
    assert sval(F.array(nz).prod(initial=5)) == mulop(list(itertools.accumulate(nz, mulop))[-1], 5)
    t, rt = a.transpose(2, 0, 1), ref.transpose(2, 0, 1)                                   # transposed view
    assert ints(np.cumsum(t, axis=1)) == acc(rt, 1, add) and ints(np.cumprod(t, axis=2)) == acc(rt, 2, mulop)
    s, rs = a[1:], ref[1:]                                                                 # a view one row in
    assert ints(np.cumsum(s, axis=1)) == acc(rs, 1, add) and ints(np.cumprod(s, axis=0)) == acc(rs, 0, mulop)
    f1 = F.array(flat)[1:]                                                                 # odd element offset
    assert ints(np.cumsum(f1)) == list(itertools.accumulate(flat[1:], add))
    # 3 long rows: the cell of sum(axis) that used to loop over rows in Python
    k = 2000 if not binary else 300
    v3 = draw(rng, order, 3 * k)
    a3, r3 = F.array(np.array(v3, dtype=object).reshape(3, k)), np.array(v3, dtype=object).reshape(3, k)
    assert ints(a3.sum(axis=1)) == red(r3, 1, add) and ints(a3.prod(axis=1)) == red(r3, 1, mulop)
    assert ints(a3.T.sum(axis=0)) == red(r3, 1, add)
    # unchanged edges: 1 element, 0-d, empty axis
    one = F.array([vals[0]])
    assert ints(np.cumsum(one)) == [vals[0]] and ints(np.cumprod(one)) == [vals[0]] and sval(one.prod()) == vals[0]
    e = F.array(np.zeros((2, 0, 3), dtype=object))
    assert np.cumsum(e, axis=1).shape == (2, 0, 3) and ints(e.prod(axis=1)) == [1] * 6 and ints(e.sum(axis=1)) == [0] * 6
    assert np.cumulative_sum(e, axis=1, include_initial=True).shape == (2, 1, 3)


def device_array(api, modulus, limbs_np, shape):
    """FieldArray over an uploaded limb array (canonical by construction)"""
    F = gf(api, modulus)
    ctx = F.array([0]).ctx
    return F, F.array._wrap(ctx.from_numpy(limbs_np), shape)


def canonical_limbs(rs, modulus, n):
    """uniform below a power of two under the modulus: canonical without a reduction on the host"""
    if modulus == P61:
        a = rs.integers(0, modulus, n, dtype=np.uint64)
    elif modulus == P128:
        a = rs.integers(0, 2**63, (n, 2), dtype=np.uint64)
        a[:, 0] = rs.integers(0, 2**64, n, dtype=np.uint64)
    else:
        assert modulus == P80
        a = rs.integers(0, 2**32, (n, 3), dtype=np.uint32)
        a[:, 2] &= 0x7fff
    return a


def plant(a, idx, value):
    if a.ndim == 1:
        a[idx] = value
    else:
        a[idx] = 0
        a[idx, 0] = value


@pytest.mark.timeout(300)
@pytest.mark.parametrize('modulus', [P61, P128], ids=hex)
def test_full_size_flat_scans_every_element(api, modulus):
    """flat 10^7: out[0] == a[0] and out[i] == out[i-1] o a[i] for every i, the right-hand side by the C oracle"""
    n = 10**7
    rs = np.random.default_rng(20261016)
    A = canonical_limbs(rs, modulus, n)
    plant(A, 5, 1)
    plant(A, n - 1000, 0)                                               # zeroes the last 1000 products
    F, a = device_array(api, modulus, A, (n,))
    cf = coracle.CField(modulus, False)
    for name, fn, op in (('cumsum', np.cumsum, coracle.ADD), ('cumprod', np.cumprod, coracle.MUL)):
        out = fn(a)
        assert out.shape == (n,)
        O = out._dev.to_numpy()
        assert O.shape == A.shape and O[0].tobytes() == A[0].tobytes(), name
        step = cf.ew(op, O[:-1], A[1:])
        assert step.tobytes() == O[1:].tobytes(), name
        if op == coracle.MUL:
            assert not O[n - 1000:].any() and O[n - 1001].any()


@pytest.mark.timeout(300)
def test_full_size_comparison_shape(api):
    """the cumsum of a secure comparison (runtime.np_sgn): axis 0 of (33, 10^6) over 2^80 - 65 (12-byte storage), every
    column step by the C oracle"""
    k, m = 33, 10**6
    rs = np.random.default_rng(20261017)
    A = canonical_limbs(rs, P80, k * m)
    F, a = device_array(api, P80, A, (k, m))
    out = np.cumsum(a, axis=0)
    assert out.shape == (k, m)
    O = out._dev.to_numpy()
    assert O[:m].tobytes() == A[:m].tobytes()
    cf = coracle.CField(P80, False)
    assert cf.ew(coracle.ADD, O[:-m], A[m:]).tobytes() == O[m:].tobytes()


@pytest.mark.timeout(300)
@pytest.mark.parametrize('shape,axis', [((3, 10**6), 1), ((10**6, 3), 1), ((3, 10**6), 0), ((10**6, 3), 0)], ids=str)
def test_full_size_prod_and_sum_along_an_axis(api, shape, axis):
    p = P61
    rs = np.random.default_rng(20261018)
    A = canonical_limbs(rs, p, shape[0] * shape[1])
    F, a = device_array(api, p, A, shape)
    v = [int(x) for x in A]
    rows = [v[r * shape[1]:(r + 1) * shape[1]] for r in range(shape[0])]
    lines = rows if axis == 1 else list(zip(*rows))
    want_sum = [sum(line) % p for line in lines]
    if len(lines) <= 3:
        want_prod = []
        for line in lines:
            acc = 1
            for x in line:
                acc = acc * x % p
            want_prod.append(acc)
    else:
        want_prod = [x * y % p * z % p for x, y, z in lines]
    assert ints(a.sum(axis=axis)) == want_sum
    assert ints(a.prod(axis=axis)) == want_prod


def test_c_abi(monkeypatch):
    """ffgpu_scan / ffgpu_axis_reduce / ffgpu_scan_workspace_bytes directly: statuses for overlap, zero sizes, overflowing
    products, a missing workspace; refused calls write nothing"""
    from mpyc_amd import _ffi
    L = _ffi.lib()
    ctx = make_ctx(monkeypatch, P61, False)
    h, eb = ctx._h, ctx.elem_bytes
    st = torch.cuda.current_stream(0).cuda_stream
    rng = random.Random(9)
    outer, k, inner = 2, 10000, 1                                       # three default tiles per line: needs a workspace
    n = outer * k * inner
    vals = draw(rng, P61, n)
    a, out = ctx.from_ints(vals), ctx.empty(n + outer)
    out.t.zero_()
    need = L.ffgpu_scan_workspace_bytes(h, outer, k, inner)
    assert need == outer * 3 * eb and need * 256 <= n * eb * 2
    assert L.ffgpu_scan_workspace_bytes(h, 1, 10**7, 1) * 256 <= 10**7 * eb + 256 * eb      # one element per 256 at most
    assert L.ffgpu_scan_workspace_bytes(h, 1, 33, 10**6) == 0                               # the column walk needs none
    ws = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    W = ws.data_ptr()
    assert L.ffgpu_scan(h, 0, a.ptr, out.ptr, outer, k, inner, 0, W, need, st) == _ffi.OK
    torch.cuda.synchronize()
    want = expect_scan(P61, False, vals, outer, k, inner, False)
    assert out.to_ints()[:n] == want
    assert L.ffgpu_axis_reduce(h, 1, a.ptr, out.ptr, outer, k, inner, W, need, st) == _ffi.OK
    torch.cuda.synchronize()
    assert out.to_ints()[:outer] == expect_reduce(P61, False, vals, outer, k, inner, True)
    out.t.zero_()
    torch.cuda.synchronize()
    E = _ffi.EINVAL
    big = 1 << 40
    refused = [
        L.ffgpu_scan(None, 0, a.ptr, out.ptr, outer, k, inner, 0, W, need, st),
        L.ffgpu_scan(h, 2, a.ptr, out.ptr, outer, k, inner, 0, W, need, st),              # no such operator
        L.ffgpu_scan(h, 0, None, out.ptr, outer, k, inner, 0, W, need, st),
        L.ffgpu_scan(h, 0, a.ptr, None, outer, k, inner, 0, W, need, st),
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, 0, k, inner, 0, W, need, st),                  # zero sizes
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, outer, 0, inner, 0, W, need, st),
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, outer, k, 0, 0, W, need, st),
        L.ffgpu_axis_reduce(h, 0, a.ptr, out.ptr, outer, 0, inner, W, need, st),
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, big, big, 2, 0, W, need, st),                  # outer * k * inner overflows
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, big, 3, big, 0, W, need, st),                  # outer * inner overflows
        L.ffgpu_axis_reduce(h, 0, a.ptr, out.ptr, big, big, big, W, need, st),
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, 1, (1 << 61), 1, 0, W, need, st),              # bytes overflow
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, outer, k, inner, 0, None, 0, st),              # several tiles, no workspace
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, outer, k, inner, 0, W, need - eb, st),         # too small
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, outer, k, inner, 0, W + 8, need, st),          # misaligned
        L.ffgpu_axis_reduce(h, 0, a.ptr, out.ptr, outer, k, inner, None, 0, st),
        L.ffgpu_scan(h, 0, a.ptr, a.ptr + eb, outer, k, inner, 0, W, need, st),           # overlap, not in place
        L.ffgpu_scan(h, 0, a.ptr + eb, a.ptr, outer, k - 1, inner, 0, W, need, st),
        L.ffgpu_scan(h, 0, a.ptr, a.ptr, outer, k, inner, 1, W, need, st),                # in place with the initial
        L.ffgpu_axis_reduce(h, 0, a.ptr, a.ptr, outer, k, inner, W, need, st),            # a reduction in place
        L.ffgpu_axis_reduce(h, 0, a.ptr, a.ptr + (n - 1) * eb, outer, k, inner, W, need, st),
        L.ffgpu_scan(h, 0, a.ptr, out.ptr, outer, k, inner, 0, a.ptr, need, st),          # workspace inside the operand
    ]
    assert refused == [E] * len(refused), refused
    assert L.ffgpu_scan_workspace_bytes(h, big, big, 2) == 0 and L.ffgpu_scan_workspace_bytes(h, 0, 5, 5) == 0
    assert L.ffgpu_scan_workspace_bytes(None, 1, 5, 1) == 0
    torch.cuda.synchronize()
    assert not out.t.any() and a.to_ints() == vals                                         # refused calls wrote nothing
    assert L.ffgpu_scan(h, 0, a.ptr, a.ptr, outer, k, inner, 0, W, need, st) == _ffi.OK    # in place is allowed
    torch.cuda.synchronize()
    assert a.to_ints() == want
    # the engine refuses what the library would
    b = ctx.from_ints(vals)
    from mpyc_amd.engine import DevArray
    with pytest.raises(ValueError):
        ctx.scan(b, outer, k, inner, out=DevArray(ctx, b.t[1:], n - 1))
    with pytest.raises(ValueError):                                                        # overlapping, not identical
        ctx.scan(DevArray(ctx, b.t[:n - outer], n - outer), outer, k - 1, inner, out=DevArray(ctx, b.t[1:n - outer + 1], n - outer))
    with pytest.raises(ValueError):
        ctx.scan(b, outer, k, inner, with_initial=True, out=b)
    with pytest.raises(ValueError):
        ctx.axis_reduce(b, outer, k, inner, out=DevArray(ctx, b.t[:outer], outer))
    with pytest.raises(ValueError):
        ctx.scan(b, outer, 0, inner)
    with pytest.raises(ValueError):
        ctx.scan(b, outer, k + 1, inner)
    # a stream of its own has a workspace of its own
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side):
        o2 = ctx.scan(b, outer, k, inner)
    side.synchronize()
    assert o2.to_ints() == want


@pytest.mark.timeout(120)
def test_memory_is_the_output_and_the_tile_aggregates(api):
    """a flat cumsum of 10^7 elements over 2^61 - 1 allocates its output and at most one aggregate per 256 elements (plus
    1 MiB of allocator rounding); the composed route held one more whole array beside its result"""
    n = 10**7
    rs = np.random.default_rng(20261019)
    F, a = device_array(api, P61, canonical_limbs(rs, P61, n), (n,))
    eb = a.ctx.elem_bytes
    assert eb == 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = np.cumsum(a)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak extra memory of a flat cumsum of 10^7: {extra} bytes (output: {n * eb})')
    assert out.shape == (n,)
    assert extra <= n * eb + n * eb // 256 + (1 << 20), extra


def median_pair(new, old):
    """alternating, one warm-up pair, median of five by device events (ms)"""
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        del r
        return e0.elapsed_time(e1)
    timed(new), timed(old)
    tn, to = [], []
    for _ in range(5):
        tn.append(timed(new))
        to.append(timed(old))
    return statistics.median(tn), statistics.median(to)


@pytest.mark.timeout(300)
@pytest.mark.parametrize('shape,axis', [((10**7,), 0), ((33, 10**6), 0)], ids=str)
def test_not_slower_than_the_composed_route(api, shape, axis):
    """np.cumsum over 2^61 - 1 against the retained Hillis-Steele helper called directly, same process, alternating"""
    finfields, _ = api
    n = int(np.prod(shape))
    rs = np.random.default_rng(20261020)
    F, a = device_array(api, P61, canonical_limbs(rs, P61, n), shape)
    new = lambda: np.cumsum(a, axis=axis)
    old = lambda: finfields._scan_hillis_steele(a, axis, False)
    assert new()._dev.to_numpy().tobytes() == old()._dev.to_numpy().tobytes()
    t_new, t_old = median_pair(new, old)
    print(f'cumsum {shape} axis {axis}: kernels {t_new:.3f} ms, composed {t_old:.3f} ms, ratio {t_old / t_new:.1f}')
    assert t_new < t_old, (t_new, t_old)
