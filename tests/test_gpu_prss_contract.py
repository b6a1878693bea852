"""ffgpu_prss_combine (k_prss) and ffgpu_prss_chacha (k_prss_chacha) at their per-call limits, at every draw and mask width,
on crafted draws, with accumulate != 0 and at the edges of their launch geometry, on every field policy, byte for byte against
Python integers and oracle/pyoracle, through the C ABI with `out` a view between guards (aligned, and one element in) and the
streams at odd byte offsets.

combine: l = 1..64 (every partial top limb of every word width, the plain reduction of l <= LB, 1 to 16 Horner steps); draws
crafted around the multiples of p and the limb boundaries, under the weights 0, 1, q - 1 and a random one; every mask width
that selects a branch of the 16- and 24-byte words, with every bit above the mask set; 48 streams, 96 weights and one past
each, every bad argument, 2^mask_bits > order, n = 0; accumulate on a preload of q - 1 and on edge values, and 48 streams split
at 1, 24 and 47 over two calls; n around one and two workgroups, and n = 2 G + 1 on a grid capped at G threads, where the
grid-stride loop of k_prss iterates.
chacha: 32 streams, 64 weights and one past each, l = 65, rounds = 10; the same accumulate checks with 32 streams split at 1,
16 and 31; every tile shape (tb, dpt) that l = 1..64 produces, at n around one workgroup of tiles and two workgroups plus a
cut tile, d = 1 and 3.  (Its width and mask sweeps are tests/test_prss_chacha.py::test_every_draw_width_and_mask; a block
counter that crosses 2^32 needs more than 10^8 elements and stays unmeasured.)
The mirror: m = 9, t = 4 -- 70 subset keys per party, three and five launches for the zero sharing -- in both PRF modes.

The case logic, the references and the layout are tests/prss_contract.py; tests/test_prss_contract_host.py shows that driver
fails when it should.  Expected values never come from the library.

Wall time on the MI355X: the slowest test takes 1.7 s (test_chacha_geometry of the first field, which restates the keystream
that the other fields reuse; 0.2 s after that), the m = 9 mirror tests 0.5 to 1.4 s, the module 20 s."""
import itertools

import pytest

import prss_contract as pc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def ids_of(fields):
    return [('gf2:' if b else '') + hex(m) for m, b in fields]


FIELDS = pc.contract_fields()
PRIMES = [f for f in FIELDS if not f[1]]
GEOMETRY = pc.GEOMETRY_FIELDS
MIRROR_FIELDS = [(2**61 - 1, False), (2**128 - 173, False), (0x1000000000000001b, True)]

_ctxs = {}


def default_ctx(modulus, binary):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from mpyc_amd import engine
    if (modulus, binary) not in _ctxs:
        _ctxs[modulus, binary] = engine.FieldContext(modulus, binary, device=0)
    return _ctxs[modulus, binary]


def env_ctx(monkeypatch, modulus, binary, name, value):
    """a context of its own with one launch switch set (they are read at creation)"""
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from mpyc_amd import engine
    monkeypatch.setenv(name, value)
    ctx = engine.FieldContext(modulus, binary, device=0)
    monkeypatch.delenv(name)
    return ctx


def driver(modulus, binary, ctx=None):
    ctx = ctx or default_ctx(modulus, binary)
    assert ctx.order == po.Field(modulus, binary).order
    return pc.Driver(pc.GpuAdapter(ctx), modulus, binary)


def test_fields_cover_every_word_width():
    assert sorted({pc.elem_bytes(m, b) for m, b in FIELDS}) == [1, 4, 8, 12, 16, 24]
    assert {default_ctx(m, b).reduction for m, b in ((2**136 - 113, False), pc.MONT192)} == {'pseudo-mersenne', 'montgomery'}
    assert sorted({pc.limb_bytes(pc.elem_bytes(m, b)) for m, b in GEOMETRY}) == [1, 4, 8, 16, 24]
    assert sorted({pc.elem_bytes(m, b) for m, b in GEOMETRY if not b}) == [4, 8, 12, 16, 24]


# ---- ffgpu_prss_combine ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_combine_every_draw_width(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_width_sweep()
    assert drv.cases == 64 * 2 * 2 and all(('width', l, kind) in drv.seen for l in range(1, 65) for kind in ('ramp', 'random'))
    print('%d cases' % drv.cases)


@pytest.mark.parametrize('modulus,binary', PRIMES, ids=ids_of(PRIMES))
def test_combine_crafted_draws(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_crafted()
    widths = pc.crafted_widths(modulus, drv.LB)
    assert {drv.LB, min(2 * drv.LB + 1, 64), min(drv.l0, 64), 64} <= set(widths)
    assert drv.cases == len(widths) * 2 * 4 * 2
    assert all(('crafted', l, d, w) in drv.seen for l in widths for d in (1, 3) for w in pc.CRAFTED_WEIGHTS)
    print('%d cases, l in %r' % (drv.cases, widths))


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_combine_every_mask_width(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_mask_sweep()
    masks = pc.mask_widths(drv.F, drv.bits)
    if binary:
        assert masks == list(range(1, drv.F.n + 1))
    else:
        assert set(masks) == {mb for mb in pc.MASK_WIDTHS + (drv.bits - 2, drv.bits - 1) if 1 <= mb < drv.bits}
    assert drv.cases == len(masks) * 2 * 2 and all(('mask', mb, (mb + 7) // 8 + 16) in drv.seen for mb in masks)
    print('%d cases' % drv.cases)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_combine_limits(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_limits()
    assert drv.cases == 4 * 2 + 8 + 1
    assert all(('combine', 'runs', ks, d) in drv.seen for ks, d in ((48, 1), (48, 2), (1, 96), (32, 3)))
    refused = {k[2]: k[3] for k in drv.seen if k[:2] == ('combine', 'refused')}
    assert refused == {'ks=49': pc.ENOTSUP, 'ks*d=97': pc.ENOTSUP, 'ks=33 d=3': pc.ENOTSUP, 'l=65': pc.EINVAL, 'l=0': pc.EINVAL,
                       'd=0': pc.EINVAL, 'null stream': pc.EINVAL, '2^mask_bits > order': pc.EINVAL}
    print('%d cases' % drv.cases)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_combine_accumulate(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_accumulate()
    assert drv.cases == (2 + 3) * 2 and drv.calls == drv.cases + 3 * 2
    assert all(('combine', 'split', a) in drv.seen for a in (1, 24, 47))
    print('%d cases' % drv.cases)


@pytest.mark.parametrize('modulus,binary', GEOMETRY, ids=ids_of(GEOMETRY))
def test_combine_geometry(monkeypatch, modulus, binary):
    """the default grid, and FFGPU_BLOCKS_PER_CU=1: G = CUs x 256 threads and n = 2 G + 1, so every thread of k_prss loops twice
    and one a third time"""
    drv = driver(modulus, binary)
    drv.run_geometry()
    assert drv.cases == 6 * 2
    capped = driver(modulus, binary, env_ctx(monkeypatch, modulus, binary, 'FFGPU_BLOCKS_PER_CU', '1'))
    G = torch.cuda.get_device_properties(0).multi_processor_count * pc.BLOCK
    capped.run_capped(G)
    assert capped.cases == 2 and ('geometry', 'grid of %d threads' % G, 2 * G + 1) in capped.seen
    print('%d + %d cases, n = %d on the capped grid' % (drv.cases, capped.cases, 2 * G + 1))


# ---- ffgpu_prss_chacha -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_chacha_limits_and_accumulate(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_limits('chacha')
    assert drv.cases == 4 * 2 + 6
    assert all(('chacha', 'runs', ks, d) in drv.seen for ks, d in ((32, 1), (32, 2), (1, 64), (16, 4)))
    refused = {k[2]: k[3] for k in drv.seen if k[:2] == ('chacha', 'refused')}
    assert refused == {'ks=33': pc.ENOTSUP, 'ks*d=65': pc.ENOTSUP, 'ks=17 d=4': pc.ENOTSUP, 'l=65': pc.EINVAL,
                       'rounds=10': pc.EINVAL, '2^mask_bits > order': pc.EINVAL}
    drv.run_accumulate('chacha', n=19)
    assert drv.cases == 4 * 2 + 6 + (2 + 3) * 2 and all(('chacha', 'split', a) in drv.seen for a in (1, 16, 31))
    print('%d cases' % drv.cases)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_chacha_geometry(modulus, binary):
    drv = driver(modulus, binary)
    drv.run_cc_geometry()
    shapes = pc.cc_tile_shapes()
    assert set(shapes) == {po.prss_chacha_layout(l) for l in range(1, 65)} and len(shapes) == 10
    assert drv.cases == len(shapes) * 2 * 4 * 2
    assert all(('cc-geometry', tb, dpt, d, n) in drv.seen for tb, dpt in shapes for d in (1, 3) for n in pc.cc_geometry_sizes(dpt))
    print('%d cases, tile shapes %r' % (drv.cases, sorted(shapes)))


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def keys_for(m, t, i):
    return {S: bytes([(11 * sum(S) + 3 * len(S) + b) % 251 for b in range(16)])
            for S in itertools.combinations(range(m), m - t) if i in S}


@pytest.mark.parametrize('prf', ['shake', 'chacha'])
@pytest.mark.parametrize('modulus,binary', MIRROR_FIELDS, ids=ids_of(MIRROR_FIELDS))
def test_mirror_chunks_70_keys(monkeypatch, modulus, binary, prf):
    """m = 9, t = 4: C(8, 4) = 70 subset keys per party -- two and three launches for a share, three and five (d = 4) for a zero
    sharing, all but the first accumulating.  Parties 0 and 8 against the oracle, both conventions of the zero sharing; all
    nine on the device: two sets of t + 1 recombine to one secret, 2t + 1 zero shares to 0."""
    import numpy as np
    from mpyc_amd import engine, finfields, gfpx, thresha
    assert torch.cuda.is_available()
    m, t, n = 9, 4, 37
    chacha = prf == 'chacha'
    monkeypatch.setattr(thresha, 'prss_prf', prf)
    monkeypatch.setattr(thresha, 'prss_rounds', 8)
    monkeypatch.setattr(thresha, 'prss_allow_chacha8', True)
    launches = []
    for name in ('prss_combine', 'prss_chacha'):
        def counted(self, *a, _inner=getattr(engine.FieldContext, name), **kw):
            launches.append(bool(kw.get('accumulate')))
            return _inner(self, *a, **kw)
        monkeypatch.setattr(engine.FieldContext, name, counted)
    F = finfields.GF(gfpx.BinaryPolynomial(modulus)) if binary else finfields.GF(modulus)
    OF = po.Field(modulus, binary)
    share = po.np_pseudorandom_share_chacha if chacha else po.np_pseudorandom_share
    zero = po.np_pseudorandom_share_0_chacha if chacha else po.np_pseudorandom_share_0
    kw = {'rounds': 8} if chacha else {}
    ints = lambda a: [int(v) for v in np.asarray(a.value).reshape(-1)]
    shares, zeros = [], []
    for i in range(m):
        keys = keys_for(m, t, i)
        assert len(keys) == 70
        prfs = {S: thresha.PRF(k, F.order) for S, k in keys.items()}
        del launches[:]
        shares.append(thresha.np_pseudorandom_share(F, m, i, prfs, b'u', n))
        assert launches == [False] + [True] * (2 if chacha else 1)
        del launches[:]
        zeros.append(thresha.np_pseudorandom_share_0(F, m, i, prfs, b'u', n))
        assert launches == [False] + [True] * (4 if chacha else 2)
        if i in (0, m - 1):
            assert ints(shares[-1]) == share(OF, m, i, keys, F.order, b'u', n, **kw), (prf, i)
            assert ints(zeros[-1]) == zero(OF, m, i, keys, F.order, b'u', n, **kw), (prf, i)
            assert [int(v.value) for v in thresha.pseudorandom_share_zero(F, m, i, prfs, b'u', n)] == \
                zero(OF, m, i, keys, F.order, b'u', n, list_convention=True, **kw)
    a = thresha.np_recombine(F, [(i + 1, shares[i]) for i in range(t + 1)])
    b = thresha.np_recombine(F, [(i + 1, shares[i]) for i in range(m - t - 1, m)])
    assert ints(a) == ints(b)
    assert ints(thresha.np_recombine(F, [(i + 1, zeros[i]) for i in range(2 * t + 1)])) == [0] * n and any(ints(zeros[0]))
    with pytest.raises(NotImplementedError, match='exceeds the field order'):
        thresha.np_pseudorandom_share(F, m, 0, {S: thresha.PRF(k, 1 << OF.order.bit_length()) for S, k in keys_for(m, t, 0).items()}, b'u', n)
