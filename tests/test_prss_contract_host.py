"""The driver of the PRSS contract tests (tests/prss_contract.py) without a GPU: it passes on the Python-integer context of
tests/cpuctx.py, it fails -- in the check meant for it, with the right kind of violation -- on contexts that are wrong the
way k_prss, k_prss_chacha or their launchers could be, what it enumerates and restates is what the library and the mirror
use, and the mirror's chunking of a call with more subset keys than one launch takes gives the reference's shares with both
PRFs.  A driver that cannot see these mutants would not see the kernel bugs it exists for."""
import functools
import itertools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import prss_contract as pc
from cpuctx import CpuFieldContext
from ew_contract import ContractViolation
from oracle import pyoracle as po

P31, P61, P96, P128, P136 = ((2**31 - 1, False), (2**61 - 1, False), (2**96 - 17, False), (2**128 - 173, False),
                             (2**136 - 113, False))
GF256, GF64 = (0x11b, True), (0x1000000000000001b, True)
FIELDS = [P31, P61, P96, P128, P136, GF256, GF64]         # one prime per word width, GF(2^8), GF(2^64)
PRIMES = [f for f in FIELDS if not f[1]]
IDS = [('gf2:' if b else '') + hex(m) for m, b in FIELDS]
WIDTHS = (1, 3, 4, 5, 8, 9, 15, 16, 17, 23, 24, 25, 32, 33, 47, 48, 49, 63, 64)       # thinned: Python integers on both sides


def driver(cls, modulus, binary, adapter=pc.CpuAdapter):
    return pc.Driver(adapter(cls(modulus, binary)), modulus, binary)


# ---- the honest context passes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_combine_passes_on_the_integer_context(modulus, binary):
    drv = driver(CpuFieldContext, modulus, binary)
    drv.run_width_sweep(WIDTHS, n=19)
    assert drv.cases == len(WIDTHS) * 2 * 2
    cases = drv.cases
    masks = pc.mask_widths(drv.F, drv.bits)
    thin = [mb for mb in masks if mb in pc.MASK_WIDTHS or mb >= drv.bits - 2] if not binary else masks[::7] + masks[-1:]
    drv.run_mask_sweep(thin, n=8)
    assert drv.cases == cases + len(thin) * 2 * 2
    cases = drv.cases
    drv.run_limits()
    assert drv.cases == cases + 4 * 2 + 8 + 1
    cases = drv.cases
    drv.run_accumulate(n=7)
    assert drv.cases == cases + (2 + 3) * 2 and drv.calls == drv.cases + 3 * 2
    cases = drv.cases
    drv.run_geometry(sizes=(1, 31, 33))
    drv.run_capped(16)
    assert drv.cases == cases + 3 * 2 + 2


@pytest.mark.parametrize('modulus,binary', PRIMES, ids=IDS[:len(PRIMES)])
def test_crafted_draws_pass_on_the_integer_context(modulus, binary):
    drv = driver(CpuFieldContext, modulus, binary)
    drv.run_crafted()
    widths = pc.crafted_widths(modulus, drv.LB)
    assert drv.cases == len(widths) * 2 * 4 * 2 and {drv.LB, 2 * drv.LB, 64} <= set(widths)
    for l in widths:
        names = [nm for nm, _ in pc.crafted_values(modulus, drv.LB, l)]
        assert {'0', 'p-1', '2^(8l)-1', 'top multiple of p', 'every limb 2^(8LB)-1'} <= set(names)
        assert ('p' in names) == (modulus < 1 << 8 * l) and ('2^(8LB)' in names) == (l > drv.LB)


@pytest.mark.parametrize('modulus,binary', [P61, P136, GF256], ids=['p61', 'p136', 'gf256'])
def test_chacha_passes_on_the_integer_context(modulus, binary):
    drv = driver(CpuFieldContext, modulus, binary)
    drv.run_limits('chacha', n=3)
    assert drv.cases == 4 * 2 + 6
    drv.run_accumulate('chacha', n=5)
    assert drv.cases == 4 * 2 + 6 + 5 * 2


def test_chacha_geometry_passes_on_the_integer_context(monkeypatch):
    """every tile shape, at sizes cut down to a workgroup of four threads"""
    monkeypatch.setattr(pc, 'BLOCK', 4)
    drv = driver(CpuFieldContext, *P61)
    drv.run_cc_geometry()
    assert drv.cases == len(pc.cc_tile_shapes()) * 2 * 4 * 2


# ---- what the driver enumerates and restates ---------------------------------------------------------------------------------
def test_enumerations_are_complete():
    shapes = pc.cc_tile_shapes()
    assert all(pc.cc_layout(l) == po.prss_chacha_layout(l) for l in range(1, 65))
    assert set(shapes) == {po.prss_chacha_layout(l) for l in range(1, 65)} and len(shapes) == 10
    assert all(po.prss_chacha_layout(l) == shape for shape, l in shapes.items())
    assert all(1 <= tb <= pc.CC_MAXTB and 1 <= dpt <= pc.CC_MAXDPT for tb, dpt in shapes)
    # one limb width of every kind, and the limits, against the sources that hold them
    assert [pc.limb_bytes(eb) for eb in (1, 4, 8, 12, 16, 24)] == [1, 4, 8, 16, 16, 24]
    assert sorted({pc.elem_bytes(m, b) for m, b in pc.contract_fields()}) == [1, 4, 8, 12, 16, 24]
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'mpyc_amd', 'csrc', 'kernels.hpp')) as fh:
        src = fh.read()
    enums = dict(re.findall(r'(PRSS_\w+) = (\d+)', src))
    assert [int(enums[k]) for k in ('PRSS_MAXS', 'PRSS_MAXW', 'PRSS_CC_MAXS', 'PRSS_CC_MAXW', 'PRSS_CC_MAXDPT', 'PRSS_CC_MAXTB')] \
        == [pc.MAXS, pc.MAXW, pc.CC_MAXS, pc.CC_MAXW, pc.CC_MAXDPT, pc.CC_MAXTB]
    with open(os.path.join(root, 'mpyc_amd', 'thresha.py')) as fh:
        mirror = fh.read()
    assert 'min(%d, %d // d)' % (pc.MAXS, pc.MAXW) in mirror and 'min(%d, %d // d)' % (pc.CC_MAXS, pc.CC_MAXW) in mirror
    with open(os.path.join(root, 'include', 'ffgpu.h')) as fh:
        header = fh.read()
    assert 'ks <= 48 and ks * d <= 96 (FFGPU_ENOTSUP' in header and 'ks <= 32 and\n * ks * d <= 64 (FFGPU_ENOTSUP' in header
    assert pc.chunk_sizes(70, 4, False) == [24, 24, 22] and pc.chunk_sizes(70, 4, True) == [16, 16, 16, 16, 6]
    assert pc.chunk_sizes(70, 1, False) == [48, 22] and pc.chunk_sizes(70, 1, True) == [32, 32, 6]


def test_the_reference_of_the_driver():
    """mul_by is po.mul; combine_ref on real SHAKE streams is po.np_pseudorandom_share; chacha_ref is the oracle's"""
    import random
    from hashlib import shake_128
    rng = random.Random(5)
    for modulus, binary in FIELDS:
        F = po.Field(modulus, binary)
        for _ in range(20):
            w, x = rng.randrange(F.order), rng.randrange(F.order)
            assert pc.mul_by(F, w)(x) == po.mul(F, x, w)
        m, t, i, n = 5, 2, 1, 11
        keys = {S: bytes([sum(S), len(S)] * 8) for S in itertools.combinations(range(m), m - t) if i in S}
        l = (F.n + 7) // 8 if binary else ((F.order - 1).bit_length() + 7) // 8 + 16
        streams = [shake_128(k + b'u').digest(n * l) for k in keys.values()]
        weights = [po.f_S_i(F, m, i, S) for S in keys]
        assert pc.combine_ref(F, streams, 1, l, F.n if binary else 0, weights, n) == \
            po.np_pseudorandom_share(F, m, i, keys, F.order, b'u', n)
        k40 = [po.prss_chacha_stream_key(k, b'u') for k in keys.values()]
        assert pc.chacha_ref(F, k40, 1, l, F.n if binary else 0, 20, weights, n) == \
            po.np_pseudorandom_share_chacha(F, m, i, keys, F.order, b'u', n)


# ---- wrong contexts ----------------------------------------------------------------------------------------------------------
class KernelLike(CpuFieldContext):
    """prss_combine draw by draw the way k_prss goes about it, with one thing wrong (`flaw`)"""
    flaw = None

    def draw(self, raw, o, l, mask_bits):
        LB, flaw, p = pc.limb_bytes(self.elem_bytes), self.flaw, self.order
        if mask_bits:
            v = int.from_bytes(raw[o:o + min(l, LB)], 'little')
            if flaw == 'mask: low limb only' and mask_bits >= 64:
                return v & (2**64 - 1)
            return v & ((1 << mask_bits) - 1)
        top = (l - 1) // LB * LB
        nb = l - top
        if flaw == 'top limb: one byte more' and nb < LB:
            nb += 1
        if flaw == 'top limb: a full limb':
            nb = LB
        v = int.from_bytes(raw[o + top:o + top + nb], 'little') << (8 * top) | int.from_bytes(raw[o:o + top], 'little')
        if flaw == 'no final reduction' and v and v % p == 0 and (v == p or v + p >= 1 << 8 * l):
            return p
        return v % p

    def prss_combine(self, streams, d, l, weights, n, mask_bits=0, out=None, accumulate=False):
        flaw, F, ks = self.flaw, self.F, len(streams)
        pre = out.to_ints()
        if flaw == 'accumulate: overwrites' and accumulate:
            return out
        acc = pre if accumulate and flaw != 'accumulate: ignored' else [0] * n
        stride = (l + 3) // 4 * 4 if flaw == 'stride: 4 bytes' else l
        for s, sb in enumerate(streams):
            raw = bytes(sb.numpy().tobytes())
            for h in range(n):
                for j in range(d):
                    w = weights[j * ks + s] if flaw == 'weights: transposed' else weights[s * d + j]
                    x = self.draw(raw, (h * d + j) * stride, l, mask_bits)
                    acc[h] = po.add(F, acc[h], po.mul(F, po.reduce(F, x), w)) if F.binary else acc[h] + x * w
        if F.binary:
            return self._put(out, acc)
        p = self.order
        # the last step of the kernel: one conditional subtraction that the flawed draw escapes
        return self._put(out, [v if flaw == 'no final reduction' and v == p else v % p for v in acc])


def flawed(flaw):
    return type('KernelLike_' + flaw.replace(' ', '_').replace(':', ''), (KernelLike,), {'flaw': flaw})


class LeavesTheRestUnderACappedGrid(pc.CpuAdapter):
    """(9) k_prss without its grid-stride loop on a grid of 16 threads"""

    def combine(self, buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n):
        return super().combine(buf, streams, ks, d, l, mask_bits, weights, accumulate, out, min(n, 16))


class WritesElementN(pc.CpuAdapter):
    """(10)"""

    def combine(self, buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n):
        rc = super().combine(buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n)
        if rc == pc.OK and n:
            buf[out + n * self.eb:out + (n + 1) * self.eb] = 0
        return rc

    def chacha(self, buf, keys40, ks, d, l, mask_bits, rounds, weights, accumulate, out, n):
        rc = super().chacha(buf, keys40, ks, d, l, mask_bits, rounds, weights, accumulate, out, n)
        if rc == pc.OK and n % pc.cc_layout(l)[1]:                 # the tile that the end of the array cuts is stored whole
            buf[out + n * self.eb:out + (n + 1) * self.eb] = 0
        return rc


class ModifiesAStreamByte(pc.CpuAdapter):
    """(11)"""

    def combine(self, buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n):
        rc = super().combine(buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n)
        if rc == pc.OK and n:
            buf[streams[-1] + n * d * l - 1] ^= 1
        return rc


class ARefusedCallWritesOut(pc.CpuAdapter):
    """(12)"""

    def combine(self, buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n):
        rc = super().combine(buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n)
        if rc != pc.OK:
            buf[out:out + self.eb] = 0
        return rc

    def chacha(self, buf, keys40, ks, d, l, mask_bits, rounds, weights, accumulate, out, n):
        rc = super().chacha(buf, keys40, ks, d, l, mask_bits, rounds, weights, accumulate, out, n)
        if rc != pc.OK:
            buf[out:out + self.eb] = 0
        return rc


class ChachaIgnoresAccumulate(CpuFieldContext):
    """(1) on the second entry point"""

    def prss_chacha(self, keys40, d, l, weights, n, mask_bits=0, rounds=20, out=None, accumulate=False):
        return super().prss_chacha(keys40, d, l, weights, n, mask_bits, rounds, out, False)


def named(name, fn):
    fn.__name__ = name
    return fn


def widths(*ls):
    return named('widths_' + '_'.join(map(str, ls)), lambda drv: drv.run_width_sweep(ls, n=9))


def masks(*mbs):
    return named('masks_' + '_'.join(map(str, mbs)), lambda drv: drv.run_mask_sweep(mbs, n=6))


def accumulate(drv):
    drv.run_accumulate(n=5)


def cc_accumulate(drv):
    drv.run_accumulate('chacha', n=3)


def limits(drv):
    drv.run_limits(n=3)


def cc_limits(drv):
    drv.run_limits('chacha', n=3)


def crafted(drv):
    drv.run_crafted()


def capped(drv):
    drv.run_capped(16)


def geometry(drv):
    drv.run_geometry(sizes=(1, 31))


def within_the_grid(drv):
    drv.run_geometry(sizes=(1, 15, 16))


def cc_geometry(drv):
    drv.run_cc_geometry({(1, 5): 9})


# (context, adapter, the part of the matrix meant to catch it, kind of violation, words of its message, fields)
WRONG = [
    (flawed('accumulate: ignored'), pc.CpuAdapter, accumulate, 'out', 'preload q-1', [P61, GF256]),
    (flawed('accumulate: ignored'), pc.CpuAdapter, limits, None, '', [P61]),                         # nothing accumulates: it passes
    (flawed('accumulate: overwrites'), pc.CpuAdapter, accumulate, 'out', 'preload q-1', [P61, GF256]),
    (ChachaIgnoresAccumulate, pc.CpuAdapter, cc_accumulate, 'out', 'preload q-1', [P61]),
    (flawed('weights: transposed'), pc.CpuAdapter, widths(24), 'out', 'width', [P61, P128]),
    (flawed('stride: 4 bytes'), pc.CpuAdapter, widths(8, 24, 64), None, '', [P61]),                   # whole words: it passes
    (flawed('stride: 4 bytes'), pc.CpuAdapter, widths(24, 25), 'out', 'l=25', [P61, P136]),
    (flawed('top limb: one byte more'), pc.CpuAdapter, widths(8, 16, 24), None, '', [P61]),           # no partial limb: it passes
    (flawed('top limb: one byte more'), pc.CpuAdapter, widths(24, 25), 'out', 'l=25', [P61, P136]),
    (flawed('top limb: one byte more'), pc.CpuAdapter, widths(16, 24), 'out', 'l=24', [P96, P128]),     # 16-byte limbs
    (flawed('mask: low limb only'), pc.CpuAdapter, masks(1, 33, 63), None, '', [P128]),               # inside the low limb: it passes
    (flawed('mask: low limb only'), pc.CpuAdapter, masks(63, 65), 'out', 'mask=65', [P96, P128, P136]),
    (flawed('top limb: a full limb'), pc.CpuAdapter, widths(17, 24), 'out', 'l=17', [P61, P128]),
    (flawed('no final reduction'), pc.CpuAdapter, widths(8, 24, 33), None, '', [P61]),                # random draws: it passes
    (flawed('no final reduction'), pc.CpuAdapter, crafted, 'canonical', 'top multiple of p', PRIMES),
    (CpuFieldContext, LeavesTheRestUnderACappedGrid, within_the_grid, None, '', [P61]),               # no thread loops: it passes
    (CpuFieldContext, LeavesTheRestUnderACappedGrid, capped, 'out', 'element 16 of 33', [P61, GF256]),
    (CpuFieldContext, WritesElementN, geometry, 'guard', 'guard byte', [P61, P136, GF256]),
    (CpuFieldContext, WritesElementN, cc_geometry, 'guard', 'guard byte', [P61]),
    (CpuFieldContext, ModifiesAStreamByte, geometry, 'input', 'stream 1 changed', [P61, GF256]),
    (CpuFieldContext, ARefusedCallWritesOut, limits, 'out', 'refused ks=49', [P61, GF256]),
    (CpuFieldContext, ARefusedCallWritesOut, cc_limits, 'out', 'refused ks=33', [P61]),
]


@pytest.mark.parametrize('cls,adapter,part,kind,words,fields', WRONG,
                         ids=['%s-%s-%s-%s' % (c.__name__, a.__name__, p.__name__, k) for c, a, p, k, _, _ in WRONG])
def test_driver_fails_on_a_wrong_context(cls, adapter, part, kind, words, fields):
    for modulus, binary in fields:
        drv = driver(cls, modulus, binary, adapter)
        if kind is None:
            part(drv)
            continue
        with pytest.raises(ContractViolation) as err:
            part(drv)
        assert kind in err.value.kinds and words in str(err.value), (cls.__name__, hex(modulus), str(err.value))
        good = driver(CpuFieldContext, modulus, binary)          # and the same part passes on the honest context
        part(good)
        assert good.cases > drv.cases


def test_kernel_like_context_is_honest_without_a_flaw():
    for modulus, binary in (P61, P96, P136):
        drv = driver(KernelLike, modulus, binary)
        drv.run_width_sweep((1, 15, 16, 17, 25, 48, 64), n=5)
        drv.run_mask_sweep(n=4)
        drv.run_crafted()
        drv.run_accumulate(n=3)


# ---- the mirror's chunking ---------------------------------------------------------------------------------------------------
def keys_for(m, t, i):
    return {S: bytes([(11 * sum(S) + 3 * len(S) + b) % 251 for b in range(16)])
            for S in itertools.combinations(range(m), m - t) if i in S}


@pytest.mark.parametrize('m,t', [(9, 4), (8, 3)])
def test_mirror_chunks_a_call_with_more_keys_than_a_launch_takes(monkeypatch, m, t):
    """np_pseudorandom_share, np_pseudorandom_share_0 and the list versions of every party against the oracle, for bound = order
    and a power of two, with both PRFs (ChaCha8: the rounds are a loop count); the launches are counted on the stand-in; shares
    recombine to one secret from two sets of t + 1 parties, zero sharings to 0 from 2t + 1"""
    from cpuctx import use_cpu_contexts
    import mpyc_amd.finfields as gff
    import mpyc_amd.thresha as gth
    use_cpu_contexts(monkeypatch)
    monkeypatch.setattr(gff, '_ctx_cache', {})
    gff._pGF.cache_clear()
    launches = {'shake': 0, 'chacha': 0}
    for name, key in (('prss_combine', 'shake'), ('prss_chacha', 'chacha')):
        def counted(self, *a, _inner=getattr(CpuFieldContext, name), _key=key, **kw):
            launches[_key] += 1
            return _inner(self, *a, **kw)
        monkeypatch.setattr(CpuFieldContext, name, counted)
    monkeypatch.setattr(gth, 'prss_rounds', 8)
    monkeypatch.setattr(gth, 'prss_allow_chacha8', True)
    # the stand-in and the oracle ask for the same keystream blocks (pinned to RFC 8439 by tests/test_prss_chacha.py): once each
    monkeypatch.setattr(po, 'chacha_block', functools.lru_cache(maxsize=None)(po.chacha_block))
    p, n = 2**61 - 1, 37
    F, OF = gff.GF(p), po.Field(p)
    nkeys = len(keys_for(m, t, 0))
    assert nkeys == {(9, 4): 70, (8, 3): 35}[m, t]
    ints = lambda a: [int(v) for v in np.asarray(a.value)]
    for bound in (p, 1 << 40):
        for prf in ('shake', 'chacha'):
            monkeypatch.setattr(gth, 'prss_prf', prf)
            chacha = prf == 'chacha'
            share = po.np_pseudorandom_share_chacha if chacha else po.np_pseudorandom_share
            zero = po.np_pseudorandom_share_0_chacha if chacha else po.np_pseudorandom_share_0
            kw = {'rounds': 8} if chacha else {}
            shares, zeros = [], []
            for i in range(m):
                keys = keys_for(m, t, i)
                prfs = {S: gth.PRF(k, bound) for S, k in keys.items()}
                launches[prf] = 0
                shares.append(ints(gth.np_pseudorandom_share(F, m, i, prfs, b'u', n)))
                assert launches[prf] == len(pc.chunk_sizes(nkeys, 1, chacha))
                assert shares[-1] == share(OF, m, i, keys, bound, b'u', n, **kw), (prf, bound, i)
                launches[prf] = 0
                zeros.append(ints(gth.np_pseudorandom_share_0(F, m, i, prfs, b'u', n)))
                assert launches[prf] == len(pc.chunk_sizes(nkeys, t, chacha))
                if (m, t) == (9, 4):
                    assert launches[prf] == (5 if chacha else 3)
                assert zeros[-1] == zero(OF, m, i, keys, bound, b'u', n, **kw), (prf, bound, i)
                if i in (0, m - 1):
                    assert [int(v.value) for v in gth.pseudorandom_share(F, m, i, prfs, b'u', n)] == shares[-1]
                    assert [int(v.value) for v in gth.pseudorandom_share_zero(F, m, i, prfs, b'u', n)] == \
                        zero(OF, m, i, keys, bound, b'u', n, list_convention=True, **kw)
            secret = po.np_recombine(OF, [(i + 1, shares[i]) for i in range(t + 1)])
            assert po.np_recombine(OF, [(i + 1, shares[i]) for i in range(m - t - 1, m)]) == secret
            assert po.np_recombine(OF, [(i + 1, zeros[i]) for i in range(2 * t + 1)]) == [0] * n and any(zeros[0])
    # a power of two above the order is refused by the mirror, and by the stand-in as by the C entry points
    monkeypatch.setattr(gth, 'prss_prf', 'shake')
    with pytest.raises(NotImplementedError, match='exceeds the field order'):
        gth.np_pseudorandom_share(F, 3, 0, {(0, 1): gth.PRF(b'k' * 16, 1 << 61)}, b'u', 3)
    with pytest.raises(ValueError):
        CpuFieldContext(p).prss_combine([bytes(24)], 1, 8, [1], 3, mask_bits=61)
