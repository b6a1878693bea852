"""TEST INFRASTRUCTURE ONLY: the driver of the contract tests of the two PRSS combination entry points of include/ffgpu.h --
ffgpu_prss_combine (k_prss: caller-supplied streams, the SHAKE parity mode) and ffgpu_prss_chacha (k_prss_chacha: the
production mode) -- at their per-call limits, at every draw and mask width, on crafted draws, with accumulate != 0 and at the
edges of their launch geometry.

One case = one call (an accumulate split: two calls in a row) on views into ONE backing tensor
guard | stream 0 | guard | stream 1 | ... | guard | out | guard, guards of 0xA5.  The streams start at odd byte offsets; `out`
starts on a 16-byte boundary or one element past it, and is prefilled.  After every call the whole tensor is compared with an
image built from the reference, and four things are told apart (ContractViolation.kinds): 'guard' -- a byte outside every
operand changed; 'input' -- a stream byte changed; 'canonical' -- an element of `out` is not below the order; 'out' -- a wrong
value, or a refused call that wrote `out`.

Expected values never come from the library.  A draw is int.from_bytes(chunk, 'little') % order, or & (2^mask_bits - 1) for
a mask; the combination is sum_s sum_j draw * w[s * d + j] with po.add / po.mul of oracle/pyoracle.  (GF(2^n): x -> w x is
GF(2)-linear, so the products w 2^i come from po.mul once per weight and a product is the XOR of the rows of the set bits of
x, a byte at a time.)  For ffgpu_prss_chacha the keystream is po.chacha_block at the counters of po.prss_chacha_layout; it
does not depend on the field and is kept across the fields of a run.

Not covered: a block counter of ffgpu_prss_chacha that crosses 2^32 ((tile * d + j) * tb + b: more than 10^8 elements, whose
keystream Python would have to restate) -- the high counter word stays unmeasured.

Nothing here imports the GPU at module level: tests/test_prss_contract_host.py drives the same code against
tests/cpuctx.CpuFieldContext and against deliberately wrong contexts."""
import ctypes
import functools
import random
import zlib

import numpy as np

import ew_contract as ew
from ew_contract import ContractViolation, GUARD_BYTE, bytes_to_ints, ints_to_bytes
from fieldutil import edge_values
from oracle import pyoracle as po
from oracle.coracle import elem_bytes

OK, EINVAL, ENOTSUP = 0, 1, 2           # include/ffgpu.h: FFGPU_OK, FFGPU_EINVAL, FFGPU_ENOTSUP

# ---- the limits and the launch geometry, restated (each constant with the place it lives) -------------------------------
BLOCK = 256                             # mpyc_amd/csrc/kernels.hpp: enum { BLOCK = 256 }
MAXS, MAXW = 48, 96                     # kernels.hpp: enum { PRSS_MAXW = 96, PRSS_MAXS = 48 }; thresha._prss_device chunks by them
CC_MAXS, CC_MAXW = 32, 64               # kernels.hpp: enum { PRSS_CC_MAXS = 32, PRSS_CC_MAXW = 64, ... }
CC_MAXDPT, CC_MAXTB = 8, 3              # ... PRSS_CC_MAXDPT = 8, PRSS_CC_MAXTB = 3 }
MAX_L, MAX_MASK = 64, 192               # api.hip: l <= 64 && mask_bits <= 192
CC_ROUNDS = (20, 12, 8)

GUARD = 1024                            # bytes of guard between the operands (>= 42 elements of any field)
PREFILL = 0x3C                          # what `out` holds before a call that does not accumulate
MONT192 = (2**135 + 4823, False)        # a 24-byte prime of no special shape: the second policy with 24-byte words
# one prime per word width (4, 8, 16 -- stored in 12 and in 16 bytes --, 24), GF(2^8) (packed) and GF(2^64)
GEOMETRY_FIELDS = [(2**31 - 1, False), (2**61 - 1, False), (2**96 - 17, False), (2**128 - 173, False), (2**136 - 113, False),
                   (0x11b, True), (0x1000000000000001b, True)]
GEOMETRY_SIZES = (1, 255, 256, 257, 511, 513)
MASK_WIDTHS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 94, 127, 128, 129)       # and bits - 2, bits - 1
SPLITS = {MAXS: (1, 24, 47), CC_MAXS: (1, 16, 31)}
CRAFTED_WEIGHTS = ('0', '1', 'q-1', 'rnd')


def contract_fields():
    return ew.contract_fields() + [MONT192]


def limb_bytes(eb):
    """LB of prss_draw: sizeof(F::word), fields.hpp -- GF(2^n <= 8) draws a byte, 12-byte elements compute in 16-byte words"""
    return {1: 1, 4: 4, 8: 8, 12: 16, 16: 16, 24: 24}[eb]


def cc_layout(l):
    """prss_cc_layout, kernels.hpp: LW = ceil(l / 4) words per draw, a tile of TB blocks holds DPT = min(8, 16 TB / LW) draws,
    TB in 1..3 taken where a block carries the most draws (the smallest such TB)"""
    lw = (l + 3) // 4
    tb, dpt = 1, min(CC_MAXDPT, 16 // lw)
    for t in range(2, CC_MAXTB + 1):
        dp = min(CC_MAXDPT, 16 * t // lw)
        if dp * tb > dpt * t:
            tb, dpt = t, dp
    return tb, dpt


def cc_tile_shapes():
    """(tb, dpt) -> the first l that has it, for every pair l = 1..64 produces"""
    shapes = {}
    for l in range(1, MAX_L + 1):
        shapes.setdefault(cc_layout(l), l)
    return shapes


def cc_geometry_sizes(dpt):
    """one tile short of a full workgroup of tiles, exactly one, one element into the second, and two workgroups plus a tile
    that the end of the array cuts after dpt - 1 draws"""
    return (dpt * BLOCK - 1, dpt * BLOCK, dpt * BLOCK + 1, 2 * dpt * BLOCK + dpt - 1)


def chunk_sizes(nkeys, d, chacha):
    """the launches thresha._prss_device makes for nkeys subset keys of d draws each"""
    per = max(1, min(CC_MAXS, CC_MAXW // d)) if chacha else max(1, min(MAXS, MAXW // d))
    return [min(per, nkeys - k0) for k0 in range(0, nkeys, per)]


# ---- references ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=512)
def _gf2_rows(modulus, w):
    """per byte position k the 256 products w * (b << 8 k), from the products w * 2^i of po.mul"""
    F = po.Field(modulus, True)
    tabs = []
    for k in range((F.n + 7) // 8):
        basis = [po.mul(F, w, 1 << (8 * k + i)) if 8 * k + i < F.n else 0 for i in range(8)]
        t = [0] * 256
        for b in range(1, 256):
            low = b & -b
            t[b] = t[b ^ low] ^ basis[low.bit_length() - 1]
        tabs.append(t)
    return tabs


def mul_by(F, w):
    """x -> x * w for canonical x"""
    if not F.binary:
        return lambda x: po.mul(F, x, w)
    tabs = _gf2_rows(F.modulus, w)

    def mul(x):
        r, k = 0, 0
        while x:
            r ^= tabs[k][x & 255]
            x >>= 8
            k += 1
        return r
    return mul


def draw_values(raw, count, l, order, mask_bits):
    """the first `count` l-byte draws of a stream"""
    raw = bytes(raw)
    if mask_bits:
        m = (1 << mask_bits) - 1
        return [int.from_bytes(raw[i * l:(i + 1) * l], 'little') & m for i in range(count)]
    return [int.from_bytes(raw[i * l:(i + 1) * l], 'little') % order for i in range(count)]


def _combine(F, draws, d, weights, n, preload):
    """draws: per stream the n * d values; out[h] = preload[h] + sum_s sum_j draws[s][h d + j] w[s d + j]"""
    acc = list(preload) if preload is not None else [0] * n
    for s, x in enumerate(draws):
        for j in range(d):
            mw = mul_by(F, weights[s * d + j])
            for h in range(n):
                acc[h] = po.add(F, acc[h], mw(x[h * d + j]))
    return acc


def combine_ref(F, streams, d, l, mask_bits, weights, n, preload=None):
    return _combine(F, [draw_values(s, n * d, l, F.order, mask_bits) for s in streams], d, weights, n, preload)


@functools.lru_cache(maxsize=None)
def cc_raw_draws(k40, l, d, n, rounds):
    """the n * d draws (h, j) -> index h d + j of one stream as l-byte integers, not yet reduced: they depend on the key and
    the layout only, so every field of a run shares them"""
    tb, dpt = po.prss_chacha_layout(l)
    lw = (l + 3) // 4
    out = []
    for tile in range(-(-n // dpt)):
        ks = [b''.join(po.chacha_block(k40[:32], (tile * d + j) * tb + b, k40[32:], rounds) for b in range(tb)) for j in range(d)]
        for slot in range(min(dpt, n - tile * dpt)):
            out += [int.from_bytes(ks[j][4 * slot * lw:4 * slot * lw + l], 'little') for j in range(d)]
    return tuple(out)


def chacha_ref(F, keys40, d, l, mask_bits, rounds, weights, n, preload=None):
    m = (1 << mask_bits) - 1
    draws = [[v & m if mask_bits else v % F.order for v in cc_raw_draws(bytes(k), l, d, n, rounds)] for k in keys40]
    return _combine(F, draws, d, weights, n, preload)


def crafted_values(p, LB, l):
    """(name, value) of the l-byte draws at which a wide reduction can go wrong, as far as they fit l bytes"""
    W = 8 * l
    top = ((1 << W) - 1) // p * p
    limbs = -(-l // LB)
    vals = [('0', 0), ('1', 1), ('p-1', p - 1), ('p', p), ('p+1', p + 1), ('2p-1', 2 * p - 1), ('2^(8l)-1', (1 << W) - 1),
            ('top multiple of p', top), ('top multiple - 1', top - 1), ('top multiple + 1', top + 1),
            ('2^(8LB)-1', (1 << 8 * LB) - 1), ('2^(8LB)', 1 << 8 * LB), ('(p-1) 2^(8LB)', (p - 1) << 8 * LB),
            ('every limb p-1', sum((p - 1) << (8 * LB * i) for i in range(limbs)) & ((1 << W) - 1)),
            ('every limb 2^(8LB)-1', sum(((1 << 8 * LB) - 1) << (8 * LB * i) for i in range(limbs)) & ((1 << W) - 1))]
    return [(name, v) for name, v in vals if 0 <= v < (1 << W)]


def crafted_widths(p, LB):
    bl = ((p - 1).bit_length() + 7) // 8
    return sorted({l for l in (LB, LB + 1, 2 * LB - 1, 2 * LB, 2 * LB + 1, bl + 16, MAX_L) if 1 <= l <= MAX_L})


def mask_widths(F, bits):
    if F.binary:
        return list(range(1, F.n + 1))
    return sorted(mb for mb in set(MASK_WIDTHS) | {bits - 2, bits - 1} if 1 <= mb < bits)


def _align16(x):
    return -(-x // 16) * 16


def _hex(raw):
    return bytes(raw)[::-1].hex()


def stream_key(s):
    return bytes((7 * i + 3 * s + 1) % 256 for i in range(40))


# ---- adapters --------------------------------------------------------------------------------------------------------------
class CpuAdapter:
    """an engine-style context on CPU tensors (tests/cpuctx.CpuFieldContext and the wrong contexts of the host test) behind the
    signature of the C ABI: the argument checks of api.hip and launch.hpp in their order, `out` a view of the caller's bytes"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.eb, self.device = torch, ctx, ctx.elem_bytes, torch.device('cpu')
        self.launches = 0

    def _view(self, buf, off, n):
        from mpyc_amd import engine
        t = buf[off:off + n * self.eb].view(engine._torch_dtype(self.eb))
        limbs = engine.limbs_of(self.eb)
        return engine.DevArray(self.ctx, t.reshape(n, limbs) if limbs else t, n)

    def _status(self, ks, d, l, mask_bits, n, pointers, maxs, maxw):
        if ks < 1 or d < 1 or not 1 <= l <= MAX_L or not 0 <= mask_bits <= MAX_MASK:
            return EINVAL
        if (1 << mask_bits) > self.ctx.order:
            return EINVAL
        if n == 0:
            return OK
        if any(p is None for p in pointers):
            return EINVAL
        if ks > maxs or ks * d > maxw:
            return ENOTSUP
        return None

    def combine(self, buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n):
        rc = self._status(ks, d, l, mask_bits, n, [streams, weights, out] + list(streams or ()), MAXS, MAXW)
        if rc is not None:
            return rc
        self.launches += 1
        self.ctx.prss_combine([buf[o:o + n * d * l] for o in streams], d, l, list(weights), n, mask_bits=mask_bits,
                              out=self._view(buf, out, n), accumulate=bool(accumulate))
        return OK

    def chacha(self, buf, keys40, ks, d, l, mask_bits, rounds, weights, accumulate, out, n):
        if rounds not in CC_ROUNDS:
            return EINVAL
        rc = self._status(ks, d, l, mask_bits, n, [keys40, weights, out], CC_MAXS, CC_MAXW)
        if rc is not None:
            return rc
        self.launches += 1
        self.ctx.prss_chacha([bytes(k) for k in keys40], d, l, list(weights), n, mask_bits=mask_bits, rounds=rounds,
                             out=self._view(buf, out, n), accumulate=bool(accumulate))
        return OK

    def sync(self):
        pass


class GpuAdapter:
    """the C ABI itself on base pointer + byte offset"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.eb, self.device = torch, ctx, ctx.elem_bytes, ctx.torch_device

    @staticmethod
    def _p(buf, off):
        return None if off is None else buf.data_ptr() + off

    def combine(self, buf, streams, ks, d, l, mask_bits, weights, accumulate, out, n):
        c = self.ctx
        ptrs = (ctypes.c_void_p * max(1, len(streams)))(*[self._p(buf, o) for o in streams])
        return c._L.ffgpu_prss_combine(c._h, ptrs, ks, d, l, mask_bits, c._scalars(weights), int(accumulate), self._p(buf, out),
                                       n, c._stream())

    def chacha(self, buf, keys40, ks, d, l, mask_bits, rounds, weights, accumulate, out, n):
        c = self.ctx
        kb = ctypes.create_string_buffer(b''.join(bytes(k) for k in keys40), 40 * max(1, len(keys40)))
        return c._L.ffgpu_prss_chacha(c._h, ctypes.cast(kb, ctypes.POINTER(ctypes.c_uint8)), ks, d, l, mask_bits, rounds,
                                      c._scalars(weights), int(accumulate), self._p(buf, out), n, c._stream())

    def sync(self):
        self.torch.cuda.synchronize()


# ---- the driver ------------------------------------------------------------------------------------------------------------
class Driver:
    def __init__(self, adapter, modulus, binary):
        self.ad, self.F = adapter, po.Field(modulus, binary)
        self.modulus, self.binary = int(modulus), bool(binary)
        self.eb = elem_bytes(modulus, binary)
        assert adapter.eb == self.eb
        self.q = self.F.order
        self.bits = self.modulus.bit_length()
        self.LB = limb_bytes(self.eb)
        self.mask = self.F.n if binary else 0                       # the mask of a draw over the whole field: none for a prime
        # the width a real PRF draws with (thresha.PRF.byte_length): GF(2^n) ceil(n / 8), primes byte_length + 16
        self.l0 = (self.F.n + 7) // 8 if binary else ((self.q - 1).bit_length() + 7) // 8 + 16
        self.seed = self.modulus % 100003
        self.rng = random.Random(self.seed + 23)
        self.w4 = [self.rng.randrange(self.q), 1, self.q - 1, self.rng.randrange(self.q)]
        self.cases = 0              # cases compared with the reference
        self.calls = 0              # calls issued
        self.seen = set()

    # ---- data ----
    def _bytes(self, count, salt):
        return np.random.default_rng([self.seed, zlib.crc32(repr(salt).encode())]).integers(0, 256, size=count, dtype=np.uint8)

    def _streams(self, ks, nbytes, salt, kind='random'):
        if kind == 'ramp':
            return [((np.arange(nbytes) + 37 * s + salt) & 255).astype(np.uint8) for s in range(ks)]
        return [self._bytes(nbytes, (salt, s)) for s in range(ks)]

    def _weights(self, count):
        return [self.rng.randrange(self.q) for _ in range(count)]

    # ---- one case ----
    def _run(self, entry, inputs, d, l, mask_bits, weights, n, expected=None, accumulate=0, preload=None, one_in=False,
             status=OK, steps=None, rounds=8, null_stream=None, label=''):
        """entry 'combine': inputs are the streams (uint8 arrays of at least n d l bytes); 'chacha': the 40-byte stream keys.
        steps: (lo, hi, accumulate, expected) per call, over inputs[lo:hi]; by default the one call over all of them.
        status != OK: that status from every call, and not a byte changes.  preload: the elements `out` holds before."""
        eb, ks = self.eb, len(inputs)
        steps = steps or [(0, ks, accumulate, expected)]
        off, cur = [], 0
        if entry == 'combine':
            for s, raw in enumerate(inputs):
                off.append(_align16(cur + GUARD) + 1 + 2 * (s % 7))            # odd byte offsets
                cur = off[-1] + raw.size
        off_o = _align16(cur + GUARD) + (eb if one_in else 0)
        total = _align16(off_o + n * eb + GUARD)
        img = np.full(total, GUARD_BYTE, dtype=np.uint8)
        for o, raw in zip(off, inputs):
            img[o:o + raw.size] = raw
        img[off_o:off_o + n * eb] = ints_to_bytes(preload, eb) if preload is not None else PREFILL
        buf = self.ad.torch.from_numpy(img.copy()).to(self.ad.device)
        regions = [('stream %d' % s, o, o + raw.size, 'input') for s, (o, raw) in enumerate(zip(off, inputs))]
        regions.append(('out', off_o, off_o + n * eb, 'out'))
        want = img
        for step, (lo, hi, acc, exp) in enumerate(steps):
            where = (entry, label, 'ks=%d d=%d l=%d mask=%d n=%d' % (hi - lo, d, l, mask_bits, n),
                     'one-in' if one_in else 'aligned', 'call %d' % (step + 1))
            w = None if weights is None else weights[lo * d:hi * d]
            if entry == 'combine':
                ptrs = [None if s == null_stream else o for s, o in enumerate(off)][lo:hi]
                rc = self.ad.combine(buf, ptrs, hi - lo, d, l, mask_bits, w, acc, off_o, n)
            else:
                rc = self.ad.chacha(buf, inputs[lo:hi], hi - lo, d, l, mask_bits, rounds, w, acc, off_o, n)
            self.ad.sync()
            self.calls += 1
            assert rc == status, (where, 'status %d, want %d' % (rc, status))
            got = buf.cpu().numpy()
            if status == OK and n:
                want = want.copy()
                want[off_o:off_o + n * eb] = ints_to_bytes(exp, eb)
            self._check(got, want, regions, off_o, n if status == OK else 0, where)
        self.cases += 1
        del buf

    def _check(self, got, want, regions, off_o, n, where):
        """the guards, the streams, that the n results are canonical, the values -- in that order"""
        eb = self.eb
        kinds, notes = set(), []
        covered = np.zeros(got.size, dtype=bool)
        for _, lo, hi, _ in regions:
            covered[lo:hi] = True
        if not np.array_equal(got, want):
            diff = np.nonzero((got != want) & ~covered)[0]
            if diff.size:
                kinds.add('guard')
                notes.append('guard byte %d changed (out at %d, %d bytes)' % (int(diff[0]), off_o, regions[-1][2] - off_o))
            for name, lo, hi, kind in regions:
                if kind == 'input' and not np.array_equal(got[lo:hi], want[lo:hi]):
                    kinds.add('input')
                    notes.append('%s changed at byte %d' % (name, int(np.nonzero(got[lo:hi] != want[lo:hi])[0][0])))
        if n and self.q < 1 << (8 * eb):
            vals = bytes_to_ints(got[off_o:off_o + n * eb], eb)
            bad = next((h for h, v in enumerate(vals) if v >= self.q), None)
            if bad is not None:
                kinds.add('canonical')
                notes.append('out[%d] = %x is not below the order' % (bad, vals[bad]))
        lo, hi = regions[-1][1], regions[-1][2]
        diff = np.nonzero(got[lo:hi] != want[lo:hi])[0]
        if diff.size:
            h = int(diff[0]) // eb
            kinds.add('out')
            notes.append('out differs at element %d of %d: got %s, want %s' % (
                h, (hi - lo) // eb, _hex(got[lo + h * eb:lo + (h + 1) * eb]), _hex(want[lo + h * eb:lo + (h + 1) * eb])))
        if kinds:
            raise ContractViolation(kinds, '%r: %s' % (where, '; '.join(notes)))

    def _both(self, entry, inputs, d, l, mask_bits, weights, n, **kw):
        for one_in in (False, True):
            self._run(entry, inputs, d, l, mask_bits, weights, n, one_in=one_in, **kw)

    def _ref(self, entry, inputs, d, l, mask_bits, weights, n, preload=None, rounds=8):
        if entry == 'combine':
            return combine_ref(self.F, inputs, d, l, mask_bits, weights, n, preload)
        return chacha_ref(self.F, inputs, d, l, mask_bits, rounds, weights, n, preload)

    # ---- ffgpu_prss_combine ----
    def run_width_sweep(self, widths=range(1, MAX_L + 1), n=2 * BLOCK + 3):
        """every l: every partial top limb, the plain reduction of l <= LB, 1 to 16 Horner steps; ks = 2, d = 2, a byte ramp
        and random bytes; no mask over a prime field, the mask of the degree over GF(2^n)"""
        for l in widths:
            for kind in ('ramp', 'random'):
                streams = self._streams(2, n * 2 * l, l, kind)
                exp = combine_ref(self.F, streams, 2, l, self.mask, self.w4, n)
                self._both('combine', streams, 2, l, self.mask, self.w4, n, expected=exp, label='width ' + kind)
                self.seen.add(('width', l, kind))

    def run_crafted(self, widths=None):
        """prime fields: one stream whose draws are crafted_values, under the weights 0, 1, q - 1 and a random one, as the
        only draw of an element (d = 1) and as the last of three"""
        assert not self.binary
        p = self.q
        for l in widths or crafted_widths(p, self.LB):
            vals = crafted_values(p, self.LB, l)
            n = len(vals)
            for d in (1, 3):
                raw = self._bytes(n * d * l, ('crafted', l)).reshape(n, d * l)
                for h, (_, v) in enumerate(vals):
                    raw[h, (d - 1) * l:] = np.frombuffer(v.to_bytes(l, 'little'), dtype=np.uint8)
                streams = [raw.reshape(-1)]
                for name, w in zip(CRAFTED_WEIGHTS, (0, 1, p - 1, self.w4[0])):
                    weights = self._weights(d - 1) + [w]
                    exp = combine_ref(self.F, streams, d, l, 0, weights, n)
                    self._both('combine', streams, d, l, 0, weights, n, expected=exp,
                               label='crafted w=%s: %s' % (name, ', '.join(nm for nm, _ in vals)))
                    self.seen.add(('crafted', l, d, name))

    def run_mask_sweep(self, widths=None, n=64):
        """every mask width at l = ceil(mask_bits / 8) and 16 bytes more; in the first half of the elements every bit above
        the mask is set, the second half is random"""
        for mb in widths or mask_widths(self.F, self.bits):
            for l in ((mb + 7) // 8, (mb + 7) // 8 + 16):
                above = np.frombuffer((((1 << 8 * l) - 1) ^ ((1 << mb) - 1)).to_bytes(l, 'little'), dtype=np.uint8)
                streams = self._streams(2, n * 2 * l, ('mask', mb, l))
                for raw in streams:
                    raw.reshape(n * 2, l)[:n] |= above
                exp = combine_ref(self.F, streams, 2, l, mb, self.w4, n)
                self._both('combine', streams, 2, l, mb, self.w4, n, expected=exp, label='mask')
                self.seen.add(('mask', mb, l))

    def _refused(self, entry):
        """(label, ks, d, l, mask_bits, rounds, status, null stream) of the calls that must be refused"""
        maxs, maxw = (MAXS, MAXW) if entry == 'combine' else (CC_MAXS, CC_MAXW)
        l, mask = (self.l0, self.mask) if entry == 'combine' else (24, self.mask)
        wide = self.bits if not self.binary else self.F.n + 1           # the first mask with 2^mask_bits > order
        over = (33, 3) if entry == 'combine' else (17, 4)               # ks within its limit, ks * d past it
        calls = [('ks=%d' % (maxs + 1), maxs + 1, 1, l, mask, 8, ENOTSUP, None),
                 ('ks*d=%d' % (maxw + 1), 1, maxw + 1, l, mask, 8, ENOTSUP, None),
                 ('ks=%d d=%d' % over, over[0], over[1], l, mask, 8, ENOTSUP, None),
                 ('l=65', 2, 2, MAX_L + 1, mask, 8, EINVAL, None),
                 ('2^mask_bits > order', 2, 2, (wide + 7) // 8, wide, 8, EINVAL, None)]
        if entry == 'combine':
            calls += [('l=0', 2, 2, 0, mask, 8, EINVAL, None), ('d=0', 2, 0, l, mask, 8, EINVAL, None),
                      ('null stream', 3, 1, l, mask, 8, EINVAL, 1)]
        else:
            calls += [('rounds=10', 2, 2, l, mask, 10, EINVAL, None)]
        return calls

    def _inputs(self, entry, ks, nbytes, salt):
        return self._streams(ks, nbytes, salt) if entry == 'combine' else [stream_key(s) for s in range(ks)]

    def run_limits(self, entry='combine', n=5):
        """the largest calls run and match; one past each limit, and every bad argument, is refused with the documented status
        and without a byte written; n = 0 is FFGPU_OK and writes nothing"""
        ran = ((MAXS, 1), (MAXS, 2), (1, MAXW), (32, 3)) if entry == 'combine' else ((CC_MAXS, 1), (CC_MAXS, 2), (1, CC_MAXW), (16, 4))
        l, mask = (self.l0, self.mask) if entry == 'combine' else (24, self.mask)
        for ks, d in ran:
            inputs = self._inputs(entry, ks, n * d * l, ('limits', ks, d))
            weights = self._weights(ks * d)
            exp = self._ref(entry, inputs, d, l, mask, weights, n)
            self._both(entry, inputs, d, l, mask, weights, n, expected=exp, label='limits')
            self.seen.add((entry, 'runs', ks, d))
        for label, ks, d, l_, mb, rounds, status, null in self._refused(entry):
            inputs = self._inputs(entry, ks, n * max(d, 1) * max(l_, 1), ('refused', label))
            self._run(entry, inputs, d, l_, mb, self._weights(ks * d), n, status=status, rounds=rounds, null_stream=null,
                      label='refused ' + label)
            self.seen.add((entry, 'refused', label, status))
        if entry == 'combine':
            self._run(entry, self._inputs(entry, 2, 64, 'empty'), 2, l, mask, self._weights(4), 0, label='n=0')
            self.seen.add((entry, 'n=0'))

    def run_accumulate(self, entry='combine', n=BLOCK + 3):
        """accumulate = 1 on a preload of q - 1 everywhere and of a periodic edge pattern; the streams [0, a) and then,
        accumulating, [a, ks) against the one call over all ks"""
        F, ks = self.F, MAXS if entry == 'combine' else CC_MAXS
        l, mask = (self.l0, self.mask) if entry == 'combine' else (24, self.mask)
        inputs = self._inputs(entry, ks, n * l, 'accumulate')
        weights = self._weights(ks)
        full = self._ref(entry, inputs, 1, l, mask, weights, n)
        edges = edge_values(F)
        for name, pre in (('q-1', [self.q - 1] * n), ('edges', [edges[h % len(edges)] for h in range(n)])):
            exp = [po.add(F, a, b) for a, b in zip(pre, full)]
            self._both(entry, inputs, 1, l, mask, weights, n, expected=exp, accumulate=1, preload=pre, label='preload ' + name)
            self.seen.add((entry, 'preload', name))
        for a in SPLITS[ks]:
            part = self._ref(entry, inputs[:a], 1, l, mask, weights[:a], n)
            self._both(entry, inputs, 1, l, mask, weights, n, steps=[(0, a, 0, part), (a, ks, 1, full)], label='split at %d' % a)
            self.seen.add((entry, 'split', a))

    def run_geometry(self, sizes=GEOMETRY_SIZES, label='default grid'):
        """ks = 2, d = 2, l = 24 at the sizes around one and two workgroups; one reference, the sizes are prefixes of it"""
        l, top = 24, max(sizes)
        streams = self._streams(2, top * 2 * l, 'geometry')
        exp = combine_ref(self.F, streams, 2, l, self.mask, self.w4, top)
        for n in sizes:
            self._both('combine', [s[:n * 2 * l] for s in streams], 2, l, self.mask, self.w4, n, expected=exp[:n], label=label)
            self.seen.add(('geometry', label, n))

    def run_capped(self, G):
        """on a context whose grid is capped at G threads: n = 2 G + 1, every thread of k_prss loops twice and one a third time"""
        self.run_geometry(sizes=(2 * G + 1,), label='grid of %d threads' % G)

    # ---- ffgpu_prss_chacha ----
    def run_cc_geometry(self, shapes=None):
        """per tile shape (tb, dpt) one l; n around one workgroup of tiles and two workgroups plus a cut tile; d = 1 and 3; two
        streams, ChaCha8 (the rounds are a loop count: tests/test_prss_chacha.py pins 20, 12 and 8)"""
        every = shapes is None
        shapes = cc_tile_shapes() if every else shapes
        keys = [stream_key(s) for s in range(2)]
        for (tb, dpt), l in shapes.items():
            assert cc_layout(l) == (tb, dpt)
            sizes = cc_geometry_sizes(dpt)
            for d in (1, 3):
                weights = (self.w4 + self.w4[::-1])[:2 * d]
                exp = chacha_ref(self.F, keys, d, l, self.mask, 8, weights, max(sizes))
                for n in sizes:
                    self._both('chacha', keys, d, l, self.mask, weights, n, expected=exp[:n], label='tile %dx%d' % (tb, dpt))
                    self.seen.add(('cc-geometry', tb, dpt, d, n))
        if every:
            assert {k[1:3] for k in self.seen if k[0] == 'cc-geometry'} == {cc_layout(l) for l in range(1, MAX_L + 1)}
