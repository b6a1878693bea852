"""TEST INFRASTRUCTURE ONLY: the driver of the memory contract of share generation, the fused gate and Lagrange recombination
(include/ffgpu.h: inputs are never written; nothing outside the n elements of each output row is written, not the padding
between n and the row stride either; with w = 1 the output of a recombination may be exactly one of its rows).

One case = one entry point, one parameter set, one size, one stride class.  All memory of a case is ONE backing byte tensor
guard | input | guard | input ... | guard | output block | guard  (guards: at least 64 elements of 0xA5).  A matrix operand
(coefficients, shares, a w > 1 output, the operand and output blocks of a batched gate) occupies rows * stride elements; the
elements between n and the stride of every row are padding, filled with the guard byte.  The call goes through an ADAPTER
(entry point, byte offsets into the tensor, strides, parameters): GpuAdapter issues the raw C ABI with base pointer + offset,
PyAdapter works on the bytes with Python integers (tests/test_share_contract_host.py drives it and wrong variants of it).
After the call the whole tensor is compared, byte for byte, with an image built on the host; a difference is of kind 'out'
(an output row), 'input' (a row that is read), 'pad' (inside a matrix operand, outside its rows) or 'guard'.

Expected values never come from the code under test: fields of up to 128 bits take oracle/fforacle.c (CField.split,
CField.recombine, rng_coeffs, the element-wise MUL), 24-byte fields Python integers and the restatement of the generator
layout below (rng_coeffs_ints, checked against the C oracle on the narrower fields by the host test).

Nothing here imports the GPU at module level."""
import ctypes
import hashlib

import numpy as np

from ew_contract import (GUARD_BYTE, GUARD_ELEMS, LARGE_SIZES, SMALL_SIZES, ContractViolation, bytes_to_ints, contract_fields,
                         ints_to_bytes, make_ref)
from oracle import pyoracle as po

OK, EINVAL, ENOTSUP = 0, 1, 2
FULL_SIZES = (1, 17, 65, 129, 1025)
TM = ((0, 1), (0, 3), (1, 3), (2, 5), (3, 7), (4, 9), (5, 11))          # (5, 11): beyond MAXT, k_split_any
TM_REDUCED = ((1, 3), (2, 5))
KW = ((1, 1), (2, 1), (3, 1), (4, 4), (5, 1), (9, 1), (9, 8), (3, 9), (3, 11), (10, 1), (10, 2), (64, 1))
KW_REDUCED = ((3, 1), (4, 4), (3, 9), (10, 2))
KW_ALIAS = (3, 9, 10)                     # w = 1, out = one of the rows: k_recombine, its widest instantiation, k_recombine_any
KW_LARGE = ((3, 1), (4, 4), (9, 8), (10, 1))
GATE_KA = ('1p', '1', '3', '5', '7')      # '1p': one row with lambda = 1 (the plain load)
GATE_KB = ('0', '1p', '3')                # '0': squaring
GATE_T = (1, 2, 3)
GATE_REDUCED = (('3', '0', 1), ('1p', '3', 2))
GATE_LARGE = (('3', '0', 1), ('7', '3', 3))
BATCH_COMBOS = tuple((a, b, o) for a in (0, 1) for b in (0, 1) for o in (0, 1))     # which batch strides get + 1
BATCH_GATES = (('3', '0', 1), ('1', '3', 2))
KEY = bytes((7 * i + 3) & 0xff for i in range(32))
NONCE = 0x5eed0123


def pack_unit(eb):
    """elements in the smallest row stride that keeps every row on a 16-byte boundary (Launchers::stride_ok; 12-byte rows need
    dword alignment only, so every stride passes there)"""
    return 16 // eb if eb <= 8 else 2 if eb == 24 else 1


def epv_of(eb):
    """elements per pack of the streaming kernels (one lane's access)"""
    return 16 // eb if eb <= 8 else 1


def pitched(eb, n):
    """the row stride engine.FieldContext.empty_matrix chooses (restated; the GPU test compares the two)"""
    per = 64 if eb == 12 else 32 if eb == 24 else 256 // eb
    stride = max(per, (n + per - 1) // per * per)
    if (stride * eb) % 16384 == 0:
        stride += 17 * per
    return stride


def stride_classes(eb):
    """every class has its bases on 16-byte boundaries; 'one-in' moves every base one element in.  12- and 16-byte elements:
    every stride is whole packs, 'pack' is 'tight'; 16-byte elements: one element in is still aligned"""
    sc = ['tight', 'pack', 'pack+1', 'pitched', 'one-in']
    if eb in (12, 16):
        sc.remove('pack')
    if eb == 16:
        sc.remove('one-in')
    return tuple(sc)


def stride_of(eb, n, sc):
    u = pack_unit(eb)
    p = -(-n // u) * u
    return {'tight': n, 'pack': p, 'pack+1': p + 1, 'pitched': pitched(eb, n)}.get(sc, p)


# ---- Python-integer field arithmetic and the generator layout (24-byte reference, PyAdapter) ------------------------------
class IntField:
    def __init__(self, modulus, binary):
        self.modulus, self.binary = int(modulus), bool(binary)
        self.q = 1 << (self.modulus.bit_length() - 1) if binary else self.modulus

    def add(self, a, b):
        return a ^ b if self.binary else (a + b) % self.modulus

    def mul(self, a, b):
        return po.clmod(po.clmul(a, b), self.modulus) if self.binary else a * b % self.modulus

    def share(self, s, c, x):
        """s + c[0] x + c[1] x^2 + ... at the point x (an integer; for GF(2^n) the polynomial with that bit pattern)"""
        if not c:
            return s
        y = c[-1]
        for cj in reversed(c[:-1]):
            y = self.add(self.mul(y, x), cj)
        return self.add(self.mul(y, x), s)

    def dot(self, lam, xs):
        if self.binary:
            r = 0
            for l, x in zip(lam, xs):
                r ^= self.mul(l, x)
            return r
        return sum(l * x for l, x in zip(lam, xs)) % self.modulus


def is_pseudo_mersenne(modulus, binary):
    """fields sampled by rejection (mpyc_amd/csrc/rng.hpp): p = 2^k - c of at least 33 bits with a small c; -> k or 0"""
    if binary:
        return 0
    k = modulus.bit_length()
    if k < 33:
        return 0
    c = (1 << k) - modulus
    if k <= 64:
        if k == 64 and c == 1:
            return 0
        return k if c < (1 << min((k - 1) // 2, 31)) else 0
    return k if c < (1 << 31) else 0


def rng_coeffs_ints(modulus, binary, eb, key, nonce, rounds, t, n, block):
    """the (t, n) coefficients of the device generator as Python integers: the keystream layout and the samplers of
    mpyc_amd/csrc/rng.hpp restated (groups of G packs share B blocks; rejection with a re-draw block per sample for
    2^k - c primes, wide samples mod p for other primes, masks for GF(2^n); rows of t > 4 are streams of their own).
    block(key, counter, nonce_lo, nonce_hi, rounds) -> the 16 words of one ChaCha block"""
    rounds = rounds or 20
    epv = epv_of(eb)
    packed = binary and eb == 1
    wpp = 4 if packed else epv
    k = is_pseudo_mersenne(modulus, binary)
    S = 4 if packed else eb if (binary or k) else 32 if eb >= 16 else 16
    used = eb // 4 if (binary or k) else {4: 3, 8: 4}.get(eb, 8)            # words of a sample that count
    deg = modulus.bit_length() - 1
    npacks = -(-n // epv)
    out = [[0] * n for _ in range(t)]
    M32 = 0xffffffff

    def words(w, at, cnt):
        v = 0
        for i in reversed(range(cnt)):
            v = (v << 32) | w[at + i]
        return v

    for d in range(1 if t <= 4 else t):
        T = t if t <= 4 else 1
        NS = T * wpp
        blocks = lambda g: (g * NS * S + 63) // 64
        G = 1
        for g in (2, 3, 4):
            if blocks(g) * G < blocks(G) * g:
                G = g
        B = blocks(G)
        n0, n1 = nonce & M32, (nonce >> 32) & M32
        if t > 4:
            n1 = (n1 + d + 1) & M32
        ngroups = -(-npacks // G)
        for grp in range(ngroups):
            ks = []
            for b in range(B):
                ks += block(key, grp * B + b, n0, n1, rounds)
            for u in range(G):
                i = u * ngroups + grp
                if i >= npacks:
                    continue
                for sn in range(NS):
                    j, q = divmod(sn, wpp)
                    at = (u * NS + sn) * (S // 4)
                    row = d if t > 4 else j
                    if packed:
                        for b_ in range(4):
                            e = i * epv + q * 4 + b_
                            if e < n:
                                out[row][e] = (ks[at] >> (8 * b_)) & 0xff & ((1 << deg) - 1)
                        continue
                    if binary:
                        v = words(ks, at, used) & ((1 << deg) - 1)
                    elif k:
                        v = words(ks, at, used) & ((1 << k) - 1)
                        if v >= modulus:
                            sidx = grp * G * NS + u * NS + sn
                            blk = block(key, sidx | (1 << 63), n0, n1, rounds)
                            for ci in range(64 // S):
                                v = words(blk, ci * (S // 4), used) & ((1 << k) - 1)
                                if v < modulus:
                                    break
                            else:
                                v -= modulus
                    else:
                        v = words(ks, at, used) % modulus
                    e = i * epv + q
                    if e < n:
                        out[row][e] = v
    return out


def block_from_pyoracle(key, counter, n0, n1, rounds):
    raw = po.chacha_block(key, counter, n0.to_bytes(4, 'little') + n1.to_bytes(4, 'little'), rounds)
    return [int.from_bytes(raw[4 * i:4 * i + 4], 'little') for i in range(16)]


def block_from_coracle(co):
    def block(key, counter, n0, n1, rounds):
        return co.chacha_block(key, (counter & 0xffffffff, counter >> 32, n0, n1), rounds)
    return block


# ---- the reference --------------------------------------------------------------------------------------------------------
class ShareRef:
    """split, recombine, mul and the generator's coefficients on flat uint8 limb images; a matrix is a list of rows"""

    def __init__(self, co, modulus, binary):
        self.co, self.modulus, self.binary = co, int(modulus), bool(binary)
        self.ew = make_ref(co, modulus, binary)
        self.eb, self.q = self.ew.eb, self.ew.q
        self.cf = getattr(self.ew, 'cf', None)                  # None: 24-byte elements, Python integers
        self._block = block_from_coracle(co)
        self._coeffs = {}
        self._results = {}

    MEMO_MIN_BYTES = 1 << 19

    def mul(self, a, b):
        return self.ew.mul(a, b)

    def split(self, s, coef, t, m):
        return self._memo('split', [s] + list(coef), (t, m), lambda: self._split(s, coef, t, m))

    def recombine(self, rows, lam, w):
        return self._memo('recombine', rows, (tuple(lam), w), lambda: self._recombine(rows, lam, w))

    def _memo(self, what, arrays, par, compute):
        """results on large arrays are kept (cases that share their inputs share the reference): read-only"""
        if arrays[0].nbytes < self.MEMO_MIN_BYTES:
            return compute()
        at = (what, par) + tuple(hashlib.blake2b(np.ascontiguousarray(a), digest_size=16).digest() for a in arrays)
        if at not in self._results:
            self._results[at] = compute()
            for r in self._results[at]:
                r.setflags(write=False)
        return self._results[at]

    def _split(self, s, coef, t, m):
        n = s.size // self.eb
        if n == 0:
            return [s.copy() for _ in range(m)]
        if self.cf is not None:
            c = np.concatenate(coef) if t else np.zeros(0, dtype=np.uint8)
            return list(self.cf.split(np.ascontiguousarray(s), c, t, m))
        # (prime fields only: whole rows as NumPy object arrays of Python integers)
        S, C, p = self.ew._obj(s), [self.ew._obj(c) for c in coef], self.modulus
        out = []
        for x in range(1, m + 1):
            y = S * 0
            for cj in reversed(C):
                y = (y + cj) * x % p
            out.append(self.ew._raw((y + S) % p))
        return out

    def _recombine(self, rows, lam, w):
        n, k = rows[0].size // self.eb, len(rows)
        if n == 0:
            return [rows[0].copy() for _ in range(w)]
        if self.cf is not None:
            out = self.cf.recombine(rows, lam, w)
            return [out] if w == 1 else list(out)
        R = [self.ew._obj(r) for r in rows]
        return [self.ew._raw(sum(int(l) * x for l, x in zip(lam[r * k:(r + 1) * k], R)) % self.modulus) for r in range(w)]

    def rng_coeffs(self, key, nonce, rounds, t, n):
        """t rows; computed once per (nonce, rounds, t, n) and shared by the cases (read-only)"""
        at = (key, nonce, rounds or 20, t, n)
        if at not in self._coeffs:
            if n == 0 or t == 0:
                rows = [np.zeros(0, dtype=np.uint8) for _ in range(t)]
            elif self.cf is not None:
                c = self.co.rng_coeffs(self.cf, key, nonce, rounds, t, n)
                rows = list(np.ascontiguousarray(c).view(np.uint8).reshape(t, n * self.eb))
            else:
                rows = [ints_to_bytes(r, self.eb) for r in
                        rng_coeffs_ints(self.modulus, self.binary, self.eb, key, nonce, rounds, t, n, self._block)]
            for r in rows:
                r.setflags(write=False)
            self._coeffs[at] = rows
        return self._coeffs[at]


# ---- adapters -------------------------------------------------------------------------------------------------------------
class GpuAdapter:
    """the raw C ABI on base pointer + byte offset (the engine wrappers cannot express these strides)"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.eb = torch, ctx, ctx.elem_bytes
        self._keep = []

    def upload(self, img):
        t = self.torch.from_numpy(img.copy()).to(self.ctx.torch_device)
        self._keep = self._keep[-2:] + [t]      # stay allocated: the next case's tensor is another address range
        return t

    def snapshot(self, buf):
        return buf.clone()

    def download(self, buf):
        return buf.cpu().numpy()

    def state_init(self, key, nonce, rounds):
        from mpyc_amd import _ffi
        c = self.ctx
        st = self.torch.zeros(int(c._L.ffgpu_rng_state_bytes()), dtype=self.torch.uint8, device=c.torch_device)
        _ffi.check(c._L.ffgpu_rng_state_init(c._h, st.data_ptr(), key, nonce, rounds, c._stream()), 'rng_state_init')
        return st

    def call(self, buf, name, a):
        c = self.ctx
        L, h, st, base = c._L, c._h, c._stream(), buf.data_ptr()

        def P(off):
            return None if off is None else base + off

        def rows(offs):
            if offs is None:
                return None
            return (ctypes.c_void_p * max(1, len(offs)))(*[P(o) for o in offs])

        def lam(v):
            return None if v is None else c._scalars(v)
        if name == 'split':
            return L.ffgpu_split(h, P(a['a']), P(a['coef']), a['cstride'], a['t'], a['m'], P(a['out']), a['ostride'], a['n'], st)
        if name == 'mul_split':
            return L.ffgpu_mul_split(h, P(a['a']), P(a['b']), P(a['coef']), a['cstride'], a['t'], a['m'], P(a['out']),
                                     a['ostride'], a['n'], st)
        if name == 'rng_coeffs':
            return L.ffgpu_rng_coeffs(h, a['key'], a['nonce'], a['rounds'], a['t'], P(a['out']), a['ostride'], a['n'], st)
        if name == 'split_rng':
            return L.ffgpu_split_rng(h, P(a['a']), a['key'], a['nonce'], a['rounds'], a['t'], a['m'], P(a['out']), a['ostride'],
                                     a['n'], st)
        if name == 'mul_split_rng':
            return L.ffgpu_mul_split_rng(h, P(a['a']), P(a['b']), a['key'], a['nonce'], a['rounds'], a['t'], a['m'], P(a['out']),
                                         a['ostride'], a['n'], st)
        if name == 'split_rng_state':
            return L.ffgpu_split_rng_state(h, P(a['a']), P(a['b']), a['state'].data_ptr(), a['t'], a['m'], P(a['out']),
                                           a['ostride'], a['n'], st)
        if name == 'gate_rng':
            return L.ffgpu_gate_rng(h, rows(a['rows_a']), lam(a['lam_a']), a['ka'], rows(a['rows_b']), lam(a['lam_b']), a['kb'],
                                    a['key'], a['nonce'], a['rounds'], None if a.get('state') is None else a['state'].data_ptr(),
                                    a['t'], a['m'], P(a['out']), a['ostride'], a['n'], st)
        if name == 'gate_rng_batch':
            return L.ffgpu_gate_rng_batch(h, rows(a['rows_a']), lam(a['lam_a']), a['ka'], a['ya'], rows(a['rows_b']),
                                          lam(a['lam_b']), a['kb'], a['yb'], a['key'], a['nonce'], a['rounds'], None, 0, a['t'],
                                          a['m'], P(a['out']), a['ostride'], a['yo'], a['n'], a['nbatch'], st)
        if name == 'recombine':
            return L.ffgpu_recombine(h, rows(a['rows']), lam(a['lam']), a['k'], a['w'], P(a['out']), a['ostride'], a['n'], st)
        raise ValueError(name)


class PyAdapter:
    """the same calls on the bytes with Python integers and pyoracle's ChaCha; the small methods are what the wrong adapters
    of the host test override"""

    def __init__(self, modulus, binary, eb):
        self.modulus, self.binary, self.eb = int(modulus), bool(binary), eb
        self.F = IntField(modulus, binary)
        self._coeffs = {}

    def upload(self, img):
        return img.copy()

    def snapshot(self, buf):
        return buf.copy()

    def download(self, buf):
        return buf

    def state_init(self, key, nonce, rounds):
        return {'key': key, 'nonce': nonce, 'rounds': rounds}

    def call(self, buf, name, a):
        return getattr(self, 'do_' + name)(buf, **a)

    # -- what a wrong adapter changes
    def point(self, i):
        return i + 1

    def row(self, base, r, stride, n):
        return base + r * stride * self.eb

    def store(self, buf, off, vals, first):
        buf[off:off + len(vals) * self.eb] = ints_to_bytes(vals, self.eb)

    def batch(self, which, y, stride):
        return y * stride * self.eb

    def chunk_row(self, r0):
        return r0

    def gate_done(self, buf, rows_a, A):
        pass

    # -- helpers
    def load(self, buf, off, n):
        return bytes_to_ints(buf[off:off + n * self.eb], self.eb)

    def coeffs(self, key, nonce, rounds, t, n):
        at = (key, nonce, rounds or 20, t, n)
        if at not in self._coeffs:
            self._coeffs[at] = rng_coeffs_ints(self.modulus, self.binary, self.eb, key, nonce, rounds, t, n, block_from_pyoracle)
        return self._coeffs[at]

    def shares(self, buf, s, c, t, m, out, ostride, n):
        for i in range(m):
            x = self.point(i)
            self.store(buf, self.row(out, i, ostride, n), [self.F.share(s[h], [cj[h] for cj in c], x) for h in range(n)], i == 0)

    @staticmethod
    def split_status(t, m, ostride, n, rounds=20, cstride=None):
        if not (m >= 1 and 0 <= t < m) or rounds not in (0, 8, 12, 20):
            return EINVAL
        if n and ((m > 1 and ostride < n) or (cstride is not None and t > 1 and cstride < n)):
            return EINVAL
        return OK

    # -- entry points
    def do_split(self, buf, a, coef, cstride, t, m, out, ostride, n, b=None):
        rc = self.split_status(t, m, ostride, n, cstride=cstride)
        if rc or n == 0:
            return rc
        s = self.load(buf, a, n)
        if b is not None:
            s = [self.F.mul(x, y) for x, y in zip(s, self.load(buf, b, n))]
        c = [self.load(buf, self.row(coef, j, cstride, n), n) for j in range(t)]
        self.shares(buf, s, c, t, m, out, ostride, n)
        return OK

    do_mul_split = do_split

    def do_rng_coeffs(self, buf, key, nonce, rounds, t, out, ostride, n):
        if t < 1 or rounds not in (0, 8, 12, 20) or (n and t > 1 and ostride < n):
            return EINVAL
        for j, r in enumerate(self.coeffs(key, nonce, rounds, t, n) if n else []):
            self.store(buf, self.row(out, j, ostride, n), r, j == 0)
        return OK

    def do_split_rng(self, buf, a, key, nonce, rounds, t, m, out, ostride, n, b=None):
        rc = self.split_status(t, m, ostride, n, rounds)
        if rc or n == 0:
            return rc
        s = self.load(buf, a, n)
        if b is not None:
            s = [self.F.mul(x, y) for x, y in zip(s, self.load(buf, b, n))]
        self.shares(buf, s, self.coeffs(key, nonce, rounds, t, n) if t else [], t, m, out, ostride, n)
        return OK

    do_mul_split_rng = do_split_rng

    def do_split_rng_state(self, buf, a, b, state, t, m, out, ostride, n):
        rc = self.do_split_rng(buf, a, state['key'], state['nonce'], state['rounds'], t, m, out, ostride, n, b=b)
        if rc == OK and n and t > 0:
            state['nonce'] += 1
        return rc

    def do_gate_rng(self, buf, state=None, **a):
        """with a device-resident state the key, nonce and rounds of the call are not used: the state's are"""
        if state is not None:
            a = dict(a, key=state['key'], nonce=state['nonce'], rounds=state['rounds'])
        rc = self.do_gate_rng_batch(buf, ya=0, yb=0, yo=0, nbatch=1, **a)
        if rc == OK and state is not None and a['n']:
            state['nonce'] += 1
        return rc

    def do_gate_rng_batch(self, buf, rows_a, lam_a, ka, ya, rows_b, lam_b, kb, yb, key, nonce, rounds, t, m, out, ostride, yo, n,
                          nbatch):
        if not 1 <= nbatch <= 255 or (nbatch > 1 and nonce >= 1 << 40):
            return EINVAL
        if not (m >= 1 and 1 <= t < m and ka >= 1 and kb >= 0):
            return EINVAL
        if t > 3 or ka > 7 or kb > 7:
            return ENOTSUP
        if rounds not in (0, 8, 12, 20):
            return EINVAL
        if n == 0:
            return OK
        if m > 1 and ostride < n:
            return EINVAL
        for y in range(nbatch):
            offa, offb = self.batch('a', y, ya), self.batch('b', y, yb)
            A = [self.F.dot(lam_a, xs) for xs in zip(*[self.load(buf, r + offa, n) for r in rows_a])]
            B = A if kb == 0 else [self.F.dot(lam_b, xs) for xs in zip(*[self.load(buf, r + offb, n) for r in rows_b])]
            s = [self.F.mul(x, z) for x, z in zip(A, B)]
            self.shares(buf, s, self.coeffs(key, nonce + (y << 40), rounds, t, n), t, m, out + self.batch('o', y, yo), ostride, n)
            self.gate_done(buf, [r + offa for r in rows_a], A)
        return OK

    def do_recombine(self, buf, rows, lam, k, w, out, ostride, n):
        if k < 1 or w < 1:
            return EINVAL
        if n == 0:
            return OK
        if w > 1 and ostride < n:
            return EINVAL
        if k > 64:
            return ENOTSUP
        X = [self.load(buf, r, n) for r in rows]
        for r0 in range(0, w, 8):                                   # chunks of 8 output rows, as the launcher
            o = self.row(out, self.chunk_row(r0), ostride, n)
            for r in range(r0, min(w, r0 + 8)):
                self.store(buf, self.row(o, r - r0, ostride, n), [self.F.dot(lam[r * k:(r + 1) * k], xs) for xs in zip(*X)],
                           r == 0)
        return OK


# ---- the layout of a case ---------------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, eb):
        self.eb, self.cur, self.regions = eb, 0, []

    def add(self, name, role, nelems, row_elems, n, one_in=False):
        """a block of nelems elements with rows of n elements at the given element offsets; -> its byte offset.  The block
        starts at an offset = 0 (mod 16), or = eb (mod 16) -- one element in; at least GUARD_ELEMS elements of guard before"""
        eb = self.eb
        base = -(-(self.cur + GUARD_ELEMS * eb) // 16) * 16 + (eb if one_in else 0)
        self.cur = base + nelems * eb
        self.regions.append({'name': name, 'role': role, 'base': base, 'bytes': nelems * eb,
                             'rows': [base + r * eb for r in row_elems], 'n': n})
        return base

    def vec(self, name, n, one_in=False):
        return self.add(name, 'input', n, [0], n, one_in)

    def mat(self, name, role, rows, stride, n, one_in=False):
        return self.add(name, role, (rows - 1) * stride + max(stride, n) if rows else 0, [r * stride for r in range(rows)], n,
                        one_in)

    def total(self):
        return -(-(self.cur + GUARD_ELEMS * self.eb) // 16) * 16


class Driver:
    def __init__(self, adapter, ref, seed=1):
        assert adapter.eb == ref.eb
        self.ad, self.ref, self.eb, self.q = adapter, ref, ref.eb, ref.q
        self.rng = np.random.default_rng(seed)
        self.seen = set()          # (entry point, parameters, n, stride class) of every case that was checked
        self.cases = 0             # cases run (the tiers of a matrix overlap: a case that is in two of them runs twice)
        self.steps = 0             # calls compared with the reference
        self._mixed = 0
        self._pool = None

    # ---- data
    POOL = 16384

    def draw(self, n):
        """n uniform canonical elements out of a pool drawn once (converting fresh elements would be most of the time of a
        24-byte case): a window at a random place, for large n windows of 4096 elements strung together"""
        eb, W = self.eb, 4096
        if self._pool is None:
            self._pool = self.ref.ew.random(self.rng, self.POOL)
        if 2 * n <= self.POOL:
            at = int(self.rng.integers(0, self.POOL - n + 1)) * eb
            return self._pool[at:at + n * eb].copy()
        ats = self.rng.integers(0, self.POOL - W + 1, size=-(-n // W))
        return np.concatenate([self._pool[int(at) * eb:(int(at) + W) * eb] for at in ats])[:n * eb]

    def scalar(self, nonzero=True):
        while True:
            v = bytes_to_ints(self.draw(1), self.eb)[0]
            if v or not nonzero:
                return v

    def scalars(self, count):
        """canonical scalars, none zero; one of them 1 and one repeated where there is room (what a Lagrange vector looks
        like over GF(2^n))"""
        v = [self.scalar() for _ in range(count)]
        if count >= 4:
            v[1], v[3] = 1, v[0]
        return v

    def image(self, lay, data=None):
        """the uploaded tensor: guard bytes everywhere, random canonical elements in input rows, random bytes in output rows.
        data: block name -> its rows, for cases that share their inputs (and with them the reference results, which ShareRef
        keeps for large arrays)"""
        img = np.full(lay.total(), GUARD_BYTE, dtype=np.uint8)
        for reg in lay.regions:
            nb = reg['n'] * self.eb
            for i, r in enumerate(() if reg.get('alias') else reg['rows']):
                if data is not None and reg['name'] in data:
                    img[r:r + nb] = data[reg['name']][i]
                else:
                    img[r:r + nb] = self.draw(reg['n']) if reg['role'] == 'input' else \
                        self.rng.integers(0, 256, size=nb, dtype=np.uint8)
        return img

    # ---- one or more calls on one tensor, the state after each compared with its image
    def issue(self, lay, img, calls, where):
        """calls: (entry point, arguments, expected status, fill(want) or None).  fill writes the expected output into the
        image `want`, which carries over to the next call"""
        buf = self.ad.upload(img)
        snaps = []
        for name, args, status, _ in calls:
            rc = self.ad.call(buf, name, args)
            if rc != status:
                raise AssertionError('%r: %s returned status %d, expected %d' % (where, name, rc, status))
            snaps.append(self.ad.snapshot(buf) if len(calls) > 1 else buf)
        want = img
        for step, (name, args, status, fill) in enumerate(calls):
            got = self.ad.download(snaps[step])
            if fill is not None:
                want = want.copy()
                fill(want)
            self.compare(got, want, lay, where + ('call %d: %s' % (step + 1, name),))
            self.steps += 1

    def compare(self, got, want, lay, where):
        if np.array_equal(got, want):
            return
        eb = self.eb
        role = np.zeros(got.size, dtype=np.uint8)               # 0 guard, 1 pad, 2 input, 3 output
        for reg in lay.regions:
            role[reg['base']:reg['base'] + reg['bytes']] = np.maximum(role[reg['base']:reg['base'] + reg['bytes']], 1)
        for code, which in ((2, 'input'), (3, 'out')):
            for reg in lay.regions:
                if reg['role'] == which:
                    for r in reg['rows']:
                        role[r:r + reg['n'] * eb] = code
        bad = np.nonzero(got != want)[0]
        kinds = {('guard', 'pad', 'input', 'out')[c] for c in np.unique(role[bad])}
        at = int(bad[0])
        hit = [(reg['name'], i, r) for reg in lay.regions for i, r in enumerate(reg['rows']) if r <= at < r + reg['n'] * eb]
        lo = at - (at - hit[0][2]) % eb if hit else at - at % eb
        raise ContractViolation(kinds, '%r: %d bytes differ (%s); the first is byte %d, %s: got %s, want %s; blocks %r' % (
            where, bad.size, ', '.join(sorted(kinds)), at,
            'element %d of row %d of %r' % ((at - hit[0][2]) // eb, hit[0][1], hit[0][0]) if hit else 'outside every row',
            bytes(got[lo:lo + eb])[::-1].hex(), bytes(want[lo:lo + eb])[::-1].hex(),
            [(reg['name'], reg['base'], reg['bytes']) for reg in lay.regions]))

    @staticmethod
    def fill_rows(offsets, rows, nb):
        def fill(want):
            for o, r in zip(offsets, rows):
                want[o:o + nb] = r
        return fill

    # ---- share generation -------------------------------------------------------------------------------------------------
    def run_split(self, name, t, m, n, sc, rounds=20, data=None):
        """name: split, mul_split, rng_coeffs, split_rng, mul_split_rng, split_rng_state, split_rng_state+mul"""
        eb, ref = self.eb, self.ref
        one_in = sc == 'one-in'
        # 'coef+1': share rows of whole packs, coefficient rows a whole pack plus one apart (with t = 1 the vector path holds)
        stride = stride_of(eb, n, 'pack' if sc == 'coef+1' else sc)
        cstride = stride_of(eb, n, 'pack+1') if sc == 'coef+1' else stride
        nb = n * eb
        lay = Layout(eb)
        fused = name in ('mul_split', 'mul_split_rng', 'split_rng_state+mul')
        host_coef = name in ('split', 'mul_split')
        a = b = coef = None
        if name != 'rng_coeffs':
            a = lay.vec('a', n, one_in)
            if fused:
                b = lay.vec('b', n, one_in)
            if host_coef and t:
                coef = lay.mat('coef', 'input', t, cstride, n, one_in)
        rows_out = t if name == 'rng_coeffs' else m
        out = lay.mat('out', 'out', rows_out, stride, n, one_in)
        img = self.image(lay, data)
        offs = [out + r * stride * eb for r in range(rows_out)]

        def secrets():
            s = img[a:a + nb].copy()
            return ref.mul(s, img[b:b + nb].copy()) if fused else s
        where = (name, 't=%d m=%d' % (t, m), n, sc)
        if name == 'rng_coeffs':
            args = dict(key=KEY, nonce=NONCE, rounds=rounds, t=t, out=out, ostride=stride, n=n)
            calls = [(name, args, OK, self.fill_rows(offs, ref.rng_coeffs(KEY, NONCE, rounds, t, n), nb))]
        elif host_coef:
            c = [img[coef + j * cstride * eb:coef + j * cstride * eb + nb].copy() for j in range(t)]
            args = dict(a=a, coef=coef, cstride=cstride, t=t, m=m, out=out, ostride=stride, n=n)
            if fused:
                args['b'] = b
            calls = [(name, args, OK, self.fill_rows(offs, ref.split(secrets(), c, t, m), nb))]
        elif name in ('split_rng', 'mul_split_rng'):
            args = dict(a=a, key=KEY, nonce=NONCE, rounds=rounds, t=t, m=m, out=out, ostride=stride, n=n)
            if fused:
                args['b'] = b
            want = ref.split(secrets(), ref.rng_coeffs(KEY, NONCE, rounds, t, n), t, m)
            calls = [(name, args, OK, self.fill_rows(offs, want, nb))]
        else:
            # two calls in a row on a state created with a known key and nonce: nonces NONCE and NONCE + 1 (a call that
            # draws nothing -- t = 0 or n = 0 -- does not advance the state)
            state = self.ad.state_init(KEY, NONCE, rounds)
            args = dict(a=a, b=b, state=state, t=t, m=m, out=out, ostride=stride, n=n)
            step = 1 if t > 0 and n > 0 else 0
            calls = [('split_rng_state', args, OK,
                      self.fill_rows(offs, ref.split(secrets(), ref.rng_coeffs(KEY, NONCE + i * step, rounds, t, n), t, m), nb))
                     for i in range(2)]
        self.issue(lay, img, calls, where)
        self.seen.add(where)
        self.cases += 1

    # ---- the gate -----------------------------------------------------------------------------------------------------------
    def gate_operand(self, kind):
        """'0' -> (0, None); '1p' -> one row, lambda = 1; '1' -> one row, lambda != 1; 'k' -> k rows"""
        if kind == '0':
            return 0, None
        if kind == '1p':
            return 1, [1]
        k = int(kind)
        lam = self.scalars(k)
        if k == 1 and lam[0] == 1:
            lam[0] = self.q - 1 if self.q > 2 else 1
        return k, lam

    def scatter(self, offs):
        """row pointers in scattered order, not ascending"""
        offs = list(offs)
        return offs[1::2] + offs[0::2][::-1] if len(offs) > 2 else offs[::-1]

    def run_gate(self, ka_, kb_, t, n, sc, rounds=20, nbatch=0, plus=(0, 0, 0), state=False):
        """nbatch = 0: ffgpu_gate_rng; else ffgpu_gate_rng_batch with gate y's rows BETWEEN gate y - 1's: row r of an operand
        or of the output block is nbatch batch strides long, gate y sits y batch strides in.  plus: which of the batch strides
        (A, B, output) are a whole-pack value plus one instead of a whole-pack value.  state (ffgpu_gate_rng): two calls in a
        row on a device-resident state with a known key and nonce, handed a key and a nonce that must NOT be used (the entry
        point forwards nonce offset 0 with a state); expected: the state's key with nonces NONCE and NONCE + 1"""
        eb, ref = self.eb, self.ref
        one_in = sc == 'one-in'
        m = 2 * t + 1
        nb = n * eb
        ka, lam_a = self.gate_operand(ka_)
        kb, lam_b = self.gate_operand(kb_)
        lay = Layout(eb)
        ny = max(nbatch, 1)
        if nbatch:
            u = pack_unit(eb)
            p = -(-n // u) * u
            ya, yb, yo = (p + d for d in plus)
            ostride = ny * yo
        else:
            ya = yb = yo = 0
            ostride = stride_of(eb, n, sc)

        def operand(name, k, y_stride):
            # k rows; batched: each row is ny gates y_stride apart (row j at j * ny * y_stride)
            rs = y_stride if nbatch else n
            base = lay.add(name, 'input', k * ny * rs if nbatch else k * n,
                           [(j * ny + y) * rs for j in range(k) for y in range(ny)], n, one_in)
            return [base + j * ny * rs * eb for j in range(k)]
        rows_a = self.scatter(operand('A', ka, ya))
        rows_b = self.scatter(operand('B', kb, yb)) if kb else None
        if nbatch:
            out = lay.add('out', 'out', m * ostride, [i * ostride + y * yo for i in range(m) for y in range(ny)], n, one_in)
        else:
            out = lay.mat('out', 'out', m, ostride, n, one_in)
        img = self.image(lay)
        fills = []
        for call in range(2 if state else 1):
            offs, rows = [], []
            for y in range(ny):
                A = ref.recombine([img[r + y * ya * eb:r + y * ya * eb + nb].copy() for r in rows_a], lam_a, 1)[0]
                B = A if kb == 0 else \
                    ref.recombine([img[r + y * yb * eb:r + y * yb * eb + nb].copy() for r in rows_b], lam_b, 1)[0]
                nonce = NONCE + (y << 40) + (call if n else 0)
                rows += ref.split(ref.mul(A, B), ref.rng_coeffs(KEY, nonce, rounds, t, n), t, m)
                offs += [out + (y * yo + i * ostride) * eb for i in range(m)]
            fills.append(self.fill_rows(offs, rows, nb))
        args = dict(rows_a=rows_a, lam_a=lam_a, ka=ka, rows_b=rows_b, lam_b=lam_b, kb=kb, key=KEY, nonce=NONCE, rounds=rounds,
                    t=t, m=m, out=out, ostride=ostride, n=n)
        name = 'gate_rng'
        if nbatch:
            name = 'gate_rng_batch'
            args.update(ya=ya, yb=yb, yo=yo, nbatch=nbatch)
        if state:
            assert not nbatch
            args.update(state=self.ad.state_init(KEY, NONCE, rounds), key=bytes(32), nonce=0x77000000077)
        where = (name, 'ka=%s kb=%s t=%d nbatch=%d +%d%d%d%s' % ((ka_, kb_, t, nbatch) + tuple(plus) + (' state' * state,)), n, sc)
        self.issue(lay, img, [(name, args, OK, fill) for fill in fills], where)
        self.seen.add(where)
        self.cases += 1

    # ---- recombination ----------------------------------------------------------------------------------------------------
    def run_recombine(self, k, w, n, sc, alias=False, lam=None, data=None):
        """sc 'mixed': every row pointer and the output with an alignment of its own (taken in turn).  alias (w = 1): the
        output IS one of the rows"""
        eb, ref = self.eb, self.ref
        nb = n * eb
        stride = stride_of(eb, n, sc)
        lay = Layout(eb)

        def one_in():
            if sc == 'mixed':
                self._mixed += 1
                return self._mixed % 3 == 0
            return sc == 'one-in'
        rows = self.scatter([lay.vec('row%d' % j, n, one_in()) for j in range(k)])
        if alias:
            assert w == 1
            out = rows[k // 2]
            reg = next(r for r in lay.regions if r['base'] == out)
            lay.regions.append(dict(reg, name='out', role='out', alias=True))
        else:
            out = lay.mat('out', 'out', w, stride, n, one_in())
        img = self.image(lay, data)
        lam = lam if lam is not None else self.scalars(w * k)
        res = ref.recombine([img[r:r + nb].copy() for r in rows], lam, w)
        args = dict(rows=rows, lam=lam, k=k, w=w, out=out, ostride=stride, n=n)
        where = ('recombine', 'k=%d w=%d%s' % (k, w, ' out=row' if alias else ''), n, sc)
        self.issue(lay, img, [('recombine', args, OK, self.fill_rows([out + r * stride * eb for r in range(w)], res, nb))], where)
        self.seen.add(where)
        self.cases += 1

    # ---- chained calls: mul_split writes a block, recombine reads its rows, split reads the result ------------------------
    def run_chain(self, t, m, n, sc):
        eb, ref = self.eb, self.ref
        one_in = sc == 'one-in'
        stride = stride_of(eb, n, sc)
        nb = n * eb
        lay = Layout(eb)
        a, b = lay.vec('a', n, one_in), lay.vec('b', n, one_in)
        coef = lay.mat('coef', 'input', t, stride, n, one_in)
        sh = lay.mat('shares', 'out', m, stride, n, one_in)
        rec = lay.mat('rec', 'out', 1, stride, n, one_in)
        sh2 = lay.mat('shares2', 'out', m, stride, n, one_in)
        img = self.image(lay)
        lam = self.scalars(m)
        c = [img[coef + j * stride * eb:coef + j * stride * eb + nb].copy() for j in range(t)]
        s1 = ref.split(ref.mul(img[a:a + nb].copy(), img[b:b + nb].copy()), c, t, m)
        r = ref.recombine(s1, lam, 1)
        s2 = ref.split(r[0], c, t, m)
        o1 = [sh + i * stride * eb for i in range(m)]
        o2 = [sh2 + i * stride * eb for i in range(m)]
        calls = [('mul_split', dict(a=a, b=b, coef=coef, cstride=stride, t=t, m=m, out=sh, ostride=stride, n=n), OK,
                  self.fill_rows(o1, s1, nb)),
                 ('recombine', dict(rows=self.scatter(o1), lam=self.scatter(lam), k=m, w=1, out=rec, ostride=stride, n=n), OK,
                  self.fill_rows([rec], r, nb)),
                 ('split', dict(a=rec, coef=coef, cstride=stride, t=t, m=m, out=sh2, ostride=stride, n=n), OK,
                  self.fill_rows(o2, s2, nb))]
        where = ('chain', 't=%d m=%d' % (t, m), n, sc)
        self.issue(lay, img, calls, where)
        self.seen.add(where)
        self.cases += 1

    # ---- status codes on the same layouts: the tensor stays as it was ------------------------------------------------------
    def run_status(self, n=17):
        eb = self.eb
        stride = stride_of(eb, n, 'pack+1')
        lay = Layout(eb)
        rows = [lay.vec('row%d' % j, n) for j in range(3)]
        out = lay.mat('out', 'out', 9, stride, n)
        img = self.image(lay)
        lam3 = self.scalars(3)
        gate = dict(rows_a=rows, lam_a=lam3, ka=3, rows_b=None, lam_b=None, kb=0, key=KEY, nonce=NONCE, rounds=20, t=1, m=3,
                    out=out, ostride=stride, n=n)
        batch = dict(gate, ya=0, yb=0, yo=3 * stride, nbatch=2)
        none = dict(rows_a=[None] * 3, rows_b=None, out=None, n=0)
        calls = [
            ('recombine', dict(rows=[rows[j % 3] for j in range(65)], lam=self.scalars(65), k=65, w=1, out=out, ostride=stride,
                               n=n), ENOTSUP),
            ('gate_rng', dict(gate, t=4, m=9), ENOTSUP),
            ('gate_rng', dict(gate, rows_a=[rows[j % 3] for j in range(8)], lam_a=self.scalars(8), ka=8), ENOTSUP),
            ('gate_rng_batch', dict(batch, t=4, m=9), ENOTSUP),
            ('gate_rng_batch', dict(batch, nonce=1 << 40), EINVAL),
            ('gate_rng_batch', dict(batch, nonce=(1 << 40) - 1, ostride=n - 1), EINVAL),
            ('gate_rng', dict(gate, ostride=n - 1), EINVAL),
            ('split', dict(a=rows[0], coef=rows[1], cstride=n, t=1, m=3, out=out, ostride=n - 1, n=n), EINVAL),
            ('mul_split', dict(a=rows[0], b=rows[2], coef=rows[1], cstride=n, t=1, m=3, out=out, ostride=n - 1, n=n), EINVAL),
            ('split_rng', dict(a=rows[0], key=KEY, nonce=NONCE, rounds=20, t=1, m=3, out=out, ostride=n - 1, n=n), EINVAL),
            ('mul_split_rng', dict(a=rows[0], b=rows[1], key=KEY, nonce=NONCE, rounds=20, t=1, m=3, out=out, ostride=n - 1, n=n),
             EINVAL),
            ('split_rng_state', dict(a=rows[0], b=None, state=self.ad.state_init(KEY, NONCE, 20), t=1, m=3, out=out,
                                     ostride=n - 1, n=n), EINVAL),
            ('recombine', dict(rows=rows, lam=self.scalars(6), k=3, w=2, out=out, ostride=n - 1, n=n), EINVAL),
            # n = 0 with NULL device pointers
            ('split', dict(a=None, coef=None, cstride=0, t=1, m=3, out=None, ostride=0, n=0), OK),
            ('mul_split', dict(a=None, b=None, coef=None, cstride=0, t=2, m=5, out=None, ostride=0, n=0), OK),
            ('rng_coeffs', dict(key=KEY, nonce=NONCE, rounds=20, t=2, out=None, ostride=0, n=0), OK),
            ('split_rng', dict(a=None, key=KEY, nonce=NONCE, rounds=20, t=1, m=3, out=None, ostride=0, n=0), OK),
            ('mul_split_rng', dict(a=None, b=None, key=KEY, nonce=NONCE, rounds=20, t=1, m=3, out=None, ostride=0, n=0), OK),
            ('split_rng_state', dict(a=None, b=None, state=self.ad.state_init(KEY, NONCE, 20), t=1, m=3, out=None, ostride=0,
                                     n=0), OK),
            ('gate_rng', dict(gate, **none), OK),
            ('gate_rng_batch', dict(batch, **none), OK),
            ('recombine', dict(rows=[None] * 3, lam=lam3, k=3, w=1, out=None, ostride=0, n=0), OK),
        ]
        self.issue(lay, img, [(name, args, rc, None) for name, args, rc in calls], ('status', '', n, 'pack+1'))
        return len(calls)

    # ---- the matrices -------------------------------------------------------------------------------------------------------
    SPLIT_HOST = ('split', 'mul_split')
    SPLIT_RNG = ('split_rng', 'mul_split_rng', 'split_rng_state', 'split_rng_state+mul')
    REDUCED_CLASSES = ('tight', 'pack+1')
    LARGE_CLASSES = ('tight', 'pitched')

    def tm_list(self, full):
        """pairs with m >= the field order are skipped (party points must be distinct field elements)"""
        return [(t, m) for t, m in (TM if full else TM_REDUCED) if m < self.q]

    @staticmethod
    def rounds_of(sc):
        return {'tight': 0, 'pitched': 8, 'pack': 12}.get(sc, 20)

    def tiers(self, small=SMALL_SIZES, full=FULL_SIZES, large=LARGE_SIZES):
        """(sizes, stride classes, full parameter list?) of the three tiers of the matrix"""
        return ((small, self.REDUCED_CLASSES, False), (full, stride_classes(self.eb), True), (large, self.LARGE_CLASSES, False))

    def run_split_matrix(self, names, **sizes):
        for ns, classes, full in self.tiers(**sizes):
            for n in ns:
                for sc in classes:
                    for name in names:
                        if name == 'rng_coeffs':
                            for t in ((1, 2, 3, 4, 5) if full else (1, 3)):
                                self.run_split(name, t, t + 1, n, sc, self.rounds_of(sc))
                        else:
                            for t, m in self.tm_list(full):
                                self.run_split(name, t, m, n, sc, self.rounds_of(sc))
                if full:
                    for name in names:
                        if name in self.SPLIT_HOST:
                            for t, m in self.tm_list(False):
                                self.run_split(name, t, m, n, 'coef+1')

    def run_recombine_matrix(self, **sizes):
        for tier, (ns, classes, full) in enumerate(self.tiers(**sizes)):
            if full and self.eb != 16:
                classes = classes + ('mixed',)
            for n in ns:
                for sc in classes:
                    for k, w in (KW if full else KW_LARGE if tier == 2 else KW_REDUCED):
                        self.run_recombine(k, w, n, sc)
                    for k in (KW_ALIAS if full else KW_ALIAS[:1]):
                        self.run_recombine(k, 1, n, sc, alias=True)

    def run_gate_matrix(self, **sizes):
        for tier, (ns, classes, full) in enumerate(self.tiers(**sizes)):
            for n in ns:
                for sc in classes:
                    gates = [(a, b, t) for a in GATE_KA for b in GATE_KB for t in GATE_T] if full else \
                        GATE_LARGE if tier == 2 else GATE_REDUCED
                    for ka, kb, t in gates:
                        self.run_gate(ka, kb, t, n, sc, self.rounds_of(sc))
                    self.run_gate('3', '0', 1 + tier, n, sc, self.rounds_of(sc), state=True)

    def run_batch_matrix(self, **sizes):
        """nbatch = 3 with each batch stride a whole-pack value or that plus one, independently; nbatch = 1 through the batched
        entry point.  The stride class only says where the bases are: 'aligned' or 'one-in'"""
        for tier, (ns, classes, full) in enumerate(self.tiers(**sizes)):
            bases = ('aligned', 'one-in') if full and self.eb != 16 else ('aligned',)
            for n in ns:
                for sc in bases:
                    for ka, kb, t in BATCH_GATES:
                        for plus in (BATCH_COMBOS if full else ((0, 0, 0), (1, 1, 1), (0, 1, 1))):
                            self.run_gate(ka, kb, t, n, sc, 20, nbatch=3, plus=plus)
                    self.run_gate('3', '1p', 1, n, sc, 20, nbatch=1, plus=(0, 0, 1))

    def run_reduced(self, sizes=SMALL_SIZES):
        """the reduced matrix: every entry point at every small size in 'tight' and 'pack+1'"""
        z = dict(small=sizes, full=(), large=())
        self.run_split_matrix(self.SPLIT_HOST + ('rng_coeffs',) + self.SPLIT_RNG, **z)
        self.run_recombine_matrix(**z)
        self.run_gate_matrix(**z)
        self.run_batch_matrix(**z)


# ---- the number of cases, from the lists above (the tests assert them) ---------------------------------------------------------
def count_split(eb, q, names, small=len(SMALL_SIZES), full=len(FULL_SIZES), large=len(LARGE_SIZES)):
    red = sum(2 if nm == 'rng_coeffs' else sum(m < q for _, m in TM_REDUCED) for nm in names)
    ful = sum(5 if nm == 'rng_coeffs' else sum(m < q for _, m in TM) for nm in names)
    host = sum(nm in Driver.SPLIT_HOST for nm in names) * sum(m < q for _, m in TM_REDUCED)         # the class 'coef+1'
    return (small + large) * 2 * red + full * (len(stride_classes(eb)) * ful + host)


def count_recombine(eb, small=len(SMALL_SIZES), full=len(FULL_SIZES), large=len(LARGE_SIZES)):
    classes = len(stride_classes(eb)) + (eb != 16)
    return small * 2 * (len(KW_REDUCED) + 1) + full * classes * (len(KW) + len(KW_ALIAS)) + large * 2 * (len(KW_LARGE) + 1)


def count_gate(eb, small=len(SMALL_SIZES), full=len(FULL_SIZES), large=len(LARGE_SIZES)):
    every = len(GATE_KA) * len(GATE_KB) * len(GATE_T)
    return small * 2 * (len(GATE_REDUCED) + 1) + full * len(stride_classes(eb)) * (every + 1) + \
        large * 2 * (len(GATE_LARGE) + 1)                  # + 1: the case on a device-resident state (two calls)


def count_batch(eb, small=len(SMALL_SIZES), full=len(FULL_SIZES), large=len(LARGE_SIZES)):
    return (small + large) * (len(BATCH_GATES) * 3 + 1) + full * (1 + (eb != 16)) * (len(BATCH_GATES) * len(BATCH_COMBOS) + 1)


def count_reduced(eb, q, small=len(SMALL_SIZES)):
    z = dict(small=small, full=0, large=0)
    return count_split(eb, q, Driver.SPLIT_HOST + ('rng_coeffs',) + Driver.SPLIT_RNG, **z) + count_recombine(eb, **z) + \
        count_gate(eb, **z) + count_batch(eb, **z)
