"""TEST INFRASTRUCTURE ONLY: a stand-in for engine.FieldContext.keccak_local / keccak_round on numpy uint8, written from
the map include/ffgpu_math.h states (recombine, iota in front, theta, rho, pi, chi's local product, share generation), not from
the kernel: theta and rho-pi are the array operations of demos/sha3.py:85-95, the field products go through a
multiplication table built from Python-integer carry-less products.  The `-m "not gpu"` tests run protocols.keccak_f1600 /
sha3 / shake end to end on it, and the GPU tests compare the kernels with it byte for byte.  Matrices are engine.DevMatrix
over CPU torch tensors, so the protocols' byte-tensor XORs run unchanged."""
import itertools

import numpy as np
import torch

from mpyc_amd.engine import DevArray, DevMatrix

B = 1600
IRREDUCIBLE = {1: 0b11, 2: 0b111, 3: 0b1011, 4: 0b10011, 5: 0b100101, 6: 0b1000011, 7: 0b10000011, 8: 0x11b}
TRIANGULAR = tuple((i + 1) * (i + 2) // 2 % 64 for i in range(24))


def _polymulmod(a: int, b: int, modulus: int) -> int:
    deg, r = modulus.bit_length() - 1, 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> deg:
            a ^= modulus
    return r


def rc_bit(i: int) -> int:
    """coefficient of x^0 of x^i mod x^8 + x^6 + x^5 + x^4 + 1 (sha3.py:31-33)"""
    v = 1
    for _ in range(i):
        v = _polymulmod(v, 2, 0x171)
    return v & 1


ROUND_BITS = tuple(tuple(rc_bit(7 * r + j) for j in range(7)) for r in range(24))


def mul_table(modulus: int) -> np.ndarray:
    q = 1 << (modulus.bit_length() - 1)
    return np.array([[_polymulmod(a, b, modulus) for b in range(q)] for a in range(q)], dtype=np.uint8)


def keccak_map(T: np.ndarray, a: np.ndarray, iota_round: int, apply_round: bool) -> np.ndarray:
    """steps 1b-4 on one sender's recombined share a, an (nstates, 1600) uint8 array: iota of `iota_round` in front, then
    (apply_round) theta, rho, pi and out = b + (b[x+1] + 1) b[x+2]"""
    A = a.reshape(-1, 5, 5, 64).copy()                                 # [state, y, x, z]
    if iota_round >= 0:
        for j in range(7):
            A[:, 0, 0, (1 << j) - 1] ^= ROUND_BITS[iota_round][j]
    if not apply_round:
        return A.reshape(-1, B)
    C = np.bitwise_xor.reduce(A, axis=1)                               # [state, x, z]
    D = np.roll(C, 1, axis=1) ^ np.roll(np.roll(C, -1, axis=1), 1, axis=2)
    A ^= D[:, np.newaxis, :, :]
    Bm = A.copy()
    x, y = 1, 0
    for shift in TRIANGULAR:
        lane = A[:, y, x]
        x, y = y, (2 * x + 3 * y) % 5
        Bm[:, y, x] = np.roll(lane, shift, axis=1)
    out = Bm ^ T[np.roll(Bm, -1, axis=2) ^ 1, np.roll(Bm, -2, axis=2)]
    return out.reshape(-1, B)


class KeccakCpuContext:
    """GF(2^n), 1 <= n <= 8, with the two Keccak methods of engine.FieldContext and the memory calls protocols.sponge uses."""
    binary = True
    elem_bytes = 1
    device = 0
    pad = 24                       # row pitch of empty_matrix beyond n: a multiple of 4, so that strides are exercised

    def __init__(self, modulus: int, seed: int = 1):
        self.modulus = int(modulus)
        self.n_bits = self.modulus.bit_length() - 1
        self.order = 1 << self.n_bits
        self.T = mul_table(self.modulus)
        self.rng = np.random.default_rng(seed)
        self.launches = []

    # ---- memory ----
    def empty_matrix(self, rows: int, n: int) -> DevMatrix:
        stride = n + self.pad
        return DevMatrix(self, torch.zeros((rows, stride), dtype=torch.uint8), rows, n, stride)

    def matrix_from_numpy(self, a: np.ndarray) -> DevMatrix:
        mtx = self.empty_matrix(a.shape[0], a.shape[1])
        mtx.t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a))
        return mtx

    @staticmethod
    def _at(row: DevArray, byte_offset: int, n: int) -> np.ndarray:
        """the n bytes that start byte_offset after the row's first"""
        return torch.as_strided(row.t, (n,), (1,), row.t.storage_offset() + byte_offset).numpy()

    def _recombined(self, rows, lam, n, offset):
        if not 1 <= len(rows) <= 7 or len(lam) != len(rows) or any(r.n != n for r in rows):
            raise NotImplementedError('keccak: 1..7 rows of 1600 * nstates elements, one lambda each')
        a = np.zeros(n, dtype=np.uint8)
        for r, l in zip(rows, lam):
            a ^= self.T[int(l)][self._at(r, offset, n)]
        return a

    # ---- the two methods ----
    def keccak_local(self, rows, lam, nstates, iota_round=-1, apply_round=True, nbatch=1, stride_in=0, out=None):
        if not -1 <= iota_round <= 23:
            raise NotImplementedError('keccak: iota_round in -1..23')
        n = B * nstates
        out = self.empty_matrix(nbatch, n) if out is None else out
        self.launches.append(('local', iota_round, bool(apply_round), nbatch))
        res = [keccak_map(self.T, self._recombined(rows, lam, n, y * stride_in).reshape(nstates, B), iota_round, apply_round)
               for y in range(nbatch)]                                  # every sender reads before any row is written
        for y in range(nbatch):
            out.t[y, :n] = torch.from_numpy(res[y].reshape(n))
        return out

    def keccak_round(self, rows, lam, nstates, t, m, iota_round=-1, stride_in=0, out=None, key=None, nonce=0, rounds=20,
                     state=None):
        if not -1 <= iota_round <= 23 or not ((m, t) == (1, 0) or (1 <= t <= 3 and 2 * t + 1 <= m <= 7)) or self.order <= m:
            raise NotImplementedError('keccak_round: (m, t) and iota_round as include/ffgpu_math.h lists them')
        n, k = B * nstates, 2 * t + 1
        out = self.empty_matrix(m * k, n) if out is None else out
        if state is not None:
            state.take_offset()
        self.launches.append(('round', iota_round, t, m))
        vals = [keccak_map(self.T, self._recombined(rows, lam, n, y * stride_in).reshape(nstates, B), iota_round, True).reshape(n)
                for y in range(k)]
        for y in range(k):
            coef = self.rng.integers(0, self.order, size=(t, n), dtype=np.uint8)
            for j in range(m):
                share, xp = vals[y].copy(), 1
                for q in range(t):
                    xp = _polymulmod(xp, j + 1, self.modulus)
                    share ^= self.T[xp][coef[q]]
                out.t[j * k + y, :n] = torch.from_numpy(share)
        return out


# ---- helpers the tests share -----------------------------------------------------------------------------------------
def lagrange_at_zero(modulus: int, xs):
    """Lagrange coefficients at 0 for the points xs over GF(2^n) as bit patterns (brute-force inverses)"""
    q = 1 << (modulus.bit_length() - 1)
    inv = {a: next(b for b in range(1, q) if _polymulmod(a, b, modulus) == 1) for a in range(1, q)}
    lam = []
    for i in xs:
        num = den = 1
        for j in xs:
            if j != i:
                num = _polymulmod(num, j, modulus)
                den = _polymulmod(den, i ^ j, modulus)
        lam.append(_polymulmod(num, inv[den], modulus))
    return lam


def share_bits(modulus: int, bits: np.ndarray, t: int, m: int, rng) -> np.ndarray:
    """(m, n) degree-t Shamir shares over GF(2^n) of the flat 0 / 1 array `bits` (parties at the points 1..m)"""
    T, q = mul_table(modulus), 1 << (modulus.bit_length() - 1)
    flat = np.asarray(bits, dtype=np.uint8).reshape(-1)
    coef = rng.integers(0, q, size=(t, flat.size), dtype=np.uint8)
    out = np.empty((m, flat.size), dtype=np.uint8)
    for j in range(m):
        share, xp = flat.copy(), 1
        for c in coef:
            xp = _polymulmod(xp, j + 1, modulus)
            share ^= T[xp][c]
        out[j] = share
    return out


def open_shares(modulus: int, rows: np.ndarray, t: int) -> np.ndarray:
    """the secret of degree-t shares held by the parties 1..t+1 (rows[0..t])"""
    T = mul_table(modulus)
    out = np.zeros(rows.shape[1], dtype=np.uint8)
    for l, r in zip(lagrange_at_zero(modulus, range(1, t + 2)), rows[:t + 1]):
        out ^= T[l][r]
    return out


def subsets(m: int, size: int):
    return itertools.combinations(range(m), size)
