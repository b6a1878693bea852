"""References, inputs and case lists for the contract of the six ffgpu_gf256_* entry points (include/ffgpu.h; the kernels are in
mpyc_amd/csrc/misc.hip).  tests/test_gpu_gf256_contract.py runs them on the device, tests/test_gf256_contract_host.py holds the
references against each other and against tests/golden/sbox.json without one.

Every expected value is Python-integer arithmetic of oracle/pyoracle.py (po.Field, po.mul, po.inv, po.pow254, po.sbox).  Two
forms of each reference:
  * `*_py`: the formula of ffgpu.h written out element by element on Python integers;
  * the same formula on numpy / torch arrays, where a product with a constant is a look-up into a row of the field's
    multiplication table -- and that table is filled by po.mul.  The host test shows the two forms equal at small sizes; the
    array form is what sizes of 10^5 .. 10^6 bytes are held against.
Nothing of the library is on the reference side.

    bit_affine        y_r = bias_r + sum_c M[r][c] x_c;  from_bits: sum_r 2^r y_r  (2^r = the field element x^r)
    to_bits           out[8 i + j] = ((in[i] >> j) & 1) + addend[8 i + j]
    mask_open         out[h] = sum_r coef[r] rows[r][h] + sum_p mu[p] (sum_b 2^b rbits_p[8 h + b])
    bits_affine_fold  out_y[h] = sum_r 2^r (M (bits(c[h]) + rbits_y[8h .. 8h+7]) + bias)_r
    sbox_layer        c_h = x_h^254 + sum_b 2^b r_{h,b};  out_j[h] = sum_r 2^r (M (bits(c_h) + R_j[8h .. 8h+7]) + bias)_r
                      (x, r: the secrets; R_j: party j's shares of the r) -- the re-sharing randomness of the eleven secure
                      products cancels in the opening, so every byte of every party's output row is known beforehand
"""
import itertools
import json
import os
import random

import numpy as np

from oracle import pyoracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
AES = 0x11b
# irreducible over GF(2), degrees 1 .. 8 (test_gf256_contract_host.py checks it)
BIT_AFFINE_MODULI = (0b11, 0b111, 0b1011, 0x13, 0x25, 0x43, 0x83, 0x11b, 0x11d)
TO_BITS_MODULI = (0b11, 0x13, 0x11b)
MT = ((3, 1), (4, 1), (5, 1), (5, 2), (6, 1), (6, 2), (7, 1), (7, 2), (7, 3))
PAD = 240                       # guard bytes on both sides of an output: a multiple of 16
GUARD = 0xa5


def golden_sbox():
    with open(os.path.join(GOLDEN, 'sbox.json')) as fh:
        return json.load(fh)


def field(modulus):
    return po.Field(modulus, True)


def irreducible(modulus):
    """no polynomial of degree 1 .. n / 2 divides it"""
    n = modulus.bit_length() - 1
    return all(po.clmod(modulus, d) != 0 for d in range(2, 1 << (n // 2 + 1)))


# ---- the field's tables, filled by po.mul ------------------------------------------------------------------------------------
_tables = {}


def mul_table(F):
    """(order, order) uint8: [a][b] = a b"""
    if F.modulus not in _tables:
        q = F.order
        _tables[F.modulus] = np.array([[po.mul(F, a, b) for b in range(q)] for a in range(q)], dtype=np.uint8)
    return _tables[F.modulus]


def pow2(F, r):
    """the field element x^r"""
    return po.reduce(F, 1 << r)


def xor_all(arrs, like):
    out = np.zeros_like(like)
    for a in arrs:
        out = out ^ a
    return out


# ---- matrices ------------------------------------------------------------------------------------------------------------------
def aes_map():
    rows8, b = po.aes_affine_rows()
    return [[(rows8[r] >> c) & 1 for c in range(8)] for r in range(8)], [(b >> r) & 1 for r in range(8)]


def identity():
    return [[int(r == c) for c in range(8)] for r in range(8)]


def shift_matrix(d):
    """one diagonal: y_r = x_{(r + d) % 8}"""
    return [[int(c == (r + d) % 8) for c in range(8)] for r in range(8)]


def random_matrix(F, rnd, bits_only):
    return [[rnd.randrange(2 if bits_only else F.order) for _ in range(8)] for _ in range(8)]


def random_bias(F, rnd):
    return [rnd.randrange(F.order) for _ in range(8)]


def general_map(F, seed=5):
    """a matrix over the whole field with every bit plane on some diagonal, plus a bias"""
    rnd = random.Random(seed)
    M = random_matrix(F, rnd, False)
    M[0][0] |= F.order >> 1
    return M, random_bias(F, rnd)


# ---- references on Python integers ---------------------------------------------------------------------------------------------
def affine_py(F, M, bias, x8):
    out = []
    for r in range(8):
        y = bias[r] if bias is not None else 0
        for c in range(8):
            y ^= po.mul(F, M[r][c], x8[c])
        out.append(y)
    return out


def fold_py(F, y8):
    v = 0
    for r in range(8):
        v ^= po.mul(F, pow2(F, r), y8[r])
    return v


def bit_affine_py(F, M, bias, from_bits, x):
    out = []
    for g in range(len(x) // 8):
        y = affine_py(F, M, bias, x[8 * g:8 * g + 8])
        out += [fold_py(F, y)] if from_bits else y
    return out


def to_bits_py(inp, addend):
    return [((v >> j) & 1) ^ (addend[8 * i + j] if addend is not None else 0) for i, v in enumerate(inp) for j in range(8)]


def mask_open_py(F, rows, coef, rbits, mu, n):
    out = []
    for h in range(n):
        v = 0
        for r, row in enumerate(rows):
            v ^= po.mul(F, coef[r], row[h])
        for p, rb in enumerate(rbits):
            v ^= po.mul(F, mu[p], fold_py(F, rb[8 * h:8 * h + 8]))
        out.append(v)
    return out


def bits_affine_fold_py(F, M, bias, c, rbits):
    out = []
    for h, cv in enumerate(c):
        x8 = [((cv >> b) & 1) ^ rbits[8 * h + b] for b in range(8)]
        out.append(fold_py(F, affine_py(F, M, bias, x8)))
    return out


def layer_py(F, M, bias, x, r, R):
    """x: the n secret bytes, r: their 8 n secret "bits" (any bytes), R: the parties' shares of r.  -> one row per party"""
    c = [po.pow254(F, xv) ^ fold_py(F, r[8 * h:8 * h + 8]) for h, xv in enumerate(x)]
    return [bits_affine_fold_py(F, M, bias, c, Rj) for Rj in R]


def share_rows_py(F, secrets, coefs, m):
    """party j (point j + 1) of secrets[h] + sum_q coefs[q][h] X^(q+1)"""
    rows = []
    for j in range(m):
        pt, row = j + 1, []
        for h, s in enumerate(secrets):
            v, pw = s, 1
            for cq in coefs:
                pw = po.mul(F, pw, pt)
                v ^= po.mul(F, cq[h], pw)
            row.append(v)
        rows.append(row)
    return rows


def recombine_py(F, points, rows):
    lam = po.recombination_vector(F, list(points), 0)
    out = []
    for h in range(len(rows[0])):
        v = 0
        for l, row in zip(lam, rows):
            v ^= po.mul(F, l, row[h])
        out.append(v)
    return out


# ---- the same formulas on numpy arrays -----------------------------------------------------------------------------------------
def affine_np(F, M, bias, x8):
    """x8: eight arrays (component c of every group)"""
    T = mul_table(F)
    out = []
    for r in range(8):
        y = xor_all([T[M[r][c]][x8[c]] for c in range(8) if M[r][c]], x8[0])
        out.append(y ^ np.uint8(bias[r]) if bias is not None else y)
    return out


def fold_np(F, y8):
    T = mul_table(F)
    return xor_all([T[pow2(F, r)][y8[r]] for r in range(8)], y8[0])


def bit_affine_np(F, M, bias, from_bits, x):
    g = np.asarray(x, dtype=np.uint8).reshape(-1, 8)
    y = affine_np(F, M, bias, [g[:, c] for c in range(8)])
    return fold_np(F, y) if from_bits else np.stack(y, axis=1).reshape(-1)


def to_bits_np(inp, addend):
    inp = np.asarray(inp, dtype=np.uint8)
    out = ((inp[:, None] >> np.arange(8, dtype=np.uint8)[None, :]) & 1).astype(np.uint8).reshape(-1)
    return out ^ np.asarray(addend, dtype=np.uint8) if addend is not None else out


def mask_open_np(F, rows, coef, rbits, mu, n):
    T = mul_table(F)
    out = np.zeros(n, dtype=np.uint8)
    for r, row in enumerate(rows):
        out ^= T[coef[r]][np.asarray(row, dtype=np.uint8)]
    for p, rb in enumerate(rbits):
        g = np.asarray(rb, dtype=np.uint8).reshape(-1, 8)
        out ^= T[mu[p]][fold_np(F, [g[:, b] for b in range(8)])]
    return out


def bits_affine_fold_np(F, M, bias, c, rbits):
    c = np.asarray(c, dtype=np.uint8)
    g = np.asarray(rbits, dtype=np.uint8).reshape(-1, 8)
    x8 = [((c >> np.uint8(b)) & 1) ^ g[:, b] for b in range(8)]
    return fold_np(F, affine_np(F, M, bias, x8))


def sbox_lut(rows8, b):
    """the byte -> byte map of ffgpu_gf256_sbox"""
    return np.array(po.sbox(range(256), list(rows8), b), dtype=np.uint8)


# ---- the layer as byte tables (torch; the device for the MB-sized cases, the CPU in the host test) -----------------------------
class LayerTables:
    """out = S[c] ^ T_0[R_0] ^ ... ^ T_7[R_7], c = P254[x] ^ W_0[r_0] ^ ... ^ W_7[r_7]: the formula of layer_py, linear in
    the bit shares, so table by table.  Every entry is layer_py's own arithmetic on one unit input."""

    def __init__(self, F, M, bias):
        zero8 = [0] * 8
        self.F, self.M, self.bias = F, M, bias
        self.P254 = [po.pow254(F, v) for v in range(256)]
        self.W = [[po.mul(F, pow2(F, b), v) for v in range(256)] for b in range(8)]
        lin = lambda x8: fold_py(F, affine_py(F, M, None, x8))
        self.T = [[lin(zero8[:b] + [v] + zero8[b + 1:]) for v in range(256)] for b in range(8)]
        self.S = [fold_py(F, affine_py(F, M, bias, [(c >> b) & 1 for b in range(8)])) for c in range(256)]
        self.MULC = [[po.mul(F, k, v) for v in range(256)] for k in range(256)]

    def on(self, torch, device):
        t = lambda a: torch.tensor(a, dtype=torch.uint8, device=device)
        return dict(P254=t(self.P254), W=t(self.W), T=t(self.T), S=t(self.S), MULC=t(self.MULC))


def _lut(torch, table, idx):
    return table[idx.to(torch.int64)]


def layer_inputs_torch(torch, tabs, dev, n, m, t, seed, device, xs=None, rs=None, any_bytes=True):
    """-> x (n), r (8 n): the secrets; X (m, xs), R (m, rs): the parties' shares, rows of n / 8 n bytes at strides xs / rs with
    GUARD between them.  x covers all 256 values from n = 256 on, 255 and 0 first; the polynomials' coefficients are any
    bytes, and so is r with any_bytes (the layer's formula is linear in r: the kernels must not assume 0 / 1) -- the output
    opens to the S-box of x only for r in {0, 1}, any_bytes = False.  Party j holds s + sum_q coef_q (j + 1)^q."""
    F = tabs.F
    xs, rs = xs or n, rs or 8 * n
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    draw = lambda cnt: torch.randint(0, 256, (cnt,), dtype=torch.uint8, generator=g).to(device)
    x = ((torch.arange(n, dtype=torch.int64, device=device) * 167 + 255) % 256).to(torch.uint8)
    if n >= 2:
        x[1] = 0
    r = draw(8 * n) if any_bytes else draw(8 * n) & 1
    X = torch.full((m, xs), GUARD, dtype=torch.uint8, device=device)
    R = torch.full((m, rs), GUARD, dtype=torch.uint8, device=device)
    cx, cr = [draw(n) for _ in range(t)], [draw(8 * n) for _ in range(t)]
    for j in range(m):
        sx, sr, pw = x.clone(), r.clone(), 1
        for q in range(t):
            pw = po.mul(F, pw, j + 1)
            sx ^= _lut(torch, dev['MULC'][pw], cx[q])
            sr ^= _lut(torch, dev['MULC'][pw], cr[q])
        X[j, :n], R[j, :8 * n] = sx, sr
    return x, r, X, R, cx, cr


def layer_expected_torch(torch, dev, x, r, R, n):
    """-> (m, n): every party's output row"""
    rg = r.reshape(n, 8)
    c = _lut(torch, dev['P254'], x)
    for b in range(8):
        c = c ^ _lut(torch, dev['W'][b], rg[:, b])
    s = _lut(torch, dev['S'], c)
    out = []
    for j in range(R.shape[0]):
        Rg = R[j, :8 * n].reshape(n, 8)
        o = s.clone()
        for b in range(8):
            o ^= _lut(torch, dev['T'][b], Rg[:, b])
        out.append(o)
    return torch.stack(out)


def opened_torch(torch, tabs, dev, rows, points):
    """recombination of the rows of the parties at `points` (1-based), on the device"""
    lam = po.recombination_vector(tabs.F, list(points), 0)
    out = torch.zeros_like(rows[0])
    for l, row in zip(lam, rows):
        out ^= _lut(torch, dev['MULC'][l], row)
    return out


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
def layer_resident(m, t):
    """resident workgroups per compute unit of k_gf8_sbox_layer, as the issue of this contract states them"""
    return (4 if m <= 4 else 3) if t == 1 else (3 if t == 2 else 2)


def layer_gsz(num_cu, m, t):
    return 256 * num_cu * layer_resident(m, t)


def trips(units, gsz):
    """iterations of a grid-stride loop of gsz threads over `units` units, thread 0"""
    return (units + gsz - 1) // gsz


def capped_n(entry, gsz):
    """smallest n at which thread 0 of a grid of gsz threads takes three trips through the vector loop of `entry`:
    sbox: 16 bytes a unit; to_bits: 2 bytes; the others: two units per trip, `half` apart, 2 bytes (bit_affine: 2 groups) each"""
    if entry == 'sbox':
        return 16 * (2 * gsz + 1)
    if entry == 'to_bits':
        return 2 * (2 * gsz + 1)
    return 2 * (2 * (2 * gsz + 1) - 1)          # half = (npair + 1) / 2 = 2 gsz + 1


def capped_trips(entry, n, gsz):
    if entry == 'sbox':
        return trips(n // 16, gsz)
    if entry == 'to_bits':
        return trips(n // 2, gsz)
    return trips((n // 2 + 1) // 2, gsz)


def subsets(m, k):
    return list(itertools.combinations(range(1, m + 1), k))
