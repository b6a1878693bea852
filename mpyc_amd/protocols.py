"""Local parts of the reference's secure-array protocols, composed from the kernels, for ALL m parties of a
computation held on one GPU.

MPyC runs one process per party and moves shares over TCP (runtime.py); what each party computes between
two messages is exactly the kernels of this package.  The functions below chain those kernels in the order
the reference's protocols do, for every party at once, with the "network" replaced by handing device rows
from one party's share matrix to the other parties' recombination.  They exist to (a) test the gate
compositions end to end (open(result) must equal the plaintext function) and (b) measure the compute of a
whole protocol (bench.py: the np_aes S-box layer over secure bytes, BASELINE config 5).

A secret-shared array is a list of m DevArrays: entry i is the share of party i+1 (x-coordinate i+1,
thresha.py:61).  Nothing here runs on the CPU except Lagrange vectors (a handful of scalars, as in the
reference, thresha.py:67-85).
"""
from typing import List, Optional, Sequence

from . import thresha
from .engine import DevArray, FieldContext

Shares = List[DevArray]


def _lagrange(field, xs: Sequence[int]) -> List[int]:
    return [int(v) for v in thresha._recombination_vector(field, tuple(xs), 0)]


def _parties(what: str, t: int, m: int, *others: int) -> int:
    """k = 2t+1, the number of parties that re-share a degree-2t product; refuses fewer than k parties and an operand
    (`others`: how many parties each further operand has shares of) that is not there for every party."""
    k = 2 * t + 1
    if m < k or any(o != m for o in others):
        raise ValueError(f'{what} needs m >= 2t+1 parties, and every operand for each of them')
    return k


def _axis_check(what: str, xs: Shares, outer: int, k: int, inner: int):
    if outer < 1 or k < 1 or inner < 1 or any(x.n != outer * k * inner for x in xs):
        raise ValueError(f'{what}: the shares are not (outer, k, inner) arrays')


def share(ctx: FieldContext, x: DevArray, t: int, m: int, rng=None) -> Shares:
    """np_random_split (thresha.py:47-64) with coefficients from the device CSPRNG; row i -> party i+1.
    rng: an engine.RngState (device-resident generator, required inside HIP-graph capture) or None (fresh
    host key per call)."""
    mtx = ctx.split_rng(x, t, m, state=rng)
    return [mtx.row(i) for i in range(m)]


def open_(ctx: FieldContext, field, xs: Shares, t: int, degree: Optional[int] = None) -> DevArray:
    """runtime.output (runtime.py:560-600): recombine the first degree+1 shares at x = 0."""
    k = (t if degree is None else degree) + 1
    return ctx.recombine(xs[:k], _lagrange(field, range(1, k + 1)))


def add_public(ctx: FieldContext, xs: Shares, c: DevArray) -> Shares:
    """Shamir: every party adds the public value to its share."""
    return [ctx.add(x, c) for x in xs]


# ---- the re-sharing round (runtime._reshare, runtime.py:603-689) -----------------------------------------------
class Pending:
    """A secret-shared value each party holds as a RECOMBINATION it has not performed yet: party j's share
    is sum_i lam[i] * rows[j][i] (rows[j] = the sub-shares party j received).  A materialised sharing is the
    1-row case with lam = [1]."""

    __slots__ = ('rows', 'lam')

    def __init__(self, rows, lam):
        self.rows, self.lam = rows, lam

    @classmethod
    def of(cls, xs: Shares) -> 'Pending':
        return cls([[x] for x in xs], [1])

    @classmethod
    def dealt(cls, mats, lam, m: int) -> 'Pending':
        """From the senders' share matrices: row j of mats[i] is what sender i dealt to party j."""
        return cls([[mat.row(j) for mat in mats] for j in range(m)], lam)


def materialize(ctx: FieldContext, x) -> Shares:
    """Pending -> the parties' shares (the recombination of runtime._reshare, runtime.py:677-689)."""
    if not isinstance(x, Pending):
        return x
    if len(x.lam) == 1 and x.lam[0] == 1:
        return [r[0] for r in x.rows]
    return [ctx.recombine(r, x.lam) for r in x.rows]


def reshare(ctx: FieldContext, field, xs, t: int, m: int, rng=None, mul_by: Optional[Shares] = None,
            what: str = 'multiplication') -> Pending:
    """The re-sharing of a secure round: each of the first 2t+1 parties deals its degree-2t value xs[i] (with mul_by: the
    product xs[i] * mul_by[i], formed inside the share generation, ffgpu_mul_split_rng) to all m parties with a fresh
    degree-t polynomial, senders in order.  The result is Pending: rows[j] are the sub-shares party j received, lam the
    Lagrange vector for x = 0 -- materialize() recombines them, a round with a fused apply end hands rows[j] and lam to
    its apply wrapper.  xs may be an iterator; only its first 2t+1 values are taken, each when its sender's turn comes."""
    k = _parties(what, t, m)
    mats = [ctx.split_rng(x, t, m, mul_by=None if mul_by is None else mul_by[i], state=rng) for i, x in zip(range(k), xs)]
    return Pending.dealt(mats, _lagrange(field, range(1, k + 1)), m)


def multiply(ctx: FieldContext, field, xs: Shares, ys: Shares, t: int, rng=None) -> Shares:
    """runtime.np_multiply (runtime.py:1096-1141) = local product of shares (degree 2t) + _reshare
    (runtime.py:603-689): each of the first 2t+1 parties re-shares its product with a fresh degree-t
    polynomial -- the product is formed inside the share-generation kernel (ffgpu_mul_split_rng) --, then
    every party recombines the 2t+1 sub-shares it received with the Lagrange vector for x = 0."""
    return materialize(ctx, reshare(ctx, field, xs, t, len(xs), rng, mul_by=ys))


# ---- chains of multiplications with the recombined share kept in registers ------------------------------
def multiply_pending(ctx: FieldContext, field, x, y, t: int, rng=None) -> Pending:
    """multiply() for operands that may be Pending (y is x: a squaring): the first 2t+1 parties recombine both
    factors, multiply and re-share in ONE kernel (ffgpu_gate_rng); the result stays Pending, so the next
    multiplication consumes the new sub-shares directly.  Needs t <= 3."""
    px = x if isinstance(x, Pending) else Pending.of(x)
    py = None if y is x else (y if isinstance(y, Pending) else Pending.of(y))
    m = len(px.rows)
    k = _parties('multiplication', t, m)
    mats = [ctx.gate(px.rows[i], px.lam, py.rows[i] if py else None, py.lam if py else None, t, m, state=rng)
            for i in range(k)]
    return Pending.dealt(mats, _lagrange(field, range(1, k + 1)), m)


def _pow254_chain(mul, d):
    """x^254 by the reference's addition chain (runtime.py:1356-1367): 11 multiplications.  The reference stacks
    (c, d) in two rounds to halve the number of MESSAGES; locally the stacked product is two products, issued here
    as such (no concatenation traffic)."""
    c = mul(d, d)
    c = mul(c, c)
    c = mul(c, c)
    c = mul(c, d)
    c = mul(c, c)
    c, d = mul(c, c), mul(c, d)
    c, d = mul(c, c), mul(c, d)
    c = mul(c, d)
    return mul(c, c)


def pow254_fused(ctx: FieldContext, field, xs: Shares, t: int, rng=None) -> Shares:
    """pow254() with every intermediate share kept Pending: 11 fused gate kernels + 1 recombination per party
    instead of 11 x (share generation + recombination)."""
    return materialize(ctx, _pow254_chain(lambda a, b: multiply_pending(ctx, field, a, b, t, rng), Pending.of(xs)))


def matmul(ctx: FieldContext, field, xs: Shares, ys: Shares, M: int, K: int, N: int, t: int, rng=None) -> Shares:
    """runtime.np_matmul (runtime.py:2481-2541): every party multiplies its share matrices locally
    (`A @ B` then one reduction, :2531 -- the dense-product kernel) and the degree-2t result is re-shared as
    in multiply().  xs: (M, K) and ys: (K, N) row-major share matrices; returns shares of the (M, N) product."""
    prod = (ctx.matmul(x, y, M, K, N) for x, y in zip(xs, ys))             # each sender's product right before it deals it
    return materialize(ctx, reshare(ctx, field, prod, t, len(xs), rng))


def pow254(ctx: FieldContext, field, xs: Shares, t: int, rng=None) -> Shares:
    """x^254 in 11 secure multiplications (_pow254_chain)."""
    return _pow254_chain(lambda a, b: multiply(ctx, field, a, b, t, rng), xs)


def to_bits_gf256(ctx: FieldContext, field, xs: Shares, rbits: Shares, t: int) -> Shares:
    """runtime.np_to_bits for a binary field (runtime.py:4411-4423): with shared random bits r_j,
    r = sum_j r_j 2^j, open c = x + r, return bits(c) + r_bits.  xs: n bytes, rbits: 8n bit shares."""
    weights = [[1 << j for j in range(8)]]
    masked = [ctx.add(x, ctx.group_matvec(r, weights)) for x, r in zip(xs, rbits)]     # a + r_modl
    c = open_(ctx, field, masked, t)
    return [ctx.to_bits(c, addend=r) for r in rbits]                               # c_bits + r_bits


def from_bits(ctx: FieldContext, bits: Shares, l: int = 8) -> Shares:
    """runtime.np_from_bits (runtime.py:4475-4484): sum_j x_j 2^j over the last axis (local).  Groups of more than 16 bits
    (ffgpu_group_matvec serves up to 16) are the product of the (n, l) bit matrix with the power vector."""
    if l <= 16:
        weights = [[1 << j for j in range(l)]]
        return [ctx.group_matvec(b, weights) for b in bits]
    if any(b.n % l for b in bits):
        raise ValueError('array length is not a multiple of the group size')
    pw = ctx.from_ints([(1 << j) % ctx.modulus for j in range(l)])
    return [ctx.matmul(b, pw, b.n // l, l, 1) for b in bits]


# ---- secure comparison over a prime field (runtime.np_sgn, runtime.py:3622-3693) -------------------------------
def _rows(ctx: FieldContext, x: DevArray, lo: int, hi: int, n: int) -> DevArray:
    """rows lo .. hi-1 of a bit-major (rows, n) array: a view"""
    return DevArray(ctx, x.t[lo * n:hi * n], (hi - lo) * n)


def prod_rows(ctx: FieldContext, field, xs: Shares, rows: int, t: int, rng=None) -> Shares:
    """runtime.np_prod along the leading axis (runtime.py:2198-2203) of a bit-major (rows, n) sharing: each level
    multiplies the lower half of the rows with the upper half in one secure multiplication, an odd leading row is carried
    over to the next level; ceil(log2 rows) rounds.  Returns shares of the n products."""
    if rows < 1 or xs[0].n % rows:
        raise ValueError('prod_rows: the arrays are not (rows, n)')
    n = xs[0].n // rows
    while rows > 1:
        n0, half = rows % 2, (rows + 1) // 2
        prod = multiply(ctx, field, [_rows(ctx, x, n0, half, n) for x in xs], [_rows(ctx, x, half, rows, n) for x in xs], t, rng)
        xs = [_cat(ctx, [_rows(ctx, x, 0, 1, n), p]) for x, p in zip(xs, prod)] if n0 else prod
        rows = half
    return list(xs)


def is_zero_public(ctx: FieldContext, field, xs: Shares, rzero: Shares, t: int) -> DevArray:
    """runtime.np_is_zero_public for large fields (runtime.py:946-949 and the opening at threshold 2t): every party
    multiplies its share with its share of nonzero randomness (a degree-2t sharing of x r) and the product is opened from
    2t+1 parties.  Returns the PUBLIC w = x r: zero exactly where x is.  rzero: a caller-supplied sharing of nonzero
    random values."""
    k = _parties('the zero test', t, len(xs))
    return open_(ctx, field, [ctx.mul(xs[i], rzero[i]) for i in range(k)], t, degree=2 * t)


def compare_zero(ctx: FieldContext, field, xs: Shares, rbits: Shares, sbits: Optional[Shares], rdivl: Shares,
                 rzero: Optional[Shares], t: int, l: int, mode: str = 'lt', rng=None) -> Shares:
    """runtime.np_sgn (runtime.py:3622-3693) on integers for all parties: mask -> open -> expand -> prod_rows(e) ->
    is_zero_public -> finish, the three local steps one kernel each (ffgpu_sgn_mask / _expand / _finish).

    mode 'lt': shares of [a < 0] (LT=True); 'eq': shares of [a == 0] = prod_rows(1 - Xor) (EQ=True; sbits and rzero are
    not used and may be None); 'sgn': shares of the sign, (eq - 1) (2 lt - 1), one more multiplication.

    It is assumed that -2^(l-1) <= a < 2^(l-1), and the caller guarantees 2^(l+1) + 2^l max(rdivl) < p so that the opened
    value does not wrap.  The random inputs are sharings supplied by the caller: rbits n*l random bits per party
    (element-major, most significant first), sbits n random bits, rdivl n random values below the statistical bound,
    rzero n nonzero random values."""
    if mode not in ('lt', 'eq', 'sgn'):
        raise ValueError("mode is 'lt', 'eq' or 'sgn'")
    m = len(xs)
    c = open_(ctx, field, [ctx.sgn_mask(xs[i], rbits[i], rdivl[i], l) for i in range(t + 1)], t)
    want_e, want_nx = mode != 'eq', mode != 'lt'
    ex = [ctx.sgn_expand(c, xs[i], rbits[i], sbits[i] if want_e else None, l, want_e=want_e, want_nx=want_nx) for i in range(m)]
    eq = prod_rows(ctx, field, [x[1] for x in ex], l, t, rng) if want_nx else None
    if mode == 'eq':
        return eq
    w = is_zero_public(ctx, field, prod_rows(ctx, field, [x[0] for x in ex], l + 1, t, rng), rzero, t)
    lt = [ctx.sgn_finish(w, sbits[i], ex[i][2], l) for i in range(m)]
    if mode == 'lt':
        return lt
    p = ctx.modulus
    return multiply(ctx, field, [ctx.add_scalar(x, p - 1) for x in eq],
                    [ctx.add_scalar(ctx.mul_scalar(x, 2), p - 1) for x in lt], t, rng)


# ---- secure equality over a Blum prime: the Legendre zero test (runtime.np_equal, runtime.py:3569-3579; _np_is_zero,
# runtime.py:3581-3620) ---------------------------------------------------------------------------------------------
def equal_route(p: int, l: int, sec_param: int) -> str:
    """The dispatch of runtime.np_equal (runtime.py:3576) for a secure integer or fixed-point type of bit length l over the
    prime p: 'legendre' (the probabilistic zero test, is_zero) when l / 2 > sec_param >= 8 and p = 3 mod 4, else 'bits'
    (np_sgn(EQ=True): compare_zero(mode='eq'))."""
    return 'legendre' if l / 2 > sec_param >= 8 and p % 4 == 3 else 'bits'


def is_zero(ctx: FieldContext, field, xs: Shares, t: int, k: int, rand_zero, rng=None) -> Shares:
    """runtime._np_is_zero (runtime.py:3581-3620) for all parties: shares of [x == 0], wrong (1 for a nonzero x) with
    probability 2^-k per element.  p = 3 mod 4, so -1 is a non-residue: with z a random bit, r and u random elements,
    c = x r + (1 - 2 z) u^2 is a residue exactly when z = 0 if x = 0, and independently of z otherwise.

    u2 = multiply(s, s) (one re-sharing round) -> iszero_mask per party (degree 2t) -> one opening from 2t+1 parties -> ONE
    legendre_code on the public values -> iszero_finish per party -> prod_rows over the k rows: 2 + ceil(log2 k) rounds.
    The arrays are row-major (k, n): row i holds the i-th masked copy.

    rand_zero(count) supplies three sharings of count = k n entries: uniform bits z, uniform field elements r, uniform field
    elements s.  The inputs are never written."""
    m = len(xs)
    if ctx.binary or ctx.modulus % 4 != 3:
        raise ValueError('is_zero: a prime field with p = 3 mod 4')
    if k < 1:
        raise ValueError('is_zero: k >= 1')
    senders = _parties('the zero test', t, m)                                      # 2t+1: the masked values have degree 2t
    n = xs[0].n
    z, r, s = rand_zero(k * n)
    if not (len(z) == len(r) == len(s) == m) or any(v.n != k * n for w in (z, r, s) for v in w):
        raise ValueError('is_zero: rand_zero(count) returns three sharings of count entries for every party')
    u2 = multiply(ctx, field, s, s, t, rng)
    c = open_(ctx, field, [ctx.iszero_mask(xs[i], r[i], z[i], u2[i], k) for i in range(senders)], t, degree=2 * t)
    code = ctx.legendre_code(c)
    return prod_rows(ctx, field, [ctx.iszero_finish(code, z[i]) for i in range(m)], k, t, rng)


def equal(ctx: FieldContext, field, xs: Shares, ys: Shares, t: int, k: int, rand_zero, rng=None) -> Shares:
    """runtime.np_equal on the Legendre route (runtime.py:3571, 3577): is_zero of the difference; shares of [x == y]."""
    if len(xs) != len(ys):
        raise ValueError('equal: both operands for every party')
    return is_zero(ctx, field, [ctx.sub(x, y) for x, y in zip(xs, ys)], t, k, rand_zero, rng)


# ---- sorting along one axis (runtime.np_sort, runtime.py:1738-1774) ---------------------------------------------
def sort_stages(k: int):
    """The stages (p, d, r) of Batcher's merge-exchange network over k elements (Knuth 5.2.2M), in the order of the
    reference's loop (runtime.py:1759-1772): stage (p, d, r) compares position i with i + d for every i < k - d with
    i & p == r."""
    if k < 2:
        return
    t = (k - 1).bit_length()
    p = 1 << t - 1
    while p:
        d, q, r = p, 1 << t - 1, 0
        while d:
            yield p, d, r
            d, q, r = q - p, q >> 1, p
        p >>= 1


def sort(ctx: FieldContext, field, xs: Shares, outer: int, k: int, inner: int, t: int, l: int, rand, rng=None) -> Shares:
    """runtime.np_sort along k of a sharing of the contiguous (outer, k, inner) integer array, ascending, for all parties:
    every party's share is copied once (np_copy, runtime.py:1750), then per stage (p, d, r) of sort_stages(k)
      cx_diff per party: the compact differences b1 - b0 (ffgpu_cx_diff),
      compare_zero(..., mode='lt') on them: shares of [b1 < b0],
      the first 2t+1 parties re-share [b1 < b0] (b1 - b0) (the product inside ffgpu_mul_split_rng),
      cx_apply per party: the received sub-shares recombined and added to b0, subtracted from b1 in place (ffgpu_cx_apply).
    Returns the sorted sharing; xs is not written.

    rand(count) returns (rbits, sbits, rdivl, rzero) as Shares for `count` comparisons of bit length l -- count * l random
    bits (element-major), count random bits, count values below the statistical bound, count nonzero values: the inputs
    of compare_zero, drawn by the caller per stage.

    It is assumed that every difference of two values along k lies in [-2^(l-1), 2^(l-1)), and, as for compare_zero, that
    2^(l+1) + 2^l max(rdivl) < p.  Needs m >= 2t+1 parties."""
    m = len(xs)
    _parties('sort', t, m)
    _axis_check('sort', xs, outer, k, inner)
    a = [x.clone() for x in xs]
    for p, d, r in sort_stages(k):
        pairs = ctx.cx_pairs(k, p, d, r)
        if pairs == 0:
            continue
        diff = [ctx.cx_diff(x, outer, k, inner, p, d, r) for x in a]
        rbits, sbits, rdivl, rzero = rand(outer * pairs * inner)
        c = compare_zero(ctx, field, diff, rbits, sbits, rdivl, rzero, t, l, mode='lt', rng=rng)
        sub = reshare(ctx, field, c, t, m, rng, mul_by=diff)
        for j in range(m):
            ctx.cx_apply(a[j], sub.rows[j], sub.lam, outer, k, inner, p, d, r)
    return a


# ---- bit decomposition over a prime field (runtime.np_to_bits, runtime.py:4391-4456) ----------------------------
def carry_prefix(ctx: FieldContext, field, G: Shares, P: Shares, l: int, n: int, t: int, rng=None) -> Shares:
    """The prefix-carry network of runtime.np_add_bits (runtime.py:4301-4334) for all parties, on Shares of the bit-major
    (l, n) generate / propagate values, ceil(log2 l) rounds (csrc/bits_geom.hpp); per round
      carry_prod per party: the compact (R, n) local products of the round (ffgpu_carry_prod),
      the first 2t+1 parties re-share them (ffgpu_split_rng),
      carry_apply per party: the received sub-shares recombined and added into G / stored to P in place (ffgpu_carry_apply).
    Overwrites G with the prefix carries (carry k = the carry out of bit positions 0..k) and returns it; P is overwritten
    too.  Needs m >= 2t+1 parties."""
    m = len(G)
    kk = _parties('the carry network', t, m, len(P))
    if l < 1 or n < 0 or any(x.n != l * n for x in G) or any(x.n != l * n for x in P):
        raise ValueError('carry_prefix: the shares are not (l, n) arrays')
    for rho in range(1, ctx.carry_rounds(l) + 1):
        sub = reshare(ctx, field, [ctx.carry_prod(G[i], P[i], l, rho) for i in range(kk)], t, m, rng)
        for j in range(m):
            ctx.carry_apply(G[j], P[j], sub.rows[j], sub.lam, l, rho)
    return G


def to_bits(ctx: FieldContext, field, xs: Shares, rbits: Shares, rdivl: Shares, t: int, l: int, offset: Optional[int] = None,
            rng=None) -> Shares:
    """runtime.np_to_bits (runtime.py:4391-4456) on integers over a prime field, for all parties: bits_mask on t+1
    parties -> open -> bits_expand -> carry_prefix -> bits_finish, each per party (ffgpu_bits_mask / _expand / _finish and
    the two level kernels).  Returns Shares of the (n, l) bits, element-major, least significant first; from_bits(..., l)
    is their inverse.

    rbits: n*l random bits per party (element-major, least significant first), rdivl: n random values below the
    statistical bound; offset (default 2^l) is added before the opening.  The caller guarantees that
    -2^(l-1) <= a < 2^(l-1) or 0 <= a < 2^l, and that 0 <= a + offset + 2^l rdivl - r < p for every element (r the value of
    the random bits), so that the opened value does not wrap.  Needs m >= 2t+1 parties."""
    m = len(xs)
    _parties('bit decomposition', t, m)
    n = xs[0].n
    if any(x.n != n for x in xs) or len(rbits) != m or len(rdivl) != m or any(r.n != n * l for r in rbits):
        raise ValueError('to_bits: n values, n*l bit shares and n high masks per party')
    off = (1 << l) if offset is None else int(offset)
    c = open_(ctx, field, [ctx.bits_mask(xs[i], rbits[i], rdivl[i], l, off) for i in range(t + 1)], t)
    gp = [ctx.bits_expand(c, rbits[i], l) for i in range(m)]
    G = carry_prefix(ctx, field, [x[0] for x in gp], [x[1] for x in gp], l, n, t, rng)
    return [ctx.bits_finish(c, rbits[i], G[i], l) for i in range(m)]


# ---- maximum, minimum and their positions along one axis (runtime.np_amax / np_amin, runtime.py:3377-3473;
# np_argmax / np_argmin, runtime.py:3695-3949; np_maximum / np_minimum, runtime.py:3346-3360) --------------------
def _tour_round(ctx: FieldContext, field, a: Shares, outer: int, k: int, inner: int, mode: int, neg: bool, t: int, l: int, rand,
                rng):
    """One round along k >= 2 for all parties: (the next level (outer, k // 2 + k % 2, inner), the comparison bits)."""
    diff = [ctx.tour_diff(x, outer, k, inner, mode, neg) for x in a]
    rbits, sbits, rdivl, rzero = rand(outer * (k // 2) * inner)
    c = compare_zero(ctx, field, diff, rbits, sbits, rdivl, rzero, t, l, mode='lt', rng=rng)
    sub = reshare(ctx, field, c, t, len(a), rng, mul_by=diff)
    return [ctx.tour_select(x, rows, sub.lam, outer, k, inner, mode, neg) for x, rows in zip(a, sub.rows)], c


def _amax(what: str, neg: bool, ctx, field, xs, outer, k, inner, t, l, rand, rng) -> Shares:
    _parties(what, t, len(xs))
    _axis_check(what, xs, outer, k, inner)
    a = list(xs)
    while k > 1:
        a, _ = _tour_round(ctx, field, a, outer, k, inner, ctx.TOUR_HALVES, neg, t, l, rand, rng)
        k = k // 2 + k % 2
    return a if a[0] is not xs[0] else [x.clone() for x in xs]


def amax(ctx: FieldContext, field, xs: Shares, outer: int, k: int, inner: int, t: int, l: int, rand, rng=None) -> Shares:
    """runtime.np_amax along k of a sharing of the contiguous (outer, k, inner) integer array, for all parties: rounds that
    pair the lower half of the axis with the upper half (an odd leading position has a bye) until one position is left, per
    round
      tour_diff per party: the compact differences a1 - a2 (ffgpu_tour_diff),
      compare_zero(..., mode='lt') on them: shares of [a1 < a2],
      the first 2t+1 parties re-share [a1 < a2] (a1 - a2) (the product inside ffgpu_mul_split_rng),
      tour_select per party: the received sub-shares recombined and subtracted from a1, the bye copied: the next level
      (ffgpu_tour_select).
    Returns shares of the (outer, 1, inner) maxima; xs is not written.

    rand(count) returns (rbits, sbits, rdivl, rzero) as Shares for `count` comparisons of bit length l, as for sort(),
    drawn by the caller per round.

    It is assumed that every difference of two values along k lies in [-2^(l-1), 2^(l-1)), and, as for compare_zero, that
    2^(l+1) + 2^l max(rdivl) < p.  Needs m >= 2t+1 parties."""
    return _amax('amax', True, ctx, field, xs, outer, k, inner, t, l, rand, rng)


def amin(ctx: FieldContext, field, xs: Shares, outer: int, k: int, inner: int, t: int, l: int, rand, rng=None) -> Shares:
    """runtime.np_amin along k: amax() with a2 - a1 compared and [a2 < a1] (a2 - a1) added to a1."""
    return _amax('amin', False, ctx, field, xs, outer, k, inner, t, l, rand, rng)


def _argmax(what: str, neg: bool, ctx, field, xs, outer, k, inner, t, l, rand, rng):
    m = len(xs)
    kk = _parties(what, t, m)
    _axis_check(what, xs, outer, k, inner)
    a, kept = list(xs), []
    while k > 1:                                        # downward: the values, every round's bits kept
        a, c = _tour_round(ctx, field, a, outer, k, inner, ctx.TOUR_ODD_EVEN, neg, t, l, rand, rng)
        kept.append((k, c))
        k = k // 2 + k % 2
    value = a if kept else [x.clone() for x in xs]
    one = ctx.empty(outer * inner)
    one.t.zero_()
    one = ctx.add_scalar(one, 1)                        # the public 1: every party's share of it
    u = [one] * m
    for k, c in reversed(kept):                         # upward: the unit vectors
        if k == 2:                                      # the child is the 1: (1 - c, c) without a multiplication
            u = [ctx.tour_unit_expand(u[j], [c[j]], [1], outer, k, inner) for j in range(m)]
            continue
        sub = reshare(ctx, field, [ctx.tour_unit_prod(u[i], c[i], outer, k, inner) for i in range(kk)], t, m, rng)
        u = [ctx.tour_unit_expand(u[j], sub.rows[j], sub.lam, outer, k, inner) for j in range(m)]
    return u, value


def argmax(ctx: FieldContext, field, xs: Shares, outer: int, k: int, inner: int, t: int, l: int, rand, rng=None):
    """runtime.np_argmax(..., arg_unary=True, arg_only=False) along k of a sharing of the contiguous (outer, k, inner)
    integer array, for all parties.  Downward, rounds as in amax() but pairing neighbours (position n0 + 2j with
    n0 + 2j + 1), so that ties give the first occurrence; every round's comparison bits c are kept.  Upward, from the public
    1, per round
      tour_unit_prod on the first 2t+1 parties: the child's unit vector times c (ffgpu_tour_unit_prod),
      they re-share the product (ffgpu_split_rng),
      tour_unit_expand per party: the received sub-shares recombined to u c, and (u - u c, u c) interleaved
      (ffgpu_tour_unit_expand);
    the round whose child has length 1 needs no multiplication (the reference's n == 2 case).
    Returns (unit, value): shares of the (outer, k, inner) unit vectors, one-hot along k at the first maximum, and of the
    (outer, 1, inner) maxima; xs is not written.  arg_index() turns the unit vectors into positions.

    rand, l and the number of parties: as for amax()."""
    return _argmax('argmax', True, ctx, field, xs, outer, k, inner, t, l, rand, rng)


def argmin(ctx: FieldContext, field, xs: Shares, outer: int, k: int, inner: int, t: int, l: int, rand, rng=None):
    """runtime.np_argmin(..., arg_unary=True, arg_only=False) along k: argmax() for the first minimum."""
    return _argmax('argmin', False, ctx, field, xs, outer, k, inner, t, l, rand, rng)


def arg_index(ctx: FieldContext, unit: Shares, outer: int, k: int, inner: int) -> Shares:
    """The positions the unit vectors of argmax() / argmin() point at: u @ arange(k) along k (runtime.py:3754-3757, 3882-3885),
    local.  Returns shares of the (outer, inner) positions."""
    _axis_check('arg_index', unit, outer, k, inner)
    iv = ctx.from_ints([j % ctx.modulus for j in range(k)])
    if inner == 1:
        return [ctx.matmul(u, iv, outer, k, 1) for u in unit]
    return [ctx.matmul_stack(iv, u, outer, 1, k, inner, 0, k * inner) for u in unit]


def _maximum(what: str, neg: bool, ctx, field, xs, ys, t, l, rand, rng) -> Shares:
    m = len(xs)
    _parties(what, t, m, len(ys))
    n = xs[0].n
    if any(x.n != n for x in xs) or any(y.n != n for y in ys):
        raise ValueError(f'{what}: operands of different lengths')
    diff = [ctx.sub(x, y) if neg else ctx.sub(y, x) for x, y in zip(xs, ys)]
    rbits, sbits, rdivl, rzero = rand(n)
    c = compare_zero(ctx, field, diff, rbits, sbits, rdivl, rzero, t, l, mode='lt', rng=rng)
    v = materialize(ctx, reshare(ctx, field, c, t, m, rng, mul_by=diff))
    return [ctx.sub(x, w) if neg else ctx.add(x, w) for x, w in zip(xs, v)]


def maximum(ctx: FieldContext, field, xs: Shares, ys: Shares, t: int, l: int, rand, rng=None) -> Shares:
    """runtime.np_maximum (runtime.py:3354-3360) of two sharings of equal length, for all parties: x + [x < y] (y - x) as
    x - [x < y] (x - y), one round without a gather, from sub, compare_zero, the re-shared product, recombine and sub.
    rand, l and the number of parties: as for amax(), with x - y for the differences."""
    return _maximum('maximum', True, ctx, field, xs, ys, t, l, rand, rng)


def minimum(ctx: FieldContext, field, xs: Shares, ys: Shares, t: int, l: int, rand, rng=None) -> Shares:
    """runtime.np_minimum (runtime.py:3346-3352): x + [y < x] (y - x)."""
    return _maximum('minimum', False, ctx, field, xs, ys, t, l, rand, rng)


# ---- first occurrence along one axis (runtime.np_find, runtime.py:4603-4698) -----------------------------------
def _find_functions(f, cs_f):
    """(f, cs_f, single) with tuple-valued f and cs_f, as the reference normalises them (runtime.py:4641-4663); single: the
    caller's function is int-valued and one Shares comes back instead of a tuple."""
    if cs_f is None:
        if f is None:
            return (lambda i: (i,)), (lambda b, i: (i + b,)), True
        single = isinstance(f(0), int)
        g = (lambda i: (f(i),)) if single else (lambda i: tuple(f(i)))
        return g, (lambda b, i: tuple(b * (y - x) + x for x, y in zip(g(i), g(i + 1)))), single           # (**), runtime.py:4521
    single = isinstance(cs_f(0, 0), int)
    cs = (lambda b, i: (cs_f(b, i),)) if single else (lambda b, i: tuple(cs_f(b, i)))
    if f is None:
        return (lambda i: cs(0, i)), cs, single
    return ((lambda i: (f(i),)) if isinstance(f(0), int) else (lambda i: tuple(f(i)))), cs, single


def _find_root(ctx: FieldContext, field, b: Shares, tab: DevArray, outer: int, k: int, inner: int, C: int, flip: int, virt: int, t: int,
               rng) -> Shares:
    """The rounds of find() over the k + virt >= 2 leaves: every party's root (C, outer, 1, inner), component 0 = nf."""
    m = len(b)
    kk = _parties('find', t, m)
    sub = reshare(ctx, field, [ctx.find_leaf_prod(b[i], tab, outer, k, inner, C, flip, virt) for i in range(kk)], t, m, rng)
    level = [ctx.find_leaf_apply(b[j], tab, sub.rows[j], sub.lam, outer, k, inner, C, flip, virt) for j in range(m)]
    kp = (k + virt) // 2 + (k + virt) % 2
    while kp > 1:
        sub = reshare(ctx, field, [ctx.find_prod(level[i], outer, kp, inner, C) for i in range(kk)], t, m, rng)
        level = [ctx.tour_select(level[j], sub.rows[j], sub.lam, C * outer, kp, inner, ctx.TOUR_ODD_EVEN) for j in range(m)]
        kp = kp // 2 + kp % 2
    return level


def find(ctx: FieldContext, field, xs: Shares, outer: int, k: int, inner: int, t: int, s: int = 0, e='k', f=None, cs_f=None,
         bits: bool = True, l: Optional[int] = None, rand=None, rng=None):
    """runtime.np_find along k of a sharing of the contiguous (outer, k, inner) array, for all parties: the index ix of the
    first occurrence of the public s, or f(ix).  s in {0, 1} on shared bits (bits=True); bits=False is for a public integer
    s and arbitrary l-bit integers: [a == s] = compare_zero(a - s, mode='eq') with rand(outer * k * inner) as for sort() /
    amax() is searched for its first 1 -- the complement of the reference's `a != s`, so no extra gate.

    f, cs_f and e have the reference's meaning: cs_f(b, i) = f(i + b) for a bit b is the conditional step, derived from f by
    (**) of runtime.py:4521 when only f is given; e is the index when s does not occur, a string e an expression in k
    (default 'k'); e=None returns the raw pair (nf, values) with nf = 1 where s does not occur.  An int-valued f / cs_f gives
    one Shares, a tuple-valued one (up to four values) a tuple of Shares, each (outer, inner).

    The tree pairs neighbours (position n0 + 2j with n0 + 2j + 1; the combine L + nf_L (R - L) is associative), and the value
    for "not found" is the public leaf (1, f(e)) at position k, so the root is the answer after bit_length(k) rounds (raw:
    bit_length(k - 1)) instead of the reference's ceil(log2 k) + 1.  Per round
      the product nf_L (R - L) on the first 2t+1 parties (ffgpu_find_leaf_prod, the leaves computed from the bits in
      registers, in the first round; ffgpu_find_prod later),
      they re-share it (ffgpu_split_rng),
      the received sub-shares recombined and added to L, the bye carried over, per party (ffgpu_find_leaf_apply;
      ffgpu_tour_select on the components as rows later).
    k == 1 with e=None has no round.  Needs m >= 2t+1 parties; xs is not written."""
    _parties('find', t, len(xs))
    _axis_check('find', xs, outer, k, inner)
    if not isinstance(s, int) or (bits and s not in (0, 1)):
        raise ValueError('find: s is a public integer, 0 or 1 for bits')
    f_, cs, single = _find_functions(f, cs_f)
    if isinstance(e, str):
        e = eval(e, {'__builtins__': {}}, {'k': k})
    cs0, cs1 = [cs(0, j) for j in range(k)], [cs(1, j) for j in range(k)]
    fe = None if e is None else f_(e)
    nval = len(cs0[0])
    if not 1 <= nval <= ctx.FIND_MAX_VALUES:
        raise ValueError(f'find: 1 to {ctx.FIND_MAX_VALUES} values per index')
    C, p = 1 + nval, ctx.modulus
    if bits:
        b, flip = list(xs), s
    else:
        if l is None or rand is None:
            raise ValueError('find: bits=False compares: l and rand are needed')
        rbits, _, rdivl, _ = rand(outer * k * inner)
        b = compare_zero(ctx, field, [ctx.add_scalar(x, -s % p) for x in xs], rbits, None, rdivl, None, t, l, mode='eq', rng=rng)
        flip = 1
    virt = 0 if e is None else 1
    plane = outer * inner
    if k + virt == 1:                                   # one leaf, no round: (b', cs_f(0, 0) + b' (cs_f(1, 0) - cs_f(0, 0)))
        nf = [ctx.rsub_scalar(x, 1) if flip else x.clone() for x in b]
        vals = [[ctx.add_scalar(ctx.mul_scalar(x, (cs1[0][q] - cs0[0][q]) % p), cs0[0][q] % p) for x in nf] for q in range(nval)]
        return nf, (vals[0] if single else tuple(vals))
    level = _find_root(ctx, field, b, ctx.find_table(k, cs0, cs1, fe), outer, k, inner, C, flip, virt, t, rng)
    comp = lambda q: [_rows(ctx, x, q, q + 1, plane) for x in level]                          # views of the root (C, outer, 1, inner)
    vals = [comp(1 + q) for q in range(nval)]
    y = vals[0] if single else tuple(vals)
    return (comp(0), y) if e is None else y


# ---- fixed point: truncation, product, normalisation, reciprocal and division (runtime.np_trunc, runtime.py:839-873;
# _norm, _rec, runtime.py:4718-4745; np_divide) ----------------------------------------------------------------------
# All on RAW integers: a fixed-point number with f fractional bits and bit length l is the shared field element
# a = round(x 2^f), -2^(l-1) <= a < 2^(l-1).
def trunc(ctx: FieldContext, field, xs: Shares, rbits: Shares, rdivf: Shares, t: int, f: int, L: int) -> Shares:
    """runtime.np_trunc for all parties: shares of floor(a / 2^f) or of that plus one (the reference's probabilistic
    rounding), from trunc_mask per party (ffgpu_trunc_mask: ar = a + r and the masked value ar + 2^(L-1) + 2^f R) and
    trunc_finish per party on the masked shares of the first t+1 parties (ffgpu_trunc_finish: the opening in registers,
    (ar - (c mod 2^f)) 2^-f).  The integer is fixed by the randomness: (a + r - ((a + 2^(L-1) + r + 2^f R) mod 2^f)) / 2^f
    with r the value of the random bits and R of rdivf.

    rbits: n*f random bits per party (element-major, least significant first), rdivf: n random values below the statistical
    bound.  The caller guarantees |a| < 2^(L-1) and that the opened value a + 2^(L-1) + r + 2^f R stays below p.  xs is
    not written."""
    m = len(xs)
    if m < t + 1:
        raise ValueError('truncation opens a degree-t sharing: m >= t+1 parties')
    n = xs[0].n
    if any(x.n != n for x in xs) or len(rbits) != m or len(rdivf) != m or any(r.n != n * f for r in rbits):
        raise ValueError('trunc: n values, n*f bit shares and n high masks per party')
    lam = _lagrange(field, range(1, t + 2))
    am = [ctx.trunc_mask(xs[j], rbits[j], rdivf[j], f, 1 << (L - 1)) for j in range(m)]
    return [ctx.trunc_finish([am[i][1] for i in range(t + 1)], lam, am[j][0], f) for j in range(m)]


def fxp_multiply(ctx: FieldContext, field, xs: Shares, ys: Shares, t: int, f: int, l: int, rand_trunc, rng=None) -> Shares:
    """The product of two fixed-point sharings (runtime.np_multiply with frac_length f): multiply() -- the product inside
    the share generation, then the recombination -- and trunc() by f bits with L = l + f.

    rand_trunc(count, f) returns (rbits, rdivf) as Shares for `count` truncations by f bits: count * f random bits
    (element-major, least significant first) and count values below the statistical bound, drawn by the caller per
    truncation.  The caller guarantees |x y| < 2^(l+f-1) on the raw integers and, as for trunc(), that the opened value does
    not wrap.  Needs m >= 2t+1 parties."""
    prod = multiply(ctx, field, xs, ys, t, rng)
    rbits, rdivf = rand_trunc(xs[0].n, f)
    return trunc(ctx, field, prod, rbits, rdivf, t, f, l + f)


def norm(ctx: FieldContext, field, xs: Shares, t: int, l: int, f: int, rand_bits, rng=None) -> Shares:
    """runtime._norm for all parties: the signed normalisation factor v = (2s - 1) 2^(i + 2f - l + 1) with s the inverted
    sign bit and i the number of leading bits below the sign bit that differ from s (i = l - 1 if all do), so that a v lies
    in [2^(2f-1), 2^2f] -- 1/2 <= x v <= 1 after the truncation.  Steps:
      to_bits (l bits, least significant first),
      norm_prod on the first 2t+1 parties: (1 - 2s) times the bits below the sign bit, reversed (ffgpu_norm_prod),
      they re-share it (ffgpu_split_rng),
      norm_apply per party: s + (1 - 2s) x with the recombination folded in (ffgpu_norm_apply),
      find(..., s=0, e=l-1, cs_f=lambda b, i: (b+1) << i) along the l - 1 bits: shares of 2^i,
      one multiply() with 2s - 1 and the public factor 2^(2f-l+1).

    rand_bits(count, l) returns (rbits, rdivl) as Shares: the inputs of to_bits().  Requires f <= l <= 2f + 1.  Needs
    m >= 2t+1 parties; xs is not written."""
    if not (f <= l <= 2 * f + 1) or l < 2:
        raise ValueError('norm: f <= l <= 2f + 1 and l >= 2')
    m = len(xs)
    kk = _parties('norm', t, m)
    n = xs[0].n
    rbits, rdivl = rand_bits(n, l)
    bits = to_bits(ctx, field, xs, rbits, rdivl, t, l, rng=rng)
    ps = [ctx.norm_prod(bits[i], l) for i in range(kk)]
    sub = reshare(ctx, field, [p[0] for p in ps], t, m, rng)
    x = [ctx.norm_apply(bits[j], sub.rows[j], sub.lam, l) for j in range(m)]
    nf = find(ctx, field, x, n, l - 1, 1, t, s=0, e=l - 1, cs_f=lambda b, i: (b + 1) << i, rng=rng)
    v = multiply(ctx, field, nf, [p[1] for p in ps], t, rng)
    return [ctx.mul_scalar(w, 1 << (2 * f - l + 1)) for w in v]


def reciprocal(ctx: FieldContext, field, xs: Shares, t: int, l: int, f: int, rand_bits, rand_trunc, rng=None) -> Shares:
    """runtime._rec for all parties: b = a v with v = norm(a), c = 2.9142135623731 - 2b, theta = ceil(log2((f+1)/3.54))
    Newton steps c <- c (2 - c b), and c v; every product is fxp_multiply().

    The caller guarantees a != 0 and a representable reciprocal, |a| > 2^(2f-l+1) on the raw integers.  rand_bits and
    rand_trunc: as for norm() and fxp_multiply().  Needs m >= 2t+1 parties."""
    import math
    mul = lambda a, b: fxp_multiply(ctx, field, a, b, t, f, l, rand_trunc, rng)
    v = norm(ctx, field, xs, t, l, f, rand_bits, rng)
    b = mul(xs, v)
    c = [ctx.rsub_scalar(ctx.mul_scalar(x, 2), round(2.9142135623731 * 2**f)) for x in b]
    for _ in range(int(math.ceil(math.log2((f + 1) / 3.54)))):
        cb = mul(c, b)
        c = mul(c, [ctx.rsub_scalar(x, 1 << (f + 1)) for x in cb])
    return mul(c, v)


def divide(ctx: FieldContext, field, num: Shares, den: Shares, t: int, l: int, f: int, rand_bits, rand_trunc, rng=None) -> Shares:
    """runtime.np_divide of two fixed-point sharings for all parties: fxp_multiply(reciprocal(den), num).

    The caller guarantees den != 0 and a representable reciprocal, |den| > 2^(2f-l+1) on the raw integers."""
    return fxp_multiply(ctx, field, reciprocal(ctx, field, den, t, l, f, rand_bits, rand_trunc, rng), num, t, f, l, rand_trunc, rng)


# ---- the same layer with ALL parties in every launch ---------------------------------------------------------
# The per-party functions above issue one launch per party and step (what each MPyC party does in its own
# process).  When all m parties of a computation sit on one GPU the parties' launches of a step are identical
# up to pointers, so they become grid rows of ONE launch: shares of all parties are the rows of one DevMatrix,
# sub-shares live in an (m * k)-row block used as [recipient][sender], and a layer of the x^254 chain is one
# ffgpu_gate_rng_batch.  The two local steps around the opening inside np_to_bits are one kernel each
# (ffgpu_gf256_mask_open, ffgpu_gf256_bits_affine_fold).  13 launches per S-box layer instead of 49.
def as_matrix(ctx: FieldContext, xs: Shares):
    """The parties' shares as the rows of one DevMatrix: a view when they already are equally spaced rows of one
    allocation (what share() / split return), else a copy."""
    import torch
    from .engine import DevMatrix, limbs_of
    m, n, eb = len(xs), xs[0].n, ctx.elem_bytes
    unit = xs[0].t.element_size()                     # bytes of one tensor element (8 for the 16- and 24-byte layouts)
    step = (xs[1].ptr - xs[0].ptr) if m > 1 else 0
    lb = limbs_of(eb)
    same_storage = all(x.t.untyped_storage().data_ptr() == xs[0].t.untyped_storage().data_ptr() for x in xs)
    if m > 1 and same_storage and step > 0 and step % eb == 0 and step // eb >= n and \
            all(xs[i].ptr - xs[0].ptr == i * step for i in range(m)) and all(x.n == n for x in xs) and \
            xs[0].t.storage_offset() * unit + (m - 1) * step + n * eb <= xs[0].t.untyped_storage().nbytes():
        stride = step // eb
        shape, strides = ((m, stride, lb), (stride * lb, lb, 1)) if lb else ((m, stride), (stride, 1))
        span = xs[0].t.storage_offset() + ((m - 1) * stride + stride) * (lb or 1)
        if span * unit <= xs[0].t.untyped_storage().nbytes():
            return DevMatrix(ctx, torch.as_strided(xs[0].t, shape, strides, xs[0].t.storage_offset()), m, n, stride)
    mtx = ctx.empty_matrix(m, n)
    for i, x in enumerate(xs):
        mtx.row(i).t.copy_(x.t)
    return mtx


class _Block:
    """Pending for the all-parties layout: the sub-shares of one re-sharing round as ONE [recipient][sender] block, row
    j * k + s of `mtx` = the sub-share sender s+1 dealt to party j+1.  `rows` and `lam` read as Pending's; rows_of(j) is
    rows[j] without the other parties' views."""

    __slots__ = ('mtx', 'k', 'lam')

    def __init__(self, mtx, k, lam):
        self.mtx, self.k, self.lam = mtx, k, lam

    def rows_of(self, j: int):
        return [self.mtx.row(j * self.k + s) for s in range(self.k)]

    @property
    def rows(self):
        return [self.rows_of(j) for j in range(self.mtx.rows // self.k)]


def _gate_all(ctx: FieldContext, x, y, t: int, m: int, lam, rng):
    """One secure multiplication (runtime.py:1096-1141 + :603-689) for all parties: the k = 2t+1 senders recombine
    their factors (pending _Blocks or plain share matrices), multiply and re-share in ONE launch."""
    k = 2 * t + 1

    def operand(v):
        if isinstance(v, _Block):
            return v.rows_of(0), v.lam, v.k * v.mtx.stride
        return [v.row(0)], [1], v.stride
    ra, la, sa = operand(x)
    rb, lb, sb = (None, None, 0) if y is x else operand(y)
    n = ra[0].n
    out = ctx.empty_matrix(m * k, n)
    ctx.gate_batch(ra, la, sa, rb, lb, sb, t, m, k, out, k, state=rng)
    return _Block(out, k, lam)


def sbox_layer_all(ctx: FieldContext, field, xs, rbits, t: int, A: Sequence[Sequence[int]], B: Sequence[int], rng=None,
                   fused: bool = True):
    """sbox_layer() with all parties in every launch (see above): xs / rbits are Shares lists or DevMatrix (one row
    per party); returns a DevMatrix of the parties' shares of S-box(x).  GF(2^8), t <= 3.  fused (default): the
    whole layer as ONE kernel (ffgpu_gf256_sbox_layer) where it applies; fused=False: the 13-launch composition
    (11 batched chain gates + masked opening + bits/affine/fold)."""
    from .engine import DevMatrix
    X = xs if isinstance(xs, DevMatrix) else as_matrix(ctx, xs)
    R = rbits if isinstance(rbits, DevMatrix) else as_matrix(ctx, rbits)
    m = X.rows
    k = _parties('the S-box layer', t, m, R.rows)
    lam = _lagrange(field, range(1, k + 1))
    if fused and ctx.elem_bytes == 1:
        # everything below is element-wise: one kernel carries the parties' shares through the whole layer in registers
        try:
            out = ctx.gf256_sbox_layer(X, R, t, lam, _lagrange(field, range(1, t + 2)), A, B, state=rng)
            if rng is not None:
                rng.commit()
            return out
        except NotImplementedError:
            pass                                        # shape not covered: per-step kernels
    y = _pow254_chain(lambda a, b: _gate_all(ctx, a, b, t, m, lam, rng), X)    # pending: party j holds sum_s lam[s] * y.rows_of(j)[s]
    mu = _lagrange(field, range(1, t + 2))              # opening from the first t+1 parties (runtime.py:582-585)
    rows, coefs = [], []
    for p in range(t + 1):
        for s, r in enumerate(y.rows_of(p)):
            rows.append(r)
            coefs.append(int(field(mu[p]) * field(lam[s])))
    if rng is not None:
        rng.commit()                                    # one nonce update for the 11 gates (deferred advance)
    opened = ctx.gf256_mask_open(rows, coefs, [R.row(p) for p in range(t + 1)], mu[:t + 1])
    return ctx.gf256_bits_affine_fold(opened, R, A, B)


def sbox_layer(ctx: FieldContext, field, xs: Shares, rbits: Shares, t: int, A: Sequence[Sequence[int]],
               B: Sequence[int], fused: bool = True, rng=None, chain: bool = True) -> Shares:
    """The AES S-box on secret-shared bytes, as demos/np_aes.py:37-43:
    x = np_to_bits(x**254); x = A @ x + B over GF(2) (on bit shares, local); x = np_from_bits(x)."""
    y = pow254_fused(ctx, field, xs, t, rng) if chain and t <= 3 else pow254(ctx, field, xs, t, rng)
    bits = to_bits_gf256(ctx, field, y, rbits, t)
    if fused:
        return [ctx.bit_affine(b, A, B, from_bits=True) for b in bits]           # both local steps in one pass
    bits = [ctx.group_matvec(b, A, B) for b in bits]
    return from_bits(ctx, bits)


def _sbox_any(ctx: FieldContext, field, xs: Shares, rbits: Shares, t: int, A, B, rng) -> Shares:
    """S-box layer for the AES functions below: all parties per launch when the fused chain applies (t <= 3)."""
    if t <= 3:
        out = sbox_layer_all(ctx, field, xs, rbits, t, A, B, rng)
        return [out.row(i) for i in range(out.rows)]
    return sbox_layer(ctx, field, xs, rbits, t, A, B, rng=rng)


# ---- AES-128 on secret-shared blocks (demos/np_aes.py:55-86) ------------------------------------------
# Layout: position-major.  A batch of nblk blocks is ONE array of 16*nblk bytes per party; byte position
# p = r + 4c of the AES state s[r][c] (= input byte p of the block, FIPS-197 sec. 3.4) occupies
# buf[p*nblk : (p+1)*nblk].  SubBytes is then one S-box layer over the whole array, ShiftRows is a relabelling
# of row views (no data movement) and MixColumns is the small-public-matrix-times-rows kernel
# (ffgpu_recombine with w = k = 4, finfields.py:1126-1146 `C @ s`).
_MIX = [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]          # circulant([2, 3, 1, 1]), np_aes.py:33


def _xpow(modulus: int, k: int) -> int:
    """x^k in GF(2)[x] / modulus (bit patterns)."""
    v, deg = 1, modulus.bit_length() - 1
    for _ in range(k):
        v <<= 1
        if v >> deg:
            v ^= modulus
    return v


def _row(ctx: FieldContext, buf: DevArray, p: int, nblk: int) -> DevArray:
    return DevArray(ctx, buf.t[p * nblk:(p + 1) * nblk], nblk)


def _cat(ctx: FieldContext, rows: Sequence[DevArray]) -> DevArray:
    import torch
    t = torch.cat([r.t for r in rows])
    return DevArray(ctx, t, t.shape[0])


def aes128_key_expansion(ctx: FieldContext, field, key: Shares, nblk: int, rbits_fn, t: int, A, B, rng=None):
    """key_expansion for Nk = 4 (np_aes.py:55-72).  key: 16*nblk bytes per party (one key per block,
    position-major).  Returns the 11 round keys, each a Shares of 16*nblk bytes.  rbits_fn(nbytes) supplies
    shares of 8*nbytes random bits (np_random_bits) for each S-box call."""
    m = len(key)
    w = [[[_row(ctx, key[i], r + 4 * c, nblk) for r in range(4)] for i in range(m)] for c in range(4)]   # w[c][party][r]
    for i in range(4, 44):
        prev = w[i - 1]
        if i % 4 == 0:
            sub = _sbox_any(ctx, field, [_cat(ctx, prev[pi]) for pi in range(m)], rbits_fn(4 * nblk), t, A, B, rng)
            tcol = [[_row(ctx, sub[pi], (r + 1) % 4, nblk) for r in range(4)] for pi in range(m)]        # RotWord
            rcon = _xpow(ctx.modulus, i // 4 - 1)                   # f256(1) << i//Nk - 1  (np_aes.py:67)
            for pi in range(m):
                tcol[pi][0] = ctx.add_scalar(tcol[pi][0], rcon)                                          # every party adds the public constant
        else:
            tcol = prev
        w.append([[ctx.add(tcol[pi][r], w[i - 4][pi][r]) for r in range(4)] for pi in range(m)])
    return [[_cat(ctx, [w[4 * j + c][pi][r] for c in range(4) for r in range(4)]) for pi in range(m)] for j in range(11)]


def aes128_encrypt(ctx: FieldContext, field, K, state: Shares, nblk: int, rbits_fn, t: int, A, B, rng=None) -> Shares:
    """encrypt (np_aes.py:75-86): AddRoundKey, 9 x (SubBytes, ShiftRows, MixColumns, AddRoundKey), final round
    without MixColumns.  state: 16*nblk bytes per party, position-major."""
    from .engine import DevMatrix
    m = len(state)
    lam = [v for row in _MIX for v in row]
    s = [ctx.add(state[pi], K[0][pi]) for pi in range(m)]
    for rnd in range(1, 11):
        s = _sbox_any(ctx, field, s, rbits_fn(16 * nblk), t, A, B, rng)
        nxt = []
        for pi in range(m):
            # ShiftRows: s'[r][c] = s[r][(c + r) % 4]  (np.roll(s[r], -r))
            shifted = lambda r, c: _row(ctx, s[pi], r + 4 * ((c + r) % 4), nblk)
            if rnd < 10:
                out = ctx.empty(16 * nblk)
                for c in range(4):
                    view = DevMatrix(ctx, out.t[4 * c * nblk:(4 * c + 4) * nblk].view(4, nblk), 4, nblk, nblk)
                    ctx.recombine([shifted(k, c) for k in range(4)], lam, w=4, out=view)                 # C @ column c
            else:
                out = _cat(ctx, [shifted(r, c) for c in range(4) for r in range(4)])
            nxt.append(ctx.add(out, K[rnd][pi]))
        s = nxt
    return s


# ---- inverse cipher (demos/np_aes.py:46-52, 89-99) ------------------------------------------------------
_MIX_INV = [[14, 11, 13, 9], [9, 14, 11, 13], [13, 9, 14, 11], [11, 13, 9, 14]]     # np.linalg.inv(C), np_aes.py:34


def _gf2_inverse(A: Sequence[Sequence[int]]) -> List[List[int]]:
    """Inverse of an 8x8 0/1 matrix over GF(2) (np.linalg.inv(A), np_aes.py:31): host scalars."""
    n = len(A)
    M = [list(r) + [int(i == j) for j in range(n)] for i, r in enumerate(A)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c])
        M[c], M[p] = M[p], M[c]
        for r in range(n):
            if r != c and M[r][c]:
                M[r] = [x ^ y for x, y in zip(M[r], M[c])]
    return [row[n:] for row in M]


def sbox1_layer(ctx: FieldContext, field, xs: Shares, rbits: Shares, t: int, A, B, rng=None) -> Shares:
    """AES inverse S-box on secret-shared bytes (np_aes.py:46-52): x = np_to_bits(x); x += B; x = A1 @ x;
    x = np_from_bits(x) ** 254.  The two local steps are one pass: A1 (x + B) = A1 x + A1 B."""
    A1 = _gf2_inverse(A)
    bias = [0] * 8
    for r in range(8):
        for c in range(8):
            bias[r] ^= A1[r][c] & B[c]
    bits = to_bits_gf256(ctx, field, xs, rbits, t)
    y = [ctx.bit_affine(b, A1, bias, from_bits=True) for b in bits]
    return pow254(ctx, field, y, t, rng)


def aes128_decrypt(ctx: FieldContext, field, K, state: Shares, nblk: int, rbits_fn, t: int, A, B, rng=None) -> Shares:
    """decrypt (np_aes.py:89-99): for i = 10..1: AddRoundKey(K[i]); InvMixColumns unless i = 10; InvShiftRows;
    InvSubBytes; finally AddRoundKey(K[0]).  Same position-major layout as aes128_encrypt."""
    from .engine import DevMatrix
    m = len(state)
    lam = [v for row in _MIX_INV for v in row]
    s = list(state)
    for rnd in range(10, 0, -1):
        nxt = []
        for pi in range(m):
            x = ctx.add(s[pi], K[rnd][pi])
            if rnd < 10:
                mixed = ctx.empty(16 * nblk)
                for c in range(4):
                    view = DevMatrix(ctx, mixed.t[4 * c * nblk:(4 * c + 4) * nblk].view(4, nblk), 4, nblk, nblk)
                    ctx.recombine([_row(ctx, x, k + 4 * c, nblk) for k in range(4)], lam, w=4, out=view)     # C1 @ column c
                x = mixed
            # InvShiftRows: s'[r][c] = s[r][(c - r) % 4]  (np.roll(s[r], r))
            nxt.append(_cat(ctx, [_row(ctx, x, r + 4 * ((c - r) % 4), nblk) for c in range(4) for r in range(4)]))
        s = sbox1_layer(ctx, field, nxt, rbits_fn(16 * nblk), t, A, B, rng=rng)
    return [ctx.add(s[pi], K[0][pi]) for pi in range(m)]


# ---- fixed point: logarithm, exponential and powers (runtime.np_vander, runtime.py:4947-4977; np_log, np_log2, np_log10,
# np_exp2, np_exp, runtime.py:4853-4945; _np_pow_public_int_base_secret_integral_exponent, runtime.py:1389-1425) -----------------
# On RAW integers as above.  A public float c enters a product as the reference's np_multiply takes it (runtime.py:1114-1140):
# b = round(c 2^f) loses its z <= f trailing zero bits, the product is truncated by f - z bits.
def _public_float(c: float, f: int):
    """(b >> z, f - z) for the public float c: the integer factor and the bits to truncate afterwards"""
    b = round(c * 2**f)
    z = max(0, min(f, (b & -b).bit_length() - 1))
    return b >> z, f - z


def _mul_public_float(ctx: FieldContext, field, xs: Shares, c: float, t: int, f: int, l: int, rand_trunc) -> Shares:
    b, shift = _public_float(c, f)
    prod = [ctx.mul_scalar(x, b % ctx.modulus) for x in xs]
    if shift == 0:
        return prod
    rbits, rdivf = rand_trunc(xs[0].n, shift)
    return trunc(ctx, field, prod, rbits, rdivf, t, shift, l + shift)


def taylor_log_degree(f: int) -> int:
    """runtime._taylor_log_degree (runtime.py:4855-4863): the degree k with 1/(k+1) w^-(k+1) <= 2^-f, w = 1/(sqrt 2 - 1)"""
    import math
    w = 1 / (math.sqrt(2) - 1)
    k = f - 1
    while math.log2(k) + k * math.log2(w) >= f:
        k -= 1
    return k


def taylor_exp2_degree(f: int) -> int:
    """runtime._taylor_exp2_degree (runtime.py:4903-4911)"""
    import math
    log2ln2 = math.log2(math.log(2))
    k = 1
    log2factorial = 1
    while log2factorial - (k + 1) * log2ln2 < f + 1:
        k += 1
        log2factorial += math.log2(k + 1)
    return k


def power_ladder(N: int):
    """The rounds (h, w) of np_vander's doubling recursion f(N) (runtime.py:4959-4968), first round first: from the powers
    y^1..y^h, y^h times the w lowest gives y^(h+1)..y^(h+w); h = ceil(n/2) and w = n - h at every level n of the recursion."""
    if N <= 1:
        return []
    h = (N + 1) // 2
    return power_ladder(h) + [(h, N - h)]


def powers(ctx: FieldContext, field, ys: Shares, N: int, t: int, f: int, l: int, rand_trunc, rng=None) -> Shares:
    """The columns y^1..y^N of runtime.np_vander for a fixed-point sharing, for all parties: every party's POWER-MAJOR (N, n)
    block, row j = y^(j+1).  The rounds are exactly those of the reference's recursion (power_ladder) -- which power
    multiplies which fixes every rounding.  Per round (h, w)
      powers_prod on the first 2t+1 parties: y^h times the w lowest powers (ffgm_powers_prod),
      they re-share it (ffgpu_split_rng) and every party recombines into rows h.. of its block,
      trunc() by f bits with L = l + f over the w n new elements.
    rand_trunc: as for fxp_multiply().  Needs m >= 2t+1 parties; ys is not written."""
    m = len(ys)
    kk = _parties('powers', t, m)
    n = ys[0].n
    if N < 1 or any(y.n != n for y in ys):
        raise ValueError('powers: N >= 1 and shares of one length')
    blocks = [ctx.empty(N * n) for _ in range(m)]
    for b, y in zip(blocks, ys):
        _rows(ctx, b, 0, 1, n).t.copy_(y.t)
    for h, w in power_ladder(N):
        sub = reshare(ctx, field, [ctx.powers_prod(blocks[i], n, h, w) for i in range(kk)], t, m, rng)
        new = [_rows(ctx, b, h, h + w, n) for b in blocks]
        for j in range(m):
            ctx.recombine(sub.rows[j], sub.lam, out=new[j])
        rbits, rdivf = rand_trunc(w * n, f)
        for v, r in zip(new, trunc(ctx, field, new, rbits, rdivf, t, f, l + f)):
            v.t.copy_(r.t)
    return blocks


def _taylor(ctx: FieldContext, field, ys: Shares, coefs, c0: int, t: int, f: int, l: int, rand_trunc, rng) -> Shares:
    """c0 + sum_j coefs[j] y^(j+1) on raw integers, truncated by f bits: powers(), one poly_dot per party, one trunc()."""
    n = ys[0].n
    blocks = powers(ctx, field, ys, len(coefs), t, f, l, rand_trunc, rng)
    tab = ctx.poly_table(coefs)
    acc = [ctx.poly_dot(b, n, tab, c0) for b in blocks]
    rbits, rdivf = rand_trunc(n, f)
    return trunc(ctx, field, acc, rbits, rdivf, t, f, l + f)


def log(ctx: FieldContext, field, xs: Shares, t: int, l: int, f: int, rand_bits, rand_trunc, rng=None) -> Shares:
    """runtime.np_log for all parties: the natural logarithm of a fixed-point sharing, a > 0.  Steps:
      to_bits of the l - 1 bits below the sign bit, bits_reverse (ffgm_bits_reverse),
      find(..., s=1, cs_f=lambda b, i: (i+1+b, (b+1) << i)): k = 1 + the number of leading zeros and v = 2^(k-1),
      v scaled by the public 2^(2f-l+1) (2^(f-l+1) as a fixed-point number), b = fxp_multiply(a, v) in [1/2, 1),
      y = b - round(2^f / sqrt 2), the Taylor polynomial of degree taylor_log_degree(f) in y around 1/sqrt 2: powers(),
      poly_dot with the coefficients round(c_i 2^f) and the constant round(log(1/sqrt 2) 2^f) 2^f (ffgm_poly_dot), one trunc(),
      minus (k - f) round(log 2 * 2^f), local.
    rand_bits and rand_trunc: as for norm() and fxp_multiply().  Requires f + 2 <= l <= 2f + 1 (below, the reference takes an
    integral path without truncation; above, its scale factor rounds to 0).  Needs m >= 2t+1 parties; xs is not written."""
    import math
    import numpy as np
    if not f + 2 <= l <= 2 * f + 1:
        raise ValueError('log: f + 2 <= l <= 2f + 1')
    m = len(xs)
    _parties('log', t, m)
    n = xs[0].n
    if any(x.n != n for x in xs):
        raise ValueError('log: shares of one length')
    p = ctx.modulus
    rbits, rdivl = rand_bits(n, l - 1)
    bits = to_bits(ctx, field, xs, rbits, rdivl, t, l - 1, offset=1 << l, rng=rng)
    rev = [ctx.bits_reverse(b, l - 1) for b in bits]
    k, v = find(ctx, field, rev, n, l - 1, 1, t, s=1, cs_f=lambda b, i: (i + 1 + b, (b + 1) << i), rng=rng)
    v = [ctx.mul_scalar(x, 1 << (2 * f - l + 1)) for x in v]
    b = fxp_multiply(ctx, field, xs, v, t, f, l, rand_trunc, rng)
    alpha = 0.5 * math.sqrt(2)
    y = [ctx.add_scalar(x, -round(alpha * 2**f) % p) for x in b]
    i = np.arange(1, taylor_log_degree(f) + 1)
    coefs = [int(c) for c in np.vectorize(round, otypes='O')((-1 / (i * (-alpha)**i)) * 2**f)]
    c = _taylor(ctx, field, y, coefs, (round(math.log(alpha) * 2**f) << f) % p, t, f, l, rand_trunc, rng)
    ln2, _ = _public_float(math.log(2), f)
    ln2 <<= f - _
    # c - (k - f) ln2 = c + f ln2 - k ln2
    return [ctx.add_scalar(ctx.sub(cj, ctx.mul_scalar(kj, ln2 % p)), f * ln2 % p) for cj, kj in zip(c, k)]


def log2(ctx: FieldContext, field, xs: Shares, t: int, l: int, f: int, rand_bits, rand_trunc, rng=None) -> Shares:
    """runtime.np_log2: log() times the public float log2(e)."""
    import math
    return _mul_public_float(ctx, field, log(ctx, field, xs, t, l, f, rand_bits, rand_trunc, rng), math.log2(math.e), t, f, l, rand_trunc)


def log10(ctx: FieldContext, field, xs: Shares, t: int, l: int, f: int, rand_bits, rand_trunc, rng=None) -> Shares:
    """runtime.np_log10: log() times the public float log10(e)."""
    import math
    return _mul_public_float(ctx, field, log(ctx, field, xs, t, l, f, rand_bits, rand_trunc, rng), math.log10(math.e), t, f, l, rand_trunc)


def _pow_public_base(ctx: FieldContext, field, g: int, bs: Shares, t: int, l: int, shift: int, rand_exp, rng, sec_param: int) -> Shares:
    """Shares of g^(b >> shift) as plain integers (not scaled by 2^f), b a multiple of 2^shift."""
    m = len(bs)
    _parties('pow_public_base', t, m)
    n = bs[0].n
    if any(b.n != n for b in bs):
        raise ValueError('pow_public_base: shares of one length')
    p = ctx.modulus
    rbound = 1 << (l + sec_param) // (t + 1)
    rs = rand_exp(n, rbound)
    if len(rs) != t + 1 or any(r.n != n for r in rs):
        raise ValueError('pow_public_base: t+1 senders draw n exponents each')
    rbits = max(1, (rbound - 1).bit_length())
    inv_tab = ctx.pow_table(pow(g, -1, p), rbits)
    r_sh = [share(ctx, r, t, m, rng) for r in rs]
    gr_sh = [share(ctx, ctx.pow_base(r, inv_tab, rbits), t, m, rng) for r in rs]
    rsum, gr = r_sh[0], gr_sh[0]
    for i in range(1, t + 1):
        rsum = [ctx.add(a, b) for a, b in zip(rsum, r_sh[i])]
        gr = multiply(ctx, field, gr, gr_sh[i], t, rng)
    masked = [ctx.add(b, ctx.mul_scalar(r, (1 << shift) % p)) for b, r in zip(bs[:t + 1], rsum)]
    c = open_(ctx, field, masked, t)
    ebits = max(l - shift, rbits + (t + 1).bit_length()) + 1
    if ebits > p.bit_length():
        raise ValueError('pow_public_base: the masked exponent does not fit the field')
    gc = ctx.pow_base(c, ctx.pow_table(g, ebits), ebits, shift=shift)
    return [ctx.mul(gc, x) for x in gr]


def pow_public_base(ctx: FieldContext, field, g: int, bs: Shares, t: int, l: int, f: int, rand_exp, rng=None,
                    sec_param: int = 30) -> Shares:
    """runtime._np_pow_public_int_base_secret_integral_exponent for all parties: g^b for a public integer g and a sharing of
    nonnegative INTEGRAL fixed-point exponents (raw b = B 2^f); the result g^B 2^f is exact.  Steps:
      each of the first t+1 parties draws r_i below 2^((l + sec_param) // (t+1)), computes g^(-r_i) (ffgm_pow_base on the
      window table of g^-1) and shares both,
      the r sharings are summed, the t+1 sharings of g^(-r_i) multiplied (multiply()),
      b + r 2^f is opened, g^((b + r 2^f) >> f) computed (ffgm_pow_base, shift = f), every party multiplies it by its share
      of g^(-r), and by 2^f.
    rand_exp(count, bound) returns the t+1 senders' plain draws as DevArrays of `count` values below bound.  The caller
    guarantees 0 <= B < 2^(l-f) and that b + r 2^f stays below p.  Needs m >= 2t+1 parties; bs is not written."""
    return [ctx.mul_scalar(x, (1 << f) % ctx.modulus) for x in _pow_public_base(ctx, field, g, bs, t, l, f, rand_exp, rng, sec_param)]


def exp2(ctx: FieldContext, field, xs: Shares, t: int, l: int, f: int, rand_trunc, rand_exp, rng=None, sec_param: int = 30) -> Shares:
    """runtime.np_exp2 for all parties: 2^a for a fixed-point sharing.  Domain: -f <= a and 2^a < 2^(l-1-f) on the values
    (below -f the reference itself returns field garbage).  Steps:
      the integral part: trunc() by f bits at L = max_a_bit_length + f, max_a_bit_length = f + bit_length(l-1-f) + 1,
      y = a_frac log 2 (a public float: one trunc()),
      the Taylor polynomial of degree taylor_exp2_degree(f): powers(), poly_dot with round(2^f / j!) and the constant 2^2f
      (ffgm_poly_dot), one trunc(),
      2^(a_int + 2^(l-1-f)) by pow_public_base's steps, one multiply(),
      the product by the public field element 2^(-2^(l-1-f)) 2^f and a last trunc() by f bits.
    rand_trunc and rand_exp: as for fxp_multiply() and pow_public_base().  Needs m >= 2t+1 parties; xs is not written."""
    import math
    m = len(xs)
    _parties('exp2', t, m)
    n = xs[0].n
    if any(x.n != n for x in xs) or not 1 <= f < l - 1:
        raise ValueError('exp2: shares of one length, 1 <= f < l - 1')
    p = ctx.modulus
    mabl = f + (l - 1 - f).bit_length() + 1
    rbits, rdivf = rand_trunc(n, f)
    a_int = trunc(ctx, field, xs, rbits, rdivf, t, f, mabl + f)
    a_frac = [ctx.sub(x, ctx.mul_scalar(ai, (1 << f) % p)) for x, ai in zip(xs, a_int)]
    y = _mul_public_float(ctx, field, a_frac, math.log(2), t, f, l, rand_trunc)
    theta = taylor_exp2_degree(f)
    coefs, fact = [], 1
    for j in range(1, theta + 1):
        fact *= j
        coefs.append(round((1 / fact) * 2**f))
    c = _taylor(ctx, field, y, coefs, (1 << 2 * f) % p, t, f, l, rand_trunc, rng)
    E = 1 << (l - 1 - f)
    pw = _pow_public_base(ctx, field, 2, [ctx.add_scalar(ai, E % p) for ai in a_int], t, l - f, 0, rand_exp, rng, sec_param + f)
    c = multiply(ctx, field, c, pw, t, rng)
    c = [ctx.mul_scalar(x, pow(2, -E, p) * (1 << f) % p) for x in c]
    rbits, rdivf = rand_trunc(n, f)
    return trunc(ctx, field, c, rbits, rdivf, t, f, l + f)


def exp(ctx: FieldContext, field, xs: Shares, t: int, l: int, f: int, rand_trunc, rand_exp, rng=None, sec_param: int = 30) -> Shares:
    """runtime.np_exp: exp2() of a times the public float log2(e)."""
    import math
    return exp2(ctx, field, _mul_public_float(ctx, field, xs, math.log2(math.e), t, f, l, rand_trunc), t, l, f, rand_trunc, rand_exp,
                rng, sec_param)


# ---- secure random bits over a prime field (runtime.np_random_bits, runtime.py:4187-4273, the PRSS branch :4243-4267) and
# the supplier of the protocols' correlated randomness ------------------------------------------------------------------
def _nonzero_mask(x: DevArray):
    """entries of x that are not 0, as a torch mask over the elements"""
    nz = x.t != 0
    return nz if nz.dim() == 1 else nz.any(dim=1)


def random_bits(ctx: FieldContext, field, count: int, t: int, draw, signed: bool = False, f: int = 0) -> Shares:
    """runtime.np_random_bits over a prime field for all parties: shares of `count` uniform bits scaled by 2^f, in {0, 1}, or
    in {-1, 1} when signed.  draw(h) returns (r, z): two sharings of h entries for all m >= 2t+1 parties, r uniform field
    elements, z a sharing of zero of degree 2t.  The loop is the reference's (runtime.py:4246-4264):

      draw h entries -> rbits_open on the first 2t+1 parties (ffgm_rbits_open: r^2 + z recombined in one pass, the zeros
      counted on the device) -> read the counter (one 4-byte copy per round, the reference's own synchronisation point) ->
      no zero and nothing kept: straight on; else keep the entries whose square is not 0 and draw as many again as were 0.

    The entries kept from earlier draws come first, then the last draw whole (np.append, runtime.py:4256-4261).  Then
    r (r^2)^(-1/2), a uniform +-1, and (bits + 1) / 2, shifted by f: one ffgm_rbits_finish for all parties when p = 3 mod 4
    (the exponentiation of the public squares runs once), composed from sqrt_cl, inv, mul, add_scalar and mul_scalar when
    p = 1 mod 4.  A compaction has probability count / p and uses torch indexing.  What draw() returns is never written."""
    if ctx.binary:
        raise ValueError('random_bits: a prime field (over GF(2^n) a random bit is one PRSS draw with mask_bits = 1)')
    p = ctx.modulus
    if count < 0 or f < 0 or t < 0:
        raise ValueError('random_bits: count, t and f are not negative')
    k = 2 * t + 1
    lam = _lagrange(field, range(1, k + 1))
    kept_r, kept_c, h, m = None, None, count, None
    while True:
        r, z = draw(h)
        if m is None:
            m = len(r)
        _parties('random bits', t, m, len(r), len(z))
        if any(x.n != h for w in (r, z) for x in w):
            raise ValueError('random_bits: draw(h) returns two sharings of h entries for every party')
        if count == 0:
            return [ctx.empty(0) for _ in range(m)]
        zeros = ctx.zero_counter()
        c = ctx.rbits_open(r[:k], z[:k], lam, zeros=zeros)
        h = int(zeros.item())
        if h == 0:
            break
        keep = _nonzero_mask(c)
        part_r, part_c = [x.t[keep] for x in r], c.t[keep]
        kept_r = part_r if kept_r is None else [_torch().cat([a, b]) for a, b in zip(kept_r, part_r)]
        kept_c = part_c if kept_c is None else _torch().cat([kept_c, part_c])
    own = kept_r is not None and kept_c.shape[0] > 0
    if own:                                                                         # the kept entries, then the last draw whole
        r = [DevArray(ctx, _torch().cat([a, x.t]), count) for a, x in zip(kept_r, r)]
        c = DevArray(ctx, _torch().cat([kept_c, c.t]), count)
    if p % 4 == 3:
        return ctx.rbits_finish(c, r, signed=signed, f=f, outs=r if own else None)
    s = ctx.inv(ctx.sqrt_cl(c))                                                     # (c has no zero left)
    bits = [ctx.mul(x, s) for x in r]
    if not signed:
        bits = [ctx.mul_scalar(ctx.add_scalar(b, 1), (p + 1) >> 1) for b in bits]
    return [ctx.mul_scalar(b, (1 << f) % p) for b in bits] if f else bits


# ---- the secure binary sign by Legendre symbols (the bsgn_0 / bsgn_1 / bsgn_2 of demos/np_bnnmnist.py:44-156) ------------
def bsgn_rows(d: int) -> int:
    """the symbols (2a + 1 + 2j | p), |j| <= (w - 1) / 2, variant d takes per element: w = 1, 3, 5"""
    if d not in (0, 1, 2):
        raise ValueError('bsgn: d is 0, 1 or 2')
    return (1, 3, 5)[d]


def bsgn_draws(d: int) -> int:
    """the (sign, element) pairs variant d draws per input element: 1, 3, 6 (np_bnnmnist.py:62, :92, :135)"""
    if d not in (0, 1, 2):
        raise ValueError('bsgn: d is 0, 1 or 2')
    return (1, 3, 6)[d]


def _legendre(p: int, v: int) -> int:
    v %= p
    if v == 0:
        return 0
    return 1 if pow(v, (p - 1) >> 1, p) == 1 else -1


def bsgn_value(p: int, d: int, a: int) -> int:
    """What bsgn() opens to for the input a over the odd prime p, as a signed integer: d = 0: (2a + 1 | p); d = 1:
    (u + v + w - u v w) / 2 over u, v, w = (2a - 1 | p), (2a + 1 | p), (2a + 3 | p), their majority; d = 2: (t | p) with t the
    sum of the five symbols (2a + 1 + 2j | p), |j| <= 2.  (0 | p) = 0, as gmpy2.legendre has it."""
    w = bsgn_rows(d)
    h = [_legendre(p, 2 * a + 1 + 2 * j) for j in range(-(w // 2), w // 2 + 1)]
    if d == 0:
        return h[0]
    if d == 2:
        return _legendre(p, sum(h))
    x = (h[0] + h[1] + h[2] - h[0] * h[1] * h[2]) * ((p + 1) >> 1) % p
    return x if x <= p >> 1 else x - p


def bsgn_range(p: int, d: int, limit: int = 4096) -> int:
    """The largest B <= limit with bsgn_value(p, d, a) = (1 if a >= 0 else -1) for every |a| <= B; -1 if there is none."""
    B = -1
    while B < limit and bsgn_value(p, d, B + 1) == 1 and (B + 1 == 0 or bsgn_value(p, d, -B - 1) == -1):
        B += 1
    return B


def bsgn(ctx: FieldContext, field, xs: Shares, t: int, d: int, rand_bsgn, rng=None) -> Shares:
    """The binary sign of the demo (np_bnnmnist.py:44-156) for all parties: shares of bsgn_value(p, d, a), which is 1 for
    a >= 0 and -1 otherwise for every |a| <= bsgn_range(p, d).  p = 3 mod 4, so (s | p) = s for a sign s: with z = s r^2, r a
    random nonzero element, y = (2a + 1) z is uniform among the nonzero elements, and s (y | p) = (2a + 1 | p).

    r2 = multiply(r, r) -> z = multiply(s, r2) (two re-sharing rounds) -> bsgn_mask per party (alpha = 2, beta = 1 + 2j:
    degree 2t) -> one opening from 2t+1 parties -> bsgn_finish for all parties (ONE exponentiation per opened value), then
      d = 0: the shares h s are the result;
      d = 1: the three rows of shares go through prod_rows (two rounds); (t0 + t1 + t2 - prod) (p + 1) / 2;
      d = 2: bsgn_finish in sum mode gives shares of T, the sum of the five symbols; bsgn_mask(T, z5, alpha = 1, beta = 0),
             a second opening at degree 2t, bsgn_finish with s5.
    Unlike the demo's d = 1 and d = 2 (which open s0 s1 s2 and s5 r5^2, and thereby the product of the three symbols and
    T), nothing but uniformly masked values is opened.  The arrays are row-major (w, n).

    rand_bsgn(count) supplies two sharings of count = bsgn_draws(d) n entries: uniform signs s in {1, -1} and uniform field
    elements r.  A zero symbol (r = 0, or 2a + 1 + 2j = 0 mod p) gives 0 in its term.  The inputs are never written."""
    w, draws = bsgn_rows(d), bsgn_draws(d)
    if ctx.binary or ctx.modulus % 4 != 3:
        raise ValueError('bsgn: a prime field with p = 3 mod 4')
    m = len(xs)
    senders = _parties('the binary sign', t, m)                                    # 2t+1: the masked values have degree 2t
    n, p = xs[0].n, ctx.modulus
    drawn = rand_bsgn(draws * n)
    if (not isinstance(drawn, (tuple, list)) or len(drawn) != 2 or any(len(v) != m for v in drawn)
            or any(x.n != draws * n for v in drawn for x in v)):
        raise ValueError('bsgn: rand_bsgn(count) returns two sharings of count entries for every party')
    s, r = drawn
    r2 = multiply(ctx, field, r, r, t, rng)
    z = multiply(ctx, field, s, r2, t, rng)
    betas = [1 + 2 * j for j in range(-(w // 2), w // 2 + 1)]
    zw, sw = [_rows(ctx, x, 0, w, n) for x in z], [_rows(ctx, x, 0, w, n) for x in s]
    c = open_(ctx, field, [ctx.bsgn_mask(xs[i], zw[i], 2, betas) for i in range(senders)], t, degree=2 * t)
    if d == 0:
        return ctx.bsgn_finish(c, sw, w)
    if d == 1:
        ts = ctx.bsgn_finish(c, sw, w)
        prod = prod_rows(ctx, field, ts, w, t, rng)
        out = []
        for x, q in zip(ts, prod):
            acc = ctx.add(ctx.add(_rows(ctx, x, 0, 1, n), _rows(ctx, x, 1, 2, n)), _rows(ctx, x, 2, 3, n))
            out.append(ctx.mul_scalar(ctx.sub(acc, q), (p + 1) >> 1))
        return out
    T = ctx.bsgn_finish(c, sw, w, sum=True)
    z5, s5 = [_rows(ctx, x, w, w + 1, n) for x in z], [_rows(ctx, x, w, w + 1, n) for x in s]
    c2 = open_(ctx, field, [ctx.bsgn_mask(T[i], z5[i], 1, [0]) for i in range(senders)], t, degree=2 * t)
    return ctx.bsgn_finish(c2, s5, 1)


# ---- unit vectors of secret indices and table lookup at them (runtime.np_unit_vector, runtime.py:5002-5029; runtime.unit_vector,
# runtime.py:4979-5000; mpyc.random.np_random_unit_vector, random.py:123-152), for a BATCH of n indices into one table --------
def unit_rounds(K: int, full: bool = False):
    """The plan of the demultiplexer for K positions, kbits = bit_length(K - 1) rounds: [(h, keep)] per round -- the round
    multiplies the first h rows of its level by the next index bit (most significant first), expands them to 2h rows and
    keeps the first `keep` of them as the next level.  Level s holds N_s = ceil(K / 2^(kbits-s)) rows (2^s when full: all
    K2 = 2^kbits positions), h = ceil(N_(s+1) / 2) <= N_s.  The first round has h = 1 and its parent is the public 1: it costs
    no multiplication.  About 2K rows are multiplied and written in all, not 2 K2."""
    if K < 1:
        raise ValueError('unit_rounds: at least one position')
    kbits = (K - 1).bit_length()
    plan = []
    for s in range(kbits):
        keep = 1 << (s + 1) if full else -(-K >> (kbits - s - 1))
        plan.append(((keep + 1) // 2, keep))
    return plan


def _public_ones(ctx: FieldContext, n: int) -> DevArray:
    one = ctx.empty(n)
    one.t.zero_()
    return ctx.add_scalar(one, 1)


def demux(ctx: FieldContext, field, bits: Shares, n: int, kbits: int, K: int, t: int, xstride: int = 1, full: bool = False,
          rng=None) -> Shares:
    """Shares of the position-major (K, n) unit vectors ((2^kbits, n) when full) of the n indices whose bits are shared in
    `bits`: row j is 1 where the index is j.  From the public 1, for the index bits most significant first (unit_rounds):
      unit_prod on the first 2t+1 parties: v = x u for the h rows the round needs (ffgm_unit_prod, x kept in registers),
      they re-share v (ffgpu_split_rng),
      tour_unit_expand per party: the received sub-shares recombined to v, and (u - v, v) interleaved to rows 2j, 2j + 1
      (ffgpu_tour_unit_expand as argmax uses it);
    the first round has the 1 for a parent and needs no multiplication.  After kbits rounds the 1 sits at row
    (x_(kbits-1) ... x_0)_2.

    xstride == 1: bits is bit-major (>= kbits, n), row i the bit of weight 2^i.  xstride == l >= kbits: bits is the
    element-major (n, l) output of to_bits(), bit i of element e at e*l + i.  Needs m >= 2t+1 parties; bits is not written."""
    m = len(bits)
    kk = _parties('the demultiplexer', t, m)
    if n < 0 or kbits != (K - 1).bit_length() or xstride < 1:
        raise ValueError('demux: K positions take kbits = bit_length(K - 1) bits')
    need = kbits * n if xstride == 1 else (n * xstride if xstride >= kbits else -1)
    if need < 0 or any(b.n < need for b in bits):
        raise ValueError('demux: kbits bits per index, bit-major (xstride 1) or element-major (xstride l >= kbits)')
    u = [_public_ones(ctx, n) for _ in range(m)]           # an array of its own per party: a caller may write one in place
    for s, (h, keep) in enumerate(unit_rounds(K, full)):
        i = kbits - 1 - s
        xoff = i * n if xstride == 1 else i
        if s == 0:                                      # the parent is the 1: (1 - x, x) without a multiplication
            top = [_rows(ctx, b, i, i + 1, n) if xstride == 1 else ctx.unit_prod(b, x, 1, xstride, xoff) for b, x in zip(bits, u)]
            u = [ctx.tour_unit_expand(u[j], [top[j]], [1], 1, 2, n) for j in range(m)]
        else:
            par = [_rows(ctx, x, 0, h, n) for x in u]
            sub = reshare(ctx, field, [ctx.unit_prod(bits[q], par[q], h, xstride, xoff) for q in range(kk)], t, m, rng)
            u = [ctx.tour_unit_expand(par[j], sub.rows[j], sub.lam, 1, 2 * h, n) for j in range(m)]
        if keep < 2 * h:
            u = [_rows(ctx, x, 0, keep, n) for x in u]
    return u


def random_unit_vectors(ctx: FieldContext, field, n: int, kbits: int, t: int, bits: Shares, rng=None) -> Shares:
    """mpyc.random.np_random_unit_vector for n vectors at once: shares of the position-major (2^kbits, n) unit vectors at
    uniformly random positions, from kbits*n shared random bits (bit-major).  The full demultiplexer: no position is left
    out, so nothing is opened and nothing restarts (the reference rejects and redraws for lengths that are no power of two)."""
    return demux(ctx, field, bits, n, kbits, 1 << kbits, t, full=True, rng=rng)


def _unit_positions(ctx: FieldContext, u: Shares, kbits: int, n: int) -> Shares:
    """u @ arange(K2) (runtime.py:5016), local: arg_index(u), through ffgm_unit_dot without a rotation on the table 0 .. K2 - 1
    where that table fits its LDS (a sixth of the time of arg_index's one-row matmul_stack: profiles/unitvec_kernels.md)"""
    K2 = 1 << kbits
    if kbits > ctx.unit_dot_max_kbits():
        return arg_index(ctx, u, 1, K2, n)
    iv = ctx.unit_iota(K2)
    return [ctx.unit_dot(x, iv, K2) for x in u]


def _unit_offsets(what: str, ctx: FieldContext, field, idx: Shares, K: int, t: int, rand_unit, sec_param: int, rng):
    """(u, c, kbits): shares of random (K2, n) unit vectors and the opened c = a - r + R K2, r their positions"""
    m = len(idx)
    _parties(what, t, m)
    n, p = idx[0].n, ctx.modulus
    kbits = (K - 1).bit_length()
    if ctx.binary or K < 2 or any(x.n != n for x in idx):
        raise ValueError(f'{what}: a prime field, at least two positions, shares of one length')
    if p.bit_length() <= sec_param + kbits + 1:
        raise ValueError(f'{what}: the field is too small: bit_length(p) > sec_param + kbits + 1')
    drawn = rand_unit(n, kbits, sec_param)
    if (not isinstance(drawn, (tuple, list)) or len(drawn) != 2 or any(len(v) != m for v in drawn)
            or any(b.n != kbits * n for b in drawn[0]) or any(r.n != n for r in drawn[1])):
        raise ValueError(f'{what}: rand_unit(count, kbits, sec_param) returns count*kbits bits and count values for every party')
    bits, R = drawn
    K2 = 1 << kbits
    u = random_unit_vectors(ctx, field, n, kbits, t, bits, rng)
    r = _unit_positions(ctx, u, kbits, n)
    masked = [ctx.add(ctx.sub(idx[i], r[i]), ctx.mul_scalar(R[i], K2)) for i in range(t + 1)]
    return u, open_(ctx, field, masked, t), kbits


def unit_vectors(ctx: FieldContext, field, idx: Shares, K: int, t: int, rand_unit, sec_param: int = 30, rng=None) -> Shares:
    """runtime.np_unit_vector for n secret indices at once, for all parties: shares of the position-major (K, n) unit vectors,
    row j is 1 where the index is j.  With K2 = 2^kbits, kbits = bit_length(K - 1):
      random_unit_vectors: u, (K2, n), from kbits*n random bits,
      r = arg_index(u), local (as a unit_dot on the table 0 .. K2 - 1 where that fits),
      c = a - r + R K2 is opened, R uniform in [1, 2^sec_param] per index (positive and below p: ValueError unless
      bit_length(p) > sec_param + kbits + 1),
      unit_roll per party: out[j] = u[(j - c) mod K2], j < K (ffgm_unit_roll).
    The reference rotates modulo n; here the rotation is modulo K2 and the first K rows are kept: the same function of a for
    0 <= a < K, which the caller guarantees -- otherwise the result is the unit vector of a mod K2 cut to K rows.  No bit
    decomposition.  rand_unit(count, kbits, sec_param) returns (bits, R): count*kbits shared bits, bit-major, and count
    shared values in [1, 2^sec_param] (Randomness.rand_unit).  K == 1 is the public 1.  idx is not written."""
    if K == 1:
        _parties('unit_vectors', t, len(idx))
        return [_public_ones(ctx, idx[0].n) for _ in idx]
    u, c, kbits = _unit_offsets('unit_vectors', ctx, field, idx, K, t, rand_unit, sec_param, rng)
    return [ctx.unit_roll(x, c, kbits, K) for x in u]


def unit_vectors_from_bits(ctx: FieldContext, field, bits: Shares, l: int, K: int, t: int, rng=None) -> Shares:
    """runtime.unit_vector for n secret indices at once, for all parties, behind to_bits(): bits is its element-major (n, l)
    output, l >= bit_length(K - 1).  The truncated demultiplexer on the low kbits bits, most significant first; nothing is
    opened.  Returns shares of the position-major (K, n) unit vectors of a mod 2^kbits cut to K rows."""
    kbits = (K - 1).bit_length() if K >= 1 else -1
    if l < 1 or kbits < 0 or kbits > l or any(b.n % l for b in bits):
        raise ValueError('unit_vectors_from_bits: (n, l) bits with l >= bit_length(K - 1)')
    return demux(ctx, field, bits, bits[0].n // l, kbits, K, t, xstride=l, rng=rng)


def lookup(ctx: FieldContext, field, idx: Shares, table, K: int, t: int, rand_unit, sec_param: int = 30, rng=None) -> Shares:
    """table[a] for n secret indices a at once, for all parties: `T @ np_unit_vector(a, K)` without the rotated vectors ever
    being stored.  table: a public DevArray of K entries, or Shares of one.  The steps of unit_vectors() up to the opening
    of c, then T[a] = sum_{i < K2} T[(i + c) mod K2] u[i] with T zero beyond K (ffgm_unit_dot, the table in LDS):
      public table: per party, local;
      shared table: on the first 2t+1 parties (degree 2t), then one re-sharing of n elements.
    Returns Shares of n entries.  0 <= a < K is the caller's guarantee; K == 1 is table[0].  2^kbits entries must fit the LDS
    of ffgm_unit_dot (FieldContext.unit_dot_max_kbits)."""
    m = len(idx)
    public = isinstance(table, DevArray)
    if (table.n if public else min((x.n for x in table), default=0)) != K or not public and len(table) != m:
        raise ValueError('lookup: a table of K entries, public or shared among all parties')
    if K == 1:
        _parties('lookup', t, m)
        one = _public_ones(ctx, idx[0].n)
        return [ctx.unit_dot(one, table if public else table[j], 1) for j in range(m)]
    u, c, kbits = _unit_offsets('lookup', ctx, field, idx, K, t, rand_unit, sec_param, rng)
    K2 = 1 << kbits
    if public:
        return [ctx.unit_dot(x, table, K2, c=c, kbits=kbits) for x in u]
    kk = 2 * t + 1
    return materialize(ctx, reshare(ctx, field, [ctx.unit_dot(u[q], table[q], K2, c=c, kbits=kbits) for q in range(kk)], t, m, rng))


# ---- secure 2-D convolution layers (demos/np_cnnmnist.py:53-92, :133-172) ------------------------------------------------------
# Dense row-major tensors on RAW integers, as for the fixed-point functions above: x (k, r, m, n) -- k images, r input
# channels --, W (v, r, s, s), b (v), the result (k, v, m, n).
def _per_sender(what: str, a, kk: int, m: int):
    """a public DevArray for every sender, or the first kk of the m parties' shares"""
    if isinstance(a, DevArray):
        return [a] * kk
    if len(a) != m:
        raise ValueError(f'{what}: an operand is public or shared among all parties')
    return list(a[:kk])


def _trunc_by(ctx: FieldContext, field, ys: Shares, t: int, f: int, l: Optional[int], rand_trunc) -> Shares:
    """trunc() by f bits with the draws of rand_trunc(count, f); L = l, by default the largest the field admits with the
    default draws of Randomness.rand_trunc: bit_length(p) - 2"""
    if rand_trunc is None:
        raise ValueError('a truncation needs rand_trunc')
    rbits, rdivf = rand_trunc(ys[0].n, f)
    return trunc(ctx, field, ys, rbits, rdivf, t, f, ctx.modulus.bit_length() - 2 if l is None else l)


def conv2d(ctx: FieldContext, field, xs: Shares, ws, bs, k: int, r: int, m: int, n: int, v: int, s: int, t: int, rng=None,
           f: int = 0, l: Optional[int] = None, rand_trunc=None) -> Shares:
    """The demo's convolvetensor (np_cnnmnist.py:53-85) for all parties:
      Y[i, j, I, J] = b[j] + sum_{l, di, dj} x[i, l, I + di - (s-1)//2, J + dj - s//2] W[j, l, di, dj], x outside the image 0,
    the local correlation of the first 2t+1 senders in ONE launch (ffgm_conv2d; degree 2t), the re-sharing round, and for
    f > 0 trunc() by f bits (np_cnnmnist.py:83-84; rand_trunc(count, f) as for fxp_multiply, l: the L of trunc()).

    ws: Shares of W, or one public DevArray for all parties (the result is then still re-shared, as the reference does).
    bs: Shares of b scaled by the caller as the demo's load() does, one public DevArray, or None.  1 <= s <= 16, s <= n."""
    M = len(xs)
    kk = _parties('conv2d', t, M)
    prod = ctx.conv2d(list(xs[:kk]), _per_sender('conv2d', ws, kk, M), None if bs is None else _per_sender('conv2d', bs, kk, M),
                      k, r, m, n, v, s)
    ys = materialize(ctx, reshare(ctx, field, prod, t, M, rng, what='conv2d'))
    return _trunc_by(ctx, field, ys, t, f, l, rand_trunc) if f > 0 else ys


def maxpool2x2(ctx: FieldContext, field, xs: Shares, planes: int, m: int, n: int, t: int, l: int, rand, rng=None) -> Shares:
    """The demo's maxpool (np_cnnmnist.py:88-92) on `planes` = k v images of (m, n): the maxima of 2 x 2 squares with stride
    2, as two amax() calls: rows in pairs, (planes m/2, 2, n), then columns in pairs, (planes m/2 n/2, 2, 1).  Returns shares
    of the (planes, m/2, n/2) array.  rand, l and the assumptions: amax()'s."""
    if m % 2 or n % 2:
        raise ValueError('maxpool2x2: m and n must be even')
    rows = amax(ctx, field, xs, planes * (m // 2), 2, n, t, l, rand, rng)
    return amax(ctx, field, rows, planes * (m // 2) * (n // 2), 2, 1, t, l, rand, rng)


def relu(ctx: FieldContext, field, xs: Shares, t: int, l: int, rand, rng=None) -> Shares:
    """(x >= 0) * x (np_cnnmnist.py:142): compare_zero(mode='lt') for [x < 0], then one secure multiplication of 1 - [x < 0]
    with x.  rand(count): (rbits, sbits, rdivl, rzero) as for amax() (Randomness.rand_compare(l)); -2^(l-1) <= x < 2^(l-1)."""
    _parties('relu', t, len(xs))
    rbits, sbits, rdivl, rzero = rand(xs[0].n)
    lt = compare_zero(ctx, field, xs, rbits, sbits, rdivl, rzero, t, l, mode='lt', rng=rng)
    return multiply(ctx, field, [ctx.rsub_scalar(b, 1) for b in lt], xs, t, rng)


def conv_layer(ctx: FieldContext, field, xs: Shares, ws, bs, k: int, r: int, m: int, n: int, v: int, s: int, t: int, l: int, rand,
               rng=None, f: int = 0, trunc_l: Optional[int] = None, rand_trunc=None) -> Shares:
    """conv2d -> maxpool2x2 -> relu: layers 1 and 2 of the demo (np_cnnmnist.py:133-155).  Returns shares of the
    (k, v, m/2, n/2) tensor.  l, rand: of the comparisons; f, trunc_l, rand_trunc: of conv2d's truncation."""
    y = conv2d(ctx, field, xs, ws, bs, k, r, m, n, v, s, t, rng, f, trunc_l, rand_trunc)
    y = maxpool2x2(ctx, field, y, k * v, m, n, t, l, rand, rng)
    return relu(ctx, field, y, t, l, rand, rng)


def dense(ctx: FieldContext, field, xs: Shares, ws, bs, M: int, K: int, N: int, t: int, rng=None, f: int = 0, l: Optional[int] = None,
          rand_trunc=None) -> Shares:
    """x @ W + b (np_cnnmnist.py:162, :172) for the (M, K) sharing xs: matmul() with shared W (K, N) -- a public DevArray W
    is a local product --, for f > 0 trunc() by f bits, then the bias b (N), public or shared or None, added to every row
    (its broadcast is the product of a column of ones with b, ffgpu_matmul)."""
    m = len(xs)
    if isinstance(ws, DevArray):
        _parties('dense', t, m)
        ys = [ctx.matmul(x, ws, M, K, N) for x in xs]
    else:
        ys = matmul(ctx, field, xs, ws, M, K, N, t, rng)
    if f > 0:
        ys = _trunc_by(ctx, field, ys, t, f, l, rand_trunc)
    if bs is None:
        return ys
    ones = _public_ones(ctx, M)
    rows = {}

    def spread(b: DevArray) -> DevArray:
        if id(b) not in rows:
            rows[id(b)] = ctx.matmul(ones, b, M, 1, N)
        return rows[id(b)]
    return [ctx.add(y, spread(b)) for y, b in zip(ys, _per_sender('dense', bs, m, m))]


def _torch():
    import torch
    return torch


class Randomness:
    """The shipped supplier of the protocols' correlated randomness for all m parties on one GPU: pseudorandom secret
    sharing (thresha.py:135-217) with one PRF key per subset of m - t parties, derived from `key`, and a counter as the
    common input, so that no two calls see the same one.  The PRF is the device's (a ChaCha stream per subset key and common
    input, thresha.prss_chacha_stream_key; ffgpu_prss_chacha with the weights f_S(i) of thresha._f_S_i, as
    thresha._prss_device fills one party's row), so the values are pinned by (key, rounds) and the order of the calls.

    elements / zeros / bits are the reference's _np_randoms, np_pseudorandom_share_0 and np_random_bits; rand_bits,
    rand_trunc, rand_zero, rand_bsgn, rand_unit, rand_exp and rand_compare(l) are the callables the protocols of this module document."""

    KEY_BYTES = 16                      # the reference's PRSS keys (runtime.py:130-140)
    DOMAIN = b'mpyc_amd randomness v1\0'

    def __init__(self, ctx: FieldContext, field, t: int, m: int, key: bytes, rounds: int = 20, sec_param: int = 30):
        import itertools
        from hashlib import shake_128
        if ctx.binary:
            raise ValueError('Randomness: a prime field')
        if not 0 <= t or m < 2 * t + 1:
            raise ValueError('Randomness: m >= 2t+1 parties')
        self.ctx, self.field, self.t, self.m, self.rounds, self.sec_param = ctx, field, t, m, rounds, sec_param
        key = bytes(key)
        head = self.DOMAIN + len(key).to_bytes(2, 'little') + key
        self._subsets = [tuple(S) for S in itertools.combinations(range(m), m - t)]
        self._keys = {S: shake_128(head + b'S' + bytes(S)).digest(self.KEY_BYTES) for S in self._subsets}
        self._own = [shake_128(head + b'P' + bytes([i])).digest(self.KEY_BYTES) for i in range(m)]     # a party's private draws
        self._ncomb = len(self._subsets)
        self.counter = 0                # common inputs handed out so far

    def _uci(self) -> bytes:
        """the next common input: every call takes one, none is used twice"""
        c = self.counter
        self.counter += 1
        return c.to_bytes(8, 'little')

    def _prss(self, count: int, bound: int, zero: bool) -> Shares:
        """one PRSS call for all parties: thresha._prss_device (np convention) per party, the device PRF"""
        ctx, m, t, p = self.ctx, self.m, self.t, self.ctx.modulus
        uci = self._uci()
        if bound & (bound - 1) == 0:
            mask_bits, l = bound.bit_length() - 1, (bound.bit_length() - 1 + 7) // 8
        elif bound == p:
            mask_bits, l = 0, ((p - 1).bit_length() + 7) // 8 + self.KEY_BYTES
        else:
            raise ValueError('Randomness: the bound is the field order or a power of two')
        d = t if zero else 1
        if count == 0 or mask_bits == 0 and l == 0 or d == 0:                       # nothing, bound 1, or t = 0: zeros
            out = [ctx.empty(count) for _ in range(m)]
            for x in out:
                x.t.zero_()
            return out
        if l > thresha.PRSS_MAX_DRAW_BYTES or d > 64:
            raise NotImplementedError('Randomness: the draw is wider than ffgpu_prss_chacha takes')
        per = max(1, min(32, 64 // d))
        out = []
        for i in range(m):
            mine = [S for S in self._subsets if i in S]
            weights = []
            for S in mine:
                fs = int(thresha._f_S_i(self.field, m, i, S))
                weights += [fs * pow(i + 1, j + 1, p) % p if zero else fs for j in range(d)]
            keys = [thresha.prss_chacha_stream_key(self._keys[S], uci) for S in mine]
            x = ctx.empty(count)
            for k0 in range(0, len(mine), per):
                ctx.prss_chacha(keys[k0:k0 + per], d, l, weights[k0 * d:(k0 + per) * d], count, mask_bits=mask_bits, rounds=self.rounds,
                                out=x, accumulate=k0 > 0)
            out.append(x)
        return out

    def rounded_bound(self, bound: int) -> int:
        """the power of two _np_randoms draws below per subset key (runtime.py:4074-4075): the sum stays below `bound`"""
        return 1 << max(0, (bound // self._ncomb).bit_length() - 1)

    def elements(self, count: int, bound: Optional[int] = None) -> Shares:
        """runtime._np_randoms: a degree-t sharing of `count` random values, uniform field elements, or, with a bound, sums of
        comb(m, t) draws below rounded_bound(bound) each."""
        return self._prss(count, self.ctx.modulus if bound is None else self.rounded_bound(bound), False)

    def zeros(self, count: int) -> Shares:
        """thresha.np_pseudorandom_share_0: a random sharing of zero of degree 2t"""
        return self._prss(count, self.ctx.modulus, True)

    def _draw(self, h: int):
        return self.elements(h), self.zeros(h)

    def bits(self, count: int, signed: bool = False, f: int = 0) -> Shares:
        """runtime.np_random_bits: `count` uniform bits (random_bits with this supplier's own draws)"""
        return random_bits(self.ctx, self.field, count, self.t, self._draw, signed=signed, f=f)

    # ---- the callables of the protocols ----
    def rand_bits(self, count: int, l: int, bit_length: Optional[int] = None):
        """(rbits, rdivl) of to_bits() / norm(): count * l bits and count values below 2^(bit_length + sec_param - l)
        (runtime.py:4412, :4439; bit_length: of the secure type, l by default)."""
        return self.bits(count * l), self.elements(count, 1 << ((l if bit_length is None else bit_length) + self.sec_param - l))

    def rand_trunc(self, count: int, f: int, l: Optional[int] = None):
        """(rbits, rdivf) of trunc() / fxp_multiply(): count * f bits and count values below 2^(sec_param + l - f)
        (runtime.py:859-862), l the bit length np_trunc works with -- the L of trunc(), bit length plus f for a fixed-point
        product.  By default the largest the field admits: the opened a + 2^(l-1) + r + 2^f R is below 2^l + 2^f +
        2^(sec_param + l) < p for l = bit_length(p) - sec_param - 2."""
        if l is None:
            l = self.ctx.modulus.bit_length() - self.sec_param - 2
        if l < f:
            raise ValueError('rand_trunc: the field is too small for this truncation')
        return self.bits(count * f), self.elements(count, 1 << (self.sec_param + l - f))

    def rand_zero(self, count: int):
        """(z, r, s) of is_zero(): bits, and two sharings of uniform elements (runtime.py:3594-3599)"""
        z = self.bits(count)
        s = self.elements(count)
        return z, self.elements(count), s

    def rand_bsgn(self, count: int):
        """(s, r) of bsgn(): signs in {1, -1}, then uniform elements -- the draw order of the demo (np_random_bits, then
        _np_randoms: np_bnnmnist.py:62-63)"""
        s = self.bits(count, signed=True)
        return s, self.elements(count)

    def rand_unit(self, count: int, kbits: int, sec_param: Optional[int] = None):
        """(bits, R) of unit_vectors() / lookup(): count * kbits bits, bit-major, and count values in [1, 2^sec_param]
        (runtime.py:5021-5024: `_random(type(a), 1 << sec_param)` plus 1)"""
        sec = self.sec_param if sec_param is None else sec_param
        bits = self.bits(count * kbits)
        return bits, [self.ctx.add_scalar(x, 1) for x in self.elements(count, 1 << sec)]

    def rand_compare(self, l: int):
        """rand(count) of compare_zero() / sort() / amax() ...: (rbits, sbits, rdivl, rzero) for `count` comparisons of bit
        length l -- count * l bits element-major, count bits, count values below 2^sec_param (runtime.py:3644-3645) and count
        uniform elements, nonzero but for a probability of count / p (runtime.py:947)."""
        def rand(count: int):
            return self.bits(count * l), self.bits(count), self.elements(count, 1 << self.sec_param), self.elements(count)
        return rand

    def rand_exp(self, count: int, bound: int):
        """the t+1 senders' plain draws of pow_public_base(): `count` values below bound (a power of two) each, from a stream
        only that sender holds"""
        if bound < 1 or bound & (bound - 1):
            raise ValueError('rand_exp: the bound is a power of two')
        ctx, uci = self.ctx, self._uci()
        mask_bits = bound.bit_length() - 1
        out = []
        for i in range(self.t + 1):
            x = ctx.empty(count)
            if count and mask_bits:
                ctx.prss_chacha([thresha.prss_chacha_stream_key(self._own[i], uci)], 1, (mask_bits + 7) // 8, [1], count,
                                mask_bits=mask_bits, rounds=self.rounds, out=x)
            else:
                x.t.zero_()
            out.append(x)
        return out


# ---- threshold SHA-3: Keccak-f[1600] on secret-shared bits (demos/sha3.py) ---------------------------------------------
# Every bit of a Keccak state is shared as one element of GF(2^e), 2^e > m (the reference's SecFld(2) does the same,
# sha3.py:13-17): GF(4) for three parties, GF(8) for up to seven, one element per byte.  A party's share of a batch of
# `nstates` states is one row of 1600 * nstates bytes, state-major, position i = 64 (5 y + x) + z of a state at byte i
# (S[i] of sha3.py:43); all parties are the rows of one DevMatrix.  A round is ONE launch for all 2t+1 senders
# (FieldContext.keccak_round): it recombines the previous round's [recipient][sender] block, adds that round's constants,
# runs theta, rho, pi and chi's local product and re-shares the 1600 elements of every state.  Messages are bit shares too:
# bit j of message byte B is (B >> j) & 1 (FIPS 202), a batch of `nstates` messages of one common length `nbits` is a
# state-major (nstates, nbits) array per party.
KECCAK_B = 1600


def _state_view(mtx, nstates: int, width: int):
    """(parties, nstates, width) view of a DevMatrix whose rows are state-major (nstates, width) arrays"""
    return mtx.t[:, :nstates * width].unflatten(1, (nstates, width))


def keccak_f1600(ctx: FieldContext, field, S, nstates: int, t: int, rng=None):
    """keccak_f1600 (sha3.py:72-106) on a batch of states for all parties: S is a DevMatrix, row j = party j+1's share of
    nstates x 1600 bits; returns a new DevMatrix of the same shape, S is not written.  24 launches of keccak_round -- launch
    r recombines round r-1's sub-shares and adds the constants of round r-1 in its front -- and one keccak_local that
    recombines the last block and adds the constants of round 23, for all parties at once.  t = 0 (nothing to re-share,
    runtime.py:603-606): the same 25 launches of keccak_local on the parties' rows.  rng: an engine.RngState (one
    rng.commit() follows the 24 rounds) or None (a fresh host key per launch)."""
    m, n = S.rows, KECCAK_B * nstates
    if S.n != n:
        raise ValueError('keccak_f1600: rows of 1600 * nstates elements')
    k = _parties('keccak_f1600', t, m)
    if t == 0:
        cur, spare = S, None
        for r in range(24):
            nxt = ctx.keccak_local([cur.row(0)], [1], nstates, iota_round=r - 1, nbatch=m, stride_in=cur.stride, out=spare)
            cur, spare = nxt, (cur if r else None)
        return ctx.keccak_local([cur.row(0)], [1], nstates, iota_round=23, apply_round=False, nbatch=m, stride_in=cur.stride,
                                out=spare)
    lam = _lagrange(field, range(1, k + 1))
    rows, la, stride, spare = [S.row(0)], [1], S.stride, None
    for r in range(24):
        blk = ctx.keccak_round(rows, la, nstates, t, m, iota_round=r - 1, stride_in=stride, out=spare, state=rng)
        spare = cur if r else None                   # two blocks take turns: a launch never writes what it reads
        cur = blk
        rows, la, stride = [blk.row(s) for s in range(k)], lam, k * blk.stride
    if rng is not None:
        rng.commit()                                 # one nonce update for the 24 rounds (deferred advance)
    return ctx.keccak_local(rows, la, nstates, iota_round=23, apply_round=False, nbatch=m, stride_in=stride)


def sponge(ctx: FieldContext, field, bits, nbits: int, nstates: int, t: int, r: int, d: int, suffix: Sequence[int] = (),
           rng=None):
    """sponge (sha3.py:109-128) with rate r and output length d over a batch: bits is a DevMatrix, row j = party j+1's
    shares of the (nstates, nbits) message bits (nbits == 0: a matrix of empty rows, one per party); `suffix` the public
    domain bits appended to every message.  Suffix, the 10*1 padding and the zero initial state are public: they are XORed as the field's 1 into every
    party's row.  Returns a DevMatrix of (nstates, d) bit shares per party."""
    import numpy as np
    import torch
    if not (0 < r < KECCAK_B) or d < 1 or nbits < 0 or nstates < 1:
        raise ValueError('sponge: 0 < r < 1600, d >= 1, nstates >= 1')
    if bits.n != nstates * nbits:
        raise ValueError('sponge: the message is (nstates, nbits) bit shares per party')
    npub = nbits + len(suffix)
    public = np.zeros(npub + 2 + (-(npub + 2)) % r, dtype=np.uint8)          # P of sha3.py:112, message bits left zero
    public[nbits:npub] = np.asarray(suffix, dtype=np.uint8)
    public[npub] = 1
    public[-1] ^= 1
    m = bits.rows
    _parties('sponge', t, m)
    S = ctx.empty_matrix(m, KECCAK_B * nstates)
    S.t.zero_()
    pub = torch.from_numpy(public).to(S.t.device)
    msg = _state_view(bits, nstates, nbits) if nbits else None
    for i in range(len(public) // r):
        sv = _state_view(S, nstates, KECCAK_B)
        lo, hi = i * r, min((i + 1) * r, nbits)
        if hi > lo:
            sv[:, :, :hi - lo] ^= msg[:, :, lo:hi]
        sv[:, :, :r] ^= pub[i * r:(i + 1) * r]
        S = keccak_f1600(ctx, field, S, nstates, t, rng)
    out = ctx.empty_matrix(m, nstates * d)
    ov, got = _state_view(out, nstates, d), 0
    while True:
        take = min(r, d - got)
        ov[:, :, got:got + take] = _state_view(S, nstates, KECCAK_B)[:, :, :take]
        got += take
        if got == d:
            return out
        S = keccak_f1600(ctx, field, S, nstates, t, rng)


def sha3(ctx: FieldContext, field, bits, nbits: int, nstates: int, t: int, d: int = 256, rng=None):
    """SHA3-d (sha3.py:137-141) of a batch of secret-shared messages: capacity 2d, domain bits 01."""
    if d not in (224, 256, 384, 512):
        raise ValueError('sha3: d is 224, 256, 384 or 512')
    return sponge(ctx, field, bits, nbits, nstates, t, KECCAK_B - 2 * d, d, (0, 1), rng)


def shake(ctx: FieldContext, field, bits, nbits: int, nstates: int, t: int, d: int, c: int = 256, rng=None):
    """SHAKE[c/2] (sha3.py:144-148) with d output bits: domain bits 1111."""
    if c not in (256, 512):
        raise ValueError('shake: c is 256 (SHAKE128) or 512 (SHAKE256)')
    return sponge(ctx, field, bits, nbits, nstates, t, KECCAK_B - c, d, (1, 1, 1, 1), rng)


def message_bits(messages: Sequence[bytes]):
    """The (nstates, 8 * len) bit array of a batch of equally long byte strings, bit j of byte B = (B >> j) & 1 (numpy uint8)."""
    import numpy as np
    a = np.frombuffer(b''.join(messages), dtype=np.uint8).reshape(len(messages), len(messages[0]))
    return np.unpackbits(a, axis=1, bitorder='little')


def digest_bytes(opened) -> List[bytes]:
    """Opened digest bits, an (nstates, d) array of 0 / 1 with d a multiple of 8, packed into bytes LSB first (what
    sha3.py:151-158 xprint undoes per byte): one bytes object per state."""
    import numpy as np
    a = np.asarray(opened, dtype=np.uint8)
    if a.ndim != 2 or a.shape[1] % 8 or (a > 1).any():
        raise ValueError('digest_bytes: (nstates, d) bits, d a multiple of 8')
    return [bytes(row) for row in np.packbits(a, axis=1, bitorder='little')]
