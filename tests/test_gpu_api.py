"""GPU tests of the host-side mirror (mpyc_amd.finfields / mpyc_amd.thresha): the reference's own
tests for this path restated against the mirror (tests/test_thresha.py:15-40 round trips,
tests/test_finfields.py:94-99,327-335,372-404 array behaviour), plus bit-exact parity with the
golden vectors through the public API using the `randbelow` hook (the reference's tests patch
secrets.randbelow the same way)."""
import random

import numpy as np
import pytest

from fieldutil import unhex

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    from mpyc_amd import finfields, gfpx, thresha
    return finfields, gfpx, thresha


def field_from_case(api, case):
    finfields, gfpx, _ = api
    mod = int(case['modulus'], 16)
    return finfields.GF(gfpx.BinaryPolynomial(mod)) if case['binary'] else finfields.GF(mod)


def ints(a):
    return [int(v) for v in np.asarray(a.value).reshape(-1)]


def test_thresha_round_trips(api):
    """tests/test_thresha.py:15-40: random_split -> recombine for t in [0,8), m = 2t+1 and m = 17."""
    finfields, gfpx, thresha = api
    for field in (finfields.GF(19), finfields.GF(gfpx.GFpX(2)(0x11b)), finfields.GF(2**61 - 1),
                  finfields.GF(2**128 - 173)):
        a = [field(0), field(1), field(field.order - 1)] + [field(i + 2) for i in range(5)]
        for t in range(8):
            for m in (2 * t + 1, 17):
                if m >= field.order:
                    continue
                shares = thresha.random_split(field, a, t, m)
                assert len(shares) == m and len(shares[0]) == len(a)
                pts = [(i + 1, shares[i]) for i in range(t + 1)]
                b = thresha.recombine(field, pts)
                assert [int(x) for x in b] == [int(x.value) for x in a], (field, t, m)
                pts = [(i + 1, [field(int(v)) for v in shares[i]]) for i in range(m - t - 1, m)]
                b = thresha.recombine(field, pts)
                assert b == a, (field, t, m)
                # array path
                sh = thresha.np_random_split(field, field.array([int(x.value) for x in a]), t, m)
                assert sh.shape == (m, len(a))
                y = thresha.np_recombine(field, [(j + 1, sh[j]) for j in range(t + 1)])
                assert isinstance(y, field.array) and ints(y) == [int(x.value) for x in a]
    assert thresha.random_split(finfields.GF(19), [], 1, 3) == [[], [], []]


def test_golden_parity_through_api(api, golden_fields):
    """np_random_split / random_split / np_recombine reproduce the reference bit for bit when the
    same draws are replayed (the two paths use different conventions)."""
    finfields, gfpx, thresha = api
    try:
        for name, case in golden_fields.items():
            field = field_from_case(api, case)
            a = unhex(case['a'])
            s = a[:13] + a[-5:]
            for sc in case['sharing']:
                t, m, draws = sc['t'], sc['m'], unhex(sc['draws'])
                it = iter(draws)
                thresha.randbelow = lambda bound: next(it)
                sh = thresha.np_random_split(field, field.array(s), t, m)
                assert [[int(v) for v in row] for row in sh.value] == [unhex(r) for r in sc['np_shares']], (name, t, m)
                it = iter(draws)
                li = thresha.random_split(field, list(s), t, m)
                assert [[int(v) for v in row] for row in li] == [unhex(r) for r in sc['list_shares']], (name, t, m)
                for rec in sc['recombine']:
                    xs = tuple(rec['xs'])
                    assert [int(v) for v in thresha._recombination_vector(field, xs, 0)] == unhex(rec['vector'])
                    y = thresha.np_recombine(field, [(x, sh[x - 1]) for x in xs])
                    assert ints(y) == unhex(rec['np_out']), (name, xs)
                    # rows as plain object ndarrays (what pickle.loads hands the runtime)
                    y2 = thresha.np_recombine(field, [(x, sh[x - 1].value) for x in xs])
                    assert ints(y2) == unhex(rec['np_out'])
                mu = sc['multi']
                yw = thresha.np_recombine(field, [(x, sh[x - 1]) for x in mu['xs']], mu['x_rs'])
                assert yw.shape == (len(mu['x_rs']), len(s))
                assert [[int(v) for v in row] for row in yw.value] == [unhex(r) for r in mu['out']], name
    finally:
        thresha.randbelow = None


def test_array_semantics(api, golden_fields):
    finfields, gfpx, _ = api
    for name in ('P61', 'P64', 'P128', 'P127', 'GF19', 'GF2_8', 'GF2_128', 'P31'):
        case = golden_fields[name]
        F = field_from_case(api, case)
        a, b = unhex(case['a']), unhex(case['b'])
        A, B = F.array(a), F.array(b)
        assert A.shape == (len(a),) and A.ndim == 1 and len(A) == len(a) and A.size == len(a)
        assert ints(A + B) == unhex(case['add']) and ints(A - B) == unhex(case['sub'])
        assert ints(A * B) == unhex(case['mul']) and ints(-A) == unhex(case['neg'])
        sc = int(case['scalar'], 16)
        for other in (sc, F(sc), np.int64(sc) if sc < 2**63 else sc):
            assert ints(A + other) == unhex(case['add_scalar']), name
            assert ints(other + A) == unhex(case['add_scalar']), name
            assert ints(A * other) == unhex(case['mul_scalar']), name
            assert ints(other - A) == unhex(case['rsub_scalar']), name
        # ndarray operand (finfields.py:1045-1054)
        assert ints(A * np.array(b, dtype=object)) == unhex(case['mul'])
        # in place
        C = A.copy()
        C *= B
        assert ints(C) == unhex(case['mul'])
        C = A.copy()
        C += B
        C -= B
        assert ints(C) == a
        # raw inputs are reduced, not rejected (finfields.py:724); negatives wrap (test_finfields.py:327-335)
        assert ints(F.array(unhex(case['raw']))) == unhex(case['raw_reduced'])
        if 'neg_in' in case:
            assert ints(F.array(case['neg_in'])) == unhex(case['neg_in_reduced'])
        # value is the reference representation
        v = A.value
        assert v.dtype == object and v.shape == (len(a),)
        if case['binary']:
            assert isinstance(v[0], gfpx.BinaryPolynomial)
        # wire format == field.to_bytes / from_bytes (finfields.py:91-102)
        assert A.to_wire() == F.to_bytes(a)
        assert ints(F.array.from_wire(F.to_bytes(a))) == a
        assert F.from_bytes(A.to_wire()) == a
        # reciprocal / division / pow
        nz = [x for x in a if x][:12]
        N = F.array(nz)
        inv = N.reciprocal()
        assert ints(inv * N) == [1] * len(nz)
        assert ints(N / N) == [1] * len(nz)
        assert ints(N ** 3) == [int((F(x) ** 3).value) for x in nz]
        assert ints(N ** 0) == [1] * len(nz)
        assert ints(N ** -1) == ints(inv)
        with pytest.raises(ZeroDivisionError):
            F.array([1, 0, 2] if F.order > 2 else [1, 0]).reciprocal()
        # equality
        assert (A == A).all() and not (A != A).any()
        assert list(A == B) == [x == y for x, y in zip(a, b)]


def test_type_errors_and_shapes(api):
    finfields, gfpx, _ = api
    F = finfields.GF(101)
    G = finfields.GF(19)
    with pytest.raises(TypeError):
        F.array([1.5, 2.0])                          # tests/test_finfields.py:372-382
    with pytest.raises(TypeError):
        F.array([1, 2]) + 1.5
    with pytest.raises(TypeError):
        F.array([1, 2]) + G.array([1, 2])            # :296-314 mixed fields
    with pytest.raises(ValueError):
        finfields.GF(15)
    with pytest.raises(ValueError):
        finfields.GF(gfpx.BinaryPolynomial(0b101))   # x^2+1 is reducible
    a = F.array([[1, 2, 3], [4, 5, 6]])
    assert a.shape == (2, 3) and a.ndim == 2
    assert ints(a + F.array([10, 20, 30])) == [11, 22, 33, 14, 25, 36]      # broadcasting
    assert ints(a * F.array([[2], [3]])) == [2, 4, 6, 12, 15, 18]
    assert ints(a.reshape(3, 2)) == [1, 2, 3, 4, 5, 6] and a.reshape(-1).shape == (6,)
    assert ints(a[1]) == [4, 5, 6] and int(a[1][2].value) == 6 and int(a[0, 1].value) == 2
    assert ints(a[:, 1]) == [2, 5]
    b = a.copy()
    b[0] = F.array([7, 8, 9])
    b[1, 2] = 100
    assert ints(b) == [7, 8, 9, 4, 5, 100] and ints(a) == [1, 2, 3, 4, 5, 6]
    assert ints(a << 2) == [4, 8, 12, 16, 20, 24]
    assert ints((a << 2) >> 2) == [1, 2, 3, 4, 5, 6]
    assert [int(v) for v in a.signed_().reshape(-1)] == [1, 2, 3, 4, 5, 6]
    assert [int(v) for v in (-a).signed_().reshape(-1)] == [-1, -2, -3, -4, -5, -6]
    # small public matrix @ array (Vandermonde / Lagrange shape, finfields.py:1126-1135)
    rng = random.Random(3)
    P = finfields.GF(2**127 - 1)
    p = P.modulus
    X = [[rng.randrange(p) for _ in range(50)] for _ in range(4)]
    M = [[rng.randrange(p) for _ in range(4)] for _ in range(3)]
    got = np.array(M, dtype=object) @ P.array(X)
    want = (np.array(M, dtype=object) @ np.array(X, dtype=object)) % p
    assert got.shape == (3, 50) and [[int(v) for v in r] for r in got.value] == [[int(v) for v in r] for r in want]
    v = np.array(M[0], dtype=object) @ P.array(X)
    assert v.shape == (50,) and ints(v) == [int(x) for x in want[0]]


def test_large_prime_array_ops(api):
    """tests/test_finfields.py:389-404 shape: a 2^127-1 prime array: multiply, add, reciprocal."""
    finfields, _, _ = api
    p = 2**127 - 1
    F = finfields.GF(p)
    rng = random.Random(9)
    a = [rng.randrange(1, p) for _ in range(1000)]
    b = [rng.randrange(p) for _ in range(1000)]
    A, B = F.array(a), F.array(b)
    assert ints(A * B) == [x * y % p for x, y in zip(a, b)]
    assert ints(A + B) == [(x + y) % p for x, y in zip(a, b)]
    assert ints(A.reciprocal()) == [pow(x, -1, p) for x in a]
    assert ints(B / A) == [y * pow(x, -1, p) % p for x, y in zip(a, b)]


def test_sqrt_and_is_sqr(api):
    """tests/test_finfields.py:389-404 (sqrt of squares over a Blum prime), GF(2^8) sqrt."""
    finfields, gfpx, _ = api
    for p in (2**61 - 1, 2**127 - 1, 2**64 - 189, 19):
        F = finfields.GF(p)
        rng = random.Random(p)
        a = [rng.randrange(1, p) for _ in range(500)]
        A = F.array(a)
        sq = A * A
        r = sq.sqrt()
        assert ints(r * r) == ints(sq)
        assert sq.is_sqr().all()
        leg = A.is_sqr()
        assert list(leg) == [pow(x, (p - 1) // 2, p) != p - 1 for x in a]
        ri = sq.sqrt(INV=True)
        assert ints(ri * ri * sq) == [1] * len(a)
    G = finfields.GF(gfpx.GFpX(2)(0x11b))
    x = G.array(list(range(256)))
    r = x.sqrt()
    assert ints(r * r) == list(range(256))
    with pytest.raises(ZeroDivisionError):
        x.sqrt(INV=True)


def test_lazy_product_fuses_into_split_and_stays_correct(api):
    """a * b is deferred; np_random_split consumes it through the fused mul_split kernel; any other use
    (or an in-place update of an operand) materialises it first.  Results are identical either way."""
    finfields, gfpx, thresha = api
    F = finfields.GF(2**61 - 1)
    p = F.modulus
    rng = random.Random(4)
    n = 5000
    a = [rng.randrange(p) for _ in range(n)]
    b = [rng.randrange(p) for _ in range(n)]
    prod = [x * y % p for x, y in zip(a, b)]
    A, B = F.array(a), F.array(b)
    C = A * B
    assert C._take_lazy_product() is not None                 # nothing launched yet
    draws = [rng.randrange(p) for _ in range(n)]
    try:
        it = iter(draws)
        thresha.randbelow = lambda bound: next(it)
        sh = thresha.np_random_split(F, C.reshape(-1), 1, 3)   # fused: product never written
        it = iter(draws)
        finfields.lazy_products = False
        sh_ref = thresha.np_random_split(F, A * B, 1, 3)
    finally:
        thresha.randbelow = None
        finfields.lazy_products = True
    for i in range(3):
        assert ints(sh[i]) == ints(sh_ref[i]) == [(c + d * (i + 1)) % p for c, d in zip(prod, draws)]
    y = thresha.np_recombine(F, [(1, sh[0]), (2, sh[1])])
    assert ints(y) == prod
    # any other use materialises
    D = A * B
    assert ints(D + 0) == prod and D._take_lazy_product() is None
    # in-place update of an operand after the product was formed must not leak into it
    E = A * B
    A += 1
    assert ints(E) == prod
    assert ints(A) == [(x + 1) % p for x in a]
    G = A * B
    B[0] = 5
    assert ints(G)[0] == (a[0] + 1) * b[0] % p


def test_prss_matches_reference(api):
    """np_pseudorandom_share / _0 and the list versions against golden vectors from the reference
    (every party, several (m, t), bound = field order and a power of two); tests/test_thresha.py:56-86."""
    import json, os
    finfields, gfpx, thresha = api
    gold = {}
    for fname in ('prss.json', 'prss_wide.json'):            # prss_wide.json: three-limb prime fields
        with open(os.path.join(os.path.dirname(__file__), 'golden', fname)) as fh:
            gold.update(json.load(fh))
    for name, case in gold.items():
        mod = int(case['modulus'], 16)
        F = finfields.GF(gfpx.BinaryPolynomial(mod)) if case['binary'] else finfields.GF(mod)
        uci, n = bytes.fromhex(case['uci']), case['n']
        for st in case['settings']:
            m, t, bound = st['m'], st['t'], int(st['bound'], 16)
            keys = {tuple(int(x) for x in k.split(',')): bytes.fromhex(v) for k, v in st['keys'].items()}
            first = next(iter(keys))
            assert [int(v) for v in thresha.PRF(keys[first], bound)(uci, n)] == unhex(st['prf0'])
            for i, party in enumerate(st['parties']):
                prfs = {S: thresha.PRF(k, bound) for S, k in keys.items() if i in S}
                sh = thresha.np_pseudorandom_share(F, m, i, prfs, uci, n)
                assert isinstance(sh, F.array) and ints(sh) == unhex(party['share']), (name, m, i)
                assert [int(v.value) for v in thresha.pseudorandom_share(F, m, i, prfs, uci, n)] == unhex(party['share'])
                if 'zero_np' in party:
                    assert ints(thresha.np_pseudorandom_share_0(F, m, i, prfs, uci, n)) == unhex(party['zero_np'])
                    assert [int(v.value) for v in thresha.pseudorandom_share_zero(F, m, i, prfs, uci, n)] == \
                        unhex(party['zero_list'])
    # reference KATs for the PRF (tests/test_thresha.py:42-54)
    key = int('0x00112233445566778899aabbccddeeff', 16).to_bytes(16, byteorder='little')
    assert thresha.PRF(key, 1)(b'test') == 0
    y = thresha.PRF(key, 100)(b'')
    assert 0 <= y < 100 and y == thresha.PRF(key, 100)(b'')
    # larger batch: round trip across parties for m = 3, t = 1 over P61 (shares of a common secret)
    F = finfields.GF(2**61 - 1)
    n = 20000
    ks = {(0, 1): b'k01' * 6, (0, 2): b'k02' * 6, (1, 2): b'k12' * 6}
    shares = []
    for i in range(3):
        prfs = {S: thresha.PRF(k[:16], F.order) for S, k in ks.items() if i in S}
        shares.append(thresha.np_pseudorandom_share(F, 3, i, prfs, b'uci-1', n))
    a = thresha.np_recombine(F, [(1, shares[0]), (2, shares[1])])
    b = thresha.np_recombine(F, [(2, shares[1]), (3, shares[2])])
    assert ints(a) == ints(b)
    zs = []
    for i in range(3):
        prfs = {S: thresha.PRF(k[:16], F.order) for S, k in ks.items() if i in S}
        zs.append(thresha.np_pseudorandom_share_0(F, 3, i, prfs, b'uci-2', n))
    z = thresha.np_recombine(F, [(1, zs[0]), (2, zs[1]), (3, zs[2])])
    assert ints(z) == [0] * n


def test_prss_streamed_equals_one_shot(api, monkeypatch):
    """Large PRSS calls squeeze / upload / combine the XOF streams slice by slice (engine.prss_streamed over
    ffgpu_shake128_open / _squeeze); the one-shot path is the one pinned to the reference's vectors above.  Slices of 4 KiB
    here, so that 20 011 draws cross many slice boundaries, the last slice is partial and the two staging halves alternate;
    prime (one, two and three limbs) and binary fields, the share and the zero-sharing (d = t draws per element)."""
    import itertools
    finfields, gfpx, thresha = api
    from mpyc_amd import engine
    n, m, t = 20011, 5, 2
    for F in (finfields.GF(2**61 - 1), finfields.GF(2**128 - 173), finfields.GF(finfields.find_prime_root(136)[0]),
              finfields.GF(gfpx.BinaryPolynomial((1 << 64) | 27)), finfields.GF(gfpx.BinaryPolynomial(283))):
        for i in (0, m - 1):
            keys = {S: bytes([7 * sum(S) % 251, len(S)]) * 8 for S in itertools.combinations(range(m), m - t) if i in S}
            for bound in (F.order, 1 << 7):
                prfs = {S: thresha.PRF(k, bound) for S, k in keys.items()}
                want = ints(thresha.np_pseudorandom_share(F, m, i, prfs, b'slices', n))
                want0 = ints(thresha.np_pseudorandom_share_0(F, m, i, prfs, b'slices', n))
                with monkeypatch.context() as mp:
                    mp.setattr(thresha, 'PRSS_STREAM_MIN', 0)
                    mp.setattr(engine.FieldContext, 'PRSS_SLICE_BYTES', 4096)
                    assert ints(thresha.np_pseudorandom_share(F, m, i, prfs, b'slices', n)) == want, (F, i, bound)
                    assert ints(thresha.np_pseudorandom_share_0(F, m, i, prfs, b'slices', n)) == want0, (F, i, bound)


def test_matmul_operator(api):
    """tests/test_finfields.py:389-404: `@` on arrays over the 2^127-1 prime vs NumPy object ints."""
    finfields, gfpx, _ = api
    p = 2**127 - 1
    F = finfields.GF(p)
    rng = random.Random(11)
    A = [[rng.randrange(p) for _ in range(6)] for _ in range(4)]
    B = [[rng.randrange(p) for _ in range(5)] for _ in range(6)]
    want = (np.array(A, dtype=object) @ np.array(B, dtype=object)) % p
    C = F.array(A) @ F.array(B)
    assert C.shape == (4, 5) and [[int(v) for v in r] for r in C.value] == [[int(v) for v in r] for r in want]
    v = F.array(A[1]) @ F.array(B)
    assert v.shape == (5,) and ints(v) == [int(x) for x in want[1]]
    w = F.array(A) @ F.array([r[2] for r in B])
    assert w.shape == (4,) and ints(w) == [int(x) for x in want[:, 2]]
    d = F.array(A[0]) @ F.array([r[0] for r in B])
    assert isinstance(d, F) and int(d.value) == int(want[0, 0])
    assert ints(F.array(A) @ np.array(B, dtype=object)) == [int(x) for x in want.reshape(-1)]
    with pytest.raises(ValueError):
        F.array(A) @ F.array(A)


def test_numpy_protocol(api):
    """np.* functions and ufuncs on GPU field arrays (finfields.py:728-819 restated): results equal the same
    NumPy call on plain integer arrays reduced mod p; unsupported functions raise instead of falling back."""
    finfields, gfpx, _ = api
    p = 2**61 - 1
    F = finfields.GF(p)
    rng = random.Random(21)
    a = [[rng.randrange(p) for _ in range(5)] for _ in range(3)]
    b = [[rng.randrange(p) for _ in range(5)] for _ in range(3)]
    A, B = F.array(a), F.array(b)
    na, nb = np.array(a, dtype=object), np.array(b, dtype=object)

    def same(x, want):
        assert isinstance(x, F.array) and x.shape == want.shape, (x.shape, want.shape)
        assert [int(v) for v in np.asarray(x.value).reshape(-1)] == [int(v) % p for v in want.reshape(-1)]

    same(np.add(A, B), na + nb)
    same(np.multiply(A, B), na * nb)
    same(np.subtract(A, B), na - nb)
    same(np.negative(A), -na)
    same(np.multiply(3, A), 3 * na)
    same(np.concatenate((A, B)), np.concatenate((na, nb)))
    same(np.concatenate((A, B), axis=1), np.concatenate((na, nb), axis=1))
    same(np.stack((A, B)), np.stack((na, nb)))
    same(np.stack((A, B), axis=2), np.stack((na, nb), axis=2))
    same(np.vstack((A[0], B[1])), np.vstack((na[0], nb[1])))
    same(np.hstack((A[0], B[1])), np.hstack((na[0], nb[1])))
    same(np.transpose(A), na.T)
    same(A.T, na.T)
    same(np.reshape(A, (5, 3)), na.reshape(5, 3))
    same(np.roll(A, 2, axis=1), np.roll(na, 2, axis=1))
    same(np.roll(A, 4), np.roll(na, 4))
    same(np.flip(A, axis=0), np.flip(na, axis=0))
    same(A.T @ B, na.T @ nb)
    same(np.matmul(A, B.T), na @ nb.T)
    assert int(np.sum(A).value) == int(na.sum()) % p
    assert np.shape(A) == (3, 5) and np.ndim(A) == 2 and np.size(A) == 15
    assert (np.equal(A, A)).all() and not np.not_equal(A, A).any()
    assert [int(v) for v in np.asarray(A.value).reshape(-1)] == [v for row in a for v in row]
    assert [int(v) for v in np.cumsum(A, axis=1).value.reshape(-1)] == [int(v) % p for v in np.cumsum(na, axis=1).reshape(-1)]
    assert [int(v) for v in np.cumsum(A).value] == [int(v) % p for v in np.cumsum(na)]
    assert [int(v) for v in np.cumprod(A, axis=0).value.reshape(-1)] == [int(v) % p for v in np.cumprod(na, axis=0).reshape(-1)]
    with pytest.raises(NotImplementedError):
        np.einsum('ij->i', A)
    G = finfields.GF(2**128 - 173)                      # two-limb elements: trailing limb axis handled
    q = G.modulus
    c = [[rng.randrange(q) for _ in range(4)] for _ in range(2)]
    C = G.array(c)
    nc = np.array(c, dtype=object)
    assert [int(v) for v in np.asarray(C.T.value).reshape(-1)] == [int(v) for v in nc.T.reshape(-1)]
    assert [int(v) for v in np.asarray(np.concatenate((C, C), axis=1).value).reshape(-1)] == \
        [int(v) for v in np.concatenate((nc, nc), axis=1).reshape(-1)]
    assert [int(v) for v in np.asarray(np.roll(C, 1, axis=1).value).reshape(-1)] == \
        [int(v) for v in np.roll(nc, 1, axis=1).reshape(-1)]


def test_small_matrix_over_last_axis(api):
    """`A @ x[..., np.newaxis]` (demos/np_aes.py:40): public 8x8 matrix over a batch of 8-vectors."""
    import functools
    from oracle.pyoracle import Field, mul
    finfields, gfpx, _ = api
    F = finfields.GF(gfpx.GFpX(2)(0x11b))
    rng = random.Random(5)
    A = [[rng.randrange(256) for _ in range(8)] for _ in range(8)]
    x = [[rng.randrange(256) for _ in range(8)] for _ in range(300)]
    y = F.array(A) @ F.array(x).reshape(300, 8, 1)
    assert y.shape == (300, 8, 1)
    Fo = Field(0x11b, True)
    want = [functools.reduce(lambda s, c: s ^ mul(Fo, A[r][c], row[c]), range(8), 0) for row in x for r in range(8)]
    assert ints(y) == want


def test_linalg_golden(api):
    """np.linalg.det / inv / solve / matrix_power on GPU field arrays vs the reference's outputs
    (tests/test_finfields.py:405-431 use the same entry points)."""
    import json
    import os
    finfields, gfpx, _ = api
    g = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'linalg.json')))
    for name, fc in g.items():
        modulus = int(fc['modulus'], 16)
        F = finfields.GF(gfpx.BinaryPolynomial(modulus)) if fc['binary'] else finfields.GF(modulus)
        red = lambda v: int(v, 16) if fc['binary'] else int(v, 16) % modulus
        mat = lambda m: [[red(v) for v in row] for row in m]
        for c in fc['cases']:
            a = F.array(mat(c['A']))
            d = np.linalg.det(a)
            assert isinstance(d, F) and int(d) % F.order == red(c['det']) % F.order if not fc['binary'] else int(d) == red(c['det'])
            assert ints(np.linalg.matrix_power(a, 5)) == [v for row in mat(c['pow5']) for v in row], (name, c['kind'])
            if 'error' in c:
                with pytest.raises(ZeroDivisionError, match='no inverse exists'):
                    np.linalg.inv(a)
                continue
            assert ints(np.linalg.inv(a)) == [v for row in mat(c['inv']) for v in row]
            x = np.linalg.solve(a, F.array(mat(c['B'])))
            assert x.shape == (c['n'], 2) and ints(x) == [v for row in mat(c['solve']) for v in row]
            assert ints(np.linalg.matrix_power(a, -3)) == [v for row in mat(c['pow_m3']) for v in row]
            assert ints(a @ np.linalg.inv(a)) == [int(i == j) for i in range(c['n']) for j in range(c['n'])]
        st = F.array([mat(m) for m in fc['stack']]).reshape(2, 2, 3, 3)
        dets = np.linalg.det(st)
        assert dets.shape == (2, 2) and ints(dets) == [red(v) for row in fc['stack_det'] for v in row]
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.det(F.array([[1, 2, 3], [4, 5, 6]]))
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.inv(F.array([[1, 2, 3], [4, 5, 6]]))


def test_numpy_functions_golden(api):
    """convolve / outer / prod / trace / sum(axis) on GPU field arrays vs the reference's outputs."""
    import json
    import os
    finfields, gfpx, _ = api
    g = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'npfuncs.json')))
    for name, c in g.items():
        modulus = int(c['modulus'], 16)
        F = finfields.GF(gfpx.BinaryPolynomial(modulus)) if c['binary'] else finfields.GF(modulus)
        red = lambda v: int(v, 16) if c['binary'] else int(v, 16) % modulus
        L = lambda key: [red(v) for v in c[key]]
        a, v, m = F.array(L('a')), F.array(L('v')), F.array([[red(x) for x in row] for row in c['m']])
        assert ints(np.convolve(a, v)) == L('conv_full'), name
        assert ints(np.convolve(a, v, 'same')) == L('conv_same')
        assert ints(np.convolve(a, v, 'valid')) == L('conv_valid')
        assert ints(np.convolve(v, a)) == L('conv_swapped')
        o = np.outer(a, v)
        assert o.shape == (9, 4) and ints(o) == L('outer')
        val = lambda e: int(e) % modulus if not c['binary'] else int(e)
        assert val(np.prod(a)) == red(c['prod']) and val(m.prod()) == red(c['prod_m'])
        assert val(np.trace(m)) == red(c['trace']) and val(np.sum(m)) == red(c['sum'])
        assert ints(np.sum(m, axis=0)) == L('sum0') and ints(m.sum(axis=1)) == L('sum1')


def test_numpy_movement_functions(api):
    """Pure data-movement NumPy functions: the reference applies NumPy to the object array
    (finfields.py:766-819), so NumPy on the plain values is the expected result."""
    finfields, gfpx, _ = api
    rng = random.Random(9)
    for F in (finfields.GF(2**61 - 1), finfields.GF(gfpx.GFpX(2)(0x11b)), finfields.GF(2**127 - 1)):
        q = F.order
        A = np.array([[rng.randrange(q) for _ in range(4)] for _ in range(3)], dtype=object)
        B = np.array([[rng.randrange(q) for _ in range(4)] for _ in range(3)], dtype=object)
        v = np.array([rng.randrange(q) for _ in range(5)], dtype=object)
        a, b, w = F.array(A), F.array(B), F.array(v)

        def same(got, want):
            want = np.asarray(want, dtype=object)
            assert got.shape == want.shape, (got.shape, want.shape)
            assert ints(got) == [int(x) for x in want.reshape(-1)]

        same(np.tile(a, (2, 3)), np.tile(A, (2, 3)))
        same(np.repeat(a, 2, axis=1), np.repeat(A, 2, axis=1))
        same(np.tril(a), np.tril(A))
        same(np.triu(a, 1), np.triu(A, 1))
        same(np.diag(w), np.diag(v))
        same(np.diag(a), np.diag(A))
        same(np.diagonal(a, 1), np.diagonal(A, 1))
        same(np.block([[a, b], [b, a]]), np.block([[A, B], [B, A]]))
        same(np.dstack((a, b)), np.dstack((A, B)))
        same(np.column_stack((w, w)), np.column_stack((v, v)))
        same(np.take(a, [0, 3, 5, 11]), np.take(A, [0, 3, 5, 11]))
        same(np.delete(w, 2), np.delete(v, 2))
        same(np.append(w, [1, 2]), np.append(v, [1, 2]))
        same(np.rot90(a), np.rot90(A))
        same(np.swapaxes(a, 0, 1), np.swapaxes(A, 0, 1))
        same(np.expand_dims(w, 0), np.expand_dims(v, 0))
        same(np.pad(w, (1, 2)), np.pad(v, (1, 2)))
        same(np.where(np.arange(12).reshape(3, 4) % 2 == 0, a, b), np.where(np.arange(12).reshape(3, 4) % 2 == 0, A, B))
        same(np.broadcast_to(w, (2, 5)), np.broadcast_to(v, (2, 5)))
        parts = np.hsplit(a, 2)
        assert isinstance(parts, (list, tuple)) and len(parts) == 2
        same(parts[1], np.hsplit(A, 2)[1])
        same(np.concatenate((a, [[1, 2, 3, 4]]), axis=0), np.concatenate((A, [[1, 2, 3, 4]]), axis=0))
        z = F.array([0, 3, 0, 7])
        assert list(np.flatnonzero(z)) == [1, 3] and np.count_nonzero(z) == 2 and np.any(z) and not np.all(z)
        assert np.array_equal(a, F.array(A)) and not np.array_equal(a, b)
        with pytest.raises(NotImplementedError):
            np.einsum('ij->i', a)


def test_sqrt_p_1_mod_4_golden(api):
    """sqrt / inverse sqrt / is_sqr for primes p = 1 mod 4 (Cipolla-Lehmer) vs the reference's outputs,
    including its values for zero and for non-residues."""
    import json
    import os
    finfields, _, _ = api
    g = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'sqrt.json')))
    for name, c in g.items():
        p = int(c['modulus'], 16)
        assert p % 4 == 1
        F = finfields.GF(p)
        a = F.array([int(v, 16) for v in c['a']])
        assert ints(a.sqrt()) == [int(v, 16) for v in c['sqrt']], name
        assert ints(np.sqrt(a)) == [int(v, 16) for v in c['sqrt']]
        assert [bool(b) for b in a.is_sqr()] == c['is_sqr']
        sq = F.array([int(v, 16) for v in c['sq']])
        assert ints(sq.sqrt(INV=True)) == [int(v, 16) for v in c['inv_sqrt']], name
        r = sq.sqrt()
        assert ints(r * r) == ints(sq)
        with pytest.raises(ZeroDivisionError):
            F.array([1, 0]).sqrt(INV=True)


@pytest.mark.parametrize('p', [2**31 - 19, 2**64 - 59, 2**80 - 143, 2**100 - 15, 2**136 - 243], ids=hex)
def test_sqrt_p_1_mod_4_shapes_against_integers(api, p):
    """a.sqrt(), np.sqrt(a), a.sqrt(INV=True) and a.is_sqr() through k_sqrt_cl on one field per storage size (4, 8, 12, 16 and
    24 bytes): a (3, 5) array, an empty one and a single element, against oracle.pyoracle.sqrt_prime (the root the reference
    returns, and its value for a non-residue), its modular inverse, and Euler's criterion on Python integers"""
    import ew_contract as ew
    from oracle import pyoracle as po
    finfields, _, _ = api
    eb = {m: b for m, _, b in ew.sqrt_fields()}[p]
    assert eb == {2**31 - 19: 4, 2**64 - 59: 8, 2**80 - 143: 12, 2**100 - 15: 16, 2**136 - 243: 24}[p]
    F, G = finfields.GF(p), po.Field(p, False)
    rng = random.Random(p % 997)
    inv4 = pow(4, -1, p)
    vals = [0, 1, p - 1, inv4, 9 * inv4 % p, 4, 2, 3] + [rng.randrange(1, p) for _ in range(7)]
    root = lambda vs: [po.sqrt_prime(G, v) for v in vs]
    euler = lambda vs: [v == 0 or pow(v, (p - 1) >> 1, p) == 1 for v in vs]
    assert True in euler(vals[5:]) and False in euler(vals[5:])
    a = F.array(vals).reshape(3, 5)
    for r in (a.sqrt(), np.sqrt(a)):
        assert r.shape == (3, 5) and ints(r) == root(vals)
    assert a.is_sqr().shape == (3, 5) and [bool(b) for b in a.is_sqr().reshape(-1)] == euler(vals)
    assert ints(a) == vals, 'sqrt wrote its operand'
    with pytest.raises(ZeroDivisionError):
        a.sqrt(INV=True)
    nz = vals[1:] + [5]
    b = F.array(nz).reshape(3, 5)
    r = b.sqrt(INV=True)
    assert r.shape == (3, 5) and ints(r) == [pow(v, -1, p) for v in root(nz)]
    empty = F.array([])
    for r in (empty.sqrt(), np.sqrt(empty), empty.sqrt(INV=True)):
        assert r.shape == (0,) and ints(r) == []
    assert empty.is_sqr().shape == (0,)
    for v in (inv4, vals[9], 0):                    # a single element, taken out of the array: no axis left
        one = F.array([v, 1])[0:1].reshape(())
        assert one.shape == () and ints(one.sqrt()) == root([v]) and ints(np.sqrt(one)) == root([v])
        assert [bool(x) for x in np.asarray(one.is_sqr()).reshape(-1)] == euler([v])
        if v:
            assert ints(one.sqrt(INV=True)) == [pow(root([v])[0], -1, p)]
        else:
            with pytest.raises(ZeroDivisionError):
                one.sqrt(INV=True)


def test_twelve_byte_field_through_the_mirror(api):
    """SecInt(64)'s field size (96-bit Blum-like prime 2^96 - 17 and the 80-bit 2^80 - 65): elements live in
    12 bytes on the device (3 x uint32); everything the mirror does with limb tensors must handle the
    3-limb trailing axis: indexing, broadcasting, NumPy movement, linear algebra, wire format, sharing."""
    finfields, _, thresha = api
    rng = random.Random(96)
    for p in (2**96 - 17, 2**80 - 65):
        F = finfields.GF(p)
        assert F.array([1]).ctx.elem_bytes == 12
        a = [[rng.randrange(p) for _ in range(5)] for _ in range(4)]
        b = [[rng.randrange(p) for _ in range(5)] for _ in range(4)]
        A, B = F.array(a), F.array(b)
        na, nb = np.array(a, dtype=object), np.array(b, dtype=object)

        def same(got, want):
            want = np.asarray(want, dtype=object) % p
            assert got.shape == want.shape
            assert ints(got) == [int(v) for v in want.reshape(-1)]

        same(A * B + A - B, na * nb + na - nb)
        same(-A, -na)
        same(A * 3 + 7, na * 3 + 7)
        same(A + F.array(b[0]), na + nb[0])                                   # broadcasting
        same(A[1:3, ::2], na[1:3, ::2])
        assert int(A[2, 3].value) == a[2][3]
        C = A.copy()
        C[0] = B[1]
        C[3, 4] = -1
        nc = na.copy()
        nc[0] = nb[1]
        nc[3, 4] = p - 1
        same(C, nc)
        same(A.T @ B, na.T @ nb)
        same(np.concatenate((A, B), axis=1), np.concatenate((na, nb), axis=1))
        same(np.tile(A, (2, 1)), np.tile(na, (2, 1)))
        same(np.tril(A), np.tril(na))
        same(np.sum(A, axis=0), na.sum(axis=0))
        same((A ** 5).reshape(-1), (na ** 5).reshape(-1))
        assert ints(A.reciprocal() * A) == [1] * 20
        assert (A == F.array(a)).all() and not (A == B).all()
        S = F.array([[rng.randrange(p) for _ in range(4)] for _ in range(4)])
        assert ints(S @ np.linalg.inv(S)) == [int(i == j) for i in range(4) for j in range(4)]
        # wire format (finfields.py:91-102): byte_length bytes per element; for the 96-bit prime = the device bytes
        w = A.to_wire()
        assert F.byte_length == (p.bit_length() + 7) // 8
        assert w == b''.join(int(v).to_bytes(F.byte_length, 'little') for row in a for v in row)
        same(F.array.from_wire(w, shape=(4, 5)), na)
        # sharing round trip through the public API (device CSPRNG) and through the randbelow hook
        s = F.array([rng.randrange(p) for _ in range(1000)])
        sh = thresha.np_random_split(F, s, 2, 5)
        back = thresha.np_recombine(F, [(x, sh[x - 1]) for x in (5, 1, 3)])
        assert ints(back) == ints(s)
        # negative / oversized host inputs reduce like the reference (finfields.py:724)
        same(F.array([-1, p, p + 5, 2**200 + 3]), np.array([p - 1, 0, 5, (2**200 + 3) % p], dtype=object))


def test_recombine_multiply_split_chain_stays_in_registers(api):
    """np_recombine defers; `y * y` / `y * z` of deferred recombinations defers; np_random_split of that
    issues ONE fused kernel (ffgpu_gate_rng) and never materialises y.  Results equal plain arithmetic, and
    every other use of a deferred array materialises it transparently."""
    finfields, gfpx, thresha = api
    rng = random.Random(77)
    for F, t, m in ((finfields.GF(2**61 - 1), 1, 3), (finfields.GF(2**96 - 17), 2, 5),
                    (finfields.GF(gfpx.GFpX(2)(0x11b)), 1, 3)):
        q = F.order
        n = 3001
        a = [rng.randrange(q) for _ in range(n)]
        b = [rng.randrange(q) for _ in range(n)]
        A, B = F.array(a), F.array(b)
        k = 2 * t + 1
        sa = thresha.np_random_split(F, A, t, m)
        sb = thresha.np_random_split(F, B, t, m)
        # party 1's view of a multiplication chain: recombine the rows it "received", square, re-share
        y = thresha.np_recombine(F, [(x, sa[x - 1]) for x in range(1, t + 2)])
        z = thresha.np_recombine(F, [(x, sb[x - 1]) for x in range(1, t + 2)])
        assert y._take_lazy_product() is not None and y._devv is None          # deferred
        sq = y * y
        sh = thresha.np_random_split(F, sq, t, m)                             # fused chain gate
        assert y._devv is None and sq._devv is None                            # nothing was materialised
        back = thresha.np_recombine(F, [(x, sh[x - 1]) for x in range(1, t + 2)])
        assert ints(back) == ints(A * A)
        yz = thresha.np_random_split(F, y * z, t, m)
        assert y._devv is None and z._devv is None
        assert ints(thresha.np_recombine(F, [(x, yz[x - 1]) for x in range(m, m - t - 1, -1)])) == ints(A * B)
        mixed = thresha.np_random_split(F, y * B, t, m)                       # one deferred, one plain operand
        assert ints(thresha.np_recombine(F, [(x, mixed[x - 1]) for x in range(1, t + 2)])) == ints(A * B)
        # any other use materialises: arithmetic, indexing, .value, in-place updates of a row
        assert ints(y + 1) == ints(A + 1) and y._devv is not None
        assert int(z[5].value) == b[5] and z._devv is not None
        w = thresha.np_recombine(F, [(x, sa[x - 1]) for x in range(1, t + 2)])
        p = w * w
        row = sa[0]
        row += 1                                                               # mutates a row w still reads
        assert ints(p) == ints(A * A)                                          # ... after p was flushed
    # parity mode (randbelow hook) never takes the fused path but still accepts deferred operands
    F = finfields.GF(2**61 - 1)
    A = F.array([3, 5, 7, 11])
    sa = thresha.np_random_split(F, A, 1, 3)
    y = thresha.np_recombine(F, [(1, sa[0]), (2, sa[1])])
    draws = iter(range(100, 200))
    thresha.randbelow = lambda order: next(draws)
    try:
        sh = thresha.np_random_split(F, y * y, 1, 3)
    finally:
        thresha.randbelow = None
    assert ints(sh[0]) == [(v * v + 100 + i) % F.order for i, v in enumerate([3, 5, 7, 11])]


def test_sum_along_an_axis_regimes(api):
    """np.sum(a, axis): short rows (one thread per row), many long rows (matrix x ones), few long rows (one
    reduction per row), for scalar-limb, 3-limb and 2-limb fields and for every axis of a 3-D array."""
    finfields, gfpx, _ = api
    rng = np.random.default_rng(11)
    for F in (finfields.GF(2**61 - 1), finfields.GF(2**96 - 17), finfields.GF(2**127 - 1), finfields.GF(gfpx.GFpX(2)(0x11b))):
        q = F.order
        binary = not isinstance(F.modulus, int)
        for shape in ((300, 9), (100, 40), (5, 700), (6, 5, 33)):
            vals = np.array([int(v) % q for v in rng.integers(0, 2**62, size=int(np.prod(shape)))], dtype=object).reshape(shape)
            a = F.array(vals)
            for ax in range(len(shape)):
                got = np.sum(a, axis=ax)
                if binary:
                    want = np.bitwise_xor.reduce(vals.astype(np.int64), axis=ax)
                else:
                    want = vals.sum(axis=ax) % q
                assert got.shape == want.shape, (shape, ax)
                assert ints(got) == [int(v) for v in np.asarray(want, dtype=object).reshape(-1)], (F.order, shape, ax)


def test_mirror_calls_in_a_hip_graph(api):
    """With thresha.device_rng_state the mirror's share generation reads a device-resident generator state, so
    a sequence of mirror calls (a gate: product, share generation, recombination) can be captured once and
    replayed: same opened values, fresh shares on every replay."""
    finfields, _, thresha = api
    from mpyc_amd.engine import CapturedLaunches
    F = finfields.GF(2**61 - 1)
    rng = random.Random(4)
    n = 4096
    a = [rng.randrange(F.order) for _ in range(n)]
    b = [rng.randrange(F.order) for _ in range(n)]
    A, B = F.array(a), F.array(b)
    thresha.device_rng_state = True
    try:
        def gate():
            sh = thresha.np_random_split(F, A * B, 1, 3)
            y = thresha.np_recombine(F, [(1, sh[0]), (3, sh[2])])
            return sh, y + 0                       # `+ 0` materialises the deferred recombination inside the graph
        cg = CapturedLaunches(gate)
        seen = []
        for _ in range(3):
            cg.replay()
            torch.cuda.synchronize()
            sh, y = cg.result
            assert ints(y) == [u * v % F.order for u, v in zip(a, b)]
            seen.append(ints(sh[0])[:8])
        assert seen[0] != seen[1] != seen[2]
    finally:
        thresha.device_rng_state = False


@pytest.mark.gpu
def test_deferred_products_never_see_later_in_place_updates_through_aliases(api):
    """A deferred `a * b` must be evaluated from the operands as they were when it was written, also when the
    later in-place update goes through an ALIAS of an operand (a basic-slice view, a row of a share matrix, the
    materialised value of a deferred recombination) -- the reference is eager NumPy and never does otherwise."""
    finfields, gfpx, thresha = api
    F = finfields.GF(2**61 - 1)
    p = F.order
    a = [(7 * i + 3) % p for i in range(50)]
    b = [(11 * i + 5) % p for i in range(50)]
    want = [x * y % p for x, y in zip(a, b)]
    # (1) update through an offset view of an operand
    A, B = F.array(a), F.array(b)
    c = A * B
    v = A[2:]
    v += 1
    assert ints(c) == want
    assert ints(A)[2:] == [(x + 1) % p for x in a[2:]] and ints(A)[:2] == a[:2]
    # (2) product of a view, then item assignment into the base array
    A = F.array(a)
    c2 = A[2:] * B[2:]
    A[3] = 0
    assert ints(c2) == want[2:]
    # (3) a deferred recombination that has been materialised, squared lazily, then updated in place
    t, m = 1, 3
    sh = thresha.np_random_split(F, F.array(a), t, m)
    X = thresha.np_recombine(F, [(x, sh[x - 1]) for x in range(1, t + 2)])
    assert ints(X) == a                                  # materialises the recombination
    Y = X * X
    X += 1
    assert ints(Y) == [x * x % p for x in a]
    assert ints(X) == [(x + 1) % p for x in a]
    # the fused path (share generation of a deferred product) sees the same values
    X2 = thresha.np_recombine(F, [(x, sh[x - 1]) for x in range(1, t + 2)])
    Y2 = X2 * X2
    row = sh[0]
    row *= 2                                             # a row X2 still reads
    s2 = thresha.np_random_split(F, Y2, t, m)
    assert ints(thresha.np_recombine(F, [(x, s2[x - 1]) for x in range(1, t + 2)])) == [x * x % p for x in a]


@pytest.mark.gpu
def test_matmul_scratch_is_per_stream():
    """Two streams issue matrix-core products of DIFFERENT sizes on one context back to back (the second, larger
    one makes its stream's scratch grow): each stream has its own digit-plane scratch, so neither product reads
    planes the other is writing, and growing one buffer never frees memory the other stream still uses."""
    import torch
    from mpyc_amd.engine import DevArray, FieldContext
    p = 2**61 - 1
    ctx = FieldContext(p, device=0)
    gen = torch.Generator(device='cuda:0')
    gen.manual_seed(5)

    def rnd(n):
        return DevArray(ctx, (torch.randint(0, 2**62, (n,), dtype=torch.int64, device='cuda:0', generator=gen) >> 1) % p, n)
    shapes = [(512, 512, 512), (768, 1024, 640)]
    ops = [(rnd(M * K), rnd(K * N)) for (M, K, N) in shapes]
    want = [ctx.matmul(a, b, M, K, N).t.clone() for (a, b), (M, K, N) in zip(ops, shapes)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [ctx.empty(M * N) for (M, K, N) in shapes]
    for rep in range(6):
        with torch.cuda.stream(s1):
            ctx.matmul(ops[0][0], ops[0][1], *shapes[0], out=outs[0])
        with torch.cuda.stream(s2):
            ctx.matmul(ops[1][0], ops[1][1], *shapes[1], out=outs[1])
    torch.cuda.synchronize()
    assert torch.equal(outs[0].t, want[0]) and torch.equal(outs[1].t, want[1])
    with torch.cuda.stream(s1):
        d1 = ctx.dot(ops[0][0], ops[0][0])
    with torch.cuda.stream(s2):
        d2 = ctx.dot(ops[1][0], ops[1][0])
    torch.cuda.synchronize()
    assert d1.to_ints() == ctx.dot(ops[0][0], ops[0][0]).to_ints() and d2.to_ints() == ctx.dot(ops[1][0], ops[1][0]).to_ints()


def test_scalar_comparisons_of_large_arrays_uniform_masks(api):
    """Round 6: `a == c` / `a != c` of a large array against a scalar -- np_random_bits' `_r2.value != 0` over f x n opened
    squares (runtime.py:4257) -- is decided on the device by the lowest limb; when no element matches, the result is a
    uniform mask (a zero-stride boolean ndarray: nothing mask-sized is built or copied).  Same values as the elementwise
    comparison in every case: no match, one match, a match of the lowest limb only, negative / out-of-range scalars,
    2-D shapes, every storage width; and what the runtime does with the mask (count_nonzero, boolean indexing, ~)."""
    finfields, gfpx, _ = api
    rng = np.random.default_rng(77)
    for modulus in (2**61 - 1, 2**64 - 189, 2**31 - 1, 2**80 - 65, 2**128 - 173, 2**136 - 113):
        F = finfields.GF(modulus)
        n = (1 << 16) + 37
        vals = [int(v) % modulus or 1 for v in rng.integers(1, 2**63, size=n, dtype=np.int64)]
        if modulus > 2**64:
            vals = [(v * 0x9E3779B97F4A7C15F39CC0605CEDC835 + 12345) % modulus or 1 for v in vals]
        a = F.array(vals)
        ref = np.array(vals, dtype=object)
        for c in (0, modulus, -modulus):                                   # no element is 0 (mod p)
            eq, ne = (a == c), (a != c)
            assert isinstance(eq, np.ndarray) and eq.dtype == np.bool_ and eq.shape == (n,)
            assert type(eq).__name__ == '_UniformMask' and not eq.any() and ne.all()
            assert np.count_nonzero(ne) == n and np.count_nonzero(eq) == 0 and int(np.sum(ne)) == n
            assert np.asarray(a.value)[ne].shape == (n,) and np.asarray(a.value)[eq].shape == (0,)
            assert np.array_equal(np.asarray(~ne), np.zeros(n, dtype=bool))
        hit = vals[1234]
        eq = a == hit
        assert type(eq) is np.ndarray and np.array_equal(eq, ref == hit) and eq[1234]
        assert np.array_equal(a != hit, ref != hit)
        assert np.array_equal(a == hit - modulus, ref == hit)               # scalars are reduced (finfields.py:1045-1054)
        lim = 2**32 if F.array([0]).ctx.elem_bytes in (4, 12) else 2**64
        if modulus > lim:                                                  # same lowest limb, different element
            near = (hit + lim) % modulus
            if near not in vals:
                assert not (a == near).any() and type(a == near) is np.ndarray
        b = a.reshape(37 + (1 << 16) // 1, 1) if False else a[:1 << 16].reshape(256, 256)
        assert (b != 0).shape == (256, 256) and np.count_nonzero(b != 0) == 1 << 16
        small = F.array(vals[:100])
        assert type(small == 0) is np.ndarray and not (small == 0).any()    # below the threshold: the ordinary path
    from mpyc_amd.finfields import _UniformMask
    m = _UniformMask((3, 4), True)
    assert (m & np.eye(3, 4, dtype=bool)).sum() == 3 and type(m & m) is np.ndarray and np.count_nonzero(m[1:]) == 8


def test_public_operand_uploads_are_keyed_by_content(api):
    """Round 6: a large public integer array used with share arrays several times in a row (np_sgn's bit matrix,
    runtime.py:3663-3671) is converted and uploaded once -- the cache is keyed by a digest of the CONTENT: an array updated
    in place between two uses must give the new values, and what a caller does to a result must not reach the cache."""
    finfields, _, _ = api
    from mpyc_amd.finfields import HostView, _PUBLIC_UPLOADS
    F = finfields.GF(2**64 - 189)
    n = (1 << 16) + 5
    rng = np.random.default_rng(3)
    a = F.array([int(v) for v in rng.integers(0, 2**62, size=n)])
    bits = rng.integers(0, 2, size=n).astype(np.int8)
    v = HostView(a, lazy=True)
    want = np.asarray(a.value).astype(object)
    _PUBLIC_UPLOADS.clear()
    s1 = (bits + v)._real()
    assert len(_PUBLIC_UPLOADS) == 1 and (s1 == (want + bits.astype(object)) % F.order).all()
    p1 = (bits * v)._real()
    assert len(_PUBLIC_UPLOADS) == 1 and (p1 == (want * bits.astype(object)) % F.order).all()        # second use: a hit
    bits[:100] ^= 1                                                                                   # in-place update
    s2 = (bits + v)._real()
    assert len(_PUBLIC_UPLOADS) == 2 and (s2 == (want + bits.astype(object)) % F.order).all()
    d = v - bits                                    # a result updated in place by its owner ...
    r = F.array(bits)                               # (ordinary construction: not through the cache)
    r += 5
    s3 = (bits + v)._real()                       # ... and the cached operand still holds the values of `bits`
    assert (s3 == s2).all() and (d._real() == (want - bits.astype(object)) % F.order).all()


def _contract_fields():
    import ew_contract
    return ew_contract.contract_fields()


@pytest.mark.parametrize('modulus,binary', _contract_fields(), ids=[('gf2:' if b else '') + hex(m) for m, b in _contract_fields()])
def test_in_place_operators_on_aliased_operands(api, modulus, binary):
    """A *= A, A += A, A -= A (ctx.mul(a, a, out=a), ...) and the scalar forms in place, on every field policy, against the
    Python-integer oracle; the right operand of A *= B is left as it was (include/ffgpu.h: inputs are never written, `out` may
    alias an input; tests/test_gpu_elementwise_contract.py checks the same at the C ABI)."""
    from oracle import pyoracle as po
    finfields, gfpx, _ = api
    F = finfields.GF(gfpx.BinaryPolynomial(modulus)) if binary else finfields.GF(modulus)
    Fo = po.Field(modulus, binary)
    q = Fo.order
    r = random.Random(modulus % 1009)
    n = 1025
    a, b = [r.randrange(q) for _ in range(n)], [r.randrange(q) for _ in range(n)]
    a[:3] = [0, 1, q - 1]
    s = r.randrange(q)

    def imul(x, y):
        x *= y
        return x

    def iadd(x, y):
        x += y
        return x

    def isub(x, y):
        x -= y
        return x
    for op, ref in ((imul, po.mul), (iadd, po.add), (isub, po.sub)):
        A = F.array(a)
        got = op(A, A)
        assert got is A and ints(A) == [ref(Fo, x, x) for x in a], (hex(modulus), ref.__name__, 'A op= A')
        A = F.array(a)
        got = op(A, s)
        assert got is A and ints(A) == [ref(Fo, x, s) for x in a], (hex(modulus), ref.__name__, 'A op= s')
    A, B = F.array(a), F.array(b)
    A *= B
    assert ints(B) == b and ints(A) == [po.mul(Fo, x, y) for x, y in zip(a, b)]
