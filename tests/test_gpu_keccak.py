"""Threshold SHA-3 on the device (mpyc_amd/csrc/keccak.hpp; engine.FieldContext.keccak_local / keccak_round; protocols.
keccak_f1600 / sha3 / shake): keccak_local byte for byte against the numpy stand-in written from the map
(tests/keccak_cpuctx.py) on every path, between guard bytes, and every refusal with nothing written; keccak_round's shares
recombine to keccak_local's output from every (t+1)-subset, draw fresh and uniform coefficients, and do not depend on the
batch size; the 24-round chain in one HIP graph; the digests against hashlib and the reference's fixture."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import keccak_cpuctx as kc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
B = 1600
STATES_PER_WG = 16
GUARD = 0xA5
KEY = bytes(range(32))


@pytest.fixture(scope='module')
def mods():
    assert torch.cuda.is_available()
    from mpyc_amd import engine, finfields, gfpx, protocols
    return engine, finfields, gfpx, protocols


def field_of(mods, modulus):
    _, finfields, gfpx, _ = mods
    return finfields.GF(gfpx.GFpX(2)(modulus))


def dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def rows_on_device(engine, ctx, data: np.ndarray, pad: int = 36, lead: int = 4):
    """data (nrows, n) -> one device buffer with the rows `n + pad` bytes apart, the first `lead` bytes in; returns
    (buffer, rows as DevArray views, pitch)"""
    nrows, n = data.shape
    pitch = n + pad
    host = np.full(lead + nrows * pitch + 8, GUARD, dtype=np.uint8)
    for i in range(nrows):
        host[lead + i * pitch:lead + i * pitch + n] = data[i]
    buf = dev(host)
    return buf, [engine.DevArray(ctx, buf[lead + i * pitch:lead + i * pitch + n], n) for i in range(nrows)], pitch


def guarded_matrix(engine, ctx, rows: int, n: int, pad: int = 28, lead: int = 64):
    pitch = n + pad
    buf = torch.full((2 * lead + rows * pitch,), GUARD, dtype=torch.uint8, device='cuda:0')
    return buf, engine.DevMatrix(ctx, buf[lead:lead + rows * pitch].view(rows, pitch), rows, n, pitch)


def check_guards(buf, rows: int, n: int, pad: int = 28, lead: int = 64):
    """everything outside the rows' first n bytes is untouched; returns the (rows, n) payload"""
    host = buf.cpu().numpy()
    body = host[lead:lead + rows * (n + pad)].reshape(rows, n + pad)
    assert (host[:lead] == GUARD).all() and (host[lead + rows * (n + pad):] == GUARD).all() and (body[:, n:] == GUARD).all()
    return body[:, :n]


def recombined(T, data, lam):
    acc = np.zeros(data.shape[1], dtype=np.uint8)
    for row, l in zip(data, lam):
        acc ^= T[l][row]
    return acc


# Lagrange-like scalars per field, the first k taken: non-trivial, and distinct where the field has seven nonzero values
LAMS = {2: [3, 2, 1, 2, 3, 1, 3], 3: [3, 5, 7, 1, 2, 4, 6], 8: [0x53, 0xca, 0x02, 0xff, 0x8d, 0x1b, 0x80]}


@pytest.mark.parametrize('e', [2, 3, 8])
def test_keccak_local_is_the_map_byte_for_byte(mods, e):
    """whole-field random bytes; nstates 1..33 (one state to two workgroups and a state); k in {1, 3, 7}; iota in front of
    rounds -1, 0, 23; with and without the round; three senders in one launch; padded pitches, a base 4 bytes in; guards"""
    engine = mods[0]
    modulus = kc.IRREDUCIBLE[e]
    ctx = engine.FieldContext(modulus, True, device=0)
    T, rng = kc.mul_table(modulus), np.random.default_rng(e)
    combos = list(itertools.product((1, 3, 7), (-1, 0, 23), (False, True)))
    cases = [(ns, combos[(5 * ns) % len(combos)], 1) for ns in range(1, 2 * STATES_PER_WG + 2)]
    cases += [(ns, c, nb) for ns, nb in ((1, 1), (17, 3), (33, 2)) for c in combos]
    for nstates, (k, iota, apply_round), nbatch in cases:
        n = B * nstates
        data = rng.integers(0, 1 << e, size=(nbatch * k, n), dtype=np.uint8)
        lam = LAMS[e][:k]
        buf, rows, pitch = rows_on_device(engine, ctx, data)
        before = buf.clone()
        gbuf, out = guarded_matrix(engine, ctx, nbatch, n)
        res = ctx.keccak_local(rows[:k], lam, nstates, iota_round=iota, apply_round=apply_round, nbatch=nbatch, stride_in=k * pitch,
                               out=out)
        assert res is out
        got = check_guards(gbuf, nbatch, n)
        assert torch.equal(buf, before)
        for y in range(nbatch):
            want = kc.keccak_map(T, recombined(T, data[y * k:(y + 1) * k], lam).reshape(nstates, B), iota, apply_round).reshape(n)
            assert (got[y] == want).all(), (nstates, k, iota, apply_round, y)


def test_refusals_write_nothing(mods):
    engine = mods[0]
    ctx = engine.FieldContext(0b111, True, device=0)
    n = B * 2
    data = np.random.default_rng(1).integers(0, 4, size=(8, n), dtype=np.uint8)
    buf, rows, pitch = rows_on_device(engine, ctx, data)
    gbuf, out = guarded_matrix(engine, ctx, 21, n)

    def untouched():
        assert (gbuf.cpu().numpy() == GUARD).all()

    def off_by_two(a):
        return engine.DevArray(ctx, torch.as_strided(a.t, (n,), (1,), a.t.storage_offset() + 2), n)

    def refused(fn):
        with pytest.raises(NotImplementedError):
            fn()
        untouched()

    refused(lambda: ctx.keccak_local(rows, [1] * 8, 2, out=out))                                      # k > 7
    refused(lambda: ctx.keccak_local(rows[:1], [1], 2, iota_round=24, out=out))
    refused(lambda: ctx.keccak_local(rows[:1], [1], 2, iota_round=-2, out=out))
    refused(lambda: ctx.keccak_local([off_by_two(rows[0])], [1], 2, out=out))                         # row pointer
    refused(lambda: ctx.keccak_local(rows[:1], [1], 2, nbatch=2, stride_in=pitch + 2, out=out))       # stride
    refused(lambda: ctx.keccak_local(rows[:1], [1], 2, out=engine.DevMatrix(ctx, out.t[:, 2:], 1, n, out.stride)))
    refused(lambda: ctx.keccak_local(rows[:1], [1], 2, nbatch=2, stride_in=pitch, out=engine.DevMatrix(ctx, gbuf[64:64 + 2 * (n + 30)].view(2, n + 30), 2, n, n + 30)))
    for m, t in ((2, 0), (4, 2), (8, 1), (6, 3), (8, 3)):                                             # (m, t) not listed
        refused(lambda: ctx.keccak_round(rows[:1], [1], 2, t, m, key=KEY, out=engine.DevMatrix(ctx, out.t, m * (2 * t + 1), n, out.stride)))
    refused(lambda: ctx.keccak_round(rows[:1], [1], 2, 1, 4, stride_in=pitch, key=KEY, out=out))                       # GF(4): no fourth point
    refused(lambda: ctx.keccak_round(rows, [1] * 8, 2, 1, 3, key=KEY, out=out))
    refused(lambda: ctx.keccak_round(rows[:1], [1], 2, 1, 3, iota_round=24, key=KEY, out=out))
    refused(lambda: ctx.keccak_round([off_by_two(rows[0])], [1], 2, 1, 3, stride_in=pitch, key=KEY, out=out))
    refused(lambda: ctx.keccak_round(rows[:1], [1], 2, 1, 3, stride_in=pitch + 1, key=KEY, out=out))
    refused(lambda: ctx.keccak_round(rows[:1], [1], 2, 1, 3, stride_in=pitch, key=KEY, out=engine.DevMatrix(ctx, out.t[:, 2:], 9, n, out.stride)))
    # contexts that are not GF(2^n <= 8)
    for other in (engine.FieldContext(2**61 - 1, device=0), engine.FieldContext((1 << 16) | 0x2b, True, device=0)):
        x = other.empty_matrix(3, n)
        x.t.fill_(1)
        o = other.empty_matrix(9, n)
        o.t.fill_(7)
        with pytest.raises(NotImplementedError):
            other.keccak_local([x.row(0)], [1], 2, out=o)
        with pytest.raises(NotImplementedError):
            other.keccak_round([x.row(0)], [1], 2, 1, 3, key=KEY, out=o)
        assert bool((o.t == 7).all())
    with pytest.raises(ValueError):
        ctx.keccak_local(rows[:1], [1], 3, out=out)                                                   # rows are two states
    untouched()


@pytest.mark.parametrize('m,t,e', [(3, 1, 2), (5, 2, 3), (7, 3, 3)])
def test_keccak_round_deals_shares_of_the_local_output(mods, m, t, e):
    """for each sender, every (t+1)-subset of the m rows it dealt recombines to keccak_local's output of the same input; a
    second nonce gives other shares of the same values; the input is a pending block with an iota in front"""
    engine = mods[0]
    modulus = kc.IRREDUCIBLE[e]
    ctx = engine.FieldContext(modulus, True, device=0)
    T, rng = kc.mul_table(modulus), np.random.default_rng(10 * m + t)
    k, nstates = 2 * t + 1, 5
    n = B * nstates
    lam = kc.lagrange_at_zero(modulus, range(1, k + 1))
    data = rng.integers(0, 1 << e, size=(k * k, n), dtype=np.uint8)          # [sender][sub-share row]
    buf, rows, pitch = rows_on_device(engine, ctx, data)
    local = ctx.keccak_local(rows[:k], lam, nstates, iota_round=5, nbatch=k, stride_in=k * pitch).to_numpy()
    for y in range(k):
        want = kc.keccak_map(T, recombined(T, data[y * k:(y + 1) * k], lam).reshape(nstates, B), 5, True).reshape(n)
        assert (local[y] == want).all()
    gbuf, out = guarded_matrix(engine, ctx, m * k, n)
    ctx.keccak_round(rows[:k], lam, nstates, t, m, iota_round=5, stride_in=k * pitch, key=KEY, nonce=1, out=out)
    blk = check_guards(gbuf, m * k, n).copy()
    for y in range(k):
        dealt = blk[[j * k + y for j in range(m)]]                             # what sender y dealt to the parties 1..m
        for sub in itertools.combinations(range(m), t + 1):
            mu = kc.lagrange_at_zero(modulus, [j + 1 for j in sub])
            assert (recombined(T, dealt[list(sub)], mu) == local[y]).all(), (y, sub)
        assert (dealt[0] != local[y]).any()
    blk2 = ctx.keccak_round(rows[:k], lam, nstates, t, m, iota_round=5, stride_in=k * pitch, key=KEY, nonce=2).to_numpy()
    assert (blk2 != blk).any(axis=1).all()                                       # every row is re-drawn
    mu = kc.lagrange_at_zero(modulus, range(1, t + 2))
    for y in range(k):
        assert (recombined(T, blk2[[j * k + y for j in range(t + 1)]], mu) == local[y]).all()
    # the senders draw from streams of their own: equal inputs, different shares
    same = np.tile(data[:k], (k, 1))
    _, rows_s, pitch_s = rows_on_device(engine, ctx, same)
    blk3 = ctx.keccak_round(rows_s[:k], lam, nstates, t, m, stride_in=k * pitch_s, key=KEY, nonce=3).to_numpy()
    assert (blk3[0] != blk3[1]).any()


@pytest.mark.parametrize('e', [2, 3])
def test_keccak_round_coefficients_cover_the_field_and_ignore_the_batch_size(mods, e):
    """t = 1: the coefficient (share + value) / x_j of every position is the same for the three parties and takes every
    field value over 4800 positions; state b receives the same shares whether the launch holds b + 1 states or more"""
    engine = mods[0]
    modulus = kc.IRREDUCIBLE[e]
    ctx = engine.FieldContext(modulus, True, device=0)
    T, rng = kc.mul_table(modulus), np.random.default_rng(e)
    q = 1 << e
    inv = {a: next(b for b in range(1, q) if T[a][b] == 1) for a in range(1, q)}
    big = rng.integers(0, q, size=(1, B * 20), dtype=np.uint8)
    X20 = ctx.matrix_from_numpy(np.repeat(big, 3, axis=0))
    X3 = ctx.matrix_from_numpy(np.repeat(big[:, :B * 3], 3, axis=0))
    out3 = ctx.keccak_round([X3.row(0)], [1], 3, 1, 3, stride_in=X3.stride, key=KEY, nonce=9).to_numpy()
    out20 = ctx.keccak_round([X20.row(0)], [1], 20, 1, 3, stride_in=X20.stride, key=KEY, nonce=9).to_numpy()
    assert (out20[:, :B * 3] == out3).all()
    value = ctx.keccak_local([X3.row(0)], [1], 3, nbatch=3, stride_in=X3.stride).to_numpy()
    for y in range(3):
        coef = out3[0 * 3 + y] ^ value[y]                                       # party 1 sits at x = 1
        assert coef.size >= 4800 and set(np.unique(coef)) == set(range(q))
        assert np.bincount(coef, minlength=q).min() > coef.size // (2 * q)      # 4800 / q expected; a stuck bit halves a count to 0
        for j in (1, 2):
            assert (T[inv[j + 1]][out3[j * 3 + y] ^ value[y]] == coef).all()


@pytest.mark.parametrize('m,t,e', [(3, 1, 2), (7, 3, 3)])
def test_the_24_round_chain_in_one_hip_graph(mods, m, t, e):
    engine, _, _, protocols = mods
    modulus = kc.IRREDUCIBLE[e]
    ctx = engine.FieldContext(modulus, True, device=0)
    F = field_of(mods, modulus)
    rng = np.random.default_rng(m)
    nstates = 5
    bits = rng.integers(0, 2, size=(nstates, B), dtype=np.uint8)
    plain = kc.KeccakCpuContext(0b11)
    want = protocols.keccak_f1600(plain, None, plain.matrix_from_numpy(bits.reshape(1, -1)), nstates, 0).t.numpy()[0, :B * nstates]
    S = ctx.matrix_from_numpy(kc.share_bits(modulus, bits, t, m, rng))
    st = ctx.rng_state(key=KEY)
    cg = engine.CapturedLaunches(lambda: protocols.keccak_f1600(ctx, F, S, nstates, t, rng=st))
    n0 = st.nonce()
    seen = []
    for _ in range(2):
        cg.replay()
        torch.cuda.synchronize()
        rows = cg.result.to_numpy().copy()
        assert (kc.open_shares(modulus, rows, t) == want).all()
        seen.append(rows)
    assert st.nonce() == n0 + 2 * 24                                             # one advance by 24 per replay
    assert (seen[0] != seen[1]).any()                                            # fresh coefficients on every replay


def _digests(mods, m, t, e, name, msgs=None, bits=None, d=256):
    engine, _, _, protocols = mods
    modulus = kc.IRREDUCIBLE[e]
    ctx = engine.FieldContext(modulus, True, device=0)
    F = field_of(mods, modulus) if t else None
    rng = np.random.default_rng(len(name) + m)
    bits = protocols.message_bits(msgs) if bits is None else bits
    nstates, nbits = bits.shape
    shares = ctx.matrix_from_numpy(kc.share_bits(modulus, bits, t, m, rng)) if nbits else ctx.empty_matrix(m, 0)
    st = ctx.rng_state(key=KEY) if t else None
    if name.startswith('sha3'):
        out = protocols.sha3(ctx, F, shares, nbits, nstates, t, d=d, rng=st)
    else:
        out = protocols.shake(ctx, F, shares, nbits, nstates, t, d, c=256 if name == 'shake_128' else 512, rng=st)
    rows = out.to_numpy()
    opened = kc.open_shares(modulus, rows, t)
    if t:
        last = kc.lagrange_at_zero(modulus, range(m - t, m + 1))
        assert (recombined(kc.mul_table(modulus), rows[m - t - 1:], last) == opened).all()
    return protocols.digest_bytes(opened.reshape(nstates, d))


@pytest.mark.parametrize('m,t,e', [(3, 1, 2), (7, 3, 3), (1, 0, 1)])
def test_sha3_and_shake_on_the_device(mods, m, t, e):
    """five messages per configuration at the padding edges of their function (0, 1, r/8 - 1, r/8, r/8 + 1 bytes), one
    SHAKE128 with d > r, and the bit lengths of the fixture"""
    rng = np.random.default_rng(e)
    cases = [('sha3_256', 0, 256), ('sha3_512', 1, 512), ('shake_128', 167, 256), ('sha3_224', 144, 224), ('sha3_384', 105, 384)]
    for name, nbytes, d in cases:
        msgs = [rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for _ in range(2)]
        got = _digests(mods, m, t, e, name, msgs=msgs, d=d)
        want = [getattr(hashlib, name)(v).digest(d // 8) if name.startswith('shake') else getattr(hashlib, name)(v).digest() for v in msgs]
        assert got == want, (name, nbytes)
    msg = [bytes([i]) * 7 for i in range(9)]                                      # two permutations of nine states
    assert _digests(mods, m, t, e, 'shake_128', msgs=msg, d=1344 + 8) == [hashlib.shake_128(v).digest(169) for v in msg]
    doc = json.load(open(os.path.join(GOLDEN, 'keccak', 'keccak.json')))
    for entry in doc['digests']:
        bits = np.array([int(c) for c in entry['message']], dtype=np.uint8).reshape(1, -1)
        for name, key in (('sha3_256', 'sha3_256'), ('shake_128', 'shake128_256')):
            got = _digests(mods, m, t, e, name, bits=bits)
            want = np.packbits(np.array([int(c) for c in entry[key]], dtype=np.uint8), bitorder='little').tobytes()
            assert got == [want], (name, entry['nbits'])
