"""The cache policy of a launch (mpyc_amd/csrc/handoff.hpp) moves no byte: fused share generation -> recombination -> share
generation of the result -> recombination on one stream, so that the tracker gives both of each of its answers (the first
launch reads cold operands, the others what the launch before them wrote; the first recombination streams its output, the
launches after it keep theirs: share generation write-through, recombination with the default policy), with the hand-off
on and off, over 2^61 - 1 (two elements per 16-byte pack) and 2^128 - 173 (one):
  * n in {1, 2, 511, 512, 513, 1537}: less than a pack, one pack, a workgroup of packs less one element / exactly / plus
    one (2^61 - 1: 512 elements = 256 packs = one workgroup), and 1537 = 2 * 256 * 3 + 1: three workgroups and a ragged
    tail over 2^61 - 1, seven workgroups (an odd count, the last one with one pack) over 2^128 - 173;
  * rows on 16-byte boundaries; every operand and output one element into its buffer with rows an odd number of
    elements apart (over 2^61 - 1 no row is 16-byte aligned then: the element-by-element path; a 16-byte element stays a
    pack); both recombinations writing over the first of their own rows.
Every result is compared with Python-integer arithmetic, byte for byte over the WHOLE buffer it lives in: 32 guard
elements on either side, the offset element and the padding between n and the row pitch keep their fill pattern, and the
inputs are unchanged at the end.  No host round trip between the four launches (device-side snapshots)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

FIELDS = (2**61 - 1, 2**128 - 173)
SIZES = sorted({1, 2, 511, 512, 513, 1537, 2 * 256 * 3 + 1})
LAYOUTS = ('aligned', 'offset', 'inplace')
GUARD = 32
FILL = 0x5A5A5A5A5A5A5A5A
T, M = 1, 3

_ctxs = {}


def ctx_of(monkeypatch, modulus, handoff):
    """the switch is read when a context is created"""
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from mpyc_amd import engine
    if (modulus, handoff) not in _ctxs:
        monkeypatch.setenv('FFGPU_HANDOFF', '1' if handoff else '0')
        _ctxs[modulus, handoff] = engine.FieldContext(modulus, device=0)
        monkeypatch.delenv('FFGPU_HANDOFF')
    return _ctxs[modulus, handoff]


class Buf:
    """rows x n elements, `pitch` elements apart, `off` elements into a buffer with GUARD elements on either side"""

    def __init__(self, ctx, rows, n, pitch, off):
        from mpyc_amd.engine import DevMatrix
        self.ctx, self.rows, self.n, self.pitch = ctx, rows, n, pitch
        self.limbs = ctx.elem_bytes // 8
        self.lo = GUARD + off
        total = self.lo + rows * pitch + GUARD
        tail = (self.limbs,) if self.limbs > 1 else ()
        self.flat = torch.full((total,) + tail, FILL, dtype=torch.int64, device=ctx.torch_device)
        view = self.flat[self.lo:self.lo + rows * pitch].view((rows, pitch) + tail)
        self.mat = DevMatrix(ctx, view, rows, n, pitch)
        self.want = np.full((total,) + tail, FILL, dtype=np.uint64)

    def row(self, i):
        return self.mat.row(i)

    def expect(self, i, vals):
        from mpyc_amd.engine import ints_to_np
        lo = self.lo + i * self.pitch
        self.want[lo:lo + self.n] = ints_to_np(vals, self.ctx.elem_bytes)

    def upload(self, i, vals):
        self.expect(i, vals)
        lo = self.lo + i * self.pitch
        self.flat[lo:lo + self.n] = torch.from_numpy(self.want[lo:lo + self.n].view(np.int64)).to(self.flat.device)

    def snapshot(self):
        """(the buffer now, what it must hold now)"""
        return self.flat.clone(), self.want.copy()


def run_sequence(ctx, p, n, layout, seed):
    rs = np.random.default_rng(seed)
    eb = ctx.elem_bytes
    epv = 16 // eb

    def draw():
        v = [int.from_bytes(rs.bytes(17), 'little') % p for _ in range(n)]
        v[:3] = [p - 1, 0, 1][:n]
        return v
    off = 1 if layout == 'offset' else 0
    pitch = (n + epv - 1) // epv * epv + 2 * epv + off            # whole packs; 'offset': an odd number of elements
    assert (pitch * eb) % 16 == (0 if not off or eb == 16 else 8)
    a, b, c = draw(), draw(), draw()
    A, B, C = (Buf(ctx, 1, n, pitch, off) for _ in range(3))
    for buf, v in ((A, a), (B, b), (C, c)):
        buf.upload(0, v)
    S1, S2 = Buf(ctx, M, n, pitch, off), Buf(ctx, M, n, pitch, off)
    Y1, Y2 = Buf(ctx, 1, n, pitch, off), Buf(ctx, 1, n, pitch, off)
    from oracle import pyoracle as po
    lam = po.recombination_vector(po.Field(p, False), [1, 2, 3], 0)
    prod = [x * y % p for x, y in zip(a, b)]
    shares = [[(s + (j + 1) * r) % p for s, r in zip(prod, c)] for j in range(M)]
    snaps = []
    # 1: a * b -> shares (cold operands; streamed by a context's first sequence, kept by the later ones)
    ctx.split(A.row(0), C.mat, T, M, out=S1.mat, mul_by=B.row(0))
    for j in range(M):
        S1.expect(j, shares[j])
    snaps.append(('split 1', S1.snapshot()))
    # 2: shares -> y1 (reads what launch 1 wrote)
    out1 = S1 if layout == 'inplace' else Y1
    ctx.recombine([S1.row(j) for j in range(M)], lam, out=out1.row(0))
    out1.expect(0, prod)
    snaps.append(('recombine 1', out1.snapshot()))
    # 3: y1 -> shares (reads what launch 2 wrote; share generation has fed its successor before: it keeps its outputs)
    ctx.split(out1.row(0), C.mat, T, M, out=S2.mat)
    for j in range(M):
        S2.expect(j, shares[j])
    snaps.append(('split 2', S2.snapshot()))
    # 4: shares -> y2 (fed again; recombination has fed its successor before, too)
    out2 = S2 if layout == 'inplace' else Y2
    ctx.recombine([S2.row(j) for j in range(M)], lam, out=out2.row(0))
    out2.expect(0, prod)
    snaps.append(('recombine 2', out2.snapshot()))
    for name, buf in (('a', A), ('b', B), ('coef', C), ('y1 at the end', out1)):
        snaps.append((name, buf.snapshot()))
    for name, (got, want) in snaps:
        got = got.cpu().numpy().view(np.uint64)
        assert got.shape == want.shape
        bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
        assert bad.size == 0, '%s: n=%d %s: %d elements differ, first at buffer element %d (rows start at %d)' % (
            name, n, layout, bad.size, bad[0], GUARD + off)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('handoff', (True, False), ids=('handoff', 'streamed'))
@pytest.mark.parametrize('modulus', FIELDS, ids=('p61', 'p128'))
def test_policy_moves_no_byte(monkeypatch, modulus, handoff, layout):
    ctx = ctx_of(monkeypatch, modulus, handoff)
    assert SIZES == [1, 2, 511, 512, 513, 1537]
    for n in SIZES:
        run_sequence(ctx, modulus, n, layout, seed=n + LAYOUTS.index(layout))
