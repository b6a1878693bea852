"""The memory contract of include/ffgpu.h for share generation, the fused gate and Lagrange recombination -- inputs are never
written; nothing outside the n elements of each output row is written, not the padding between n and the row stride either;
with w = 1 a recombination may write over one of its rows -- for ffgpu_split, ffgpu_mul_split, ffgpu_rng_coeffs,
ffgpu_split_rng, ffgpu_mul_split_rng, ffgpu_split_rng_state (with and without mul_by), ffgpu_gate_rng, ffgpu_gate_rng_batch and
ffgpu_recombine on every field policy: at every size at which a path changes, with tight rows, whole-pack rows, rows of a
whole pack plus one element (an aligned base with a stride that is not a whole pack: Launchers::stride_ok false), the pitch of
engine.empty_matrix and bases one element in, with guards around every operand and the padding of every row checked; with the
hand-off switched off, in chains, on a capped grid, in the grouped generator loop and on the GF(2^n) table route.  The case
logic, the references and the layout are tests/share_contract.py; tests/test_share_contract_host.py shows that driver fails
when it should.  Expected values never come from the library; every comparison is byte for byte over the whole tensor."""
import contextlib

import pytest

import ew_contract as ew
import share_contract as sc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

FIELDS = ew.contract_fields()
IDS = [('gf2:' if b else '') + hex(m) for m, b in FIELDS]

# plan_rng (mpyc_amd/csrc/launch.hpp) leaves the spread loop of the in-kernel generator at this many packs: the grouped-loop
# cases below sit one pack and one element above it
SPREAD_MAX_PACKS = 262144
# ffgpu_recombine (mpyc_amd/csrc/api.hip) takes the table kernel of sparse GF(2^n) moduli from this many elements on, k <= 9
GF2W_TABLE_MIN_N = 65536

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


def driver(coracle, ctx, modulus, binary, salt=0):
    ref = sc.ShareRef(coracle, modulus, binary)
    assert ref.q == ctx.order
    return sc.Driver(sc.GpuAdapter(ctx), ref, seed=modulus % 1009 + 100 + salt)


@contextlib.contextmanager
def oracle_threads(coracle):
    """the C oracle on all its threads for the large arrays (one thread is faster on the small ones)"""
    coracle.set_threads(min(16, coracle.max_threads()))
    try:
        yield
    finally:
        coracle.set_threads(1)


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def fields_where(pred):
    from oracle.coracle import elem_bytes
    sel = [(m, b) for m, b in FIELDS if pred(m, b, elem_bytes(m, b))]
    return {'argvalues': sel, 'ids': [('gf2:' if b else '') + hex(m) for m, b in sel]}


def check_matrix(drv, cases):
    """the counts of the lists of share_contract.py; every tier ran: the reduced classes at every small and large size, every
    class of this element width at the five sizes of the full lists"""
    assert drv.cases == cases and drv.steps >= cases
    sizes = {(k[2], k[3]) for k in drv.seen}
    assert all((n, 'tight') in sizes for n in ew.SMALL_SIZES + ew.LARGE_SIZES)
    return sizes


# ---- the matrix, one test per group of entry points ------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_split_with_given_coefficients(coracle, modulus, binary):
    """ffgpu_split, ffgpu_mul_split, ffgpu_rng_coeffs; the status codes; the restated pitch against the engine's"""
    ctx = default_ctx(modulus, binary)
    drv = driver(coracle, ctx, modulus, binary)
    names = drv.SPLIT_HOST + ('rng_coeffs',)
    drv.run_split_matrix(names)
    sizes = check_matrix(drv, sc.count_split(drv.eb, drv.q, names))
    assert all((n, c) in sizes for n in sc.FULL_SIZES for c in sc.stride_classes(drv.eb))
    assert all((n, c) in sizes for n in ew.SMALL_SIZES for c in ('tight', 'pack+1'))
    assert all((n, 'pitched') in sizes for n in ew.LARGE_SIZES)
    assert {k[0] for k in drv.seen} == set(names) and ('split', 't=5 m=11', 1025, 'pack+1') in drv.seen
    assert all((nm, 't=1 m=3', n, 'coef+1') in drv.seen for nm in drv.SPLIT_HOST for n in sc.FULL_SIZES)
    steps = drv.steps
    assert drv.run_status() == 22 and drv.steps == steps + 22
    for n in ew.SMALL_SIZES + ew.LARGE_SIZES + (16384 // drv.eb * 3,):
        assert ctx.empty_matrix(2, n).stride == sc.pitched(drv.eb, n)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_split_with_the_device_generator(coracle, modulus, binary):
    """ffgpu_split_rng, ffgpu_mul_split_rng, ffgpu_split_rng_state with and without mul_by (two calls in a row on a state with a
    known key and nonce, against the nonces `nonce` and `nonce + 1`)"""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 1)
    drv.run_split_matrix(drv.SPLIT_RNG)
    cases = sc.count_split(drv.eb, drv.q, drv.SPLIT_RNG)
    check_matrix(drv, cases)
    assert drv.steps == cases + cases // 2                      # half the cases are on a state: two calls each
    assert {k[0] for k in drv.seen} == set(drv.SPLIT_RNG)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_recombine(coracle, modulus, binary):
    """row pointers in scattered order; 'mixed': every pointer with an alignment of its own; w = 1 with out = one of the rows"""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 2)
    drv.run_recombine_matrix()
    sizes = check_matrix(drv, sc.count_recombine(drv.eb))
    assert drv.eb == 16 or all((n, 'mixed') in sizes for n in sc.FULL_SIZES)
    for k, w in sc.KW:
        assert all(('recombine', 'k=%d w=%d' % (k, w), n, 'pack+1') in drv.seen for n in sc.FULL_SIZES)
    assert all(('recombine', 'k=%d w=1 out=row' % k, 1025, 'tight') in drv.seen for k in sc.KW_ALIAS)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_gate(coracle, modulus, binary):
    """ffgpu_gate_rng itself: kb = 0, the plain loads, the nonce it forwards with a host key and, with a device-resident state,
    the offset 0 it forwards instead of the caller's nonce"""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 3)
    drv.run_gate_matrix()
    check_matrix(drv, sc.count_gate(drv.eb))
    assert len({k[1] for k in drv.seen if 'state' not in k[1]}) == 45 and {k[0] for k in drv.seen} == {'gate_rng'}
    on_state = [k for k in drv.seen if 'state' in k[1]]
    assert drv.steps == drv.cases + len(on_state) and len(on_state) == (15 + 4) * 2 + 5 * len(sc.stride_classes(drv.eb))


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_batched_gate(coracle, modulus, binary):
    """three gates in one launch, gate y's rows between gate y - 1's, each batch stride a whole-pack value or that plus one;
    row y draws with nonce + (y << 40)"""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 4)
    drv.run_batch_matrix()
    assert drv.cases == sc.count_batch(drv.eb)
    assert len({k[1] for k in drv.seen if 'nbatch=3' in k[1]}) == 16


# ---- launch switches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_without_handoff(coracle, monkeypatch, modulus, binary):
    """the reduced matrix with every store non-temporal (FFGPU_HANDOFF=0)"""
    drv = driver(coracle, env_ctx(monkeypatch, modulus, binary, 'FFGPU_HANDOFF', '0'), modulus, binary, 5)
    drv.run_reduced()
    assert drv.cases == len(drv.seen) == sc.count_reduced(drv.eb, drv.q)
    assert len({k[0] for k in drv.seen}) == 10


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_chained_calls(coracle, modulus, binary):
    """mul_split writes a block, recombine reads its rows, split reads the result, on one stream without a host round trip in
    between: the hand-off tracker sees strided output ranges consumed by the next launch"""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 6)
    for n in ew.SMALL_SIZES + ew.LARGE_SIZES:
        for cls in ('pack+1', 'tight'):
            for t, m in sc.TM_REDUCED:
                drv.run_chain(t, m, n, cls)
    assert drv.cases == len(drv.seen) == 19 * 2 * 2 and drv.steps == 3 * drv.cases


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_capped_grid(coracle, monkeypatch, modulus, binary):
    """FFGPU_BLOCKS_PER_CU=1: G = CUs x 256 threads take more than three packs each, so the vector loops iterate and the
    tails start past them; n = 3 G EPV + EPV + 1 (24-byte elements, which move in waves of 64: 3 G + 65)"""
    ctx = env_ctx(monkeypatch, modulus, binary, 'FFGPU_BLOCKS_PER_CU', '1')
    drv = driver(coracle, ctx, modulus, binary, 7)
    G, epv = num_cu() * 256, sc.epv_of(drv.eb)
    n = 3 * G + 65 if drv.eb == 24 else 3 * G * epv + epv + 1
    rows = [drv.draw(n) for _ in range(3)]                 # drawn once, shared by the cases and, with them, the references
    lam = drv.scalars(6)
    with oracle_threads(coracle):
        for cls in ('pack+1', 'pitched'):
            drv.run_split('split', 1, 3, n, cls, data={'a': rows[:1], 'coef': rows[1:2]})
            drv.run_split('split_rng', 1, 3, n, cls, data={'a': rows[:1]})
            drv.run_recombine(3, 2, n, cls, lam=lam, data={'row%d' % j: rows[j:j + 1] for j in range(3)})
    assert drv.cases == len(drv.seen) == 6


# ---- routes chosen by size -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=IDS)
def test_grouped_generator_loop(coracle, monkeypatch, modulus, binary):
    """SPREAD_MAX_PACKS packs and more leave the spread loop of k_split for the grouped one (Launchers::plan_rng): split_rng
    (t = 1, m = 3) and gate_rng (ka = 3, kb = 0) at one pack and one element above it, rows a whole pack plus one apart.  Every
    element width is kept: the Python-integer reference of the two 24-byte fields takes one to two seconds of the test."""
    drv = driver(coracle, default_ctx(modulus, binary), modulus, binary, 8)
    epv = sc.epv_of(drv.eb)
    n = SPREAD_MAX_PACKS * epv + epv + 1
    with oracle_threads(coracle):
        drv.run_split('split_rng', 1, 3, n, 'pack+1')
        drv.run_gate('3', '0', 1, n, 'pack+1')
        # and with the grid capped, so that the grouped loop iterates (the same coefficients: one reference for both)
        capped = sc.Driver(sc.GpuAdapter(env_ctx(monkeypatch, modulus, binary, 'FFGPU_BLOCKS_PER_CU', '1')), drv.ref, seed=3)
        capped.run_split('split_rng', 1, 3, n, 'tight')
    assert drv.cases == 2 and capped.cases == 1


@pytest.mark.parametrize('modulus,binary', **fields_where(lambda m, b, eb: b and eb >= 8 and bin(m).count('1') <= 5))
def test_gf2n_table_recombination(coracle, modulus, binary):
    """GF(2^64) and GF(2^128) with sparse moduli, n >= GF2W_TABLE_MIN_N and k <= 9: nibble tables in LDS.  The Lagrange vector of
    parties 1..5 at 0 (two dense values twice each and a 1) and a row with a zero, a one and a repeated value; w = 2 rows a
    whole pack plus one apart, and w = 1 over one of the rows"""
    ctx = default_ctx(modulus, binary)
    drv = driver(coracle, ctx, modulus, binary, 9)
    n = GF2W_TABLE_MIN_N + 17
    lagrange = po.recombination_vector(po.Field(modulus, True), [1, 2, 3, 4, 5], 0)
    assert sorted(lagrange.count(v) for v in set(lagrange)) == [1, 2, 2] and 1 in lagrange
    v = drv.scalar()
    with oracle_threads(coracle):
        drv.run_recombine(5, 2, n, 'pack+1', lam=lagrange + [v, 0, 1, drv.scalar(), v])
        drv.run_recombine(5, 1, n, 'tight', alias=True, lam=lagrange)
        drv.run_recombine(3, 1, n, 'tight', alias=True, lam=[1, 1, 1])
    assert drv.cases == 3
