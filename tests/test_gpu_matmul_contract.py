"""ffgpu_matmul on every route of its dispatcher, byte for byte against oracle/fforacle.c (Python integers for 24-byte fields),
through the C ABI on views between guards.

tests/matmul_contract.py restates Launchers::matmul as plan() and derives the shapes from its constants and from the CU
count of the device: every case names the kernel and the flags it means to reach, and the driver asserts them against the
plan before it makes the call.  One parametrised test per route family on every field of ew.contract_fields() plus the
Montgomery 24-byte prime; the flush cases -- a thread accumulates more than FLUSH terms, on periodic data and on all q - 1 --
on one modulus per accumulator type.  The case counts are asserted, and the closing test holds the routes and edges that
passed against the full list, so a dispatcher change that starves a route fails here.

tests/test_matmul_contract_host.py shows that the driver fails when it should.  Expected values never come from the library."""
import time

import pytest

import ew_contract as ew
import matmul_contract as mc
from test_gpu_second_tier_contract import FLUSH_FIELDS, MONT192, default_ctx, ids_of

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

FIELDS = ew.contract_fields() + [MONT192]
NAMES = list(mc.FAMILIES) + list(mc.FLUSH_FAMILIES)
# cases per family, in the order of NAMES, by (element bytes, binary, digit accumulators)
COUNTS = {
    (4, 0, 0): (17, 12, 21, 0, 0, 0, 0, 0, 25, 5, 14, 7, 6, 2, 4, 0, 0, 0, 12, 2),
    (8, 0, 0): (17, 7, 7, 43, 42, 42, 17, 12, 0, 6, 22, 7, 6, 2, 4, 4, 4, 4, 0, 2),
    (12, 0, 1): (17, 14, 17, 0, 0, 0, 0, 0, 24, 6, 9, 4, 6, 2, 2, 0, 0, 0, 12, 2),
    (16, 0, 1): (17, 14, 17, 0, 0, 0, 0, 0, 24, 6, 9, 4, 6, 2, 2, 0, 0, 0, 12, 2),
    (16, 0, 0): (17, 11, 17, 0, 0, 0, 0, 0, 24, 6, 9, 4, 6, 2, 2, 0, 0, 0, 12, 2),
    (24, 0, 1): (13, 15, 13, 0, 0, 0, 0, 0, 24, 6, 0, 6, 6, 2, 4, 0, 0, 0, 12, 2),
    (24, 0, 0): (13, 12, 13, 0, 0, 0, 0, 0, 24, 6, 0, 6, 6, 2, 4, 0, 0, 0, 12, 2),
    (1, 1, 0): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 6, 0, 0, 0, 0, 0, 0, 0),
    (4, 1, 0): (17, 12, 21, 0, 0, 0, 0, 0, 25, 5, 0, 9, 6, 2, 4, 0, 0, 0, 12, 2),
    (8, 1, 0): (17, 12, 21, 0, 0, 0, 0, 0, 25, 5, 0, 9, 6, 2, 4, 0, 0, 0, 12, 2),
    (16, 1, 0): (17, 11, 17, 0, 0, 0, 0, 0, 24, 6, 0, 6, 6, 2, 2, 0, 0, 0, 12, 2),
}
SEEN = set()                    # routes and edges of every case that passed in this run


@pytest.fixture(scope='module')
def co(coracle):
    return coracle


def driver(co, modulus, binary):
    ctx = default_ctx(modulus, binary)
    return mc.Driver(mc.GpuAdapter(ctx), co, modulus, binary)


def run_family(co, name, modulus, binary):
    drv = driver(co, modulus, binary)
    t = drv.t
    t0 = time.time()
    n = drv.run_family(name)
    torch.cuda.synchronize()
    assert drv.cases == n == COUNTS[t.eb, int(t.binary), int(t.lazy)][NAMES.index(name)], (name, hex(modulus), n)
    SEEN.update(drv.seen)
    print('%s: %d cases, %.2f s, largest tensor: %d bytes, %d CUs' % (name, n, time.time() - t0, drv.max_bytes, drv.env.num_cu))
    return drv


def test_environment_restated(co):
    """the matrix-core threshold is the one tests/conftest.py sets, the CU count the device's own, and the fields fall into the
    policy classes the plan assumes"""
    drv = driver(co, 2**61 - 1, False)
    assert drv.env.mfma_min == 1.6e7 and drv.env.mfma_on == 1 and drv.env.num_cu >= 1
    for m, b in FIELDS:
        t = mc.traits(m, b)
        if not b and t.eb >= 12:                    # digit accumulators: the multi-limb 2^k - c primes
            assert (default_ctx(m, b).reduction == 'pseudo-mersenne') == t.lazy, hex(m)
    assert sorted({mc.traits(m, b).eb for m, b in FIELDS}) == [1, 4, 8, 12, 16, 24]


# ---- matrix x few columns ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_short_rows(co, modulus, binary):
    run_family(co, 'short_rows', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_rows_r(co, modulus, binary):
    run_family(co, 'rows_r', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_rows(co, modulus, binary):
    run_family(co, 'rows', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_sub_col16(co, modulus, binary):
    """k_matvec_sub_col<F, NN, 16>: from (M + 15) / 16 >= 2 x CUs on, M = 8177 at 256 CUs"""
    run_family(co, 'sub_col16', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_sub_col64(co, modulus, binary):
    run_family(co, 'sub_col64', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_rows_col(co, modulus, binary):
    run_family(co, 'rows_col', modulus, binary)


# ---- few rows x matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_vecmat_col(co, modulus, binary):
    run_family(co, 'vecmat_col', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_vecmat_col_tiles_and_flush(co, modulus, binary):
    """the second staged tile of k_vecmat_partial_col with dead lanes behind the barrier, and its flush"""
    run_family(co, 'vecmat_col_tiles', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_vecmat(co, modulus, binary):
    run_family(co, 'vecmat', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_vecmat_final(co, modulus, binary):
    """k_vecmat_final at ks = 7, 8, 9, 39, 40, 41.  ks = 1 is not reachable through the ABI on any field, ks = 7 not on
    fields whose threads take a pack of two or four columns (matmul_contract.vecmat_final_shape says why)"""
    drv = run_family(co, 'vecmat_final', modulus, binary)
    if drv.t.epw == 1:
        assert mc.final_ks_unreachable(drv.t, drv.env) == ((1,) if drv.t.col_mac or drv.t.pack == 1 else (1, 7))


# ---- dense products ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_matrix_cores(co, modulus, binary):
    run_family(co, 'mfma', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_valu_tiles(co, modulus, binary):
    run_family(co, 'valu', modulus, binary)


@pytest.mark.parametrize('modulus,binary', FIELDS, ids=ids_of(FIELDS))
def test_degenerate_and_refused(co, modulus, binary):
    drv = run_family(co, 'degenerate', modulus, binary)
    assert drv.run_refused() == 6 and drv.cases == 12
    SEEN.update(drv.seen)


# ---- the flush edges, one modulus per accumulator type -----------------------------------------------------------------------
@pytest.mark.parametrize('modulus,binary', FLUSH_FIELDS, ids=ids_of(FLUSH_FIELDS))
@pytest.mark.parametrize('name', list(mc.FLUSH_FAMILIES))
def test_flush(co, name, modulus, binary):
    """a thread accumulates FLUSH terms, flushes, and accumulates again; all q - 1 is the most the accumulator holds"""
    run_family(co, name, modulus, binary)


def test_every_route_and_edge_was_reached():
    """after the tests above (it needs them to have run): nothing of the list is missing"""
    assert not sorted(mc.REQUIRED - SEEN)
