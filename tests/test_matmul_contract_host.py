"""The driver of the ffgpu_matmul contract tests (tests/matmul_contract.py) without a GPU: plan() gives every generated case
the route and the edge it claims -- and the existing shapes of test_skinny_products the routes that show why they were not
enough --, the driver passes on the Python-integer context of tests/cpuctx.py, and it fails, with the right kind of violation,
on adapters that are wrong the way a kernel could be.  A driver that cannot see these would not see the kernel bugs it
exists for."""
import pytest

torch = pytest.importorskip('torch')

import ew_contract as ew
import matmul_contract as mc
from cpuctx import CpuFieldContext
from ew_contract import ContractViolation

P31, P61, RC64, P96, P128, M128, P136, M192 = (2**31 - 1, False), (2**61 - 1, False), (6616326157076047771, False), (2**96 - 17, False), \
    (2**128 - 173, False), (2**127 + 2**100 + 0x101, False), (2**136 - 113, False), (2**135 + 4823, False)
GF256, GF32, GF64, GF128 = (0x11b, True), (0x10000008d, True), (0x1000000000000001b, True), (0x100000000000000000000000000000087, True)
ALL_FIELDS = ew.contract_fields() + [M192]
HOST_FIELDS = [P31, P61, P96, P136, GF256, GF64]
IDS = lambda fields: [('gf2:' if b else '') + hex(m) for m, b in fields]
ENV256 = mc.env_of(256, 1.6e7, 1)
HOST_ENV = mc.env_of(8, 5e5, 1)                      # thinned: 8 CUs, matrix cores from 5e5 multiply-adds on
HOST_MACS = 150000                                  # Python integers: cases up to this many multiply-adds
FAMILY_NAMES = list(mc.FAMILIES) + list(mc.FLUSH_FAMILIES)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def test_traits_follow_the_policy_classes():
    """policy_build.hpp: RC32 | PM64 / RC64 (column sums) | PM96, PM128, PM192 (digit accumulators, flush 32) | MONT128, MONT192"""
    cls = lambda f: (mc.traits(*f).eb, mc.traits(*f).col_mac, mc.traits(*f).lazy, mc.traits(*f).flush, mc.traits(*f).pack, mc.traits(*f).mfma)
    assert cls(P31) == (4, False, False, 192, 4, 4)
    assert cls(P61) == cls(RC64) == (8, True, False, 192, 2, 8)
    assert cls(P96) == (12, False, True, 32, 1, 12)
    assert cls(P128) == (16, False, True, 32, 1, 16) and cls(M128) == (16, False, False, 192, 1, 16)
    assert cls(P136) == (24, False, True, 32, 1, 0) and cls(M192) == (24, False, False, 192, 1, 0)
    assert cls(GF256) == (1, False, False, 192, 4, 0) and cls(GF64) == (8, False, False, 192, 2, 0)
    assert [mc.traits(*f).one_in_unaligned for f in (GF256, P31, P61, P96, P128, P136)] == [True, True, True, False, False, True]
    assert [mc.traits(*f).ld_unit for f in (GF256, P31, P61, P96, P128, P136)] == [16, 4, 2, 1, 1, 2]


@pytest.mark.parametrize('num_cu', [256, 304, 64])
def test_every_generated_case_takes_the_route_and_the_edge_it_claims(num_cu):
    env = mc.env_of(num_cu, 1.6e7, 1)
    seen = {'refused/' + s for s in ('M=0', 'N=0', 'lda<K', 'ldb<N', 'ldc<N', 'C=NULL')}
    for modulus, binary in ALL_FIELDS:
        t = mc.traits(modulus, binary)
        for name in FAMILY_NAMES:
            for case in mc.family(name, modulus, binary, env):
                p = case.check_plan(t, env)
                assert p.route in mc.ROUTES
                seen.add(p.route)
                seen.update(case.edges)
    # (ks = 1 needs a target of at most one workgroup per column block: column-sum fields on a device of at most 128 CUs)
    assert not sorted(mc.REQUIRED - seen) and seen - mc.REQUIRED <= {'vecmat_final/ks=1'}


def test_the_edges_sit_where_the_dispatcher_turns():
    """some of the derived numbers, spelled out at 256 CUs"""
    t, env = mc.traits(*P61), ENV256
    assert mc.sub_col16_min_m(env) == 8177
    assert [c.M for c in mc.family('sub_col16', *P61, env)][:3] == [8177 + 17, 8177, 8177 + 1]
    route = lambda M, K, N, **kw: mc.plan(t, M, K, N, kw.pop('lda', K), kw.pop('ldb', N), env=env, **kw)
    assert route(8176, 4096, 4).route == 'sub_col64' and route(16384, 4096, 4).route == 'sub_col16'       # the README's row
    assert route(8177, 4096, 4, ldb=5).route == 'rows_col' and route(8177, 63, 4).route == 'rows_col'
    assert route(8177, 4096, 4, b_aligned=False).route == 'rows_col' and route(8177, 4096, 4, a_aligned=False).vec == 0
    assert route(1024, 32, 8).route == 'short_rows' and route(1023, 32, 8).route == 'rows' and route(1024, 33, 8).route == 'rows_col'
    assert route(2048, 1024, 1).route == 'rows_r' and route(2047, 1024, 1).route == 'rows' and route(2048, 1022, 1).route == 'rows'
    assert route(8, 64, 64).route == 'vecmat_col' and route(8, 63, 64).route == 'valu_2x2' and route(9, 64, 64).route == 'valu_2x2'
    assert route(256, 245, 256).route == 'mfma_glds' and route(256, 244, 256).route == 'valu_2x2'
    p = route(128, 256, 512)
    assert p.braw == 1 and route(129, 256, 512).braw == 0 and route(128, 256, 512, ldb=513).braw == 0
    # the flush sizes: a thread of the 256 takes FLUSH terms and one more pack, thread 0 the odd element
    assert mc.flush_k(t) == 256 * 194 + 1 and mc.flush_k(mc.traits(*P136)) == 256 * 33 + 1
    for f in (P61, P96, M192):
        worst, grant = mc.scratch_halving_unreachable(mc.traits(*f))
        assert worst <= grant, (f, worst)            # the halving loop of mm_skinny_m never runs


SKINNY_SHAPES = [(200, 333, 1), (100, 257, 3), (64, 1000, 8), (77, 5, 2), (1, 500, 300), (3, 1000, 129), (8, 2100, 64), (2, 7, 1000),
                 (64, 300, 200), (40, 1000, 90), (130, 2000, 70), (9, 129, 9), (5000, 7, 1), (3000, 32, 3), (4096, 1024, 1),
                 (4101, 1030, 2), (8192, 2050, 1), (1, 4096, 4096), (2, 300, 4098), (5, 1111, 640), (8, 4500, 300), (7, 129, 70)]
SKINNY_FLUSH_SHAPES = [(3, 97, 70), (8, 1000, 129), (6, 33, 300)] + [(M, K if K != 1000 else K + M, N) for M in range(1, 9) for K, N in ((1000, 130), (389, 261))]
SKINNY_COL_SHAPES = [(M, K if K != 1000 else K + N, N) for N in range(2, 9) for M, K in ((71, 1000), (130, 389), (64, 60001))]


def test_why_the_shapes_of_test_skinny_products_were_not_enough():
    """tests/test_gpu_parity.py test_skinny_products at 256 CUs: no shape takes k_matvec_sub_col<., ., 16>, no few-rows shape
    runs a chunk of more than 64 rows (so neither the 192-term flush nor the second 128-row tile of k_vecmat_partial_col), the
    'around the flush' shapes of the digit accumulators run chunks of 8 (K = 33 has no scratch and goes to the tiles), and
    k_matvec_rows_col never runs its vector loop"""
    plans = lambda f, shapes: [mc.plan(mc.traits(*f), M, K, N, K, N, env=ENV256) for M, K, N in shapes]
    for f in (P61, RC64, P96, P128, P31, GF64):
        ps = plans(f, SKINNY_SHAPES + SKINNY_FLUSH_SHAPES)
        assert 'sub_col16' not in {p.route for p in ps}
        assert max(p.kchunk for p in ps if p.route.startswith('vecmat')) <= 64
    assert max(p.kchunk for p in plans(P61, SKINNY_FLUSH_SHAPES)) == 8
    assert [(p.route, p.kchunk) for p in plans(P96, SKINNY_FLUSH_SHAPES[:3])] == [('vecmat', 8), ('vecmat', 8), ('valu_2x2', 0)]    # (K = 33: no scratch)
    # matrix x 2..8 columns: an even K goes to sub_col<64>; an odd one is an odd lda, so k_matvec_rows_col runs without its
    # vector loop -- its scalar loop does flush at (64, 60001): 235 terms per thread
    ps = plans(P61, SKINNY_COL_SHAPES)
    assert {(p.route, p.vec) for p in ps} == {('sub_col64', 1), ('rows_col', 0)}
    assert max(p.terms for p in ps if p.route == 'rows_col') == 235 and max(p.terms for p in ps if p.route == 'sub_col64') < 192
    # and the shapes of test_matmul_leading_dimensions: lda = K + 5 is odd, A never goes in packs
    t = mc.traits(*P61)
    assert mc.plan(t, 70, 300, 3, 305, 6, env=ENV256).vec == 0 and mc.plan(t, 130, 1000, 8, 1005, 11, env=ENV256).vec == 0


# ---- the honest context passes -----------------------------------------------------------------------------------------------
def driver(co, modulus, binary, adapter=mc.CpuAdapter, ctx=CpuFieldContext):
    return mc.Driver(adapter(ctx(modulus, binary)), co, modulus, binary, env=HOST_ENV)


def host_cases(modulus, binary):
    out = []
    for name in FAMILY_NAMES:
        out += [c for c in mc.family(name, modulus, binary, HOST_ENV) if c.macs() <= (HOST_MACS // 8 if binary else HOST_MACS)]     # (GF(2^n) products are slow in Python)
    return out


HOST_COUNTS = {P31: 30, P61: 98, P96: 36, P136: 45, GF256: 13, GF64: 17}        # the 6 refused calls included


@pytest.mark.parametrize('modulus,binary', HOST_FIELDS, ids=IDS(HOST_FIELDS))
def test_driver_passes_on_the_integer_context(coracle, modulus, binary):
    drv = driver(coracle, modulus, binary)
    cases = host_cases(modulus, binary)
    drv.run_all(cases)
    assert drv.run_refused() == 6
    assert drv.cases == len(cases) + 6 == HOST_COUNTS[modulus, binary], drv.cases
    routes = drv.seen & set(mc.ROUTES)
    assert routes >= ({'valu_bytes'} if drv.t.epw > 1 else {'short_rows', 'valu_2x2', 'vecmat_col' if drv.t.col_mac else 'vecmat'}), routes
    print('largest tensor: %d bytes' % drv.max_bytes)


# ---- wrong adapters ----------------------------------------------------------------------------------------------------------
class DropsTheLastRowOfAnOddM(mc.CpuAdapter):
    """(1) two rows per workgroup, the last workgroup of an odd M forgotten"""

    def matmul(self, buf, a, lda, b, ldb, c, ldc, M, K, N):
        return super().matmul(buf, a, lda, b, ldb, c, ldc, M - M % 2 if M > 1 else M, K, N)


class IgnoresLda(mc.CpuAdapter):
    """(2) rows of A taken K apart"""

    def product(self, buf, a, lda, b, ldb, M, K, N):
        return super().product(buf, a, K, b, ldb, M, K, N)


class IgnoresLdb(mc.CpuAdapter):
    """(3) rows of B taken N apart"""

    def product(self, buf, a, lda, b, ldb, M, K, N):
        return super().product(buf, a, lda, b, N, M, K, N)


class ForgetsTheLastTermOfAnOddK(mc.CpuAdapter):
    """(4) pairs of terms without the odd one behind them"""

    def product(self, buf, a, lda, b, ldb, M, K, N):
        if K % 2 == 0 or K == 1:
            return super().product(buf, a, lda, b, ldb, M, K, N)
        A, B = self._gather(buf, a, M, lda, K - 1), self._gather(buf, b, K - 1, ldb, N)
        return self.ctx.matmul(A, B, M, K - 1, N)


class WrapsInsteadOfFlushing(mc.CpuAdapter):
    """(5) an accumulator with room for FLUSH products of (q - 1)^2 that is never flushed: the sum wraps at that bound.  Uniform
    data stays far below it (a product is q^2 / 4 on average), all q - 1 crosses it at FLUSH + 1 terms"""

    def product(self, buf, a, lda, b, ldb, M, K, N):
        q = self.ctx.modulus
        room = mc.traits(q, False).flush * (q - 1) ** 2 + 1
        A, B = self._gather(buf, a, M, lda, K).to_ints(), self._gather(buf, b, K, ldb, N).to_ints()
        vals = [sum(A[i * K + k] * B[k * N + j] for k in range(K)) % room % q for i in range(M) for j in range(N)]
        return self.ctx._put(self.ctx.empty(M * N), vals)


class WritesThePad(mc.CpuAdapter):
    """(6) stores whole rows of ldc elements"""

    def matmul(self, buf, a, lda, b, ldb, c, ldc, M, K, N):
        rc = super().matmul(buf, a, lda, b, ldb, c, ldc, M, K, N)
        if rc == mc.OK and M > 1 and ldc > N:
            buf[c + N * self.eb:c + ldc * self.eb] = 0
        return rc


class WritesOnePastC(mc.CpuAdapter):
    """(7) a row past M is stored"""

    def matmul(self, buf, a, lda, b, ldb, c, ldc, M, K, N):
        rc = super().matmul(buf, a, lda, b, ldb, c, ldc, M, K, N)
        if rc == mc.OK and M and N:
            end = c + ((M - 1) * ldc + N) * self.eb
            buf[end:end + self.eb] = 0
        return rc


class WritesIntoA(mc.CpuAdapter):
    """(8) the converted operand stored in place"""

    def matmul(self, buf, a, lda, b, ldb, c, ldc, M, K, N):
        rc = super().matmul(buf, a, lda, b, ldb, c, ldc, M, K, N)
        if rc == mc.OK and a is not None and K:
            buf[a:a + self.eb] = 0xFF
        return rc


class LeavesCUntouchedForAnEmptyK(mc.CpuAdapter):
    """(9) K == 0 returns before any kernel"""

    def matmul(self, buf, a, lda, b, ldb, c, ldc, M, K, N):
        return mc.OK if K == 0 else super().matmul(buf, a, lda, b, ldb, c, ldc, M, K, N)


class WritesOnARefusedCall(mc.CpuAdapter):
    """(10) the argument check after the first store"""

    def matmul(self, buf, a, lda, b, ldb, c, ldc, M, K, N):
        rc = super().matmul(buf, a, lda, b, ldb, c, ldc, M, K, N)
        if rc == mc.EINVAL and c is not None:
            buf[c:c + self.eb] = 0
        return rc


def small(label, M, K, N, **kw):
    return mc.Case(label, M, K, N, None, **kw)


def part(*cases):
    def run(drv):
        drv.run_all(mc.resolve(drv.t, drv.env, [small(*c[:4], **(c[4] if len(c) > 4 else {})) for c in cases]))
    return run


def flush_part(data):
    def run(drv):
        K = drv.t.flush + 9
        drv.run_all(mc.resolve(drv.t, drv.env, [small('past-flush', 3, K, 5, data=data)]))
    return run


def refused(drv):
    drv.run_refused()


def degenerate(drv):
    drv.run_family('degenerate')


PRIMES = [P61, P96, P136]
# (adapter, the cases meant to catch it, kind of violation, words of its message, fields); kind None: these cases pass
WRONG = [
    (DropsTheLastRowOfAnOddM, part(('even', 66, 9, 3)), None, '', HOST_FIELDS),
    (DropsTheLastRowOfAnOddM, part(('even', 66, 9, 3), ('odd', 67, 9, 3)), 'out', 'C[66, 0]', HOST_FIELDS),
    (IgnoresLda, part(('contiguous', 5, 9, 7)), None, '', HOST_FIELDS),
    (IgnoresLda, part(('lda', 5, 9, 7, dict(lda=10))), 'out', 'C[1, 0]', HOST_FIELDS),
    (IgnoresLdb, part(('ldb', 5, 9, 7, dict(ldb=8))), 'out', 'C[0, 0]', HOST_FIELDS),
    (ForgetsTheLastTermOfAnOddK, part(('even', 5, 10, 7)), None, '', HOST_FIELDS),
    (ForgetsTheLastTermOfAnOddK, part(('odd', 5, 11, 7)), 'out', 'C[0, 0]', HOST_FIELDS),
    (WrapsInsteadOfFlushing, flush_part('per'), None, '', PRIMES),
    (WrapsInsteadOfFlushing, flush_part('max'), 'out', 'past-flush', PRIMES),
    (WritesThePad, part(('pad', 5, 9, 7)), 'pad', 'pad: C[0, 7]', HOST_FIELDS),
    (WritesOnePastC, part(('past', 5, 9, 7)), 'guard', '0 past its end', HOST_FIELDS),
    (WritesIntoA, part(('into-A', 5, 9, 7)), 'input', 'input A', HOST_FIELDS),
    (LeavesCUntouchedForAnEmptyK, degenerate, 'out', 'K=0', [P61, GF256]),
    (WritesOnARefusedCall, refused, 'out', 'refused/l', [P61, GF256]),
]


@pytest.mark.parametrize('adapter,run,kind,words,fields', WRONG, ids=['%s-%s' % (a.__name__, k) for a, _, k, _, _ in WRONG])
def test_driver_fails_on_a_wrong_adapter(coracle, adapter, run, kind, words, fields):
    for modulus, binary in fields:
        drv = driver(coracle, modulus, binary, adapter)
        if kind is None:
            run(drv)
            assert drv.cases
            continue
        with pytest.raises(ContractViolation) as err:
            run(drv)
        assert err.value.kinds == {kind} and words in str(err.value), (adapter.__name__, hex(modulus), str(err.value))
        good = driver(coracle, modulus, binary)               # and the same cases pass on the honest adapter
        run(good)
        assert good.cases > drv.cases
