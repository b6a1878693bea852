"""The two operand conventions every engine wrapper shares, on the device, over one 8-byte and one 24-byte prime policy (the
element-wise wrappers, sqrt_cl among them, also over an 8-byte and a 24-byte prime = 1 mod 4, the only ones sqrt_cl serves):

  out=   a caller's output comes back as THE SAME OBJECT (an empty one too: a DevArray of no elements is falsy, so `out or ...`
         would hand back a fresh allocation), and an output one element short is refused with ValueError before anything is
         launched: the inputs, the in-place operands among them, are unchanged.
  rows   the seven wrappers that recombine sub-share rows (engine.FieldContext._rows) refuse no rows, a lambda count other than
         the row count, a row an element short and a row of another modulus with ValueError; ten rows are more than the
         kernels stage (NotImplementedError).

Shapes are the smallest the entries accept: one element; outer = inner = 1 with k = 2 (k = 1 for the scans); l = 2, n = 1,
round 1 for the carry entries; l = 2 for the norm entries; f = 1 for the truncation."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

FIELDS = {'pm64-mersenne': 2**61 - 1, 'pm192': 2**136 - 113}
ONE_MOD_FOUR = {'pm64-k64-1mod4': 2**64 - 59, 'pm192-1mod4': 2**136 - 243}
OTHER = 2**40 - 87                                   # rows "of another modulus" come from this field


@pytest.fixture(scope='module')
def ctxs():
    assert torch.cuda.is_available()
    from mpyc_amd import engine
    return {name: engine.FieldContext(p, device=0) for name, p in {**FIELDS, **ONE_MOD_FOUR}.items()}, engine.FieldContext(OTHER, device=0)


def ones(ctx, n):
    return ctx.from_ints([1] * n)


# ---- out= ------------------------------------------------------------------------------------------------------------------------
def elementwise(ctx, n):
    """name -> (call(out), inputs) for the element-wise wrappers and recombine (w = 1) on n elements; sqrt_cl where the field
    has it"""
    a, b, c, d, e = (ones(ctx, n) for _ in range(5))
    sqrt = {'sqrt_cl': (lambda out: ctx.sqrt_cl(a, out=out), [a])} if ctx.modulus % 4 == 1 else {}
    return {
        **sqrt,
        'add': (lambda out: ctx.add(a, b, out=out), [a, b]),
        'sub': (lambda out: ctx.sub(a, b, out=out), [a, b]),
        'mul': (lambda out: ctx.mul(a, b, out=out), [a, b]),
        'neg': (lambda out: ctx.neg(a, out=out), [a]),
        'reduce': (lambda out: ctx.reduce(a, out=out), [a]),
        'add_scalar': (lambda out: ctx.add_scalar(a, 5, out=out), [a]),
        'mul_scalar': (lambda out: ctx.mul_scalar(a, 5, out=out), [a]),
        'rsub_scalar': (lambda out: ctx.rsub_scalar(a, 5, out=out), [a]),
        'muladd': (lambda out: ctx.muladd(a, b, c, out=out), [a, b, c]),
        'pow': (lambda out: ctx.pow(a, 3, out=out), [a]),
        'inv': (lambda out: ctx.inv(a, out=out), [a]),
        'beaver_combine': (lambda out: ctx.beaver_combine(a, b, c, d, e, True, out=out), [a, b, c, d, e]),
        'recombine': (lambda out: ctx.recombine([a, b, c], [1, 2, 3], out=out), [a, b, c]),
    }


def structured(ctx):
    """name -> (call(out) returning the array `out` became, inputs, elements of the output) at the smallest shapes"""
    x1, x2, x4 = ones(ctx, 1), ones(ctx, 2), ones(ctx, 4)
    y1, y2 = ones(ctx, 1), ones(ctx, 2)
    R = ctx.carry_rows(2, 1)
    tab = ctx.find_table(2, [0, 1], [1, 2])           # (1, 2, 2): one value per position
    return {
        'matmul': (lambda out: ctx.matmul(x2, y2, 1, 2, 1, out=out), [x2, y2], 1),
        'matmul_stack': (lambda out: ctx.matmul_stack(x2, y2, 1, 1, 2, 1, 2, 2, out=out), [x2, y2], 1),
        'convolve': (lambda out: ctx.convolve(x2, y1, out=out), [x2, y1], 2),
        'scan': (lambda out: ctx.scan(x1, 1, 1, 1, out=out), [x1], 1),
        'scan_with_initial': (lambda out: ctx.scan(x1, 1, 1, 1, with_initial=True, out=out), [x1], 2),
        'axis_reduce': (lambda out: ctx.axis_reduce(x2, 1, 2, 1, out=out), [x2], 1),
        'sgn_mask': (lambda out: ctx.sgn_mask(x1, x2, y1, 2, out=out), [x1, x2, y1], 1),
        'sgn_finish': (lambda out: ctx.sgn_finish(x1, y1, x1, 2, out=out), [x1, y1], 1),
        'cx_diff': (lambda out: ctx.cx_diff(x2, 1, 2, 1, 1, 1, 0, out=out), [x2], 1),
        'bits_mask': (lambda out: ctx.bits_mask(x1, x2, y1, 2, 4, out=out), [x1, x2, y1], 1),
        'carry_prod': (lambda out: ctx.carry_prod(x2, y2, 2, 1, out=out), [x2, y2], R),
        'bits_finish': (lambda out: ctx.bits_finish(x1, x2, y2, 2, out=out), [x1, x2, y2], 2),
        'tour_diff': (lambda out: ctx.tour_diff(x2, 1, 2, 1, ctx.TOUR_HALVES, out=out), [x2], 1),
        'tour_select': (lambda out: ctx.tour_select(x2, [x1, y1], [1, 2], 1, 2, 1, ctx.TOUR_ODD_EVEN, out=out), [x2, x1, y1], 1),
        'tour_unit_prod': (lambda out: ctx.tour_unit_prod(x1, y1, 1, 2, 1, out=out), [x1, y1], 1),
        'tour_unit_expand': (lambda out: ctx.tour_unit_expand(x1, [y1], [1], 1, 2, 1, out=out), [x1, y1], 2),
        'find_leaf_prod': (lambda out: ctx.find_leaf_prod(x2, tab, 1, 2, 1, 2, out=out), [x2, tab], 2),
        'find_leaf_apply': (lambda out: ctx.find_leaf_apply(x2, tab, [y2], [1], 1, 2, 1, 2, out=out), [x2, tab, y2], 2),
        'find_prod': (lambda out: ctx.find_prod(x4, 1, 2, 1, 2, out=out), [x4], 2),
        'trunc_mask_ar': (lambda out: ctx.trunc_mask(x1, y1, x1, 1, 4, ar_out=out)[0], [x1, y1], 1),
        'trunc_mask_masked': (lambda out: ctx.trunc_mask(x1, y1, x1, 1, 4, out=out)[1], [x1, y1], 1),
        'trunc_finish': (lambda out: ctx.trunc_finish([x1, y1], [1, 2], x1, 1, out=out), [x1, y1], 1),
        'norm_prod': (lambda out: ctx.norm_prod(x2, 2, out=out)[0], [x2], 1),
        'norm_prod_sign': (lambda out: ctx.norm_prod(x2, 2, sign_out=out)[1], [x2], 1),
        'norm_apply': (lambda out: ctx.norm_apply(x2, [x1, y1], [1, 2], 2, out=out), [x2, x1, y1], 1),
        'group_matvec': (lambda out: ctx.group_matvec(x2, [[1, 2]], out=out), [x2], 1),
    }


ELEMENTWISE = ['add', 'sub', 'mul', 'neg', 'reduce', 'add_scalar', 'mul_scalar', 'rsub_scalar', 'muladd', 'pow', 'inv', 'beaver_combine',
               'recombine']
ELEMENTWISE_CASES = [(name, fn) for name in FIELDS for fn in ELEMENTWISE] + \
                    [(name, fn) for name in ONE_MOD_FOUR for fn in ELEMENTWISE + ['sqrt_cl']]
STRUCTURED = ['matmul', 'matmul_stack', 'convolve', 'scan', 'scan_with_initial', 'axis_reduce', 'sgn_mask', 'sgn_finish', 'cx_diff',
              'bits_mask', 'carry_prod', 'bits_finish', 'tour_diff', 'tour_select', 'tour_unit_prod', 'tour_unit_expand',
              'find_leaf_prod', 'find_leaf_apply', 'find_prod', 'trunc_mask_ar', 'trunc_mask_masked', 'trunc_finish', 'norm_prod',
              'norm_prod_sign', 'norm_apply', 'group_matvec']


def check_out(ctx, call, inputs, nout):
    out = ctx.empty(nout)
    assert call(out) is out
    torch.cuda.synchronize()
    keep = [x.t.clone() for x in inputs]
    with pytest.raises(ValueError):
        call(ctx.empty(nout - 1))
    torch.cuda.synchronize()
    assert all(torch.equal(x.t, k) for x, k in zip(inputs, keep)), 'a refused call wrote an input'


@pytest.mark.parametrize('name', list(FIELDS))
def test_the_tables_name_every_case(ctxs, name):
    ctx = ctxs[0][name]
    assert sorted(elementwise(ctx, 1)) == sorted(ELEMENTWISE) and sorted(structured(ctx)) == sorted(STRUCTURED)


@pytest.mark.parametrize('name', list(ONE_MOD_FOUR))
def test_the_table_names_sqrt_cl_where_the_field_has_it(ctxs, name):
    assert sorted(elementwise(ctxs[0][name], 1)) == sorted(ELEMENTWISE + ['sqrt_cl'])
    assert sorted(fn for nm, fn in ELEMENTWISE_CASES if nm == name) == sorted(ELEMENTWISE + ['sqrt_cl'])
    assert all(p % 4 == 1 for p in ONE_MOD_FOUR.values()) and all(p % 4 == 3 for p in FIELDS.values())


@pytest.mark.parametrize('name,fn', ELEMENTWISE_CASES, ids=['%s-%s' % c for c in ELEMENTWISE_CASES])
def test_elementwise_out_comes_back_and_a_short_one_is_refused(ctxs, name, fn):
    ctx = ctxs[0][name]
    call, inputs = elementwise(ctx, 1)[fn]
    check_out(ctx, call, inputs, 1)
    # no elements: the caller's empty output is the result, not a fresh allocation
    call, _ = elementwise(ctx, 0)[fn]
    out = ctx.empty(0)
    assert call(out) is out


@pytest.mark.parametrize('fn', STRUCTURED)
@pytest.mark.parametrize('name', list(FIELDS))
def test_structured_out_comes_back_and_a_short_one_is_refused(ctxs, name, fn):
    ctx = ctxs[0][name]
    check_out(ctx, *structured(ctx)[fn])


@pytest.mark.parametrize('name', list(FIELDS))
def test_short_out_is_refused_where_the_entry_needs_more_than_this_file_sets_up(ctxs, name):
    """sqrt_cl on a prime = 3 mod 4, which the entry would refuse (on the primes = 1 mod 4 it is one of the element-wise cases
    above), and the PRSS entries, which need key material: their outputs go through the same check, which comes before the
    entry is reached"""
    ctx = ctxs[0][name]
    a = ones(ctx, 2)
    with pytest.raises(ValueError):
        ctx.sqrt_cl(a, out=ctx.empty(1))
    with pytest.raises(ValueError):
        ctx.prss_combine([bytes(64)], 1, 32, [1], 2, out=ctx.empty(1))
    with pytest.raises(ValueError):
        ctx.prss_chacha([bytes(40)], 1, 32, [1], 2, out=ctx.empty(1))


# ---- rows ------------------------------------------------------------------------------------------------------------------------
def rows_cases(ctx):
    """name -> (call(rows, lambdas), elements of a row, in-place operands)"""
    x1, x2 = ones(ctx, 1), ones(ctx, 2)
    g2, p2 = ones(ctx, 2), ones(ctx, 2)
    tab = ctx.find_table(2, [0, 1], [1, 2])
    return {
        'cx_apply': (lambda rows, lam: ctx.cx_apply(x2, rows, lam, 1, 2, 1, 1, 1, 0), 1, [x2]),
        'carry_apply': (lambda rows, lam: ctx.carry_apply(g2, p2, rows, lam, 2, 1), ctx.carry_rows(2, 1), [g2, p2]),
        'tour_select': (lambda rows, lam: ctx.tour_select(x2, rows, lam, 1, 2, 1, ctx.TOUR_HALVES), 1, [x2]),
        'tour_unit_expand': (lambda rows, lam: ctx.tour_unit_expand(x1, rows, lam, 1, 2, 1), 1, [x1]),
        'find_leaf_apply': (lambda rows, lam: ctx.find_leaf_apply(x2, tab, rows, lam, 1, 2, 1, 2), 2, [x2, tab]),
        'trunc_finish': (lambda rows, lam: ctx.trunc_finish(rows, lam, x1, 1), 1, [x1]),
        'norm_apply': (lambda rows, lam: ctx.norm_apply(x2, rows, lam, 2), 1, [x2]),
    }


ROWS = ['cx_apply', 'carry_apply', 'tour_select', 'tour_unit_expand', 'find_leaf_apply', 'trunc_finish', 'norm_apply']


@pytest.mark.parametrize('fn', ROWS)
@pytest.mark.parametrize('name', list(FIELDS))
def test_rows_are_checked_before_the_launch(ctxs, name, fn):
    by_name, other = ctxs
    ctx = by_name[name]
    cases = rows_cases(ctx)
    assert sorted(cases) == sorted(ROWS)
    call, n, operands = cases[fn]
    row = lambda: ones(ctx, n)
    call([row(), row()], [1, 2])                      # the shapes above are ones the entry accepts
    torch.cuda.synchronize()
    keep = [x.t.clone() for x in operands]
    for rows, lam in (([], []),
                      ([row(), row()], [1]),
                      ([row(), row()], [1, 2, 3]),
                      ([row(), ones(ctx, n - 1)], [1, 2]),
                      ([ones(ctx, n - 1), row()], [1, 2]),
                      ([row(), ones(other, n)], [1, 2])):
        with pytest.raises(ValueError):
            call(rows, lam)
    with pytest.raises(NotImplementedError):
        call([row()] * 10, [1] * 10)
    torch.cuda.synchronize()
    assert all(torch.equal(x.t, k) for x, k in zip(operands, keep)), 'a refused call wrote an operand'
