"""TEST INFRASTRUCTURE ONLY: the driver of the element-wise contract tests (include/ffgpu.h: inputs are never written, `out`
may alias an input exactly, elements are canonical on return).

One case = one entry point, one alias pattern, one size, one alignment class.  All operands of a case are views into ONE
backing tensor  guard | a | guard | b | ... | guard | o | guard | o2 | guard  (guards: at least 64 elements of 0xA5).  The
call is issued twice in a row on the same stream: in place the second call reads what the first one wrote; with a fresh
output the second call takes the first result as its first operand and writes a second fresh slot.  (On the device the
second call is therefore the one whose stores go out under the kept-in-cache policy of handoff.hpp.)  A device-side copy of
the tensor is taken between the two calls, so the state after EACH call is compared, byte for byte, with an image built on
the host: the output slot holds the reference result, every other byte -- operands and guards -- is what was uploaded.

Expected values never come from the code under test: fields of up to 128 bits take the C oracle's element-wise ADD / SUB /
MUL / NEG / REDUCE (OracleRef; scalars as broadcast arrays, muladd and beaver_combine composed, pow by square-and-multiply over
whole arrays), 24-byte fields Python integers (IntRef).  An inverse is checked by what defines it: canonical, zero exactly
where the input is zero, a * r == 1 elsewhere -- the inverse is unique, so this is an exact comparison.  A square root
(sqrt_cl, primes = 1 mod 4: sqrt_fields()) is not unique: the expectation is oracle.pyoracle.sqrt_prime on Python integers,
element by element, for every width -- the root the reference returns and its value for a non-residue (tests/golden/sqrt.json).

Nothing here imports the GPU at module level: tests/test_elementwise_contract_host.py drives the same code against
tests/cpuctx.CpuFieldContext and against deliberately wrong contexts."""
import numpy as np

GUARD_ELEMS = 64
GUARD_BYTE = 0xA5
SMALL_SIZES = (0, 1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129)
LARGE_SIZES = (1023, 1024, 1025, 4099)
ALIGN_SIZES = (1, 17, 65, 129, 1025)
BIG_EXP_MAX_N = 129                 # the exponents q - 2 and 3e' + 1 stop here
BIG_EXPS = ('q-2', '3e+1')

OPERANDS = {'add': 'ab', 'sub': 'ab', 'mul': 'ab', 'neg': 'a', 'reduce': 'a', 'add_scalar': 'a', 'mul_scalar': 'a',
            'rsub_scalar': 'a', 'muladd': 'abc', 'pow': 'a', 'inv': 'a', 'beaver_combine': 'zxyde', 'sqrt_cl': 'a'}

# alias patterns per number of array operands: name -> (slot of every operand, slot of the output); 'o' is a fresh slot
PATTERNS = {
    1: {'fresh': ('a', 'o'), 'o=a': ('a', 'a')},
    2: {'fresh': ('ab', 'o'), 'o=a': ('ab', 'a'), 'o=b': ('ab', 'b'), 'a=b': ('aa', 'o'), 'o=a=b': ('aa', 'a')},
    3: {'fresh': ('abc', 'o'), 'o=a': ('abc', 'a'), 'o=b': ('abc', 'b'), 'o=c': ('abc', 'c'), 'a=b,o=c': ('aac', 'c'),
        'o=a=b=c': ('aaa', 'a')},
    5: {'fresh': ('zxyde', 'o'), 'o=z': ('zxyde', 'z'), 'o=x': ('zxyde', 'x'), 'o=d': ('zxyde', 'd')},
}
FRESH_AND_IN_PLACE = {1: ('fresh', 'o=a'), 2: ('fresh', 'o=a'), 3: ('fresh', 'o=a'), 5: ('fresh', 'o=z')}


class ContractViolation(AssertionError):
    """kinds: which of 'out' (wrong result), 'input' (an operand that is not the output changed), 'guard' (bytes outside
    every operand changed) were seen; tests/share_contract.py adds 'pad' (bytes between the n elements of a row and its
    stride changed), tests/prss_contract.py 'canonical' (an output element that is not below the order)"""

    def __init__(self, kinds, message):
        super().__init__(message)
        self.kinds = frozenset(kinds)


def order_of(modulus, binary):
    return 1 << (modulus.bit_length() - 1) if binary else modulus


def ints_to_bytes(vals, eb):
    return np.frombuffer(b''.join(int(v).to_bytes(eb, 'little') for v in vals), dtype=np.uint8).copy()


def bytes_to_ints(raw, eb):
    b = np.ascontiguousarray(raw).tobytes()
    return [int.from_bytes(b[i:i + eb], 'little') for i in range(0, len(b), eb)]


def nonzero_elems(raw, eb):
    return raw.reshape(-1, eb).any(axis=1)


# ---- square roots: the reference, element by element --------------------------------------------------------------------
SQRT_POOL = 1024                    # distinct random operands of sqrt_cl per field: the integer reference runs once per value
DEEP_WALK_BOUND = 50000
_sqrt_memo = {}
_deep_memo = {}
_pool_memo = {}


def sqrt_ints(p, vals):
    """oracle.pyoracle.sqrt_prime on Python integers, every distinct (p, value) computed once per process"""
    from oracle import pyoracle as po
    F = po.Field(p, False)
    memo = _sqrt_memo.setdefault(p, {})
    out = []
    for v in vals:
        r = memo.get(v)
        if r is None:
            r = memo[v] = po.sqrt_prime(F, v)
        out.append(r)
    return out


def sqrt_depth(p, a):
    """how many candidates b = 1, 2, ... the reference tries for a != 0 until b^2 - 4a is a non-residue"""
    b = 1
    while pow((b * b - 4 * a) % p, (p - 1) >> 1, p) != p - 1:
        b += 1
    return b


def deep_elements(p):
    """{6: the first 64 squares i^2, i = 1, 2, ..., of depth >= 6, 8: the first 8 of depth >= 8, 11: the first 2 of depth >= 11};
    the walk stops at DEEP_WALK_BOUND candidates (or at p), so a list may come back short: the callers assert"""
    if p not in _deep_memo:
        need = {6: 64, 8: 8, 11: 2}
        found = {d: [] for d in need}
        for i in range(1, min(p, DEEP_WALK_BOUND + 1)):
            a = i * i % p
            d = sqrt_depth(p, a)
            for lvl, k in need.items():
                if d >= lvl and len(found[lvl]) < k and a not in found[lvl]:
                    found[lvl].append(a)
            if all(len(found[lvl]) == k for lvl, k in need.items()):
                break
        _deep_memo[p] = found
    return _deep_memo[p]


def sqrt_specials(p):
    """0, 1, p - 1, 4^-1 and 9 * 4^-1 (b^2 - 4a = 0 at b = 1 and at b = 3: a candidate to pass over), and the deepest element
    the walk found (none for a field as small as GF(13))"""
    inv4 = pow(4, -1, p)
    deep = deep_elements(p)
    deepest = next((deep[lvl][0] for lvl in (11, 8, 6) if deep[lvl]), None)
    return [0, 1, p - 1, inv4, 9 * inv4 % p] + ([deepest] if deepest is not None else [])


# ---- references ---------------------------------------------------------------------------------------------------------
class OracleRef:
    """fields of at most 128 bits: oracle/fforacle.c through coracle.CField.ew; arrays are flat uint8 limb images"""

    def __init__(self, co, modulus, binary):
        self.co, self.modulus, self.binary = co, int(modulus), bool(binary)
        self.cf = co.CField(self.modulus, self.binary)
        self.eb = self.cf.eb
        self.q = order_of(self.modulus, self.binary)

    def add(self, a, b):
        return self.cf.ew(self.co.ADD, a, b)

    def sub(self, a, b):
        return self.cf.ew(self.co.SUB, a, b)

    def mul(self, a, b):
        return self.cf.ew(self.co.MUL, a, b)

    def neg(self, a):
        return self.cf.ew(self.co.NEG, a)

    def reduce(self, a):
        return self.cf.ew(self.co.REDUCE, a)

    def const(self, s, n):
        return np.tile(np.frombuffer(int(s).to_bytes(self.eb, 'little'), dtype=np.uint8), n)

    def pow(self, a, e):
        r = self.const(1, a.size // self.eb)
        for bit in bin(e)[2:]:
            r = self.mul(r, r)
            if bit == '1':
                r = self.mul(r, a)
        return r

    def sqrt_cl(self, a):
        return ints_to_bytes(sqrt_ints(self.modulus, bytes_to_ints(a, self.eb)), self.eb)

    def check_inv(self, a, r):
        """None if r is the element-wise inverse of a (zero for zero), else what is wrong at the first bad element"""
        eb = self.eb
        n = a.size // eb
        bad = ~self.canonical(r)
        if bad.any():
            return 'not canonical at element %d' % int(np.argmax(bad))
        za, zr = ~nonzero_elems(a, eb), ~nonzero_elems(r, eb)
        if (za != zr).any():
            return 'zero pattern differs at element %d' % int(np.argmax(za != zr))
        one = (self.mul(a, r).reshape(n, eb) != self.const(1, n).reshape(n, eb)).any(axis=1) & ~za
        if one.any():
            return 'a * r != 1 at element %d' % int(np.argmax(one))
        return None

    def canonical(self, r):
        """per element: is it canonical?  One-word elements by comparison (below p; no bit at or above the degree), the
        others by the oracle's REDUCE leaving them unchanged"""
        eb = self.eb
        if eb <= 8:
            v = np.ascontiguousarray(r).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[eb])
            if not self.binary:
                return v < v.dtype.type(self.modulus)
            deg = self.modulus.bit_length() - 1
            return (v >> v.dtype.type(deg)) == 0 if deg < 8 * eb else np.ones(v.size, dtype=bool)
        n = r.size // eb
        return ~(self.reduce(r).reshape(n, eb) != r.reshape(n, eb)).any(axis=1)

    def random(self, rng, n):
        """uniform canonical elements"""
        eb = self.eb
        if eb <= 8:
            dt = {1: np.uint8, 4: np.uint32, 8: np.uint64}[eb]
            return rng.integers(0, self.q, size=n, dtype=np.uint64, endpoint=False).astype(dt).view(np.uint8) if self.q < 2**64 \
                else rng.integers(0, 256, size=n * eb, dtype=np.uint8)
        return self.reduce(rng.integers(0, 256, size=n * self.eb, dtype=np.uint8))


class IntRef:
    """24-byte prime fields: Python integers in NumPy object arrays, %, built-in pow"""

    def __init__(self, modulus):
        self.modulus, self.binary, self.eb, self.q = int(modulus), False, 24, int(modulus)

    def _obj(self, raw):
        b = np.ascontiguousarray(raw).tobytes()
        v = np.empty(len(b) // 24, dtype=object)
        v[:] = [int.from_bytes(b[i:i + 24], 'little') for i in range(0, len(b), 24)]
        return v

    def _raw(self, v):
        return np.frombuffer(b''.join([int(x).to_bytes(24, 'little') for x in v]), dtype=np.uint8).copy()

    def add(self, a, b):
        return self._raw((self._obj(a) + self._obj(b)) % self.q)

    def sub(self, a, b):
        return self._raw((self._obj(a) - self._obj(b)) % self.q)

    def mul(self, a, b):
        return self._raw((self._obj(a) * self._obj(b)) % self.q)

    def neg(self, a):
        return self._raw((-self._obj(a)) % self.q)

    def reduce(self, a):
        return self._raw(self._obj(a) % self.q)

    def const(self, s, n):
        return np.tile(np.frombuffer(int(s).to_bytes(24, 'little'), dtype=np.uint8), n)

    def pow(self, a, e):
        return self._raw(np.array([pow(x, e, self.q) for x in self._obj(a)], dtype=object))

    def sqrt_cl(self, a):
        return ints_to_bytes(sqrt_ints(self.q, bytes_to_ints(a, 24)), 24)

    def check_inv(self, a, r):
        A, R = self._obj(a), self._obj(r)
        for what, bad in (('not canonical', R >= self.q), ('zero pattern differs', (A == 0) != (R == 0)),
                          ('a * r != 1', (A != 0) & (A * R % self.q != 1))):
            bad = np.asarray(bad, dtype=bool)
            if bad.any():
                return '%s at element %d' % (what, int(np.argmax(bad)))
        return None

    def random(self, rng, n):
        return self.reduce(rng.integers(0, 256, size=n * 24, dtype=np.uint8))


def make_ref(co, modulus, binary):
    return IntRef(modulus) if co.elem_bytes(modulus, binary) == 24 else OracleRef(co, modulus, binary)


def apply_ref(ref, entry, args):
    """the reference result of one call; args: the operands' limb images in the entry point's order"""
    name, _, par = entry
    n = args[0].size // ref.eb
    if name in ('add', 'sub', 'mul'):
        return getattr(ref, name)(args[0], args[1])
    if name in ('neg', 'reduce'):
        return getattr(ref, name)(args[0])
    if name == 'add_scalar':
        return ref.add(args[0], ref.const(par, n))
    if name == 'mul_scalar':
        return ref.mul(args[0], ref.const(par, n))
    if name == 'rsub_scalar':
        return ref.sub(ref.const(par, n), args[0])
    if name == 'muladd':
        return ref.add(ref.mul(args[0], args[1]), args[2])
    if name == 'pow':
        return ref.pow(args[0], par)
    if name == 'sqrt_cl':
        return ref.sqrt_cl(args[0])
    if name == 'beaver_combine':                      # z + d*y + e*x (+ d*e)
        z, x, y, d, e = args
        r = ref.add(ref.add(z, ref.mul(d, y)), ref.mul(e, x))
        return ref.add(r, ref.mul(d, e)) if par else r
    raise ValueError(name)


def invoke(ctx, entry, ops, out):
    name, _, par = entry
    if name in ('add', 'sub', 'mul'):
        getattr(ctx, name)(ops[0], ops[1], out=out)
    elif name in ('neg', 'reduce'):
        getattr(ctx, name)(ops[0], out=out)
    elif name in ('add_scalar', 'mul_scalar', 'rsub_scalar', 'pow'):
        getattr(ctx, name)(ops[0], par, out=out)
    elif name == 'muladd':
        ctx.muladd(ops[0], ops[1], ops[2], out=out)
    elif name == 'inv':
        ctx.inv(ops[0], out=out, check_zero=False)
    elif name == 'sqrt_cl':
        ctx.sqrt_cl(ops[0], out=out)
    elif name == 'beaver_combine':
        ctx.beaver_combine(ops[0], ops[1], ops[2], ops[3], ops[4], par, out=out)
    else:
        raise ValueError(name)


def all_entries(q, rnd):
    """(entry point, label, parameter) of every call the contract covers; rnd: one random canonical scalar.  sqrt_cl, which
    serves the primes = 1 mod 4 only, comes last and only for those (the order of a binary field is even)"""
    ent = [(name, '', None) for name in ('add', 'sub', 'mul', 'neg', 'reduce')]
    for name in ('add_scalar', 'mul_scalar', 'rsub_scalar'):
        ent += [(name, label, s) for label, s in (('0', 0), ('1', 1), ('q-1', q - 1), ('rnd', rnd))]
    ent.append(('muladd', '', None))
    ent += [('pow', label, e) for label, e in (('0', 0), ('1', 1), ('2', 2), ('65537', 65537), ('q-2', q - 2),
                                               ('3e+1', 3 * (2**20 - 1) + 1))]
    ent.append(('inv', '', None))
    ent += [('beaver_combine', 'add_de=%d' % v, bool(v)) for v in (0, 1)]
    if q % 4 == 1:
        ent.append(('sqrt_cl', '', None))
    return ent


def sqrt_cases_of(q):
    """(pairs, matrix cases, alignment cases) that sqrt_cl adds to run_matrix / run_alignment on a field of order q"""
    return (2, 2 * len(SMALL_SIZES) + 2 * len(LARGE_SIZES), 2 * 2 * len(ALIGN_SIZES)) if q % 4 == 1 else (0, 0, 0)


def layout(eb, n, slots, one_in):
    """byte offset of every slot and the size of the tensor: at least GUARD_ELEMS elements of guard before, between and after
    the slots; a slot starts at an offset = 0 (mod 16), or = eb (mod 16) -- one element in -- if it is in `one_in`"""
    off, cur = {}, 0
    for s in slots:
        cur = -(-(cur + GUARD_ELEMS * eb) // 16) * 16
        if s in one_in:
            cur += eb
        off[s] = cur
        cur += n * eb
    return off, -(-(cur + GUARD_ELEMS * eb) // 16) * 16


# ---- the driver ---------------------------------------------------------------------------------------------------------
class Driver:
    def __init__(self, ctx, ref, seed=1):
        assert ctx.elem_bytes == ref.eb
        self.ctx, self.ref, self.eb, self.q = ctx, ref, ref.eb, ref.q
        self.rng = np.random.default_rng(seed)
        self.rnd_scalar = bytes_to_ints(ref.random(self.rng, 1), self.eb)[0]
        self.entries = all_entries(self.q, self.rnd_scalar)
        self.seen = set()          # (entry point, label, pattern, n, alignment class) of every case that was checked
        self.steps = 0             # calls compared with the reference (two per case)
        self._mixed = 0
        self._rot = 0
        self._prev = None

    def entry(self, name, label=''):
        return next(e for e in self.entries if e[0] == name and e[1] == label)

    def draw(self, entry, n):
        """canonical random elements with 0, 1 and q - 1 planted; raw limbs for reduce; for sqrt_cl see draw_sqrt"""
        if entry[0] == 'reduce':
            return self.rng.integers(0, 256, size=n * self.eb, dtype=np.uint8)
        if entry[0] == 'sqrt_cl':
            return self.draw_sqrt(n)
        v = self.ref.random(self.rng, n).reshape(n, self.eb)
        if n >= 3:
            pos = self.rng.choice(n, size=3, replace=False)
            for p, s in zip(pos, (0, 1, self.q - 1)):
                v[p] = self.ref.const(s, 1)
        elif n == 2:
            v[int(self.rng.integers(2))] = 0
        return v.reshape(-1)

    def sqrt_pool(self):
        """SQRT_POOL canonical random elements, the same for every driver of a field, as an (., eb) byte matrix"""
        if self.q not in _pool_memo:
            _pool_memo[self.q] = self.ref.random(np.random.default_rng(self.q % 1009 + 4), SQRT_POOL).reshape(SQRT_POOL, self.eb)
        return _pool_memo[self.q]

    def draw_sqrt(self, n):
        """operands of sqrt_cl: elements of the pool (about half of them non-residues) at random, with sqrt_specials planted at
        random places -- all of them from n = 6 on; below, as many as fit, starting with another one at every draw"""
        pool = self.sqrt_pool()
        v = pool[self.rng.integers(0, len(pool), size=n)].copy()
        sp = sqrt_specials(self.q)
        k = min(n, len(sp))
        pos = self.rng.choice(n, size=k, replace=False) if n else ()
        for i, p in enumerate(pos):
            v[p] = self.ref.const(sp[(self._rot + i) % len(sp)], 1)
        self._rot += k
        return v.reshape(-1)

    def _view(self, base, off, n):
        from mpyc_amd import engine
        eb = self.eb
        t = base[off:off + n * eb].view(engine._torch_dtype(eb))
        limbs = engine.limbs_of(eb)
        return engine.DevArray(self.ctx, t.reshape(n, limbs) if limbs else t, n)

    def run(self, entry, pattern, n, align='aligned', inputs=None, chain=True):
        """one case: two chained calls, each compared with the reference.  align: 'aligned', 'one-in' (every operand one element
        past a 16-byte boundary) or 'mixed' (one operand, taken in turn, one element in).  inputs: slot -> limb image, for
        cases that plant their own values.  chain=False: the first call only."""
        import torch
        eb, ref = self.eb, self.ref
        ops, out = PATTERNS[len(OPERANDS[entry[0]])][pattern]
        ins = sorted(set(ops), key=ops.index)
        slots = ins + (['o', 'o2'] if out == 'o' else [])
        if align == 'aligned':
            one_in = ()
        elif align == 'one-in':
            one_in = slots
        else:
            one_in = (slots[self._mixed % len(slots)],)
            self._mixed += 1
        off, total = layout(eb, n, slots, one_in)
        img = np.full(total, GUARD_BYTE, dtype=np.uint8)
        for s in slots:
            if inputs is not None and s in inputs:
                img[off[s]:off[s] + n * eb] = inputs[s]
            elif s in ins:
                img[off[s]:off[s] + n * eb] = self.draw(entry, n)
            else:
                img[off[s]:off[s] + n * eb] = self.rng.integers(0, 256, size=n * eb, dtype=np.uint8)
        base = torch.from_numpy(img.copy()).to(self.ctx.torch_device)
        view = {s: self._view(base, off[s], n) for s in slots}
        # call 2: in place the same call again; with a fresh output the first result replaces the first operand
        calls = [(ops, out)]
        calls.append((ops.replace(ops[0], 'o'), 'o2') if out == 'o' else (ops, out))
        invoke(self.ctx, entry, [view[s] for s in calls[0][0]], view[calls[0][1]])
        if chain:
            mid = base.clone()
            invoke(self.ctx, entry, [view[s] for s in calls[1][0]], view[calls[1][1]])
            got = [mid.cpu().numpy(), base.cpu().numpy()]
        else:
            got = [base.cpu().numpy()]
        self._prev = base            # stays allocated: the next case's tensor is another address range (no false hand-off)
        want = img
        for step in range(len(got)):
            cops, cout = calls[step]
            args = [want[off[s]:off[s] + n * eb].copy() for s in cops]
            lo = off[cout]
            where = (entry[0], entry[1], pattern, n, align, 'call %d' % (step + 1))
            if entry[0] == 'inv':
                res = got[step][lo:lo + n * eb].copy()
                msg = ref.check_inv(args[0], res)
                if msg:
                    raise ContractViolation({'out'}, '%r: inverse %s' % (where, msg))
            else:
                res = apply_ref(ref, entry, args)
            want = want.copy()
            want[lo:lo + n * eb] = res
            self._compare(got[step], want, off, n, slots, cout, where)
            self.steps += 1
        self.seen.add((entry[0], entry[1], pattern, n, align))

    def _compare(self, got, want, off, n, slots, out, where):
        if np.array_equal(got, want):
            return
        eb = self.eb
        kinds, notes = set(), []
        covered = np.zeros(got.size, dtype=bool)
        for s in slots:
            lo, hi = off[s], off[s] + n * eb
            covered[lo:hi] = True
            diff = np.nonzero(got[lo:hi] != want[lo:hi])[0]
            if diff.size:
                i = int(diff[0]) // eb
                kinds.add('out' if s == out else 'input')
                notes.append('%s %r differs at element %d of %d: got %s, want %s' % (
                    'output' if s == out else 'operand', s, i, n, bytes(got[lo + i * eb:lo + (i + 1) * eb])[::-1].hex(),
                    bytes(want[lo + i * eb:lo + (i + 1) * eb])[::-1].hex()))
        diff = np.nonzero((got != want) & ~covered)[0]
        if diff.size:
            kinds.add('guard')
            notes.append('guard byte %d changed (slots at %r, %d bytes each)' % (int(diff[0]), off, n * eb))
        raise ContractViolation(kinds, '%r: %s' % (where, '; '.join(notes)))

    # ---- the matrices -----------------------------------------------------------------------------------------------
    def patterns_of(self, entry):
        return tuple(PATTERNS[len(OPERANDS[entry[0]])])

    def in_place_pair(self, entry):
        return FRESH_AND_IN_PLACE[len(OPERANDS[entry[0]])]

    def run_matrix(self, small=SMALL_SIZES, large=LARGE_SIZES, entries=None):
        """every entry point x every alias pattern at the small sizes; fresh and in place at the large ones"""
        for e in entries or self.entries:
            for n in small:
                for pat in self.patterns_of(e):
                    self.run(e, pat, n)
            if e[1] in BIG_EXPS:
                continue
            for n in large:
                for pat in self.in_place_pair(e):
                    self.run(e, pat, n)

    def run_alignment(self, sizes=ALIGN_SIZES, entries=None, aligns=('one-in', 'mixed')):
        """every entry point, fresh and in place, with all operands one element in and with one operand one element in"""
        for e in entries or self.entries:
            for n in sizes:
                if e[1] in BIG_EXPS and n > BIG_EXP_MAX_N:
                    continue
                for pat in self.in_place_pair(e):
                    for align in aligns:
                        self.run(e, pat, n, align)

    def run_reduced(self, small=SMALL_SIZES, large=LARGE_SIZES):
        """the reduced matrix of the contexts without hand-off tracking: add, mul, muladd, mul_scalar; fresh, o = a, o = b"""
        ent = [self.entry('add'), self.entry('mul'), self.entry('muladd')] + [e for e in self.entries if e[0] == 'mul_scalar']
        for e in ent:
            pats = [p for p in ('fresh', 'o=a', 'o=b') if p in self.patterns_of(e)]
            for n in small:
                for pat in pats:
                    self.run(e, pat, n)
            for n in large:
                for pat in pats[:2]:
                    self.run(e, pat, n)

    def plant(self, entry, n, values_at):
        """a drawn operand with the given {position: value} planted"""
        v = self.draw(entry, n).reshape(n, self.eb)
        for pos, s in values_at.items():
            v[pos] = self.ref.const(s, 1)
        return v.reshape(-1)


def noncanonical_values(modulus, binary, eb):
    """limb patterns at which a reduction can go wrong, as far as they fit W = 8 * eb bits: for a prime p, 2p and the largest
    multiple of p below 2^W with their neighbours; for GF(2^n) the modulus, 2^n, 2^n | 1; all ones and a lone top bit"""
    W = 8 * eb
    if binary:
        deg = modulus.bit_length() - 1
        vals = [modulus, 1 << deg, (1 << deg) | 1]
    else:
        top = ((1 << W) - 1) // modulus * modulus
        vals = [modulus, modulus + 1, 2 * modulus - 1, 2 * modulus, top - 1, top, top + 1]
    return [v for v in vals + [(1 << W) - 1, 1 << (W - 1)] if v < (1 << W)]


def run_noncanonical_reduce(drv, clmod, n=257):
    """reduce, fresh and in place, on random raw limbs with noncanonical_values planted (first, last and spread between);
    the expectation is Python's % p, for GF(2^n) clmod (oracle.pyoracle.clmod), and the driver's reference must agree"""
    ref = drv.ref
    vals = noncanonical_values(ref.modulus, ref.binary, ref.eb)
    raw = bytes_to_ints(drv.rng.integers(0, 256, size=n * ref.eb, dtype=np.uint8), ref.eb)
    pos = [0, n - 1] + [3 + 5 * i for i in range(len(vals) - 2)]
    for p, v in zip(pos, vals):
        raw[p] = v
    want = [clmod(x, ref.modulus) if ref.binary else x % ref.modulus for x in raw]
    img = ints_to_bytes(raw, ref.eb)
    assert np.array_equal(ref.reduce(img), ints_to_bytes(want, ref.eb)), 'the reference disagrees with Python integers'
    for pat in ('fresh', 'o=a'):
        drv.run(drv.entry('reduce'), pat, n, inputs={'a': img})
    return len(vals)


# PolicyKind of mpyc_amd/csrc/policy_build.hpp (what tests/hostcheck.cpp reports) and the name engine.FieldContext.reduction has
POLICY_KINDS = {'PM64_MERSENNE': 1, 'PM64_K64': 2, 'PM64_GEN': 3, 'RC64': 4, 'RC32': 5, 'PM128_K128': 6, 'PM128_GEN': 7, 'PM96': 8,
                'MONT128': 9, 'PM192': 13, 'MONT192': 14}
REDUCTION_OF = {'PM': 'pseudo-mersenne', 'RC': 'reciprocal', 'MO': 'montgomery'}
SQRT_ROWS = ('RC32', 'PM64_GEN', 'PM64_K64', 'RC64', 'PM96', 'PM128_GEN', 'PM128_K128', 'MONT128', 'PM192', 'MONT192')


def sqrt_fields():
    """(modulus, policy, element bytes) of the fields sqrt_cl is tested on: primes = 1 mod 4, at least one per prime policy and
    storage size.  The Mersenne policy has none: 2^k - 1 = 3 mod 4 for every k >= 2."""
    return [(13, 'RC32', 4), (2**31 - 19, 'RC32', 4),
            (2**33 - 79, 'PM64_GEN', 8), (2**40 - 87, 'PM64_GEN', 8), (2**63 - 259, 'PM64_GEN', 8),
            (2**64 - 59, 'PM64_K64', 8),
            (0x5bd1e995c6a4a715, 'RC64', 8),
            (2**80 - 143, 'PM96', 12), (2**96 - 87, 'PM96', 12),
            (2**100 - 15, 'PM128_GEN', 16), (2**127 - 39, 'PM128_GEN', 16),
            (2**128 - 159, 'PM128_K128', 16),
            (2**127 + 2**100 + 0x101, 'MONT128', 16), (0xc2b2ae3d27d4eb4f165667b19e377991, 'MONT128', 16),
            (2**136 - 243, 'PM192', 24), (2**192 - 399, 'PM192', 24),
            (2**135 + 33, 'MONT192', 24), (2**192 - 2**40 + 341, 'MONT192', 24)]


def contract_fields():
    """(modulus, binary) of every field the contract tests run on: ALL_FIELDS of tests/test_gpu_scan.py -- one modulus per
    ops_*.hip unit and reduction policy -- and two dense binary moduli, whose products take the window kernel"""
    from mpyc_amd.gfpx import BinaryPolynomial
    primes = [2**31 - 1, 19, 2**61 - 1, 2**64 - 189, 2**63 - 25, 6616326157076047771, 2**80 - 65, 2**96 - 17, 2**127 - 1,
              2**128 - 173, 2**127 + 2**100 + 0x101, 2**136 - 113, 2**192 - 2**40 + 341]
    binaries = [0x11b, 0x1002b, 0x10000008d, 0x1000000000000001b, 0x100000000000000000000000000000087]
    dense = [int(BinaryPolynomial.next_irreducible((1 << 64) | (1 << 45))),
             int(BinaryPolynomial.next_irreducible((1 << 128) | (1 << 100)))]
    return [(p, False) for p in primes] + [(m, True) for m in binaries + dense]
