"""Device-side engine: a field context plus device-resident limb arrays.

This is the layer directly above the C ABI (include/ffgpu.h).  Arrays live in HBM
as fixed-width little-endian limbs (DevArray); Python integers exist only at the
API edges (from_ints / to_ints), because boxing 10^7 PyLongs costs more than every
kernel here put together.  torch is used for device memory (caching allocator,
streams, interop with torch.distributed); all arithmetic goes through libffgpu.so.
"""
from __future__ import annotations

import collections
import ctypes
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _ffi

_MASK64 = (1 << 64) - 1

# what FieldContext.conv2d_plan reports (ffgm_conv2d_plan_t of include/ffgpu_math.h); grid: (workgroups, senders)
Conv2dPlan = collections.namedtuple('Conv2dPlan', 'tile_rows tile_cols out_channels in_channels_step flush_rows wide grid lds_bytes')


def _np_dtype(eb: int):
    return {1: np.uint8, 4: np.uint32, 8: np.uint64, 12: np.uint32, 16: np.uint64, 24: np.uint64}[eb]


def _torch_dtype(eb: int):
    return {1: torch.uint8, 4: torch.int32, 8: torch.int64, 12: torch.int32, 16: torch.int64, 24: torch.int64}[eb]


_MASK64_OBJ = (1 << 64) - 1


def limbs_of(eb: int) -> int:
    """Trailing limb dimension of a device tensor: 0 (scalar dtype), 2 (16 bytes = 2 x int64), 3 (12 bytes = 3 x int32,
    24 bytes = 3 x int64)."""
    return {16: 2, 12: 3, 24: 3}.get(eb, 0)


def ints_to_np(vals: Iterable[int], eb: int) -> np.ndarray:
    """Canonical Python ints -> limb array ((n,) for eb<=8, (n,2) uint64 for eb=16, (n,3) uint32 for eb=12)."""
    if isinstance(vals, np.ndarray) and vals.dtype != object:
        vals = vals.reshape(-1)
        if eb in (16, 24):
            out = np.zeros((vals.size, eb // 8), dtype=np.uint64)
            out[:, 0] = vals.astype(np.uint64)
            return out
        if eb == 12:
            v64 = vals.astype(np.uint64)
            out = np.zeros((vals.size, 3), dtype=np.uint32)
            out[:, 0] = (v64 & np.uint64(0xffffffff)).astype(np.uint32)
            out[:, 1] = (v64 >> np.uint64(32)).astype(np.uint32)
            return out
        return vals.astype(_np_dtype(eb))
    vals = list(vals) if not isinstance(vals, (list, np.ndarray)) else vals
    n = len(vals)
    if n == 0:
        return np.zeros((0, limbs_of(eb)) if limbs_of(eb) else 0, dtype=_np_dtype(eb))
    obj = vals if isinstance(vals, np.ndarray) else np.array(vals, dtype=object)
    if eb <= 8:
        return obj.astype(np.uint64).astype(_np_dtype(eb))
    # two / three limbs: split inside NumPy's object loops (3 big-int operations per element instead of a Python-level
    # to_bytes + join per element)
    if eb == 24:
        try:
            out = np.empty((n, 3), dtype=np.uint64)
            out[:, 0] = (obj & _MASK64_OBJ).astype(np.uint64)
            out[:, 1] = ((obj >> 64) & _MASK64_OBJ).astype(np.uint64)
            out[:, 2] = (obj >> 128).astype(np.uint64)
            return out
        except (TypeError, OverflowError):
            buf = b''.join(int(v).to_bytes(24, 'little') for v in obj)
            return np.frombuffer(buf, dtype=np.uint64).reshape(n, 3).copy()
    try:
        lo64 = (obj & _MASK64_OBJ).astype(np.uint64)
        hi64 = (obj >> 64).astype(np.uint64)
    except (TypeError, OverflowError):       # elements that are not plain ints (numpy integers in an object array, ...)
        ints = [int(v) for v in obj]
        buf = b''.join(v.to_bytes(16, 'little') for v in ints)
        both = np.frombuffer(buf, dtype=np.uint64).reshape(n, 2)
        lo64, hi64 = both[:, 0], both[:, 1]
    if eb == 16:
        out = np.empty((n, 2), dtype=np.uint64)
        out[:, 0], out[:, 1] = lo64, hi64
        return out
    out = np.empty((n, 3), dtype=np.uint32)
    out[:, 0] = (lo64 & np.uint64(0xffffffff)).astype(np.uint32)
    out[:, 1] = (lo64 >> np.uint64(32)).astype(np.uint32)
    out[:, 2] = hi64.astype(np.uint32)
    return out


def np_to_objects(arr: np.ndarray, eb: int) -> np.ndarray:
    """Limb array -> 1-D object ndarray of Python ints, converted inside NumPy's C loops (this is the price of the
    reference's representation: ~30 ns per element for one limb, three object operations per element for two)."""
    if eb == 24:
        a = arr.reshape(-1, 3)
        if not len(a):
            return np.empty(0, dtype=object)
        return (a[:, 2].astype(object) << 128) | (a[:, 1].astype(object) << 64) | a[:, 0].astype(object)
    if eb == 16:
        a = arr.reshape(-1, 2)
        if not len(a):
            return np.empty(0, dtype=object)
        return (a[:, 1].astype(object) << 64) | a[:, 0].astype(object)
    if eb == 12:
        a = arr.view(np.uint32).reshape(-1, 3)
        if not len(a):
            return np.empty(0, dtype=object)
        lo = a[:, 0].astype(np.uint64) | (a[:, 1].astype(np.uint64) << np.uint64(32))
        return (a[:, 2].astype(object) << 64) | lo.astype(object)
    return arr.reshape(-1).astype(object)


def np_to_ints(arr: np.ndarray, eb: int) -> List[int]:
    return np_to_objects(arr, eb).tolist()


class DevArray:
    """n field elements resident in HBM (row of limbs).  Thin wrapper over a torch tensor."""

    __slots__ = ('ctx', 't', 'n')

    def __init__(self, ctx: 'FieldContext', t: torch.Tensor, n: int):
        self.ctx, self.t, self.n = ctx, t, n

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()

    def to_numpy(self) -> np.ndarray:
        a = self.t.cpu().numpy()
        eb = self.ctx.elem_bytes
        if eb in (4, 12):
            a = a.view(np.uint32)
        elif eb >= 8:
            a = a.view(np.uint64)
        return a

    def to_ints(self) -> List[int]:
        return np_to_ints(self.to_numpy(), self.ctx.elem_bytes)

    def clone(self) -> 'DevArray':
        return DevArray(self.ctx, self.t.clone(), self.n)

    def __len__(self):
        return self.n


class DevMatrix:
    """(rows, n) elements with 256-byte aligned rows (so every row takes the 16 B/lane path)."""

    __slots__ = ('ctx', 't', 'rows', 'n', 'stride')

    def __init__(self, ctx, t, rows, n, stride):
        self.ctx, self.t, self.rows, self.n, self.stride = ctx, t, rows, n, stride

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()

    def row(self, i: int) -> DevArray:
        eb = self.ctx.elem_bytes
        if limbs_of(eb):
            return DevArray(self.ctx, self.t[i, :self.n, :], self.n)
        return DevArray(self.ctx, self.t[i, :self.n], self.n)

    def to_numpy(self) -> np.ndarray:
        a = self.t.cpu().numpy()
        eb = self.ctx.elem_bytes
        if eb in (4, 12):
            a = a.view(np.uint32)
        elif eb >= 8:
            a = a.view(np.uint64)
        return a[:, :self.n]

    def to_ints(self) -> List[List[int]]:
        a = self.to_numpy()
        return [np_to_ints(a[i], self.ctx.elem_bytes) for i in range(self.rows)]


class RngState:
    """Key / nonce / rounds of the device CSPRNG in device memory (FieldContext.rng_state)."""

    __slots__ = ('ctx', 't', 'pending')

    def __init__(self, ctx, t):
        self.ctx, self.t, self.pending = ctx, t, 0

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()

    def take_offset(self) -> int:
        """Deferred advance (ffgpu_rng_state_advance): the next launch of a sequence draws from nonce + offset and
        leaves the device nonce alone; commit() advances it once by the number of launches."""
        off = self.pending
        self.pending += 1
        return off

    def commit(self):
        """One nonce update for all deferred launches since the last commit (stream-ordered, capturable).  Every
        engine call that advances the nonce itself commits first, so offsets never collide with it."""
        if self.pending:
            by, self.pending = self.pending, 0
            _ffi.check(self.ctx._L.ffgpu_rng_state_advance(self.ctx._h, self.ptr, by, self.ctx._stream()), 'rng_state_advance')

    def nonce(self) -> int:
        w = self.t.cpu().numpy().view(np.uint32)
        return int(w[8]) | (int(w[9]) << 32)


class CapturedLaunches:
    """A fixed sequence of engine calls captured into a HIP graph (through torch.cuda.CUDAGraph, which
    captures every launch issued on the capture stream -- including libffgpu's, since the engine always
    launches on torch's current stream).  For launch-bound work: a gate on a few thousand elements is
    three kernels of ~3 us each, dominated by per-launch host cost when issued one by one.
    The captured kernels read and write the SAME device buffers on every replay: refresh inputs with
    tensor.copy_() into those buffers, then replay()."""

    def __init__(self, fn, warmup: int = 2):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.result = fn()          # arrays allocated during capture live in the graph's pool

    def replay(self):
        self.graph.replay()


class FieldContext:
    """One finite field on one GPU.  modulus: prime p, or (binary=True) the bit pattern of the
    irreducible polynomial.  Mirrors what finfields.GF(modulus) fixes for an array type
    (finfields.py:23-60)."""

    def __init__(self, modulus: int, binary: bool = False, device: Optional[int] = None):
        L = _ffi.lib()
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.modulus = int(modulus)
        self.binary = bool(binary)
        self.device = int(device)
        h = ctypes.c_void_p()
        nl = 3
        rc = L.ffgpu_ctx_create(_ffi.BINARY if binary else _ffi.PRIME, _ffi.limbs(self.modulus, nl), nl,
                                self.device, ctypes.byref(h))
        _ffi.check(rc, 'ctx_create')
        self._h = h
        self.elem_bytes = L.ffgpu_ctx_elem_bytes(h)
        self.limbs = limbs_of(self.elem_bytes)        # trailing limb dimension of device tensors (0, 2 or 3)
        self.scalar_limbs = int(L.ffgpu_ctx_scalar_limbs(h))   # limbs per host scalar in the C ABI (2; 3 for 24-byte fields)
        self.reduction = _ffi.RED_NAMES.get(L.ffgpu_ctx_reduction(h), '?')
        if binary:
            self.order = 1 << (self.modulus.bit_length() - 1)
        else:
            self.order = self.modulus
        self._L = L

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                self._L.ffgpu_ctx_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- memory ---------------------------------------------------------
    @property
    def torch_device(self):
        return torch.device('cuda', self.device)

    def pci_bus_id(self) -> str:
        """PCI bus id of this context's GPU (multi-process runs report it per rank)."""
        buf = ctypes.create_string_buffer(32)
        _ffi.check(self._L.ffgpu_device_pci_bus_id(self.device, buf, 32), "device_pci_bus_id")
        return buf.value.decode()

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def empty(self, n: int) -> DevArray:
        eb = self.elem_bytes
        shape = (n, limbs_of(eb)) if limbs_of(eb) else (n,)
        return DevArray(self, torch.empty(shape, dtype=_torch_dtype(eb), device=self.torch_device), n)

    def empty_matrix(self, rows: int, n: int) -> DevMatrix:
        eb = self.elem_bytes
        per = 64 if eb == 12 else 32 if eb == 24 else 256 // eb      # elements per 256-byte-aligned pitch unit (768 B for 12- and 24-byte elements)
        stride = max(per, (n + per - 1) // per * per)
        if (stride * eb) % 16384 == 0:
            # rows a multiple of 16 KiB apart alias onto the same HBM channels when m rows are
            # written at once (measured -12 % at a 64 MiB pitch): skew the pitch by 17 x 256 B
            stride += 17 * per
        shape = (rows, stride, limbs_of(eb)) if limbs_of(eb) else (rows, stride)
        return DevMatrix(self, torch.empty(shape, dtype=_torch_dtype(eb), device=self.torch_device), rows, n,
                         stride)

    def from_numpy(self, a: np.ndarray) -> DevArray:
        """a: limb array as produced by ints_to_np (already canonical)."""
        eb = self.elem_bytes
        a = np.ascontiguousarray(a)
        if not a.flags.writeable:
            a = a.copy()
        n = a.shape[0]
        if eb in (4, 12):
            t = torch.from_numpy(a.view(np.int32))
        elif eb >= 8:
            t = torch.from_numpy(a.view(np.int64))
        else:
            t = torch.from_numpy(a)
        return DevArray(self, t.to(self.torch_device), n)

    def from_ints(self, vals: Sequence[int]) -> DevArray:
        """Canonical ints (0 <= v < order) -> device."""
        return self.from_numpy(ints_to_np(vals, self.elem_bytes))

    def matrix_from_numpy(self, a: np.ndarray) -> DevMatrix:
        rows, n = a.shape[0], a.shape[1]
        mtx = self.empty_matrix(rows, n)
        for i in range(rows):
            mtx.row(i).t.copy_(self.from_numpy(a[i]).t)
        return mtx

    # ---- operand checks ---------------------------------------------------
    # The kernels take raw pointers and ONE element count: every operand (and a caller-supplied output) must have
    # exactly that many elements and belong to this field, otherwise a launch would read or write past an
    # allocation.  Share rows arrive from peers (from_wire derives their length from the message size), so a short
    # or ragged row must be refused here -- the reference's field.array(shares) raises on the same input.
    def _same(self, n: int, *arrays, what: str = 'operand'):
        for a in arrays:
            if a is None:
                continue
            if a.ctx is not self and (a.ctx.modulus != self.modulus or a.ctx.binary != self.binary
                                      or a.ctx.device != self.device):
                raise ValueError(f'{what} belongs to a different field context')
            if a.n != n:
                raise ValueError(f'{what} has {a.n} elements, expected {n}')

    def _out(self, n: int, out: Optional[DevArray], what: str = 'output') -> DevArray:
        """The caller's output, checked as an operand of n elements, or a fresh array.  The test is `is None`: an empty
        DevArray is falsy, and the caller gets back the object it passed."""
        if out is None:
            return self.empty(n)
        self._same(n, out, what=what)
        return out

    def _rows(self, rows: Sequence[DevArray], lambdas: Sequence[int], n: int, what: str):
        """(nrows, row pointers, lambdas) of the sub-share rows an apply end recombines: rows of n elements each, one lambda
        per row."""
        args = self._rec_args(rows, lambdas, 1)
        self._same(n, *rows, what=what)
        return args

    def _axis(self, what: str, a: DevArray, outer: int, k: int, inner: int, kmin: int = 1, na: Optional[int] = None,
              stack: int = 1):
        """An (outer, k, inner) call with k >= kmin whose operand is `stack` contiguous (outer, na, inner) arrays (na = k by
        default)."""
        if outer < 1 or k < kmin or inner < 1:
            raise ValueError(f'{what}: outer and inner must be at least 1, k at least {kmin}')
        self._same(stack * outer * (k if na is None else na) * inner, a, what=f'{what} operand')

    def _bit_matrix(self, what: str, x: DevArray, l: int, lmin: int = 1) -> int:
        """n of the (l, n) or (n, l) bit matrix x, l >= lmin"""
        if l < lmin or x.n % l:
            raise ValueError(f'{what}: the operand is not a bit matrix of l >= {lmin} bits per element')
        return x.n // l

    def _out_matrix(self, out: Optional[DevMatrix], rows: int, n: int) -> DevMatrix:
        if out is None:
            return self.empty_matrix(rows, n)
        if out.rows < rows or out.n != n:
            raise ValueError(f'output matrix is ({out.rows}, {out.n}), need ({rows}, {n})')
        return out

    # ---- element-wise -----------------------------------------------------
    def _ew2(self, fn, a: DevArray, b: DevArray, out: Optional[DevArray]) -> DevArray:
        self._same(a.n, b)
        out = self._out(a.n, out)
        _ffi.check(fn(self._h, a.ptr, b.ptr, out.ptr, a.n, self._stream()), fn.__name__)
        return out

    def add(self, a, b, out=None):
        return self._ew2(self._L.ffgpu_add, a, b, out)

    def sub(self, a, b, out=None):
        return self._ew2(self._L.ffgpu_sub, a, b, out)

    def mul(self, a, b, out=None):
        return self._ew2(self._L.ffgpu_mul, a, b, out)

    def neg(self, a, out=None):
        out = self._out(a.n, out)
        _ffi.check(self._L.ffgpu_neg(self._h, a.ptr, out.ptr, a.n, self._stream()), 'neg')
        return out

    def reduce(self, raw: DevArray, out=None):
        out = self._out(raw.n, out)
        _ffi.check(self._L.ffgpu_reduce(self._h, raw.ptr, out.ptr, raw.n, self._stream()), 'reduce')
        return out

    def _ews(self, fn, a, scalar: int, out):
        out = self._out(a.n, out)
        _ffi.check(fn(self._h, a.ptr, _ffi.limbs(scalar, self.scalar_limbs), out.ptr, a.n, self._stream()), fn.__name__)
        return out

    def add_scalar(self, a, s: int, out=None):
        return self._ews(self._L.ffgpu_add_scalar, a, s, out)

    def mul_scalar(self, a, s: int, out=None):
        return self._ews(self._L.ffgpu_mul_scalar, a, s, out)

    def rsub_scalar(self, a, s: int, out=None):
        return self._ews(self._L.ffgpu_rsub_scalar, a, s, out)

    def muladd(self, a, b, c, out=None):
        self._same(a.n, b, c)
        out = self._out(a.n, out)
        _ffi.check(self._L.ffgpu_muladd(self._h, a.ptr, b.ptr, c.ptr, out.ptr, a.n, self._stream()), 'muladd')
        return out

    def pow(self, a, e: int, out=None):
        """a ** e for a public exponent 0 <= e < 2^128, one kernel (finfields.py:1159-1187)."""
        if e < 0 or e >> 192:
            raise ValueError('exponent out of range')
        out = self._out(a.n, out)
        _ffi.check(self._L.ffgpu_pow(self._h, a.ptr, _ffi.limbs(e, 3), 3, out.ptr, a.n, self._stream()), 'pow')
        return out

    def inv(self, a, out=None, check_zero: bool = True):
        """Element-wise inverse (batched, one kernel).  Raises ZeroDivisionError like the reference
        if any element is zero (costs one device->host flag read); check_zero=False skips that."""
        out = self._out(a.n, out)
        flag = torch.zeros(1, dtype=torch.int32, device=self.torch_device) if check_zero else None
        _ffi.check(self._L.ffgpu_inv(self._h, a.ptr, out.ptr, a.n, flag.data_ptr() if check_zero else None,
                                     self._stream()), 'inv')
        if check_zero and int(flag.item()):
            raise ZeroDivisionError('inverse of 0 does not exist')
        return out

    def beaver_combine(self, z, x, y, d, e, add_de: bool, out=None):
        """z + d*y + e*x (+ d*e): local step of Beaver multiplication (not a reference function; see ffgpu.h)."""
        self._same(z.n, x, y, d, e)
        out = self._out(z.n, out)
        _ffi.check(self._L.ffgpu_beaver_combine(self._h, z.ptr, x.ptr, y.ptr, d.ptr, e.ptr, int(bool(add_de)), out.ptr,
                                                z.n, self._stream()), 'beaver_combine')
        return out

    # ---- sharing ----------------------------------------------------------
    def split(self, secrets: DevArray, coeffs: Optional[DevMatrix], t: int, m: int,
              out: Optional[DevMatrix] = None, mul_by: Optional[DevArray] = None) -> DevMatrix:
        """np_random_split with the coefficient matrix supplied (thresha.py:47-64).
        mul_by: fuse the local product secrets*mul_by (runtime.py:1134-1138)."""
        n = secrets.n
        if t and (coeffs is None or coeffs.rows < t or coeffs.n != n):
            raise ValueError('coefficient matrix must be (t, n)')
        self._same(n, mul_by)
        out = self._out_matrix(out, m, n)
        cptr = coeffs.ptr if t else None
        cstride = coeffs.stride if t else 0
        if mul_by is None:
            rc = self._L.ffgpu_split(self._h, secrets.ptr, cptr, cstride, t, m, out.ptr, out.stride, n,
                                     self._stream())
        else:
            rc = self._L.ffgpu_mul_split(self._h, secrets.ptr, mul_by.ptr, cptr, cstride, t, m, out.ptr,
                                         out.stride, n, self._stream())
        _ffi.check(rc, 'split')
        return out

    def rng_state(self, key: Optional[bytes] = None, nonce: int = 0, rounds: int = 20) -> 'RngState':
        """Device-resident generator state (key from the host CSPRNG by default).  Pass it as `state=` to
        split_rng: the kernels then read key/nonce from device memory and the nonce advances on the device
        after every call, so the calls can be captured in a HIP graph and every replay draws fresh
        coefficients."""
        import secrets as _secrets
        key = key if key is not None else _secrets.token_bytes(32)
        if len(key) != 32:
            raise ValueError('key must be 32 bytes')
        t = torch.zeros(int(self._L.ffgpu_rng_state_bytes()), dtype=torch.uint8, device=self.torch_device)
        _ffi.check(self._L.ffgpu_rng_state_init(self._h, t.data_ptr(), key, nonce, rounds, self._stream()),
                   'rng_state_init')
        return RngState(self, t)

    def rng_coeffs(self, key: bytes, nonce: int, t: int, n: int, rounds: int = 20,
                   out: Optional[DevMatrix] = None) -> DevMatrix:
        """Materialise the (t, n) coefficient matrix the fused split_rng kernel draws for
        (key, nonce, rounds) -- device CSPRNG, mpyc_amd/csrc/rng.hpp."""
        if len(key) != 32:
            raise ValueError('key must be 32 bytes')
        out = out or self.empty_matrix(t, n)
        _ffi.check(self._L.ffgpu_rng_coeffs(self._h, key, nonce, rounds, t, out.ptr, out.stride, n,
                                            self._stream()), 'rng_coeffs')
        return out

    def split_rng(self, secrets: DevArray, t: int, m: int, key: Optional[bytes] = None, nonce: int = 0,
                  rounds: int = 20, out: Optional[DevMatrix] = None,
                  mul_by: Optional[DevArray] = None, state: Optional['RngState'] = None) -> DevMatrix:
        """np_random_split with coefficients drawn on the device (production mode): the t*n
        random coefficients never touch HBM.  key: 32 bytes; default = fresh from the host CSPRNG
        (the reference draws from `secrets` too, thresha.py:58)."""
        import secrets as _secrets
        n = secrets.n
        self._same(n, mul_by)
        out = self._out_matrix(out, m, n)
        if state is not None:
            state.commit()
            _ffi.check(self._L.ffgpu_split_rng_state(self._h, secrets.ptr, mul_by.ptr if mul_by is not None else None,
                                                     state.ptr, t, m, out.ptr, out.stride, n, self._stream()),
                       'split_rng_state')
            return out
        if key is None:
            key = _secrets.token_bytes(32)
        if len(key) != 32:
            raise ValueError('key must be 32 bytes')
        if mul_by is None:
            rc = self._L.ffgpu_split_rng(self._h, secrets.ptr, key, nonce, rounds, t, m, out.ptr, out.stride, n,
                                         self._stream())
        else:
            rc = self._L.ffgpu_mul_split_rng(self._h, secrets.ptr, mul_by.ptr, key, nonce, rounds, t, m, out.ptr,
                                             out.stride, n, self._stream())
        _ffi.check(rc, 'split_rng')
        return out

    def gate(self, rows_a: Sequence[DevArray], lam_a: Sequence[int], rows_b: Optional[Sequence[DevArray]],
             lam_b: Optional[Sequence[int]], t: int, m: int, key: Optional[bytes] = None, nonce: int = 0,
             rounds: int = 20, state: Optional['RngState'] = None, out: Optional[DevMatrix] = None) -> DevMatrix:
        """Fused chain gate (ffgpu_gate_rng): shares of A*B with A = sum lam_a[j]*rows_a[j], B likewise
        (rows_b None: B = A); recombination, product and share generation in one pass."""
        import secrets as _secrets
        n = rows_a[0].n
        ka, pa, la = self._rec_args(rows_a, lam_a, 1)
        kb, pb, lb = self._rows(rows_b, lam_b, n, 'share row') if rows_b else (0, None, None)
        out = self._out_matrix(out, m, n)
        if state is None and key is None:
            key = _secrets.token_bytes(32)
        if state is not None:
            state.commit()
        _ffi.check(self._L.ffgpu_gate_rng(self._h, pa, la, ka, pb, lb, kb, key, nonce, rounds,
                                          state.ptr if state is not None else None, t, m, out.ptr, out.stride, n,
                                          self._stream()), 'gate_rng')
        return out

    def gate_batch(self, rows_a: Sequence[DevArray], lam_a: Sequence[int], stride_a: int,
                   rows_b: Optional[Sequence[DevArray]], lam_b: Optional[Sequence[int]], stride_b: int,
                   t: int, m: int, nbatch: int, out: DevMatrix, out_rows_per_party: int,
                   key: Optional[bytes] = None, nonce: int = 0, rounds: int = 20,
                   state: Optional['RngState'] = None) -> DevMatrix:
        """`nbatch` chain gates in one launch (ffgpu_gate_rng_batch): rows_a / rows_b are the operand rows of gate 0;
        gate y reads them `y * stride_a` (`y * stride_b`) elements further on.  `out` is a DevMatrix of
        m * out_rows_per_party rows used as [recipient][sender]: gate y writes the share row for party i+1 into row
        i * out_rows_per_party + y.  The caller owns the layout (mpyc_amd/protocols.py); operand rows of gate 0
        and the output are length-checked here."""
        import secrets as _secrets
        n = rows_a[0].n
        if nbatch < 1 or out_rows_per_party < nbatch or out.rows < m * out_rows_per_party or out.n != n:
            raise ValueError('output block does not hold m x nbatch share rows of n elements')
        ka, pa, la = self._rec_args(rows_a, lam_a, 1)
        kb, pb, lb = self._rows(rows_b, lam_b, n, 'share row') if rows_b else (0, None, None)
        if state is None and key is None:
            key = _secrets.token_bytes(32)
        defer = 0
        if state is not None:
            nonce, defer = state.take_offset(), 1          # deferred advance: state.commit() follows the sequence
        _ffi.check(self._L.ffgpu_gate_rng_batch(self._h, pa, la, ka, stride_a, pb, lb, kb, stride_b, key, nonce, rounds,
                                                state.ptr if state is not None else None, defer, t, m, out.ptr,
                                                out.stride * out_rows_per_party, out.stride, n, nbatch,
                                                self._stream()), 'gate_rng_batch')
        return out

    def _rec_args(self, rows: Sequence[DevArray], lambdas: Sequence[int], w: int):
        k = len(rows)
        if not k:
            raise ValueError('no share rows')
        if len(lambdas) != w * k:
            raise ValueError('need w*k lambda values')
        self._same(rows[0].n, *rows, what='share row')
        ptrs = (ctypes.c_void_p * k)(*[r.ptr for r in rows])
        lam = self._scalars(lambdas)
        return k, ptrs, lam

    def recombine(self, rows: Sequence[DevArray], lambdas: Sequence[int], w: int = 1, out=None):
        """out[r] = sum_j lambdas[r*k+j] * rows[j]  (thresha.py:119-132)."""
        k, ptrs, lam = self._rec_args(rows, lambdas, w)
        n = rows[0].n
        if w == 1:
            out = self._out(n, out)
            stride = n
        else:
            out = self._out_matrix(out, w, n)
            stride = out.stride
        _ffi.check(self._L.ffgpu_recombine(self._h, ptrs, lam, k, w, out.ptr, stride, n, self._stream()),
                   'recombine')
        return out

    def recombine_plan(self, rows: Sequence[DevArray], lambdas: Sequence[int], out, w: int = 1):
        """Pre-marshal a recombination (row pointers + Lagrange vector) for repeated launches:
        the returned callable only issues the kernel (hot loops, benchmarks)."""
        k, ptrs, lam = self._rec_args(rows, lambdas, w)
        n = rows[0].n
        if w == 1:
            self._same(n, out, what='output')
        else:
            self._out_matrix(out, w, n)
        stride = n if w == 1 else out.stride
        fn, h, optr = self._L.ffgpu_recombine, self._h, out.ptr
        keep = (rows, out)

        def launch():
            _ffi.check(fn(h, ptrs, lam, k, w, optr, stride, n, self._stream()), 'recombine')
            return keep[1]
        return launch

    def matmul(self, A: DevArray, B: DevArray, M: int, K: int, N: int, out: Optional[DevArray] = None) -> DevArray:
        """C (M, N) = A (M, K) @ B (K, N): contiguous row-major operands (finfields.py:1126-1135)."""
        if A.n != M * K or B.n != K * N:
            raise ValueError('matmul: operand sizes do not match the shapes')
        if out is not None:
            eb = self.elem_bytes
            for x in (A, B):                       # C is written while other tiles still read A and B
                if out.ptr < x.ptr + x.n * eb and x.ptr < out.ptr + out.n * eb:
                    raise ValueError('matmul: the output overlaps an operand')
        out = self._out(M * N, out, 'matmul output')
        _ffi.check(self._L.ffgpu_matmul(self._h, A.ptr, K, B.ptr, N, out.ptr, N, M, K, N, self._stream()), 'matmul')
        return out

    def matmul_stack(self, A: DevArray, B: DevArray, batch: int, M: int, K: int, N: int, a_stride: int, b_stride: int,
                     out: Optional[DevArray] = None) -> DevArray:
        """C[b] (M, N) = A[b] (M, K) @ B[b] (K, N) for b < batch in one library call (NumPy's matmul on stacks of matrices,
        finfields.py:1126-1135; the local product of runtime.np_matmul, runtime.py:2481-2541).  Row-major matrices, matrix b
        of an operand a_stride / b_stride ELEMENTS after matrix b - 1; stride 0: the one matrix is shared by the whole
        stack.  The result is a contiguous stack of batch * M * N elements."""
        if batch < 0 or M < 0 or K < 0 or N < 0:
            raise ValueError('matmul_stack: negative size')
        for what, x, stride, per in (('left', A, a_stride, M * K), ('right', B, b_stride, K * N)):
            if stride != 0 and stride < per:
                raise ValueError(f'matmul_stack: the {what} stride is smaller than a matrix')
            if x.n < ((batch - 1) * stride + per if batch else 0):
                raise ValueError('matmul_stack: operand sizes do not match the shapes')
        n = batch * M * N
        if out is not None:
            eb = self.elem_bytes
            for x in (A, B):                       # matrices of C are written while others still read A and B
                if out.ptr < x.ptr + x.n * eb and x.ptr < out.ptr + out.n * eb:
                    raise ValueError('matmul_stack: the output overlaps an operand')
        out = self._out(n, out, 'matmul_stack output')
        _ffi.check(self._L.ffgpu_matmul_stack(self._h, A.ptr, K, a_stride, B.ptr, N, b_stride, out.ptr, N, M * N,
                                              M, K, N, batch, self._stream()), 'matmul_stack')
        return out

    def convolve(self, a: DevArray, v: DevArray, out: Optional[DevArray] = None) -> DevArray:
        """Full convolution out[k] = sum_j a[k - j] * v[j], len(a) + len(v) - 1 elements, in one kernel with memory linear
        in the operands (finfields.py:796-801; the local part of runtime.np_convolve, runtime.py:2627).  The operand
        order does not matter; modes 'same' / 'valid' are slices the caller takes."""
        if a.n == 0 or v.n == 0:
            raise ValueError('convolve: non-empty arrays required')
        n = a.n + v.n - 1
        self._same(a.n, a, what='convolve operand')
        self._same(v.n, v, what='convolve operand')
        out = self._out(n, out, 'convolve output')
        _ffi.check(self._L.ffgpu_convolve(self._h, a.ptr, a.n, v.ptr, v.n, out.ptr, self._stream()), 'convolve')
        return out

    def _scan_workspace(self, outer: int, k: int, inner: int):
        """tile-aggregate workspace of scan / axis_reduce: one per stream, grown on demand (with the default tile one
        element per 4096 input elements, 2048 above 8-byte elements); (pointer, bytes)"""
        need = int(self._L.ffgpu_scan_workspace_bytes(self._h, outer, k, inner))
        if need == 0:
            return None, 0
        wss = self.__dict__.setdefault('_scan_ws', {})
        key = self._stream()
        ws = wss.get(key)
        if ws is None or ws.numel() < need:
            ws = wss[key] = torch.empty(need, dtype=torch.uint8, device=self.torch_device)
        return ws.data_ptr(), ws.numel()

    def _scan_args(self, what: str, a: DevArray, outer: int, k: int, inner: int, nout: int, out: Optional[DevArray],
                   in_place_ok: bool):
        self._axis(what, a, outer, k, inner)
        if out is not None:
            eb = self.elem_bytes
            if not (in_place_ok and out.ptr == a.ptr):    # tiles / columns are written while others are still read
                if out.ptr < a.ptr + a.n * eb and a.ptr < out.ptr + out.n * eb:
                    raise ValueError(f'{what}: the output overlaps the operand')
        return self._out(nout, out, f'{what} output')

    def scan(self, a: DevArray, outer: int, k: int, inner: int, mul: bool = False, with_initial: bool = False,
             out: Optional[DevArray] = None) -> DevArray:
        """Inclusive prefix sums (mul: products) along k of the contiguous (outer, k, inner) array `a` (np.cumsum / np.cumprod
        on field arrays, finfields.py:801, 807; runtime.np_cumsum, runtime.py:3510-3549).  with_initial: k + 1 entries along
        the axis, the identity first.  out may be `a` itself when with_initial is False."""
        kk = k + (1 if with_initial else 0)
        out = self._scan_args('scan', a, outer, k, inner, outer * kk * inner, out, not with_initial)
        ws, wsb = self._scan_workspace(outer, k, inner)
        _ffi.check(self._L.ffgpu_scan(self._h, 1 if mul else 0, a.ptr, out.ptr, outer, k, inner, 1 if with_initial else 0,
                                      ws, wsb, self._stream()), 'scan')
        return out

    def axis_reduce(self, a: DevArray, outer: int, k: int, inner: int, mul: bool = False,
                    out: Optional[DevArray] = None) -> DevArray:
        """Sums (mul: products) along k of the contiguous (outer, k, inner) array `a`: outer * inner elements
        (FiniteFieldArray.sum / .prod along an axis, finfields.py:1332-1349)."""
        out = self._scan_args('axis_reduce', a, outer, k, inner, outer * inner, out, False)
        ws, wsb = self._scan_workspace(outer, k, inner)
        _ffi.check(self._L.ffgpu_axis_reduce(self._h, 1 if mul else 0, a.ptr, out.ptr, outer, k, inner, ws, wsb,
                                             self._stream()), 'axis_reduce')
        return out

    # ---- secure comparison: the local steps of runtime.np_sgn (runtime.py:3622-3693), prime fields ----
    def sgn_mask(self, a: DevArray, rbits: DevArray, rdivl: DevArray, l: int, out: Optional[DevArray] = None) -> DevArray:
        """masked[h] = a[h] + 2^l + sum_i rbits[h*l+i] 2^(l-1-i) + rdivl[h] 2^l, the value np_sgn opens
        (runtime.py:3649-3657).  rbits: n*l bit shares, element-major, most significant bit first."""
        n = a.n
        self._same(n, rdivl, what='sgn_mask operand')
        self._same(n * l, rbits, what='sgn_mask bit shares')
        out = self._out(n, out, 'sgn_mask output')
        _ffi.check(self._L.ffgpu_sgn_mask(self._h, a.ptr, rbits.ptr, rdivl.ptr, l, out.ptr, n, self._stream()), 'sgn_mask')
        return out

    def sgn_expand(self, c: DevArray, a: DevArray, rbits: DevArray, sbit: Optional[DevArray], l: int, want_e: bool = True,
                   want_nx: bool = False):
        """From the opened c: (e, nx, z) of runtime.py:3658-3671, :3679 -- e the (l+1, n) operands of the product tree,
        nx = 1 - Xor as (l, n), both bit-major, z = (c mod 2^l) - a_r.  e / nx are None unless asked for; sbit (the
        sign-mask bit shares) may be None when want_e is False."""
        n = a.n
        self._same(n, c, sbit, what='sgn_expand operand')
        self._same(n * l, rbits, what='sgn_expand bit shares')
        if want_e and sbit is None:
            raise ValueError('sgn_expand: e needs the sign-mask bit shares')
        e = self.empty((l + 1) * n) if want_e else None
        nx = self.empty(l * n) if want_nx else None
        z = self.empty(n)
        _ffi.check(self._L.ffgpu_sgn_expand(self._h, c.ptr, a.ptr, rbits.ptr, sbit.ptr if sbit is not None else None, l,
                                            e.ptr if want_e else None, nx.ptr if want_nx else None, z.ptr, n,
                                            self._stream()), 'sgn_expand')
        return e, nx, z

    def sgn_finish(self, w: DevArray, sbit: DevArray, z: DevArray, l: int, out: Optional[DevArray] = None) -> DevArray:
        """lt[h] = (z[h] + ((1 - 2 [w[h] == 0]) (2 sbit[h] - 1) + 3) 2^(l-1)) 2^-l: the share of [a < 0] from the
        opened masked product w (runtime.py:3674-3676)."""
        n = w.n
        self._same(n, sbit, z, what='sgn_finish operand')
        out = self._out(n, out, 'sgn_finish output')
        _ffi.check(self._L.ffgpu_sgn_finish(self._h, w.ptr, sbit.ptr, z.ptr, l, out.ptr, n, self._stream()), 'sgn_finish')
        return out

    # ---- sorting network: the two ends of a compare-exchange stage of runtime.np_sort (runtime.py:1764-1770), prime fields ----
    def cx_pairs(self, k: int, p: int, d: int, r: int) -> int:
        """pairs of stage (p, d, r) of Batcher's merge-exchange network over k elements: |{i < k - d : i & p == r}|;
        0 when (p, d, r) is not a stage"""
        if min(k, p, d, r) < 0:
            return 0
        return int(self._L.ffgpu_cx_pairs(k, p, d, r))

    def _cx_args(self, what: str, a: DevArray, outer: int, k: int, inner: int, p: int, d: int, r: int) -> int:
        self._axis(what, a, outer, k, inner)
        if min(p, d, r) < 0:
            raise ValueError(f'{what}: ({p}, {d}, {r}) is not a stage')
        return self.cx_pairs(k, p, d, r)

    def cx_diff(self, a: DevArray, outer: int, k: int, inner: int, p: int, d: int, r: int,
                out: Optional[DevArray] = None) -> DevArray:
        """out[o, j, i] = a[o, I_j + d, i] - a[o, I_j, i] over the contiguous (outer, k, inner) array `a`, I the index set of
        stage (p, d, r): the compact (outer, P, inner) differences np_sort compares with zero (runtime.py:1764-1767)."""
        P = self._cx_args('cx_diff', a, outer, k, inner, p, d, r)
        out = self._out(outer * P * inner, out, 'cx_diff output')
        _ffi.check(self._L.ffgpu_cx_diff(self._h, a.ptr, out.ptr, outer, k, inner, p, d, r, self._stream()), 'cx_diff')
        return out

    def cx_apply(self, a: DevArray, rows: Sequence[DevArray], lambdas: Sequence[int], outer: int, k: int, inner: int, p: int,
                 d: int, r: int) -> DevArray:
        """a[o, I_j, i] += h, a[o, I_j + d, i] -= h in place with h = sum_s lambdas[s] * rows[s] over the compact
        (outer, P, inner) rows: the exchange of np_sort (runtime.py:1768-1770) with the recombination of the re-shared
        product folded in.  Returns a."""
        P = self._cx_args('cx_apply', a, outer, k, inner, p, d, r)
        nrows, ptrs, lam = self._rows(rows, lambdas, outer * P * inner, 'cx_apply row')
        _ffi.check(self._L.ffgpu_cx_apply(self._h, a.ptr, ptrs, lam, nrows, outer, k, inner, p, d, r, self._stream()),
                   'cx_apply')
        return a

    # ---- bit decomposition: the local steps of runtime.np_to_bits (runtime.py:4391-4456) and the carry network of
    # np_add_bits (runtime.py:4301-4334), prime fields; bit index k least significant first ----
    def carry_rounds(self, l: int) -> int:
        """rounds of the prefix-carry network over l bits: ceil(log2 l)"""
        r = int(self._L.ffgpu_carry_rounds(l))
        if r < 0:
            raise ValueError('carry_rounds: bit length out of range')
        return r

    def carry_level(self, l: int, round: int):
        """(Rc, Rd, [(k, q), ...]) of a round: Rc c-products G[q] P[k], then Rd d-products P[q] P[k] (csrc/bits_geom.hpp)"""
        rc, rd = ctypes.c_int(), ctypes.c_int()
        _ffi.check(self._L.ffgpu_carry_rows(l, round, ctypes.byref(rc), ctypes.byref(rd)), 'carry_rows')
        ks, qs = (ctypes.c_uint8 * 63)(), (ctypes.c_uint8 * 63)()
        _ffi.check(self._L.ffgpu_carry_level(l, round, ks, qs), 'carry_level')
        return rc.value, rd.value, [(ks[j], qs[j]) for j in range(rc.value + rd.value)]

    def carry_rows(self, l: int, round: int) -> int:
        """product rows R = Rc + Rd of a round"""
        rc, rd, _ = self.carry_level(l, round)
        return rc + rd

    def bits_mask(self, a: DevArray, rbits: DevArray, rdivl: DevArray, l: int, offset: int,
                  out: Optional[DevArray] = None) -> DevArray:
        """masked[h] = a[h] + offset + rdivl[h] 2^l - sum_k rbits[h*l+k] 2^k, the value np_to_bits opens
        (runtime.py:4414-4415, 4446).  rbits: n*l bit shares, element-major, least significant bit first."""
        n = a.n
        self._same(n, rdivl, what='bits_mask operand')
        self._same(n * l, rbits, what='bits_mask bit shares')
        out = self._out(n, out, 'bits_mask output')
        _ffi.check(self._L.ffgpu_bits_mask(self._h, a.ptr, rbits.ptr, rdivl.ptr, self._scalars([int(offset) % self.modulus]), l,
                                           out.ptr, n, self._stream()), 'bits_mask')
        return out

    def bits_expand(self, c: DevArray, rbits: DevArray, l: int):
        """From the opened c: (G, P), bit-major (l, n): G[k] = cb_k ? r_k : 0, P[k] = cb_k ? 1 - r_k : r_k with cb_k bit k
        of c mod 2^l -- the leaves of np_add_bits for public bits (runtime.py:4309-4314, 4447-4448)."""
        n = c.n
        self._same(n * l, rbits, what='bits_expand bit shares')
        g, p = self.empty(l * n), self.empty(l * n)
        _ffi.check(self._L.ffgpu_bits_expand(self._h, c.ptr, rbits.ptr, l, g.ptr, p.ptr, n, self._stream()), 'bits_expand')
        return g, p

    def carry_prod(self, g: DevArray, p: DevArray, l: int, round: int, out: Optional[DevArray] = None) -> DevArray:
        """The local products of a round, compact (R, n): G[q_j] P[k_j] for the c-rows, then P[q_j] P[k_j] for the d-rows
        (runtime.py:4320-4325)."""
        n = self._bit_matrix('carry_prod', g, l)
        self._same(l * n, p, what='carry_prod operand')
        out = self._out(self.carry_rows(l, round) * n, out, 'carry_prod output')
        _ffi.check(self._L.ffgpu_carry_prod(self._h, g.ptr, p.ptr, l, round, out.ptr, n, self._stream()), 'carry_prod')
        return out

    def carry_apply(self, g: DevArray, p: DevArray, rows: Sequence[DevArray], lambdas: Sequence[int], l: int, round: int):
        """G[k_j] += v for the c-rows, P[k_j] = v for the d-rows, in place, with v = sum_s lambdas[s] * rows[s] over the compact
        (R, n) rows: the merge of np_add_bits (runtime.py:4320-4325) with the recombination of the re-shared products folded
        in.  Returns (g, p)."""
        n = self._bit_matrix('carry_apply', g, l)
        self._same(l * n, p, what='carry_apply operand')
        nrows, ptrs, lam = self._rows(rows, lambdas, self.carry_rows(l, round) * n, 'carry_apply row')
        _ffi.check(self._L.ffgpu_carry_apply(self._h, g.ptr, p.ptr, ptrs, lam, nrows, l, round, n, self._stream()),
                   'carry_apply')
        return g, p

    def bits_finish(self, c: DevArray, rbits: DevArray, g: DevArray, l: int, out: Optional[DevArray] = None) -> DevArray:
        """out[h*l+k] = rbits[h*l+k] + cb_k - 2 G[k*n+h] + G[(k-1)*n+h]: the shares of the bits, element-major
        (runtime.py:4332-4334)."""
        n = c.n
        self._same(n * l, rbits, g, what='bits_finish operand')
        out = self._out(n * l, out, 'bits_finish output')
        _ffi.check(self._L.ffgpu_bits_finish(self._h, c.ptr, rbits.ptr, g.ptr, l, out.ptr, n, self._stream()), 'bits_finish')
        return out

    # ---- tournament along an axis: the ends of a round of runtime.np_amax / np_amin (runtime.py:3413-3419, 3462-3468) and
    # runtime._np_argmax / _np_argmin (runtime.py:3806-3820, 3934-3948), prime fields.  k >= 2, n0 = k % 2, h = k // 2 pairs,
    # kc = h + n0 survivors; pair j is (n0 + j, kc + j) for TOUR_HALVES and (n0 + 2j, n0 + 2j + 1) for TOUR_ODD_EVEN ----
    TOUR_HALVES, TOUR_ODD_EVEN = 0, 1

    def _tour_args(self, what: str, a: DevArray, na: int, outer: int, k: int, inner: int, mode: int):
        self._axis(what, a, outer, k, inner, kmin=2, na=na)
        if mode not in (self.TOUR_HALVES, self.TOUR_ODD_EVEN):
            raise ValueError(f'{what}: unknown pairing {mode}')
        return k // 2, k // 2 + k % 2

    def tour_diff(self, a: DevArray, outer: int, k: int, inner: int, mode: int, neg: bool = False,
                  out: Optional[DevArray] = None) -> DevArray:
        """out[o, j, i] = a[o, second_j, i] - a[o, first_j, i] (neg: first - second) over the contiguous (outer, k, inner)
        array `a`: the compact (outer, h, inner) differences a round compares with zero (runtime.py:3415-3416, 3935-3936)."""
        h, _ = self._tour_args('tour_diff', a, k, outer, k, inner, mode)
        out = self._out(outer * h * inner, out, 'tour_diff output')
        _ffi.check(self._L.ffgpu_tour_diff(self._h, a.ptr, out.ptr, outer, k, inner, mode, 1 if neg else 0, self._stream()),
                   'tour_diff')
        return out

    def tour_select(self, a: DevArray, rows: Sequence[DevArray], lambdas: Sequence[int], outer: int, k: int, inner: int,
                    mode: int, neg: bool = False, out: Optional[DevArray] = None) -> DevArray:
        """The next level (outer, kc, inner): out[o, n0 + j, i] = a[o, first_j, i] + v (neg: - v) with
        v = sum_s lambdas[s] * rows[s] over the compact (outer, h, inner) rows, and the bye out[o, 0, i] = a[o, 0, i] when k is
        odd: the survivors of a round (runtime.py:3416-3418, 3938-3940) with the recombination of the re-shared product
        folded in."""
        h, kc = self._tour_args('tour_select', a, k, outer, k, inner, mode)
        nrows, ptrs, lam = self._rows(rows, lambdas, outer * h * inner, 'tour_select row')
        out = self._out(outer * kc * inner, out, 'tour_select output')
        _ffi.check(self._L.ffgpu_tour_select(self._h, a.ptr, ptrs, lam, nrows, out.ptr, outer, k, inner, mode, 1 if neg else 0,
                                             self._stream()), 'tour_select')
        return out

    def tour_unit_prod(self, u: DevArray, c: DevArray, outer: int, k: int, inner: int, out: Optional[DevArray] = None) -> DevArray:
        """out[o, j, i] = u[o, n0 + j, i] * c[o, j, i], compact (outer, h, inner): the local product of the upward pass of
        argmax, u the child level's (outer, kc, inner) unit vectors, c this level's comparison bits (runtime.py:3943-3944)."""
        h, kc = self._tour_args('tour_unit_prod', u, k // 2 + k % 2, outer, k, inner, self.TOUR_HALVES)
        self._same(outer * h * inner, c, what='tour_unit_prod bits')
        out = self._out(outer * h * inner, out, 'tour_unit_prod output')
        _ffi.check(self._L.ffgpu_tour_unit_prod(self._h, u.ptr, c.ptr, out.ptr, outer, k, inner, self._stream()), 'tour_unit_prod')
        return out

    def tour_unit_expand(self, u: DevArray, rows: Sequence[DevArray], lambdas: Sequence[int], outer: int, k: int, inner: int,
                         out: Optional[DevArray] = None) -> DevArray:
        """This level's unit vectors (outer, k, inner) from the child's (outer, kc, inner): out[o, n0 + 2j, i] =
        u[o, n0 + j, i] - v, out[o, n0 + 2j + 1, i] = v with v = sum_s lambdas[s] * rows[s] over the compact rows, and
        out[o, 0, i] = u[o, 0, i] when k is odd (runtime.py:3945-3948) with the recombination of u * c folded in."""
        h, kc = self._tour_args('tour_unit_expand', u, k // 2 + k % 2, outer, k, inner, self.TOUR_ODD_EVEN)
        nrows, ptrs, lam = self._rows(rows, lambdas, outer * h * inner, 'tour_unit_expand row')
        out = self._out(outer * k * inner, out, 'tour_unit_expand output')
        _ffi.check(self._L.ffgpu_tour_unit_expand(self._h, u.ptr, ptrs, lam, nrows, out.ptr, outer, k, inner, self._stream()),
                   'tour_unit_expand')
        return out

    # ---- first occurrence along an axis: the ends of a round of runtime.np_find (runtime.py:4603-4698), prime fields.  A level
    # is component-major (C, outer, kk, inner), component 0 = nf; rounds pair neighbours as TOUR_ODD_EVEN does; the leaf round
    # runs over kv = k + virt positions of the (outer, k, inner) bits, position k the public leaf (1, f(e)) ----
    FIND_MAX_VALUES = 4

    def _find_args(self, what: str, a: DevArray, outer: int, k: int, inner: int, ncomp: int, flip: int, virt: int, leaf: bool):
        if not 2 <= ncomp <= 1 + self.FIND_MAX_VALUES:
            raise ValueError(f'{what}: 2 to {1 + self.FIND_MAX_VALUES} components')
        if flip not in (0, 1) or virt not in (0, 1):
            raise ValueError(f'{what}: flip and virt are 0 or 1')
        self._axis(what, a, outer, k, inner, kmin=2 - virt, stack=1 if leaf else ncomp)     # a round needs two positions
        kv = k + virt
        return kv, kv // 2, kv // 2 + kv % 2

    def find_table(self, k: int, cs0: Sequence, cs1: Sequence, fe=None) -> DevArray:
        """The leaf table (F, 2, kv) of find_leaf_prod / find_leaf_apply from Python integers: cs0[j] and cs1[j] are the F
        values of cs_f(0, j) and cs_f(1, j) for j < k (a plain integer counts as F = 1), fe the F values of f(e) for the public
        leaf at position k (kv = k + 1) or None (kv = k).  Row (q, 0) is cs_f(0, .)_q, row (q, 1) cs_f(1, .)_q - cs_f(0, .)_q,
        with (f(e)_q, 0) in column k; negative values are reduced mod p."""
        if self.binary:
            raise ValueError('find_table: prime fields only')
        tup = lambda v: tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),)
        if k < 1 or len(cs0) != k or len(cs1) != k:
            raise ValueError('find_table: k values of cs_f(0, j) and of cs_f(1, j)')
        c0, c1 = [tup(v) for v in cs0], [tup(v) for v in cs1]
        nf_ = len(c0[0])
        if fe is not None:
            c0.append(tup(fe))
            c1.append(c0[-1])
        if not 1 <= nf_ <= self.FIND_MAX_VALUES or any(len(v) != nf_ for v in c0 + c1):
            raise ValueError(f'find_table: 1 to {self.FIND_MAX_VALUES} values per position, the same number everywhere')
        p = self.modulus
        return self.from_ints([x for q in range(nf_) for x in ([v[q] % p for v in c0] + [(w[q] - v[q]) % p for v, w in zip(c0, c1)])])

    def find_leaf_prod(self, bits: DevArray, tab: DevArray, outer: int, k: int, inner: int, ncomp: int, flip: int = 0, virt: int = 0,
                       out: Optional[DevArray] = None) -> DevArray:
        """out[q, o, j, i] = leaf_0(first_j) * (leaf_q(second_j) - leaf_q(first_j)), compact (ncomp, outer, h, inner): the local
        product of the first round of np_find over the kv = k + virt positions, pair j = (n0 + 2j, n0 + 2j + 1); leaf j is
        (b', tab[q, 0, j] + b' tab[q, 1, j]), b' = bits[o, j, i] (flip: 1 - bits), the public leaf (1, f(e)) at position k when
        virt (runtime.py:4679-4684)."""
        kv, h, _ = self._find_args('find_leaf_prod', bits, outer, k, inner, ncomp, flip, virt, True)
        self._same((ncomp - 1) * 2 * kv, tab, what='find_leaf_prod table')
        out = self._out(ncomp * outer * h * inner, out, 'find_leaf_prod output')
        _ffi.check(self._L.ffgpu_find_leaf_prod(self._h, bits.ptr, tab.ptr, out.ptr, outer, k, inner, ncomp, flip, virt,
                                                self._stream()), 'find_leaf_prod')
        return out

    def find_leaf_apply(self, bits: DevArray, tab: DevArray, rows: Sequence[DevArray], lambdas: Sequence[int], outer: int, k: int,
                        inner: int, ncomp: int, flip: int = 0, virt: int = 0, out: Optional[DevArray] = None) -> DevArray:
        """The level after the first round, (ncomp, outer, kc, inner): out[q, o, n0 + j, i] = leaf_q(first_j) + v with
        v = sum_s lambdas[s] * rows[s] over the compact (ncomp, outer, h, inner) rows, and the bye out[q, o, 0, i] = leaf_q(0)
        when kv is odd (runtime.py:4684) with the recombination of the re-shared product folded in."""
        kv, h, kc = self._find_args('find_leaf_apply', bits, outer, k, inner, ncomp, flip, virt, True)
        self._same((ncomp - 1) * 2 * kv, tab, what='find_leaf_apply table')
        nrows, ptrs, lam = self._rows(rows, lambdas, ncomp * outer * h * inner, 'find_leaf_apply row')
        out = self._out(ncomp * outer * kc * inner, out, 'find_leaf_apply output')
        _ffi.check(self._L.ffgpu_find_leaf_apply(self._h, bits.ptr, tab.ptr, ptrs, lam, nrows, out.ptr, outer, k, inner, ncomp, flip,
                                                 virt, self._stream()), 'find_leaf_apply')
        return out

    def find_prod(self, level: DevArray, outer: int, k: int, inner: int, ncomp: int, out: Optional[DevArray] = None) -> DevArray:
        """out[q, o, j, i] = level[0, o, first_j, i] * (level[q, o, second_j, i] - level[q, o, first_j, i]), compact (ncomp,
        outer, h, inner), for a stored level (ncomp, outer, k, inner), k >= 2: the local product of a later round
        (runtime.py:4683-4684).  Its apply is tour_select on (ncomp * outer, k, inner) with TOUR_ODD_EVEN."""
        _, h, _ = self._find_args('find_prod', level, outer, k, inner, ncomp, 0, 0, False)
        out = self._out(ncomp * outer * h * inner, out, 'find_prod output')
        _ffi.check(self._L.ffgpu_find_prod(self._h, level.ptr, out.ptr, outer, k, inner, ncomp, self._stream()), 'find_prod')
        return out

    # ---- fixed point: the local steps of runtime.np_trunc (runtime.py:839-873) and the gate in front of the search of
    # runtime._norm (runtime.py:4718-4727), prime fields, on raw integers a = round(x 2^f).  Bit index k least significant first ----
    def trunc_mask(self, a: DevArray, rbits: DevArray, rdivf: DevArray, f: int, offset: int, ar_out: Optional[DevArray] = None,
                   out: Optional[DevArray] = None):
        """(ar, masked): ar[h] = a[h] + sum_k rbits[h*f+k] 2^k and masked[h] = ar[h] + offset + rdivf[h] 2^f, the value
        np_trunc opens (runtime.py:860-861, 869-870).  rbits: n*f bit shares, element-major, least significant bit first; ar
        is what trunc_finish subtracts the opened low bits from."""
        n = a.n
        self._same(n, rdivf, ar_out, out, what='trunc_mask operand')      # both outputs before either is allocated
        self._same(n * f, rbits, what='trunc_mask bit shares')
        ar_out, out = self._out(n, ar_out), self._out(n, out)
        _ffi.check(self._L.ffgpu_trunc_mask(self._h, a.ptr, rbits.ptr, rdivf.ptr, self._scalars([int(offset) % self.modulus]), f,
                                            ar_out.ptr, out.ptr, n, self._stream()), 'trunc_mask')
        return ar_out, out

    def trunc_finish(self, rows: Sequence[DevArray], lambdas: Sequence[int], ar: DevArray, f: int,
                     out: Optional[DevArray] = None) -> DevArray:
        """out[h] = (ar[h] - (c[h] mod 2^f)) 2^-f with c = sum_s lambdas[s] * rows[s] taken as its canonical integer: the
        shares of the truncated values (runtime.py:871-872) with the opening of the masked shares folded in, so the opened
        value never goes to memory.  rows = [c], lambdas = [1] takes a c that is already open."""
        n = ar.n
        nrows, ptrs, lam = self._rows(rows, lambdas, n, 'trunc_finish row')
        out = self._out(n, out, 'trunc_finish output')
        _ffi.check(self._L.ffgpu_trunc_finish(self._h, ptrs, lam, nrows, ar.ptr, f, out.ptr, n, self._stream()), 'trunc_finish')
        return out

    def norm_prod(self, bits: DevArray, l: int, want_sign: bool = True, out: Optional[DevArray] = None,
                  sign_out: Optional[DevArray] = None):
        """(out, sign): out[h*(l-1)+j] = (2 x_top - 1) * bits[h*l + l-2-j], compact (n, l-1), with x_top = bits[h*l + l-1] the
        sign bit of the element-major (n, l) bits of bits_finish: the local product of (1 - 2s), s = 1 - x_top, with the bits
        below the sign bit, most significant first (runtime.py:4723-4725, the local part of :4636).  sign[h] = 1 - 2 x_top =
        2s - 1, or None with want_sign=False."""
        n = self._bit_matrix('norm_prod', bits, l, 2)
        self._same(n, sign_out, what='norm_prod sign output')
        out = self._out(n * (l - 1), out, 'norm_prod output')
        if want_sign and sign_out is None:
            sign_out = self.empty(n)
        _ffi.check(self._L.ffgpu_norm_prod(self._h, bits.ptr, l, out.ptr, sign_out.ptr if sign_out is not None else None, n,
                                           self._stream()), 'norm_prod')
        return out, sign_out

    def norm_apply(self, bits: DevArray, rows: Sequence[DevArray], lambdas: Sequence[int], l: int,
                   out: Optional[DevArray] = None) -> DevArray:
        """out[h*(l-1)+j] = 1 - x_top + v with v = sum_s lambdas[s] * rows[s] over the compact (n, l-1) rows: s + (1 - 2s) x as
        a dense (n, l-1, 1) array, which find_leaf_prod / find_leaf_apply search for its first 0 (the rest of runtime.py:4636)
        with the recombination of the re-shared product folded in."""
        n = self._bit_matrix('norm_apply', bits, l, 2)
        nrows, ptrs, lam = self._rows(rows, lambdas, n * (l - 1), 'norm_apply row')
        out = self._out(n * (l - 1), out, 'norm_apply output')
        _ffi.check(self._L.ffgpu_norm_apply(self._h, bits.ptr, ptrs, lam, nrows, l, out.ptr, n, self._stream()), 'norm_apply')
        return out

    # ---- logarithm and exponential: the local steps under runtime.np_log / np_exp2 (runtime.py:4853-4945) that the calls above
    # do not serve (include/ffgpu_math.h), prime fields.  A block of powers is power-major: row j holds y^(j+1) for the n
    # elements, rows `stride` elements apart (default n) ----
    POLY_MAX_TERMS = 64

    def _power_rows(self, what: str, P: DevArray, n: int, rows: int, stride: Optional[int]) -> int:
        stride = n if stride is None else stride
        if self.binary:
            raise NotImplementedError(f'{what}: prime fields only')
        if n < 0 or rows < 1 or stride < n:
            raise ValueError(f'{what}: at least one row of n elements, rows at least n elements apart')
        self._same(P.n, P, what=f'{what} block')
        if P.n < (rows - 1) * stride + n:
            raise ValueError(f'{what}: the block has {P.n} elements, {rows} rows of {n} need {(rows - 1) * stride + n}')
        return stride

    def powers_prod(self, P: DevArray, n: int, h: int, w: int, stride: Optional[int] = None, out: Optional[DevArray] = None) -> DevArray:
        """out[j*n + e] = P[(h-1)*stride + e] * P[j*stride + e] for j < w <= h, dense (w, n): the top power of a block of h
        powers times its w lowest -- the local products of one doubling step of np_vander's ladder (runtime.py:4966-4967).
        out may be a view of the same block from row h on."""
        if not 1 <= w <= h:
            raise ValueError('powers_prod: 1 <= w <= h')
        stride = self._power_rows('powers_prod', P, n, h, stride)
        out = self._out(w * n, out, 'powers_prod output')
        _ffi.check(self._L.ffgm_powers_prod(self._h, P.ptr, stride, h, w, out.ptr, n, self._stream()), 'powers_prod')
        return out

    def poly_table(self, coefs: Sequence[int]) -> DevArray:
        """The device table of poly_dot from 1 to 64 public integer coefficients (negative values are reduced mod p)."""
        if self.binary:
            raise ValueError('poly_table: prime fields only')
        if not 1 <= len(coefs) <= self.POLY_MAX_TERMS:
            raise ValueError(f'poly_table: 1 to {self.POLY_MAX_TERMS} coefficients')
        return self.from_ints([int(c) % self.modulus for c in coefs])

    def poly_dot(self, P: DevArray, n: int, tab: DevArray, c0: int, stride: Optional[int] = None, out: Optional[DevArray] = None) -> DevArray:
        """out[e] = c0 + sum_j tab[j] * P[j*stride + e] over the tab.n rows of the block: a polynomial without its constant
        term in the powers y^1.., plus the public constant (runtime.py:4887, 4934)."""
        if not 1 <= tab.n <= self.POLY_MAX_TERMS:
            raise ValueError(f'poly_dot: 1 to {self.POLY_MAX_TERMS} coefficients')
        self._same(tab.n, tab, what='poly_dot table')
        stride = self._power_rows('poly_dot', P, n, tab.n, stride)
        out = self._out(n, out, 'poly_dot output')
        _ffi.check(self._L.ffgm_poly_dot(self._h, P.ptr, stride, tab.n, tab.ptr, self._scalars([int(c0) % self.modulus]), out.ptr, n,
                                         self._stream()), 'poly_dot')
        return out

    def _pow_bits(self, what: str, ebits: int) -> int:
        if self.binary:
            raise NotImplementedError(f'{what}: prime fields only')
        if not 1 <= ebits <= self.modulus.bit_length():
            raise ValueError(f'{what}: 1 <= ebits <= bit length of the modulus')
        return (ebits + 3) // 4

    def pow_table(self, g: int, ebits: int) -> DevArray:
        """The fixed-base window table of pow_base for exponents below 2^ebits: g^(d * 16^i) at 15*i + d - 1, d = 1..15,
        i < ceil(ebits/4).  g: a public integer, reduced mod p (g^-1 is pow(g, -1, p))."""
        nwin, p = self._pow_bits('pow_table', ebits), self.modulus
        tab, base = [], int(g) % p
        for _ in range(nwin):
            v = 1
            for _ in range(15):
                v = v * base % p
                tab.append(v)
            base = v * base % p                         # g^(16^(i+1))
        return self.from_ints(tab)

    def pow_base(self, x: DevArray, tab: DevArray, ebits: int, shift: int = 0, out: Optional[DevArray] = None) -> DevArray:
        """out[e] = g^(x[e] >> shift) for the g of pow_table(g, ebits), x[e] as its canonical integer; the caller guarantees
        x[e] >> shift < 2^ebits (runtime.py:1408, 1421-1422)."""
        nwin = self._pow_bits('pow_base', ebits)
        if not 0 <= shift < 192:
            raise ValueError('pow_base: 0 <= shift < 192')
        self._same(15 * nwin, tab, what='pow_base table')
        out = self._out(x.n, out, 'pow_base output')
        _ffi.check(self._L.ffgm_pow_base(self._h, x.ptr, shift, ebits, tab.ptr, out.ptr, x.n, self._stream()), 'pow_base')
        return out

    def bits_reverse(self, bits: DevArray, l: int, out: Optional[DevArray] = None) -> DevArray:
        """out[h*l + j] = bits[h*l + l-1-j] over the element-major (n, l) bits of bits_finish, 1 <= l <= 64: np_flip along the
        bit axis (runtime.py:4876)."""
        if self.binary:
            raise NotImplementedError('bits_reverse: prime fields only')
        n = self._bit_matrix('bits_reverse', bits, l, 1)
        if l > 64:
            raise ValueError('bits_reverse: l <= 64')
        out = self._out(n * l, out, 'bits_reverse output')
        _ffi.check(self._L.ffgm_bits_reverse(self._h, bits.ptr, l, out.ptr, n, self._stream()), 'bits_reverse')
        return out

    # ---- the Legendre zero test over a Blum prime: the local steps of runtime._np_is_zero (runtime.py:3581-3620;
    # include/ffgpu_math.h), prime fields.  The masked copies are row-major (k, n): row i holds the i-th copy of the n
    # elements; a code is one byte per entry: 0 a non-residue, 1 a residue, 2 zero ----
    def _codes(self, what: str, code: torch.Tensor, count: int) -> torch.Tensor:
        if (not isinstance(code, torch.Tensor) or code.dtype != torch.uint8 or code.dim() != 1 or code.numel() != count
                or not code.is_contiguous() or code.device != torch.device(self.torch_device)):
            raise ValueError(f'{what}: the codes are a contiguous torch.uint8 tensor of {count} bytes on the context\'s device')
        return code

    def iszero_mask(self, a: DevArray, r: DevArray, z: DevArray, u2: DevArray, k: int, out: Optional[DevArray] = None) -> DevArray:
        """out[i*n + e] = a[e]*r[i*n + e] + (1 - 2*z[i*n + e])*u2[i*n + e] for i < k, n = a.n: the k masked copies of every
        element that are opened (runtime.py:3608); z holds shares of bits."""
        if self.binary:
            raise NotImplementedError('iszero_mask: prime fields only')
        if k < 1:
            raise ValueError('iszero_mask: k >= 1')
        self._same(a.n, a, what='iszero_mask operand')
        self._same(k * a.n, r, z, u2, what='iszero_mask operand')
        out = self._out(k * a.n, out, 'iszero_mask output')
        _ffi.check(self._L.ffgm_iszero_mask(self._h, a.ptr, r.ptr, z.ptr, u2.ptr, k, out.ptr, a.n, self._stream()), 'iszero_mask')
        return out

    def legendre_code(self, c: DevArray, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """code[j] = 2 if c[j] == 0, else 1 if c[j] is a quadratic residue, else 0: c.n bytes (finfields.py:1464-1470 and the
        test c == 0 of runtime.py:3614)."""
        if self.binary:
            raise NotImplementedError('legendre_code: prime fields only')
        if self.modulus == 2:
            raise NotImplementedError('legendre_code: odd primes only')
        self._same(c.n, c, what='legendre_code operand')
        if out is None:
            out = torch.empty(c.n, dtype=torch.uint8, device=self.torch_device)
        self._codes('legendre_code', out, c.n)
        _ffi.check(self._L.ffgm_legendre_code(self._h, c.ptr, out.data_ptr(), c.n, self._stream()), 'legendre_code')
        return out

    def iszero_finish(self, code: torch.Tensor, z: DevArray, out: Optional[DevArray] = None) -> DevArray:
        """out[j] = z[j] if code[j] == 0, 1 - z[j] if code[j] == 1, 1 if code[j] == 2 (runtime.py:3614-3615; 0 counts as a
        square)."""
        if self.binary:
            raise NotImplementedError('iszero_finish: prime fields only')
        self._same(z.n, z, what='iszero_finish operand')
        self._codes('iszero_finish', code, z.n)
        out = self._out(z.n, out, 'iszero_finish output')
        _ffi.check(self._L.ffgm_iszero_finish(self._h, code.data_ptr(), z.ptr, out.ptr, z.n, self._stream()), 'iszero_finish')
        return out

    # ---- secure random bits over a prime field: the local steps of runtime.np_random_bits (runtime.py:4243-4272;
    # include/ffgpu_math.h).  Rows are separate arrays of n entries, at most 64 of them ----
    def zero_counter(self) -> torch.Tensor:
        """A device int32 set to 0: what rbits_open adds its zeros to."""
        return torch.zeros(1, dtype=torch.int32, device=self.torch_device)

    def _counter(self, what: str, zeros: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        if zeros is not None and (not isinstance(zeros, torch.Tensor) or zeros.dtype != torch.int32 or zeros.numel() != 1
                                  or zeros.device != torch.device(self.torch_device)):
            raise ValueError(f'{what}: the counter is one torch.int32 on the context\'s device')
        return zeros

    def rbits_open(self, rs: Sequence[DevArray], zs: Sequence[DevArray], lambdas: Sequence[int], zeros: Optional[torch.Tensor] = None,
                   out: Optional[DevArray] = None) -> DevArray:
        """out[h] = sum_i lambdas[i] * (rs[i][h]^2 + zs[i][h]): the masked squares, opened (runtime.py:4251-4252); the number of
        entries with out[h] == 0 is ADDED to zeros (a device int32, zero_counter()) when one is given."""
        if self.binary:
            raise NotImplementedError('rbits_open: prime fields only')
        if len(zs) != len(rs):
            raise ValueError('rbits_open: one row of z per row of r')
        k, ptrs, lam = self._rec_args(rs, lambdas, 1)
        n = rs[0].n
        self._same(n, *zs, what='rbits_open operand')
        self._counter('rbits_open', zeros)
        out = self._out(n, out, 'rbits_open output')
        zptrs = (ctypes.c_void_p * k)(*[z.ptr for z in zs])
        _ffi.check(self._L.ffgm_rbits_open(self._h, ptrs, zptrs, lam, k, out.ptr, None if zeros is None else zeros.data_ptr(), n,
                                           self._stream()), 'rbits_open')
        return out

    def rbits_finish(self, c: DevArray, rs: Sequence[DevArray], signed: bool = False, f: int = 0,
                     outs: Optional[Sequence[DevArray]] = None) -> List[DevArray]:
        """With s = c^((3p-5)/4) (p = 3 mod 4): outs[i] = rs[i] * s * 2^f when signed, else (rs[i] * s + 1) * (p+1)/2 * 2^f; 0 in
        every row where c is 0 (runtime.py:4265-4272).  One exponentiation of the public c serves every row.  outs[i] may be
        rs[i]."""
        if self.binary:
            raise NotImplementedError('rbits_finish: prime fields only')
        if self.modulus % 4 != 3:
            raise NotImplementedError('rbits_finish: p = 3 mod 4')
        m = len(rs)
        if not m or f < 0 or f >= 192:
            raise ValueError('rbits_finish: at least one row, 0 <= f < 192')
        self._same(c.n, c, *rs, what='rbits_finish operand')
        if outs is None:
            outs = [self.empty(c.n) for _ in range(m)]
        if len(outs) != m:
            raise ValueError('rbits_finish: one output per row')
        self._same(c.n, *outs, what='rbits_finish output')
        rp = (ctypes.c_void_p * m)(*[r.ptr for r in rs])
        bp = (ctypes.c_void_p * m)(*[b.ptr for b in outs])
        _ffi.check(self._L.ffgm_rbits_finish(self._h, c.ptr, rp, bp, m, int(bool(signed)), f, c.n, self._stream()), 'rbits_finish')
        return list(outs)

    # ---- the secure binary sign by Legendre symbols: the local steps of the demo's bsgn (np_bnnmnist.py:44-156;
    # include/ffgpu_math.h), prime fields.  The arrays are row-major (w, n), 1 <= w <= 8: row i belongs to the i-th symbol ----
    def bsgn_mask(self, a: DevArray, z: DevArray, alpha: int, betas: Sequence[int], out: Optional[DevArray] = None) -> DevArray:
        """out[i*n + e] = z[i*n + e] * (alpha*a[e] + betas[i]) for i < w = len(betas), n = a.n: the masked values that are
        opened (np_bnnmnist.py:72, :106-110, :147-150)."""
        if self.binary:
            raise NotImplementedError('bsgn_mask: prime fields only')
        w = len(betas)
        if not 1 <= w <= 8:
            raise ValueError('bsgn_mask: 1 to 8 rows')
        p = self.modulus
        self._same(a.n, a, what='bsgn_mask operand')
        self._same(w * a.n, z, what='bsgn_mask operand')
        out = self._out(w * a.n, out, 'bsgn_mask output')
        _ffi.check(self._L.ffgm_bsgn_mask(self._h, a.ptr, z.ptr, self._scalars([int(alpha) % p]), self._scalars([int(b) % p for b in betas]),
                                          w, out.ptr, a.n, self._stream()), 'bsgn_mask')
        return out

    def bsgn_finish(self, c: DevArray, ss: Sequence[DevArray], w: int, sum: bool = False,
                    outs: Optional[Sequence[DevArray]] = None) -> List[DevArray]:
        """With h = (c | p), the Legendre symbols (1, -1 or 0) of the public (w, n) array c: outs[q] = h * ss[q] entry by
        entry, or, with sum, outs[q][e] = sum_i h[i*n + e] * ss[q][i*n + e] (np_bnnmnist.py:74, :113-114, :154).  One
        exponentiation of each public value serves every party."""
        if self.binary:
            raise NotImplementedError('bsgn_finish: prime fields only')
        if self.modulus == 2:
            raise NotImplementedError('bsgn_finish: odd primes only')
        m = len(ss)
        if not m or not 1 <= w <= 8 or c.n % w:
            raise ValueError('bsgn_finish: at least one party, 1 to 8 rows, a (w, n) array')
        n = c.n // w
        self._same(c.n, c, *ss, what='bsgn_finish operand')
        on = n if sum else c.n
        if outs is None:
            outs = [self.empty(on) for _ in range(m)]
        if len(outs) != m:
            raise ValueError('bsgn_finish: one output per party')
        self._same(on, *outs, what='bsgn_finish output')
        sp = (ctypes.c_void_p * m)(*[s.ptr for s in ss])
        op = (ctypes.c_void_p * m)(*[o.ptr for o in outs])
        _ffi.check(self._L.ffgm_bsgn_finish(self._h, c.ptr, sp, op, m, w, int(bool(sum)), n, self._stream()), 'bsgn_finish')
        return list(outs)

    # ---- secure unit vectors and table lookup at secret indices: the local steps under runtime.np_unit_vector / unit_vector
    # (runtime.py:4979-5029; include/ffgpu_math.h), prime fields.  Unit vectors are position-major (rows, n): row j holds
    # position j for the n indices; K2 = 2^kbits ----
    UNIT_MAX_KBITS = 30

    def unit_dot_max_kbits(self) -> int:
        """the largest kbits whose 2^kbits-entry table unit_dot holds in LDS: 14, 13, 12, 12, 11 for 4, 8, 12, 16, 24 bytes --
        unit_dot_max_kbits of csrc/unitvec_geom.hpp restated (tests/test_unitvec_host.py holds the two together, and the GPU
        tests run the library at this value and are refused one above it)"""
        word = {4: 4, 8: 8, 24: 24}.get(self.elem_bytes, 16)
        return (65536 // word).bit_length() - 1

    def unit_iota(self, count: int) -> DevArray:
        """The table 0, 1, .., count - 1 on the device, uploaded once per context and count and kept: unit_dot on it without a
        rotation gives the positions u @ arange(count) (runtime.py:5016), and a second call allocates and copies nothing.
        Never written by the library (a table is an input); the caller must not write it either."""
        cache = self.__dict__.setdefault('_unit_iota', {})
        if count not in cache:
            if not 1 <= count <= self.modulus:
                raise ValueError('unit_iota: 1 <= count <= p')
            cache[count] = self.from_ints(list(range(count)))
        return cache[count]

    def _unit_rows(self, what: str, U: DevArray, rows: int) -> int:
        """n of the position-major (rows, n) array U"""
        if self.binary:
            raise NotImplementedError(f'{what}: prime fields only')
        if rows < 1 or U.n % rows:
            raise ValueError(f'{what}: the operand is not a (rows, n) array of {rows} rows')
        self._same(U.n, U, what=f'{what} operand')
        return U.n // rows

    def unit_prod(self, x: DevArray, U: DevArray, h: int, xstride: int = 1, xoffset: int = 0, out: Optional[DevArray] = None) -> DevArray:
        """out[j*n + e] = x[xoffset + e*xstride] * U[j*n + e] for j < h, n = U.n / h: one bit of every index times the h rows
        of a demultiplexer round (random.py:141-151, runtime.py:4993-4996).  xstride = 1: a row of n bits starting at xoffset;
        xstride = l, xoffset = i: bit i of the element-major (n, l) bits of bits_finish."""
        n = self._unit_rows('unit_prod', U, h)
        if xstride < 1 or xoffset < 0 or (n and xoffset + (n - 1) * xstride >= x.n):
            raise ValueError('unit_prod: the factors x[xoffset + e*xstride], e < n, lie inside x')
        self._same(x.n, x, what='unit_prod factor')
        out = self._out(h * n, out, 'unit_prod output')
        _ffi.check(self._L.ffgm_unit_prod(self._h, x.ptr + xoffset * self.elem_bytes, xstride, U.ptr, h, out.ptr, n, self._stream()),
                   'unit_prod')
        return out

    def unit_roll(self, U: DevArray, c: DevArray, kbits: int, K: int, out: Optional[DevArray] = None) -> DevArray:
        """out[j*n + e] = U[((j - c[e]) mod 2^kbits)*n + e] for j < K <= 2^kbits: the (2^kbits, n) unit vectors rotated by the
        public canonical c (its low kbits bits), the first K rows kept (runtime.py:5026-5028)."""
        if not 0 <= kbits <= self.UNIT_MAX_KBITS or not 1 <= K <= 1 << kbits:
            raise ValueError('unit_roll: 0 <= kbits <= 30 and 1 <= K <= 2^kbits')
        n = self._unit_rows('unit_roll', U, 1 << kbits)
        self._same(n, c, what='unit_roll offsets')
        out = self._out(K * n, out, 'unit_roll output')
        _ffi.check(self._L.ffgm_unit_roll(self._h, U.ptr, c.ptr, kbits, K, out.ptr, n, self._stream()), 'unit_roll')
        return out

    def unit_dot(self, U: DevArray, tab: DevArray, rows: int, c: Optional[DevArray] = None, kbits: int = 0,
                 out: Optional[DevArray] = None) -> DevArray:
        """out[e] = sum_{j<rows} tab[(j + c[e]) mod 2^kbits] * U[j*n + e], tab zero from tab.n up: a table read through unit
        vectors that are never rotated (runtime.py:5016 and `T @ np_unit_vector(a, n)`).  With c: rows == 2^kbits and
        1 <= tab.n <= rows.  Without c: tab[j], any rows, tab.n == rows.  The table lives in LDS: NotImplementedError beyond
        unit_dot_max_kbits()."""
        n = self._unit_rows('unit_dot', U, rows)
        if c is not None:
            if not 0 <= kbits <= self.UNIT_MAX_KBITS or rows != 1 << kbits or not 1 <= tab.n <= rows:
                raise ValueError('unit_dot: with offsets, rows == 2^kbits and a table of 1 to rows entries')
            self._same(n, c, what='unit_dot offsets')
        elif tab.n != rows:
            raise ValueError('unit_dot: without offsets, a table of `rows` entries')
        self._same(tab.n, tab, what='unit_dot table')
        out = self._out(n, out, 'unit_dot output')
        _ffi.check(self._L.ffgm_unit_dot(self._h, U.ptr, rows, None if c is None else c.ptr, kbits, tab.ptr, tab.n, out.ptr, n,
                                         self._stream()), 'unit_dot')
        return out

    # ---- secure 2-D convolution layers: the local correlation of the demo's convolvetensor (np_cnnmnist.py:69-80;
    # include/ffgpu_math.h), prime fields.  Dense row-major tensors: x (k, r, m, n), W (v, r, s, s), b (v), out (k, v, m, n) ----
    CONV2D_MAX_S = 16
    CONV2D_MAX_SENDERS = 64

    def _conv2d_counts(self, what: str, k: int, r: int, m: int, n: int, v: int, s: int, nsend: int):
        if self.binary:
            raise NotImplementedError(f'{what}: prime fields only')
        if nsend > self.CONV2D_MAX_SENDERS:
            raise NotImplementedError(f'{what}: at most 64 senders')
        if nsend < 1 or min(k, r, m, n, v) < 0 or not 1 <= s <= self.CONV2D_MAX_S:
            raise ValueError(f'{what}: at least one sender, counts >= 0 and 1 <= s <= 16')
        if k * v * m * n and (s > n or r < 1):
            raise ValueError(f'{what}: s <= n and at least one input channel')
        if not k * v * m * n and n and s > n:
            raise ValueError(f'{what}: s <= n')

    def conv2d_plan(self, k: int, r: int, m: int, n: int, v: int, s: int, nsend: int = 1) -> Conv2dPlan:
        """The shape conv2d takes for these sizes on this context (ffgm_conv2d_plan): host-only, launches nothing."""
        self._conv2d_counts('conv2d_plan', k, r, m, n, v, s, nsend)
        pl = _ffi.Conv2dPlanStruct()
        _ffi.check(self._L.ffgm_conv2d_plan(self._h, k, r, m, n, v, s, nsend, ctypes.byref(pl)), 'conv2d_plan')
        return Conv2dPlan(pl.tile_rows, pl.tile_cols, pl.out_channels, pl.in_channels_step, pl.flush_rows, bool(pl.wide),
                          (int(pl.grid_x), int(pl.grid_y)), int(pl.lds_bytes))

    def conv2d(self, xs: Sequence[DevArray], ws: Sequence[DevArray], bs: Optional[Sequence[DevArray]], k: int, r: int, m: int,
               n: int, v: int, s: int, outs: Optional[Sequence[DevArray]] = None) -> List[DevArray]:
        """outs[q][i, j, I, J] = bs[q][j] + sum_{l, di, dj} xs[q][i, l, I + di - (s-1)//2, J + dj - s//2] * ws[q][j, l, di, dj]
        for every sender q in ONE launch, x outside the image counting as 0 (np_cnnmnist.py:69-80).  bs None: no bias.  The
        operands may be the same arrays for several senders (public weights); no output may overlap an operand."""
        nsend = len(xs)
        self._conv2d_counts('conv2d', k, r, m, n, v, s, nsend)
        if len(ws) != nsend or (bs is not None and len(bs) != nsend):
            raise ValueError('conv2d: one x, one W and one b per sender')
        self._same(k * r * m * n, *xs, what='conv2d image tensor')
        self._same(v * r * s * s, *ws, what='conv2d filter tensor')
        if bs is not None:
            self._same(v, *bs, what='conv2d bias')
        on = k * v * m * n
        if outs is None:
            outs = [self.empty(on) for _ in range(nsend)]
        if len(outs) != nsend:
            raise ValueError('conv2d: one output per sender')
        self._same(on, *outs, what='conv2d output')
        ptrs = lambda arrs: (ctypes.c_void_p * nsend)(*[a.ptr for a in arrs])
        _ffi.check(self._L.ffgm_conv2d(self._h, ptrs(xs), ptrs(ws), None if bs is None else ptrs(bs), ptrs(outs), nsend, k, r, m, n, v, s,
                                       self._stream()), 'conv2d')
        return list(outs)

    def sqrt_cl(self, a: DevArray, out: Optional[DevArray] = None) -> DevArray:
        """Square roots for p = 1 mod 4 (Cipolla-Lehmer, finfields.py:447-470)."""
        out = self._out(a.n, out)
        _ffi.check(self._L.ffgpu_sqrt_cl(self._h, a.ptr, out.ptr, a.n, self._stream()), 'sqrt_cl')
        return out

    def gauss(self, a: DevArray, n: int, ncols: int, batch: int = 1, det: bool = False):
        """Gaussian elimination in place on `batch` row-major (n, ncols) matrices (finfields.py:872-955).
        det=False: (A | B) -> (. | A^-1 B).  det=True: returns the reference's determinant per matrix.
        Returns (det DevArray or None, singular flags as an int32 tensor on the device)."""
        if a.n != batch * n * ncols:
            raise ValueError('array size does not match (batch, n, ncols)')
        sing = torch.empty(max(batch, 1), dtype=torch.int32, device=self.torch_device)
        d = self.empty(batch) if det else None
        _ffi.check(self._L.ffgpu_gauss(self._h, a.ptr, n, ncols, batch, 1 if det else 0, d.ptr if det else None,
                                       sing.data_ptr(), self._stream()), 'gauss')
        return d, sing

    def group_matvec(self, x: DevArray, matrix: Sequence[Sequence[int]], bias: Optional[Sequence[int]] = None,
                     out: Optional[DevArray] = None) -> DevArray:
        """out[i*r+a] = bias[a] + sum_c matrix[a][c] * x[i*g+c] over groups of g = len(matrix[0]) consecutive
        elements (public r x g matrix; np_aes affine layer, np_from_bits)."""
        r, g = len(matrix), len(matrix[0])
        if x.n % g:
            raise ValueError('array length is not a multiple of the group size')
        ng = x.n // g
        out = self._out(ng * r, out)
        m = self._scalars([v for row in matrix for v in row])
        b = self._scalars(bias) if bias is not None else None
        _ffi.check(self._L.ffgpu_group_matvec(self._h, m, b, r, g, x.ptr, out.ptr, ng, self._stream()), 'group_matvec')
        return out

    def _workspace(self):
        """partial-sum workspace of dot / sum: one per stream (launches on different streams must not share it)"""
        wss = self.__dict__.setdefault('_ws', {})
        key = self._stream()
        ws = wss.get(key)
        if ws is None:
            ws = wss[key] = torch.empty(1024 * 16, dtype=torch.uint8, device=self.torch_device)
        return ws

    def dot(self, a: DevArray, b: DevArray) -> DevArray:
        """sum_i a[i]*b[i] as a 1-element device array (local part of runtime.in_prod)."""
        if a.n != b.n:
            raise ValueError('length mismatch')
        out = self.empty(1)
        _ffi.check(self._L.ffgpu_dot(self._h, a.ptr, b.ptr, out.ptr, self._workspace().data_ptr(), a.n,
                                     self._stream()), 'dot')
        return out

    def sum(self, a: DevArray) -> DevArray:
        out = self.empty(1)
        _ffi.check(self._L.ffgpu_sum(self._h, a.ptr, out.ptr, self._workspace().data_ptr(), a.n, self._stream()), 'sum')
        return out

    def _stage(self, nbytes: int) -> torch.Tensor:
        """grow-only pinned host staging buffer of this context (uint8)"""
        stages = self.__dict__.setdefault('_pinned_stage', {})
        key = self._stream()                              # one staging buffer per stream
        stage = stages.get(key)
        if stage is None or stage.numel() < nbytes:
            stage = stages[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        return stage

    def download_bytes(self, t: torch.Tensor) -> np.ndarray:
        """Device tensor -> uint8 numpy VIEW of the pinned staging buffer (valid until the next staged
        transfer): a pinned copy runs at PCIe speed, a pageable one at a third of it."""
        flat = t.contiguous().view(torch.uint8).reshape(-1)
        stage = self._stage(flat.numel())
        stage[:flat.numel()].copy_(flat, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return stage[:flat.numel()].numpy()

    def upload_bytes(self, data, dtype: torch.dtype, shape) -> torch.Tensor:
        """Host bytes (any buffer: a message off the wire) -> device tensor of `dtype` / `shape`: ONE host copy into
        the pinned staging buffer, then an asynchronous copy at PCIe speed (a pageable source costs an extra pass
        and transfers at a fraction of that rate)."""
        src = np.frombuffer(data, dtype=np.uint8)
        nbytes = src.size
        stage = self._stage(nbytes)
        stage[:nbytes].numpy()[:] = src
        dev = torch.empty(nbytes, dtype=torch.uint8, device=self.torch_device)
        dev.copy_(stage[:nbytes], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()        # the staging buffer is reused by the next transfer
        return dev.view(dtype).reshape(shape)

    def shake128_streams(self, msgs: Sequence[bytes], out_len: int, threads: int = 0) -> List[torch.Tensor]:
        """SHAKE128(msg).digest(out_len) for every msg, expanded in parallel on host threads into pinned
        buffers (libffgpu's ffgpu_shake128_expand) and uploaded: the XOF streams of a PRSS call
        (thresha.py:255, one per subset key).  Returns uint8 device tensors."""
        msgs = [bytes(mg) for mg in msgs]
        k = len(msgs)
        if k == 0 or out_len == 0:
            return [torch.empty(0, dtype=torch.uint8, device=self.torch_device) for _ in msgs]
        # one grow-only pinned staging buffer per context (allocating pinned memory per call costs more than
        # the expansion itself), rows padded to 256 bytes
        pitch = (out_len + 255) // 256 * 256
        need = k * pitch
        stage = self._stage(need)
        keep = [ctypes.create_string_buffer(mg, max(len(mg), 1)) for mg in msgs]
        mp = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in keep])
        ml = (ctypes.c_size_t * k)(*[len(mg) for mg in msgs])
        op = (ctypes.c_void_p * k)(*[stage.data_ptr() + j * pitch for j in range(k)])
        _ffi.check(self._L.ffgpu_shake128_expand(mp, ml, k, out_len, op, threads), 'shake128_expand')
        dev = stage[:need].to(self.torch_device, non_blocking=True)
        torch.cuda.current_stream().synchronize()          # the staging buffer is reused by the next call
        devs = [dev[j * pitch:j * pitch + out_len] for j in range(k)]
        return devs

    PRSS_SLICE_BYTES = 8 << 20        # per stream and slice: 10 ms of one host thread, 160 MB per half for 20 keys

    def prss_streamed(self, msgs: Sequence[bytes], d: int, l: int, weights: Sequence[int], n: int, mask_bits: int,
                      out: DevArray, accumulate: bool, slice_bytes: int = 0, threads: int = 0) -> DevArray:
        """The PRSS combination of `prss_combine` with the XOF streams SHAKE128(msg) produced on the fly
        (ffgpu_shake128_open / _squeeze): every stream is squeezed a slice (~slice_bytes) at a time on host threads into
        one half of a pinned staging buffer; the slice is uploaded and combined into its range of `out` on the device
        while the host squeezes the next slice into the other half.  Pinned memory: 2 * len(msgs) * slice_bytes."""
        msgs = [bytes(mg) for mg in msgs]
        k = len(msgs)
        slice_bytes = slice_bytes or self.PRSS_SLICE_BYTES
        per = d * l                                                  # XOF bytes per output element and stream
        step = max(256, slice_bytes // per // 256 * 256)             # elements per slice (aligned ranges of `out`)
        pitch = (step * per + 255) // 256 * 256
        stage = self._stage(2 * k * pitch)
        keep = [ctypes.create_string_buffer(mg, max(len(mg), 1)) for mg in msgs]
        mp = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in keep])
        ml = (ctypes.c_size_t * k)(*[len(mg) for mg in msgs])
        handle = ctypes.c_void_p()
        _ffi.check(self._L.ffgpu_shake128_open(mp, ml, k, ctypes.byref(handle)), 'shake128_open')
        free = [None, None]                                          # event: the half has been uploaded
        try:
            for c, h0 in enumerate(range(0, n, step)):
                cnt = min(step, n - h0)
                half = c & 1
                base = stage.data_ptr() + half * k * pitch
                if free[half] is not None:
                    free[half].synchronize()
                op = (ctypes.c_void_p * k)(*[base + j * pitch for j in range(k)])
                _ffi.check(self._L.ffgpu_shake128_squeeze(handle, op, cnt * per, threads), 'shake128_squeeze')
                dev = torch.empty(k * pitch, dtype=torch.uint8, device=self.torch_device)
                dev.copy_(stage[half * k * pitch:(half + 1) * k * pitch], non_blocking=True)
                free[half] = torch.cuda.Event()
                free[half].record()
                self.prss_combine([dev[j * pitch:j * pitch + cnt * per] for j in range(k)], d, l, weights, cnt,
                                  mask_bits=mask_bits, out=DevArray(self, out.t[h0:h0 + cnt], cnt), accumulate=accumulate)
        finally:
            self._L.ffgpu_shake128_close(handle)
            for ev in free:
                if ev is not None:
                    ev.synchronize()                                 # the staging buffer is reused by the next call
        return out

    def prss_combine(self, streams: Sequence, d: int, l: int, weights: Sequence[int], n: int,
                     mask_bits: int = 0, out: Optional[DevArray] = None, accumulate: bool = False) -> DevArray:
        """out[h] (+)= sum_s sum_j draw_s[h*d+j] * weights[s*d+j]; streams are the raw XOF outputs, n*d*l
        bytes each: host bytes (uploaded as they are) or uint8 device tensors from shake128_streams
        (thresha.py:163-173, 201-217)."""
        ks = len(streams)
        if len(weights) != ks * d:
            raise ValueError('need ks*d weights')
        out = self._out(n, out)
        devs = []
        for sbytes in streams:
            if isinstance(sbytes, torch.Tensor):
                if sbytes.numel() < n * d * l:
                    raise ValueError('XOF stream too short')
                devs.append(sbytes)
                continue
            if len(sbytes) < n * d * l:
                raise ValueError('XOF stream too short')
            a = np.frombuffer(sbytes, dtype=np.uint8, count=n * d * l)
            devs.append(torch.from_numpy(a.copy()).to(self.torch_device))
        ptrs = (ctypes.c_void_p * ks)(*[t.data_ptr() for t in devs])
        w = self._scalars(weights)
        _ffi.check(self._L.ffgpu_prss_combine(self._h, ptrs, ks, d, l, mask_bits, w, int(accumulate), out.ptr, n,
                                              self._stream()), 'prss_combine')
        return out

    def prss_chacha(self, keys40: Sequence[bytes], d: int, l: int, weights: Sequence[int], n: int, mask_bits: int = 0,
                    rounds: int = 20, out: Optional[DevArray] = None, accumulate: bool = False) -> DevArray:
        """The same combination with the draws expanded ON THE DEVICE from one ChaCha stream per subset key (production
        mode, ffgpu_prss_chacha): keys40[s] = 32-byte key + 8-byte nonce of stream s; a draw = l keystream bytes reduced
        by the reference's rule (thresha.py:234-266).  At most 32 streams and 64 weights per call."""
        ks = len(keys40)
        if len(weights) != ks * d or any(len(k_) != 40 for k_ in keys40):
            raise ValueError('need ks 40-byte stream keys and ks*d weights')
        out = self._out(n, out)
        w = self._scalars(weights)
        kb = ctypes.create_string_buffer(b''.join(bytes(k_) for k_ in keys40), 40 * ks)
        _ffi.check(self._L.ffgpu_prss_chacha(self._h, ctypes.cast(kb, ctypes.POINTER(ctypes.c_uint8)), ks, d, l, mask_bits,
                                             rounds, w, int(accumulate), out.ptr, n, self._stream()), 'prss_chacha')
        return out

    def bit_affine(self, bits: DevArray, matrix: Sequence[Sequence[int]], bias: Optional[Sequence[int]] = None,
                   from_bits: bool = False, out: Optional[DevArray] = None) -> DevArray:
        """GF(2^n<=8): y = M bits + bias per group of 8 bit shares (np_aes.py:40-41); from_bits: also
        recompose sum_r 2^r y_r in the same pass (np_aes.py:42)."""
        if bits.n % 8:
            raise ValueError('bit array length must be a multiple of 8')
        ng = bits.n // 8
        out = self._out(ng if from_bits else bits.n, out)
        m = (ctypes.c_uint64 * 128)()
        for i, v in enumerate(v for row in matrix for v in row):
            m[2 * i] = int(v)
        b = None
        if bias is not None:
            b = (ctypes.c_uint64 * 16)()
            for i, v in enumerate(bias):
                b[2 * i] = int(v)
        _ffi.check(self._L.ffgpu_gf256_bit_affine(self._h, m, b, 1 if from_bits else 0, bits.ptr, out.ptr, ng,
                                                  self._stream()), 'bit_affine')
        return out

    def _scalars(self, vals: Sequence[int]):
        """Host scalars in the C ABI's layout: scalar_limbs little-endian 64-bit limbs each (ffgpu_ctx_scalar_limbs)."""
        sl = self.scalar_limbs
        w = (ctypes.c_uint64 * (sl * max(1, len(vals))))()
        for i, v in enumerate(vals):
            v = int(v)
            for q in range(sl):
                w[sl * i + q] = (v >> (64 * q)) & _MASK64
        return w

    def gf256_mask_open(self, rows: Sequence[DevArray], coefs: Sequence[int], rbits: Sequence[DevArray],
                        mus: Sequence[int], out: Optional[DevArray] = None) -> DevArray:
        """GF(2^8): c = sum_r coefs[r] * rows[r] + sum_p mus[p] * from_bits(rbits[p]) -- the opened masked value of
        np_to_bits (runtime.py:4414-4421) in one pass (ffgpu_gf256_mask_open)."""
        if len(rows) != len(coefs) or len(rbits) != len(mus) or not (rows or rbits):
            raise ValueError('one coefficient per row')
        n = rows[0].n if rows else rbits[0].n // 8
        self._same(n, *rows, what='share row')
        self._same(8 * n, *rbits, what='bit-share row')
        out = self._out(n, out)
        pr = (ctypes.c_void_p * max(1, len(rows)))(*[r.ptr for r in rows])
        pb = (ctypes.c_void_p * max(1, len(rbits)))(*[r.ptr for r in rbits])
        _ffi.check(self._L.ffgpu_gf256_mask_open(self._h, pr, self._scalars(coefs), len(rows), pb, self._scalars(mus),
                                                 len(rbits), out.ptr, n, self._stream()), 'gf256_mask_open')
        return out

    def gf256_bits_affine_fold(self, c: DevArray, rbits: DevMatrix, matrix: Sequence[Sequence[int]],
                               bias: Optional[Sequence[int]] = None, out: Optional[DevMatrix] = None) -> DevMatrix:
        """GF(2^8), all parties in one launch: out[y] = from_bits(M (bits(c) + rbits[y]) + bias) for every row y of
        the (parties, 8n) matrix of bit shares (runtime.py:4422-4423 + np_aes.py:40-42; ffgpu_gf256_bits_affine_fold)."""
        n = c.n
        if rbits.n != 8 * n:
            raise ValueError('need 8 bit shares per byte')
        out = self._out_matrix(out, rbits.rows, n)
        mm = self._scalars([v for row in matrix for v in row])
        bb = self._scalars(bias) if bias is not None else None
        _ffi.check(self._L.ffgpu_gf256_bits_affine_fold(self._h, mm, bb, c.ptr, rbits.ptr, rbits.stride, out.ptr, out.stride,
                                                        n, rbits.rows, self._stream()), 'gf256_bits_affine_fold')
        return out

    def gf256_sbox_layer(self, X: DevMatrix, R: DevMatrix, t: int, lam: Sequence[int], mu: Sequence[int],
                         matrix: Sequence[Sequence[int]], bias: Optional[Sequence[int]] = None, key: Optional[bytes] = None,
                         nonce: int = 0, rounds: int = 20, state: Optional['RngState'] = None,
                         out: Optional[DevMatrix] = None) -> DevMatrix:
        """The whole secure S-box layer of np_aes.py:37-43 for all parties in ONE launch (ffgpu_gf256_sbox_layer): X
        = the parties' shares (one row each), R = their shares of 8 random bits per byte.  Raises
        NotImplementedError for shapes the fused kernel does not cover (the caller composes the layer from the
        per-step kernels then)."""
        import secrets as _secrets
        m, n = X.rows, X.n
        if R.rows != m or R.n != 8 * n:
            raise ValueError('need 8 bit shares per byte and party')
        out = self._out_matrix(out, m, n)
        mm = self._scalars([v for row in matrix for v in row])
        bb = self._scalars(bias) if bias is not None else None
        if state is None and key is None:
            key = _secrets.token_bytes(32)
        defer = 0
        if state is not None:
            if state.pending:
                nonce, defer = state.take_offset(), 1          # inside a sequence of deferred launches: commit() follows
            else:
                nonce = 0          # the layer is ONE launch: it advances the device nonce itself (the last workgroup of the
                #                    kernel for grids of up to RNG_RELEASE_MAX_GRID = 512 workgroups -- up to ~5.2 * 10^5 bytes;
                #                    10^6 bytes are 977 workgroups --, a one-thread kernel, k_rng_advance, above that)
        _ffi.check(self._L.ffgpu_gf256_sbox_layer(self._h, mm, bb, self._scalars(lam), self._scalars(mu), t, m, X.ptr, X.stride,
                                                  R.ptr, R.stride, out.ptr, out.stride, n, key, nonce, rounds,
                                                  state.ptr if state is not None else None, defer, self._stream()),
                   'gf256_sbox_layer')
        return out

    # ---- threshold SHA-3: secure Keccak-f[1600] rounds over GF(2^n <= 8) (ffgpu_math.h; csrc/keccak.hpp) -------------------
    KECCAK_STATE = 1600

    def _keccak_rows(self, rows: Sequence[DevArray], lam: Sequence[int], nstates: int):
        if nstates < 1:
            raise ValueError('keccak: at least one state')
        return self._rows(rows, lam, self.KECCAK_STATE * nstates, 'keccak share row')

    def keccak_local(self, rows: Sequence[DevArray], lam: Sequence[int], nstates: int, iota_round: int = -1,
                     apply_round: bool = True, nbatch: int = 1, stride_in: int = 0, out: Optional[DevMatrix] = None) -> DevMatrix:
        """One Keccak-f[1600] round on shares, without the re-sharing (ffgm_gf2_keccak_local): a = sum lam[s] * rows[s]
        (shares of `nstates` states, 1600 bytes each, state-major), plus iota of round `iota_round` (-1: none), then
        theta, rho, pi and chi's local product -- or, with apply_round=False, only the recombined state plus iota.  For
        `nbatch` senders in one launch, sender y reads every row y * stride_in bytes further on and writes row y of
        `out` (the caller owns that layout, as for gate_batch).  Raises NotImplementedError where the kernels do not
        apply (not GF(2^n <= 8), more than 7 rows, unaligned rows, iota_round outside -1..23)."""
        k, ptrs, la = self._keccak_rows(rows, lam, nstates)
        out = self._out_matrix(out, nbatch, self.KECCAK_STATE * nstates)
        _ffi.check(self._L.ffgm_gf2_keccak_local(self._h, ptrs, la, k, stride_in, nbatch, iota_round, 1 if apply_round else 0,
                                                  out.ptr, out.stride, nstates, self._stream()), 'gf2_keccak_local')
        return out

    def keccak_round(self, rows: Sequence[DevArray], lam: Sequence[int], nstates: int, t: int, m: int, iota_round: int = -1,
                     stride_in: int = 0, out: Optional[DevMatrix] = None, key: Optional[bytes] = None, nonce: int = 0,
                     rounds: int = 20, state: Optional['RngState'] = None) -> DevMatrix:
        """keccak_local(apply_round=True) for the senders 1..2t+1 followed by the share generation of the re-sharing round
        (ffgm_gf2_keccak_round): `out` is the [recipient][sender] block of gate_batch, m * (2t+1) rows -- row
        j * (2t+1) + y = what sender y+1 deals to party j+1.  With `state` the launch is one of a sequence of deferred
        launches: state.commit() follows.  (m, t) = (1, 0): one row, the round's output."""
        import secrets as _secrets
        k, ptrs, la = self._keccak_rows(rows, lam, nstates)
        senders = 2 * t + 1
        out = self._out_matrix(out, m * senders, self.KECCAK_STATE * nstates)
        if state is None and key is None:
            key = _secrets.token_bytes(32)
        defer = 0
        if state is not None:
            nonce, defer = state.take_offset(), 1
        _ffi.check(self._L.ffgm_gf2_keccak_round(self._h, ptrs, la, k, stride_in, iota_round, key, nonce, rounds,
                                                  state.ptr if state is not None else None, defer, t, m, out.ptr,
                                                  out.stride * senders, out.stride, nstates, self._stream()), 'gf2_keccak_round')
        return out

    def to_bits(self, x: DevArray, addend: Optional[DevArray] = None, out: Optional[DevArray] = None) -> DevArray:
        """GF(2^n<=8): bits of PUBLIC bytes as field elements (8 per byte), plus `addend` (runtime.py:4418-4423)."""
        out = self._out(8 * x.n, out)
        _ffi.check(self._L.ffgpu_gf256_to_bits(self._h, x.ptr, addend.ptr if addend is not None else None, out.ptr,
                                               x.n, self._stream()), 'to_bits')
        return out

    def sbox(self, x: DevArray, rows8: Sequence[int], b: int, out=None):
        out = self._out(x.n, out)
        r = (ctypes.c_uint8 * 8)(*rows8)
        _ffi.check(self._L.ffgpu_gf256_sbox(self._h, x.ptr, r, ctypes.c_uint8(b), out.ptr, x.n, self._stream()),
                   'sbox')
        return out

    def set_timing(self, enable: bool = True, accumulate: bool = False):
        """Record GPU events around every compute call (off by default).  accumulate: keep one event pair per call
        so that busy_ms() can return the summed GPU time of all calls (ffgpu_busy_ms)."""
        _ffi.check(self._L.ffgpu_ctx_set_timing(self._h, (2 if accumulate else 1) if enable else 0), 'set_timing')

    def busy_ms(self, reset: bool = True):
        """(summed GPU ms, number of compute calls) since the last reset; waits for the calls issued so far.  Needs
        set_timing(True, accumulate=True)."""
        ms, calls = ctypes.c_double(), ctypes.c_ulonglong()
        _ffi.check(self._L.ffgpu_busy_ms(self._h, ctypes.byref(ms), ctypes.byref(calls), int(reset)), 'busy_ms')
        return float(ms.value), int(calls.value)

    def last_kernel_ms(self) -> float:
        """GPU time of the most recent compute call (waits for it); needs set_timing(True)."""
        ms = ctypes.c_float()
        _ffi.check(self._L.ffgpu_last_kernel_ms(self._h, ctypes.byref(ms)), 'last_kernel_ms')
        return float(ms.value)

    def sync(self):
        _ffi.check(self._L.ffgpu_stream_sync(self._h, self._stream()), 'sync')

    # ---- timing (HIP events on the launch stream, inside the library) --------
    def time_mul(self, a, b, out, reps: int) -> float:
        ms = ctypes.c_float()
        _ffi.check(self._L.ffgpu_time_mul(self._h, a.ptr, b.ptr, out.ptr, a.n, reps, self._stream(),
                                          ctypes.byref(ms)), 'time_mul')
        return ms.value

    def time_split(self, secrets, coeffs, t, m, out, reps: int) -> float:
        ms = ctypes.c_float()
        _ffi.check(self._L.ffgpu_time_split(self._h, secrets.ptr, coeffs.ptr if t else None,
                                            coeffs.stride if t else 0, t, m, out.ptr, out.stride, secrets.n,
                                            reps, self._stream(), ctypes.byref(ms)), 'time_split')
        return ms.value

    def time_recombine(self, rows, lambdas, out, reps: int, w: int = 1) -> float:
        k, ptrs, lam = self._rec_args(rows, lambdas, w)
        ms = ctypes.c_float()
        stride = rows[0].n if w == 1 else out.stride
        _ffi.check(self._L.ffgpu_time_recombine(self._h, ptrs, lam, k, w, out.ptr, stride, rows[0].n, reps,
                                                self._stream(), ctypes.byref(ms)), 'time_recombine')
        return ms.value

    def copy(self, src: torch.Tensor, dst: torch.Tensor):
        """Streaming device copy with the library's own kernel (bandwidth yardstick)."""
        nbytes = src.numel() * src.element_size()
        _ffi.check(self._L.ffgpu_copy(self._h, src.data_ptr(), dst.data_ptr(), nbytes, self._stream()), 'copy')

    def valu_probe(self, op: int = 0, iters: int = 2000, waves_per_simd: int = 4):
        """(lane-operations per second, shader clock in MHz, shader cycles per wave instruction and SIMD) the integer VALU
        sustains right now for one instruction kind (0: v_bitop3_b32, 1: v_add_u32, 2: v_mad_u64_u32): the compute-side
        yardstick beside `copy` (ffgpu_valu_probe)."""
        scratch = torch.zeros(4, dtype=torch.int64, device=self.torch_device)
        out = (ctypes.c_double * 3)()
        _ffi.check(self._L.ffgpu_valu_probe(self._h, op, iters, waves_per_simd, scratch.data_ptr(), out, self._stream()), 'valu_probe')
        return float(out[0]), float(out[1]), float(out[2])

    def time_copy(self, src: torch.Tensor, dst: torch.Tensor, reps: int) -> float:
        ms = ctypes.c_float()
        nbytes = src.numel() * src.element_size()
        _ffi.check(self._L.ffgpu_time_copy(self._h, src.data_ptr(), dst.data_ptr(), nbytes, reps,
                                           self._stream(), ctypes.byref(ms)), 'time_copy')
        return ms.value
