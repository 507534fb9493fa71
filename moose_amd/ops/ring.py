"""Ring tensors: Z_2^64, Z_2^128 and Z_2 (bits) on CPU or MI355X.

``RT`` wraps a torch tensor:

* Z_2^64  -> ``torch.int64`` of the logical shape (two's complement = u64 bits),
* Z_2^128 -> ``torch.int64`` of shape ``(*shape, 2)`` holding (lo, hi) words, i.e. the
  in-memory layout of ``unsigned __int128``; the native kernels read it as such,
* Z_2     -> ``torch.uint8`` holding 0/1.

Elementwise Z_2^64 / Z_2 arithmetic uses torch's wrapping integer kernels; everything
that torch cannot express (Z_2^128 arithmetic, exact ring GEMM, AES-CTR PRG, the fused RSS
step) goes to ``libmoosex`` (``csrc/``), on the tensor's device and current HIP stream.

Axis arguments are *logical*: ``nb`` leading batch dimensions (e.g. the party axis of a
stacked 3-party session) are skipped.

Parity: reference host ring kernels ``moose/src/host/ops.rs:1709-2036``.
"""
from __future__ import annotations

import builtins
import ctypes
import functools
import math
import os
import threading
from contextlib import contextmanager
from fractions import Fraction
from typing import List
from typing import NamedTuple
from typing import Sequence

import numpy as np
import torch

from moose_amd.ops import native as nat

MASK64 = (1 << 64) - 1
MASK128 = (1 << 128) - 1

_BIN = {"add": 0, "sub": 1, "mul": 2, "and": 3, "or": 4, "xor": 5}
_UN = {"neg": 0, "not": 1, "shl": 2, "shr": 3, "sar": 4}
_CMP = {"lt": 0, "gt": 1, "eq": 2, "msb": 3}


# Every host->device copy made while a computation runs goes through to_device, so that
# hipGraph capture (runtime/graphs.py) can substitute copies staged before the capture.
# The hook is per thread (in-process parties record and capture on their own threads).
_UPLOAD_HOOK = None  # process-wide fallback
_TLS = threading.local()


def upload_hook():
    h = getattr(_TLS, "hook", None)
    return h if h is not None else _UPLOAD_HOOK


def set_upload_hook(hook):
    """Install ``hook`` for the calling thread; returns the previous one."""
    prev = getattr(_TLS, "hook", None)
    _TLS.hook = hook
    return prev


def to_device(t: torch.Tensor, device) -> torch.Tensor:
    device = torch.device(device)
    if device.type == "cpu" or t.device == device:
        return t
    hook = upload_hook()
    if hook is not None:
        return hook(t, device)
    return t.to(device)


def _words(bits):
    return {1: 0, 64: 1, 128: 2}[bits]


class RT:
    """A ring tensor (see module docstring)."""

    __slots__ = ("data", "bits", "_shape")

    def __init__(self, data: torch.Tensor, bits: int):
        self.data = data
        self.bits = bits
        self._shape = None

    # -- shape -------------------------------------------------------------
    @property
    def shape(self):
        s = self._shape
        if s is None:  # computed once: shapes are read several times per launch
            s = tuple(self.data.shape)
            s = self._shape = s[:-1] if self.bits == 128 else s
        return s

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def device(self):
        return self.data.device

    def numel(self):
        return math.prod(self.shape)

    def __repr__(self):
        return f"RT(bits={self.bits}, shape={self.shape}, device={self.device})"

    def contiguous(self):
        return RT(self.data.contiguous(), self.bits)

    def clone(self):
        return RT(self.data.clone(), self.bits)

    # -- arithmetic --------------------------------------------------------
    def __add__(self, o):
        return binary("add", self, o)

    def __sub__(self, o):
        return binary("sub", self, o)

    def __mul__(self, o):
        return binary("mul", self, o)

    def __and__(self, o):
        return binary("and", self, o)

    def __or__(self, o):
        return binary("or", self, o)

    def __xor__(self, o):
        return binary("xor", self, o)

    def __neg__(self):
        return unary("neg", self)

    def __invert__(self):
        return unary("not", self)

    def shl(self, k):
        return unary("shl", self, k)

    def shr(self, k):
        return unary("shr", self, k)

    def sar(self, k):
        return unary("sar", self, k)


# ---------------------------------------------------------------------------
# construction / conversion
# ---------------------------------------------------------------------------
def empty(shape, bits, device) -> RT:
    shape = tuple(shape)
    if bits == 128:
        return RT(torch.empty(shape + (2,), dtype=torch.int64, device=device), 128)
    if bits == 64:
        return RT(torch.empty(shape, dtype=torch.int64, device=device), 64)
    return RT(torch.empty(shape, dtype=torch.uint8, device=device), 1)


def empty2(shape, bits, device):
    """Two ring tensors of one shape from ONE allocation (the paired outputs of the share-
    pair / stacked-protocol kernels)."""
    both = empty((2,) + tuple(shape), bits, device).data
    return RT(both[0], bits), RT(both[1], bits)


_RING4 = os.environ.get("MOOSEX_RING4", "1") != "0"


def ring4(shape, bits, device):
    """The two share vectors of a stacked replicated value ([3, ...]) as views of ONE
    [4, ...] buffer holding slots x0, x1, x2, x0: s0 = buf[0:3], s1 = buf[1:4] = s0 rolled
    by one party.  Pair-producing kernels detect out1 == out0 + slot and write 4 slots, not
    6; every consumer sees two ordinary contiguous [3, ...] tensors."""
    shape = tuple(shape)
    if not shape or shape[0] != 3 or not _RING4:
        return empty2(shape, bits, device)
    buf = empty((4,) + shape[1:], bits, device).data
    return RT(buf[0:3], bits), RT(buf[1:4], bits)


def zeros(shape, bits, device) -> RT:
    r = empty(shape, bits, device)
    r.data.zero_()
    return r


_SCALARS = {}
# > 0 while several threads issue work on their own streams of one device (the in-process
# parties, parallel/threads.py): a cached constant is then read by other streams too.  A
# count, so that overlapping evaluations of several runtimes do not clear it for each other
SHARED_STREAMS = 0
_SHARED_LOCK = threading.Lock()


def shared_streams(delta: int):
    global SHARED_STREAMS
    with _SHARED_LOCK:
        SHARED_STREAMS = max(0, SHARED_STREAMS + delta)


# MOOSEX_CONST_CACHE=0: no shared device constants (every use makes its own; diagnostics)
CONST_CACHE = os.environ.get("MOOSEX_CONST_CACHE", "1") != "0"


def _cache_put(cache, key, t, limit):
    """Insert a freshly made device constant into a shared cache.  While dataflow lanes
    run (runtime/lanes.py) other streams may read it next, so the producing stream is
    drained first (once per constant)."""
    if len(cache) >= limit or not CONST_CACHE:
        return
    from moose_amd.runtime import lanes

    d = t[1].data if isinstance(t, tuple) else t.data
    if (lanes.ACTIVE or SHARED_STREAMS) and d.is_cuda:
        torch.cuda.current_stream(d.device).synchronize()
    with _SHARED_LOCK:
        # first in wins: parties on threads may make one constant at once, and an entry
        # keyed by an object's id must keep that object alive (never replaced)
        cache.setdefault(key, t)


def fill(shape, value: int, bits, device) -> RT:
    """Constant ring tensor (``value`` taken mod 2^bits).

    Scalars (shape ``()``) are the public constants of the protocols (encoded
    coefficients, masks, 1/n ...); they are created once per device and shared -- callers
    never write into a fill result.  Not while a hipGraph is being captured: the tensor
    would live in the graph's private pool."""
    shape = tuple(shape)
    if not shape:
        key = (int(value), bits, str(device))
        hit = _SCALARS.get(key)
        if hit is not None:
            return hit
        t = _fill(shape, value, bits, device)
        if torch.device(device).type == "cpu" or not torch.cuda.is_current_stream_capturing():
            _cache_put(_SCALARS, key, t, 65536)
        return t
    return _fill(shape, value, bits, device)


def _fill(shape, value: int, bits, device) -> RT:
    if bits == 1:
        return RT(torch.full(shape, int(value) & 1, dtype=torch.uint8, device=device), 1)
    if bits == 64:
        v = _to_i64(int(value) & MASK64)
        return RT(torch.full(shape, v, dtype=torch.int64, device=device), 64)
    v = int(value) & MASK128
    lo, hi = _to_i64(v & MASK64), _to_i64(v >> 64)
    # one native fill kernel (slice assignment of a python int would be a host->device
    # copy, which is not allowed while a hipGraph is being captured)
    out = empty(shape, 128, device)
    nat.check(nat.lib().mx_fill(nat.dev_of(out.data), 2, nat.ptr(out.data), math.prod(shape),
                                lo & MASK64, hi & MASK64, nat.stream_of(out.data)), "fill")
    return out


def _to_i64(u):
    u &= MASK64
    return u - (1 << 64) if u >= (1 << 63) else u


def from_ints(values, bits, device="cpu") -> RT:
    """Build from python ints / nested lists (values reduced mod 2^bits)."""
    arr = np.array(values, dtype=object)
    shape = arr.shape
    flat = [int(x) for x in arr.reshape(-1)]
    if bits == 1:
        t = torch.tensor([v & 1 for v in flat], dtype=torch.uint8).reshape(shape)
        return RT(to_device(t, device), 1)
    if bits == 64:
        t = torch.tensor([_to_i64(v) for v in flat], dtype=torch.int64).reshape(shape)
        return RT(to_device(t, device), 64)
    pairs = [[_to_i64(v & MASK64), _to_i64((v >> 64) & MASK64)] for v in flat]
    t = torch.tensor(pairs, dtype=torch.int64).reshape(shape + (2,))
    return RT(to_device(t, device), 128)


def to_ints(x: RT) -> np.ndarray:
    """Unsigned python-int view (object ndarray) -- test/inspection helper."""
    d = x.data.detach().cpu()
    if x.bits == 1:
        return d.numpy().astype(object)
    if x.bits == 64:
        return np.vectorize(lambda v: int(v) & MASK64, otypes=[object])(d.numpy())
    a = d.numpy()
    lo = np.vectorize(lambda v: int(v) & MASK64, otypes=[object])(a[..., 0])
    hi = np.vectorize(lambda v: int(v) & MASK64, otypes=[object])(a[..., 1])
    return lo + hi * (1 << 64)


def to_signed_ints(x: RT) -> np.ndarray:
    u = to_ints(x)
    half = 1 << (x.bits - 1)
    return np.vectorize(lambda v: v - (1 << x.bits) if v >= half else v, otypes=[object])(u)


# ---------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------
def _as_rt(o, like: RT) -> RT:
    if isinstance(o, RT):
        return o
    if isinstance(o, int):
        return fill((), o, like.bits, like.device)
    raise TypeError(f"cannot combine RT with {type(o)}")


def _broadcast(a: RT, b: RT):
    if a.shape == b.shape:
        return a, b
    shp = torch.broadcast_shapes(a.shape, b.shape)
    return expand(a, shp), expand(b, shp)


def expand(a: RT, shape) -> RT:
    shape = tuple(shape)
    if a.shape == shape:
        return a
    if a.bits == 128:
        return RT(a.data.expand(shape + (2,)), 128)
    return RT(a.data.expand(shape), a.bits)


def binary(op: str, a, b, alloc=None) -> RT:
    """a op b elementwise; ``alloc(shape, dtype)``: where the result goes (a session's
    outbox when it is a message; Z_2^64 / Z_2^128 only)."""
    if not isinstance(a, RT):
        a = _as_rt(a, b)
    b = _as_rt(b, a)
    if a.bits != b.bits:
        raise TypeError(f"ring width mismatch {a.bits} vs {b.bits}")
    bits = a.bits
    if bits == 1:
        x, y = a.data, b.data
        if op in ("add", "sub", "xor"):
            return RT(x ^ y, 1)
        if op in ("mul", "and"):
            return RT(x & y, 1)
        if op == "or":
            return RT(x | y, 1)
    # Z_2^64 / Z_2^128: one native kernel (libmoosex, gfx950 on the device); scalar
    # operands broadcast natively, other broadcasts are expanded first
    na, nb_ = a.numel(), b.numel()
    if na != nb_ and na != 1 and nb_ != 1:
        a, b = _broadcast(a, b)
        na = nb_ = a.numel()
    n = max(na, nb_)
    out_shape = a.shape if na >= nb_ else b.shape
    out = _empty_in(alloc, out_shape, bits, a.device)
    ad, bd = a.data.contiguous(), b.data.contiguous()
    nat.check(
        nat.lib().mx_ew_binary(
            nat.dev_of(ad), _BIN[op], _words(bits), nat.ptr(ad), na, nat.ptr(bd), nb_,
            nat.ptr(out.data), n, nat.stream_of(ad),
        ),
        f"ring{bits} {op}",
    )
    return out


def unary(op: str, a: RT, k: int = 0) -> RT:
    bits = a.bits
    if bits == 1:
        if op == "neg":
            return RT(a.data.clone(), 1)
        if op == "not":
            return RT(a.data ^ 1, 1)
        return RT(a.data.clone() if k == 0 else torch.zeros_like(a.data), 1)
    out = empty(a.shape, bits, a.device)
    ad = a.data.contiguous()
    nat.check(
        nat.lib().mx_ew_unary(
            nat.dev_of(ad), _UN[op], _words(bits), nat.ptr(ad), nat.ptr(out.data), a.numel(),
            int(k), nat.stream_of(ad),
        ),
        f"ring128 {op}",
    )
    return out


def transpose2(a0: RT, a1: RT):
    """(a0^T, a1^T) of two [rows, cols] ring matrices (a party's share components) in one
    launch (mx_transpose2: 32 x 32 tiles through LDS) instead of two strided copies."""
    rows, cols = a0.shape
    bits = a0.bits
    d0, d1 = a0.data.contiguous(), a1.data.contiguous()
    o0, o1 = empty2((cols, rows), bits, d0.device)
    nat.check(nat.lib().mx_transpose2(
        nat.dev_of(d0), _words(bits), nat.ptr(d0), nat.ptr(o0.data), nat.ptr(d1),
        nat.ptr(o1.data), rows, cols, nat.stream_of(d0)), "transpose2")
    return o0, o1


def binary2(op: str, a0: RT, b0: RT, a1: RT, b1: RT):
    """(a0 op b0, a1 op b1) -- both share vectors of a share-wise replicated op -- in one
    launch (mx_ew_binary2).  Operands of each pair have the same shapes as the other pair's;
    anything else (bit tensors, general broadcasts) takes two binary() calls."""
    bits = a0.bits
    na, nb_ = a0.numel(), b0.numel()
    if (bits == 1 or not all(isinstance(t, RT) and t.bits == bits for t in (b0, a1, b1))
            or a1.shape != a0.shape or b1.shape != b0.shape
            or (na != nb_ and na != 1 and nb_ != 1)):
        return binary(op, a0, b0), binary(op, a1, b1)
    n = max(na, nb_)
    shp = a0.shape if na >= nb_ else b0.shape
    o0, o1 = empty2(shp, bits, a0.device)
    d = [t.data.contiguous() for t in (a0, b0, a1, b1)]
    nat.check(nat.lib().mx_ew_binary2(
        nat.dev_of(d[0]), _BIN[op], _words(bits), nat.ptr(d[0]), nat.ptr(d[1]),
        nat.ptr(o0.data), nat.ptr(d[2]), nat.ptr(d[3]), nat.ptr(o1.data), na, nb_, n,
        nat.stream_of(d[0])), f"ring{bits} {op} (pair)")
    return o0, o1


def unary2(op: str, a0: RT, a1: RT, k: int = 0):
    """(op a0, op a1) in one launch (mx_ew_unary2)."""
    if a0.bits == 1 or a1.bits != a0.bits or a1.shape != a0.shape:
        return unary(op, a0, k), unary(op, a1, k)
    o0, o1 = empty2(a0.shape, a0.bits, a0.device)
    d0, d1 = a0.data.contiguous(), a1.data.contiguous()
    nat.check(nat.lib().mx_ew_unary2(
        nat.dev_of(d0), _UN[op], _words(a0.bits), nat.ptr(d0), nat.ptr(o0.data), nat.ptr(d1),
        nat.ptr(o1.data), a0.numel(), int(k), nat.stream_of(d0)), f"ring{a0.bits} {op} (pair)")
    return o0, o1


def compare(op: str, a: RT, b: RT = None) -> RT:
    """Signed comparison -> bit tensor (op: lt, gt, eq, msb)."""
    if a.bits == 64 and op != "msb":
        x, y = a.data, b.data
        r = {"lt": x < y, "gt": x > y, "eq": x == y}[op]
        return RT(r.to(torch.uint8), 1)
    if a.bits == 64:
        return RT(((a.data >> 63) & 1).to(torch.uint8), 1)
    if b is not None and a.shape != b.shape and b.numel() != 1 and a.numel() != 1:
        a, b = _broadcast(a, b)
    n = max(a.numel(), b.numel() if b is not None else 0)
    shape = a.shape if b is None or a.numel() >= b.numel() else b.shape
    out = torch.empty(shape, dtype=torch.uint8, device=a.device)
    ad = a.data.contiguous()
    bd = b.data.contiguous() if b is not None else None
    nat.check(
        nat.lib().mx_ew_compare(
            nat.dev_of(ad), _CMP[op], _words(a.bits), nat.ptr(ad), a.numel(), nat.ptr(bd),
            b.numel() if b is not None else 0, nat.ptr(out), n, nat.stream_of(ad),
        ),
        f"compare {op}",
    )
    return RT(out, 1)


def bit_extract(a: RT, bit: int) -> RT:
    if a.data.is_cuda and a.bits in (64, 128) and 0 <= bit < a.bits:  # one kernel
        ad = a.data.contiguous()
        out = torch.empty(a.shape, dtype=torch.uint8, device=ad.device)
        nat.check(nat.lib().mx_bit_extract(nat.dev_of(ad), _words(a.bits), nat.ptr(ad),
                                           nat.ptr(out), out.numel(), bit, nat.stream_of(ad)),
                  "bit_extract")
        return RT(out, 1)
    if a.bits == 64:
        return RT(((a.data >> bit) & 1).to(torch.uint8), 1)
    w = a.data[..., bit // 64]
    return RT(((w >> (bit % 64)) & 1).to(torch.uint8), 1)


def ring_inject(bitsrt: RT, bit: int, ring_bits: int) -> RT:
    """bit tensor -> ring tensor with the bit placed at position ``bit``."""
    if bitsrt.data.is_cuda and ring_bits in (64, 128) and 0 <= bit < ring_bits:  # one kernel
        bd = bitsrt.data.contiguous()
        if bd.dtype != torch.uint8:
            bd = bd.to(torch.uint8)
        out = empty(tuple(bd.shape), ring_bits, bd.device)
        nat.check(nat.lib().mx_ring_inject(nat.dev_of(bd), _words(ring_bits), nat.ptr(bd),
                                           nat.ptr(out.data), bd.numel(), bit,
                                           nat.stream_of(bd)), "ring_inject")
        return out
    b = bitsrt.data.to(torch.int64) & 1
    if ring_bits == 64:
        return RT(b << bit if bit < 64 else torch.zeros_like(b), 64)
    out = torch.zeros(tuple(b.shape) + (2,), dtype=torch.int64, device=b.device)
    if bit < 64:
        out[..., 0] = b << bit
    else:
        out[..., 1] = b << (bit - 64)
    return RT(out, 128)


def cast(a: RT, bits: int) -> RT:
    """Ring width change: truncation 128->64, zero extension 64->128, bit->ring."""
    if a.bits == bits:
        return a
    if a.bits == 128 and bits == 64:
        return RT(a.data[..., 0].contiguous(), 64)
    if a.bits == 64 and bits == 128:
        out = torch.zeros(tuple(a.data.shape) + (2,), dtype=torch.int64, device=a.device)
        out[..., 0] = a.data
        return RT(out, 128)
    if a.bits == 1:
        return ring_inject(a, 0, bits)
    if bits == 1:
        return bit_extract(a, 0)
    raise TypeError(f"cannot cast ring {a.bits} -> {bits}")


def sign_extend(a: RT, from_bits: int, bits: int) -> RT:
    """64 -> 128 with sign extension."""
    assert a.bits == 64 and bits == 128
    out = torch.empty(tuple(a.data.shape) + (2,), dtype=torch.int64, device=a.device)
    out[..., 0] = a.data
    out[..., 1] = a.data >> 63
    return RT(out, 128)


# ---------------------------------------------------------------------------
# fixed-point encode / decode (reference host/fixedpoint.rs, host/ops.rs: truncating,
# saturating `as i64` / `as i128` at the ring's own width; correctly rounded `as f64`)
# ---------------------------------------------------------------------------
def encode(x: torch.Tensor, frac: int, bits: int) -> RT:
    x = x.to(torch.float64).contiguous()
    out = empty(tuple(x.shape), bits, x.device)
    nat.check(
        nat.lib().mx_encode(
            nat.dev_of(x), _words(bits), nat.ptr(x), nat.ptr(out.data), x.numel(), int(frac),
            nat.stream_of(x),
        ),
        "encode",
    )
    return out


def _stream_of(t: torch.Tensor):
    """The current stream of ``t``'s device (None on the host): where a lazy value's inputs
    were issued."""
    return torch.cuda.current_stream(t.device) if t.is_cuda else None


def _join(stream):
    """Order the current stream after the work issued so far on ``stream`` -- a lazy value
    created on one stream and consumed on another (dataflow lanes, step streams)."""
    if stream is not None:
        cur = torch.cuda.current_stream(stream.device)
        if cur != stream:
            cur.wait_stream(stream)


class Encoded(RT):
    """A float64 tensor's fixed-point encoding (x * 2^frac), formed on first use of
    ``data``.  Input sharing of it encodes inside the share kernel (kind MX_SHARE_F64): the
    ring-valued encoding never goes to memory."""

    __slots__ = ("src", "frac", "stream")

    def __init__(self, x: torch.Tensor, frac: int, bits: int):
        _RT_DATA.__set__(self, None)
        self.bits = bits
        self._shape = tuple(x.shape)
        self.src = x
        self.frac = int(frac)
        self.stream = _stream_of(x)

    def pending(self) -> bool:
        return _RT_DATA.__get__(self) is None

    @property
    def data(self):
        d = _RT_DATA.__get__(self)
        if d is None:
            _join(self.stream)
            d = encode(self.src, self.frac, self.bits).data
            _RT_DATA.__set__(self, d)
            self.src = None
        return d

    @data.setter
    def data(self, v):
        _RT_DATA.__set__(self, v)

    @property
    def device(self):
        return self.src.device if self.pending() else self.data.device


# ids of cached computation constants (runtime/interpreter.py _CONST_LV keeps them alive)
CONST_IDS = set()
_ENCODED_CONSTS = {}


def encode_lazy(x: torch.Tensor, frac: int, bits: int) -> RT:
    """encode(), deferred to the first use (:class:`Encoded`) for 64/128-bit rings; a
    cached computation constant is encoded once (not while a hipGraph is being captured:
    the result would live in the graph's pool)."""
    if id(x) in CONST_IDS and x.is_cuda:
        key = (id(x), int(frac), bits)
        hit = _ENCODED_CONSTS.get(key)
        # the entry holds its source tensor: an id is only ever matched while that very
        # tensor lives (a freed tensor's id may come back as another tensor's)
        if hit is not None and hit[0] is x:
            return hit[1]
        if not torch.cuda.is_current_stream_capturing():
            e = encode(x, frac, bits)
            _cache_put(_ENCODED_CONSTS, key, (x, e), 4096)
            return e
    if bits not in (64, 128):
        return encode(x, frac, bits)
    return Encoded(x.to(torch.float64).contiguous(), frac, bits)


def share_source(x: RT, kind: str):
    """(kind code, device tensor, aux) for the share kernels: an unencoded float64 input is
    passed as is (MX_SHARE_F64 = 2, aux = its fractional bits), else the ring data."""
    if kind == "arith" and isinstance(x, Encoded) and x.pending():
        _join(x.stream)
        return 2, x.src, x.frac
    return (1 if kind == "bool" else 0), x.data.contiguous(), None


def decode(a: RT, frac: int) -> torch.Tensor:
    if isinstance(a, OpenedTail) and a.pending():  # tail + reveal + decode: one kernel
        out = a.src.open(frac)
        if out is not None:
            return out
        a = a.shares()  # the shares exist by now: the ordinary reveal of them
    if isinstance(a, Opened) and a.pending():  # the reveal's add fused into the decode
        _join(a.stream)
        d = [t.data.contiguous() for t in a.parts]
        out = torch.empty(a.shape, dtype=torch.float64, device=a.device)
        ptrs = [nat.ptr(x) for x in d] + [None] * (4 - len(d))
        nat.check(nat.lib().mx_addn_decode(
            nat.dev_of(d[0]), _words(a.bits), *ptrs, nat.ptr(out), a.numel(),
            int(frac), nat.stream_of(d[0])), "addn_decode")
        return out
    ad = a.data.contiguous()
    out = torch.empty(a.shape, dtype=torch.float64, device=a.device)
    nat.check(
        nat.lib().mx_decode(
            nat.dev_of(ad), _words(a.bits), nat.ptr(ad), nat.ptr(out), a.numel(), int(frac),
            nat.stream_of(ad),
        ),
        "decode",
    )
    return out


# ---------------------------------------------------------------------------
# shape ops (logical axes after `nb` batch dims)
# ---------------------------------------------------------------------------
def _ax(a: RT, axis: int, nb: int) -> int:
    nd = a.ndim - nb
    if axis < 0:
        axis += nd
    if not 0 <= axis < max(nd, 1):
        raise IndexError(f"axis {axis} out of range for logical rank {nd}")
    return axis + nb


def reshape(a: RT, shape, nb=0) -> RT:
    shape = tuple(int(s) for s in shape)
    full = a.shape[:nb] + shape
    if a.bits == 128:
        return RT(a.data.reshape(full + (2,)), 128)
    return RT(a.data.reshape(full), a.bits)


def transpose(a: RT, nb=0, perm=None) -> RT:
    nd = a.ndim - nb
    perm = list(range(nd))[::-1] if perm is None else list(perm)
    full = list(range(nb)) + [p + nb for p in perm]
    if a.bits == 128:
        full.append(a.ndim)
    return RT(a.data.permute(full).contiguous(), a.bits)


def expand_dims(a: RT, axes, nb=0) -> RT:
    d = a.data
    nd = a.ndim - nb
    for ax in sorted(int(x) for x in axes):
        if ax < 0:
            ax += nd + 1
        d = d.unsqueeze(ax + nb)
        nd += 1
    return RT(d, a.bits)


def squeeze(a: RT, axis=None, nb=0) -> RT:
    if axis is None:
        shape = a.shape[:nb] + tuple(s for s in a.shape[nb:] if s != 1)
        return reshape(a, shape[nb:], nb)
    ax = _ax(a, axis, nb)
    return RT(a.data.squeeze(ax), a.bits)


def concat(xs: Sequence[RT], axis=0, nb=0) -> RT:
    ax = _ax(xs[0], axis, nb)
    return RT(torch.cat([x.data for x in xs], dim=ax), xs[0].bits)


def index_axis(a: RT, axis: int, index: int, nb=0) -> RT:
    ax = _ax(a, axis, nb)
    v = a.data.select(ax, index)
    if nb == 1 and ax == 1 and v.dim() >= 1 and v[0].is_contiguous():
        # one entry of a party-stacked batch ([P, k, ...] -> [P, ...]): a view whose party
        # slots stay dense -- consumers read it in place or copy on demand
        return RT(v, a.bits)
    return RT(v.contiguous(), a.bits)


def slice_axis(a: RT, axis: int, start, end, step=None, nb=0) -> RT:
    ax = _ax(a, axis, nb)
    idx = [slice(None)] * a.data.dim()
    idx[ax] = slice(start, end, step)
    return RT(a.data[tuple(idx)].contiguous(), a.bits)


def strided_slice(a: RT, slices, nb=0) -> RT:
    idx = [slice(None)] * nb + list(slices)
    d = a.data
    # torch lacks negative steps: emulate with flip
    for i, s in enumerate(idx):
        if isinstance(s, slice) and s.step is not None and s.step < 0:
            raise NotImplementedError("negative slice steps")
    return RT(d[tuple(idx)].contiguous(), a.bits)


_ELEM_BYTES = {1: 1, 64: 8, 128: 16}


def _elem_bytes(bits):
    """Bytes of one element as the native image leaves count them (a bit is a uint8)."""
    return _ELEM_BYTES[bits]


def _leaf_operand(t: RT, nb, dense, rank4=None, lead=()):
    """(data, slot stride in elements) of an image leaf's operand after ``nb`` batch dims: a
    [slots, ...] view with dense slots is read in place (its slot stride non-negative and a
    multiple of the words per element), anything else as a contiguous copy at the ``dense``
    stride.  With ``rank4`` (dwconv) a rank-4 operand beside batch dims is public -- one copy
    for every slot, stride 0 -- and any other operand has to be ``lead + rank4``."""
    d = t.data
    if rank4 is not None:
        if len(t.shape) == 4 and nb:
            return d.contiguous(), 0
        if tuple(t.shape[:nb]) != tuple(lead) or tuple(t.shape[nb:]) != tuple(rank4):
            raise ValueError(f"dwconv: operand of shape {tuple(t.shape)} does not match the batch "
                             f"dims {lead} and the shape {tuple(rank4)}")
    if nb == 1 and d.shape[0] and d[0].is_contiguous():
        st, w = d.stride(0), 2 if t.bits == 128 else 1  # int64 words per element (uint8: bits)
        if st >= 0 and st % w == 0:
            return d, st // w
    return d.contiguous(), dense


def _leaf_pair(d0, st0, d1, st1, dense):
    """Both components of a pair go to the leaf at one slot stride: ``(d0, d1, stride)`` as
    they are when their strides agree, else both dense."""
    if st0 == st1:
        return d0, d1, st0
    return d0.contiguous(), d1.contiguous(), dense


def im2col_geometry(shape, kernel_shape, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
                    data_format="NCHW"):
    """Validate the attributes of an im2col over a rank-4 ``shape`` and return
    ``(N, C, H, W, KH, KW, sh, sw, pt, pl, pb, pr, dh, dw, OH, OW)``; ``pads`` is (top, left,
    bottom, right), the ONNX order.  ``ValueError`` on anything malformed, and on an output
    that would be empty (``OH <= 0`` or ``OW <= 0``)."""
    if data_format not in ("NCHW", "NHWC"):
        raise ValueError(f"im2col: data_format must be 'NCHW' or 'NHWC', found {data_format!r}")
    shape = tuple(int(s) for s in shape)
    if len(shape) != 4:
        raise ValueError(f"im2col expects a rank-4 {data_format} tensor, found shape {shape}")
    for name, v, n in (("kernel_shape", kernel_shape, 2), ("strides", strides, 2),
                       ("pads", pads, 4), ("dilations", dilations, 2)):
        if not isinstance(v, (tuple, list)) or len(v) != n or \
                not all(isinstance(x, (int, np.integer)) for x in v):
            raise ValueError(f"im2col: `{name}` must be {n} ints, found {v!r}")
    KH, KW = (int(k) for k in kernel_shape)
    sh, sw = (int(s) for s in strides)
    pt, pl, pb, pr = (int(p) for p in pads)
    dh, dw = (int(d) for d in dilations)
    if min(KH, KW) <= 0 or min(sh, sw) <= 0 or min(dh, dw) <= 0:
        raise ValueError("im2col: kernel_shape, strides and dilations must be positive, found "
                         f"{tuple(kernel_shape)}, {tuple(strides)}, {tuple(dilations)}")
    if min(pt, pl, pb, pr) < 0:
        raise ValueError(f"im2col: pads must be non-negative, found {tuple(pads)}")
    if data_format == "NCHW":
        N, C, H, W = shape
    else:
        N, H, W, C = shape
    OH = (H + pt + pb - dh * (KH - 1) - 1) // sh + 1
    OW = (W + pl + pr - dw * (KW - 1) - 1) // sw + 1
    if OH <= 0 or OW <= 0:
        raise ValueError(
            f"im2col: a {KH}x{KW} kernel (dilations {(dh, dw)}) does not fit the padded "
            f"{H + pt + pb}x{W + pl + pr} image: output would be {OH}x{OW}")
    return N, C, H, W, KH, KW, sh, sw, pt, pl, pb, pr, dh, dw, OH, OW


def im2col_torch(d: torch.Tensor, geom, data_format, nb=0) -> torch.Tensor:
    """im2col as a torch composition (zero pad, ``as_strided`` window view, ``contiguous``)
    on a tensor of dims ``[nb batch dims, N, C, H, W, trailing...]`` (or N, H, W, C): the
    path of plain host tensors, and the yardstick of the ring kernel."""
    N, C, H, W, KH, KW, sh, sw, pt, pl, pb, pr, dh, dw, OH, OW = geom
    lead, tail = tuple(d.shape[:nb]), tuple(d.shape[nb + 4:])
    nhwc = data_format == "NHWC"
    hax = nb + (1 if nhwc else 2)
    if pt or pl or pb or pr:
        shp = list(d.shape)
        shp[hax] += pt + pb
        shp[hax + 1] += pl + pr
        padded = d.new_zeros(shp)
        idx = [slice(None)] * d.dim()
        idx[hax], idx[hax + 1] = slice(pt, pt + H), slice(pl, pl + W)
        padded[tuple(idx)] = d
    else:
        padded = d.contiguous()
    st = padded.stride()
    sN, sH, sW = st[nb], st[hax], st[hax + 1]
    sC = st[nb + 3] if nhwc else st[nb + 1]
    if nhwc:
        size = (N, OH, OW, KH, KW, C)
        stride = (sN, sH * sh, sW * sw, sH * dh, sW * dw, sC)
    else:
        size = (N, OH, OW, C, KH, KW)
        stride = (sN, sH * sh, sW * sw, sC, sH * dh, sW * dw)
    nt = len(tail)
    view = padded.as_strided(lead + size + tail,
                             tuple(st[:nb]) + stride + tuple(st[len(st) - nt:] if nt else ()))
    return view.contiguous().reshape(lead + (N * OH * OW, C * KH * KW) + tail)


# The device default of im2col: the gather kernel, or the torch composition when False
# (benchmarks/conv2d.py measures both; profiles/conv2d.md has the numbers)
IM2COL_KERNEL = True


def im2col(a: RT, kernel_shape, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
           data_format="NCHW", nb=0) -> RT:
    """Patch matrix of a rank-4 ring tensor after ``nb`` batch dims: ``[..., N*OH*OW,
    C*KH*KW]``, rows (n, oh, ow), columns (c, kh, kw) for NCHW and (kh, kw, c) for NHWC, zero
    in the padding.  One native launch over all batch slots (``mx_im2col``), which reads a
    slot-strided view ([slots, ...] with dense slots) in place."""
    geom = im2col_geometry(a.shape[nb:], kernel_shape, strides, pads, dilations, data_format)
    N, C, H, W, KH, KW, sh, sw, pt, pl, _pb, _pr, dh, dw, OH, OW = geom
    lead = tuple(a.shape[:nb])
    out_shape = lead + (N * OH * OW, C * KH * KW)
    if a.device.type == "meta":  # shape inference of the symbolic session
        return empty(out_shape, a.bits, a.device)
    if a.device.type == "cuda" and not IM2COL_KERNEL:
        tail = 1 if a.bits == 128 else 0
        assert a.data.dim() == nb + 4 + tail
        return RT(im2col_torch(a.data, geom, data_format, nb), a.bits)
    d, slot_stride = _leaf_operand(a, nb, N * C * H * W)
    slots = math.prod(lead)
    out = empty(out_shape, a.bits, a.device)
    nat.check(
        nat.lib().mx_im2col(
            nat.dev_of(d), _elem_bytes(a.bits), nat.ptr(d), nat.ptr(out.data),
            slots, slot_stride, N, C, H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW,
            1 if data_format == "NHWC" else 0, nat.stream_of(d)),
        "im2col",
    )
    return out


def col2im_geometry(cols_shape, image_chw, kernel_shape, strides=(1, 1), pads=(0, 0, 0, 0),
                    dilations=(1, 1), data_format="NCHW"):
    """Validate a col2im of a patch matrix ``cols_shape = [N*OH*OW, C*KH*KW]`` into an image
    of ``image_chw = (C, H, W)`` and return :func:`im2col_geometry`'s tuple for that image,
    with ``N`` read off the rows.  ``ValueError`` when the attributes are malformed, the
    column count is not ``C*KH*KW`` or the rows are not a multiple of ``OH*OW``."""
    cols_shape = tuple(int(s) for s in cols_shape)
    if len(cols_shape) != 2:
        raise ValueError(f"col2im expects a rank-2 patch matrix, found shape {cols_shape}")
    if not isinstance(image_chw, (tuple, list)) or len(image_chw) != 3 or \
            not all(isinstance(x, (int, np.integer)) and x > 0 for x in image_chw):
        raise ValueError("col2im: `image_shape` must be 3 positive ints (C, H, W), found "
                         f"{image_chw!r}")
    C, H, W = (int(s) for s in image_chw)
    shape = (1, C, H, W) if data_format != "NHWC" else (1, H, W, C)
    try:
        g = im2col_geometry(shape, kernel_shape, strides, pads, dilations, data_format)
    except ValueError as e:
        raise ValueError(str(e).replace("im2col", "col2im")) from None
    KH, KW, OH, OW = g[4], g[5], g[14], g[15]
    if cols_shape[1] != C * KH * KW:
        raise ValueError(f"col2im: the patch matrix has {cols_shape[1]} columns, a {KH}x{KW} "
                         f"kernel over {C} channels needs {C * KH * KW}")
    if cols_shape[0] % (OH * OW):
        raise ValueError(f"col2im: {cols_shape[0]} rows are not a multiple of the {OH}x{OW} "
                         f"windows of a {H}x{W} image")
    return (cols_shape[0] // (OH * OW),) + g[1:]


def col2im_torch(d: torch.Tensor, geom, data_format, nb=0) -> torch.Tensor:
    """col2im as a torch composition on a tensor of dims ``[nb batch dims, N*OH*OW,
    C*KH*KW]``: ``F.fold`` into the padded image, then the crop ``[pt:pt+H, pl:pl+W]`` (which
    takes asymmetric pads).  The path of plain host tensors."""
    N, C, H, W, KH, KW, sh, sw, pt, pl, pb, pr, dh, dw, OH, OW = geom
    lead = tuple(d.shape[:nb])
    B = math.prod(lead) * N
    if data_format == "NHWC":
        m = d.reshape(B, OH * OW, KH * KW, C).permute(0, 3, 2, 1)
    else:
        m = d.reshape(B, OH * OW, C, KH * KW).permute(0, 2, 3, 1)
    m = m.reshape(B, C * KH * KW, OH * OW)
    img = torch.nn.functional.fold(m, (H + pt + pb, W + pl + pr), (KH, KW), dilation=(dh, dw),
                                   padding=0, stride=(sh, sw))
    img = img[:, :, pt:pt + H, pl:pl + W]
    if data_format == "NHWC":
        return img.permute(0, 2, 3, 1).reshape(lead + (N, H, W, C)).contiguous()
    return img.reshape(lead + (N, C, H, W)).contiguous()


def col2im(a: RT, image_chw, kernel_shape, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
           data_format="NCHW", nb=0) -> RT:
    """The exact adjoint of :func:`im2col`: the patch matrix ``[..., N*OH*OW, C*KH*KW]`` after
    ``nb`` batch dims summed (wrapping) into the image ``[..., N, C, H, W]`` (NHWC: ``[..., N,
    H, W, C]``) of ``image_chw = (C, H, W)``.  Entries whose tap lies in the padding are
    dropped and a pixel no window reaches is zero.  One native launch over all batch slots
    (``mx_col2im``), which reads a slot-strided view ([slots, ...] with dense slots) in
    place."""
    if a.bits not in (64, 128):
        raise ValueError(f"col2im is arithmetic only: Z_2^64 / Z_2^128, found {a.bits} bits")
    geom = col2im_geometry(a.shape[nb:], image_chw, kernel_shape, strides, pads, dilations,
                           data_format)
    N, C, H, W, KH, KW, sh, sw, pt, pl, _pb, _pr, dh, dw, OH, OW = geom
    lead = tuple(a.shape[:nb])
    nhwc = data_format == "NHWC"
    out_shape = lead + ((N, H, W, C) if nhwc else (N, C, H, W))
    if a.device.type == "meta":  # shape inference of the symbolic session
        return empty(out_shape, a.bits, a.device)
    d, slot_stride = _leaf_operand(a, nb, N * OH * OW * C * KH * KW)
    slots = math.prod(lead)
    out = empty(out_shape, a.bits, a.device)
    nat.check(
        nat.lib().mx_col2im(
            nat.dev_of(d), _elem_bytes(a.bits), nat.ptr(d), nat.ptr(out.data),
            slots, slot_stride, N, C, H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW,
            1 if nhwc else 0, nat.stream_of(d)),
        "col2im",
    )
    return out


RESIZE_MODES = ("nearest", "linear")
RESIZE_COORDS = ("half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric")
RESIZE_NEAREST = ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil")
RESIZE_MAX_WEIGHT_BITS = 12


def resize_scale(scale):
    """A resize scale as the exact rational of its binary value; ``None`` stays ``None`` (the
    scale is then O/I).  Accepts a float, an int, a ``Fraction`` or a ``(num, den)`` pair."""
    if scale is None:
        return None
    if isinstance(scale, (tuple, list)):
        scale = Fraction(int(scale[0]), int(scale[1]))
    s = Fraction(scale)
    if s <= 0:
        raise ValueError(f"resize: `scales` must be positive, found {scale!r}")
    return s


@functools.lru_cache(maxsize=1024)
def _resize_coords(I, O, mode, ctm, nearest_mode, scale):  # noqa: E741
    """Per output index of one axis: (i0, t) with the source coordinate i0 + t, 0 <= t < 1, per
    the ONNX ``Resize`` definition in exact rational arithmetic, clamped to [0, I - 1].  In
    nearest mode i0 is the chosen pixel and t is 0."""
    s = scale if scale is not None else Fraction(O, I)
    half = Fraction(1, 2)
    out = []
    for o in range(O):
        if ctm == "half_pixel":
            x = (o + half) / s - half
        elif ctm == "pytorch_half_pixel":
            x = (o + half) / s - half if O > 1 else Fraction(0)
        elif ctm == "align_corners":
            x = Fraction(o * (I - 1), O - 1) if O > 1 else Fraction(0)
        else:  # asymmetric
            x = o / s
        x = min(max(x, Fraction(0)), Fraction(I - 1))
        i0 = math.floor(x)
        t = x - i0
        if mode == "nearest":
            if nearest_mode == "round_prefer_floor":
                i0 += 1 if t > half else 0
            elif nearest_mode == "round_prefer_ceil":
                i0 += 1 if t >= half else 0
            elif nearest_mode == "ceil":
                i0 += 1 if t > 0 else 0
            t = Fraction(0)
        out.append((i0, t))
    return tuple(out)


def _resize_check_axis(I, O, mode, ctm, nearest_mode):  # noqa: E741
    if mode not in RESIZE_MODES:
        raise ValueError(f"resize: `mode` must be one of {RESIZE_MODES}, found {mode!r}")
    if ctm not in RESIZE_COORDS:
        raise ValueError("resize: `coordinate_transformation_mode` must be one of "
                         f"{RESIZE_COORDS}, found {ctm!r}")
    if nearest_mode not in RESIZE_NEAREST:
        raise ValueError(f"resize: `nearest_mode` must be one of {RESIZE_NEAREST}, found "
                         f"{nearest_mode!r}")
    if I <= 0 or O <= 0:
        raise ValueError(f"resize: sizes must be positive, found {I} -> {O}")


def resize_weight_bits(I, O, mode="linear", coordinate_transformation_mode="half_pixel",  # noqa: E741
                       nearest_mode="round_prefer_floor", scale=None):
    """The smallest weight width in 0..12 at which every interpolation weight of one axis is
    exact (2x ``half_pixel``: t in {1/4, 3/4}, so 2; nearest and an axis that keeps its size:
    0), else 12."""
    I, O = int(I), int(O)  # noqa: E741
    _resize_check_axis(I, O, mode, coordinate_transformation_mode, nearest_mode)
    coords = _resize_coords(I, O, mode, coordinate_transformation_mode, nearest_mode,
                            resize_scale(scale))
    for wb in range(RESIZE_MAX_WEIGHT_BITS + 1):
        if all((t * (1 << wb)).denominator == 1 for _i, t in coords):
            return wb
    return RESIZE_MAX_WEIGHT_BITS


@functools.lru_cache(maxsize=1024)
def _resize_tables(I, O, mode, ctm, nearest_mode, scale, wb):  # noqa: E741
    coords = _resize_coords(I, O, mode, ctm, nearest_mode, scale)
    tab = np.zeros((3, O), dtype=np.int32)
    for o, (i0, t) in enumerate(coords):
        w1 = math.floor(t * (1 << wb) + Fraction(1, 2))
        if wb == 0 and w1:  # the whole weight on the upper tap: it becomes the one tap
            i0, w1 = min(i0 + 1, I - 1), 0
        tab[:, o] = (i0, min(i0 + 1, I - 1), w1)
    tab.setflags(write=False)
    return tab


def resize_tables(I, O, mode="linear", coordinate_transformation_mode="half_pixel",  # noqa: E741
                  nearest_mode="round_prefer_floor", scale=None, weight_bits=0):
    """The table of one resized axis, int32 ``[3, O]`` with the rows ``i0``, ``i1``, ``w1``:
    output ``o`` is ``(2^wb - w1) * x[i0] + w1 * x[i1]`` with ``wb = weight_bits``.  The only
    place that turns resize attributes into numbers -- the CPU twin, the gfx950 kernel, the
    torch composition, shape inference and the tests' integer model all read it.  Source
    coordinates follow the ONNX ``Resize`` definition in exact rational arithmetic (a float
    ``scale`` is taken as its exact binary value; ``None``: O/I), are clamped to ``[0, I -
    1]``, ``i1 = min(i0 + 1, I - 1)`` and ``w1 = floor(t * 2^wb + 1/2)``: the same table on
    every machine.  Nearest mode has ``w1 = 0`` and ``i0`` the chosen pixel, whatever
    ``weight_bits`` says; so has a table of width 0 (a weight that rounds to the upper tap
    moves ``i0`` there).  The array is shared and read-only."""
    I, O, wb = int(I), int(O), int(weight_bits)  # noqa: E741
    _resize_check_axis(I, O, mode, coordinate_transformation_mode, nearest_mode)
    if not 0 <= wb <= RESIZE_MAX_WEIGHT_BITS:
        raise ValueError(f"resize: `weight_bits` must be in 0..{RESIZE_MAX_WEIGHT_BITS}, found "
                         f"{weight_bits!r}")
    if mode == "nearest":
        wb = 0
    return _resize_tables(I, O, mode, coordinate_transformation_mode, nearest_mode,
                          resize_scale(scale), wb)


def resize_geometry(shape, sizes, mode="nearest", coordinate_transformation_mode="half_pixel",
                    nearest_mode="round_prefer_floor", scales=(), weight_bits=(0, 0),
                    data_format="NCHW"):
    """Validate a resize of a rank-4 ``shape`` to ``sizes = (OH, OW)`` and return ``(N, C, H,
    W, OH, OW, wbh, wbw, sh, sw)``: the weight widths as the tables use them (0 in nearest
    mode) and the two scales as exact rationals or ``None``.  ``scales`` is empty, or one
    scale per axis (floats, or ``(num, den)`` pairs flattened to four ints, the form the
    serialised operator carries).  ``ValueError`` names the malformed argument."""
    if data_format not in ("NCHW", "NHWC"):
        raise ValueError(f"resize: data_format must be 'NCHW' or 'NHWC', found {data_format!r}")
    shape = tuple(int(s) for s in shape)
    if len(shape) != 4:
        raise ValueError(f"resize expects a rank-4 {data_format} tensor, found shape {shape}")
    for name, v in (("sizes", sizes), ("weight_bits", weight_bits)):
        if not isinstance(v, (tuple, list)) or len(v) != 2 or \
                not all(isinstance(x, (int, np.integer)) for x in v):
            raise ValueError(f"resize: `{name}` must be 2 ints, found {v!r}")
    OH, OW = (int(s) for s in sizes)
    if OH <= 0 or OW <= 0:
        raise ValueError(f"resize: `sizes` must be positive, found {tuple(sizes)}")
    if not isinstance(scales, (tuple, list)) or len(scales) not in (0, 2, 4):
        raise ValueError(f"resize: `scales` must be empty or one scale per axis, found "
                         f"{scales!r}")
    if len(scales) == 4:
        scales = (tuple(scales[0:2]), tuple(scales[2:4]))
    sh, sw = (resize_scale(s) for s in scales) if len(scales) else (None, None)
    N, C, H, W = shape if data_format == "NCHW" else (shape[0], shape[3], shape[1], shape[2])
    if H <= 0 or W <= 0:
        raise ValueError(f"resize: the image is empty ({H}x{W})")
    wbh, wbw = (int(b) for b in weight_bits)
    for I, O in ((H, OH), (W, OW)):  # noqa: E741
        _resize_check_axis(I, O, mode, coordinate_transformation_mode, nearest_mode)
    if not (0 <= wbh <= RESIZE_MAX_WEIGHT_BITS and 0 <= wbw <= RESIZE_MAX_WEIGHT_BITS):
        raise ValueError(f"resize: `weight_bits` must be in 0..{RESIZE_MAX_WEIGHT_BITS}, found "
                         f"{tuple(weight_bits)}")
    if mode == "nearest":
        wbh = wbw = 0
    return N, C, H, W, OH, OW, wbh, wbw, sh, sw


def _resize_axis_tables(geom, mode, ctm, nearest_mode):
    N, C, H, W, OH, OW, wbh, wbw, sh, sw = geom
    return (resize_tables(H, OH, mode, ctm, nearest_mode, sh, wbh),
            resize_tables(W, OW, mode, ctm, nearest_mode, sw, wbw))


def resize_torch(d: torch.Tensor, geom, mode="nearest",
                 coordinate_transformation_mode="half_pixel",
                 nearest_mode="round_prefer_floor", data_format="NCHW", nb=0,
                 bits=None) -> torch.Tensor:
    """Resize as a torch composition on a tensor of dims ``[nb batch dims, N, C, H, W,
    trailing...]`` (or N, H, W, C): ``index_select`` of the two taps on each axis, multiply by
    the table's weights, add.  Integer tensors (the int64 of Z_2^64, wrapping) get the integer
    weights -- the arithmetic of the ring kernel, its A/B baseline; ``bits=128`` says that the
    trailing dim holds the (lo, hi) words of Z_2^128, which are then summed as four 32-bit
    limbs (a limb's weighted sum stays below 2^56) with one carry pass at the end.  Float
    tensors get the same weights over ``2^wb``; bool and uint8 (bit) tensors only the gather
    of nearest mode."""
    N, C, H, W, OH, OW, wbh, wbw, _sh, _sw = geom
    th, tw = _resize_axis_tables(geom, mode, coordinate_transformation_mode, nearest_mode)
    hax = nb + (1 if data_format == "NHWC" else 2)
    x = d
    exact = not x.dtype.is_floating_point
    limbs = bits == 128 and wbh + wbw > 0
    if limbs:  # [..., 2] words -> [..., 4] limbs of 32 bits
        x = torch.stack((x[..., 0] & 0xffffffff, (x[..., 0] >> 32) & 0xffffffff,
                         x[..., 1] & 0xffffffff, (x[..., 1] >> 32) & 0xffffffff), dim=-1)
    for ax, tab, wb in ((hax, th, wbh), (hax + 1, tw, wbw)):
        i0 = to_device(torch.from_numpy(tab[0].astype(np.int64)), x.device)
        a = x.index_select(ax, i0)
        if tab[2].any():
            if x.dtype in (torch.bool, torch.uint8):
                raise ValueError("resize: a weighted sum of bits is not a bit; `linear` needs "
                                 "an arithmetic tensor")
            i1 = to_device(torch.from_numpy(tab[1].astype(np.int64)), x.device)
            view = [1] * x.dim()
            view[ax] = -1
            w1 = torch.from_numpy(tab[2].astype(np.int64))
            w0 = (1 << wb) - w1
            if not exact:
                w0, w1 = (w.to(x.dtype) / (1 << wb) for w in (w0, w1))
            w0, w1 = (to_device(w, x.device).reshape(view) for w in (w0, w1))
            a = a * w0 + x.index_select(ax, i1) * w1
        elif wb and exact:
            a = a * (1 << wb)
        x = a
    if limbs:
        v0 = x[..., 0]
        v1 = x[..., 1] + (v0 >> 32)
        v2 = x[..., 2] + (v1 >> 32)
        v3 = x[..., 3] + (v2 >> 32)
        x = torch.stack(((v0 & 0xffffffff) | (v1 << 32), (v2 & 0xffffffff) | (v3 << 32)),
                        dim=-1)
    return x.contiguous()


# The device default of resize: the stencil kernel, or the torch composition when False
# (benchmarks/resize.py measures both; profiles/resize.md has the numbers)
RESIZE_KERNEL = True

_RESIZE_TABLES = {}


def _resize_device_tables(key, tabs, device):
    """The two axis tables on ``device``, made once per (geometry, device) and shared (no
    upload per evaluation, so none inside a captured hipGraph; not cached while one is being
    captured: the tensors would live in the graph's pool)."""
    device = torch.device(device)
    if device.type == "cpu":
        return tabs
    key = key + (str(device),)
    hit = _RESIZE_TABLES.get(key)
    if hit is not None:
        return hit
    t = tuple(to_device(torch.from_numpy(t.copy()), device) for t in tabs)
    if not torch.cuda.is_current_stream_capturing():
        _cache_put(_RESIZE_TABLES, key, t, 4096)
    return t


def _table_ptr(t):
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def resize(a: RT, sizes, mode="nearest", coordinate_transformation_mode="half_pixel",
           nearest_mode="round_prefer_floor", scales=(), weight_bits=(0, 0),
           data_format="NCHW", nb=0) -> RT:
    """Resize the rank-4 ring tensor after ``nb`` batch dims to ``sizes = (OH, OW)``, exactly:
    ``out = sum_{a,b} wh_a * ww_b * x[ih_a, iw_b]`` (wrapping) with the integer weights of
    :func:`resize_tables`, so a ``linear`` result carries ``wbh + wbw`` more fractional bits
    (the leaf does not truncate).  One native launch over all batch slots (``mx_resize2d``),
    which reads a slot-strided view ([slots, ...] with dense slots) in place.  Bit tensors:
    nearest only, through the torch gather."""
    geom = resize_geometry(a.shape[nb:], sizes, mode, coordinate_transformation_mode,
                           nearest_mode, scales, weight_bits, data_format)
    N, C, H, W, OH, OW, wbh, wbw, sh, sw = geom
    lead = tuple(a.shape[:nb])
    nhwc = data_format == "NHWC"
    out_shape = lead + ((N, OH, OW, C) if nhwc else (N, C, OH, OW))
    if a.bits == 1 and mode != "nearest":
        raise ValueError("resize: a weighted sum of bits is not a bit; `linear` needs an "
                         "arithmetic tensor")
    if a.device.type == "meta":  # shape inference of the symbolic session
        return empty(out_shape, a.bits, a.device)
    if a.bits == 1 or (a.device.type == "cuda" and not RESIZE_KERNEL):
        return RT(resize_torch(a.data, geom, mode, coordinate_transformation_mode,
                               nearest_mode, data_format, nb, a.bits), a.bits)
    d, slot_stride = _leaf_operand(a, nb, N * C * H * W)
    slots = math.prod(lead)
    out = empty(out_shape, a.bits, a.device)
    if out.data.numel() == 0:
        return out
    key = (H, W, OH, OW, mode, coordinate_transformation_mode, nearest_mode, sh, sw, wbh, wbw)
    th, tw = _resize_device_tables(
        key, _resize_axis_tables(geom, mode, coordinate_transformation_mode, nearest_mode),
        a.device)
    nat.check(
        nat.lib().mx_resize2d(
            nat.dev_of(d), _elem_bytes(a.bits), nat.ptr(d), nat.ptr(out.data), slots,
            slot_stride, N, C, H, W, OH, OW, _table_ptr(th), _table_ptr(tw), wbh, wbw,
            1 if nhwc else 0, nat.stream_of(d)),
        "resize2d",
    )
    return out


def dwconv_geometry(x_shape, w_shape, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
                    data_format="NCHW"):
    """Validate a depthwise convolution of a rank-4 ``x_shape`` with the ONNX depthwise weight
    ``w_shape = [C*mult, 1, KH, KW]`` (as :func:`im2col_geometry`, plus the weight) and return
    ``(N, C, H, W, mult, KH, KW, sh, sw, pt, pl, pb, pr, dh, dw, OH, OW)``."""
    w_shape = tuple(int(s) for s in w_shape)
    if len(w_shape) != 4:
        raise ValueError("dwconv expects a rank-4 weight [C*mult, 1, KH, KW], found shape "
                         f"{w_shape}")
    try:
        g = im2col_geometry(x_shape, w_shape[2:], strides, pads, dilations, data_format)
    except ValueError as e:
        raise ValueError(str(e).replace("im2col", "dwconv")) from None
    N, C, H, W, KH, KW, sh, sw, pt, pl, pb, pr, dh, dw, OH, OW = g
    if w_shape[1] != 1:
        raise ValueError(f"dwconv: a depthwise weight is [C*mult, 1, KH, KW], found {w_shape} "
                         f"(w.shape[1] = {w_shape[1]})")
    if C <= 0 or w_shape[0] <= 0 or w_shape[0] % C:
        raise ValueError(f"dwconv: the weight's {w_shape[0]} output channels are not a positive "
                         f"multiple of the input's {C} channels")
    return N, C, H, W, w_shape[0] // C, KH, KW, sh, sw, pt, pl, pb, pr, dh, dw, OH, OW


def _dwconv(x0, x1, w0, w1, strides, pads, dilations, data_format, nb):
    bits = x0.bits
    ops = [t for t in (x0, x1, w0, w1) if t is not None]
    if bits not in (64, 128) or any(t.bits != bits for t in ops):
        raise ValueError("dwconv is arithmetic only: operands over one of Z_2^64 / Z_2^128, "
                         f"found {[t.bits for t in ops]} bits")
    xpub, wpub = bool(nb) and len(x0.shape) == 4, bool(nb) and len(w0.shape) == 4
    if xpub and wpub:
        raise ValueError("dwconv: with batch dims, the image or the weight has to carry them")
    lead = tuple((w0 if xpub else x0).shape[:nb])
    xs = tuple(x0.shape) if xpub else tuple(x0.shape[nb:])
    ws = tuple(w0.shape) if wpub else tuple(w0.shape[nb:])
    geom = dwconv_geometry(xs, ws, strides, pads, dilations, data_format)
    N, C, H, W, mult, KH, KW, sh, sw, pt, pl, _pb, _pr, dh, dw, OH, OW = geom
    nhwc = data_format == "NHWC"
    out_shape = lead + ((N, OH, OW, C * mult) if nhwc else (N, C * mult, OH, OW))
    if x0.device.type == "meta":  # shape inference of the symbolic session
        return empty(out_shape, bits, x0.device)
    xn, wn = N * C * H * W, C * mult * KH * KW
    xd0, xst = _leaf_operand(x0, nb, xn, xs, lead)
    wd0, wst = _leaf_operand(w0, nb, wn, ws, lead)
    xd1 = wd1 = None
    if x1 is not None:
        xd1, xst1 = _leaf_operand(x1, nb, xn, xs, lead)
        wd1, wst1 = _leaf_operand(w1, nb, wn, ws, lead)
        xd0, xd1, xst = _leaf_pair(xd0, xst, xd1, xst1, 0 if xpub else xn)
        wd0, wd1, wst = _leaf_pair(wd0, wst, wd1, wst1, 0 if wpub else wn)
    out = empty(out_shape, bits, x0.device)
    nat.check(
        nat.lib().mx_dwconv(
            nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(xd0),
            nat.ptr(xd1) if xd1 is not None else None, nat.ptr(wd0),
            nat.ptr(wd1) if wd1 is not None else None, nat.ptr(out.data), math.prod(lead),
            xst, wst, N, C, H, W, mult, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW,
            1 if nhwc else 0, nat.stream_of(out.data)),
        "dwconv",
    )
    return out


def dwconv(x: RT, w: RT, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
           data_format="NCHW", nb=0) -> RT:
    """Ring depthwise convolution of a rank-4 tensor after ``nb`` batch dims with the dense
    weight ``[..., C*mult, 1, KH, KW]``: ``out[n, oh, ow, c*mult + j] = sum_taps x[n, ., ., c]
    * w[c*mult + j, 0, kh, kw]`` (wrapping), in the input's layout.  One native launch over all
    batch slots (``mx_dwconv``); a [slots, ...] view with dense slots is read in place, and a
    rank-4 operand beside a batched one is public: every slot reads the one copy."""
    return _dwconv(x, None, w, None, strides, pads, dilations, data_format, nb)


def dwconv_cross(x0: RT, x1: RT, w0: RT, w1: RT, strides=(1, 1), pads=(0, 0, 0, 0),
                 dilations=(1, 1), data_format="NCHW", nb=0) -> RT:
    """RSS cross terms of a depthwise convolution, ``x0 * (w0 + w1) + x1 * w0`` summed over the
    taps in one pass (:func:`dwconv`'s conventions; x1 / w1 are the next party's components)."""
    return _dwconv(x0, x1, w0, w1, strides, pads, dilations, data_format, nb)


# ---------------------------------------------------------------------------
# piecewise-linear local step
# ---------------------------------------------------------------------------
PWL_MAX = 8  # MX_PWL_MAX (moosex.h): the flag planes one launch takes

# the device path of pwl / pwl_cross: the native kernel (True) or the torch composition
# pwl_torch (False); a CPU tensor always takes the native loops
PWL_KERNEL = True


@functools.lru_cache(maxsize=1024)
def _pwl_tables(da, db, ak, bits):
    return _ring_words(da, bits), _ring_words(db, bits), _ring_words((ak,), bits)


def _pwl_check(s0, s1, x0, x1, da, db, nb):
    k = len(da)
    if not 1 <= k <= PWL_MAX or len(db) != k:
        raise ValueError(f"pwl: between 1 and {PWL_MAX} flag planes with one DA and one DB entry "
                         f"each, found {k} and {len(db)}")
    if (s1 is None) != (x1 is None):
        raise ValueError("pwl: the cross form takes both next components")
    ops = [t for t in (s0, s1, x0, x1) if t is not None]
    bits = x0.bits
    if bits not in (64, 128) or any(t.bits != bits for t in ops):
        raise ValueError("pwl is arithmetic only: operands over one of Z_2^64 / Z_2^128, found "
                         f"{[t.bits for t in ops]} bits")
    if nb not in (0, 1):
        raise ValueError("pwl takes at most one batch dim")
    lead, shape = tuple(x0.shape[:nb]), tuple(x0.shape[nb:])
    for t, want in ((s0, lead + (k,) + shape), (s1, lead + (k,) + shape), (x1, lead + shape)):
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"pwl: operand of shape {tuple(t.shape)}, expected {want}")
    return k, bits, lead, shape


def pwl_torch(s0: RT, s1, x0: RT, x1, da, db, ak, nb=0) -> RT:
    """:func:`pwl_cross` as a composition of the existing kernels (weighted sums of the flag
    planes, then elementwise products and sums): the fallback and the benchmark's opponent."""
    _pwl_check(s0, s1, x0, x1, da, db, nb)
    g0, h = weighted_sum(s0, da, nb), weighted_sum(s0, db, nb)
    v = binary("add", binary("mul", binary("add", g0, int(ak)), x0), h)
    if s1 is not None:
        g1 = weighted_sum(s1, da, nb)
        v = binary("add", v, binary("add", binary("mul", g0, x1), binary("mul", g1, x0)))
    return v


def pwl_cross(s0: RT, s1, x0: RT, x1, da, db, ak, nb=0) -> RT:
    """One party's local step of a secret piecewise-linear function, exact in the ring: with
    the flag planes ``s0`` / ``s1`` ([.., k, *shape]), the input components ``x0`` / ``x1``
    ([.., *shape]) and public python ints ``da[k]``, ``db[k]``, ``ak``,
    ``G0 * (x0 + x1) + G1 * x0 + ak * x0 + sum_j db[j] * s0[j]`` where ``Gc = sum_j da[j] *
    sc[j]`` (own times the sum plus next times own, as :func:`dwconv_cross`).  ``s1 = x1 =
    None``: the plain form ``G0 * x0 + ak * x0 + sum_j db[j] * s0[j]``.  One native launch
    over all batch slots (``mx_pwl_cross``); [slots, ...] views with dense slots are read in
    place and the tables travel in the launch's arguments."""
    k, bits, lead, shape = _pwl_check(s0, s1, x0, x1, da, db, nb)
    if x0.device.type == "meta":  # shape inference of the symbolic session
        return empty(lead + shape, bits, x0.device)
    if x0.device.type == "cuda" and not PWL_KERNEL:
        return pwl_torch(s0, s1, x0, x1, da, db, ak, nb)
    n = math.prod(shape)
    out = empty(lead + shape, bits, x0.device)
    if out.data.numel() == 0:
        return out
    sd0, sst = _leaf_operand(s0, nb, k * n)
    xd0, xst = _leaf_operand(x0, nb, n)
    sd1 = xd1 = None
    if s1 is not None:
        sd1, sst1 = _leaf_operand(s1, nb, k * n)
        xd1, xst1 = _leaf_operand(x1, nb, n)
        sd0, sd1, sst = _leaf_pair(sd0, sst, sd1, sst1, k * n)
        xd0, xd1, xst = _leaf_pair(xd0, xst, xd1, xst1, n)
    tda, tdb, tak = _pwl_tables(tuple(int(v) for v in da), tuple(int(v) for v in db), int(ak),
                                bits)
    nat.check(
        nat.lib().mx_pwl_cross(
            nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(sd0),
            nat.ptr(sd1) if sd1 is not None else None, nat.ptr(xd0),
            nat.ptr(xd1) if xd1 is not None else None, nat.ptr(out.data), math.prod(lead), sst,
            xst, n, k, tda, tdb, tak, nat.stream_of(out.data)),
        "pwl_cross",
    )
    return out


def pwl(s: RT, x: RT, da, db, ak, nb=0) -> RT:
    """The plain form of :func:`pwl_cross`: ``(ak + sum_j da[j] * s[j]) * x + sum_j db[j] *
    s[j]`` over the flag planes ``s`` ([.., k, *shape]) -- a host's ring tensor, or slot-wise
    use."""
    return pwl_cross(s, None, x, None, da, db, ak, nb)


# ---------------------------------------------------------------------------
# piecewise-polynomial local step
# ---------------------------------------------------------------------------
PWP_MAX = 8  # MX_PWP_MAX (moosex.h): the flag planes one launch takes
PWP_DEG = 3  # MX_PWP_DEG: the largest degree

# the device path of pwp / pwp_cross: the native kernel (True) or the torch composition
# pwp_torch (False); a CPU tensor always takes the native loops
PWP_KERNEL = True


@functools.lru_cache(maxsize=1024)
def _pwp_tables(D, CK, bits):
    return _ring_words([v for row in D for v in row], bits), _ring_words(CK, bits)


def _pwp_check(s0, s1, p0, p1, D, CK, nb):
    """-> (k, d, bits, lead, shape).  ``D``: d + 1 rows of k ring integers, row i the
    differences of the degree-i coefficients (row 0 the constants); ``CK``: the last piece's d
    coefficients of degrees 1..d; ``p0`` / ``p1``: the d powers' components."""
    d = len(D) - 1
    if not 1 <= d <= PWP_DEG:
        raise ValueError(f"pwp: a degree between 1 and {PWP_DEG} (one table row per degree and "
                         f"one for the constants), found {len(D)} rows")
    k = len(D[0])
    if not 1 <= k <= PWP_MAX or any(len(row) != k for row in D):
        raise ValueError(f"pwp: between 1 and {PWP_MAX} flag planes with one entry per plane in "
                         f"every table row, found rows of {[len(row) for row in D]}")
    if len(CK) != d:
        raise ValueError(f"pwp: degree {d} takes {d} last-piece coefficients (degrees 1..{d}), "
                         f"found {len(CK)}")
    if isinstance(p0, RT) or len(p0) != d or (p1 is not None and (isinstance(p1, RT)
                                                                  or len(p1) != d)):
        raise ValueError(f"pwp: degree {d} takes {d} powers per component")
    if (s1 is None) != (p1 is None):
        raise ValueError("pwp: the cross form takes both next components")
    ops = [s0, *p0] + ([s1, *p1] if s1 is not None else [])
    bits = p0[0].bits
    if bits not in (64, 128) or any(t.bits != bits for t in ops):
        raise ValueError("pwp is arithmetic only: operands over one of Z_2^64 / Z_2^128, found "
                         f"{[t.bits for t in ops]} bits")
    if nb not in (0, 1):
        raise ValueError("pwp takes at most one batch dim")
    lead, shape = tuple(p0[0].shape[:nb]), tuple(p0[0].shape[nb:])
    wants = [(s0, lead + (k,) + shape), (s1, lead + (k,) + shape)]
    wants += [(t, lead + shape) for t in (*p0, *(p1 or ()))]
    for t, want in wants:
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"pwp: operand of shape {tuple(t.shape)}, expected {want}")
    return k, d, bits, lead, shape


def pwp_torch(s0: RT, s1, p0, p1, D, CK, nb=0) -> RT:
    """:func:`pwp_cross` as a composition of the existing kernels (weighted sums of the flag
    planes, then elementwise products and sums): the fallback and the benchmark's opponent."""
    _k, d, _bits, _lead, _shape = _pwp_check(s0, s1, p0, p1, D, CK, nb)
    v = weighted_sum(s0, D[0], nb)
    for i in range(1, d + 1):
        g0 = weighted_sum(s0, D[i], nb)
        v = binary("add", v, binary("mul", binary("add", g0, int(CK[i - 1])), p0[i - 1]))
        if s1 is not None:
            g1 = weighted_sum(s1, D[i], nb)
            v = binary("add", v, binary("add", binary("mul", g0, p1[i - 1]),
                                        binary("mul", g1, p0[i - 1])))
    return v


def pwp_cross(s0: RT, s1, p0, p1, D, CK, nb=0) -> RT:
    """One party's local step of a secret piecewise polynomial of degree ``d = len(D) - 1`` in
    {1, 2, 3}, exact in the ring: with the flag planes ``s0`` / ``s1`` ([.., k, *shape]), the
    components ``p0[i-1]`` / ``p1[i-1]`` of the powers P_1 = x, .., P_d ([.., *shape] each) and
    public python ints ``D[i][j]`` (row 0: the constants) and ``CK[i-1]``,
    ``sum_{i=1..d} [G_i^0 * (P_i^0 + P_i^1) + G_i^1 * P_i^0 + CK_i * P_i^0] + sum_j D[0][j] *
    s0[j]`` where ``G_i^c = sum_j D[i][j] * sc[j]`` (own times the sum plus next times own, as
    :func:`pwl_cross`, which it equals bit for bit at d = 1).  ``s1 = p1 = None``: the plain
    form.  One native launch over all batch slots (``mx_pwp_cross``); every power is read in
    place through its own pointer, [slots, ...] views with dense slots included, and the
    tables travel in the launch's arguments."""
    k, d, bits, lead, shape = _pwp_check(s0, s1, p0, p1, D, CK, nb)
    dev = p0[0].device
    if dev.type == "meta":  # shape inference of the symbolic session
        return empty(lead + shape, bits, dev)
    if dev.type == "cuda" and not PWP_KERNEL:
        return pwp_torch(s0, s1, p0, p1, D, CK, nb)
    n = math.prod(shape)
    out = empty(lead + shape, bits, dev)
    if out.data.numel() == 0:
        return out
    sd0, sst = _leaf_operand(s0, nb, k * n)
    sd1 = None
    if s1 is not None:
        sd1, sst1 = _leaf_operand(s1, nb, k * n)
        sd0, sd1, sst = _leaf_pair(sd0, sst, sd1, sst1, k * n)
    pd0, pd1, pst = [], [], []
    for i in range(d):
        a0, st = _leaf_operand(p0[i], nb, n)
        a1 = None
        if p1 is not None:
            a1, st1 = _leaf_operand(p1[i], nb, n)
            a0, a1, st = _leaf_pair(a0, st, a1, st1, n)
        pd0.append(a0), pd1.append(a1), pst.append(st)
    tdt, tck = _pwp_tables(tuple(tuple(int(v) for v in row) for row in D),
                           tuple(int(v) for v in CK), bits)
    ptrs = ctypes.c_void_p * d
    nat.check(
        nat.lib().mx_pwp_cross(
            nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(sd0),
            nat.ptr(sd1) if sd1 is not None else None, ptrs(*[nat.ptr(t) for t in pd0]),
            ptrs(*[nat.ptr(t) for t in pd1]) if p1 is not None else None, nat.ptr(out.data),
            math.prod(lead), sst, (ctypes.c_int64 * d)(*pst), n, k, d, tdt, tck,
            nat.stream_of(out.data)),
        "pwp_cross",
    )
    return out


def pwp(s: RT, p, D, CK, nb=0) -> RT:
    """The plain form of :func:`pwp_cross`: ``sum_i (CK_i + sum_j D[i][j] * s[j]) * p[i-1] +
    sum_j D[0][j] * s[j]`` over the flag planes ``s`` ([.., k, *shape]) and the powers ``p`` --
    a host's ring tensors, or slot-wise use."""
    return pwp_cross(s, None, p, None, D, CK, nb)


# ---------------------------------------------------------------------------
# compare-exchange stages of a bitonic sorting network
# ---------------------------------------------------------------------------
# the device path of cswap_diff / cswap_cross / cswap_apply: the native kernels (True) or the
# torch compositions cswap_*_torch (False); a CPU tensor always takes the native loops
CSWAP_KERNEL = True


class CswapGeom(NamedTuple):
    """One stage (k, j) of a bitonic network along the middle axis of an [outer, n, inner]
    array (csrc/cswap_geom.h): element (o, pos, c) lives at (o*n + pos)*inner + c; n, k, j
    powers of two with j < k <= n; ``by = -1`` sorts every inner index on its own, ``by >= 0``
    orders whole rows by column ``by`` (table mode)."""

    outer: int
    n: int
    inner: int
    by: int = -1
    k: int = 2
    j: int = 1
    descending: bool = False

    @property
    def cols(self):
        return 1 if self.by >= 0 else self.inner


def cswap_stages(n: int):
    """The (k, j) stages of a bitonic network on n = 2^m elements: m (m + 1) / 2 of them."""
    out, k = [], 2
    while k <= n:
        j = k // 2
        while j >= 1:
            out.append((k, j))
            j //= 2
        k *= 2
    return out


def cswap_pairs(g: CswapGeom):
    """(i, l, ascending) of the n/2 pairs of stage ``g``: i is t with a zero bit inserted at
    bit log2 j, l = i | j, ascending iff (i & k) == 0, flipped by ``descending``."""
    lj = g.j.bit_length() - 1
    out = []
    for t in range(g.n // 2):
        i = ((t >> lj) << (lj + 1)) | (t & (g.j - 1))
        out.append((i, i | g.j, ((i & g.k) == 0) != bool(g.descending)))
    return out


def _cswap_check(what, g: CswapGeom, nb, x: RT, others=()):
    g = CswapGeom(*(int(v) for v in g))
    n, k, j = g.n, g.k, g.j
    if (g.outer < 0 or g.inner < 0 or n < 2 or n & (n - 1) or k & (k - 1) or j < 1 or j & (j - 1)
            or not j < k <= n or not -1 <= g.by < max(g.inner, 1)):
        raise ValueError(f"{what}: malformed stage {g}")
    bits = x.bits
    if bits not in (64, 128) or any(t.bits != bits for t, _ in others if t is not None):
        raise ValueError(f"{what} is arithmetic only: operands over one of Z_2^64 / Z_2^128")
    if nb not in (0, 1):
        raise ValueError(f"{what} takes at most one batch dim")
    lead = tuple(x.shape[:nb])
    if math.prod(x.shape[nb:]) != g.outer * n * g.inner:
        raise ValueError(f"{what}: operand of shape {tuple(x.shape)} does not hold "
                         f"{g.outer} x {n} x {g.inner} elements after {nb} batch dims")
    for t, want in others:
        if t is not None and (tuple(t.shape[:nb]) != lead or math.prod(t.shape[nb:]) != want):
            raise ValueError(f"{what}: operand of shape {tuple(t.shape)}, expected {want} "
                             f"elements after the batch dims {lead}")
    return g, bits, lead


def _cswap_args(g: CswapGeom):
    return (g.outer, g.n, g.inner, g.by, g.k, g.j, int(bool(g.descending)))


def _cswap_halves(t: RT, g: CswapGeom, nb, cols):
    """The low and the high element of every pair as two [.., outer, n/(2j), j, cols] views."""
    lead = tuple(t.shape[:nb])
    v = reshape(RT(t.data, t.bits), (g.outer, g.n // (2 * g.j), 2, g.j, cols), nb)
    return (RT(v.data.select(nb + 2, 0), t.bits), RT(v.data.select(nb + 2, 1), t.bits)), lead


def cswap_diff_torch(x: RT, g: CswapGeom, nb=0) -> RT:
    """:func:`cswap_diff` as a composition of the existing kernels (slices, a subtraction and a
    product with the public +-1 direction of every block): the benchmark's opponent."""
    g, bits, lead = _cswap_check("cswap_diff", g, nb, x)
    cols = g.cols
    if g.by >= 0:
        x = slice_axis(reshape(x, (g.outer, g.n, g.inner), nb), 2, g.by, g.by + 1, nb=nb)
    (lo, hi), _ = _cswap_halves(x, g, nb, cols)
    c = binary("sub", hi, lo)
    blocks = g.n // (2 * g.j)
    dirs = [1 if (((a * 2 * g.j) & g.k) == 0) != bool(g.descending) else -1
            for a in range(blocks)]
    if any(d < 0 for d in dirs):
        c = binary("mul", c, reshape(const_ints(dirs, bits, x.device), (blocks, 1, 1)))
    return reshape(c, (g.outer, g.n // 2, cols), nb)


def cswap_cross_torch(s0: RT, s1, x0: RT, x1, g: CswapGeom, nb=0) -> RT:
    """:func:`cswap_cross` as a composition of the existing kernels."""
    g, bits, lead = _cswap_check("cswap_cross", g, nb, x0, _cswap_others(g, s0, s1, x1))
    blocks = g.n // (2 * g.j)

    def diff(x):
        (lo, hi), _ = _cswap_halves(x, g, nb, g.inner)
        return binary("sub", lo, hi)

    def flags(s):
        return reshape(s, (g.outer, blocks, g.j, g.cols), nb)

    d0 = diff(x0)
    if x1 is None:
        v = binary("mul", flags(s0), d0)
    else:
        v = binary("add", binary("mul", flags(s0), binary("add", d0, diff(x1))),
                   binary("mul", flags(s1), d0))
    return reshape(v, (g.outer, g.n // 2, g.inner), nb)


def cswap_apply_torch(x: RT, p: RT, g: CswapGeom, nb=0) -> RT:
    """:func:`cswap_apply` as a composition of the existing kernels."""
    g, bits, lead = _cswap_check("cswap_apply", g, nb, x,
                                 ((p, g.outer * (g.n // 2) * g.inner),))
    (lo, hi), _ = _cswap_halves(x, g, nb, g.inner)
    pp = reshape(p, (g.outer, g.n // (2 * g.j), g.j, g.inner), nb)
    lo, hi = binary("sub", lo, pp), binary("add", hi, pp)
    out = RT(torch.stack((lo.data, hi.data), dim=nb + 2), bits)
    return reshape(out, x.shape[nb:], nb)


def _cswap_others(g, s0, s1, x1):
    nf = g.outer * (g.n // 2) * g.cols
    if (s1 is None) != (x1 is None):
        raise ValueError("cswap_cross: the cross form takes both next components")
    return ((s0, nf), (s1, nf), (x1, g.outer * g.n * g.inner))


def cswap_diff(x: RT, g: CswapGeom, nb=0) -> RT:
    """The signed differences of stage ``g``'s pairs, exact in the ring: ``x[l] - x[i]`` for an
    ascending pair, ``x[i] - x[l]`` for a descending one -- negative where the pair is out of
    order -- as [.., outer, n/2, inner], or on the key column only, [.., outer, n/2, 1], in
    table mode.  One native launch over all batch slots (``mx_cswap_diff``); a [slots, ...]
    view with dense slots is read in place and the stage travels in the launch's arguments."""
    g, bits, lead = _cswap_check("cswap_diff", g, nb, x)
    shape = lead + (g.outer, g.n // 2, g.cols)
    if x.device.type == "meta":  # shape inference of the symbolic session
        return empty(shape, bits, x.device)
    if x.device.type == "cuda" and not CSWAP_KERNEL:
        return cswap_diff_torch(x, g, nb)
    out = empty(shape, bits, x.device)
    if out.data.numel() == 0:
        return out
    xd, xst = _leaf_operand(x, nb, g.outer * g.n * g.inner)
    nat.check(
        nat.lib().mx_cswap_diff(nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(xd),
                                nat.ptr(out.data), math.prod(lead), xst, *_cswap_args(g),
                                nat.stream_of(out.data)),
        "cswap_diff",
    )
    return out


def cswap_cross(s0: RT, s1, x0: RT, x1, g: CswapGeom, nb=0) -> RT:
    """One party's local product of the flags and the differences of stage ``g``: with ``D =
    x[i] - x[l]``, ``s0 * (D0 + D1) + s1 * D0`` (own times the sum plus next times own, as
    :func:`pwl_cross`) as [.., outer, n/2, inner]; the flags are [.., outer, n/2, inner], or
    [.., outer, n/2, 1] broadcast over the columns in table mode.  ``s1 = x1 = None``: the
    plain form ``s0 * D0``.  One native launch over all batch slots (``mx_cswap_cross``)."""
    g, bits, lead = _cswap_check("cswap_cross", g, nb, x0, _cswap_others(g, s0, s1, x1))
    shape = lead + (g.outer, g.n // 2, g.inner)
    if x0.device.type == "meta":
        return empty(shape, bits, x0.device)
    if x0.device.type == "cuda" and not CSWAP_KERNEL:
        return cswap_cross_torch(s0, s1, x0, x1, g, nb)
    out = empty(shape, bits, x0.device)
    if out.data.numel() == 0:
        return out
    nf, nx = g.outer * (g.n // 2) * g.cols, g.outer * g.n * g.inner
    sd0, sst = _leaf_operand(s0, nb, nf)
    xd0, xst = _leaf_operand(x0, nb, nx)
    sd1 = xd1 = None
    if s1 is not None:
        sd1, sst1 = _leaf_operand(s1, nb, nf)
        xd1, xst1 = _leaf_operand(x1, nb, nx)
        sd0, sd1, sst = _leaf_pair(sd0, sst, sd1, sst1, nf)
        xd0, xd1, xst = _leaf_pair(xd0, xst, xd1, xst1, nx)
    nat.check(
        nat.lib().mx_cswap_cross(
            nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(sd0),
            nat.ptr(sd1) if sd1 is not None else None, nat.ptr(xd0),
            nat.ptr(xd1) if xd1 is not None else None, nat.ptr(out.data), math.prod(lead), sst,
            xst, *_cswap_args(g), nat.stream_of(out.data)),
        "cswap_cross",
    )
    return out


def cswap_apply(x: RT, p: RT, g: CswapGeom, nb=0) -> RT:
    """The exchange of stage ``g``: ``out[i] = x[i] - p[t]`` and ``out[l] = x[l] + p[t]`` with
    the products ``p`` [.., outer, n/2, inner], in ``x``'s shape.  With ``p = s * (x[i] -
    x[l])`` and ``s`` the 0/1 flag of an out-of-order pair, the pair is swapped where it has to
    be.  One native launch over all batch slots (``mx_cswap_apply``)."""
    g, bits, lead = _cswap_check("cswap_apply", g, nb, x, ((p, g.outer * (g.n // 2) * g.inner),))
    shape = tuple(x.shape)
    if x.device.type == "meta":
        return empty(shape, bits, x.device)
    if x.device.type == "cuda" and not CSWAP_KERNEL:
        return cswap_apply_torch(x, p, g, nb)
    out = empty(shape, bits, x.device)
    if out.data.numel() == 0:
        return out
    xd, xst = _leaf_operand(x, nb, g.outer * g.n * g.inner)
    pd, pst = _leaf_operand(p, nb, g.outer * (g.n // 2) * g.inner)
    nat.check(
        nat.lib().mx_cswap_apply(nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(xd),
                                 nat.ptr(pd), nat.ptr(out.data), math.prod(lead), xst, pst,
                                 *_cswap_args(g), nat.stream_of(out.data)),
        "cswap_apply",
    )
    return out


# ---------------------------------------------------------------------------
# the local step of an oblivious shuffle: a permutation from PRF output, and a row gather
# ---------------------------------------------------------------------------
# the device path of perm_gather: the native kernel (True) or the torch composition
# perm_gather_torch (False); a CPU tensor always takes the native loops
SHUFFLE_KERNEL = True

_I64_MIN = torch.iinfo(torch.int64).min


def perm_from_keys(keys: RT) -> torch.Tensor:
    """The permutation of 0..n-1 that sorts the n 64-bit ``keys`` (a Z_2^64 vector of PRF
    output) as unsigned integers, ascending and STABLE: equal keys keep their order, so both
    holders of a PRF key derive the same permutation on any device.  An int64 tensor on the
    keys' device -- the only producer of the index vectors :func:`perm_gather` takes.  torch
    has no unsigned 64-bit sort: the top bit is flipped and the values sort as int64."""
    if not isinstance(keys, RT) or keys.bits != 64 or keys.ndim != 1:
        raise ValueError("perm_from_keys takes a Z_2^64 vector of sort keys")
    if keys.device.type == "meta":  # shape inference of the symbolic session
        return torch.empty(keys.shape, dtype=torch.int64, device="meta")
    return torch.argsort(keys.data ^ _I64_MIN, dim=0, stable=True)


def _perm_gather_check(a: RT, perm, others, axis, nb):
    if not isinstance(a, RT) or a.bits not in (64, 128):
        raise ValueError("perm_gather is arithmetic only: operands over one of Z_2^64 / Z_2^128")
    if nb not in (0, 1):
        raise ValueError("perm_gather takes at most one batch dim")
    nd = a.ndim - nb
    if nd < 1 or isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) \
            or not -nd <= axis < nd:
        raise ValueError(f"perm_gather: axis {axis!r} out of range for a tensor of rank {nd}")
    ax = int(axis) % nd + nb
    shape = tuple(a.shape)
    n = shape[ax]
    if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64:
        raise ValueError("perm_gather: `perm` must be an int64 tensor (R.perm_from_keys), found "
                         f"{getattr(perm, 'dtype', type(perm).__name__)}")
    if perm.dim() != 1 or perm.shape[0] != n:
        raise ValueError(f"perm_gather: `perm` of shape {tuple(perm.shape)} does not match the "
                         f"axis length {n}")
    if perm.device != a.device:
        raise ValueError(f"perm_gather: `perm` lives on {perm.device}, the operands on "
                         f"{a.device}")
    for name, t in others:
        if t is not None and (not isinstance(t, RT) or t.bits != a.bits
                              or tuple(t.shape) != shape or t.device != a.device):
            raise ValueError(f"perm_gather: `{name}` must be a Z_2^{a.bits} tensor of shape "
                             f"{shape} on {a.device}, found {t!r}")
    return ax, math.prod(shape[nb:ax]), n, math.prod(shape[ax + 1:])


def _add128(x, y):
    lo = x[..., 0] + y[..., 0]
    carry = ((lo ^ _I64_MIN) < (x[..., 0] ^ _I64_MIN)).to(torch.int64)
    return torch.stack((lo, x[..., 1] + y[..., 1] + carry), dim=-1)


def _sub128(x, y):
    borrow = ((x[..., 0] ^ _I64_MIN) < (y[..., 0] ^ _I64_MIN)).to(torch.int64)
    return torch.stack((x[..., 0] - y[..., 0], x[..., 1] - y[..., 1] - borrow), dim=-1)


def perm_gather_torch(a: RT, perm, b=None, plus=None, minus=None, axis=0, nb=0) -> RT:
    """:func:`perm_gather` as a torch composition on the int64 views (index_select, add and
    sub, with the carry between the two words for Z_2^128): the benchmark's opponent."""
    ax, _, _, _ = _perm_gather_check(a, perm, (("b", b), ("plus", plus), ("minus", minus)),
                                     axis, nb)
    add, sub = (_add128, _sub128) if a.bits == 128 else (torch.add, torch.sub)
    v = a.data.index_select(ax, perm)
    if b is not None:
        v = add(v, b.data.index_select(ax, perm))
    if plus is not None:
        v = add(v, plus.data)
    if minus is not None:
        v = sub(v, minus.data)
    return RT(v, a.bits)


def perm_gather(a: RT, perm, b=None, plus=None, minus=None, axis=0, nb=0) -> RT:
    """Rows of ``a`` gathered along ``axis`` through ``perm``, fused with the sums of a shuffle
    step, wrapping in the ring: over ``a`` seen as [.., outer, n, inner],

        out[o, r, c] = a[o, perm[r], c] (+ b[o, perm[r], c]) (+ plus[o, r, c]) (- minus[o, r, c])

    ``b``, ``plus`` and ``minus`` are optional tensors of ``a``'s shape; without them it is a
    plain row gather.  ``perm`` is an int64 [n] tensor on the operands' device and MUST be a
    permutation of 0..n-1 (:func:`perm_from_keys` is the one producer): the CPU twin refuses
    anything else, but nothing reads a device ``perm`` back to check it -- there the kernel
    only clamps what it reads, so a bad ``perm`` gathers wrong rows, never outside the tensor.
    One native launch over all batch slots (``mx_perm_gather``); [slots, ...] views with dense
    slots are read in place.  The result is a new tensor: a gather is not in-place safe."""
    others = (("b", b), ("plus", plus), ("minus", minus))
    ax, outer, n, inner = _perm_gather_check(a, perm, others, axis, nb)
    bits, shape, lead = a.bits, tuple(a.shape), tuple(a.shape[:nb])
    if a.device.type == "meta":
        return empty(shape, bits, a.device)
    if a.device.type == "cuda" and not SHUFFLE_KERNEL:
        return perm_gather_torch(a, perm, b, plus, minus, axis, nb)
    out = empty(shape, bits, a.device)
    if out.data.numel() == 0:
        return out
    dense = outer * n * inner
    ops = [_leaf_operand(t, nb, dense) if t is not None else (None, 0)
           for t in (a, b, plus, minus)]
    pd = perm.contiguous()
    nat.check(
        nat.lib().mx_perm_gather(
            nat.dev_of(out.data), _elem_bytes(bits),
            *[nat.ptr(d) if d is not None else None for d, _ in ops], nat.ptr(pd),
            nat.ptr(out.data), math.prod(lead), *[st for _, st in ops], outer, n, inner,
            nat.stream_of(out.data)),
        "perm_gather",
    )
    return out


# ---------------------------------------------------------------------------
# prefix sums: the plain scan and the stages of a segmented scan
# ---------------------------------------------------------------------------
# the device path of scan, and of segscan_cross / segscan_apply: the native kernels (True) or
# the torch compositions *_torch (False); a CPU tensor always takes the native loops
SCAN_KERNEL = True
SEGSCAN_KERNEL = True
# positions of the axis one lane walks with the running sum in registers (csrc/segscan_geom.h
# kScanChunk, mx_scan_chunk()); a longer axis takes three phases and a workspace
SCAN_CHUNK = 256


class ScanGeom(NamedTuple):
    """A prefix sum along the middle axis of an [outer, n, inner] array
    (csrc/segscan_geom.h): element (o, pos, c) lives at (o*n + pos)*inner + c."""

    outer: int
    n: int
    inner: int
    exclusive: bool = False
    reverse: bool = False


class SegscanGeom(NamedTuple):
    """Stage ``j`` (1 <= j < n, any n) of a segmented Hillis-Steele scan over a state
    [outer, n, inner] whose last column is the continuation flag (csrc/segscan_geom.h)."""

    outer: int
    n: int
    inner: int
    j: int = 1


def segscan_stages(n: int):
    """The offsets j = 1, 2, 4, ... < n of a segmented scan over n positions: ceil(log2 n)."""
    out, j = [], 1
    while j < n:
        out.append(j)
        j *= 2
    return out


def scan_ws_elems(slots: int, outer: int, n: int, inner: int) -> int:
    """Elements of the workspace :func:`scan` hands the native entry (mx_scan_ws_elems): the
    sums and the offsets of every level of chunks, 0 for an axis of one chunk."""
    ws = 0
    while n > SCAN_CHUNK:
        n = -(-n // SCAN_CHUNK)
        ws += 2 * outer * inner * n
    return slots * ws


def _scan_check(what, g, nb, x: RT, others=()):
    bits = x.bits
    if bits not in (64, 128) or any(t.bits != bits for t, _ in others if t is not None):
        raise ValueError(f"{what} is arithmetic only: operands over one of Z_2^64 / Z_2^128")
    if nb not in (0, 1):
        raise ValueError(f"{what} takes at most one batch dim")
    lead = tuple(x.shape[:nb])
    if math.prod(x.shape[nb:]) != g.outer * g.n * g.inner:
        raise ValueError(f"{what}: operand of shape {tuple(x.shape)} does not hold "
                         f"{g.outer} x {g.n} x {g.inner} elements after {nb} batch dims")
    for t, want in others:
        if t is not None and (tuple(t.shape[:nb]) != lead or math.prod(t.shape[nb:]) != want):
            raise ValueError(f"{what}: operand of shape {tuple(t.shape)}, expected {want} "
                             f"elements after the batch dims {lead}")
    return bits, lead


def _scan_geom(g) -> ScanGeom:
    g = ScanGeom(*g)
    g = ScanGeom(int(g.outer), int(g.n), int(g.inner), bool(g.exclusive), bool(g.reverse))
    if g.outer < 0 or g.n < 0 or g.inner < 0:
        raise ValueError(f"scan: malformed geometry {g}")
    return g


def _segscan_geom(what, g) -> SegscanGeom:
    g = SegscanGeom(*(int(v) for v in SegscanGeom(*g)))
    if g.outer < 0 or g.inner < 0 or g.j < 1 or not g.j < g.n:
        raise ValueError(f"{what}: malformed stage {g}")
    return g


def scan_torch(x: RT, g: ScanGeom, nb=0) -> RT:
    """:func:`scan` as a torch composition: ``torch.cumsum`` on the int64 view for Z_2^64 (it
    wraps as the ring does); for Z_2^128, whose two words cumsum cannot carry between,
    Hillis-Steele steps of ``binary("add")`` on slices.  The benchmark's opponent."""
    g = _scan_geom(g)
    bits, lead = _scan_check("scan", g, nb, x)
    if x.data.numel() == 0:
        return RT(x.data.clone(), bits)
    v = reshape(x, (g.outer, g.n, g.inner), nb)
    ax = nb + 1
    if bits == 64:
        d = v.data.flip(ax) if g.reverse else v.data
        c = torch.cumsum(d, dim=ax)
        if g.exclusive:
            c = c - d
        out = RT((c.flip(ax) if g.reverse else c).contiguous(), 64)
    else:
        acc, d, n = v, 1, g.n
        while d < n:
            lo, hi = slice_axis(acc, 1, 0, n - d, nb=nb), slice_axis(acc, 1, d, n, nb=nb)
            s = binary("add", lo, hi)
            if g.reverse:
                acc = concat([s, slice_axis(acc, 1, n - d, n, nb=nb)], 1, nb)
            else:
                acc = concat([slice_axis(acc, 1, 0, d, nb=nb), s], 1, nb)
            d *= 2
        out = binary("sub", acc, v.contiguous()) if g.exclusive else acc
    return reshape(out, x.shape[nb:], nb)


def scan(x: RT, g: ScanGeom, nb=0) -> RT:
    """The prefix sums of ``x`` seen as [.., outer, n, inner] along the middle axis, wrapping
    in the ring, in ``x``'s shape: ``out[o, pos, c]`` is the sum of ``x[o, t, c]`` over ``t <=
    pos`` (``exclusive``: ``t < pos``, the first element 0; ``reverse``: from the far end).
    One native entry over all batch slots (``mx_scan``); a [slots, ...] view with dense slots
    is read in place.  An axis of up to ``SCAN_CHUNK`` positions is one launch; a longer one
    takes the sums of its chunks, their scan and an add pass, in a workspace allocated here."""
    g = _scan_geom(g)
    bits, lead = _scan_check("scan", g, nb, x)
    shape = tuple(x.shape)
    if x.device.type == "meta":  # shape inference of the symbolic session
        return empty(shape, bits, x.device)
    if x.device.type == "cuda" and not SCAN_KERNEL:
        return scan_torch(x, g, nb)
    out = empty(shape, bits, x.device)
    if out.data.numel() == 0:
        return out
    slots = math.prod(lead)
    xd, xst = _leaf_operand(x, nb, g.outer * g.n * g.inner)
    nws = scan_ws_elems(slots, g.outer, g.n, g.inner)
    ws = empty((nws,), bits, x.device) if nws else None
    nat.check(
        nat.lib().mx_scan(nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(xd),
                          nat.ptr(out.data), nat.ptr(ws.data) if nws else None, nws, slots, xst,
                          g.outer, g.n, g.inner, int(g.exclusive), int(g.reverse),
                          nat.stream_of(out.data)),
        "scan",
    )
    return out


def _segscan_flag(t: RT, g: SegscanGeom, nb):
    """The flag column of positions [j, n), [.., outer, n - j, 1], and the state of positions
    [0, n - j), [.., outer, n - j, inner]."""
    v = reshape(t, (g.outer, g.n, g.inner), nb)
    flag = slice_axis(slice_axis(v, 1, g.j, g.n, nb=nb), 2, g.inner - 1, g.inner, nb=nb)
    return flag, slice_axis(v, 1, 0, g.n - g.j, nb=nb)


def segscan_cross_torch(a: RT, b, g: SegscanGeom, nb=0) -> RT:
    """:func:`segscan_cross` as a composition of the existing kernels."""
    g = _segscan_geom("segscan_cross", g)
    _scan_check("segscan_cross", g, nb, a, ((b, g.outer * g.n * g.inner),))
    ga, ta = _segscan_flag(a, g, nb)
    if b is None:
        return binary("mul", ga, ta)
    gb, tb = _segscan_flag(b, g, nb)
    return binary("add", binary("mul", ga, binary("add", ta, tb)), binary("mul", gb, ta))


def segscan_apply_torch(x: RT, p: RT, g: SegscanGeom, nb=0) -> RT:
    """:func:`segscan_apply` as a composition of the existing kernels."""
    g = _segscan_geom("segscan_apply", g)
    _scan_check("segscan_apply", g, nb, x, ((p, g.outer * (g.n - g.j) * g.inner),))
    v = reshape(x, (g.outer, g.n, g.inner), nb)
    pp = reshape(p, (g.outer, g.n - g.j, g.inner), nb)
    tail = slice_axis(pp, 2, g.inner - 1, g.inner, nb=nb)
    if g.inner > 1:
        hi = slice_axis(slice_axis(v, 1, g.j, g.n, nb=nb), 2, 0, g.inner - 1, nb=nb)
        vals = binary("add", hi, slice_axis(pp, 2, 0, g.inner - 1, nb=nb))
        tail = concat([vals, tail], 2, nb)
    out = concat([slice_axis(v, 1, 0, g.j, nb=nb), tail], 1, nb)
    return reshape(out, x.shape[nb:], nb)


def segscan_cross(a: RT, b, g: SegscanGeom, nb=0) -> RT:
    """One party's local products of stage ``g`` of a segmented scan, with its own component
    ``a`` of the state and the next party's ``b``: for ``pos`` in [j, n) and every column,
    ``ga * (Ta + Tb) + gb * Ta`` with ``g*`` the flag column at ``pos`` and ``T*`` the state
    at ``pos - j`` (own times the sum plus next times own, as :func:`cswap_cross`), as
    [.., outer, n - j, inner].  ``b = None``: the plain form ``ga * Ta``.  One native launch
    over all batch slots (``mx_segscan_cross``); the stage travels in its arguments."""
    g = _segscan_geom("segscan_cross", g)
    bits, lead = _scan_check("segscan_cross", g, nb, a, ((b, g.outer * g.n * g.inner),))
    shape = lead + (g.outer, g.n - g.j, g.inner)
    if a.device.type == "meta":
        return empty(shape, bits, a.device)
    if a.device.type == "cuda" and not SEGSCAN_KERNEL:
        return segscan_cross_torch(a, b, g, nb)
    out = empty(shape, bits, a.device)
    if out.data.numel() == 0:
        return out
    nx = g.outer * g.n * g.inner
    ad, st = _leaf_operand(a, nb, nx)
    bd = None
    if b is not None:
        bd, bst = _leaf_operand(b, nb, nx)
        ad, bd, st = _leaf_pair(ad, st, bd, bst, nx)
    nat.check(
        nat.lib().mx_segscan_cross(nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(ad),
                                   nat.ptr(bd) if bd is not None else None, nat.ptr(out.data),
                                   math.prod(lead), st, g.outer, g.n, g.inner, g.j,
                                   nat.stream_of(out.data)),
        "segscan_cross",
    )
    return out


def segscan_apply(x: RT, p: RT, g: SegscanGeom, nb=0) -> RT:
    """The update of stage ``g``: from position j on, the value columns of the state ``x`` take
    the products ``p`` [.., outer, n - j, inner] of position ``pos - j`` and the flag column is
    replaced by its product; positions below j are copied.  In ``x``'s shape.  One native
    launch over all batch slots (``mx_segscan_apply``)."""
    g = _segscan_geom("segscan_apply", g)
    bits, lead = _scan_check("segscan_apply", g, nb, x,
                             ((p, g.outer * (g.n - g.j) * g.inner),))
    shape = tuple(x.shape)
    if x.device.type == "meta":
        return empty(shape, bits, x.device)
    if x.device.type == "cuda" and not SEGSCAN_KERNEL:
        return segscan_apply_torch(x, p, g, nb)
    out = empty(shape, bits, x.device)
    if out.data.numel() == 0:
        return out
    xd, xst = _leaf_operand(x, nb, g.outer * g.n * g.inner)
    pd, pst = _leaf_operand(p, nb, g.outer * (g.n - g.j) * g.inner)
    nat.check(
        nat.lib().mx_segscan_apply(nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(xd),
                                   nat.ptr(pd), nat.ptr(out.data), math.prod(lead), xst, pst,
                                   g.outer, g.n, g.inner, g.j, nat.stream_of(out.data)),
        "segscan_apply",
    )
    return out


# ---------------------------------------------------------------------------
# row-wise outer products: a level of a demultiplexer
# ---------------------------------------------------------------------------
# the device path of outer_cross: the native kernel (True) or the torch composition
# outer_cross_torch (False); a CPU tensor always takes the native loops
OUTER_KERNEL = True


class OuterGeom(NamedTuple):
    """Row-wise outer products (csrc/outer_geom.h): ``L`` is [groups, rows, A], ``H`` is
    [groups, rows, B] and the output [groups, rows, n_out] holds ``L[.., c % A] * H[.., c // A]``
    at column c; A, B >= 1 and 1 <= n_out <= A * B."""

    groups: int
    rows: int
    A: int
    B: int
    n_out: int


def _outer_geom(g) -> OuterGeom:
    g = OuterGeom(*(int(v) for v in OuterGeom(*g)))
    if g.groups < 0 or g.rows < 0 or g.A < 1 or g.B < 1 or not 1 <= g.n_out <= g.A * g.B:
        raise ValueError(f"outer_cross: malformed geometry {g}")
    return g


def _outer_check(g, nb, la: RT, lb, ha: RT, hb):
    bits = la.bits
    if bits not in (64, 128) or any(t is not None and t.bits != bits for t in (lb, ha, hb)):
        raise ValueError("outer_cross is arithmetic only: operands over one of Z_2^64 / Z_2^128")
    if nb not in (0, 1):
        raise ValueError("outer_cross takes at most one batch dim")
    if (lb is None) != (hb is None):
        raise ValueError("outer_cross takes the next components of both operands or of neither")
    lead = tuple(la.shape[:nb])
    for t, x in ((la, g.A), (lb, g.A), (ha, g.B), (hb, g.B)):
        if t is not None and (tuple(t.shape[:nb]) != lead
                              or tuple(t.shape[nb:]) != (g.groups, g.rows, x)):
            raise ValueError(f"outer_cross: operand of shape {tuple(t.shape)}, expected "
                             f"{lead + (g.groups, g.rows, x)}")
    return bits, lead


def _outer_operand(t: RT, nb, groups, rows, x):
    """(data, slot stride, group stride in elements) of an operand [slots?, groups, rows, x]: a
    view whose rows are dense within a group is read in place at its own strides (the even or
    odd groups of a wider array, the slot views of a share-pair buffer), anything else as a
    contiguous copy."""
    d, w = t.data, 2 if t.bits == 128 else 1
    dense = (groups * rows * x, rows * x)
    if d.numel() and d[(0,) * (nb + 1)].is_contiguous():
        st = (d.stride(0) if nb and d.shape[0] > 1 else dense[0] * w,
              d.stride(nb) if groups > 1 else dense[1] * w)
        if all(s >= 0 and s % w == 0 for s in st):
            return d, st[0] // w, st[1] // w
    return d.contiguous(), dense[0], dense[1]


def _outer_component_pair(a, b, nb, groups, rows, x):
    """Both components of one operand at one pair of strides: as they are when their strides
    agree, else both dense."""
    ad, ast, agr = _outer_operand(a, nb, groups, rows, x)
    if b is None:
        return ad, None, ast, agr
    bd, bst, bgr = _outer_operand(b, nb, groups, rows, x)
    if (ast, agr) != (bst, bgr):
        ad, bd, ast, agr = ad.contiguous(), bd.contiguous(), groups * rows * x, rows * x
    return ad, bd, ast, agr


def outer_pairs(x: RT, nb=0):
    """The groups (2g, 2g + 1) of ``x`` [.., G, rows, A] as two uncopied views ``(L, H)`` of
    [.., G // 2, rows, A]: ``H = L + rows * A`` at a group stride of ``2 * rows * A``.  An odd
    last group belongs to neither."""
    G = x.shape[nb]
    idx = (slice(None),) * nb
    return (RT(x.data[idx + (slice(0, G - G % 2, 2),)], x.bits),
            RT(x.data[idx + (slice(1, G, 2),)], x.bits))


def outer_cross_torch(la: RT, lb, ha: RT, hb, g: OuterGeom, nb=0) -> RT:
    """:func:`outer_cross` as a composition of the existing kernels: broadcast products over a
    [.., groups, rows, B, A] buffer, trimmed to ``n_out`` columns.  The benchmark's opponent."""
    g = _outer_geom(g)
    _outer_check(g, nb, la, lb, ha, hb)

    wide = (g.groups, g.rows, g.B, g.A)

    def col(t):
        return broadcast_to(reshape(t.contiguous(), (g.groups, g.rows, 1, g.A), nb), wide, nb)

    def row(t):
        return broadcast_to(reshape(t.contiguous(), (g.groups, g.rows, g.B, 1), nb), wide, nb)

    if lb is None:
        v = binary("mul", col(la), row(ha))
    else:
        v = binary("add", binary("mul", col(la), row(binary("add", ha.contiguous(),
                                                            hb.contiguous()))),
                   binary("mul", col(lb), row(ha)))
    v = reshape(v, (g.groups, g.rows, g.A * g.B), nb)
    return v if g.n_out == g.A * g.B else slice_axis(v, 2, 0, g.n_out, nb=nb)


def outer_cross(la: RT, lb, ha: RT, hb, g: OuterGeom, nb=0) -> RT:
    """Row-wise outer products of ``L`` [.., groups, rows, A] and ``H`` [.., groups, rows, B]:
    ``out[.., c] = L[.., c % A] * H[.., c // A]`` for ``c < n_out``, as [.., groups, rows,
    n_out] -- one level of a demultiplexer tree, whose one-hot groups of A and B entries become
    one of A * B (the last level trims to ``n_out``).  With the next party's components ``lb``
    and ``hb`` it is one party's local products of a replicated multiplication, ``La * (Ha +
    Hb) + Lb * Ha`` (as :func:`segscan_cross`); ``lb = hb = None`` is the plain product.  One
    native launch over all batch slots (``mx_outer_cross``); ``L`` and ``H`` go to the entry at
    their own slot and group strides, so the views of :func:`outer_pairs` and the slot views
    of a share-pair buffer are read in place."""
    g = _outer_geom(g)
    bits, lead = _outer_check(g, nb, la, lb, ha, hb)
    shape = lead + (g.groups, g.rows, g.n_out)
    if la.device.type == "meta":
        return empty(shape, bits, la.device)
    if la.device.type == "cuda" and not OUTER_KERNEL:
        return outer_cross_torch(la, lb, ha, hb, g, nb)
    out = empty(shape, bits, la.device)
    if out.data.numel() == 0:
        return out
    lad, lbd, lst, lgr = _outer_component_pair(la, lb, nb, g.groups, g.rows, g.A)
    had, hbd, hst, hgr = _outer_component_pair(ha, hb, nb, g.groups, g.rows, g.B)
    nat.check(
        nat.lib().mx_outer_cross(nat.dev_of(out.data), _elem_bytes(bits), nat.ptr(lad),
                                 nat.ptr(lbd) if lbd is not None else None, nat.ptr(had),
                                 nat.ptr(hbd) if hbd is not None else None, nat.ptr(out.data),
                                 math.prod(lead), lst, lgr, hst, hgr, g.groups, g.rows, g.A, g.B,
                                 g.n_out, nat.stream_of(out.data)),
        "outer_cross",
    )
    return out


def select_mask(a: RT, axis: int, mask: torch.Tensor, nb=0) -> RT:
    ax = _ax(a, axis, nb)
    keep = torch.nonzero(mask.reshape(-1).to(torch.bool)).reshape(-1).to(a.device)
    return RT(a.data.index_select(ax, keep).contiguous(), a.bits)


def diag(a: RT, nb=0) -> RT:
    d = a.data
    if a.bits == 128:
        return RT(torch.diagonal(d, dim1=nb, dim2=nb + 1).movedim(-1, -2).contiguous(), 128)
    return RT(torch.diagonal(d, dim1=nb, dim2=nb + 1).contiguous(), a.bits)


def broadcast_to(a: RT, shape, nb=0) -> RT:
    shape = tuple(shape)
    lead = len(shape) - (a.ndim - nb)
    if lead > 0:  # numpy rule: missing dims are prepended (after the batch axes)
        a = reshape(a, (1,) * lead + a.shape[nb:], nb)
    return expand(a, a.shape[:nb] + shape).contiguous()


def atleast_2d(a: RT, to_column_vector=False, nb=0) -> RT:
    nd = a.ndim - nb
    if nd >= 2:
        return a
    if nd == 0:
        return reshape(a, (1, 1), nb)
    n = a.shape[nb]
    return reshape(a, (n, 1) if to_column_vector else (1, n), nb)


# ---------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------
def sum(a: RT, axis=None, nb=0) -> RT:  # noqa: A001 - mirrors the Moose op name
    if axis is None:
        # reduce all logical dims
        flat = reshape(a, (a.numel() // max(1, math.prod(a.shape[:nb])),), nb)
        return sum(flat, 0, nb)
    ax = _ax(a, axis, nb)
    if a.bits == 1:
        return RT((a.data.to(torch.int64).sum(dim=ax) & 1).to(torch.uint8), 1)
    if a.bits == 64:
        return RT(a.data.sum(dim=ax), 64)
    shape = a.shape
    outer = math.prod(shape[:ax])
    red = shape[ax]
    inner = math.prod(shape[ax + 1 :])
    out = empty(shape[:ax] + shape[ax + 1 :], 128, a.device)
    ad = a.data.contiguous()
    nat.check(
        nat.lib().mx_sum_axis(
            nat.dev_of(ad), 2, nat.ptr(ad), nat.ptr(out.data), outer, red, inner,
            nat.stream_of(ad),
        ),
        "ring128 sum",
    )
    return out


def add_n(xs: List[RT]) -> RT:
    acc = xs[0]
    for x in xs[1:]:
        acc = acc + x
    return acc


# ---------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------
def _gemm_call(bits, batch, M, N, K, a0, a1, b0, b1, mode, out, accumulate=0):
    lib = nat.lib()
    limit = (16384 if bits == 64 else 8192) // (2 if mode else 1)
    if out.is_cuda and K > limit:
        # split K so every limb diagonal stays exact in the i32 accumulators
        for k0 in range(0, K, limit):
            k1 = min(K, k0 + limit)
            A0c = _kslice_rows(a0, batch, M, K, k0, k1, bits)
            A1c = _kslice_rows(a1, batch, M, K, k0, k1, bits) if a1 is not None else None
            B0c = _kslice_cols(b0, batch, K, N, k0, k1, bits)
            B1c = _kslice_cols(b1, batch, K, N, k0, k1, bits) if b1 is not None else None
            _gemm_call(bits, batch, M, N, k1 - k0, A0c, A1c, B0c, B1c, mode, out,
                       accumulate if k0 == 0 else 1)
        return
    nat.check(
        lib.mx_gemm(
            nat.dev_of(out), _words(bits), batch, M, N, K, nat.ptr(a0), nat.ptr(a1), nat.ptr(b0),
            nat.ptr(b1), mode, nat.ptr(out), accumulate, nat.stream_of(out),
        ),
        "ring gemm",
    )


def dot_slots(x: RT, c: RT):
    """x[b] . c for every slot b of a device ring tensor x [B, M, K] (or [B, K]) whose slots
    may be any evenly strided views (e.g. the four slots of a share-pair ring buffer) and a
    public operand c [K, N] (or [K]) read by every slot in place -- one launch, no copy of
    c per slot.  None when the layout does not fit (the caller runs R.dot)."""
    d, cd = x.data, c.data
    if (not d.is_cuda or cd.device != d.device or x.bits not in (64, 128)
            or c.bits != x.bits):
        return None
    el = 2 if x.bits == 128 else 1
    xl, cl = tuple(x.shape[1:]), tuple(c.shape)
    if len(xl) == 2 and len(cl) == 2:
        M, K, N, oshape = xl[0], xl[1], cl[1], (xl[0], cl[1])
    elif len(xl) == 2 and len(cl) == 1:
        M, K, N, oshape = xl[0], xl[1], 1, (xl[0],)
    elif len(xl) == 1 and len(cl) == 2:
        M, K, N, oshape = 1, xl[0], cl[1], (cl[1],)
    else:
        return None
    if cl[0] != K or d.stride(0) % el:
        return None
    inner = d[0]
    if not inner.is_contiguous() or not cd.is_contiguous():
        return None
    B = d.shape[0]
    out = empty((B,) + oshape, x.bits, d.device)
    nat.check(nat.lib().mxh_gemm_bs(_words(x.bits), B, M, N, K, nat.ptr(d), d.stride(0) // el,
                                    nat.ptr(cd), 0, nat.ptr(out.data), nat.stream_of(d)),
              "ring gemm (slots)")
    return out


def _kslice_rows(t, batch, M, K, k0, k1, bits):
    v = t.reshape(batch, M, K, -1) if bits == 128 else t.reshape(batch, M, K)
    return v[:, :, k0:k1].contiguous()


def _kslice_cols(t, batch, K, N, k0, k1, bits):
    v = t.reshape(batch, K, N, -1) if bits == 128 else t.reshape(batch, K, N)
    return v[:, k0:k1].contiguous()


def _dot_shapes(xs, ys, nb):
    """Normalise rank-1/2 operands to [batch, M, K] x [batch, K, N]."""
    xl, yl = xs[nb:], ys[nb:]
    bshape = xs[:nb]
    if len(xl) == 1 and len(yl) == 1:
        M, K, N = 1, xl[0], 1
        out = ()
    elif len(xl) == 1:
        M, K, N = 1, xl[0], yl[1]
        out = (N,)
    elif len(yl) == 1:
        M, K, N = xl[0], xl[1], 1
        out = (M,)
    else:
        M, K, N = xl[0], xl[1], yl[1]
        out = (M, N)
    if K != (yl[0]):
        raise ValueError(f"dot shape mismatch {xl} . {yl}")
    return bshape, M, K, N, out


def dot(x: RT, y: RT, nb=0) -> RT:
    """Ring matrix product (np.dot semantics for logical ranks 1/2), batched over nb dims."""
    bits = x.bits
    bshape, M, K, N, oshape = _dot_shapes(x.shape, y.shape, nb)
    batch = math.prod(bshape)
    out = empty(bshape + (M, N), bits, x.device)
    if bits == 1:
        r = (x.data.reshape(batch, M, K).to(torch.int64) @ y.data.reshape(batch, K, N).to(torch.int64)) & 1
        return RT(r.to(torch.uint8).reshape(bshape + oshape), 1)
    a0 = x.data.contiguous()
    b0 = y.data.contiguous()
    _gemm_call(bits, batch, M, N, K, a0, None, b0, None, 0, out.data)
    return reshape(out, oshape, nb) if oshape != (M, N) else out


class PreparedCross:
    """The B' = [y0 + y1; y0] operand of a stacked RSS cross GEMM, limb-split once on the
    device (mx_gemm_prep_b) so that several row blocks of x reuse it (dot_cross_rows).  On
    the host, or when K is too long for one exact chunk, it just keeps y0, y1."""

    def __init__(self, y0: RT, y1: RT):
        self.y0, self.y1, self.bits = y0, y1, y0.bits
        self.batch, self.K, self.N = y0.shape[0], y0.shape[1], y0.shape[2]
        self.lb = None
        if y0.data.is_cuda:
            w = _words(self.bits)
            nbytes = nat.lib().mx_gemm_b_bytes(w, self.batch, self.N, self.K, 1)
            if nbytes > 0:
                d0, d1 = y0.data.contiguous(), y1.data.contiguous()
                self.lb = torch.empty(nbytes, dtype=torch.uint8, device=d0.device)
                nat.check(nat.lib().mx_gemm_prep_b(
                    w, self.batch, self.K, self.N, nat.ptr(d0), nat.ptr(d1), 1,
                    nat.ptr(self.lb), nat.stream_of(d0)), "gemm_prep_b")


def dot_cross_rows(x0: RT, x1: RT, r0: int, r1: int, pb: PreparedCross) -> RT:
    """Rows [r0, r1) of the stacked cross GEMM x0.(y0+y1) + x1.y0 for x* [batch, M, K]
    (no copy of the row block on the device)."""
    if pb.lb is None:
        rows = lambda t: RT(t.data[:, r0:r1], t.bits)  # noqa: E731
        return dot_cross(rows(x0), rows(x1), pb.y0, pb.y1, nb=1)
    batch, M, K = x0.shape
    d0, d1 = x0.data, x1.data
    if not (d0.is_contiguous() and d1.is_contiguous()):
        d0, d1 = d0.contiguous(), d1.contiguous()
    el = 2 if pb.bits == 128 else 1  # int64 words per element
    out = empty((batch, r1 - r0, pb.N), pb.bits, d0.device)
    off = r0 * K * el * 8
    nat.check(nat.lib().mx_gemm_with_b(
        _words(pb.bits), batch, r1 - r0, pb.N, K, ctypes.c_void_p(d0.data_ptr() + off),
        ctypes.c_void_p(d1.data_ptr() + off), M * K, 1,
        nat.ptr(pb.lb), nat.ptr(out.data), 0, nat.stream_of(d0)), "gemm_with_b")
    return out


def dot_cross_pair(x0: RT, y0: RT, y1: RT, roll: int, pb: PreparedCross = None, r0=0,
                   r1=None):
    """dot_cross(x0, x1, y0, y1) for a stacked RSS pair whose second share is the first
    rolled over the flattened batch (x1[b] = x0[(b + roll) % batch]): the CRT GEMM prepares
    each share's residues once and reads them for both K halves.  Rows [r0, r1) of x0 only
    when given.  None when the device path does not apply (the caller runs dot_cross)."""
    d0 = x0.data
    if not d0.is_cuda or len(x0.shape) != 3:
        return None
    if not d0.is_contiguous():
        d0 = d0.contiguous()
    batch, M, K = x0.shape
    r1 = M if r1 is None else r1
    bits = x0.bits
    el = 2 if bits == 128 else 1
    if pb is not None:
        if pb.lb is None:
            return None
        N, lb, b0, b1 = pb.N, nat.ptr(pb.lb), None, None
    else:
        # [batch, K, N] right operands only (a stacked secret vector [batch, K] takes the
        # generic dot_cross path, which handles rank-1 operands)
        if (len(y0.shape) != 3 or tuple(y1.shape) != tuple(y0.shape)
                or y0.shape[0] != batch or y0.shape[1] != K):
            return None
        N = y0.shape[2]
        b0, b1 = y0.data.contiguous(), y1.data.contiguous()
        lb = None
    out = empty((batch, r1 - r0, N), bits, d0.device)
    rc = nat.lib().mx_gemm_roll(
        _words(bits), batch, r1 - r0, N, K, ctypes.c_void_p(d0.data_ptr() + r0 * K * el * 8),
        M * K, roll, None if b0 is None else nat.ptr(b0), None if b1 is None else nat.ptr(b1),
        lb, nat.ptr(out.data), 0, nat.stream_of(d0))
    if rc == -7:
        return None
    nat.check(rc, "gemm_roll")
    return out


def _asym_operands(x0: RT, x1: RT, y0: RT, y1: RT):
    """Stacks (A0, A1, B0, B1) whose mode-1 cross GEMM A0.(B0 + B1) + A1.B0 is the
    asymmetric z_p of dot_cross_asym, per party p with (a, b, c, d) = (x0, x1, y0, y1)[p]:
    (a + b, 0, c, d), (b, a, d, c), (a, b, c, d - c)."""
    def at(t, p):
        return RT(t.data[p], t.bits)

    a, b, c, d = ([at(t, p) for p in range(3)] for t in (x0, x1, y0, y1))
    zero = zeros(tuple(x0.shape[1:]), x0.bits, x0.device)
    stk = lambda ts: RT(torch.stack([t.data for t in ts]), x0.bits)  # noqa: E731
    A0 = stk([binary("add", a[0], b[0]), b[1], a[2]])
    A1 = stk([zero, a[1], b[2]])
    B0 = stk([c[0], d[1], c[2]])
    B1 = stk([d[0], c[1], binary("sub", d[2], c[2])])
    return A0, A1, B0, B1


_DEFER = threading.local()


@contextmanager
def deferred_products(on: bool = True):
    """Within the block, dot_cross_asym / dot_cross_asym_src may return their product as a
    :class:`CrtProduct` (the caller is a tail that waits for its first reader)."""
    prev = getattr(_DEFER, "on", False)
    _DEFER.on = bool(on)
    try:
        yield
    finally:
        _DEFER.on = prev


def _defer_residues(bits: int, M: int, N: int, K: int, device):
    """The residue buffer of a deferred M x N x K product, or None where products are not
    deferred (outside deferred_products, or the native form declines the layout or sizes)."""
    if not getattr(_DEFER, "on", False):
        return None
    nbytes = nat.lib().mx_crt_defer_bytes(_words(bits), M, N, K)
    if nbytes < 0:
        return None
    return torch.empty(nbytes, dtype=torch.int8, device=device)


def dot_cross_asym(x0: RT, x1: RT, y0: RT, y1: RT, rolled: bool = False) -> RT:
    """The three parties' local products of a replicated matrix product, in the asymmetric
    form (x0/x1: [3, M, K] first/second share stacks, y0/y1: [3, K, N]).  With party p
    holding (a, b) = (x_p, x_{p+1}), (c, d) = (y_p, y_{p+1}):

        z_0 = (a + b)(c + d),   z_1 = b (c + d) + a d,   z_2 = a d + b c.

    Every x_i y_j appears exactly once over the three parties, so sum_p z_p = x.y as in the
    symmetric form z_p = a (c + d) + b c (Araki et al.; the reference's
    replicated/arith.rs:436-492), and each z_p is a function of party p's own shares only.
    Party 0's product is one K-long GEMM instead of two: five K-long GEMMs per product
    instead of six.  The zero share added before the reshare masks z_p exactly as before.
    On the device the five run as one CRT GEMM launch (mx_gemm_asym; ``rolled``: x1/y1 are
    x0/y0 rolled by one party, so x_2's residues are shared by parties 1 and 2); elsewhere
    the same z_p by the generic cross GEMM of rearranged operands (_asym_operands)."""
    bits = x0.bits
    M, K = x0.shape[1], x0.shape[2]
    N = y0.shape[2]
    d = x0.data
    if d.is_cuda and bits in (64, 128) and x0.shape[0] == 3 and y0.shape[0] == 3:
        ts = [t.data if t is not None else None for t in (x0, x1, y0, y1)]
        if rolled:
            ts[1] = ts[3] = None
        if all(t is None or t.is_contiguous() for t in ts):
            res = _defer_residues(bits, M, N, K, d.device)
            out = empty((3, M, N), bits, d.device) if res is None else None
            rc = nat.lib().mx_gemm_asym(
                _words(bits), M, N, K, nat.ptr(ts[0]), None if ts[1] is None else nat.ptr(ts[1]),
                nat.ptr(ts[2]), None if ts[3] is None else nat.ptr(ts[3]), 1 if rolled else 0,
                None if out is None else nat.ptr(out.data), nat.stream_of(d), nat.ptr(res))
            if rc != -7:
                nat.check(rc, "gemm_asym")
                return out if res is None else CrtProduct(res, M, N, K, bits)
    if x1 is None or y1 is None:
        x1 = RT(torch.roll(x0.data, -1, dims=0), bits)
        y1 = RT(torch.roll(y0.data, -1, dims=0), bits)
    A0, A1, B0, B1 = _asym_operands(x0, x1, y0, y1)
    return dot_cross(A0, A1, B0, B1, nb=1)


def dot_cross_asym_src(x0, y0, xsrc, ysrc, M: int, K: int, N: int):
    """dot_cross_asym over Z_2^128 (rolled) with one or both operands still the plain input
    of their sharing: ``xsrc`` / ``ysrc`` is None (then ``x0`` / ``y0`` is the [3, ..] share
    stack) or the arguments of the mx_share3_k launch that would write the stack -- (kind
    code | SHARE_MIRROR, plain device tensor, fractional bits, owner slot, key slot, nonce).
    The operand prep shares such an input in registers (mx_gemm_asym_src); the product is
    bitwise that of the written shares.  None when the native form does not apply (nothing
    has run: the caller writes the shares and takes dot_cross_asym)."""
    ts = [None if t is None else t.data for t in (x0, y0)]
    if any(t is not None and not t.is_contiguous() for t in ts):
        return None
    words = []
    for s in (xsrc, ysrc):
        if s is None:
            words.append(None)
            continue
        code, d, frac, j0, slot, nonce = s
        if not d.is_cuda or not d.is_contiguous():
            return None
        words.append((ctypes.c_int64 * 6)(d.data_ptr(), code, int(frac or 0), j0, int(slot),
                                          _i64(nonce)))
    anyt = next(s[1] for s in (xsrc, ysrc) if s is not None)
    res = _defer_residues(128, M, N, K, anyt.device)
    out = empty((3, M, N), 128, anyt.device) if res is None else None
    rc = nat.lib().mx_gemm_asym_src(2, M, N, K, nat.ptr(ts[0]), nat.ptr(ts[1]), words[0],
                                    words[1], None if out is None else nat.ptr(out.data),
                                    nat.stream_of(anyt), nat.ptr(res))
    if rc == -7:
        return None
    nat.check(rc, "gemm_asym_src")
    return out if res is None else CrtProduct(res, M, N, K, 128)


def _i64(v: int) -> int:
    """A 64-bit pattern as the signed value ctypes' c_int64 takes."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _party_batch_strides(t: RT):
    """(party stride, batch stride) in ring elements of a [P, B, *inner] device tensor whose
    inner dims are contiguous (e.g. an expanded, stride-0 stack of one operand); None if
    the layout is anything else."""
    d = t.data
    el = 2 if t.bits == 128 else 1
    if d.dim() < 3:
        return None
    expect = 1
    for size, st in zip(reversed(d.shape[2:]), reversed(d.stride()[2:])):
        if size != 1 and st != expect:
            return None
        expect *= size
    if d.stride(0) % el or d.stride(1) % el:
        return None
    return d.stride(0) // el, d.stride(1) // el


def _dot_cross_strided(x0, x1, y0, y1, out, M, K, N):
    """Per-party strided GEMMs for [3, B, M, K] x [3, B, K, N] operands that are views
    (no copy of an expanded stack).  False when the layout does not allow it."""
    bits = x0.bits
    limit = (16384 if bits == 64 else 8192) // 2
    if not out.data.is_cuda or K > limit:
        return False
    st = [_party_batch_strides(t) for t in (x0, x1, y0, y1)]
    if any(s is None for s in st) or st[0][1] != st[1][1] or st[2][1] != st[3][1]:
        return False
    eb = 16 if bits == 128 else 8
    B = out.shape[1]
    lib = nat.lib()
    for p in range(out.shape[0]):
        def at(t, s):
            return ctypes.c_void_p(t.data.data_ptr() + p * s[0] * eb)
        optr = ctypes.c_void_p(out.data.data_ptr() + p * B * M * N * eb)
        nat.check(lib.mx_gemm_strided(_words(bits), B, M, N, K, at(x0, st[0]), at(x1, st[1]),
                                      st[0][1], at(y0, st[2]), at(y1, st[3]), st[2][1], 1, optr,
                                      0, nat.stream_of(out.data)), "gemm_strided")
    return True


def dot_cross(x0: RT, x1: RT, y0: RT, y1: RT, nb=0) -> RT:
    """RSS cross terms of a matrix product: x0.(y0+y1) + x1.y0 in one K-doubled GEMM."""
    bits = x0.bits
    bshape, M, K, N, oshape = _dot_shapes(x0.shape, y0.shape, nb)
    batch = math.prod(bshape)
    out = empty(bshape + (M, N), bits, x0.device)
    if (nb == 2 and oshape == (M, N) and not all(
            t.data.is_contiguous() for t in (x0, x1, y0, y1))
            and _dot_cross_strided(x0, x1, y0, y1, out, M, K, N)):
        return out
    _gemm_call(
        bits, batch, M, N, K, x0.data.contiguous(), x1.data.contiguous(), y0.data.contiguous(),
        y1.data.contiguous(), 1, out.data,
    )
    return reshape(out, oshape, nb) if oshape != (M, N) else out


# ---------------------------------------------------------------------------
# randomness (AES-128-CTR)
# ---------------------------------------------------------------------------
def prf_expand(keys: Sequence[bytes], nonce: int, shape, bits, device) -> RT:
    """out[p] = PRF(keys[p], nonce) of the given logical shape; stacked over keys."""
    shape = tuple(shape)
    n = math.prod(shape)
    out = empty((len(keys),) + shape, bits, device)
    kb = nat.key_buffer(keys)
    if len(keys) > 4:
        raise ValueError("at most 4 keys per call")
    nat.check(
        nat.lib().mx_prf_expand(
            nat.dev_of(out.data), _words(bits), nat.ptr(out.data), n, len(keys), kb,
            nonce & MASK64, nat.stream_of(out.data),
        ),
        "prf_expand",
    )
    return out


def bit_planes(a: RT, start: int, count: int, nb=0) -> RT:
    """Bits start..start+count-1 of ``a`` as a bit tensor with a new logical leading axis
    (after ``nb`` batch axes): out[.., j, ..] = bit start+j.  One kernel."""
    shp = a.shape
    outer = math.prod(shp[:nb])
    inner = math.prod(shp[nb:])
    out = torch.empty(tuple(shp[:nb]) + (count,) + tuple(shp[nb:]), dtype=torch.uint8,
                      device=a.device)
    ad = a.data.contiguous()
    nat.check(nat.lib().mx_bit_planes(nat.dev_of(ad), _words(a.bits), nat.ptr(ad), nat.ptr(out),
                                      outer, inner, start, count, nat.stream_of(ad)),
              "bit_planes")
    return RT(out, 1)


_WEIGHTS = {}


_CONSTS = {}


def const_ints(values, bits, device) -> RT:
    """A public constant vector of python ints on ``device``, made once per (values, bits,
    device) and shared -- callers never write into it (no upload per evaluation; not
    cached while a hipGraph is being captured: it would live in the graph's pool)."""
    key = (tuple(int(v) for v in values), bits, str(device))
    hit = _CONSTS.get(key)
    if hit is not None:
        return hit
    t = from_ints(np.array(list(key[0]), dtype=object), bits, device)
    if torch.device(device).type == "cpu" or not torch.cuda.is_current_stream_capturing():
        _cache_put(_CONSTS, key, t, 4096)
        if _CONSTS.get(key) is t:  # only what the cache keeps (it is bounded)
            _const_key[id(t)] = key
    return t


_const_key = {}  # id of a cached constant -> its _CONSTS key (constants are never freed)


_LEADING = {}


def mul_leading(a: RT, c: RT, nb: int) -> RT:
    """a[.., i, ..] * c[i] along the first non-batch axis of ``a``: the public vector
    broadcast to a's shape is made once per (constant, shape) when ``c`` is a shared
    constant (const_ints), so an evaluation runs one multiply kernel and no copy."""
    k = len(a.shape) - nb - 1
    cb = reshape(c, (c.shape[0],) + (1,) * k)
    shared = c.data.is_cuda and _CONSTS.get(_const_key.get(id(c))) is c
    if not shared:
        return binary("mul", a, cb)
    key = (id(c), tuple(a.shape))
    full = _LEADING.get(key)
    if full is None:
        full = RT(expand(cb, tuple(a.shape)).data.contiguous(), a.bits)
        if not torch.cuda.is_current_stream_capturing():
            _cache_put(_LEADING, key, full, 1024)
    return binary("mul", a, full)


def mul_leading_add2(a0: RT, a1: RT, c: RT, cadd: RT, add0: bool, add1: bool):
    """One party's two share components scaled by the public vector ``c`` along the leading
    axis (mul_leading, nb = 1) plus the public scalar ``cadd`` on the components flagged
    ``add0`` / ``add1`` (add_public on this party's copies of x_0), one launch
    (mx_mul_add2).  None when the operands do not fit (then the caller runs the steps)."""
    if not (a0.bits in (64, 128) and a1.bits == a0.bits and a1.shape == a0.shape
            and isinstance(cadd, RT) and cadd.bits == a0.bits and cadd.numel() == 1
            and c.bits == a0.bits and len(a0.shape) >= 1 and c.numel() == a0.shape[0]):
        return None
    k = len(a0.shape) - 1
    # the broadcast is cached only for a shared constant (its id stays its own)
    shared = _CONSTS.get(_const_key.get(id(c))) is c
    key = (id(c), tuple(a0.shape), "pair")
    full = _LEADING.get(key) if shared else None
    if full is None:
        full = RT(expand(reshape(c, (c.shape[0],) + (1,) * k), tuple(a0.shape)).data
                  .contiguous(), a0.bits)
        if shared and not (a0.data.is_cuda and torch.cuda.is_current_stream_capturing()):
            _cache_put(_LEADING, key, full, 1024)
    d0, d1 = a0.data.contiguous(), a1.data.contiguous()
    cd = cadd.data.contiguous()
    if cd.device != d0.device:
        cd = cd.to(d0.device)
    o0, o1 = empty2(a0.shape, a0.bits, a0.device)
    nat.check(nat.lib().mx_mul_add2(
        nat.dev_of(d0), _words(a0.bits), nat.ptr(d0), nat.ptr(d1), nat.ptr(full.data),
        nat.ptr(cd), int(bool(add0)), int(bool(add1)), nat.ptr(o0.data), nat.ptr(o1.data),
        a0.numel(), nat.stream_of(d0)), "mul_add2")
    return o0, o1


def mul_leading_add(a: RT, c: RT, nb: int, cadd: RT, rows) -> RT:
    """mul_leading(a, c, nb) plus the public scalar ``cadd`` on batch rows ``rows`` (two of
    a's leading axis) in one launch (k_mul_rows_add); None when mul_leading would not use a
    cached broadcast (then the caller runs the two steps)."""
    if not (a.data.is_cuda and a.bits in (64, 128) and nb == 1 and isinstance(cadd, RT)
            and cadd.bits == a.bits and cadd.numel() == 1):
        return None
    if not (c.data.is_cuda and _CONSTS.get(_const_key.get(id(c))) is c):
        return None
    k = len(a.shape) - nb - 1
    cb = reshape(c, (c.shape[0],) + (1,) * k)
    key = (id(c), tuple(a.shape))
    full = _LEADING.get(key)
    if full is None:
        full = RT(expand(cb, tuple(a.shape)).data.contiguous(), a.bits)
        if not torch.cuda.is_current_stream_capturing():
            _cache_put(_LEADING, key, full, 1024)
    ad = a.data.contiguous()
    cd = cadd.data.contiguous()
    if cd.device != ad.device:
        cd = cd.to(ad.device)
    out = empty(a.shape, a.bits, a.device)
    n = a.numel()
    nat.check(nat.lib().mxh_mul_rows_add(_words(a.bits), nat.ptr(ad), nat.ptr(full.data),
                                         nat.ptr(out.data), n, n // a.shape[0], nat.ptr(cd),
                                         int(rows[0]), int(rows[1]), nat.stream_of(ad)),
              "mul_rows_add")
    return out


def weighted_sum(a: RT, weights, nb=0) -> RT:
    """sum_j weights[j] * a[.., j, ..] over the leading logical axis (public integer
    weights, e.g. bit composition).  One kernel."""
    bits = a.bits
    key = (tuple(int(w) for w in weights), bits, str(a.device))
    w = _WEIGHTS.get(key)
    if w is None:
        w = from_ints(np.array([int(v) for v in weights], dtype=object), bits, a.device)
        if a.device.type == "cpu" or not torch.cuda.is_current_stream_capturing():
            _cache_put(_WEIGHTS, key, w, 4096)
    shp = a.shape
    k = shp[nb]
    outer = math.prod(shp[:nb])
    inner = math.prod(shp[nb + 1:])
    out = empty(tuple(shp[:nb]) + tuple(shp[nb + 1:]), bits, a.device)
    ad = a.data.contiguous()
    nat.check(nat.lib().mx_weighted_sum(nat.dev_of(ad), _words(bits), nat.ptr(ad),
                                        nat.ptr(w.data), nat.ptr(out.data), outer, k, inner,
                                        nat.stream_of(ad)), "weighted_sum")
    return out


def prf_expand_k(slot_ptr: int, nkeys: int, nonce: int, shape, bits, device) -> RT:
    """``prf_expand`` with the keys read from ``nkeys`` consecutive key slots."""
    shape = tuple(shape)
    n = math.prod(shape)
    out = empty((nkeys,) + shape, bits, device)
    nat.check(
        nat.lib().mx_prf_expand_k(
            nat.dev_of(out.data), _words(bits), nat.ptr(out.data), n, nkeys,
            ctypes.c_void_p(slot_ptr), nonce & MASK64, nat.stream_of(out.data),
        ),
        "prf_expand_k",
    )
    return out


def ring_extend3_k(s0: RT, slot_k0: int, slot_k2: int, nonces, out=None):
    """Exact widening Z_2^64 -> Z_2^128 of a stacked replicated sharing (slots ``s0``,
    [3, ...]), all three parties in one kernel (csrc/rss_fused.h: ring_extend_z1; valid for
    -2^62 <= x < 2^62).  ``slot_k0`` / ``slot_k2``: addresses of the dealer key slots;
    ``nonces``: r0, r1, R0, M0, z0, z2.  Returns the two share vectors (a ``ring4`` pair
    unless ``out`` = (out0, out1) is given)."""
    if s0.bits != 64 or not s0.shape or s0.shape[0] != 3:
        raise TypeError("ring_extend3_k: expects stacked [3, ...] Z_2^64 slots")
    d = s0.data.contiguous()
    n = d.numel() // 3
    out0, out1 = out if out is not None else ring4(s0.shape, 128, d.device)
    nn = (ctypes.c_uint64 * 6)(*[int(v) & MASK64 for v in nonces])
    nat.check(
        nat.lib().mx_ring_extend3_k(
            nat.dev_of(d), nat.ptr(d), nat.ptr(out0.data), nat.ptr(out1.data), n,
            ctypes.c_void_p(slot_k0), ctypes.c_void_p(slot_k2), nn, nat.stream_of(d),
        ),
        "ring_extend3",
    )
    return out0, out1


def prg_bytes(key: bytes, nonce: int, nbytes: int, device="cpu", ctr0=0) -> torch.Tensor:
    out = torch.empty(nbytes, dtype=torch.uint8, device=device)
    kb = nat.key_buffer([key])
    nat.check(
        nat.lib().mx_prg(nat.dev_of(out), kb, nonce & MASK64, ctr0, nat.ptr(out), nbytes,
                         nat.stream_of(out)),
        "prg",
    )
    return out


def aes_encrypt(key: bytes, block: bytes) -> bytes:
    import ctypes

    kb = nat.key_buffer([key])
    inp = ctypes.create_string_buffer(bytes(block), 16)
    out = ctypes.create_string_buffer(16)
    nat.check(nat.lib().mx_aes_encrypt_blocks(kb, inp, out, 1), "aes")
    return out.raw


def _party_view(t: RT):
    """(party stride, period) in elements of a stacked [3, *inner] operand: element e of
    party p lives at p * ps + e % per.  Covers contiguous data, slices along the first inner
    axis and one row broadcast over it (stride 0); None for anything else."""
    d = t.data
    shape, strides = list(d.shape), list(d.stride())
    if t.bits == 128:
        if shape[-1] != 2 or strides[-1] != 1 or any(st % 2 for st in strides[:-1]):
            return None
        shape, strides = shape[:-1], [st // 2 for st in strides[:-1]]
    inner, ist = shape[1:], strides[1:]

    def dense(sh, st):
        expect = 1
        for size, stride in zip(reversed(sh), reversed(st)):
            if size != 1 and stride != expect:
                return False
            expect *= size
        return True

    if dense(inner, ist):
        return strides[0], math.prod(inner)
    if inner and ist[0] == 0 and dense(inner[1:], ist[1:]):
        return strides[0], math.prod(inner[1:])
    return None


def rss_mul3_k(kind: str, x0: RT, x1: RT, y0: RT, y1: RT, slot_ptr: int, nonce: int):
    """Stacked 3-party product with the reshare fused in: returns (s0, s1) with
    s0[p] = z_p and s1[p] = z_{p+1} (one kernel, see mx_rss_mul3_k)."""
    bits = x0.bits
    shp = x0.shape
    if y0 is not None and y0.shape != shp:
        x0, y0 = _broadcast(x0, y0)
        shp = x0.shape
    # x1/y0/y1 may be None: y0 None -> out = x0 + zero share (then reshared)
    ops = [None if p is None else (p if p.shape == shp else expand(p, shp)) for p in (x0, x1, y0, y1)]
    n = math.prod(shp) // 3
    out0, out1 = empty2(shp, bits, x0.device)
    if x0.data.is_cuda and any(o is not None and not o.data.is_contiguous() for o in ops):
        views = [(n, n) if o is None else _party_view(o) for o in ops]
        if all(v is not None for v in views):  # slices / row broadcasts read in place
            desc = (ctypes.c_int64 * 8)(*[v[0] for v in views], *[v[1] for v in views])
            nat.check(nat.lib().mx_rss_mul3_kv(
                nat.dev_of(out0.data), 1 if kind == "bool" else 0, _words(bits),
                *[nat.ptr(None if o is None else o.data) for o in ops], nat.ptr(out0.data),
                nat.ptr(out1.data), n, ctypes.c_void_p(slot_ptr), nonce & MASK64, desc,
                nat.stream_of(out0.data)), "rss_mul3_kv")
            return out0, out1
    datas = [None if o is None else o.data.contiguous() for o in ops]
    nat.check(
        nat.lib().mx_rss_mul3_k(
            nat.dev_of(out0.data), 1 if kind == "bool" else 0, _words(bits),
            *[nat.ptr(d) for d in datas], nat.ptr(out0.data), nat.ptr(out1.data), n,
            ctypes.c_void_p(slot_ptr), nonce & MASK64, nat.stream_of(out0.data),
        ),
        "rss_mul3_k",
    )
    return out0, out1


def mul_trunc3_k(x0: RT, x1: RT, y0: RT, y1: RT, slot_ptr: int, nmul: int, m: int, nonces,
                 out=None):
    """Fixed-point product of three stacked parties in one kernel on the device
    (mx_mul_trunc3_kv): ``rss_mul3_k(arith)`` + the stacked TruncPr of its result, bitwise
    the same.  ``out``: optional (s0, s1) views with dense party slots to write into.
    Returns (s0, s1), or None when not applicable (host, large or mixed-shape operands)."""
    bits = x0.bits
    if not x0.data.is_cuda or bits not in (64, 128):
        return None
    shp = x0.shape
    ops = (x0, x1, y0, y1)
    if any(o.shape != shp or o.bits != bits for o in ops):
        return None
    n = math.prod(shp) // 3
    if n == 0:
        return None
    views = None
    if any(not o.data.is_contiguous() for o in ops):
        vs = [_party_view(o) for o in ops]
        if any(v is None for v in vs):
            return None
        views = (ctypes.c_int64 * 8)(*[v[0] for v in vs], *[v[1] for v in vs])
    w = 2 if bits == 128 else 1
    if out is None:
        o0, o1 = ring4(shp, bits, x0.device)
        os_ = n
    else:
        o0, o1 = out
        os_ = o0.data.stride(0) // w
        if not (o0.shape == shp and o1.shape == shp and o1.data.stride(0) == o0.data.stride(0)
                and o0.data[0].is_contiguous() and o1.data[0].is_contiguous()):
            return None
    nn = (ctypes.c_uint64 * 6)(*[v & MASK64 for v in nonces])
    rc = nat.lib().mx_mul_trunc3_kv(
        nat.dev_of(o0.data), _words(bits), *[nat.ptr(o.data) for o in ops], nat.ptr(o0.data),
        nat.ptr(o1.data), n, os_, ctypes.c_void_p(slot_ptr), nmul & MASK64, int(m), nn, views,
        nat.stream_of(o0.data))
    if rc == 1:
        return None
    nat.check(rc, "mul_trunc3")
    return o0, o1


def _mt3_args(x0: RT, x1: RT, y0: RT, y1: RT, out=None):
    """mul_trunc3_k's argument checks and layout: (ops, (o0, o1), n, out stride, views) or
    None when the device kernel does not apply."""
    bits = x0.bits
    if not x0.data.is_cuda or bits not in (64, 128):
        return None
    shp = x0.shape
    ops = (x0, x1, y0, y1)
    if any(o.shape != shp or o.bits != bits for o in ops):
        return None
    n = math.prod(shp) // 3
    if n == 0:
        return None
    views = None
    if any(not o.data.is_contiguous() for o in ops):
        vs = [_party_view(o) for o in ops]
        if any(v is None for v in vs):
            return None
        views = [v[0] for v in vs] + [v[1] for v in vs]
    w = 2 if bits == 128 else 1
    if out is None:
        o0, o1 = ring4(shp, bits, x0.device)
        os_ = n
    else:
        o0, o1 = out
        os_ = o0.data.stride(0) // w
        if not (o0.shape == shp and o1.shape == shp and o1.data.stride(0) == o0.data.stride(0)
                and o0.data[0].is_contiguous() and o1.data[0].is_contiguous()):
            return None
    return ops, (o0, o1), n, os_, views


def mul_trunc3_k2(jobs, slot_ptr: int):
    """Two independent fixed-point products of one placement in ONE launch
    (mx_mul_trunc3_kv2): ``jobs`` = [(x0, x1, y0, y1, nmul, m, nonces, out), ...] (two),
    each exactly mul_trunc3_k's.  Returns [(s0, s1), (s0, s1)], or None when the batched
    kernel does not apply (the caller runs them one by one)."""
    if len(jobs) != 2:
        return None
    prep = [_mt3_args(*j[:4], out=j[7]) for j in jobs]
    if any(p is None for p in prep) or jobs[0][0].bits != jobs[1][0].bits:
        return None
    bits = jobs[0][0].bits
    if any(p[2] > 8192 * (16 // (16 if bits == 128 else 8)) for p in prep):
        return None  # throughput sizes: one by one
    P2 = ctypes.c_void_p * 2
    ptr = lambda t: t.data.data_ptr()  # noqa: E731
    vws = [None if p[4] is None else (ctypes.c_int64 * 8)(*p[4]) for p in prep]
    views = (ctypes.c_void_p * 2)(*[None if v is None else ctypes.addressof(v) for v in vws])
    nn = (ctypes.c_uint64 * 12)(*[v & MASK64 for j in jobs for v in j[6]])
    rc = nat.lib().mxh_mul_trunc3_kv2(
        _words(bits), P2(*[ptr(p[0][0]) for p in prep]), P2(*[ptr(p[0][1]) for p in prep]),
        P2(*[ptr(p[0][2]) for p in prep]), P2(*[ptr(p[0][3]) for p in prep]),
        P2(*[ptr(p[1][0]) for p in prep]), P2(*[ptr(p[1][1]) for p in prep]),
        (ctypes.c_int64 * 2)(*[p[2] for p in prep]), (ctypes.c_int64 * 2)(*[p[3] for p in prep]),
        ctypes.c_void_p(slot_ptr), (ctypes.c_uint64 * 2)(*[j[4] & MASK64 for j in jobs]),
        (ctypes.c_int * 2)(*[int(j[5]) for j in jobs]), nn, views,
        nat.stream_of(jobs[0][0].data))
    if rc == -1:
        return None
    nat.check(rc, "mul_trunc3 x2")
    return [p[1] for p in prep]


def zs_trunc3_k(z: RT, slot_ptr: int, nmul: int, m: int, nonces):
    """Zero share + reshare + TruncPr of three stacked parties' local products ``z``
    ([3, ...], e.g. a dot's GEMM output) in one kernel (mx_mul_trunc3_kv with the product
    given): bitwise ``trunc_pr3(rss_mul3_k(arith, z))`` -- the reshared product is never
    written.  Returns (s0, s1), or None on the host."""
    bits = z.bits
    if not z.data.is_cuda or bits not in (64, 128):
        return None
    d = z.data.contiguous()
    shp = z.shape
    n = math.prod(shp) // 3
    if n == 0:
        return None
    o0, o1 = ring4(shp, bits, d.device)
    nn = (ctypes.c_uint64 * 6)(*[v & MASK64 for v in nonces])
    rc = nat.lib().mx_mul_trunc3_kv(
        nat.dev_of(d), _words(bits), nat.ptr(d), None, None, None, nat.ptr(o0.data),
        nat.ptr(o1.data), n, n, ctypes.c_void_p(slot_ptr), nmul & MASK64, int(m), nn, None,
        nat.stream_of(d))
    if rc == 1:
        return None
    nat.check(rc, "zs_trunc3")
    return o0, o1


def zs_trunc3_open(z: RT, slot_ptr: int, nmul: int, m: int, nonces, frac: int):
    """decode(reveal(zs_trunc3_k(z, ...)), frac) in one kernel (mx_mul_trunc3_open): the tail
    of a dot that is only revealed.  Same keys and nonces as zs_trunc3_k, so bitwise the
    decode of the sum of its shares -- which are not written.  ``z``: [3, ...] local
    products, dense or party slots of a larger stack.  Returns the float64 tensor, or None
    when the layout does not apply."""
    bits = z.bits
    if bits not in (64, 128):
        return None
    if isinstance(z, CrtProduct) and z.pending():
        return z.open(slot_ptr, nmul, m, nonces, frac)
    pv = _party_view(z)
    n = math.prod(z.shape) // 3
    if pv is None or pv[1] != n or pv[0] < n:
        d, xs = z.data.contiguous(), n
    else:
        d, xs = z.data, pv[0]
    if n == 0:
        return None
    out = torch.empty(z.shape[1:], dtype=torch.float64, device=d.device)
    nn = (ctypes.c_uint64 * 6)(*[v & MASK64 for v in nonces])
    nat.check(nat.lib().mx_mul_trunc3_open(
        nat.dev_of(d), _words(bits), nat.ptr(d), xs, nat.ptr(out), n, ctypes.c_void_p(slot_ptr),
        nmul & MASK64, int(m), nn, int(frac), nat.stream_of(d), None), "zs_trunc3_open")
    return out


def zs_trunc3_rows(z: RT, slot_ptr: int, nmul: int, m: int, nonces, buf4, r0: int):
    """zs_trunc3_k for the row block [r0, r0 + rows) of a pipelined product: ``z`` =
    [3, rows, N] local products, the shares written straight into rows of ``buf4`` (the
    result's [4, M, N] share-pair ring buffer, slots x0, x1, x2, x0)."""
    bits = z.bits
    d = z.data.contiguous()
    n = math.prod(z.shape) // 3  # ring elements per party in the block
    el = 2 if bits == 128 else 1
    os_ = math.prod(buf4.shape[1:]) // el  # party stride of the result (elements)
    o0 = buf4.data_ptr() + r0 * math.prod(buf4.shape[2:]) * 8
    nn = (ctypes.c_uint64 * 6)(*[v & MASK64 for v in nonces])
    rc = nat.lib().mx_mul_trunc3_kv(
        nat.dev_of(d), _words(bits), nat.ptr(d), None, None, None, ctypes.c_void_p(o0),
        ctypes.c_void_p(o0 + os_ * el * 8), n, os_, ctypes.c_void_p(slot_ptr), nmul & MASK64,
        int(m), nn, None, nat.stream_of(d))
    nat.check(rc, "zs_trunc3_rows")


def add_zs3(v: RT, r: RT):
    """Stacked arith zero share from precomputed keystreams ``r`` (= PRF(k_p) per party)
    plus the reshare: returns (s0, s1) exactly like ``rss_mul3_k(arith, v)``."""
    vd, rd = v.data.contiguous(), r.data.contiguous()
    n = math.prod(v.shape) // 3
    o0, o1 = empty(v.shape, v.bits, v.device), empty(v.shape, v.bits, v.device)
    nat.check(nat.lib().mx_add_zs3(nat.dev_of(vd), _words(v.bits), nat.ptr(vd), nat.ptr(rd),
                                   nat.ptr(o0.data), nat.ptr(o1.data), n, nat.stream_of(vd)),
              "add_zs3")
    return o0, o1


def _slot_operand_ok(a: RT, b: RT) -> bool:
    """b broadcasts over one slot of stacked a as a period: a scalar, or b's shape (leading
    1s dropped) is a suffix of the slot's shape."""
    if b.numel() == 1:
        return True
    bs = list(b.shape)
    while bs and bs[0] == 1:
        bs.pop(0)
    ss = list(a.shape[1:])
    return len(bs) <= len(ss) and ss[len(ss) - len(bs):] == bs


def binary_slot(op: str, a: RT, b: RT, which: int):
    """Stacked [nparties, *shape] ``a``: ``op`` with public ``b`` (same shape as one slot,
    or a scalar) applied to slot ``which`` only, one kernel (mx_ew_binary_slot)."""
    np_, m = a.shape[0], math.prod(a.shape[1:])
    nb = b.numel()
    if not _slot_operand_ok(a, b):
        raise ValueError("binary_slot: operand must be a scalar, one slot's shape or a "
                         "trailing-axes suffix of it")
    ad = a.data.contiguous()
    bd = b.data.contiguous()
    if bd.device != ad.device:
        bd = bd.to(ad.device)
    out = empty(a.shape, a.bits, a.device)
    nat.check(
        nat.lib().mx_ew_binary_slot(
            nat.dev_of(ad), _BIN[op], _words(a.bits), nat.ptr(ad), nat.ptr(bd), nb,
            nat.ptr(out.data), m, np_, int(which), nat.stream_of(ad),
        ),
        "binary_slot",
    )
    return out


def binary_slot2(op: str, a0: RT, a1: RT, b: RT, which0: int, which1: int):
    """binary_slot on both share vectors (slots which0 / which1) in one launch."""
    if a0.bits == 1 or a1.shape != a0.shape:
        return binary_slot(op, a0, b, which0), binary_slot(op, a1, b, which1)
    np_, m = a0.shape[0], math.prod(a0.shape[1:])
    nb = b.numel()
    if not _slot_operand_ok(a0, b):
        raise ValueError("binary_slot2: operand must be a scalar, one slot's shape or a "
                         "trailing-axes suffix of it")
    d0, d1, bd = a0.data.contiguous(), a1.data.contiguous(), b.data.contiguous()
    if bd.device != d0.device:
        bd = bd.to(d0.device)
    o0, o1 = empty2(a0.shape, a0.bits, a0.device)
    nat.check(nat.lib().mx_ew_binary_slot2(
        nat.dev_of(d0), _BIN[op], _words(a0.bits), nat.ptr(d0), nat.ptr(d1), nat.ptr(bd), nb,
        nat.ptr(o0.data), nat.ptr(o1.data), m, np_, int(which0), int(which1),
        nat.stream_of(d0)), "binary_slot (pair)")
    return o0, o1


_RT_DATA = RT.__dict__["data"]  # the base class's slot descriptor


class Opened(RT):
    """An opened (revealed) value a + b + c [+ d] whose sum is formed on first use of
    ``data``.  A decode of it runs one fused pass (mx_addn_decode) instead of add + decode:
    the ring-valued sum never goes to memory."""

    __slots__ = ("parts", "stream")

    def __init__(self, a: RT, b: RT, c: RT, d: RT = None):
        _RT_DATA.__set__(self, None)
        self.bits = a.bits
        self._shape = a.shape
        self.parts = (a, b, c) if d is None else (a, b, c, d)
        self.stream = _stream_of(a.data)

    def pending(self) -> bool:
        return _RT_DATA.__get__(self) is None

    @property
    def data(self):
        d = _RT_DATA.__get__(self)
        if d is None:
            _join(self.stream)
            s = add3(*self.parts[:3])
            if len(self.parts) == 4:
                s = binary("add", s, self.parts[3])
            d = s.data
            _RT_DATA.__set__(self, d)
            self.parts = None
        return d

    @data.setter
    def data(self, v):
        _RT_DATA.__set__(self, v)

    @property
    def device(self):
        return self.parts[0].device if self.pending() else self.data.device


class OpenedTail(RT):
    """The opened value of a fixed-point dot whose tail has not run (``src``: a
    protocols/replicated.StackedTail, revealed to its party ``j``).  A decode of it runs the
    tail and the reveal as one kernel (``src.open``: mx_mul_trunc3_open) -- the new shares
    never go to memory.  Any other use, or a decode after something read the shares, takes
    the ordinary tail and an :class:`Opened` of its shares: the same value bitwise."""

    __slots__ = ("src", "j")

    def __init__(self, src, j: int, shape):
        _RT_DATA.__set__(self, None)
        self.bits = src.bits
        self._shape = tuple(shape)
        self.src = src
        self.j = j

    def pending(self) -> bool:
        return _RT_DATA.__get__(self) is None

    def shares(self) -> RT:
        """The ordinary reveal: an Opened of party j's two shares and P_{j+1}'s second."""
        v0, v1 = self.src.s0.v, self.src.s1.v
        j, j1 = self.j, (self.j + 1) % 3
        return opened(RT(v0.data[j], v0.bits), RT(v1.data[j], v1.bits),
                      RT(v1.data[j1], v1.bits))

    @property
    def data(self):
        d = _RT_DATA.__get__(self)
        if d is None:
            d = self.shares().data
            _RT_DATA.__set__(self, d)
            self.src = None
        return d

    @data.setter
    def data(self, v):
        _RT_DATA.__set__(self, v)

    @property
    def device(self):
        return self.src.device if self.pending() else self.data.device


class CrtProduct(RT):
    """The three parties' local products [3, M, N] of a stacked dot (dot_cross_asym under
    :func:`deferred_products`) still held as the CRT GEMM's output residues.  A tail that is
    opened by its first reader reconstructs them inside the opening kernel (:meth:`open`:
    mx_mul_trunc3_open's crt form) and the products never go to memory; any read of ``data``
    runs the reconstruction the product skipped (mx_crt_recon) -- the same values bitwise.
    The residues are the product's own buffer, not the GEMM workspace, so later products on
    the stream do not touch them."""

    __slots__ = ("residues", "mnk", "stream")

    def __init__(self, residues: torch.Tensor, M: int, N: int, K: int, bits: int):
        _RT_DATA.__set__(self, None)
        self.bits = bits
        self._shape = (3, M, N)
        self.residues = residues
        self.mnk = (M, N, K)
        self.stream = _stream_of(residues)

    def pending(self) -> bool:
        return _RT_DATA.__get__(self) is None

    def _residues_here(self) -> torch.Tensor:
        """The residues, ordered before (and kept alive for) the current stream's use."""
        _join(self.stream)
        cur = torch.cuda.current_stream(self.residues.device)
        if cur != self.stream:
            self.residues.record_stream(cur)
        return self.residues

    def open(self, slot_ptr: int, nmul: int, m: int, nonces, frac: int) -> torch.Tensor:
        """zs_trunc3_open of the product, reconstructed on the way; the residues stay (a
        later read of the shares rebuilds the product from them)."""
        res = self._residues_here()
        M, N, K = self.mnk
        out = torch.empty((M, N), dtype=torch.float64, device=res.device)
        nn = (ctypes.c_uint64 * 6)(*[v & MASK64 for v in nonces])
        crt = (ctypes.c_int64 * 4)(res.data_ptr(), M, N, K)
        nat.check(nat.lib().mx_mul_trunc3_open(
            1, _words(self.bits), None, 0, nat.ptr(out), M * N, ctypes.c_void_p(slot_ptr),
            nmul & MASK64, int(m), nn, int(frac), nat.stream_of(res), crt), "zs_trunc3_open (crt)")
        return out

    @property
    def data(self):
        d = _RT_DATA.__get__(self)
        if d is None:
            res = self._residues_here()
            M, N, K = self.mnk
            out = empty((3, M, N), self.bits, res.device)
            nat.check(nat.lib().mx_crt_recon(_words(self.bits), M, N, K, nat.ptr(res),
                                             nat.ptr(out.data), nat.stream_of(res)), "crt_recon")
            d = out.data
            _RT_DATA.__set__(self, d)
            self.residues = None
        return d

    @data.setter
    def data(self, v):
        _RT_DATA.__set__(self, v)

    @property
    def device(self):
        return self.residues.device if self.pending() else self.data.device


def opened(a: RT, b: RT, c: RT, d: RT = None) -> RT:
    """a + b + c [+ d] as an :class:`Opened` (lazy) when the fused decode applies.  The
    addends are shares of the value at its own type's scale: a reveal never opens a value
    with more fractional bits than its type (no truncation is ever deferred into a reveal)."""
    parts = (a, b, c) if d is None else (a, b, c, d)
    if a.bits in (64, 128) and all(t.shape == a.shape and t.bits == a.bits for t in parts):
        return Opened(*parts)
    s = add3(a, b, c)
    return s if d is None else binary("add", s, d)


def add3(a: RT, b: RT, c: RT) -> RT:
    """a + b + c of one shape in one pass (mx_ew_add3)."""
    if not (a.shape == b.shape == c.shape and a.bits == b.bits == c.bits) or a.bits == 1:
        return binary("add", binary("add", a, b), c)
    d = [t.data.contiguous() for t in (a, b, c)]
    out = empty(a.shape, a.bits, a.device)
    nat.check(nat.lib().mx_ew_add3(nat.dev_of(d[0]), _words(a.bits), *[nat.ptr(x) for x in d],
                                   nat.ptr(out.data), a.numel(), nat.stream_of(d[0])), "add3")
    return out


def lincomb2(terms, b=None, which0: int = 0, which1: int = 2):
    """Share-wise sum_t coef_t * (s0_t, s1_t) of stacked [nparties, ...] share vectors (+ the
    public ``b`` at slots which0 / which1) in one launch (mx_lincomb2).  ``terms``: up to 3
    (int coef, RT s0, RT s1) of one shape.  Returns (out0, out1)."""
    c0, a0, _ = terms[0]
    bits, shp = a0.bits, a0.shape
    np_, m = shp[0], math.prod(shp[1:])
    datas = []
    for _, x0, x1 in terms:
        datas += [x0.data.contiguous(), x1.data.contiguous()]
    bd = None
    if b is not None:
        bd = b.data.contiguous()
        if bd.device != a0.device:
            bd = bd.to(a0.device)
    o0, o1 = empty2(shp, bits, a0.device)
    ins = (ctypes.c_void_p * len(datas))(*[d.data_ptr() for d in datas])
    coef = (ctypes.c_int64 * len(terms))(*[int(t[0]) for t in terms])
    nat.check(nat.lib().mx_lincomb2(
        nat.dev_of(o0.data), _words(bits), len(terms), ins, coef, nat.ptr(bd),
        b.numel() if b is not None else 0, nat.ptr(o0.data), nat.ptr(o1.data), m, np_,
        int(which0), int(which1), nat.stream_of(o0.data)), "lincomb2")
    return o0, o1


def _even_views(ts):
    """(base tensor, element step, party stride) when the stacked RTs ``ts`` are views of one
    buffer at a constant step with dense party slots; None otherwise."""
    d0 = ts[0].data
    w = 2 if ts[0].bits == 128 else 1
    if d0.dim() < 1 or not d0[0].is_contiguous() or d0.stride(0) % w:
        return None
    es = d0.element_size() * w
    ptrs = [t.data.data_ptr() for t in ts]
    for t in ts:
        d = t.data
        if (d.shape != d0.shape or d.stride() != d0.stride() or d.dtype != d0.dtype
                or d.device != d0.device or t.bits != ts[0].bits):
            return None
    if len(ts) > 1:
        step = ptrs[1] - ptrs[0]
        if step <= 0 or step % es or any(ptrs[i + 1] - ptrs[i] != step for i in range(len(ts) - 1)):
            return None
        step //= es
    else:
        step = 0
    return d0, step, d0.stride(0) // w


def sum_views2(ts0, ts1):
    """(sum of ts0, sum of ts1) -- k stacked share vectors each -- in one launch when both
    lists are evenly spaced views of one buffer (mx_sum_views2); None otherwise."""
    v0, v1 = _even_views(ts0), _even_views(ts1)
    if v0 is None or v1 is None or ts0[0].shape != ts1[0].shape:
        return None
    bits, shp = ts0[0].bits, ts0[0].shape
    o0, o1 = empty2(shp, bits, ts0[0].device)
    np_, m = shp[0], math.prod(shp[1:])
    nat.check(nat.lib().mx_sum_views2(
        nat.dev_of(o0.data), _words(bits), v0[0].data_ptr(), v1[0].data_ptr(), v0[1], v1[1],
        v0[2], v1[2], len(ts0), nat.ptr(o0.data), nat.ptr(o1.data), m, np_,
        nat.stream_of(o0.data)), "sum_views2")
    return o0, o1


def b2a_prep3(b0: RT, b1: RT, ring_bits: int):
    """rep.b2a's local values for three stacked parties in one launch (k_b2a_prep3): P0's
    a = b_0 ^ b_1 as a ring tensor [...] and the trivial sharing of b_2 (slot 2) as a
    pair of [3, ...] party vectors.  None when not on the device."""
    d0, d1 = b0.data, b1.data
    if not d0.is_cuda or ring_bits not in (64, 128) or d0.dtype != torch.uint8 \
            or d1.dtype != torch.uint8 or d0.shape != d1.shape or d0.shape[0] != 3:
        return None
    d0, d1 = d0.contiguous(), d1.contiguous()
    shp = tuple(d0.shape[1:])
    a = empty(shp, ring_bits, d0.device)
    o0, o1 = empty2((3,) + shp, ring_bits, d0.device)
    nat.check(nat.lib().mxh_b2a_prep3(_words(ring_bits), nat.ptr(d0), nat.ptr(d1),
                                      math.prod(shp), nat.ptr(a.data), nat.ptr(o0.data),
                                      nat.ptr(o1.data), nat.stream_of(d0)), "b2a_prep3")
    return a, o0, o1


def b2a3(b0: RT, b1: RT, ring_bits: int, slot_ptr: int, mir: bool, n1: int, nmul: int):
    """The whole of rep.b2a for three stacked parties in one launch (k_b2a3): P0's sharing
    of a = b_0 ^ b_1 (mask nonce n1, key k_0, or k_1 mirrored), its product with the trivial
    sharing of b_2 (zero-share nonce nmul) and A + B - 2 AB.  Returns the (s0, s1) pair of
    [3, ...] arithmetic share vectors, or None when not on the device."""
    d0, d1 = b0.data, b1.data
    if not d0.is_cuda or ring_bits not in (64, 128) or d0.dtype != torch.uint8 \
            or d1.dtype != torch.uint8 or d0.shape != d1.shape or d0.shape[0] != 3:
        return None
    d0, d1 = d0.contiguous(), d1.contiguous()
    o0, o1 = ring4(tuple(d0.shape), ring_bits, d0.device)
    nat.check(nat.lib().mxh_b2a3(_words(ring_bits), nat.ptr(d0), nat.ptr(d1),
                                 math.prod(d0.shape[1:]), nat.ptr(o0.data), nat.ptr(o1.data),
                                 ctypes.c_void_p(slot_ptr), int(bool(mir)), n1 & MASK64,
                                 nmul & MASK64, nat.stream_of(d0)), "b2a3")
    return o0, o1


def b2a3_planes(w0: RT, w1: RT, start: int, count: int, slot_ptr: int, mir: bool, n1: int,
                nmul: int):
    """b2a3 of BitSplit(start, count) of a packed boolean share pair (w0, w1: [3, ...] ring
    words) in one launch, the planes never materialised: (s0, s1) arithmetic [3, count,
    ...] pairs, or None (host)."""
    d0, d1 = w0.data, w1.data
    bits = w0.bits
    if not d0.is_cuda or bits not in (64, 128) or w1.bits != bits or w0.shape != w1.shape \
            or w0.shape[0] != 3 or start < 0 or count < 1 or start + count > bits:
        return None
    d0, d1 = d0.contiguous(), d1.contiguous()
    rest = tuple(w0.shape[1:])
    o0, o1 = ring4((3, count) + rest, bits, d0.device)
    nat.check(nat.lib().mxh_b2a3_planes(
        _words(bits), nat.ptr(d0), nat.ptr(d1), math.prod(rest), int(start), int(count),
        nat.ptr(o0.data), nat.ptr(o1.data), ctypes.c_void_p(slot_ptr), int(bool(mir)),
        n1 & MASK64, nmul & MASK64, nat.stream_of(d0)), "b2a3_planes")
    return o0, o1


def mux3(s0: RT, s1: RT, x0: RT, x1: RT, y0: RT, y1: RT, slot_ptr: int, nonce: int,
         absv: bool = False):
    """rep.mux(s, x, y) = s * (x - y) + y for arithmetic stacked sharings in one launch
    (k_mux3_lat, zero-share nonce ``nonce``); ``absv``: x - 2 s x instead (y = x, unused).
    Returns (s0, s1), or None (host, shapes)."""
    ts = (s0, s1, x0, x1, y0, y1)
    bits = s0.bits
    if not s0.data.is_cuda or bits not in (64, 128) or any(
            t.bits != bits or t.shape != s0.shape for t in ts) or s0.shape[0] != 3:
        return None
    ds = [t.data.contiguous() for t in ts]
    o0, o1 = ring4(s0.shape, bits, ds[0].device)
    nat.check(nat.lib().mxh_mux3(_words(bits), *[nat.ptr(d) for d in ds], nat.ptr(o0.data),
                                 nat.ptr(o1.data), math.prod(s0.shape[1:]),
                                 ctypes.c_void_p(slot_ptr), nonce & MASK64, int(bool(absv)),
                                 nat.stream_of(ds[0])), "mux3")
    return o0, o1


def bitdec3(x0: RT, x1: RT, slot_ptr: int, mir: bool, n1: int, nmul: int, nonces,
            sign_nonces=None):
    """The whole of rep.bit_decompose for three stacked parties in one launch (k_bitdec3):
    P0's boolean sharing of y = x_0 + x_1 (mask nonce n1, key k_0 or mirrored k_1), the
    trivial sharing of x_2, the adder's xor and AND (zero-share nonce nmul) and its
    Kogge-Stone chain (``nonces``, one per level) with the sum.  Returns the (s0, s1) pair of
    packed boolean share vectors [3, ...], or None (host, or above the latency sizes).
    ``sign_nonces`` = (n1', nmul'): instead, the b2a of the sum's top bit (rep.b2a of
    rep.msb: its sharing and product nonces) as an arithmetic share pair."""
    d0, d1 = x0.data, x1.data
    bits = x0.bits
    if not d0.is_cuda or bits not in (64, 128) or x1.bits != bits or x0.shape != x1.shape \
            or x0.shape[0] != 3:
        return None
    n = math.prod(x0.shape[1:])
    if n > 65536 or len(nonces) != bits.bit_length() - 1:
        return None
    d0, d1 = d0.contiguous(), d1.contiguous()
    sign = sign_nonces is not None
    o0, o1 = (ring4 if sign else empty2)(x0.shape, bits, d0.device)
    arr = (ctypes.c_uint64 * len(nonces))(*[int(v) & MASK64 for v in nonces])
    sb = sign_nonces or (0, 0)
    rc = nat.lib().mxh_bitdec3(_words(bits), nat.ptr(d0), nat.ptr(d1), nat.ptr(o0.data),
                               nat.ptr(o1.data), n, len(nonces), ctypes.c_void_p(slot_ptr),
                               int(bool(mir)), n1 & MASK64, nmul & MASK64, arr, int(sign),
                               sb[0] & MASK64, sb[1] & MASK64, nat.stream_of(d0))
    nat.check(rc, "bitdec3")
    return o0, o1


def slot_place2(x0: RT, x1: RT, which0: int, which1: int, nparties: int = 3):
    """Two trivial stacked sharings [nparties, *x.shape] in one launch: slot which0 of the
    first = x0, slot which1 of the second = x1, zeros elsewhere (mx_slot_place2)."""
    bits = x0.bits
    shp = (nparties,) + tuple(x0.shape)
    o0, o1 = empty2(shp, bits, x0.device)
    d0, d1 = x0.data.contiguous(), x1.data.contiguous()
    nat.check(nat.lib().mx_slot_place2(
        nat.dev_of(d0), _words(bits), nat.ptr(d0), nat.ptr(d1), nat.ptr(o0.data),
        nat.ptr(o1.data), x0.numel(), nparties, int(which0), int(which1), nat.stream_of(d0)),
        "slot_place2")
    return o0, o1


def ks_cross1(g0: RT, g1: RT, p0: RT, p1: RT, d: int, both: bool, keys, nonce: int) -> RT:
    """One party's masked cross terms of a Kogge-Stone level (mx_ks_cross1): shape
    ``[2, *shape]`` (t, pk') if ``both`` else ``shape``; ``keys`` = (k_p, k_{p+1})."""
    bits = g0.bits
    shp = g0.shape
    datas = [x.data.contiguous() for x in (g0, g1, p0, p1)]
    n = math.prod(shp)
    z = empty(((2,) + tuple(shp)) if both else tuple(shp), bits, g0.device)
    kbuf = nat.key_buffer(list(keys))
    nat.check(
        nat.lib().mx_ks_cross1(
            nat.dev_of(z.data), _words(bits), *[nat.ptr(x) for x in datas], nat.ptr(z.data),
            n, int(d), 1 if both else 0, kbuf, nonce & MASK64, nat.stream_of(z.data),
        ),
        "ks_cross1",
    )
    return z


def _empty_in(alloc, shape, bits, device) -> RT:
    """``empty``, or from ``alloc(shape, dtype)`` (a session's outbox: a message)."""
    if alloc is None:
        return empty(shape, bits, device)
    shape = tuple(shape)
    if bits == 128:
        return RT(alloc(shape + (2,), torch.int64), 128)
    return RT(alloc(shape, torch.int64 if bits == 64 else torch.uint8), bits)


def ks_cross1_s(g0: RT, g1: RT, p0: RT, p1: RT, d: int, both: bool, slot_ptrs,
                nonce: int, alloc=None) -> RT:
    """ks_cross1 with the keys (k_p, k_{p+1}) read from two device key slots (``alloc``:
    where z, the level's message, goes)."""
    bits = g0.bits
    shp = g0.shape
    datas = [x.data.contiguous() for x in (g0, g1, p0, p1)]
    n = math.prod(shp)
    z = _empty_in(alloc, ((2,) + tuple(shp)) if both else tuple(shp), bits, g0.device)
    nat.check(
        nat.lib().mx_ks_cross1_s(
            nat.dev_of(z.data), _words(bits), *[nat.ptr(x) for x in datas], nat.ptr(z.data),
            n, int(d), 1 if both else 0, _slots_arr(slot_ptrs), nonce & MASK64,
            nat.stream_of(z.data),
        ),
        "ks_cross1_s",
    )
    return z


def ks_cross1x_s(g0: RT, g1: RT, t0, t1, p0: RT, p1: RT, d: int, both: bool, slot_ptrs,
                 nonce: int, alloc=None):
    """ks_cross1_s on g ^ t (the previous level's xor folded into this level's launch;
    t0 = t1 = None: plain ks_cross1_s).  Returns (z, (g0 ^ t0, g1 ^ t1) or None)."""
    if t0 is None:
        return ks_cross1_s(g0, g1, p0, p1, d, both, slot_ptrs, nonce, alloc=alloc), None
    bits = g0.bits
    shp = g0.shape
    datas = [x.data.contiguous() for x in (g0, g1, t0, t1, p0, p1)]
    n = math.prod(shp)
    z = _empty_in(alloc, ((2,) + tuple(shp)) if both else tuple(shp), bits, g0.device)
    go0, go1 = empty2(shp, bits, g0.device)
    nat.check(
        nat.lib().mx_ks_cross1x_s(
            nat.dev_of(z.data), _words(bits), *[nat.ptr(x) for x in datas[:4]],
            nat.ptr(go0.data), nat.ptr(go1.data), nat.ptr(datas[4]), nat.ptr(datas[5]),
            nat.ptr(z.data), n, int(d), 1 if both else 0, _slots_arr(slot_ptrs),
            nonce & MASK64, nat.stream_of(z.data),
        ),
        "ks_cross1x_s",
    )
    return z, (go0, go1)


def ks_sum2(p0: RT, p1: RT, g0: RT, g1: RT, t0: RT, t1: RT):
    """The adder's sum after its last level for both share components, one launch:
    p ^ ((g ^ t) << 1) (mx_ks_sum2)."""
    bits = p0.bits
    datas = [x.data.contiguous() for x in (p0, p1, g0, g1, t0, t1)]
    o0, o1 = empty2(p0.shape, bits, p0.device)
    nat.check(nat.lib().mx_ks_sum2(
        nat.dev_of(o0.data), _words(bits), *[nat.ptr(x) for x in datas], nat.ptr(o0.data),
        nat.ptr(o1.data), math.prod(p0.shape), nat.stream_of(o0.data)), "ks_sum2")
    return o0, o1


def ks_adder3_k(g0: RT, g1: RT, p0: RT, p1: RT, slot_ptr: int, nonces,
                sum_out: bool = False) -> tuple:
    """The whole Kogge-Stone carry chain (len(nonces) levels d = 1, 2, 4, ...) for three
    stacked parties in one launch (mx_ks_adder3_k): bitwise the chain of ks_level3_k calls
    with those nonces; returns the final (g0, g1) -- or, with ``sum_out`` (device only),
    the adder's sum p ^ (g << 1) (p = the initial p0, p1)."""
    bits = g0.bits
    datas = [x.data.contiguous() for x in (g0, g1, p0, p1)]
    n = math.prod(g0.shape) // 3
    o0, o1 = empty2(g0.shape, bits, g0.device)
    arr = (ctypes.c_uint64 * len(nonces))(*[int(v) & MASK64 for v in nonces])
    if sum_out:
        nat.check(nat.lib().mxh_ks_adder3_sum(
            _words(bits), *[nat.ptr(x) for x in datas], nat.ptr(o0.data), nat.ptr(o1.data), n,
            len(nonces), ctypes.c_void_p(slot_ptr), arr, nat.stream_of(o0.data), 1),
            "ks_adder3 (sum)")
        return o0, o1
    nat.check(nat.lib().mx_ks_adder3_k(
        nat.dev_of(o0.data), _words(bits), *[nat.ptr(x) for x in datas], nat.ptr(o0.data),
        nat.ptr(o1.data), n, len(nonces), ctypes.c_void_p(slot_ptr), arr,
        nat.stream_of(o0.data)), "ks_adder3_k")
    return o0, o1


def ks_level3_k(g0: RT, g1: RT, p0: RT, p1: RT, d: int, both: bool, slot_ptr: int,
                nonce: int):
    """One fused Kogge-Stone level for three stacked parties (mx_ks_level3_k): returns
    the reshared (g0', g1', p0', p1') -- p0'/p1' are None unless ``both``."""
    bits = g0.bits
    shp = g0.shape
    datas = [x.data.contiguous() for x in (g0, g1, p0, p1)]
    n = math.prod(shp) // 3
    nout = 4 if both else 2
    blk = empty((nout,) + tuple(shp), bits, g0.device).data
    outs = [RT(blk[i], bits) for i in range(nout)]
    dummy = outs[0].data
    nat.check(
        nat.lib().mx_ks_level3_k(
            nat.dev_of(outs[0].data), _words(bits), *[nat.ptr(x) for x in datas],
            nat.ptr(outs[0].data), nat.ptr(outs[1].data),
            nat.ptr(outs[2].data if both else dummy), nat.ptr(outs[3].data if both else dummy),
            n, int(d), 1 if both else 0, ctypes.c_void_p(slot_ptr), nonce & MASK64,
            nat.stream_of(outs[0].data),
        ),
        "ks_level3_k",
    )
    return (outs[0], outs[1], outs[2], outs[3]) if both else (outs[0], outs[1], None, None)


def rss_cross_k(kind: str, x0: RT, x1, y0, y1, slot_ptr: int, nslots: int, nonce: int,
                nparties: int) -> RT:
    """``rss_cross`` with the zero-share keys read from key slots: party p uses slots
    p % nslots and (p + 1) % nslots."""
    return rss_cross(kind, x0, x1, y0, y1, None, nonce, nparties, _slots=(slot_ptr, nslots))


def rss_cross_kp(kind: str, x0: RT, x1, y0, y1, slot_ptrs, nonce: int) -> RT:
    """``rss_cross`` for stacked parties with independent key PAIRS: party p masks with
    PRF(slot_ptrs[2p]) - PRF(slot_ptrs[2p+1]) (``len(slot_ptrs) == 2 * nparties``).  The
    parties of one stack may then belong to different sessions (mx_rss_cross_kp)."""
    nparties = len(slot_ptrs) // 2
    bits = x0.bits
    shp = x0.shape
    if y0 is not None and y0.shape != shp:
        x0, y0 = _broadcast(x0, y0)
        shp = x0.shape
    datas = [None if p is None else (p if p.shape == shp else expand(p, shp)).data.contiguous()
             for p in (x0, x1, y0, y1)]
    n = math.prod(shp) // nparties
    out = empty(shp, bits, x0.device)
    arr = (ctypes.c_void_p * len(slot_ptrs))(*slot_ptrs)
    nat.check(
        nat.lib().mx_rss_cross_kp(
            nat.dev_of(out.data), 1 if kind == "bool" else 0, _words(bits),
            *[nat.ptr(d) for d in datas], nat.ptr(out.data), n, nparties, arr,
            nonce & MASK64, nat.stream_of(out.data),
        ),
        "rss_cross_kp",
    )
    return out


def rss_cross(kind: str, x0: RT, x1, y0: RT, y1, keys, nonce: int, nparties: int,
              _slots=None) -> RT:
    """Fused RSS local step.  Stacked layout: x* are [nparties, *shape]; party p gets
    x0*y0 + x0*y1 + x1*y0 + PRF(k_p) - PRF(k_{p+1}) (boolean: & / ^).  ``keys`` is a list
    of nparties+1 keys (or None for no zero share)."""
    bits = x0.bits
    shp = x0.shape
    if y0 is not None and y0.shape != shp:
        x0, y0 = _broadcast(x0, y0)
        shp = x0.shape
    parts = [x0, x1, y0, y1]
    datas = []
    for p in parts:
        if p is None:
            datas.append(None)
        else:
            if p.shape != shp:
                p = expand(p, shp)
            datas.append(p.data.contiguous())
    n_total = math.prod(shp)
    n = n_total // nparties
    out = empty(shp, bits, x0.device)
    if _slots is not None:
        nat.check(
            nat.lib().mx_rss_cross_k(
                nat.dev_of(out.data), 1 if kind == "bool" else 0, _words(bits),
                nat.ptr(datas[0]), nat.ptr(datas[1]), nat.ptr(datas[2]), nat.ptr(datas[3]),
                nat.ptr(out.data), n, nparties, ctypes.c_void_p(_slots[0]), _slots[1],
                nonce & MASK64, nat.stream_of(out.data),
            ),
            "rss_cross_k",
        )
        return out
    kbuf = nat.key_buffer(keys) if keys is not None else None
    nat.check(
        nat.lib().mx_rss_cross(
            nat.dev_of(out.data), 1 if kind == "bool" else 0, _words(bits),
            nat.ptr(datas[0]), nat.ptr(datas[1]), nat.ptr(datas[2]), nat.ptr(datas[3]),
            nat.ptr(out.data), n, nparties, kbuf, nonce & MASK64, nat.stream_of(out.data),
        ),
        "rss_cross",
    )
    return out


def zero_share(kind: str, shape, bits, keys, nonce: int, nparties: int, device) -> RT:
    shape = tuple(shape)
    out = empty(shape, bits, device)
    n = math.prod(shape) // nparties
    nat.check(
        nat.lib().mx_zero_share(
            nat.dev_of(out.data), 1 if kind == "bool" else 0, _words(bits), nat.ptr(out.data), n,
            nparties, nat.key_buffer(keys), nonce & MASK64, nat.stream_of(out.data),
        ),
        "zero_share",
    )
    return out


# ---------------------------------------------------------------------------
# per-party protocol rounds (parties of a session on different GPUs)
# ---------------------------------------------------------------------------
def _roles_arr(roles):
    return (ctypes.c_int * len(roles))(*roles)


def _slots_arr(slots):
    return (ctypes.c_void_p * len(slots))(*slots)


def _nonces_arr(nonces):
    return (ctypes.c_uint64 * len(nonces))(*[v & MASK64 for v in nonces])


def trunc_party_r0(s0: RT, s1: RT, m: int, roles, slots, nonces, alloc=None):
    """Round 0 of the per-party TruncPr (mx_trunc_party_r0) on stacked [ncomp, ...] shares.
    Returns (msg, msg_rm, out0, out1): outgoing messages and the (partly filled) new
    shares.  ``alloc``: where the messages go."""
    ncomp = len(roles)
    d0 = s0.data.contiguous()
    d1 = s1.data.contiguous()
    n = math.prod(s0.shape) // ncomp
    msg = _new(alloc, d0.shape, d0.dtype, d0.device)
    out0, out1 = torch.empty_like(d0), torch.empty_like(d0)
    msg_rm = _new(alloc, (ncomp, n), torch.int64, d0.device)
    nat.check(nat.lib().mx_trunc_party_r0(
        nat.dev_of(d0), _words(s0.bits), n, m, ncomp, _roles_arr(roles), nat.ptr(d0),
        nat.ptr(d1), nat.ptr(msg), nat.ptr(msg_rm), nat.ptr(out0), nat.ptr(out1),
        _slots_arr(slots), _nonces_arr(nonces), nat.stream_of(d0)), "trunc_party_r0")
    return msg, msg_rm, out0, out1


def trunc_party_r1(msg, rmk, rrt, rrm, out0, out1, bits, m, roles, slots, nonces,
                   alloc=None):
    """Round 1 (mx_trunc_party_r1): returns w; writes P0's s0 / P1's s1 into out0/out1."""
    ncomp = len(roles)
    n = msg.numel() // ncomp // (2 if bits == 128 else 1)
    w = _new(alloc, msg.shape, msg.dtype, msg.device)
    nat.check(nat.lib().mx_trunc_party_r1(
        nat.dev_of(msg), _words(bits), n, m, ncomp, _roles_arr(roles), nat.ptr(msg),
        nat.ptr(rmk), nat.ptr(rrt), nat.ptr(rrm), nat.ptr(w), nat.ptr(out0), nat.ptr(out1),
        _slots_arr(slots), _nonces_arr(nonces), nat.stream_of(msg)), "trunc_party_r1")
    return w


def ring_extend_party_r0(s0: RT, s1: RT, roles, slots, nonces, alloc=None):
    """Round 0 of the per-party ring extension Z_2^64 -> Z_2^128 (mx_ring_extend_party_r0) on
    stacked [ncomp, ...] shares over Z_2^64.  Returns (msg, msg_R, msg_M, out0, out1): the
    outgoing messages (P0 / P1: msg; the dealer P2: msg_R over Z_2^128 and msg_M) and the
    (partly filled) new shares over Z_2^128.  ``nonces``: r0, r1, R0, M0, z0, z2.  ``alloc``:
    where the messages go."""
    if s0.bits != 64 or s1.bits != 64:
        raise TypeError("ring_extend_party_r0: expects shares over Z_2^64")
    ncomp = len(roles)
    d0 = s0.data.contiguous()
    d1 = s1.data.contiguous()
    n = math.prod(s0.shape) // ncomp
    wide = tuple(d0.shape) + (2,)
    msg = _new(alloc, d0.shape, torch.int64, d0.device)
    msg_R = _new(alloc, wide, torch.int64, d0.device)
    msg_M = _new(alloc, d0.shape, torch.int64, d0.device)
    out0 = torch.empty(wide, dtype=torch.int64, device=d0.device)
    out1 = torch.empty(wide, dtype=torch.int64, device=d0.device)
    nat.check(nat.lib().mx_ring_extend_party_r0(
        nat.dev_of(d0), n, ncomp, _roles_arr(roles), nat.ptr(d0), nat.ptr(d1), nat.ptr(msg),
        nat.ptr(msg_R), nat.ptr(msg_M), nat.ptr(out0), nat.ptr(out1), _slots_arr(slots),
        _nonces_arr(nonces), nat.stream_of(d0)), "ring_extend_party_r0")
    return msg, msg_R, msg_M, out0, out1


def ring_extend_party_r1(msg, rmk, rR, rM, out0, out1, roles, slots, nonces, alloc=None):
    """Round 1 (mx_ring_extend_party_r1): returns w (over Z_2^128); writes P0's s0 / P1's s1
    into out0 / out1."""
    ncomp = len(roles)
    n = msg.numel() // ncomp
    w = _new(alloc, tuple(msg.shape) + (2,), torch.int64, msg.device)
    nat.check(nat.lib().mx_ring_extend_party_r1(
        nat.dev_of(msg), n, ncomp, _roles_arr(roles), nat.ptr(msg), nat.ptr(rmk), nat.ptr(rR),
        nat.ptr(rM), nat.ptr(w), nat.ptr(out0), nat.ptr(out1), _slots_arr(slots),
        _nonces_arr(nonces), nat.stream_of(msg)), "ring_extend_party_r1")
    return w


SHARE_MIRROR = 8  # MX_SHARE_MIRROR (moosex.h): the masked slot goes to P_{j+2}


def share_party(kind: str, x: RT, ncomp: int, rel, slots, n1: int, na: int, mirror=False,
                alloc=None, msg_slot=None):
    """Per-component slots of a sharing by member j (mx_share_party); the owner's out1
    (slot x_{j+1}) is the message to P_{j+1} (whose out0 it becomes).  A pending
    :class:`Encoded` input is encoded inside the kernel.  ``alloc``: two separate buffers
    (a receiver lands its slot whole), slot ``msg_slot`` (the owner's message) from
    ``alloc(shape, dtype)``."""
    code, xd, aux = share_source(x, kind)
    na = na if aux is None else aux
    if alloc is None:
        out0, out1 = empty2((ncomp,) + tuple(x.shape), x.bits, xd.device)
        out0, out1 = out0.data, out1.data
    else:
        out0, out1 = (_empty_in(alloc if s == msg_slot else None, (ncomp,) + tuple(x.shape),
                                x.bits, xd.device).data for s in (0, 1))
    nat.check(nat.lib().mx_share_party(
        nat.dev_of(xd), code | (SHARE_MIRROR if mirror else 0), _words(x.bits), x.numel(), ncomp,
        _roles_arr(rel), nat.ptr(xd), nat.ptr(out0), nat.ptr(out1), _slots_arr(slots),
        n1 & MASK64, na & MASK64, nat.stream_of(xd)), "share_party")
    return out0, out1


# ---------------------------------------------------------------------------
# fixed-point dot tail, per party (csrc/rss_party.hip; moose_amd/parallel/party.py)
# ---------------------------------------------------------------------------
def _vp(ts):
    """Per-component pointer array (None -> null) of dense tensors."""
    for t in ts:
        if t is not None and not t.is_contiguous():
            raise ValueError("per-component buffers must be dense")
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _dev_stream(ts):
    t = next(t for t in ts if t is not None)
    return nat.dev_of(t), nat.stream_of(t)


def _new(alloc, shape, dtype, device):
    """A message buffer: from ``alloc(shape, dtype)`` (a session's outbox, where the
    receiver reads it in place) or fresh."""
    if alloc is not None:
        return alloc(tuple(shape), dtype)
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def dot_tail_r0(cross, bits, m, roles, slots, nonces, out0, out1, n, dealer=True,
                alloc=None):
    """Round 0 of the per-party dot tail (mx_dot_tail_r0): returns the per-component
    outgoing messages (P0 m0, P1 m1, P2 z2), the dealer's rt1 and rm1 (P2 only); writes
    P2's new shares into out0 / out1.  ``dealer=False``: the dealer's part already ran
    (:func:`dot_tail_dealer`), rt / rm are None.  ``alloc``: where the messages go."""
    msg = [_new(alloc, x.shape, x.dtype, x.device) for x in cross]
    rt = [_new(alloc, x.shape, x.dtype, x.device) if r == 2 and dealer else None
          for x, r in zip(cross, roles)]
    rm = [_new(alloc, (n,), torch.int64, x.device) if r == 2 and dealer else None
          for x, r in zip(cross, roles)]
    dev, st = _dev_stream(cross)
    nat.check(nat.lib().mx_dot_tail_r0(
        dev, _words(bits), n, m, len(roles), _roles_arr(roles), _vp(cross), _vp(msg), _vp(rt),
        _vp(rm), _vp(out0), _vp(out1), _slots_arr(slots), _nonces_arr(nonces), st),
        "dot_tail_r0")
    return msg, rt, rm


def dot_tail_dealer(bits, m, roles, slots, nonces, out0, out1, n, alloc=None):
    """The dealer P2's part of round 0 on its own (mx_dot_tail_r0 without the products):
    it depends on PRF keys and nonces only, so it runs before the product exists and its
    messages rt1 / rm1 travel while the GEMM runs.  Returns (rt, rm) per component (P2's
    components only); writes P2's new shares into out0 / out1."""
    like = [o if r == 2 else None for o, r in zip(out0, roles)]
    rt = [_new(alloc, o.shape, o.dtype, o.device) if o is not None else None for o in like]
    rm = [_new(alloc, (n,), torch.int64, o.device) if o is not None else None for o in like]
    if not any(o is not None for o in like):
        return rt, rm
    only = [r if r == 2 else -1 for r in roles]
    none = [None] * len(roles)
    dev, st = _dev_stream(like)
    nat.check(nat.lib().mx_dot_tail_r0(
        dev, _words(bits), n, m, len(roles), _roles_arr(only), _vp(none), _vp(none), _vp(rt),
        _vp(rm), _vp(out0), _vp(out1), _slots_arr(slots), _nonces_arr(nonces), st),
        "dot_tail_dealer")
    return rt, rm


def dot_tail_r1(msg, rmk, rz, rrt, rrm, bits, m, roles, slots, nonces, out0, out1, n,
                alloc=None):
    """Round 1 (mx_dot_tail_r1): returns w per component (P0, P1); writes P0's s0 and
    P1's s1 into out0 / out1."""
    w = [_new(alloc, x.shape, x.dtype, x.device) if r in (0, 1) else None
         for x, r in zip(msg, roles)]
    dev, st = _dev_stream(msg)
    nat.check(nat.lib().mx_dot_tail_r1(
        dev, _words(bits), n, m, len(roles), _roles_arr(roles), _vp(msg), _vp(rmk), _vp(rz),
        _vp(rrt), _vp(rrm), _vp(w), _vp(out0), _vp(out1), _slots_arr(slots),
        _nonces_arr(nonces), st), "dot_tail_r1")
    return w


def dot_tail_r2(a, b, out, bits, roles, n):
    """out[c] = a[c] + b[c] for the components of P0 and P1 (mx_dot_tail_r2)."""
    if not any(t is not None for t in out):
        return
    dev, st = _dev_stream([t for t in out if t is not None])
    nat.check(nat.lib().mx_dot_tail_r2(dev, _words(bits), n, len(roles), _roles_arr(roles),
                                       _vp(a), _vp(b), _vp(out), st), "dot_tail_r2")


# ---------------------------------------------------------------------------
# the per-party tail over several products at once (csrc/rss_jobs.hip)
# ---------------------------------------------------------------------------
MAX_JOBS = 4


class MulJob:
    """One product of a batched per-party tail: ``rows`` rows of length L (the call's row
    length) with value[r] = cb (x0 y0 + x0 y1 + x1 y0)[r] + ca a[r] + ca2 a2[r], where
    operand rows are read at ``r * stride`` (stride 0: one row broadcast to every row) and
    a / a2 are additive shares (e.g. a party's first share component); the new shares are
    written to the dense rows ``o0`` / ``o1``.  Operands are ring-tensor data (torch)."""

    __slots__ = ("x0", "x1", "y0", "y1", "a", "a2", "o0", "o1", "rows", "sx", "sy", "sa",
                 "sa2", "ca", "ca2", "cb")

    def __init__(self, rows, o0, o1, x=None, y=None, sx=0, sy=0, a=None, sa=0, ca=1, cb=1,
                 a2=None, sa2=0, ca2=1):
        self.rows, self.o0, self.o1 = rows, o0, o1
        self.x0, self.x1 = x if x is not None else (None, None)
        self.y0, self.y1 = y if y is not None else (None, None)
        self.sx, self.sy, self.a, self.sa, self.a2, self.sa2 = sx, sy, a, sa, a2, sa2
        self.ca, self.ca2, self.cb = ca, ca2, (cb if x is not None else 0)


def _jobs_abi(jobs):
    if not 1 <= len(jobs) <= MAX_JOBS:
        raise ValueError(f"1..{MAX_JOBS} jobs per call, got {len(jobs)}")
    ptrs, dims = [], []
    for j in jobs:
        for t in (j.x0, j.x1, j.y0, j.y1, j.a, j.a2, j.o0, j.o1):
            ptrs.append(None if t is None else t.data_ptr())
        for v in (j.rows, j.sx, j.sy, j.sa, j.sa2, j.ca, j.ca2, j.cb):
            v = int(v)
            dims.append(v - (1 << 64) if v >= (1 << 63) else v)
    return (ctypes.c_void_p * len(ptrs))(*ptrs), (ctypes.c_int64 * len(dims))(*dims)


def jobs_r0(jobs, L, bits, m, role, slots, nonces, like, main=True, dealer=True, pend=None,
            alloc=None):
    """Round 0 of the batched per-party tail (mx_jobs_r0): the outgoing message over the
    concatenation of the jobs' rows (P0 m0, P1 m1, P2 z2), the dealer's rt1 / rm1 (P2, when
    ``dealer``), P2's new shares into the jobs' outputs.  ``like``: any tensor of the call's
    device (allocation and stream).  ``pend``: the previous level's round-2 sums still
    pending, [(o, a, b)] with o = a + b elementwise (flat tensors of equal size): operands
    are read through them and they are written too (mx_jobs_r0p)."""
    n = builtins.sum(j.rows for j in jobs) * L
    w = _words(bits)
    shp = (n,) + ((2,) if bits == 128 else ())
    # ``alloc(shape)``: where the outgoing messages go (a session's outbox), else fresh
    new = alloc or (lambda s: torch.empty(s, dtype=torch.int64, device=like.device))
    msg = new(shp) if main else None
    rt = new(shp) if role == 2 and dealer else None
    rm = new((n,)) if role == 2 and dealer else None
    p, d = _jobs_abi(jobs)
    pend = pend or []
    pp = (ctypes.c_void_p * max(1, 3 * len(pend)))(*[t.data_ptr() for r in pend for t in r])
    pl = (ctypes.c_int64 * max(1, len(pend)))(*[r[0].numel() // (2 if bits == 128 else 1)
                                                 for r in pend])
    nat.check(nat.lib().mx_jobs_r0p(
        nat.dev_of(like), w, len(jobs), p, d, L, m, role, int(main), int(dealer),
        None if msg is None else msg.data_ptr(), None if rt is None else rt.data_ptr(),
        None if rm is None else rm.data_ptr(), _slots_arr(slots), _nonces_arr(nonces),
        len(pend), pp, pl, nat.stream_of(like)), "jobs_r0")
    return msg, rt, rm


def jobs_r1(jobs, L, bits, m, role, slots, nonces, msg, rmk, rz, rrt, rrm, alloc=None):
    """Round 1 (mx_jobs_r1): P0 / P1 open c from their message, the other's and z2; returns
    w (P0 w0, P1 w1; None for P2) and writes P0's o0 = z0, P1's o1 = z2.  ``alloc``: where
    w goes (the session's outbox)."""
    if role == 2:
        return None
    w = alloc(tuple(msg.shape)) if alloc is not None else torch.empty_like(msg)
    p, d = _jobs_abi(jobs)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    nat.check(nat.lib().mx_jobs_r1(
        nat.dev_of(msg), _words(bits), len(jobs), p, d, L, m, role, ptr(msg), ptr(rmk), ptr(rz),
        ptr(rrt), ptr(rrm), w.data_ptr(), _slots_arr(slots), _nonces_arr(nonces),
        nat.stream_of(msg)), "jobs_r1")
    return w


def jobs_r2(jobs, L, bits, role, a, b):
    """Round 2 (mx_jobs_r2): P0's o1 / P1's o0 = w0 + w1."""
    if role == 2:
        return
    p, d = _jobs_abi(jobs)
    nat.check(nat.lib().mx_jobs_r2(nat.dev_of(a), _words(bits), len(jobs), p, d, L, role,
                                   a.data_ptr(), b.data_ptr(), nat.stream_of(a)), "jobs_r2")


# ---------------------------------------------------------------------------
# per-party bit decomposition front and B2A (csrc/rss_bits_party.hip, bits_party.h)
# ---------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


def bits_front(role, xa, xb, arecv, bits, slots, n1, ng, alloc=None):
    """This party's adder inputs of the bit decomposition of (xa, xb) (its two arithmetic
    components, torch data): (message a1 (P0) or None, z (its zero-shared AND term, the
    reshare message), p0, p1.  ``alloc``: where the messages go)."""
    like = next(t for t in (xa, xb, arecv) if t is not None)
    n = like.numel() // (2 if bits == 128 else 1)
    p0, p1 = torch.empty_like(like), torch.empty_like(like)
    msg = _new(alloc, like.shape, like.dtype, like.device) if role == 0 else None
    z = _new(alloc, like.shape, like.dtype, like.device)
    nat.check(nat.lib().mx_bits_front(
        nat.dev_of(like), _words(bits), role, n, _p(xa), _p(xb), _p(arecv), _p(msg), _p(z),
        _p(p0), _p(p1), _slots_arr(slots), _nonces_arr((n1, ng)), nat.stream_of(like)),
        "bits_front")
    return msg, z, p0, p1


def bits_b2a(phase, role, src, start, count, bits, slots, n1, ng, arecv=None, state=None,
             xbit=-1, blocks=1, alloc=None):
    """B2A of bit planes start.. of a boolean sharing (src = (s0, s1, g0, g1, t0, t1) torch
    data of one party; g = None: s are the sum words), phases 0 / 1 / 2 (bits_party.h).
    ``xbit`` >= 0: rows 0..count-2 are planes start.. XORed with plane xbit, the last row is
    plane xbit; ``blocks`` > 1: the source holds that many blocks of the output's elements and
    the last ``blocks`` rows are plane xbit of each (bits_party.h plane_of).  Phases 0 / 1
    return state (msg, z, base0, base1);
    phase 2 (state + the received z in ``arecv``) returns the result pair [count, ...]."""
    like = next(t for t in src if t is not None) if src is not None else state[1]
    per = tuple(like.shape[:-1] if bits == 128 else like.shape) if src is not None else None
    if phase == 2:
        msg, z, b0, b1 = state
        S = z.numel() // (2 if bits == 128 else 1) // count
        o0, o1 = torch.empty_like(z), torch.empty_like(z)
        nat.check(nat.lib().mx_bits_b2a(
            nat.dev_of(z), _words(bits), 2, role, S, start, count, xbit, blocks, None, None,
            None, _p(z),
            _p(b0), _p(b1), _p(arecv), _p(o0), _p(o1), _slots_arr(slots), _nonces_arr((n1, ng)),
            nat.stream_of(z)), "bits_b2a")
        return o0, o1
    nb = blocks & 0xff  # bits_party.h plane_of: blocks >> 8 is the tail rows' sign plane
    if nb > 1:  # ``nb`` copies concatenated on axis 0: the rows are one block's
        per = (per[0] // nb,) + per[1:]
    S = math.prod(per)
    shp = (count,) + per + ((2,) if bits == 128 else ())
    b0, b1 = (torch.empty(shp, dtype=torch.int64, device=like.device) for _ in range(2))
    msg = _new(alloc, shp, torch.int64, like.device) if role == 0 else None
    z = _new(alloc, shp, torch.int64, like.device)
    srcs = (ctypes.c_void_p * 6)(*[_p(t) for t in src])
    nat.check(nat.lib().mx_bits_b2a(
        nat.dev_of(like), _words(bits), phase, role, S, start, count, xbit, blocks, srcs,
        _p(arecv),
        _p(msg),
        _p(z), _p(b0), _p(b1), None, None, None, _slots_arr(slots), _nonces_arr((n1, ng)),
        nat.stream_of(like)), "bits_b2a")
    return msg, z, b0, b1


def _ring_words(values, bits):
    """Python ints -> a ctypes int64 array of their little-endian 64-bit words (mod 2^bits)."""
    w = _words(bits)
    out = []
    for v in values:
        v = int(v) % (1 << bits)
        for j in range(w):
            out.append(_to_i64((v >> (64 * j)) & MASK64))
    return (ctypes.c_int64 * max(1, len(out)))(*out)


def wsum_pair(bits, L, rows=None, weights=(), x=None, wx=0, pub=(False, False), cblk=(0,),
              second=None, like=None, lead=False):
    """Per-party fused weighted sums over both share components (csrc/wsum_pair.h):
    s_c = sum_k weights[k] rows_c[k] + wx x_c; returns (o0, o1) of nblk = len(cblk) blocks
    of L elements, block b = s_c + cblk[b] on the public slots ``pub`` (this party's copies
    of x_0), and with ``second`` = (m2, c2) also (q0, q1) = m2 s_c + c2 on those slots.
    ``rows`` = (r0, r1) tensors holding len(weights) rows of L elements, contiguous.
    ``lead``: (q0, q1) is block 0 of the outputs instead -- (o0, o1) of 1 + nblk blocks,
    no concatenation afterwards."""
    ref = like if like is not None else (rows[0] if rows is not None else x[0])
    nrows = len(weights)
    if nrows > 64 or not 1 <= len(cblk) <= 3:
        raise ValueError("wsum_pair: at most 64 rows and 3 blocks")
    dev = ref.device
    tail = (2,) if bits == 128 else ()
    q0 = q1 = None
    if lead:
        if second is None:
            raise ValueError("wsum_pair: lead needs second")
        b0 = torch.empty(((1 + len(cblk)) * L,) + tail, dtype=torch.int64, device=dev)
        b1 = torch.empty_like(b0)
        q0, q1, o0, o1 = b0[:L], b1[:L], b0[L:], b1[L:]
    else:
        o0 = torch.empty((len(cblk) * L,) + tail, dtype=torch.int64, device=dev)
        o1 = torch.empty_like(o0)
    if second is not None and not lead:
        q0 = torch.empty(((L,) + tail), dtype=torch.int64, device=dev)
        q1 = torch.empty_like(q0)
    r = [None, None] if rows is None else [t.contiguous() for t in rows]
    xx = [None, None] if x is None else [t.contiguous() for t in x]
    m2, c2 = second if second is not None else (0, 0)
    nat.check(nat.lib().mx_wsum_pair(
        nat.dev_of(o0), _words(bits), nrows, len(cblk), 1 if second is not None else 0,
        1 if pub[0] else 0, 1 if pub[1] else 0, L, L, _ring_words(weights, bits),
        _ring_words([wx], bits), _ring_words([m2], bits), _ring_words([c2], bits),
        _ring_words(cblk, bits), _p(r[0]), _p(r[1]), _p(xx[0]), _p(xx[1]), _p(o0), _p(o1),
        _p(q0), _p(q1), nat.stream_of(o0)), "wsum_pair")
    if lead:
        return b0, b1
    return (o0, o1) if second is None else (o0, o1, q0, q1)
