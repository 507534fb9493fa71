"""Host-level primitive operations (the leaf kernels of a lowered graph).

Each primitive has a name -- the operator kind it becomes in a lowered computation
(``Add``, ``Dot``, ``SampleSeeded`` ... and this framework's fused extensions
``RingMulCross``/``RingDotCross``/``BitAndCross``/``ZeroShare``) -- an eager
implementation on python/torch values, and a result-type rule used by the symbolic
session.  Eager values are:

* :class:`moose_amd.ops.ring.RT` for ring / bit tensors,
* ``torch.Tensor`` for plaintext host tensors (float, int, uint, bool),
* ``tuple`` for shapes, ``bytes`` for PRF keys / seeds, ``str`` for strings.

Implementations take ``nb`` -- the number of leading batch dims (1 when the three
parties of a session are stacked on one device) -- so axis attributes stay logical.

Parity: the ``runtime`` flavour rows of the reference dispatch tables
(``moose/src/kernels/*.rs``) are the host kernels in ``moose/src/host/ops.rs``.
"""
from __future__ import annotations

import math

import torch

from moose_amd.ir import types as T
from moose_amd.ops import ring as R


class Prim:
    __slots__ = ("name", "impl", "ty")

    def __init__(self, name, impl, ty=None):
        self.name = name
        self.impl = impl
        self.ty = ty or (lambda tys, **a: tys[0])


PRIMS = {}


def prim(name, ty=None):
    def deco(fn):
        PRIMS[name] = Prim(name, fn, ty)
        return fn

    return deco


def _is_rt(x):
    return isinstance(x, R.RT)


def _tensorish(x):
    return isinstance(x, (R.RT, torch.Tensor))


# ---------------------------------------------------------------------------
# arithmetic (ring or plaintext)
# ---------------------------------------------------------------------------
def _arith(op):
    def impl(nb, a, b):
        if _is_rt(a) or _is_rt(b):
            return R.binary(op, a, b)
        if op == "add":
            return a + b
        if op == "sub":
            return a - b
        if op == "mul":
            return a * b
        if op == "and":
            return a & b
        if op == "or":
            return a | b
        if op == "xor":
            return a ^ b
        raise AssertionError(op)

    return impl


prim("Add")(_arith("add"))
prim("Sub")(_arith("sub"))
prim("Mul")(_arith("mul"))
prim("And")(_arith("and"))
prim("Or")(_arith("or"))
prim("Xor")(_arith("xor"))


@prim("MulLeading")
def _mul_leading(nb, a, c):
    """a[..., i, ...] * c[i] along the first non-party axis of ``a`` (``c`` 1-D public):
    a rank-agnostic scaling, so shape-polymorphic lowering can express it."""
    if not _is_rt(a):
        k = a.dim() - nb - 1
        return a * c.reshape((c.shape[0],) + (1,) * k)
    return R.mul_leading(a, c, nb)


@prim("Neg")
def _neg(nb, a):
    if _is_rt(a):  # on bit tensors Neg is NOT (reference host/ops.rs:1519-1527)
        return ~a if a.bits == 1 else -a
    if a.dtype == torch.bool:
        return ~a
    return -a


@prim("Div")
def _div(nb, a, b):
    if _is_rt(a):
        return _ring_div(a, b)
    if a.dtype in (torch.float32, torch.float64):
        return a / b
    return torch.div(a, b, rounding_mode="trunc")


def _ring_div(a, b):
    """Unsigned integer division of ring tensors (``Wrapping<u64> / Wrapping<u128>``,
    reference host/ops.rs:334-343).  A host-only kernel on python integers: no protocol
    divides ring values, so it is never on a hot path."""
    import numpy as np

    x, y = R.to_ints(a), R.to_ints(b)
    x, y = np.broadcast_arrays(x, y)
    if any(int(v) == 0 for v in y.reshape(-1)):
        raise ZeroDivisionError("ring division by zero")
    q = np.vectorize(lambda u, v: int(u) // int(v), otypes=[object])(x, y)
    return R.from_ints(q, a.bits, a.device)


@prim("Shl")
def _shl(nb, a, amount):
    return a.shl(amount)


@prim("Shr")
def _shr(nb, a, amount):
    return a.shr(amount)


@prim("Sar")
def _sar(nb, a, amount):
    return a.sar(amount)


@prim("Dot")
def _dot(nb, a, b):
    if _is_rt(a):
        return R.dot(a, b, nb)
    if nb:
        return torch.matmul(a, b)
    if a.dim() <= 2 and b.dim() <= 2:
        return a @ b if (a.dim() > 0 and b.dim() > 0) else a * b
    return torch.tensordot(a, b, dims=([a.dim() - 1], [0]))


@prim("Sum", ty=lambda tys, **a: tys[0])
def _sum(nb, a, axis=None):
    if _is_rt(a):
        return R.sum(a, axis, nb)
    if axis is None:
        return a.reshape(a.shape[:nb] + (-1,)).sum(dim=nb) if nb else a.sum()
    return a.sum(dim=_lax(a.dim(), axis, nb))


def _lax(ndim, axis, nb):
    nd = ndim - nb
    return (axis + nd if axis < 0 else axis) + nb


@prim("AddN")
def _addn(nb, *xs):
    acc = xs[0]
    for x in xs[1:]:
        acc = _arith("add")(nb, acc, x)
    return acc


@prim("Mean")
def _mean(nb, a, axis=None):
    if axis is None:
        return a.mean() if not nb else a.reshape(a.shape[:nb] + (-1,)).mean(dim=nb)
    return a.mean(dim=_lax(a.dim(), axis, nb))


@prim("RingFixedpointMean")
def _ring_fixedpoint_mean(nb, a, axis=None, scaling_base=2, scaling_exp=0):
    """Sum along ``axis`` (all entries when None) times the mean weight 1/n encoded with
    scaling_base^scaling_exp -- the float product truncated toward zero, as the
    reference's encode (host/fixedpoint.rs:66-76, 10-38).  No truncation of the product:
    the result carries twice the fractional bits, as the reference's."""
    shape = a.shape[nb:]
    n = shape[axis] if axis is not None else math.prod(shape)
    w = int((1.0 / n) * float(int(scaling_base) ** int(scaling_exp)))
    s = R.sum(a, axis, nb)
    return R.binary("mul", s, R.fill((), w % (1 << a.bits), a.bits, a.device))


@prim("RingFixedpointArgmax", ty=lambda tys, **a: T.Ty("HostRing64Tensor"))
def _ring_fixedpoint_argmax(nb, a, axis, upmost_index=None):
    """Index of the first maximum along ``axis``, entries read as signed ring values; a
    Z_2^64 tensor of indices (reference host/ops.rs:2374-2445)."""
    ax = _lax(a.ndim, axis, nb)
    d = a.data
    n = d.shape[ax]
    hi = d.select(ax, 0)
    lo = None
    if a.bits == 128:  # (lo, hi) words: signed high word, unsigned low word
        lo = hi[..., 0] ^ _SIGN64
        hi = hi[..., 1]
    best_hi, best_lo = hi.clone(), None if lo is None else lo.clone()
    idx = torch.zeros(best_hi.shape, dtype=torch.int64, device=d.device)
    for i in range(1, n):
        v = d.select(ax, i)
        if a.bits == 128:
            vl, vh = v[..., 0] ^ _SIGN64, v[..., 1]
            gt = (vh > best_hi) | ((vh == best_hi) & (vl > best_lo))
            best_lo = torch.where(gt, vl, best_lo)
        else:
            vh = v
            gt = vh > best_hi
        best_hi = torch.where(gt, vh, best_hi)
        idx = torch.where(gt, torch.full_like(idx, i), idx)
    return R.RT(idx.contiguous(), 64)


_SIGN64 = -(1 << 63)


# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------
@prim("Shape", ty=lambda tys, **a: T.HOST_SHAPE)
def _shape(nb, a):
    if _is_rt(a):
        return tuple(a.shape[nb:])
    return tuple(a.shape[nb:])


@prim("Reshape")
def _reshape(nb, a, shape=None):
    if _is_rt(a):
        return R.reshape(a, shape, nb)
    return a.reshape(tuple(a.shape[:nb]) + tuple(shape))


@prim("ExpandDims")
def _expand_dims(nb, a, axis):
    if _is_rt(a):
        return R.expand_dims(a, axis, nb)
    d = a
    nd = a.dim() - nb
    for ax in sorted(axis):
        if ax < 0:
            ax += nd + 1
        d = d.unsqueeze(ax + nb)
        nd += 1
    return d


@prim("Squeeze")
def _squeeze(nb, a, axis=None):
    if _is_rt(a):
        return R.squeeze(a, axis, nb)
    if axis is None:
        keep = list(a.shape[:nb]) + [s for s in a.shape[nb:] if s != 1]
        return a.reshape(keep)
    return a.squeeze(_lax(a.dim(), axis, nb))


@prim("Transpose")
def _transpose(nb, a):
    if _is_rt(a):
        return R.transpose(a, nb)
    nd = a.dim() - nb
    perm = list(range(nb)) + [nb + i for i in reversed(range(nd))]
    return a.permute(perm).contiguous()


@prim("Concat")
def _concat(nb, *xs, axis=0):
    if _is_rt(xs[0]):
        return R.concat(xs, axis, nb)
    return torch.cat(xs, dim=_lax(xs[0].dim(), axis, nb))


@prim("IndexAxis")
def _index_axis(nb, a, axis, index):
    if _is_rt(a):
        return R.index_axis(a, axis, index, nb)
    return a.select(_lax(a.dim(), axis, nb), index).contiguous()


@prim("Slice")
def _slice(nb, a, slice):
    if isinstance(slice, list):  # one (start, end, step) per leading axis
        return _strided_slice(nb, a, [builtins_slice(*s) for s in slice])
    start, end, step = slice
    if isinstance(a, tuple):  # a shape (HostShape slice, reference host/ops.rs Slice)
        return a[start:end:step]
    if _is_rt(a):
        return R.slice_axis(a, 0, start, end, step, nb)
    idx = [builtins_slice(None)] * nb + [builtins_slice(start, end, step)]
    return a[tuple(idx)].contiguous()


builtins_slice = slice


@prim("Permute")
def _permute(nb, a, perm=None, axes=None):
    perm = list(axes if perm is None else perm)  # `axes` is the IR operator's attribute
    rank = (a.ndim if _is_rt(a) else a.dim()) - nb
    if sorted(perm) != list(range(rank)):
        raise ValueError(f"Permute: axes {perm} are not a permutation of the tensor's axes")
    if _is_rt(a):
        return R.transpose(a, nb, perm)
    return a.permute(list(range(nb)) + [p + nb for p in perm]).contiguous()


@prim("Im2Col")
def _im2col(nb, a, kernel_shape, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
            data_format="NCHW"):
    """Patch matrix [N*OH*OW, C*KH*KW] of a rank-4 tensor (R.im2col): ring tensors through
    the native gather, plain tensors through pad + as_strided + contiguous."""
    if _is_rt(a):
        return R.im2col(a, kernel_shape, strides, pads, dilations, data_format, nb)
    geom = R.im2col_geometry(tuple(a.shape[nb:]), kernel_shape, strides, pads, dilations,
                             data_format)
    return R.im2col_torch(a, geom, data_format, nb)


@prim("Col2Im")
def _col2im(nb, a, image_shape, kernel_shape, strides=(1, 1), pads=(0, 0, 0, 0),
            dilations=(1, 1), data_format="NCHW"):
    """Image [N, C, H, W] (NHWC: [N, H, W, C]) summed from the patch matrix [N*OH*OW,
    C*KH*KW] (R.col2im, the adjoint of Im2Col): ring tensors through the native gather, plain
    float tensors through F.fold + crop."""
    image_shape = tuple(image_shape)
    if _is_rt(a):
        return R.col2im(a, image_shape, kernel_shape, strides, pads, dilations, data_format, nb)
    if a.dtype == torch.bool:
        raise ValueError("Col2Im sums its input: a bool tensor has no col2im")
    geom = R.col2im_geometry(tuple(a.shape[nb:]), image_shape, kernel_shape, strides, pads,
                             dilations, data_format)
    return R.col2im_torch(a, geom, data_format, nb)


@prim("Resize")
def _resize(nb, a, sizes, mode="nearest", coordinate_transformation_mode="half_pixel",
            nearest_mode="round_prefer_floor", scales=(), weight_bits=(0, 0),
            data_format="NCHW"):
    """Rank-4 image resized to sizes = (OH, OW) with public coordinates (R.resize): ring
    tensors through the native stencil, exactly and without truncation (a linear result has
    weight_bits more fractional bits); plain tensors through the torch composition over the
    same tables -- floats with the weights over 2^weight_bits, bools in nearest mode only."""
    sizes, scales, weight_bits = tuple(sizes), tuple(scales), tuple(weight_bits)
    if _is_rt(a):
        return R.resize(a, sizes, mode, coordinate_transformation_mode, nearest_mode, scales,
                        weight_bits, data_format, nb)
    geom = R.resize_geometry(tuple(a.shape[nb:nb + 4]), sizes, mode,
                             coordinate_transformation_mode, nearest_mode, scales, weight_bits,
                             data_format)
    if a.dtype == torch.bool and mode != "nearest":
        raise ValueError("Resize: a weighted sum of bits is not a bit; `linear` on a bool "
                         "tensor")
    return R.resize_torch(a, geom, mode, coordinate_transformation_mode, nearest_mode,
                          data_format, nb)


@prim("DepthwiseConv")
def _dwconv(nb, x, w, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1), data_format="NCHW"):
    """Depthwise convolution of a rank-4 x with w = [C*mult, 1, KH, KW] (R.dwconv): ring
    tensors through the native stencil kernel, plain float tensors through
    ``torch.nn.functional.conv2d(groups=C)``."""
    if _is_rt(x) or _is_rt(w):
        if not (_is_rt(x) and _is_rt(w)):
            raise TypeError("DepthwiseConv: a ring tensor and a plain tensor do not combine")
        return R.dwconv(x, w, strides, pads, dilations, data_format, nb)
    if nb:
        raise ValueError("DepthwiseConv of plain tensors takes no batch dims")
    g = R.dwconv_geometry(tuple(x.shape), tuple(w.shape), strides, pads, dilations, data_format)
    C, (pt, pl, pb, pr) = g[1], g[9:13]
    nhwc = data_format == "NHWC"
    xc = x.permute(0, 3, 1, 2) if nhwc else x
    xc = torch.nn.functional.pad(xc, (pl, pr, pt, pb))
    y = torch.nn.functional.conv2d(xc, w.to(xc.dtype), stride=tuple(strides),
                                   dilation=tuple(dilations), groups=C)
    return y.permute(0, 2, 3, 1).contiguous() if nhwc else y


@prim("DepthwiseConvCross")
def _dwconv_cross(nb, x0, x1, w0, w1, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
                  data_format="NCHW"):
    """The replicated local product of a depthwise convolution, x0 * (w0 + w1) + x1 * w0 over
    the taps in one pass (R.dwconv_cross)."""
    return R.dwconv_cross(x0, x1, w0, w1, strides, pads, dilations, data_format, nb)


@prim("PwlPlain")
def _pwl_plain(nb, s, x, da, db, ak):
    """The plain piecewise-linear leaf on ring tensors (R.pwl): (ak + sum_j da[j] * s[j]) * x +
    sum_j db[j] * s[j] over the flag planes s stacked on the leading logical axis."""
    return R.pwl(s, x, tuple(da), tuple(db), int(ak), nb)


@prim("CswapDiff")
def _cswap_diff(nb, x, geom):
    """The signed differences of one compare-exchange stage (R.cswap_diff): negative where a
    pair is out of order."""
    return R.cswap_diff(x, R.CswapGeom(*geom), nb)


@prim("CswapApply")
def _cswap_apply(nb, x, p, geom):
    """The exchange of one compare-exchange stage (R.cswap_apply): x[i] - p, x[l] + p."""
    return R.cswap_apply(x, p, R.CswapGeom(*geom), nb)


@prim("Scan")
def _scan(nb, x, geom):
    """The prefix sums of a ring tensor seen as [outer, n, inner] (R.scan)."""
    return R.scan(x, R.ScanGeom(*geom), nb)


@prim("SegscanApply")
def _segscan_apply(nb, x, p, geom):
    """The update of one stage of a segmented scan (R.segscan_apply)."""
    return R.segscan_apply(x, p, R.SegscanGeom(*geom), nb)


def _axis_geom(shape, axis, what):
    nd = len(shape)
    if isinstance(axis, bool) or not isinstance(axis, int) or nd < 1 or not -nd <= axis < nd:
        raise ValueError(f"{what}: axis {axis!r} out of range for a tensor of rank {nd}")
    axis %= nd
    return axis, (math.prod(shape[:axis]), shape[axis], math.prod(shape[axis + 1:]))


@prim("CumSum")
def _cumsum(nb, x, axis=0, exclusive=False, reverse=False):
    """Plaintext prefix sums of a host's tensor along ``axis``: floats through torch.cumsum,
    fixed-point ring values through R.scan (exact, wrapping in the ring)."""
    axis, geom = _axis_geom(tuple(x.shape[nb:]), axis, "cumsum")
    if _is_rt(x):
        return R.scan(x, R.ScanGeom(*geom, bool(exclusive), bool(reverse)), nb)
    ax = axis + nb
    d = x.flip(ax) if reverse else x
    c = torch.cumsum(d, dim=ax)
    if exclusive:  # shifted, not subtracted: floats do not cancel exactly
        c = torch.cat([torch.zeros_like(c.narrow(ax, 0, 1)), c.narrow(ax, 0, c.shape[ax] - 1)],
                      dim=ax) if c.shape[ax] else c
    return c.flip(ax) if reverse else c


@prim("GroupBySum")
def _group_by_sum(nb, x, by=0, count=False, one=1):
    """Plaintext group-by of a host's table [n, c] -- the specification of the secure path:
    the rows sorted by column ``by``; the LAST row of every run of equal keys holds the key,
    the sums of the other columns over the run, the run's length times ``one`` where ``count``,
    and ``one`` (valid); every other row is zero.  [n, c + count + 1].  ``one`` is the
    encoding of 1: 1.0 for floats, 2^frac for the ring values of a fixed-point tensor."""
    rt = _is_rt(x)
    if nb or len(x.shape) != 2 or not 0 <= by < x.shape[1]:
        raise ValueError(f"group_by_sum takes a rank-2 table with more than {by} columns, found "
                         f"shape {tuple(x.shape)}")
    n, c = x.shape
    s = _sort(0, x, axis=0, by=by)
    d = s.data if rt else s
    w128 = rt and x.bits == 128
    ncol = c + int(bool(count)) + 1
    tail = (2,) if w128 else ()
    if n == 0:
        out = torch.zeros((n, ncol) + tail, dtype=d.dtype, device=d.device)
        return R.RT(out, x.bits) if rt else out
    # Every step keeps the shape [n, ...] whatever the data: nothing waits for the device.
    key = d[:, by]
    same = key[1:] == key[:-1]
    if w128:
        same = same.all(dim=-1)
    first = torch.ones(n, dtype=torch.bool, device=d.device)
    last = torch.ones(n, dtype=torch.bool, device=d.device)
    first[1:] = ~same
    last[:-1] = ~same
    vals = torch.cat([d[:, :by], d[:, by + 1:]], dim=1)  # (no index list: no upload)
    if rt:
        ones = R.fill((n, 1), int(one), x.bits, d.device).data
    else:
        ones = torch.full((n, 1), one, dtype=d.dtype, device=d.device)
    if count:
        vals = torch.cat([vals, ones], dim=1)
    nv = vals.shape[1]
    cols = [key.unsqueeze(1)]
    if nv and rt:
        # the prefix sums less those at the end of the run before: exact in the ring
        idx = torch.arange(n, device=d.device)
        start = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), 0).values
        cs = R.scan(R.RT(vals.contiguous(), x.bits), R.ScanGeom(1, n, nv))
        prev = cs.data[(start - 1).clamp(min=0)]
        none = (start == 0).reshape((n,) + (1,) * (prev.dim() - 1))
        prev = torch.where(none, torch.zeros_like(prev), prev)
        cols.append(R.binary("sub", cs, R.RT(prev.contiguous(), x.bits)).data)
    elif nv:  # every run summed on its own
        gid = torch.cumsum(first.to(torch.int64), 0) - 1
        runs = torch.zeros((n, nv), dtype=d.dtype, device=d.device).index_add_(0, gid, vals)
        cols.append(runs[gid])
    cols.append(ones)
    row = torch.cat(cols, dim=1)
    keep = last.reshape((n,) + (1,) * (row.dim() - 1))
    out = torch.where(keep, row, torch.zeros_like(row))
    return R.RT(out, x.bits) if rt else out


def _plain_index(idx, n, frac):
    """The indices a host's tensor holds, as int64 in [0, 2^w), w = max(1, ceil(log2 n)): bit t
    of a uint64 tensor, bit frac + t of a fixed-point tensor's ring values (fractional bits
    and higher bits are ignored, as on the replicated placement)."""
    w = max(1, (int(n) - 1).bit_length())
    if _is_rt(idx):
        if idx.bits == 1 or frac + w > 63:
            raise ValueError(f"an index of {w} bits above {frac} fractional bits in a "
                             f"{idx.bits}-bit tensor is not supported")
        v = (idx.data[..., 0] if idx.bits == 128 else idx.data) >> frac
    else:
        v = idx.to(torch.int64)
    return v & ((1 << w) - 1)


def _plain_ring(x, one, bits):
    """An integer tensor times ``one`` as a ring tensor of ``bits`` (0: as float64)."""
    if not bits:
        return x.to(torch.float64) * float(one)
    lo = x.to(torch.int64) * int(one)
    return R.RT(lo if bits == 64 else torch.stack([lo, torch.zeros_like(lo)], dim=-1), bits)


@prim("OneHot")
def _one_hot(nb, idx, depth=1, idx_frac=0, one=1, bits=0):
    """Plaintext one-hot rows [..., depth] of a host's indices -- the specification of the
    secure path: ``one`` at column idx, 0 elsewhere, all zeros where idx >= depth."""
    v = _plain_index(idx, depth, idx_frac)
    cols = torch.arange(int(depth), device=v.device)
    return _plain_ring(v.unsqueeze(-1) == cols, one, bits)


@prim("Lookup")
def _lookup(nb, table, idx, idx_frac=0):
    """Plaintext ``table[idx]`` of a host's table [n, d] or [n]: the rows the indices name, 0
    where idx >= n."""
    rt = _is_rt(table)
    if len(table.shape) not in (1, 2):
        raise ValueError(f"lookup takes a table [n, d] or [n], found shape {tuple(table.shape)}")
    n = table.shape[0]
    v = _plain_index(idx, n, idx_frac)
    d = table.data if rt else table
    got = d[v.clamp(max=n - 1)]
    keep = (v < n).reshape(tuple(v.shape) + (1,) * (got.dim() - v.dim()))
    out = torch.where(keep, got, torch.zeros_like(got))
    return R.RT(out.contiguous(), table.bits) if rt else out


@prim("BinCount")
def _bincount(nb, idx, weights=None, length=1, idx_frac=0, one=1, bits=0):
    """Plaintext histogram of a host's indices over ``length`` bins: the counts times ``one``
    [length], or with weights [rows, d] / [rows] the sums of the weights per bin, exact in the
    ring; an idx >= length is counted nowhere."""
    n = int(length)
    v = _plain_index(idx, n, idx_frac).reshape(-1)
    oh = v.unsqueeze(-1) == torch.arange(n, device=v.device)  # [rows, n]
    if weights is None:
        return _plain_ring(oh.sum(0), one, bits)
    wshape = tuple(weights.shape)
    if len(wshape) not in (1, 2) or wshape[0] != v.shape[0]:
        raise ValueError(f"bincount: {v.shape[0]} indices take weights [{v.shape[0]}, d] or "
                         f"[{v.shape[0]}], found shape {wshape}")
    if not _is_rt(weights):
        return oh.to(weights.dtype).t() @ weights
    rows, d = wshape[0], (wshape[1] if len(wshape) == 2 else 1)
    sel = R.broadcast_to(_plain_ring(oh.unsqueeze(-1), 1, weights.bits), (rows, n, d))
    w = R.broadcast_to(R.reshape(weights, (rows, 1, d)), (rows, n, d))
    out = R.sum(R.binary("mul", sel, w), 0)
    return out if len(wshape) == 2 else R.reshape(out, (n,))


@prim("PermFromKeys", ty=lambda tys, **a: T.Ty("HostUint64Tensor"))
def _perm_from_keys(nb, keys):
    """The permutation that stably sorts a Z_2^64 vector of PRF output as unsigned integers
    (R.perm_from_keys): what both holders of a PRF key derive alike in a shuffle step."""
    return R.perm_from_keys(keys)


PERM_GATHER_FORMS = {"": (), "b": ("b",), "p": ("plus",), "m": ("minus",), "bp": ("b", "plus"),
                     "bm": ("b", "minus"), "pm": ("plus", "minus"),
                     "bpm": ("b", "plus", "minus")}


@prim("PermGather")
def _perm_gather(nb, a, perm, *rest, axis=0, form=""):
    """Rows of ``a`` gathered along ``axis`` through ``perm`` with the sums of a shuffle step
    (R.perm_gather).  ``form`` names the optional operands that follow ``perm``, in order:
    ``b`` (gathered and added), ``p`` (added in place), ``m`` (subtracted in place)."""
    names = PERM_GATHER_FORMS.get(form)
    if names is None or len(names) != len(rest):
        raise ValueError(f"PermGather: form {form!r} does not name its {len(rest)} optional "
                         "operand(s)")
    return R.perm_gather(a, perm, axis=int(axis), nb=nb, **dict(zip(names, rest)))


@prim("Sort")
def _sort(nb, x, axis=-1, descending=False, by=-1):
    """Plaintext sort of a host's tensor along ``axis`` -- floats, or fixed-point ring values by
    their signed value; ``by >= 0``: the rows of a rank-2 tensor ordered by column ``by``."""
    rt = _is_rt(x)
    d = x.data if rt else x
    if rt and x.bits == 128:  # (lo, hi) words: one signed key per element, ordered by rank
        key = _rank128(d)
    else:
        key = d
    nd = key.dim() - nb
    ax = (axis + nd if axis < 0 else axis) + nb
    if by >= 0:
        order = torch.argsort(key.select(nb + 1, by), dim=nb, descending=bool(descending))
        idx = order.reshape(order.shape + (1,) * (d.dim() - order.dim()))
        out = torch.take_along_dim(d, idx.expand(d.shape), dim=nb)
    elif rt and x.bits == 128:
        order = torch.argsort(key, dim=ax, descending=bool(descending))
        out = torch.take_along_dim(d, order.unsqueeze(-1).expand(d.shape), dim=ax)
    else:
        out = torch.sort(d, dim=ax, descending=bool(descending)).values
    return R.RT(out.contiguous(), x.bits) if rt else out


def _rank128(d):
    """The rank of every signed 128-bit element ([..., 2] int64 words, low word first) among
    all of them, as an int64 tensor of the elements' shape: equal elements share a rank."""
    flat = d.reshape(-1, 2)
    lo = flat[:, 0] ^ torch.iinfo(torch.int64).min  # the low word compares unsigned
    o1 = torch.argsort(lo, stable=True)
    o2 = torch.argsort(flat[o1, 1], stable=True)
    order = o1[o2]
    s = flat[order]
    new = torch.ones(len(s), dtype=torch.int64, device=d.device)
    if len(s) > 1:
        new[1:] = ((s[1:] != s[:-1]).any(dim=1)).to(torch.int64)
    rank = torch.empty(len(s), dtype=torch.int64, device=d.device)
    rank[order] = torch.cumsum(new, 0)
    return rank.reshape(d.shape[:-1])


@prim("PwpPlain")
def _pwp_plain(nb, s, *powers, dt, ck):
    """The plain piecewise-polynomial leaf on ring tensors (R.pwp): sum_i (ck[i-1] + sum_j
    dt[i][j] * s[j]) * powers[i-1] + sum_j dt[0][j] * s[j] over the flag planes s stacked on the
    leading logical axis."""
    return R.pwp(s, list(powers), tuple(tuple(r) for r in dt), tuple(int(c) for c in ck), nb)


@prim("StridedSlice")
def _strided_slice(nb, a, slices):
    if _is_rt(a):
        return R.strided_slice(a, slices, nb)
    idx = [builtins_slice(None)] * nb + list(slices)
    return a[tuple(idx)].contiguous()


@prim("Select")
def _select(nb, a, mask, axis):
    # session primitive order (x, index); the IR op is (index, x) (graph_executor swaps)
    m = mask.data if _is_rt(mask) else mask
    if _is_rt(a):
        return R.select_mask(a, axis, m, nb)
    keep = torch.nonzero(m.reshape(-1).to(torch.bool)).reshape(-1).to(a.device)
    return a.index_select(_lax(a.dim(), axis, nb), keep).contiguous()


@prim("Diag")
def _diag(nb, a):
    if _is_rt(a):
        return R.diag(a, nb)
    return torch.diagonal(a, dim1=nb, dim2=nb + 1).contiguous()


@prim("Broadcast")
def _broadcast(nb, a, shape=None):
    if _is_rt(a):
        return R.broadcast_to(a, shape, nb)
    lead = len(shape) - (a.dim() - nb)
    if lead > 0:
        a = a.reshape(tuple(a.shape[:nb]) + (1,) * lead + tuple(a.shape[nb:]))
    return a.expand(tuple(a.shape[:nb]) + tuple(shape)).contiguous()


@prim("BroadcastLike")
def _broadcast_like(nb, a, like):
    """Broadcast ``a`` to the (run-time) shape of ``like`` -- the shape-polymorphic form of
    Broadcast, for lowered graphs whose shapes are only known when they run."""
    return _broadcast(nb, a, tuple(like.shape[nb:]))


@prim("AtLeast2D")
def _atleast_2d(nb, a, to_column_vector=False):
    if _is_rt(a):
        return R.atleast_2d(a, to_column_vector, nb)
    nd = a.dim() - nb
    if nd >= 2:
        return a
    if nd == 0:
        return a.reshape(tuple(a.shape[:nb]) + (1, 1))
    n = a.shape[nb]
    return a.reshape(tuple(a.shape[:nb]) + ((n, 1) if to_column_vector else (1, n)))


# ---------------------------------------------------------------------------
# constants / randomness
# ---------------------------------------------------------------------------
@prim("Fill")
def _fill(nb, shape, value, bits, device="cpu"):
    return R.fill(shape, value, bits, device)


@prim("AddConst")
def _add_const(nb, x, value, bits):
    """x + value (mod 2^bits); lowers to Fill + Add."""
    return R.binary("add", x, R.fill((), int(value), bits, x.device))


@prim("SampleSeeded")
def _sample_seeded(nb, shape, seed, bits, device="cpu"):
    """Uniform ring tensor expanded from a 16-byte seed: the PRF stream (ChaCha12,
    csrc/prf_core.h) keyed by the seed, nonce 0 (reference ``host/ops.rs:1883-2036`` +
    ``host/prim.rs:123-150``)."""
    if hasattr(seed, "table"):  # a KeyRef: the seed lives in a device key slot
        out = R.prf_expand_k(seed.ptr, 1, 0, tuple(shape), bits, device)
        return R.RT(out.data[0], bits)
    out = R.prf_expand([bytes(seed)[:16]], 0, tuple(shape), bits, device)
    return R.RT(out.data[0], bits)


@prim("DeriveSeed")
def _derive_seed(nb, key, sync_key):
    """16-byte seed = PRF(key) at the 128-bit input given by the sync key (reference
    ``host/prim.rs`` DeriveSeed: a keyed derivation of the sync key; parity of the bytes
    unpinned -- the reference hashes with its own KDF).  Sync keys longer than 16 bytes are
    compressed with BLAKE2b first."""
    import ctypes
    import hashlib

    sk = bytes(sync_key)
    sk = hashlib.blake2b(sk, digest_size=16).digest() if len(sk) > 16 else sk.ljust(16, b"\0")
    out = ctypes.create_string_buffer(16)
    from moose_amd.ops import native as nat

    nat.check(nat.lib().mx_derive_seed(bytes(key)[:16], sk, out), "derive_seed")
    return out.raw


@prim("PrfKeyGen")
def _prf_key_gen(nb):
    import os

    return os.urandom(16)


@prim("Sample")
def _sample(nb, shape, bits, device="cpu"):
    import os

    return _sample_seeded(nb, shape, os.urandom(16), bits, device)


@prim("Zeros")
def _zeros(nb, shape, dtype=torch.float64, device="cpu"):
    return torch.zeros(tuple(shape), dtype=dtype, device=device)


@prim("Ones")
def _ones(nb, shape, dtype=torch.float64, device="cpu"):
    return torch.ones(tuple(shape), dtype=dtype, device=device)


# ---------------------------------------------------------------------------
# ring <-> plaintext
# ---------------------------------------------------------------------------
@prim("RingFixedpointEncode")
def _encode(nb, x, scaling_exp, bits):
    # deferred: an input sharing of the result encodes inside the share kernel
    return R.encode_lazy(x, scaling_exp, bits)


@prim("RingFixedpointDecode")
def _decode(nb, x, scaling_exp, dtype=None):
    out = R.decode(x, scaling_exp)
    return out if dtype is None or out.dtype == dtype else out.to(dtype)


@prim("BitExtract")
def _bit_extract(nb, x, bit_idx):
    return R.bit_extract(x, bit_idx)


@prim("RingInject")
def _ring_inject(nb, x, bit_idx, bits):
    return R.ring_inject(x, bit_idx, bits)


@prim("RingCast")
def _ring_cast(nb, x, bits):
    return R.cast(x, bits)


@prim("BitSplit")
def _bit_split(nb, x, start, count):
    """Packed word -> bit tensor with a new logical leading axis: out[j] = bit start+j."""
    return R.bit_planes(x, start, count, nb)


@prim("WeightedSum")
def _weighted_sum(nb, x, weights, bits):
    """sum_j weights[j] * x[j] over the leading logical axis (public integer weights)."""
    return R.weighted_sum(x, weights, nb)


@prim("BitDecompose")
def _bit_decompose(nb, x, to_bits=True):
    """Ring tensor -> its bits stacked on a new leading logical axis (LSB first), as a
    bit tensor or as 0/1 ring elements (reference host/ops.rs:855-937)."""
    out = R.bit_planes(x, 0, x.bits, nb)
    if to_bits:
        return out
    return R.ring_inject(out, 0, x.bits)


@prim("ShlDim")
def _shl_dim(nb, x, amount, bit_length):
    """Shift along the leading (bit) axis: out[i] = x[i - amount], zeros below
    (reference host/ops.rs:835-853)."""
    d = x.data if _is_rt(x) else x
    ax = nb
    head = torch.zeros_like(d.narrow(ax, 0, amount))
    out = torch.cat([head, d.narrow(ax, 0, bit_length - amount)], dim=ax)
    return R.RT(out, x.bits) if _is_rt(x) else out


@prim("BitAffine")
def _bit_affine(nb, x, aff):
    """Linear part of a GF(2) affine map over the leading logical axis of a bit tensor
    (``aff`` is a ``bristol._SparseAffine``; one sparse GEMM, see protocols/bristol)."""
    d = x.data
    if nb:
        d = d.movedim(0, 1)  # party axis behind the wire axis
    y = aff.linear(d)
    if nb:
        y = y.movedim(1, 0)
    return R.RT(y.contiguous(), 1)


@prim("ToBool")
def _to_bool(nb, x):
    return x.data.to(torch.bool) if _is_rt(x) else x.to(torch.bool)


@prim("FromBool")
def _from_bool(nb, x):
    if _is_rt(x):  # already a bit tensor (e.g. a host comparison result)
        return R.RT(x.data.to(torch.uint8), 1)
    return R.RT(x.to(torch.uint8), 1)


@prim("RingToInt")
def _ring_to_int(nb, x):
    return R.cast(x, 64).data


@prim("IntToRing")
def _int_to_ring(nb, x):
    return R.RT(x.to(torch.int64), 64)


@prim("Less")
def _less(nb, a, b):
    if _is_rt(a):
        return R.compare("lt", a, b)
    return a < b


@prim("Greater")
def _greater(nb, a, b):
    if _is_rt(a):
        return R.compare("gt", a, b)
    return a > b


@prim("Equal")
def _equal(nb, a, b):
    if _is_rt(a):
        return R.compare("eq", a, b)
    return a == b


@prim("Msb")
def _msb(nb, a):
    return R.compare("msb", a)


@prim("Mux")
def _mux(nb, s, x, y):
    if _is_rt(s) and not _is_rt(x):  # a bit selector over plaintext operands
        s = s.data
    if _is_rt(x):
        sel = s if _is_rt(s) else R.RT(s.to(torch.uint8), 1)
        m = R.ring_inject(sel, 0, x.bits) if sel.bits == 1 else sel
        return R.binary("add", R.binary("mul", m, R.binary("sub", x, y)), y)
    return torch.where(s.to(torch.bool), x, y)


# ---------------------------------------------------------------------------
# plaintext float math (host placements)
# ---------------------------------------------------------------------------
def _f(fn):
    def impl(nb, a, **kw):
        return fn(a, **kw)

    return impl


prim("Exp")(_f(torch.exp))
prim("Log")(_f(torch.log))
prim("Log2")(_f(torch.log2))
prim("Sqrt")(_f(torch.sqrt))
prim("Sigmoid")(_f(torch.sigmoid))
prim("Relu")(_f(torch.relu))
prim("Abs")(_f(torch.abs))
@prim("Sign")
def _sign(nb, a):
    """Plaintext: torch.sign.  Ring: -1 for negative (two's complement) entries, +1
    otherwise -- zero included (reference host/ops.rs:1420-1452)."""
    if not _is_rt(a):
        return torch.sign(a)
    d = a.data if a.bits == 64 else a.data[..., 1]
    neg = d < 0
    if a.bits == 64:
        return R.RT(torch.where(neg, -1, 1).to(torch.int64), 64)
    lo = torch.where(neg, -1, 1).to(torch.int64)
    hi = torch.where(neg, -1, 0).to(torch.int64)
    return R.RT(torch.stack([lo, hi], dim=-1), 128)
def _inverse(a):
    """torch.linalg.inv without its error check on device tensors: the check reads the
    solver's info flag back to the host, which a hipGraph capture cannot do (a singular
    input gives inf/nan entries instead of an exception, like numpy's LinAlgError-free
    paths; on the host the checked form runs)."""
    if a.is_cuda:
        return torch.linalg.inv_ex(a)[0]
    return torch.linalg.inv(a)


prim("Inverse")(_f(_inverse))


@prim("Softmax")
def _softmax(nb, a, axis, upmost_index):
    ax = _lax(a.dim(), axis, nb)
    return torch.softmax(a, dim=ax)


@prim("Argmax", ty=lambda tys, **a: T.Ty("HostUint64Tensor"))
def _argmax(nb, a, axis, upmost_index):
    ax = _lax(a.dim(), axis, nb)
    return torch.argmax(a, dim=ax)


@prim("Maximum")
def _maximum(nb, *xs):
    if _is_rt(xs[0]):
        return _ring_maximum(xs)
    acc = xs[0]
    for x in xs[1:]:
        acc = torch.maximum(acc, x)
    return acc


def _ring_maximum(xs):
    """Elementwise maximum of ring tensors compared as UNSIGNED integers -- the reference's
    ring Maximum compares ``Wrapping<u64>`` / ``Wrapping<u128>`` (host/ops.rs:2475-2497)."""
    bits = xs[0].bits
    acc = xs[0].data
    for x in xs[1:]:
        d = x.data
        if bits == 128:
            ah, bh = acc[..., 1] ^ _SIGN64, d[..., 1] ^ _SIGN64
            al, bl = acc[..., 0] ^ _SIGN64, d[..., 0] ^ _SIGN64
            gt = (bh > ah) | ((bh == ah) & (bl > al))
            acc = torch.where(gt.unsqueeze(-1), d, acc)
        elif bits == 64:
            acc = torch.where((d ^ _SIGN64) > (acc ^ _SIGN64), d, acc)
        else:
            acc = torch.maximum(acc, d)
    return R.RT(acc.contiguous(), bits)


@prim("Cast")
def _cast(nb, x, dtype=torch.float64, ty=None):
    """Host casts (reference kernels/conversion.rs:26-48).  ``ty`` is the result type name
    when known (a lowered graph): rings and bits need it."""
    if ty == "HostBitTensor":  # x != 0 (host/ops.rs:2334-2371)
        d = x.data if _is_rt(x) else x
        return R.RT((d != 0).to(torch.uint8), 1)
    if ty in ("HostRing64Tensor", "HostRing128Tensor"):
        bits = 64 if ty == "HostRing64Tensor" else 128
        return x if x.bits == bits else R.cast(x, bits)
    if _is_rt(x):  # bit -> float / u64 (0 / 1); Z_2^64 -> u64 (the same 64 bits)
        return x.data.to(dtype)
    return x.to(dtype)


@prim("Identity")
def _identity(nb, x):
    return x


def numel_of(shape):
    return math.prod(shape)
