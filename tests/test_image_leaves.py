"""The plumbing the image leaves share (im2col, col2im, resize2d, dwconv, pwl_cross): the
return codes of the native entry points on the host path, pinned as constants, and the
operand helpers of ``moose_amd.ops.ring`` that decide between reading a slot view in place
and taking a dense copy."""
import pytest
import torch

from moose_amd.ops import native as nat
from moose_amd.ops import ring as R

BIG = 1 << 31

# a valid small problem: N C H W = 1 2 3 3, a 2x2 window, unit strides and dilations, no pads
_GEOM = dict(N=1, C=2, H=3, W=3, KH=2, KW=2, sh=1, sw=1, pt=0, pl=0, dh=1, dw=1, OH=2, OW=2)
_WINDOW = ("N", "C", "H", "W", "KH", "KW", "sh", "sw", "pt", "pl", "dh", "dw", "OH", "OW")


_BUFS = [torch.zeros(512, dtype=torch.int64) for _ in range(5)]
_TAB = torch.zeros((3, 6), dtype=torch.int32)  # resize: tap 0 with weight 0 everywhere
_PWL = torch.zeros(32, dtype=torch.int64)


def _p(i, given=True):
    return nat.ptr(_BUFS[i]) if given else None


def _im2col(fn, eb=8, slots=1, stride=18, **kw):
    g = dict(_GEOM, **kw)
    return getattr(nat.lib(), fn)(0, eb, _p(0), _p(1), slots, stride,
                                  *(g[k] for k in _WINDOW), 0, None)


def _resize(eb=8, slots=1, stride=18, th=True, tw=True, wb=0, **kw):
    g = dict(N=1, C=2, H=3, W=3, OH=6, OW=6)
    g.update(kw)
    tab = _TAB
    return nat.lib().mx_resize2d(0, eb, _p(0), _p(1), slots, stride,
                                 *(g[k] for k in ("N", "C", "H", "W", "OH", "OW")),
                                 nat.ptr(tab) if th else None, nat.ptr(tab) if tw else None, wb,
                                 wb, 0, None)


def _dwconv(eb=8, slots=1, x1=False, w1=False, xst=18, wst=8, mult=1, **kw):
    g = dict(_GEOM, **kw)
    v = [g[k] for k in _WINDOW]
    return nat.lib().mx_dwconv(0, eb, _p(0), _p(1, x1), _p(2), _p(3, w1), _p(4),
                               slots, xst, wst, *v[:4], mult, *v[4:], 0, None)


def _pwl(eb=8, slots=1, s1=False, x1=False, sst=16, xst=8, n=8, k=2, da=True, ak=True):
    tab = _PWL
    return nat.lib().mx_pwl_cross(0, eb, _p(0), _p(1, s1), _p(2), _p(3, x1), _p(4), slots, sst,
                                  xst, n, k,
                                  nat.ptr(tab) if da else None, nat.ptr(tab), nat.ptr(tab) if ak
                                  else None, None)


def _i2c(**kw):
    return _im2col("mx_im2col", **kw)


def _c2i(**kw):
    return _im2col("mx_col2im", **kw)


# (entry point, arguments changed from the valid problem, the code it returns).  The codes
# were recorded from the entry points before their checks moved into csrc/img_geom.h; the one
# that changed on purpose is im2col's negative slot stride (0 before: the host half did not
# look at it, its device half and every other leaf rejected it).
CODES = [
    (_i2c, {}, 0),
    (_i2c, dict(eb=1), 0),
    (_i2c, dict(eb=16), 0),
    (_i2c, dict(slots=0), 0),
    (_i2c, dict(N=0), 0),
    (_i2c, dict(C=0), 0),
    (_i2c, dict(N=-1), -3),
    (_i2c, dict(slots=-1), -3),
    (_i2c, dict(KH=0), -3),
    (_i2c, dict(pt=-1), -3),
    (_i2c, dict(N=BIG), -3),
    (_i2c, dict(H=BIG), -3),
    (_i2c, dict(OH=BIG - 1, sh=2), -3),
    (_i2c, dict(eb=4), -2),
    (_i2c, dict(eb=4, slots=0), 0),
    (_i2c, dict(eb=4, N=BIG), -3),
    (_i2c, dict(stride=-1), -3),
    (_c2i, {}, 0),
    (_c2i, dict(eb=16), 0),
    (_c2i, dict(slots=0), 0),
    (_c2i, dict(N=0), 0),
    (_c2i, dict(H=0), 0),
    (_c2i, dict(N=-1), -3),
    (_c2i, dict(sw=0), -3),
    (_c2i, dict(stride=-1), -3),
    (_c2i, dict(N=BIG), -3),
    (_c2i, dict(W=BIG), -3),
    (_c2i, dict(H=BIG - 1, pt=1), -3),
    (_c2i, dict(eb=1), -2),
    (_c2i, dict(eb=4), -2),
    (_c2i, dict(eb=4, slots=0), -2),
    (_c2i, dict(eb=4, N=BIG), -2),
    (_c2i, dict(eb=4, N=-1), -3),
    (_resize, {}, 0),
    (_resize, dict(eb=16), 0),
    (_resize, dict(slots=0), 0),
    (_resize, dict(C=0), 0),
    (_resize, dict(slots=0, th=False), 0),
    (_resize, dict(N=-1), -3),
    (_resize, dict(H=0), -3),
    (_resize, dict(OW=0), -3),
    (_resize, dict(stride=-1), -3),
    (_resize, dict(OH=BIG), -3),
    (_resize, dict(wb=13), -3),
    (_resize, dict(th=False), -3),
    (_resize, dict(tw=False), -3),
    (_resize, dict(eb=1), -2),
    (_resize, dict(eb=4, slots=0), -2),
    (_resize, dict(eb=4, OH=BIG), -2),
    (_resize, dict(eb=4, th=False), -2),
    (_dwconv, {}, 0),
    (_dwconv, dict(eb=16), 0),
    (_dwconv, dict(x1=True, w1=True), 0),
    (_dwconv, dict(slots=0), 0),
    (_dwconv, dict(N=0), 0),
    (_dwconv, dict(N=-1), -3),
    (_dwconv, dict(mult=0), -3),
    (_dwconv, dict(xst=-1), -3),
    (_dwconv, dict(wst=-1), -3),
    (_dwconv, dict(N=BIG), -3),
    (_dwconv, dict(mult=BIG), -3),
    (_dwconv, dict(C=1 << 16, mult=1 << 16), -3),
    (_dwconv, dict(OW=BIG - 1, sw=2), -3),
    (_dwconv, dict(x1=True), -3),
    (_dwconv, dict(w1=True), -3),
    (_dwconv, dict(eb=1), -2),
    (_dwconv, dict(eb=4), -2),
    (_dwconv, dict(eb=4, slots=0), 0),
    (_dwconv, dict(eb=4, N=BIG), -3),
    (_pwl, {}, 0),
    (_pwl, dict(eb=16, n=4), 0),
    (_pwl, dict(s1=True, x1=True), 0),
    (_pwl, dict(k=0, da=False), 0),
    (_pwl, dict(slots=0), 0),
    (_pwl, dict(n=0), 0),
    (_pwl, dict(n=0, ak=False), 0),
    (_pwl, dict(n=-1), -3),
    (_pwl, dict(k=9), -3),
    (_pwl, dict(k=-1), -3),
    (_pwl, dict(sst=-1), -3),
    (_pwl, dict(s1=True), -3),
    (_pwl, dict(x1=True), -3),
    (_pwl, dict(da=False), -3),
    (_pwl, dict(ak=False), -3),
    (_pwl, dict(eb=1), -2),
    (_pwl, dict(eb=4, slots=0), -2),
    (_pwl, dict(eb=4, k=9), -3),
]

# A slot stride above 2^61 / slots: (slots - 1) * stride would wrap int64_t (3 * 2^61 and
# 2 * (2^62 + 1) both do) and come out looking like a small or a negative extent.  Refused
# before any extent is formed and before anything is read.
_FAR = (dict(slots=4, stride=1 << 61), dict(slots=3, stride=(1 << 62) + 1))
for _call, _names in ((_i2c, ("stride",)), (_c2i, ("stride",)), (_resize, ("stride",)),
                      (_dwconv, ("xst", "wst")), (_pwl, ("sst", "xst"))):
    for _name in _names:
        CODES += [(_call, {"slots": f["slots"], _name: f["stride"]}, -3) for f in _FAR]
# a slot's element count above 2^61 / slots: N * C * H * W = 2^60 with four slots
CODES += [(_i2c, dict(slots=4, N=1 << 30, C=1 << 30), -3),
          (_pwl, dict(slots=4, n=1 << 59), -3),
          (_pwl, dict(slots=1, n=1 << 59, k=8), -3)]


def _rt(words, bits):
    """A ring tensor over ``words`` ([.., 2] int64 for 128 bits)."""
    return R.RT(words, bits)


@pytest.mark.parametrize("bits", [64, 128])
def test_leaf_operand_reads_dense_slot_views_in_place(bits):
    w = bits // 64
    tail = (2,) if w == 2 else ()
    base = torch.arange(4 * 5 * 6 * w, dtype=torch.int64).reshape((4, 5, 6) + tail)
    dense = 30
    # no batch dims: the dense stride, whatever the operand
    d, st = R._leaf_operand(_rt(base[0], bits), 0, dense)
    assert st == dense and d.is_contiguous()
    # three slots of a four-slot buffer, step 1: the same storage, its stride in elements
    for view in (base[:3], base[1:]):
        d, st = R._leaf_operand(_rt(view, bits), 1, dense)
        assert st == 30 and d.data_ptr() == view.data_ptr() and d.stride() == view.stride()
    # dense slots two apart: still in place
    d, st = R._leaf_operand(_rt(base[::2], bits), 1, dense)
    assert st == 60 and d.data_ptr() == base.data_ptr()
    # anything else comes back contiguous at the dense stride, with the view's values
    # (torch has no negative strides, so the helper's guard against one cannot be reached here)
    views = [base[:, :, :3], base.transpose(1, 2)]
    if w == 2:
        # an int64 view whose slot stride is an odd number of words: not a multiple of the
        # two words of an element
        words = torch.arange(3 * 13, dtype=torch.int64)
        views.append(words.as_strided((3, 3, 2), (13, 2, 1)))
    for view in views:
        n = view.numel() // view.shape[0] // w
        d, st = R._leaf_operand(_rt(view, bits), 1, n)
        assert st == n and d.is_contiguous() and torch.equal(d, view)
    # no slots at all, and more than one batch dim: dense
    d, st = R._leaf_operand(_rt(base[:0], bits), 1, dense)
    assert st == dense and d.is_contiguous()
    d, st = R._leaf_operand(_rt(base, bits), 2, 6)
    assert st == 6 and d.is_contiguous()


@pytest.mark.parametrize("bits", [64, 128])
def test_leaf_operand_public_rank4_and_shape_mismatch(bits):
    tail = (2,) if bits == 128 else ()
    pub = _rt(torch.zeros((1, 2, 3, 3) + tail, dtype=torch.int64), bits)
    d, st = R._leaf_operand(pub, 1, 18, (1, 2, 3, 3), (3,))
    assert st == 0 and d.is_contiguous()
    # without batch dims a rank-4 operand is the one image: dense
    assert R._leaf_operand(pub, 0, 18, (1, 2, 3, 3), ())[1] == 18
    batched = _rt(torch.zeros((3, 1, 2, 3, 3) + tail, dtype=torch.int64), bits)
    assert R._leaf_operand(batched, 1, 18, (1, 2, 3, 3), (3,))[1] == 18
    for rank4, lead in (((1, 2, 3, 4), (3,)), ((1, 2, 3, 3), (2,))):
        with pytest.raises(ValueError, match=r"dwconv: operand of shape \(3, 1, 2, 3, 3\) does "
                                             r"not match the batch dims"):
            R._leaf_operand(batched, 1, 18, rank4, lead)


@pytest.mark.parametrize("bits", [64, 128])
def test_leaf_pair_shares_one_stride(bits):
    w = bits // 64
    tail = (2,) if w == 2 else ()
    base = torch.arange(4 * 6 * w, dtype=torch.int64).reshape((4, 6) + tail)
    a, sa = R._leaf_operand(_rt(base[:3], bits), 1, 6)
    b, sb = R._leaf_operand(_rt(base[1:], bits), 1, 6)
    d0, d1, st = R._leaf_pair(a, sa, b, sb, 6)
    assert d0 is a and d1 is b and st == 6 and a.data_ptr() == base.data_ptr()
    c, sc = R._leaf_operand(_rt(base[::2], bits), 1, 6)
    assert sc == 12
    d0, d1, st = R._leaf_pair(c, sc, a[:2], sa, 6)
    assert st == 6 and d0.is_contiguous() and d1.is_contiguous()
    assert torch.equal(d0, base[::2]) and torch.equal(d1, base[:2])


def test_elem_bytes():
    assert [R._elem_bytes(b) for b in (1, 64, 128)] == [1, 8, 16]


@pytest.mark.parametrize("call, change, code", CODES,
                         ids=[f"{c.__name__[1:]}-{'-'.join(f'{k}={v}' for k, v in d.items()) or 'valid'}"
                              for c, d, _ in CODES])
def test_native_return_codes(call, change, code):
    assert call(**change) == code
