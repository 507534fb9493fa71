"""R.perm_gather and R.perm_from_keys: the CPU twin against a Python-integer model mod 2^64 and
2^128, the device kernel bitwise against the twin and the torch composition, over every
combination of the optional operands, slot views of a stacked buffer, and the argument checks;
the permutation against numpy's stable argsort on uint64, and its uniformity for n = 4."""
import itertools

import numpy as np
import pytest
import torch

from moose_amd.ops import ring as R

DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
# (outer, n, inner): a single element, a pair, an odd outer and n, an odd inner (no 16-byte
# path for u64), several rows of an odd width, an axis that crosses a 256-thread block, more
# slices than a block has row lanes, and a longer axis of even width
SHAPES = [(1, 1, 1), (1, 2, 1), (3, 5, 1), (1, 8, 3), (2, 16, 5), (1, 260, 1), (65, 8, 2),
          (1, 1024, 4)]
FORMS = list(itertools.product((False, True), repeat=3))  # b, plus, minus present or absent
_REF = {}


def _perms(n, rng):
    return {"identity": np.arange(n), "reversal": np.arange(n)[::-1].copy(),
            "random": rng.permutation(n)}


def _operands(shape, bits):
    """Four operands of Python integers with 0 and 2^bits - 1 among them."""
    key = (shape, bits)
    if key not in _REF:
        rng = np.random.default_rng(sum(shape) + bits)
        top = (1 << bits) - 1
        ops = []
        for _ in range(4):
            words = rng.integers(0, 1 << 62, size=(int(np.prod(shape)), 3))
            v = [(int(w[0]) | (int(w[1]) << 62) | (int(w[2]) << 124)) & top for w in words]
            v[0], v[-1] = top, 0
            if len(v) > 2:
                v[1] = 0
            ops.append(np.array(v, dtype=object).reshape(shape))
        _REF[key] = (ops, _perms(shape[1], rng))
    return _REF[key]


def _model(a, perm, b, plus, minus, bits):
    """out[o, r, c] = a[o, perm[r], c] + b[o, perm[r], c] + plus[o, r, c] - minus[o, r, c]."""
    out = a[:, perm, :]
    if b is not None:
        out = out + b[:, perm, :]
    if plus is not None:
        out = out + plus
    if minus is not None:
        out = out - minus
    return out % (1 << bits)


_RTS = {}


def _run(fn, ints, perm, form, bits, device, **kw):
    key = (id(ints), bits, device)  # the operands are converted once and never written
    if key not in _RTS:
        _RTS[key] = (ints, [R.from_ints(v, bits, device) for v in ints])
    a, b, p, m = (t if use else None for t, use in zip(_RTS[key][1], (True,) + form))
    return fn(a, torch.as_tensor(perm.copy()).to(device), b=b, plus=p, minus=m, axis=1, **kw)


@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_twin_equals_the_integer_model(shape, bits):
    ints, perms = _operands(shape, bits)
    for name, perm in perms.items():
        for form in FORMS:
            want = _model(ints[0], perm, *[v if use else None for v, use in zip(ints[1:], form)],
                          bits)
            got = R.to_ints(_run(R.perm_gather, ints, perm, form, bits, "cpu"))
            assert (got == want).all(), (name, form)
            comp = R.to_ints(_run(R.perm_gather_torch, ints, perm, form, bits, "cpu"))
            assert (comp == want).all(), (name, form)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_device_kernel_equals_twin_and_composition_bitwise(shape, bits, monkeypatch):
    monkeypatch.setattr(R, "SHUFFLE_KERNEL", True)
    ints, perms = _operands(shape, bits)
    for name, perm in perms.items():
        for form in FORMS:
            twin = _run(R.perm_gather, ints, perm, form, bits, "cpu")
            got = _run(R.perm_gather, ints, perm, form, bits, "cuda:0")
            comp = _run(R.perm_gather_torch, ints, perm, form, bits, "cuda:0")
            assert got.device.type == "cuda" and tuple(got.shape) == shape
            assert torch.equal(got.data.cpu(), twin.data), (name, form)
            assert torch.equal(comp.data.cpu(), twin.data), (name, form)


@pytest.mark.gpu
def test_the_kernel_switch_selects_the_composition(monkeypatch):
    ints, perms = _operands((2, 16, 5), 128)
    calls = []
    real = R.perm_gather_torch
    monkeypatch.setattr(R, "perm_gather_torch", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(R, "SHUFFLE_KERNEL", False)
    off = _run(R.perm_gather, ints, perms["random"], (True, False, True), 128, "cuda:0")
    assert calls == [1]
    monkeypatch.setattr(R, "SHUFFLE_KERNEL", True)
    on = _run(R.perm_gather, ints, perms["random"], (True, False, True), 128, "cuda:0")
    assert calls == [1] and torch.equal(on.data, off.data)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("shape", [(1, 8, 3), (2, 16, 5), (1, 260, 1), (3, 6, 2)])
def test_slot_views_of_a_stacked_buffer_are_read_in_place(shape, bits, device):
    """The operands as non-contiguous slot views: s0 = buf[0:3] and s1 = buf[1:4] of a
    four-slot ring, and every second slot of a six-slot buffer; one launch over the slots."""
    rng = np.random.default_rng(bits + shape[1])
    top = (1 << bits) - 1
    slots = rng.integers(0, 1 << 62, size=(6,) + shape).astype(object) * 0x3FFFFFFFFFFFFFFF3 & top
    slots[0].flat[0], slots[3].flat[-1] = top, 0
    buf = R.from_ints(slots, bits, device)
    perm = rng.permutation(shape[1])
    pt = torch.as_tensor(perm).to(device)

    def view(sl):
        return R.RT(buf.data[sl], bits)

    a, b, p, m = view(slice(0, 3)), view(slice(1, 4)), view(slice(2, 5)), view(slice(0, 6, 2))
    assert not m.data.is_contiguous()
    got = R.to_ints(R.perm_gather(a, pt, b=b, plus=p, minus=m, axis=1, nb=1))
    for s in range(3):
        want = _model(slots[s], perm, slots[1 + s], slots[2 + s], slots[2 * s], bits)
        assert (got[s] == want).all(), s
    plain = R.to_ints(R.perm_gather(m, pt, axis=1, nb=1))
    for s in range(3):
        assert (plain[s] == slots[2 * s][:, perm, :]).all(), s


def test_a_wrong_perm_is_rejected():
    a = R.from_ints(np.arange(12, dtype=object).reshape(4, 3), 64)
    with pytest.raises(ValueError, match="int64"):
        R.perm_gather(a, torch.arange(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        R.perm_gather(a, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="axis length 4"):
        R.perm_gather(a, torch.arange(3))
    with pytest.raises(ValueError, match="axis length 3"):
        R.perm_gather(a, torch.arange(4), axis=-1)
    with pytest.raises(ValueError, match="lives on meta"):
        R.perm_gather(a, torch.arange(4, device="meta"))
    with pytest.raises(ValueError, match="axis 2 out of range"):
        R.perm_gather(a, torch.arange(4), axis=2)
    with pytest.raises(ValueError, match="`minus` must be a Z_2\\^64 tensor of shape"):
        R.perm_gather(a, torch.arange(4), minus=R.from_ints(np.zeros((4, 2), dtype=object), 64))
    with pytest.raises(ValueError, match="arithmetic only"):
        R.perm_gather(R.from_ints(np.zeros(4, dtype=object), 1), torch.arange(4))
    with pytest.raises(Exception, match="perm_gather"):  # the CPU twin checks the values
        R.perm_gather(a, torch.tensor([0, 1, 1, 3]))


def test_the_entry_point_refuses_sizes_whose_extents_overflow():
    """mx_perm_gather bounds slots * elements and slots * stride before either side forms an
    extent: -3, nothing read."""
    from moose_amd.ops import native as nat

    a = R.from_ints(np.arange(4, dtype=object), 64)
    perm = torch.arange(4)
    out = R.empty((4,), 64, "cpu")

    def call(slots, stride, outer, n, inner):
        return nat.lib().mx_perm_gather(0, 8, nat.ptr(a.data), None, None, None, nat.ptr(perm),
                                        nat.ptr(out.data), slots, stride, 0, 0, 0, outer, n,
                                        inner, None)

    assert call(1, 4, 1, 4, 1) == 0
    assert (R.to_ints(out) == np.arange(4)).all()
    assert call(1 << 40, 0, 1 << 20, 4, 1) == -3  # slots * n_x
    assert call(1 << 31, 1 << 40, 1, 4, 1) == -3  # slots * stride
    assert call(2, 1 << 62, 1, 4, 1) == -3
    assert call(1, 4, 1 << 30, 1 << 30, 4) == -3  # outer * n * inner
    assert call(1, -1, 1, 4, 1) == -3
    assert call(1, 4, 1, 4, 1) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("shape", [(1, 8, 3), (2, 16, 4), (1, 260, 1)])
def test_the_kernel_clamps_a_bad_perm_to_the_axis(shape, bits, monkeypatch):
    """Nothing reads a device ``perm`` back: the kernel clamps every entry to [0, n) -- a
    negative one, read as unsigned, and one past the end both name the last row -- so a perm
    that is no permutation gathers wrong rows and never reads outside the tensor.  (The torch
    composition has no such clamp and is not called here.)"""
    monkeypatch.setattr(R, "SHUFFLE_KERNEL", True)
    n = shape[1]
    ints, _ = _operands(shape, bits)
    rng = np.random.default_rng(n + bits)
    bad = rng.integers(0, n, size=n)  # duplicates
    bad[0], bad[1], bad[2], bad[-1] = -1, n, 2 ** 40, -(2 ** 62)
    bad[3] = n - 1
    clamped = np.where((bad >= 0) & (bad < n), bad, n - 1)
    for form in ((False, False, False), (True, False, True), (False, True, True)):
        got = R.to_ints(_run(R.perm_gather, ints, bad, form, bits, "cuda:0"))
        want = _model(ints[0], clamped, *[v if use else None for v, use in zip(ints[1:], form)],
                      bits)
        assert (got == want).all(), form


@pytest.mark.gpu
def test_a_perm_on_another_device_is_rejected():
    a = R.from_ints(np.arange(4, dtype=object), 64, "cuda:0")
    with pytest.raises(ValueError, match="lives on cpu"):
        R.perm_gather(a, torch.arange(4))


@pytest.mark.parametrize("device", DEVICES)
def test_perm_from_keys_is_the_stable_unsigned_argsort(device):
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 1 << 64, size=300, dtype=np.uint64)
    keys[:4] = [0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]  # both sides of 2^63
    keys[10:40] = keys[100:130]  # duplicates
    keys[50:60] = keys[0]
    keys[60:70] = 1 << 63
    want = np.argsort(keys, kind="stable")
    rt = R.from_ints(keys.astype(object), 64, device)
    got = R.perm_from_keys(rt)
    assert got.dtype == torch.int64 and got.device == rt.device
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="Z_2\\^64 vector"):
        R.perm_from_keys(R.from_ints(keys[:4].astype(object), 128, device))


SEED = 2024  # the draws are seeded: deterministic


def test_permutations_of_four_are_uniform():
    """2400 permutations of n = 4 from 2400 seeded PRF draws: chi-square over the 24 orders
    below 49.7, the 99.9 % point at 23 degrees of freedom."""
    from moose_amd.ir.computation import ReplicatedPlacement
    from moose_amd.runtime.session import HV
    from moose_amd.runtime.session import StackedSession

    plc = ReplicatedPlacement(("a", "b", "c"))
    sess = StackedSession("cpu", seed=SEED)
    sess.setup(plc)
    counts = {}
    for _ in range(2400):
        keys = sess.h_prf(plc, "a", 0, HV("a", (4,)), 64, sess.nonce(plc))
        order = tuple(R.perm_from_keys(keys.v).tolist())
        counts[order] = counts.get(order, 0) + 1
    assert all(sorted(o) == [0, 1, 2, 3] for o in counts)
    chi2 = sum((counts.get(o, 0) - 100) ** 2 / 100 for o in itertools.permutations(range(4)))
    print(f"chi-square {chi2:.2f} over {len(counts)} orders")
    assert chi2 < 49.7
