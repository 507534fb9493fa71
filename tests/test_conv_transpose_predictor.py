"""ConvNetwork with ConvTranspose: a small encoder / decoder built as ONNX bytes, imported
with from_onnx and run on the local runtime against the same network in float64 torch."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moose_amd.models import predictors
from moose_amd.models.predictors import conv
from moose_amd.models.predictors import onnx_proto as op
from moose_amd.runtime.local import LocalMooseRuntime

ROLES = ["alice", "bob", "carole"]
FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "fixtures", "onnx", "*.onnx")))
RNG = np.random.default_rng(21)
f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
W1, B1 = f32(RNG.uniform(-0.5, 0.5, (4, 2, 3, 3))), f32(RNG.uniform(-0.5, 0.5, 4))
WT1, BT1 = f32(RNG.uniform(-0.5, 0.5, (4, 3, 4, 4))), f32(RNG.uniform(-0.5, 0.5, 3))
WT2, BT2 = f32(RNG.uniform(-0.5, 0.5, (3, 2, 3, 3))), f32(RNG.uniform(-0.5, 0.5, 2))
# 4x4 -> Conv 4x4 -> ConvTranspose(4x4, s2, p1) 8x8 -> ConvTranspose(3x3, s2, op 1) 18x18
FLAT = 2 * 18 * 18
WD, BD = f32(RNG.uniform(-0.1, 0.1, (5, FLAT))), f32(RNG.uniform(-0.5, 0.5, 5))  # transB = 1
INITS = {"w1": W1, "b1": B1, "wt1": WT1, "bt1": BT1, "wt2": WT2, "bt2": BT2, "wd": WD, "bd": BD}
F_BITS = 40  # DEFAULT_FIXED_DTYPE = fixed(24, 40)


def _tensor(name, a):
    a = np.asarray(a, dtype=np.float32)
    return op.make("TensorProto", name=name, dims=list(a.shape), data_type=1,
                   raw_data=a.tobytes())


def _node(kind, ins, out, **attrs):
    return op.make("NodeProto", input=list(ins), output=[out], name=f"{kind}_{out}",
                   op_type=kind, attribute=[op.attr(k, v) for k, v in attrs.items()])


def _model(nodes, inits, chw=(2, 4, 4)):
    dims = [op.make("Dimension", dim_param="N")] + [op.make("Dimension", dim_value=d)
                                                    for d in chw]
    inp = op.make("ValueInfoProto", name="x", type=op.make(
        "TypeProto", tensor_type=op.make("TypeProtoTensor", elem_type=1,
                                         shape=op.make("TensorShapeProto", dim=dims))))
    out = op.make("ValueInfoProto", name="y", type=op.make(
        "TypeProto", tensor_type=op.make("TypeProtoTensor", elem_type=1)))
    graph = op.make("GraphProto", node=nodes, name="decoder", input=[inp], output=[out],
                    initializer=[_tensor(k, v) for k, v in inits.items()])
    return op.serialize(op.make("ModelProto", ir_version=8, producer_name="pytorch",
                                producer_version="2.0", graph=graph,
                                opset_import=[op.make("OperatorSetIdProto", domain="",
                                                      version=15)]))


def _net(t1=None, t1_inputs=("r1", "wt1", "bt1")):
    return [
        _node("Conv", ["x", "w1", "b1"], "c1", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
        _node("Relu", ["c1"], "r1"),
        _node("ConvTranspose", list(t1_inputs), "t1", **(t1 or dict(
            kernel_shape=[4, 4], strides=[2, 2], pads=[1, 1, 1, 1], output_padding=[0, 0]))),
        _node("Relu", ["t1"], "r2"),
        _node("ConvTranspose", ["r2", "wt2", "bt2"], "t2", kernel_shape=[3, 3], strides=[2, 2],
              output_padding=[1, 1]),
        _node("Flatten", ["t2"], "f", axis=1),
        _node("Gemm", ["f", "wd", "bd"], "y", transB=1),
    ]


def _torch_reference(x):
    """-> (prediction, the largest |activation| entering each of the four linear layers)."""
    t = torch.tensor
    a0 = t(x)
    a1 = F.relu(F.conv2d(a0, t(W1), t(B1), padding=1))
    a2 = F.relu(F.conv_transpose2d(a1, t(WT1), t(BT1), stride=2, padding=1))
    a3 = F.conv_transpose2d(a2, t(WT2), t(BT2), stride=2, output_padding=1)
    y = a3.flatten(1) @ t(WD).T + t(BD)
    return y.numpy(), [float(a.abs().max()) for a in (a0, a1, a2, a3)]


X = np.random.default_rng(22).uniform(-1, 1, (3, 2, 4, 4))
WANT, MAGS = _torch_reference(X)


def _tolerance():
    """The error bound that accumulates through the layers, in units of u = 2^-f.  A linear
    layer with e_in on its inputs of magnitude <= m, n weights per output of absolute sum <=
    a, and r units of its own rounding answers with e_out <= a * e_in + n * u * (m + e_in) +
    r * u: the first term carries the input error, the second the weights' encoding (each
    truncated by less than u), the third the truncation.  r is (K + 2) for a convolution or
    a dense layer over K terms (tests/test_conv2d.py) and T * (C + 1) + 1 for a transposed
    convolution whose pixels sum at most T patch-matrix entries of C products each
    (tests/test_conv_transpose.py).  ReLU is exact and 1-Lipschitz."""
    u = 2.0 ** -F_BITS
    e = u  # the input's encoding
    layers = [
        # (a, n, r): Conv 3x3 over 2 channels
        (np.abs(W1).sum(axis=(1, 2, 3)).max(), 18, 18 + 2),
        # ConvTranspose 4x4 stride 2: a pixel sums T = 2 * 2 taps over C = 4
        (np.abs(WT1).sum(axis=(0, 2, 3)).max(), 4 * 16, 4 * (4 + 1) + 1),
        # ConvTranspose 3x3 stride 2: T = 2 * 2 over C = 3
        (np.abs(WT2).sum(axis=(0, 2, 3)).max(), 3 * 9, 4 * (3 + 1) + 1),
        (np.abs(WD).sum(axis=1).max(), FLAT, FLAT + 2),
    ]
    for (a, n, r), m in zip(layers, MAGS):
        e = a * e + n * u * (m + e) + r * u
    return e


def test_from_onnx_reads_conv_transpose():
    net = predictors.from_onnx(_model(_net(), INITS))
    assert isinstance(net, conv.ConvNetwork) and net.n_outputs == 5
    assert [l["op"] for l in net.layers] == ["conv", "relu", "convtranspose", "relu",
                                             "convtranspose", "flatten", "dense"]
    t1, t2 = (l for l in net.layers if l["op"] == "convtranspose")
    assert t1["fmt"] == t2["fmt"] == "NHWC"
    assert t1["chw"] == (4, 4, 4) and t1["out_chw"] == (3, 8, 8)
    assert t2["chw"] == (3, 8, 8) and t2["out_chw"] == (2, 18, 18)
    assert t2["output_padding"] == (1, 1) and t2["pads"] == (0, 0, 0, 0)
    assert net._flat_size() == (2, 18, 18)
    # a decoder alone, reading the NCHW model input
    alone = predictors.from_onnx(_model(
        [_node("ConvTranspose", ["x", "wt2"], "t", kernel_shape=[3, 3], strides=[2, 2]),
         _node("Flatten", ["t"], "f", axis=1),
         _node("MatMul", ["f", "wm"], "y")],
        {"wt2": WT2, "wm": np.zeros((2 * 9 * 9, 2))}, chw=(3, 4, 4)))
    assert isinstance(alone, conv.ConvNetwork) and alone.layers[0]["fmt"] == "NCHW"
    assert alone.layers[0]["out_chw"] == (2, 9, 9)


def _check(device):
    net = predictors.from_onnx(_model(_net(), INITS))
    kw = {"use_graphs": True} if device != "cpu" else {}
    rt = LocalMooseRuntime(ROLES, device=device, **kw)
    comp = net.predictor_factory()
    tol = _tolerance()
    assert tol < 1e-6
    for _ in range(2):  # with hipGraphs the second evaluation is a replay
        got = rt.evaluate_computation(comp, {"x": X})["output_0"]
        assert got.shape == WANT.shape
        err = np.abs(got - WANT).max()
        print(f"conv-transpose predictor on {device}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol


def test_predictor_matches_torch_cpu():
    _check("cpu")


@pytest.mark.gpu
def test_predictor_matches_torch_gpu():
    _check("cuda:0")


def test_decoder_reading_the_model_input_matches_torch():
    """A ConvTranspose as the first layer reads NCHW: one permutation, then NHWC."""
    wm = f32(np.random.default_rng(3).uniform(-0.1, 0.1, (2 * 9 * 9, 2)))
    net = predictors.from_onnx(_model(
        [_node("ConvTranspose", ["x", "wt2", "bt2"], "t", kernel_shape=[3, 3], strides=[2, 2]),
         _node("Flatten", ["t"], "f", axis=1),
         _node("MatMul", ["f", "wm"], "y")],
        {"wt2": WT2, "bt2": BT2, "wm": wm}, chw=(3, 4, 4)))
    x = np.random.default_rng(4).uniform(-1, 1, (2, 3, 4, 4))
    t = torch.tensor
    a = F.conv_transpose2d(t(x), t(WT2), t(BT2), stride=2)
    want = (a.flatten(1) @ t(wm)).numpy()
    u = 2.0 ** -F_BITS
    e = np.abs(WT2).sum(axis=(0, 2, 3)).max() * u + 27 * u * (1 + u) + (4 * (3 + 1) + 1) * u
    e = np.abs(wm).sum(axis=0).max() * e + 162 * u * (float(a.abs().max()) + e) + (162 + 2) * u
    got = LocalMooseRuntime(ROLES, device="cpu").evaluate_computation(
        net.predictor_factory(), {"x": x})["output_0"]
    err = np.abs(got - want).max()
    print(f"decoder on the model input: err {err:.3e} tol {e:.3e}")
    assert got.shape == want.shape and err <= e


@pytest.mark.parametrize("t1,inputs,match", [
    (dict(kernel_shape=[4, 4], strides=[2, 2], pads=[1, 1, 1, 1], group=2), None,
     "ConvTranspose_t1.*group=2"),
    (dict(kernel_shape=[4, 4], strides=[2, 2], auto_pad="SAME_UPPER"), None,
     "ConvTranspose_t1.*auto_pad=SAME_UPPER"),
    (dict(kernel_shape=[4, 4], strides=[2, 2], output_shape=[8, 8]), None,
     "ConvTranspose_t1.*output_shape"),
    (None, ("r1", "c1", "bt1"), "ConvTranspose_t1.*not an initializer"),
    (None, ("r1", "wd", "bt1"), "ConvTranspose_t1.*not 2-D"),
    (None, ("r1", "wt2", "bt1"), "ConvTranspose_t1.*input channels"),
])
def test_unsupported_nodes_are_named(t1, inputs, match):
    nodes = _net(t1, inputs) if inputs else _net(t1)
    with pytest.raises(ValueError, match=match):
        predictors.from_onnx(_model(nodes, INITS))


def test_output_padding_not_below_the_stride_is_rejected():
    with pytest.raises(ValueError, match="output_padding"):
        predictors.from_onnx(_model(_net(dict(kernel_shape=[4, 4], strides=[2, 2],
                                              pads=[1, 1, 1, 1], output_padding=[2, 0])),
                                    INITS))


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_existing_fixtures_resolve_as_before(path):
    """No committed fixture has a ConvTranspose node: none turns into a ConvNetwork."""
    model = predictors.load_model(path)
    assert not any(n.op_type == "ConvTranspose" for n in model.graph.node)
    try:
        got = predictors.from_onnx(model)
    except ValueError:
        return
    assert not isinstance(got, conv.ConvNetwork)
