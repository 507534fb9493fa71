"""ConvNetwork with the piecewise-linear activations and Tanh: a MobileNet-style block and a
small decoder built as ONNX bytes, imported with from_onnx and run on the local runtime
against the same networks in float64 torch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moose_amd.models import predictors
from moose_amd.models.predictors import conv
from moose_amd.models.predictors import onnx_proto as op
from moose_amd.runtime.local import LocalMooseRuntime

ROLES = ["alice", "bob", "carole"]
RNG = np.random.default_rng(31)
f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
# model one, 2x6x6: Conv 3x3 (pad 1) -> Clip(0, 6) -> depthwise 3x3 -> HardSwish -> dense
W1, B1 = f32(RNG.uniform(-1.5, 1.5, (4, 2, 3, 3))), f32(RNG.uniform(-0.5, 0.5, 4))
WDW, BDW = f32(RNG.uniform(-1, 1, (4, 1, 3, 3))), f32(RNG.uniform(-0.5, 0.5, 4))
WD, BD = f32(RNG.uniform(-0.3, 0.3, (5, 4 * 4 * 4))), f32(RNG.uniform(-0.5, 0.5, 5))
# model two, 6x1x1: dense -> [3, 4, 4] -> ConvTranspose 4x4 s2 p1 -> LeakyRelu -> Conv -> Tanh
WG, BG = f32(RNG.uniform(-1, 1, (6, 3 * 4 * 4))), f32(RNG.uniform(-0.5, 0.5, 3 * 4 * 4))
WT, BT = f32(RNG.uniform(-0.5, 0.5, (3, 4, 4, 4))), f32(RNG.uniform(-0.5, 0.5, 4))
W2, B2 = f32(RNG.uniform(-0.3, 0.3, (2, 4, 3, 3))), f32(RNG.uniform(-0.3, 0.3, 2))
ALPHA = 0.125


def _tensor(name, a):
    a = np.asarray(a)
    if a.dtype.kind == "i":
        a = a.astype(np.int64)
        return op.make("TensorProto", name=name, dims=list(a.shape), data_type=7,
                       raw_data=a.tobytes())
    a = a.astype(np.float32)
    return op.make("TensorProto", name=name, dims=list(a.shape), data_type=1,
                   raw_data=a.tobytes())


def _node(kind, ins, out, **attrs):
    return op.make("NodeProto", input=list(ins), output=[out], name=f"{kind}_{out}",
                   op_type=kind, attribute=[op.attr(k, v) for k, v in attrs.items()])


def _model(nodes, inits, chw, opset=15):
    dims = [op.make("Dimension", dim_param="N")] + [op.make("Dimension", dim_value=d)
                                                    for d in chw]
    inp = op.make("ValueInfoProto", name="x", type=op.make(
        "TypeProto", tensor_type=op.make("TypeProtoTensor", elem_type=1,
                                         shape=op.make("TensorShapeProto", dim=dims))))
    out = op.make("ValueInfoProto", name="y", type=op.make(
        "TypeProto", tensor_type=op.make("TypeProtoTensor", elem_type=1)))
    graph = op.make("GraphProto", node=nodes, name="net", input=[inp], output=[out],
                    initializer=[_tensor(k, v) for k, v in inits.items()])
    return op.serialize(op.make("ModelProto", ir_version=8, producer_name="pytorch",
                                producer_version="2.0", graph=graph,
                                opset_import=[op.make("OperatorSetIdProto", domain="",
                                                      version=opset)]))


INITS1 = {"w1": W1, "b1": B1, "wdw": WDW, "bdw": BDW, "wd": WD, "bd": BD,
          "lo": np.float32(0.0).reshape(()), "hi": np.float32(6.0).reshape(())}


def _one(clip=None, act="HardSwish", act_inputs=("d1",), inits=INITS1, **act_attrs):
    nodes = [
        _node("Conv", ["x", "w1", "b1"], "c1", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
        clip or _node("Clip", ["c1", "lo", "hi"], "a1"),
        _node("Conv", ["a1", "wdw", "bdw"], "d1", kernel_shape=[3, 3], group=4),
        _node(act, list(act_inputs), "a2", **act_attrs),
        _node("Flatten", ["a2"], "f", axis=1),
        _node("Gemm", ["f", "wd", "bd"], "y", transB=1),
    ]
    return _model(nodes, inits, (2, 6, 6))


def _torch_one(x, lo=0.0, hi=6.0, act=F.hardswish):
    t = torch.tensor
    a = torch.clamp(F.conv2d(t(x), t(W1), t(B1), padding=1), lo, hi)
    a = act(F.conv2d(a, t(WDW), t(BDW), groups=4))
    return (a.flatten(1) @ t(WD).T + t(BD)).numpy()


INITS2 = {"wg": WG, "bg": BG, "shape": np.array([-1, 3, 4, 4]), "wt": WT, "bt": BT, "w2": W2,
          "b2": B2}


def _two():
    nodes = [
        _node("Flatten", ["x"], "f", axis=1),
        _node("Gemm", ["f", "wg", "bg"], "g"),
        _node("Reshape", ["g", "shape"], "img"),
        _node("ConvTranspose", ["img", "wt", "bt"], "t1", kernel_shape=[4, 4], strides=[2, 2],
              pads=[1, 1, 1, 1]),
        _node("LeakyRelu", ["t1"], "a1", alpha=ALPHA),
        _node("Conv", ["a1", "w2", "b2"], "c2", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
        _node("Tanh", ["c2"], "y"),
    ]
    return _model(nodes, INITS2, (6, 1, 1))


def _torch_two(x):
    t = torch.tensor
    a = (t(x).flatten(1) @ t(WG) + t(BG)).reshape(-1, 3, 4, 4)
    a = F.leaky_relu(F.conv_transpose2d(a, t(WT), t(BT), stride=2, padding=1), ALPHA)
    a = torch.tanh(F.conv2d(a, t(W2), t(B2), padding=1))
    return a.permute(0, 2, 3, 1).numpy()  # the predictor answers NHWC


X1 = np.random.default_rng(32).uniform(-1, 1, (3, 2, 6, 6))
X2 = np.random.default_rng(33).uniform(-1, 1, (3, 6, 1, 1))
WANT1, WANT2 = _torch_one(X1), _torch_two(X2)


def test_from_onnx_reads_the_activations():
    net = predictors.from_onnx(_one())
    assert isinstance(net, conv.ConvNetwork) and net.n_outputs == 5
    assert [l["op"] for l in net.layers] == ["conv", "clip", "conv", "hardswish", "flatten",
                                             "dense"]
    assert net.layers[1]["lo"] == 0.0 and net.layers[1]["hi"] == 6.0
    assert net.layers[2]["group"] == 4
    net = predictors.from_onnx(_two())
    assert [l["op"] for l in net.layers] == ["flatten", "dense", "unflatten", "convtranspose",
                                             "leakyrelu", "conv", "tanh"]
    assert net.layers[2]["out_chw"] == (3, 4, 4) and net.layers[3]["fmt"] == "NCHW"
    assert net.layers[4]["alpha"] == ALPHA and net.layers[5]["fmt"] == "NHWC"
    # the interior of a MobileNet block saturates: the Clip is not the identity here
    t = torch.tensor
    pre = F.conv2d(t(X1), t(W1), t(B1), padding=1)
    assert float(pre.max()) > 6 and float(pre.min()) < 0


def _check(device):
    kw = {"use_graphs": True} if device != "cpu" else {}
    for model, x, want in ((_one(), X1, WANT1), (_two(), X2, WANT2)):
        net = predictors.from_onnx(model)
        rt = LocalMooseRuntime(ROLES, device=device, **kw)
        comp = net.predictor_factory()
        for _ in range(2):  # with hipGraphs the second evaluation is a replay
            got = rt.evaluate_computation(comp, {"x": x})["output_0"]
            assert got.shape == want.shape
            err = np.abs(got - want).max()
            print(f"{[l['op'] for l in net.layers][1]} model on {device}: max abs error {err:.3e}")
            # the atol of tests/test_conv_predictor.py
            np.testing.assert_allclose(got, want, atol=1e-2)


def test_predictors_match_torch_cpu():
    _check("cpu")


@pytest.mark.gpu
def test_predictors_match_torch_gpu():
    _check("cuda:0")


@pytest.mark.parametrize("clip,lo,hi", [
    (_node("Clip", ["c1"], "a1", min=-0.5, max=2.0), -0.5, 2.0),       # opset 6 attributes
    (_node("Clip", ["c1", "lo"], "a1"), 0.0, None),                    # lower bound alone
    (_node("Clip", ["c1", "", "hi"], "a1"), None, 6.0),                # upper bound alone
])
def test_clip_bounds_from_attributes_and_one_sided(clip, lo, hi):
    net = predictors.from_onnx(_one(clip=clip))
    assert net.layers[1] == {"op": "clip", "lo": lo, "hi": hi}
    got = LocalMooseRuntime(ROLES, device="cpu").evaluate_computation(
        net.predictor_factory(), {"x": X1})["output_0"]
    inf = float("inf")
    want = _torch_one(X1, -inf if lo is None else lo, inf if hi is None else hi)
    np.testing.assert_allclose(got, want, atol=1e-2)


@pytest.mark.parametrize("act,inputs,attrs,ref", [
    ("PRelu", ("d1", "slope"), {}, lambda a: F.leaky_relu(a, 0.25)),
    ("HardSigmoid", ("d1",), {"alpha": 0.25, "beta": 0.5},
     lambda a: torch.clamp(0.25 * a + 0.5, 0, 1)),
    ("ThresholdedRelu", ("d1",), {"alpha": 0.5}, lambda a: torch.where(a > 0.5, a, 0 * a)),
])
def test_other_activations_match_torch(act, inputs, attrs, ref):
    inits = dict(INITS1, slope=np.array([0.25], np.float32))
    net = predictors.from_onnx(_one(act=act, act_inputs=inputs, inits=inits, **attrs))
    got = LocalMooseRuntime(ROLES, device="cpu").evaluate_computation(
        net.predictor_factory(), {"x": X1})["output_0"]
    want = _torch_one(X1, act=ref)
    if act == "ThresholdedRelu":
        # discontinuous: an activation within the fixed-point error of the threshold may fall
        # on either side, so the inputs of this check must stay clear of it
        t = torch.tensor
        a = F.conv2d(torch.clamp(F.conv2d(t(X1), t(W1), t(B1), padding=1), 0, 6), t(WDW),
                     t(BDW), groups=4)
        assert float((a - 0.5).abs().min()) > 1e-6
    np.testing.assert_allclose(got, want, atol=1e-2)


def test_per_channel_prelu_and_bad_bounds_are_rejected_by_name():
    inits = dict(INITS1, slope=np.full((4, 1, 1), 0.25, np.float32))
    with pytest.raises(ValueError, match="PRelu_a2.*per-channel slope of 4 elements"):
        predictors.from_onnx(_one(act="PRelu", act_inputs=("d1", "slope"), inits=inits))
    with pytest.raises(ValueError, match="PRelu_a2.*not an initializer"):
        predictors.from_onnx(_one(act="PRelu", act_inputs=("d1", "c1")))
    with pytest.raises(ValueError, match="Clip_a1.*without bounds"):
        predictors.from_onnx(_one(clip=_node("Clip", ["c1"], "a1")))
    with pytest.raises(ValueError, match="Clip_a1.*not below"):
        predictors.from_onnx(_one(clip=_node("Clip", ["c1"], "a1", min=2.0, max=1.0)))
    with pytest.raises(ValueError, match="Clip_a1.*`min` input is not an initializer"):
        predictors.from_onnx(_one(clip=_node("Clip", ["c1", "x"], "a1")))
    with pytest.raises(ValueError, match="HardSigmoid_a2.*alpha"):
        predictors.from_onnx(_one(act="HardSigmoid", alpha=-1.0))
    with pytest.raises(ValueError, match="Gelu_a2.*not an operator"):
        predictors.from_onnx(_one(act="Gelu"))


def test_reshape_to_an_image_needs_a_matching_dense_layer():
    bad = dict(INITS2, shape=np.array([-1, 3, 4, 5]))
    with pytest.raises(ValueError, match="Reshape to the image"):
        predictors.from_onnx(_model(_two_nodes_with(bad), bad, (6, 1, 1)))
    # a Reshape that follows no dense layer stays what it was: only [N, -1]
    nodes = [_node("Reshape", ["x", "shape"], "img"),
             _node("Conv", ["img", "w2", "b2"], "y", kernel_shape=[3, 3])]
    with pytest.raises(ValueError, match="Reshape_img.*only a Reshape to"):
        predictors.from_onnx(_model(nodes, INITS2, (6, 1, 1)))


def _two_nodes_with(_inits):
    return [
        _node("Flatten", ["x"], "f", axis=1),
        _node("Gemm", ["f", "wg", "bg"], "g"),
        _node("Reshape", ["g", "shape"], "img"),
        _node("ConvTranspose", ["img", "wt", "bt"], "t1", kernel_shape=[4, 4], strides=[2, 2]),
    ]
