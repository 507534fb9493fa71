"""ConvNetwork: a small CNN built as ONNX bytes, imported with from_onnx and run on the
local runtime against the same network in float64 torch."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moose_amd.models import predictors
from moose_amd.models.predictors import conv
from moose_amd.models.predictors import linear
from moose_amd.models.predictors import neural
from moose_amd.models.predictors import onnx_proto as op
from moose_amd.models.predictors import trees
from moose_amd.runtime.local import LocalMooseRuntime

ROLES = ["alice", "bob", "carole"]
FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "fixtures", "onnx", "*.onnx")))
RNG = np.random.default_rng(12)
W1, B1 = RNG.uniform(-0.5, 0.5, (4, 2, 3, 3)), RNG.uniform(-0.5, 0.5, 4)
W2, B2 = RNG.uniform(-0.5, 0.5, (3, 4, 3, 3)), RNG.uniform(-0.5, 0.5, 3)
WD, BD = RNG.uniform(-0.5, 0.5, (5, 3)), RNG.uniform(-0.5, 0.5, 5)  # Gemm, transB = 1


def _tensor(name, a):
    a = np.asarray(a, dtype=np.float32)
    return op.make("TensorProto", name=name, dims=list(a.shape), data_type=1,
                   raw_data=a.tobytes())


def _node(kind, ins, out, **attrs):
    return op.make("NodeProto", input=list(ins), output=[out], name=f"{kind}_{out}",
                   op_type=kind, attribute=[op.attr(k, v) for k, v in attrs.items()])


def _model(nodes, inits, producer="pytorch"):
    dims = [op.make("Dimension", dim_param="N")] + [op.make("Dimension", dim_value=d)
                                                    for d in (2, 8, 8)]
    inp = op.make("ValueInfoProto", name="x", type=op.make(
        "TypeProto", tensor_type=op.make("TypeProtoTensor", elem_type=1,
                                         shape=op.make("TensorShapeProto", dim=dims))))
    out = op.make("ValueInfoProto", name="y", type=op.make(
        "TypeProto", tensor_type=op.make("TypeProtoTensor", elem_type=1)))
    graph = op.make("GraphProto", node=nodes, name="cnn", input=[inp], output=[out],
                    initializer=[_tensor(k, v) for k, v in inits.items()])
    return op.serialize(op.make("ModelProto", ir_version=8, producer_name=producer,
                                producer_version="2.0", graph=graph,
                                opset_import=[op.make("OperatorSetIdProto", domain="",
                                                      version=15)]))


INITS = {"w1": W1, "b1": B1, "w2": W2, "b2": B2, "wd": WD, "bd": BD}


def _cnn(conv1=None, pool1=None):
    return [
        _node("Conv", ["x", "w1", "b1"], "c1", **(conv1 or dict(
            kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[1, 1]))),
        _node("Relu", ["c1"], "r1"),
        _node("MaxPool", ["r1"], "p1", **(pool1 or dict(kernel_shape=[2, 2], strides=[2, 2]))),
        _node("Conv", ["p1", "w2", "b2"], "c2", kernel_shape=[3, 3]),
        _node("Relu", ["c2"], "r2"),
        _node("AveragePool", ["r2"], "p2", kernel_shape=[2, 2], strides=[2, 2]),
        _node("Flatten", ["p2"], "f", axis=1),
        _node("Gemm", ["f", "wd", "bd"], "g", transB=1),
        _node("Softmax", ["g"], "y", axis=1),
    ]


def _torch_reference(x):
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))  # noqa: E731
    t = F.relu(F.conv2d(torch.tensor(x), f32(W1), f32(B1), padding=1))
    t = F.max_pool2d(t, 2)
    t = F.relu(F.conv2d(t, f32(W2), f32(B2)))
    t = F.avg_pool2d(t, 2)
    return F.softmax(t.flatten(1) @ f32(WD).T + f32(BD), dim=1).numpy()


X = np.random.default_rng(13).uniform(-1, 1, (3, 2, 8, 8))
WANT = _torch_reference(X)


def test_from_onnx_returns_a_conv_network():
    net = predictors.from_onnx(_model(_cnn(), INITS))
    assert isinstance(net, conv.ConvNetwork) and isinstance(net, predictors.Predictor)
    assert net.input_chw == (2, 8, 8) and net.n_outputs == 5
    assert [l["op"] for l in net.layers] == ["conv", "relu", "maxpool", "conv", "relu",
                                             "avgpool", "flatten", "dense", "softmax"]
    assert [l["fmt"] for l in net.layers if "fmt" in l] == ["NCHW", "NHWC", "NHWC", "NHWC"]
    assert isinstance(predictors.from_onnx(_model(_cnn(), INITS, "tf2onnx")), conv.ConvNetwork)


def _check(device):
    net = predictors.from_onnx(_model(_cnn(), INITS))
    kw = {"use_graphs": True} if device != "cpu" else {}
    rt = LocalMooseRuntime(ROLES, device=device, **kw)
    comp = net.predictor_factory()
    for _ in range(2):  # with hipGraphs the second evaluation is a replay
        got = rt.evaluate_computation(comp, {"x": X})["output_0"]
        assert got.shape == WANT.shape
        err = np.abs(got - WANT).max()
        print(f"conv predictor on {device}: max abs error {err:.3e}")
        # the atol of the multi-layer softmax networks in tests/test_predictors.py
        np.testing.assert_allclose(got, WANT, atol=1e-2)


def test_predictor_matches_torch_cpu():
    _check("cpu")


@pytest.mark.gpu
def test_predictor_matches_torch_gpu():
    _check("cuda:0")


def test_first_dense_rows_follow_the_nhwc_flatten():
    c, h, w, out = 3, 2, 4, 5
    rng = np.random.default_rng(2)
    act = rng.normal(size=(6, c, h, w))  # NCHW activation
    dense = rng.normal(size=(c * h * w, out))
    nchw_flat = act.reshape(6, -1)
    nhwc_flat = act.transpose(0, 2, 3, 1).reshape(6, -1)
    assert np.allclose(nhwc_flat @ conv.hwc_rows(dense, c, h, w), nchw_flat @ dense,
                       rtol=0, atol=1e-12)
    assert not np.allclose(nhwc_flat @ dense, nchw_flat @ dense)


@pytest.mark.parametrize("bad,match", [
    (dict(conv1=dict(kernel_shape=[3, 3], pads=[1, 1, 1, 1], group=2)), "Conv_c1.*group=2"),
    (dict(pool1=dict(kernel_shape=[2, 2], strides=[2, 2], ceil_mode=1)), "MaxPool_p1.*ceil_mode"),
    (dict(pool1=dict(kernel_shape=[2, 2], strides=[2, 2], pads=[1, 1, 1, 1])),
     "MaxPool_p1.*pads"),
])
def test_unsupported_nodes_are_named(bad, match):
    with pytest.raises(ValueError, match=match):
        predictors.from_onnx(_model(_cnn(**bad), INITS))


def test_unknown_operator_is_named():
    nodes = _cnn()
    nodes.insert(2, _node("LRN", ["r1"], "r1", size=3))
    with pytest.raises(ValueError, match="LRN_r1"):
        predictors.from_onnx(_model(nodes, INITS))


def _resolve_as_before(model):
    """The dispatch of from_onnx before convolutional networks existed."""
    if model.producer_name in ("pytorch", "tf2onnx"):
        return neural.NeuralNetwork
    ops = [n.op_type for n in model.graph.node]
    known = {"LinearRegressor": linear.LinearRegressor,
             "LinearClassifier": linear.LinearClassifier,
             "TreeEnsembleRegressor": trees.TreeEnsembleRegressor,
             "TreeEnsembleClassifier": trees.TreeEnsembleClassifier}
    found = [o for o in ops if o in known]
    if len(found) == 1:
        return known[found[0]]
    if not found and sum(1 for t in model.graph.initializer if "coefficient" in t.name) > 1:
        return neural.MLPClassifier if "ZipMap" in ops else neural.MLPRegressor
    return None


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_existing_fixtures_resolve_as_before(path):
    model = predictors.load_model(path)
    want = _resolve_as_before(model)
    if want is None:
        with pytest.raises(ValueError):
            predictors.from_onnx(model)
        return
    got = predictors.from_onnx(model)
    assert type(got) is want and not isinstance(got, conv.ConvNetwork)
