"""Convolutional networks exported from PyTorch or Keras/tf2onnx.

The reference has no convolution; this predictor is this framework's own.  A graph is a
chain of ``Conv`` (any ``group`` that divides the channels: ``group = C`` is the depthwise
operator, other groups a composition of per-group products), ``ConvTranspose`` (``group = 1``, explicit ``pads`` and ``output_padding``: a ``dot`` of the
pixels followed by the ``col2im`` sum), ``Resize`` (opset 11+) / ``Upsample`` (opset 7, 9) in
``nearest`` or ``linear`` mode with constant ``scales`` / ``sizes`` (``pm.resize2d`` in the
activation's layout), ``Relu`` / ``Sigmoid`` / ``Tanh``, the piecewise-linear activations ``Clip``
(attribute or initializer bounds, one-sided included), ``LeakyRelu``, ``PRelu`` (one slope),
``HardSigmoid``, ``HardSwish`` and ``ThresholdedRelu``, the smooth activations ``Gelu`` (both
``approximate`` values), ``Mish``, ``Softplus``, ``Elu``, ``Selu`` (default constants), ``Celu``,
``Erf`` and ``Swish`` (``alpha = 1``) as one piecewise polynomial each, in a model whose opset has
the operator, ``MaxPool`` / ``AveragePool``,
``Flatten`` (or ``Reshape`` to ``[N, -1]``), ``Gemm`` / ``MatMul`` + ``Add``, a ``Reshape`` of a
dense layer's output back to an image ``[N, C, H, W]`` (a decoder's first step) and a final
``Softmax``.  The model input is rank 4, NCHW.  Inside the MPC the activations are NHWC from
the first convolution on, so no permutation ever runs on shares: the first ``im2col`` reads
NCHW, the convolution weights are re-ordered to the patch matrix's (kh, kw, c) rows and the
first dense layer's rows from the ONNX (c, h, w) flatten order to (h, w, c), all in numpy when
the model is loaded.  Weights are mirrored fixed-point constants, as in ``DenseNetwork``.
"""
from __future__ import annotations

import numpy as np

import moose_amd as pm
from moose_amd.models.predictors import onnx_proto
from moose_amd.models.predictors.base import DEFAULT_FIXED_DTYPE
from moose_amd.models.predictors.base import Predictor
from moose_amd.models.predictors.base import find_attribute
from moose_amd.models.predictors.base import initializers
from moose_amd.models.predictors.base import load_onnx


def _ints(node, name, default):
    a = find_attribute(node, name, enforce=False)
    return tuple(int(v) for v in a.ints) if a is not None and list(a.ints) else tuple(default)


def _int(node, name, default=0):
    a = find_attribute(node, name, enforce=False)
    return int(a.i) if a is not None else default


def _unsupported(node, why):
    return ValueError(f"unsupported ONNX node {node.name or node.op_type} ({node.op_type}): {why}")


def _window_attrs(node):
    """(kernel_shape, strides, pads) of a pooling node, rejecting what the MPC does not run."""
    ap = find_attribute(node, "auto_pad", enforce=False)
    if ap is not None and ap.s not in (b"", b"NOTSET"):
        raise _unsupported(node, f"auto_pad={ap.s.decode()}")
    if _int(node, "ceil_mode"):
        raise _unsupported(node, "ceil_mode=1")
    kernel = _ints(node, "kernel_shape", ())
    if len(kernel) != 2:
        raise _unsupported(node, f"kernel_shape {kernel} is not 2-D")
    if any(d != 1 for d in _ints(node, "dilations", (1, 1))):
        raise _unsupported(node, "dilations")
    return kernel, _ints(node, "strides", (1, 1)), _ints(node, "pads", (0, 0, 0, 0))


def _str(node, name, default):
    a = find_attribute(node, name, enforce=False)
    return a.s.decode() if a is not None and a.s else default


def _float(node, name, default):
    a = find_attribute(node, name, enforce=False)
    return float(a.f) if a is not None else default


def _scalar_operand(node, init, index, what):
    """The one-element constant input ``index`` of a node as a float; None when it is absent
    or empty-named."""
    if len(node.input) <= index or not node.input[index]:
        return None
    if node.input[index] not in init:
        raise _unsupported(node, f"its `{what}` input is not an initializer or a Constant")
    v = np.asarray(init[node.input[index]], dtype=np.float64).reshape(-1)
    if v.size != 1:
        raise _unsupported(node, f"its `{what}` input has {v.size} elements, not 1")
    return float(v[0])


def _activation_layer(node, init):
    """The layer of a piecewise-linear activation node (or Tanh)."""
    op = node.op_type
    if op == "Clip":
        lo = find_attribute(node, "min", enforce=False)  # opset < 11: attributes
        hi = find_attribute(node, "max", enforce=False)
        lo = float(lo.f) if lo is not None else _scalar_operand(node, init, 1, "min")
        hi = float(hi.f) if hi is not None else _scalar_operand(node, init, 2, "max")
        # float32's extremes stand for "no bound" in exported graphs
        big = float(np.finfo(np.float32).max)
        lo = None if lo is not None and lo <= -big else lo
        hi = None if hi is not None and hi >= big else hi
        if lo is None and hi is None:
            raise _unsupported(node, "a Clip without bounds")
        if lo is not None and hi is not None and not lo < hi:
            raise _unsupported(node, f"min={lo} is not below max={hi}")
        return {"op": "clip", "lo": lo, "hi": hi}
    if op == "LeakyRelu":
        return {"op": "leakyrelu", "alpha": _float(node, "alpha", 0.01)}
    if op == "PRelu":
        if len(node.input) < 2 or node.input[1] not in init:
            raise _unsupported(node, "its slope is not an initializer or a Constant")
        slope = np.asarray(init[node.input[1]], dtype=np.float64).reshape(-1)
        if slope.size != 1:
            raise _unsupported(node, f"a per-channel slope of {slope.size} elements: only a "
                                     "one-element slope is supported")
        return {"op": "leakyrelu", "alpha": float(slope[0])}
    if op == "HardSigmoid":
        alpha = _float(node, "alpha", 0.2)
        if not alpha > 0:
            raise _unsupported(node, f"alpha={alpha} is not positive")
        return {"op": "hardsigmoid", "alpha": alpha, "beta": _float(node, "beta", 0.5)}
    if op == "ThresholdedRelu":
        return {"op": "thresholdedrelu", "alpha": _float(node, "alpha", 1.0)}
    return {"op": op.lower()}  # HardSwish, Tanh


# the smooth activations (one PiecewisePolynomial operator each): the opset of the default
# domain that introduced the operator, and the attributes it may carry
_SMOOTH = {"Gelu": (20, ("approximate",)), "Mish": (18, ()), "Softplus": (1, ()),
           "Elu": (1, ("alpha",)), "Selu": (1, ("alpha", "gamma")), "Celu": (12, ("alpha",)),
           "Erf": (9, ()), "Swish": (24, ("alpha",))}
_SELU = (1.6732632423543772, 1.0507009873554805)  # ONNX Selu's default alpha and gamma


def _smooth_layer(node, opset):
    """The layer of a smooth activation node."""
    op = node.op_type
    since, allowed = _SMOOTH[op]
    if 0 < opset < since:
        raise _unsupported(node, f"not an operator of opset {opset}: {op} enters the default "
                                 f"domain with opset {since}")
    extra = sorted(a.name for a in node.attribute if a.name not in allowed)
    if extra:
        raise _unsupported(node, f"unsupported attribute(s) {', '.join(extra)}")
    if op == "Gelu":
        approximate = _str(node, "approximate", "none")
        if approximate not in ("none", "tanh"):
            raise _unsupported(node, f"approximate={approximate!r} is neither 'none' nor 'tanh'")
        return {"op": "gelu", "approximate": approximate}
    if op in ("Elu", "Celu"):
        alpha = _float(node, "alpha", 1.0)
        if op == "Celu" and alpha == 0:
            raise _unsupported(node, "alpha=0")
        return {"op": op.lower(), "alpha": alpha}
    if op == "Selu":
        got = (_float(node, "alpha", _SELU[0]), _float(node, "gamma", _SELU[1]))
        if any(abs(g - w) > 1e-6 for g, w in zip(got, _SELU)):
            raise _unsupported(node, f"alpha={got[0]}, gamma={got[1]}: only the default "
                                     "self-normalising constants are supported")
        return {"op": "selu"}
    if op == "Swish":
        alpha = _float(node, "alpha", 1.0)
        if alpha != 1.0:
            raise _unsupported(node, f"alpha={alpha}: only x * sigmoid(x) is supported")
        return {"op": "silu"}
    return {"op": op.lower()}  # Mish, Softplus, Erf


def _opset(model):
    """Version of the default ONNX operator set the model imports (0: not stated)."""
    return max((int(o.version) for o in model.opset_import if o.domain in ("", "ai.onnx")),
               default=0)


def _resize_operand(node, init, index, what):
    """The constant input ``index`` of a Resize / Upsample node as a flat array; None when
    it is absent, empty-named or empty."""
    if len(node.input) <= index or not node.input[index]:
        return None
    if node.input[index] not in init:
        raise _unsupported(node, f"its `{what}` input is not an initializer or a Constant")
    v = np.asarray(init[node.input[index]]).reshape(-1)
    return v if v.size else None


def _resize_layer(node, init, opset):
    """The ``resize`` layer of an ONNX ``Resize`` (opset 11+) or ``Upsample`` (7, 9) node."""
    mode = _str(node, "mode", "nearest")
    if node.op_type == "Upsample":
        ctm, nearest = "asymmetric", "floor"
        mode = "linear" if mode == "bilinear" else mode
        a = find_attribute(node, "scales", enforce=False)
        if a is not None and list(a.floats):  # opset 7: an attribute
            scales, sizes = np.asarray(list(a.floats), dtype=np.float32), None
        else:  # opset 9: an input
            scales, sizes = _resize_operand(node, init, 1, "scales"), None
    else:
        if opset and opset < 11:
            raise _unsupported(node, f"Resize of opset {opset}: opset 11 or later is supported")
        ctm = _str(node, "coordinate_transformation_mode", "half_pixel")
        nearest = _str(node, "nearest_mode", "round_prefer_floor")
        if ctm == "tf_crop_and_resize":
            raise _unsupported(node, "coordinate_transformation_mode=tf_crop_and_resize")
        if _int(node, "antialias"):
            raise _unsupported(node, "antialias=1")
        if _int(node, "exclude_outside"):
            raise _unsupported(node, "exclude_outside=1")
        if _ints(node, "axes", ()):
            raise _unsupported(node, "an `axes` attribute (give all four scales or sizes)")
        policy = _str(node, "keep_aspect_ratio_policy", "stretch")
        if policy != "stretch":
            raise _unsupported(node, f"keep_aspect_ratio_policy={policy}")
        scales = _resize_operand(node, init, 2, "scales")  # input 1 is roi: ignored
        sizes = _resize_operand(node, init, 3, "sizes")
    if mode not in ("nearest", "linear"):
        raise _unsupported(node, f"mode={mode}: nearest and linear are supported")
    if ctm not in ("half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric"):
        raise _unsupported(node, f"coordinate_transformation_mode={ctm}")
    if nearest not in ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil"):
        raise _unsupported(node, f"nearest_mode={nearest}")
    if (scales is None) == (sizes is None):
        raise _unsupported(node, "exactly one of `scales` and `sizes` must be given")
    given = scales if scales is not None else sizes
    if len(given) != 4:
        raise _unsupported(node, f"{len(given)} scales / sizes: a rank-4 input needs 4")
    layer = {"op": "resize", "mode": mode, "ctm": ctm, "nearest_mode": nearest}
    if scales is not None:
        if float(scales[0]) != 1 or float(scales[1]) != 1:
            raise _unsupported(node, f"batch / channel scales {tuple(map(float, scales[:2]))} "
                                     "are not 1")
        layer["scales"] = (float(scales[2]), float(scales[3]))
    else:
        layer["sizes_nchw"] = tuple(int(s) for s in sizes)
    return layer


def hwc_rows(w, c, h, w_):
    """Rows of a dense weight ``[c*h*w_, out]`` moved from the (c, h, w) flatten order of an
    NCHW activation to the (h, w, c) order of its NHWC form."""
    w = np.asarray(w)
    return w.reshape(c, h, w_, -1).transpose(1, 2, 0, 3).reshape(c * h * w_, -1)


def conv_layers_from_onnx(model):
    """-> (input (C, H, W), layers): each layer a dict with ``op`` in conv / convtranspose /
    resize / relu / sigmoid / tanh / clip / leakyrelu / hardsigmoid / hardswish /
    thresholdedrelu / gelu / silu / mish / softplus / elu / selu / celu / erf / maxpool /
    avgpool / flatten / dense / unflatten / softmax and its parameters (ONNX layouts)."""
    dims = model.graph.input[0].type.tensor_type.shape.dim
    if len(dims) != 4:
        raise ValueError("a convolutional predictor expects a rank-4 [batch, C, H, W] model input")
    chw = tuple(int(d.dim_value) for d in dims[1:])
    if min(chw) <= 0:
        raise ValueError(f"the model input's channel and image sizes must be static, found {chw}")
    init = dict(initializers(model))
    opset = _opset(model)
    layers = []
    channels = chw[0]  # of the activation that reaches the next Conv
    for node in model.graph.node:
        op = node.op_type
        if op == "Constant":
            t = find_attribute(node, "value", enforce=False)
            if t is None:
                raise _unsupported(node, "a Constant without a tensor value")
            init[node.output[0]] = onnx_proto.to_array(t.t)
        elif op == "Conv":
            group = _int(node, "group", 1)
            ap = find_attribute(node, "auto_pad", enforce=False)
            if ap is not None and ap.s not in (b"", b"NOTSET"):
                raise _unsupported(node, f"auto_pad={ap.s.decode()}")
            if len(node.input) < 2 or node.input[1] not in init:
                raise _unsupported(node, "its weight is not an initializer")
            w = np.asarray(init[node.input[1]], dtype=np.float64)
            if w.ndim != 4:
                raise _unsupported(node, f"weight of shape {w.shape} is not 2-D")
            if group < 1 or channels % group or w.shape[0] % group:
                raise _unsupported(node, f"group={group} does not divide the {channels} input "
                                         f"and {w.shape[0]} output channels")
            if w.shape[1] * group != channels:
                raise _unsupported(node, f"group={group} with a weight of shape {w.shape} does "
                                         f"not match {channels} input channels")
            channels = w.shape[0]
            b = init[node.input[2]] if len(node.input) > 2 else np.zeros(w.shape[0])
            layers.append({"op": "conv", "w": w, "group": group, "b": np.asarray(b, np.float64).reshape(-1),
                           "strides": _ints(node, "strides", (1, 1)),
                           "pads": _ints(node, "pads", (0, 0, 0, 0)),
                           "dilations": _ints(node, "dilations", (1, 1))})
        elif op == "ConvTranspose":
            group = _int(node, "group", 1)
            if group != 1:
                raise _unsupported(node, f"group={group}: only group=1 is supported")
            ap = find_attribute(node, "auto_pad", enforce=False)
            if ap is not None and ap.s not in (b"", b"NOTSET"):
                raise _unsupported(node, f"auto_pad={ap.s.decode()}")
            if _ints(node, "output_shape", ()):
                raise _unsupported(node, "an explicit output_shape (give pads and "
                                         "output_padding instead)")
            if len(node.input) < 2 or node.input[1] not in init:
                raise _unsupported(node, "its weight is not an initializer")
            w = np.asarray(init[node.input[1]], dtype=np.float64)
            if w.ndim != 4:
                raise _unsupported(node, f"weight of shape {w.shape} is not 2-D")
            if w.shape[0] != channels:
                raise _unsupported(node, f"a weight of shape {w.shape} does not match "
                                         f"{channels} input channels")
            channels = w.shape[1]
            b = init[node.input[2]] if len(node.input) > 2 else np.zeros(w.shape[1])
            layers.append({"op": "convtranspose", "w": w,
                           "b": np.asarray(b, np.float64).reshape(-1),
                           "strides": _ints(node, "strides", (1, 1)),
                           "pads": _ints(node, "pads", (0, 0, 0, 0)),
                           "dilations": _ints(node, "dilations", (1, 1)),
                           "output_padding": _ints(node, "output_padding", (0, 0))})
        elif op in ("Resize", "Upsample"):
            layer = _resize_layer(node, init, opset)
            nc = layer.pop("sizes_nchw", None)
            if nc is not None:
                if nc[1] != channels:
                    raise _unsupported(node, f"sizes {nc} change the {channels} channels "
                                             "(batch / channel scales are not 1)")
                layer["sizes"] = nc[2:]  # (the batch entry is the export's; the batch is free)
            layers.append(layer)
        elif op in ("Relu", "Sigmoid"):
            layers.append({"op": op.lower()})
        elif op in ("Clip", "LeakyRelu", "PRelu", "HardSigmoid", "HardSwish",
                    "ThresholdedRelu", "Tanh"):
            layers.append(_activation_layer(node, init))
        elif op in _SMOOTH:
            layers.append(_smooth_layer(node, _opset(model)))
        elif op == "MaxPool":
            kernel, strides, pads = _window_attrs(node)
            if any(pads):
                raise _unsupported(node, f"pads={pads}")
            layers.append({"op": "maxpool", "kernel": kernel, "strides": strides})
        elif op == "AveragePool":
            kernel, strides, pads = _window_attrs(node)
            if any(pads) and not _int(node, "count_include_pad"):
                raise _unsupported(node, f"pads={pads} without count_include_pad=1")
            layers.append({"op": "avgpool", "kernel": kernel, "strides": strides, "pads": pads})
        elif op == "Flatten":
            if _int(node, "axis", 1) != 1:
                raise _unsupported(node, f"axis={_int(node, 'axis', 1)}")
            layers.append({"op": "flatten"})
        elif op == "Reshape":
            shape = init.get(node.input[1]) if len(node.input) > 1 else None
            shape = None if shape is None else [int(s) for s in np.asarray(shape).reshape(-1)]
            if (shape is not None and len(shape) == 4 and min(shape[1:]) > 0 and layers
                    and layers[-1]["op"] == "dense"):  # a decoder: dense -> image
                layers.append({"op": "unflatten", "out_chw": tuple(shape[1:])})
                channels = shape[1]
                continue
            if shape is None or len(shape) != 2 or -1 not in shape:
                raise _unsupported(node, f"only a Reshape to [N, -1] is supported, found {shape}")
            layers.append({"op": "flatten"})
        elif op == "Gemm" and len(node.input) >= 2 and node.input[1] in init:
            w = np.asarray(init[node.input[1]], dtype=np.float64)
            if _int(node, "transB"):
                w = w.T
            if _int(node, "transA"):
                raise _unsupported(node, "transA=1")
            alpha = find_attribute(node, "alpha", enforce=False)
            if alpha is not None:  # present: its value holds, an explicit 0 included
                w = w * float(alpha.f)
            b = init[node.input[2]] if len(node.input) > 2 else np.zeros(w.shape[1])
            beta = find_attribute(node, "beta", enforce=False)
            if beta is not None:
                b = np.asarray(b, np.float64) * float(beta.f)
            layers.append({"op": "dense", "w": w, "b": np.asarray(b, np.float64).reshape(-1)})
        elif op == "MatMul" and len(node.input) == 2 and node.input[1] in init:
            w = np.asarray(init[node.input[1]], dtype=np.float64)
            layers.append({"op": "dense", "w": w, "b": np.zeros(w.shape[1])})
        elif (op == "Add" and layers and layers[-1]["op"] == "dense"
              and any(i in init for i in node.input)):
            b = init[next(i for i in node.input if i in init)]
            layers[-1]["b"] = layers[-1]["b"] + np.asarray(b, np.float64).reshape(-1)
        elif op == "Softmax":
            layers.append({"op": "softmax"})
        else:
            raise _unsupported(node, "not an operator of a convolutional predictor")
    if any(l["op"] == "softmax" for l in layers[:-1]):
        raise ValueError("unsupported ONNX graph: Softmax is only supported as the final node")
    if not any(l["op"] in ("conv", "convtranspose") for l in layers):
        raise ValueError("no Conv node found in the ONNX graph")
    return chw, layers


class ConvNetwork(Predictor):
    """A convolutional network (see the module doc); ``input_chw`` is the model input's
    (C, H, W), the batch size is free."""

    def __init__(self, input_chw, layers):
        super().__init__()
        self.input_chw = tuple(int(v) for v in input_chw)
        self.layers = [dict(l) for l in layers]
        self._plan()

    @classmethod
    def from_onnx(cls, model):
        return cls(*conv_layers_from_onnx(load_onnx(model)))

    def _plan(self):
        """Walk the layers once in numpy: per-layer activation shapes, the layouts (NCHW
        until the first convolution, NHWC after it) and the re-ordered weight matrices."""
        c, h, w = self.input_chw
        fmt, flat = "NCHW", None
        for l in self.layers:
            op = l["op"]
            if op in ("conv", "convtranspose", "resize", "maxpool", "avgpool") and \
                    flat is not None:
                raise ValueError(f"unsupported ONNX graph: {op} after Flatten")
            if op == "conv":
                oc, wc, kh, kw = l["w"].shape
                group = l.setdefault("group", 1)
                if group < 1 or c % group or oc % group or wc * group != c:
                    raise ValueError(f"Conv weight {l['w'].shape} with group={group} does not "
                                     f"match {c} channels")
                l.update(fmt=fmt, chw=(c, h, w), kernel=(kh, kw))
                if group > 1:  # the ONNX weight as it is: pm.conv2d(groups=) takes it
                    pass
                elif fmt == "NCHW":  # columns (c, kh, kw): the ONNX weight as it is
                    l["wm"] = l["w"].reshape(oc, -1).T
                else:  # columns (kh, kw, c)
                    l["wm"] = l["w"].transpose(2, 3, 1, 0).reshape(-1, oc)
                h, w = _out_hw(h, w, (kh, kw), l["strides"], l["pads"], l["dilations"])
                c, fmt = oc, "NHWC"
            elif op == "convtranspose":
                wc, oc, kh, kw = l["w"].shape
                if wc != c:
                    raise ValueError(f"ConvTranspose weight {l['w'].shape} does not match {c} "
                                     "channels")
                l.update(fmt=fmt, chw=(c, h, w), kernel=(kh, kw))
                # the pixels times [C, (kh, kw, oc)]: the NHWC patch matrix of the output
                l["wm"] = l["w"].transpose(0, 2, 3, 1).reshape(c, -1)
                h, w = _out_hw_t(h, w, (kh, kw), l["strides"], l["pads"], l["dilations"],
                                 l.setdefault("output_padding", (0, 0)))
                if not all(0 <= o < s for o, s in zip(l["output_padding"], l["strides"])):
                    raise ValueError(f"ConvTranspose output_padding {l['output_padding']} is "
                                     f"not below the strides {l['strides']}")
                l["out_chw"] = (oc, h, w)
                c, fmt = oc, "NHWC"
            elif op == "resize":
                l.update(fmt=fmt, chw=(c, h, w))
                h, w = _resize_hw(h, w, l)
                l["out_hw"] = (h, w)
            elif op in ("maxpool", "avgpool"):
                l.update(fmt=fmt, chw=(c, h, w))
                h, w = _out_hw(h, w, l["kernel"], l["strides"], l.get("pads", (0, 0, 0, 0)),
                               (1, 1))
            elif op == "flatten":
                flat = (fmt, c, h, w)
            elif op == "unflatten":
                c, h, w = l["out_chw"]
                if flat is None or flat[0] is not None or self.n_outputs != c * h * w:
                    raise ValueError(f"unsupported ONNX graph: a Reshape to the image {(c, h, w)} "
                                     "has to follow a dense layer of as many outputs")
                fmt, flat = "NCHW", None
            elif op == "dense":
                if flat is None:
                    raise ValueError("unsupported ONNX graph: Gemm / MatMul before Flatten")
                wm = l["w"]
                if flat[0] is not None:
                    f, fc, fh, fw = flat
                    if wm.shape[0] != fc * fh * fw:
                        raise ValueError(f"dense weight {wm.shape} does not match the flattened "
                                         f"{(fc, fh, fw)} activation")
                    if f == "NHWC":
                        wm = hwc_rows(wm, fc, fh, fw)
                    flat = (None,) + flat[1:]
                l["wm"] = wm
                self.n_outputs = wm.shape[1]
            if min(h, w) <= 0:
                raise ValueError(f"layer {op} leaves an empty {h}x{w} image")

    def predict(self, x, fixedpoint_dtype=DEFAULT_FIXED_DTYPE):
        const = lambda v: self.fixedpoint_constant(v, plc=self.mirrored,  # noqa: E731
                                                   dtype=fixedpoint_dtype)
        for l in self.layers:
            op = l["op"]
            if op == "conv":
                c, h, w = l["chw"]
                shape = (None, c, h, w) if l["fmt"] == "NCHW" else (None, h, w, c)
                if l["group"] > 1:
                    # depthwise (group = C) is one operator; other groups compose.  The first
                    # convolution reads NCHW and answers NCHW: one permutation to NHWC
                    fn = pm.depthwise_conv2d if l["group"] == c else pm.conv2d
                    kw = {} if l["group"] == c else {"groups": l["group"]}
                    x = fn(x, const(l["w"]), const(l["b"]), l["strides"], l["pads"],
                           l["dilations"], l["fmt"], input_shape=shape,
                           weight_shape=l["w"].shape, **kw)
                    if l["fmt"] == "NCHW":
                        x = pm.permute(x, (0, 2, 3, 1))
                    continue
                cols = pm.im2col(x, l["kernel"], l["strides"], l["pads"], l["dilations"],
                                 l["fmt"], input_shape=shape)
                y = pm.add(pm.dot(cols, const(l["wm"])), const(l["b"]))
                oh, ow = _out_hw(h, w, l["kernel"], l["strides"], l["pads"], l["dilations"])
                x = pm.reshape(y, [-1, oh, ow, l["w"].shape[0]])
            elif op == "convtranspose":
                # pm.conv_transpose2d's composition on NHWC, the weight re-ordered at load: a
                # dot of the pixels, then the col2im sum into the output image
                if l["fmt"] == "NCHW":
                    x = pm.permute(x, (0, 2, 3, 1))
                cols = pm.dot(pm.reshape(x, [-1, l["chw"][0]]), const(l["wm"]))
                y = pm.col2im(cols, l["out_chw"], l["kernel"], l["strides"], l["pads"],
                              l["dilations"], "NHWC")
                x = pm.add(y, const(l["b"]))
            elif op == "resize":
                # in the activation's own layout: no permutation runs on shares
                c, h, w = l["chw"]
                shape = (None, c, h, w) if l["fmt"] == "NCHW" else (None, h, w, c)
                x = pm.resize2d(x, sizes=l.get("sizes"), scales=l.get("scales"), mode=l["mode"],
                                coordinate_transformation_mode=l["ctm"],
                                nearest_mode=l["nearest_mode"], data_format=l["fmt"],
                                weight_bits=l.get("weight_bits"), input_shape=shape)
            elif op in ("maxpool", "avgpool"):
                c, h, w = l["chw"]
                shape = (None, c, h, w) if l["fmt"] == "NCHW" else (None, h, w, c)
                if op == "maxpool":
                    x = pm.max_pool2d(x, l["kernel"], l["strides"], l["fmt"], input_shape=shape)
                else:
                    x = pm.avg_pool2d(x, l["kernel"], l["strides"], l["pads"], l["fmt"],
                                      input_shape=shape)
            elif op == "relu":
                x = pm.relu(x)
            elif op == "sigmoid":
                x = pm.sigmoid(x)
            elif op == "tanh":
                x = pm.tanh(x)
            elif op == "clip":
                x = pm.clip(x, l["lo"], l["hi"])
            elif op == "leakyrelu":
                x = pm.leaky_relu(x, l["alpha"])
            elif op == "hardsigmoid":
                x = pm.hard_sigmoid(x, l["alpha"], l["beta"])
            elif op == "hardswish":
                x = pm.hard_swish(x)
            elif op == "thresholdedrelu":
                x = pm.thresholded_relu(x, l["alpha"])
            elif op == "gelu":
                x = pm.gelu(x, approximate=l["approximate"])
            elif op in ("elu", "celu"):
                x = getattr(pm, op)(x, l["alpha"])
            elif op in ("silu", "mish", "softplus", "selu", "erf"):
                x = getattr(pm, op)(x)
            elif op == "unflatten":
                x = pm.reshape(x, [-1, *l["out_chw"]])
            elif op == "flatten":
                c, h, w = self._flat_size()
                x = pm.reshape(x, [-1, c * h * w])
            elif op == "dense":
                x = pm.add(pm.dot(x, const(l["wm"])), const(l["b"]))
            elif op == "softmax":
                x = pm.softmax(x, axis=1, upmost_index=self.n_outputs)
        return x

    def _flat_size(self):
        c, h, w = self.input_chw
        for l in self.layers:
            if l["op"] == "conv":
                h, w = _out_hw(h, w, l["kernel"], l["strides"], l["pads"], l["dilations"])
                c = l["w"].shape[0]
            elif l["op"] == "convtranspose":
                c, h, w = l["out_chw"]
            elif l["op"] == "resize":
                h, w = l["out_hw"]
            elif l["op"] in ("maxpool", "avgpool"):
                h, w = _out_hw(h, w, l["kernel"], l["strides"], l.get("pads", (0, 0, 0, 0)),
                               (1, 1))
            elif l["op"] == "flatten":
                break
        return c, h, w


def _out_hw(h, w, kernel, strides, pads, dilations):
    (kh, kw), (sh, sw), (pt, pl, pb, pr), (dh, dw) = kernel, strides, pads, dilations
    return ((h + pt + pb - dh * (kh - 1) - 1) // sh + 1,
            (w + pl + pr - dw * (kw - 1) - 1) // sw + 1)


def _resize_hw(h, w, l):
    """Spatial size of a resize layer's output: its sizes, or floor(I * scale) with the scale
    taken as its exact binary value (as pm.resize2d does)."""
    if l.get("sizes") is not None:
        oh, ow = (int(s) for s in l["sizes"])
    else:
        from fractions import Fraction

        oh, ow = (int(i * Fraction(s)) for i, s in zip((h, w), l["scales"]))
    if min(oh, ow) <= 0:
        raise ValueError(f"Resize leaves an empty {oh}x{ow} image")
    return oh, ow


def _out_hw_t(h, w, kernel, strides, pads, dilations, output_padding):
    """Spatial size of a ConvTranspose output."""
    (kh, kw), (sh, sw), (pt, pl, pb, pr), (dh, dw) = kernel, strides, pads, dilations
    return ((h - 1) * sh + dh * (kh - 1) + 1 - pt - pb + output_padding[0],
            (w - 1) * sw + dw * (kw - 1) + 1 - pl - pr + output_padding[1])
