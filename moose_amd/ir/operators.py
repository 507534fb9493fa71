"""Operator catalogue of the native IR.

Parity: reference ``moose/src/computation.rs:828-914`` -- the 81 operators and their
attribute fields (``:922-1547``).  Each entry maps an operator name to its ordered
attribute schema ``[(attr, kind)]`` where ``kind`` drives both the textual parser and
the printer:

* ``int`` / ``opt_int`` / ``ints`` (list) / ``bool`` / ``str`` / ``key`` (16 raw bytes
  printed as hex) / ``const`` (a :class:`Constant`) / ``slice``.

Operators listed in ``EXTENSION_OPERATORS`` are this framework's fused host kernels
(one HIP launch for a whole RSS local step); they only appear in lowered graphs
produced by our compiler and are documented in ``docs/ARCHITECTURE.md``.
"""

OPERATORS = {
    "Abs": [],
    "Add": [],
    "And": [],
    "AtLeast2D": [("to_column_vector", "bool")],
    "BitExtract": [("bit_idx", "int")],
    "Broadcast": [("shape", "opt_ints")],
    "Cast": [],
    "Concat": [("axis", "int")],
    "Constant": [("value", "const")],
    "Decrypt": [],
    "DeriveSeed": [("sync_key", "key")],
    "Div": [],
    "Diag": [],
    "Dot": [],
    "ExpandDims": [("axis", "ints")],
    "Identity": [],
    "IndexAxis": [("axis", "int"), ("index", "int")],
    "Inverse": [],
    "Input": [("arg_name", "str")],
    "Load": [],
    "Mul": [],
    "Mean": [("axis", "opt_int")],
    "Output": [("tag", "str")],
    "Ones": [],
    "Or": [],
    "PrfKeyGen": [],
    "Reshape": [("shape", "opt_ints")],
    "Receive": [("rendezvous_key", "key"), ("sender", "str")],
    "Relu": [],
    "RingFixedpointArgmax": [("axis", "int"), ("upmost_index", "int")],
    "RingFixedpointDecode": [("scaling_base", "int"), ("scaling_exp", "int")],
    "RingFixedpointEncode": [("scaling_base", "int"), ("scaling_exp", "int")],
    "RingInject": [("bit_idx", "int")],
    "RingFixedpointMean": [
        ("axis", "opt_int"),
        ("scaling_base", "int"),
        ("scaling_exp", "int"),
    ],
    "Sample": [("max_value", "opt_int")],
    "SampleSeeded": [("max_value", "opt_int")],
    "Select": [("axis", "int")],
    "Send": [("rendezvous_key", "key"), ("receiver", "str")],
    "Save": [],
    "Shape": [],
    "Shl": [("amount", "int")],
    "Shr": [("amount", "int")],
    "Sign": [],
    "Slice": [("slice", "slice")],
    "Sqrt": [],
    "Squeeze": [("axis", "opt_int")],
    "Sub": [],
    "Sum": [("axis", "opt_int")],
    "Transpose": [],
    "Xor": [],
    "Zeros": [],
    "Equal": [],
    "EqualZero": [],
    "Exp": [],
    "FixedpointEncode": [("fractional_precision", "int"), ("integral_precision", "int")],
    "FixedpointDecode": [("fractional_precision", "int")],
    "Greater": [],
    "Less": [],
    "Neg": [],
    "Pow2": [],
    "Sigmoid": [],
    "AdtToRep": [],
    "AddN": [],
    "Argmax": [("axis", "int"), ("upmost_index", "int")],
    "BitDecompose": [],
    "BitCompose": [],
    "Fill": [("value", "const")],
    "Index": [("index", "int")],
    "Log2": [],
    "Log": [],
    "Maximum": [],
    "Msb": [],
    "Mux": [],
    "RepToAdt": [],
    "Reveal": [],
    "Share": [],
    "Softmax": [("axis", "int"), ("upmost_index", "int")],
    "ShlDim": [("amount", "int"), ("bit_length", "int")],
    "TruncPr": [("amount", "int")],
    "Demirror": [],
    "Mirror": [],
}

# Fused host kernels introduced by this framework's lowering (MI355X-first: one
# kernel per RSS local step instead of several tiny host ops).
EXTENSION_OPERATORS = {
    # z = x0*y0 + x0*y1 + x1*y0  (RSS multiplication cross terms)
    "RingMulCross": [],
    # z = x0.(y0+y1) + x1.y0     (RSS matmul cross terms, one K-concatenated GEMM)
    "RingDotCross": [],
    # z = x0&y0 ^ x0&y1 ^ x1&y0  (RSS AND cross terms on packed bit words)
    "BitAndCross": [],
    # zero share alpha_i = PRF(k_i) - PRF(k_{i+1}) expanded from two seeds
    "ZeroShare": [("bits", "int")],
    # logical right shift of a packed boolean word tensor along the bit axis
    "ShrWord": [("amount", "int")],
    "ShlWord": [("amount", "int")],
    # host primitives of lowered graphs that the reference expresses with other ops
    "Sar": [("amount", "int")],                      # arithmetic right shift
    "AddConst": [("value", "const")],                # x + public ring constant
    "RingCast": [],                                  # ring width change (width = ret type)
    "FromBool": [],
    "ToBool": [],
    "RingToInt": [],
    "IntToRing": [],
    "BitSplit": [("start", "int"), ("count", "int")],  # packed word -> bit planes
    "WeightedSum": [("weights", "ints"), ("bits", "int")],
    "StridedSlice": [("slices", "ints")],
    "MulLeading": [],  # x[i, ...] * c[i]: rank-agnostic public scaling (polymorphic plans)
    # patch gather of a 2-D convolution: rank-4 NCHW / NHWC -> [N*OH*OW, C*KH*KW], rows
    # (n, oh, ow), columns (c, kh, kw) (NHWC: (kh, kw, c)); pads are (top, left, bottom,
    # right) and padded taps are zero.  Share-wise on replicated values (a convolution is
    # linear): the GEMM that follows is the ordinary fixed-point Dot
    "Im2Col": [("kernel_shape", "ints"), ("strides", "ints"), ("pads", "ints"),
               ("dilations", "ints"), ("data_format", "str")],
    # the exact adjoint of Im2Col, and the scatter-sum of a transposed convolution: a patch
    # matrix [N*OH*OW, C*KH*KW] in Im2Col's order -> the image [N, C, H, W] (NHWC: [N, H, W,
    # C]) of image_shape = (C, H, W), every pixel the sum of the entries whose tap lands on
    # it.  N comes from the rows.  Linear, so share-wise on replicated values
    "Col2Im": [("image_shape", "ints"), ("kernel_shape", "ints"), ("strides", "ints"),
               ("pads", "ints"), ("dilations", "ints"), ("data_format", "str")],
    # 2-D image resize with public coordinates (ONNX Resize: nearest / linear): a rank-4
    # NCHW / NHWC tensor -> spatial size sizes = (OH, OW), every output the exact integer-
    # weighted sum of its (up to) four taps, weights of weight_bits = (wbh, wbw) bits per
    # axis (moose_amd.ops.ring.resize_tables).  The leaf does not truncate: a fixed-point
    # linear result is truncated by wbh + wbw afterwards.  scales is empty (the scale is O/I)
    # or the two given scales as exact rationals [num_h, den_h, num_w, den_w].  Linear, so
    # share-wise on replicated values
    "Resize": [("sizes", "ints"), ("mode", "str"), ("coordinate_transformation_mode", "str"),
               ("nearest_mode", "str"), ("scales", "ints"), ("weight_bits", "ints"),
               ("data_format", "str")],
    # general axis permutation (Transpose reverses all axes); share-wise
    "Permute": [("axes", "ints")],
    # depthwise 2-D convolution of a rank-4 NCHW / NHWC x with the ONNX depthwise weight
    # w = [C*mult, 1, KH, KW]: out[n, oh, ow, c*mult + j] = sum_taps x[n, ., ., c] * w[c*mult
    # + j, 0, kh, kw], in the input's layout; pads as Im2Col.  A direct stencil kernel over
    # shares (no patch matrix): secret x secret is the replicated local product + dot tail
    "DepthwiseConv": [("strides", "ints"), ("pads", "ints"), ("dilations", "ints"),
                      ("data_format", "str")],
    # elementwise piecewise-linear function with public pieces: k sorted breakpoints and k + 1
    # slopes and intercepts, signed integers at the input dtype's fractional precision;
    # segment i is slopes[i] * x + intercepts[i] on [breakpoints[i-1], breakpoints[i]).  On a
    # secret x: one stacked sign extraction for the k flags, one local kernel, one truncation
    "PiecewiseLinear": [("breakpoints", "ints"), ("slopes", "ints"), ("intercepts", "ints")],
    # elementwise piecewise polynomial of degree 1..3 with public pieces: k sorted breakpoints
    # and (k + 1) x (degree + 1) coefficients, row-major, row j = (c_0, .., c_degree) of piece
    # j on [breakpoints[j-1], breakpoints[j]); signed integers at the input dtype's fractional
    # precision.  On a secret x: degree - 1 multiplications for the powers, one stacked sign
    # extraction for the k flags, one local kernel, one truncation
    "PiecewisePolynomial": [("breakpoints", "ints"), ("coefficients", "ints"),
                            ("degree", "int")],
    # sort along `axis` (ascending unless `descending`); by >= 0: the rows of a rank-2 tensor
    # reordered so that column `by` is sorted (equal keys in unspecified order).  On a secret
    # fixed-point x: a bitonic network of compare-exchange stages, each one sign extraction and
    # one multiplication, exact (nothing truncates)
    "Sort": [("axis", "int"), ("descending", "bool"), ("by", "int")],
    # oblivious shuffle along `axis` by a uniformly random permutation no single party knows.
    # On a secret x: three steps, one per PRF key; the key's two holders derive a permutation
    # and two masks from it, gather their share components through it and send one masked
    # tensor each to the third party.  Exact: the result is the input's values, reordered
    "Shuffle": [("axis", "int")],
    # the two host operators a lowered Shuffle step is made of: the permutation that stably
    # sorts a vector of 64-bit PRF output as unsigned integers, and the row gather through it
    # fused with the step's sums -- inputs (a, perm, then the optional operands `form` names:
    # b gathered and added, p added in place, m subtracted in place)
    "PermFromKeys": [],
    # prefix sums along `axis` (exclusive: of the elements before each one; reverse: from the
    # far end).  Linear: on a secret fixed-point x a local kernel on every share component
    "CumSum": [("axis", "int"), ("exclusive", "bool"), ("reverse", "bool")],
    # group the rows of a rank-2 table [n, c] by column `by` and sum the other columns per
    # key: [n, c + count + 1] in key order, the last row of each group holding (key, sums...,
    # the group's size if `count`, valid = 1), every other row zero; `shuffle` reorders the
    # rows obliviously at the end.  On a secret x: a sort, one sign extraction, a segmented
    # scan of ceil(log2 n) multiplications and one more multiplication, exact
    "GroupBySum": [("by", "int"), ("count", "bool"), ("shuffle", "bool")],
    # addressing by a secret index (a replicated uint64 tensor, as Argmax returns, or a
    # fixed-point tensor holding an integer; 0 <= idx < 2^ceil(log2 n), an idx past the last
    # entry selects nothing).  OneHot: [..., depth] rows of 0 / 1.0 in the result type.  Lookup:
    # inputs (table [n, d] or [n], idx), the rows table[idx].  BinCount: inputs (idx[, weights]),
    # the counts per bin [length] or the sums of the weights per bin [length, d].  On a secret
    # index: a demultiplexer of ceil(log2 ceil(log2 n)) multiplications, then one untruncated
    # ring GEMM; exact
    "OneHot": [("depth", "int")],
    "Lookup": [],
    "BinCount": [("length", "int")],
    "PermGather": [("axis", "int"), ("form", "str")],
}

ALL_OPERATORS = {**OPERATORS, **EXTENSION_OPERATORS}

# Deprecated operator names accepted by the parser (computation.rs:815-820).
OPERATOR_ALIASES = {
    "PrimDeriveSeed": "DeriveSeed",
    "PrimPrfKeyGen": "PrfKeyGen",
    "HostMean": "Mean",
    "FixedpointMeanOp": "Mean",
    "FloatingpointMeanOp": "Mean",
    "RepFixedpointMean": "Mean",
}

# Signature used when the textual form omits one (parsing.rs DeriveSeed).
DEFAULT_RETURN = {"DeriveSeed": "HostSeed", "PrfKeyGen": "HostPrfKey"}

assert len(OPERATORS) == 81, len(OPERATORS)
