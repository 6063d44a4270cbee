"""Per-unit fp64 reference of a fused net - a plain helper module for tests (tests/test_unit_reference_host.py on the CPU
stand-in, tests/test_gpu_unit_reference.py on the device).

What it is for.  The kernel-against-twin checks hand the twin the kernel's own arguments (codes, scales, `bn_scale`, `bn_shift`,
`act`, residual): they prove a launch computes what it was told, not that quantize/fuse.py and quantize/convert/* told it the
right thing.  Here every fused unit's stored output is compared with the reference's own composition of that unit,

    unit_act( act( BN( conv( fq(x), fq(w) ) + bias ) ) + shortcut )

evaluated in float64 on the CPU from the block's RAW parameters (the weight as it was before the first forward froze it, the four
BatchNorm vectors, eps, fix_gamma) and the unit's ACTUAL input tensor.  Which BatchNorm, activation and shortcut belong to a
convolution is read off the model definition (`describe`, before `fuse_inference` runs); no `_fq_*` attribute and no kernel
argument other than activation tensors is looked at.  The two fake-quantisers are oracle.fq_oracle's, whose fp32 semantics the
goldens pin bit for bit.

The gate.  With ref the float64 composition, ref32 the SAME composition in float32 torch on the CPU (what the reference does)
and m = max|ref| of the unit:

    e_fused = max|y - ref| / m        e_fp32 = max|ref32 - ref| / m        pass:  e_fused <= 4 * max(e_fp32, 2^-23)

A unit with m == 0 must be exactly zero.  The 3x3 layers of a Winograd-domain quantised net that run on three int8 digit slices
(16 in ResNet-50 F43) multiply m * p, not the reference's filter: measured the same way they sit at 4 - 11.5 times the yardstick on
the stand-in (e_fused 1.0e-6 - 2.4e-6: the documented 2^-20 max|g^_c| per weight, honest).  Their gate is the same, taken on what
exceeds the most that tolerance can move each output element by (`sliced_filter_allowance`).  That allowance is 3e-5 - 5e-5 of
m on ResNet-50; a folded shift that is 2 % off still puts such a layer at 160 - 8000 times the yardstick.  The factor 4 is margin over the spread of the reference path alone; it is not to be
raised - a unit that misses it is either a wrong layer or something to explain here.

Worst e_fused / max(e_fp32, 2^-23) per net on the CPU stand-in (oracle.patch.oracle_ops: the kernels' arithmetic), randomised
BatchNorm, batch 2, the sizes of tests/test_unit_reference_host.py; online | offline after one EMA step:

    net                 weights               units   online  offline
    mobilenet1.0        per-layer                28     1.42     1.12
    mobilenet1.0        per-channel              28     1.38     1.11
    mobilenet0.75       per-layer                27     1.49     1.20
    mobilenet0.75       per-channel              27     1.50     1.14
    mobilenet0.5        per-layer                27     1.24     1.30
    mobilenet0.5        per-channel              27     1.39     1.37
    mobilenet0.25       per-layer                27     1.19     1.13
    mobilenet0.25       per-channel              27     1.16     0.97
    mobilenetv2_1.0     per-layer                53     1.14     1.45
    mobilenetv2_1.0     per-channel              53     1.14     1.14
    mobilenetv2_0.75    per-layer                52     1.19     1.21
    mobilenetv2_0.75    per-channel              52     1.58     1.14
    mobilenetv2_0.5     per-layer                52     1.29     1.27
    mobilenetv2_0.5     per-channel              52     1.44     1.31
    mobilenetv2_0.25    per-layer                52     1.46     1.37
    mobilenetv2_0.25    per-channel              52     1.40     1.31
    resnet18_v1         per-layer                21     1.24     1.19
    resnet18_v1         per-channel              21     1.02     1.23
    resnet34_v1         per-layer                37     1.44     1.08
    resnet34_v1         per-channel              37     1.31     1.08
    resnet50_v1         per-layer                54     0.79     0.88
    resnet50_v1         per-channel              54     0.69     0.74
    cifar_resnet20_v1   per-layer                20     1.41     1.14
    cifar_resnet20_v1   per-channel              20     1.15     1.23
    vgg11_bn            per-layer                10     1.00     1.00
    vgg11_bn            per-channel              10     1.00     1.00
    mobilenet1.0        group-wise               28     1.70     1.10
    resnet50_v1         per-ch., last_gamma      54     1.18     0.77
    resnet50_v1         per-channel, F43         54     0.79     0.98   (the 16 sliced layers beyond their tolerance)

None exceeds 2 (the worst, 1.70, is a depthwise layer of mobilenet1.0: nine terms, so the yardstick itself is within a few ulp).
The ResNet-50 rows sit below 1: on wide layers the exact integer sums beat an fp32 convolution.  vgg11_bn's 1.00 is its two
Dense(4096, relu) layers, which stay with the tensor library - on the CPU the very GEMM the yardstick runs.

A recorder (`Recorder`) spies on `ops.*` - forward hooks would switch the special forms off - and `bind` attaches every launch
to its unit by forward order (one convolution event per quantised block, in the order the fused forward runs them: shortcut
branch first, then the body) and follows the unit's tensor through later passes by tensor identity.
"""
import numpy as np
import torch

from oracle import fq_oracle as O

GATE_FACTOR = 4.0
GATE_FLOOR = 2.0 ** -23

# launches that run a quantised block's convolution on the integer codes / quantise on load: (x, ...) -> (y, stat)
CONV_LAUNCHES = ("dwconv3x3", "pwconv_i8", "conv3x3_i8")
# the apply pass of a block whose convolution stays with the tensor library: (x, ...) -> (xq, cur, codes)
APPLY_LAUNCHES = ("fake_quant_online", "fake_quant_online_prestat", "fake_quant_offline")
# passes over a stored tensor: (x, ...) -> (y, stat)
POST_LAUNCHES = ("bn_act_stat", "add_act_stat", "global_avg_pool_stat", "bn_act_maxpool_stat")
STEM_LAUNCHES = ("stem_conv_s2",)
# the special forms (counted, never gated: their results are tied to the plain forms by bit-equality of the logits)
FORM_LAUNCHES = ("pwconv_i8_stat", "pwdw_fused", "pwconv_i8_shortcut", "pwconv_i8_gap", "dwconv3x3_c16")


# ---- nets ------------------------------------------------------------------------------------------------------------------------
def randomise_batchnorm(net, seed, keep_zero_gamma=False):
    """Every nn.BatchNorm of `net` gets the statistics of a trained checkpoint instead of the identity: running_var in [0.5, 2],
    running_mean and beta ~ 0.3 N(0, 1), gamma in [0.5, 1.5] with about a fifth of the channels negated and about one in twenty
    exactly 0.  `keep_zero_gamma`: a BatchNorm whose gamma is all zero (the zoo's `last_gamma=True`) keeps gamma = 0 and beta = 0.
    Written in place (the parameters' version counters move, so every cache of folded constants is refreshed).  Returns the count."""
    from quantization.mxnet_amd.mx.gluon import nn
    rng = np.random.default_rng(seed)
    found = []
    net.apply(lambda b: found.append(b) if type(b) is nn.BatchNorm else None)
    with torch.no_grad():
        for bn in found:
            g = bn.gamma.data()._t
            c = g.numel()
            var = rng.uniform(0.5, 2.0, c)
            mean = 0.3 * rng.standard_normal(c)
            beta = 0.3 * rng.standard_normal(c)
            gamma = rng.uniform(0.5, 1.5, c)
            u = rng.uniform(0.0, 1.0, c)
            gamma = np.where(u < 0.2, -gamma, gamma)
            gamma = np.where(u > 0.95, 0.0, gamma)
            if keep_zero_gamma and not bool((g != 0).any()):
                gamma, beta = np.zeros(c), np.zeros(c)
            for p, v in ((bn.gamma, gamma), (bn.beta, beta), (bn.running_mean, mean), (bn.running_var, var)):
                t = p.data()._t
                t.copy_(torch.from_numpy(v.astype(np.float32)).to(t.device))
    return len(found)


def build(model, classes, ctx=None, quant_type="layer", wt=8, in_w=8, wino="none", rand_bn=None, last_gamma=False):
    """A converted zoo net with the reference CLI's exclusions (the first convolution and its BatchNorm; MobileNetV2's classifier
    convolution; the CIFAR ResNets' first unit's first pair), as tests/test_gpu_net.py::_build has them."""
    from quantization.mxnet_amd.mx.gluon import nn
    from quantization.mxnet_amd.mx.gluon.model_zoo import get_model
    from quantization.mxnet_amd.quantize import convert
    from quantization.mxnet_amd.quantize.initialize import qparams_init
    np.random.seed(7)
    net = get_model(model, classes=classes, **(dict(last_gamma=True) if last_gamma else {}))
    convert_fn = {nn.Conv2D: convert.gen_conv2d_converter(quantize_input=True, wino_quantize=wino, weight_width=wt,
                                                          input_width=in_w, quant_type=quant_type),
                  nn.Dense: convert.gen_dense_converter(quantize_input=True, weight_width=wt, input_width=in_w,
                                                        quant_type=quant_type),
                  nn.Activation: None, nn.BatchNorm: None}
    exclude = [net.features[0], net.features[1]]
    if model.startswith("mobilenetv2_"):
        exclude.append(net.output[0])
    if model.startswith("cifar_resnet"):
        exclude.extend([net.features[2][0].body[0], net.features[2][0].body[1]])
    convert.convert_model(net, exclude=exclude, convert_fn=convert_fn)
    qparams_init(net)
    if ctx is not None:
        net.collect_params().reset_ctx(ctx)
    if rand_bn is not None:
        randomise_batchnorm(net, rand_bn, keep_zero_gamma=last_gamma)
    return net


# ---- the structural description -----------------------------------------------------------------------------------------------------
class Unit(object):
    """One convolution / Dense of the model definition with what follows it in its container.
    shortcut: None, ("input", i) - the input of unit i - or ("output", i) - the stored output of unit i."""

    def __init__(self, block, bn, act):
        self.block, self.bn, self.act = block, bn, act
        self.quantised = hasattr(block, "quantize_args")
        self.shortcut, self.unit_act = None, None
        self.raw_w = block.weight.data()._t.detach().cpu().numpy().copy()
        self.raw_b = None if block.bias is None else block.bias.data()._t.detach().cpu().numpy().copy()

    @property
    def is_dense(self):
        return not hasattr(self.block, "_kwargs")

    @property
    def name(self):
        return self.block.name


def _act_name(b):
    from quantization.mxnet_amd.mx.gluon import nn
    if type(b) is nn.Activation and b._act_type == "relu":
        return "relu"
    if type(b).__name__ == "RELU6":
        return "relu6"
    return None


def describe(net):
    """The units of `net` in the order the fused forward runs them (a residual unit's shortcut branch before its body), from the
    model definition alone.  Call it before the first forward: `fix_params` overwrites the weights with their fake-quantised
    values, and the reference quantises the raw ones."""
    from quantization.mxnet_amd.mx.gluon import nn
    from quantization.mxnet_amd.mx.gluon import model_zoo as zoo
    units = []

    def walk_seq(seq):
        kids = list(seq._children.values())
        first = len(units)
        for i, b in enumerate(kids):
            if type(b) in (nn.Conv2D, nn.Dense):
                bn = kids[i + 1] if i + 1 < len(kids) and type(kids[i + 1]) is nn.BatchNorm else None
                j = i + 1 + (bn is not None)
                act = _act_name(kids[j]) if j < len(kids) else None
                units.append(Unit(b, bn, act))
            else:
                walk(b)
        return first

    def walk(b):
        if isinstance(b, (zoo.BasicBlockV1, zoo.BottleneckV1)):
            ds = None
            if b.downsample is not None:
                ds = walk_seq(b.downsample)
                assert len(units) == ds + 1
            first = walk_seq(b.body)
            tail = units[-1]
            assert tail.act is None and tail.shortcut is None
            tail.shortcut = ("input", first) if ds is None else ("output", ds)
            tail.unit_act = "relu"
        elif isinstance(b, zoo.LinearBottleneck):
            first = walk_seq(b.out)
            if b.use_shortcut:
                tail = units[-1]
                assert tail.act is None
                tail.shortcut, tail.unit_act = ("input", first), None
        elif isinstance(b, (nn.Sequential, nn.HybridSequential)):
            walk_seq(b)
        elif type(b) in (nn.Conv2D, nn.Dense):
            units.append(Unit(b, None, None))
        else:
            for c in b._children.values():
                walk(c)
    walk(net)
    return units


# ---- the reference's composition of one unit -------------------------------------------------------------------------------------
def _act(t, kind):
    if kind == "relu":
        return torch.clamp(t, min=0)
    if kind == "relu6":
        return torch.clamp(t, min=0, max=6)
    assert kind in (None, "none"), kind
    return t


def _fq_weight(u):
    a = u.block.quantize_args
    if u.is_dense:
        return O.weight_fake_quant(u.raw_w, "channel" if a.quant_type == "channel" else "layer", a.wt_width)[0]
    k = u.block._kwargs
    if a.quant_type == "channel" and a.wino_quantize != "none" and tuple(k["kernel"]) == (3, 3):
        return O.wino_weight_fake_quant(u.raw_w, a.wino_quantize, a.wt_width)[0]
    return O.weight_fake_quant(u.raw_w, a.quant_type, a.wt_width, num_group=k["num_group"])[0]


def quantised_operands(u, x, offline):
    """(fq(x), fq(w)) as float32 numpy arrays and the batch statistic `current_input_max` the block should report: computed once
    per unit, shared by the float64 reference and its float32 yardstick."""
    x = np.ascontiguousarray(x.detach().cpu().numpy(), dtype=np.float32)
    if not u.quantised:
        return x, u.raw_w, None
    a = u.block.quantize_args
    thr = np.float32(u.block.input_max.data()._t.detach().cpu().numpy().reshape(-1)[0]) if offline else None
    if u.is_dense:
        xq, cur, _, _ = O.dense_input_fake_quant(x.reshape(x.shape[0], -1), a.in_signed, a.in_width, offline_threshold=thr)
    else:
        xq, cur, _, _ = O.conv_input_fake_quant(x, a.in_signed, a.in_width, offline_threshold=thr)
    return xq, _fq_weight(u), cur


def reference_unit(u, xq, wq, shortcut=None, dtype=torch.float64, conv_out=None):
    """act(BN(conv(xq, wq) + bias)) [+ shortcut, unit activation] in `dtype` on the CPU.  Convolution with the block's own
    `_kwargs`; BatchNorm by gluon's formula (x - mean) / sqrt(var + eps) * gamma + beta with `fix_gamma` honoured.
    `conv_out`: the stored output of the block's own forward (a tensor-library convolution) - the composition from there on."""
    if conv_out is not None:
        return _reference_tail(u, conv_out.detach().cpu().to(dtype), shortcut, dtype)
    x = torch.from_numpy(np.ascontiguousarray(xq)).to(dtype)
    w = torch.from_numpy(np.ascontiguousarray(wq)).to(dtype)
    b = None if u.raw_b is None else torch.from_numpy(u.raw_b).to(dtype)
    if u.is_dense:
        y = torch.nn.functional.linear(x.reshape(x.shape[0], -1), w, b)
    else:
        k = u.block._kwargs
        y = torch.nn.functional.conv2d(x, w, b, stride=tuple(k["stride"]), padding=tuple(k["pad"]),
                                       dilation=tuple(k["dilate"]), groups=k["num_group"])
    if u.block.act is not None:
        y = _act(y, _act_name(u.block.act))
    return _reference_tail(u, y, shortcut, dtype)


def _reference_tail(u, y, shortcut, dtype):
    if u.bn is not None:
        bn = u.bn
        gamma, beta, mean, var = (p.data()._t.detach().cpu().to(dtype) for p in (bn.gamma, bn.beta, bn.running_mean, bn.running_var))
        if bn._kwargs.get("fix_gamma", False):
            gamma = torch.ones_like(gamma)
        shape = (1, -1) + (1,) * (y.dim() - 2)
        eps = torch.tensor(bn._kwargs["eps"], dtype=dtype)
        y = (y - mean.reshape(shape)) / torch.sqrt(var + eps).reshape(shape) * gamma.reshape(shape) + beta.reshape(shape)
    y = _act(y, u.act)
    if u.shortcut is not None:
        y = _act(y + shortcut.detach().cpu().to(dtype).reshape(y.shape), u.unit_act)
    return y


# ---- the recorder ----------------------------------------------------------------------------------------------------------------
class Launch(object):
    __slots__ = ("name", "x", "b", "residual", "y", "stat", "subsample", "codes_out")


class Recorder(object):
    """`with Recorder() as rec: net(X)` - every producer launch of the forward with its activation tensors (references, not
    copies: the forward allocates its outputs afresh) and a copy of the per-sample statistic it returned."""

    def __init__(self):
        self.launches = []
        self._saved = {}

    def _spy(self, name, real):
        def spy(*a, **k):
            out = real(*a, **k)
            r = Launch()
            r.name, r.x = name, a[0]
            r.b = a[1] if name == "add_act_stat" else None
            r.residual = k.get("residual")
            r.subsample = bool(k.get("subsample"))
            r.codes_out = k.get("out_codes") is not None or k.get("side_codes") is not None
            many = isinstance(out, tuple)
            r.y = out[0] if many else out
            st = out[1] if many and len(out) > 1 and name not in APPLY_LAUNCHES else None
            r.stat = st.detach().clone() if torch.is_tensor(st) else None
            self.launches.append(r)
            return out
        return spy

    def __enter__(self):
        from quantization.mxnet_amd import ops
        for name in CONV_LAUNCHES + APPLY_LAUNCHES + POST_LAUNCHES + STEM_LAUNCHES + FORM_LAUNCHES:
            real = getattr(ops, name, None)
            if real is not None:
                self._saved[name] = real
                setattr(ops, name, self._spy(name, real))
        return self

    def __exit__(self, *exc):
        from quantization.mxnet_amd import ops
        for name, real in self._saved.items():
            setattr(ops, name, real)
        self._saved = {}
        return False

    def count(self, name=None, **flags):
        return sum(1 for r in self.launches if (name is None or r.name == name) and all(getattr(r, f) == v for f, v in flags.items()))


def _key(t):
    return (t.data_ptr(), t.numel()) if torch.is_tensor(t) else None


class Bound(object):
    __slots__ = ("unit", "x", "y", "launch", "shortcut", "post")


def bind(units, launches, net_out):
    """One convolution event per quantised block, in forward order: an integer launch, or the apply pass of a block whose
    convolution is the tensor library's.  The unit's stored output is the launch's own; behind a library convolution it is the
    next BatchNorm / activation pass (or, with neither, the tensor the next block is handed); a residual add in a pass of its own
    (`add_act_stat` of this very tensor) extends it.  Every quantised block is bound exactly once - asserted."""
    q = [u for u in units if u.quantised]
    ev = [i for i, r in enumerate(launches) if r.name in CONV_LAUNCHES + APPLY_LAUNCHES]
    assert len(ev) == len(q), "%d convolution events for %d quantised blocks" % (len(ev), len(q))
    bound = {}
    for n, (u, li) in enumerate(zip(q, ev)):
        lj = ev[n + 1] if n + 1 < len(ev) else len(launches)
        r, posts = launches[li], launches[li + 1:lj]
        assert torch.is_tensor(r.x) and r.x.dtype == torch.float32, "%s: %s was handed codes" % (u.name, r.name)
        cout, post = u.raw_w.shape[0], None
        cin = int(np.prod(u.raw_w.shape[1:])) if u.is_dense else u.raw_w.shape[1] * u.block._kwargs["num_group"]
        assert int(np.prod(r.x.shape[1:])) == cin if u.is_dense else r.x.shape[1] == cin, \
            "%s: bound to a %s launch with input %s" % (u.name, r.name, tuple(r.x.shape))
        if r.name in CONV_LAUNCHES:
            y = r.y
        elif u.bn is not None or u.act is not None:
            cand = [p for p in posts if p.name == "bn_act_stat" and p.x.shape[0] == r.x.shape[0] and p.x.shape[1] == cout]
            assert cand, "%s: no BatchNorm / activation pass behind its library convolution" % u.name
            y, post = cand[0].y, cand[0]
        else:
            y = launches[lj].x if lj < len(launches) else net_out
        assert torch.is_tensor(y) and y.shape[1] == cout, "%s: output %s" % (u.name, tuple(y.shape))
        if u.shortcut is not None:
            for p in posts:
                if p.name == "add_act_stat" and _key(p.x) == _key(y):
                    y = p.y
            # a sum no launch made (the zoo's own `out + x` of a linear bottleneck whose projection no residual-adding form takes):
            # nothing reads the stored tensor again, and the next block is handed another one of its shape
            read = any(_key(t) == _key(y) for p in launches[li + 1:] for t in (p.x, p.b, p.residual))
            if not read and lj < len(launches) and torch.is_tensor(launches[lj].x) and launches[lj].x.shape == y.shape:
                y = launches[lj].x
        b = Bound()
        b.unit, b.x, b.y, b.launch, b.shortcut, b.post = u, r.x, y, r, None, post
        bound[id(u)] = b
    stems = [r for r in launches if r.name in STEM_LAUNCHES]
    if stems:                            # the un-quantised first convolution, when it ran as this project's kernel
        assert len(stems) == 1 and not units[0].quantised
        b = Bound()
        b.unit, b.x, b.y, b.launch, b.shortcut, b.post = units[0], stems[0].x, stems[0].y, stems[0], None, None
        bound[id(units[0])] = b
    out = []
    for u in units:
        b = bound.get(id(u))
        if b is None:
            continue
        if u.shortcut is not None:
            other = bound.get(id(units[u.shortcut[1]]))
            if other is not None:
                b.shortcut = other.x if u.shortcut[0] == "input" else other.y
            else:
                # the unit opens with a convolution that was left un-quantised (the CIFAR ResNets' first unit under the CLI's
                # exclusions): no launch of this project saw the unit's input - the add's own second operand then
                adds = [p for p in launches if p.name == "add_act_stat" and _key(p.y) == _key(b.y)]
                assert len(adds) == 1 and u.shortcut[0] == "input", u.name
                b.shortcut = adds[0].b
        out.append(b)
    assert len([b for b in out if b.unit.quantised]) == len(q) == len({id(b.launch) for b in out if b.unit.quantised})
    return out


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def sliced_filter_allowance(u, xq, wq):
    """The one place where the fused path multiplies something other than the reference's operand: a Winograd-domain
    quantised 3x3 filter g^ on the integer path is three int8 digit slices m * p with |g^ - m * p| <= 2^-20 max|g^_c| per weight
    (asserted per layer in tests/test_gpu_net.py).  What that tolerance can move one output element by, at most:
    2^-20 max|g^_c| * sum |fq(x)| over the element's receptive field * |gamma_c / sqrt(var_c + eps)| - activation and shortcut add
    are 1-Lipschitz.  Returned as a float64 tensor of the output's shape; the gate of these layers is taken on what exceeds it."""
    k = u.block._kwargs
    x = torch.from_numpy(np.ascontiguousarray(xq)).to(torch.float64).abs().sum(dim=1, keepdim=True)
    s = torch.nn.functional.conv2d(x, torch.ones(1, 1, 3, 3, dtype=torch.float64), stride=tuple(k["stride"]), padding=tuple(k["pad"]))
    wmax = torch.from_numpy(np.abs(wq).reshape(wq.shape[0], -1).max(axis=1).astype(np.float64))
    if u.bn is not None:
        g, var = u.bn.gamma.data()._t.detach().cpu().double(), u.bn.running_var.data()._t.detach().cpu().double()
        if u.bn._kwargs.get("fix_gamma", False):
            g = torch.ones_like(g)
        wmax = wmax * (g / torch.sqrt(var + u.bn._kwargs["eps"])).abs()
    return 2.0 ** -20 * wmax.reshape(1, -1, 1, 1) * s


def is_sliced(u, launch):
    """A Winograd-domain quantised 3x3 convolution (the converter's settings) that ran as an integer launch."""
    a = getattr(u.block, "quantize_args", None)
    return (a is not None and not u.is_dense and a.quant_type == "channel" and a.wino_quantize != "none"
            and tuple(u.block._kwargs["kernel"]) == (3, 3) and launch.name == "conv3x3_i8")


def gate(y, ref, ref32, allowance=None):
    """(e_fused, e_fp32, m) of one unit; raises nothing.  `allowance`: per element, subtracted from |y - ref| (floored at 0)."""
    d = (y.detach().cpu().to(torch.float64).reshape(ref.shape) - ref).abs()
    if allowance is not None:
        d = torch.clamp(d - allowance.reshape(ref.shape), min=0)
    d = float(d.max())
    ref = ref.reshape(-1)
    m = float(ref.abs().max())
    d32 = float((ref32.to(torch.float64).reshape(-1) - ref).abs().max())
    if m == 0.0:
        return d, d32, m
    return d / m, d32 / m, m


def check_units(bound, offline, report=None, last_gamma=False, library="unit"):
    """The gate on every bound unit, and `current_input_max` of every quantised block against the statistic of the unit's actual
    input.  Returns the worst ratio e_fused / max(e_fp32, 2^-23); `report` (a list) receives one line per unit.
    `library`: what is gated of a unit whose convolution stayed with the tensor library.  "unit" - all of it, as everywhere else
    (the CPU tests: the library is then torch's CPU convolution, the yardstick's own).  "launch" - this project's launch alone:
    the BatchNorm / activation pass (and the add behind it) from the library convolution's stored output on.  The device library
    accumulates its long dot products in an order of its own - ResNet-34's 256 -> 512 stride-2 3x3 (2304 terms) measured 4.6 times
    the CPU yardstick, ResNet-18's 3.0 - which is no property of this project's code; that the library is handed fq(x) and fq(w) is
    pinned bit for bit by tests/test_gpu_net.py."""
    worst, failures = 0.0, []
    for b in bound:
        u = b.unit
        xq, wq, cur = quantised_operands(u, b.x, offline)
        conv_out = b.post.x if (library == "launch" and b.launch.name in APPLY_LAUNCHES and b.post is not None) else None
        ref = reference_unit(u, xq, wq, b.shortcut, torch.float64, conv_out)
        ref32 = reference_unit(u, xq, wq, b.shortcut, torch.float32, conv_out)
        sliced = is_sliced(u, b.launch)
        e, e32, m = gate(b.y, ref, ref32, sliced_filter_allowance(u, xq, wq) if sliced else None)
        if m == 0.0:
            ok, ratio = (e == 0.0 and e32 == 0.0), 0.0
        else:
            ratio = e / max(e32, GATE_FLOOR)
            ok = e <= GATE_FACTOR * max(e32, GATE_FLOOR)
        worst = max(worst, ratio)
        line = "%-40s %-25s e_fused %.3e  e_fp32 %.3e  ratio %7.2f  max|ref| %.3e%s" % (
            u.name, b.launch.name if conv_out is None else "library + bn_act_stat", e, e32, ratio, m,
            "  (beyond the three-slice tolerance)" if sliced else "")
        if report is not None:
            report.append(line)
        if not ok:
            failures.append(line)
        if last_gamma and u.shortcut is not None:
            want = torch.clamp(b.shortcut.detach().cpu().to(torch.float64), min=0).reshape(ref.shape)
            assert torch.equal(ref, want), "%s: a unit closed by a zero gamma is relu(shortcut)" % u.name
        if cur is not None:
            got = np.float32(float(u.block.current_input_max))
            assert got == cur, "%s: current_input_max %r, statistic of its input %r" % (u.name, got, cur)
    assert not failures, "units outside 4 * max(e_fp32, 2^-23):\n" + "\n".join(failures)
    return worst


def check_statistics(launches):
    """Each launch's per-sample statistic is `absmax_per_sample` of the tensor it stored, bit for bit."""
    n = 0
    for r in launches:
        if r.stat is None or r.subsample or not torch.is_tensor(r.y) or r.y.dtype != torch.float32:
            continue
        want = r.y.detach().abs().reshape(r.y.shape[0], -1).amax(dim=1)
        assert torch.equal(r.stat.reshape(-1)[:want.numel()], want), "%s: statistic of %s" % (r.name, tuple(r.y.shape))
        n += 1
    return n

