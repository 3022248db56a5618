"""Our own torch restatement of pose_resnet (the SimpleBaseline network), written from its description: ResNet-18/34/50/101/152
trunk (conv 7x7 s2 + BN + ReLU + max-pool 3x3 s2 p1; BasicBlocks, or Bottlenecks with the stride on the 3x3; the first block of
layer2..layer4 is stride 2 with a Conv2d 1x1 stride 2 + BN `downsample` on the residual, as is layer1.0 of the Bottleneck nets at
stride 1), NUM_DECONV_LAYERS x (ConvTranspose2d stride 2 [+ bias] + BN + ReLU) with (padding, output_padding) = (1, 0), (1, 1),
(0, 0) for kernels 4, 3, 2, and a final 1x1 / 3x3 Conv2d with bias.

spec(cfg)                       the ordered (key, shape) list of the module's state_dict
forward(sd, cfg, x)             plain float arithmetic in x's dtype (float32 or float64), eval-mode BatchNorm (eps 1e-5)
forward(sd, cfg, x, emulate=d)  the engine's number model: BN folded into the weights in float64 and cast to float32, weights and
                                every stored activation rounded to the 16-bit type d ("bf16" / "f16"), sums in float64, heat-maps f32
taps={}                         filled with every named intermediate (the engine's tap names)
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

SPEC = {18: (False, (2, 2, 2, 2)), 34: (False, (3, 4, 6, 3)), 50: (True, (3, 4, 6, 3)), 101: (True, (3, 4, 23, 3)),
        152: (True, (3, 8, 36, 3))}
DECONV = {4: (1, 0), 3: (1, 1), 2: (0, 0)}
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
EPS = 1e-5


def _extra(cfg):
    e = cfg["MODEL"]["EXTRA"]
    n = int(e["NUM_DECONV_LAYERS"])
    return (int(e["NUM_LAYERS"]), bool(e["DECONV_WITH_BIAS"]), [int(f) for f in e["NUM_DECONV_FILTERS"]][:n],
            [int(k) for k in e["NUM_DECONV_KERNELS"]][:n], int(e["FINAL_CONV_KERNEL"]), int(cfg["MODEL"]["NUM_JOINTS"]))


def blocks(cfg):
    """[(prefix, bottleneck, cin, planes, stride, has_downsample)] of layer1..layer4, and the trunk's output channels."""
    bneck, counts = SPEC[_extra(cfg)[0]]
    exp, inpl, out = (4 if bneck else 1), 64, []
    for li, nb in enumerate(counts):
        planes = 64 << li
        for b in range(nb):
            s = 2 if (li > 0 and b == 0) else 1
            out.append(("layer%d.%d" % (li + 1, b), bneck, inpl, planes, s, b == 0 and (s != 1 or inpl != planes * exp)))
            inpl = planes * exp
    return out, inpl


def spec(cfg):
    layers, with_bias, filters, kernels, fk, joints = _extra(cfg)
    keys = []

    def bn(p, c):
        keys.extend([(p + ".weight", (c,)), (p + ".bias", (c,)), (p + ".running_mean", (c,)), (p + ".running_var", (c,)),
                     (p + ".num_batches_tracked", ())])
    keys.append(("conv1.weight", (64, 3, 7, 7))); bn("bn1", 64)
    blks, c = blocks(cfg)
    for p, bneck, cin, planes, s, ds in blks:
        if bneck:
            keys.append((p + ".conv1.weight", (planes, cin, 1, 1))); bn(p + ".bn1", planes)
            keys.append((p + ".conv2.weight", (planes, planes, 3, 3))); bn(p + ".bn2", planes)
            keys.append((p + ".conv3.weight", (4 * planes, planes, 1, 1))); bn(p + ".bn3", 4 * planes)
        else:
            keys.append((p + ".conv1.weight", (planes, cin, 3, 3))); bn(p + ".bn1", planes)
            keys.append((p + ".conv2.weight", (planes, planes, 3, 3))); bn(p + ".bn2", planes)
        if ds:
            co = planes * (4 if bneck else 1)
            keys.append((p + ".downsample.0.weight", (co, cin, 1, 1))); bn(p + ".downsample.1", co)
    for i, (f, k) in enumerate(zip(filters, kernels)):
        keys.append(("deconv_layers.%d.weight" % (3 * i), (c, f, k, k)))
        if with_bias:
            keys.append(("deconv_layers.%d.bias" % (3 * i), (f,)))
        bn("deconv_layers.%d" % (3 * i + 1), f)
        c = f
    keys.append(("final_layer.weight", (joints, c, fk, fk))); keys.append(("final_layer.bias", (joints,)))
    return keys


class _Net:
    def __init__(self, sd, x, emulate, cache=None):
        self.sd, self.emu, self.cache = sd, emulate, cache
        self.dt = torch.float64 if emulate else x.dtype

    def q(self, t):   # round to the 16-bit grid (emulation only)
        return t.to(DT[self.emu]).to(torch.float64) if self.emu else t

    def fold(self, conv, bn, transposed=False, bias=False):
        if self.cache is not None:       # folded weights kept between calls (timing runs): fold once, like an exported model
            if conv not in self.cache:
                self.cache[conv] = self._fold(conv, bn, transposed, bias)
            return self.cache[conv]
        return self._fold(conv, bn, transposed, bias)

    def _fold(self, conv, bn, transposed, bias):
        w = self.sd[conv + ".weight"].double()
        b = self.sd[conv + ".bias"].double() if bias else torch.zeros(w.shape[1 if transposed else 0], dtype=torch.float64, device=w.device)
        if bn:
            s = self.sd[bn + ".weight"].double() / torch.sqrt(self.sd[bn + ".running_var"].double() + EPS)
            w = w * (s.view(1, -1, 1, 1) if transposed else s.view(-1, 1, 1, 1))
            b = b * s + self.sd[bn + ".bias"].double() - self.sd[bn + ".running_mean"].double() * s
        w, b = w.float(), b.float()           # the engine keeps folded weights and biases in float32
        return (self.q(w.double()) if self.emu else w.to(self.dt)), b.to(self.dt)

    def conv(self, x, conv, bn, stride=1, relu=False, res=None, bias=False, store=True):
        w, b = self.fold(conv, bn, bias=bias)
        y = F.conv2d(x, w, b, stride, (w.shape[-1] - 1) // 2)
        if res is not None:
            y = y + res
        if relu:
            y = torch.relu(y)
        return self.q(y) if store else y

    def deconv(self, x, conv, bn, k, bias):
        w, b = self.fold(conv, bn, transposed=True, bias=bias)
        pad, opad = DECONV[k]
        return self.q(torch.relu(F.conv_transpose2d(x, w, b, 2, pad, opad)))


def forward(sd, cfg, x, emulate=None, taps=None, cache=None):
    layers, with_bias, filters, kernels, fk, joints = _extra(cfg)
    net = _Net(sd, x, emulate, cache)
    taps = {} if taps is None else taps
    x = net.q(x.double()) if emulate else x
    y = net.conv(x, "conv1", "bn1", 2, relu=True)
    y = taps["maxpool"] = F.max_pool2d(y, 3, 2, 1)
    for p, bneck, cin, planes, s, ds in blocks(cfg)[0]:
        res = y
        if ds:
            res = taps[p + ".downsample"] = net.conv(y, p + ".downsample.0", p + ".downsample.1", s)
        if bneck:
            t = taps[p + ".conv1"] = net.conv(y, p + ".conv1", p + ".bn1", 1, relu=True)
            t = taps[p + ".conv2"] = net.conv(t, p + ".conv2", p + ".bn2", s, relu=True)
            y = net.conv(t, p + ".conv3", p + ".bn3", 1, relu=True, res=res)
        else:
            t = taps[p + ".conv1"] = net.conv(y, p + ".conv1", p + ".bn1", s, relu=True)
            y = net.conv(t, p + ".conv2", p + ".bn2", 1, relu=True, res=res)
        taps[p] = y
    for i, k in enumerate(kernels):
        y = taps["deconv_layers.%d" % (3 * i)] = net.deconv(y, "deconv_layers.%d" % (3 * i), "deconv_layers.%d" % (3 * i + 1), k, with_bias)
    y = net.conv(y, "final_layer", "", 1, bias=True, store=False)
    return y.float() if emulate else y


def walk(cfg):
    """The engine's ops in order, name -> {"kind", "inputs", "stages", "out_f32"} in the stage format of oracle/hrnet_ref.run_op
    (("conv", source, conv, bn, stride, relu, residual, store)), for the teacher-forced per-op check.  Names are the engine's tap
    names; "heatmaps" is the final layer.  Kinds the oracle does not know: "resnet_stem" (its one conv stage is followed by the
    max-pool) and "deconv" (extra keys "conv", "bn", "k", "bias").  layer1 of the Bottleneck nets is one fused launch per block:
    a composite op whose downsample residual (block 0) is never rounded."""
    layers, with_bias, filters, kernels, fk, joints = _extra(cfg)
    ops = OrderedDict()
    IN0, IN1 = ("in", 0), ("in", 1)

    def conv(src, c, bn, stride=1, relu=True, res=None, store=True):
        return ("conv", src, c, bn, stride, relu, res, store)

    def add(name, kind, inputs, stages, out_f32=False, **kw):
        ops[name] = dict({"kind": kind, "inputs": list(inputs), "stages": stages, "out_f32": out_f32}, **kw)
        return name
    x = add("maxpool", "resnet_stem", ["input"], [conv(IN0, "conv1", "bn1", 2)])
    for p, bneck, cin, planes, s, ds in blocks(cfg)[0]:
        if bneck and p.startswith("layer1."):
            res = [conv(IN0, p + ".downsample.0", p + ".downsample.1", relu=False, store=False)] if ds else []
            o = len(res)
            x = add(p, "bottleneck", [x], res + [conv(IN0, p + ".conv1", p + ".bn1"), conv(("st", o), p + ".conv2", p + ".bn2"),
                                                 conv(("st", o + 1), p + ".conv3", p + ".bn3", res=("st", 0) if ds else IN0)])
            continue
        r = x
        if ds:
            r = add(p + ".downsample", "downsample", [x], [conv(IN0, p + ".downsample.0", p + ".downsample.1", s, relu=False)])
        if bneck:
            y = add(p + ".conv1", "bneck_conv1", [x], [conv(IN0, p + ".conv1", p + ".bn1")])
            y = add(p + ".conv2", "bneck_conv2", [y], [conv(IN0, p + ".conv2", p + ".bn2", s)])
            x = add(p, "bneck_conv3", [y, r], [conv(IN0, p + ".conv3", p + ".bn3", res=IN1)])
        else:
            y = add(p + ".conv1", "block_conv1", [x], [conv(IN0, p + ".conv1", p + ".bn1", s)])
            x = add(p, "block_conv2", [y, r], [conv(IN0, p + ".conv2", p + ".bn2", res=IN1)])
    for i, k in enumerate(kernels):
        n = "deconv_layers.%d" % (3 * i)
        x = add(n, "deconv", [x], [], conv=n, bn="deconv_layers.%d" % (3 * i + 1), k=k, bias=with_bias)
    add("heatmaps", "final_layer", [x], [conv(IN0, "final_layer", None, relu=False, store=False)], out_f32=True)
    return ops


def run_deconv(sd, op, x, emulate):
    """A "deconv" op of walk() on the 16-bit input x: (float64 result rounded once, allowance E of an fp32 accumulation).
    Each output element sums at most 2 x 2 taps of every input channel: K = 4 Cin + 2."""
    net = _Net(sd, x, emulate)
    w, b = net.fold(op["conv"], op["bn"], transposed=True, bias=op["bias"])
    pad, opad = DECONV[op["k"]]
    x = x.double()
    v = torch.relu(F.conv_transpose2d(x, w, b, 2, pad, opad))
    S = F.conv_transpose2d(x.abs(), w.abs(), b.abs(), 2, pad, opad)
    return net.q(v), (4 * w.shape[0] + 2) * 2.0 ** -24 * S
