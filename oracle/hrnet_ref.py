"""fp32 CPU restatement of the reference pose_hrnet forward (TEST ORACLE, not product).

Follows /root/reference/landmark_regression/lib/models/pose_hrnet.py:
  * stem + layer1 ................. :425-432, Bottleneck :78-98, _make_layer :374-391
  * transition layers ............. :333-372, use in forward :434-455
  * HighResolutionModule .......... branches :139-185, fuse layers :187-242, forward :247-265
  * stages ........................ _make_stage :393-423 (last stage-4 module fuses to branch 0 only)
  * final 1x1 (or 3x3) conv + bias  :323-329, :458
and, for MODEL.NAME hrnet_cms / hrnet_cms_384 (lib/models/hrnet_cms.py, hrnet_cms_384.py):
  * stage 4 keeps all four outputs  hrnet_cms.py:321-322 (multi_scale_output=True)
  * four heads ConvTranspose2d(C_b -> 32, k5 s4 p1 op1 | k3 s2 p1 op1) + Conv2d(32 -> J)   :353-419
  * top-down pyramid: x_b = head_b(y_b) + bilinear_x2(x_{b+1}), eval returns x_0             :551-562

The network is evaluated functionally from a plain ``state_dict`` whose keys and
shapes are those of the reference module (``state_dict_spec``), so checkpoints
interchange.  No nn.Module tree of the reference is reproduced here.

``emulate`` selects the arithmetic model:
  None   -- the reference's own arithmetic: fp32 conv, eval BatchNorm, ReLU, adds.
  'bf16' / 'f16' -- the storage model of the HIP path: BatchNorm folded into the
           conv weight/bias, folded weights rounded to the 16-bit type, every
           tensor that the HIP path writes to HBM rounded to it, fp32 accumulation.
           Used to separate "logic differs" from "precision differs" in the tests.

walk() / run_op() restate the same forward op by op, one entry per tensor the HIP path writes (named as
scpose_hrnet_forward_tap offers it), for teacher-forced per-op parity: run_op evaluates one op on given inputs in the
storage model above (bit-identical to forward()'s taps, tests/test_op_bound.py) or in float64 with one rounding per
storage point, together with the arithmetic error allowance tests/op_bound.py checks against.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
EXPANSION = {"BASIC": 1, "BOTTLENECK": 4}


# ----------------------------------------------------------------------------- cfg
def extra_of(cfg):
    return cfg["MODEL"]["EXTRA"]


def w32_cfg(num_joints=11, image=256):
    return _wN_cfg(32, num_joints, image)


def w48_cfg(num_joints=11, image=384):
    return _wN_cfg(48, num_joints, image)


HEADS = {"pose_hrnet": None, "hrnet_cms": ("equal_to_image", 5, 4), "hrnet_cms_384": ("4x", 3, 2)}


def head_of(cfg):
    """None for pose_hrnet, else (key suffix, kernel, stride) of the four transposed-conv heads."""
    return HEADS[cfg["MODEL"].get("NAME", "pose_hrnet")]


def head_names(cfg):
    suffix = head_of(cfg)[0]
    return ["final_layer%s_%s" % ("" if b == 0 else str(b + 1), suffix) for b in range(4)]


def with_model(cfg, name):
    """Copy of cfg for another member of the family (pose_hrnet / hrnet_cms / hrnet_cms_384)."""
    out = {"MODEL": dict(cfg["MODEL"])}
    out["MODEL"]["NAME"] = name
    up = {None: 1}.get(head_of(out), None) or head_of(out)[2]
    img = out["MODEL"]["IMAGE_SIZE"][0]
    out["MODEL"]["HEATMAP_SIZE"] = [img // 4 * up, img // 4 * up]
    return out


def _wN_cfg(c, num_joints, image, modules=(1, 4, 3), block="BASIC", blocks=4):
    def stage(nb, nm):
        return {"NUM_MODULES": nm, "NUM_BRANCHES": nb, "BLOCK": block,
                "NUM_BLOCKS": [blocks] * nb, "NUM_CHANNELS": [c * (2 ** i) for i in range(nb)],
                "FUSE_METHOD": "SUM"}
    return {"MODEL": {"NAME": "pose_hrnet", "NUM_JOINTS": num_joints, "INIT_WEIGHTS": False,
                      "PRETRAINED": "", "IMAGE_SIZE": [image, image],
                      "HEATMAP_SIZE": [image // 4, image // 4],
                      "EXTRA": {"PRETRAINED_LAYERS": ["*"], "FINAL_CONV_KERNEL": 1,
                                "STAGE2": stage(2, modules[0]), "STAGE3": stage(3, modules[1]),
                                "STAGE4": stage(4, modules[2])}}}


def tiny_cfg(num_joints=11, image=64, c=16, modules=(1, 1, 1)):
    """Small HRNet of the same topology (for fast CPU tests)."""
    return _wN_cfg(c, num_joints, image, modules)


def bneck_cfg(num_joints=11, image=64, c=16, modules=(1, 1, 1), blocks=2):
    """STAGEk.BLOCK = BOTTLENECK (blocks_dict, pose_hrnet.py:266-269): branch b carries 4 * c * 2^b channels.  No shipped YAML
    uses it; the reference module builds and runs it (tests/golden/hrnet_bneck_reference_outputs.npz)."""
    return _wN_cfg(c, num_joints, image, modules, block="BOTTLENECK", blocks=blocks)


# ----------------------------------------------------------------------------- key/shape census
def _conv(sd, name, cout, cin, k, bias=False):
    sd[name + ".weight"] = (cout, cin, k, k)
    if bias:
        sd[name + ".bias"] = (cout,)


def _bn(sd, name, c):
    sd[name + ".weight"] = (c,)
    sd[name + ".bias"] = (c,)
    sd[name + ".running_mean"] = (c,)
    sd[name + ".running_var"] = (c,)
    sd[name + ".num_batches_tracked"] = ()


def _stage_channels(scfg):
    e = EXPANSION[scfg["BLOCK"]]
    return [c * e for c in scfg["NUM_CHANNELS"]]


def state_dict_spec(cfg):
    """name -> shape, in the reference module's registration order."""
    ex = extra_of(cfg)
    sd = OrderedDict()
    _conv(sd, "conv1", 64, 3, 3); _bn(sd, "bn1", 64)
    _conv(sd, "conv2", 64, 64, 3); _bn(sd, "bn2", 64)
    inpl = 64
    for b in range(4):                               # layer1: Bottleneck(planes 64) x4
        p = "layer1.%d" % b
        _conv(sd, p + ".conv1", 64, inpl, 1); _bn(sd, p + ".bn1", 64)
        _conv(sd, p + ".conv2", 64, 64, 3); _bn(sd, p + ".bn2", 64)
        _conv(sd, p + ".conv3", 256, 64, 1); _bn(sd, p + ".bn3", 256)
        if b == 0:
            _conv(sd, p + ".downsample.0", 256, inpl, 1); _bn(sd, p + ".downsample.1", 256)
        inpl = 256
    pre = [256]
    for si, sname in enumerate(("STAGE2", "STAGE3", "STAGE4")):
        scfg = ex[sname]
        cur = _stage_channels(scfg)
        tname = "transition%d" % (si + 1)
        for i in range(len(cur)):
            if i < len(pre):
                if cur[i] != pre[i]:
                    _conv(sd, "%s.%d.0" % (tname, i), cur[i], pre[i], 3); _bn(sd, "%s.%d.1" % (tname, i), cur[i])
            else:
                for j in range(i + 1 - len(pre)):
                    cin = pre[-1]
                    cout = cur[i] if j == i - len(pre) else cin
                    _conv(sd, "%s.%d.%d.0" % (tname, i, j), cout, cin, 3); _bn(sd, "%s.%d.%d.1" % (tname, i, j), cout)
        nb = scfg["NUM_BRANCHES"]
        last_stage = sname == "STAGE4"
        stname = "stage%d" % (si + 2)
        for m in range(scfg["NUM_MODULES"]):
            multi = head_of(cfg) is not None or not (last_stage and m == scfg["NUM_MODULES"] - 1)
            mp = "%s.%d" % (stname, m)
            for b in range(nb):
                for k in range(scfg["NUM_BLOCKS"][b]):
                    p = "%s.branches.%d.%d" % (mp, b, k)
                    if scfg["BLOCK"] == "BOTTLENECK":      # pose_hrnet.py:60-98, :142-154: in = out = 4 * planes, no downsample
                        pl = scfg["NUM_CHANNELS"][b]
                        _conv(sd, p + ".conv1", pl, cur[b], 1); _bn(sd, p + ".bn1", pl)
                        _conv(sd, p + ".conv2", pl, pl, 3); _bn(sd, p + ".bn2", pl)
                        _conv(sd, p + ".conv3", cur[b], pl, 1); _bn(sd, p + ".bn3", cur[b])
                        continue
                    _conv(sd, p + ".conv1", cur[b], cur[b], 3); _bn(sd, p + ".bn1", cur[b])
                    _conv(sd, p + ".conv2", cur[b], cur[b], 3); _bn(sd, p + ".bn2", cur[b])
            for i in range(nb if multi else 1):
                for j in range(nb):
                    fp = "%s.fuse_layers.%d.%d" % (mp, i, j)
                    if j > i:
                        _conv(sd, fp + ".0", cur[i], cur[j], 1); _bn(sd, fp + ".1", cur[i])
                    elif j < i:
                        for k in range(i - j):
                            cout = cur[i] if k == i - j - 1 else cur[j]
                            _conv(sd, "%s.%d.0" % (fp, k), cout, cur[j], 3); _bn(sd, "%s.%d.1" % (fp, k), cout)
        pre = cur
    fk = ex["FINAL_CONV_KERNEL"]
    if head_of(cfg) is None:
        _conv(sd, "final_layer", cfg["MODEL"]["NUM_JOINTS"], pre[0], fk, bias=True)
    else:
        _, k, _ = head_of(cfg)
        for b, name in enumerate(head_names(cfg)):
            sd[name + ".0.weight"] = (pre[b], 32, k, k)          # ConvTranspose2d: (in, out, k, k)
            sd[name + ".0.bias"] = (32,)
            _conv(sd, name + ".1", cfg["MODEL"]["NUM_JOINTS"], 32, fk, bias=True)
    return sd


def make_state_dict(cfg, seed=0):
    """Seeded synthetic checkpoint (SURVEY.md 8d recipe): kaiming-uniform(a=sqrt 5) convs,
    BN gamma~U[.75,1.25], beta,mean~N(0,.1^2), var~U[.75,1.25].  Deterministic for a torch build."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for name, shape in state_dict_spec(cfg).items():
        leaf = name.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            sd[name] = torch.tensor(0, dtype=torch.long)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            bound = (1.0 / fan_in) ** 0.5                    # kaiming_uniform(a=sqrt(5)) == U(+-1/sqrt(fan_in))
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif name.startswith("final_layer") and leaf == "bias":
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * 0.05
        elif leaf in ("weight", "running_var"):
            sd[name] = 0.75 + 0.5 * torch.rand(shape, generator=g)
        else:                                                # bn bias / running_mean
            sd[name] = 0.1 * torch.randn(shape, generator=g)
    return sd


# ----------------------------------------------------------------------------- arithmetic models
class _Arith:
    """conv(+bn)(+residual)(+relu) under one of the two arithmetic models."""

    def __init__(self, sd, emulate=None):
        self.sd = sd
        self.emulate = emulate
        self.dt = {None: None, "bf16": torch.bfloat16, "f16": torch.float16}[emulate]

    def rnd(self, t):
        return t if self.dt is None else t.to(self.dt).to(torch.float32)

    def conv_bn(self, x, conv, bn, stride=1, relu=False, residual=None, bias=None, store=True, round_w=True):
        sd = self.sd
        w = sd[conv + ".weight"].float()
        pad = (w.shape[-1] - 1) // 2
        if self.dt is None:
            y = F.conv2d(x, w, sd.get(conv + ".bias") if bias is None else bias, stride, pad)
            if bn is not None:
                y = F.batch_norm(y, sd[bn + ".running_mean"], sd[bn + ".running_var"],
                                 sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, BN_EPS)
            if residual is not None:
                y = y + residual
            return F.relu(y) if relu else y
        # HIP storage model: fold, round weights, fp32 accumulate, epilogue in fp32, round on store
        if bn is not None:
            s = (sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + BN_EPS))
            b = (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s).float()
            w = (w.double() * s.view(-1, 1, 1, 1)).float()
        else:
            b = sd[conv + ".bias"].float() if (conv + ".bias") in sd else None
        y = F.conv2d(x, self.rnd(w) if round_w else w, b, stride, pad)
        if residual is not None:
            y = y + residual
        if relu:
            y = F.relu(y)
        return self.rnd(y) if store else y


    def head(self, x, name, k, s):
        """ConvTranspose2d(k, stride s, padding 1, output_padding 1) + Conv2d (hrnet_cms.py:353-368)."""
        sd = self.sd
        wt, bt = sd[name + ".0.weight"].float(), sd[name + ".0.bias"].float()
        wc, bc = sd[name + ".1.weight"].float(), sd[name + ".1.bias"].float()
        if self.dt is None:
            y = F.conv_transpose2d(x, wt, bt, stride=s, padding=1, output_padding=1)
            return F.conv2d(y, wc, bc, 1, (wc.shape[-1] - 1) // 2)
        # HIP storage model (csrc/head.hip): the two linear layers are folded into one transposed convolution
        # C -> J; every kernel tap is a 1x1 convolution whose result ("tap map") is stored in the 16-bit type;
        # the taps that reach an output pixel are summed in fp32 together with the folded bias.
        if wc.shape[-1] != 1:
            raise NotImplementedError("folded heads need FINAL_CONV_KERNEL == 1")
        w, b = head_fold(sd, name)
        return head_gather(lambda ky, kx: self.rnd(F.conv2d(x, self.rnd(w[:, :, ky, kx]).t().reshape(w.shape[1], w.shape[0], 1, 1))),
                           b, k, s, x.shape)


def head_fold(sd, name):
    """The folded transposed convolution of an hrnet_cms head (csrc/hrnet.cpp: Builder::head): weight (C, J, k, k), bias (J,)."""
    wt, bt = sd[name + ".0.weight"].float(), sd[name + ".0.bias"].float()
    wc, bc = sd[name + ".1.weight"].float(), sd[name + ".1.bias"].float()
    w = torch.einsum("cmyx,jm->cjyx", wt.double(), wc[:, :, 0, 0].double()).float()      # (C, J, k, k)
    b = (wc[:, :, 0, 0].double() @ bt.double() + bc.double()).float()
    return w, b


def head_gather(tap, b, k, s, shape):
    """Sum of the tap maps tap(ky, kx) (N, J, h, w) that reach each output pixel of the stride-s transposed convolution
    (padding 1, output_padding 1), plus the bias b: the gather of csrc/head.hip, in the dtype of b."""
    n, _, h, wd = shape
    out = b.view(1, -1, 1, 1).repeat(n, 1, s * h, s * wd).contiguous()
    for ky in range(k):
        for kx in range(k):
            t = tap(ky, kx)
            # output row = s*iy - 1 + ky, for the input rows whose target lies inside the map
            iy0 = 1 if ky == 0 else 0
            ix0 = 1 if kx == 0 else 0
            iy1 = min(h, (s * h - ky) // s + 1)
            ix1 = min(wd, (s * wd - kx) // s + 1)
            out[:, :, s * iy0 - 1 + ky: s * (iy1 - 1) + ky: s, s * ix0 - 1 + kx: s * (ix1 - 1) + kx: s] += t[:, :, iy0:iy1, ix0:ix1]
    return out


def forward(sd, cfg, x, emulate=None, taps=None):
    """x: (N,3,H,W) float32, ImageNet-normalised.  Returns (N,J,H/4,W/4) float32 heatmaps
    (hrnet_cms: (N,J,H,W); hrnet_cms_384: (N,J,H/2,W/2)).
    ``taps``: optional dict that receives named intermediate tensors."""
    ex = extra_of(cfg)
    A = _Arith(sd, emulate)

    def tap(name, t):
        if taps is not None:
            taps[name] = t
        return t

    x = x.float()
    # the HIP stem (csrc/stem_fused.hip) runs conv1 on MFMA like every other layer: the normalised input and the folded
    # weights are rounded to the 16-bit operand type, the sum is fp32, the stored result is rounded
    x = tap("stem1", A.conv_bn(A.rnd(x), "conv1", "bn1", 2, relu=True))
    x = tap("stem2", A.conv_bn(x, "conv2", "bn2", 2, relu=True))
    for b in range(4):
        p = "layer1.%d" % b
        # storage model: the HIP plan runs the first Bottleneck's downsample 1x1 conv and its conv3 as ONE K-concatenated
        # convolution (csrc/hrnet.cpp: conv_cat), so that residual is summed in fp32 and never rounded to 16 bits
        res = A.conv_bn(x, p + ".downsample.0", p + ".downsample.1", store=False) if b == 0 else x
        y = A.conv_bn(x, p + ".conv1", p + ".bn1", relu=True)
        y = A.conv_bn(y, p + ".conv2", p + ".bn2", relu=True)
        x = A.conv_bn(y, p + ".conv3", p + ".bn3", relu=True, residual=res)
    tap("layer1", x)

    ylist = [x]
    pre = [256]
    for si, sname in enumerate(("STAGE2", "STAGE3", "STAGE4")):
        scfg = ex[sname]
        cur = _stage_channels(scfg)
        tname = "transition%d" % (si + 1)
        xs = []
        for i in range(len(cur)):
            if i < len(pre):
                if cur[i] != pre[i]:
                    src = ylist[-1]                            # reference :437,:445,:453 -- always the LAST branch
                    xs.append(A.conv_bn(src, "%s.%d.0" % (tname, i), "%s.%d.1" % (tname, i), relu=True))
                else:
                    xs.append(ylist[i])
            else:
                t = ylist[-1]                                  # reference :445,:453 -- from the LAST branch
                for j in range(i + 1 - len(pre)):
                    t = A.conv_bn(t, "%s.%d.%d.0" % (tname, i, j), "%s.%d.%d.1" % (tname, i, j), 2, relu=True)
                xs.append(t)
        nb = scfg["NUM_BRANCHES"]
        stname = "stage%d" % (si + 2)
        for m in range(scfg["NUM_MODULES"]):
            multi = head_of(cfg) is not None or not (sname == "STAGE4" and m == scfg["NUM_MODULES"] - 1)
            mp = "%s.%d" % (stname, m)
            for b in range(nb):
                t = xs[b]
                for k in range(scfg["NUM_BLOCKS"][b]):
                    p = "%s.branches.%d.%d" % (mp, b, k)
                    if scfg["BLOCK"] == "BOTTLENECK":      # pose_hrnet.py:78-98 with identity residual
                        u = A.conv_bn(t, p + ".conv1", p + ".bn1", relu=True)
                        u = A.conv_bn(u, p + ".conv2", p + ".bn2", relu=True)
                        t = A.conv_bn(u, p + ".conv3", p + ".bn3", relu=True, residual=t)
                        continue
                    u = A.conv_bn(t, p + ".conv1", p + ".bn1", relu=True)
                    t = A.conv_bn(u, p + ".conv2", p + ".bn2", relu=True, residual=t)
                xs[b] = t
            outs = []
            for i in range(nb if multi else 1):
                acc = None
                for j in range(nb):
                    fp = "%s.fuse_layers.%d.%d" % (mp, i, j)
                    if j == i:
                        term = xs[j]
                    elif j > i:
                        z = A.conv_bn(xs[j], fp + ".0", fp + ".1")
                        term = F.interpolate(z, scale_factor=2 ** (j - i), mode="nearest")
                    else:
                        term = xs[j]
                        for k in range(i - j):
                            last = k == i - j - 1
                            term = A.conv_bn(term, "%s.%d.0" % (fp, k), "%s.%d.1" % (fp, k), 2, relu=not last)
                    acc = term if acc is None else acc + term
                outs.append(A.rnd(F.relu(acc)))
            xs = outs
            tap("%s.out0" % mp, xs[0])
        ylist = xs
        pre = cur
    if head_of(cfg) is None:
        out = A.conv_bn(ylist[0], "final_layer", None, store=False)
        return tap("heatmaps", out)
    # hrnet_cms.py:551-557: coarse-to-fine sum of the four heads
    _, k, s = head_of(cfg)
    names = head_names(cfg)
    out = None
    for b in (3, 2, 1, 0):
        y = A.head(ylist[b], names[b], k, s)
        if out is not None:
            y = y + F.interpolate(out, scale_factor=2, mode="bilinear", align_corners=False)
        out = tap("head%d" % b, y)
    return tap("heatmaps", out)


# ----------------------------------------------------------------------------- op-level walk (teacher forcing)
# walk(cfg) lists every tensor the HIP forward writes, by the name scpose_hrnet_forward_tap offers it under, as one op of the
# reference: its kind, the names of its input tensors, the state-dict prefixes it reads, and its stages.  run_op() evaluates
# one op from given inputs (the HIP's own 16-bit tensors in the GPU tests), in the fp32 storage model of forward() or in
# float64 with one rounding per storage point.  A stage is
#   ("conv", src, conv, bn, stride, relu, res, store)   src / res: ("in", i) an input of the op, ("st", j) an earlier stage
#   ("sum", [(src, shift), ...])                        relu(sum of nearest-upsampled terms), stored (fuse row)
#   ("tapmap", src, head)                               the 16-bit tap map of an hrnet_cms head (csrc/hrnet.cpp: Builder::head)
#   ("pyramid", [src per branch 0..3])                  the hrnet_cms heads' gather + coarse-to-fine sum, f32 (head.hip)
# Composite ops (a fused BasicBlock / Bottleneck / stem) keep their internal 16-bit rounding points as stages.

def walk(cfg, offered=None):
    """OrderedDict name -> {"kind", "inputs", "prefixes", "stages", "out_f32"}.  ``offered``: the engine's tap names; a block
    whose "<block>.conv1" (stem: "stem1") is offered is split into single-rounding ops, else it is one composite op."""
    ex = extra_of(cfg)
    ops = OrderedDict()
    split = lambda n: offered is None or n in offered

    def add(name, kind, inputs, stages, out_f32=False):
        pre = sorted({st[2] for st in stages if st[0] in ("conv", "tapmap")})
        ops[name] = {"kind": kind, "inputs": list(inputs), "prefixes": pre, "stages": stages, "out_f32": out_f32}
        return name

    IN0, IN1 = ("in", 0), ("in", 1)

    def conv(src, c, bn, stride=1, relu=True, res=None, store=True):
        return ("conv", src, c, bn, stride, relu, res, store)

    if split("stem1"):
        x = add("stem1", "stem_conv", ["input"], [conv(IN0, "conv1", "bn1", 2)])
        x = add("stem2", "stem_conv", [x], [conv(IN0, "conv2", "bn2", 2)])
    else:
        x = add("stem2", "stem_fused", ["input"], [conv(IN0, "conv1", "bn1", 2), conv(("st", 0), "conv2", "bn2", 2)])
    for b in range(4):
        p = "layer1.%d" % b
        # layer1.0's downsample residual rides in conv3's accumulator (conv_cat / bottleneck.hip): never rounded
        res = [conv(IN0, p + ".downsample.0", p + ".downsample.1", relu=False, store=False)] if b == 0 else []
        rref = ("st", 0) if b == 0 else IN0
        o = len(res)
        if split(p + ".conv1"):
            y = add(p + ".conv1", "bneck_conv1", [x], [conv(IN0, p + ".conv1", p + ".bn1")])
            y = add(p + ".conv2", "bneck_conv2", [y], [conv(IN0, p + ".conv2", p + ".bn2")])
            ds = [conv(IN1, p + ".downsample.0", p + ".downsample.1", relu=False, store=False)] if b == 0 else []
            x = add(p, "bneck_conv3", [y, x], ds + [conv(IN0, p + ".conv3", p + ".bn3", res=("st", 0) if b == 0 else IN1)])
        else:
            x = add(p, "bottleneck", [x], res + [conv(IN0, p + ".conv1", p + ".bn1"), conv(("st", o), p + ".conv2", p + ".bn2"),
                                                 conv(("st", o + 1), p + ".conv3", p + ".bn3", res=rref)])
    add("layer1", "alias", [x], [])
    ylist, pre = [x], [256]
    for si, sname in enumerate(("STAGE2", "STAGE3", "STAGE4")):
        scfg = ex[sname]
        cur = _stage_channels(scfg)
        tname = "transition%d" % (si + 1)
        xs = []
        for i in range(len(cur)):
            if i < len(pre):
                if cur[i] != pre[i]:
                    n = "%s.%d" % (tname, i)
                    xs.append(add(n, "transition", [ylist[-1]], [conv(IN0, n + ".0", n + ".1")]))     # from the LAST branch
                else:
                    xs.append(ylist[i])
            else:
                t = ylist[-1]
                for j in range(i + 1 - len(pre)):
                    n = "%s.%d.%d" % (tname, i, j)
                    t = add(n, "transition_s2", [t], [conv(IN0, n + ".0", n + ".1", 2)])
                xs.append(t)
        nb = scfg["NUM_BRANCHES"]
        for m in range(scfg["NUM_MODULES"]):
            multi = head_of(cfg) is not None or not (sname == "STAGE4" and m == scfg["NUM_MODULES"] - 1)
            mp = "stage%d.%d" % (si + 2, m)
            for b in range(nb):
                t = xs[b]
                for k in range(scfg["NUM_BLOCKS"][b]):
                    p = "%s.branches.%d.%d" % (mp, b, k)
                    if scfg["BLOCK"] == "BOTTLENECK":
                        if split(p + ".conv1"):
                            u = add(p + ".conv1", "bneck_conv1", [t], [conv(IN0, p + ".conv1", p + ".bn1")])
                            u = add(p + ".conv2", "bneck_conv2", [u], [conv(IN0, p + ".conv2", p + ".bn2")])
                            t = add(p, "bneck_conv3", [u, t], [conv(IN0, p + ".conv3", p + ".bn3", res=IN1)])
                        else:
                            t = add(p, "bottleneck", [t], [conv(IN0, p + ".conv1", p + ".bn1"), conv(("st", 0), p + ".conv2", p + ".bn2"),
                                                           conv(("st", 1), p + ".conv3", p + ".bn3", res=IN0)])
                    elif split(p + ".conv1"):
                        u = add(p + ".conv1", "block_conv1", [t], [conv(IN0, p + ".conv1", p + ".bn1")])
                        t = add(p, "block_conv2", [u, t], [conv(IN0, p + ".conv2", p + ".bn2", res=IN1)])
                    else:
                        t = add(p, "block_fused", [t], [conv(IN0, p + ".conv1", p + ".bn1"), conv(("st", 0), p + ".conv2", p + ".bn2", res=IN0)])
                xs[b] = t
            outs = []
            for i in range(nb if multi else 1):
                terms = []
                for j in range(nb):
                    fp = "%s.fuse_layers.%d.%d" % (mp, i, j)
                    if j == i:
                        terms.append((xs[j], 0))
                    elif j > i:
                        terms.append((add(fp, "fuse_up", [xs[j]], [conv(IN0, fp + ".0", fp + ".1", relu=False)]), j - i))
                    else:
                        t = xs[j]
                        for k in range(i - j):
                            last = k == i - j - 1                  # the last hop of a down path has no ReLU
                            n = "%s.%d" % (fp, k)
                            t = add(n, "fuse_down_last" if last else "fuse_down_hop", [t], [conv(IN0, n + ".0", n + ".1", 2, relu=not last)])
                        terms.append((t, 0))
                outs.append(add("%s.out%d" % (mp, i), "fuse_sum", [t for t, _ in terms],
                                [("sum", [(("in", q), sh) for q, (_, sh) in enumerate(terms)])]))
            xs = outs
        ylist, pre = xs, cur
    if head_of(cfg) is None:
        add("heatmaps", "final_layer", [ylist[0]], [conv(IN0, "final_layer", None, relu=False, store=False)], out_f32=True)
    else:
        names = head_names(cfg)
        maps = [None] * 4
        for b in (3, 2, 1, 0):
            maps[b] = add(names[b] + ".tapmap", "head_tapmap", [ylist[b]], [("tapmap", IN0, names[b])])
        add("heatmaps", "head_pyramid", maps, [("pyramid", [("in", b) for b in range(4)])], out_f32=True)
    return ops


_DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def u16(t, emulate):
    """Spacing of the 16-bit grid at |t| (float64): 2^(e - p) with the subnormal floor; p = 7 (bf16) / 10 (f16) fraction bits."""
    frac, emin = {"bf16": (7, -126), "f16": (10, -14)}[emulate]
    e = torch.floor(torch.log2(t.abs().double().clamp_min(2.0 ** emin)))
    return torch.exp2(e.clamp_min(emin) - frac)


def folded(sd, c, bn, emulate):
    """Folded weight (16-bit values, f32 / f64 exact) and f32 bias of conv c + bn, as csrc/hrnet.cpp: fold() makes them."""
    w = sd[c + ".weight"].float()
    if bn is not None:
        s_ = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + BN_EPS)
        b = (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s_).float()
        w = (w.double() * s_.view(-1, 1, 1, 1)).float()
    else:
        b = sd[c + ".bias"].float() if (c + ".bias") in sd else torch.zeros(w.shape[0])
    return w.to(_DT[emulate]).float(), b


def _up(t, sh):
    return t if sh == 0 else F.interpolate(t, scale_factor=2 ** sh, mode="nearest")


def run_op(sd, cfg, op, inputs, emulate, acc="fp32", bound=False):
    """Evaluates walk() op ``op`` on ``inputs`` (tensors in the order of op["inputs"]).
    acc="fp32": the storage model of forward(emulate=...) -- bit-identical to its taps.
    acc="f64":  float64 accumulation, bias / residual / ReLU in float64, one 16-bit rounding (RNE) at each point the HIP path
                stores; weights folded in double and rounded to 16 bits once.  With bound=True also returns E, the arithmetic
                error allowance of an fp32-accumulating implementation on the same inputs, WITHOUT the final store's rounding
                term (tests/op_bound.py adds u16 of the output): per stage y = round16(relu(sum w x + b + r)),
                  E = K 2^-24 S + conv(E_in, |w|) + E_res,  K = Cin k^2 + 2,  S = conv(|x|, |w|) + |b| + |r|,
                and an internal stored stage passes on E + u16(|y| + E) (its rounding and the other side's may differ by a step)."""
    if op["kind"] == "alias":
        return (inputs[0], torch.zeros_like(inputs[0], dtype=torch.float64)) if bound else inputs[0]
    f64 = acc == "f64"
    A = _Arith(sd, emulate)
    dt = torch.float64 if f64 else torch.float32
    vals, errs, sums, ks = [], [], [], []     # per stage: value, error allowance, S, K (unstored stages only pass S, K on)
    ins = [t.to(dt) for t in inputs]

    def ref(r):
        if r[0] == "in":
            return ins[r[1]], torch.zeros_like(ins[r[1]]), ins[r[1]].abs(), 0
        return vals[r[1]], errs[r[1]], sums[r[1]], ks[r[1]]

    def stored(v, e):
        y = v.to(_DT[emulate]).to(dt)
        return y, (e + u16(y.abs() + e, emulate) if bound else e)

    last = len(op["stages"]) - 1
    for si, st in enumerate(op["stages"]):
        kind = st[0]
        if kind == "conv":
            _, src, c, bn, stride, relu, res, store = st
            x, ex_, _, _ = ref(src)
            if not f64:
                r = ref(res)[0] if res is not None else None
                v = A.conv_bn(x, c, bn, stride, relu=relu, residual=r, store=store)
                vals.append(v); errs.append(None); sums.append(None); ks.append(0)
                continue
            w, b = folded(sd, c, bn, emulate)
            w, b = w.double(), b.double()
            pad = (w.shape[-1] - 1) // 2
            v = F.conv2d(x, w, b, stride, pad)
            K = w.shape[1] * w.shape[2] * w.shape[3] + 2
            S = e = None
            if bound:
                S = F.conv2d(x.abs(), w.abs(), b.abs(), stride, pad)
                e = F.conv2d(ex_, w.abs(), None, stride, pad)
            if res is not None:
                r, er, Sr, Kr = ref(res)
                v = v + r
                if bound:
                    S, e = S + Sr, e + er
                    K += Kr                 # an unstored residual (conv_cat) is summed in the same fp32 accumulator
            if relu:
                v = F.relu(v)
            if bound and not (si < last and not store):
                e = e + K * 2.0 ** -24 * S
            if store and si < last:
                v, e = stored(v, e)
            elif si == last and store and not op["out_f32"]:
                v = v.to(_DT[emulate]).to(dt)
            vals.append(v); errs.append(e); sums.append(S); ks.append(K if not store else 0)
        elif kind == "sum":
            terms = [(ref(r), sh) for r, sh in st[1]]
            v = None
            for (t, _, _, _), sh in terms:
                v = _up(t, sh) if v is None else v + _up(t, sh)
            v = F.relu(v)
            if not f64:
                vals.append(A.rnd(v)); errs.append(None); sums.append(None); ks.append(0)
                continue
            e = None
            if bound:
                S = sum(_up(t.abs(), sh) for (t, _, _, _), sh in terms)
                e = len(terms) * 2.0 ** -24 * S + sum(_up(et, sh) for (_, et, _, _), sh in terms)
            vals.append(v.to(_DT[emulate]).to(dt)); errs.append(e); sums.append(None); ks.append(0)
        elif kind == "tapmap":
            _, src, name = st
            x, ex_, _, _ = ref(src)
            w, _ = head_fold(sd, name)                                   # (C, J, k, k)
            C, J, k, _ = w.shape
            cpt = 8 if J <= 8 else 16
            wt = torch.zeros(k * k * cpt, C)
            wt.view(k * k, cpt, C)[:, :J] = w.permute(2, 3, 1, 0).reshape(k * k, J, C)
            wt = wt.to(_DT[emulate]).to(dt).view(-1, C, 1, 1)
            v = F.conv2d(x, wt)
            if f64:
                e = None
                if bound:
                    e = (C + 2) * 2.0 ** -24 * F.conv2d(x.abs(), wt.abs()) + F.conv2d(ex_, wt.abs())
                vals.append(v.to(_DT[emulate]).to(dt)); errs.append(e)
            else:
                vals.append(A.rnd(v)); errs.append(None)
            sums.append(None); ks.append(0)
        elif kind == "pyramid":
            _, k, s = head_of(cfg)
            names = head_names(cfg)
            out = e = None
            for b in (3, 2, 1, 0):
                t, et, _, _ = ref(st[1][b])
                J = cfg["MODEL"]["NUM_JOINTS"]
                cpt = t.shape[1] // (k * k)
                tap = lambda ky, kx, t=t: t[:, (ky * k + kx) * cpt:(ky * k + kx) * cpt + J]
                bias = head_fold(sd, names[b])[1].to(dt)
                y = head_gather(tap, bias, k, s, t.shape)
                if bound:
                    Sy = head_gather(lambda ky, kx, t=t: tap(ky, kx, t).abs(), bias.abs(), k, s, t.shape)
                    eb = head_gather(lambda ky, kx, et=et: et[:, (ky * k + kx) * cpt:(ky * k + kx) * cpt + J], torch.zeros_like(bias), k, s, t.shape)
                if out is not None:
                    up = F.interpolate(out, scale_factor=2, mode="bilinear", align_corners=False)
                    y = y + up
                    if bound:
                        Sy = Sy + F.interpolate(Sy_prev, scale_factor=2, mode="bilinear", align_corners=False)
                        eb = eb + F.interpolate(e, scale_factor=2, mode="bilinear", align_corners=False)
                if bound:
                    e = eb + (k * k + 8) * 2.0 ** -24 * Sy     # taps + bias + the bilinear term's 4 products and 3 sums
                    Sy_prev = Sy
                out = y
            vals.append(out); errs.append(e); sums.append(None); ks.append(0)
    if bound:
        return vals[-1], errs[-1]
    return vals[-1]
