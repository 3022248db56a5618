"""Host-side mirror of the reference pose_resnet module API (the SimpleBaseline network), executing on the HIP engine.

Interface kept from landmark_regression/lib/models/pose_resnet.py:
  get_pose_net(cfg, is_train, **kwargs) -> nn.Module
  module(x: float32 N x 3 x H x W, normalised) -> float32 N x J x H/32 * 2^L x W/32 * 2^L   (L = NUM_DECONV_LAYERS)
  .state_dict() / .load_state_dict(sd, strict=False) with the reference's key names and shapes: conv1 / bn1,
  layer1..layer4 of BasicBlocks (NUM_LAYERS 18, 34) or Bottlenecks (50, 101, 152), deconv_layers (ConvTranspose2d,
  BatchNorm2d, ReLU triples, so the parameters sit at indices 3i and 3i + 1), final_layer.

Like pose_hrnet.py here, the module tree only HOLDS parameters; forward() hands them to libscpose_hip.so
(csrc/hrnet.cpp: resnet_build).  Engine lifetime, forward, forward_decode and the flip test are pose_hrnet's.
"""
import torch.nn as nn

from .pose_hrnet import BN_MOMENTUM, PoseHighResolutionNet, _Params, _bottleneck, _conv, _get_pose_net

RESNET_SPEC = {18: (False, (2, 2, 2, 2)), 34: (False, (3, 4, 6, 3)), 50: (True, (3, 4, 6, 3)),
               101: (True, (3, 4, 23, 3)), 152: (True, (3, 8, 36, 3))}
DECONV_CFG = {4: (1, 0), 3: (1, 1), 2: (0, 0)}     # kernel -> (padding, output_padding), _get_deconv_cfg


def _block(bneck, cin, planes, stride, downsample):
    if bneck:
        m = _bottleneck(cin, planes, False)
        m.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)          # the stride sits on the 3x3
        cout = planes * 4
    else:
        m = _Params()
        m.conv1 = nn.Conv2d(cin, planes, 3, stride, 1, bias=False); m.bn1 = nn.BatchNorm2d(planes, momentum=BN_MOMENTUM)
        m.conv2 = _conv(planes, planes, 3); m.bn2 = nn.BatchNorm2d(planes, momentum=BN_MOMENTUM)
        cout = planes
    if downsample:
        m.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout, momentum=BN_MOMENTUM))
    return m


class PoseResNet(PoseHighResolutionNet):
    MODEL_NAME = "pose_resnet"

    def __init__(self, cfg, **kwargs):
        nn.Module.__init__(self)
        extra = cfg["MODEL"]["EXTRA"]
        layers = int(extra["NUM_LAYERS"])
        if layers not in RESNET_SPEC:
            raise ValueError("EXTRA.NUM_LAYERS=%d: pose_resnet is built for %s" % (layers, sorted(RESNET_SPEC)))
        n_deconv = int(extra["NUM_DECONV_LAYERS"])
        filters, kernels = list(extra["NUM_DECONV_FILTERS"]), list(extra["NUM_DECONV_KERNELS"])
        if n_deconv != len(filters) or n_deconv != len(kernels):
            raise ValueError("EXTRA.NUM_DECONV_LAYERS=%d differs from len(NUM_DECONV_FILTERS)=%d or len(NUM_DECONV_KERNELS)=%d"
                             % (n_deconv, len(filters), len(kernels)))
        with_bias = bool(extra["DECONV_WITH_BIAS"])
        fk = int(extra["FINAL_CONV_KERNEL"])
        self._cfg_model = {"NAME": self.MODEL_NAME, "NUM_JOINTS": int(cfg["MODEL"]["NUM_JOINTS"]),
                           "EXTRA": {"NUM_LAYERS": layers, "DECONV_WITH_BIAS": with_bias, "NUM_DECONV_LAYERS": n_deconv,
                                     "NUM_DECONV_FILTERS": [int(f) for f in filters], "NUM_DECONV_KERNELS": [int(k) for k in kernels],
                                     "FINAL_CONV_KERNEL": fk}}
        self.dtype_name = kwargs.get("dtype", "bf16")
        bneck, blocks = RESNET_SPEC[layers]
        exp = 4 if bneck else 1
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False); self.bn1 = nn.BatchNorm2d(64, momentum=BN_MOMENTUM)
        inplanes = 64
        for li, nb in enumerate(blocks):
            planes, stride = 64 << li, (1 if li == 0 else 2)
            mods = []
            for b in range(nb):
                s = stride if b == 0 else 1
                mods.append(_block(bneck, inplanes, planes, s, b == 0 and (s != 1 or inplanes != planes * exp)))
                inplanes = planes * exp
            setattr(self, "layer%d" % (li + 1), nn.Sequential(*mods))
        deconv = []
        for f, k in zip(filters, kernels):
            if int(k) not in DECONV_CFG:
                raise ValueError("EXTRA.NUM_DECONV_KERNELS entry %s: deconv kernels are 4, 3 or 2" % k)
            pad, opad = DECONV_CFG[int(k)]
            deconv += [nn.ConvTranspose2d(inplanes, int(f), int(k), 2, pad, opad, bias=with_bias),
                       nn.BatchNorm2d(int(f), momentum=BN_MOMENTUM), nn.ReLU(inplace=True)]
            inplanes = int(f)
        self.deconv_layers = nn.Sequential(*deconv)
        self.final_layer = _conv(inplanes, int(cfg["MODEL"]["NUM_JOINTS"]), fk, 1, bias=True)
        self.pretrained_layers = extra["PRETRAINED_LAYERS"] if "PRETRAINED_LAYERS" in extra else ["*"]
        self._engine = None
        self._engine_version = None
        self._param_tensors = None


def get_pose_net(cfg, is_train, **kwargs):
    return _get_pose_net(PoseResNet, cfg, is_train, **kwargs)
