#!/usr/bin/env python3
"""Golden vectors for HRNet widths that are no multiple of 16 (W18 / W40 / W44 scaled down): the REFERENCE modules
(lib/models/pose_hrnet.py, hrnet_cms.py, hrnet_cms_384.py, imported the way make_golden.py does) built at those widths,
loaded strictly with the seeded synthetic checkpoint and run in fp32 on a seeded input.  Only data is written:
tests/golden/hrnet_widths_reference_outputs.npz holds, per case, the heat-maps, meta = [size, n, weight seed, input seed]
and the number of state_dict keys.  Re-run: python tests/golden/make_hrnet_widths_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (the reference importer and the cfg wrapper)

R = G.R


def cases():
    """name -> (MODEL.NAME, cfg, size, n, weight seed, input seed); shared with the tests through the npz's meta."""
    c18 = R.tiny_cfg(c=18)
    return {
        "c18_64": ("pose_hrnet", c18, 64, 2, 31, 32),
        "c18_m143_64": ("pose_hrnet", R.tiny_cfg(c=18, modules=(1, 4, 3)), 64, 1, 33, 34),
        "c40_64": ("pose_hrnet", R.tiny_cfg(c=40), 64, 1, 35, 36),
        "c44_64": ("pose_hrnet", R.tiny_cfg(c=44), 64, 1, 37, 38),
        "bneck18_64": ("pose_hrnet", R.bneck_cfg(c=18, blocks=1), 64, 1, 39, 40),
        "cms_c18_64": ("hrnet_cms", R.with_model(c18, "hrnet_cms"), 64, 1, 41, 42),
        "cms384_c18_64": ("hrnet_cms_384", R.with_model(c18, "hrnet_cms_384"), 64, 1, 43, 44),
    }


def main():
    torch.manual_seed(0)
    out = {}
    for name, (model, cfg, size, n, wseed, xseed) in cases().items():
        net = G.ref_pose_hrnet(model).get_pose_net(G.AttrDict(cfg), False).eval()
        sd = R.make_state_dict(cfg, seed=wseed)
        net.load_state_dict(sd, strict=True)
        x = torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(xseed))
        with torch.no_grad():
            y = net(x)
        out[name + "/heatmaps"] = y.numpy()
        out[name + "/meta"] = np.array([size, n, wseed, xseed], dtype=np.int64)
        out[name + "/num_keys"] = np.array([len(sd)], dtype=np.int64)
        print(name, tuple(y.shape), float(y.std()))
    np.savez_compressed(os.path.join(HERE, "hrnet_widths_reference_outputs.npz"), **out)


if __name__ == "__main__":
    main()
