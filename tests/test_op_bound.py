"""CPU self-tests of the op-level parity harness (oracle/hrnet_ref.walk / run_op, tests/op_bound.py).

  * the walk IS the forward: evaluated on its own outputs in the fp32 storage model it reproduces every tap of
    forward(emulate=...) and the heat-maps bit for bit (transitions from the LAST branch, no ReLU on the last down hop,
    layer1.0's unrounded downsample residual, the folded hrnet_cms heads);
  * the bound accepts a correct implementation: CPU fp32 conv2d (another summation order) on the same 16-bit operands
    passes the hard bound and the bias check against the float64 reference, for every op kind, bf16 and f16;
  * the bound rejects the kernel bugs it is there for (a misplaced lane, a missing halo tap, a missing bias, truncation,
    a stale tile, a dropped K-chunk).
"""
import pytest
import torch
import torch.nn.functional as F

import op_bound as OB
from oracle import hrnet_ref as R


def _final3(cfg):
    cfg = {"MODEL": dict(cfg["MODEL"])}
    cfg["MODEL"]["EXTRA"] = dict(cfg["MODEL"]["EXTRA"], FINAL_CONV_KERNEL=3)
    return cfg


WALK_CASES = {
    "tiny": (R.tiny_cfg(), (64, 64), "bf16", None),
    "tiny_composite": (R.tiny_cfg(), (96, 64), "f16", set()),     # nothing offered: every fusable group is one composite op
    "w32_64": (R.w32_cfg(), (64, 64), "bf16", None),
    "bneck16_64": (R.bneck_cfg(c=16), (64, 64), "bf16", set()),
    "hrnet_cms": (R.with_model(R.tiny_cfg(), "hrnet_cms"), (64, 64), "bf16", None),
    "hrnet_cms_384": (R.with_model(R.tiny_cfg(), "hrnet_cms_384"), (64, 64), "bf16", None),
}


def _walk_env(cfg, x, dt, offered, acc="fp32", sd=None):
    env = {"input": x.to(R._DT[dt]).float()}
    for name, op in R.walk(cfg, offered).items():
        env[name] = R.run_op(sd, cfg, op, [env[i] for i in op["inputs"]], dt, acc=acc)
    return env


@pytest.mark.parametrize("name", list(WALK_CASES))
def test_walk_reproduces_forward_bit_for_bit(name):
    cfg, (h, w), dt, offered = WALK_CASES[name]
    sd = R.make_state_dict(cfg, seed=3)
    x = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(4))
    taps = {}
    with torch.no_grad():
        hm = R.forward(sd, cfg, x, emulate=dt, taps=taps)
        env = _walk_env(cfg, x, dt, offered, sd=sd)
    shared = [k for k in taps if k in env]
    assert len(shared) >= 5 and set(taps) - set(shared) <= {"stem1", "head0", "head1", "head2", "head3"}
    for k in shared:
        assert torch.equal(env[k], taps[k]), k
    assert torch.equal(env["heatmaps"], hm)
    walk = R.walk(cfg, offered)
    assert all(op["inputs"] and all(i in walk or i == "input" for i in op["inputs"]) for op in walk.values())


def test_walk_wiring():
    """Spot checks of what the bit-exact test relies on: transitions start from the LAST branch; the last down hop has no
    ReLU; the first Bottleneck's downsample is an unstored stage; 1x1 up paths are stored before upsampling."""
    walk = R.walk(R.w32_cfg())
    assert walk["transition2.2.0"]["inputs"] == ["stage2.0.out1"]
    assert walk["transition3.3.0"]["inputs"] == ["stage3.3.out2"]
    assert walk["transition1.0"]["inputs"] == ["layer1.3"] and walk["transition1.1.0"]["inputs"] == ["layer1.3"]
    hop = walk["stage4.0.fuse_layers.3.0.2"]["stages"][0]
    assert hop[5] is False and walk["stage4.0.fuse_layers.3.0.1"]["stages"][0][5] is True
    ds = walk["layer1.0"]["stages"][0]
    assert ds[2] == "layer1.0.downsample.0" and ds[7] is False
    up = walk["stage3.0.fuse_layers.0.2"]["stages"][0]
    assert up[4] == 1 and up[5] is False and up[7] is True
    assert "stage4.2.out1" not in walk and "stage4.2.out0" in walk          # the last module fuses to branch 0 only


CORRECT_CASES = {
    "tiny": (R.tiny_cfg(), (64, 64), None),
    "tiny_composite": (R.tiny_cfg(), (64, 96), set()),
    "bneck": (R.bneck_cfg(c=16), (64, 64), None),
    "bneck_composite": (R.bneck_cfg(c=16), (64, 64), set()),
    "hrnet_cms": (R.with_model(R.tiny_cfg(), "hrnet_cms"), (64, 64), None),
    "hrnet_cms_384": (R.with_model(R.tiny_cfg(), "hrnet_cms_384"), (64, 64), None),
    "final3": (_final3(R.tiny_cfg()), (64, 64), None),
}


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(CORRECT_CASES))
def test_bound_accepts_fp32_conv2d(name, dt):
    """Teacher forcing with CPU fp32 conv2d as the 'kernel': each op, fed with the fp32 model's own 16-bit inputs, passes
    the hard bound and the bias check against its float64 reference."""
    cfg, (h, w), offered = CORRECT_CASES[name]
    sd = R.make_state_dict(cfg, seed=5)
    x = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(6))
    kinds = set()
    with torch.no_grad():
        env = _walk_env(cfg, x, dt, offered, sd=sd)
        for op_name, op in R.walk(cfg, offered).items():
            if op["kind"] == "alias":
                continue
            ins = [env[i] for i in op["inputs"]]
            ref, E = R.run_op(sd, cfg, op, ins, dt, acc="f64", bound=True)
            OB.check(env[op_name], ref, E, dt, "%s %s" % (op_name, op["kind"]), out_f32=op["out_f32"],
                     bias_check=ref.numel() >= 4096)
            kinds.add(op["kind"])
    assert len(kinds) >= 5


def _conv_case(dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    tdt = R._DT[dt]
    x = torch.randn(2, 32, 24, 24, generator=g).to(tdt).float()
    w = (torch.randn(32, 32, 3, 3, generator=g) / (32 * 9) ** 0.5).to(tdt).float()
    b = torch.randn(32, generator=g) * 0.1
    b[5] = 0.5
    return x, w, b


def _store(v, dt, trunc=False):
    y = v.to(R._DT[dt]).float()
    if trunc:                                   # round toward zero: step back where RNE rounded away
        away = y.abs() > v.abs()
        step = torch.nextafter(y.to(R._DT[dt]), torch.zeros_like(y).to(R._DT[dt])).float()
        y = torch.where(away, step, y)
    return y


MUTATIONS = ["none", "lane_shift", "halo_row", "bias_channel", "truncate", "stale_tile", "kchunk"]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mut", MUTATIONS)
def test_bound_rejects_kernel_bugs(mut, dt):
    x, w, b = _conv_case(dt)
    ref, E, _ = OB.conv_ref(x, w, b, 1, dt, relu=True)
    pre = F.conv2d(x, w, b, 1, 1)                                   # fp32: a correct implementation's accumulator
    if mut == "lane_shift":
        pre[0, :, 9, 10] = pre[0, :, 9, 11]
    elif mut == "halo_row":                                         # row 16 (a tile's first row) without the row above it
        w0 = w.clone(); w0[:, :, 0, :] = 0
        pre[:, :, 16] = F.conv2d(x, w0, b, 1, 1)[:, :, 16]
    elif mut == "bias_channel":
        pre[:, 5] -= b[5]
    elif mut == "stale_tile":
        pre[0, :, 0:16, 0:16] = pre[1, :, 0:16, 0:16]
    elif mut == "kchunk":
        wk = w.clone(); wk[:, 8:16] = 0
        pre = F.conv2d(x, wk, b, 1, 1)
    got = _store(F.relu(pre), dt, trunc=mut == "truncate")
    if mut == "none":
        OB.check(got, ref, E, dt, "correct")
    else:
        with pytest.raises(AssertionError):
            OB.check(got, ref, E, dt, mut)


def test_u16_grid_spacing():
    for dt, frac, emin in (("bf16", 7, -126), ("f16", 10, -14)):
        t = torch.tensor([1.0, 1.5, 2.0, 0.75, 2.0 ** emin, 2.0 ** (emin - 3), 0.0])
        want = torch.tensor([1.0, 1.0, 2.0, 0.5, 1.0, 1.0, 1.0], dtype=torch.float64) * 2.0 ** -frac
        want[4:] = 2.0 ** (emin - frac)
        assert torch.equal(OB.u16(t, dt), want)
        y = torch.tensor([1.0]).to(R._DT[dt])
        assert torch.nextafter(y, torch.tensor([2.0]).to(R._DT[dt])).double().item() - 1.0 == OB.u16(torch.tensor([1.0]), dt).item()
