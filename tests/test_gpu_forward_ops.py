"""Every op of the real HIP forward against a float64 reference of that op alone (teacher forcing).

Each tensor the engine writes is read through scpose_hrnet_forward_tap; each op of oracle/hrnet_ref.walk() is evaluated
in float64 (run_op(acc="f64")) on the HIP's OWN 16-bit inputs and compared with the HIP's output by the arithmetic rule
of tests/op_bound.py.  Chaotic accumulation of two free-running 16-bit pipelines (test_gpu_hrnet.TAP_BOUNDS) drops out,
so every op at every depth -- branches 1..3, transitions, fuse rows, down hops, heads -- is held to about one grid step.
The oracle runs on frames 0 and n - 1; the bit-invariance tests of test_gpu_hrnet.py tie these small batches to full ones.

Coverage: the engine's tap names must equal the walk's op names, so a kernel or plan op added without a reference op
fails here.  Beyond the hard bound (derived, every element) and the rounding-bias bound, the only fitted numbers are the
fractions of elements more than one grid step off, per op class, ~2x the largest value measured on the MI355X:
BEYOND_STEP below (measured values beside each entry).
"""
import time

import pytest
import torch

import op_bound as OB
from oracle import hrnet_ref as R

pytestmark = pytest.mark.gpu


def _final3(cfg):
    cfg = {"MODEL": dict(cfg["MODEL"])}
    cfg["MODEL"]["EXTRA"] = dict(cfg["MODEL"]["EXTRA"], FINAL_CONV_KERNEL=3)
    return cfg


CASES = {  # name: (cfg, (H, W), n, dtype)
    "w48_384_bf16": (R.w48_cfg(), (384, 384), 3, "bf16"),             # headline geometry: every default kernel class
    "w48_96x160_bf16": (R.w48_cfg(), (96, 160), 3, "bf16"),           # partial tiles both ways: branch 0 24 x 40, branch 3 3 x 5
    "w32_256_f16": (R.w32_cfg(), (256, 256), 2, "f16"),               # BASELINE configs[1]/[4] geometry in f16
    "w32_64_bf16": (R.w32_cfg(), (64, 64), 2, "bf16"),                # 2 x 2 maps at branch 3
    "tiny_96x64_bf16": (R.tiny_cfg(), (96, 64), 3, "bf16"),           # 16-channel paths, non-square input
    "bneck16_64_bf16": (R.bneck_cfg(c=16), (64, 64), 2, "bf16"),      # stage Bottleneck blocks
    "cms_64_bf16": (R.with_model(R.tiny_cfg(), "hrnet_cms"), (64, 64), 2, "bf16"),
    "cms384_64_bf16": (R.with_model(R.tiny_cfg(), "hrnet_cms_384"), (64, 64), 2, "bf16"),
    "final3_64_bf16": (_final3(R.tiny_cfg()), (64, 64), 2, "bf16"),   # unfused 3x3 final layer, f32 output
}

# Per op class (walk kind, dtype): the largest fraction of one op's elements allowed more than one grid step u16(ref) from
# the float64 reference, ~2x the largest value measured over CASES on the MI355X (measured beside each entry; where nothing
# was measured beyond one step, 2e-5 -- a few elements of a W48 branch-3 tensor).  Most of these elements are relu
# cancellations (ref 0 or tiny, |sum| << S) and, in composite ops, intermediates whose rounding flipped.
# The f32 outputs (final_layer, head_pyramid) have no 16-bit grid and are held by the hard bound alone; a fuse row is a sum
# of at most four 16-bit terms with a single rounding and must never be a step off.
BEYOND_STEP = {
    ("stem_fused", "bf16"): 4e-5,       # 2.03e-05  tiny 96x64
    ("stem_fused", "f16"): 4e-4,        # 1.98e-04  w32 256
    ("bottleneck", "bf16"): 5e-4,       # 2.44e-04  bneck16 64 (c256, stage Bottleneck)
    ("bottleneck", "f16"): 6.4e-4,      # 3.19e-04  w32 256
    ("bneck_conv1", "bf16"): 2e-5,      # 0
    ("bneck_conv2", "bf16"): 2e-5,      # 0
    ("bneck_conv3", "bf16"): 2e-5,      # 0
    ("transition", "bf16"): 6e-5,       # 3.05e-05  bneck16 64
    ("transition", "f16"): 2e-5,        # 0
    ("transition_s2", "bf16"): 2e-5,    # 2.26e-06  w48 384
    ("transition_s2", "f16"): 1.2e-4,   # 6.10e-05  w32 256
    ("block_fused", "bf16"): 3.3e-4,    # 1.63e-04  tiny 96x64
    ("block_fused", "f16"): 1e-3,       # 5.15e-04  w32 256
    ("block_conv1", "bf16"): 9e-5,      # 4.34e-05  w48 96x160
    ("block_conv1", "f16"): 1.8e-4,     # 9.16e-05  w32 256
    ("block_conv2", "bf16"): 9e-5,      # 4.34e-05  w48 96x160
    ("block_conv2", "f16"): 9e-5,       # 4.58e-05  w32 256
    ("fuse_up", "bf16"): 7e-5,          # 3.62e-05  w48 384
    ("fuse_up", "f16"): 5e-4,           # 2.44e-04  w32 256
    ("fuse_down_hop", "bf16"): 9e-5,    # 4.34e-05  w48 96x160
    ("fuse_down_hop", "f16"): 6e-5,     # 3.05e-05  w32 256
    ("fuse_down_last", "bf16"): 4.5e-5, # 2.17e-05  w48 96x160
    ("fuse_down_last", "f16"): 6e-5,    # 3.05e-05  w32 256
    ("fuse_sum", "bf16"): 0.0,          # 0
    ("fuse_sum", "f16"): 0.0,           # 0
    ("head_tapmap", "bf16"): 2e-5,      # 0
}


def _class(op, out):
    return "%s/%s" % (op["kind"], "f32" if op["out_f32"] else "c%d" % out.shape[1])


@pytest.mark.parametrize("name", list(CASES))
def test_every_forward_op_matches_float64_reference(gpu_ops, name):
    cfg, (h, w), n, dt = CASES[name]
    t0 = time.time()
    sd = R.make_state_dict(cfg, seed=21)
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(22))
    eng = gpu_ops.HrnetEngine(cfg, sd, dtype=dt)
    offered = eng.tap_names()
    assert len(offered) == len(set(offered))
    walk = R.walk(cfg, set(offered))
    assert set(offered) == set(walk) - {"heatmaps"}, "engine taps without a reference op: %s; reference ops not offered: %s" % (
        sorted(set(offered) - set(walk)), sorted(set(walk) - set(offered) - {"heatmaps"}))
    frames = [0, n - 1]
    xc = x.cuda()
    env = {"input": x[frames].to(R._DT[dt]).float()}
    for tap in offered:
        env[tap] = eng.forward_tap(xc, tap)[frames].cpu()
    env["heatmaps"] = eng(xc)[frames].cpu()
    t_gpu = time.time() - t0
    classes = {}
    with torch.no_grad():
        for op_name, op in walk.items():
            ins = [env[i] for i in op["inputs"]]
            got = env[op_name]
            if op["kind"] == "alias":
                assert torch.equal(got, ins[0]), op_name
                continue
            ref, E = R.run_op(sd, cfg, op, ins, dt, acc="f64", bound=True)
            assert got.shape == ref.shape, op_name
            s = OB.check(got, ref, E, dt, "%s %s (%s)" % (name, op_name, op["kind"]), out_f32=op["out_f32"],
                         bias_check=ref.numel() >= 4096)
            c = classes.setdefault(_class(op, got), {"n": 0, "ops": 0, "max_ulp": 0.0, "diff": 0.0, "beyond": 0.0, "signed": 0.0})
            c["ops"] += 1
            c["max_ulp"] = max(c["max_ulp"], s["max_ulp"])
            c["use"] = max(c.get("use", 0.0), s["use"])
            c["beyond_max"] = max(c.get("beyond_max", 0.0), s["beyond"])
            for k in ("diff", "beyond", "signed"):
                c[k] += s[k] * s["n"]
            c["n"] += s["n"]
    print("\n%s: %d ops, engine %.1f s, total %.1f s" % (name, len(walk), t_gpu, time.time() - t0))
    # max|d|/u: in steps of u16(max(|got|, |ref|)); bound: max |d| / allowance (< 1 everywhere, or the op failed above);
    # beyond1: elements more than u16(ref) off, over the class / in its worst op (asserted: BEYOND_STEP)
    print("  %-24s %4s %9s %6s %8s %9s %9s %8s" % ("class", "ops", "max|d|/u", "bound", "diff", "beyond1", "worst op", "signed"))
    for k in sorted(classes):
        c = classes[k]
        print("  %-24s %4d %9.3f %6.3f %8.4f %9.2e %9.2e %+8.4f" % (k, c["ops"], c["max_ulp"], c["use"], c["diff"] / c["n"],
                                                                 c["beyond"] / c["n"], c["beyond_max"], c["signed"] / c["n"]))
    for k, c in classes.items():
        if not k.endswith("/f32"):
            assert abs(c["signed"] / c["n"]) <= OB.BIAS_LIMIT, "%s %s: signed mean %.3f" % (name, k, c["signed"] / c["n"])
        lim = BEYOND_STEP.get((k.split("/")[0], dt))
        assert lim is not None or k.endswith("/f32"), "%s: no BEYOND_STEP entry for %s" % (name, (k.split("/")[0], dt))
        if lim is not None:
            assert c["beyond_max"] <= lim, "%s %s: %.3g of an op's elements beyond one step (limit %.3g)" % (name, k, c["beyond_max"], lim)
    eng.close()
