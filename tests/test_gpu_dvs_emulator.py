"""DVS emulator on the device (csrc/dvs_emulator.hip through ops.dvs_emulator and the C ABI) against the torch-CPU restatement
and the reference's recorded rows, bit for bit in every column, the event count and the final state; chunking, determinism,
reset, capacity overflow behind a guard pattern, the rejections, the chain into the event renderer and the v2e command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dvs_emulator_restated as R
import event_render_restated as ER

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "dvs_emulator_reference.npz")
SHAPES = ((24, 40), (5, 37))             # 40 x 24: no multiple of the 64-pixel tile, every row crosses one; 37 x 5: odd, partial tile
CASES = ("scalar", "perpixel", "cutoff", "leak", "refractory", "repeat", "step", "all")
_restated = {}


def restated(h, w, name):
    """(columns, state, num_iters) of the restatement, computed once per case."""
    key = (h, w, name)
    if key not in _restated:
        case = R.make_cases(h, w)[name]
        e = R.RestatedEmulator(**R.case_params(case))
        rows = e.emulate(case["frames"], case["t"])
        _restated[key] = (R.columns(rows), e.state(), list(e.num_iters))
    return _restated[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_device(ops, case, h, w, chunks=None, emu=None):
    emu = emu or ops.dvs_emulator(h, w, **R.case_params(case))
    frames, t = case["frames"], np.asarray(case["t"], np.float64)
    parts, s = [], 0
    for c in (chunks or [len(frames)]):
        parts.append(emu.emulate(frames[s:s + c], t[s:s + c]))
        s += c
    assert s == len(frames)
    cols = tuple(torch.cat([p[j] for p in parts]).cpu().numpy() for j in range(5))
    return cols, {k: v.cpu().numpy() for k, v in emu.state().items()}, emu


def assert_same(cols, ref_cols, what):
    assert len(cols[0]) == len(ref_cols[0]), "%s: %d events, expected %d" % (what, len(cols[0]), len(ref_cols[0]))
    for name, a, b in zip(("t", "x", "y", "p", "t_s"), cols, ref_cols):
        assert a.dtype == b.dtype, (what, name, a.dtype, b.dtype)
        assert np.array_equal(bits(a), bits(b)), "%s: column %s differs at %s" % (what, name, np.flatnonzero(bits(a) != bits(b))[:5])


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % (s[1], s[0]))
@pytest.mark.parametrize("name", CASES)
def test_device_equals_restatement(gpu_ops, name, hw):
    h, w = hw
    case = R.make_cases(h, w)[name]
    ref_cols, ref_state, iters = restated(h, w, name)
    cols, state, _ = run_device(gpu_ops, case, h, w)
    assert_same(cols, ref_cols, name)
    for k in ("base", "lp0", "lp1", "tmem"):
        assert np.array_equal(bits(state[k]), bits(ref_state[k])), "%s: state %s differs" % (name, k)
    # the cases hold what their names promise
    if name == "repeat":
        assert iters.count(0) == 2
    if name == "step":
        assert max(iters) == 27 and len(cols[0]) == 27 and (cols[3] == 1).all()
    if name == "refractory":
        case_t = np.asarray(case["t"])
        steps = [np.float32(np.float32(1.0) / np.float32(n)) * np.float32(case_t[k + 1] - case_t[k]) for k, n in enumerate(iters) if n]
        active = [bool(np.float32(0.01) > s) for s in steps]
        assert any(active) and not all(active)
    if name == "perpixel":
        assert float(np.min(case["pos_thres"])) == np.float32(0.01)


SCAN_TILE = 4096                         # table entries per workgroup of the device-wide scan (csrc/scan_device.h)
SCAN_SHAPES = {"two_scan_blocks": (16, 16, 1), "carry_loop": (240, 256, 256)}     # h, w, scan blocks the longest table must exceed


def scan_case(h, w, f=3):
    """A moving background at threshold 0.2 and one pixel at pos_thres 0.01 that steps 0 -> 255 in frame 1: that frame needs
    ln(255) / 0.01 sub-iterations while the events stay few; in frame 2 the pixel rests and the table is short again."""
    frames = R.moving_frames(8, f, h, w)
    y, x = h // 2, w // 3
    frames[0, y, x] = 0
    frames[1:, y, x] = 255
    pos = np.full((h, w), 0.2, np.float32)
    pos[y, x] = 0.01
    return dict(frames=frames, t=0.5 + 0.01 * np.arange(f), pos_thres=pos, neg_thres=0.2)


@pytest.mark.parametrize("name", sorted(SCAN_SHAPES))
def test_scan_past_one_block_equals_restatement(gpu_ops, name):
    """The scanned table has 2 * num_iters * ceil(h * w / 64) entries.  two_scan_blocks: more than one scan tile, the last one
    partial (the aggregate pass).  carry_loop: more than 256 scan tiles (the carry loop of the one-workgroup middle pass), followed
    by a frame with a shorter table (blocks past the device-side length return early, over aggregates the long frame left)."""
    h, w, blocks = SCAN_SHAPES[name]
    case = scan_case(h, w)
    e = R.RestatedEmulator(**R.case_params(case))
    ref_cols = R.columns(e.emulate(case["frames"], case["t"]))
    ref_state = e.state()
    tiles = (h * w + 63) // 64
    lens = [2 * n * tiles for n in e.num_iters]
    assert max(e.num_iters) <= 1024                                  # max_iters stays at its default
    assert max(lens) > blocks * SCAN_TILE, (e.num_iters, tiles)
    if name == "two_scan_blocks":
        assert max(lens) % SCAN_TILE != 0
    else:
        assert lens.index(max(lens)) < len(lens) - 1 and lens[-1] < max(lens), lens
    cols, state, _ = run_device(gpu_ops, case, h, w)
    assert_same(cols, ref_cols, name)
    for k in ("base", "lp0", "lp1", "tmem"):
        assert np.array_equal(bits(state[k]), bits(ref_state[k])), "%s: state %s differs" % (name, k)


def test_device_equals_reference_rows(gpu_ops):
    g = np.load(GOLDEN)
    for name in g["cases"]:
        kw = {k: g[name + "_" + k] for k in R.PARAM_KEYS if name + "_" + k in g.files}
        kw = {k: (float(v) if v.ndim == 0 else v) for k, v in kw.items()}
        frames = g[name + "_frames"]
        emu = gpu_ops.dvs_emulator(frames.shape[1], frames.shape[2], **kw)
        out = emu.emulate(frames, g[name + "_t"])
        assert_same(tuple(c.cpu().numpy() for c in out), R.columns(g[name + "_rows"]), name)
        state = emu.state()
        for k in ("base", "lp0", "lp1", "tmem"):
            if name + "_" + k in g.files:
                assert np.array_equal(bits(state[k].cpu().numpy()), bits(g[name + "_" + k])), (name, k)


def test_chunks_runs_and_reset(gpu_ops):
    h, w = SHAPES[0]
    case = R.make_cases(h, w)["all"]
    one, state_one, emu = run_device(gpu_ops, case, h, w)
    chunked, state_chunked, _ = run_device(gpu_ops, case, h, w, chunks=[3, 1, len(case["frames"]) - 4])
    assert_same(chunked, one, "3 + 1 + rest")
    again, state_again, _ = run_device(gpu_ops, case, h, w)
    assert_same(again, one, "second run")
    emu.reset()
    after_reset, state_reset, _ = run_device(gpu_ops, case, h, w, emu=emu)
    assert_same(after_reset, one, "after reset")
    for st in (state_chunked, state_again, state_reset):
        for k in state_one:
            assert np.array_equal(bits(st[k]), bits(state_one[k])), k
    assert_same(one, restated(h, w, "all")[0], "all")


def test_inputs_on_the_device_and_empty_calls(gpu_ops):
    h, w = SHAPES[1]
    case = R.make_cases(h, w)["scalar"]
    emu = gpu_ops.dvs_emulator(h, w, **R.case_params(case))
    fr = torch.from_numpy(case["frames"]).cuda(); t = torch.from_numpy(np.asarray(case["t"], np.float64)).cuda()
    first = emu.emulate(fr[:1], t[:1])                               # frame 0 only initialises
    assert all(c.numel() == 0 for c in first)
    rest = emu.emulate(fr[1:], t[1:])
    assert rest[0].is_cuda and [c.dtype for c in rest] == [torch.int64, torch.int32, torch.int32, torch.int8, torch.float32]
    assert_same(tuple(c.cpu().numpy() for c in rest), restated(h, w, "scalar")[0], "device inputs")


def test_capacity_overflow_is_a_status_and_writes_nothing_past_the_end(gpu_ops):
    h, w = SHAPES[0]
    case = R.make_cases(h, w)["scalar"]
    ref = restated(h, w, "scalar")[0]
    n = len(ref[0])
    cap = n // 3
    emu = gpu_ops.dvs_emulator(h, w, **R.case_params(case))
    emu.emulate(case["frames"][:1], case["t"][:1])
    nat, lib = gpu_ops.nat, gpu_ops.nat.lib()
    guard = 64
    dts = (torch.float32, torch.int64, torch.int32, torch.int32, torch.int8)
    cols = [torch.full((cap + guard,), 0x5A if dt == torch.int8 else 0x5A5A5A5A, dtype=torch.int64, device="cuda").to(dt) for dt in dts]
    before = [c.clone() for c in cols]
    fr = torch.from_numpy(case["frames"][1:]).cuda(); t = torch.from_numpy(np.asarray(case["t"][1:], np.float64)).cuda()
    f = fr.shape[0]
    ws = ctypes.c_size_t()
    nat.check(lib.scpose_dvs_workspace_bytes(h, w, f, 1024, ctypes.byref(ws)))
    work = torch.empty(ws.value, dtype=torch.uint8, device="cuda")
    cs = torch.empty(2, dtype=torch.int64, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    nat.check(lib.scpose_dvs_emulate(p(emu._state), p(fr), p(t), f, ctypes.byref(emu._c), p(cols[0]), p(cols[1]), p(cols[2]), p(cols[3]),
                                     p(cols[4]), cap, p(cs), p(work), ws.value, None))
    torch.cuda.synchronize()
    count, status = cs.tolist()
    assert count == n and status == nat.DVS_CAPACITY
    order = (4, 0, 1, 2, 3)                                          # the buffers are (t_s, t, x, y, p), the reference columns (t, x, y, p, t_s)
    for c, b, j in zip(cols, before, order):
        assert torch.equal(c[cap:], b[cap:]), "rows past the capacity were written"
        assert np.array_equal(bits(c[:cap].cpu().numpy()), bits(ref[j][:cap]))
    # the wrapper: a fixed capacity raises with the full count, the default one grows and succeeds
    emu2 = gpu_ops.dvs_emulator(h, w, **R.case_params(case))
    with pytest.raises(gpu_ops.DvsCapacity) as ei:
        emu2.emulate(case["frames"], case["t"], capacity=cap)
    assert ei.value.n_events == n
    emu2.reset(); emu2._per_frame = 1e-6
    assert_same(tuple(c.cpu().numpy() for c in emu2.emulate(case["frames"], case["t"])), ref, "grown capacity")


def test_too_many_sub_iterations_is_a_status(gpu_ops):
    h, w = SHAPES[1]
    case = R.make_cases(h, w)["step"]                                # 27 sub-iterations in one frame
    emu = gpu_ops.dvs_emulator(h, w, max_iters=26, **R.case_params(case))
    with pytest.raises(gpu_ops.nat.NativeError, match="max_iters"):
        emu.emulate(case["frames"], case["t"])
    assert emu.last_status & gpu_ops.nat.DVS_ITERS
    emu = gpu_ops.dvs_emulator(h, w, max_iters=27, **R.case_params(case))
    assert emu.emulate(case["frames"], case["t"])[0].numel() == 27


def test_rejections(gpu_ops):
    h, w = SHAPES[1]
    with pytest.raises(ValueError, match="shot_noise_rate_hz"):
        gpu_ops.dvs_emulator(h, w, shot_noise_rate_hz=5.0)
    with pytest.raises(ValueError, match="leak_jitter_fraction"):
        gpu_ops.dvs_emulator(h, w, leak_jitter_fraction=0.1)
    case = R.make_cases(h, w)["scalar"]
    emu = gpu_ops.dvs_emulator(h, w)
    t = np.asarray(case["t"], np.float64).copy(); t[3] = t[2]
    with pytest.raises(ValueError, match="must be later"):
        emu.emulate(case["frames"], t)
    emu.emulate(case["frames"][:2], case["t"][:2])
    with pytest.raises(ValueError, match="must be later"):          # against the state's time, across calls
        emu.emulate(case["frames"][2:3], case["t"][1:2])
    with pytest.raises(ValueError, match="frames must be uint8"):
        emu.emulate(case["frames"].astype(np.float32), case["t"])
    # the C ABI checks the stamps on the device as well
    nat, lib = gpu_ops.nat, gpu_ops.nat.lib()
    fr = torch.from_numpy(case["frames"][2:4]).cuda(); td = torch.tensor([float(case["t"][2]), float(case["t"][2])], dtype=torch.float64).cuda()
    ws = ctypes.c_size_t(); nat.check(lib.scpose_dvs_workspace_bytes(h, w, 2, 1024, ctypes.byref(ws)))
    work = torch.empty(ws.value, dtype=torch.uint8, device="cuda"); cs = torch.empty(2, dtype=torch.int64, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    nat.check(lib.scpose_dvs_emulate(p(emu._state), p(fr), p(td), 2, ctypes.byref(emu._c), None, None, None, None, None, 0, p(cs), p(work),
                                     ws.value, None))
    assert cs.tolist()[1] & nat.DVS_TIME


def test_chain_into_the_event_renderer(gpu_ops):
    h, w = SHAPES[0]
    case = R.make_cases(h, w)["scalar"]
    emu = gpu_ops.dvs_emulator(h, w, **R.case_params(case))
    t, x, y, p, _ = emu.emulate(case["frames"], case["t"])
    rt, rx, ry, rp, _ = restated(h, w, "scalar")[0]
    for fold in (True, False):
        d, names = gpu_ops.render_events(t, x, y, p, (h, w), interval=10000.0, full_scale=2, fold_polarity=fold)
        frames, ref_names = ER.render(rt, rx, ry, rp, (h, w), interval=10000.0, fs=2, fold_polarity=fold)
        assert names == ref_names and len(names) >= 4
        assert np.array_equal(d["flat"].view(-1, h, w, 3).cpu().numpy(), frames)


def test_v2e_command_line(gpu_ops, tmp_path):
    from PIL import Image
    h, w = SHAPES[1]
    frames = R.moving_frames(11, 5, h, w)
    src = tmp_path / "in"; src.mkdir()
    for k, f in enumerate(frames):
        if k == 2:
            Image.fromarray(np.repeat(f[..., None], 3, 2)).save(src / ("%03d.png" % k))     # an RGB file with equal channels
        else:
            Image.fromarray(f).save(src / ("%03d.bmp" % k if k % 2 else "%03d.png" % k))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "v2e", "v2e.py"), "--input", str(src), "--input_frame_rate", "100", "--dvs_params", "clean",
           "--sigma_thres", "0", "--output_folder", str(out), "--dvs_text", "events"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # 'clean' sets sigma_thres = 0.02: the thresholds are drawn (unseeded), so compare against the stream's own invariants ...
    t, x, y, p = gpu_ops.parse_events_csv(str(out / "events.txt"), delim_whitespace=True)
    assert t.numel() > 0 and bool((t[1:] >= t[:-1]).all()) and int(x.max()) < w and int(y.max()) < h and set(p.unique().tolist()) <= {0, 1}
    # ... and with scalar thresholds against the restatement
    cmd2 = [c for c in cmd if c not in ("--dvs_params", "clean")]
    r = subprocess.run(cmd2, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = tuple(c.cpu().numpy() for c in gpu_ops.parse_events_csv(str(out / "events.txt"), delim_whitespace=True))
    ref = R.columns(R.RestatedEmulator(0.2, 0.2).emulate(frames, np.arange(5) / 100.0))
    for a, b in zip(got, ref[:4]):
        assert np.array_equal(a, b)
    r = subprocess.run(cmd + ["--dvs_h5", "x.h5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--dvs_h5" in r.stderr
