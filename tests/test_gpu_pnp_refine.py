"""Levenberg-Marquardt refinement of the RANSAC poses on the device (scpose_pnp_epnp_ransac_refine; csrc/pnp.hip lm_refine).

  1. refine_iters = 0 leaves every output bit-identical to scpose_pnp_epnp_ransac / _rows;
  2. the inlier mask is the point set of the final fit (popcount = status, a subset of the confidence filter, and the oracle's
     EPnP over exactly those points reproduces the unrefined pose);
  3. the kernel runs the algorithm of tests/pnp_lm_restated.py (1, 2 and 20 iterations pin the damping schedule);
  4. 20 iterations reach the least-squares optimum on the kernel's mask (tests/pnp_independent.py, SciPy);
  5. statuses and failure codes do not change, the 4- and 5-point branches are refined too, rotations stay orthonormal;
  6. a frame's refined row does not depend on the batch size or on its position in the batch;
  7. export_predicted_poses_real.py --pnp_refine lm writes the refined poses.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from oracle import pnp_ref as P
import pnp_independent as I
import pnp_lm_restated as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rot_dist(Ra, Rb):
    """Geodesic angle through the quaternion of Ra^T Rb (resolves 1e-12 rad; arccos of the trace stops near 1e-8)."""
    return float(Rotation.from_matrix(Ra.T @ Rb).magnitude())


def _dev(gpu_ops, kp, landmarks):
    return (torch.from_numpy(np.ascontiguousarray(kp)).cuda(), torch.from_numpy(landmarks).cuda(),
            torch.from_numpy(P.CAMERA_K).cuda(), torch.from_numpy(P.CAMERA_DIST).cuda())


def solve(gpu_ops, kp, landmarks=P.LANDMARKS, **kw):
    """Per-array form -> dict of NumPy arrays (R, t, status, rvec[, inliers])."""
    out = gpu_ops.pnp_epnp_ransac(*_dev(gpu_ops, kp, landmarks), want_rvec=True, **kw)
    keys = ("R", "t", "status", "rvec", "inliers")
    return {k: v.cpu().numpy() for k, v in zip(keys, out)}


def solve_rows(gpu_ops, kp, landmarks=P.LANDMARKS, **kw):
    rows = torch.full((kp.shape[0], 13), float("nan"), dtype=torch.float64, device="cuda")
    out = gpu_ops.pnp_epnp_ransac(*_dev(gpu_ops, kp, landmarks), rows=rows, **kw)
    if isinstance(out, tuple):
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def edge_frames(rng, landmarks=P.LANDMARKS):
    """Frames for every branch: < 4 points (-1), exactly 4 (P3P), exactly 5 (one EPnP), 6, all; pure clutter (-2 likely)."""
    j = len(landmarks)
    kp, _, _ = P.synth_keypoints(12, rng, 1.0, 0.0, landmarks=landmarks)
    kp[0, :, 2] = 0.0
    kp[1, 3:, 2] = 0.0
    kp[2, 4:, 2] = -1.0
    kp[3, 5:, 2] = 0.0
    kp[4, 6:, 2] = 1e-12
    kp[5, ::2, 2] = 0.0
    for i in range(6, 12):                              # clutter: no consistent pose
        kp[i, :, 0] = rng.uniform(0, 1920, j)
        kp[i, :, 1] = rng.uniform(0, 1200, j)
    return kp


def landmarks24(rng):
    return rng.uniform(-0.6, 0.6, (24, 3)) * np.array([1.0, 1.0, 0.4])


CASES = [(0.0, 0.0), (1.0, 0.0), (1.0, 0.1), (1.0, 0.3), (3.0, 0.1), (3.0, 0.3)]


@pytest.mark.parametrize("j", [11, 24])
def test_refine_off_is_bit_identical_to_the_existing_entries(gpu_ops, j):
    rng = np.random.default_rng(100 + j)
    lm = P.LANDMARKS if j == 11 else landmarks24(rng)
    kp = np.concatenate([P.synth_keypoints(48, rng, noise, out, landmarks=lm)[0] for noise, out in CASES] + [edge_frames(rng, lm)])
    base = solve(gpu_ops, kp, lm)
    base_rows = solve_rows(gpu_ops, kp, lm)
    assert {-1, 4, 5} <= set(base["status"].tolist())
    for want in (False, True):       # False: routed to the existing kernel; True: the refinement kernel with 0 iterations
        got = solve(gpu_ops, kp, lm, refine_iters=0, want_inliers=want)
        for k in ("R", "t", "status", "rvec"):
            assert np.array_equal(got[k], base[k]) and got[k].tobytes() == base[k].tobytes(), (want, k)
        rows = solve_rows(gpu_ops, kp, lm, refine_iters=0, want_inliers=want)
        rows = rows[0] if want else rows
        assert rows.tobytes() == base_rows.tobytes(), want


def test_inlier_mask_is_the_final_fit_point_set(gpu_ops):
    rng = np.random.default_rng(7)
    kp = np.concatenate([P.synth_keypoints(64, rng, noise, out)[0] for noise, out in CASES] + [edge_frames(rng)])
    kp[::5, 9, 2] = 1e-12                                # the confidence filter drops a point in some frames
    o = solve(gpu_ops, kp, want_inliers=True)
    st, inl = o["status"], o["inliers"]
    assert inl.shape == kp.shape[:2] and inl.dtype == bool
    assert np.array_equal(inl.sum(1)[st > 0], st[st > 0])
    assert not inl[st <= 0].any()
    worst_r = worst_t = 0.0
    for i in np.nonzero(st > 0)[0]:
        cm = P.conf_mask(kp[i, :, 2])
        assert not (inl[i] & ~cm).any(), i
        if cm.sum() <= 5:
            assert np.array_equal(inl[i], cm), i         # 4 (P3P) and 5 points: the whole filtered set
            continue
        rv, tv = P.epnp(P.LANDMARKS[inl[i]].astype(np.float32).astype(np.float64), kp[i, inl[i], :2].astype(np.float64))
        worst_r = max(worst_r, P.rot_angle(P.rodrigues(rv), o["R"][i]))
        worst_t = max(worst_t, np.linalg.norm(tv - o["t"][i]) / np.linalg.norm(o["t"][i]))
    assert worst_r <= 1e-4 and worst_t <= 1e-4, (worst_r, worst_t)


@pytest.mark.parametrize("iters", [1, 2, 20])
def test_kernel_runs_the_restated_algorithm(gpu_ops, iters):
    rng = np.random.default_rng(30 + iters)
    kp = np.concatenate([P.synth_keypoints(32, rng, noise, out)[0] for noise, out in CASES[1:]] + [edge_frames(rng)])
    base = solve(gpu_ops, kp, want_inliers=True)
    ref = solve(gpu_ops, kp, refine_iters=iters, want_inliers=True)
    assert np.array_equal(ref["inliers"], base["inliers"])
    worst_r = worst_t = 0.0
    for i in np.nonzero(base["status"] > 0)[0]:
        m = base["inliers"][i]
        r, t = L.refine(base["rvec"][i], base["t"][i], P.LANDMARKS[m], kp[i, m, :2], P.CAMERA_K, P.CAMERA_DIST, iters=iters)
        worst_r = max(worst_r, rot_dist(L.rodrigues(r), ref["R"][i]))
        worst_t = max(worst_t, np.linalg.norm(t - ref["t"][i]) / np.linalg.norm(t))
    print("refine_iters %d: kernel vs restatement %.2e rad, %.2e relative" % (iters, worst_r, worst_t))
    # 1 and 2 iterations: the same steps up to summation order (measured 2e-15).  At 20 the runs have converged, and where the
    # last step sits on the |d| <= FLT_EPSILON |p| threshold, rounding can stop one of the two an iteration earlier: they then
    # differ by what that sub-threshold step would still have moved (measured 1.7e-9 rad on one frame of 172).
    tol = 1e-9 if iters < 20 else 1e-8
    assert worst_r <= tol and worst_t <= tol, (worst_r, worst_t)


def _audit_on_mask(kp, R, t, masks, Rs, ts):
    X = P.LANDMARKS.astype(np.float32).astype(np.float64)
    out = {k: [] for k in ("ratio", "ang_ls", "t_ls", "ang_gt", "rms")}
    for i in range(len(kp)):
        m = masks[i]
        uv = kp[i, m, :2].astype(np.float64)
        Rl, tl = I.refine(R[i], t[i], X[m], uv, P.CAMERA_K, P.CAMERA_DIST)
        r = I.rms(R[i], t[i], X[m], uv, P.CAMERA_K, P.CAMERA_DIST)
        out["rms"].append(r)
        out["ratio"].append(r / max(I.rms(Rl, tl, X[m], uv, P.CAMERA_K, P.CAMERA_DIST), 1e-12))
        out["ang_ls"].append(rot_dist(R[i], Rl))
        out["t_ls"].append(np.linalg.norm(t[i] - tl) / np.linalg.norm(tl))
        out["ang_gt"].append(rot_dist(R[i], Rs[i]))
    return {k: np.array(v) for k, v in out.items()}


@pytest.mark.parametrize("outliers", [0.1, 0.3])
def test_twenty_iterations_reach_the_least_squares_optimum(gpu_ops, outliers):
    rng = np.random.default_rng(11)
    kp, Rs, ts = P.synth_keypoints(256, rng, 1.0, outliers)
    base = solve(gpu_ops, kp, want_inliers=True)
    ref = solve(gpu_ops, kp, refine_iters=20, want_inliers=True)
    assert (base["status"] > 0).all() and np.array_equal(ref["status"], base["status"])
    masks = base["inliers"]
    a0 = _audit_on_mask(kp, base["R"], base["t"], masks, Rs, ts)
    a1 = _audit_on_mask(kp, ref["R"], ref["t"], masks, Rs, ts)
    print(json.dumps({"outliers": outliers, "frames": len(kp),
                      "unrefined": {"rms_ratio_median": float(np.median(a0["ratio"])), "rms_ratio_max": float(a0["ratio"].max()),
                                    "ang_ls_median": float(np.median(a0["ang_ls"])), "ang_ls_max": float(a0["ang_ls"].max()),
                                    "ang_gt_median": float(np.median(a0["ang_gt"]))},
                      "refined": {"rms_ratio_median": float(np.median(a1["ratio"])), "rms_ratio_max": float(a1["ratio"].max()),
                                  "ang_ls_median": float(np.median(a1["ang_ls"])), "ang_ls_max": float(a1["ang_ls"].max()),
                                  "t_ls_max": float(a1["t_ls"].max()), "ang_gt_median": float(np.median(a1["ang_gt"]))}}))
    assert a1["ratio"].max() <= 1 + 1e-6, a1["ratio"].max()
    assert a1["ang_ls"].max() <= 1e-6, a1["ang_ls"].max()
    assert (a1["rms"] <= a0["rms"]).all()
    assert np.median(a1["ang_gt"]) <= np.median(a0["ang_gt"])


def test_noise_free_frames_refine_to_the_generating_pose(gpu_ops):
    rng = np.random.default_rng(12)
    kp, Rs, ts = P.synth_keypoints(128, rng, 0.0, 0.0)
    o = solve(gpu_ops, kp, refine_iters=20)
    assert (o["status"] == 11).all()
    ang = max(rot_dist(o["R"][i], Rs[i]) for i in range(len(kp)))
    terr = (np.linalg.norm(o["t"] - ts, axis=1) / np.linalg.norm(ts, axis=1)).max()
    assert ang <= 1e-6 and terr <= 1e-6, (ang, terr)


def test_failures_and_small_point_sets(gpu_ops):
    rng = np.random.default_rng(21)
    kp = np.concatenate([edge_frames(rng) for _ in range(8)])
    base = solve(gpu_ops, kp, want_inliers=True)
    ref = solve(gpu_ops, kp, refine_iters=20, want_inliers=True)
    assert np.array_equal(ref["status"], base["status"])
    fail = base["status"] <= 0
    assert fail.any() and np.array_equal(ref["R"][fail], base["R"][fail]) and np.array_equal(ref["t"][fail], base["t"][fail])
    small = np.isin(base["status"], (4, 5))
    assert small.sum() >= 8
    X = P.LANDMARKS.astype(np.float32).astype(np.float64)
    for i in np.nonzero(small)[0]:
        m = base["inliers"][i]
        uv = kp[i, m, :2].astype(np.float32).astype(np.float64)
        c0 = L.cost(np.concatenate([base["rvec"][i], base["t"][i]]), X[m], uv, P.CAMERA_K, P.CAMERA_DIST)
        c1 = L.cost(np.concatenate([ref["rvec"][i], ref["t"][i]]), X[m], uv, P.CAMERA_K, P.CAMERA_DIST)
        assert c1 <= c0 * (1 + 1e-12), (i, c0, c1)
    ok = ref["status"] > 0
    eye = np.einsum("nij,nkj->nik", ref["R"][ok], ref["R"][ok])
    assert np.abs(eye - np.eye(3)).max() < 1e-12


def test_refined_rows_do_not_depend_on_the_batch(gpu_ops):
    rng = np.random.default_rng(33)
    kp = np.concatenate([P.synth_keypoints(40, rng, noise, out)[0] for noise, out in CASES] + [edge_frames(rng)] * 2)[:256]
    r256, m256 = solve_rows(gpu_ops, kp, refine_iters=20, want_inliers=True)
    perm = np.random.default_rng(1).permutation(2048)
    big = np.tile(kp, (8, 1, 1))[perm]
    r2048, m2048 = solve_rows(gpu_ops, big, refine_iters=20, want_inliers=True)
    src = perm % 256
    assert r2048.tobytes() == r256[src].tobytes() and np.array_equal(m2048, m256[src])
    for i in range(0, 256, 37):
        r1 = solve_rows(gpu_ops, kp[i:i + 1], refine_iters=20)
        assert r1.tobytes() == r256[i:i + 1].tobytes(), i


def test_cli_pnp_refine_lm_writes_the_refined_poses(gpu_ops, tmp_path):
    from scipy.io import savemat
    kp, _, _ = P.synth_keypoints(6, np.random.default_rng(4), 1.0, 0.1)
    savemat(tmp_path / "kp.mat", {"preds": kp})
    (tmp_path / "landmarks.csv").write_text("x,y,z\n" + "\n".join(",".join(repr(float(v)) for v in r) for r in P.LANDMARKS))
    (tmp_path / "calib.json").write_text(json.dumps({"intrinsics": {"camera_matrix": P.CAMERA_K.tolist(),
                                                                    "distortion_coefficients": P.CAMERA_DIST.tolist()}}))
    images = [{"id": i + 1, "file_name": "frame_%03d.png" % i, "width": 1920, "height": 1200} for i in range(6)]
    anns = [{"image_id": i + 1, "bbox": [10, 10, 100, 100], "id": i, "category_id": 1} for i in range(6)]
    (tmp_path / "det.json").write_text(json.dumps({"images": images, "annotations": anns}))
    (tmp_path / "frames").mkdir()
    cmd = [sys.executable, "export_predicted_poses_real.py", "--frames_dir", str(tmp_path / "frames"),
           "--detection_annotations", str(tmp_path / "det.json"), "--pose_annotations", str(tmp_path / "kp.mat"),
           "--landmarks_file", str(tmp_path / "landmarks.csv"), "--calibration_file_path", str(tmp_path / "calib.json"),
           "--output_dir", str(tmp_path / "poses"), "--no_overlay", "--pnp_refine", "lm"]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "pose_estimation"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    poses = json.load(open(tmp_path / "poses" / "opencv_poses.json"))
    ref = solve(gpu_ops, kp, refine_iters=20)
    plain = solve(gpu_ops, kp)
    assert [p["image_name"] for p in poses] == [im["file_name"] for im in images]
    for i, p in enumerate(poses):
        assert np.array_equal(np.array(p["rotation_matrix"]), ref["R"][i])
        assert np.array_equal(np.array(p["T"]).ravel(), ref["t"][i])
    assert any(not np.array_equal(ref["R"][i], plain["R"][i]) for i in range(6))     # the flag did change the poses
