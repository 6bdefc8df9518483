"""Stereo rectification without a GPU: the specification tests/rectify_ref.py pinned to the ingest
oracle and to a direct evaluation of the camera model, rectify.stereo_rectify's geometry, the
reason the feature exists (SGBM on a 1.9 degree rig with and without rectification), the tile-path
facts the GPU tests rely on, the golden vector and the argument checks of csrc/capi_rectify.cpp
under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import rectify_ref as ref
import rectify_scene as scene
from conftest import GOLDEN, ROOT

RIGS = {"x4": scene.rig, "vertical": scene.vertical_rig, "translation": scene.translation_rig}


def _rectify(rig, **kw):
    from forest_slam_amd.rectify import stereo_rectify
    Kl, dl, Kr, dr, R, T = rig
    return stereo_rectify(Kl, dl, Kr, dr, (scene.W, scene.H), R, T, **kw)


# ------------------------------------------------------------------ the specification is pinned
@pytest.mark.parametrize("W,H", [(64, 64), (96, 40)])
def test_spec_equals_ingest_oracle_at_single_stripe_sizes(oracle_mod, W, H):
    """R = I, newK = K, 5 coefficients, 4096 // W >= H (cv2.undistort has one stripe there):
    the map and the gray image equal oracle/ingest_ref.cpp bit for bit."""
    assert 4096 // W >= H
    Kl, dl, Kr, dr, _, _ = scene.rig()
    for K, d in ((Kl, dl), (Kr, dr), (Kl, np.array([-0.3, 0.12, 1e-3, -2e-3, 0.01]))):
        mxy, fr = oracle_mod.undistort_map(H, W, K, d)
        for R, newK in ((None, None), (np.eye(3), K)):
            m1, m2 = ref.rectify_map(K, d, R, newK, W, H)
            assert np.array_equal(mxy, m1) and np.array_equal(fr, m2)
        bgr = np.random.default_rng(W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert np.array_equal(oracle_mod.undistort_gray(bgr, K, d), ref.rectify_gray(bgr, K, d, None, None))


def test_spec_map_matches_camera_model_with_rotation_and_rational_distortion():
    """An independent float64 evaluation (matrix inverse, the model written from its definition)
    at a non-trivial R with 8 coefficients; tolerance 1/64 px as tests/test_ingest.py."""
    W, H = 200, 120
    Kl, _, _, _, _, _ = scene.rig()
    d = np.array([-0.21, 0.09, 1.2e-3, -0.8e-3, -0.02, 0.11, -0.03, 0.004])
    R = scene.rodrigues(np.array([0.03, -0.05, 0.08]))
    newK = np.array([[190.0, 0, 101.5], [0, 188.0, 58.25], [0, 0, 1]])
    m1, m2 = ref.rectify_map(Kl, d, R, newK, W, H)
    u_s = m1[..., 0] + (m2 & 31) / 32.0
    v_s = m1[..., 1] + (m2 >> 5) / 32.0
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.einsum("ij,jhw->ihw", np.linalg.inv(newK @ R), np.stack([x, y, np.ones_like(x)]))
    xn, yn = ray[0] / ray[2], ray[1] / ray[2]
    r2 = xn ** 2 + yn ** 2
    rad = (1 + d[0] * r2 + d[1] * r2 ** 2 + d[4] * r2 ** 3) / (1 + d[5] * r2 + d[6] * r2 ** 2 + d[7] * r2 ** 3)
    u = Kl[0, 0] * (xn * rad + 2 * d[2] * xn * yn + d[3] * (r2 + 2 * xn ** 2)) + Kl[0, 2]
    v = Kl[1, 1] * (yn * rad + d[2] * (r2 + 2 * yn ** 2) + 2 * d[3] * xn * yn) + Kl[1, 2]
    assert np.abs(u_s - u).max() <= 1 / 64 + 1e-9 and np.abs(v_s - v).max() <= 1 / 64 + 1e-9
    # with 4 or 5 coefficients the denominator is exactly 1
    assert all(np.array_equal(a, b) for a, b in zip(ref.rectify_map(Kl, d[:4], R, newK, W, H),
                                                    ref.rectify_map(Kl, np.r_[d[:4], 0.0], R, newK, W, H)))


def test_spec_remap_border_and_frac_mask():
    img = np.random.default_rng(0).integers(1, 256, (5, 7), dtype=np.uint8)
    map1 = np.zeros((5, 7, 2), np.int16)
    map1[..., 0], map1[..., 1] = np.arange(7)[None, :], np.arange(5)[:, None]
    assert np.array_equal(ref.remap(img, map1, np.zeros((5, 7), np.uint16)), img)
    assert np.array_equal(ref.remap(img, map1, np.full((5, 7), 1024, np.uint16)), img)  # map2 & 1023
    far = map1.copy()
    far[..., 0] = 7  # wholly outside
    assert not ref.remap(img, far, np.zeros((5, 7), np.uint16)).any()
    edge = map1.copy()
    edge[..., 0] = -1  # x taps -1 (outside, 0) and 0, half each
    got = ref.remap(img, edge, np.full((5, 7), 16, np.uint16))
    assert np.array_equal(got, np.repeat(((img[:, :1].astype(int) * 16 * 32 * 32 + (1 << 14)) >> 15), 7, 1))


# ------------------------------------------------------------------ stereo_rectify
@pytest.mark.parametrize("name", list(RIGS))
def test_stereo_rectify_geometry(name):
    rig = RIGS[name]()
    Kl, dl, Kr, dr, R, T = rig
    r = _rectify(rig)
    idx = r.idx
    assert idx == (1 if name == "vertical" else 0)
    for M in (r.R1, r.R2):
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(M) - 1) < 1e-12
    assert np.abs(r.R2 @ R - r.R1).max() < 1e-12
    t = r.R2 @ T
    assert abs(abs(t[idx]) - np.linalg.norm(T)) < 1e-12 and np.abs(np.delete(t, idx)).max() < 1e-12
    assert abs(r.baseline - np.linalg.norm(T)) < 1e-12
    assert np.array_equal(r.K_rect, r.P1[:, :3]) and r.P1[0, 0] == r.P1[1, 1] == r.P2[0, 0] == r.P2[1, 1]
    # 200 points in front of both cameras
    rng = np.random.default_rng(7)
    X = rng.uniform([-2, -1.2, 2], [2, 1.2, 6], (200, 3)).T
    Xl, Xr = r.R1 @ X, r.R2 @ (R @ X + T[:, None])
    a = (r.P1[:, :3] @ Xl + r.P1[:, 3:]); a = a[:2] / a[2]
    b = r.P2[:, :3] @ Xr; b = b[:2] / b[2]                        # the right camera's own geometry
    b1 = (r.P2[:, :3] @ Xl + r.P2[:, 3:]); b1 = b1[:2] / b1[2]    # P2 takes rectified-left points
    assert np.abs(b - b1).max() < 1e-9
    assert np.abs(a[idx ^ 1] - b[idx ^ 1]).max() < 1e-9          # the shared image coordinate
    f = r.P1[0, 0]
    disp = a[idx] - b[idx]
    want = f * r.baseline / Xl[2] * (1 if r.P2[idx, 3] < 0 else -1)
    assert np.abs(disp / want - 1).max() < 1e-9
    # Q takes (u, v, d, 1) back to the rectified-left point; the same evaluation as
    # tests/dense_ref.py's reprojection (h_k / h_3)
    h = r.Q @ np.stack([a[0], a[1], disp, np.ones(200)])
    assert np.abs(h[:3] / h[3] / Xl - 1).max() < 1e-9
    import dense_ref
    d = 12.5 * (1 if disp[0] > 0 else -1)
    pts = dense_ref.reproject(np.full((scene.H, scene.W), d, np.float32), r.Q).astype(np.float64)
    for v, u in ((0, 0), (37, 211), (scene.H - 1, scene.W - 1)):
        Xp = pts[v, u]
        pa = r.P1[:, :3] @ Xp + r.P1[:, 3]
        pb = r.P2[:, :3] @ Xp + r.P2[:, 3]
        want_b = np.array([u, v], np.float64)
        want_b[idx] -= d
        assert np.abs(pa[:2] / pa[2] - [u, v]).max() < 1e-3 and np.abs(pb[:2] / pb[2] - want_b).max() < 1e-3


@pytest.mark.parametrize("name", list(RIGS))
def test_stereo_rectify_principal_points_alpha_and_rois(name):
    from forest_slam_amd.rectify import CALIB_ZERO_DISPARITY
    rig = RIGS[name]()
    Kl, dl, Kr, dr, R, T = rig
    z = _rectify(rig, flags=CALIB_ZERO_DISPARITY)
    assert np.array_equal(z.P1[:2, 2], z.P2[:2, 2])
    n = _rectify(rig, flags=0)
    assert n.P1[n.idx ^ 1, 2] == n.P2[n.idx ^ 1, 2]
    if name != "translation":
        assert n.P1[n.idx, 2] != n.P2[n.idx, 2]
    W, H = scene.W, scene.H
    a0, a1 = _rectify(rig, alpha=0.0), _rectify(rig, alpha=1.0)
    for K, d, Rk, P in ((Kl, dl, a0.R1, a0.P1), (Kr, dr, a0.R2, a0.P2)):  # alpha 0: only valid pixels
        m1, _ = ref.rectify_map(K, d, Rk, P[:, :3], W, H)
        assert m1[..., 0].min() >= 0 and m1[..., 0].max() <= W - 1
        assert m1[..., 1].min() >= 0 and m1[..., 1].max() <= H - 1
    # alpha 0 scales the inscribed rectangle of the pixel-centre grid until it covers the output's
    # pixel centres [0, W-1] x [0, H-1]; the ROI is ceil(corner), floor(size) of it, so it starts at 0
    # and spans at least W-1 x H-1 (one less where the product lands an ulp under the integer)
    for x, y, w, h in (a0.roi1, a0.roi2):
        assert (x, y) == (0, 0) and W - 2 <= w <= W and H - 2 <= h <= H
    cu, cv = np.array([0.0, W - 1, 0, W - 1]), np.array([0.0, 0, H - 1, H - 1])
    for K, d, Rk, P in ((Kl, dl, a1.R1, a1.P1), (Kr, dr, a1.R2, a1.P2)):  # alpha 1: every source pixel kept
        x, y = scene.undistort_points(cu, cv, K, d)
        q = P[:, :3] @ (Rk @ np.stack([x, y, np.ones(4)]))
        u, v = q[0] / q[2], q[1] / q[2]
        assert u.min() >= 0 and u.max() <= W - 1 and v.min() >= 0 and v.max() <= H - 1
    assert a0.P1[0, 0] > a1.P1[0, 0]
    for roi in (a1.roi1, a1.roi2, _rectify(rig).roi1):
        x, y, w, h = roi
        assert 0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= W and y + h <= H


def test_stereo_rectify_refuses_what_it_does_not_restate():
    rig = scene.rig()
    for kw in ({"flags": 2}, {"alpha": 1.5}, {"alpha": -0.5}, {"newImageSize": (320, 200)}):
        with pytest.raises(NotImplementedError):
            _rectify(rig, **kw)
    from forest_slam_amd.rectify import stereo_rectify
    Kl, dl, Kr, dr, R, T = rig
    for bad in (dict(d1=np.zeros(14)), dict(T=np.zeros(3)), dict(K1=np.eye(4)), dict(size=(0, 200)),
                dict(R=np.diag([1.0, -1.0, -1.0]))):
        a = dict(K1=Kl, d1=dl, K2=Kr, d2=dr, size=(320, 200), R=R, T=T)
        a.update(bad)
        with pytest.raises(NotImplementedError):
            stereo_rectify(a["K1"], a["d1"], a["K2"], a["d2"], a["size"], a["R"], a["T"])


def test_stereo_rectify_matches_opencv():
    """Version-independent outputs only: the rotations, the baseline term and fx == fy (fc_new and
    the principal points differ between OpenCV releases, rectify.py's docstring)."""
    cv2 = pytest.importorskip("cv2")
    for name, make in RIGS.items():
        Kl, dl, Kr, dr, R, T = make()
        r = _rectify((Kl, dl, Kr, dr, R, T))
        R1, R2, P1, P2, Q, _, _ = cv2.stereoRectify(Kl, dl, Kr, dr, (scene.W, scene.H), R, T,
                                                    flags=cv2.CALIB_ZERO_DISPARITY, alpha=-1)
        assert np.abs(R1 - r.R1).max() < 1e-9 and np.abs(R2 - r.R2).max() < 1e-9, name
        assert abs(P2[r.idx, 3] / P2[0, 0] - r.P2[r.idx, 3] / r.P2[0, 0]) < 1e-9
        assert P1[0, 0] == P1[1, 1]


def test_run_stereo_bag_refuses_rigs_that_cannot_go_on_to_sgbm(tmp_path):
    """A vertical rig, and a horizontal one given in right, left order (negative disparities), are
    refused before anything runs on a device."""
    from forest_slam_amd import pipeline as pl
    from forest_slam_amd import rosbag as rb
    path = str(tmp_path / "two.bag")
    with rb.BagWriter(path) as w:
        for i in range(2):
            img = np.zeros((scene.H, scene.W), np.uint8)
            w.write(pl.LEFT, rb.image_message(img, rb.Time(10 + i, 0), encoding="mono8"), rb.Time(10 + i, 0))
            w.write(pl.RIGHT, rb.image_message(img, rb.Time(10 + i, 5), encoding="mono8"), rb.Time(10 + i, 5))
    Kl, dl, Kr, dr, R, T = scene.rig()
    swapped = (R.T, -R.T @ T)  # x_left = R^T x_right - R^T T
    for rig_rt, (Ka, da, Kb, db) in ((swapped, (Kr, dr, Kl, dl)), (scene.vertical_rig()[4:], (Kl, dl, Kr, dr))):
        with pytest.raises(ValueError):
            pl.run_stereo_bag(path, K_left=Ka, dist_left=da, K_right=Kb, dist_right=db, rectify=rig_rt)


# ------------------------------------------------------------------ why the feature exists
def test_rectification_rescues_sgbm_on_a_two_degree_rig(oracle_mod):
    """The x4 rig (1.9 degrees), a textured plane at 2.7 m, 320 x 200, D = 64: share of pixels whose
    oracle SGBM disparity is within 1 px of the geometric truth.  Undistort-only (today's path):
    measured 0.0210; specification-rectified: measured 0.9943 (seeds 1..3: 0.9937, 0.9948,
    0.9948).  Floor = the measured value - 0.02 (re-seeding the texture)."""
    rig = scene.rig()
    Kl, dl, Kr, dr, R, T = rig
    rawL, rawR = scene.Scene(0).stereo_pair(*rig)
    und = oracle_mod.sgbm(ref.rectify_gray(rawL, Kl, dl, None, None), ref.rectify_gray(rawR, Kr, dr, None, None),
                          num_disp=scene.D)
    truth, voff = scene.truth_unrectified(Kl, Kr, R, T)
    reg = scene.region()[0]
    assert voff[reg].max() < -3.0 and voff[reg].min() > -7.7  # the table's -7.6 .. -3.1 px
    share_und = scene.share_within_1px(und, truth)
    r = _rectify(rig)
    rec = oracle_mod.sgbm(ref.rectify_gray(rawL, Kl, dl, r.R1, r.P1[:, :3]),
                          ref.rectify_gray(rawR, Kr, dr, r.R2, r.P2[:, :3]), num_disp=scene.D)
    share_rec = scene.share_within_1px(rec, scene.truth_rectified(r.R1, r.P1, r.baseline))
    print(f"share within 1 px: undistort only {share_und:.4f}, rectified {share_rec:.4f}")
    assert share_und < 0.5
    assert share_rec > 0.9943 - 0.02


# ------------------------------------------------------------------ tile paths
def test_tile_path_cases():
    """Facts tests/test_rectify_gpu.py relies on, from the specification's path rule."""
    tw, th, lds = ref.header_macros()
    assert (tw // 4) * th == 256 and lds % 4 == 0 and 4 * lds <= 160 * 1024
    from forest_slam_amd import _lib
    assert (tw, th, lds) == (_lib.RECTIFY_TILE_W, _lib.RECTIFY_TILE_H, _lib.RECTIFY_LDS_BYTES)
    r = _rectify(scene.rig())
    W, H = scene.W, scene.H
    K, d, R, newK = scene.lens_case("aligned", r)
    m1, _ = ref.rectify_map(K, d, R, newK, W, H)
    assert ref.tile_paths(m1, 1).all() and ref.tile_paths(m1, 3).all()
    assert not ref.tile_paths(m1, 3, budget=0).any()
    K, d, R, newK = scene.lens_case("rolled")
    m1, _ = ref.rectify_map(K, d, R, newK, W, H)
    p = ref.tile_paths(m1, 3)
    assert p.any() and not p.all()
    m1, _ = scene.scatter_map()
    assert not ref.tile_paths(m1, 1).any() and not ref.tile_paths(m1, 3).any()


# ------------------------------------------------------------------ golden
def test_golden_rectify_reproduces():
    g = np.load(os.path.join(GOLDEN, "golden_rectify.npz"))
    W, H = int(g["size"][0]), int(g["size"][1])
    from forest_slam_amd.rectify import stereo_rectify
    r = stereo_rectify(g["K1"], g["d1"], g["K2"], g["d2"], (W, H), g["R"], g["T"])
    assert np.allclose(r.R1, g["R1"], rtol=0, atol=1e-12) and np.allclose(r.P2, g["P2"], rtol=0, atol=1e-9)
    for k, (K, d, Rk, P) in enumerate(((g["K1"], g["d1"], g["R1"], g["P1"]), (g["K2"], g["d2"], g["R2"], g["P2"]))):
        m1, m2 = ref.rectify_map(K, d, Rk, P[:, :3], W, H)
        assert np.array_equal(m1, g[f"map1_{k}"]) and np.array_equal(m2, g[f"map2_{k}"])
    assert np.array_equal(ref.rectify_gray(g["bgr"], g["K1"], g["d1"], g["R1"], g["P1"][:, :3]), g["gray"])


# ------------------------------------------------------------------ the argument checks, sanitized
def test_rectify_boundary_checks_under_sanitizers(tmp_path):
    """csrc/capi_rectify.cpp's refusals by their exact messages, the accepted bound next to each and
    the valid calls reaching exactly their launcher: tests/sanitize/rectify_check.cpp (its own main
    and its own stubs of the three launchers), built like sanitize_build.run_check builds the
    others, plus capi_rectify.cpp."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    shared = hasattr(ctypes.CDLL(None), "__asan_init")  # see sanitize_build.run_check
    rt = subprocess.run([gxx, "-print-file-name=" + ("libasan.so" if shared else "libasan.a")], capture_output=True,
                        text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("the ASan runtime of g++ is not installed")
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("HIP headers not found")
    exe = str(tmp_path / "rectify_check")
    san, csrc = os.path.join(ROOT, "tests", "sanitize"), os.path.join(ROOT, "forest-slam_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-g", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", hip_inc,
           "-I", os.path.join(ROOT, "include"), os.path.join(csrc, "capi.cpp"), os.path.join(csrc, "capi_rectify.cpp"),
           os.path.join(san, "host_stubs.cpp"), os.path.join(san, "rectify_check.cpp"), "-o", exe]
    b = subprocess.run(cmd + ([] if shared else ["-static-libasan", "-static-libubsan"]), capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "0 failed" in r.stdout
