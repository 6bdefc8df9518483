"""Sparse stereo on the CPU: the specification tests/sparse_stereo_ref.py against known answers
(hand-built boundary cases), against the oracle's SGBM and ground truth on the synthetic forest, and
the host layer csrc/capi_stereo.cpp under the sanitizers.  The GPU kernels are compared bit for
bit against the same specification in tests/test_sparse_stereo_gpu.py."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import sparse_stereo_cases as cases
import sparse_stereo_ref as ref
from conftest import ROOT


# ------------------------------------------------------------------ hand-built boundary cases
@pytest.mark.parametrize("name", list(cases.boundary_cases()))
def test_boundary_case(name):
    """Both sides of every boundary of the rule: the row band (equal / one ulp past), d0 at min and
    max, octave difference 1 / 2, hamming 75 / 76, the contests' tie rules, a SAD tie, k* = +-S, the
    windows touching / crossing each image side, and each status 1..6."""
    c = cases.boundary_cases()[name]
    stereo, info = cases.run_ref(c, cases.BOUNDARY_K, cases.BOUNDARY_BASELINE, **cases.BOUNDARY_PARAMS)
    assert stereo.shape == (len(c["kpL"]), 4) and info.shape == (len(c["kpL"]), 4)
    for i, status, j, ham, k in c["expect"]:
        for got, want, what in zip(info[i], (j, ham, k, status), ("right index", "hamming", "k*", "status")):
            assert want is None or int(got) == want, (name, i, what, info[i].tolist())
    # the record is all zeros exactly where the status is not 0, and Z passes the gate elsewhere
    ok = info[:, 3] == 0
    assert not stereo[~ok].any()
    assert ((stereo[ok, 2] > 0.1) & (stereo[ok, 2] < 1000)).all()


def test_boundary_cases_cover_every_status():
    seen = set()
    for c in cases.boundary_cases().values():
        _, info = cases.run_ref(c, cases.BOUNDARY_K, cases.BOUNDARY_BASELINE, **cases.BOUNDARY_PARAMS)
        seen |= set(info[:, 3].tolist())
    assert seen == set(range(7))


def test_d0_at_max_is_a_candidate():
    c = cases.boundary_cases()["d0_equal_max"]
    _, info = cases.run_ref(c, cases.BOUNDARY_K, cases.BOUNDARY_BASELINE, **cases.BOUNDARY_PARAMS)
    assert info[0, 3] != ref.STATUS_NO_MATCH and info[0, 0] == 0


def test_unique_off_keeps_every_suitor():
    c = cases.boundary_cases()["contest_equal"]
    stereo, info = cases.run_ref(c, cases.BOUNDARY_K, cases.BOUNDARY_BASELINE, unique=0, **cases.BOUNDARY_PARAMS)
    assert info[:, 3].tolist() == [0, 0] and info[:, 0].tolist() == [0, 0] and stereo[:, 2].all()


def test_parabola_on_known_sads():
    """Flat images with one bright pixel at the left window's centre; the right image has it 1 px
    right of xr and a 40 beside it: SAD(0), SAD(1), SAD(2) = 230, 30, 170 (every other shift 230), so
    k* = 1 and delta = (230 - 170) / (2 (230 + 170 - 60)) = 60 / 680 in float32."""
    xl, xr, yl = 50, 44, 30
    L = np.full((cases.H, cases.W), 10, np.uint8)
    R = L.copy()
    L[yl, xl] = 110
    R[yl, xr + 1] = 110
    R[yl, xr + 2] = 40
    d = np.zeros((1, 32), np.uint8)
    stereo, info = ref.sparse_stereo(L, R, cases.kp_rows([(xl, yl, 0)]), d, cases.kp_rows([(xr, yl, 0)]), d,
                                     cases.BOUNDARY_K, cases.BOUNDARY_BASELINE, ref.Params(**cases.BOUNDARY_PARAMS))
    assert info[0].tolist() == [0, 0, 1, 0]
    f32 = np.float32
    want_d = f32(50) - (f32(45) + f32(60) / f32(680))
    assert stereo[0, 3] == want_d and stereo[0, 2] == f32(1.0) / want_d
    assert stereo[0, 0] == ((f32(50) - f32(48)) / f32(10)) * stereo[0, 2]
    assert stereo[0, 1] == ((f32(30) - f32(32)) / f32(10)) * stereo[0, 2]


# ------------------------------------------------------------------ the synthetic forest
# The forest is planted along the sequence's path, so the scene depends on the sequence's length.
# The figures these tests were specified with (388 and 408 points on frames 0 and 30, 0.9707 and
# 0.9722 within 1 px of SGBM, 109 pure-shift keypoints, the pose errors below) are those of the
# 40-frame sequence, which reproduces every one of them to the last digit; the 963-frame default
# gives another forest (611 and 597 points, 0.988 and 0.976, 98 keypoints).
W, H, N_FRAMES = 640, 400, 40


@functools.lru_cache(maxsize=None)
def _seq():
    from forest_slam_amd import synth
    return synth.StereoSequence(seed=0, n_frames=N_FRAMES, W=W, H=H)


@functools.lru_cache(maxsize=None)
def _frame(i):
    return tuple(x.numpy() for x in _seq().frame(i))


@functools.lru_cache(maxsize=None)
def _orb(i, side, nfeatures):
    import oracle
    oracle.build()
    return oracle.orb_detect_compute(_frame(i)[side], nfeatures)


@functools.lru_cache(maxsize=None)
def _sparse(i, nfeatures=1000):
    from forest_slam_amd import synth
    (kl, dl), (kr, dr) = _orb(i, 0, nfeatures), _orb(i, 1, nfeatures)
    return ref.sparse_stereo(_frame(i)[0], _frame(i)[1], kl, dl, kr, dr, _seq().K, synth.BASELINE)


def test_pure_shift(oracle_mod):
    """The right image is the left shifted 12 px: every octave-0 left keypoint whose twin exists
    (xL - 12 >= 31, ORB's border) is matched with hamming 0 and slide 0, |d - 12| <= 0.5."""
    from forest_slam_amd import synth
    L = _frame(0)[0]
    R = np.zeros_like(L)
    R[:, :-12] = L[:, 12:]
    kl, dl = oracle_mod.orb_detect_compute(L, 500)
    kr, dr = oracle_mod.orb_detect_compute(R, 500)
    stereo, info = ref.sparse_stereo(L, R, kl, dl, kr, dr, _seq().K, synth.BASELINE)
    sel = (kl[:, 5] == 0) & (kl[:, 0] - 12 >= 31)
    assert sel.sum() == 109
    assert (info[sel, 3] == 0).all() and (info[sel, 1] == 0).all() and (info[sel, 2] == 0).all()
    err = np.abs(stereo[sel, 3] - 12)
    print(f"pure shift: {sel.sum()} keypoints, max |d - 12| = {err.max():.4f}")
    assert (err <= 0.5).all()


@pytest.mark.parametrize("frame", [0, 30])
def test_agrees_with_sgbm(oracle_mod, frame):
    """At least 300 of 1000 left keypoints get a point, and of those where SGBM is valid at the
    keypoint's pixel at least 0.95 lie within 1 px of its disparity: a condition on the rule."""
    stereo, info = _sparse(frame)
    ok = info[:, 3] == 0
    kl = _orb(frame, 0, 1000)[0]
    d16 = oracle_mod.sgbm(_frame(frame)[0], _frame(frame)[1], num_disp=96)
    sg = d16[kl[ok, 1].astype(int), kl[ok, 0].astype(int)]
    valid = sg >= 0
    diff = np.abs(stereo[ok, 3][valid] - sg[valid] / 16.0)
    frac = float((diff <= 1.0).mean())
    print(f"frame {frame}: {ok.sum()} points, {valid.sum()} with SGBM, {frac:.4f} within 1 px, "
          f"median {np.median(diff):.3f} px")
    assert ok.sum() >= 300
    assert frac >= 0.95


@pytest.mark.parametrize("pair", [(10, 11), (30, 31)])
def test_pose_from_sparse_points(oracle_mod, pair):
    """solvePnPRansac on the sparse points of the matched keypoints: ok, and the translation error
    against the ground truth at most 1.5 x that of the SGBM path (oracle.frame_pose) + 2 mm.  The
    frames are rendered through a pinhole, so both paths solve with zero distortion (the
    reference's coefficients would add a common bias of 20-50 mm, under which the bound says
    nothing).  Measured: (10, 11) sparse 341 points / 306 inliers, 2.7 mm, SGBM path 654 / 571,
    2.4 mm; (30, 31) sparse 346 / 240, 13.9 mm, SGBM path 658 / 404, 16.5 mm.

    A third of pair (30, 31)'s temporal matches are outliers, and its pose moves by centimetres
    with the set of points that enters RANSAC, whichever path the depths come from: the third
    figure printed is the pose from SGBM's own depths at the sparse path's points.  On the
    963-frame forest the same pair gives sparse 12.8 mm, SGBM path 3.7 mm, and SGBM's depths at
    the sparse points 20.8 mm (dropping the 11 sparse points more than 1 px from SGBM: 3.7 mm) --
    the bound would be missed there by the choice of points, not by their depths."""
    from forest_slam_amd import synth
    i, j = pair
    seq = _seq()
    dist = np.zeros(5)
    (k0, d0), (k1, d1) = _orb(i, 0, 1000), _orb(j, 0, 1000)
    m = oracle_mod.bf_match(d0, d1)
    P3, p2, keep = ref.backproject_stereo(_sparse(i)[0], k1, m)
    T_gt = np.linalg.inv(seq.T_wc[j]) @ seq.T_wc[i]  # previous camera -> current camera
    ok, rv, tv, inl, _, _ = oracle_mod.solve_pnp_ransac(P3, p2, seq.K, dist)
    assert ok
    dense = oracle_mod.frame_pose(_frame(i)[0], _frame(i)[1], _frame(j)[0], seq.K, dist, synth.BASELINE, 1000)
    e_sparse = float(np.linalg.norm(tv - T_gt[:3, 3]))
    e_dense = float(np.linalg.norm(dense["T"][:3, 3] - T_gt[:3, 3]))
    sub = m[keep]
    P3m, p2m, _ = oracle_mod.backproject(oracle_mod.disparity_map(dense["disp16"]), k0[sub[:, 0], :2], k1[sub[:, 1], :2],
                                         seq.K, synth.BASELINE)
    e_mixed = float(np.linalg.norm(oracle_mod.solve_pnp_ransac(P3m, p2m, seq.K, dist)[2] - T_gt[:3, 3]))
    print(f"pair {pair}: sparse {len(P3)} points / {len(inl)} inliers, {1e3 * e_sparse:.1f} mm; SGBM path "
          f"{len(dense['P3'])} points / {len(dense['inliers'])} inliers, {1e3 * e_dense:.1f} mm; SGBM depths at the "
          f"sparse points ({len(P3m)}): {1e3 * e_mixed:.1f} mm")
    assert e_sparse <= 1.5 * e_dense + 2e-3


def test_run_stereo_bag_refuses_a_dense_map_without_disparities():
    from forest_slam_amd import pipeline
    with pytest.raises(ValueError, match="sparse"):
        pipeline.run_stereo_bag("no-such.bag", depth="sparse", dense_map=object())


# ------------------------------------------------------------------ the argument checks, sanitized
def test_stereo_boundary_checks_under_sanitizers(tmp_path):
    """csrc/capi_stereo.cpp's refusals by their exact messages, the accepted bound next to each and
    the valid calls reaching exactly their launcher: tests/sanitize/stereo_check.cpp (its own main
    and its own stubs of the two launchers), built like tests/test_rectify_cpu.py builds
    rectify_check.cpp, with capi_stereo.cpp in place of capi_rectify.cpp."""
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
    exe = str(tmp_path / "stereo_check")
    san, csrc = os.path.join(ROOT, "tests", "sanitize"), os.path.join(ROOT, "forest-slam_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-g", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", hip_inc,
           "-I", os.path.join(ROOT, "include"), os.path.join(csrc, "capi.cpp"), os.path.join(csrc, "capi_stereo.cpp"),
           os.path.join(san, "host_stubs.cpp"), os.path.join(san, "stereo_check.cpp"), "-o", exe]
    b = subprocess.run(cmd + ([] if shared else ["-static-libasan", "-static-libubsan"]), capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "0 failed" in r.stdout
