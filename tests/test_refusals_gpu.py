"""Refusals of the C ABI on the real library: every argument / config check that once lived in a
device translation unit, by its exact message.  Each case creates the smallest context that
reaches the check (one stage, 64x64 or 64x32, max_batch 1) and launches nothing beyond context
initialisation.  Entry-point refusals surface as Context's RuntimeError; fvo_create's go to stderr
as "fvo_create: <message>".  (The host-only twin with the accepted bounds next to each refusal:
tests/sanitize/capi_check.cpp.)"""
import ctypes
import functools

import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

CAP, F = 64, 4  # keypoint capacity of the ORB-less contexts; frames of the BA arrays


@functools.lru_cache(maxsize=None)
def _ctx(stage, nlevels=8):
    from forest_slam_amd import _lib
    return _lib.Context(64, 64, max_batch=1, stages=getattr(_lib, "STAGE_" + stage), kp_capacity=CAP, nlevels=nlevels,
                        ba_max_landmarks=64, ba_max_obs=256)


def _refused(message, call, *args, **kw):
    with pytest.raises(RuntimeError) as e:
        call(*args, **kw)
    assert str(e.value) == "libfvo: " + message


def _z(shape, dtype):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def _ba_args():
    return dict(kp=_z((F, CAP, 8), torch.float32), nkp=_z((F,), torch.int32), matches=_z((F, CAP, 3), torch.int32),
                nmatch=_z((F,), torch.int32), stereo=_z((F, CAP, 4), torch.float32), T_rel=_z((F, 4, 4), torch.float64),
                K=torch.eye(3, dtype=torch.float64), baseline=0.25, n_windows=1)


@pytest.mark.parametrize("kw, message", [
    (dict(first_end=0, first_valid=0), "ba: windows exceed the frame range"),
    (dict(first_end=2, first_valid=2), "ba: first_valid out of range"),
    (dict(first_end=2, first_valid=0, iterations=101), "ba: iterations out of range"),
])
def test_ba_windows_ranges(kw, message):
    _refused(message, _ctx("BA").ba_windows, **_ba_args(), **kw)


def test_ba_windows_level_count():
    # Context.ba_windows passes fvo_config.nlevels, which nothing checks while the ORB stage is off
    _refused("ba: bad level count", _ctx("BA", nlevels=13).ba_windows, **_ba_args(), first_end=2, first_valid=0)


def test_ba_landmarks_window_index():
    _refused("ba: window index out of range", _ctx("BA").ba_landmarks, window=1)


@pytest.mark.parametrize("max_iters", [0, 1001])
def test_find_essential_max_iters(max_iters):
    p = _z((1, CAP, 2), torch.float32)
    _refused("essential: max_iters out of range", _ctx("MONO").find_essential, p, p, _z((1,), torch.int32), 100.0,
             (32.0, 32.0), max_iters=max_iters)


def test_pnp_ransac_iterations():
    _refused("iterations out of range", _ctx("POSE").pnp_ransac, _z((1, CAP, 3), torch.float32),
             _z((1, CAP, 2), torch.float32), _z((1,), torch.int32), torch.eye(3, dtype=torch.float64), [0.0] * 5,
             iterations=1001)


def test_bf_match_misaligned_descriptors():
    n = _z((1,), torch.int32)
    d = _z((CAP * 32 + 16,), torch.uint8)
    off = d[1:1 + CAP * 32].view(1, CAP, 32)
    assert off.data_ptr() % 16 == 1 and off.is_contiguous()
    _refused("descriptor buffers must be 16-byte aligned", _ctx("BF").bf_match, off, n, d[:CAP * 32].view(1, CAP, 32), n)


def test_motion_blur_misaligned_mask():
    mask = _z((64 * 64 + 4,), torch.uint8)[1:1 + 64 * 64].view(1, 64, 64)
    assert mask.data_ptr() % 4 == 1
    _refused("motion blur: mask must be 4-byte aligned", _ctx("BF").motion_blur, _z((1, 64, 64), torch.uint8), 5,
             centers=_z((1, 8), torch.int32), n_centers=_z((1,), torch.int32), mask=mask)


def test_voxel_workspace_one_byte_short():
    ctx, n = _ctx("BF"), 10
    wb = int(ctx.L.fvo_voxel_workspace_bytes(n))
    assert wb > 0
    pts, ws, out = _z((n, 3), torch.float64), _z((wb,), torch.uint8), _z((n, 3), torch.float64)
    cnt = _z((1,), torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _refused("voxel_down_sample: workspace too small", lambda: ctx._check(ctx.L.fvo_voxel_down_sample(
        ctx.h, p(pts), n, 0.5, p(ws), wb - 1, p(out), p(cnt), None, None)))


def _lens(base, **entries):
    """A lens of tests/ingest_cases.py with entries of K (k0..k8) or dist (d0..d4) replaced."""
    import ingest_cases as ic
    K, d = ic.lens(base)
    K, d = K.reshape(9).copy(), d.copy()
    for name, v in entries.items():
        (K if name[0] == "k" else d)[int(name[1:])] = v
    return K, d


# What cv2.undistort defines no output for (the map would be NaN): refused as fvo_rectify_map refuses
# it.  `_w` changes sign across the 64 columns with K[6] = 2 (-2.7 at column 0, +2.1 at column 63).
@pytest.mark.parametrize("base, entries, message", [
    ("tang", dict(k0=0.0), "undistort_gray: K is singular (a stripe's camera matrix has det == 0)"),
    ("tang", dict(k8=0.0), "undistort_gray: K is singular (a stripe's camera matrix has det == 0)"),
    ("persp", dict(k6=2.0), "undistort_gray: _w <= 0 at a stripe corner (the view reaches the camera's horizon)"),
    ("tang", dict(d3=float("nan")), "undistort_gray: K and dist must be finite"),
    ("tang", dict(k2=float("inf")), "undistort_gray: K and dist must be finite"),
], ids=["K0=0", "K8=0", "w-changes-sign", "nan-in-dist", "inf-in-K"])
def test_undistort_gray_refuses_lens(base, entries, message):
    K, d = _lens(base, **entries)
    _refused(message, _ctx("BF").undistort_gray, _z((1, 64, 64, 3), torch.uint8), K, d)


def test_undistort_gray_accepts_the_lens_cases():
    import ingest_cases as ic
    for name in ic.LENSES:
        _ctx("BF").undistort_gray(_z((1, 64, 64, 3), torch.uint8), *ic.lens(name))


# width 80 for the 16-bit case: at 64 columns every accepted numDisparities leaves no column
# ("image narrower than numDisparities" comes first)
@pytest.mark.parametrize("stage, size, cfg, message", [
    ("SGBM", (64, 32), dict(block_size=5), "SGBM: only blockSize=7 is supported"),
    ("SGBM", (64, 32), dict(num_disparities=80), "SGBM: numDisparities must be 64, 96 or 128"),
    ("SGBM", (64, 32), dict(sgbm_stripes=0), "SGBM: stripes must be >= 1"),
    ("SGBM", (64, 32), dict(sgbm_lanes=8, sgbm_cols=64),
     "SGBM: (sgbm_lanes, sgbm_cols) must be (4, 32|64), (8, 16|32) or (16, 32)"),
    ("SGBM", (80, 32), dict(num_disparities=64, P2=17000, pre_filter_cap=63),
     "SGBM: P2/preFilterCap too large for the 16-bit aggregated cost"),
    ("BA", (64, 64), dict(kp_capacity=CAP, ba_window=2), "ba_window must be in [3, 21]"),
    ("BA", (64, 64), dict(kp_capacity=CAP, ba_window=22), "ba_window must be in [3, 21]"),
    ("ORB", (64, 64), dict(nlevels=13), "nlevels out of range"),
    ("ORB", (64, 64), dict(edge_threshold=14), "edgeThreshold must be >= patchSize/2 (15)"),
    ("BF", (64, 64), dict(kp_capacity=70000), "BF: kp_capacity must be <= 65535 (16-bit indices in the keys)"),
])
def test_create_refuses_config(capfd, stage, size, cfg, message):
    from forest_slam_amd import _lib
    cfg = dict(dict(ba_max_landmarks=64, ba_max_obs=256), **cfg)
    with pytest.raises(RuntimeError):
        _lib.Context(*size, max_batch=1, stages=getattr(_lib, "STAGE_" + stage), **cfg)
    said = [line for line in capfd.readouterr().err.splitlines() if line.startswith("fvo_create: ")]
    assert said == ["fvo_create: " + message]
