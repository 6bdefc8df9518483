"""Dense stereo mapping without a GPU: the NumPy specification tests/dense_ref.py pinned to the
existing oracles (oracle.backproject for the camera-frame point, oracle.map_transform for the map
transform), its sampling order and overflow rule by known answers, and the argument validation of
the dense-mapping entry points as a stand-alone ASan + UBSan program (tests/sanitize/dense_check.cpp)."""
import numpy as np
import pytest

import dense_ref as dr
from sanitize_build import run_check


def _random_image(H, W, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(-40, 3000, size=(H, W)).astype(np.int16)
    img[rng.random((H, W)) < 0.2] = -16  # SGBM's invalid value
    img.flat[rng.choice(H * W, len(dr.HAND_SPECIALS), replace=False)] = dr.HAND_SPECIALS
    return img


def _pose(seed):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-np.pi, np.pi, 2)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Rx
    T[:3, 3] = rng.uniform(-50, 50, 3)
    return T


def _all_pixels(H, W):
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)


@pytest.mark.parametrize("img", [dr.hand_image(), _random_image(19, 37, 1)], ids=["hand", "random"])
def test_ref_step1_identity_equals_backproject_oracle(oracle_mod, img):
    """dense_ref at step 1 with T = I and the reference's filter (min_disp16 = -32768, 0.1 < Z <
    1000) is oracle.backproject with a keypoint at every pixel centre, bit for bit."""
    H, W = img.shape
    mk = _all_pixels(H, W)
    P, _, valid = oracle_mod.backproject(oracle_mod.disparity_map(img), mk, mk, dr.HAND_K, dr.HAND_BASELINE)
    got = dr.camera_points(img, dr.HAND_K, dr.HAND_BASELINE, 1, -32768, 0.1, 1000.0)
    assert 0 < len(P) < H * W
    assert got.dtype == np.float32 and np.array_equal(got, P)
    cloud, n = dr.dense_cloud(img[None], dr.HAND_K, dr.HAND_BASELINE, np.eye(4)[None], 1, -32768)
    assert n.tolist() == [int(valid.sum())] and np.array_equal(cloud, P.astype(np.float64))


def test_ref_hand_image_special_values():
    """Which of the hand-built image's special values survive, by value: 3 (Z = 870) and 26100
    (Z just above float32 0.1) are kept; 0 / -16 (-> 0.1: Z = 1631), 1 and 2 (Z > 1000), the
    negative disparities, 26101 and 32767 (Z < 0.1) are dropped."""
    row = np.array([dr.HAND_SPECIALS], np.int16)
    P = dr.camera_points(row, dr.HAND_K, dr.HAND_BASELINE, 1, -32768, 0.1, 1000.0)
    x = np.rint(P[:, 0] / P[:, 2] * np.float32(dr.HAND_K[0, 0]) + np.float32(dr.HAND_K[0, 2])).astype(int)
    assert [dr.HAND_SPECIALS[i] for i in x] == [3, 26100]
    assert P[1, 2] > np.float32(0.1) and np.float32(163.128) / np.float32(26101 / 16) < np.float32(0.1)
    # min_disp16 = 1 changes nothing here (every non-positive disparity fails the depth test), a
    # larger floor does
    assert np.array_equal(dr.camera_points(row, dr.HAND_K, dr.HAND_BASELINE, 1, 1), P)
    assert len(dr.camera_points(row, dr.HAND_K, dr.HAND_BASELINE, 1, 4)) == 1
    # and with a wider depth range the floor is what drops 0 and the negative disparities' neighbours
    wide = dr.camera_points(row, dr.HAND_K, dr.HAND_BASELINE, 1, -32768, 0.0, 1e6)
    assert len(wide) == 8 and len(dr.camera_points(row, dr.HAND_K, dr.HAND_BASELINE, 1, 1, 0.0, 1e6)) == 6


def test_ref_general_pose_equals_map_transform_oracle(oracle_mod):
    img = _random_image(19, 37, 2)
    P = dr.camera_points(img, dr.HAND_K, dr.HAND_BASELINE)
    for seed in (3, 4):
        T = _pose(seed)
        o64, o32 = oracle_mod.map_transform(P, T)
        got = dr.map_points(P, T)
        assert np.array_equal(got, o64)
        m64, m32, cnt = dr.append(got, 0, np.zeros((len(P), 3)), np.zeros((len(P), 3), np.float32))
        assert cnt == len(P) and np.array_equal(m64, o64) and np.array_equal(m32, o32)


def test_ref_sampling_order_frames_and_overflow():
    K = np.array([[100.0, 0, 0.0], [0, 100.0, 0.0], [0, 0, 1]])
    img = np.full((2, 3, 5), 160, np.int16)  # d = 10, Z = 100 * 0.5 / 10 = 5
    img[1, 0, 2] = -16
    T = np.stack([np.eye(4), np.eye(4)])
    T[1, :3, 3] = [1000.0, 2000.0, 3000.0]
    cloud, n = dr.dense_cloud(img, K, 0.5, T, step=2)
    # frame 0: (y, x) = (0,0) (0,2) (0,4) (2,0) (2,2) (2,4); frame 1 without its invalid (0,2)
    px = [(0, 0), (2, 0), (4, 0), (0, 2), (2, 2), (4, 2)]
    want = [[x / 100 * 5, y / 100 * 5, 5.0] for x, y in px]
    want += [[x / 100 * 5 + 1000, y / 100 * 5 + 2000, 3005.0] for x, y in px if (x, y) != (2, 0)]
    assert n.tolist() == [6, 5] and np.allclose(cloud, want, rtol=0, atol=1e-6)
    assert dr.dense_cloud(img, K, 0.5, T, step=2, frame_keep=[0, 1])[1].tolist() == [0, 5]
    assert dr.dense_cloud(img, K, 0.5, T, step=5)[1].tolist() == [1, 1]
    # the overflow rule: written up to map_cap, counted in full, clamped at INT32_MAX
    guard = np.full((12, 3), -7.0)
    m64, m32, cnt = dr.append(cloud, 3, guard, None, map_cap=9)
    assert cnt == 14 and np.array_equal(m64[3:9], cloud[:6]) and (m64[:3] == -7).all() and (m64[9:] == -7).all()
    m64, m32, cnt = dr.append(cloud, 3, guard, guard.astype(np.float32), map_cap=0)
    assert cnt == 14 and (m64 == -7).all() and (m32 == -7).all()
    assert dr.append(cloud, dr.INT32_MAX - 4, guard, None, map_cap=12)[2] == dr.INT32_MAX


def test_ref_reproject_known_answers():
    Q = np.array([[1.0, 0, 0, -2.0], [0, 1.0, 0, -1.0], [0, 0, 0, 50.0], [0, 0, 0.25, 0.0]])
    d = np.array([[4, 8, 4], [16, -4, 4]], np.int16)  # the raw value is the disparity: no / 16
    out = dr.reproject(d, Q)
    assert out.dtype == np.float32 and out.shape == (2, 3, 3)
    assert np.array_equal(out[0, 1], [(1 - 2) / 2.0, (0 - 1) / 2.0, 25.0])
    assert np.array_equal(out[1, 0], [(0 - 2) / 4.0, 0.0, 12.5])
    assert np.array_equal(dr.reproject(d.astype(np.float32), Q), out)
    miss = dr.reproject(d, Q, handle_missing=True)
    assert miss[1, 1, 2] == 10000.0 and np.array_equal(miss[..., :2], out[..., :2])
    miss[1, 1, 2] = out[1, 1, 2]
    assert np.array_equal(miss, out)
    # the minimum occurring several times: all of them
    assert (dr.reproject(np.abs(d), Q, handle_missing=True)[..., 2] == 10000.0).sum() == 4


def test_dense_boundary_checks_under_sanitizers(tmp_path):
    """Every refusal of the dense-mapping entry points of csrc/capi.cpp by its exact message with
    nothing launched, the accepted bound next to each, and a valid call reaching exactly its
    launcher: the stand-alone ASan + UBSan program tests/sanitize/dense_check.cpp."""
    run_check("dense_check", tmp_path)
