"""NumPy specification of the dense stereo mapping (fvo_dense_map_append) and of
cv2.reprojectImageTo3D as fvo_reproject_to_3d evaluates it.  Shared by tests/test_dense_cpu.py
(pinned there to oracle.backproject and oracle.map_transform) and tests/test_dense_gpu.py (the
HIP kernels, bit for bit).

Every cast and the order of every operation is spelled out: float32 for the camera-frame point
(the reference's NumPy 1.x arithmetic, stereo_slam.py:117-121 and :265-289), fp64 without
contraction for the map transform (stereo_slam.py:308-311), NumPy elementwise ops fuse nothing."""
import numpy as np

f32 = np.float32
INT32_MAX = 2 ** 31 - 1
FLT_EPSILON = float(np.finfo(np.float32).eps)


def camera_points(d16, K, baseline, step=1, min_disp16=1, z_min=0.1, z_max=1000.0):
    """One int16 [H,W] disparity map -> float32 [n,3] camera-frame points of the kept samples:
    pixels (y, x), y = 0, step, ... < H and x likewise, in row-major order."""
    d16 = np.asarray(d16)
    assert d16.dtype == np.int16 and d16.ndim == 2 and step >= 1
    H, W = d16.shape
    K = np.asarray(K, np.float64).reshape(3, 3)
    ys, xs = np.meshgrid(np.arange(0, H, step), np.arange(0, W, step), indexing="ij")
    s16 = d16[::step, ::step]
    d = s16.astype(f32) / f32(16)
    d[d == f32(0.0)] = f32(0.1)
    d[d == f32(-1.0)] = f32(0.1)
    Z = f32(K[0, 0] * baseline) / d  # (float)(K[0] * baseline) / d
    X = ((xs.astype(f32) - f32(K[0, 2])) / f32(K[0, 0])) * Z
    Y = ((ys.astype(f32) - f32(K[1, 2])) / f32(K[1, 1])) * Z
    assert Z.dtype == X.dtype == Y.dtype == f32
    keep = (s16.astype(np.int64) >= int(min_disp16)) & (Z > f32(z_min)) & (Z < f32(z_max))
    return np.stack([X[keep], Y[keep], Z[keep]], axis=1).astype(f32).reshape(-1, 3)


def map_points(P, T):
    """float32 [n,3] points, fp64 4x4 T -> fp64 [n,3]: x' = ((T0 X + T1 Y) + T2 Z) + T3 * 1.0."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = (np.asarray(P, f32)[:, k].astype(np.float64) for k in range(3))
    return np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] * 1.0 for k in range(3)],
                    axis=1).reshape(-1, 3)


def dense_cloud(disp, K, baseline, T, step=1, min_disp16=1, z_min=0.1, z_max=1000.0, frame_keep=None):
    """int16 [B,H,W] maps, fp64 [B,4,4] poses -> (fp64 [n,3] map-frame cloud, frames in batch
    order; n_added int32 [B])."""
    parts, n_added = [], []
    for b in range(len(disp)):
        if frame_keep is not None and int(frame_keep[b]) == 0:
            P = np.zeros((0, 3), f32)
        else:
            P = camera_points(disp[b], K, baseline, step, min_disp16, z_min, z_max)
        parts.append(map_points(P, T[b]))
        n_added.append(len(P))
    return np.concatenate(parts).reshape(-1, 3), np.asarray(n_added, np.int32)


def append(cloud, map_count, map64=None, map32=None, map_cap=None):
    """fvo_map_transform's overflow contract: the cloud is appended from map_count; points at
    positions >= map_cap are counted but not written; the count clamps at INT32_MAX.  Returns
    (map64, map32, new count) with the arrays (either may be None) updated as copies."""
    caps = [len(m) for m in (map64, map32) if m is not None]
    cap = min(caps) if map_cap is None else int(map_cap)
    k = max(0, min(len(cloud), cap - int(map_count)))
    if map64 is not None:
        map64 = map64.copy()
        map64[map_count:map_count + k] = cloud[:k]
    if map32 is not None:
        map32 = map32.copy()
        map32[map_count:map_count + k] = cloud[:k].astype(f32)  # the PointCloud2 FLOAT32 record
    return map64, map32, min(int(map_count) + len(cloud), INT32_MAX)


# The camera of the hand-built image: fx * baseline = 163.128, so that d16 = 26100 | 26101 give Z on
# either side of float32 0.1 and d16 = 2 | 3 on either side of 1000.
HAND_K = np.array([[1631.28, 0.0, 19.5], [0.0, 1500.0, 11.25], [0.0, 0.0, 1.0]])
HAND_BASELINE = 0.1
HAND_SPECIALS = [0, -16, -1, -17, 1, 2, 3, 26100, 26101, 32767, -32768]


def hand_image():
    """int16 [24,40]: the special values (the invalid / zero disparities and their neighbours,
    the two pairs around the depth bounds, the int16 extremes) scattered over rows 0, 11 and 23
    and the corners, on a ramp of valid disparities."""
    H, W = 24, 40
    img = (16 + 7 * np.arange(H * W, dtype=np.int64)).astype(np.int16).reshape(H, W)  # 16 .. 6729
    for r, x0 in ((0, 0), (11, 17), (23, W - len(HAND_SPECIALS))):
        img[r, x0:x0 + len(HAND_SPECIALS)] = HAND_SPECIALS
    img[0, W - 1], img[23, 0] = -16, 3
    return img


def reproject(disp, Q, handle_missing=False):
    """cv2.reprojectImageTo3D on an int16 / float32 [H,W] image, OpenCV 4.x's Matx form in fp64:
    h_k = (((0 + Q[k][0] x) + Q[k][1] y) + Q[k][2] d) + Q[k][3], out = (float)(h_k / h_3), d the
    raw value; handle_missing: z = 10000 where |d - min| <= FLT_EPSILON."""
    disp = np.asarray(disp)
    assert disp.dtype in (np.int16, np.float32) and disp.ndim == 2
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    H, W = disp.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = disp.astype(np.float64)
    h = [(((0.0 + Q[k, 0] * x) + Q[k, 1] * y) + Q[k, 2] * d) + Q[k, 3] * 1.0 for k in range(4)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out = np.stack([(h[k] / h[3]).astype(f32) for k in range(3)], axis=2)
    if handle_missing:
        out[..., 2][np.abs(d - d.min()) <= FLT_EPSILON] = f32(10000.0)
    return out
