"""Stereo rectification on the host: ``stereo_rectify`` restates OpenCV 4.x cvStereoRectify
(Bouguet's algorithm, calibration.cpp) in float64 NumPy on the 3x3 / 3x4 values of one rig.

    rect = stereo_rectify(K1, d1, K2, d2, (W, H), R, T)       # x_right = R x_left + T
    L = ctx.rectify_gray(left,  K1, d1, rect.R1, rect.P1[:, :3])
    R = ctx.rectify_gray(right, K2, d2, rect.R2, rect.P2[:, :3])
    fe = vo.StereoFrontEnd(W, H, rect.K_rect, np.zeros(5), rect.baseline, ...)

Kept from OpenCV: the half rotation r_r = Rodrigues(-om/2), idx = the dominant axis of r_r T, the
rotation wR about t x uu by acos(|c| / |t|), R1 = wR r_r^T, R2 = wR r_r, fc_new = the smaller
idx^1 focal length (shrunk by 1 + k1 (nx^2 + ny^2) / (4 fc^2) when k1 < 0), the principal points
from the four image corners (undistortPoints' 5 iterations, rotated, projected with fc_new,
averaged), CALIB_ZERO_DISPARITY's or the single-axis averaging, P2[idx, 3] = t[idx] fc_new, Q,
icvGetRectangles' 9 x 9 grid with the alpha scaling, and the two valid-pixel ROIs.
OpenCV parity is unpinned (the tests carry an importorskip("cv2") cross-check of the outputs that
do not depend on the OpenCV release).  Not restated: OpenCV rounds the corner and grid points to
float32 and divides (nx - 1) / 2 as integers; everything here is float64.  Releases differ in two
places: newer ones derive fc_new from the mean of the two focal lengths, and older ones span the
9 x 9 grid over [0, nx] x [0, ny] and scale alpha with nx - cx; here the grid spans the pixel
centres [0, nx - 1] x [0, ny - 1] and alpha scales with nx - 1 - cx (one convention, the newer)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

CALIB_ZERO_DISPARITY = 1024


@dataclass
class StereoRectification:
    """cv2.stereoRectify's outputs plus what the front end takes: K_rect = P1[:, :3] (both
    rectified cameras share it up to the principal point of the non-shared axis) and the
    rectified baseline |P2[idx, 3]| / fc_new.  idx: 0 horizontal rig, 1 vertical rig."""
    R1: np.ndarray
    R2: np.ndarray
    P1: np.ndarray
    P2: np.ndarray
    Q: np.ndarray
    roi1: tuple
    roi2: tuple
    K_rect: np.ndarray
    baseline: float
    idx: int

    def cv2_tuple(self):
        return self.R1, self.R2, self.P1, self.P2, self.Q, self.roi1, self.roi2


def _rodrigues(r):
    th = float(np.sqrt(r @ r))
    if th < np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return math.cos(th) * np.eye(3) + (1.0 - math.cos(th)) * np.outer(k, k) + math.sin(th) * kx


def _rotation_vector(R):
    """cv2.Rodrigues(matrix) away from theta = pi (a stereo rig's two cameras look the same way)."""
    U, _, Vt = np.linalg.svd(R)
    R = U @ Vt
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = math.sqrt((r @ r) * 0.25)
    c = min(1.0, max(-1.0, (np.trace(R) - 1) * 0.5))
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        raise NotImplementedError("stereo_rectify: a relative rotation of 180 degrees is not implemented")
    return r * (math.acos(c) / (2 * s))


def _dist8(d):
    d = np.zeros(0) if d is None else np.asarray(d, np.float64).reshape(-1)
    if d.size not in (0, 4, 5, 8):
        raise NotImplementedError("stereo_rectify: distortion must be (k1 k2 p1 p2 [k3 [k4 k5 k6]])")
    return np.concatenate([d, np.zeros(8 - d.size)])


def _undistort_points(u, v, K, d, R=None, P=None):
    """cv2.undistortPoints: 5 fixed-point iterations of the radial-tangential / rational model,
    then R and the projection P (fx, fy, cx, cy of its left 3x3)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    x0 = (u - K[0, 2]) / K[0, 0]
    y0 = (v - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    if R is not None:
        X = R @ np.stack([x, y, np.ones_like(x)])
        x, y = X[0] / X[2], X[1] / X[2]
    if P is not None:
        x, y = x * P[0, 0] + P[0, 2], y * P[1, 1] + P[1, 2]
    return x, y


def _rectangles(K, d, R, P, nx, ny):
    """icvGetRectangles: the inscribed and the bounding rectangle (x, y, w, h) of the rectified
    image of a 9 x 9 grid over the source image's pixel centres [0, nx - 1] x [0, ny - 1]."""
    N = 9
    gy, gx = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64), indexing="ij")
    px, py = _undistort_points((gx * (nx - 1) / (N - 1)).ravel(), (gy * (ny - 1) / (N - 1)).ravel(), K, d, R, P)
    px, py = px.reshape(N, N), py.reshape(N, N)
    ix0, ix1, iy0, iy1 = px[:, 0].max(), px[:, -1].min(), py[0].max(), py[-1].min()
    inner = (ix0, iy0, ix1 - ix0, iy1 - iy0)
    outer = (px.min(), py.min(), px.max() - px.min(), py.max() - py.min())
    return inner, outer


def stereo_rectify(K1, d1, K2, d2, image_size, R, T, flags=CALIB_ZERO_DISPARITY, alpha=-1.0,
                   newImageSize=(0, 0)) -> StereoRectification:
    """cv2.stereoRectify(K1, d1, K2, d2, image_size, R, T, flags=, alpha=) in float64.
    R (3x3 or a rotation vector), T: x_right = R x_left + T.  flags: 0 or CALIB_ZERO_DISPARITY;
    alpha: -1 (no scaling) or [0, 1]; newImageSize: (0, 0) only.  Anything else raises
    NotImplementedError.  Horizontal and vertical rigs both give matrices; only a horizontal
    rig's pair (idx == 0) can go on to SGBM."""
    if flags not in (0, CALIB_ZERO_DISPARITY):
        raise NotImplementedError("stereo_rectify: flags must be 0 or CALIB_ZERO_DISPARITY")
    if tuple(int(v) for v in newImageSize) != (0, 0):
        raise NotImplementedError("stereo_rectify: only newImageSize=(0, 0) is implemented")
    alpha = float(alpha)
    if not (alpha == -1.0 or 0.0 <= alpha <= 1.0):
        raise NotImplementedError("stereo_rectify: alpha must be -1 or in [0, 1]")
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    if K1.shape != (3, 3) or K2.shape != (3, 3):
        raise NotImplementedError("stereo_rectify: camera matrices must be 3x3")
    d1, d2 = _dist8(d1), _dist8(d2)
    nx, ny = int(image_size[0]), int(image_size[1])
    if nx < 1 or ny < 1:
        raise NotImplementedError("stereo_rectify: image_size must be (width >= 1, height >= 1)")
    Rm = np.asarray(R, np.float64)
    T = np.asarray(T, np.float64).reshape(-1)
    if T.size != 3 or Rm.size not in (3, 9):
        raise NotImplementedError("stereo_rectify: R must be 3x3 or a rotation vector, T a 3-vector")
    om = _rotation_vector(Rm.reshape(3, 3)) if Rm.size == 9 else Rm.reshape(3).copy()

    r_r = _rodrigues(om * -0.5)  # both cameras turned to the average orientation
    t = r_r @ T
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    c, nt = t[idx], float(np.sqrt(t @ t))
    if not nt > 0.0:
        raise NotImplementedError("stereo_rectify: T must not be zero")
    uu = np.zeros(3)
    uu[idx] = 1.0 if c > 0 else -1.0
    ww = np.cross(t, uu)  # the rotation that takes t onto the image axis
    nw = float(np.sqrt(ww @ ww))
    if nw > 0.0:
        ww = ww * (math.acos(min(1.0, abs(c) / nt)) / nw)
    wR = _rodrigues(ww)
    R1, R2 = wR @ r_r.T, wR @ r_r
    t = R2 @ T

    fc_new = np.inf
    for K, d in ((K1, d1), (K2, d2)):
        fc = K[idx ^ 1, idx ^ 1]
        if d[0] < 0:
            fc = fc * (1 + d[0] * (nx * nx + ny * ny) / (4 * fc * fc))
        fc_new = min(fc_new, fc)
    cu = np.array([0.0, nx - 1.0, 0.0, nx - 1.0])
    cv = np.array([0.0, 0.0, ny - 1.0, ny - 1.0])
    cc = []
    for K, d, Rk in ((K1, d1, R1), (K2, d2, R2)):
        x, y = _undistort_points(cu, cv, K, d, Rk)
        cc.append([(nx - 1) / 2 - (fc_new * x).mean(), (ny - 1) / 2 - (fc_new * y).mean()])
    if flags & CALIB_ZERO_DISPARITY:
        cc[0][0] = cc[1][0] = (cc[0][0] + cc[1][0]) * 0.5
        cc[0][1] = cc[1][1] = (cc[0][1] + cc[1][1]) * 0.5
    elif idx == 0:
        cc[0][1] = cc[1][1] = (cc[0][1] + cc[1][1]) * 0.5
    else:
        cc[0][0] = cc[1][0] = (cc[0][0] + cc[1][0]) * 0.5

    def proj(k, f, tk):
        P = np.zeros((3, 4))
        P[0, 0] = P[1, 1] = f
        P[0, 2], P[1, 2], P[2, 2] = cc[k][0], cc[k][1], 1.0
        if k == 1:
            P[idx, 3] = tk
        return P

    P1, P2 = proj(0, fc_new, 0.0), proj(1, fc_new, t[idx] * fc_new)
    inner1, outer1 = _rectangles(K1, d1, R1, P1, nx, ny)
    inner2, outer2 = _rectangles(K2, d2, R2, P2, nx, ny)
    s = 1.0
    if alpha >= 0:
        def scale(rect, k, pick):
            x, y, w, h = rect
            cx, cy = cc[k]
            return pick(cx / (cx - x), cy / (cy - y), (nx - 1 - cx) / (x + w - cx), (ny - 1 - cy) / (y + h - cy))
        s0 = max(scale(inner1, 0, max), scale(inner2, 1, max))
        s1 = min(scale(outer1, 0, min), scale(outer2, 1, min))
        s = s0 * (1 - alpha) + s1 * alpha
    tx = s * P2[idx, 3]
    fc_new = fc_new * s
    P1, P2 = proj(0, fc_new, 0.0), proj(1, fc_new, tx)

    def roi(inner, k):
        x, y, w, h = inner
        x0, y0 = math.ceil((x - cc[k][0]) * s + cc[k][0]), math.ceil((y - cc[k][1]) * s + cc[k][1])
        x1, y1 = x0 + math.floor(w * s), y0 + math.floor(h * s)
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, nx), min(y1, ny)
        return (x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else (0, 0, 0, 0)

    Q = np.array([[1, 0, 0, -cc[0][0]], [0, 1, 0, -cc[0][1]], [0, 0, 0, fc_new],
                  [0, 0, -1.0 / t[idx], (cc[0][0] - cc[1][0] if idx == 0 else cc[0][1] - cc[1][1]) / t[idx]]])
    return StereoRectification(R1=R1, R2=R2, P1=P1, P2=P2, Q=Q, roi1=roi(inner1, 0), roi2=roi(inner2, 1),
                               K_rect=P1[:, :3].copy(), baseline=abs(P2[idx, 3]) / fc_new, idx=idx)
