"""Lens, image and motion-blur cases shared by the ingest case tests (test_ingest_cases_gpu.py on
the GPU, test_ingest_cases_cpu.py without one): fvo_undistort_gray off the reference's cameras
(tangential terms, k3, skew, K[8] != 1, a projective bottom row, saturating map entries) and
fvo_motion_blur at the kernel sizes, image sizes and seed positions where its kernel takes
another path.

NumPy only.  Every lens case names what it is meant to reach; test_ingest_cases_cpu.py asserts on
the oracle's own map that it does, so a badly chosen lens fails there and not silently on the GPU.
"""
import functools
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_ingest import synthetic_bgr  # noqa: E402

KC = np.array([[70.0, 0.0, 48.3], [0.0, 69.0, 37.6], [0.0, 0.0, 1.0]])
DIST_TANG = (-0.2, 0.05, 0.01, -0.02, 0.03)
K_SKEW = KC.copy()
K_SKEW[0, 1] = 0.8
K_K8 = np.array([[140.0, 0.0, 96.6], [0.0, 138.0, 75.2], [0.0, 0.0, 2.0]])
K_PERSP = np.array([[70.0, 0.8, 48.3], [0.3, 69.0, 37.6], [2e-4, -3e-4, 1.0]])

SIZES = ((100, 76), (101, 77))  # (W, H)
# tang alone: two 256-column blocks with H % 4 == 0 and 15-row stripes; 4096 / W > H, one stripe;
# H % 4 != 0
TANG_SIZES = ((260, 40), (64, 40), (66, 35))

LENSES = {
    "tang": dict(K=KC, dist=DIST_TANG, reach="tangential terms and k3"),
    "pincushion": dict(K=KC, dist=(0.4, 0.1, 0.003, 0.002, 0.05),
                       reach="output pixels whose 2x2 support lies partly or wholly outside the image"),
    "skew": dict(K=K_SKEW, dist=DIST_TANG, reach="the non-pinhole instantiation with a constant w"),
    "k8": dict(K=K_K8, dist=DIST_TANG, reach="K[8] != 1"),
    "persp": dict(K=K_PERSP, dist=(0.1, 0.05, 0.01, -0.02, 0.03), reach="a per-pixel 1/_w"),
    "saturate": dict(K=KC, dist=(1e7, 0.0, 0.0, 0.0, 0.0),
                     reach="both saturation branches of the map rounding, some reading a real pixel"),
}
# the lenses whose striped map is an exact row shift of the unstriped model (K[7] == 0, K[8] == 1)
MODEL_LENSES = ("tang", "pincushion", "skew")

LENS_CASES = tuple((name, W, H) for name in LENSES for (W, H) in SIZES) + \
    tuple(("tang", W, H) for (W, H) in TANG_SIZES)


def case_id(case):
    return "%s-%dx%d" % case


def lens(name):
    L = LENSES[name]
    return np.asarray(L["K"], np.float64), np.asarray(L["dist"], np.float64)


def stripe_rows(W, H):
    """cv2.undistort's stripe height (oracle/ingest_ref.cpp)."""
    return min(max(1, 4096 // max(W, 1)), H)


@functools.lru_cache(maxsize=None)
def images(W, H):
    """[3, H, W, 3] u8: two synthetic images and one of random bytes."""
    imgs = np.stack([synthetic_bgr(H, W, s) for s in range(3)])
    imgs[2] = np.random.default_rng(9).integers(0, 256, (H, W, 3), dtype=np.uint8)
    imgs.setflags(write=False)
    return imgs


def model_uv(K, dist, W, H):
    """Independent fp64 evaluation of initUndistortRectifyMap's source position (u, v) of every
    output pixel: the ray through np.linalg.inv(K), the full k1 k2 p1 p2 k3 model, no stripes."""
    K = np.asarray(K, np.float64)
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    row, col = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.einsum("ij,jhw->ihw", np.linalg.inv(K), np.stack([col, row, np.ones_like(col)]))
    x, y = ray[0] / ray[2], ray[1] / ray[2]
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def oracle_uv(mxy, frac):
    """(u, v) a CV_16SC2 map entry and its fractional index stand for."""
    return mxy[..., 0] + (frac & 31) / 32.0, mxy[..., 1] + (frac >> 5) / 32.0


def support(mxy, W, H):
    """Per map entry, how many of the four taps (sx, sy) .. (sx + 1, sy + 1) lie in the image."""
    sx, sy = mxy[..., 0].astype(np.int64), mxy[..., 1].astype(np.int64)
    nx = ((sx >= 0) & (sx < W)).astype(int) + ((sx + 1 >= 0) & (sx + 1 < W))
    ny = ((sy >= 0) & (sy < H)).astype(int) + ((sy + 1 >= 0) & (sy + 1 < H))
    return nx * ny


def stripe_w(K, W, H):
    """_w = ir[6]*col + ir[7]*i + ir[8] of every output pixel, ir the inverse of K with cy moved to
    the pixel's stripe (cv2.undistort)."""
    K = np.asarray(K, np.float64)
    s0 = stripe_rows(W, H)
    out = np.empty((H, W))
    col = np.arange(W, dtype=np.float64)
    for y0 in range(0, H, s0):
        A = K.copy()
        A[1, 2] -= y0
        ir = np.linalg.inv(A)
        for i in range(min(s0, H - y0)):
            out[y0 + i] = ir[2, 0] * col + ir[2, 1] * i + ir[2, 2]
    return out


# ------------------------------------------------------------------------------- motion blur
# 11 / 12: the direct / DFT switch at k*k < 130; 1; 2: an even k, asymmetric anchor; 30 / 31: the
# largest LDS tile and seed bitmap
BLUR_KS = (1, 2, 11, 12, 30, 31)
# (W, H): the smallest image that takes k = 31 and narrower than one 256-column tile; two row
# tiles; two column tiles and two row tiles
BLUR_SIZES = ((33, 32), (70, 48), (260, 40))
BLUR_CASES = tuple((W, H, k) for (W, H) in BLUR_SIZES for k in BLUR_KS if k < min(W, H))


def gray_images(W, H):
    """[3, H, W] u8: the green channel of two synthetic images and one of random bytes."""
    return np.ascontiguousarray(images(W, H)[..., 1])


def blur_centers(W, H, seed):
    """Seed pixels (flat indices) of one image: the four corners, the image centre, both sides of
    the column-tile seam (y, 255) | (y, 256) and of the row-tile seam (31, x) | (32, x) where the
    image has them, one duplicate, then about 1 % random pixels."""
    y, x = H // 3, W // 3
    fixed = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]
    fixed += [(y, c) for c in (255, 256) if c < W]
    fixed += [(r, x) for r in (31, 32) if r < H]
    fixed.append((H // 2, W // 2))
    flat = [r * W + c for r, c in fixed]
    flat += random.Random(seed).sample(range(H * W), max(1, H * W // 100))
    return np.asarray(flat, np.int32)
