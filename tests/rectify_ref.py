"""SPECIFICATION of the rectification kernels (csrc/rectify.hip) -- test infrastructure only.

Vectorised float64 / integer NumPy restatements, written from OpenCV's definitions and the
conventions of oracle/ingest_ref.cpp, independent of the package's code:
  rectify_map   cv2.initUndistortRectifyMap(K, dist, R, newK, (W, H), CV_16SC2)
  remap         cv2.remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT 0), u8, 1 or 3 channels
  bgr2gray      cv2.cvtColor(., COLOR_BGR2GRAY), 14-bit
  rectify_gray  the three in sequence (mono8: the remap alone)
  tile_paths    which output tiles the kernels stage in LDS (include/fvo.h's rule)
NumPy evaluates every expression below operation by operation in IEEE double, in the written
order: that order is the specification (the kernels are compiled without contraction)."""
import os
import re

import numpy as np

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fvo.h")


def header_macros():
    """FVO_RECTIFY_TILE_W, FVO_RECTIFY_TILE_H, FVO_RECTIFY_LDS_BYTES as include/fvo.h publishes them."""
    src = open(_HDR).read()
    return tuple(int(re.search(r"#define\s+%s\s+(\d+)" % n, src).group(1))
                 for n in ("FVO_RECTIFY_TILE_W", "FVO_RECTIFY_TILE_H", "FVO_RECTIFY_LDS_BYTES"))


def inv3(S):
    """OpenCV invert() 3x3 closed form on a flat 9-vector; None when det == 0."""
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if d == 0.0:
        return None
    d = 1.0 / d
    return np.array([(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
                     (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
                     (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d])


def inverse_view(newK, R):
    """ir = inverse(newK * R), the product's entries as (a0 b0 + a1 b1) + a2 b2."""
    N = np.asarray(newK, np.float64).reshape(3, 3)
    Rm = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    A = np.array([[(N[i, 0] * Rm[0, j] + N[i, 1] * Rm[1, j]) + N[i, 2] * Rm[2, j] for j in range(3)] for i in range(3)])
    return inv3(A.reshape(9))


def _round_sat(v):
    r = np.rint(np.clip(np.nan_to_num(v, nan=-np.inf), -2147483648.0, 2147483647.0)).astype(np.int64)
    return r  # values at or past +-2^31 saturate; NaN (refused by the library) would give INT_MIN


def rectify_map(K, dist, R, newK, W, H):
    """-> (map1 int16 [H,W,2], map2 uint16 [H,W]).  dist: 4, 5 or 8 coefficients."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = np.asarray(dist, np.float64).reshape(-1)
    assert d.size in (4, 5, 8)
    k1, k2, p1, p2 = d[:4]
    k3 = d[4] if d.size >= 5 else 0.0
    ir = inverse_view(K if newK is None else newK, R)
    i = np.arange(H, dtype=np.float64)[:, None]
    j = np.arange(W, dtype=np.float64)[None, :]
    _x = (i * ir[1] + ir[2]) + j * ir[0]
    _y = (i * ir[4] + ir[5]) + j * ir[3]
    _w = (i * ir[7] + ir[8]) + j * ir[6]
    w = 1.0 / _w
    x, y = _x * w, _y * w
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    if d.size == 8:
        kr = kr / (1 + ((d[7] * r2 + d[6]) * r2 + d[5]) * r2)
    # (the thin-prism terms s1..s4 = 0 stay in the sum, as in OpenCV and oracle/ingest_ref.cpp: they
    # matter only once r2 overflows, where 0 * inf makes the entry NaN -> INT_MIN)
    xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + 0.0 * r2 + 0.0 * r2 * r2
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + 0.0 * r2 + 0.0 * r2 * r2
    iu = _round_sat((K[0, 0] * xd + K[0, 2]) * 32.0)
    iv = _round_sat((K[1, 1] * yd + K[1, 2]) * 32.0)
    map1 = np.stack([iu >> 5, iv >> 5], axis=-1).astype(np.int16)  # the (short) cast wraps
    map2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map1, map2


def remap(src, map1, map2):
    """src u8 [H,W] or [H,W,C] -> same shape.  Taps outside the image read 0."""
    img = src if src.ndim == 3 else src[..., None]
    H, W, _ = img.shape
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    f = map2.astype(np.int64) & 1023
    tx, ty = (f & 31)[..., None], (f >> 5)[..., None]

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(ok[..., None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0).astype(np.int64)

    s = tap(sy, sx) * ((32 - ty) * (32 - tx) * 32) + tap(sy, sx + 1) * ((32 - ty) * tx * 32) + \
        tap(sy + 1, sx) * (ty * (32 - tx) * 32) + tap(sy + 1, sx + 1) * (ty * tx * 32)
    out = np.clip((s + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    return out if src.ndim == 3 else out[..., 0]


def bgr2gray(bgr):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def rectify_gray(src, K, dist, R, newK):
    """src u8 [H,W,3] (bgr8) or [H,W] (mono8) -> gray u8 [H,W]."""
    H, W = src.shape[:2]
    out = remap(src, *rectify_map(K, dist, R, newK, W, H))
    return bgr2gray(out) if src.ndim == 3 and src.shape[2] == 3 else out.reshape(H, W)


def tile_paths(map1, channels, budget=None):
    """bool [tiles_y, tiles_x]: True where the block of that FVO_RECTIFY_TILE_W x _H output tile
    stages its source box in LDS, i.e. ((bw*channels + 6) & ~3) * bh <= budget with
    bw = max(sx) - min(sx) + 2 and bh = max(sy) - min(sy) + 2 over the tile's pixels."""
    tw, th, lds = header_macros()
    budget = lds if budget is None else budget
    H, W = map1.shape[:2]
    out = np.zeros(((H + th - 1) // th, (W + tw - 1) // tw), bool)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            m = map1[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].astype(np.int64)
            bw = int(m[..., 0].max() - m[..., 0].min()) + 2
            bh = int(m[..., 1].max() - m[..., 1].min()) + 2
            out[ty, tx] = ((bw * channels + 6) & ~3) * bh <= budget
    return out
