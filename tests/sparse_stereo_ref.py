"""The specification of sparse stereo (fvo_sparse_stereo, fvo_backproject_stereo) in NumPy.

Per rectified pair: every left ORB keypoint is matched to a right keypoint on its own row band by
descriptor, the match is refined to sub-pixel by a SAD search on the level-0 images and written as
the per-keypoint stereo record (X, Y, Z, d) that fvo_keypoint_stereo produces from a disparity map.
All float arithmetic is float32, in the order written here; the SADs are integers.

Candidates.  Right keypoint j is a candidate of left keypoint i iff
    both octaves (record field 5) are integers in [0, n_levels),
    fabsf(yR - yL) <= row_tol * level_scale[oL],
    |oR - oL| <= max_octave_diff,
    min_disparity <= xL - xR <= max_disparity
(a non-finite coordinate fails the comparisons).  The best candidate is the minimum of
(hamming << 16) | j; it is accepted iff hamming <= max_hamming, else STATUS_NO_MATCH.

Uniqueness (unique != 0).  Of the left keypoints whose accepted best candidate is j, the one with
the smallest (hamming << 16) | i keeps it; the others get STATUS_NOT_UNIQUE.  This is decided
before the refinement: a winner that fails later does not hand j on.

Refinement on the level-0 images.  xl = floorf(xL + 0.5f), yl from yL, xr from xR.  The (2w+1)^2
window around (xl, yl) and the 2S+1 windows around (xr + k, yl), |k| <= S, must lie inside the
image (checked on the float32 values, which are whole numbers, before they become ints), else
STATUS_BORDER.  SAD(k) = sum |L(yl+dy, xl+dx) - R(yl+dy, xr+k+dx)|; k* is its first minimum;
k* = +-S: STATUS_SLIDE_END.  With d1, d2, d3 = SAD(k*-1), SAD(k*), SAD(k*+1):
    delta = (float)(d1 - d3) / (float)(2 * (d1 + d3 - 2 * d2))     (denominator >= 2, |delta| <= 0.5)
    d = xL - ((float)(xr + k*) + delta)
d outside [min_disparity, max_disparity]: STATUS_DISPARITY.  Z = (float)(K[0,0] * baseline) / d,
X = ((xL - cx) / fx) * Z, Y = ((yL - cy) / fy) * Z (oracle.backproject's expressions); unless
0.1 < Z < 1000: STATUS_DEPTH.

stereo row = (X, Y, Z, d), zeros for every status != 0.  info row = (right index, hamming, k*,
status); right index and hamming are -1 under STATUS_NO_MATCH, k* is 0 under statuses 1-3.
"""
from dataclasses import dataclass

import numpy as np

STATUS_OK, STATUS_NO_MATCH, STATUS_NOT_UNIQUE, STATUS_BORDER, STATUS_SLIDE_END, STATUS_DISPARITY, STATUS_DEPTH = range(7)
NO_KEY = 0xFFFFFFFF
f32 = np.float32


@dataclass
class Params:
    min_disparity: float = 1.0
    max_disparity: float = 96.0
    row_tol: float = 2.0
    max_hamming: int = 75
    max_octave_diff: int = 1
    half_window: int = 5
    half_slide: int = 5
    unique: int = 1


_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def level_scales(scale_factor=1.2, n_levels=8):
    """The table both sides take as given: float32(scale_factor ** o)."""
    return np.array([f32(float(scale_factor) ** o) for o in range(n_levels)], f32)


def hamming_matrix(dL, dR):
    return _POP[dL[:, None, :] ^ dR[None, :, :]].sum(-1, dtype=np.int64)


def _octaves(kp, n_levels):
    o = kp[:, 5]
    with np.errstate(invalid="ignore"):
        ok = (o >= f32(0)) & (o < f32(n_levels)) & (o == np.floor(o))
    return np.where(ok, o, f32(-1)).astype(np.int64)


def best_candidates(kpL, descL, kpR, descR, p, level_scale):
    """uint32 key (hamming << 16 | j) of every left keypoint's best candidate, NO_KEY without one."""
    nL, nR = len(kpL), len(kpR)
    if nL == 0 or nR == 0:
        return np.full(nL, NO_KEY, np.int64)
    level_scale = np.asarray(level_scale, f32)
    oL, oR = _octaves(kpL, len(level_scale)), _octaves(kpR, len(level_scale))
    xL, yL, xR, yR = kpL[:, 0].astype(f32), kpL[:, 1].astype(f32), kpR[:, 0].astype(f32), kpR[:, 1].astype(f32)
    band = f32(p.row_tol) * level_scale[np.maximum(oL, 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        d0 = xL[:, None] - xR[None, :]
        cand = ((oL >= 0)[:, None] & (oR >= 0)[None, :] & (np.abs(yR[None, :] - yL[:, None]) <= band[:, None]) &
                (np.abs(oR[None, :] - oL[:, None]) <= p.max_octave_diff) & (d0 >= f32(p.min_disparity)) &
                (d0 <= f32(p.max_disparity)))
    key = (hamming_matrix(descL, descR) << 16) | np.arange(nR, dtype=np.int64)[None, :]
    return np.where(cand, key, NO_KEY).min(axis=1)


def sparse_stereo(imgL, imgR, kpL, descL, kpR, descR, K, baseline, p=None, level_scale=None):
    """One pair.  imgL/imgR u8 [H,W]; kp* f32 [n, >= 6]; desc* u8 [n,32].  Returns (stereo f32
    [nL,4], info int32 [nL,4])."""
    p = p or Params()
    level_scale = level_scales() if level_scale is None else np.asarray(level_scale, f32)
    kpL, kpR = np.asarray(kpL, f32), np.asarray(kpR, f32)
    nL = len(kpL)
    H, W = imgL.shape
    stereo = np.zeros((nL, 4), f32)
    info = np.zeros((nL, 4), np.int32)
    info[:, :2] = -1
    info[:, 3] = STATUS_NO_MATCH
    key = best_candidates(kpL, descL, kpR, descR, p, level_scale)
    acc = (key != NO_KEY) & ((key >> 16) <= p.max_hamming)
    idx = np.nonzero(acc)[0]
    j_of, ham_of = key & 0xFFFF, key >> 16
    colkey = np.full(max(len(kpR), 1), NO_KEY, np.int64)
    np.minimum.at(colkey, j_of[idx], (ham_of[idx] << 16) | idx)
    fxB = f32(K[0, 0] * baseline)
    fx, fy, cx, cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
    w, S = p.half_window, p.half_slide
    iL, iR = imgL.astype(np.int32), imgR.astype(np.int32)
    for i in idx:
        j, ham = int(j_of[i]), int(ham_of[i])
        info[i] = (j, ham, 0, STATUS_OK)
        if p.unique and (colkey[j] & 0xFFFF) != i:
            info[i, 3] = STATUS_NOT_UNIQUE
            continue
        xL, yL, xR = f32(kpL[i, 0]), f32(kpL[i, 1]), f32(kpR[j, 0])
        fxl, fyl, fxr = np.floor(xL + f32(0.5)), np.floor(yL + f32(0.5)), np.floor(xR + f32(0.5))
        fw, fs = f32(w), f32(S + w)
        if not (fxl - fw >= 0 and fxl + fw <= f32(W - 1) and fyl - fw >= 0 and fyl + fw <= f32(H - 1) and
                fxr - fs >= 0 and fxr + fs <= f32(W - 1)):
            info[i, 3] = STATUS_BORDER
            continue
        xl, yl, xr = int(fxl), int(fyl), int(fxr)
        Lw = iL[yl - w:yl + w + 1, xl - w:xl + w + 1]
        sad = [int(np.abs(Lw - iR[yl - w:yl + w + 1, xr + k - w:xr + k + w + 1]).sum()) for k in range(-S, S + 1)]
        kb = int(np.argmin(sad))  # the first minimum
        info[i, 2] = kb - S
        if kb == 0 or kb == 2 * S:
            info[i, 3] = STATUS_SLIDE_END
            continue
        d1, d2, d3 = sad[kb - 1], sad[kb], sad[kb + 1]
        delta = f32(d1 - d3) / f32(2 * (d1 + d3 - 2 * d2))
        d = xL - (f32(xr + kb - S) + delta)
        if not (d >= f32(p.min_disparity) and d <= f32(p.max_disparity)):
            info[i, 3] = STATUS_DISPARITY
            continue
        Z = fxB / d
        X = ((xL - cx) / fx) * Z
        Y = ((yL - cy) / fy) * Z
        if not (Z > f32(0.1) and Z < f32(1000)):
            info[i, 3] = STATUS_DEPTH
            continue
        stereo[i] = (X, Y, Z, d)
    return stereo, info


def backproject_stereo(stereo, kp1, matches):
    """fvo_backproject_stereo of one frame: the records of the matches' query keypoints with
    Z != 0, in match order.  Returns (P3 f32 [n,3], p2 f32 [n,2], kept mask)."""
    rec = stereo[matches[:, 0]]
    keep = rec[:, 2] != 0
    return rec[keep, :3].astype(f32), kp1[matches[:, 1], :2][keep].astype(f32), keep
