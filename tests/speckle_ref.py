"""Plain restatement of cv2.filterSpeckles (OpenCV 4.x, CV_16SC1) for the tests — flood fill
with an explicit stack, independent of the kernels' method (csrc/speckle.hip uses union-find).

    filter_speckles(img, new_val, max_speckle_size, max_diff) -> filtered copy
    regions(img, new_val, max_diff) -> (labels int32 [H,W] (-1 = no region), sizes list)
    apply(img, labels, sizes, new_val, max_speckle_size) -> filtered copy from known regions

Semantics: a pixel equal to new_val belongs to no region and is never changed; 4-neighbours p, q
are connected when both differ from new_val and abs(int(p) - int(q)) <= max_diff (the difference
in int, not in 16 bits); regions are the connected components of that relation; every pixel of a
region of at most max_speckle_size pixels becomes new_val; max_speckle_size <= 0 changes nothing.
Test infrastructure only."""
from __future__ import annotations

import numpy as np


def regions(img: np.ndarray, new_val: int, max_diff: int):
    img = np.asarray(img)
    assert img.dtype == np.int16 and img.ndim == 2
    H, W = img.shape
    v = img.astype(np.int64).ravel().tolist()  # Python ints: no 16-bit wrap in the difference
    nv, md = int(new_val), int(max_diff)
    lab = [-1] * (H * W)
    sizes = []
    for s in range(H * W):
        if lab[s] >= 0 or v[s] == nv:
            continue
        cur = len(sizes)
        lab[s] = cur
        stack = [s]
        n = 0
        while stack:
            p = stack.pop()
            n += 1
            y, x = divmod(p, W)
            vp = v[p]
            if x + 1 < W:
                q = p + 1
                if lab[q] < 0 and v[q] != nv and abs(vp - v[q]) <= md:
                    lab[q] = cur
                    stack.append(q)
            if x > 0:
                q = p - 1
                if lab[q] < 0 and v[q] != nv and abs(vp - v[q]) <= md:
                    lab[q] = cur
                    stack.append(q)
            if y + 1 < H:
                q = p + W
                if lab[q] < 0 and v[q] != nv and abs(vp - v[q]) <= md:
                    lab[q] = cur
                    stack.append(q)
            if y > 0:
                q = p - W
                if lab[q] < 0 and v[q] != nv and abs(vp - v[q]) <= md:
                    lab[q] = cur
                    stack.append(q)
        sizes.append(n)
    return np.asarray(lab, np.int32).reshape(H, W), sizes


def apply(img: np.ndarray, lab: np.ndarray, sizes, new_val: int, max_speckle_size: int) -> np.ndarray:
    """The filtered copy of img given its regions (one flood fill serves several size limits)."""
    out = np.array(img, dtype=np.int16, copy=True)
    if max_speckle_size <= 0 or out.size == 0:
        return out
    small = np.asarray([n <= max_speckle_size for n in sizes] + [False], bool)  # lab -1 -> the last entry
    out[small[lab]] = np.int16(new_val)
    return out


def filter_speckles(img: np.ndarray, new_val: int, max_speckle_size: int, max_diff: int) -> np.ndarray:
    img = np.asarray(img)
    if max_speckle_size <= 0 or img.size == 0:
        return np.array(img, dtype=np.int16, copy=True)
    lab, sizes = regions(img, new_val, max_diff)
    return apply(img, lab, sizes, new_val, max_speckle_size)
