"""Specification of fvo_statistical_outliers / fvo_radius_outliers / fvo_select_points: Open3D 0.17
``PointCloud::RemoveStatisticalOutliers`` and ``RemoveRadiusOutliers`` restated (unpinned: Open3D is
not a dependency) in NumPy float64, brute force over all pairs.  This file is the definition; the
GPU kernels are compared against it bit for bit (tests/test_outlier_gpu.py).

    d2(i, j) = ((dx*dx + dy*dy) + dz*dz),  dx = p_j.x - p_i.x      (fp64, no contraction)

Statistical (nb_neighbors, std_ratio): k = min(nb_neighbors, n); point i's neighbours are the k
smallest d2(i, j) over all j in [0, n), j = i included (the KD-tree returns the query itself at
distance 0); avg_i = (((0 + sqrt(d2_(0))) + sqrt(d2_(1))) + ...) / (double)k, summed in ascending
order of d2 (equal terms commute, so ties need no rule); valid = n; mean = sum of the avg_i > 0 over
n; std = sqrt(sum of (avg_i - mean)^2 over the avg_i > 0, over n - 1); thr = mean + std_ratio * std;
keep_i = avg_i > 0 and avg_i < thr.  A point whose k nearest all coincide with it has avg = 0: it
is dropped and is in neither sum.  With n = 1, std is 0/0 and nothing is kept.  The two global sums
are formed with math.fsum.

Radius (nb_points, radius): r2 = radius*radius; count_i = #{j : d2(i, j) < r2} (strict, as
nanoflann's radius result set adds a point; j = i included); keep_i = count_i > nb_points."""
from __future__ import annotations

import math

import numpy as np


def pairwise_d2(points: np.ndarray) -> np.ndarray:
    """d2[i, j] of the docstring for float64 [n, 3] points."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    dx = p[None, :, 0] - p[:, None, 0]
    dy = p[None, :, 1] - p[:, None, 1]
    dz = p[None, :, 2] - p[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def avg_distances(points: np.ndarray, nb_neighbors: int) -> np.ndarray:
    d2 = pairwise_d2(points)
    n = d2.shape[0]
    k = min(int(nb_neighbors), n)
    near = np.sqrt(np.sort(d2, axis=1)[:, :k])
    s = np.zeros(n, np.float64)
    for c in range(k):  # ascending order of d2, one rounding per term
        s = s + near[:, c]
    return s / np.float64(k)


def statistical(points: np.ndarray, nb_neighbors: int, std_ratio: float):
    """-> (keep bool [n], avg f64 [n], stats f64 [5] = mean, std, thr, valid, kept)."""
    avg = avg_distances(points, nb_neighbors)
    n = len(avg)
    pos = avg[avg > 0.0]
    mean = np.float64(math.fsum(pos.tolist())) / np.float64(n)
    dev = ((pos - mean) * (pos - mean)).tolist()
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(np.float64(math.fsum(dev)) / np.float64(n - 1))
    thr = mean + np.float64(std_ratio) * std
    keep = (avg > 0.0) & (avg < thr)
    return keep, avg, np.array([mean, std, thr, n, keep.sum()], np.float64)


def radius(points: np.ndarray, nb_points: int, radius_: float):
    """-> (keep bool [n], count int32 [n])."""
    r = np.float64(radius_)
    count = (pairwise_d2(points) < r * r).sum(axis=1).astype(np.int32)
    return count > int(nb_points), count


def scene(seed: int):
    """1400 points on a jittered 0.5 m sheet, z = 5 + 0.3 sin x + N(0, 0.03), plus 40 uniform flyers
    in a 30 x 27 x 30 m box, permuted.  -> (points f64 [1440, 3], is_flyer bool [1440])."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(40), np.arange(35), indexing="ij")
    xy = 0.5 * np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-0.15, 0.15, (1400, 2))
    z = 5.0 + 0.3 * np.sin(xy[:, 0]) + rng.normal(0.0, 0.03, 1400)
    sheet = np.column_stack([xy, z])
    fly = rng.uniform([-5.0, -5.0, -10.0], [25.0, 22.0, 20.0], (40, 3))
    pts = np.concatenate([sheet, fly]).astype(np.float64)
    flyer = np.arange(1440) >= 1400
    perm = rng.permutation(1440)
    return np.ascontiguousarray(pts[perm]), flyer[perm]


def lattice(nx: int, ny: int, nz: int) -> np.ndarray:
    """The unit lattice [0, nx) x [0, ny) x [0, nz) as float64 [n, 3]."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1)
    return np.ascontiguousarray(g.reshape(-1, 3).astype(np.float64))


def duplicates(seed: int = 3) -> np.ndarray:
    """30 copies of one point among 200 others (k <= 30: the copies have avg = 0)."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.0, 6.0, (230, 3))
    pts[rng.choice(230, 30, replace=False)] = np.array([2.5, 3.25, 1.125])
    return np.ascontiguousarray(pts)


def margin_to_threshold(avg: np.ndarray, thr: float) -> float:
    """The closest any avg comes to thr, relative to thr (the GPU mask comparison is unconditional
    when this is far above the sums' error)."""
    return float(np.min(np.abs(avg - thr)) / thr) if thr > 0 else float("inf")
