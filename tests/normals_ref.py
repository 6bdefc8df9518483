"""Specification of fvo_estimate_normals / fvo_orient_normals: Open3D 0.17 ``PointCloud::EstimateNormals``,
``EstimateCovariances``, ``OrientNormalsTowardsCameraLocation`` and ``OrientNormalsToAlignWithDirection``
restated (unpinned: Open3D is not a dependency) in NumPy / plain Python float64, brute force over all
pairs.  This file is the definition; the GPU kernels are compared against it bit for bit
(tests/test_normals_gpu.py).  Every operation is one fp64 rounding, no FMA.

    d2(i, j) = ((dx*dx + dy*dy) + dz*dz),  dx = p_j.x - p_i.x          (outlier_ref.pairwise_d2)

Neighbours of i (``KDTreeSearchParamHybrid(radius, max_nn)``; radius = inf: ``KDTreeSearchParamKNN``):
all j in [0, n), j = i included, ordered by (d2(i, j), j); the first min(max_nn, n) of them, and of
those the ones with d2 < radius*radius (strict, as nanoflann's result set and ``SearchHybrid``); m_i is
their number.  Equal d2 at the cut: the lower index (Open3D leaves it to the KD-tree's traversal).

Covariance (``utility::ComputeCovariance``): nine cumulants x, y, z, xx, xy, xz, yy, yz, zz summed over
the neighbours in that order, ``cum = cum + term`` with term one product of raw coordinates (the
cancellation far from the origin is Open3D's and is reproduced), each divided by (double)m_i;
C00 = c3 - c0*c0, C01 = c4 - c0*c1, C02 = c5 - c0*c2, C11 = c6 - c1*c1, C12 = c7 - c1*c2, C22 = c8 -
c2*c2, symmetric.  m_i < 3: C = I.

Normal: (0, 0, 1) when m_i < 3 or every C_ab is 0.  Otherwise a cyclic Jacobi eigen-solve (Open3D's
analytic ``FastEigen3x3`` needs acos and cos, whose last bits differ between libms; this needs + - * /
sqrt and comparisons only): sweeps over the pairs (0,1), (0,2), (1,2); a pair with a_pq == 0 is skipped,
else th = (a_qq - a_pp) / (2*a_pq), t = 1 / (|th| + sqrt(th*th + 1)) negated when th < 0, c = 1 /
sqrt(t*t + 1), s = t*c, a_pp -= t*a_pq, a_qq += t*a_pq, a_pq = 0, and with r the third index a_rp' =
c*a_rp - s*a_rq, a_rq' = s*a_rp + c*a_rq; the columns p, q of V (from I) are rotated the same way.  The
solve stops when the three off-diagonals are exactly 0, after SWEEP_CAP sweeps at most.  The eigenvalue
is the smallest diagonal entry (ties: the lowest index), the normal that column of V divided by
sqrt((x*x + y*y) + z*z).

Prior ("a cloud that has normals keeps their side"): with a prior o_i an all-zero result becomes o_i,
any other is negated when ((n.x*o.x + n.y*o.y) + n.z*o.z) < 0.

Orientation: ref = c - p (camera location c) or ref = d (direction); a normal with all components 0
becomes ref / sqrt((x*x + y*y) + z*z), or (0, 0, 1) when ref is all zeros; any other is negated when
((n.x*ref.x + n.y*ref.y) + n.z*ref.z) < 0."""
from __future__ import annotations

import math

import numpy as np

from outlier_ref import duplicates, lattice, pairwise_d2, scene  # noqa: F401  (the tests' shared inputs)

SWEEP_CAP = 10


def neighbours(points: np.ndarray, max_nn: int, radius: float = math.inf):
    """-> (order int64 [n, k]: row i's first k = min(max_nn, n) points by (d2, index), m int32 [n]:
    how many of them have d2 < radius^2 — the neighbours are order[i, :m[i]])."""
    d2 = pairwise_d2(points)
    n = d2.shape[0]
    k = min(int(max_nn), n)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]  # stable: equal d2 stay in index order
    r = np.float64(radius)
    m = (np.take_along_axis(d2, order, axis=1) < r * r).sum(axis=1).astype(np.int32)
    return order, m


def covariances(points: np.ndarray, order: np.ndarray, m: np.ndarray) -> np.ndarray:
    """-> C f64 [n, 3, 3] from the neighbours order[i, :m[i]]."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = p.shape[0]
    cum = np.zeros((9, n), np.float64)
    for c in range(order.shape[1]):  # the neighbours in order, one rounding per term
        q = p[order[:, c]]
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        terms = (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)
        live = c < m
        for a in range(9):
            cum[a] = np.where(live, cum[a] + terms[a], cum[a])
    with np.errstate(invalid="ignore", divide="ignore"):
        cum = cum / m.astype(np.float64)
    C = np.empty((n, 3, 3), np.float64)
    C[:, 0, 0] = cum[3] - cum[0] * cum[0]
    C[:, 0, 1] = C[:, 1, 0] = cum[4] - cum[0] * cum[1]
    C[:, 0, 2] = C[:, 2, 0] = cum[5] - cum[0] * cum[2]
    C[:, 1, 1] = cum[6] - cum[1] * cum[1]
    C[:, 1, 2] = C[:, 2, 1] = cum[7] - cum[1] * cum[2]
    C[:, 2, 2] = cum[8] - cum[2] * cum[2]
    C[m < 3] = np.eye(3)
    return C


def jacobi(C):
    """The cyclic Jacobi of the docstring on one symmetric 3x3 (anything indexable [a][b]) in plain
    Python floats -> (diagonal [3], V [3][3], sweeps done, the off-diagonals left [3])."""
    a = [[float(C[i][j]) for j in range(3)] for i in range(3)]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    sweeps = 0
    while sweeps < SWEEP_CAP and not (a[0][1] == 0.0 and a[0][2] == 0.0 and a[1][2] == 0.0):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            th = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(th) + math.sqrt(th * th + 1.0))
            if th < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            for k in range(3):
                vp, vq = v[k][p], v[k][q]
                v[k][p] = c * vp - s * vq
                v[k][q] = s * vp + c * vq
        sweeps += 1
    return [a[0][0], a[1][1], a[2][2]], v, sweeps, [a[0][1], a[0][2], a[1][2]]


def normal_of(C, m: int):
    """-> (normal [3], eigenvalue, sweeps): the docstring's normal of one covariance with m neighbours."""
    if m < 3 or not np.any(np.asarray(C) != 0.0):
        return [0.0, 0.0, 1.0], math.nan, 0
    d, v, sweeps, _ = jacobi(C)
    e = 0
    for a in (1, 2):
        if d[a] < d[e]:
            e = a
    x, y, z = v[0][e], v[1][e], v[2][e]
    ln = math.sqrt((x * x + y * y) + z * z)
    return [x / ln, y / ln, z / ln], d[e], sweeps


def estimate(points: np.ndarray, max_nn: int = 30, radius: float = math.inf, prior: np.ndarray | None = None):
    """-> (normals f64 [n, 3], covariances f64 [n, 3, 3], m int32 [n], sweeps int [n])."""
    order, m = neighbours(points, max_nn, radius)
    C = covariances(points, order, m)
    n = len(m)
    N = np.empty((n, 3), np.float64)
    sweeps = np.zeros(n, np.int64)
    for i in range(n):
        nrm, _, sweeps[i] = normal_of(C[i], int(m[i]))
        if prior is not None:
            o = [float(t) for t in prior[i]]
            if nrm[0] == 0.0 and nrm[1] == 0.0 and nrm[2] == 0.0:
                nrm = o
            elif (nrm[0] * o[0] + nrm[1] * o[1]) + nrm[2] * o[2] < 0.0:
                nrm = [-nrm[0], -nrm[1], -nrm[2]]
        N[i] = nrm
    return N, C, m, sweeps


def orient(points: np.ndarray, normals: np.ndarray, camera=None, direction=None) -> np.ndarray:
    """Exactly one of camera / direction -> the oriented normals f64 [n, 3] (a new array)."""
    assert (camera is None) != (direction is None)
    out = np.array(normals, np.float64)
    for i in range(len(out)):
        if camera is not None:
            ref = [float(camera[a]) - float(points[i][a]) for a in range(3)]
        else:
            ref = [float(direction[a]) for a in range(3)]
        x, y, z = (float(t) for t in out[i])
        if x == 0.0 and y == 0.0 and z == 0.0:
            if ref[0] == 0.0 and ref[1] == 0.0 and ref[2] == 0.0:
                out[i] = [0.0, 0.0, 1.0]
            else:
                ln = math.sqrt((ref[0] * ref[0] + ref[1] * ref[1]) + ref[2] * ref[2])
                out[i] = [ref[0] / ln, ref[1] / ln, ref[2] / ln]
        elif (x * ref[0] + y * ref[1]) + z * ref[2] < 0.0:
            out[i] = [-x, -y, -z]
    return out


# ------------------------------------------------------------------ the inputs the tests share
def plane() -> np.ndarray:
    """600 points with dyadic coordinates (multiples of 1/16) on z = 0.25 x + 0.5 y inside [0, 16)^2:
    every coordinate, product and partial sum of the cumulants is exact in fp64."""
    rng = np.random.default_rng(11)
    xy = rng.integers(0, 256, (600, 2)).astype(np.float64) / 16.0
    return np.ascontiguousarray(np.column_stack([xy, 0.25 * xy[:, 0] + 0.5 * xy[:, 1]]))


def collinear() -> np.ndarray:
    """40 points on the line (1, 2, 0.5) + t (0.5, 0.25, 1), t = 0 .. 39."""
    t = np.arange(40, dtype=np.float64)[:, None]
    return np.ascontiguousarray(np.array([1.0, 2.0, 0.5]) + t * np.array([0.5, 0.25, 1.0]))


def cloud(name: str) -> np.ndarray:
    """The named inputs of tests/test_normals_cpu.py and tests/test_normals_gpu.py."""
    kind, _, arg = name.partition(":")
    if kind == "scene":
        return scene(int(arg))[0]
    if kind == "far":  # scene 1 moved by 1000 on every coordinate
        return np.ascontiguousarray(scene(1)[0] + 1000.0)
    if kind == "f32":  # scene 1 rounded to float32, as a map built from float32 clouds holds it
        return np.ascontiguousarray(scene(1)[0].astype(np.float32).astype(np.float64))
    if kind == "lattice":
        return lattice(12, 12, 10)
    if kind == "dup":
        return duplicates()
    if kind == "line":
        return collinear()
    if kind == "plane":
        return plane()
    if kind == "head":  # the first n points of scene 1
        return np.ascontiguousarray(scene(1)[0][:int(arg)])
    raise KeyError(name)


# (input, max_nn, radius) of every bit-for-bit comparison on the GPU
CASES = ([("scene:1", k, math.inf) for k in (3, 10, 30, 32, 33, 64)] + [("scene:1", 30, 0.8), ("scene:1", 30, 0.3),
         ("scene:1", 64, 0.8), ("far", 30, math.inf), ("f32", 30, math.inf), ("f32", 30, 0.8), ("lattice", 7, math.inf), ("lattice", 27, math.inf), ("lattice", 30, math.inf),
         ("lattice", 30, 1.0), ("lattice", 30, 1.5), ("dup", 30, math.inf), ("dup", 31, math.inf),
         ("line", 10, math.inf), ("plane", 30, math.inf), ("head:1", 30, math.inf), ("head:2", 30, math.inf),
         ("head:3", 30, math.inf), ("head:20", 30, math.inf)])
