"""Specification of fvo_registration_icp / fvo_transform_points: Open3D 0.17 ``registration_icp`` with
``TransformationEstimationPointToPoint`` / ``TransformationEstimationPointToPlane`` and
``evaluate_registration``, restated (unpinned: Open3D is not a dependency) in NumPy / plain Python
float64, brute force over all pairs.  This file is the definition; the GPU kernels are compared with
it in tests/test_icp_gpu.py.  Every written operation is one fp64 rounding, no FMA; wherever a result
must match the device bit for bit only + - * / sqrt and comparisons are used (the last
bits of sin / cos / acos differ between libms).

Transform.  s' = T s, always of the *original* source (Open3D transforms the cloud incrementally and
accumulates the roundings: a deviation), x' = ((r00*x + r01*y) + r02*z) + t0 and likewise y', z'.

Correspondence of source i (``KDTreeFlann::SearchHybrid(s', r, 1)``): the target index j that minimises
(d2(s'_i, t_j), j) with d2 = ((dx*dx + dy*dy) + dz*dz), dx = t_j.x - s'_i.x (outlier_ref.pairwise_d2);
kept iff d2 < r*r (strict), else -1.  Equal d2 go to the lower index.

Evaluation: m correspondences, fitness = m / n_source, inlier_rmse = sqrt(sum d2 / m), 0 when m = 0.

Sums.  Coordinates are taken relative to the pivot c, the target's per-axis minimum (exact, order
independent): p = s' - c, q = t - c, n = the target's normal.  SUMS values per pass:
  point-to-plane  d = p - q, r = ((d.x*n.x + d.y*n.y) + d.z*n.z), J = [p x n, n] with
                  p x n = (p.y*n.z - p.z*n.y, p.z*n.x - p.x*n.z, p.x*n.y - p.y*n.x);
                  [0..20] the upper triangle of sum J J^T row by row (J_a*J_b, a <= b), [21..26] sum J_a*r,
                  [27] sum d2.
  point-to-point  [0..2] sum p, [3..5] sum q, [6..14] sum p_a*q_b row by row, [15..26] unused (0),
                  [27] sum d2.
The specification forms every sum with math.fsum (the exact sum, rounded once) and returns sum |term|
beside it; the device's fixed tree is another order of the same terms.

Update from the sums (arithmetic only: reproducible bit for bit), a function of the sums, m, T and c.
  point-to-plane  A x = -b by the 6x6 LDL^T of ldlt6() in its written order (Open3D: ``ldlt``), x = (w, v).
                  Rotation from the Gibbs vector g = w/2, G = [g]x: R = I + (2 / (1 + g.g)) (G + G G),
                  G G = g g^T - (g.g) I.  Open3D composes Euler angles; both agree to O(|w|^3) and have
                  the same fixed point (a deviation of the kind of the Jacobi for FastEigen3x3).
                  A pivot that is not > 0 or not finite, or m = 0: the update is the identity and the
                  status gets DEGENERATE.
  point-to-point  Horn's closed form (Open3D: Umeyama without scale, the same optimum): means pm = sum p
                  / m, qm = sum q / m, M_ab = sum p_a q_b / m - pm_a*qm_b, the symmetric 4x4 N(M), its
                  eigenvector of the largest eigenvalue by the cyclic Jacobi of normals_ref.jacobi over
                  the pairs (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) until the six off-diagonals are
                  exactly 0 (SWEEP_CAP4 sweeps at most; the largest diagonal entry, ties to the lowest
                  index), the quaternion normalised, R from it, v = qm - R pm.  m = 0: as above.
  In both cases the update is x -> c + R (x - c) + v, as a matrix U = [R | (v + c) - R c], and
  T <- U T with the bottom row exactly (0, 0, 0, 1).

Loop (Open3D ``RegistrationICP``): evaluate at init; up to max_iteration times: update, evaluate, stop
when |d fitness| < relative_fitness and |d inlier_rmse| < relative_rmse.  ``iterations`` counts the
updates applied (an identity update counts).  max_iteration = 0 is evaluate_registration."""
from __future__ import annotations

import functools
import math

import numpy as np

import normals_ref
from outlier_ref import duplicates, lattice  # noqa: F401  (the tests' shared inputs)

SUMS = 28
SWEEP_CAP4 = 12      # tests/test_icp_cpu.py records at most 7 sweeps
MAX_ITERATION = 1000  # FVO_ICP_MAX_ITERATION
POINT, PLANE = 0, 1
DEGENERATE = 2       # status bit
# The largest entry-wise spread of the final T between the sums taken by fsum, forward, reversed and
# pairwise (tests/test_icp_cpu.py measures it: 7.8e-16, 1.4e-14, 7.8e-16, 3.5e-14, 1.5e-11, 4.0e-12; the
# far cases carry |c| ~ 1000 in T's last column), rounded up to twice that.  (input, estimation,
# max_iteration) -> figure; tests/test_icp_gpu.py allows the device 1000 x it.
ORDER_SPREAD = {("subset", 1, 30): 1.6e-15, ("subset", 0, 30): 3e-14, ("partial", 1, 30): 1.6e-15,
                ("partial", 0, 10): 7e-14, ("far", 1, 30): 3e-11, ("far", 0, 30): 8e-12}
# max |T - the known motion| of the specification on `subset` (tests/test_icp_cpu.py measures 3.1e-16 and
# 1.9e-15); both test files allow 1000 x it.  estimation -> figure
KNOWN_MOTION_ERR = {1: 3.1e-16, 0: 2.0e-15}


# ------------------------------------------------------------------ transform, search, evaluation
def transform(T, P) -> np.ndarray:
    T = np.asarray(T, np.float64).reshape(4, 4)
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def rotate(T, N) -> np.ndarray:
    """The normals under T: ((r00*x + r01*y) + r02*z) per row."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    N = np.ascontiguousarray(N, np.float64).reshape(-1, 3)
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    return np.stack([(T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z for a in range(3)], axis=1)


def cross_d2(S, Tg) -> np.ndarray:
    """d2[i, j] between S [ns, 3] and Tg [nt, 3]."""
    dx = Tg[None, :, 0] - S[:, None, 0]
    dy = Tg[None, :, 1] - S[:, None, 1]
    dz = Tg[None, :, 2] - S[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def correspondences(Sp, Tg, r):
    """-> (index int32 [ns] (-1: none), d2 f64 [ns] of the kept ones, else 0)."""
    ns = len(Sp)
    if ns == 0 or len(Tg) == 0:
        return np.full(ns, -1, np.int32), np.zeros(ns)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = cross_d2(np.asarray(Sp, np.float64), np.asarray(Tg, np.float64))
        j = np.argmin(np.where(np.isnan(d2), np.inf, d2), axis=1)  # the first minimum: the lower index
        best = d2[np.arange(ns), j]
        r = np.float64(r)
        keep = best < r * r
    return np.where(keep, j, -1).astype(np.int32), np.where(keep, best, 0.0)


def pivot(Tg) -> np.ndarray:
    return np.asarray(Tg, np.float64).reshape(-1, 3).min(axis=0)


def terms(Sp, Tg, Nt, idx, d2, estimation) -> np.ndarray:
    """-> f64 [m, SUMS]: the terms of the docstring for the kept correspondences, in source order."""
    k = np.flatnonzero(idx >= 0)
    out = np.zeros((len(k), SUMS), np.float64)
    if len(k) == 0:
        return out
    c = pivot(Tg)
    p = Sp[k] - c
    q = Tg[idx[k]] - c
    if estimation == PLANE:
        n = np.asarray(Nt, np.float64)[idx[k]]
        d = p - q
        r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        J = [p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
             p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
        o = 0
        for a in range(6):
            for b in range(a, 6):
                out[:, o] = J[a] * J[b]
                o += 1
        for a in range(6):
            out[:, 21 + a] = J[a] * r
    else:
        out[:, 0:3] = p
        out[:, 3:6] = q
        for a in range(3):
            for b in range(3):
                out[:, 6 + 3 * a + b] = p[:, a] * q[:, b]
    out[:, 27] = d2[k]
    return out


def _pairwise(v):
    v = list(v)
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else 0.0


def reduce(tm: np.ndarray, how: str = "fsum"):
    """-> (sums [SUMS], sum |term| [SUMS]).  how: fsum (the definition), or forward / reversed /
    pairwise one-rounding-per-addition orders (tests/test_icp_cpu.py's order sensitivity)."""
    sums = np.zeros(SUMS, np.float64)
    for a in range(SUMS):
        col = tm[:, a].tolist()
        if how == "fsum":
            sums[a] = math.fsum(col)
        elif how == "pairwise":
            sums[a] = _pairwise(col)
        else:
            acc = 0.0
            for v in (col if how == "forward" else reversed(col)):
                acc = acc + v
            sums[a] = acc
    return sums, np.array([math.fsum(np.abs(tm[:, a]).tolist()) for a in range(SUMS)])


def evaluate(source, target, normals, r, T, estimation=POINT, how="fsum") -> dict:
    """One pass at T: correspondences, fitness, inlier_rmse and the sums."""
    Sp = transform(T, source)
    Tg = np.ascontiguousarray(target, np.float64).reshape(-1, 3)
    idx, d2 = correspondences(Sp, Tg, r)
    tm = terms(Sp, Tg, normals, idx, d2, estimation)
    sums, sabs = reduce(tm, how)
    m = len(tm)
    ns = len(Sp)
    fitness = float(m) / float(ns) if ns else 0.0
    rmse = math.sqrt(float(sums[27]) / float(m)) if m else 0.0
    return dict(correspondences=idx, m=m, fitness=fitness, inlier_rmse=rmse, sums=sums, sums_abs=sabs,
                T=np.array(T, np.float64).reshape(4, 4))


# ------------------------------------------------------------------ the update
def ldlt6(A, rhs):
    """A x = rhs for a symmetric 6x6 (only a <= b of A[a][b] is read) -> (x [6], ok).  D_j = A_jj -
    sum_{k<j} (L_jk*L_jk)*D_k in ascending k, one subtraction per term; not (D_j > 0 and finite): not ok;
    L_ij = (A_ji - sum_{k<j} (L_ik*L_jk)*D_k) / D_j; y_i = rhs_i - sum_{k<i} L_ik*y_k; z_i = y_i / D_i;
    x_i = z_i - sum_{k>i} L_ki*x_k, k ascending, i from 5 down."""
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        d = float(A[j][j])
        for k in range(j):
            d = d - (L[j][k] * L[j][k]) * D[k]
        if not (d > 0.0) or math.isinf(d):
            return [0.0] * 6, False
        D[j] = d
        for i in range(j + 1, 6):
            v = float(A[j][i])
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = v / d
    y = [0.0] * 6
    for i in range(6):
        v = float(rhs[i])
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i] / D[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v
    return x, True


def gibbs(w):
    """R [3][3] of the rotation vector w (small angles) through the Gibbs vector g = w / 2."""
    g = [0.5 * float(w[0]), 0.5 * float(w[1]), 0.5 * float(w[2])]
    gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    k = 2.0 / (1.0 + gg)
    G = [[0.0, -g[2], g[1]], [g[2], 0.0, -g[0]], [-g[1], g[0], 0.0]]
    R = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(3):
            GG = g[a] * g[b] - (gg if a == b else 0.0)
            R[a][b] = (1.0 if a == b else 0.0) + k * (G[a][b] + GG)
    return R


def jacobi4(C):
    """normals_ref.jacobi on a symmetric 4x4 over the six pairs -> (diagonal [4], V [4][4], sweeps,
    the off-diagonals left [6])."""
    a = [[float(C[i][j]) for j in range(4)] for i in range(4)]
    v = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
    sweeps = 0
    while sweeps < SWEEP_CAP4 and any(a[p][q] != 0.0 for p, q in pairs):
        for p, q in pairs:
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
            for r in range(4):
                if r == p or r == q:
                    continue
                arp, arq = a[r][p], a[r][q]
                a[r][p] = a[p][r] = c * arp - s * arq
                a[r][q] = a[q][r] = s * arp + c * arq
            for k in range(4):
                vp, vq = v[k][p], v[k][q]
                v[k][p] = c * vp - s * vq
                v[k][q] = s * vp + c * vq
        sweeps += 1
    return [a[i][i] for i in range(4)], v, sweeps, [a[p][q] for p, q in pairs]


def horn(sums, m: int):
    """-> (R [3][3], v [3], sweeps) from the point-to-point sums of m > 0 correspondences."""
    dm = float(m)
    pm = [float(sums[a]) / dm for a in range(3)]
    qm = [float(sums[3 + a]) / dm for a in range(3)]
    M = [[float(sums[6 + 3 * a + b]) / dm - pm[a] * qm[b] for b in range(3)] for a in range(3)]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2]
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2]
    N[2][2] = (M[1][1] - M[0][0]) - M[2][2]
    N[3][3] = (M[2][2] - M[0][0]) - M[1][1]
    N[0][1] = N[1][0] = M[1][2] - M[2][1]
    N[0][2] = N[2][0] = M[2][0] - M[0][2]
    N[0][3] = N[3][0] = M[0][1] - M[1][0]
    N[1][2] = N[2][1] = M[0][1] + M[1][0]
    N[1][3] = N[3][1] = M[2][0] + M[0][2]
    N[2][3] = N[3][2] = M[1][2] + M[2][1]
    d, V, sweeps, _ = jacobi4(N)
    e = 0
    for a in (1, 2, 3):
        if d[a] > d[e]:
            e = a
    w, x, y, z = V[0][e], V[1][e], V[2][e], V[3][e]
    ln = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / ln, x / ln, y / ln, z / ln
    R = [[((w * w + x * x) - y * y) - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
         [2.0 * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, 2.0 * (y * z - w * x)],
         [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((w * w - x * x) - y * y) + z * z]]
    v = [qm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2]) for a in range(3)]
    return R, v, sweeps


def update(sums, m: int, T, c, estimation):
    """-> (the next T f64 [4, 4], degenerate bool, Jacobi sweeps)."""
    T = [[float(v) for v in row] for row in np.asarray(T, np.float64).reshape(4, 4)]
    c = [float(v) for v in c]
    sweeps = 0
    if m == 0:
        return np.array(T), True, 0
    if estimation == PLANE:
        A = [[0.0] * 6 for _ in range(6)]
        o = 0
        for a in range(6):
            for b in range(a, 6):
                A[a][b] = float(sums[o])
                o += 1
        x, ok = ldlt6(A, [-float(sums[21 + a]) for a in range(6)])
        if not ok:
            return np.array(T), True, 0
        R = gibbs(x[0:3])
        v = x[3:6]
    else:
        R, v, sweeps = horn(sums, m)
    U = [[R[a][0], R[a][1], R[a][2], (v[a] + c[a]) - ((R[a][0] * c[0] + R[a][1] * c[1]) + R[a][2] * c[2])]
         for a in range(3)]
    out = np.zeros((4, 4), np.float64)
    for a in range(3):
        for b in range(4):
            s = (U[a][0] * T[0][b] + U[a][1] * T[1][b]) + U[a][2] * T[2][b]
            out[a, b] = s + U[a][3] if b == 3 else s
    out[3, 3] = 1.0
    return out, False, sweeps


# ------------------------------------------------------------------ the loop
def registration(source, target, normals, r, init=None, estimation=POINT, relative_fitness=1e-6,
                 relative_rmse=1e-6, max_iteration=30, how="fsum") -> dict:
    """-> evaluate()'s dict for the final T plus iterations, status and the largest Jacobi sweep count."""
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    c = pivot(target) if len(target) else np.zeros(3)
    ev = evaluate(source, target, normals, r, T, estimation, how)
    iterations, status, most = 0, 0, 0
    for _ in range(int(max_iteration)):
        T, degenerate, sweeps = update(ev["sums"], ev["m"], T, c, estimation)
        most = max(most, sweeps)
        if degenerate:
            status |= DEGENERATE
        iterations += 1
        nxt = evaluate(source, target, normals, r, T, estimation, how)
        done = abs(nxt["fitness"] - ev["fitness"]) < relative_fitness and \
            abs(nxt["inlier_rmse"] - ev["inlier_rmse"]) < relative_rmse
        ev = nxt
        if done:
            break
    ev.update(iterations=iterations, status=status, sweeps=most)
    return ev


# ------------------------------------------------------------------ the inputs the tests share
def _surface(x, y):
    return 5.0 + 0.4 * np.sin(0.9 * x) * np.cos(0.7 * y) + 0.02 * x * x


@functools.lru_cache(maxsize=None)
def bumpy(seed: int = 1) -> np.ndarray:
    """1444 points of a 38 x 38 grid of 0.25 m jittered by +-0.08 m on z = 5 + 0.4 sin(0.9 x) cos(0.7 y) +
    0.02 x^2 + N(0, 0.005), permuted: the surface constrains all six degrees of freedom (the sheet of
    outlier_ref.scene is z = f(x) and slides along y)."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(38), np.arange(38), indexing="ij")
    xy = 0.25 * np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-0.08, 0.08, (1444, 2))
    z = _surface(xy[:, 0], xy[:, 1]) + rng.normal(0.0, 0.005, 1444)
    P = np.ascontiguousarray(np.column_stack([xy, z])[rng.permutation(1444)])
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def bumpy_normals(seed: int = 1) -> np.ndarray:
    """normals_ref.estimate(bumpy, 30, 0.6) flipped to +z."""
    N = normals_ref.estimate(bumpy(seed), 30, 0.6)[0]
    N = np.ascontiguousarray(np.where(N[:, 2:3] < 0.0, -N, N))
    N.setflags(write=False)
    return N


ROTVEC = (0.02, -0.03, 0.04)
TRANSLATION = (0.06, -0.05, 0.04)


def rodrigues(w) -> np.ndarray:
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def motion(center) -> np.ndarray:
    """The known rigid motion x -> center + R (x - center) + t as a 4x4."""
    R = rodrigues(ROTVEC)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = np.asarray(center) - R @ np.asarray(center) + np.asarray(TRANSLATION)
    return M


def _moved_back(P, center) -> np.ndarray:
    Mi = np.linalg.inv(motion(center))
    return np.ascontiguousarray(P @ Mi[:3, :3].T + Mi[:3, 3])


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (source, target, target normals, r, the known motion): the named inputs of the ICP tests,
    read-only.  subset: every second point of bumpy moved by the inverse of motion(); partial: 900
    fresh samples of the surface over x in [3, 12), y in [0, 9.25) with their own noise, moved the same
    way; far: subset with both clouds + 1000 m."""
    Tg, Nt = bumpy(1), bumpy_normals(1)
    center = Tg.mean(axis=0)
    M = motion(center)
    if name == "subset":
        S = _moved_back(Tg[::2], center)
    elif name == "partial":
        rng = np.random.default_rng(5)
        xy = np.column_stack([rng.uniform(3.0, 12.0, 900), rng.uniform(0.0, 9.25, 900)])
        z = _surface(xy[:, 0], xy[:, 1]) + rng.normal(0.0, 0.005, 900)
        S = _moved_back(np.column_stack([xy, z]), center)
    elif name == "far":
        S, Tg0, Nt, r, _ = case("subset")
        S, Tg = np.ascontiguousarray(S + 1000.0), np.ascontiguousarray(Tg0 + 1000.0)
        M = motion(center + 1000.0)
    else:
        raise KeyError(name)
    for a in (S, Tg, Nt, M):
        a.setflags(write=False)
    return S, Tg, Nt, 0.3, M


@functools.lru_cache(maxsize=None)
def solved(name: str, estimation: int, max_iteration: int = 30, how: str = "fsum") -> dict:
    """registration() of a named case with the default criteria, computed once and shared."""
    S, Tg, Nt, r, _ = case(name)
    return registration(S, Tg, Nt, r, None, estimation, 1e-6, 1e-6, max_iteration, how)
