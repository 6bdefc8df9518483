"""Deterministic local-BA problems for the tests (helper module, not a test file).

`clean_problem` builds a stereo VO window with known geometry: landmarks in front of a
forward-moving camera, keypoints = projections + Gaussian noise scaled by a random ORB
octave, one-to-one matches between consecutive frames, stereo disparities with noise,
and relative poses perturbed from the truth (the "PnP" initial guess).  Arrays come in
the frame layout of fvo_ba_windows (keypoint records of 8 floats, match rows, per-keypoint
stereo (X, Y, Z, d)) and in the list layout of oracle/ba_ref.py.
"""
import numpy as np

K_TEST = np.array([[428.6, 0.0, 306.8], [0.0, 428.0, 205.7], [0.0, 0.0, 1.0]])
B_TEST = 0.2537


def _expso3(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def clean_problem(n=10, n_pts=3000, seed=0, W=640, H=400, cap=4096, pose_noise=0.03, drop=0.0, K=None, B=None,
                  octaves=(0, 3), one_to_one=True):
    """K, B: the camera (K_TEST, B_TEST when None); the stereo points are made with the same one.
    octaves: the half-open range the keypoint octaves are drawn from.  one_to_one=False keeps the
    duplicate train indices that the outlier matches of drop > 0 produce (a ratio-test match list
    without cross-check); every query index still appears at most once per frame."""
    rng = np.random.default_rng(seed)
    K = K_TEST if K is None else np.asarray(K, np.float64)
    B = B_TEST if B is None else float(B)
    Tg = [np.eye(4)]
    for _ in range(n - 1):
        T = np.eye(4)
        T[:3, :3] = _expso3(rng.normal(0, 0.01, 3))
        T[:3, 3] = [0.01, 0.0, -0.15]
        Tg.append(T @ Tg[-1])
    Tg = np.array(Tg)
    Xw = np.c_[rng.uniform(-8, 8, n_pts), rng.uniform(-3, 2, n_pts), rng.uniform(3, 30, n_pts)]
    kp = np.zeros((n, cap, 8), np.float32)
    nkp = np.zeros(n, np.int32)
    proj = []
    for j in range(n):
        Xc = (Tg[j][:3, :3] @ Xw.T).T + Tg[j][:3, 3]
        u = K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2]
        v = K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]
        vis = (Xc[:, 2] > 0.5) & (u >= 0) & (u < W - 1) & (v >= 0) & (v < H - 1)
        if drop > 0:
            vis &= rng.random(n_pts) >= drop
        idx = np.nonzero(vis)[0][:cap]
        octv = rng.integers(octaves[0], octaves[1], len(idx))
        sc = 1.2 ** octv
        kp[j, :len(idx), 0] = u[idx] + rng.normal(0, 0.5, len(idx)) * sc
        kp[j, :len(idx), 1] = v[idx] + rng.normal(0, 0.5, len(idx)) * sc
        kp[j, :len(idx), 5] = octv
        kp[j, :len(idx), 6] = -1
        nkp[j] = len(idx)
        proj.append(idx)
    matches = np.zeros((n, cap, 3), np.int32)
    nmatch = np.zeros(n, np.int32)
    stereo = np.zeros((n, cap, 4), np.float32)
    f32 = np.float32
    for j in range(n - 1):
        pos = {p: i for i, p in enumerate(proj[j + 1])}
        rows = [(i, pos[p], 0) for i, p in enumerate(proj[j]) if p in pos]
        if drop > 0:  # some outlier matches
            rows = [(a, (b + 7) % nkp[j + 1], c) if rng.random() < drop else (a, b, c) for a, b, c in rows]
            seen, uniq = set(), []
            for a, b, c in rows:  # keep the one-to-one property of cross-checked matching
                if b not in seen or not one_to_one:
                    seen.add(b)
                    uniq.append((a, b, c))
            rows = uniq
        m = np.array(rows, np.int32).reshape(-1, 3)
        matches[j, :len(m)] = m
        nmatch[j] = len(m)
        Xc = (Tg[j][:3, :3] @ Xw[proj[j]].T).T + Tg[j][:3, 3]
        d = (K[0, 0] * B / Xc[:, 2] + rng.normal(0, 0.3, len(Xc))).astype(f32)
        Z = f32(K[0, 0] * B) / d
        x, y = kp[j, :len(d), 0], kp[j, :len(d), 1]
        X = ((x - f32(K[0, 2])) / f32(K[0, 0])) * Z
        Y = ((y - f32(K[1, 2])) / f32(K[1, 1])) * Z
        ok = (Z > f32(0.1)) & (Z < f32(1000))
        stereo[j, :len(d)] = np.where(ok[:, None], np.stack([X, Y, Z, d], 1), 0).astype(f32)
    relg = np.array([Tg[j + 1] @ np.linalg.inv(Tg[j]) for j in range(n - 1)])
    relp = relg.copy()
    for j in range(n - 1):
        relp[j, :3, 3] += rng.normal(0, pose_noise, 3)
        relp[j, :3, :3] = _expso3(rng.normal(0, pose_noise / 6, 3)) @ relp[j, :3, :3]
    T_rel = np.zeros((n, 4, 4))
    T_rel[:n - 1] = relp
    T_rel[n - 1] = np.eye(4)
    return dict(kp=kp, nkp=nkp, matches=matches, nmatch=nmatch, stereo=stereo, T_rel=T_rel, relg=relg, K=K, B=B)


# ---- edits of a problem in place (tests/ba_cases.py).  Every edit keeps the preconditions of
# fvo_ba_windows: match indices inside [0, n_keypoints) of their frames, a query index at most once
# per frame.
def empty_matches(p, f):
    """Frame f has no match rows to frame f + 1 (every track breaks there)."""
    p["nmatch"][f] = 0


def empty_keypoints(p, f):
    """Frame f has no keypoints, hence no match rows into it or out of it."""
    p["nkp"][f] = 0
    p["nmatch"][f] = 0
    if f > 0:
        p["nmatch"][f - 1] = 0


def invalidate_stereo(p, f):
    """Every stereo point of frame f fails 0.1 < Z < 1000 (stored as zeros): no landmark is born there."""
    p["stereo"][f] = 0


def add_duplicate_train(p, f, count, seed=0):
    """`count` match rows of frame f get the train index of another row of the frame."""
    rng = np.random.default_rng(seed)
    M = int(p["nmatch"][f])
    rows = rng.choice(M, size=2 * count, replace=False)
    p["matches"][f, rows[:count], 1] = p["matches"][f, rows[count:], 1]


def set_octaves(p, f, octaves):
    """The octaves of frame f's keypoints, cycling through `octaves`."""
    n = int(p["nkp"][f])
    p["kp"][f, :n, 5] = np.resize(np.asarray(octaves, np.float32), n)


def poison(p, frames, seed=99):
    """Overwrite the frames `frames`, and in every other frame the rows beyond nkp[f] / nmatch[f],
    with data that is safe to read but wrong: keypoints inside the image with octaves 0..2, finite
    stereo points with a valid depth, match rows of shuffled indices in [0, cap) (each query index
    once), nkp = nmatch = cap and another rigid transform in T_rel.  A solver that reads any of it
    computes something else; none of it can make a read leave the arrays."""
    rng = np.random.default_rng(seed)
    F, cap = p["kp"].shape[:2]
    f32 = np.float32

    def rows(n):
        kp = np.zeros((n, 8), f32)
        kp[:, 0] = rng.uniform(1, 600, n)
        kp[:, 1] = rng.uniform(1, 380, n)
        kp[:, 5] = rng.integers(0, 3, n)
        kp[:, 6] = -1
        Z = rng.uniform(2, 40, n)
        st = np.stack([rng.uniform(-5, 5, n), rng.uniform(-3, 3, n), Z, 100.0 / Z], 1).astype(f32)
        m = np.stack([rng.permutation(cap)[:n], rng.integers(0, cap, n), np.zeros(n, np.int64)], 1).astype(np.int32)
        return kp, st, m

    for f in range(F):
        if f in frames:
            p["kp"][f], p["stereo"][f], p["matches"][f] = rows(cap)
            p["nkp"][f] = p["nmatch"][f] = cap
            T = np.eye(4)
            T[:3, :3] = _expso3(rng.normal(0, 0.3, 3))
            T[:3, 3] = rng.normal(0, 1.0, 3)
            p["T_rel"][f] = T
        else:
            nk, nm = int(p["nkp"][f]), int(p["nmatch"][f])
            kp, st, m = rows(cap)
            p["kp"][f, nk:], p["stereo"][f, nk:], p["matches"][f, nm:] = kp[nk:], st[nk:], m[nm:]
    return p


def oracle_lists(p, s, e):
    """Frames s..e of a frame-layout problem in oracle/ba_ref.py's list layout."""
    kps = [p["kp"][f, :p["nkp"][f], :6] for f in range(s, e + 1)]
    matches = [p["matches"][f, :p["nmatch"][f]] for f in range(s, e)]
    st = []
    for f in range(s, e):
        a = p["stereo"][f, :p["nkp"][f]]
        st.append((a[:, :3], a[:, 3], a[:, 2] > 0))
    return kps, matches, st, p["T_rel"][s:e]
