"""Inputs, call parameters and cached oracle outputs shared by the pose parameter tests
(test_pose_params_gpu.py on the GPU, test_pose_cases_cpu.py without one): PnP-RANSAC,
the essential-matrix RANSAC + recoverPose, and the back-projection of matched keypoints.

NumPy only.  Every case is a dict with a name, its inputs, the call parameters and `reach`,
the branch of the implementation it is meant to reach; test_pose_cases_cpu.py asserts that
the oracle takes that branch, so a badly chosen input fails there and not silently on the GPU.

UNSTABLE_PNP / UNSTABLE_EM list the cases whose oracle result moves when the inputs move by
one float32 ulp (classify_pnp / classify_em; the CPU test recomputes the classification and
compares it with these sets).  For those cases two correct implementations need not agree, and
the GPU tests assert only the status, finite outputs and a mask inside [0, n).
"""
import functools

import numpy as np

import mono_cases as mc

# forest_slam_amd.synth.K0 / DIST_L / BASELINE (stereo_slam.py:45-64); the CPU test compares them
K = np.array([[642.9165664800531, 0.0, 460.1840658156501],
              [0.0, 641.9171825800378, 308.5846449100310],
              [0.0, 0.0, 1.0]])
DIST = np.array([-0.060164620903866, 0.094005180631043, 0.0, 0.0, 0.0])
BASELINE = 0.253736175410149

PNP_DEFAULTS = dict(reproj=1.0, confidence=0.99, iterations=1000)
EM_DEFAULTS = dict(prob=0.999, threshold=1.0, max_iters=1000)
PNP_FIRST = 128  # iterations of RANSAC round 1 (csrc/pose.hip PNP_FIRST, csrc/essential.hip)

# the only cases that may be unstable (the degenerate ones), and those that are
MAY_BE_UNSTABLE_PNP = frozenset({"all_identical", "duplicated_half", "collinear"})
MAY_BE_UNSTABLE_EM = frozenset({"identical_50", "pure_noise_100", "pure_rotation"})
UNSTABLE_PNP = frozenset({"all_identical", "collinear"})  # the status flips between 0 and 1
UNSTABLE_EM = frozenset({"identical_50", "pure_rotation"})  # same mask, an unrelated E (drift > 1)


# ---------------------------------------------------------------------------- camera model
def rodrigues(r):
    return mc.rot(np.asarray(r, np.float64))


def project(P, rvec, tvec):
    """projectPoints with K, DIST (k1, k2 only) in float64."""
    Xc = np.asarray(P, np.float64) @ rodrigues(rvec).T + np.asarray(tvec, np.float64)
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = x * x + y * y
    cd = 1 + DIST[0] * r2 + DIST[1] * r2 * r2
    return np.c_[x * cd * K[0, 0] + K[0, 2], y * cd * K[1, 1] + K[1, 2]]


def _observe(rng, P, rv, tv, outlier_frac, noise):
    """The generator of test_gpu_parity._pnp_case after the points are drawn."""
    n = len(P)
    uv = project(P.astype(np.float64), rv, tv) + rng.normal(0, noise, (n, 2))
    out = rng.random(n) < outlier_frac
    uv[out] += rng.uniform(-40, 40, (int(out.sum()), 2))
    return uv.astype(np.float32)


def _cloud(rng, n):
    return np.c_[rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(2, 40, n)].astype(np.float32)


def _generic(seed, n, outlier_frac, noise, rv=None, tv=None):
    rng = np.random.default_rng(seed)
    P = _cloud(rng, n)
    rv0, tv0 = rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)
    rv = rv0 if rv is None else np.asarray(rv, np.float64)
    tv = tv0 if tv is None else np.asarray(tv, np.float64)
    return P, _observe(rng, P, rv, tv, outlier_frac, noise)


def _planar(seed, n, outlier_frac, noise, frontoparallel=False):
    """Points on Z = 10 + 0.3 x - 0.2 y rounded to float32.  frontoparallel: Z = 10 to within
    one float32 ulp (10 or one of its two neighbours, by a seeded draw).  With Z exactly constant
    the covariance of every 5-point subset has an exactly zero singular value, EPnP's fourth
    control point coincides with the centroid and no subset yields a model with 5 inliers: the
    oracle returns status 0 for every seed tried (13-18), so the refinement is never reached.  One
    ulp of jitter keeps the plane's normal within 1e-6 of the optical axis, far inside the
    Rt[2]^2 + Rt[5]^2 < 1e-10 test."""
    rng = np.random.default_rng(seed)
    P = _cloud(rng, n)
    if frontoparallel:
        ten, k = np.full(n, 10, np.float32), rng.integers(-1, 2, n)
        up, down = np.nextafter(ten, np.float32(20)), np.nextafter(ten, np.float32(0))
        P[:, 2] = np.where(k > 0, up, np.where(k < 0, down, ten))
    else:
        P[:, 2] = (10 + 0.3 * P[:, 0].astype(np.float64) - 0.2 * P[:, 1].astype(np.float64)).astype(np.float32)
    rv, tv = rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)
    return P, _observe(rng, P, rv, tv, outlier_frac, noise)


def _few_inliers(seed, n, k, noise=0.0):
    """k correspondences among n that are exact (or carry `noise` px), the rest far off (50-300 px
    away)."""
    rng = np.random.default_rng(seed)
    P = _cloud(rng, n)
    rv, tv = rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)
    uv = project(P.astype(np.float64), rv, tv)
    perm = rng.permutation(n)
    bad = perm[k:]
    ang = rng.uniform(0, 2 * np.pi, len(bad))
    uv[bad] += (rng.uniform(50, 300, len(bad)) * np.array([np.cos(ang), np.sin(ang)])).T
    if noise:
        uv[perm[:k]] += rng.normal(0, noise, (k, 2))
    return P, uv.astype(np.float32)


def _no_model(seed, n):
    rng = np.random.default_rng(seed)
    return _cloud(rng, n), rng.uniform([0, 0], [920, 616], (n, 2)).astype(np.float32)


def _all_identical(seed, n):
    rng = np.random.default_rng(seed)
    P = np.repeat(_cloud(rng, 1), n, axis=0)
    return P, np.repeat(project(P[:1].astype(np.float64), np.zeros(3), np.zeros(3)), n, axis=0).astype(np.float32)


def _duplicated_half(seed, n):
    rng = np.random.default_rng(seed)
    P = _cloud(rng, n)
    P[n // 2:] = P[:n // 2]
    rv, tv = rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)
    return P, _observe(rng, P, rv, tv, 0.1, 0.2)


def _collinear(seed, n):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 1, n)[:, None]
    P = (np.array([-4.0, -1.0, 5.0]) + s * np.array([8.0, 2.0, 25.0])).astype(np.float32)
    rv, tv = rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)
    return P, _observe(rng, P, rv, tv, 0.0, 0.1)


def _pnp(name, data, reach, cap=None, **params):
    P, uv = data
    P.setflags(write=False)
    uv.setflags(write=False)
    return dict(name=name, P=P, uv=uv, params={**PNP_DEFAULTS, **params}, reach=reach, cap=cap,
                stable=name not in UNSTABLE_PNP)


@functools.lru_cache(maxsize=None)
def pnp_cases():
    hard50 = lambda: _generic(305, 300, 0.5, 0.3)  # noqa: E731  (the iters_* set)
    hard40 = lambda: _generic(310, 300, 0.4, 0.3)  # noqa: E731  (the reproj_* / conf_* set)
    c = [
        _pnp("generic", _generic(0, 300, 0.3, 0.3), "dlt"),
        _pnp("planar_noisy", _planar(125, 200, 0.2, 0.2), "planar"),
        _pnp("planar_clean", _planar(56, 30, 0.0, 0.0), "planar"),
        _pnp("planar_frontoparallel", _planar(21, 100, 0.1, 0.2, frontoparallel=True), "planar_identity_rt"),
        _pnp("five_inliers", _few_inliers(22, 9, 5), "kept_ransac_model"),
        # exact inliers leave the RANSAC model within 6e-7 of the refined one; with 0.1 px on them a
        # kernel that refined the five inliers would move the pose by 5e-3 (measured on the oracle)
        _pnp("five_inliers_noisy", _few_inliers(519, 9, 5, noise=0.1), "kept_ransac_model"),
        _pnp("six_inliers", _few_inliers(25, 10, 6), "dlt_six"),
        _pnp("no_model", _no_model(23, 60), "status0"),
        _pnp("all_identical", _all_identical(31, 50), "degenerate"),
        _pnp("duplicated_half", _duplicated_half(32, 100), "degenerate"),
        _pnp("collinear", _collinear(33, 50), "degenerate"),
        _pnp("identity_motion", _generic(41, 300, 0.1, 0.2, rv=(0, 0, 0), tv=(0, 0, 0)), "theta_zero"),
        _pnp("large_rotation", _generic(42, 300, 0.1, 0.2, rv=(0, 3.0, 0), tv=(0, 0, 30)), "theta_near_pi"),
        _pnp("iters_1_clean", _generic(303, 300, 0.0, 0.1), "round1_only", iterations=1),
    ]
    for it in (1, 5, 100, 127, 128, 129, 200):
        reach = "round1_only" if it <= PNP_FIRST else ("round2_one_unit" if it == 129 else "round2_adaptive_end")
        c.append(_pnp(f"iters_{it}", hard50(), reach, iterations=it))
    for r in (0.5, 2.0, 8.0):
        c.append(_pnp(f"reproj_{r:g}", hard40(), "param", reproj=r))
    for p in (0.5, 0.9, 0.999, 0.999999):
        c.append(_pnp(f"conf_{p:g}", hard40(), "param", confidence=p))
    c.append(_pnp("param_defaults", hard40(), "param_base"))
    c.append(_pnp("hard_default", hard50(), "round2_adaptive_end"))  # the iters_* set at the default call
    c.append(_pnp("shim_default", hard40(), "param", reproj=8.0, iterations=100))  # cv2_compat.solvePnPRansac's
    c.append(_pnp("cap_smaller_than_context", _generic(51, 300, 0.3, 0.3), "dlt", cap=384))
    return tuple(c)


def pnp_case(name):
    return next(c for c in pnp_cases() if c["name"] == name)


_pnp_ref = {}


def pnp_reference(oracle_mod, case):
    """The oracle's (ok, rvec, tvec, inlier_idx, iters, best, info) of a case (computed once)."""
    if case["name"] not in _pnp_ref:
        p = case["params"]
        _pnp_ref[case["name"]] = oracle_mod.solve_pnp_ransac(case["P"].astype(np.float64), case["uv"], K, DIST,
                                                             reproj=p["reproj"], confidence=p["confidence"],
                                                             iters=p["iterations"], info=True)
    return _pnp_ref[case["name"]]


def ulp_moved(a, seed):
    """Every float32 entry of a moved by one ulp, up or down by a seeded coin."""
    rng = np.random.default_rng(seed)
    up = rng.random(a.shape) < 0.5
    return np.where(up, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))).astype(np.float32)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def transform(oracle_mod, rvec, tvec):
    T = np.eye(4)
    T[:3, :3] = oracle_mod.rodrigues(rvec)
    T[:3, 3] = tvec
    return T


STABLE_REL = 1e-6


def classify_pnp(oracle_mod, case):
    """(flips, drift) of the oracle's result under one-ulp moves of the 3-D points (three seeds):
    flips is True if the status or the inlier set changed; drift is the largest relative move of
    the pose, measured on the transform T = [R | t] as max |dT| / max |T|.  (rvec and tvec
    themselves have no usable relative scale: for identity_motion both are noise around zero, so
    any move is large relative to them.)  A case is stable if it does not flip and drift <
    STABLE_REL."""
    ok, rv, tv, inl, _, _, _ = pnp_reference(oracle_mod, case)
    p = case["params"]
    drift = 0.0
    for seed in (1, 2, 3):
        ok2, rv2, tv2, inl2, _, _ = oracle_mod.solve_pnp_ransac(ulp_moved(case["P"], seed).astype(np.float64),
                                                                case["uv"], K, DIST, reproj=p["reproj"],
                                                                confidence=p["confidence"], iters=p["iterations"])
        if ok2 != ok or not np.array_equal(inl, inl2):
            return True, float("inf")
        if ok:
            drift = max(drift, _rel(transform(oracle_mod, rv2, tv2), transform(oracle_mod, rv, tv)))
    return False, drift


# ---------------------------------------------------------------------------- essential matrix
def _two_view_scene(seed, n, X, noise, outliers, forward=True):
    """mono_cases.two_view with the scene points given."""
    rng = np.random.default_rng(seed)
    R = mc.rot(rng.normal(size=3) * 0.05)
    t = rng.normal(size=3)
    if forward:
        t[2] = abs(t[2]) + 0.5
    t /= np.linalg.norm(t)
    X2 = X @ R.T + t
    p0 = np.c_[mc.F * X[:, 0] / X[:, 2] + mc.CX, mc.F * X[:, 1] / X[:, 2] + mc.CY]
    p1 = np.c_[mc.F * X2[:, 0] / X2[:, 2] + mc.CX, mc.F * X2[:, 1] / X2[:, 2] + mc.CY]
    p1 = p1 + rng.normal(size=p1.shape) * noise
    k = int(round(outliers * n))
    if k:
        p1[rng.choice(n, k, replace=False)] = rng.uniform([0, 0], [920, 616], (k, 2))
    return p0.astype(np.float32), p1.astype(np.float32)


def _em(name, data, reach, cap=512, **params):
    p0, p1 = (np.ascontiguousarray(a, np.float32) for a in data)
    p0.setflags(write=False)
    p1.setflags(write=False)
    return dict(name=name, p0=p0, p1=p1, params={**EM_DEFAULTS, **params}, reach=reach, cap=cap,
                stable=name not in UNSTABLE_EM)


FIVE_POINT_SEEDS = tuple(range(60, 70))
DISTANCE_THRESH = 50.0  # recoverPose's distanceThresh


def _planar_scene(seed):
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-5, 5, 300), rng.uniform(-3, 3, 300), np.zeros(300)]
    X[:, 2] = 10 + 0.2 * X[:, 0]
    return _two_view_scene(seed, 300, X, 0.3, 0.2)


def _deep_scene(seed):
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-5, 5, 300), rng.uniform(-3, 3, 300), rng.uniform(4, 30, 300)]
    X[:40, 2] = rng.uniform(80, 400, 40)  # deeper than distanceThresh = 50 baselines (|t| = 1)
    X[:40, :2] *= X[:40, 2:3] / 20  # kept inside the field of view
    return _two_view_scene(seed, 300, X, 0.1, 0.1)


def _duplicated(seed):
    d0, d1 = (a.copy() for a in mc.two_view(seed, 200, 0.3, 0.2)[:2])
    d0[100:], d1[100:] = d0[:100], d1[:100]
    return d0, d1


@functools.lru_cache(maxsize=None)
def em_cases():
    """The seeds are the first of a bounded search (a few hundred per case) at
    which the oracle alone is stable: the 5-point solver amplifies a one-ulp move of p1 by
    1e2 - 1e4, so most seeds fail the 1e-6 bound without ever flipping the inlier set.  The
    max_iters cases share one set; every prob / threshold case has a set of its own, and the CPU
    test runs the default call on that set to show that the parameter moves the result."""
    hard = lambda: mc.two_view(248, 300, 0.3, 0.5)[:2]  # noqa: E731  (default bound 210: round 2)
    c = [_em("param_defaults", hard(), "round2")]
    for it in (1, 10, 64, 127, 128, 129, 300):
        reach = "round1_only" if it <= PNP_FIRST else "round2"
        c.append(_em(f"max_iters_{it}", hard(), reach, max_iters=it))
    c.append(_em("threshold_0.25", mc.two_view(553, 300, 0.3, 0.4)[:2], "param", threshold=0.25))
    c.append(_em("threshold_3", mc.two_view(422, 300, 0.3, 0.4)[:2], "param", threshold=3.0))
    c.append(_em("prob_0.5", mc.two_view(178, 300, 0.3, 0.4)[:2], "param", prob=0.5))
    c.append(_em("prob_0.9", mc.two_view(379, 300, 0.3, 0.4)[:2], "param", prob=0.9))
    c.append(_em("prob_0.99999", mc.two_view(286, 300, 0.3, 0.4)[:2], "param", prob=0.99999))
    c.append(_em("backward_or_sideways", mc.two_view(209, 300, 0.3, 0.2, forward=False)[:2], "motion"))
    c.append(_em("planar_scene", _planar_scene(119), "planar"))
    p0 = mc.two_view(74, 200, 0.0, 0.0)[0]
    c.append(_em("pure_rotation", (p0, p0.copy()), "zero_cheirality"))
    q0, q1 = mc.two_view(75, 1, 0.0, 0.0)[:2]
    c.append(_em("identical_50", (np.repeat(q0, 50, axis=0), np.repeat(q1, 50, axis=0)), "degenerate"))
    c.append(_em("duplicated_half", _duplicated(421), "duplicates"))
    rng = np.random.default_rng(77)
    c.append(_em("pure_noise_100", (rng.uniform([0, 0], [920, 616], (100, 2)),
                                    rng.uniform([0, 0], [920, 616], (100, 2))), "noise"))
    c.append(_em("deep_points", _deep_scene(513), "distance_mask"))
    for s in FIVE_POINT_SEEDS:
        c.append(_em(f"five_points_{s}", mc.two_view(s, 5, 0.0, 0.0)[:2], "five_points"))
    c.append(_em("cap_2049", mc.two_view(158, 2049, 0.3, 0.3)[:2], "lds_over_64k", cap=2049))
    c.append(_em("cap_5040", mc.two_view(282, 5040, 0.3, 0.3)[:2], "lds_limit", cap=5040))
    return tuple(c)


def em_case(name):
    return next(c for c in em_cases() if c["name"] == name)


_em_ref = {}


def em_oracle(oracle_mod, p0, p1, params):
    """dict(status, E, mask, iters, best, trimmed, nomodel, good, R, t); good / R / t are None
    unless status is 1."""
    st, E, mask, ni, bg, (trim, nomod) = oracle_mod.find_essential(p0, p1, mc.F, (mc.CX, mc.CY), prob=params["prob"],
                                                                   threshold=params["threshold"],
                                                                   max_iters=params["max_iters"], stats=True)
    r = dict(status=st, E=E, mask=mask, iters=ni, best=bg, trimmed=trim, nomodel=nomod, good=None, R=None, t=None)
    if st == 1:
        r["good"], r["R"], r["t"] = oracle_mod.recover_pose(E, p0, p1, mc.F, (mc.CX, mc.CY), dist=DISTANCE_THRESH)
    return r


def em_reference(oracle_mod, case):
    """em_oracle of a case (computed once)."""
    if case["name"] not in _em_ref:
        _em_ref[case["name"]] = em_oracle(oracle_mod, case["p0"], case["p1"], case["params"])
    return _em_ref[case["name"]]


def classify_em(oracle_mod, case):
    """(flips, drift) as classify_pnp, with p1 moved: flips if the status, the inlier mask or the
    cheirality count changed; drift is the largest relative move of E, R or t."""
    ref = em_reference(oracle_mod, case)
    drift = 0.0
    for seed in (1, 2, 3):
        r = em_oracle(oracle_mod, case["p0"], ulp_moved(case["p1"], seed), case["params"])
        if r["status"] != ref["status"]:
            return True, float("inf")
        if r["status"] != 1:
            continue
        if not np.array_equal(r["mask"], ref["mask"]) or r["good"] != ref["good"]:
            return True, float("inf")
        drift = max(drift, *(_rel(r[k], ref[k]) for k in ("E", "R", "t")))
    return False, drift


# ---------------------------------------------------------------------------- back-projection
BP_W, BP_H, BP_CAP = 40, 24, 600
BP_BLOCK = 256  # k_backproject's block size: one pass of the ordered compaction
SPECIAL_DISP = (0, -16, -1, -17, 1, 2, 3, 16, 32767, -32768, 26100, 26101)


@functools.lru_cache(maxsize=None)
def backproject_case():
    """dict(disp i16[B,H,W], kp0 / kp1 f32[B,cap,8], matches i32[B,cap,3], n_matches i32[B],
    n_kp i32[B]) with B = 5 frames: (0) every match kept, n = cap; (1) none kept; (2) mixed,
    n = 300 > BP_BLOCK; (3) n = 0; (4) mixed, n = cap.  Z = fx B / (d / 16): disparity 2 gives
    Z > 1000, 3 gives Z < 1000, 26100 gives Z > float32(0.1) and 26101 Z < it."""
    rng = np.random.default_rng(2024)
    B, W, H, cap = 5, BP_W, BP_H, BP_CAP
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (3 + 7 * xx + 41 * yy).astype(np.int16)  # 3 .. 1219: every pixel kept
    disp = np.stack([ramp] * B)
    bad = np.array([0, -16, -1, -17, 1, 2, 32767, -32768, 26101], np.int16)
    disp[1] = bad[rng.integers(0, len(bad), (H, W))]
    for b in (2, 4):
        sp = rng.random((H, W)) < 0.5
        disp[b][sp] = np.array(SPECIAL_DISP, np.int16)[rng.integers(0, len(SPECIAL_DISP), int(sp.sum()))]
        disp[b].flat[:len(SPECIAL_DISP)] = SPECIAL_DISP  # every value at least once, incl. pixel (0, 0)
        disp[b][H - 1, W - 1] = 16
    kp0 = np.zeros((B, cap, 8), np.float32)
    kp1 = np.zeros((B, cap, 8), np.float32)
    kp0[:, :, 0] = rng.uniform(0, W, (B, cap))
    kp0[:, :, 1] = rng.uniform(0, H, (B, cap))
    kp0[:, :, 2:] = rng.uniform(0, 100, (B, cap, 6))
    kp1[:, :, :2] = rng.uniform(0, 900, (B, cap, 2))
    kp1[:, :, 2:] = rng.uniform(0, 100, (B, cap, 6))
    edge = np.array([[W - 1 + 0.99, H - 1 + 0.99], [0, 0], [W - 1 + 0.99, 0.5], [0.25, H - 1 + 0.99],
                     [W - 1, H - 1], [0.999, 0.999]], np.float32)
    kp0[:, :len(edge), :2] = edge
    kp0 = np.minimum(kp0, np.float32([W - 0.01, H - 0.01] + [1e9] * 6))  # (int)x stays inside the image
    matches = np.zeros((B, cap, 3), np.int32)
    for b in range(B):
        matches[b, :, 0] = rng.permutation(cap)
        matches[b, :, 1] = rng.permutation(cap)
        matches[b, :len(edge), 0] = np.arange(len(edge))[::-1]  # the edge keypoints are matched
        rest = np.setdiff1d(np.arange(cap), matches[b, :len(edge), 0])
        matches[b, len(edge):, 0] = rng.permutation(rest)
        matches[b, :, 2] = rng.integers(0, 256, cap)
    n_matches = np.array([cap, cap, 300, 0, cap], np.int32)
    n_kp = np.array([cap, 300, cap, 0, 257], np.int32)
    out = dict(disp=disp, kp0=kp0, kp1=kp1, matches=matches, n_matches=n_matches, n_kp=n_kp)
    for v in out.values():
        v.setflags(write=False)
    return out


def backproject_reference(oracle_mod, bp):
    """Per frame (P3 f32[k,3], p2 f32[k,2], valid bool[n]) of oracle.backproject on the matches."""
    out = []
    for b in range(len(bp["disp"])):
        n = int(bp["n_matches"][b])
        m = bp["matches"][b, :n]
        mk0 = bp["kp0"][b, m[:, 0], :2]
        mk1 = bp["kp1"][b, m[:, 1], :2]
        out.append(oracle_mod.backproject(oracle_mod.disparity_map(bp["disp"][b]), mk0, mk1, K, BASELINE))
    return out


def keypoint_stereo_reference(oracle_mod, bp):
    """f32 [B,cap,4] (X, Y, Z, d) of every keypoint of kp0 below n_kp with 0.1 < Z < 1000, zeros
    elsewhere: oracle.backproject's arithmetic per keypoint."""
    B, cap = bp["kp0"].shape[:2]
    out = np.zeros((B, cap, 4), np.float32)
    for b in range(B):
        n = int(bp["n_kp"][b])
        xy = bp["kp0"][b, :n, :2]
        d = oracle_mod.disparity_map(bp["disp"][b])
        P, _, valid = oracle_mod.backproject(d, xy, xy, K, BASELINE)
        idx = np.nonzero(valid)[0]
        out[b, idx, :3] = P
        out[b, idx, 3] = d[xy[idx, 1].astype(int), xy[idx, 0].astype(int)]
    return out
