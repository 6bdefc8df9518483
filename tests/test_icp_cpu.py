"""ICP registration on the CPU: the specification tests/icp_ref.py on its own (the known motion, Horn
against an SVD Kabsch, the 4x4 Jacobi's termination, the Gibbs rotation, the LDL^T, the tie and radius
rules, the empty correspondence set, the order sensitivity from which the GPU tolerance is derived),
the Open3D-shaped module's refusals, and the host layer csrc/capi_icp.cpp under the sanitizers.  The
GPU kernels are compared with the same specification in tests/test_icp_gpu.py."""
import ctypes
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_ref as ref
from conftest import ROOT

EPS = 2.0 ** -53


# ------------------------------------------------------------------ the loop on the named inputs
@pytest.mark.parametrize("estimation", [ref.PLANE, ref.POINT])
def test_subset_recovers_the_known_motion(estimation):
    """Measured here: max |T - motion| = 3.1e-16 (plane, 4 updates) and 1.9e-15 (point, 8 updates);
    asserted: 1000 x the recorded figure."""
    out = ref.solved("subset", estimation)
    err = np.abs(out["T"] - ref.case("subset")[4]).max()
    print(f"subset est {estimation}: {out['iterations']} updates, max |T - motion| {err:.3e}, rmse {out['inlier_rmse']:.3e}")
    assert out["fitness"] == 1.0 and out["status"] == 0 and out["iterations"] < 30
    assert err <= 1000.0 * ref.KNOWN_MOTION_ERR[estimation]
    assert out["T"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert np.array_equal(out["correspondences"], np.arange(0, 1444, 2))


def test_partial_overlap():
    """partial / plane converges with fitness ~ 0.73; partial / point slides along the surface and
    is still moving after 10 updates (the exit the GPU test runs)."""
    plane = ref.solved("partial", ref.PLANE)
    point = ref.solved("partial", ref.POINT, 10)
    M = ref.case("partial")[4]
    print(f"partial: plane {plane['iterations']} updates, fitness {plane['fitness']:.4f}, |T - motion| "
          f"{np.abs(plane['T'] - M).max():.2e}; point {point['iterations']} updates, fitness {point['fitness']:.4f}")
    assert 0.70 < plane["fitness"] < 0.76 and plane["iterations"] < 10 and np.abs(plane["T"] - M).max() < 5e-3
    assert point["iterations"] == 10 and point["status"] == 0


def test_far_from_the_origin():
    """Both clouds + 1000 m: the pivot keeps the solve as exact as at the origin (same update count);
    T's last column carries |c| ~ 1000, so its entries are good to ~1e-11."""
    for est in (ref.PLANE, ref.POINT):
        near, far = ref.solved("subset", est), ref.solved("far", est)
        err = np.abs(far["T"] - ref.case("far")[4]).max()
        print(f"far est {est}: {far['iterations']} updates, max |T - motion| {err:.3e}")
        assert far["iterations"] == near["iterations"] and far["fitness"] == 1.0 and err < 1e-9
        assert np.abs(far["T"][:3, :3] - near["T"][:3, :3]).max() < 1e-13


# ------------------------------------------------------------------ the solvers
def _kabsch(P, Q):
    """R, t minimising sum |R p + t - q|^2 by SVD."""
    pm, qm = P.mean(axis=0), Q.mean(axis=0)
    H = (P - pm).T @ (Q - qm)
    Uu, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ Uu.T))])
    R = Vt.T @ D @ Uu.T
    return R, qm - R @ pm


def _horn_problems():
    rng = np.random.default_rng(21)
    for k in range(300):
        n = int(rng.integers(3, 60))
        P = rng.uniform(0.0, 10.0 ** rng.integers(-1, 3), (n, 3))
        w = rng.normal(size=3)
        w *= rng.choice([1e-6, 1e-3, 0.1, 1.0, 3.0]) / np.linalg.norm(w)
        Q = P @ ref.rodrigues(w).T + rng.normal(size=3) + rng.normal(0.0, rng.choice([0.0, 1e-6, 1e-2]), (n, 3))
        yield P, Q


def test_horn_equals_kabsch_and_the_jacobi_terminates():
    """300 seeded problems (3 .. 59 points, angles 1e-6 .. 3 rad, noise 0 .. 1e-2): Horn's R against an
    SVD Kabsch; measured worst |R_horn - R_svd| = 5.9e-14 (a three-point problem), asserted 1000 x.  Every
    4x4 Jacobi ends with six exact zeros; the most sweeps seen here: 7 (SWEEP_CAP4 = 12)."""
    worst, most = 0.0, 0
    for P, Q in _horn_problems():
        sums = np.zeros(ref.SUMS)
        sums[0:3], sums[3:6] = P.sum(axis=0), Q.sum(axis=0)
        sums[6:15] = (P[:, :, None] * Q[:, None, :]).sum(axis=0).reshape(-1)
        R, v, sweeps = ref.horn(sums, len(P))
        Rk, tk = _kabsch(P, Q)
        worst = max(worst, np.abs(np.array(R) - Rk).max())
        most = max(most, sweeps)
        assert np.abs(np.array(R).T @ np.array(R) - np.eye(3)).max() <= 16 * EPS
        assert np.abs(np.array(v) - tk).max() <= 1e-12 * max(1.0, np.abs(P).max())
    print(f"Horn vs Kabsch: worst |dR| {worst:.3e}, most sweeps {most}")
    assert worst <= 1000 * 5.9e-14 and most < ref.SWEEP_CAP4  # below the cap: ended by the six exact zeros


def test_jacobi4_ends_with_exact_zeros_on_every_input_of_the_tests():
    """The N(M) of every pass of the point-to-point runs the tests make (at most 6 sweeps) and 200
    random symmetric 4x4s end with six exact zeros below the cap.  A triple eigenvalue (an isotropic
    cloud: N = Q diag(1, 1, 1, -3) Q^T) can keep rotating inside its eigenspace: there the cap may end
    the solve, with off-diagonals of a few ulps at most and the same accurate decomposition, and host
    and device still agree bit for bit because both stop at the same sweep."""
    most = 0
    for name, mi in (("subset", 30), ("partial", 10), ("far", 30)):
        assert ref.solved(name, ref.POINT, mi)["sweeps"] < ref.SWEEP_CAP4
        most = max(most, ref.solved(name, ref.POINT, mi)["sweeps"])
    rng = np.random.default_rng(4)
    mats = [(np.zeros((4, 4)), True), (np.eye(4), True), (np.ones((4, 4)), True), (np.diag([1.0, 1.0, 2.0, 2.0]), True)]
    for _ in range(200):
        A = rng.normal(size=(4, 4))
        mats.append((A + A.T, True))
        Qm = np.linalg.qr(rng.normal(size=(4, 4)))[0]
        mats.append((Qm @ np.diag([1.0, 1.0, 1.0, -3.0]) @ Qm.T, False))
    capped = 0
    for A, simple in mats:
        A = (A + A.T) / 2
        d, V, sweeps, off = ref.jacobi4(A)
        if simple:
            assert off == [0.0] * 6 and sweeps < ref.SWEEP_CAP4, (A, off, sweeps)
            most = max(most, sweeps)
        else:
            capped += sweeps == ref.SWEEP_CAP4
            assert max(abs(v) for v in off) <= 4 * EPS * np.abs(A).max(), (A, off, sweeps)
        V = np.array(V)
        assert np.abs(V @ np.diag(d) @ V.T - A).max() <= 64 * EPS * max(1.0, np.abs(A).max())
        assert np.allclose(np.sort(d), np.linalg.eigvalsh(A), atol=64 * EPS * max(1.0, np.abs(A).max()))
    print(f"jacobi4: most sweeps {most}; {capped} of 200 triple-eigenvalue matrices ran into the cap")


def test_gibbs_rotation_is_orthogonal_and_close_to_rodrigues():
    rng = np.random.default_rng(8)
    for scale in (0.0, 1e-12, 1e-6, 1e-3, 0.05, 0.5, 2.0):
        for _ in range(20):
            w = rng.normal(size=3) * scale
            R = np.array(ref.gibbs(w))
            assert np.abs(R.T @ R - np.eye(3)).max() <= 8 * EPS, (w, R)
            assert np.linalg.det(R) > 0
            th = np.linalg.norm(w)  # the Gibbs vector w / 2 turns by 2 atan(|w| / 2): |w|^3 / 12 off
            assert np.abs(R - ref.rodrigues(w)).max() <= th ** 3 / 12 + 8 * EPS
    assert np.array_equal(np.array(ref.gibbs([0.0, 0.0, 0.0])), np.eye(3))


def test_ldlt_agrees_with_numpy_relative_to_the_condition():
    rng = np.random.default_rng(12)
    worst = 0.0
    for k in range(100):
        J = rng.normal(size=(40, 6)) * 10.0 ** rng.uniform(-2, 2, 6)
        A = J.T @ J
        b = rng.normal(size=6)
        x, ok = ref.ldlt6(np.triu(A), b)  # only the upper triangle is read
        assert ok
        want = np.linalg.solve(A, b)
        rel = np.abs(np.array(x) - want).max() / np.abs(want).max()
        worst = max(worst, rel / (np.linalg.cond(A) * EPS))
        assert rel <= 64 * np.linalg.cond(A) * EPS
    print(f"ldlt6: worst relative error / (cond * 2^-53) = {worst:.3f}")
    for bad in (np.zeros((6, 6)), -np.eye(6), np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), np.full((6, 6), np.nan),
                np.diag([1.0, math.inf, 1.0, 1.0, 1.0, 1.0])):
        assert ref.ldlt6(bad, np.ones(6)) == ([0.0] * 6, False)


# ------------------------------------------------------------------ the search's rules
def test_ties_take_the_lower_index_and_the_radius_is_strict():
    Tg = ref.lattice(6, 6, 5)
    S = Tg + np.array([0.5, 0.0, 0.0])
    idx, d2 = ref.correspondences(S, Tg, 0.6)
    assert (d2 == 0.25).all() and np.array_equal(idx, np.arange(len(Tg)))  # x and x + 1 tie; x has the lower index
    assert (ref.correspondences(S, Tg, 0.5)[0] == -1).all()  # r exactly the distance: excluded
    assert (ref.correspondences(S, Tg, math.nextafter(0.5, 1.0))[0] >= 0).all()
    D = ref.duplicates()
    dup = np.flatnonzero((D == np.array([2.5, 3.25, 1.125])).all(axis=1))
    assert len(dup) == 30 and (ref.correspondences(D[dup], D, 0.1)[0] == dup[0]).all()


def test_empty_correspondence_set():
    """m = 0: the update is the identity with the degenerate bit; with the default criteria the loop
    applies it once and stops (no change), with criteria 0 it runs to max_iteration."""
    S, Tg, Nt, r, _ = ref.case("subset")
    far = S + np.array([0.0, 0.0, 40.0])
    init = ref.motion(np.zeros(3))
    for est in (ref.POINT, ref.PLANE):
        out = ref.registration(far, Tg, Nt, r, init, est)
        assert out["m"] == 0 and out["fitness"] == 0.0 and out["inlier_rmse"] == 0.0
        assert out["iterations"] == 1 and out["status"] == ref.DEGENERATE and np.array_equal(out["T"], init)
        assert ref.registration(far, Tg, Nt, r, init, est, 0.0, 0.0, 5)["iterations"] == 5
        ev = ref.registration(far, Tg, Nt, r, init, est, max_iteration=0)
        assert ev["iterations"] == 0 and ev["status"] == 0
    e = np.zeros((0, 3))
    assert ref.registration(e, Tg, Nt, r, init)["fitness"] == 0.0 and ref.registration(S, e, e, r, init)["m"] == 0


# ------------------------------------------------------------------ order sensitivity
CASES = sorted(ref.ORDER_SPREAD)


@pytest.mark.parametrize("name,estimation,max_iteration", CASES, ids=[f"{n}-{e}-{m}" for n, e, m in CASES])
def test_order_sensitivity(name, estimation, max_iteration):
    """The full loop with the sums taken by fsum, forward, reversed and pairwise: the same iteration
    count and correspondences, and the largest entry-wise spread of the final T recorded in
    icp_ref.ORDER_SPREAD (measured: 7.8e-16 subset / plane, 1.4e-14 subset / point, 7.8e-16 partial /
    plane, 3.5e-14 partial / point at 10, 1.5e-11 far / plane, 4.0e-12 far / point; the recorded figure
    is twice that).  tests/test_icp_gpu.py allows the device 1000 x the recorded figure."""
    outs = [ref.solved(name, estimation, max_iteration, how) for how in ("fsum", "forward", "reversed", "pairwise")]
    spread = max(np.abs(a["T"] - b["T"]).max() for a, b in itertools.combinations(outs, 2))
    print(f"{name} est {estimation}: spread of T {spread:.3e} (recorded {ref.ORDER_SPREAD[(name, estimation, max_iteration)]:.1e})")
    for o in outs[1:]:
        assert o["iterations"] == outs[0]["iterations"]
        assert np.array_equal(o["correspondences"], outs[0]["correspondences"])
    assert spread <= ref.ORDER_SPREAD[(name, estimation, max_iteration)]
    assert 1000.0 * ref.ORDER_SPREAD[(name, estimation, max_iteration)] < 1e-7  # far below one changed correspondence


# ------------------------------------------------------------------ the Open3D-shaped module
def test_registration_module_refuses_what_it_does_not_offer():
    from forest_slam_amd import registration as reg
    c = reg.ICPConvergenceCriteria()
    assert (c.relative_fitness, c.relative_rmse, c.max_iteration) == (1e-6, 1e-6, 30)
    assert reg.TransformationEstimationPointToPoint().estimation == 0
    assert reg.TransformationEstimationPointToPlane().estimation == 1
    with pytest.raises(NotImplementedError):
        reg.TransformationEstimationPointToPoint(with_scaling=True)
    with pytest.raises(NotImplementedError):
        reg.TransformationEstimationPointToPlane(kernel=object())
    for name in ("TransformationEstimationForColoredICP", "TransformationEstimationForGeneralizedICP",
                 "registration_colored_icp", "registration_generalized_icp", "HuberLoss", "TukeyLoss"):
        with pytest.raises(NotImplementedError):
            getattr(reg, name)()
    with pytest.raises(NotImplementedError):
        reg.registration_icp(None, None, 0.3, estimation_method=object())
    from forest_slam_amd import _lib
    from forest_slam_amd.mapping import PointMap
    assert callable(PointMap.transform) and callable(PointMap.registration_icp)
    for fn in ("fvo_icp_workspace_bytes", "fvo_registration_icp", "fvo_transform_points"):
        assert fn in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["fvo_registration_icp"][1]) == 20


# ------------------------------------------------------------------ the argument checks, sanitized
def test_icp_boundary_checks_under_sanitizers(tmp_path):
    """csrc/capi_icp.cpp's refusals by their exact messages, the accepted bound next to each, the valid
    calls reaching exactly their launcher and no search launched for an empty source or target:
    tests/sanitize/icp_check.cpp (its own main and its own stubs of the launchers), built as
    tests/test_normals_cpu.py builds normals_check.cpp, with capi_icp.cpp in place of capi_normals.cpp."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    shared = hasattr(ctypes.CDLL(None), "__asan_init")  # see sanitize_build.run_check
    rt = subprocess.run([gxx, "-print-file-name=" + ("libasan.so" if shared else "libasan.a")], capture_output=True,
                        text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("the ASan runtime of g++ is not installed")
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("HIP headers not found")
    exe = str(tmp_path / "icp_check")
    san, csrc = os.path.join(ROOT, "tests", "sanitize"), os.path.join(ROOT, "forest-slam_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-g", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", hip_inc,
           "-I", os.path.join(ROOT, "include"), os.path.join(csrc, "capi.cpp"), os.path.join(csrc, "capi_icp.cpp"),
           os.path.join(san, "host_stubs.cpp"), os.path.join(san, "icp_check.cpp"), "-o", exe]
    b = subprocess.run(cmd + ([] if shared else ["-static-libasan", "-static-libubsan"]), capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "0 failed" in r.stdout
