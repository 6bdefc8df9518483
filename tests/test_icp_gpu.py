"""fvo_registration_icp / fvo_transform_points, forest_slam_amd.registration and PointMap's transform on
the GPU against the specification tests/icp_ref.py: the correspondences and the fitness bit for bit
whatever the grid's cell, the sums within their derived bound and deterministic, the update bit for
bit from the device's own sums, the whole loop (iterations, final correspondences, T within 1000 x the
CPU order-sensitivity figure), graph capture, and the map's faces.  The specification's answers are
computed once per case and shared read-only; the largest cloud has 1444 points."""
import functools

import numpy as np
import pytest
import torch

import icp_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

U = 2.0 ** -53
I4 = np.eye(4)


@functools.lru_cache(maxsize=None)
def _ctx():
    from forest_slam_amd import _lib
    return _lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_BF, kp_capacity=64)


def _dev(a):
    return torch.from_numpy(np.array(a, np.float64, order="C")).cuda()  # a copy: the shared inputs are read-only


def _outside(kind):
    """Sources outside the target's bounding box, on the low and the high side of each axis, nearer
    and farther than r = 0.3: target points pushed past a face by 0.1 .. 1e7 m (partly: plus 60
    points inside)."""
    Tg = ref.bumpy(1)
    lo, hi = Tg.min(axis=0), Tg.max(axis=0)
    rows = []
    for a in range(3):
        for side in (0, 1):
            order = np.argsort(Tg[:, a])
            near = Tg[order[:12] if side == 0 else order[-12:]].copy()
            for k, d in enumerate((0.1, 0.2, 0.29, 0.31, 0.35, 1.0, 3.0, 50.0, 1e7, 0.05, 0.299, 0.301)):
                near[k, a] = lo[a] - d if side == 0 else hi[a] + d
            rows.append(near)
    S = np.concatenate(rows)
    if kind == "partly":
        S = np.concatenate([S, Tg[100:160] + np.array([0.03, -0.02, 0.01])])
    return np.ascontiguousarray(S)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """-> (source, target, target normals or None, r, init) of a named search case, read-only."""
    if name in ("subset", "partial", "far"):
        S, Tg, Nt, r, _ = ref.case(name)
        out = (S, Tg, Nt, r, I4)
    elif name in ("subset@motion", "partial@motion"):
        S, Tg, Nt, r, M = ref.case(name.split("@")[0])
        out = (S, Tg, Nt, r, M)
    elif name == "lattice":  # every source point is 0.5 from two target points: the lower index wins
        Tg = ref.lattice(6, 6, 5)
        out = (np.ascontiguousarray(Tg + np.array([0.5, 0.0, 0.0])), Tg, None, 0.6, I4)
    elif name == "dup":  # 30 copies of one target point: the lowest index of them
        Tg = ref.duplicates()
        out = (np.ascontiguousarray(np.concatenate([Tg[::2], Tg[1::5] + np.array([0.01, 0.0, -0.02])])), Tg, None, 0.5,
               I4)
    elif name in ("outside:partly", "outside:wholly"):
        out = (_outside(name.split(":")[1]), ref.bumpy(1), ref.bumpy_normals(1), 0.3, I4)
    elif name == "one-target":
        S = ref.case("subset")[0]
        out = (S, np.ascontiguousarray(S[40:41] + 0.01), None, 0.3, I4)
    elif name == "one-source":
        S, Tg, Nt, r, _ = ref.case("subset")
        out = (np.ascontiguousarray(S[7:8]), Tg, Nt, r, I4)
    else:
        raise KeyError(name)
    for a in out[:3]:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _spec_eval(name, estimation):
    S, Tg, Nt, r, init = _inputs(name)
    return ref.evaluate(S, Tg, Nt, r, init, estimation)


def _run(name, estimation=0, max_iteration=0, cell=None, rel=(1e-6, 1e-6), init=None, **kw):
    S, Tg, Nt, r, init0 = _inputs(name)
    res, sums, corr, st = _ctx().registration_icp(
        _dev(S), _dev(Tg), r, init0 if init is None else init, estimation, _dev(Nt) if estimation == 1 else None,
        rel[0], rel[1], max_iteration, cell, sums=True, **kw)
    return res.cpu().numpy(), sums.cpu().numpy(), corr.cpu().numpy(), int(st.item())


SEARCH = ["subset", "partial", "subset@motion", "partial@motion", "lattice", "dup", "outside:partly", "outside:wholly",
          "one-target", "one-source", "far"]


# ------------------------------------------------------------------ correspondences
@pytest.mark.parametrize("name", SEARCH)
def test_correspondences_bit_for_bit(name):
    """max_iteration = 0 (evaluate_registration): the indices and the fitness equal the brute-force
    specification's; T is init, no update was applied."""
    want = _spec_eval(name, 0)
    res, sums, corr, st = _run(name)
    print(f"{name}: {want['m']} of {len(corr)} correspondences, fitness {want['fitness']}")
    assert st == 0
    assert np.array_equal(corr, want["correspondences"])
    assert res[16] == want["fitness"] and res[18] == want["m"] and res[19] == 0
    assert np.array_equal(res[:16].reshape(4, 4), _inputs(name)[4])
    if name == "lattice":
        assert want["m"] == len(corr) and (np.diff(corr) > 0).all()
    if name == "outside:wholly":
        assert 0 < want["m"] < len(corr)


@pytest.mark.parametrize("factor", [0.25, 1.0, 4.0])
@pytest.mark.parametrize("name", ["subset", "outside:partly", "lattice", "dup"])
def test_result_does_not_depend_on_the_cell(name, factor):
    """cell = r / 4 (R = 5 rings), r and 4 r: the same correspondences."""
    want = _spec_eval(name, 0)
    res, _, corr, st = _run(name, cell=factor * _inputs(name)[3])
    assert st == 0 and np.array_equal(corr, want["correspondences"]) and res[16] == want["fitness"]


def test_status_of_a_bad_target_or_source():
    """A target coordinate 2^21 cells away, a NaN in the target, a NaN in the source: status bit 1."""
    ctx = _ctx()
    S, Tg, _, r, _ = ref.case("subset")
    bad = Tg.copy()
    bad[17, 2] = np.delete(Tg[:, 2], 17).min() + r * 2.0 ** 21
    assert int(ctx.registration_icp(_dev(S), _dev(bad), r, max_iteration=0)[3].item()) & 1
    bad = Tg.copy()
    bad[3, 1] = np.nan
    assert int(ctx.registration_icp(_dev(S), _dev(bad), r, max_iteration=0)[3].item()) & 1
    src = S.copy()
    src[5, 0] = np.nan
    res, _, corr, st = ctx.registration_icp(_dev(src), _dev(Tg), r, max_iteration=0)
    want = ref.evaluate(src, Tg, None, r, I4)
    assert int(st.item()) == 1 and np.array_equal(corr.cpu().numpy(), want["correspondences"]) and corr[5].item() == -1


# ------------------------------------------------------------------ sums
@pytest.mark.parametrize("estimation", [0, 1])
@pytest.mark.parametrize("name", ["subset", "partial", "far", "subset@motion", "outside:partly"])
def test_sums_within_their_bound_and_deterministic(name, estimation):
    """Every device sum is within 2 m 2^-53 sum|term| of the specification's fsum: any order of m terms
    errs by at most (m - 1) u sum|term|, and the terms' own roundings are the specification's.  Two
    calls give the same bits."""
    want = _spec_eval(name, estimation)
    res, sums, corr, st = _run(name, estimation)
    m = want["m"]
    assert np.array_equal(corr, want["correspondences"]) and sums[28] == m
    err = np.abs(sums[:28] - want["sums"])
    bound = 2.0 * m * U * want["sums_abs"]
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{name} est {estimation}: m {m}, worst error / bound {np.nanmax(np.where(bound > 0, err / bound, 0)):.3f}")
    assert (err <= bound).all(), (err, bound)
    assert np.array_equal(sums[29:].reshape(4, 4), _inputs(name)[4])
    assert abs(res[17] - want["inlier_rmse"]) <= 2.0 * m * U * max(want["inlier_rmse"], 1e-300)
    again = _run(name, estimation)
    assert np.array_equal(again[1], sums) and np.array_equal(again[0], res)


# ------------------------------------------------------------------ the update
@pytest.mark.parametrize("estimation", [0, 1])
@pytest.mark.parametrize("name", ["subset", "partial", "far"])
def test_update_bit_for_bit(name, estimation):
    """The device's sums and entering T of pass k, fed to the specification's update, give exactly the
    T that the device enters pass k + 1 with (criteria 0: the loop never stops early)."""
    Tg = _inputs(name)[1]
    c = ref.pivot(Tg)
    prev = _run(name, estimation, 0, rel=(0.0, 0.0))
    assert np.array_equal(prev[0][:16], prev[1][29:])
    for k in (1, 2, 3):
        cur = _run(name, estimation, k, rel=(0.0, 0.0))
        want, degenerate, _ = ref.update(prev[1][:28], int(prev[1][28]), prev[1][29:].reshape(4, 4), c, estimation)
        assert not degenerate and cur[3] == 0 and cur[0][19] == k
        assert np.array_equal(cur[1][29:].reshape(4, 4), want), (name, estimation, k)
        assert np.array_equal(cur[0][:16], cur[1][29:])  # the last pass does not update
        prev = cur


@pytest.mark.parametrize("estimation", [0, 1])
def test_no_correspondence_is_the_identity_update(estimation):
    """m = 0: identity, the degenerate bit, and the loop's own count: one update, then no change."""
    S, Tg, Nt, r, _ = ref.case("subset")
    far = np.ascontiguousarray(S + np.array([0.0, 0.0, 40.0]))
    want = ref.registration(far, Tg, Nt, r, ref.motion(np.zeros(3)), estimation)
    res, _, corr, st = _ctx().registration_icp(_dev(far), _dev(Tg), r, ref.motion(np.zeros(3)), estimation,
                                               _dev(Nt) if estimation else None)
    res = res.cpu().numpy()
    assert want["iterations"] == 1 and want["status"] == ref.DEGENERATE and want["m"] == 0
    assert int(st.item()) == 2 and res[19] == 1 and res[16] == 0.0 and res[17] == 0.0 and res[18] == 0
    ev = _ctx().registration_icp(_dev(far), _dev(Tg), r, ref.motion(np.zeros(3)), estimation,
                                 _dev(Nt) if estimation else None, max_iteration=0, sums=True)[1].cpu().numpy()
    nxt, degenerate, _ = ref.update(ev[:28], int(ev[28]), ev[29:].reshape(4, 4), ref.pivot(Tg), estimation)
    assert degenerate and not ev[:29].any() and np.array_equal(nxt, res[:16].reshape(4, 4))  # the device's own sums
    assert np.array_equal(res[:16].reshape(4, 4), ref.motion(np.zeros(3))) and (corr.cpu().numpy() == -1).all()
    res = _ctx().registration_icp(_dev(far), _dev(Tg), r, None, estimation, _dev(Nt) if estimation else None, 0.0, 0.0,
                                  7)[0].cpu().numpy()
    assert res[19] == 7  # criteria 0 never stop the loop


def test_planar_target_is_degenerate_for_point_to_plane():
    """A target on z = 0 with normals (0, 0, 1): J's columns 2, 3, 4 are exactly 0, the third pivot is 0."""
    Tg = ref.lattice(8, 8, 1)
    Nt = np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (64, 1)))
    S = np.ascontiguousarray(Tg[5:50] + np.array([0.1, 0.1, 0.05]))
    want = ref.registration(S, Tg, Nt, 0.5, None, ref.PLANE)
    res, _, corr, st = _ctx().registration_icp(_dev(S), _dev(Tg), 0.5, None, 1, _dev(Nt))
    res = res.cpu().numpy()
    assert want["status"] == ref.DEGENERATE and want["m"] == 45 and int(st.item()) == 2
    ev = _ctx().registration_icp(_dev(S), _dev(Tg), 0.5, None, 1, _dev(Nt), max_iteration=0, sums=True)[1].cpu().numpy()
    nxt, degenerate, _ = ref.update(ev[:28], int(ev[28]), ev[29:].reshape(4, 4), ref.pivot(Tg), ref.PLANE)
    assert degenerate and ev[28] == 45 and ev[11] == 0.0 and np.array_equal(nxt, I4)  # [11] = sum J_2 J_2: the third pivot
    assert np.array_equal(res[:16].reshape(4, 4), I4) and res[19] == want["iterations"] == 1
    assert np.array_equal(corr.cpu().numpy(), want["correspondences"]) and res[16] == 1.0
    # point-to-point on the same clouds is well posed: the in-plane shift is found
    res, _, _, st = _ctx().registration_icp(_dev(S), _dev(Tg), 0.5, None, 0)
    assert int(st.item()) == 0 and np.abs(res.cpu().numpy()[:16].reshape(4, 4)[:3, 3] + [0.1, 0.1, 0.05]).max() < 1e-12


# ------------------------------------------------------------------ end to end
E2E = sorted(ref.ORDER_SPREAD)


@pytest.mark.parametrize("name,estimation,max_iteration", E2E, ids=[f"{n}-{e}-{m}" for n, e, m in E2E])
def test_registration_end_to_end(name, estimation, max_iteration):
    """The default criteria: the iteration count and the final correspondences equal the
    specification's, every entry of T is within 1000 x the CPU order-sensitivity figure (the device's
    tree is one more order of the same sums; one changed correspondence moves T by 1e-6 or more).
    partial / point-to-point slides and stops at max_iteration = 10.  Measured max |T - spec|: 5.6e-17
    and 2.4e-15 (subset plane, point), 6.7e-16 and 8.6e-15 (partial), 7.4e-12 and 2.5e-12 (far)."""
    want = ref.solved(name, estimation, max_iteration)
    res, _, corr, st = _run(name, estimation, max_iteration)
    T = res[:16].reshape(4, 4)
    tol = 1000.0 * ref.ORDER_SPREAD[(name, estimation, max_iteration)]
    print(f"{name} est {estimation}: {int(res[19])} updates, fitness {res[16]:.4f}, rmse {res[17]:.3e}, "
          f"max |T - spec| {np.abs(T - want['T']).max():.3e} (allowed {tol:.1e})")
    assert st == 0 and res[19] == want["iterations"]
    assert np.array_equal(corr, want["correspondences"]) and res[16] == want["fitness"]
    assert np.abs(T - want["T"]).max() <= tol
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    if name == "subset":  # the known motion, within the CPU test's bound
        assert np.abs(T - ref.case(name)[4]).max() <= 1000.0 * ref.KNOWN_MOTION_ERR[estimation]
    if (name, estimation) == ("partial", 0):
        assert res[19] == 10


def test_graph_capture():
    """A call captured into a graph and replayed gives the eager call's bits: nothing in the call
    waits for the host."""
    ctx = _ctx()
    S, Tg, Nt, r, _ = ref.case("subset")
    s, t, n = _dev(S), _dev(Tg), _dev(Nt)
    ws = torch.empty((ctx.icp_workspace_bytes(len(S), len(Tg)),), dtype=torch.uint8, device="cuda")
    eager = ctx.registration_icp(s, t, r, None, 1, n, workspace=ws, sums=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ctx.registration_icp(s, t, r, None, 1, n, workspace=ws, sums=True)
    for x in out:
        x.fill_(5)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert out[0][19].item() == ref.solved("subset", 1)["iterations"]


def test_empty_clouds_sentinels_and_refusals():
    ctx = _ctx()
    S, Tg, Nt, r, M = ref.case("subset")
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    for s, t in ((e, _dev(Tg)), (_dev(S), e), (e, e)):
        res, sums, corr, st = ctx.registration_icp(s, t, r, M, 1, t.clone(), sums=True)
        res = res.cpu().numpy()
        assert np.array_equal(res[:16].reshape(4, 4), M) and not res[16:].any() and int(st.item()) == 0
        assert (corr.cpu().numpy() == -1).all() and len(corr) == len(s)
    # nothing is written past n_source or past the stated workspace size; a dirty workspace serves
    from forest_slam_amd import _lib
    import ctypes
    wb = ctx.icp_workspace_bytes(len(S), len(Tg))
    ws = torch.full((wb + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    corr = torch.full((len(S) + 8,), -7, dtype=torch.int32, device="cuda")
    res = torch.full((24,), 123.0, dtype=torch.float64, device="cuda")
    s, t = _dev(S), _dev(Tg)
    rc = ctx.L.fvo_registration_icp(ctx.h, _lib._ptr(s), len(S), _lib._ptr(t), None, len(Tg), r, r,
                                    (ctypes.c_double * 16)(*I4.reshape(-1)), 0, 1e-6, 1e-6, 30, _lib._ptr(ws), wb,
                                    _lib._ptr(res), None, _lib._ptr(corr), None, _lib._stream(ctx.device))
    assert rc == 0
    torch.cuda.synchronize()
    want = ref.solved("subset", 0)
    assert np.array_equal(corr.cpu().numpy()[:len(S)], want["correspondences"]) and (corr[len(S):] == -7).all()
    assert (res[20:] == 123.0).all() and res[19].item() == want["iterations"] and (ws[wb:] == 0xFF).all()
    with pytest.raises(RuntimeError, match="point-to-plane needs target_normals"):
        ctx.registration_icp(_dev(S), _dev(Tg), r, None, 1)
    with pytest.raises(RuntimeError, match=r"max_correspondence_distance / cell must be <= 8"):
        ctx.registration_icp(_dev(S), _dev(Tg), r, cell=r / 9)
    with pytest.raises(RuntimeError, match=r"bottom row of init"):
        ctx.registration_icp(_dev(S), _dev(Tg), r, np.full((4, 4), 1.0))
    with pytest.raises(RuntimeError, match=r"max_iteration must be in \[0, 1000\]"):
        ctx.registration_icp(_dev(S), _dev(Tg), r, max_iteration=1001)


# ------------------------------------------------------------------ the Open3D-shaped face and PointMap
def test_registration_module_and_point_map():
    """PointMap.transform equals the specification's expression bit for bit on xyz64, xyz32 is its
    cast, the normals are rotated; PointMap.registration_icp against a second map returns what the raw
    call returns; point-to-plane on a target without normals raises; an append drops the normals."""
    from forest_slam_amd import registration as reg
    from forest_slam_amd.mapping import PointMap
    S, Tg, Nt, r, M = ref.case("subset")
    tgt, src = PointMap(2000), PointMap(2000)
    for pm, P in ((tgt, Tg), (src, S)):  # fp64 clouds put into the maps as they are
        pm.xyz64[:len(P)] = _dev(P)
        pm.xyz32[:len(P)] = _dev(P).to(torch.float32)
        pm.count += len(P)
    with pytest.raises(RuntimeError, match="no normals"):
        src.registration_icp(tgt, r, estimation_method=reg.TransformationEstimationPointToPlane())
    tgt.estimate_normals(30, 0.6)
    tgt.orient_normals_to_align_with_direction((0.0, 0.0, 1.0))
    assert np.array_equal(tgt.normals(), Nt)
    res = src.registration_icp(tgt, r, np.eye(4), reg.TransformationEstimationPointToPlane(),
                               reg.ICPConvergenceCriteria(max_iteration=30))
    raw = _run("subset", 1, 30)
    assert isinstance(res.result, torch.Tensor) and res.result.is_cuda  # on the device until asked for
    assert np.array_equal(res.transformation.reshape(-1), raw[0][:16]) and res.fitness == raw[0][16]
    assert res.inlier_rmse == raw[0][17] and res.iterations == raw[0][19] and res.status == 0
    k = np.flatnonzero(raw[2] >= 0)
    assert np.array_equal(res.correspondence_set, np.stack([k, raw[2][k]], axis=1))
    ev = reg.evaluate_registration(src, tgt, r, M)
    want = ref.evaluate(S, Tg, None, r, M)
    assert ev.fitness == want["fitness"] and ev.iterations == 0 and np.array_equal(ev.transformation, M)
    t2 = reg.registration_icp(_dev(S), _dev(Tg), r, target_normals=_dev(Nt),
                              estimation_method=reg.TransformationEstimationPointToPlane())
    assert np.array_equal(t2.transformation, res.transformation)
    # transform: the source map moved onto the target, the target's normals rotated
    T = res.transformation
    src.transform(T)
    moved = ref.transform(T, S)
    assert np.array_equal(src.cloud64(), moved) and np.array_equal(src.cloud32(), moved.astype(np.float32))
    assert np.abs(src.cloud64() - Tg[::2]).max() < 1e-12
    tgt.transform(M)
    assert tgt.has_normals() and np.array_equal(tgt.normals(), ref.rotate(M, Nt))
    assert np.array_equal(tgt.cloud64(), ref.transform(M, Tg))
    assert np.array_equal(tgt.cloud32(), ref.transform(M, Tg).astype(np.float32))
    tgt.add_cloud(Tg[:5].astype(np.float32) + np.float32(100.0), np.eye(4), voxel_size=0.01)
    assert not tgt.has_normals()
    with pytest.raises(RuntimeError, match="bottom row of T"):
        tgt.transform(np.full((4, 4), 2.0))
