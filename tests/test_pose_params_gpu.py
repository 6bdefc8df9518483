"""GPU parity of the pose stages beyond their default call (cases in pose_cases.py, each proven
to reach its branch in the oracle by test_pose_cases_cpu.py): fvo_pnp_ransac over the planar /
kept-model / no-model refinement branches, iteration counts around the 128-iteration first round
and the reproj / confidence parameters; fvo_find_essential + fvo_recover_pose over max_iters,
prob, threshold, degenerate scenes and capacities past the 64 KB LDS switch; fvo_backproject and
fvo_keypoint_stereo bit-exact on a hand-built disparity image; and, for both RANSACs, the same
frame at several batch slots and a second call on a context whose workspaces hold a harder batch.

Contexts hold only the stage under test with an explicit kp_capacity; the cases that share call
parameters run in one batched launch.  Tolerances are the project's existing ones: rvec / tvec
within 1e-4 scale + 1e-9 (test_gpu_parity.py), E / R / t within 1e-9 (test_mono.py)."""
import numpy as np
import pytest
import torch

import mono_cases as mc
import pose_cases as pc
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

PNP_CAP = 512
EM_CAP = 512
PP = (mc.CX, mc.CY)


# ---------------------------------------------------------------------------- PnP
def _pnp_pack(sets, cap):
    B = len(sets)
    P3 = np.zeros((B, cap, 3), np.float32)
    p2 = np.zeros((B, cap, 2), np.float32)
    n = np.zeros(B, np.int32)
    for b, (P, uv) in enumerate(sets):
        P3[b, :len(P)], p2[b, :len(P)], n[b] = P, uv, len(P)
    return torch.from_numpy(P3).cuda(), torch.from_numpy(p2).cuda(), torch.from_numpy(n).cuda()


def _pnp_run(ctx, sets, cap, reproj=1.0, confidence=0.99, iterations=1000):
    """One fvo_pnp_ransac launch -> dict of host arrays, with the per-frame RANSAC state (debug
    buffer 8: maxGood, niters, best_it, n) and per-iteration inlier counts (debug buffer 6)."""
    B = len(sets)
    P3, p2, n = _pnp_pack(sets, cap)
    keep = [t.clone() for t in (P3, p2, n)]
    rvec, tvec, T, st, inl = ctx.pnp_ransac(P3, p2, n, pc.K, pc.DIST, reproj=reproj, confidence=confidence,
                                            iterations=iterations)
    torch.cuda.synchronize()
    for a, b in zip(keep, (P3, p2, n)):
        assert torch.equal(a, b)  # the caller's inputs are unchanged
    state = ctx.debug_buffer(8).view(torch.int32).view(-1, 4)[:B].numpy().copy()
    good = ctx.debug_buffer(6).view(torch.int32)[:B * iterations].view(B, iterations).numpy().copy()
    return dict(rvec=rvec.cpu().numpy(), tvec=tvec.cpu().numpy(), T=T.cpu().numpy(), st=st.cpu().numpy(),
                inl=inl.cpu().numpy(), state=state, good=good)


def _frame(res, b):
    return {k: v[b] for k, v in res.items()}


def _pnp_groups():
    groups = {}
    for c in pc.pnp_cases():
        p = c["params"]
        groups.setdefault((p["reproj"], p["confidence"], p["iterations"], c["cap"] or PNP_CAP), []).append(c)
    return groups


SHORT = [(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32))] + [
    (pc.pnp_case("generic")["P"][:k], pc.pnp_case("generic")["uv"][:k]) for k in (3, 5)]


@pytest.fixture(scope="module")
def pnp_results():
    """name -> one frame's outputs, every case run in the launch of its parameter group; the
    default group also carries frames of 0, 3 and 5 points ("short_0/3/5")."""
    from forest_slam_amd import _lib
    ctx = _lib.Context(64, 64, max_batch=32, stages=_lib.STAGE_POSE, kp_capacity=PNP_CAP)
    out = {}
    for (reproj, conf, iters, cap), cases in _pnp_groups().items():
        sets = [(c["P"], c["uv"]) for c in cases]
        names = [c["name"] for c in cases]
        if (reproj, conf, iters, cap) == (1.0, 0.99, 1000, PNP_CAP):
            sets, names = sets + SHORT, names + ["short_0", "short_3", "short_5"]
        assert cap <= ctx.kp_cap and (cap < ctx.kp_cap) == (cases[0]["cap"] is not None)
        res = _pnp_run(ctx, sets, cap, reproj, conf, iters)
        for b, name in enumerate(names):
            out[name] = _frame(res, b)
    ctx.close()
    return out


def _assert_pnp_empty(f, status):
    assert f["st"] == status
    assert not f["rvec"].any() and not f["tvec"].any()
    assert np.array_equal(f["T"], np.eye(4))
    assert not f["inl"].any()


def _assert_pnp_matches(oracle_mod, case, f, check_counts=False):
    """The strong comparison of one frame with the oracle (stable cases)."""
    ok, r_ref, t_ref, inl_ref, iters, best, _ = pc.pnp_reference(oracle_mod, case)
    n = len(case["P"])
    assert f["st"] == int(ok)
    if not ok:
        _assert_pnp_empty(f, 0)
        return
    assert np.array_equal(np.nonzero(f["inl"][:n])[0], inl_ref)
    assert not f["inl"][n:].any()
    maxgood, niters, best_it, sn = f["state"]
    assert sn == n and maxgood == best
    assert max(niters, best_it + 1) == iters  # the serial loop ends at its bound or right after the last accept
    scale = max(np.abs(r_ref).max(), np.abs(t_ref).max(), 1e-3)
    assert np.abs(f["rvec"] - r_ref).max() <= 1e-4 * scale + 1e-9, (f["rvec"], r_ref)
    assert np.abs(f["tvec"] - t_ref).max() <= 1e-4 * scale + 1e-9, (f["tvec"], t_ref)
    assert np.abs(f["T"][:3, :3] - oracle_mod.rodrigues(f["rvec"])).max() <= 1e-12
    assert np.abs(f["T"][:3, 3] - f["tvec"]).max() <= 1e-12
    assert np.array_equal(f["T"][3], [0, 0, 0, 1])
    if check_counts:
        _, counts = oracle_mod.pnp_hypotheses(case["P"].astype(np.float64), case["uv"], pc.K, pc.DIST, iters=iters,
                                              reproj=case["params"]["reproj"])
        assert np.array_equal(f["good"][:iters], counts), np.nonzero(f["good"][:iters] != counts)[0][:5]


@pytest.mark.parametrize("name", [c["name"] for c in pc.pnp_cases()])
def test_pnp_case_matches_oracle(oracle_mod, pnp_results, name):
    case, f = pc.pnp_case(name), pnp_results[name]
    n = len(case["P"])
    ok = pc.pnp_reference(oracle_mod, case)[0]
    assert f["st"] == int(ok)
    if name in pc.UNSTABLE_PNP:  # two correct implementations need not agree beyond the status
        assert all(np.isfinite(f[k]).all() for k in ("rvec", "tvec", "T"))
        assert not f["inl"][n:].any() and set(np.unique(f["inl"])) <= {0, 1}
        return
    _assert_pnp_matches(oracle_mod, case, f, check_counts=name.startswith("iters_"))
    if name == "no_model":
        _assert_pnp_empty(f, 0)


def test_pnp_fewer_than_six_points(pnp_results):
    for name in ("short_0", "short_3", "short_5"):
        _assert_pnp_empty(pnp_results[name], -1)


def _same_frame(a, b, keys):
    return all(np.array_equal(a[k], b[k]) for k in keys)


PNP_OUT = ("rvec", "tvec", "T", "st", "inl")


def test_pnp_batch_position_and_neighbours(oracle_mod):
    """A frame that needs RANSAC round 2 at the first, a middle and the last slot of a batch,
    between easy, empty and other hard frames: bit-identical in every slot and to a batch of
    one (k_pnp_plan's prefix sums hand every frame exactly its own units)."""
    from forest_slam_amd import _lib
    hard = pc.pnp_case("hard_default")
    assert pc.pnp_reference(oracle_mod, hard)[4] > pc.PNP_FIRST
    H = (hard["P"], hard["uv"])
    easy = tuple(pc.pnp_case("generic")[k] for k in ("P", "uv"))
    hard2 = tuple(pc.pnp_case("no_model")[k] for k in ("P", "uv"))  # never accepts: all 1000 iterations
    clean = tuple(pc.pnp_case("iters_1_clean")[k] for k in ("P", "uv"))
    sets = [H, easy, SHORT[1], hard2, H, SHORT[0], clean, hard2, H]
    ctx = _lib.Context(64, 64, max_batch=len(sets), stages=_lib.STAGE_POSE, kp_capacity=PNP_CAP)
    res = _pnp_run(ctx, sets, PNP_CAP)
    one = _frame(_pnp_run(_lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_POSE, kp_capacity=PNP_CAP), [H],
                          PNP_CAP), 0)
    _assert_pnp_matches(oracle_mod, hard, one)
    for slot in (0, 4, 8):
        f = _frame(res, slot)
        assert _same_frame(f, one, PNP_OUT), slot
        assert np.array_equal(f["state"], one["state"]), slot
    _assert_pnp_matches(oracle_mod, pc.pnp_case("generic"), _frame(res, 1))
    _assert_pnp_empty(_frame(res, 2), -1)
    _assert_pnp_empty(_frame(res, 5), -1)


def test_pnp_second_call_ignores_the_first_calls_workspace(oracle_mod):
    """A batch of hard frames (round 2, 1000 iterations), then on the same context easy frames
    with iterations = 100 and other point counts: bit-identical to that call on a fresh context
    (pnp_good, pnp_models, pnp_plan and the per-frame state still hold the first call)."""
    from forest_slam_amd import _lib
    hard = [tuple(pc.pnp_case(nm)[k] for k in ("P", "uv")) for nm in ("hard_default", "no_model", "param_defaults",
                                                                     "hard_default")]
    easy = [tuple(pc.pnp_case(nm)[k] for k in ("P", "uv")) for nm in ("generic", "planar_clean", "five_inliers")]
    easy = [easy[0], SHORT[1], easy[1], easy[2]]
    used = _lib.Context(64, 64, max_batch=4, stages=_lib.STAGE_POSE, kp_capacity=PNP_CAP)
    first = _pnp_run(used, hard, PNP_CAP)
    assert (first["state"][:, 1] > pc.PNP_FIRST).sum() >= 3
    second = _pnp_run(used, easy, PNP_CAP, iterations=100)
    fresh = _pnp_run(_lib.Context(64, 64, max_batch=4, stages=_lib.STAGE_POSE, kp_capacity=PNP_CAP), easy, PNP_CAP,
                     iterations=100)
    for k in PNP_OUT + ("state",):
        assert np.array_equal(second[k], fresh[k]), k
    for b in range(4):  # the iterations that the serial loop ran
        ran = max(fresh["state"][b, 1], fresh["state"][b, 2] + 1) if fresh["state"][b, 3] >= 6 else 0
        assert np.array_equal(second["good"][b, :ran], fresh["good"][b, :ran]), b
    ref = oracle_mod.solve_pnp_ransac(easy[0][0].astype(np.float64), easy[0][1], pc.K, pc.DIST, iters=100)
    assert second["st"][0] == int(ref[0]) and np.array_equal(np.nonzero(second["inl"][0])[0], ref[3])


# ---------------------------------------------------------------------------- essential matrix
def _em_pack(sets, cap):
    B = len(sets)
    P0 = np.zeros((B, cap, 2), np.float32)
    P1 = np.zeros((B, cap, 2), np.float32)
    n = np.zeros(B, np.int32)
    for b, (p0, p1) in enumerate(sets):
        P0[b, :len(p0)], P1[b, :len(p1)], n[b] = p0, p1, len(p0)
    return torch.from_numpy(P0).cuda(), torch.from_numpy(P1).cuda(), torch.from_numpy(n).cuda()


def _em_run(ctx, sets, cap, prob=0.999, threshold=1.0, max_iters=1000, use_status=True):
    P0, P1, n = _em_pack(sets, cap)
    keep = [t.clone() for t in (P0, P1, n)]
    E, mask, st = ctx.find_essential(P0, P1, n, mc.F, PP, prob=prob, threshold=threshold, max_iters=max_iters)
    R, t, T, g = ctx.recover_pose(E, P0, P1, n, mc.F, PP, e_status=st if use_status else None)
    torch.cuda.synchronize()
    for a, b in zip(keep, (P0, P1, n)):
        assert torch.equal(a, b)
    return {k: v.cpu().numpy() for k, v in dict(E=E, mask=mask, st=st, R=R, t=t, T=T, g=g).items()}


EM_OUT = ("E", "mask", "st", "R", "t", "T", "g")


def _em_groups():
    groups = {}
    for c in pc.em_cases():
        p = c["params"]
        groups.setdefault((p["prob"], p["threshold"], p["max_iters"], c["cap"]), []).append(c)
    return groups


@pytest.fixture(scope="module")
def em_results():
    from forest_slam_amd import _lib
    out, ctxs = {}, {}
    for (prob, thr, iters, cap), cases in _em_groups().items():
        if cap not in ctxs:
            ctxs[cap] = _lib.Context(64, 64, max_batch=32 if cap == EM_CAP else 1, stages=_lib.STAGE_MONO,
                                     kp_capacity=cap)
        res = _em_run(ctxs[cap], [(c["p0"], c["p1"]) for c in cases], cap, prob, thr, iters)
        for b, c in enumerate(cases):
            out[c["name"]] = _frame(res, b)
    for ctx in ctxs.values():
        ctx.close()
    return out


def _assert_em_matches(oracle_mod, case, f):
    ref = pc.em_reference(oracle_mod, case)
    n = len(case["p0"])
    assert f["st"] == ref["status"]
    if ref["status"] != 1:
        assert f["g"] == -1 and np.array_equal(f["T"], np.eye(4))
        return
    assert np.abs(f["E"] - ref["E"]).max() < 1e-9
    assert np.array_equal(f["mask"][:n], ref["mask"]) and not f["mask"][n:].any()
    assert f["g"] == ref["good"]
    assert np.abs(f["R"] - ref["R"]).max() < 1e-9 and np.abs(f["t"] - ref["t"]).max() < 1e-9
    assert np.array_equal(f["T"][:3, :3], f["R"]) and np.array_equal(f["T"][:3, 3], f["t"])
    assert np.array_equal(f["T"][3], [0, 0, 0, 1])


@pytest.mark.parametrize("name", [c["name"] for c in pc.em_cases()])
def test_essential_case_matches_oracle(oracle_mod, em_results, name):
    case, f = pc.em_case(name), em_results[name]
    n = len(case["p0"])
    assert f["st"] == pc.em_reference(oracle_mod, case)["status"]
    if name in pc.UNSTABLE_EM:  # two correct implementations need not agree beyond the status
        assert all(np.isfinite(f[k]).all() for k in ("E", "R", "t", "T"))
        assert not f["mask"][n:].any() and set(np.unique(f["mask"])) <= {0, 1}
        if name == "pure_rotation":
            # p1 == p0 satisfies x^T E x = 0 for every E = [t]x, whichever t a solver returns (the
            # oracle's mask does not move under the one-ulp classification either): all inliers.
            # The first subset's polynomial is degree-trimmed, so this is k_em_roots' tested copy.
            assert f["mask"][:n].all() and pc.em_reference(oracle_mod, case)["mask"].all()
        return
    _assert_em_matches(oracle_mod, case, f)


def test_recover_pose_without_status(oracle_mod):
    """fvo_recover_pose with e_status = NULL on sets that all have an essential matrix."""
    from forest_slam_amd import _lib
    cases = [pc.em_case(nm) for nm in ("param_defaults", "planar_scene", "deep_points", "backward_or_sideways")]
    assert all(pc.em_reference(oracle_mod, c)["status"] == 1 for c in cases)
    ctx = _lib.Context(64, 64, max_batch=len(cases), stages=_lib.STAGE_MONO, kp_capacity=EM_CAP)
    res = _em_run(ctx, [(c["p0"], c["p1"]) for c in cases], EM_CAP, use_status=False)
    for b, c in enumerate(cases):
        _assert_em_matches(oracle_mod, c, _frame(res, b))


def test_essential_batch_position_and_neighbours(oracle_mod):
    """As test_pnp_batch_position_and_neighbours for the essential RANSAC: a frame that runs past
    the 128-subset first round at the first, a middle and the last slot."""
    from forest_slam_amd import _lib
    hard = pc.em_case("param_defaults")
    assert pc.em_reference(oracle_mod, hard)["iters"] > pc.PNP_FIRST
    H = (hard["p0"], hard["p1"])
    easy = tuple(pc.em_case("planar_scene")[k] for k in ("p0", "p1"))
    hard2 = tuple(pc.em_case("pure_noise_100")[k] for k in ("p0", "p1"))
    few = (hard["p0"][:3], hard["p1"][:3])
    none = (hard["p0"][:0], hard["p1"][:0])
    sets = [H, easy, few, hard2, H, none, easy, hard2, H]
    ctx = _lib.Context(64, 64, max_batch=len(sets), stages=_lib.STAGE_MONO, kp_capacity=EM_CAP)
    res = _em_run(ctx, sets, EM_CAP)
    one = _frame(_em_run(_lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_MONO, kp_capacity=EM_CAP), [H], EM_CAP), 0)
    _assert_em_matches(oracle_mod, hard, one)
    for slot in (0, 4, 8):
        assert _same_frame(_frame(res, slot), one, EM_OUT), slot
    _assert_em_matches(oracle_mod, pc.em_case("planar_scene"), _frame(res, 1))
    for slot in (2, 5):
        assert res["st"][slot] == -1 and res["g"][slot] == -1 and np.array_equal(res["T"][slot], np.eye(4))


def test_essential_second_call_ignores_the_first_calls_workspace(oracle_mod):
    """A batch of hard sets at max_iters 1000, then easy sets at max_iters 64 on the same context:
    bit-identical to that call on a fresh context (em_good, em_nmod, em_models and the per-frame
    state still hold the first call)."""
    from forest_slam_amd import _lib
    hard = [tuple(pc.em_case(nm)[k] for k in ("p0", "p1")) for nm in ("param_defaults", "pure_noise_100",
                                                                      "threshold_0.25", "param_defaults")]
    e = [tuple(pc.em_case(nm)[k] for k in ("p0", "p1")) for nm in ("planar_scene", "deep_points", "five_points_60")]
    easy = [e[0], (e[0][0][:4], e[0][1][:4]), e[1], e[2]]
    used = _lib.Context(64, 64, max_batch=4, stages=_lib.STAGE_MONO, kp_capacity=EM_CAP)
    _em_run(used, hard, EM_CAP)
    second = _em_run(used, easy, EM_CAP, max_iters=64)
    fresh = _em_run(_lib.Context(64, 64, max_batch=4, stages=_lib.STAGE_MONO, kp_capacity=EM_CAP), easy, EM_CAP,
                    max_iters=64)
    for k in EM_OUT:
        assert np.array_equal(second[k], fresh[k]), k
    rst, rE, rmask, _, _ = oracle_mod.find_essential(easy[0][0], easy[0][1], mc.F, PP, max_iters=64)
    assert second["st"][0] == rst == 1 and np.array_equal(second["mask"][0, :len(rmask)], rmask)
    assert np.abs(second["E"][0] - rE).max() < 1e-9


# ---------------------------------------------------------------------------- back-projection
def _dev(bp, *names):
    return [torch.from_numpy(np.array(bp[k])).cuda() for k in names]


def test_backproject_bit_exact(oracle_mod):
    """fvo_backproject against oracle.backproject(oracle.disparity_map(.)) on a hand-built int16
    disparity image: the special values, the 0.1 < Z < 1000 edges, (int)x truncation at the last
    column and row, an ordered compaction that crosses a block pass, frames with every match
    kept, none kept, n_matches 0 and n_matches = cap."""
    from forest_slam_amd import _lib
    bp = pc.backproject_case()
    B, cap = bp["matches"].shape[:2]
    ctx = _lib.Context(pc.BP_W, pc.BP_H, max_batch=B, stages=_lib.STAGE_POSE, kp_capacity=cap)
    args = _dev(bp, "disp", "kp0", "kp1", "matches", "n_matches")
    keep = [t.clone() for t in args]
    P3 = torch.full((B, cap, 3), -7.0, dtype=torch.float32, device="cuda")
    p2 = torch.full((B, cap, 2), -7.0, dtype=torch.float32, device="cuda")
    npts = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ctx.backproject(*args, pc.K, pc.BASELINE, out=(P3, p2, npts))
    torch.cuda.synchronize()
    for a, b in zip(keep, args):
        assert torch.equal(a, b)
    P3, p2, npts = P3.cpu().numpy(), p2.cpu().numpy(), npts.cpu().numpy()
    ref = pc.backproject_reference(oracle_mod, bp)
    kept = [len(r[0]) for r in ref]
    assert kept[0] == cap and kept[1] == 0 and kept[3] == 0 and pc.BP_BLOCK < kept[4] < cap and 0 < kept[2] < 300
    for b, (rP, rp2, valid) in enumerate(ref):
        k = len(rP)
        assert npts[b] == k, b
        assert np.array_equal(P3[b, :k].view(np.uint32), rP.view(np.uint32)), b
        assert np.array_equal(p2[b, :k].view(np.uint32), rp2.view(np.uint32)), b
        assert (P3[b, k:] == -7).all() and (p2[b, k:] == -7).all(), b  # nothing written past n_points


def test_keypoint_stereo_bit_exact(oracle_mod):
    """fvo_keypoint_stereo on the same image: (X, Y, Z, d) per keypoint by the same arithmetic,
    zeros where 0.1 < Z < 1000 fails and zeros past n_keypoints."""
    from forest_slam_amd import _lib
    bp = pc.backproject_case()
    B, cap = bp["kp0"].shape[:2]
    ctx = _lib.Context(pc.BP_W, pc.BP_H, max_batch=B, stages=_lib.STAGE_BA, kp_capacity=cap, ba_window=3)
    args = _dev(bp, "disp", "kp0", "n_kp")
    keep = [t.clone() for t in args]
    out = torch.full((B, cap, 4), -7.0, dtype=torch.float32, device="cuda")
    ctx.keypoint_stereo(*args, pc.K, pc.BASELINE, out=out)
    torch.cuda.synchronize()
    for a, b in zip(keep, args):
        assert torch.equal(a, b)
    ref = pc.keypoint_stereo_reference(oracle_mod, bp)
    assert (ref[0, :, 2] > 0).all() and not ref[3].any() and 0 < (ref[2, :, 2] > 0).sum() < cap
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
