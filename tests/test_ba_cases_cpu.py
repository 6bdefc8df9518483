"""The local-BA case table (tests/ba_cases.py) on the oracle alone, without a GPU: every case runs,
reaches what it is for, and none of its discrete decisions sits on a rounding edge, so the GPU
tests (test_ba_cases_gpu.py) may compare counts and the number of accepted LM steps exactly."""
import numpy as np
import pytest

import ba_cases as bc
import ba_synth

MARGIN = 1e-6


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_reaches_and_is_decisive(name):
    i = bc.Info(name)
    assert i.case["reaches"](i), i.case["reach"]
    live = 0
    for w, ref in enumerate(i.refs):
        if ref is None:
            continue
        live += 1
        assert len(ref["trace"]) == (i.case["call"]["iterations"] if len(ref["X"]) else 0)
        assert sum(t["accepted"] for t in ref["trace"]) == ref["accepted"]
        for k, t in enumerate(ref["trace"]):
            assert t["c2"] is not None, "Cholesky failure in the oracle: window %d iteration %d" % (w, k)
            assert abs(t["c2"] - t["cost"]) >= MARGIN * t["cost"], (w, k, t)
            if "reject_margin" in t:
                assert t["reject_margin"] >= MARGIN, (w, k, t)
    assert live >= 1


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_is_well_conditioned(name):
    """The oracle against itself in another summation order (observations reversed within each
    landmark, the Schur loop backwards): the same decisions, and 100 times what its own rounding
    moves stays inside the GPU test's tolerances on cost (1e-8 of cost0) and T_out (1e-8).  Measured
    over the table: cost <= 5.3e-15 of cost0, T_out <= 7.4e-12 (landmarks_1: one landmark holds four
    poses).  The landmarks of the problems with outlier matches are softer (a landmark left with
    little parallax after the rejection moves along its ray): up to 1.7e-7 (cap_birth_frame_2),
    which the 1e-6 of test_ba.py covers 6 times, not 100, so for the landmarks the bound is a fifth
    of that tolerance; the cases without outliers stay below 4e-9.  A case that is ill-conditioned
    outright (no_stereo_first at 10 iterations: 3.1e-4) fails here."""
    for w, ref in enumerate(bc.oracle(name)):
        if ref is None or len(ref["X"]) == 0:
            continue
        alt = bc.oracle_reordered(name, w)
        assert [t["accepted"] for t in alt["trace"]] == [t["accepted"] for t in ref["trace"]]
        assert 100 * abs(alt["cost"] - ref["cost"]) <= 1e-8 * ref["cost0"]
        assert 100 * np.abs(alt["rel"][-1] - ref["rel"][-1]).max() <= 1e-8
        assert np.abs(alt["X"] - ref["X"]).max() <= 1e-6 / 5


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_inputs_are_valid(name):
    """The preconditions of fvo_ba_windows on the clean and on the poisoned arrays, and creation-time
    depths off their thresholds: a stored depth is 0 (invalid) or inside (0.1, 1000) by more than a
    float32 ulp, so `valid` cannot differ between two correct readers."""
    f32 = np.float32
    for p in (bc.problem(name), bc.poisoned(name)):
        F, cap = p["kp"].shape[:2]
        assert cap == bc.CASES[name]["cfg"]["kp_capacity"] and F == bc.CASES[name]["gen"]["n"]
        assert np.all((p["matches"][:, :, :2] >= 0) & (p["matches"][:, :, :2] < cap))
        assert np.all(np.isfinite(p["kp"])) and np.all(np.isfinite(p["stereo"])) and np.all(np.isfinite(p["T_rel"]))
        for f in range(F):
            nk, nm = int(p["nkp"][f]), int(p["nmatch"][f])
            assert 0 <= nk <= cap and 0 <= nm <= cap
            m = p["matches"][f, :nm]
            assert len(set(m[:, 0])) == nm, "a query index twice in frame %d" % f
            if p is not bc.problem(name) and f in bc.outside_frames(bc.CASES[name]):
                continue  # a poisoned frame: indices inside [0, cap) is all it promises
            assert np.all(m[:, 0] < nk)
            if f + 1 < F:
                assert np.all(m[:, 1] < p["nkp"][f + 1])
        Z = p["stereo"][:, :, 2]
        lo, hi = np.nextafter(f32(0.1), f32(1)), np.nextafter(f32(1000), f32(0))
        assert np.all((Z == 0) | ((Z > lo) & (Z < hi)))


def test_poison_changes_what_it_covers():
    """ba_synth.poison leaves the frames and rows of the call alone and changes everything else."""
    name = "first_valid_slide"
    case, p, q = bc.CASES[name], bc.problem(name), bc.poisoned(name)
    out = bc.outside_frames(case)
    assert out == [0, 1, 2, 9]
    for f in range(case["gen"]["n"]):
        nk, nm = int(p["nkp"][f]), int(p["nmatch"][f])
        if f in out:
            assert q["nmatch"][f] == q["nkp"][f] == 512 and not np.array_equal(p["T_rel"][f], q["T_rel"][f])
            assert not np.array_equal(p["kp"][f], q["kp"][f]) and not np.array_equal(p["stereo"][f], q["stereo"][f])
            R = q["T_rel"][f][:3, :3]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.array_equal(q["T_rel"][f][3], [0, 0, 0, 1])
        else:
            assert (q["nkp"][f], q["nmatch"][f]) == (nk, nm) and np.array_equal(p["T_rel"][f], q["T_rel"][f])
            for k, n in (("kp", nk), ("stereo", nk), ("matches", nm)):
                assert np.array_equal(p[k][f, :n], q[k][f, :n])
                assert n == 512 or not np.array_equal(p[k][f, n:], q[k][f, n:])


def test_generator_defaults_unchanged():
    """The keyword arguments added to clean_problem default to what it did before: the counts
    test_ba.py hard-codes for this problem (oracle/ba_ref.py on the CPU) still hold."""
    import ba_ref
    p = ba_synth.clean_problem(n=7, n_pts=400, seed=11, drop=0.05, cap=512)
    q = ba_synth.clean_problem(n=7, n_pts=400, seed=11, drop=0.05, cap=512, K=ba_synth.K_TEST, B=ba_synth.B_TEST,
                               octaves=(0, 3), one_to_one=True)
    assert all(np.array_equal(p[k], q[k]) for k in p)
    kps, matches, st, rel = ba_synth.oracle_lists(p, 0, 2)
    _, X, obs = ba_ref.build_problem(kps, matches, st, rel)
    assert (len(X), len(obs["lm"])) == (333, 946)


def test_oracle_clamp_and_trace_are_additive():
    """n_levels=None reproduces the oracle without the clamp; with octaves inside the table the clamp
    changes nothing; outside it changes the weights."""
    import ba_ref
    p = bc.problem("octaves_clamped")
    kps, matches, st, rel = ba_synth.oracle_lists(p, 0, 4)
    a = ba_ref.build_problem(kps, matches, st, rel)[2]["isig2"]
    b = ba_ref.build_problem(kps, matches, st, rel, n_levels=12)[2]["isig2"]
    c = ba_ref.build_problem(kps, matches, st, rel, n_levels=8)[2]["isig2"]
    assert a.max() == 1.0 / 1.2 ** -2 and b.max() == 1.0 and np.array_equal(a[a <= 1], b[a <= 1])
    assert c.min() == 1.0 / 1.2 ** 14 and a.min() == 1.0 / 1.2 ** 18


def test_make_dims_constants():
    """The restated launch shape at the shapes the table relies on."""
    assert (bc.LMAX_NPART1, bc.LMAX_NPART2, bc.LMAX_NPART12) == (960, 1024, 6144)
    lmax = (960, 961, 1024, 4096, 6080, 6144, 1 << 16)
    assert [bc.make_dims(10, L)["NPART"] for L in lmax] == [1, 2, 2, 8, 11, 12, 12]
    assert [bc.make_dims(K, 4096)["NR"] for K in (3, 11, 12, 21)] == [64, 64, 128, 128]
    assert [bc.make_dims(K, 4096)["LPU"] for K in (16, 17)] == [128, 64]
    assert [bc.make_dims(K, 4096)["solve_shm"] > 65536 for K in (14, 15)] == [False, True]
    assert not bc.global_maps(4, 512) and bc.global_maps(4, 24576) and not bc.global_maps(21, 3072)
