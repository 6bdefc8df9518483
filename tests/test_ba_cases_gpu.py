"""fvo_ba_windows / fvo_ba_count_births / fvo_ba_landmarks over the case table of tests/ba_cases.py.

Oracle parity per case and window (oracle/ba_ref.py, float64): landmark, observation and frame
counts and the number of accepted LM steps exactly (test_ba_cases_cpu.py shows that no decision
of the oracle sits on a rounding edge), cost0 / cost / T_out / landmarks within the tolerances of
test_ba.py (1e-9 relative, 1e-8 of cost0, 1e-8, 1e-6).  Measured over the table on an MI355X:
cost0 <= 3.7e-15, cost <= 6e-15, T_out <= 5e-12 (cap_obs_one_less), landmarks <= 1.3e-7
(first_valid_slide; the problems with outlier matches have soft landmarks, see
test_case_is_well_conditioned).  The solver reads the poisoned arrays
of every case, the oracle the clean ones.

Bitwise invariances, no oracle involved (every reduction of csrc/ba.hip has a fixed order): what
the call must not read, first_valid against sliced arrays, the births-ahead cache and its
invalidation, and a used context against a fresh one in both homes of the match maps."""
import numpy as np
import pytest
import torch

import ba_cases as bc
import ba_synth
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

_ARRAYS = ("kp", "nkp", "matches", "nmatch", "stereo", "T_rel")


def _context(cfg, max_batch):
    from forest_slam_amd import _lib
    return _lib.Context(64, 64, max_batch=max_batch, stages=_lib.STAGE_BA, **cfg)


def _device(p):
    return {k: torch.from_numpy(np.ascontiguousarray(p[k])).cuda() for k in _ARRAYS}


def _windows(ctx, d, p, call):
    """One fvo_ba_windows call and every window's landmarks, on the host."""
    T, stats = ctx.ba_windows(d["kp"], d["nkp"], d["matches"], d["nmatch"], d["stereo"], d["T_rel"], call["first_end"],
                              call["n_windows"], call["first_valid"], p["K"], p["B"], iterations=call["iterations"],
                              scale_factor=call["scale_factor"])
    lms = []
    for w in range(call["n_windows"]):
        xyz, cnt = ctx.ba_landmarks(w)
        lms.append(xyz[:int(cnt.item())].cpu().numpy())
    torch.cuda.synchronize()
    return dict(T=T.cpu().numpy(), stats=stats.cpu().numpy(), lms=lms)


def _births(ctx, d, call):
    ctx.ba_count_births(d["matches"], d["nmatch"], d["stereo"], call["first_end"], call["n_windows"],
                        call["first_valid"])


def _fresh(p, cfg, call, max_batch=None):
    ctx = _context(cfg, max_batch or call["n_windows"])
    return _windows(ctx, _device(p), p, call)


_RUNS = {}


def _run(name, poisoned=True):
    """The case's call on a fresh context (cached: the tests share the runs)."""
    if (name, poisoned) not in _RUNS:
        case = bc.CASES[name]
        _RUNS[name, poisoned] = _fresh(bc.poisoned(name) if poisoned else bc.problem(name), case["cfg"], case["call"])
    return _RUNS[name, poisoned]


def _assert_bitwise(a, b):
    assert np.array_equal(a["T"], b["T"])
    assert np.array_equal(a["stats"], b["stats"])
    assert len(a["lms"]) == len(b["lms"])
    for xa, xb in zip(a["lms"], b["lms"]):
        assert xa.shape == xb.shape and np.array_equal(xa, xb)


@pytest.mark.parametrize("name", bc.NAMES)
def test_gpu_ba_case_matches_oracle(name):
    case, p, refs = bc.CASES[name], bc.problem(name), bc.oracle(name)
    got = _run(name)
    for (w, s, e), ref in zip(bc.windows(case), refs):
        T, st, X = got["T"][w], got["stats"][w], got["lms"][w]
        n = e - s + 1
        if ref is None or len(ref["X"]) == 0:  # a pass-through window
            assert np.array_equal(T, p["T_rel"][e - 1]), (name, w)
            assert np.array_equal(st, [0, 0, 0, 0, n, 0]) and len(X) == 0, (name, w, st)
            continue
        dc0 = abs(st[0] - ref["cost0"]) / ref["cost0"]
        dc = abs(st[1] - ref["cost"]) / ref["cost0"]
        dT = np.abs(T - ref["rel"][-1]).max()
        dX = np.abs(X - ref["X"]).max() if X.shape == ref["X"].shape else np.inf
        print("%s w%d: L %d/%d O %d/%d n %d/%d accepted %d/%d  dcost0 %.2e dcost %.2e dT %.2e dX %.2e" % (
            name, w, st[2], len(ref["X"]), st[3], len(ref["obs"]["lm"]), st[4], n, st[5], ref["accepted"], dc0, dc, dT,
            dX))
        assert (st[2], st[3], st[4]) == (len(ref["X"]), len(ref["obs"]["lm"]), n), (name, w)
        assert st[5] == ref["accepted"], (name, w)
        assert dc0 <= 1e-9 and dc <= 1e-8, (name, w)
        assert dT < 1e-8, (name, w)
        assert dX < 1e-6, (name, w)


@pytest.mark.parametrize("name", bc.NAMES)
def test_gpu_ba_unread_data(name):
    """Frames outside [first_valid, last end] and rows beyond the counts are not read: the poisoned
    arrays give the bits of the clean ones."""
    p, q = bc.problem(name), bc.poisoned(name)
    assert any(not np.array_equal(p[k], q[k]) for k in _ARRAYS)
    _assert_bitwise(_run(name, poisoned=True), _run(name, poisoned=False))


@pytest.mark.parametrize("name", ["first_valid_1", "first_valid_pair", "first_valid_slide"])
def test_gpu_ba_first_valid_is_a_slice(name):
    """first_valid = v on the full arrays against first_valid = 0 on the arrays from frame v on."""
    case = bc.CASES[name]
    v = case["call"]["first_valid"]
    call = dict(case["call"], first_end=case["call"]["first_end"] - v, first_valid=0)
    _assert_bitwise(_run(name, poisoned=False), _fresh(bc.sliced(bc.problem(name), v), case["cfg"], call))


# ---- the births-ahead cache (fvo_ba_count_births) on the 12-frame sliding problem, window 4
# (first_valid = 1 cuts the first window, ending at frame 3, to frames 1..3)
_B_CALL = dict(bc.CASES["sliding_9"]["call"], first_end=3, n_windows=5, first_valid=1)


def _sliding_fresh(call):
    key = ("sliding", tuple(sorted(call.items())))
    if key not in _RUNS:
        _RUNS[key] = _fresh(bc.problem("sliding_9"), bc.CASES["sliding_9"]["cfg"], call, max_batch=9)
    return _RUNS[key]


@pytest.mark.parametrize("other", [dict(first_end=4), dict(n_windows=4), dict(first_valid=0)],
                         ids=["first_end", "n_windows", "first_valid"])
def test_gpu_ba_births_ahead_of_another_range(other):
    """fvo_ba_count_births for one range, fvo_ba_windows for another (one argument differs): the
    counts are not reused."""
    p = bc.problem("sliding_9")
    ctx, d = _context(bc.CASES["sliding_9"]["cfg"], 9), _device(p)
    _births(ctx, d, dict(_B_CALL, **other))
    _assert_bitwise(_windows(ctx, d, p, _B_CALL), _sliding_fresh(_B_CALL))


def test_gpu_ba_births_ahead_after_another_call():
    """fvo_ba_count_births, an fvo_ba_windows call of another range (which invalidates the counts),
    then the call the counts were made for."""
    p = bc.problem("sliding_9")
    ctx, d = _context(bc.CASES["sliding_9"]["cfg"], 9), _device(p)
    other = dict(_B_CALL, first_end=6, n_windows=3)
    _births(ctx, d, _B_CALL)
    _assert_bitwise(_windows(ctx, d, p, other), _sliding_fresh(other))
    _assert_bitwise(_windows(ctx, d, p, _B_CALL), _sliding_fresh(_B_CALL))


def test_gpu_ba_births_ahead_then_landmarks():
    """fvo_ba_count_births, fvo_ba_landmarks (of the previous call), then the matching
    fvo_ba_windows, which uses the counts."""
    p = bc.problem("sliding_9")
    ctx, d = _context(bc.CASES["sliding_9"]["cfg"], 9), _device(p)
    first = _windows(ctx, d, p, _B_CALL)
    _births(ctx, d, _B_CALL)
    xyz, cnt = ctx.ba_landmarks(2)
    assert np.array_equal(xyz[:int(cnt.item())].cpu().numpy(), first["lms"][2])
    _assert_bitwise(_windows(ctx, d, p, _B_CALL), _sliding_fresh(_B_CALL))
    _assert_bitwise(first, _sliding_fresh(_B_CALL))


def test_gpu_ba_births_ahead_two_streams():
    """Births ahead with 9 windows: both streams of the split consume the ahead counts."""
    case, p = bc.CASES["sliding_9"], bc.problem("sliding_9")
    ctx, d = _context(case["cfg"], 9), _device(p)
    _births(ctx, d, case["call"])
    _assert_bitwise(_windows(ctx, d, p, case["call"]), _run("sliding_9", poisoned=False))


def test_gpu_ba_two_live_contexts():
    """Two contexts alive at once whose kernels need different amounts of dynamic LDS (ba_init raises
    the per-function limits for its own shape: k_ba_lin 101376 B at NR = 64, 99840 B at NR = 128;
    k_ba_solve 152704 B at K = 21, 89984 B at K = 17): creating the second must not break the first."""
    runs = []
    for first, second in (("landmarks_33", "window_17"), ("window_21", "window_17")):
        if first == "window_21":  # the K = 21 window of test_ba.py at fewer points
            p1 = ba_synth.clean_problem(n=21, seed=5, n_pts=200, cap=512)
            cfg1 = dict(bc.CASES["window_17"]["cfg"], ba_window=21)
            call1 = dict(bc.CASES["window_17"]["call"], first_end=20)
        else:
            p1, cfg1, call1 = bc.problem(first), bc.CASES[first]["cfg"], bc.CASES[first]["call"]
        p2, cfg2, call2 = bc.problem(second), bc.CASES[second]["cfg"], bc.CASES[second]["call"]
        alone = _fresh(p1, cfg1, call1)
        ctx1 = _context(cfg1, 1)
        ctx2 = _context(cfg2, 1)
        _assert_bitwise(_windows(ctx2, _device(p2), p2, call2), _run(second, poisoned=False))
        _assert_bitwise(_windows(ctx1, _device(p1), p1, call1), alone)
        runs.append(alone)
    assert runs[1]["stats"][0][4] == 21 and runs[1]["stats"][0][2] > 0


# ---- state carried in the context: a small problem (its first window has no landmark, its second
# fewer frames' worth) after a large one, against a fresh context, in both homes of the match maps
@pytest.mark.parametrize("cap", [512, 24576], ids=["lds_maps", "global_maps"])
def test_gpu_ba_used_context(cap):
    assert bc.global_maps(4, cap) == (cap == 24576)  # (2 (4 - 1) + 1) 24576 B = 172032 B > 159744 B
    cfg = dict(ba_window=4, ba_max_landmarks=4096, ba_max_obs=32768, nlevels=8, kp_capacity=cap)
    big = ba_synth.clean_problem(n=8, n_pts=400, seed=61, drop=0.05, cap=cap)
    small = ba_synth.clean_problem(n=6, n_pts=120, seed=62, drop=0.05, cap=cap)
    for f in range(3):
        ba_synth.invalidate_stereo(small, f)
    big_call = dict(first_end=2, n_windows=6, first_valid=0, iterations=6, scale_factor=1.2)
    small_call = dict(first_end=3, n_windows=3, first_valid=0, iterations=6, scale_factor=1.2)
    ctx = _context(cfg, 6)
    used_big = _windows(ctx, _device(big), big, big_call)
    used_small = _windows(ctx, _device(small), small, small_call)
    fresh_small = _fresh(small, cfg, small_call, max_batch=6)
    assert fresh_small["stats"][0][2] == 0 and fresh_small["stats"][0][4] == 4  # a live window with L = 0
    assert np.array_equal(fresh_small["T"][0], small["T_rel"][2]) and len(fresh_small["lms"][0]) == 0
    assert fresh_small["stats"][1][2] > 0 and used_big["stats"][:, 2].min() > fresh_small["stats"][:, 2].max()
    _assert_bitwise(used_small, fresh_small)
