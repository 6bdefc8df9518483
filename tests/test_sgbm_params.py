"""GPU parity of SGBM over every accepted parameter: min_disparity of either sign, P1 / P2,
disp12_max_diff, pre_filter_cap and sgbm_stripes, one at a time and combined, bit-exact
against the oracle at small ragged shapes, under the classic cost-pass shapes and the L-path
schedule; degenerate inputs (constant, checkerboard, periodic, ramp, noise against constant)
at the defaults; and inputs whose aggregated cost passes 32767 (the oracle's S saturates in
int16, the kernel's is an unsaturated u16).  Cases and inputs: tests/sgbm_cases.py; their
guards also run without a GPU in tests/test_sgbm_cases_cpu.py.
"""
import numpy as np
import pytest
import torch

import sgbm_cases as sc
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

# fvo_config schedule fields: classic default, classic (lanes, cols) = (4, 64) and (16, 32), L path
SCHEDULES = {
    "classic": {},
    "classic4x64": dict(sgbm_lanes=4, sgbm_cols=64),
    "classic16x32": dict(sgbm_lanes=16, sgbm_cols=32),
    "lpath": dict(sgbm_mode=1),
}


def _ids(v):
    return sc.case_id(v) if isinstance(v, dict) else str(v)


def _sgbm_ctl(ctx):
    """SGBM control words (debug buffer 9): [2] = L-path hand-off timeouts."""
    return ctx.debug_buffer(9).view(torch.int32).numpy()


def _run(W, H, D, sched, L, R, **cfg):
    """fvo_sgbm on a batch of pairs under a schedule -> int16 [B,H,W]; under the L path also
    asserts that no hand-off timed out and every status is SGBM_OK."""
    from forest_slam_amd import _lib
    B = len(L)
    ctx = _lib.Context(W, H, max_batch=B, num_disparities=D, stages=_lib.STAGE_SGBM, **SCHEDULES[sched], **cfg)
    st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    # (copies: the shared inputs are read-only arrays)
    d = ctx.sgbm(torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda(), status=st)
    torch.cuda.synchronize()
    assert st.tolist() == [_lib.SGBM_OK] * B
    if sched == "lpath":
        assert _sgbm_ctl(ctx)[2] == 0
    out = d.cpu().numpy()
    ctx.close()
    return out


def _assert_equal(got, want, what):
    for i in range(len(want)):
        bad = np.argwhere(got[i] != want[i])
        assert len(bad) == 0, f"{what} image {i}: {len(bad)} px differ, first {bad[:5].tolist()}"


def _param_cases():
    """(sched, W, H, D, case): the whole list at the first shape under every schedule, the
    reduced list at the other shapes under classic default and the L path."""
    out = []
    for i, (W, H, D) in enumerate(sc.SHAPES):
        for sched in (SCHEDULES if i == 0 else ("classic", "lpath")):
            for c in (sc.full_cases(D) if i == 0 else sc.reduced_cases(D)):
                out.append((sched, W, H, D, c))
    return out


@pytest.mark.parametrize("sched,W,H,D,case", _param_cases(), ids=_ids)
def test_sgbm_parameter_bit_exact(oracle_mod, sched, W, H, D, case):
    # guard: the oracle's output moves with the parameter, so a kernel ignoring it cannot pass
    assert sc.moved_pixels(oracle_mod, W, H, D, case) > 0
    L, R = sc.pair_batch(W, H)
    got = _run(W, H, D, sched, L, R, **case)
    _assert_equal(got, sc.reference(oracle_mod, W, H, D, case), f"{W}x{H}/{D} {sched} {sc.case_id(case)}")
    if "min_disparity" in case:  # columns outside [minX1, maxX1) are invalid: (minD - 1) * 16
        minD = case["min_disparity"]
        inv = (minD - 1) * 16
        assert (got[:, :, :max(minD + D, 0)] == inv).all() and (got[:, :, W + min(minD, 0):] == inv).all()


@pytest.mark.parametrize("sched", ["classic", "lpath"])
def test_sgbm_defaults_bit_exact_at_the_case_shapes(oracle_mod, sched):
    """The control of the parameter cases: the same inputs at the defaults."""
    for W, H, D in sc.SHAPES:
        L, R = sc.pair_batch(W, H)
        _assert_equal(_run(W, H, D, sched, L, R), sc.reference(oracle_mod, W, H, D, {}), f"{W}x{H}/{D} {sched}")


@pytest.mark.parametrize("sched", ["classic", "lpath"])
def test_sgbm_minimum_height(oracle_mod, sched):
    """An SGBM-only context takes images from 64x32 (the 64-row minimum is ORB's): 31 rows are
    refused at creation, 32 rows (stripes of 8 rows, 5 overlap rows) are bit-exact."""
    from forest_slam_amd import _lib
    W, H, D = 160, 32, 64
    with pytest.raises(RuntimeError, match="fvo_create"):
        _lib.Context(W, H - 1, num_disparities=D, stages=_lib.STAGE_SGBM)
    with pytest.raises(RuntimeError, match="fvo_create"):
        _lib.Context(W, H, num_disparities=D, stages=_lib.STAGE_SGBM | _lib.STAGE_ORB)
    L, R = sc.pair_batch(W, H)
    _assert_equal(_run(W, H, D, sched, L, R), sc.reference(oracle_mod, W, H, D, {}), f"{W}x{H}/{D} {sched}")


@pytest.fixture(scope="module")
def degenerate_ref(oracle_mod):
    D = sc.DEGENERATE_SHAPE[2]
    return {k: oracle_mod.sgbm(L, R, num_disp=D) for k, (L, R) in sc.degenerate_inputs().items()}


@pytest.mark.parametrize("sched", ["classic", "lpath"])
def test_sgbm_degenerate_inputs_bit_exact(degenerate_ref, sched):
    """Constant, checkerboard against its shift, period-8 stripes, ramp against ramp + 5, noise
    against constant: cost ties across d decide the WTA and max(denom, 1) the sub-pixel step."""
    W, H, D = sc.DEGENERATE_SHAPE
    inp = sc.degenerate_inputs()
    names = sorted(inp)
    got = _run(W, H, D, sched, np.stack([inp[k][0] for k in names]), np.stack([inp[k][1] for k in names]))
    for i, k in enumerate(names):
        _assert_equal(got[i:i + 1], degenerate_ref[k][None], f"{k} {sched}")


@pytest.mark.parametrize("sched", ["classic", "lpath"])
@pytest.mark.parametrize("P2", sc.SATURATED_P2)
def test_sgbm_saturated_aggregate_bit_exact(oracle_mod, sched, P2):
    """S = L + R + V above 32767: the oracle (as OpenCV) saturates it in int16, the kernel sums
    an unsaturated u16.  Bit-equal as long as no clipped entry is the winner or its neighbour;
    the oracle's clip counter shows the inputs do clip."""
    W, H, D = sc.SATURATED_SHAPE
    inp = sc.saturated_inputs()
    names = sorted(inp)
    refs = [sc.saturated_reference(oracle_mod, k, P2) for k in names]
    for k, (_, nclip) in zip(names, refs):
        assert nclip > 0, f"{k} P2={P2}: the oracle never clipped"
    got = _run(W, H, D, sched, np.stack([inp[k][0] for k in names]), np.stack([inp[k][1] for k in names]), P2=P2)
    for i, k in enumerate(names):
        _assert_equal(got[i:i + 1], refs[i][0][None], f"{k} P2={P2} {sched}")


def test_cv2_shim_forwards_sgbm_parameters(oracle_mod):
    """cv2_compat.StereoSGBM_create forwards minDisparity, disp12MaxDiff and preFilterCap:
    compute() equals the oracle and invalid pixels read (16 - 1) * 16."""
    from forest_slam_amd import cv2_compat as cv2
    W, H, D = sc.SHAPES[0]
    L, R = sc.pair_batch(W, H)
    m = cv2.StereoSGBM_create(minDisparity=16, numDisparities=64, blockSize=7, P1=8 * 49, P2=32 * 49, disp12MaxDiff=2,
                              preFilterCap=31, mode=cv2.STEREO_SGBM_MODE_SGBM_3WAY)
    case = dict(min_disparity=16, P1=8 * 49, P2=32 * 49, disp12_max_diff=2, pre_filter_cap=31)
    want = sc.reference(oracle_mod, W, H, D, case)
    assert (want[0] != sc.reference(oracle_mod, W, H, D, dict(min_disparity=16))[0]).any()
    for i in range(2):
        got = m.compute(L[i].copy(), R[i].copy())
        assert got.dtype == np.int16 and np.array_equal(got, want[i])
        assert (got[:, :16 + D] == (16 - 1) * 16).all() and ((got < 16 * 16) == (got == (16 - 1) * 16)).all()
