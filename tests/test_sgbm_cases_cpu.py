"""CPU checks of the SGBM parameter cases (no GPU): the oracle's new arguments default to what
it computed before, and the guards of tests/test_sgbm_params.py hold for the inputs chosen --
every parameter case moves the oracle's output on the synthetic frame, and the saturated
inputs do clip the oracle's 16-bit aggregate -- so a bad input choice is caught here.
"""
import numpy as np
import pytest

import sgbm_cases as sc


def test_oracle_sgbm_defaults_equal_explicit_values(oracle_mod):
    """disp12_max_diff=0 / pre_filter_cap=0 / stripes=4 (the defaults) are OpenCV's 1 / ftzero
    15 / 4 stripes: byte-identical output, median and raw, on two inputs."""
    for W, H, D in sc.SHAPES[:2]:
        L, R = sc.pair_batch(W, H)
        for i in range(2):
            d0, r0 = oracle_mod.sgbm(L[i], R[i], num_disp=D, raw=True)
            d1, r1 = oracle_mod.sgbm(L[i], R[i], num_disp=D, raw=True, disp12_max_diff=1, pre_filter_cap=15,
                                     stripes=4)
            assert d0.tobytes() == d1.tobytes() and r0.tobytes() == r1.tobytes(), (W, H, D, i)


@pytest.mark.parametrize("W,H,D,case", sc.shape_cases(), ids=lambda v: sc.case_id(v) if isinstance(v, dict) else str(v))
def test_parameter_case_moves_the_oracle(oracle_mod, W, H, D, case):
    n = sc.moved_pixels(oracle_mod, W, H, D, case)
    print(f"{W}x{H} D={D} {sc.case_id(case)}: {n} px differ from the defaults")
    assert n > 0


def test_min_disparity_cases_reach_minx1_zero():
    """-(D + 16) is the case with maxD <= 0: minX1 = 0 and width1 = W - D - 16 > 0."""
    for W, H, D in sc.SHAPES:
        minD = -(D + 16)
        assert minD + D <= 0 and W + minD > 0


@pytest.mark.parametrize("P2", sc.SATURATED_P2)
@pytest.mark.parametrize("name", sorted(sc.saturated_inputs()))
def test_saturated_inputs_clip_the_oracle(oracle_mod, name, P2):
    _, nclip = sc.saturated_reference(oracle_mod, name, P2)
    print(f"{name} P2={P2}: {nclip} aggregated costs clipped at 32767")
    assert nclip > 0


def test_default_parameters_do_not_clip(oracle_mod):
    """The clip counter is not vacuous: at the default P2 nothing saturates."""
    L, R = sc.saturated_inputs()["noise_vs_shift9"]
    _, nclip = oracle_mod.sgbm(L, R, num_disp=sc.SATURATED_SHAPE[2], clipped=True)
    assert nclip == 0
