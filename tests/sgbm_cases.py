"""Inputs, parameter cases and cached oracle outputs shared by the SGBM parameter tests
(test_sgbm_params.py on the GPU, test_sgbm_cases_cpu.py without one).

Shapes are small and leave every partial unit: partial 16/32/64-column cost blocks, partial
8-column segments, partial 4-row blocks, stripes of unequal length.  Inputs come from seeds.
"""
import functools

import numpy as np

SHAPES = [(213, 75, 64), (261, 53, 96), (333, 41, 128)]  # (W, H, numDisparities)

# fvo_config names; the oracle's keyword names are in ORACLE_KW
DEFAULTS = dict(min_disparity=0, P1=392, P2=1568, disp12_max_diff=0, pre_filter_cap=0, sgbm_stripes=4)
ORACLE_KW = dict(min_disparity="min_disp", P1="P1", P2="P2", disp12_max_diff="disp12_max_diff",
                 pre_filter_cap="pre_filter_cap", sgbm_stripes="stripes")


def full_cases(D):
    """One parameter at a time, then all of them non-default; min_disparity -(D + 16) makes
    maxD <= 0 and therefore minX1 = 0."""
    cases = [dict(min_disparity=m) for m in (16, -16, 5, -7, -(D + 16))]
    cases += [dict(P1=a, P2=b) for a, b in ((8, 32), (100, 101), (392, 6000), (392, 17000))]
    cases += [dict(disp12_max_diff=v) for v in (2, 8)]
    cases += [dict(pre_filter_cap=v) for v in (31, 63)]
    cases += [dict(sgbm_stripes=v) for v in (1, 3, 5)]
    cases.append(dict(min_disparity=-7, P1=100, P2=6000, disp12_max_diff=2, pre_filter_cap=31, sgbm_stripes=3))
    return cases


def reduced_cases(D):
    return [dict(min_disparity=16), dict(min_disparity=-(D + 16)), dict(P1=8, P2=32), dict(disp12_max_diff=8),
            dict(pre_filter_cap=63), dict(sgbm_stripes=5)]


def case_id(case):
    return "-".join(f"{k}={v}" for k, v in case.items()) or "defaults"


def shape_cases():
    """(W, H, D, case) of every parity case: the whole list at the first shape, the reduced
    list at the other two."""
    out = []
    for i, (W, H, D) in enumerate(SHAPES):
        for c in (full_cases(D) if i == 0 else reduced_cases(D)):
            out.append((W, H, D, c))
    return out


@functools.lru_cache(maxsize=None)
def pair_batch(W, H):
    """The batch of 2 every parameter case runs: (a) the synthetic forest frame, (b) two
    independent uniform-noise images.  Returns read-only (L u8[2,H,W], R u8[2,H,W])."""
    from forest_slam_amd import synth
    La, Ra = (x.numpy() for x in synth.StereoSequence(seed=5, n_frames=1, W=W, H=H, device="cpu").frame(0))
    rng = np.random.default_rng(1000 * W + H)
    Lb = rng.integers(0, 256, (H, W), dtype=np.uint8)
    Rb = rng.integers(0, 256, (H, W), dtype=np.uint8)
    L, R = np.stack([La, Lb]), np.stack([Ra, Rb])
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


def _oracle_kw(case):
    return {ORACLE_KW[k]: v for k, v in case.items()}


_ref_cache = {}


def reference(oracle_mod, W, H, D, case):
    """Oracle disparities int16 [2,H,W] of pair_batch(W, H) under `case` (computed once)."""
    key = (W, H, D, tuple(sorted(case.items())))
    if key not in _ref_cache:
        L, R = pair_batch(W, H)
        out = np.stack([oracle_mod.sgbm(L[i], R[i], num_disp=D, **_oracle_kw(case)) for i in range(2)])
        out.setflags(write=False)
        _ref_cache[key] = out
    return _ref_cache[key]


def moved_pixels(oracle_mod, W, H, D, case):
    """Pixels of input (a) by which the oracle's output under `case` differs from its output
    with defaults: the vacuity guard (a kernel that ignores the parameter cannot pass)."""
    return int((reference(oracle_mod, W, H, D, case)[0] != reference(oracle_mod, W, H, D, {})[0]).sum())


# ---------------------------------------------------------------------------- degenerate inputs
DEGENERATE_SHAPE = (213, 75, 64)


def degenerate_inputs():
    """name -> (L, R) at DEGENERATE_SHAPE: inputs where first-minimum WTA ties and the
    sub-pixel max(denom, 1) decide the output."""
    W, H, _ = DEGENERATE_SHAPE
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(77)
    const = np.full((H, W), 128, np.uint8)
    checker = (((xx + yy) & 1) * 255).astype(np.uint8)
    stripes = np.where((xx % 8) < 4, 40, 200).astype(np.uint8)
    ramp = (xx % 251).astype(np.uint8)
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    return {
        "constant128": (const, const.copy()),
        "checkerboard_vs_shift1": (checker, np.roll(checker, -1, axis=1)),
        "stripes_period8": (stripes, stripes.copy()),
        "ramp_vs_ramp_plus5": (ramp, (ramp + 5).astype(np.uint8)),
        "noise_vs_constant": (noise, const.copy()),
    }


# ---------------------------------------------------------------------------- saturated aggregate
SATURATED_SHAPE = (208, 72, 64)
SATURATED_P2 = (12000, 17000)


def saturated_inputs():
    """name -> (L, R) at SATURATED_SHAPE whose aggregated cost S = L + R + V passes 32767 at
    large P2 (the oracle's S saturates in int16, the kernel's is an unsaturated u16): noise
    against itself shifted 9 px, and 8x8 blocks of random 0/255 against their 13 px shift."""
    W, H, _ = SATURATED_SHAPE
    rng = np.random.default_rng(4242)
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    blocks = (rng.integers(0, 2, ((H + 7) // 8, (W + 7) // 8)) * 255).astype(np.uint8)
    blocks = np.kron(blocks, np.ones((8, 8), np.uint8))[:H, :W]
    return {
        "noise_vs_shift9": (noise, np.roll(noise, -9, axis=1)),
        "blocks8_vs_shift13": (np.ascontiguousarray(blocks), np.roll(blocks, -13, axis=1)),
    }


_sat_cache = {}


def saturated_reference(oracle_mod, name, P2):
    """(oracle disparity, number of clipped S entries) of a saturated input at P2."""
    if (name, P2) not in _sat_cache:
        L, R = saturated_inputs()[name]
        _sat_cache[(name, P2)] = oracle_mod.sgbm(L, R, num_disp=SATURATED_SHAPE[2], P2=P2, clipped=True)
    return _sat_cache[(name, P2)]
