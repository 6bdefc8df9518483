"""The ordered compaction of csrc/fvo_device.h (block_rank) through fvo_backproject: which matches
are kept is decided by the disparity pixel under the match's keypoint, so every keep / drop
pattern over the 256-thread passes, the waves of a pass and the lanes of a wave can be dialled in.
Expected points3d, points2d and n_points come from oracle.backproject on the CPU, bit for bit.
The CPU twin asserts that the oracle keeps exactly the matches each pattern means to keep, so the
GPU test cannot pass vacuously."""
import numpy as np
import pytest

import dense_ref as dr
from conftest import gpu_available

W, H, CAP = 40, 24, 600
KEPT, DROPPED = 3 * 16, 0  # d = 3: Z = 54; d = 0 -> 0.1: Z = 1631 > 1000
N_MATCHES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 513]  # around a wave, one pass, two passes
PATTERNS = {
    "all": lambda i, n: np.ones_like(i, bool),
    "none": lambda i, n: np.zeros_like(i, bool),
    "every_other": lambda i, n: i % 2 == 0,
    "first_only": lambda i, n: i == 0,
    "last_only": lambda i, n: i == n - 1,
    "wave1_dropped": lambda i, n: (i % 256) // 64 != 1,  # lanes 64-127 of every pass
}
# the kept count each pattern means, without evaluating its flags
INTENDED = {
    "all": lambda n: n,
    "none": lambda n: 0,
    "every_other": lambda n: (n + 1) // 2,
    "first_only": lambda n: min(n, 1),
    "last_only": lambda n: min(n, 1),
    "wave1_dropped": lambda n: n - sum(min(max(n - p - 64, 0), 64) for p in range(0, n, 256)),
}
SENTINEL = -7.25


def _image():
    img = np.full((H, W), DROPPED, np.int16)
    img[:, :W // 2] = KEPT  # the left half is kept
    return img


def _case(pattern, n):
    """(kp0, kp1, matches, flags) of one frame: match i joins keypoint perm0[i] of kp0, which lies
    on a pixel of the kind flags[i] asks for (fractional, all different), and perm1[i] of kp1."""
    rng = np.random.default_rng(1000 * list(PATTERNS).index(pattern) + n)
    i = np.arange(n)
    flags = PATTERNS[pattern](i, n)
    perm0, perm1 = rng.permutation(CAP)[:n], rng.permutation(CAP)[:n]
    kp0 = np.zeros((CAP, 8), np.float32)
    kp1 = np.zeros((CAP, 8), np.float32)
    kp0[perm0, 0] = (i // H) % (W // 2) + np.where(flags, 0, W // 2) + 0.25 + 0.5 * (i // (H * W // 2))
    kp0[perm0, 1] = i % H + 0.125 * (i % 7)
    kp1[:, 0], kp1[:, 1] = np.arange(CAP) + 0.5, rng.uniform(0, H, CAP)
    m = np.full((CAP, 3), -1, np.int32)
    m[:n, 0], m[:n, 1], m[:n, 2] = perm0, perm1, rng.integers(0, 256, n)
    return kp0, kp1, m, flags


def _expected(oracle_mod, pattern, n):
    kp0, kp1, m, flags = _case(pattern, n)
    P, p2, valid = oracle_mod.backproject(oracle_mod.disparity_map(_image()), kp0[m[:n, 0], :2], kp1[m[:n, 1], :2],
                                          dr.HAND_K, dr.HAND_BASELINE)
    return P.reshape(-1, 3), p2.reshape(-1, 2), valid, flags


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_oracle_keeps_the_intended_matches(oracle_mod, pattern):
    for n in N_MATCHES:
        P, p2, valid, flags = _expected(oracle_mod, pattern, n)
        assert np.array_equal(valid, flags)
        assert len(P) == len(p2) == int(flags.sum()) == INTENDED[pattern](n)
        assert len(np.unique(P, axis=0)) == len(P)  # a wrong order or a repeated row would show


@pytest.fixture(scope="module")
def ctx():
    from forest_slam_amd import _lib
    return _lib.Context(W, H, max_batch=len(N_MATCHES), stages=_lib.STAGE_POSE, kp_capacity=CAP)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_backproject_compaction(ctx, oracle_mod, pattern):
    import torch
    B = len(N_MATCHES)
    cases = [_case(pattern, n) for n in N_MATCHES]
    kp0, kp1, m = (torch.from_numpy(np.stack([c[k] for c in cases])).cuda() for k in range(3))
    disp = torch.from_numpy(np.repeat(_image()[None], B, axis=0)).cuda()
    nm = torch.tensor(N_MATCHES, dtype=torch.int32, device="cuda")
    out = (torch.full((B, CAP, 3), SENTINEL, dtype=torch.float32, device="cuda"),
           torch.full((B, CAP, 2), SENTINEL, dtype=torch.float32, device="cuda"),
           torch.full((B,), -1, dtype=torch.int32, device="cuda"))
    P3, p2, npts = (t.cpu().numpy() for t in ctx.backproject(disp, kp0, kp1, m, nm, dr.HAND_K, dr.HAND_BASELINE,
                                                             out=out))
    for b, n in enumerate(N_MATCHES):
        P_ref, p2_ref, _, _ = _expected(oracle_mod, pattern, n)
        k = len(P_ref)
        print(f"compaction {pattern}: n_matches {n}: {npts[b]} points, expected {k}")
        assert npts[b] == k
        assert np.array_equal(P3[b, :k].view(np.uint32), P_ref.view(np.uint32))
        assert np.array_equal(p2[b, :k].view(np.uint32), p2_ref.view(np.uint32))
        assert (P3[b, k:] == SENTINEL).all() and (p2[b, k:] == SENTINEL).all()
