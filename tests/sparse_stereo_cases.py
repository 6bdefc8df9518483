"""Hand-built inputs of the sparse-stereo tests (CPU: against known answers; GPU: bit-exact against
tests/sparse_stereo_ref.py).  Every case is a dict of one pair's inputs: imgL, imgR u8 [H,W], kpL,
kpR f32 [n,8], descL, descR u8 [n,32]; the boundary cases add `expect`, rows of (left index,
status, right index, hamming, k*) with None for "whatever the rule gives"."""
import functools

import numpy as np

import sparse_stereo_ref as ref

W, H = 96, 64
f32 = np.float32
# the boundary cases' call: a disparity range that a 96-px image holds, and fx * baseline = 1, so
# that Z = 1 / d crosses the 0.1 gate inside the range
BOUNDARY_PARAMS = dict(min_disparity=1.0, max_disparity=12.0)
BOUNDARY_K = np.array([[10.0, 0, 48.0], [0, 10.0, 32.0], [0, 0, 1]])
BOUNDARY_BASELINE = 0.1
# the random sets' call (their images carry disparity 7): the refined d = 7 - delta crosses
# max_disparity, and Z = 0.7 / d crosses the 0.1 gate
SET_PARAMS = dict(min_disparity=1.0, max_disparity=7.3)
SET_K = np.array([[100.0, 0, 47.5], [0, 101.0, 31.5], [0, 0, 1]])
SET_BASELINE = 0.007


def noise_pair(shift, seed):
    """Noise images with R(y, x) = L(y, x + shift): every left pixel's disparity is `shift`."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R[:, :W - shift] = L[:, shift:]
    return L, R


def kp_rows(rows):
    """(x, y, octave) triples -> keypoint records (size, angle, response and class_id arbitrary)."""
    kp = np.zeros((len(rows), 8), f32)
    for i, (x, y, o) in enumerate(rows):
        kp[i] = (x, y, 31.0, 10.0 * i, 0.01, o, -1.0, 0.0)
    return kp


def flip_bits(d, n, seed=0):
    """d with n distinct bits flipped."""
    bits = np.unpackbits(d)
    bits[np.random.default_rng(seed).choice(256, n, replace=False)] ^= 1
    return np.packbits(bits)


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """name -> case.  The images carry disparity 6 unless a case says otherwise, so a right
    keypoint at xL - 6 refines to k* = 0 with SAD(0) = 0."""
    D = np.random.default_rng(5).integers(0, 256, 32, dtype=np.uint8)
    up = lambda v: np.nextafter(f32(v), f32(np.inf))  # noqa: E731
    down = lambda v: np.nextafter(f32(v), f32(-np.inf))  # noqa: E731
    cases = {}

    def add(name, left, right, expect, shift=6, descL=None, descR=None, images=None):
        L, R = images if images is not None else noise_pair(shift, 11)
        cases[name] = dict(imgL=L, imgR=R, kpL=kp_rows(left), kpR=kp_rows(right),
                           descL=np.array(descL if descL is not None else [D] * len(left), np.uint8).reshape(-1, 32),
                           descR=np.array(descR if descR is not None else [D] * len(right), np.uint8).reshape(-1, 32),
                           expect=expect)

    add("plain", [(50, 30, 0)], [(44, 30, 0)], [(0, 0, 0, 0, 0)])
    add("fractional", [(50.3, 30.4, 0)], [(44.2, 29.8, 0)], [(0, 0, 0, 0, 0)])
    # the row band: octave 0, row_tol 2 -> |dy| <= 2 exactly
    add("band_equal", [(50, 30, 0)], [(44, 32, 0)], [(0, 0, 0, 0, 0)])
    add("band_one_ulp_above", [(50, 30, 0)], [(44, up(32), 0)], [(0, 1, -1, -1, 0)])
    add("band_equal_below", [(50, 30, 0)], [(44, 28, 0)], [(0, 0, 0, 0, 0)])
    add("band_one_ulp_below", [(50, 30, 0)], [(44, down(28), 0)], [(0, 1, -1, -1, 0)])
    # the band scales with the LEFT octave: level 2 of 1.2 -> 2 * float32(1.44) = 2.88
    add("band_left_octave", [(50, 30, 2), (50, 30, 0)], [(44, 32.5, 1)], [(0, 0, 0, 0, 0), (1, 1, -1, -1, 0)])
    # the disparity range on d0 = xL - xR; at d0 = min the true match is 5 px away: k* = -S
    add("d0_equal_min", [(50, 30, 0)], [(49, 30, 0)], [(0, 4, 0, 0, -5)])
    add("d0_below_min", [(50, 30, 0)], [(up(49), 30, 0)], [(0, 1, -1, -1, 0)])
    add("d0_equal_max", [(50, 30, 0)], [(38, 30, 0)], [(0, None, 0, 0, None)], shift=12)
    add("d0_above_max", [(50, 30, 0)], [(down(38), 30, 0)], [(0, 1, -1, -1, 0)], shift=12)
    add("slide_end_plus", [(50, 30, 0)], [(39, 30, 0)], [(0, 4, 0, 0, 5)])
    add("slide_inside", [(50, 30, 0)], [(40, 30, 0), ], [(0, 0, 0, 0, 4)])
    # octaves
    add("octave_diff_1", [(50, 30, 2)], [(44, 30, 3)], [(0, 0, 0, 0, 0)])
    add("octave_diff_2", [(50, 30, 2)], [(44, 30, 4)], [(0, 1, -1, -1, 0)])
    add("octave_not_integer", [(50, 30, 2.5), (50, 30, 1)], [(44, 30, 1.5)], [(0, 1, -1, -1, 0), (1, 1, -1, -1, 0)])
    add("octave_out_of_range", [(50, 30, 8), (50, 30, -1), (50, 30, 7)], [(44, 30, 8), (44, 30, 7)],
        [(0, 1, -1, -1, 0), (1, 1, -1, -1, 0), (2, 0, 1, 0, 0)])
    add("not_finite", [(np.nan, 30, 0), (50, np.inf, 0), (50, 30, np.nan), (50, 30, 0)],
        [(np.nan, 30, 0), (44, -np.inf, 0), (44, 30, 0)],
        [(0, 1, -1, -1, 0), (1, 1, -1, -1, 0), (2, 1, -1, -1, 0), (3, 0, 2, 0, 0)])
    # coordinates no int holds: refused by the float32 bounds before any conversion
    add("huge", [(3e30, 30, 0), (16777226.0, 30, 0)], [(3e30, 30, 0), (16777220.0, 30, 0)],
        [(0, 1, -1, -1, 0), (1, 3, 1, 0, 0)])
    # hamming
    add("hamming_75", [(50, 30, 0)], [(44, 30, 0)], [(0, 0, 0, 75, 0)], descR=[flip_bits(D, 75)])
    add("hamming_76", [(50, 30, 0)], [(44, 30, 0)], [(0, 1, -1, -1, 0)], descR=[flip_bits(D, 76)])
    # a nearer descriptor outside the band does not count; the farther candidate is taken
    add("nearest_is_no_candidate", [(50, 30, 0)], [(44, 40, 0), (44, 30, 0)], [(0, 0, 1, 9, 0)],
        descR=[D, flip_bits(D, 9)])
    # two candidates at the same distance: the lower right index (1 px off the true match: k* = -1)
    add("equal_candidates", [(50, 30, 0)], [(45, 30, 0), (44, 30, 0)], [(0, 0, 0, 0, -1)])
    # two left keypoints contest one right keypoint at the same distance: the lower left index
    add("contest_equal", [(50, 30, 0), (51, 30, 0)], [(44, 30, 0)], [(0, 0, 0, 0, 0), (1, 2, 0, 0, 0)])
    add("contest_nearer_wins", [(50, 30, 0), (51, 30, 0)], [(45, 30, 0)], [(0, 2, 0, 3, 0), (1, 0, 0, 0, 0)],
        descL=[flip_bits(D, 3), D])
    # the winner fails the refinement (its window crosses the top) and does not hand the keypoint on
    add("contest_winner_fails", [(50, 4, 0), (50, 5, 0)], [(44, 5, 0)], [(0, 3, 0, 0, 0), (1, 2, 0, 1, 0)],
        descL=[D, flip_bits(D, 1)])
    # a loser does not fall back to its second candidate
    add("contest_no_second_choice", [(50, 30, 0), (50, 30, 0)], [(44, 30, 0), (44, 30, 0)],
        [(0, 0, 0, 0, 0), (1, 2, 0, 0, 0)])
    # the windows at the image sides: touching is refined, crossing is status 3
    add("left_touch", [(16, 30, 0)], [(10, 30, 0)], [(0, 0, 0, 0, 0)])
    add("left_cross", [(15, 30, 0)], [(9, 30, 0)], [(0, 3, 0, 0, 0)])
    add("right_touch", [(90, 30, 0)], [(84, 30, 0)], [(0, 0, 0, 0, 0)])
    add("right_cross", [(91, 30, 0)], [(85, 30, 0)], [(0, 3, 0, 0, 0)])
    add("right_strip_cross", [(88, 30, 0)], [(86, 30, 0)], [(0, 3, 0, 0, 0)])
    add("top_touch", [(50, 5, 0)], [(44, 5, 0)], [(0, 0, 0, 0, 0)])
    add("top_cross", [(50, 4, 0)], [(44, 4, 0)], [(0, 3, 0, 0, 0)])
    add("bottom_touch", [(50, 58, 0)], [(44, 58, 0)], [(0, 0, 0, 0, 0)])
    add("bottom_cross", [(50, 59, 0)], [(44, 59, 0)], [(0, 3, 0, 0, 0)])
    # floorf(x + 0.5): 15.5 rounds to 16 (touching), 15.49 to 15 (crossing)
    add("round_half_up", [(15.5, 30, 0)], [(9.5, 30, 0)], [(0, 0, 0, 0, 0)])
    add("round_down", [(15.49, 30, 0)], [(9.49, 30, 0)], [(0, 3, 0, 0, 0)])
    # the refined disparity leaves the range (true disparity 13 > 12; d0 = 9 is inside)
    add("refined_above_max", [(50, 30, 0)], [(41, 30, 0)], [(0, 5, 0, 0, -4)], shift=13)
    # Z = 1 / d: d ~ 11 gives Z ~ 0.09 <= 0.1
    add("depth_gate", [(50, 30, 0)], [(39, 30, 0)], [(0, 6, 0, 0, 0)], shift=11)
    # a SAD tie: the right image has period 3 in x and the left window equals it, so SAD(k) = 0
    # at k = -3, 0, 3; the smallest k wins
    P = np.random.default_rng(3).integers(0, 256, (H, 3), dtype=np.uint8)
    per = np.tile(P, (1, W // 3))
    add("sad_tie", [(50, 30, 0)], [(44, 30, 0)], [(0, 0, 0, 0, -3)], images=(per, per))
    # no right keypoints, no left keypoints
    add("no_right", [(50, 30, 0)], [], [(0, 1, -1, -1, 0)], descR=np.zeros((0, 32), np.uint8))
    add("no_left", [], [(44, 30, 0)], [], descL=np.zeros((0, 32), np.uint8))
    for c in cases.values():
        assert c["descL"].dtype == np.uint8 and c["descR"].dtype == np.uint8
    return cases


@functools.lru_cache(maxsize=None)
def random_set(nL, nR, seed, shift=7):
    """A dense set on a 96x64 pair of disparity `shift`: a third of the left keypoints are
    near-copies of other left keypoints; two thirds of the right keypoints are twins of left keypoints
    (position - shift with a jitter that for every fourth reaches past the slide, the descriptor
    with 0..89 flipped bits, the octave moved by up to 2), the rest random; the right order is
    shuffled.  Positions cover the
    whole image, so many windows cross its sides, and the row bands of 2..7 px over 64 rows give
    every left keypoint several candidates and many right keypoints several suitors."""
    rng = np.random.default_rng(seed)
    L, R = noise_pair(shift, seed + 1000)
    kpL = np.zeros((nL, 8), f32)
    kpL[:, 0] = rng.uniform(0, W, nL)
    kpL[:, 1] = rng.uniform(0, H, nL)
    kpL[:, 2:5] = rng.uniform(0, 100, (nL, 3))
    kpL[:, 5] = rng.integers(0, 8, nL)
    kpL[:, 6] = -1
    descL = rng.integers(0, 256, (nL, 32), dtype=np.uint8)
    for i in range(nL // 3):  # near-copies of other left keypoints: suitors of the same right keypoint
        src = nL // 3 + int(rng.integers(0, nL - nL // 3))
        kpL[i, :2] = kpL[src, :2] + rng.uniform(-1, 1, 2)
        kpL[i, 5] = kpL[src, 5]
        descL[i] = flip_bits(descL[src], int(rng.integers(0, 10)), seed=int(rng.integers(1 << 30)))
    kpR = np.zeros((nR, 8), f32)
    kpR[:, 0] = rng.uniform(0, W, nR)
    kpR[:, 1] = rng.uniform(0, H, nR)
    kpR[:, 2:5] = rng.uniform(0, 100, (nR, 3))
    kpR[:, 5] = rng.integers(0, 8, nR)
    kpR[:, 6] = -1
    descR = rng.integers(0, 256, (nR, 32), dtype=np.uint8)
    ntwin = min(2 * nR // 3, nL)
    src = rng.permutation(nL)[:ntwin]
    for j, i in enumerate(src):
        kpR[j, 0] = kpL[i, 0] - shift + (rng.uniform(-1.5, 1.5) if j % 4 else rng.uniform(-6.5, 6.5))
        kpR[j, 1] = kpL[i, 1] + rng.uniform(-2.5, 2.5)
        kpR[j, 5] = np.clip(kpL[i, 5] + rng.integers(-2, 3), 0, 7)
        descR[j] = flip_bits(descL[i], int(rng.integers(0, 90)), seed=int(rng.integers(1 << 30)))
    if nR >= 8:  # exact duplicates: equal distances, the lower index must win
        descR[-4:] = descR[:4]
        kpR[-4:] = kpR[:4]
    perm = rng.permutation(nR)
    return dict(imgL=L, imgR=R, kpL=kpL, descL=descL, kpR=kpR[perm], descR=descR[perm])


def run_ref(case, K, baseline, **params):
    return ref.sparse_stereo(case["imgL"], case["imgR"], case["kpL"], case["descL"], case["kpR"], case["descR"], K,
                             baseline, ref.Params(**params))
