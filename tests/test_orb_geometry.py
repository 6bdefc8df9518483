"""ORB at ragged geometries and non-default FAST thresholds, bit-exact against the oracle:
keypoints [:, :6], descriptors and counts at odd widths and heights, pyramids whose upper levels
are narrower than 2 * edgeThreshold (no keypoint can lie there), levels with fewer candidates
than their quota, n < nfeatures, and images without a single corner (count 0), alone and
beside textured images in one batch.
"""
import numpy as np
import pytest
import torch

from conftest import gpu_available

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")

SIZES = [(333, 217), (211, 173), (97, 83), (76, 70), (500, 77), (1003, 131)]
EDGE = 31  # fvo_config.edge_threshold default


def _images(W, H):
    """(synthetic forest frame (seed 4), uniform noise, constant 77) at W x H."""
    from forest_slam_amd import synth
    s = synth.StereoSequence(seed=4, n_frames=1, W=W, H=H, device="cpu").frame(0)[0].numpy()
    n = np.random.default_rng(W * 1000 + H).integers(0, 256, (H, W), dtype=np.uint8)
    return [s, n, np.full((H, W), 77, np.uint8)]


_ref_cache = {}


def _reference(oracle_mod, W, H, nfeatures):
    """[(kp, desc)] of _images(W, H) from the oracle (computed once)."""
    if (W, H, nfeatures) not in _ref_cache:
        _ref_cache[(W, H, nfeatures)] = [oracle_mod.orb_detect_compute(im, nfeatures) for im in _images(W, H)]
    return _ref_cache[(W, H, nfeatures)]


def test_oracle_counts_cover_the_edge_cases(oracle_mod):
    """The sizes reach what they were chosen for (checked without a GPU): populated octaves stop
    where a level gets narrower than 2 * edgeThreshold, n < nfeatures, and a count of zero."""
    want = {(333, 217): (451, 6), (211, 173): (372, 5), (500, 77): (152, 1), (1003, 131): (353, 4)}
    for W, H in SIZES:
        (skp, _), (nkp, _), (ckp, _) = _reference(oracle_mod, W, H, 500)
        assert len(ckp) == 0
        assert 0 < len(skp) < 500 and 0 < len(nkp) < 500
        # the highest level still wider and taller than 2 * edgeThreshold (scale 1.2 per level)
        top = max(l for l in range(8) if min(round(W / 1.2 ** l), round(H / 1.2 ** l)) > 2 * EDGE)
        assert top < 7
        assert int(nkp[:, 5].max()) == top
        if (W, H) in want:
            assert (len(skp), int(skp[:, 5].max())) == want[(W, H)]
    # 50 features: at the large sizes every level has more candidates than its quota, at the
    # small ones fewer
    assert len(_reference(oracle_mod, 76, 70, 50)[1][0]) < 50 < len(_reference(oracle_mod, 333, 217, 500)[1][0])


def _orb_gpu(ctx, imgs):
    kp, desc, cnt = ctx.orb(torch.from_numpy(np.stack(imgs)).cuda())
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    return [(kp[i, :cnt[i]].cpu().numpy(), desc[i, :cnt[i]].cpu().numpy()) for i in range(len(imgs))], cnt


def _assert_orb_equal(got, ref, what):
    for i, ((kp, desc), (rkp, rdesc)) in enumerate(zip(got, ref)):
        assert kp.shape[0] == rkp.shape[0], f"{what} image {i}: {kp.shape[0]} keypoints, oracle {rkp.shape[0]}"
        assert np.array_equal(kp[:, :6], rkp), f"{what} image {i}: rows {np.argwhere(kp[:, :6] != rkp)[:5].tolist()}"
        assert np.array_equal(desc, rdesc), f"{what} image {i}: descriptors differ"


@gpu
@needs_gpu
@pytest.mark.parametrize("nfeatures", [50, 500])
@pytest.mark.parametrize("W,H", SIZES)
def test_orb_ragged_geometry_bit_exact(oracle_mod, W, H, nfeatures):
    from forest_slam_amd import _lib
    ref = _reference(oracle_mod, W, H, nfeatures)
    ctx = _lib.Context(W, H, max_batch=3, nfeatures=nfeatures, stages=_lib.STAGE_ORB)
    got, cnt = _orb_gpu(ctx, _images(W, H))
    assert cnt.tolist() == [len(r[0]) for r in ref] and cnt[2] == 0
    _assert_orb_equal(got, ref, f"{W}x{H} nfeatures={nfeatures}")


@gpu
@needs_gpu
def test_orb_mixed_batch_zero_counts_beside_textured(oracle_mod):
    """constant, textured, constant through one call: counts 0, n, 0, and the textured image's
    keypoints are the ones it has alone."""
    from forest_slam_amd import _lib
    W, H = 333, 217
    s, _, c = _images(W, H)
    ref = _reference(oracle_mod, W, H, 500)
    ctx = _lib.Context(W, H, max_batch=3, nfeatures=500, stages=_lib.STAGE_ORB)
    got, cnt = _orb_gpu(ctx, [c, s, c])
    assert cnt.tolist() == [0, len(ref[0][0]), 0] and cnt[1] > 0
    _assert_orb_equal(got, [ref[2], ref[0], ref[2]], "mixed batch")


@gpu
@needs_gpu
@pytest.mark.parametrize("W,H", [(333, 217), (960, 600)])
@pytest.mark.parametrize("thr", [5, 60])
def test_orb_fast_threshold_bit_exact(oracle_mod, thr, W, H):
    from forest_slam_amd import _lib, synth
    img = synth.StereoSequence(seed=4, n_frames=1, W=W, H=H, device="cpu").frame(0)[0].numpy()
    ref = oracle_mod.orb_detect_compute(img, 500, fast_threshold=thr)
    dflt = oracle_mod.orb_detect_compute(img, 500)
    # the threshold matters on this image: a kernel ignoring it cannot pass
    assert len(ref[0]) != len(dflt[0]) or not np.array_equal(ref[0], dflt[0])
    ctx = _lib.Context(W, H, max_batch=1, nfeatures=500, fast_threshold=thr, stages=_lib.STAGE_ORB)
    got, _ = _orb_gpu(ctx, [img])
    _assert_orb_equal(got, [ref], f"{W}x{H} fast_threshold={thr}")


@gpu
@needs_gpu
def test_orb_intermediates_bit_exact_at_ragged_size(oracle_mod):
    """Pyramid, blurred pyramid and FAST score map at 333x217 (every level of odd size, the top
    ones narrower than 2 * edgeThreshold) through debug_buffer(0 / 1 / 2)."""
    from forest_slam_amd import _lib
    W, H = 333, 217
    img = _images(W, H)[0]
    ctx = _lib.Context(W, H, max_batch=1, nfeatures=500, stages=_lib.STAGE_ORB)
    _orb_gpu(ctx, [img])
    geo, total = ctx.geometry()
    ref_levels = oracle_mod.orb_pyramid(img, 8)
    pyr = ctx.debug_buffer(0).numpy()[:total]
    for (w, h, off), ref in zip(geo, ref_levels):
        got = pyr[off:off + w * h].reshape(h, w)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), f"pyramid level {w}x{h} differs at {np.argwhere(got != ref)[:5].tolist()}"
    score = ctx.debug_buffer(2).numpy()[:total]
    for (w, h, off), lvl in zip(geo, ref_levels):
        ref = oracle_mod.fast_score_map(lvl, 20)
        got = score[off:off + w * h].reshape(h, w)
        assert np.array_equal(got, ref), f"FAST score {w}x{h}: {np.argwhere(got != ref)[:5].tolist()}"
    blur = ctx.debug_buffer(1).numpy()[:total]
    for (w, h, off), ref in zip(geo, oracle_mod.orb_pyramid(img, 8, blurred=True)):
        assert np.array_equal(blur[off:off + w * h].reshape(h, w), ref), f"blurred level {w}x{h} differs"
