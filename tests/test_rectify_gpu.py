"""Stereo rectification on the GPU: fvo_rectify_map, fvo_remap_u8 and fvo_rectify_gray bit for bit
against the specification tests/rectify_ref.py (both tile paths and their boundary, 1 and 3
channels, batches with gaps, padded and misaligned rows, maps pointing outside the image), the
fused ingest against map -> remap -> gray, and pipeline.run_stereo_bag(rectify=(R, T)) against the
oracle chain on a rendered two-topic bag."""
import os
import sys

import numpy as np
import pytest
import torch

import rectify_ref as ref
import rectify_scene as scene
from conftest import ROOT, gpu_available

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden_ingest import synthetic_bgr  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

W, H = scene.W, scene.H
D8 = np.array([-0.21, 0.09, 1.2e-3, -0.8e-3, -0.02, 0.11, -0.03, 0.004])


@pytest.fixture(scope="module")
def rect():
    from forest_slam_amd.rectify import stereo_rectify
    Kl, dl, Kr, dr, R, T = scene.rig()
    return stereo_rectify(Kl, dl, Kr, dr, (W, H), R, T)


@pytest.fixture(scope="module")
def ctx():
    from forest_slam_amd import _lib
    return _lib.Context(W, H, max_batch=3, stages=_lib.STAGE_BF, kp_capacity=64)


@pytest.fixture(scope="module")
def images():
    """u8 [3, H, W, 3]: two smooth synthetic images and one of noise."""
    imgs = np.stack([synthetic_bgr(H, W, s) for s in range(3)])
    imgs[2] = np.random.default_rng(9).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return imgs


def _small_ctx(w, h):
    from forest_slam_amd import _lib
    return _lib.Context(w, h, max_batch=3, stages=_lib.STAGE_BF, kp_capacity=64)


# ------------------------------------------------------------------ the map
def test_rectify_map_matches_spec(ctx, rect):
    Kl, dl, Kr, dr, _, _ = scene.rig()
    cases = [(Kl, dl, rect.R1, rect.P1[:, :3]), (Kr, dr, rect.R2, rect.P2[:, :3]),   # the x4 rig, both cameras
             (Kl, D8, scene.rodrigues(np.array([0.03, -0.05, 0.08])), Kr),           # rational model
             (Kl, dl[:4], None, None),                                               # 4 coefficients, R = I, newK = K
             scene.lens_case("rolled")]
    for K, d, R, newK in cases:
        m1, m2 = ctx.rectify_map(K, d, R, newK)
        w1, w2 = ref.rectify_map(K, d, R, newK, W, H)
        assert np.array_equal(m1.cpu().numpy(), w1) and np.array_equal(m2.cpu().numpy(), w2), len(d)


def test_rectify_map_97x64(rect):
    """A width that is no multiple of 4 and leaves the narrowest remainder of a tile."""
    w, h = 97, 64
    c = _small_ctx(w, h)
    Kl, dl, _, _, _, _ = scene.rig(4.0, 0.1)
    for K, d, R, newK in ((Kl, dl, rect.R1, None), (Kl, D8, scene.rotz(30.0), Kl)):
        m1, m2 = c.rectify_map(K, d, R, newK)
        w1, w2 = ref.rectify_map(K, d, R, newK, w, h)
        assert np.array_equal(m1.cpu().numpy(), w1) and np.array_equal(m2.cpu().numpy(), w2)


# ------------------------------------------------------------------ remap and the fused ingest
def _outside_map():
    """Taps partly outside on the left and at the bottom, a band wholly outside, int16 extremes."""
    y, x = np.mgrid[0:H, 0:W]
    m1 = np.stack([x - 200, y + 150], axis=-1).astype(np.int16)
    m1[40:60, :, 1] = -500                      # wholly outside
    m1[100:120, :, 0] = W - 1                   # the second x tap is outside
    m1[0:16, 0:64] = np.random.default_rng(3).choice(np.array([-32768, 32767, -1, 0, 5], np.int16), (16, 64, 2))
    return m1, np.random.default_rng(4).integers(0, 1024, (H, W)).astype(np.uint16)


def _maps(name, rect):
    if name == "scatter":
        return scene.scatter_map()
    if name == "outside":
        return _outside_map()
    return ref.rectify_map(*scene.lens_case(name, rect), W, H)


def _layout(B, C, pitch_pad, gap, offset, fill, w=W, h=H):
    """A flat device buffer of `fill` bytes and the [B,h,w,C] view inside it: rows pitch_pad bytes
    longer than the pixels, images gap bytes apart, the first pixel at `offset`."""
    pitch = w * C + pitch_pad
    stride = pitch * h + gap
    flat = torch.full((offset + B * stride + 16,), fill, dtype=torch.uint8, device="cuda")
    return flat, flat.as_strided((B, h, w, C), (stride, pitch, C, 1), offset)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", ["aligned", "rolled", "scatter", "outside"])
def test_remap_matches_spec_on_both_paths(ctx, rect, images, name, channels):
    src_np = images if channels == 3 else np.ascontiguousarray(images[..., 1:2])
    map1, map2 = _maps(name, rect)
    staged = ref.tile_paths(map1, channels)
    if name == "aligned":
        assert staged.all()
    elif name == "scatter":
        assert not staged.any()
    elif (name, channels) in (("rolled", 3), ("outside", 1), ("outside", 3)):
        assert staged.any() and not staged.all()
    want = np.stack([ref.remap(src_np[b], map1, map2) for b in range(3)])
    m1, m2 = torch.from_numpy(map1).cuda(), torch.from_numpy(map2).cuda()
    sflat, sview = _layout(3, channels, 5, 11, 2, 0xA5)     # odd pitch: the rows' dword alignment varies
    sview.copy_(torch.from_numpy(src_np).cuda())
    sbefore = sflat.clone()
    dflat, dview = _layout(3, channels, 3, 7, 1, 0x5A)      # misaligned rows: the scalar store path
    expect = dflat.clone()
    expect.as_strided(dview.shape, dview.stride(), 1).copy_(torch.from_numpy(want).cuda())
    try:
        for budget in (ref.header_macros()[2], 0):          # staged where the rule says so; all direct
            dview.fill_(0x5A)
            ctx.rectify_lds_budget(budget)
            ctx.remap(sview, m1, m2, out=dview)
            assert torch.equal(dflat, expect), (name, channels, budget)  # the images, and the sentinels around them
            got = ctx.remap(torch.from_numpy(src_np).cuda(), m1, m2)     # contiguous: the dword store path
            assert np.array_equal(got.cpu().numpy(), want), (name, channels, budget)
    finally:
        ctx.rectify_lds_budget(ref.header_macros()[2])
    assert torch.equal(sflat, sbefore)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", ["aligned", "rolled"])
def test_rectify_gray_matches_spec_and_the_unfused_chain(ctx, rect, images, name, channels):
    src_np = images if channels == 3 else np.ascontiguousarray(images[..., 1])
    K, d, R, newK = scene.lens_case(name, rect)
    want = np.stack([ref.rectify_gray(src_np[b], K, d, R, newK) for b in range(3)])
    sflat, sview = _layout(3, channels, 5, 11, 2, 0xA5)
    sview.copy_(torch.from_numpy(src_np.reshape(3, H, W, channels)).cuda())
    sbefore = sflat.clone()
    dflat, dview = _layout(3, 1, 3, 7, 1, 0x5A)
    expect = dflat.clone()
    expect.as_strided(dview.shape, dview.stride(), 1).copy_(torch.from_numpy(want[..., None]).cuda())
    try:
        for budget in (ref.header_macros()[2], 0):
            dview.fill_(0x5A)
            ctx.rectify_lds_budget(budget)
            ctx.rectify_gray(sview, K, d, R, newK, out=dview)
            assert torch.equal(dflat, expect), (name, channels, budget)
            got = ctx.rectify_gray(torch.from_numpy(src_np).cuda(), K, d, R, newK)
            assert np.array_equal(got.cpu().numpy(), want), (name, channels, budget)
    finally:
        ctx.rectify_lds_budget(ref.header_macros()[2])
    assert torch.equal(sflat, sbefore)
    # fused == map -> remap -> 14-bit gray, all on the device path
    m1, m2 = ctx.rectify_map(K, d, R, newK)
    chain = ctx.remap(torch.from_numpy(src_np).cuda(), m1, m2).cpu().numpy()
    chain = ref.bgr2gray(chain) if channels == 3 else chain[..., 0]
    assert np.array_equal(chain, want)


@pytest.mark.parametrize("channels", [1, 3])
def test_rectify_gray_97x64(rect, channels):
    w, h = 97, 64
    c = _small_ctx(w, h)
    Kl, dl, _, _, _, _ = scene.rig(4.0, 0.1)
    src = np.random.default_rng(channels).integers(0, 256, (2, h, w, channels), dtype=np.uint8)
    for K, d, R, newK in ((Kl, dl, rect.R1, None), (Kl, D8, scene.rotz(30.0), Kl)):
        want = np.stack([ref.rectify_gray(src[b] if channels == 3 else src[b, ..., 0], K, d, R, newK) for b in range(2)])
        dflat, dview = _layout(2, 1, 0, 0, 0, 0x5A, w, h)   # pitch 97: three rows of four are misaligned
        c.rectify_gray(torch.from_numpy(src).cuda(), K, d, R, newK, out=dview)
        assert np.array_equal(dview[..., 0].cpu().numpy(), want)
        assert bool((dflat[2 * w * h:] == 0x5A).all())
        m1, m2 = c.rectify_map(K, d, R, newK)
        got = c.remap(torch.from_numpy(src).cuda(), m1, m2).cpu().numpy()
        assert np.array_equal(got, np.stack([ref.remap(src[b], *ref.rectify_map(K, d, R, newK, w, h)) for b in range(2)]))


def test_cv2_compat_rectification_calls(rect, images):
    from forest_slam_amd import cv2_compat as cv
    Kl, dl, Kr, dr, R, T = scene.rig()
    R1, R2, P1, P2, Q, roi1, roi2 = cv.stereoRectify(Kl, dl, Kr, dr, (W, H), R, T)
    assert np.array_equal(R1, rect.R1) and np.array_equal(P2, rect.P2) and roi1 == rect.roi1
    m1, m2 = cv.initUndistortRectifyMap(Kr, dr, R2, P2, (W, H), cv.CV_16SC2)   # a 3x4 P is sliced
    w1, w2 = ref.rectify_map(Kr, dr, R2, P2[:, :3], W, H)
    assert np.array_equal(m1, w1) and np.array_equal(m2, w2)
    assert np.array_equal(cv.remap(images[0], m1, m2, cv.INTER_LINEAR), ref.remap(images[0], w1, w2))
    assert np.array_equal(cv.remap(images[0][..., 0], m1, m2, cv.INTER_LINEAR), ref.remap(images[0][..., 0], w1, w2))
    with pytest.raises(NotImplementedError):
        cv.initUndistortRectifyMap(Kr, dr, R2, P2, (W, H), 5)
    with pytest.raises(NotImplementedError):
        cv.remap(images[0], m1, m2, 0)


# ------------------------------------------------------------------ the bag pipeline
def _bag(path, encoding, n=4):
    from forest_slam_amd import pipeline as pl
    from forest_slam_amd import rosbag as rb
    rig = scene.rig()
    sc = scene.Scene(6, cells_per_m=15.0, relief=0.4)  # corners ORB can follow; points off the plane for PnP
    frames = []
    with rb.BagWriter(path) as w:
        for i in range(n):
            Rc = scene.rodrigues(np.array([0.002, -0.004, 0.003]) * i)
            L, R = (np.clip((g.astype(np.int32) - 128) * 3 + 128, 0, 255).astype(np.uint8)   # camera gain
                    for g in sc.stereo_pair(*rig, Rc=Rc, Tc=np.array([-0.03, 0.01, -0.05]) * i))
            if encoding == "bgr8":  # three different channels, so BGR2GRAY's weights matter
                L, R = (np.stack([255 - g, g, g], axis=2) for g in (L, R))
            frames.append((L, R))
            tl, tr = rb.Time(3000 + i, 0), rb.Time(3000 + i, 400)
            w.write(pl.LEFT, rb.image_message(L, tl, encoding=encoding), tl)
            w.write(pl.RIGHT, rb.image_message(R, tr, encoding=encoding), tr)
    return frames


def test_run_stereo_bag_rectified_matches_oracle(tmp_path, oracle_mod, rect, monkeypatch, encoding="mono8"):
    """A 320 x 200 two-topic mono8 bag of 4 pairs of the x4 rig through run_stereo_bag(rectify=(R, T)):
    one ingested frame bit-identical to the specification, statuses and poses equal to the oracle
    chain on specification-rectified images (as test_run_stereo_bag_600p_bgr8_matches_oracle)."""
    from forest_slam_amd import eval as ev
    from forest_slam_amd import pipeline as pl
    Kl, dl, Kr, dr, R, T = scene.rig()
    path = str(tmp_path / "r.bag")
    frames = _bag(path, encoding)
    from forest_slam_amd import _lib
    ingested = []  # every gray batch the bag run's own ingest produced, in call order: L, R per batch
    inner = _lib.Context.rectify_gray

    def spy(self, *a, **kw):
        out = inner(self, *a, **kw)
        ingested.append(out.cpu().numpy().copy())
        return out

    monkeypatch.setattr(_lib.Context, "rectify_gray", spy)
    rows, Tg, st = pl.run_stereo_bag(path, batch=2, nfeatures=300, device="cuda:0", K_left=Kl, dist_left=dl,
                                     K_right=Kr, dist_right=dr, rectify=(R, T))
    monkeypatch.undo()
    grays = [(ref.rectify_gray(L, Kl, dl, rect.R1, rect.P1[:, :3]), ref.rectify_gray(Rr, Kr, dr, rect.R2, rect.P2[:, :3]))
             for L, Rr in frames]
    # the frames the pipeline fed its front end: pair 0 alone (prime), then batches of 2 -> pairs 1-2, pair 3
    assert [len(g) for g in ingested] == [1, 1, 2, 2, 1, 1]
    got_l, got_r = np.concatenate(ingested[0::2]), np.concatenate(ingested[1::2])
    for i in range(4):
        assert np.array_equal(got_l[i], grays[i][0]) and np.array_equal(got_r[i], grays[i][1]), i
    import pipeline_ref
    outs, _ = pipeline_ref.sequence(oracle_mod, grays, rect.K_rect, np.zeros(5), rect.baseline, 300)
    valid = np.array([o["T"] is not None for o in outs])
    Ts = np.stack([o["T"] if o["T"] is not None else np.eye(4) for o in outs])
    assert len(Tg) == 3 and valid.all()
    assert all(np.abs(t[:3, 3]).max() < 0.2 for t in Ts)  # the camera moves 6 cm per frame: sane poses
    assert np.array_equal(st != -1, valid)
    for i in np.flatnonzero(valid):
        assert np.abs(Tg[i] - Ts[i]).max() < 1e-4, i
    ref_rows = ev.tum_rows(np.array([3001 + 400e-9, 3002 + 400e-9, 3003 + 400e-9])[valid], ev.chain(Ts, valid))
    assert rows.shape == ref_rows.shape
    assert np.abs(rows[:, 0] - ref_rows[:, 0]).max() < 1e-6 and np.abs(rows[:, 1:4] - ref_rows[:, 1:4]).max() < 1e-3


def test_run_stereo_bag_without_rectify_is_unchanged(tmp_path):
    from forest_slam_amd import pipeline as pl
    Kl, dl, Kr, dr, R, T = scene.rig(1.0)
    path = str(tmp_path / "u.bag")
    _bag(path, "bgr8", n=3)
    kw = dict(batch=2, nfeatures=300, device="cuda:0", K_left=Kl, dist_left=dl, K_right=Kr, dist_right=dr)
    a, b = pl.run_stereo_bag(path, **kw), pl.run_stereo_bag(path, rectify=None, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_mono_batch_whose_count_equals_height_and_width():
    """64 mono images of 64 x 64: the shape alone reads as [B,H,W]; channels= states it."""
    from forest_slam_amd import _lib
    c = _lib.Context(64, 64, max_batch=64, stages=_lib.STAGE_BF, kp_capacity=64)
    Kl, dl, _, _, _, _ = scene.rig(4.0, 0.1)
    src = np.random.default_rng(8).integers(0, 256, (64, 64, 64), dtype=np.uint8)
    want = np.stack([ref.rectify_gray(src[b], Kl, dl, scene.rotz(3.0), None) for b in (0, 63)])
    for kw in ({}, {"channels": 1}):
        got = c.rectify_gray(torch.from_numpy(src).cuda(), Kl, dl, scene.rotz(3.0), None, **kw).cpu().numpy()
        assert got.shape == (64, 64, 64) and np.array_equal(got[[0, 63]], want)
    with pytest.raises(ValueError):
        c.rectify_gray(torch.from_numpy(src).cuda(), Kl, dl, None, None, channels=3)
