"""Disparity speckle filter (cv2.filterSpeckles, CV_16SC1): fvo_filter_speckles, its bindings,
the cv2 shim and the stereo front end, against the flood-fill restatement tests/speckle_ref.py.
A region's size is a fact about the image, so every GPU comparison is exact (np.array_equal)."""
import functools

import numpy as np
import pytest

import speckle_ref as ref
from conftest import gpu_available
from sanitize_build import run_check

NV = -16  # (minDisparity - 1) * 16 of the reference's StereoSGBM


# ----------------------------------------------------------------------------- known answers
def _known():
    """(name, img, newVal, maxSpeckleSize, maxDiff, expected) on tiny arrays, written by hand."""
    i16 = lambda a: np.asarray(a, np.int16)  # noqa: E731
    out = []
    # newVal pixels must not bridge two regions, although they are within maxDiff of both: the
    # left and right columns (3 px each) touch only the newVal column between them
    a = i16([[10, NV, 10], [10, NV, 10], [10, NV, 10]])
    out.append(("newval_no_bridge_removed", a, NV, 3, 100, np.full((3, 3), NV, np.int16)))
    out.append(("newval_no_bridge_kept", a, NV, 2, 100, a))
    # one newVal pixel in the centre of a ring: the ring (8 px) is one region around it
    ring = i16([[10, 10, 10], [10, NV, 10], [10, 10, 10]])
    out.append(("newval_centre_ring_kept", ring, NV, 7, 100, ring))
    out.append(("newval_centre_ring_removed", ring, NV, 8, 100, np.full((3, 3), NV, np.int16)))
    # which value is newVal is the caller's choice: with 10 as newVal the -16 column is a 3-px region
    out.append(("newval_is_a_value", a, 10, 3, 0, np.full((3, 3), 10, np.int16)))
    # diagonal-only contact stays separate: four singletons
    d = i16([[5, NV, 5], [NV, 5, NV], [5, NV, 5]])
    out.append(("diagonal_separate", d, NV, 1, 100, np.full((3, 3), NV, np.int16)))
    # ... while with 4-contact the same five pixels are one region of 5
    p = i16([[NV, 5, NV], [5, 5, 5], [NV, 5, NV]])
    out.append(("plus_is_one_region", p, NV, 4, 0, p))
    out.append(("plus_removed_at_5", p, NV, 5, 0, np.full((3, 3), NV, np.int16)))
    # a ramp stepping by exactly maxDiff is one region (ends 7 * maxDiff apart) ...
    r = i16([[0, 16, 32, 48, 64, 80, 96, 112]])
    out.append(("ramp_step_eq_maxdiff_kept", r, NV, 7, 16, r))
    out.append(("ramp_step_eq_maxdiff_removed", r, NV, 8, 16, np.full((1, 8), NV, np.int16)))
    # ... stepping by maxDiff + 1 it is all singletons
    out.append(("ramp_step_gt_maxdiff", r, NV, 1, 15, np.full((1, 8), NV, np.int16)))
    # sizes exactly maxSpeckleSize (removed) and maxSpeckleSize + 1 (kept), side by side
    s = i16([[7, 7, 7, NV, 9, 9, 9, 9], [NV] * 8])
    out.append(("size_boundary", s, NV, 3, 0, i16([[NV, NV, NV, NV, 9, 9, 9, 9], [NV] * 8])))
    # the difference is taken in int: -32768 next to 32767 differ by 65535, not by 1
    e = i16([[-32768, 32767]])
    out.append(("int16_extremes_maxdiff_32767", e, 0, 1, 32767, i16([[0, 0]])))
    out.append(("int16_extremes_maxdiff_65534", e, 0, 1, 65534, i16([[0, 0]])))
    out.append(("int16_extremes_maxdiff_65535", e, 0, 1, 65535, e))
    out.append(("int16_extremes_maxdiff_int32max", e, 0, 1, 2**31 - 1, e))
    out.append(("newval_int16_min", i16([[-32768, 5, -32768]]), -32768, 1, 0, i16([[-32768] * 3])))
    out.append(("newval_int16_max", i16([[32767, 5, 5]]), 32767, 1, 0, i16([[32767, 5, 5]])))
    # maxDiff = 0: only equal neighbours join
    z = i16([[3, 3, 4, 4, 4], [3, 5, 5, 4, 6]])
    out.append(("maxdiff_0", z, NV, 3, 0, i16([[NV, NV, 4, 4, 4], [NV, NV, NV, 4, NV]])))
    # maxSpeckleSize <= 0 changes nothing
    out.append(("maxsize_0", z, NV, 0, 100, z))
    out.append(("maxsize_negative", z, NV, -3, 100, z))
    return out


@pytest.mark.parametrize("case", _known(), ids=lambda c: c[0])
def test_restatement_known_answers(case):
    _, img, nv, ms, md, want = case
    keep = img.copy()
    assert np.array_equal(ref.filter_speckles(img, nv, ms, md), want)
    assert np.array_equal(img, keep)  # the restatement returns a copy


def test_restatement_chain_joins_distant_values_and_ignores_scan_order():
    rng = np.random.default_rng(5)
    a = (rng.integers(0, 4, (40, 50)) * 16).astype(np.int16)
    a[rng.random(a.shape) < 0.2] = NV
    want = ref.filter_speckles(a, NV, 12, 16)
    assert (want != a).any() and (want == a).any()
    # flips and the transpose visit the pixels in other orders: the same regions come out
    assert np.array_equal(ref.filter_speckles(a[::-1, ::-1], NV, 12, 16)[::-1, ::-1], want)
    assert np.array_equal(ref.filter_speckles(np.ascontiguousarray(a.T), NV, 12, 16).T, want)


@functools.lru_cache(maxsize=None)
def _real_disparity():
    import oracle
    from forest_slam_amd import synth
    oracle.build()
    seq = synth.StereoSequence(seed=3, n_frames=2, W=320, H=200, device="cpu")
    L, R = (x.numpy() for x in seq.frame(0))
    disp = oracle.sgbm(L, R, num_disp=64)
    lab, sizes = ref.regions(disp, NV, 32)
    return L, R, disp, sizes, ref.apply(disp, lab, sizes, NV, 100)


def test_restatement_on_real_disparity():
    """oracle.sgbm of synth seed 3 frame 0, window 100, range 2: the figures the GPU test's
    "some change, some stay" rests on."""
    _, _, disp, sizes, want = _real_disparity()
    assert int((disp != NV).sum()) == 46679
    assert int((want != disp).sum()) == 999 and sum(1 for s in sizes if s <= 100) == 97
    assert max(sizes) == 22935


def test_restatement_matches_opencv():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(11)
    imgs = [c[1] for c in _known()] + [(rng.integers(0, 4, (60, 90)) * 16).astype(np.int16), _real_disparity()[2]]
    for img in imgs:
        for ms, md in ((1, 0), (3, 16), (100, 32), (img.size, 65535)):
            got = img.copy()
            cv2.filterSpeckles(got, NV, ms, md)
            assert np.array_equal(got, ref.filter_speckles(img, NV, ms, md)), (img.shape, ms, md)


def test_sgbm_with_speckle_arguments_matches_opencv():
    cv2 = pytest.importorskip("cv2")
    L, R, _, _, want = _real_disparity()
    sg = cv2.StereoSGBM_create(numDisparities=64, minDisparity=0, blockSize=7, P1=392, P2=1568, speckleWindowSize=100,
                               speckleRange=2, mode=cv2.STEREO_SGBM_MODE_SGBM_3WAY)
    assert np.array_equal(sg.compute(L, R), want)


def test_host_validation_under_sanitizers(tmp_path):
    """fvo_filter_speckles and fvo_speckle_workspace_bytes of csrc/capi.cpp (every error path, the
    no-launch cases, the workspace arithmetic) as a stand-alone ASan + UBSan program:
    tests/sanitize/speckle_check.cpp."""
    run_check("speckle_check", tmp_path)


def test_shim_accepts_speckle_arguments_and_refuses_uint8():
    from forest_slam_amd import cv2_compat as cv2
    sg = cv2.StereoSGBM_create(numDisparities=64, blockSize=7, P1=392, P2=1568, speckleWindowSize=100, speckleRange=2,
                               mode=cv2.STEREO_SGBM_MODE_SGBM_3WAY)
    assert (sg.speckle_window, sg.speckle_range) == (100, 2)
    with pytest.raises(NotImplementedError):
        cv2.StereoSGBM_create(numDisparities=64, blockSize=7, uniquenessRatio=10, speckleWindowSize=100,
                              mode=cv2.STEREO_SGBM_MODE_SGBM_3WAY)
    with pytest.raises(NotImplementedError):
        cv2.filterSpeckles(np.zeros((4, 4), np.uint8), 0, 10, 1)
    with pytest.raises(cv2.error):
        cv2.filterSpeckles(np.zeros((4, 4), np.float32), 0, 10, 1)


# ----------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _ctx():
    from forest_slam_amd import _lib
    return _lib.Context(64, 64, max_batch=4, stages=_lib.STAGE_BF, kp_capacity=64)


def _gpu_filter(imgs, nv, ms, md, workspace=None):
    """imgs: NumPy int16 [B,H,W] -> the kernel's result as NumPy."""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    out = _ctx().filter_speckles(d, nv, ms, md, workspace=workspace)
    assert out is d
    return d.cpu().numpy()


def _path_image(H, W, path, vals, fill=NV):
    a = np.full((H, W), fill, np.int16)
    for (y, x), v in zip(path, vals):
        a[y, x] = v
    return a


def _serpentine(H, W):
    """One-pixel-wide path: every even row in full, joined alternately at its right / left end."""
    path = []
    for k, y in enumerate(range(0, H, 2)):
        xs = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H:
            path.append((y + 1, W - 1 if k % 2 == 0 else 0))
    return path


def _spiral(H, W):
    """One-pixel-wide inward spiral with one-pixel gaps between the turns."""
    path = [(0, 0)]
    y, x, dy, dx = 0, 0, 0, 1
    blocked = np.zeros((H, W), bool)
    blocked[0, 0] = True

    def free(yy, xx, py, px):
        if not (0 <= yy < H and 0 <= xx < W) or blocked[yy, xx]:
            return False
        for ny, nx in ((yy + 1, xx), (yy - 1, xx), (yy, xx + 1), (yy, xx - 1)):  # no contact but the predecessor
            if (ny, nx) != (py, px) and 0 <= ny < H and 0 <= nx < W and blocked[ny, nx]:
                return False
        return True

    while True:
        if free(y + dy, x + dx, y, x):
            y, x = y + dy, x + dx
        else:
            dy, dx = dx, -dy  # turn right
            if not free(y + dy, x + dx, y, x):
                break
            y, x = y + dy, x + dx
        path.append((y, x))
        blocked[y, x] = True
    return path


SIZES = [(1, 1), (1, 300), (300, 1), (33, 65), (127, 129), (200, 320)]


def _adversarial(H, W):
    """[(name, imgs int16 [3,H,W] with different content per image, newVal, maxDiff, [maxSpeckleSize ...])]"""
    rng = np.random.default_rng(1000 * H + W)
    cases = []
    for name, path in (("serpentine", _serpentine(H, W)), ("spiral", _spiral(H, W))):
        n = len(path)
        ramp = (100 + 16 * (np.arange(n) % 7)).astype(np.int16)   # steps of 16 and one of -96 per period
        tri = (100 + 16 * np.abs((np.arange(n) % 12) - 6)).astype(np.int16)  # steps of exactly 16 throughout
        whole = _path_image(H, W, path, tri)                       # one region of n pixels, values 96 apart
        pieces = _path_image(H, W, path, ramp)                     # maxDiff 16: broken every 7 pixels
        cut = whole.copy()                                         # a few newVal cuts: pieces of uneven length
        for k in sorted(set(int(v) for v in rng.integers(0, n, 5))):
            cut[path[k]] = NV
        cases.append((name, np.stack([whole, pieces, cut]), NV, 16, [6, 7, max(1, n // 6), n - 1, n]))
    board = np.stack([np.where((np.add.outer(np.arange(H), np.arange(W)) + b) % 2 == 0, 200 + b, NV).astype(np.int16)
                      for b in range(3)])
    if W > 3:
        board[2, H // 2, 1:3] = 77  # a domino among the singletons
    cases.append(("checkerboard", board, NV, 100, [1, 2]))
    alpha = (rng.integers(0, 4, (3, H, W)) * 16).astype(np.int16)
    alpha[1][rng.random((H, W)) < 0.3] = NV
    alpha[2] = (rng.integers(0, 4, (H, W)) * 17).astype(np.int16)  # steps of 17: only equal values join
    cases.append(("alphabet4", alpha, NV, 16, [1, 3, 20, 200]))
    uni = np.full((3, H, W), 640, np.int16)
    uni[1, H // 2, W // 2] = 0          # a singleton hole in the middle
    uni[2, :, W // 2] = NV              # split into two halves
    cases.append(("uniform", uni, NV, 0, [1, H * W // 2, H * W - 1, H * W, H * W + 5]))
    return cases


@functools.lru_cache(maxsize=None)
def _adversarial_with_reference(H, W):
    out = []
    for name, imgs, nv, md, sizes in _adversarial(H, W):
        regs = [ref.regions(im, nv, md) for im in imgs]
        out.append((name, imgs, nv, md, [(ms, np.stack([ref.apply(im, lab, sz, nv, ms) for im, (lab, sz) in
                                                        zip(imgs, regs)])) for ms in sizes]))
    return out


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
@pytest.mark.parametrize("H,W", SIZES)
def test_gpu_adversarial_maps(H, W):
    changed = kept = 0
    for name, imgs, nv, md, per_size in _adversarial_with_reference(H, W):
        for ms, want in per_size:
            got = _gpu_filter(imgs, nv, ms, md)
            assert np.array_equal(got, want), (name, H, W, ms, int((got != want).sum()))
            changed += int((want != imgs).sum())
            kept += int(((want == imgs) & (imgs != nv)).sum())
    assert changed > 0 and (kept > 0 or H * W == 1)


def test_adversarial_generators():
    """The paths are what they claim: one pixel wide, one region, crossing the whole image."""
    for H, W in ((33, 65), (127, 129)):
        for gen in (_serpentine, _spiral):
            path = gen(H, W)
            assert len(set(path)) == len(path) > (H * W) // 3
            img = _path_image(H, W, path, [5] * len(path))
            _, sizes = ref.regions(img, NV, 0)
            assert sizes == [len(path)]
            steps = np.abs(np.diff(np.asarray(path), axis=0)).sum(1)
            assert (steps == 1).all()


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
@pytest.mark.parametrize("case", _known(), ids=lambda c: c[0])
def test_gpu_known_answers(case):
    _, img, nv, ms, md, want = case
    assert np.array_equal(ref.filter_speckles(img, nv, ms, md), want)
    assert np.array_equal(_gpu_filter(img[None], nv, ms, md)[0], want)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_thresholds_across_tiles():
    """The boundary size, the ramp and maxDiff = 0 again, with regions that straddle tile seams."""
    H, W = 70, 150
    a = np.full((H, W), NV, np.int16)
    a[30:34, 60:70] = 5          # 40 pixels over the corner of four tiles
    a[10, 20:61] = 9             # 41 pixels in a row
    a[40:50, 100] = np.arange(10) * 3 + 100   # a vertical ramp of step 3, 10 pixels
    a[60, 0:140] = (np.arange(140) * 2).astype(np.int16)  # a horizontal ramp of step 2, 140 pixels
    for ms, md in ((40, 0), (39, 0), (41, 0), (10, 3), (10, 2), (140, 2), (139, 2), (1, 1)):
        want = ref.filter_speckles(a, NV, ms, md)
        assert np.array_equal(_gpu_filter(a[None], NV, ms, md)[0], want), (ms, md)
    keep = ref.filter_speckles(a, NV, 40, 0)
    assert (keep[30:34, 60:70] == NV).all() and (keep[10, 20:61] == 9).all()


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_real_disparity():
    _, _, disp, _, want = _real_disparity()
    got = _gpu_filter(disp[None], NV, 100, 32)[0]
    assert np.array_equal(got, want)
    assert (got != disp).any() and ((got == disp) & (disp != NV)).any()


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_pitch_view_leaves_outside_columns():
    import torch
    rng = np.random.default_rng(3)
    buf = (rng.integers(0, 4, (2, 100, 200)) * 16).astype(np.int16)
    d = torch.from_numpy(buf).cuda()
    view = d[:, :, 30:180]
    assert view.stride(1) == 200
    assert _ctx().filter_speckles(view, NV, 6, 16) is view
    got = d.cpu().numpy()
    want = buf.copy()
    for b in range(2):
        want[b, :, 30:180] = ref.filter_speckles(buf[b, :, 30:180], NV, 6, 16)
    assert np.array_equal(got, want)
    assert (want != buf).any()
    assert np.array_equal(got[:, :, :30], buf[:, :, :30]) and np.array_equal(got[:, :, 180:], buf[:, :, 180:])
    # a 2-D view (one image)
    one = torch.from_numpy(buf[0]).cuda()
    _ctx().filter_speckles(one[:, 30:180], NV, 6, 16)
    assert np.array_equal(one.cpu().numpy(), want[0])


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_workspace_reuse_and_determinism():
    import torch
    rng = np.random.default_rng(4)
    a = (rng.integers(0, 4, (3, 127, 129)) * 16).astype(np.int16)
    b = (rng.integers(0, 3, (3, 127, 129)) * 16).astype(np.int16)
    b[:, ::5] = NV
    ctx = _ctx()
    ws = torch.full((ctx.speckle_workspace_bytes(3, 127, 129),), 0xA5, dtype=torch.uint8, device="cuda")
    want_a = np.stack([ref.filter_speckles(x, NV, 9, 16) for x in a])
    want_b = np.stack([ref.filter_speckles(x, NV, 9, 16) for x in b])
    got_a = _gpu_filter(a, NV, 9, 16, workspace=ws)
    got_b = _gpu_filter(b, NV, 9, 16, workspace=ws)   # the workspace as the first call left it
    got_a2 = _gpu_filter(a, NV, 9, 16, workspace=ws)
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
    assert got_a.tobytes() == got_a2.tobytes()
    with pytest.raises(ValueError):
        ctx.filter_speckles(torch.from_numpy(a).cuda(), NV, 9, 16, workspace=ws[:-1])
    with pytest.raises(RuntimeError, match="max_diff"):
        ctx.filter_speckles(torch.from_numpy(a).cuda(), NV, 9, -1, workspace=ws)
    with pytest.raises(RuntimeError, match="max_batch"):
        ctx.filter_speckles(torch.zeros((5, 4, 4), dtype=torch.int16, device="cuda"), NV, 9, 1)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_hip_graph_replay_equals_eager():
    import torch
    _, _, disp, _, want = _real_disparity()
    ctx = _ctx()
    src = torch.from_numpy(disp[None]).cuda()
    ws = torch.empty((ctx.speckle_workspace_bytes(1, 200, 320),), dtype=torch.uint8, device="cuda")
    eager = ctx.filter_speckles(src.clone(), NV, 100, 32, workspace=ws).cpu().numpy()
    buf = src.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.filter_speckles(buf, NV, 100, 32, workspace=ws)
    buf.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), eager) and np.array_equal(eager[0], want)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_cv2_shim():
    import torch
    from forest_slam_amd import cv2_compat as cv2
    L, R, disp, _, want = _real_disparity()
    sg = cv2.StereoSGBM_create(numDisparities=64, blockSize=7, P1=392, P2=1568, speckleWindowSize=100, speckleRange=2,
                               mode=cv2.STEREO_SGBM_MODE_SGBM_3WAY)
    assert np.array_equal(sg.compute(L, R), want)
    assert np.array_equal(sg.computeDevice(L, R).cpu().numpy(), want)
    plain = cv2.StereoSGBM_create(numDisparities=64, blockSize=7, P1=392, P2=1568, mode=cv2.STEREO_SGBM_MODE_SGBM_3WAY)
    assert np.array_equal(plain.compute(L, R), disp)
    # filterSpeckles on a NumPy array: in place, like cv2
    a = disp.copy()
    img, buf = cv2.filterSpeckles(a, NV, 100, 32)
    assert img is a and np.array_equal(a, want)
    # ... and on a device tensor, reusing the returned scratch
    t = torch.from_numpy(disp).cuda()
    img2, buf2 = cv2.filterSpeckles(t, NV, 100, 32, buf)
    assert img2 is t and buf2 is buf and np.array_equal(t.cpu().numpy(), want)
    # maxSpeckleSize 0 changes nothing
    b = disp.copy()
    cv2.filterSpeckles(b, NV, 0, 32)
    assert np.array_equal(b, disp)


# ----------------------------------------------------------------------------- front end
@functools.lru_cache(maxsize=None)
def _frontend_oracle():
    """Oracle chain orb -> bf_match -> sgbm -> restatement -> disparity_map -> backproject of the
    pairs (j, j+1), j = 0..2, of synth seed 3 (320x200)."""
    import oracle
    from forest_slam_amd import synth
    oracle.build()
    seq = synth.StereoSequence(seed=3, n_frames=4, W=320, H=200, device="cpu")
    frames = [tuple(x.numpy() for x in seq.frame(i)) for i in range(4)]
    orb = [oracle.orb_detect_compute(f[0], 300) for f in frames]
    pairs = []
    for j in range(3):
        (kp0, d0), (kp1, d1) = orb[j], orb[j + 1]
        m = oracle.bf_match(d0, d1)
        mk0 = kp0[:, :2].astype(np.float32)[m[:, 0]]
        mk1 = kp1[:, :2].astype(np.float32)[m[:, 1]]
        raw = oracle.sgbm(frames[j][0], frames[j][1], num_disp=64)
        disp = ref.filter_speckles(raw, NV, 100, 32)
        P3, p2, _ = oracle.backproject(oracle.disparity_map(disp), mk0, mk1, seq.K, synth.BASELINE)
        P3_raw, _, _ = oracle.backproject(oracle.disparity_map(raw), mk0, mk1, seq.K, synth.BASELINE)
        hit = int((disp != raw)[mk0[:, 1].astype(int), mk0[:, 0].astype(int)].sum())
        pose = oracle.solve_pnp_ransac(P3, p2, seq.K, synth.DIST_L) if len(P3) >= 6 else None
        pairs.append(dict(raw=raw, disp=disp, P3=P3, P3_raw=P3_raw, hit=hit, pose=pose))
    return seq, frames, pairs


def test_frontend_oracle_keypoints_sit_on_removed_pixels():
    """Seed 3: matched keypoints of every pair sit on removed pixels, so the filtered chain's
    points3D differ from the unfiltered one's (at this focal length they move to Z = 543.77 m)."""
    _, _, pairs = _frontend_oracle()
    assert [p["hit"] for p in pairs] == [4, 13, 7]
    for p in pairs:
        assert p["P3"].shape == p["P3_raw"].shape and not np.array_equal(p["P3"], p["P3_raw"])
        moved = (p["P3"] != p["P3_raw"]).any(1)
        assert int(moved.sum()) == p["hit"] and np.allclose(p["P3"][moved, 2], 543.7706, atol=1e-3)


def _run_frontend(seq, frames, **kw):
    import torch
    from forest_slam_amd import synth, vo
    fe = vo.StereoFrontEnd(320, 200, seq.K, synth.DIST_L, synth.BASELINE, batch=2, nfeatures=300, num_disparities=64,
                           ba_window=0, **kw)
    L = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    R = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    fe.prime(L[0], R[0])
    out = []
    for s, e in ((1, 3), (3, 4)):  # a full step and a partial one
        T, st = fe.step(L[s:e], R[s:e])
        torch.cuda.synchronize()
        n = e - s
        npts = fe.npts[:n].cpu().numpy()
        for i in range(n):
            out.append(dict(disp=fe.disp[i].cpu().numpy(), npts=int(npts[i]), P3=fe.P3[i, :npts[i]].cpu().numpy(),
                            T=T[i].cpu().numpy().copy(), st=int(st[i].item()), rvec=fe.rvec[i].cpu().numpy(),
                            tvec=fe.tvec[i].cpu().numpy()))
    return fe, out


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_frontend_filters_before_backprojection():
    seq, frames, pairs = _frontend_oracle()
    fe, got = _run_frontend(seq, frames, speckle_window=100, speckle_range=2)
    for j, (g, w) in enumerate(zip(got, pairs)):
        assert np.array_equal(g["disp"], w["disp"]), j
        assert g["npts"] == len(w["P3"]) and np.array_equal(g["P3"], w["P3"]), j
        assert not np.array_equal(g["P3"], w["P3_raw"]), j
        ok, rv, tv = w["pose"][:3]
        assert g["st"] == int(ok)
        if ok:
            assert np.abs(g["rvec"] - rv).max() < 1e-4 and np.abs(g["tvec"] - tv).max() < 1e-4, j
    # the other front-stage order and the overlapped front stage: the same bytes
    for kw in (dict(sgbm_last=True), dict(overlap_sgbm=True), dict(overlap_sgbm=True, sgbm_last=True)):
        _, other = _run_frontend(seq, frames, speckle_window=100, speckle_range=2, **kw)
        for j, (g, o) in enumerate(zip(got, other)):
            for k in ("disp", "P3", "T"):
                assert g[k].tobytes() == o[k].tobytes(), (kw, j, k)
            assert (g["npts"], g["st"]) == (o["npts"], o["st"]), (kw, j)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_frontend_default_launches_no_speckle_kernel():
    import torch
    from forest_slam_amd import synth, vo
    seq, frames, pairs = _frontend_oracle()
    L = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    R = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    seen = {}
    for window in (0, 100):
        fe = vo.StereoFrontEnd(320, 200, seq.K, synth.DIST_L, synth.BASELINE, batch=2, nfeatures=300,
                               num_disparities=64, ba_window=0, speckle_window=window, speckle_range=2)
        assert (fe.speckle_ws is None) == (window == 0)
        fe.prime(L[0], R[0])
        fe.ctx.timing_enable(None)
        fe.step(L[1:3], R[1:3])
        seen[window] = fe.ctx.timing_read()
        fe.ctx.timing_enable([])
        torch.cuda.synchronize()
        want = pairs[0]["raw"] if window == 0 else pairs[0]["disp"]
        assert np.array_equal(fe.disp[0].cpu().numpy(), want)
    assert "sgbm_rows" in seen[0] and not [k for k in seen[0] if k.startswith("speckle")]
    assert {k: seen[100][k][1] for k in seen[100] if k.startswith("speckle")} == {
        "speckle_local": 1, "speckle_seams": 1, "speckle_sum": 1, "speckle_apply": 1}
