"""Dense stereo mapping on the GPU (csrc/dense.hip): fvo_dense_map_append, its Python faces
(Context.dense_map_append, PointMap.add_disparity, StereoFrontEnd.append_dense) and
cv2_compat.reprojectImageTo3D, bit for bit against the NumPy specification tests/dense_ref.py
(pinned to the oracles by tests/test_dense_cpu.py): the fp64 map, the float32 map, n_added and
map_count.  Shapes are the smallest that reach every path: both load paths (8-byte groups at step
1 with aligned rows of a multiple of 4 pixels; scalar loads otherwise), four-sample groups that
straddle row ends, several blocks per frame and several frames."""
import numpy as np
import pytest
import torch

import dense_ref as dr
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

GUARD = 7          # untouched elements kept behind every map
SENTINEL = -7.25


@pytest.fixture(scope="module")
def ctx():
    from forest_slam_amd import _lib
    return _lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_BF, kp_capacity=64)


def _image(B, H, W, seed, specials=True):
    rng = np.random.default_rng(seed)
    img = rng.integers(-40, 3000, size=(B, H, W)).astype(np.int16)
    img[rng.random((B, H, W)) < 0.2] = -16  # SGBM's invalid value
    if specials:
        for b in range(B):
            img[b].flat[rng.choice(H * W, len(dr.HAND_SPECIALS), replace=False)] = dr.HAND_SPECIALS
    return img


def _pose(seed):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-np.pi, np.pi, 2)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Rx
    T[:3, 3] = rng.uniform(-50, 50, 3)
    return T


def _append(ctx, view, T, count0=0, map_cap=None, step=1, min_disp16=1, z_min=0.1, z_max=1000.0, keep=None,
            use64=True, use32=True, K=dr.HAND_K, baseline=dr.HAND_BASELINE):
    """One fvo_dense_map_append on the int16 device tensor `view` (possibly a window of a wider
    buffer) against dense_ref: maps of map_cap + GUARD sentinel elements, everything compared bit
    for bit, the disparity buffer compared before and after.  map_cap None = exactly the total.
    Returns (cloud, n_added, new count) of the reference."""
    host = view.cpu().numpy()
    before = view.clone()
    cloud, n_ref = dr.dense_cloud(host, K, baseline, T, step, min_disp16, z_min, z_max, keep)
    cap = count0 + len(cloud) if map_cap is None else map_cap
    g64 = np.full((cap + GUARD, 3), SENTINEL) if use64 else None
    g32 = np.full((cap + GUARD, 3), SENTINEL, np.float32) if use32 else None
    w64, w32, cnt_ref = dr.append(cloud, count0, g64, g32, map_cap=cap)
    m64 = torch.from_numpy(g64).cuda() if use64 else None
    m32 = torch.from_numpy(g32).cuda() if use32 else None
    cnt = torch.tensor([count0], dtype=torch.int32, device="cuda")
    n_added = torch.full((len(host),), -1, dtype=torch.int32, device="cuda")
    kt = None if keep is None else torch.tensor(keep, dtype=torch.int32, device="cuda")
    ctx.dense_map_append(view, K, baseline, torch.from_numpy(np.ascontiguousarray(T)).cuda(), cnt, m64, m32,
                         step=step, min_disp16=min_disp16, z_min=z_min, z_max=z_max, frame_keep=kt,
                         n_added=n_added, map_cap=cap)
    torch.cuda.synchronize()
    print(f"dense: {tuple(host.shape)} step {step} min {min_disp16}: {len(cloud)} points, count {cnt_ref}")
    assert int(cnt.item()) == cnt_ref
    assert np.array_equal(n_added.cpu().numpy(), n_ref)
    if use64:
        assert np.array_equal(m64.cpu().numpy().view(np.uint64), w64.view(np.uint64))
    if use32:
        assert np.array_equal(m32.cpu().numpy().view(np.uint32), w32.view(np.uint32))
    assert torch.equal(view, before)
    return cloud, n_ref, cnt_ref


@pytest.mark.parametrize("min_disp16", [-32768, 1])
def test_hand_built_image(ctx, min_disp16):
    """40x24 (one 8-byte group per thread), step 1, T = I: the invalid / zero disparities and
    their neighbours, 2 | 3 and 26100 | 26101 on either side of the depth bounds, the int16
    extremes, a ramp.  With the reference's filter the three entry points that compute the stereo
    point agree with each other, not only each with its oracle: for a keypoint at every pixel,
    fvo_backproject's points3d, fvo_keypoint_stereo's non-zero rows and the float32 map appended
    here are the same float32 triples in the same order."""
    from forest_slam_amd import _lib
    img = dr.hand_image()
    H, W = img.shape
    dev = torch.from_numpy(img[None]).cuda()
    cloud, n, _ = _append(ctx, dev, np.eye(4)[None], min_disp16=min_disp16)
    assert 0 < len(cloud) < H * W
    if min_disp16 != -32768:
        return
    pctx = _lib.Context(W, H, max_batch=1, stages=_lib.STAGE_POSE | _lib.STAGE_BA, kp_capacity=H * W, ba_window=3)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    kp = np.zeros((1, H * W, _lib.KP_STRIDE), np.float32)
    kp[0, :, 0], kp[0, :, 1] = xs.ravel(), ys.ravel()
    m = np.zeros((1, H * W, 3), np.int32)
    m[0, :, 0] = m[0, :, 1] = np.arange(H * W)
    kpt = torch.from_numpy(kp).cuda()
    nkp = torch.tensor([H * W], dtype=torch.int32, device="cuda")
    P3, _, npts = pctx.backproject(dev, kpt, kpt, torch.from_numpy(m).cuda(), nkp, dr.HAND_K, dr.HAND_BASELINE)
    assert int(npts.item()) == len(cloud)
    assert np.array_equal(P3[0, :len(cloud)].cpu().numpy(), cloud.astype(np.float32))
    stereo = pctx.keypoint_stereo(dev, kpt, nkp, dr.HAND_K, dr.HAND_BASELINE)[0].cpu().numpy()
    m32 = torch.full((len(cloud) + GUARD, 3), SENTINEL, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.dense_map_append(dev, dr.HAND_K, dr.HAND_BASELINE, torch.eye(4, dtype=torch.float64, device="cuda")[None],
                         cnt, None, m32, step=1, min_disp16=-32768, map_cap=len(cloud))
    assert int(cnt.item()) == len(cloud)
    a = P3[0, :len(cloud)].cpu().numpy().view(np.uint32)
    assert np.array_equal(stereo[stereo[:, 2] != 0][:, :3].view(np.uint32), a)
    assert np.array_equal(m32[:len(cloud)].cpu().numpy().view(np.uint32), a)


@pytest.mark.parametrize("step", [1, 2, 3, 5])
def test_ragged_grid(ctx, step):
    """37x19: scalar loads, four-sample groups that straddle row ends, the last row and column
    fall off the grid at steps 2, 3 and 5."""
    img = _image(2, 19, 37, 10 + step)
    T = np.stack([_pose(20), _pose(21)])
    _append(ctx, torch.from_numpy(img).cuda(), T, step=step)
    _append(ctx, torch.from_numpy(img).cuda(), T, step=step, min_disp16=-32768, z_min=0.0, z_max=1e6)


def test_several_blocks_and_frames(ctx):
    """131x67, B = 4 (9 blocks per frame at step 1, 3 at step 2): a general pose per frame, frame
    1 switched off by frame_keep, frame 2 entirely invalid, frame 3 entirely valid; a second
    call appends behind the first one's count."""
    img = _image(4, 67, 131, 30)
    img[2] = -16
    img[3] = np.random.default_rng(31).integers(16, 3000, size=img[3].shape).astype(np.int16)
    T = np.stack([_pose(40 + b) for b in range(4)])
    keep = [1, 0, 1, 1]
    dev = torch.from_numpy(img).cuda()
    _, n, cnt = _append(ctx, dev, T, keep=keep)
    assert n[1] == 0 and n[2] == 0 and n[3] == 67 * 131 and 0 < n[0] < 67 * 131
    _, n2, cnt2 = _append(ctx, dev, T, count0=cnt, step=2, keep=[1, 1, 0, 1])
    assert cnt2 == cnt + int(n2.sum()) and n2[1] > 0 and n2[3] == 34 * 66
    _append(ctx, dev, T, count0=5)  # frame_keep NULL


def test_vector_path_equals_scalar_path(ctx):
    """A 64-column window of a 96-wide buffer at step 1 (pitch > width; 1280 samples, two
    blocks): starting at column 0 its rows are 8-byte aligned (one load per four samples);
    the same window one column further in another buffer is misaligned and takes scalar loads."""
    win = _image(2, 20, 64, 50)
    rng = np.random.default_rng(51)
    a = rng.integers(16, 3000, size=(2, 20, 96)).astype(np.int16)
    b = a.copy()
    a[:, :, 0:64] = win
    b[:, :, 1:65] = win
    T = np.stack([_pose(52), _pose(53)])
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    assert da.data_ptr() % 8 == 0 and db.data_ptr() % 8 == 0
    ca, na, _ = _append(ctx, da[:, :, 0:64], T)
    cb, nb, _ = _append(ctx, db[:, :, 1:65], T)
    assert np.array_equal(ca, cb) and np.array_equal(na, nb)
    # the same geometry sampled at step 2 (scalar) and a 4-aligned window that is not 8-aligned
    _append(ctx, da[:, :, 0:64], T, step=2)
    _append(ctx, db[:, :, 2:66], T)
    _append(ctx, db[:, :, 4:68], T)


@pytest.mark.parametrize("arrays", ["both", "f64", "f32"])
def test_overflow_and_optional_arrays(ctx, arrays):
    """map_cap 0 and map_cap = total - 5 (here from a non-zero count): the first map_cap points
    are written, the guard elements behind them stay untouched, map_count holds the full total;
    with map_xyz64 = NULL and map_xyz32 = NULL in turn."""
    use = dict(use64=arrays != "f32", use32=arrays != "f64")
    img = _image(2, 67, 131, 60)  # 9 blocks per frame: the map ends inside a block of frame 1
    T = np.stack([_pose(61), _pose(62)])
    dev = torch.from_numpy(img).cuda()
    cloud, _, total = _append(ctx, dev, T, **use)
    assert total == len(cloud) > 2048
    _append(ctx, dev, T, map_cap=0, **use)
    _append(ctx, dev, T, map_cap=total - 5, **use)
    _append(ctx, dev, T, count0=3, map_cap=total - 2, **use)
    _append(ctx, dev, T, count0=11, map_cap=4, **use)           # the map already past its end
    _append(ctx, dev, T, count0=0, map_cap=total // 2, **use)   # ends in frame 0


def test_count_clamps_at_int32_max(ctx):
    img = _image(1, 19, 37, 70)
    _, _, cnt = _append(ctx, torch.from_numpy(img).cuda(), np.eye(4)[None], count0=dr.INT32_MAX - 3, map_cap=8)
    assert cnt == dr.INT32_MAX


def test_point_map_add_disparity_with_voxel_filter(oracle_mod):
    """PointMap.add_disparity(voxel_size=0.5): dense_ref, then oracle.voxel_down_sample, appended
    as add_cloud does; a second call appends behind the first."""
    from forest_slam_amd.mapping import PointMap
    pm = PointMap(60_000)
    want = []
    for k in range(2):
        img = _image(2, 67, 131, 80 + k)
        T = np.stack([_pose(82 + k), _pose(84 + k)])
        n = pm.add_disparity(torch.from_numpy(img).cuda(), dr.HAND_K, dr.HAND_BASELINE, T, step=1 + k,
                             z_max=60.0, voxel_size=0.5)
        cloud, n_ref = dr.dense_cloud(img, dr.HAND_K, dr.HAND_BASELINE, T, step=1 + k, z_max=60.0)
        assert np.array_equal(n.cpu().numpy(), n_ref)
        want.append(oracle_mod.voxel_down_sample(cloud, 0.5))
        assert 0 < len(want[-1]) < len(cloud)
    want = np.concatenate(want)
    assert np.array_equal(pm.cloud64(), want) and np.array_equal(pm.cloud32(), want.astype(np.float32))
    # without the filter: straight into the map, with add_frames' overflow report
    n = pm.add_disparity(torch.from_numpy(img).cuda(), dr.HAND_K, dr.HAND_BASELINE, T, step=3, keep=torch.tensor(
        [0, 1], dtype=torch.int32, device="cuda"), check=True)
    cloud, n_ref = dr.dense_cloud(img, dr.HAND_K, dr.HAND_BASELINE, T, step=3, frame_keep=[0, 1])
    assert np.array_equal(n.cpu().numpy(), n_ref) and np.array_equal(pm.cloud64()[len(want):], cloud)
    small = PointMap(10, ctx=pm.ctx)
    with pytest.raises(RuntimeError, match="overflow"):
        small.add_disparity(torch.from_numpy(img).cuda(), dr.HAND_K, dr.HAND_BASELINE, T, check=True)


def test_front_end_append_dense_overlap_on_and_off():
    """StereoFrontEnd.append_dense on synth.StereoSequence, 320x200, batch 4, three steps: the
    maps with overlap_sgbm on and off are bit-identical, and both equal dense_ref applied to host
    copies of fe.disp taken after each step (under overlap the slot is rewritten two steps later:
    append_dense re-records the event that write waits for)."""
    from forest_slam_amd import synth, vo
    from forest_slam_amd.mapping import PointMap
    W, H, B = 320, 200, 4
    seq = synth.StereoSequence(seed=33, n_frames=1 + 3 * B, W=W, H=H, device="cuda")
    L, R = seq.frames(range(1 + 3 * B))
    torch.cuda.synchronize()
    cums = np.stack([_pose(90 + i) for i in range(3 * B)])
    keep = torch.tensor([1, 1, 0, 1], dtype=torch.int32, device="cuda")
    maps = []
    for overlap in (False, True):
        fe = vo.StereoFrontEnd(W, H, seq.K, synth.DIST_L, synth.BASELINE, batch=B, nfeatures=300, num_disparities=64,
                               ba_window=0, overlap_sgbm=overlap)
        pm = PointMap(3 * B * (H // 2) * (W // 2), ctx=None)
        fe.prime(L[0], R[0])
        snaps, ns = [], []
        for s in range(3):  # no host synchronisation between the steps
            fe.step(L[1 + s * B:1 + (s + 1) * B], R[1 + s * B:1 + (s + 1) * B])
            snaps.append(fe.disp[:B].clone())  # (queued before append_dense's event, like its launches)
            ns.append(fe.append_dense(pm, cums[s * B:(s + 1) * B], step=2, z_max=80.0, keep=keep))
        torch.cuda.synchronize()
        want = []
        for s in range(3):
            c, nr = dr.dense_cloud(snaps[s].cpu().numpy(), seq.K, synth.BASELINE, cums[s * B:(s + 1) * B], step=2,
                                   z_max=80.0, frame_keep=[1, 1, 0, 1])
            assert np.array_equal(ns[s].cpu().numpy(), nr) and nr[2] == 0 and nr[0] > 1000
            want.append(c)
        want = np.concatenate(want)
        assert np.array_equal(pm.cloud64(), want) and np.array_equal(pm.cloud32(), want.astype(np.float32))
        maps.append(pm.cloud64())
    assert np.array_equal(maps[0], maps[1])


def test_second_call_and_graph_replay_append_behind_the_count(ctx):
    """Two calls on one map, then the second call captured into a graph and replayed twice:
    every append starts at the device-side count the one before left (nothing is allocated in
    the call; its three launches are stream-ordered)."""
    img = _image(3, 19, 40, 75)  # 40 columns: the 8-byte path
    T = np.stack([_pose(76 + b) for b in range(3)])
    c1, n1 = dr.dense_cloud(img, dr.HAND_K, dr.HAND_BASELINE, T)
    c2, n2 = dr.dense_cloud(img, dr.HAND_K, dr.HAND_BASELINE, T[::-1], step=3, min_disp16=-32768)
    want = np.concatenate([c1, c2, c2, c2])
    dev, T1 = torch.from_numpy(img).cuda(), torch.from_numpy(T).cuda()
    T2 = torch.from_numpy(np.ascontiguousarray(T[::-1])).cuda()
    m64 = torch.full((len(want) + GUARD, 3), SENTINEL, dtype=torch.float64, device="cuda")
    m32 = torch.full((len(want) + GUARD, 3), SENTINEL, dtype=torch.float32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    na = torch.zeros((3,), dtype=torch.int32, device="cuda")
    ws = torch.empty((ctx.dense_workspace_bytes(3, 19, 40, 1),), dtype=torch.uint8, device="cuda")
    kw = dict(n_added=na, workspace=ws, map_cap=len(want))
    ctx.dense_map_append(dev, dr.HAND_K, dr.HAND_BASELINE, T1, cnt, m64, m32, **kw)
    assert np.array_equal(na.cpu().numpy(), n1) and int(cnt.item()) == len(c1)
    ctx.dense_map_append(dev, dr.HAND_K, dr.HAND_BASELINE, T2, cnt, m64, m32, step=3, min_disp16=-32768, **kw)
    assert np.array_equal(na.cpu().numpy(), n2) and int(cnt.item()) == len(c1) + len(c2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.dense_map_append(dev, dr.HAND_K, dr.HAND_BASELINE, T2, cnt, m64, m32, step=3, min_disp16=-32768, **kw)
    cnt.fill_(len(c1) + len(c2))  # (whether or not capture ran the launches)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert int(cnt.item()) == len(want)
    got = m64.cpu().numpy()
    assert np.array_equal(got[:len(want)], want) and (got[len(want):] == SENTINEL).all()
    assert np.array_equal(m32.cpu().numpy()[:len(want)], want.astype(np.float32))


def test_run_stereo_bag_dense_map(tmp_path):
    """pipeline.run_stereo_bag(dense_map=, dense_step=, dense_z_max=): the dense map is placed by
    the poses and frame mask of the sparse point_map path.  Checked against dense_ref on the
    disparity maps, poses and statuses of the same front end run by hand over the same images."""
    from forest_slam_amd import pipeline as pl
    from forest_slam_amd import rosbag as rb
    from forest_slam_amd import synth, vo
    from forest_slam_amd.mapping import PointMap
    W, H, n, B = 320, 200, 6, 2
    seq = synth.StereoSequence(seed=4, n_frames=n, W=W, H=H, device="cpu", start=110)
    path = str(tmp_path / "d.bag")
    bgr = []
    with rb.BagWriter(path) as w:
        for i in range(n):
            pair = [np.repeat(x.numpy()[..., None], 3, axis=2) for x in seq.frame(i)]
            bgr.append(pair)
            w.write(pl.LEFT, rb.image_message(pair[0], rb.Time(1000 + i, 0)), rb.Time(1000 + i, 0))
            w.write(pl.RIGHT, rb.image_message(pair[1], rb.Time(1000 + i, 500)), rb.Time(1000 + i, 500))
    cam = dict(K_left=seq.K, dist_left=pl.DIST_L, K_right=seq.K, dist_right=pl.DIST_R, baseline=synth.BASELINE)
    dense, sparse = PointMap(n * (H // 4) * (W // 4)), PointMap(20000)
    _, T, st = pl.run_stereo_bag(path, batch=B, nfeatures=300, device="cuda:0", point_map=sparse, dense_map=dense,
                                 dense_step=4, dense_z_max=30.0, **cam)
    assert len(sparse) > 0
    # by hand: the same ingest and front end, fe.disp after each step
    fe = vo.StereoFrontEnd(W, H, seq.K, pl.DIST_L, synth.BASELINE, batch=B, nfeatures=300, device="cuda:0",
                           ba_window=0)
    up = lambda k, side, Kc, dc: fe.ctx.undistort_gray(torch.from_numpy(np.stack([bgr[i][side] for i in k])).cuda(),
                                                       Kc, dc)  # noqa: E731
    fe.prime(up([0], 0, seq.K, pl.DIST_L)[0], up([0], 1, seq.K, pl.DIST_R)[0])
    want, cum = [], np.eye(4)
    for s in range(1, n, B):
        k = list(range(s, min(s + B, n)))
        Ts, sts = fe.step(up(k, 0, seq.K, pl.DIST_L), up(k, 1, seq.K, pl.DIST_R))
        Ts, sts = Ts.cpu().numpy(), sts.cpu().numpy()
        assert np.array_equal(Ts, T[s - 1:s - 1 + len(k)]) and np.array_equal(sts, st[s - 1:s - 1 + len(k)])
        cums = []
        for i in range(len(k)):
            if sts[i] != -1:
                cum = np.dot(cum, Ts[i])
            cums.append(cum.copy())
        want.append(dr.dense_cloud(fe.disp[:len(k)].cpu().numpy(), seq.K, synth.BASELINE, np.stack(cums), step=4,
                                   z_max=30.0, frame_keep=(sts != -1).astype(np.int32))[0])
    want = np.concatenate(want)
    assert len(want) > 1000 and np.array_equal(dense.cloud64(), want)


# --------------------------------------------------------------------------- reprojectImageTo3D
def _rectify_q(cx=18.25, cy=9.5, f=420.0, tx=-0.12, cx2=17.0):
    """Q as cv2.stereoRectify returns it (cx, cy not on a pixel: no 0 / 0)."""
    return np.array([[1.0, 0, 0, -cx], [0, 1.0, 0, -cy], [0, 0, 0, f], [0, 0, -1.0 / tx, (cx - cx2) / tx]])


def _reproject_images():
    rng = np.random.default_rng(100)
    i16 = rng.integers(-16, 1500, size=(19, 37)).astype(np.int16)
    i16[rng.random(i16.shape) < 0.15] = -16  # the minimum, many times
    f32 = (i16.astype(np.float32) / np.float32(16)) + rng.random(i16.shape).astype(np.float32) * np.float32(1e-3)
    f32[i16 == -16] = np.float32(-1.0)
    f32[3, 5] = np.float32(-1.0) + np.float32(2.0 ** -24)  # within FLT_EPSILON of the minimum
    f32[3, 6] = np.float32(-1.0) + np.float32(2.0 ** -22)  # just outside
    return i16, f32


@pytest.mark.parametrize("handle", [False, True])
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_reproject_image_to_3d(kind, handle):
    from forest_slam_amd import cv2_compat as cv
    img = _reproject_images()[0 if kind == "int16" else 1]
    Q = _rectify_q()
    want = dr.reproject(img, Q, handle)
    got = cv.reprojectImageTo3D(img, Q, handleMissingValues=handle)
    assert got.dtype == np.float32 and got.shape == (19, 37, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    nmiss = int((want[..., 2] == 10000.0).sum())
    assert nmiss == (0 if not handle else int((img == img.min()).sum()) + (kind == "float32"))
    if handle:
        assert nmiss > 20
    # a batch of windows of a wider device buffer (pitch > width), each with its own minimum
    wide = np.zeros((3, 19, 48), img.dtype)
    wide[:, :, 5:42] = np.stack([img, img + img.dtype.type(3), img[::-1]])
    out = cv.reprojectImageTo3D(torch.from_numpy(wide).cuda()[:, :, 5:42], Q, handleMissingValues=handle)
    assert out.is_cuda and out.shape == (3, 19, 37, 3)
    for b in range(3):
        wb = dr.reproject(wide[b, :, 5:42], Q, handle)
        assert np.array_equal(out[b].cpu().numpy().view(np.uint32), wb.view(np.uint32)), b
    with pytest.raises(NotImplementedError):
        cv.reprojectImageTo3D(img, Q, ddepth=6)
    assert np.array_equal(cv.reprojectImageTo3D(img, Q, handle, cv.CV_32F), got)


def test_reproject_image_to_3d_against_cv2():
    """Guarded cross-check against OpenCV itself (the shim restates OpenCV 4.x's Matx form; cv2
    scales by the reciprocal of W where the shim divides: within one float32 ulp)."""
    cv2 = pytest.importorskip("cv2")
    from forest_slam_amd import cv2_compat as cv
    Q = _rectify_q()
    for img in _reproject_images():
        for handle in (False, True):
            got = cv.reprojectImageTo3D(img, Q, handleMissingValues=handle)
            want = cv2.reprojectImageTo3D(img, Q, handleMissingValues=handle)
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(got))
            assert np.allclose(got[fin], want[fin], rtol=2.0 ** -22, atol=0)
