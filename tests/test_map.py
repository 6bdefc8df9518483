"""Map accumulation: the per-frame map update of stereo_slam.py:308-318
(cum @ [P; 1], PointCloud2 FLOAT32 packing) and mono_slam.py:144-164 / gt_mapping.py:62-66
(Open3D voxel_down_sample(0.5)).  Open3D is not installed here: the oracle (oracle/map_ref.cpp)
restates VoxelDownSample and is checked against an independent NumPy/dict restatement of the
same algorithm ("parity unpinned" against Open3D itself; its output order, an unordered_map's,
is unspecified, so voxels are compared in index order).  CPU: oracle vs NumPy.  GPU: the HIP
kernels bit-exact against the oracle."""
import functools

import numpy as np
import pytest
import torch

from conftest import gpu_available


def _cloud(n, seed, spread=20.0):
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, 3)) * spread
    P[: n // 4] = np.round(P[: n // 4] * 2) / 2  # points exactly on voxel boundaries
    return P.astype(np.float32)


def _pose(seed):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-np.pi, np.pi, 2)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Rx
    T[:3, 3] = rng.uniform(-50, 50, 3)
    return T


def _voxel_numpy(P, v):
    """Open3D 0.17 VoxelDownSample restated with a dict (insertion-order sums)."""
    vmin = P.min(axis=0) - v * 0.5
    acc = {}
    for p in P:
        key = tuple(int(np.floor(c)) for c in (p - vmin) / v)
        s = acc.setdefault(key, [0.0, 0.0, 0.0, 0])
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += 1
    return np.array([[s[0] / s[3], s[1] / s[3], s[2] / s[3]] for _, s in sorted(acc.items())]).reshape(-1, 3)


def test_map_transform_oracle_matches_numpy(oracle_mod):
    P, T = _cloud(5000, 1), _pose(2)
    o64, o32 = oracle_mod.map_transform(P, T)
    ref = (T @ np.hstack((P, np.ones((len(P), 1)))).T)[:3].T  # stereo_slam.py:308-311
    assert np.allclose(o64, ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    assert np.mean(o32 == ref.astype(np.float32)) > 0.999


@pytest.mark.parametrize("v", [0.5, 0.3])
def test_voxel_oracle_matches_numpy(oracle_mod, v):
    P = _cloud(3000, 3, spread=3.0).astype(np.float64)
    assert np.array_equal(oracle_mod.voxel_down_sample(P, v), _voxel_numpy(P, v))


def test_voxel_oracle_known_answers(oracle_mod):
    assert oracle_mod.voxel_down_sample(np.zeros((0, 3)), 0.5).shape == (0, 3)
    one = np.array([[1.25, -3.0, 7.5]])
    assert np.array_equal(oracle_mod.voxel_down_sample(one, 0.5), one)
    # min bound - v/2 puts the minimum point at the centre of voxel 0: these two share it
    two = np.array([[0.0, 0.0, 0.0], [0.2, 0.1, -0.1]])
    assert np.array_equal(oracle_mod.voxel_down_sample(two, 0.5), [[0.1, 0.05, -0.05]])


@functools.lru_cache(maxsize=None)
def _ctx():
    from forest_slam_amd import _lib
    return _lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_BF, kp_capacity=64)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_map_transform_matches_oracle(oracle_mod):
    ctx = _ctx()
    B, cap = 5, 1200
    counts = [1000, 0, 1200, 37, 999]
    P = np.zeros((B, cap, 3), np.float32)
    for b in range(B):
        P[b] = _cloud(cap, 10 + b)
    T = np.stack([_pose(20 + b) for b in range(B)])
    M = sum(counts) + 100
    m64 = torch.zeros((M, 3), dtype=torch.float64, device="cuda")
    m32 = torch.zeros((M, 3), dtype=torch.float32, device="cuda")
    cnt = torch.tensor([100], dtype=torch.int32, device="cuda")  # append after 100 existing points
    ctx.map_transform(torch.from_numpy(P).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda"),
                      torch.from_numpy(T).cuda(), cnt, m64, m32)
    assert int(cnt.item()) == M
    g64, g32 = m64.cpu().numpy(), m32.cpu().numpy()
    assert not g64[:100].any()
    o = 100
    for b in range(B):
        w64, w32 = oracle_mod.map_transform(P[b, :counts[b]], T[b])
        assert np.array_equal(g64[o:o + counts[b]], w64) and np.array_equal(g32[o:o + counts[b]], w32), b
        o += counts[b]
    # overflow: points past map_cap are dropped, the count still advances
    small = torch.zeros((50, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ctx.map_transform(torch.from_numpy(P[:1]).cuda(), torch.tensor([1000], dtype=torch.int32, device="cuda"),
                      torch.from_numpy(T[:1]).cuda(), cnt, None, small)
    assert int(cnt.item()) == 1000
    assert np.array_equal(small.cpu().numpy(), oracle_mod.map_transform(P[0, :50], T[0])[1])


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_voxel_down_sample_matches_oracle(oracle_mod):
    ctx = _ctx()
    cases = [_cloud(200_000, 5).astype(np.float64), _cloud(3000, 6, spread=0.05).astype(np.float64),
             np.array([[1.0, 2.0, 3.0]]), np.repeat([[0.3, 0.3, 0.3]], 700, axis=0)]
    # a transformed lidar-like map (mono_slam.py:148-155)
    o64, _ = oracle_mod.map_transform(_cloud(50_000, 7, spread=30.0), _pose(8))
    cases.append(o64)
    for v in (0.5, 0.1):
        for P in cases:
            out, n, st = ctx.voxel_down_sample(torch.from_numpy(P).cuda(), v)
            want = oracle_mod.voxel_down_sample(P, v)
            assert int(st.item()) == 0
            assert int(n.item()) == len(want), (len(P), v)
            assert np.array_equal(out[:len(want)].cpu().numpy(), want), (len(P), v)
    out, n, st = ctx.voxel_down_sample(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), 0.5)
    assert int(n.item()) == 0


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_point_map_mono_update_matches_oracle(oracle_mod):
    """mono_slam.py:144-164: cloud -> pose -> voxel_down_sample(0.5) -> appended to the map."""
    from forest_slam_amd.mapping import PointMap
    pm = PointMap(100_000)
    want = []
    for k in range(3):
        cloud, T = _cloud(20_000, 40 + k, spread=10.0), _pose(50 + k)
        pm.add_cloud(cloud, T, 0.5)
        o64, _ = oracle_mod.map_transform(cloud, T)
        want.append(oracle_mod.voxel_down_sample(o64, 0.5))
    want = np.concatenate(want)
    assert np.array_equal(pm.cloud64(), want)
    assert np.array_equal(pm.cloud32(), want.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_point_map_overflow_is_reported():
    """an append past the capacity is surfaced (check=True raises at once,
    overflowed() / len() report it) instead of silently dropping later batches."""
    from forest_slam_amd.mapping import PointMap
    pm = PointMap(capacity=100, device="cuda:0")
    P = torch.from_numpy(_cloud(80, 3)).cuda().reshape(1, 80, 3)
    T = np.eye(4)[None]
    pm.add_frames(P, torch.tensor([80], dtype=torch.int32, device="cuda"), T, check=True)
    assert len(pm) == 80 and not pm.overflowed()
    with pytest.raises(RuntimeError, match="overflow"):
        pm.add_frames(P, torch.tensor([80], dtype=torch.int32, device="cuda"), T, check=True)
    assert pm.overflowed()


def _chain_ref(T, S, N, cum0):
    """stereo_slam.py:292-306 restated per sequence: cum = cum @ T for posed frames
    (status >= 0), summed over k ascending without contraction (fvo_chain_poses' order)."""
    cum = cum0.copy()
    out = np.zeros_like(T)
    nout = np.zeros_like(N)
    for s in range(T.shape[0]):
        c = cum[s]
        for f in range(T.shape[1]):
            if S[s, f] >= 0:
                t = T[s, f]
                c = np.array([[((c[i, 0] * t[0, j] + c[i, 1] * t[1, j]) + c[i, 2] * t[2, j]) + c[i, 3] * t[3, j]
                               for j in range(4)] for i in range(4)])
                nout[s, f] = N[s, f]
            out[s, f] = c
        cum[s] = c
    return out, nout, cum


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_chain_poses_matches_reference_chain():
    """fvo_chain_poses (the multi-sequence map's placing poses on the device): per sequence
    cum = cum @ T for every posed frame (status >= 0; -1 = the < 6 points skip, -2 padding, -3
    overflow leave it unchanged), carried across calls; equal to the ascending-k restatement bit
    for bit and to eval.chain's np.dot chain within 1e-12; points of unposed frames zeroed."""
    from forest_slam_amd import _lib
    from forest_slam_amd import eval as ev
    rng = np.random.default_rng(9)
    S_, n = 5, 7
    T = np.stack([[_pose(100 * s + f) for f in range(2 * n)] for s in range(S_)])
    T[..., :3, 3] *= 0.01
    St = rng.choice([1, 1, 1, 0, -1, -2, -3], size=(S_, 2 * n)).astype(np.int32)
    N = rng.integers(0, 900, size=(S_, 2 * n)).astype(np.int32)
    ctx = _lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_BF, kp_capacity=64, device="cuda:0")
    cum = torch.eye(4, dtype=torch.float64, device="cuda:0").repeat(S_, 1, 1).contiguous()
    ref_cum = np.tile(np.eye(4), (S_, 1, 1))
    for h in range(2):  # two calls: the chain carries over
        sl = slice(h * n, (h + 1) * n)
        dT = torch.from_numpy(np.ascontiguousarray(T[:, sl])).cuda()
        got, gn = ctx.chain_poses(dT, torch.from_numpy(np.ascontiguousarray(St[:, sl])).cuda(), cum,
                                  n_points=torch.from_numpy(np.ascontiguousarray(N[:, sl])).cuda())
        want, wn, ref_cum = _chain_ref(T[:, sl], St[:, sl], N[:, sl], ref_cum)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(gn.cpu().numpy(), wn)
    assert np.array_equal(cum.cpu().numpy(), ref_cum)
    for s in range(S_):
        posed = St[s] >= 0
        assert np.allclose(ev.chain(T[s], posed)[-1], ref_cum[s], rtol=0, atol=1e-12)


# ------------------------------------------------------------------ off the default layout
# fvo_map_transform with record strides, many sets, the capacity edge, the count clamps;
# fvo_chain_poses over every block shape; fvo_voxel_down_sample at the edge of its key range,
# without a status word and in a dirty workspace.  Bit for bit against the oracle.
SENTINEL = 123.0
INT32_MAX = 2 ** 31 - 1


def _map_transform_raw(ctx, P, n, T, cnt, map_cap, m64=None, m32=None):
    """fvo_map_transform with map_cap of the caller's choice (Context.map_transform passes the
    tensors' rows)."""
    from forest_slam_amd import _lib
    B, cap, st = P.shape
    ctx._check(ctx.L.fvo_map_transform(ctx.h, _lib._ptr(P), st, _lib._ptr(n), B, cap, _lib._ptr(T), _lib._ptr(cnt),
                                       map_cap, _lib._ptr(m64), _lib._ptr(m32), _lib._stream(ctx.device)))


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _map(rows, dtype):
    return torch.full((rows, 3), SENTINEL, dtype=dtype, device="cuda")


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
@pytest.mark.parametrize("stride", [4, 7])
def test_gpu_map_transform_record_stride(oracle_mod, stride):
    """The [cap][4] stereo records (and a wider record): floats past xyz are NaN and must not be
    read; once with only the fp64 map and once with only the PointCloud2 float32 map."""
    ctx = _ctx()
    B, cap, counts = 2, 300, [300, 257]
    P = np.full((B, cap, stride), np.nan, np.float32)
    for b in range(B):
        P[b, :, :3] = _cloud(cap, 60 + b)
    T = np.stack([_pose(70 + b) for b in range(B)])
    want = [oracle_mod.map_transform(P[b, :counts[b]], T[b]) for b in range(B)]
    for k, dtype in enumerate((torch.float64, torch.float32)):
        m = _map(sum(counts) + 3 + 4, dtype)
        cnt = _i32([3])
        ctx.map_transform(torch.from_numpy(P).cuda(), _i32(counts), torch.from_numpy(T).cuda(), cnt,
                          m if k == 0 else None, m if k == 1 else None)
        got = m.cpu().numpy()
        assert int(cnt.item()) == 3 + sum(counts)
        o = 3
        for b in range(B):
            assert np.array_equal(got[o:o + counts[b]], want[b][k]), (stride, k, b)
            o += counts[b]
        assert (got[:3] == SENTINEL).all() and (got[o:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_map_transform_many_sets(oracle_mod):
    """130 sets: three trips of the 64-lane loop that sums the counts before a set; a count above
    cap is clamped; every set lands at the prefix sum of the clamped counts after *map_count = 7."""
    ctx = _ctx()
    B, cap, first = 130, 3, 7
    counts = [(0, 1, 3, 5)[b % 4] for b in range(B)]
    used = [min(c, cap) for c in counts]
    P = _cloud(B * cap, 80).reshape(B, cap, 3)
    T = np.stack([_pose(1000 + b) for b in range(B)])
    rows = first + sum(used) + 5
    m64, m32, cnt = _map(rows, torch.float64), _map(rows, torch.float32), _i32([first])
    ctx.map_transform(torch.from_numpy(P).cuda(), _i32(counts), torch.from_numpy(T).cuda(), cnt, m64, m32)
    assert int(cnt.item()) == first + sum(used)
    g64, g32 = m64.cpu().numpy(), m32.cpu().numpy()
    o = first
    for b in range(B):
        w64, w32 = oracle_mod.map_transform(P[b, :used[b]], T[b])
        assert np.array_equal(g64[o:o + used[b]], w64) and np.array_equal(g32[o:o + used[b]], w32), b
        o += used[b]
    for g in (g64, g32):
        assert (g[:first] == SENTINEL).all() and (g[o:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_map_transform_capacity_inside_a_block(oracle_mod):
    """map_cap falls inside a set and inside a 256-thread block: rows below it are written, guard
    rows above it keep their sentinel, *map_count advances by the whole set."""
    ctx = _ctx()
    n, first = 600, 5
    map_cap = 300 + first
    P, T = _cloud(n, 81)[None], _pose(82)[None]
    m64, m32, cnt = _map(n + 100, torch.float64), _map(n + 100, torch.float32), _i32([first])
    _map_transform_raw(ctx, torch.from_numpy(P).cuda(), _i32([n]), torch.from_numpy(T).cuda(), cnt, map_cap, m64, m32)
    assert int(cnt.item()) == first + n
    w64, w32 = oracle_mod.map_transform(P[0, :map_cap - first], T[0])
    for g, w in ((m64.cpu().numpy(), w64), (m32.cpu().numpy(), w32)):
        assert np.array_equal(g[first:map_cap], w)
        assert (g[:first] == SENTINEL).all() and (g[map_cap:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_map_transform_count_saturates():
    """*map_count = INT32_MAX - 10 and a set of 100 points: the count stops at INT32_MAX; with
    map_cap = 0 nothing is written through the (non-null) map pointers."""
    ctx = _ctx()
    P, T = _cloud(100, 83)[None], _pose(84)[None]
    m64, m32, cnt = _map(16, torch.float64), _map(16, torch.float32), _i32([INT32_MAX - 10])
    _map_transform_raw(ctx, torch.from_numpy(P).cuda(), _i32([100]), torch.from_numpy(T).cuda(), cnt, 0, m64, m32)
    assert int(cnt.item()) == INT32_MAX
    assert (m64.cpu().numpy() == SENTINEL).all() and (m32.cpu().numpy() == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_map_transform_negative_count_is_empty(oracle_mod):
    """n_points[b] < 0 counts as 0 (include/fvo.h): counts [4, -7, 3] append 7 points and advance
    the count by 7.  Before the clamp the third set started 7 rows early, over the map's earlier
    points, and the count moved by 0.  (*map_count starts at 10, so that those rows exist.)"""
    ctx = _ctx()
    cap, first, counts = 8, 10, [4, -7, 3]
    P = _cloud(3 * cap, 85).reshape(3, cap, 3)
    T = np.stack([_pose(86 + b) for b in range(3)])
    m64, m32, cnt = _map(32, torch.float64), _map(32, torch.float32), _i32([first])
    ctx.map_transform(torch.from_numpy(P).cuda(), _i32(counts), torch.from_numpy(T).cuda(), cnt, m64, m32)
    assert int(cnt.item()) == first + 7
    a64, a32 = oracle_mod.map_transform(P[0, :4], T[0])
    c64, c32 = oracle_mod.map_transform(P[2, :3], T[2])
    for g, a, c in ((m64.cpu().numpy(), a64, c64), (m32.cpu().numpy(), a32, c32)):
        assert (g[:first] == SENTINEL).all() and (g[first + 7:] == SENTINEL).all()
        assert np.array_equal(g[first:first + 4], a) and np.array_equal(g[first + 4:first + 7], c)


def _chain_longdouble(T, S, cum0):
    cum = cum0.astype(np.longdouble)
    out = np.zeros(T.shape, np.longdouble)
    for s in range(T.shape[0]):
        for f in range(T.shape[1]):
            if S[s, f] >= 0:
                cum[s] = cum[s] @ T[s, f].astype(np.longdouble)
            out[s, f] = cum[s]
    return out, cum


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("n_seq", [1, 3, 4, 5, 9])
def test_gpu_chain_poses_shapes(n_seq, n):
    """Fewer sequences than a wave holds, exactly one wave's four, one more, three blocks; from a
    non-identity cum_state.  First call with n_points; second call without, and with sequence 0
    unposed throughout: its cum_state stays bit-identical and is repeated in cum_out."""
    rng = np.random.default_rng(100 * n_seq + n)
    ctx = _ctx()
    T = np.stack([[_pose(500 * s + f + n) for f in range(2 * n)] for s in range(n_seq)])
    T[..., :3, 3] *= 0.01
    St = rng.choice([1, 1, 1, 0, -1, -2, -3], size=(n_seq, 2 * n)).astype(np.int32)
    St[:, 0] = 1  # every sequence moves in the first call
    St[0, n:] = rng.choice([-1, -2, -3], size=n)
    N = rng.integers(0, 900, size=(n_seq, 2 * n)).astype(np.int32)
    cum0 = np.stack([_pose(900 + s) for s in range(n_seq)])
    cum0[:, :3, 3] *= 0.01
    cum = torch.from_numpy(cum0.copy()).cuda()
    ref_cum, ld_cum = cum0.copy(), cum0.copy()
    for h in range(2):
        sl = slice(h * n, (h + 1) * n)
        Th, Sh, Nh = (np.ascontiguousarray(a[:, sl]) for a in (T, St, N))
        before = ref_cum.copy()
        got, gn = ctx.chain_poses(torch.from_numpy(Th).cuda(), torch.from_numpy(Sh).cuda(), cum,
                                  n_points=torch.from_numpy(Nh).cuda() if h == 0 else None)
        want, wn, ref_cum = _chain_ref(Th, Sh, Nh, ref_cum)
        ld, ld_cum = _chain_longdouble(Th, Sh, ld_cum)
        got = got.cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(cum.cpu().numpy(), ref_cum)
        assert np.abs(got - ld).max() <= 1e-12
        if h == 0:
            assert np.array_equal(gn.cpu().numpy(), wn)
            assert not np.array_equal(ref_cum, before)
        else:
            assert gn is None
            assert np.array_equal(ref_cum[0], before[0]) and all(np.array_equal(got[0, f], before[0]) for f in range(n))


VOX = 0.5
VOX_FAR = VOX * (2 ** 21 - 1)  # the last voxel index of the 21-bit key
VOX_PAST = VOX * 2 ** 21 + 1


def _voxel_points(axis, far):
    P = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.1, 0.2, 0.3]])
    P[1, axis] = far
    return P


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gpu_voxel_key_range(oracle_mod, axis):
    """A point in the last voxel of the 21-bit key range is fine (status 0, the oracle's three
    voxels); one past it reports status 1."""
    ctx = _ctx()
    P = _voxel_points(axis, VOX_FAR)
    want = oracle_mod.voxel_down_sample(P, VOX)
    assert len(want) == 3
    out, n, st = ctx.voxel_down_sample(torch.from_numpy(P).cuda(), VOX)
    assert int(st.item()) == 0 and int(n.item()) == 3
    assert np.array_equal(out[:3].cpu().numpy(), want)
    out, n, st = ctx.voxel_down_sample(torch.from_numpy(_voxel_points(axis, VOX_PAST)).cuda(), VOX)
    assert int(st.item()) == 1


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_voxel_without_status(oracle_mod):
    """status = NULL: the valid input gives the same out and n_out; the overflowing input returns 0
    and writes nothing outside out[0:n], *n_out and the workspace."""
    import ctypes
    from forest_slam_amd import _lib
    ctx = _ctx()
    n = 3
    wb = int(ctx.L.fvo_voxel_workspace_bytes(n))
    assert wb > 0
    guard = 256
    for far, want in ((VOX_FAR, oracle_mod.voxel_down_sample(_voxel_points(0, VOX_FAR), VOX)), (VOX_PAST, None)):
        P = torch.from_numpy(_voxel_points(0, far)).cuda()
        ws = torch.full((wb + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.full((n + 4, 3), SENTINEL, dtype=torch.float64, device="cuda")
        cnt = torch.full((3,), -99, dtype=torch.int32, device="cuda")  # n_out is the middle word
        rc = ctx.L.fvo_voxel_down_sample(ctx.h, _lib._ptr(P), n, VOX, _lib._ptr(ws), wb, _lib._ptr(out),
                                         ctypes.c_void_p(cnt.data_ptr() + 4), None, _lib._stream(ctx.device))
        assert rc == 0
        torch.cuda.synchronize()
        c, o = cnt.cpu().numpy(), out.cpu().numpy()
        assert c[0] == -99 and c[2] == -99 and 1 <= c[1] <= n
        assert (o[n:] == SENTINEL).all()
        assert (ws[wb:].cpu().numpy() == 0xA5).all()
        assert np.array_equal(P.cpu().numpy(), _voxel_points(0, far))
        if want is not None:
            assert c[1] == len(want) and np.array_equal(o[:len(want)], want)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_voxel_dirty_workspace_and_block_edges(oracle_mod):
    """One workspace sized for 5000 points, filled with 0xFF, used for 5000 points and then for
    257: nothing may depend on what the workspace held.  Then n on both sides of one 256-thread
    block."""
    ctx = _ctx()
    ws = torch.full((int(ctx.L.fvo_voxel_workspace_bytes(5000)),), 0xFF, dtype=torch.uint8, device="cuda")
    for P in (_cloud(5000, 90, spread=3.0).astype(np.float64), _cloud(257, 91, spread=1.0).astype(np.float64)):
        out, n, st = ctx.voxel_down_sample(torch.from_numpy(P).cuda(), VOX, workspace=ws)
        want = oracle_mod.voxel_down_sample(P, VOX)
        assert int(st.item()) == 0 and int(n.item()) == len(want)
        assert np.array_equal(out[:len(want)].cpu().numpy(), want), len(P)
    for k in (255, 256, 257):
        P = _cloud(k, 92 + k, spread=1.0).astype(np.float64)
        out, n, st = ctx.voxel_down_sample(torch.from_numpy(P).cuda(), VOX)
        want = oracle_mod.voxel_down_sample(P, VOX)
        assert int(st.item()) == 0 and int(n.item()) == len(want)
        assert np.array_equal(out[:len(want)].cpu().numpy(), want), k
