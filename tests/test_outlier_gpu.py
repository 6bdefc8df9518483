"""fvo_statistical_outliers / fvo_radius_outliers / fvo_select_points and PointMap's clean-up on the
GPU, every comparison against the specification tests/outlier_ref.py: avg_distance, the neighbour
counts and the masks bit for bit; the three statistics that come from a device sum within 1e-10
relative (chains of at most 4096 non-negative terms bound the summation error near 4096 * 2^-53 ~
5e-13, and the mean's error enters the deviation sum about twice).  The mask comparison is
unconditional because no avg of any input used here lies within 1e-9 thr of thr (asserted)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import outlier_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

SENTINEL = 123.0


@functools.lru_cache(maxsize=None)
def _ctx():
    from forest_slam_amd import _lib
    return _lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_BF, kp_capacity=64)


@functools.lru_cache(maxsize=None)
def _scene(seed):
    return ref.scene(seed)[0]


@functools.lru_cache(maxsize=None)
def _stat_ref(name, k, ratio=2.0):
    """The specification's answer, computed once per (input, k) and shared; arrays are read-only."""
    keep, avg, stats = ref.statistical(_input(name), k, ratio)
    # no avg within 1e-9 thr of thr; n <= 2 cannot meet it (n = 2: both avg equal the mean, thr ==
    # mean) and does not need it: one or two equal terms, every operation of the sums is exact
    assert ref.margin_to_threshold(avg, stats[2]) > 1e-9 or len(avg) <= 2
    for a in (keep, avg, stats):
        a.setflags(write=False)
    return keep, avg, stats


@functools.lru_cache(maxsize=None)
def _input(name):
    kind, _, arg = name.partition(":")
    if kind == "scene":
        p = _scene(int(arg))
    elif kind == "lattice":
        p = ref.lattice(12, 12, 10)
    elif kind == "dup":
        p = ref.duplicates()
    elif kind == "head":  # the first n points of scene 1
        p = np.ascontiguousarray(_scene(1)[:int(arg)])
    elif kind == "rand":
        p = np.random.default_rng(int(arg)).uniform(0, 3, (int(arg), 3))
    else:
        raise KeyError(name)
    p.setflags(write=False)
    return p


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def _close(got, want):
    """stats[0..2]: 1e-10 relative, NaN where the specification has NaN (n = 1)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all((np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= 1e-10 * np.abs(want))))


def _check_statistical(name, k, cell, max_rings, ratio=2.0, **kw):
    P = _input(name)
    d = _dev(P)
    keep, avg, stats, st = _ctx().statistical_outliers(d, k, ratio, cell, max_rings, **kw)
    wkeep, wavg, wstats = _stat_ref(name, k, ratio)
    assert int(st.item()) == 0
    s = stats.cpu().numpy()
    print(f"{name} k={k} cell={cell} rings={max_rings}: stats {s.tolist()}, spec {wstats.tolist()}")
    assert np.array_equal(avg.cpu().numpy(), wavg), (name, k, cell, max_rings)
    assert np.array_equal(keep.cpu().numpy().astype(bool), wkeep)
    assert s[3] == wstats[3] and s[4] == wstats[4]
    assert _close(s[:3], wstats[:3]), (s[:3], wstats[:3])
    assert np.array_equal(d.cpu().numpy(), P)  # the input is not modified
    return s


# ------------------------------------------------------------------ statistical
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_statistical_scene(seed):
    s = _check_statistical(f"scene:{seed}", 20, 1.0, 2)
    assert 0 < s[5] < 1440  # both paths ran: the flyers' 20th neighbour is metres away


@pytest.mark.parametrize("cell,max_rings", [(0.25, 0), (1.0, 2), (4.0, 8), (100.0, 0)])
def test_statistical_does_not_depend_on_the_grid(cell, max_rings):
    """Every (cell, max_rings) gives the specification's bits, so all four agree: (0.25, 0) sends
    nearly every query to the exact pass, (100, 0) resolves every query in its own cell or not at
    all, (4, 8) walks 17^3 cells."""
    _check_statistical("scene:0", 20, cell, max_rings)


@pytest.mark.parametrize("cell", [1.0, 0.5])
@pytest.mark.parametrize("k", [7, 27])
def test_statistical_points_on_cell_faces(k, cell):
    """A 12 x 12 x 10 unit lattice: every point lies exactly on cell faces, and every k-th
    distance is tied many times over."""
    _check_statistical("lattice", k, cell, 2)


@pytest.mark.parametrize("name,k", [("rand:1", 20), ("rand:2", 20), ("rand:5", 20), ("head:255", 20), ("head:256", 20),
                                    ("head:257", 20), ("head:300", 1), ("head:300", 48), ("head:300", 49), ("head:300", 64),
                                    ("dup", 20), ("dup", 31)])
def test_statistical_edges(name, k):
    """n < k (straight to the exact pass; n = 1: std is 0/0, nothing kept), n on both sides of a
    256-thread block, k = 1 (every avg 0, everything dropped), k = 48 / 49 (128- and 64-thread blocks of
    the two searches) and k = 64 (the longest LDS columns),
    30 copies of one point (avg = 0 at k <= 30: dropped, in neither sum)."""
    s = _check_statistical(name, k, 1.0, 2)
    if k == 1:
        assert s[:3].tolist() == [0.0, 0.0, 0.0] and s[4] == 0
    if name == "rand:1":
        assert s[4] == 0 and np.isnan(s[1])


def test_statistical_status():
    """A NaN coordinate, and an extent / cell of at least 2^21: status 1 for both."""
    ctx = _ctx()
    P = _scene(0).copy()
    P[17, 1] = np.nan
    assert int(ctx.statistical_outliers(_dev(P), 20, 2.0, 1.0, 2)[3].item()) == 1
    P = _scene(0).copy()
    zmin = np.delete(P[:, 2], 17).min()
    P[17, 2] = zmin + 2.0 ** 21
    assert int(ctx.statistical_outliers(_dev(P), 20, 2.0, 1.0, 0)[3].item()) == 1
    P[17, 2] = zmin + 2.0 ** 21 - 1.0  # the last cell of the key range
    assert int(ctx.statistical_outliers(_dev(P), 20, 2.0, 1.0, 0)[3].item()) == 0
    assert int(ctx.radius_outliers(_dev(_scene(0)), 5, 1.0)[2].item()) == 0
    P[17, 0] = np.inf
    assert int(ctx.radius_outliers(_dev(P), 5, 1.0)[2].item()) == 1


def test_statistical_null_outputs_and_dirty_workspace():
    """status = NULL and avg_distance = NULL are accepted; one workspace filled with 0xFF serves two
    different clouds in turn, and nothing is written past its stated size."""
    from forest_slam_amd import _lib
    ctx = _ctx()
    wb = ctx.outlier_workspace_bytes(1440, 20)
    guard = 256
    ws = torch.full((wb + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    for name in ("scene:2", "head:257", "scene:2"):
        P = _input(name)
        n = len(P)
        d = _dev(P)
        keep = torch.full((n + 8,), 77, dtype=torch.uint8, device="cuda")
        stats = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
        rc = ctx.L.fvo_statistical_outliers(ctx.h, _lib._ptr(d), n, 20, 2.0, 1.0, 2, _lib._ptr(ws), wb, _lib._ptr(keep),
                                            None, _lib._ptr(stats), None, _lib._stream(ctx.device))
        assert rc == 0
        torch.cuda.synchronize()
        wkeep, _, wstats = _stat_ref(name, 20)
        k = keep.cpu().numpy()
        assert np.array_equal(k[:n].astype(bool), wkeep) and (k[n:] == 77).all()
        s = stats.cpu().numpy()
        assert _close(s[:3], wstats[:3]) and s[3] == n and s[4] == wstats[4] and (s[6:] == SENTINEL).all()
        assert (ws[wb:].cpu().numpy() == 0xFF).all()
        assert np.array_equal(d.cpu().numpy(), P)


def test_statistical_repeats_bit_for_bit():
    """The sums are deterministic: two calls give the same six statistics, bit for bit."""
    d = _dev(_scene(1))
    a = _ctx().statistical_outliers(d, 20, 2.0, 1.0, 2)[2].cpu().numpy()
    b = _ctx().statistical_outliers(d, 20, 2.0, 1.0, 2)[2].cpu().numpy()
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ radius
@functools.lru_cache(maxsize=None)
def _radius_ref(name, r):
    count = ref.radius(_input(name), 0, r)[1]
    count.setflags(write=False)
    return count


@pytest.mark.parametrize("name,r", [("lattice", 1.0), ("lattice", 1.5), ("scene:0", 1.0)])
@pytest.mark.parametrize("div", [1, 4])
def test_radius(name, r, div):
    """cell = radius and radius / 4; nb_points 0, 5 and n.  On the lattice at radius 1.0 the six
    face neighbours sit at exactly d2 == r2 and do not count."""
    P = _input(name)
    d = _dev(P)
    want = _radius_ref(name, r)
    for nb in (0, 5, len(P)):
        keep, cnt, st = _ctx().radius_outliers(d, nb, r, cell=r / div)
        assert int(st.item()) == 0
        assert np.array_equal(cnt.cpu().numpy(), want), (name, r, div)
        assert np.array_equal(keep.cpu().numpy().astype(bool), want > nb)
    if name == "lattice" and r == 1.0:
        assert (want == 1).all()
    keep, cnt, st = _ctx().radius_outliers(d, 5, r, cell=r / div, n_neighbors=False, status=False)
    assert cnt is None and st is None and np.array_equal(keep.cpu().numpy().astype(bool), want > 5)
    assert np.array_equal(d.cpu().numpy(), P)


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize("n", [1, 257, 1440])
@pytest.mark.parametrize("mask", ["random", "all", "none"])
def test_select_points(n, mask):
    """Against NumPy boolean indexing: each output alone and both together; nothing is written
    past n_out.  The mask holds values other than 1 too (any non-zero byte keeps), and starts at
    an odd address for one of the calls."""
    ctx = _ctx()
    P = np.ascontiguousarray(_scene(0)[:n])
    rng = np.random.default_rng(n)
    m = {"random": rng.integers(0, 3, n) * rng.integers(1, 128, n), "all": np.full(n, 255), "none": np.zeros(n)}[mask]
    m = m.astype(np.uint8)
    want = P[m != 0]
    d = _dev(P)
    buf = torch.zeros((n + 1,), dtype=torch.uint8, device="cuda")
    buf[1:] = _dev(m)
    for km in (_dev(m), buf[1:]):
        for use64, use32 in ((True, True), (True, False), (False, True)):
            o64 = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda") if use64 else None
            o32 = torch.full((n, 3), SENTINEL, dtype=torch.float32, device="cuda") if use32 else None
            cnt = torch.full((3,), -99, dtype=torch.int32, device="cuda")
            ctx.select_points(d, km, o64, o32, cnt[1:2])
            c = cnt.cpu().numpy()
            assert c.tolist() == [-99, len(want), -99]
            if use64:
                g = o64.cpu().numpy()
                assert np.array_equal(g[:len(want)], want) and (g[len(want):] == SENTINEL).all()
            if use32:
                g = o32.cpu().numpy()
                assert np.array_equal(g[:len(want)], want.astype(np.float32)) and (g[len(want):] == SENTINEL).all()
    assert np.array_equal(d.cpu().numpy(), P)


def test_empty_cloud():
    ctx = _ctx()
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    keep, avg, stats, st = ctx.statistical_outliers(e)
    assert keep.numel() == 0 and not stats.cpu().numpy().any() and int(st.item()) == 0
    keep, cnt, st = ctx.radius_outliers(e, 5, 1.0)
    assert keep.numel() == 0 and int(st.item()) == 0
    _, _, n = ctx.select_points(e, torch.zeros((0,), dtype=torch.uint8, device="cuda"))
    assert int(n.item()) == 0


def test_refusals_reach_python():
    ctx = _ctx()
    d = _dev(_scene(0))
    with pytest.raises(RuntimeError, match="std_ratio must be finite"):
        ctx.statistical_outliers(d, 20, float("inf"))
    with pytest.raises(RuntimeError, match=r"max_rings must be in \[0, 8\]"):
        ctx.statistical_outliers(d, 20, 2.0, 1.0, 9)
    with pytest.raises(RuntimeError, match="radius / cell must be <= 8"):
        ctx.radius_outliers(d, 5, 1.0, cell=0.1)
    with pytest.raises(RuntimeError, match="out64 overlaps points"):
        ctx.select_points(d, torch.ones((1440,), dtype=torch.uint8, device="cuda"), out64=d)
    with pytest.raises(ValueError):
        ctx.outlier_workspace_bytes(1440, 65)


# ------------------------------------------------------------------ PointMap
def test_point_map_clean_up():
    """A map built with add_frames (identity poses: the points are float32 values, exact in fp64);
    remove_statistical_outlier then remove_radius_outlier leave cloud64() equal to the
    specification applied in turn, cloud32() its float32 cast; len() and the indices match."""
    from forest_slam_amd.mapping import PointMap
    P32 = _scene(0).astype(np.float32)
    pm = PointMap(2000)
    for part in (P32[:700], P32[700:]):
        pm.add_frames(_dev(part[None]), torch.tensor([len(part)], dtype=torch.int32, device="cuda"), np.eye(4)[None])
    P = P32.astype(np.float64)
    assert np.array_equal(pm.cloud64(), P)
    k1, avg, stats = ref.statistical(P, 20, 2.0)
    assert ref.margin_to_threshold(avg, stats[2]) > 1e-9
    ind = pm.remove_statistical_outlier(20, 2.0, cell=1.0)
    assert ind.dtype == torch.int64 and np.array_equal(ind.cpu().numpy(), np.flatnonzero(k1))
    Q = P[k1]
    assert len(pm) == len(Q) and np.array_equal(pm.cloud64(), Q) and np.array_equal(pm.cloud32(), Q.astype(np.float32))
    k2, _ = ref.radius(Q, 8, 0.8)
    assert 0 < k2.sum() < len(Q)
    ind = pm.remove_radius_outlier(8, 0.8)
    assert np.array_equal(ind.cpu().numpy(), np.flatnonzero(k2))
    assert len(pm) == k2.sum() and np.array_equal(pm.cloud64(), Q[k2])
    assert np.array_equal(pm.cloud32(), Q[k2].astype(np.float32))
    # rows past the count are untouched history, never read: the map keeps appending after them
    pm.add_frames(_dev(P32[None, :5]), torch.tensor([5], dtype=torch.int32, device="cuda"), np.eye(4)[None])
    assert len(pm) == k2.sum() + 5 and np.array_equal(pm.cloud64()[-5:], P[:5])


def test_point_map_status_raises():
    from forest_slam_amd.mapping import PointMap
    pm = PointMap(16)
    P = np.zeros((1, 3, 3), np.float32)
    P[0, 1, 0] = 3.0e6  # extent / cell >= 2^21 at cell 1
    pm.add_frames(_dev(P), torch.tensor([3], dtype=torch.int32, device="cuda"), np.eye(4)[None])
    with pytest.raises(RuntimeError, match="21-bit"):
        pm.remove_statistical_outlier(2, 2.0, cell=1.0)
    with pytest.raises(RuntimeError, match="21-bit"):
        pm.remove_radius_outlier(1, 1.0)
    assert len(pm) == 3
