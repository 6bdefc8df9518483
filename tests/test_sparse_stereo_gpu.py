"""Sparse stereo on the GPU (csrc/sparse_stereo.hip: fvo_sparse_stereo, fvo_backproject_stereo and
StereoFrontEnd(depth="sparse")), bit-exact against the specification tests/sparse_stereo_ref.py:
the float32 expressions are evaluated in the specification's order and the SADs are integers, so
`stereo` and `info` are compared as bit patterns."""
import functools

import numpy as np
import pytest

import sparse_stereo_cases as cases
import sparse_stereo_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

STEREO_FILL, INFO_FILL, IMG_FILL = -77.5, -99, 0xA5
LEVELS = ref.level_scales()


@functools.lru_cache(maxsize=None)
def _ctx(W, H, max_batch, cap):
    from forest_slam_amd import _lib
    return _lib.Context(W, H, max_batch=max_batch, stages=_lib.STAGE_BF, kp_capacity=cap)


def _run(items, K, baseline, params, cap, counts=None, pitch=None, gap_rows=0, with_info=True,
         size=(cases.W, cases.H)):
    """One fvo_sparse_stereo call on `items` (a batch).  counts: (nL, nR) per item when they differ
    from the sets' sizes.  pitch: bytes between rows (default W); gap_rows: unused rows between one
    image's last row and the next image (image_stride = (H + gap_rows) * pitch).  Every buffer is
    pre-filled, the inputs are compared before and after the call, and the padding of pitched
    images must keep its fill.  Returns (stereo, info) as NumPy
    arrays [B, cap, 4] (info None without with_info)."""
    import torch
    W, H = size
    B = len(items)
    ctx = _ctx(W, H, max(B, 1), cap)
    pitch = pitch or W
    rng = np.random.default_rng(B * 131 + cap)
    imgL = np.full((B, H + gap_rows, pitch), IMG_FILL, np.uint8)
    imgR = np.full((B, H + gap_rows, pitch), IMG_FILL, np.uint8)
    kpL = rng.uniform(0, 90, (B, cap, 8)).astype(np.float32)  # rows past the counts hold plausible keypoints
    kpR = rng.uniform(0, 90, (B, cap, 8)).astype(np.float32)
    kpL[..., 5] = kpR[..., 5] = 0
    descL = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    descR = descL.copy()
    nL, nR = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, it in enumerate(items):
        imgL[b, :H, :W], imgR[b, :H, :W] = it["imgL"], it["imgR"]
        l, r = min(len(it["kpL"]), cap), min(len(it["kpR"]), cap)
        kpL[b, :l], descL[b, :l] = it["kpL"][:l], it["descL"][:l]
        kpR[b, :r], descR[b, :r] = it["kpR"][:r], it["descR"][:r]
        nL[b], nR[b] = (len(it["kpL"]), len(it["kpR"])) if counts is None else counts[b]
    host = (imgL, imgR, kpL, kpR, descL, descR, nL, nR)
    dev = [torch.from_numpy(a).cuda() for a in host]
    stereo = torch.full((B, cap, 4), STEREO_FILL, dtype=torch.float32, device="cuda")
    info = torch.full((B, cap, 4), INFO_FILL, dtype=torch.int32, device="cuda") if with_info else None
    ws = torch.full((ctx.sparse_stereo_workspace_bytes(B, cap) + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    ctx.sparse_stereo(dev[0][:, :H, :W], dev[1][:, :H, :W], dev[2], dev[6], dev[4], dev[3], dev[7], dev[5], K, baseline,
                      params=params, level_scale=LEVELS, workspace=ws, out=stereo, info=info)
    torch.cuda.synchronize()
    for a, d in zip(host, dev):
        assert a.tobytes() == d.cpu().numpy().tobytes(), "an input buffer changed"  # (bytes: the keypoints hold NaNs)
    assert (ws[-64:] == 0x3C).all(), "written past the workspace"
    return stereo.cpu().numpy(), (info.cpu().numpy() if with_info else None)


def _check(items, stereo, info, K, baseline, params, cap, counts=None):
    """Rows below the (clamped) left count equal the specification bit for bit; the rest keep their fill."""
    for b, it in enumerate(items):
        nl, nr = (len(it["kpL"]), len(it["kpR"])) if counts is None else counts[b]
        nl, nr = min(max(nl, 0), cap), min(max(nr, 0), cap)
        want_s, want_i = ref.sparse_stereo(it["imgL"], it["imgR"], it["kpL"][:nl], it["descL"][:nl], it["kpR"][:nr],
                                           it["descR"][:nr], K, baseline, ref.Params(**params), LEVELS)
        assert np.array_equal(stereo[b, :nl].view(np.uint32), want_s.view(np.uint32)), f"item {b}: stereo differs"
        assert (stereo[b, nl:] == np.float32(STEREO_FILL)).all(), f"item {b}: stereo rows past the count written"
        if info is not None:
            bad = np.nonzero((info[b, :nl] != want_i).any(1))[0]
            assert len(bad) == 0, f"item {b}: info differs at {bad[:5]}: {info[b, bad[:5]]} vs {want_i[bad[:5]]}"
            assert (info[b, nl:] == INFO_FILL).all(), f"item {b}: info rows past the count written"


# ------------------------------------------------------------------ hand-built sets
N_LEFT, N_RIGHT = (0, 1, 63, 64, 65, 257), (1, 255, 256, 257, 513)  # across the tile edges of both kernels
SET_CAP = 520


def _count_sets():
    return [cases.random_set(nl, nr, 1000 * nl + nr) for nl in N_LEFT for nr in N_RIGHT]


@pytest.mark.parametrize("unique", [0, 1])
@pytest.mark.parametrize("w,S", [(1, 1), (5, 5), (7, 8)])
def test_count_sets(w, S, unique):
    """Thirty sets in one batch: every left count with every right count, each window / slide
    size, with and without the uniqueness pass."""
    params = dict(cases.SET_PARAMS, half_window=w, half_slide=S, unique=unique)
    items = _count_sets()
    stereo, info = _run(items, cases.SET_K, cases.SET_BASELINE, params, SET_CAP)
    _check(items, stereo, info, cases.SET_K, cases.SET_BASELINE, params, SET_CAP)
    if (w, S, unique) == (5, 5, 1):  # the sets exercise every status
        seen = set()
        for b, it in enumerate(items):
            seen |= set(info[b, :len(it["kpL"]), 3].tolist())
        assert seen == set(range(7))


@pytest.mark.parametrize("unique", [0, 1])
def test_boundary_cases(unique):
    """The CPU test's boundary cases (tests/sparse_stereo_cases.py), one batch item each."""
    params = dict(cases.BOUNDARY_PARAMS, unique=unique)
    items = list(cases.boundary_cases().values())
    stereo, info = _run(items, cases.BOUNDARY_K, cases.BOUNDARY_BASELINE, params, 8)
    _check(items, stereo, info, cases.BOUNDARY_K, cases.BOUNDARY_BASELINE, params, 8)


def test_counts_above_cap_and_negative():
    """A count above cap is clamped to cap, a count <= 0 is an empty set."""
    cap = 96
    full = cases.random_set(cap, cap, 77)
    items = [full, full, full, full, full]
    counts = [(cap + 5, cap + 1000), (-3, cap), (cap, -1), (2 ** 31 - 1, -2 ** 31), (0, 0)]
    stereo, info = _run(items, cases.SET_K, cases.SET_BASELINE, cases.SET_PARAMS, cap, counts=counts)
    _check(items, stereo, info, cases.SET_K, cases.SET_BASELINE, cases.SET_PARAMS, cap, counts=counts)
    assert (info[2, :, 3] == ref.STATUS_NO_MATCH).all() and (info[0, :, 3] == 0).any()


def test_info_null_and_pitched_images():
    """info = NULL gives the same records; a pitched image buffer (13 bytes of padding after every
    row, image_stride = pitch * H) and one with 3 unused rows between the images as well
    (image_stride > pitch * H) give the same result, and the padding keeps its fill."""
    items = [cases.random_set(65, 257, 9), cases.random_set(257, 65, 10)]
    args = (cases.SET_K, cases.SET_BASELINE, cases.SET_PARAMS, 260)
    stereo, info = _run(items, *args)
    _check(items, stereo, info, *args)
    stereo_n, none = _run(items, *args, with_info=False)
    assert none is None and np.array_equal(stereo_n.view(np.uint32), stereo.view(np.uint32))
    stereo_p, info_p = _run(items, *args, pitch=cases.W + 13)  # (_run compares the whole buffers, padding included)
    assert np.array_equal(stereo_p.view(np.uint32), stereo.view(np.uint32)) and np.array_equal(info_p, info)
    stereo_g, info_g = _run(items, *args, pitch=cases.W + 13, gap_rows=3)
    assert np.array_equal(stereo_g.view(np.uint32), stereo.view(np.uint32)) and np.array_equal(info_g, info)


# ------------------------------------------------------------------ one real pair
RW, RH = 320, 200


@functools.lru_cache(maxsize=None)
def _real_items():
    """Seed-0 frame 0 at 320x200 with the oracle's ORB (500 features) on the CPU, an empty item and
    the pure-shift pair (right = left shifted 12 px)."""
    import oracle
    from forest_slam_amd import synth
    oracle.build()
    seq = synth.StereoSequence(seed=0, W=RW, H=RH)
    L, R = (x.numpy() for x in seq.frame(0))
    S = np.zeros_like(L)
    S[:, :-12] = L[:, 12:]

    def item(a, b):
        (ka, da), (kb, db) = oracle.orb_detect_compute(a, 500), oracle.orb_detect_compute(b, 500)
        pad = lambda k: np.concatenate([k, np.zeros((len(k), 2), np.float32)], 1)  # noqa: E731
        return dict(imgL=a, imgR=b, kpL=pad(ka), descL=da, kpR=pad(kb), descR=db)

    real, shifted = item(L, R), item(L, S)
    empty = dict(real, kpL=real["kpL"][:0], descL=real["descL"][:0], kpR=real["kpR"][:0], descR=real["descR"][:0])
    return real, empty, shifted, seq.K


@pytest.mark.parametrize("order", [(0,), (0, 1, 2), (1, 0, 2), (2, 1, 0)])
def test_real_pair(order):
    """The real pair alone, and as item 0, 1 and 2 of a batch beside an empty item and the shifted pair."""
    from forest_slam_amd import synth
    real, empty, shifted, K = _real_items()
    items = [(real, empty, shifted)[k] for k in order]
    params = {}
    stereo, info = _run(items, K, synth.BASELINE, params, 560, size=(RW, RH))
    _check(items, stereo, info, K, synth.BASELINE, params, 560)
    b = order.index(0)
    assert (info[b, :len(real["kpL"]), 3] == 0).sum() >= 100  # the comparison is not vacuous


# ------------------------------------------------------------------ fvo_backproject_stereo
@pytest.mark.parametrize("case", ["mixed_600", "all_kept", "none_kept", "no_matches", "cap_matches"])
def test_backproject_stereo(case):
    """Bit-exact against a NumPy gather: 600 matches (three compaction passes of 256), all kept,
    none kept, n_matches 0 and cap; nothing is written past n_points."""
    import torch
    cap, B = 640, 3
    ctx = _ctx(cases.W, cases.H, 48, 8)
    rng = np.random.default_rng(len(case))
    stereo = rng.uniform(0.5, 50, (B, cap, 4)).astype(np.float32)
    kp1 = rng.uniform(0, 300, (B, cap, 8)).astype(np.float32)
    matches = np.zeros((B, cap, 3), np.int32)
    nm = {"mixed_600": 600, "all_kept": 300, "none_kept": 300, "no_matches": 0, "cap_matches": cap}[case]
    n = np.array([nm, max(nm - 1, 0), nm], np.int32)
    for b in range(B):
        matches[b, :, 0] = rng.permutation(cap)
        matches[b, :, 1] = rng.permutation(cap)
        matches[b, :, 2] = rng.integers(0, 100, cap)
    if case in ("mixed_600", "cap_matches"):
        stereo[rng.uniform(size=(B, cap)) < 0.4] = 0
        stereo[0, matches[0, 5, 0]] = (1.0, 2.0, -0.0, 3.0)   # Z = -0 is "no point" too
        stereo[0, matches[0, 6, 0]] = (1.0, 2.0, -4.0, 3.0)   # any other Z is kept as it is
    elif case == "none_kept":
        stereo[..., 2] = 0
    dev = [torch.from_numpy(a).cuda() for a in (stereo, kp1, matches, n)]
    P3 = torch.full((B, cap, 3), STEREO_FILL, dtype=torch.float32, device="cuda")
    p2 = torch.full((B, cap, 2), STEREO_FILL, dtype=torch.float32, device="cuda")
    npts = torch.full((B,), INFO_FILL, dtype=torch.int32, device="cuda")
    ctx.backproject_stereo(dev[0], dev[1], dev[2], dev[3], out=(P3, p2, npts))
    torch.cuda.synchronize()
    P3, p2, npts = P3.cpu().numpy(), p2.cpu().numpy(), npts.cpu().numpy()
    for b in range(B):
        w3, w2, keep = ref.backproject_stereo(stereo[b], kp1[b], matches[b, :n[b]])
        k = int(keep.sum())
        assert npts[b] == k
        assert np.array_equal(P3[b, :k].view(np.uint32), w3.view(np.uint32))
        assert np.array_equal(p2[b, :k].view(np.uint32), w2.view(np.uint32))
        assert (P3[b, k:] == np.float32(STEREO_FILL)).all() and (p2[b, k:] == np.float32(STEREO_FILL)).all()
    if case == "all_kept":
        assert npts.tolist() == n.tolist()
    if case == "none_kept":
        assert not npts.any()


# ------------------------------------------------------------------ the front end
FW, FH, NFEAT = 320, 200, 300


@functools.lru_cache(maxsize=None)
def _sequence():
    """Seven frames at 320x200 (rendered on the GPU and copied to the host, so both sides see the
    same bytes) and the oracle pipeline with the specification's stereo records: per frame the
    oracle's ORB of both images and ref.sparse_stereo, per pair the oracle's BF matches, the
    records of the matched previous-left keypoints and solvePnPRansac."""
    import oracle
    import torch
    from forest_slam_amd import synth
    oracle.build()
    n = 7
    seq = synth.StereoSequence(seed=21, n_frames=n, W=FW, H=FH, device="cuda", start=150)
    Ls, Rs = seq.frames(range(n))
    torch.cuda.synchronize()
    fr = [(Ls[i].cpu().numpy(), Rs[i].cpu().numpy()) for i in range(n)]
    scales = np.array([float(np.float32(1.2)) ** o for o in range(8)], np.float32)  # Context.level_scales()
    orb = [(oracle.orb_detect_compute(a, NFEAT), oracle.orb_detect_compute(b, NFEAT)) for a, b in fr]
    stereo = [ref.sparse_stereo(fr[j][0], fr[j][1], orb[j][0][0], orb[j][0][1], orb[j][1][0], orb[j][1][1], seq.K,
                                synth.BASELINE, ref.Params(), scales)[0] for j in range(n)]
    pairs = []
    for j in range(n - 1):
        m = oracle.bf_match(orb[j][0][1], orb[j + 1][0][1])
        P3, p2, _ = ref.backproject_stereo(stereo[j], orb[j + 1][0][0], m)
        p = dict(matches=m, P3=P3, T=None)
        if len(P3) >= 6:
            ok, rv, tv, _, _, _ = oracle.solve_pnp_ransac(P3, p2, seq.K, synth.DIST_L)
            T = np.eye(4)
            T[:3, :3] = oracle.rodrigues(rv)
            T[:3, 3] = tv
            p.update(ok=ok, T=T)
        pairs.append(p)
    return seq, Ls, Rs, [o[0][0] for o in orb], stereo, pairs


def _front_end(seq, ba_window, **kw):
    from forest_slam_amd import synth, vo
    return vo.StereoFrontEnd(FW, FH, seq.K, synth.DIST_L, synth.BASELINE, batch=3, nfeatures=NFEAT,
                             ba_window=ba_window, **kw)


def _steps(fe, Ls, Rs):
    """prime + two steps of three frames; per pair the matches, records, points, PnP and returned T."""
    import torch
    fe.prime(Ls[0], Rs[0])
    out = dict(T=[], T_pnp=[], st=[], m=[], P3=[], rec=[])
    for s in (1, 4):
        T, st = fe.step(Ls[s:s + 3], Rs[s:s + 3])
        torch.cuda.synchronize()
        out["T"].append(T.cpu().numpy().copy())
        out["T_pnp"].append(fe.T[:3].cpu().numpy().copy())
        out["st"].append(st.cpu().numpy().copy())
        for i in range(3):
            out["m"].append(fe.matches[i, :int(fe.nmatch[i].item())].cpu().numpy().copy())
            out["P3"].append(fe.P3[i, :int(fe.npts[i].item())].cpu().numpy().copy())
            if fe.sparse:
                out["rec"].append(fe.q_stereo[i, :int(fe.q_cnt[i].item())].cpu().numpy().copy())
    return {k: (np.concatenate(v) if k in ("T", "T_pnp", "st") else v) for k, v in out.items()}


def _check_pnp(got, stereo, pairs):
    for j, p in enumerate(pairs):
        assert np.array_equal(got["m"][j], p["matches"]), f"pair {j}: BF matches differ"
        assert np.array_equal(got["rec"][j].view(np.uint32), stereo[j].view(np.uint32)), f"pair {j}: records differ"
        assert np.array_equal(got["P3"][j].view(np.uint32), p["P3"].view(np.uint32)), f"pair {j}: 3D points differ"
        if p["T"] is None:
            assert got["st"][j] == -1
            continue
        assert got["st"][j] == int(p["ok"])
        assert np.abs(got["T_pnp"][j] - p["T"]).max() <= 1e-4 * max(1.0, np.abs(p["T"]).max()), f"pair {j}: PnP pose"


def test_front_end_sparse_pnp():
    """StereoFrontEnd(depth="sparse", ba_window=0): prime + two steps of three frames against the
    oracle pipeline with the specification's records -- matches, records and point sets identical,
    statuses equal, T within 1e-4; its workspace is smaller than the default front end's."""
    seq, Ls, Rs, kps, stereo, pairs = _sequence()
    fe = _front_end(seq, 0, depth="sparse")
    got = _steps(fe, Ls, Rs)
    _check_pnp(got, stereo, pairs)
    assert np.array_equal(got["T"], got["T_pnp"])
    assert min(len(p["P3"]) for p in pairs) >= 20 and (got["st"] == 1).all()  # the comparison is not vacuous
    dense = _front_end(seq, 0, num_disparities=64)
    assert fe.ctx.workspace_bytes < dense.ctx.workspace_bytes
    with pytest.raises(RuntimeError, match="sparse"):
        fe.append_dense(None, np.zeros((3, 4, 4)))
    # the right temporal match is not needed
    got2 = _steps(_front_end(seq, 0, depth="sparse", match_right=False), Ls, Rs)
    assert np.array_equal(got2["T"], got["T"]) and np.array_equal(got2["st"], got["st"])


def test_front_end_sparse_local_ba():
    """ba_window=3: the same records go into the BA history; every window against ba_ref
    (initialised, like the product, with the product's PnP transforms) within 1e-8."""
    import ba_ref
    from forest_slam_amd import synth
    seq, Ls, Rs, kps, stereo, pairs = _sequence()
    Kw = 3
    got = _steps(_front_end(seq, Kw, depth="sparse"), Ls, Rs)
    _check_pnp(got, stereo, pairs)
    st3 = [(s[:, :3], s[:, 3], s[:, 2] != 0) for s in stereo]
    matches = [p["matches"] for p in pairs]
    for e in range(1, len(kps)):
        s = max(0, e - Kw + 1)
        if e - s + 1 < 3:
            assert np.array_equal(got["T"][e - 1], got["T_pnp"][e - 1])
            continue
        want = ba_ref.ba_window(kps[s:e + 1], matches[s:e], st3[s:e], got["T_pnp"][s:e], seq.K, synth.BASELINE, iters=10)
        assert np.abs(got["T"][e - 1] - want["rel"][-1]).max() < 1e-8, f"BA window ending at frame {e}"


def _steps_unsynchronised(fe, Ls, Rs):
    """prime + two steps with no host synchronisation in between (a slow kernel is queued ahead of
    prime on the caller's stream); each step's outputs are cloned on the caller's stream."""
    import torch
    torch.cuda.synchronize()
    torch.cuda._sleep(200_000_000)  # ~0.1 s of spinning on the caller's stream
    fe.prime(Ls[0], Rs[0])
    got = []
    for s in (1, 4):
        T, st = fe.step(Ls[s:s + 3], Rs[s:s + 3])
        got.append([t.clone() for t in (T, st, fe.T[:3], fe.P3[:3], fe.npts[:3], fe.q_stereo[:3], fe.q_cnt[:3])])
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in g] for g in got]


def test_front_end_sparse_overlapped_equals_in_order():
    """overlap_sgbm=True puts the front stage (ORB, BF, the sparse records and their moves) on its
    own stream into the two q_stereo slots, while cur_stereo, last_stereo and the workspace have
    one slot each and are touched on that stream only.  With and without local BA, prime and two
    steps queued without a host synchronisation give the in-order front end's transforms, statuses,
    points and records bit for bit."""
    seq, Ls, Rs, *_ = _sequence()
    for Kw in (0, 3):
        want = _steps_unsynchronised(_front_end(seq, Kw, depth="sparse"), Ls, Rs)
        got = _steps_unsynchronised(_front_end(seq, Kw, depth="sparse", overlap_sgbm=True), Ls, Rs)
        for k, (w, g) in enumerate(zip(want, got)):
            T, st, T_pnp, P3, npts, rec, cnt = g
            assert all(x.tobytes() == y.tobytes() for x, y in zip(w[:3], g[:3])), (Kw, k)
            assert np.array_equal(npts, w[4]) and np.array_equal(cnt, w[6]) and (st == 1).all() and npts.min() >= 20
            for i in range(3):
                assert P3[i, :npts[i]].tobytes() == w[3][i, :npts[i]].tobytes(), (Kw, k, i)
                assert rec[i, :cnt[i]].tobytes() == w[5][i, :cnt[i]].tobytes(), (Kw, k, i)


def test_front_end_sgbm_argument_is_todays_path():
    """depth="sgbm" is the default: bit-identical to a front end constructed without the argument."""
    seq, Ls, Rs, *_ = _sequence()
    a = _steps(_front_end(seq, 3, num_disparities=64), Ls, Rs)
    b = _steps(_front_end(seq, 3, num_disparities=64, depth="sgbm"), Ls, Rs)
    for k in ("T", "T_pnp", "st"):
        assert a[k].tobytes() == b[k].tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(a["P3"], b["P3"]))
    with pytest.raises(ValueError, match="depth"):
        _front_end(seq, 0, depth="dense")
