"""ORB with the FAST tiles laid over a level's interior only (origin (edge, edge), extent
(w - 2 edge) x (h - 2 edge)) and the orientation formed inside the BRIEF kernel: keypoints
[:, :6], descriptors and counts bit-exact against the oracle at the shapes where that geometry
can go wrong.

Reference.  oracle.orb_detect_compute has edgeThreshold fixed at 31, so the cases at 15 and 16
compare against tests/orb_edge_ref.py, the oracle's own stages with the border filter as a
parameter; test_edge_reference_is_the_oracle_at_31 pins it to oracle.orb_detect_compute
without a GPU, and the edge-31 cases compare against oracle.orb_detect_compute itself.

edge values.  check_orb_config accepts edgeThreshold >= patchSize / 2 = 15 (patchSize is pinned
to 31) and has no upper bound: 15 is the low end, 16 and 31 are the other two values, and an
edge past half the image (40 at 64x64) leaves no level an interior at all.

Orientation.  Every configuration check_orb_config accepts takes the path with the orientation
inside k_brief, which all cases but one therefore run.  The separate k_angle pass is selected
only for patchSize / 2 > 15 or edgeThreshold < patchSize / 2, both refused at creation;
fvo_debug_buffer(ctx, 10) switches a context to it, and test_orb_orientation_paths_bit_exact
runs the same images through both.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLDEN, gpu_available
import orb_edge_ref

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")

NFEAT = 500
TW, TH = 64, 32  # FAST tile
# (edge, W, H) -> the interior (w - 2 edge, h - 2 edge) the size is there for, and its level.
# Image sides must be >= 64, so at edge 15 and 16 the one-tile interiors sit on level 1.
SHAPES = {
    (15, 113, 74): ((64, 32), 1), (15, 114, 76): ((65, 33), 1), (15, 230, 100): ((200, 70), 0),
    (16, 115, 77): ((64, 32), 1), (16, 116, 78): ((65, 33), 1), (16, 232, 102): ((200, 70), 0),
    (31, 126, 94): ((64, 32), 0), (31, 127, 95): ((65, 33), 0), (31, 262, 132): ((200, 70), 0),
}


def _levels(W, H):
    out = []
    for l in range(8):
        inv = np.float32(1.0) / np.float32(float(np.float32(1.2)) ** l)
        out.append((int(np.rint(np.float32(W) * inv)), int(np.rint(np.float32(H) * inv))))
    return out


_nat = {}


def _crops(W, H):
    """Two different textured W x H crops (gravel, grass): FAST fires right up to their sides."""
    if not _nat:
        z = np.load(f"{GOLDEN}/natural_images.npz")
        _nat.update(gravel=z["gravel"], grass=z["grass"])
    return [np.ascontiguousarray(_nat["gravel"][:H, :W]), np.ascontiguousarray(_nat["grass"][40:40 + H, 60:60 + W])]


_ref_cache = {}


def _reference(oracle_mod, key, imgs, edge):
    if key not in _ref_cache:
        if edge == 31:
            _ref_cache[key] = [oracle_mod.orb_detect_compute(im, NFEAT) for im in imgs]
        else:
            _ref_cache[key] = [orb_edge_ref.orb_reference(oracle_mod, im, NFEAT, edge) for im in imgs]
    return _ref_cache[key]


def _dots(edge, W=200, H=150):
    """Flat 100 with single bright pixels (each a FAST corner scoring its contrast - 1) on and just
    outside the border filter's four sides, alone and as adjacent pairs in which the outer or
    the inner one is the stronger, and the same across the first tile seam.  Returns the image,
    the level-0 positions that must survive and those that must not."""
    im = np.full((H, W), 100, np.uint8)
    keep, drop = [], []
    lo, hi = edge, W - edge - 1     # first / last kept column
    rows = iter(range(edge + 6, H - edge - 4, 9))
    for x_in, x_out in ((lo, lo - 1), (hi, hi + 1)):
        y = next(rows); im[y, x_in] = 220; keep.append((x_in, y))            # alone, inside
        y = next(rows); im[y, x_out] = 220; drop.append((x_out, y))          # alone, outside
        y = next(rows); im[y, x_in], im[y, x_out] = 200, 250                 # the outer one wins the NMS
        drop += [(x_in, y), (x_out, y)]
        y = next(rows); im[y, x_in], im[y, x_out] = 250, 200                 # the inner one wins
        keep.append((x_in, y)); drop.append((x_out, y))
    lo, hi = edge, H - edge - 1
    cols = iter(range(edge + 9, W - edge - 9, 9))
    for y_in, y_out in ((lo, lo - 1), (hi, hi + 1)):
        x = next(cols); im[y_in, x] = 220; keep.append((x, y_in))
        x = next(cols); im[y_out, x] = 220; drop.append((x, y_out))
        x = next(cols); im[y_in, x], im[y_out, x] = 200, 250
        drop += [(x, y_in), (x, y_out)]
        x = next(cols); im[y_in, x], im[y_out, x] = 250, 200
        keep.append((x, y_in)); drop.append((x, y_out))
    # the corner of the interior against its diagonal neighbour outside
    im[edge, edge], im[edge - 1, edge - 1] = 200, 250
    drop += [(edge, edge), (edge - 1, edge - 1)]
    # across the seam between tile columns 0 and 1 and tile rows 0 and 1
    y = next(rows); im[y, edge + TW - 1], im[y, edge + TW] = 200, 250
    drop.append((edge + TW - 1, y)); keep.append((edge + TW, y))
    x = next(cols); im[edge + TH - 1, x], im[edge + TH, x] = 250, 200
    keep.append((x, edge + TH - 1)); drop.append((x, edge + TH))
    return im, keep, drop


# ------------------------------------------------------------------ without a GPU
def test_shapes_reach_the_cases():
    """The sizes have the interiors they were chosen for; each set has a level whose interior is
    smaller than a tile and a level without interior."""
    for (edge, W, H), (want, lvl) in SHAPES.items():
        inter = [(w - 2 * edge, h - 2 * edge) for w, h in _levels(W, H)]
        assert inter[lvl] == want, (edge, W, H, inter)
        assert any(0 < iw <= TW and 0 < ih <= TH and (iw, ih) != (TW, TH) for iw, ih in inter), (edge, W, H, inter)
        assert any(iw <= 0 or ih <= 0 for iw, ih in inter), (edge, W, H, inter)
    iw, ih = 200, 70  # several tiles, ragged last column and row
    assert iw % TW and ih % TH and iw > 2 * TW and ih > 2 * TH


def test_edge_reference_is_the_oracle_at_31(oracle_mod):
    for W, H in ((127, 95), (262, 132)):
        for im in _crops(W, H):
            rk, rd = oracle_mod.orb_detect_compute(im, NFEAT)
            k, d = orb_edge_ref.orb_reference(oracle_mod, im, NFEAT, 31)
            assert len(rk) > 20
            assert np.array_equal(k, rk) and np.array_equal(d, rd)


@pytest.mark.parametrize("edge", [15, 16, 31])
def test_dot_image_keeps_and_drops_what_it_was_painted_for(oracle_mod, edge):
    im, keep, drop = _dots(edge)
    kp, _ = _reference(oracle_mod, ("dots", edge), [im], edge)[0]
    lvl0 = {(int(x), int(y)) for x, y, _, _, _, o in kp if o == 0}
    assert set(keep) <= lvl0 and not (set(drop) & lvl0)


# ------------------------------------------------------------------ on the GPU
def _orb_gpu(ctx, imgs):
    """Runs ORB into sentinel-filled outputs; returns [(kp, desc)] and the counts, and checks
    that nothing past an image's count was written."""
    B, cap = len(imgs), ctx.kp_cap
    kp = torch.full((B, cap, 8), -12345.0, dtype=torch.float32, device="cuda")
    desc = torch.full((B, cap, 32), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ctx.orb(torch.from_numpy(np.stack(imgs)).cuda(), out=(kp, desc, cnt))
    torch.cuda.synchronize()
    kp, desc, cnt = kp.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy()
    for i in range(B):
        assert 0 <= cnt[i] <= cap
        assert (kp[i, cnt[i]:] == -12345.0).all() and (desc[i, cnt[i]:] == 0xA5).all(), f"image {i}: wrote past its count"
    return [(kp[i, :cnt[i]], desc[i, :cnt[i]]) for i in range(B)], cnt


def _assert_orb_equal(got, ref, what):
    for i, ((kp, desc), (rkp, rdesc)) in enumerate(zip(got, ref)):
        assert kp.shape[0] == rkp.shape[0], f"{what} image {i}: {kp.shape[0]} keypoints, reference {rkp.shape[0]}"
        assert np.array_equal(kp[:, :6], rkp), f"{what} image {i}: rows {np.argwhere(kp[:, :6] != rkp)[:5].tolist()}"
        assert np.array_equal(desc, rdesc), f"{what} image {i}: descriptors differ"


@gpu
@needs_gpu
@pytest.mark.parametrize("edge,W,H", list(SHAPES))
def test_orb_interior_tiles_bit_exact(oracle_mod, edge, W, H):
    """A batch of two different images per shape: one-tile, one-pixel-overhang and ragged
    multi-tile interiors, with sub-tile and empty levels above them."""
    from forest_slam_amd import _lib
    imgs = _crops(W, H)
    ref = _reference(oracle_mod, (edge, W, H), imgs, edge)
    ctx = _lib.Context(W, H, max_batch=2, nfeatures=NFEAT, edge_threshold=edge, stages=_lib.STAGE_ORB)
    got, cnt = _orb_gpu(ctx, imgs)
    assert cnt.tolist() == [len(r[0]) for r in ref] and cnt.min() > 20
    assert not np.array_equal(ref[0][0][:20], ref[1][0][:20])  # the two images differ
    _assert_orb_equal(got, ref, f"edge {edge} {W}x{H}")
    # levels without interior: no candidate, nothing selected
    empty = [l for l, (w, h) in enumerate(_levels(W, H)) if w <= 2 * edge or h <= 2 * edge]
    assert empty
    for which in (3, 4, 5):
        n = ctx.debug_buffer(which).view(torch.int32).view(2, -1).numpy()
        assert (n[:, empty] == 0).all(), (which, n.tolist())


@gpu
@needs_gpu
@pytest.mark.parametrize("separate_pass", [False, True])
@pytest.mark.parametrize("edge,W,H", [(15, 114, 76), (31, 262, 132)])
def test_orb_orientation_paths_bit_exact(oracle_mod, edge, W, H, separate_pass):
    """The orientation inside k_brief and as k_angle's pass of its own (debug switch 10), at the
    default edge and at 15, where patches near the border are staged with REFLECT_101."""
    from forest_slam_amd import _lib
    imgs = _crops(W, H)
    ref = _reference(oracle_mod, (edge, W, H), imgs, edge)
    ctx = _lib.Context(W, H, max_batch=2, nfeatures=NFEAT, edge_threshold=edge, stages=_lib.STAGE_ORB)
    if separate_pass:
        p, nb = ctypes.c_void_p(), ctypes.c_int64(-1)
        assert ctx.L.fvo_debug_buffer(ctx.h, 10, ctypes.byref(p), ctypes.byref(nb)) == 0 and nb.value == 0
    # the path taken shows in the launches: orb_angle runs only as the separate pass
    ctx.timing_enable(None)
    got, _ = _orb_gpu(ctx, imgs)
    launched = ctx.timing_read()
    ctx.timing_enable([])
    assert ("orb_angle" in launched) == separate_pass and "orb_brief" in launched, sorted(launched)
    _assert_orb_equal(got, ref, f"edge {edge} {W}x{H} separate_pass={separate_pass}")


@gpu
@needs_gpu
def test_orb_no_level_has_an_interior(oracle_mod):
    """edge 40 at 64x64: no FAST tile at all; counts are 0 and nothing is written."""
    from forest_slam_amd import _lib
    imgs = _crops(64, 64)
    ctx = _lib.Context(64, 64, max_batch=2, nfeatures=NFEAT, edge_threshold=40, stages=_lib.STAGE_ORB)
    _, cnt = _orb_gpu(ctx, imgs)
    assert cnt.tolist() == [0, 0]
    assert all(len(orb_edge_ref.orb_reference(oracle_mod, im, NFEAT, 40)[0]) == 0 for im in imgs)


@gpu
@needs_gpu
@pytest.mark.parametrize("edge", [15, 16, 31])
def test_orb_corners_on_the_border_filter(oracle_mod, edge):
    """Corners at x = edge, edge - 1, w - edge - 1, w - edge (and in y): the inner ones kept, and
    suppressed when the neighbour just outside the interior scores higher."""
    from forest_slam_amd import _lib
    im, keep, drop = _dots(edge)
    ref = _reference(oracle_mod, ("dots", edge), [im], edge)
    ctx = _lib.Context(im.shape[1], im.shape[0], max_batch=1, nfeatures=NFEAT, edge_threshold=edge,
                       stages=_lib.STAGE_ORB)
    got, _ = _orb_gpu(ctx, [im])
    _assert_orb_equal(got, ref, f"dots, edge {edge}")
    lvl0 = {(int(x), int(y)) for x, y, _, _, _, o in got[0][0][:, :6] if o == 0}
    assert set(keep) <= lvl0 and not (set(drop) & lvl0)


@gpu
@needs_gpu
def test_orb_score_map_stays_whole_level(oracle_mod):
    """debug_buffer(2) after an interior-tiled call: the FAST score of every pixel of every
    level, border included."""
    from forest_slam_amd import _lib
    edge, W, H = 31, 127, 95
    imgs = _crops(W, H)
    ctx = _lib.Context(W, H, max_batch=2, nfeatures=NFEAT, edge_threshold=edge, stages=_lib.STAGE_ORB)
    _orb_gpu(ctx, imgs)
    geo, total = ctx.geometry()
    score = ctx.debug_buffer(2).numpy()
    stride = len(score) // 2
    for b, im in enumerate(imgs):
        border = 0
        for (w, h, off), lvl in zip(geo, oracle_mod.orb_pyramid(im, 8)):
            ref = oracle_mod.fast_score_map(lvl, 20)
            got = score[b * stride + off:b * stride + off + w * h].reshape(h, w)
            assert np.array_equal(got, ref), f"image {b} FAST score {w}x{h}: {np.argwhere(got != ref)[:5].tolist()}"
            inner = np.zeros_like(ref, bool)
            inner[edge:h - edge, edge:w - edge] = True
            border += int((ref[~inner] > 0).sum())
        assert border > 50  # the map has corners where the hot path lays no tile
