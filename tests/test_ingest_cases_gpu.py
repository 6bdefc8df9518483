"""fvo_undistort_gray and fvo_motion_blur off the reference's cameras and off contiguous buffers,
bit for bit against the oracle (cases: tests/ingest_cases.py; what each case reaches is asserted
without a GPU in test_ingest_cases_cpu.py).  Lenses with tangential terms, k3, skew, K[8] != 1, a
projective bottom row and saturating map entries; pitched sources and misaligned / pitched
destinations through the C ABI, with every byte between rows and images checked; the blur at the
kernel sizes on both sides of its direct / DFT switch, at the smallest and largest k, on images
narrower than a tile, with seeds on the tile seams; the count clamp and the ignored indices."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import as_strided

import ingest_cases as ic
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

FILL = 0xA5
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


@functools.lru_cache(maxsize=None)
def _ctx(W, H):
    from forest_slam_amd import _lib
    return _lib.Context(W, H, max_batch=3, stages=_lib.STAGE_BF, kp_capacity=64)


def _stream(ctx):
    from forest_slam_amd import _lib
    return _lib._stream(ctx.device)


def _p(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def _rows(buf, B, H, R, pitch, stride, offset=0):
    """The [B, H, R] bytes of B images of H rows of R bytes inside the flat buffer."""
    return as_strided(buf[offset:], (B, H, R), (stride, pitch, 1))


def _pitched(data, pitch, stride, offset=0):
    """A flat buffer of FILL bytes holding data [B, H, R] with rows `pitch` and images `stride`
    bytes apart, the first byte at `offset`."""
    B, H, R = data.shape
    buf = np.full(offset + stride * B + 8, FILL, np.uint8)
    _rows(buf, B, H, R, pitch, stride, offset)[...] = data
    return buf


def _only_rows_written(buf, B, H, R, pitch, stride, offset=0):
    rest = buf.copy()
    _rows(rest, B, H, R, pitch, stride, offset)[...] = FILL
    return bool((rest == FILL).all())


@functools.lru_cache(maxsize=None)
def _undistort_want(name, W, H):
    K, dist = ic.lens(name)
    import oracle
    return np.stack([oracle.undistort_gray(img, K, dist) for img in ic.images(W, H)])


# ------------------------------------------------------------------------------ undistort
@pytest.mark.parametrize("case", ic.LENS_CASES, ids=ic.case_id)
def test_undistort_lens_cases_match_oracle(oracle_mod, case):
    name, W, H = case
    K, dist = ic.lens(name)
    got = _ctx(W, H).undistort_gray(torch.from_numpy(np.array(ic.images(W, H))).cuda(), K, dist).cpu().numpy()
    want = _undistort_want(name, W, H)
    for b in range(3):
        assert np.array_equal(got[b], want[b]), (case, b, int((got[b] != want[b]).sum()))


# (W, H, destination offset, dst_pitch - W, dst_stride - dst_pitch*H): a destination one byte off
# an aligned allocation with odd gaps (the byte-wise stores), and a 4-byte aligned pitched one (the
# dword stores next to gap bytes)
UNDISTORT_LAYOUTS = [(101, 77, 1, 3, 5), (100, 76, 1, 3, 5), (100, 76, 0, 4, 4)]


@pytest.mark.parametrize("layout", UNDISTORT_LAYOUTS, ids=lambda v: "%dx%d-off%d-pitch+%d-stride+%d" % v)
def test_undistort_pitched_layouts(oracle_mod, layout):
    W, H, off, dp, ds = layout
    ctx, B = _ctx(W, H), 3
    K, dist = ic.lens("tang")
    imgs = np.array(ic.images(W, H))
    spitch = 3 * W + 5
    sstride = spitch * H + 7
    dpitch = W + dp
    dstride = dpitch * H + ds
    src_h = _pitched(imgs.reshape(B, H, 3 * W), spitch, sstride)
    dst_h = np.full(off + dstride * B + 8, FILL, np.uint8)
    src, dst = torch.from_numpy(src_h).cuda(), torch.from_numpy(dst_h).cuda()
    assert dst.data_ptr() % 4 == 0 and (off or (dpitch % 4 == 0 and dstride % 4 == 0))
    Kh = (ctypes.c_double * 9)(*K.reshape(-1))
    dh = (ctypes.c_double * 5)(*dist)
    ctx._check(ctx.L.fvo_undistort_gray(ctx.h, _p(src), B, sstride, spitch, Kh, dh, _p(dst, off), dstride, dpitch,
                                        _stream(ctx)))
    got = dst.cpu().numpy()
    contiguous = ctx.undistort_gray(torch.from_numpy(imgs).cuda(), K, dist).cpu().numpy()
    assert np.array_equal(contiguous, _undistort_want("tang", W, H))
    assert np.array_equal(_rows(got, B, H, W, dpitch, dstride, off), contiguous)
    assert _only_rows_written(got, B, H, W, dpitch, dstride, off)
    assert np.array_equal(src.cpu().numpy(), src_h)


# ----------------------------------------------------------------------------- motion blur
def _centers_tensor(lists, cap, pad):
    C = np.full((len(lists), cap), pad, np.int32)
    for b, c in enumerate(lists):
        C[b, :min(len(c), cap)] = c[:cap]
    return torch.from_numpy(C).cuda()


@pytest.mark.parametrize("case", ic.BLUR_CASES, ids=lambda c: "%dx%d-k%d" % c)
def test_blur_kernel_sizes_match_oracle(oracle_mod, case):
    W, H, k = case
    ctx = _ctx(W, H)
    imgs = ic.gray_images(W, H)
    cs = [ic.blur_centers(W, H, 10 * k + b) for b in range(3)]
    cap = max(len(c) for c in cs)
    n = torch.tensor([len(c) for c in cs], dtype=torch.int32, device="cuda")
    out, mask = ctx.motion_blur(torch.from_numpy(imgs).cuda(), k, _centers_tensor(cs, cap, 0), n)
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    for b in range(3):
        want, wmask = oracle_mod.motion_blur(imgs[b], k, cs[b])
        assert np.array_equal(mask[b], wmask), (case, b)
        assert np.array_equal(out[b], want), (case, b, int((out[b] != want).sum()))
        if k > 1:
            assert (want != imgs[b]).any()  # the blur is visible in the expected image


@pytest.mark.parametrize("last_count", [0, -3])
def test_blur_counts_and_indices(oracle_mod, last_count):
    """Image 0: n_centers above centers_cap uses the first centers_cap entries.  Image 1: entries
    that are no pixel index (-1, H*W, INT32_MAX, INT32_MIN) among valid ones are ignored.  Image 2:
    a zero or negative count blurs nothing.  Every unused entry of the centres array is a valid
    pixel index, so reading past a count shows in the mask."""
    W, H, k = 70, 48, 11
    ctx = _ctx(W, H)
    imgs = ic.gray_images(W, H)
    full = ic.blur_centers(W, H, 5)
    cap = 24
    assert len(full) > cap
    valid = ic.blur_centers(W, H, 6)[:12]
    mixed = np.concatenate([valid[:3], [-1], valid[3:6], [H * W], valid[6:9], [INT32_MAX, INT32_MIN],
                            valid[9:]]).astype(np.int32)
    assert len(mixed) < cap
    lists = [full, mixed, np.zeros(0, np.int32)]
    used = [full[:cap], mixed[(mixed >= 0) & (mixed < H * W)], lists[2]]  # what the kernel is specified to use
    assert len(used[1]) == len(valid) and np.array_equal(used[1], valid)
    n = torch.tensor([len(full), len(mixed), last_count], dtype=torch.int32, device="cuda")
    out, mask = ctx.motion_blur(torch.from_numpy(imgs).cuda(), k, _centers_tensor(lists, cap, (H // 2) * W + 7), n)
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    for b in range(3):
        want, wmask = oracle_mod.motion_blur(imgs[b], k, used[b])
        assert np.array_equal(mask[b], wmask), b
        assert np.array_equal(out[b], want), b
    assert not mask[2].any() and np.array_equal(out[2], imgs[2])
    assert not np.array_equal(mask[0], oracle_mod.motion_blur(imgs[0], k, full)[1])  # the clamp shows


def test_blur_without_centers_is_identity():
    W, H, k = 101, 77, 15
    ctx = _ctx(W, H)
    imgs = ic.gray_images(W, H)
    out = torch.full((3, H, W), 0xFF, dtype=torch.uint8, device="cuda")
    mask = torch.full((3, H, W), 0xFF, dtype=torch.uint8, device="cuda")
    ctx.motion_blur(torch.from_numpy(imgs).cuda(), k, None, None, out=out, mask=mask)
    assert not mask.cpu().numpy().any()
    assert np.array_equal(out.cpu().numpy(), imgs)


def test_blur_pitched_layouts(oracle_mod):
    W, H, k, B, off = 101, 77, 12, 3, 1
    ctx = _ctx(W, H)
    imgs = ic.gray_images(W, H)
    cs = [ic.blur_centers(W, H, 40 + b) for b in range(B)]
    cap = max(len(c) for c in cs)
    C = _centers_tensor(cs, cap, 0)
    n = torch.tensor([len(c) for c in cs], dtype=torch.int32, device="cuda")
    spitch = W + 5
    sstride = spitch * H + 7
    dpitch = W + 3
    dstride = dpitch * H + 5
    src_h = _pitched(imgs, spitch, sstride)
    dst_h = np.full(off + dstride * B + 8, FILL, np.uint8)
    src, dst = torch.from_numpy(src_h).cuda(), torch.from_numpy(dst_h).cuda()
    mask = torch.full((B, H, W), FILL, dtype=torch.uint8, device="cuda")  # [batch][H][W], 4-byte aligned
    assert dst.data_ptr() % 4 == 0 and mask.data_ptr() % 4 == 0
    ctx._check(ctx.L.fvo_motion_blur(ctx.h, _p(src), B, sstride, spitch, k, 0.0, _p(C), _p(n), cap, _p(mask),
                                     _p(dst, off), dstride, dpitch, _stream(ctx)))
    got = dst.cpu().numpy()
    want_out, want_mask = ctx.motion_blur(torch.from_numpy(imgs).cuda(), k, C, n)
    want_out, want_mask = want_out.cpu().numpy(), want_mask.cpu().numpy()
    for b in range(B):
        o, m = oracle_mod.motion_blur(imgs[b], k, cs[b])
        assert np.array_equal(want_out[b], o) and np.array_equal(want_mask[b], m), b
    assert np.array_equal(_rows(got, B, H, W, dpitch, dstride, off), want_out)
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    assert _only_rows_written(got, B, H, W, dpitch, dstride, off)
    assert np.array_equal(src.cpu().numpy(), src_h)
