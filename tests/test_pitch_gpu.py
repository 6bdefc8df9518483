"""fvo_sgbm and fvo_orb_detect_compute on pitched, strided inputs.  The Context wrappers always
pass contiguous images (pitch = W, stride = H * W), so the C entry points are called directly:
the images sit inside a larger uint8 device buffer pre-filled with 0xA5 (SGBM's left and right
batches in the same buffer), with rows `pitch` and images `stride` bytes apart.  The output must
equal the oracle on the tight images bit for bit, and the parent buffer must come back unchanged.

Layouts: (W + 13, pitch * H + 7) at an odd offset -- ORB's scalar level-0 copy; (W + 16,
pitch * H + 64) at a 16-byte aligned offset -- at W % 16 == 0 ORB's vector copy with
pitch != W; and the contiguous control.
"""
import numpy as np
import pytest
import torch

import sgbm_cases as sc
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

FILL = 0xA5
LAYOUTS = ["pad13_stride7", "pad16_stride64", "contiguous"]


def _layout(name, W, H):
    """(pitch, stride, byte offset of the first image in the parent buffer)."""
    if name == "pad13_stride7":
        p = W + 13
        return p, p * H + 7, 3
    if name == "pad16_stride64":
        p = W + 16
        return p, p * H + 64, 32
    return W, W * H, 16


def _place(parent, off, imgs, pitch, stride):
    """Write imgs u8 [B,H,W] into the host parent buffer at off + b * stride, rows pitch apart."""
    B, H, W = imgs.shape
    for b in range(B):
        rows = np.lib.stride_tricks.as_strided(parent[off + b * stride:], shape=(H, W), strides=(pitch, 1))
        rows[:] = imgs[b]


def _parent(groups, layout, pitch, stride, off):
    """Host parent buffer (0xA5 everywhere) holding every group of images one after another with
    a gap between them (the groups stay 16-byte aligned except in the odd layout); returns
    (buffer, offsets of the groups)."""
    offs, pos = [], off
    for g in groups:
        offs.append(pos)
        pos += len(g) * stride + 29
        if layout != "pad13_stride7":
            pos = (pos + 15) // 16 * 16
    host = np.full(pos + 64, FILL, np.uint8)
    for g, o in zip(groups, offs):
        _place(host, o, g, pitch, stride)
    return host, offs


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H,D", [(213, 75, 64), (320, 200, 96)])
def test_sgbm_pitched_input_bit_exact(oracle_mod, W, H, D, layout):
    from forest_slam_amd import _lib
    L, R = sc.pair_batch(W, H)
    want = sc.reference(oracle_mod, W, H, D, {})
    pitch, stride, off = _layout(layout, W, H)
    host, (oL, oR) = _parent([L, R], layout, pitch, stride, off)
    dev = torch.from_numpy(host.copy()).cuda()
    ctx = _lib.Context(W, H, max_batch=2, num_disparities=D, stages=_lib.STAGE_SGBM)
    out = torch.empty((2, H, W), dtype=torch.int16, device="cuda")
    st = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    rc = ctx.L.fvo_sgbm(ctx.h, _lib._ptr(dev[oL:]), _lib._ptr(dev[oR:]), 2, stride, pitch, _lib._ptr(out),
                        _lib._ptr(st), _lib._stream(ctx.device))
    assert rc == 0, ctx.L.fvo_last_error(ctx.h).decode()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(2):
        bad = np.argwhere(got[i] != want[i])
        assert len(bad) == 0, f"{layout} image {i}: {len(bad)} px differ, first {bad[:5].tolist()}"
    assert st.tolist() == [_lib.SGBM_OK] * 2
    assert np.array_equal(dev.cpu().numpy(), host), "the caller's buffer changed"


@pytest.fixture(scope="module")
def orb_inputs(oracle_mod):
    """(W, H) -> (images u8 [2,H,W], oracle (kp, desc) per image) at nfeatures = 300."""
    from forest_slam_amd import synth
    out = {}
    for W, H in ((320, 200), (333, 217)):
        imgs = np.stack([x.numpy() for x in synth.StereoSequence(seed=21, n_frames=1, W=W, H=H, device="cpu").frame(0)])
        out[(W, H)] = (imgs, [oracle_mod.orb_detect_compute(im, 300) for im in imgs])
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", [(320, 200), (333, 217)])
def test_orb_pitched_input_bit_exact(orb_inputs, W, H, layout):
    """320 wide: the 16-aligned layout takes the vector level-0 copy with pitch != W, the W + 13
    layout the scalar one; 333 wide: always the scalar copy."""
    from forest_slam_amd import _lib
    imgs, refs = orb_inputs[(W, H)]
    assert min(len(kp) for kp, _ in refs) > 50
    pitch, stride, off = _layout(layout, W, H)
    host, (o,) = _parent([imgs], layout, pitch, stride, off)
    dev = torch.from_numpy(host.copy()).cuda()
    ctx = _lib.Context(W, H, max_batch=2, nfeatures=300, stages=_lib.STAGE_ORB)
    cap = ctx.kp_cap
    kp = torch.zeros((2, cap, _lib.KP_STRIDE), dtype=torch.float32, device="cuda")
    desc = torch.zeros((2, cap, _lib.DESC_BYTES), dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    rc = ctx.L.fvo_orb_detect_compute(ctx.h, _lib._ptr(dev[o:]), 2, stride, pitch, _lib._ptr(kp), _lib._ptr(desc),
                                      _lib._ptr(cnt), cap, _lib._stream(ctx.device))
    assert rc == 0, ctx.L.fvo_last_error(ctx.h).decode()
    torch.cuda.synchronize()
    n = cnt.cpu().numpy()
    for i, (rkp, rdesc) in enumerate(refs):
        assert n[i] == len(rkp), f"{layout} image {i}: {n[i]} keypoints, oracle {len(rkp)}"
        assert np.array_equal(kp[i, :n[i], :6].cpu().numpy(), rkp)
        assert np.array_equal(desc[i, :n[i]].cpu().numpy(), rdesc)
    assert np.array_equal(dev.cpu().numpy(), host), "the caller's buffer changed"


def test_bad_pitch_and_stride_are_refused_before_any_launch():
    """pitch < width and image_stride < pitch * height: both entry points return an error with
    fvo_last_error set, and the outputs keep their sentinel (nothing was launched)."""
    from forest_slam_amd import _lib
    W, H = 320, 200
    ctx = _lib.Context(W, H, max_batch=2, num_disparities=64, nfeatures=300, stages=_lib.STAGE_SGBM | _lib.STAGE_ORB)
    img = torch.zeros((2 * (W + 16) * H + 64,), dtype=torch.uint8, device="cuda")
    stream = _lib._stream(ctx.device)
    for pitch, stride in ((W - 1, W * H), (W, W * H - 1), (W + 16, W * H)):
        out = torch.full((2, H, W), 1234, dtype=torch.int16, device="cuda")
        st = torch.full((2,), 7, dtype=torch.int32, device="cuda")
        rc = ctx.L.fvo_sgbm(ctx.h, _lib._ptr(img), _lib._ptr(img), 2, stride, pitch, _lib._ptr(out), _lib._ptr(st),
                            stream)
        assert rc != 0 and b"pitch/stride" in ctx.L.fvo_last_error(ctx.h)
        torch.cuda.synchronize()
        assert bool((out == 1234).all()) and st.tolist() == [7, 7]
        cap = ctx.kp_cap
        kp = torch.full((2, cap, _lib.KP_STRIDE), -5.0, dtype=torch.float32, device="cuda")
        desc = torch.full((2, cap, _lib.DESC_BYTES), 0x5A, dtype=torch.uint8, device="cuda")
        cnt = torch.full((2,), -9, dtype=torch.int32, device="cuda")
        rc = ctx.L.fvo_orb_detect_compute(ctx.h, _lib._ptr(img), 2, stride, pitch, _lib._ptr(kp), _lib._ptr(desc),
                                          _lib._ptr(cnt), cap, stream)
        assert rc != 0 and b"pitch/stride" in ctx.L.fvo_last_error(ctx.h)
        torch.cuda.synchronize()
        assert cnt.tolist() == [-9, -9] and bool((kp == -5.0).all()) and bool((desc == 0x5A).all())
