"""fvo_sgbm against oracle.sgbm, bit for bit, after the median and before it (debug buffer 11),
at the smallest shapes where the cost pass's LDS tile indexing (csrc/sgbm_costmap.h: per-pixel BT
records, pixel-cost task slots, box-sum runs) can go wrong: width1 = W - D columns with a
disparity range of 1 (a single column of a single partial block), 31 and 33 (one column either
side of a 32-column block boundary) and 64 + 21 (full blocks and a ragged last one), each at the
32-row height floor of test_sgbm_minimum_height, for D = 64, 96, 128 under the default launch and
every (lanes, cols) variant; one pitched, strided input; one L-path case."""
import functools

import numpy as np
import pytest
import torch

import sgbm_cases as sc
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

H = 32
WIDTH1 = [1, 31, 33, 64 + 21]
LAUNCHES = {"default": {}, "4x64": dict(sgbm_lanes=4, sgbm_cols=64), "4x32": dict(sgbm_lanes=4, sgbm_cols=32),
            "8x16": dict(sgbm_lanes=8, sgbm_cols=16), "8x32": dict(sgbm_lanes=8, sgbm_cols=32),
            "16x32": dict(sgbm_lanes=16, sgbm_cols=32)}


@functools.lru_cache(maxsize=None)
def _reference(oracle_mod, W, D):
    """(median, raw) int16 [2,H,W] of sgbm_cases.pair_batch(W, H), computed once per shape."""
    L, R = sc.pair_batch(W, H)
    both = [oracle_mod.sgbm(L[i], R[i], num_disp=D, raw=True) for i in range(2)]
    out = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    for a in out:
        a.setflags(write=False)
    return out


def _raw(ctx, B, W):
    return ctx.debug_buffer(11).view(torch.int16).view(-1, H, W)[:B].numpy()


def _assert_equal(got, want, what):
    for i in range(len(want)):
        bad = np.argwhere(got[i] != want[i])
        assert len(bad) == 0, f"{what} image {i}: {len(bad)} px differ, first {bad[:5].tolist()}"


@pytest.mark.parametrize("width1", WIDTH1)
@pytest.mark.parametrize("D", [64, 96, 128])
def test_cost_tile_edges_bit_exact_under_every_launch(oracle_mod, D, width1):
    from forest_slam_amd import _lib
    W = D + width1
    L, R = sc.pair_batch(W, H)
    want, want_raw = _reference(oracle_mod, W, D)
    assert (want_raw[:, :, D:] != -16).any(), "vacuous: the oracle finds no disparity in the valid columns"
    Ld, Rd = torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda()
    for name, launch in LAUNCHES.items():
        ctx = _lib.Context(W, H, max_batch=2, num_disparities=D, stages=_lib.STAGE_SGBM, **launch)
        st = torch.full((2,), 7, dtype=torch.int32, device="cuda")
        got = ctx.sgbm(Ld, Rd, status=st)
        torch.cuda.synchronize()
        assert st.tolist() == [_lib.SGBM_OK] * 2
        _assert_equal(_raw(ctx, 2, W), want_raw, f"{W}x{H}/{D} {name} raw")
        _assert_equal(got.cpu().numpy(), want, f"{W}x{H}/{D} {name} median")
        ctx.close()


def test_cost_tile_pitched_strided_input_bit_exact(oracle_mod):
    """Rows pitch = W + 13 bytes apart and images pitch * H + 7 apart, inside a buffer of 0xA5."""
    from forest_slam_amd import _lib
    D, W = 96, 96 + 64 + 21
    L, R = sc.pair_batch(W, H)
    want, want_raw = _reference(oracle_mod, W, D)
    pitch = W + 13
    stride = pitch * H + 7
    host = np.full(3 + 4 * stride + 64, 0xA5, np.uint8)
    offs = []
    for g, imgs in enumerate((L, R)):
        offs.append(3 + g * 2 * stride)
        for b in range(2):
            rows = np.lib.stride_tricks.as_strided(host[offs[g] + b * stride:], shape=(H, W), strides=(pitch, 1))
            rows[:] = imgs[b]
    dev = torch.from_numpy(host.copy()).cuda()
    ctx = _lib.Context(W, H, max_batch=2, num_disparities=D, stages=_lib.STAGE_SGBM)
    out = torch.empty((2, H, W), dtype=torch.int16, device="cuda")
    st = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    rc = ctx.L.fvo_sgbm(ctx.h, _lib._ptr(dev[offs[0]:]), _lib._ptr(dev[offs[1]:]), 2, stride, pitch, _lib._ptr(out),
                        _lib._ptr(st), _lib._stream(ctx.device))
    assert rc == 0, ctx.L.fvo_last_error(ctx.h).decode()
    torch.cuda.synchronize()
    assert st.tolist() == [_lib.SGBM_OK] * 2
    _assert_equal(_raw(ctx, 2, W), want_raw, "pitched raw")
    _assert_equal(out.cpu().numpy(), want, "pitched median")
    assert np.array_equal(dev.cpu().numpy(), host), "the caller's buffer changed"
    ctx.close()


def test_cost_tile_lpath_bit_exact(oracle_mod):
    """The L-path schedule over three column blocks (two hand-offs, a ragged last block)."""
    from forest_slam_amd import _lib
    D, W = 96, 96 + 64 + 21
    L, R = sc.pair_batch(W, H)
    want, want_raw = _reference(oracle_mod, W, D)
    ctx = _lib.Context(W, H, max_batch=2, num_disparities=D, stages=_lib.STAGE_SGBM, sgbm_mode=_lib.SGBM_LPATH)
    st = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    got = ctx.sgbm(torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda(), status=st)
    torch.cuda.synchronize()
    assert st.tolist() == [_lib.SGBM_OK] * 2
    assert ctx.debug_buffer(9).view(torch.int32).numpy()[2] == 0  # no hand-off timed out
    _assert_equal(_raw(ctx, 2, W), want_raw, "lpath raw")
    _assert_equal(got.cpu().numpy(), want, "lpath median")
    ctx.close()
