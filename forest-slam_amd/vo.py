"""Batched stereo-VO front end + local BA on the GPU — the ORB branch of ros_ws/src/stereo_slam.py.

One ``StereoFrontEnd.step`` processes B consecutive stereo frames of one sequence in a
fixed sequence of HIP launches (no host synchronisation inside):

  ORB on the B current left + B current right images          (stereo_slam.py:232-233,240-241)
  BF cross-check match prev->cur, left and right (right unused,
  kept for work-equivalence with the reference)                (:234,242)
  SGBM of the B *previous* stereo pairs                         (:262 -> :108-117)
  back-projection of the matched previous-left keypoints        (:265-289)
  (depth="sparse": instead of the two, the per-keypoint stereo records of the current pairs from
  their left-right ORB matches, fvo_sparse_stereo, and the back-projection through the records
  of the previous-left frames -- no disparity map and no SGBM workspace)
  PnP-RANSAC + Rodrigues -> relative T                          (:292-303)
  local BA over the last K frames of every new frame            (north_star; oracle/ba_ref.py)

Frames of a sequence are independent except through the chained pose (:306), which the
host composes left to right in float64 (``eval.chain``), so batching B frames per step is
exact.  The previous image / keypoints of the last frame are carried to
the next step, and the BA keeps the per-frame keypoints, matches, stereo points and PnP
transforms of the last K-1 frames as history so that every window spans K frames
regardless of where the step boundaries fall.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


# step() status codes: 1 pose valid, 0 RANSAC failed, -1 skipped (< 6 points, the reference's
# guard at stereo_slam.py:292), STATUS_KP_OVERFLOW: an image of the pair had more ORB keypoints
# than the context's kp_capacity (no result; raise kp_capacity).
STATUS_KP_OVERFLOW = -3
# ... STATUS_SGBM_FAILED: the pair's SGBM hand-off timed out (only under sgbm_mode=SGBM_LPATH;
# fvo_sgbm status SGBM_HANDOFF_TIMEOUT), so it has no disparities and no pose.
STATUS_SGBM_FAILED = -4


def _match_ratio(match_ratio) -> float:
    r = float(match_ratio)
    if not (np.isfinite(r) and r >= 0.0):
        raise ValueError("match_ratio must be finite and >= 0 (0 = cross-check only)")
    return r


def _match(ctx, match_ratio, d0, n0, d1, n1, out):
    """The front ends' matcher: cross-checked nearest neighbours (the reference's BFMatcher), and
    with match_ratio > 0 only those that also pass Lowe's ratio test against the runner-up.  The
    mutual form keeps the matches injective in trainIdx, which the BA's landmark chaining needs."""
    if match_ratio > 0.0:
        return ctx.bf_ratio_match(d0, n0, d1, n1, match_ratio, mutual=True, out=out)
    return ctx.bf_match(d0, n0, d1, n1, out=out)


class StereoFrontEnd:
    def __init__(self, width: int, height: int, K: np.ndarray, dist: np.ndarray, baseline: float, batch: int,
                 nfeatures: int = 500, match_right: bool = True, device=None, ba_window: int = 10,
                 ba_iters: int = 10, overlap_sgbm: bool = False, sgbm_last: bool = False, births_ahead: bool = False,
                 speckle_window: int = 0, speckle_range: int = 0, match_ratio: float = 0.0, depth: str = "sgbm",
                 sparse_params: dict | None = None, **params):
        if depth not in ("sgbm", "sparse"):
            raise ValueError('depth must be "sgbm" or "sparse"')
        self.sparse = depth == "sparse"
        if self.sparse and speckle_window:
            raise ValueError('depth="sparse" computes no disparity map: speckle_window does not apply')
        self.B = batch
        self.match_ratio = _match_ratio(match_ratio)
        self.K = np.asarray(K, np.float64)
        self.dist = np.resize(np.asarray(dist, np.float64), 5)
        self.baseline = float(baseline)
        self.match_right = match_right
        self.ba_window = int(ba_window)
        self.ba_iters = int(ba_iters)
        stages = _lib.STAGE_ORB | _lib.STAGE_BF | _lib.STAGE_POSE | (0 if self.sparse else _lib.STAGE_SGBM)
        if self.ba_window:
            stages |= _lib.STAGE_BA
            params.setdefault("ba_window", self.ba_window)
        if not self.sparse:
            params.setdefault("sgbm_max_batch", batch)  # SGBM runs on the step's B pairs (ORB on 2B images)
        self.ctx = _lib.Context(width, height, max_batch=2 * batch, device=device, nfeatures=nfeatures,
                                stages=stages, **params)
        self.dev = self.ctx.device
        self.cap = self.ctx.kp_cap
        self.W, self.H = width, height
        B, cap, dev = batch, self.cap, self.dev
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        # persistent device buffers (no allocation inside step).  The per-step front-stage
        # outputs (images, ORB, BF, SGBM) have two slots: with overlap_sgbm the front stage of
        # step k+1 fills one slot while the back stage of step k reads the other.
        two = lambda shape, dt: [e(shape, dt), e(shape, dt)]  # noqa: E731
        self.kp_buf = two((2 * B, cap, _lib.KP_STRIDE), torch.float32)
        self.desc_buf = two((2 * B, cap, _lib.DESC_BYTES), torch.uint8)
        self.cnt_buf = two((2 * B,), torch.int32)
        self.q_desc = e((2 * B, cap, _lib.DESC_BYTES), torch.uint8)
        self.q_cnt_buf = two((2 * B,), torch.int32)
        self.q_kp_buf = two((B, cap, _lib.KP_STRIDE), torch.float32)
        self.matches_buf = two((2 * B, cap, 3), torch.int32)
        self.nmatch_buf = two((2 * B,), torch.int32)
        if self.sparse:
            # the sparse records (X, Y, Z, d per left keypoint) of the step's current pairs, of the
            # last pair (kept across steps, written by prime()) and of the step's previous-left
            # frames: the last pair's, then the current ones' [:n-1] -- q_kp's order.  The back
            # stage and the BA read the latter, so it has two slots like q_kp.
            self.sparse_params = self.ctx.sparse_stereo_params(**(sparse_params or {}))
            self.level_scale = self.ctx.level_scales()
            self.cur_stereo = torch.zeros((B, cap, 4), dtype=torch.float32, device=dev)
            self.last_stereo = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
            self.q_stereo_buf = [torch.zeros((B, cap, 4), dtype=torch.float32, device=dev) for _ in range(2)]
            self.sparse_ws = e((self.ctx.sparse_stereo_workspace_bytes(B, cap),), torch.uint8)
        self.prevL = None if self.sparse else e((B, height, width), torch.uint8)
        self.prevR = None if self.sparse else e((B, height, width), torch.uint8)
        self.disp_buf = [None, None] if self.sparse else two((B, height, width), torch.int16)
        self.sg_status_buf = [None, None] if self.sparse else two((B,), torch.int32)
        self.sgbm_can_fail = not self.sparse and int(self.ctx.cfg.sgbm_mode) == _lib.SGBM_LPATH
        # StereoSGBM_create(speckleWindowSize=, speckleRange=): cv2.filterSpeckles on the step's
        # disparity maps right after SGBM (0 = off, the reference's setting: no launch).  Its
        # scratch is used on the front stage's stream only, so one allocation serves both slots.
        self.speckle_window, self.speckle_range = int(speckle_window), int(speckle_range)
        self.speckle_new_val = (int(self.ctx.cfg.min_disparity) - 1) * 16
        self.speckle_ws = (torch.empty((self.ctx.speckle_workspace_bytes(B, height, width),), dtype=torch.uint8,
                                       device=dev) if self.speckle_window > 0 else None)
        # the BA's per-keypoint stereo points of the step's previous-left frames, computed in the
        # front stage (they need only its disparities and keypoints) into a slot like disp
        # (depth="sparse": they ARE the records of the previous-left frames, so kstereo and q_stereo
        # name the same two slots and no fvo_keypoint_stereo is launched)
        self.kstereo_buf = (self.q_stereo_buf if self.sparse else
                            two((B, cap, 4), torch.float32) if self.ba_window else [None, None])
        self._select(0)
        self.P3 = e((B, cap, 3), torch.float32)
        self.p2 = e((B, cap, 2), torch.float32)
        self.npts = e((B,), torch.int32)
        self.rvec = e((B, 3), torch.float64)
        self.tvec = e((B, 3), torch.float64)
        self.T = e((B, 4, 4), torch.float64)
        self.status = e((B,), torch.int32)
        self.inl = e((B, cap), torch.uint8)
        self.imgs = e((2 * B, height, width), torch.uint8)
        self.last_kp = e((cap, _lib.KP_STRIDE), torch.float32)
        self.last_desc = e((2, cap, _lib.DESC_BYTES), torch.uint8)
        self.last_cnt = e((2,), torch.int32)
        if self.ba_window:
            Kw = self.ba_window
            F = Kw - 1 + B  # history slots [0, K-1) + the step's frames
            self.hkp = e((F, cap, _lib.KP_STRIDE), torch.float32)
            self.hnkp = torch.zeros((F,), dtype=torch.int32, device=dev)
            self.hmatch = e((F, cap, 3), torch.int32)
            self.hnmatch = torch.zeros((F,), dtype=torch.int32, device=dev)
            self.hstereo = e((F, cap, 4), torch.float32)
            self.hT = torch.zeros((F, 4, 4), dtype=torch.float64, device=dev)
            self.T_ba = e((B, 4, 4), torch.float64)
            self.ba_stats = e((B, 6), torch.float64)
            self.valid_from = Kw - 2
        # overlap_sgbm: the front stage (SGBM of the previous pairs, ORB + BF of the new frames
        # -- throughput-bound) runs on its own stream into double-buffered outputs, so the front
        # stage of step k+1 overlaps the back stage (back-projection, PnP, local BA -- latency-
        # bound) of step k, which runs on the caller's stream and joins the front stage first.
        # The step inputs must then be complete when step() is called (resident in HBM, or
        # pass inputs_ready).  Default: everything in order on the caller's stream.
        # Under HIP-graph capture the front stage forks from the captured step's own start, so a
        # replayed graph runs the step without the cross-step overlap (front stage of step k+1
        # beside the back stage of step k): capture is for launch-bound callers, not for speed.
        self.overlap_sgbm = bool(overlap_sgbm)
        # front-stage order: SGBM first (default), or ORB + BF first and SGBM last (the previous
        # step's back stage then starts beside the small ORB / BF blocks instead of SGBM's)
        self.sgbm_last = bool(sgbm_last)
        self.s_sgbm = torch.cuda.Stream(dev) if self.overlap_sgbm else None
        # births_ahead: local BA's birth counting (fvo_ba_count_births) on its own stream beside PnP
        # -- it needs the step's matches and stereo points only, and in the back stage's chain its
        # launch waits for room beside the next front stage's SGBM waves (r6 VERDICT item 4).
        # Measured slower on the overlapped bench (5632-5667 vs 5689-5705 frames/s), so off by
        # default; bit-identical either way (tests/test_frontend_gpu.py)
        self.s_births = torch.cuda.Stream(dev) if (self.ba_window and births_ahead) else None
        # prime() runs on the caller's stream: the first front stage after it waits for it
        self.primed = None
        self.sg_lastL = None if self.sparse else e((height, width), torch.uint8)
        self.sg_lastR = None if self.sparse else e((height, width), torch.uint8)
        self.main_done = [None, None]
        self.k = 0
        self.has_prev = False

    def prime(self, L0: torch.Tensor, R0: torch.Tensor):
        """Feed the first stereo pair of a sequence (no pose is produced for it)."""
        imgs = torch.stack([L0, R0]).to(self.dev)
        kp, desc, cnt = self.ctx.orb(imgs)
        if self.sparse:
            self._sparse_stereo(imgs, kp, desc, cnt, 1, self.last_stereo[None])
        else:
            self.sg_lastL.copy_(imgs[0])
            self.sg_lastR.copy_(imgs[1])
        self.last_kp.copy_(kp[0])
        self.last_desc.copy_(desc[:2])
        self.last_cnt.copy_(cnt[:2])
        if self.ba_window:
            Kw = self.ba_window
            self.hkp[Kw - 2].copy_(kp[0])
            self.hnkp[Kw - 2:Kw - 1].copy_(cnt[0:1].clamp(min=0))  # clamped like count_guard's output
            self.valid_from = Kw - 2
        self.has_prev = True
        # prime's kernels and copies (ORB, last_*) are queued on the caller's stream; the next
        # front stage reads their outputs on the front stream, so it waits for this event
        self.primed = torch.cuda.current_stream(self.dev).record_event() if self.overlap_sgbm else None

    def step(self, L: torch.Tensor, R: torch.Tensor, inputs_ready=None):
        """L, R: u8 [n,H,W] device tensors, n <= B consecutive frames after the primed/last
        pair.  Returns (T f64[n,4,4], status i32[n]) device tensors (async): the BA-refined
        relative transforms when local BA is enabled, else the PnP ones (``self.T``)."""
        if not self.has_prev:
            raise RuntimeError("call prime() with the first stereo pair first")
        n = L.shape[0]
        B = self.B
        if n > B:
            raise ValueError("more frames than the configured batch")
        ctx = self.ctx
        main = torch.cuda.current_stream(self.dev)
        slot = self.k % 2
        self._select(slot)
        fs = self.s_sgbm if self.overlap_sgbm else main
        capturing = torch.cuda.is_current_stream_capturing()
        if self.overlap_sgbm:
            if capturing:
                # inside a HIP graph the front stage forks from the step's own start (graph
                # replays are stream-ordered, so no earlier step still reads its slot)
                fs.wait_stream(main)
            else:
                if self.primed is not None:  # the first step after prime(): its outputs first
                    fs.wait_event(self.primed)
                    self.primed = None
                if inputs_ready is not None:
                    fs.wait_event(inputs_ready)
                if self.main_done[slot] is not None:  # the back stage of step k-2 read this slot
                    fs.wait_event(self.main_done[slot])
                L.record_stream(fs)
                R.record_stream(fs)
        with torch.cuda.stream(fs):
            # ---- front stage: SGBM of the previous pairs (needs only images), ORB + BF.  The
            # step's buffer moves go in three batched launches (fvo_copy_regions) instead of a
            # dozen separate copies: (A) the SGBM pairs and the ORB images, (B) after ORB the
            # query sets (previous descriptors / counts / keypoints) and the last images,
            # (C) after BF the last frame's keypoints / descriptors / counts
            ctx.copy_regions(([] if self.sparse else self._sgbm_pairs(L, R, n)) +
                             [(self.imgs[:n], L), (self.imgs[n:2 * n], R)])
            # SGBM first: ORB + BF first measured slower (r3 4242 vs 4284, r4 5051 vs 5227 frames/s)
            if not self.sgbm_last and not self.sparse:
                disp = self._sgbm(n)
            kp, desc, cnt = ctx.orb(self.imgs[:2 * n], out=(self.kp[:2 * n], self.desc[:2 * n], self.cnt[:2 * n]))
            # query (previous) sets: left frames then right frames; previous-left keypoints
            ctx.copy_regions([(self.q_desc[0], self.last_desc[0]), (self.q_cnt[0:1], self.last_cnt[0:1]),
                              (self.q_desc[1:n], desc[:n - 1]), (self.q_cnt[1:n], cnt[:n - 1]),
                              (self.q_desc[n], self.last_desc[1]), (self.q_cnt[n:n + 1], self.last_cnt[1:2]),
                              (self.q_desc[n + 1:2 * n], desc[n:2 * n - 1]), (self.q_cnt[n + 1:2 * n], cnt[n:2 * n - 1]),
                              (self.q_kp[0], self.last_kp), (self.q_kp[1:n], kp[:n - 1])] +
                             ([] if self.sparse else [(self.sg_lastL, L[n - 1]), (self.sg_lastR, R[n - 1])]))
            nb = 2 * n if self.match_right else n
            m, nm = _match(ctx, self.match_ratio, self.q_desc[:nb], self.q_cnt[:nb], desc[:nb], cnt[:nb],
                           out=(self.matches[:nb], self.nmatch[:nb]))
            ctx.copy_regions([(self.last_kp, kp[n - 1]), (self.last_desc[0], desc[n - 1]),
                              (self.last_desc[1], desc[2 * n - 1]), (self.last_cnt[0:1], cnt[n - 1:n]),
                              (self.last_cnt[1:2], cnt[2 * n - 1:2 * n])])
            if self.sparse:
                # the current pairs' records; the previous-left frames' are the last pair's, then
                # these [:n-1]; the last pair's is replaced only after it was read
                self._sparse_stereo(self.imgs, kp, desc, cnt, n, self.cur_stereo[:n])
                ctx.copy_regions([(self.q_stereo[0], self.last_stereo), (self.q_stereo[1:n], self.cur_stereo[:n - 1])])
                ctx.copy_regions([(self.last_stereo, self.cur_stereo[n - 1])])
                disp = None
            elif self.sgbm_last:
                disp = self._sgbm(n)
            if self.ba_window and not self.sparse:  # (a negative count -- ORB overflow -- reads as no keypoints)
                ctx.keypoint_stereo(disp[:n], self.q_kp[:n], self.q_cnt[:n], self.K, self.baseline,
                                    out=self.kstereo[:n])
        if self.overlap_sgbm:
            main.wait_stream(fs)
        # ---- back stage: back-projection, PnP, local BA.  The BA history's frame data (everything
        # but the PnP transforms) is in place before PnP, and the BA's birth counting starts on a
        # side stream right away
        births = self._ba_births(n, kp, m, nm) if self.ba_window else None  # (None without births_ahead)
        if self.sparse:
            P3, p2, npts = ctx.backproject_stereo(self.q_stereo[:n], kp[:n], m[:n], nm[:n],
                                                  out=(self.P3[:n], self.p2[:n], self.npts[:n]))
        else:
            P3, p2, npts = ctx.backproject(disp, self.q_kp[:n], kp[:n], m[:n], nm[:n], self.K, self.baseline,
                                           out=(self.P3[:n], self.p2[:n], self.npts[:n]))
        rv, tv, T, st, _ = ctx.pnp_ransac(P3, p2, npts, self.K, self.dist,
                                          out=(self.rvec[:n], self.tvec[:n], self.T[:n], self.status[:n],
                                               self.inl[:n]))
        # ORB writes -(needed) when a frame has more keypoints than kp_capacity (its outputs
        # are then unspecified): mark the frame STATUS_KP_OVERFLOW instead of letting it pass
        # as a "fewer than 6 points" skip (device-side, no host sync; the right sets feed
        # bf_match too).  An overflowed frame enters the BA history as a frame without
        # keypoints (clamped count): the BA kernels never see a negative count.
        ctx.count_guard(cnt, n, 2 if self.match_right else 1, q_counts=self.q_cnt, status=st,
                        code=STATUS_KP_OVERFLOW,
                        clamped_out=self.hnkp[self.ba_window - 1:self.ba_window - 1 + n] if self.ba_window else None)
        if self.sgbm_can_fail:  # the L-path schedule's dropped pairs (classic SGBM cannot fail)
            ctx.count_guard(self.sg_status[:n], n, 1, status=st, code=STATUS_SGBM_FAILED)
        out = T
        if self.ba_window:
            out = self._local_ba(n, T, births)
        if self.overlap_sgbm and not capturing:
            self.main_done[slot] = main.record_event()
        self.k += 1
        return out, st

    def append_dense(self, point_map, cum, **kw):
        """Dense stereo mapping of the step just run: ``point_map.add_disparity`` on its disparity
        maps (``self.disp[:n]``, of the step's previous pairs -- frame i's points3D come from the
        same map) with cum f64 [n,4,4], on the current stream; kw: add_disparity's (step,
        min_disp16, z_max, keep, ...).  Returns n_added.

        self.disp is one of two slots; with overlap_sgbm the front stage of step k+2 overwrites it
        after waiting for main_done[slot], recorded at the end of step() -- before these launches
        -- so it is recorded again behind them (not under capture, where step() records none)."""
        if self.sparse:
            raise RuntimeError('append_dense: depth="sparse" computes no disparity map')
        n = int(cum.shape[0])
        if self.k == 0 or n > self.B:
            raise RuntimeError("append_dense: call it after step(), with that step's n poses")
        n_added = point_map.add_disparity(self.disp[:n], self.K, self.baseline, cum, **kw)
        if self.overlap_sgbm and not torch.cuda.is_current_stream_capturing():
            self.main_done[(self.k - 1) % 2] = torch.cuda.current_stream(self.dev).record_event()
        return n_added

    def _sparse_stereo(self, imgs, kp, desc, cnt, n, out):
        """fvo_sparse_stereo of n pairs laid out as ORB's batch (left images / sets [:n], right
        [n:2n]) into out [n,cap,4], on the current stream.  (A negative count -- ORB overflow --
        reads as no keypoints.)"""
        self.ctx.sparse_stereo(imgs[:n], imgs[n:2 * n], kp[:n], cnt[:n], desc[:n], kp[n:2 * n], cnt[n:2 * n],
                               desc[n:2 * n], self.K, self.baseline, params=self.sparse_params,
                               level_scale=self.level_scale, workspace=self.sparse_ws, out=out)

    def _sgbm(self, n):
        """SGBM of the step's previous pairs, then the speckle filter when it is enabled
        (StereoSGBM::compute's order), on the current stream."""
        disp = self.ctx.sgbm(self.prevL[:n], self.prevR[:n], out=self.disp[:n], status=self.sg_status[:n])
        if self.speckle_window > 0:
            self.ctx.filter_speckles(disp, self.speckle_new_val, self.speckle_window, 16 * self.speckle_range,
                                     workspace=self.speckle_ws)
        return disp

    def _sgbm_pairs(self, L, R, n):
        """Copy list for SGBM's previous pairs (the last pair of the previous step, then
        L/R[:n-1])."""
        return [(self.prevL[0], self.sg_lastL), (self.prevR[0], self.sg_lastR),
                (self.prevL[1:n], L[:n - 1]), (self.prevR[1:n], R[:n - 1])]

    def _select(self, slot: int):
        """Point the per-step buffer names at one of the two slots."""
        self.kp, self.desc, self.cnt = self.kp_buf[slot], self.desc_buf[slot], self.cnt_buf[slot]
        self.q_cnt, self.q_kp = self.q_cnt_buf[slot], self.q_kp_buf[slot]
        self.matches, self.nmatch = self.matches_buf[slot], self.nmatch_buf[slot]
        self.disp = self.disp_buf[slot]
        self.sg_status = self.sg_status_buf[slot]
        self.kstereo = self.kstereo_buf[slot]
        self.q_stereo = self.q_stereo_buf[slot] if self.sparse else None

    def _ba_births(self, n, kp, m, nm):
        """The step's frames into the BA history (keypoints, matches, stereo points; the PnP
        transforms follow in _local_ba) and fvo_ba_count_births on the side stream; returns the
        event _local_ba's BA call waits for."""
        Kw, ctx = self.ba_window, self.ctx
        a, b = Kw - 2, Kw - 1  # first pair slot, first new-frame slot
        ctx.copy_regions([(self.hkp[b:b + n], kp[:n]), (self.hmatch[a:a + n], m[:n]),
                          (self.hnmatch[a:a + n], nm[:n]), (self.hstereo[a:a + n], self.kstereo[:n])])
        F = b + n
        sb = self.s_births
        if sb is None:  # births_ahead=False: fvo_ba_windows counts them itself, in its chain
            return None
        sb.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(sb):
            ctx.ba_count_births(self.hmatch[:F], self.hnmatch[:F], self.hstereo[:F], b, n, self.valid_from)
            return sb.record_event()

    def _local_ba(self, n, T, births):
        Kw, ctx = self.ba_window, self.ctx
        a, b = Kw - 2, Kw - 1  # first pair slot, first new-frame slot
        # (hnkp[b:b+n], the clamped counts, came from count_guard; the rest of the frame data from
        # _ba_births)
        ctx.copy_regions([(self.hT[a:a + n], T[:n])])
        if births is not None:
            torch.cuda.current_stream(self.dev).wait_event(births)
        F = b + n
        Tba, _ = ctx.ba_windows(self.hkp[:F], self.hnkp[:F], self.hmatch[:F], self.hnmatch[:F], self.hstereo[:F],
                                self.hT[:F], b, n, self.valid_from, self.K, self.baseline, iterations=self.ba_iters,
                                out=(self.T_ba[:n], self.ba_stats[:n]))
        # slide the history: frames [n, n+K-1) -> [0, K-1), pair data [n, n+K-2) -> [0, K-2);
        # one launch when source and destination do not overlap (n >= K-1), else via clones
        slides = [(self.hkp, b), (self.hnkp, b)] + ([(t, a) for t in (self.hmatch, self.hnmatch, self.hstereo, self.hT)]
                                                    if a > 0 else [])
        if n >= b:
            ctx.copy_regions([(t[:k], t[n:n + k]) for t, k in slides])
        else:
            for t, k in slides:
                t[:k].copy_(t[n:n + k].clone())
        self.valid_from = max(0, self.valid_from - n)
        return Tba


def _check_overflow(st: np.ndarray):
    bad = np.nonzero(st == STATUS_KP_OVERFLOW)[0]
    if len(bad):
        raise RuntimeError(f"ORB keypoint capacity exceeded on frame pair(s) {bad[:8].tolist()}: "
                           "create the front end with a larger kp_capacity")


def run_sequence(frontend: StereoFrontEnd, L_all: torch.Tensor, R_all: torch.Tensor, stamps=None,
                 use_ba: bool = True):
    """Process a whole sequence (images on device) -> (TUM rows, relative poses, statuses).
    With local BA enabled the chain uses the BA-refined relative transforms (``use_ba``)."""
    from . import eval as ev
    n = L_all.shape[0]
    frontend.prime(L_all[0], R_all[0])
    Ts, sts = [], []
    for s in range(1, n, frontend.B):
        e = min(s + frontend.B, n)
        T, st = frontend.step(L_all[s:e], R_all[s:e])
        if not use_ba:
            T = frontend.T[:e - s]
        Ts.append(T.cpu().numpy())
        sts.append(st.cpu().numpy())
    T = np.concatenate(Ts) if Ts else np.zeros((0, 4, 4))
    st = np.concatenate(sts) if sts else np.zeros((0,), np.int32)
    _check_overflow(st)
    # status -1 = fewer than 6 points: the reference skips the frame (no pose, no TUM row,
    # stereo_slam.py:292); status 0 = RANSAC failure: identity T (the reference would chain
    # whatever solvePnPRansac left in rvec/tvec), row emitted; STATUS_SGBM_FAILED (the pair had no
    # disparities) is skipped like -1.
    valid = (st != -1) & (st != STATUS_SGBM_FAILED)
    cum = ev.chain(T, valid)
    if stamps is None:
        stamps = np.arange(n, dtype=np.float64)
    rows = ev.tum_rows(np.asarray(stamps)[1:][valid], cum)
    return rows, T, st


class MonoFrontEnd:
    """Batched mono VO on the GPU — the ORB variant of ros_ws/src/mono_slam.py:97-118
    (SURVEY.md §8 a16): per frame pair ORB on the current image, BF cross-check
    previous -> current, mkpts gather (:106-108), findEssentialMat(RANSAC, 0.999, 1.0)
    (:111), recoverPose (:112) and T = [R | t] (:114-117).  The chain (:118) is composed on
    the host (``eval.chain``); translations are unit-norm (mono is scale-free).

    ``step`` status per frame: 1 pose valid; 0 RANSAC found no model, -1 fewer than 5
    matches, -2 five matches with several solutions, -3 (STATUS_KP_OVERFLOW) keypoint
    capacity exceeded — the cases where the reference's
    cv2.recoverPose would raise; T is the identity there."""

    def __init__(self, width: int, height: int, K: np.ndarray, batch: int, nfeatures: int = 500, device=None,
                 prob: float = 0.999, threshold: float = 1.0, overlap: bool = False, match_ratio: float = 0.0,
                 **params):
        self.B = batch
        self.match_ratio = _match_ratio(match_ratio)
        self.K = np.asarray(K, np.float64)
        self.focal = float(self.K[0, 0])
        self.pp = (float(self.K[0, 2]), float(self.K[1, 2]))
        self.prob, self.threshold = float(prob), float(threshold)
        stages = _lib.STAGE_ORB | _lib.STAGE_BF | _lib.STAGE_MONO
        self.ctx = _lib.Context(width, height, max_batch=batch, device=device, nfeatures=nfeatures, stages=stages,
                                **params)
        self.dev = self.ctx.device
        self.cap = cap = self.ctx.kp_cap
        B, dev = batch, self.dev
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        # overlap: the front stage (ORB + BF, throughput-bound) of step k+1 runs on its own
        # stream beside the back stage (gather, essential-matrix RANSAC, recoverPose --
        # latency-bound) of step k, as StereoFrontEnd(overlap_sgbm=True) does; the front
        # stage's outputs then have two slots.  Identical results either way.
        self.overlap = bool(overlap)
        two = lambda shape, dt: [e(shape, dt), e(shape, dt)]  # noqa: E731
        self.kp_buf = two((B, cap, _lib.KP_STRIDE), torch.float32)
        self.desc_buf = two((B, cap, _lib.DESC_BYTES), torch.uint8)
        self.cnt_buf = two((B,), torch.int32)
        self.q_kp_buf = two((B, cap, _lib.KP_STRIDE), torch.float32)
        self.q_cnt_buf = two((B,), torch.int32)
        self.matches_buf = two((B, cap, 3), torch.int32)
        self.nmatch_buf = two((B,), torch.int32)
        self.q_desc = e((B, cap, _lib.DESC_BYTES), torch.uint8)
        self._select(0)
        self.p0 = e((B, cap, 2), torch.float32)
        self.p1 = e((B, cap, 2), torch.float32)
        self.npts = e((B,), torch.int32)
        self.E = e((B, 3, 3), torch.float64)
        self.mask = e((B, cap), torch.uint8)
        self.status = e((B,), torch.int32)
        self.R = e((B, 3, 3), torch.float64)
        self.t = e((B, 3), torch.float64)
        self.T = e((B, 4, 4), torch.float64)
        self.ngood = e((B,), torch.int32)
        self.last_kp = e((cap, _lib.KP_STRIDE), torch.float32)
        self.last_desc = e((cap, _lib.DESC_BYTES), torch.uint8)
        self.last_cnt = e((1,), torch.int32)
        self.s_front = torch.cuda.Stream(dev) if self.overlap else None
        self.primed = None
        self.main_done = [None, None]
        self.k = 0
        self.has_prev = False

    def _select(self, slot: int):
        self.kp, self.desc, self.cnt = self.kp_buf[slot], self.desc_buf[slot], self.cnt_buf[slot]
        self.q_kp, self.q_cnt = self.q_kp_buf[slot], self.q_cnt_buf[slot]
        self.matches, self.nmatch = self.matches_buf[slot], self.nmatch_buf[slot]

    def prime(self, img0: torch.Tensor):
        kp, desc, cnt = self.ctx.orb(img0.to(self.dev)[None])
        self.last_kp.copy_(kp[0])
        self.last_desc.copy_(desc[0])
        self.last_cnt.copy_(cnt[:1])
        self.has_prev = True
        self.primed = torch.cuda.current_stream(self.dev).record_event() if self.overlap else None

    def step(self, imgs: torch.Tensor, inputs_ready=None):
        """imgs: u8 [n,H,W] device tensor of the next n <= B selected frames.  Returns
        (T f64[n,4,4], status i32[n]) device tensors (async).  With overlap the images must
        be complete when step() is called (or pass inputs_ready, an event)."""
        if not self.has_prev:
            raise RuntimeError("call prime() with the first frame first")
        n, ctx = imgs.shape[0], self.ctx
        if n > self.B:
            raise ValueError("more frames than the configured batch")
        main = torch.cuda.current_stream(self.dev)
        slot = self.k % 2
        self._select(slot)
        fs = self.s_front if self.overlap else main
        capturing = torch.cuda.is_current_stream_capturing()
        if self.overlap:
            if capturing:
                fs.wait_stream(main)
            else:
                if self.primed is not None:
                    fs.wait_event(self.primed)
                    self.primed = None
                if inputs_ready is not None:
                    fs.wait_event(inputs_ready)
                if self.main_done[slot] is not None:  # the back stage of step k-2 read this slot
                    fs.wait_event(self.main_done[slot])
                imgs.record_stream(fs)
        with torch.cuda.stream(fs):
            # ---- front stage: ORB of the new frames, query sets, BF (buffer moves batched)
            kp, desc, cnt = ctx.orb(imgs, out=(self.kp[:n], self.desc[:n], self.cnt[:n]))
            ctx.copy_regions([(self.q_kp[0], self.last_kp), (self.q_desc[0], self.last_desc),
                              (self.q_cnt[0:1], self.last_cnt), (self.q_kp[1:n], kp[:n - 1]),
                              (self.q_desc[1:n], desc[:n - 1]), (self.q_cnt[1:n], cnt[:n - 1])])
            m, nm = _match(ctx, self.match_ratio, self.q_desc[:n], self.q_cnt[:n], desc, cnt,
                           out=(self.matches[:n], self.nmatch[:n]))
            ctx.copy_regions([(self.last_kp, kp[n - 1]), (self.last_desc, desc[n - 1]),
                              (self.last_cnt, cnt[n - 1:n])])
        if self.overlap:
            main.wait_stream(fs)
        # ---- back stage: gather, essential-matrix RANSAC, recoverPose, overflow statuses
        p0, p1, npts = ctx.gather_matches(self.q_kp[:n], kp, m, nm, out=(self.p0[:n], self.p1[:n], self.npts[:n]))
        E, _, st = ctx.find_essential(p0, p1, npts, self.focal, self.pp, self.prob, self.threshold,
                                      out=(self.E[:n], self.mask[:n], self.status[:n]))
        _, _, T, _ = ctx.recover_pose(E, p0, p1, npts, self.focal, self.pp, e_status=st,
                                      out=(self.R[:n], self.t[:n], self.T[:n], self.ngood[:n]))
        ctx.count_guard(cnt, n, 1, q_counts=self.q_cnt, status=st, code=STATUS_KP_OVERFLOW)
        if self.overlap and not capturing:
            self.main_done[slot] = main.record_event()
        self.k += 1
        return T, st


def run_mono_sequence(frontend: MonoFrontEnd, imgs: torch.Tensor, stamps=None, frame_interval: int = 1):
    """mono_slam.py's loop over a sequence: frames with index % frame_interval == 0 form the
    consecutive pairs (:97); returns (TUM rows, relative T, statuses)."""
    from . import eval as ev
    sel = np.arange(0, imgs.shape[0], frame_interval)
    if stamps is None:
        stamps = np.arange(imgs.shape[0], dtype=np.float64)
    frontend.prime(imgs[sel[0]])
    Ts, sts = [], []
    for s in range(1, len(sel), frontend.B):
        idx = sel[s:s + frontend.B]
        T, st = frontend.step(imgs[torch.as_tensor(idx, device=imgs.device)])
        Ts.append(T.cpu().numpy())
        sts.append(st.cpu().numpy())
    T = np.concatenate(Ts) if Ts else np.zeros((0, 4, 4))
    st = np.concatenate(sts) if sts else np.zeros((0,), np.int32)
    _check_overflow(st)
    cum = ev.chain(T, np.ones(len(T), bool))
    rows = ev.tum_rows(np.asarray(stamps)[sel[1:]], cum)
    return rows, T, st
