"""ctypes binding of libfvo.so (include/fvo.h) with torch tensors as the buffer type.

The product path: every call lands in a hand-written HIP kernel.  There is no CPU
fallback — if the library or the GPU is missing, construction raises.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# FVO_LIB: an alternative build of the same library (launch-shape experiments, tools/
# build_variant.py); the product path is the in-tree libfvo.so
LIB_PATH = os.environ.get("FVO_LIB") or os.path.join(_HERE, "libfvo.so")

KP_STRIDE = 8
DESC_BYTES = 32

_lib = None


class FvoConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "max_batch", "nfeatures")] + [
        ("scale_factor", ctypes.c_float)] + [(n, ctypes.c_int32) for n in (
            "nlevels", "edge_threshold", "first_level", "wta_k", "score_type", "patch_size", "fast_threshold",
            "min_disparity", "num_disparities", "block_size", "P1", "P2", "disp12_max_diff", "pre_filter_cap",
            "uniqueness_ratio", "sgbm_stripes", "kp_capacity", "stages", "ba_window", "ba_max_landmarks",
            "ba_max_obs", "sgbm_max_batch", "sgbm_mode", "sgbm_lanes", "sgbm_cols", "sgbm_handoff_us")]


class FvoRegion(ctypes.Structure):
    """fvo_region of include/fvo.h."""
    _fields_ = [("dst", ctypes.c_void_p), ("src", ctypes.c_void_p), ("bytes", ctypes.c_int64)]


class FvoSparseStereoParams(ctypes.Structure):
    """fvo_sparse_stereo_params of include/fvo.h."""
    _fields_ = [(n, ctypes.c_float) for n in ("min_disparity", "max_disparity", "row_tol")] + [
        (n, ctypes.c_int32) for n in ("max_hamming", "max_octave_diff", "half_window", "half_slide", "unique")]


FVO_MAX_REGIONS = 32
ABI_VERSION = 7  # FVO_ABI_VERSION of include/fvo.h
STAGE_ORB, STAGE_BF, STAGE_SGBM, STAGE_POSE, STAGE_BA, STAGE_MONO = 1, 2, 4, 8, 16, 32
SGBM_CLASSIC, SGBM_LPATH = 0, 1  # fvo_config.sgbm_mode
SGBM_OK, SGBM_HANDOFF_TIMEOUT = 0, -1  # fvo_sgbm status values
RECTIFY_TILE_W, RECTIFY_TILE_H, RECTIFY_LDS_BYTES = 64, 16, 8192  # FVO_RECTIFY_* of include/fvo.h

# name -> (restype, argtypes); mirrors include/fvo.h
_P = ctypes.c_void_p
_I = ctypes.c_int32
_L = ctypes.c_int64
SIGNATURES = {
    "fvo_abi_version": (ctypes.c_int, []),
    "fvo_config_default": (None, [ctypes.POINTER(FvoConfig), _I, _I]),
    "fvo_config_size": (ctypes.c_int32, []),
    "fvo_config_offset": (ctypes.c_int32, [ctypes.c_char_p]),
    "fvo_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(FvoConfig), ctypes.POINTER(_P)]),
    "fvo_destroy": (None, [_P]),
    "fvo_last_error": (ctypes.c_char_p, [_P]),
    "fvo_kp_capacity": (ctypes.c_int, [_P]),
    "fvo_workspace_bytes": (ctypes.c_int64, [_P]),
    "fvo_orb_detect_compute": (ctypes.c_int, [_P, _P, _I, _L, _I, _P, _P, _P, _I, _P]),
    "fvo_bf_match": (ctypes.c_int, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "fvo_bf_knn_match": (ctypes.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "fvo_bf_ratio_match": (ctypes.c_int, [_P, _P, _P, _P, _P, _I, _I, ctypes.c_double, _I, _P, _P, _P]),
    "fvo_sgbm": (ctypes.c_int, [_P, _P, _P, _I, _L, _I, _P, _P, _P]),
    "fvo_backproject": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _P, ctypes.c_double, _P, _P, _P, _P]),
    "fvo_pnp_ransac": (ctypes.c_int, [_P, _P, _P, _P, _I, _I, _P, _P, ctypes.c_float, ctypes.c_double, _I, _P, _P,
                                      _P, _P, _P, _P]),
    "fvo_keypoint_stereo": (ctypes.c_int, [_P, _P, _P, _P, _I, _I, _P, ctypes.c_double, _P, _P]),
    "fvo_ba_windows": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, ctypes.c_double, _P, _I, _I,
                                      _P, _P, _P]),
    "fvo_ba_landmarks": (ctypes.c_int, [_P, _I, _P, _P, _P]),
    "fvo_ba_count_births": (ctypes.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "fvo_gather_matches": (ctypes.c_int, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "fvo_find_essential": (ctypes.c_int, [_P, _P, _P, _P, _I, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_double, _I, _P, _P, _P, _P]),
    "fvo_recover_pose": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, ctypes.c_double, _P, _P, _P, _P, _P]),
    "fvo_undistort_gray": (ctypes.c_int, [_P, _P, _I, _L, _I, _P, _P, _P, _L, _I, _P]),
    "fvo_rectify_map": (ctypes.c_int, [_P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "fvo_remap_u8": (ctypes.c_int, [_P, _P, _I, _L, _I, _I, _P, _P, _P, _L, _I, _P]),
    "fvo_rectify_gray": (ctypes.c_int, [_P, _P, _I, _L, _I, _I, _P, _P, _I, _P, _P, _P, _L, _I, _P]),
    "fvo_rectify_lds_budget": (ctypes.c_int, [_P, _I]),
    "fvo_map_transform": (ctypes.c_int, [_P, _P, _I, _P, _I, _L, _P, _P, _L, _P, _P, _P]),
    "fvo_chain_poses": (ctypes.c_int, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "fvo_copy_regions": (ctypes.c_int, [_P, _I, _P, _P]),
    "fvo_count_guard": (ctypes.c_int, [_P, _P, _P, _I, _I, _P, _I, _P, _P]),
    "fvo_voxel_workspace_bytes": (ctypes.c_int64, [_L]),
    "fvo_voxel_down_sample": (ctypes.c_int, [_P, _P, _L, ctypes.c_double, _P, _L, _P, _P, _P, _P]),
    "fvo_outlier_workspace_bytes": (ctypes.c_int64, [_L, _I]),
    "fvo_statistical_outliers": (ctypes.c_int, [_P, _P, _L, _I, ctypes.c_double, ctypes.c_double, _I, _P, _L, _P, _P,
                                                _P, _P, _P]),
    "fvo_radius_outliers": (ctypes.c_int, [_P, _P, _L, _I, ctypes.c_double, ctypes.c_double, _P, _L, _P, _P, _P, _P]),
    "fvo_select_points": (ctypes.c_int, [_P, _P, _L, _P, _P, _P, _P, _P]),
    "fvo_normals_workspace_bytes": (ctypes.c_int64, [_L, _I]),
    "fvo_estimate_normals": (ctypes.c_int, [_P, _P, _L, _I, ctypes.c_double, ctypes.c_double, _I, _P, _L, _P, _I, _P,
                                            _P, _P, _P, _P]),
    "fvo_orient_normals": (ctypes.c_int, [_P, _P, _P, _L, _I, ctypes.POINTER(ctypes.c_double), _P]),
    "fvo_icp_workspace_bytes": (ctypes.c_int64, [_L, _L]),
    "fvo_registration_icp": (ctypes.c_int, [_P, _P, _L, _P, _P, _L, ctypes.c_double, ctypes.c_double,
                                            ctypes.POINTER(ctypes.c_double), _I, ctypes.c_double, ctypes.c_double, _I,
                                            _P, _L, _P, _P, _P, _P, _P]),
    "fvo_transform_points": (ctypes.c_int, [_P, _P, _P, _P, _L, ctypes.POINTER(ctypes.c_double), _P]),
    "fvo_speckle_workspace_bytes": (ctypes.c_int64, [_I, _I, _I]),
    "fvo_filter_speckles": (ctypes.c_int, [_P, _P, _I, _I, _I, _L, _I, _I, _I, _I, _P, _L, _P]),
    "fvo_dense_workspace_bytes": (ctypes.c_int64, [_I, _I, _I, _I]),
    "fvo_dense_map_append": (ctypes.c_int, [_P, _P, _I, _I, _I, _L, _I, _P, ctypes.c_double, _I, _I, ctypes.c_float,
                                            ctypes.c_float, _P, _P, _P, _L, _P, _P, _P, _P, _L, _P]),
    "fvo_reproject_to_3d": (ctypes.c_int, [_P, _P, _I, _I, _I, _I, _L, _I, _P, _I, _P, _P, _P]),
    "fvo_sparse_stereo_params_default": (None, [ctypes.POINTER(FvoSparseStereoParams)]),
    "fvo_sparse_stereo_workspace_bytes": (ctypes.c_int64, [_I, _I]),
    "fvo_sparse_stereo": (ctypes.c_int, [_P, _P, _P, _I, _L, _I, _P, _P, _P, _P, _P, _P, _I,
                                         ctypes.POINTER(FvoSparseStereoParams), _P, _I, _P, ctypes.c_double, _P, _L, _P,
                                         _P, _P]),
    "fvo_backproject_stereo": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "fvo_motion_blur": (ctypes.c_int, [_P, _P, _I, _L, _I, _I, ctypes.c_double, _P, _P, _I, _P, _P, _L, _I, _P]),
    "fvo_test_retain_best": (ctypes.c_int, [_P, _P, _I, _I, _P, _P, _P]),
    "fvo_debug_buffer": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "fvo_debug_copy": (ctypes.c_int, [_P, ctypes.c_int, _P, _L]),
    "fvo_kernel_count": (ctypes.c_int, []),
    "fvo_kernel_name": (ctypes.c_char_p, [ctypes.c_int]),
    "fvo_timing_enable": (ctypes.c_int, [_P, ctypes.c_uint64]),
    "fvo_timing_read": (ctypes.c_int, [_P, _P, _P]),
}


def check_config_layout(L) -> None:
    """Refuse a library whose fvo_config layout differs from FvoConfig (size and every
    field offset), so fvo_config_default can never write past the ctypes struct."""
    if L.fvo_config_size() != ctypes.sizeof(FvoConfig):
        raise RuntimeError(f"fvo_config is {L.fvo_config_size()} B in libfvo.so, {ctypes.sizeof(FvoConfig)} B here")
    for name, _ in FvoConfig._fields_:
        if L.fvo_config_offset(name.encode()) != getattr(FvoConfig, name).offset:
            raise RuntimeError(f"fvo_config.{name} offset differs between libfvo.so and the binding")


def kernel_names() -> list[str]:
    L = load()
    return [L.fvo_kernel_name(i).decode() for i in range(L.fvo_kernel_count())]


def load(path: str = LIB_PATH):
    """Load libfvo.so (raises if it is missing: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise RuntimeError(f"libfvo.so not found at {path}: run __graft_entry__.build() "
                               "(python -m forest_slam_amd.build); the HIP path has no CPU fallback")
        L = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.fvo_abi_version() != ABI_VERSION:
            raise RuntimeError("libfvo.so ABI version mismatch")
        check_config_layout(L)
        _lib = L
    return _lib


def _ptr(t: torch.Tensor | None):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libfvo takes device tensors")
    return ctypes.c_void_p(t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _i32(x, dev):
    return torch.as_tensor(x, dtype=torch.int32, device=dev)


class Context:
    """One fvo context (device workspace) for a fixed image size and max batch."""

    def __init__(self, width: int, height: int, max_batch: int = 1, device: int | str | torch.device | None = None,
                 **params):
        if not torch.cuda.is_available():
            raise RuntimeError("forest_slam_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.L = load()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("device must be a cuda (ROCm) device")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        cfg = FvoConfig()
        self.L.fvo_config_default(ctypes.byref(cfg), width, height)
        cfg.max_batch = max_batch
        for k, v in params.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown fvo_config field {k}")
            setattr(cfg, k, v)
        self.cfg = cfg
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            rc = self.L.fvo_create(dev.index, ctypes.byref(cfg), ctypes.byref(h))
        if rc != 0 or not h.value:
            raise RuntimeError("fvo_create failed (see stderr)")
        self.h = h
        self.kp_cap = self.L.fvo_kp_capacity(h)
        self.width, self.height, self.max_batch = width, height, max_batch

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.fvo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError("libfvo: " + self.L.fvo_last_error(self.h).decode())

    @property
    def workspace_bytes(self) -> int:
        return int(self.L.fvo_workspace_bytes(self.h))

    def timing_enable(self, names=None):
        """Bracket launches of the named kernels (all if None, none if []) with HIP events."""
        all_names = kernel_names()
        if names is None:
            mask = (1 << len(all_names)) - 1
        else:
            mask = 0
            for n in names:
                mask |= 1 << all_names.index(n)
        self._check(self.L.fvo_timing_enable(self.h, mask))

    def timing_read(self) -> dict:
        """{kernel: (total_ms, launches)} for the launches recorded since the last read."""
        import numpy as np
        nk = self.L.fvo_kernel_count()
        ms = np.zeros(nk, np.float64)
        cnt = np.zeros(nk, np.int32)
        self._check(self.L.fvo_timing_read(self.h, ms.ctypes.data_as(ctypes.c_void_p),
                                           cnt.ctypes.data_as(ctypes.c_void_p)))
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(kernel_names()) if cnt[i] > 0}

    # ------------------------------------------------------------------ stages
    def orb(self, images: torch.Tensor, out=None):
        """images u8 [B,H,W] (or [H,W]) on device -> (kp f32[B,cap,8], desc u8[B,cap,32], counts i32[B])."""
        if images.dim() == 2:
            images = images[None]
        if images.dtype != torch.uint8:
            raise TypeError("images must be uint8")
        images = images.contiguous()
        B, H, W = images.shape
        if (H, W) != (self.height, self.width):
            raise ValueError(f"context is {self.width}x{self.height}, got {W}x{H}")
        cap = self.kp_cap
        if out is None:
            kp = torch.empty((B, cap, KP_STRIDE), dtype=torch.float32, device=self.device)
            desc = torch.empty((B, cap, DESC_BYTES), dtype=torch.uint8, device=self.device)
            cnt = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            kp, desc, cnt = out
        self._check(self.L.fvo_orb_detect_compute(self.h, _ptr(images), B, H * W, W, _ptr(kp), _ptr(desc),
                                                  _ptr(cnt), cap, _stream(self.device)))
        return kp, desc, cnt

    def bf_match(self, d0, n0, d1, n1, out=None):
        """Cross-checked Hamming matching; d* u8 [B,cap,32], n* i32 [B]."""
        B, cap = d0.shape[0], d0.shape[1]
        if out is None:
            m = torch.empty((B, cap, 3), dtype=torch.int32, device=self.device)
            nm = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            m, nm = out
        self._check(self.L.fvo_bf_match(self.h, _ptr(d0.contiguous()), _ptr(n0), _ptr(d1.contiguous()), _ptr(n1), B,
                                        cap, _ptr(m), _ptr(nm), _stream(self.device)))
        return m, nm

    def bf_knn_match(self, d0, n0, d1, n1, k, out=None):
        """k nearest train descriptors per query row, no cross-check (fvo_bf_knn_match); d* u8
        [B,cap,32], n* i32 [B] -> int32 [B,cap,k,2] rows of (trainIdx, distance) by ascending
        (distance, trainIdx), (-1, -1) past the train set's size; rows >= n0 are not written."""
        B, cap, k = d0.shape[0], d0.shape[1], int(k)
        if out is None:
            out = torch.empty((B, cap, max(k, 0), 2), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or out.shape != (B, cap, k, 2) or not out.is_contiguous():
            raise TypeError(f"bf_knn_match: out must be a contiguous int32 [{B},{cap},{k},2] tensor")
        self._check(self.L.fvo_bf_knn_match(self.h, _ptr(d0.contiguous()), _ptr(n0), _ptr(d1.contiguous()), _ptr(n1),
                                            B, cap, k, _ptr(out), _stream(self.device)))
        return out

    def bf_ratio_match(self, d0, n0, d1, n1, ratio, mutual=True, out=None):
        """Lowe's ratio test on the two nearest neighbours (fvo_bf_ratio_match): rows (queryIdx,
        trainIdx, distance) with float(d1) < ratio * float(d2); mutual=True also requires the
        reverse nearest neighbour (a subset of bf_match's rows).  Buffers as for bf_match."""
        B, cap = d0.shape[0], d0.shape[1]
        if out is None:
            m = torch.empty((B, cap, 3), dtype=torch.int32, device=self.device)
            nm = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            m, nm = out
        self._check(self.L.fvo_bf_ratio_match(self.h, _ptr(d0.contiguous()), _ptr(n0), _ptr(d1.contiguous()), _ptr(n1),
                                              B, cap, float(ratio), int(bool(mutual)), _ptr(m), _ptr(nm),
                                              _stream(self.device)))
        return m, nm

    def sgbm(self, left, right, out=None, status=None):
        """StereoSGBM 3-way + medianBlur(3) of u8 [B,H,W] pairs -> int16 [B,H,W] disparity*16.
        status: optional int32 [B] device tensor, written SGBM_OK / SGBM_HANDOFF_TIMEOUT."""
        if left.dim() == 2:
            left, right = left[None], right[None]
        left, right = left.contiguous(), right.contiguous()
        B, H, W = left.shape
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.int16, device=self.device)
        if status is not None and (status.dtype != torch.int32 or status.numel() < B or not status.is_contiguous()):
            raise TypeError("status must be a contiguous int32 tensor of >= batch entries")
        self._check(self.L.fvo_sgbm(self.h, _ptr(left), _ptr(right), B, H * W, W, _ptr(out), _ptr(status),
                                    _stream(self.device)))
        return out

    def backproject(self, disp, kp0, kp1, matches, nmatch, K, baseline, out=None):
        B, cap = matches.shape[0], matches.shape[1]
        if out is None:
            P3 = torch.empty((B, cap, 3), dtype=torch.float32, device=self.device)
            p2 = torch.empty((B, cap, 2), dtype=torch.float32, device=self.device)
            n = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            P3, p2, n = out
        Kh = (ctypes.c_double * 9)(*[float(v) for v in K.reshape(-1)])
        self._check(self.L.fvo_backproject(self.h, _ptr(disp), _ptr(kp0), _ptr(kp1), _ptr(matches), _ptr(nmatch), B,
                                           cap, Kh, float(baseline), _ptr(P3), _ptr(p2), _ptr(n),
                                           _stream(self.device)))
        return P3, p2, n

    def pnp_ransac(self, P3, p2, n, K, dist, reproj=1.0, confidence=0.99, iterations=1000, out=None):
        B, cap = P3.shape[0], P3.shape[1]
        if out is None:
            rvec = torch.empty((B, 3), dtype=torch.float64, device=self.device)
            tvec = torch.empty((B, 3), dtype=torch.float64, device=self.device)
            T = torch.empty((B, 4, 4), dtype=torch.float64, device=self.device)
            st = torch.empty((B,), dtype=torch.int32, device=self.device)
            inl = torch.empty((B, cap), dtype=torch.uint8, device=self.device)
        else:
            rvec, tvec, T, st, inl = out
        Kh = (ctypes.c_double * 9)(*[float(v) for v in K.reshape(-1)])
        dh = (ctypes.c_double * 5)(*([float(v) for v in list(dist)[:5]] + [0.0] * (5 - min(5, len(dist)))))
        self._check(self.L.fvo_pnp_ransac(self.h, _ptr(P3), _ptr(p2), _ptr(n), B, cap, Kh, dh, float(reproj),
                                          float(confidence), int(iterations), _ptr(rvec), _ptr(tvec), _ptr(T),
                                          _ptr(st), _ptr(inl), _stream(self.device)))
        return rvec, tvec, T, st, inl

    def keypoint_stereo(self, disp, kp, nkp, K, baseline, out=None):
        """Stereo point (X, Y, Z, d) of every keypoint (fvo_keypoint_stereo); Z = 0 invalid."""
        B, cap = kp.shape[0], kp.shape[1]
        if out is None:
            out = torch.empty((B, cap, 4), dtype=torch.float32, device=self.device)
        Kh = (ctypes.c_double * 9)(*[float(v) for v in K.reshape(-1)])
        self._check(self.L.fvo_keypoint_stereo(self.h, _ptr(disp), _ptr(kp), _ptr(nkp), B, cap, Kh, float(baseline),
                                               _ptr(out), _stream(self.device)))
        return out

    def ba_windows(self, kp, nkp, matches, nmatch, stereo, T_rel, first_end, n_windows, first_valid, K, baseline,
                   iterations=10, scale_factor=1.2, out=None):
        """Windowed local BA over frame arrays [F,...] (fvo_ba_windows).  Observation
        weights 1 / scale_factor^(2 octave) (scale_factor as a Python float, the value
        ORB_create() receives).  Returns (T_out f64[n_windows,4,4] refined last-pair
        transforms, stats f64[n_windows,6])."""
        F, cap = kp.shape[0], kp.shape[1]
        if out is None:
            Tout = torch.empty((n_windows, 4, 4), dtype=torch.float64, device=self.device)
            stats = torch.empty((n_windows, 6), dtype=torch.float64, device=self.device)
        else:
            Tout, stats = out
        Kh = (ctypes.c_double * 9)(*[float(v) for v in K.reshape(-1)])
        nl = int(self.cfg.nlevels)
        isig = (ctypes.c_double * nl)(*[1.0 / (float(scale_factor) ** (2 * o)) for o in range(nl)])
        self._check(self.L.fvo_ba_windows(self.h, _ptr(kp), _ptr(nkp), _ptr(matches), _ptr(nmatch), _ptr(stereo),
                                          _ptr(T_rel), F, cap, int(first_end), int(n_windows), int(first_valid), Kh,
                                          float(baseline), isig, nl, int(iterations), _ptr(Tout), _ptr(stats),
                                          _stream(self.device)))
        return Tout, stats

    def ba_count_births(self, matches, nmatch, stereo, first_end, n_windows, first_valid):
        """fvo_ba_count_births: the landmark-birth counting of the next ba_windows call with the
        same frame arrays and window range, issued ahead on the current stream (it needs neither
        T_rel nor the keypoints)."""
        F, cap = matches.shape[0], matches.shape[1]
        self._check(self.L.fvo_ba_count_births(self.h, _ptr(matches), _ptr(nmatch), _ptr(stereo), F, cap,
                                               int(first_end), int(n_windows), int(first_valid),
                                               _stream(self.device)))

    def ba_landmarks(self, window: int, out=None):
        """Refined landmarks of one window of the last ba_windows call (device tensors,
        no host sync): (xyz f64[ba_max_landmarks,3], count i32[1])."""
        if out is None:
            xyz = torch.empty((int(self.cfg.ba_max_landmarks), 3), dtype=torch.float64, device=self.device)
            cnt = torch.empty((1,), dtype=torch.int32, device=self.device)
        else:
            xyz, cnt = out
        self._check(self.L.fvo_ba_landmarks(self.h, int(window), _ptr(xyz), _ptr(cnt), _stream(self.device)))
        return xyz, cnt

    def undistort_gray(self, bgr, K, dist, out=None):
        """cv2.undistort + cvtColor(BGR2GRAY): bgr u8 [B,H,W,3] (or [H,W,3]) -> gray u8 [B,H,W]."""
        if bgr.dim() == 3:
            bgr = bgr[None]
        if bgr.dtype != torch.uint8 or bgr.shape[-1] != 3:
            raise TypeError("bgr must be uint8 [B,H,W,3]")
        bgr = bgr.contiguous()
        B, H, W, _ = bgr.shape
        if (H, W) != (self.height, self.width):
            raise ValueError(f"context is {self.width}x{self.height}, got {W}x{H}")
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        Kh = (ctypes.c_double * 9)(*[float(v) for v in np.asarray(K, np.float64).reshape(-1)])
        d = [float(v) for v in np.asarray(dist, np.float64).reshape(-1)[:5]]
        dh = (ctypes.c_double * 5)(*(d + [0.0] * (5 - len(d))))
        self._check(self.L.fvo_undistort_gray(self.h, _ptr(bgr), B, H * W * 3, W * 3, Kh, dh, _ptr(out), H * W, W,
                                              _stream(self.device)))
        return out

    def _u8_images(self, t, name, channels=None):
        """(tensor, B, channels, image stride, row pitch) of u8 images of the context's size:
        [B,H,W,C], [H,W,C], [B,H,W] or [H,W] (C = 1 or 3), pixels contiguous within a row; rows and
        images may be spaced (a view of a wider buffer).  A 3-d tensor is [B,H,W] when channels
        is 1 and [H,W,C] when it is 3; with channels None it is told by its shape ([B,H,W] unless
        only [H,W,C] fits)."""
        H, W = self.height, self.width
        if t.dtype != torch.uint8:
            raise TypeError(f"{name}: expected a uint8 tensor")
        if channels not in (None, 1, 3):
            raise ValueError(f"{name}: channels must be 1 or 3")
        if t.dim() == 3 and channels is not None:
            mono = channels == 1 and t.shape[2] != 1
        else:
            mono = t.dim() == 3 and tuple(t.shape[1:]) == (H, W) and not (tuple(t.shape[:2]) == (H, W) and
                                                                          t.shape[2] in (1, 3))
        if t.dim() == 2 or mono:
            t = t[..., None]
        if t.dim() == 3:
            t = t[None]
        if t.dim() != 4 or tuple(t.shape[1:3]) != (H, W) or t.shape[3] not in (1, 3):
            raise ValueError(f"{name}: context is {W}x{H}, expected [B,{H},{W},1|3], got {tuple(t.shape)}")
        B, C = t.shape[0], t.shape[3]
        if channels is not None and C != channels:
            raise ValueError(f"{name}: expected {channels} channel(s), got {C}")
        if (C > 1 and t.stride(3) != 1) or (W > 1 and t.stride(2) != C):
            raise ValueError(f"{name}: the pixels of a row must be contiguous")
        pitch = t.stride(1) if H > 1 else W * C
        return t, B, C, (t.stride(0) if B > 1 else pitch * H), pitch

    @staticmethod
    def _lens_args(K, dist, R, newK):
        d = [float(v) for v in np.asarray(dist, np.float64).reshape(-1)]
        if len(d) not in (4, 5, 8):
            raise ValueError("dist must have 4, 5 or 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]])")
        m9 = lambda M: None if M is None else (ctypes.c_double * 9)(*[float(v) for v in
                                                                      np.asarray(M, np.float64).reshape(9)])
        return m9(K), (ctypes.c_double * len(d))(*d), len(d), m9(R), m9(newK)

    def rectify_map(self, K, dist, R=None, newK=None, out=None):
        """cv2.initUndistortRectifyMap(K, dist, R, newK, (W, H), CV_16SC2) for the context's image
        size (fvo_rectify_map) -> (map1 i16 [H,W,2], map2 u16 [H,W]) on the device.  R None = I,
        newK None = K; dist has 4, 5 or 8 coefficients."""
        H, W = self.height, self.width
        if out is None:
            out = (torch.empty((H, W, 2), dtype=torch.int16, device=self.device),
                   torch.empty((H, W), dtype=torch.uint16, device=self.device))
        m1, m2 = out
        if m1.dtype != torch.int16 or tuple(m1.shape) != (H, W, 2) or not m1.is_contiguous() or \
                m2.dtype != torch.uint16 or tuple(m2.shape) != (H, W) or not m2.is_contiguous():
            raise TypeError(f"rectify_map: out must be contiguous (int16 [{H},{W},2], uint16 [{H},{W}])")
        Kh, dh, nd, Rh, Nh = self._lens_args(K, dist, R, newK)
        self._check(self.L.fvo_rectify_map(self.h, Kh, dh, nd, Rh, Nh, _ptr(m1), _ptr(m2), _stream(self.device)))
        return m1, m2

    def remap(self, src, map1, map2, out=None, channels=None):
        """cv2.remap(src, map1, map2, INTER_LINEAR) with BORDER_CONSTANT 0 (fvo_remap_u8) on u8
        images [B,H,W,C] / [H,W,C] / [B,H,W] / [H,W], C = 1 or 3 -> u8 [B,H,W,C].  channels (1 or 3)
        says which layout a 3-d src has where its shape alone cannot (B == H == W)."""
        H, W = self.height, self.width
        s, B, C, sstride, spitch = self._u8_images(src, "remap", channels)
        if map1.dtype != torch.int16 or tuple(map1.shape) != (H, W, 2) or not map1.is_contiguous() or \
                map2.dtype != torch.uint16 or tuple(map2.shape) != (H, W) or not map2.is_contiguous():
            raise TypeError(f"remap: the map must be contiguous (int16 [{H},{W},2], uint16 [{H},{W}])")
        if out is None:
            out = torch.empty((B, H, W, C), dtype=torch.uint8, device=self.device)
        o, Bo, Co, dstride, dpitch = self._u8_images(out, "remap out", C if out.dim() == 3 else None)
        if (Bo, Co) != (B, C):
            raise ValueError("remap: out must have the batch and channels of src")
        self._check(self.L.fvo_remap_u8(self.h, _ptr(s), B, sstride, spitch, C, _ptr(map1), _ptr(map2), _ptr(o),
                                        dstride, dpitch, _stream(self.device)))
        return out

    def rectify_gray(self, src, K, dist, R=None, newK=None, out=None, channels=None):
        """The rectifying ingest (fvo_rectify_gray): initUndistortRectifyMap + remap + BGR2GRAY in
        one kernel, no map stored.  src u8 bgr8 [B,H,W,3] / [H,W,3] or mono8 [B,H,W] / [H,W]
        -> gray u8 [B,H,W].  channels (1 or 3) says which layout a 3-d src has where its shape
        alone cannot (B == H == W)."""
        H, W = self.height, self.width
        s, B, C, sstride, spitch = self._u8_images(src, "rectify_gray", channels)
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        o, Bo, Co, dstride, dpitch = self._u8_images(out, "rectify_gray out", 1 if out.dim() == 3 else None)
        if (Bo, Co) != (B, 1):
            raise ValueError("rectify_gray: out must be [B,H,W] with the batch of src")
        Kh, dh, nd, Rh, Nh = self._lens_args(K, dist, R, newK)
        self._check(self.L.fvo_rectify_gray(self.h, _ptr(s), B, sstride, spitch, C, Kh, dh, nd, Rh, Nh, _ptr(o),
                                            dstride, dpitch, _stream(self.device)))
        return out

    def rectify_lds_budget(self, nbytes: int):
        """Measurement / test hook (fvo_rectify_lds_budget): LDS bytes a block of remap /
        rectify_gray may stage; 0 = every block gathers directly.  The output does not depend on it."""
        self._check(self.L.fvo_rectify_lds_budget(self.h, int(nbytes)))

    def motion_blur(self, img, ksize, centers=None, n_centers=None, angle=0.0, out=None, mask=None):
        """apply_random_motion_blur (stereo_slam.py:142-178) on gray u8 [B,H,W] images.
        centers: i32 [B,cap] flat pixel indices on the device (or None: no blurred pixel),
        n_centers: i32 [B] device counts.  Returns (out u8 [B,H,W], mask u8 [B,H,W])."""
        if img.dim() == 2:
            img = img[None]
        if img.dtype != torch.uint8:
            raise TypeError("img must be uint8 [B,H,W]")
        img = img.contiguous()
        B, H, W = img.shape
        if (H, W) != (self.height, self.width):
            raise ValueError(f"context is {self.width}x{self.height}, got {W}x{H}")
        if out is None:
            out = torch.empty_like(img)
        if mask is None:
            mask = torch.empty_like(img)
        if centers is None:
            cptr, nptr, cap = None, None, 0
        else:
            if centers.dtype != torch.int32 or n_centers is None or n_centers.dtype != torch.int32:
                raise TypeError("centers / n_centers must be int32 device tensors")
            centers, n_centers = centers.contiguous(), n_centers.contiguous()
            if centers.dim() != 2 or centers.shape[0] != B or n_centers.numel() != B:
                raise ValueError("centers must be [B, cap] and n_centers [B]")
            cptr, nptr, cap = _ptr(centers), _ptr(n_centers), int(centers.shape[1])
        self._check(self.L.fvo_motion_blur(self.h, _ptr(img), B, H * W, W, int(ksize), float(angle), cptr, nptr, cap,
                                           _ptr(mask), _ptr(out), H * W, W, _stream(self.device)))
        return out, mask

    def map_transform(self, points, n_points, T, map_count, map_xyz64=None, map_xyz32=None):
        """Append T[b] @ [p; 1] of every set b to the map (stereo_slam.py:308-318; fvo_map_transform).
        points f32 [B,cap,>=3], n_points i32 [B], T f64 [B,4,4] (all device); map_count i32 [1]
        (device, advanced by the call); map_xyz64 f64 [M,3] and/or map_xyz32 f32 [M,3]."""
        if points.dtype != torch.float32 or points.dim() != 3 or points.shape[2] < 3:
            raise TypeError("points must be float32 [B, cap, >=3]")
        if map_xyz64 is None and map_xyz32 is None:
            raise ValueError("need map_xyz64 and/or map_xyz32")
        points, T = points.contiguous(), T.to(torch.float64).contiguous()
        B, cap, st = points.shape
        if T.shape != (B, 4, 4) or n_points.dtype != torch.int32 or n_points.numel() != B:
            raise ValueError("T must be [B,4,4] and n_points int32 [B]")
        caps = [m.shape[0] for m in (map_xyz64, map_xyz32) if m is not None]
        self._check(self.L.fvo_map_transform(self.h, _ptr(points), st, _ptr(n_points), B, cap, _ptr(T),
                                             _ptr(map_count), min(caps),
                                             _ptr(map_xyz64) if map_xyz64 is not None else None,
                                             _ptr(map_xyz32) if map_xyz32 is not None else None,
                                             _stream(self.device)))
        return map_count

    def chain_poses(self, T, status, cum_state, n_points=None, out=None):
        """Advance the pose chains of S sequences over one batch of n frames each on the device
        (stereo_slam.py:292-306; fvo_chain_poses).  T f64 [S,n,4,4], status i32 [S,n], n_points
        i32 [S,n] or None, cum_state f64 [S,4,4] (advanced in place).  Returns (cum f64
        [S,n,4,4] = each frame's cumulative pose, n_points_out i32 [S,n] = n_points of the
        posed frames (status >= 0), 0 elsewhere; None without n_points)."""
        if T.dim() != 4 or T.shape[2:] != (4, 4) or T.dtype != torch.float64 or not T.is_contiguous():
            raise TypeError("T must be contiguous float64 [S, n, 4, 4]")
        S, n = T.shape[0], T.shape[1]
        if status.dtype != torch.int32 or status.shape != (S, n) or not status.is_contiguous():
            raise TypeError("status must be contiguous int32 [S, n]")
        if cum_state.dtype != torch.float64 or cum_state.shape != (S, 4, 4) or not cum_state.is_contiguous():
            raise TypeError("cum_state must be contiguous float64 [S, 4, 4]")
        if n_points is not None and (n_points.dtype != torch.int32 or n_points.shape != (S, n)
                                     or not n_points.is_contiguous()):
            raise TypeError("n_points must be contiguous int32 [S, n]")
        if out is None:
            cum = torch.empty_like(T)
            npo = torch.empty_like(n_points) if n_points is not None else None
        else:
            cum, npo = out
        self._check(self.L.fvo_chain_poses(self.h, _ptr(T), _ptr(status), _ptr(n_points), S, n, _ptr(cum_state),
                                           _ptr(cum), _ptr(npo), _stream(self.device)))
        return cum, npo

    def copy_regions(self, pairs):
        """Device-to-device copies ``dst.copy_(src)`` for every (dst, src) in pairs, in list
        order, batched into fvo_copy_regions launches of up to FVO_MAX_REGIONS (same-dtype
        contiguous pairs; any other pair is copied by torch after the batch before it has been
        launched, so a torch copy never overtakes an earlier batched one).  No destination may
        overlap any source or other destination of one batch (the library refuses it)."""
        batch = []

        def flush():
            for k in range(0, len(batch), FVO_MAX_REGIONS):
                part = batch[k:k + FVO_MAX_REGIONS]
                arr = (FvoRegion * len(part))(*[FvoRegion(dp, sp, nb) for dp, sp, nb in part])
                self._check(self.L.fvo_copy_regions(self.h, len(part), ctypes.cast(arr, _P), _stream(self.device)))
            batch.clear()

        for d, src in pairs:
            nb = d.numel() * d.element_size()
            if d.dtype != src.dtype or d.shape != src.shape or not (d.is_contiguous() and src.is_contiguous()):
                flush()
                d.copy_(src)
                continue
            if nb:
                batch.append((d.data_ptr(), src.data_ptr(), nb))
        flush()

    def count_guard(self, counts, n, sets=1, q_counts=None, status=None, code=0, clamped_out=None):
        """fvo_count_guard: status[i] = code where any counts[s*n + i] / q_counts[s*n + i]
        (s < sets) is negative; clamped_out[i] = max(counts[i], 0)."""
        for t in (counts, q_counts, status, clamped_out):
            if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
                raise TypeError("count_guard takes contiguous int32 tensors")
        if counts.numel() < sets * n or (q_counts is not None and q_counts.numel() < sets * n):
            raise ValueError("count_guard: counts shorter than sets * n")
        if (status is not None and status.numel() < n) or (clamped_out is not None and clamped_out.numel() < n):
            raise ValueError("count_guard: outputs shorter than n")
        self._check(self.L.fvo_count_guard(self.h, _ptr(counts), _ptr(q_counts), n, sets, _ptr(status), code,
                                           _ptr(clamped_out), _stream(self.device)))

    def voxel_down_sample(self, points, voxel_size, workspace=None):
        """Open3D voxel_down_sample (mono_slam.py:155): points f64 [N,3] (device) ->
        (out f64 [N,3] (first n rows valid, voxel-index order), n i32[1], status i32[1])."""
        if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3:
            raise TypeError("points must be float64 [N, 3]")
        points = points.contiguous()
        n = points.shape[0]
        out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=self.device)
        cnt = torch.zeros((1,), dtype=torch.int32, device=self.device)
        status = torch.zeros((1,), dtype=torch.int32, device=self.device)
        wb = int(self.L.fvo_voxel_workspace_bytes(n)) if n > 0 else 0
        if n > 0 and wb < 0:
            raise RuntimeError("fvo_voxel_workspace_bytes failed")
        if workspace is None or workspace.numel() < wb:
            workspace = torch.empty((max(wb, 1),), dtype=torch.uint8, device=self.device)
        self._check(self.L.fvo_voxel_down_sample(self.h, _ptr(points), n, float(voxel_size), _ptr(workspace), wb,
                                                 _ptr(out), _ptr(cnt), _ptr(status), _stream(self.device)))
        return out, cnt, status

    def outlier_workspace_bytes(self, n_points: int, nb_neighbors: int = 1) -> int:
        """fvo_outlier_workspace_bytes: scratch bytes of statistical_outliers / radius_outliers."""
        wb = int(self.L.fvo_outlier_workspace_bytes(int(n_points), int(nb_neighbors)))
        if wb < 0:
            raise ValueError(f"outlier removal: unsupported size n_points={n_points} nb_neighbors={nb_neighbors}")
        return wb

    def _outlier_args(self, points, workspace, nb_neighbors, name):
        if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
            raise TypeError(f"{name}: points must be a contiguous float64 [N, 3] tensor")
        n = points.shape[0]
        wb = self.outlier_workspace_bytes(n, nb_neighbors)
        if workspace is None:
            workspace = torch.empty((max(wb, 8),), dtype=torch.uint8, device=self.device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < wb:
            raise ValueError(f"{name}: workspace must be a contiguous uint8 tensor of >= {wb} bytes")
        return n, workspace

    def statistical_outliers(self, points, nb_neighbors=20, std_ratio=2.0, cell=1.0, max_rings=2, workspace=None,
                             avg_distance=True, status=True):
        """Open3D remove_statistical_outlier's mask (fvo_statistical_outliers; the rule:
        tests/outlier_ref.py): points f64 [N,3] (device, not modified) -> (keep u8 [N], avg_distance
        f64 [N] or None, stats f64 [6] = mean, std, threshold, valid, kept, queries finished by the
        exact pass, status i32 [1] or None: 1 = a cell index outside the 21-bit range or a non-finite
        coordinate).  cell and max_rings change the time only.  workspace: uint8 device tensor of >=
        outlier_workspace_bytes(N, nb_neighbors) bytes, allocated here only when none is passed;
        avg_distance / status False: that output is not requested (NULL)."""
        n, workspace = self._outlier_args(points, workspace, nb_neighbors, "statistical_outliers")
        keep = torch.empty((n,), dtype=torch.uint8, device=self.device)
        avg = torch.empty((n,), dtype=torch.float64, device=self.device) if avg_distance else None
        stats = torch.empty((6,), dtype=torch.float64, device=self.device)
        st = torch.empty((1,), dtype=torch.int32, device=self.device) if status else None
        self._check(self.L.fvo_statistical_outliers(self.h, _ptr(points), n, int(nb_neighbors), float(std_ratio),
                                                    float(cell), int(max_rings), _ptr(workspace), workspace.numel(),
                                                    _ptr(keep), _ptr(avg), _ptr(stats), _ptr(st),
                                                    _stream(self.device)))
        return keep, avg, stats, st

    def radius_outliers(self, points, nb_points, radius, cell=None, workspace=None, n_neighbors=True, status=True):
        """Open3D remove_radius_outlier's mask (fvo_radius_outliers): points f64 [N,3] (device) ->
        (keep u8 [N], n_neighbors i32 [N] or None: the points with d2 < radius^2, the query included,
        status i32 [1] or None).  cell None = radius; radius / cell <= 8."""
        n, workspace = self._outlier_args(points, workspace, 1, "radius_outliers")
        keep = torch.empty((n,), dtype=torch.uint8, device=self.device)
        cnt = torch.empty((n,), dtype=torch.int32, device=self.device) if n_neighbors else None
        st = torch.empty((1,), dtype=torch.int32, device=self.device) if status else None
        self._check(self.L.fvo_radius_outliers(self.h, _ptr(points), n, int(nb_points), float(radius),
                                               float(radius if cell is None else cell), _ptr(workspace),
                                               workspace.numel(), _ptr(keep), _ptr(cnt), _ptr(st),
                                               _stream(self.device)))
        return keep, cnt, st

    def select_points(self, points, keep, out64=None, out32=None, n_out=None):
        """The points with keep != 0 in input order (fvo_select_points): points f64 [N,3], keep u8 [N]
        (device) -> (out64 f64 [N,3] or None, out32 f32 [N,3] or None, n_out i32 [1]); the first n_out
        rows are written, nothing past them.  With neither output given both are allocated."""
        if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
            raise TypeError("select_points: points must be a contiguous float64 [N, 3] tensor")
        n = points.shape[0]
        if keep.dtype != torch.uint8 or keep.numel() != n or not keep.is_contiguous():
            raise TypeError("select_points: keep must be a contiguous uint8 [N] tensor")
        if out64 is None and out32 is None:
            out64 = torch.empty((max(n, 1), 3), dtype=torch.float64, device=self.device)  # n = 0: not NULL
            out32 = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        for o, dt in ((out64, torch.float64), (out32, torch.float32)):
            if o is not None and (o.dtype != dt or o.numel() < 3 * n or not o.is_contiguous()):
                raise TypeError(f"select_points: outputs must be contiguous {dt} tensors of >= N rows")
        if n_out is None:
            n_out = torch.empty((1,), dtype=torch.int32, device=self.device)
        self._check(self.L.fvo_select_points(self.h, _ptr(points), n, _ptr(keep), _ptr(out64), _ptr(out32),
                                             _ptr(n_out), _stream(self.device)))
        return out64, out32, n_out

    def normals_workspace_bytes(self, n_points: int, max_nn: int = 30) -> int:
        """fvo_normals_workspace_bytes: scratch bytes of estimate_normals."""
        wb = int(self.L.fvo_normals_workspace_bytes(int(n_points), int(max_nn)))
        if wb < 0:
            raise ValueError(f"estimate_normals: unsupported size n_points={n_points} max_nn={max_nn}")
        return wb

    def estimate_normals(self, points, max_nn=30, radius=math.inf, cell=None, max_rings=2, prior=None,
                         covariances=False, n_neighbors=False, workspace=None):
        """Open3D estimate_normals / estimate_covariances with KDTreeSearchParamKNN(max_nn) (radius inf)
        or KDTreeSearchParamHybrid(radius, max_nn) (fvo_estimate_normals; the rule: tests/normals_ref.py):
        points f64 [N,3] (device, not modified) -> (normals f64 [N,3], covariances f64 [N,3,3] or None,
        n_neighbors i32 [N] or None, stats i32 [2] = queries finished by the exact pass, points with
        fewer than 3 neighbours, status i32 [1]: 1 = a cell index outside the 21-bit range or a
        non-finite coordinate).  prior: f64 [N,3] normals whose side the result keeps; it is written in
        place and returned as the normals.  cell (None: radius when finite, else 1.0) and max_rings
        change the time only.  workspace: uint8 device tensor of >= normals_workspace_bytes(N, max_nn)
        bytes, allocated here only when none is passed."""
        if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
            raise TypeError("estimate_normals: points must be a contiguous float64 [N, 3] tensor")
        n = points.shape[0]
        wb = self.normals_workspace_bytes(n, max_nn)
        if workspace is None:
            workspace = torch.empty((max(wb, 8),), dtype=torch.uint8, device=self.device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < wb:
            raise ValueError(f"estimate_normals: workspace must be a contiguous uint8 tensor of >= {wb} bytes")
        if prior is None:
            normals = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        elif prior.dtype != torch.float64 or prior.dim() != 2 or prior.shape[1] != 3 or prior.shape[0] < n or \
                not prior.is_contiguous():
            raise TypeError("estimate_normals: prior must be a contiguous float64 tensor of >= N rows of 3")
        else:
            normals = prior
        radius = float(radius)
        if cell is None:
            cell = radius if math.isfinite(radius) else 1.0
        cov = torch.empty((n, 3, 3), dtype=torch.float64, device=self.device) if covariances else None
        cnt = torch.empty((n,), dtype=torch.int32, device=self.device) if n_neighbors else None
        stats = torch.empty((2,), dtype=torch.int32, device=self.device)
        st = torch.empty((1,), dtype=torch.int32, device=self.device)
        self._check(self.L.fvo_estimate_normals(self.h, _ptr(points), n, int(max_nn), radius, float(cell),
                                                int(max_rings), _ptr(workspace), workspace.numel(), _ptr(normals),
                                                int(prior is not None), _ptr(cov), _ptr(cnt), _ptr(stats), _ptr(st),
                                                _stream(self.device)))
        return normals[:n], cov, cnt, stats, st

    def orient_normals(self, points, normals, camera_location=None, direction=None):
        """Open3D orient_normals_towards_camera_location(camera_location) or
        orient_normals_to_align_with_direction(direction) (fvo_orient_normals): exactly one of the two,
        three host numbers; points, normals f64 [N,3] (device); normals are changed in place and returned."""
        if (camera_location is None) == (direction is None):
            raise ValueError("orient_normals: give exactly one of camera_location and direction")
        for t in (points, normals):
            if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
                raise TypeError("orient_normals: points and normals must be contiguous float64 [N, 3] tensors")
        if normals.shape[0] != points.shape[0]:
            raise ValueError("orient_normals: points and normals differ in length")
        ref = [float(v) for v in (camera_location if direction is None else direction)]
        if len(ref) != 3:
            raise ValueError("orient_normals: camera_location / direction must have three components")
        self._check(self.L.fvo_orient_normals(self.h, _ptr(points), _ptr(normals), points.shape[0],
                                              0 if direction is None else 1, (ctypes.c_double * 3)(*ref),
                                              _stream(self.device)))
        return normals

    def icp_workspace_bytes(self, n_source: int, n_target: int) -> int:
        """fvo_icp_workspace_bytes: scratch bytes of registration_icp."""
        wb = int(self.L.fvo_icp_workspace_bytes(int(n_source), int(n_target)))
        if wb < 0:
            raise ValueError(f"registration_icp: unsupported size n_source={n_source} n_target={n_target}")
        return wb

    def registration_icp(self, source, target, max_correspondence_distance, init=None, estimation=0,
                         target_normals=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, cell=None,
                         workspace=None, sums=False, correspondences=True):
        """Open3D registration_icp (max_iteration 0: evaluate_registration) of source onto target
        (fvo_registration_icp; the rule: tests/icp_ref.py): f64 [N,3] device tensors, not modified;
        estimation 0 point-to-point, 1 point-to-plane (target_normals f64 [Nt,3]); init: 4x4 host numbers
        (None: the identity) -> (result f64 [20] = T row-major, fitness, inlier_rmse, correspondences,
        iterations; sums f64 [45] or None: the last pass's 28 sums, m and the T that entered it;
        correspondences i32 [N] or None: the target index or -1; status i32 [1]: bit 1 = a target cell
        index outside the 21-bit range or a non-finite coordinate, bit 2 = a degenerate system).
        Everything stays on the device: the call does not synchronise.  cell None = the distance.
        workspace: uint8 device tensor of >= icp_workspace_bytes(N, Nt) bytes, allocated here only when
        none is passed."""
        for t, name in ((source, "source"), (target, "target"), (target_normals, "target_normals")):
            if t is not None and (t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous()):
                raise TypeError(f"registration_icp: {name} must be a contiguous float64 [N, 3] tensor")
        ns, nt = source.shape[0], target.shape[0]
        if target_normals is not None and target_normals.shape[0] < nt:
            raise ValueError("registration_icp: target_normals has fewer rows than target")
        wb = self.icp_workspace_bytes(ns, nt)
        if workspace is None:
            workspace = torch.empty((max(wb, 8),), dtype=torch.uint8, device=self.device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < wb:
            raise ValueError(f"registration_icp: workspace must be a contiguous uint8 tensor of >= {wb} bytes")
        T = [float(v) for v in (np.eye(4) if init is None else np.asarray(init, np.float64)).reshape(-1)]
        if len(T) != 16:
            raise ValueError("registration_icp: init must be a 4x4 matrix")
        r = float(max_correspondence_distance)
        result = torch.empty((20,), dtype=torch.float64, device=self.device)
        sm = torch.empty((45,), dtype=torch.float64, device=self.device) if sums else None
        corr = torch.empty((ns,), dtype=torch.int32, device=self.device) if correspondences else None
        st = torch.empty((1,), dtype=torch.int32, device=self.device)
        self._check(self.L.fvo_registration_icp(self.h, _ptr(source), ns, _ptr(target), _ptr(target_normals), nt, r,
                                                float(r if cell is None else cell), (ctypes.c_double * 16)(*T),
                                                int(estimation), float(relative_fitness), float(relative_rmse),
                                                int(max_iteration), _ptr(workspace), workspace.numel(), _ptr(result),
                                                _ptr(sm), _ptr(corr), _ptr(st), _stream(self.device)))
        return result, sm, corr, st

    def transform_points(self, points, T, points32=None, normals=None):
        """Open3D PointCloud.transform (fvo_transform_points): points f64 [N,3] (device) become
        ((r00*x + r01*y) + r02*z) + t0 ... in place; points32 f32 [N,3] receives their casts, normals
        f64 [N,3] are rotated in place.  T: 4x4 host numbers.  Returns points."""
        for t, dt in ((points, torch.float64), (points32, torch.float32), (normals, torch.float64)):
            if t is not None and (t.dtype != dt or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous() or
                                  t.shape[0] < points.shape[0]):
                raise TypeError("transform_points: points, points32 and normals must be contiguous [N, 3] tensors "
                                "(float64, float32, float64)")
        M = [float(v) for v in np.asarray(T, np.float64).reshape(-1)]
        if len(M) != 16:
            raise ValueError("transform_points: T must be a 4x4 matrix")
        self._check(self.L.fvo_transform_points(self.h, _ptr(points), _ptr(points32), _ptr(normals), points.shape[0],
                                                (ctypes.c_double * 16)(*M), _stream(self.device)))
        return points

    def speckle_workspace_bytes(self, batch: int, height: int, width: int) -> int:
        """fvo_speckle_workspace_bytes: scratch bytes of filter_speckles for [batch, height, width]."""
        wb = int(self.L.fvo_speckle_workspace_bytes(int(batch), int(height), int(width)))
        if wb < 0:
            raise ValueError(f"filter_speckles: unsupported size batch={batch} {width}x{height}")
        return wb

    def filter_speckles(self, disp, new_val, max_speckle_size, max_diff, workspace=None):
        """cv2.filterSpeckles on int16 [B,H,W] (or [H,W]) device disparity maps, in place
        (fvo_filter_speckles); returns disp.  disp may be a column range of a wider buffer (row
        pitch > W); rows must be element-contiguous.  workspace: uint8 device tensor of at least
        speckle_workspace_bytes(B, H, W) bytes, allocated here only when none is passed."""
        if disp.dtype != torch.int16 or disp.dim() not in (2, 3):
            raise TypeError("disp must be int16 [B,H,W] or [H,W]")
        d3 = disp if disp.dim() == 3 else disp[None]
        B, H, W = d3.shape
        if B == 0 or H == 0 or W == 0:
            return disp
        if W > 1 and d3.stride(2) != 1:
            raise ValueError("filter_speckles: the last dimension must be contiguous")
        pitch = d3.stride(1) if H > 1 else W
        istride = d3.stride(0) if B > 1 else pitch * H
        wb = self.speckle_workspace_bytes(B, H, W)
        if workspace is None:
            workspace = torch.empty((max(wb, 1),), dtype=torch.uint8, device=self.device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < wb:
            raise ValueError(f"filter_speckles: workspace must be a contiguous uint8 tensor of >= {wb} bytes")
        self._check(self.L.fvo_filter_speckles(self.h, _ptr(d3), B, H, W, istride, pitch, int(new_val),
                                               int(max_speckle_size), int(max_diff), _ptr(workspace),
                                               workspace.numel(), _stream(self.device)))
        return disp

    @staticmethod
    def _image_view(t, name):
        """(3-d view, B, H, W, image stride, row pitch) of a [B,H,W] / [H,W] tensor whose rows are
        element-contiguous (e.g. a column range of a wider buffer)."""
        if t.dim() not in (2, 3):
            raise TypeError(f"{name}: expected [B,H,W] or [H,W]")
        t3 = t if t.dim() == 3 else t[None]
        B, H, W = t3.shape
        if W > 1 and t3.stride(2) != 1:
            raise ValueError(f"{name}: the last dimension must be contiguous")
        pitch = t3.stride(1) if H > 1 else W
        istride = t3.stride(0) if B > 1 else pitch * H
        return t3, B, H, W, istride, pitch

    def dense_workspace_bytes(self, batch: int, height: int, width: int, step: int = 1) -> int:
        """fvo_dense_workspace_bytes: scratch bytes of dense_map_append for [batch, height, width]."""
        wb = int(self.L.fvo_dense_workspace_bytes(int(batch), int(height), int(width), int(step)))
        if wb < 0:
            raise ValueError(f"dense_map_append: unsupported size batch={batch} {width}x{height} step={step}")
        return wb

    def dense_map_append(self, disp, K, baseline, T, map_count, map_xyz64=None, map_xyz32=None, step=1,
                         min_disp16=1, z_min=0.1, z_max=1000.0, frame_keep=None, n_added=None, workspace=None,
                         map_cap=None):
        """Append the disparity maps of a batch to the map as a world-frame point cloud
        (fvo_dense_map_append): every step-th pixel of every step-th row of int16 [B,H,W] (or
        [H,W]) device maps, back-projected as backproject() does (float32), kept iff d16 >=
        min_disp16 and z_min < Z < z_max, transformed by T f64 [B,4,4] (device) as map_transform()
        does and appended from map_count i32 [1] in frame, then row-major, order.  frame_keep i32
        [B] (device): 0 = the frame contributes nothing.  disp may be a column range of a wider
        buffer and is not modified.  workspace: uint8 device tensor of >= dense_workspace_bytes(B,
        H, W, step) bytes, allocated here (as n_added i32 [B] is) only when none is passed.
        Returns n_added: the kept samples per frame."""
        if disp.dtype != torch.int16:
            raise TypeError("disp must be int16 [B,H,W] or [H,W]")
        if map_xyz64 is None and map_xyz32 is None:
            raise ValueError("need map_xyz64 and/or map_xyz32")
        d3, B, H, W, istride, pitch = self._image_view(disp, "dense_map_append")
        if n_added is None:
            n_added = torch.zeros((B,), dtype=torch.int32, device=self.device)
        elif n_added.dtype != torch.int32 or n_added.numel() < B or not n_added.is_contiguous():
            raise TypeError("n_added must be a contiguous int32 tensor of >= batch entries")
        if B == 0 or H == 0 or W == 0:
            return n_added
        T = T.to(torch.float64).contiguous()
        if T.shape != (B, 4, 4):
            raise ValueError("T must be [B,4,4]")
        if frame_keep is not None and (frame_keep.dtype != torch.int32 or frame_keep.numel() != B
                                       or not frame_keep.is_contiguous()):
            raise TypeError("frame_keep must be a contiguous int32 [B] tensor")
        wb = self.dense_workspace_bytes(B, H, W, step)
        if workspace is None:
            workspace = torch.empty((wb,), dtype=torch.uint8, device=self.device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < wb:
            raise ValueError(f"dense_map_append: workspace must be a contiguous uint8 tensor of >= {wb} bytes")
        if map_cap is None:
            map_cap = min(m.shape[0] for m in (map_xyz64, map_xyz32) if m is not None)
        Kh = (ctypes.c_double * 9)(*[float(v) for v in np.asarray(K, np.float64).reshape(-1)])
        self._check(self.L.fvo_dense_map_append(self.h, _ptr(d3), B, H, W, istride, pitch, Kh, float(baseline),
                                                int(step), int(min_disp16), float(z_min), float(z_max),
                                                _ptr(frame_keep), _ptr(T), _ptr(map_count), int(map_cap),
                                                _ptr(map_xyz64), _ptr(map_xyz32), _ptr(n_added), _ptr(workspace),
                                                workspace.numel(), _stream(self.device)))
        return n_added

    def reproject_to_3d(self, disp, Q, handle_missing=False, out=None):
        """cv2.reprojectImageTo3D on int16 or float32 [B,H,W] (or [H,W]) device images
        (fvo_reproject_to_3d) -> f32 [B,H,W,3]; the RAW pixel value is the disparity (int16 maps
        are not divided by 16, as in cv2).  Q: 4x4."""
        if disp.dtype not in (torch.int16, torch.float32):
            raise TypeError("disp must be int16 or float32")
        d3, B, H, W, istride, pitch = self._image_view(disp, "reproject_to_3d")
        if out is None:
            out = torch.empty((B, H, W, 3), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or out.shape != (B, H, W, 3) or not out.is_contiguous():
            raise TypeError(f"reproject_to_3d: out must be a contiguous float32 [{B},{H},{W},3] tensor")
        if B == 0 or H == 0 or W == 0:
            return out
        Qh = (ctypes.c_double * 16)(*[float(v) for v in np.asarray(Q, np.float64).reshape(16)])
        key = torch.empty((B,), dtype=torch.int32, device=self.device) if handle_missing else None
        self._check(self.L.fvo_reproject_to_3d(self.h, _ptr(d3), int(disp.dtype == torch.float32), B, H, W, istride,
                                               pitch, Qh, int(bool(handle_missing)), _ptr(key), _ptr(out),
                                               _stream(self.device)))
        return out

    def sparse_stereo_params(self, **kw) -> FvoSparseStereoParams:
        """fvo_sparse_stereo_params_default with the given fields replaced."""
        p = FvoSparseStereoParams()
        self.L.fvo_sparse_stereo_params_default(ctypes.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown fvo_sparse_stereo_params field {k}")
            setattr(p, k, v)
        return p

    def sparse_stereo_workspace_bytes(self, batch: int, cap: int) -> int:
        """fvo_sparse_stereo_workspace_bytes: scratch bytes of sparse_stereo for [batch, cap]."""
        wb = int(self.L.fvo_sparse_stereo_workspace_bytes(int(batch), int(cap)))
        if wb < 0:
            raise ValueError(f"sparse_stereo: unsupported size batch={batch} cap={cap}")
        return wb

    def level_scales(self) -> np.ndarray:
        """The context's ORB level scales as sparse_stereo takes them: float32(scale_factor ** o)."""
        return np.array([float(self.cfg.scale_factor) ** o for o in range(int(self.cfg.nlevels))], np.float32)

    def sparse_stereo(self, left, right, kpL, nL, descL, kpR, nR, descR, K, baseline, params=None, level_scale=None,
                      workspace=None, out=None, info=None):
        """Per-keypoint stereo records from left-right ORB matches (fvo_sparse_stereo; the rule:
        tests/sparse_stereo_ref.py).  left/right u8 [B,H,W] (or [H,W]) of the context's size, rows
        and images may be spaced; kp* f32 [B,cap,8], n* i32 [B], desc* u8 [B,cap,32].  params: a
        sparse_stereo_params() struct or a dict of its fields; level_scale: float32 per octave
        (default level_scales()).  workspace: uint8 device tensor of >= sparse_stereo_workspace_bytes(B,
        cap) bytes, allocated here only when none is passed.  info: int32 [B,cap,4] to receive
        (right index, hamming, k*, status), or None.  Returns stereo f32 [B,cap,4] = (X, Y, Z, d),
        zeros where no point was found; rows >= nL are not written."""
        l, B, _, istride, pitch = self._u8_images(left, "sparse_stereo left", 1)
        r, Br, _, rstride, rpitch = self._u8_images(right, "sparse_stereo right", 1)
        if (Br, rstride, rpitch) != (B, istride, pitch):
            raise ValueError("sparse_stereo: left and right must have the same batch, stride and pitch")
        cap = kpL.shape[1]
        for t, shape, dt in ((kpL, (B, cap, KP_STRIDE), torch.float32), (kpR, (B, cap, KP_STRIDE), torch.float32),
                             (descL, (B, cap, DESC_BYTES), torch.uint8), (descR, (B, cap, DESC_BYTES), torch.uint8)):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise TypeError(f"sparse_stereo: expected a contiguous {dt} {list(shape)} tensor")
        if out is None:
            out = torch.empty((B, cap, 4), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, cap, 4) or not out.is_contiguous():
            raise TypeError(f"sparse_stereo: out must be a contiguous float32 [{B},{cap},4] tensor")
        if info is not None and (info.dtype != torch.int32 or tuple(info.shape) != (B, cap, 4) or
                                 not info.is_contiguous()):
            raise TypeError(f"sparse_stereo: info must be a contiguous int32 [{B},{cap},4] tensor")
        if B == 0:
            return out
        if params is None or isinstance(params, dict):
            params = self.sparse_stereo_params(**(params or {}))
        ls = np.ascontiguousarray(self.level_scales() if level_scale is None else level_scale, np.float32)
        wb = self.sparse_stereo_workspace_bytes(B, cap)
        if workspace is None:
            workspace = torch.empty((wb,), dtype=torch.uint8, device=self.device)
        elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < wb:
            raise ValueError(f"sparse_stereo: workspace must be a contiguous uint8 tensor of >= {wb} bytes")
        Kh = (ctypes.c_double * 9)(*[float(v) for v in np.asarray(K, np.float64).reshape(-1)])
        self._check(self.L.fvo_sparse_stereo(self.h, _ptr(l), _ptr(r), B, istride, pitch, _ptr(kpL), _ptr(nL),
                                             _ptr(descL), _ptr(kpR), _ptr(nR), _ptr(descR), cap, ctypes.byref(params),
                                             ls.ctypes.data_as(ctypes.c_void_p), len(ls), Kh, float(baseline),
                                             _ptr(workspace), workspace.numel(), _ptr(out), _ptr(info),
                                             _stream(self.device)))
        return out

    def backproject_stereo(self, stereo, kp1, matches, nmatch, out=None):
        """backproject() with the depth taken from the stereo record of the match's query keypoint
        (fvo_backproject_stereo): the records with Z != 0, compacted in match order."""
        B, cap = matches.shape[0], matches.shape[1]
        if out is None:
            P3 = torch.empty((B, cap, 3), dtype=torch.float32, device=self.device)
            p2 = torch.empty((B, cap, 2), dtype=torch.float32, device=self.device)
            n = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            P3, p2, n = out
        self._check(self.L.fvo_backproject_stereo(self.h, _ptr(stereo), None, _ptr(kp1), _ptr(matches), _ptr(nmatch),
                                                  B, cap, _ptr(P3), _ptr(p2), _ptr(n), _stream(self.device)))
        return P3, p2, n

    def gather_matches(self, kp0, kp1, matches, nmatch, out=None):
        """mkpts0/mkpts1 of a BF match list (fvo_gather_matches): (p0 f32[B,cap,2], p1, n i32[B])."""
        B, cap = matches.shape[0], matches.shape[1]
        if out is None:
            p0 = torch.empty((B, cap, 2), dtype=torch.float32, device=self.device)
            p1 = torch.empty((B, cap, 2), dtype=torch.float32, device=self.device)
            n = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            p0, p1, n = out
        self._check(self.L.fvo_gather_matches(self.h, _ptr(kp0), _ptr(kp1), _ptr(matches), _ptr(nmatch), B, cap,
                                              _ptr(p0), _ptr(p1), _ptr(n), _stream(self.device)))
        return p0, p1, n

    def find_essential(self, p0, p1, n, focal, pp, prob=0.999, threshold=1.0, max_iters=1000, out=None):
        """findEssentialMat(RANSAC) on [B] point sets: (E f64[B,3,3], mask u8[B,cap], status i32[B])."""
        B, cap = p0.shape[0], p0.shape[1]
        if out is None:
            E = torch.empty((B, 3, 3), dtype=torch.float64, device=self.device)
            mask = torch.empty((B, cap), dtype=torch.uint8, device=self.device)
            st = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            E, mask, st = out
        self._check(self.L.fvo_find_essential(self.h, _ptr(p0.contiguous()), _ptr(p1.contiguous()), _ptr(n), B, cap,
                                              float(focal), float(pp[0]), float(pp[1]), float(prob), float(threshold),
                                              int(max_iters), _ptr(E), _ptr(mask), _ptr(st), _stream(self.device)))
        return E, mask, st

    def recover_pose(self, E, p0, p1, n, focal, pp, e_status=None, distance_thresh=50.0, out=None):
        """recoverPose on [B] frames: (R f64[B,3,3], t f64[B,3], T f64[B,4,4], n_good i32[B])."""
        B, cap = p0.shape[0], p0.shape[1]
        if out is None:
            R = torch.empty((B, 3, 3), dtype=torch.float64, device=self.device)
            t = torch.empty((B, 3), dtype=torch.float64, device=self.device)
            T = torch.empty((B, 4, 4), dtype=torch.float64, device=self.device)
            g = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            R, t, T, g = out
        self._check(self.L.fvo_recover_pose(self.h, _ptr(E.contiguous()), _ptr(e_status), _ptr(p0.contiguous()),
                                            _ptr(p1.contiguous()), _ptr(n), B, cap, float(focal), float(pp[0]),
                                            float(pp[1]), float(distance_thresh), _ptr(R), _ptr(t), _ptr(T), _ptr(g),
                                            _stream(self.device)))
        return R, t, T, g

    def debug_buffer(self, which: int) -> torch.Tensor:
        """Host copy (u8 CPU tensor) of an internal workspace buffer (fvo_debug_buffer for the size,
        fvo_debug_copy for the bytes)."""
        p = ctypes.c_void_p()
        nb = ctypes.c_int64()
        self._check(self.L.fvo_debug_buffer(self.h, which, ctypes.byref(p), ctypes.byref(nb)))
        host = torch.empty((nb.value,), dtype=torch.uint8)
        self._check(self.L.fvo_debug_copy(self.h, which, ctypes.c_void_p(host.data_ptr()), nb.value))
        return host

    def geometry(self):
        """Pyramid level (w, h, offset) list, mirroring OpenCV ORB's layer sizes."""
        import numpy as np
        sf = float(np.float32(self.cfg.scale_factor))
        out, off = [], 0
        for l in range(self.cfg.nlevels):
            s = np.float32(sf ** l)
            inv = np.float32(1.0) / s
            w = int(np.rint(np.float32(self.width) * inv))
            h = int(np.rint(np.float32(self.height) * inv))
            out.append((w, h, off))
            off += w * h
        return out, off

    def test_retain_best(self, keys: torch.Tensor, keep: int):
        keys = keys.to(self.device, torch.float32).contiguous()
        n = keys.numel()
        idx = torch.empty((max(n, 1),), dtype=torch.int32, device=self.device)
        nout = torch.empty((1,), dtype=torch.int32, device=self.device)
        self._check(self.L.fvo_test_retain_best(self.h, _ptr(keys), n, keep, _ptr(idx), _ptr(nout),
                                                _stream(self.device)))
        k = int(nout.item())
        return idx[:k].clone()
