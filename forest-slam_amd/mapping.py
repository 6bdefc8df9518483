"""Map accumulation on the GPU over libfvo's fvo_map_transform and
fvo_voxel_down_sample.

* ``PointMap.add_frames`` — stereo_slam.py:308-318: every frame's points3D transformed by its
  cumulative pose, ``(cum @ hstack(points3D, 1).T)[:3].T``, appended to ``all_points_3D``;
  ``cloud32()`` is the float32 x/y/z payload ``create_point_cloud(np.concatenate(...))`` packs
  (PointCloud2, point_step 12).
* ``PointMap.add_cloud`` — mono_slam.py:144-164 / gt_mapping.py:62-66: one point cloud
  transformed by the pose, ``voxel_down_sample(voxel_size=0.5)``, appended to the map.
* ``PointMap.add_disparity`` — dense stereo mapping over fvo_dense_map_append (no reference
  counterpart): whole disparity maps back-projected and appended, optionally voxel-filtered.
* ``PointMap.remove_statistical_outlier`` / ``remove_radius_outlier`` — Open3D's map clean-up
  (fvo_statistical_outliers, fvo_radius_outliers, fvo_select_points) on the device, in place.
* ``PointMap.estimate_normals`` / ``estimate_covariances`` / ``orient_normals_*`` — Open3D's normal
  estimation (fvo_estimate_normals, fvo_orient_normals): one fp64 normal per map point, kept aligned
  with the points by the clean-up and dropped by any append.
* ``PointMap.transform`` / ``registration_icp`` — Open3D's ``transform(T)`` in place (fvo_transform_points;
  the normals are rotated and kept) and ICP of this map onto another (fvo_registration_icp through
  ``registration.registration_icp``).

The map lives in HBM (fp64 + the float32 record), sized once; the append offset is a device
counter, so batches append without host synchronisation."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


class PointMap:
    def __init__(self, capacity: int, device="cuda:0", ctx: _lib.Context | None = None):
        self.dev = torch.device(device)
        self.ctx = ctx or _lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_BF, kp_capacity=64, device=self.dev)
        self.capacity = int(capacity)
        self.xyz64 = torch.zeros((self.capacity, 3), dtype=torch.float64, device=self.dev)
        self.xyz32 = torch.zeros((self.capacity, 3), dtype=torch.float32, device=self.dev)
        self.count = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self._tmp64 = None
        self._ws = None
        self._dense_ws = None
        self._ol_ws = None
        self.normals64 = None  # [capacity, 3] f64, allocated by the first estimate_normals
        self._has_normals = False
        self._nm_ws = None

    def __len__(self) -> int:
        n = int(self.count.item())
        if n > self.capacity:
            raise RuntimeError(f"PointMap overflow: {n} points for capacity {self.capacity}")
        return n

    def add_frames(self, points: torch.Tensor, n_points: torch.Tensor, cum: np.ndarray | torch.Tensor,
                   check: bool = False):
        """points f32 [B,cap,3] (device), n_points i32 [B] (device; 0 for frames the reference
        skips), cum f64 [B,4,4] (each frame's cumulative pose, stereo_slam.py:306).

        The device counter keeps counting points past ``capacity`` (they are not written), so
        an overflow is detected exactly by the next ``len()``; ``check=True`` synchronises
        and raises right here instead, before another batch is appended."""
        T = torch.as_tensor(np.asarray(cum, np.float64) if not isinstance(cum, torch.Tensor) else cum,
                            dtype=torch.float64).to(self.dev)
        self._has_normals = False
        self.ctx.map_transform(points, n_points, T, self.count, self.xyz64, self.xyz32)
        if check:
            len(self)

    def overflowed(self) -> bool:
        """True once more points were appended than the map holds (host sync)."""
        return int(self.count.item()) > self.capacity

    def add_cloud(self, points, cum, voxel_size: float = 0.5):
        """mono_slam.py:144-164: points f32 [n,3] (PointCloud2 x/y/z), pose cum f64 [4,4]."""
        P = torch.as_tensor(np.asarray(points, np.float32) if not isinstance(points, torch.Tensor) else points,
                            dtype=torch.float32).to(self.dev).reshape(1, -1, 3).contiguous()
        n = P.shape[1]
        if n == 0:
            return
        self._has_normals = False
        if self._tmp64 is None or self._tmp64.shape[0] < n:
            self._tmp64 = torch.empty((n, 3), dtype=torch.float64, device=self.dev)
            self._ws = torch.empty((int(self.ctx.L.fvo_voxel_workspace_bytes(n)),), dtype=torch.uint8,
                                   device=self.dev)
        c0 = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        T = torch.as_tensor(np.asarray(cum, np.float64), dtype=torch.float64, device=self.dev).reshape(1, 4, 4)
        self.ctx.map_transform(P, torch.tensor([n], dtype=torch.int32, device=self.dev), T, c0, self._tmp64[:n], None)
        out, nv, st = self.ctx.voxel_down_sample(self._tmp64[:n], voxel_size, workspace=self._ws)
        if int(st.item()) != 0:
            raise RuntimeError("voxel_down_sample: voxel index outside the 21-bit key range")
        k, base = int(nv.item()), len(self)
        if base + k > self.capacity:
            raise RuntimeError(f"PointMap overflow: {base + k} points for capacity {self.capacity}")
        self.xyz64[base:base + k] = out[:k]
        self.xyz32[base:base + k] = out[:k].to(torch.float32)  # pc2.create_cloud_xyz32
        self.count += k

    def add_disparity(self, disp: torch.Tensor, K, baseline: float, cum, step: int = 1, min_disp16: int = 1,
                      z_min: float = 0.1, z_max: float = 1000.0, keep: torch.Tensor | None = None,
                      voxel_size: float | None = None, check: bool = False) -> torch.Tensor:
        """Dense stereo mapping (fvo_dense_map_append): every step-th pixel of every step-th row
        of the int16 [B,H,W] device disparity maps (StereoSGBM's x16 values), back-projected with
        the reference's float32 arithmetic (stereo_slam.py:117-121, :265-289), kept iff d16 >=
        min_disp16 and z_min < Z < z_max, placed by cum f64 [B,4,4] (each frame's cumulative pose)
        and appended in frame, then row-major, order.  keep: i32 [B] device tensor, 0 = the frame
        contributes nothing (frames the reference skips).

        voxel_size=None appends straight into the map, with add_frames' overflow contract
        (``check=True`` raises right here).  Otherwise the points go into a scratch cloud, through
        voxel_down_sample(voxel_size), and the result is appended as add_cloud does (host sync).
        Returns n_added i32 [B] (device): the kept samples of each frame, before any voxel filter."""
        T = torch.as_tensor(np.asarray(cum, np.float64) if not isinstance(cum, torch.Tensor) else cum,
                            dtype=torch.float64).to(self.dev).reshape(-1, 4, 4)
        d3 = disp if disp.dim() == 3 else disp[None]
        B, H, W = d3.shape
        self._has_normals = False
        wb = self.ctx.dense_workspace_bytes(B, H, W, step)
        if self._dense_ws is None or self._dense_ws.numel() < wb:
            self._dense_ws = torch.empty((wb,), dtype=torch.uint8, device=self.dev)
        kw = dict(step=step, min_disp16=min_disp16, z_min=z_min, z_max=z_max, frame_keep=keep,
                  workspace=self._dense_ws)
        if voxel_size is None:
            n_added = self.ctx.dense_map_append(d3, K, baseline, T, self.count, self.xyz64, self.xyz32, **kw)
            if check:
                len(self)
            return n_added
        n = B * ((H - 1) // step + 1) * ((W - 1) // step + 1)  # every sample kept
        if n == 0:
            return torch.zeros((B,), dtype=torch.int32, device=self.dev)
        if self._tmp64 is None or self._tmp64.shape[0] < n:
            self._tmp64 = torch.empty((n, 3), dtype=torch.float64, device=self.dev)
            self._ws = torch.empty((int(self.ctx.L.fvo_voxel_workspace_bytes(n)),), dtype=torch.uint8,
                                   device=self.dev)
        c0 = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        n_added = self.ctx.dense_map_append(d3, K, baseline, T, c0, self._tmp64[:n], None, **kw)
        m = int(c0.item())
        if m == 0:
            return n_added
        out, nv, st = self.ctx.voxel_down_sample(self._tmp64[:m], voxel_size, workspace=self._ws)
        if int(st.item()) != 0:
            raise RuntimeError("voxel_down_sample: voxel index outside the 21-bit key range")
        k, base = int(nv.item()), len(self)
        if base + k > self.capacity:
            raise RuntimeError(f"PointMap overflow: {base + k} points for capacity {self.capacity}")
        self.xyz64[base:base + k] = out[:k]
        self.xyz32[base:base + k] = out[:k].to(torch.float32)
        self.count += k
        return n_added

    def _apply_mask(self, n: int, keep: torch.Tensor) -> torch.Tensor:
        """Compact the first n points by the u8 mask, in place through a scratch copy, keeping the
        order, and the normals with them; returns the kept indices (int64, device)."""
        src = self.xyz64[:n].clone()
        self.ctx.select_points(src, keep, self.xyz64, self.xyz32, self.count)
        if self._has_normals:
            self.ctx.select_points(self.normals64[:n].clone(), keep, out64=self.normals64)
        return torch.nonzero(keep).reshape(-1)

    def _outlier_ws(self, n: int, nb_neighbors: int) -> torch.Tensor:
        wb = self.ctx.outlier_workspace_bytes(n, nb_neighbors)
        if self._ol_ws is None or self._ol_ws.numel() < wb:
            self._ol_ws = torch.empty((max(wb, 8),), dtype=torch.uint8, device=self.dev)
        return self._ol_ws

    def remove_statistical_outlier(self, nb_neighbors: int = 20, std_ratio: float = 2.0, cell: float = 1.0,
                                   max_rings: int = 2) -> torch.Tensor:
        """Open3D ``remove_statistical_outlier(nb_neighbors, std_ratio)`` on the map, in place: the
        points whose mean distance to their nb_neighbors nearest (themselves included) is > 0 and
        below mean + std_ratio * std stay, in order.  cell (metres) and max_rings tune the search
        only.  Returns the kept indices (Open3D's ``ind``) as an int64 device tensor (host sync)."""
        n = len(self)
        if n == 0:
            return torch.zeros((0,), dtype=torch.int64, device=self.dev)
        keep, _, _, st = self.ctx.statistical_outliers(self.xyz64[:n], nb_neighbors, std_ratio, cell, max_rings,
                                                       workspace=self._outlier_ws(n, nb_neighbors),
                                                       avg_distance=False)
        if int(st.item()) != 0:
            raise RuntimeError("remove_statistical_outlier: cell index outside the 21-bit key range or a "
                               "non-finite coordinate")
        return self._apply_mask(n, keep)

    def remove_radius_outlier(self, nb_points: int, radius: float, cell: float | None = None) -> torch.Tensor:
        """Open3D ``remove_radius_outlier(nb_points, radius)`` on the map, in place: the points with
        more than nb_points points (themselves included) closer than radius stay, in order.
        cell None = radius.  Returns the kept indices as an int64 device tensor (host sync)."""
        n = len(self)
        if n == 0:
            return torch.zeros((0,), dtype=torch.int64, device=self.dev)
        keep, _, st = self.ctx.radius_outliers(self.xyz64[:n], nb_points, radius, cell,
                                               workspace=self._outlier_ws(n, 1), n_neighbors=False)
        if int(st.item()) != 0:
            raise RuntimeError("remove_radius_outlier: cell index outside the 21-bit key range or a "
                               "non-finite coordinate")
        return self._apply_mask(n, keep)

    def _search(self, name, max_nn, radius):
        if max_nn is None:
            raise NotImplementedError(f"{name}: a pure radius search has no bound on the neighbour count; give "
                                      "max_nn (KDTreeSearchParamKNN or KDTreeSearchParamHybrid)")
        n = len(self)
        wb = self.ctx.normals_workspace_bytes(n, max_nn)
        if self._nm_ws is None or self._nm_ws.numel() < wb:
            self._nm_ws = torch.empty((max(wb, 8),), dtype=torch.uint8, device=self.dev)
        return n, float("inf") if radius is None else float(radius)

    def _checked(self, name, st):
        if int(st.item()) != 0:
            raise RuntimeError(f"{name}: cell index outside the 21-bit key range or a non-finite coordinate")

    def estimate_normals(self, max_nn: int | None = 30, radius: float | None = None, cell: float | None = None,
                         max_rings: int = 2) -> None:
        """Open3D ``estimate_normals(KDTreeSearchParamKNN(max_nn))`` (radius None) or
        ``KDTreeSearchParamHybrid(radius, max_nn)`` on the map: one unit normal per point in
        ``normals64`` (the rule: tests/normals_ref.py).  A map that has normals keeps their side.
        cell (metres; None: radius, else 1.0) and max_rings tune the search only (host sync)."""
        n, radius = self._search("estimate_normals", max_nn, radius)
        if self.normals64 is None:
            self.normals64 = torch.zeros((self.capacity, 3), dtype=torch.float64, device=self.dev)
        if n:
            out = self.ctx.estimate_normals(self.xyz64[:n], max_nn, radius, cell, max_rings, workspace=self._nm_ws,
                                            prior=self.normals64 if self._has_normals else None)
            if not self._has_normals:
                self.normals64[:n] = out[0]
            self._checked("estimate_normals", out[4])
        self._has_normals = True

    def estimate_covariances(self, max_nn: int | None = 30, radius: float | None = None, cell: float | None = None,
                             max_rings: int = 2) -> torch.Tensor:
        """Open3D ``estimate_covariances`` with the same searches: f64 [n, 3, 3] (device; the identity
        where a point has fewer than 3 neighbours).  The map's normals are not touched."""
        n, radius = self._search("estimate_covariances", max_nn, radius)
        if n == 0:
            return torch.zeros((0, 3, 3), dtype=torch.float64, device=self.dev)
        out = self.ctx.estimate_normals(self.xyz64[:n], max_nn, radius, cell, max_rings, workspace=self._nm_ws,
                                        covariances=True)
        self._checked("estimate_covariances", out[4])
        return out[1]

    def _orient(self, start, stop, **ref):
        if not self._has_normals:
            raise RuntimeError("the map has no normals: call estimate_normals first")
        n = len(self)
        start, stop, _ = slice(start, stop).indices(n)
        if stop > start:
            self.ctx.orient_normals(self.xyz64[start:stop], self.normals64[start:stop], **ref)

    def orient_normals_towards_camera_location(self, camera=(0.0, 0.0, 0.0), start: int = 0, stop: int | None = None):
        """Open3D ``orient_normals_towards_camera_location(camera)`` on the points [start, stop) (all
        by default): a caller orients each batch of frames towards its own camera centre."""
        self._orient(start, stop, camera_location=camera)

    def orient_normals_to_align_with_direction(self, direction=(0.0, 0.0, 1.0)):
        """Open3D ``orient_normals_to_align_with_direction(direction)`` on every point."""
        self._orient(0, None, direction=direction)

    def transform(self, T) -> "PointMap":
        """Open3D ``transform(T)`` on the map, in place (fvo_transform_points): every point becomes T p in
        fp64 (the expression of tests/icp_ref.py), the float32 record is its cast, the normals are
        rotated and kept.  T: 4x4 host numbers, bottom row (0, 0, 0, 1).  Host sync (the length)."""
        n = len(self)
        self.ctx.transform_points(self.xyz64[:n], T, self.xyz32[:n], self.normals64[:n] if self._has_normals else None)
        return self

    def registration_icp(self, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None,
                         **kw):
        """Open3D ``registration_icp(self, target, ...)``: this map as the source; see
        ``registration.registration_icp``.  Point-to-plane needs ``target.has_normals()``."""
        from . import registration
        return registration.registration_icp(self, target, max_correspondence_distance, init, estimation_method,
                                             criteria, **kw)

    def has_normals(self) -> bool:
        """False until estimate_normals, and again after any append."""
        return self._has_normals

    def normals(self) -> np.ndarray:
        """f64 [n, 3] on the host."""
        if not self._has_normals:
            raise RuntimeError("the map has no normals: call estimate_normals first")
        return self.normals64[: len(self)].cpu().numpy()

    def cloud32_normals(self) -> np.ndarray:
        """f32 [n, 6]: x, y, z, normal_x, normal_y, normal_z (the PointCloud2 record of point_step 24)."""
        n = len(self)
        if not self._has_normals:
            raise RuntimeError("the map has no normals: call estimate_normals first")
        return torch.cat([self.xyz32[:n], self.normals64[:n].to(torch.float32)], dim=1).cpu().numpy()

    def cloud32(self) -> np.ndarray:
        return self.xyz32[: len(self)].cpu().numpy()

    def cloud64(self) -> np.ndarray:
        return self.xyz64[: len(self)].cpu().numpy()
