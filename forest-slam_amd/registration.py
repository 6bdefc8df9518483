"""Open3D-shaped ICP registration over libfvo's fvo_registration_icp, as cv2_compat is cv2-shaped:

    from forest_slam_amd import registration as reg
    res = reg.registration_icp(source, target, 0.3, np.eye(4), reg.TransformationEstimationPointToPlane(),
                               reg.ICPConvergenceCriteria(max_iteration=30))
    res.transformation, res.fitness, res.inlier_rmse, res.correspondence_set, res.iterations

``source`` / ``target`` are ``mapping.PointMap``s or fp64 ``[n, 3]`` device tensors (``target_normals=`` for
point-to-plane on a tensor target).  The rule is tests/icp_ref.py; DESIGN 4.9 lists where it departs
from Open3D (the transform is always applied to the original source, the Gibbs-vector rotation, Horn's
quaternion, the tie rule).  What Open3D offers here and libfvo does not raises ``NotImplementedError``:
``with_scaling=True``, robust kernels, coloured and generalised ICP.  The call never synchronises: a
``RegistrationResult`` keeps its tensors on the device until a field is read."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


class ICPConvergenceCriteria:
    def __init__(self, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, max_iteration: int = 30):
        self.relative_fitness = float(relative_fitness)
        self.relative_rmse = float(relative_rmse)
        self.max_iteration = int(max_iteration)

    def __repr__(self):
        return (f"ICPConvergenceCriteria(relative_fitness={self.relative_fitness}, relative_rmse={self.relative_rmse}, "
                f"max_iteration={self.max_iteration})")


class TransformationEstimationPointToPoint:
    estimation = 0

    def __init__(self, with_scaling: bool = False):
        if with_scaling:
            raise NotImplementedError("TransformationEstimationPointToPoint(with_scaling=True) is not supported")
        self.with_scaling = False


class TransformationEstimationPointToPlane:
    estimation = 1

    def __init__(self, kernel=None):
        if kernel is not None:
            raise NotImplementedError("robust kernels are not supported: TransformationEstimationPointToPlane() only")
        self.kernel = None


def _unsupported(name):
    def ctor(*args, **kwargs):
        raise NotImplementedError(f"{name} is not supported: point-to-point and point-to-plane ICP only")
    ctor.__name__ = name
    return ctor


TransformationEstimationForColoredICP = _unsupported("TransformationEstimationForColoredICP")
TransformationEstimationForGeneralizedICP = _unsupported("TransformationEstimationForGeneralizedICP")
registration_colored_icp = _unsupported("registration_colored_icp")
registration_generalized_icp = _unsupported("registration_generalized_icp")
for _k in ("L1Loss", "L2Loss", "HuberLoss", "CauchyLoss", "GMLoss", "TukeyLoss"):
    globals()[_k] = _unsupported(_k)


class RegistrationResult:
    """fvo_registration_icp's outputs, on the device until read (each property synchronises).
    ``status``: bit 1 = a target cell index outside the 21-bit range or a non-finite coordinate (a
    property raises), bit 2 = a degenerate system met (an identity update was applied)."""

    def __init__(self, result: torch.Tensor, correspondences: torch.Tensor | None, status: torch.Tensor,
                 sums: torch.Tensor | None = None):
        self.result = result  # f64 [20]: T, fitness, inlier_rmse, correspondences, iterations
        self.correspondences = correspondences  # i32 [n_source]: the target index or -1
        self.status_word = status
        self.sums = sums
        self._host = None

    def _read(self):
        if self._host is None:
            st = int(self.status_word.item())
            if st & 1:
                raise RuntimeError("registration_icp: cell index outside the 21-bit key range or a non-finite coordinate")
            self._host = (self.result.cpu().numpy(), st)
        return self._host

    @property
    def transformation(self) -> np.ndarray:
        return self._read()[0][:16].reshape(4, 4).copy()

    @property
    def fitness(self) -> float:
        return float(self._read()[0][16])

    @property
    def inlier_rmse(self) -> float:
        return float(self._read()[0][17])

    @property
    def iterations(self) -> int:
        return int(self._read()[0][19])

    @property
    def status(self) -> int:
        return self._read()[1]

    @property
    def correspondence_set(self) -> np.ndarray:
        """int32 [m, 2]: (source index, target index) of every kept correspondence, in source order."""
        self._read()
        if self.correspondences is None:
            raise RuntimeError("the correspondences were not requested")
        c = self.correspondences.cpu().numpy()
        k = np.flatnonzero(c >= 0)
        return np.stack([k.astype(np.int32), c[k]], axis=1)

    def __repr__(self):
        return (f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, and "
                f"correspondence_set size of {int(self._read()[0][18])}")


def _cloud(x, name):
    """-> (points f64 [n, 3] device tensor, normals or None, a context or None)."""
    from .mapping import PointMap
    if isinstance(x, PointMap):
        n = len(x)
        return x.xyz64[:n], (x.normals64[:n] if x.has_normals() else None), x.ctx
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"registration_icp: {name} must be a PointMap or a float64 [n, 3] device tensor")
    return x, None, None


_default_ctx = {}


def _context(device, *ctxs):
    for c in ctxs:
        if c is not None:
            return c
    key = str(device)
    if key not in _default_ctx:
        _default_ctx[key] = _lib.Context(64, 64, max_batch=1, stages=_lib.STAGE_BF, kp_capacity=64, device=device)
    return _default_ctx[key]


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None,
                     target_normals=None, cell=None, workspace=None, sums=False, ctx=None) -> RegistrationResult:
    """Open3D ``registration_icp(source, target, max_correspondence_distance, init, estimation_method,
    criteria)``.  estimation_method None: point-to-point; criteria None: ICPConvergenceCriteria()."""
    est = TransformationEstimationPointToPoint() if estimation_method is None else estimation_method
    if not isinstance(est, (TransformationEstimationPointToPoint, TransformationEstimationPointToPlane)):
        raise NotImplementedError("registration_icp: estimation_method must be TransformationEstimationPointToPoint() "
                                  "or TransformationEstimationPointToPlane()")
    crit = ICPConvergenceCriteria() if criteria is None else criteria
    S, _, sctx = _cloud(source, "source")
    T, tn, tctx = _cloud(target, "target")
    if target_normals is not None:
        tn = target_normals
    if est.estimation == 1 and tn is None:
        raise RuntimeError("the map has no normals: call estimate_normals first" if tctx is not None else
                           "registration_icp: point-to-plane needs target_normals")
    c = _context(S.device, ctx, sctx, tctx)
    out = c.registration_icp(S, T, max_correspondence_distance, init, est.estimation,
                             tn if est.estimation == 1 else None, crit.relative_fitness, crit.relative_rmse,
                             crit.max_iteration, cell, workspace, sums)
    return RegistrationResult(out[0], out[2], out[3], out[1])


def evaluate_registration(source, target, max_correspondence_distance, transformation=None, **kw) -> RegistrationResult:
    """Open3D ``evaluate_registration``: fitness, inlier_rmse and the correspondences at ``transformation``."""
    return registration_icp(source, target, max_correspondence_distance, transformation,
                            criteria=ICPConvergenceCriteria(max_iteration=0), **kw)
