// The normal-estimation entry points of include/fvo.h (fvo_normals_workspace_bytes,
// fvo_estimate_normals, fvo_orient_normals) and every refusal of theirs: the fifth file of the
// host-only layer, under capi.cpp's rules (one exact message per refusal through fvo_fail, nothing
// launched or allocated on refusal, no checks in normals.hip).  Host-only: links against stubs of the
// launchers for the sanitizer program tests/sanitize/normals_check.cpp.
#include <cmath>
#include <cstdint>

#include "fvo_internal.h"

static bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

extern "C" {

int64_t fvo_normals_workspace_bytes(int64_t n_points, int32_t max_nn) {
  if (n_points < 0 || n_points > INT32_MAX || max_nn < 1 || max_nn > FVO_NORMALS_MAX_NN) return -1;
  if (n_points == 0) return 0;
  return normals_workspace_bytes(n_points);
}

int fvo_estimate_normals(fvo_ctx* c, const double* points, int64_t n_points, int32_t max_nn, double radius,
                         double cell, int32_t max_rings, void* workspace, int64_t workspace_bytes, double* normals,
                         int32_t has_prior, double* covariances, int32_t* n_neighbors, int32_t* stats,
                         int32_t* status, fvo_stream stream) {
  if (!c) return -1;
  if (!stats || (n_points > 0 && (!points || !workspace || !normals))) return fvo_fail(c, "null pointer argument");
  if (n_points < 0 || n_points > INT32_MAX) return fvo_fail(c, "n_points out of range");
  if (max_nn < 1 || max_nn > FVO_NORMALS_MAX_NN) return fvo_fail(c, "estimate_normals: max_nn must be in [1, 64]");
  if (!(radius > 0.0)) return fvo_fail(c, "estimate_normals: radius must be > 0");  // NaN too; +inf: plain k-NN
  if (!finite_pos(cell)) return fvo_fail(c, "estimate_normals: cell must be finite and > 0");
  if (max_rings < 0 || max_rings > 8) return fvo_fail(c, "estimate_normals: max_rings must be in [0, 8]");
  if (n_points == 0) {
    FVO_HIP(c, hipMemsetAsync(stats, 0, 2 * sizeof(int32_t), (hipStream_t)stream));
    if (status) FVO_HIP(c, hipMemsetAsync(status, 0, 4, (hipStream_t)stream));
    return 0;
  }
  const int64_t need = normals_workspace_bytes(n_points);  // estimate_normals_run's layout total
  if (need < 0) return fvo_fail(c, "estimate_normals: workspace size query failed");
  if (workspace_bytes < need) return fvo_fail(c, "estimate_normals: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 7)
    return fvo_fail(c, "estimate_normals: workspace must be 8-byte aligned");
  return estimate_normals_run(c, points, n_points, max_nn, radius, cell, max_rings, workspace, normals,
                              has_prior != 0, covariances, n_neighbors, stats, status, (hipStream_t)stream);
}

int fvo_orient_normals(fvo_ctx* c, const double* points, double* normals, int64_t n_points, int32_t mode,
                       const double* ref, fvo_stream stream) {
  if (!c) return -1;
  if (!ref || (n_points > 0 && (!points || !normals))) return fvo_fail(c, "null pointer argument");
  if (n_points < 0 || n_points > INT32_MAX) return fvo_fail(c, "n_points out of range");
  if (mode != 0 && mode != 1) return fvo_fail(c, "orient_normals: mode must be 0 or 1");
  if (!host_all_finite(ref, 3)) return fvo_fail(c, "orient_normals: ref must be finite");
  if (mode == 1 && ref[0] == 0.0 && ref[1] == 0.0 && ref[2] == 0.0)
    return fvo_fail(c, "orient_normals: direction must not be all zeros");
  if (n_points == 0) return 0;
  return orient_normals_run(c, points, normals, n_points, mode, ref, (hipStream_t)stream);
}

}  // extern "C"
