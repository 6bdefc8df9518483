// The registration entry points of include/fvo.h (fvo_icp_workspace_bytes, fvo_registration_icp,
// fvo_transform_points) and every refusal of theirs: the sixth file of the host-only layer, under
// capi.cpp's rules (one exact message per refusal through fvo_fail, nothing launched or allocated on
// refusal, no checks in icp.hip).  Host-only: links against stubs of the launchers for the sanitizer
// program tests/sanitize/icp_check.cpp.
#include <cmath>
#include <cstdint>

#include "fvo_internal.h"

static bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

// the checks of a host 4x4 rigid transform; nullptr when it passes
static const char* bad_transform(const double* T, const char* not_finite, const char* bottom) {
  if (!host_all_finite(T, 16)) return not_finite;
  if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) return bottom;
  return nullptr;
}

extern "C" {

int64_t fvo_icp_workspace_bytes(int64_t n_source, int64_t n_target) {
  if (n_source < 0 || n_source > INT32_MAX || n_target < 0 || n_target > INT32_MAX) return -1;
  if (n_source == 0 || n_target == 0) return 0;
  return icp_workspace_bytes(n_source, n_target);
}

int fvo_registration_icp(fvo_ctx* c, const double* source, int64_t n_source, const double* target,
                         const double* target_normals, int64_t n_target, double max_correspondence_distance,
                         double cell, const double* init, int32_t estimation, double relative_fitness,
                         double relative_rmse, int32_t max_iteration, void* workspace, int64_t workspace_bytes,
                         double* result, double* sums, int32_t* correspondences, int32_t* status, fvo_stream stream) {
  if (!c) return -1;
  if (!init || !result || (n_source > 0 && !source) || (n_target > 0 && !target) ||
      (n_source > 0 && n_target > 0 && !workspace))
    return fvo_fail(c, "null pointer argument");
  if (n_source < 0 || n_source > INT32_MAX) return fvo_fail(c, "n_source out of range");
  if (n_target < 0 || n_target > INT32_MAX) return fvo_fail(c, "n_target out of range");
  if (estimation != 0 && estimation != 1) return fvo_fail(c, "registration_icp: estimation must be 0 or 1");
  if (!finite_pos(max_correspondence_distance))
    return fvo_fail(c, "registration_icp: max_correspondence_distance must be finite and > 0");
  if (!finite_pos(cell)) return fvo_fail(c, "registration_icp: cell must be finite and > 0");
  if (!(max_correspondence_distance / cell <= 8.0))
    return fvo_fail(c, "registration_icp: max_correspondence_distance / cell must be <= 8");
  if (const char* m = bad_transform(init, "registration_icp: init must be finite",
                                    "registration_icp: the bottom row of init must be (0, 0, 0, 1)"))
    return fvo_fail(c, m);
  if (estimation == 1 && n_target > 0 && !target_normals)
    return fvo_fail(c, "registration_icp: point-to-plane needs target_normals");
  if (!(relative_fitness >= 0.0) || !(relative_rmse >= 0.0))
    return fvo_fail(c, "registration_icp: relative_fitness and relative_rmse must be >= 0");
  if (max_iteration < 0 || max_iteration > FVO_ICP_MAX_ITERATION)
    return fvo_fail(c, "registration_icp: max_iteration must be in [0, 1000]");
  if (n_source == 0 || n_target == 0)  // no search: the init transform, fitness 0, every correspondence -1
    return icp_trivial_run(c, init, n_source, result, sums, correspondences, status, (hipStream_t)stream);
  const int64_t need = icp_workspace_bytes(n_source, n_target);  // registration_icp_run's layout total
  if (need < 0) return fvo_fail(c, "registration_icp: workspace size query failed");
  if (workspace_bytes < need) return fvo_fail(c, "registration_icp: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 7)
    return fvo_fail(c, "registration_icp: workspace must be 8-byte aligned");
  return registration_icp_run(c, source, n_source, target, target_normals, n_target, max_correspondence_distance,
                              cell, init, estimation, relative_fitness, relative_rmse, max_iteration, workspace,
                              result, sums, correspondences, status, (hipStream_t)stream);
}

int fvo_transform_points(fvo_ctx* c, double* points, float* points32, double* normals, int64_t n_points,
                         const double* T, fvo_stream stream) {
  if (!c) return -1;
  if (!T || (n_points > 0 && !points)) return fvo_fail(c, "null pointer argument");
  if (n_points < 0 || n_points > INT32_MAX) return fvo_fail(c, "n_points out of range");
  if (const char* m = bad_transform(T, "transform_points: T must be finite",
                                    "transform_points: the bottom row of T must be (0, 0, 0, 1)"))
    return fvo_fail(c, m);
  if (n_points == 0) return 0;
  return transform_points_run(c, points, points32, normals, n_points, T, (hipStream_t)stream);
}

}  // extern "C"
