// The outlier-removal entry points of include/fvo.h (fvo_outlier_workspace_bytes,
// fvo_statistical_outliers, fvo_radius_outliers, fvo_select_points) and every refusal of theirs: the
// fourth file of the host-only layer, under capi.cpp's rules (one exact message per refusal through
// fvo_fail, nothing launched or allocated on refusal, no checks in outlier.hip).  Host-only: links
// against stubs of the launchers for the sanitizer program tests/sanitize/outlier_check.cpp.
#include <cmath>
#include <cstdint>

#include "fvo_internal.h"

static bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

// do [a, a + na) and [b, b + nb) share a byte
static bool ranges_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

extern "C" {

int64_t fvo_outlier_workspace_bytes(int64_t n_points, int32_t nb_neighbors) {
  if (n_points < 0 || n_points > INT32_MAX || nb_neighbors < 1 || nb_neighbors > FVO_OUTLIER_MAX_K) return -1;
  if (n_points == 0) return 0;
  return outlier_workspace_bytes(n_points);
}

int fvo_statistical_outliers(fvo_ctx* c, const double* points, int64_t n_points, int32_t nb_neighbors,
                             double std_ratio, double cell, int32_t max_rings, void* workspace,
                             int64_t workspace_bytes, uint8_t* keep, double* avg_distance, double* stats,
                             int32_t* status, fvo_stream stream) {
  if (!c) return -1;
  if (!stats || (n_points > 0 && (!points || !workspace || !keep))) return fvo_fail(c, "null pointer argument");
  if (n_points < 0 || n_points > INT32_MAX) return fvo_fail(c, "n_points out of range");
  if (nb_neighbors < 1 || nb_neighbors > FVO_OUTLIER_MAX_K)
    return fvo_fail(c, "statistical_outliers: nb_neighbors must be in [1, 64]");
  if (!std::isfinite(std_ratio)) return fvo_fail(c, "statistical_outliers: std_ratio must be finite");
  if (!finite_pos(cell)) return fvo_fail(c, "statistical_outliers: cell must be finite and > 0");
  if (max_rings < 0 || max_rings > 8) return fvo_fail(c, "statistical_outliers: max_rings must be in [0, 8]");
  if (n_points == 0) {  // Open3D: an empty cloud keeps nothing; every statistic is 0
    FVO_HIP(c, hipMemsetAsync(stats, 0, 6 * sizeof(double), (hipStream_t)stream));
    if (status) FVO_HIP(c, hipMemsetAsync(status, 0, 4, (hipStream_t)stream));
    return 0;
  }
  const int64_t need = outlier_workspace_bytes(n_points);  // statistical_outliers_run's layout total
  if (need < 0) return fvo_fail(c, "statistical_outliers: workspace size query failed");
  if (workspace_bytes < need) return fvo_fail(c, "statistical_outliers: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 7)
    return fvo_fail(c, "statistical_outliers: workspace must be 8-byte aligned");
  return statistical_outliers_run(c, points, n_points, nb_neighbors, std_ratio, cell, max_rings, workspace, keep,
                                  avg_distance, stats, status, (hipStream_t)stream);
}

int fvo_radius_outliers(fvo_ctx* c, const double* points, int64_t n_points, int32_t nb_points, double radius,
                        double cell, void* workspace, int64_t workspace_bytes, uint8_t* keep, int32_t* n_neighbors,
                        int32_t* status, fvo_stream stream) {
  if (!c) return -1;
  if (n_points > 0 && (!points || !workspace || !keep)) return fvo_fail(c, "null pointer argument");
  if (n_points < 0 || n_points > INT32_MAX) return fvo_fail(c, "n_points out of range");
  if (nb_points < 0) return fvo_fail(c, "radius_outliers: nb_points must be >= 0");
  if (!finite_pos(radius)) return fvo_fail(c, "radius_outliers: radius must be finite and > 0");
  if (!finite_pos(cell)) return fvo_fail(c, "radius_outliers: cell must be finite and > 0");
  if (!(radius / cell <= 8.0)) return fvo_fail(c, "radius_outliers: radius / cell must be <= 8");
  if (n_points == 0) {
    if (status) FVO_HIP(c, hipMemsetAsync(status, 0, 4, (hipStream_t)stream));
    return 0;
  }
  const int64_t need = outlier_workspace_bytes(n_points);  // radius_outliers_run's layout total
  if (need < 0) return fvo_fail(c, "radius_outliers: workspace size query failed");
  if (workspace_bytes < need) return fvo_fail(c, "radius_outliers: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return fvo_fail(c, "radius_outliers: workspace must be 8-byte aligned");
  return radius_outliers_run(c, points, n_points, nb_points, radius, cell, workspace, keep, n_neighbors, status,
                             (hipStream_t)stream);
}

int fvo_select_points(fvo_ctx* c, const double* points, int64_t n_points, const uint8_t* keep, double* out64,
                      float* out32, int32_t* n_out, fvo_stream stream) {
  if (!c) return -1;
  if (!n_out || (n_points > 0 && (!points || !keep))) return fvo_fail(c, "null pointer argument");
  if (!out64 && !out32) return fvo_fail(c, "select_points: out64 and out32 are both NULL");
  if (n_points < 0 || n_points > INT32_MAX) return fvo_fail(c, "n_points out of range");
  if (n_points == 0) {
    FVO_HIP(c, hipMemsetAsync(n_out, 0, 4, (hipStream_t)stream));
    return 0;
  }
  if (out64 && ranges_overlap(points, 24 * n_points, out64, 24 * n_points))
    return fvo_fail(c, "select_points: out64 overlaps points");
  if (out32 && ranges_overlap(points, 24 * n_points, out32, 12 * n_points))
    return fvo_fail(c, "select_points: out32 overlaps points");
  return select_points_run(c, points, n_points, keep, out64, out32, n_out, (hipStream_t)stream);
}

}  // extern "C"
