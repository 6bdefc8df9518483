// The sparse-stereo entry points of include/fvo.h (fvo_sparse_stereo_params_default,
// fvo_sparse_stereo_workspace_bytes, fvo_sparse_stereo, fvo_backproject_stereo) and every refusal
// of theirs: the third file of the host-only layer, under capi.cpp's rules (one exact message per
// refusal through fvo_fail, nothing launched or allocated on refusal, no checks in
// sparse_stereo.hip).  Host-only: links against stubs of the two launchers for the sanitizer
// program tests/sanitize/stereo_check.cpp.
#include <cmath>
#include <cstring>

#include "fvo_internal.h"

extern "C" {

void fvo_sparse_stereo_params_default(fvo_sparse_stereo_params* p) {
  if (!p) return;
  p->min_disparity = 1.0f;
  p->max_disparity = 96.0f;
  p->row_tol = 2.0f;
  p->max_hamming = 75;
  p->max_octave_diff = 1;
  p->half_window = 5;
  p->half_slide = 5;
  p->unique = 1;
}

int64_t fvo_sparse_stereo_workspace_bytes(int32_t batch, int32_t cap) {
  if (batch < 0 || cap < 1 || cap > 0xFFFF) return -1;
  return 8 * (int64_t)batch * cap;  // a u32 key per left and per right keypoint
}

int fvo_sparse_stereo(fvo_ctx* c, const uint8_t* left, const uint8_t* right, int32_t batch, int64_t image_stride,
                      int32_t pitch, const float* kpL, const int32_t* nL, const uint8_t* descL, const float* kpR,
                      const int32_t* nR, const uint8_t* descR, int32_t cap, const fvo_sparse_stereo_params* p,
                      const float* level_scale, int32_t n_levels, const double* K, double baseline, void* workspace,
                      int64_t workspace_bytes, float* stereo, int32_t* info, fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 0;
  if (!left || !right || !kpL || !nL || !descL || !kpR || !nR || !descR || !p || !level_scale || !K || !workspace ||
      !stereo)
    return fvo_fail(c, "null pointer argument");
  if (c->cfg.width < 1 || c->cfg.height < 1)
    return fvo_fail(c, "sparse_stereo: the context's width and height must be >= 1");
  if (pitch < c->cfg.width || image_stride < (int64_t)pitch * c->cfg.height) return fvo_fail(c, "bad pitch/stride");
  if (!std::isfinite(p->min_disparity) || p->min_disparity <= 0.f)
    return fvo_fail(c, "sparse_stereo: min_disparity must be finite and > 0");
  if (!(p->max_disparity >= p->min_disparity))
    return fvo_fail(c, "sparse_stereo: max_disparity must be >= min_disparity");
  if (!std::isfinite(p->row_tol) || p->row_tol < 0.f)
    return fvo_fail(c, "sparse_stereo: row_tol must be finite and >= 0");
  if (p->max_hamming < 0 || p->max_hamming > 256) return fvo_fail(c, "sparse_stereo: max_hamming must be in [0, 256]");
  if (p->half_window < 1 || p->half_window > kSparseMaxHalfWindow)
    return fvo_fail(c, "sparse_stereo: half_window must be in [1, 7]");
  if (p->half_slide < 1 || p->half_slide > kSparseMaxHalfSlide)
    return fvo_fail(c, "sparse_stereo: half_slide must be in [1, 8]");
  if (p->max_octave_diff < 0) return fvo_fail(c, "sparse_stereo: max_octave_diff must be >= 0");
  if (n_levels < 1 || n_levels > kSparseMaxLevels) return fvo_fail(c, "sparse_stereo: n_levels must be in [1, 32]");
  if (cap < 1 || cap > 0xFFFF) return fvo_fail(c, "sparse_stereo: cap must be in [1, 65535]");
  if (workspace_bytes < fvo_sparse_stereo_workspace_bytes(batch, cap))
    return fvo_fail(c, "sparse_stereo: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return fvo_fail(c, "sparse_stereo: workspace must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(descL) | reinterpret_cast<uintptr_t>(descR)) & 15)
    return fvo_fail(c, "descriptor buffers must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(stereo) | reinterpret_cast<uintptr_t>(info)) & 15)
    return fvo_fail(c, "sparse_stereo: stereo and info must be 16-byte aligned");
  SparseLevels lv;
  std::memset(&lv, 0, sizeof(lv));
  std::memcpy(lv.scale, level_scale, sizeof(float) * n_levels);
  lv.n = n_levels;
  return sparse_stereo_run(c, left, right, batch, image_stride, pitch, kpL, nL, descL, kpR, nR, descR, cap, *p, lv, K,
                           baseline, workspace, stereo, info, (hipStream_t)stream);
}

int fvo_backproject_stereo(fvo_ctx* c, const float* stereo, const float* kp0, const float* kp1,
                           const int32_t* matches, const int32_t* n_matches, int32_t batch, int32_t cap,
                           float* points3d, float* points2d, int32_t* n_points, fvo_stream stream) {
  (void)kp0;
  if (!c) return -1;
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 0;
  if (!stereo || !kp1 || !matches || !n_matches || !points3d || !points2d || !n_points)
    return fvo_fail(c, "null pointer argument");
  if (cap < 1) return fvo_fail(c, "cap must be >= 1");
  if (reinterpret_cast<uintptr_t>(stereo) & 15) return fvo_fail(c, "stereo buffer must be 16-byte aligned");
  return backproject_stereo_run(c, stereo, kp1, matches, n_matches, batch, cap, points3d, points2d, n_points,
                                (hipStream_t)stream);
}

}  // extern "C"
