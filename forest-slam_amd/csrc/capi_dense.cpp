// The dense-mapping entry points of libfvo.so (include/fvo.h): fvo_dense_workspace_bytes,
// fvo_dense_map_append and fvo_reproject_to_3d.  Host-only, under capi.cpp's rules: every refusal
// that depends only on the arguments is made here, by its exact message through fvo_fail, before
// anything is launched; batch == 0 returns 0 before the pointer checks; the launchers
// (dense_append_run, reproject_run: dense.hip) call fvo_fail for HIP runtime errors only.  Links
// against tests/sanitize/host_stubs.cpp + dense_stubs.cpp for the sanitizer program
// tests/sanitize/dense_check.cpp.
#include <cmath>
#include <cstdint>

#include "fvo_internal.h"

namespace {

// blocks of all frames, or -1 when the size is refused
int64_t dense_blocks(int32_t batch, int32_t height, int32_t width, int32_t step) {
  if (batch < 0 || height < 1 || width < 1 || step < 1) return -1;
  if ((int64_t)height * width > INT32_MAX) return -1;  // flat sample indices are 32-bit
  const int64_t n = dense_frame_blocks(height, width, step) * batch;
  return n > INT32_MAX ? -1 : n;  // one launch block each
}

}  // namespace

extern "C" {

int64_t fvo_dense_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t step) {
  const int64_t n = dense_blocks(batch, height, width, step);
  if (n < 0) return -1;
  if (batch == 0) return 0;
  return 8 + 12 * n;  // the map base, an int64 offset and an int32 count per block
}

int fvo_dense_map_append(fvo_ctx* c, const int16_t* disparity, int32_t batch, int32_t height, int32_t width,
                         int64_t image_stride, int32_t pitch, const double* K, double baseline, int32_t step,
                         int32_t min_disp16, float z_min, float z_max, const int32_t* frame_keep, const double* T,
                         int32_t* map_count, int64_t map_cap, double* map_xyz64, float* map_xyz32, int32_t* n_added,
                         void* workspace, int64_t workspace_bytes, fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0) return fvo_fail(c, "batch < 0");
  if (batch == 0) return 0;
  if (!disparity || !K || !T || !map_count || !workspace || (!map_xyz64 && !map_xyz32))
    return fvo_fail(c, "null pointer argument");
  if (height < 1 || width < 1) return fvo_fail(c, "dense_map_append: height and width must be >= 1");
  if ((int64_t)height * width > INT32_MAX) return fvo_fail(c, "dense_map_append: height*width exceeds INT32_MAX");
  if (pitch < width || image_stride < (int64_t)pitch * height) return fvo_fail(c, "bad pitch/stride");
  if (step < 1) return fvo_fail(c, "dense_map_append: step must be >= 1");
  if (!std::isfinite(z_min) || !std::isfinite(z_max) || !(z_min >= 0.f && z_min < z_max))
    return fvo_fail(c, "dense_map_append: z_min and z_max must be finite with 0 <= z_min < z_max");
  if (!std::isfinite(K[0]) || !std::isfinite(K[4]) || !std::isfinite(baseline) || K[0] <= 0.0 || K[4] <= 0.0 ||
      baseline <= 0.0)
    return fvo_fail(c, "dense_map_append: K[0], K[4] and baseline must be finite and > 0");
  if (map_cap < 0) return fvo_fail(c, "map_cap < 0");
  const int64_t need = fvo_dense_workspace_bytes(batch, height, width, step);
  if (need < 0) return fvo_fail(c, "dense_map_append: batch * sample blocks exceeds INT32_MAX");
  if (workspace_bytes < need) return fvo_fail(c, "dense_map_append: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 7)
    return fvo_fail(c, "dense_map_append: workspace must be 8-byte aligned");
  return dense_append_run(c, disparity, batch, height, width, image_stride, pitch, K, baseline, step, min_disp16,
                          z_min, z_max, frame_keep, T, map_count, map_cap, map_xyz64, map_xyz32, n_added, workspace,
                          (hipStream_t)stream);
}

int fvo_reproject_to_3d(fvo_ctx* c, const void* disparity, int32_t is_float32, int32_t batch, int32_t height,
                        int32_t width, int64_t image_stride, int32_t pitch, const double* Q,
                        int32_t handle_missing_values, uint32_t* min_key, float* out, fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0) return fvo_fail(c, "batch < 0");
  if (batch == 0) return 0;
  if (!disparity || !Q || !out || (handle_missing_values && !min_key)) return fvo_fail(c, "null pointer argument");
  if (is_float32 != 0 && is_float32 != 1)
    return fvo_fail(c, "reproject_to_3d: is_float32 must be 0 (int16) or 1 (float32)");
  if (height < 1 || width < 1) return fvo_fail(c, "reproject_to_3d: height and width must be >= 1");
  if ((int64_t)height * width > INT32_MAX) return fvo_fail(c, "reproject_to_3d: height*width exceeds INT32_MAX");
  if (pitch < width || image_stride < (int64_t)pitch * height) return fvo_fail(c, "bad pitch/stride");
  // one launch block per 256 pixels of every image
  if ((((int64_t)height * width + 255) / 256) * batch > INT32_MAX)
    return fvo_fail(c, "reproject_to_3d: batch*height*width too large for one launch");
  return reproject_run(c, disparity, is_float32, batch, height, width, image_stride, pitch, Q,
                       handle_missing_values != 0, min_key, out, (hipStream_t)stream);
}

}  // extern "C"
