// extern "C" entry points of the speckle filter (include/fvo.h): argument checks and the
// workspace-size arithmetic, host-only; the launches are speckle_run's (speckle.hip).  Kept out
// of capi.cpp so that file's host-only sanitizer build (tools/sanitize.sh) links unchanged.
#include <cstdint>

#include "fvo_internal.h"

extern "C" {

int64_t fvo_speckle_workspace_bytes(int32_t batch, int32_t height, int32_t width) {
  if (batch < 0 || height < 1 || width < 1) return -1;
  const int64_t hw = (int64_t)height * width;
  if (hw > INT32_MAX) return -1;  // labels are int32 pixel indices
  if (batch == 0) return 0;
  if (hw > INT64_MAX / 8 / batch) return -1;
  return 8 * hw * batch;  // label + size plane, int32 each
}

int fvo_filter_speckles(fvo_ctx* c, int16_t* disparity, int32_t batch, int32_t height, int32_t width,
                        int64_t image_stride, int32_t pitch, int32_t new_val, int32_t max_speckle_size,
                        int32_t max_diff, void* workspace, int64_t workspace_bytes, fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 0;
  if (!disparity || !workspace) return fvo_fail(c, "null pointer argument");
  if (height < 1 || width < 1) return fvo_fail(c, "filter_speckles: height and width must be >= 1");
  if ((int64_t)height * width > INT32_MAX) return fvo_fail(c, "filter_speckles: height*width exceeds INT32_MAX");
  if (pitch < width || image_stride < (int64_t)pitch * height) return fvo_fail(c, "bad pitch/stride");
  if (new_val < INT16_MIN || new_val > INT16_MAX) return fvo_fail(c, "filter_speckles: new_val outside int16");
  if (max_diff < 0) return fvo_fail(c, "filter_speckles: max_diff < 0");
  const int64_t need = fvo_speckle_workspace_bytes(batch, height, width);
  if (need < 0 || workspace_bytes < need) return fvo_fail(c, "filter_speckles: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return fvo_fail(c, "filter_speckles: workspace must be 4-byte aligned");
  if (max_speckle_size <= 0) return 0;  // cv2: nothing is a speckle
  return speckle_run(c, disparity, batch, height, width, image_stride, pitch, new_val, max_speckle_size, max_diff,
                     workspace, (hipStream_t)stream);
}

}  // extern "C"
