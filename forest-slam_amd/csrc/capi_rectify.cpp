// The stereo-rectification entry points of include/fvo.h (fvo_rectify_map, fvo_remap_u8,
// fvo_rectify_gray, fvo_rectify_lds_budget) and every refusal of theirs: the second file of the
// host-only layer, under capi.cpp's rules (one exact message per refusal through fvo_fail, nothing
// launched or allocated on refusal, no checks in rectify.hip).  It also derives what the kernels
// take instead of the raw calibration: ir = inverse(newK * R).  Host-only: links against stubs of
// the three launchers for the sanitizer program tests/sanitize/rectify_check.cpp.
#include <cmath>
#include <cstring>

#include "fvo_internal.h"

namespace {

// The calibration checks shared by fvo_rectify_map and fvo_rectify_gray; fills L on success.
int make_lens(fvo_ctx* c, const double* K, const double* dist, int32_t n_dist, const double* R, const double* newK,
              RectifyLens* L) {
  if (n_dist != 4 && n_dist != 5 && n_dist != 8) return fvo_fail(c, "rectify: n_dist must be 4, 5 or 8");
  if (!host_all_finite(K, 9) || !host_all_finite(dist, n_dist) || (R && !host_all_finite(R, 9)) ||
      (newK && !host_all_finite(newK, 9)))
    return fvo_fail(c, "rectify: K, dist, R and newK must be finite");
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double* Rm = R ? R : I;
  const double* Nk = newK ? newK : K;
  double A[9];  // newK * R, each entry (a0 b0 + a1 b1) + a2 b2
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[3 * i + j] = (Nk[3 * i] * Rm[j] + Nk[3 * i + 1] * Rm[3 + j]) + Nk[3 * i + 2] * Rm[6 + j];
  if (!host_inv3(A, L->ir)) return fvo_fail(c, "rectify: newK*R is singular");
  // _w is affine in (row, col): the four corners bound it over the image
  const int W = c->cfg.width, H = c->cfg.height;
  for (int k = 0; k < 4; ++k) {
    const int row = (k >> 1) ? H - 1 : 0, col = (k & 1) ? W - 1 : 0;
    const double w = (row * L->ir[7] + L->ir[8]) + col * L->ir[6];
    if (!host_ray_w_ok(w))
      return fvo_fail(c, "rectify: _w <= 0 at an image corner (the view reaches the camera's horizon)");
  }
  L->fx = K[0]; L->fy = K[4]; L->u0 = K[2]; L->v0 = K[5];
  L->k1 = dist[0]; L->k2 = dist[1]; L->p1 = dist[2]; L->p2 = dist[3];
  L->k3 = n_dist >= 5 ? dist[4] : 0.0;
  L->rational = n_dist == 8;
  L->k4 = L->rational ? dist[5] : 0.0;
  L->k5 = L->rational ? dist[6] : 0.0;
  L->k6 = L->rational ? dist[7] : 0.0;
  return 0;
}

// batch, pointers aside: channels and the two image layouts (out_ch bytes per output pixel)
int check_images(fvo_ctx* c, int32_t channels, int64_t src_stride, int32_t src_pitch, int out_ch, int64_t dst_stride,
                 int32_t dst_pitch) {
  if (channels != 1 && channels != 3) return fvo_fail(c, "rectify: channels must be 1 or 3");
  const int64_t W = c->cfg.width, H = c->cfg.height;
  if (W < 1 || H < 1) return fvo_fail(c, "rectify: the context's width and height must be >= 1");
  if (src_pitch < channels * W || src_stride < (int64_t)src_pitch * H || dst_pitch < out_ch * W ||
      dst_stride < (int64_t)dst_pitch * H)
    return fvo_fail(c, "bad pitch/stride");
  return 0;
}

// do the bytes of the two image sets (batch images, the last row ending with its last pixel) overlap
bool images_overlap(fvo_ctx* c, const uint8_t* a, int64_t a_stride, int32_t a_pitch, int a_ch, const uint8_t* b,
                    int64_t b_stride, int32_t b_pitch, int b_ch, int32_t batch) {
  const int64_t W = c->cfg.width, H = c->cfg.height;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  const uintptr_t a1 = a0 + (uintptr_t)((batch - 1) * a_stride + (H - 1) * a_pitch + W * a_ch);
  const uintptr_t b1 = b0 + (uintptr_t)((batch - 1) * b_stride + (H - 1) * b_pitch + W * b_ch);
  return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" {

int fvo_rectify_map(fvo_ctx* c, const double* K, const double* dist, int32_t n_dist, const double* R,
                    const double* newK, int16_t* map1, uint16_t* map2, fvo_stream stream) {
  if (!c) return -1;
  if (!K || !dist || !map1 || !map2) return fvo_fail(c, "null pointer argument");
  if (c->cfg.width < 1 || c->cfg.height < 1)
    return fvo_fail(c, "rectify: the context's width and height must be >= 1");
  if ((reinterpret_cast<uintptr_t>(map1) & 3) || (reinterpret_cast<uintptr_t>(map2) & 1))
    return fvo_fail(c, "rectify: map1 must be 4-byte and map2 2-byte aligned");
  RectifyLens L;
  if (int rc = make_lens(c, K, dist, n_dist, R, newK, &L)) return rc;
  return rectify_map_run(c, L, map1, map2, (hipStream_t)stream);
}

int fvo_remap_u8(fvo_ctx* c, const uint8_t* src, int32_t batch, int64_t src_stride, int32_t src_pitch,
                 int32_t channels, const int16_t* map1, const uint16_t* map2, uint8_t* dst, int64_t dst_stride,
                 int32_t dst_pitch, fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 0;
  if (!src || !map1 || !map2 || !dst) return fvo_fail(c, "null pointer argument");
  if ((reinterpret_cast<uintptr_t>(map1) & 3) || (reinterpret_cast<uintptr_t>(map2) & 1))
    return fvo_fail(c, "rectify: map1 must be 4-byte and map2 2-byte aligned");
  if (int rc = check_images(c, channels, src_stride, src_pitch, channels, dst_stride, dst_pitch)) return rc;
  if (images_overlap(c, src, src_stride, src_pitch, channels, dst, dst_stride, dst_pitch, channels, batch))
    return fvo_fail(c, "remap: dst must not overlap src");
  return remap_run(c, src, batch, src_stride, src_pitch, channels, map1, map2, dst, dst_stride, dst_pitch,
                   (hipStream_t)stream);
}

int fvo_rectify_gray(fvo_ctx* c, const uint8_t* src, int32_t batch, int64_t src_stride, int32_t src_pitch,
                     int32_t channels, const double* K, const double* dist, int32_t n_dist, const double* R,
                     const double* newK, uint8_t* gray, int64_t dst_stride, int32_t dst_pitch, fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 0;
  if (!src || !K || !dist || !gray) return fvo_fail(c, "null pointer argument");
  if (int rc = check_images(c, channels, src_stride, src_pitch, 1, dst_stride, dst_pitch)) return rc;
  if (images_overlap(c, src, src_stride, src_pitch, channels, gray, dst_stride, dst_pitch, 1, batch))
    return fvo_fail(c, "rectify_gray: gray must not overlap src");
  RectifyLens L;
  if (int rc = make_lens(c, K, dist, n_dist, R, newK, &L)) return rc;
  return rectify_gray_run(c, src, batch, src_stride, src_pitch, channels, L, gray, dst_stride, dst_pitch,
                          (hipStream_t)stream);
}

int fvo_rectify_lds_budget(fvo_ctx* c, int32_t bytes) {
  if (!c) return -1;
  if (bytes < 0 || bytes > FVO_RECTIFY_LDS_BYTES)
    return fvo_fail(c, "rectify_lds_budget: bytes outside [0, FVO_RECTIFY_LDS_BYTES]");
  c->rectify_budget = bytes;
  return 0;
}

}  // extern "C"
