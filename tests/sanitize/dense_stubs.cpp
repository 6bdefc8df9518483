// Host-only test doubles of dense.hip's launchers, linked beside host_stubs.cpp (which stubs the
// HIP runtime and every other launcher) into the sanitizer program dense_check.cpp: they record
// what csrc/capi_dense.cpp passed on and touch the first / last element of the buffers as the
// entry point sized them.  Nothing runs on a GPU.  Test infrastructure only.
#include "dense_stubs.h"

DenseArgs g_dense;
ReprojectArgs g_rp;

int dense_append_run(fvo_ctx*, const int16_t* disp, int batch, int H, int W, int64_t image_stride, int pitch,
                     const double* K, double baseline, int step, int min_disp16, float z_min, float z_max,
                     const int32_t* frame_keep, const double* T, int32_t* count, int64_t map_cap, double* out64,
                     float* out32, int32_t* n_added, void* ws, hipStream_t) {
  g_dense = {disp, K,    frame_keep, T,          count,        out64,   out32,    n_added, ws,   batch,
             H,    W,    pitch,      step,       min_disp16,   image_stride, map_cap, baseline, z_min, z_max};
  // the workspace as fvo_dense_workspace_bytes sizes it: the base, then per block an offset and a count
  const int64_t n = dense_frame_blocks(H, W, step) * batch;
  int64_t* base = static_cast<int64_t*>(ws);
  int32_t* cnt = reinterpret_cast<int32_t*>(base + 1 + n);
  base[0] = disp[0] + disp[(int64_t)(batch - 1) * image_stride + (int64_t)(H - 1) * pitch + W - 1];
  base[n] = (int64_t)(K[8] + T[16 * batch - 1]);
  cnt[n - 1] = count[0] + (frame_keep ? frame_keep[batch - 1] : 0);
  if (n_added) n_added[batch - 1] = 0;
  g_last_launch = "dense_append_run";
  ++g_launches;
  return 0;
}

int reproject_run(fvo_ctx*, const void* disp, int is_f32, int batch, int H, int W, int64_t image_stride, int pitch,
                  const double* Q, int handle_missing, uint32_t* min_key, float* out, hipStream_t) {
  g_rp = {disp, Q, min_key, out, is_f32, batch, H, W, pitch, handle_missing, image_stride};
  const int64_t last = (int64_t)(batch - 1) * image_stride + (int64_t)(H - 1) * pitch + W - 1;
  const float d = is_f32 ? static_cast<const float*>(disp)[last] : (float)static_cast<const int16_t*>(disp)[last];
  out[(int64_t)batch * H * W * 3 - 1] = d + (float)Q[15];
  out[0] = 0.f;
  if (handle_missing) min_key[batch - 1] = 0;
  g_last_launch = "reproject_run";
  ++g_launches;
  return 0;
}
