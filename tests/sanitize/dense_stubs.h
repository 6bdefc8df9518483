// What tests/sanitize/dense_stubs.cpp records for dense_check.cpp to read (beside host_stubs.h).
#pragma once

#include "host_stubs.h"

// the arguments dense_append_run / reproject_run were last called with
struct DenseArgs {
  const void *disp, *K, *keep, *T, *count, *out64, *out32, *n_added, *ws;
  int batch, H, W, pitch, step, min_disp16;
  int64_t stride, map_cap;
  double baseline;
  float z_min, z_max;
};
struct ReprojectArgs {
  const void *disp, *Q, *key, *out;
  int is_f32, batch, H, W, pitch, handle;
  int64_t stride;
};
extern DenseArgs g_dense;
extern ReprojectArgs g_rp;
