// What tests/sanitize/host_stubs.cpp records for the check programs to read.
#pragma once

#include <string>

#include "../../forest-slam_amd/csrc/fvo_internal.h"

extern std::string g_last_launch;   // name of the init or launcher reached last
extern int g_launches;              // launcher calls (inits not counted)
extern int g_live_allocs;           // hipMalloc calls not yet matched by a hipFree
extern hipError_t g_memcpy_result;  // what the hipMemcpy stub answers (hipSuccess: it copies)

// the arguments bf_knn_run / bf_ratio_run, speckle_run, dense_append_run and reproject_run were last
// called with
struct BfArgs {
  int batch, cap, k, mutual;
  double ratio;
  const void *q, *t, *out;
};
struct SpeckleArgs {
  int batch, H, W, pitch, new_val, max_size, max_diff;
  int64_t stride;
  void* ws;
};
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
extern BfArgs g_bf;
extern SpeckleArgs g_spk;
extern DenseArgs g_dense;
extern ReprojectArgs g_rp;
