// Host-only test double of libfvo's device layer, for the sanitizer programs of this directory
// (capi.cpp + this file + one check program): the per-stage init / launch functions and the few
// HIP runtime calls capi.cpp makes are replaced by functions that record what the entry point
// reached (host_stubs.h).  The inits only allocate, through fvo_alloc and the hipMalloc stub, so
// capi.cpp's own release path frees them; no check or limit of the product is restated here.
// Nothing runs on a GPU.  Test infrastructure only; never linked into libfvo.so.
#include "host_stubs.h"

#include <cstring>

std::string g_last_launch;
int g_launches = 0, g_live_allocs = 0;
hipError_t g_memcpy_result = hipSuccess;
BfArgs g_bf;
SpeckleArgs g_spk;
DenseArgs g_dense;
ReprojectArgs g_rp;
static int g_fake_event = 0;

static int hit(const char* name) {
  g_last_launch = name;
  ++g_launches;
  return 0;
}

// one small allocation the context owns, and the init's name
template <typename T>
static int init(fvo_ctx* c, T** field, const char* name, size_t n = 16) {
  g_last_launch = name;
  return fvo_alloc(c, field, n);
}

// --- HIP runtime calls made by capi.cpp and fvo_alloc
extern "C" {
hipError_t hipSetDevice(int d) { return d >= 0 && d < 8 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipMalloc(void** p, size_t n) {
  *p = new char[n]();
  ++g_live_allocs;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  delete[] static_cast<char*>(p);
  --g_live_allocs;
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind) {
  if (g_memcpy_result == hipSuccess) std::memcpy(dst, src, n);
  return g_memcpy_result;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = reinterpret_cast<hipEvent_t>(&g_fake_event);
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  *ms = 1.0f;
  return hipSuccess;
}
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub hip error"; }
}

// --- stage inits
int orb_init(fvo_ctx* c) { return init(c, &c->pyr, "orb_init"); }
int bf_init(fvo_ctx* c) { return init(c, &c->bf_rowkey, "bf_init"); }
int sgbm_init(fvo_ctx* c) { return init(c, &c->sg_ctl, "sgbm_init", 4 + c->cfg.max_batch); }  // debug buffer 9
int pose_init(fvo_ctx* c) { return init(c, &c->pnp_good, "pose_init"); }
int ba_init(fvo_ctx* c) { return init(c, reinterpret_cast<char**>(&c->ba_ws), "ba_init"); }
int mono_init(fvo_ctx* c) { return init(c, &c->em_x, "mono_init"); }

// --- launchers
int orb_run(fvo_ctx*, const uint8_t*, int, int64_t, int, float*, uint8_t*, int32_t*, int, hipStream_t) {
  return hit("orb_run");
}
int bf_run(fvo_ctx*, const uint8_t*, const int32_t*, const uint8_t*, const int32_t*, int, int, int32_t*, int32_t*,
           hipStream_t) {
  return hit("bf_run");
}
// (the five below also touch the first / last element of every buffer as the entry point sized them)
int bf_knn_run(fvo_ctx*, const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch, int cap,
               int k, int32_t* knn, hipStream_t) {
  g_bf = {batch, cap, k, -1, 0.0, q, t, knn};
  knn[((int64_t)batch * cap * k - 1) * 2 + 1] = q[(int64_t)batch * cap * 32 - 1] + t[(int64_t)batch * cap * 32 - 1];
  knn[0] = nq[batch - 1] + nt[batch - 1] + q[0] + t[0];
  return hit("bf_knn_run");
}
int bf_ratio_run(fvo_ctx*, const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch,
                 int cap, double ratio, int mutual, int32_t* matches, int32_t* nmatch, hipStream_t) {
  g_bf = {batch, cap, 2, mutual, ratio, q, t, matches};
  matches[(int64_t)batch * cap * 3 - 1] = q[(int64_t)batch * cap * 32 - 1] + t[(int64_t)batch * cap * 32 - 1];
  nmatch[batch - 1] = nq[batch - 1] + nt[batch - 1];
  return hit("bf_ratio_run");
}
int speckle_run(fvo_ctx*, int16_t* disp, int batch, int H, int W, int64_t image_stride, int pitch, int new_val,
                int max_speckle_size, int max_diff, void* ws, hipStream_t) {
  g_spk = {batch, H, W, pitch, new_val, max_speckle_size, max_diff, image_stride, ws};
  disp[0] = disp[(int64_t)(batch - 1) * image_stride + (int64_t)(H - 1) * pitch + W - 1];
  return hit("speckle_run");
}
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
  return hit("dense_append_run");
}
int reproject_run(fvo_ctx*, const void* disp, int is_f32, int batch, int H, int W, int64_t image_stride, int pitch,
                  const double* Q, int handle_missing, uint32_t* min_key, float* out, hipStream_t) {
  g_rp = {disp, Q, min_key, out, is_f32, batch, H, W, pitch, handle_missing, image_stride};
  const int64_t last = (int64_t)(batch - 1) * image_stride + (int64_t)(H - 1) * pitch + W - 1;
  const float d = is_f32 ? static_cast<const float*>(disp)[last] : (float)static_cast<const int16_t*>(disp)[last];
  out[(int64_t)batch * H * W * 3 - 1] = d + (float)Q[15];
  out[0] = 0.f;
  if (handle_missing) min_key[batch - 1] = 0;
  return hit("reproject_run");
}
int sgbm_run(fvo_ctx*, const uint8_t*, const uint8_t*, int, int64_t, int, int16_t*, int32_t*, hipStream_t) {
  return hit("sgbm_run");
}
int backproject_run(fvo_ctx*, const int16_t*, const float*, const float*, const int32_t*, const int32_t*, int, int,
                    const double*, double, float*, float*, int32_t*, hipStream_t) {
  return hit("backproject_run");
}
int pnp_run(fvo_ctx*, const float*, const float*, const int32_t*, int, int, const double*, const double*, float, double,
            int, double*, double*, double*, int32_t*, uint8_t*, hipStream_t) {
  return hit("pnp_run");
}
int ba_stereo_run(fvo_ctx*, const int16_t*, const float*, const int32_t*, int, int, const double*, double, float*,
                  hipStream_t) {
  return hit("ba_stereo_run");
}
int ba_run(fvo_ctx*, const float*, const int32_t*, const int32_t*, const int32_t*, const float*, const double*, int, int,
           int, int, int, const double*, double, const double*, int, int, double*, double*, hipStream_t) {
  return hit("ba_run");
}
int ba_export_run(fvo_ctx*, int, double*, int32_t*, hipStream_t) { return hit("ba_export_run"); }
int ba_births_run(fvo_ctx*, const int32_t*, const int32_t*, const float*, int, int, int, int, int, hipStream_t) {
  return hit("ba_births_run");
}
int gather_run(fvo_ctx*, const float*, const float*, const int32_t*, const int32_t*, int, int, float*, float*, int32_t*,
               hipStream_t) {
  return hit("gather_run");
}
int essential_run(fvo_ctx*, const float*, const float*, const int32_t*, int, int, double, double, double, double, double,
                  int, double*, uint8_t*, int32_t*, hipStream_t) {
  return hit("essential_run");
}
int recover_run(fvo_ctx*, const double*, const int32_t*, const float*, const float*, const int32_t*, int, int, double,
                double, double, double, double*, double*, double*, int32_t*, hipStream_t) {
  return hit("recover_run");
}
int ingest_run(fvo_ctx*, const uint8_t*, int, int64_t, int, const double*, const double*, uint8_t*, int64_t, int,
               hipStream_t) {
  return hit("ingest_run");
}
int motion_blur_run(fvo_ctx*, const uint8_t*, int, int64_t, int, int, const int32_t*, const int32_t*, int, uint8_t*,
                    uint8_t*, int64_t, int, hipStream_t) {
  return hit("motion_blur_run");
}
int map_transform_run(fvo_ctx*, const float*, int, const int32_t*, int, int64_t, const double*, int32_t*, int64_t,
                      double*, float*, hipStream_t) {
  return hit("map_transform_run");
}
int chain_poses_run(fvo_ctx*, const double*, const int32_t*, const int32_t*, int, int, double*, double*, int32_t*,
                    hipStream_t) {
  return hit("chain_poses_run");
}
int copy_regions_run(fvo_ctx*, int, const fvo_region*, hipStream_t) { return hit("copy_regions_run"); }
int count_guard_run(fvo_ctx*, const int32_t*, const int32_t*, int, int, int32_t*, int32_t, int32_t*, hipStream_t) {
  return hit("count_guard_run");
}
int64_t voxel_workspace_bytes(int64_t n) { return 64 * n + 4096; }
int voxel_run(fvo_ctx*, const double*, int64_t, double, void*, double*, int32_t*, int32_t*, hipStream_t) {
  return hit("voxel_run");
}
int orb_blur_debug(fvo_ctx*) { return hit("orb_blur_debug"); }
int orb_score_debug(fvo_ctx*) { return hit("orb_score_debug"); }
int orb_retain_best_run(fvo_ctx*, const float*, int, int, int32_t*, int32_t*, hipStream_t) {
  return hit("orb_retain_best_run");
}
