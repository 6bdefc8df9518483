// Every extern "C" entry point of libfvo.so (include/fvo.h) and every refusal that depends only on
// the arguments, fvo_config and host fields of fvo_ctx: config checks (check_<stage>_config, run by
// fvo_create before the first allocation), argument checks, context lifetime, dispatch to the
// per-stage launchers.  Host-only: links against tests/sanitize/host_stubs.cpp for the sanitizer
// programs.  No allocation in the hot calls.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "fvo_internal.h"
#include "sgbm_params.h"

int fvo_fail(fvo_ctx* ctx, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return -1;
}

hipEvent_t fvo_event(fvo_ctx* ctx) {
  if (!ctx->tpool.empty()) {
    hipEvent_t e = ctx->tpool.back();
    ctx->tpool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

// The ABI layout: 31 int32 / float fields, no padding (include/fvo.h).
static_assert(sizeof(fvo_config) == 31 * 4, "fvo_config layout changed: bump FVO_ABI_VERSION");
static_assert(offsetof(fvo_config, scale_factor) == 16 && offsetof(fvo_config, sgbm_max_batch) == 104 &&
                  offsetof(fvo_config, sgbm_handoff_us) == 120,
              "fvo_config field offsets changed: bump FVO_ABI_VERSION");

extern "C" {

int fvo_abi_version(void) { return FVO_ABI_VERSION; }

int32_t fvo_config_size(void) { return (int32_t)sizeof(fvo_config); }

int32_t fvo_config_offset(const char* f) {
  if (!f) return -1;
#define FVO_OFS(name) if (!std::strcmp(f, #name)) return (int32_t)offsetof(fvo_config, name);
  FVO_OFS(width) FVO_OFS(height) FVO_OFS(max_batch) FVO_OFS(nfeatures) FVO_OFS(scale_factor) FVO_OFS(nlevels)
  FVO_OFS(edge_threshold) FVO_OFS(first_level) FVO_OFS(wta_k) FVO_OFS(score_type) FVO_OFS(patch_size)
  FVO_OFS(fast_threshold) FVO_OFS(min_disparity) FVO_OFS(num_disparities) FVO_OFS(block_size) FVO_OFS(P1)
  FVO_OFS(P2) FVO_OFS(disp12_max_diff) FVO_OFS(pre_filter_cap) FVO_OFS(uniqueness_ratio) FVO_OFS(sgbm_stripes)
  FVO_OFS(kp_capacity) FVO_OFS(stages) FVO_OFS(ba_window) FVO_OFS(ba_max_landmarks) FVO_OFS(ba_max_obs)
  FVO_OFS(sgbm_max_batch) FVO_OFS(sgbm_mode) FVO_OFS(sgbm_lanes) FVO_OFS(sgbm_cols) FVO_OFS(sgbm_handoff_us)
#undef FVO_OFS
  return -1;
}

void fvo_config_default(fvo_config* c, int32_t width, int32_t height) {
  std::memset(c, 0, sizeof(*c));
  c->width = width;
  c->height = height;
  c->max_batch = 1;
  c->nfeatures = 500;
  c->scale_factor = 1.2f;
  c->nlevels = 8;
  c->edge_threshold = 31;
  c->first_level = 0;
  c->wta_k = 2;
  c->score_type = 0;
  c->patch_size = 31;
  c->fast_threshold = 20;
  c->min_disparity = 0;
  c->num_disparities = 6 * 16;
  c->block_size = 7;
  c->P1 = 8 * 7 * 7;
  c->P2 = 32 * 7 * 7;
  c->disp12_max_diff = 0;
  c->pre_filter_cap = 0;
  c->uniqueness_ratio = 0;
  c->sgbm_stripes = 4;
  c->kp_capacity = 0;
  c->stages = FVO_STAGE_ALL;
  c->ba_window = 10;
  c->ba_max_landmarks = 4096;
  c->ba_max_obs = 32768;
  c->sgbm_max_batch = 0;
  c->sgbm_mode = FVO_SGBM_CLASSIC;
  c->sgbm_lanes = 0;
  c->sgbm_cols = 0;
  c->sgbm_handoff_us = 0;
}

static void release(fvo_ctx* c) {
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->ba_s2) (void)hipStreamDestroy(c->ba_s2);
  if (c->ba_fork) (void)hipEventDestroy(c->ba_fork);
  if (c->ba_join) (void)hipEventDestroy(c->ba_join);
}

// ---- config checks, one per stage, in the order fvo_create runs the stage inits
static int check_orb_config(fvo_ctx* ctx) {
  const fvo_config& c = ctx->cfg;
  if (c.nlevels < 1 || c.nlevels > FVO_MAX_LEVELS) return fvo_fail(ctx, "nlevels out of range");
  if (c.first_level != 0 || c.wta_k != 2 || c.score_type != 0 || c.patch_size != 31)
    return fvo_fail(ctx, "only firstLevel=0, WTA_K=2, HARRIS_SCORE, patchSize=31 are supported");
  if (c.width > 4095 || c.height > 4095) return fvo_fail(ctx, "image dimensions must be < 4096");
  // k_angle reads the whole 31x31 square around a keypoint unguarded; keypoints are kept
  // edgeThreshold px inside the level, so it must cover the half patch (k_brief stages its
  // rotated patch with REFLECT_101 and needs no such bound)
  if (c.edge_threshold < c.patch_size / 2) return fvo_fail(ctx, "edgeThreshold must be >= patchSize/2 (15)");
  return 0;
}

static int check_bf_config(fvo_ctx* ctx) {
  if (ctx->kp_cap > 0xFFFF) return fvo_fail(ctx, "BF: kp_capacity must be <= 65535 (16-bit indices in the keys)");
  return 0;
}

static int check_sgbm_config(fvo_ctx* ctx) {
  const fvo_config& c = ctx->cfg;
  if (c.block_size != 7) return fvo_fail(ctx, "SGBM: only blockSize=7 is supported");
  if (c.num_disparities != 64 && c.num_disparities != 96 && c.num_disparities != 128)
    return fvo_fail(ctx, "SGBM: numDisparities must be 64, 96 or 128");
  if (c.uniqueness_ratio != 0) return fvo_fail(ctx, "SGBM: only uniquenessRatio=0 is supported");
  if (c.sgbm_stripes < 1) return fvo_fail(ctx, "SGBM: stripes must be >= 1");
  if (c.sgbm_mode != FVO_SGBM_CLASSIC && c.sgbm_mode != FVO_SGBM_LPATH)
    return fvo_fail(ctx, "SGBM: sgbm_mode must be FVO_SGBM_CLASSIC or FVO_SGBM_LPATH");
  if (c.sgbm_mode == FVO_SGBM_CLASSIC) {
    const int g = sg_lanes(c), cb = sg_cols(c);
    if (!((g == 4 && (cb == 32 || cb == 64)) || (g == 8 && (cb == 16 || cb == 32)) || (g == 16 && cb == 32)))
      return fvo_fail(ctx, "SGBM: (sgbm_lanes, sgbm_cols) must be (4, 32|64), (8, 16|32) or (16, 32)");
  } else if (c.sgbm_lanes != 0 || c.sgbm_cols != 0) {
    return fvo_fail(ctx, "SGBM: sgbm_lanes / sgbm_cols apply to the classic schedule only (leave them 0)");
  }
  if (c.sgbm_handoff_us < -1) return fvo_fail(ctx, "SGBM: sgbm_handoff_us must be >= -1");
  const SgParams p = make_params(c);
  if (p.width1 <= 0) return fvo_fail(ctx, "SGBM: image narrower than numDisparities");
  // path values are at most C + P2 with C <= 49 x the largest BT pixel cost (2 ftzero + 255/4);
  // the kernels add P1 to them in u16 (min(a, b) + P1 for min(a + P1, b + P1)), so that sum
  // must not wrap -- OpenCV's 16-bit CostType carries the same assumption
  if (49 * (2 * p.ftzero + 63) + p.P2 + p.P1 > 0xFFFF)
    return fvo_fail(ctx, "SGBM: P1/P2/preFilterCap too large for 16-bit path costs");
  // the row pass sums S = L + R + V in u16 lanes and its WTA keys on S: each path is at most
  // C + P2, so 3 (C + P2) must not wrap either
  if (3 * (49 * (2 * p.ftzero + 63) + p.P2) > 0xFFFF)
    return fvo_fail(ctx, "SGBM: P2/preFilterCap too large for the 16-bit aggregated cost");
  // the L path's hand-off tags carry the column block in 7 bits
  if (c.sgbm_mode == FVO_SGBM_LPATH && sg_nk(p) >= 128)
    return fvo_fail(ctx, "SGBM: FVO_SGBM_LPATH needs width - numDisparities <= 4064 (use the classic schedule)");
  return 0;
}

static int check_ba_config(fvo_ctx* ctx) {
  const fvo_config& c = ctx->cfg;
  if (c.ba_window < 3 || c.ba_window > kBaMaxWindow) return fvo_fail(ctx, "ba_window must be in [3, 21]");
  if (c.ba_max_landmarks < 1 || c.ba_max_obs < 2) return fvo_fail(ctx, "bad BA landmark / observation caps");
  return 0;
}

int fvo_create(int device, const fvo_config* cfg, fvo_ctx** out) {
  if (!cfg || !out) return -1;
  *out = nullptr;
  fvo_ctx* c = new fvo_ctx();
  c->device = device;
  c->cfg = *cfg;
  auto bail = [&](int rc) {
    std::fprintf(stderr, "fvo_create: %s\n", c->err.c_str());
    release(c);
    delete c;
    return rc;
  };
  if (hipSetDevice(device) != hipSuccess) { c->err = "hipSetDevice failed"; return bail(-1); }
  if (c->cfg.stages == 0) c->cfg.stages = FVO_STAGE_ALL;
  const int st = c->cfg.stages;
  if (st & ~FVO_STAGE_ALL) { c->err = "unknown bits in stages"; return bail(-1); }
  if (cfg->max_batch < 1) { c->err = "max_batch must be >= 1"; return bail(-1); }
  if ((st & FVO_STAGE_ORB) && (cfg->width < 64 || cfg->height < 64)) {
    c->err = "image size must be at least 64x64";
    return bail(-1);
  }
  // SGBM alone: its kernels clamp rows to the stripe and to the image and have no use for a tall
  // image (OpenCV takes any size); 32 rows is the smallest height the parity tests run
  if ((st & FVO_STAGE_SGBM) && (cfg->width < 64 || cfg->height < 32)) {
    c->err = "image size must be at least 64x32 for SGBM (64x64 with ORB)";
    return bail(-1);
  }
  if (!(st & FVO_STAGE_ORB) && (st & (FVO_STAGE_BF | FVO_STAGE_POSE | FVO_STAGE_BA | FVO_STAGE_MONO)) &&
      cfg->kp_capacity < 1) {
    c->err = "kp_capacity must be set when the ORB stage is not enabled";
    return bail(-1);
  }
  c->kp_cap = cfg->kp_capacity > 0 ? cfg->kp_capacity : 2 * cfg->nfeatures + 64;
  // (the POSE and MONO stages have no config of their own to check)
  if (((st & FVO_STAGE_ORB) && check_orb_config(c)) || ((st & FVO_STAGE_BF) && check_bf_config(c)) ||
      ((st & FVO_STAGE_SGBM) && check_sgbm_config(c)) || ((st & FVO_STAGE_BA) && check_ba_config(c)))
    return bail(-1);
  int rc = 0;
  if (((st & FVO_STAGE_ORB) && (rc = orb_init(c))) || ((st & FVO_STAGE_BF) && (rc = bf_init(c))) ||
      ((st & FVO_STAGE_SGBM) && (rc = sgbm_init(c))) || ((st & FVO_STAGE_POSE) && (rc = pose_init(c))) ||
      ((st & FVO_STAGE_BA) && (rc = ba_init(c))) || ((st & FVO_STAGE_MONO) && (rc = mono_init(c))))
    return bail(rc);
  *out = c;
  return 0;
}

void fvo_destroy(fvo_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (auto& r : c->trecs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : c->tpool) (void)hipEventDestroy(e);
  release(c);
  delete c;
}

const char* fvo_last_error(const fvo_ctx* c) { return c ? c->err.c_str() : "null context"; }
int fvo_kp_capacity(const fvo_ctx* c) { return c ? c->kp_cap : 0; }
int64_t fvo_workspace_bytes(const fvo_ctx* c) { return c ? c->ws_bytes : 0; }

static int check_batch(fvo_ctx* c, int32_t batch, int stage) {
  if (!c) return -1;
  if (!(c->cfg.stages & stage)) return fvo_fail(c, "stage not enabled in this context (fvo_config.stages)");
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  return 0;
}

int fvo_orb_detect_compute(fvo_ctx* c, const uint8_t* images, int32_t batch, int64_t image_stride, int32_t pitch,
                           float* keypoints, uint8_t* descriptors, int32_t* counts, int32_t cap, fvo_stream stream) {
  if (check_batch(c, batch, FVO_STAGE_ORB)) return -1;
  if (batch == 0) return 0;
  if (!images || !keypoints || !descriptors || !counts) return fvo_fail(c, "null pointer argument");
  if (pitch < c->cfg.width || image_stride < (int64_t)pitch * c->cfg.height) return fvo_fail(c, "bad pitch/stride");
  if (cap < 1) return fvo_fail(c, "cap must be >= 1");
  return orb_run(c, images, batch, image_stride, pitch, keypoints, descriptors, counts, cap, (hipStream_t)stream);
}

int fvo_bf_match(fvo_ctx* c, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                 const int32_t* n_train, int32_t batch, int32_t cap, int32_t* matches, int32_t* n_matches,
                 fvo_stream stream) {
  if (check_batch(c, batch, FVO_STAGE_BF)) return -1;
  if (batch == 0) return 0;
  if (!query || !n_query || !train || !n_train || !matches || !n_matches) return fvo_fail(c, "null pointer argument");
  if (cap < 1 || cap > c->kp_cap) return fvo_fail(c, "cap must be in [1, fvo_kp_capacity()]");
  if ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(train)) & 15)
    return fvo_fail(c, "descriptor buffers must be 16-byte aligned");
  return bf_run(c, query, n_query, train, n_train, batch, cap, matches, n_matches, (hipStream_t)stream);
}

// The checks fvo_bf_knn_match and fvo_bf_ratio_match share; 1 = nothing to do (batch == 0), < 0 = refused.
static int bf_check(fvo_ctx* c, const void* query, const void* n_query, const void* train, const void* n_train,
                    int32_t batch, int32_t cap) {
  if (check_batch(c, batch, FVO_STAGE_BF)) return -1;
  if (batch == 0) return 1;
  if (!query || !n_query || !train || !n_train) return fvo_fail(c, "null pointer argument");
  if (cap < 1 || cap > c->kp_cap) return fvo_fail(c, "cap must be in [1, fvo_kp_capacity()]");
  if ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(train)) & 15)
    return fvo_fail(c, "descriptor buffers must be 16-byte aligned");
  return 0;
}

int fvo_bf_knn_match(fvo_ctx* c, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                     const int32_t* n_train, int32_t batch, int32_t cap, int32_t k, int32_t* knn, fvo_stream stream) {
  const int rc = bf_check(c, query, n_query, train, n_train, batch, cap);
  if (rc) return rc < 0 ? rc : 0;
  if (k < 1 || k > FVO_BF_MAX_K) return fvo_fail(c, "bf_knn_match: k must be in [1, 8]");
  if (!knn) return fvo_fail(c, "null pointer argument");
  return bf_knn_run(c, query, n_query, train, n_train, batch, cap, k, knn, (hipStream_t)stream);
}

int fvo_bf_ratio_match(fvo_ctx* c, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                       const int32_t* n_train, int32_t batch, int32_t cap, double ratio, int32_t mutual,
                       int32_t* matches, int32_t* n_matches, fvo_stream stream) {
  const int rc = bf_check(c, query, n_query, train, n_train, batch, cap);
  if (rc) return rc < 0 ? rc : 0;
  if (!matches || !n_matches) return fvo_fail(c, "null pointer argument");
  if (!std::isfinite(ratio) || ratio <= 0.0) return fvo_fail(c, "bf_ratio_match: ratio must be finite and > 0");
  return bf_ratio_run(c, query, n_query, train, n_train, batch, cap, ratio, mutual != 0, matches, n_matches,
                      (hipStream_t)stream);
}

int fvo_sgbm(fvo_ctx* c, const uint8_t* left, const uint8_t* right, int32_t batch, int64_t image_stride,
             int32_t pitch, int16_t* disparity, int32_t* status, fvo_stream stream) {
  if (check_batch(c, batch, FVO_STAGE_SGBM)) return -1;
  if (batch == 0) return 0;
  if (!left || !right || !disparity) return fvo_fail(c, "null pointer argument");
  if (pitch < c->cfg.width || image_stride < (int64_t)pitch * c->cfg.height) return fvo_fail(c, "bad pitch/stride");
  if (batch > (c->cfg.sgbm_max_batch > 0 ? c->cfg.sgbm_max_batch : c->cfg.max_batch))
    return fvo_fail(c, "batch exceeds sgbm_max_batch");
  return sgbm_run(c, left, right, batch, image_stride, pitch, disparity, status, (hipStream_t)stream);
}

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

int fvo_backproject(fvo_ctx* c, const int16_t* disparity, const float* kp0, const float* kp1, const int32_t* matches,
                    const int32_t* n_matches, int32_t batch, int32_t cap, const double* K, double baseline,
                    float* points3d, float* points2d, int32_t* n_points, fvo_stream stream) {
  if (check_batch(c, batch, FVO_STAGE_POSE)) return -1;
  if (batch == 0) return 0;
  if (!disparity || !kp0 || !kp1 || !matches || !n_matches || !K || !points3d || !points2d || !n_points)
    return fvo_fail(c, "null pointer argument");
  if (cap < 1) return fvo_fail(c, "cap must be >= 1");
  return backproject_run(c, disparity, kp0, kp1, matches, n_matches, batch, cap, K, baseline, points3d, points2d,
                         n_points, (hipStream_t)stream);
}

int fvo_pnp_ransac(fvo_ctx* c, const float* points3d, const float* points2d, const int32_t* n_points, int32_t batch,
                   int32_t cap, const double* K, const double* dist, float reprojection_error, double confidence,
                   int32_t iterations, double* rvec, double* tvec, double* T, int32_t* status, uint8_t* inliers,
                   fvo_stream stream) {
  if (check_batch(c, batch, FVO_STAGE_POSE)) return -1;
  if (batch == 0) return 0;
  if (!points3d || !points2d || !n_points || !K || !dist || !rvec || !tvec || !T || !status)
    return fvo_fail(c, "null pointer argument");
  if (cap < 1) return fvo_fail(c, "cap must be >= 1");
  if (iterations < 1 || iterations > kRansacMaxIters) return fvo_fail(c, "iterations out of range");
  if (!(confidence > 0 && confidence < 1)) return fvo_fail(c, "confidence must be in (0,1)");
  if (cap > c->kp_cap) return fvo_fail(c, "pnp: cap exceeds the context keypoint capacity");
  return pnp_run(c, points3d, points2d, n_points, batch, cap, K, dist, reprojection_error, confidence, iterations,
                 rvec, tvec, T, status, inliers, (hipStream_t)stream);
}

int fvo_keypoint_stereo(fvo_ctx* c, const int16_t* disparity, const float* keypoints, const int32_t* n_keypoints,
                        int32_t batch, int32_t cap, const double* K, double baseline, float* stereo,
                        fvo_stream stream) {
  if (check_batch(c, batch, FVO_STAGE_BA)) return -1;
  if (batch == 0) return 0;
  if (!disparity || !keypoints || !n_keypoints || !K || !stereo) return fvo_fail(c, "null pointer argument");
  if (cap < 1 || cap > c->kp_cap) return fvo_fail(c, "cap must be in [1, fvo_kp_capacity()]");
  if (reinterpret_cast<uintptr_t>(stereo) & 15) return fvo_fail(c, "stereo buffer must be 16-byte aligned");
  return ba_stereo_run(c, disparity, keypoints, n_keypoints, batch, cap, K, baseline, stereo, (hipStream_t)stream);
}

// The window range fvo_ba_windows and fvo_ba_count_births share (n_windows <= max_batch: check_batch).
static int check_ba_range(fvo_ctx* c, int32_t n_frames, int32_t cap, int32_t first_end, int32_t n_windows,
                          int32_t first_valid) {
  if (cap != c->kp_cap) return fvo_fail(c, "ba: cap must equal the context keypoint capacity");
  if (first_end < 1 || first_end + n_windows > n_frames) return fvo_fail(c, "ba: windows exceed the frame range");
  if (first_valid < 0 || first_valid >= first_end) return fvo_fail(c, "ba: first_valid out of range");
  return 0;
}

int fvo_ba_windows(fvo_ctx* c, const float* keypoints, const int32_t* n_keypoints, const int32_t* matches,
                   const int32_t* n_matches, const float* stereo, const double* T_rel, int32_t n_frames,
                   int32_t cap, int32_t first_end, int32_t n_windows, int32_t first_valid, const double* K,
                   double baseline, const double* inv_sigma2, int32_t n_levels, int32_t iterations,
                   double* T_out, double* stats, fvo_stream stream) {
  if (check_batch(c, n_windows, FVO_STAGE_BA)) return -1;
  if (n_windows == 0) return 0;
  if (!keypoints || !n_keypoints || !matches || !n_matches || !stereo || !T_rel || !K || !inv_sigma2 || !T_out ||
      !stats)
    return fvo_fail(c, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(stereo) & 15) return fvo_fail(c, "stereo buffer must be 16-byte aligned");
  if (check_ba_range(c, n_frames, cap, first_end, n_windows, first_valid)) return -1;
  if (n_levels < 1 || n_levels > FVO_MAX_LEVELS) return fvo_fail(c, "ba: bad level count");
  if (iterations < 0 || iterations > 100) return fvo_fail(c, "ba: iterations out of range");
  return ba_run(c, keypoints, n_keypoints, matches, n_matches, stereo, T_rel, n_frames, cap, first_end, n_windows,
                first_valid, K, baseline, inv_sigma2, n_levels, iterations, T_out, stats, (hipStream_t)stream);
}

int fvo_ba_count_births(fvo_ctx* c, const int32_t* matches, const int32_t* n_matches, const float* stereo,
                        int32_t n_frames, int32_t cap, int32_t first_end, int32_t n_windows, int32_t first_valid,
                        fvo_stream stream) {
  if (check_batch(c, n_windows, FVO_STAGE_BA)) return -1;
  c->ba_births.valid = false;
  if (n_windows == 0) return 0;
  if (!matches || !n_matches || !stereo) return fvo_fail(c, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(stereo) & 15) return fvo_fail(c, "stereo buffer must be 16-byte aligned");
  if (check_ba_range(c, n_frames, cap, first_end, n_windows, first_valid)) return -1;
  return ba_births_run(c, matches, n_matches, stereo, n_frames, cap, first_end, n_windows, first_valid,
                       (hipStream_t)stream);
}

int fvo_ba_landmarks(fvo_ctx* c, int32_t window, double* xyz, int32_t* count, fvo_stream stream) {
  if (check_batch(c, 1, FVO_STAGE_BA)) return -1;
  if (!xyz || !count) return fvo_fail(c, "null pointer argument");
  if (window < 0 || window >= c->cfg.max_batch) return fvo_fail(c, "ba: window index out of range");
  return ba_export_run(c, window, xyz, count, (hipStream_t)stream);
}

int fvo_gather_matches(fvo_ctx* c, const float* kp0, const float* kp1, const int32_t* matches,
                       const int32_t* n_matches, int32_t batch, int32_t cap, float* p0, float* p1, int32_t* n_points,
                       fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 0;
  if (!kp0 || !kp1 || !matches || !n_matches || !p0 || !p1 || !n_points) return fvo_fail(c, "null pointer argument");
  if (cap < 1) return fvo_fail(c, "cap must be >= 1");
  return gather_run(c, kp0, kp1, matches, n_matches, batch, cap, p0, p1, n_points, (hipStream_t)stream);
}

int fvo_find_essential(fvo_ctx* c, const float* p0, const float* p1, const int32_t* n_points, int32_t batch,
                       int32_t cap, double focal, double cx, double cy, double prob, double threshold,
                       int32_t max_iters, double* E, uint8_t* mask, int32_t* status, fvo_stream stream) {
  if (check_batch(c, batch, FVO_STAGE_MONO)) return -1;
  if (batch == 0) return 0;
  if (!p0 || !p1 || !n_points || !E || !status) return fvo_fail(c, "null pointer argument");
  if (cap < 1 || cap > c->kp_cap) return fvo_fail(c, "cap must be in [1, fvo_kp_capacity()]");
  if (!(focal > 0.0)) return fvo_fail(c, "focal must be > 0");
  if (max_iters < 1 || max_iters > kRansacMaxIters) return fvo_fail(c, "essential: max_iters out of range");
  // k_em_hyp stages a frame's normalised points in LDS
  if (cap > kEmMaxCap) return fvo_fail(c, "essential: point capacity exceeds LDS (cap <= 5040)");
  return essential_run(c, p0, p1, n_points, batch, cap, focal, cx, cy, prob, threshold, max_iters, E, mask, status,
                       (hipStream_t)stream);
}

int fvo_recover_pose(fvo_ctx* c, const double* E, const int32_t* e_status, const float* p0, const float* p1,
                     const int32_t* n_points, int32_t batch, int32_t cap, double focal, double cx, double cy,
                     double distance_thresh, double* R, double* t, double* T, int32_t* n_good, fvo_stream stream) {
  if (check_batch(c, batch, FVO_STAGE_MONO)) return -1;
  if (batch == 0) return 0;
  if (!E || !p0 || !p1 || !n_points || !R || !t || !T || !n_good) return fvo_fail(c, "null pointer argument");
  if (cap < 1 || cap > c->kp_cap) return fvo_fail(c, "cap must be in [1, fvo_kp_capacity()]");
  if (!(focal > 0.0)) return fvo_fail(c, "focal must be > 0");
  return recover_run(c, E, e_status, p0, p1, n_points, batch, cap, focal, cx, cy, distance_thresh, R, t, T, n_good,
                     (hipStream_t)stream);
}

int fvo_undistort_gray(fvo_ctx* c, const uint8_t* bgr, int32_t batch, int64_t src_stride, int32_t src_pitch,
                       const double* K, const double* dist, uint8_t* gray, int64_t dst_stride, int32_t dst_pitch,
                       fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 0;
  if (!bgr || !K || !dist || !gray) return fvo_fail(c, "null pointer argument");
  const int W = c->cfg.width, H = c->cfg.height;
  if (src_pitch < 3 * W || src_stride < (int64_t)src_pitch * H || dst_pitch < W || dst_stride < (int64_t)dst_pitch * H)
    return fvo_fail(c, "bad pitch/stride");
  // fvo_rectify_map's calibration rule for every stripe of cv2.undistort: the kernel inverts K with
  // cy moved to the stripe's first row and divides by _w = (i*ir[7] + ir[8]) + col*ir[6], i the
  // row inside the stripe.  _w is affine in (i, col): the stripe's four corners bound it.
  if (!host_all_finite(K, 9) || !host_all_finite(dist, 5))
    return fvo_fail(c, "undistort_gray: K and dist must be finite");
  const int stripe0 = ingest_stripe_rows(W, H);
  for (int y0 = 0; y0 < H; y0 += stripe0) {
    double A[9], ir[9];
    std::memcpy(A, K, sizeof(A));
    A[5] = K[5] - y0;
    if (!host_inv3(A, ir)) return fvo_fail(c, "undistort_gray: K is singular (a stripe's camera matrix has det == 0)");
    const int rows = H - y0 < stripe0 ? H - y0 : stripe0;
    for (int k = 0; k < 4; ++k) {
      const int i = (k >> 1) ? rows - 1 : 0, col = (k & 1) ? W - 1 : 0;
      if (!host_ray_w_ok((i * ir[7] + ir[8]) + col * ir[6]))
        return fvo_fail(c, "undistort_gray: _w <= 0 at a stripe corner (the view reaches the camera's horizon)");
    }
  }
  return ingest_run(c, bgr, batch, src_stride, src_pitch, K, dist, gray, dst_stride, dst_pitch, (hipStream_t)stream);
}

int fvo_motion_blur(fvo_ctx* c, const uint8_t* img, int32_t batch, int64_t src_stride, int32_t src_pitch,
                    int32_t ksize, double angle, const int32_t* centers, const int32_t* n_centers, int32_t centers_cap,
                    uint8_t* mask, uint8_t* out, int64_t dst_stride, int32_t dst_pitch, fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 0;
  if (!img || !mask || !out || (centers_cap > 0 && (!centers || !n_centers))) return fvo_fail(c, "null pointer argument");
  if (angle != 0.0) return fvo_fail(c, "motion blur: only angle 0 is supported (the reference's value)");
  const int W = c->cfg.width, H = c->cfg.height;
  if (ksize < 1 || ksize > 31) return fvo_fail(c, "motion blur: ksize must be in [1, 31]");
  if (W <= ksize || H <= ksize) return fvo_fail(c, "motion blur: image smaller than the kernel");
  if (centers_cap < 0) return fvo_fail(c, "centers_cap < 0");
  if (src_pitch < W || src_stride < (int64_t)src_pitch * H || dst_pitch < W || dst_stride < (int64_t)dst_pitch * H)
    return fvo_fail(c, "bad pitch/stride");
  if (img == out) return fvo_fail(c, "motion blur: out must not alias img");
  // k_mb_fix rewrites the mask a dword at a time: refuse a misaligned mask before any launch,
  // so an error never leaves the mask in its intermediate (seed / dilated bit) encoding
  if (centers_cap > 0 && (reinterpret_cast<uintptr_t>(mask) & 3))
    return fvo_fail(c, "motion blur: mask must be 4-byte aligned");
  return motion_blur_run(c, img, batch, src_stride, src_pitch, ksize, centers, n_centers, centers_cap, mask, out,
                         dst_stride, dst_pitch, (hipStream_t)stream);
}

int fvo_map_transform(fvo_ctx* c, const float* points, int32_t point_stride, const int32_t* n_points, int32_t batch,
                      int64_t cap, const double* T, int32_t* map_count, int64_t map_cap, double* map_xyz64,
                      float* map_xyz32, fvo_stream stream) {
  if (!c) return -1;
  if (batch < 0) return fvo_fail(c, "batch < 0");
  if (batch == 0) return 0;
  if (!points || !n_points || !T || !map_count || (!map_xyz64 && !map_xyz32)) return fvo_fail(c, "null pointer argument");
  if (point_stride < 3) return fvo_fail(c, "point_stride must be >= 3 floats");
  if (cap < 1 || cap > (int64_t)1 << 31) return fvo_fail(c, "cap must be in [1, 2^31]");
  if (map_cap < 0) return fvo_fail(c, "map_cap < 0");
  return map_transform_run(c, points, point_stride, n_points, batch, cap, T, map_count, map_cap, map_xyz64, map_xyz32,
                           (hipStream_t)stream);
}

int fvo_chain_poses(fvo_ctx* c, const double* T, const int32_t* status, const int32_t* n_points, int32_t n_seq,
                    int32_t n, double* cum_state, double* cum_out, int32_t* n_points_out, fvo_stream stream) {
  if (!c) return -1;
  if (n_seq < 0 || n < 0) return fvo_fail(c, "n_seq and n must be >= 0");
  if (n_seq == 0 || n == 0) return 0;
  if (!T || !status || !cum_state || !cum_out) return fvo_fail(c, "null pointer argument");
  if ((n_points == nullptr) != (n_points_out == nullptr)) return fvo_fail(c, "n_points and n_points_out: both or neither");
  return chain_poses_run(c, T, status, n_points, n_seq, n, cum_state, cum_out, n_points_out, (hipStream_t)stream);
}

int fvo_copy_regions(fvo_ctx* c, int32_t count, const fvo_region* regions, fvo_stream stream) {
  if (!c) return -1;
  if (count < 0 || count > FVO_MAX_REGIONS) return fvo_fail(c, "copy_regions: count out of [0, FVO_MAX_REGIONS]");
  if (count == 0) return 0;
  if (!regions) return fvo_fail(c, "null pointer argument");
  int used = 0;
  fvo_region live[FVO_MAX_REGIONS];
  for (int i = 0; i < count; ++i) {
    const fvo_region& g = regions[i];
    if (g.bytes < 0) return fvo_fail(c, "copy_regions: bytes < 0");
    if (g.bytes == 0) continue;
    if (!g.dst || !g.src) return fvo_fail(c, "copy_regions: null region pointer");
    live[used++] = g;
  }
  auto overlap = [](const void* a, const void* b, int64_t na, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
  };
  for (int i = 0; i < used; ++i)
    for (int j = 0; j < used; ++j) {
      if (overlap(live[i].dst, live[j].src, live[i].bytes, live[j].bytes) ||
          (i != j && overlap(live[i].dst, live[j].dst, live[i].bytes, live[j].bytes)))
        return fvo_fail(c, "copy_regions: a destination overlaps a source or another destination");
    }
  if (used == 0) return 0;
  return copy_regions_run(c, used, live, (hipStream_t)stream);
}

int fvo_count_guard(fvo_ctx* c, const int32_t* counts, const int32_t* q_counts, int32_t n, int32_t sets,
                    int32_t* status, int32_t code, int32_t* counts_clamped, fvo_stream stream) {
  if (!c) return -1;
  if (n < 0 || sets < 1 || sets > 8) return fvo_fail(c, "count_guard: n < 0 or sets outside [1, 8]");
  if (n == 0) return 0;
  if (!counts) return fvo_fail(c, "null pointer argument");
  return count_guard_run(c, counts, q_counts, n, sets, status, code, counts_clamped, (hipStream_t)stream);
}

int64_t fvo_voxel_workspace_bytes(int64_t n_points) {
  if (n_points < 1 || n_points > INT32_MAX) return -1;
  return voxel_workspace_bytes(n_points);
}

int fvo_voxel_down_sample(fvo_ctx* c, const double* points, int64_t n_points, double voxel_size, void* workspace,
                          int64_t workspace_bytes, double* out, int32_t* n_out, int32_t* status, fvo_stream stream) {
  if (!c) return -1;
  if (!out || !n_out || (n_points > 0 && (!points || !workspace))) return fvo_fail(c, "null pointer argument");
  if (!(voxel_size > 0.0)) return fvo_fail(c, "voxel_size must be > 0");
  if (n_points < 0 || n_points > INT32_MAX) return fvo_fail(c, "n_points out of range");
  if (n_points == 0) {  // Open3D: an empty cloud downsamples to an empty cloud
    FVO_HIP(c, hipMemsetAsync(n_out, 0, 4, (hipStream_t)stream));
    if (status) FVO_HIP(c, hipMemsetAsync(status, 0, 4, (hipStream_t)stream));
    return 0;
  }
  if (workspace_bytes < 0) return fvo_fail(c, "workspace_bytes < 0");
  const int64_t need = voxel_workspace_bytes(n_points);  // voxel_run's layout total
  if (need < 0) return fvo_fail(c, "voxel_down_sample: workspace size query failed");
  if (workspace_bytes < need) return fvo_fail(c, "voxel_down_sample: workspace too small");
  return voxel_run(c, points, n_points, voxel_size, workspace, out, n_out, status, (hipStream_t)stream);
}

// Dense mapping: blocks of all frames, or -1 when the size is refused.
static int64_t dense_blocks(int32_t batch, int32_t height, int32_t width, int32_t step) {
  if (batch < 0 || height < 1 || width < 1 || step < 1) return -1;
  if ((int64_t)height * width > INT32_MAX) return -1;  // flat sample indices are 32-bit
  const int64_t n = dense_frame_blocks(height, width, step) * batch;
  return n > INT32_MAX ? -1 : n;  // one launch block each
}

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

int fvo_kernel_count(void) { return KN_COUNT; }

const char* fvo_kernel_name(int id) {
#define FVO_KERNEL_NAME(id, name) name,
  static const char* names[KN_COUNT] = {FVO_KERNELS(FVO_KERNEL_NAME)};
#undef FVO_KERNEL_NAME
  return (id >= 0 && id < KN_COUNT) ? names[id] : "";
}

int fvo_timing_enable(fvo_ctx* c, uint64_t mask) {
  if (!c) return -1;
  c->tmask = mask;
  return 0;
}

int fvo_timing_read(fvo_ctx* c, double* ms, int32_t* launches) {
  if (!c || !ms || !launches) return -1;
  for (int i = 0; i < KN_COUNT; ++i) { ms[i] = 0.0; launches[i] = 0; }
  for (auto& r : c->trecs) {
    FVO_HIP(c, hipEventSynchronize(r.b));
    float t = 0.f;
    FVO_HIP(c, hipEventElapsedTime(&t, r.a, r.b));
    ms[r.id] += t;
    launches[r.id] += 1;
    c->tpool.push_back(r.a);
    c->tpool.push_back(r.b);
  }
  c->trecs.clear();
  return 0;
}

// Debug/test hook: device pointer + size of an internal workspace buffer of the last call.
// which: 0 pyramid, 1 blurred pyramid, 2 FAST score map (all [max_batch][total_px] u8),
//        3 per-level candidate counts, 4 after retainBest(2n), 5 after retainBest(n) (i32 [B][L]),
//        6 PnP RANSAC inlier count per iteration (i32 [B][1000]), 7 PnP hypotheses (f64 [B][1000][6]),
//        8 PnP RANSAC state (i32 [B][4]: best inlier count, iteration bound, best iteration, points),
//        9 SGBM control words, 10 no buffer (0 bytes): ORB orientation as a separate pass from now on,
//        11 SGBM raw disparity (before the median) of the last call's last chunk of pairs.
int fvo_debug_buffer(fvo_ctx* c, int which, void** ptr, int64_t* bytes) {
  if (!c || !ptr || !bytes) return -1;
  const int64_t B = c->cfg.max_batch;
  switch (which) {
    case 0: *ptr = c->pyr; *bytes = B * c->g.total_px; return 0;
    case 1:  // computed on request from the last call's pyramid (not part of the hot path)
      if (!c->pyr) return fvo_fail(c, "orb stage not enabled");
      if (orb_blur_debug(c)) return -1;
      *ptr = c->blur; *bytes = B * c->g.total_px; return 0;
    case 2:  // computed on request from the last call's pyramid (not part of the hot path)
      if (!c->pyr) return fvo_fail(c, "orb stage not enabled");
      if (orb_score_debug(c)) return -1;
      *ptr = c->score; *bytes = B * c->g.total_px; return 0;
    case 3: *ptr = c->ncand; *bytes = B * c->g.nlevels * 4; return 0;
    case 4: *ptr = c->nsel1; *bytes = B * c->g.nlevels * 4; return 0;
    case 5: *ptr = c->nsel2; *bytes = B * c->g.nlevels * 4; return 0;
    case 6: *ptr = c->pnp_good; *bytes = B * c->pnp_max_iters * 4; return 0;
    case 7: *ptr = c->pnp_models; *bytes = B * c->pnp_max_iters * 6 * 8; return 0;
    case 8: *ptr = c->pnp_state; *bytes = B * 16; return 0;
    case 9:  // SGBM control words: ticket, generation, hand-off timeouts, per-pair failure flags
      if (!c->sg_ctl) return fvo_fail(c, "no SGBM workspace");
      *ptr = c->sg_ctl; *bytes = (4 + B) * 4; return 0;
    case 10:  // no buffer: a switch, so that tests and tools/bench_orb.py can run the ORB path that
              // no accepted configuration selects (orb_init) -- from the next call on this context
              // forms the orientation in a pass of its own (k_angle) instead of inside k_brief
      if (!c->pyr) return fvo_fail(c, "orb stage not enabled");
      c->g.angle_pass = true;
      *ptr = nullptr; *bytes = 0; return 0;
    case 11: {  // SGBM's disparity before the median, i16 [sgbm batch][H][W] (sgbm_init's allocation)
      if (!c->sg_raw) return fvo_fail(c, "no SGBM workspace");
      const int64_t sb = c->cfg.sgbm_max_batch > 0 ? std::min<int64_t>(c->cfg.sgbm_max_batch, B) : B;
      *ptr = c->sg_raw; *bytes = sb * c->cfg.height * c->cfg.width * 2; return 0;
    }
    default: return fvo_fail(c, "unknown debug buffer");
  }
}

int fvo_debug_copy(fvo_ctx* c, int which, void* host_dst, int64_t bytes) {
  void* src = nullptr;
  int64_t have = 0;
  if (fvo_debug_buffer(c, which, &src, &have)) return -1;
  if (!host_dst) return fvo_fail(c, "null pointer argument");
  if (bytes < 0 || bytes > have) return fvo_fail(c, "debug_copy: bytes outside [0, the buffer's size]");
  FVO_HIP(c, hipSetDevice(c->device));
  FVO_HIP(c, hipDeviceSynchronize());
  FVO_HIP(c, hipMemcpy(host_dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
  return 0;
}

int fvo_test_retain_best(fvo_ctx* c, const float* keys, int32_t n, int32_t keep, int32_t* idx_out, int32_t* n_out,
                         fvo_stream stream) {
  return orb_retain_best_run(c, keys, n, keep, idx_out, n_out, (hipStream_t)stream);
}

}  // extern "C"
