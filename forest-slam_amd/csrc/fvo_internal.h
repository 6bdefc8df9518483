// Internal declarations shared by the HIP translation units of libfvo.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fvo.h"

#define FVO_MAX_LEVELS 12

// Pyramid geometry computed on the host exactly as OpenCV's ORB does
// (orb.cpp detectAndCompute: getScale, cvRound(cols * (1.f/scale))).
struct OrbGeom {
  int nlevels;
  int w[FVO_MAX_LEVELS], h[FVO_MAX_LEVELS];
  float scale[FVO_MAX_LEVELS];         // layerScale
  int64_t off[FVO_MAX_LEVELS + 1];      // plane offsets inside one image's pyramid
  int row0[FVO_MAX_LEVELS + 1];         // first global row of each level
  int nfeat[FVO_MAX_LEVELS];            // nfeaturesPerLevel
  int64_t cand_off[FVO_MAX_LEVELS + 1]; // candidate-array offsets per level (per image)
  int64_t total_px;
  int total_rows;
  int64_t cand_total;
  bool angle_pass;                      // orientation as a pass of its own (k_angle), not inside k_brief
};

// Constant tables for the INTER_LINEAR_EXACT pyramid resize (per level, per axis).
struct ResizeTab {
  int32_t* xofs;  // per level l>=1: w[l] entries: source index, -1 left clamp, -2 right clamp
  int32_t* xc1;   // ufixedpoint16 weight of ofs+1 (weight of ofs is 256 - c1)
  int32_t* yofs;
  int32_t* yc1;
  int64_t xoff[FVO_MAX_LEVELS], yoff[FVO_MAX_LEVELS];
};

// Limits that capi.cpp checks and a device file depends on (the device file static_asserts them).
constexpr int kBaMaxWindow = 21;        // ba.hip kKMax: frames of a BA window
constexpr int kEmMaxCap = 5040;         // essential.hip: points of one frame that fit k_em_hyp's LDS
constexpr int kRansacMaxIters = 1000;   // pose.hip / essential.hip: hypothesis buffers, the subset table

// Kernel ids for the optional per-launch event timing (fvo_timing_enable / _read) and their names
// (fvo_kernel_name), in id order.
#define FVO_KERNELS(X)                                                                                    \
  X(KN_ORB_COPY, "orb_copy_level0") X(KN_ORB_RESIZE, "orb_resize") X(KN_ORB_FAST, "orb_fast_score")       \
  X(KN_ORB_NMS_COUNT, "orb_nms_count") X(KN_ORB_ROW_SCAN, "orb_row_scan") X(KN_ORB_COMPACT, "orb_nms_compact") \
  X(KN_ORB_SELECT1, "orb_select_fast") X(KN_ORB_HARRIS, "orb_harris") X(KN_ORB_SELECT2, "orb_select_harris") \
  X(KN_ORB_OFFSETS, "orb_offsets") X(KN_ORB_ANGLE, "orb_angle") X(KN_ORB_BLUR, "orb_blur")                \
  X(KN_ORB_BRIEF, "orb_brief") X(KN_BF_ARGMIN, "bf_argmin") X(KN_BF_FINISH, "bf_finish")                  \
  X(KN_SG_VERT, "sgbm_vert") X(KN_SG_ROWS, "sgbm_rows") X(KN_SG_MEDIAN, "sgbm_median")                    \
  X(KN_BACKPROJECT, "backproject") X(KN_PNP, "pnp_ransac") X(KN_BA_STEREO, "ba_stereo")                   \
  X(KN_BA_BUILD, "ba_build") X(KN_BA_SOLVE, "ba_solve") X(KN_GATHER, "gather_matches")                    \
  X(KN_ESSENTIAL, "essential_ransac") X(KN_RECOVER, "recover_pose") X(KN_INGEST, "ingest_undistort_gray") \
  X(KN_MOTION_BLUR, "motion_blur") X(KN_MAP_XFORM, "map_transform") X(KN_VOXEL, "voxel_down_sample")      \
  X(KN_BF_KNN, "bf_knn") X(KN_BF_RATIO, "bf_ratio") X(KN_SPK_LOCAL, "speckle_local")                      \
  X(KN_SPK_SEAMS, "speckle_seams") X(KN_SPK_SUM, "speckle_sum") X(KN_SPK_APPLY, "speckle_apply")
#define FVO_KERNEL_ID(id, name) id,
enum FvoKernel { FVO_KERNELS(FVO_KERNEL_ID) KN_COUNT };
#undef FVO_KERNEL_ID

struct TimingRec {
  int id;
  hipEvent_t a, b;
};

struct fvo_ctx {
  int device = 0;
  uint64_t tmask = 0;                 // kernels whose launches are bracketed by events
  std::vector<TimingRec> trecs;
  std::vector<hipEvent_t> tpool;
  fvo_config cfg{};
  OrbGeom g{};
  std::string err;
  int kp_cap = 0;
  int64_t ws_bytes = 0;
  std::vector<void*> allocs;          // every fvo_alloc of this context; freed by capi.cpp's release()
  // ORB workspace (per image b < max_batch)
  uint8_t* pyr = nullptr;     // [B][total_px]
  uint8_t* blur = nullptr;    // [B][total_px] debug only (orb_blur_debug), allocated on first use
  int orb_last_batch = 0;     // images of the last ORB call
  uint8_t* score = nullptr;   // [B][total_px]
  uint32_t* cand = nullptr;   // [B][cand_total] packed (score<<24 | y<<12 | x)
  uint64_t* hel = nullptr;    // [B][cand_total] (harris float bits << 32 | packed)
  int32_t* ncand = nullptr;   // [B][L]
  int32_t* nsel1 = nullptr;   // [B][L]
  int32_t* nsel2 = nullptr;   // [B][L]
  int32_t* koff = nullptr;    // [B][L+1]
  int32_t* scratch = nullptr; // [B*L][2*maxcand] selection position lists
  int64_t scratch_per = 0;
  ResizeTab rt{};
  int32_t* umax = nullptr;    // IC angle row extents
  // BF workspace
  uint32_t* bf_rowkey = nullptr;  // [B][cap] (distance << 16 | train index) minimum per query row
  uint32_t* bf_colkey = nullptr;  // [B][cap] (distance << 16 | query index) minimum per train column
  uint32_t* bf_knn = nullptr;     // [3][B][cap] ratio test: forward keys 1 and 2 per row, reverse key per column
  // SGBM workspace
  uint16_t* sg_V = nullptr;     // top-down path V, [B][HG4 + nstripes][width1][4][D] (4-row groups)
  uint16_t* sg_M = nullptr;     // min over d of each V row, [B][HG4 + nstripes][width1][4]
  uint32_t* sg_ckpt = nullptr;  // [B][4-row blocks][nck][64 lanes][ckw] left->right path checkpoints
  int16_t* sg_raw = nullptr;    // [B][H][W] pre-median disparity
  uint64_t* sg_hand = nullptr;  // [B][H][2][D/32][16] L-path hand-off granules (cost pass, column block to block)
  uint32_t* sg_ctl = nullptr;   // [4 + B] ticket, generation, hand-off timeouts, per-pair failure flags
  // fvo_ba_count_births's record: the window range whose birth counts are already in the BA
  // workspace (valid until the next BA call)
  struct {
    bool valid = false;
    const void* matches = nullptr;
    const void* nmatch = nullptr;
    const void* stereo = nullptr;
    int nframes = 0, first_end = 0, nwin = 0, first_valid = 0;
  } ba_births;
  // pose workspace
  double* pnp_hyp = nullptr;      // [B][cap][2] normalised inlier points (refinement)
  int32_t* pnp_sub = nullptr;     // [B][cap] inlier indices
  int16_t* rs_table = nullptr;    // [cap+1][rs_table_iters][5] RNG(-1) RANSAC subsets per point count
  int32_t rs_table_iters = 0;     //   (shared by PnP and the essential-matrix RANSAC)
  double* pnp_models = nullptr;   // [B][max_iters][6] hypotheses (rvec, tvec)
  double* pnp_ws = nullptr;       // [B][max_iters][PNP_WS] EPnP null space + subset state between launches
  int32_t* pnp_good = nullptr;    // [B][max_iters] inlier counts
  void* pnp_state = nullptr;      // [B] PnpState
  float* pnp_pts = nullptr;        // [B][5 * cap] the refinement's compacted inliers past its LDS
  int32_t* pnp_plan = nullptr;    // [3][B + 1] round-2 work-unit prefix sums (units of 64, 8, 16 iterations)
  int32_t pnp_max_iters = 0;
  uint8_t* fast_rec = nullptr;    // [B][tiles][kTRec] per FAST tile: row keep words + prefixes + kept scores
  // local BA workspace (per window w < max_batch; strides in ba_* counts)
  void* ba_ws = nullptr;          // one allocation, carved per window (ba.hip)
  int64_t ba_win_bytes = 0;
  hipStream_t ba_s2 = nullptr;    // second stream: half of the windows' LM sequences (ba.hip)
  hipEvent_t ba_fork = nullptr, ba_join = nullptr;
  // mono (essential matrix) workspace
  double* em_x = nullptr;         // [B][cap][4] normalised (x1, y1, x2, y2)
  double* em_models = nullptr;    // [B][max_iters][10][9] 5-point solutions
  int32_t* em_good = nullptr;     // [B][max_iters][10] inlier counts
  int8_t* em_nmod = nullptr;      // [B][max_iters] solutions per subset
  double* em_ws = nullptr;        // [B][max_iters][EM_WS] per-subset solver stages (basis, 10x20, B(z), det)
  void* em_state = nullptr;       // [B] EmState
  int32_t em_max_iters = 0;
  // rectification (rectify.hip): LDS bytes a block may stage (fvo_rectify_lds_budget)
  int32_t rectify_budget = FVO_RECTIFY_LDS_BYTES;
};

// Error helpers: set ctx->err and return negative status.
int fvo_fail(fvo_ctx* ctx, const std::string& msg);
#define FVO_HIP(ctx, expr)                                                                 \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fvo_fail(ctx, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define FVO_LAUNCH_CHECK(ctx) FVO_HIP(ctx, hipGetLastError())

hipEvent_t fvo_event(fvo_ctx* ctx);
// Launch `...` on stream `s`; when kernel `id` is in ctx->tmask, bracket it with events.
#define FVO_TIMED(ctx, id, s, ...)                               \
  do {                                                           \
    const bool t_ = ((ctx)->tmask >> (id)) & 1ull;               \
    hipEvent_t a_ = nullptr, b_ = nullptr;                       \
    if (t_) {                                                    \
      a_ = fvo_event(ctx);                                       \
      (void)hipEventRecord(a_, s);                               \
    }                                                            \
    __VA_ARGS__;                                                 \
    if (t_) {                                                    \
      b_ = fvo_event(ctx);                                       \
      (void)hipEventRecord(b_, s);                               \
      (ctx)->trecs.push_back(TimingRec{(int)(id), a_, b_});      \
    }                                                            \
  } while (0)

// Per-module init/launchers (defined in the .hip files).  Arguments and fvo_config are validated by
// capi.cpp before any of them runs; they call fvo_fail for HIP runtime errors only.
int orb_init(fvo_ctx* ctx);
int orb_run(fvo_ctx* ctx, const uint8_t* images, int batch, int64_t image_stride, int pitch, float* kp, uint8_t* desc,
            int32_t* counts, int cap, hipStream_t s);
int bf_init(fvo_ctx* ctx);
int bf_run(fvo_ctx* ctx, const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch, int cap,
           int32_t* matches, int32_t* nmatch, hipStream_t s);
// k-nearest neighbours / ratio test (bf.hip)
int bf_knn_run(fvo_ctx* ctx, const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch,
               int cap, int k, int32_t* knn, hipStream_t s);
int bf_ratio_run(fvo_ctx* ctx, const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch,
                 int cap, double ratio, int mutual, int32_t* matches, int32_t* nmatch, hipStream_t s);
int sgbm_init(fvo_ctx* ctx);
int sgbm_run(fvo_ctx* ctx, const uint8_t* L, const uint8_t* R, int batch, int64_t image_stride, int pitch,
             int16_t* disp, int32_t* status, hipStream_t s);
int pose_init(fvo_ctx* ctx);
int ransac_table_init(fvo_ctx* ctx);
int orb_blur_debug(fvo_ctx* ctx);
int orb_score_debug(fvo_ctx* ctx);
int orb_retain_best_run(fvo_ctx* ctx, const float* keys, int n, int keep, int32_t* idx_out, int32_t* n_out,
                         hipStream_t s);
int backproject_run(fvo_ctx* ctx, const int16_t* disp, const float* kp0, const float* kp1, const int32_t* matches,
                    const int32_t* nmatch, int batch, int cap, const double* K, double baseline, float* P3, float* p2,
                    int32_t* npts, hipStream_t s);
int pnp_run(fvo_ctx* ctx, const float* P3, const float* p2, const int32_t* npts, int batch, int cap, const double* K,
            const double* dist, float reproj, double conf, int iters, double* rvec, double* tvec, double* T,
            int32_t* status, uint8_t* inliers, hipStream_t s);

// Host arithmetic of the calibration checks (capi.cpp, capi_rectify.cpp).  inv3: OpenCV invert() 3x3
// closed form, operation for operation as the device copies (csrc/ingest.hip, oracle/ingest_ref.cpp),
// so det == 0 here is det == 0 there; false: det == 0.
inline bool host_inv3(const double* S, double* t) {
  double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
  if (d == 0.) return false;
  d = 1. / d;
  t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
  t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
  t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
  t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
  t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
  t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
  t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
  t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
  t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
  return true;
}
inline bool host_all_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}
// is the ray denominator w > 0 with a finite reciprocal (the kernels divide by it)
inline bool host_ray_w_ok(double w) { return w > 0.0 && std::isfinite(1. / w); }

// cv2.undistort's stripe height (oracle/ingest_ref.cpp): the rows that share one camera matrix, K with
// cy moved to the stripe's first row.  ingest_run launches with it, fvo_undistort_gray checks every
// stripe's matrix.
inline int ingest_stripe_rows(int W, int H) {
  const int s = 4096 / (W > 1 ? W : 1);
  return s < 1 ? 1 : (s > H ? H : s);
}
int ingest_run(fvo_ctx* ctx, const uint8_t* bgr, int batch, int64_t sstride, int spitch, const double* K,
               const double* dist, uint8_t* gray, int64_t dstride, int dpitch, hipStream_t s);
int motion_blur_run(fvo_ctx* ctx, const uint8_t* img, int batch, int64_t sstride, int spitch, int ksize,
                    const int32_t* centers, const int32_t* ncent, int cap, uint8_t* mask, uint8_t* out,
                    int64_t dstride, int dpitch, hipStream_t s);
int map_transform_run(fvo_ctx* ctx, const float* pts, int stride, const int32_t* npts, int batch, int64_t cap,
                      const double* T, int32_t* count, int64_t map_cap, double* out64, float* out32, hipStream_t s);
int chain_poses_run(fvo_ctx* ctx, const double* T, const int32_t* status, const int32_t* npts, int n_seq, int n,
                    double* cum, double* cum_out, int32_t* npts_out, hipStream_t s);
struct FvoRegions {
  fvo_region r[FVO_MAX_REGIONS];
};
int copy_regions_run(fvo_ctx* ctx, int count, const fvo_region* regions, hipStream_t s);
int count_guard_run(fvo_ctx* ctx, const int32_t* cnt, const int32_t* q_cnt, int n, int sets, int32_t* status,
                    int32_t code, int32_t* nkp_out, hipStream_t s);
int64_t voxel_workspace_bytes(int64_t n);
int voxel_run(fvo_ctx* ctx, const double* pts, int64_t n, double voxel, void* ws, double* out,
              int32_t* n_out, int32_t* status, hipStream_t s);
// Speckle filter (speckle.hip).  ws: two int32 planes
// [batch][H*W] (fvo_speckle_workspace_bytes).
int speckle_run(fvo_ctx* ctx, int16_t* disp, int batch, int H, int W, int64_t image_stride, int pitch, int new_val,
                int max_speckle_size, int max_diff, void* ws, hipStream_t s);
// Dense stereo mapping (dense.hip).  A frame's samples
// (every step-th pixel of every step-th row, row-major) are cut into blocks of kDenseBlock; ws:
// [int64 map base][int64 offset per block][int32 count per block] over batch * blocks
// (fvo_dense_workspace_bytes).
constexpr int kDenseBlock = 1024;  // 256 threads x 4 consecutive samples
inline int64_t dense_frame_samples(int H, int W, int step) {
  return (int64_t)((H - 1) / step + 1) * ((W - 1) / step + 1);
}
inline int64_t dense_frame_blocks(int H, int W, int step) {
  return (dense_frame_samples(H, W, step) + kDenseBlock - 1) / kDenseBlock;
}
int dense_append_run(fvo_ctx* ctx, const int16_t* disp, int batch, int H, int W, int64_t image_stride, int pitch,
                     const double* K, double baseline, int step, int min_disp16, float z_min, float z_max,
                     const int32_t* frame_keep, const double* T, int32_t* count, int64_t map_cap, double* out64,
                     float* out32, int32_t* n_added, void* ws, hipStream_t s);
// cv2.reprojectImageTo3D (dense.hip).  min_key: [batch] u32, used with handle_missing only.
int reproject_run(fvo_ctx* ctx, const void* disp, int is_f32, int batch, int H, int W, int64_t image_stride,
                  int pitch, const double* Q, int handle_missing, uint32_t* min_key, float* out, hipStream_t s);
// Stereo rectification (rectify.hip).  capi_rectify.cpp validates the calibration and hands the
// launchers this: ir = inverse(newK * R) by the 3x3 closed form, the camera's own fx, fy, cx, cy
// and the radial-tangential coefficients (rational: n_dist == 8, else k4..k6 = 0 and the
// denominator, exactly 1, is dropped).
struct RectifyLens {
  double ir[9];
  double fx, fy, u0, v0;
  double k1, k2, p1, p2, k3, k4, k5, k6;
  int rational;
};
int rectify_map_run(fvo_ctx* ctx, const RectifyLens& L, int16_t* map1, uint16_t* map2, hipStream_t s);
int remap_run(fvo_ctx* ctx, const uint8_t* src, int batch, int64_t sstride, int spitch, int channels,
              const int16_t* map1, const uint16_t* map2, uint8_t* dst, int64_t dstride, int dpitch, hipStream_t s);
int rectify_gray_run(fvo_ctx* ctx, const uint8_t* src, int batch, int64_t sstride, int spitch, int channels,
                     const RectifyLens& L, uint8_t* gray, int64_t dstride, int dpitch, hipStream_t s);
// Sparse stereo (sparse_stereo.hip).  capi_stereo.cpp validates the parameters and hands the
// launcher the level scales by value.  ws: two u32 key planes [batch][cap] (left rows, right columns).
constexpr int kSparseMaxLevels = 32;
constexpr int kSparseMaxHalfWindow = 7, kSparseMaxHalfSlide = 8;  // sparse_stereo.hip sizes its LDS by them
struct SparseLevels {
  float scale[kSparseMaxLevels];
  int n;
};
int sparse_stereo_run(fvo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int64_t image_stride,
                      int pitch, const float* kpL, const int32_t* nL, const uint8_t* descL, const float* kpR,
                      const int32_t* nR, const uint8_t* descR, int cap, const fvo_sparse_stereo_params& p,
                      const SparseLevels& levels, const double* K, double baseline, void* ws, float* stereo,
                      int32_t* info, hipStream_t s);
int backproject_stereo_run(fvo_ctx* ctx, const float* stereo, const float* kp1, const int32_t* matches,
                           const int32_t* nmatch, int batch, int cap, float* P3, float* p2, int32_t* npts,
                           hipStream_t s);
// Outlier removal (outlier.hip).  capi_outlier.cpp validates the arguments.  ws: the grid's sorted
// keys, the points in that order, the averages, the exact pass's list and the sums' partials
// (fvo_outlier_workspace_bytes; the top-k lists are in LDS, so the size does not depend on k).
int64_t outlier_workspace_bytes(int64_t n);
int statistical_outliers_run(fvo_ctx* ctx, const double* pts, int64_t n, int nb_neighbors, double std_ratio,
                             double cell, int max_rings, void* ws, uint8_t* keep, double* avg_distance, double* stats,
                             int32_t* status, hipStream_t s);
int radius_outliers_run(fvo_ctx* ctx, const double* pts, int64_t n, int nb_points, double radius, double cell,
                        void* ws, uint8_t* keep, int32_t* n_neighbors, int32_t* status, hipStream_t s);
int select_points_run(fvo_ctx* ctx, const double* pts, int64_t n, const uint8_t* keep, double* out64, float* out32,
                      int32_t* n_out, hipStream_t s);
// Normal and covariance estimation (normals.hip).  capi_normals.cpp validates the arguments.  ws: the
// grid's sorted keys, the points in that order and the exact pass's list
// (fvo_normals_workspace_bytes; the candidate lists are in LDS, so the size does not depend on max_nn).
// ref: host double[3], read before the launch.
int64_t normals_workspace_bytes(int64_t n);
int estimate_normals_run(fvo_ctx* ctx, const double* pts, int64_t n, int max_nn, double radius, double cell,
                         int max_rings, void* ws, double* normals, int has_prior, double* covariances,
                         int32_t* n_neighbors, int32_t* stats, int32_t* status, hipStream_t s);
int orient_normals_run(fvo_ctx* ctx, const double* pts, double* normals, int64_t n, int mode, const double* ref,
                       hipStream_t s);
// ICP registration (icp.hip).  capi_icp.cpp validates the arguments.  ws: the target's grid (sorted
// keys, points and normals in that order), the source's order, one row of partial sums per block of
// 256 source points and the call's state (fvo_icp_workspace_bytes).  init / T: host double[16], read
// before the first launch.  icp_trivial_run: the result of an empty source or target (no search).
int64_t icp_workspace_bytes(int64_t n_source, int64_t n_target);
int registration_icp_run(fvo_ctx* ctx, const double* source, int64_t ns, const double* target,
                         const double* target_normals, int64_t nt, double radius, double cell, const double* init,
                         int estimation, double rel_fitness, double rel_rmse, int max_iteration, void* ws,
                         double* result, double* sums, int32_t* correspondences, int32_t* status, hipStream_t s);
int icp_trivial_run(fvo_ctx* ctx, const double* init, int64_t ns, double* result, double* sums,
                    int32_t* correspondences, int32_t* status, hipStream_t s);
int transform_points_run(fvo_ctx* ctx, double* points, float* points32, double* normals, int64_t n, const double* T,
                         hipStream_t s);
int mono_init(fvo_ctx* ctx);
int gather_run(fvo_ctx* ctx, const float* kp0, const float* kp1, const int32_t* matches, const int32_t* nmatch,
               int batch, int cap, float* p0, float* p1, int32_t* npts, hipStream_t s);
int essential_run(fvo_ctx* ctx, const float* p0, const float* p1, const int32_t* npts, int batch, int cap,
                  double focal, double cx, double cy, double prob, double threshold, int maxIters, double* E,
                  uint8_t* mask, int32_t* status, hipStream_t s);
int recover_run(fvo_ctx* ctx, const double* E, const int32_t* est, const float* p0, const float* p1,
                const int32_t* npts, int batch, int cap, double focal, double cx, double cy, double dist, double* R,
                double* t, double* T, int32_t* ngood, hipStream_t s);

int ba_init(fvo_ctx* ctx);
int ba_export_run(fvo_ctx* ctx, int window, double* xyz, int32_t* count, hipStream_t s);
int ba_births_run(fvo_ctx* ctx, const int32_t* matches, const int32_t* nmatch, const float* stereo, int nframes,
                  int cap, int first_end, int nwin, int first_valid, hipStream_t s);
int ba_stereo_run(fvo_ctx* ctx, const int16_t* disp, const float* kp, const int32_t* nkp, int batch, int cap,
                  const double* K, double baseline, float* stereo, hipStream_t s);
int ba_run(fvo_ctx* ctx, const float* kp, const int32_t* nkp, const int32_t* matches, const int32_t* nmatch,
           const float* stereo, const double* Trel, int nframes, int cap, int first_end, int nwin, int first_valid,
           const double* K, double baseline, const double* inv_sigma2, int nlev, int iters, double* Tout,
           double* stats, hipStream_t s);

template <typename T>
int fvo_alloc(fvo_ctx* ctx, T** p, size_t n) {
  size_t bytes = n * sizeof(T);
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc((void**)p, bytes);
  if (e != hipSuccess) return fvo_fail(ctx, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  ctx->allocs.push_back(*p);
  ctx->ws_bytes += (int64_t)bytes;
  return 0;
}
