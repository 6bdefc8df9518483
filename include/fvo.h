/* fvo.h — C ABI of the MI355X stereo-VO hot path (forest-slam_amd, libfvo.so).
 *
 * Drop-in boundary for the OpenCV calls of si220/Forest-SLAM's ORB branch
 * (ros_ws/src/stereo_slam.py).  Every entry point replaces one reference call:
 *
 *   fvo_orb_detect_compute  <- cv2.ORB_create() + orb.detectAndCompute(img, None)
 *                              stereo_slam.py:84, :232-233, :240-241
 *   fvo_bf_match            <- cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True).match(d0, d1)
 *                              stereo_slam.py:85, :234, :242 (+ the :235-238 gather)
 *   fvo_bf_knn_match        <- cv2.DescriptorMatcher_create("BruteForce-Hamming").knnMatch(d0, d1, k)
 *   fvo_bf_ratio_match      <- ... + [m for m, n in knn if m.distance < ratio * n.distance]
 *                              (Lowe's ratio test; no reference counterpart)
 *   fvo_sgbm                <- cv2.StereoSGBM_create(numDisparities=96, minDisparity=0,
 *                              blockSize=7, P1=392, P2=1568, mode=SGBM_3WAY).compute(L, R)
 *                              stereo_slam.py:108-117 (get_disparity_map)
 *   fvo_backproject         <- depth = fx*B/disp, Z = depth[int(y), int(x)], X/Y, 0.1<Z<1000
 *                              stereo_slam.py:117-121 (0/-1 -> 0.1) and :262-289
 *   fvo_pnp_ransac          <- cv2.solvePnPRansac(P, p, K0, dist_l, reprojectionError=1.0,
 *                              confidence=0.99, iterationsCount=1000, SOLVEPNP_ITERATIVE)
 *                              + cv2.Rodrigues + T assembly, stereo_slam.py:292-303
 *   fvo_ba_windows          <- (new) windowed local bundle adjustment, no reference counterpart
 *                              (+ fvo_keypoint_stereo, fvo_ba_landmarks)
 *   fvo_gather_matches      <- mkpts0 = kpts0[valid], mkpts1 = kpts1[matches[valid]]
 *                              mono_slam.py:106-108 (stereo_slam.py:235-238 for the BF DMatch list)
 *   fvo_find_essential      <- cv2.findEssentialMat(mkpts0, mkpts1, focal=K0[0,0], pp=(K0[0,2], K0[1,2]),
 *                              method=cv2.RANSAC, prob=0.999, threshold=1.0)   mono_slam.py:111
 *   fvo_recover_pose        <- cv2.recoverPose(E, mkpts0, mkpts1, focal=, pp=) + the [R|t] matrix
 *                              mono_slam.py:112-117
 *   fvo_undistort_gray      <- cv2.cvtColor(cv2.undistort(img, K, dist), cv2.COLOR_BGR2GRAY)
 *                              stereo_slam.py:184-186, :196-198; mono_slam.py:92-93
 *   fvo_motion_blur         <- apply_random_motion_blur(img, blur_percentage, kernel_size, angle=0)
 *                              (cv2.getRotationMatrix2D + warpAffine + filter2D + np.where)
 *                              forest_slam_ros/src/stereo_slam.py:142-178, :194, :206
 *   fvo_chain_poses         <- cumulative_est_tf_mat = np.dot(cumulative_est_tf_mat, T) per posed frame
 *                              (the len(points3D) >= 6 guard), stereo_slam.py:292, :306 — on the device
 *   fvo_map_transform       <- (cum @ hstack(points3D, 1).T)[:3].T appended to the map + PointCloud2
 *                              float32 packing: stereo_slam.py:308-318; mono_slam.py:148; gt_mapping.py
 *   fvo_voxel_down_sample   <- open3d PointCloud.voxel_down_sample(voxel_size=0.5)
 *                              mono_slam.py:151-155, gt_mapping.py:62-66
 *   fvo_statistical_outliers <- open3d PointCloud.remove_statistical_outlier(nb_neighbors, std_ratio)
 *   fvo_radius_outliers     <- open3d PointCloud.remove_radius_outlier(nb_points, radius)
 *   fvo_select_points       <- open3d PointCloud.select_by_index(ind) of the kept points, in order
 *   fvo_estimate_normals    <- open3d PointCloud.estimate_normals / estimate_covariances (k-NN, hybrid search)
 *   fvo_orient_normals      <- open3d PointCloud.orient_normals_towards_camera_location / _to_align_with_direction
 *   fvo_registration_icp    <- open3d pipelines.registration.registration_icp / evaluate_registration
 *                              (TransformationEstimationPointToPoint / PointToPlane)
 *   fvo_transform_points    <- open3d PointCloud.transform(T)
 *                              (the map clean-up after voxel_down_sample; no reference counterpart)
 *   fvo_filter_speckles     <- cv2.filterSpeckles / StereoSGBM_create(speckleWindowSize=, speckleRange=)
 *   fvo_dense_map_append    <- (new) the disparity maps of a batch as one world-frame point cloud: the
 *                              back-projection of stereo_slam.py:262-289 at every step-th pixel + the
 *                              map update of :308-318, no reference counterpart
 *   fvo_reproject_to_3d     <- cv2.reprojectImageTo3D(disparity, Q, handleMissingValues)
 *   fvo_rectify_map         <- cv2.initUndistortRectifyMap(K, dist, R, P, size, cv2.CV_16SC2)
 *   fvo_remap_u8            <- cv2.remap(img, map1, map2, cv2.INTER_LINEAR)
 *   fvo_rectify_gray        <- both fused + cv2.cvtColor(., COLOR_BGR2GRAY): the rectifying ingest
 *                              (no reference counterpart: the reference does not rectify)
 *
 * Conventions
 *  - All array pointers are DEVICE pointers owned by the caller (e.g. torch tensors'
 *    data_ptr()).  Calls are asynchronous on `stream` (a hipStream_t, may be NULL for
 *    the default stream); counts and statuses are written to device memory.
 *  - Every call works on a BATCH of independent items (images / image pairs / frames);
 *    `batch` <= fvo_config.max_batch.
 *  - Return value: 0 on success, <0 on argument/launch error (see fvo_last_error()).
 *    No exceptions cross this boundary.  Data-dependent failures (too few points,
 *    capacity overflow) are reported per item in the status/count outputs.
 *  - A context is not re-entrant: one context per (device, host thread).  All device
 *    workspace is allocated by fvo_create(); hot calls do not allocate and can be
 *    captured into a hipGraph.
 */
#ifndef FVO_H_
#define FVO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FVO_ABI_VERSION 7

typedef struct fvo_ctx fvo_ctx;
typedef void* fvo_stream; /* hipStream_t */

/* Keypoint record written by fvo_orb_detect_compute (8 x float32 per keypoint):
 * x, y (level-0 pixels), size, angle (deg), response (Harris), octave, class_id (-1), 0 */
#define FVO_KP_STRIDE 8
#define FVO_DESC_BYTES 32

typedef struct fvo_config {
  int32_t width, height; /* image size shared by every call on this context: at least 64x64
                            with the ORB stage, 64x32 with the SGBM stage alone           */
  int32_t max_batch;     /* max images (ORB) / pairs (BF, SGBM) / frames (pose) per call */
  /* cv2.ORB_create() parameters; defaults = OpenCV defaults (stereo_slam.py:84) */
  int32_t nfeatures;       /* 500 */
  float scale_factor;      /* 1.2f */
  int32_t nlevels;         /* 8 */
  int32_t edge_threshold;  /* 31 */
  int32_t first_level;     /* 0 (only 0 supported) */
  int32_t wta_k;           /* 2 (only 2 supported) */
  int32_t score_type;      /* 0 = HARRIS_SCORE (only Harris supported) */
  int32_t patch_size;      /* 31 (only 31 supported: the rBRIEF table) */
  int32_t fast_threshold;  /* 20 */
  /* cv2.StereoSGBM_create() parameters used at stereo_slam.py:109-115 */
  int32_t min_disparity;    /* 0 */
  int32_t num_disparities;  /* 96, multiple of 16 */
  int32_t block_size;       /* 7 */
  int32_t P1, P2;           /* 392, 1568 */
  int32_t disp12_max_diff;  /* 0 (-> 1 as in OpenCV) */
  int32_t pre_filter_cap;   /* 0 (-> 15) */
  int32_t uniqueness_ratio; /* 0 (only 0 supported) */
  int32_t sgbm_stripes;     /* 4: OpenCV's fixed stripe count for MODE_SGBM_3WAY */
  int32_t kp_capacity;      /* per-image keypoint capacity of the ORB outputs (0 = auto) */
  int32_t stages;           /* FVO_STAGE_* mask of the workspaces to allocate (0 = all) */
  /* local bundle adjustment (no reference counterpart: BASELINE.json north_star) */
  int32_t ba_window;        /* frames per BA window K (10); max 21 */
  int32_t ba_max_landmarks; /* per-window landmark cap (4096) */
  int32_t ba_max_obs;       /* per-window observation cap (32768) */
  int32_t sgbm_max_batch;   /* max pairs per fvo_sgbm call (0 = max_batch): the SGBM path
                               volume (one u16 volume, ~100 MB per pair at 600p) is sized by it */
  /* SGBM schedule (every schedule and launch shape is bit-identical).  Chosen
   * here, at fvo_create, and nowhere else: the library reads no environment variables. */
  int32_t sgbm_mode;        /* FVO_SGBM_CLASSIC (0, default) or FVO_SGBM_LPATH */
  int32_t sgbm_lanes;       /* classic cost pass: lanes per column, 4 / 8 / 16 (0 = 8) */
  int32_t sgbm_cols;        /* classic cost pass: columns per block (0 = default; lanes 4: 32 or 64
                               (default 64), lanes 8: 16 or 32 (default 32), lanes 16: 32) */
  int32_t sgbm_handoff_us;  /* lpath: bound on one column-block hand-off wait in microseconds
                               (0 = 250000); -1 = test hook: every hand-off times out */
} fvo_config;

/* fvo_config.sgbm_mode */
#define FVO_SGBM_CLASSIC 0 /* cost pass + row pass running both horizontal sweeps */
#define FVO_SGBM_LPATH 1   /* left->right path inside the cost pass, handed between column blocks */
/* fvo_sgbm status values */
#define FVO_SGBM_OK 0
#define FVO_SGBM_HANDOFF_TIMEOUT (-1) /* lpath: a hand-off wait of the pair timed out; its disparity
                                         map is all invalid ((min_disparity-1)*16) */

/* fvo_config.stages: a context only serves the stages it was created for (e.g. a
 * BFMatcher-only context needs no image-sized workspace). */
#define FVO_STAGE_ORB 1
#define FVO_STAGE_BF 2
#define FVO_STAGE_SGBM 4
#define FVO_STAGE_POSE 8
#define FVO_STAGE_BA 16
#define FVO_STAGE_MONO 32
#define FVO_STAGE_ALL 63

/* Fill `cfg` with the reference's parameters for a width x height image. */
void fvo_config_default(fvo_config* cfg, int32_t width, int32_t height);

/* Layout of fvo_config as this library was compiled: sizeof, and offsetof(field) in bytes
 * (-1 for an unknown name).  A binding that declares the struct itself (ctypes, cffi, cgo)
 * checks its declaration against these before calling fvo_config_default / fvo_create. */
int32_t fvo_config_size(void);
int32_t fvo_config_offset(const char* field);

int fvo_create(int device, const fvo_config* cfg, fvo_ctx** out);
void fvo_destroy(fvo_ctx* ctx);
const char* fvo_last_error(const fvo_ctx* ctx);
int fvo_abi_version(void);
/* Per-image keypoint capacity (rows of the keypoint/descriptor outputs). */
int fvo_kp_capacity(const fvo_ctx* ctx);
/* Device workspace bytes held by the context. */
int64_t fvo_workspace_bytes(const fvo_ctx* ctx);

/* ORB detectAndCompute on `batch` grayscale u8 images.
 * images:      batch images, image b at images + b*image_stride, rows `pitch` bytes apart.
 * keypoints:   [batch][cap][FVO_KP_STRIDE] f32     descriptors: [batch][cap][32] u8
 * counts:      [batch] i32 = number of keypoints, or -(needed) if it exceeds `cap`
 *              (outputs then unspecified).  Keypoint order = OpenCV's output order. */
int fvo_orb_detect_compute(fvo_ctx* ctx, const uint8_t* images, int32_t batch, int64_t image_stride,
                           int32_t pitch, float* keypoints, uint8_t* descriptors, int32_t* counts,
                           int32_t cap, fvo_stream stream);

/* Cross-checked brute-force Hamming matching of `batch` (query, train) descriptor sets.
 * query/train: [batch][cap][32] u8 with per-item counts n_query/n_train [batch] (<=0: empty).
 * matches:     [batch][cap][3] i32 rows (queryIdx, trainIdx, distance), ascending queryIdx.
 * n_matches:   [batch] i32. */
int fvo_bf_match(fvo_ctx* ctx, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                 const int32_t* n_train, int32_t batch, int32_t cap, int32_t* matches, int32_t* n_matches,
                 fvo_stream stream);

/* The k nearest train descriptors of every query descriptor, without cross-check
 * (DescriptorMatcher.knnMatch(q, t, k) for NORM_HAMMING): row q's neighbours are the min(k, n_train)
 * train indices with the smallest (distance, trainIdx), in that order -- equal distances keep
 * ascending train index, batchDistance's strict-< insertion.  query/train/counts as for
 * fvo_bf_match; 1 <= k <= FVO_BF_MAX_K.
 * knn: [batch][cap][k][2] i32 = (trainIdx, distance); (-1, -1) where a row has fewer than k
 *      neighbours; rows >= n_query are not written.
 * Stateless: the call reads and leaves no context state (so does fvo_bf_ratio_match). */
#define FVO_BF_MAX_K 8
int fvo_bf_knn_match(fvo_ctx* ctx, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                     const int32_t* n_train, int32_t batch, int32_t cap, int32_t k, int32_t* knn, fvo_stream stream);

/* Lowe's ratio test on the two nearest neighbours (m, n = knnMatch(q, t, 2)[i]): query row q is
 * kept iff it has two neighbours and (double)m.distance < ratio * (double)n.distance (one IEEE
 * double multiply, strict compare: Python's `m.distance < ratio * n.distance`), and, with
 * mutual != 0, q is also the nearest query of m.trainIdx (smallest (distance, queryIdx): the
 * cross-check of fvo_bf_match), which makes the result a subset of fvo_bf_match's.
 * ratio must be finite and > 0.  matches/n_matches exactly as fvo_bf_match. */
int fvo_bf_ratio_match(fvo_ctx* ctx, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                       const int32_t* n_train, int32_t batch, int32_t cap, double ratio, int32_t mutual,
                       int32_t* matches, int32_t* n_matches, fvo_stream stream);

/* StereoSGBM 3-way disparity (incl. the final 3x3 median) of `batch` rectified pairs.
 * disparity: [batch][height][width] i16, disparity*16, invalid = (min_disparity-1)*16.
 * status:    [batch] i32 (device, may be NULL): FVO_SGBM_OK, or FVO_SGBM_HANDOFF_TIMEOUT (only
 *            under FVO_SGBM_LPATH) when the pair's disparities were dropped. */
int fvo_sgbm(fvo_ctx* ctx, const uint8_t* left, const uint8_t* right, int32_t batch, int64_t image_stride,
             int32_t pitch, int16_t* disparity, int32_t* status, fvo_stream stream);

/* Matched-keypoint back-projection through the disparity map (stereo_slam.py:262-289).
 * kp0/kp1:   keypoint records of the previous / current left images ([batch][cap][8]).
 * matches:   fvo_bf_match output (query = previous, train = current).
 * K:         host double[9] row-major camera matrix; baseline in metres.
 * points3d:  [batch][cap][3] f32 valid points (0.1 < Z < 1000), compacted in match order.  f32
 *            because the reference's NumPy 1.x (Python 3.8) evaluates float64-scalar x
 *            float32-array expressions in float32 (value-based casting), DESIGN.md §Parity.
 * points2d:  [batch][cap][2] f32 matching current-image keypoints.  n_points: [batch]. */
int fvo_backproject(fvo_ctx* ctx, const int16_t* disparity, const float* kp0, const float* kp1,
                    const int32_t* matches, const int32_t* n_matches, int32_t batch, int32_t cap, const double* K,
                    double baseline, float* points3d, float* points2d, int32_t* n_points, fvo_stream stream);

/* solvePnPRansac(SOLVEPNP_ITERATIVE) + Rodrigues on `batch` independent frames.
 * K, dist:   host double[9] / double[5] (k1 k2 p1 p2 k3).
 * rvec/tvec: [batch][3] f64.   T: [batch][16] f64 row-major [R|t;0 0 0 1].
 * status:    [batch] i32: 1 pose valid, 0 RANSAC failed, -1 skipped (n_points < 6,
 *            the reference's `len(points3D) >= 6` guard, stereo_slam.py:292).
 * inliers:   [batch][cap] u8 RANSAC inlier mask (may be NULL). */
int fvo_pnp_ransac(fvo_ctx* ctx, const float* points3d, const float* points2d, const int32_t* n_points,
                   int32_t batch, int32_t cap, const double* K, const double* dist, float reprojection_error,
                   double confidence, int32_t iterations, double* rvec, double* tvec, double* T, int32_t* status,
                   uint8_t* inliers, fvo_stream stream);

/* Stereo point of every keypoint of `batch` left images: the back-projection of
 * fvo_backproject (same float32 arithmetic, stereo_slam.py:265-289) applied to all
 * keypoints instead of the matched ones.  stereo: [batch][cap][4] f32 (X, Y, Z, d) in
 * camera coordinates with d the disparity used; Z = 0 when 0.1 < Z < 1000 fails.
 * Feeds fvo_ba_windows (stage FVO_STAGE_BA). */
int fvo_keypoint_stereo(fvo_ctx* ctx, const int16_t* disparity, const float* keypoints, const int32_t* n_keypoints,
                        int32_t batch, int32_t cap, const double* K, double baseline, float* stereo,
                        fvo_stream stream);

/* Windowed local bundle adjustment (specification: oracle/ba_ref.py).
 * Frame arrays cover `n_frames` consecutive frames f of one sequence:
 *   keypoints [F][cap][8], n_keypoints [F]      left-image ORB records
 *   matches [F][cap][3], n_matches [F]          BF matches frame f -> f+1 (f < F-1)
 *   stereo [F][cap][4]                          fvo_keypoint_stereo of frame f (f < F-1)
 *   T_rel [F][16]                               camera f -> camera f+1 (PnP), f < F-1
 * Window w (0 <= w < n_windows) ends at frame e = first_end + w and spans frames
 * max(first_valid, e - ba_window + 1) .. e; windows of fewer than 3 frames copy T_rel.
 * inv_sigma2: host double[n_levels] = 1 / scale_factor^(2*octave) observation weights.  A
 * keypoint's octave (record field 5, truncated toward zero) is clamped to [0, n_levels - 1]
 * before the lookup, so an octave outside the table takes the weight of its nearest entry.
 * Preconditions on the match rows (not checked; an index outside its frame reads or writes out
 * of bounds): rows r < n_matches[f] hold a query index in [0, n_keypoints[f]) and a train index
 * in [0, n_keypoints[f+1]), and a query index appears at most once per frame (the forward map
 * keypoint -> match is written without ordering, so a repeated query index would leave either
 * row's train index).  Duplicate train indices are allowed (a ratio-test match list without
 * cross-check): the tracks that share the keypoint all continue through it.
 * Only frames max(first_valid, first_end - ba_window + 1) .. first_end + n_windows - 1 are read
 * -- of the last one its keypoints alone, of T_rel the rows of the frames before it -- and only
 * rows below n_keypoints[f] / n_matches[f] (counts are clamped to [0, cap]); frames outside
 * [first_valid, first_end + n_windows - 1] and rows beyond the counts may hold anything.
 * Outputs: T_out [n_windows][16] refined camera (e-1) -> camera e transform;
 *          stats [n_windows][6] f64: cost0, cost, landmarks, observations, frames, accepted. */
int fvo_ba_windows(fvo_ctx* ctx, const float* keypoints, const int32_t* n_keypoints, const int32_t* matches,
                   const int32_t* n_matches, const float* stereo, const double* T_rel, int32_t n_frames,
                   int32_t cap, int32_t first_end, int32_t n_windows, int32_t first_valid, const double* K,
                   double baseline, const double* inv_sigma2, int32_t n_levels, int32_t iterations,
                   double* T_out, double* stats, fvo_stream stream);

/* The first step of fvo_ba_windows -- counting each window's landmark births and observations
 * per birth frame -- issued ahead of it, e.g. on a side stream while PnP runs (it reads only the
 * match rows and the keypoints' stereo points, not T_rel or the keypoints).  Arguments as for
 * fvo_ba_windows.  The next fvo_ba_windows call on this context with the same matches, n_matches,
 * stereo, n_frames, first_end, n_windows and first_valid skips that step; the caller orders the
 * two calls (the stream of fvo_ba_windows waits for this one's).  Any other BA call in between (or
 * a different window range) makes fvo_ba_windows count again itself.  The caller must not change
 * the contents of matches, n_matches or stereo between the two calls. */
int fvo_ba_count_births(fvo_ctx* ctx, const int32_t* matches, const int32_t* n_matches, const float* stereo,
                        int32_t n_frames, int32_t cap, int32_t first_end, int32_t n_windows, int32_t first_valid,
                        fvo_stream stream);

/* Refined landmarks of BA window `window` of the most recent fvo_ba_windows call (the
 * keyframe map a rank shares with the others): xyz [ba_max_landmarks][3] f64
 * in the window's first-camera frame, count [1] i32.  Device-side, no host sync. */
int fvo_ba_landmarks(fvo_ctx* ctx, int32_t window, double* xyz, int32_t* count, fvo_stream stream);

/* Matched keypoint coordinates of `batch` frame pairs (mono_slam.py:106-108):
 * p0[i] = kp0[matches[i].queryIdx].xy, p1[i] = kp1[matches[i].trainIdx].xy, f32 [batch][cap][2];
 * n_points [batch] = n_matches clamped to [0, cap]. */
int fvo_gather_matches(fvo_ctx* ctx, const float* kp0, const float* kp1, const int32_t* matches,
                       const int32_t* n_matches, int32_t batch, int32_t cap, float* p0, float* p1, int32_t* n_points,
                       fvo_stream stream);

/* cv2.findEssentialMat(p0, p1, focal, pp, cv2.RANSAC, prob, threshold, max_iters) on `batch`
 * frame pairs (stage FVO_STAGE_MONO; mono_slam.py:111).  5-point solver inside OpenCV's
 * RANSAC (RNG(-1) subsets, adaptive iterations, max_iters <= 1000).
 * E:      [batch][9] f64 row-major unit-norm essential matrix (zeros when status != 1).
 * mask:   [batch][cap] u8 inlier mask of E (may be NULL).
 * status: [batch] i32: 1 ok, 0 RANSAC found no model, -1 fewer than 5 points, -2 exactly 5
 *         points with several solutions (OpenCV returns a stacked 3k x 3 E that recoverPose rejects). */
int fvo_find_essential(fvo_ctx* ctx, const float* p0, const float* p1, const int32_t* n_points, int32_t batch,
                       int32_t cap, double focal, double cx, double cy, double prob, double threshold,
                       int32_t max_iters, double* E, uint8_t* mask, int32_t* status, fvo_stream stream);

/* cv2.recoverPose(E, p0, p1, focal=, pp=) (distanceThresh 50 for that overload) on `batch`
 * frame pairs, all points (the reference passes no mask, mono_slam.py:112), + T = [R|t].
 * e_status: fvo_find_essential status (may be NULL); frames with status != 1 get R = I, t = 0,
 *           T = I and n_good = -1 (the reference's cv2 call would raise there).
 * R [batch][9], t [batch][3], T [batch][16] f64; n_good [batch] i32 = cheirality inliers. */
int fvo_recover_pose(fvo_ctx* ctx, const double* E, const int32_t* e_status, const float* p0, const float* p1,
                     const int32_t* n_points, int32_t batch, int32_t cap, double focal, double cx, double cy,
                     double distance_thresh, double* R, double* t, double* T, int32_t* n_good, fvo_stream stream);

/* Image ingest of `batch` BGR8 camera images of one camera (any stage; no workspace):
 * cv2.undistort(img, K, dist) (new camera matrix = K, INTER_LINEAR remap, BORDER_CONSTANT 0)
 * followed by cv2.cvtColor(., COLOR_BGR2GRAY).  Image size = the context's width x height.
 * bgr:  [batch] images, image b at bgr + b*src_stride, rows src_pitch (>= 3*width) bytes apart.
 * K:    host double[9] row-major; dist: host double[5] (k1 k2 p1 p2 k3).
 * gray: [batch] u8 images at gray + b*dst_stride, rows dst_pitch bytes apart.
 * Refused, as fvo_rectify_map refuses them, but per stripe of cv2.undistort (stripe =
 * min(max(1, 4096 / width), height) rows; the stripe starting at row y0 uses K with K[5] - y0):
 * a non-finite entry of K or dist; a K for which some stripe's matrix has det == 0 by the 3x3
 * closed form; a K for which some stripe's ray denominator _w = ir[6]*col + ir[7]*i + ir[8] (ir
 * the inverse of the stripe's matrix, i the row inside the stripe) is not > 0 with a finite
 * reciprocal at one of the stripe's four corners.  OpenCV defines no output for these (the map
 * would be NaN); finite coefficients of any size are accepted (map entries saturate as cvRound
 * does). */
int fvo_undistort_gray(fvo_ctx* ctx, const uint8_t* bgr, int32_t batch, int64_t src_stride, int32_t src_pitch,
                       const double* K, const double* dist, uint8_t* gray, int64_t dst_stride, int32_t dst_pitch,
                       fvo_stream stream);

/* Stereo rectification (any stage; no workspace; image size = the context's width x height;
 * asynchronous and graph-capturable like every hot call).  Conventions of fvo_undistort_gray's
 * map: fp64, the column term evaluated directly, iu = cvRound(u*32), (short)(iu >> 5),
 * frac = (iv & 31)*32 + (iu & 31); no stripes and no cy shift (those are cv2.undistort's).
 *
 * fvo_rectify_map   <- cv2.initUndistortRectifyMap(K, dist, R, newK, (width, height), CV_16SC2)
 *   K, R, newK: host double[9] row-major; R NULL = identity, newK NULL = K (for a 3x4 projection
 *   matrix pass its left 3x3).  dist: host double[n_dist], n_dist 4 (k1 k2 p1 p2), 5 (+ k3) or
 *   8 (+ k4 k5 k6, the rational model).  Refused: non-finite entries, det(newK*R) == 0, and a
 *   view whose ray denominator _w = ir[6]*col + ir[7]*row + ir[8] (ir = inverse(newK*R)) is not
 *   > 0 (with a finite reciprocal) at every image corner.
 *   map1: device int16 [height][width][2] (x, y), 4-byte aligned; map2: device uint16
 *   [height][width].
 * fvo_remap_u8      <- cv2.remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) on `batch` u8
 *   images of `channels` (1 or 3) interleaved channels; dst has the same channel count.  Any
 *   int16 map values are safe (taps outside the image read 0); map2 is read as map2 & 1023.
 *   dst must not overlap src (refused; likewise gray and src of fvo_rectify_gray).
 * fvo_rectify_gray  <- both of the above fused, no map stored, then cv2.cvtColor(., BGR2GRAY)
 *   when channels == 3 (a mono8 image is only remapped): the rectifying ingest.  Its bytes equal
 *   fvo_rectify_map -> fvo_remap_u8 -> the 14-bit gray conversion.
 * src: image b at src + b*src_stride, rows src_pitch (>= channels*width) bytes apart; dst
 * likewise (dst_pitch >= channels*width), gray with dst_pitch >= width.
 *
 * Kernel shape: a block makes one FVO_RECTIFY_TILE_W x FVO_RECTIFY_TILE_H output tile.  With
 * [x0, x1] x [y0, y1] the bounds of the tile's integer map entries, bw = x1 - x0 + 2 and
 * bh = y1 - y0 + 2, the block stages that source box in LDS iff
 *   ((bw*channels + 6) & ~3) * bh <= FVO_RECTIFY_LDS_BYTES
 * and gathers its taps from global memory otherwise; both paths produce the same bytes. */
#define FVO_RECTIFY_TILE_W 64
#define FVO_RECTIFY_TILE_H 16
#define FVO_RECTIFY_LDS_BYTES 8192
int fvo_rectify_map(fvo_ctx* ctx, const double* K, const double* dist, int32_t n_dist, const double* R,
                    const double* newK, int16_t* map1, uint16_t* map2, fvo_stream stream);
int fvo_remap_u8(fvo_ctx* ctx, const uint8_t* src, int32_t batch, int64_t src_stride, int32_t src_pitch,
                 int32_t channels, const int16_t* map1, const uint16_t* map2, uint8_t* dst, int64_t dst_stride,
                 int32_t dst_pitch, fvo_stream stream);
int fvo_rectify_gray(fvo_ctx* ctx, const uint8_t* src, int32_t batch, int64_t src_stride, int32_t src_pitch,
                     int32_t channels, const double* K, const double* dist, int32_t n_dist, const double* R,
                     const double* newK, uint8_t* gray, int64_t dst_stride, int32_t dst_pitch, fvo_stream stream);
/* Measurement / test hook, NOT for production use: the staging budget of this context's later
 * fvo_remap_u8 and fvo_rectify_gray launches, in [0, FVO_RECTIFY_LDS_BYTES] (0 = every block
 * gathers directly; the default, FVO_RECTIFY_LDS_BYTES, is the measured faster choice).  It exists
 * so that tools/bench_rectify.py can time both paths and the tests can run both on one input; the
 * value stays on the context until set again.  The output bytes do not depend on it. */
int fvo_rectify_lds_budget(fvo_ctx* ctx, int32_t bytes);

/* Motion-blur ablation on `batch` gray images (any stage; no workspace), image size = the
 * context's width x height:  out = np.where(mask, cv2.filter2D(img, -1, diag(ones(k))/k), img)
 * where mask = union of the (2*(k//2)+1)^2 squares (clipped) centred on the sampled pixels.
 * ksize in [1, 31], smaller than the image; angle must be 0 (the only value the reference uses;
 * other angles return an error).  filter2D arithmetic: direct float path for k*k < 130, exact
 * S/k (the DFT path's value) otherwise — see csrc/ingest.hip.
 * centers: [batch][centers_cap] int32 flat pixel indices y*W+x (random.sample(range(H*W), n)),
 *          n_centers [batch] device counts; centers_cap 0 (centers may then be NULL) = no blur
 *          (mask empty).  Image b uses its first min(max(n_centers[b], 0), centers_cap) entries: a
 *          count above centers_cap is clamped to it, a negative count is an empty list.  An entry
 *          outside [0, H*W) is not a pixel and is ignored (it blurs nothing); duplicates are fine.
 * mask:    [batch][H][W] u8 device buffer (4-byte aligned), written (0/1).
 * img/out: [batch] u8 images (b*stride, rows pitch bytes apart); out must not alias img. */
int fvo_motion_blur(fvo_ctx* ctx, const uint8_t* img, int32_t batch, int64_t src_stride, int32_t src_pitch,
                    int32_t ksize, double angle, const int32_t* centers, const int32_t* n_centers, int32_t centers_cap,
                    uint8_t* mask, uint8_t* out, int64_t dst_stride, int32_t dst_pitch, fvo_stream stream);

/* Map accumulation (any stage; no workspace).  For each of `batch` point sets b (float32 xyz,
 * point p of set b at points + (b*cap + p)*point_stride, point_stride >= 3 floats (e.g. 4 for the
 * [cap][4] stereo records; floats past xyz are not read), n_points[b] device counts) and
 * its 4x4 row-major fp64 transform T[b] (device, [batch][16]):
 *   x' = ((T[0] x + T[1] y) + T[2] z) + T[3]   (likewise rows 1, 2; fp64, no contraction)
 * appended to the map in set order starting at *map_count (device), which is then advanced by
 * the total (saturating at INT32_MAX).  Every count is clamped to [0, cap] as fvo_gather_matches
 * clamps its counts: n_points[b] < 0 counts as 0 (an empty set; it moves neither the later sets
 * nor *map_count backwards), n_points[b] > cap as cap.  map_xyz64 (fp64, [map_cap][3]) and/or
 * map_xyz32 (the PointCloud2 FLOAT32 x/y/z record, [map_cap][3]) may be NULL (not both); points
 * past map_cap are dropped while *map_count still counts them (caller checks for overflow). */
int fvo_map_transform(fvo_ctx* ctx, const float* points, int32_t point_stride, const int32_t* n_points, int32_t batch,
                      int64_t cap, const double* T, int32_t* map_count, int64_t map_cap, double* map_xyz64,
                      float* map_xyz32, fvo_stream stream);

/* Pose chains of n_seq sequences advanced over one batch of n frames each (any stage; no
 * workspace) — stereo_slam.py:292-306 on the device, for the map of every posed frame:
 * for s < n_seq, i < n in order, a frame is posed when status[s*n + i] >= 0 (pose valid, or
 * RANSAC failure with its identity T; -1 = the len(points3D) >= 6 skip, other negatives =
 * padding / overflow: not posed).  A posed frame advances cum[s] = cum[s] @ T[s*n + i] (fp64,
 * C_ij = ((c_i0 t_0j + c_i1 t_1j) + c_i2 t_2j) + c_i3 t_3j, no contraction — NumPy's BLAS order
 * is unpinned, <= 1 ulp).  Outputs: cum_out[s*n + i] = cum[s] after frame i, n_points_out[s*n + i]
 * = n_points[s*n + i] for posed frames, 0 otherwise (so fvo_map_transform(points, n_points_out,
 * cum_out) appends exactly the posed frames' points3D, stereo_slam.py:308-314).
 * cum_state: [n_seq][16] fp64 row-major, read and advanced in place (identity at a sequence's
 * start).  T, cum_out: [n_seq*n][16] fp64; status, n_points, n_points_out: [n_seq*n] int32.
 * n_points may be NULL (n_points_out then NULL too). */
int fvo_chain_poses(fvo_ctx* ctx, const double* T, const int32_t* status, const int32_t* n_points, int32_t n_seq,
                    int32_t n, double* cum_state, double* cum_out, int32_t* n_points_out, fvo_stream stream);

/* Step bookkeeping in one launch each (no reference call: the reference keeps these per frame
 * as Python lists; a batched front end would otherwise issue a dozen small copies and
 * elementwise ops per step, each a separate dispatch).  Any stage; no workspace.
 * fvo_copy_regions: `count` (0..FVO_MAX_REGIONS) device-to-device copies of regions[i].bytes
 * from regions[i].src to regions[i].dst, in one launch.  No region's destination may overlap
 * another region's source or destination, or its own source (refused: copy through a
 * temporary).  The region array is host memory, read before the call returns.
 * fvo_count_guard: for i < n, status[i] = code when any of counts[s*n + i] or
 * q_counts[s*n + i] (s < sets; q_counts may be NULL) is negative -- ORB's -(needed) overflow
 * report; counts_clamped[i] = max(counts[i], 0) (status and counts_clamped may be NULL). */
#define FVO_MAX_REGIONS 32
typedef struct {
  void* dst;
  const void* src;
  int64_t bytes;
} fvo_region;
int fvo_copy_regions(fvo_ctx* ctx, int32_t count, const fvo_region* regions, fvo_stream stream);
int fvo_count_guard(fvo_ctx* ctx, const int32_t* counts, const int32_t* q_counts, int32_t n, int32_t sets,
                    int32_t* status, int32_t code, int32_t* counts_clamped, fvo_stream stream);

/* Open3D PointCloud::VoxelDownSample(voxel_size) of n_points fp64 xyz points (device [n][3]):
 * vmin = min_bound - voxel/2, voxel index floor((p - vmin)/voxel), per voxel the fp64 sum of
 * its points in input order divided by the count.  Output: out [<= n][3] fp64 ordered by
 * voxel index (x, then y, then z — Open3D's hash-map order is unspecified), *n_out (device).
 * workspace: device scratch of fvo_voxel_workspace_bytes(n_points) bytes (caller-owned).
 * status (device, may be NULL): 0 ok, 1 = a voxel index outside [0, 2^21) (result invalid). */
int64_t fvo_voxel_workspace_bytes(int64_t n_points);
int fvo_voxel_down_sample(fvo_ctx* ctx, const double* points, int64_t n_points, double voxel_size, void* workspace,
                          int64_t workspace_bytes, double* out, int32_t* n_out, int32_t* status, fvo_stream stream);

/* Open3D PointCloud::RemoveStatisticalOutliers / RemoveRadiusOutliers (0.17, restated; any stage,
 * no context workspace) on n_points fp64 xyz points (device [n][3], not modified), and the
 * selection of the kept points.  Specification: tests/outlier_ref.py.  All arithmetic is fp64 in
 * the order written here; d2(i, j) = ((dx*dx + dy*dy) + dz*dz) with dx = p_j.x - p_i.x.
 * Statistical: k = min(nb_neighbors, n); point i's neighbours are the k smallest d2(i, j) over all
 * j in [0, n), j = i included (the KD-tree returns the query at distance 0); avg_i = (((0 +
 * sqrt(d2_(0))) + sqrt(d2_(1))) + ...) / (double)k in ascending order of d2; mean = sum of the
 * avg_i > 0 over n, std = sqrt(sum of (avg_i - mean)^2 over the avg_i > 0, over n - 1), threshold =
 * mean + std_ratio * std; keep[i] = avg_i > 0 && avg_i < threshold.  A point whose k nearest all
 * coincide with it (avg = 0) is dropped and is in neither sum; with n = 1 std is 0/0 and nothing
 * is kept.  avg_distance, keep and stats[3..5] are exact; the two sums are deterministic (fixed
 * order, no floating-point atomics, serial chains of <= 4096 terms), so stats[0..2] repeat bit
 * for bit and differ from a correctly rounded sum by ~1e-12 relative at most.
 * Radius: count_i = #{ j : d2(i, j) < radius*radius } (strict, j = i included), keep[i] =
 * count_i > nb_points.
 * Both search a uniform grid of side `cell` (origin: the min bound; keys as
 * fvo_voxel_down_sample's): cell and max_rings change the time only, never a result.  The
 * statistical search visits the cells at Chebyshev distance 0 .. max_rings of the query's own and
 * finishes the queries it cannot prove complete there (true flyers) by a brute-force pass over
 * all n points, which gives the same bits; the radius search visits ceil(radius / cell) + 1 rings,
 * so radius / cell > 8 is refused.
 * workspace: device scratch of fvo_outlier_workspace_bytes(n_points, nb_neighbors) bytes
 *            (nb_neighbors = 1 for the radius call; caller-owned, 8-byte aligned, needs no clearing
 *            between calls); that function returns -1 for a refused size.
 * keep:      device [n] u8, 1 = kept.  avg_distance: device [n] or NULL.  n_neighbors: [n] or NULL.
 * stats:     device double[6]: mean, std, threshold, valid (= n), kept, queries finished by the
 *            brute-force pass.
 * status (device, may be NULL): 0 ok, 1 = a cell index outside [0, 2^21) or a non-finite
 *            coordinate (every result invalid).
 * fvo_select_points: out64 / out32 (one may be NULL) receive the points with keep[i] != 0 in input
 * order, as fp64 rows and / or their float32 casts, *n_out (device) their number; nothing is
 * written past it.  Neither output may overlap points.
 * n_points == 0 returns 0 after the argument checks (points, workspace and keep may then be NULL;
 * stats and *n_out are zeroed).  Nothing is allocated; the calls are stream-ordered and can be
 * captured into a hipGraph; their launches are not in the fvo_timing_* table. */
#define FVO_OUTLIER_MAX_K 64
int64_t fvo_outlier_workspace_bytes(int64_t n_points, int32_t nb_neighbors);
int fvo_statistical_outliers(fvo_ctx* ctx, const double* points, int64_t n_points, int32_t nb_neighbors,
                             double std_ratio, double cell, int32_t max_rings, void* workspace,
                             int64_t workspace_bytes, uint8_t* keep, double* avg_distance, double* stats,
                             int32_t* status, fvo_stream stream);
int fvo_radius_outliers(fvo_ctx* ctx, const double* points, int64_t n_points, int32_t nb_points, double radius,
                        double cell, void* workspace, int64_t workspace_bytes, uint8_t* keep, int32_t* n_neighbors,
                        int32_t* status, fvo_stream stream);
int fvo_select_points(fvo_ctx* ctx, const double* points, int64_t n_points, const uint8_t* keep, double* out64,
                      float* out32, int32_t* n_out, fvo_stream stream);

/* Open3D PointCloud::EstimateNormals / EstimateCovariances (0.17, restated; any stage, no context
 * workspace) with a k-NN or hybrid search on n_points fp64 xyz points (device [n][3], not
 * modified), and OrientNormalsTowardsCameraLocation / OrientNormalsToAlignWithDirection.
 * Specification: tests/normals_ref.py.  All arithmetic is fp64, one rounding per operation written
 * here, d2 as above.
 * Neighbours of i: every j in [0, n), j = i included, in the order (d2(i, j), j); the first
 * min(max_nn, n) of them, and of those the ones with d2 < radius*radius (strict) — m_i points.
 * radius = +inf is the plain k-NN search.  Equal d2 at the cut go to the lower index (Open3D leaves
 * it unspecified).
 * Covariance (utility::ComputeCovariance): the cumulants x, y, z, xx, xy, xz, yy, yz, zz summed over
 * the neighbours in that order (cum = cum + term, term one product of raw coordinates), each
 * divided by (double)m_i; C00 = c3 - c0*c0, C01 = c4 - c0*c1, C02 = c5 - c0*c2, C11 = c6 - c1*c1,
 * C12 = c7 - c1*c2, C22 = c8 - c2*c2, symmetric.  m_i < 3: C = I.
 * Normal: (0, 0, 1) when m_i < 3 or C is all zeros; else the eigenvector of C's smallest eigenvalue
 * by a cyclic Jacobi solve: sweeps over the pairs (0,1), (0,2), (1,2); a pair with a_pq == 0 is
 * skipped, else th = (a_qq - a_pp) / (2*a_pq), t = 1 / (|th| + sqrt(th*th + 1)) negated when th <
 * 0, c = 1 / sqrt(t*t + 1), s = t*c, a_pp -= t*a_pq, a_qq += t*a_pq, a_pq = 0, a_rp' = c*a_rp -
 * s*a_rq, a_rq' = s*a_rp + c*a_rq for the third index r, and the columns p, q of V (from I) rotated
 * the same way; until the three off-diagonals are exactly 0, 10 sweeps at most.  The column of V
 * at the smallest diagonal entry (ties: the lowest index) divided by sqrt((x*x + y*y) + z*z).
 * has_prior != 0: normals holds a prior o_i on entry; an all-zero result becomes o_i, any other is
 * negated when ((n.x*o.x + n.y*o.y) + n.z*o.z) < 0.
 * The search walks fvo_statistical_outliers' grid (cell, max_rings: the time only, never a
 * result); a query is finished once the visited cube's nearest face is radius away, whatever it
 * holds, so a hybrid search with cell ~ radius leaves nothing to the brute-force pass.
 * workspace:   device scratch of fvo_normals_workspace_bytes(n_points, max_nn) bytes (caller-owned,
 *              8-byte aligned, needs no clearing between calls); -1 for a refused size.
 * normals:     device [n][3], written at every point (read first when has_prior).
 * covariances: device [n][9] (row-major 3x3) or NULL.  n_neighbors: device [n] (m_i) or NULL.
 * stats:       device int32[2]: queries finished by the brute-force pass, points with m_i < 3.
 * status (device, may be NULL): 0 ok, 1 = a cell index outside [0, 2^21) or a non-finite
 *              coordinate (every result invalid).
 * fvo_orient_normals: ref is a host double[3], read before the call returns.  mode 0: ref is the
 * camera location c, r_i = c - p_i; mode 1: ref is a direction, r_i = ref (not all zeros).  A normal
 * with all components 0 becomes r_i / sqrt((x*x + y*y) + z*z), or (0, 0, 1) when r_i is all zeros;
 * any other is negated when ((n.x*r.x + n.y*r.y) + n.z*r.z) < 0.
 * n_points == 0 returns 0 after the argument checks (stats is zeroed).  Nothing is allocated; the
 * calls are stream-ordered and can be captured into a hipGraph; their launches are not in the
 * fvo_timing_* table. */
#define FVO_NORMALS_MAX_NN 64
int64_t fvo_normals_workspace_bytes(int64_t n_points, int32_t max_nn);
int fvo_estimate_normals(fvo_ctx* ctx, const double* points, int64_t n_points, int32_t max_nn, double radius,
                         double cell, int32_t max_rings, void* workspace, int64_t workspace_bytes, double* normals,
                         int32_t has_prior, double* covariances, int32_t* n_neighbors, int32_t* stats,
                         int32_t* status, fvo_stream stream);
int fvo_orient_normals(fvo_ctx* ctx, const double* points, double* normals, int64_t n_points, int32_t mode,
                       const double* ref, fvo_stream stream);

/* Open3D pipelines::registration::RegistrationICP / EvaluateRegistration (0.17, restated; any stage,
 * no context workspace) of n_source fp64 xyz points onto n_target (device [n][3], not modified), and
 * PointCloud::Transform.  Specification: tests/icp_ref.py.  All arithmetic is fp64, one rounding per
 * operation written here.
 * Transform: s' = T s, always of the original source (Open3D transforms the cloud incrementally and
 * accumulates the roundings), x' = ((r00*x + r01*y) + r02*z) + t0 and likewise y', z'.
 * Correspondence of source i (KDTreeFlann::SearchHybrid(s', r, 1), r = max_correspondence_distance):
 * the target index j that minimises (d2(s'_i, t_j), j), d2 as above with dx = t.x - s'.x; kept iff d2 <
 * r*r (strict), else -1; equal d2 go to the lower index.  m kept: fitness = m / n_source, inlier_rmse =
 * sqrt(sum d2 / m), 0 when m = 0.
 * Sums: with the pivot c = the target's per-axis minimum, p = s' - c, q = t - c, n the target's normal:
 *   point-to-plane (1): d = p - q, r = ((d.x*n.x + d.y*n.y) + d.z*n.z), J = [p x n, n]; [0..20] the upper
 *     triangle of sum J J^T row by row, [21..26] sum J_a*r, [27] sum d2.  A x = -b by a 6x6 LDL^T (D_j =
 *     A_jj - sum_{k<j} (L_jk*L_jk)*D_k, L_ij = (A_ji - sum_{k<j} (L_ik*L_jk)*D_k) / D_j, y_i = rhs_i -
 *     sum_{k<i} L_ik*y_k, x_i = y_i / D_i - sum_{k>i} L_ki*x_k, every sum one subtraction per term in
 *     ascending k), x = (w, v); R = I + (2 / (1 + g.g)) (G + G G) with the Gibbs vector g = w / 2, G = [g]x,
 *     G G = g g^T - (g.g) I (Open3D composes Euler angles: the same to O(|w|^3), the same fixed point).
 *     A pivot that is not > 0 and finite, or m = 0: the identity update and status bit 2.
 *   point-to-point (0): [0..2] sum p, [3..5] sum q, [6..14] sum p_a*q_b row by row, [27] sum d2.  Horn's
 *     closed form (Open3D's Umeyama without scale): pm = sum p / m, qm = sum q / m, M_ab = sum p_a q_b / m
 *     - pm_a*qm_b, the symmetric 4x4 N(M) (N00 = (Mxx + Myy) + Mzz, N11 = (Mxx - Myy) - Mzz, N22 = (Myy -
 *     Mxx) - Mzz, N33 = (Mzz - Mxx) - Myy, N01 = Myz - Mzy, N02 = Mzx - Mxz, N03 = Mxy - Myx, N12 = Mxy +
 *     Myx, N13 = Mzx + Mxz, N23 = Myz + Mzy), the eigenvector of its largest diagonal entry (ties: the
 *     lowest index) after fvo_estimate_normals' cyclic Jacobi over the pairs (0,1), (0,2), (0,3), (1,2),
 *     (1,3), (2,3) until the six off-diagonals are exactly 0, 12 sweeps at most; the quaternion (w, x, y,
 *     z) divided by sqrt(((w*w + x*x) + y*y) + z*z), R from it, v = qm - R pm.  m = 0: as above.
 *   The update is x -> c + R (x - c) + v: U = [R | (v + c) - R c], T <- U T, bottom row (0, 0, 0, 1).
 *   The device sums the terms by a fixed tree (the same bits on every call); the specification's
 *   math.fsum differs from it by at most 2 m 2^-53 sum |term|.
 * Loop: evaluate at init; up to max_iteration times: update, evaluate, stop when |d fitness| <
 * relative_fitness and |d inlier_rmse| < relative_rmse.  max_iteration = 0 is evaluate_registration;
 * max_iteration + 1 passes of two launches are enqueued and skip themselves once the loop has stopped:
 * no host synchronisation.  The search walks fvo_radius_outliers' grid built on the target (cell: the
 * time only, never a result; max_correspondence_distance / cell > 8 is refused).
 * init:      host double[16], row-major, read before the call returns; finite, bottom row (0, 0, 0, 1).
 * target_normals: device [n_target][3], NULL unless estimation is 1.
 * workspace: device scratch of fvo_icp_workspace_bytes(n_source, n_target) bytes (caller-owned, 8-byte
 *            aligned, needs no clearing between calls); that function returns -1 for a refused size.
 * result:    device double[20]: T (row-major), fitness, inlier_rmse, the number of correspondences,
 *            iterations (the updates applied; an identity update counts).
 * sums:      device double[FVO_ICP_SUMS] or NULL: the last pass's 28 sums, m, and the T that entered it.
 * correspondences: device int32[n_source] or NULL, for the final T.
 * status (device, may be NULL): bit 1 = a target cell index outside [0, 2^21) or a non-finite
 *            coordinate (every result invalid), bit 2 = a degenerate system (identity update applied).
 * n_source == 0 or n_target == 0 (after the argument checks): result holds init, fitness 0, every
 * correspondence -1; no search is launched and workspace may be NULL.
 * fvo_transform_points: the transform expression above on points (device [n][3], in place); points32
 * (device float [n][3] or NULL) receives the float32 casts, normals (device [n][3] or NULL) are rotated
 * in place, ((r00*x + r01*y) + r02*z).  T: host double[16] as init.
 * Nothing is allocated; the calls are stream-ordered and can be captured into a hipGraph; their
 * launches are not in the fvo_timing_* table. */
#define FVO_ICP_MAX_ITERATION 1000
#define FVO_ICP_SUMS 45
int64_t fvo_icp_workspace_bytes(int64_t n_source, int64_t n_target);
int fvo_registration_icp(fvo_ctx* ctx, const double* source, int64_t n_source, const double* target,
                         const double* target_normals, int64_t n_target, double max_correspondence_distance,
                         double cell, const double* init, int32_t estimation, double relative_fitness,
                         double relative_rmse, int32_t max_iteration, void* workspace, int64_t workspace_bytes,
                         double* result, double* sums, int32_t* correspondences, int32_t* status,
                         fvo_stream stream);
int fvo_transform_points(fvo_ctx* ctx, double* points, float* points32, double* normals, int64_t n_points,
                         const double* T, fvo_stream stream);

/* cv2.filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on `batch` CV_16SC1 disparity maps, in
 * place (any stage; any image size, not tied to the context's).  Two 4-neighbours are connected
 * when both differ from new_val and |int(p) - int(q)| <= max_diff; every pixel of a connected
 * region of at most max_speckle_size pixels becomes new_val, every other pixel is untouched.
 * StereoSGBM::compute applies it after the median when speckleWindowSize > 0, as
 * (disp, (minDisparity - 1) * 16, speckleWindowSize, 16 * speckleRange).
 * disparity: image b at disparity + b*image_stride, rows `pitch` apart (both in int16 elements;
 *            pitch >= width, e.g. a column range of a wider map).  height*width <= INT32_MAX.
 * workspace: device scratch of fvo_speckle_workspace_bytes(batch, height, width) bytes (8 per
 *            pixel; caller-owned, 4-byte aligned, needs no clearing between calls); that function
 *            returns -1 for sizes the filter refuses.
 * Arguments are checked even when nothing is launched: batch == 0 (checked like every entry
 * point: before the pointers) and max_speckle_size <= 0 (nothing is a speckle) return 0. */
int64_t fvo_speckle_workspace_bytes(int32_t batch, int32_t height, int32_t width);
int fvo_filter_speckles(fvo_ctx* ctx, int16_t* disparity, int32_t batch, int32_t height, int32_t width,
                        int64_t image_stride, int32_t pitch, int32_t new_val, int32_t max_speckle_size,
                        int32_t max_diff, void* workspace, int64_t workspace_bytes, fvo_stream stream);

/* Dense stereo mapping (any stage; any image size, not tied to the context's): the disparity maps
 * of `batch` frames appended to the map as one world-frame point cloud, in a deterministic order.
 * Frame b samples the pixels (y, x) with y = 0, step, 2*step, ... < height and x likewise, in
 * row-major order; frames in batch order.  A sample's camera-frame point is fvo_backproject's
 * float32 arithmetic at the integer pixel: d = (float)d16 / 16.f (0 and -1 -> 0.1f),
 * Z = (float)(K[0]*baseline) / d, X = (((float)x - (float)cx) / (float)fx) * Z, Y likewise.  It is
 * kept iff d16 >= min_disp16 and z_min < Z < z_max (min_disp16 = -32768, z 0.1 / 1000: the
 * reference's filter exactly; min_disp16 = 1 drops SGBM's invalid pixels and zero disparities by
 * value).  The kept point goes through fvo_map_transform's fp64 expression with T[b] and is
 * appended from *map_count exactly as there: *map_count advances by the total (clamped at
 * INT32_MAX), points at positions >= map_cap are counted but not written.
 * disparity:  image b at disparity + b*image_stride, rows `pitch` apart (int16 elements, pitch >=
 *             width, as fvo_filter_speckles); not modified.  height*width <= INT32_MAX.
 * K:          host double[9] row-major; baseline in metres (both as fvo_backproject).
 * frame_keep: device [batch] int32 or NULL; 0 = frame b contributes nothing.
 * T:          device [batch][16] fp64 row-major.  map_count / map_cap / map_xyz64 / map_xyz32: as
 *             fvo_map_transform (one of the two arrays may be NULL).
 * n_added:    device [batch] int32 or NULL: kept samples of each frame.
 * workspace:  device scratch of fvo_dense_workspace_bytes(batch, height, width, step) bytes
 *             (caller-owned, 8-byte aligned, needs no clearing); that function returns -1 for sizes
 *             the call refuses.  With step 1, width % 4 == 0 and 8-byte aligned rows (pointer,
 *             pitch and image_stride) the disparities are read 8 bytes at a time.
 * Nothing is allocated; the call is stream-ordered and can be captured into a hipGraph.  Three
 * launches that are not in the fvo_timing_* table. */
int64_t fvo_dense_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t step);
int fvo_dense_map_append(fvo_ctx* ctx, const int16_t* disparity, int32_t batch, int32_t height, int32_t width,
                         int64_t image_stride, int32_t pitch, const double* K, double baseline, int32_t step,
                         int32_t min_disp16, float z_min, float z_max, const int32_t* frame_keep, const double* T,
                         int32_t* map_count, int64_t map_cap, double* map_xyz64, float* map_xyz32, int32_t* n_added,
                         void* workspace, int64_t workspace_bytes, fvo_stream stream);

/* cv2.reprojectImageTo3D(disparity, Q, handleMissingValues) on `batch` CV_16SC1 (is_float32 0) or
 * CV_32FC1 (is_float32 1) disparity images (any stage; any image size), OpenCV 4.x's Matx form in
 * fp64:  h_k = (((0 + Q[k][0] x) + Q[k][1] y) + Q[k][2] d) + Q[k][3],  out_k = (float)(h_k / h_3)
 * with d the RAW pixel value (cv2 does not divide int16 disparities by 16).  With
 * handle_missing_values != 0, z = 10000 where |d - min| <= FLT_EPSILON, min the image's minimum
 * (minMaxIdx), found by a pass of its own.
 * disparity: image b at disparity + b*image_stride, rows `pitch` apart (in elements).
 * Q:         host double[16] row-major.
 * min_key:   device [batch] uint32 scratch, needed (and written) only with handle_missing_values.
 * out:       [batch][height][width][3] f32. */
int fvo_reproject_to_3d(fvo_ctx* ctx, const void* disparity, int32_t is_float32, int32_t batch, int32_t height,
                        int32_t width, int64_t image_stride, int32_t pitch, const double* Q,
                        int32_t handle_missing_values, uint32_t* min_key, float* out, fvo_stream stream);

/* Sparse stereo (any stage; specification: tests/sparse_stereo_ref.py): the stereo point of every
 * left keypoint from a left-right ORB match on its own row band, refined to sub-pixel by a SAD
 * search on the level-0 images, as the per-keypoint record of fvo_keypoint_stereo -- without a
 * disparity map.  All float arithmetic is float32 in the order written here.
 * Right keypoint j is a candidate of left keypoint i iff both octaves (record field 5) are
 * integers in [0, n_levels), fabsf(yR - yL) <= row_tol * level_scale[oL], |oR - oL| <=
 * max_octave_diff and min_disparity <= xL - xR <= max_disparity.  The best candidate is the
 * minimum of (hamming << 16) | j, accepted iff hamming <= max_hamming (else status 1).  With
 * unique != 0, of the left keypoints whose accepted best candidate is j only the one with the
 * smallest (hamming << 16) | i keeps it (the others: status 2), before the refinement.
 * Refinement: xl = floorf(xL + 0.5f), yl and xr likewise; the (2w+1)^2 window around (xl, yl) and
 * the 2S+1 windows around (xr + k, yl), |k| <= S, must lie inside the image (else status 3);
 * SAD(k) over the window, k* its first minimum; k* = +-S: status 4; delta = (float)(d1 - d3) /
 * (float)(2 (d1 + d3 - 2 d2)) over SAD(k* - 1), SAD(k*), SAD(k* + 1); d = xL - ((float)(xr + k*) +
 * delta); d outside [min_disparity, max_disparity]: status 5; Z = (float)(K[0] baseline) / d with
 * X, Y as fvo_backproject at (xL, yL); 0.1 < Z < 1000 failing: status 6.
 * left/right:  u8 image b at + b*image_stride, rows `pitch` bytes apart, the context's size.
 * kpL/kpR:     [batch][cap][8] records, nL/nR [batch] counts (<= 0: empty, > cap: clamped),
 *              descL/descR [batch][cap][32] (16-byte aligned).  cap in [1, 65535].
 * level_scale: host float[n_levels], n_levels in [1, 32].  K: host double[9]; baseline in metres.
 * workspace:   device scratch of fvo_sparse_stereo_workspace_bytes(batch, cap) bytes (caller-owned,
 *              4-byte aligned, needs no clearing: the call's first kernel initialises it).
 * stereo:      [batch][cap][4] f32 (X, Y, Z, d), 16-byte aligned; zeros for every status != 0.
 * info:        [batch][cap][4] i32 or NULL: (right index, hamming, k*, status); right index and
 *              hamming are -1 under status 1, k* is 0 under statuses 1-3.
 * Rows >= the left count are not written.  Nothing is allocated; three launches that are not in
 * the fvo_timing_* table. */
typedef struct fvo_sparse_stereo_params {
  float min_disparity;     /* 1.0: finite, > 0 */
  float max_disparity;     /* 96.0: >= min_disparity */
  float row_tol;           /* 2.0: finite, >= 0 */
  int32_t max_hamming;     /* 75: [0, 256] */
  int32_t max_octave_diff; /* 1: >= 0 */
  int32_t half_window;     /* 5: w in [1, 7] */
  int32_t half_slide;      /* 5: S in [1, 8] */
  int32_t unique;          /* 1 */
} fvo_sparse_stereo_params;
void fvo_sparse_stereo_params_default(fvo_sparse_stereo_params* params);
int64_t fvo_sparse_stereo_workspace_bytes(int32_t batch, int32_t cap);
int fvo_sparse_stereo(fvo_ctx* ctx, const uint8_t* left, const uint8_t* right, int32_t batch, int64_t image_stride,
                      int32_t pitch, const float* kpL, const int32_t* nL, const uint8_t* descL, const float* kpR,
                      const int32_t* nR, const uint8_t* descR, int32_t cap, const fvo_sparse_stereo_params* params,
                      const float* level_scale, int32_t n_levels, const double* K, double baseline, void* workspace,
                      int64_t workspace_bytes, float* stereo, int32_t* info, fvo_stream stream);

/* fvo_backproject with the depth taken from the stereo record (fvo_sparse_stereo or
 * fvo_keypoint_stereo, [batch][cap][4]) of the match's query keypoint: a match is kept iff the
 * record's Z != 0, points3d = its (X, Y, Z), compacted in match order; nothing is written past
 * n_points.  kp0 is not read (the record holds the point; the argument keeps fvo_backproject's
 * shape) and may be NULL.  Any stage. */
int fvo_backproject_stereo(fvo_ctx* ctx, const float* stereo, const float* kp0, const float* kp1,
                           const int32_t* matches, const int32_t* n_matches, int32_t batch, int32_t cap,
                           float* points3d, float* points2d, int32_t* n_points, fvo_stream stream);

/* Test hook: KeyPointsFilter::retainBest on `n` float responses (device memory) with the
 * product's selection kernel.  idx_out [n] receives the surviving original indices in
 * OpenCV's output order, *n_out the survivor count.  Allocates (stream-ordered). */
int fvo_test_retain_best(fvo_ctx* ctx, const float* keys, int32_t n, int32_t keep, int32_t* idx_out, int32_t* n_out,
                         fvo_stream stream);

/* Per-kernel timing with HIP events recorded on the launch stream (measurement hooks for
 * bench.py).  mask: bit i brackets every launch of kernel i (0..fvo_kernel_count()-1,
 * names from fvo_kernel_name()).  fvo_timing_read synchronises on the recorded events,
 * writes the summed milliseconds and launch counts per kernel (arrays of
 * fvo_kernel_count() entries) and clears the record. */
int fvo_kernel_count(void);
const char* fvo_kernel_name(int id);
int fvo_timing_enable(fvo_ctx* ctx, uint64_t mask);
int fvo_timing_read(fvo_ctx* ctx, double* ms, int32_t* launches);

/* Debug hook: device pointer and byte size of an internal buffer of the most recent ORB
 * call (0 pyramid, 1 blurred pyramid, 2 FAST score map, 3/4/5 per-level counts before /
 * after the two retainBest passes, 6/7 PnP RANSAC per-iteration inlier counts / hypotheses of the
 * last fvo_pnp_ransac, 8 its per-frame RANSAC state: int32 best count, iteration bound, best
 * iteration, points, 9 the SGBM control words: u32 ticket, generation, L-path hand-off timeouts
 * (must stay 0), reserved, then one failure flag per pair, 11 the disparity of the last fvo_sgbm
 * before its median filter, int16 [pairs of the last chunk][height][width]).  For stage-by-stage
 * parity tests only. */
int fvo_debug_buffer(fvo_ctx* ctx, int which, void** ptr, int64_t* bytes);
/* The first `bytes` bytes (<= the size fvo_debug_buffer reports) of that buffer copied to host
 * memory, after synchronising the context's device.  A HIP error is reported by fvo_last_error. */
int fvo_debug_copy(fvo_ctx* ctx, int which, void* host_dst, int64_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* FVO_H_ */
