// Argument / config validation of libfvo's C ABI (csrc/capi.cpp) exercised on the host under
// AddressSanitizer + UndefinedBehaviorSanitizer (tools/sanitize.sh, SURVEY.md §5 "Race
// detection / sanitizers").  Linked against tests/sanitize/host_stubs.cpp instead of the device
// layer: every entry point is called with good arguments (the stub launcher must be reached)
// and with each class of bad argument the boundary rejects (status < 0, fvo_last_error set,
// no launch).  Exit status 0 = all checks passed.
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "host_stubs.h"

static int g_fail = 0, g_checks = 0;

#define CHECK(cond)                                                       \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      ++g_fail;                                                           \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                     \
  } while (0)

// rc must be < 0 with an error message and no launcher reached
static void rejected(fvo_ctx* c, int rc) {
  CHECK(rc < 0);
  CHECK(std::strlen(fvo_last_error(c)) > 0);
  CHECK(g_last_launch.empty());
}

static void reached(int rc, const char* launcher) {
  CHECK(rc == 0);
  CHECK(g_last_launch == launcher);
}

// as rejected(), with exactly this message
static void refused(fvo_ctx* c, int rc, const char* msg) {
  CHECK(rc < 0);
  CHECK(std::strcmp(fvo_last_error(c), msg) == 0);
  CHECK(g_last_launch.empty());
}

// fvo_create must refuse cfg saying exactly "fvo_create: <msg>" on stderr, before any init, and
// leave nothing allocated
static void create_refused(const fvo_config& cfg, const char* msg) {
  char said[512] = {0};
  fvo_ctx* c = reinterpret_cast<fvo_ctx*>(said);  // must come back null
  int fds[2] = {-1, -1};
  g_last_launch.clear();
  std::fflush(stderr);
  const int saved = dup(2);
  CHECK(pipe(fds) == 0 && dup2(fds[1], 2) == 2);
  const int rc = fvo_create(0, &cfg, &c);
  std::fflush(stderr);
  dup2(saved, 2);
  close(saved);
  close(fds[1]);
  const long n = read(fds[0], said, sizeof(said) - 1);
  close(fds[0]);
  CHECK(rc < 0 && c == nullptr);
  CHECK(n > 0 && std::string(said) == std::string("fvo_create: ") + msg + "\n");
  if (std::string(said) != std::string("fvo_create: ") + msg + "\n") std::fprintf(stderr, "  said: %s", said);
  CHECK(g_last_launch.empty());
  CHECK(g_live_allocs == 0);
}

// fvo_create must accept cfg, the stage init named last must have run, and fvo_destroy frees everything
static void create_reached(const fvo_config& cfg, const char* last_init) {
  fvo_ctx* c = nullptr;
  g_last_launch.clear();
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  CHECK(g_last_launch == last_init);
  CHECK(g_live_allocs > 0);
  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
}

static fvo_config stage_config(int stages, int width = 960, int height = 600) {
  fvo_config cfg;
  fvo_config_default(&cfg, width, height);
  cfg.stages = stages;
  cfg.kp_capacity = 64;
  return cfg;
}

// ---- every config refusal of fvo_create by its message, and the accepted bound next to it
static void config_checks() {
  fvo_config k = stage_config(FVO_STAGE_ORB), b;
  const char* orb_only = "only firstLevel=0, WTA_K=2, HARRIS_SCORE, patchSize=31 are supported";
  b = k; b.nlevels = 0; create_refused(b, "nlevels out of range");
  b = k; b.nlevels = 13; create_refused(b, "nlevels out of range");
  b = k; b.nlevels = 1; create_reached(b, "orb_init");
  b = k; b.nlevels = 12; create_reached(b, "orb_init");
  b = k; b.first_level = 1; create_refused(b, orb_only);
  b = k; b.wta_k = 3; create_refused(b, orb_only);
  b = k; b.score_type = 1; create_refused(b, orb_only);
  b = k; b.patch_size = 29; create_refused(b, orb_only);
  b = k; b.width = 4096; create_refused(b, "image dimensions must be < 4096");
  b = k; b.height = 4096; create_refused(b, "image dimensions must be < 4096");
  b = k; b.width = b.height = 4095; create_reached(b, "orb_init");
  b = k; b.edge_threshold = 14; create_refused(b, "edgeThreshold must be >= patchSize/2 (15)");
  b = k; b.edge_threshold = 15; create_reached(b, "orb_init");

  k = stage_config(FVO_STAGE_BF);
  b = k; b.kp_capacity = 65536; create_refused(b, "BF: kp_capacity must be <= 65535 (16-bit indices in the keys)");
  b = k; b.kp_capacity = 65535; create_reached(b, "bf_init");

  k = stage_config(FVO_STAGE_SGBM);
  const char* shapes = "SGBM: (sgbm_lanes, sgbm_cols) must be (4, 32|64), (8, 16|32) or (16, 32)";
  b = k; b.block_size = 5; create_refused(b, "SGBM: only blockSize=7 is supported");
  b = k; b.num_disparities = 80; create_refused(b, "SGBM: numDisparities must be 64, 96 or 128");
  for (int d : {64, 96, 128}) { b = k; b.num_disparities = d; create_reached(b, "sgbm_init"); }
  b = k; b.uniqueness_ratio = 1; create_refused(b, "SGBM: only uniquenessRatio=0 is supported");
  b = k; b.sgbm_stripes = 0; create_refused(b, "SGBM: stripes must be >= 1");
  b = k; b.sgbm_stripes = 1; create_reached(b, "sgbm_init");
  b = k; b.sgbm_mode = 2; create_refused(b, "SGBM: sgbm_mode must be FVO_SGBM_CLASSIC or FVO_SGBM_LPATH");
  b = k; b.sgbm_lanes = 8; b.sgbm_cols = 64; create_refused(b, shapes);
  b = k; b.sgbm_lanes = 16; b.sgbm_cols = 16; create_refused(b, shapes);
  b = k; b.sgbm_lanes = 2; create_refused(b, shapes);
  const int ok_shapes[][2] = {{4, 32}, {4, 64}, {8, 16}, {8, 32}, {16, 32}, {4, 0}, {0, 16}};
  for (auto& s : ok_shapes) { b = k; b.sgbm_lanes = s[0]; b.sgbm_cols = s[1]; create_reached(b, "sgbm_init"); }
  b = k; b.sgbm_mode = FVO_SGBM_LPATH; b.sgbm_lanes = 8;
  create_refused(b, "SGBM: sgbm_lanes / sgbm_cols apply to the classic schedule only (leave them 0)");
  b = k; b.sgbm_mode = FVO_SGBM_LPATH; create_reached(b, "sgbm_init");
  b = k; b.sgbm_handoff_us = -2; create_refused(b, "SGBM: sgbm_handoff_us must be >= -1");
  b = k; b.sgbm_handoff_us = -1; create_reached(b, "sgbm_init");
  b = k; b.width = 96; create_refused(b, "SGBM: image narrower than numDisparities");
  b = k; b.width = 97; create_reached(b, "sgbm_init");
  b = k; b.min_disparity = -960; create_refused(b, "SGBM: image narrower than numDisparities");  // no column left of 960
  b = k; b.min_disparity = -959; create_reached(b, "sgbm_init");
  // the 16-bit bounds at pre_filter_cap 0: C = 49 (2 * 15 + 63) = 4557.  The aggregated cost
  // 3 (C + P2) <= 65535 allows P2 <= 17288; the path cost C + P2 + P1 <= 65535 is the weaker one
  // for every P1 < P2, so the last P2 it passes is still refused, by the aggregated-cost check
  const char* path16 = "SGBM: P1/P2/preFilterCap too large for 16-bit path costs";
  const char* sum16 = "SGBM: P2/preFilterCap too large for the 16-bit aggregated cost";
  b = k; b.P2 = 17288; create_reached(b, "sgbm_init");
  b = k; b.P2 = 17289; create_refused(b, sum16);
  b = k; b.P1 = 30000; b.P2 = 65535 - 4557 - 30000; create_refused(b, sum16);
  b = k; b.P1 = 30000; b.P2 = 65535 - 4557 - 30000 + 1; create_refused(b, path16);
  b = k; b.pre_filter_cap = 63; b.P2 = 12584; create_reached(b, "sgbm_init");  // C = 49 * 189 = 9261
  b = k; b.pre_filter_cap = 63; b.P2 = 12585; create_refused(b, sum16);
  // L path: 128 column blocks of 32 at width - numDisparities = 4065
  b = k; b.sgbm_mode = FVO_SGBM_LPATH; b.width = 4065 + 96;
  create_refused(b, "SGBM: FVO_SGBM_LPATH needs width - numDisparities <= 4064 (use the classic schedule)");
  b.width = 4064 + 96; create_reached(b, "sgbm_init");
  b.sgbm_mode = FVO_SGBM_CLASSIC; b.width = 4065 + 96; create_reached(b, "sgbm_init");

  k = stage_config(FVO_STAGE_BA);
  b = k; b.ba_window = 2; create_refused(b, "ba_window must be in [3, 21]");
  b = k; b.ba_window = 22; create_refused(b, "ba_window must be in [3, 21]");
  b = k; b.ba_window = 3; create_reached(b, "ba_init");
  b = k; b.ba_window = 21; create_reached(b, "ba_init");
  b = k; b.ba_max_landmarks = 0; create_refused(b, "bad BA landmark / observation caps");
  b = k; b.ba_max_obs = 1; create_refused(b, "bad BA landmark / observation caps");
  b = k; b.ba_max_landmarks = 1; b.ba_max_obs = 2; create_reached(b, "ba_init");

  // stage order: the first message is the earliest stage's, and no earlier stage was initialised
  b = stage_config(FVO_STAGE_ALL); b.ba_window = 2; b.block_size = 5; create_refused(b, "SGBM: only blockSize=7 is supported");
  b.nlevels = 13; create_refused(b, "nlevels out of range");
  b = stage_config(FVO_STAGE_POSE | FVO_STAGE_MONO); create_reached(b, "mono_init");
}

// ---- the calibration refusals of fvo_undistort_gray by their messages, and every lens case of
// tests/ingest_cases.py accepted, on a context of W x H
static void lens_checks(fvo_ctx* c, int W, int H) {
  static uint8_t img[8];  // the stub launcher never dereferences it
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  auto call = [&](const double* K, const double* d) {
    g_last_launch.clear();
    return fvo_undistort_gray(c, img, 1, (int64_t)3 * W * H, 3 * W, K, d, img, (int64_t)W * H, W, nullptr);
  };
  const char* finite = "undistort_gray: K and dist must be finite";
  const char* singular = "undistort_gray: K is singular (a stripe's camera matrix has det == 0)";
  const char* horizon = "undistort_gray: _w <= 0 at a stripe corner (the view reaches the camera's horizon)";
  const double Kc[9] = {70, 0, 48.3, 0, 69, 37.6, 0, 0, 1}, Kskew[9] = {70, 0.8, 48.3, 0, 69, 37.6, 0, 0, 1};
  const double K8[9] = {140, 0, 96.6, 0, 138, 75.2, 0, 0, 2};
  const double Kpersp[9] = {70, 0.8, 48.3, 0.3, 69, 37.6, 2e-4, -3e-4, 1};
  const double tang[5] = {-0.2, 0.05, 0.01, -0.02, 0.03}, pin[5] = {0.4, 0.1, 0.003, 0.002, 0.05};
  const double dpersp[5] = {0.1, 0.05, 0.01, -0.02, 0.03}, sat[5] = {1e7, 0, 0, 0, 0};
  reached(call(Kc, tang), "ingest_run");
  reached(call(Kc, pin), "ingest_run");
  reached(call(Kskew, tang), "ingest_run");
  reached(call(K8, tang), "ingest_run");
  reached(call(Kpersp, dpersp), "ingest_run");
  reached(call(Kc, sat), "ingest_run");  // finite, and only large
  double K[9], d[5];
  std::memcpy(K, Kc, sizeof(K)); K[0] = 0; refused(c, call(K, tang), singular);
  std::memcpy(K, Kc, sizeof(K)); K[8] = 0; refused(c, call(K, tang), singular);
  // _w changes sign across the width: with K[6] = 2 it runs from -2.7 at column 0 to +2.1 at column
  // 63 (4.9 at column 99, 72 at column 959).  K[6] = -0.02 does not do that: _w stays inside
  // [0.986, 1.26] up to 960x600, a lens the rule accepts.
  std::memcpy(K, Kpersp, sizeof(K)); K[6] = 2.0; refused(c, call(K, dpersp), horizon);
  std::memcpy(K, Kpersp, sizeof(K)); K[6] = -0.02; reached(call(K, dpersp), "ingest_run");
  std::memcpy(K, Kc, sizeof(K)); K[8] = -1; refused(c, call(K, tang), horizon);           // _w < 0 everywhere
  for (int i = 0; i < 5; ++i) {
    std::memcpy(d, tang, sizeof(d)); d[i] = nan; refused(c, call(Kc, d), finite);
    std::memcpy(d, tang, sizeof(d)); d[i] = -inf; refused(c, call(Kc, d), finite);
  }
  for (int i = 0; i < 9; ++i) {
    std::memcpy(K, Kc, sizeof(K)); K[i] = inf; refused(c, call(K, tang), finite);
    std::memcpy(K, Kc, sizeof(K)); K[i] = nan; refused(c, call(K, tang), finite);
  }
  // the rule holds per stripe: with K[7] = -1 the determinant 70 * (69 + (K[5] - y0)) vanishes in the
  // stripe that starts at row y0 = K[5] + 69 and nowhere else
  const int stripe = 4096 / W < 1 ? 1 : (4096 / W > H ? H : 4096 / W);
  if (stripe < H) {
    const double Kstripe[9] = {70, 0, 48.3, 0, 69, (double)stripe - 69, 0, -1, 1};
    refused(c, call(Kstripe, tang), singular);
  }
  if (stripe < H && 2 * stripe >= H) {  // two stripes: the determinant is > 0 in both and zero at row stripe + 1
    const double Kbetween[9] = {70, 0, 48.3, 0, 69, (double)stripe - 68, 0, -1, 1};
    reached(call(Kbetween, tang), "ingest_run");
  }
}

int main() {
  // ---- config
  fvo_config cfg;
  fvo_config_default(&cfg, 960, 600);
  CHECK(fvo_config_size() == (int32_t)sizeof(fvo_config));
  CHECK(cfg.nfeatures == 500 && cfg.num_disparities == 96 && cfg.P1 == 392 && cfg.P2 == 1568);
  const char* fields[] = {"width", "height", "max_batch", "nfeatures", "scale_factor", "nlevels", "edge_threshold",
                          "first_level", "wta_k", "score_type", "patch_size", "fast_threshold", "min_disparity",
                          "num_disparities", "block_size", "P1", "P2", "disp12_max_diff", "pre_filter_cap",
                          "uniqueness_ratio", "sgbm_stripes", "kp_capacity", "stages", "ba_window",
                          "ba_max_landmarks", "ba_max_obs", "sgbm_max_batch", "sgbm_mode", "sgbm_lanes",
                          "sgbm_cols", "sgbm_handoff_us"};
  for (size_t i = 0; i < sizeof(fields) / sizeof(fields[0]); ++i) CHECK(fvo_config_offset(fields[i]) == (int32_t)(4 * i));
  CHECK(fvo_config_offset("nope") == -1 && fvo_config_offset(nullptr) == -1);
  CHECK(fvo_abi_version() == FVO_ABI_VERSION);

  // ---- context creation
  fvo_ctx* c = nullptr;
  CHECK(fvo_create(0, nullptr, &c) < 0 && c == nullptr);
  CHECK(fvo_create(0, &cfg, nullptr) < 0);
  fvo_config bad = cfg;
  bad.max_batch = 0;
  CHECK(fvo_create(0, &bad, &c) < 0 && c == nullptr);
  bad = cfg;
  bad.width = 32;
  CHECK(fvo_create(0, &bad, &c) < 0);
  bad = cfg;
  bad.stages = 1 << 12;
  CHECK(fvo_create(0, &bad, &c) < 0);
  bad = cfg;
  bad.stages = FVO_STAGE_BF;  // no ORB stage and no kp_capacity
  CHECK(fvo_create(0, &bad, &c) < 0);
  bad = cfg;
  bad.block_size = 5;  // refused by the SGBM stage init: the context is released cleanly
  CHECK(fvo_create(0, &bad, &c) < 0 && c == nullptr);
  CHECK(fvo_create(99, &cfg, &c) < 0);
  CHECK(g_live_allocs == 0);  // every refused create released what it had
  config_checks();
  cfg.max_batch = 4;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  CHECK(g_live_allocs == 6);  // one per stage init of the stub layer
  CHECK(fvo_kp_capacity(c) == 2 * 500 + 64 && fvo_kp_capacity(nullptr) == 0);
  CHECK(std::strcmp(fvo_last_error(nullptr), "null context") == 0);

  // host stand-ins for device buffers (the stubs never dereference them)
  static uint8_t u8[1 << 16];
  static int32_t i32[1 << 12];
  static float f32[1 << 12];
  static double f64[1 << 12];
  static int16_t i16[1 << 12];
  const int cap = fvo_kp_capacity(c), W = 960, H = 600;
  auto reset = [] { g_last_launch.clear(); };

  // ---- ORB
  reset(); rejected(c, fvo_orb_detect_compute(c, nullptr, 1, W * H, W, f32, u8, i32, cap, nullptr));
  reset(); rejected(c, fvo_orb_detect_compute(c, u8, 5, W * H, W, f32, u8, i32, cap, nullptr));
  reset(); rejected(c, fvo_orb_detect_compute(c, u8, -1, W * H, W, f32, u8, i32, cap, nullptr));
  reset(); rejected(c, fvo_orb_detect_compute(c, u8, 1, W * H, W - 1, f32, u8, i32, cap, nullptr));
  reset(); rejected(c, fvo_orb_detect_compute(c, u8, 1, W * H - 1, W, f32, u8, i32, cap, nullptr));
  reset(); rejected(c, fvo_orb_detect_compute(c, u8, 1, W * H, W, f32, u8, i32, 0, nullptr));
  reset(); CHECK(fvo_orb_detect_compute(c, u8, 0, W * H, W, f32, u8, i32, cap, nullptr) == 0 && g_last_launch.empty());
  reset(); reached(fvo_orb_detect_compute(c, u8, 4, W * H, W, f32, u8, i32, cap, nullptr), "orb_run");
  CHECK(fvo_orb_detect_compute(nullptr, u8, 1, W * H, W, f32, u8, i32, cap, nullptr) < 0);

  // ---- BF
  reset(); rejected(c, fvo_bf_match(c, u8, i32, nullptr, i32, 1, cap, i32, i32, nullptr));
  reset(); rejected(c, fvo_bf_match(c, u8, i32, u8, i32, 1, cap + 1, i32, i32, nullptr));
  reset(); rejected(c, fvo_bf_match(c, u8, i32, u8, i32, 1, 0, i32, i32, nullptr));
  reset(); reached(fvo_bf_match(c, u8, i32, u8, i32, 2, cap, i32, i32, nullptr), "bf_run");
  reset(); refused(c, fvo_bf_match(c, u8 + 1, i32, u8, i32, 1, cap, i32, i32, nullptr),
                   "descriptor buffers must be 16-byte aligned");
  reset(); refused(c, fvo_bf_match(c, u8, i32, u8 + 8, i32, 1, cap, i32, i32, nullptr),
                   "descriptor buffers must be 16-byte aligned");
  reset(); reached(fvo_bf_match(c, u8 + 16, i32, u8 + 32, i32, 1, cap, i32, i32, nullptr), "bf_run");

  // ---- SGBM
  reset(); rejected(c, fvo_sgbm(c, u8, nullptr, 1, W * H, W, i16, nullptr, nullptr));
  reset(); rejected(c, fvo_sgbm(c, u8, u8, 1, W * H, W - 8, i16, nullptr, nullptr));
  reset(); rejected(c, fvo_sgbm(c, u8, u8, 9, W * H, W, i16, nullptr, nullptr));
  reset(); reached(fvo_sgbm(c, u8, u8, 4, W * H, W, i16, nullptr, nullptr), "sgbm_run");

  // ---- back-projection / PnP
  reset(); rejected(c, fvo_backproject(c, i16, f32, f32, i32, i32, 1, cap, nullptr, 0.25, f32, f32, i32, nullptr));
  reset(); rejected(c, fvo_backproject(c, i16, f32, f32, i32, i32, 1, 0, f64, 0.25, f32, f32, i32, nullptr));
  reset(); reached(fvo_backproject(c, i16, f32, f32, i32, i32, 1, cap, f64, 0.25, f32, f32, i32, nullptr),
                   "backproject_run");
  reset(); rejected(c, fvo_pnp_ransac(c, f32, f32, i32, 1, cap, f64, f64, 1.f, 0.99, 0, f64, f64, f64, i32, u8, nullptr));
  reset(); rejected(c, fvo_pnp_ransac(c, f32, f32, i32, 1, cap, f64, f64, 1.f, 0.99, 1001, f64, f64, f64, i32, u8,
                                      nullptr));
  reset(); rejected(c, fvo_pnp_ransac(c, f32, f32, i32, 1, cap, f64, f64, 1.f, 1.0, 1000, f64, f64, f64, i32, u8,
                                      nullptr));
  reset(); rejected(c, fvo_pnp_ransac(c, f32, f32, i32, 1, cap, f64, nullptr, 1.f, 0.99, 1000, f64, f64, f64, i32, u8,
                                      nullptr));
  reset(); reached(fvo_pnp_ransac(c, f32, f32, i32, 1, cap, f64, f64, 1.f, 0.99, 1000, f64, f64, f64, i32, u8, nullptr),
                   "pnp_run");
  reset(); refused(c, fvo_pnp_ransac(c, f32, f32, i32, 1, cap, f64, f64, 1.f, 0.99, 1001, f64, f64, f64, i32, u8,
                                     nullptr), "iterations out of range");
  reset(); refused(c, fvo_pnp_ransac(c, f32, f32, i32, 1, cap + 1, f64, f64, 1.f, 0.99, 1000, f64, f64, f64, i32, u8,
                                     nullptr), "pnp: cap exceeds the context keypoint capacity");
  reset(); reached(fvo_pnp_ransac(c, f32, f32, i32, 1, 1, f64, f64, 1.f, 0.99, 1, f64, f64, f64, i32, u8, nullptr),
                   "pnp_run");

  // ---- BA
  float* unaligned = reinterpret_cast<float*>(reinterpret_cast<char*>(f32) + 4);
  reset(); rejected(c, fvo_keypoint_stereo(c, i16, f32, i32, 1, cap, f64, 0.25, unaligned, nullptr));
  reset(); rejected(c, fvo_keypoint_stereo(c, i16, f32, i32, 1, cap + 1, f64, 0.25, f32, nullptr));
  reset(); reached(fvo_keypoint_stereo(c, i16, f32, i32, 1, cap, f64, 0.25, f32, nullptr), "ba_stereo_run");
  reset(); rejected(c, fvo_ba_windows(c, f32, i32, i32, i32, f32, f64, 12, cap, 9, 5, 0, f64, 0.25, f64, 8, 10, f64,
                                      f64, nullptr));  // n_windows > max_batch
  reset(); rejected(c, fvo_ba_windows(c, f32, i32, i32, i32, f32, f64, 12, cap, 9, 2, 0, f64, 0.25, nullptr, 8, 10,
                                      f64, f64, nullptr));
  reset(); reached(fvo_ba_windows(c, f32, i32, i32, i32, f32, f64, 12, cap, 9, 2, 0, f64, 0.25, f64, 8, 10, f64, f64,
                                  nullptr), "ba_run");
  reset(); rejected(c, fvo_ba_count_births(c, nullptr, i32, f32, 12, cap, 9, 2, 0, nullptr));
  reset(); rejected(c, fvo_ba_count_births(c, i32, i32, unaligned, 12, cap, 9, 2, 0, nullptr));
  reset(); rejected(c, fvo_ba_count_births(c, i32, i32, f32, 12, cap, 9, 5, 0, nullptr));  // n_windows > max_batch
  reset(); reached(fvo_ba_count_births(c, i32, i32, f32, 12, cap, 9, 2, 0, nullptr), "ba_births_run");
  reset(); rejected(c, fvo_ba_landmarks(c, 0, nullptr, i32, nullptr));
  reset(); reached(fvo_ba_landmarks(c, 0, f64, i32, nullptr), "ba_export_run");
  reset(); refused(c, fvo_ba_landmarks(c, -1, f64, i32, nullptr), "ba: window index out of range");
  reset(); refused(c, fvo_ba_landmarks(c, 4, f64, i32, nullptr), "ba: window index out of range");  // = max_batch
  reset(); reached(fvo_ba_landmarks(c, 3, f64, i32, nullptr), "ba_export_run");
  {  // the window range, one helper for both entry points: (n_frames 12) cap, first_end, n_windows, first_valid
    auto windows = [&](int cp, int fe, int nw, int fv, int nlev = 8, int iters = 10) {
      reset();
      return fvo_ba_windows(c, f32, i32, i32, i32, f32, f64, 12, cp, fe, nw, fv, f64, 0.25, f64, nlev, iters, f64, f64,
                            nullptr);
    };
    auto births = [&](int cp, int fe, int nw, int fv) {
      reset();
      return fvo_ba_count_births(c, i32, i32, f32, 12, cp, fe, nw, fv, nullptr);
    };
    const char* range = "ba: windows exceed the frame range";
    refused(c, windows(cap - 1, 9, 2, 0), "ba: cap must equal the context keypoint capacity");
    refused(c, births(cap - 1, 9, 2, 0), "ba: cap must equal the context keypoint capacity");
    refused(c, windows(cap, 0, 2, 0), range);
    refused(c, births(cap, 0, 2, 0), range);
    refused(c, windows(cap, 11, 2, 0), range);
    refused(c, births(cap, 11, 2, 0), range);
    reached(windows(cap, 10, 2, 0), "ba_run");  // first_end + n_windows = n_frames
    reached(births(cap, 10, 2, 0), "ba_births_run");
    reached(windows(cap, 1, 4, 0), "ba_run");   // first_end 1, n_windows = max_batch
    reached(births(cap, 1, 4, 0), "ba_births_run");
    refused(c, windows(cap, 9, 2, -1), "ba: first_valid out of range");
    refused(c, births(cap, 9, 2, -1), "ba: first_valid out of range");
    refused(c, windows(cap, 9, 2, 9), "ba: first_valid out of range");
    refused(c, births(cap, 9, 2, 9), "ba: first_valid out of range");
    reached(windows(cap, 9, 2, 8), "ba_run");
    reached(births(cap, 9, 2, 8), "ba_births_run");
    refused(c, windows(cap, 9, 2, 0, 0), "ba: bad level count");
    refused(c, windows(cap, 9, 2, 0, 13), "ba: bad level count");
    reached(windows(cap, 9, 2, 0, 1), "ba_run");
    reached(windows(cap, 9, 2, 0, 12), "ba_run");
    refused(c, windows(cap, 9, 2, 0, 8, -1), "ba: iterations out of range");
    refused(c, windows(cap, 9, 2, 0, 8, 101), "ba: iterations out of range");
    reached(windows(cap, 9, 2, 0, 8, 0), "ba_run");
    reached(windows(cap, 9, 2, 0, 8, 100), "ba_run");
  }

  // ---- mono
  reset(); rejected(c, fvo_gather_matches(c, f32, f32, i32, i32, 5, cap, f32, f32, i32, nullptr));
  reset(); reached(fvo_gather_matches(c, f32, f32, i32, i32, 2, cap, f32, f32, i32, nullptr), "gather_run");
  reset(); rejected(c, fvo_find_essential(c, f32, f32, i32, 1, cap, 0.0, 480, 300, 0.999, 1.0, 1000, f64, u8, i32,
                                          nullptr));
  reset(); rejected(c, fvo_find_essential(c, f32, f32, i32, 1, cap + 1, 640, 480, 300, 0.999, 1.0, 1000, f64, u8, i32,
                                          nullptr));
  reset(); reached(fvo_find_essential(c, f32, f32, i32, 1, cap, 640, 480, 300, 0.999, 1.0, 1000, f64, u8, i32, nullptr),
                   "essential_run");
  for (int it : {0, -1, 1001}) {
    reset(); refused(c, fvo_find_essential(c, f32, f32, i32, 1, cap, 640, 480, 300, 0.999, 1.0, it, f64, u8, i32, nullptr),
                     "essential: max_iters out of range");
  }
  reset(); reached(fvo_find_essential(c, f32, f32, i32, 1, cap, 640, 480, 300, 0.999, 1.0, 1, f64, u8, i32, nullptr),
                   "essential_run");
  reset(); rejected(c, fvo_recover_pose(c, f64, i32, f32, f32, i32, 1, cap, 640, 480, 300, 50, nullptr, f64, f64, i32,
                                        nullptr));
  reset(); reached(fvo_recover_pose(c, f64, i32, f32, f32, i32, 1, cap, 640, 480, 300, 50, f64, f64, f64, i32, nullptr),
                   "recover_run");

  // ---- ingest / blur
  const double Kc[9] = {70, 0, 48.3, 0, 69, 37.6, 0, 0, 1}, tang[5] = {-0.2, 0.05, 0.01, -0.02, 0.03};
  reset(); rejected(c, fvo_undistort_gray(c, u8, 1, 3 * W * H, 3 * W - 1, Kc, tang, u8, W * H, W, nullptr));
  reset(); reached(fvo_undistort_gray(c, u8, 1, 3 * W * H, 3 * W, Kc, tang, u8, W * H, W, nullptr), "ingest_run");
  lens_checks(c, W, H);
  reset(); rejected(c, fvo_motion_blur(c, u8, 1, W * H, W, 10, 0.5, i32, i32, 16, u8, u8 + 8, W * H, W, nullptr));
  reset(); rejected(c, fvo_motion_blur(c, u8, 1, W * H, W, 32, 0.0, i32, i32, 16, u8, u8 + 8, W * H, W, nullptr));
  reset(); rejected(c, fvo_motion_blur(c, u8, 1, W * H, W, 10, 0.0, i32, i32, 16, u8, u8, W * H, W, nullptr));
  reset(); reached(fvo_motion_blur(c, u8, 1, W * H, W, 10, 0.0, i32, i32, 16, u8, u8 + 8, W * H, W, nullptr),
                   "motion_blur_run");
  for (int off : {1, 2, 3}) {  // the mask is rewritten a dword at a time when there are seeds
    reset(); refused(c, fvo_motion_blur(c, u8, 1, W * H, W, 10, 0.0, i32, i32, 16, u8 + 16 + off, u8 + 8, W * H, W, nullptr),
                     "motion blur: mask must be 4-byte aligned");
  }
  reset(); reached(fvo_motion_blur(c, u8, 1, W * H, W, 10, 0.0, i32, i32, 16, u8 + 4, u8 + 8, W * H, W, nullptr),
                   "motion_blur_run");
  reset(); reached(fvo_motion_blur(c, u8, 1, W * H, W, 10, 0.0, nullptr, nullptr, 0, u8 + 1, u8 + 8, W * H, W, nullptr),
                   "motion_blur_run");  // no seeds: any mask

  // ---- map
  reset(); rejected(c, fvo_map_transform(c, f32, 2, i32, 1, cap, f64, i32, 100, f64, f32, nullptr));
  reset(); rejected(c, fvo_map_transform(c, f32, 3, i32, 1, cap, f64, i32, 100, nullptr, nullptr, nullptr));
  reset(); reached(fvo_map_transform(c, f32, 3, i32, 1, cap, f64, i32, 100, f64, nullptr, nullptr), "map_transform_run");
  reset(); rejected(c, fvo_chain_poses(c, f64, i32, i32, 2, 3, f64, f64, nullptr, nullptr));
  reset(); rejected(c, fvo_chain_poses(c, f64, nullptr, nullptr, 2, 3, f64, f64, nullptr, nullptr));
  reset(); rejected(c, fvo_chain_poses(c, f64, i32, nullptr, -1, 3, f64, f64, nullptr, nullptr));
  reset(); CHECK(fvo_chain_poses(c, f64, i32, nullptr, 0, 3, f64, f64, nullptr, nullptr) == 0 && g_last_launch.empty());
  reset(); reached(fvo_chain_poses(c, f64, i32, i32, 2, 3, f64, f64, i32, nullptr), "chain_poses_run");
  {  // step bookkeeping: region count / overlap validation, count guard ranges
    static char buf[4096];
    fvo_region r[FVO_MAX_REGIONS + 1];
    for (int i = 0; i <= FVO_MAX_REGIONS; ++i) r[i] = fvo_region{buf + 64 * i, buf + 3000, 16};
    reset(); rejected(c, fvo_copy_regions(c, FVO_MAX_REGIONS + 1, r, nullptr));
    reset(); rejected(c, fvo_copy_regions(c, 2, nullptr, nullptr));
    reset(); CHECK(fvo_copy_regions(c, 0, nullptr, nullptr) == 0 && g_last_launch.empty());
    reset(); reached(fvo_copy_regions(c, 2, r, nullptr), "copy_regions_run");
    fvo_region ov[2] = {{buf, buf + 8, 16}, {buf + 100, buf + 200, 16}};  // own source overlaps
    reset(); rejected(c, fvo_copy_regions(c, 2, ov, nullptr));
    fvo_region dd[2] = {{buf, buf + 1000, 16}, {buf + 8, buf + 2000, 16}};  // destinations overlap
    reset(); rejected(c, fvo_copy_regions(c, 2, dd, nullptr));
    fvo_region xs[2] = {{buf, buf + 1000, 16}, {buf + 1000, buf + 2000, 16}};  // dst 0 = src 0? no: dst 1 = src 0
    reset(); rejected(c, fvo_copy_regions(c, 2, xs, nullptr));
    fvo_region nb[1] = {{buf, buf + 100, -1}};
    reset(); rejected(c, fvo_copy_regions(c, 1, nb, nullptr));
    fvo_region z[1] = {{nullptr, nullptr, 0}};  // empty regions are skipped
    reset(); CHECK(fvo_copy_regions(c, 1, z, nullptr) == 0 && g_last_launch.empty());
    reset(); rejected(c, fvo_count_guard(c, i32, i32, 4, 0, i32, -3, nullptr, nullptr));
    reset(); rejected(c, fvo_count_guard(c, nullptr, i32, 4, 1, i32, -3, nullptr, nullptr));
    reset(); CHECK(fvo_count_guard(c, i32, nullptr, 0, 1, nullptr, -3, nullptr, nullptr) == 0 && g_last_launch.empty());
    reset(); reached(fvo_count_guard(c, i32, nullptr, 4, 2, i32, -3, i32, nullptr), "count_guard_run");
  }
  CHECK(fvo_voxel_workspace_bytes(0) == -1 && fvo_voxel_workspace_bytes(10) > 0);
  reset(); rejected(c, fvo_voxel_down_sample(c, f64, 10, 0.0, u8, 1 << 16, f64, i32, i32, nullptr));
  reset(); rejected(c, fvo_voxel_down_sample(c, f64, 10, 0.5, u8, -1, f64, i32, i32, nullptr));
  reset(); CHECK(fvo_voxel_down_sample(c, nullptr, 0, 0.5, nullptr, 0, f64, i32, i32, nullptr) == 0);
  reset(); reached(fvo_voxel_down_sample(c, f64, 10, 0.5, u8, 1 << 16, f64, i32, i32, nullptr), "voxel_run");
  const int64_t vneed = fvo_voxel_workspace_bytes(10);
  reset(); refused(c, fvo_voxel_down_sample(c, f64, 10, 0.5, u8, vneed - 1, f64, i32, i32, nullptr),
                   "voxel_down_sample: workspace too small");
  reset(); reached(fvo_voxel_down_sample(c, f64, 10, 0.5, u8, vneed, f64, i32, i32, nullptr), "voxel_run");

  // ---- timing / debug / names
  CHECK(fvo_kernel_count() > 0 && std::strlen(fvo_kernel_name(0)) > 0 && fvo_kernel_name(-1)[0] == 0 &&
        fvo_kernel_name(fvo_kernel_count())[0] == 0);
  CHECK(fvo_timing_enable(c, ~0ull) == 0);
  double ms[64];
  int32_t launches[64];
  CHECK(fvo_timing_read(c, ms, launches) == 0 && fvo_timing_read(c, nullptr, launches) < 0);
  void* ptr = nullptr;
  int64_t bytes = 0;
  CHECK(fvo_debug_buffer(c, 99, &ptr, &bytes) < 0 && fvo_debug_buffer(c, 3, nullptr, &bytes) < 0);
  reset(); CHECK(fvo_debug_buffer(c, 2, &ptr, &bytes) == 0 && g_last_launch == "orb_score_debug");
  reset(); reached(fvo_test_retain_best(c, f32, 16, 4, i32, i32, nullptr), "orb_retain_best_run");
  // the kernel ids and their names come from one list: the count, and a name from its middle
  CHECK(fvo_kernel_count() == 36 && !std::strcmp(fvo_kernel_name(21), "ba_build") &&
        !std::strcmp(fvo_kernel_name(35), "speckle_apply"));
  {  // fvo_debug_copy: buffer 9 is (4 + max_batch) words
    unsigned char host[40];
    std::memset(host, 0xAB, sizeof(host));
    reset();
    CHECK(fvo_debug_buffer(c, 9, &ptr, &bytes) == 0 && bytes == 32);
    CHECK(fvo_debug_copy(c, 9, host, bytes) == 0 && host[0] == 0 && host[31] == 0 && host[32] == 0xAB);
    CHECK(fvo_debug_copy(c, 9, host, 0) == 0);
    refused(c, fvo_debug_copy(c, 9, host, bytes + 1), "debug_copy: bytes outside [0, the buffer's size]");
    refused(c, fvo_debug_copy(c, 9, host, -1), "debug_copy: bytes outside [0, the buffer's size]");
    refused(c, fvo_debug_copy(c, 9, nullptr, bytes), "null pointer argument");
    refused(c, fvo_debug_copy(c, 99, host, 1), "unknown debug buffer");
    CHECK(fvo_debug_copy(nullptr, 9, host, 1) < 0);
    g_memcpy_result = hipErrorInvalidValue;  // a failing copy is reported with the runtime's text
    CHECK(fvo_debug_copy(c, 9, host, bytes) < 0 && std::strstr(fvo_last_error(c), "stub hip error") != nullptr);
    g_memcpy_result = hipSuccess;
  }

  CHECK(g_live_allocs == 6);
  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
  fvo_destroy(nullptr);

  // a context without the ORB stage: stage checks and kp_capacity handling
  fvo_config_default(&cfg, 960, 600);
  cfg.stages = FVO_STAGE_BF;
  cfg.kp_capacity = 64;
  CHECK(fvo_create(0, &cfg, &c) == 0);
  reset(); rejected(c, fvo_orb_detect_compute(c, u8, 1, W * H, W, f32, u8, i32, 64, nullptr));
  reset(); rejected(c, fvo_sgbm(c, u8, u8, 1, W * H, W, i16, nullptr, nullptr));
  reset(); reached(fvo_bf_match(c, u8, i32, u8, i32, 1, 64, i32, i32, nullptr), "bf_run");
  reset(); refused(c, fvo_debug_buffer(c, 1, &ptr, &bytes), "orb stage not enabled");
  reset(); refused(c, fvo_debug_buffer(c, 2, &ptr, &bytes), "orb stage not enabled");
  reset(); refused(c, fvo_debug_buffer(c, 9, &ptr, &bytes), "no SGBM workspace");
  fvo_destroy(c);
  CHECK(g_live_allocs == 0);

  // the lens cases at their own size: two stripes of 40 rows
  cfg.width = 100;
  cfg.height = 76;
  CHECK(fvo_create(0, &cfg, &c) == 0);
  lens_checks(c, 100, 76);
  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
  cfg.width = 960;
  cfg.height = 600;

  // a mono context whose capacity passes the essential-matrix LDS bound
  cfg.stages = FVO_STAGE_MONO;
  cfg.kp_capacity = 6000;
  CHECK(fvo_create(0, &cfg, &c) == 0);
  reset(); refused(c, fvo_find_essential(c, f32, f32, i32, 1, 5041, 640, 480, 300, 0.999, 1.0, 1000, f64, u8, i32, nullptr),
                   "essential: point capacity exceeds LDS (cap <= 5040)");
  reset(); reached(fvo_find_essential(c, f32, f32, i32, 1, 5040, 640, 480, 300, 0.999, 1.0, 1000, f64, u8, i32, nullptr),
                   "essential_run");
  reset(); reached(fvo_recover_pose(c, f64, i32, f32, f32, i32, 1, 6000, 640, 480, 300, 50, f64, f64, f64, i32, nullptr),
                   "recover_run");
  fvo_destroy(c);
  CHECK(g_live_allocs == 0);

  std::printf("capi_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
