// Argument validation of the stereo-rectification C ABI (csrc/capi_rectify.cpp: fvo_rectify_map,
// fvo_remap_u8, fvo_rectify_gray, fvo_rectify_lds_budget) exercised on the host under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Linked with csrc/capi.cpp, csrc/capi_rectify.cpp
// and host_stubs.cpp; the stubs of the three rectification launchers are here (host_stubs.cpp is
// shared with programs that do not link capi_rectify.cpp): each records what the entry point passed
// on and touches the first and last element of every buffer as the entry point sized it.
// Built and run by tests/test_rectify_cpu.py.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host_stubs.h"

static int g_fail = 0, g_checks = 0;

struct RectArgs {
  const void *src, *map1, *map2, *dst;
  int batch, channels, spitch, dpitch;
  int64_t sstride, dstride;
  RectifyLens L;
};
static RectArgs g_rect;

static int hit(const char* name) {
  g_last_launch = name;
  ++g_launches;
  return 0;
}

int rectify_map_run(fvo_ctx* c, const RectifyLens& L, int16_t* map1, uint16_t* map2, hipStream_t) {
  const int64_t n = (int64_t)c->cfg.width * c->cfg.height;
  g_rect = RectArgs{nullptr, map1, map2, nullptr, 0, 0, 0, 0, 0, 0, L};
  map1[0] = map1[2 * n - 1] = 1;
  map2[0] = map2[n - 1] = 2;
  return hit("rectify_map_run");
}
int remap_run(fvo_ctx* c, const uint8_t* src, int batch, int64_t sstride, int spitch, int channels,
              const int16_t* map1, const uint16_t* map2, uint8_t* dst, int64_t dstride, int dpitch, hipStream_t) {
  const int W = c->cfg.width, H = c->cfg.height;
  g_rect = RectArgs{src, map1, map2, dst, batch, channels, spitch, dpitch, sstride, dstride, RectifyLens{}};
  const int64_t n = (int64_t)W * H;
  dst[0] = (uint8_t)(src[0] + map1[0] + map2[0]);
  dst[(batch - 1) * dstride + (int64_t)(H - 1) * dpitch + (int64_t)W * channels - 1] =
      (uint8_t)(src[(batch - 1) * sstride + (int64_t)(H - 1) * spitch + (int64_t)W * channels - 1] + map1[2 * n - 1] +
                map2[n - 1]);
  return hit("remap_run");
}
int rectify_gray_run(fvo_ctx* c, const uint8_t* src, int batch, int64_t sstride, int spitch, int channels,
                     const RectifyLens& L, uint8_t* gray, int64_t dstride, int dpitch, hipStream_t) {
  const int W = c->cfg.width, H = c->cfg.height;
  g_rect = RectArgs{src, nullptr, nullptr, gray, batch, channels, spitch, dpitch, sstride, dstride, L};
  gray[0] = src[0];
  gray[(batch - 1) * dstride + (int64_t)(H - 1) * dpitch + W - 1] =
      src[(batch - 1) * sstride + (int64_t)(H - 1) * spitch + (int64_t)W * channels - 1];
  return hit("rectify_gray_run");
}

#define CHECK(cond)                                                       \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      ++g_fail;                                                           \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                     \
  } while (0)

// rc must be < 0 with exactly this message, nothing launched and nothing allocated
#define REFUSED(c, call, msg)                          \
  do {                                                 \
    g_launches = 0;                                    \
    const int live_ = g_live_allocs;                   \
    CHECK((call) < 0);                                 \
    CHECK(!std::strcmp(fvo_last_error(c), msg));       \
    CHECK(g_launches == 0 && g_live_allocs == live_);  \
  } while (0)

// rc must be 0 and exactly `launcher` reached, once
#define ACCEPTED(call, launcher)                       \
  do {                                                 \
    g_launches = 0;                                    \
    g_last_launch.clear();                             \
    const int live_ = g_live_allocs;                   \
    CHECK((call) == 0);                                \
    CHECK(g_launches == 1 && g_last_launch == launcher && g_live_allocs == live_); \
  } while (0)

int main() {
  const double dinf = std::numeric_limits<double>::infinity(), dnan = std::nan("");
  const int W = 12, H = 5, B = 3;
  fvo_config cfg;
  fvo_config_default(&cfg, W, H);
  cfg.max_batch = B;
  cfg.stages = FVO_STAGE_BF;
  cfg.kp_capacity = 64;
  fvo_ctx* c = nullptr;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  if (!c) return 1;

  // every buffer of exactly the size the call needs (heap: ASan sees one byte too many)
  std::vector<int16_t> map1(2 * W * H);
  std::vector<uint16_t> map2(W * H);
  const int sp3 = 3 * W + 4, sp1 = W + 3, dp3 = 3 * W + 1, dp1 = W + 2;  // padded rows
  const int64_t ss3 = (int64_t)sp3 * H + 7, ss1 = (int64_t)sp1 * H + 5, ds3 = (int64_t)dp3 * H + 3,
                ds1 = (int64_t)dp1 * H + 9;
  std::vector<uint8_t> src3((B - 1) * ss3 + (H - 1) * sp3 + 3 * W, 1), src1((B - 1) * ss1 + (H - 1) * sp1 + W, 1);
  std::vector<uint8_t> dst3((B - 1) * ds3 + (H - 1) * dp3 + 3 * W), dst1((B - 1) * ds1 + (H - 1) * dp1 + W);
  const double K[9] = {40.0, 0, 5.5, 0, 41.0, 2.0, 0, 0, 1};
  const double newK[9] = {38.0, 0, 6.0, 0, 38.0, 2.5, 0, 0, 1};
  const double R[9] = {0.9998, -0.02, 0.0, 0.02, 0.9998, 0.0, 0.0, 0.0, 1.0};
  const double d8[8] = {-0.1, 0.02, 1e-3, -1e-3, 0.01, 0.2, -0.03, 0.004};

#define MAP(ctx, k, d, n, r, nk, m1, m2) fvo_rectify_map(ctx, k, d, n, r, nk, m1, m2, nullptr)
#define REMAP(ctx, s, b, sst, sp, ch, m1, m2, d, dst_, dp) fvo_remap_u8(ctx, s, b, sst, sp, ch, m1, m2, d, dst_, dp, nullptr)
#define GRAY(ctx, s, b, sst, sp, ch, k, d, n, r, nk, g, dst_, dp) \
  fvo_rectify_gray(ctx, s, b, sst, sp, ch, k, d, n, r, nk, g, dst_, dp, nullptr)

  // ---- fvo_rectify_map
  ACCEPTED(MAP(c, K, d8, 8, R, newK, map1.data(), map2.data()), "rectify_map_run");
  CHECK(g_rect.map1 == map1.data() && g_rect.map2 == map2.data() && g_rect.L.rational == 1 && g_rect.L.k6 == d8[7] &&
        g_rect.L.fx == K[0] && g_rect.L.v0 == K[5] && g_rect.L.p2 == d8[3]);
  ACCEPTED(MAP(c, K, d8, 5, nullptr, nullptr, map1.data(), map2.data()), "rectify_map_run");  // R = I, newK = K
  CHECK(g_rect.L.rational == 0 && g_rect.L.k3 == d8[4] && g_rect.L.k4 == 0.0);
  CHECK(g_rect.L.ir[0] == 1.0 / K[0] && g_rect.L.ir[6] == 0.0 && g_rect.L.ir[7] == 0.0 && g_rect.L.ir[8] == 1.0);
  ACCEPTED(MAP(c, K, d8, 4, R, nullptr, map1.data(), map2.data()), "rectify_map_run");
  CHECK(g_rect.L.k3 == 0.0 && g_rect.L.rational == 0);
  CHECK(MAP(nullptr, K, d8, 5, R, newK, map1.data(), map2.data()) < 0);
  const char* null_msg = "null pointer argument";
  REFUSED(c, MAP(c, nullptr, d8, 5, R, newK, map1.data(), map2.data()), null_msg);
  REFUSED(c, MAP(c, K, nullptr, 5, R, newK, map1.data(), map2.data()), null_msg);
  REFUSED(c, MAP(c, K, d8, 5, R, newK, nullptr, map2.data()), null_msg);
  REFUSED(c, MAP(c, K, d8, 5, R, newK, map1.data(), nullptr), null_msg);
  const char* al_msg = "rectify: map1 must be 4-byte and map2 2-byte aligned";
  REFUSED(c, MAP(c, K, d8, 5, R, newK, map1.data() + 1, map2.data()), al_msg);
  REFUSED(c, MAP(c, K, d8, 5, R, newK, map1.data(),
                 reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(map2.data()) + 1)), al_msg);
  const char* nd_msg = "rectify: n_dist must be 4, 5 or 8";
  for (int n : {0, 3, 6, 7, 9, 12, 14, -1})
    REFUSED(c, MAP(c, K, d8, n, R, newK, map1.data(), map2.data()), nd_msg);
  const char* fin_msg = "rectify: K, dist, R and newK must be finite";
  for (double bad : {dinf, -dinf, dnan}) {
    double Kb[9], Rb[9], Nb[9], db[8];
    std::memcpy(Kb, K, sizeof(Kb));
    std::memcpy(Rb, R, sizeof(Rb));
    std::memcpy(Nb, newK, sizeof(Nb));
    std::memcpy(db, d8, sizeof(db));
    Kb[7] = Rb[8] = Nb[0] = db[7] = bad;
    REFUSED(c, MAP(c, Kb, d8, 8, R, newK, map1.data(), map2.data()), fin_msg);
    REFUSED(c, MAP(c, K, db, 8, R, newK, map1.data(), map2.data()), fin_msg);
    REFUSED(c, MAP(c, K, d8, 8, Rb, newK, map1.data(), map2.data()), fin_msg);
    REFUSED(c, MAP(c, K, d8, 8, R, Nb, map1.data(), map2.data()), fin_msg);
    ACCEPTED(MAP(c, K, db, 5, R, newK, map1.data(), map2.data()), "rectify_map_run");  // dist[7] is not read with 5
    db[7] = d8[7];
    db[4] = bad;
    ACCEPTED(MAP(c, K, db, 4, R, newK, map1.data(), map2.data()), "rectify_map_run");
  }
  {
    const char* det_msg = "rectify: newK*R is singular";
    const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, R2[9] = {1, 0, 0, 1, 0, 0, 0, 0, 1};
    REFUSED(c, MAP(c, K, d8, 5, R, Z, map1.data(), map2.data()), det_msg);
    REFUSED(c, MAP(c, K, d8, 5, R2, newK, map1.data(), map2.data()), det_msg);
    REFUSED(c, MAP(c, Z, d8, 5, nullptr, nullptr, map1.data(), map2.data()), det_msg);  // newK = K
    // _w: a view turned 90 degrees about y looks along the camera's image plane; one turned so that
    // the horizon cuts the image has corners on both sides; a mirrored one has _w < 0 everywhere
    const char* w_msg = "rectify: _w <= 0 at an image corner (the view reaches the camera's horizon)";
    const double Ry90[9] = {0, 0, 1, 0, 1, 0, -1, 0, 0};
    REFUSED(c, MAP(c, K, d8, 5, Ry90, newK, map1.data(), map2.data()), w_msg);
    const double a = 1.45, Ry[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)};
    REFUSED(c, MAP(c, K, d8, 5, Ry, newK, map1.data(), map2.data()), w_msg);
    const double Rm[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};
    REFUSED(c, MAP(c, K, d8, 5, Rm, newK, map1.data(), map2.data()), w_msg);
    const double b = 1.40, Rok[9] = {std::cos(b), 0, std::sin(b), 0, 1, 0, -std::sin(b), 0, std::cos(b)};
    ACCEPTED(MAP(c, K, d8, 5, Rok, newK, map1.data(), map2.data()), "rectify_map_run");  // horizon outside the image
    const double Kw[9] = {1e300, 0, 0, 0, 1e300, 0, 0, 0, 1e-10};  // finite entries, det overflows: _w is NaN
    REFUSED(c, MAP(c, K, d8, 5, nullptr, Kw, map1.data(), map2.data()), w_msg);  }

  // ---- fvo_remap_u8
  ACCEPTED(REMAP(c, src3.data(), B, ss3, sp3, 3, map1.data(), map2.data(), dst3.data(), ds3, dp3), "remap_run");
  CHECK(g_rect.src == src3.data() && g_rect.dst == dst3.data() && g_rect.map1 == map1.data() && g_rect.batch == B &&
        g_rect.channels == 3 && g_rect.spitch == sp3 && g_rect.dpitch == dp3 && g_rect.sstride == ss3 &&
        g_rect.dstride == ds3);
  ACCEPTED(REMAP(c, src1.data(), B, ss1, sp1, 1, map1.data(), map2.data(), dst1.data(), ds1, dp1), "remap_run");
  {  // the tightest layout: pitch == channels*width, stride == pitch*height
    std::vector<uint8_t> s(3 * W * H * B, 1), d(3 * W * H * B);
    ACCEPTED(REMAP(c, s.data(), B, 3 * W * H, 3 * W, 3, map1.data(), map2.data(), d.data(), 3 * W * H, 3 * W), "remap_run");
    REFUSED(c, REMAP(c, s.data(), B, 3 * W * H, 3 * W - 1, 3, map1.data(), map2.data(), d.data(), 3 * W * H, 3 * W),
            "bad pitch/stride");
    REFUSED(c, REMAP(c, s.data(), B, 3 * W * H - 1, 3 * W, 3, map1.data(), map2.data(), d.data(), 3 * W * H, 3 * W),
            "bad pitch/stride");
    REFUSED(c, REMAP(c, s.data(), B, 3 * W * H, 3 * W, 3, map1.data(), map2.data(), d.data(), 3 * W * H, 3 * W - 1),
            "bad pitch/stride");
    REFUSED(c, REMAP(c, s.data(), B, 3 * W * H, 3 * W, 3, map1.data(), map2.data(), d.data(), 3 * W * H - 1, 3 * W),
            "bad pitch/stride");
    REFUSED(c, REMAP(c, s.data(), B, -1, 3 * W, 3, map1.data(), map2.data(), d.data(), 3 * W * H, 3 * W),
            "bad pitch/stride");
    // a mono layout is too narrow for 3 channels
    REFUSED(c, REMAP(c, s.data(), B, W * H, W, 3, map1.data(), map2.data(), d.data(), 3 * W * H, 3 * W),
            "bad pitch/stride");
    const char* ov_msg = "remap: dst must not overlap src";
    REFUSED(c, REMAP(c, s.data(), B, 3 * W * H, 3 * W, 3, map1.data(), map2.data(), s.data(), 3 * W * H, 3 * W), ov_msg);
    {  // one buffer holding both: dst may begin where src's last pixel ends, and not one byte sooner
      const int64_t n = 3 * W * H * B;
      std::vector<uint8_t> both(2 * n, 1);
      ACCEPTED(REMAP(c, both.data(), B, 3 * W * H, 3 * W, 3, map1.data(), map2.data(), both.data() + n, 3 * W * H, 3 * W),
               "remap_run");
      ACCEPTED(REMAP(c, both.data() + n, B, 3 * W * H, 3 * W, 3, map1.data(), map2.data(), both.data(), 3 * W * H, 3 * W),
               "remap_run");
      REFUSED(c, REMAP(c, both.data(), B, 3 * W * H, 3 * W, 3, map1.data(), map2.data(), both.data() + n - 1, 3 * W * H,
                       3 * W), ov_msg);
      REFUSED(c, REMAP(c, both.data() + n - 1, B, 3 * W * H, 3 * W, 3, map1.data(), map2.data(), both.data(), 3 * W * H,
                       3 * W), ov_msg);
    }
  }
  g_launches = 0;
  CHECK(REMAP(c, nullptr, 0, 0, 0, 7, nullptr, nullptr, nullptr, 0, 0) == 0 && g_launches == 0);  // batch == 0 first
  CHECK(REMAP(nullptr, src3.data(), B, ss3, sp3, 3, map1.data(), map2.data(), dst3.data(), ds3, dp3) < 0);
  REFUSED(c, REMAP(c, src3.data(), B + 1, ss3, sp3, 3, map1.data(), map2.data(), dst3.data(), ds3, dp3),
          "batch exceeds max_batch");
  REFUSED(c, REMAP(c, src3.data(), -1, ss3, sp3, 3, map1.data(), map2.data(), dst3.data(), ds3, dp3),
          "batch exceeds max_batch");
  REFUSED(c, REMAP(c, nullptr, B, ss3, sp3, 3, map1.data(), map2.data(), dst3.data(), ds3, dp3), null_msg);
  REFUSED(c, REMAP(c, src3.data(), B, ss3, sp3, 3, nullptr, map2.data(), dst3.data(), ds3, dp3), null_msg);
  REFUSED(c, REMAP(c, src3.data(), B, ss3, sp3, 3, map1.data(), nullptr, dst3.data(), ds3, dp3), null_msg);
  REFUSED(c, REMAP(c, src3.data(), B, ss3, sp3, 3, map1.data(), map2.data(), nullptr, ds3, dp3), null_msg);
  REFUSED(c, REMAP(c, src3.data(), B, ss3, sp3, 3, map1.data() + 1, map2.data(), dst3.data(), ds3, dp3), al_msg);
  REFUSED(c, REMAP(c, src3.data(), B, ss3, sp3, 3, map1.data(),
                   reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(map2.data()) + 1), dst3.data(), ds3, dp3), al_msg);
  const char* ch_msg = "rectify: channels must be 1 or 3";
  for (int ch : {0, 2, 4, -1})
    REFUSED(c, REMAP(c, src3.data(), B, ss3, sp3, ch, map1.data(), map2.data(), dst3.data(), ds3, dp3), ch_msg);

  // ---- fvo_rectify_gray
  ACCEPTED(GRAY(c, src3.data(), B, ss3, sp3, 3, K, d8, 8, R, newK, dst1.data(), ds1, dp1), "rectify_gray_run");
  CHECK(g_rect.src == src3.data() && g_rect.dst == dst1.data() && g_rect.batch == B && g_rect.channels == 3 &&
        g_rect.spitch == sp3 && g_rect.dpitch == dp1 && g_rect.sstride == ss3 && g_rect.dstride == ds1 &&
        g_rect.L.rational == 1 && g_rect.L.k5 == d8[6]);
  ACCEPTED(GRAY(c, src1.data(), B, ss1, sp1, 1, K, d8, 5, nullptr, nullptr, dst1.data(), ds1, dp1), "rectify_gray_run");
  ACCEPTED(GRAY(c, src1.data(), 1, ss1, sp1, 1, K, d8, 4, R, nullptr, dst1.data(), ds1, dp1), "rectify_gray_run");
  {
    std::vector<uint8_t> s(3 * W * H * B, 1), g(W * H * B);
    ACCEPTED(GRAY(c, s.data(), B, 3 * W * H, 3 * W, 3, K, d8, 5, R, newK, g.data(), W * H, W), "rectify_gray_run");
    REFUSED(c, GRAY(c, s.data(), B, 3 * W * H, 3 * W - 1, 3, K, d8, 5, R, newK, g.data(), W * H, W), "bad pitch/stride");
    REFUSED(c, GRAY(c, s.data(), B, 3 * W * H - 1, 3 * W, 3, K, d8, 5, R, newK, g.data(), W * H, W), "bad pitch/stride");
    REFUSED(c, GRAY(c, s.data(), B, 3 * W * H, 3 * W, 3, K, d8, 5, R, newK, g.data(), W * H, W - 1), "bad pitch/stride");
    REFUSED(c, GRAY(c, s.data(), B, 3 * W * H, 3 * W, 3, K, d8, 5, R, newK, g.data(), W * H - 1, W), "bad pitch/stride");
    REFUSED(c, GRAY(c, s.data(), B, W * H, W, 3, K, d8, 5, R, newK, g.data(), W * H, W), "bad pitch/stride");
    ACCEPTED(GRAY(c, s.data(), B, W * H, W, 1, K, d8, 5, R, newK, g.data(), W * H, W), "rectify_gray_run");
    const char* gov_msg = "rectify_gray: gray must not overlap src";
    REFUSED(c, GRAY(c, s.data(), B, W * H, W, 1, K, d8, 5, R, newK, s.data(), W * H, W), gov_msg);
    // the gray images inside the bgr buffer: its last byte overlaps, the byte after src's last pixel does not
    REFUSED(c, GRAY(c, s.data(), B, 3 * W * H, 3 * W, 3, K, d8, 5, R, newK, s.data() + 3 * W * H * B - 1, W * H, W),
            gov_msg);
    REFUSED(c, GRAY(c, s.data() + W * H - 1, 1, 3 * W * H, 3 * W, 3, K, d8, 5, R, newK, s.data(), W * H, W), gov_msg);
    ACCEPTED(GRAY(c, s.data() + W * H, 1, W * H, W, 1, K, d8, 5, R, newK, s.data(), W * H, W), "rectify_gray_run");
  }
  g_launches = 0;
  CHECK(GRAY(c, nullptr, 0, 0, 0, 7, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0) == 0 && g_launches == 0);
  CHECK(GRAY(nullptr, src3.data(), B, ss3, sp3, 3, K, d8, 8, R, newK, dst1.data(), ds1, dp1) < 0);
  REFUSED(c, GRAY(c, src3.data(), B + 1, ss3, sp3, 3, K, d8, 8, R, newK, dst1.data(), ds1, dp1), "batch exceeds max_batch");
  REFUSED(c, GRAY(c, src3.data(), -1, ss3, sp3, 3, K, d8, 8, R, newK, dst1.data(), ds1, dp1), "batch exceeds max_batch");
  REFUSED(c, GRAY(c, nullptr, B, ss3, sp3, 3, K, d8, 8, R, newK, dst1.data(), ds1, dp1), null_msg);
  REFUSED(c, GRAY(c, src3.data(), B, ss3, sp3, 3, nullptr, d8, 8, R, newK, dst1.data(), ds1, dp1), null_msg);
  REFUSED(c, GRAY(c, src3.data(), B, ss3, sp3, 3, K, nullptr, 8, R, newK, dst1.data(), ds1, dp1), null_msg);
  REFUSED(c, GRAY(c, src3.data(), B, ss3, sp3, 3, K, d8, 8, R, newK, nullptr, ds1, dp1), null_msg);
  for (int ch : {0, 2, 4})
    REFUSED(c, GRAY(c, src3.data(), B, ss3, sp3, ch, K, d8, 8, R, newK, dst1.data(), ds1, dp1), ch_msg);
  REFUSED(c, GRAY(c, src3.data(), B, ss3, sp3, 3, K, d8, 6, R, newK, dst1.data(), ds1, dp1), nd_msg);
  {
    double Kb[9];
    std::memcpy(Kb, K, sizeof(Kb));
    Kb[2] = dnan;
    REFUSED(c, GRAY(c, src3.data(), B, ss3, sp3, 3, Kb, d8, 8, R, newK, dst1.data(), ds1, dp1), fin_msg);
    const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Rm[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};
    REFUSED(c, GRAY(c, src3.data(), B, ss3, sp3, 3, K, d8, 8, Z, newK, dst1.data(), ds1, dp1), "rectify: newK*R is singular");
    REFUSED(c, GRAY(c, src3.data(), B, ss3, sp3, 3, K, d8, 8, Rm, newK, dst1.data(), ds1, dp1),
            "rectify: _w <= 0 at an image corner (the view reaches the camera's horizon)");
  }

  // ---- a context without an image size (fvo_create accepts one when no stage needs the size):
  // every entry point refuses before its launch would get an empty grid
  for (int k = 0; k < 2; ++k) {
    fvo_config z;
    fvo_config_default(&z, k == 0 ? 0 : W, k == 0 ? H : 0);
    z.max_batch = B;
    z.stages = FVO_STAGE_BF;
    z.kp_capacity = 64;
    fvo_ctx* e = nullptr;
    CHECK(fvo_create(0, &z, &e) == 0 && e != nullptr);
    if (!e) return 1;
    const char* sz_msg = "rectify: the context's width and height must be >= 1";
    REFUSED(e, MAP(e, K, d8, 5, R, newK, map1.data(), map2.data()), sz_msg);
    REFUSED(e, REMAP(e, src3.data(), B, ss3, sp3, 3, map1.data(), map2.data(), dst3.data(), ds3, dp3), sz_msg);
    REFUSED(e, REMAP(e, src1.data(), 1, 0, 0, 1, map1.data(), map2.data(), dst1.data(), 0, 0), sz_msg);
    REFUSED(e, GRAY(e, src3.data(), B, ss3, sp3, 3, K, d8, 8, R, newK, dst1.data(), ds1, dp1), sz_msg);
    REFUSED(e, GRAY(e, src1.data(), 1, 0, 0, 1, K, d8, 5, nullptr, nullptr, dst1.data(), 0, 0), sz_msg);
    fvo_destroy(e);
  }

  // ---- fvo_rectify_lds_budget
  CHECK(c->rectify_budget == FVO_RECTIFY_LDS_BYTES);
  CHECK(fvo_rectify_lds_budget(c, 0) == 0 && c->rectify_budget == 0);
  CHECK(fvo_rectify_lds_budget(c, FVO_RECTIFY_LDS_BYTES) == 0 && c->rectify_budget == FVO_RECTIFY_LDS_BYTES);
  REFUSED(c, fvo_rectify_lds_budget(c, -1), "rectify_lds_budget: bytes outside [0, FVO_RECTIFY_LDS_BYTES]");
  REFUSED(c, fvo_rectify_lds_budget(c, FVO_RECTIFY_LDS_BYTES + 1),
          "rectify_lds_budget: bytes outside [0, FVO_RECTIFY_LDS_BYTES]");
  CHECK(c->rectify_budget == FVO_RECTIFY_LDS_BYTES && fvo_rectify_lds_budget(nullptr, 0) < 0);

  // the frozen timing table is untouched
  CHECK(fvo_kernel_count() == 36);

  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
  std::printf("rectify_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
