// Argument validation and workspace arithmetic of the dense-mapping C ABI (csrc/capi.cpp:
// fvo_dense_workspace_bytes, fvo_dense_map_append, fvo_reproject_to_3d) exercised on the host
// under AddressSanitizer + UndefinedBehaviorSanitizer.  Linked with csrc/capi.cpp and
// host_stubs.cpp, whose stubs of the launchers record what the entry points passed on (g_dense,
// g_rp).  Built and run by tests/test_dense_cpu.py.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

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

// rc must be < 0 with exactly this message and nothing launched
#define REFUSED(c, call, msg)                          \
  do {                                                 \
    g_launches = 0;                                    \
    CHECK((call) < 0);                                 \
    CHECK(!std::strcmp(fvo_last_error(c), msg));       \
    CHECK(g_launches == 0);                            \
  } while (0)

// rc must be 0 and exactly dense_append_run / reproject_run reached, once
#define ACCEPTED(call, launcher)                       \
  do {                                                 \
    g_launches = 0;                                    \
    g_last_launch.clear();                             \
    CHECK((call) == 0);                                \
    CHECK(g_launches == 1 && g_last_launch == launcher); \
  } while (0)

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nanf_ = std::nanf("");
  const double dinf = std::numeric_limits<double>::infinity(), dnan = std::nan("");

  // ---- workspace arithmetic: 8 + 12 per block of 1024 samples, -1 for sizes the call refuses
  CHECK(fvo_dense_workspace_bytes(1, 1, 1, 1) == 8 + 12);
  CHECK(fvo_dense_workspace_bytes(1, 32, 32, 1) == 8 + 12);       // exactly one block
  CHECK(fvo_dense_workspace_bytes(1, 32, 33, 1) == 8 + 12 * 2);
  CHECK(fvo_dense_workspace_bytes(64, 600, 960, 1) == 8 + 12ll * 64 * 563);  // 576000 / 1024 = 562.5
  CHECK(fvo_dense_workspace_bytes(64, 600, 960, 4) == 8 + 12ll * 64 * 36);   // 150 x 240 samples
  CHECK(fvo_dense_workspace_bytes(3, 19, 37, 5) == 8 + 12 * 3);             // 4 x 8 samples
  CHECK(fvo_dense_workspace_bytes(2, 19, 37, 1000) == 8 + 12 * 2);          // one sample per frame
  CHECK(fvo_dense_workspace_bytes(2, 19, 37, INT32_MAX) == 8 + 12 * 2);
  CHECK(fvo_dense_workspace_bytes(0, 600, 960, 1) == 0);
  CHECK(fvo_dense_workspace_bytes(-1, 600, 960, 1) == -1);
  CHECK(fvo_dense_workspace_bytes(1, 0, 960, 1) == -1);
  CHECK(fvo_dense_workspace_bytes(1, 600, 0, 1) == -1);
  CHECK(fvo_dense_workspace_bytes(1, 600, 960, 0) == -1);
  CHECK(fvo_dense_workspace_bytes(1, 600, 960, -3) == -1);
  CHECK(fvo_dense_workspace_bytes(0, 0, 960, 1) == -1);  // a bad size is refused at batch 0 too
  // height*width: INT32_MAX is the last size accepted
  CHECK(fvo_dense_workspace_bytes(1, 1, INT32_MAX, 1) == 8 + 12ll * 2097152);
  CHECK(fvo_dense_workspace_bytes(1, INT32_MAX, 1, 1) == 8 + 12ll * 2097152);
  CHECK(fvo_dense_workspace_bytes(1, 46341, 46341, 1) == -1);  // 46341^2 = 2^31 + 4633
  CHECK(fvo_dense_workspace_bytes(1, INT32_MAX, INT32_MAX, 1) == -1);
  CHECK(fvo_dense_workspace_bytes(1, INT32_MAX, INT32_MAX, INT32_MAX) == -1);
  // batch * blocks: INT32_MAX launch blocks is the last count accepted
  CHECK(fvo_dense_workspace_bytes(1023, 1, INT32_MAX, 1) == 8 + 12ll * 1023 * 2097152);
  CHECK(fvo_dense_workspace_bytes(1024, 1, INT32_MAX, 1) == -1);  // 2^31 blocks
  CHECK(fvo_dense_workspace_bytes(INT32_MAX, 32, 32, 1) == 8 + 12ll * INT32_MAX);
  CHECK(fvo_dense_workspace_bytes(INT32_MAX, 32, 33, 1) == -1);

  // ---- a context (stub device layer); the dense calls are tied to no stage, batch or image size
  fvo_config cfg;
  fvo_config_default(&cfg, 64, 64);
  cfg.max_batch = 1;
  cfg.stages = FVO_STAGE_BF;
  cfg.kp_capacity = 64;
  fvo_ctx* c = nullptr;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  if (!c) return 1;

  // a [3][5][16] buffer of which calls use a 12-wide view; everything of exactly the needed size
  static int16_t disp[3 * 5 * 16];
  for (int i = 0; i < 3 * 5 * 16; ++i) disp[i] = (int16_t)(i - 100);
  const double K[9] = {400.0, 0, 6.0, 0, 410.0, 2.5, 0, 0, 1};
  static double T[3 * 16];
  static int32_t keep[3] = {1, 0, 1}, n_added[3], count[1] = {7};
  static double m64[4 * 3];
  static float m32[4 * 3];
  const int64_t need = fvo_dense_workspace_bytes(3, 5, 12, 1);
  CHECK(need == 8 + 12 * 3);
  alignas(8) static unsigned char ws[8 + 12 * 3 + 8];

#define DENSE(ctx, d, b, h, w, st, pi, k, bl, sp, md, z0, z1, kp, t, cn, cap, o64, o32, na, wsp, wb) \
  fvo_dense_map_append(ctx, d, b, h, w, st, pi, k, bl, sp, md, z0, z1, kp, t, cn, cap, o64, o32, na, wsp, wb, nullptr)

  // good call: the launcher is reached, once, with the arguments as given
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, -32768, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                 need),
           "dense_append_run");
  CHECK(g_dense.disp == disp && g_dense.K == K && g_dense.keep == keep && g_dense.T == T && g_dense.count == count &&
        g_dense.out64 == m64 && g_dense.out32 == m32 && g_dense.n_added == n_added && g_dense.ws == ws);
  CHECK(g_dense.batch == 3 && g_dense.H == 5 && g_dense.W == 12 && g_dense.stride == 80 && g_dense.pitch == 16 &&
        g_dense.step == 1 && g_dense.min_disp16 == -32768 && g_dense.map_cap == 4 && g_dense.baseline == 0.12 &&
        g_dense.z_min == 0.1f && g_dense.z_max == 1000.f);
  // the optional pointers; a batch beyond the context's max_batch; any image size
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, nullptr, T, count, 4, nullptr, m32, nullptr,
                 ws, need + 1),
           "dense_append_run");
  CHECK(g_dense.keep == nullptr && g_dense.out64 == nullptr && g_dense.n_added == nullptr);
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, nullptr, n_added, ws,
                 need),
           "dense_append_run");

  // batch == 0 returns 0 before the pointer checks; nothing launched
  g_launches = 0;
  CHECK(DENSE(c, nullptr, 0, 5, 12, 80, 16, nullptr, 0.12, 1, 1, 0.1f, 1000.f, nullptr, nullptr, nullptr, 4, nullptr,
              nullptr, nullptr, nullptr, 0) == 0);
  CHECK(DENSE(c, disp, 0, 0, 0, 0, 0, K, -1.0, 0, 1, 5.f, 1.f, keep, T, count, -1, m64, m32, n_added, ws, 0) == 0);
  CHECK(g_launches == 0);

  // ---- every refusal by its message, the accepted bound next to it
  CHECK(DENSE(nullptr, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
              need) < 0);
  REFUSED(c, DENSE(c, disp, -1, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need),
          "batch < 0");
  const char* null_msg = "null pointer argument";
  REFUSED(c, DENSE(c, nullptr, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), null_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, nullptr, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added,
                   ws, need), null_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, nullptr, count, 4, m64, m32, n_added,
                   ws, need), null_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, nullptr, 4, m64, m32, n_added, ws,
                   need), null_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added,
                   nullptr, need), null_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, nullptr, nullptr,
                   n_added, ws, need), null_msg);
  // height / width
  const char* hw_msg = "dense_map_append: height and width must be >= 1";
  REFUSED(c, DENSE(c, disp, 3, 0, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), hw_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 0, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), hw_msg);
  REFUSED(c, DENSE(c, disp, 3, -5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), hw_msg);
  ACCEPTED(DENSE(c, disp, 3, 1, 1, 1, 1, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws, need),
           "dense_append_run");
  REFUSED(c, DENSE(c, disp, 1, 65536, 32768, (int64_t)1 << 31, 32768, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4,
                   m64, m32, n_added, ws, need),
          "dense_map_append: height*width exceeds INT32_MAX");
  REFUSED(c, DENSE(c, disp, 1, INT32_MAX, INT32_MAX, INT64_MAX, INT32_MAX, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count,
                   4, m64, m32, n_added, ws, need),
          "dense_map_append: height*width exceeds INT32_MAX");
  // pitch / stride
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 11, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), "bad pitch/stride");
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 79, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), "bad pitch/stride");
  REFUSED(c, DENSE(c, disp, 3, 5, 12, -80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), "bad pitch/stride");
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 60, 12, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                 need),
           "dense_append_run");  // pitch == width, stride == pitch * height
  // step
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 0, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), "dense_map_append: step must be >= 1");
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, -4, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need), "dense_map_append: step must be >= 1");
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, INT32_MAX, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added,
                 ws, need),
           "dense_append_run");
  // the depth range: finite, 0 <= z_min < z_max
  const char* z_msg = "dense_map_append: z_min and z_max must be finite with 0 <= z_min < z_max";
  const float zbad[][2] = {{-0.1f, 1000.f}, {1.f, 1.f}, {2.f, 1.f}, {0.1f, inf}, {-inf, 1.f}, {nanf_, 1.f}, {0.1f, nanf_}};
  for (const auto& z : zbad)
    REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, z[0], z[1], keep, T, count, 4, m64, m32, n_added, ws,
                     need), z_msg);
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.f, 1e-30f, keep, T, count, 4, m64, m32, n_added, ws,
                 need),
           "dense_append_run");
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, -0.f, std::numeric_limits<float>::max(), keep, T, count, 4,
                 m64, m32, n_added, ws, need),
           "dense_append_run");
  // the camera: K[0], K[4] and the baseline finite and > 0
  const char* k_msg = "dense_map_append: K[0], K[4] and baseline must be finite and > 0";
  const double bad[] = {0.0, -1.0, dinf, dnan};
  for (double v : bad) {
    double Kb[9];
    std::memcpy(Kb, K, sizeof(Kb));
    Kb[0] = v;
    REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, Kb, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                     need), k_msg);
    Kb[0] = K[0];
    Kb[4] = v;
    REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, Kb, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                     need), k_msg);
    REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, v, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                     need), k_msg);
  }
  {
    const double Ks[9] = {5e-324, 0, dnan, 0, 5e-324, -dinf, 0, 0, 0};  // only K[0], K[4] are checked
    ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, Ks, 5e-324, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need),
             "dense_append_run");
  }
  // map_cap
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, -1, m64, m32, n_added, ws,
                   need), "map_cap < 0");
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 0, m64, m32, n_added, ws,
                 need),
           "dense_append_run");
  CHECK(g_dense.map_cap == 0);
  // the workspace
  const char* ws_msg = "dense_map_append: workspace too small";
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   need - 1), ws_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   0), ws_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws,
                   -1), ws_msg);
  REFUSED(c, DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added,
                   ws + 4, need), "dense_map_append: workspace must be 8-byte aligned");
  ACCEPTED(DENSE(c, disp, 3, 5, 12, 80, 16, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4, m64, m32, n_added, ws + 8,
                 need),
           "dense_append_run");
  // more launch blocks than one launch takes (no buffer is touched: refused first)
  REFUSED(c, DENSE(c, disp, 1024, 1, INT32_MAX, INT32_MAX, INT32_MAX, K, 0.12, 1, 1, 0.1f, 1000.f, keep, T, count, 4,
                   m64, m32, n_added, ws, INT64_MAX),
          "dense_map_append: batch * sample blocks exceeds INT32_MAX");

  // ---- fvo_reproject_to_3d
  static float fdisp[2 * 5 * 16];
  static float out[2 * 5 * 12 * 3];
  static uint32_t key[2];
  const double Q[16] = {1, 0, 0, -6.0, 0, 1, 0, -2.5, 0, 0, 0, 400.0, 0, 0, 8.0, 0.5};
#define RP(ctx, d, f, b, h, w, st, pi, q, hm, k, o) fvo_reproject_to_3d(ctx, d, f, b, h, w, st, pi, q, hm, k, o, nullptr)
  ACCEPTED(RP(c, disp, 0, 2, 5, 12, 80, 16, Q, 1, key, out), "reproject_run");
  CHECK(g_rp.disp == disp && g_rp.Q == Q && g_rp.key == key && g_rp.out == out && g_rp.is_f32 == 0 &&
        g_rp.batch == 2 && g_rp.H == 5 && g_rp.W == 12 && g_rp.stride == 80 && g_rp.pitch == 16 && g_rp.handle == 1);
  ACCEPTED(RP(c, fdisp, 1, 2, 5, 12, 80, 16, Q, 0, nullptr, out), "reproject_run");  // no key without the flag
  CHECK(g_rp.is_f32 == 1 && g_rp.handle == 0 && g_rp.key == nullptr);
  ACCEPTED(RP(c, fdisp, 1, 2, 5, 12, 60, 12, Q, 7, key, out), "reproject_run");
  CHECK(g_rp.handle == 1);
  g_launches = 0;
  CHECK(RP(c, nullptr, 5, 0, 0, 0, 0, 0, nullptr, 1, nullptr, nullptr) == 0);  // batch == 0 first
  CHECK(g_launches == 0);
  CHECK(RP(nullptr, disp, 0, 2, 5, 12, 80, 16, Q, 1, key, out) < 0);
  REFUSED(c, RP(c, disp, 0, -1, 5, 12, 80, 16, Q, 1, key, out), "batch < 0");
  REFUSED(c, RP(c, nullptr, 0, 2, 5, 12, 80, 16, Q, 1, key, out), null_msg);
  REFUSED(c, RP(c, disp, 0, 2, 5, 12, 80, 16, nullptr, 1, key, out), null_msg);
  REFUSED(c, RP(c, disp, 0, 2, 5, 12, 80, 16, Q, 1, key, nullptr), null_msg);
  REFUSED(c, RP(c, disp, 0, 2, 5, 12, 80, 16, Q, 1, nullptr, out), null_msg);
  const char* f_msg = "reproject_to_3d: is_float32 must be 0 (int16) or 1 (float32)";
  REFUSED(c, RP(c, disp, 2, 2, 5, 12, 80, 16, Q, 1, key, out), f_msg);
  REFUSED(c, RP(c, disp, -1, 2, 5, 12, 80, 16, Q, 1, key, out), f_msg);
  REFUSED(c, RP(c, disp, 0, 2, 0, 12, 80, 16, Q, 1, key, out), "reproject_to_3d: height and width must be >= 1");
  REFUSED(c, RP(c, disp, 0, 2, 5, 0, 80, 16, Q, 1, key, out), "reproject_to_3d: height and width must be >= 1");
  REFUSED(c, RP(c, disp, 0, 1, 46341, 46341, (int64_t)1 << 32, 46341, Q, 1, key, out),
          "reproject_to_3d: height*width exceeds INT32_MAX");
  REFUSED(c, RP(c, disp, 0, 2, 5, 12, 80, 11, Q, 1, key, out), "bad pitch/stride");
  REFUSED(c, RP(c, disp, 0, 2, 5, 12, 79, 16, Q, 1, key, out), "bad pitch/stride");
  REFUSED(c, RP(c, disp, 0, 257, 1, INT32_MAX, INT32_MAX, INT32_MAX, Q, 1, key, out),
          "reproject_to_3d: batch*height*width too large for one launch");

  // the frozen timing table is untouched
  CHECK(fvo_kernel_count() == 36);

  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
  std::printf("dense_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
