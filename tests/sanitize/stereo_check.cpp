// Argument validation of the sparse-stereo C ABI (csrc/capi_stereo.cpp: fvo_sparse_stereo,
// fvo_sparse_stereo_workspace_bytes, fvo_sparse_stereo_params_default, fvo_backproject_stereo)
// exercised on the host under AddressSanitizer + UndefinedBehaviorSanitizer.  Linked with
// csrc/capi.cpp, csrc/capi_stereo.cpp and host_stubs.cpp; the stubs of the two launchers are here
// (host_stubs.cpp is shared with programs that do not link capi_stereo.cpp): each records what the
// entry point passed on and touches the first and last element of every buffer as the entry point
// sized it.  Built and run by tests/test_sparse_stereo_cpu.py.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host_stubs.h"

static int g_fail = 0, g_checks = 0;

struct StereoArgs {
  const void *left, *right, *kpL, *kpR, *descL, *descR, *ws, *stereo, *info;
  int batch, cap, pitch;
  int64_t stride;
  fvo_sparse_stereo_params p;
  SparseLevels lv;
  double fx, baseline;
};
static StereoArgs g_ss;
struct BackArgs {
  const void *stereo, *kp1, *matches, *P3;
  int batch, cap;
};
static BackArgs g_bp;

static int hit(const char* name) {
  g_last_launch = name;
  ++g_launches;
  return 0;
}

int sparse_stereo_run(fvo_ctx* c, const uint8_t* left, const uint8_t* right, int batch, int64_t image_stride,
                      int pitch, const float* kpL, const int32_t* nL, const uint8_t* descL, const float* kpR,
                      const int32_t* nR, const uint8_t* descR, int cap, const fvo_sparse_stereo_params& p,
                      const SparseLevels& levels, const double* K, double baseline, void* ws, float* stereo,
                      int32_t* info, hipStream_t) {
  const int W = c->cfg.width, H = c->cfg.height;
  g_ss = StereoArgs{left, right, kpL, kpR, descL, descR, ws, stereo, info, batch, cap, pitch, image_stride, p, levels,
                    K[0], baseline};
  const int64_t last_px = (batch - 1) * image_stride + (int64_t)(H - 1) * pitch + W - 1;
  const int64_t n = (int64_t)batch * cap;
  uint32_t* keys = static_cast<uint32_t*>(ws);
  keys[0] = keys[2 * n - 1] = (uint32_t)(left[0] + right[0] + left[last_px] + right[last_px]);
  stereo[0] = stereo[4 * n - 1] = kpL[0] + kpL[FVO_KP_STRIDE * n - 1] + kpR[0] + kpR[FVO_KP_STRIDE * n - 1] + K[8];
  if (info) info[0] = info[4 * n - 1] = nL[0] + nL[batch - 1] + nR[0] + nR[batch - 1] + descL[0] + descL[32 * n - 1] +
                                        descR[0] + descR[32 * n - 1];
  return hit("sparse_stereo_run");
}
int backproject_stereo_run(fvo_ctx*, const float* stereo, const float* kp1, const int32_t* matches,
                           const int32_t* nmatch, int batch, int cap, float* P3, float* p2, int32_t* npts,
                           hipStream_t) {
  g_bp = BackArgs{stereo, kp1, matches, P3, batch, cap};
  const int64_t n = (int64_t)batch * cap;
  P3[0] = P3[3 * n - 1] = stereo[0] + stereo[4 * n - 1] + kp1[0] + kp1[FVO_KP_STRIDE * n - 1];
  p2[0] = p2[2 * n - 1] = (float)(matches[0] + matches[3 * n - 1]);
  npts[0] = npts[batch - 1] = nmatch[0] + nmatch[batch - 1];
  return hit("backproject_stereo_run");
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
  const float finf = std::numeric_limits<float>::infinity(), fnan = std::nanf("");
  const int W = 40, H = 24, B = 3, CAP = 8;
  fvo_config cfg;
  fvo_config_default(&cfg, W, H);
  cfg.max_batch = B;
  cfg.stages = FVO_STAGE_BF;
  cfg.kp_capacity = 64;
  fvo_ctx* c = nullptr;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  if (!c) return 1;

  // every buffer of exactly the size the call needs (heap: ASan sees one byte too many)
  const int pitch = W + 3;
  const int64_t stride = (int64_t)pitch * H + 5;
  std::vector<uint8_t> left((B - 1) * stride + (H - 1) * pitch + W, 1), right(left.size(), 2);
  std::vector<float> kpL(B * CAP * FVO_KP_STRIDE, 0.f), kpR(kpL.size(), 0.f);
  std::vector<int32_t> nL(B, 1), nR(B, 1);
  // 16-byte aligned descriptor, stereo and info buffers of exactly B * CAP rows: new[] of an over-aligned type
  struct alignas(16) Row16 { uint8_t b[16]; };
  std::vector<Row16> descL_(B * CAP * 2), descR_(B * CAP * 2), stereo_(B * CAP), info_(B * CAP);
  uint8_t* descL = descL_[0].b;
  uint8_t* descR = descR_[0].b;
  float* stereo = reinterpret_cast<float*>(stereo_.data());
  int32_t* info = reinterpret_cast<int32_t*>(info_.data());
  std::memset(descL, 0, 32 * B * CAP);
  std::memset(descR, 0, 32 * B * CAP);
  const int64_t wsb = fvo_sparse_stereo_workspace_bytes(B, CAP);
  CHECK(wsb == 8 * B * CAP);
  std::vector<uint32_t> ws(wsb / 4);
  const double K[9] = {40.0, 0, 20.0, 0, 41.0, 12.0, 0, 0, 1};
  float scale[32];
  for (int i = 0; i < 32; ++i) scale[i] = 1.f + 0.2f * i;

  fvo_sparse_stereo_params def;
  std::memset(&def, 0xAB, sizeof(def));
  fvo_sparse_stereo_params_default(&def);
  CHECK(def.min_disparity == 1.0f && def.max_disparity == 96.0f && def.row_tol == 2.0f && def.max_hamming == 75 &&
        def.max_octave_diff == 1 && def.half_window == 5 && def.half_slide == 5 && def.unique == 1);
  fvo_sparse_stereo_params_default(nullptr);  // ignored

#define SS(ctx, l, r, b, st, pi, kl, nl, dl, kr, nr, dr, cap, pp, sc, nlev, k, w, wb, out, inf) \
  fvo_sparse_stereo(ctx, l, r, b, st, pi, kl, nl, dl, kr, nr, dr, cap, pp, sc, nlev, k, 0.25, w, wb, out, inf, nullptr)
#define SS_P(pp) \
  SS(c, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(), descR, CAP, \
     pp, scale, 8, K, ws.data(), wsb, stereo, info)

  // ---- the valid call, and what reaches the launcher
  ACCEPTED(SS_P(&def), "sparse_stereo_run");
  CHECK(g_ss.left == left.data() && g_ss.right == right.data() && g_ss.kpL == kpL.data() && g_ss.kpR == kpR.data() &&
        g_ss.descL == descL && g_ss.descR == descR && g_ss.ws == ws.data() && g_ss.stereo == stereo &&
        g_ss.info == info && g_ss.batch == B && g_ss.cap == CAP && g_ss.pitch == pitch && g_ss.stride == stride &&
        g_ss.fx == 40.0 && g_ss.baseline == 0.25);
  CHECK(g_ss.lv.n == 8 && g_ss.lv.scale[0] == 1.f && g_ss.lv.scale[7] == scale[7] && g_ss.lv.scale[8] == 0.f &&
        !std::memcmp(&g_ss.p, &def, sizeof(def)));
  ACCEPTED(SS(c, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(), descR,
              CAP, &def, scale, 8, K, ws.data(), wsb, stereo, nullptr), "sparse_stereo_run");  // info is optional
  CHECK(g_ss.info == nullptr);
  {  // the tightest image layout
    std::vector<uint8_t> l(W * H * B, 1), r(W * H * B, 1);
    ACCEPTED(SS(c, l.data(), r.data(), B, W * H, W, kpL.data(), nL.data(), descL, kpR.data(), nR.data(), descR, CAP, &def,
                scale, 8, K, ws.data(), wsb, stereo, info), "sparse_stereo_run");
    REFUSED(c, SS(c, l.data(), r.data(), B, W * H, W - 1, kpL.data(), nL.data(), descL, kpR.data(), nR.data(), descR, CAP,
                  &def, scale, 8, K, ws.data(), wsb, stereo, info), "bad pitch/stride");
    REFUSED(c, SS(c, l.data(), r.data(), B, W * H - 1, W, kpL.data(), nL.data(), descL, kpR.data(), nR.data(), descR, CAP,
                  &def, scale, 8, K, ws.data(), wsb, stereo, info), "bad pitch/stride");
  }
  g_launches = 0;
  CHECK(SS(c, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0,
           nullptr, nullptr, 0, nullptr, nullptr) == 0 && g_launches == 0);  // batch == 0 first
  CHECK(SS(nullptr, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(),
           descR, CAP, &def, scale, 8, K, ws.data(), wsb, stereo, info) < 0);
  for (int b : {B + 1, -1})
    REFUSED(c, SS(c, left.data(), right.data(), b, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(),
                  descR, CAP, &def, scale, 8, K, ws.data(), wsb, stereo, info), "batch exceeds max_batch");

  // ---- NULL pointers, one at a time
  const char* null_msg = "null pointer argument";
  for (int k = 0; k < 13; ++k) {
    auto z = [&](int i, auto* p) { return i == k ? nullptr : p; };
    REFUSED(c, SS(c, z(0, left.data()), z(1, right.data()), B, stride, pitch, z(2, kpL.data()), z(3, nL.data()),
                  z(4, descL), z(5, kpR.data()), z(6, nR.data()), z(7, descR), CAP, z(8, &def), z(9, scale), 8,
                  z(10, K), z(11, (void*)ws.data()), wsb, z(12, stereo), info), null_msg);
  }

  // ---- the parameters: every refusal with the accepted bound beside it
  auto with = [&](auto set) {
    fvo_sparse_stereo_params p = def;
    set(p);
    return p;
  };
  fvo_sparse_stereo_params p;
  const char* min_msg = "sparse_stereo: min_disparity must be finite and > 0";
  for (float v : {0.f, -1.f, finf, -finf, fnan}) {
    p = with([&](auto& q) { q.min_disparity = v; q.max_disparity = finf; });
    REFUSED(c, SS_P(&p), min_msg);
  }
  p = with([&](auto& q) { q.min_disparity = std::numeric_limits<float>::denorm_min(); });
  ACCEPTED(SS_P(&p), "sparse_stereo_run");
  const char* max_msg = "sparse_stereo: max_disparity must be >= min_disparity";
  p = with([&](auto& q) { q.min_disparity = 4.f; q.max_disparity = std::nextafterf(4.f, 0.f); });
  REFUSED(c, SS_P(&p), max_msg);
  p = with([&](auto& q) { q.max_disparity = fnan; });
  REFUSED(c, SS_P(&p), max_msg);
  p = with([&](auto& q) { q.min_disparity = 4.f; q.max_disparity = 4.f; });
  ACCEPTED(SS_P(&p), "sparse_stereo_run");
  p = with([&](auto& q) { q.max_disparity = finf; });
  ACCEPTED(SS_P(&p), "sparse_stereo_run");
  const char* tol_msg = "sparse_stereo: row_tol must be finite and >= 0";
  for (float v : {-1e-30f, finf, fnan}) {
    p = with([&](auto& q) { q.row_tol = v; });
    REFUSED(c, SS_P(&p), tol_msg);
  }
  p = with([&](auto& q) { q.row_tol = 0.f; });
  ACCEPTED(SS_P(&p), "sparse_stereo_run");
  const char* ham_msg = "sparse_stereo: max_hamming must be in [0, 256]";
  for (int v : {-1, 257, INT32_MIN, INT32_MAX}) {
    p = with([&](auto& q) { q.max_hamming = v; });
    REFUSED(c, SS_P(&p), ham_msg);
  }
  for (int v : {0, 256}) {
    p = with([&](auto& q) { q.max_hamming = v; });
    ACCEPTED(SS_P(&p), "sparse_stereo_run");
  }
  const char* w_msg = "sparse_stereo: half_window must be in [1, 7]";
  for (int v : {0, 8, -1, INT32_MAX}) {
    p = with([&](auto& q) { q.half_window = v; });
    REFUSED(c, SS_P(&p), w_msg);
  }
  for (int v : {1, 7}) {
    p = with([&](auto& q) { q.half_window = v; });
    ACCEPTED(SS_P(&p), "sparse_stereo_run");
  }
  const char* s_msg = "sparse_stereo: half_slide must be in [1, 8]";
  for (int v : {0, 9, -1, INT32_MAX}) {
    p = with([&](auto& q) { q.half_slide = v; });
    REFUSED(c, SS_P(&p), s_msg);
  }
  for (int v : {1, 8}) {
    p = with([&](auto& q) { q.half_slide = v; });
    ACCEPTED(SS_P(&p), "sparse_stereo_run");
  }
  p = with([&](auto& q) { q.max_octave_diff = -1; });
  REFUSED(c, SS_P(&p), "sparse_stereo: max_octave_diff must be >= 0");
  for (int v : {0, INT32_MAX}) {
    p = with([&](auto& q) { q.max_octave_diff = v; });
    ACCEPTED(SS_P(&p), "sparse_stereo_run");
  }
  p = with([&](auto& q) { q.unique = -7; });  // any non-zero value means "on"
  ACCEPTED(SS_P(&p), "sparse_stereo_run");

  // ---- n_levels, cap, the workspace
#define SS_N(nlev, cap, w, wb) \
  SS(c, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(), descR, cap, \
     &def, scale, nlev, K, w, wb, stereo, info)
  const char* lev_msg = "sparse_stereo: n_levels must be in [1, 32]";
  for (int v : {0, 33, -1}) REFUSED(c, SS_N(v, CAP, ws.data(), wsb), lev_msg);
  for (int v : {1, 32}) {
    ACCEPTED(SS_N(v, CAP, ws.data(), wsb), "sparse_stereo_run");
    CHECK(g_ss.lv.n == v && g_ss.lv.scale[v - 1] == scale[v - 1]);
  }
  const char* cap_msg = "sparse_stereo: cap must be in [1, 65535]";
  for (int v : {0, -1, 65536, INT32_MAX}) REFUSED(c, SS_N(8, v, ws.data(), INT64_MAX), cap_msg);
  ACCEPTED(SS_N(8, 1, ws.data(), 8 * B), "sparse_stereo_run");  // cap 1: every buffer is larger than needed
  CHECK(fvo_sparse_stereo_workspace_bytes(B, 0) == -1 && fvo_sparse_stereo_workspace_bytes(B, 65536) == -1 &&
        fvo_sparse_stereo_workspace_bytes(-1, CAP) == -1 && fvo_sparse_stereo_workspace_bytes(0, CAP) == 0 &&
        fvo_sparse_stereo_workspace_bytes(1, 65535) == 8 * 65535 &&
        fvo_sparse_stereo_workspace_bytes(INT32_MAX, 65535) == 8 * (int64_t)INT32_MAX * 65535);
  const char* ws_msg = "sparse_stereo: workspace too small";
  REFUSED(c, SS_N(8, CAP, ws.data(), wsb - 1), ws_msg);
  REFUSED(c, SS_N(8, CAP, ws.data(), 0), ws_msg);
  REFUSED(c, SS_N(8, CAP, ws.data(), -1), ws_msg);
  {
    std::vector<uint32_t> big(wsb / 4 + 1);
    ACCEPTED(SS_N(8, CAP, big.data(), wsb + 4), "sparse_stereo_run");
    REFUSED(c, SS_N(8, CAP, reinterpret_cast<char*>(big.data()) + 1, wsb), "sparse_stereo: workspace must be 4-byte aligned");
  }
  // ---- alignment of the descriptor and output buffers
  {
    std::vector<Row16> d(B * CAP * 2 + 1), o(B * CAP + 1);
    REFUSED(c, SS(c, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), d[0].b + 4, kpR.data(), nR.data(),
                  descR, CAP, &def, scale, 8, K, ws.data(), wsb, stereo, info), "descriptor buffers must be 16-byte aligned");
    REFUSED(c, SS(c, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(),
                  d[0].b + 8, CAP, &def, scale, 8, K, ws.data(), wsb, stereo, info), "descriptor buffers must be 16-byte aligned");
    const char* al_msg = "sparse_stereo: stereo and info must be 16-byte aligned";
    REFUSED(c, SS(c, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(),
                  descR, CAP, &def, scale, 8, K, ws.data(), wsb, reinterpret_cast<float*>(o[0].b + 4), info), al_msg);
    REFUSED(c, SS(c, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(),
                  descR, CAP, &def, scale, 8, K, ws.data(), wsb, stereo, reinterpret_cast<int32_t*>(o[0].b + 8)), al_msg);
  }

  // ---- fvo_backproject_stereo
  std::vector<float> kp1(B * CAP * FVO_KP_STRIDE, 0.f), P3(B * CAP * 3), p2(B * CAP * 2);
  std::vector<int32_t> matches(B * CAP * 3, 0), nm(B, 0), npts(B);
#define BP(ctx, st, k0, k1, m, n, b, cap, a3, a2, np) fvo_backproject_stereo(ctx, st, k0, k1, m, n, b, cap, a3, a2, np, nullptr)
  ACCEPTED(BP(c, stereo, kpL.data(), kp1.data(), matches.data(), nm.data(), B, CAP, P3.data(), p2.data(), npts.data()),
           "backproject_stereo_run");
  CHECK(g_bp.stereo == stereo && g_bp.kp1 == kp1.data() && g_bp.matches == matches.data() && g_bp.P3 == P3.data() &&
        g_bp.batch == B && g_bp.cap == CAP);
  ACCEPTED(BP(c, stereo, nullptr, kp1.data(), matches.data(), nm.data(), B, CAP, P3.data(), p2.data(), npts.data()),
           "backproject_stereo_run");  // kp0 is not read
  g_launches = 0;
  CHECK(BP(c, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == 0 && g_launches == 0);
  CHECK(BP(nullptr, stereo, nullptr, kp1.data(), matches.data(), nm.data(), B, CAP, P3.data(), p2.data(), npts.data()) < 0);
  for (int b : {B + 1, -1})
    REFUSED(c, BP(c, stereo, nullptr, kp1.data(), matches.data(), nm.data(), b, CAP, P3.data(), p2.data(), npts.data()),
            "batch exceeds max_batch");
  for (int k = 0; k < 7; ++k) {
    auto z = [&](int i, auto* q) { return i == k ? nullptr : q; };
    REFUSED(c, BP(c, z(0, stereo), nullptr, z(1, kp1.data()), z(2, matches.data()), z(3, nm.data()), B, CAP,
                  z(4, P3.data()), z(5, p2.data()), z(6, npts.data())), null_msg);
  }
  for (int v : {0, -1})
    REFUSED(c, BP(c, stereo, nullptr, kp1.data(), matches.data(), nm.data(), B, v, P3.data(), p2.data(), npts.data()),
            "cap must be >= 1");
  REFUSED(c, BP(c, stereo + 1, nullptr, kp1.data(), matches.data(), nm.data(), B, CAP, P3.data(), p2.data(), npts.data()),
          "stereo buffer must be 16-byte aligned");

  // ---- a context without an image size
  {
    fvo_config z;
    fvo_config_default(&z, 0, H);
    z.max_batch = B;
    z.stages = FVO_STAGE_BF;
    z.kp_capacity = 64;
    fvo_ctx* e = nullptr;
    CHECK(fvo_create(0, &z, &e) == 0 && e != nullptr);
    if (!e) return 1;
    REFUSED(e, SS(e, left.data(), right.data(), B, stride, pitch, kpL.data(), nL.data(), descL, kpR.data(), nR.data(),
                  descR, CAP, &def, scale, 8, K, ws.data(), wsb, stereo, info),
            "sparse_stereo: the context's width and height must be >= 1");
    fvo_destroy(e);
  }

  // the frozen timing table and the ABI are untouched
  CHECK(fvo_kernel_count() == 36);
  CHECK(fvo_abi_version() == 7);
  CHECK(fvo_config_size() == 31 * 4);

  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
  std::printf("stereo_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
