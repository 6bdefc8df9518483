// Argument validation of the k-nearest-neighbour matcher's and the ratio test's C ABI
// (csrc/capi.cpp) exercised on the host under AddressSanitizer + UndefinedBehaviorSanitizer.
// Linked with csrc/capi.cpp and tests/sanitize/host_stubs.cpp, whose stubs of the launchers
// bf_knn_run / bf_ratio_run record what the entry points passed on (g_bf).  Built and run by
// tests/test_bf_knn.py.  Exit status 0 = all checks passed.
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

// rc must be < 0 with an error message and no launch
static void rejected(fvo_ctx* c, int rc) {
  CHECK(rc < 0);
  CHECK(std::strlen(fvo_last_error(c)) > 0);
  CHECK(g_launches == 0);
}

int main() {
  // ---- a context (stub device layer): max_batch 3, capacity 8
  constexpr int B = 3, CAP = 8;
  fvo_config cfg;
  fvo_config_default(&cfg, 64, 64);
  cfg.max_batch = B;
  cfg.stages = FVO_STAGE_BF;
  cfg.kp_capacity = CAP;
  fvo_ctx* c = nullptr;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  if (!c) return 1;
  CHECK(fvo_kp_capacity(c) == CAP);
  CHECK(fvo_abi_version() == 7);

  alignas(16) static uint8_t q[B * CAP * 32 + 16], t[B * CAP * 32 + 16];
  static int32_t nq[B] = {1, 2, 3}, nt[B] = {4, 5, 6};
  static int32_t knn[B * CAP * FVO_BF_MAX_K * 2], matches[B * CAP * 3], nm[B];
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

  // ---- knn: good calls reach the launcher with the arguments as given, for every k in 1..8
  for (int k = 1; k <= FVO_BF_MAX_K; ++k) {
    g_launches = 0;
    CHECK(fvo_bf_knn_match(c, q, nq, t, nt, B, CAP, k, knn, nullptr) == 0);
    CHECK(g_launches == 1 && g_bf.batch == B && g_bf.cap == CAP && g_bf.k == k && g_bf.q == q &&
          g_bf.t == t && g_bf.out == knn);
  }
  g_launches = 0;
  CHECK(fvo_bf_knn_match(c, q + 16, nq, t + 16, nt, 1, 1, 1, knn, nullptr) == 0);  // 16-byte aligned is enough
  CHECK(g_launches == 1);
  // batch 0: nothing to do, checked before the pointers
  g_launches = 0;
  CHECK(fvo_bf_knn_match(c, nullptr, nullptr, nullptr, nullptr, 0, CAP, 2, nullptr, nullptr) == 0);
  CHECK(fvo_bf_ratio_match(c, nullptr, nullptr, nullptr, nullptr, 0, CAP, 0.75, 1, nullptr, nullptr, nullptr) == 0);
  CHECK(g_launches == 0);
  // refusals
  CHECK(fvo_bf_knn_match(nullptr, q, nq, t, nt, B, CAP, 2, knn, nullptr) < 0);
  for (int k : {0, -1, FVO_BF_MAX_K + 1, INT32_MAX, INT32_MIN}) rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, B, CAP, k, knn, nullptr));
  CHECK(std::strstr(fvo_last_error(c), "k must be") != nullptr);
  rejected(c, fvo_bf_knn_match(c, nullptr, nq, t, nt, B, CAP, 2, knn, nullptr));
  rejected(c, fvo_bf_knn_match(c, q, nullptr, t, nt, B, CAP, 2, knn, nullptr));
  rejected(c, fvo_bf_knn_match(c, q, nq, nullptr, nt, B, CAP, 2, knn, nullptr));
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nullptr, B, CAP, 2, knn, nullptr));
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, B, CAP, 2, nullptr, nullptr));
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, -1, CAP, 2, knn, nullptr));
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, B + 1, CAP, 2, knn, nullptr));   // > max_batch
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, B, CAP + 1, 2, knn, nullptr));   // > the context's capacity
  CHECK(std::strstr(fvo_last_error(c), "cap must be") != nullptr);
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, B, INT32_MAX, 2, knn, nullptr));
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, B, 0, 2, knn, nullptr));
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, B, -CAP, 2, knn, nullptr));
  for (int off : {1, 4, 8, 15}) {
    rejected(c, fvo_bf_knn_match(c, q + off, nq, t, nt, 1, 1, 2, knn, nullptr));
    rejected(c, fvo_bf_knn_match(c, q, nq, t + off, nt, 1, 1, 2, knn, nullptr));
  }
  CHECK(std::strstr(fvo_last_error(c), "aligned") != nullptr);

  // ---- ratio: good calls
  g_launches = 0;
  CHECK(fvo_bf_ratio_match(c, q, nq, t, nt, B, CAP, 0.75, 1, matches, nm, nullptr) == 0);
  CHECK(g_launches == 1 && g_bf.batch == B && g_bf.cap == CAP && g_bf.ratio == 0.75 && g_bf.mutual == 1 &&
        g_bf.q == q && g_bf.t == t && g_bf.out == matches && nm[B - 1] == 9);
  CHECK(fvo_bf_ratio_match(c, q, nq, t, nt, 1, 1, 1e-300, 0, matches, nm, nullptr) == 0);
  CHECK(g_bf.mutual == 0 && g_bf.ratio == 1e-300);
  CHECK(fvo_bf_ratio_match(c, q, nq, t, nt, 2, CAP, 1e300, -7, matches, nm, nullptr) == 0);  // any non-zero = mutual
  CHECK(g_bf.mutual == 1 && g_launches == 3);
  // refusals
  g_launches = 0;
  CHECK(fvo_bf_ratio_match(nullptr, q, nq, t, nt, B, CAP, 0.75, 1, matches, nm, nullptr) < 0);
  for (double r : {0.0, -0.0, -0.75, nan, inf, -inf})
    rejected(c, fvo_bf_ratio_match(c, q, nq, t, nt, B, CAP, r, 1, matches, nm, nullptr));
  CHECK(std::strstr(fvo_last_error(c), "ratio must be") != nullptr);
  rejected(c, fvo_bf_ratio_match(c, nullptr, nq, t, nt, B, CAP, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nullptr, t, nt, B, CAP, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, nullptr, nt, B, CAP, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t, nullptr, B, CAP, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t, nt, B, CAP, 0.75, 1, nullptr, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t, nt, B, CAP, 0.75, 1, matches, nullptr, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t, nt, -1, CAP, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t, nt, B + 1, CAP, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t, nt, B, CAP + 1, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t, nt, B, 0, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q + 8, nq, t, nt, 1, 1, 0.75, 1, matches, nm, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t + 1, nt, 1, 1, 0.75, 1, matches, nm, nullptr));
  fvo_destroy(c);

  // ---- a context without the BF stage serves neither call
  cfg.stages = FVO_STAGE_POSE;
  c = nullptr;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  if (!c) return 1;
  rejected(c, fvo_bf_knn_match(c, q, nq, t, nt, 1, CAP, 2, knn, nullptr));
  rejected(c, fvo_bf_ratio_match(c, q, nq, t, nt, 1, CAP, 0.75, 1, matches, nm, nullptr));
  CHECK(std::strstr(fvo_last_error(c), "stage not enabled") != nullptr);

  // the timing names of the new kernels exist, once each
  int seen_knn = 0, seen_ratio = 0;
  for (int i = 0; i < fvo_kernel_count(); ++i) {
    seen_knn += !std::strcmp(fvo_kernel_name(i), "bf_knn");
    seen_ratio += !std::strcmp(fvo_kernel_name(i), "bf_ratio");
  }
  CHECK(seen_knn == 1 && seen_ratio == 1 && fvo_kernel_count() <= 64);

  fvo_destroy(c);
  std::printf("bf_knn_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
