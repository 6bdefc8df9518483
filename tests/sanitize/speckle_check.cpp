// Argument validation and workspace arithmetic of the speckle filter's C ABI
// (csrc/capi.cpp) exercised on the host under AddressSanitizer + UndefinedBehaviorSanitizer.
// Linked with csrc/capi.cpp and tests/sanitize/host_stubs.cpp, whose stub of the launcher
// speckle_run records what the entry point passed on (g_spk).  Built and run by
// tests/test_speckle.py.  Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <cstring>

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
  // ---- workspace arithmetic: 8 bytes per pixel, -1 for sizes the filter refuses
  CHECK(fvo_speckle_workspace_bytes(1, 1, 1) == 8);
  CHECK(fvo_speckle_workspace_bytes(3, 200, 320) == 8ll * 3 * 200 * 320);
  CHECK(fvo_speckle_workspace_bytes(64, 600, 960) == 8ll * 64 * 600 * 960);
  CHECK(fvo_speckle_workspace_bytes(0, 600, 960) == 0);
  CHECK(fvo_speckle_workspace_bytes(-1, 600, 960) == -1);
  CHECK(fvo_speckle_workspace_bytes(1, 0, 960) == -1);
  CHECK(fvo_speckle_workspace_bytes(1, 600, 0) == -1);
  CHECK(fvo_speckle_workspace_bytes(1, -600, -960) == -1);
  // batch*height*width beyond 32 bits
  CHECK(fvo_speckle_workspace_bytes(64, 8192, 8192) == 8ll * 64 * 8192 * 8192);
  CHECK(fvo_speckle_workspace_bytes(4, 32768, 32768) == 8ll * 4 * 32768 * 32768);
  // height*width: INT32_MAX is the last size accepted
  CHECK(fvo_speckle_workspace_bytes(1, 1, INT32_MAX) == 8ll * INT32_MAX);
  CHECK(fvo_speckle_workspace_bytes(1, INT32_MAX, 1) == 8ll * INT32_MAX);
  CHECK(fvo_speckle_workspace_bytes(1, 46341, 46341) == -1);  // 46341^2 = 2^31 + 4633
  CHECK(fvo_speckle_workspace_bytes(1, 65536, 32768) == -1);
  CHECK(fvo_speckle_workspace_bytes(1, INT32_MAX, INT32_MAX) == -1);
  // the byte count itself beyond int64
  CHECK(fvo_speckle_workspace_bytes(INT32_MAX, 1, INT32_MAX) == -1);
  CHECK(fvo_speckle_workspace_bytes(1 << 30, 1, INT32_MAX) == -1);                    // 2^64 - 2^33
  CHECK(fvo_speckle_workspace_bytes(1 << 29, 1, INT32_MAX) == INT64_MAX - 0xffffffffll);  // 2^63 - 2^32: the largest
  CHECK(fvo_speckle_workspace_bytes(1 << 28, 1, 1 << 30) == (int64_t)1 << 61);

  // ---- a context (stub device layer), max_batch 4
  fvo_config cfg;
  fvo_config_default(&cfg, 64, 64);
  cfg.max_batch = 4;
  cfg.stages = FVO_STAGE_BF;
  cfg.kp_capacity = 64;
  fvo_ctx* c = nullptr;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  if (!c) return 1;

  // a [3][5][16] buffer of which calls use a 12-wide view; workspace of exactly the needed size
  static int16_t disp[3 * 5 * 16];
  for (int i = 0; i < 3 * 5 * 16; ++i) disp[i] = (int16_t)i;
  const int64_t need = fvo_speckle_workspace_bytes(3, 5, 12);
  CHECK(need == 8 * 3 * 5 * 12);
  alignas(8) static unsigned char ws[8 * 3 * 5 * 12];

  // good call: the launcher is reached with the arguments as given
  CHECK(fvo_filter_speckles(c, disp, 3, 5, 12, 5 * 16, 16, -16, 100, 32, ws, need, nullptr) == 0);
  CHECK(g_launches == 1);
  CHECK(g_spk.batch == 3 && g_spk.H == 5 && g_spk.W == 12 && g_spk.stride == 80 && g_spk.pitch == 16 &&
        g_spk.new_val == -16 && g_spk.max_size == 100 && g_spk.max_diff == 32 && g_spk.ws == ws);
  // int16 extremes of new_val, max_diff 0, a larger workspace, any image size (not the context's)
  g_launches = 0;
  CHECK(fvo_filter_speckles(c, disp, 1, 5, 12, 80, 16, -32768, 1, 0, ws, need + 1, nullptr) == 0);
  CHECK(fvo_filter_speckles(c, disp, 1, 5, 12, 80, 16, 32767, 1, INT32_MAX, ws, need, nullptr) == 0);
  CHECK(fvo_filter_speckles(c, disp, 4, 1, 1, 1, 1, 0, INT32_MAX, 1, ws, 32, nullptr) == 0);
  CHECK(g_launches == 3);

  // no-launch cases
  g_launches = 0;
  CHECK(fvo_filter_speckles(c, disp, 0, 5, 12, 80, 16, -16, 100, 32, ws, need, nullptr) == 0);
  CHECK(fvo_filter_speckles(c, nullptr, 0, 5, 12, 80, 16, -16, 100, 32, nullptr, 0, nullptr) == 0);
  CHECK(fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, 0, 32, ws, need, nullptr) == 0);
  CHECK(fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, -5, 32, ws, need, nullptr) == 0);
  CHECK(g_launches == 0);

  // every error path
  CHECK(fvo_filter_speckles(nullptr, disp, 3, 5, 12, 80, 16, -16, 100, 32, ws, need, nullptr) < 0);
  rejected(c, fvo_filter_speckles(c, nullptr, 3, 5, 12, 80, 16, -16, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, 100, 32, nullptr, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, -1, 5, 12, 80, 16, -16, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 5, 5, 12, 80, 16, -16, 100, 32, ws, need, nullptr));  // > max_batch
  rejected(c, fvo_filter_speckles(c, disp, 3, 0, 12, 80, 16, -16, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 0, 80, 16, -16, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, -5, 12, 80, 16, -16, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 1, 65536, 32768, (int64_t)1 << 31, 32768, -16, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 1, INT32_MAX, INT32_MAX, INT64_MAX, INT32_MAX, -16, 100, 32, ws, need,
                                  nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 11, -16, 100, 32, ws, need, nullptr));  // pitch < width
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 79, 16, -16, 100, 32, ws, need, nullptr));  // stride < pitch*H
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, -80, 16, -16, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, 32768, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -32769, 100, 32, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, 100, -1, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, 100, 32, ws, need - 1, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, 100, 32, ws, 0, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, 100, 32, ws, -1, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, 100, 32, ws + 2, need, nullptr));  // misaligned
  // arguments are checked before the max_speckle_size <= 0 return
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 16, -16, 0, -1, ws, need, nullptr));
  rejected(c, fvo_filter_speckles(c, disp, 3, 5, 12, 80, 11, -16, 0, 32, ws, need, nullptr));

  // the timing names of the new kernels are the last four
  const int nk = fvo_kernel_count();
  CHECK(nk >= 4 && !std::strcmp(fvo_kernel_name(nk - 4), "speckle_local") &&
        !std::strcmp(fvo_kernel_name(nk - 3), "speckle_seams") && !std::strcmp(fvo_kernel_name(nk - 2), "speckle_sum") &&
        !std::strcmp(fvo_kernel_name(nk - 1), "speckle_apply"));

  fvo_destroy(c);
  std::printf("speckle_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
