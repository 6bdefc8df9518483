// Argument validation of the normal-estimation C ABI (csrc/capi_normals.cpp: fvo_normals_workspace_bytes,
// fvo_estimate_normals, fvo_orient_normals) exercised on the host under AddressSanitizer +
// UndefinedBehaviorSanitizer.  Linked with csrc/capi.cpp, csrc/capi_normals.cpp and host_stubs.cpp; the
// stubs of the launchers are here: each records what the entry point passed on and touches the first
// and last element of every buffer as the entry point sized it.  Built and run by
// tests/test_normals_cpu.py.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host_stubs.h"

static int g_fail = 0, g_checks = 0;

struct EstArgs {
  const void *pts, *ws, *normals, *cov, *cnt, *stats, *status;
  int64_t n;
  int max_nn, rings, prior;
  double radius, cell;
};
static EstArgs g_est;
struct OriArgs {
  const void *pts, *normals;
  int64_t n;
  int mode;
  double ref[3];
};
static OriArgs g_ori;

static int hit(const char* name) {
  g_last_launch = name;
  ++g_launches;
  return 0;
}

int64_t normals_workspace_bytes(int64_t n) { return n < 1 ? -1 : 64 * n + 8192; }

int estimate_normals_run(fvo_ctx*, const double* pts, int64_t n, int max_nn, double radius, double cell, int max_rings,
                         void* ws, double* normals, int has_prior, double* cov, int32_t* cnt, int32_t* stats,
                         int32_t* status, hipStream_t) {
  g_est = EstArgs{pts, ws, normals, cov, cnt, stats, status, n, max_nn, max_rings, has_prior, radius, cell};
  char* w = static_cast<char*>(ws);
  w[0] = w[normals_workspace_bytes(n) - 1] = 1;
  normals[0] = normals[3 * n - 1] = pts[0] + pts[3 * n - 1];
  if (cov) cov[0] = cov[9 * n - 1] = 0.0;
  if (cnt) cnt[0] = cnt[n - 1] = 0;
  stats[0] = stats[1] = 0;
  if (status) status[0] = 0;
  return hit("estimate_normals_run");
}
int orient_normals_run(fvo_ctx*, const double* pts, double* normals, int64_t n, int mode, const double* ref,
                       hipStream_t) {
  g_ori = OriArgs{pts, normals, n, mode, {ref[0], ref[1], ref[2]}};
  normals[0] = normals[3 * n - 1] = pts[0] + pts[3 * n - 1];
  return hit("orient_normals_run");
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

// rc must be 0 with nothing launched (n_points == 0)
#define NOTHING(call)                                  \
  do {                                                 \
    g_launches = 0;                                    \
    CHECK((call) == 0);                                \
    CHECK(g_launches == 0);                            \
  } while (0)

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const double tiny = std::numeric_limits<double>::denorm_min(), big = std::numeric_limits<double>::max();
  const int64_t N = 37;
  fvo_config cfg;
  fvo_config_default(&cfg, 64, 64);
  cfg.max_batch = 1;
  cfg.stages = FVO_STAGE_BF;
  cfg.kp_capacity = 64;
  fvo_ctx* c = nullptr;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  if (!c) return 1;

  // every buffer of exactly the size the call needs (heap: ASan sees one byte too many)
  std::vector<double> pts(3 * N, 1.0), nrm(3 * N), cov(9 * N);
  std::vector<int32_t> cnt(N), stats(2), status(1);
  const int64_t wsb = fvo_normals_workspace_bytes(N, 30);
  CHECK(wsb == 64 * N + 8192);
  std::vector<double> ws_(wsb / 8);
  void* ws = ws_.data();

  // ---- fvo_normals_workspace_bytes
  CHECK(fvo_normals_workspace_bytes(N, 1) == wsb && fvo_normals_workspace_bytes(N, 64) == wsb);
  CHECK(fvo_normals_workspace_bytes(N, 0) == -1 && fvo_normals_workspace_bytes(N, 65) == -1 &&
        fvo_normals_workspace_bytes(N, -1) == -1);
  CHECK(fvo_normals_workspace_bytes(-1, 30) == -1 && fvo_normals_workspace_bytes((int64_t)INT32_MAX + 1, 30) == -1);
  CHECK(fvo_normals_workspace_bytes(0, 30) == 0);
  CHECK(fvo_normals_workspace_bytes(INT32_MAX, 30) == 64 * (int64_t)INT32_MAX + 8192);

  // ---- fvo_estimate_normals
#define EST(ctx, p, n, k, rad, cell, rings, w, wb, nr, pri, cv, cn, stt, sta) \
  fvo_estimate_normals(ctx, p, n, k, rad, cell, rings, w, wb, nr, pri, cv, cn, stt, sta, nullptr)
#define EST_V(k, rad, cell, rings) \
  EST(c, pts.data(), N, k, rad, cell, rings, ws, wsb, nrm.data(), 0, cov.data(), cnt.data(), stats.data(), status.data())
  const char* run = "estimate_normals_run";
  ACCEPTED(EST_V(30, 1.5, 0.5, 2), run);
  CHECK(g_est.pts == pts.data() && g_est.ws == ws && g_est.normals == nrm.data() && g_est.cov == cov.data() &&
        g_est.cnt == cnt.data() && g_est.stats == stats.data() && g_est.status == status.data() && g_est.n == N &&
        g_est.max_nn == 30 && g_est.rings == 2 && g_est.prior == 0 && g_est.radius == 1.5 && g_est.cell == 0.5);
  ACCEPTED(EST(c, pts.data(), N, 30, inf, 1.0, 2, ws, wsb, nrm.data(), 7, nullptr, nullptr, stats.data(), nullptr), run);
  CHECK(g_est.cov == nullptr && g_est.cnt == nullptr && g_est.status == nullptr && g_est.prior == 1 &&
        g_est.radius == inf);  // covariances, n_neighbors and status are optional; +inf is the k-NN search
  CHECK(EST(nullptr, pts.data(), N, 30, 1.5, 0.5, 2, ws, wsb, nrm.data(), 0, cov.data(), cnt.data(), stats.data(),
            status.data()) < 0);
  const char* null_msg = "null pointer argument";
  for (int k = 0; k < 4; ++k) {
    auto z = [&](int i, auto* p) { return i == k ? nullptr : p; };
    REFUSED(c, EST(c, z(0, pts.data()), N, 30, 1.5, 0.5, 2, z(1, ws), wsb, z(2, nrm.data()), 0, cov.data(), cnt.data(),
                   z(3, stats.data()), status.data()), null_msg);
  }
  const char* n_msg = "n_points out of range";
  REFUSED(c, EST(c, pts.data(), -1, 30, 1.5, 0.5, 2, ws, wsb, nrm.data(), 0, cov.data(), cnt.data(), stats.data(),
                 status.data()), n_msg);
  REFUSED(c, EST(c, pts.data(), (int64_t)INT32_MAX + 1, 30, 1.5, 0.5, 2, ws, wsb, nrm.data(), 0, cov.data(),
                 cnt.data(), stats.data(), status.data()), n_msg);
  const char* k_msg = "estimate_normals: max_nn must be in [1, 64]";
  for (int v : {0, 65, -1, INT32_MAX, INT32_MIN}) REFUSED(c, EST_V(v, 1.5, 0.5, 2), k_msg);
  for (int v : {1, 64}) {
    ACCEPTED(EST_V(v, 1.5, 0.5, 2), run);
    CHECK(g_est.max_nn == v);
  }
  const char* rad_msg = "estimate_normals: radius must be > 0";
  for (double v : {0.0, -0.0, -1.0, -inf, nan}) REFUSED(c, EST_V(30, v, 0.5, 2), rad_msg);
  for (double v : {tiny, big, inf}) {
    ACCEPTED(EST_V(30, v, 0.5, 2), run);
    CHECK(g_est.radius == v);
  }
  const char* cell_msg = "estimate_normals: cell must be finite and > 0";
  for (double v : {0.0, -1.0, inf, -inf, nan}) REFUSED(c, EST_V(30, 1.5, v, 2), cell_msg);
  for (double v : {tiny, big}) ACCEPTED(EST_V(30, 1.5, v, 2), run);
  const char* ring_msg = "estimate_normals: max_rings must be in [0, 8]";
  for (int v : {-1, 9, INT32_MAX, INT32_MIN}) REFUSED(c, EST_V(30, 1.5, 0.5, v), ring_msg);
  for (int v : {0, 8}) {
    ACCEPTED(EST_V(30, 1.5, 0.5, v), run);
    CHECK(g_est.rings == v);
  }
  const char* ws_msg = "estimate_normals: workspace too small";
  for (int64_t v : {wsb - 1, (int64_t)0, (int64_t)-1})
    REFUSED(c, EST(c, pts.data(), N, 30, 1.5, 0.5, 2, ws, v, nrm.data(), 0, cov.data(), cnt.data(), stats.data(),
                   status.data()), ws_msg);
  {
    std::vector<double> more(wsb / 8 + 1);
    ACCEPTED(EST(c, pts.data(), N, 30, 1.5, 0.5, 2, more.data(), wsb + 8, nrm.data(), 0, cov.data(), cnt.data(),
                 stats.data(), status.data()), run);
    REFUSED(c, EST(c, pts.data(), N, 30, 1.5, 0.5, 2, reinterpret_cast<char*>(more.data()) + 4, wsb, nrm.data(), 0,
                   cov.data(), cnt.data(), stats.data(), status.data()),
            "estimate_normals: workspace must be 8-byte aligned");
  }
  // n_points == 0: the checks still run, nothing is launched, the data pointers may be NULL
  NOTHING(EST(c, nullptr, 0, 30, 1.5, 0.5, 2, nullptr, 0, nullptr, 0, nullptr, nullptr, stats.data(), nullptr));
  NOTHING(EST(c, pts.data(), 0, 30, 1.5, 0.5, 2, ws, wsb, nrm.data(), 1, cov.data(), cnt.data(), stats.data(),
              status.data()));
  REFUSED(c, EST(c, nullptr, 0, 30, 1.5, 0.5, 2, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr), null_msg);
  REFUSED(c, EST(c, nullptr, 0, 0, 1.5, 0.5, 2, nullptr, 0, nullptr, 0, nullptr, nullptr, stats.data(), nullptr), k_msg);
  REFUSED(c, EST(c, nullptr, 0, 30, nan, 0.5, 2, nullptr, 0, nullptr, 0, nullptr, nullptr, stats.data(), nullptr),
          rad_msg);
  REFUSED(c, EST(c, nullptr, 0, 30, 1.5, 0.0, 2, nullptr, 0, nullptr, 0, nullptr, nullptr, stats.data(), nullptr),
          cell_msg);
  REFUSED(c, EST(c, nullptr, 0, 30, 1.5, 0.5, 9, nullptr, 0, nullptr, 0, nullptr, nullptr, stats.data(), nullptr),
          ring_msg);
  {  // a single point
    std::vector<double> p1(3, 0.5), n1(3), c1(9), w1(fvo_normals_workspace_bytes(1, 30) / 8);
    std::vector<int32_t> k1(1);
    ACCEPTED(EST(c, p1.data(), 1, 30, inf, 1.0, 2, w1.data(), (int64_t)w1.size() * 8, n1.data(), 0, c1.data(),
                 k1.data(), stats.data(), status.data()), run);
  }

  // ---- fvo_orient_normals
#define ORI(ctx, p, nr, n, mode, ref) fvo_orient_normals(ctx, p, nr, n, mode, ref, nullptr)
  const char* orun = "orient_normals_run";
  std::vector<double> ref{1.0, -2.0, 3.0};
  ACCEPTED(ORI(c, pts.data(), nrm.data(), N, 0, ref.data()), orun);
  CHECK(g_ori.pts == pts.data() && g_ori.normals == nrm.data() && g_ori.n == N && g_ori.mode == 0 &&
        g_ori.ref[0] == 1.0 && g_ori.ref[1] == -2.0 && g_ori.ref[2] == 3.0);
  ACCEPTED(ORI(c, pts.data(), nrm.data(), N, 1, ref.data()), orun);
  CHECK(g_ori.mode == 1);
  CHECK(ORI(nullptr, pts.data(), nrm.data(), N, 0, ref.data()) < 0);
  for (int k = 0; k < 3; ++k) {
    auto z = [&](int i, auto* p) { return i == k ? nullptr : p; };
    REFUSED(c, ORI(c, z(0, pts.data()), z(1, nrm.data()), N, 0, z(2, ref.data())), null_msg);
  }
  REFUSED(c, ORI(c, pts.data(), nrm.data(), -1, 0, ref.data()), n_msg);
  REFUSED(c, ORI(c, pts.data(), nrm.data(), (int64_t)INT32_MAX + 1, 0, ref.data()), n_msg);
  for (int v : {-1, 2, INT32_MAX, INT32_MIN})
    REFUSED(c, ORI(c, pts.data(), nrm.data(), N, v, ref.data()), "orient_normals: mode must be 0 or 1");
  for (int a = 0; a < 3; ++a)
    for (double v : {inf, -inf, nan})
      for (int mode : {0, 1}) {
        std::vector<double> r{1.0, 1.0, 1.0};
        r[a] = v;
        REFUSED(c, ORI(c, pts.data(), nrm.data(), N, mode, r.data()), "orient_normals: ref must be finite");
      }
  {
    std::vector<double> zero{0.0, -0.0, 0.0}, nearly{0.0, 0.0, tiny}, far{big, -big, big};
    REFUSED(c, ORI(c, pts.data(), nrm.data(), N, 1, zero.data()), "orient_normals: direction must not be all zeros");
    ACCEPTED(ORI(c, pts.data(), nrm.data(), N, 0, zero.data()), orun);  // a camera at the origin
    ACCEPTED(ORI(c, pts.data(), nrm.data(), N, 1, nearly.data()), orun);
    ACCEPTED(ORI(c, pts.data(), nrm.data(), N, 1, far.data()), orun);
    ACCEPTED(ORI(c, pts.data(), nrm.data(), N, 0, far.data()), orun);
    NOTHING(ORI(c, nullptr, nullptr, 0, 0, ref.data()));
    NOTHING(ORI(c, pts.data(), nrm.data(), 0, 1, ref.data()));
    REFUSED(c, ORI(c, nullptr, nullptr, 0, 0, nullptr), null_msg);
    REFUSED(c, ORI(c, nullptr, nullptr, 0, 2, ref.data()), "orient_normals: mode must be 0 or 1");
    REFUSED(c, ORI(c, nullptr, nullptr, 0, 1, zero.data()), "orient_normals: direction must not be all zeros");
  }
  {  // a single point
    std::vector<double> p1(3, 0.5), n1(3);
    ACCEPTED(ORI(c, p1.data(), n1.data(), 1, 0, ref.data()), orun);
  }

  // the calls run on any stage: a context with no stage at all
  {
    fvo_config z;
    fvo_config_default(&z, 64, 64);
    z.max_batch = 1;
    z.stages = 0;
    fvo_ctx* e = nullptr;
    if (fvo_create(0, &z, &e) == 0 && e) {
      ACCEPTED(EST(e, pts.data(), N, 30, 1.5, 0.5, 2, ws, wsb, nrm.data(), 0, cov.data(), cnt.data(), stats.data(),
                   status.data()), run);
      ACCEPTED(ORI(e, pts.data(), nrm.data(), N, 0, ref.data()), orun);
      fvo_destroy(e);
    }
  }

  // the frozen timing table and the ABI are untouched
  CHECK(fvo_kernel_count() == 36);
  CHECK(fvo_abi_version() == 7);
  CHECK(fvo_config_size() == 31 * 4);

  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
  std::printf("normals_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
