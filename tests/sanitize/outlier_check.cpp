// Argument validation of the outlier-removal C ABI (csrc/capi_outlier.cpp: fvo_outlier_workspace_bytes,
// fvo_statistical_outliers, fvo_radius_outliers, fvo_select_points) exercised on the host under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Linked with csrc/capi.cpp, csrc/capi_outlier.cpp
// and host_stubs.cpp; the stubs of the launchers are here (host_stubs.cpp is shared with programs
// that do not link capi_outlier.cpp): each records what the entry point passed on and touches the
// first and last element of every buffer as the entry point sized it.  Built and run by
// tests/test_outlier_cpu.py.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host_stubs.h"

static int g_fail = 0, g_checks = 0;

struct StatArgs {
  const void *pts, *ws, *keep, *avg, *stats, *status;
  int64_t n;
  int k, rings;
  double ratio, cell;
};
static StatArgs g_st;
struct RadArgs {
  const void *pts, *ws, *keep, *cnt, *status;
  int64_t n;
  int nb;
  double radius, cell;
};
static RadArgs g_rad;
struct SelArgs {
  const void *pts, *keep, *o64, *o32, *n_out;
  int64_t n;
};
static SelArgs g_sel;

static int hit(const char* name) {
  g_last_launch = name;
  ++g_launches;
  return 0;
}

int64_t outlier_workspace_bytes(int64_t n) { return n < 1 ? -1 : 96 * n + 8192; }

int statistical_outliers_run(fvo_ctx*, const double* pts, int64_t n, int nb_neighbors, double std_ratio, double cell,
                             int max_rings, void* ws, uint8_t* keep, double* avg, double* stats, int32_t* status,
                             hipStream_t) {
  g_st = StatArgs{pts, ws, keep, avg, stats, status, n, nb_neighbors, max_rings, std_ratio, cell};
  char* w = static_cast<char*>(ws);
  w[0] = w[outlier_workspace_bytes(n) - 1] = 1;
  keep[0] = keep[n - 1] = (uint8_t)(pts[0] + pts[3 * n - 1]);
  if (avg) avg[0] = avg[n - 1] = 0.0;
  stats[0] = stats[5] = 0.0;
  if (status) status[0] = 0;
  return hit("statistical_outliers_run");
}
int radius_outliers_run(fvo_ctx*, const double* pts, int64_t n, int nb_points, double radius, double cell, void* ws,
                        uint8_t* keep, int32_t* n_neighbors, int32_t* status, hipStream_t) {
  g_rad = RadArgs{pts, ws, keep, n_neighbors, status, n, nb_points, radius, cell};
  char* w = static_cast<char*>(ws);
  w[0] = w[outlier_workspace_bytes(n) - 1] = 1;
  keep[0] = keep[n - 1] = (uint8_t)(pts[0] + pts[3 * n - 1]);
  if (n_neighbors) n_neighbors[0] = n_neighbors[n - 1] = 0;
  if (status) status[0] = 0;
  return hit("radius_outliers_run");
}
int select_points_run(fvo_ctx*, const double* pts, int64_t n, const uint8_t* keep, double* out64, float* out32,
                      int32_t* n_out, hipStream_t) {
  g_sel = SelArgs{pts, keep, out64, out32, n_out, n};
  const double v = pts[0] + pts[3 * n - 1] + keep[0] + keep[n - 1];
  if (out64) out64[0] = out64[3 * n - 1] = v;
  if (out32) out32[0] = out32[3 * n - 1] = (float)v;
  n_out[0] = 0;
  return hit("select_points_run");
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
  const double tiny = std::numeric_limits<double>::denorm_min();
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
  std::vector<double> pts(3 * N, 1.0), avg(N), stats(6), out64(3 * N);
  std::vector<float> out32(3 * N);
  std::vector<uint8_t> keep(N, 1);
  std::vector<int32_t> cnt(N), status(1), n_out(1);
  const int64_t wsb = fvo_outlier_workspace_bytes(N, 20);
  CHECK(wsb == 96 * N + 8192);
  std::vector<double> ws_(wsb / 8);
  void* ws = ws_.data();

  // ---- fvo_outlier_workspace_bytes
  CHECK(fvo_outlier_workspace_bytes(N, 1) == wsb && fvo_outlier_workspace_bytes(N, 64) == wsb);
  CHECK(fvo_outlier_workspace_bytes(N, 0) == -1 && fvo_outlier_workspace_bytes(N, 65) == -1 &&
        fvo_outlier_workspace_bytes(N, -1) == -1);
  CHECK(fvo_outlier_workspace_bytes(-1, 20) == -1 && fvo_outlier_workspace_bytes((int64_t)INT32_MAX + 1, 20) == -1);
  CHECK(fvo_outlier_workspace_bytes(0, 20) == 0);
  CHECK(fvo_outlier_workspace_bytes(INT32_MAX, 20) == 96 * (int64_t)INT32_MAX + 8192);

  // ---- fvo_statistical_outliers
#define ST(ctx, p, n, k, ratio, cell, rings, w, wb, kp, av, stt, sta) \
  fvo_statistical_outliers(ctx, p, n, k, ratio, cell, rings, w, wb, kp, av, stt, sta, nullptr)
#define ST_V(k, ratio, cell, rings) \
  ST(c, pts.data(), N, k, ratio, cell, rings, ws, wsb, keep.data(), avg.data(), stats.data(), status.data())
  ACCEPTED(ST_V(20, 2.0, 1.0, 2), "statistical_outliers_run");
  CHECK(g_st.pts == pts.data() && g_st.ws == ws && g_st.keep == keep.data() && g_st.avg == avg.data() &&
        g_st.stats == stats.data() && g_st.status == status.data() && g_st.n == N && g_st.k == 20 &&
        g_st.rings == 2 && g_st.ratio == 2.0 && g_st.cell == 1.0);
  ACCEPTED(ST(c, pts.data(), N, 20, 2.0, 1.0, 2, ws, wsb, keep.data(), nullptr, stats.data(), nullptr),
           "statistical_outliers_run");  // avg_distance and status are optional
  CHECK(g_st.avg == nullptr && g_st.status == nullptr);
  CHECK(ST(nullptr, pts.data(), N, 20, 2.0, 1.0, 2, ws, wsb, keep.data(), avg.data(), stats.data(), status.data()) < 0);
  const char* null_msg = "null pointer argument";
  for (int k = 0; k < 4; ++k) {
    auto z = [&](int i, auto* p) { return i == k ? nullptr : p; };
    REFUSED(c, ST(c, z(0, pts.data()), N, 20, 2.0, 1.0, 2, z(1, ws), wsb, z(2, keep.data()), avg.data(),
                  z(3, stats.data()), status.data()), null_msg);
  }
  const char* n_msg = "n_points out of range";
  REFUSED(c, ST(c, pts.data(), -1, 20, 2.0, 1.0, 2, ws, wsb, keep.data(), avg.data(), stats.data(), status.data()),
          n_msg);
  REFUSED(c, ST(c, pts.data(), (int64_t)INT32_MAX + 1, 20, 2.0, 1.0, 2, ws, wsb, keep.data(), avg.data(),
                stats.data(), status.data()), n_msg);
  const char* k_msg = "statistical_outliers: nb_neighbors must be in [1, 64]";
  for (int v : {0, 65, -1, INT32_MAX, INT32_MIN}) REFUSED(c, ST_V(v, 2.0, 1.0, 2), k_msg);
  for (int v : {1, 64}) {
    ACCEPTED(ST_V(v, 2.0, 1.0, 2), "statistical_outliers_run");
    CHECK(g_st.k == v);
  }
  const char* ratio_msg = "statistical_outliers: std_ratio must be finite";
  for (double v : {inf, -inf, nan}) REFUSED(c, ST_V(20, v, 1.0, 2), ratio_msg);
  for (double v : {0.0, -3.0, std::numeric_limits<double>::max()}) ACCEPTED(ST_V(20, v, 1.0, 2), "statistical_outliers_run");
  const char* cell_msg = "statistical_outliers: cell must be finite and > 0";
  for (double v : {0.0, -1.0, inf, -inf, nan}) REFUSED(c, ST_V(20, 2.0, v, 2), cell_msg);
  for (double v : {tiny, std::numeric_limits<double>::max()}) ACCEPTED(ST_V(20, 2.0, v, 2), "statistical_outliers_run");
  const char* ring_msg = "statistical_outliers: max_rings must be in [0, 8]";
  for (int v : {-1, 9, INT32_MAX, INT32_MIN}) REFUSED(c, ST_V(20, 2.0, 1.0, v), ring_msg);
  for (int v : {0, 8}) {
    ACCEPTED(ST_V(20, 2.0, 1.0, v), "statistical_outliers_run");
    CHECK(g_st.rings == v);
  }
  const char* st_ws_msg = "statistical_outliers: workspace too small";
  for (int64_t v : {wsb - 1, (int64_t)0, (int64_t)-1})
    REFUSED(c, ST(c, pts.data(), N, 20, 2.0, 1.0, 2, ws, v, keep.data(), avg.data(), stats.data(), status.data()),
            st_ws_msg);
  {
    std::vector<double> big(wsb / 8 + 1);
    ACCEPTED(ST(c, pts.data(), N, 20, 2.0, 1.0, 2, big.data(), wsb + 8, keep.data(), avg.data(), stats.data(),
                status.data()), "statistical_outliers_run");
    REFUSED(c, ST(c, pts.data(), N, 20, 2.0, 1.0, 2, reinterpret_cast<char*>(big.data()) + 4, wsb, keep.data(),
                  avg.data(), stats.data(), status.data()), "statistical_outliers: workspace must be 8-byte aligned");
  }
  // n_points == 0: the checks still run, nothing is launched, the data pointers may be NULL
  NOTHING(ST(c, nullptr, 0, 20, 2.0, 1.0, 2, nullptr, 0, nullptr, nullptr, stats.data(), nullptr));
  NOTHING(ST(c, pts.data(), 0, 20, 2.0, 1.0, 2, ws, wsb, keep.data(), avg.data(), stats.data(), status.data()));
  REFUSED(c, ST(c, nullptr, 0, 20, 2.0, 1.0, 2, nullptr, 0, nullptr, nullptr, nullptr, nullptr), null_msg);
  REFUSED(c, ST(c, nullptr, 0, 0, 2.0, 1.0, 2, nullptr, 0, nullptr, nullptr, stats.data(), nullptr), k_msg);
  REFUSED(c, ST(c, nullptr, 0, 20, 2.0, 0.0, 2, nullptr, 0, nullptr, nullptr, stats.data(), nullptr), cell_msg);
  {  // a single point
    std::vector<double> p1(3, 0.5), a1(1), w1(fvo_outlier_workspace_bytes(1, 20) / 8);
    std::vector<uint8_t> k1(1);
    ACCEPTED(ST(c, p1.data(), 1, 20, 2.0, 1.0, 2, w1.data(), (int64_t)w1.size() * 8, k1.data(), a1.data(), stats.data(),
                status.data()), "statistical_outliers_run");
  }

  // ---- fvo_radius_outliers
#define RD(ctx, p, n, nb, rad, cell, w, wb, kp, cn, sta) \
  fvo_radius_outliers(ctx, p, n, nb, rad, cell, w, wb, kp, cn, sta, nullptr)
#define RD_V(nb, rad, cell) RD(c, pts.data(), N, nb, rad, cell, ws, wsb, keep.data(), cnt.data(), status.data())
  ACCEPTED(RD_V(5, 1.5, 0.5), "radius_outliers_run");
  CHECK(g_rad.pts == pts.data() && g_rad.ws == ws && g_rad.keep == keep.data() && g_rad.cnt == cnt.data() &&
        g_rad.status == status.data() && g_rad.n == N && g_rad.nb == 5 && g_rad.radius == 1.5 && g_rad.cell == 0.5);
  ACCEPTED(RD(c, pts.data(), N, 5, 1.5, 0.5, ws, wsb, keep.data(), nullptr, nullptr), "radius_outliers_run");
  CHECK(g_rad.cnt == nullptr && g_rad.status == nullptr);
  CHECK(RD(nullptr, pts.data(), N, 5, 1.5, 0.5, ws, wsb, keep.data(), cnt.data(), status.data()) < 0);
  for (int k = 0; k < 3; ++k) {
    auto z = [&](int i, auto* p) { return i == k ? nullptr : p; };
    REFUSED(c, RD(c, z(0, pts.data()), N, 5, 1.5, 0.5, z(1, ws), wsb, z(2, keep.data()), cnt.data(), status.data()),
            null_msg);
  }
  REFUSED(c, RD(c, pts.data(), -1, 5, 1.5, 0.5, ws, wsb, keep.data(), cnt.data(), status.data()), n_msg);
  REFUSED(c, RD(c, pts.data(), (int64_t)INT32_MAX + 1, 5, 1.5, 0.5, ws, wsb, keep.data(), cnt.data(), status.data()),
          n_msg);
  for (int v : {-1, INT32_MIN}) REFUSED(c, RD_V(v, 1.5, 0.5), "radius_outliers: nb_points must be >= 0");
  for (int v : {0, INT32_MAX}) {
    ACCEPTED(RD_V(v, 1.5, 0.5), "radius_outliers_run");
    CHECK(g_rad.nb == v);
  }
  const char* rad_msg = "radius_outliers: radius must be finite and > 0";
  for (double v : {0.0, -1.0, inf, -inf, nan}) REFUSED(c, RD_V(5, v, 0.5), rad_msg);
  const char* rcell_msg = "radius_outliers: cell must be finite and > 0";
  for (double v : {0.0, -1.0, inf, -inf, nan}) REFUSED(c, RD_V(5, 1.5, v), rcell_msg);
  ACCEPTED(RD_V(5, tiny, tiny), "radius_outliers_run");
  ACCEPTED(RD_V(5, 1.0, std::numeric_limits<double>::max()), "radius_outliers_run");
  const char* rc_msg = "radius_outliers: radius / cell must be <= 8";
  REFUSED(c, RD_V(5, std::nextafter(8.0, 9.0), 1.0), rc_msg);
  REFUSED(c, RD_V(5, 1.0, 0.1), rc_msg);
  REFUSED(c, RD_V(5, std::numeric_limits<double>::max(), tiny), rc_msg);  // the quotient overflows
  ACCEPTED(RD_V(5, 8.0, 1.0), "radius_outliers_run");
  ACCEPTED(RD_V(5, 2.0, 0.25), "radius_outliers_run");
  const char* rd_ws_msg = "radius_outliers: workspace too small";
  for (int64_t v : {wsb - 1, (int64_t)0, (int64_t)-1})
    REFUSED(c, RD(c, pts.data(), N, 5, 1.5, 0.5, ws, v, keep.data(), cnt.data(), status.data()), rd_ws_msg);
  REFUSED(c, RD(c, pts.data(), N, 5, 1.5, 0.5, reinterpret_cast<char*>(ws) + 4, wsb - 8, keep.data(), cnt.data(),
                status.data()), rd_ws_msg);
  {
    std::vector<double> big(wsb / 8 + 1);
    REFUSED(c, RD(c, pts.data(), N, 5, 1.5, 0.5, reinterpret_cast<char*>(big.data()) + 4, wsb, keep.data(), cnt.data(),
                  status.data()), "radius_outliers: workspace must be 8-byte aligned");
  }
  NOTHING(RD(c, nullptr, 0, 5, 1.5, 0.5, nullptr, 0, nullptr, nullptr, nullptr));
  NOTHING(RD(c, pts.data(), 0, 5, 1.5, 0.5, ws, wsb, keep.data(), cnt.data(), status.data()));
  REFUSED(c, RD(c, nullptr, 0, -1, 1.5, 0.5, nullptr, 0, nullptr, nullptr, nullptr),
          "radius_outliers: nb_points must be >= 0");
  REFUSED(c, RD(c, nullptr, 0, 5, 1.5, 0.1, nullptr, 0, nullptr, nullptr, nullptr), rc_msg);

  // ---- fvo_select_points
#define SEL(ctx, p, n, kp, o64, o32, no) fvo_select_points(ctx, p, n, kp, o64, o32, no, nullptr)
  ACCEPTED(SEL(c, pts.data(), N, keep.data(), out64.data(), out32.data(), n_out.data()), "select_points_run");
  CHECK(g_sel.pts == pts.data() && g_sel.keep == keep.data() && g_sel.o64 == out64.data() &&
        g_sel.o32 == out32.data() && g_sel.n_out == n_out.data() && g_sel.n == N);
  ACCEPTED(SEL(c, pts.data(), N, keep.data(), out64.data(), nullptr, n_out.data()), "select_points_run");
  CHECK(g_sel.o32 == nullptr);
  ACCEPTED(SEL(c, pts.data(), N, keep.data(), nullptr, out32.data(), n_out.data()), "select_points_run");
  CHECK(g_sel.o64 == nullptr);
  CHECK(SEL(nullptr, pts.data(), N, keep.data(), out64.data(), out32.data(), n_out.data()) < 0);
  for (int k = 0; k < 3; ++k) {
    auto z = [&](int i, auto* p) { return i == k ? nullptr : p; };
    REFUSED(c, SEL(c, z(0, pts.data()), N, z(1, keep.data()), out64.data(), out32.data(), z(2, n_out.data())), null_msg);
  }
  REFUSED(c, SEL(c, pts.data(), N, keep.data(), nullptr, nullptr, n_out.data()),
          "select_points: out64 and out32 are both NULL");
  REFUSED(c, SEL(c, pts.data(), -1, keep.data(), out64.data(), out32.data(), n_out.data()), n_msg);
  REFUSED(c, SEL(c, pts.data(), (int64_t)INT32_MAX + 1, keep.data(), out64.data(), out32.data(), n_out.data()), n_msg);
  {  // out64 / out32 may touch points' ends, not overlap them
    std::vector<double> buf(6 * N, 1.0);
    const char* o64_msg = "select_points: out64 overlaps points";
    REFUSED(c, SEL(c, buf.data(), N, keep.data(), buf.data(), nullptr, n_out.data()), o64_msg);
    REFUSED(c, SEL(c, buf.data(), N, keep.data(), buf.data() + 3 * N - 1, nullptr, n_out.data()), o64_msg);
    REFUSED(c, SEL(c, buf.data() + 3 * N - 1, N, keep.data(), buf.data(), nullptr, n_out.data()), o64_msg);
    ACCEPTED(SEL(c, buf.data(), N, keep.data(), buf.data() + 3 * N, nullptr, n_out.data()), "select_points_run");
    ACCEPTED(SEL(c, buf.data() + 3 * N, N, keep.data(), buf.data(), nullptr, n_out.data()), "select_points_run");
    const char* o32_msg = "select_points: out32 overlaps points";
    float* f = reinterpret_cast<float*>(buf.data());
    REFUSED(c, SEL(c, buf.data(), N, keep.data(), nullptr, f, n_out.data()), o32_msg);
    REFUSED(c, SEL(c, buf.data(), N, keep.data(), nullptr, f + 6 * N - 1, n_out.data()), o32_msg);
    REFUSED(c, SEL(c, buf.data() + 3 * N, N, keep.data(), nullptr, f + 3 * N + 1, n_out.data()), o32_msg);
    ACCEPTED(SEL(c, buf.data(), N, keep.data(), nullptr, f + 6 * N, n_out.data()), "select_points_run");
    ACCEPTED(SEL(c, buf.data() + 3 * N, N, keep.data(), nullptr, f + 3 * N, n_out.data()), "select_points_run");
  }
  NOTHING(SEL(c, nullptr, 0, nullptr, out64.data(), nullptr, n_out.data()));
  REFUSED(c, SEL(c, nullptr, 0, nullptr, nullptr, nullptr, n_out.data()), "select_points: out64 and out32 are both NULL");
  REFUSED(c, SEL(c, nullptr, 0, nullptr, out64.data(), nullptr, nullptr), null_msg);

  // the calls run on any stage: a context with no stage at all
  {
    fvo_config z;
    fvo_config_default(&z, 64, 64);
    z.max_batch = 1;
    z.stages = 0;
    fvo_ctx* e = nullptr;
    if (fvo_create(0, &z, &e) == 0 && e) {
      ACCEPTED(ST(e, pts.data(), N, 20, 2.0, 1.0, 2, ws, wsb, keep.data(), avg.data(), stats.data(), status.data()),
               "statistical_outliers_run");
      fvo_destroy(e);
    }
  }

  // the frozen timing table and the ABI are untouched
  CHECK(fvo_kernel_count() == 36);
  CHECK(fvo_abi_version() == 7);
  CHECK(fvo_config_size() == 31 * 4);

  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
  std::printf("outlier_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
