// Argument validation of the registration C ABI (csrc/capi_icp.cpp: fvo_icp_workspace_bytes,
// fvo_registration_icp, fvo_transform_points) exercised on the host under AddressSanitizer +
// UndefinedBehaviorSanitizer.  Linked with csrc/capi.cpp, csrc/capi_icp.cpp and host_stubs.cpp; the
// stubs of the launchers are here: each records what the entry point passed on and touches the first
// and last element of every buffer as the entry point sized it.  Built and run by
// tests/test_icp_cpu.py.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host_stubs.h"

static int g_fail = 0, g_checks = 0;

struct IcpArgs {
  const void *src, *tgt, *nrm, *ws, *result, *sums, *corr, *status;
  int64_t ns, nt;
  int est, max_it;
  double r, cell, rel_fit, rel_rmse, init[16];
};
static IcpArgs g_icp;
struct TrivialArgs {
  const void *result, *sums, *corr, *status;
  int64_t ns;
  double init[16];
};
static TrivialArgs g_triv;
struct XfArgs {
  const void *pts, *p32, *nrm;
  int64_t n;
  double T[16];
};
static XfArgs g_xf;

static int hit(const char* name) {
  g_last_launch = name;
  ++g_launches;
  return 0;
}

int64_t icp_workspace_bytes(int64_t ns, int64_t nt) { return ns < 1 || nt < 1 ? -1 : 32 * ns + 64 * nt + 8192; }

int registration_icp_run(fvo_ctx*, const double* src, int64_t ns, const double* tgt, const double* nrm, int64_t nt,
                         double r, double cell, const double* init, int est, double rel_fit, double rel_rmse,
                         int max_it, void* ws, double* result, double* sums, int32_t* corr, int32_t* status,
                         hipStream_t) {
  g_icp = IcpArgs{src, tgt, nrm, ws, result, sums, corr, status, ns, nt, est, max_it, r, cell, rel_fit, rel_rmse, {}};
  std::memcpy(g_icp.init, init, sizeof g_icp.init);
  char* w = static_cast<char*>(ws);
  w[0] = w[icp_workspace_bytes(ns, nt) - 1] = 1;
  result[0] = result[19] = src[0] + src[3 * ns - 1] + tgt[0] + tgt[3 * nt - 1] + (nrm ? nrm[0] + nrm[3 * nt - 1] : 0.0);
  if (sums) sums[0] = sums[FVO_ICP_SUMS - 1] = 0.0;
  if (corr) corr[0] = corr[ns - 1] = -1;
  if (status) status[0] = 0;
  return hit("registration_icp_run");
}
int icp_trivial_run(fvo_ctx*, const double* init, int64_t ns, double* result, double* sums, int32_t* corr,
                    int32_t* status, hipStream_t) {
  g_triv = TrivialArgs{result, sums, corr, status, ns, {}};
  std::memcpy(g_triv.init, init, sizeof g_triv.init);
  result[0] = result[19] = 0.0;
  if (sums) sums[0] = sums[FVO_ICP_SUMS - 1] = 0.0;
  if (corr && ns > 0) corr[0] = corr[ns - 1] = -1;
  if (status) status[0] = 0;
  return hit("icp_trivial_run");
}
int transform_points_run(fvo_ctx*, double* pts, float* p32, double* nrm, int64_t n, const double* T, hipStream_t) {
  g_xf = XfArgs{pts, p32, nrm, n, {}};
  std::memcpy(g_xf.T, T, sizeof g_xf.T);
  pts[0] = pts[3 * n - 1] = T[0] + T[15];
  if (p32) p32[0] = p32[3 * n - 1] = 0.f;
  if (nrm) nrm[0] = nrm[3 * n - 1] = 0.0;
  return hit("transform_points_run");
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

// rc must be 0 with nothing launched at all
#define NOTHING(call)                                  \
  do {                                                 \
    g_launches = 0;                                    \
    CHECK((call) == 0);                                \
    CHECK(g_launches == 0);                            \
  } while (0)

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const double tiny = std::numeric_limits<double>::denorm_min(), big = std::numeric_limits<double>::max();
  const int64_t NS = 37, NT = 53;
  fvo_config cfg;
  fvo_config_default(&cfg, 64, 64);
  cfg.max_batch = 1;
  cfg.stages = FVO_STAGE_BF;
  cfg.kp_capacity = 64;
  fvo_ctx* c = nullptr;
  CHECK(fvo_create(0, &cfg, &c) == 0 && c != nullptr);
  if (!c) return 1;

  // every buffer of exactly the size the call needs (heap: ASan sees one byte too many)
  std::vector<double> src(3 * NS, 1.0), tgt(3 * NT, 2.0), nrm(3 * NT, 0.5), res(20), sums(FVO_ICP_SUMS);
  std::vector<int32_t> corr(NS), status(1);
  std::vector<float> p32(3 * NS);
  std::vector<double> eye{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const int64_t wsb = fvo_icp_workspace_bytes(NS, NT);
  CHECK(wsb == 32 * NS + 64 * NT + 8192);
  std::vector<double> ws_(wsb / 8);
  void* ws = ws_.data();

  // ---- fvo_icp_workspace_bytes
  CHECK(fvo_icp_workspace_bytes(-1, NT) == -1 && fvo_icp_workspace_bytes(NS, -1) == -1);
  CHECK(fvo_icp_workspace_bytes((int64_t)INT32_MAX + 1, NT) == -1 && fvo_icp_workspace_bytes(NS, (int64_t)INT32_MAX + 1) == -1);
  CHECK(fvo_icp_workspace_bytes(0, NT) == 0 && fvo_icp_workspace_bytes(NS, 0) == 0 && fvo_icp_workspace_bytes(0, 0) == 0);
  CHECK(fvo_icp_workspace_bytes(INT32_MAX, INT32_MAX) == 96 * (int64_t)INT32_MAX + 8192);
  CHECK(fvo_icp_workspace_bytes(1, 1) == 32 + 64 + 8192);

  // ---- fvo_registration_icp
#define ICP(ctx, s, ns, t, n, nt, r, cell, init, est, rf, rr, it, w, wb, rs, sm, co, st) \
  fvo_registration_icp(ctx, s, ns, t, n, nt, r, cell, init, est, rf, rr, it, w, wb, rs, sm, co, st, nullptr)
#define ICP_V(r, cell, init, est, rf, rr, it)                                                                     \
  ICP(c, src.data(), NS, tgt.data(), nrm.data(), NT, r, cell, init, est, rf, rr, it, ws, wsb, res.data(), sums.data(), \
      corr.data(), status.data())
  const char* run = "registration_icp_run";
  const char* triv = "icp_trivial_run";
  std::vector<double> init{0.5, 0, 0, 1, 0, 0.5, 0, 2, 0, 0, 0.5, 3, 0, 0, 0, 1};
  ACCEPTED(ICP_V(0.3, 0.25, init.data(), 1, 1e-6, 1e-7, 30), run);
  CHECK(g_icp.src == src.data() && g_icp.tgt == tgt.data() && g_icp.nrm == nrm.data() && g_icp.ws == ws &&
        g_icp.result == res.data() && g_icp.sums == sums.data() && g_icp.corr == corr.data() &&
        g_icp.status == status.data() && g_icp.ns == NS && g_icp.nt == NT && g_icp.est == 1 && g_icp.max_it == 30 &&
        g_icp.r == 0.3 && g_icp.cell == 0.25 && g_icp.rel_fit == 1e-6 && g_icp.rel_rmse == 1e-7 &&
        !std::memcmp(g_icp.init, init.data(), sizeof g_icp.init));
  // target_normals (point-to-point), sums, correspondences and status are optional
  ACCEPTED(ICP(c, src.data(), NS, tgt.data(), nullptr, NT, 0.3, 0.3, eye.data(), 0, 0.0, 0.0, 0, ws, wsb, res.data(),
               nullptr, nullptr, nullptr), run);
  CHECK(g_icp.nrm == nullptr && g_icp.sums == nullptr && g_icp.corr == nullptr && g_icp.status == nullptr &&
        g_icp.est == 0 && g_icp.max_it == 0);
  CHECK(ICP(nullptr, src.data(), NS, tgt.data(), nrm.data(), NT, 0.3, 0.3, eye.data(), 0, 0.0, 0.0, 0, ws, wsb,
            res.data(), nullptr, nullptr, nullptr) < 0);
  const char* null_msg = "null pointer argument";
  for (int k = 0; k < 5; ++k) {
    auto z = [&](int i, auto* p) { return i == k ? nullptr : p; };
    REFUSED(c, ICP(c, z(0, src.data()), NS, z(1, tgt.data()), nrm.data(), NT, 0.3, 0.3, z(2, eye.data()), 1, 1e-6, 1e-6,
                   30, z(3, ws), wsb, z(4, res.data()), sums.data(), corr.data(), status.data()), null_msg);
  }
  for (int64_t v : {(int64_t)-1, (int64_t)INT32_MAX + 1}) {
    REFUSED(c, ICP(c, src.data(), v, tgt.data(), nrm.data(), NT, 0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, 30, ws, wsb,
                   res.data(), sums.data(), corr.data(), status.data()), "n_source out of range");
    REFUSED(c, ICP(c, src.data(), NS, tgt.data(), nrm.data(), v, 0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, 30, ws, wsb,
                   res.data(), sums.data(), corr.data(), status.data()), "n_target out of range");
  }
  for (int v : {-1, 2, INT32_MAX, INT32_MIN})
    REFUSED(c, ICP_V(0.3, 0.3, eye.data(), v, 1e-6, 1e-6, 30), "registration_icp: estimation must be 0 or 1");
  const char* r_msg = "registration_icp: max_correspondence_distance must be finite and > 0";
  for (double v : {0.0, -0.0, -1.0, inf, -inf, nan}) REFUSED(c, ICP_V(v, 0.3, eye.data(), 1, 1e-6, 1e-6, 30), r_msg);
  for (double v : {tiny, big}) {
    ACCEPTED(ICP_V(v, v, eye.data(), 1, 1e-6, 1e-6, 30), run);
    CHECK(g_icp.r == v && g_icp.cell == v);
  }
  const char* cell_msg = "registration_icp: cell must be finite and > 0";
  for (double v : {0.0, -1.0, inf, -inf, nan}) REFUSED(c, ICP_V(0.3, v, eye.data(), 1, 1e-6, 1e-6, 30), cell_msg);
  const char* ratio_msg = "registration_icp: max_correspondence_distance / cell must be <= 8";
  REFUSED(c, ICP_V(8.5, 1.0, eye.data(), 1, 1e-6, 1e-6, 30), ratio_msg);
  REFUSED(c, ICP_V(big, 1.0, eye.data(), 1, 1e-6, 1e-6, 30), ratio_msg);
  REFUSED(c, ICP_V(1.0, tiny, eye.data(), 1, 1e-6, 1e-6, 30), ratio_msg);  // the quotient overflows
  ACCEPTED(ICP_V(8.0, 1.0, eye.data(), 1, 1e-6, 1e-6, 30), run);
  ACCEPTED(ICP_V(1.0, big, eye.data(), 1, 1e-6, 1e-6, 30), run);
  for (int a = 0; a < 16; ++a)
    for (double v : {inf, -inf, nan}) {
      std::vector<double> t = eye;
      t[a] = v;
      REFUSED(c, ICP_V(0.3, 0.3, t.data(), 1, 1e-6, 1e-6, 30), "registration_icp: init must be finite");
    }
  const char* row_msg = "registration_icp: the bottom row of init must be (0, 0, 0, 1)";
  for (int a = 12; a < 16; ++a) {
    std::vector<double> t = eye;
    t[a] = a == 15 ? 1.0 + 0x1p-52 : tiny;
    REFUSED(c, ICP_V(0.3, 0.3, t.data(), 1, 1e-6, 1e-6, 30), row_msg);
  }
  {
    std::vector<double> t = eye;  // -0.0 is 0; the upper rows are not checked (any finite affine part)
    t[12] = -0.0;
    t[0] = big;
    t[7] = -big;
    ACCEPTED(ICP_V(0.3, 0.3, t.data(), 1, 1e-6, 1e-6, 30), run);
  }
  const char* nrm_msg = "registration_icp: point-to-plane needs target_normals";
  REFUSED(c, ICP(c, src.data(), NS, tgt.data(), nullptr, NT, 0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, 30, ws, wsb, res.data(),
                 sums.data(), corr.data(), status.data()), nrm_msg);
  const char* crit_msg = "registration_icp: relative_fitness and relative_rmse must be >= 0";
  for (double v : {-tiny, -1.0, -inf, nan}) {
    REFUSED(c, ICP_V(0.3, 0.3, eye.data(), 1, v, 1e-6, 30), crit_msg);
    REFUSED(c, ICP_V(0.3, 0.3, eye.data(), 1, 1e-6, v, 30), crit_msg);
  }
  for (double v : {0.0, -0.0, tiny, big, inf}) ACCEPTED(ICP_V(0.3, 0.3, eye.data(), 1, v, v, 30), run);
  const char* it_msg = "registration_icp: max_iteration must be in [0, 1000]";
  for (int v : {-1, 1001, INT32_MAX, INT32_MIN}) REFUSED(c, ICP_V(0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, v), it_msg);
  for (int v : {0, 1000}) {
    ACCEPTED(ICP_V(0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, v), run);
    CHECK(g_icp.max_it == v);
  }
  const char* ws_msg = "registration_icp: workspace too small";
  for (int64_t v : {wsb - 1, (int64_t)0, (int64_t)-1})
    REFUSED(c, ICP(c, src.data(), NS, tgt.data(), nrm.data(), NT, 0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, 30, ws, v,
                   res.data(), sums.data(), corr.data(), status.data()), ws_msg);
  {
    std::vector<double> more(wsb / 8 + 1);
    ACCEPTED(ICP(c, src.data(), NS, tgt.data(), nrm.data(), NT, 0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, 30, more.data(),
                 wsb + 8, res.data(), sums.data(), corr.data(), status.data()), run);
    REFUSED(c, ICP(c, src.data(), NS, tgt.data(), nrm.data(), NT, 0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, 30,
                   reinterpret_cast<char*>(more.data()) + 4, wsb, res.data(), sums.data(), corr.data(), status.data()),
            "registration_icp: workspace must be 8-byte aligned");
  }
  // n_source == 0 or n_target == 0: the checks still run, the search is never launched (only the
  // launcher that writes init and the zeros), the data pointers and the workspace may be NULL
  ACCEPTED(ICP(c, nullptr, 0, tgt.data(), nrm.data(), NT, 0.3, 0.3, init.data(), 1, 1e-6, 1e-6, 30, nullptr, 0,
               res.data(), sums.data(), nullptr, status.data()), triv);
  CHECK(g_triv.ns == 0 && g_triv.result == res.data() && g_triv.sums == sums.data() && g_triv.corr == nullptr &&
        !std::memcmp(g_triv.init, init.data(), sizeof g_triv.init));
  ACCEPTED(ICP(c, src.data(), NS, nullptr, nullptr, 0, 0.3, 0.3, init.data(), 1, 1e-6, 1e-6, 30, nullptr, 0, res.data(),
               nullptr, corr.data(), nullptr), triv);
  CHECK(g_triv.ns == NS && g_triv.corr == corr.data() && g_triv.sums == nullptr && g_triv.status == nullptr);
  ACCEPTED(ICP(c, nullptr, 0, nullptr, nullptr, 0, 0.3, 0.3, eye.data(), 0, 0.0, 0.0, 0, nullptr, 0, res.data(), nullptr,
               nullptr, nullptr), triv);
  REFUSED(c, ICP(c, nullptr, 0, nullptr, nullptr, 0, 0.3, 0.3, eye.data(), 0, 0.0, 0.0, 0, nullptr, 0, nullptr, nullptr,
                 nullptr, nullptr), null_msg);
  REFUSED(c, ICP(c, nullptr, 0, nullptr, nullptr, 0, nan, 0.3, eye.data(), 0, 0.0, 0.0, 0, nullptr, 0, res.data(),
                 nullptr, nullptr, nullptr), r_msg);
  REFUSED(c, ICP(c, nullptr, 0, nullptr, nullptr, 0, 0.3, 0.0, eye.data(), 0, 0.0, 0.0, 0, nullptr, 0, res.data(),
                 nullptr, nullptr, nullptr), cell_msg);
  REFUSED(c, ICP(c, nullptr, 0, nullptr, nullptr, 0, 0.3, 0.3, eye.data(), 2, 0.0, 0.0, 0, nullptr, 0, res.data(),
                 nullptr, nullptr, nullptr), "registration_icp: estimation must be 0 or 1");
  REFUSED(c, ICP(c, nullptr, 0, nullptr, nullptr, 0, 0.3, 0.3, eye.data(), 0, 0.0, 0.0, 1001, nullptr, 0, res.data(),
                 nullptr, nullptr, nullptr), it_msg);
  {  // a single point on either side
    std::vector<double> s1(3, 0.5), t1(3, 0.25), n1(3, 1.0), w1(fvo_icp_workspace_bytes(1, 1) / 8);
    std::vector<int32_t> c1(1);
    ACCEPTED(ICP(c, s1.data(), 1, t1.data(), n1.data(), 1, 0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, 30, w1.data(),
                 (int64_t)w1.size() * 8, res.data(), sums.data(), c1.data(), status.data()), run);
  }

  // ---- fvo_transform_points
#define XF(ctx, p, q, nr, n, T) fvo_transform_points(ctx, p, q, nr, n, T, nullptr)
  const char* xrun = "transform_points_run";
  std::vector<double> nn(3 * NS, 0.0);
  ACCEPTED(XF(c, src.data(), p32.data(), nn.data(), NS, init.data()), xrun);
  CHECK(g_xf.pts == src.data() && g_xf.p32 == p32.data() && g_xf.nrm == nn.data() && g_xf.n == NS &&
        !std::memcmp(g_xf.T, init.data(), sizeof g_xf.T));
  ACCEPTED(XF(c, src.data(), nullptr, nullptr, NS, eye.data()), xrun);  // points32 and normals are optional
  CHECK(g_xf.p32 == nullptr && g_xf.nrm == nullptr);
  CHECK(XF(nullptr, src.data(), nullptr, nullptr, NS, eye.data()) < 0);
  REFUSED(c, XF(c, nullptr, p32.data(), nn.data(), NS, eye.data()), null_msg);
  REFUSED(c, XF(c, src.data(), p32.data(), nn.data(), NS, nullptr), null_msg);
  REFUSED(c, XF(c, src.data(), p32.data(), nn.data(), -1, eye.data()), "n_points out of range");
  REFUSED(c, XF(c, src.data(), p32.data(), nn.data(), (int64_t)INT32_MAX + 1, eye.data()), "n_points out of range");
  for (int a = 0; a < 16; ++a)
    for (double v : {inf, -inf, nan}) {
      std::vector<double> t = eye;
      t[a] = v;
      REFUSED(c, XF(c, src.data(), p32.data(), nn.data(), NS, t.data()), "transform_points: T must be finite");
    }
  for (int a = 12; a < 16; ++a) {
    std::vector<double> t = eye;
    t[a] = a == 15 ? 1.0 - 0x1p-53 : -tiny;
    REFUSED(c, XF(c, src.data(), p32.data(), nn.data(), NS, t.data()),
            "transform_points: the bottom row of T must be (0, 0, 0, 1)");
  }
  NOTHING(XF(c, nullptr, nullptr, nullptr, 0, eye.data()));  // n_points == 0 launches nothing at all
  NOTHING(XF(c, src.data(), p32.data(), nn.data(), 0, init.data()));
  REFUSED(c, XF(c, nullptr, nullptr, nullptr, 0, nullptr), null_msg);
  {
    std::vector<double> t = eye;
    t[14] = 1.0;
    REFUSED(c, XF(c, nullptr, nullptr, nullptr, 0, t.data()), "transform_points: the bottom row of T must be (0, 0, 0, 1)");
  }
  {  // a single point
    std::vector<double> p1(3, 0.5);
    ACCEPTED(XF(c, p1.data(), nullptr, nullptr, 1, eye.data()), xrun);
  }

  // the calls run on any stage: a context with no stage at all
  {
    fvo_config z;
    fvo_config_default(&z, 64, 64);
    z.max_batch = 1;
    z.stages = 0;
    fvo_ctx* e = nullptr;
    if (fvo_create(0, &z, &e) == 0 && e) {
      ACCEPTED(ICP(e, src.data(), NS, tgt.data(), nrm.data(), NT, 0.3, 0.3, eye.data(), 1, 1e-6, 1e-6, 30, ws, wsb,
                   res.data(), sums.data(), corr.data(), status.data()), run);
      ACCEPTED(XF(e, src.data(), nullptr, nullptr, NS, eye.data()), xrun);
      fvo_destroy(e);
    }
  }

  // the frozen timing table and the ABI are untouched
  CHECK(fvo_kernel_count() == 36);
  CHECK(fvo_abi_version() == 7);
  CHECK(fvo_config_size() == 31 * 4);

  fvo_destroy(c);
  CHECK(g_live_allocs == 0);
  std::printf("icp_check: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
