// ICP registration for gfx950: Open3D registration_icp with TransformationEstimationPointToPoint /
// PointToPlane and evaluate_registration (fvo_registration_icp), and the rigid transform of a cloud in
// place (fvo_transform_points).  Specification: tests/icp_ref.py (restated from Open3D 0.17, unpinned).
// All arithmetic is fp64, compiled with -ffp-contract=off, one rounding per written operation;
//   s' = T s of the original source, x' = ((r00*x + r01*y) + r02*z) + t0,
//   d2(s', t) = ((dx*dx + dy*dy) + dz*dz),  dx = t.x - s'.x.
// The correspondence of a source point is the target index that minimises (d2, index), kept iff
// d2 < r^2.  The search is nn_grid.h's: exact by face_gap()'s argument, which exists there only.
//
//   target grid  vx_grid.h's keys with side `cell` and the min bound as origin, sorted once per call;
//                k_ol_gather puts the points, and the normals, into that order.
//   k_icp_init   the state of the call in the workspace: T = init, the grid's origin (also the pivot
//                of the sums), done = 0.
//   k_icp_src_keys + sort   the source's order by its cell under init: a wave's queries walk the same
//                cells.  The source moves little afterwards; every pass reuses the order and writes at
//                original indices.
//   k_icp_pass   thread per source point: transform, its cell against the target's origin (int64,
//                clamped so that a far query visits nothing), the cells within R = ceil(r / cell) + 1
//                rings from its own outwards, less the columns and z ends whose face_gap bound is >=
//                r^2 or above the best d2 held; the best (d2, original index).  With s', t and n in
//                registers the 28 terms are formed and summed by a fixed xor-shuffle tree per wave and
//                the waves in order; one row of 29 doubles (28 sums + the count) per block.
//   k_icp_finish one block: the rows summed in block order, fitness and inlier_rmse, the convergence
//                test against the previous pass's values kept in the state, the 6x6 LDL^T + Gibbs
//                rotation or Horn's quaternion by a 4x4 cyclic Jacobi, T <- U T, the done word.  One
//                thread; its small matrices are in LDS (indexed freely, no scratch).
//   k_icp_apply  thread per point of fvo_transform_points.
// The call enqueues max_iteration + 1 passes of two launches; every kernel reads `done` first and
// returns at once when it is set, the last pass never updates: no host round trip, no in-launch
// hand-off between blocks (the launch boundary is the hand-off).  No floating-point atomics, no scratch.
#include <cfloat>

#include "nn_grid.h"

namespace {

constexpr int kIcpThreads = 256;
constexpr int kIcpRow = 29;     // 28 sums + the number of correspondences
constexpr int kIcpSweeps = 12;  // the 4x4 Jacobi's cap (tests/icp_ref.py SWEEP_CAP4)

struct IcpMat {
  double m[16];
};

// the call's state, in the workspace
struct IcpState {
  double T[16];
  double o[3];           // the target grid's origin = the pivot of the sums
  double fitness, rmse;  // of the previous pass
  int32_t done, iterations;
};

struct IcpLayout {
  VxLayout vx;  // the target's grid
  size_t spts, snrm, skeys_a, skeys_b, sidx_a, sidx_b, scub, rows, state, total, ssort_bytes;
};

inline int64_t icp_blocks(int64_t ns) { return (ns + kIcpThreads - 1) / kIcpThreads; }

int icp_layout(int64_t ns, int64_t nt, IcpLayout& L) {
  VxLayout src;
  if (vx_layout(nt, L.vx) || vx_layout(ns, src)) return -1;
  size_t o = L.vx.total;
  auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes); return r; };
  L.spts = take(24 * (size_t)nt);
  L.snrm = take(24 * (size_t)nt);
  L.skeys_a = take(8 * (size_t)ns);
  L.skeys_b = take(8 * (size_t)ns);
  L.sidx_a = take(4 * (size_t)ns);
  L.sidx_b = take(4 * (size_t)ns);
  L.ssort_bytes = src.sort_bytes;
  L.scub = take(src.sort_bytes);
  L.rows = take(8 * (size_t)kIcpRow * (size_t)icp_blocks(ns));
  L.state = take(sizeof(IcpState));
  L.total = o;
  return 0;
}

__global__ void k_icp_init(IcpMat init, const double* __restrict__ part, int nparts, double cell,
                           IcpState* __restrict__ st) {
  const int t = threadIdx.x;
  if (t < 16) st->T[t] = init.m[t];
  if (t < 3) st->o[t] = vx_origin(part, nparts, cell, 0.0, t);
  if (t == 0) {
    st->fitness = 0.0;
    st->rmse = 0.0;
    st->done = 0;
    st->iterations = 0;
  }
}

__device__ __forceinline__ void icp_map(const double* __restrict__ T, double x, double y, double z, double& px,
                                        double& py, double& pz) {
  px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// The cell index of a coordinate against the target's origin, kept in [lo, hi] (as doubles): a query
// at lo or hi is at least R cells outside the grid and visits nothing.  NaN gives lo.
__device__ __forceinline__ int64_t icp_cell(double p, double o, double cell, double lo, double hi) {
  const double f = floor((p - o) / cell);
  return (int64_t)(f > lo ? (f < hi ? f : hi) : lo);
}

// g2 of an axis offset d (cells) for a query whose own index c may lie outside the grid: as
// outlier.hip's ol_axis_g2, with the face moved to the grid's nearest end where the slab is outside it
// (m = 0 below, kVxCells above).  face_gap() wants the query's index on the other side of the face and
// a face inside [0, kVxCells]: c < max(c + d, 0) for d > 0 because the caller skips slabs below 0 unless
// c < 0, and c >= min(c + d + 1, kVxCells) for d < 0 likewise.  A face below 0 would make m * cell
// negative and shrink face_gap's margin, which is sized for m >= 0.
__device__ __forceinline__ double icp_axis_g2(double o, double cell, double p, int64_t c, int d) {
  if (d == 0) return 0.0;
  const double g = d > 0 ? face_gap(o, cell, p, max(c + d, (int64_t)0), 1)
                         : face_gap(o, cell, p, min(c + d + 1, kVxCells), -1);
  return g > 0.0 ? g * g : 0.0;
}

__global__ __launch_bounds__(256) void k_icp_src_keys(const double* __restrict__ src, int64_t ns,
                                                      const IcpState* __restrict__ st, double cell,
                                                      uint64_t* __restrict__ keys, int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  double p[3];
  icp_map(st->T, src[3 * i], src[3 * i + 1], src[3 * i + 2], p[0], p[1], p[2]);
  uint64_t key = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) key = (key << 21) | (uint64_t)icp_cell(p[a], st->o[a], cell, 0.0, (double)(kVxCells - 1));
  keys[i] = key;  // the order only: a cell outside the grid shares the nearest end's
  idx[i] = (int32_t)i;
}

// the 0, -1, +1, -2, +2, ... order of the offsets within R
__device__ __forceinline__ int icp_offset(int i) { return (i & 1) ? -((i + 1) >> 1) : (i >> 1); }

template <int EST>
__global__ __launch_bounds__(kIcpThreads) void k_icp_pass(
    const double* __restrict__ src, const int32_t* __restrict__ sorder, int64_t ns, const double* __restrict__ sp,
    const double* __restrict__ sn, const uint64_t* __restrict__ keys, const int32_t* __restrict__ sidx, int64_t nt,
    double r2, int R, double cell, const IcpState* __restrict__ st, double* __restrict__ rows,
    int32_t* __restrict__ corr, int32_t* __restrict__ status) {
  __shared__ double s_red[kIcpThreads / 64][kIcpRow];
  if (st->done) return;  // uniform over the grid
  const int tid = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * kIcpThreads + tid;
  double v[kIcpRow];
#pragma unroll
  for (int k = 0; k < kIcpRow; ++k) v[k] = 0.0;
  if (s < ns) {
    const int64_t i = sorder[s];
    const double o0 = st->o[0], o1 = st->o[1], o2 = st->o[2];
    double px, py, pz;
    icp_map(st->T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
    double best = INFINITY;
    int32_t bj = INT32_MAX;
    int64_t bpos = -1;
    if (!(fabs(px) < INFINITY && fabs(py) < INFINITY && fabs(pz) < INFINITY)) {
      atomicOr(status, 1);
    } else {
      const double lo = (double)(-(R + 1)), hi = (double)(kVxCells + R);
      const int64_t cx = icp_cell(px, o0, cell, lo, hi), cy = icp_cell(py, o1, cell, lo, hi),
                    cz = icp_cell(pz, o2, cell, lo, hi);
      // every d2 behind a bound g is >= g: out of reach of the radius, or of the best held (a tie
      // at g == best may still win by its index)
      auto out = [&](double g) { return g >= r2 || g > best; };
      for (int ix = 0; ix <= 2 * R; ++ix) {
        const int dx = icp_offset(ix);
        const int64_t x = cx + dx;
        if (x < 0 || x >= kVxCells) continue;
        const double gx = icp_axis_g2(o0, cell, px, cx, dx);
        if (out(gx)) continue;
        for (int iy = 0; iy <= 2 * R; ++iy) {
          const int dy = icp_offset(iy);
          const int64_t y = cy + dy;
          if (y < 0 || y >= kVxCells) continue;
          const double gxy = gx + icp_axis_g2(o1, cell, py, cy, dy);
          if (out(gxy)) continue;
          int z0 = -R, z1 = R;  // drop the ends of the z run that are out of reach
          while (z0 < 0 && out(gxy + icp_axis_g2(o2, cell, pz, cz, z0))) ++z0;
          while (z1 > 0 && out(gxy + icp_axis_g2(o2, cell, pz, cz, z1))) --z1;
          const int64_t za = max(cz + z0, (int64_t)0), zb = min(cz + z1, kVxCells - 1);
          if (za > zb) continue;
          const uint64_t base = ((uint64_t)x << 42) | ((uint64_t)y << 21);
          const uint64_t hik = base | (uint64_t)zb;
          for (int64_t j = ol_lower_bound(keys, nt, base | (uint64_t)za); j < nt && keys[j] <= hik; ++j) {
            const double d = ol_d2(px, py, pz, sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]);
            if (d < r2 && d <= best) {
              const int32_t oj = sidx[j];
              if (d < best || oj < bj) {
                best = d;
                bj = oj;
                bpos = j;
              }
            }
          }
        }
      }
    }
    if (corr) corr[i] = bpos >= 0 ? bj : -1;
    if (bpos >= 0) {
      const double p0 = px - o0, p1 = py - o1, p2 = pz - o2;
      const double q0 = sp[3 * bpos] - o0, q1 = sp[3 * bpos + 1] - o1, q2 = sp[3 * bpos + 2] - o2;
      if (EST == 1) {
        const double n0 = sn[3 * bpos], n1 = sn[3 * bpos + 1], n2 = sn[3 * bpos + 2];
        const double e0 = p0 - q0, e1 = p1 - q1, e2 = p2 - q2;
        const double r = (e0 * n0 + e1 * n1) + e2 * n2;
        const double J[6] = {p1 * n2 - p2 * n1, p2 * n0 - p0 * n2, p0 * n1 - p1 * n0, n0, n1, n2};
        int o = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) v[o++] = J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) v[21 + a] = J[a] * r;
      } else {
        v[0] = p0;
        v[1] = p1;
        v[2] = p2;
        v[3] = q0;
        v[4] = q1;
        v[5] = q2;
        v[6] = p0 * q0;
        v[7] = p0 * q1;
        v[8] = p0 * q2;
        v[9] = p1 * q0;
        v[10] = p1 * q1;
        v[11] = p1 * q2;
        v[12] = p2 * q0;
        v[13] = p2 * q1;
        v[14] = p2 * q2;
      }
      v[27] = best;
      v[28] = 1.0;
    }
  }
  // the block's row: a fixed xor tree per wave, then the waves in order
#pragma unroll
  for (int k = 0; k < kIcpRow; ++k) {
    if (EST == 0 && k >= 15 && k < 27) continue;  // unused by point-to-point: 0
    const double w = wave_sum(v[k]);
    if (wave_lane() == 0) s_red[tid >> 6][k] = w;
  }
  __syncthreads();
  if (tid < kIcpRow) {
    double t = 0.0;
    if (!(EST == 0 && tid >= 15 && tid < 27))
      t = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    rows[(size_t)blockIdx.x * kIcpRow + tid] = t;
  }
}

// ---------------------------------------------------------------- the update (one thread, arrays in LDS)
struct IcpSolve {
  double A[6][6], L[6][6], D[6], y[6], x[6];  // LDL^T; the Jacobi uses A as a[4][4] and L as v[4][4]
  double R[3][3], v[3], M[3][3], pm[3], qm[3];
};

// tests/icp_ref.py ldlt6: A x = rhs, false for a pivot that is not > 0 and finite
__device__ bool icp_ldlt6(IcpSolve& w, const double* rhs) {
  for (int j = 0; j < 6; ++j) {
    double d = w.A[j][j];
    for (int k = 0; k < j; ++k) d = d - (w.L[j][k] * w.L[j][k]) * w.D[k];
    if (!(d > 0.0) || !(d < INFINITY)) return false;
    w.D[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double u = w.A[j][i];
      for (int k = 0; k < j; ++k) u = u - (w.L[i][k] * w.L[j][k]) * w.D[k];
      w.L[i][j] = u / d;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double u = rhs[i];
    for (int k = 0; k < i; ++k) u = u - w.L[i][k] * w.y[k];
    w.y[i] = u;
  }
  for (int i = 5; i >= 0; --i) {
    double u = w.y[i] / w.D[i];
    for (int k = i + 1; k < 6; ++k) u = u - w.L[k][i] * w.x[k];
    w.x[i] = u;
  }
  return true;
}

// tests/icp_ref.py gibbs: R = I + (2 / (1 + g.g)) (G + G G), g = w / 2
__device__ void icp_gibbs(IcpSolve& w) {
  const double g[3] = {0.5 * w.x[0], 0.5 * w.x[1], 0.5 * w.x[2]};
  const double gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
  const double k = 2.0 / (1.0 + gg);
  const double G[3][3] = {{0.0, -g[2], g[1]}, {g[2], 0.0, -g[0]}, {-g[1], g[0], 0.0}};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double GG = g[a] * g[b] - (a == b ? gg : 0.0);
      w.R[a][b] = (a == b ? 1.0 : 0.0) + k * (G[a][b] + GG);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a) w.v[a] = w.x[3 + a];
}

// tests/icp_ref.py horn: the point-to-point sums S of m > 0 correspondences -> w.R, w.v
__device__ void icp_horn(IcpSolve& w, const double* S, double dm) {
  for (int a = 0; a < 3; ++a) {
    w.pm[a] = S[a] / dm;
    w.qm[a] = S[3 + a] / dm;
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) w.M[a][b] = S[6 + 3 * a + b] / dm - w.pm[a] * w.qm[b];
  double(*a)[6] = w.A;  // a[4][4] in the corner of A, v[4][4] in the corner of L
  double(*v)[6] = w.L;
  a[0][0] = (w.M[0][0] + w.M[1][1]) + w.M[2][2];
  a[1][1] = (w.M[0][0] - w.M[1][1]) - w.M[2][2];
  a[2][2] = (w.M[1][1] - w.M[0][0]) - w.M[2][2];
  a[3][3] = (w.M[2][2] - w.M[0][0]) - w.M[1][1];
  a[0][1] = a[1][0] = w.M[1][2] - w.M[2][1];
  a[0][2] = a[2][0] = w.M[2][0] - w.M[0][2];
  a[0][3] = a[3][0] = w.M[0][1] - w.M[1][0];
  a[1][2] = a[2][1] = w.M[0][1] + w.M[1][0];
  a[1][3] = a[3][1] = w.M[2][0] + w.M[0][2];
  a[2][3] = a[3][2] = w.M[1][2] + w.M[2][1];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kIcpSweeps; ++sweep) {
    if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[0][3] == 0.0 && a[1][2] == 0.0 && a[1][3] == 0.0 && a[2][3] == 0.0) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double th = (a[q][q] - a[p][p]) / (2.0 * apq);
        double t = 1.0 / (fabs(th) + sqrt(th * th + 1.0));
        if (th < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        a[p][p] = a[p][p] - t * apq;
        a[q][q] = a[q][q] + t * apq;
        a[p][q] = a[q][p] = 0.0;
        for (int r = 0; r < 4; ++r) {
          if (r == p || r == q) continue;
          const double arp = a[r][p], arq = a[r][q];
          a[r][p] = a[p][r] = c * arp - s * arq;
          a[r][q] = a[q][r] = s * arp + c * arq;
        }
        for (int k = 0; k < 4; ++k) {
          const double vp = v[k][p], vq = v[k][q];
          v[k][p] = c * vp - s * vq;
          v[k][q] = s * vp + c * vq;
        }
      }
  }
  int e = 0;  // the largest diagonal entry, ties to the lowest index
  for (int k = 1; k < 4; ++k)
    if (a[k][k] > a[e][e]) e = k;
  double qw = v[0][e], qx = v[1][e], qy = v[2][e], qz = v[3][e];
  const double len = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  qw = qw / len;
  qx = qx / len;
  qy = qy / len;
  qz = qz / len;
  w.R[0][0] = ((qw * qw + qx * qx) - qy * qy) - qz * qz;
  w.R[0][1] = 2.0 * (qx * qy - qw * qz);
  w.R[0][2] = 2.0 * (qx * qz + qw * qy);
  w.R[1][0] = 2.0 * (qx * qy + qw * qz);
  w.R[1][1] = ((qw * qw - qx * qx) + qy * qy) - qz * qz;
  w.R[1][2] = 2.0 * (qy * qz - qw * qx);
  w.R[2][0] = 2.0 * (qx * qz - qw * qy);
  w.R[2][1] = 2.0 * (qy * qz + qw * qx);
  w.R[2][2] = ((qw * qw - qx * qx) - qy * qy) + qz * qz;
  for (int k = 0; k < 3; ++k)
    w.v[k] = w.qm[k] - ((w.R[k][0] * w.pm[0] + w.R[k][1] * w.pm[1]) + w.R[k][2] * w.pm[2]);
}

template <int EST>
__global__ __launch_bounds__(64) void k_icp_finish(IcpState* __restrict__ st, const double* __restrict__ rows,
                                                   int64_t nblocks, int64_t ns, double rel_fitness, double rel_rmse,
                                                   int pass, int last, double* __restrict__ result,
                                                   double* __restrict__ sums, int32_t* __restrict__ status) {
  __shared__ double S[kIcpRow];
  __shared__ double s_T[16];
  __shared__ IcpSolve w;
  if (st->done) return;
  const int tid = threadIdx.x;
  if (tid < kIcpRow) {  // the rows in block order
    double acc = 0.0;
    for (int64_t b = 0; b < nblocks; ++b) acc = acc + rows[(size_t)b * kIcpRow + tid];
    S[tid] = acc;
  }
  __syncthreads();
  if (tid != 0) return;
  const double dm = S[28];
  const double fitness = dm / (double)ns;
  const double rmse = dm > 0.0 ? sqrt(S[27] / dm) : 0.0;
  if (sums) {  // this pass's sums and the T that entered it
    for (int k = 0; k < kIcpRow; ++k) sums[k] = S[k];
    for (int k = 0; k < 16; ++k) sums[kIcpRow + k] = st->T[k];
  }
  const bool converged = pass > 0 && fabs(fitness - st->fitness) < rel_fitness && fabs(rmse - st->rmse) < rel_rmse;
  if (last || converged) {
    for (int k = 0; k < 16; ++k) result[k] = st->T[k];
    result[16] = fitness;
    result[17] = rmse;
    result[18] = dm;
    result[19] = (double)st->iterations;
    st->done = 1;
    return;
  }
  st->fitness = fitness;
  st->rmse = rmse;
  st->iterations = st->iterations + 1;
  bool ok = dm > 0.0;
  if (ok) {
    if (EST == 1) {
      int o = 0;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) w.A[a][b] = S[o++];
      double rhs[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) rhs[a] = -S[21 + a];
      ok = icp_ldlt6(w, rhs);
      if (ok) icp_gibbs(w);
    } else {
      icp_horn(w, S, dm);
    }
  }
  if (!ok) {  // the identity update
    atomicOr(status, 2);
    return;
  }
  // U = [R | (v + c) - R c], T <- U T
  const double c0 = st->o[0], c1 = st->o[1], c2 = st->o[2];
  for (int k = 0; k < 16; ++k) s_T[k] = st->T[k];
  for (int a = 0; a < 3; ++a) {
    const double u3 = (w.v[a] + st->o[a]) - ((w.R[a][0] * c0 + w.R[a][1] * c1) + w.R[a][2] * c2);
    for (int b = 0; b < 4; ++b) {
      const double t = (w.R[a][0] * s_T[b] + w.R[a][1] * s_T[4 + b]) + w.R[a][2] * s_T[8 + b];
      st->T[4 * a + b] = b == 3 ? t + u3 : t;
    }
  }
  st->T[12] = 0.0;
  st->T[13] = 0.0;
  st->T[14] = 0.0;
  st->T[15] = 1.0;
}

// n_source == 0 or n_target == 0: the init transform, fitness 0, no correspondences
__global__ void k_icp_trivial(IcpMat init, double* __restrict__ result, double* __restrict__ sums) {
  const int t = threadIdx.x;
  if (t < 16) result[t] = init.m[t];
  if (t >= 16 && t < 20) result[t] = 0.0;
  if (sums) {
    if (t < kIcpRow) sums[t] = 0.0;
    if (t < 16) sums[kIcpRow + t] = init.m[t];
  }
}

__global__ __launch_bounds__(256) void k_icp_apply(double* __restrict__ p, float* __restrict__ p32,
                                                   double* __restrict__ nrm, int64_t n, IcpMat T) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  icp_map(T.m, p[3 * i], p[3 * i + 1], p[3 * i + 2], x, y, z);
  p[3 * i] = x;
  p[3 * i + 1] = y;
  p[3 * i + 2] = z;
  if (p32) {
    p32[3 * i] = (float)x;
    p32[3 * i + 1] = (float)y;
    p32[3 * i + 2] = (float)z;
  }
  if (nrm) {
    const double a = nrm[3 * i], b = nrm[3 * i + 1], c = nrm[3 * i + 2];
    nrm[3 * i] = (T.m[0] * a + T.m[1] * b) + T.m[2] * c;
    nrm[3 * i + 1] = (T.m[4] * a + T.m[5] * b) + T.m[6] * c;
    nrm[3 * i + 2] = (T.m[8] * a + T.m[9] * b) + T.m[10] * c;
  }
}

IcpMat icp_mat(const double* T) {
  IcpMat m;
  for (int k = 0; k < 16; ++k) m.m[k] = T[k];
  return m;
}

}  // namespace

int64_t icp_workspace_bytes(int64_t n_source, int64_t n_target) {
  IcpLayout L;
  if (n_source < 1 || n_target < 1 || icp_layout(n_source, n_target, L)) return -1;
  return (int64_t)L.total;
}

int registration_icp_run(fvo_ctx* ctx, const double* source, int64_t ns, const double* target,
                         const double* target_normals, int64_t nt, double radius, double cell, const double* init,
                         int estimation, double rel_fitness, double rel_rmse, int max_iteration, void* ws,
                         double* result, double* sums, int32_t* correspondences, int32_t* status, hipStream_t s) {
  // arguments were validated by capi_icp.cpp (radius / cell <= 8, so R <= 9; the workspace size against
  // icp_workspace_bytes); init is read here, on the host, before the first launch
  IcpLayout L;
  if (icp_layout(ns, nt, L)) return fvo_fail(ctx, "registration_icp: workspace size query failed");  // a hipcub error
  char* w = (char*)ws;
  int32_t* st = status ? status : (int32_t*)(w + L.vx.status);
  IcpState* state = (IcpState*)(w + L.state);
  const double* sp = (const double*)(w + L.spts);
  const double* sn = (const double*)(w + L.snrm);
  const uint64_t* keys = (const uint64_t*)(w + L.vx.keys_b);
  const int32_t* sidx = (const int32_t*)(w + L.vx.idx_b);
  double* rows = (double*)(w + L.rows);
  FVO_HIP(ctx, hipMemsetAsync(st, 0, 4, s));
  vx_sort_keys(target, nt, cell, 0.0, w, L.vx, st, s);
  FVO_LAUNCH_CHECK(ctx);
  const unsigned gt = (unsigned)((nt + 255) / 256), gs = (unsigned)((ns + 255) / 256);
  hipLaunchKernelGGL(k_ol_gather, dim3(gt), dim3(256), 0, s, target, sidx, nt, (double*)(w + L.spts));
  if (estimation == 1)
    hipLaunchKernelGGL(k_ol_gather, dim3(gt), dim3(256), 0, s, target_normals, sidx, nt, (double*)(w + L.snrm));
  hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, icp_mat(init), (const double*)(w + L.vx.part), vx_parts(nt),
                     cell, state);
  FVO_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_icp_src_keys, dim3(gs), dim3(256), 0, s, source, ns, state, cell, (uint64_t*)(w + L.skeys_a),
                     (int32_t*)(w + L.sidx_a));
  size_t sb = L.ssort_bytes;
  (void)hipcub::DeviceRadixSort::SortPairs(w + L.scub, sb, (const uint64_t*)(w + L.skeys_a), (uint64_t*)(w + L.skeys_b),
                                           (const int32_t*)(w + L.sidx_a), (int32_t*)(w + L.sidx_b), (int)ns, 0, 63, s);
  FVO_LAUNCH_CHECK(ctx);
  const int32_t* sorder = (const int32_t*)(w + L.sidx_b);
  const double r2 = radius * radius;
  const int R = (int)ceil(radius / cell) + 1;
  const int64_t nb = icp_blocks(ns);
  for (int pass = 0; pass <= max_iteration; ++pass) {
    const int last = pass == max_iteration;
    if (estimation == 1) {
      hipLaunchKernelGGL(k_icp_pass<1>, dim3((unsigned)nb), dim3(kIcpThreads), 0, s, source, sorder, ns, sp, sn, keys,
                         sidx, nt, r2, R, cell, state, rows, correspondences, st);
      hipLaunchKernelGGL(k_icp_finish<1>, dim3(1), dim3(64), 0, s, state, rows, nb, ns, rel_fitness, rel_rmse, pass,
                         last, result, sums, st);
    } else {
      hipLaunchKernelGGL(k_icp_pass<0>, dim3((unsigned)nb), dim3(kIcpThreads), 0, s, source, sorder, ns, sp, sn, keys,
                         sidx, nt, r2, R, cell, state, rows, correspondences, st);
      hipLaunchKernelGGL(k_icp_finish<0>, dim3(1), dim3(64), 0, s, state, rows, nb, ns, rel_fitness, rel_rmse, pass,
                         last, result, sums, st);
    }
    FVO_LAUNCH_CHECK(ctx);
  }
  return 0;
}

int icp_trivial_run(fvo_ctx* ctx, const double* init, int64_t ns, double* result, double* sums,
                    int32_t* correspondences, int32_t* status, hipStream_t s) {
  if (status) FVO_HIP(ctx, hipMemsetAsync(status, 0, 4, s));
  if (correspondences && ns > 0) FVO_HIP(ctx, hipMemsetAsync(correspondences, 0xFF, 4 * (size_t)ns, s));  // -1
  hipLaunchKernelGGL(k_icp_trivial, dim3(1), dim3(64), 0, s, icp_mat(init), result, sums);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int transform_points_run(fvo_ctx* ctx, double* points, float* points32, double* normals, int64_t n, const double* T,
                         hipStream_t s) {
  // arguments were validated by capi_icp.cpp; T is read here, on the host, before the launch
  hipLaunchKernelGGL(k_icp_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points, points32, normals, n,
                     icp_mat(T));
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
