// The grid neighbour search's device code shared by outlier.hip (statistical and radius outlier
// removal) and normals.hip (normal and covariance estimation): the squared distance both
// specifications state, the gather into cell order, the binary search for a run of cells in the
// sorted keys, and the rounding-safe distance from a query to the faces of the cube of cells it has
// visited.  The rounding argument of face_gap() exists here only.  Included by .hip files only, in the
// anonymous namespace like vx_grid.h.
#pragma once

#include "vx_grid.h"

namespace {

__device__ __forceinline__ double ol_d2(double px, double py, double pz, double qx, double qy, double qz) {
  const double dx = qx - px, dy = qy - py, dz = qz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(256) void k_ol_gather(const double* __restrict__ p, const int32_t* __restrict__ sidx,
                                                   int64_t n, double* __restrict__ sp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t q = sidx[i];
  sp[3 * i] = p[3 * q];
  sp[3 * i + 1] = p[3 * q + 1];
  sp[3 * i + 2] = p[3 * q + 2];
}

// first sorted position whose key is >= k
__device__ __forceinline__ int64_t ol_lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// A lower bound, safe under rounding, of |q_a - p_a| for every point q whose cell index along axis
// a is >= m (side > 0) or < m (side < 0), where p's own index is on the other side of m; +inf when
// the grid has no such cell.  With u = 2^-53: the key is floor(fl(fl(q - o) / cell)), so an index
// >= m gives q - o >= m cell (1 - 2u) and an index < m gives q - o < m cell (1 + 2.01u) exactly.
// The face F = fl(o + fl(m cell)) is within u (|o| + 2.01 m cell) of o + m cell, and B = fl(F - p)
// within u |B| of F - p.  All of it is below 2^-50 S with S = |o| + |p| + m cell, so B - 2^-48 S
// leaves the true gap at least 2^-49 S >= 2^-49 B above the returned g.  Then every such q has a
// computed d2 >= fl(fl(q_a - p_a)^2) >= gap^2 (1 - u)^3 > g^2 (1 + 2^-49) > fl(g * g) (rounding is
// monotonic and the other two squares are >= 0): `kth <= fl(g * g)` proves that no unvisited point
// can replace one of the k held values.  The margin only ever sends a query to a further ring or to
// the exact pass.
__device__ __forceinline__ double face_gap(double o, double cell, double p, int64_t m, int side) {
  if (side > 0 ? m >= kVxCells : m <= 0) return INFINITY;
  const double mc = (double)m * cell;
  const double F = o + mc;
  const double B = side > 0 ? F - p : p - F;
  return B - 0x1p-48 * ((fabs(o) + fabs(p)) + mc);
}

// b_r: the smallest face_gap over the six faces of the cube of cells within Chebyshev distance r
__device__ __forceinline__ double ring_bound(const double* o, double cell, const double* p, const int64_t* c, int r) {
  double b = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    b = fmin(b, face_gap(o[a], cell, p[a], c[a] + r + 1, 1));
    b = fmin(b, face_gap(o[a], cell, p[a], c[a] - r, -1));
  }
  return b;
}

}  // namespace
