// Point-cloud normal and covariance estimation for gfx950: Open3D PointCloud::EstimateNormals /
// EstimateCovariances with a k-NN or hybrid (radius, max_nn) search (fvo_estimate_normals) and
// OrientNormalsTowardsCameraLocation / OrientNormalsToAlignWithDirection (fvo_orient_normals).
// Specification: tests/normals_ref.py (restated from Open3D 0.17, unpinned).  All arithmetic is fp64,
// compiled with -ffp-contract=off, one rounding per written operation;
//   d2(i, j) = ((dx*dx + dy*dy) + dz*dz),  dx = p_j.x - p_i.x.
// The neighbours of i are the first min(max_nn, n) points in the order (d2(i, j), j), of them those
// with d2 < radius^2.  The points below radius^2 are a prefix of that order, so this is the first
// max_nn of the points with d2 < radius^2: a candidate at or past radius^2 is never held.
//
// Grid.  As outlier.hip's: vx_grid.h's keys with side `cell` and the min bound as origin, sorted as
// (key, index) pairs, the points gathered into that order (nn_grid.h).  `cell` and `max_rings` change
// the time only, never a result.
//
//   k_nm_ring    thread per query (in sorted order); its first max_nn candidates as (d2, sorted
//                position) pairs in two LDS columns d[j][thread], pos[j][thread] (8 + 4 bytes x max_nn x
//                128 threads; 64 threads past max_nn = 32: 48 KB at most).  Two pairs with equal d2
//                are ordered by the original index sidx[position], read only then.  After the shell at
//                Chebyshev distance r every unvisited point has a computed d2 > fl(g * g), g =
//                ring_bound() (nn_grid.h), so the query is resolved when it holds min(max_nn, n) pairs
//                with the largest d2 <= fl(g * g), or when fl(g * g) >= radius^2 whatever it holds (the
//                hybrid search's exit: with cell ~ radius no query goes further than ring 2).
//                Resolved: the column is sorted by (d2, index) and handed to nm_solve.  Not resolved
//                after max_rings: appended to a list (an integer counter, stats[0]).
//   k_nm_exact   a block per listed query streams all n points, each thread holding the first max_nn
//                of its share in its columns; the sorted columns are merged by rounds of a block
//                argmin on (d2, index), the winner's point entering the cumulants in every thread in
//                turn: the same neighbours in the same order as the ring path, the same bits.
//   nm_solve     the nine cumulants / m, the covariance, the cyclic Jacobi (pairs (0,1), (0,2), (1,2),
//                at most kNmSweeps sweeps, + - * / sqrt only), the eigenvector of the smallest
//                diagonal entry normalised, the prior's side; one thread per query.
//   k_nm_orient  thread per point: towards a camera location or along a direction.
// No kernel uses floating-point atomics or scratch: the Jacobi works on named scalars.
#include <cfloat>

#include "nn_grid.h"

namespace {

constexpr int kNmThreads = 128;      // ring / exact: max_nn x 128 x 12 bytes of LDS per block; 64 threads past kNmWideK
constexpr int kNmWideK = 32;
constexpr int kNmExactBlocks = 4096; // blocks of the exact pass (they stride over the list)
constexpr int kNmSweeps = 10;        // the Jacobi's cap (tests/normals_ref.py: at most 6 were ever needed)
static_assert(kNmWideK * kNmThreads * 12 <= 49152 && FVO_NORMALS_MAX_NN * 64 * 12 <= 49152, "the candidate columns");

enum { NM_EXACT = 0, NM_FEW = 1 };  // stats (int32): queries finished by the exact pass, points with m < 3

struct NmLayout {
  VxLayout vx;
  size_t spts, list, total;
};

int nm_layout(int64_t n, NmLayout& L) {
  if (vx_layout(n, L.vx)) return -1;
  size_t o = L.vx.total;
  auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes); return r; };
  L.spts = take(24 * (size_t)n);
  L.list = take(4 * (size_t)n);
  L.total = o;
  return 0;
}

// A thread's first k candidates in the order (d2, original index), unsorted, in its LDS columns
// D[j * st], P[j * st] (P: the sorted position); mx / mp / mpos: the last of them in that order, its
// sorted position and where it is.
struct NmTopK {
  double* D;
  int32_t* P;
  const int32_t* __restrict__ sidx;
  int st;  // the column stride: the block's threads
  int k, cnt, mpos;
  int32_t mp;
  double mx;
  __device__ __forceinline__ NmTopK(double* lds, int k_, const int32_t* sidx_)
      : D(lds + threadIdx.x), P(reinterpret_cast<int32_t*>(lds + (size_t)k_ * blockDim.x) + threadIdx.x), sidx(sidx_),
        st((int)blockDim.x), k(k_), cnt(0), mpos(0), mp(0), mx(0.0) {}
  // is (d, p) after (e, q) in the order
  __device__ __forceinline__ bool after(double d, int32_t p, double e, int32_t q) const {
    return d > e || (d == e && sidx[p] > sidx[q]);
  }
  __device__ __forceinline__ void insert(double d, int32_t p) {
    if (cnt < k) {
      D[cnt * st] = d;
      P[cnt * st] = p;
      if (cnt == 0 || after(d, p, mx, mp)) {
        mx = d;
        mp = p;
        mpos = cnt;
      }
      ++cnt;
    } else if (after(mx, mp, d, p)) {
      D[mpos * st] = d;
      P[mpos * st] = p;
      mx = D[0];
      mp = P[0];
      mpos = 0;
      for (int j = 1; j < k; ++j) {
        const double v = D[j * st];
        if (v >= mx) {
          const int32_t q = P[j * st];
          if (after(v, q, mx, mp)) {
            mx = v;
            mp = q;
            mpos = j;
          }
        }
      }
    }
  }
  // insertion sort of the cnt pairs into the order
  __device__ __forceinline__ void sort() {
    for (int i = 1; i < cnt; ++i) {
      const double v = D[i * st];
      const int32_t p = P[i * st];
      int j = i - 1;
      while (j >= 0 && after(D[j * st], P[j * st], v, p)) {
        D[(j + 1) * st] = D[j * st];
        P[(j + 1) * st] = P[j * st];
        --j;
      }
      D[(j + 1) * st] = v;
      P[(j + 1) * st] = p;
    }
  }
};

// utility::ComputeCovariance's nine cumulants x, y, z, xx, xy, xz, yy, yz, zz
struct NmCum {
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0, c5 = 0.0, c6 = 0.0, c7 = 0.0, c8 = 0.0;
  __device__ __forceinline__ void add(double x, double y, double z) {
    c0 = c0 + x;
    c1 = c1 + y;
    c2 = c2 + z;
    c3 = c3 + x * x;
    c4 = c4 + x * y;
    c5 = c5 + x * z;
    c6 = c6 + y * y;
    c7 = c7 + y * z;
    c8 = c8 + z * z;
  }
};

// One Jacobi rotation that zeroes a_pq; r is the third index.  (vkp, vkq): row k of V's columns p, q.
__device__ __forceinline__ void nm_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                          double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double th = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(th) + sqrt(th * th + 1.0));
  if (th < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp;
  arq = rq;
  const double x0 = c * v0p - s * v0q, y0 = s * v0p + c * v0q;
  v0p = x0;
  v0q = y0;
  const double x1 = c * v1p - s * v1q, y1 = s * v1p + c * v1q;
  v1p = x1;
  v1q = y1;
  const double x2 = c * v2p - s * v2q, y2 = s * v2p + c * v2q;
  v2p = x2;
  v2q = y2;
}

// From the cumulants of the m neighbours to point i's outputs.
__device__ __forceinline__ void nm_solve(const NmCum& u, int m, int64_t i, double* __restrict__ normals, int has_prior,
                                         double* __restrict__ cov, int32_t* __restrict__ n_neighbors,
                                         int32_t* __restrict__ stats) {
  double a00 = 1.0, a01 = 0.0, a02 = 0.0, a11 = 1.0, a12 = 0.0, a22 = 1.0;  // m < 3: the identity
  double nx = 0.0, ny = 0.0, nz = 1.0;
  if (m >= 3) {
    const double dm = (double)m;
    const double c0 = u.c0 / dm, c1 = u.c1 / dm, c2 = u.c2 / dm;
    a00 = u.c3 / dm - c0 * c0;
    a01 = u.c4 / dm - c0 * c1;
    a02 = u.c5 / dm - c0 * c2;
    a11 = u.c6 / dm - c1 * c1;
    a12 = u.c7 / dm - c1 * c2;
    a22 = u.c8 / dm - c2 * c2;
  } else {
    atomicAdd(&stats[NM_FEW], 1);
  }
  if (cov) {
    double* C = cov + 9 * i;
    C[0] = a00;
    C[1] = a01;
    C[2] = a02;
    C[3] = a01;
    C[4] = a11;
    C[5] = a12;
    C[6] = a02;
    C[7] = a12;
    C[8] = a22;
  }
  if (n_neighbors) n_neighbors[i] = m;
  const bool zero = a00 == 0.0 && a01 == 0.0 && a02 == 0.0 && a11 == 0.0 && a12 == 0.0 && a22 == 0.0;
  if (m >= 3 && !zero) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < kNmSweeps && !(a01 == 0.0 && a02 == 0.0 && a12 == 0.0); ++sweep) {
      nm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
      nm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
      nm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
    }
    // the smallest diagonal entry, ties to the lowest index (selects, not an indexed column: no scratch)
    const bool e1 = a11 < a00;
    const bool e2 = a22 < (e1 ? a11 : a00);
    const double x = e2 ? v02 : (e1 ? v01 : v00);
    const double y = e2 ? v12 : (e1 ? v11 : v10);
    const double z = e2 ? v22 : (e1 ? v21 : v20);
    const double len = sqrt((x * x + y * y) + z * z);
    nx = x / len;
    ny = y / len;
    nz = z / len;
  }
  double* N = normals + 3 * i;
  if (has_prior) {  // Open3D: a cloud that has normals keeps their side
    const double ox = N[0], oy = N[1], oz = N[2];
    if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
      nx = ox;
      ny = oy;
      nz = oz;
    } else if ((nx * ox + ny * oy) + nz * oz < 0.0) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
  }
  N[0] = nx;
  N[1] = ny;
  N[2] = nz;
}

__global__ __launch_bounds__(kNmThreads) void k_nm_ring(const double* __restrict__ sp,
                                                         const uint64_t* __restrict__ keys,
                                                         const int32_t* __restrict__ sidx, int64_t n, int k, double r2,
                                                         double cell, int max_rings,
                                                         const double* __restrict__ part, int nparts,
                                                         double* __restrict__ normals, int has_prior,
                                                         double* __restrict__ cov, int32_t* __restrict__ n_neighbors,
                                                         int32_t* __restrict__ list, int32_t* __restrict__ stats) {
  extern __shared__ double s_cols[];
  __shared__ double s_o[3];
  if (threadIdx.x < 3) s_o[threadIdx.x] = vx_origin(part, nparts, cell, 0.0, threadIdx.x);
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const double o[3] = {s_o[0], s_o[1], s_o[2]};
  const double p[3] = {sp[3 * s], sp[3 * s + 1], sp[3 * s + 2]};
  const uint64_t key = keys[s];
  const int64_t c[3] = {(int64_t)(key >> 42), (int64_t)((key >> 21) & 0x1FFFFF), (int64_t)(key & 0x1FFFFF)};
  NmTopK t(s_cols, k, sidx);
  // the points of the cells (x, y, z0 .. z1): one run of the sorted order
  auto visit = [&](int64_t x, int64_t y, int64_t z0, int64_t z1) {
    const uint64_t base = ((uint64_t)x << 42) | ((uint64_t)y << 21);
    const uint64_t hi = base | (uint64_t)z1;
    for (int64_t j = ol_lower_bound(keys, n, base | (uint64_t)z0); j < n && keys[j] <= hi; ++j) {
      const double d = ol_d2(p[0], p[1], p[2], sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]);
      if (d < r2) t.insert(d, (int32_t)j);
    }
  };
  bool resolved = false;
  for (int r = 0; r <= max_rings && !resolved; ++r) {
    for (int dx = -r; dx <= r; ++dx) {
      const int64_t x = c[0] + dx;
      if (x < 0 || x >= kVxCells) continue;
      for (int dy = -r; dy <= r; ++dy) {
        const int64_t y = c[1] + dy;
        if (y < 0 || y >= kVxCells) continue;
        if (max(abs(dx), abs(dy)) == r) {  // a side column of the shell: its whole z run
          visit(x, y, max(c[2] - r, (int64_t)0), min(c[2] + r, kVxCells - 1));
        } else {  // an inner column (r > 0): the shell's floor and ceiling cells
          if (c[2] - r >= 0) visit(x, y, c[2] - r, c[2] - r);
          if (c[2] + r < kVxCells) visit(x, y, c[2] + r, c[2] + r);
        }
      }
    }
    const double g = ring_bound(o, cell, p, c, r);
    resolved = g > 0.0 && (g * g >= r2 || (t.cnt == k && t.mx <= g * g));
  }
  if (!resolved) {
    list[atomicAdd(&stats[NM_EXACT], 1)] = (int32_t)s;
    return;
  }
  t.sort();
  NmCum u;
  for (int j = 0; j < t.cnt; ++j) {
    const int64_t q = t.P[j * t.st];
    u.add(sp[3 * q], sp[3 * q + 1], sp[3 * q + 2]);
  }
  nm_solve(u, t.cnt, sidx[s], normals, has_prior, cov, n_neighbors, stats);
}

__global__ __launch_bounds__(kNmThreads) void k_nm_exact(const double* __restrict__ sp,
                                                          const int32_t* __restrict__ sidx, int64_t n, int k, double r2,
                                                          const int32_t* __restrict__ list,
                                                          double* __restrict__ normals, int has_prior,
                                                          double* __restrict__ cov, int32_t* __restrict__ n_neighbors,
                                                          int32_t* __restrict__ stats) {
  extern __shared__ double s_cols[];
  __shared__ double s_wv[kNmThreads / 64];
  __shared__ int32_t s_wi[kNmThreads / 64], s_wp[kNmThreads / 64];
  const int tid = threadIdx.x;
  const int nlist = stats[NM_EXACT];  // final: the ring kernel has finished
  for (int u = blockIdx.x; u < nlist; u += gridDim.x) {  // uniform over the block
    const int64_t s = list[u];
    const double px = sp[3 * s], py = sp[3 * s + 1], pz = sp[3 * s + 2];
    NmTopK t(s_cols, k, sidx);
    // four points in flight per thread: the stream is bound by the loads' latency, not their number
    const int64_t T = blockDim.x;
    int64_t j = tid;
    for (; j + 3 * T < n; j += 4 * T) {
      double d[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int64_t q = j + a * T;
        d[a] = ol_d2(px, py, pz, sp[3 * q], sp[3 * q + 1], sp[3 * q + 2]);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
        if (d[a] < r2) t.insert(d[a], (int32_t)(j + a * T));
    }
    for (; j < n; j += T) {
      const double d = ol_d2(px, py, pz, sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]);
      if (d < r2) t.insert(d, (int32_t)j);
    }
    t.sort();
    // up to k rounds: the first head of the sorted columns in the order leaves its column
    int head = 0, m = 0;
    NmCum cum;
    for (int r = 0; r < k; ++r) {
      const bool has = head < t.cnt;
      double v = has ? t.D[head * t.st] : INFINITY;
      int32_t pos = has ? t.P[head * t.st] : 0;
      const int32_t mine = has ? sidx[pos] : INT32_MAX;
      int32_t oi = mine;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int32_t oo = __shfl_xor(oi, off, 64);
        const int32_t op = __shfl_xor(pos, off, 64);
        if (ov < v || (ov == v && oo < oi)) {
          v = ov;
          oi = oo;
          pos = op;
        }
      }
      if (wave_lane() == 0) {
        s_wv[tid >> 6] = v;
        s_wi[tid >> 6] = oi;
        s_wp[tid >> 6] = pos;
      }
      __syncthreads();
      v = s_wv[0];
      oi = s_wi[0];
      pos = s_wp[0];
      for (int q = 1; q < (int)(blockDim.x >> 6); ++q)
        if (s_wv[q] < v || (s_wv[q] == v && s_wi[q] < oi)) {
          v = s_wv[q];
          oi = s_wi[q];
          pos = s_wp[q];
        }
      __syncthreads();
      if (oi == INT32_MAX) break;  // every column is empty: uniform over the block
      if (mine == oi) ++head;
      cum.add(sp[3 * (int64_t)pos], sp[3 * (int64_t)pos + 1], sp[3 * (int64_t)pos + 2]);
      ++m;
    }
    if (tid == 0) nm_solve(cum, m, sidx[s], normals, has_prior, cov, n_neighbors, stats);
    __syncthreads();  // the columns are rewritten by the next query
  }
}

// mode 0: ref = camera - p; mode 1: ref = the direction.  A zero normal becomes ref normalised
// ((0, 0, 1) where ref is 0 too), any other is negated when it points away from ref.
__global__ __launch_bounds__(256) void k_nm_orient(const double* __restrict__ p, double* __restrict__ normals, int64_t n,
                                                   int mode, double rx, double ry, double rz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (mode == 0) {
    rx = rx - p[3 * i];
    ry = ry - p[3 * i + 1];
    rz = rz - p[3 * i + 2];
  }
  double nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
  if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
    if (rx == 0.0 && ry == 0.0 && rz == 0.0) {
      nz = 1.0;
    } else {
      const double len = sqrt((rx * rx + ry * ry) + rz * rz);
      nx = rx / len;
      ny = ry / len;
      nz = rz / len;
    }
  } else if ((nx * rx + ny * ry) + nz * rz < 0.0) {
    nx = -nx;
    ny = -ny;
    nz = -nz;
  } else {
    return;
  }
  normals[3 * i] = nx;
  normals[3 * i + 1] = ny;
  normals[3 * i + 2] = nz;
}

}  // namespace

int64_t normals_workspace_bytes(int64_t n) {
  NmLayout L;
  if (n < 1 || nm_layout(n, L)) return -1;
  return (int64_t)L.total;
}

int estimate_normals_run(fvo_ctx* ctx, const double* pts, int64_t n, int max_nn, double radius, double cell,
                         int max_rings, void* ws, double* normals, int has_prior, double* covariances,
                         int32_t* n_neighbors, int32_t* stats, int32_t* status, hipStream_t s) {
  // arguments were validated by capi_normals.cpp (the workspace size against normals_workspace_bytes)
  NmLayout L;
  if (nm_layout(n, L)) return fvo_fail(ctx, "estimate_normals: workspace size query failed");  // a hipcub error
  char* w = (char*)ws;
  int32_t* st = status ? status : (int32_t*)(w + L.vx.status);
  const double* sp = (const double*)(w + L.spts);
  const uint64_t* keys = (const uint64_t*)(w + L.vx.keys_b);
  const int32_t* sidx = (const int32_t*)(w + L.vx.idx_b);
  int32_t* list = (int32_t*)(w + L.list);
  FVO_HIP(ctx, hipMemsetAsync(st, 0, 4, s));
  FVO_HIP(ctx, hipMemsetAsync(stats, 0, 8, s));
  vx_sort_keys(pts, n, cell, 0.0, w, L.vx, st, s);
  FVO_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_ol_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts, sidx, n, (double*)(w + L.spts));
  FVO_LAUNCH_CHECK(ctx);
  const int k = (int)(n < max_nn ? n : max_nn);
  const int nt = max_nn > kNmWideK ? 64 : kNmThreads;
  const size_t lds = (size_t)k * nt * 12;
  const double r2 = radius * radius;
  hipLaunchKernelGGL(k_nm_ring, dim3((unsigned)((n + nt - 1) / nt)), dim3(nt), lds, s, sp, keys, sidx, n, k, r2, cell,
                     max_rings, (const double*)(w + L.vx.part), vx_parts(n), normals, has_prior, covariances, n_neighbors,
                     list, stats);
  FVO_LAUNCH_CHECK(ctx);
  const unsigned ge = (unsigned)(n < kNmExactBlocks ? n : kNmExactBlocks);
  hipLaunchKernelGGL(k_nm_exact, dim3(ge), dim3(nt), lds, s, sp, sidx, n, k, r2, list, normals, has_prior, covariances,
                     n_neighbors, stats);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int orient_normals_run(fvo_ctx* ctx, const double* pts, double* normals, int64_t n, int mode, const double* ref,
                       hipStream_t s) {
  // arguments were validated by capi_normals.cpp; ref is read here, on the host, before the launch
  hipLaunchKernelGGL(k_nm_orient, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts, normals, n, mode, ref[0],
                     ref[1], ref[2]);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
