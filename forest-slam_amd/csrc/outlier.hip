// Point-cloud outlier removal for gfx950: Open3D PointCloud::RemoveStatisticalOutliers and
// RemoveRadiusOutliers (fvo_statistical_outliers, fvo_radius_outliers) and the order-preserving
// selection of the kept points (fvo_select_points).  Specification: tests/outlier_ref.py (restated
// from Open3D 0.17, unpinned).  All arithmetic is fp64, compiled with -ffp-contract=off;
//   d2(i, j) = ((dx*dx + dy*dy) + dz*dz),  dx = p_j.x - p_i.x.
//
// Grid.  vx_grid.h's keys with side `cell` and the min bound as origin, sorted as (key, index)
// pairs; k_ol_gather puts the points in that order, so a cell's points, and the cells of one z run
// (the key's low 21 bits), are contiguous.  A run of cells is found by one binary search in the
// sorted keys.  `cell` changes the time only, never the result.
//
// Statistical.
//   k_ol_ring    thread per query (in sorted order), its k smallest d2 in an LDS column
//                (list[j][thread], k x 128 doubles per block; 64 threads when k > 48).  The shells at Chebyshev distance
//                r = 0 .. max_rings of the query's cell are visited in turn; after shell r every
//                unvisited point is at least b_r away (the nearest face of the visited cube), and the
//                query is resolved when it holds k values with the k-th <= b_r (ring_bound() for the
//                rounding margin).  Resolved: the list is sorted, avg = (sum of sqrt ascending) / k.
//                Not resolved after max_rings: appended to a list (an integer counter).
//   k_ol_exact   a block per listed query streams all n points, each thread keeping the k smallest
//                of its share in its LDS column; the columns are sorted and merged by k rounds
//                of a block argmin.  The same d2, the same k smallest values, the same ascending
//                sum: the same bits as the ring path.  n < nb_neighbors lists every query.
//   k_ol_sum1 / k_ol_sum2 / k_ol_mask / k_ol_finish   mean and deviation by deterministic two-level
//                sums (per-thread chains of <= 2048 terms in index order, xor-shuffle wave sums,
//                waves in order, <= 4096 block partials summed the same way), then the mask.
// Radius.  k_ol_radius: thread per query; the cells within ceil(radius / cell) + 1 (the + 1: the
//   floor of a rounded quotient can be one cell off), less the columns and z ends whose nearest face
//   is provably >= radius away; count of d2 < radius^2.
// Selection.  k_ol_select: blocks of 256 threads x 4 consecutive points; a block counts the kept
//   flags before it (the call has no workspace: 16-byte loads of the mask, a few hundred KB from L2
//   per block at a million points), ranks its own (block_rank) and emits.  No block waits for another.
#include <cfloat>

#include "nn_grid.h"

namespace {

constexpr int kOlThreads = 128;      // ring / exact: k x 128 doubles of LDS per block; 64 threads past kOlWideK
constexpr int kOlWideK = 48;         // (48 KB + the static words stay inside the 64 KB a block gets by default)
constexpr int kOlMaxParts = 4096;    // block partials of the sums
constexpr int kOlExactBlocks = 4096; // blocks of the exact pass (they stride over the list)
static_assert(kOlWideK * kOlThreads * 8 <= 49152 && FVO_OUTLIER_MAX_K * 64 * 8 <= 49152, "the top-k columns");

// counters (int32) in the workspace
enum { OL_UNRESOLVED = 0, OL_KEPT = 1, OL_COUNTERS = 2 };

struct OlLayout {
  VxLayout vx;
  size_t spts, avg, list, part1, part2, counters, total;
};

int ol_layout(int64_t n, OlLayout& L) {
  if (vx_layout(n, L.vx)) return -1;
  size_t o = L.vx.total;
  auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes); return r; };
  L.spts = take(24 * (size_t)n);
  L.avg = take(8 * (size_t)n);
  L.list = take(4 * (size_t)n);
  L.part1 = take(8 * kOlMaxParts);
  L.part2 = take(8 * kOlMaxParts);
  L.counters = take(4 * OL_COUNTERS);
  L.total = o;
  return 0;
}

__global__ __launch_bounds__(256) void k_ol_iota(int64_t n, int32_t* __restrict__ list, int32_t* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) list[i] = (int32_t)i;
  if (i == 0) counters[OL_UNRESOLVED] = (int32_t)n;
}

// A thread's k smallest values, unsorted, in its LDS column L[j * threads]; mx / mpos: the largest
// of them and where it is.  Equal values need no rule: only the values are used.
struct TopK {
  double* L;
  int st;  // the column stride: the block's threads
  int k, cnt, mpos;
  double mx;
  __device__ __forceinline__ TopK(double* lds, int k_) : L(lds + threadIdx.x), st((int)blockDim.x), k(k_), cnt(0), mpos(0), mx(0.0) {}
  __device__ __forceinline__ void insert(double d) {
    if (cnt < k) {
      L[cnt * st] = d;
      if (cnt == 0 || d > mx) {
        mx = d;
        mpos = cnt;
      }
      ++cnt;
    } else if (d < mx) {
      L[mpos * st] = d;
      mx = L[0];
      mpos = 0;
      for (int j = 1; j < k; ++j) {
        const double v = L[j * st];
        if (v > mx) {
          mx = v;
          mpos = j;
        }
      }
    }
  }
  // ascending insertion sort of the cnt values
  __device__ __forceinline__ void sort() {
    for (int i = 1; i < cnt; ++i) {
      const double v = L[i * st];
      int j = i - 1;
      while (j >= 0 && L[j * st] > v) {
        L[(j + 1) * st] = L[j * st];
        --j;
      }
      L[(j + 1) * st] = v;
    }
  }
};

__global__ __launch_bounds__(kOlThreads) void k_ol_ring(const double* __restrict__ sp,
                                                         const uint64_t* __restrict__ keys,
                                                         const int32_t* __restrict__ sidx, int64_t n, int k,
                                                         double cell, int max_rings,
                                                         const double* __restrict__ part, int nparts,
                                                         double* __restrict__ avg, int32_t* __restrict__ list,
                                                         int32_t* __restrict__ counters) {
  extern __shared__ double s_list[];
  __shared__ double s_o[3];
  if (threadIdx.x < 3) s_o[threadIdx.x] = vx_origin(part, nparts, cell, 0.0, threadIdx.x);
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const double o[3] = {s_o[0], s_o[1], s_o[2]};
  const double p[3] = {sp[3 * s], sp[3 * s + 1], sp[3 * s + 2]};
  const uint64_t key = keys[s];
  const int64_t c[3] = {(int64_t)(key >> 42), (int64_t)((key >> 21) & 0x1FFFFF), (int64_t)(key & 0x1FFFFF)};
  TopK t(s_list, k);
  // the points of the cells (x, y, z0 .. z1): one run of the sorted order
  auto visit = [&](int64_t x, int64_t y, int64_t z0, int64_t z1) {
    const uint64_t base = ((uint64_t)x << 42) | ((uint64_t)y << 21);
    const uint64_t hi = base | (uint64_t)z1;
    for (int64_t j = ol_lower_bound(keys, n, base | (uint64_t)z0); j < n && keys[j] <= hi; ++j)
      t.insert(ol_d2(p[0], p[1], p[2], sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]));
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
    if (t.cnt == k) {
      const double g = ring_bound(o, cell, p, c, r);
      resolved = g > 0.0 && t.mx <= g * g;
    }
  }
  if (resolved) {
    t.sort();
    double sum = 0.0;
    for (int j = 0; j < k; ++j) sum = sum + sqrt(t.L[j * t.st]);
    avg[sidx[s]] = sum / (double)k;
  } else {
    list[atomicAdd(&counters[OL_UNRESOLVED], 1)] = (int32_t)s;
  }
}

__global__ __launch_bounds__(kOlThreads) void k_ol_exact(const double* __restrict__ sp,
                                                          const int32_t* __restrict__ sidx, int64_t n, int k,
                                                          const int32_t* __restrict__ list,
                                                          const int32_t* __restrict__ counters,
                                                          double* __restrict__ avg) {
  extern __shared__ double s_list[];
  __shared__ double s_wv[kOlThreads / 64];
  __shared__ int s_wt[kOlThreads / 64];
  const int tid = threadIdx.x;
  const int nlist = counters[OL_UNRESOLVED];
  for (int u = blockIdx.x; u < nlist; u += gridDim.x) {  // uniform over the block
    const int64_t s = list[u];
    const double px = sp[3 * s], py = sp[3 * s + 1], pz = sp[3 * s + 2];
    TopK t(s_list, k);
    for (int64_t j = tid; j < n; j += blockDim.x) t.insert(ol_d2(px, py, pz, sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]));
    t.sort();
    // k rounds: the smallest head of the sorted columns leaves its column (ties: the lowest thread)
    int head = 0;
    double sum = 0.0;
    for (int r = 0; r < k; ++r) {
      double v = head < t.cnt ? t.L[head * t.st] : INFINITY;
      int w = tid;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int ow = __shfl_xor(w, off, 64);
        if (ov < v || (ov == v && ow < w)) {
          v = ov;
          w = ow;
        }
      }
      if (wave_lane() == 0) {
        s_wv[tid >> 6] = v;
        s_wt[tid >> 6] = w;
      }
      __syncthreads();
      v = s_wv[0];
      w = s_wt[0];
      for (int q = 1; q < (int)(blockDim.x >> 6); ++q)
        if (s_wv[q] < v) {  // the waves in order: an equal value keeps the lower thread
          v = s_wv[q];
          w = s_wt[q];
        }
      __syncthreads();
      if (tid == w) ++head;
      sum = sum + sqrt(v);
    }
    if (tid == 0) avg[sidx[s]] = sum / (double)k;
    __syncthreads();  // the columns are rewritten by the next query
  }
}

// ---------------------------------------------------------------- mean, deviation, mask
// The sum of f(avg_i) over the points with avg_i > 0: a thread's chain runs over i = t, t + T, ...
// (T = threads of the grid; <= 2048 terms for n <= INT32_MAX at 4096 blocks), block_sum, one partial
// per block.
template <bool DEV>
__device__ __forceinline__ double ol_chain(const double* __restrict__ avg, int64_t n, double mean) {
  double a = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double v = avg[i];
    if (v > 0.0) a = a + (DEV ? (v - mean) * (v - mean) : v);
  }
  return a;
}

// the sum of the block partials, the same in every thread of every block (256 chains of <= 16 terms)
__device__ __forceinline__ double ol_total(const double* __restrict__ part, int nparts, double* s_red) {
  double a = 0.0;
  for (int j = threadIdx.x; j < nparts; j += 256) a = a + part[j];
  return block_sum<256>(a, s_red);
}

__global__ __launch_bounds__(256) void k_ol_sum1(const double* __restrict__ avg, int64_t n, double* __restrict__ part1) {
  __shared__ double s_red[4];
  const double t = block_sum<256>(ol_chain<false>(avg, n, 0.0), s_red);
  if (threadIdx.x == 0) part1[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void k_ol_sum2(const double* __restrict__ avg, int64_t n,
                                                 const double* __restrict__ part1, double* __restrict__ part2) {
  __shared__ double s_red[4];
  const double mean = ol_total(part1, gridDim.x, s_red) / (double)n;
  const double t = block_sum<256>(ol_chain<true>(avg, n, mean), s_red);
  if (threadIdx.x == 0) part2[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void k_ol_mask(const double* __restrict__ avg, int64_t n,
                                                 const double* __restrict__ part1, const double* __restrict__ part2,
                                                 int nparts, double std_ratio, uint8_t* __restrict__ keep,
                                                 int32_t* __restrict__ counters, double* __restrict__ stats) {
  __shared__ double s_red[4];
  __shared__ int s_w[4];
  const double mean = ol_total(part1, nparts, s_red) / (double)n;
  const double sd = sqrt(ol_total(part2, nparts, s_red) / (double)(n - 1));
  const double thr = mean + std_ratio * sd;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = mean;
    stats[1] = sd;
    stats[2] = thr;
    stats[3] = (double)n;
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool kp = false;
  if (i < n) {
    const double v = avg[i];
    kp = v > 0.0 && v < thr;
    keep[i] = kp ? 1 : 0;
  }
  int total;
  block_rank<256>(kp, s_w, total);
  if (threadIdx.x == 0 && total) atomicAdd(&counters[OL_KEPT], total);
}

__global__ void k_ol_finish(const int32_t* __restrict__ counters, double* __restrict__ stats) {
  if (threadIdx.x != 0) return;
  stats[4] = (double)counters[OL_KEPT];
  stats[5] = (double)counters[OL_UNRESOLVED];
}

// ---------------------------------------------------------------- radius
// g2 of an axis offset d (cells): 0 for the query's own slab, else face_gap^2 towards that slab: a
// lower bound of the squared axis distance to every point of it, below every such computed square.
__device__ __forceinline__ double ol_axis_g2(double o, double cell, double p, int64_t c, int d) {
  if (d == 0) return 0.0;
  const double g = d > 0 ? face_gap(o, cell, p, c + d, 1) : face_gap(o, cell, p, c + d + 1, -1);
  return g > 0.0 ? g * g : 0.0;
}

__global__ __launch_bounds__(256) void k_ol_radius(const double* __restrict__ sp, const uint64_t* __restrict__ keys,
                                                   const int32_t* __restrict__ sidx, int64_t n, double r2, int R,
                                                   double cell, int nb_points, const double* __restrict__ part,
                                                   int nparts, uint8_t* __restrict__ keep,
                                                   int32_t* __restrict__ n_neighbors) {
  __shared__ double s_o[3];
  if (threadIdx.x < 3) s_o[threadIdx.x] = vx_origin(part, nparts, cell, 0.0, threadIdx.x);
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const double px = sp[3 * s], py = sp[3 * s + 1], pz = sp[3 * s + 2];
  const uint64_t key = keys[s];
  const int64_t cx = (int64_t)(key >> 42), cy = (int64_t)((key >> 21) & 0x1FFFFF), cz = (int64_t)(key & 0x1FFFFF);
  int count = 0;
  for (int dx = -R; dx <= R; ++dx) {
    const int64_t x = cx + dx;
    if (x < 0 || x >= kVxCells) continue;
    const double gx = ol_axis_g2(s_o[0], cell, px, cx, dx);
    if (gx >= r2) continue;  // every d2 of the slab is > gx >= r2
    for (int dy = -R; dy <= R; ++dy) {
      const int64_t y = cy + dy;
      if (y < 0 || y >= kVxCells) continue;
      const double gxy = gx + ol_axis_g2(s_o[1], cell, py, cy, dy);
      if (gxy >= r2) continue;
      int z0 = -R, z1 = R;  // drop the ends of the z run that are out of reach
      while (z0 < 0 && gxy + ol_axis_g2(s_o[2], cell, pz, cz, z0) >= r2) ++z0;
      while (z1 > 0 && gxy + ol_axis_g2(s_o[2], cell, pz, cz, z1) >= r2) --z1;
      const int64_t za = max(cz + z0, (int64_t)0), zb = min(cz + z1, kVxCells - 1);
      const uint64_t base = ((uint64_t)x << 42) | ((uint64_t)y << 21);
      const uint64_t hi = base | (uint64_t)zb;
      for (int64_t j = ol_lower_bound(keys, n, base | (uint64_t)za); j < n && keys[j] <= hi; ++j)
        count += ol_d2(px, py, pz, sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]) < r2 ? 1 : 0;
    }
  }
  const int64_t i = sidx[s];
  keep[i] = count > nb_points ? 1 : 0;
  if (n_neighbors) n_neighbors[i] = count;
}

// ---------------------------------------------------------------- selection
constexpr int kSelBlock = 1024;  // 256 threads x 4 consecutive points

// non-zero bytes of a 32-bit word
__device__ __forceinline__ int nz_bytes(uint32_t w) {
  return __popc((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u);
}

__global__ __launch_bounds__(256) void k_ol_select(const double* __restrict__ p, int64_t n,
                                                   const uint8_t* __restrict__ keep, double* __restrict__ out64,
                                                   float* __restrict__ out32, int32_t* __restrict__ n_out) {
  __shared__ int s_red[4];
  __shared__ int s_w[4];
  const int tid = threadIdx.x;
  // kept flags before this block: bytes [0, len), the 16-byte aligned middle by uint4 loads
  const int64_t len = (int64_t)blockIdx.x * kSelBlock;
  const int64_t head = min(len, (int64_t)((16 - (reinterpret_cast<uintptr_t>(keep) & 15)) & 15));
  const int64_t nvec = (len - head) / 16;
  int before = 0;
  const uint4* kv = reinterpret_cast<const uint4*>(keep + head);
  for (int64_t j = tid; j < nvec; j += 256) {
    const uint4 v = kv[j];
    before += nz_bytes(v.x) + nz_bytes(v.y) + nz_bytes(v.z) + nz_bytes(v.w);
  }
  for (int64_t j = tid; j < head; j += 256) before += keep[j] != 0;
  for (int64_t j = head + 16 * nvec + tid; j < len; j += 256) before += keep[j] != 0;
  before = block_sum<256>(before, s_red);
  const int64_t i0 = len + 4 * (int64_t)tid;
  bool kp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) kp[j] = i0 + j < n && keep[i0 + j] != 0;
  int total;
  int64_t o = (int64_t)before + block_rank<256, 4>(kp, s_w, total);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!kp[j]) continue;
    const double x = p[3 * (i0 + j)], y = p[3 * (i0 + j) + 1], z = p[3 * (i0 + j) + 2];
    if (out64) {
      out64[3 * o] = x;
      out64[3 * o + 1] = y;
      out64[3 * o + 2] = z;
    }
    if (out32) {
      out32[3 * o] = (float)x;
      out32[3 * o + 1] = (float)y;
      out32[3 * o + 2] = (float)z;
    }
    ++o;
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) n_out[0] = before + total;
}

// the shared front of both searches: counters and status cleared, the cell table, the sorted points
int ol_grid(fvo_ctx* ctx, const double* pts, int64_t n, double cell, char* w, const OlLayout& L, int32_t* st,
            hipStream_t s) {
  int32_t* counters = (int32_t*)(w + L.counters);
  FVO_HIP(ctx, hipMemsetAsync(st, 0, 4, s));
  FVO_HIP(ctx, hipMemsetAsync(counters, 0, 4 * OL_COUNTERS, s));
  vx_sort_keys(pts, n, cell, 0.0, w, L.vx, st, s);
  FVO_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_ol_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts,
                     (const int32_t*)(w + L.vx.idx_b), n, (double*)(w + L.spts));
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

}  // namespace

int64_t outlier_workspace_bytes(int64_t n) {
  OlLayout L;
  if (n < 1 || ol_layout(n, L)) return -1;
  return (int64_t)L.total;
}

int statistical_outliers_run(fvo_ctx* ctx, const double* pts, int64_t n, int nb_neighbors, double std_ratio,
                             double cell, int max_rings, void* ws, uint8_t* keep, double* avg_distance, double* stats,
                             int32_t* status, hipStream_t s) {
  // arguments were validated by capi_outlier.cpp (the workspace size against outlier_workspace_bytes)
  OlLayout L;
  if (ol_layout(n, L)) return fvo_fail(ctx, "statistical_outliers: workspace size query failed");  // a hipcub error
  char* w = (char*)ws;
  int32_t* st = status ? status : (int32_t*)(w + L.vx.status);
  int32_t* counters = (int32_t*)(w + L.counters);
  int32_t* list = (int32_t*)(w + L.list);
  const double* sp = (const double*)(w + L.spts);
  const uint64_t* keys = (const uint64_t*)(w + L.vx.keys_b);
  const int32_t* sidx = (const int32_t*)(w + L.vx.idx_b);
  double* avg = avg_distance ? avg_distance : (double*)(w + L.avg);
  double *part1 = (double*)(w + L.part1), *part2 = (double*)(w + L.part2);
  if (int rc = ol_grid(ctx, pts, n, cell, w, L, st, s)) return rc;
  const int k = (int)(n < nb_neighbors ? n : nb_neighbors);
  const int nt = k > kOlWideK ? 64 : kOlThreads;
  const size_t lds = (size_t)k * nt * sizeof(double);
  const unsigned g256 = (unsigned)((n + 255) / 256);
  if (n < nb_neighbors)  // the ring search can never hold k values: every query to the exact pass
    hipLaunchKernelGGL(k_ol_iota, dim3(g256), dim3(256), 0, s, n, list, counters);
  else
    hipLaunchKernelGGL(k_ol_ring, dim3((unsigned)((n + nt - 1) / nt)), dim3(nt), lds, s, sp,
                       keys, sidx, n, k, cell, max_rings, (const double*)(w + L.vx.part), vx_parts(n), avg, list,
                       counters);
  FVO_LAUNCH_CHECK(ctx);
  const unsigned ge = (unsigned)(n < kOlExactBlocks ? n : kOlExactBlocks);
  hipLaunchKernelGGL(k_ol_exact, dim3(ge), dim3(nt), lds, s, sp, sidx, n, k, list, counters, avg);
  FVO_LAUNCH_CHECK(ctx);
  const unsigned np = g256 < (unsigned)kOlMaxParts ? g256 : (unsigned)kOlMaxParts;
  hipLaunchKernelGGL(k_ol_sum1, dim3(np), dim3(256), 0, s, avg, n, part1);
  hipLaunchKernelGGL(k_ol_sum2, dim3(np), dim3(256), 0, s, avg, n, part1, part2);
  hipLaunchKernelGGL(k_ol_mask, dim3(g256), dim3(256), 0, s, avg, n, part1, part2, (int)np, std_ratio, keep, counters,
                     stats);
  hipLaunchKernelGGL(k_ol_finish, dim3(1), dim3(64), 0, s, counters, stats);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int radius_outliers_run(fvo_ctx* ctx, const double* pts, int64_t n, int nb_points, double radius, double cell,
                        void* ws, uint8_t* keep, int32_t* n_neighbors, int32_t* status, hipStream_t s) {
  // arguments were validated by capi_outlier.cpp (radius / cell <= 8, so R <= 9)
  OlLayout L;
  if (ol_layout(n, L)) return fvo_fail(ctx, "radius_outliers: workspace size query failed");  // a hipcub error
  char* w = (char*)ws;
  int32_t* st = status ? status : (int32_t*)(w + L.vx.status);
  if (int rc = ol_grid(ctx, pts, n, cell, w, L, st, s)) return rc;
  const int R = (int)ceil(radius / cell) + 1;
  hipLaunchKernelGGL(k_ol_radius, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)(w + L.spts),
                     (const uint64_t*)(w + L.vx.keys_b), (const int32_t*)(w + L.vx.idx_b), n, radius * radius, R, cell,
                     nb_points, (const double*)(w + L.vx.part), vx_parts(n), keep, n_neighbors);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int select_points_run(fvo_ctx* ctx, const double* pts, int64_t n, const uint8_t* keep, double* out64, float* out32,
                      int32_t* n_out, hipStream_t s) {
  // arguments were validated by capi_outlier.cpp
  hipLaunchKernelGGL(k_ol_select, dim3((unsigned)((n + kSelBlock - 1) / kSelBlock)), dim3(256), 0, s, pts, n, keep,
                     out64, out32, n_out);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
