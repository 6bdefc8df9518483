// The uniform-grid cell table shared by map.hip (voxel_down_sample) and, through nn_grid.h, outlier.hip
// and normals.hip (the neighbour searches): min bound by block partials, cell keys floor((p - vmin) / cell) packed 3x21 bits,
// stable radix sort of (key, index) (hipcub), and for the voxel filter segment heads + exclusive scan
// + the cell start table (the neighbour searches find a run of cells in the sorted keys directly).
// Included by .hip files only; everything is in the anonymous namespace, so each translation unit
// (each its own code object) carries its own copy of these kernels.
#pragma once

#include <hipcub/hipcub.hpp>

#include "fvo_device.h"

namespace {

constexpr int kVxBlocks = 256;
constexpr int64_t kVxCells = 2097152;  // cells per axis: 21 bits of the key each (x high, z low)

__global__ __launch_bounds__(256) void k_vx_bounds(const double* __restrict__ p, int64_t n, double* __restrict__ part) {
  __shared__ double sm[6][256];
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = p[3 * i + k];
      mn[k] = fmin(mn[k], v);
      mx[k] = fmax(mx[k], v);
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    sm[k][threadIdx.x] = mn[k];
    sm[3 + k][threadIdx.x] = mx[k];
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        sm[k][threadIdx.x] = fmin(sm[k][threadIdx.x], sm[k][threadIdx.x + s]);
        sm[3 + k][threadIdx.x] = fmax(sm[3 + k][threadIdx.x], sm[3 + k][threadIdx.x + s]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = sm[threadIdx.x][0];
}

// The grid's origin along one axis: the min over the block partials (min/max are exact, any
// order) less `shift` cells (0.5: Eigen `GetMinBound() - voxel_size3 * 0.5`; 0: the min bound itself).
__device__ __forceinline__ double vx_origin(const double* __restrict__ part, int nparts, double voxel, double shift,
                                            int axis) {
  double m = INFINITY;
  for (int j = 0; j < nparts; ++j) m = fmin(m, part[j * 6 + axis]);
  return m - voxel * shift;
}

// keys: ref = (p - vmin) / v, index = int(floor(ref)).
__global__ __launch_bounds__(256) void k_vx_keys(const double* __restrict__ p, int64_t n, double voxel, double shift,
                                                 const double* __restrict__ part, int nparts,
                                                 uint64_t* __restrict__ keys, int32_t* __restrict__ idx,
                                                 int32_t* __restrict__ status) {
  __shared__ double vmin[3];
  if (threadIdx.x < 3) vmin[threadIdx.x] = vx_origin(part, nparts, voxel, shift, threadIdx.x);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t key = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ref = (p[3 * i + k] - vmin[k]) / voxel;
    const double f = floor(ref);
    int64_t v = (f >= 0.0 && f < 2097152.0) ? (int64_t)f : -1;
    if (v < 0) {
      status[0] = 1;  // outside the 21-bit key range (or not finite): result invalid, reported
      v = 0;
    }
    key = (key << 21) | (uint64_t)v;
  }
  keys[i] = key;
  idx[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_vx_heads(const uint64_t* __restrict__ keys, int64_t n,
                                                  int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_vx_starts(const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                   int64_t n, int32_t* __restrict__ start,
                                                   int32_t* __restrict__ n_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) start[pos[i]] = (int32_t)i;
  if (i == n - 1) {
    const int32_t nv = pos[i] + flag[i];
    start[nv] = (int32_t)n;
    n_out[0] = nv;
  }
}

struct VxLayout {
  size_t keys_a, keys_b, idx_a, idx_b, flag, pos, start, part, status, cub, total, sort_bytes, scan_bytes;
};

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

inline int vx_layout(int64_t n, VxLayout& L) {
  size_t sort_bytes = 0, scan_bytes = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (const int32_t*)nullptr, (int32_t*)nullptr, (int)n, 0, 63) != hipSuccess)
    return -1;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n) !=
      hipSuccess)
    return -1;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes); return r; };
  L.keys_a = take(8 * (size_t)n);
  L.keys_b = take(8 * (size_t)n);
  L.idx_a = take(4 * (size_t)n);
  L.idx_b = take(4 * (size_t)n);
  L.flag = take(4 * (size_t)n);
  L.pos = take(4 * (size_t)n);
  L.start = take(4 * ((size_t)n + 1));
  L.part = take(8 * 6 * kVxBlocks);
  L.status = take(4);
  L.sort_bytes = sort_bytes;
  L.scan_bytes = scan_bytes;
  L.cub = take(sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
  L.total = o;
  return 0;
}

inline int vx_parts(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (int)(g < kVxBlocks ? g : kVxBlocks);
}

// Bounds, keys and the sort on stream s, in the workspace w laid out by L: on return
// (stream-ordered) keys_b / idx_b hold the sorted (key, index) pairs.  st: the status word.
inline void vx_sort_keys(const double* pts, int64_t n, double voxel, double shift, char* w, const VxLayout& L,
                         int32_t* st, hipStream_t s) {
  uint64_t *ka = (uint64_t*)(w + L.keys_a), *kb = (uint64_t*)(w + L.keys_b);
  int32_t *ia = (int32_t*)(w + L.idx_a), *ib = (int32_t*)(w + L.idx_b);
  double* part = (double*)(w + L.part);
  const unsigned g = (unsigned)((n + 255) / 256);
  const int nparts = vx_parts(n);
  hipLaunchKernelGGL(k_vx_bounds, dim3(nparts), dim3(256), 0, s, pts, n, part);
  hipLaunchKernelGGL(k_vx_keys, dim3(g), dim3(256), 0, s, pts, n, voxel, shift, part, nparts, ka, ia, st);
  size_t sb = L.sort_bytes;
  (void)hipcub::DeviceRadixSort::SortPairs(w + L.cub, sb, ka, kb, ia, ib, (int)n, 0, 63, s);
}

// Heads, scan, starts over the sorted keys: pos = the cell number of every sorted position,
// start[0 .. nv] the cell start table and *n_cells = nv.
inline void vx_cell_table(int64_t n, char* w, const VxLayout& L, int32_t* n_cells, hipStream_t s) {
  const uint64_t* kb = (const uint64_t*)(w + L.keys_b);
  int32_t *flag = (int32_t*)(w + L.flag), *pos = (int32_t*)(w + L.pos), *start = (int32_t*)(w + L.start);
  const unsigned g = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_vx_heads, dim3(g), dim3(256), 0, s, kb, n, flag);
  size_t cb = L.scan_bytes;
  (void)hipcub::DeviceScan::ExclusiveSum(w + L.cub, cb, flag, pos, (int)n, s);
  hipLaunchKernelGGL(k_vx_starts, dim3(g), dim3(256), 0, s, flag, pos, n, start, n_cells);
}

}  // namespace
