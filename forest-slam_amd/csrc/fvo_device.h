// Device-side helpers shared by the HIP translation units (the host-only declarations are in
// fvo_internal.h, which capi.cpp includes alone: it compiles as plain host C++ too, e.g. for
// the sanitizer build of the argument validation, tools/sanitize.sh).
#pragma once

#include "fvo_internal.h"

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ int wave_lane() { return (int)(threadIdx.x & 63); }

// XCD-aware block order.  Dispatch sends linear block L to XCD L mod 8, so neighbouring
// blocks (which read overlapping image rows / patches) would land in 8 different L2s; the
// logical index returned here hands each XCD one contiguous eighth of the grid instead.
struct XcdBlock {
  int x, y, z;
};
__device__ __forceinline__ XcdBlock xcd_block() {
  const int gx = gridDim.x, gy = gridDim.y;
  const int N = gx * gy * gridDim.z;
  const int L = (blockIdx.z * gy + blockIdx.y) * gx + blockIdx.x;
  const int per = N >> 3;
  const int lg = L < (per << 3) ? (L & 7) * per + (L >> 3) : L;
  const int t = lg / gx;
  return XcdBlock{lg - t * gx, t % gy, t / gy};
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Inclusive scan over the wave.
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
  const int lane = wave_lane();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// ---------------------------------------------------------------- block helpers (NT threads)
// Exclusive scan of v over the block; total = the block's sum.  s_tmp: NT / 64 ints, free again
// on return.
template <int NT>
__device__ __forceinline__ int block_scan_excl(int v, int* s_tmp, int& total) {
  const int wid = threadIdx.x >> 6;
  const int x = wave_scan_incl(v);
  if (wave_lane() == 63) s_tmp[wid] = x;
  __syncthreads();
  int pre = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    if (k < wid) pre += s_tmp[k];
    total += s_tmp[k];
  }
  __syncthreads();
  return pre + x - v;
}

// Deterministic block sum (wave sums, then the waves in order); the result is valid in every
// thread.  s_red: NT / 64 elements, free again on return.
template <int NT, typename T>
__device__ __forceinline__ T block_sum(T v, T* s_red) {
  v = wave_sum(v);
  if (wave_lane() == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) t += s_red[k];
  __syncthreads();
  return t;
}

// Ordered compaction.  A thread holds K consecutive elements of the block's sequence; returns the
// rank of its first kept element among the block's kept elements (its further kept elements
// follow it), and total = the block's kept count.  Wave ballots and popcounts below the lane, the
// per-wave counts through s_w[NT / 64], one barrier, the prefix over the waves.  s_w is read after
// that barrier only: a caller that loops (a running carry) puts a barrier before the next call.
template <int NT, int K>
__device__ __forceinline__ int block_rank(const bool (&keep)[K], int* s_w, int& total) {
  const unsigned long long below = (1ull << wave_lane()) - 1ull;
  const int wid = threadIdx.x >> 6;
  int pre = 0, wtot = 0;  // kept elements of the lanes before this one, of the wave
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const unsigned long long m = __ballot(keep[j]);
    pre += __popcll(m & below);
    wtot += __popcll(m);
  }
  if (wave_lane() == 0) s_w[wid] = wtot;
  __syncthreads();
  int wpre = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    if (w < wid) wpre += s_w[w];
    total += s_w[w];
  }
  return wpre + pre;
}
template <int NT>
__device__ __forceinline__ int block_rank(bool keep, int* s_w, int& total) {
  const bool k[1] = {keep};
  return block_rank<NT, 1>(k, s_w, total);
}

// ---------------------------------------------------------------- stereo point, map transform
// The camera-frame point of a pixel with disparity d16 (int16, 16 = one pixel), in float32 and in
// exactly this operation order (-ffp-contract=off): oracle.disparity_map and oracle.backproject
// (oracle/oracle.py) are the specification.  The camera's doubles are rounded to float32 first.
struct StereoCamF {
  float fxB, fx, fy, cx, cy;
};
inline StereoCamF stereo_cam(const double K[9], double baseline) {
  return StereoCamF{(float)(K[0] * baseline), (float)K[0], (float)K[4], (float)K[2], (float)K[5]};
}

// d = d16 / 16 with 0 and -1 replaced by (float)0.1; returns Z = fx B / d
__device__ __forceinline__ float stereo_depth(int d16, float fxB, float& d) {
  d = (float)d16 / 16.f;
  if (d == 0.0f) d = (float)0.1;
  if (d == -1.0f) d = (float)0.1;
  return fxB / d;
}

// (x, y): the keypoint's or the pixel's image position
__device__ __forceinline__ void stereo_xy(float x, float y, float Z, const StereoCamF& c, float& X, float& Y) {
  X = ((x - c.cx) / c.fx) * Z;
  Y = ((y - c.cy) / c.fy) * Z;
}

// r = (M (x, y, z, 1))[:3] for a row-major 4x4 M, in fp64 and in exactly this order (numpy's dgemm
// order is unpinned): oracle/map_ref.cpp ref_map_transform is the specification.
__device__ __forceinline__ void map_point(const double* M, double x, double y, double z, double r[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = ((M[4 * k] * x + M[4 * k + 1] * y) + M[4 * k + 2] * z) + M[4 * k + 3] * 1.0;
}
