// Dense stereo mapping for gfx950: a batch of disparity maps to a world-frame point cloud
// (fvo_dense_map_append), and cv2.reprojectImageTo3D (fvo_reproject_to_3d).
//
// fvo_dense_map_append.  Frame b samples the pixels (y, x), y = 0, step, 2 step, ... < H and x
// likewise, in row-major order; a sample's camera-frame point is the stereo point of fvo_device.h
// (stereo_slam.py:117-121, :265-289) at the integer pixel, kept iff d16 >= min_disp16 and
// z_min < Z < z_max; the kept point goes through map_point (fvo_device.h) and is appended at the
// map's running count, frames in batch order.  The order is deterministic: two passes over the
// disparities and a scan between them, no block waits for another.
//   k_dense_count  a frame's flat sample index space in blocks of 256 threads x 4 consecutive
//                  samples; the block's valid count (block_rank's total).
//   k_dense_scan   one block: exclusive offsets over [batch][blocks], the per-frame totals
//                  (n_added), the map's old count (the base, kept in the workspace) and its
//                  advanced count (clamped at INT32_MAX).
//   k_dense_emit   the same predicate again, rank in the block (block_rank), the point, placed
//                  at base + offset + rank when below map_cap: the block's points meet in
//                  LDS in rank order and leave as one contiguous run,
//                  lane after lane (stored straight from the sample loop, adjacent lanes were
//                  ~96 B apart: 0.51 ms per 64 frames at 960x600 against 0.32 staged).
// At step 1 with width % 4 == 0 and 8-byte aligned rows a thread's four samples are one 8-byte
// load (VEC); every other geometry takes scalar loads.  HBM-bound: 2 B per sample in each pass,
// 24 + 12 B per emitted point.
//
// fvo_reproject_to_3d.  One thread per pixel, OpenCV 4.x's Matx form in fp64:
//   h_k = (((0 + Q[k][0] x) + Q[k][1] y) + Q[k][2] d) + Q[k][3],  out_k = (float)(h_k / h_3)
// with d the raw disparity value.  handleMissingValues: a min pass first (wave minimum of an
// order-preserving integer key, one atomicMin per wave), then z = 10000 where
// |d - min| <= FLT_EPSILON.
// Compiled with -ffp-contract=off.
#include <cfloat>

#include "fvo_device.h"

namespace {

constexpr int kDenseThreads = 256;
static_assert(kDenseBlock == 4 * kDenseThreads, "a thread takes 4 consecutive samples");

struct DenseGrid {
  int W, nx, step, pitch, nb;  // nx: samples per row, nb: blocks per frame
  uint32_t ns;                 // samples per frame
  int64_t stride;
};

// The block's frame and its four samples per thread: disparities, pixel coordinates, the kept
// flags (both passes evaluate exactly this).  Returns false (uniform) when frame b contributes
// nothing.
struct DenseSamples {
  int x[4], y[4];
  float Z[4];
  bool keep[4];
};

template <bool VEC>
__device__ __forceinline__ void dense_samples(const int16_t* __restrict__ disp, const DenseGrid& g, int b, int k,
                                              float fxB, int min_disp16, float z_min, float z_max, DenseSamples& s) {
  const int16_t* img = disp + (int64_t)b * g.stride;
  const uint32_t i0 = ((uint32_t)k * kDenseThreads + threadIdx.x) * 4u;
  int d16[4];
  bool in[4];
  if (VEC) {  // step 1, W % 4 == 0: i0 .. i0 + 3 lie in one row, all inside the frame or none
    const int y = (int)(i0 / (uint32_t)g.W), x = (int)(i0 - (uint32_t)y * (uint32_t)g.W);
    int2 v = make_int2(0, 0);
    const bool ok = i0 < g.ns;
    if (ok) v = *reinterpret_cast<const int2*>(img + (int64_t)y * g.pitch + x);
    d16[0] = (int16_t)(v.x & 0xFFFF);
    d16[1] = v.x >> 16;
    d16[2] = (int16_t)(v.y & 0xFFFF);
    d16[3] = v.y >> 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      in[j] = ok;
      s.x[j] = x + j;
      s.y[j] = y;
    }
  } else {
    int sy = (int)(i0 / (uint32_t)g.nx), sx = (int)(i0 - (uint32_t)sy * (uint32_t)g.nx);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      in[j] = i0 + (uint32_t)j < g.ns;
      s.x[j] = sx * g.step;
      s.y[j] = sy * g.step;
      d16[j] = in[j] ? (int)img[(int64_t)s.y[j] * g.pitch + s.x[j]] : 0;
      if (++sx == g.nx) {
        sx = 0;
        ++sy;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float d;
    s.Z[j] = stereo_depth(d16[j], fxB, d);
    s.keep[j] = in[j] && d16[j] >= min_disp16 && s.Z[j] > z_min && s.Z[j] < z_max;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kDenseThreads) void k_dense_count(const int16_t* __restrict__ disp, DenseGrid g,
                                                               float fxB, int min_disp16, float z_min, float z_max,
                                                               const int32_t* __restrict__ frame_keep,
                                                               int32_t* __restrict__ cnt) {
  const int blk = blockIdx.x, b = blk / g.nb, k = blk - b * g.nb;
  if (frame_keep && frame_keep[b] == 0) {  // uniform
    if (threadIdx.x == 0) cnt[blk] = 0;
    return;
  }
  DenseSamples s;
  dense_samples<VEC>(disp, g, b, k, fxB, min_disp16, z_min, z_max, s);
  __shared__ int s_w[kDenseThreads / 64];
  int total;
  block_rank<kDenseThreads>(s.keep, s_w, total);
  if (threadIdx.x == 0) cnt[blk] = total;
}

// One block.  Exclusive scan of cnt[n] into off[n] (tiles of 1024 threads x 4 entries, a carry
// between tiles), then the per-frame totals, the base and the advanced map count.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_dense_scan(const int32_t* __restrict__ cnt, int64_t* __restrict__ off,
                                                             int n, int nb, int batch, int32_t* __restrict__ n_added,
                                                             int64_t* __restrict__ base,
                                                             int32_t* __restrict__ map_count) {
  __shared__ int64_t s_w[kScanThreads / 64];
  __shared__ int64_t s_carry;
  const int tid = threadIdx.x, wave = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int64_t tile = 0; tile < n; tile += 4 * kScanThreads) {
    const int64_t i = tile + 4 * (int64_t)tid;
    int32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? cnt[i + j] : 0;
    const int64_t own = ((int64_t)v[0] + v[1]) + ((int64_t)v[2] + v[3]);
    const int64_t inc = wave_scan_incl(own);
    if (wave_lane() == 63) s_w[wave] = inc;
    __syncthreads();
    int64_t wpre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      if (w < wave) wpre += s_w[w];
      tot += s_w[w];
    }
    int64_t e = s_carry + wpre + (inc - own);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < n) off[i + j] = e;
      e += v[j];
    }
    __syncthreads();
    if (tid == 0) s_carry += tot;
    __syncthreads();  // (also orders this tile's off[] stores before the reads below)
  }
  const int64_t total = s_carry;
  if (n_added)
    for (int b = tid; b < batch; b += kScanThreads) {
      const int64_t end = b + 1 < batch ? off[(int64_t)(b + 1) * nb] : total;
      n_added[b] = (int32_t)(end - off[(int64_t)b * nb]);
    }
  if (tid == 0) {
    const int64_t old = map_count[0];
    base[0] = old;
    map_count[0] = (int32_t)min(old + total, (int64_t)INT32_MAX);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kDenseThreads) void k_dense_emit(const int16_t* __restrict__ disp, DenseGrid g,
                                                              StereoCamF cam, int min_disp16, float z_min, float z_max,
                                                              const int32_t* __restrict__ frame_keep,
                                                              const double* __restrict__ T,
                                                              const int32_t* __restrict__ cnt,
                                                              const int64_t* __restrict__ off,
                                                              const int64_t* __restrict__ base, int64_t map_cap,
                                                              double* __restrict__ out64, float* __restrict__ out32) {
  const int blk = blockIdx.x, b = blk / g.nb, k = blk - b * g.nb;
  // uniform exits: a frame that contributes nothing, an empty block, a block past the map's end
  if (frame_keep && frame_keep[b] == 0) return;
  if (cnt[blk] == 0) return;
  const int64_t o0 = base[0] + off[blk];
  if (o0 >= map_cap) return;
  DenseSamples s;
  dense_samples<VEC>(disp, g, b, k, cam.fxB, min_disp16, z_min, z_max, s);
  __shared__ int s_w[kDenseThreads / 64];
  __shared__ double s_pt[3 * kDenseBlock];  // the block's points in rank order (24 KB)
  int total;
  int r = block_rank<kDenseThreads>(s.keep, s_w, total);
  const double* M = T + 16 * (int64_t)b;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!s.keep[j]) continue;
    float X, Y;
    stereo_xy((float)s.x[j], (float)s.y[j], s.Z[j], cam, X, Y);
    map_point(M, X, Y, s.Z[j], &s_pt[3 * r]);
    ++r;
  }
  __syncthreads();
  // the block's points are one contiguous run of the map: stored lane after lane (adjacent lanes
  // of the loop above are ~4 points = 96 B apart), up to the map's end
  const int64_t room = map_cap - o0;
  const int ne = 3 * (int)(room < (int64_t)total ? room : (int64_t)total);
  double* o64 = out64 ? out64 + 3 * o0 : nullptr;
  float* o32 = out32 ? out32 + 3 * o0 : nullptr;
  for (int e = threadIdx.x; e < ne; e += kDenseThreads) {
    const double v = s_pt[e];
    if (o64) o64[e] = v;
    if (o32) o32[e] = (float)v;
  }
}

// ------------------------------------------------------------------ reprojectImageTo3D
// Order-preserving keys: a < b <=> key(a) < key(b) as unsigned integers.
__device__ __forceinline__ uint32_t rp_key(int16_t v) { return (uint32_t)((int)v + 32768); }
__device__ __forceinline__ uint32_t rp_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
template <typename TIn>
__device__ __forceinline__ double rp_unkey(uint32_t k);
template <>
__device__ __forceinline__ double rp_unkey<int16_t>(uint32_t k) {
  return (double)((int)k - 32768);
}
template <>
__device__ __forceinline__ double rp_unkey<float>(uint32_t k) {
  return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

struct RpGeom {
  int W, pitch, nb;  // nb: blocks per image
  uint32_t hw;
  int64_t stride;
};

constexpr int kRpMinPer = 4;  // pixels per thread of the min pass, 256 apart

template <typename TIn>
__global__ __launch_bounds__(256) void k_rp_min(const TIn* __restrict__ disp, RpGeom g, uint32_t* __restrict__ key) {
  const int blk = blockIdx.x, b = blk / g.nb, k = blk - b * g.nb;
  const TIn* img = disp + (int64_t)b * g.stride;
  uint32_t m = 0xFFFFFFFFu;
#pragma unroll
  for (int j = 0; j < kRpMinPer; ++j) {
    const uint32_t p = ((uint32_t)k * kRpMinPer + j) * 256u + threadIdx.x;
    if (p < g.hw) {
      const uint32_t y = p / (uint32_t)g.W, x = p - y * (uint32_t)g.W;
      m = min(m, rp_key(img[(int64_t)y * g.pitch + x]));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if (wave_lane() == 0 && m != 0xFFFFFFFFu) atomicMin(key + b, m);
}

struct RpQ {
  double q[16];
};

template <typename TIn>
__global__ __launch_bounds__(256) void k_rp_main(const TIn* __restrict__ disp, RpGeom g, RpQ Q, int handle,
                                                 const uint32_t* __restrict__ key, float* __restrict__ out) {
  const int blk = blockIdx.x, b = blk / g.nb, k = blk - b * g.nb;
  const uint32_t p = (uint32_t)k * 256u + threadIdx.x;
  if (p >= g.hw) return;
  const uint32_t yi = p / (uint32_t)g.W, xi = p - yi * (uint32_t)g.W;
  const double d = (double)disp[(int64_t)b * g.stride + (int64_t)yi * g.pitch + xi];
  const double x = (double)xi, y = (double)yi;
  double h[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    h[r] = (((0.0 + Q.q[4 * r] * x) + Q.q[4 * r + 1] * y) + Q.q[4 * r + 2] * d) + Q.q[4 * r + 3] * 1.0;
  float* o = out + ((int64_t)b * g.hw + p) * 3;
  o[0] = (float)(h[0] / h[3]);
  o[1] = (float)(h[1] / h[3]);
  float z = (float)(h[2] / h[3]);
  if (handle && fabs(d - rp_unkey<TIn>(key[b])) <= (double)FLT_EPSILON) z = 10000.f;
  o[2] = z;
}

template <typename TIn>
void rp_launch(const TIn* disp, const RpGeom& g0, int batch, const RpQ& Q, int handle, uint32_t* key, float* out,
               hipStream_t s) {
  RpGeom g = g0;
  if (handle) {
    g.nb = (int)(((int64_t)g.hw + 256 * kRpMinPer - 1) / (256 * kRpMinPer));
    hipLaunchKernelGGL(k_rp_min<TIn>, dim3((unsigned)(g.nb * batch)), dim3(256), 0, s, disp, g, key);
  }
  g.nb = (int)(((int64_t)g.hw + 255) / 256);
  hipLaunchKernelGGL(k_rp_main<TIn>, dim3((unsigned)(g.nb * batch)), dim3(256), 0, s, disp, g, Q, handle, key, out);
}

}  // namespace

int dense_append_run(fvo_ctx* ctx, const int16_t* disp, int batch, int H, int W, int64_t image_stride, int pitch,
                     const double* K, double baseline, int step, int min_disp16, float z_min, float z_max,
                     const int32_t* frame_keep, const double* T, int32_t* count, int64_t map_cap, double* out64,
                     float* out32, int32_t* n_added, void* ws, hipStream_t s) {
  // arguments were validated by capi.cpp (batch * blocks fits an int32, the workspace holds it)
  DenseGrid g;
  g.W = W;
  g.nx = (W - 1) / step + 1;
  g.step = step;
  g.pitch = pitch;
  g.nb = (int)dense_frame_blocks(H, W, step);
  g.ns = (uint32_t)dense_frame_samples(H, W, step);
  g.stride = image_stride;
  const int n = g.nb * batch;
  const StereoCamF cam = stereo_cam(K, baseline);
  int64_t* base = (int64_t*)ws;
  int64_t* off = base + 1;
  int32_t* cnt = (int32_t*)(off + n);
  // one 8-byte load per thread: every sample row starts 8-byte aligned and holds whole groups of 4
  const bool vec = step == 1 && W % 4 == 0 && pitch % 4 == 0 && image_stride % 4 == 0 &&
                   (reinterpret_cast<uintptr_t>(disp) & 7) == 0;
  const dim3 grid((unsigned)n), blk(kDenseThreads);
  if (vec)
    hipLaunchKernelGGL(k_dense_count<true>, grid, blk, 0, s, disp, g, cam.fxB, min_disp16, z_min, z_max, frame_keep,
                       cnt);
  else
    hipLaunchKernelGGL(k_dense_count<false>, grid, blk, 0, s, disp, g, cam.fxB, min_disp16, z_min, z_max, frame_keep,
                       cnt);
  FVO_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_dense_scan, dim3(1), dim3(kScanThreads), 0, s, cnt, off, n, g.nb, batch, n_added, base, count);
  FVO_LAUNCH_CHECK(ctx);
  if (vec)
    hipLaunchKernelGGL(k_dense_emit<true>, grid, blk, 0, s, disp, g, cam, min_disp16, z_min, z_max, frame_keep, T, cnt,
                       off, base, map_cap, out64, out32);
  else
    hipLaunchKernelGGL(k_dense_emit<false>, grid, blk, 0, s, disp, g, cam, min_disp16, z_min, z_max, frame_keep, T,
                       cnt, off, base, map_cap, out64, out32);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int reproject_run(fvo_ctx* ctx, const void* disp, int is_f32, int batch, int H, int W, int64_t image_stride,
                  int pitch, const double* Q, int handle_missing, uint32_t* min_key, float* out, hipStream_t s) {
  // arguments were validated by capi.cpp
  RpGeom g;
  g.W = W;
  g.pitch = pitch;
  g.nb = 0;
  g.hw = (uint32_t)((int64_t)H * W);
  g.stride = image_stride;
  RpQ q;
  for (int i = 0; i < 16; ++i) q.q[i] = Q[i];
  if (handle_missing) FVO_HIP(ctx, hipMemsetAsync(min_key, 0xFF, 4 * (size_t)batch, s));
  if (is_f32)
    rp_launch(static_cast<const float*>(disp), g, batch, q, handle_missing, min_key, out, s);
  else
    rp_launch(static_cast<const int16_t*>(disp), g, batch, q, handle_missing, min_key, out, s);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
