// Stereo rectification for gfx950: the undistort-rectify map, the fixed-point bilinear remap and the
// fused rectifying ingest (fvo_rectify_map / fvo_remap_u8 / fvo_rectify_gray).
//   map1, map2 = cv2.initUndistortRectifyMap(K, dist, R, newK, (W, H), cv2.CV_16SC2)
//   dst        = cv2.remap(src, map1, map2, cv2.INTER_LINEAR)          (BORDER_CONSTANT 0)
//   gray       = cv2.cvtColor(dst, cv2.COLOR_BGR2GRAY)                 (3 channels; mono8 is kept)
// in the conventions of ingest.hip / oracle/ingest_ref.cpp: fp64 map entry with the column term
// evaluated directly, iu = round_sat(u*32), (short)(iu >> 5), frac = (iv & 31)*32 + (iu & 31),
// 15-bit weights, (s + 2^14) >> 15, 14-bit BGR2GRAY.  No stripes and no cy shift (cv2.undistort's).
// ir = inverse(newK * R) comes from capi_rectify.cpp, which validated every argument.
// Specification: tests/rectify_ref.py.
//
// One kernel family.  A block produces a FVO_RECTIFY_TILE_W x FVO_RECTIFY_TILE_H output tile, a
// thread 4 consecutive pixels of a row.  The tile's map entries (computed, or read from the stored
// map) are reduced to their integer bounding box [x0, x1] x [y0, y1]; with bw = x1 - x0 + 2 and
// bh = y1 - y0 + 2 (the second taps) the box is staged in LDS when
//   ((bw*channels + 6) & ~3) * bh <= budget  (FVO_RECTIFY_LDS_BYTES)
// by dword loads, zeros outside the image, and sampled from there without per-tap tests;
// otherwise (strong roll, arbitrary user maps) the block gathers its taps from global memory as
// ingest.hip does.  The branch is block-uniform and both paths give the same bytes.
#include <climits>

#include "fvo_device.h"

namespace {

constexpr int kTW = FVO_RECTIFY_TILE_W, kTH = FVO_RECTIFY_TILE_H;
constexpr int kPix = 4, kThreads = 256;
static_assert((kTW / kPix) * kTH == kThreads && kTW % kPix == 0, "a thread owns 4 pixels of a 256-thread tile");
static_assert(FVO_RECTIFY_LDS_BYTES % 4 == 0 && FVO_RECTIFY_LDS_BYTES <= 40 * 1024,
              "four 256-thread blocks (four waves per SIMD) must fit the CU's 160 KiB");

__device__ __forceinline__ int round_sat(double v) {  // NaN (refused by the host layer) would give INT_MIN
  return v >= 2147483647.0 ? 2147483647 : (v > -2147483648.0 ? (int)rint(v) : (-2147483647 - 1));
}

// Map entry of output pixel (row, col): integer source (sx, sy) as stored in CV_16SC2 and the
// fractional index (iv & 31)*32 + (iu & 31).
__device__ __forceinline__ void map_entry(const RectifyLens& L, int row, int col, int& sx, int& sy, int& frac) {
  const double bx = row * L.ir[1] + L.ir[2], by = row * L.ir[4] + L.ir[5], bw = row * L.ir[7] + L.ir[8];
  const double _x = bx + col * L.ir[0], _y = by + col * L.ir[3], _w = bw + col * L.ir[6];
  const double w = 1. / _w, x = _x * w, y = _y * w;
  const double x2 = x * x, y2 = y * y;
  const double r2 = x2 + y2, _2xy = 2 * x * y;
  double kr = (1 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2);
  if (L.rational) kr = kr / (1 + ((L.k6 * r2 + L.k5) * r2 + L.k4) * r2);
  const double xd = (x * kr + L.p1 * _2xy + L.p2 * (r2 + 2 * x2) + 0.0 * r2 + 0.0 * r2 * r2);
  const double yd = (y * kr + L.p1 * (r2 + 2 * y2) + L.p2 * _2xy + 0.0 * r2 + 0.0 * r2 * r2);
  const int iu = round_sat((L.fx * xd + L.u0) * 32.0), iv = round_sat((L.fy * yd + L.v0) * 32.0);
  sx = (int16_t)(iu >> 5);
  sy = (int16_t)(iv >> 5);
  frac = (iv & 31) * 32 + (iu & 31);
}

__device__ __forceinline__ void tile_pos(int& row, int& c0) {
  row = blockIdx.y * kTH + threadIdx.x / (kTW / kPix);
  c0 = blockIdx.x * kTW + (threadIdx.x % (kTW / kPix)) * kPix;
}

// map1 [H][W][2] int16 (4-byte aligned: one dword per pixel), map2 [H][W] uint16
__global__ __launch_bounds__(kThreads) void k_rect_map(uint32_t* __restrict__ map1, uint16_t* __restrict__ map2, int W,
                                                       int H, RectifyLens L) {
  int row, c0;
  tile_pos(row, c0);
  if (row >= H) return;
#pragma unroll
  for (int q = 0; q < kPix; ++q) {
    const int col = c0 + q;
    if (col >= W) break;
    int sx, sy, fr;
    map_entry(L, row, col, sx, sy, fr);
    const int64_t p = (int64_t)row * W + col;
    map1[p] = (uint32_t)(sx & 0xffff) | ((uint32_t)(sy & 0xffff) << 16);
    map2[p] = (uint16_t)fr;
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// kCh source channels; kGray: one gray byte per pixel (BGR2GRAY of 3 channels, the value itself
// of 1), else kCh bytes per pixel; kFused: the map entry is computed, else read from map1 / map2.
template <int kCh, bool kGray, bool kFused>
__global__ __launch_bounds__(kThreads) void k_rect_sample(const uint8_t* __restrict__ src, int64_t sstride, int spitch,
                                                          const uint32_t* __restrict__ map1,
                                                          const uint16_t* __restrict__ map2,
                                                          uint8_t* __restrict__ dst, int64_t dstride, int dpitch,
                                                          int W, int H, int budget, RectifyLens L) {
  __shared__ uint32_t s_tile[FVO_RECTIFY_LDS_BYTES / 4];
  __shared__ int s_box[kThreads / 64][4];
  int row, c0;
  tile_pos(row, c0);
  const int b = blockIdx.z;
  const uint8_t* S = src + b * sstride;
  int sx[kPix], sy[kPix], fr[kPix];
  // -max instead of max: one reduction operator
  int mnx = INT_MAX, mny = INT_MAX, nmxx = INT_MAX, nmxy = INT_MAX;
#pragma unroll
  for (int q = 0; q < kPix; ++q) {
    const int col = c0 + q;
    sx[q] = sy[q] = fr[q] = 0;
    if (row < H && col < W) {
      if (kFused) {
        map_entry(L, row, col, sx[q], sy[q], fr[q]);
      } else {
        const int64_t p = (int64_t)row * W + col;
        const uint32_t m = map1[p];
        sx[q] = (int16_t)(m & 0xffff);
        sy[q] = (int16_t)(m >> 16);
        fr[q] = map2[p] & 1023;
      }
      mnx = min(mnx, sx[q]);
      mny = min(mny, sy[q]);
      nmxx = min(nmxx, -sx[q]);
      nmxy = min(nmxy, -sy[q]);
    }
  }
  mnx = wave_min(mnx);
  mny = wave_min(mny);
  nmxx = wave_min(nmxx);
  nmxy = wave_min(nmxy);
  if (wave_lane() == 0) {
    s_box[threadIdx.x >> 6][0] = mnx;
    s_box[threadIdx.x >> 6][1] = mny;
    s_box[threadIdx.x >> 6][2] = nmxx;
    s_box[threadIdx.x >> 6][3] = nmxy;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) {
    mnx = min(mnx, s_box[k][0]);
    mny = min(mny, s_box[k][1]);
    nmxx = min(nmxx, s_box[k][2]);
    nmxy = min(nmxy, s_box[k][3]);
  }
  // the block's first pixel is always inside the image, so the box is not empty; |values| <= 32768
  const int bw = -nmxx - mnx + 2, bh = -nmxy - mny + 2;
  const int lpitch = (bw * kCh + 6) & ~3;  // LDS row: bw pixels + up to 3 bytes of dword alignment
  const bool staged = (int64_t)lpitch * bh <= (int64_t)budget;
  const intptr_t base = (intptr_t)S + (int64_t)mnx * kCh;  // address of (x0, row 0); never dereferenced as such
  if (staged) {
    const int pd = lpitch >> 2, n = pd * bh;
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const int r = i / pd, k = i - r * pd;
      const int y = mny + r;
      uint32_t v = 0;
      if (y >= 0 && y < H) {
        const intptr_t lo = (intptr_t)S + (int64_t)y * spitch, hi = lo + (int64_t)W * kCh;  // the row's pixels
        const intptr_t g = ((base + (int64_t)y * spitch) & ~(intptr_t)3) + 4 * k;
        if (g >= lo && g + 4 <= hi) {
          v = *reinterpret_cast<const uint32_t*>(g);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (g + j >= lo && g + j < hi) v |= (uint32_t) * reinterpret_cast<const uint8_t*>(g + j) << (8 * j);
        }
      }
      s_tile[i] = v;
    }
    __syncthreads();
  }
  if (row >= H || c0 >= W) return;
  const uint8_t* T8 = reinterpret_cast<const uint8_t*>(s_tile);
  constexpr int kOut = kGray ? 1 : kCh;
  uint32_t packed[kOut];
#pragma unroll
  for (int k = 0; k < kOut; ++k) packed[k] = 0;
#pragma unroll
  for (int q = 0; q < kPix; ++q) {
    if (c0 + q >= W) break;
    const int tx = fr[q] & 31, ty = fr[q] >> 5;
    const int w0 = (32 - ty) * (32 - tx) * 32, w1 = (32 - ty) * tx * 32, w2 = ty * (32 - tx) * 32, w3 = ty * tx * 32;
    int ch[kCh];
#pragma unroll
    for (int k = 0; k < kCh; ++k) ch[k] = 0;
    if (staged) {
      const int r = sy[q] - mny;
      // byte offset of (x0, y) inside its LDS row = the low address bits of that pixel
      const int a0 = r * lpitch + (int)((base + (int64_t)sy[q] * spitch) & 3) + (sx[q] - mnx) * kCh;
      const int a1 = (r + 1) * lpitch + (int)((base + (int64_t)(sy[q] + 1) * spitch) & 3) + (sx[q] - mnx) * kCh;
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        int s = T8[a0 + k] * w0 + T8[a0 + kCh + k] * w1 + T8[a1 + k] * w2 + T8[a1 + kCh + k] * w3;
        s = (s + (1 << 14)) >> 15;
        ch[k] = s < 0 ? 0 : (s > 255 ? 255 : s);
      }
    } else if (!(sx[q] >= W || sx[q] + 1 < 0 || sy[q] >= H || sy[q] + 1 < 0)) {
      const bool xin0 = sx[q] >= 0, xin1 = sx[q] + 1 < W, yin0 = sy[q] >= 0, yin1 = sy[q] + 1 < H;
      const int64_t o0 = (int64_t)sy[q] * spitch + sx[q] * kCh, o1 = o0 + spitch;
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        const int v00 = (yin0 && xin0) ? S[o0 + k] : 0, v01 = (yin0 && xin1) ? S[o0 + kCh + k] : 0;
        const int v10 = (yin1 && xin0) ? S[o1 + k] : 0, v11 = (yin1 && xin1) ? S[o1 + kCh + k] : 0;
        int s = v00 * w0 + v01 * w1 + v10 * w2 + v11 * w3;
        s = (s + (1 << 14)) >> 15;
        ch[k] = s < 0 ? 0 : (s > 255 ? 255 : s);
      }
    }
    if (kGray) {
      const uint32_t g = kCh == 3 ? (uint32_t)((ch[0] * 1868 + ch[1 % kCh] * 9617 + ch[2 % kCh] * 4899 + (1 << 13)) >> 14)
                                  : (uint32_t)ch[0];
      packed[0] |= g << (8 * q);
    } else {
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        const int byte = q * kCh + k;
        packed[byte >> 2] |= (uint32_t)ch[k] << (8 * (byte & 3));
      }
    }
  }
  uint8_t* D = dst + b * dstride + (int64_t)row * dpitch + (int64_t)c0 * kOut;
  if (c0 + kPix <= W && (((uintptr_t)D) & 3) == 0) {
#pragma unroll
    for (int k = 0; k < kOut; ++k) reinterpret_cast<uint32_t*>(D)[k] = packed[k];
  } else {
    for (int j = 0; j < kPix * kOut && c0 * kOut + j < W * kOut; ++j) D[j] = (uint8_t)(packed[j >> 2] >> (8 * (j & 3)));
  }
}

dim3 tile_grid(int W, int H, int batch) { return dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, batch); }

}  // namespace

// The launches below are outside FVO_TIMED: the timing table (fvo_kernel_count) is frozen.

int rectify_map_run(fvo_ctx* ctx, const RectifyLens& L, int16_t* map1, uint16_t* map2, hipStream_t s) {
  const int W = ctx->cfg.width, H = ctx->cfg.height;
  hipLaunchKernelGGL(k_rect_map, tile_grid(W, H, 1), dim3(kThreads), 0, s, reinterpret_cast<uint32_t*>(map1), map2, W, H,
                     L);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int remap_run(fvo_ctx* ctx, const uint8_t* src, int batch, int64_t sstride, int spitch, int channels,
              const int16_t* map1, const uint16_t* map2, uint8_t* dst, int64_t dstride, int dpitch, hipStream_t s) {
  const int W = ctx->cfg.width, H = ctx->cfg.height;
  const uint32_t* m1 = reinterpret_cast<const uint32_t*>(map1);
  const RectifyLens none{};
  if (channels == 3)
    hipLaunchKernelGGL((k_rect_sample<3, false, false>), tile_grid(W, H, batch), dim3(kThreads), 0, s, src, sstride,
                       spitch, m1, map2, dst, dstride, dpitch, W, H, ctx->rectify_budget, none);
  else
    hipLaunchKernelGGL((k_rect_sample<1, false, false>), tile_grid(W, H, batch), dim3(kThreads), 0, s, src, sstride,
                       spitch, m1, map2, dst, dstride, dpitch, W, H, ctx->rectify_budget, none);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int rectify_gray_run(fvo_ctx* ctx, const uint8_t* src, int batch, int64_t sstride, int spitch, int channels,
                     const RectifyLens& L, uint8_t* gray, int64_t dstride, int dpitch, hipStream_t s) {
  const int W = ctx->cfg.width, H = ctx->cfg.height;
  if (channels == 3)
    hipLaunchKernelGGL((k_rect_sample<3, true, true>), tile_grid(W, H, batch), dim3(kThreads), 0, s, src, sstride,
                       spitch, nullptr, nullptr, gray, dstride, dpitch, W, H, ctx->rectify_budget, L);
  else
    hipLaunchKernelGGL((k_rect_sample<1, true, true>), tile_grid(W, H, batch), dim3(kThreads), 0, s, src, sstride,
                       spitch, nullptr, nullptr, gray, dstride, dpitch, W, H, ctx->rectify_budget, L);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
