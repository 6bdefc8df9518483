// Disparity speckle filter for gfx950 — cv2.filterSpeckles on CV_16SC1 (OpenCV calib3d), the
// post-filter StereoSGBM::compute applies after its 3x3 median when speckleWindowSize > 0:
//   filterSpeckles(disp, (minDisparity - 1) * 16, speckleWindowSize, 16 * speckleRange)
// Two 4-neighbours are connected when both differ from newVal and |int(p) - int(q)| <= maxDiff;
// every pixel of a connected component of at most maxSpeckleSize pixels becomes newVal.  A
// component's size is a fact about the image, so the result is independent of the schedule.
//
// Workspace: two int32 planes [batch][H*W] (8 B per pixel): label (parent pointers of a
// union-find forest, pixel indices inside the image, -1 for pixels of no region) and size.
// Kernels (one launch each, ordered by kernel boundaries only — no block waits for another):
//   k_spk_local  per 64x32 tile: connected components in LDS (row runs from one ballot per row,
//                vertical unions with LDS atomicMin); label[p] = the tile-local root's pixel
//                index, size[root] = the tile-local component's pixel count, 0 elsewhere.
//                Writes both planes whole, so the workspace needs no clearing between calls.
//   k_spk_seams  one thread per pixel pair across a tile seam: union of the two tile-local roots
//                in global memory, `old = atomicMin(&label[a], b)` and continue with (old, b).
//   k_spk_sum    every tile-local root adds its size to its global root with ONE integer atomic
//                (not one per pixel), and points itself at that root.
//   k_spk_apply  every pixel finds its root and stores newVal when the total is <= maxSpeckleSize.
// Termination and visibility: labels only ever decrease (label[i] <= i), so find
// takes at most i steps; a union iteration that does not finish lowers max(a, b) strictly.
// Inside k_spk_seams correctness rests on the values atomicMin returns alone: a stale parent read
// by find is a former parent of that node, and whoever replaced it went on to unite the two, so it
// is in the same final set.  k_spk_sum / k_spk_apply read what earlier kernels wrote.
#include "fvo_device.h"

namespace {

constexpr int kSpkTW = 64;  // tile width = one wave per row
constexpr int kSpkTH = 32;
constexpr int kSpkTP = kSpkTW * kSpkTH;
constexpr int kSpkNone = INT32_MIN;  // value of a pixel that belongs to no region (newVal / outside)

__device__ __forceinline__ bool spk_conn(int a, int b, int maxd) {
  return a != kSpkNone && b != kSpkNone && abs(a - b) <= maxd;
}

__device__ __forceinline__ int spk_load(const int16_t* img, int64_t off, int newval) {
  const int d = img[off];
  return d == newval ? kSpkNone : d;
}

// ---- LDS union-find (lab[i] <= i always; -1 entries are never visited)
__device__ __forceinline__ int lds_find(const volatile int* lab, int i) {
  int p;
  while ((p = lab[i]) != i) i = p;  // strictly decreasing: at most i steps
  return i;
}

__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
  for (;;) {  // every unfinished iteration lowers max(a, b): at most a + b iterations
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(256) void k_spk_local(const int16_t* __restrict__ disp, int64_t istride, int pitch, int H,
                                                   int W, int ntx, int newval, int maxd, int32_t* __restrict__ label,
                                                   int32_t* __restrict__ size) {
  __shared__ int s_val[kSpkTP], s_lab[kSpkTP], s_cnt[kSpkTP];
  const int b = blockIdx.y;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = tx * kSpkTW + lane, y0 = ty * kSpkTH;
  const int16_t* img = disp + (int64_t)b * istride;
  int start[8], len[8], root[8];
  // rows of this wave: one ballot per row gives every pixel its run's first lane and, for the
  // first pixel of a run, the run's length
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int r = wv * 8 + k, y = y0 + r, i = r * kSpkTW + lane;
    const int v = (x < W && y < H) ? spk_load(img, (int64_t)y * pitch + x, newval) : kSpkNone;
    const int vl = __shfl_up(v, 1, 64);
    const bool cl = lane > 0 && spk_conn(v, vl, maxd);
    const unsigned long long m = __ballot(cl);             // bit x: pixel x continues the run of x - 1
    const unsigned long long upto = (2ull << lane) - 1ull;  // bits 0..lane (lane 63: all)
    start[k] = 63 - __clzll((long long)(~m & upto));        // bit 0 of m is clear: never empty
    const unsigned long long above = ~m & ~upto;
    len[k] = (above ? __ffsll((long long)above) - 1 : kSpkTW) - lane;
    s_val[i] = v;
    s_lab[i] = v != kSpkNone ? r * kSpkTW + start[k] : -1;
    s_cnt[i] = 0;
  }
  __syncthreads();
  // vertical unions; a pair whose left neighbours are joined to it and to each other is implied
  // by the left pair's union (same rows, by induction down to a pair that is not skipped)
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int r = wv * 8 + k, i = r * kSpkTW + lane;
    if (r == 0) continue;
    const int v = s_val[i], u = s_val[i - kSpkTW];
    if (!spk_conn(v, u, maxd)) continue;
    if (lane > 0) {
      const int vl = s_val[i - 1], ul = s_val[i - kSpkTW - 1];
      if (spk_conn(v, vl, maxd) && spk_conn(u, ul, maxd) && spk_conn(vl, ul, maxd)) continue;
    }
    lds_union(s_lab, i, i - kSpkTW);
  }
  __syncthreads();
  // run heads: find the root, add the run's length to it
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int r = wv * 8 + k, i = r * kSpkTW + lane;
    root[k] = -1;
    if (s_val[i] != kSpkNone && start[k] == lane) {
      root[k] = lds_find(s_lab, i);
      atomicAdd(&s_cnt[root[k]], len[k]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (root[k] >= 0) s_lab[(wv * 8 + k) * kSpkTW + lane] = root[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int r = wv * 8 + k, y = y0 + r, i = r * kSpkTW + lane;
    if (x >= W || y >= H) continue;
    const int64_t g = (int64_t)b * H * W + (int64_t)y * W + x;
    if (s_val[i] == kSpkNone) {
      label[g] = -1;
      size[g] = 0;
      continue;
    }
    const int f = s_lab[r * kSpkTW + start[k]];  // the tile-local root
    label[g] = (y0 + (f >> 6)) * W + tx * kSpkTW + (f & 63);
    size[g] = f == i ? s_cnt[i] : 0;
  }
}

// ---- global union-find over the tile-local roots
__device__ __forceinline__ int spk_find_racing(const int32_t* lab, int i) {
  // relaxed device-scope loads: a value read here may be stale, i.e. a former parent of i —
  // still a member of i's final set; the caller's atomicMin decides
  int p;
  while ((p = __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != i) i = p;
  return i;
}

__device__ __forceinline__ int spk_find(const int32_t* lab, int i) {
  int p;
  while ((p = lab[i]) != i) i = p;
  return i;
}

__global__ __launch_bounds__(256) void k_spk_seams(const int16_t* __restrict__ disp, int64_t istride, int pitch, int H,
                                                   int W, int nvs, int nseam, int newval, int maxd, int32_t* label) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nseam) return;
  const int16_t* img = disp + (int64_t)b * istride;
  int32_t* lab = label + (int64_t)b * H * W;
  int xa, ya, xq, yq;      // the pair (a, q) across the seam
  int dx = 0, dy = 0;      // step to the previous pair along the seam (same tiles), or none
  if (idx < nvs * H) {     // vertical seam s: columns (s+1)*64 - 1 | (s+1)*64
    const int s = idx / H;
    ya = yq = idx - s * H;
    xa = (s + 1) * kSpkTW;
    xq = xa - 1;
    if (ya % kSpkTH) dy = -1;
  } else {                 // horizontal seam s: rows (s+1)*32 - 1 | (s+1)*32
    const int j = idx - nvs * H, s = j / W;
    xa = xq = j - s * W;
    ya = (s + 1) * kSpkTH;
    yq = ya - 1;
    if (xa % kSpkTW) dx = -1;
  }
  const int va = spk_load(img, (int64_t)ya * pitch + xa, newval), vq = spk_load(img, (int64_t)yq * pitch + xq, newval);
  if (!spk_conn(va, vq, maxd)) return;
  if (dx | dy) {  // implied by the previous pair of the same two tiles (as in k_spk_local)
    const int pa = spk_load(img, (int64_t)(ya + dy) * pitch + xa + dx, newval);
    const int pq = spk_load(img, (int64_t)(yq + dy) * pitch + xq + dx, newval);
    if (spk_conn(pa, pq, maxd) && spk_conn(va, pa, maxd) && spk_conn(vq, pq, maxd)) return;
  }
  int a = ya * W + xa, q = yq * W + xq;
  for (;;) {  // every unfinished iteration lowers max(a, q): bounded by a + q
    a = spk_find_racing(lab, a);
    q = spk_find_racing(lab, q);
    if (a == q) return;
    if (a < q) { const int t = a; a = q; q = t; }
    const int old = atomicMin(&lab[a], q);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(256) void k_spk_sum(int64_t hw, int32_t* label, int32_t* size) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  int32_t* lab = label + (int64_t)blockIdx.y * hw;
  int32_t* sz = size + (int64_t)blockIdx.y * hw;
  // > 0 exactly at tile-local roots; only global roots receive adds, and those skip theirs
  const int s = sz[p];
  if (s <= 0) return;
  // no root changes in this kernel; the pointer written below is either unseen by another
  // thread's find (it then walks the old chain) or seen (it jumps to the same root)
  const int g = spk_find(lab, (int)p);
  if (g == (int)p) return;
  atomicAdd(&sz[g], s);
  lab[p] = g;
}

__global__ __launch_bounds__(256) void k_spk_apply(int16_t* __restrict__ disp, int64_t istride, int pitch, int W,
                                                   int64_t hw, int newval, int maxsize,
                                                   const int32_t* __restrict__ label, const int32_t* __restrict__ size) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int32_t* lab = label + (int64_t)blockIdx.y * hw;
  const int l = lab[p];
  if (l < 0) return;
  const int g = spk_find(lab, l);
  if (size[(int64_t)blockIdx.y * hw + g] > maxsize) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  disp[(int64_t)blockIdx.y * istride + (int64_t)y * pitch + x] = (int16_t)newval;
}

}  // namespace

int speckle_run(fvo_ctx* ctx, int16_t* disp, int batch, int H, int W, int64_t istride, int pitch, int newval,
                int maxsize, int maxdiff, void* ws, hipStream_t s) {
  // arguments and config were validated by capi.cpp
  const int64_t hw = (int64_t)H * W;
  const int maxd = maxdiff > 65535 ? 65535 : maxdiff;  // int16 values differ by at most 65535
  const int ntx = (W + kSpkTW - 1) / kSpkTW, nty = (H + kSpkTH - 1) / kSpkTH;
  const int nvs = ntx - 1;
  const int64_t nseam = (int64_t)nvs * H + (int64_t)(nty - 1) * W;  // < 2 * hw / 32
  const unsigned gpx = (unsigned)((hw + 255) / 256);
  int32_t* label = (int32_t*)ws;
  int32_t* size = label + (int64_t)batch * hw;
  // (batch is grid.y: a batch beyond the grid limit fails the launch check)
  FVO_TIMED(ctx, KN_SPK_LOCAL, s, {
    hipLaunchKernelGGL(k_spk_local, dim3((unsigned)(ntx * nty), batch), dim3(256), 0, s, disp, istride, pitch, H, W,
                       ntx, newval, maxd, label, size);
  });
  FVO_LAUNCH_CHECK(ctx);
  if (nseam > 0) {
    FVO_TIMED(ctx, KN_SPK_SEAMS, s, {
      hipLaunchKernelGGL(k_spk_seams, dim3((unsigned)((nseam + 255) / 256), batch), dim3(256), 0, s, disp, istride,
                         pitch, H, W, nvs, (int)nseam, newval, maxd, label);
    });
    FVO_LAUNCH_CHECK(ctx);
  }
  FVO_TIMED(ctx, KN_SPK_SUM, s, { hipLaunchKernelGGL(k_spk_sum, dim3(gpx, batch), dim3(256), 0, s, hw, label, size); });
  FVO_LAUNCH_CHECK(ctx);
  FVO_TIMED(ctx, KN_SPK_APPLY, s, {
    hipLaunchKernelGGL(k_spk_apply, dim3(gpx, batch), dim3(256), 0, s, disp, istride, pitch, W, hw, newval, maxsize,
                       label, size);
  });
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
