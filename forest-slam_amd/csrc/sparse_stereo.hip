// Sparse stereo for gfx950: the stereo point of every left keypoint from a left-right ORB match on
// its own row band, refined to sub-pixel by a SAD search on the level-0 images, written as the
// per-keypoint record (X, Y, Z, d) of k_ba_stereo -- without a disparity map.  Specification:
// tests/sparse_stereo_ref.py (the rule is also in include/fvo.h); every float is float32 in the
// specification's order (-ffp-contract=off), the SADs are integer sums, so the result is bit-exact
// whatever order the pairs and the pixels are visited in.
//
// k_ss_init    the right keypoints' uniqueness keys to "no key": the call leaves nothing behind and
//              needs nothing from an earlier one (the workspace is the caller's).
// k_ss_match   k_bf_knn's shape: block = 4 waves serving the same 64 left keypoints (one descriptor
//              per lane, 8 VGPRs, its x, y, octave and row band beside it); the right set is staged
//              in LDS kChunk keypoints at a time, (x, y, octave) beside the descriptors, and wave w
//              takes the chunk's w-th 64-keypoint block.  All lanes of a wave take the same right
//              keypoint, so its descriptor and position are broadcast LDS reads.  The distance is
//              computed for every pair and masked by the geometric predicate; the minimum is a
//              packed key (hamming << 16 | right index).  The four waves' keys meet in LDS; the
//              row's key goes to the workspace and, when it is accepted, one atomicMin of
//              (hamming << 16 | left index) to the right keypoint's key.
// k_ss_refine  one wave per left keypoint, 4 per block.  The (2w+1)^2 left window and the
//              (2w+1) x (2w+1+2S) right strip are staged in LDS (byte loads: the window starts at
//              any byte of a row of any pitch), rows padded to whole dwords; a lane takes one
//              (shift, row) pair at a time: the strip's dwords at the shift come out of two
//              neighbours by v_alignbyte, v_sad_u8 sums four pixels per instruction, the row sums
//              meet by ds_add.  Lane 0 finds the first minimum, fits the parabola and writes the
//              record.  No block waits for another block.
// k_backproject_stereo  k_backproject with the point taken from the stereo record of the match's
//              query keypoint (kept iff its Z != 0), the same ordered compaction (block_rank).
#include "fvo_device.h"

namespace {

constexpr int kChunk = 256;  // right keypoints staged per trip (4 blocks of 64, one per wave)
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t hamming(const u32x4& a0, const u32x4& a1, const uint4* p) {
  const u32x4 b0 = *reinterpret_cast<const u32x4*>(p) ^ a0;
  const u32x4 b1 = *reinterpret_cast<const u32x4*>(p + 1) ^ a1;
  return (uint32_t)(__popc(b0.x) + __popc(b0.y) + __popc(b0.z) + __popc(b0.w) + __popc(b1.x) + __popc(b1.y) +
                    __popc(b1.z) + __popc(b1.w));
}

// the record's octave as an index into the level table, -1 when it is not an integer in [0, n)
// (NaN fails every comparison)
__device__ __forceinline__ int octave_of(float o, int n) {
  return (o >= 0.f && o < (float)n && o == floorf(o)) ? (int)o : -1;
}

__device__ __forceinline__ int clamp_count(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

__global__ __launch_bounds__(256) void k_ss_init(int cap, uint32_t* __restrict__ colkey) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < cap) colkey[(int64_t)blockIdx.y * cap + i] = kNoKey;
}

__global__ __launch_bounds__(256) void k_ss_match(const float* __restrict__ kpL, const int32_t* __restrict__ nL,
                                                  const uint8_t* __restrict__ descL, const float* __restrict__ kpR,
                                                  const int32_t* __restrict__ nR, const uint8_t* __restrict__ descR,
                                                  int cap, fvo_sparse_stereo_params P, SparseLevels lv,
                                                  uint32_t* __restrict__ rowkey, uint32_t* __restrict__ colkey) {
  __shared__ uint4 s_desc[kChunk * 2];  // the chunk's right descriptors (32 B each)
  __shared__ float s_x[kChunk], s_y[kChunk];
  __shared__ int s_o[kChunk];
  __shared__ uint32_t s_key[3][64];  // the keys of waves 1..3, for wave 0's minimum
  const int b = blockIdx.y;
  const int nr = clamp_count(nL[b], cap), nc = clamp_count(nR[b], cap);
  const int r0 = blockIdx.x * 64;
  if (r0 >= nr) return;  // uniform per block
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = r0 + lane;
  const bool rv = r < nr;
  u32x4 q0 = {0, 0, 0, 0}, q1 = q0;
  float xL = 0.f, yL = 0.f, band = 0.f;
  int oL = -1;
  if (rv) {
    const u32x4* p = reinterpret_cast<const u32x4*>(descL + ((int64_t)b * cap + r) * 32);
    q0 = p[0];
    q1 = p[1];
    const float* a = kpL + ((int64_t)b * cap + r) * FVO_KP_STRIDE;
    xL = a[0];
    yL = a[1];
    oL = octave_of(a[5], lv.n);
    if (oL >= 0) band = P.row_tol * lv.scale[oL];
  }
  uint32_t best = kNoKey;
  for (int c0 = 0; c0 < nc; c0 += kChunk) {
    const int ncols = min(kChunk, nc - c0);
    if (c0) __syncthreads();  // every wave is done with the previous chunk
    const uint4* cb = reinterpret_cast<const uint4*>(descR + ((int64_t)b * cap + c0) * 32);
    for (int i = tid; i < 2 * ncols; i += 256) s_desc[i] = cb[i];
    for (int i = tid; i < ncols; i += 256) {
      const float* a = kpR + ((int64_t)b * cap + c0 + i) * FVO_KP_STRIDE;
      s_x[i] = a[0];
      s_y[i] = a[1];
      s_o[i] = octave_of(a[5], lv.n);
    }
    __syncthreads();
    const int j0 = wave * 64;
    const int nj = min(64, ncols - j0);  // this wave's valid keypoints of the chunk (uniform; may be <= 0)
    for (int j = 0; j < nj; ++j) {
      const int jj = j0 + j;
      const uint32_t d = hamming(q0, q1, &s_desc[2 * jj]);
      const float yR = s_y[jj], d0 = xL - s_x[jj];
      const int oR = s_o[jj];
      const bool ok = oL >= 0 && oR >= 0 && fabsf(yR - yL) <= band && abs(oR - oL) <= P.max_octave_diff &&
                      d0 >= P.min_disparity && d0 <= P.max_disparity;
      best = min(best, ok ? (d << 16) | (uint32_t)(c0 + jj) : kNoKey);
    }
  }
  if (wave) s_key[wave - 1][lane] = best;
  __syncthreads();
  if (wave || !rv) return;
  best = min(min(best, s_key[0][lane]), min(s_key[1][lane], s_key[2][lane]));
  rowkey[(int64_t)b * cap + r] = best;
  if (P.unique && best != kNoKey && (int)(best >> 16) <= P.max_hamming)
    atomicMin(&colkey[(int64_t)b * cap + (best & 0xFFFFu)], (best & 0xFFFF0000u) | (uint32_t)r);
}

constexpr int kRefineWaves = 4;
constexpr int kMaxWin = 2 * kSparseMaxHalfWindow + 1;                 // 15 rows / columns
constexpr int kLeftDw = (kMaxWin + 3) / 4;                            // 4 dwords per left row
constexpr int kRightDw = (kMaxWin + 2 * kSparseMaxHalfSlide + 3) / 4 + 1;  // 8 dwords of strip + the alignbyte neighbour
constexpr int kMaxShifts = 2 * kSparseMaxHalfSlide + 1;

__global__ __launch_bounds__(kRefineWaves * 64) void k_ss_refine(
    const uint8_t* __restrict__ imgL, const uint8_t* __restrict__ imgR, int64_t image_stride, int pitch, int W, int H,
    const float* __restrict__ kpL, const int32_t* __restrict__ nL, const float* __restrict__ kpR, int cap,
    fvo_sparse_stereo_params P, StereoCamF cam, const uint32_t* __restrict__ rowkey,
    const uint32_t* __restrict__ colkey, float4* __restrict__ stereo, int4* __restrict__ info) {
  __shared__ uint32_t s_left[kRefineWaves][kMaxWin * kLeftDw];
  __shared__ uint32_t s_right[kRefineWaves][kMaxWin * kRightDw];
  __shared__ int s_sad[kRefineWaves][kMaxShifts];
  const int b = blockIdx.y;
  const int n = clamp_count(nL[b], cap);
  if (blockIdx.x * kRefineWaves >= n) return;  // uniform per block
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x * kRefineWaves + wave;
  const bool active = i < n;
  const int w = P.half_window, S = P.half_slide;
  const int nrow = 2 * w + 1, nshift = 2 * S + 1;
  // everything below is uniform over the wave
  int status = 1, j = -1, ham = -1, xl = 0, yl = 0, xr = 0;
  float xL = 0.f, yL = 0.f;
  if (active) {
    const uint32_t key = rowkey[(int64_t)b * cap + i];
    if (key != kNoKey && (int)(key >> 16) <= P.max_hamming) {
      j = (int)(key & 0xFFFFu);
      ham = (int)(key >> 16);
      status = 0;
      if (P.unique && (colkey[(int64_t)b * cap + j] & 0xFFFFu) != (uint32_t)i) status = 2;
    }
    if (status == 0) {
      const float* a = kpL + ((int64_t)b * cap + i) * FVO_KP_STRIDE;
      xL = a[0];
      yL = a[1];
      const float xR = kpR[((int64_t)b * cap + j) * FVO_KP_STRIDE];
      // the bounds in float32 (exact: whole numbers below 2^24), so that a coordinate no int holds
      // is refused before the conversion
      const float fxl = floorf(xL + 0.5f), fyl = floorf(yL + 0.5f), fxr = floorf(xR + 0.5f);
      const float fw = (float)w, fs = (float)(S + w), xmax = (float)(W - 1), ymax = (float)(H - 1);
      if (fxl - fw >= 0.f && fxl + fw <= xmax && fyl - fw >= 0.f && fyl + fw <= ymax && fxr - fs >= 0.f &&
          fxr + fs <= xmax) {
        xl = (int)fxl;
        yl = (int)fyl;
        xr = (int)fxr;
      } else {
        status = 3;
      }
    }
  }
  const bool refine = status == 0;
  if (lane < nshift) s_sad[wave][lane] = 0;
  if (refine) {
    const uint8_t* L = imgL + b * image_stride + (int64_t)(yl - w) * pitch + (xl - w);
    const uint8_t* R = imgR + b * image_stride + (int64_t)(yl - w) * pitch + (xr - S - w);
    uint8_t* sl = reinterpret_cast<uint8_t*>(s_left[wave]);
    uint8_t* sr = reinterpret_cast<uint8_t*>(s_right[wave]);
    const int strip = nrow + 2 * S;
    // the bytes past a row's end are zero in the left window; the strip's are masked where they are read
    for (int t = lane; t < nrow * (4 * kLeftDw); t += 64) {
      const int row = t / (4 * kLeftDw), col = t % (4 * kLeftDw);
      sl[t] = col < nrow ? L[(int64_t)row * pitch + col] : (uint8_t)0;
    }
    for (int t = lane; t < nrow * (4 * kRightDw); t += 64) {
      const int row = t / (4 * kRightDw), col = t % (4 * kRightDw);
      sr[t] = col < strip ? R[(int64_t)row * pitch + col] : (uint8_t)0;
    }
  }
  __syncthreads();
  if (refine) {
    const int ndw = (nrow + 3) >> 2;
    const uint32_t tail = 0xFFFFFFFFu >> (8 * (4 * ndw - nrow));  // the valid bytes of a row's last dword
    for (int t = lane; t < nshift * nrow; t += 64) {
      const int k = t / nrow, dy = t - k * nrow;  // shift k - S, row dy
      const uint32_t* lrow = &s_left[wave][dy * kLeftDw];
      const uint32_t* rrow = &s_right[wave][dy * kRightDw + (k >> 2)];
      const uint32_t sh = (uint32_t)(k & 3);
      uint32_t sad = 0;
      for (int m = 0; m < ndw; ++m) {
        uint32_t rr = __builtin_amdgcn_alignbyte(rrow[m + 1], rrow[m], sh);
        if (m == ndw - 1) rr &= tail;
        sad = __builtin_amdgcn_sad_u8(lrow[m], rr, sad);
      }
      atomicAdd(&s_sad[wave][k], (int)sad);
    }
  }
  __syncthreads();
  if (!active || lane) return;
  float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
  int ks = 0;
  if (refine) {
    int kb = 0, sb = s_sad[wave][0];
    for (int k = 1; k < nshift; ++k) {
      const int v = s_sad[wave][k];
      if (v < sb) {  // the first minimum: the smallest shift on ties
        sb = v;
        kb = k;
      }
    }
    ks = kb - S;
    if (kb == 0 || kb == nshift - 1) {
      status = 4;
    } else {
      const int d1 = s_sad[wave][kb - 1], d2 = sb, d3 = s_sad[wave][kb + 1];
      const float delta = (float)(d1 - d3) / (float)(2 * (d1 + d3 - 2 * d2));  // the denominator is >= 2
      const float xRs = (float)(xr + ks) + delta;
      const float d = xL - xRs;
      if (!(d >= P.min_disparity && d <= P.max_disparity)) {
        status = 5;
      } else {
        const float Z = cam.fxB / d;
        float X, Y;
        stereo_xy(xL, yL, Z, cam, X, Y);
        if (Z > (float)0.1 && Z < 1000.f) rec = make_float4(X, Y, Z, d);
        else status = 6;
      }
    }
  }
  stereo[(int64_t)b * cap + i] = rec;
  if (info) info[(int64_t)b * cap + i] = make_int4(j, ham, ks, status);
}

constexpr int kBackprojectThreads = 256;

__global__ __launch_bounds__(kBackprojectThreads) void k_backproject_stereo(
    const float4* __restrict__ stereo, const float* __restrict__ kp1, const int32_t* __restrict__ matches,
    const int32_t* __restrict__ nmatch, int cap, float* __restrict__ P3, float* __restrict__ p2,
    int32_t* __restrict__ npts) {
  const int b = blockIdx.x;
  const int n = clamp_count(nmatch[b], cap);
  __shared__ int s_w[16];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kBackprojectThreads) {
    const int i = base + threadIdx.x;
    bool keep = false;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    float u = 0, v = 0;
    if (i < n) {
      const int32_t* m = matches + ((int64_t)b * cap + i) * 3;
      r = stereo[(int64_t)b * cap + m[0]];
      const float* c = kp1 + ((int64_t)b * cap + m[1]) * FVO_KP_STRIDE;
      keep = r.z != 0.f;
      u = c[0];
      v = c[1];
    }
    int tot;
    const int rank = block_rank<kBackprojectThreads>(keep, s_w, tot);
    if (keep) {
      const int64_t o = (int64_t)b * cap + s_carry + rank;
      P3[o * 3] = r.x;
      P3[o * 3 + 1] = r.y;
      P3[o * 3 + 2] = r.z;
      p2[o * 2] = u;
      p2[o * 2 + 1] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) npts[b] = s_carry;
}

}  // namespace

// Arguments are validated by capi_stereo.cpp.  The launches are outside FVO_TIMED: the timing table
// is frozen.
int sparse_stereo_run(fvo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int64_t image_stride,
                      int pitch, const float* kpL, const int32_t* nL, const uint8_t* descL, const float* kpR,
                      const int32_t* nR, const uint8_t* descR, int cap, const fvo_sparse_stereo_params& p,
                      const SparseLevels& levels, const double* K, double baseline, void* ws, float* stereo,
                      int32_t* info, hipStream_t s) {
  static_assert(kMaxWin == 15 && kLeftDw == 4 && kRightDw == 9 && kMaxShifts == 17, "k_ss_refine's LDS layout");
  uint32_t* rowkey = static_cast<uint32_t*>(ws);
  uint32_t* colkey = rowkey + (int64_t)batch * cap;
  hipLaunchKernelGGL(k_ss_init, dim3((cap + 255) / 256, batch), dim3(256), 0, s, cap, colkey);
  hipLaunchKernelGGL(k_ss_match, dim3((cap + 63) / 64, batch), dim3(256), 0, s, kpL, nL, descL, kpR, nR, descR, cap,
                     p, levels, rowkey, colkey);
  hipLaunchKernelGGL(k_ss_refine, dim3((cap + kRefineWaves - 1) / kRefineWaves, batch), dim3(kRefineWaves * 64), 0,
                     s, left, right, image_stride, pitch, ctx->cfg.width, ctx->cfg.height, kpL, nL, kpR, cap, p,
                     stereo_cam(K, baseline), rowkey, colkey, reinterpret_cast<float4*>(stereo),
                     reinterpret_cast<int4*>(info));
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int backproject_stereo_run(fvo_ctx* ctx, const float* stereo, const float* kp1, const int32_t* matches,
                           const int32_t* nmatch, int batch, int cap, float* P3, float* p2, int32_t* npts,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_backproject_stereo, dim3(batch), dim3(kBackprojectThreads), 0, s,
                     reinterpret_cast<const float4*>(stereo), kp1, matches, nmatch, cap, P3, p2, npts);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
