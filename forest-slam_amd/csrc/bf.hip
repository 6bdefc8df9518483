// Cross-checked brute-force Hamming matcher for gfx950 — replaces
// cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True).match(d0, d1)
// (ros_ws/src/stereo_slam.py:85, :234, :242).
//
// One pass over the distance matrix gives both directions' nearest neighbours (r6; r1-r5 ran
// the two directions as separate grids, every popcount twice).  The minima are packed keys
// (distance << 16 | index): min over keys = smallest distance, then the smallest index, which
// is batchDistance(K=1)'s first-index-wins rule in either direction, independent of the order
// the distances are visited in.
// k_bf_pass: block = 4 waves x 64 query rows (one row descriptor per lane, 8 VGPRs) x a chunk of
//   kChunk train columns staged in LDS.  A wave walks each 64-column block of the chunk
//   diagonally: at step s lane i takes column (i + s) mod 64, so the 64 lanes touch 64 different
//   columns and a column's running minimum over the wave's rows travels with it -- one DPP
//   wave_rol:1 per step (folded into the v_min_u32) hands each lane the accumulator of the column
//   it takes next.  The row minimum stays in the lane.  Per distance: 8 xor + 8 v_bcnt, two key
//   builds, two mins -- no cross-lane argmin reduction, no second pass.  Column minima of the
//   block's 4 waves meet in LDS (ds_min), then one global atomicMin per column; row minima one
//   global atomicMin per row (blocks of other column chunks).
// k_bf_finish: mutual-nearest check + ordered compaction (ascending queryIdx); resets the key
//   arrays for the next call.
//
// k-nearest neighbours and Lowe's ratio test (cv2 knnMatch(q, t, k) + m.distance < r * n.distance;
// specification: tests/bf_knn_ref.py).  Stateless: no atomics, nothing kept between calls.
// k_bf_knn<K>: block = 4 waves serving the same 64 query rows (one row descriptor per lane, 8 VGPRs);
//   the train set is staged in LDS kChunk columns at a time and wave w takes the chunk's w-th
//   64-column block.  All lanes of a wave take the same column, so the descriptor is one broadcast
//   ds_read_b128 pair and no lane rotation is needed.  Each lane keeps its K smallest keys
//   (distance << 16 | train index) in ascending order with a branch-free min/max insertion; keys
//   are unique, so the K smallest are the same whatever order the columns are visited in.  The
//   four waves' lists meet in LDS and wave 0 merges them with the same insertion.  Columns past
//   the set's end never enter a list; empty slots stay kNoKey.
// k_bf_ratio: the ratio decision in f64 (one multiply, one strict compare), optionally the
//   reverse nearest-neighbour check (k_bf_knn<1> with query and train swapped), and k_bf_finish's
//   ordered compaction.
#include <type_traits>

#include "fvo_device.h"

namespace {

constexpr int kChunk = 256;  // train columns per block (4 column blocks of 64)
constexpr int kRows = 256;   // query rows per block (4 waves)
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

// popcount accumulated in one instruction (v_bcnt_u32_b32 d, x, acc): the compiler otherwise
// turns a chain of popcount + add into separate counts and v_add3s
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Hamming distance of a row descriptor (a0, a1) and a column descriptor at p (LDS, 32 B: loaded
// as two whole 16-B vectors -- ds_read_b128 -- before the scalar popcounts take them apart)
__device__ __forceinline__ uint32_t hamming(const u32x4& a0, const u32x4& a1, const uint4* p) {
  const u32x4 b0 = *reinterpret_cast<const u32x4*>(p) ^ a0;
  const u32x4 b1 = *reinterpret_cast<const u32x4*>(p + 1) ^ a1;
  uint32_t d = bcnt_acc(b0.x, 0u);
  d = bcnt_acc(b0.y, d);
  d = bcnt_acc(b0.z, d);
  d = bcnt_acc(b0.w, d);
  d = bcnt_acc(b1.x, d);
  d = bcnt_acc(b1.y, d);
  d = bcnt_acc(b1.z, d);
  return bcnt_acc(b1.w, d);
}

// DPP wave_rol:1 -- lane i receives lane i + 1's value (lane 63 lane 0's)
__device__ __forceinline__ uint32_t wave_rol1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x134, 0xF, 0xF, false);
}

__global__ __launch_bounds__(kRows) void k_bf_pass(const uint8_t* __restrict__ query, const int32_t* __restrict__ nq,
                                                   const uint8_t* __restrict__ train, const int32_t* __restrict__ nt,
                                                   int cap, uint32_t* __restrict__ rowkey,
                                                   uint32_t* __restrict__ colkey) {
  __shared__ uint4 s_desc[kChunk * 2];  // the chunk's train descriptors (32 B each)
  __shared__ uint32_t s_col[kChunk];    // column minima of the block's rows
  const int b = blockIdx.z;
  int nr = nq[b], nc = nt[b];
  nr = nr < 0 ? 0 : (nr > cap ? cap : nr);
  nc = nc < 0 ? 0 : (nc > cap ? cap : nc);
  const int r0 = blockIdx.x * kRows, c0 = blockIdx.y * kChunk;
  if (r0 >= nr || c0 >= nc) return;  // uniform per block
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncols = min(kChunk, nc - c0);
  const uint4* cb = reinterpret_cast<const uint4*>(train + ((int64_t)b * cap + c0) * 32);
  for (int i = tid; i < 2 * kChunk; i += kRows) s_desc[i] = i < 2 * ncols ? cb[i] : make_uint4(0, 0, 0, 0);
  for (int i = tid; i < kChunk; i += kRows) s_col[i] = kNoKey;
  const int r = r0 + tid;
  const bool rv = r < nr;
  u32x4 q0 = {0, 0, 0, 0}, q1 = q0;
  if (rv) {
    const u32x4* p = reinterpret_cast<const u32x4*>(query + ((int64_t)b * cap + r) * 32);
    q0 = p[0];
    q1 = p[1];
  }
  // a row past the set's end contributes kNoKey to every column minimum: (d << 16) | ~0 = ~0
  const uint32_t rbits = rv ? (uint32_t)r : kNoKey;
  uint32_t rkey = kNoKey;
  __syncthreads();
  // one 64-column block (PART: the set's last, partial one -- its columns past the end never win a row)
  auto walk = [&](int cbk, auto part_t) {
    constexpr bool PART = decltype(part_t)::value;
    const uint32_t nv = (uint32_t)(ncols - cbk * 64);  // valid columns of the block
    uint32_t j = (uint32_t)lane;  // this lane's column in the block at step s: (lane + s) mod 64
    uint32_t acc = kNoKey, rk = kNoKey;
#pragma unroll 8
    for (int s = 0; s < 64; ++s) {
      const uint32_t d = hamming(q0, q1, &s_desc[(cbk * 64 + j) * 2]);
      uint32_t kr = (d << 16) | j;  // the block's column offset is added after the walk
      if constexpr (PART) kr = j < nv ? kr : kNoKey;
      rk = min(rk, kr);
      // the accumulator of column (lane + s) comes from lane + 1, which held it at step s - 1
      // (at s = 0 every lane's is still kNoKey, so the rotation is harmless there)
      acc = min(wave_rol1(acc), (d << 16) | rbits);
      j = (j + 1) & 63;
    }
    if (rk != kNoKey) rkey = min(rkey, rk | (uint32_t)(c0 + cbk * 64));
    // after step 63 lane i holds column i - 1's minimum: one more rotation puts column i on lane i
    atomicMin(&s_col[cbk * 64 + lane], wave_rol1(acc));
  };
  const int nfull = ncols >> 6;
  for (int cbk = 0; cbk < nfull; ++cbk) walk(cbk, std::false_type{});
  if (ncols & 63) walk(nfull, std::true_type{});
  if (rv && rkey != kNoKey) atomicMin(&rowkey[(int64_t)b * cap + r], rkey);
  __syncthreads();
  for (int i = tid; i < ncols; i += kRows)
    if (s_col[i] != kNoKey) atomicMin(&colkey[(int64_t)b * cap + c0 + i], s_col[i]);
}

constexpr int kFinishThreads = 256;  // k_bf_finish, k_bf_ratio

__global__ __launch_bounds__(kFinishThreads) void k_bf_finish(const int32_t* __restrict__ nq,
                                                              const int32_t* __restrict__ nt, int cap,
                                                              uint32_t* __restrict__ rowkey,
                                                              uint32_t* __restrict__ colkey,
                                                              int32_t* __restrict__ matches,
                                                              int32_t* __restrict__ nmatch) {
  const int b = blockIdx.x;
  int n0 = nq[b], n1 = nt[b];
  n0 = n0 < 0 ? 0 : (n0 > cap ? cap : n0);
  n1 = n1 < 0 ? 0 : (n1 > cap ? cap : n1);
  const int r0 = n0, r1 = n1;  // the key entries the pass may have lowered
  if (n1 == 0) n0 = 0;
  __shared__ int s_w[16];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  uint32_t* rk = rowkey + (int64_t)b * cap;
  uint32_t* ck = colkey + (int64_t)b * cap;
  for (int base = 0; base < n0; base += kFinishThreads) {
    int q = base + threadIdx.x;
    uint32_t key = kNoKey;
    bool keep = false;
    if (q < n0) {
      key = rk[q];
      keep = key != kNoKey && (ck[key & 0xFFFFu] & 0xFFFFu) == (uint32_t)q;
    }
    int tot;
    const int rank = block_rank<kFinishThreads>(keep, s_w, tot);
    if (keep) {
      int32_t* o = matches + ((int64_t)b * cap + s_carry + rank) * 3;
      o[0] = q;
      o[1] = (int32_t)(key & 0xFFFFu);
      o[2] = (int32_t)(key >> 16);
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) nmatch[b] = s_carry;
  // every read of this set's keys is behind the loop's last barrier: reset them for the next call
  for (int i = threadIdx.x; i < r0; i += kFinishThreads) rk[i] = kNoKey;
  for (int i = threadIdx.x; i < r1; i += kFinishThreads) ck[i] = kNoKey;
}

// Keeps the K smallest keys seen, ascending: key falls through the slots, each keeping the smaller.
template <int K>
__device__ __forceinline__ void knn_insert(uint32_t (&k)[K], uint32_t key) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const uint32_t t = max(k[i], key);
    k[i] = min(k[i], key);
    key = t;
  }
}

// RAW: out = u32 key planes [K][plane], entry b * cap + row.  Otherwise out = int32
// [batch][cap][kout][2] rows of (trainIdx, distance), (-1, -1) for the empty slots.
template <int K, bool RAW>
__global__ __launch_bounds__(256) void k_bf_knn(const uint8_t* __restrict__ query, const int32_t* __restrict__ nq,
                                                const uint8_t* __restrict__ train, const int32_t* __restrict__ nt,
                                                int cap, int kout, int64_t plane, void* __restrict__ out) {
  __shared__ uint4 s_desc[kChunk * 2];    // the chunk's train descriptors (32 B each)
  __shared__ uint32_t s_list[3][K][64];   // the lists of waves 1..3, for wave 0's merge
  const int b = blockIdx.y;
  int nr = nq[b], nc = nt[b];
  nr = nr < 0 ? 0 : (nr > cap ? cap : nr);
  nc = nc < 0 ? 0 : (nc > cap ? cap : nc);
  const int r0 = blockIdx.x * 64;
  if (r0 >= nr) return;  // uniform per block; rows >= n_query are not written
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform: the column loop's bounds are scalar
  const int r = r0 + lane;
  const bool rv = r < nr;
  u32x4 q0 = {0, 0, 0, 0}, q1 = q0;
  if (rv) {
    const u32x4* p = reinterpret_cast<const u32x4*>(query + ((int64_t)b * cap + r) * 32);
    q0 = p[0];
    q1 = p[1];
  }
  uint32_t k[K];
#pragma unroll
  for (int i = 0; i < K; ++i) k[i] = kNoKey;
  for (int c0 = 0; c0 < nc; c0 += kChunk) {
    const int ncols = min(kChunk, nc - c0);
    const uint4* cb = reinterpret_cast<const uint4*>(train + ((int64_t)b * cap + c0) * 32);
    if (c0) __syncthreads();  // every wave is done with the previous chunk
    for (int i = tid; i < 2 * ncols; i += 256) s_desc[i] = cb[i];
    __syncthreads();
    // this wave's 64-column block of the chunk, valid columns only (uniform per wave)
    const int nj = min(64, ncols - wave * 64);
    const uint4* col = &s_desc[wave * 128];
    const uint32_t base = (uint32_t)(c0 + wave * 64);
    auto take = [&](int j) { knn_insert<K>(k, (hamming(q0, q1, col + 2 * j) << 16) | (base + (uint32_t)j)); };
    int j = 0;
    for (; j + 8 <= nj; j += 8) {  // 8 columns per trip: their LDS reads are in flight together
#pragma unroll
      for (int u = 0; u < 8; ++u) take(j + u);
    }
    for (; j < nj; ++j) take(j);
  }
  if (wave) {
#pragma unroll
    for (int i = 0; i < K; ++i) s_list[wave - 1][i][lane] = k[i];
  }
  __syncthreads();
  if (wave || !rv) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int i = 0; i < K; ++i) knn_insert<K>(k, s_list[w][i][lane]);  // kNoKey changes nothing
  const int64_t row = (int64_t)b * cap + r;
  if constexpr (RAW) {
    uint32_t* o = static_cast<uint32_t*>(out) + row;
#pragma unroll
    for (int i = 0; i < K; ++i) o[i * plane] = k[i];
  } else {
    int2* o = static_cast<int2*>(out) + row * kout;
#pragma unroll
    for (int i = 0; i < K; ++i)
      if (i < kout) o[i] = k[i] == kNoKey ? make_int2(-1, -1) : make_int2((int)(k[i] & 0xFFFFu), (int)(k[i] >> 16));
  }
}

// fwd0 / fwd1: the rows' smallest and second-smallest forward keys; rev (mutual only): the
// columns' smallest reverse keys (distance << 16 | query index).
__global__ __launch_bounds__(kFinishThreads) void k_bf_ratio(const int32_t* __restrict__ nq, int cap,
                                                             const uint32_t* __restrict__ fwd0,
                                                             const uint32_t* __restrict__ fwd1,
                                                             const uint32_t* __restrict__ rev, double ratio,
                                                             int32_t* __restrict__ matches,
                                                             int32_t* __restrict__ nmatch) {
  const int b = blockIdx.x;
  int n0 = nq[b];
  n0 = n0 < 0 ? 0 : (n0 > cap ? cap : n0);
  __shared__ int s_w[16];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const int64_t off = (int64_t)b * cap;
  for (int base = 0; base < n0; base += kFinishThreads) {
    const int q = base + threadIdx.x;
    uint32_t key = kNoKey;
    bool keep = false;
    if (q < n0) {
      key = fwd0[off + q];
      const uint32_t k2 = fwd1[off + q];
      // a row with fewer than two neighbours is dropped; d1 < ratio * d2 as Python computes it
      keep = k2 != kNoKey && (double)(key >> 16) < ratio * (double)(k2 >> 16);
      if (keep && rev) keep = (rev[off + (key & 0xFFFFu)] & 0xFFFFu) == (uint32_t)q;
    }
    int tot;
    const int rank = block_rank<kFinishThreads>(keep, s_w, tot);
    if (keep) {
      int32_t* o = matches + (off + s_carry + rank) * 3;
      o[0] = q;
      o[1] = (int32_t)(key & 0xFFFFu);
      o[2] = (int32_t)(key >> 16);
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) nmatch[b] = s_carry;
}

template <int K, bool RAW>
void knn_launch(const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch, int cap, int kout,
                int64_t plane, void* out, hipStream_t s) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bf_knn<K, RAW>), dim3((cap + 63) / 64, batch), dim3(256), 0, s, q, nq, t, nt,
                     cap, kout, plane, out);
}

}  // namespace

int bf_init(fvo_ctx* ctx) {
  // arguments and config were validated by capi.cpp (check_bf_config: 16-bit indices in the keys)
  const int64_t n = (int64_t)ctx->cfg.max_batch * ctx->kp_cap;
  int rc;
  if ((rc = fvo_alloc(ctx, &ctx->bf_rowkey, n)) || (rc = fvo_alloc(ctx, &ctx->bf_colkey, n))) return rc;
  // the key arrays start (and are left by every k_bf_finish) at "no key"
  FVO_HIP(ctx, hipMemset(ctx->bf_rowkey, 0xFF, n * sizeof(uint32_t)));
  FVO_HIP(ctx, hipMemset(ctx->bf_colkey, 0xFF, n * sizeof(uint32_t)));
  // k_bf_knn's key planes for the ratio test (forward K = 2, reverse K = 1): every entry read is
  // written by the same call, so they need no initial value
  return fvo_alloc(ctx, &ctx->bf_knn, 3 * n);
}

int bf_run(fvo_ctx* ctx, const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch, int cap,
           int32_t* matches, int32_t* nmatch, hipStream_t s) {
  // arguments and config were validated by capi.cpp
  const dim3 grid((cap + kRows - 1) / kRows, (cap + kChunk - 1) / kChunk, batch);
  FVO_TIMED(ctx, KN_BF_ARGMIN, s, hipLaunchKernelGGL(k_bf_pass, grid, dim3(kRows), 0, s, q, nq, t, nt, cap,
                                                     ctx->bf_rowkey, ctx->bf_colkey));
  FVO_TIMED(ctx, KN_BF_FINISH, s,
            hipLaunchKernelGGL(k_bf_finish, dim3(batch), dim3(kFinishThreads), 0, s, nq, nt, cap, ctx->bf_rowkey,
                               ctx->bf_colkey, matches, nmatch));
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int bf_knn_run(fvo_ctx* ctx, const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch,
               int cap, int k, int32_t* knn, hipStream_t s) {
  // arguments and config were validated by capi.cpp
  FVO_TIMED(ctx, KN_BF_KNN, s, {
    if (k == 1) knn_launch<1, false>(q, nq, t, nt, batch, cap, k, 0, knn, s);
    else if (k == 2) knn_launch<2, false>(q, nq, t, nt, batch, cap, k, 0, knn, s);
    else if (k <= 4) knn_launch<4, false>(q, nq, t, nt, batch, cap, k, 0, knn, s);
    else knn_launch<8, false>(q, nq, t, nt, batch, cap, k, 0, knn, s);
  });
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int bf_ratio_run(fvo_ctx* ctx, const uint8_t* q, const int32_t* nq, const uint8_t* t, const int32_t* nt, int batch,
                 int cap, double ratio, int mutual, int32_t* matches, int32_t* nmatch, hipStream_t s) {
  // arguments and config were validated by capi.cpp
  const int64_t plane = (int64_t)ctx->cfg.max_batch * ctx->kp_cap;
  uint32_t* fwd = ctx->bf_knn;
  uint32_t* rev = mutual ? ctx->bf_knn + 2 * plane : nullptr;
  FVO_TIMED(ctx, KN_BF_KNN, s, {
    knn_launch<2, true>(q, nq, t, nt, batch, cap, 2, plane, fwd, s);
    if (mutual) knn_launch<1, true>(t, nt, q, nq, batch, cap, 1, plane, rev, s);
  });
  FVO_TIMED(ctx, KN_BF_RATIO, s,
            hipLaunchKernelGGL(k_bf_ratio, dim3(batch), dim3(kFinishThreads), 0, s, nq, cap, fwd, fwd + plane, rev,
                               ratio, matches, nmatch));
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
