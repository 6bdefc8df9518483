// Map accumulation for gfx950 — SURVEY.md §8f rank 4, the reference's per-frame map update:
//   stereo_slam.py:308-318   homogeneous = hstack(points3D, 1); pts = (cum @ homogeneous.T)[:3].T
//                            all_points_3D.append(pts); create_point_cloud(concat) (PointCloud2,
//                            x/y/z FLOAT32 fields, point_step 12)
//   mono_slam.py:144-164     points = np.dot(cum, vstack(points.T, 1))[:3].T,
//                            o3d PointCloud.voxel_down_sample(0.5), concatenated into the map,
//                            pc2.create_cloud_xyz32
//   gt_mapping.py:62-66      the same with the ground-truth pose
// Kernels:
//   k_map_xform   thread per point: map_point (fvo_device.h) in fp64, appended at the map's running
//                 count as f64 xyz and/or the PointCloud2 float32 xyz record; HBM-bound (12 B in,
//                 24+12 out).
//   k_chain       the pose chain stereo_slam.py:306 on the device (fvo_chain_poses): the map's
//                 placing poses without a host round trip.
//   voxel_down_sample (Open3D PointCloud::VoxelDownSample): min bound by block partials, voxel
//                 keys floor((p - (min - v/2)) / v) packed 3x21 bits, stable radix sort of
//                 (key, index) (hipcub), segment heads + exclusive scan, then one thread per
//                 voxel sums its points in the original order (= Open3D's AccumulatedPoint
//                 insertion order, so the fp64 sums are bit-identical) and divides by the count.
//                 Output ordered by voxel key (Open3D's unordered_map order is unspecified).
//                 The bounds, keys, sort and cell table are vx_grid.h's, shared with outlier.hip.
// Specification: oracle/map_ref.cpp.
#include "vx_grid.h"

namespace {

// the points of set j that are appended: n_points[j] clamped to [0, cap] (as fvo_gather_matches clamps
// its counts; a negative count is an empty set, not a step backwards in the map)
__device__ __forceinline__ int64_t set_count(const int32_t* __restrict__ npts, int j, int64_t cap) {
  return max((int64_t)0, min((int64_t)npts[j], cap));
}

__global__ __launch_bounds__(256) void k_map_xform(const float* __restrict__ pts, int stride, int64_t cap,
                                                   const int32_t* __restrict__ npts, int batch,
                                                   const double* __restrict__ T, const int32_t* __restrict__ count,
                                                   int64_t map_cap, double* __restrict__ out64,
                                                   float* __restrict__ out32) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n = set_count(npts, b, cap);
  if ((int64_t)blockIdx.x * 256 >= n) return;  // uniform: no point of set b in this block
  // the set's offset in the map: one wave sums the counts of the sets before it
  __shared__ int64_t s_base;
  if (threadIdx.x < 64) {
    int64_t part = 0;
    for (int j = threadIdx.x; j < b; j += 64) part += set_count(npts, j, cap);
    part = wave_sum(part);
    if (threadIdx.x == 0) s_base = count[0] + part;
  }
  __syncthreads();
  if (i >= n) return;
  const int64_t o = s_base + i;
  if (o >= map_cap) return;
  const float* p = pts + ((int64_t)b * cap + i) * stride;
  double r[3];
  map_point(T + 16 * b, p[0], p[1], p[2], r);
  if (out64) {
    out64[3 * o] = r[0];
    out64[3 * o + 1] = r[1];
    out64[3 * o + 2] = r[2];
  }
  if (out32) {
    out32[3 * o] = (float)r[0];
    out32[3 * o + 1] = (float)r[1];
    out32[3 * o + 2] = (float)r[2];
  }
}

__global__ void k_map_count(const int32_t* __restrict__ npts, int batch, int64_t cap, int32_t* __restrict__ count) {
  if (threadIdx.x != 0) return;
  int64_t t = count[0];
  for (int j = 0; j < batch; ++j) t += set_count(npts, j, cap);
  count[0] = (int32_t)min(t, (int64_t)INT32_MAX);
}

// Pose chains (fvo_chain_poses): 16 lanes per sequence, lane (i, j) holds cum[i][j]; per frame
// in order, c'_ij = ((c_i0 t_0j + c_i1 t_1j) + c_i2 t_2j) + c_i3 t_3j with the row of cum from the
// sequence's lanes (stereo_slam.py:306, np.dot(cumulative, T)), applied when the frame is posed
// (status >= 0: the reference chained it, :292).  Four sequences per wave; the serial chain is
// ~n dependent 4-term dot products, a few microseconds per batch.
__global__ __launch_bounds__(64) void k_chain(const double* __restrict__ T, const int32_t* __restrict__ status,
                                              const int32_t* __restrict__ npts, int n_seq, int n,
                                              double* __restrict__ cum, double* __restrict__ cum_out,
                                              int32_t* __restrict__ npts_out) {
  const int lane = threadIdx.x, sq = blockIdx.x * 4 + (lane >> 4), e = lane & 15, i = e >> 2, j = e & 3;
  const bool live = sq < n_seq;
  const int sqc = live ? sq : n_seq - 1;  // lanes past the last sequence mirror it and store nothing
  const int row = (lane & ~15) + 4 * i;
  double c = cum[(int64_t)sqc * 16 + e];
  for (int f = 0; f < n; ++f) {
    const int64_t k = (int64_t)sqc * n + f;
    const int st = status[k];
    const double* M = T + k * 16;
    const double t0 = M[j], t1 = M[4 + j], t2 = M[8 + j], t3 = M[12 + j];
    const double c0 = __shfl(c, row, 64), c1 = __shfl(c, row + 1, 64), c2 = __shfl(c, row + 2, 64),
                 c3 = __shfl(c, row + 3, 64);
    const double nc = ((c0 * t0 + c1 * t1) + c2 * t2) + c3 * t3;
    if (st >= 0) c = nc;
    if (live) cum_out[k * 16 + e] = c;
    if (live && npts_out && e == 0) npts_out[k] = st >= 0 ? npts[k] : 0;
  }
  if (live) cum[(int64_t)sq * 16 + e] = c;
}

__global__ __launch_bounds__(256) void k_vx_average(const double* __restrict__ p, const int32_t* __restrict__ sidx,
                                                    const int32_t* __restrict__ start,
                                                    const int32_t* __restrict__ n_out, double* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n_out[0]) return;
  const int32_t s = start[v], e = start[v + 1];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;  // AccumulatedPoint: point_ += points_[index], insertion order
  for (int32_t j = s; j < e; ++j) {
    const int64_t q = sidx[j];
    a0 = a0 + p[3 * q];
    a1 = a1 + p[3 * q + 1];
    a2 = a2 + p[3 * q + 2];
  }
  const double c = (double)(e - s);
  out[3 * v] = a0 / c;
  out[3 * v + 1] = a1 / c;
  out[3 * v + 2] = a2 / c;
}

}  // namespace

int map_transform_run(fvo_ctx* ctx, const float* pts, int stride, const int32_t* npts, int batch, int64_t cap,
                      const double* T, int32_t* count, int64_t map_cap, double* out64, float* out32, hipStream_t s) {
  // arguments and config were validated by capi.cpp
  dim3 grid((unsigned)((cap + 255) / 256), batch);
  FVO_TIMED(ctx, KN_MAP_XFORM, s, {
    hipLaunchKernelGGL(k_map_xform, grid, dim3(256), 0, s, pts, stride, cap, npts, batch, T, count, map_cap, out64,
                       out32);
  });
  FVO_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_map_count, dim3(1), dim3(64), 0, s, npts, batch, cap, count);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int chain_poses_run(fvo_ctx* ctx, const double* T, const int32_t* status, const int32_t* npts, int n_seq, int n,
                    double* cum, double* cum_out, int32_t* npts_out, hipStream_t s) {
  // arguments and config were validated by capi.cpp
  hipLaunchKernelGGL(k_chain, dim3((n_seq + 3) / 4), dim3(64), 0, s, T, status, npts, n_seq, n, cum, cum_out,
                     npts_out);
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}

int64_t voxel_workspace_bytes(int64_t n) {
  VxLayout L;
  if (n < 1 || vx_layout(n, L)) return -1;
  return (int64_t)L.total;
}

int voxel_run(fvo_ctx* ctx, const double* pts, int64_t n, double voxel, void* ws, double* out,
              int32_t* n_out, int32_t* status, hipStream_t s) {
  // arguments and config were validated by capi.cpp (the workspace size against voxel_workspace_bytes)
  VxLayout L;
  if (vx_layout(n, L)) return fvo_fail(ctx, "voxel_down_sample: workspace size query failed");  // a hipcub error
  char* w = (char*)ws;
  int32_t* st = status ? status : (int32_t*)(w + L.status);
  const unsigned g = (unsigned)((n + 255) / 256);
  FVO_HIP(ctx, hipMemsetAsync(st, 0, 4, s));
  FVO_TIMED(ctx, KN_VOXEL, s, {
    vx_sort_keys(pts, n, voxel, 0.5, w, L, st, s);
    vx_cell_table(n, w, L, n_out, s);
    hipLaunchKernelGGL(k_vx_average, dim3(g), dim3(256), 0, s, pts, (const int32_t*)(w + L.idx_b),
                       (const int32_t*)(w + L.start), n_out, out);
  });
  FVO_LAUNCH_CHECK(ctx);
  return 0;
}
