// Index maps of the SGBM cost pass's LDS tile (k_sg_costvert, sgbm.hip): which cells a pixel-cost
// task computes and what it reads for them, where a pixel's BT words lie, and the run of pixel
// costs a lane box-sums.  Host and device: tests/test_sgbm_costmap_cpu.py walks them on the CPU.
//
// The tile of a block of CB columns is kCX = CB + 6 pixel-cost columns (the 7-wide box apron) x D
// disparities, u16, column-major ([i][d]).  Its sources are one BT record per staged pixel:
//   left  pixel k (k in [0, nl), nl <= kCX):      6 words (x-Sobel u, min, max, intensity u, min,
//                                                 max), each the pixel's value in both u16 halves
//   right pixel k (k in [1, nr), nr = nl + D - 1): the same 6 words as pairs (pixel k, pixel k - 1)
// A record is kSgRec consecutive words, so a task takes it with three 8-byte reads; 6 words is also
// the pitch that keeps a 32-lane read group on 64 distinct banks (bank = word mod 64 for 8-byte
// reads): the group's 32 tasks read one left record per 4 lanes (8 records, broadcast within the 4) and 32 consecutive
// right records, at words 6 n + {0, 1}, and 6 n = 6 m (mod 64) only for n = m (mod 32).
#pragma once

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

constexpr int kSgRec = 6;  // words of a pixel's BT record (three 8-byte pieces)

__host__ __device__ constexpr int sg_kcx(int CB) { return CB + 6; }                 // pixel-cost columns
__host__ __device__ constexpr int sg_nrc(int D, int CB) { return CB + 6 + D - 1; }  // right core pixels
// task slots: groups of 32 (8 columns x 4 runs of 8 disparities), D / 32 groups per 8 columns
__host__ __device__ constexpr int sg_nslot(int D, int CB) { return ((sg_kcx(CB) + 7) / 8) * (D / 32) * 32; }
__host__ __device__ constexpr int sg_ntask(int D, int CB, int NT) { return (sg_nslot(D, CB) + NT - 1) / NT; }

// word offset of word e of pixel k's record in a row's sU / sV
__host__ __device__ constexpr int sg_rec(int k, int e) { return k * kSgRec + e; }

// Task slot t (thread tid's m-th task is slot tid + NT m): 8 disparities d0 .. d0 + 7 of tile column
// i, as 4 packed pairs; pair h (d0 + 2h, d0 + 2h + 1) is the right record jr0 + 2 (3 - h).
//   kl   left record (the column's pixel, clamped to the image's columns [0, width1))
//   jr0  the lowest right record the task reads (pair 3); the highest is jr0 + 6
//   out  u16 offset of the 8 costs in the tile, -1 for a slot without cells
// Within a group of 32 slots w >> 2 steps the column by +1 and w & 3 the right record by -8.
struct SgTask {
  int kl, jr0, out;
};
__host__ __device__ inline SgTask sg_task(int t, int D, int CB, int c0, int width1, int minX1, int xl0) {
  const int NDB = D / 32;
  const int g = t >> 5, w = t & 31;
  const int i = (g / NDB) * 8 + (w >> 2), d0 = ((g % NDB) * 4 + (w & 3)) * 8;
  const int x1c = c0 - 3 + i < 0 ? 0 : (c0 - 3 + i > width1 - 1 ? width1 - 1 : c0 - 3 + i);
  SgTask k;
  k.kl = x1c + minX1 - xl0;
  k.jr0 = k.kl + (D - 1) - d0 - 6;
  k.out = (t < sg_nslot(D, CB) && i < sg_kcx(CB)) ? i * D + d0 : -1;
  return k;
}

// u16 offset in the tile of the DQ costs lane q of column col adds for box column t (0..6)
__host__ __device__ constexpr int sg_box_run(int D, int DQ, int col, int t, int q) { return (col + t) * D + q * DQ; }
