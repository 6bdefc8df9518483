// SGBM's derived parameters: host arithmetic on fvo_config, no HIP constructs.  Shared by
// sgbm.hip (launch shapes, kernel argument) and capi.cpp (check_sgbm_config).
#pragma once

#include <algorithm>
#include <cmath>

#include "../../include/fvo.h"

// (unnamed namespace: SgParams is a kernel argument of sgbm.hip's file-local kernels)
namespace {

struct SgParams {
  int W, H, D, minD, minX1, width1, P1, P2, ftzero, disp12, ss, ov, nstripes;
  int HG;   // row groups of 16
  int HG4;  // row groups of 4 (volume layout)
};

// Schedules and launch shapes (fvo_config, validated by capi.cpp's check_sgbm_config; every variant
// is bit-identical and parity-tested), sgbm_mode:
//   FVO_SGBM_CLASSIC  one cost pass, one row pass running both sweeps, with sgbm_lanes lanes per
//                     column (4, 8 or 16) and sgbm_cols columns per block (4: 32/64; 8: 16/32; 16: 32)
//   FVO_SGBM_LPATH    the L path in the cost pass, handed from column block to column block: one V
//                     read per pair fewer (<= 300 MB/pair) but slower -- DESIGN.md §4.2 r5
int sg_lanes(const fvo_config& c) { return c.sgbm_lanes > 0 ? c.sgbm_lanes : 8; }
int sg_cols(const fvo_config& c) { return c.sgbm_cols > 0 ? c.sgbm_cols : (sg_lanes(c) == 4 ? 64 : 32); }

SgParams make_params(const fvo_config& c) {
  SgParams p;
  p.W = c.width;
  p.H = c.height;
  p.D = c.num_disparities;
  p.minD = c.min_disparity;
  int maxD = p.minD + p.D;
  p.minX1 = maxD > 0 ? maxD : 0;
  int maxX1 = c.width + (p.minD < 0 ? p.minD : 0);
  p.width1 = maxX1 - p.minX1;
  p.P1 = c.P1 > 0 ? c.P1 : 2;
  p.P2 = std::max(c.P2 > 0 ? c.P2 : 5, p.P1 + 1);
  p.ftzero = std::max(c.pre_filter_cap, 15) | 1;
  p.disp12 = c.disp12_max_diff > 0 ? c.disp12_max_diff : 1;
  p.nstripes = c.sgbm_stripes;
  p.ss = (int)std::ceil(c.height / (double)p.nstripes);
  p.ov = (c.block_size / 2 + 1) + (int)std::ceil(0.1 * p.ss);
  p.HG = (c.height + 15) / 16;
  p.HG4 = (c.height + 3) / 4;
  return p;
}

constexpr int kSgCB = 32;  // columns per cost block of the L-path schedule
int sg_nk(const SgParams& p) { return (p.width1 + kSgCB - 1) / kSgCB; }

}  // namespace
