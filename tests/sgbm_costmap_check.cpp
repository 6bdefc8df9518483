// Host walk of the SGBM cost tile's index maps (csrc/sgbm_costmap.h), built and run by
// tests/test_sgbm_costmap_cpu.py.  For every cost-pass instantiation the library dispatches
// (D, G lanes per column, CB columns per block) and blocks at the first, an interior and the last
// partial position of images of several widths:
//   - the pixel-cost tasks write every cell of the (CB + 6) x D tile exactly once
//   - every record a task reads lies inside its array and inside the part the BT phase writes
//   - the records are the pixels the cost needs (left x, right x - d)
//   - every 8-byte read and every 16-byte store is aligned
//   - a lane's box-sum runs stay inside the tile, and a column's lanes cover its D costs once
//   - the 8-byte reads of a 32-lane group fall on distinct banks (word mod 64) unless they are
//     the same address
// Prints "<n> checks, <m> failed".
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "../forest-slam_amd/csrc/sgbm_costmap.h"

static long g_checks = 0, g_failed = 0;
#define CHECK(c, ...)                                 \
  do {                                                \
    ++g_checks;                                       \
    if (!(c)) {                                       \
      if (++g_failed <= 20) {                         \
        std::printf("FAILED %s: ", #c);               \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

// the block's pixel ranges as k_sg_costvert derives them
struct Block {
  int xl0, nl, nr;
};
static Block block_of(int D, int CB, int c0, int width1, int minX1) {
  Block b;
  b.xl0 = std::max(c0 - 3, 0) + minX1;
  const int xl1 = std::min(c0 + CB + 2, width1 - 1) + minX1;
  b.nl = xl1 - b.xl0 + 1;
  b.nr = b.nl + D - 1;
  return b;
}

static void check_block(int D, int G, int CB, int c0, int width1, int minX1) {
  const int NT = G * CB, kCX = sg_kcx(CB), NRC = sg_nrc(D, CB), DQ = D / G;
  const int NTASK = sg_ntask(D, CB, NT);
  const Block b = block_of(D, CB, c0, width1, minX1);
  CHECK(b.nl >= 1 && b.nl <= kCX && b.nr <= NRC, "D %d G %d CB %d c0 %d w1 %d: nl %d nr %d", D, G, CB, c0, width1, b.nl, b.nr);
  std::vector<int> written(kCX * D, 0);
  for (int g0 = 0; g0 < NTASK * NT; g0 += 32) {
    // word addresses of the group's reads, per read instruction: the left pieces, 4 x the right pieces
    constexpr int NP = kSgRec / 2;
    std::set<int> addr[5 * NP];
    for (int w = 0; w < 32; ++w) {
      const int t = g0 + w;
      const SgTask k = sg_task(t, D, CB, c0, width1, minX1, b.xl0);
      if (k.out < 0) continue;
      const int i = k.out / D, d0 = k.out % D;
      CHECK(k.out % 8 == 0 && k.out + 8 <= kCX * D, "slot %d: out %d", t, k.out);
      CHECK((k.out * 2) % 16 == 0, "slot %d: 16-byte store at byte %d", t, k.out * 2);
      for (int j = 0; j < 8 && k.out + j < kCX * D; ++j) ++written[k.out + j];
      // left record: inside the array and the written part, and the column's (clamped) pixel
      CHECK(k.kl >= 0 && k.kl < b.nl && sg_rec(k.kl, kSgRec - 1) < kCX * kSgRec, "slot %d: kl %d nl %d", t, k.kl, b.nl);
      const int x = std::min(std::max(c0 - 3 + i, 0), width1 - 1) + minX1;
      CHECK(b.xl0 + k.kl == x, "slot %d: left pixel %d, column's %d", t, b.xl0 + k.kl, x);
      for (int e = 0; e < kSgRec / 2; ++e) {
        CHECK((sg_rec(k.kl, 2 * e) * 4) % 8 == 0, "slot %d: left piece %d at byte %d", t, e, sg_rec(k.kl, 2 * e) * 4);
        addr[e].insert(sg_rec(k.kl, 2 * e));
      }
      for (int h = 0; h < 4; ++h) {
        const int jr = k.jr0 + 2 * (3 - h);
        // pairs (pixel jr, pixel jr - 1): records 1 .. nr - 1 are written
        CHECK(jr >= 1 && jr < b.nr && sg_rec(jr, kSgRec - 1) < NRC * kSgRec, "slot %d pair %d: jr %d nr %d", t, h, jr, b.nr);
        // disparity index d0 + 2h at right pixel x - (d0 + 2h); record 0 is pixel x = xl0 - (D - 1)
        CHECK(jr == k.kl + (D - 1) - (d0 + 2 * h), "slot %d pair %d: jr %d", t, h, jr);
        for (int e = 0; e < kSgRec / 2; ++e) {
          CHECK((sg_rec(jr, 2 * e) * 4) % 8 == 0, "slot %d: right piece at byte %d", t, sg_rec(jr, 2 * e) * 4);
          addr[NP + NP * h + e].insert(sg_rec(jr, 2 * e));
        }
      }
    }
    for (int r = 0; r < 5 * NP; ++r) {
      std::set<int> banks;
      for (int a : addr[r]) {
        banks.insert(a % 64);
        banks.insert((a + 1) % 64);
      }
      CHECK(banks.size() == 2 * addr[r].size(), "group %d read %d: %zu addresses on %zu banks", g0 / 32, r, addr[r].size(),
            banks.size());
    }
  }
  int once = 0;
  for (int v : written) once += v == 1;
  CHECK(once == kCX * D, "D %d G %d CB %d c0 %d w1 %d: %d of %d cells written once", D, G, CB, c0, width1, once, kCX * D);
  // box sum: lane q of column col reads DQ costs of columns col .. col + 6
  for (int col = 0; col < CB; ++col)
    for (int t = 0; t < 7; ++t) {
      std::vector<int> seen(D, 0);
      for (int q = 0; q < G; ++q) {
        const int o = sg_box_run(D, DQ, col, t, q);
        CHECK(o >= 0 && o + DQ <= kCX * D, "box col %d t %d q %d: run at %d", col, t, q, o);
        CHECK(o / D == col + t && (o % D) + DQ <= D, "box col %d t %d q %d: run at %d leaves the column", col, t, q, o);
        CHECK((o * 2) % (DQ % 4 == 0 ? 8 : 4) == 0, "box col %d t %d q %d: byte %d", col, t, q, o * 2);
        for (int j = 0; j < DQ; ++j) ++seen[(o + j) % D];
      }
      CHECK(std::count(seen.begin(), seen.end(), 1) == D, "box col %d t %d: the lanes do not cover D once", col, t);
    }
}

int main() {
  const int shapes[5][2] = {{4, 32}, {4, 64}, {8, 16}, {8, 32}, {16, 32}};  // (G, CB); the L path runs (8, 32)
  const int Ds[3] = {64, 96, 128};
  for (int D : Ds)
    for (const auto& s : shapes) {
      const int G = s[0], CB = s[1];
      // widths (width1 = columns with a disparity range): one partial block (1, CB - 1), a block
      // boundary +-1, three blocks and a ragged fourth
      const int widths[5] = {1, CB - 1, CB + 1, 2 * CB, 3 * CB + 21};
      for (int w1 : widths) {
        const int nblk = (w1 + CB - 1) / CB;
        std::set<int> blocks = {0, nblk / 2, nblk - 1};
        for (int kb : blocks)
          for (int minX1 : {D, 0, D + 5}) check_block(D, G, CB, kb * CB, w1, minX1);
      }
    }
  std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
