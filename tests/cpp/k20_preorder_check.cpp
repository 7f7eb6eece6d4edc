// Host check of csrc/k20_preorder.hpp: the 20-state pre-order walk's two A gathers, proven on an
// emulation of v_mfma_f64_4x4x4_4b_f64 by its lane map (kernels_clv_mfma.hip: with col = lane % 16
// and grp = lane / 16, A: i = col % 4, k = grp, of the block col / 4; B: site = col, k = grp;
// D: site = col, i = grp).  Random ASYMMETRIC 20 x 20 matrices of small integers (every product is
// exact) and 16-site vectors placed by the tile index; the MFMA-ready copy is built by
// pmat_to_mfma_kernel's formula.  For every lane the forward product must equal dense P c and the
// transposed one dense P^T t; two swapped-index variants must NOT (an asymmetric matrix tells them
// apart).  Also the LDS bound at 1 to 8 rate categories and the workspace size.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "k20_preorder.hpp"

using namespace rdamd;

// one four-block MFMA: d += A . B, every operand one double per lane
static void mfma_4x4x4_4b(const double (&a)[64], const double (&b)[64], double (&d)[64]) {
  double out[64];
  for (unsigned lane = 0; lane < 64; ++lane) {
    const unsigned col = lane % 16, i = lane / 16, block = col / 4;
    double acc = d[lane];
    for (unsigned k = 0; k < 4; ++k) {
      const double a_ik = a[16 * k + 4 * block + i];   // the lane of this block with col % 4 = i, grp = k
      const double b_ks = b[16 * k + col];             // the lane with site = col, grp = k
      acc += a_ik * b_ks;
    }
    out[lane] = acc;
  }
  for (unsigned lane = 0; lane < 64; ++lane) d[lane] = out[lane];
}

typedef unsigned (*Gather)(unsigned rg, unsigned ks, unsigned col, unsigned grp);

// the product as the kernel forms it: result[lane][rg] = operand rg of the lane's result vector
static void product(const std::vector<double> &copy, Gather gather, const std::vector<double> &tile, double (&res)[64][5]) {
  for (unsigned rg = 0; rg < kK20Groups; ++rg) {
    double d[64] = {0};
    for (unsigned ks = 0; ks < kK20Steps; ++ks) {
      double a[64], b[64];
      for (unsigned lane = 0; lane < 64; ++lane) {
        const unsigned at = gather(rg, ks, lane % 16, lane / 16);
        if (at >= copy.size()) { std::printf("gather out of range\n"); std::exit(1); }
        a[lane] = copy[at];
        b[lane] = tile[k20p_lane_operand(lane, ks)];
      }
      mfma_4x4x4_4b(a, b, d);
    }
    for (unsigned lane = 0; lane < 64; ++lane) res[lane][rg] = d[lane];
  }
}

static unsigned forward_swapped(unsigned rg, unsigned ks, unsigned col, unsigned grp) { return k20_a_forward(ks, rg, col, grp); }
static unsigned transposed_swapped(unsigned rg, unsigned ks, unsigned col, unsigned grp) { return k20_a_transposed(ks, rg, col, grp); }

// lanes whose five results differ from want[site][state]
static unsigned mismatches(const double (&res)[64][5], const double (&want)[16][20]) {
  unsigned bad = 0;
  for (unsigned lane = 0; lane < 64; ++lane)
    for (unsigned t = 0; t < 5; ++t)
      if (res[lane][t] != want[lane % 16][k20p_state_of(lane / 16, t)]) ++bad;
  return bad;
}

int main() {
  unsigned long checks = 0;
  int bad = 0;
  // the restated layout: a bijection of (site, state) onto the tile, each lane's operands where the kernel reads them
  {
    std::vector<int> seen(kK20TileDoubles, 0);
    for (unsigned c = 0; c < 16; ++c)
      for (unsigned s = 0; s < 20; ++s) {
        const unsigned at = k20p_tile_index(c, s);
        if (at >= kK20TileDoubles || seen[at]++) { std::printf("tile index (%u, %u)\n", c, s); ++bad; }
      }
    for (unsigned lane = 0; lane < 64; ++lane)
      for (unsigned t = 0; t < 5; ++t, ++checks)
        if (k20p_lane_operand(lane, t) != k20p_tile_index(lane % 16, k20p_state_of(lane / 16, t))) {
          std::printf("operand (%u, %u)\n", lane, t); ++bad;
        }
  }
  std::mt19937 rng(20);
  for (int trial = 0; trial < 50; ++trial) {
    double P[20][20], c[16][20];
    for (auto &row : P) for (double &x : row) x = (double)(rng() % 8u);
    P[3][11] = 7.0; P[11][3] = 1.0;   // never symmetric
    for (auto &row : c) for (double &x : row) x = (double)(rng() % 5u);
    // the MFMA-ready copy, element (rg, ks, k, i) = P[state_of(i, rg)][state_of(k, ks)]
    std::vector<double> copy(kK20CopyDoubles, -1.0);
    for (unsigned rg = 0; rg < 5; ++rg)
      for (unsigned ks = 0; ks < 5; ++ks)
        for (unsigned k = 0; k < 4; ++k)
          for (unsigned i = 0; i < 4; ++i) copy[k20_copy_index(rg, ks, k, i)] = P[k20p_state_of(i, rg)][k20p_state_of(k, ks)];
    std::vector<double> tile(kK20TileDoubles, -1.0);
    for (unsigned s = 0; s < 16; ++s)
      for (unsigned j = 0; j < 20; ++j) tile[k20p_tile_index(s, j)] = c[s][j];
    double pc[16][20], ptc[16][20];
    for (unsigned s = 0; s < 16; ++s)
      for (unsigned i = 0; i < 20; ++i) {
        pc[s][i] = ptc[s][i] = 0.0;
        for (unsigned j = 0; j < 20; ++j) { pc[s][i] += P[i][j] * c[s][j]; ptc[s][i] += P[j][i] * c[s][j]; }
      }
    double res[64][5];
    product(copy, k20_a_forward, tile, res);
    if (mismatches(res, pc)) { std::printf("trial %d: forward product wrong in %u entries\n", trial, mismatches(res, pc)); ++bad; }
    if (!mismatches(res, ptc)) { std::printf("trial %d: the matrix does not tell P from P^T\n", trial); ++bad; }
    product(copy, k20_a_transposed, tile, res);
    if (mismatches(res, ptc)) { std::printf("trial %d: transposed product wrong in %u entries\n", trial, mismatches(res, ptc)); ++bad; }
    if (!mismatches(res, pc)) { std::printf("trial %d: transposed product equals the forward one\n", trial); ++bad; }
    // the swapped variants must fail both ways
    product(copy, forward_swapped, tile, res);
    if (!mismatches(res, pc) || !mismatches(res, ptc)) { std::printf("trial %d: swapped forward gather passes\n", trial); ++bad; }
    product(copy, transposed_swapped, tile, res);
    if (!mismatches(res, ptc) || !mismatches(res, pc)) { std::printf("trial %d: swapped transposed gather passes\n", trial); ++bad; }
    checks += 6 * 64 * 5;
  }
  // LDS: the parts add up, grow with R and fit a CU; the workspace is whole tiles
  for (unsigned R = 1; R <= kK20MaxRates; ++R, ++checks) {
    const size_t lds = k20_preorder_lds_bytes(R);
    if (lds != R * (2 * 3200 + 2 * 2560) + 128 || lds > 160 * 1024 || (R > 1 && lds <= k20_preorder_lds_bytes(R - 1))) {
      std::printf("LDS at R = %u: %zu bytes\n", R, lds); ++bad;
    }
    if (k20_preorder_stage_bytes(R) % 16 || k20_preorder_exchange_bytes(R) % 16) { std::printf("LDS parts misaligned\n"); ++bad; }
  }
  if (k20_preorder_workspace_doubles(3, 4, 625) != (size_t)3 * 4 * 625 * 320 || k20_preorder_workspace_doubles(0, 8, 7) != 0) {
    std::printf("workspace size\n"); ++bad;
  }
  if (bad) { std::printf("k20 preorder FAILED: %d\n", bad); return 1; }
  std::printf("k20 preorder OK %lu\n", checks);
  return 0;
}
