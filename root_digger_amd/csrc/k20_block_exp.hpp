// The 20-state device block exponential's index arithmetic (kernels_block_exp.hip): which entry of a
// dense row-major 20 x 20 matrix a lane holds as the A operand and as the B operand / accumulator of
// v_mfma_f64_16x16x4_f64, the LDS layout of the one re-deal a squaring needs, and the record of one
// problem as the host hands it over.  Plain arithmetic over plain numbers -- no HIP -- so that
// tests/cpp/k20_blockexp_check.cpp can emulate the matrix cores' lane map on the host and prove the
// left product, the Taylor step, the re-deal and the squaring before any GPU run.
//
// Lanes: col = lane % 16, grp = lane / 16.  One v_mfma_f64_16x16x4_f64 takes from lane (col, grp)
//   A[row = col][k = grp]  and  B[k = grp][n = col]
// and leaves in result register q of that lane  D[row = grp + 4 q][n = col],  q = 0..3.
//
// 20 pads to 32: two row tiles (rt) and two column tiles (ct) of 16, of which tile 1 holds the states
// 16..19 in its first four rows / columns and nothing else.  The k-steps of a product are not the
// consecutive quadruples but the five residue sets {grp + 4 r : grp = 0..3}, r = 0..4, which cover
// 0..19 exactly.  With that choice the accumulator of one product IS the B operand of the next:
// register q of row tile 0 holds row grp + 4 q, the B operand of k-step r = q, and register 0 of row
// tile 1 holds row 16 + grp, the B operand of k-step r = 4.  So a matrix in B layout is
// b[ct][r] = M[grp + 4 r][16 ct + col]  (ten doubles a lane; zero where 16 ct + col >= 20), a left
// product leaves its result in B layout, and the Taylor recurrences, written as left products by the
// constant matrices X and E, move nothing between lanes.  A matrix in A layout is
// a[rt][r] = M[16 rt + col][grp + 4 r]  (zero where 16 rt + col >= 20): the B layout of its transpose.
//
// A product is 2 x 2 tiles x 5 k-steps = 20 MFMAs of 16 x 16 x 4 = 20 480 multiply-adds for the 8 000
// of a 20 x 20 x 20 product: 39 % of the issue slots do work (tile (0, 0) all of them, tiles (0, 1)
// and (1, 0) a quarter, tile (1, 1) a sixteenth).
#pragma once

#include <cstddef>

namespace rdamd {

constexpr unsigned kBx20States = 20, kBx20Steps = 5, kBx20Tiles = 2;
constexpr unsigned kBx20Absent = 0xffffffffu;   // a padding position: the operand is 0, nothing is stored
constexpr int kBx20TaylorTerms = 18;            // pgrad::kBlockTaylorTerms (param_gradient.hpp asserts it)

// B layout / accumulator: dense index (row * 20 + column) of b[ct][r] in `lane`, or kBx20Absent
constexpr unsigned k20x_b_index(unsigned lane, unsigned ct, unsigned r) {
  const unsigned col = lane & 15u, grp = lane >> 4, n = 16u * ct + col;
  return n < kBx20States ? (grp + 4u * r) * kBx20States + n : kBx20Absent;
}
// A layout: dense index of a[rt][r] in `lane`, or kBx20Absent
constexpr unsigned k20x_a_index(unsigned lane, unsigned rt, unsigned r) {
  const unsigned col = lane & 15u, grp = lane >> 4, row = 16u * rt + col;
  return row < kBx20States ? row * kBx20States + grp + 4u * r : kBx20Absent;
}
// where result register q of output tile (rt, .) lands in B layout: r = q for row tile 0; row tile 1
// keeps register 0 alone, as r = 4 (its registers 1..3 are the padding rows 20..31)
constexpr unsigned k20x_acc_step(unsigned rt, unsigned q) { return rt == 0u ? q : (q == 0u ? 4u : kBx20Absent); }

// The re-deal of a squaring: the wave writes P and F from B layout to LDS and reads them back in A
// layout.  Row-major with an odd row stride, so that the 16 rows an A-layout read touches at once fall
// into different banks.  [matrix 0: P, 1: F][20][21] doubles.
constexpr unsigned kBx20LdsStride = 21;
constexpr unsigned kBx20LdsMatrix = kBx20States * kBx20LdsStride;
constexpr unsigned k20x_lds_index(unsigned matrix, unsigned dense) {
  return matrix * kBx20LdsMatrix + (dense / kBx20States) * kBx20LdsStride + dense % kBx20States;
}
constexpr size_t k20x_lds_bytes() { return 2 * kBx20LdsMatrix * sizeof(double); }

// One problem as the host hands it to the device: the rate-matrix set, the factor rho tau, and the
// scaling pgrad::block_scaling chose for X = rho tau Q^T -- the wave's trip count is the host's.
struct k20x_problem_t {
  double rho_tau, scale;
  unsigned set;
  int squarings;
};

}  // namespace rdamd
