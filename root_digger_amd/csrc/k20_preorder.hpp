// The 20-state pre-order walk's index arithmetic (kernels_preorder_k20.hip): where a lane finds its
// A operand of the forward product P L and of the transposed product P^T t in the ONE MFMA-ready
// copy of a P-matrix, the sizes of the walk's workspace and LDS, the host-side packing of such a copy
// (the derivative consumer's rate matrices), that consumer's LDS layout, and the pair-sum consumer's
// re-deal of its two operands, its LDS layout and its row of partial sums.  Plain arithmetic over
// plain numbers -- no HIP, no partition -- so that tests/cpp/k20_preorder_check.cpp,
// tests/cpp/k20_qcopy_check.cpp and tests/cpp/k20_pairsum_check.cpp can emulate the matrix cores'
// lane map on the host and prove the gathers, the packing and the re-deal before any GPU run.
//
// Lanes (kernels_clv_mfma.hip): col = lane % 16 is the site of the wave's tile, grp = lane / 16; a
// vector of 20 states lives as five doubles per lane, operand t = state k20p_state_of(grp, t).
// One v_mfma_f64_4x4x4_4b_f64 takes from lane (col, grp)  A[i = col % 4][k = grp]  and
// B[k = grp][site = col]  and leaves  D[i = grp][site = col].
#pragma once

#include <cstddef>

namespace rdamd {

constexpr unsigned kK20States = 20, kK20Steps = 5, kK20Groups = 5;
constexpr unsigned kK20TileDoubles = 16 * kK20States;                  // one CLV tile: 16 sites of one rate
constexpr unsigned kK20CopyDoubles = kK20Groups * kK20Steps * 16;      // the MFMA-ready copy of one (matrix, rate)
constexpr unsigned kK20MaxRates = 8;

// (the same dealing and the same tile as common.hpp's k20_state_of / k20_tile_index, restated here
// without HIP; kernels_preorder_k20.hip asserts that they agree everywhere)
constexpr unsigned k20p_state_of(unsigned g, unsigned t) { return 5u * g + (t + (g & 1u)) % 5u; }
constexpr unsigned k20p_tile_index(unsigned site_in_tile, unsigned state) {
  const unsigned g = state / 5u, t = (state % 5u + 5u - (g & 1u)) % 5u, lane = 16u * g + site_in_tile;
  return t < 4u ? (t >> 1) * 128u + lane * 2u + (t & 1u) : 256u + lane;
}
// a lane's operand t of a tile, in doubles from the tile's start (k20p_tile_index of its state)
constexpr unsigned k20p_lane_operand(unsigned lane, unsigned t) {
  return t < 4u ? (t >> 1) * 128u + lane * 2u + (t & 1u) : 256u + lane;
}

// pmat_to_mfma_kernel's formula: the copy holds P[state_of(i, rg)][state_of(k, ks)] here
constexpr unsigned k20_copy_index(unsigned rg, unsigned ks, unsigned k, unsigned i) {
  return ((rg * kK20Steps + ks) * 4u + k) * 4u + i;
}

// FORWARD product  d[rg] = sum_ks A . b[ks]  with  d = P c:  the lane needs
// P[state_of(col % 4, rg)][state_of(grp, ks)]  = element (k = grp, i = col % 4) of block (rg, ks)
constexpr unsigned k20_a_forward(unsigned rg, unsigned ks, unsigned col, unsigned grp) {
  return k20_copy_index(rg, ks, grp, col & 3u);
}
// TRANSPOSED product  d[rg] = sum_ks A' . t[ks]  with  d = P^T t:  the lane needs
// P[state_of(grp, ks)][state_of(col % 4, rg)]  = element (k = col % 4, i = grp) of block (ks, rg):
// the same copy serves both products
constexpr unsigned k20_a_transposed(unsigned rg, unsigned ks, unsigned col, unsigned grp) {
  return k20_copy_index(ks, rg, col & 3u, grp);
}

// The MFMA-ready copy of a dense row-major 20 x 20 matrix, built on the host: what pmat_to_mfma_kernel
// makes of a P-matrix on the device, for the matrices that never pass through it (the derivative
// consumer's normalised rate matrices).  m: [20][20], copy: [kK20CopyDoubles].
inline void k20_pack_copy(const double *m, double *copy) {
  for (unsigned rg = 0; rg < kK20Groups; ++rg)
    for (unsigned ks = 0; ks < kK20Steps; ++ks)
      for (unsigned k = 0; k < 4u; ++k)
        for (unsigned i = 0; i < 4u; ++i)
          copy[k20_copy_index(rg, ks, k, i)] = m[k20p_state_of(i, rg) * kK20States + k20p_state_of(k, ks)];
}

// workspace of a program with `slots` slots: outer vectors in the operand layout, whole tiles
constexpr size_t k20_preorder_workspace_doubles(size_t slots, size_t rate_cats, size_t tiles) {
  return slots * rate_cats * tiles * kK20TileDoubles;
}

// LDS of one workgroup (R waves), in bytes: per wave the A copies of the operation's two children
// (wave-private), the consumer's exchange area of both children ([child][rate][320 doubles]: the
// posteriors' sum over rates), and the rescale flags ([parity][16] words)
constexpr size_t k20_preorder_stage_bytes(size_t rate_cats) { return rate_cats * 2 * kK20CopyDoubles * sizeof(double); }
constexpr size_t k20_preorder_exchange_bytes(size_t rate_cats) { return 2 * rate_cats * kK20TileDoubles * sizeof(double); }
constexpr size_t k20_preorder_flag_bytes() { return 2 * 16 * sizeof(unsigned); }
constexpr size_t k20_preorder_lds_bytes(size_t rate_cats) {
  return k20_preorder_stage_bytes(rate_cats) + k20_preorder_exchange_bytes(rate_cats) + k20_preorder_flag_bytes();
}
constexpr size_t kK20LdsLimit = 160 * 1024;   // one CU's LDS on gfx950
static_assert(k20_preorder_lds_bytes(kK20MaxRates) <= kK20LdsLimit, "the walk's LDS fits a CU at 8 rate categories");

// The derivative consumer's use of the exchange area, in doubles from its start: the R staged copies
// of the rate matrices ([rate][400]), then the per-rate terms w f0, w rho f1, w rho^2 f2 of both
// children of an operation, double-buffered by operation parity ([parity][child][rate][3][16 sites])
constexpr size_t k20_brlen_term_doubles(size_t rate_cats) { return 2 * 2 * rate_cats * 3 * 16; }
constexpr size_t k20_brlen_terms_at(size_t rate_cats) { return rate_cats * kK20CopyDoubles; }
constexpr size_t k20_brlen_term_index(size_t rate_cats, unsigned parity, unsigned child, unsigned rate, unsigned term,
                                      unsigned site_in_tile) {
  return k20_brlen_terms_at(rate_cats) + (((parity * 2u + child) * rate_cats + rate) * 3u + term) * 16u + site_in_tile;
}
constexpr size_t k20_brlen_exchange_doubles(size_t rate_cats) {
  return k20_brlen_terms_at(rate_cats) + k20_brlen_term_doubles(rate_cats);
}
constexpr bool k20_brlen_fits_exchange() {
  for (size_t r = 1; r <= kK20MaxRates; ++r)
    if (k20_brlen_exchange_doubles(r) * sizeof(double) > k20_preorder_exchange_bytes(r)) return false;
  return true;
}
static_assert(k20_brlen_fits_exchange(), "the derivative consumer lives in the exchange area: the walk's LDS does not grow");

// The pair-sum consumer.  A wave's sum over its 16 sites, N[i][j] = sum_s T[i][s] L[s][j], is a
// 20 x 16 by 16 x 20 product whose reduction dimension is the SITE, and a lane holds five states of
// ONE site: both operands are re-dealt.  With the four blocks of an MFMA taken as the four quads of
// sites (block b: sites 4 b .. 4 b + 3), lane (col, grp) supplies
//   A[i = col % 4][k = grp] = T[state_of(col % 4, ib)][site 4 (col / 4) + grp]
//   B[k = grp][n = col % 4] = L[site 4 (col / 4) + grp][state_of(col % 4, jb)]
// for ib, jb = 0..4: operand ib (jb) of the lane that holds that site and those states, which is
// the SAME lane for both operands and all five indices -- (col % 4, grp) transposed inside the quad.
// So the re-deal is one fixed lane permutation (its own inverse) of ten doubles and takes no LDS.
constexpr unsigned k20_pair_source_lane(unsigned lane) {
  const unsigned col = lane & 15u, grp = lane >> 4;
  return 16u * (col & 3u) + 4u * (col >> 2) + grp;
}
// MFMA (ib, jb) leaves in lane (col, grp) the quad's share of N[state_of(grp, ib)][state_of(col % 4, jb)];
// the four quads are folded over col / 4 (lanes 4 apart, then 8 apart).  The entry, i * 20 + j:
constexpr unsigned k20_pair_entry(unsigned lane, unsigned ib, unsigned jb) {
  return k20p_state_of(lane >> 4, ib) * kK20States + k20p_state_of(lane & 3u, jb);
}
// a tile's row of partial sums (= the result): [nops][2][R][20][20] pair sums, then [R][21]: M[r][0..19], W[r]
constexpr size_t k20_pair_sum_entries(size_t nops, size_t rate_cats) {
  return nops * 2 * rate_cats * kK20States * kK20States + rate_cats * (kK20States + 1);
}
constexpr size_t k20_pair_root_at(size_t nops, size_t rate_cats) { return nops * 2 * rate_cats * kK20States * kK20States; }
// Its use of the exchange area, in doubles from the start: the per-rate terms w_r t.(P_a L_a) of both
// children of an operation, double-buffered by operation parity ([parity][child][rate][16 sites]),
// then the per-rate terms w_r pi.L_root of the root ([rate][16 sites])
constexpr size_t k20_pair_term_index(size_t rate_cats, unsigned parity, unsigned child, unsigned rate, unsigned site_in_tile) {
  return ((parity * 2u + child) * rate_cats + rate) * 16u + site_in_tile;
}
constexpr size_t k20_pair_root_index(size_t rate_cats, unsigned rate, unsigned site_in_tile) {
  return (4u * rate_cats + rate) * 16u + site_in_tile;
}
constexpr size_t k20_pair_exchange_doubles(size_t rate_cats) { return 5 * rate_cats * 16; }
constexpr bool k20_pair_fits_exchange() {
  for (size_t r = 1; r <= kK20MaxRates; ++r)
    if (k20_pair_exchange_doubles(r) * sizeof(double) > k20_preorder_exchange_bytes(r)) return false;
  return true;
}
static_assert(k20_pair_fits_exchange(), "the pair-sum consumer lives in the exchange area: the walk's LDS does not grow");

}  // namespace rdamd
