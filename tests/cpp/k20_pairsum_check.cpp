// Host check of csrc/k20_preorder.hpp's pair-sum arithmetic: the re-deal of the two operands and the
// 25 MFMAs of the 20-state pair-sum consumer (kernels_preorder_k20.hip, PairSumK20), proven on the
// emulation of v_mfma_f64_4x4x4_4b_f64 by its lane map that k20_preorder_check.cpp uses.  A wave
// holds, per lane (col = site, grp), five states of the scaled outer vector T and of the child's
// vector L; small integers without symmetry, so every product is exact.  The re-dealt operands and
// the 25 MFMAs, folded over the four quads of sites, must give N[i][j] = sum_s T[s][i] L[s][j] in every
// entry; sites masked as past S (T = 0 there) must add nothing; the swapped gather (T and L exchanged)
// yields N^T and must fail.  Also the consumer's LDS layout inside the walk's exchange area at 1 to 8
// rate categories, and the partial row's size.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "k20_preorder.hpp"

using namespace rdamd;

// one four-block MFMA: d += A . B, every operand one double per lane (k20_preorder_check.cpp's)
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

// the wave's sum as the kernel forms it: x is the A side, y the B side, both [lane][5] as the walk
// holds them; n[entry] from the lanes with col < 4 after the fold over the quads (4 apart, then 8)
static void wave_sum(const double (&x)[64][5], const double (&y)[64][5], double (&n)[400], int (&written)[400]) {
  double av[64][5], bv[64][5];
  for (unsigned lane = 0; lane < 64; ++lane) {
    const unsigned src = k20_pair_source_lane(lane);
    if (src >= 64) { std::printf("source lane out of range\n"); std::exit(1); }
    for (unsigned t = 0; t < 5; ++t) { av[lane][t] = x[src][t]; bv[lane][t] = y[src][t]; }
  }
  for (unsigned ib = 0; ib < 5; ++ib)
    for (unsigned jb = 0; jb < 5; ++jb) {
      double a[64], b[64], d[64] = {0};
      for (unsigned lane = 0; lane < 64; ++lane) { a[lane] = av[lane][ib]; b[lane] = bv[lane][jb]; }
      mfma_4x4x4_4b(a, b, d);
      double f[64];
      for (unsigned lane = 0; lane < 64; ++lane) f[lane] = d[lane] + d[lane ^ 4u];
      for (unsigned lane = 0; lane < 64; ++lane) d[lane] = f[lane] + f[lane ^ 8u];
      for (unsigned lane = 0; lane < 64; ++lane) {
        if (lane % 16 >= 4) continue;
        const unsigned e = k20_pair_entry(lane, ib, jb);
        if (e >= 400) { std::printf("entry out of range\n"); std::exit(1); }
        n[e] = d[lane];
        ++written[e];
      }
    }
}

int main() {
  unsigned long checks = 0;
  int bad = 0;
  // the re-deal is a permutation of the lanes and its own inverse
  for (unsigned lane = 0; lane < 64; ++lane, ++checks)
    if (k20_pair_source_lane(lane) >= 64 || k20_pair_source_lane(k20_pair_source_lane(lane)) != lane) {
      std::printf("source lane of %u\n", lane); ++bad;
    }
  std::mt19937 rng(2020);
  for (int trial = 0; trial < 60; ++trial) {
    const unsigned S = trial < 16 ? (unsigned)trial + 1u : 1u + rng() % 16u;   // sites of the tile that exist
    double T[16][20], L[16][20];
    for (auto &row : T) for (double &v : row) v = (double)(rng() % 7u);
    for (auto &row : L) for (double &v : row) v = (double)(rng() % 5u);
    T[0][3] = 5.0; L[0][3] = 0.0; T[0][11] = 0.0; L[0][11] = 3.0;   // never symmetric: N[3][11] != N[11][3]
    double x[64][5], y[64][5];
    for (unsigned lane = 0; lane < 64; ++lane)
      for (unsigned t = 0; t < 5; ++t) {
        const unsigned s = lane % 16, state = k20p_state_of(lane / 16, t);
        x[lane][t] = s < S ? T[s][state] : 0.0;   // a lane past S: its factor is 0, its L the last site's
        y[lane][t] = L[s < S ? s : S - 1][state];
      }
    double want[400], want_t[400];
    for (unsigned i = 0; i < 20; ++i)
      for (unsigned j = 0; j < 20; ++j) {
        double acc = 0.0;
        for (unsigned s = 0; s < S; ++s) acc += T[s][i] * L[s][j];
        want[i * 20 + j] = acc;
        want_t[j * 20 + i] = acc;
      }
    double n[400];
    int written[400] = {0};
    wave_sum(x, y, n, written);
    unsigned wrong = 0, wrong_t = 0;
    for (unsigned e = 0; e < 400; ++e, ++checks) {
      if (written[e] != 1) { std::printf("trial %d: entry %u written %d times\n", trial, e, written[e]); ++bad; }
      if (n[e] != want[e]) ++wrong;
      if (n[e] != want_t[e]) ++wrong_t;
    }
    if (wrong) { std::printf("trial %d (S %u): %u entries wrong\n", trial, S, wrong); ++bad; }
    if (!wrong_t) { std::printf("trial %d: the operands do not tell N from N^T\n", trial); ++bad; }
    // the swapped gather: N^T in every entry, so it must fail against N
    int written2[400] = {0};
    wave_sum(y, x, n, written2);
    wrong = wrong_t = 0;
    for (unsigned e = 0; e < 400; ++e, ++checks) {
      if (n[e] != want[e]) ++wrong;
      if (n[e] != want_t[e]) ++wrong_t;
    }
    if (!wrong) { std::printf("trial %d: the swapped gather passes\n", trial); ++bad; }
    if (wrong_t) { std::printf("trial %d: the swapped gather is not N^T\n", trial); ++bad; }
  }
  // LDS: the terms of both parities, both children and the root, disjoint, inside the exchange area
  for (unsigned R = 1; R <= kK20MaxRates; ++R) {
    std::vector<int> seen(k20_pair_exchange_doubles(R), 0);
    auto take = [&](size_t at) {
      ++checks;
      if (at >= seen.size() || seen[at]++) { std::printf("R %u: LDS index %zu\n", R, at); ++bad; }
    };
    for (unsigned par = 0; par < 2; ++par)
      for (unsigned ch = 0; ch < 2; ++ch)
        for (unsigned r = 0; r < R; ++r)
          for (unsigned s = 0; s < 16; ++s) take(k20_pair_term_index(R, par, ch, r, s));
    for (unsigned r = 0; r < R; ++r)
      for (unsigned s = 0; s < 16; ++s) take(k20_pair_root_index(R, r, s));
    if (k20_pair_exchange_doubles(R) * sizeof(double) > k20_preorder_exchange_bytes(R)) { std::printf("R %u: LDS does not fit\n", R); ++bad; }
    if (k20_preorder_lds_bytes(R) != R * (2 * 3200 + 2 * 2560) + 128) { std::printf("R %u: the walk's LDS grew\n", R); ++bad; }
  }
  if (k20_pair_sum_entries(199, 4) * 8 != 8 * (199ul * 2 * 4 * 400 + 4 * 21) || k20_pair_root_at(3, 2) != 3 * 2 * 2 * 400) {
    std::printf("row size\n"); ++bad;
  }
  if (bad) { std::printf("k20 pairsum FAILED: %d\n", bad); return 1; }
  std::printf("k20 pairsum OK %lu\n", checks);
  return 0;
}
