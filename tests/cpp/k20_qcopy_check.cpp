// Host check of the 20-state derivative consumer's host-side packing (csrc/k20_preorder.hpp,
// k20_pack_copy): the MFMA-ready copy of a normalised rate matrix that rdamd_branch_length_derivatives
// builds on the host and the kernel reads as the A operand of z = Q y and z2 = Q z.  The matrix
// cores are emulated by their lane map as in k20_preorder_check.cpp (v_mfma_f64_4x4x4_4b_f64: with
// col = lane % 16 and grp = lane / 16, A: i = col % 4, k = grp, of the block col / 4; B: site = col,
// k = grp; D: site = col, i = grp).  Random ASYMMETRIC 20 x 20 matrices of small integers, so every
// product is exact: through the forward gather the copy must give dense Q y and, fed its own result,
// dense Q (Q y), in every lane; the copy of the TRANSPOSED matrix and the transposed gather must not.
// Also the consumer's LDS layout: copies and terms are disjoint, inside the exchange area, at 1 to 8
// rate categories.
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
    for (unsigned k = 0; k < 4; ++k) acc += a[16 * k + 4 * block + i] * b[16 * k + col];
    out[lane] = acc;
  }
  for (unsigned lane = 0; lane < 64; ++lane) d[lane] = out[lane];
}

typedef unsigned (*Gather)(unsigned rg, unsigned ks, unsigned col, unsigned grp);

// the kernel's k20_product: in[lane][t] = operand t of the lane's vector, res likewise
static void product(const std::vector<double> &copy, Gather gather, const double (&in)[64][5], double (&res)[64][5]) {
  for (unsigned rg = 0; rg < kK20Groups; ++rg) {
    double d[64] = {0};
    for (unsigned ks = 0; ks < kK20Steps; ++ks) {
      double a[64], b[64];
      for (unsigned lane = 0; lane < 64; ++lane) {
        const unsigned at = gather(rg, ks, lane % 16, lane / 16);
        if (at >= copy.size()) { std::printf("gather out of range\n"); std::exit(1); }
        a[lane] = copy[at];
        b[lane] = in[lane][ks];
      }
      mfma_4x4x4_4b(a, b, d);
    }
    for (unsigned lane = 0; lane < 64; ++lane) res[lane][rg] = d[lane];
  }
}

// lanes' entries that differ from want[site][state]
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
  std::mt19937 rng(19);
  for (int trial = 0; trial < 50; ++trial) {
    std::vector<double> Q(400), QT(400);
    for (double &x : Q) x = (double)(rng() % 7u) - 3.0;   // (a rate matrix has both signs)
    Q[3 * 20 + 11] = 3.0; Q[11 * 20 + 3] = -2.0;          // never symmetric
    for (unsigned i = 0; i < 20; ++i)
      for (unsigned j = 0; j < 20; ++j) QT[i * 20 + j] = Q[j * 20 + i];
    double y[16][20], qy[16][20], qqy[16][20], qty[16][20];
    for (auto &row : y) for (double &x : row) x = (double)(rng() % 5u);
    for (unsigned s = 0; s < 16; ++s) {
      for (unsigned i = 0; i < 20; ++i) {
        qy[s][i] = qty[s][i] = 0.0;
        for (unsigned j = 0; j < 20; ++j) { qy[s][i] += Q[i * 20 + j] * y[s][j]; qty[s][i] += Q[j * 20 + i] * y[s][j]; }
      }
      for (unsigned i = 0; i < 20; ++i) {
        qqy[s][i] = 0.0;
        for (unsigned j = 0; j < 20; ++j) qqy[s][i] += Q[i * 20 + j] * qy[s][j];
      }
    }
    std::vector<double> copy(kK20CopyDoubles, -1000.0), copy_t(kK20CopyDoubles, -1000.0);
    k20_pack_copy(Q.data(), copy.data());
    k20_pack_copy(QT.data(), copy_t.data());
    // every entry of the copy is written, and holds Q[state_of(i, rg)][state_of(k, ks)]
    for (unsigned rg = 0; rg < 5; ++rg)
      for (unsigned ks = 0; ks < 5; ++ks)
        for (unsigned k = 0; k < 4; ++k)
          for (unsigned i = 0; i < 4; ++i, ++checks)
            if (copy[k20_copy_index(rg, ks, k, i)] != Q[k20p_state_of(i, rg) * 20 + k20p_state_of(k, ks)]) {
              std::printf("trial %d: copy entry (%u, %u, %u, %u)\n", trial, rg, ks, k, i); ++bad;
            }
    double in[64][5], z[64][5], z2[64][5], other[64][5];
    for (unsigned lane = 0; lane < 64; ++lane)
      for (unsigned t = 0; t < 5; ++t) in[lane][t] = y[lane % 16][k20p_state_of(lane / 16, t)];
    product(copy, k20_a_forward, in, z);
    if (mismatches(z, qy)) { std::printf("trial %d: Q y wrong in %u entries\n", trial, mismatches(z, qy)); ++bad; }
    if (!mismatches(z, qty)) { std::printf("trial %d: the matrix does not tell Q from Q^T\n", trial); ++bad; }
    product(copy, k20_a_forward, z, z2);   // (the D layout is the B layout: the result feeds the next product as it lies)
    if (mismatches(z2, qqy)) { std::printf("trial %d: Q (Q y) wrong in %u entries\n", trial, mismatches(z2, qqy)); ++bad; }
    product(copy_t, k20_a_forward, in, other);
    if (!mismatches(other, qy) || mismatches(other, qty)) { std::printf("trial %d: the transposed matrix's copy\n", trial); ++bad; }
    product(copy, k20_a_transposed, in, other);
    if (!mismatches(other, qy) || mismatches(other, qty)) { std::printf("trial %d: the transposed gather\n", trial); ++bad; }
    checks += 4 * 64 * 5;
  }
  // the consumer's LDS: [rate][400] copies, then [parity][child][rate][3][16] terms, inside the exchange area
  for (unsigned R = 1; R <= kK20MaxRates; ++R) {
    const size_t area = k20_preorder_exchange_bytes(R) / sizeof(double);
    std::vector<int> seen(area, 0);
    for (size_t e = 0; e < (size_t)R * kK20CopyDoubles; ++e) seen[e]++;
    for (unsigned par = 0; par < 2; ++par)
      for (unsigned ch = 0; ch < 2; ++ch)
        for (unsigned r = 0; r < R; ++r)
          for (unsigned term = 0; term < 3; ++term)
            for (unsigned s = 0; s < 16; ++s, ++checks) {
              const size_t at = k20_brlen_term_index(R, par, ch, r, term, s);
              if (at >= area || seen[at]++) { std::printf("R %u: term (%u, %u, %u, %u, %u)\n", R, par, ch, r, term, s); ++bad; }
            }
    if (k20_brlen_exchange_doubles(R) > area || k20_brlen_terms_at(R) % 2) { std::printf("R %u: layout\n", R); ++bad; }
    // (the kernel reads the three terms of a site 16 doubles apart)
    if (k20_brlen_term_index(R, 1, 1, R - 1, 2, 3) != k20_brlen_term_index(R, 1, 1, R - 1, 0, 3) + 32) { std::printf("pitch\n"); ++bad; }
  }
  if (bad) { std::printf("k20 qcopy FAILED: %d\n", bad); return 1; }
  std::printf("k20 qcopy OK %lu\n", checks);
  return 0;
}
