// Host check of csrc/k20_block_exp.hpp: the operand layouts of the 20-state device block exponential
// (kernels_block_exp.hip), proven on an emulation of v_mfma_f64_16x16x4_f64 by its lane map.  With
// small-integer matrices without symmetry every product is exact, so every entry must agree exactly:
//   - a left product c = a b taken with b straight from accumulator layout, 20 MFMAs;
//   - one full Taylor step  D' = (X D + E T) / k, T' = X T / k  (k a power of two: exact);
//   - the re-deal of a squaring, B layout -> LDS -> A layout;
//   - one squaring step  (P, F) -> (P P, P F + F P);
//   - the transposed gather (k20x_a_index's entry transposed) yields the product with a^T and fails.
// Also: the layouts cover every entry exactly once, the padding positions stay zero, and the LDS
// indices of the re-deal are distinct and inside k20x_lds_bytes().
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "k20_block_exp.hpp"

using namespace rdamd;

constexpr unsigned K = kBx20States, NT = kBx20Tiles, NS = kBx20Steps;
typedef double mat_t[K * K];
typedef double frag_t[64][NT][NS];   // a matrix in A or B layout, per lane

// one v_mfma_f64_16x16x4_f64: d += A . B; a and b one double per lane, d four
static void mfma_16x16x4(const double (&a)[64], const double (&b)[64], double (&d)[64][4]) {
  for (unsigned lane = 0; lane < 64; ++lane) {
    const unsigned col = lane % 16, grp = lane / 16;
    for (unsigned q = 0; q < 4; ++q) {
      const unsigned row = grp + 4 * q;
      double acc = d[lane][q];
      for (unsigned k = 0; k < 4; ++k) acc += a[16 * k + row] * b[16 * k + col];   // A[row][k] of lane (row, k), B[k][col] of lane (col, k)
      d[lane][q] = acc;
    }
  }
}

static unsigned long checks = 0;
static int bad = 0;
static void fail(const char *what) { std::printf("%s\n", what); ++bad; }

static void to_a(const mat_t &m, frag_t &f, bool transposed = false) {
  for (unsigned lane = 0; lane < 64; ++lane)
    for (unsigned rt = 0; rt < NT; ++rt)
      for (unsigned r = 0; r < NS; ++r) {
        const unsigned at = k20x_a_index(lane, rt, r);
        if (at != kBx20Absent && at >= K * K) { fail("A index out of range"); std::exit(1); }
        f[lane][rt][r] = at == kBx20Absent ? 0.0 : m[transposed ? (at % K) * K + at / K : at];
      }
}
static void to_b(const mat_t &m, frag_t &f) {
  for (unsigned lane = 0; lane < 64; ++lane)
    for (unsigned ct = 0; ct < NT; ++ct)
      for (unsigned r = 0; r < NS; ++r) {
        const unsigned at = k20x_b_index(lane, ct, r);
        if (at != kBx20Absent && at >= K * K) { fail("B index out of range"); std::exit(1); }
        f[lane][ct][r] = at == kBx20Absent ? 0.0 : m[at];
      }
}
// B layout back to a dense matrix: every entry exactly once, padding exactly zero
static void from_b(const frag_t &f, mat_t &m) {
  int written[K * K] = {0};
  for (unsigned lane = 0; lane < 64; ++lane)
    for (unsigned ct = 0; ct < NT; ++ct)
      for (unsigned r = 0; r < NS; ++r, ++checks) {
        const unsigned at = k20x_b_index(lane, ct, r);
        if (at == kBx20Absent) { if (f[lane][ct][r] != 0.0) fail("a padding position is not zero"); continue; }
        m[at] = f[lane][ct][r];
        ++written[at];
      }
  for (unsigned e = 0; e < K * K; ++e, ++checks)
    if (written[e] != 1) fail("B layout does not hold every entry once");
}

// the kernel's left_product: c = a b, the accumulators placed by k20x_acc_step
static void left_product(const frag_t &a, const frag_t &b, frag_t &c) {
  for (unsigned ct = 0; ct < NT; ++ct)
    for (unsigned rt = 0; rt < NT; ++rt) {
      double acc[64][4] = {{0}};
      for (unsigned r = 0; r < NS; ++r) {
        double av[64], bv[64];
        for (unsigned lane = 0; lane < 64; ++lane) { av[lane] = a[lane][rt][r]; bv[lane] = b[lane][ct][r]; }
        mfma_16x16x4(av, bv, acc);
      }
      for (unsigned lane = 0; lane < 64; ++lane)
        for (unsigned q = 0; q < 4; ++q) {
          const unsigned step = k20x_acc_step(rt, q);
          if (step == kBx20Absent) { if (acc[lane][q] != 0.0) fail("a padding row is not zero"); continue; }
          if (step >= NS) { fail("accumulator step out of range"); std::exit(1); }
          c[lane][ct][step] = acc[lane][q];
        }
    }
}

// the re-deal of a squaring: B layout -> LDS -> A layout
static void redeal(const frag_t &p, const frag_t &f, frag_t &pa, frag_t &fa) {
  std::vector<double> lds(k20x_lds_bytes() / sizeof(double), -77.0);
  std::vector<int> seen(lds.size(), 0);
  for (unsigned lane = 0; lane < 64; ++lane)
    for (unsigned ct = 0; ct < NT; ++ct)
      for (unsigned r = 0; r < NS; ++r) {
        const unsigned at = k20x_b_index(lane, ct, r);
        if (at == kBx20Absent) continue;
        for (unsigned m = 0; m < 2; ++m, ++checks) {
          const unsigned i = k20x_lds_index(m, at);
          if (i >= lds.size() || seen[i]++) { fail("LDS index out of range or taken twice"); std::exit(1); }
          lds[i] = m == 0 ? p[lane][ct][r] : f[lane][ct][r];
        }
      }
  for (unsigned lane = 0; lane < 64; ++lane)
    for (unsigned rt = 0; rt < NT; ++rt)
      for (unsigned r = 0; r < NS; ++r) {
        const unsigned at = k20x_a_index(lane, rt, r);
        pa[lane][rt][r] = at == kBx20Absent ? 0.0 : lds[k20x_lds_index(0, at)];
        fa[lane][rt][r] = at == kBx20Absent ? 0.0 : lds[k20x_lds_index(1, at)];
      }
}

static void dense_product(const mat_t &a, const mat_t &b, mat_t &c) {
  for (unsigned i = 0; i < K; ++i)
    for (unsigned j = 0; j < K; ++j) {
      double s = 0.0;
      for (unsigned l = 0; l < K; ++l) s += a[i * K + l] * b[l * K + j];
      c[i * K + j] = s;
    }
}
static unsigned differ(const mat_t &a, const mat_t &b) {
  unsigned n = 0;
  for (unsigned e = 0; e < K * K; ++e, ++checks) n += a[e] != b[e];
  return n;
}
static void random_matrix(std::mt19937 &rng, mat_t &m, unsigned span) {
  for (double &v : m) v = (double)(rng() % span) - (double)(span / 3);
  m[3 * K + 11] = 5.0; m[11 * K + 3] = -2.0; m[0 * K + 19] = 4.0; m[19 * K + 0] = 1.0;   // never symmetric
}

int main() {
  std::mt19937 rng(2121);
  static frag_t xa, ea, db, tb, t1, t2, d2, tn, pa, fa, pb, fb, got;
  for (int trial = 0; trial < 40; ++trial) {
    mat_t X, E, D, T, want, tmp, back;
    random_matrix(rng, X, 9); random_matrix(rng, E, 7); random_matrix(rng, D, 11); random_matrix(rng, T, 5);

    // 1. a left product: the accumulator of X D is the B operand of X (X D)
    to_a(X, xa); to_b(D, db);
    from_b(db, back);
    if (differ(back, D)) fail("B layout does not round-trip");
    left_product(xa, db, t1);
    from_b(t1, back);
    dense_product(X, D, want);
    if (differ(back, want)) fail("left product X D");
    left_product(xa, t1, t2);   // straight from accumulator layout
    from_b(t2, back);
    dense_product(X, want, tmp);
    if (differ(back, tmp)) fail("left product X (X D) from the accumulator");

    // the transposed gather yields X^T D: it must fail against X D and be X^T D
    mat_t XT, want_t;
    for (unsigned i = 0; i < K; ++i) for (unsigned j = 0; j < K; ++j) XT[i * K + j] = X[j * K + i];
    to_a(X, got, true);
    left_product(got, db, t2);
    from_b(t2, back);
    dense_product(XT, D, want_t);
    if (!differ(back, want)) fail("the transposed gather passes");
    if (differ(back, want_t)) fail("the transposed gather is not X^T D");

    // 2. one full Taylor step with k = 2 (1 / k exact):  D' = (X D + E T) / 2,  T' = X T / 2
    to_a(E, ea); to_b(T, tb);
    left_product(xa, db, t1);
    left_product(ea, tb, t2);
    for (unsigned lane = 0; lane < 64; ++lane)
      for (unsigned ct = 0; ct < NT; ++ct)
        for (unsigned r = 0; r < NS; ++r) d2[lane][ct][r] = (t1[lane][ct][r] + t2[lane][ct][r]) * 0.5;
    left_product(xa, tb, t1);
    for (unsigned lane = 0; lane < 64; ++lane)
      for (unsigned ct = 0; ct < NT; ++ct)
        for (unsigned r = 0; r < NS; ++r) tn[lane][ct][r] = t1[lane][ct][r] * 0.5;
    mat_t xd, et, xt;
    dense_product(X, D, xd); dense_product(E, T, et); dense_product(X, T, xt);
    for (unsigned e = 0; e < K * K; ++e) { want[e] = (xd[e] + et[e]) * 0.5; tmp[e] = xt[e] * 0.5; }
    from_b(d2, back);
    if (differ(back, want)) fail("Taylor step: D'");
    from_b(tn, back);
    if (differ(back, tmp)) fail("Taylor step: T'");

    // 3. the re-deal: P and F from B layout are P and F in A layout
    const mat_t &P = D, &F = T;
    to_b(P, pb); to_b(F, fb);
    redeal(pb, fb, pa, fa);
    to_a(P, got);
    for (unsigned lane = 0; lane < 64; ++lane)
      for (unsigned rt = 0; rt < NT; ++rt)
        for (unsigned r = 0; r < NS; ++r, checks += 2) {
          if (pa[lane][rt][r] != got[lane][rt][r]) fail("re-deal of P");
        }
    to_a(F, got);
    for (unsigned lane = 0; lane < 64; ++lane)
      for (unsigned rt = 0; rt < NT; ++rt)
        for (unsigned r = 0; r < NS; ++r)
          if (fa[lane][rt][r] != got[lane][rt][r]) fail("re-deal of F");

    // 4. one squaring step: (P, F) -> (P P, P F + F P)
    left_product(pa, fb, t1);
    left_product(fa, pb, t2);
    left_product(pa, pb, d2);
    for (unsigned lane = 0; lane < 64; ++lane)
      for (unsigned ct = 0; ct < NT; ++ct)
        for (unsigned r = 0; r < NS; ++r) tn[lane][ct][r] = t1[lane][ct][r] + t2[lane][ct][r];
    mat_t pf, fp, pp;
    dense_product(P, F, pf); dense_product(F, P, fp); dense_product(P, P, pp);
    for (unsigned e = 0; e < K * K; ++e) want[e] = pf[e] + fp[e];
    from_b(tn, back);
    if (differ(back, want)) fail("squaring: P F + F P");
    if (!differ(pf, fp)) fail("P and F commute: the test cannot tell P F from F P");
    from_b(d2, back);
    if (differ(back, pp)) fail("squaring: P P");
  }
  // the identity in B layout, as the kernel forms it: the diagonal is where row = column
  for (unsigned lane = 0; lane < 64; ++lane)
    for (unsigned ct = 0; ct < NT; ++ct)
      for (unsigned r = 0; r < NS; ++r, ++checks) {
        const unsigned at = k20x_b_index(lane, ct, r);
        const unsigned row = (lane >> 4) + 4 * r, col = 16 * ct + (lane & 15);
        if ((at != kBx20Absent) != (col < K) || (at != kBx20Absent && (at / K != row || at % K != col))) fail("B index");
      }
  if (k20x_lds_bytes() != 2 * 20 * 21 * 8) fail("LDS size");
  if (bad) { std::printf("k20 blockexp FAILED: %d\n", bad); return 1; }
  std::printf("k20 blockexp OK %lu\n", checks);
  return 0;
}
