// csrc/subst_map.hpp without a device (tests/test_subst_host.py): the count matrices
// C = F(X, offdiag(X)) and the typed counts from pair sums, for K = 2, 4 and 20, branch lengths 0,
// 1e-6, 0.1, 3 and 100 and R = 3 rate categories over two rate matrices.
//   equal rates:   X = a (J - K I)  gives  C = a (K - 1) J / K - a exp(-K a) (I - J / K)   (closed form)
//   any X:         C >= 0;  C = 0 at length 0;  C = d/de exp(X + e offdiag(X)) at e = 0, taken as a
//                  central difference of block_exp's own exponential
//   typed counts:  sum_i D[i] = tau sum_r <N_r, P_r>   and
//                  sum_{i != j} E[i][j] + sum_r sum_i X_r[i][i] F_r[i][i] = sum_r <N_r, X_r P_r>
//   error codes:   64 (null, state count, length), 7 (index)
// Prints the number of checks.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "subst_map.hpp"

namespace {

long checks = 0;

void near(double got, double want, double scale, double tol, const char *what, unsigned K, double tau) {
  ++checks;
  if (!(std::fabs(got - want) <= tol * scale)) {
    std::printf("FAIL %s K %u length %g: got %.17g want %.17g (scale %g)\n", what, K, tau, got, want, scale);
    std::exit(1);
  }
}

void expect(bool ok, const char *what) {
  ++checks;
  if (!ok) {
    std::printf("FAIL %s\n", what);
    std::exit(1);
  }
}

struct Lcg {
  unsigned long long s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
};

}  // namespace

int main() {
  using namespace rdamd;
  Lcg rng{2024};
  const unsigned sizes[] = {2, 4, 20};
  const double taus[] = {0.0, 1e-6, 0.1, 3.0, 100.0};
  const unsigned R = 3, sets = 2;
  const unsigned pidx[R] = {1, 0, 1};
  const double rates[R] = {0.07, 0.9, 2.6};
  for (unsigned K : sizes) {
    const size_t n = (size_t)K * K, nsub = n - K;
    // ---- equal rates: the closed form, through count_matrices with one matrix and one category
    {
      std::vector<double> q(n), c(n * 5);
      for (unsigned i = 0; i < K; ++i)
        for (unsigned j = 0; j < K; ++j) q[i * K + j] = i == j ? -1.0 : 1.0 / (K - 1);
      const unsigned zero = 0;
      const double one = 1.0;
      smap::count_matrices(K, 1, q.data(), &zero, &one, taus, 5, c.data());
      for (unsigned b = 0; b < 5; ++b) {
        const double a = taus[b] / (K - 1), decay = a * std::exp(-(double)K * a);
        for (unsigned i = 0; i < K; ++i)
          for (unsigned j = 0; j < K; ++j) {
            const double want = a * (K - 1) / K - decay * ((i == j ? 1.0 : 0.0) - 1.0 / K);
            near(c[b * n + i * K + j], want, std::fmax(a, 1e-300), 1e-12, "equal-rates C", K, taus[b]);
          }
      }
    }
    // ---- UNREST matrices
    std::vector<double> subst(sets * nsub), freqs(sets * K), raw(n), q(sets * n);
    for (double &v : subst) v = 0.1 + 1.4 * rng.next();
    for (unsigned m = 0; m < sets; ++m) {
      double sum = 0.0;
      for (unsigned i = 0; i < K; ++i) sum += freqs[m * K + i] = 0.2 + rng.next();
      for (unsigned i = 0; i < K; ++i) freqs[m * K + i] /= sum;
      pgrad::build_q(K, subst.data() + m * nsub, freqs.data() + m * K, raw.data(), q.data() + m * n);
    }
    const unsigned n_ops = 3;   // six branches: the five lengths and 0 again
    const double lengths[6] = {taus[0], taus[1], taus[2], taus[3], taus[4], 0.0};
    std::vector<double> cm(6 * R * n);
    smap::count_matrices(K, R, q.data(), pidx, rates, lengths, 6, cm.data());
    std::vector<double> x(n), e(n), xp(n), xm(n), pp(n), pm(n), f(n), p(n), xpm(n);
    for (unsigned b = 0; b < 6; ++b)
      for (unsigned r = 0; r < R; ++r) {
        const double *c = cm.data() + (b * R + r) * n, *qm = q.data() + pidx[r] * n;
        const double rt = rates[r] * lengths[b];
        double largest = 0.0, norm = 0.0;
        for (unsigned i = 0; i < K; ++i) norm = std::fmax(norm, -rt * qm[i * K + i]);   // the row sums of offdiag(X)
        // the step: h norm <= 1e-3 keeps the truncation (h norm)^2 norm / 6 below 2e-7 of C ~ norm, and
        // the rounding 2^-53 / h below 1e-7 of the smallest C here (length 1e-6)
        const double h = 1e-3 / std::fmax(1.0, norm);
        for (size_t i = 0; i < n; ++i) {
          x[i] = rt * qm[i];
          e[i] = i % (K + 1) == 0 ? 0.0 : x[i];
          xp[i] = x[i] + h * e[i];
          xm[i] = x[i] - h * e[i];
          largest = std::fmax(largest, c[i]);
        }
        pgrad::block_exp(K, xp.data(), e.data(), pp.data(), f.data());
        pgrad::block_exp(K, xm.data(), e.data(), pm.data(), f.data());
        for (size_t i = 0; i < n; ++i) {
          expect(c[i] >= 0.0 && std::isfinite(c[i]), "C is finite and not negative");
          if (lengths[b] == 0.0) expect(c[i] == 0.0, "C = 0 on a branch of length 0");
          near(c[i], (pp[i] - pm[i]) / (2 * h), std::fmax(largest, 1e-12), 1e-6, "C is the derivative of exp", K, lengths[b]);
        }
      }
    // ---- typed counts from random non-negative pair sums
    std::vector<double> pair(6 * R * n), typed(6 * n);
    for (double &v : pair) v = rng.next() < 0.2 ? 0.0 : 5.0 * rng.next();
    expect(smap::counts_from_pair_sums(K, R, sets, n_ops, pair.data(), lengths, subst.data(), freqs.data(), pidx, rates,
                                       typed.data()) == 0, "counts_from_pair_sums succeeds");
    for (unsigned b = 0; b < 6; ++b) {
      double dwell = 0.0, np_sum = 0.0, e_sum = 0.0, diag = 0.0, nxp = 0.0, scale = 0.0;
      for (unsigned i = 0; i < K; ++i)
        for (unsigned j = 0; j < K; ++j) {
          expect(typed[b * n + i * K + j] >= 0.0, "typed counts are not negative");
          if (i == j) dwell += typed[b * n + i * K + j];
          else e_sum += typed[b * n + i * K + j];
        }
      for (unsigned r = 0; r < R; ++r) {
        const double *qm = q.data() + pidx[r] * n, *nn = pair.data() + (b * R + r) * n;
        const double rt = rates[r] * lengths[b];
        for (unsigned i = 0; i < K; ++i)
          for (unsigned j = 0; j < K; ++j) { x[i * K + j] = rt * qm[i * K + j]; xpm[i * K + j] = rt * qm[j * K + i]; }
        pgrad::block_exp(K, x.data(), x.data(), p.data(), f.data());
        pgrad::matmul(K, x.data(), p.data(), xp.data());
        for (size_t i = 0; i < n; ++i) { np_sum += nn[i] * p[i]; nxp += nn[i] * xp[i]; scale += nn[i] * std::fabs(xp[i]); }
        pgrad::block_exp(K, xpm.data(), nn, p.data(), f.data());   // F_r, for the diagonal term
        for (unsigned i = 0; i < K; ++i) { diag += x[i * K + i] * f[i * K + i]; scale += std::fabs(x[i * K + i]) * f[i * K + i]; }
      }
      near(dwell, lengths[b] * np_sum, lengths[b] * np_sum, 1e-11, "sum D = tau <N, P>", K, lengths[b]);
      near(e_sum + diag, nxp, scale + e_sum, 1e-11, "sum E + diagonal term = <N, X P>", K, lengths[b]);
      if (lengths[b] == 0.0) expect(e_sum == 0.0 && dwell == 0.0, "no counts on a branch of length 0");
    }
    // ---- error codes
    const unsigned bad_idx[R] = {0, 2, 1};
    double bad_len[6] = {0.1, 0.1, -1.0, 0.1, 0.1, 0.1};
    expect(smap::counts_from_pair_sums(K, R, sets, n_ops, pair.data(), lengths, subst.data(), freqs.data(), bad_idx, rates,
                                       typed.data()) == 7, "index out of range is 7");
    expect(smap::counts_from_pair_sums(K, R, sets, n_ops, nullptr, lengths, subst.data(), freqs.data(), pidx, rates,
                                       typed.data()) == 64, "null input is 64");
    expect(smap::counts_from_pair_sums(K, R, sets, n_ops, pair.data(), bad_len, subst.data(), freqs.data(), pidx, rates,
                                       typed.data()) == 64, "negative length is 64");
    bad_len[2] = INFINITY;
    expect(smap::counts_from_pair_sums(K, R, sets, n_ops, pair.data(), bad_len, subst.data(), freqs.data(), pidx, rates,
                                       typed.data()) == 64, "infinite length is 64");
    expect(smap::counts_from_pair_sums(65, R, sets, n_ops, pair.data(), lengths, subst.data(), freqs.data(), pidx, rates,
                                       typed.data()) == 64, "65 states is 64");
    expect(smap::counts_from_pair_sums(1, R, sets, n_ops, pair.data(), lengths, subst.data(), freqs.data(), pidx, rates,
                                       typed.data()) == 64, "1 state is 64");
  }
  std::printf("subst counts OK %ld\n", checks);
  return 0;
}
