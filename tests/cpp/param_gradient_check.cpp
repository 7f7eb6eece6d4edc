// csrc/param_gradient.hpp without a device (tests/test_param_gradient_host.py): the block
// exponential F(X, E) = integral_0^1 exp(xX) E exp((1 - x)X) dx against two closed forms.
//   diagonal X = diag(a):   F_ij = E_ij (exp(a_i) - exp(a_j)) / (a_i - a_j),  E_ij exp(a_i) where a_i = a_j
//   commuting arguments:    F(X, X) = X exp(X), and F(X, I) = exp(X)
// over sizes 2, 4, 5 and 20 and norms that need 0 to 12 squarings.  Prints the number of checks.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "param_gradient.hpp"

namespace {

long checks = 0;

// |got - want| against tol * scale
void near(double got, double want, double scale, double tol, const char *what, unsigned K, double norm) {
  ++checks;
  if (!(std::fabs(got - want) <= tol * scale)) {
    std::printf("FAIL %s K %u norm %g: got %.17g want %.17g (scale %g)\n", what, K, norm, got, want, scale);
    std::exit(1);
  }
}

// a small reproducible generator (values in [0, 1))
struct Lcg {
  unsigned long long s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
};

}  // namespace

int main() {
  using rdamd::pgrad::block_exp;
  using rdamd::pgrad::matmul;
  Lcg rng{12345};
  const unsigned sizes[] = {2, 4, 5, 20};
  const double norms[] = {1e-6, 0.2, 1.0, 30.0, 800.0};
  for (unsigned K : sizes)
    for (double norm : norms) {
      const size_t n = (size_t)K * K;
      std::vector<double> x(n, 0.0), e(n), p(n), f(n), xp(n), id(n, 0.0);
      // diagonal X with non-positive entries (a rate matrix's spectrum), two of them equal
      std::vector<double> a(K);
      for (unsigned i = 0; i < K; ++i) a[i] = -norm * rng.next();
      a[K - 1] = a[0];
      for (unsigned i = 0; i < K; ++i) x[i * K + i] = a[i];
      for (size_t i = 0; i < n; ++i) e[i] = rng.next();
      block_exp(K, x.data(), e.data(), p.data(), f.data());
      for (unsigned i = 0; i < K; ++i)
        for (unsigned j = 0; j < K; ++j) {
          // (exp(a_i) - exp(a_j)) / (a_i - a_j) = exp(hi) expm1(-d) / -d,  hi the larger, d = hi - lo >= 0
          const double hi = std::fmax(a[i], a[j]), d = hi - std::fmin(a[i], a[j]);
          const double want = e[i * K + j] * (d == 0.0 ? std::exp(hi) : std::exp(hi) * std::expm1(-d) / -d);
          near(f[i * K + j], want, e[i * K + j], 1e-12, "diagonal F", K, norm);
          near(p[i * K + j], i == j ? std::exp(a[i]) : 0.0, 1.0, 1e-12, "diagonal exp", K, norm);
        }
      // a rate matrix: non-negative off-diagonals, zero row sums, scaled to the 1-norm wanted
      double cs_max = 0.0;
      for (unsigned i = 0; i < K; ++i) {
        double row = 0.0;
        for (unsigned j = 0; j < K; ++j)
          if (j != i) { x[i * K + j] = 0.1 + rng.next(); row += x[i * K + j]; }
        x[i * K + i] = -row;
      }
      for (unsigned j = 0; j < K; ++j) {
        double cs = 0.0;
        for (unsigned i = 0; i < K; ++i) cs += std::fabs(x[i * K + j]);
        cs_max = std::fmax(cs_max, cs);
      }
      for (size_t i = 0; i < n; ++i) x[i] *= norm / cs_max;
      for (unsigned i = 0; i < K; ++i) id[i * K + i] = 1.0;
      block_exp(K, x.data(), x.data(), p.data(), f.data());
      matmul(K, x.data(), p.data(), xp.data());
      for (unsigned i = 0; i < K; ++i) {
        double row = 0.0;
        for (unsigned j = 0; j < K; ++j) {
          near(f[i * K + j], xp[i * K + j], norm, 1e-11, "F(X, X) = X exp(X)", K, norm);
          row += p[i * K + j];
        }
        near(row, 1.0, 1.0, 1e-11, "rows of exp(X) sum to one", K, norm);
      }
      std::vector<double> p2(n), f2(n);
      block_exp(K, x.data(), id.data(), p2.data(), f2.data());
      for (size_t i = 0; i < n; ++i) {
        near(f2[i], p[i], 1.0, 1e-11, "F(X, I) = exp(X)", K, norm);
        near(p2[i], p[i], 1.0, 0.0, "exp(X) does not depend on E", K, norm);
      }
    }
  std::printf("param gradient OK %ld\n", checks);
  return 0;
}
