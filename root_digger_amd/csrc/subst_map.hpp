// Substitution mapping on the host (include/root_digger_amd.h): the count matrices the pre-order
// walk's substitution consumer reads, and rdamd_substitution_counts_from_pair_sums.  Plain host C++
// for any state count, no device and no HIP include: the definitions are in the public header,
// this file follows them with the block exponential of param_gradient.hpp.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

#include "param_gradient.hpp"

namespace rdamd {
namespace smap {

inline bool length_ok(double l) { return l >= 0.0 && std::isfinite(l); }

// out[branch][r] = C = F(X, offdiag(X)), X = rho_r tau_branch Q_(pidx[r]): t^T C L is the expected
// number of substitutions on the branch times the likelihood, multiple hits included.
// q: [rate matrix][K][K]; lengths: [branches]; out: [branches][R][K][K]
inline void count_matrices(unsigned K, unsigned R, const double *q, const unsigned *pidx, const double *rates,
                           const double *lengths, size_t branches, double *out) {
  const size_t n = (size_t)K * K;
  std::vector<double> x(n), e(n), p(n);
  for (size_t b = 0; b < branches; ++b)
    for (unsigned r = 0; r < R; ++r) {
      const double *qm = q + (size_t)pidx[r] * n;
      const double rt = rates[r] * lengths[b];
      for (size_t i = 0; i < n; ++i) {
        x[i] = rt * qm[i];
        e[i] = i % (K + 1) == 0 ? 0.0 : x[i];
      }
      pgrad::block_exp(K, x.data(), e.data(), p.data(), out + (b * R + r) * n);
    }
}

// 0: done; 64: a null input, a state count out of range or a length that is negative or not finite;
// 7: an index out of range
inline int counts_check(unsigned K, unsigned R, unsigned sets, unsigned n_ops, const void *pair, const double *lengths,
                        const double *subst, const double *freqs, const unsigned *pidx, const double *rates,
                        const void *out) {
  if (!pair || !lengths || !subst || !freqs || !pidx || !rates || !out) return 64;
  if (K < 2 || K > 64 || R == 0 || sets == 0) return 64;
  for (size_t b = 0; b < (size_t)n_ops * 2; ++b)
    if (!length_ok(lengths[b])) return 64;
  for (unsigned r = 0; r < R; ++r)
    if (pidx[r] >= sets) return 7;
  return 0;
}

// typed[k][c][i][j], i != j: E = sum_r X_r[i][j] F_r[i][j];  typed[k][c][i][i]: D = tau sum_r F_r[i][i];
// F_r = adjoint[k][c][r] = F(X_r^T, N[k][c][r]) (pgrad::adjoints).  Errors as counts_check.
inline int counts_from_adjoints(unsigned K, unsigned R, unsigned sets, unsigned n_ops, const double *adjoint,
                                const double *lengths, const double *subst, const double *freqs, const unsigned *pidx,
                                const double *rates, double *typed) {
  if (const int e = counts_check(K, R, sets, n_ops, adjoint, lengths, subst, freqs, pidx, rates, typed)) return e;
  const size_t n = (size_t)K * K, nsub = n - K;
  std::vector<double> raw(n), q(sets * n);
  for (unsigned m = 0; m < sets; ++m) pgrad::build_q(K, subst + m * nsub, freqs + (size_t)m * K, raw.data(), q.data() + m * n);
  for (size_t b = 0; b < (size_t)n_ops * 2; ++b) {
    const double tau = lengths[b];
    double *out = typed + b * n;
    for (size_t i = 0; i < n; ++i) out[i] = 0.0;
    for (unsigned r = 0; r < R; ++r) {
      const double *qm = q.data() + (size_t)pidx[r] * n, *f = adjoint + (b * R + r) * n;
      const double rt = rates[r] * tau;
      for (unsigned i = 0; i < K; ++i)
        for (unsigned j = 0; j < K; ++j) out[i * K + j] += i == j ? tau * f[i * K + i] : (rt * qm[i * K + j]) * f[i * K + j];
    }
  }
  return 0;
}

// adjoints on the host, then the assembly
inline int counts_from_pair_sums(unsigned K, unsigned R, unsigned sets, unsigned n_ops, const double *pair,
                                 const double *lengths, const double *subst, const double *freqs, const unsigned *pidx,
                                 const double *rates, double *typed) {
  if (const int e = counts_check(K, R, sets, n_ops, pair, lengths, subst, freqs, pidx, rates, typed)) return e;
  std::vector<double> adjoint((size_t)n_ops * 2 * R * K * K);
  pgrad::adjoints(K, R, sets, n_ops, pair, lengths, subst, freqs, pidx, rates, adjoint.data());
  return counts_from_adjoints(K, R, sets, n_ops, adjoint.data(), lengths, subst, freqs, pidx, rates, typed);
}

}  // namespace smap
}  // namespace rdamd
