// rdamd_gradient_from_pair_sums (include/root_digger_amd.h): the exact gradient of lnL in the
// substitution rates, frequencies, category rates and weights from the pair sums of the pre-order
// walk.  Plain host C++ for any state count, no device and no HIP include: the definitions are in
// the public header, this file follows them.
//
// block_exp is the arithmetic of expm_k4.hpp carried one block further: scaling and squaring on the
// pair (exp(X), F(X, E)), F(X, E) = integral_0^1 exp(xX) E exp((1 - x)X) dx, the top-right block of
// exp([[X, E], [0, X]]).
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace rdamd {
namespace pgrad {

constexpr int kBlockTaylorTerms = 18;   // ||X / 2^s||_1 <= 1/4: the terms left out are below 4^-19 / 19!

// c = a b, K x K row-major
inline void matmul(unsigned K, const double *a, const double *b, double *c) {
  for (unsigned i = 0; i < K; ++i)
    for (unsigned j = 0; j < K; ++j) {
      double s = 0.0;
      for (unsigned l = 0; l < K; ++l) s += a[i * K + l] * b[l * K + j];
      c[i * K + j] = s;
    }
}

// the scaling of block_exp: ||x||_1 halved *s times until it is at most 1/4, *scale = 2^-*s.  The
// device route of rdamd_pair_sum_adjoints is handed these two numbers, so its trip count is the host's.
inline void block_scaling(unsigned K, const double *x, int *s_out, double *scale_out) {
  double norm = 0.0;
  for (unsigned j = 0; j < K; ++j) {
    double cs = 0.0;
    for (unsigned i = 0; i < K; ++i) cs += std::fabs(x[i * K + j]);
    norm = std::fmax(norm, cs);
  }
  int s = 0;
  double scale = 1.0;
  while (norm * scale > 0.25 && s < 60) { scale *= 0.5; ++s; }
  *s_out = s;
  *scale_out = scale;
}

// p = exp(x), f = F(x, e); all K x K row-major, p and f distinct from x and e
inline void block_exp(unsigned K, const double *x, const double *e, double *p, double *f) {
  const size_t n = (size_t)K * K;
  int s = 0;
  double scale = 1.0;
  block_scaling(K, x, &s, &scale);
  std::vector<double> xs(n), es(n), term(n), d(n), t1(n), t2(n);
  for (size_t i = 0; i < n; ++i) { xs[i] = x[i] * scale; es[i] = e[i] * scale; }
  // term = X^(k-1) / (k-1)!, d = D_(k-1);  D_k = (X D_(k-1) + E X^(k-1)/(k-1)!) / k
  for (size_t i = 0; i < n; ++i) { term[i] = p[i] = (i % (K + 1) == 0) ? 1.0 : 0.0; d[i] = f[i] = 0.0; }
  for (int k = 1; k <= kBlockTaylorTerms; ++k) {
    const double inv = 1.0 / (double)k;
    matmul(K, xs.data(), d.data(), t1.data());
    matmul(K, es.data(), term.data(), t2.data());
    for (size_t i = 0; i < n; ++i) { d[i] = (t1[i] + t2[i]) * inv; f[i] += d[i]; }
    matmul(K, term.data(), xs.data(), t1.data());
    for (size_t i = 0; i < n; ++i) { term[i] = t1[i] * inv; p[i] += term[i]; }
  }
  // (P, F) -> (P P, P F + F P)
  for (int k = 0; k < s; ++k) {
    matmul(K, p, f, t1.data());
    matmul(K, f, p, t2.data());
    for (size_t i = 0; i < n; ++i) f[i] = t1[i] + t2[i];
    matmul(K, p, p, t1.data());
    for (size_t i = 0; i < n; ++i) p[i] = t1[i];
  }
}

// raw (zero row sums, raw_ij = s_ij pi_j) and mu = -sum_i pi_i raw_ii; q = raw / mu
inline double build_q(unsigned K, const double *subst, const double *pi, double *raw, double *q) {
  size_t at = 0;
  double mu = 0.0;
  for (unsigned i = 0; i < K; ++i) {
    double row = 0.0;
    for (unsigned j = 0; j < K; ++j)
      if (j != i) { raw[i * K + j] = subst[at++] * pi[j]; row += raw[i * K + j]; }
    raw[i * K + i] = -row;
    mu += pi[i] * row;
  }
  for (size_t i = 0; i < (size_t)K * K; ++i) q[i] = raw[i] / mu;
  return mu;
}

// The adjoints of the pair sums, the loop both assemblies share: adjoint[branch][r] =
// F((rho_r tau Q_m)^T, N[branch][r]), m = pidx[r], one block exponential each.  pair and adjoint:
// [n_ops][2][R][K][K].  The arguments are the caller's to check.
inline void adjoints(unsigned K, unsigned R, unsigned sets, unsigned n_ops, const double *pair, const double *lengths,
                     const double *subst, const double *freqs, const unsigned *pidx, const double *rates, double *adjoint) {
  const size_t n = (size_t)K * K, nsub = n - K;
  std::vector<double> raw(n), q(sets * n), xt(n), p(n);
  for (unsigned m = 0; m < sets; ++m) build_q(K, subst + m * nsub, freqs + (size_t)m * K, raw.data(), q.data() + m * n);
  for (size_t b = 0; b < (size_t)n_ops * 2; ++b)
    for (unsigned r = 0; r < R; ++r) {
      const double *qm = q.data() + (size_t)pidx[r] * n;
      const double rt = rates[r] * lengths[b];
      for (unsigned i = 0; i < K; ++i)
        for (unsigned j = 0; j < K; ++j) xt[i * K + j] = rt * qm[j * K + i];   // (rho tau Q)^T
      block_exp(K, xt.data(), pair + (b * R + r) * n, p.data(), adjoint + (b * R + r) * n);
    }
}

// 0: done; 64: a null input or a state count out of range; 7: an index out of range
inline int gradient_check(unsigned K, unsigned R, unsigned sets, const void *pair, const double *root, const double *cat,
                          const double *lengths, const double *subst, const double *freqs, const unsigned *pidx,
                          const unsigned *fidx, const double *rates, const double *weights) {
  if (!pair || !root || !cat || !lengths || !subst || !freqs || !pidx || !fidx || !rates || !weights) return 64;
  if (K < 2 || K > 64 || R == 0 || sets == 0) return 64;
  for (unsigned r = 0; r < R; ++r)
    if (pidx[r] >= sets || fidx[r] >= sets) return 7;
  return 0;
}

// The gradient from the adjoints: gq += rho tau F and d_rates += tau <F, Q> over the branches, the
// root term and the chain rule through Q = raw / mu.  Errors as gradient_check.
inline int gradient_from_adjoints(unsigned K, unsigned R, unsigned sets, unsigned n_ops, const double *adjoint,
                                  const double *root, const double *cat, const double *lengths, const double *subst,
                                  const double *freqs, const unsigned *pidx, const unsigned *fidx, const double *rates,
                                  const double *weights, double *d_subst, double *d_freqs, double *d_rates,
                                  double *d_weights) {
  if (const int e = gradient_check(K, R, sets, adjoint, root, cat, lengths, subst, freqs, pidx, fidx, rates, weights)) return e;
  const size_t n = (size_t)K * K, nsub = n - K;
  std::vector<double> raw(sets * n), q(sets * n), mu(sets), gq(sets * n, 0.0);
  for (unsigned m = 0; m < sets; ++m)
    mu[m] = build_q(K, subst + m * nsub, freqs + (size_t)m * K, raw.data() + m * n, q.data() + m * n);
  if (d_rates)
    for (unsigned r = 0; r < R; ++r) d_rates[r] = 0.0;
  for (size_t b = 0; b < (size_t)n_ops * 2; ++b) {
    const double tau = lengths[b];
    for (unsigned r = 0; r < R; ++r) {
      const unsigned m = pidx[r];
      const double *qm = q.data() + m * n, *f = adjoint + (b * R + r) * n;
      const double rt = rates[r] * tau;
      double fq = 0.0;
      for (size_t i = 0; i < n; ++i) { gq[m * n + i] += rt * f[i]; fq += f[i] * qm[i]; }
      if (d_rates) d_rates[r] += tau * fq;   // <N, tau Q P> = tau <F, Q>, the adjoint property
    }
  }
  if (d_freqs) {
    for (size_t i = 0; i < (size_t)sets * K; ++i) d_freqs[i] = 0.0;
    for (unsigned r = 0; r < R; ++r)
      for (unsigned i = 0; i < K; ++i) d_freqs[(size_t)fidx[r] * K + i] += root[(size_t)r * K + i];
  }
  // the chain rule through Q = raw / mu, all K K entries of G free
  for (unsigned m = 0; m < sets; ++m) {
    const double *g = gq.data() + m * n, *qm = q.data() + m * n, *rw = raw.data() + m * n;
    const double *pi = freqs + (size_t)m * K, *sub = subst + m * nsub;
    double h = 0.0;   // <G, Q>: d lnL / d mu = -h / mu
    for (size_t i = 0; i < n; ++i) h += g[i] * qm[i];
    size_t at = 0;
    for (unsigned a = 0; a < K; ++a) {
      for (unsigned b = 0; b < K; ++b) {
        if (a == b) continue;
        const double graw = ((g[a * K + b] - g[a * K + a]) - h * pi[a]) / mu[m];   // d lnL / d raw_ab
        if (d_subst) d_subst[m * nsub + at] = graw * pi[b];
        if (d_freqs) d_freqs[(size_t)m * K + b] += graw * sub[at];
        ++at;
      }
      if (d_freqs) d_freqs[(size_t)m * K + a] += h / mu[m] * rw[a * K + a];   // mu's own pi_a: d mu / d pi_a = -raw_aa
    }
  }
  if (d_weights)
    for (unsigned r = 0; r < R; ++r) d_weights[r] = cat[r];
  return 0;
}

// adjoints on the host, then the assembly
inline int gradient_from_pair_sums(unsigned K, unsigned R, unsigned sets, unsigned n_ops, const double *pair,
                                   const double *root, const double *cat, const double *lengths, const double *subst,
                                   const double *freqs, const unsigned *pidx, const unsigned *fidx, const double *rates,
                                   const double *weights, double *d_subst, double *d_freqs, double *d_rates,
                                   double *d_weights) {
  if (const int e = gradient_check(K, R, sets, pair, root, cat, lengths, subst, freqs, pidx, fidx, rates, weights)) return e;
  std::vector<double> adjoint((size_t)n_ops * 2 * R * K * K);
  adjoints(K, R, sets, n_ops, pair, lengths, subst, freqs, pidx, rates, adjoint.data());
  return gradient_from_adjoints(K, R, sets, n_ops, adjoint.data(), root, cat, lengths, subst, freqs, pidx, fidx, rates,
                                weights, d_subst, d_freqs, d_rates, d_weights);
}

}  // namespace pgrad
}  // namespace rdamd
