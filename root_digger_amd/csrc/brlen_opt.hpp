// Maximising lnL over all branch lengths of a rooted tree (rdamd_model_optimize_branch_lengths):
// a projected L-BFGS, memory 8, whose initial metric is the diagonal Newton one.  Pure host logic
// over a callback x -> (lnL, first derivatives, second derivatives) -- no HIP, no model -- so that
// tests/cpp/brlen_opt_check.cpp can drive it on closed-form objectives (as outer_plan.hpp).  The
// library links no optimiser; this is its own.
//
// One iteration at lengths x with value f, gradient g and second derivatives h, in [lo, hi]:
//   1. branch b is FREE unless (x_b = lo and g_b <= 0) or (x_b = hi and g_b >= 0)
//   2. curvature c_b = -h_b if h_b < 0, else |g_b| / max(x_b, lo); 1 where that is 0
//   3. predicted gain G = sum over free b of g_b^2 / (2 c_b); G < atol: stop, converged
//   4. direction d: the L-BFGS two-loop recursion on the free coordinates with H0 = diag(1 / c);
//      g / c, and the history dropped, where that is not an ascent direction
//   5. step x' = clamp(x + lambda d), lambda = 1, 1/2, 1/4, ... (at most 40 halvings), accepted when
//      f(x') >= f(x) + 1e-4 lambda (d.g) -- once lambda < 1e-6, on f(x') >= f(x) alone; no step
//      accepted: stop, not converged
//   6. the pair (s, y) = (x' - x, g - g') is kept only if s.y > 1e-12 |s| |y|
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <deque>
#include <utility>
#include <vector>

namespace rdamd {

struct BrlenOptResult {
  std::vector<double> x, g, h;     // the lengths reached, the derivatives there
  double f_before = 0.0, f_after = 0.0;
  double gain = 0.0;               // the predicted gain G left at x
  unsigned iterations = 0, evaluations = 0;
  bool converged = false;
  std::vector<double> trace;       // f at the start and after every accepted step
};

constexpr unsigned kBrlenOptMemory = 8;

// the free set, the curvatures and the predicted gain at (x, g, h)
inline double brlen_predicted_gain(const std::vector<double> &x, const std::vector<double> &g, const std::vector<double> &h,
                                   double lo, double hi, std::vector<char> *free_out, std::vector<double> *c_out) {
  const size_t n = x.size();
  if (free_out) free_out->assign(n, 0);
  if (c_out) c_out->assign(n, 1.0);
  double gain = 0.0;
  for (size_t b = 0; b < n; ++b) {
    const bool is_free = !((x[b] <= lo && g[b] <= 0.0) || (x[b] >= hi && g[b] >= 0.0));
    double c = h[b] < 0.0 ? -h[b] : std::fabs(g[b]) / std::max(x[b], lo);
    if (!(c > 0.0)) c = 1.0;
    if (free_out) (*free_out)[b] = is_free ? 1 : 0;
    if (c_out) (*c_out)[b] = c;
    if (is_free) gain += g[b] * g[b] / (2.0 * c);
  }
  return gain;
}

// eval(x, &f, g, h) fills the value and both derivative vectors (sized like x) at x in [lo, hi]^n
template <class Eval>
BrlenOptResult optimize_branch_lengths(std::vector<double> x, double lo, double hi, double atol, unsigned max_iters,
                                       Eval &&eval) {
  const size_t n = x.size();
  BrlenOptResult res;
  for (double &v : x) v = std::min(std::max(v, lo), hi);
  std::vector<double> g(n), h(n), x2(n), g2(n), h2(n), d(n), q(n), c;
  std::vector<char> is_free;
  double f = 0.0;
  eval(x, &f, g, h);
  res.evaluations = 1;
  res.f_before = f;
  res.trace.push_back(f);
  struct Pair { std::vector<double> s, y; };
  std::deque<Pair> history;   // oldest first
  const auto dot_free = [&](const std::vector<double> &a, const std::vector<double> &b) {
    double v = 0.0;
    for (size_t i = 0; i < n; ++i)
      if (is_free[i]) v += a[i] * b[i];
    return v;
  };
  for (;;) {
    res.gain = brlen_predicted_gain(x, g, h, lo, hi, &is_free, &c);
    if (res.gain < atol) { res.converged = true; break; }
    if (res.iterations >= max_iters) break;
    // the two-loop recursion for an ASCENT direction: y = g - g' stands for the (negated) gradient change
    for (size_t i = 0; i < n; ++i) q[i] = is_free[i] ? g[i] : 0.0;
    std::vector<double> alpha(history.size()), rho(history.size());
    for (size_t k = history.size(); k-- > 0;) {
      const double sy = dot_free(history[k].s, history[k].y);
      rho[k] = sy > 0.0 ? 1.0 / sy : 0.0;
      alpha[k] = rho[k] * dot_free(history[k].s, q);
      for (size_t i = 0; i < n; ++i)
        if (is_free[i]) q[i] -= alpha[k] * history[k].y[i];
    }
    for (size_t i = 0; i < n; ++i) d[i] = is_free[i] ? q[i] / c[i] : 0.0;
    for (size_t k = 0; k < history.size(); ++k) {
      const double beta = rho[k] * dot_free(history[k].y, d);
      for (size_t i = 0; i < n; ++i)
        if (is_free[i]) d[i] += history[k].s[i] * (alpha[k] - beta);
    }
    double slope = dot_free(d, g);
    if (!(slope > 0.0) || !std::isfinite(slope)) {
      history.clear();
      for (size_t i = 0; i < n; ++i) d[i] = is_free[i] ? g[i] / c[i] : 0.0;
      slope = dot_free(d, g);
    }
    bool accepted = false;
    double lambda = 1.0, f2 = 0.0;
    for (int halvings = 0; halvings <= 40; ++halvings, lambda *= 0.5) {
      for (size_t i = 0; i < n; ++i) x2[i] = std::min(std::max(x[i] + lambda * d[i], lo), hi);
      eval(x2, &f2, g2, h2);
      ++res.evaluations;
      if (!std::isfinite(f2)) continue;
      if (lambda < 1e-6 ? f2 >= f : f2 >= f + 1e-4 * lambda * slope) { accepted = true; break; }
    }
    if (!accepted) break;
    Pair p;
    p.s.resize(n);
    p.y.resize(n);
    double sy = 0.0, ss = 0.0, yy = 0.0;
    for (size_t i = 0; i < n; ++i) {
      p.s[i] = x2[i] - x[i];
      p.y[i] = g[i] - g2[i];
      sy += p.s[i] * p.y[i]; ss += p.s[i] * p.s[i]; yy += p.y[i] * p.y[i];
    }
    if (sy > 1e-12 * std::sqrt(ss) * std::sqrt(yy)) {
      if (history.size() == kBrlenOptMemory) history.pop_front();
      history.push_back(std::move(p));
    }
    x.swap(x2); g.swap(g2); h.swap(h2);
    f = f2;
    ++res.iterations;
    res.trace.push_back(f);
  }
  res.f_after = f;
  res.x = std::move(x); res.g = std::move(g); res.h = std::move(h);
  return res;
}

}  // namespace rdamd
