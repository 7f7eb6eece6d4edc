// Stand-alone checker of csrc/brlen_opt.hpp (tests/test_brlen_opt.py): the projected L-BFGS on
// closed-form concave objectives whose optimum is known.  Per coordinate one of
//   kLog:     k (ln x - x / m)      optimum x = m
//   kDown:    -k x                  optimum at the lower bound
//   kUp:      k x                   optimum at the upper bound
// and, over coordinates 0 and 1 together,
//   pair:     k (ln(x0 + x1) - (x0 + x1) / m): only the sum is identified (the root branch of a
//             reversible model); its diagonal second derivatives are what a caller would hand in.
// For every case: the lnL sequence never decreases, every point evaluated is inside the box, the
// predicted gain recomputed at exit is below atol when converged is reported, the known optimum is
// reached, and max_iters = 1 reports converged = 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "brlen_opt.hpp"

namespace {

long checks = 0;
void check(bool ok, const std::string &what) {
  ++checks;
  if (!ok) { std::printf("FAILED: %s\n", what.c_str()); std::exit(1); }
}

enum Kind { kLog, kDown, kUp };
struct Term { Kind kind; double k, m; };

struct Objective {
  std::vector<Term> terms;
  bool pair = false;   // coordinates 0 and 1 enter through their sum only (their own terms are ignored)
  double pair_k = 0, pair_m = 0;
  double lo, hi;
  long evaluations = 0;
  void operator()(const std::vector<double> &x, double *f, std::vector<double> &g, std::vector<double> &h) {
    ++evaluations;
    double v = 0.0;
    for (size_t i = 0; i < x.size(); ++i) {
      check(x[i] >= lo && x[i] <= hi, "a point outside the box was evaluated");
      if (pair && i < 2) continue;
      const Term &t = terms[i];
      if (t.kind == kLog) { v += t.k * (std::log(x[i]) - x[i] / t.m); g[i] = t.k * (1.0 / x[i] - 1.0 / t.m); h[i] = -t.k / (x[i] * x[i]); }
      else if (t.kind == kDown) { v -= t.k * x[i]; g[i] = -t.k; h[i] = 0.0; }
      else { v += t.k * x[i]; g[i] = t.k; h[i] = 0.0; }
    }
    if (pair) {
      const double s = x[0] + x[1];
      v += pair_k * (std::log(s) - s / pair_m);
      g[0] = g[1] = pair_k * (1.0 / s - 1.0 / pair_m);
      h[0] = h[1] = -pair_k / (s * s);
    }
    *f = v;
  }
};

void run_case(const std::string &name, Objective obj, const std::vector<double> &start, double atol) {
  const size_t n = start.size();
  Objective counted = obj;
  const rdamd::BrlenOptResult r = rdamd::optimize_branch_lengths(start, obj.lo, obj.hi, atol, 500, counted);
  check(r.converged, name + ": did not converge");
  check(r.evaluations == (unsigned)counted.evaluations, name + ": evaluation count");
  check(r.trace.size() == r.iterations + 1 && r.trace.front() == r.f_before && r.trace.back() == r.f_after, name + ": trace");
  for (size_t i = 1; i < r.trace.size(); ++i) check(r.trace[i] >= r.trace[i - 1], name + ": lnL decreased");
  for (size_t i = 0; i < n; ++i) check(r.x[i] >= obj.lo && r.x[i] <= obj.hi, name + ": bounds");
  // G recomputed from a fresh evaluation at the returned point
  std::vector<double> g(n), h(n);
  double f = 0.0;
  obj(r.x, &f, g, h);
  check(f == r.f_after, name + ": f_after is not the value at x");
  check(rdamd::brlen_predicted_gain(r.x, g, h, obj.lo, obj.hi, nullptr, nullptr) < atol, name + ": gain at exit");
  // the known optimum: within what a gain below atol allows (g^2 / (2 k / m^2) < atol  =>  |x - m| < m sqrt(2 atol / k), doubled)
  for (size_t i = obj.pair ? 2 : 0; i < n; ++i) {
    const Term &t = obj.terms[i];
    if (t.kind == kLog && t.m > obj.lo && t.m < obj.hi)
      check(std::fabs(r.x[i] - t.m) <= 2.0 * t.m * std::sqrt(2.0 * atol / t.k) + 1e-12, name + ": interior optimum");
    else if (t.kind == kDown || (t.kind == kLog && t.m <= obj.lo)) check(r.x[i] == obj.lo, name + ": lower bound");
    else check(r.x[i] == obj.hi, name + ": upper bound");
  }
  if (obj.pair) {
    const double s = r.x[0] + r.x[1];
    check(std::fabs(s - obj.pair_m) <= 2.0 * obj.pair_m * std::sqrt(2.0 * atol / obj.pair_k) + 1e-12, name + ": the sum of the pair");
  }
  // one iteration is not enough from here: converged = 0 is reported
  const rdamd::BrlenOptResult one = rdamd::optimize_branch_lengths(start, obj.lo, obj.hi, atol, 1, obj);
  check(!one.converged && one.iterations <= 1, name + ": max_iters = 1 must report converged = 0");
  check(one.f_after >= one.f_before, name + ": max_iters = 1 decreased lnL");
  std::printf("%-28s iterations %3u evaluations %3u gain %.2e\n", name.c_str(), r.iterations, r.evaluations, r.gain);
}

}  // namespace

int main() {
  const double lo = 1e-6, hi = 100.0, atol = 1e-8;
  std::mt19937_64 rng(12);
  std::uniform_real_distribution<double> um(0.01, 2.0), uk(5.0, 500.0), uf(0.3, 3.0);
  for (int rep = 0; rep < 6; ++rep) {
    const size_t n = 4 + 9 * (size_t)rep;
    Objective base;
    base.lo = lo; base.hi = hi;
    for (size_t i = 0; i < n; ++i) base.terms.push_back({kLog, uk(rng), um(rng)});
    std::vector<double> start(n);
    for (size_t i = 0; i < n; ++i) start[i] = base.terms[i].m * uf(rng);
    const std::string tag = " n=" + std::to_string(n);

    run_case("separable" + tag, base, start, atol);

    Objective pair = base;
    pair.pair = true; pair.pair_k = uk(rng); pair.pair_m = um(rng);
    run_case("pair, sum identified" + tag, pair, start, atol);

    Objective low = base;
    low.terms[1] = {kDown, uk(rng), 0.0};
    low.terms[2] = {kLog, uk(rng), 1e-9};     // an optimum below the box
    run_case("optimum at lower bound" + tag, low, start, atol);

    Objective high = base;
    high.terms[0] = {kUp, uk(rng), 0.0};
    high.terms[3] = {kLog, uk(rng), 1e4};     // an optimum above the box
    run_case("optimum at upper bound" + tag, high, start, atol);

    std::vector<double> at_bound = start;
    at_bound[0] = lo; at_bound[1] = hi; at_bound[2] = lo / 10; at_bound[3] = hi * 10;   // (the last two are brought in)
    run_case("start at a bound" + tag, base, at_bound, atol);
    Objective mixed = low;
    mixed.terms[0] = {kUp, uk(rng), 0.0};
    run_case("start at a bound, mixed" + tag, mixed, at_bound, atol);
  }
  std::printf("brlen opt OK %ld\n", checks);
  return 0;
}
