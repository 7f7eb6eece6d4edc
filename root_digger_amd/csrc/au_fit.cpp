// rdamd_au_fit (include/root_digger_amd.h): the AU test's weighted least-squares fit of the
// multiscale bootstrap counts of rdamd_rell_multiscale.  Plain host code in double precision; the
// definitions are in the public header, this file follows them line by line.
#include <cmath>
#include <cstdint>

#include "../../include/root_digger_amd.h"
#include "common.hpp"
#include "rell.hpp"

namespace {

constexpr double kSqrt2 = 1.41421356237309504880, kInvSqrt2Pi = 0.39894228040143267794;

double phi(double x) { return kInvSqrt2Pi * std::exp(-0.5 * x * x); }
double upper_tail(double x) { return 0.5 * std::erfc(x / kSqrt2); }

// Phi^-1(p) for 0 < p <= 1/2: Wichura's AS 241 PPND16, then one Halley step on Phi(x) - p with
// Phi from erfc (relative accuracy in the tail)
double quantile_lower(double p) {
  const double q = p - 0.5;
  double x;
  if (std::fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    x = q * (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                 4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
              1.3314166789178437745e+2) * r + 3.3871328727963666080) /
        (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
             2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
          4.2313330701600911252e+1) * r + 1.0);
  } else {
    double r = std::sqrt(-std::log(p));   // (q < 0 here: the lower tail)
    if (r <= 5.0) {
      r -= 1.6;
      x = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
               1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.76949722146069140550) * r +
            4.63033784615654529590) * r + 1.42343711074968357734) /
          (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940) * r +
            2.05319162663775882187) * r + 1.0);
    } else {
      r -= 5.0;
      x = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580) * r +
            5.46378491116411436990) * r + 6.65790464350110377720) /
          (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
            5.99832206555887937690e-1) * r + 1.0);
    }
    x = -x;
  }
  const double e = upper_tail(-x) - p, u = e / phi(x);
  return x - u / (1.0 + 0.5 * x * u);
}

}  // namespace

extern "C" int rdamd_au_fit(const unsigned int *counts, unsigned int n_scales, unsigned int n_rows,
                            const uint64_t *n_draws, uint64_t N, unsigned int n_replicates, double *p_au,
                            double *d_out, double *c_out, double *rss_out, double *se_out, unsigned int *used_out) {
  using rdamd::set_error;
  const char *who = "rdamd_au_fit";
  rdamd::clear_error();
  if (!counts || !n_draws || !p_au) {
    set_error(62, "%s: counts, n_draws and p_au are required", who);
    return RDAMD_FAILURE;
  }
  if (n_scales < 2 || n_scales > rdamd::RELL_MAX_SCALES) {
    set_error(62, "%s: 2 .. %u scales are supported (%u given)", who, rdamd::RELL_MAX_SCALES, n_scales);
    return RDAMD_FAILURE;
  }
  if (n_rows == 0 || n_replicates == 0 || N == 0 || (N >> 32)) {
    set_error(62, "%s: %u rows, %u replicates, %llu columns: at least 1 each and fewer than 2^32 columns", who,
              n_rows, n_replicates, (unsigned long long)N);
    return RDAMD_FAILURE;
  }
  for (unsigned k = 0; k < n_scales; ++k) {
    if (n_draws[k] == 0 || (n_draws[k] >> 32)) {
      set_error(62, "%s: scale %u draws %llu columns; 1 .. 2^32 - 1 are supported", who, k,
                (unsigned long long)n_draws[k]);
      return RDAMD_FAILURE;
    }
    for (unsigned j = 0; j < k; ++j)
      if (n_draws[j] == n_draws[k]) {
        set_error(62, "%s: scales %u and %u both draw %llu columns", who, j, k, (unsigned long long)n_draws[k]);
        return RDAMD_FAILURE;
      }
  }
  for (size_t t = 0; t < (size_t)n_scales * n_rows; ++t)
    if (counts[t] > n_replicates) {
      set_error(62, "%s: a count of %u with %u replicates", who, counts[t], n_replicates);
      return RDAMD_FAILURE;
    }
  // the scale nearest the alignment's own length (the lowest k among equals)
  unsigned nearest = 0;
  const auto away = [&](unsigned k) { return n_draws[k] > N ? n_draws[k] - N : N - n_draws[k]; };
  for (unsigned k = 1; k < n_scales; ++k)
    if (away(k) < away(nearest)) nearest = k;
  double x1[rdamd::RELL_MAX_SCALES], x2[rdamd::RELL_MAX_SCALES], z[rdamd::RELL_MAX_SCALES],
      w[rdamd::RELL_MAX_SCALES];
  bool usable[rdamd::RELL_MAX_SCALES];
  for (unsigned k = 0; k < n_scales; ++k) {
    x1[k] = std::sqrt((double)n_draws[k] / (double)N);
    x2[k] = 1.0 / x1[k];
  }
  const double B = (double)n_replicates;
  for (unsigned i = 0; i < n_rows; ++i) {
    unsigned used = 0;
    double a11 = 0.0, a12 = 0.0, a22 = 0.0, t1 = 0.0, t2 = 0.0;
    for (unsigned k = 0; k < n_scales; ++k) {
      const unsigned n = counts[(size_t)k * n_rows + i];
      usable[k] = n > 0 && n < n_replicates;
      if (!usable[k]) continue;
      ++used;
      // z = -Phi^-1(n / B) = Phi^-1((B - n) / B), on the side that is a lower tail
      const unsigned m = n_replicates - n;
      z[k] = n <= m ? -quantile_lower((double)n / B) : quantile_lower((double)m / B);
      const double p = (double)n / B, f = phi(z[k]);
      w[k] = (f * f * B) / (p * (1.0 - p));
      a11 += w[k] * x1[k] * x1[k];
      a12 += w[k] * x1[k] * x2[k];
      a22 += w[k] * x2[k] * x2[k];
      t1 += w[k] * x1[k] * z[k];
      t2 += w[k] * x2[k] * z[k];
    }
    double d = 0.0, c = 0.0, rss = 0.0, se = 0.0;
    if (used >= 2) {
      const double det = a11 * a22 - a12 * a12;
      d = (a22 * t1 - a12 * t2) / det;
      c = (a11 * t2 - a12 * t1) / det;
      // (two points are fitted exactly: 0, not the rounding residue)
      for (unsigned k = 0; k < n_scales && used > 2; ++k) {
        if (!usable[k]) continue;
        const double e = z[k] - d * x1[k] - c * x2[k];
        rss += w[k] * e * e;
      }
      p_au[i] = upper_tail(d - c);
      se = phi(d - c) * std::sqrt((a11 + a22 + 2.0 * a12) / det);
    } else {
      p_au[i] = (double)counts[(size_t)nearest * n_rows + i] / B;
    }
    if (d_out) d_out[i] = d;
    if (c_out) c_out[i] = c;
    if (rss_out) rss_out[i] = rss;
    if (se_out) se_out[i] = se;
    if (used_out) used_out[i] = used;
  }
  return RDAMD_SUCCESS;
}
