// rdamd_rell_bootstrap / rdamd_rell_tests / rdamd_rell_column (include/root_digger_amd.h): host
// side of the RELL bootstrap and of the KH / SH / weighted-SH tests made from its sums.  Host
// pointers in and out; the call owns its device memory and its stream.  Both calls are one
// function: the tests are what follows the bootstrap's launches on the same stream.
// rdamd_rell_multiscale: the same conventions for the bootstrap at several replicate lengths
// (the AU test's counts; the fit itself is au_fit.cpp).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/root_digger_amd.h"
#include "common.hpp"
#include "rell.hpp"

namespace {

thread_local double g_last_resample_ms = 0.0, g_last_tests_ms = 0.0, g_last_multiscale_ms = 0.0;

// A call's device allocations, its stream and its events: released on every way out.
template <class T> struct device_array_t {
  T *p = nullptr;
  device_array_t() = default;
  device_array_t(const device_array_t &) = delete;
  device_array_t &operator=(const device_array_t &) = delete;
  ~device_array_t() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) { return hipMalloc((void **)&p, count * sizeof(T)); }
  operator T *() const { return p; }
};
template <class T, hipError_t (*DESTROY)(T)> struct owned_t {
  T h = nullptr;
  owned_t() = default;
  owned_t(const owned_t &) = delete;
  owned_t &operator=(const owned_t &) = delete;
  ~owned_t() { if (h) (void)DESTROY(h); }
  operator T() const { return h; }
};
using stream_t = owned_t<hipStream_t, hipStreamDestroy>;
using event_t = owned_t<hipEvent_t, hipEventDestroy>;

// What both calls resample from: the padded table [n_patterns][shape.padded] and the column ->
// pattern map of the N columns on the device, the call's stream and the events around its
// resampling launches.  (Members are destroyed last first: the buffers, the events, the stream.)
struct rell_staged_t {
  stream_t stream;
  event_t t0, t1;
  device_array_t<double> table;
  device_array_t<unsigned> col2pat;
  rdamd::rell_shape_t shape;
  unsigned N;
};

// The checks both calls share (own_checks() -> false: the call's own have failed and set the
// error; they come after "nothing to resample", before the column count), the upload and the
// transposition.  The row-major copy is gone when this returns: the large shapes need the room for
// what the caller allocates next.
template <class F>
int rell_stage(const char *who, const double *site_lnl, unsigned n_rows, unsigned n_patterns,
               const unsigned *pattern_weights, unsigned n_replicates, F &&own_checks, rell_staged_t &s) {
  using rdamd::set_error;
  if (n_rows == 0 || n_patterns == 0 || n_replicates == 0) {
    set_error(62, "%s: nothing to resample (%u rows, %u patterns, %u replicates)", who, n_rows, n_patterns,
              n_replicates);
    return RDAMD_FAILURE;
  }
  if (!own_checks()) return RDAMD_FAILURE;
  uint64_t N = 0;
  for (unsigned p = 0; p < n_patterns; ++p) N += pattern_weights[p];
  if (N == 0 || (N >> 32)) {
    set_error(62, "%s: the pattern weights sum to %llu columns; 1 .. 2^32 - 1 are supported", who,
              (unsigned long long)N);
    return RDAMD_FAILURE;
  }
  // pattern p owns pattern_weights[p] consecutive columns
  std::vector<unsigned> col2pat;
  col2pat.reserve((size_t)N);
  for (unsigned p = 0; p < n_patterns; ++p) col2pat.insert(col2pat.end(), pattern_weights[p], p);

  s.shape = rdamd::rell_shape(n_rows);
  s.N = (unsigned)N;
  const size_t cells = (size_t)n_rows * n_patterns;
  device_array_t<double> rows;
  RDAMD_HIP_TRY(hipStreamCreateWithFlags(&s.stream.h, hipStreamNonBlocking), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&s.t0.h), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&s.t1.h), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rows.alloc(cells), RDAMD_FAILURE);
  RDAMD_HIP_TRY(s.table.alloc((size_t)n_patterns * s.shape.padded), RDAMD_FAILURE);
  RDAMD_HIP_TRY(s.col2pat.alloc((size_t)N), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(rows, site_lnl, cells * sizeof(double), hipMemcpyHostToDevice), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(s.col2pat, col2pat.data(), (size_t)N * sizeof(unsigned), hipMemcpyHostToDevice),
                RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_transpose(rows, n_rows, n_patterns, s.shape, s.table, s.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipStreamSynchronize(s.stream), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

// what rdamd_rell_tests returns beyond the bootstrap's (host pointers; lnl, p_wsh, spread may be NULL)
struct rell_tests_out_t {
  double *lnl, *p_kh, *p_sh, *p_wsh, *spread;
};

int rell_run(const char *who, const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
             const unsigned int *pattern_weights, unsigned int n_replicates, uint64_t seed, double *bp, double *elw,
             double *sums, const rell_tests_out_t *tests);

}  // namespace

extern "C" {

uint32_t rdamd_rell_column(uint64_t seed, uint64_t b, uint64_t d, uint64_t N) {
  return rdamd::rell_draw(rdamd::rell_key(seed, b), d, (uint32_t)N);
}

double rdamd_rell_last_resample_ms(void) { return g_last_resample_ms; }
double rdamd_rell_last_tests_ms(void) { return g_last_tests_ms; }
double rdamd_rell_last_multiscale_ms(void) { return g_last_multiscale_ms; }

uint64_t rdamd_rell_scale_seed(uint64_t seed, uint64_t k) { return rdamd::rell_scale_seed(seed, k); }

int rdamd_rell_multiscale(const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
                          const unsigned int *pattern_weights, unsigned int n_scales, const uint64_t *n_draws,
                          unsigned int n_replicates, uint64_t seed, unsigned int *counts, double *sums) {
  using rdamd::set_error;
  const char *who = "rdamd_rell_multiscale";
  rdamd::clear_error();
  g_last_multiscale_ms = 0.0;
  if (!site_lnl || !pattern_weights || !n_draws || !counts) {
    set_error(62, "%s: site_lnl, pattern_weights, n_draws and counts are required", who);
    return RDAMD_FAILURE;
  }
  const auto own_checks = [&] {
    if (n_scales < 2 || n_scales > rdamd::RELL_MAX_SCALES) {
      set_error(62, "%s: 2 .. %u scales are supported (%u given)", who, rdamd::RELL_MAX_SCALES, n_scales);
      return false;
    }
    for (unsigned k = 0; k < n_scales; ++k) {
      if (n_draws[k] == 0 || (n_draws[k] >> 32)) {
        set_error(62, "%s: scale %u draws %llu columns; 1 .. 2^32 - 1 are supported", who, k,
                  (unsigned long long)n_draws[k]);
        return false;
      }
      for (unsigned j = 0; j < k; ++j)
        if (n_draws[j] == n_draws[k]) {
          set_error(62, "%s: scales %u and %u both draw %llu columns", who, j, k, (unsigned long long)n_draws[k]);
          return false;
        }
    }
    return true;
  };
  rell_staged_t st;
  if (rell_stage(who, site_lnl, n_rows, n_patterns, pattern_weights, n_replicates, own_checks, st) != RDAMD_SUCCESS)
    return RDAMD_FAILURE;
  // longest first; equal lengths do not occur
  rdamd::rell_scales_t scales;
  scales.n = n_scales;
  std::vector<unsigned> order(n_scales);
  for (unsigned k = 0; k < n_scales; ++k) order[k] = k;
  std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return n_draws[a] > n_draws[b]; });
  for (unsigned s = 0; s < rdamd::RELL_MAX_SCALES; ++s) {
    const bool on = s < n_scales;
    scales.draws[s] = on ? (unsigned)n_draws[order[s]] : 0u;
    scales.index[s] = on ? order[s] : 0u;
    scales.seed[s] = on ? rdamd::rell_scale_seed(seed, order[s]) : 0u;
  }

  const unsigned chunks = rdamd::rell_row_chunks(st.shape);
  const size_t count_cells = (size_t)n_scales * n_rows, out_cells = (size_t)n_scales * n_replicates * n_rows,
               chunk_cells = (size_t)n_scales * n_replicates * chunks;
  device_array_t<double> d_sums, d_chunk_max;
  device_array_t<unsigned> d_counts, d_chunk_row;
  RDAMD_HIP_TRY(d_counts.alloc(count_cells), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemsetAsync(d_counts, 0, count_cells * sizeof(unsigned), st.stream), RDAMD_FAILURE);
  if (sums) RDAMD_HIP_TRY(d_sums.alloc(out_cells), RDAMD_FAILURE);
  if (chunks > 1) {
    RDAMD_HIP_TRY(d_chunk_max.alloc(chunk_cells), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d_chunk_row.alloc(chunk_cells), RDAMD_FAILURE);
  }
  RDAMD_HIP_TRY(hipEventRecord(st.t0, st.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_multiscale(st.table, st.shape, st.col2pat, st.N, n_rows, n_replicates, scales,
                                              d_counts, d_sums, d_chunk_max, d_chunk_row, st.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventRecord(st.t1, st.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipStreamSynchronize(st.stream), RDAMD_FAILURE);
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, st.t0, st.t1) == hipSuccess) g_last_multiscale_ms = ms;
  RDAMD_HIP_TRY(hipMemcpy(counts, d_counts, count_cells * sizeof(unsigned), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (sums) RDAMD_HIP_TRY(hipMemcpy(sums, d_sums, out_cells * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

int rdamd_rell_bootstrap(const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
                         const unsigned int *pattern_weights, unsigned int n_replicates,
                         uint64_t seed, double *bp, double *elw, double *sums) {
  return rell_run("rdamd_rell_bootstrap", site_lnl, n_rows, n_patterns, pattern_weights, n_replicates, seed, bp, elw,
                  sums, nullptr);
}

int rdamd_rell_tests(const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
                     const unsigned int *pattern_weights, unsigned int n_replicates, uint64_t seed,
                     double *lnl, double *bp, double *elw, double *p_kh, double *p_sh, double *p_wsh,
                     double *sums, double *spread) {
  const rell_tests_out_t tests = {lnl, p_kh, p_sh, p_wsh, spread};
  return rell_run("rdamd_rell_tests", site_lnl, n_rows, n_patterns, pattern_weights, n_replicates, seed, bp, elw,
                  sums, &tests);
}

}  // extern "C"

namespace {

int rell_run(const char *who, const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
             const unsigned int *pattern_weights, unsigned int n_replicates, uint64_t seed, double *bp, double *elw,
             double *sums, const rell_tests_out_t *tests) {
  using rdamd::set_error;
  rdamd::clear_error();
  g_last_resample_ms = 0.0;
  if (tests) g_last_tests_ms = 0.0;
  if (!site_lnl || !pattern_weights || !bp || !elw) {
    set_error(62, "%s: site_lnl, pattern_weights, bp and elw are required", who);
    return RDAMD_FAILURE;
  }
  if (tests && (!tests->p_kh || !tests->p_sh)) {
    set_error(62, "%s: p_kh and p_sh are required", who);
    return RDAMD_FAILURE;
  }
  const bool pairs = tests && (tests->p_wsh || tests->spread);
  const auto own_checks = [&] {
    if (tests && n_replicates < 2) {
      set_error(62, "%s: the tests need at least 2 replicates", who);
      return false;
    }
    if (pairs && n_rows > rdamd::RELL_MAX_PAIR_ROWS) {
      set_error(62, "%s: p_wsh and spread take a table of n_rows^2 doubles; at most %u rows are supported (%u given)",
                who, rdamd::RELL_MAX_PAIR_ROWS, n_rows);
      return false;
    }
    return true;
  };
  rell_staged_t st;
  if (rell_stage(who, site_lnl, n_rows, n_patterns, pattern_weights, n_replicates, own_checks, st) != RDAMD_SUCCESS)
    return RDAMD_FAILURE;
  const hipStream_t stream = st.stream;
  const size_t out_cells = (size_t)n_replicates * n_rows;
  struct {
    device_array_t<double> sums, weights, bp, elw;
    device_array_t<unsigned> winner;
    // the tests' own
    device_array_t<double> partial, lnl, mean, cmax, cbest, rinv, spread, tobs;
    device_array_t<unsigned> pattern_weights, best, counts;   // counts: kh, sh, wsh
    event_t t2;
  } d;
  RDAMD_HIP_TRY(d.sums.alloc(out_cells), RDAMD_FAILURE);
  RDAMD_HIP_TRY(d.weights.alloc(out_cells), RDAMD_FAILURE);
  RDAMD_HIP_TRY(d.winner.alloc(n_replicates), RDAMD_FAILURE);
  RDAMD_HIP_TRY(d.bp.alloc(n_rows), RDAMD_FAILURE);
  RDAMD_HIP_TRY(d.elw.alloc(n_rows), RDAMD_FAILURE);
  if (tests) {
    const size_t chunks = std::max(rdamd::rell_chunks(n_patterns), rdamd::rell_chunks(n_replicates));
    RDAMD_HIP_TRY(hipEventCreate(&d.t2.h), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.pattern_weights.alloc(n_patterns), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMemcpy(d.pattern_weights, pattern_weights, (size_t)n_patterns * sizeof(unsigned),
                            hipMemcpyHostToDevice), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.partial.alloc(chunks * n_rows), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.lnl.alloc(n_rows), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.mean.alloc(n_rows), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.tobs.alloc(n_rows), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.cmax.alloc(n_replicates), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.cbest.alloc(n_replicates), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.best.alloc(1), RDAMD_FAILURE);
    RDAMD_HIP_TRY(d.counts.alloc(3 * (size_t)n_rows), RDAMD_FAILURE);
    if (pairs) RDAMD_HIP_TRY(d.rinv.alloc((size_t)n_rows * n_rows), RDAMD_FAILURE);
    if (tests->spread) RDAMD_HIP_TRY(d.spread.alloc((size_t)n_rows * n_rows), RDAMD_FAILURE);
  }

  RDAMD_HIP_TRY(hipEventRecord(st.t0, stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_sums(st.table, st.shape, st.col2pat, st.N, n_rows, n_replicates, seed, d.sums,
                                        stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventRecord(st.t1, stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_support(d.sums, n_rows, n_replicates, d.weights, d.winner, d.bp, d.elw, stream),
                RDAMD_FAILURE);
  if (tests) {
    unsigned *kh = d.counts, *sh = d.counts + n_rows, *wsh = d.counts + 2 * (size_t)n_rows;
    RDAMD_HIP_TRY(rdamd::launch_rell_totals(st.table, st.shape.padded, d.pattern_weights, n_patterns, n_rows, d.partial,
                                            d.lnl, d.best, stream), RDAMD_FAILURE);
    RDAMD_HIP_TRY(rdamd::launch_rell_means(d.sums, n_rows, n_replicates, d.partial, d.mean, stream), RDAMD_FAILURE);
    RDAMD_HIP_TRY(rdamd::launch_rell_kh_sh(d.sums, d.mean, d.lnl, d.best, n_rows, n_replicates, d.cmax, d.cbest, kh,
                                           sh, stream), RDAMD_FAILURE);
    if (pairs)
      RDAMD_HIP_TRY(rdamd::launch_rell_spreads(d.sums, d.mean, n_rows, n_replicates, d.rinv, d.spread, stream),
                    RDAMD_FAILURE);
    if (tests->p_wsh)
      RDAMD_HIP_TRY(rdamd::launch_rell_wsh(d.sums, d.mean, d.lnl, d.rinv, n_rows, n_replicates, d.tobs, wsh,
                                           stream), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipEventRecord(d.t2, stream), RDAMD_FAILURE);
  }
  RDAMD_HIP_TRY(hipStreamSynchronize(stream), RDAMD_FAILURE);
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, st.t0, st.t1) == hipSuccess) g_last_resample_ms = ms;
  if (tests) {
    if (hipEventElapsedTime(&ms, st.t1, d.t2) == hipSuccess) g_last_tests_ms = ms;
    std::vector<unsigned> counts(3 * (size_t)n_rows);
    RDAMD_HIP_TRY(hipMemcpy(counts.data(), d.counts, counts.size() * sizeof(unsigned), hipMemcpyDeviceToHost),
                  RDAMD_FAILURE);
    for (unsigned i = 0; i < n_rows; ++i) {
      tests->p_kh[i] = (double)counts[i] / (double)n_replicates;
      tests->p_sh[i] = (double)counts[n_rows + i] / (double)n_replicates;
      if (tests->p_wsh) tests->p_wsh[i] = (double)counts[2 * (size_t)n_rows + i] / (double)n_replicates;
    }
    if (tests->lnl)
      RDAMD_HIP_TRY(hipMemcpy(tests->lnl, d.lnl, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost),
                    RDAMD_FAILURE);
    if (tests->spread)
      RDAMD_HIP_TRY(hipMemcpy(tests->spread, d.spread, (size_t)n_rows * n_rows * sizeof(double),
                              hipMemcpyDeviceToHost), RDAMD_FAILURE);
  }
  RDAMD_HIP_TRY(hipMemcpy(bp, d.bp, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(elw, d.elw, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (sums) RDAMD_HIP_TRY(hipMemcpy(sums, d.sums, out_cells * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

}  // namespace
