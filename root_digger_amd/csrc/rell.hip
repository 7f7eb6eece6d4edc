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

// everything the call allocates; released on every way out
struct rell_buffers_t {
  double *rows = nullptr, *table = nullptr, *sums = nullptr, *weights = nullptr, *bp = nullptr, *elw = nullptr;
  unsigned *col2pat = nullptr, *winner = nullptr;
  // the tests' own
  double *partial = nullptr, *lnl = nullptr, *mean = nullptr, *cmax = nullptr, *cbest = nullptr, *rinv = nullptr,
         *spread = nullptr, *tobs = nullptr;
  unsigned *pattern_weights = nullptr, *best = nullptr, *counts = nullptr;   // counts: kh, sh, wsh
  hipStream_t stream = nullptr;
  hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr;
  ~rell_buffers_t() {
    for (void *p : {(void *)rows, (void *)table, (void *)sums, (void *)weights, (void *)bp, (void *)elw,
                    (void *)col2pat, (void *)winner, (void *)partial, (void *)lnl, (void *)mean, (void *)cmax,
                    (void *)cbest, (void *)rinv, (void *)spread, (void *)tobs, (void *)pattern_weights,
                    (void *)best, (void *)counts})
      if (p) (void)hipFree(p);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (t2) (void)hipEventDestroy(t2);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

thread_local double g_last_resample_ms = 0.0, g_last_tests_ms = 0.0, g_last_multiscale_ms = 0.0;

// what rdamd_rell_multiscale allocates; released on every way out
struct multiscale_buffers_t {
  double *rows = nullptr, *table = nullptr, *sums = nullptr, *chunk_max = nullptr;
  unsigned *col2pat = nullptr, *counts = nullptr, *chunk_row = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  ~multiscale_buffers_t() {
    for (void *p : {(void *)rows, (void *)table, (void *)sums, (void *)chunk_max, (void *)col2pat, (void *)counts,
                    (void *)chunk_row})
      if (p) (void)hipFree(p);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

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
  if (n_rows == 0 || n_patterns == 0 || n_replicates == 0) {
    set_error(62, "%s: nothing to resample (%u rows, %u patterns, %u replicates)", who, n_rows, n_patterns,
              n_replicates);
    return RDAMD_FAILURE;
  }
  if (n_scales < 2 || n_scales > rdamd::RELL_MAX_SCALES) {
    set_error(62, "%s: 2 .. %u scales are supported (%u given)", who, rdamd::RELL_MAX_SCALES, n_scales);
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

  const rdamd::rell_shape_t shape = rdamd::rell_shape(n_rows);
  const unsigned chunks = rdamd::rell_row_chunks(shape);
  const size_t cells = (size_t)n_rows * n_patterns, count_cells = (size_t)n_scales * n_rows,
               out_cells = (size_t)n_scales * n_replicates * n_rows,
               chunk_cells = (size_t)n_scales * n_replicates * chunks;
  multiscale_buffers_t d;
  RDAMD_HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&d.t0), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&d.t1), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.rows, cells * sizeof(double)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.table, (size_t)n_patterns * shape.padded * sizeof(double)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.col2pat, (size_t)N * sizeof(unsigned)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.counts, count_cells * sizeof(unsigned)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(d.rows, site_lnl, cells * sizeof(double), hipMemcpyHostToDevice), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(d.col2pat, col2pat.data(), (size_t)N * sizeof(unsigned), hipMemcpyHostToDevice),
                RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemsetAsync(d.counts, 0, count_cells * sizeof(unsigned), d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_transpose(d.rows, n_rows, n_patterns, shape, d.table, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipStreamSynchronize(d.stream), RDAMD_FAILURE);
  (void)hipFree(d.rows);   // (the row-major copy has served: the large shapes need the room)
  d.rows = nullptr;
  if (sums) RDAMD_HIP_TRY(hipMalloc(&d.sums, out_cells * sizeof(double)), RDAMD_FAILURE);
  if (chunks > 1) {
    RDAMD_HIP_TRY(hipMalloc(&d.chunk_max, chunk_cells * sizeof(double)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.chunk_row, chunk_cells * sizeof(unsigned)), RDAMD_FAILURE);
  }
  RDAMD_HIP_TRY(hipEventRecord(d.t0, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_multiscale(d.table, shape, d.col2pat, (unsigned)N, n_rows, n_replicates, scales,
                                              d.counts, d.sums, d.chunk_max, d.chunk_row, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventRecord(d.t1, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipStreamSynchronize(d.stream), RDAMD_FAILURE);
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, d.t0, d.t1) == hipSuccess) g_last_multiscale_ms = ms;
  RDAMD_HIP_TRY(hipMemcpy(counts, d.counts, count_cells * sizeof(unsigned), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (sums) RDAMD_HIP_TRY(hipMemcpy(sums, d.sums, out_cells * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
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
  if (n_rows == 0 || n_patterns == 0 || n_replicates == 0) {
    set_error(62, "%s: nothing to resample (%u rows, %u patterns, %u replicates)", who, n_rows, n_patterns,
              n_replicates);
    return RDAMD_FAILURE;
  }
  if (tests && n_replicates < 2) {
    set_error(62, "%s: the tests need at least 2 replicates", who);
    return RDAMD_FAILURE;
  }
  const bool pairs = tests && (tests->p_wsh || tests->spread);
  if (pairs && n_rows > rdamd::RELL_MAX_PAIR_ROWS) {
    set_error(62, "%s: p_wsh and spread take a table of n_rows^2 doubles; at most %u rows are supported (%u given)",
              who, rdamd::RELL_MAX_PAIR_ROWS, n_rows);
    return RDAMD_FAILURE;
  }
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

  const rdamd::rell_shape_t shape = rdamd::rell_shape(n_rows);
  const size_t cells = (size_t)n_rows * n_patterns, out_cells = (size_t)n_replicates * n_rows;
  rell_buffers_t d;
  RDAMD_HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&d.t0), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&d.t1), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.rows, cells * sizeof(double)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.table, (size_t)n_patterns * shape.padded * sizeof(double)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.col2pat, (size_t)N * sizeof(unsigned)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(d.rows, site_lnl, cells * sizeof(double), hipMemcpyHostToDevice), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(d.col2pat, col2pat.data(), (size_t)N * sizeof(unsigned), hipMemcpyHostToDevice),
                RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_transpose(d.rows, n_rows, n_patterns, shape, d.table, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipStreamSynchronize(d.stream), RDAMD_FAILURE);
  (void)hipFree(d.rows);   // (the row-major copy has served: the large shapes need the room)
  d.rows = nullptr;
  RDAMD_HIP_TRY(hipMalloc(&d.sums, out_cells * sizeof(double)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.weights, out_cells * sizeof(double)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.winner, (size_t)n_replicates * sizeof(unsigned)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.bp, (size_t)n_rows * sizeof(double)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMalloc(&d.elw, (size_t)n_rows * sizeof(double)), RDAMD_FAILURE);
  if (tests) {
    const size_t chunks = std::max(rdamd::rell_chunks(n_patterns), rdamd::rell_chunks(n_replicates));
    RDAMD_HIP_TRY(hipEventCreate(&d.t2), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.pattern_weights, (size_t)n_patterns * sizeof(unsigned)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMemcpy(d.pattern_weights, pattern_weights, (size_t)n_patterns * sizeof(unsigned),
                            hipMemcpyHostToDevice), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.partial, chunks * n_rows * sizeof(double)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.lnl, (size_t)n_rows * sizeof(double)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.mean, (size_t)n_rows * sizeof(double)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.tobs, (size_t)n_rows * sizeof(double)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.cmax, (size_t)n_replicates * sizeof(double)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.cbest, (size_t)n_replicates * sizeof(double)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.best, sizeof(unsigned)), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipMalloc(&d.counts, 3 * (size_t)n_rows * sizeof(unsigned)), RDAMD_FAILURE);
    if (pairs) RDAMD_HIP_TRY(hipMalloc(&d.rinv, (size_t)n_rows * n_rows * sizeof(double)), RDAMD_FAILURE);
    if (tests->spread) RDAMD_HIP_TRY(hipMalloc(&d.spread, (size_t)n_rows * n_rows * sizeof(double)), RDAMD_FAILURE);
  }

  RDAMD_HIP_TRY(hipEventRecord(d.t0, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_sums(d.table, shape, d.col2pat, (unsigned)N, n_rows, n_replicates, seed, d.sums,
                                        d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventRecord(d.t1, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_support(d.sums, n_rows, n_replicates, d.weights, d.winner, d.bp, d.elw, d.stream),
                RDAMD_FAILURE);
  if (tests) {
    unsigned *kh = d.counts, *sh = d.counts + n_rows, *wsh = d.counts + 2 * (size_t)n_rows;
    RDAMD_HIP_TRY(rdamd::launch_rell_totals(d.table, shape.padded, d.pattern_weights, n_patterns, n_rows, d.partial,
                                            d.lnl, d.best, d.stream), RDAMD_FAILURE);
    RDAMD_HIP_TRY(rdamd::launch_rell_means(d.sums, n_rows, n_replicates, d.partial, d.mean, d.stream), RDAMD_FAILURE);
    RDAMD_HIP_TRY(rdamd::launch_rell_kh_sh(d.sums, d.mean, d.lnl, d.best, n_rows, n_replicates, d.cmax, d.cbest, kh,
                                           sh, d.stream), RDAMD_FAILURE);
    if (pairs)
      RDAMD_HIP_TRY(rdamd::launch_rell_spreads(d.sums, d.mean, n_rows, n_replicates, d.rinv, d.spread, d.stream),
                    RDAMD_FAILURE);
    if (tests->p_wsh)
      RDAMD_HIP_TRY(rdamd::launch_rell_wsh(d.sums, d.mean, d.lnl, d.rinv, n_rows, n_replicates, d.tobs, wsh,
                                           d.stream), RDAMD_FAILURE);
    RDAMD_HIP_TRY(hipEventRecord(d.t2, d.stream), RDAMD_FAILURE);
  }
  RDAMD_HIP_TRY(hipStreamSynchronize(d.stream), RDAMD_FAILURE);
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, d.t0, d.t1) == hipSuccess) g_last_resample_ms = ms;
  if (tests) {
    if (hipEventElapsedTime(&ms, d.t1, d.t2) == hipSuccess) g_last_tests_ms = ms;
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
