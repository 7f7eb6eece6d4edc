// rdamd_rell_bootstrap / rdamd_rell_column (include/root_digger_amd.h): host side of the RELL
// bootstrap.  Host pointers in and out; the call owns its device memory and its stream.
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
  hipStream_t stream = nullptr;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  ~rell_buffers_t() {
    for (void *p : {(void *)rows, (void *)table, (void *)sums, (void *)weights, (void *)bp, (void *)elw,
                    (void *)col2pat, (void *)winner})
      if (p) (void)hipFree(p);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

thread_local double g_last_resample_ms = 0.0;

}  // namespace

extern "C" {

uint32_t rdamd_rell_column(uint64_t seed, uint64_t b, uint64_t d, uint64_t N) {
  return rdamd::rell_draw(rdamd::rell_key(seed, b), d, (uint32_t)N);
}

double rdamd_rell_last_resample_ms(void) { return g_last_resample_ms; }

int rdamd_rell_bootstrap(const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
                         const unsigned int *pattern_weights, unsigned int n_replicates,
                         uint64_t seed, double *bp, double *elw, double *sums) {
  using rdamd::set_error;
  rdamd::clear_error();
  g_last_resample_ms = 0.0;
  if (!site_lnl || !pattern_weights || !bp || !elw) {
    set_error(62, "rdamd_rell_bootstrap: site_lnl, pattern_weights, bp and elw are required");
    return RDAMD_FAILURE;
  }
  if (n_rows == 0 || n_patterns == 0 || n_replicates == 0) {
    set_error(62, "rdamd_rell_bootstrap: nothing to resample (%u rows, %u patterns, %u replicates)", n_rows,
              n_patterns, n_replicates);
    return RDAMD_FAILURE;
  }
  uint64_t N = 0;
  for (unsigned p = 0; p < n_patterns; ++p) N += pattern_weights[p];
  if (N == 0 || (N >> 32)) {
    set_error(62, "rdamd_rell_bootstrap: the pattern weights sum to %llu columns; 1 .. 2^32 - 1 are supported",
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

  RDAMD_HIP_TRY(hipEventRecord(d.t0, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_sums(d.table, shape, d.col2pat, (unsigned)N, n_rows, n_replicates, seed, d.sums,
                                        d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventRecord(d.t1, d.stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(rdamd::launch_rell_support(d.sums, n_rows, n_replicates, d.weights, d.winner, d.bp, d.elw, d.stream),
                RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipStreamSynchronize(d.stream), RDAMD_FAILURE);
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, d.t0, d.t1) == hipSuccess) g_last_resample_ms = ms;
  RDAMD_HIP_TRY(hipMemcpy(bp, d.bp, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(elw, d.elw, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (sums) RDAMD_HIP_TRY(hipMemcpy(sums, d.sums, out_cells * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

}  // extern "C"
