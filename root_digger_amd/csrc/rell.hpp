// RELL bootstrap (include/root_digger_amd.h, rdamd_rell_bootstrap): the draw function shared by
// host and device, and the launchers of kernels_rell.hip.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

namespace rdamd {

// splitmix64's output function on x + golden ratio; all arithmetic mod 2^64
__host__ __device__ inline uint64_t rell_sm(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the key of replicate b, and the column draw d of that replicate resamples (N < 2^32 columns)
__host__ __device__ inline uint64_t rell_key(uint64_t seed, uint64_t b) { return rell_sm(seed ^ rell_sm(b)); }
__host__ __device__ inline uint32_t rell_draw(uint64_t key, uint64_t d, uint32_t N) {
  return (uint32_t)(((rell_sm(key + d) >> 32) * (uint64_t)N) >> 32);
}

// How the rows (candidate roots) of one replicate are laid over a wave: `lanes` lanes per replicate
// (8, 16, 32 or 64; 64 / lanes replicates share a wave), `per_lane` consecutive rows per lane
// (1, 2 or 4; more than 1 only with 64 lanes), rows padded to `padded` (a multiple of
// lanes * per_lane; several row chunks per replicate beyond 256 rows).
struct rell_shape_t {
  unsigned lanes, per_lane, padded;
};
rell_shape_t rell_shape(unsigned n_rows);

// d_rows[n_rows][n_patterns] -> d_table[n_patterns][shape.padded], padding rows zero
hipError_t launch_rell_transpose(const double *d_rows, unsigned n_rows, unsigned n_patterns,
                                 const rell_shape_t &shape, double *d_table, hipStream_t stream);
// d_sums[n_replicates][n_rows]
hipError_t launch_rell_sums(const double *d_table, const rell_shape_t &shape, const unsigned *d_col2pat,
                            unsigned n_columns, unsigned n_rows, unsigned n_replicates, uint64_t seed,
                            double *d_sums, hipStream_t stream);
// d_weights[n_replicates][n_rows] (a replicate's likelihood weights), d_winner[n_replicates], then
// d_bp[n_rows], d_elw[n_rows]
hipError_t launch_rell_support(const double *d_sums, unsigned n_rows, unsigned n_replicates,
                               double *d_weights, unsigned *d_winner, double *d_bp, double *d_elw,
                               hipStream_t stream);

}  // namespace rdamd
