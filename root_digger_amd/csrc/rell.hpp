// RELL bootstrap (include/root_digger_amd.h, rdamd_rell_bootstrap and rdamd_rell_multiscale): the
// draw function shared by host and device, the tie-break of a replicate's winner shared by the
// kernels, and the launchers of kernels_rell.hip and kernels_rell_tests.hip.
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

#ifdef __HIPCC__
// A running (largest value, the lowest row that has it); RELL_NO_ROW: no row yet, the value means nothing.
constexpr unsigned RELL_NO_ROW = 0xffffffffu;
// One butterfly step: this lane's pair merged with lane ^ off's.  The larger value wins, among
// equals the lowest row, an empty pair never.
__device__ __forceinline__ void rell_merge_best(double &best, unsigned &at, int off) {
  const double ob = __shfl_xor(best, off);
  const unsigned oa = (unsigned)__shfl_xor((int)at, off);
  if (oa != RELL_NO_ROW && (at == RELL_NO_ROW || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
}
#endif

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

// ---- multiscale bootstrap (rdamd_rell_multiscale; kernels_rell.hip: launch_rell_sums' kernel
// template with a scale per wave and the winner found in place)
constexpr unsigned RELL_MAX_SCALES = 64;
// seed of scale k (rdamd_rell_scale_seed)
inline uint64_t rell_scale_seed(uint64_t seed, uint64_t k) { return rell_sm(seed + k + 1); }
// The scales of one launch in the order they are issued, longest first: `draws` draws per
// replicate, replicate b's key is rell_key(seed, b), results go to scale `index` of the outputs.
struct rell_scales_t {
  unsigned n;
  unsigned draws[RELL_MAX_SCALES], index[RELL_MAX_SCALES];
  uint64_t seed[RELL_MAX_SCALES];
};
// row chunks of one replicate: 1 up to 256 rows (one wave holds a replicate)
inline unsigned rell_row_chunks(const rell_shape_t &shape) { return shape.padded / (shape.lanes * shape.per_lane); }
// d_counts[scales.n][n_rows] += replicates won (the caller zeroes it; integer atomics),
// d_sums[scales.n][n_replicates][n_rows] unless NULL.  With more than one row chunk
// d_chunk_max / d_chunk_row hold scales.n * n_replicates * chunks entries each: the chunks'
// (largest sum, its lowest row), from which a second kernel picks; otherwise they may be NULL.
hipError_t launch_rell_multiscale(const double *d_table, const rell_shape_t &shape, const unsigned *d_col2pat,
                                  unsigned n_columns, unsigned n_rows, unsigned n_replicates,
                                  const rell_scales_t &scales, unsigned *d_counts, double *d_sums,
                                  double *d_chunk_max, unsigned *d_chunk_row, hipStream_t stream);

// ---- KH / SH / weighted-SH tests of the rows (rdamd_rell_tests; kernels_rell_tests.hip).
// c[b][i] = d_sums[b][i] - d_mean[i] is never stored: every kernel subtracts as it loads.
// All counts are unsigned integers (integer atomics only); no result depends on a launch shape.

// Sums over the leading axis are made in chunks of RELL_CHUNK entries: d_partial holds
// rell_chunks(K) * n_rows doubles for a sum over K entries.
constexpr unsigned RELL_CHUNK = 512;
inline unsigned rell_chunks(unsigned K) { return (K + RELL_CHUNK - 1) / RELL_CHUNK; }
// at most this many rows with a pair table (n^2 doubles: 512 MB here)
constexpr unsigned RELL_MAX_PAIR_ROWS = 8192;

// d_lnl[i] = sum_p weights[p] * table[p][i] (patterns of weight 0 are left out), d_best[0] = the
// lowest row with the largest d_lnl
hipError_t launch_rell_totals(const double *d_table, unsigned padded, const unsigned *d_pattern_weights,
                              unsigned n_patterns, unsigned n_rows, double *d_partial, double *d_lnl,
                              unsigned *d_best, hipStream_t stream);
// d_mean[i] = (sum_b d_sums[b][i]) / n_replicates
hipError_t launch_rell_means(const double *d_sums, unsigned n_rows, unsigned n_replicates, double *d_partial,
                             double *d_mean, hipStream_t stream);
// d_cmax[b] = max_j c[b][j], d_cbest[b] = c[b][best]; then d_kh[i] / d_sh[i] = replicates with
// d_cbest[b] - c[b][i] / d_cmax[b] - c[b][i] >= d_lnl[best] - d_lnl[i]
hipError_t launch_rell_kh_sh(const double *d_sums, const double *d_mean, const double *d_lnl,
                             const unsigned *d_best, unsigned n_rows, unsigned n_replicates, double *d_cmax,
                             double *d_cbest, unsigned *d_kh, unsigned *d_sh, hipStream_t stream);
// s[i][j] = sqrt(sum_b (c[b][i] - c[b][j])^2 / (n_replicates - 1)), replicates added in order:
// d_rinv[i][j] = s > 0 ? 1 / s : 0 and, unless NULL, d_spread[i][j] = s; both symmetric to the bit
hipError_t launch_rell_spreads(const double *d_sums, const double *d_mean, unsigned n_rows,
                               unsigned n_replicates, double *d_rinv, double *d_spread, hipStream_t stream);
// t(x)_i = max(0, max_j (x_j - x_i) * d_rinv[i][j]); d_tobs[i] = t(d_lnl)_i,
// d_wsh[i] = replicates with t(c[b])_i >= d_tobs[i]
hipError_t launch_rell_wsh(const double *d_sums, const double *d_mean, const double *d_lnl,
                           const double *d_rinv, unsigned n_rows, unsigned n_replicates, double *d_tobs,
                           unsigned *d_wsh, hipStream_t stream);

}  // namespace rdamd
