// KH, SH and weighted-SH tests of candidate roots (include/root_digger_amd.h, rdamd_rell_tests):
// what is computed from the resampled sums[B][n] of kernels_rell.hip once they exist.
//
// The centred sums c[b][i] = sums[b][i] - mean[i] are never stored: every kernel subtracts as it
// loads, always as that one subtraction, so c[b][i] has the same bits wherever it is formed.
//
// Orders of addition, none of which depends on a launch shape:
//   sums over the leading axis (observed totals over patterns, means over replicates): entry k goes
//   to chunk k / 512, inside it to slice (k % 512) / 128, inside that to partial sum k % 4; a
//   partial sum adds its entries by increasing k, a slice is (p0 + p1) + (p2 + p3), a chunk is
//   (s0 + s1) + (s2 + s3), and the chunks are added by increasing index;
//   pair spreads: one chain per pair, replicates by increasing b.
// Counts are unsigned integers; blocks add theirs with integer atomics.
//
// The two O(n^2 B) kernels:
//   spreads   64 x 64 pairs per block, 4 x 4 per thread in registers; 16 replicates of both row
//             tiles at a time in LDS (the next 16 are in flight meanwhile).  Only tiles on or above
//             the diagonal are computed: (x - y)^2 and (y - x)^2 have the same bits, so the mirror
//             image is stored, not recomputed.
//   WSH       a block is 64 rows x 64 replicates; a lane is a row, a wave takes 16 of the replicates
//             and keeps their running maxima in registers.  Rows j are walked 32 at a time: the 32
//             values 1 / s[i][j] of the lane's row sit in registers for all 16 replicates (read as
//             rinv[j][i]: the table is symmetric, so lanes read consecutive addresses), and the
//             replicates' centred rows are in LDS, read as wave-wide broadcasts.  Per (b, i, j):
//             one subtraction, one multiplication, one maximum, and half an LDS read.
#include "rell.hpp"

namespace rdamd {

namespace {

template <bool WEIGHTED>
__global__ void __launch_bounds__(256)
rell_colsum_kernel(const double *__restrict__ values, unsigned stride, const unsigned *__restrict__ weights,
                   unsigned K, unsigned n, double *__restrict__ partial) {
  __shared__ double red[4][64];
  const unsigned lane = threadIdx.x & 63u, s = threadIdx.x >> 6;
  const unsigned i = blockIdx.y * 64u + lane;
  const uint64_t k0 = (uint64_t)blockIdx.x * RELL_CHUNK + s * (RELL_CHUNK / 4);
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    for (unsigned q = 0; q < RELL_CHUNK / 4; q += 4) {
#pragma unroll
      for (unsigned e = 0; e < 4; ++e) {
        const uint64_t k = k0 + q + e;
        if (k < K) {
          if constexpr (WEIGHTED) {
            const unsigned w = weights[k];   // (a pattern of weight 0 may hold anything, NaN included)
            if (w) a[e] = fma((double)w, values[k * stride + i], a[e]);
          } else {
            a[e] += values[k * stride + i];
          }
        }
      }
    }
  }
  red[s][lane] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (s == 0 && i < n)
    partial[(size_t)blockIdx.x * n + i] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ void __launch_bounds__(256)
rell_colsum_finish_kernel(const double *__restrict__ partial, unsigned chunks, unsigned n, double divisor,
                          double *__restrict__ out) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (unsigned c = 0; c < chunks; ++c) a += partial[(size_t)c * n + i];
  out[i] = a / divisor;
}

// one wave: the lowest row with the largest total
__global__ void __launch_bounds__(64)
rell_best_kernel(const double *__restrict__ lnl, unsigned n, unsigned *__restrict__ best) {
  const unsigned lane = threadIdx.x;
  double top = 0.0;
  unsigned at = RELL_NO_ROW;
  for (unsigned i = lane; i < n; i += 64) {
    const double x = lnl[i];
    if (at == RELL_NO_ROW || x > top) { top = x; at = i; }
  }
  for (int off = 32; off; off >>= 1) rell_merge_best(top, at, off);
  if (lane == 0) best[0] = at;
}

// one wave per replicate: the largest centred sum and the best row's
__global__ void __launch_bounds__(256)
rell_cmax_kernel(const double *__restrict__ sums, const double *__restrict__ mean,
                 const unsigned *__restrict__ best, unsigned n, unsigned B, double *__restrict__ cmax,
                 double *__restrict__ cbest) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned b = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (b >= B) return;
  const double *s = sums + (size_t)b * n;
  double mx = -__builtin_huge_val();
  for (unsigned i = lane; i < n; i += 64) {
    const double c = s[i] - mean[i];
    mx = c > mx ? c : mx;
  }
  for (int off = 32; off; off >>= 1) {
    const double o = __shfl_xor(mx, off);
    mx = o > mx ? o : mx;
  }
  if (lane == 0) {
    const unsigned m = best[0];
    cmax[b] = mx;
    cbest[b] = s[m] - mean[m];
  }
}

// 64 rows x 256 replicates per block; a lane is a row, a wave takes 64 of the replicates
__global__ void __launch_bounds__(256)
rell_kh_sh_kernel(const double *__restrict__ sums, const double *__restrict__ mean, const double *__restrict__ lnl,
                  const unsigned *__restrict__ best, const double *__restrict__ cmax,
                  const double *__restrict__ cbest, unsigned n, unsigned B, unsigned *__restrict__ kh,
                  unsigned *__restrict__ sh) {
  const unsigned i = blockIdx.y * 64u + (threadIdx.x & 63u);
  if (i >= n) return;
  const uint64_t b0 = (uint64_t)blockIdx.x * 256u + (threadIdx.x >> 6) * 64u;
  const double obs = lnl[best[0]] - lnl[i], mi = mean[i];
  unsigned k = 0, h = 0;
  for (unsigned q = 0; q < 64; ++q) {
    const uint64_t b = b0 + q;
    if (b >= B) break;
    const double c = sums[b * n + i] - mi;
    k += (cbest[b] - c >= obs) ? 1u : 0u;
    h += (cmax[b] - c >= obs) ? 1u : 0u;
  }
  if (k) atomicAdd(&kh[i], k);
  if (h) atomicAdd(&sh[i], h);
}

__global__ void __launch_bounds__(256)
rell_spread_kernel(const double *__restrict__ sums, const double *__restrict__ mean, unsigned n, unsigned B,
                   double *__restrict__ rinv, double *__restrict__ spread) {
  const unsigned ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  __shared__ alignas(16) double a[16][64];
  __shared__ alignas(16) double c[16][64];
  const unsigned tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
  // staging: this thread brings column l of both tiles for replicates kk, kk + 4, kk + 8, kk + 12
  const unsigned l = threadIdx.x & 63u, kk = threadIdx.x >> 6;
  const unsigned gi = ti * 64u + l, gj = tj * 64u + l;
  const double mi = gi < n ? mean[gi] : 0.0, mj = gj < n ? mean[gj] : 0.0;
  double na[4], nc[4];
  // rows beyond n and replicates beyond B are zero: their differences add exactly nothing
  const auto fetch = [&](unsigned b0) {
#pragma unroll
    for (unsigned e = 0; e < 4; ++e) {
      const uint64_t b = (uint64_t)b0 + kk + 4 * e;
      na[e] = (b < B && gi < n) ? sums[b * n + gi] - mi : 0.0;
      nc[e] = (b < B && gj < n) ? sums[b * n + gj] - mj : 0.0;
    }
  };
  double acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;

  fetch(0);
  for (unsigned b0 = 0; b0 < B; b0 += 16) {
    __syncthreads();   // (the last round's reads are over)
#pragma unroll
    for (unsigned e = 0; e < 4; ++e) {
      a[kk + 4 * e][l] = na[e];
      c[kk + 4 * e][l] = nc[e];
    }
    __syncthreads();
    if (b0 + 16 < B) fetch(b0 + 16);
#pragma unroll
    for (unsigned k = 0; k < 16; ++k) {
      double ci[4], cj[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) { ci[x] = a[k][ty * 4 + x]; cj[x] = c[k][tx * 4 + x]; }
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          const double d = ci[x] - cj[y];
          acc[x][y] = fma(d, d, acc[x][y]);
        }
    }
  }
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const unsigned i = ti * 64u + ty * 4u + x, j = tj * 64u + tx * 4u + y;
      if (i >= n || j >= n) continue;
      const double s = sqrt(acc[x][y] / (double)(B - 1));
      const double r = s > 0.0 ? 1.0 / s : 0.0;
      rinv[(size_t)i * n + j] = r;
      if (spread) spread[(size_t)i * n + j] = s;
      if (ti != tj) {
        rinv[(size_t)j * n + i] = r;
        if (spread) spread[(size_t)j * n + i] = s;
      }
    }
}

// the statistic of the observed totals, one thread per row (the arithmetic of rell_wsh_kernel)
__global__ void __launch_bounds__(256)
rell_wsh_observed_kernel(const double *__restrict__ lnl, const double *__restrict__ rinv, unsigned n,
                         double *__restrict__ tobs) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const double xi = lnl[i];
  double t = 0.0;
  for (unsigned j = 0; j < n; ++j) t = fmax(t, (lnl[j] - xi) * rinv[(size_t)j * n + i]);
  tobs[i] = t;
}

constexpr unsigned WSH_R = 16;   // replicates per wave (running maxima per lane)
constexpr unsigned WSH_J = 32;   // rows j per step (reciprocal spreads per lane)

__global__ void __launch_bounds__(256)
rell_wsh_kernel(const double *__restrict__ sums, const double *__restrict__ mean, const double *__restrict__ rinv,
                const double *__restrict__ tobs, unsigned n, unsigned B, unsigned *__restrict__ wsh) {
  __shared__ alignas(16) double c[4 * WSH_R][WSH_J];
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned i = blockIdx.y * 64u + lane;
  const unsigned ic = i < n ? i : n - 1;   // (lanes beyond the rows work on the last row and count nothing)
  const uint64_t b0 = (uint64_t)blockIdx.x * (4 * WSH_R);
  const double mi = mean[ic];
  double ci[WSH_R], t[WSH_R];
#pragma unroll
  for (unsigned k = 0; k < WSH_R; ++k) {
    const uint64_t b = b0 + w * WSH_R + k;
    ci[k] = b < B ? sums[b * n + ic] - mi : 0.0;
    t[k] = 0.0;   // (the j = i term)
  }
  const unsigned jj = threadIdx.x & (WSH_J - 1), slot0 = threadIdx.x / WSH_J;
  for (unsigned j0 = 0; j0 < n; j0 += WSH_J) {
    __syncthreads();   // (the last step's reads are over)
    {
      const unsigned j = j0 + jj;
      const double mj = j < n ? mean[j] : 0.0;
      for (unsigned slot = slot0; slot < 4 * WSH_R; slot += 256 / WSH_J) {
        const uint64_t b = b0 + slot;
        c[slot][jj] = (b < B && j < n) ? sums[b * n + j] - mj : 0.0;
      }
    }
    // 0 for j = i, for a pair of spread 0 and beyond the rows: such a term is +-0, the zero term again
    double r[WSH_J];
#pragma unroll
    for (unsigned e = 0; e < WSH_J; ++e) r[e] = j0 + e < n ? rinv[(size_t)(j0 + e) * n + ic] : 0.0;
    __syncthreads();
#pragma unroll
    for (unsigned e = 0; e < WSH_J; e += 2) {
      // (all 16 broadcast reads are issued before the first is used: one read's latency, not 16)
      double2 v[WSH_R];
#pragma unroll
      for (unsigned k = 0; k < WSH_R; ++k) v[k] = *reinterpret_cast<const double2 *>(&c[w * WSH_R + k][e]);
#pragma unroll
      for (unsigned k = 0; k < WSH_R; ++k) {
        t[k] = fmax(t[k], (v[k].x - ci[k]) * r[e]);
        t[k] = fmax(t[k], (v[k].y - ci[k]) * r[e + 1]);
      }
    }
  }
  if (i >= n) return;
  const double obs = tobs[i];
  unsigned count = 0;
#pragma unroll
  for (unsigned k = 0; k < WSH_R; ++k) count += (b0 + w * WSH_R + k < B && t[k] >= obs) ? 1u : 0u;
  if (count) atomicAdd(&wsh[i], count);
}

// out[i] = (sum over k < K of [weights[k] *] values[k][i]) / divisor
hipError_t column_sums(const double *d_values, unsigned stride, const unsigned *d_weights, unsigned K, unsigned n,
                       double divisor, double *d_partial, double *d_out, hipStream_t stream) {
  const unsigned chunks = rell_chunks(K), tiles = (n + 63) / 64;
  if (tiles > 65535u) return hipErrorInvalidConfiguration;
  if (d_weights)
    rell_colsum_kernel<true><<<dim3(chunks, tiles), dim3(256), 0, stream>>>(d_values, stride, d_weights, K, n, d_partial);
  else
    rell_colsum_kernel<false><<<dim3(chunks, tiles), dim3(256), 0, stream>>>(d_values, stride, nullptr, K, n, d_partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  rell_colsum_finish_kernel<<<dim3((n + 255) / 256), dim3(256), 0, stream>>>(d_partial, chunks, n, divisor, d_out);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_rell_totals(const double *d_table, unsigned padded, const unsigned *d_pattern_weights,
                              unsigned n_patterns, unsigned n_rows, double *d_partial, double *d_lnl,
                              unsigned *d_best, hipStream_t stream) {
  hipError_t e = column_sums(d_table, padded, d_pattern_weights, n_patterns, n_rows, 1.0, d_partial, d_lnl, stream);
  if (e != hipSuccess) return e;
  rell_best_kernel<<<dim3(1), dim3(64), 0, stream>>>(d_lnl, n_rows, d_best);
  return hipGetLastError();
}

hipError_t launch_rell_means(const double *d_sums, unsigned n_rows, unsigned n_replicates, double *d_partial,
                             double *d_mean, hipStream_t stream) {
  return column_sums(d_sums, n_rows, nullptr, n_replicates, n_rows, (double)n_replicates, d_partial, d_mean, stream);
}

hipError_t launch_rell_kh_sh(const double *d_sums, const double *d_mean, const double *d_lnl,
                             const unsigned *d_best, unsigned n_rows, unsigned n_replicates, double *d_cmax,
                             double *d_cbest, unsigned *d_kh, unsigned *d_sh, hipStream_t stream) {
  const unsigned tiles = (n_rows + 63) / 64;
  if (tiles > 65535u) return hipErrorInvalidConfiguration;
  hipError_t e = hipMemsetAsync(d_kh, 0, (size_t)n_rows * sizeof(unsigned), stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(d_sh, 0, (size_t)n_rows * sizeof(unsigned), stream);
  if (e != hipSuccess) return e;
  rell_cmax_kernel<<<dim3((n_replicates + 3) / 4), dim3(256), 0, stream>>>(d_sums, d_mean, d_best, n_rows,
                                                                          n_replicates, d_cmax, d_cbest);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  rell_kh_sh_kernel<<<dim3((n_replicates + 255) / 256, tiles), dim3(256), 0, stream>>>(
      d_sums, d_mean, d_lnl, d_best, d_cmax, d_cbest, n_rows, n_replicates, d_kh, d_sh);
  return hipGetLastError();
}

hipError_t launch_rell_spreads(const double *d_sums, const double *d_mean, unsigned n_rows,
                               unsigned n_replicates, double *d_rinv, double *d_spread, hipStream_t stream) {
  if (n_rows > RELL_MAX_PAIR_ROWS || n_replicates < 2) return hipErrorInvalidValue;
  const unsigned tiles = (n_rows + 63) / 64;
  rell_spread_kernel<<<dim3(tiles, tiles), dim3(256), 0, stream>>>(d_sums, d_mean, n_rows, n_replicates, d_rinv,
                                                                  d_spread);
  return hipGetLastError();
}

hipError_t launch_rell_wsh(const double *d_sums, const double *d_mean, const double *d_lnl,
                           const double *d_rinv, unsigned n_rows, unsigned n_replicates, double *d_tobs,
                           unsigned *d_wsh, hipStream_t stream) {
  if (n_rows > RELL_MAX_PAIR_ROWS) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(d_wsh, 0, (size_t)n_rows * sizeof(unsigned), stream);
  if (e != hipSuccess) return e;
  rell_wsh_observed_kernel<<<dim3((n_rows + 255) / 256), dim3(256), 0, stream>>>(d_lnl, d_rinv, n_rows, d_tobs);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  rell_wsh_kernel<<<dim3((n_replicates + 4 * WSH_R - 1) / (4 * WSH_R), (n_rows + 63) / 64), dim3(256), 0, stream>>>(
      d_sums, d_mean, d_rinv, d_tobs, n_rows, n_replicates, d_wsh);
  return hipGetLastError();
}

}  // namespace rdamd
