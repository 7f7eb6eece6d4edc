// RELL bootstrap kernels (include/root_digger_amd.h, rdamd_rell_bootstrap and rdamd_rell_multiscale):
// resampled sums of the site log-likelihoods of many candidate roots; then either bootstrap
// proportion and expected likelihood weight, or -- the multiscale bootstrap -- the same sums at
// several replicate lengths in one launch and the winner of every replicate found where its sums
// are made.
//
// Lanes are rows (roots).  The matrix is held transposed and padded, table[pattern][padded rows],
// so that one draw is one contiguous read of a table row.  The draws themselves are made 64 (or
// `lanes`) at a time with lanes as DRAWS -- hash, scale, column -> pattern look-up -- and then
// handed round: with 64 lanes per replicate draw j of the batch is a wave-uniform value (readlane:
// the table row's address is scalar), with fewer it is a shuffle inside the replicate's lanes.
//
// The order of the additions of one (replicate, row) is a function of the draw count alone:
// draw d goes to partial sum d mod 8 (batches start at multiples of 8), each partial sum takes
// its draws by increasing d, and the eight are combined as ((0+1)+(2+3))+((4+5)+(6+7)).  Eight
// independent chains keep the FP64 adder busy; no floating-point atomics anywhere.
//
// Both calls run ONE kernel template, rell_resample_kernel<W, V, MULTISCALE>: the loop and the
// order rule exist once, in the kernel's body (a __device__ helper called from two kernels costs
// registers: DESIGN.md 7a).  What MULTISCALE switches, at compile time:
//   before the loop, a wave looks up its scale: draw count M, seed and output index come from the
//   launch's scale list, which the host sorts LONGEST FIRST so that the tail of the grid is short
//   work; the waves of one scale never share a wave with another's, so M is wave-uniform;
//   after it, the winner: a lane's rows, then the replicate's lanes by rell_merge_best's butterfly.
//   Up to 256 rows one wave holds the whole replicate and the butterfly ends in ONE integer atomic
//   add on counts[scale][winner]; beyond, a wave leaves (max, row) of its 256-row chunk and
//   rell_pick_kernel walks a replicate's chunks in row order; the sums go to memory only when the
//   caller wants them.
#include "rell.hpp"

namespace rdamd {

namespace {

template <int V> struct rows_t;
template <> struct rows_t<1> { double v[1]; };
template <> struct alignas(16) rows_t<2> { double v[2]; };
template <> struct alignas(32) rows_t<4> { double v[4]; };

// what the two calls pass beyond the table, the column map and the sizes
template <bool MULTISCALE> struct rell_args_t;
template <> struct rell_args_t<false> {
  uint64_t seed;
  double *sums;
};
template <> struct rell_args_t<true> {
  unsigned groups;   // waves' worth of replicates per scale, ceil(B / (64 / W)) (the launcher fills it in)
  rell_scales_t scales;
  unsigned *counts;
  double *sums, *chunk_max;
  unsigned *chunk_row;
};

// W lanes per replicate, V consecutive rows per lane.  One wave: 64 / W replicates x W * V rows
// (of one scale); M draws out of N columns per replicate.
template <int W, int V, bool MULTISCALE>
__global__ void __launch_bounds__(256)
rell_resample_kernel(const double *__restrict__ table, unsigned padded, const unsigned *__restrict__ col2pat,
                     unsigned N, unsigned n_rows, unsigned B, rell_args_t<MULTISCALE> a) {
  static_assert(W == 64 || V == 1, "several rows per lane only with a whole wave per replicate");
  constexpr unsigned R = 64 / W;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  const unsigned chunks = padded / (W * V);
  unsigned first, M, slot = 0, k = 0;   // first replicate of this wave, its draw count, scale as issued and as output
  uint64_t seed;
  if constexpr (MULTISCALE) {
    const unsigned group = wave / chunks;
    slot = (unsigned)__builtin_amdgcn_readfirstlane((int)(group / a.groups));
    if (slot >= a.scales.n) return;
    first = (group % a.groups) * R;
    M = a.scales.draws[slot];
    k = a.scales.index[slot];
    seed = a.scales.seed[slot];
  } else {
    first = (wave / chunks) * R;
    M = N;
    seed = a.seed;
  }
  if (first >= B) return;
  const unsigned sub = lane / W, l = lane % W;
  const unsigned b = first + sub;
  const bool live = b < B;
  // (a wave with 64 lanes per replicate: b is wave-uniform, the key is scalar arithmetic)
  const uint64_t key = rell_key(seed, W == 64 ? (uint64_t)__builtin_amdgcn_readfirstlane(b) : (uint64_t)(live ? b : first));
  const unsigned chunk = wave % chunks;
  const unsigned row0 = chunk * (W * V) + l * V;
  const double *base = table + row0;

  double acc[V][8];
#pragma unroll
  for (int v = 0; v < V; ++v)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[v][j] = 0.0;

  // the pattern of draw d0 + l of this lane's replicate (lanes beyond M: pattern 0, never added)
  const auto draw = [&](uint64_t d0) -> unsigned {
    const uint64_t d = d0 + l;
    return d < M ? col2pat[rell_draw(key, d, N)] : 0u;
  };
  const auto take = [&](unsigned pat, int j) {
    unsigned p;
    if constexpr (W == 64) p = (unsigned)__builtin_amdgcn_readlane((int)pat, j);
    else p = (unsigned)__shfl((int)pat, j, W);
    const rows_t<V> x = *reinterpret_cast<const rows_t<V> *>(base + (size_t)p * padded);
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v][j & 7] += x.v[v];
  };
  const auto total = [&](int v) {
    return ((acc[v][0] + acc[v][1]) + (acc[v][2] + acc[v][3])) + ((acc[v][4] + acc[v][5]) + (acc[v][6] + acc[v][7]));
  };

  unsigned pat = draw(0);
  for (uint64_t d0 = 0; d0 < M; d0 += W) {
    // the next batch's draws are under way while this one's rows are read
    const unsigned next = d0 + W < M ? draw(d0 + W) : 0u;
    const uint64_t left = M - d0;
    if (left >= W) {
#pragma unroll
      for (int j = 0; j < W; ++j) take(pat, j);
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j)
        if ((uint64_t)j < left) take(pat, j);
    }
    pat = next;
  }

  if constexpr (!MULTISCALE) {
    if (!live) return;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const unsigned row = row0 + v;
      if (row < n_rows) a.sums[(size_t)b * n_rows + row] = total(v);
    }
  } else {
    // this lane's rows (they ascend: the first of equals stays), then the replicate's lanes
    double best = 0.0;
    unsigned at = RELL_NO_ROW;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const unsigned row = row0 + v;
      if (row >= n_rows) continue;
      const double s = total(v);
      if (a.sums && live) a.sums[((size_t)k * B + b) * n_rows + row] = s;
      if (s > best || at == RELL_NO_ROW) { best = s; at = row; }
    }
#pragma unroll
    for (int off = W / 2; off; off >>= 1) rell_merge_best(best, at, off);
    // (row0 of lane 0 is a real row in every chunk: `at` is one)
    if (l != 0 || !live) return;
    if (chunks == 1) {
      atomicAdd(&a.counts[(size_t)k * n_rows + at], 1u);
    } else {
      const size_t cell = ((size_t)slot * B + b) * chunks + chunk;
      a.chunk_max[cell] = best;
      a.chunk_row[cell] = at;
    }
  }
}

// More than 256 rows: one thread per (scale, replicate) walks its chunks in row order.
__global__ void __launch_bounds__(256)
rell_pick_kernel(const double *__restrict__ chunk_max, const unsigned *__restrict__ chunk_row, unsigned chunks,
                 unsigned n_rows, unsigned B, rell_scales_t scales, unsigned *__restrict__ counts) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= (uint64_t)scales.n * B) return;
  const unsigned slot = (unsigned)(t / B);
  const double *m = chunk_max + (size_t)t * chunks;
  double best = m[0];
  unsigned in = 0;
  for (unsigned c = 1; c < chunks; ++c)
    if (m[c] > best) { best = m[c]; in = c; }
  atomicAdd(&counts[(size_t)scales.index[slot] * n_rows + chunk_row[(size_t)t * chunks + in]], 1u);
}

// rows[n_rows][P] -> table[P][padded]; rows >= n_rows read as zero
__global__ void __launch_bounds__(256)
rell_transpose_kernel(const double *__restrict__ rows, unsigned n_rows, unsigned P, unsigned padded,
                      double *__restrict__ table) {
  __shared__ double tile[32][33];
  const unsigned p0 = blockIdx.x * 32u, r0 = blockIdx.y * 32u;
  const unsigned tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;   // 32 x 8
  for (unsigned k = ty; k < 32; k += 8) {
    const unsigned r = r0 + k, p = p0 + tx;
    tile[k][tx] = (r < n_rows && p < P) ? rows[(size_t)r * P + p] : 0.0;
  }
  __syncthreads();
  for (unsigned k = ty; k < 32; k += 8) {
    const unsigned p = p0 + k, r = r0 + tx;
    if (p < P && r < padded) table[(size_t)p * padded + r] = tile[tx][k];
  }
}

// One wave per replicate: its largest sum, the lowest row that has it, and the likelihood weights
// exp(s_i - max) / sum_j exp(s_j - max).  A lane takes rows lane, lane + 64, ...; the lanes'
// partial sums are combined by a fixed butterfly.
__global__ void __launch_bounds__(256)
rell_weights_kernel(const double *__restrict__ sums, unsigned n_rows, unsigned B,
                    double *__restrict__ weights, unsigned *__restrict__ winner) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned b = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (b >= B) return;
  const double *s = sums + (size_t)b * n_rows;
  double best = 0.0;
  unsigned at = RELL_NO_ROW;
  for (unsigned i = lane; i < n_rows; i += 64) {
    const double x = s[i];
    if (x > best || at == RELL_NO_ROW) { best = x; at = i; }   // (rows ascend: the first of equals stays)
  }
  for (int off = 32; off; off >>= 1) rell_merge_best(best, at, off);
  double z = 0.0;
  for (unsigned i = lane; i < n_rows; i += 64) z += exp(s[i] - best);
  for (int off = 32; off; off >>= 1) z += __shfl_xor(z, off);
  for (unsigned i = lane; i < n_rows; i += 64) weights[(size_t)b * n_rows + i] = exp(s[i] - best) / z;
  if (lane == 0) winner[b] = at;
}

// One thread per row: the replicates are walked in order, four interleaved partial sums.
__global__ void __launch_bounds__(256)
rell_support_kernel(const double *__restrict__ weights, const unsigned *__restrict__ winner,
                    unsigned n_rows, unsigned B, double *__restrict__ bp, double *__restrict__ elw) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_rows) return;
  double w[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned wins = 0;
  unsigned b = 0;
  for (; b + 4 <= B; b += 4) {
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
      w[k] += weights[(size_t)(b + k) * n_rows + i];
      wins += winner[b + k] == i ? 1u : 0u;
    }
  }
  for (unsigned k = 0; b < B; ++b, ++k) {
    w[k] += weights[(size_t)b * n_rows + i];
    wins += winner[b] == i ? 1u : 0u;
  }
  bp[i] = (double)wins / (double)B;
  elw[i] = ((w[0] + w[1]) + (w[2] + w[3])) / (double)B;
}

// one launch of the resampling kernel over `slots` scales' worth of replicates
template <bool MULTISCALE>
hipError_t launch_resample(const double *d_table, const rell_shape_t &shape, const unsigned *d_col2pat, unsigned N,
                           unsigned n_rows, unsigned B, unsigned slots, uint64_t max_blocks,
                           rell_args_t<MULTISCALE> args, hipStream_t stream) {
  void (*kernel)(const double *, unsigned, const unsigned *, unsigned, unsigned, unsigned, rell_args_t<MULTISCALE>) = nullptr;
#define RDAMD_RELL_CASE(W, V) \
  if (shape.lanes == W && shape.per_lane == V) kernel = rell_resample_kernel<W, V, MULTISCALE>
  RDAMD_RELL_CASE(8, 1);
  RDAMD_RELL_CASE(16, 1);
  RDAMD_RELL_CASE(32, 1);
  RDAMD_RELL_CASE(64, 1);
  RDAMD_RELL_CASE(64, 2);
  RDAMD_RELL_CASE(64, 4);
#undef RDAMD_RELL_CASE
  if (!kernel) return hipErrorInvalidValue;
  const unsigned R = 64 / shape.lanes;
  const uint64_t groups = ((uint64_t)B + R - 1) / R;
  const uint64_t waves = groups * slots * rell_row_chunks(shape);
  const uint64_t blocks = (waves + 3) / 4;
  if (blocks == 0 || blocks > max_blocks) return hipErrorInvalidConfiguration;
  if constexpr (MULTISCALE) args.groups = (unsigned)groups;
  kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(d_table, shape.padded, d_col2pat, N, n_rows, B, args);
  return hipGetLastError();
}

}  // namespace

rell_shape_t rell_shape(unsigned n_rows) {
  rell_shape_t s;
  s.lanes = n_rows <= 8 ? 8u : n_rows <= 16 ? 16u : n_rows <= 32 ? 32u : 64u;
  s.per_lane = n_rows <= 64 ? 1u : n_rows <= 128 ? 2u : 4u;
  const unsigned chunk = s.lanes * s.per_lane;
  s.padded = (unsigned)(((uint64_t)n_rows + chunk - 1) / chunk * chunk);
  return s;
}

hipError_t launch_rell_transpose(const double *d_rows, unsigned n_rows, unsigned n_patterns,
                                 const rell_shape_t &shape, double *d_table, hipStream_t stream) {
  const dim3 grid((n_patterns + 31) / 32, (shape.padded + 31) / 32);
  if (grid.y > 65535u) return hipErrorInvalidConfiguration;
  rell_transpose_kernel<<<grid, dim3(256), 0, stream>>>(d_rows, n_rows, n_patterns, shape.padded, d_table);
  return hipGetLastError();
}

hipError_t launch_rell_sums(const double *d_table, const rell_shape_t &shape, const unsigned *d_col2pat,
                            unsigned n_columns, unsigned n_rows, unsigned n_replicates, uint64_t seed,
                            double *d_sums, hipStream_t stream) {
  return launch_resample<false>(d_table, shape, d_col2pat, n_columns, n_rows, n_replicates, 1, 0x3fffffffull,
                                {seed, d_sums}, stream);
}

hipError_t launch_rell_multiscale(const double *d_table, const rell_shape_t &shape, const unsigned *d_col2pat,
                                  unsigned n_columns, unsigned n_rows, unsigned n_replicates,
                                  const rell_scales_t &scales, unsigned *d_counts, double *d_sums,
                                  double *d_chunk_max, unsigned *d_chunk_row, hipStream_t stream) {
  const unsigned chunks = rell_row_chunks(shape);
  if (scales.n == 0 || scales.n > RELL_MAX_SCALES || (chunks > 1 && (!d_chunk_max || !d_chunk_row)))
    return hipErrorInvalidValue;
  const hipError_t e = launch_resample<true>(d_table, shape, d_col2pat, n_columns, n_rows, n_replicates, scales.n,
                                             0x00ffffffull, {0, scales, d_counts, d_sums, d_chunk_max, d_chunk_row},
                                             stream);
  if (e != hipSuccess || chunks == 1) return e;
  const uint64_t threads = (uint64_t)scales.n * n_replicates;
  rell_pick_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream>>>(
      d_chunk_max, d_chunk_row, chunks, n_rows, n_replicates, scales, d_counts);
  return hipGetLastError();
}

hipError_t launch_rell_support(const double *d_sums, unsigned n_rows, unsigned n_replicates,
                               double *d_weights, unsigned *d_winner, double *d_bp, double *d_elw,
                               hipStream_t stream) {
  rell_weights_kernel<<<dim3((n_replicates + 3) / 4), dim3(256), 0, stream>>>(d_sums, n_rows, n_replicates,
                                                                             d_weights, d_winner);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  rell_support_kernel<<<dim3((n_rows + 255) / 256), dim3(256), 0, stream>>>(d_weights, d_winner, n_rows,
                                                                           n_replicates, d_bp, d_elw);
  return hipGetLastError();
}

}  // namespace rdamd
