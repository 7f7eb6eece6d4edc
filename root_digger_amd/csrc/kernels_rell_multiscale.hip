// Multiscale RELL bootstrap kernels (include/root_digger_amd.h, rdamd_rell_multiscale): the
// resampled sums of kernels_rell.hip at several replicate lengths in one launch, and the winner of
// every replicate found where its sums are made.
//
// The table layout, the lane-as-draw batches, the readlane / shuffle hand-round and the eight
// chains are rell_sums_kernel's (that kernel is left alone: its own instantiations are what
// rdamd_rell_bootstrap runs, and its code is repeated here rather than shared so that they do not
// move).  What differs:
//   a wave looks up its scale: draw count M, seed and output index come from the launch's scale
//   list, which the host sorts LONGEST FIRST so that the tail of the grid is short work; the waves
//   of one scale never share a wave with another's, so M is wave-uniform;
//   the winner: a lane's rows, then the replicate's lanes by rell_weights_kernel's butterfly
//   (larger sum, lowest row among equals).  Up to 256 rows one wave holds the whole replicate and
//   the butterfly ends in ONE integer atomic add on counts[scale][winner]; beyond, a wave leaves
//   (max, row) of its 256-row chunk and rell_pick_kernel walks a replicate's chunks in row order;
//   the sums go to memory only when the caller wants them.
#include "rell.hpp"

namespace rdamd {

namespace {

template <int V> struct rows_t;
template <> struct rows_t<1> { double v[1]; };
template <> struct alignas(16) rows_t<2> { double v[2]; };
template <> struct alignas(32) rows_t<4> { double v[4]; };

constexpr unsigned NO_ROW = 0xffffffffu;

// W lanes per replicate, V consecutive rows per lane.  One wave: 64 / W replicates x W * V rows of
// one scale.  groups = waves' worth of replicates per scale, ceil(B / (64 / W)).
template <int W, int V>
__global__ void __launch_bounds__(256)
rell_multiscale_kernel(const double *__restrict__ table, unsigned padded, const unsigned *__restrict__ col2pat,
                       unsigned N, unsigned n_rows, unsigned B, unsigned groups, rell_scales_t scales,
                       unsigned *__restrict__ counts, double *__restrict__ sums,
                       double *__restrict__ chunk_max, unsigned *__restrict__ chunk_row) {
  static_assert(W == 64 || V == 1, "several rows per lane only with a whole wave per replicate");
  constexpr unsigned R = 64 / W;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  const unsigned chunks = padded / (W * V);
  const unsigned group = wave / chunks;
  const unsigned slot = (unsigned)__builtin_amdgcn_readfirstlane((int)(group / groups));
  if (slot >= scales.n) return;
  const unsigned first = (group % groups) * R;   // first replicate of this wave
  if (first >= B) return;
  const unsigned M = scales.draws[slot];
  const unsigned k = scales.index[slot];
  const unsigned sub = lane / W, l = lane % W;
  const unsigned b = first + sub;
  const bool live = b < B;
  const uint64_t key = rell_key(scales.seed[slot], W == 64 ? (uint64_t)__builtin_amdgcn_readfirstlane(b)
                                                            : (uint64_t)(live ? b : first));
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

  // this lane's rows (they ascend: the first of equals stays), then the replicate's lanes
  double best = 0.0;
  unsigned at = NO_ROW;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const unsigned row = row0 + v;
    if (row >= n_rows) continue;
    const double s = ((acc[v][0] + acc[v][1]) + (acc[v][2] + acc[v][3])) +
                     ((acc[v][4] + acc[v][5]) + (acc[v][6] + acc[v][7]));
    if (sums && live) sums[((size_t)k * B + b) * n_rows + row] = s;
    if (s > best || at == NO_ROW) { best = s; at = row; }
  }
#pragma unroll
  for (int off = W / 2; off; off >>= 1) {
    const double ob = __shfl_xor(best, off);
    const unsigned oa = (unsigned)__shfl_xor((int)at, off);
    if (oa != NO_ROW && (at == NO_ROW || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
  }
  // (row0 of lane 0 is a real row in every chunk: `at` is one)
  if (l != 0 || !live) return;
  if (chunks == 1) {
    atomicAdd(&counts[(size_t)k * n_rows + at], 1u);
  } else {
    const size_t cell = ((size_t)slot * B + b) * chunks + chunk;
    chunk_max[cell] = best;
    chunk_row[cell] = at;
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

template <int W, int V>
hipError_t launch_multiscale(const double *d_table, unsigned padded, const unsigned *d_col2pat, unsigned N,
                             unsigned n_rows, unsigned B, const rell_scales_t &scales, unsigned *d_counts,
                             double *d_sums, double *d_chunk_max, unsigned *d_chunk_row, hipStream_t stream) {
  const uint64_t groups = ((uint64_t)B + 64 / W - 1) / (64 / W);
  const uint64_t waves = groups * scales.n * (padded / (W * V));
  const uint64_t blocks = (waves + 3) / 4;
  if (blocks == 0 || blocks > 0x00ffffffull) return hipErrorInvalidConfiguration;
  rell_multiscale_kernel<W, V><<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(
      d_table, padded, d_col2pat, N, n_rows, B, (unsigned)groups, scales, d_counts, d_sums, d_chunk_max, d_chunk_row);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_rell_multiscale(const double *d_table, const rell_shape_t &shape, const unsigned *d_col2pat,
                                  unsigned n_columns, unsigned n_rows, unsigned n_replicates,
                                  const rell_scales_t &scales, unsigned *d_counts, double *d_sums,
                                  double *d_chunk_max, unsigned *d_chunk_row, hipStream_t stream) {
  const unsigned chunks = rell_row_chunks(shape);
  if (scales.n == 0 || scales.n > RELL_MAX_SCALES || (chunks > 1 && (!d_chunk_max || !d_chunk_row)))
    return hipErrorInvalidValue;
  hipError_t e = hipErrorInvalidValue;
#define RDAMD_RELL_CASE(W, V)                                                                              \
  if (shape.lanes == W && shape.per_lane == V)                                                             \
    e = launch_multiscale<W, V>(d_table, shape.padded, d_col2pat, n_columns, n_rows, n_replicates, scales, \
                                d_counts, d_sums, d_chunk_max, d_chunk_row, stream)
  RDAMD_RELL_CASE(8, 1);
  RDAMD_RELL_CASE(16, 1);
  RDAMD_RELL_CASE(32, 1);
  RDAMD_RELL_CASE(64, 1);
  RDAMD_RELL_CASE(64, 2);
  RDAMD_RELL_CASE(64, 4);
#undef RDAMD_RELL_CASE
  if (e != hipSuccess || chunks == 1) return e;
  const uint64_t threads = (uint64_t)scales.n * n_replicates;
  rell_pick_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream>>>(
      d_chunk_max, d_chunk_row, chunks, n_rows, n_replicates, scales, d_counts);
  return hipGetLastError();
}

}  // namespace rdamd
