// The lane map the pre-order kernels share (kernels_outer.hip, kernels_brlen.hip): one lane per
// (site, rate) pair, the R lanes of a site adjacent in the wave, R in {1, 2, 4, 8}.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace rdamd {

// a rate's matrix in LDS starts this many doubles after the previous one (kernels_clv.hip)
constexpr unsigned kOuterRateStride = 18;

// lanes of the wave whose SITE (R adjacent lanes) is small in every rate (kernels_clv.hip)
template <int R>
__device__ __forceinline__ bool site_small(bool lane_small, unsigned lane) {
  constexpr unsigned long long kGroupMask = R == 1 ? ~0ull : R == 2 ? 0x5555555555555555ull
                                          : R == 4 ? 0x1111111111111111ull : 0x0101010101010101ull;
  unsigned long long m = __builtin_amdgcn_ballot_w64(lane_small);
#pragma unroll
  for (int off = 1; off < R; off <<= 1) m &= m >> off;
  m &= kGroupMask;
#pragma unroll
  for (int off = 1; off < R; off <<= 1) m |= m << off;
  return ((m >> lane) & 1ull) != 0;
}

// sum over the R lanes of the site (every lane gets it)
template <int R>
__device__ __forceinline__ double rate_sum(double v) {
#pragma unroll
  for (int off = 1; off < R; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

// sum over the lanes of the wave that hold the same rate (lane % R), in one fixed order (every lane gets it)
template <int R>
__device__ __forceinline__ double site_sum(double v) {
#pragma unroll
  for (int off = R; off < 64; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

}  // namespace rdamd
