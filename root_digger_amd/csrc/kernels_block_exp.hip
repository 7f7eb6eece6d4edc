// The 20-state block exponential on the matrix cores: the device route of rdamd_pair_sum_adjoints
// (include/root_digger_amd.h).  One wave per (branch, rate) problem forms
//   F = F(X, E),  X = rho tau Q_m^T,  E = N[branch][rate]
// with the arithmetic of pgrad::block_exp (param_gradient.hpp): 18 Taylor terms on the pair (exp, F)
// of X / 2^s, then s squarings (P, F) -> (P P, P F + F P).  s and 2^-s come from the host's own loop
// (pgrad::block_scaling), so the trip count is uniform over the wave and equal to the host's.
//
// Every 20 x 20 x 20 product is 20 v_mfma_f64_16x16x4_f64 (k20_block_exp.hpp: 20 pads to 32, the
// k-steps are the residue sets {grp + 4 r}, 39 % of the issue slots do work).  The Taylor recurrences
// are left products by the constant matrices,
//   D_k = (X D_{k-1} + E T_{k-1}) / k,   T_k = X T_{k-1} / k      (the host's T X: powers of X commute)
// and an accumulator is already the B operand of the next left product, so the Taylor phase moves
// nothing between lanes.  A squaring needs P and F as A operands too: one re-deal through LDS
// (6.7 KB a wave).  The two products of a sum are accumulated apart and added afterwards, and no
// multiply-add outside the matrix cores is contracted, as on the host: the two routes differ only
// in the order inside the dot products of length 20.
//
// Inputs and outputs are dense row-major matrices in the natural state order.  Vector stores only, no
// atomics; the bits of a problem depend on nothing but its inputs.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "k20_block_exp.hpp"
#include "param_gradient.hpp"

namespace rdamd {

static_assert(kBx20TaylorTerms == pgrad::kBlockTaylorTerms, "the device runs the host's Taylor series");

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// c = a b: a in A layout, b and c in B layout (c distinct from a and b)
__device__ __forceinline__ void left_product(const double (&a)[kBx20Tiles][kBx20Steps],
                                             const double (&b)[kBx20Tiles][kBx20Steps],
                                             double (&c)[kBx20Tiles][kBx20Steps]) {
#pragma unroll
  for (unsigned ct = 0; ct < kBx20Tiles; ++ct) {
    f64x4 lo = {0.0, 0.0, 0.0, 0.0}, hi = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (unsigned r = 0; r < kBx20Steps; ++r) {
      lo = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][r], b[ct][r], lo, 0, 0, 0);
      hi = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1][r], b[ct][r], hi, 0, 0, 0);
    }
    // k20x_acc_step: row tile 0's registers are steps 0..3, row tile 1's register 0 is step 4
    c[ct][0] = lo[0]; c[ct][1] = lo[1]; c[ct][2] = lo[2]; c[ct][3] = lo[3];
    c[ct][4] = hi[0];
  }
}

// q: [sets][20][20]; pair, adjoint: [problems][20][20]; one workgroup is one wave
__global__ void __launch_bounds__(64)
k20_block_exp_kernel(const double *__restrict__ q, const double *__restrict__ pair,
                     const k20x_problem_t *__restrict__ problems, size_t n_problems, double *__restrict__ adjoint) {
#pragma clang fp contract(off)
  constexpr unsigned K = kBx20States, NT = kBx20Tiles, NS = kBx20Steps;
  __shared__ double lds[2 * kBx20LdsMatrix];
  const unsigned lane = threadIdx.x;
  for (size_t prob = blockIdx.x; prob < n_problems; prob += gridDim.x) {
    const k20x_problem_t pr = problems[prob];
    const double *qm = q + (size_t)pr.set * (K * K), *nn = pair + prob * (K * K);
    // A layout of X = rho tau Q^T (the dense index transposed) and of E, both scaled as the host scales them
    double xa[NT][NS], ea[NT][NS];
#pragma unroll
    for (unsigned rt = 0; rt < NT; ++rt)
#pragma unroll
      for (unsigned r = 0; r < NS; ++r) {
        const unsigned at = k20x_a_index(lane, rt, r);
        const bool there = at != kBx20Absent;
        xa[rt][r] = there ? (pr.rho_tau * qm[(at % K) * K + at / K]) * pr.scale : 0.0;
        ea[rt][r] = there ? nn[at] * pr.scale : 0.0;
      }
    // B layout: term = X^(k-1) / (k-1)!, d = D_(k-1), and the sums p and f
    double term[NT][NS], p[NT][NS], d[NT][NS], f[NT][NS], t1[NT][NS], t2[NT][NS];
#pragma unroll
    for (unsigned ct = 0; ct < NT; ++ct)
#pragma unroll
      for (unsigned r = 0; r < NS; ++r) {
        const unsigned at = k20x_b_index(lane, ct, r);
        term[ct][r] = p[ct][r] = (at != kBx20Absent && at / K == at % K) ? 1.0 : 0.0;
        d[ct][r] = f[ct][r] = 0.0;
      }
#pragma unroll 1
    for (int k = 1; k <= kBx20TaylorTerms; ++k) {
      const double inv = 1.0 / (double)k;
      left_product(xa, d, t1);
      left_product(ea, term, t2);
#pragma unroll
      for (unsigned ct = 0; ct < NT; ++ct)
#pragma unroll
        for (unsigned r = 0; r < NS; ++r) { d[ct][r] = (t1[ct][r] + t2[ct][r]) * inv; f[ct][r] += d[ct][r]; }
      left_product(xa, term, t1);
#pragma unroll
      for (unsigned ct = 0; ct < NT; ++ct)
#pragma unroll
        for (unsigned r = 0; r < NS; ++r) { term[ct][r] = t1[ct][r] * inv; p[ct][r] += term[ct][r]; }
    }
    // (P, F) -> (P P, P F + F P): P and F once more as A operands, through LDS
#pragma unroll 1
    for (int k = 0; k < pr.squarings; ++k) {
#pragma unroll
      for (unsigned ct = 0; ct < NT; ++ct)
#pragma unroll
        for (unsigned r = 0; r < NS; ++r) {
          const unsigned at = k20x_b_index(lane, ct, r);
          if (at != kBx20Absent) { lds[k20x_lds_index(0, at)] = p[ct][r]; lds[k20x_lds_index(1, at)] = f[ct][r]; }
        }
      __syncthreads();
      double pa[NT][NS], fa[NT][NS];
#pragma unroll
      for (unsigned rt = 0; rt < NT; ++rt)
#pragma unroll
        for (unsigned r = 0; r < NS; ++r) {
          const unsigned at = k20x_a_index(lane, rt, r);
          const bool there = at != kBx20Absent;
          pa[rt][r] = there ? lds[k20x_lds_index(0, at)] : 0.0;
          fa[rt][r] = there ? lds[k20x_lds_index(1, at)] : 0.0;
        }
      __syncthreads();   // (the next squaring, or the next problem, writes the same LDS)
      left_product(pa, f, t1);
      left_product(fa, p, t2);
      left_product(pa, p, d);
#pragma unroll
      for (unsigned ct = 0; ct < NT; ++ct)
#pragma unroll
        for (unsigned r = 0; r < NS; ++r) { f[ct][r] = t1[ct][r] + t2[ct][r]; p[ct][r] = d[ct][r]; }
    }
    double *out = adjoint + prob * (K * K);
#pragma unroll
    for (unsigned ct = 0; ct < NT; ++ct)
#pragma unroll
      for (unsigned r = 0; r < NS; ++r) {
        const unsigned at = k20x_b_index(lane, ct, r);
        if (at != kBx20Absent) out[at] = f[ct][r];
      }
  }
}

}  // namespace

hipError_t launch_k20_block_exp(const double *q, const double *pair, const k20x_problem_t *problems, size_t n_problems,
                                double *adjoint, hipStream_t stream) {
  if (n_problems == 0) return hipSuccess;
  const unsigned grid = (unsigned)(n_problems < (1u << 20) ? n_problems : (1u << 20));
  hipLaunchKernelGGL(k20_block_exp_kernel, dim3(grid), dim3(64), 0, stream, q, pair, problems, n_problems, adjoint);
  return hipGetLastError();
}

}  // namespace rdamd
