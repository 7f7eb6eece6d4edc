// The pre-order pass: OUTER vectors, marginal ancestral state posteriors, site-rate posteriors.
//
// New here -- the reference computes no ancestral states; it extends the traversal it makes with
// corax_update_clvs at /root/reference/src/model.cpp:402 by the complementary pass.
// For the tree rooted as the operation list says, site s and rate category r:
//   L_v[i]  the CLV of node v (rdamd_update_clvs; a tip's is its 0/1 code vector)
//   U_v[j]  P(data outside the subtree of v, state j at v):  U_root = pi, and for an operation with
//           parent u and children a, b
//             U_a[j] = sum_i U_u[i] (P_b L_b)[i] P_a[i][j]         (U_b: a and b swapped)
//   post[v][s][j] = sum_r w_r U_v[j] L_v[j], normalised over j
// with the 2^256 rule of the CLVs on the outer vectors: a site whose
// entries are below 2^-256 in EVERY rate is multiplied by 2^256.  The rule acts per site, so the
// counts cancel in the normalisation and are not kept; the CLVs' own scalers cancel the same way.
//
// The whole program (outer_plan.hpp: the operation list read backwards) runs in ONE launch.  As in
// clv_dna_traversal_kernel every dependency is site-local and each lane owns one (site, rate) pair
// for the whole program; the R lanes of a site are adjacent, so the rescale test and the sums over
// rates are exchanges inside a wave.  The outer vector of the child whose operation comes next stays
// in the lane's registers, any other waits in a workspace slot (host-side liveness analysis); the
// posterior of an inner child is formed where its outer vector is, its CLV being in registers
// already.  The partition is only read.
#include "common.hpp"
#include "outer_lanes.hpp"
#include "outer_plan.hpp"

namespace rdamd {

namespace {

struct OuterArgs {
  const double *clv;          // the partition's inner CLVs, [buffer][site][rate][4]
  size_t clv_stride;          // doubles per buffer
  const uint8_t *tipcodes;
  unsigned tip_stride;
  const uint64_t *codemask;
  const double *pmat;         // [matrix][rate][4][4], rows = parent state
  const double *freqs;        // [rate matrix][4]
  const unsigned *fidx;       // rate -> frequency set
  const double *rate_w;
  unsigned tips, sites, api_states;
  double *work;               // [slots (+ 4, generic kernel)][site][rate][4]
  double *post;               // [node][site][api_states]
  const OuterOp *prog;
  unsigned nops, slots;
};

// ---------------------------------------------------------------------------
// 4-state path (binary data embedded): one lane per (site, rate), R in {1, 2, 4, 8}, tip codes
// that are their own state masks (16-code alphabet)
// ---------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(256)
outer_dna_kernel(OuterArgs a) {
  // (a rate's matrix starts kRateStride doubles after the previous one: kernels_clv.hip)
  constexpr unsigned kRateStride = 18;
  constexpr unsigned kMatDoubles = 2 * R * 16;   // both children's matrices of one operation: <= 256
  __shared__ double smat[2][2][R * kRateStride];
  const unsigned tid = threadIdx.x, lane = tid & 63;
  const unsigned S = a.sites;
  const unsigned total = S * R;                      // < 2^26 (outer_fast_shape)
  const unsigned idx = blockIdx.x * 256 + tid;       // one (site, rate) pair per lane
  const bool active = idx < total;
  const unsigned cidx = active ? idx : total - 1;    // clamped: every lane takes part in the exchanges
  const unsigned s = cidx / R, r = cidx % R;
  const bool writer = active && r == 0;
  const size_t slot_doubles = (size_t)total * 4;

  double pi[4];
  {
    const double *f = a.freqs + (size_t)a.fidx[r] * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) pi[k] = f[k];
  }
  const double w = a.rate_w[r];

  // P-matrices: the block stages both matrices of the NEXT operation while it works on this one
  // (thread t fetches one double; one barrier per operation)
  const unsigned mc = tid / (R * 16), me = tid % (R * 16);
  auto mat_fetch = [&](unsigned k) {
    if (tid >= kMatDoubles || k >= a.nops) return 0.0;
    return a.pmat[(size_t)a.prog[k].child_mat[mc] * (R * 16) + me];
  };
  auto mat_put = [&](unsigned buf, double v) {
    if (tid < kMatDoubles) smat[buf][mc][(me / 16) * kRateStride + (me % 16)] = v;
  };
  auto load_clv = [&](unsigned clv, double (&x)[4]) {
    if (clv < a.tips) {
      const unsigned code = a.tipcodes[(size_t)clv * a.tip_stride + s];
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = (code >> k) & 1u ? 1.0 : 0.0;
    } else {
      const double2 *p = reinterpret_cast<const double2 *>(a.clv + (size_t)(clv - a.tips) * a.clv_stride) + (size_t)cidx * 2;
      const double2 lo = p[0], hi = p[1];
      x[0] = lo.x; x[1] = lo.y; x[2] = hi.x; x[3] = hi.y;
    }
  };
  // sum over the R lanes of the site (every lane gets it)
  auto rate_sum = [&](double v) {
#pragma unroll
    for (int off = 1; off < R; off <<= 1) v += __shfl_xor(v, off);
    return v;
  };
  auto write_post = [&](unsigned node, const double (&u)[4], const double (&l)[4]) {
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = rate_sum(w * u[k] * l[k]);
    const double den = (q[0] + q[1]) + (q[2] + q[3]);
    if (writer) {
      double *o = a.post + ((size_t)node * S + s) * a.api_states;
      reinterpret_cast<double2 *>(o)[0] = make_double2(q[0] / den, q[1] / den);
      if (a.api_states == 4) reinterpret_cast<double2 *>(o)[1] = make_double2(q[2] / den, q[3] / den);
    }
  };

  {   // the root: U = pi
    double l[4];
    load_clv(a.prog[0].parent_clv, l);
    write_post(0, pi, l);
  }
  mat_put(0, mat_fetch(0));
  __syncthreads();

  double u[4] = {0, 0, 0, 0};   // the outer vector the next operation reads from registers
  for (unsigned k = 0; k < a.nops; ++k) {
    const OuterOp op = a.prog[k];
    const unsigned buf = k & 1u;
    const double next_m = mat_fetch(k + 1);
    double up[4];
    if (op.parent_src == kOuterFromSlot) {
      const double2 *p = reinterpret_cast<const double2 *>(a.work + (size_t)op.parent_slot * slot_doubles) + (size_t)cidx * 2;
      const double2 lo = p[0], hi = p[1];
      up[0] = lo.x; up[1] = lo.y; up[2] = hi.x; up[3] = hi.y;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) up[i] = op.parent_src == kOuterFromPi ? pi[i] : u[i];
    }
    double l[2][4], pl[2][4];
    load_clv(op.child_clv[0], l[0]);
    load_clv(op.child_clv[1], l[1]);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const double *m = &smat[buf][c][r * kRateStride];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        pl[c][i] = m[i * 4 + 0] * l[c][0] + m[i * 4 + 1] * l[c][1] + m[i * 4 + 2] * l[c][2] + m[i * 4 + 3] * l[c][3];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (!op.inner[c]) continue;   // (wave-uniform)
      const double *m = &smat[buf][c][r * kRateStride];
      double t[4], uc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = up[i] * pl[1 - c][i];   // the parent's vector masked by the sibling
#pragma unroll
      for (int j = 0; j < 4; ++j) uc[j] = t[0] * m[j] + t[1] * m[4 + j] + t[2] * m[8 + j] + t[3] * m[12 + j];
      // entries are non-negative: uc < 2^-256 is a comparison of high words
      const unsigned hmax = max(max((unsigned)__double2hiint(uc[0]), (unsigned)__double2hiint(uc[1])),
                                max((unsigned)__double2hiint(uc[2]), (unsigned)__double2hiint(uc[3])));
      if (site_small<R>(hmax < 0x2FF00000u, lane)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) uc[j] *= kScaleFactor;
      }
      write_post(op.node[c], uc, l[c]);
      if (op.keep[c] == kOuterKeepReg) {
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = uc[j];
      } else if (op.keep[c] == kOuterKeepSlot && active) {
        double2 *p = reinterpret_cast<double2 *>(a.work + (size_t)op.slot[c] * slot_doubles) + (size_t)idx * 2;
        p[0] = make_double2(uc[0], uc[1]);
        p[1] = make_double2(uc[2], uc[3]);
      }
    }
    mat_put(buf ^ 1u, next_m);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Generic path (4 states, any R): one lane per site, looping over rates.  The same program; what
// the fast kernel keeps in registers lives in four more workspace buffers: two that alternate as
// "the registers" and one per child for a vector nobody reads later (it is still needed for the
// second pass: the rescale rule looks at all rates of the site first).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
outer_generic_kernel(OuterArgs a, unsigned R) {
  const unsigned S = a.sites;
  const unsigned s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const size_t buf_doubles = (size_t)S * R * 4;
  auto load_clv = [&](unsigned clv, unsigned r, double (&x)[4]) {
    if (clv < a.tips) {
      const uint64_t mask = a.codemask[a.tipcodes[(size_t)clv * a.tip_stride + s]];
      for (int k = 0; k < 4; ++k) x[k] = (mask >> k) & 1u ? 1.0 : 0.0;
    } else {
      const double *p = a.clv + (size_t)(clv - a.tips) * a.clv_stride + ((size_t)s * R + r) * 4;
      for (int k = 0; k < 4; ++k) x[k] = p[k];
    }
  };
  auto write_post = [&](unsigned node, const double (&q)[4]) {
    const double den = (q[0] + q[1]) + (q[2] + q[3]);
    double *o = a.post + ((size_t)node * S + s) * a.api_states;
    for (unsigned k = 0; k < a.api_states; ++k) o[k] = q[k] / den;
  };
  {
    double q[4] = {0, 0, 0, 0}, l[4];
    for (unsigned r = 0; r < R; ++r) {
      const double *f = a.freqs + (size_t)a.fidx[r] * 4;
      load_clv(a.prog[0].parent_clv, r, l);
      for (int k = 0; k < 4; ++k) q[k] += a.rate_w[r] * f[k] * l[k];
    }
    write_post(0, q);
  }
  for (unsigned k = 0; k < a.nops; ++k) {
    const OuterOp op = a.prog[k];
    const double *src = op.parent_src == kOuterFromSlot ? a.work + (size_t)op.parent_slot * buf_doubles
                      : op.parent_src == kOuterFromReg ? a.work + (size_t)(a.slots + (k & 1u)) * buf_doubles : nullptr;
    double *dst[2];
    for (int c = 0; c < 2; ++c)
      dst[c] = a.work + (size_t)(op.keep[c] == kOuterKeepSlot ? op.slot[c]
                                 : op.keep[c] == kOuterKeepReg ? a.slots + ((k + 1) & 1u) : a.slots + 2u + (unsigned)c) * buf_doubles;
    bool small[2] = {true, true};
    for (unsigned r = 0; r < R; ++r) {   // (a freed slot may be written by this very operation: read rate r first)
      const size_t at = ((size_t)s * R + r) * 4;
      double up[4], l[2][4], pl[2][4];
      const double *f = src ? src + at : a.freqs + (size_t)a.fidx[r] * 4;
      for (int i = 0; i < 4; ++i) up[i] = f[i];
      for (int c = 0; c < 2; ++c) {
        load_clv(op.child_clv[c], r, l[c]);
        const double *m = a.pmat + ((size_t)op.child_mat[c] * R + r) * 16;
        for (int i = 0; i < 4; ++i)
          pl[c][i] = m[i * 4 + 0] * l[c][0] + m[i * 4 + 1] * l[c][1] + m[i * 4 + 2] * l[c][2] + m[i * 4 + 3] * l[c][3];
      }
      for (int c = 0; c < 2; ++c) {
        if (!op.inner[c]) continue;
        const double *m = a.pmat + ((size_t)op.child_mat[c] * R + r) * 16;
        for (int j = 0; j < 4; ++j) {
          const double uc = up[0] * pl[1 - c][0] * m[j] + up[1] * pl[1 - c][1] * m[4 + j] +
                            up[2] * pl[1 - c][2] * m[8 + j] + up[3] * pl[1 - c][3] * m[12 + j];
          dst[c][at + j] = uc;
          small[c] = small[c] && uc < kScaleThreshold;
        }
      }
    }
    for (int c = 0; c < 2; ++c) {
      if (!op.inner[c]) continue;
      double q[4] = {0, 0, 0, 0}, l[4];
      for (unsigned r = 0; r < R; ++r) {
        const size_t at = ((size_t)s * R + r) * 4;
        load_clv(op.child_clv[c], r, l);
        for (int j = 0; j < 4; ++j) {
          double uc = dst[c][at + j];
          if (small[c]) dst[c][at + j] = uc = uc * kScaleFactor;
          q[j] += a.rate_w[r] * uc * l[j];
        }
      }
      write_post(op.node[c], q);
    }
  }
}

// posterior of every rate category and the posterior mean rate of every site, from the root CLV
// (any state count; one lane per site).  Per-site scalers cancel in the normalisation.
__global__ void __launch_bounds__(256)
site_rates_kernel(const double *__restrict__ clv, const double *__restrict__ freqs, const unsigned *__restrict__ fidx,
                  const double *__restrict__ rate_w, const double *__restrict__ rates, unsigned S, unsigned R,
                  unsigned K, double *__restrict__ cat, double *__restrict__ mean) {
  const unsigned s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  auto term = [&](unsigned r) {
    const double *c = clv + ((size_t)s * R + r) * K, *f = freqs + (size_t)fidx[r] * K;
    double t = 0.0;
    for (unsigned i = 0; i < K; ++i) t += f[i] * c[i];
    return rate_w[r] * t;
  };
  double den = 0.0, m = 0.0;
  for (unsigned r = 0; r < R; ++r) den += term(r);
  for (unsigned r = 0; r < R; ++r) {
    const double pr = term(r) / den;
    if (cat) cat[(size_t)s * R + r] = pr;
    m += pr * rates[r];
  }
  if (mean) mean[s] = m;
}

}  // namespace

// the shapes outer_dna_kernel takes (kernels_clv.hip's dna_fast_ok: 32-bit lane indices, one CLV under 2 GB)
bool outer_fast_shape(const rdamd_partition *p) {
  const unsigned R = p->rate_cats;
  return p->states == 4 && p->ncodes_cap == 16 && (R == 1 || R == 2 || R == 4 || R == 8) &&
         (size_t)p->sites * R < ((size_t)1 << 26);
}

size_t outer_workspace_doubles(const rdamd_partition *p, unsigned slots) {
  const size_t buffers = outer_fast_shape(p) ? slots : (size_t)slots + 4;
  return buffers * p->sites * p->rate_cats * 4;
}

hipError_t launch_outer_program(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, unsigned slots,
                                const unsigned *d_fidx, double *d_work, double *d_post) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  OuterArgs a;
  a.clv = p->d_clv; a.clv_stride = p->clv_doubles();
  a.tipcodes = p->d_tipcodes; a.tip_stride = p->tip_stride(); a.codemask = p->d_codemask;
  a.pmat = p->d_pmat; a.freqs = p->d_freqs; a.fidx = d_fidx; a.rate_w = p->d_rate_weights;
  a.tips = p->tips; a.sites = p->sites; a.api_states = p->api_states;
  a.work = d_work; a.post = d_post; a.prog = d_prog; a.nops = nops; a.slots = slots;
  const unsigned R = p->rate_cats;
  if (outer_fast_shape(p)) {
    const unsigned grid = (unsigned)(((size_t)p->sites * R + 255) / 256);
    switch (R) {
      case 1: outer_dna_kernel<1><<<grid, 256, 0, p->stream>>>(a); break;
      case 2: outer_dna_kernel<2><<<grid, 256, 0, p->stream>>>(a); break;
      case 4: outer_dna_kernel<4><<<grid, 256, 0, p->stream>>>(a); break;
      default: outer_dna_kernel<8><<<grid, 256, 0, p->stream>>>(a); break;
    }
  } else {
    outer_generic_kernel<<<(p->sites + 255) / 256, 256, 0, p->stream>>>(a, R);
  }
  return hipGetLastError();
}

hipError_t launch_site_rates(rdamd_partition *p, unsigned clv_phys_index, const unsigned *d_fidx, double *d_cat,
                             double *d_mean) {
  if (p->sites == 0) return hipSuccess;
  const double *clv = p->d_clv + (size_t)(clv_phys_index - p->tips) * p->clv_doubles();
  site_rates_kernel<<<(p->sites + 255) / 256, 256, 0, p->stream>>>(clv, p->d_freqs, d_fidx, p->d_rate_weights, p->d_rates,
                                                                    p->sites, p->rate_cats, p->states, d_cat, d_mean);
  return hipGetLastError();
}

}  // namespace rdamd
