// First and second derivative of lnL with respect to every branch length, in one pre-order launch.
//
// New here -- the reference has one derivative, the forward difference of its compute_dlh
// (src/model.cpp), for the root's position alone.  With the OUTER vectors of
// kernels_outer.hip the exact derivatives of every branch cost one small matrix-vector product per
// child and operation.  For the tree rooted as the operation list says, an operation with parent u
// and children a, b, site s and rate category r (rate rho_r, weight w_r, rate matrix Q_r):
//   t[i] = U_u[i] (P_b L_b)[i]      the parent's outer vector masked by the sibling
//   y = P_a L_a,  z = Q_r y,  z2 = Q_r z
//   f0 = sum_r w_r t.y              the site likelihood (up to the per-site scaling factors)
//   f1 = sum_r w_r rho_r t.z        f2 = sum_r w_r rho_r^2 t.z2
//   d1[a] = sum_s weight_s f1/f0    d2[a] = sum_s weight_s (f2/f0 - (f1/f0)^2)
// The 2^256 rule on U and the CLVs' scalers act per site over all rates: they cancel in f1/f0 and
// f2/f0, no scaler is read.  Tip children have branches too: both children of every operation get
// their derivatives, whether or not they get an outer vector.
//
// The program is plan_outer_program's, unchanged: the same OuterOp list with the same register and
// slot placement of U, one launch for the whole list.  The sums over sites are made in one fixed
// order: inside the wave by a butterfly of exchanges, the four waves of a workgroup in wave order,
// one partial per (workgroup, branch) in a workspace, and a second kernel that adds the partials
// by increasing workgroup.  No floating-point atomics; equal inputs give equal bits.  The
// partition is only read.
#include "common.hpp"
#include "outer_lanes.hpp"
#include "outer_plan.hpp"

namespace rdamd {

namespace {

struct BrlenArgs {
  const double *clv;          // the partition's inner CLVs, [buffer][site][rate][4]
  size_t clv_stride;          // doubles per buffer
  const uint8_t *tipcodes;
  unsigned tip_stride;
  const uint64_t *codemask;
  const double *pmat;         // [matrix][rate][4][4], rows = parent state
  const double *q;            // [rate matrix][4][4], normalised
  const double *freqs;        // [rate matrix][4]
  const unsigned *pidx;       // rate -> rate matrix
  const unsigned *fidx;       // rate -> frequency set
  const double *rate_w, *rates;
  const unsigned *pattern_w;
  unsigned tips, sites;
  double *work;               // [slots (+ 4, generic kernel)][site][rate][4]
  double *partials;           // [workgroup][nops][4]: d1, d2 of child 0, d1, d2 of child 1
  unsigned *bad_sites;        // sites whose likelihood is 0 or not finite
  const OuterOp *prog;
  unsigned nops, slots;
};

// the two site terms of a branch from the sums over rates; false: the site has no likelihood
__device__ __forceinline__ bool site_terms(double f0, double f1, double f2, double weight, double *d1, double *d2) {
  if (!(f0 > 0.0) || !isfinite(f0) || !isfinite(f1) || !isfinite(f2)) { *d1 = 0.0; *d2 = 0.0; return false; }
  const double g = f1 / f0;
  *d1 = weight * g;
  *d2 = weight * (f2 / f0 - g * g);
  return true;
}

// The four waves' sums of operation k wait in wsum[k & 1] (written before the operation's barrier)
// and are added in wave order after it, by the first four threads of the workgroup.
__device__ __forceinline__ void flush_block_sums(const double (&wsum)[4][4], double *partials, unsigned nops, unsigned k,
                                                 unsigned tid) {
  if (tid < 4)
    partials[((size_t)blockIdx.x * nops + k) * 4 + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
}

// ---------------------------------------------------------------------------
// 4-state path (binary data embedded): outer_dna_kernel's lane map -- one lane per (site, rate),
// R in {1, 2, 4, 8}, both children's P-matrices staged in LDS one operation ahead -- plus the R
// rate matrices in LDS once.
// ---------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(256)
brlen_dna_kernel(BrlenArgs a) {
  constexpr unsigned kRateStride = kOuterRateStride;
  constexpr unsigned kMatDoubles = 2 * R * 16;   // both children's matrices of one operation: <= 256
  __shared__ double smat[2][2][R * kRateStride];
  __shared__ double sq[R * kRateStride];
  __shared__ double wsum[2][4][4];
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned S = a.sites;
  const unsigned total = S * R;                      // < 2^26 (outer_fast_shape)
  const unsigned idx = blockIdx.x * 256 + tid;       // one (site, rate) pair per lane
  const bool active = idx < total;
  const unsigned cidx = active ? idx : total - 1;    // clamped: every lane takes part in the exchanges
  const unsigned s = cidx / R, r = cidx % R;
  const size_t slot_doubles = (size_t)total * 4;

  double pi[4];
  {
    const double *f = a.freqs + (size_t)a.fidx[r] * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) pi[k] = f[k];
  }
  const double w = a.rate_w[r], rho = a.rates[r];
  const double w1 = w * rho, w2 = w1 * rho;
  const double weight = (double)a.pattern_w[s];
  if (tid < R * 16) sq[(tid / 16) * kRateStride + (tid % 16)] = a.q[(size_t)a.pidx[tid / 16] * 16 + (tid % 16)];

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

  mat_put(0, mat_fetch(0));
  __syncthreads();

  bool site_bad = false;
  double u[4] = {0, 0, 0, 0};   // the outer vector the next operation reads from registers
  for (unsigned k = 0; k < a.nops; ++k) {
    const OuterOp op = a.prog[k];
    const unsigned buf = k & 1u;
    const double next_m = mat_fetch(k + 1);
    if (k > 0) flush_block_sums(wsum[buf ^ 1u], a.partials, a.nops, k - 1, tid);
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
    const double *qm = &sq[r * kRateStride];
    double term[4];   // d1, d2 of child 0, d1, d2 of child 1: this site's
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const double *m = &smat[buf][c][r * kRateStride];
      double t[4], z[4], z2[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = up[i] * pl[1 - c][i];   // the parent's vector masked by the sibling
#pragma unroll
      for (int i = 0; i < 4; ++i)
        z[i] = qm[i * 4 + 0] * pl[c][0] + qm[i * 4 + 1] * pl[c][1] + qm[i * 4 + 2] * pl[c][2] + qm[i * 4 + 3] * pl[c][3];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        z2[i] = qm[i * 4 + 0] * z[0] + qm[i * 4 + 1] * z[1] + qm[i * 4 + 2] * z[2] + qm[i * 4 + 3] * z[3];
      const double f0 = rate_sum<R>(w * (t[0] * pl[c][0] + t[1] * pl[c][1] + t[2] * pl[c][2] + t[3] * pl[c][3]));
      const double f1 = rate_sum<R>(w1 * (t[0] * z[0] + t[1] * z[1] + t[2] * z[2] + t[3] * z[3]));
      const double f2 = rate_sum<R>(w2 * (t[0] * z2[0] + t[1] * z2[1] + t[2] * z2[2] + t[3] * z2[3]));
      if (!site_terms(f0, f1, f2, weight, &term[2 * c], &term[2 * c + 1])) site_bad = true;
      if (!op.inner[c]) continue;   // (wave-uniform)
      double uc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) uc[j] = t[0] * m[j] + t[1] * m[4 + j] + t[2] * m[8 + j] + t[3] * m[12 + j];
      // entries are non-negative: uc < 2^-256 is a comparison of high words
      const unsigned hmax = max(max((unsigned)__double2hiint(uc[0]), (unsigned)__double2hiint(uc[1])),
                                max((unsigned)__double2hiint(uc[2]), (unsigned)__double2hiint(uc[3])));
      if (site_small<R>(hmax < 0x2FF00000u, lane)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) uc[j] *= kScaleFactor;
      }
      if (op.keep[c] == kOuterKeepReg) {
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = uc[j];
      } else if (op.keep[c] == kOuterKeepSlot && active) {
        double2 *p = reinterpret_cast<double2 *>(a.work + (size_t)op.slot[c] * slot_doubles) + (size_t)idx * 2;
        p[0] = make_double2(uc[0], uc[1]);
        p[1] = make_double2(uc[2], uc[3]);
      }
    }
    // The R lanes of a site hold the same four terms: lane r of the site stands for term r (+ R, ...),
    // so one butterfly over the sites of the wave sums R terms at once.
    constexpr int V = R >= 4 ? 1 : 4 / R;
    double val[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const unsigned q = r + (unsigned)v * R;
      const double x = q == 0 ? term[0] : q == 1 ? term[1] : q == 2 ? term[2] : q == 3 ? term[3] : 0.0;
      val[v] = site_sum<R>(active ? x : 0.0);
    }
    if (lane < (R < 4 ? R : 4)) {
#pragma unroll
      for (int v = 0; v < V; ++v) wsum[buf][wave][lane + v * R] = val[v];
    }
    mat_put(buf ^ 1u, next_m);
    __syncthreads();
  }
  if (a.nops > 0) flush_block_sums(wsum[(a.nops - 1) & 1u], a.partials, a.nops, a.nops - 1, tid);
  if (active && r == 0 && site_bad) atomicAdd(a.bad_sites, 1u);
}

// ---------------------------------------------------------------------------
// Generic path (4 states, any R): one lane per site, looping over rates, as outer_generic_kernel:
// what the fast kernel keeps in registers lives in four more workspace buffers.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
brlen_generic_kernel(BrlenArgs a, unsigned R) {
  __shared__ double wsum[2][4][4];
  const unsigned S = a.sites;
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned s = blockIdx.x * 256 + tid;
  const bool active = s < S;   // (an idle lane computes nothing and adds zeros)
  const size_t buf_doubles = (size_t)S * R * 4;
  const double weight = active ? (double)a.pattern_w[s] : 0.0;
  auto load_clv = [&](unsigned clv, unsigned r, double (&x)[4]) {
    if (clv < a.tips) {
      const uint64_t mask = a.codemask[a.tipcodes[(size_t)clv * a.tip_stride + s]];
      for (int k = 0; k < 4; ++k) x[k] = (mask >> k) & 1u ? 1.0 : 0.0;
    } else {
      const double *p = a.clv + (size_t)(clv - a.tips) * a.clv_stride + ((size_t)s * R + r) * 4;
      for (int k = 0; k < 4; ++k) x[k] = p[k];
    }
  };
  bool site_bad = false;
  for (unsigned k = 0; k < a.nops; ++k) {
    const OuterOp op = a.prog[k];
    const unsigned buf = k & 1u;
    if (k > 0) flush_block_sums(wsum[buf ^ 1u], a.partials, a.nops, k - 1, tid);
    double term[4] = {0, 0, 0, 0};
    if (active) {
      const double *src = op.parent_src == kOuterFromSlot ? a.work + (size_t)op.parent_slot * buf_doubles
                        : op.parent_src == kOuterFromReg ? a.work + (size_t)(a.slots + (k & 1u)) * buf_doubles : nullptr;
      double *dst[2];
      for (int c = 0; c < 2; ++c)
        dst[c] = a.work + (size_t)(op.keep[c] == kOuterKeepSlot ? op.slot[c]
                                   : op.keep[c] == kOuterKeepReg ? a.slots + ((k + 1) & 1u) : a.slots + 2u + (unsigned)c) * buf_doubles;
      bool small[2] = {true, true};
      double f[2][3] = {{0, 0, 0}, {0, 0, 0}};
      for (unsigned r = 0; r < R; ++r) {   // (a freed slot may be written by this very operation: read rate r first)
        const size_t at = ((size_t)s * R + r) * 4;
        double up[4], l[2][4], pl[2][4];
        const double *fr = src ? src + at : a.freqs + (size_t)a.fidx[r] * 4;
        for (int i = 0; i < 4; ++i) up[i] = fr[i];
        for (int c = 0; c < 2; ++c) {
          load_clv(op.child_clv[c], r, l[c]);
          const double *m = a.pmat + ((size_t)op.child_mat[c] * R + r) * 16;
          for (int i = 0; i < 4; ++i)
            pl[c][i] = m[i * 4 + 0] * l[c][0] + m[i * 4 + 1] * l[c][1] + m[i * 4 + 2] * l[c][2] + m[i * 4 + 3] * l[c][3];
        }
        const double *qm = a.q + (size_t)a.pidx[r] * 16;
        const double w = a.rate_w[r], rho = a.rates[r];
        for (int c = 0; c < 2; ++c) {
          double t[4], z[4], z2[4];
          for (int i = 0; i < 4; ++i) t[i] = up[i] * pl[1 - c][i];
          for (int i = 0; i < 4; ++i)
            z[i] = qm[i * 4 + 0] * pl[c][0] + qm[i * 4 + 1] * pl[c][1] + qm[i * 4 + 2] * pl[c][2] + qm[i * 4 + 3] * pl[c][3];
          for (int i = 0; i < 4; ++i)
            z2[i] = qm[i * 4 + 0] * z[0] + qm[i * 4 + 1] * z[1] + qm[i * 4 + 2] * z[2] + qm[i * 4 + 3] * z[3];
          f[c][0] += w * (t[0] * pl[c][0] + t[1] * pl[c][1] + t[2] * pl[c][2] + t[3] * pl[c][3]);
          f[c][1] += w * rho * (t[0] * z[0] + t[1] * z[1] + t[2] * z[2] + t[3] * z[3]);
          f[c][2] += w * rho * rho * (t[0] * z2[0] + t[1] * z2[1] + t[2] * z2[2] + t[3] * z2[3]);
          if (!op.inner[c]) continue;
          const double *m = a.pmat + ((size_t)op.child_mat[c] * R + r) * 16;
          for (int j = 0; j < 4; ++j) {
            const double uc = t[0] * m[j] + t[1] * m[4 + j] + t[2] * m[8 + j] + t[3] * m[12 + j];
            dst[c][at + j] = uc;
            small[c] = small[c] && uc < kScaleThreshold;
          }
        }
      }
      for (int c = 0; c < 2; ++c) {
        if (!site_terms(f[c][0], f[c][1], f[c][2], weight, &term[2 * c], &term[2 * c + 1])) site_bad = true;
        if (!op.inner[c] || !small[c]) continue;
        for (unsigned e = 0; e < R * 4; ++e) dst[c][(size_t)s * R * 4 + e] *= kScaleFactor;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = site_sum<1>(term[q]);
      if (lane == 0) wsum[buf][wave][q] = v;
    }
    __syncthreads();
  }
  if (a.nops > 0) flush_block_sums(wsum[(a.nops - 1) & 1u], a.partials, a.nops, a.nops - 1, tid);
  if (active && site_bad) atomicAdd(a.bad_sites, 1u);
}

// out[e] = the partials of entry e (operation, term) added by increasing workgroup
__global__ void __launch_bounds__(256)
brlen_sum_kernel(const double *__restrict__ partials, unsigned blocks, unsigned entries, double *__restrict__ out) {
  const unsigned e = blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  double acc = 0.0;
  for (unsigned b = 0; b < blocks; ++b) acc += partials[(size_t)b * entries + e];
  out[e] = acc;
}

}  // namespace

unsigned brlen_blocks(const rdamd_partition *p) {
  const size_t lanes = outer_fast_shape(p) ? (size_t)p->sites * p->rate_cats : (size_t)p->sites;
  return (unsigned)((lanes + 255) / 256);
}

hipError_t launch_brlen_program(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, unsigned slots,
                                const unsigned *d_pidx, const unsigned *d_fidx, double *d_work, double *d_partials,
                                unsigned *d_bad_sites, double *d_out) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  BrlenArgs a;
  a.clv = p->d_clv; a.clv_stride = p->clv_doubles();
  a.tipcodes = p->d_tipcodes; a.tip_stride = p->tip_stride(); a.codemask = p->d_codemask;
  a.pmat = p->d_pmat; a.q = p->d_q; a.freqs = p->d_freqs; a.pidx = d_pidx; a.fidx = d_fidx;
  a.rate_w = p->d_rate_weights; a.rates = p->d_rates; a.pattern_w = p->d_pattern_weights;
  a.tips = p->tips; a.sites = p->sites;
  a.work = d_work; a.partials = d_partials; a.bad_sites = d_bad_sites; a.prog = d_prog; a.nops = nops; a.slots = slots;
  const unsigned R = p->rate_cats, grid = brlen_blocks(p);
  if (outer_fast_shape(p)) {
    switch (R) {
      case 1: brlen_dna_kernel<1><<<grid, 256, 0, p->stream>>>(a); break;
      case 2: brlen_dna_kernel<2><<<grid, 256, 0, p->stream>>>(a); break;
      case 4: brlen_dna_kernel<4><<<grid, 256, 0, p->stream>>>(a); break;
      default: brlen_dna_kernel<8><<<grid, 256, 0, p->stream>>>(a); break;
    }
  } else {
    brlen_generic_kernel<<<grid, 256, 0, p->stream>>>(a, R);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned entries = nops * 4;
  brlen_sum_kernel<<<(entries + 255) / 256, 256, 0, p->stream>>>(d_partials, grid, entries, d_out);
  return hipGetLastError();
}

}  // namespace rdamd
