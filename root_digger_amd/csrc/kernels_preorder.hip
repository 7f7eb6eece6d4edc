// The pre-order pass: OUTER vectors, and what four analyses make of them -- marginal ancestral
// state posteriors, the first and second derivative of lnL in every branch length, the pair
// sums (the derivative of lnL in every entry of every P-matrix) and the substitutions mapped onto
// every branch per site.  Also the site-rate posteriors, which need the root CLV alone.
//
// New here -- the reference computes no ancestral states and has one derivative, the forward
// difference of its compute_dlh (src/model.cpp), for the root's position alone; this pass extends
// the traversal the reference makes with corax_update_clvs by the complementary one.
// For the tree rooted as the operation list says, site s and rate category r (rate rho_r, weight
// w_r, rate matrix Q_r):
//   L_v[i]  the CLV of node v (rdamd_update_clvs; a tip's is its 0/1 code vector)
//   U_v[j]  P(data outside the subtree of v, state j at v):  U_root = pi, and for an operation with
//           parent u and children a, b
//             t[i]   = U_u[i] (P_b L_b)[i]       the parent's outer vector masked by the sibling
//             U_a[j] = sum_i t[i] P_a[i][j]      (U_b: a and b swapped)
// with the 2^256 rule of the CLVs on the outer vectors: a site whose
// entries are below 2^-256 in EVERY rate is multiplied by 2^256.  The rule acts per site over all
// rates, and so do the CLVs' own scalers: both cancel in everything the consumers form, no count
// is kept and no scaler is read.
//
// The WALK is written once per lane shape (preorder_dna_walk, preorder_generic_walk): the whole
// program (outer_plan.hpp: the operation list read backwards) in ONE launch.  As in
// clv_dna_traversal_kernel every dependency is site-local and each lane owns its site for the
// whole program.  The outer vector of the child whose operation comes next stays in the lane's
// registers, any other waits in a workspace slot (host-side liveness analysis).  The partition is
// only read.
//
// A CONSUMER is a functor the walk calls at fixed places.  There are four:
//   posteriors   post[v][s][j] = sum_r w_r U_v[j] L_v[j], normalised over j: the root's from pi
//                before the loop, an inner child's where its outer vector is formed, its CLV
//                being in registers already.
//   derivatives  y = P_a L_a,  z = Q_r y,  z2 = Q_r z
//                f0 = sum_r w_r t.y   f1 = sum_r w_r rho_r t.z   f2 = sum_r w_r rho_r^2 t.z2
//                d1[a] = sum_s weight_s f1/f0    d2[a] = sum_s weight_s (f2/f0 - (f1/f0)^2)
//                for BOTH children of every operation: tip children have branches too.  The sums
//                over sites are made in one fixed order: inside the wave by a butterfly of
//                exchanges, the four waves of a workgroup in wave order, one partial per
//                (workgroup, branch) in a workspace, and a second kernel that adds the partials by
//                increasing workgroup.  No floating-point atomics; equal inputs give equal bits.
//   pair sums    N[a][r][i][j] = sum_s weight_s w_r t[i] L_a[j] / f0 for both children of every
//                operation (the one consumer that reads the child's own vector in `branch`), and
//                the root's M and W before the loop; summed as the derivatives are, in passes over
//                ranges of whole workgroups (definitions above PairSumDna).
//   substitutions  per site and branch: the joint posterior of the branch's two ends, the
//                probability of a change, the likeliest change and the expected number of
//                substitutions (definitions above SubstArgs); the one consumer that reads the
//                child's staged P-matrix, which `branch` gets as its last argument.  No sums over sites.
// A consumer names its arguments (Args), the LDS it wants beside the walk's (Lds; empty: none is
// allocated) and whether it is told of tip children (kTipBranches) and sums over the workgroup
// (kBlockSums, generic walk); its hooks are begin, op_begin, branch, (branch_done,) outer, op_end
// and end, in the order the walk reaches them.
#include "common.hpp"
#include "k20_preorder.hpp"
#include "outer_plan.hpp"

namespace rdamd {

namespace {

// what the walk reads and the one thing it writes, the workspace
struct WalkArgs {
  const double *clv;          // the partition's inner CLVs, [buffer][site][rate][4]
  size_t clv_stride;          // doubles per buffer
  const uint8_t *tipcodes;
  unsigned tip_stride;
  const uint64_t *codemask;
  const double *pmat;         // [matrix][rate][4][4], rows = parent state
  const double *freqs;        // [rate matrix][4]
  const unsigned *fidx;       // rate -> frequency set
  const double *rate_w;
  unsigned tips, sites;
  double *work;               // [slots (+ 4, generic walk)][site][rate][4]
  const OuterOp *prog;
  unsigned nops, slots;
};

struct PosteriorArgs {
  double *post;               // [node][site][api_states]
  unsigned api_states;
};

struct DerivativeArgs {
  const double *q;            // [rate matrix][4][4], normalised
  const unsigned *pidx;       // rate -> rate matrix
  const double *rates;
  const unsigned *pattern_w;
  double *partials;           // [workgroup][nops][4]: d1, d2 of child 0, d1, d2 of child 1
  unsigned *bad_sites;        // sites whose likelihood is 0 or not finite
};

struct NoLds {};

// ---------------------------------------------------------------------------
// The lane map of the 4-state walk: one lane per (site, rate) pair, the R lanes of a site adjacent
// in the wave, R in {1, 2, 4, 8}
// ---------------------------------------------------------------------------
// a rate's matrix in LDS starts this many doubles after the previous one (kernels_clv.hip)
constexpr unsigned kRateStride = 18;

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

struct DnaLane {
  unsigned tid, lane, idx, cidx, s, r;   // cidx: idx clamped, so that every lane takes part in the exchanges
  bool active;
  double pi[4], w;
};

__device__ __forceinline__ void load_clv(const WalkArgs &a, const DnaLane &ln, unsigned clv, double (&x)[4]) {
  if (clv < a.tips) {   // (16-code alphabet: a tip code is its own state mask)
    const unsigned code = a.tipcodes[(size_t)clv * a.tip_stride + ln.s];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = (code >> k) & 1u ? 1.0 : 0.0;
  } else {
    const double2 *p = reinterpret_cast<const double2 *>(a.clv + (size_t)(clv - a.tips) * a.clv_stride) + (size_t)ln.cidx * 2;
    const double2 lo = p[0], hi = p[1];
    x[0] = lo.x; x[1] = lo.y; x[2] = hi.x; x[3] = hi.y;
  }
}

// the lane-per-site walk's: any code table, one rate at a time
__device__ __forceinline__ void load_clv(const WalkArgs &a, unsigned R, unsigned s, unsigned clv, unsigned r, double (&x)[4]) {
  if (clv < a.tips) {
    const uint64_t mask = a.codemask[a.tipcodes[(size_t)clv * a.tip_stride + s]];
    for (int k = 0; k < 4; ++k) x[k] = (mask >> k) & 1u ? 1.0 : 0.0;
  } else {
    const double *p = a.clv + (size_t)(clv - a.tips) * a.clv_stride + ((size_t)s * R + r) * 4;
    for (int k = 0; k < 4; ++k) x[k] = p[k];
  }
}

// ---------------------------------------------------------------------------
// 4-state walk (binary data embedded).  Both children's P-matrices are staged in LDS one operation
// ahead: thread t fetches one double, one barrier per operation.
// ---------------------------------------------------------------------------
template <int R, class Consumer>
__global__ void __launch_bounds__(256)
preorder_dna_walk(WalkArgs a, typename Consumer::Args ca) {
  constexpr unsigned kMatDoubles = 2 * R * 16;   // both children's matrices of one operation: <= 256
  __shared__ double smat[2][2][R * kRateStride];
  __shared__ typename Consumer::Lds lds;
  Consumer con(ca, lds);
  DnaLane ln;
  ln.tid = threadIdx.x; ln.lane = ln.tid & 63;
  const unsigned tid = ln.tid;
  const unsigned total = a.sites * R;                // < 2^26 (outer_fast_shape)
  ln.idx = blockIdx.x * 256 + tid;
  ln.active = ln.idx < total;
  ln.cidx = ln.active ? ln.idx : total - 1;
  ln.s = ln.cidx / R; ln.r = ln.cidx % R;
  const unsigned r = ln.r;
  const size_t slot_doubles = (size_t)total * 4;
  {
    const double *f = a.freqs + (size_t)a.fidx[r] * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) ln.pi[k] = f[k];
  }
  ln.w = a.rate_w[r];

  const unsigned mc = tid / (R * 16), me = tid % (R * 16);
  auto mat_fetch = [&](unsigned k) {
    if (tid >= kMatDoubles || k >= a.nops) return 0.0;
    return a.pmat[(size_t)a.prog[k].child_mat[mc] * (R * 16) + me];
  };
  auto mat_put = [&](unsigned buf, double v) {
    if (tid < kMatDoubles) smat[buf][mc][(me / 16) * kRateStride + (me % 16)] = v;
  };

  con.begin(a, ln);
  mat_put(0, mat_fetch(0));
  __syncthreads();

  double u[4] = {0, 0, 0, 0};   // the outer vector the next operation reads from registers
  for (unsigned k = 0; k < a.nops; ++k) {
    const OuterOp op = a.prog[k];
    const unsigned buf = k & 1u;
    const double next_m = mat_fetch(k + 1);
    con.op_begin(a, ln, k);
    double up[4];
    if (op.parent_src == kOuterFromSlot) {
      const double2 *p = reinterpret_cast<const double2 *>(a.work + (size_t)op.parent_slot * slot_doubles) + (size_t)ln.cidx * 2;
      const double2 lo = p[0], hi = p[1];
      up[0] = lo.x; up[1] = lo.y; up[2] = hi.x; up[3] = hi.y;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) up[i] = op.parent_src == kOuterFromPi ? ln.pi[i] : u[i];
    }
    double l[2][4], pl[2][4];
    load_clv(a, ln, op.child_clv[0], l[0]);
    load_clv(a, ln, op.child_clv[1], l[1]);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const double *m = &smat[buf][c][r * kRateStride];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        pl[c][i] = m[i * 4 + 0] * l[c][0] + m[i * 4 + 1] * l[c][1] + m[i * 4 + 2] * l[c][2] + m[i * 4 + 3] * l[c][3];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (!op.inner[c] && !Consumer::kTipBranches) continue;   // (wave-uniform)
      const double *m = &smat[buf][c][r * kRateStride];
      double t[4], uc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = up[i] * pl[1 - c][i];   // the parent's vector masked by the sibling
      con.branch(ln, c, t, pl[c], l[c], m);
      if (!op.inner[c]) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) uc[j] = t[0] * m[j] + t[1] * m[4 + j] + t[2] * m[8 + j] + t[3] * m[12 + j];
      // entries are non-negative: uc < 2^-256 is a comparison of high words
      const unsigned hmax = max(max((unsigned)__double2hiint(uc[0]), (unsigned)__double2hiint(uc[1])),
                                max((unsigned)__double2hiint(uc[2]), (unsigned)__double2hiint(uc[3])));
      if (site_small<R>(hmax < 0x2FF00000u, ln.lane)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) uc[j] *= kScaleFactor;
      }
      con.outer(a, ln, op.node[c], uc, l[c]);
      if (op.keep[c] == kOuterKeepReg) {
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = uc[j];
      } else if (op.keep[c] == kOuterKeepSlot && ln.active) {
        double2 *p = reinterpret_cast<double2 *>(a.work + (size_t)op.slot[c] * slot_doubles) + (size_t)ln.idx * 2;
        p[0] = make_double2(uc[0], uc[1]);
        p[1] = make_double2(uc[2], uc[3]);
      }
    }
    con.op_end(ln, k);
    mat_put(buf ^ 1u, next_m);
    __syncthreads();
  }
  con.end(a, ln);
}

// ---------------------------------------------------------------------------
// Generic walk (4 states, any R, any code table): one lane per site, looping over rates.  The
// same program; what the fast walk keeps in registers lives in four more workspace buffers: two
// that alternate as "the registers" and one per child for a vector nobody reads later (it is
// still needed for the second pass: the rescale rule looks at all rates of the site first).
// Two points the walk settles for both consumers: an idle lane stays to the end, computing
// nothing, for the barriers of a consumer that sums over the workgroup; and a small site is
// rescaled by one multiply pass over its stored vector BEFORE the consumer reads it (the factor
// is a power of two: the product is the same number wherever it is formed).
// ---------------------------------------------------------------------------
template <class Consumer>
__global__ void __launch_bounds__(256)
preorder_generic_walk(WalkArgs a, typename Consumer::Args ca, unsigned R) {
  __shared__ typename Consumer::Lds lds;
  Consumer con(ca, lds);
  const unsigned S = a.sites;
  const unsigned tid = threadIdx.x;
  const unsigned s = blockIdx.x * 256 + tid;
  const bool active = s < S;
  const size_t buf_doubles = (size_t)S * R * 4;
  con.begin(a, R, s, active);
  for (unsigned k = 0; k < a.nops; ++k) {
    const OuterOp op = a.prog[k];
    con.op_begin(a, k, tid);
    if (active) {
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
          load_clv(a, R, s, op.child_clv[c], r, l[c]);
          const double *m = a.pmat + ((size_t)op.child_mat[c] * R + r) * 16;
          for (int i = 0; i < 4; ++i)
            pl[c][i] = m[i * 4 + 0] * l[c][0] + m[i * 4 + 1] * l[c][1] + m[i * 4 + 2] * l[c][2] + m[i * 4 + 3] * l[c][3];
        }
        for (int c = 0; c < 2; ++c) {
          if (!op.inner[c] && !Consumer::kTipBranches) continue;
          double t[4];
          for (int i = 0; i < 4; ++i) t[i] = up[i] * pl[1 - c][i];
          con.branch(a, c, r, t, pl[c], l[c], a.pmat + ((size_t)op.child_mat[c] * R + r) * 16);
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
        con.branch_done(c);
        if (!op.inner[c]) continue;
        double *uc = dst[c] + (size_t)s * R * 4;
        if (small[c])
          for (unsigned e = 0; e < R * 4; ++e) uc[e] *= kScaleFactor;
        con.outer(a, R, s, op.node[c], op.child_clv[c], uc);
      }
    }
    con.op_end(k, tid);
    if (Consumer::kBlockSums) __syncthreads();
  }
  con.end(a, active, tid);
}

// ---------------------------------------------------------------------------
// Consumer: marginal ancestral state posteriors
// ---------------------------------------------------------------------------
template <int R>
struct PosteriorDna {
  using Args = PosteriorArgs;
  using Lds = NoLds;
  static constexpr bool kTipBranches = false;
  const Args c;
  __device__ __forceinline__ PosteriorDna(const Args &c, Lds &) : c(c) {}

  __device__ __forceinline__ void write_post(const WalkArgs &a, const DnaLane &ln, unsigned node, const double (&u)[4],
                                             const double (&l)[4]) const {
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = rate_sum<R>(ln.w * u[k] * l[k]);
    const double den = (q[0] + q[1]) + (q[2] + q[3]);
    if (ln.active && ln.r == 0) {
      double *o = c.post + ((size_t)node * a.sites + ln.s) * c.api_states;
      reinterpret_cast<double2 *>(o)[0] = make_double2(q[0] / den, q[1] / den);
      if (c.api_states == 4) reinterpret_cast<double2 *>(o)[1] = make_double2(q[2] / den, q[3] / den);
    }
  }
  __device__ __forceinline__ void begin(const WalkArgs &a, const DnaLane &ln) const {   // the root: U = pi
    double l[4];
    load_clv(a, ln, a.prog[0].parent_clv, l);
    write_post(a, ln, 0, ln.pi, l);
  }
  __device__ __forceinline__ void op_begin(const WalkArgs &, const DnaLane &, unsigned) const {}
  __device__ __forceinline__ void branch(const DnaLane &, int, const double (&)[4], const double (&)[4],
                                         const double (&)[4], const double *) const {}
  __device__ __forceinline__ void outer(const WalkArgs &a, const DnaLane &ln, unsigned node, const double (&uc)[4],
                                        const double (&l)[4]) const {
    write_post(a, ln, node, uc, l);
  }
  __device__ __forceinline__ void op_end(const DnaLane &, unsigned) const {}
  __device__ __forceinline__ void end(const WalkArgs &, const DnaLane &) const {}
};

struct PosteriorGeneric {
  using Args = PosteriorArgs;
  using Lds = NoLds;
  static constexpr bool kTipBranches = false, kBlockSums = false;
  const Args c;
  __device__ __forceinline__ PosteriorGeneric(const Args &c, Lds &) : c(c) {}

  __device__ __forceinline__ void write_post(const WalkArgs &a, unsigned s, unsigned node, const double (&q)[4]) const {
    const double den = (q[0] + q[1]) + (q[2] + q[3]);
    double *o = c.post + ((size_t)node * a.sites + s) * c.api_states;
    for (unsigned k = 0; k < c.api_states; ++k) o[k] = q[k] / den;
  }
  __device__ __forceinline__ void begin(const WalkArgs &a, unsigned R, unsigned s, bool active) const {
    if (!active) return;
    double q[4] = {0, 0, 0, 0}, l[4];
    for (unsigned r = 0; r < R; ++r) {
      const double *f = a.freqs + (size_t)a.fidx[r] * 4;
      load_clv(a, R, s, a.prog[0].parent_clv, r, l);
      for (int k = 0; k < 4; ++k) q[k] += a.rate_w[r] * f[k] * l[k];
    }
    write_post(a, s, 0, q);
  }
  __device__ __forceinline__ void op_begin(const WalkArgs &, unsigned, unsigned) const {}
  __device__ __forceinline__ void branch(const WalkArgs &, int, unsigned, const double (&)[4], const double (&)[4],
                                         const double (&)[4], const double *) const {}
  __device__ __forceinline__ void branch_done(int) const {}
  // u: the site's outer vector, [rate][4]
  __device__ __forceinline__ void outer(const WalkArgs &a, unsigned R, unsigned s, unsigned node, unsigned clv,
                                        const double *u) const {
    double q[4] = {0, 0, 0, 0}, l[4];
    for (unsigned r = 0; r < R; ++r) {
      load_clv(a, R, s, clv, r, l);
      for (int j = 0; j < 4; ++j) q[j] += a.rate_w[r] * u[r * 4 + j] * l[j];
    }
    write_post(a, s, node, q);
  }
  __device__ __forceinline__ void op_end(unsigned, unsigned) const {}
  __device__ __forceinline__ void end(const WalkArgs &, bool, unsigned) const {}
};

// ---------------------------------------------------------------------------
// Consumer: first and second derivative of lnL in every branch length
// ---------------------------------------------------------------------------
// (site_terms, the two site terms of a branch from the sums over rates: common.hpp, shared with kernels_preorder_k20.hip)

// The four waves' sums of operation k wait in wsum[k & 1] (written before the operation's barrier)
// and are added in wave order after it, by the first four threads of the workgroup.
__device__ __forceinline__ void flush_block_sums(const double (&wsum)[4][4], double *partials, unsigned nops, unsigned k,
                                                 unsigned tid) {
  if (tid < 4)
    partials[((size_t)blockIdx.x * nops + k) * 4 + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
}

// Q_r y, Q_r^2 y and the three products with t
__device__ __forceinline__ void branch_products(const double *qm, const double (&t)[4], const double (&y)[4], double *p0,
                                                double *p1, double *p2) {
  double z[4], z2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) z[i] = qm[i * 4 + 0] * y[0] + qm[i * 4 + 1] * y[1] + qm[i * 4 + 2] * y[2] + qm[i * 4 + 3] * y[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) z2[i] = qm[i * 4 + 0] * z[0] + qm[i * 4 + 1] * z[1] + qm[i * 4 + 2] * z[2] + qm[i * 4 + 3] * z[3];
  *p0 = t[0] * y[0] + t[1] * y[1] + t[2] * y[2] + t[3] * y[3];
  *p1 = t[0] * z[0] + t[1] * z[1] + t[2] * z[2] + t[3] * z[3];
  *p2 = t[0] * z2[0] + t[1] * z2[1] + t[2] * z2[2] + t[3] * z2[3];
}

template <int R>
struct DerivativeDna {
  using Args = DerivativeArgs;
  struct Lds {
    alignas(16) double sq[R * kRateStride];   // the R rate matrices, staged once (aligned for 128-bit reads)
    alignas(16) double wsum[2][4][4];
  };
  static constexpr bool kTipBranches = true;
  const Args c;
  Lds &lds;
  double w1, w2, weight;
  double term[4];   // d1, d2 of child 0, d1, d2 of child 1: this site's, this operation's
  bool site_bad = false;
  __device__ __forceinline__ DerivativeDna(const Args &c, Lds &lds) : c(c), lds(lds) {}

  __device__ __forceinline__ void begin(const WalkArgs &, const DnaLane &ln) {
    const double rho = c.rates[ln.r];
    w1 = ln.w * rho; w2 = w1 * rho;
    weight = (double)c.pattern_w[ln.s];
    const unsigned tid = ln.tid;
    if (tid < R * 16) lds.sq[(tid / 16) * kRateStride + (tid % 16)] = c.q[(size_t)c.pidx[tid / 16] * 16 + (tid % 16)];
  }
  __device__ __forceinline__ void op_begin(const WalkArgs &a, const DnaLane &ln, unsigned k) const {
    if (k > 0) flush_block_sums(lds.wsum[(k & 1u) ^ 1u], c.partials, a.nops, k - 1, ln.tid);
  }
  __device__ __forceinline__ void branch(const DnaLane &ln, int ch, const double (&t)[4], const double (&y)[4],
                                         const double (&)[4], const double *) {
    double p0, p1, p2;
    branch_products(&lds.sq[ln.r * kRateStride], t, y, &p0, &p1, &p2);
    const double f0 = rate_sum<R>(ln.w * p0), f1 = rate_sum<R>(w1 * p1), f2 = rate_sum<R>(w2 * p2);
    if (!site_terms(f0, f1, f2, weight, &term[2 * ch], &term[2 * ch + 1])) site_bad = true;
  }
  __device__ __forceinline__ void outer(const WalkArgs &, const DnaLane &, unsigned, const double (&)[4],
                                        const double (&)[4]) const {}
  // The R lanes of a site hold the same four terms: lane r of the site stands for term r (+ R, ...),
  // so one butterfly over the sites of the wave sums R terms at once.
  __device__ __forceinline__ void op_end(const DnaLane &ln, unsigned k) const {
    constexpr int V = R >= 4 ? 1 : 4 / R;
    double val[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const unsigned q = ln.r + (unsigned)v * R;
      const double x = q == 0 ? term[0] : q == 1 ? term[1] : q == 2 ? term[2] : q == 3 ? term[3] : 0.0;
      val[v] = site_sum<R>(ln.active ? x : 0.0);
    }
    if (ln.lane < (R < 4 ? R : 4)) {
#pragma unroll
      for (int v = 0; v < V; ++v) lds.wsum[k & 1u][ln.tid >> 6][ln.lane + v * R] = val[v];
    }
  }
  __device__ __forceinline__ void end(const WalkArgs &a, const DnaLane &ln) const {
    if (a.nops > 0) flush_block_sums(lds.wsum[(a.nops - 1) & 1u], c.partials, a.nops, a.nops - 1, ln.tid);
    if (ln.active && ln.r == 0 && site_bad) atomicAdd(c.bad_sites, 1u);
  }
};

struct DerivativeGeneric {
  using Args = DerivativeArgs;
  struct Lds { alignas(16) double wsum[2][4][4]; };
  static constexpr bool kTipBranches = true, kBlockSums = true;
  const Args c;
  Lds &lds;
  double weight;
  double f[2][3];   // f0, f1, f2 of both children, summed over the rates so far
  double term[4];   // (an idle lane adds zeros)
  bool site_bad = false;
  __device__ __forceinline__ DerivativeGeneric(const Args &c, Lds &lds) : c(c), lds(lds) {}

  __device__ __forceinline__ void begin(const WalkArgs &, unsigned, unsigned s, bool active) {
    weight = active ? (double)c.pattern_w[s] : 0.0;
  }
  __device__ __forceinline__ void op_begin(const WalkArgs &a, unsigned k, unsigned tid) {
    if (k > 0) flush_block_sums(lds.wsum[(k & 1u) ^ 1u], c.partials, a.nops, k - 1, tid);
    for (int i = 0; i < 4; ++i) term[i] = 0.0;
    for (int i = 0; i < 6; ++i) f[i / 3][i % 3] = 0.0;
  }
  __device__ __forceinline__ void branch(const WalkArgs &a, int ch, unsigned r, const double (&t)[4], const double (&y)[4],
                                         const double (&)[4], const double *) {
    const double w = a.rate_w[r], rho = c.rates[r];
    double p0, p1, p2;
    branch_products(c.q + (size_t)c.pidx[r] * 16, t, y, &p0, &p1, &p2);
    f[ch][0] += w * p0;
    f[ch][1] += w * rho * p1;
    f[ch][2] += w * rho * rho * p2;
  }
  __device__ __forceinline__ void branch_done(int ch) {
    if (!site_terms(f[ch][0], f[ch][1], f[ch][2], weight, &term[2 * ch], &term[2 * ch + 1])) site_bad = true;
  }
  __device__ __forceinline__ void outer(const WalkArgs &, unsigned, unsigned, unsigned, unsigned, const double *) const {}
  __device__ __forceinline__ void op_end(unsigned k, unsigned tid) const {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = site_sum<1>(term[q]);
      if ((tid & 63) == 0) lds.wsum[k & 1u][tid >> 6][q] = v;
    }
  }
  __device__ __forceinline__ void end(const WalkArgs &a, bool active, unsigned tid) const {
    if (a.nops > 0) flush_block_sums(lds.wsum[(a.nops - 1) & 1u], c.partials, a.nops, a.nops - 1, tid);
    if (active && site_bad) atomicAdd(c.bad_sites, 1u);
  }
};

// out[e] = the partials of entry e (operation, term) added by increasing workgroup
__global__ void __launch_bounds__(256)
brlen_sum_kernel(const double *__restrict__ partials, unsigned blocks, unsigned entries, double *__restrict__ out) {
  const unsigned e = blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  double acc = 0.0;
  for (unsigned b = 0; b < blocks; ++b) acc += partials[(size_t)b * entries + e];
  out[e] = acc;
}

// ---------------------------------------------------------------------------
// Consumer: pair sums -- the derivative of lnL in every entry of every P-matrix
// ---------------------------------------------------------------------------
//   N[k][c][r][i][j] = sum_s weight_s w_r t_r[i] L_a,r[j] / f0(s)        f0 = sum_r w_r t_r . (P_a L_a,r)
//   M[r][i] = sum_s weight_s w_r L_root,r[i] / froot(s)                  froot = sum_r w_r pi^(r) . L_root,r
//   W[r]    = sum_s weight_s (pi^(r) . L_root,r) / froot(s)
// summed as the derivative consumer sums: inside the wave by site_sum, the four waves in wave order,
// one partial per (workgroup, entry), pair_sum_kernel over the workgroups.  A workgroup's row of
// partials is [nops][2][R][16] pair entries, then [R][5] root entries (M[r][0..3], W[r]).
struct PairSumArgs {
  const unsigned *pattern_w;
  double *partials;           // [workgroup][pair_sum_entries]
  unsigned *bad_sites;
  double *tstage;             // generic walk: [2][lane][R][4], the masked outer vectors of one operation
  unsigned R;
};

__host__ __device__ inline size_t pair_sum_entries(unsigned nops, unsigned R) {
  return (size_t)nops * 2 * R * 16 + (size_t)R * 5;
}

template <int R>
struct PairSumDna {
  using Args = PairSumArgs;
  struct Lds {
    alignas(16) double wsum[2][4][2][R][16];   // [operation parity][wave][child][rate][i][j]
    alignas(16) double rsum[4][R][5];
  };
  static constexpr bool kTipBranches = true;
  static constexpr unsigned kOpEntries = 2 * R * 16;
  const Args c;
  Lds &lds;
  double weight;
  unsigned buf = 0;
  bool site_bad = false;
  __device__ __forceinline__ PairSumDna(const Args &c, Lds &lds) : c(c), lds(lds) {}

  __device__ __forceinline__ void flush(unsigned nops, unsigned k, unsigned tid) const {
    if (tid < kOpEntries) {
      const double *w = &lds.wsum[k & 1u][0][0][0][0];
      c.partials[(size_t)blockIdx.x * pair_sum_entries(nops, R) + (size_t)k * kOpEntries + tid] =
          ((w[tid] + w[kOpEntries + tid]) + w[2 * kOpEntries + tid]) + w[3 * kOpEntries + tid];
    }
  }
  __device__ __forceinline__ void begin(const WalkArgs &a, const DnaLane &ln) {
    weight = (double)c.pattern_w[ln.s];
    double l[4], g;
    load_clv(a, ln, a.prog[0].parent_clv, l);
    const double dot = ln.pi[0] * l[0] + ln.pi[1] * l[1] + ln.pi[2] * l[2] + ln.pi[3] * l[3];
    if (!site_factor(rate_sum<R>(ln.w * dot), weight, &g)) site_bad = true;
    if (!ln.active) g = 0.0;
    const double gw = g * ln.w;
    const double term[5] = {gw * l[0], gw * l[1], gw * l[2], gw * l[3], g * dot};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const double v = site_sum<R>(term[q]);
      if (ln.lane < R) lds.rsum[ln.tid >> 6][ln.lane][q] = v;
    }
  }
  __device__ __forceinline__ void op_begin(const WalkArgs &a, const DnaLane &ln, unsigned k) {
    buf = k & 1u;
    if (k > 0) {
      flush(a.nops, k - 1, ln.tid);
    } else if (ln.tid < R * 5) {   // (the barrier after begin has passed)
      const double *w = &lds.rsum[0][0][0];
      const unsigned t = ln.tid;
      c.partials[(size_t)blockIdx.x * pair_sum_entries(a.nops, R) + (size_t)a.nops * kOpEntries + t] =
          ((w[t] + w[R * 5 + t]) + w[2 * R * 5 + t]) + w[3 * R * 5 + t];
    }
  }
  __device__ __forceinline__ void branch(const DnaLane &ln, int ch, const double (&t)[4], const double (&y)[4],
                                         const double (&l)[4], const double *) {
    const double p0 = t[0] * y[0] + t[1] * y[1] + t[2] * y[2] + t[3] * y[3];
    double g;
    if (!site_factor(rate_sum<R>(ln.w * p0), weight, &g)) site_bad = true;
    if (!ln.active) g = 0.0;
    const double gw = g * ln.w;
    double *o = &lds.wsum[buf][ln.tid >> 6][ch][ln.lane < R ? ln.lane : 0][0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double gt = gw * t[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double v = site_sum<R>(gt * l[j]);
        if (ln.lane < R) o[i * 4 + j] = v;
      }
    }
  }
  __device__ __forceinline__ void outer(const WalkArgs &, const DnaLane &, unsigned, const double (&)[4],
                                        const double (&)[4]) const {}
  __device__ __forceinline__ void op_end(const DnaLane &, unsigned) const {}
  __device__ __forceinline__ void end(const WalkArgs &a, const DnaLane &ln) const {
    if (a.nops > 0) flush(a.nops, a.nops - 1, ln.tid);
    if (ln.active && ln.r == 0 && site_bad) atomicAdd(c.bad_sites, 1u);
  }
};

// One lane per site: the site's factor weight / f0 needs every rate, so `branch` stages w_r t_r and
// op_end, which every lane of the workgroup reaches, forms and sums the products -- one (child,
// rate) chunk of 16 at a time through wsum, whose two halves alternate from chunk to chunk (one
// barrier per chunk: a half is written again only after the barrier that follows its readers).
struct PairSumGeneric {
  using Args = PairSumArgs;
  struct Lds { alignas(16) double wsum[2][4][16]; };
  static constexpr bool kTipBranches = true, kBlockSums = true;
  const Args c;
  Lds &lds;
  const WalkArgs *wa = nullptr;
  double weight = 0.0, f0[2], g[2];
  unsigned s = 0, chunk = 0;
  bool live = false, site_bad = false;
  __device__ __forceinline__ PairSumGeneric(const Args &c, Lds &lds) : c(c), lds(lds) {}

  __device__ __forceinline__ double *stage(int ch, unsigned r) const {
    return c.tstage + ((((size_t)ch * gridDim.x + blockIdx.x) * 256 + threadIdx.x) * c.R + r) * 4;
  }
  // v: this lane's terms of N entries; the workgroup's sums go to partials[at..at + N)
  template <int N>
  __device__ __forceinline__ void block_sum(const double (&v)[N], size_t at, unsigned tid) {
    double (&w)[4][16] = lds.wsum[chunk & 1u];
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const double x = site_sum<1>(v[q]);
      if ((tid & 63) == 0) w[tid >> 6][q] = x;
    }
    __syncthreads();
    if (tid < (unsigned)N) c.partials[at + tid] = ((w[0][tid] + w[1][tid]) + w[2][tid]) + w[3][tid];
    ++chunk;
  }
  __device__ __forceinline__ void begin(const WalkArgs &a, unsigned R, unsigned site, bool active) {
    wa = &a; s = site; live = active;
    weight = active ? (double)c.pattern_w[site] : 0.0;
    const unsigned root = a.prog[0].parent_clv;
    double froot = 0.0, l[4], gr = 0.0;
    if (active) {
      for (unsigned r = 0; r < R; ++r) {
        const double *f = a.freqs + (size_t)a.fidx[r] * 4;
        load_clv(a, R, site, root, r, l);
        froot += a.rate_w[r] * (f[0] * l[0] + f[1] * l[1] + f[2] * l[2] + f[3] * l[3]);
      }
      if (!site_factor(froot, weight, &gr)) site_bad = true;
    }
    const size_t row = (size_t)blockIdx.x * pair_sum_entries(a.nops, R) + (size_t)a.nops * 2 * R * 16;
    for (unsigned r = 0; r < R; ++r) {
      double v[5] = {0, 0, 0, 0, 0};
      if (active) {
        const double *f = a.freqs + (size_t)a.fidx[r] * 4;
        load_clv(a, R, site, root, r, l);
        for (int i = 0; i < 4; ++i) v[i] = gr * a.rate_w[r] * l[i];
        v[4] = gr * (f[0] * l[0] + f[1] * l[1] + f[2] * l[2] + f[3] * l[3]);
      }
      block_sum(v, row + (size_t)r * 5, threadIdx.x);
    }
  }
  __device__ __forceinline__ void op_begin(const WalkArgs &, unsigned, unsigned) { f0[0] = f0[1] = 0.0; }
  __device__ __forceinline__ void branch(const WalkArgs &a, int ch, unsigned r, const double (&t)[4], const double (&y)[4],
                                         const double (&)[4], const double *) {
    const double w = a.rate_w[r];
    f0[ch] += w * (t[0] * y[0] + t[1] * y[1] + t[2] * y[2] + t[3] * y[3]);
    double *o = stage(ch, r);
    for (int i = 0; i < 4; ++i) o[i] = w * t[i];
  }
  __device__ __forceinline__ void branch_done(int ch) {
    if (!site_factor(f0[ch], weight, &g[ch])) site_bad = true;
  }
  __device__ __forceinline__ void outer(const WalkArgs &, unsigned, unsigned, unsigned, unsigned, const double *) const {}
  __device__ __forceinline__ void op_end(unsigned k, unsigned tid) {
    const WalkArgs &a = *wa;
    const unsigned R = c.R;
    const OuterOp op = a.prog[k];
    const size_t row = (size_t)blockIdx.x * pair_sum_entries(a.nops, R) + (size_t)k * 2 * R * 16;
    for (int ch = 0; ch < 2; ++ch)
      for (unsigned r = 0; r < R; ++r) {
        double v[16];
        if (live) {
          double l[4];
          load_clv(a, R, s, op.child_clv[ch], r, l);
          const double *t = stage(ch, r);
          for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) v[i * 4 + j] = (g[ch] * t[i]) * l[j];
        } else {
          for (int e = 0; e < 16; ++e) v[e] = 0.0;
        }
        block_sum(v, row + ((size_t)ch * R + r) * 16, tid);
      }
  }
  __device__ __forceinline__ void end(const WalkArgs &, bool active, unsigned) const {
    if (active && site_bad) atomicAdd(c.bad_sites, 1u);
  }
};

// out[e] = (first pass: 0, else out[e]) + the partials of entry e added by increasing workgroup:
// the running sum of an entry goes through the workgroups in one order however the passes cut them
__global__ void __launch_bounds__(256)
pair_sum_kernel(const double *__restrict__ partials, unsigned blocks, size_t entries, int first, double *out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  double acc = first ? 0.0 : out[e];
  for (unsigned b = 0; b < blocks; ++b) acc += partials[(size_t)b * entries + e];
  out[e] = acc;
}

// ---------------------------------------------------------------------------
// Consumer: substitutions mapped onto branches, per site
// ---------------------------------------------------------------------------
//   J[i][j] = sum_r w_r t_r[i] P_r[i][j] L_a,r[j] / f0(s)     the branch starts in i and ends in j
//   change  = sum_{i != j} J[i][j]      top pair: the largest J[i][j], i != j, the smallest code i K + j at a tie
//   n       = sum_r w_r t_r^T C_r L_a,r / f0(s)               C_r = F(X_r, offdiag(X_r)), made on the host
// for both children of every operation, over the caller's K states.  Nothing is summed over sites:
// every output is written where it is formed, by vector stores, and equal inputs give equal bits.
// The count matrices of an operation ([nops][2][R][16]) are staged in LDS one operation ahead as the
// walk stages P: thread t fetches one double in op_begin and puts it in op_end, under the walk's
// own barrier.
struct SubstArgs {
  const double *cmat;         // [nops][2][R][16], rows = parent state
  double *change, *count;     // [nops][2][sites]; any output may be null
  uint8_t *top_pair;
  double *top_prob;
  double *joint;              // [nops][2][sites][K][K]
  unsigned *bad_sites;
  unsigned api_states, R;
};

// change, the top pair and its probability from the 16 joint entries (K = 2: the first 2 x 2 block)
__device__ __forceinline__ void joint_summary(const double (&J)[16], unsigned K, double *change, unsigned *code, double *top) {
  double sum = 0.0, best = -1.0;
  unsigned at = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i == j || (unsigned)i >= K || (unsigned)j >= K) continue;   // (uniform)
      const double v = J[i * 4 + j];
      sum += v;
      if (v > best) { best = v; at = (unsigned)i * K + (unsigned)j; }
    }
  *change = sum; *code = at; *top = best;
}

__device__ __forceinline__ void write_site_summary(const SubstArgs &c, size_t at, double change, double n, unsigned code,
                                                   double top) {
  if (c.change) c.change[at] = change;
  if (c.count) c.count[at] = n;
  if (c.top_pair) c.top_pair[at] = (uint8_t)code;
  if (c.top_prob) c.top_prob[at] = top;
}

template <int R>
struct SubstDna {
  using Args = SubstArgs;
  struct Lds { alignas(16) double cm[2][2][R * kRateStride]; };   // [operation parity][child][rate]
  static constexpr bool kTipBranches = true;
  static constexpr unsigned kOpDoubles = 2 * R * 16;   // <= 256: one per thread
  const Args c;
  Lds &lds;
  unsigned k = 0, sites = 0;
  double next_c = 0.0;
  bool site_bad = false;
  __device__ __forceinline__ SubstDna(const Args &c, Lds &lds) : c(c), lds(lds) {}

  __device__ __forceinline__ double fetch(unsigned nops, unsigned op, unsigned tid) const {
    if (tid >= kOpDoubles || op >= nops) return 0.0;
    return c.cmat[(size_t)op * kOpDoubles + tid];
  }
  __device__ __forceinline__ void put(unsigned buf, unsigned tid, double v) const {
    if (tid < kOpDoubles) lds.cm[buf][tid / (R * 16)][((tid % (R * 16)) / 16) * kRateStride + (tid % 16)] = v;
  }
  __device__ __forceinline__ void begin(const WalkArgs &a, const DnaLane &ln) {   // (the walk's first barrier follows)
    sites = a.sites;
    put(0, ln.tid, fetch(a.nops, 0, ln.tid));
  }
  __device__ __forceinline__ void op_begin(const WalkArgs &a, const DnaLane &ln, unsigned op) {
    k = op;
    next_c = fetch(a.nops, op + 1, ln.tid);
  }
  __device__ __forceinline__ void branch(const DnaLane &ln, int ch, const double (&t)[4], const double (&y)[4],
                                         const double (&l)[4], const double *m) {
    const double *cm = &lds.cm[k & 1u][ch][ln.r * kRateStride];
    const double p0 = t[0] * y[0] + t[1] * y[1] + t[2] * y[2] + t[3] * y[3];
    double g;
    if (!site_factor(rate_sum<R>(ln.w * p0), 1.0, &g)) site_bad = true;
    const double gw = g * ln.w;
    double tc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      tc += t[i] * (cm[i * 4 + 0] * l[0] + cm[i * 4 + 1] * l[1] + cm[i * 4 + 2] * l[2] + cm[i * 4 + 3] * l[3]);
    const double n = rate_sum<R>(gw * tc);
    double J[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double gt = gw * t[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) J[i * 4 + j] = rate_sum<R>(gt * (m[i * 4 + j] * l[j]));
    }
    if (!ln.active) return;   // (after the exchanges)
    const size_t at = ((size_t)k * 2 + (unsigned)ch) * sites + ln.s;
    if (ln.r == 0) {
      double change, top;
      unsigned code;
      joint_summary(J, c.api_states, &change, &code, &top);
      write_site_summary(c, at, change, n, code, top);
    }
    if (!c.joint) return;
    if (c.api_states == 4) {   // every lane of the site holds J: lane r writes the rows i = r (mod R)
      double2 *o = reinterpret_cast<double2 *>(c.joint + at * 16);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((unsigned)i % R == ln.r) {
          o[2 * i] = make_double2(J[i * 4], J[i * 4 + 1]);
          o[2 * i + 1] = make_double2(J[i * 4 + 2], J[i * 4 + 3]);
        }
    } else if (ln.r == 0) {
      double2 *o = reinterpret_cast<double2 *>(c.joint + at * 4);
      o[0] = make_double2(J[0], J[1]);
      o[1] = make_double2(J[4], J[5]);
    }
  }
  __device__ __forceinline__ void outer(const WalkArgs &, const DnaLane &, unsigned, const double (&)[4],
                                        const double (&)[4]) const {}
  __device__ __forceinline__ void op_end(const DnaLane &ln, unsigned op) const { put((op & 1u) ^ 1u, ln.tid, next_c); }
  __device__ __forceinline__ void end(const WalkArgs &, const DnaLane &ln) const {
    if (ln.active && ln.r == 0 && site_bad) atomicAdd(c.bad_sites, 1u);
  }
};

// one lane per site: the sums over rates are kept unnormalised until the site's f0 is known
struct SubstGeneric {
  using Args = SubstArgs;
  using Lds = NoLds;
  static constexpr bool kTipBranches = true, kBlockSums = false;
  const Args c;
  unsigned k = 0, s = 0, sites = 0;
  double f0[2], n[2], J[2][16];
  bool site_bad = false;
  __device__ __forceinline__ SubstGeneric(const Args &c, Lds &) : c(c) {}

  __device__ __forceinline__ void begin(const WalkArgs &a, unsigned, unsigned site, bool) { s = site; sites = a.sites; }
  __device__ __forceinline__ void op_begin(const WalkArgs &, unsigned op, unsigned) {
    k = op;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      f0[ch] = n[ch] = 0.0;
#pragma unroll
      for (int e = 0; e < 16; ++e) J[ch][e] = 0.0;
    }
  }
  __device__ __forceinline__ void branch(const WalkArgs &a, int ch, unsigned r, const double (&t)[4], const double (&y)[4],
                                         const double (&l)[4], const double *m) {
    const double w = a.rate_w[r];
    const double *cm = c.cmat + (((size_t)k * 2 + (unsigned)ch) * c.R + r) * 16;
    f0[ch] += w * (t[0] * y[0] + t[1] * y[1] + t[2] * y[2] + t[3] * y[3]);
    double tc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      tc += t[i] * (cm[i * 4 + 0] * l[0] + cm[i * 4 + 1] * l[1] + cm[i * 4 + 2] * l[2] + cm[i * 4 + 3] * l[3]);
    n[ch] += w * tc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double wt = w * t[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) J[ch][i * 4 + j] += wt * (m[i * 4 + j] * l[j]);
    }
  }
  __device__ __forceinline__ void branch_done(int ch) {   // (active lanes only)
    double g;
    if (!site_factor(f0[ch], 1.0, &g)) site_bad = true;
    double Jn[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) Jn[e] = g * J[ch][e];
    const size_t at = ((size_t)k * 2 + (unsigned)ch) * sites + s;
    double change, top;
    unsigned code;
    joint_summary(Jn, c.api_states, &change, &code, &top);
    write_site_summary(c, at, change, g * n[ch], code, top);
    if (!c.joint) return;
    const unsigned K = c.api_states;
    double *o = c.joint + at * K * K;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((unsigned)i < K && (unsigned)j < K) o[(unsigned)i * K + (unsigned)j] = Jn[i * 4 + j];
  }
  __device__ __forceinline__ void outer(const WalkArgs &, unsigned, unsigned, unsigned, unsigned, const double *) const {}
  __device__ __forceinline__ void op_end(unsigned, unsigned) const {}
  __device__ __forceinline__ void end(const WalkArgs &, bool active, unsigned) const {
    if (active && site_bad) atomicAdd(c.bad_sites, 1u);
  }
};

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

// one walk over the partition for a consumer pair (the fast walk's and the generic walk's), or
// over the `sites` sites from site0 on alone: a range is offset pointers and a smaller site count
// (the workspace is the range's own; a consumer offsets what it reads per site itself)
template <template <int> class Dna, class Generic>
hipError_t launch_walk(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, unsigned slots, const unsigned *d_fidx,
                       double *d_work, const typename Generic::Args &ca, unsigned site0 = 0, unsigned sites = ~0u) {
  WalkArgs a;
  const bool fast = outer_fast_shape(p);
  const unsigned R = p->rate_cats;
  if (sites == ~0u) sites = p->sites - site0;
  a.clv = p->d_clv + (size_t)site0 * R * 4; a.clv_stride = p->clv_doubles();
  a.tipcodes = p->d_tipcodes + site0; a.tip_stride = p->tip_stride(); a.codemask = p->d_codemask;
  a.pmat = p->d_pmat; a.freqs = p->d_freqs; a.fidx = d_fidx; a.rate_w = p->d_rate_weights;
  a.tips = p->tips; a.sites = sites;
  a.work = d_work; a.prog = d_prog; a.nops = nops; a.slots = slots;
  const unsigned grid = (unsigned)(((size_t)sites * (fast ? R : 1u) + 255) / 256);
  if (!fast) {
    preorder_generic_walk<Generic><<<grid, 256, 0, p->stream>>>(a, ca, R);
  } else {
    switch (R) {
      case 1: preorder_dna_walk<1, Dna<1>><<<grid, 256, 0, p->stream>>>(a, ca); break;
      case 2: preorder_dna_walk<2, Dna<2>><<<grid, 256, 0, p->stream>>>(a, ca); break;
      case 4: preorder_dna_walk<4, Dna<4>><<<grid, 256, 0, p->stream>>>(a, ca); break;
      default: preorder_dna_walk<8, Dna<8>><<<grid, 256, 0, p->stream>>>(a, ca); break;
    }
  }
  return hipGetLastError();
}

}  // namespace

// the shapes preorder_dna_walk takes (kernels_clv.hip's dna_fast_ok: 32-bit lane indices, one CLV under 2 GB)
bool outer_fast_shape(const rdamd_partition *p) {
  const unsigned R = p->rate_cats;
  return p->states == 4 && p->ncodes_cap == 16 && (R == 1 || R == 2 || R == 4 || R == 8) &&
         (size_t)p->sites * R < ((size_t)1 << 26);
}

size_t outer_workspace_doubles(const rdamd_partition *p, unsigned slots) {
  if (p->mfma_layout) return k20_preorder_workspace_doubles(slots, p->rate_cats, p->clv_tiles());   // kernels_preorder_k20.hip
  const size_t buffers = outer_fast_shape(p) ? slots : (size_t)slots + 4;
  return buffers * p->sites * p->rate_cats * 4;
}

unsigned preorder_blocks(const rdamd_partition *p) {
  const size_t lanes = outer_fast_shape(p) ? (size_t)p->sites * p->rate_cats : (size_t)p->sites;
  return (unsigned)((lanes + 255) / 256);
}

hipError_t launch_outer_program(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, unsigned slots,
                                const unsigned *d_fidx, double *d_work, double *d_post) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  const PosteriorArgs ca{d_post, p->api_states};
  return launch_walk<PosteriorDna, PosteriorGeneric>(p, d_prog, nops, slots, d_fidx, d_work, ca);
}

hipError_t launch_brlen_program(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, unsigned slots,
                                const unsigned *d_pidx, const unsigned *d_fidx, double *d_work, double *d_partials,
                                unsigned *d_bad_sites, double *d_out) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  const DerivativeArgs ca{p->d_q, d_pidx, p->d_rates, p->d_pattern_weights, d_partials, d_bad_sites};
  const hipError_t e = launch_walk<DerivativeDna, DerivativeGeneric>(p, d_prog, nops, slots, d_fidx, d_work, ca);
  if (e != hipSuccess) return e;
  return launch_brlen_sum(p, d_partials, preorder_blocks(p), nops * 4, d_out);
}

hipError_t launch_brlen_sum(rdamd_partition *p, const double *d_partials, unsigned blocks, unsigned entries, double *d_out) {
  brlen_sum_kernel<<<(entries + 255) / 256, 256, 0, p->stream>>>(d_partials, blocks, entries, d_out);
  return hipGetLastError();
}

size_t pair_sum_doubles(const rdamd_partition *p, unsigned nops) { return pair_sum_entries(nops, p->rate_cats); }

size_t pair_sum_stage_doubles(const rdamd_partition *p, unsigned blocks) {
  return outer_fast_shape(p) ? 0 : (size_t)2 * blocks * 256 * p->rate_cats * 4;
}

hipError_t launch_pair_sum_program(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, unsigned slots,
                                   const unsigned *d_fidx, double *d_work, double *d_partials, double *d_stage,
                                   unsigned blocks_per_pass, unsigned *d_bad_sites, double *d_out) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  const unsigned R = p->rate_cats, blocks = preorder_blocks(p);
  const unsigned block_sites = outer_fast_shape(p) ? 256 / R : 256;   // sites of one workgroup
  const size_t entries = pair_sum_entries(nops, R);
  for (unsigned b0 = 0; b0 < blocks; b0 += blocks_per_pass) {
    const unsigned nb = std::min(blocks_per_pass, blocks - b0);
    const unsigned site0 = b0 * block_sites, sites = std::min(p->sites - site0, nb * block_sites);
    const PairSumArgs ca{p->d_pattern_weights + site0, d_partials, d_bad_sites, d_stage, R};
    hipError_t e = launch_walk<PairSumDna, PairSumGeneric>(p, d_prog, nops, slots, d_fidx, d_work, ca, site0, sites);
    if (e != hipSuccess) return e;
    e = launch_pair_sum_fold(p, d_partials, nb, entries, b0 == 0, d_out);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_pair_sum_fold(rdamd_partition *p, const double *d_partials, unsigned blocks, size_t entries, bool first,
                                double *d_out) {
  pair_sum_kernel<<<(unsigned)((entries + 255) / 256), 256, 0, p->stream>>>(d_partials, blocks, entries, first, d_out);
  return hipGetLastError();
}

hipError_t launch_subst_program(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, unsigned slots,
                                const unsigned *d_fidx, double *d_work, const double *d_cmat, unsigned *d_bad_sites,
                                double *d_change, double *d_count, uint8_t *d_top_pair, double *d_top_prob, double *d_joint) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  const SubstArgs ca{d_cmat, d_change, d_count, d_top_pair, d_top_prob, d_joint, d_bad_sites, p->api_states, p->rate_cats};
  return launch_walk<SubstDna, SubstGeneric>(p, d_prog, nops, slots, d_fidx, d_work, ca);
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
