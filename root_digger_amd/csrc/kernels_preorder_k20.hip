// The pre-order pass for 20-state partitions in the matrix-core operand layout
// (rdamd_partition::mfma_layout): the OUTER vectors of kernels_preorder.hip on
// v_mfma_f64_4x4x4_4b_f64, and their consumers: the marginal ancestral state posteriors, the
// first and second derivative of lnL in every branch length, and the branch pair sums.
//
// New here -- the reference computes no ancestral states; this extends the traversal it makes with
// corax_update_clvs (src/model.cpp:402) by the complementary pass, for protein data.  Definitions as
// in kernels_preorder.hip:  U_root = pi_r,  t = U_u (.) (P_b L_b),  U_a = t^T P_a,
// post[v][s][j] = sum_r w_r U_v L_v normalised over j, and the 2^256 rule on the outer vectors per
// site over all rates and all 20 states (no count is kept: the outputs are normalised per site).
//
// The program is the planner's, unchanged (outer_plan.hpp): parents from pi, registers or a
// workspace slot, children kept in registers or a slot, the whole list in ONE launch; the
// partition is only read.
//
// Lane map: the traversal kernel's (kernels_clv_mfma.hip).  A wave is (16 sites, one rate), a
// workgroup the R rates of the same 16 sites; col = lane % 16 is the site, grp = lane / 16 holds the
// states k20_state_of(grp, t), t = 0..4 -- five doubles per vector and lane.
//
// Per operation, with `up` the parent's outer vector:
//   pl_c = P_c L_c     inner child: 25 MFMAs, A = the MFMA-ready copy d_pmat_mfma, B = the child's
//                      CLV tile (the forward kernel's child_product); tip child: its tip-table row,
//                      in operand order already, no MFMA
//   t    = up (.) pl_sibling   lane-wise: the D layout is the B layout, nothing moves
//   uc   = P_c^T t     inner child: 25 MFMAs, A from the SAME staged copy read transposed
//                      (k20_preorder.hpp, k20_a_transposed; proven on the host by
//                      tests/cpp/k20_preorder_check.cpp)
// so an operation costs up to 100 MFMAs per wave where the forward kernel spends 50.
//
// Rescale rule: the largest of the lane's five entries against 2^-256, one ballot folded over the
// four lane groups on the scalar unit, one word per wave (bits 0-15 child 0, 16-31 child 1) in a
// flag array double-buffered by operation parity, ONE barrier; a site small in every rate is
// multiplied by 2^256 in every rate.
//
// A CONSUMER is a functor called at fixed places (begin, op_begin, branch, outer, op_end, end), as in
// kernels_preorder.hip; it owns the exchange area of the workgroup's LDS ([child][rate][320]).
// The posteriors: each wave puts w_r U L of an inner child there in `outer`; after one barrier (op_end)
// wave c % R adds the rates r = 0, 1, ... in that order, adds the 20 states of a site in one fixed order
// (five in the lane, then lane groups 1 apart, then 2 apart), divides and stores.  No floating-point
// atomics, vector stores only, equal inputs give equal bits.  The next operation writes the area
// only behind its own flag barrier, which every wave reaches after its sums.
//
// A consumer that sets kTipBranches is told of tip children too (kernels_preorder.hip's switch): a tip
// has a branch and no outer vector, so `branch` gets y = its table row and t = up (.) pl_sibling and
// the walk goes on to the next child.  With the switch off the walk compiles to what it was.
//
// The derivatives (DerivativeK20; definitions: include/root_digger_amd.h, "Analytic branch-length
// derivatives"): per branch, site and rate  z = Q_r y,  z2 = Q_r z,  25 MFMAs each through the
// forward product, A = an MFMA-ready copy of the normalised rate matrix of set params_indices[r] --
// built on the host (k20_preorder.hpp, k20_pack_copy; proven by tests/cpp/k20_qcopy_check.cpp),
// uploaded in the call frame, staged into LDS by each wave once, in `begin`.  rho_r enters through
// w_r rho_r and w_r rho_r^2.  With d2_out NULL a template flag drops the second product.
// Fixed-order sums, no floating-point atomics: t.y, t.z, t.z2 over the lane's five states in one
// order, the four lane groups by __shfl_xor 16, then 32; each wave leaves its three terms per site
// in LDS, and behind the walk's barrier of the operation wave 0 adds the rates in rate order (lanes
// 0-15: child 0, 16-31: child 1), forms the site terms by site_terms' rule (a site whose f0 is 0 or
// not finite gives zeros and bumps the integer bad_sites counter), adds the tile's 16 sites by a
// butterfly (a lane past S adds zeros) and writes partials[tile][operation][4]; brlen_sum_kernel
// (kernels_preorder.hip) then adds the tiles by increasing number.  Equal inputs give equal bits.
// LDS hazard: `branch` runs before the operation's barrier, and wave 0 adds operation k's terms while
// the other waves already write those of operation k + 1.  The terms are DOUBLE-BUFFERED by
// operation parity, as the flags are; no barrier was added.  Parity p is written again in operation
// k + 2, behind the barrier of operation k + 1, which wave 0 reaches after its reads.
// LDS: the copies (R x 3 200 B) and the terms (R x 1 536 B) live in the exchange area (R x 5 120 B):
// k20_preorder_lds_bytes is unchanged (static_assert in k20_preorder.hpp).
//
// The pair sums (PairSumK20; definitions: include/root_digger_amd.h, "Branch pair sums"): the comment
// above the consumer has the scheme.  It needs a tip child's 0/1 vector, which the walk makes from the
// tip's code and the partition's code masks for a consumer that sets kTipVectors (off: the walk
// compiles to what it was), and it runs in passes over ranges of whole tiles: workgroup b of a launch
// walks tile tile0 + b and writes row b of the pass's partials.  Its two operands are re-dealt by a
// lane permutation (k20_preorder.hpp; proven by tests/cpp/k20_pairsum_check.cpp), not through LDS:
// its LDS is 80 doubles per rate in the exchange area.
//
// Sites past the end: loads are clamped as the forward kernel clamps them (ls, ll: a lane past S reads
// the last site's data, never a tile's padding, which no kernel writes); such lanes store nothing.
//
// Pipelining: plain.  The A copies of the operation's inner children are fetched (global -> wave-
// private LDS, four 16-byte pieces per lane, no barrier) at the start of the operation, together
// with the parent's vector and the children's tiles or table rows; the compiler overlaps those
// independent loads with each other, and other waves of the CU cover the wait.  Nothing of
// operation k + 1 is requested during operation k: no prefetch, no store deferral.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   preorder_k20_walk<256, PosteriorK20>   VGPRs 190   SGPRs 98   scratch 0 B   2 waves per SIMD
//   preorder_k20_walk<512, PosteriorK20>   VGPRs 190   SGPRs 98   scratch 0 B   2 waves per SIMD
//   preorder_k20_walk<256, DerivativeK20<true>>    VGPRs 194   SGPRs 96   scratch 0 B   2 waves per SIMD
//   preorder_k20_walk<512, DerivativeK20<true>>    VGPRs 192   SGPRs 96   scratch 0 B   2 waves per SIMD
//   preorder_k20_walk<256, DerivativeK20<false>>   VGPRs 170   SGPRs 96   scratch 0 B   2 waves per SIMD
//   preorder_k20_walk<512, DerivativeK20<false>>   VGPRs 168   SGPRs 96   scratch 0 B   3 waves per SIMD
//   preorder_k20_walk<256, PairSumK20>     VGPRs 196   SGPRs 95   scratch 0 B   2 waves per SIMD
//   preorder_k20_walk<512, PairSumK20>     VGPRs 198   SGPRs 95   scratch 0 B   2 waves per SIMD
//   LDS (dynamic, k20_preorder_lds_bytes, every consumer): R x 11 520 B + 128 B -- 46 208 B at R = 4, 92 288 B at R = 8
// (the four products of an operation are unrolled side by side: 100 A operands in flight)
#include <algorithm>
#include <mutex>

#include "common.hpp"
#include "k20_preorder.hpp"
#include "outer_plan.hpp"

namespace rdamd {

namespace {

// k20_preorder.hpp restates the dealing of states and the tile without HIP: the same everywhere
constexpr bool k20_layouts_agree() {
  for (unsigned g = 0; g < 4; ++g)
    for (unsigned t = 0; t < 5; ++t)
      if (k20p_state_of(g, t) != k20_state_of(g, t)) return false;
  for (unsigned c = 0; c < 16; ++c)
    for (unsigned s = 0; s < 20; ++s)
      if (k20p_tile_index(c, s) != k20_tile_index(c, s)) return false;
  for (unsigned lane = 0; lane < 64; ++lane)
    for (unsigned t = 0; t < 5; ++t)
      if (k20p_lane_operand(lane, t) != k20_tile_index(lane & 15u, k20_state_of(lane >> 4, t))) return false;
  return true;
}
static_assert(k20_layouts_agree(), "k20_preorder.hpp and common.hpp describe one layout");
static_assert(k20_preorder_lds_bytes(kK20MaxRates) <= kK20LdsLimit, "LDS fits a CU at 8 rate categories");

// what the walk reads and the one thing it writes, the workspace
struct K20WalkArgs {
  const double *clv;          // inner CLVs, [buffer][rate][tile][320]
  size_t clv_stride;          // doubles per buffer
  const uint8_t *tipcodes;
  unsigned tip_stride;
  const double *tiptab;       // [matrix][rate][code][20], rows in operand order
  unsigned ncodes_cap;
  const double *pmfma;        // [matrix][rate][400], the MFMA-ready copies
  const double *freqs;        // [rate matrix][20]
  const unsigned *fidx;       // rate -> frequency set
  const double *rate_w;
  unsigned tips, sites, tiles, R;
  double *work;               // [slot][rate][tile][320]
  const OuterOp *prog;
  unsigned nops;
  unsigned tile0;             // the launch's first tile: workgroup b walks tile tile0 + b
  const uint64_t *codemask;   // [code]: bit j set = state j is allowed (a consumer with kTipVectors)
};

struct K20Lane {
  unsigned lane, col, grp, r, tile, site, ll;   // ll: the lane whose data this lane loads (itself unless past S)
  bool active;                                  // site < S
  double pi[5], w;
};

// a lane's five operands of a tile (the tile's three pieces)
__device__ __forceinline__ void load_tile(const double *tile, unsigned ll, double (&x)[5]) {
  const double2 a = *reinterpret_cast<const double2 *>(tile + k20p_lane_operand(ll, 0));
  const double2 b = *reinterpret_cast<const double2 *>(tile + k20p_lane_operand(ll, 2));
  x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
  x[4] = tile[k20p_lane_operand(ll, 4)];
}
__device__ __forceinline__ void store_tile(double *tile, unsigned lane, const double (&x)[5]) {
  *reinterpret_cast<double2 *>(tile + k20p_lane_operand(lane, 0)) = make_double2(x[0], x[1]);
  *reinterpret_cast<double2 *>(tile + k20p_lane_operand(lane, 2)) = make_double2(x[2], x[3]);
  tile[k20p_lane_operand(lane, 4)] = x[4];
}

// d = P b (kTransposed: P^T b) on the matrix cores, P's staged copy in `copy` (LDS, wave-private)
template <bool kTransposed>
__device__ __forceinline__ void k20_product(const double *copy, unsigned col, unsigned grp, const double (&b)[5],
                                            double (&d)[5]) {
  const double *ap = copy + (kTransposed ? k20_a_transposed(0, 0, col, grp) : k20_a_forward(0, 0, col, grp));
  double a[kK20Groups * kK20Steps];
#pragma unroll
  for (unsigned rg = 0; rg < kK20Groups; ++rg)
#pragma unroll
    for (unsigned ks = 0; ks < kK20Steps; ++ks)   // (block (rg, ks) forward, (ks, rg) transposed: 16 doubles each)
      a[rg * kK20Steps + ks] = ap[kTransposed ? k20_copy_index(ks, rg, 0, 0) : k20_copy_index(rg, ks, 0, 0)];
#pragma unroll
  for (unsigned rg = 0; rg < kK20Groups; ++rg) {
    d[rg] = 0.0;
#pragma unroll
    for (unsigned ks = 0; ks < kK20Steps; ++ks)
      d[rg] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[rg * kK20Steps + ks], b[ks], d[rg], 0, 0, 0);
  }
}

template <int MAXT, class Consumer>   // 64 x rate categories, rounded up to 256 or 512
__global__ void __launch_bounds__(MAXT)
preorder_k20_walk(K20WalkArgs a, typename Consumer::Args ca) {
  extern __shared__ __attribute__((aligned(16))) double k20_lds[];
  const unsigned R = a.R, S = a.sites;
  K20Lane ln;
  ln.lane = threadIdx.x & 63u;
  ln.r = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave = rate
  ln.col = ln.lane & 15u; ln.grp = ln.lane >> 4;
  ln.tile = a.tile0 + blockIdx.x;
  ln.site = ln.tile * 16u + ln.col;
  ln.active = ln.site < S;
  const unsigned ls = ln.active ? ln.site : S - 1u;   // clamped for loads
  ln.ll = ln.grp * 16u + (ls & 15u);
  const unsigned lane = ln.lane, col = ln.col, grp = ln.grp, r = ln.r;
  double *stage = k20_lds + (size_t)r * 2u * kK20CopyDoubles;                      // this wave's two A copies
  double *exchange = k20_lds + (size_t)R * 2u * kK20CopyDoubles;                   // [child][rate][320]
  unsigned *flags = reinterpret_cast<unsigned *>(exchange + (size_t)2u * R * kK20TileDoubles);   // [parity][16]
  {
    const double *f = a.freqs + (size_t)a.fidx[r] * kK20States;
#pragma unroll
    for (unsigned t = 0; t < 5; ++t) ln.pi[t] = f[k20p_state_of(grp, t)];
  }
  ln.w = a.rate_w[r];
  const size_t tile_at = ((size_t)r * a.tiles + ln.tile) * kK20TileDoubles;        // this wave's tile in a CLV or a slot
  const size_t slot_doubles = (size_t)R * a.tiles * kK20TileDoubles;

  Consumer con(ca, exchange, R);
  con.begin(a, ln, tile_at);

  double u[5] = {0, 0, 0, 0, 0};   // the outer vector the next operation reads from registers
  for (unsigned k = 0; k < a.nops; ++k) {
    const OuterOp op = a.prog[k];
    con.op_begin(ln, k);
    // the A copies of the inner children: 3200 contiguous bytes each, global -> this wave's LDS
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (!op.inner[c]) continue;   // (wave-uniform)
      const double2 *src = reinterpret_cast<const double2 *>(a.pmfma + ((size_t)op.child_mat[c] * R + r) * kK20CopyDoubles);
      double2 *dst = reinterpret_cast<double2 *>(stage + (unsigned)c * kK20CopyDoubles);
#pragma unroll
      for (unsigned e = 0; e < 4; ++e) {
        const unsigned at = lane + 64u * e;
        if (at < kK20CopyDoubles / 2u) dst[at] = src[at];
      }
    }
    double up[5];
    if (op.parent_src == kOuterFromSlot) {
      load_tile(a.work + (size_t)op.parent_slot * slot_doubles + tile_at, ln.ll, up);
    } else {
#pragma unroll
      for (int t = 0; t < 5; ++t) up[t] = op.parent_src == kOuterFromPi ? ln.pi[t] : u[t];
    }
    // the children: an inner child's CLV tile, a tip's finished term P . (0/1 vector) from its table row
    double l[2][5], pl[2][5];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (op.inner[c]) {
        load_tile(a.clv + (size_t)(op.child_clv[c] - a.tips) * a.clv_stride + tile_at, ln.ll, l[c]);
      } else {
        const unsigned code = a.tipcodes[(size_t)op.child_clv[c] * a.tip_stride + ls];
        const double *row = a.tiptab + (((size_t)op.child_mat[c] * R + r) * a.ncodes_cap + code) * kK20States;
        const double2 p01 = *reinterpret_cast<const double2 *>(row + grp * 2u);
        const double2 p23 = *reinterpret_cast<const double2 *>(row + 8u + grp * 2u);
        pl[c][0] = p01.x; pl[c][1] = p01.y; pl[c][2] = p23.x; pl[c][3] = p23.y;
        pl[c][4] = row[16u + grp];
        if constexpr (Consumer::kTipVectors) {   // the tip's 0/1 vector over the lane's five states
          const uint64_t mask = a.codemask[code];
#pragma unroll
          for (unsigned t = 0; t < 5; ++t) l[c][t] = (double)((mask >> k20p_state_of(grp, t)) & 1u);
        } else {
#pragma unroll
          for (int t = 0; t < 5; ++t) l[c][t] = 0.0;   // (never read: a tip has no outer vector here)
        }
      }
    }
    __builtin_amdgcn_wave_barrier();   // the staged copies are read by other lanes of this wave than wrote them
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (op.inner[c]) k20_product<false>(stage + (unsigned)c * kK20CopyDoubles, col, grp, l[c], pl[c]);
    // the children's outer vectors, and which sites of this rate are small
    double uc[2][5];
    unsigned bits = 0u;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (!op.inner[c] && !Consumer::kTipBranches) continue;   // (wave-uniform)
      double t[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) t[i] = up[i] * pl[1 - c][i];   // the parent's vector masked by the sibling
      con.branch(ln, c, t, pl[c], l[c]);
      if constexpr (Consumer::kTipBranches) {
        if (!op.inner[c]) continue;   // a tip has a branch and no outer vector
      }
      k20_product<true>(stage + (unsigned)c * kK20CopyDoubles, col, grp, t, uc[c]);
      const double m = fmax(fmax(fmax(uc[c][0], uc[c][1]), fmax(uc[c][2], uc[c][3])), uc[c][4]);
      // across the four lane groups that hold the other states of a site (bit s = site s of the wave)
      unsigned long long bm = __builtin_amdgcn_ballot_w64(m < kScaleThreshold);
      bm &= bm >> 32;
      bm &= bm >> 16;
      bits |= ((unsigned)bm & 0xFFFFu) << (16 * c);
    }
    __builtin_amdgcn_wave_barrier();   // (the next operation's copies land only behind these reads)
    if (lane == 0) flags[(k & 1u) * 16u + r] = bits;
    __syncthreads();
    unsigned all_bits = ~0u;
    for (unsigned q = 0; q < R; ++q) all_bits &= flags[(k & 1u) * 16u + q];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (!op.inner[c]) continue;
      if ((all_bits >> (16 * c + (int)col)) & 1u) {
#pragma unroll
        for (int j = 0; j < 5; ++j) uc[c][j] *= kScaleFactor;
      }
      con.outer(ln, c, op.node[c], uc[c], l[c]);
      if (op.keep[c] == kOuterKeepReg) {
#pragma unroll
        for (int j = 0; j < 5; ++j) u[j] = uc[c][j];
      } else if (op.keep[c] == kOuterKeepSlot && ln.active) {
        store_tile(a.work + (size_t)op.slot[c] * slot_doubles + tile_at, lane, uc[c]);
      }
    }
    con.op_end(a, ln, op.inner[0] != 0u, op.inner[1] != 0u);
  }
  con.end(ln);
}

// ---------------------------------------------------------------------------
// Consumer: marginal ancestral state posteriors
// ---------------------------------------------------------------------------
struct PosteriorK20Args {
  double *post;   // [node][site][20]
};

struct PosteriorK20 {
  using Args = PosteriorK20Args;
  static constexpr bool kTipBranches = false, kTipVectors = false;
  const Args c;
  double *const exchange;   // [child][rate][t][lane]
  const unsigned R;
  unsigned node[2] = {0u, 0u};
  __device__ __forceinline__ PosteriorK20(const Args &c, double *exchange, unsigned R) : c(c), exchange(exchange), R(R) {}

  // this wave's terms w_r U L of one node
  __device__ __forceinline__ void put(const K20Lane &ln, int ch, const double (&u)[5], const double (&l)[5]) const {
    double *o = exchange + ((size_t)ch * R + ln.r) * kK20TileDoubles + ln.lane;
#pragma unroll
    for (int t = 0; t < 5; ++t) o[64 * t] = ln.w * u[t] * l[t];
  }
  // (behind a barrier) one wave: the rates in order, the states of a site in one fixed order, the division
  __device__ __forceinline__ void sum_and_store(const K20WalkArgs &a, const K20Lane &ln, int ch, unsigned nd) const {
    double q[5] = {0, 0, 0, 0, 0};
    for (unsigned r = 0; r < R; ++r) {
      const double *o = exchange + ((size_t)ch * R + r) * kK20TileDoubles + ln.lane;
#pragma unroll
      for (int t = 0; t < 5; ++t) q[t] += o[64 * t];
    }
    double den = ((q[0] + q[1]) + (q[2] + q[3])) + q[4];
    den += __shfl_xor(den, 16);
    den += __shfl_xor(den, 32);
    if (!ln.active) return;
    double *o = c.post + ((size_t)nd * a.sites + ln.site) * kK20States;
#pragma unroll
    for (unsigned t = 0; t < 5; ++t) o[k20p_state_of(ln.grp, t)] = q[t] / den;
  }
  __device__ __forceinline__ void begin(const K20WalkArgs &a, const K20Lane &ln, size_t tile_at) const {   // the root: U = pi
    double l[5];
    load_tile(a.clv + (size_t)(a.prog[0].parent_clv - a.tips) * a.clv_stride + tile_at, ln.ll, l);
    put(ln, 0, ln.pi, l);
    __syncthreads();
    if (ln.r == 0u) sum_and_store(a, ln, 0, 0u);
  }
  __device__ __forceinline__ void op_begin(const K20Lane &, unsigned) const {}
  __device__ __forceinline__ void branch(const K20Lane &, int, const double (&)[5], const double (&)[5],
                                         const double (&)[5]) const {}
  __device__ __forceinline__ void outer(const K20Lane &ln, int ch, unsigned nd, const double (&uc)[5], const double (&l)[5]) {
    node[ch] = nd;
    put(ln, ch, uc, l);
  }
  // every wave of the workgroup comes here with the same two flags
  __device__ __forceinline__ void op_end(const K20WalkArgs &a, const K20Lane &ln, bool inner0, bool inner1) const {
    if (!inner0 && !inner1) return;
    __syncthreads();
    if (inner0 && ln.r == 0u) sum_and_store(a, ln, 0, node[0]);
    if (inner1 && ln.r == 1u % R) sum_and_store(a, ln, 1, node[1]);
  }
  __device__ __forceinline__ void end(const K20Lane &) const {}
};

// ---------------------------------------------------------------------------
// Consumer: first and second derivative of lnL in every branch length
// ---------------------------------------------------------------------------
struct DerivativeK20Args {
  const double *qcopy;        // [rate][400]: the MFMA-ready copy of the rate matrix of set params_indices[rate]
  const double *rates;
  const unsigned *pattern_w;
  double *partials;           // [tile][nops][4]: d1, d2 of child 0, d1, d2 of child 1
  unsigned *bad_sites;        // sites whose likelihood is 0 or not finite
};

// kSecond = false: no z2 = Q z; the d2 entries of the partials are then formed from f2 = 0 and nobody reads them
template <bool kSecond>
struct DerivativeK20 {
  using Args = DerivativeK20Args;
  static constexpr bool kTipBranches = true, kTipVectors = false;
  const Args c;
  double *const exchange;   // k20_preorder.hpp: [rate][400] rate-matrix copies, then [parity][child][rate][3][16] terms
  const unsigned R;
  double w1 = 0.0, w2 = 0.0, weight = 0.0;
  unsigned k = 0;           // the operation under way
  bool site_bad = false;
  __device__ __forceinline__ DerivativeK20(const Args &c, double *exchange, unsigned R) : c(c), exchange(exchange), R(R) {}

  // each wave stages the copy of its own rate's matrix, once; the walk's wave barrier of the first
  // operation stands between these writes and the first read
  __device__ __forceinline__ void begin(const K20WalkArgs &a, const K20Lane &ln, size_t) {
    const double rho = c.rates[ln.r];
    w1 = ln.w * rho; w2 = w1 * rho;
    weight = (double)c.pattern_w[ln.active ? ln.site : a.sites - 1u];
    const double2 *src = reinterpret_cast<const double2 *>(c.qcopy + (size_t)ln.r * kK20CopyDoubles);
    double2 *dst = reinterpret_cast<double2 *>(exchange + (size_t)ln.r * kK20CopyDoubles);
#pragma unroll
    for (unsigned e = 0; e < 4; ++e) {
      const unsigned at = ln.lane + 64u * e;
      if (at < kK20CopyDoubles / 2u) dst[at] = src[at];
    }
  }
  __device__ __forceinline__ void op_begin(const K20Lane &, unsigned op) { k = op; }
  // this rate's three terms of branch (k, ch), every site of the tile: the five states of the lane in
  // one fixed order, then the lane groups 16 and 32 apart
  __device__ __forceinline__ void branch(const K20Lane &ln, int ch, const double (&t)[5], const double (&y)[5],
                                         const double (&)[5]) const {
    const double *qc = exchange + (size_t)ln.r * kK20CopyDoubles;
    double z[5];
    k20_product<false>(qc, ln.col, ln.grp, y, z);
    double p0 = ((t[0] * y[0] + t[1] * y[1]) + (t[2] * y[2] + t[3] * y[3])) + t[4] * y[4];
    double p1 = ((t[0] * z[0] + t[1] * z[1]) + (t[2] * z[2] + t[3] * z[3])) + t[4] * z[4];
    double p2 = 0.0;
    if constexpr (kSecond) {
      double z2[5];
      k20_product<false>(qc, ln.col, ln.grp, z, z2);
      p2 = ((t[0] * z2[0] + t[1] * z2[1]) + (t[2] * z2[2] + t[3] * z2[3])) + t[4] * z2[4];
    }
    p0 += __shfl_xor(p0, 16); p0 += __shfl_xor(p0, 32);
    p1 += __shfl_xor(p1, 16); p1 += __shfl_xor(p1, 32);
    if constexpr (kSecond) { p2 += __shfl_xor(p2, 16); p2 += __shfl_xor(p2, 32); }
    if (ln.grp == 0u) {
      double *f = exchange + k20_brlen_term_index(R, k & 1u, (unsigned)ch, ln.r, 0u, ln.col);
      f[0] = ln.w * p0; f[16] = w1 * p1; f[32] = w2 * p2;
    }
  }
  __device__ __forceinline__ void outer(const K20Lane &, int, unsigned, const double (&)[5], const double (&)[5]) const {}
  // Behind the walk's barrier of operation k the terms of all rates are there.  Wave 0 adds them in
  // rate order -- lanes 0-15 child 0, lanes 16-31 child 1, one site each --, forms the site terms,
  // adds the 16 sites of the tile by a butterfly and writes the tile's four partials.  The other
  // waves go on to operation k + 1 and write the OTHER parity; the parity of operation k is written
  // again only behind the barrier of operation k + 1, which wave 0 reaches after these reads.
  __device__ __forceinline__ void op_end(const K20WalkArgs &a, const K20Lane &ln, bool, bool) {
    if (ln.r != 0u) return;   // (wave-uniform)
    const unsigned ch = (ln.lane >> 4) & 1u;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    for (unsigned r = 0; r < R; ++r) {
      const double *f = exchange + k20_brlen_term_index(R, k & 1u, ch, r, 0u, ln.col);
      f0 += f[0]; f1 += f[16]; f2 += f[32];
    }
    double d1, d2;
    const bool ok = site_terms(f0, f1, f2, weight, &d1, &d2);
    if (!ln.active) { d1 = 0.0; d2 = 0.0; }   // (a lane past S formed its terms from the last site's data)
    else if (!ok && ln.lane < 32u) site_bad = true;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      d1 += __shfl_xor(d1, off);
      d2 += __shfl_xor(d2, off);
    }
    if (ln.lane < 32u && ln.col == 0u) {
      double *o = c.partials + ((size_t)ln.tile * a.nops + k) * 4u + 2u * ch;
      o[0] = d1; o[1] = d2;
    }
  }
  // a site is counted once, whichever of its branches found it
  __device__ __forceinline__ void end(const K20Lane &ln) const {
    if (ln.r != 0u) return;
    const bool other = __shfl_xor((int)site_bad, 16) != 0;
    if (ln.lane < 16u && (site_bad || other)) atomicAdd(c.bad_sites, 1u);
  }
};

// ---------------------------------------------------------------------------
// Consumer: pair sums -- the derivative of lnL in every entry of every P-matrix
// ---------------------------------------------------------------------------
// Definitions: kernels_preorder.hip, above PairSumDna, with 20 states.  Per branch each wave leaves
// w_r t.(P_a L_a) per site in LDS (`branch`, before the operation's barrier; double-buffered by
// operation parity as the derivative consumer's terms are, for the same hazard) and keeps t and L_a
// in registers.  Behind the barrier (op_end) every wave adds the rates in rate order, scales its t by
// weight_s w_r / f0(s) (0 for a site without a likelihood and for a lane past S), re-deals both
// vectors by the lane permutation k20_pair_source_lane so that the SITE becomes the reduction
// dimension, and forms the wave's 20 x 20 sum over its 16 sites as 25 MFMAs, the four blocks of each
// being the four quads of sites.  Order of a sum: the MFMA's own over the four sites of a quad, the
// quads by __shfl_xor 4, then 8, one partial per (tile, entry), pair_sum_kernel over the tiles by
// increasing number.  M, W: each wave its own rate, froot summed over the rates in rate order through
// LDS in `begin`, the 16 sites by a butterfly (1, 2, 4, 8).  No floating-point atomics, vector stores only.
struct PairSumK20Args {
  const unsigned *pattern_w;
  double *partials;           // [tile of the pass][k20_pair_sum_entries]
  unsigned *bad_sites;        // sites whose likelihood is 0 or not finite
};

struct PairSumK20 {
  using Args = PairSumK20Args;
  static constexpr bool kTipBranches = true, kTipVectors = true;
  const Args c;
  double *const exchange;   // k20_preorder.hpp: [parity][child][rate][16] branch terms, then [rate][16] root terms
  const unsigned R;
  double weight = 0.0;
  double ts[2][5], ls[2][5];   // t and L_a of the operation's two branches, until its barrier has passed
  double *row = nullptr;       // this tile's row of partials
  unsigned k = 0;
  bool site_bad = false;
  __device__ __forceinline__ PairSumK20(const Args &c, double *exchange, unsigned R) : c(c), exchange(exchange), R(R) {}

  // the five states of the lane in one fixed order, then the lane groups 16 and 32 apart
  static __device__ __forceinline__ double site_dot(const double (&x)[5], const double (&y)[5]) {
    double p = ((x[0] * y[0] + x[1] * y[1]) + (x[2] * y[2] + x[3] * y[3])) + x[4] * y[4];
    p += __shfl_xor(p, 16);
    p += __shfl_xor(p, 32);
    return p;
  }
  // weight / (the terms of all rates in rate order) of the lane's site; 0 for a lane past S
  __device__ __forceinline__ double factor(const K20Lane &ln, const double *terms) {
    double f = 0.0, g;
    for (unsigned q = 0; q < R; ++q) f += terms[16u * q];
    const bool ok = site_factor(f, weight, &g);
    if (!ln.active) g = 0.0;
    else if (!ok) site_bad = true;
    return g;
  }
  __device__ __forceinline__ void begin(const K20WalkArgs &a, const K20Lane &ln, size_t tile_at) {
    weight = (double)c.pattern_w[ln.active ? ln.site : a.sites - 1u];
    row = c.partials + (size_t)blockIdx.x * k20_pair_sum_entries(a.nops, R);
    double l[5];
    load_tile(a.clv + (size_t)(a.prog[0].parent_clv - a.tips) * a.clv_stride + tile_at, ln.ll, l);
    const double dot = site_dot(ln.pi, l);
    if (ln.grp == 0u) exchange[k20_pair_root_index(R, ln.r, ln.col)] = ln.w * dot;
    __syncthreads();
    const double g = factor(ln, exchange + k20_pair_root_index(R, 0u, ln.col));
    const double gw = g * ln.w;
    double m[5], wv = g * dot;
#pragma unroll
    for (int t = 0; t < 5; ++t) m[t] = gw * l[t];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
      for (int t = 0; t < 5; ++t) m[t] += __shfl_xor(m[t], off);
      wv += __shfl_xor(wv, off);
    }
    if (ln.col == 0u) {
      double *o = row + k20_pair_root_at(a.nops, R) + (size_t)ln.r * (kK20States + 1u);
#pragma unroll
      for (unsigned t = 0; t < 5; ++t) o[k20p_state_of(ln.grp, t)] = m[t];
      if (ln.grp == 0u) o[kK20States] = wv;
    }
  }
  __device__ __forceinline__ void op_begin(const K20Lane &, unsigned op) { k = op; }
  __device__ __forceinline__ void branch(const K20Lane &ln, int ch, const double (&t)[5], const double (&y)[5],
                                         const double (&l)[5]) {
    const double p0 = site_dot(t, y);
    if (ln.grp == 0u) exchange[k20_pair_term_index(R, k & 1u, (unsigned)ch, ln.r, ln.col)] = ln.w * p0;
#pragma unroll
    for (int i = 0; i < 5; ++i) { ts[ch][i] = t[i]; ls[ch][i] = l[i]; }
  }
  __device__ __forceinline__ void outer(const K20Lane &, int, unsigned, const double (&)[5], const double (&)[5]) const {}
  // Behind the walk's barrier of operation k the terms of all rates are there; every wave reads them.
  // Parity k & 1 is written again in operation k + 2, behind the barrier of operation k + 1, which
  // every wave reaches after these reads.
  __device__ __forceinline__ void op_end(const K20WalkArgs &, const K20Lane &ln, bool, bool) {
    const int src = (int)k20_pair_source_lane(ln.lane);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const double gw = factor(ln, exchange + k20_pair_term_index(R, k & 1u, (unsigned)ch, 0u, ln.col)) * ln.w;
      double av[5], bv[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        av[i] = __shfl(gw * ts[ch][i], src);
        bv[i] = __shfl(ls[ch][i], src);
      }
      double *o = row + (((size_t)k * 2u + (unsigned)ch) * R + ln.r) * (kK20States * kK20States);
#pragma unroll
      for (unsigned ib = 0; ib < 5; ++ib)
#pragma unroll
        for (unsigned jb = 0; jb < 5; ++jb) {
          double n = __builtin_amdgcn_mfma_f64_4x4x4f64(av[ib], bv[jb], 0.0, 0, 0, 0);
          n += __shfl_xor(n, 4);
          n += __shfl_xor(n, 8);
          if (ln.col < 4u) o[k20_pair_entry(ln.lane, ib, jb)] = n;
        }
    }
  }
  // a site is counted once, whichever of its branches found it (every wave finds the same sites)
  __device__ __forceinline__ void end(const K20Lane &ln) const {
    if (ln.r == 0u && ln.lane < 16u && site_bad) atomicAdd(c.bad_sites, 1u);
  }
};

// state[row] = the smallest index among the largest of post[row][0..K), prob[row] = that posterior.
// A workgroup's 256 rows come through LDS: the loads are contiguous over the workgroup (a lane
// reading its own row would stride 8 K bytes from its neighbour: measured 0.66 ms for c3's 318 MB),
// then one lane scans one row, rows an odd number of doubles apart so that they spread over the banks.
constexpr unsigned kArgmaxRows = 256;
__host__ __device__ constexpr unsigned argmax_pitch(unsigned K) { return K | 1u; }

__global__ void __launch_bounds__(kArgmaxRows)
ancestral_argmax_kernel(const double *__restrict__ post, size_t rows, unsigned K, uint8_t *__restrict__ state,
                        double *__restrict__ prob) {
  extern __shared__ __attribute__((aligned(16))) double argmax_lds[];   // [256][argmax_pitch(K)]
  const size_t row0 = (size_t)blockIdx.x * kArgmaxRows;
  const unsigned n = rows - row0 < kArgmaxRows ? (unsigned)(rows - row0) : kArgmaxRows;   // rows of this workgroup
  const unsigned pitch = argmax_pitch(K);
  const double *src = post + row0 * K;
  for (unsigned e = threadIdx.x; e < n * K; e += kArgmaxRows) argmax_lds[(e / K) * pitch + e % K] = src[e];
  __syncthreads();
  if (threadIdx.x >= n) return;
  const size_t row = row0 + threadIdx.x;
  const double *p = argmax_lds + threadIdx.x * pitch;
  double best = p[0];
  unsigned at = 0;
  for (unsigned j = 1; j < K; ++j) {
    const double v = p[j];
    if (v > best) { best = v; at = j; }
  }
  state[row] = (uint8_t)at;
  prob[row] = best;
}

}  // namespace

// the walk of one consumer over the whole program, one workgroup per tile: tiles tile0 .. tile0 + ntiles - 1
// (ntiles 0: all of them)
template <class Consumer>
static hipError_t launch_k20_walk(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, const unsigned *d_fidx, double *d_work,
                           const typename Consumer::Args &ca, unsigned tile0 = 0, unsigned ntiles = 0) {
  const unsigned R = p->rate_cats;
  if (!p->mfma_layout || R > kK20MaxRates) return hipErrorInvalidValue;
  if (ntiles == 0) ntiles = p->clv_tiles() - tile0;
  if (tile0 >= p->clv_tiles() || ntiles > p->clv_tiles() - tile0) return hipErrorInvalidValue;
  K20WalkArgs a;
  a.clv = p->d_clv; a.clv_stride = p->clv_doubles();
  a.tipcodes = p->d_tipcodes; a.tip_stride = p->tip_stride();
  a.tiptab = p->d_tiptab; a.ncodes_cap = p->ncodes_cap;
  a.pmfma = p->d_pmat_mfma; a.freqs = p->d_freqs; a.fidx = d_fidx; a.rate_w = p->d_rate_weights;
  a.tips = p->tips; a.sites = p->sites; a.tiles = p->clv_tiles(); a.R = R;
  a.work = d_work; a.prog = d_prog; a.nops = nops;
  a.tile0 = tile0; a.codemask = p->d_codemask;
  const size_t lds = k20_preorder_lds_bytes(R);
  if (R <= 4) {
    preorder_k20_walk<256, Consumer><<<ntiles, 64 * R, lds, p->stream>>>(a, ca);
  } else {
    {   // six categories and up pass the 64 KB a kernel may ask for by default
      static std::mutex lds_mu;
      static bool lds_allowed = false;   // (one per consumer)
      std::lock_guard<std::mutex> guard(lds_mu);
      if (!lds_allowed) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&preorder_k20_walk<512, Consumer>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)k20_preorder_lds_bytes(kK20MaxRates));
        if (e != hipSuccess) return e;
        lds_allowed = true;
      }
    }
    preorder_k20_walk<512, Consumer><<<ntiles, 64 * R, lds, p->stream>>>(a, ca);
  }
  return hipGetLastError();
}

hipError_t launch_outer_program_k20(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, const unsigned *d_fidx,
                                    double *d_work, double *d_post) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  return launch_k20_walk<PosteriorK20>(p, d_prog, nops, d_fidx, d_work, PosteriorK20Args{d_post});
}

hipError_t launch_brlen_program_k20(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, const unsigned *d_fidx,
                                    double *d_work, const double *d_qcopy, double *d_partials, unsigned *d_bad_sites,
                                    bool second, double *d_out) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  const DerivativeK20Args ca{d_qcopy, p->d_rates, p->d_pattern_weights, d_partials, d_bad_sites};
  const hipError_t e = second ? launch_k20_walk<DerivativeK20<true>>(p, d_prog, nops, d_fidx, d_work, ca)
                              : launch_k20_walk<DerivativeK20<false>>(p, d_prog, nops, d_fidx, d_work, ca);
  if (e != hipSuccess) return e;
  return launch_brlen_sum(p, d_partials, p->clv_tiles(), nops * 4u, d_out);
}

hipError_t launch_pair_sum_program_k20(rdamd_partition *p, const OuterOp *d_prog, unsigned nops, const unsigned *d_fidx,
                                       double *d_work, double *d_partials, unsigned tiles_per_pass, unsigned *d_bad_sites,
                                       double *d_out) {
  if (nops == 0 || p->sites == 0) return hipSuccess;
  if (tiles_per_pass == 0) return hipErrorInvalidValue;
  const unsigned tiles = p->clv_tiles();
  const size_t entries = k20_pair_sum_entries(nops, p->rate_cats);
  const PairSumK20Args ca{p->d_pattern_weights, d_partials, d_bad_sites};
  for (unsigned t0 = 0; t0 < tiles; t0 += tiles_per_pass) {
    const unsigned nt = std::min(tiles_per_pass, tiles - t0);
    hipError_t e = launch_k20_walk<PairSumK20>(p, d_prog, nops, d_fidx, d_work, ca, t0, nt);
    if (e == hipSuccess) e = launch_pair_sum_fold(p, d_partials, nt, entries, t0 == 0, d_out);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_ancestral_argmax(rdamd_partition *p, const double *d_post, size_t rows, unsigned K, uint8_t *d_state,
                                   double *d_prob) {
  if (rows == 0) return hipSuccess;
  const size_t blocks = (rows + 255) / 256;
  if (blocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
  const size_t lds = (size_t)kArgmaxRows * argmax_pitch(K) * sizeof(double);
  if (lds > 64 * 1024) return hipErrorInvalidValue;   // (no caller: 2, 4 and 20 states reach here, 43 KB at most)
  ancestral_argmax_kernel<<<(unsigned)blocks, kArgmaxRows, lds, p->stream>>>(d_post, rows, K, d_state, d_prob);
  return hipGetLastError();
}

}  // namespace rdamd
