// C ABI: partition life cycle, setters and the three hot-path entry points.
// Mirrors the coraxlib subset RootDigger calls; each
// function cites the call site it replaces in include/root_digger_amd.h.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

#include <dlfcn.h>

#include "clades.hpp"
#include "clv_plan.hpp"
#include "common.hpp"
#include "k20_preorder.hpp"
#include "outer_plan.hpp"
#include "subst_map.hpp"
#include "tip_encode.hpp"

namespace rdamd {

static thread_local int  g_errno = 0;
static thread_local char g_errmsg[512] = "";

void set_error(int code, const char *fmt, ...) {
  g_errno = code;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_errmsg, sizeof(g_errmsg), fmt, ap);
  va_end(ap);
}
void clear_error() { g_errno = 0; g_errmsg[0] = 0; }

// Small host->device copies go through a pinned ring so they can be queued on
// the partition's stream without a blocking pageable copy.
static void *stage_alloc(rdamd_partition *p, size_t bytes) {
  bytes = (bytes + 255) & ~(size_t)255;
  if (p->stage_off + bytes > p->stage_bytes) {
    (void)hipStreamSynchronize(p->stream);
    p->stage_off = 0;
  }
  void *r = p->h_stage + p->stage_off;
  p->stage_off += bytes;
  return r;
}

// upload `bytes` from host memory to `dst` on the partition stream
static hipError_t upload(rdamd_partition *p, void *dst, const void *src, size_t bytes) {
  if (bytes == 0) return hipSuccess;
  if (bytes > p->stage_bytes / 2) {  // large: plain blocking copy
    hipError_t e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return e;
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  }
  void *st = stage_alloc(p, bytes);
  memcpy(st, src, bytes);
  p->stream_dirty = true;
  return hipMemcpyAsync(dst, st, bytes, hipMemcpyHostToDevice, p->stream);
}

// device scratch carve-out (bump; reset per API call)
struct Scratch {
  rdamd_partition *p;
  size_t off = 0;
  void *take(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (off + bytes > p->scratch_bytes) return nullptr;
    void *r = (char *)p->d_scratch + off;
    off += bytes;
    return r;
  }
};

static hipError_t ensure_scratch(rdamd_partition *p, size_t bytes) {
  if (bytes <= p->scratch_bytes) return hipSuccess;
  hipError_t e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess) return e;
  if (p->d_scratch) (void)hipFree(p->d_scratch);
  p->d_scratch = nullptr;
  p->scratch_bytes = 0;
  size_t want = std::max(bytes * 2, (size_t)1 << 20);
  e = hipMalloc(&p->d_scratch, want);
  if (e == hipSuccess) p->scratch_bytes = want;
  return e;
}

static hipError_t flush_q(rdamd_partition *p) {
  const unsigned K = p->states;
  std::vector<double> q((size_t)K * K);
  for (unsigned i = 0; i < p->rate_matrices; ++i) {
    if (!p->q_dirty[i]) continue;
    build_q_host(K, p->subst[i].data(), p->freqs[i].data(), q.data());
    hipError_t e = upload(p, p->d_q + (size_t)i * K * K, q.data(), sizeof(double) * K * K);
    if (e != hipSuccess) return e;
    e = upload(p, p->d_freqs + (size_t)i * K, p->freqs[i].data(), sizeof(double) * K);
    if (e != hipSuccess) return e;
    p->q_dirty[i] = 0;
  }
  return hipSuccess;
}

}  // namespace rdamd

hipEvent_t rdamd_partition::prof_begin(int kind) {
  stream_dirty = true;   // (every launch of the partition passes here)
  if (!profiling) return nullptr;
  hipEvent_t ev[2];
  for (auto &e : ev) {
    if (!prof_pool.empty()) { e = prof_pool.back(); prof_pool.pop_back(); }
    else if (hipEventCreate(&e) != hipSuccess) return nullptr;
  }
  (void)hipEventRecord(ev[0], stream);
  prof_spans.push_back({ev[0], ev[1], kind});
  return ev[1];
}
void rdamd_partition::prof_end() {
  if (!profiling || prof_spans.empty()) return;
  (void)hipEventRecord(prof_spans.back().b, stream);
}

using namespace rdamd;


namespace rdamd {
// one more slot of a sparse pool: a bigger block, the live slots copied over (everything queued
// on the partition has drained first -- kernels in flight hold the old addresses)
static hipError_t grow_pool(rdamd_partition *p, bool scalers) {
  unsigned &cap = scalers ? p->sc_slots_cap : p->clv_slots_cap;
  const unsigned used = scalers ? p->sc_slots_used : p->clv_slots_used;
  const unsigned limit = scalers ? p->scale_buffers : p->clv_buffers;
  const size_t slot_bytes = scalers ? (size_t)p->sites * sizeof(unsigned) : p->clv_doubles() * sizeof(double);
  const unsigned fresh_cap = std::min(limit, std::max(cap * 2u, 4u));
  if (fresh_cap <= cap) return hipErrorOutOfMemory;   // (cannot happen: a pool never holds more slots than indices)
  hipError_t e = sync_streams(p);
  if (e != hipSuccess) return e;
  void *fresh = nullptr;
  e = hipMalloc(&fresh, std::max<size_t>(8, (size_t)fresh_cap * slot_bytes));
  if (e != hipSuccess) return e;
  void *old = scalers ? (void *)p->d_scaler : (void *)p->d_clv;
  if (used && slot_bytes) e = hipMemcpy(fresh, old, (size_t)used * slot_bytes, hipMemcpyDeviceToDevice);
  if (e != hipSuccess) { (void)hipFree(fresh); return e; }
  (void)hipFree(old);
  if (scalers) p->d_scaler = (unsigned *)fresh; else p->d_clv = (double *)fresh;
  cap = fresh_cap;
  return hipSuccess;
}

hipError_t clv_phys(rdamd_partition *p, unsigned clv_index, unsigned *phys) {
  if (clv_index >= p->tips + p->clv_buffers) return hipErrorInvalidValue;
  *phys = clv_index;
  if (!p->sparse || clv_index < p->tips) return hipSuccess;
  int &slot = p->clv_slot[clv_index - p->tips];
  if (slot < 0) {
    if (p->clv_slots_used == p->clv_slots_cap) {
      hipError_t e = grow_pool(p, false);
      if (e != hipSuccess) return e;
    }
    slot = (int)p->clv_slots_used++;
  }
  *phys = p->tips + (unsigned)slot;
  return hipSuccess;
}

hipError_t scaler_phys(rdamd_partition *p, int scaler_index, int *phys) {
  if (scaler_index >= (int)p->scale_buffers) return hipErrorInvalidValue;
  *phys = scaler_index;
  if (!p->sparse || scaler_index < 0) return hipSuccess;
  int &slot = p->sc_slot[(size_t)scaler_index];
  if (slot < 0) {
    if (p->sc_slots_used == p->sc_slots_cap) {
      hipError_t e = grow_pool(p, true);
      if (e != hipSuccess) return e;
    }
    slot = (int)p->sc_slots_used++;
    // a scale buffer nobody has written reads as zeros, as in a dense partition
    p->stream_dirty = true;
    hipError_t e = hipMemsetAsync(p->d_scaler + (size_t)slot * p->sites, 0, (size_t)p->sites * sizeof(unsigned), p->stream);
    if (e != hipSuccess) return e;
  }
  *phys = slot;
  return hipSuccess;
}

hipError_t op_phys(rdamd_partition *p, const rdamd_operation_t &o, rdamd_operation_t *out) {
  *out = o;
  if (!p->sparse) return hipSuccess;
  if (o.parent_clv_index < p->tips) return hipErrorInvalidValue;
  hipError_t e = clv_phys(p, o.parent_clv_index, &out->parent_clv_index);
  if (e == hipSuccess) e = clv_phys(p, o.child1_clv_index, &out->child1_clv_index);
  if (e == hipSuccess) e = clv_phys(p, o.child2_clv_index, &out->child2_clv_index);
  if (e == hipSuccess) e = scaler_phys(p, o.parent_scaler_index, &out->parent_scaler_index);
  if (e == hipSuccess) e = scaler_phys(p, o.child1_scaler_index, &out->child1_scaler_index);
  if (e == hipSuccess) e = scaler_phys(p, o.child2_scaler_index, &out->child2_scaler_index);
  return e;
}

// ---- what several entry points check or do in the same way -----------------------------------
static bool op_in_range(const rdamd_partition *p, const rdamd_operation_t &o) {
  return operation_in_range(o, p->tips, p->clv_buffers, p->prob_matrices, p->scale_buffers);
}
// the first of the per-rate-category indices (rate matrix / frequency set) that names no rate
// matrix of the partition, or null
static const unsigned *bad_rate_index(const rdamd_partition *p, const unsigned *indices) {
  for (unsigned r = 0; r < p->rate_cats; ++r)
    if (indices[r] >= p->rate_matrices) return indices + r;
  return nullptr;
}
static bool length_ok(double l) { return l >= 0.0 && std::isfinite(l); }
// a root CLV and its scaler as the root calls take them: an inner CLV; a scale buffer or none (< 0)
static bool root_index_ok(const rdamd_partition *p, unsigned clv_index, int scaler_index) {
  return clv_index >= p->tips && clv_index < p->tips + p->clv_buffers && scaler_index < (int)p->scale_buffers;
}
// tip tables made for an older set of state codes are rebuilt before a kernel reads them
static hipError_t flush_tiptab(rdamd_partition *p) {
  if (!p->tiptab_stale) return hipSuccess;
  p->stream_dirty = true;
  const hipError_t e = launch_tiptab_all(p);
  if (e == hipSuccess) p->tiptab_stale = false;
  return e;
}
// shapes the single-launch root kernels take (root_single_dna_kernel, root_multi_dna_kernel)
static bool fast_root_shape(const rdamd_partition *p, const rdamd_operation_t &root_op) {
  const unsigned R = p->rate_cats;
  return p->states == 4 && p->ncodes_cap == 16 && (R == 1 || R == 2 || R == 4 || R == 8) &&
         root_op.parent_scaler_index >= 0;
}

// What the two lnL calls do before their launch: parameters flushed, scratch for the frequency
// indices and `extra` bytes more, the indices uploaded (d_fi: the first take of `sc`) ...
static hipError_t stage_root_lnl(rdamd_partition *p, const unsigned *freqs_indices, size_t extra, Scratch &sc,
                                 unsigned *&d_fi) {
  const size_t fi_bytes = sizeof(unsigned) * p->rate_cats;
  hipError_t e = flush_q(p);
  if (e == hipSuccess) e = ensure_scratch(p, extra + fi_bytes);
  if (e != hipSuccess) return e;
  d_fi = (unsigned *)sc.take(fi_bytes);
  return upload(p, d_fi, freqs_indices, fi_bytes);
}
// ... and around it: a `root` span of the event timer, then the host waits for the stream
template <class Launch>
static hipError_t run_root_lnl(rdamd_partition *p, Launch launch) {
  p->prof_begin(2);
  const hipError_t e = launch();
  p->prof_end();
  return e == hipSuccess ? hipStreamSynchronize(p->stream) : e;
}

#ifdef RDAMD_ABLATION
// RDAMD_CLV_DEBUG: what choose_slots (clv_plan.hpp) saw for every launch of several pieces
static void print_clv_pieces(const ClvPlanInput &in, const ClvPlan &plan, const rdamd_operation_t *ops, unsigned count) {
  if (in.k20) return;
  const std::vector<unsigned> &seg = plan.cut.seg;
  for (size_t l = 0; l + 1 < plan.levels.size(); ++l) {
    const unsigned s0 = plan.levels[l], s1 = plan.levels[l + 1];
    if (s1 - s0 < 2) continue;
    fprintf(stderr, "[clv pieces] launch %zu: %u operations in %u pieces (longest %u); read-backs by slots:", l,
            seg[s1] - seg[s0], s1 - s0, seg[s0 + 1] - seg[s0]);
    for (unsigned sl = 0; sl <= in.slots_whole; ++sl) fprintf(stderr, " %u:%u", sl, clv_plan_readbacks(in, plan, ops, count, l, sl));
    fprintf(stderr, "; chosen %u\n", plan.seg_slots[s0]);
  }
  if (plan.levels.size() > 2)
    fprintf(stderr, "[clv pieces] last launch: %u operations\n", count - seg[plan.levels[plan.levels.size() - 2]]);
}
#endif

// what the planner (clv_plan.hpp) needs to know of the partition and its kernels
static ClvPlanInput clv_plan_input(const rdamd_partition *p, unsigned count) {
  ClvPlanInput in;
  in.tips = p->tips; in.clv_buffers = p->clv_buffers; in.prob_matrices = p->prob_matrices;
  in.scale_buffers = p->scale_buffers; in.sites = p->sites; in.tip_stride = p->tip_stride();
  in.clv_bytes = (uint64_t)p->clv_doubles() * sizeof(double);
  in.k20 = p->mfma_layout;   // fixed at creation, with the CLV layout
  if (in.k20) clv_k20_traversal_cut(p, count, &in.rows, &in.small, &in.min_count);
  else in.rows = clv_traversal_pieces(p, count);
  in.slots_whole = clv_traversal_slots(p);
  in.chunk = clv_traversal_chunk(p);
#ifdef RDAMD_ABLATION
  if (getenv("RDAMD_CLV_PIECE_OPS")) in.small = (unsigned)atoi(getenv("RDAMD_CLV_PIECE_OPS"));
  if (getenv("RDAMD_CLV_MIN_SPLIT")) in.min_count = (unsigned)atoi(getenv("RDAMD_CLV_MIN_SPLIT"));
  if (getenv("RDAMD_CLV_READBACK_PCT")) in.readback_tolerance_pct = (unsigned)atoi(getenv("RDAMD_CLV_READBACK_PCT"));
  if (getenv("RDAMD_CLV_PIECE_SLOTS")) in.forced_slots = (int)std::min<unsigned>((unsigned)atoi(getenv("RDAMD_CLV_PIECE_SLOTS")), 6u);
#endif
  return in;
}

// rdamd_root_loglikelihood_fused_multi: room for n_items rows (and their results) in the leader's blocks
static bool reserve_root_items(rdamd_partition *lead, unsigned n_items) {
  if (lead->root_items_cap >= n_items) return true;
  if (lead->d_root_items) (void)hipFree(lead->d_root_items);
  if (lead->h_root_items) (void)hipHostFree(lead->h_root_items);
  lead->d_root_items = lead->h_root_items = nullptr;
  lead->root_items_cap = std::max(64u, n_items * 2);
  const size_t bytes = (size_t)lead->root_items_cap * (sizeof(RootItem) + kRootMaxPositions * sizeof(double));
  RDAMD_HIP_TRY(hipMalloc(&lead->d_root_items, bytes), false);
  RDAMD_HIP_TRY(hipHostMalloc(&lead->h_root_items, bytes, hipHostMallocDefault), false);
  return true;
}

// ... and row i: partition p checked and brought up to date, everything root_multi_dna_kernel reads of it
// (lengths: n_positions of them per child; result: where its kRootMaxPositions values land)
static bool fill_root_item(rdamd_partition *p, rdamd_partition *lead, unsigned i, const rdamd_operation_t &op,
                           const unsigned *params_indices, const double *len1, const double *len2,
                           unsigned n_positions, RootItem &it, double *result) {
  if (!op_in_range(p, op)) {
    set_error(10, "rdamd_root_loglikelihood_fused_multi: item %u: index out of range", i);
    return false;
  }
  rdamd_operation_t o;
  RDAMD_HIP_TRY(op_phys(p, op, &o), false);
  for (unsigned a = 0; a < n_positions; ++a)
    if (!length_ok(len1[a]) || !length_ok(len2[a])) {
      set_error(9, "rdamd_root_loglikelihood_fused_multi: item %u: invalid branch length", i);
      return false;
    }
  if (bad_rate_index(p, params_indices)) {
    set_error(7, "rdamd_root_loglikelihood_fused_multi: item %u: params index out of range", i);
    return false;
  }
  memset(&it, 0, sizeof it);
  it.ra = root_single_args(len1, len2, n_positions, params_indices, p->rate_cats);
  RDAMD_HIP_TRY(flush_q(p), false);
  RDAMD_HIP_TRY(flush_tiptab(p), false);
  // whatever this partition's own stream still has queued (parameter uploads just now) must
  // be done before the leader's stream reads it
  if (p != lead && (p->stream_dirty || p->stream_external)) RDAMD_HIP_TRY(sync_main(p), false);
  it.v = p->view();
  level_op_fields(o, it.op);
  it.q = p->d_q; it.rates = p->d_rates; it.freqs = p->d_freqs; it.rate_w = p->d_rate_weights;
  it.pw = p->d_pattern_weights; it.codemask = p->d_codemask;
  it.partials = p->d_partials; it.counter = p->d_counter;
  it.result = result;   // (pinned host memory: the folding wave writes it there, no copy launch)
  it.blocks = root_lnl_shape(p).blocks;   // (fast_root_shape: the group layout)
  return true;
}

// rdamd_partition_create: CLV layout, stream, device buffers and pinned blocks of a partition whose sizes are set
// (false: an error is set; the caller destroys what exists)
#define TRY(expr) RDAMD_HIP_TRY(expr, false)
static bool allocate_device_state(rdamd_partition *p) {
  const unsigned K = p->states, R = p->rate_cats, tips = p->tips, clv_buffers = p->clv_buffers,
                 scale_buffers = p->scale_buffers, prob_matrices = p->prob_matrices, rate_matrices = p->rate_matrices;
  const size_t S = p->sites;
  TRY(hipGetDevice(&p->device));
  TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  // + kTipcodePad: the traversal kernel reads tip codes with dword-wide scalar
  // loads that may run a few bytes past the last row
  TRY(hipMalloc(&p->d_tipcodes, (size_t)tips * p->tip_stride() + kTipcodePad));
  if (K == 4) {
    TRY(hipMalloc(&p->d_tipcodes16, (size_t)tips * p->tip_stride() + kTipcodePad));
    p->code_rows = p->code_rows_cap = tips;
  }
  // (the 20-state matrix-core kernel keeps CLVs in its operand layout, whole 16-site tiles:
  // decided here, before the CLV buffers are sized -- common.hpp)
  p->mfma_layout = fused20_capable(K, R) &&
                   (size_t)p->clv_tiles() * 16u * R * K * sizeof(double) < ((size_t)1 << 31) &&
                   (size_t)prob_matrices * R * k20_mfma_copy_doubles() * sizeof(double) < ((size_t)1 << 31);
  p->sparse = (p->attributes & RDAMD_ATTRIB_SPARSE_CLVS) != 0;
  if (p->sparse) {   // a small pool to start with (common.hpp); it grows when more buffers are live at once
    p->clv_slot.assign(clv_buffers, -1);
    p->sc_slot.assign(scale_buffers, -1);
    p->clv_slots_cap = std::min(clv_buffers, 4u);
    p->sc_slots_cap = std::min(scale_buffers, 4u);
  }
  const size_t clv_alloc = p->sparse ? p->clv_slots_cap : clv_buffers, sc_alloc = p->sparse ? p->sc_slots_cap : scale_buffers;
  TRY(hipMalloc(&p->d_clv, std::max<size_t>(8, clv_alloc * p->clv_doubles() * sizeof(double))));
  TRY(hipMalloc(&p->d_scaler, std::max<size_t>(4, sc_alloc * S * sizeof(unsigned))));
  TRY(hipMalloc(&p->d_pmat, (size_t)prob_matrices * R * K * K * sizeof(double)));
  TRY(hipMalloc(&p->d_tiptab, (size_t)prob_matrices * R * p->ncodes_cap * K * sizeof(double)));
  if (p->mfma_layout)
    TRY(hipMalloc(&p->d_pmat_mfma, (size_t)prob_matrices * R * k20_mfma_copy_doubles() * sizeof(double)));
  TRY(hipMalloc(&p->d_codemask, 256 * sizeof(uint64_t)));
  TRY(hipMalloc(&p->d_q, (size_t)rate_matrices * K * K * sizeof(double)));
  TRY(hipMalloc(&p->d_freqs, (size_t)rate_matrices * K * sizeof(double)));
  TRY(hipMalloc(&p->d_rates, R * sizeof(double)));
  TRY(hipMalloc(&p->d_rate_weights, R * sizeof(double)));
  TRY(hipMalloc(&p->d_pattern_weights, std::max<size_t>(4, S * sizeof(unsigned))));
  TRY(hipMalloc(&p->d_partials, 32768 * sizeof(double)));   // (8 root positions x 1024 blocks x 4 waves)
  TRY(hipMalloc(&p->d_counter, sizeof(unsigned)));
  TRY(hipMemsetAsync(p->d_counter, 0, sizeof(unsigned), p->stream));
  TRY(hipMalloc(&p->d_result, 64 * sizeof(double)));
  p->stage_bytes = (size_t)4 << 20;
  TRY(hipHostMalloc(&p->h_stage, p->stage_bytes, hipHostMallocDefault));
  TRY(hipHostMalloc(&p->h_result, 64 * sizeof(double), hipHostMallocDefault));
  TRY(ensure_scratch(p, (size_t)1 << 20));
  TRY(hipMemsetAsync(p->d_scaler, 0, std::max<size_t>(4, sc_alloc * S * sizeof(unsigned)), p->stream));
  TRY(hipMemsetAsync(p->d_tipcodes, 0, (size_t)tips * p->tip_stride() + kTipcodePad, p->stream));
  if (K == 4) TRY(hipMemsetAsync(p->d_tipcodes16, 0, (size_t)tips * p->tip_stride() + kTipcodePad, p->stream));
  return true;
}

// ... and the host mirrors, with the defaults uploaded
static bool set_defaults(rdamd_partition *p) {
  const unsigned K = p->states, R = p->rate_cats, tips = p->tips, rate_matrices = p->rate_matrices;
  const size_t S = p->sites;
  // defaults as corax_partition_create leaves them: weights 1, rates 1, 1/R
  p->subst.assign(rate_matrices, std::vector<double>((size_t)K * K - K, 1.0));
  p->freqs.assign(rate_matrices, std::vector<double>(K, 1.0 / K));
  if (p->embedded()) {   // defaults of a 2-state partition, through the embedding setters
    p->api_subst.assign(rate_matrices, std::vector<double>(2, 1.0));
    p->api_freqs.assign(rate_matrices, std::vector<double>(2, 0.5));
    for (unsigned i = 0; i < rate_matrices; ++i) {
      p->subst[i].assign(12, 0.0);
      p->subst[i][0] = p->subst[i][3] = 1.0;
      p->freqs[i] = {0.5, 0.5, 0.0, 0.0};
    }
  }
  p->rates.assign(R, 1.0);
  p->rate_weights.assign(R, 1.0 / R);
  p->prop_invar.assign(rate_matrices, 0.0);
  p->pattern_weights.assign(S, 1u);
  p->tipcodes.assign((size_t)tips * S, 0);
  p->q_dirty.assign(rate_matrices, 1);
  p->codemask.assign(256, 0);
  if (K == 4) {
    for (unsigned c = 0; c < 16; ++c) p->codemask[c] = c;
    p->ncodes = 16;
  } else {
    p->ncodes = 0;
  }
  TRY(upload(p, p->d_codemask, p->codemask.data(), 256 * sizeof(uint64_t)));
  TRY(upload(p, p->d_rates, p->rates.data(), R * sizeof(double)));
  TRY(upload(p, p->d_rate_weights, p->rate_weights.data(), R * sizeof(double)));
  if (S) TRY(upload(p, p->d_pattern_weights, p->pattern_weights.data(), S * sizeof(unsigned)));
  TRY(hipStreamSynchronize(p->stream));
  return true;
}
#undef TRY

// ---- the pre-order pass's call frame (kernels_preorder.hip) -----------------------------------
// device memory of one call, given back however the call ends
template <class T>
struct DeviceArray {
  T *d = nullptr;
  ~DeviceArray() { if (d) (void)hipFree(d); }
  hipError_t alloc(size_t n) { return hipMalloc(&d, sizeof(T) * n); }
};

// the shapes the pre-order pass does not take; says so and returns true
static bool outer_refused(const rdamd_partition *p, const char *what) {
  if (p->states != 4 || p->mfma_layout) {
    set_error(63, "%s: %u-state partitions are not supported (ancestral states are computed for 4-state and binary data)",
              what, p->api_states);
    return true;
  }
  if (p->sparse) {
    set_error(63, "%s: partitions with RDAMD_ATTRIB_SPARSE_CLVS are not supported (the pass reads every inner CLV of a "
                  "materialising traversal)", what);
    return true;
  }
  return false;
}

// ... and the shapes rdamd_ancestral_sequences and rdamd_branch_length_derivatives do not take: they
// walk 4-state, binary and matrix-core 20-state partitions (`result`: what the entry point computes,
// for the message)
static bool walks_refused(const rdamd_partition *p, const char *what, const char *result) {
  if (p->sparse) {
    set_error(63, "%s: partitions with RDAMD_ATTRIB_SPARSE_CLVS are not supported (the pass reads every inner CLV of a "
                  "materialising traversal)", what);
    return true;
  }
  if (p->states == 4 || p->mfma_layout) return false;
  if (p->states == 20)
    set_error(63, "%s: 20-state partitions with %u rate categories are not supported (the matrix-core layout the walk "
                  "reads holds up to 8 categories and CLVs under 2 GB)", what, p->rate_cats);
  else
    set_error(63, "%s: %u-state partitions are not supported (%s are computed for 2, 4 and 20 states)", what, p->api_states,
              result);
  return true;
}
static bool sequences_refused(const rdamd_partition *p, const char *what) { return walks_refused(p, what, "ancestral sequences"); }
static bool derivatives_refused(const rdamd_partition *p, const char *what) {
  return walks_refused(p, what, "branch-length derivatives");
}
static bool pair_sums_refused(const rdamd_partition *p, const char *what) { return walks_refused(p, what, "pair sums"); }

// What the entry points of the pre-order pass share, in two steps: preorder_admitted, then
// preorder_run.  (RateIndices: a per-rate-category index vector of the caller and its name.)
struct RateIndices { const unsigned *host; const char *name; };

// the refusals (by shape: `refused`) and the plan; false: refused, the error set in the name of entry point `what`
static bool preorder_admitted(const rdamd_partition *p, const char *what, const rdamd_operation_t *ops, unsigned n_ops,
                              bool null_argument, std::initializer_list<RateIndices> indices, OuterPlan *plan,
                              bool (*refused)(const rdamd_partition *, const char *) = outer_refused) {
  if (refused(p, what)) return false;
  if (null_argument) {
    set_error(64, "%s: null argument", what);
    return false;
  }
  for (unsigned i = 0; i < n_ops; ++i)
    if (!op_in_range(p, ops[i])) {
      set_error(10, "%s: operation %u has an index out of range", what, i);
      return false;
    }
  *plan = plan_outer_program(ops, n_ops, p->tips);
  if (plan->bad_op >= 0) {
    set_error(64, "%s: not a complete post-order traversal ending in the root operation: operation %d: %s", what,
              plan->bad_op, plan->why);
    return false;
  }
  for (const RateIndices &v : indices)
    if (bad_rate_index(p, v.host)) {
      set_error(7, "%s: %s index out of range", what, v.name);
      return false;
    }
  return true;
}

// Allocates the workspace, has the entry point allocate its result buffers (allocate()), uploads
// the program and the index vectors and runs launch(d_prog, d_indices (in the caller's order),
// d_work) between two events on the main stream; *ms: the time between them.  Returns when the
// stream has drained.
template <class Allocate, class Launch>
static int preorder_run(rdamd_partition *p, const OuterPlan &plan, std::initializer_list<RateIndices> indices, double *ms,
                        Allocate allocate, Launch launch) {
  struct Frame {
    DeviceArray<double> work;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    ~Frame() { for (hipEvent_t e : {t0, t1}) if (e) (void)hipEventDestroy(e); }
  } mem;
  const unsigned R = p->rate_cats;
  const size_t prog_bytes = sizeof(OuterOp) * plan.prog.size();
  RDAMD_HIP_TRY(flush_q(p), RDAMD_FAILURE);
  RDAMD_HIP_TRY(ensure_scratch(p, prog_bytes + indices.size() * sizeof(unsigned) * R + 1024), RDAMD_FAILURE);
  RDAMD_HIP_TRY(mem.work.alloc(std::max<size_t>(1, outer_workspace_doubles(p, plan.slots))), RDAMD_FAILURE);
  RDAMD_HIP_TRY(allocate(), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&mem.t0), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&mem.t1), RDAMD_FAILURE);
  Scratch sc{p};
  OuterOp *d_prog = (OuterOp *)sc.take(prog_bytes);
  unsigned *d_indices[2] = {nullptr, nullptr};   // (no entry point has more)
  RDAMD_HIP_TRY(upload(p, d_prog, plan.prog.data(), prog_bytes), RDAMD_FAILURE);
  size_t n = 0;
  for (const RateIndices &v : indices) {
    d_indices[n] = (unsigned *)sc.take(sizeof(unsigned) * R);
    RDAMD_HIP_TRY(upload(p, d_indices[n++], v.host, sizeof(unsigned) * R), RDAMD_FAILURE);
  }
  p->prof_begin(5);
  RDAMD_HIP_TRY(hipEventRecord(mem.t0, p->stream), RDAMD_FAILURE);
  const hipError_t le = launch(d_prog, d_indices, mem.work.d);
  RDAMD_HIP_TRY(hipEventRecord(mem.t1, p->stream), RDAMD_FAILURE);
  p->prof_end();
  RDAMD_HIP_TRY(le, RDAMD_FAILURE);
  RDAMD_HIP_TRY(sync_main(p), RDAMD_FAILURE);
  float elapsed = 0.f;
  if (hipEventElapsedTime(&elapsed, mem.t0, mem.t1) == hipSuccess) *ms = elapsed;
  return RDAMD_SUCCESS;
}

}  // namespace rdamd

extern "C" {

int rdamd_errno(void) { return g_errno; }
const char *rdamd_errmsg(void) { return g_errmsg; }
const char *rdamd_version(void) { return "root_digger_amd 0.1 (gfx950)"; }

// the libamdhip64 that serves this library (a process may hold a second one, e.g. the copy
// PyTorch bundles): device pointers are only good between code on the SAME runtime
const char *rdamd_hip_runtime_path(void) {
  static std::string path = [] {
    Dl_info info;
    if (dladdr(reinterpret_cast<void *>(&hipGetDevice), &info) && info.dli_fname) return std::string(info.dli_fname);
    return std::string();
  }();
  return path.c_str();
}

int rdamd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rdamd_set_device(int device) {
  clear_error();
  RDAMD_HIP_TRY(hipSetDevice(device), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

int rdamd_device_memory(uint64_t *free_bytes, uint64_t *total_bytes) {
  clear_error();
  size_t f = 0, t = 0;
  RDAMD_HIP_TRY(hipMemGetInfo(&f, &t), RDAMD_FAILURE);
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return RDAMD_SUCCESS;
}

// device bytes rdamd_partition_create takes for a partition of this shape (the
// large buffers; what a replica of a model costs)
uint64_t rdamd_partition_footprint(unsigned int tips, unsigned int clv_buffers, unsigned int states,
                                   unsigned int sites, unsigned int prob_matrices,
                                   unsigned int rate_cats, unsigned int scale_buffers) {
  const uint64_t K = states == 2 ? 4 : states, R = rate_cats, S = sites;
  const uint64_t codes = K == 4 ? 16 : 64;
  const uint64_t Sclv = fused20_capable((unsigned)K, R) ? (S + 15) / 16 * 16 : S;   // operand layout: whole 16-site tiles
  // (4 states: the tip codes twice -- as codes and as LDS row offsets for the fused evaluator)
  uint64_t b = (uint64_t)tips * ((S + 3) / 4 * 4) * (K == 4 ? 2 : 1) + (uint64_t)clv_buffers * Sclv * R * K * 8 +
               (uint64_t)scale_buffers * S * 4 + (uint64_t)prob_matrices * R * K * K * 8 +
               (uint64_t)prob_matrices * R * codes * K * 8 + S * 4 + ((uint64_t)6 << 20);
  if (fused20_capable((unsigned)K, R)) b += (uint64_t)prob_matrices * R * k20_mfma_copy_doubles() * 8;
  return b;
}

#define NT(ch, v) [ch] = v, [ch + 32] = v
const uint64_t rdamd_map_nt[256] = {
    NT('A', 1),  NT('C', 2),  NT('G', 4),  NT('T', 8),  NT('U', 8),  NT('R', 5),
    NT('Y', 10), NT('S', 6),  NT('W', 9),  NT('K', 12), NT('M', 3),  NT('B', 14),
    NT('D', 13), NT('H', 11), NT('V', 7),  NT('N', 15), NT('O', 15), NT('X', 15),
    ['-'] = 15,  ['?'] = 15,
};
#undef NT
const uint64_t rdamd_map_bin[256] = {
    ['0'] = 1, ['1'] = 2, ['-'] = 3, ['?'] = 3,
};

rdamd_partition_t *rdamd_partition_create(unsigned int tips, unsigned int clv_buffers,
                                          unsigned int states, unsigned int sites,
                                          unsigned int rate_matrices,
                                          unsigned int prob_matrices,
                                          unsigned int rate_cats,
                                          unsigned int scale_buffers,
                                          unsigned int attributes) {
  clear_error();
  if (states < 2 || states > 64 || rate_cats < 1 || rate_matrices < 1 || tips < 1) {
    set_error(1, "rdamd_partition_create: unsupported sizes (states=%u rate_cats=%u "
                 "rate_matrices=%u tips=%u)", states, rate_cats, rate_matrices, tips);
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error(2, "rdamd_partition_create: no HIP device available; this library has "
                 "no CPU fallback");
    return nullptr;
  }
  rdamd_partition *p = new rdamd_partition();
  p->api_states = states;
  if (states == 2) states = 4;   // embedded, see common.hpp
  p->tips = tips; p->clv_buffers = clv_buffers; p->states = states; p->sites = sites;
  p->rate_matrices = rate_matrices; p->prob_matrices = prob_matrices;
  p->rate_cats = rate_cats; p->scale_buffers = scale_buffers; p->attributes = attributes;
  // (rdamd_partition_set_rescale_speculation's mode for partitions a caller does not reach itself --
  // model_t's, its replicas' --: RDAMD_RESCALE_SPECULATION=0|1 in the environment, read here)
  if (const char *e = getenv("RDAMD_RESCALE_SPECULATION")) {
    const int mode = atoi(e);
    p->rescale_speculation = mode <= 0 ? 0 : 1;
  }
  p->ncodes_cap = states == 4 ? 16 : 64;
  if (!allocate_device_state(p) || !set_defaults(p)) {
    rdamd_partition_destroy(p);
    return nullptr;
  }
  return p;
}

void rdamd_partition_destroy(rdamd_partition_t *p) {
  if (!p) return;
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  void *dev[] = {p->d_tipcodes, p->d_tipcodes16, p->d_codes_wide, p->d_clv, p->d_scaler, p->d_pmat, p->d_tiptab, p->d_pmat_mfma,
                 p->d_codemask, p->d_q, p->d_freqs, p->d_rates, p->d_rate_weights,
                 p->d_pattern_weights, p->d_tipclv_scratch, p->d_scratch,
                 p->d_partials, p->d_result, p->d_persite, p->d_counter};
  for (void *d : dev)
    if (d) (void)hipFree(d);
  rdamd::fused_workspace_free(p->fused);
  rdamd::fused_workspace_free(p->fused1);
  for (auto &b : p->sched_pool) (void)hipFree(b.ptr);
  for (auto &b : p->sched_retired) (void)hipFree(b.ptr);
  if (p->stream_pre) (void)hipStreamDestroy(p->stream_pre);
  rdamd::clade_cache_free(p->clades);
  for (auto &sp : p->prof_spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
  for (auto &e : p->prof_pool) (void)hipEventDestroy(e);
  if (p->h_stage) (void)hipHostFree(p->h_stage);
  if (p->h_result) (void)hipHostFree(p->h_result);
  if (p->d_root_items) (void)hipFree(p->d_root_items);
  if (p->h_root_items) (void)hipHostFree(p->h_root_items);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

void rdamd_partition_discard_clvs(rdamd_partition_t *p) {
  if (!p || !p->sparse) return;
  // (slots are reused by later calls on the partition's stream, i.e. after everything queued so
  // far; a combined root step of ANOTHER partition's stream has returned before its caller can
  // get here)
  std::fill(p->clv_slot.begin(), p->clv_slot.end(), -1);
  std::fill(p->sc_slot.begin(), p->sc_slot.end(), -1);
  p->clv_slots_used = p->sc_slots_used = 0;
}

unsigned int rdamd_update_clvs_launches(const rdamd_partition_t *p) { return p->last_clv_launches; }

uint64_t rdamd_partition_clv_bytes(const rdamd_partition_t *p) {
  const uint64_t c = p->sparse ? p->clv_slots_cap : p->clv_buffers, s = p->sparse ? p->sc_slots_cap : p->scale_buffers;
  return c * p->clv_doubles() * sizeof(double) + s * (uint64_t)p->sites * sizeof(unsigned);
}

int rdamd_set_tip_states(rdamd_partition_t *p, unsigned int tip_index,
                         const uint64_t *map, const char *sequence) {
  clear_error();
  if (tip_index >= p->tips) {
    set_error(3, "rdamd_set_tip_states: tip index %u out of range", tip_index);
    return RDAMD_FAILURE;
  }
  const size_t S = p->sites;
  // the whole sequence first, against a copy of the code table (tip_encode.hpp): a refused call
  // leaves host and device as they were
  rdamd::TipEncoding enc = rdamd::encode_tip_row(map, sequence, S, p->api_states, p->states == 4, p->codemask,
                                                 p->ncodes, p->ncodes_cap);
  if (enc.error == 4) {
    set_error(4, "rdamd_set_tip_states: character '%c' (site %zu) has no valid state "
                 "in the map", sequence[enc.site], enc.site);
    return RDAMD_FAILURE;
  }
  if (enc.error == 5) {
    set_error(5, "rdamd_set_tip_states: more than %u distinct state codes",
              p->ncodes_cap);
    return RDAMD_FAILURE;
  }
  // the device first, from the temporaries: should a copy fail, the host keeps the old sequence and
  // the old table (device entries past ncodes are not read, and the next new mask overwrites them)
  if (enc.new_code)
    RDAMD_HIP_TRY(upload(p, p->d_codemask, enc.codemask.data(), 256 * sizeof(uint64_t)), RDAMD_FAILURE);
  RDAMD_HIP_TRY(upload(p, p->d_tipcodes + (size_t)tip_index * p->tip_stride(), enc.row.data(), S), RDAMD_FAILURE);
  if (p->d_tipcodes16) {   // the same row as LDS row offsets (kernels_fused.hip)
    std::vector<uint8_t> row16(S);
    for (size_t s = 0; s < S; ++s) row16[s] = (uint8_t)(enc.row[s] << 4);
    RDAMD_HIP_TRY(upload(p, p->d_tipcodes16 + (size_t)tip_index * p->tip_stride(), row16.data(), S), RDAMD_FAILURE);
  }
  // ... then the host, all at once
  std::copy(enc.row.begin(), enc.row.end(), p->tipcodes.begin() + (size_t)tip_index * S);
  if (enc.new_code) {
    p->codemask.swap(enc.codemask);
    p->ncodes = enc.ncodes;
    p->tiptab_stale = true;
  }
  // class codes of subtrees were worked out from the old characters: forget them (schedules
  // compiled with pseudo-tips notice through the generation count)
  p->tip_generation += 1;
  if (p->clades) {
    RDAMD_HIP_TRY(sync_streams(p), RDAMD_FAILURE);
    const unsigned keep = p->clades->max_classes;
    rdamd::clade_cache_free(p->clades);
    p->clades = new rdamd::CladeCache();
    p->clades->max_classes = keep;
    p->code_rows = p->tips;
  }
  if (p->d_codes_wide) {   // (rebuilt from the host copy when the next wide schedule is compiled or run)
    RDAMD_HIP_TRY(sync_streams(p), RDAMD_FAILURE);
    (void)hipFree(p->d_codes_wide);
    p->d_codes_wide = nullptr;
    p->wide_rows = p->wide_rows_cap = 0;
  }
  return RDAMD_SUCCESS;
}

void rdamd_set_pattern_weights(rdamd_partition_t *p, const unsigned int *w) {
  p->pattern_weights.assign(w, w + p->sites);
  (void)upload(p, p->d_pattern_weights, w, sizeof(unsigned) * p->sites);
}

void rdamd_set_subst_params(rdamd_partition_t *p, unsigned int idx, const double *v) {
  if (idx >= p->rate_matrices) return;
  if (p->embedded()) {   // (q01, q10) into the row-major off-diagonals of the 4x4 matrix
    p->api_subst[idx].assign(v, v + 2);
    p->subst[idx].assign(12, 0.0);
    p->subst[idx][0] = v[0];
    p->subst[idx][3] = v[1];
  } else {
    p->subst[idx].assign(v, v + (size_t)p->states * p->states - p->states);
  }
  p->q_dirty[idx] = 1;
}

void rdamd_set_frequencies(rdamd_partition_t *p, unsigned int idx, const double *f) {
  if (idx >= p->rate_matrices) return;
  if (p->embedded()) {
    p->api_freqs[idx].assign(f, f + 2);
    p->freqs[idx] = {f[0], f[1], 0.0, 0.0};
  } else {
    p->freqs[idx].assign(f, f + p->states);
  }
  p->q_dirty[idx] = 1;
}

void rdamd_set_category_rates(rdamd_partition_t *p, const double *r) {
  p->rates.assign(r, r + p->rate_cats);
  (void)upload(p, p->d_rates, r, sizeof(double) * p->rate_cats);
}

void rdamd_set_category_weights(rdamd_partition_t *p, const double *w) {
  p->rate_weights.assign(w, w + p->rate_cats);
  (void)upload(p, p->d_rate_weights, w, sizeof(double) * p->rate_cats);
}

int rdamd_update_invariant_sites_proportion(rdamd_partition_t *p, unsigned int idx,
                                            double prop) {
  clear_error();
  if (idx >= p->rate_matrices || prop != 0.0) {
    set_error(6, "rdamd_update_invariant_sites_proportion: only 0.0 is supported (the "
                 "reference never sets anything else, src/model.cpp:292-300)");
    return RDAMD_FAILURE;
  }
  p->prop_invar[idx] = 0.0;
  return RDAMD_SUCCESS;
}

double *rdamd_msa_empirical_frequencies(rdamd_partition_t *p) {
  const unsigned K = p->api_states;
  double *f = (double *)calloc(K, sizeof(double));
  if (!f) return nullptr;
  double total = 0.0;
  for (unsigned s = 0; s < p->sites; ++s) total += p->pattern_weights[s];
  for (unsigned t = 0; t < p->tips; ++t) {
    const uint8_t *row = p->tipcodes.data() + (size_t)t * p->sites;
    for (unsigned s = 0; s < p->sites; ++s) {
      uint64_t mask = p->codemask[row[s]];
      double cnt = (double)__builtin_popcountll(mask);
      if (cnt == 0.0) continue;  // tip never set
      for (unsigned j = 0; j < K; ++j)
        if ((mask >> j) & 1) f[j] += p->pattern_weights[s] * 1.0 / cnt;
    }
  }
  for (unsigned j = 0; j < K; ++j) f[j] /= total * p->tips;
  return f;
}

unsigned int rdamd_partition_states(const rdamd_partition_t *p) { return p->api_states; }
unsigned int rdamd_partition_rate_cats(const rdamd_partition_t *p) { return p->rate_cats; }
unsigned int rdamd_partition_sites(const rdamd_partition_t *p) { return p->sites; }
unsigned int rdamd_partition_tips(const rdamd_partition_t *p) { return p->tips; }
double rdamd_partition_weight_sum(const rdamd_partition_t *p) {
  double total = 0.0;
  for (unsigned s = 0; s < p->sites; ++s) total += p->pattern_weights[s];
  return total;
}
void *rdamd_partition_stream(const rdamd_partition_t *p) {
  const_cast<rdamd_partition_t *>(p)->stream_external = true;
  return (void *)p->stream;
}

int rdamd_partition_set_stream_priority(rdamd_partition_t *p, int level) {
  clear_error();
  std::lock_guard<std::mutex> guard(p->launch_mu);
  RDAMD_HIP_TRY(sync_streams(p), RDAMD_FAILURE);
  int least = 0, greatest = 0;   // (numerically: greatest priority = lowest number)
  RDAMD_HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest), RDAMD_FAILURE);
  const int prio = level < 0 ? greatest : (level > 0 ? least : (least + greatest) / 2);
  if ((level < 0 ? -1 : (level > 0 ? 1 : 0)) == p->stream_priority && p->stream) return RDAMD_SUCCESS;   // (nothing to re-create)
  hipStream_t fresh = nullptr;
  RDAMD_HIP_TRY(hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking, prio), RDAMD_FAILURE);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  p->stream = fresh;
  p->stream_priority = level < 0 ? -1 : (level > 0 ? 1 : 0);
  return RDAMD_SUCCESS;
}
const double *rdamd_partition_subst_params(const rdamd_partition_t *p, unsigned int i) {
  if (i >= p->rate_matrices) return nullptr;
  return p->embedded() ? p->api_subst[i].data() : p->subst[i].data();
}
const double *rdamd_partition_frequencies(const rdamd_partition_t *p, unsigned int i) {
  if (i >= p->rate_matrices) return nullptr;
  return p->embedded() ? p->api_freqs[i].data() : p->freqs[i].data();
}

int rdamd_update_prob_matrices(rdamd_partition_t *p, const unsigned int *params_indices,
                               const unsigned int *matrix_indices,
                               const double *branch_lengths, unsigned int count) {
  clear_error();
  if (count == 0) return RDAMD_SUCCESS;
  const unsigned R = p->rate_cats;
  if (const unsigned *bad = bad_rate_index(p, params_indices)) {
    set_error(7, "rdamd_update_prob_matrices: params index %u out of range", *bad);
    return RDAMD_FAILURE;
  }
  for (unsigned m = 0; m < count; ++m) {
    if (matrix_indices[m] >= p->prob_matrices) {
      set_error(8, "rdamd_update_prob_matrices: matrix index %u out of range",
                matrix_indices[m]);
      return RDAMD_FAILURE;
    }
    if (!length_ok(branch_lengths[m])) {
      set_error(9, "rdamd_update_prob_matrices: invalid branch length %g for matrix %u",
                branch_lengths[m], matrix_indices[m]);
      return RDAMD_FAILURE;
    }
  }
  RDAMD_HIP_TRY(flush_q(p), RDAMD_FAILURE);
  // the three small input arrays travel as ONE host-to-device copy: lengths
  // first (8-byte aligned), then the two index arrays
  const size_t bl_bytes = sizeof(double) * count, mi_bytes = sizeof(unsigned) * count,
               pi_bytes = sizeof(unsigned) * R, packed = bl_bytes + mi_bytes + pi_bytes;
  RDAMD_HIP_TRY(ensure_scratch(p, packed + 512), RDAMD_FAILURE);
  Scratch sc{p};
  char *d_block = (char *)sc.take(packed);
  double *d_bl = (double *)d_block;
  unsigned *d_mi = (unsigned *)(d_block + bl_bytes);
  unsigned *d_pi = (unsigned *)(d_block + bl_bytes + mi_bytes);
  {
    std::vector<char> host(packed);
    memcpy(host.data(), branch_lengths, bl_bytes);
    memcpy(host.data() + bl_bytes, matrix_indices, mi_bytes);
    memcpy(host.data() + bl_bytes + mi_bytes, params_indices, pi_bytes);
    RDAMD_HIP_TRY(upload(p, d_block, host.data(), packed), RDAMD_FAILURE);
  }
  p->prof_begin(1);
  hipError_t le = launch_pmatrix(p, d_pi, d_mi, d_bl, count);
  if (le == hipSuccess && p->d_pmat_mfma) le = launch_pmat_to_mfma(p, d_mi, count);
  p->prof_end();
  RDAMD_HIP_TRY(le, RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

void rdamd_update_clvs(rdamd_partition_t *p, const rdamd_operation_t *ops,
                       unsigned int count) {
  clear_error();
  if (count == 0) return;
  std::vector<rdamd_operation_t> phys_ops;
  if (p->sparse) {   // from here on the list names pool slots (common.hpp)
    phys_ops.resize(count);
    for (unsigned i = 0; i < count; ++i) {
      const hipError_t pe = op_phys(p, ops[i], &phys_ops[i]);
      if (pe != hipSuccess) {
        set_error(pe == hipErrorInvalidValue ? 10 : 100 + (int)pe, "rdamd_update_clvs: operation %u: %s", i,
                  pe == hipErrorInvalidValue ? "an index out of range" : hipGetErrorString(pe));
        return;
      }
    }
    ops = phys_ops.data();
  }
  const ClvPlanInput in = clv_plan_input(p, count);
  const ClvPlan plan = plan_clv_traversal(in, ops, count);
  if (plan.bad_op >= 0) {
    set_error(10, "rdamd_update_clvs: operation %u has an index out of range", (unsigned)plan.bad_op);
    return;
  }
#ifdef RDAMD_ABLATION
  if (getenv("RDAMD_CLV_DEBUG")) print_clv_pieces(in, plan, ops, count);
#endif
  const size_t bytes = sizeof(LevelOp) * plan.lops.size();
  hipError_t e = ensure_scratch(p, bytes + 256);
  if (e == hipSuccess) e = flush_tiptab(p);
  Scratch sc{p};
  if (e == hipSuccess) {
    LevelOp *d_ops = (LevelOp *)sc.take(bytes);
    e = upload(p, d_ops, plan.lops.data(), bytes);
    p->prof_begin(0);
    // one launch per level of the cut: its pieces side by side
    for (size_t l = 0; e == hipSuccess && l < plan.launches(); ++l)
      e = in.k20 ? launch_clv_k20_traversal(p, d_ops, plan.pieces(l))
                 : launch_clv_traversal(p, d_ops, plan.pieces(l), plan.seg_slots[plan.levels[l]]);
    p->last_clv_launches = plan.launches();
    p->prof_end();
  }
  if (e != hipSuccess)
    set_error(100 + (int)e, "rdamd_update_clvs: %s", hipGetErrorString(e));
}

double rdamd_compute_root_loglikelihood(rdamd_partition_t *p, unsigned int clv_index,
                                        int scaler_index,
                                        const unsigned int *freqs_indices,
                                        double *persite_lnl) {
  clear_error();
  const double nan = std::nan("");
  if (!root_index_ok(p, clv_index, scaler_index)) {
    set_error(11, "rdamd_compute_root_loglikelihood: index out of range (clv %u, scaler %d)",
              clv_index, scaler_index);
    return nan;
  }
  if (bad_rate_index(p, freqs_indices)) {
    set_error(7, "rdamd_compute_root_loglikelihood: freqs index out of range");
    return nan;
  }
  if (p->sites == 0) return 0.0;   // an empty alignment has likelihood 1
  RDAMD_HIP_TRY(clv_phys(p, clv_index, &clv_index), nan);
  RDAMD_HIP_TRY(scaler_phys(p, scaler_index, &scaler_index), nan);
  Scratch sc{p};
  unsigned *d_fi;
  RDAMD_HIP_TRY(stage_root_lnl(p, freqs_indices, 1024, sc, d_fi), nan);
  if (persite_lnl && !p->d_persite)
    RDAMD_HIP_TRY(hipMalloc(&p->d_persite, std::max<size_t>(8, sizeof(double) * p->sites)), nan);
  // the finishing workgroup writes straight into the pinned host block
  RDAMD_HIP_TRY(run_root_lnl(p, [&] {
    return launch_root_lnl(p, clv_index, scaler_index, d_fi, persite_lnl ? p->d_persite : nullptr, p->h_result);
  }), nan);
  if (persite_lnl)
    RDAMD_HIP_TRY(hipMemcpy(persite_lnl, p->d_persite, sizeof(double) * p->sites,
                            hipMemcpyDeviceToHost), nan);
  return p->h_result[0];
}

int rdamd_compute_root_loglikelihoods(rdamd_partition_t *p, unsigned int count,
                                      const unsigned int *clv_indices, const int *scaler_indices,
                                      const unsigned int *freqs_indices, double *lnl_out) {
  clear_error();
  if (count == 0) return RDAMD_SUCCESS;
  std::vector<unsigned> rel(count);
  for (unsigned i = 0; i < count; ++i) {
    if (!root_index_ok(p, clv_indices[i], scaler_indices[i])) {
      set_error(11, "rdamd_compute_root_loglikelihoods: index out of range (entry %u)", i);
      return RDAMD_FAILURE;
    }
    rel[i] = clv_indices[i] - p->tips;
  }
  std::vector<int> phys_sc;
  if (p->sparse && p->sites) {
    phys_sc.assign(scaler_indices, scaler_indices + count);
    for (unsigned i = 0; i < count; ++i) {
      unsigned c = 0;
      RDAMD_HIP_TRY(clv_phys(p, clv_indices[i], &c), RDAMD_FAILURE);
      RDAMD_HIP_TRY(scaler_phys(p, scaler_indices[i], &phys_sc[i]), RDAMD_FAILURE);
      rel[i] = c - p->tips;
    }
    scaler_indices = phys_sc.data();
  }
  if (bad_rate_index(p, freqs_indices)) {
    set_error(7, "rdamd_compute_root_loglikelihoods: freqs index out of range");
    return RDAMD_FAILURE;
  }
  if (p->sites == 0) {
    std::fill(lnl_out, lnl_out + count, 0.0);
    return RDAMD_SUCCESS;
  }
  const unsigned blocks = root_lnl_shape(p).blocks;
  Scratch sc{p};
  unsigned *d_fi;
  RDAMD_HIP_TRY(stage_root_lnl(p, freqs_indices, 4096 + (size_t)count * (8 + 8) +
                               sizeof(double) * ((size_t)count * blocks + count), sc, d_fi), RDAMD_FAILURE);
  unsigned *d_rel = (unsigned *)sc.take(sizeof(unsigned) * count);
  int *d_sci = (int *)sc.take(sizeof(int) * count);
  double *d_partials = (double *)sc.take(sizeof(double) * (size_t)count * blocks);
  double *d_out = (double *)sc.take(sizeof(double) * count);
  RDAMD_HIP_TRY(upload(p, d_rel, rel.data(), sizeof(unsigned) * count), RDAMD_FAILURE);
  RDAMD_HIP_TRY(upload(p, d_sci, scaler_indices, sizeof(int) * count), RDAMD_FAILURE);
  RDAMD_HIP_TRY(run_root_lnl(p, [&] { return launch_root_lnl_batch(p, count, d_rel, d_sci, d_fi, d_partials, d_out); }),
                RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(lnl_out, d_out, sizeof(double) * count, hipMemcpyDeviceToHost),
                RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

int rdamd_root_loglikelihood_fused(rdamd_partition_t *p, const rdamd_operation_t *root_op,
                                   const unsigned int *params_indices,
                                   const double *lengths1, const double *lengths2,
                                   unsigned int n_alpha, double *lnl_out) {
  clear_error();
  if (n_alpha == 0) return RDAMD_SUCCESS;
  if (p->sites == 0) {
    std::fill(lnl_out, lnl_out + n_alpha, 0.0);
    return RDAMD_SUCCESS;
  }
  if (bad_rate_index(p, params_indices)) {   // (ahead of the fallback: its refusal would name another call)
    set_error(7, "rdamd_root_loglikelihood_fused: params index out of range");
    return RDAMD_FAILURE;
  }
  if (!fast_root_shape(p, *root_op)) {
    // generic shapes: the three calls queued back to back on the partition stream
    for (unsigned a = 0; a < n_alpha; ++a) {
      unsigned mi[2] = {root_op->child1_matrix_index, root_op->child2_matrix_index};
      double bl[2] = {lengths1[a], lengths2[a]};
      if (rdamd_update_prob_matrices(p, params_indices, mi, bl, 2) != RDAMD_SUCCESS)
        return RDAMD_FAILURE;
      rdamd_update_clvs(p, root_op, 1);
      if (rdamd_errno()) return RDAMD_FAILURE;
      lnl_out[a] = rdamd_compute_root_loglikelihood(
          p, root_op->parent_clv_index, root_op->parent_scaler_index, params_indices, nullptr);
      if (rdamd_errno()) return RDAMD_FAILURE;
    }
    return RDAMD_SUCCESS;
  }
  if (!op_in_range(p, *root_op)) {
    set_error(10, "rdamd_root_loglikelihood_fused: index out of range");
    return RDAMD_FAILURE;
  }
  rdamd_operation_t phys_root;
  RDAMD_HIP_TRY(op_phys(p, *root_op, &phys_root), RDAMD_FAILURE);
  root_op = &phys_root;
  RDAMD_HIP_TRY(flush_q(p), RDAMD_FAILURE);
  RDAMD_HIP_TRY(flush_tiptab(p), RDAMD_FAILURE);
  // One launch per chunk of up to eight positions (four at 8 rate categories;
  // root_single_dna_kernel): branch
  // lengths and parameter indices travel as kernel arguments, the P-matrices are
  // exponentiated inside the kernel, the result lands in the pinned host block.
  // The LAST position of the call leaves its matrices, root CLV and scaler in the
  // partition, exactly as the unfused call sequence would.
  LevelOp op;
  level_op_fields(*root_op, op);
  op.src1 = op.src2 = 0;
  for (unsigned a = 0; a < n_alpha; ++a)
    if (!length_ok(lengths1[a]) || !length_ok(lengths2[a])) {
      set_error(9, "rdamd_root_loglikelihood_fused: invalid branch length");
      return RDAMD_FAILURE;
    }
  const unsigned chunk = root_single_max_positions(p->rate_cats);
  for (unsigned base = 0; base < n_alpha; base += chunk) {
    const unsigned n = std::min(chunk, n_alpha - base);
    p->prof_begin(2);
    hipError_t e = launch_root_single(p, op, lengths1 + base, lengths2 + base, n, params_indices,
                                      p->d_counter, p->h_result);
    p->prof_end();
    RDAMD_HIP_TRY(e, RDAMD_FAILURE);
    RDAMD_HIP_TRY(sync_main(p), RDAMD_FAILURE);
    for (unsigned a = 0; a < n; ++a) lnl_out[base + a] = p->h_result[a];
  }
  return RDAMD_SUCCESS;
}

// Root-only evaluations of SEVERAL partitions in one launch (root_multi_dna_kernel): the
// Brent / finite-difference steps of the candidates a lock-stepped search has in flight, each
// on its own replica.  Item i: partition parts[i], its root operation ops[i], n_positions[i]
// <= 8 root positions (<= 4 at 8 rate categories) with branch lengths len1[8 i + a],
// len2[8 i + a]; out[8 i + a] = lnL.
// Every partition is left exactly as rdamd_root_loglikelihood_fused leaves it, and every value
// has that call's bits.  Shapes the one-launch kernel does not take fall back to it item by item.
int rdamd_root_loglikelihood_fused_multi(unsigned int n_items, rdamd_partition_t *const *parts,
                                         const rdamd_operation_t *ops,
                                         const unsigned int *const *params_indices,
                                         const double *len1, const double *len2,
                                         const unsigned int *n_positions, double *out) {
  clear_error();
  if (n_items == 0) return RDAMD_SUCCESS;
  bool fast = true;
  for (unsigned i = 0; i < n_items; ++i) {
    const rdamd_partition *p = parts[i];
    fast = fast && fast_root_shape(p, ops[i]) && p->rate_cats == parts[0]->rate_cats && p->sites > 0 &&
           p->device == parts[0]->device && n_positions[i] >= 1 &&
           n_positions[i] <= root_single_max_positions(p->rate_cats);
  }
  if (!fast || n_items == 1) {
    for (unsigned i = 0; i < n_items; ++i)
      if (rdamd_root_loglikelihood_fused(parts[i], &ops[i], params_indices[i], len1 + 8 * i, len2 + 8 * i,
                                         n_positions[i], out + 8 * i) != RDAMD_SUCCESS)
        return RDAMD_FAILURE;
    return RDAMD_SUCCESS;
  }
  rdamd_partition *lead = parts[0];
  if (!reserve_root_items(lead, n_items)) return RDAMD_FAILURE;
  RootItem *h_items = (RootItem *)lead->h_root_items, *d_items = (RootItem *)lead->d_root_items;
  double *h_res = (double *)(h_items + lead->root_items_cap);
  unsigned max_pos = 0, max_blocks = 0;
  for (unsigned i = 0; i < n_items; ++i) {
    if (!fill_root_item(parts[i], lead, i, ops[i], params_indices[i], len1 + 8 * i, len2 + 8 * i, n_positions[i],
                        h_items[i], h_res + kRootMaxPositions * i))
      return RDAMD_FAILURE;
    max_pos = std::max(max_pos, n_positions[i]);
    max_blocks = std::max(max_blocks, h_items[i].blocks);
  }
  RDAMD_HIP_TRY(hipMemcpyAsync(d_items, h_items, sizeof(RootItem) * n_items, hipMemcpyHostToDevice, lead->stream),
                RDAMD_FAILURE);
  lead->prof_begin(2);
  hipError_t e = launch_root_multi(d_items, n_items, lead->rate_cats, max_pos, max_blocks, lead->stream);
  lead->prof_end();
  RDAMD_HIP_TRY(e, RDAMD_FAILURE);
  RDAMD_HIP_TRY(sync_main(lead), RDAMD_FAILURE);
  for (unsigned i = 0; i < n_items; ++i)
    for (unsigned a = 0; a < n_positions[i]; ++a) out[8 * i + a] = h_res[8 * i + a];
  return RDAMD_SUCCESS;
}

// ---- the pre-order pass (kernels_preorder.hip): marginal ancestral states, branch-length derivatives, site rates ----
static thread_local double g_ancestral_ms = 0.0, g_branch_ms = 0.0;   // what the last call of each pass took

double rdamd_ancestral_last_ms(void) { return g_ancestral_ms; }

int rdamd_marginal_ancestral_nodes(const rdamd_operation_t *ops, unsigned int n_ops, unsigned int *node_clv,
                                   int *node_parent, unsigned int *node_children) {
  clear_error();
  // (host only, no partition: tips are the CLVs below every parent, as the tree numbers them)
  unsigned tips = ~0u;
  for (unsigned i = 0; i < n_ops; ++i) tips = std::min(tips, ops[i].parent_clv_index);
  const OuterPlan plan = plan_outer_program(ops, n_ops, tips);
  if (plan.bad_op >= 0) {
    set_error(64, "rdamd_marginal_ancestral_nodes: operation %d: %s", plan.bad_op, plan.why);
    return RDAMD_FAILURE;
  }
  if (node_parent) node_parent[0] = -1;
  for (unsigned k = 0; k < n_ops; ++k) {
    const OuterOp &d = plan.prog[k];
    const rdamd_operation_t &o = ops[d.op];
    if (node_clv) node_clv[k] = o.parent_clv_index;
    if (node_children) { node_children[2 * k] = o.child1_clv_index; node_children[2 * k + 1] = o.child2_clv_index; }
    for (int c = 0; c < 2; ++c)
      if (d.inner[c] && node_parent) node_parent[d.node[c]] = (int)k;
  }
  return RDAMD_SUCCESS;
}

int rdamd_marginal_ancestral(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                             const unsigned int *freqs_indices, double *post_out) {
  clear_error();
  g_ancestral_ms = 0.0;
  const std::initializer_list<RateIndices> indices = {{freqs_indices, "freqs"}};
  OuterPlan plan;
  if (!preorder_admitted(p, "rdamd_marginal_ancestral", ops, n_ops, !ops || !freqs_indices || !post_out, indices, &plan))
    return RDAMD_FAILURE;
  if (p->sites == 0) return RDAMD_SUCCESS;
  const size_t post_doubles = (size_t)n_ops * p->sites * p->api_states;
  DeviceArray<double> post;
  const auto allocate = [&] { return post.alloc(post_doubles); };
  const auto launch = [&](const OuterOp *d_prog, const unsigned *const *d_indices, double *d_work) {
    return launch_outer_program(p, d_prog, n_ops, plan.slots, d_indices[0], d_work, post.d);
  };
  if (preorder_run(p, plan, indices, &g_ancestral_ms, allocate, launch) != RDAMD_SUCCESS) return RDAMD_FAILURE;
  RDAMD_HIP_TRY(hipMemcpy(post_out, post.d, sizeof(double) * post_doubles, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

// ---- ancestral sequences: the likeliest state of every inner node and column (4-state and binary
// partitions: the posterior launch above; matrix-core 20-state ones: kernels_preorder_k20.hip), then the arg-max
static thread_local double g_sequences_ms = 0.0;

double rdamd_ancestral_sequences_last_ms(void) { return g_sequences_ms; }

int rdamd_ancestral_sequences(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                              const unsigned int *freqs_indices, uint8_t *state_out, double *prob_out, double *post_out) {
  clear_error();
  g_sequences_ms = 0.0;
  const std::initializer_list<RateIndices> indices = {{freqs_indices, "freqs"}};
  OuterPlan plan;
  if (!preorder_admitted(p, "rdamd_ancestral_sequences", ops, n_ops, !ops || !freqs_indices, indices, &plan,
                         sequences_refused))
    return RDAMD_FAILURE;
  if (p->sites == 0) return RDAMD_SUCCESS;
  const unsigned K = p->api_states;
  const size_t rows = (size_t)n_ops * p->sites;
  DeviceArray<double> post, prob;   // the table stays on the device unless the caller asks for it
  DeviceArray<uint8_t> state;
  const auto allocate = [&] {
    hipError_t e = post.alloc(rows * K);
    if (e == hipSuccess) e = prob.alloc(rows);
    if (e == hipSuccess) e = state.alloc(rows);
    if (e == hipSuccess) e = flush_tiptab(p);
    return e;
  };
  const auto launch = [&](const OuterOp *d_prog, const unsigned *const *d_indices, double *d_work) {
    hipError_t e = p->mfma_layout ? launch_outer_program_k20(p, d_prog, n_ops, d_indices[0], d_work, post.d)
                                  : launch_outer_program(p, d_prog, n_ops, plan.slots, d_indices[0], d_work, post.d);
    if (e == hipSuccess) e = launch_ancestral_argmax(p, post.d, rows, K, state.d, prob.d);
    return e;
  };
  if (preorder_run(p, plan, indices, &g_sequences_ms, allocate, launch) != RDAMD_SUCCESS) return RDAMD_FAILURE;
  hipError_t e = hipSuccess;
  if (state_out) e = hipMemcpy(state_out, state.d, rows, hipMemcpyDeviceToHost);
  if (e == hipSuccess && prob_out) e = hipMemcpy(prob_out, prob.d, sizeof(double) * rows, hipMemcpyDeviceToHost);
  if (e == hipSuccess && post_out) e = hipMemcpy(post_out, post.d, sizeof(double) * rows * K, hipMemcpyDeviceToHost);
  if (e != hipSuccess) g_sequences_ms = 0.0;
  RDAMD_HIP_TRY(e, RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

unsigned int rdamd_marginal_ancestral_workspace_slots(const rdamd_operation_t *ops, unsigned int n_ops, unsigned int tips) {
  clear_error();
  const OuterPlan plan = plan_outer_program(ops, n_ops, tips);
  if (plan.bad_op >= 0) {
    set_error(64, "rdamd_marginal_ancestral_workspace_slots: operation %d: %s", plan.bad_op, plan.why);
    return ~0u;
  }
  return plan.slots;
}

double rdamd_branch_last_ms(void) { return g_branch_ms; }

// rdamd_branch_derivatives and rdamd_branch_length_derivatives: one body, the entry point's name
// (`what`) and the shapes it refuses (`refused`) apart.  A matrix-core 20-state partition, which only
// the second admits, runs kernels_preorder_k20.hip's consumer; every other shape the launch it always ran.
static int branch_derivatives_call(rdamd_partition_t *p, const char *what, bool (*refused)(const rdamd_partition *, const char *),
                                   const rdamd_operation_t *ops, unsigned int n_ops, const unsigned int *params_indices,
                                   const unsigned int *freqs_indices, double *d1_out, double *d2_out) {
  clear_error();
  g_branch_ms = 0.0;
  const std::initializer_list<RateIndices> indices = {{params_indices, "params"}, {freqs_indices, "freqs"}};
  OuterPlan plan;
  if (!preorder_admitted(p, what, ops, n_ops, !ops || !params_indices || !freqs_indices || !d1_out, indices, &plan, refused))
    return RDAMD_FAILURE;
  const size_t entries = (size_t)n_ops * 4;
  std::fill(d1_out, d1_out + 2 * (size_t)n_ops, 0.0);
  if (d2_out) std::fill(d2_out, d2_out + 2 * (size_t)n_ops, 0.0);
  if (p->sites == 0) return RDAMD_SUCCESS;
  const bool k20 = p->mfma_layout;
  DeviceArray<double> partials, sums;   // [workgroup][entry] and [entry]
  DeviceArray<unsigned> bad_sites;      // the count of sites without a likelihood
  // 20 states: the MFMA-ready copy of the rate matrix of every category, from the rate matrices as flush_q builds them
  DeviceArray<double> qcopy;
  std::vector<double> h_qcopy;
  if (k20) {
    const unsigned R = p->rate_cats, K = p->states;
    std::vector<double> q((size_t)K * K);
    h_qcopy.resize((size_t)R * kK20CopyDoubles);
    for (unsigned r = 0; r < R; ++r) {
      const unsigned m = params_indices[r];
      build_q_host(K, p->subst[m].data(), p->freqs[m].data(), q.data());
      k20_pack_copy(q.data(), h_qcopy.data() + (size_t)r * kK20CopyDoubles);
    }
  }
  const auto allocate = [&] {
    hipError_t e = partials.alloc(entries * (k20 ? p->clv_tiles() : preorder_blocks(p)));
    if (e == hipSuccess) e = sums.alloc(entries);
    if (e == hipSuccess) e = bad_sites.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(bad_sites.d, 0, sizeof(unsigned), p->stream);
    if (e == hipSuccess && k20) e = qcopy.alloc(h_qcopy.size());
    if (e == hipSuccess && k20) e = hipMemcpy(qcopy.d, h_qcopy.data(), sizeof(double) * h_qcopy.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && k20) e = flush_tiptab(p);
    return e;
  };
  const auto launch = [&](const OuterOp *d_prog, const unsigned *const *d_indices, double *d_work) {
    if (k20)
      return launch_brlen_program_k20(p, d_prog, n_ops, d_indices[1], d_work, qcopy.d, partials.d, bad_sites.d,
                                      d2_out != nullptr, sums.d);
    return launch_brlen_program(p, d_prog, n_ops, plan.slots, d_indices[0], d_indices[1], d_work, partials.d, bad_sites.d,
                                sums.d);
  };
  if (preorder_run(p, plan, indices, &g_branch_ms, allocate, launch) != RDAMD_SUCCESS) return RDAMD_FAILURE;
  unsigned bad = 0;
  RDAMD_HIP_TRY(hipMemcpy(&bad, bad_sites.d, sizeof bad, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (bad) {
    g_branch_ms = 0.0;   // (a call that returns nothing reports no time)
    set_error(65, "%s: %u of %u sites have a likelihood that is 0 or not finite; no derivative is returned", what, bad,
              p->sites);
    return RDAMD_FAILURE;
  }
  std::vector<double> host(entries);
  RDAMD_HIP_TRY(hipMemcpy(host.data(), sums.d, sizeof(double) * entries, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  for (size_t k = 0; k < n_ops; ++k)
    for (size_t c = 0; c < 2; ++c) {
      d1_out[2 * k + c] = host[4 * k + 2 * c];
      if (d2_out) d2_out[2 * k + c] = host[4 * k + 2 * c + 1];
    }
  return RDAMD_SUCCESS;
}

int rdamd_branch_derivatives(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                             const unsigned int *params_indices, const unsigned int *freqs_indices,
                             double *d1_out, double *d2_out) {
  return branch_derivatives_call(p, "rdamd_branch_derivatives", outer_refused, ops, n_ops, params_indices, freqs_indices,
                                 d1_out, d2_out);
}

int rdamd_branch_length_derivatives(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                                    const unsigned int *params_indices, const unsigned int *freqs_indices,
                                    double *d1_out, double *d2_out) {
  return branch_derivatives_call(p, "rdamd_branch_length_derivatives", derivatives_refused, ops, n_ops, params_indices,
                                 freqs_indices, d1_out, d2_out);
}

static thread_local double g_pair_sums_ms = 0.0;
// rdamd_pair_sums, 20 states, workspace_bytes = 0: the partial sums of one pass (a tile's row is 5.1 MB
// on a 200-taxon tree with four categories, 256 MiB a pass of 52 workgroups; measured in
// profiles/r20_k20_pair_sums.md: 25.2 ms at 256 MiB, 6.7 ms at 1 GiB, 5.0 ms in one pass of 3.2 GB)
constexpr size_t kK20PairSumWorkspace = (size_t)1 << 30;

double rdamd_pair_sums_last_ms(void) { return g_pair_sums_ms; }

// rdamd_branch_pair_sums and rdamd_pair_sums: one body, the entry point's name (`what`) and the shapes
// it refuses (`refused`) apart.  A matrix-core 20-state partition, which only the second admits, runs
// kernels_preorder_k20.hip's consumer, one row of partials per tile; every other shape the launches it
// always ran.  KW: the states of the walk's rows (the caller's KA are the first of them).
static int pair_sums_call(rdamd_partition_t *p, const char *what, bool (*refused)(const rdamd_partition *, const char *),
                          const rdamd_operation_t *ops, unsigned int n_ops, const unsigned int *freqs_indices,
                          size_t workspace_bytes, double *pair_out, double *root_out, double *cat_out) {
  clear_error();
  g_pair_sums_ms = 0.0;
  const std::initializer_list<RateIndices> indices = {{freqs_indices, "freqs"}};
  OuterPlan plan;
  if (!preorder_admitted(p, what, ops, n_ops, !ops || !freqs_indices, indices, &plan, refused)) return RDAMD_FAILURE;
  if (!pair_out) {
    set_error(67, "%s: pair_out is null", what);
    return RDAMD_FAILURE;
  }
  const bool k20 = p->mfma_layout;
  const size_t R = p->rate_cats, KA = p->api_states;
  std::fill(pair_out, pair_out + (size_t)n_ops * 2 * R * KA * KA, 0.0);
  if (root_out) std::fill(root_out, root_out + R * KA, 0.0);
  if (cat_out) std::fill(cat_out, cat_out + R, 0.0);
  if (p->sites == 0 || n_ops == 0) return RDAMD_SUCCESS;
  // passes over whole workgroups: as many rows of partials as the bound holds, never less than one
  const size_t entries = k20 ? k20_pair_sum_entries(n_ops, R) : pair_sum_doubles(p, n_ops);
  if (workspace_bytes == 0) workspace_bytes = k20 ? kK20PairSumWorkspace : (size_t)256 << 20;
  const unsigned blocks = k20 ? p->clv_tiles() : preorder_blocks(p);
  const unsigned per_pass =
      (unsigned)std::min<size_t>(blocks, std::max<size_t>(1, workspace_bytes / (entries * sizeof(double))));
  DeviceArray<double> partials, stage, sums;
  DeviceArray<unsigned> bad_sites;
  const auto allocate = [&] {
    hipError_t e = partials.alloc(entries * per_pass);
    if (e == hipSuccess) e = stage.alloc(std::max<size_t>(1, k20 ? 0 : pair_sum_stage_doubles(p, per_pass)));
    if (e == hipSuccess) e = sums.alloc(entries);
    if (e == hipSuccess) e = bad_sites.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(bad_sites.d, 0, sizeof(unsigned), p->stream);
    if (e == hipSuccess && k20) e = flush_tiptab(p);
    return e;
  };
  const auto launch = [&](const OuterOp *d_prog, const unsigned *const *d_indices, double *d_work) {
    if (k20)
      return launch_pair_sum_program_k20(p, d_prog, n_ops, d_indices[0], d_work, partials.d, per_pass, bad_sites.d, sums.d);
    return launch_pair_sum_program(p, d_prog, n_ops, plan.slots, d_indices[0], d_work, partials.d, stage.d, per_pass,
                                   bad_sites.d, sums.d);
  };
  if (preorder_run(p, plan, indices, &g_pair_sums_ms, allocate, launch) != RDAMD_SUCCESS) return RDAMD_FAILURE;
  unsigned bad = 0;
  RDAMD_HIP_TRY(hipMemcpy(&bad, bad_sites.d, sizeof bad, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (bad) {
    g_pair_sums_ms = 0.0;   // (a call that returns nothing reports no time)
    set_error(65, "%s: %u of %u sites have a likelihood that is 0 or not finite; no sum is returned", what, bad, p->sites);
    return RDAMD_FAILURE;
  }
  std::vector<double> host(entries);
  RDAMD_HIP_TRY(hipMemcpy(host.data(), sums.d, sizeof(double) * entries, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  // the caller's states are the first KA of the walk's KW (4, or 20 on the matrix cores)
  const size_t KW = k20 ? kK20States : 4;
  for (size_t b = 0; b < (size_t)n_ops * 2 * R; ++b)
    for (size_t i = 0; i < KA; ++i)
      for (size_t j = 0; j < KA; ++j) pair_out[(b * KA + i) * KA + j] = host[(b * KW + i) * KW + j];
  const double *root = host.data() + (size_t)n_ops * 2 * R * KW * KW;
  for (size_t r = 0; r < R; ++r) {
    if (root_out)
      for (size_t i = 0; i < KA; ++i) root_out[r * KA + i] = root[r * (KW + 1) + i];
    if (cat_out) cat_out[r] = root[r * (KW + 1) + KW];
  }
  return RDAMD_SUCCESS;
}

int rdamd_branch_pair_sums(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                           const unsigned int *freqs_indices, size_t workspace_bytes, double *pair_out,
                           double *root_out, double *cat_out) {
  return pair_sums_call(p, "rdamd_branch_pair_sums", outer_refused, ops, n_ops, freqs_indices, workspace_bytes, pair_out,
                        root_out, cat_out);
}

int rdamd_pair_sums(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops, const unsigned int *freqs_indices,
                    size_t workspace_bytes, double *pair_out, double *root_out, double *cat_out) {
  return pair_sums_call(p, "rdamd_pair_sums", pair_sums_refused, ops, n_ops, freqs_indices, workspace_bytes, pair_out,
                        root_out, cat_out);
}

static thread_local double g_subst_ms = 0.0;

double rdamd_branch_substitutions_last_ms(void) { return g_subst_ms; }

int rdamd_branch_substitutions(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                               const unsigned int *params_indices, const unsigned int *freqs_indices,
                               const double *lengths, double *change_out, double *count_out,
                               unsigned char *top_pair_out, double *top_prob_out, double *joint_out) {
  clear_error();
  g_subst_ms = 0.0;
  const char *what = "rdamd_branch_substitutions";
  const std::initializer_list<RateIndices> indices = {{params_indices, "params"}, {freqs_indices, "freqs"}};
  OuterPlan plan;
  if (!preorder_admitted(p, what, ops, n_ops, !ops || !params_indices || !freqs_indices || !lengths, indices, &plan))
    return RDAMD_FAILURE;
  const size_t branches = (size_t)n_ops * 2;
  for (size_t b = 0; b < branches; ++b)
    if (!length_ok(lengths[b])) {
      set_error(64, "%s: the length of branch (%zu, %zu) is negative or not finite", what, b / 2, b % 2);
      return RDAMD_FAILURE;
    }
  if (p->sites == 0 || n_ops == 0) return RDAMD_SUCCESS;
  // the count matrices, from the rate matrices as flush_q builds them
  const unsigned R = p->rate_cats, K = p->states;
  const size_t KA = p->api_states, cells = branches * p->sites;
  std::vector<double> q((size_t)p->rate_matrices * K * K), cmat(branches * R * K * K);
  for (unsigned m = 0; m < p->rate_matrices; ++m)
    build_q_host(K, p->subst[m].data(), p->freqs[m].data(), q.data() + (size_t)m * K * K);
  smap::count_matrices(K, R, q.data(), params_indices, p->rates.data(), lengths, branches, cmat.data());
  DeviceArray<double> d_cmat, change, count, top_prob, joint;
  DeviceArray<uint8_t> top_pair;
  DeviceArray<unsigned> bad_sites;
  const auto allocate = [&] {
    hipError_t e = d_cmat.alloc(cmat.size());
    if (e == hipSuccess && change_out) e = change.alloc(cells);
    if (e == hipSuccess && count_out) e = count.alloc(cells);
    if (e == hipSuccess && top_pair_out) e = top_pair.alloc(cells);
    if (e == hipSuccess && top_prob_out) e = top_prob.alloc(cells);
    if (e == hipSuccess && joint_out) e = joint.alloc(cells * KA * KA);
    if (e == hipSuccess) e = bad_sites.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(bad_sites.d, 0, sizeof(unsigned), p->stream);
    if (e == hipSuccess) e = hipMemcpy(d_cmat.d, cmat.data(), sizeof(double) * cmat.size(), hipMemcpyHostToDevice);
    return e;
  };
  const auto launch = [&](const OuterOp *d_prog, const unsigned *const *d_indices, double *d_work) {
    return launch_subst_program(p, d_prog, n_ops, plan.slots, d_indices[1], d_work, d_cmat.d, bad_sites.d, change.d, count.d,
                                top_pair.d, top_prob.d, joint.d);
  };
  if (preorder_run(p, plan, indices, &g_subst_ms, allocate, launch) != RDAMD_SUCCESS) return RDAMD_FAILURE;
  unsigned bad = 0;
  RDAMD_HIP_TRY(hipMemcpy(&bad, bad_sites.d, sizeof bad, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (bad) {
    g_subst_ms = 0.0;   // (a call that returns nothing reports no time)
    set_error(65, "%s: %u of %u sites have a likelihood that is 0 or not finite; nothing is returned", what, bad, p->sites);
    return RDAMD_FAILURE;
  }
  if (change_out) RDAMD_HIP_TRY(hipMemcpy(change_out, change.d, sizeof(double) * cells, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (count_out) RDAMD_HIP_TRY(hipMemcpy(count_out, count.d, sizeof(double) * cells, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (top_pair_out) RDAMD_HIP_TRY(hipMemcpy(top_pair_out, top_pair.d, cells, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (top_prob_out) RDAMD_HIP_TRY(hipMemcpy(top_prob_out, top_prob.d, sizeof(double) * cells, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (joint_out)
    RDAMD_HIP_TRY(hipMemcpy(joint_out, joint.d, sizeof(double) * cells * KA * KA, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

int rdamd_site_rate_posteriors(rdamd_partition_t *p, unsigned int clv_index, int scaler_index,
                               const unsigned int *freqs_indices, double *cat_out, double *mean_rate_out) {
  clear_error();
  if (p->mfma_layout) {
    set_error(63, "rdamd_site_rate_posteriors: %u-state partitions in the matrix-core CLV layout are not supported",
              p->api_states);
    return RDAMD_FAILURE;
  }
  if (!root_index_ok(p, clv_index, scaler_index)) {
    set_error(11, "rdamd_site_rate_posteriors: index out of range (clv %u, scaler %d)", clv_index, scaler_index);
    return RDAMD_FAILURE;
  }
  if (!freqs_indices || bad_rate_index(p, freqs_indices)) {
    set_error(7, "rdamd_site_rate_posteriors: freqs index out of range");
    return RDAMD_FAILURE;
  }
  if (p->sites == 0 || (!cat_out && !mean_rate_out)) return RDAMD_SUCCESS;
  const size_t S = p->sites, R = p->rate_cats;
  DeviceArray<double> cat, mean;
  RDAMD_HIP_TRY(clv_phys(p, clv_index, &clv_index), RDAMD_FAILURE);
  RDAMD_HIP_TRY(flush_q(p), RDAMD_FAILURE);
  RDAMD_HIP_TRY(ensure_scratch(p, sizeof(unsigned) * R + 1024), RDAMD_FAILURE);
  if (cat_out) RDAMD_HIP_TRY(cat.alloc(S * R), RDAMD_FAILURE);
  if (mean_rate_out) RDAMD_HIP_TRY(mean.alloc(S), RDAMD_FAILURE);
  Scratch sc{p};
  unsigned *d_fi = (unsigned *)sc.take(sizeof(unsigned) * R);
  RDAMD_HIP_TRY(upload(p, d_fi, freqs_indices, sizeof(unsigned) * R), RDAMD_FAILURE);
  p->prof_begin(5);
  const hipError_t le = launch_site_rates(p, clv_index, d_fi, cat.d, mean.d);
  p->prof_end();
  RDAMD_HIP_TRY(le, RDAMD_FAILURE);
  RDAMD_HIP_TRY(sync_main(p), RDAMD_FAILURE);
  if (cat_out) RDAMD_HIP_TRY(hipMemcpy(cat_out, cat.d, sizeof(double) * S * R, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  if (mean_rate_out)
    RDAMD_HIP_TRY(hipMemcpy(mean_rate_out, mean.d, sizeof(double) * S, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

int rdamd_get_clv(rdamd_partition_t *p, unsigned int clv_index, double *out) {
  clear_error();
  const size_t S = p->sites, R = p->rate_cats, K = p->states, KA = p->api_states;
  if (clv_index < p->tips) {  // tips live as codes; expand on the host
    const uint8_t *row = p->tipcodes.data() + (size_t)clv_index * S;
    for (size_t s = 0; s < S; ++s) {
      uint64_t mask = p->codemask[row[s]];
      for (size_t r = 0; r < R; ++r)
        for (size_t j = 0; j < KA; ++j) out[(s * R + r) * KA + j] = (double)((mask >> j) & 1);
    }
    return RDAMD_SUCCESS;
  }
  if (clv_index >= p->tips + p->clv_buffers) {
    set_error(11, "rdamd_get_clv: index out of range");
    return RDAMD_FAILURE;
  }
  RDAMD_HIP_TRY(clv_phys(p, clv_index, &clv_index), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipStreamSynchronize(p->stream), RDAMD_FAILURE);
  const double *src = p->d_clv + (size_t)(clv_index - p->tips) * p->clv_doubles();
  if (p->mfma_layout) {   // device: [rate][tile][operand layout] -> the ABI's [site][rate][state]
    std::vector<double> dev(p->clv_doubles());
    RDAMD_HIP_TRY(hipMemcpy(dev.data(), src, sizeof(double) * dev.size(), hipMemcpyDeviceToHost),
                  RDAMD_FAILURE);
    const size_t tiles = p->clv_tiles();
    for (size_t s = 0; s < S; ++s)
      for (size_t r = 0; r < R; ++r) {
        const double *tile = dev.data() + (r * tiles + s / 16) * (16 * K);
        for (size_t j = 0; j < KA; ++j)
          out[(s * R + r) * KA + j] = tile[k20_tile_index((unsigned)(s % 16), (unsigned)j)];
      }
    return RDAMD_SUCCESS;
  }
  if (!p->embedded()) {
    RDAMD_HIP_TRY(hipMemcpy(out, src, sizeof(double) * S * R * K, hipMemcpyDeviceToHost), RDAMD_FAILURE);
    return RDAMD_SUCCESS;
  }
  std::vector<double> wide(S * R * K);   // the caller's states are the first KA of every K
  RDAMD_HIP_TRY(hipMemcpy(wide.data(), src, sizeof(double) * S * R * K, hipMemcpyDeviceToHost),
                RDAMD_FAILURE);
  for (size_t e = 0; e < S * R; ++e)
    for (size_t j = 0; j < KA; ++j) out[e * KA + j] = wide[e * K + j];
  return RDAMD_SUCCESS;
}

int rdamd_get_scaler(rdamd_partition_t *p, unsigned int scaler_index, unsigned int *out) {
  clear_error();
  if (scaler_index >= p->scale_buffers) {
    set_error(11, "rdamd_get_scaler: index out of range");
    return RDAMD_FAILURE;
  }
  int phys_sc = (int)scaler_index;
  RDAMD_HIP_TRY(scaler_phys(p, (int)scaler_index, &phys_sc), RDAMD_FAILURE);
  scaler_index = (unsigned)phys_sc;
  RDAMD_HIP_TRY(hipStreamSynchronize(p->stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(out, p->d_scaler + (size_t)scaler_index * p->sites,
                          sizeof(unsigned) * p->sites, hipMemcpyDeviceToHost), RDAMD_FAILURE);
  return RDAMD_SUCCESS;
}

int rdamd_get_pmatrix(rdamd_partition_t *p, unsigned int matrix_index, double *out) {
  clear_error();
  if (matrix_index >= p->prob_matrices) {
    set_error(8, "rdamd_get_pmatrix: index out of range");
    return RDAMD_FAILURE;
  }
  const size_t K = p->states, KA = p->api_states, n = (size_t)p->rate_cats * K * K;
  RDAMD_HIP_TRY(hipStreamSynchronize(p->stream), RDAMD_FAILURE);
  if (!p->embedded()) {
    RDAMD_HIP_TRY(hipMemcpy(out, p->d_pmat + (size_t)matrix_index * n, sizeof(double) * n,
                            hipMemcpyDeviceToHost), RDAMD_FAILURE);
    return RDAMD_SUCCESS;
  }
  std::vector<double> wide(n);
  RDAMD_HIP_TRY(hipMemcpy(wide.data(), p->d_pmat + (size_t)matrix_index * n, sizeof(double) * n,
                          hipMemcpyDeviceToHost), RDAMD_FAILURE);
  for (size_t r = 0; r < p->rate_cats; ++r)
    for (size_t i = 0; i < KA; ++i)
      for (size_t j = 0; j < KA; ++j) out[(r * KA + i) * KA + j] = wide[(r * K + i) * K + j];
  return RDAMD_SUCCESS;
}

void rdamd_profile_enable(rdamd_partition_t *p, int on) {
  (void)hipStreamSynchronize(p->stream);
  for (auto &sp : p->prof_spans) { p->prof_pool.push_back(sp.a); p->prof_pool.push_back(sp.b); }
  p->prof_spans.clear();
  p->profiling = on != 0;
}

int rdamd_profile_read(rdamd_partition_t *p, double ms_out[8], unsigned int launches_out[8]) {
  clear_error();
  RDAMD_HIP_TRY(hipStreamSynchronize(p->stream), RDAMD_FAILURE);
  for (int k = 0; k < 8; ++k) { ms_out[k] = 0.0; launches_out[k] = 0; }
  for (auto &sp : p->prof_spans) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess && sp.kind >= 0 && sp.kind < 8) {
      ms_out[sp.kind] += ms;
      launches_out[sp.kind] += 1;
    }
    p->prof_pool.push_back(sp.a);
    p->prof_pool.push_back(sp.b);
  }
  p->prof_spans.clear();
  return RDAMD_SUCCESS;
}

void rdamd_partition_sync(rdamd_partition_t *p) {
  if (p && p->stream) (void)hipStreamSynchronize(p->stream);
}

}  // extern "C"
