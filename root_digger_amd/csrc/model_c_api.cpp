// C wrappers over model_t (declared in include/root_digger_amd.h).
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include <algorithm>

#include "common.hpp"
#include "batch_combiner.hpp"
#include "checkpoint.hpp"
#include "lockstep_conductor.hpp"
#include "model.hpp"
#include "partition_info.hpp"
#include "tree_c_api.hpp"

struct rdamd_model {
  rdamd::model_t *model = nullptr;
  // [partition], in file order: what a replica is made of (parallel exhaustive search)
  std::vector<rdamd::msa_t> msas;
  std::vector<rdamd::ratehet_opts_t> ratehets;
  uint64_t seed = 0;
  bool     early_stop = false;
  void    *setulb = nullptr;
  rdamd::checkpoint_t *checkpoint = nullptr;
  std::unique_ptr<rdamd::model_t::progress_t> progress;   // set by rdamd_model_set_progress
  int lockstep_priority = 1;      // stream priority of the shared objective partition in a lock-stepped search
  bool children_only = true;      // rdamd_model_set_root_children_only
  unsigned lockstep_groups = 0;   // 0: the library's choice; 1: one group, blocking launches (rdamd_model_set_lockstep_groups)
  uint64_t lockstep_stats[4] = {0, 0, 0, 0};   // of the last lock-stepped search (rdamd_model_lockstep_stats)
  uint64_t round_stats[3] = {0, 0, 0};         // ... in rounds: rounds, collectives, second-pass redos
  std::vector<uint64_t> round_part_stats;      // ... per objective partition: launches, second-pass launches
  double round_seconds[4] = {0, 0, 0, 0};      // ... and the host time of the rounds' phases
  struct async_reducer_t { rdamd_lnl_reducer_t queue; void *user; };   // rdamd_model_set_lnl_reducer_async
  std::unique_ptr<async_reducer_t> async_reducer;
  int lockstep_rounds = -1;       // -1: rounds for site-sharded models only; 0 never; 1 always (rdamd_model_set_lockstep_rounds)
  ~rdamd_model() { delete model; }
};

using rdamd::root_location_t;

rdamd::checkpoint_t *rdamd_checkpoint_cpp(rdamd_checkpoint_t *c);   // checkpoint_c_api.cpp

namespace {
root_location_t to_cpp(const rdamd_root_location_t *rl) {
  root_location_t r;
  r.edge = rl->edge; r.id = (size_t)rl->id; r.saved_brlen = rl->saved_brlen;
  r.brlen_ratio = rl->brlen_ratio;
  return r;
}
void to_c(const root_location_t &r, rdamd_root_location_t *out) {
  out->edge = r.edge; out->id = r.id; out->saved_brlen = r.saved_brlen;
  out->brlen_ratio = r.brlen_ratio;
}
}  // namespace

#define GUARD(failret, ...)                             \
  try {                                                 \
    rdamd::clear_error();                               \
    __VA_ARGS__                                         \
  } catch (const std::exception &e) {                   \
    rdamd::set_error(50, "%s", e.what());               \
    return failret;                                     \
  }

extern "C" {

// The one way a model is made: its partitions' alignments and rate heterogeneity, in file order.
// `check`: the taxa of the tree and of every alignment must agree.  n_partitions / patterns[partition]
// (optional) are written once the model exists.
static rdamd_model_t *build_model(const rdamd_tree_t *tree, std::vector<rdamd::msa_t> msas,
                                  std::vector<rdamd::ratehet_opts_t> ratehets, uint64_t seed, int early_stop,
                                  bool check, unsigned int *n_partitions = nullptr, unsigned int *patterns = nullptr) {
  if (check)
    for (const auto &x : msas)
      if (!x.constiency_check(rdamd_tree_cpp(tree).label_set()))
        throw std::invalid_argument("Taxa on the tree and in the MSA are inconsistient");
  std::unique_ptr<rdamd_model_t> m(new rdamd_model());
  m->msas = std::move(msas);
  m->ratehets = std::move(ratehets);
  m->seed = seed; m->early_stop = early_stop != 0;
  m->model = new rdamd::model_t(rdamd_tree_cpp(tree), m->msas, m->ratehets, false, seed, m->early_stop);
  if (n_partitions) *n_partitions = (unsigned)m->msas.size();
  if (patterns)
    for (size_t p = 0; p < m->msas.size(); ++p) patterns[p] = (unsigned)m->msas[p].length();
  return m.release();
}
// columns [lo, hi) of site block `block` of n_blocks over len columns (src/model.cpp:1899-1907)
static std::pair<size_t, size_t> site_block(size_t len, size_t block, size_t n_blocks) {
  const size_t size = len / n_blocks, mod = len % n_blocks;
  return {size * block + std::min(mod, block), size * (block + 1) + std::min(mod, block + 1)};
}
static rdamd::ratehet_opts_t to_cpp(const rdamd_ratehet_opts_t *ratehet) {
  rdamd::ratehet_opts_t rc(ratehet->rate_cats ? ratehet->rate_cats : 1);
  rc.type = (rdamd::param_type)ratehet->type;
  rc.rate_category_type = (rdamd::rate_category)ratehet->rate_category_type;
  rc.alpha_init = ratehet->alpha_init != 0;
  rc.alpha = ratehet->alpha;
  return rc;
}
// the partition file's partitions, in file order (none: refused), and their rate heterogeneity
static rdamd::msa_partitions_t read_partition_file(const char *partition_filename,
                                                   std::vector<rdamd::ratehet_opts_t> *ratehets) {
  auto infos = rdamd::parse_partition_file(partition_filename);
  if (infos.empty()) throw std::runtime_error("The partition file holds no partitions");
  for (const auto &pi : infos) {
    rdamd::ratehet_opts_t rc = pi.model.ratehet_opts;
    if (rc.rate_cats == 0) rc.rate_cats = 1;
    ratehets->push_back(rc);
  }
  return infos;
}

rdamd_model_t *rdamd_model_create(const rdamd_tree_t *tree, unsigned int n_taxa,
                                  const char *const *labels, const char *const *sequences,
                                  const unsigned int *weights, unsigned int states,
                                  const uint64_t *map, unsigned int rate_cats, uint64_t seed,
                                  int early_stop) {
  GUARD(nullptr, {
    rdamd::msa_t msa;
    msa.states = states;
    msa.set_map(map);
    for (unsigned i = 0; i < n_taxa; ++i) {
      msa.labels.emplace_back(labels[i]);
      msa.sequences.emplace_back(sequences[i]);
    }
    if (weights) msa.weights.assign(weights, weights + msa.length());
    // (the caller's sequences are not checked against the tree: they never were)
    return build_model(tree, {msa}, {rdamd::ratehet_opts_t(rate_cats)}, seed, early_stop, false);
  })
}
static rdamd_model_t *create_from_file(const rdamd_tree_t *tree, const char *msa_filename,
                                       unsigned int states, const uint64_t *map,
                                       const rdamd::ratehet_opts_t &rc, uint64_t seed,
                                       int early_stop, int compress, unsigned int *n_patterns,
                                       unsigned int block = 0, unsigned int n_blocks = 1,
                                       unsigned int *n_columns = nullptr) {
  GUARD(nullptr, {
    rdamd::msa_t msa;
    if (n_blocks <= 1) {
      msa = rdamd::msa_t::from_file(msa_filename, map, states, compress != 0);
      if (n_columns) *n_columns = msa.total_weight();
    } else {   // one site block of a site-sharded run: cut first, compress the block
      if (block >= n_blocks) throw std::invalid_argument("site block index out of range");
      const rdamd::msa_t whole = rdamd::msa_t::from_file(msa_filename, map, states, false);
      const auto cols = site_block(whole.length(), block, n_blocks);
      if (cols.first == cols.second) throw std::invalid_argument("more site blocks than alignment columns");
      msa = whole.columns(cols.first, cols.second);
      if (compress) msa.compress();
      if (n_columns) *n_columns = (unsigned)whole.length();
    }
    return build_model(tree, {msa}, {rc}, seed, early_stop, true, nullptr, n_patterns);
  })
}
rdamd_model_t *rdamd_model_create_from_file(const rdamd_tree_t *tree, const char *msa_filename,
                                            unsigned int states, const uint64_t *map,
                                            unsigned int rate_cats, uint64_t seed,
                                            int early_stop, int compress,
                                            unsigned int *n_patterns) {
  return create_from_file(tree, msa_filename, states, map, rdamd::ratehet_opts_t(rate_cats), seed,
                          early_stop, compress, n_patterns);
}
rdamd_model_t *rdamd_model_create_from_file_ratehet(const rdamd_tree_t *tree,
                                                    const char *msa_filename,
                                                    unsigned int states, const uint64_t *map,
                                                    const rdamd_ratehet_opts_t *ratehet,
                                                    uint64_t seed, int early_stop, int compress,
                                                    unsigned int *n_patterns) {
  return create_from_file(tree, msa_filename, states, map, to_cpp(ratehet), seed, early_stop, compress,
                          n_patterns);
}
rdamd_model_t *rdamd_model_create_from_file_block(const rdamd_tree_t *tree, const char *msa_filename,
                                                  unsigned int states, const uint64_t *map,
                                                  const rdamd_ratehet_opts_t *ratehet,
                                                  uint64_t seed, int early_stop, int compress,
                                                  unsigned int block, unsigned int n_blocks,
                                                  unsigned int *n_patterns,
                                                  unsigned int *n_columns) {
  return create_from_file(tree, msa_filename, states, map, to_cpp(ratehet), seed, early_stop, compress,
                          n_patterns, block, n_blocks, n_columns);
}
int rdamd_model_set_lnl_reducer(rdamd_model_t *m, rdamd_lnl_reducer_t reduce, void *user,
                                int on_device) {
  GUARD(RDAMD_FAILURE, {
    m->model->set_lnl_reducer(reduce, user, on_device != 0);
    // the ready-made RCCL reducer comes with its two halves
    if (reduce == rdamd_comm_reducer && on_device) {
      m->model->set_lnl_reducer_async(rdamd_comm_reducer_queue, rdamd_comm_reducer_wait, user);
      m->model->set_lnl_reducer_abort([](void *u) { rdamd_comm_abort((rdamd_comm_t *)u); }, user);
    }
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_set_lnl_reducer_abort(rdamd_model_t *m, rdamd_lnl_abort_t abort, void *user) {
  GUARD(RDAMD_FAILURE, {
    if (!m->model->site_sharded()) throw std::invalid_argument("set_lnl_reducer_abort: set the reducer first");
    m->model->set_lnl_reducer_abort(abort, user);
    return RDAMD_SUCCESS;
  })
}
// the blocking form of a two-halves reducer: queue, then wait for the stream
static int blocking_from_async(double *values, unsigned int n, void *stream, void *user) {
  auto *a = (rdamd_model::async_reducer_t *)user;
  if (a->queue(values, n, stream, a->user) != RDAMD_SUCCESS) return RDAMD_FAILURE;
  return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? RDAMD_SUCCESS : RDAMD_FAILURE;
}
int rdamd_model_set_lnl_reducer_async(rdamd_model_t *m, rdamd_lnl_reducer_t queue, rdamd_lnl_wait_t wait,
                                      void *user) {
  GUARD(RDAMD_FAILURE, {
    if (!queue || !wait) throw std::invalid_argument("set_lnl_reducer_async: both halves are required");
    m->async_reducer.reset(new rdamd_model::async_reducer_t{queue, user});
    m->model->set_lnl_reducer(blocking_from_async, m->async_reducer.get(), true);
    m->model->set_lnl_reducer_async(queue, wait, user);
    return RDAMD_SUCCESS;
  })
}
// The reference's partitioned set-up (src/main.cpp:512-555): the alignment is read
// whole, cut into the partition file's column ranges, each partition compressed
// on its own; rate categories come from each partition's model string.
rdamd_model_t *rdamd_model_create_partitioned(const rdamd_tree_t *tree, const char *msa_filename,
                                              const char *partition_filename,
                                              unsigned int states, const uint64_t *map,
                                              uint64_t seed, int early_stop,
                                              unsigned int *n_partitions) {
  GUARD(nullptr, {
    const rdamd::msa_t whole = rdamd::msa_t::from_file(msa_filename, map, states, false);
    std::vector<rdamd::ratehet_opts_t> ratehets;
    const auto infos = read_partition_file(partition_filename, &ratehets);
    return build_model(tree, rdamd::partition_msa(whole, infos, true), ratehets, seed, early_stop, true,
                       n_partitions);
  })
}

// One rank's block of the partitioned model: every partition's own columns (its ranges, in file
// order) are cut into n_blocks contiguous blocks by the chunking of src/model.cpp:1899-1907 --
// the rule rdamd_model_create_from_file_block applies to the whole alignment -- and this rank keeps
// block `block` of each, compressed on its own.
rdamd_model_t *rdamd_model_create_partitioned_block(const rdamd_tree_t *tree, const char *msa_filename,
                                                    const char *partition_filename, unsigned int states,
                                                    const uint64_t *map, uint64_t seed, int early_stop,
                                                    unsigned int block, unsigned int n_blocks,
                                                    unsigned int *n_partitions, unsigned int *patterns,
                                                    unsigned int *columns) {
  GUARD(nullptr, {
    if (n_blocks < 1 || block >= n_blocks) throw std::invalid_argument("site block index out of range");
    const rdamd::msa_t whole = rdamd::msa_t::from_file(msa_filename, map, states, false);
    std::vector<rdamd::ratehet_opts_t> ratehets;
    const auto infos = read_partition_file(partition_filename, &ratehets);
    const auto full = rdamd::partition_msa(whole, infos, false);
    std::vector<rdamd::msa_t> msas;
    for (size_t p = 0; p < full.size(); ++p) {
      const size_t len = full[p].length();
      if (len < n_blocks)
        throw std::invalid_argument("Partition '" + infos[p].partition_name + "' has " + std::to_string(len) +
                                    " columns, fewer than the " + std::to_string(n_blocks) + " site blocks");
      const auto cols = site_block(len, block, n_blocks);
      msas.push_back(full[p].columns(cols.first, cols.second));
      msas.back().compress();
      if (columns) columns[p] = (unsigned)len;
    }
    return build_model(tree, std::move(msas), ratehets, seed, early_stop, true, n_partitions, patterns);
  })
}
int rdamd_model_partition_lnls(rdamd_model_t *m, const rdamd_root_location_t *rl, double *out) {
  GUARD(RDAMD_FAILURE, {
    const auto v = m->model->partition_lh(to_cpp(rl));
    std::copy(v.begin(), v.end(), out);
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_partition_frequencies(rdamd_model_t *m, unsigned int p, double *out) {
  GUARD(RDAMD_FAILURE, {
    if (p >= m->model->partition_count()) throw std::invalid_argument("partition index out of range");
    rdamd_partition_t *part = m->model->partition(p);
    const double *f = rdamd_partition_frequencies(part, 0);
    std::copy(f, f + rdamd_partition_states(part), out);
    return RDAMD_SUCCESS;
  })
}
unsigned long long rdamd_model_partition_second_passes(const rdamd_model_t *m, unsigned int p) {
  if (p >= m->model->partition_count()) return 0;
  return rdamd_evaluate_second_passes(m->model->partition(p));
}

// ---- site patterns and site log-likelihoods (include/root_digger_amd.h) ----------------
// a model that sums over a site group holds one block of the columns: error 61, not the generic 50
static bool refuse_site_sharded(const rdamd_model_t *m, const char *what) {
  if (!m->model->site_sharded()) return false;
  rdamd::set_error(61, "%s: this model sums over a site group (rdamd_model_set_lnl_reducer) and holds one block of "
                       "the columns; site-sharded models are not supported here", what);
  return true;
}
// weights and column -> pattern map of the partitions' alignments, one behind the other
static void concat_patterns(const std::vector<rdamd::msa_t> &msas, unsigned int *P_total, unsigned int *N_columns,
                            unsigned int *weights, unsigned int *pattern_of) {
  uint64_t patterns = 0, columns = 0;
  for (const auto &msa : msas) {
    const size_t len = msa.length();
    for (size_t s = 0; s < len; ++s) {
      const unsigned w = msa.weights.empty() ? 1u : msa.weights[s];
      if (weights) weights[patterns + s] = w;
      if (!msa.pattern_of.empty()) continue;
      // (never compressed here: pattern s stands for w consecutive columns)
      if (pattern_of)
        for (unsigned k = 0; k < w; ++k) pattern_of[columns + k] = (unsigned)(patterns + s);
      columns += w;
    }
    if (pattern_of)
      for (size_t c = 0; c < msa.pattern_of.size(); ++c) pattern_of[columns + c] = (unsigned)(patterns + msa.pattern_of[c]);
    columns += msa.pattern_of.size();
    patterns += len;
  }
  if ((columns >> 32) || (patterns >> 32)) throw std::overflow_error("2^32 alignment columns or more");
  if (P_total) *P_total = (unsigned)patterns;
  if (N_columns) *N_columns = (unsigned)columns;
}
int rdamd_model_site_patterns(rdamd_model_t *m, unsigned int *P_total, unsigned int *N_columns,
                              unsigned int *weights, unsigned int *pattern_of) {
  GUARD(RDAMD_FAILURE, {
    if (refuse_site_sharded(m, "rdamd_model_site_patterns")) return RDAMD_FAILURE;
    concat_patterns(m->msas, P_total, N_columns, weights, pattern_of);
    return RDAMD_SUCCESS;
  })
}
int rdamd_msa_pattern_probe(const char *msa_filename, const uint64_t *map, unsigned int n_lines,
                            const char *const *lines, unsigned int *n_taxa, unsigned int *P_total,
                            unsigned int *N_columns, unsigned int *weights, unsigned int *pattern_of,
                            char *sequences) {
  GUARD(RDAMD_FAILURE, {
    std::vector<rdamd::msa_t> msas;
    if (n_lines == 0) {
      msas.push_back(rdamd::msa_t::from_file(msa_filename, map, 4, true));
    } else {
      const rdamd::msa_t whole = rdamd::msa_t::from_file(msa_filename, map, 4, false);
      rdamd::msa_partitions_t infos;
      for (unsigned i = 0; i < n_lines; ++i) infos.push_back(rdamd::parse_partition_info(lines[i]));
      msas = rdamd::partition_msa(whole, infos, true);
    }
    unsigned total = 0;
    concat_patterns(msas, &total, N_columns, weights, pattern_of);
    if (P_total) *P_total = total;
    if (n_taxa) *n_taxa = (unsigned)msas[0].count();
    if (sequences) {
      size_t at = 0;
      for (const auto &msa : msas) {
        for (int t = 0; t < msa.count(); ++t)
          std::memcpy(sequences + (size_t)t * total + at, msa.sequences[t].data(), msa.length());
        at += msa.length();
      }
    }
    return RDAMD_SUCCESS;
  })
}
// The prologue of the analyses at a root, and their parameters: n_roots sets in the checkpoint's
// layout (per root counts[n_partitions][4], values) into *sets, which stays empty when none are
// given.  `required`: null if the parameters are optional, else why they are not (the refusal's
// second half); null_argument: one of the caller's other required pointers is null.  false: refused
// (a site-sharded model; the error is set).
using param_set_t = std::vector<rdamd::partition_parameters_t>;
static bool root_params(const rdamd_model_t *m, const char *who, bool null_argument, const char *required,
                        const uint64_t *counts, const double *values, unsigned n_roots, std::vector<param_set_t> *sets) {
  if (refuse_site_sharded(m, who)) return false;
  if (required && (null_argument || !counts || !values))
    throw std::invalid_argument(std::string(who) + ": null argument (the parameters are required: " + required + ")");
  if ((counts == nullptr) != (values == nullptr))
    throw std::invalid_argument(std::string(who) + ": counts and values come together");
  if (null_argument) throw std::invalid_argument(std::string(who) + ": null argument");
  for (unsigned i = 0; counts && i < n_roots; ++i) {
    sets->emplace_back(m->model->partition_count());
    for (rdamd::partition_parameters_t &pp : sets->back())
      for (rdamd::model_params_t *v : {&pp.subst_rates, &pp.freqs, &pp.gamma_alpha, &pp.gamma_weights}) {
        v->assign(values, values + *counts);
        values += *counts++;
      }
  }
  return true;
}
static void copy_nodes(const rdamd::model_t::nodes_t &r, unsigned int *n_nodes, unsigned int *node_clv, int *node_parent,
                       unsigned int *node_children) {
  if (n_nodes) *n_nodes = (unsigned)r.node_clv.size();
  if (node_clv) std::copy(r.node_clv.begin(), r.node_clv.end(), node_clv);
  if (node_parent) std::copy(r.node_parent.begin(), r.node_parent.end(), node_parent);
  if (node_children) std::copy(r.node_children.begin(), r.node_children.end(), node_children);
}

int rdamd_model_site_lnls(rdamd_model_t *m, unsigned int n, const rdamd_root_location_t *rls,
                          const uint64_t *counts, const double *values, double *out_patterns) {
  GUARD(RDAMD_FAILURE, {
    std::vector<param_set_t> params;
    if (!root_params(m, "rdamd_model_site_lnls", n && (!rls || !out_patterns), nullptr, counts, values, n, &params))
      return RDAMD_FAILURE;
    std::vector<root_location_t> roots;
    for (unsigned i = 0; i < n; ++i) roots.push_back(to_cpp(&rls[i]));
    m->model->site_lnls(roots, counts ? &params : nullptr, out_patterns);
    return RDAMD_SUCCESS;
  })
}

int rdamd_model_partition_shape(const rdamd_model_t *m, unsigned int p, unsigned int *patterns,
                                unsigned int *columns, unsigned int *rate_cats) {
  GUARD(RDAMD_FAILURE, {
    if (p >= m->model->partition_count() || p >= m->msas.size()) throw std::invalid_argument("partition index out of range");
    unsigned P = 0, N = 0;
    concat_patterns({m->msas[p]}, &P, &N, nullptr, nullptr);
    if (patterns) *patterns = P;
    if (columns) *columns = N;
    if (rate_cats) *rate_cats = rdamd_partition_rate_cats(m->model->partition(p));
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_ancestral(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts,
                          const double *values, unsigned int *n_nodes, unsigned int *node_clv, int *node_parent,
                          unsigned int *node_children, double *post_out, double *cat_out, double *mean_rate_out) {
  GUARD(RDAMD_FAILURE, {
    std::vector<param_set_t> params;
    if (!root_params(m, "rdamd_model_ancestral", !rl, nullptr, counts, values, 1, &params)) return RDAMD_FAILURE;
    rdamd::model_t::nodes_t nodes;
    m->model->ancestral(to_cpp(rl), counts ? &params[0] : nullptr, &nodes, post_out, cat_out, mean_rate_out);
    copy_nodes(nodes, n_nodes, node_clv, node_parent, node_children);
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_ancestral_sequences(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts,
                                    const double *values, unsigned int *n_nodes, unsigned int *node_clv,
                                    int *node_parent, unsigned int *node_children, uint8_t *state_out,
                                    double *prob_out, double *post_out) {
  GUARD(RDAMD_FAILURE, {
    std::vector<param_set_t> params;
    if (!root_params(m, "rdamd_model_ancestral_sequences", !rl, nullptr, counts, values, 1, &params)) return RDAMD_FAILURE;
    rdamd::model_t::nodes_t nodes;
    m->model->ancestral_sequences(to_cpp(rl), counts ? &params[0] : nullptr, &nodes, state_out, prob_out, post_out);
    copy_nodes(nodes, n_nodes, node_clv, node_parent, node_children);
    return RDAMD_SUCCESS;
  })
}
static void copy_branch_result(const rdamd::model_t::branch_lengths_t &r, double *lengths_out, double *d1_out, double *d2_out) {
  if (lengths_out) std::copy(r.lengths.begin(), r.lengths.end(), lengths_out);
  if (d1_out) std::copy(r.d1.begin(), r.d1.end(), d1_out);
  if (d2_out) std::copy(r.d2.begin(), r.d2.end(), d2_out);
}
int rdamd_model_branch_derivatives(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts,
                                   const double *values, unsigned int *n_nodes, unsigned int *node_clv,
                                   int *node_parent, unsigned int *node_children, double *lengths_out,
                                   double *d1_out, double *d2_out, double *lnl_out) {
  GUARD(RDAMD_FAILURE, {
    std::vector<param_set_t> params;
    if (!root_params(m, "rdamd_model_branch_derivatives", !rl, nullptr, counts, values, 1, &params)) return RDAMD_FAILURE;
    const rdamd::model_t::branch_lengths_t r = m->model->branch_lengths(to_cpp(rl), counts ? &params[0] : nullptr, nullptr);
    copy_nodes(r, n_nodes, node_clv, node_parent, node_children);
    copy_branch_result(r, lengths_out, d1_out, d2_out);
    if (lnl_out) *lnl_out = r.lnl_before;
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_gradient(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts, const double *values,
                         double *grad_out, double *lnl_out) {
  GUARD(RDAMD_FAILURE, {
    std::vector<param_set_t> params;
    if (!root_params(m, "rdamd_model_gradient", !rl || !grad_out,
                     "the gradient is taken in the optimiser's variables, which the model does not keep", counts, values, 1,
                     &params))
      return RDAMD_FAILURE;
    double lnl = 0.0;
    const param_set_t g = m->model->gradient(to_cpp(rl), params[0], &lnl);
    for (const rdamd::partition_parameters_t &pp : g)
      for (const rdamd::model_params_t *v : {&pp.subst_rates, &pp.freqs, &pp.gamma_alpha, &pp.gamma_weights})
        grad_out = std::copy(v->begin(), v->end(), grad_out);
    if (lnl_out) *lnl_out = lnl;
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_substitutions(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts,
                              const double *values, unsigned int *n_nodes, unsigned int *node_clv, int *node_parent,
                              unsigned int *node_children, double *lengths_out, double *typed_out, double *change_out,
                              double *count_out, unsigned char *top_pair_out, double *top_prob_out, double *lnl_out) {
  GUARD(RDAMD_FAILURE, {
    std::vector<param_set_t> params;
    if (!root_params(m, "rdamd_model_substitutions", !rl,
                     "the typed counts are made from the substitution rates, which the model does not keep", counts, values, 1,
                     &params))
      return RDAMD_FAILURE;
    const bool per_site = change_out || count_out || top_pair_out || top_prob_out;
    const rdamd::model_t::substitutions_t r = m->model->substitutions(to_cpp(rl), params[0], per_site);
    copy_nodes(r, n_nodes, node_clv, node_parent, node_children);
    if (lengths_out) std::copy(r.lengths.begin(), r.lengths.end(), lengths_out);
    if (typed_out) std::copy(r.typed.begin(), r.typed.end(), typed_out);
    if (change_out) std::copy(r.change.begin(), r.change.end(), change_out);
    if (count_out) std::copy(r.count.begin(), r.count.end(), count_out);
    if (top_pair_out) std::copy(r.top_pair.begin(), r.top_pair.end(), top_pair_out);
    if (top_prob_out) std::copy(r.top_prob.begin(), r.top_prob.end(), top_prob_out);
    if (lnl_out) *lnl_out = r.lnl;
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_optimize_branch_lengths(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts,
                                        const double *values, double min_len, double max_len, double atol,
                                        unsigned int max_iters, double *lengths_out, double *d1_out, double *d2_out,
                                        double *lnl_before, double *lnl_after, unsigned int *iterations,
                                        unsigned int *evaluations, int *converged) {
  GUARD(RDAMD_FAILURE, {
    std::vector<param_set_t> params;
    if (!root_params(m, "rdamd_model_optimize_branch_lengths", !rl, nullptr, counts, values, 1, &params)) return RDAMD_FAILURE;
    const rdamd::model_t::branch_bounds_t bounds{min_len, max_len, atol, max_iters};
    const rdamd::model_t::branch_lengths_t r = m->model->branch_lengths(to_cpp(rl), counts ? &params[0] : nullptr, &bounds);
    copy_branch_result(r, lengths_out, d1_out, d2_out);
    if (lnl_before) *lnl_before = r.lnl_before;
    if (lnl_after) *lnl_after = r.lnl_after;
    if (iterations) *iterations = r.iterations;
    if (evaluations) *evaluations = r.evaluations;
    if (converged) *converged = r.converged ? 1 : 0;
    return RDAMD_SUCCESS;
  })
}

namespace {
void fill_model(const rdamd::model_info_t &mi, rdamd_partition_info_t *out) {
  std::snprintf(out->subst_str, sizeof out->subst_str, "%s", mi.subst_str.c_str());
  out->freq_type = (int)mi.freq_opts.type;
  out->invar_present = mi.invar_opts.present;
  out->invar_type = (int)mi.invar_opts.type;
  out->invar_user_prop = mi.invar_opts.user_prop;
  out->ratehet = {(int32_t)mi.ratehet_opts.type, (int32_t)mi.ratehet_opts.rate_category_type,
                  mi.ratehet_opts.rate_cats, mi.ratehet_opts.alpha_init ? 1 : 0,
                  mi.ratehet_opts.alpha};
  out->asc_present = mi.asc_opts.present;
  out->asc_type = (int)mi.asc_opts.type;
  out->asc_fels_weight = mi.asc_opts.fels_weight;
  out->n_stam_weights = (unsigned)std::min<size_t>(mi.asc_opts.stam_weights.size(), 32);
  for (unsigned i = 0; i < out->n_stam_weights; ++i) out->stam_weights[i] = mi.asc_opts.stam_weights[i];
}
}  // namespace

int rdamd_parse_model_info(const char *model_string, rdamd_partition_info_t *out) {
  GUARD(RDAMD_FAILURE, {
    std::memset(out, 0, sizeof *out);
    fill_model(rdamd::parse_model_info(model_string), out);
    std::snprintf(out->model_name, sizeof out->model_name, "%s", model_string);
    return RDAMD_SUCCESS;
  })
}
int rdamd_parse_partition_info(const char *line, rdamd_partition_info_t *out) {
  GUARD(RDAMD_FAILURE, {
    std::memset(out, 0, sizeof *out);
    const auto pi = rdamd::parse_partition_info(line);
    fill_model(pi.model, out);
    std::snprintf(out->model_name, sizeof out->model_name, "%s", pi.model_name.c_str());
    std::snprintf(out->partition_name, sizeof out->partition_name, "%s", pi.partition_name.c_str());
    if (pi.parts.size() > 64) throw std::runtime_error("more than 64 ranges in one partition line");
    out->n_ranges = (unsigned)pi.parts.size();
    for (size_t i = 0; i < pi.parts.size(); ++i) {
      out->ranges[i][0] = pi.parts[i].first;
      out->ranges[i][1] = pi.parts[i].second;
    }
    return RDAMD_SUCCESS;
  })
}
// msa_t::partition on a file: lengths (patterns if compress, columns otherwise) and
// total weights of the partitions the given lines describe
int rdamd_msa_partition_probe(const char *msa_filename, const uint64_t *map,
                              unsigned int n_lines, const char *const *lines, int compress,
                              unsigned int *lengths, unsigned int *total_weights) {
  GUARD(RDAMD_FAILURE, {
    const rdamd::msa_t whole = rdamd::msa_t::from_file(msa_filename, map, 4, false);
    rdamd::msa_partitions_t infos;
    for (unsigned i = 0; i < n_lines; ++i) infos.push_back(rdamd::parse_partition_info(lines[i]));
    const auto msas = rdamd::partition_msa(whole, infos, compress != 0);
    for (size_t i = 0; i < msas.size(); ++i) {
      if (lengths) lengths[i] = (unsigned)msas[i].length();
      if (total_weights) total_weights[i] = msas[i].total_weight();
    }
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_partition_count(const rdamd_model_t *m) { return (int)m->msas.size(); }

int rdamd_msa_probe(const char *msa_filename, const uint64_t *map, int compress,
                    unsigned int *n_taxa, unsigned int *n_patterns,
                    unsigned int *total_weight) {
  GUARD(RDAMD_FAILURE, {
    rdamd::msa_t m = rdamd::msa_t::from_file(msa_filename, map, 4, compress != 0);
    if (n_taxa) *n_taxa = (unsigned)m.count();
    if (n_patterns) *n_patterns = (unsigned)m.length();
    if (total_weight) *total_weight = m.total_weight();
    return RDAMD_SUCCESS;
  })
}
void rdamd_model_destroy(rdamd_model_t *m) { delete m; }

int rdamd_model_initialize_partitions(rdamd_model_t *m, int uniform_freqs) {
  GUARD(RDAMD_FAILURE, {
    if (uniform_freqs) m->model->initialize_partitions_uniform_freqs(m->msas);
    else m->model->initialize_partitions(m->msas);
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_set_subst_rates(rdamd_model_t *m, const double *rates) {
  GUARD(RDAMD_FAILURE, {
    unsigned k = m->msas[0].states;
    m->model->set_subst_rates(0, rdamd::model_params_t(rates, rates + k * k - k));
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_set_subst_rates_uniform(rdamd_model_t *m) {
  GUARD(RDAMD_FAILURE, { m->model->set_subst_rates_uniform(); return RDAMD_SUCCESS; })
}
int rdamd_model_set_freqs(rdamd_model_t *m, const double *freqs) {
  GUARD(RDAMD_FAILURE, {
    m->model->set_freqs(0, rdamd::model_params_t(freqs, freqs + m->msas[0].states));
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_set_empirical_freqs(rdamd_model_t *m) {
  GUARD(RDAMD_FAILURE, { m->model->set_empirical_freqs(); return RDAMD_SUCCESS; })
}
int rdamd_model_set_gamma_alpha(rdamd_model_t *m, double alpha) {
  GUARD(RDAMD_FAILURE, { m->model->set_gamma_rates(0, {alpha}); return RDAMD_SUCCESS; })
}
double rdamd_model_compute_lh(rdamd_model_t *m, const rdamd_root_location_t *rl) {
  GUARD(std::nan(""), { return m->model->compute_lh(to_cpp(rl)); })
}
double rdamd_model_compute_lh_root(rdamd_model_t *m, const rdamd_root_location_t *rl) {
  GUARD(std::nan(""), { return m->model->compute_lh_root(to_cpp(rl)); })
}
int rdamd_model_compute_dlh(rdamd_model_t *m, const rdamd_root_location_t *rl, double out[2]) {
  GUARD(RDAMD_FAILURE, {
    auto d = m->model->compute_dlh(to_cpp(rl));
    out[0] = d.lh; out[1] = d.dlh;
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_move_root(rdamd_model_t *m, const rdamd_root_location_t *rl) {
  GUARD(RDAMD_FAILURE, { m->model->move_root(to_cpp(rl)); return RDAMD_SUCCESS; })
}
int rdamd_model_compute_all_root_lh(rdamd_model_t *m, double *out) {
  GUARD(RDAMD_FAILURE, {
    auto v = m->model->compute_all_root_lh();
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_compute_all_root_lh_batched(rdamd_model_t *m, double *out) {
  GUARD(RDAMD_FAILURE, {
    auto v = m->model->compute_all_root_lh_batched();
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_compute_all_root_lh_directional(rdamd_model_t *m, const double *ratios, double *out) {
  GUARD(RDAMD_FAILURE, {
    std::vector<double> r;
    if (ratios) r.assign(ratios, ratios + m->model->tree().root_count());
    const auto v = m->model->compute_all_root_lh_directional(ratios ? &r : nullptr);
    std::copy(v.begin(), v.end(), out);
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_search(rdamd_model_t *m, unsigned int min_roots, double root_ratio, double atol,
                       double pgtol, double brtol, double factor,
                       rdamd_root_location_t *best_rl, double *best_llh) {
  GUARD(RDAMD_FAILURE, {
    auto best = m->model->search(min_roots, root_ratio, atol, pgtol, brtol, factor, nullptr);
    if (best_rl) to_c(best.first, best_rl);
    if (best_llh) *best_llh = best.second;
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_optimize_alpha(rdamd_model_t *m, const rdamd_root_location_t *rl, double atol,
                               rdamd_root_location_t *out) {
  GUARD(RDAMD_FAILURE, { to_c(m->model->optimize_alpha(to_cpp(rl), atol), out); return RDAMD_SUCCESS; })
}
int rdamd_model_compute_lh_batch(rdamd_model_t *m, unsigned int n,
                                 const rdamd_root_location_t *rls, const double *subst,
                                 const double *freqs, const double *gamma_alpha, double *out) {
  GUARD(RDAMD_FAILURE, {
    const unsigned k = m->msas[0].states, np = k * k - k;
    std::vector<root_location_t> roots;
    std::vector<std::vector<rdamd::partition_parameters_t>> params(n);
    for (unsigned j = 0; j < n; ++j) {
      roots.push_back(to_cpp(&rls[j]));
      rdamd::partition_parameters_t pp;
      pp.subst_rates.assign(subst + (size_t)j * np, subst + (size_t)(j + 1) * np);
      pp.freqs.assign(freqs + (size_t)j * k, freqs + (size_t)(j + 1) * k);
      pp.gamma_alpha.assign(1, gamma_alpha ? gamma_alpha[j] : 1.0);
      params[j].push_back(pp);
    }
    auto v = m->model->compute_lh_batch(roots, params);
    for (unsigned j = 0; j < n; ++j) out[j] = v[j];
    return RDAMD_SUCCESS;
  })
}
void rdamd_model_set_lbfgsb(rdamd_model_t *m, void *fn) {
  m->setulb = fn;
  m->model->set_lbfgsb(reinterpret_cast<rdamd::model_t::setulb_fn>(fn));
}

// The candidate-root loop of exhaustive_search (src/model.cpp:1154) is
// embarrassingly parallel: the reference runs it on one MPI rank per chunk
// (src/model.cpp:1867-1911).  On one GPU the same thing is `workers` host
// threads, each with its own model replica (own partition, own HIP stream),
// pulling candidates from a shared counter -- their small launches (13-job
// L-BFGS-B batches, root-only Brent steps) overlap on the device.
// replicas keep only what the root-only steps read when the searches' compute_lh is the
// children-only one (rdamd_model_set_root_children_only, the default)
static bool replicas_are_sparse(const rdamd_model_t *m) { return m->children_only; }

unsigned int rdamd_model_max_replicas(const rdamd_model_t *m, unsigned int requested,
                                      uint64_t *replica_bytes) {
  const unsigned tips = m->model->tree().tip_count(), branches = m->model->tree().branch_count();
  uint64_t per_replica = 0;
  const auto &ratehets = m->ratehets;
  const auto &msas = m->msas;
  for (size_t i = 0; i < msas.size(); ++i) {
    // a replica's 4-state / binary partitions hold the root's two children and the root CLV, not
    // all 2n - 3 buffers (RDAMD_ATTRIB_SPARSE_CLVS; their pools start at four slots) -- plus the
    // evaluator's workspace for the one job that writes them
    const unsigned R = (unsigned)ratehets[i].rate_cats;
    const bool sparse = replicas_are_sparse(m) && rdamd::fused_capable(msas[i].states, R);
    per_replica += rdamd_partition_footprint(tips, sparse ? 4u : branches, msas[i].states, (unsigned)msas[i].length(),
                                             branches, R, sparse ? 4u : branches);
    if (sparse) {
      const uint64_t K = msas[i].states == 20 ? 20 : 4;
      per_replica += (uint64_t)branches * R * (K * K + (K == 4 ? 64 : 64 * 24)) * 8 * 2 +
                     (uint64_t)msas[i].length() * R * 8 + ((uint64_t)2 << 20);
    }
  }
  if (replica_bytes) *replica_bytes = per_replica;
  uint64_t free_b = 0, total_b = 0;
  if (rdamd_device_memory(&free_b, &total_b) != RDAMD_SUCCESS || per_replica == 0) return requested ? requested : 1;
  const uint64_t fit = (uint64_t)(0.85 * (double)free_b) / per_replica;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(requested, fit));
}

// The shared objective partition(s) on LOW stream priority for the duration of a lock-stepped
// search: their launches fill every CU for a millisecond, and the kernels beside them (front
// halves of the other group's batch, the replicas' root-only steps and traversals) get the wave
// slots that become free instead of waiting for the launch to end.  Normal priority again when
// the search is over, however it ends (the stream is re-created: rdamd_partition_stream handles
// taken before are invalid, as the header says).
struct shared_priority_t {
  rdamd_model_t *m;
  bool active;
  shared_priority_t(rdamd_model_t *m_, bool lockstep) : m(m_), active(lockstep && m_->lockstep_priority != 0) {
    for (size_t pi = 0; active && pi < m->model->partition_count(); ++pi)
      if (rdamd_partition_set_stream_priority(m->model->partition(pi), m->lockstep_priority) != RDAMD_SUCCESS) {
        // (a constructor that throws has no destructor: put back what was switched so far)
        const std::string why = rdamd_errmsg();
        for (size_t pj = 0; pj < pi; ++pj) (void)rdamd_partition_set_stream_priority(m->model->partition(pj), 0);
        throw std::runtime_error("set_stream_priority: " + why);
      }
  }
  ~shared_priority_t() {
    for (size_t pi = 0; active && pi < m->model->partition_count(); ++pi)
      (void)rdamd_partition_set_stream_priority(m->model->partition(pi), 0);
  }
};

// How many replicas fit is each rank's own finding (its free device memory), and every rank of a
// site group that searches in rounds must run the SAME number of candidates in flight: a different
// count on one rank means other rounds, other vector lengths, collectives that do not match.  So the
// group agrees before it starts -- through the reducer, like everything else:
// [1, requested, requested^2, fit, fit^2] summed; all ranks equal <=> sum == G x own for the value
// AND its square (then sum (x_i - own)^2 = 0), which every rank decides alike.
static unsigned agree_on_replicas(rdamd_model_t *m, unsigned requested, unsigned fit, uint64_t bytes) {
  double v[5] = {1.0, (double)requested, (double)requested * requested, (double)fit, (double)fit * fit};
  m->model->sum_over_site_group(v, 5);
  const double G = v[0];
  if (v[1] != G * requested || v[2] != G * requested * requested)
    throw std::runtime_error("lock step in rounds: the ranks of the site group were asked for different numbers of "
                             "candidates in flight (this rank: " + std::to_string(requested) + ")");
  if (v[3] == G * fit && v[4] == G * (double)fit * fit) return fit;
  // they differ: everybody runs the smallest.  u[i] = 1 while i < fit; the sum is G exactly
  // where every rank still fits
  std::vector<double> u(requested, 0.0);
  for (unsigned i = 0; i < fit && i < requested; ++i) u[i] = 1.0;
  m->model->sum_over_site_group(u.data(), u.size());
  unsigned least = 0;
  while (least < requested && u[least] == G) ++least;
  std::fprintf(stderr, "rdamd: the ranks of the site group fit different numbers of replicas (this rank: %u of %.2f GB "
                       "each); all of them run %u candidates in flight\n", fit, (double)bytes / 1e9, std::max(least, 1u));
  return std::max(least, 1u);
}

// where the candidates in flight of a search with replicas meet (lockstep.hpp)
enum class meeting_t {
  none,      // nowhere: every replica launches on its own
  arrival,   // in arrival order (batch_combiner.hpp), on this model's partitions
  rounds,    // in deterministic rounds (lockstep_conductor.hpp): what a site-sharded model's search is --
             // every rank of the site group runs this with the same candidates and forms the same
             // rounds, one collective each
};

// Worker w is a host thread with a model replica (sparse: the root's children only).  In lock step
// the replicas' objective batches meet on THIS model's partitions, one objective partition per model
// partition; it does nothing else meanwhile.
static int search_with_replicas(rdamd_model_t *m, meeting_t meet, unsigned int workers, double atol,
                                double pgtol, double brtol, double factor, uint64_t *root_id,
                                double *llh, double *alpha, unsigned int *n_results,
                                rdamd_root_location_t *best_rl, double *best_llh) {
  GUARD(RDAMD_FAILURE, {
    const bool rounds = meet == meeting_t::rounds, lockstep = meet != meeting_t::none;
    const bool sharded = m->model->site_sharded();
    if (sharded && !rounds)
      throw std::runtime_error("the candidates of a site-sharded model advance in rounds "
                               "(rdamd_model_exhaustive_search_lockstep); free-running replicas would "
                               "reorder the site group's collectives");
    const std::vector<size_t> todo = m->model->assigned_indicies();
    if (workers < 1) workers = 1;
    workers = (unsigned)std::min<size_t>(workers, std::max<size_t>(todo.size(), 1));
    {   // every replica is a model of its own: keep them inside the device memory
      uint64_t bytes = 0;
      unsigned fit = rdamd_model_max_replicas(m, workers, &bytes);
      if (rounds && sharded) fit = agree_on_replicas(m, workers, fit, bytes);
      if (fit < workers) {
        std::fprintf(stderr, "rdamd: %u replicas of %.2f GB each do not fit the free device memory; running %u\n",
                     workers, (double)bytes / 1e9, fit);
        workers = fit;
      }
    }
    // One worker group or two alternating ones (rdamd_model_set_lockstep_groups)?  Two hide the
    // hosts' steps behind the other group's launch (in arrival order their batches alternate in the
    // shared partition's pipeline, batch_combiner.hpp); one makes every launch twice as large and,
    // in rounds, HALVES the collectives.  Measured on one GPU (profiles/r5_shard_search.txt): an
    // unsharded c2 gains from two; c2 / 8's shard is faster with one (0.201 against 0.218 s per
    // candidate, 244 against 397 collectives per candidate), the deep shards are evaluator-bound
    // either way -- and on real links every round pays the collective's latency.  So rounds default
    // to ONE group for a site-sharded model and to two for an unsharded one; arrival order takes two
    // from four candidates in flight on unless asked for one.
    unsigned n_groups = 1;
    if (rounds) {
      const unsigned want_groups = m->lockstep_groups ? m->lockstep_groups : (sharded ? 1u : 2u);
      n_groups = workers >= 4 && want_groups >= 2 ? 2u : 1u;
    } else if (lockstep) {
      n_groups = workers >= 4 && m->lockstep_groups != 1 ? 2u : 1u;
    }
    shared_priority_t shared_priority(m, lockstep);
    std::vector<rdamd_partition_t *> parts;
    for (size_t pi = 0; pi < m->model->partition_count(); ++pi) parts.push_back(m->model->partition(pi));
    std::unique_ptr<rdamd::conductor_t> conductor;
    std::unique_ptr<rdamd::arrival_lockstep_t> arrival;
    rdamd::lockstep_t *ls = nullptr;
    if (rounds) {
      rdamd::conductor_t::config_t cfg;
      cfg.parts = parts;
      cfg.stream_wait_event = hipStreamWaitEvent;
      cfg.n_workers = workers;
      cfg.n_groups = n_groups;
      cfg.n_candidates = todo.size();
      const auto red = m->model->reducer();
      cfg.reduce = red.reduce; cfg.device = red.device; cfg.queue = red.queue; cfg.wait = red.wait;
      cfg.user = red.user; cfg.async_user = red.async_user;
      cfg.abort = red.abort; cfg.abort_user = red.abort_user;
      conductor.reset(new rdamd::conductor_t(cfg));
      ls = conductor.get();
    } else {   // (without a meeting point the replicas still take their candidates from its counter)
      arrival.reset(new rdamd::arrival_lockstep_t(parts, n_groups, todo.size()));
      ls = arrival.get();
    }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) throw std::runtime_error("no HIP device");
    std::mutex mu;
    std::vector<rdamd::rd_result_t> results;
    std::string first_error;
    auto work = [&](unsigned wid) {
      try {
        if (hipSetDevice(device) != hipSuccess) throw std::runtime_error("hipSetDevice failed");
        const bool sparse = replicas_are_sparse(m);
        rdamd::model_t replica(m->model->tree(), m->msas, m->ratehets, false, m->seed + wid, m->early_stop, sparse);
        // (no collective of its own: the group's frequencies come from the parent, every other
        // sum goes through the rounds)
        replica.adopt_empirical_freqs(*m->model);
        replica.initialize_partitions(m->msas);
        if (m->setulb) replica.set_lbfgsb(reinterpret_cast<rdamd::model_t::setulb_fn>(m->setulb));
        replica.set_checkpoint(m->checkpoint);
        replica.set_progress(m->progress.get());
        replica.set_root_children_only(m->children_only);
        if (lockstep && m->lockstep_priority)   // (the replicas' short kernels in front of the shared partition's long ones)
          for (size_t pi = 0; pi < replica.partition_count(); ++pi)
            if (rdamd_partition_set_stream_priority(replica.partition(pi), -1) != RDAMD_SUCCESS)
              throw std::runtime_error(std::string("set_stream_priority: ") + rdamd_errmsg());
        // (model_t::initialize is a full traversal whose CLVs the search never reads: a sparse
        // replica, whose first step writes the two it needs, does without.  It evaluates on the
        // replica's own partitions and never reaches the objective: the replica meets the others after it)
        if (!sparse) replica.initialize();
        if (lockstep) replica.set_lockstep(ls, wid);
        for (;;) {
          const long k = ls->next_candidate(wid);
          if (k < 0) break;
          replica.assign_indicies(std::vector<size_t>{todo[(size_t)k]});
          std::vector<rdamd::rd_result_t> r;
          replica.exhaustive_search(atol, pgtol, brtol, factor, &r);
          std::lock_guard<std::mutex> g(mu);
          results.insert(results.end(), r.begin(), r.end());
        }
      } catch (const std::exception &e) {
        ls->fail(e.what());   // (nobody waits for this worker, nobody starts another candidate)
        std::lock_guard<std::mutex> g(mu);
        if (first_error.empty()) first_error = e.what();
      }
    };
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < workers; ++w) pool.emplace_back(work, w);
    for (auto &t : pool) t.join();
    if (conductor) {
      const auto st = conductor->stats();
      m->lockstep_stats[0] = st.obj_launches; m->lockstep_stats[1] = st.obj_jobs;
      m->lockstep_stats[2] = st.root_launches; m->lockstep_stats[3] = st.root_steps;
      m->round_stats[0] = st.rounds; m->round_stats[1] = st.collectives; m->round_stats[2] = st.redos;
      for (int k = 0; k < 4; ++k) m->round_seconds[k] = st.seconds[k];
      m->round_part_stats.assign(2 * m->model->partition_count(), 0);
      for (size_t p = 0; p < st.part_launches.size() && p < m->model->partition_count(); ++p) {
        m->round_part_stats[2 * p] = st.part_launches[p];
        m->round_part_stats[2 * p + 1] = st.part_redo_launches[p];
      }
    } else if (lockstep) {
      arrival->stats(m->lockstep_stats);
    }
    if (!first_error.empty()) throw std::runtime_error(first_error);
    std::sort(results.begin(), results.end(),
              [](const rdamd::rd_result_t &a, const rdamd::rd_result_t &b) { return a.root_id < b.root_id; });
    double bl = -INFINITY;
    for (size_t i = 0; i < results.size(); ++i) {
      root_id[i] = results[i].root_id; llh[i] = results[i].llh; alpha[i] = results[i].alpha;
      if (results[i].llh > bl) {
        bl = results[i].llh;
        if (best_rl) {
          auto rl = m->model->tree().root_location(results[i].root_id);
          rl.brlen_ratio = results[i].alpha;
          to_c(rl, best_rl);
        }
      }
    }
    *n_results = (unsigned)results.size();
    if (best_llh) *best_llh = bl;
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_exhaustive_search_parallel(rdamd_model_t *m, unsigned int workers, double atol,
                                           double pgtol, double brtol, double factor,
                                           uint64_t *root_id, double *llh, double *alpha,
                                           unsigned int *n_results,
                                           rdamd_root_location_t *best_rl, double *best_llh) {
  return search_with_replicas(m, meeting_t::none, workers, atol, pgtol, brtol, factor, root_id, llh, alpha,
                              n_results, best_rl, best_llh);
}
int rdamd_model_exhaustive_search_lockstep(rdamd_model_t *m, unsigned int in_flight, double atol,
                                           double pgtol, double brtol, double factor,
                                           uint64_t *root_id, double *llh, double *alpha,
                                           unsigned int *n_results,
                                           rdamd_root_location_t *best_rl, double *best_llh) {
  // a site-sharded model's candidates meet in deterministic rounds (the ranks of its site group
  // must form the same launches and collectives); others in arrival order, unless asked
  const bool rounds = m->lockstep_rounds < 0 ? m->model->site_sharded() : m->lockstep_rounds != 0;
  return search_with_replicas(m, rounds ? meeting_t::rounds : meeting_t::arrival, in_flight, atol, pgtol, brtol,
                              factor, root_id, llh, alpha, n_results, best_rl, best_llh);
}
int rdamd_model_optimize_params(rdamd_model_t *m, const rdamd_root_location_t *rl, double pgtol,
                                double factor, int optimize_gamma, double *subst, double *freqs,
                                double *gamma_alpha, uint64_t *n_batches,
                                uint64_t *n_evaluations) {
  GUARD(RDAMD_FAILURE, {
    const unsigned k = m->msas[0].states;
    std::vector<rdamd::partition_parameters_t> params(1);
    params[0].subst_rates.assign(subst, subst + k * k - k);
    params[0].freqs.assign(freqs, freqs + k);
    params[0].gamma_alpha.assign(1, *gamma_alpha);
    const size_t b0 = m->model->objective_batches(), e0 = m->model->objective_evaluations();
    m->model->optimize_params(params, to_cpp(rl), pgtol, factor, optimize_gamma != 0);
    std::copy(params[0].subst_rates.begin(), params[0].subst_rates.end(), subst);
    std::copy(params[0].freqs.begin(), params[0].freqs.end(), freqs);
    *gamma_alpha = params[0].gamma_alpha[0];
    if (n_batches) *n_batches = m->model->objective_batches() - b0;
    if (n_evaluations) *n_evaluations = m->model->objective_evaluations() - e0;
    return RDAMD_SUCCESS;
  })
}
void rdamd_model_set_lockstep_groups(rdamd_model_t *m, unsigned int groups) { m->lockstep_groups = groups; }
void rdamd_model_set_lockstep_priority(rdamd_model_t *m, int level) { m->lockstep_priority = level; }
void rdamd_model_set_root_children_only(rdamd_model_t *m, int on) {
  m->children_only = on != 0;
  if (m->model) m->model->set_root_children_only(on != 0);
}
void rdamd_model_lockstep_stats(const rdamd_model_t *m, uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = m->lockstep_stats[i];
}
void rdamd_model_set_lockstep_rounds(rdamd_model_t *m, int mode) { m->lockstep_rounds = mode; }
void rdamd_model_round_seconds(const rdamd_model_t *m, double out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = m->round_seconds[i];
}
void rdamd_model_round_stats(const rdamd_model_t *m, uint64_t out[4]) {
  for (int i = 0; i < 3; ++i) out[i] = m->round_stats[i];
  out[3] = m->model->collectives();
}
int rdamd_model_round_partition_stats(const rdamd_model_t *m, unsigned int p, uint64_t out[2]) {
  out[0] = out[1] = 0;
  if (p >= m->model->partition_count()) return RDAMD_FAILURE;
  if (2 * p + 1 < m->round_part_stats.size()) {
    out[0] = m->round_part_stats[2 * p];
    out[1] = m->round_part_stats[2 * p + 1];
  }
  return RDAMD_SUCCESS;
}
void rdamd_model_counters(const rdamd_model_t *m, uint64_t out[6]) {
  const auto c = m->model->counters();
  for (int i = 0; i < 6; ++i) out[i] = c[i];
}

int rdamd_model_set_progress(rdamd_model_t *m, int on) {
  if (on) {
    m->progress.reset(new rdamd::model_t::progress_t());
    m->progress->total = m->model->assigned_indicies().size();
  } else {
    m->progress.reset();
  }
  m->model->set_progress(m->progress.get());
  return RDAMD_SUCCESS;
}
int rdamd_model_set_checkpoint(rdamd_model_t *m, rdamd_checkpoint_t *c) {
  m->checkpoint = rdamd_checkpoint_cpp(c);
  m->model->set_checkpoint(m->checkpoint);
  return RDAMD_SUCCESS;
}
int rdamd_model_assign_by_rank_checkpoint(rdamd_model_t *m, unsigned int rank,
                                          unsigned int num_tasks, rdamd_checkpoint_t *c) {
  GUARD(RDAMD_FAILURE, {
    std::vector<size_t> done;
    if (c) done = rdamd_checkpoint_cpp(c)->completed_indicies();
    m->model->assign_indicies_by_rank_exhaustive(rank, num_tasks, done);
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_assign_by_rank_search(rdamd_model_t *m, unsigned int min_roots, double root_ratio,
                                      unsigned int rank, unsigned int num_tasks,
                                      int initial_root_strategy, rdamd_checkpoint_t *c) {
  GUARD(RDAMD_FAILURE, {
    if (initial_root_strategy < 0 || initial_root_strategy > 2)
      throw std::runtime_error("The initial root strategy was not recognized");
    std::vector<size_t> done;
    if (c) done = rdamd_checkpoint_cpp(c)->completed_indicies();
    m->model->assign_indicies_by_rank_search(
        min_roots, root_ratio, rank, num_tasks,
        (rdamd::model_t::initial_root_strategy)initial_root_strategy, done);
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_assigned(const rdamd_model_t *m, uint64_t *root_ids, unsigned int cap) {
  const auto &idx = m->model->assigned_indicies();
  for (size_t i = 0; i < idx.size() && i < cap; ++i) root_ids[i] = idx[i];
  return (int)idx.size();
}
int rdamd_model_assign_by_rank(rdamd_model_t *m, unsigned int rank, unsigned int num_tasks) {
  GUARD(RDAMD_FAILURE, {
    m->model->assign_indicies_by_rank_exhaustive(rank, num_tasks);
    return RDAMD_SUCCESS;
  })
}
int rdamd_model_exhaustive_search(rdamd_model_t *m, double atol, double pgtol, double brtol,
                                  double factor, uint64_t *root_id, double *llh, double *alpha,
                                  unsigned int *n_results, rdamd_root_location_t *best_rl,
                                  double *best_llh) {
  GUARD(RDAMD_FAILURE, {
    std::vector<rdamd::rd_result_t> res;
    auto best = m->model->exhaustive_search(atol, pgtol, brtol, factor, &res);
    for (size_t i = 0; i < res.size(); ++i) {
      root_id[i] = res[i].root_id; llh[i] = res[i].llh; alpha[i] = res[i].alpha;
    }
    *n_results = (unsigned)res.size();
    if (best_rl) to_c(best.first, best_rl);
    if (best_llh) *best_llh = best.second;
    return RDAMD_SUCCESS;
  })
}

}  // extern "C"
