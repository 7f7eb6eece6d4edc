/*
 * root_digger_amd.h -- C ABI of the MI355X (gfx950) likelihood core for
 * RootDigger's root search.
 *
 * This is the drop-in boundary: plain C, plain pointers and sizes, no torch or
 * HIP types.  Every entry point names the reference interface it replaces.
 * The reference reaches its likelihood library (coraxlib, a C library) from
 * src/model.cpp and src/tree.cpp; citations below are relative to
 * /root/reference/.  A maintainer swaps `corax_` for `rdamd_` at the call
 * sites listed.
 *
 * All CLV / P-matrix / scaler storage lives in HBM; host pointers passed in
 * are borrowed for the duration of the call only.  Functions are NOT
 * re-entrant on the same partition (one HIP stream per partition); different
 * partitions may be driven from different host threads, as the reference does
 * (src/model.cpp:397, :429, :1935).
 */
#ifndef ROOT_DIGGER_AMD_H_
#define ROOT_DIGGER_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDAMD_SUCCESS 1 /* CORAX_SUCCESS */
#define RDAMD_FAILURE 0 /* CORAX_FAILURE */
#define RDAMD_SCALE_BUFFER_NONE (-1)

/* attribute bits accepted for source compatibility with src/model.cpp:145-157;
 * the SIMD ones are meaningless on a GPU and ignored. */
#define RDAMD_ATTRIB_ARCH_SSE (1u << 0)
#define RDAMD_ATTRIB_ARCH_AVX (1u << 1)
#define RDAMD_ATTRIB_ARCH_AVX2 (1u << 2)
#define RDAMD_ATTRIB_SITE_REPEATS (1u << 10)
#define RDAMD_ATTRIB_NONREV (1u << 11)
/* New here (coraxlib has no such thing): the partition's CLV and scale buffers get device memory
 * when a call first names them instead of at creation, and rdamd_partition_discard_clvs() returns
 * it all.  Indices, results and every other call are unchanged.  For partitions of which only a
 * few buffers are ever live -- the model replicas of a lock-stepped search keep the root's two
 * children and nothing else (rdamd_evaluate_root_children): megabytes instead of the
 * clv_buffers x sites x rates x states x 8 bytes of a dense partition. */
#define RDAMD_ATTRIB_SPARSE_CLVS (1u << 20)

#define RDAMD_GAMMA_RATES_MEAN 0   /* CORAX_GAMMA_RATES_MEAN   */
#define RDAMD_GAMMA_RATES_MEDIAN 1 /* CORAX_GAMMA_RATES_MEDIAN */

/* error channel: replaces the corax_errno / corax_errmsg globals read at
 * src/model.cpp:439, :849 and src/msa.cpp:628-629 (thread-local here). */
int         rdamd_errno(void);
const char *rdamd_errmsg(void);

/* replaces corax_operation_t (filled at src/tree.cpp:399-410, :425-436,
 * :636-647; golden indices in test/src/tree.cpp:154-179). */
typedef struct rdamd_operation {
  unsigned int parent_clv_index;
  int          parent_scaler_index;
  unsigned int child1_clv_index;
  unsigned int child1_matrix_index;
  int          child1_scaler_index;
  unsigned int child2_clv_index;
  unsigned int child2_matrix_index;
  int          child2_scaler_index;
} rdamd_operation_t;

typedef struct rdamd_partition rdamd_partition_t;

/* ------------------------------------------------------------------------
 * Partition life cycle and setters
 * --------------------------------------------------------------------- */

/* replaces corax_partition_create, src/model.cpp:159-168.  Returns NULL and
 * sets rdamd_errmsg on failure (no GPU, out of memory, bad sizes).
 * states == 2 (binary characters, `rd --states 2`, src/main.cpp:484-488) runs
 * on the 4-state kernels with two inert states; every array that crosses this
 * boundary keeps its 2-state shape (2 substitution rates, 2 frequencies,
 * [S][R][2] CLVs, [R][2][2] P-matrices), including rdamd_evaluate_batch. */
rdamd_partition_t *rdamd_partition_create(unsigned int tips,
                                          unsigned int clv_buffers,
                                          unsigned int states,
                                          unsigned int sites,
                                          unsigned int rate_matrices,
                                          unsigned int prob_matrices,
                                          unsigned int rate_cats,
                                          unsigned int scale_buffers,
                                          unsigned int attributes);
/* replaces corax_partition_destroy, src/model.cpp:180 */
void rdamd_partition_destroy(rdamd_partition_t *p);
/* RDAMD_ATTRIB_SPARSE_CLVS partitions: every CLV and scale buffer becomes undefined (scalers read
 * as 0 again) and its device memory is free for the buffers named next.  Queued work of the
 * partition is not disturbed.  A no-op on dense partitions (their buffers keep their contents). */
void rdamd_partition_discard_clvs(rdamd_partition_t *p);
/* device bytes the CLV and scale buffers of the partition hold right now */
uint64_t rdamd_partition_clv_bytes(const rdamd_partition_t *p);

/* replaces corax_set_tip_states, src/model.cpp:310.  `map` is a 256-entry
 * char -> state-bitmask table (rdamd_map_nt / rdamd_map_bin or the caller's).
 * Returns RDAMD_FAILURE on a character the map does not know (error 4; also a mask with bits
 * beyond the partition's states).  A partition that is not 4-state (or binary) numbers the distinct
 * masks it is given and holds at most 64 of them, over all its tips and for its whole life: the
 * sequence that would bring a 65th is refused (error 5).  A refused call (errors 3, 4, 5) leaves the
 * partition as it was: the tip keeps its sequence, the table its masks, on the host and on the
 * device, and schedules compiled before stay valid.  (A HIP error while the accepted sequence is
 * copied to the device leaves the host's copy as it was; the device is then in doubt.) */
int rdamd_set_tip_states(rdamd_partition_t *p, unsigned int tip_index,
                         const uint64_t *map, const char *sequence);
/* replaces corax_set_pattern_weights, src/model.cpp:324 */
void rdamd_set_pattern_weights(rdamd_partition_t *p, const unsigned int *w);
/* replaces corax_set_subst_params, src/model.cpp:185 (K*K-K values) */
void rdamd_set_subst_params(rdamd_partition_t *p, unsigned int params_index,
                            const double *params);
/* replaces corax_set_frequencies, src/model.cpp:337, :347 */
void rdamd_set_frequencies(rdamd_partition_t *p, unsigned int params_index,
                           const double *freqs);
/* replaces corax_set_category_rates, src/model.cpp:244-289 */
void rdamd_set_category_rates(rdamd_partition_t *p, const double *rates);
/* replaces corax_set_category_weights, src/model.cpp:205, :209 */
void rdamd_set_category_weights(rdamd_partition_t *p, const double *weights);
/* replaces corax_update_invariant_sites_proportion, src/model.cpp:297.  The
 * reference only ever passes 0.0; any other value is rejected. */
int rdamd_update_invariant_sites_proportion(rdamd_partition_t *p,
                                            unsigned int       params_index,
                                            double             prop_invar);
/* replaces corax_msa_empirical_frequencies, src/model.cpp:329; malloc'd
 * double[states], caller frees (src/model.cpp:338). */
double *rdamd_msa_empirical_frequencies(rdamd_partition_t *p);
/* replaces corax_compute_gamma_cats, src/model.cpp:239-270 */
int rdamd_compute_gamma_cats(double alpha, unsigned int categories,
                             double *output_rates, int rates_mode);

/* struct reads the reference performs directly on corax_partition_t
 * (src/model.cpp:330, :1043-1045, :1315): exposed as accessors. */
unsigned int  rdamd_partition_states(const rdamd_partition_t *p);
unsigned int  rdamd_partition_rate_cats(const rdamd_partition_t *p);
unsigned int  rdamd_partition_sites(const rdamd_partition_t *p);
unsigned int  rdamd_partition_tips(const rdamd_partition_t *p);
/* sum of the pattern weights (= alignment columns the partition stands for) */
double        rdamd_partition_weight_sum(const rdamd_partition_t *p);
/* the HIP stream handle (opaque here; HIP's stream type) every launch of this partition is queued on:
 * a collective queued on it runs after the batch that produced its input */
void         *rdamd_partition_stream(const rdamd_partition_t *p);
/* Dispatch priority of the partition's stream: -1 high, 0 normal (default), +1 low.  When
 * several partitions' kernels compete for the device, workgroups of a higher-priority stream
 * take the wave slots that become free first.  The lock-stepped search puts the shared
 * objective partition -- long launches that fill every CU -- on LOW priority, so that the
 * short kernels beside it (the other group's P-matrices and clade tables, the candidates'
 * root-only steps) start when a slot frees up instead of when the launch ends.  The stream is
 * re-created: call it while nothing is queued on the partition (it waits for that).  A handle
 * rdamd_partition_stream() returned before the call is INVALID afterwards: ask again. */
int           rdamd_partition_set_stream_priority(rdamd_partition_t *p, int level);
const double *rdamd_partition_subst_params(const rdamd_partition_t *p,
                                           unsigned int params_index);
const double *rdamd_partition_frequencies(const rdamd_partition_t *p,
                                          unsigned int params_index);

/* ------------------------------------------------------------------------
 * The hot path
 * --------------------------------------------------------------------- */

/* params_indices / freqs_indices, here and in every call below that takes one: `rate_cats` entries;
 * entry r names the rate matrix (params_indices) or the frequency set (freqs_indices) of rate
 * category r, one of the partition's `rate_matrices` sets as rdamd_set_subst_params /
 * rdamd_set_frequencies filled them.  An entry >= rate_matrices is refused (error 7).  The two are
 * independent: the frequency indices of a root call need not be the indices the P-matrices were
 * built with.  rdamd_root_loglikelihood_fused and rdamd_root_loglikelihood_fused_multi take ONE
 * vector and read both through it.  model_t (rdamd_model_*) and rd_amd create partitions with one
 * rate matrix and always pass index 0, as the reference does; rdamd_evaluate_batch carries one
 * parameter set per job and reads neither.
 *
 * replaces corax_update_prob_matrices, src/model.cpp:367, :432, :842.
 * P[m][r] = exp(Q * rate_r * t_m) computed on the device for the whole list in
 * one launch. */
int rdamd_update_prob_matrices(rdamd_partition_t  *p,
                               const unsigned int *params_indices,
                               const unsigned int *matrix_indices,
                               const double       *branch_lengths,
                               unsigned int        count);
/* replaces corax_update_clvs, src/model.cpp:402, :440, :461, :851.  `ops` must
 * be in dependency (post-) order, as corax_utree_create_operations emits. */
void rdamd_update_clvs(rdamd_partition_t *p, const rdamd_operation_t *ops,
                       unsigned int count);
/* Diagnostic: kernel launches the partition's last rdamd_update_clvs call took.  A full traversal
 * that leaves most of the device's wave slots empty is cut into independent subtrees that run
 * side by side, level by level -- one launch per level (a profiler sees that many launches of the
 * traversal kernel per call). */
unsigned int rdamd_update_clvs_launches(const rdamd_partition_t *p);
/* replaces corax_compute_root_loglikelihood, src/model.cpp:406, :441, :466.
 * persite_lnl may be NULL (the reference always passes nullptr). */
double rdamd_compute_root_loglikelihood(rdamd_partition_t  *p,
                                        unsigned int        clv_index,
                                        int                 scaler_index,
                                        const unsigned int *freqs_indices,
                                        double             *persite_lnl);

/* Fused form of the three calls of model_t::compute_lh_root
 * (src/model.cpp:432-445): two P-matrices + one root op + reduction in a
 * single launch, for `n_alpha` root positions on the same edge at once
 * (compute_dlh, src/model.cpp:481-519, needs two).  The root CLV/scaler of the
 * LAST position is left in the partition as the unfused calls would leave it: the
 * two P-matrices and the scaler bit for bit, the root CLV the one the returned value
 * was reduced from (an entry may differ from the traversal kernel's in its last bits:
 * the two kernels contract their products differently).  Category r reads rate matrix
 * AND frequency set params_indices[r].
 * lengths1/lengths2: child1/child2 branch length per position. */
int rdamd_root_loglikelihood_fused(rdamd_partition_t       *p,
                                   const rdamd_operation_t *root_op,
                                   const unsigned int      *params_indices,
                                   const double            *lengths1,
                                   const double            *lengths2,
                                   unsigned int             n_alpha,
                                   double                  *lnl_out);
/* The same for SEVERAL partitions of one device in ONE launch: item i = partition parts[i],
 * its root operation ops[i], n_positions[i] <= 8 root positions (RDAMD_ROOT_MAX_POSITIONS;
 * <= 4 at 8 rate categories) with branch lengths lengths1[8 i + a] / lengths2[8 i + a];
 * lnl_out[8 i + a].  A lock-stepped search
 * (rdamd_model_exhaustive_search_lockstep) serves the Brent / finite-difference steps
 * (src/model.cpp:606-794) of all candidates in flight -- each on its own model replica --
 * with it.  Every partition is left as rdamd_root_loglikelihood_fused leaves it and every
 * value has that call's bits; the partitions must be idle (no call of another thread in
 * progress on them). */
#define RDAMD_ROOT_MAX_POSITIONS 8
int rdamd_root_loglikelihood_fused_multi(unsigned int              n_items,
                                         rdamd_partition_t *const *parts,
                                         const rdamd_operation_t  *ops,
                                         const unsigned int *const *params_indices,
                                         const double             *lengths1,
                                         const double             *lengths2,
                                         const unsigned int       *n_positions,
                                         double                   *lnl_out);

/* corax_compute_root_loglikelihood for MANY root CLVs of the partition in one
 * launch; every value is bit-identical to a separate call on that CLV.  Used by
 * the all-directions sweep (rdamd_model_compute_all_root_lh_directional). */
int rdamd_compute_root_loglikelihoods(rdamd_partition_t *p, unsigned int count,
                                      const unsigned int *clv_indices, const int *scaler_indices,
                                      const unsigned int *freqs_indices, double *lnl_out);

/* ------------------------------------------------------------------------
 * Batched full-traversal evaluation (the exhaustive-search inner loop)
 *
 * model_t::compute_lh_partition (src/model.cpp:454-476) is the objective the
 * L-BFGS-B driver calls 1 + n_params times per iteration with a pre-generated
 * operation list (src/model.cpp:1488-1502), and the candidate-root loop
 * (src/model.cpp:1154) repeats that per root.  These entry points evaluate a
 * whole batch of such calls -- each job = one schedule (root placement) + one
 * parameter set -- in ONE fused launch that never writes a CLV to HBM.  They
 * are stateless with respect to the partition: its CLV / P-matrix / parameter
 * state is neither read nor changed (tip states and pattern weights are).
 * 4-state (and embedded binary) data, and 20-state data with up to 8 rate
 * categories; other shapes use the three calls above.
 * --------------------------------------------------------------------- */
typedef struct rdamd_schedule rdamd_schedule_t;

/* Compiles the (ops, matrix_indices, branch_lengths) triple that
 * rooted_tree_t::generate_operations returns (src/tree.cpp:364-413) into a
 * device-resident traversal program.  Borrowed inputs; NULL + rdamd_errmsg on a
 * list that is not a complete post-order traversal ending in the root op. */
rdamd_schedule_t *rdamd_schedule_create(rdamd_partition_t       *p,
                                        const rdamd_operation_t *ops,
                                        unsigned int             n_ops,
                                        const unsigned int      *matrix_indices,
                                        const double            *branch_lengths,
                                        unsigned int             n_matrices);
void         rdamd_schedule_destroy(rdamd_schedule_t *s);
/* LDS stack slots per site the compiled traversal needs (diagnostic). */
unsigned int rdamd_schedule_stack_depth(const rdamd_schedule_t *s);

/* Subtree site repeats (coraxlib's CORAX_ATTRIB_SITE_REPEATS, which the reference sets for
 * every 4-state partition, src/model.cpp:145-149).  A partition created with
 * RDAMD_ATTRIB_SITE_REPEATS compiles its schedules with them: a directed subtree below
 * which the alignment's columns fall into at most `max_classes` distinct tip patterns is
 * evaluated once per pattern class and job (a small table) instead of once per site, and the
 * traversal meets it as one more tip.  Results are those of the plain traversal; 4-state
 * (and embedded binary) partitions only, ignored otherwise.
 * rdamd_partition_set_site_repeats changes the class limit for schedules compiled from then
 * on: 0 = off; up to 16 = pseudo-tips share the tips' 16-row tables and 8-bit codes; up to
 * 64 (the attribute's default and the largest accepted value) = 64-row tables as well, 16-bit
 * codes.  Schedules compiled under limits on different sides of 16 cannot share a batch. */
int rdamd_partition_set_site_repeats(rdamd_partition_t *p, unsigned int max_classes);
/* the class limit in force (64 unless rdamd_partition_set_site_repeats changed it); 0: no
 * site repeats on this partition */
unsigned int rdamd_partition_site_repeats(const rdamd_partition_t *p);
/* What one (site, rate) executes per traversal of a compiled schedule, and what the
 * repeats saved: the denominators of the roofline figures (bench.py). */
typedef struct rdamd_schedule_stats {
  unsigned int operations;     /* operations of the caller's list (n - 1) */
  unsigned int steps;          /* operations left after folding clades into pseudo-tips */
  unsigned int matvecs;        /* 4x4 matrix-vector products per (site, rate) in those steps */
  unsigned int matvecs_plain;  /* ... in the plain program (= inner children of the list) */
  unsigned int pseudo_tips;    /* clades folded */
  unsigned int clade_nodes;    /* their nodes = operations evaluated per class instead of per site */
  unsigned int clade_rows;     /* table rows (class x node) computed per job and rate category */
  unsigned int stack_depth;    /* LDS stack levels of the program that runs */
  unsigned int stack_depth_plain;
  /* the program's parks (a subtree's result waits while its sibling is evaluated): all of them, those
   * that wait in the evaluator's register slot(s), those in its one LDS slot (kernels with a
   * private-segment stack); the rest wait on the in-memory stack -- LDS levels or the private segment */
  unsigned int parks, parks_in_registers, parks_in_lds_slot;
} rdamd_schedule_stats_t;
int rdamd_schedule_stats(const rdamd_schedule_t *s, rdamd_schedule_stats_t *out);

/* lnl_out[j] = log-likelihood of job j.  Row-major parameter blocks, K = the
 * partition's states: subst [n_jobs][K*K-K] (corax_set_subst_params order),
 * freqs [n_jobs][K],
 * rates [n_jobs][rate_cats] and rate_weights [n_jobs][rate_cats] (either may be
 * NULL: the partition's current category rates / weights are used). */
int rdamd_evaluate_batch(rdamd_partition_t *p, unsigned int n_jobs,
                         const rdamd_schedule_t *const *schedules,
                         const double *subst, const double *freqs,
                         const double *rates, const double *rate_weights,
                         double *lnl_out);
/* The 4-state evaluator's rescaling policy.  The reference's 2^256 rule keeps
 * CLVs of large trees inside the FP64 range; up to a few hundred tips nothing comes near its end
 * (2^-1022), and the rule only moves exponents.  mode 1: a batch's first pass runs WITHOUT the
 * rescale tests and checks every site's rate sum at the root instead; a job with a sum below 2^-900
 * (or zero) is evaluated again by the second pass -- plain program, every test --, as a job with
 * tiny table entries always was: no result is ever taken from a traversal that came near the
 * range's end.  mode 0: tests on every step (rounds 1 - 5).  mode -1 (the default): 1 for
 * partitions of up to 256 tips, 0 beyond (a 500-tip tree sends every job to the second pass).
 * A job's value depends on the job and the partition's mode only, never on what shares its batch.
 * Partitions a caller does not create itself (rdamd_model_t's and its replicas') take their mode
 * from the environment when they are created: RDAMD_RESCALE_SPECULATION=0 (tests on every step,
 * whatever the tree) or =1; unset: the default rule.
 * rdamd_evaluate_second_passes: batches of this partition that needed their second pass so far. */
int rdamd_partition_set_rescale_speculation(rdamd_partition_t *p, int mode);
unsigned long long rdamd_evaluate_second_passes(const rdamd_partition_t *p);
/* Same, but the n_jobs results are left in DEVICE memory at d_lnl_out (e.g. a
 * tensor that an RCCL all-reduce sums over site-sharded ranks next).  The call BLOCKS like
 * rdamd_evaluate_batch: it returns after the partition's stream has finished writing the
 * results (the batch's second evaluator pass, needed when a job's tables hold entries small
 * enough for the per-site rescaling rule to matter, is decided on the host from a word that
 * comes back with the batch).  Until it returns, d_lnl_out[j] of such a job is unspecified. */
int rdamd_evaluate_batch_device(rdamd_partition_t *p, unsigned int n_jobs,
                                const rdamd_schedule_t *const *schedules,
                                const double *subst, const double *freqs,
                                const double *rates, const double *rate_weights,
                                void *d_lnl_out);

/* The same batch in two halves, for callers that keep TWO batches of one partition in flight
 * (the lock-stepped exhaustive search, src/model.cpp:1139-1272 run for several candidates at
 * once: while one group's batch is on the device the other group's hosts take their L-BFGS-B
 * steps).  _submit queues the batch on `slot` (0 or 1) and returns; _wait blocks until that
 * batch is done and hands out its results.  The part of a batch in front of the evaluator
 * (parameter upload, P-matrices, clade tables) runs beside the evaluator of the batch
 * submitted before it; the evaluators follow each other in submission order.  A slot takes a
 * new batch only after its last one has been waited for.  Both calls may be made from
 * different host threads (one per slot); results are those of rdamd_evaluate_batch, bit for bit. */
int rdamd_evaluate_batch_submit(rdamd_partition_t *p, unsigned int slot, unsigned int n_jobs,
                                const rdamd_schedule_t *const *schedules,
                                const double *subst, const double *freqs,
                                const double *rates, const double *rate_weights);
int rdamd_evaluate_batch_wait(rdamd_partition_t *p, unsigned int slot, double *lnl_out);

/* The STREAM-ORDERED form of a slot's batch, for callers that queue more work behind it on
 * rdamd_partition_stream(p) -- the all-reduce of a site group's per-block lnLs, a
 * copy -- without a host round trip in between.  _submit_device queues the batch like _submit;
 * its finishing kernel writes the n_jobs results to DEVICE memory d_lnl_out[0 .. n_jobs) and,
 * into d_lnl_out[n_jobs], 1.0 if some job of the batch needs the second evaluator pass (see
 * rdamd_evaluate_batch_device) and 0.0 otherwise -- so a sum over the ranks of a site group
 * carries the answer "did anybody's?" to all of them together with the sums.  d_lnl_out must
 * hold n_jobs + 1 doubles.  Nothing is decided on the host in between: whatever the caller
 * queues on the stream next runs right behind the batch.
 *   flag (summed) == 0, the common case: the results are final; _finish_device releases the slot.
 *   flag != 0: EVERY rank of the group calls _redo_device -- it runs the second pass where THIS
 *   rank's batch asked for it, writes this rank's results to d_lnl_out[0 .. n_jobs) again (the
 *   collective summed over the first copy in place) and 0.0 behind them, all in stream order --
 *   and queues its collective again; then _finish_device.
 * _finish_device waits for what _submit_device / _redo_device queued and frees the slot.
 * Results are those of rdamd_evaluate_batch, bit for bit. */
int rdamd_evaluate_batch_submit_device(rdamd_partition_t *p, unsigned int slot, unsigned int n_jobs,
                                       const rdamd_schedule_t *const *schedules,
                                       const double *subst, const double *freqs,
                                       const double *rates, const double *rate_weights,
                                       void *d_lnl_out);
int rdamd_evaluate_batch_redo_device(rdamd_partition_t *p, unsigned int slot, void *d_lnl_out);
int rdamd_evaluate_batch_finish_device(rdamd_partition_t *p, unsigned int slot);

/* compute_lh for a caller that goes on with root-only steps (model_t::exhaustive_search between
 * optimize_params and optimize_alpha, src/model.cpp:1154-1229): ONE evaluation of the whole
 * operation list -- the last operation being the root's -- through the fused evaluator, which
 * also LEAVES THE ROOT OPERATION'S TWO CHILDREN BEHIND: their CLVs and per-site scalers are
 * written to the buffers the root operation names (child*_clv_index / child*_scaler_index; a
 * tip child has nothing to write), in the layout and with the meaning rdamd_update_clvs gives
 * them, so that rdamd_root_loglikelihood_fused / rdamd_compute_root_loglikelihood-style calls
 * on that operation find what a full traversal would have left.  NO OTHER CLV, scaler or
 * P-matrix of the partition is touched (they keep whatever an earlier call left): this replaces
 * corax_update_prob_matrices + corax_update_clvs + corax_compute_root_loglikelihood
 * (src/model.cpp:357-409) where only the root's children are read afterwards -- 13 MB written
 * instead of 1.3 GB moved on BASELINE c2.  Parameters as one job of rdamd_evaluate_batch.
 * 4-state and binary partitions, and 20-state ones with up to 8 rate categories (the fused
 * evaluators' shapes); the children need scale buffers.  *lnl_out = the tree's
 * log-likelihood (every operation of the list evaluated, the reference's rescaling rule at
 * every step). */
int rdamd_evaluate_root_children(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                                 const unsigned int *matrix_indices, const double *branch_lengths,
                                 unsigned int n_matrices, const double *subst, const double *freqs,
                                 const double *rates, const double *rate_weights, double *lnl_out);


/* parity/debug views: copy device buffers to host.  rdamd_get_clv returns coraxlib's
 * layout, out[site][rate][state] (what partition->clv[i] holds in the reference),
 * whatever layout the device keeps the CLV in. */
int rdamd_get_clv(rdamd_partition_t *p, unsigned int clv_index, double *out);
int rdamd_get_scaler(rdamd_partition_t *p, unsigned int scaler_index,
                     unsigned int *out);
int rdamd_get_pmatrix(rdamd_partition_t *p, unsigned int matrix_index,
                      double *out);

/* Measurement hooks (bench.py): while enabled, every kernel launch of the
 * partition is bracketed by HIP events on the partition's stream.
 * rdamd_profile_read synchronises, returns accumulated kernel milliseconds and
 * launch counts per kernel family {0: CLV level, 1: P-matrix, 2: root lnL,
 * 3: fused traversal (+ its finishing reduction), 4: batched P-matrix, 5: the
 * pre-order pass and the site-rate kernel, 6-7: reserved}, and resets the accumulators. */
void rdamd_profile_enable(rdamd_partition_t *p, int on);
int  rdamd_profile_read(rdamd_partition_t *p, double ms_out[8],
                        unsigned int launches_out[8]);

/* blocks until all queued device work of the partition has finished. */
void rdamd_partition_sync(rdamd_partition_t *p);


/* ------------------------------------------------------------------------
 * Host-side schedule generation: rooted_tree_t (src/tree.hpp:54-201)
 *
 * The C++ class lives in root_digger_amd/csrc/tree.hpp; these wrappers expose
 * it to C / ctypes callers.  Functions returning int give RDAMD_SUCCESS or
 * RDAMD_FAILURE (+ rdamd_errmsg) where the C++ method would throw.
 * --------------------------------------------------------------------- */
typedef struct rdamd_tree rdamd_tree_t;

/* replaces root_location_t (src/tree.hpp:24-52); `edge` is a half-edge id. */
typedef struct rdamd_root_location {
  int      edge;
  uint64_t id;
  double   saved_brlen;
  double   brlen_ratio;
} rdamd_root_location_t;

/* rooted_tree_t(const std::string &tree_filename), src/tree.hpp:58-66 */
rdamd_tree_t *rdamd_tree_from_file(const char *filename);
rdamd_tree_t *rdamd_tree_from_newick(const char *newick);
void          rdamd_tree_destroy(rdamd_tree_t *t);
unsigned int  rdamd_tree_tip_count(const rdamd_tree_t *t);    /* src/tree.cpp:102 */
unsigned int  rdamd_tree_inner_count(const rdamd_tree_t *t);  /* src/tree.cpp:103 */
unsigned int  rdamd_tree_branch_count(const rdamd_tree_t *t); /* src/tree.cpp:106 */
unsigned int  rdamd_tree_root_count(const rdamd_tree_t *t);   /* src/tree.cpp:100 */
unsigned int  rdamd_tree_root_clv_index(const rdamd_tree_t *t);   /* :110 */
int           rdamd_tree_root_scaler_index(const rdamd_tree_t *t); /* :113 */
int rdamd_tree_root_location(const rdamd_tree_t *t, unsigned int index,
                             rdamd_root_location_t *out);        /* :74-82 */
int rdamd_tree_root_location_by_label(const rdamd_tree_t *t, const char *label,
                                      rdamd_root_location_t *out); /* :84-91 */
/* rank_midpoints (:863-901) / rank_modified_mad (:907-945): the root ids ordered
 * best first by how well each branch balances the tree; root_ids holds
 * root_count entries.  midpoint() is the first of rank_midpoints. */
int rdamd_tree_rank_midpoints(const rdamd_tree_t *t, unsigned int *root_ids);
int rdamd_tree_rank_modified_mad(const rdamd_tree_t *t, unsigned int *root_ids);
/* label of a root location ("(null)" when unlabeled), src/tree.hpp:36-38 */
const char *rdamd_tree_root_label(const rdamd_tree_t *t, unsigned int index);
int rdamd_tree_root_is_internal(const rdamd_tree_t *t, unsigned int index);
/* label_map(), src/tree.cpp:117-125: tip label -> tip clv index (or -1) */
int         rdamd_tree_tip_index(const rdamd_tree_t *t, const char *label);
const char *rdamd_tree_tip_label(const rdamd_tree_t *t, unsigned int clv_index);
/* tip labels on the rl.edge side of a root branch, '\n'-joined, malloc'd */
char *rdamd_tree_side_tips(const rdamd_tree_t *t, const rdamd_root_location_t *rl);

/* generate_operations, src/tree.cpp:364-413.  ops must hold tip_count
 * entries, pmatrix_indices/branch_lengths 2*tip_count entries. */
int rdamd_tree_generate_operations(rdamd_tree_t *t, const rdamd_root_location_t *rl,
                                   rdamd_operation_t *ops, unsigned int *n_ops,
                                   unsigned int *pmatrix_indices,
                                   double *branch_lengths, unsigned int *n_matrices);
/* generate_derivative_operations, src/tree.cpp:415-441 (1 op, 2 matrices) */
int rdamd_tree_generate_derivative_operations(rdamd_tree_t *t,
                                              const rdamd_root_location_t *rl,
                                              rdamd_operation_t *op,
                                              unsigned int *pmatrix_indices,
                                              double *branch_lengths);
/* generate_root_update_operations, src/tree.cpp:572-657 */
int rdamd_tree_generate_root_update_operations(rdamd_tree_t *t,
                                               const rdamd_root_location_t *rl,
                                               rdamd_operation_t *ops, unsigned int *n_ops,
                                               unsigned int *pmatrix_indices,
                                               double *branch_lengths,
                                               unsigned int *n_matrices);
int  rdamd_tree_root_by(rdamd_tree_t *t, const rdamd_root_location_t *rl); /* :273 */
void rdamd_tree_unroot(rdamd_tree_t *t);                                   /* :334 */
int  rdamd_tree_rooted(const rdamd_tree_t *t);                             /* :360 */
int  rdamd_tree_sanity_check(const rdamd_tree_t *t);                       /* :519 */
/* newick(annotations), src/tree.cpp:443-492; malloc'd, caller frees */
char *rdamd_tree_newick(const rdamd_tree_t *t, int annotations);
/* the same string without annotations and with the inner node whose CLV index is node_clv[k]
 * labelled N<k> instead of its own label (new here: the tree that goes with the node order of
 * rdamd_marginal_ancestral_nodes; root the tree with rdamd_tree_root_by first); malloc'd */
char *rdamd_tree_newick_ancestral(const rdamd_tree_t *t, unsigned int n_nodes, const unsigned int *node_clv);
/* the same string with lengths[n_nodes][2] on the branches: lengths[k][c] above child c of the node
 * whose CLV is node_clv[k] (rdamd_model_optimize_branch_lengths); inner labels as above; malloc'd */
char *rdamd_tree_newick_branch_lengths(const rdamd_tree_t *t, unsigned int n_nodes, const unsigned int *node_clv,
                                       const double *lengths);
int   rdamd_tree_annotate_branch(rdamd_tree_t *t, const rdamd_root_location_t *rl,
                                 const char *key, const char *value); /* :731 */
/* annotate_branch(rl, key, left_value, right_value), src/tree.cpp:737-760 */
int   rdamd_tree_annotate_branch_lr(rdamd_tree_t *t, const rdamd_root_location_t *rl,
                                    const char *key, const char *left_value,
                                    const char *right_value);

/* ------------------------------------------------------------------------
 * Host-side likelihood facade: model_t (src/model.hpp:47-277)
 *
 * C wrappers over the C++ class in root_digger_amd/csrc/model.hpp for one
 * partition (the C++ class takes any number).  Rows a4-a9, a16, a17 of
 * SURVEY.md section 8a.
 * --------------------------------------------------------------------- */
typedef struct rdamd_model rdamd_model_t;

/* model_t(tree, {msa}, {rate_cats}, invariant_sites=false, seed, early_stop),
 * src/model.cpp:99-176; the tree is copied.  weights may be NULL (all 1). */
rdamd_model_t *rdamd_model_create(const rdamd_tree_t *tree, unsigned int n_taxa,
                                  const char *const *labels, const char *const *sequences,
                                  const unsigned int *weights, unsigned int states,
                                  const uint64_t *map, unsigned int rate_cats,
                                  uint64_t seed, int early_stop);
/* Same, reading the alignment from a PHYLIP / FASTA file with site-pattern
 * compression (msa_t(filename), src/msa.hpp:23-37).  *n_patterns (may be NULL)
 * receives the compressed length. */
rdamd_model_t *rdamd_model_create_from_file(const rdamd_tree_t *tree, const char *msa_filename,
                                            unsigned int states, const uint64_t *map,
                                            unsigned int rate_cats, uint64_t seed,
                                            int early_stop, int compress,
                                            unsigned int *n_patterns);
/* Parses an alignment file the way msa_t(filename) does and reports its shape
 * (host only; no GPU needed). */
int rdamd_msa_probe(const char *msa_filename, const uint64_t *map, int compress,
                    unsigned int *n_taxa, unsigned int *n_patterns,
                    unsigned int *total_weight);
void rdamd_model_destroy(rdamd_model_t *m);
/* initialize_partitions / initialize_partitions_uniform_freqs, :1297-1321 */
int rdamd_model_initialize_partitions(rdamd_model_t *m, int uniform_freqs);
int rdamd_model_set_subst_rates(rdamd_model_t *m, const double *rates);      /* :184 */
int rdamd_model_set_subst_rates_uniform(rdamd_model_t *m);                   /* :1748 */
int rdamd_model_set_freqs(rdamd_model_t *m, const double *freqs);            /* :341 */
int rdamd_model_set_empirical_freqs(rdamd_model_t *m);                       /* :327 */
int rdamd_model_set_gamma_alpha(rdamd_model_t *m, double alpha);             /* :224 */
/* compute_lh / compute_lh_root, :384-452 (NaN + rdamd_errmsg on failure) */
double rdamd_model_compute_lh(rdamd_model_t *m, const rdamd_root_location_t *rl);
double rdamd_model_compute_lh_root(rdamd_model_t *m, const rdamd_root_location_t *rl);
/* compute_dlh, :481-519: out = {lh, dlh} */
int rdamd_model_compute_dlh(rdamd_model_t *m, const rdamd_root_location_t *rl, double out[2]);
int rdamd_model_move_root(rdamd_model_t *m, const rdamd_root_location_t *rl);  /* :823 */
/* compute_all_root_lh, :1737-1746: out holds root_count values */
int rdamd_model_compute_all_root_lh(rdamd_model_t *m, double *out);
/* the same sweep as ONE fused launch (every root a job), partition untouched */
int rdamd_model_compute_all_root_lh_batched(rdamd_model_t *m, double *out);
/* the same sweep through an all-directions CLV cache: a
 * partition of its own holds the 3(n-2) directed CLVs, so the 2n-3 likelihoods
 * cost 3(n-2) + (2n-3) operations and one batched root reduction.  4-state /
 * binary single-partition models; `ratios` (root_count values) overrides the
 * stored alpha of every root when not NULL. */
int rdamd_model_compute_all_root_lh_directional(rdamd_model_t *m, const double *ratios, double *out);
/* generate_directional_operations of the tree (csrc/tree.hpp): ops holds
 * 3(n-2) + (2n-3) entries, the matrix arrays (2n-3) + 2(2n-3); sizes[3] =
 * {clv_buffers, scale_buffers, prob_matrices} the partition needs */
int rdamd_tree_generate_directional_operations(const rdamd_tree_t *t, const double *ratios,
                                               rdamd_operation_t *ops, unsigned int *n_ops,
                                               unsigned int *matrix_indices,
                                               double *branch_lengths, unsigned int *n_matrices,
                                               unsigned int *root_clv, int *root_scaler,
                                               unsigned int sizes[3]);
/* heuristic search(min_roots, root_ratio, atol, pgtol, brtol, factor), :1008-1137
 * (needs rdamd_model_set_lbfgsb); best placement and its lnL are returned. */
int rdamd_model_search(rdamd_model_t *m, unsigned int min_roots, double root_ratio, double atol,
                       double pgtol, double brtol, double factor,
                       rdamd_root_location_t *best_rl, double *best_llh);
/* optimize_alpha, :679-794 */
int rdamd_model_optimize_alpha(rdamd_model_t *m, const rdamd_root_location_t *rl, double atol,
                               rdamd_root_location_t *out);
/* batched objective over (root, parameter) pairs: subst [n][K*K-K], freqs
 * [n][K], gamma_alpha [n] (NULL = 1.0); through rdamd_evaluate_batch */
int rdamd_model_compute_lh_batch(rdamd_model_t *m, unsigned int n,
                                 const rdamd_root_location_t *rls, const double *subst,
                                 const double *freqs, const double *gamma_alpha, double *out);
/* Hands the model the caller's L-BFGS-B entry point (the reference's vendored
 * `setulb`, lib/lbfgsb/lbfgsb.h:196-201).  exhaustive_search then optimises
 * rates / frequencies / gamma alpha as optimize_params does
 * (src/model.cpp:1925-1984), with every objective + finite-difference
 * gradient evaluation (src/model.cpp:1488-1502) as ONE batched launch. */
void rdamd_model_set_lbfgsb(rdamd_model_t *m, void *setulb_entry_point);
/* optimize_params for the current parameters at root rl; returns them
 * (subst [12], freqs [4], gamma_alpha [1]) and the objective statistics. */
int rdamd_model_optimize_params(rdamd_model_t *m, const rdamd_root_location_t *rl,
                                double pgtol, double factor, int optimize_gamma,
                                double *subst, double *freqs, double *gamma_alpha,
                                uint64_t *n_batches, uint64_t *n_evaluations);
/* work counters since the model was created: out[0] objective batches (fused
 * launches), [1] objective evaluations, [2] full traversals through
 * compute_lh, [3] root-only positions (compute_lh_root / compute_dlh),
 * [4] move_root calls, [5] setulb calls.  Diagnostic. */
void rdamd_model_counters(const rdamd_model_t *m, uint64_t out[6]);
/* the last rdamd_model_exhaustive_search_lockstep: out[0] combined objective launches,
 * [1] the jobs they carried, [2] combined root-only launches
 * (rdamd_root_loglikelihood_fused_multi), [3] the candidates' root-only steps they carried */
void rdamd_model_lockstep_stats(const rdamd_model_t *m, uint64_t out[4]);
/* How the candidates in flight of a lock-stepped search meet: 0 (default) = the library's
 * choice -- from four candidates on, TWO groups whose objective batches alternate on the
 * shared partition (rdamd_evaluate_batch_submit / _wait: one group's hosts take their
 * L-BFGS-B steps while the other group's batch runs), except for a site-sharded model, whose
 * rounds each end in a collective: ONE group there (launches twice as large, half the
 * collectives); 1 = one group; 2 = two groups.
 * The records are the same either way (a job's value does not depend on its launch). */
void rdamd_model_set_lockstep_groups(rdamd_model_t *m, unsigned int groups);
/* How a lock-stepped search forms its launches.  In ARRIVAL ORDER (batch combiners: whoever has
 * asked when the others are busy elsewhere goes), or in DETERMINISTIC ROUNDS: a round closes when
 * every candidate in flight has posted its next request -- an L-BFGS-B step's evaluations, root
 * positions of its branch, a value to be summed, or "next candidate" --, the requests run as one
 * objective launch plus one root-only launch, and ONE collective sums everything the round
 * produced over the site group (csrc/lockstep_conductor.hpp).  The ranks of a site group then
 * form identical rounds, which is what lets a SITE-SHARDED model search in lock step at all.
 * mode -1 (default): rounds for site-sharded models, arrival order otherwise; 0: arrival order
 * (a site-sharded model refuses); 1: rounds always.  Records are the sequential search's either
 * way.  A partitioned model's round makes one objective launch per partition that has jobs, each
 * on that partition's stream, and still ONE collective for all of them. */
void rdamd_model_set_lockstep_rounds(rdamd_model_t *m, int mode);
/* the last search in rounds: out[0] rounds closed, [1] collectives queued (rounds that had
 * anything to sum, plus repeats), [2] rounds repeated because a rank's batch needed its second
 * evaluator pass (only the partitions whose batch did launch again); [3] (any search) collectives THIS model asked its reducer for by itself --
 * the sequential site-sharded search's count, one per request */
void rdamd_model_round_stats(const rdamd_model_t *m, uint64_t out[4]);
/* ... per objective partition p of the last search in rounds: out[0] objective launches of that
 * partition (at most one per round), [1] its second-pass launches in repeated rounds -- only the
 * partitions whose batch raised the flag launch again */
int rdamd_model_round_partition_stats(const rdamd_model_t *m, unsigned int p, uint64_t out[2]);
/* ... and where its rounds spent their host time, seconds summed over the rounds: out[0] queueing
 * the objective batch, [1] the root-only launch (it blocks), [2] queueing the sum (a host
 * reducer: waiting for the batch and summing), [3] waiting for the round's event */
void rdamd_model_round_seconds(const rdamd_model_t *m, double out[4]);
/* stream priority (rdamd_partition_set_stream_priority) of the shared objective partition
 * during a lock-stepped search: +1 low (default), 0 leave it as it is */
void rdamd_model_set_lockstep_priority(rdamd_model_t *m, int level);
/* The searches' compute_lh between optimize_params and the root-only steps: 1 (default) =
 * rdamd_evaluate_root_children where the partition allows it (4-state / binary), 0 = always
 * the full traversal that materialises every CLV (rdamd_update_clvs). */
void rdamd_model_set_root_children_only(rdamd_model_t *m, int on);
/* assign_indicies_by_rank_exhaustive, :1867-1911 */
int rdamd_model_assign_by_rank(rdamd_model_t *m, unsigned int rank, unsigned int num_tasks);
/* exhaustive_search, :1139-1272, over the assigned roots.  root_id / llh /
 * alpha hold root_count entries; *n_results is set; best_* may be NULL. */
int rdamd_model_exhaustive_search(rdamd_model_t *m, double atol, double pgtol, double brtol,
                                  double factor, uint64_t *root_id, double *llh, double *alpha,
                                  unsigned int *n_results, rdamd_root_location_t *best_rl,
                                  double *best_llh);
/* The same loop with `workers` host threads, each driving its own replica of the
 * model (own partition, own HIP stream) and pulling candidates from a shared
 * counter: the one-GPU form of the reference's one-MPI-rank-per-chunk split
 * (src/model.cpp:1867-1911).  Results come back sorted by root id. */
int rdamd_model_exhaustive_search_parallel(rdamd_model_t *m, unsigned int workers,
                                           double atol, double pgtol, double brtol,
                                           double factor, uint64_t *root_id, double *llh,
                                           double *alpha, unsigned int *n_results,
                                           rdamd_root_location_t *best_rl, double *best_llh);
/* Lock-stepped form: `in_flight` candidates advance together; whenever all of
 * those that are inside optimize_params have asked for their next objective
 * batch (the n+1 evaluations of one L-BFGS-B step, src/model.cpp:1430-1522),
 * ONE fused launch on m's own partition serves them all.  Same results as the
 * sequential loop; launch-bound (small) alignments gain the most. */
int rdamd_model_exhaustive_search_lockstep(rdamd_model_t *m, unsigned int in_flight,
                                           double atol, double pgtol, double brtol,
                                           double factor, uint64_t *root_id, double *llh,
                                           double *alpha, unsigned int *n_results,
                                           rdamd_root_location_t *best_rl, double *best_llh);

/* ------------------------------------------------------------------------
 * Result log / checkpoint: byte-compatible with the reference's <prefix>.ckp
 * (checkpoint_t, src/checkpoint.hpp:231-300, src/checkpoint.cpp).  A search
 * appends (root id, lnL, alpha, parameters) per finished candidate under an
 * fcntl lock, so one file is shared by every process of a multi-GPU run the
 * way the reference's MPI ranks share it, and an interrupted run resumes from
 * it (by either program).
 * ---------------------------------------------------------------------- */
typedef struct rdamd_checkpoint rdamd_checkpoint_t;

typedef struct {   /* ratehet_opts_t, src/util.hpp:50-70 */
  int32_t  type;                 /* param_type: 0 emperical 1 estimate 2 equal 3 user */
  int32_t  rate_category_type;   /* 0 MEDIAN 1 MEAN 2 FREE */
  uint64_t rate_cats;
  int32_t  alpha_init;
  double   alpha;
} rdamd_ratehet_opts_t;

typedef struct {   /* the serialised fields of cli_options_t, src/checkpoint.cpp:60-91 */
  const char *msa_filename, *tree_filename, *prefix, *prefix_dir, *model_filename,
             *freqs_filename, *partition_filename, *data_type, *model_string;
  const rdamd_ratehet_opts_t *rate_cats;
  uint64_t n_rate_cats;
  uint64_t seed, min_roots, threads;
  double   root_ratio, abs_tolerance, factor, br_tolerance, bfgs_tol;
  int32_t  silent, exhaustive, echo, invariant_sites;
  int32_t  early_stop;             /* 0 unset, 1 true, 2 false (initialized_flag_t) */
  int32_t  initial_root_strategy;  /* 0 random, 1 midpoint, 2 modified_mad */
} rdamd_cli_options_t;

/* checkpoint_t(prefix): opens or creates <prefix>.ckp */
rdamd_checkpoint_t *rdamd_checkpoint_open(const char *prefix);
void        rdamd_checkpoint_close(rdamd_checkpoint_t *c);
int         rdamd_checkpoint_existing(const rdamd_checkpoint_t *c);   /* existing_checkpoint() */
const char *rdamd_checkpoint_filename(rdamd_checkpoint_t *c);
/* save_options (new file only) / load_options (existing file only; the strings
 * stay valid until the next load or close) */
int rdamd_checkpoint_save_options(rdamd_checkpoint_t *c, const rdamd_cli_options_t *o);
int rdamd_checkpoint_load_options(rdamd_checkpoint_t *c, rdamd_cli_options_t *o);
/* write(result, parameters): counts[n_partitions][4] = lengths of subst_rates,
 * freqs, gamma_alpha, gamma_weights; values = those vectors back to back */
int rdamd_checkpoint_write(rdamd_checkpoint_t *c, uint64_t root_id, double llh, double alpha,
                           unsigned int n_partitions, const uint64_t *counts,
                           const double *values);
/* read_results(): takes a snapshot; its entries are then read one by one */
int rdamd_checkpoint_read_results(rdamd_checkpoint_t *c, unsigned int *n_results);
int rdamd_checkpoint_result(const rdamd_checkpoint_t *c, unsigned int index, uint64_t *root_id,
                            double *llh, double *alpha, unsigned int *n_partitions,
                            uint64_t *n_values);
int rdamd_checkpoint_result_params(const rdamd_checkpoint_t *c, unsigned int index,
                                   uint64_t *counts, double *values);
int rdamd_checkpoint_needs_cleaning(rdamd_checkpoint_t *c);   /* 1 / 0, -1 on error */
int rdamd_checkpoint_clean(rdamd_checkpoint_t *c);
/* the file's record checksums (the reference's Adler-32 variant) */
uint32_t rdamd_checkpoint_checksum_result(uint64_t root_id, double llh, double alpha);
uint32_t rdamd_checkpoint_checksum_params(unsigned int n_partitions, const uint64_t *counts,
                                          const double *values);
/* on: the searches print the reference's progress lines ("Step i / n, ETC: h",
 * src/model.cpp:1219-1223) to stdout, counting over the roots assigned at the
 * time of the call; call it after the assign function.  off: silent. */
int rdamd_model_set_progress(rdamd_model_t *m, int on);
/* searches of this model append every finished candidate to `c` (NULL detaches),
 * src/model.cpp:1107 and :1215 */
int rdamd_model_set_checkpoint(rdamd_model_t *m, rdamd_checkpoint_t *c);
/* assign_indicies_by_rank_exhaustive(rank, num_tasks, checkpoint), :1867-1911:
 * the roots already in the log are skipped */
int rdamd_model_assign_by_rank_checkpoint(rdamd_model_t *m, unsigned int rank,
                                          unsigned int num_tasks, rdamd_checkpoint_t *c);
/* assign_indicies_by_rank_search, :1809-1865: the heuristic search's starting
 * roots = the first max(root_count*root_ratio, min_roots) of an ordering
 * (0 random shuffle with the model's seed, 1 midpoint rank, 2 modified MAD
 * rank), minus the roots already in `c` (may be NULL), chunked over the ranks */
int rdamd_model_assign_by_rank_search(rdamd_model_t *m, unsigned int min_roots, double root_ratio,
                                      unsigned int rank, unsigned int num_tasks,
                                      int initial_root_strategy, rdamd_checkpoint_t *c);
/* the root ids currently assigned to this model; returns how many there are */
int rdamd_model_assigned(const rdamd_model_t *m, uint64_t *root_ids, unsigned int cap);

/* ------------------------------------------------------------------------
 * Partition file / model string front end (src/msa.cpp:91-522): which columns
 * form each partition and what its model string asks for.
 * ---------------------------------------------------------------------- */
typedef struct {   /* partition_info_t + model_info_t, src/util.hpp:86-100 */
  char     model_name[256], partition_name[128], subst_str[64];
  unsigned int n_ranges;
  uint64_t ranges[64][2];          /* 1-based, inclusive */
  int32_t  freq_type;              /* param_type: 0 emperical 1 estimate 2 equal 3 user */
  int32_t  invar_present, invar_type;
  float    invar_user_prop;
  rdamd_ratehet_opts_t ratehet;    /* rate_cats == 0: the string has no +G / +R */
  int32_t  asc_present, asc_type;  /* 0 lewis 1 fels 2 stam */
  double   asc_fels_weight;
  unsigned int n_stam_weights;
  double   stam_weights[32];
} rdamd_partition_info_t;
/* parse_model_info, :364-415 / parse_partition_info, :417-506 */
int rdamd_parse_model_info(const char *model_string, rdamd_partition_info_t *out);
int rdamd_parse_partition_info(const char *line, rdamd_partition_info_t *out);
/* msa_t::partition, :522-591: length (patterns when compress != 0) and total
 * weight of each partition described by `lines` */
int rdamd_msa_partition_probe(const char *msa_filename, const uint64_t *map,
                              unsigned int n_lines, const char *const *lines, int compress,
                              unsigned int *lengths, unsigned int *total_weights);
/* the partitioned model of src/main.cpp:512-555: one partition per line of the
 * partition file, rate categories from each line's model string */
rdamd_model_t *rdamd_model_create_partitioned(const rdamd_tree_t *tree, const char *msa_filename,
                                              const char *partition_filename,
                                              unsigned int states, const uint64_t *map,
                                              uint64_t seed, int early_stop,
                                              unsigned int *n_partitions);
int rdamd_model_partition_count(const rdamd_model_t *m);
/* rdamd_model_create_from_file with the full rate-heterogeneity option
 * (`rd --rate-cats N --rate-cats-type {mean,median,free}`, src/main.cpp:256-266) */
rdamd_model_t *rdamd_model_create_from_file_ratehet(const rdamd_tree_t *tree,
                                                    const char *msa_filename,
                                                    unsigned int states, const uint64_t *map,
                                                    const rdamd_ratehet_opts_t *ratehet,
                                                    uint64_t seed, int early_stop, int compress,
                                                    unsigned int *n_patterns);

/* character maps (replace corax_map_nt / corax_map_bin, src/main.cpp:484) */
extern const uint64_t rdamd_map_nt[256];
extern const uint64_t rdamd_map_bin[256];

/* ---- site-sharded runs ------------------------------------------------------
 * North star / SURVEY 8(e): "candidate edges and site blocks shard across the 8
 * GPUs of one node with an RCCL all-reduce of per-block log-likelihoods".  The
 * reference has no site sharding (its MPI ranks split candidates only,
 * src/model.cpp:1867-1911); here each rank of a SITE GROUP builds its model on
 * one contiguous block of alignment columns and every log-likelihood the model
 * hands to its optimisers (compute_lh, compute_lh_root, compute_dlh, the
 * L-BFGS-B objective batches of src/model.cpp:1488-1502, the root sweeps) is
 * summed over the group through this hook before it is used, so all ranks of a
 * group follow the same trajectory bit for bit.  Empirical frequencies are
 * combined the same way (weighted by each block's column count).
 *
 * on_device = 0: `values` is a host array; sum it over the group in place.
 * on_device = 1: `values` is DEVICE memory and `stream` the HIP stream handle the
 *   producing launch was queued on: queue the collective on that stream
 *   (rdamd_comm_allreduce_sum: ncclAllGather + a rank-order sum kernel by default, or
 *   ncclAllReduce(values, values, n, ncclDouble, ncclSum, comm, stream)).
 * EVERY RANK OF THE GROUP MUST RECEIVE THE SAME BITS: the optimisers branch on these sums.  A
 * reducer that cannot promise that (see RDAMD_COMM_SUM_ALLREDUCE) forks the ranks' trajectories;
 * the searches check for it with every reduction and fail at once (divergence guard: two or three
 * extra words ride behind the values of every vector handed to the reducer -- csrc/model.cpp
 * guard_check, csrc/lockstep_conductor.hpp) instead of waiting in a collective that no longer
 * matches.
 * Return RDAMD_SUCCESS.  A site-sharded model runs its candidates sequentially
 * (rdamd_model_exhaustive_search) or in lock step in deterministic rounds
 * (rdamd_model_exhaustive_search_lockstep; every rank of the group with the same `in_flight`);
 * free-running replicas (rdamd_model_exhaustive_search_parallel) would reorder the collectives. */
typedef int (*rdamd_lnl_reducer_t)(double *values, unsigned int n, void *stream, void *user);
int rdamd_model_set_lnl_reducer(rdamd_model_t *m, rdamd_lnl_reducer_t reduce, void *user,
                                int on_device);
/* A device-side reducer in TWO halves, for the lock-stepped search of a site-sharded model
 * (rdamd_model_exhaustive_search_lockstep): `queue` only queues the collective on the stream it
 * is given and returns; `wait(event, user)` blocks until the HIP event `event` -- recorded by the
 * library on that stream, behind the collective and the copy that brings the sums back -- has
 * happened, or fails.  While one group of candidates waits for its sums the other group's round
 * is queued behind them.  The blocking form every other path uses is `queue` followed by a
 * synchronisation of the stream.
 * rdamd_model_set_lnl_reducer(m, rdamd_comm_reducer, comm, 1) installs rdamd_comm_reducer_queue /
 * rdamd_comm_reducer_wait by itself. */
typedef int (*rdamd_lnl_wait_t)(void *event, void *user);
int rdamd_model_set_lnl_reducer_async(rdamd_model_t *m, rdamd_lnl_reducer_t queue, rdamd_lnl_wait_t wait,
                                      void *user);
/* How to get this process OUT of the reducer (optional).  A lock-stepped search whose round
 * fails -- the divergence guard of csrc/lockstep_conductor.hpp, a failed launch -- fails on every
 * rank in the same round, but another worker group's round may already sit in a collective that
 * the ranks which failed a moment earlier will never join.  `abort(user)` is called once, from
 * the failing thread, and must make every pending and future call of the reducer / `wait` return
 * failure promptly; it may be called from any thread.  rdamd_model_set_lnl_reducer(m,
 * rdamd_comm_reducer, comm, 1) installs rdamd_comm_abort by itself. */
typedef void (*rdamd_lnl_abort_t)(void *user);
int rdamd_model_set_lnl_reducer_abort(rdamd_model_t *m, rdamd_lnl_abort_t abort, void *user);
/* rdamd_model_create_from_file_ratehet on block `block` of `n_blocks` contiguous
 * column blocks of the alignment (chunking of src/model.cpp:1899-1907 applied to
 * columns; the block is cut BEFORE pattern compression).  n_columns: optional,
 * the whole alignment's column count. */
rdamd_model_t *rdamd_model_create_from_file_block(const rdamd_tree_t *tree, const char *msa_filename,
                                                  unsigned int states, const uint64_t *map,
                                                  const rdamd_ratehet_opts_t *ratehet,
                                                  uint64_t seed, int early_stop, int compress,
                                                  unsigned int block, unsigned int n_blocks,
                                                  unsigned int *n_patterns,
                                                  unsigned int *n_columns);
/* One rank's block of the partitioned model of src/main.cpp:512-555 (a site-sharded run with a
 * partition file).  The alignment is read whole and cut into the partition file's column ranges,
 * as rdamd_model_create_partitioned does; then EACH PARTITION'S OWN columns (its ranges, in file
 * order) are split into n_blocks contiguous blocks by the rule of rdamd_model_create_from_file_block
 * (chunking of src/model.cpp:1899-1907), and this model holds block `block` of every partition,
 * each compressed on its own.  Rate categories come from each line's model string.  A partition
 * with fewer columns than n_blocks is refused (the error names it).  n_partitions: optional.
 * patterns / columns (optional): per partition, the block's patterns and the partition's whole
 * column count -- room for one entry per non-blank line of the partition file.
 * Summation order of a site group on this model (rdamd_model_set_lnl_reducer): a partition's
 * objective value is the group's sum of its block lnLs; a root lnL is summed over the partitions
 * in file order on each rank, then over the group; empirical frequencies are the group's
 * per-partition sums.  The sequential search and the search in rounds
 * (rdamd_model_exhaustive_search_lockstep) add the same numbers in that order. */
rdamd_model_t *rdamd_model_create_partitioned_block(const rdamd_tree_t *tree, const char *msa_filename,
                                                    const char *partition_filename, unsigned int states,
                                                    const uint64_t *map, uint64_t seed, int early_stop,
                                                    unsigned int block, unsigned int n_blocks,
                                                    unsigned int *n_partitions, unsigned int *patterns,
                                                    unsigned int *columns);
/* compute_lh's per-partition terms at rl on THIS model's own columns, not summed over a site
 * group: out[p] for every partition, in file order.  Diagnostic. */
int rdamd_model_partition_lnls(rdamd_model_t *m, const rdamd_root_location_t *rl, double *out);
/* the frequencies partition p of the model evaluates with now (states doubles) */
int rdamd_model_partition_frequencies(rdamd_model_t *m, unsigned int p, double *out);
/* rdamd_evaluate_second_passes of the model's own partition p (the objective partition of a
 * search in rounds): batches that needed the evaluator's second pass so far */
unsigned long long rdamd_model_partition_second_passes(const rdamd_model_t *m, unsigned int p);

/* ------------------------------------------------------------------------
 * Site log-likelihoods of candidate roots and their RELL bootstrap
 * (Kishino, Miyata & Hasegawa 1990; not in the reference, which always passes
 * persite_lnl = NULL).
 * ---------------------------------------------------------------------- */
/* Site patterns of the model, all partitions concatenated in partition order: P_total patterns
 * standing for N_columns alignment columns.  weights[P_total]: pattern multiplicities;
 * pattern_of[N_columns]: the pattern every column was compressed into -- per partition in the
 * partition's own column order (the alignment's for an unpartitioned model, the partition file's
 * ranges back to back otherwise), partition after partition, as indices into the concatenated
 * pattern list.  A model made from caller-supplied patterns (rdamd_model_create) has no columns of
 * its own: pattern p then owns weights[p] consecutive columns.  Any pointer may be NULL.
 * Refused (error 61) for a model that sums over a site group (rdamd_model_set_lnl_reducer). */
int rdamd_model_site_patterns(rdamd_model_t *m, unsigned int *P_total, unsigned int *N_columns,
                              unsigned int *weights, unsigned int *pattern_of);
/* The same for an alignment FILE, as a model made from it holds it (host only, no device):
 * n_lines = 0: the whole alignment, compressed; otherwise the partitions the given partition-file
 * lines describe, each compressed on its own, concatenated.  sequences (optional):
 * [n_taxa][P_total] characters, the compressed alignment itself, taxa in file order (characters
 * with the same state set are merged into one, as the compression does).  Call once with the
 * buffers NULL for the sizes. */
int rdamd_msa_pattern_probe(const char *msa_filename, const uint64_t *map, unsigned int n_lines,
                            const char *const *lines, unsigned int *n_taxa, unsigned int *P_total,
                            unsigned int *N_columns, unsigned int *weights, unsigned int *pattern_of,
                            char *sequences);
/* out[n][P_total]: for each of the n root locations (rls[i].brlen_ratio is the root's position on
 * its branch) the UNWEIGHTED log-likelihood of every site pattern, partitions concatenated in
 * partition order.  Root i is evaluated with its own parameters, given in the checkpoint's layout
 * (what rdamd_checkpoint_result_params returns): counts[n][n_partitions][4] = lengths of
 * subst_rates, freqs, gamma_alpha, gamma_weights, `values` = all those vectors back to back;
 * applied as the searches apply a candidate's parameters (frequencies are normalised).
 * counts = values = NULL: the model's current parameters for every root.
 * One materialising traversal and rdamd_compute_root_loglikelihood(..., persite_lnl) per root
 * and partition: any state count the model accepts.  The model's parameters, its rooting and the
 * conditional likelihoods of that rooting are as before when the call returns.
 * Refused (error 61) for a model that sums over a site group. */
int rdamd_model_site_lnls(rdamd_model_t *m, unsigned int n, const rdamd_root_location_t *rls,
                          const uint64_t *counts, const double *values, double *out_patterns);

/* ------------------------------------------------------------------------
 * Marginal ancestral states and site rates at a chosen root (Yang, Kumar & Nei 1995; Yang 1995's
 * empirical Bayes site rates).  NEW relative to the reference, which has no ancestral
 * reconstruction: it extends the traversal made with corax_update_clvs at src/model.cpp:402 by the
 * complementary pre-order pass.  Under a non-reversible model the answers depend on the root.
 *
 * The tree is rooted as the operation list `ops` says (rdamd_tree_generate_operations: post-order,
 * the last operation the root's).  For site s and rate category r:
 *   L_v[i]  CLV of node v as rdamd_update_clvs leaves it (a tip's: its 0/1 code vector)
 *   P_v     P-matrix of the branch above v, rows = parent state
 *   pi      frequencies of the rate's frequency set freqs_indices[r];  w_r, rate_r: category weight, rate
 *   U_v[j]  = P(data outside the subtree of v, state j at v):
 *             U_root[i] = pi_i;  for an operation with parent u and children a, b
 *             U_a[j] = sum_i U_u[i] (P_b L_b)[i] P_a[i][j]      (U_b: a and b swapped)
 *   post[v][s][j] = sum_r w_r U_v[s][r][j] L_v[s][r][j]         normalised over j
 *   cat[s][r]     = w_r sum_i pi_i L_root[s][r][i]               normalised over r
 *   mean_rate[s]  = sum_r cat[s][r] rate_r
 * The outer vectors follow the 2^256 rule of the CLVs (a site below 2^-256 in every rate is
 * multiplied by 2^256); the rule acts per site, so neither these counts nor the CLVs' scalers
 * appear in the normalised outputs.  Pattern weights play no part (a pattern of weight 0 gets
 * posteriors like any other); an all-gap column gets the prior carried down the tree.
 * ---------------------------------------------------------------------- */
/* post_out[n_ops][sites][states]: the posterior of every inner node.  Node 0 is the root, node k
 * the parent of operation n_ops - 1 - k (the list read backwards: every node after its parent);
 * binary partitions keep their 2-state shape.  Precondition: rdamd_update_prob_matrices and
 * rdamd_update_clvs on exactly this list -- the inner CLVs are read as that traversal left them,
 * nothing in the partition is written.  One launch for the whole list: 4-state and binary
 * partitions, a (site, rate) pair per lane with 1, 2, 4 or 8 rate categories, a plain kernel for any
 * other count.  Refused (error 63, nothing launched): 20-state partitions, partitions with
 * RDAMD_ATTRIB_SPARSE_CLVS.  Error 64: the list is not a complete post-order traversal of one
 * tree ending in the root operation (the rule of rdamd_schedule_create). */
int rdamd_marginal_ancestral(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                             const unsigned int *freqs_indices, double *post_out);
/* The nodes in that order (host only): node_clv[n_ops]; node_parent[n_ops], a node index, -1 for
 * the root; node_children[n_ops][2], CLV indices (below the smallest parent index: a tip, named by
 * rdamd_tree_tip_label).  Any pointer may be NULL. */
int rdamd_marginal_ancestral_nodes(const rdamd_operation_t *ops, unsigned int n_ops, unsigned int *node_clv,
                                   int *node_parent, unsigned int *node_children);
/* workspace of the pass for this list, in CLV-sized slots: the most outer vectors that wait at
 * once for an operation that is not the next one (~0u: error 64) */
unsigned int rdamd_marginal_ancestral_workspace_slots(const rdamd_operation_t *ops, unsigned int n_ops,
                                                      unsigned int tips);
/* cat_out[sites][R] and mean_rate_out[sites] from the root CLV `clv_index` (any state count except
 * the 20-state matrix-core layout, error 63).  scaler_index is checked for range only: per-site
 * scalers cancel.  Either output may be NULL. */
int rdamd_site_rate_posteriors(rdamd_partition_t *p, unsigned int clv_index, int scaler_index,
                               const unsigned int *freqs_indices, double *cat_out, double *mean_rate_out);
/* device time of the pre-order launch of this thread's last rdamd_marginal_ancestral call,
 * milliseconds between two HIP events (0 after a failed call); for measurements */
double rdamd_ancestral_last_ms(void);
/* All of it for one root of a model.  Parameters in the checkpoint's layout exactly as
 * rdamd_model_site_lnls takes them for one root (counts[n_partitions][4]; counts = values = NULL:
 * the model's current parameters).  Outputs, any of which may be NULL: *n_nodes = inner nodes of
 * the rooted tree (tips - 1); node_clv / node_parent / node_children as above;
 * post_out[n_nodes][P_total][states] and mean_rate_out[P_total] with the patterns of all
 * partitions concatenated in partition order (rdamd_model_site_patterns); cat_out: the
 * partitions' [patterns][R] blocks back to back, each with its own category count
 * (rdamd_model_partition_shape).  The model's parameters, its rooting
 * and the conditional likelihoods of that rooting are as before when the call returns.
 * Refused (error 61) for a model that sums over a site group; a partition whose shape
 * rdamd_marginal_ancestral refuses fails the call and is named in the message. */
/* patterns, alignment columns and rate categories of partition p (any pointer may be NULL) */
int rdamd_model_partition_shape(const rdamd_model_t *m, unsigned int p, unsigned int *patterns,
                                unsigned int *columns, unsigned int *rate_cats);
int rdamd_model_ancestral(rdamd_model_t *m, const rdamd_root_location_t *rl,
                          const uint64_t *counts, const double *values, unsigned int *n_nodes,
                          unsigned int *node_clv, int *node_parent, unsigned int *node_children,
                          double *post_out, double *cat_out, double *mean_rate_out);

/* ------------------------------------------------------------------------
 * Ancestral sequences at a chosen root: the likeliest state of every inner node and alignment
 * column with its posterior probability -- for DNA, binary AND protein data.  NEW relative to the
 * reference, which reconstructs nothing: like the section above it extends the traversal made with
 * corax_update_clvs at src/model.cpp:402 by the complementary pre-order pass, here also for the
 * 20-state partitions that keep their CLVs in the matrix-core operand layout (20 states, up to 8
 * rate categories), where the pass runs on v_mfma_f64_4x4x4_4b_f64 like the traversal itself.
 *
 * Definitions (L, P, pi, U, post) and the 2^256 rule are those of "Marginal ancestral states"
 * above;  state[v][s] = the smallest j among the largest post[v][s][j],  prob[v][s] = that
 * posterior: exactly argmax and max of the table, bit for bit.  Equal inputs give equal bits.
 * ---------------------------------------------------------------------- */
/* state_out[n_ops][sites] (index of the likeliest state, the smallest among equals), prob_out[n_ops][sites],
 * post_out[n_ops][sites][states]; any may be NULL.  Nodes as rdamd_marginal_ancestral_nodes orders them.
 * Precondition as for rdamd_marginal_ancestral: rdamd_update_prob_matrices and rdamd_update_clvs on
 * exactly this list; nothing in the partition is written.  4-state and binary partitions run
 * rdamd_marginal_ancestral's launch (post_out has its bits), matrix-core 20-state partitions a
 * walk of their own; the posterior table stays on the device unless post_out is given (20 states:
 * five times the 4-state table).  Refused (error 63, nothing launched, the shape named):
 * partitions with RDAMD_ATTRIB_SPARSE_CLVS, state counts other than 2, 4 and 20, 20 states with
 * more than 8 rate categories (the plain CLV layout).  Errors 64, 10 and 7 as for
 * rdamd_marginal_ancestral. */
int rdamd_ancestral_sequences(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                              const unsigned int *freqs_indices, uint8_t *state_out, double *prob_out,
                              double *post_out);
/* device time of the launches (walk and arg-max) of this thread's last rdamd_ancestral_sequences
 * call, milliseconds between two HIP events (0 after a failed call); for measurements */
double rdamd_ancestral_sequences_last_ms(void);
/* The same for one root of a model, as rdamd_model_ancestral: parameters in the checkpoint's layout
 * (counts = values = NULL: the model's own), the patterns of all partitions concatenated in
 * partition order -- state_out[n_nodes][P_total], prob_out[n_nodes][P_total],
 * post_out[n_nodes][P_total][states] -- and the model's parameters, its rooting and the conditional
 * likelihoods of that rooting as before when the call returns.  Any output may be NULL.  Refused:
 * a model that sums over a site group (error 61); partitions of different state counts in one
 * model (post_out has one `states`); a partition whose shape rdamd_ancestral_sequences refuses fails
 * the call and is named in the message. */
int rdamd_model_ancestral_sequences(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts,
                                    const double *values, unsigned int *n_nodes, unsigned int *node_clv,
                                    int *node_parent, unsigned int *node_children, uint8_t *state_out,
                                    double *prob_out, double *post_out);

/* ------------------------------------------------------------------------
 * Analytic branch-length derivatives and optimised lengths at a chosen root.  NEW relative to the
 * reference, whose only derivative is the forward difference of compute_dlh (one parameter: the
 * root's position).
 *
 * The tree is rooted as the post-order list `ops` says, under the rules of
 * rdamd_marginal_ancestral.  Nodes are ordered as rdamd_marginal_ancestral_nodes orders them.
 * Branch (k, c) is the branch above child c in {0, 1} of node k.  Its length t is what
 * rdamd_update_prob_matrices was given for that child's matrix index.
 *
 * For site s, rate category r with rate rho_r, weight w_r and rate matrix Q_r:
 *   Q_r   the rate matrix of the set params_indices[r], normalised, as the P-matrix step uses it
 *   L, P, U and pi are as in the ancestral section above
 *   t[i] = U_u[i] (P_b L_b)[i]       the parent's outer vector masked by the sibling
 *   y = P_a L_a,  z = Q_r y,  z2 = Q_r z
 *   f0(s) = sum_r w_r t.y            the site likelihood, the same on every branch up to the
 *                                    per-site scaling factors
 *   f1(s) = sum_r w_r rho_r t.z
 *   f2(s) = sum_r w_r rho_r^2 t.z2
 *   d1[k][c] = sum_s weight_s f1/f0                        = d lnL / dt
 *   d2[k][c] = sum_s weight_s (f2/f0 - (f1/f0)^2)          = d2 lnL / dt2
 * The 2^256 rule on U and the CLVs' scalers act per site over all rates, so they cancel in f1/f0
 * and f2/f0.  No scaler is read.  Tip children have branches too.
 *
 * Identity: with the root on a branch of length T at ratio alpha,
 *   d lnL / d alpha = T (d1 of the root child that gets alpha T - d1 of the other).
 * ---------------------------------------------------------------------- */
/* d1_out[n_ops][2] and d2_out[n_ops][2] (d2_out may be NULL).  Precondition, as for
 * rdamd_marginal_ancestral: rdamd_update_prob_matrices with these params_indices and
 * rdamd_update_clvs on exactly this list; nothing in the partition is written.  One launch of the
 * pre-order program for the whole list (a (site, rate) pair per lane with 1, 2, 4 or 8 rate
 * categories, a plain kernel for any other count) and one small launch that adds the partial sums.
 * The sums over sites are made in one fixed order without floating-point atomics: two calls with
 * the same inputs return the same bits.  Zero sites: zeros and success.  Refused as there: error 63
 * for 20-state partitions and RDAMD_ATTRIB_SPARSE_CLVS, error 64 for a list that is not a complete
 * post-order traversal ending in the root operation, 10 / 7 for indices out of range.  Error 65: a
 * site's likelihood f0 is 0 or not finite; the message says how many sites, nothing is returned. */
int rdamd_branch_derivatives(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                             const unsigned int *params_indices, const unsigned int *freqs_indices,
                             double *d1_out, double *d2_out);
/* device time of the two launches of this thread's last rdamd_branch_derivatives or
 * rdamd_branch_length_derivatives call, milliseconds between two HIP events (0 after a failed
 * call); for measurements */
double rdamd_branch_last_ms(void);
/* The same derivatives -- for DNA, binary AND protein data.  Arguments, outputs, precondition and the
 * definitions above are those of rdamd_branch_derivatives.  4-state and binary partitions run
 * rdamd_branch_derivatives' two launches (d1_out and d2_out have its bits).  Matrix-core 20-state
 * partitions (20 states, up to 8 rate categories) run the walk of rdamd_ancestral_sequences with a
 * derivative consumer: a wave is 16 sites of one rate category, z = Q_r y and z2 = Q_r z are 25
 * v_mfma_f64_4x4x4_4b_f64 each, their A operand a matrix-core copy of Q_r that the call builds on the
 * host and uploads; with d2_out NULL z2 is not formed.  The sums are made in one fixed order without
 * floating-point atomics -- the states of a site, the rate categories in their order, the 16 sites
 * of a tile, then the tiles by increasing number in a second small launch --: two calls with the
 * same inputs return the same bits.  Tip children have branches here too.  Zero sites: zeros and
 * success.  Refused (error 63, nothing launched, the shape named): partitions with
 * RDAMD_ATTRIB_SPARSE_CLVS, state counts other than 2, 4 and 20, 20 states with more than 8 rate
 * categories (the plain CLV layout).  Errors 64, 10, 7 and 65 as for rdamd_branch_derivatives.
 * rdamd_branch_last_ms reports this call's two launches. */
int rdamd_branch_length_derivatives(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                                    const unsigned int *params_indices, const unsigned int *freqs_indices,
                                    double *d1_out, double *d2_out);
/* The same for one root of a model.  Parameters in the checkpoint's layout exactly as
 * rdamd_model_ancestral takes them.  Outputs, any of which may be NULL: *n_nodes, node_clv,
 * node_parent, node_children as there; lengths_out[n][2]: the schedule's current length of branch
 * (k, c); d1_out[n][2], d2_out[n][2]: summed over partitions in partition order; *lnl_out: the
 * log-likelihood at that root.  The model's parameters, its rooting and the conditional
 * likelihoods of that rooting are as before when the call returns.  Every partition goes through
 * rdamd_branch_length_derivatives: DNA, binary and protein models are served, and a partition whose
 * shape that call refuses fails this one and is named in the message.  Refused (error 61) for a model
 * that sums over a site group. */
int rdamd_model_branch_derivatives(rdamd_model_t *m, const rdamd_root_location_t *rl,
                                   const uint64_t *counts, const double *values, unsigned int *n_nodes,
                                   unsigned int *node_clv, int *node_parent, unsigned int *node_children,
                                   double *lengths_out, double *d1_out, double *d2_out, double *lnl_out);
/* Maximises lnL over all 2n - 2 branch lengths of the tree rooted at rl, in [min_len, max_len], at
 * fixed model parameters (counts / values as above) and fixed root.  Nothing is applied to the
 * model or its tree: the lengths are an output (lengths_out[n][2], nodes as above), with d1_out /
 * d2_out at those lengths; on return the model is bit for bit what it was.  Each evaluation at
 * lengths x is rdamd_update_prob_matrices on the schedule's matrix indices with x, a materialising
 * traversal, the root lnL, and rdamd_branch_length_derivatives per partition.
 * The method is a projected L-BFGS (memory 8) whose initial metric is the diagonal Newton one:
 * a branch is free unless it sits at a bound with the gradient pointing out; curvature
 * c_b = -d2_b where d2_b < 0, else |d1_b| / max(x_b, min_len) (1 where that is 0); it stops with
 * *converged = 1 when the predicted gain sum_free d1_b^2 / (2 c_b) is below atol, with
 * *converged = 0 after max_iters iterations or when no step of a backtracking line search
 * (Armijo, 1e-4, at most 40 halvings) is accepted.  *iterations, *evaluations: counts;
 * *lnl_before, *lnl_after: lnL at the schedule's lengths and at lengths_out.  Any output may be
 * NULL.  Refused (error 61) for a model that sums over a site group. */
int rdamd_model_optimize_branch_lengths(rdamd_model_t *m, const rdamd_root_location_t *rl,
                                        const uint64_t *counts, const double *values, double min_len,
                                        double max_len, double atol, unsigned int max_iters,
                                        double *lengths_out, double *d1_out, double *d2_out,
                                        double *lnl_before, double *lnl_after, unsigned int *iterations,
                                        unsigned int *evaluations, int *converged);

/* ------------------------------------------------------------------------
 * Branch pair sums: the derivative of lnL in every entry of every P-matrix, and from them the
 * exact gradient of lnL in the model parameters.  NEW relative to the reference, which takes its
 * gradient as 1 + n one-sided differences.
 *
 * Notation of the two sections above.  Branch (k, c) lies above child a of node k and has
 * sibling b.  For site s and rate category r, with K the caller's state count:
 *   t_r[i]   = U_u[i] (P_b L_b)[i]
 *   f0(s)    = sum_r w_r t_r . (P_a L_a,r)                 (per-site scalings cancel below)
 *   N[k][c][r][i][j] = sum_s weight_s w_r t_r[i] L_a,r[j] / f0(s)      (a tip's L: its 0/1 code vector)
 *   froot(s) = sum_r w_r pi^(r) . L_root,r                 pi^(r): the set freqs_indices[r]
 *   M[r][i]  = sum_s weight_s w_r L_root,r[i] / froot(s)
 *   W[r]     = sum_s weight_s (pi^(r) . L_root,r) / froot(s)
 * With every other quantity held fixed:
 *   d lnL / d P_(k,c),r[i][j] = N[k][c][r][i][j]
 *   d lnL / d pi^(m)_i at the root = sum over r with freqs_indices[r] = m of M[r][i]
 *   d lnL / d w_r = W[r]
 * Identities:
 *   I1  sum_{r,i,j} N[k][c][r][i][j] P_(k,c),r[i][j] = sum_s weight_s           for every branch
 *   I2  sum_r rho_r sum_{i,j} N[k][c][r][i][j] (Q_r P_(k,c),r)[i][j] = d1[k][c]   of rdamd_branch_derivatives
 *   I3  sum_r sum_i pi^(r)_i M[r][i] = sum_s weight_s   and   sum_r w_r W[r] = sum_s weight_s
 * ---------------------------------------------------------------------- */
/* pair_out[n_ops][2][R][K][K], nodes as rdamd_marginal_ancestral_nodes orders them; root_out[R][K]
 * and cat_out[R] may be NULL.  Preconditions and refusals are those of rdamd_branch_derivatives
 * (errors 63, 64, 65, 10 / 7); error 67: pair_out is NULL.  Zero sites: zeros and success.  Nothing
 * in the partition is written.  4-state and binary partitions; binary ones get the [2][2] / [2]
 * blocks of their own states.  Every term is non-negative.  The sums over sites are made in one
 * fixed order without floating-point atomics: inside a wave, the four waves of a workgroup in wave
 * order, one partial per (workgroup, entry), and a second kernel that continues each entry's running
 * sum by increasing workgroup.  The walk runs in passes over contiguous ranges of whole workgroups
 * so that the partials of one pass take at most workspace_bytes (0: 256 MiB; never less than one
 * workgroup per pass); the result is bit for bit independent of the number of passes.  The sums read
 * the CLVs and outer vectors as they are kept: one power-of-two scaling per site for all rate
 * categories, so a category's entry more than about 2^-510 below its site's largest contributes a
 * denormal or zero. */
int rdamd_branch_pair_sums(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                           const unsigned int *freqs_indices, size_t workspace_bytes, double *pair_out,
                           double *root_out, double *cat_out);
/* The same sums for every shape the pre-order walk takes: the same arguments, outputs and errors.
 * 4-state and binary partitions run the launches of rdamd_branch_pair_sums and return its bits.
 * 20-state partitions in the matrix-core CLV layout (up to 8 rate categories) run the pair-sum
 * consumer of the 20-state walk (csrc/kernels_preorder_k20.hip): a wave is (16 sites, one rate), and
 * its sum over the 16 sites is a 20 x 16 by 16 x 20 product, 25 FP64 MFMAs whose four blocks are the
 * four quads of sites.  Order of a sum: the MFMA's own accumulation over the four sites of a quad;
 * the four quads by lanes 4 apart, then 8 apart; one partial per (tile of 16 sites, entry); a second
 * kernel that continues each entry's running sum by increasing tile.  M and W: each wave its own
 * rate, froot and f0 added over the rates in rate order, the 16 sites of a tile by a butterfly (lanes
 * 1, 2, 4, 8 apart), then the tiles likewise.  No floating-point atomics.  The walk runs in passes
 * over contiguous ranges of whole tiles so that the partials of one pass take at most
 * workspace_bytes (0: 1 GiB for 20 states, 256 MiB otherwise; never less than one tile per pass);
 * the result is bit for bit independent of the number of passes.  The sums inherit the 2^-510 limit
 * stated above.  Error 63, the shape named in the message: RDAMD_ATTRIB_SPARSE_CLVS, 20 states with
 * more than 8 rate categories (the plain CLV layout), any state count other than 2, 4 and 20. */
int rdamd_pair_sums(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                    const unsigned int *freqs_indices, size_t workspace_bytes, double *pair_out,
                    double *root_out, double *cat_out);
/* device time of the launches of this thread's last rdamd_branch_pair_sums or rdamd_pair_sums call,
 * milliseconds between two HIP events (0 after a failed call); for measurements */
double rdamd_pair_sums_last_ms(void);
/* The exact gradient from the pair sums: plain host code, a pure function of its arguments, no
 * device needed.  states K in {2, ..., 64}; pair[n_ops][2][R][K][K], root[R][K], cat[R] as above;
 * lengths[n_ops][2]: the length of branch (k, c); subst[rate_matrices][K K - K]: off-diagonal
 * exchangeabilities row-major; freqs[rate_matrices][K]: K independent numbers that enter Q and the
 * root exactly as given (no renormalisation, as rdamd_set_frequencies takes them); params_indices,
 * freqs_indices, rates, weights: per rate category.
 *   Q_m = raw / mu,  raw_ij = s_ij pi_j (i != j), zero row sums,  mu = -sum_i pi_i raw_ii
 *   G_Q[m] = sum_branches sum_{r: params_indices[r] = m} rho_r tau F((rho_r tau Q_m)^T, N[branch][r])
 *   F(X, E) = integral_0^1 exp(xX) E exp((1 - x)X) dx = the top-right block of exp([[X, E], [0, X]])
 *   d lnL / d rho_r = sum_branches tau sum_ij N[branch][r][i][j] (Q P)[i][j]
 *                   = sum_branches tau sum_ij (F((rho_r tau Q)^T, N[branch][r]))_ij Q_ij     (the same adjoint)
 * F by scaling and squaring on the pair (exp, F): Taylor terms D_k = (X D_{k-1} + E X^{k-1}/(k-1)!)/k,
 * squaring (P, F) -> (P P, P F + F P).  Then the chain rule through Q = raw / mu with all K K
 * entries of G_Q free; the frequencies of set m get their part through Q (with the pi of
 * params_indices' set m) and, as set m of freqs_indices, the root term M.
 * Outputs (any may be NULL): d_subst[rate_matrices][K K - K], d_freqs[rate_matrices][K], d_rates[R],
 * d_weights[R] (= cat).  Returns RDAMD_SUCCESS, or RDAMD_FAILURE with error 64 for a NULL input or
 * a state count out of range, 7 for an index >= rate_matrices. */
int rdamd_gradient_from_pair_sums(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices,
                                  unsigned int n_ops, const double *pair, const double *root, const double *cat,
                                  const double *lengths, const double *subst, const double *freqs,
                                  const unsigned int *params_indices, const unsigned int *freqs_indices,
                                  const double *rates, const double *weights, double *d_subst, double *d_freqs,
                                  double *d_rates, double *d_weights);

/* ------------------------------------------------------------------------
 * The adjoints of the pair sums: the one expensive step that the gradient and the typed counts share,
 * on the host or -- for 20 states -- on the matrix cores.  NEW relative to the reference.
 *   adjoint[k][c][r] = F_r = F((rho_r tau Q_m)^T, N[k][c][r]),  m = params_indices[r], tau = lengths[k][c]
 * with Q_m and F as rdamd_gradient_from_pair_sums defines them.  Every F_r is computed as
 *   s, 2^-s: ||X||_1 halved until it is at most 1/4 (at most 60 times), X = (rho_r tau Q_m)^T;
 *   18 Taylor terms on the pair (exp, F) of X / 2^s and E / 2^s;  s squarings (P, F) -> (P P, P F + F P).
 * rdamd_gradient_from_pair_sums is rdamd_pair_sum_adjoints on the host followed by
 * rdamd_gradient_from_adjoints, and rdamd_substitution_counts_from_pair_sums likewise: same bits.
 * The device route (csrc/kernels_block_exp.hip) runs one (branch, rate) problem per wave with the
 * host's s, the same recurrences (Taylor terms as left products: T_k = X T_{k-1} / k where the host
 * forms T_{k-1} X) and every 20 x 20 x 20 product as 20 v_mfma_f64_16x16x4_f64; it differs from the
 * host route only in the order inside dot products of length 20.  The bits of one problem depend on
 * nothing but that problem's inputs; two calls return the same bits.
 * ---------------------------------------------------------------------- */
#define RDAMD_ADJOINTS_AUTO 0   /* the device when states = 20 and a device is present, else the host */
#define RDAMD_ADJOINTS_HOST 1   /* 2 .. 64 states; the bits of rdamd_gradient_from_pair_sums' own block exponentials */
#define RDAMD_ADJOINTS_DEVICE 2 /* 20 states on the current device */
/* pair[n_ops][2][R][K][K], lengths[n_ops][2], subst[rate_matrices][K K - K], freqs[rate_matrices][K],
 * params_indices[R], rates[R] as rdamd_gradient_from_pair_sums takes them; adjoint_out[n_ops][2][R][K][K].
 * Host pointers in and out, no partition: the device route owns its device memory, its stream and
 * its events and leaves no state behind.  Errors, before anything runs: 64 for a NULL argument, a
 * state count outside 2 .. 64, no rate category or rate matrix, a length or rate that is negative or
 * not finite, or an unknown `where`; 7 for an index >= rate_matrices; 63 for RDAMD_ADJOINTS_DEVICE
 * with a state count other than 20 or with no device present (the message says which).  Zero
 * operations: success, nothing written. */
int rdamd_pair_sum_adjoints(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices, unsigned int n_ops,
                            const double *pair, const double *lengths, const double *subst, const double *freqs,
                            const unsigned int *params_indices, const double *rates, int where, double *adjoint_out);
/* device time of the kernel of this thread's last rdamd_pair_sum_adjoints call, milliseconds between
 * two HIP events (0 after a failed call and after one that took the host route); for measurements */
double rdamd_pair_sum_adjoints_last_ms(void);
/* rdamd_gradient_from_pair_sums' assembly alone: the arguments, outputs and errors of that function
 * with adjoint[n_ops][2][R][K][K] (rdamd_pair_sum_adjoints) in place of pair.  Host only and pure. */
int rdamd_gradient_from_adjoints(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices,
                                 unsigned int n_ops, const double *adjoint, const double *root, const double *cat,
                                 const double *lengths, const double *subst, const double *freqs,
                                 const unsigned int *params_indices, const unsigned int *freqs_indices,
                                 const double *rates, const double *weights, double *d_subst, double *d_freqs,
                                 double *d_rates, double *d_weights);

/* The exact gradient of lnL at one root of a model.  counts / values: the parameters in the
 * checkpoint's layout exactly as rdamd_model_branch_derivatives takes them, here required (the
 * model does not keep the optimiser's variables).  grad_out has the layout of values and holds the
 * gradient in the variables L-BFGS-B sees in the parameter steps of the search:
 *   the substitution rates as given;
 *   the unnormalised frequency vector x, pi = x / sum x:  g_x = (g_pi - pi . g_pi) / sum x;
 *   alpha through rdamd_compute_gamma_cats(alpha, R, rates, RDAMD_GAMMA_RATES_MEDIAN): the Jacobian
 *     d rho / d alpha is a CENTRAL DIFFERENCE of that host function with step 1e-6 max(1, alpha);
 *   the unnormalised category weights u of a FREE partition, w = u / sum u; a FREE partition's rates
 *     are inert, so its alpha entry is 0; the weight entries of any other partition are 0.
 * Each evaluation is rdamd_update_prob_matrices, a materialising traversal, the root lnL (*lnl_out,
 * may be NULL), rdamd_pair_sums per partition, rdamd_pair_sum_adjoints (RDAMD_ADJOINTS_AUTO: a
 * protein partition's on the device, every other on the host with the bits of
 * rdamd_gradient_from_pair_sums) and rdamd_gradient_from_adjoints: DNA, binary and
 * protein models are served (a protein partition: 380 rates, 20 frequencies and alpha from one pass
 * of the walk, where a one-sided difference takes 381 evaluations).  The model's
 * parameters, its rooting and the conditional likelihoods of that rooting are as before when the
 * call returns.  Refused (error 61) for a model that sums over a site group; a partition whose shape
 * rdamd_pair_sums refuses fails the call and is named in the message. */
int rdamd_model_gradient(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts,
                         const double *values, double *grad_out, double *lnl_out);

/* ------------------------------------------------------------------------
 * Substitutions mapped onto branches: per site, the joint posterior of a branch's two ends and the
 * expected number of substitutions on it; per branch, the expected number of substitutions of every
 * type and the expected time spent in every state.  NEW relative to the reference.  Under a rooted
 * non-reversible model the direction of a substitution is identified; under a reversible one
 * i -> j and j -> i on a branch cannot be told apart.
 *
 * Notation of the three sections above.  The tree is rooted as the operation list says.  Branch
 * (k, c) lies above child a = child c of node k, has sibling b and length tau.  For rate category
 * r: rate rho_r, weight w_r, Q_r = Q[params_indices[r]], X_r = rho_r tau Q_r, P_r = exp(X_r);
 *   t_r[i] = U_u[i] (P_b L_b)[i]          L_r = L_a,r (a tip's: its 0/1 code vector)
 *   f0(s)  = sum_r w_r t_r . (P_r L_r)    weight_s: the pattern weight
 * Per site, for every branch, tip branches included:
 *   J_s[i][j] = sum_r w_r t_r[i] P_r[i][j] L_r[j] / f0(s)   the posterior probability that the branch
 *               starts in state i and ends in state j; sum_ij J_s = 1
 *   change_s  = sum_{i != j} J_s[i][j]
 *   top pair: the pair i != j with the largest J_s[i][j], as the code i K + j (K: the caller's state
 *               count); the smallest code wins an exact tie.  top_prob_s: that largest value
 *   n_s       = sum_r w_r t_r^T C_r L_r / f0(s),  C_r = F(X_r, offdiag(X_r)): the expected number of
 *               substitutions at the site on the branch, multiple hits included
 *   F(X, E) = integral_0^1 exp(xX) E exp((1 - x)X) dx, as in rdamd_gradient_from_pair_sums
 * The 2^256 rule on U and the CLVs' scalers act per site over all rates and cancel.  No scaler is
 * read.
 * Per branch, from the pair sums N of rdamd_branch_pair_sums, with F_r = F(X_r^T, N[k][c][r]):
 *   E[k][c][i][j] = sum_r X_r[i][j] F_r[i][j], i != j: the expected number of i -> j substitutions
 *               on the branch over the whole alignment
 *   D[k][c][i]    = tau sum_r F_r[i][i]: the expected time spent in state i, in branch-length units
 * Identities:
 *   A  sum_s weight_s n_s = sum_{i != j} E[i][j]
 *   B  sum_s weight_s J_s[i][j] = sum_r N_r[i][j] P_r[i][j]
 *   C  tau d1 = sum_{i != j} E[i][j] + sum_r sum_i X_r[i][i] F_r[i][i],  d1 of rdamd_branch_derivatives
 *   D  sum_i D[i] = tau sum_s weight_s
 * ---------------------------------------------------------------------- */
/* change_out, count_out, top_prob_out[n_ops][2][sites], top_pair_out[n_ops][2][sites] (bytes) and
 * joint_out[n_ops][2][sites][K][K], nodes as rdamd_marginal_ancestral_nodes orders them; each may be
 * NULL and is then not written.  lengths[n_ops][2]: the length of branch (k, c).  THESE MUST BE THE
 * LENGTHS THE P-MATRICES OF THE LIST WERE LAST BUILT WITH (rdamd_update_prob_matrices, with these
 * params_indices): the partition does not keep them, and the count matrices C_r are made from them on
 * the host (one block exponential per branch and rate category) and uploaded.  Otherwise the
 * preconditions and refusals of rdamd_branch_derivatives: error 63 for 20-state partitions and
 * RDAMD_ATTRIB_SPARSE_CLVS, 64 for a NULL input, a list that is not a complete post-order traversal
 * ending in the root operation or a length that is negative or not finite, 10 / 7 for indices out
 * of range, 65 when a site's f0 is 0 or not finite (nothing is returned).  4-state and binary
 * partitions; binary ones get [2][2] joints and codes 2 i + j.  One launch of the pre-order program;
 * nothing is summed over sites, so there is no second launch and two calls with the same inputs
 * return the same bits.  Nothing in the partition is written.  Zero sites: success. */
int rdamd_branch_substitutions(rdamd_partition_t *p, const rdamd_operation_t *ops, unsigned int n_ops,
                               const unsigned int *params_indices, const unsigned int *freqs_indices,
                               const double *lengths, double *change_out, double *count_out,
                               unsigned char *top_pair_out, double *top_prob_out, double *joint_out);
/* device time of the launch of this thread's last rdamd_branch_substitutions call, milliseconds
 * between two HIP events (0 after a failed call); for measurements */
double rdamd_branch_substitutions_last_ms(void);
/* E and D from the pair sums: plain host code, a pure function of its arguments, no device needed.
 * states K in {2, ..., 64}; pair[n_ops][2][R][K][K], lengths[n_ops][2], subst[rate_matrices][K K - K],
 * freqs[rate_matrices][K], params_indices[R], rates[R] as rdamd_gradient_from_pair_sums takes them.
 * typed_out[n_ops][2][K][K]: the off-diagonal entries are E, the diagonal entries are D.  Returns
 * RDAMD_SUCCESS, or RDAMD_FAILURE with error 64 for a NULL argument, a state count out of range or
 * a length that is negative or not finite, 7 for an index >= rate_matrices. */
int rdamd_substitution_counts_from_pair_sums(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices,
                                             unsigned int n_ops, const double *pair, const double *lengths,
                                             const double *subst, const double *freqs,
                                             const unsigned int *params_indices, const double *rates,
                                             double *typed_out);
/* rdamd_substitution_counts_from_pair_sums' assembly alone: the arguments, output and errors of that
 * function with adjoint[n_ops][2][R][K][K] (rdamd_pair_sum_adjoints) in place of pair.  Host only
 * and pure. */
int rdamd_substitution_counts_from_adjoints(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices,
                                            unsigned int n_ops, const double *adjoint, const double *lengths,
                                            const double *subst, const double *freqs,
                                            const unsigned int *params_indices, const double *rates,
                                            double *typed_out);
/* All of it for one root of a model.  counts / values: the parameters in the checkpoint's layout
 * exactly as rdamd_model_gradient takes them (required).  Outputs, any of which may be NULL:
 * *n_nodes, node_clv, node_parent, node_children, lengths_out[n][2] as
 * rdamd_model_branch_derivatives gives them; typed_out: one [n][2][K][K] block per partition, back
 * to back in partition order, K the partition's state count; change_out, count_out,
 * top_prob_out[n][2][P_total] and top_pair_out[n][2][P_total] (bytes) with the patterns of all
 * partitions concatenated in partition order (rdamd_model_site_patterns); *lnl_out: the
 * log-likelihood at that root.  Each partition: rdamd_update_prob_matrices, a materialising
 * traversal, rdamd_pair_sums, rdamd_pair_sum_adjoints (RDAMD_ADJOINTS_AUTO),
 * rdamd_substitution_counts_from_adjoints and -- unless change_out,
 * count_out, top_pair_out and top_prob_out are all NULL -- rdamd_branch_substitutions.  With those
 * four NULL the call serves every shape rdamd_pair_sums takes, protein models among them: typed_out
 * then holds the expected i -> j counts over 20 x 20 amino-acid pairs and the dwell times.  The
 * per-site outputs are for 4-state and binary partitions.  The model's parameters, its rooting and
 * the conditional likelihoods of that rooting are as before when the call returns.  Refused (error
 * 61) for a model that sums over a site group; a partition whose shape rdamd_pair_sums or (per-site
 * outputs) rdamd_branch_substitutions refuses fails the call and is named in the message. */
int rdamd_model_substitutions(rdamd_model_t *m, const rdamd_root_location_t *rl, const uint64_t *counts,
                              const double *values, unsigned int *n_nodes, unsigned int *node_clv, int *node_parent,
                              unsigned int *node_children, double *lengths_out, double *typed_out, double *change_out,
                              double *count_out, unsigned char *top_pair_out, double *top_prob_out, double *lnl_out);

/* Column that draw d (0 <= d < N) of bootstrap replicate b resamples, N < 2^32 columns.
 * Stateless and counter-based (all arithmetic mod 2^64):
 *   sm(x):  x += 0x9E3779B97F4A7C15; z = x;
 *           z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *           z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *           return z ^ (z >> 31)
 *   key = sm(seed ^ sm(b));  u = sm(key + d);  column = ((u >> 32) * N) >> 32
 * Replicate b does not depend on the number of replicates, and a process that holds a block of
 * the columns can draw the same GLOBAL columns.  Plain host code: no device needed. */
uint32_t rdamd_rell_column(uint64_t seed, uint64_t b, uint64_t d, uint64_t N);
/* RELL bootstrap of n_rows rows (candidate roots) of site log-likelihoods, on the current device.
 * site_lnl[n_rows][n_patterns] (host) holds UNWEIGHTED pattern lnLs; pattern p stands for
 * pattern_weights[p] consecutive columns of the N = sum(pattern_weights) < 2^32 columns, so
 * col2pat[c] is the pattern whose column range holds c (a pattern of weight 0 is never drawn).
 *   sums[b][i] = sum over d in [0, N) of site_lnl[i][col2pat[rdamd_rell_column(seed, b, d, N)]]
 *   bp[i]      = (replicates whose largest sum is row i's; ties go to the LOWEST i) / n_replicates
 *   elw[i]     = mean over b of exp(sums[b][i] - m_b) / sum_j exp(sums[b][j] - m_b),
 *                m_b = the replicate's largest sum (expected likelihood weight, Strimmer & Rambaut 2002)
 * The additions of one (b, i) are made in ONE order that depends on N alone -- not on the row, on
 * n_rows, on n_replicates or on the launch shape: draw d goes to partial sum d mod 8; each partial
 * sum adds its draws by increasing d; the eight are combined as ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)).
 * Equal rows therefore get equal bits, the first B1 replicates of a longer run are the B1-replicate
 * run's, and a repeated call returns the same bits.
 * Host pointers in and out: bp[n_rows], elw[n_rows], sums[n_replicates][n_rows] (may be NULL).
 * The call owns its device memory and leaves no state behind.  Error 62: n_rows, n_patterns or
 * n_replicates is 0, N is 0 or >= 2^32, or a pointer is missing -- nothing is launched. */
int rdamd_rell_bootstrap(const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
                         const unsigned int *pattern_weights, unsigned int n_replicates,
                         uint64_t seed, double *bp, double *elw, double *sums);
/* device time of the resampling kernel alone in this thread's last rdamd_rell_bootstrap call,
 * milliseconds between two HIP events (0 after a failed call); for measurements */
double rdamd_rell_last_resample_ms(void);

/* KH, SH and weighted-SH tests of the rows (candidate roots), made on the device from the
 * resampled sums of rdamd_rell_bootstrap (Kishino & Hasegawa 1989; Shimodaira & Hasegawa 1999).
 * The inputs are those of rdamd_rell_bootstrap. sums[b][i] is exactly that function's: same
 * draws, same order of additions, same bits. With B replicates and n rows:
 *
 * - Observed lnL. lnl[i] = sum_p pattern_weights[p] * site_lnl[i][p].
 *   - It is summed on the device in one fixed order that depends on the pattern count alone.
 *   - m is the lowest i with the largest lnl[i].
 * - Centred sums. mean[i] = (1/B) sum_b sums[b][i], the replicates added in one fixed order that
 *   depends on B alone. c[b][i] = sums[b][i] - mean[i].
 * - KH. p_kh[i] = #{b : c[b][m] - c[b][i] >= lnl[m] - lnl[i]} / B.
 * - SH. p_sh[i] = #{b : max_j c[b][j] - c[b][i] >= lnl[m] - lnl[i]} / B.
 * - Pair spread. s[i][j] = sqrt( sum_b (c[b][i] - c[b][j])^2 / (B - 1) ).
 *   - It is computed from the differences themselves, not from a Gram matrix.
 *   - Rows whose sums are bit-identical therefore have s = 0 exactly.
 * - WSH. The statistic is t(x)_i = max( 0, max over j != i with s[i][j] > 0 of (x_j - x_i) / s[i][j] ).
 *   - p_wsh[i] = #{b : t(c[b])_i >= t(lnl)_i} / B.
 *   - The zero term is the j = i term. Pairs with s = 0 differ by nothing and are left out.
 *
 * All comparisons are >=. For row m both sides of KH and SH are exactly 0, and x - x is exactly 0
 * in floating point. So p_kh[m] = p_sh[m] = 1 by arithmetic, not by a special case. A row whose
 * WSH statistic is 0 is equally robust.
 *
 * Every p is an integer count divided by B. With n = 1 all three are 1. The call needs B >= 2.
 *
 * How the device computes it (csrc/kernels_rell_tests.hip):
 *   the sums over patterns (lnl) and over replicates (mean): entry k goes to chunk k / 512, in it
 *   to slice (k % 512) / 128, in that to partial sum k % 4; a partial sum adds its entries by
 *   increasing k (lnl: one fused multiply-add per pattern; a pattern of weight 0 is left out, so it
 *   may hold anything), a slice is (p0 + p1) + (p2 + p3), a chunk (s0 + s1) + (s2 + s3), and the
 *   chunks are added by increasing index; mean = that sum / B;
 *   a pair's squares are added by increasing b, one fused multiply-add each, so s is symmetric to
 *   the bit; a statistic divides by multiplying with 1 / s[i][j], rounded once per pair;
 *   counts are integers added with integer atomics.  No result depends on a launch shape; a
 *   repeated call returns the same bits; a row's lnl, mean, p_kh do not depend on the other rows
 *   beyond lnl[m] and c[.][m].
 * Host pointers: lnl[n_rows] (may be NULL), bp, elw, sums as in rdamd_rell_bootstrap and
 * bit-identical to its results for the same arguments, p_kh[n_rows], p_sh[n_rows], p_wsh[n_rows]
 * (may be NULL: the O(n_rows^2 B) part is then not run), spread[n_rows][n_rows] (may be NULL):
 * the pair spreads s, for checks.
 * Error 62: as rdamd_rell_bootstrap; also n_replicates < 2, p_kh or p_sh missing, and p_wsh or
 * spread given with more than 8192 rows (the table of n_rows^2 doubles is 512 MB there) --
 * nothing is launched. */
int rdamd_rell_tests(const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
                     const unsigned int *pattern_weights, unsigned int n_replicates, uint64_t seed,
                     double *lnl, double *bp, double *elw, double *p_kh, double *p_sh, double *p_wsh,
                     double *sums, double *spread);
/* device time of everything this thread's last rdamd_rell_tests call launched after the
 * resampling kernel (BP / ELW included), milliseconds between two HIP events (0 after a failed
 * call); rdamd_rell_last_resample_ms holds the resampling kernel's own time of that call */
double rdamd_rell_last_tests_ms(void);

/* Approximately unbiased (AU) test of the rows (candidate roots) from a MULTISCALE RELL bootstrap
 * (Shimodaira 2002).  The inputs are those of rdamd_rell_bootstrap: site_lnl[n_rows][n_patterns],
 * pattern_weights, N = sum(pattern_weights), col2pat.  In addition there are K = n_scales scales,
 * given as integer draw counts n_draws[K] (scale k resamples M_k = n_draws[k] columns per
 * replicate, each drawn from all N columns), and B = n_replicates replicates per scale.
 *
 * - Scale seed. rdamd_rell_scale_seed(seed, k) = sm((seed + k + 1) mod 2^64), sm as in the
 *   rdamd_rell_column comment.  Host only.
 * - Sums. sums[k][b][i] = sum over d in [0, M_k) of
 *     site_lnl[i][col2pat[rdamd_rell_column(rdamd_rell_scale_seed(seed, k), b, d, N)]].
 *   The order rule is rdamd_rell_bootstrap's with M_k in place of N: draw d goes to partial sum
 *   d mod 8; each partial sum adds its draws by increasing d; the eight are combined as
 *   ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)).  A scale with M_k = N therefore gives exactly
 *   rdamd_rell_bootstrap's sums for seed rdamd_rell_scale_seed(seed, k), to the bit.  No sum
 *   depends on K, B, n_rows or a launch shape.
 * - Counts. counts[k][i] (unsigned) = the number of replicates b of scale k whose largest sum is
 *   row i's; ties go to the LOWEST i.  Each counts[k] sums to B.
 *
 * How the device computes it (csrc/kernels_rell.hip, the bootstrap's kernel template): one launch
 * covers every (scale, replicate) pair, the scales issued longest first; the winner of a replicate is found by
 * the wave that makes its sums and counted with one integer atomic add (more than 256 rows: the
 * waves of a replicate leave the largest sum and its lowest row of each 256-row chunk, 16 bytes,
 * and a second kernel picks among the chunks in row order).  The K x B x n_rows sums are written to
 * device memory only when `sums` is given; without it the call holds the transposed table,
 * K x n_rows counts and, beyond 256 rows, K x B x chunks of those 16 bytes.  A repeated call
 * returns the same bits.
 * Host pointers: n_draws[n_scales], counts[n_scales][n_rows],
 * sums[n_scales][n_replicates][n_rows] (may be NULL).
 * Error 62 -- nothing is launched: everything rdamd_rell_bootstrap refuses; n_scales < 2 or > 64;
 * an n_draws[k] of 0 or >= 2^32; two equal draw counts; site_lnl, pattern_weights, n_draws or
 * counts missing. */
uint64_t rdamd_rell_scale_seed(uint64_t seed, uint64_t k);
int rdamd_rell_multiscale(const double *site_lnl, unsigned int n_rows, unsigned int n_patterns,
                          const unsigned int *pattern_weights, unsigned int n_scales,
                          const uint64_t *n_draws, unsigned int n_replicates, uint64_t seed,
                          unsigned int *counts, double *sums);
/* device time of the resampling launch and, beyond 256 rows, the winner launch of this thread's
 * last rdamd_rell_multiscale call, milliseconds between two HIP events (0 after a failed call) */
double rdamd_rell_last_multiscale_ms(void);
/* The AU fit.  Host code, double precision, one row at a time, from the integer counts only; no
 * device is needed.  N = the column count the scales are relative to, B = n_replicates.
 * - r_k = M_k / N.  Scale k is usable for row i when 0 < counts[k][i] < B; used[i] = the number of
 *   usable scales.
 * - used >= 2: for each usable k, p = counts[k][i] / B, z = -Phi^-1(p) (evaluated as
 *   Phi^-1((B - counts[k][i]) / B) on the side where the argument is at most 1/2),
 *   v = p (1 - p) / (phi(z)^2 B), w = 1 / v, x1 = sqrt(r_k), x2 = 1 / sqrt(r_k).
 *   Minimise sum_k w (z - d x1 - c x2)^2 through the 2 x 2 normal equations
 *     a11 = sum w x1^2, a12 = sum w x1 x2, a22 = sum w x2^2, t1 = sum w x1 z, t2 = sum w x2 z,
 *     det = a11 a22 - a12^2, d = (a22 t1 - a12 t2) / det, c = (a11 t2 - a12 t1) / det,
 *   every sum taking its terms in order of k.
 *   p_au = 1 - Phi(d - c), computed as the upper tail erfc((d - c) / sqrt 2) / 2;
 *   rss = sum_k w (z - d x1 - c x2)^2, in order of k (degrees of freedom: used - 2; with
 *   used = 2 the two points are fitted exactly and rss is 0, not the rounding residue);
 *   se = phi(d - c) sqrt((a11 + a22 + 2 a12) / det): the standard error of d - c from the
 *   inverse of the normal matrix, times the density.
 * - used < 2: p_au = counts[k*][i] / B, k* = the scale whose M_k is nearest N (the lowest k among
 *   equals), and d = c = rss = se = 0.
 * Phi^-1 is Wichura's algorithm AS 241, routine PPND16 (Appl. Statist. 37, 1988), followed by one
 * Halley step against erfc; Phi and phi are erfc and exp of the C library.
 * p_au[n_rows] is required; d, c, rss, se (doubles) and used (unsigned) [n_rows] may be NULL.
 * Error 62: counts, n_draws or p_au missing, n_scales < 2 or > 64, n_rows, N or n_replicates 0,
 * N >= 2^32, an n_draws[k] of 0 or >= 2^32, two equal draw counts, a count above n_replicates. */
int rdamd_au_fit(const unsigned int *counts, unsigned int n_scales, unsigned int n_rows,
                 const uint64_t *n_draws, uint64_t N, unsigned int n_replicates, double *p_au,
                 double *d, double *c, double *rss, double *se, unsigned int *used);

/* RCCL communicator of one site group (librccl is loaded on first use; the
 * library has no link-time dependency on it).  Rank 0 of the group calls
 * rdamd_comm_unique_id and hands the 128 bytes to the others by any means
 * (rd_amd: its TCP rendezvous); every rank then calls rdamd_comm_create on its
 * own device.  rdamd_comm_reducer is a ready-made rdamd_lnl_reducer_t
 * (on_device = 1) whose `user` is the communicator.
 * A lost peer must not leave the other ranks of the group inside the collective:
 * rdamd_comm_reducer waits for its all-reduce by polling the stream and FAILS (after
 * ncclCommAbort; rdamd_errmsg says why) when RCCL reports an asynchronous error, when
 * nothing has arrived within the time limit (rdamd_comm_set_timeout; default 600 s, or
 * RDAMD_COMM_TIMEOUT seconds in the environment), or when another thread has called
 * rdamd_comm_abort -- rd_amd does from the thread that watches its rendezvous
 * connections.  An aborted communicator is unusable: exit and start a new process. */
typedef struct rdamd_comm rdamd_comm_t;
int           rdamd_comm_unique_id(char id[128]);
rdamd_comm_t *rdamd_comm_create(const char id[128], int rank, int n_ranks);
/* device_values[0 .. n) summed over the group in place, queued on `stream`.  HOW is the
 * communicator's sum mode:
 *   RDAMD_COMM_SUM_GATHER (default): ncclAllGather of the G vectors + a kernel on the same stream
 *     that adds them in RANK ORDER, ((v0 + v1) + v2) + ...: every rank holds the same bits by
 *     construction, whatever algorithm RCCL picks for a message of this size, and the sum is the
 *     one a host loop over the ranks makes (rd_amd --site-reduce host, dist.py) -- so a
 *     lock-stepped search gives the sequential sharded search's records bit for bit on real links;
 *   RDAMD_COMM_SUM_ALLREDUCE: one ncclAllReduce(values, values, n, ncclDouble, ncclSum).  The
 *     sum's association is RCCL's; identical bits on all ranks are NOT promised by the interface
 *     (ring / tree algorithms deliver them, direct small-message paths need not).
 * RDAMD_COMM_SUM=gather|allreduce in the environment sets the mode a new communicator starts in.
 * All ranks of a group must use the same mode. */
#define RDAMD_COMM_SUM_GATHER    0
#define RDAMD_COMM_SUM_ALLREDUCE 1
int           rdamd_comm_set_sum_mode(rdamd_comm_t *c, int mode);
int           rdamd_comm_sum_mode(const rdamd_comm_t *c);
int           rdamd_comm_allreduce_sum(rdamd_comm_t *c, double *device_values, unsigned int n,
                                       void *stream);
/* the second half of RDAMD_COMM_SUM_GATHER by itself: `ranks` vectors of n doubles, one behind
 * the other in device memory, added in rank order into out[0 .. n) (may be the first vector) */
int           rdamd_rank_order_sum(const double *gathered, double *out, unsigned int n,
                                   unsigned int ranks, void *stream);
int           rdamd_comm_reducer(double *values, unsigned int n, void *stream, void *user);
/* its two halves (rdamd_model_set_lnl_reducer_async): queue the all-reduce and return; wait for
 * a HIP event recorded behind it, with rdamd_comm_reducer's failure handling */
int           rdamd_comm_reducer_queue(double *values, unsigned int n, void *stream, void *user);
int           rdamd_comm_reducer_wait(void *event, void *user);
void          rdamd_comm_set_timeout(rdamd_comm_t *c, double seconds);
void          rdamd_comm_abort(rdamd_comm_t *c);   /* any thread */
void          rdamd_comm_destroy(rdamd_comm_t *c);

/* library / device info */
const char *rdamd_version(void);
/* Path of the HIP runtime (libamdhip64) this library runs on.  A caller that hands over
 * DEVICE pointers it got elsewhere (rdamd_evaluate_batch_device, rdamd_comm_allreduce_sum)
 * must have got them from the same runtime instance: a process can hold two (ML frameworks
 * bundle their own ROCm next to /opt/rocm); bench.py checks before it passes a tensor. */
const char *rdamd_hip_runtime_path(void);
int         rdamd_device_count(void);
/* selects the HIP device later rdamd_partition_create calls of this thread use
 * (one process per GPU: call with LOCAL_RANK). */
int         rdamd_set_device(int device);
/* free / total memory of the current device in bytes (hipMemGetInfo) */
int         rdamd_device_memory(uint64_t *free_bytes, uint64_t *total_bytes);
/* device bytes a partition of this shape takes (rdamd_partition_create's buffers) */
uint64_t    rdamd_partition_footprint(unsigned int tips, unsigned int clv_buffers,
                                      unsigned int states, unsigned int sites,
                                      unsigned int prob_matrices, unsigned int rate_cats,
                                      unsigned int scale_buffers);
/* Replicas rdamd_model_exhaustive_search_parallel / _lockstep may hold for this
 * model on the current device: `requested`, clamped so that the replicas'
 * partitions fit in 85 % of the device memory that is free now; at least 1.  A replica's
 * 4-state / binary partitions are RDAMD_ATTRIB_SPARSE_CLVS ones while the searches'
 * compute_lh is the children-only one (the default): three CLVs, not 2n - 3.  replica_bytes (optional): what one
 * replica takes.  The two searches apply this clamp themselves and say so on
 * stderr when it bites. */
unsigned int rdamd_model_max_replicas(const rdamd_model_t *m, unsigned int requested,
                                      uint64_t *replica_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ROOT_DIGGER_AMD_H_ */
