// rd_amd: the `rd` command line of the reference (/root/reference/src/main.cpp)
// as a native program on top of the C ABI -- include/root_digger_amd.h is the
// only project header it uses, so it doubles as the example of a whole-program
// caller.  Same option names as the reference; `--lbfgsb <lib>` names the shared
// library that exports the caller's L-BFGS-B entry point `setulb` (lib/lbfgsb of
// the reference builds as one).  Several processes (one per GPU: RANK,
// LOCAL_RANK, WORLD_SIZE in the environment, the way torch.distributed.run or
// any launcher sets them) split the candidate roots like the reference's MPI
// ranks (src/model.cpp:1867-1911) and meet in the <prefix>.ckp file; they
// synchronise over TCP at MASTER_ADDR:MASTER_PORT.
//
// --site-shards G (new here; north star / SURVEY 8e): the ranks form WORLD_SIZE/G
// candidate groups of G adjacent ranks.  A group shares its candidates; each
// member holds one contiguous block of the alignment's columns, and every
// log-likelihood is summed over the group -- on the device over RCCL (default:
// ncclAllGather + a sum in rank order, identical bits on every rank by
// construction; --site-reduce rccl-allreduce: one ncclAllReduce), or through the
// host with --site-reduce host (ranks that share one GPU).  G = WORLD_SIZE is BASELINE config c4's layout (site blocks
// only), 1 < G < WORLD_SIZE config c5's 2-D grid.  With --partition, each member holds block b of
// EVERY partition's own columns (rdamd_model_create_partitioned_block); every partition keeps its
// own parameters, as in the reference's partitioned runs.
//
// --rell B [--rell-seed N] / --site-lh (new here, with --exhaustive): after the search rank 0 reads
// every candidate's parameters back from the checkpoint, evaluates their site log-likelihoods
// (rdamd_model_site_lnls) and writes <prefix>.sitelh (Tree-Puzzle / CONSEL layout) and, from a RELL
// bootstrap of B replicates on the device (rdamd_rell_bootstrap), <prefix>.support.tsv and the BP /
// ELW annotations of <prefix>.lwr.tree.  --root-tests (with --rell): the KH, SH and weighted-SH tests of
// every candidate from the same replicates (rdamd_rell_tests instead of rdamd_rell_bootstrap):
// <prefix>.roottests.tsv, and pKH / pSH / pWSH next to BP / ELW on <prefix>.lwr.tree.  --au (with --rell):
// the approximately unbiased test from B replicates at each of ten scales (rdamd_rell_multiscale,
// rdamd_au_fit): <prefix>.au.tsv and pAU on <prefix>.lwr.tree.
//
// --ancestral / --site-rates (new here, with --exhaustive): after the search rank 0 takes the best
// record's root and parameters from the checkpoint and reconstructs what that root implies
// (rdamd_model_ancestral, one call): <prefix>.ancestral.tsv, the posterior of every state at every inner
// node and alignment column; <prefix>.ancestral.tree, the tree rooted there with the inner nodes named
// N0 (the root), N1, ... as in the rows; with --site-rates <prefix>.siterates.tsv, the posterior mean
// rate and the rate-category posteriors of every column.
//
// --branch-lengths [--brlen-min 1e-6] [--brlen-max 100] (new here, with --exhaustive): after the search
// rank 0 takes the best record's root and parameters from the checkpoint and maximises lnL over all
// 2n - 2 branch lengths of the tree rooted there (rdamd_model_optimize_branch_lengths; nothing is fed
// back into the search): <prefix>.brlen.tsv, one row per branch with the input and the optimised length
// and both derivatives at the optimum; <prefix>.brlen.tree, the rooted tree with the optimised lengths.
//
// --gradient (new here, with --exhaustive): after the search rank 0 takes the best record's root and
// parameters from the checkpoint and writes the exact gradient of lnL there in the variables the
// search's L-BFGS-B sees (rdamd_model_gradient): <prefix>.gradient.tsv, one row per parameter with its
// value, the exact gradient, the forward difference with the search's own step h = max(1e-4 |x|, 1e-4)
// and whether the value sits at the optimiser's bound; one line with the largest projected component.
//
// --substitutions [--subst-min-prob P] (new here, with --exhaustive): after the search rank 0 maps the
// substitutions onto the branches at the best record's root and parameters (rdamd_model_substitutions):
// <prefix>.substitutions.tsv, one row per branch with the child's name as in .ancestral.tree, the length,
// the expected number of substitutions, the K K - K typed counts, the K dwell times and the sum over
// columns of the probability of a change; <prefix>.mutations.tsv, one row per (branch, alignment column)
// whose likeliest change i -> j has posterior probability >= P (default 0.5), with that probability and
// the expected number of substitutions at the column; <prefix>.substitutions.tree, the rooted tree with
// the inner nodes named as in the rows.
//
//   rd_amd --msa aln.fasta --tree t.nwk --prefix out --exhaustive --lbfgsb liblbfgsb.so
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <fstream>
#include <getopt.h>
#include <iostream>
#include <stdexcept>
#include <string>
#include <memory>
#include <thread>
#include <vector>

#include "root_digger_amd.h"
#include "rendezvous.hpp"

namespace {

struct options_t {
  std::string msa, tree, prefix, partition, model, lbfgsb, rate_cats_type = "mean";
  unsigned states = 4, rate_cats = 1, min_roots = 1, workers = 4;
  int lockstep = -1, device = -1, site_shards = 1, lockstep_rounds = -1, lockstep_groups = 0;
  bool site_reduce_host = false, site_allreduce = false, stats = false;
  uint64_t seed = 1;
  double root_ratio = 0.01, atol = 1e-7, bfgstol = 1e-7, brtol = 1e-12, factor = 1e4;
  int early_stop = 0;   // initialized_flag_t: 0 unset, 1 true, 2 false
  int strategy = 2;     // random, midpoint, modified-mad
  bool exhaustive = false, silent = false, clean = false, echo = false, no_checkpoint = false,
       invariant_sites = false;
  // RELL bootstrap of the candidates' site lnLs (--rell B, 0: off) and the .sitelh file
  long rell = 0;
  bool rell_given = false, rell_seed_given = false, site_lh = false, root_tests = false, au = false;
  // what the best root implies: ancestral states (.ancestral.tsv, .ancestral.tree), site rates (.siterates.tsv)
  bool ancestral = false, site_rates = false;
  // the ML branch lengths at the best root (.brlen.tsv, .brlen.tree) and their box
  bool branch_lengths = false, gradient = false;   // gradient: the exact gradient at the best record (.gradient.tsv)
  // substitutions mapped onto the branches at the best record (.substitutions.tsv / .tree, .mutations.tsv)
  bool substitutions = false;
  double subst_min_prob = 0.5;
  double brlen_min = 1e-6, brlen_max = 100.0;
  uint64_t rell_seed = 0;
};

[[noreturn]] void die(const std::string &what) {
  std::cout << "There was an error during processing:\n" << what << std::endl;
  std::exit(1);
}
void need(int rc, const char *what) {
  if (rc != RDAMD_SUCCESS) die(std::string(what) + ": " + rdamd_errmsg());
}

void usage() {
  std::puts(
      "Usage: rd_amd --msa <FILE> --tree <FILE> [--prefix <STRING>] [--exhaustive]\n"
      "  --partition <FILE>  --model <STRING>  --states {2,4}  --rate-cats <N>\n"
      "  --rate-cats-type {mean,median,free}  --seed <N>  --min-roots <N>  --root-ratio <X>\n"
      "  --atol <X>  --brtol <X>  --bfgstol <X>  --factor <X>  --early-stop  --no-early-stop\n"
      "  --initial-root-strategy {random,midpoint,modified-mad}  --threads <N>  --lockstep <N>\n"
      "  --site-shards <G>  --site-reduce {rccl,rccl-allreduce,host}  --lockstep-rounds {0,1}  --lockstep-groups {1,2}  --stats\n"
      "  --lbfgsb <LIB>  --device <N>  --silent  --echo  --clean  --no-checkpoint  --version\n"
      "  --rell <B>  --rell-seed <N>  --site-lh   (with --exhaustive: RELL support and site lnLs of every root)\n"
      "  --root-tests   (with --rell: KH, SH and weighted-SH p-values of every root, <prefix>.roottests.tsv)\n"
      "  --au   (with --rell: AU test of every root from B replicates at each of ten scales, <prefix>.au.tsv)\n"
      "  --ancestral   (with --exhaustive: ancestral state posteriors at the best root, <prefix>.ancestral.tsv / .tree)\n"
      "  --site-rates   (with --exhaustive: posterior mean rate of every column at the best root, <prefix>.siterates.tsv)\n"
      "  --branch-lengths [--brlen-min <X>] [--brlen-max <X>]   (with --exhaustive: ML branch lengths at the best root,\n"
      "                <prefix>.brlen.tsv / .tree)\n"
      "  --gradient   (with --exhaustive: exact gradient of lnL in the model parameters at the best record,\n"
      "                <prefix>.gradient.tsv)\n"
      "  --substitutions [--subst-min-prob <P>]   (with --exhaustive: expected substitution counts per branch and the\n"
      "                mutations with posterior probability >= P (default 0.5) at the best record,\n"
      "                <prefix>.substitutions.tsv / .tree, <prefix>.mutations.tsv)");
}

options_t parse(int argc, char **argv) {
  static option long_opts[] = {
      {"msa", required_argument, 0, 0},          {"tree", required_argument, 0, 0},
      {"model", required_argument, 0, 0},        {"seed", required_argument, 0, 0},
      {"verbose", no_argument, 0, 0},            {"silent", no_argument, 0, 0},
      {"min-roots", required_argument, 0, 0},    {"root-ratio", required_argument, 0, 0},
      {"atol", required_argument, 0, 0},         {"brtol", required_argument, 0, 0},
      {"bfgstol", required_argument, 0, 0},      {"factor", required_argument, 0, 0},
      {"partition", required_argument, 0, 0},    {"prefix", required_argument, 0, 0},
      {"exhaustive", no_argument, 0, 0},         {"early-stop", no_argument, 0, 0},
      {"no-early-stop", no_argument, 0, 0},      {"rate-cats", required_argument, 0, 0},
      {"rate-cats-type", required_argument, 0, 0}, {"invariant-sites", no_argument, 0, 0},
      {"states", required_argument, 0, 0},       {"initial-root-strategy", required_argument, 0, 0},
      {"threads", required_argument, 0, 0},      {"version", no_argument, 0, 0},
      {"debug", no_argument, 0, 0},              {"mpi-debug", no_argument, 0, 0},
      {"clean", no_argument, 0, 0},              {"echo", no_argument, 0, 0},
      {"help", no_argument, 0, 0},               {"lbfgsb", required_argument, 0, 0},
      {"lockstep", required_argument, 0, 0},     {"device", required_argument, 0, 0},
      {"no-checkpoint", no_argument, 0, 0},      {"site-shards", required_argument, 0, 0},
      {"site-reduce", required_argument, 0, 0},  {"lockstep-rounds", required_argument, 0, 0},
      {"stats", no_argument, 0, 0},              {"lockstep-groups", required_argument, 0, 0},
      {"rell", required_argument, 0, 0},         {"rell-seed", required_argument, 0, 0},
      {"site-lh", no_argument, 0, 0},            {"root-tests", no_argument, 0, 0},
      {"au", no_argument, 0, 0},                 {"ancestral", no_argument, 0, 0},
      {"site-rates", no_argument, 0, 0},         {"branch-lengths", no_argument, 0, 0},
      {"brlen-min", required_argument, 0, 0},    {"brlen-max", required_argument, 0, 0},
      {"gradient", no_argument, 0, 0},
      {"substitutions", no_argument, 0, 0},      {"subst-min-prob", required_argument, 0, 0},
      {0, 0, 0, 0}};
  options_t o;
  int index = 0;
  while (getopt_long_only(argc, argv, "", long_opts, &index) == 0) {
    const std::string name = long_opts[index].name;
    const char *v = optarg;
    if (name == "msa") o.msa = v;
    else if (name == "tree") o.tree = v;
    else if (name == "model") o.model = v;
    else if (name == "seed") o.seed = std::strtoull(v, nullptr, 10);
    else if (name == "silent") o.silent = true;
    else if (name == "min-roots") o.min_roots = (unsigned)std::atol(v);
    else if (name == "root-ratio") o.root_ratio = std::atof(v);
    else if (name == "atol") o.atol = std::atof(v);
    else if (name == "brtol") o.brtol = std::atof(v);
    else if (name == "bfgstol") o.bfgstol = std::atof(v);
    else if (name == "factor") o.factor = std::atof(v);
    else if (name == "partition") o.partition = v;
    else if (name == "prefix") o.prefix = v;
    else if (name == "exhaustive") o.exhaustive = true;
    else if (name == "early-stop") o.early_stop = 1;
    else if (name == "no-early-stop") o.early_stop = 2;
    else if (name == "rate-cats") o.rate_cats = (unsigned)std::atol(v);
    else if (name == "rate-cats-type") o.rate_cats_type = v;
    else if (name == "invariant-sites") o.invariant_sites = true;
    else if (name == "states") o.states = (unsigned)std::atol(v);
    else if (name == "initial-root-strategy") {
      const std::string s = v;
      o.strategy = s == "random" ? 0 : s == "midpoint" ? 1 : s == "modified-mad" ? 2 : -1;
      if (o.strategy < 0) die("An argument is required for --initial-root-strategy");
    } else if (name == "threads") o.workers = (unsigned)std::atol(v);
    else if (name == "version") { std::puts(rdamd_version()); std::exit(0); }
    else if (name == "clean") o.clean = true;
    else if (name == "echo") o.echo = true;
    else if (name == "help") { usage(); std::exit(0); }
    else if (name == "lbfgsb") o.lbfgsb = v;
    else if (name == "lockstep") o.lockstep = std::atoi(v);
    else if (name == "device") o.device = std::atoi(v);
    else if (name == "no-checkpoint") o.no_checkpoint = true;
    else if (name == "site-shards") o.site_shards = std::atoi(v);
    else if (name == "lockstep-rounds") o.lockstep_rounds = std::atoi(v);
    else if (name == "lockstep-groups") o.lockstep_groups = std::atoi(v);
    else if (name == "stats") o.stats = true;
    else if (name == "rell") { o.rell = std::atol(v); o.rell_given = true; }
    else if (name == "rell-seed") { o.rell_seed = std::strtoull(v, nullptr, 10); o.rell_seed_given = true; }
    else if (name == "site-lh") o.site_lh = true;
    else if (name == "root-tests") o.root_tests = true;
    else if (name == "au") o.au = true;
    else if (name == "ancestral") o.ancestral = true;
    else if (name == "site-rates") o.site_rates = true;
    else if (name == "branch-lengths") o.branch_lengths = true;
    else if (name == "gradient") o.gradient = true;
    else if (name == "substitutions") o.substitutions = true;
    else if (name == "subst-min-prob") o.subst_min_prob = std::atof(v);
    else if (name == "brlen-min") o.brlen_min = std::atof(v);
    else if (name == "brlen-max") o.brlen_max = std::atof(v);
    else if (name == "site-reduce") {
      const std::string s = v;
      if (s != "rccl" && s != "rccl-allreduce" && s != "host") die("--site-reduce takes rccl, rccl-allreduce or host");
      o.site_reduce_host = s == "host";
      o.site_allreduce = s == "rccl-allreduce";
    }
  }
  return o;
}

int env_int(const char *name, int fallback) {
  const char *v = std::getenv(name);
  return v ? std::atoi(v) : fallback;
}

}  // namespace

static int run(int argc, char **argv);

int main(int argc, char **argv) {
  try {
    return run(argc, argv);
  } catch (const std::exception &e) {
    die(e.what());
  }
}

static int run(int argc, char **argv) {
  using rdamd_tools::rendezvous_t;
  using rdamd_tools::site_group_t;
  const auto start = std::chrono::steady_clock::now();
  options_t o = parse(argc, argv);
  const int rank = env_int("RANK", 0), world = env_int("WORLD_SIZE", 1);
  if (o.prefix.empty()) o.prefix = o.msa;
  if (world > 1 && o.no_checkpoint) die("--no-checkpoint: the ranks of a run meet in the checkpoint file");
  // the candidates' records and parameters are read back from the checkpoint; a site group's
  // member holds one block of the columns
  const char *support_opt = o.rell_given ? "--rell" : o.site_lh ? "--site-lh" : o.ancestral ? "--ancestral"
                            : o.site_rates ? "--site-rates" : o.branch_lengths ? "--branch-lengths"
                            : o.gradient ? "--gradient" : o.substitutions ? "--substitutions" : nullptr;
  const bool site_support = o.rell_given || o.site_lh;   // the site lnLs of every candidate are wanted
  if (o.rell_seed_given && !o.rell_given) die("--rell-seed: there is no --rell to seed");
  if (o.root_tests && !o.rell_given) die("--root-tests: the tests are made from the replicates of --rell <B>");
  if (o.root_tests && o.rell < 2) die("--root-tests: --rell must give at least 2 replicates");
  if (o.au && !o.rell_given) die("--au: the test is made from --rell <B> replicates at every scale");
  if (o.au && o.rell < 2) die("--au: --rell must give at least 2 replicates");
  if (o.branch_lengths && !(o.brlen_min > 0.0 && o.brlen_min < o.brlen_max && std::isfinite(o.brlen_max)))
    die("--branch-lengths: 0 < --brlen-min < --brlen-max is required");
  if (!(o.subst_min_prob >= 0.0 && o.subst_min_prob <= 1.0)) die("--subst-min-prob: a probability in [0, 1] is required");
  if (support_opt) {
    const std::string opt = support_opt;
    if (o.rell_given && (o.rell < 1 || o.rell > 0x7fffffffl)) die("--rell: the number of replicates must be at least 1");
    if (o.no_checkpoint) die(opt + ": the candidates' parameters are read from the checkpoint; not with --no-checkpoint");
    if (o.site_shards > 1) die(opt + ": not supported with --site-shards > 1 (each rank holds one block of the columns)");
  }
  need(rdamd_set_device(o.device >= 0 ? o.device : env_int("LOCAL_RANK", 0)), "set_device");
  rendezvous_t ranks(rank, world);
  // candidate groups x site shards (see the header comment): rank = cgroup * G + srank
  const int G = o.site_shards;
  if (G < 1 || world % G) die("--site-shards must divide the number of ranks");
  const int cgroups = world / G, cgroup = rank / G, srank = rank % G;
  std::unique_ptr<site_group_t> host_group;
  rdamd_comm_t *comm = nullptr;
  if (G > 1 && o.site_reduce_host) {
    host_group.reset(new site_group_t(ranks, G));
    // (test hook, see rendezvous.hpp: RDAMD_FAULT_ULP=<rank>:<call>)
    if (const char *f = std::getenv("RDAMD_FAULT_ULP")) {
      int fr = -1;
      unsigned long long fc = 0;
      if (std::sscanf(f, "%d:%llu", &fr, &fc) == 2 && fr == rank) host_group->set_fault(fc);
    }
  } else if (G > 1) {   // the group leader's RCCL id reaches the members over the world star
    char id[128] = {0};
    if (srank == 0) need(rdamd_comm_unique_id(id), "RCCL unique id");
    std::vector<char> all;
    ranks.allgather(id, sizeof id, all);
    comm = rdamd_comm_create(all.data() + sizeof id * (size_t)(cgroup * G), srank, G);
    if (!comm) die(std::string("RCCL communicator: ") + rdamd_errmsg());
    if (o.site_allreduce) need(rdamd_comm_set_sum_mode(comm, RDAMD_COMM_SUM_ALLREDUCE), "sum mode");
  }

  // ---- checkpoint: mpi_create_checkpoint + merge_options_checkpoint, src/main.cpp:335-409
  rdamd_checkpoint_t *ckp = nullptr;
  std::vector<rdamd_ratehet_opts_t> header_cats;
  if (!o.no_checkpoint) {
    if (rank == 0) {
      ckp = rdamd_checkpoint_open(o.prefix.c_str());
      if (!ckp) die(std::string("checkpoint: ") + rdamd_errmsg());
      if (o.clean) {
        need(rdamd_checkpoint_clean(ckp), "checkpoint clean");
        return 0;
      }
      if (!rdamd_checkpoint_existing(ckp)) {
        rdamd_ratehet_opts_t rc{1, o.rate_cats_type == "median" ? 0 : o.rate_cats_type == "free" ? 2 : 1,
                                o.rate_cats, 0, 1.0};
        rdamd_cli_options_t h;
        std::memset(&h, 0, sizeof h);
        h.msa_filename = o.msa.c_str(); h.tree_filename = o.tree.c_str(); h.prefix = o.prefix.c_str();
        h.prefix_dir = ""; h.model_filename = ""; h.freqs_filename = "";
        h.partition_filename = o.partition.c_str(); h.data_type = o.states == 2 ? "bin" : "nt";
        h.model_string = o.model.c_str();
        h.rate_cats = &rc; h.n_rate_cats = 1;
        h.seed = o.seed; h.min_roots = o.min_roots; h.threads = o.workers;
        h.root_ratio = o.root_ratio; h.abs_tolerance = o.atol; h.factor = o.factor;
        h.br_tolerance = o.brtol; h.bfgs_tol = o.bfgstol;
        h.silent = o.silent; h.exhaustive = o.exhaustive; h.invariant_sites = o.invariant_sites;
        h.early_stop = o.early_stop; h.initial_root_strategy = o.strategy;
        need(rdamd_checkpoint_save_options(ckp, &h), "checkpoint save_options");
      }
      if (rdamd_checkpoint_needs_cleaning(ckp) == 1) need(rdamd_checkpoint_clean(ckp), "checkpoint clean");
    } else if (o.clean) {
      return 0;
    }
    ranks.barrier();
    if (rank != 0) {
      ckp = rdamd_checkpoint_open(o.prefix.c_str());
      if (!ckp) die(std::string("checkpoint: ") + rdamd_errmsg());
    }
    rdamd_cli_options_t h;
    if (rdamd_checkpoint_existing(ckp) && rdamd_checkpoint_load_options(ckp, &h) == RDAMD_SUCCESS) {
      if (!o.silent && rank == 0)
        std::cerr << "Loading options from the checkpoint file. Some cli options are ignored. If "
                     "the program is not working, try deleting the checkpoint file\n";
      o.msa = h.msa_filename; o.tree = h.tree_filename; o.partition = h.partition_filename;
      o.model = h.model_string;
      if (h.n_rate_cats) {
        o.rate_cats = (unsigned)h.rate_cats[0].rate_cats;
        o.rate_cats_type = h.rate_cats[0].rate_category_type == 0   ? "median"
                           : h.rate_cats[0].rate_category_type == 2 ? "free" : "mean";
      }
      o.seed = h.seed; o.atol = h.abs_tolerance; o.factor = h.factor; o.brtol = h.br_tolerance;
      o.bfgstol = h.bfgs_tol; o.exhaustive = h.exhaustive != 0; o.min_roots = (unsigned)h.min_roots;
      o.root_ratio = h.root_ratio; o.strategy = h.initial_root_strategy; o.early_stop = h.early_stop;
    }
  }
  if (support_opt && !o.exhaustive)
    die(std::string(support_opt) + ": needs --exhaustive (the heuristic search evaluates one root)");
  if (!o.rell_seed_given) o.rell_seed = o.seed;
  if (o.msa.empty()) { std::puts("No MSA was given, please supply an MSA"); usage(); return 1; }
  if (o.tree.empty()) { std::puts("No tree was given, please supply an tree"); usage(); return 1; }

  // ---- tree, alignment, model (src/main.cpp:484-584)
  rdamd_tree_t *tree = rdamd_tree_from_file(o.tree.c_str());
  if (!tree) die(rdamd_errmsg());
  const unsigned roots = rdamd_tree_root_count(tree);
  if (o.min_roots > roots) die("Min roots is larger than the number of roots on the tree");
  const bool early_stop = o.early_stop == 1 || (o.early_stop == 0 && !o.exhaustive);
  const uint64_t *map = o.states == 2 ? rdamd_map_bin : rdamd_map_nt;
  if (!o.model.empty()) {
    rdamd_partition_info_t mi;
    need(rdamd_parse_model_info(o.model.c_str(), &mi), "model string");
    o.rate_cats = mi.ratehet.rate_cats ? (unsigned)mi.ratehet.rate_cats : 1u;
  }
  rdamd_model_t *model = nullptr;
  // (the partition file may come from a resumed run's checkpoint: it is known only here.  A site
  // group's member builds its own block of every partition -- the whole partitioned model on every
  // member would count every lnL G times once the group's reduction is installed)
  if (!o.partition.empty() && G > 1) {
    // (room for one entry per line: at least one per partition)
    size_t lines = 1;
    {
      std::ifstream pf(o.partition);
      for (std::string line; std::getline(pf, line);) ++lines;
    }
    unsigned n_parts = 0;
    std::vector<unsigned> patterns(lines), columns(lines);
    model = rdamd_model_create_partitioned_block(tree, o.msa.c_str(), o.partition.c_str(), o.states, map, o.seed,
                                                 early_stop, (unsigned)srank, (unsigned)G, &n_parts, patterns.data(),
                                                 columns.data());
    if (model && !o.silent)
      for (unsigned p = 0; p < n_parts; ++p)
        std::printf("[rank %d] candidate group %d/%d, partition %u, site block %d/%d: %u patterns of %u columns\n",
                    rank, cgroup, cgroups, p, srank, G, patterns[p], columns[p]);
  } else if (!o.partition.empty()) {
    unsigned n_parts = 0;
    model = rdamd_model_create_partitioned(tree, o.msa.c_str(), o.partition.c_str(), o.states, map,
                                           o.seed, early_stop, &n_parts);
  } else {
    rdamd_ratehet_opts_t rc{1, o.rate_cats_type == "median" ? 0 : o.rate_cats_type == "free" ? 2 : 1,
                            o.rate_cats, 0, 1.0};
    unsigned patterns = 0, columns = 0;
    model = G > 1 ? rdamd_model_create_from_file_block(tree, o.msa.c_str(), o.states, map, &rc, o.seed,
                                                       early_stop, 1, (unsigned)srank, (unsigned)G,
                                                       &patterns, &columns)
                  : rdamd_model_create_from_file_ratehet(tree, o.msa.c_str(), o.states, map, &rc,
                                                         o.seed, early_stop, 1, &patterns);
    if (model && G > 1 && !o.silent)
      std::printf("[rank %d] candidate group %d/%d, site block %d/%d: %u patterns of %u columns\n",
                  rank, cgroup, cgroups, srank, G, patterns, columns);
  }
  if (!model) die(rdamd_errmsg());
  // before anything is evaluated: the empirical frequencies are reduced too
  if (host_group) {
    need(rdamd_model_set_lnl_reducer(model, site_group_t::reducer, host_group.get(), 0), "reducer");
    need(rdamd_model_set_lnl_reducer_abort(model, site_group_t::abort_hook, host_group.get()), "reducer abort");
  } else if (comm)
    need(rdamd_model_set_lnl_reducer(model, rdamd_comm_reducer, comm, 1), "reducer");
  if (o.echo) {
    char *nw = rdamd_tree_newick(tree, 1);
    std::cout << nw << std::endl;
    std::free(nw);
  }
  if (rdamd_model_initialize_partitions(model, 0) != RDAMD_SUCCESS)     // invalid empirical
    need(rdamd_model_initialize_partitions(model, 1), "initialize_partitions");   // frequencies -> uniform
  if (!o.lbfgsb.empty()) {
    void *lib = dlopen(o.lbfgsb.c_str(), RTLD_NOW | RTLD_GLOBAL);
    void *fn = lib ? dlsym(lib, "setulb") : nullptr;
    if (!fn) die("--lbfgsb: " + o.lbfgsb + " does not export setulb");
    rdamd_model_set_lbfgsb(model, fn);
  }
  rdamd_root_location_t rl0;
  need(rdamd_tree_root_location(tree, 0, &rl0), "root_location");
  rdamd_model_compute_lh(model, &rl0);                                   // model.initialize()
  if (ckp && srank == 0) rdamd_model_set_checkpoint(model, ckp);   // one record per candidate
  if (o.lockstep < 0) o.lockstep = !o.lbfgsb.empty() ? 32 : 0;   // (partitioned models lock-step too)
  // A site group's candidates advance in lock step in deterministic rounds (every rank of the
  // group forms the same launches and one collective per round; --lockstep 0: one candidate
  // at a time, a collective per request); free-running replicas would reorder the collectives.
  if (G > 1) o.workers = 0;
  if (o.lockstep_rounds >= 0) rdamd_model_set_lockstep_rounds(model, o.lockstep_rounds);
  if (o.lockstep_groups > 0) rdamd_model_set_lockstep_groups(model, (unsigned)o.lockstep_groups);

  // While the ranks search they exchange nothing over the rendezvous: the end of a
  // connection now means that a rank has died.  Nobody must stay behind inside a
  // collective (or wait for the dead rank's checkpoint records): abort the site group's
  // communicator and leave; closing our own connections passes the news on.
  const auto watch_ranks = [&ranks, comm, rank] {
    ranks.watch([comm, rank] {
      std::fprintf(stderr, "[rank %d] another rank of this run has gone; giving up\n", rank);
      if (comm) rdamd_comm_abort(comm);
      std::this_thread::sleep_for(std::chrono::seconds(comm ? 2 : 0));   // let a blocked reducer fail first
      std::_Exit(3);
    });
  };

  // ---- the search (src/main.cpp:586-635)
  std::vector<uint64_t> ids(roots);
  std::vector<double> llh(roots), alpha(roots);
  unsigned n_results = 0;
  rdamd_root_location_t best;
  double best_llh = -INFINITY;
  std::memset(&best, 0, sizeof best);
  if (o.exhaustive) {
    need(rdamd_model_assign_by_rank_checkpoint(model, (unsigned)cgroup, (unsigned)cgroups, ckp), "assign");
    ranks.barrier();
    watch_ranks();
    if (!o.silent && rank == 0) {
      std::puts("Starting exhaustive search");
      rdamd_model_set_progress(model, 1);
    }
    if (o.lockstep > 0)
      need(rdamd_model_exhaustive_search_lockstep(model, (unsigned)o.lockstep, o.atol, o.bfgstol, o.brtol,
                                                  o.factor, ids.data(), llh.data(), alpha.data(),
                                                  &n_results, &best, &best_llh), "exhaustive_search");
    else if (o.workers > 0)
      need(rdamd_model_exhaustive_search_parallel(model, o.workers, o.atol, o.bfgstol, o.brtol, o.factor,
                                                  ids.data(), llh.data(), alpha.data(), &n_results,
                                                  &best, &best_llh), "exhaustive_search");
    else
      need(rdamd_model_exhaustive_search(model, o.atol, o.bfgstol, o.brtol, o.factor, ids.data(),
                                         llh.data(), alpha.data(), &n_results, &best, &best_llh),
           "exhaustive_search");
  } else {
    if (o.lbfgsb.empty()) die("the heuristic search optimises the model parameters: it needs --lbfgsb");
    need(rdamd_model_assign_by_rank_search(model, o.min_roots, o.root_ratio, (unsigned)cgroup,
                                           (unsigned)cgroups, o.strategy, ckp), "assign");
    ranks.barrier();
    watch_ranks();
    std::vector<uint64_t> mine(roots);
    const int assigned = rdamd_model_assigned(model, mine.data(), roots);
    if (!o.silent && rank == 0) {
      std::puts("Starting root search");
      rdamd_model_set_progress(model, 1);
    }
    need(rdamd_model_search(model, o.min_roots, o.root_ratio, o.atol, o.bfgstol, o.brtol, o.factor,
                            &best, &best_llh), "search");
    if (assigned > 0) {
      ids[0] = best.id; llh[0] = best_llh; alpha[0] = best.brlen_ratio;
      n_results = 1;
    }
  }
  if (o.stats) {   // one line per rank on stderr: what the search launched and summed
    uint64_t ls[4] = {0, 0, 0, 0}, rs[4] = {0, 0, 0, 0}, ct[6] = {0, 0, 0, 0, 0, 0};
    rdamd_model_lockstep_stats(model, ls);
    rdamd_model_round_stats(model, rs);
    rdamd_model_counters(model, ct);
    double rsec[4] = {0, 0, 0, 0};
    rdamd_model_round_seconds(model, rsec);
    const std::chrono::duration<double> took = std::chrono::steady_clock::now() - start;
    uint64_t digest = 1469598103934665603ull;   // FNV-1a over the bits of this rank's (id, lnL, alpha) triples
    auto mix = [&digest](const void *ptr, size_t n) {
      for (size_t i = 0; i < n; ++i) digest = (digest ^ ((const unsigned char *)ptr)[i]) * 1099511628211ull;
    };
    for (unsigned i = 0; i < n_results; ++i) { mix(&ids[i], 8); mix(&llh[i], 8); mix(&alpha[i], 8); }
    std::fprintf(stderr, "[rank %d] stats: candidates=%u results_digest=%016llx lockstep=%d rounds=%llu collectives=%llu redos=%llu "
                         "own_collectives=%llu objective_launches=%llu objective_jobs=%llu root_launches=%llu "
                         "root_steps=%llu round_seconds=%.2f/%.2f/%.2f/%.2f seconds=%.3f\n",
                 rank, n_results, (unsigned long long)digest, o.lockstep, (unsigned long long)rs[0], (unsigned long long)rs[1],
                 (unsigned long long)rs[2], (unsigned long long)rs[3],
                 (unsigned long long)(ls[0] ? ls[0] : ct[0]), (unsigned long long)(ls[1] ? ls[1] : ct[1]),
                 (unsigned long long)ls[2], (unsigned long long)ls[3], rsec[0], rsec[1], rsec[2], rsec[3], took.count());
  }
  const std::chrono::duration<double> search_took = std::chrono::steady_clock::now() - start;
  ranks.barrier();
  if (rank != 0) {
    rdamd_model_destroy(model);
    if (comm) rdamd_comm_destroy(comm);
    return 0;
  }

  // ---- rank 0: everybody's results from the log (src/model.cpp:1237-1268), the trees
  if (ckp) {
    unsigned n = 0;
    need(rdamd_checkpoint_read_results(ckp, &n), "checkpoint read_results");
    ids.assign(n, 0); llh.assign(n, 0.0); alpha.assign(n, 0.0);
    n_results = n;
    for (unsigned i = 0; i < n; ++i) {
      unsigned np = 0;
      uint64_t nv = 0;
      rdamd_checkpoint_result(ckp, i, &ids[i], &llh[i], &alpha[i], &np, &nv);
    }
    unsigned k = 0;
    for (unsigned i = 1; i < n; ++i)
      if (llh[i] > llh[k]) k = i;   // first maximum, as std::max_element
    if (n) {
      need(rdamd_tree_root_location(tree, (unsigned)ids[k], &best), "root_location");
      best.brlen_ratio = alpha[k];
      best_llh = llh[k];
    }
  }
  if (n_results == 0) die("no candidate root was evaluated");

  // ---- site lnLs of every candidate at its own parameters, .sitelh, RELL support
  std::vector<double> bp, elw, p_kh, p_sh, p_wsh, p_au;
  double site_seconds = 0.0, rell_seconds = 0.0;
  if (site_support) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<rdamd_root_location_t> rls(n_results);
    std::vector<uint64_t> counts;
    std::vector<double> values;
    for (unsigned i = 0; i < n_results; ++i) {
      uint64_t id = 0, nv = 0;
      double l = 0, a = 0;
      unsigned np = 0;
      need(rdamd_checkpoint_result(ckp, i, &id, &l, &a, &np, &nv), "checkpoint result");
      const size_t c0 = counts.size(), v0 = values.size();
      counts.resize(c0 + 4 * (size_t)np);
      values.resize(v0 + nv + 1);
      need(rdamd_checkpoint_result_params(ckp, i, counts.data() + c0, values.data() + v0), "checkpoint result_params");
      values.resize(v0 + nv);
      need(rdamd_tree_root_location(tree, (unsigned)ids[i], &rls[i]), "root_location");
      rls[i].brlen_ratio = alpha[i];
    }
    values.push_back(0.0);   // (never empty)
    unsigned P = 0, columns = 0;
    need(rdamd_model_site_patterns(model, &P, &columns, nullptr, nullptr), "site_patterns");
    std::vector<unsigned> weights(P), pattern_of(columns);
    need(rdamd_model_site_patterns(model, nullptr, nullptr, weights.data(), pattern_of.data()), "site_patterns");
    std::vector<double> lnls((size_t)n_results * P);
    need(rdamd_model_site_lnls(model, n_results, rls.data(), counts.data(), values.data(), lnls.data()), "site_lnls");
    // the log keeps a candidate's BEST lnL but its LAST parameters: say when they are not one iterate's
    unsigned off = 0;
    for (unsigned i = 0; i < n_results; ++i) {
      double total = 0.0;
      for (unsigned p = 0; p < P; ++p) total += weights[p] * lnls[(size_t)i * P + p];
      if (!(std::fabs(total - llh[i]) <= o.atol)) ++off;
    }
    if (off)
      std::cerr << off << " of " << n_results << " candidates: the lnL re-evaluated from the recorded parameters "
                << "differs from the recorded lnL by more than --atol (the record keeps the best iterate's lnL and "
                << "the last iterate's parameters)\n";
    site_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (o.site_lh) {
      std::FILE *f = std::fopen((o.prefix + ".sitelh").c_str(), "w");
      if (!f) die("could not write " + o.prefix + ".sitelh");
      std::fprintf(f, "%u %u\n", n_results, columns);
      for (unsigned i = 0; i < n_results; ++i) {
        std::fprintf(f, "root%llu", (unsigned long long)ids[i]);
        for (unsigned c = 0; c < columns; ++c) std::fprintf(f, " %.17g", lnls[(size_t)i * P + pattern_of[c]]);
        std::fputc('\n', f);
      }
      std::fclose(f);
    }
    if (o.rell_given) {
      const auto t1 = std::chrono::steady_clock::now();
      bp.assign(n_results, 0.0);
      elw.assign(n_results, 0.0);
      if (o.root_tests) {
        p_kh.assign(n_results, 0.0);
        p_sh.assign(n_results, 0.0);
        p_wsh.assign(n_results, 0.0);
        need(rdamd_rell_tests(lnls.data(), n_results, P, weights.data(), (unsigned)o.rell, o.rell_seed, nullptr,
                              bp.data(), elw.data(), p_kh.data(), p_sh.data(), p_wsh.data(), nullptr, nullptr),
             "rell_tests");
      } else {
        need(rdamd_rell_bootstrap(lnls.data(), n_results, P, weights.data(), (unsigned)o.rell, o.rell_seed, bp.data(),
                                  elw.data(), nullptr), "rell_bootstrap");
      }
      // the AU test: B replicates at each of the ten scales 0.5 .. 1.4, then the fit on the host
      std::vector<double> au_se, au_d, au_c, au_rss;
      std::vector<unsigned> au_used;
      if (o.au) {
        std::vector<uint64_t> n_draws(10);
        for (unsigned k = 0; k < 10; ++k) n_draws[k] = ((uint64_t)columns * (5 + k) + 5) / 10;
        std::vector<unsigned> counts((size_t)10 * n_results);
        need(rdamd_rell_multiscale(lnls.data(), n_results, P, weights.data(), 10, n_draws.data(), (unsigned)o.rell,
                                   o.rell_seed, counts.data(), nullptr), "rell_multiscale");
        p_au.assign(n_results, 0.0);
        au_se.assign(n_results, 0.0);
        au_d.assign(n_results, 0.0);
        au_c.assign(n_results, 0.0);
        au_rss.assign(n_results, 0.0);
        au_used.assign(n_results, 0u);
        need(rdamd_au_fit(counts.data(), 10, n_results, n_draws.data(), columns, (unsigned)o.rell, p_au.data(),
                          au_d.data(), au_c.data(), au_rss.data(), au_se.data(), au_used.data()), "au_fit");
      }
      rell_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
      double mx = -INFINITY, total = 0.0;
      for (unsigned i = 0; i < n_results; ++i) mx = std::max(mx, llh[i]);
      for (unsigned i = 0; i < n_results; ++i) total += std::exp(llh[i] - mx);
      std::vector<unsigned> by_id(n_results);
      for (unsigned i = 0; i < n_results; ++i) by_id[i] = i;
      std::stable_sort(by_id.begin(), by_id.end(), [&](unsigned a, unsigned b) { return ids[a] < ids[b]; });
      std::FILE *f = std::fopen((o.prefix + ".support.tsv").c_str(), "w");
      if (!f) die("could not write " + o.prefix + ".support.tsv");
      std::fprintf(f, "root_id\tllh\tlwr\tbp\telw\n");
      for (unsigned i : by_id)
        std::fprintf(f, "%llu\t%.17g\t%.17g\t%.17g\t%.17g\n", (unsigned long long)ids[i], llh[i],
                     std::exp(llh[i] - mx) / total, bp[i], elw[i]);
      std::fclose(f);
      if (o.au) {
        f = std::fopen((o.prefix + ".au.tsv").c_str(), "w");
        if (!f) die("could not write " + o.prefix + ".au.tsv");
        std::fprintf(f, "root_id\tllh\tp_au\tse\td\tc\trss\tdf\tused\n");
        for (unsigned i : by_id)
          std::fprintf(f, "%llu\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%u\t%u\n", (unsigned long long)ids[i],
                       llh[i], p_au[i], au_se[i], au_d[i], au_c[i], au_rss[i], au_used[i] >= 2 ? au_used[i] - 2 : 0u,
                       au_used[i]);
        std::fclose(f);
        if (!o.silent) {
          unsigned kept = 0;
          for (unsigned i = 0; i < n_results; ++i) kept += p_au[i] >= 0.05;
          std::cout << "AU test: " << kept << " of " << n_results << " roots kept at 0.05" << std::endl;
        }
      }
      if (o.root_tests) {
        // the 95 % ELW set: rows by decreasing elw, equal values by lower index, until the sum reaches 0.95
        std::vector<unsigned> by_elw(n_results);
        for (unsigned i = 0; i < n_results; ++i) by_elw[i] = i;
        std::stable_sort(by_elw.begin(), by_elw.end(), [&](unsigned a, unsigned b) { return elw[a] > elw[b]; });
        std::vector<int> in_set(n_results, 0);
        double running = 0.0;
        for (unsigned i : by_elw) {
          in_set[i] = 1;
          running += elw[i];
          if (running >= 0.95) break;
        }
        f = std::fopen((o.prefix + ".roottests.tsv").c_str(), "w");
        if (!f) die("could not write " + o.prefix + ".roottests.tsv");
        std::fprintf(f, "root_id\tllh\tlwr\tbp\telw\tp_kh\tp_sh\tp_wsh\tin_elw95\n");
        for (unsigned i : by_id)
          std::fprintf(f, "%llu\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%d\n", (unsigned long long)ids[i],
                       llh[i], std::exp(llh[i] - mx) / total, bp[i], elw[i], p_kh[i], p_sh[i], p_wsh[i], in_set[i]);
        std::fclose(f);
        if (!o.silent) {
          unsigned kh = 0, sh = 0, wsh = 0, in95 = 0;
          for (unsigned i = 0; i < n_results; ++i) {
            kh += p_kh[i] >= 0.05;
            sh += p_sh[i] >= 0.05;
            wsh += p_wsh[i] >= 0.05;
            in95 += in_set[i];
          }
          std::cout << "Root tests: of " << n_results << " roots, not rejected at 0.05 by KH " << kh << ", SH " << sh
                    << ", WSH " << wsh << "; 95% ELW set " << in95 << std::endl;
        }
      }
    }
  }
  // the parameters of the record `best` was taken from, in the checkpoint's layout
  const auto best_record_params = [&](std::vector<uint64_t> &counts, std::vector<double> &values) {
    unsigned k = 0;
    for (unsigned i = 1; i < n_results; ++i)
      if (llh[i] > llh[k]) k = i;
    uint64_t id = 0, nv = 0;
    double l = 0, a = 0;
    unsigned np = 0;
    need(rdamd_checkpoint_result(ckp, k, &id, &l, &a, &np, &nv), "checkpoint result");
    counts.assign(4 * (size_t)np, 0);
    values.assign(nv + 1, 0.0);
    need(rdamd_checkpoint_result_params(ckp, k, counts.data(), values.data()), "checkpoint result_params");
  };
  // ---- what the best root implies: ancestral states and site rates at its own parameters
  if (o.ancestral || o.site_rates) {
    std::vector<uint64_t> counts;
    std::vector<double> values;
    best_record_params(counts, values);
    unsigned P = 0, columns = 0;
    need(rdamd_model_site_patterns(model, &P, &columns, nullptr, nullptr), "site_patterns");
    std::vector<unsigned> pattern_of(columns);
    need(rdamd_model_site_patterns(model, nullptr, nullptr, nullptr, pattern_of.data()), "site_patterns");
    const unsigned n_parts = (unsigned)rdamd_model_partition_count(model), K = o.states;
    std::vector<unsigned> part_columns(n_parts), part_cats(n_parts);
    size_t cat_doubles = 0;
    unsigned max_cats = 1;
    for (unsigned p = 0; p < n_parts; ++p) {
      unsigned patterns = 0;
      need(rdamd_model_partition_shape(model, p, &patterns, &part_columns[p], &part_cats[p]), "partition_shape");
      cat_doubles += (size_t)patterns * part_cats[p];
      max_cats = std::max(max_cats, part_cats[p]);
    }
    unsigned n_nodes = rdamd_tree_tip_count(tree) - 1;
    std::vector<unsigned> node_clv(n_nodes);
    std::vector<double> post(o.ancestral ? (size_t)n_nodes * P * K : 0), cat(o.site_rates ? cat_doubles + 1 : 0),
        mean(o.site_rates ? P : 0);
    need(rdamd_model_ancestral(model, &best, counts.data(), values.data(), &n_nodes, node_clv.data(), nullptr, nullptr,
                               o.ancestral ? post.data() : nullptr, o.site_rates ? cat.data() : nullptr,
                               o.site_rates ? mean.data() : nullptr), "ancestral");
    std::string files;
    if (o.ancestral) {
      const char *letters = K == 2 ? "01" : "ACGT";
      std::FILE *f = std::fopen((o.prefix + ".ancestral.tsv").c_str(), "w");
      if (!f) die("could not write " + o.prefix + ".ancestral.tsv");
      std::fprintf(f, "node\tpartition\tcolumn\tstate");
      for (unsigned j = 0; j < K; ++j) std::fprintf(f, "\tp_%c", letters[j]);
      std::fputc('\n', f);
      for (unsigned v = 0; v < n_nodes; ++v) {
        size_t col = 0;   // column of the concatenated partitions
        for (unsigned p = 0; p < n_parts; ++p)
          for (unsigned c = 0; c < part_columns[p]; ++c, ++col) {
            const double *row = post.data() + ((size_t)v * P + pattern_of[col]) * K;
            unsigned top = 0;
            for (unsigned j = 1; j < K; ++j)
              if (row[j] > row[top]) top = j;   // the first state with the largest posterior
            std::fprintf(f, "N%u\t%u\t%u\t%c", v, p, c + 1, letters[top]);
            for (unsigned j = 0; j < K; ++j) std::fprintf(f, "\t%.6f", row[j]);
            std::fputc('\n', f);
          }
      }
      std::fclose(f);
      rdamd_tree_t *named = rdamd_tree_from_file(o.tree.c_str());
      if (!named) die(rdamd_errmsg());
      rdamd_root_location_t rl;
      need(rdamd_tree_root_location(named, (unsigned)best.id, &rl), "root_location");
      rl.brlen_ratio = best.brlen_ratio;
      need(rdamd_tree_root_by(named, &rl), "root_by");
      char *nw = rdamd_tree_newick_ancestral(named, n_nodes, node_clv.data());
      if (!nw) die(rdamd_errmsg());
      std::ofstream(o.prefix + ".ancestral.tree") << nw;
      std::free(nw);
      rdamd_tree_destroy(named);
      files = o.prefix + ".ancestral.tsv " + o.prefix + ".ancestral.tree";
    }
    if (o.site_rates) {
      std::FILE *f = std::fopen((o.prefix + ".siterates.tsv").c_str(), "w");
      if (!f) die("could not write " + o.prefix + ".siterates.tsv");
      std::fprintf(f, "partition\tcolumn\tmean_rate\tcategory");
      for (unsigned r = 0; r < max_cats; ++r) std::fprintf(f, "\tp_%u", r + 1);
      std::fputc('\n', f);
      size_t col = 0, pat0 = 0, cat0 = 0;   // first column / pattern / category posterior of the partition
      for (unsigned p = 0; p < n_parts; ++p) {
        unsigned patterns = 0;
        need(rdamd_model_partition_shape(model, p, &patterns, nullptr, nullptr), "partition_shape");
        const unsigned R = part_cats[p];
        for (unsigned c = 0; c < part_columns[p]; ++c, ++col) {
          const size_t pat = pattern_of[col];
          const double *row = cat.data() + cat0 + (pat - pat0) * R;
          unsigned top = 0;
          for (unsigned r = 1; r < R; ++r)
            if (row[r] > row[top]) top = r;
          std::fprintf(f, "%u\t%u\t%.6f\t%u", p, c + 1, mean[pat], top + 1);
          for (unsigned r = 0; r < R; ++r) std::fprintf(f, "\t%.6f", row[r]);
          std::fputc('\n', f);
        }
        pat0 += patterns;
        cat0 += (size_t)patterns * R;
      }
      std::fclose(f);
      files += (files.empty() ? "" : " ") + o.prefix + ".siterates.tsv";
    }
    if (!o.silent) std::cout << "Ancestral reconstruction at root " << best.id << " written to: " << files << std::endl;
  }
  // ---- the ML branch lengths at the best root and its own parameters
  if (o.branch_lengths) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> counts;
    std::vector<double> values;
    best_record_params(counts, values);
    unsigned n_nodes = rdamd_tree_tip_count(tree) - 1;
    std::vector<unsigned> node_clv(n_nodes), node_children(2 * (size_t)n_nodes);
    std::vector<double> input(2 * (size_t)n_nodes), lengths(input.size()), d1(input.size()), d2(input.size());
    need(rdamd_model_branch_derivatives(model, &best, counts.data(), values.data(), &n_nodes, node_clv.data(), nullptr,
                                        node_children.data(), input.data(), nullptr, nullptr, nullptr),
         "branch_derivatives");
    double before = 0.0, after = 0.0;
    unsigned iterations = 0, evaluations = 0;
    int converged = 0;
    need(rdamd_model_optimize_branch_lengths(model, &best, counts.data(), values.data(), o.brlen_min, o.brlen_max, 1e-8,
                                             200, lengths.data(), d1.data(), d2.data(), &before, &after, &iterations,
                                             &evaluations, &converged),
         "optimize_branch_lengths");
    std::FILE *f = std::fopen((o.prefix + ".brlen.tsv").c_str(), "w");
    if (!f) die("could not write " + o.prefix + ".brlen.tsv");
    std::fprintf(f, "node\tchild\tname\tinput_length\tlength\td1\td2\tat_bound\n");
    for (unsigned v = 0; v < n_nodes; ++v)
      for (unsigned c = 0; c < 2; ++c) {
        const size_t b = 2 * (size_t)v + c;
        std::string name;
        const auto inner = std::find(node_clv.begin(), node_clv.end(), node_children[b]);
        if (inner != node_clv.end()) name = "N" + std::to_string(inner - node_clv.begin());
        else name = rdamd_tree_tip_label(tree, node_children[b]);
        const char *bound = lengths[b] <= o.brlen_min ? "min" : lengths[b] >= o.brlen_max ? "max" : "no";
        std::fprintf(f, "N%u\t%u\t%s\t%.10f\t%.10f\t%.6e\t%.6e\t%s\n", v, c, name.c_str(), input[b], lengths[b], d1[b],
                     d2[b], bound);
      }
    std::fclose(f);
    rdamd_tree_t *rooted = rdamd_tree_from_file(o.tree.c_str());
    if (!rooted) die(rdamd_errmsg());
    rdamd_root_location_t rl;
    need(rdamd_tree_root_location(rooted, (unsigned)best.id, &rl), "root_location");
    rl.brlen_ratio = best.brlen_ratio;
    need(rdamd_tree_root_by(rooted, &rl), "root_by");
    char *nw = rdamd_tree_newick_branch_lengths(rooted, n_nodes, node_clv.data(), lengths.data());
    if (!nw) die(rdamd_errmsg());
    std::ofstream(o.prefix + ".brlen.tree") << nw;
    std::free(nw);
    rdamd_tree_destroy(rooted);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    char line[512];
    std::snprintf(line, sizeof line, "Branch lengths at root %llu: lnL before %.6f, after %.6f, iterations %u, evaluations %u, "
                  "converged %d, %.3f s; written to: %s.brlen.tsv %s.brlen.tree", (unsigned long long)best.id, before, after,
                  iterations, evaluations, converged, seconds, o.prefix.c_str(), o.prefix.c_str());
    std::cout << line << std::endl;
  }
  // ---- the exact gradient at the best record, beside the forward difference the search took there
  if (o.gradient) {
    std::vector<uint64_t> counts;
    std::vector<double> values;
    best_record_params(counts, values);
    const size_t n_parts = counts.size() / 4;
    size_t n_values = 0;
    for (uint64_t c : counts) n_values += c;
    std::vector<double> grad(n_values + 1, 0.0);
    double lnl = 0.0;
    need(rdamd_model_gradient(model, &best, counts.data(), values.data(), grad.data(), &lnl), "gradient");
    // the optimiser's box and step (model.cpp, optimize_params): rates, frequencies, alpha; weights are not searched
    const char *field[4] = {"subst_rate", "freq", "alpha", "weight"};
    const double lo[4] = {1e-4, 1e-4, 0.2, -INFINITY}, hi[4] = {1e4, 1.0 - 1e-4 * 3, 10000.0, INFINITY};
    std::FILE *f = std::fopen((o.prefix + ".gradient.tsv").c_str(), "w");
    if (!f) die("could not write " + o.prefix + ".gradient.tsv");
    std::fprintf(f, "partition\tname\tvalue\tgradient\tforward_difference\tat_bound\n");
    double worst = 0.0;
    std::string worst_name = "-";
    size_t at = 0;
    for (size_t p = 0; p < n_parts; ++p)
      for (unsigned k = 0; k < 4; ++k)
        for (uint64_t i = 0; i < counts[4 * p + k]; ++i, ++at) {
          const double x = values[at], g = grad[at], h = std::max(1e-4 * std::fabs(x), 1e-4);
          std::vector<double> moved(values);
          moved[at] = x + h;
          double up = 0.0;
          need(rdamd_model_branch_derivatives(model, &best, counts.data(), moved.data(), nullptr, nullptr, nullptr, nullptr,
                                              nullptr, nullptr, nullptr, &up), "lnL at a moved parameter");
          const char *bound = x <= lo[k] ? "min" : x >= hi[k] ? "max" : "no";
          // a component that points out of the box at a bound is not a direction the optimiser has (it maximises lnL)
          const double projected = (x <= lo[k] && g < 0.0) || (x >= hi[k] && g > 0.0) ? 0.0 : g;
          const std::string name = std::string(field[k]) + "_" + std::to_string(i);
          if (std::fabs(projected) > std::fabs(worst)) { worst = projected; worst_name = "partition " + std::to_string(p) + " " + name; }
          std::fprintf(f, "%zu\t%s\t%.17g\t%.17g\t%.10e\t%s\n", p, name.c_str(), x, g, (up - lnl) / h, bound);
        }
    std::fclose(f);
    char line[512];
    std::snprintf(line, sizeof line, "Gradient at root %llu: lnL %.6f, %zu parameters, largest projected component %.6e (%s); "
                  "written to: %s.gradient.tsv", (unsigned long long)best.id, lnl, n_values, worst, worst_name.c_str(),
                  o.prefix.c_str());
    std::cout << line << std::endl;
  }
  // ---- substitutions mapped onto the branches at the best record's root and parameters
  if (o.substitutions) {
    std::vector<uint64_t> counts;
    std::vector<double> values;
    best_record_params(counts, values);
    unsigned P = 0, columns = 0;
    need(rdamd_model_site_patterns(model, &P, &columns, nullptr, nullptr), "site_patterns");
    std::vector<unsigned> weights(P), pattern_of(columns);
    need(rdamd_model_site_patterns(model, nullptr, nullptr, weights.data(), pattern_of.data()), "site_patterns");
    const unsigned n_parts = (unsigned)rdamd_model_partition_count(model), K = o.states;
    std::vector<unsigned> part_columns(n_parts);
    for (unsigned p = 0; p < n_parts; ++p)
      need(rdamd_model_partition_shape(model, p, nullptr, &part_columns[p], nullptr), "partition_shape");
    unsigned n_nodes = rdamd_tree_tip_count(tree) - 1;
    const size_t branches = 2 * (size_t)n_nodes, cells = branches * P;
    std::vector<unsigned> node_clv(n_nodes), node_children(branches);
    std::vector<double> lengths(branches), typed((size_t)n_parts * branches * K * K), change(cells), count(cells), top_prob(cells);
    std::vector<unsigned char> top_pair(cells);
    double lnl = 0.0;
    need(rdamd_model_substitutions(model, &best, counts.data(), values.data(), &n_nodes, node_clv.data(), nullptr,
                                   node_children.data(), lengths.data(), typed.data(), change.data(), count.data(),
                                   top_pair.data(), top_prob.data(), &lnl), "substitutions");
    const char *letters = K == 2 ? "01" : "ACGT";
    std::vector<std::string> name(branches);
    for (size_t b = 0; b < branches; ++b) {
      const auto inner = std::find(node_clv.begin(), node_clv.end(), node_children[b]);
      name[b] = inner != node_clv.end() ? "N" + std::to_string(inner - node_clv.begin())
                                        : std::string(rdamd_tree_tip_label(tree, node_children[b]));
    }
    std::FILE *f = std::fopen((o.prefix + ".substitutions.tsv").c_str(), "w");
    if (!f) die("could not write " + o.prefix + ".substitutions.tsv");
    std::fprintf(f, "node\tchild\tname\tlength\texpected_total");
    for (unsigned i = 0; i < K; ++i)
      for (unsigned j = 0; j < K; ++j)
        if (i != j) std::fprintf(f, "\t%c>%c", letters[i], letters[j]);
    for (unsigned i = 0; i < K; ++i) std::fprintf(f, "\tdwell_%c", letters[i]);
    std::fprintf(f, "\tchange_probability_sum\n");
    double all = 0.0;
    for (size_t b = 0; b < branches; ++b) {
      std::vector<double> sum((size_t)K * K, 0.0);   // the partitions in partition order
      for (unsigned p = 0; p < n_parts; ++p)
        for (size_t e = 0; e < (size_t)K * K; ++e) sum[e] += typed[((size_t)p * branches + b) * K * K + e];
      double total = 0.0, changed = 0.0;
      for (unsigned i = 0; i < K; ++i)
        for (unsigned j = 0; j < K; ++j)
          if (i != j) total += sum[i * K + j];
      for (unsigned s = 0; s < P; ++s) changed += weights[s] * change[b * P + s];
      all += total;
      std::fprintf(f, "N%zu\t%zu\t%s\t%.10f\t%.17g", b / 2, b % 2, name[b].c_str(), lengths[b], total);
      for (unsigned i = 0; i < K; ++i)
        for (unsigned j = 0; j < K; ++j)
          if (i != j) std::fprintf(f, "\t%.17g", sum[i * K + j]);
      for (unsigned i = 0; i < K; ++i) std::fprintf(f, "\t%.17g", sum[i * K + i]);
      std::fprintf(f, "\t%.17g\n", changed);
    }
    std::fclose(f);
    f = std::fopen((o.prefix + ".mutations.tsv").c_str(), "w");
    if (!f) die("could not write " + o.prefix + ".mutations.tsv");
    std::fprintf(f, "node\tchild\tname\tpartition\tcolumn\tfrom\tto\tprobability\texpected_count\n");
    size_t listed = 0;
    for (size_t b = 0; b < branches; ++b) {
      size_t col = 0;   // column of the concatenated partitions
      for (unsigned p = 0; p < n_parts; ++p)
        for (unsigned c = 0; c < part_columns[p]; ++c, ++col) {
          const size_t at = b * P + pattern_of[col];
          if (!(top_prob[at] >= o.subst_min_prob)) continue;
          std::fprintf(f, "N%zu\t%zu\t%s\t%u\t%u\t%c\t%c\t%.17g\t%.17g\n", b / 2, b % 2, name[b].c_str(), p, c + 1,
                       letters[top_pair[at] / K], letters[top_pair[at] % K], top_prob[at], count[at]);
          ++listed;
        }
    }
    std::fclose(f);
    rdamd_tree_t *named = rdamd_tree_from_file(o.tree.c_str());
    if (!named) die(rdamd_errmsg());
    rdamd_root_location_t rl;
    need(rdamd_tree_root_location(named, (unsigned)best.id, &rl), "root_location");
    rl.brlen_ratio = best.brlen_ratio;
    need(rdamd_tree_root_by(named, &rl), "root_by");
    char *nw = rdamd_tree_newick_ancestral(named, n_nodes, node_clv.data());
    if (!nw) die(rdamd_errmsg());
    std::ofstream(o.prefix + ".substitutions.tree") << nw;
    std::free(nw);
    rdamd_tree_destroy(named);
    char line[640];
    std::snprintf(line, sizeof line, "Substitutions at root %llu: lnL %.6f, %.6f expected on %zu branches, %zu mutations with "
                  "probability >= %g; written to: %s.substitutions.tsv %s.mutations.tsv %s.substitutions.tree",
                  (unsigned long long)best.id, lnl, all, branches, listed, o.subst_min_prob, o.prefix.c_str(), o.prefix.c_str(),
                  o.prefix.c_str());
    std::cout << line << std::endl;
  }
  rdamd_tree_t *out = rdamd_tree_from_file(o.tree.c_str());
  std::string final_tree;
  if (o.exhaustive) {
    double mx = -INFINITY, total = 0.0;
    for (unsigned i = 0; i < n_results; ++i) mx = std::max(mx, llh[i]);
    for (unsigned i = 0; i < n_results; ++i) total += std::exp(llh[i] - mx);
    for (unsigned i = 0; i < n_results; ++i) {
      rdamd_root_location_t rl;
      need(rdamd_tree_root_location(out, (unsigned)ids[i], &rl), "root_location");
      rl.brlen_ratio = alpha[i];
      rdamd_tree_annotate_branch(out, &rl, "LWR", std::to_string(std::exp(llh[i] - mx) / total).c_str());
      if (!bp.empty()) {
        rdamd_tree_annotate_branch(out, &rl, "BP", std::to_string(bp[i]).c_str());
        rdamd_tree_annotate_branch(out, &rl, "ELW", std::to_string(elw[i]).c_str());
        if (!p_kh.empty()) {
          rdamd_tree_annotate_branch(out, &rl, "pKH", std::to_string(p_kh[i]).c_str());
          rdamd_tree_annotate_branch(out, &rl, "pSH", std::to_string(p_sh[i]).c_str());
          rdamd_tree_annotate_branch(out, &rl, "pWSH", std::to_string(p_wsh[i]).c_str());
        }
        if (!p_au.empty()) rdamd_tree_annotate_branch(out, &rl, "pAU", std::to_string(p_au[i]).c_str());
      }
      rdamd_tree_annotate_branch(out, &rl, "LLH", std::to_string(llh[i]).c_str());
      rdamd_tree_annotate_branch_lr(out, &rl, "alpha", std::to_string(alpha[i]).c_str(),
                                    std::to_string(1 - alpha[i]).c_str());
    }
  }
  rdamd_root_location_t final_rl;
  need(rdamd_tree_root_location(out, (unsigned)best.id, &final_rl), "root_location");
  final_rl.brlen_ratio = best.brlen_ratio;
  if (o.exhaustive) {   // virtual_rooted_tree(final_rl).newick(): rooted there, then unrooted again
    need(rdamd_tree_root_by(out, &final_rl), "root_by");
    rdamd_tree_unroot(out);
    char *nw = rdamd_tree_newick(out, 1);
    final_tree = nw;
    std::free(nw);
    std::ofstream(o.prefix + ".lwr.tree") << final_tree;
  }
  need(rdamd_tree_root_by(out, &final_rl), "root_by");
  {
    char *nw = rdamd_tree_newick(out, 0);
    std::ofstream(o.prefix + ".rooted.tree") << nw;
    if (!o.exhaustive) final_tree = nw;
    std::free(nw);
  }
  if (!o.silent) std::printf("Final LogLH: %.5f\n", best_llh);
  std::cout << final_tree << std::endl;
  if (!o.silent && site_support) {
    std::cout << "Search took: " << search_took.count() << "s" << std::endl;
    std::cout << "Site lnLs took: " << site_seconds << "s" << std::endl;
    if (o.rell_given) std::cout << "RELL bootstrap took: " << rell_seconds << "s" << std::endl;
  }
  if (!o.silent) {
    const std::chrono::duration<double> took = std::chrono::steady_clock::now() - start;
    std::cout << "Inference took: " << took.count() << "s" << std::endl;
  }
  rdamd_tree_destroy(out);
  rdamd_model_destroy(model);
  if (comm) rdamd_comm_destroy(comm);
  rdamd_tree_destroy(tree);
  if (ckp) rdamd_checkpoint_close(ckp);
  return 0;
}
