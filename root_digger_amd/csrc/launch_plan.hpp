// Which instantiation of the fused 4-state evaluator a batch gets (kernels_fused.hip,
// fused_dna_eval_kernel<NS, TTCHECK, RL, TR, RW, SP, EXPORT, SPEC>): sites per lane, one wave per
// rate category, the XCD mapping, speculation, and per pass the kind of stack and the LDS bytes of
// the launch.  One pure function over plain numbers -- no HIP call, no partition, no environment --
// that tests/cpp/host_logic_check.cpp runs without a GPU.  It restates, in one place, the choices
// that rdamd_evaluate_batch (evaluate.hip) and launch_fused_variant_rl (kernels_fused.hip) make
// today, and adds one: one wave per rate category is dropped where R waves would pass a
// workgroup's LDS.  THE LIBRARY DOES NOT CALL IT YET -- evaluate.hip and kernels_fused.hip still
// decide for themselves --: keep the two in step until the launch path takes its shape from here.
// The thresholds' measurements are with the kernels they belong to and in DESIGN.md 4.1.
#pragma once

#include <algorithm>
#include <cstddef>

namespace rdamd {

// LDS a workgroup can have on gfx950 (one CU's 160 KB)
constexpr size_t kFusedLdsLimit = 160u * 1024u;
// in-memory stack entries up to which a 64-row program takes the private-segment stack
// (fused.hpp, kFusedSpillLevels; host_logic_check.cpp asserts that the two agree)
constexpr unsigned kPlanSpillLevels = 7;
// tips up to which a partition speculates by default (include/root_digger_amd.h,
// rdamd_partition_set_rescale_speculation; evaluate.hip, kSpeculateTips)
constexpr unsigned kPlanSpeculateTips = 256;

// why a forced value (FusedLaunchInput::force_*) was not taken, or the rule's own choice changed:
// bits of FusedLaunchShape::not_honoured
enum : unsigned {
  kLaunchRwRates = 1u,       // one wave per rate category was forced, but R is outside 2..8
  kLaunchRwSpeculate = 2u,   // ... but the launch speculates (one-wave workgroups)
  kLaunchRwExport = 4u,      // ... but the launch exports the root's children
  kLaunchRwLds = 8u,         // ... but R waves' table slots and stacks pass the LDS limit
  kLaunchRuleRwLds = 16u,    // nothing was forced: the RULE wanted one wave per rate and the LDS limit said no
  kLaunchNsExport = 32u,     // two sites per lane were forced on an exporting launch (one job: one site per lane)
  kLaunchJobMajorExport = 64u,   // whole jobs per XCD were forced on an exporting launch
};

struct FusedLaunchInput {
  unsigned rate_cats = 1, n_jobs = 0;
  unsigned blocks_x = 0;              // 64-site blocks per job, padded (ensure_workspace)
  size_t tipcodes_bytes = 0;          // the code arena the launch reads, rows in use
  size_t table_bytes_per_job = 0;     // a job's tip and pseudo-tip tables
  unsigned table_rows = 16;           // 16 or 64: TR
  unsigned max_depth[2] = {1, 1};     // in-memory stack levels: [0] programs with pseudo-tips, [1] plain programs
  unsigned reg_levels[2] = {1, 1};    // register levels they were compiled for
  int speculation = -1;               // the partition's mode: -1 by tip count, 0 off, 1 on
  unsigned tips = 0;
  bool export_children = false;       // rdamd_evaluate_root_children: one job, plain program, pass [1] only
  int force_ns = -1, force_rw = -1, force_job_major = -1;   // -1: the rule; 1 | 2, 0 | 1, 0 | 1
  unsigned spill_min = 2;             // smallest in-memory depth that takes the private-segment stack
  size_t lds_limit = kFusedLdsLimit;
};

struct FusedPassShape {
  unsigned reg_levels = 1;   // RL: 1 or 2
  unsigned mem_levels = 1;   // in-memory stack levels of the launch's deepest program
  unsigned spill = 0;        // SP: kPlanSpillLevels with the private-segment stack (one LDS level then), 0 all-LDS
  unsigned lds_levels = 1;   // stack levels a wave has in LDS
  size_t lds_bytes = 0;      // dynamic LDS of the launch
};

struct FusedLaunchShape {
  unsigned sites_per_lane = 1, rates_across_waves = 0, job_major = 0, speculate = 0;
  FusedPassShape pass[2];   // [0] first pass, [1] second pass (plain programs, TTCHECK; the exporting launch)
  unsigned not_honoured = 0;
};

// LDS one wave of the evaluator needs: its two table slots (8 TR doubles) and `lds_levels` stack
// levels of NS x 64 entries (four doubles and a rescale count each)
inline size_t fused_lds_per_wave(unsigned table_rows, unsigned ns, unsigned lds_levels) {
  return (size_t)8 * table_rows * sizeof(double) + (size_t)lds_levels * ns * 64 * (4 * sizeof(double) + sizeof(int));
}

// the stack of one pass and the LDS bytes of its launch
inline FusedPassShape fused_pass_shape(unsigned table_rows, unsigned ns, unsigned n_waves, unsigned max_depth,
                                       unsigned reg_levels, unsigned spill_min = 2) {
  FusedPassShape s;
  // two or more stack levels behind the register one: one in LDS, the rest in the private segment
  // -- for the kernels with 64-row table slots (kernels_fused.hip, SP)
  const bool spill = table_rows > 16 && reg_levels < 2 && max_depth >= spill_min && max_depth <= kPlanSpillLevels;
  s.reg_levels = !spill && reg_levels >= 2 ? 2u : 1u;
  s.mem_levels = max_depth;
  s.spill = spill ? kPlanSpillLevels : 0u;
  s.lds_levels = spill || !max_depth ? 1u : max_depth;
  // (one wave per rate: at least the room the rate terms need when they meet: R x NS x 64 x 12 bytes)
  s.lds_bytes = std::max<size_t>(fused_lds_per_wave(table_rows, ns, s.lds_levels) * n_waves, (size_t)n_waves * ns * 64 * 12);
  return s;
}

inline FusedLaunchShape plan_fused_launch(const FusedLaunchInput &in) {
  FusedLaunchShape out;
  const unsigned R = in.rate_cats;
  // two sites per lane when half the waves still fill the chip: >= 4 waves for each of the 1024 SIMDs
  unsigned ns = (size_t)in.n_jobs * in.blocks_x >= 8192 ? 2u : 1u;
  if (in.force_ns == 1 || in.force_ns == 2) ns = (unsigned)in.force_ns;
  // one wave per rate category where re-reading the code arena once per rate pass is what
  // hurts: when it is far beyond every cache level
  const bool rw_legal_r = R >= 2 && R <= 8;
  bool rw = rw_legal_r && in.tipcodes_bytes >= ((size_t)512 << 20);
  const bool rw_forced = in.force_rw == 0 || in.force_rw == 1;
  if (rw_forced) {
    rw = in.force_rw == 1;
    if (rw && !rw_legal_r) {
      rw = false;
      out.not_honoured |= kLaunchRwRates;
    }
  }
  // whole jobs per XCD once the tables of the jobs that are on the device together outgrow the L2s
  const double jobs_in_flight = 4096.0 / std::max(1u, in.blocks_x / 2u);   // ~16 one-wave workgroups on 256 CUs
  bool job_major = in.n_jobs >= 16 && jobs_in_flight * (double)in.table_bytes_per_job > 16.0 * (1 << 20);
  if (in.force_job_major == 0 || in.force_job_major == 1) job_major = in.force_job_major == 1;
  // the speculative kernels are one-wave workgroups
  bool speculate = in.speculation < 0 ? in.tips <= kPlanSpeculateTips : in.speculation > 0;
  if (in.export_children) {
    // one job through the exporting variant: one site per lane, all-LDS stack, every rescale test
    if (rw && rw_forced) out.not_honoured |= kLaunchRwExport;
    if (in.force_ns == 2) out.not_honoured |= kLaunchNsExport;
    if (in.force_job_major == 1) out.not_honoured |= kLaunchJobMajorExport;
    ns = 1;
    rw = job_major = speculate = false;
  }
  if (speculate) {
    if (rw && rw_forced) out.not_honoured |= kLaunchRwSpeculate;
    rw = false;
  }
  if (rw) {
    // R waves' slots and stacks in one workgroup: both passes must fit (the second one is only
    // known to be needed when the first has run)
    size_t most = 0;
    for (int k = 0; k < 2; ++k)
      most = std::max(most, fused_pass_shape(in.table_rows, ns, R, in.max_depth[k], in.reg_levels[k], in.spill_min).lds_bytes);
    if (most > in.lds_limit) {
      rw = false;
      out.not_honoured |= rw_forced ? kLaunchRwLds : kLaunchRuleRwLds;
    }
  }
  out.sites_per_lane = ns;
  out.rates_across_waves = rw;
  out.job_major = job_major;
  out.speculate = speculate;
  for (int k = 0; k < 2; ++k)
    out.pass[k] = in.export_children ? fused_pass_shape(16, 1, 1, in.max_depth[1], in.reg_levels[1], ~0u)   // (never the private segment)
                                     : fused_pass_shape(in.table_rows, ns, rw ? R : 1u, in.max_depth[k], in.reg_levels[k], in.spill_min);
  return out;
}

}  // namespace rdamd
