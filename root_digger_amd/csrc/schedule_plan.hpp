// What rdamd_schedule_create (evaluate.hip) decides before it touches the device: whether the
// operation list is a full post-order traversal, how rdamd::Compiler is set up for the 4-state
// (16- and 64-row) and 20-state evaluators, which clades become pseudo-tips, and how the pieces
// are laid out in the schedule's one device block.  Pure host logic over plain numbers and
// rdamd_operation_t -- no HIP call, no partition, no environment -- so that
// tests/cpp/host_logic_check.cpp runs the recipe the kernels get without a GPU.
#pragma once

#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "clades.hpp"
#include "fused.hpp"
#include "traversal_compiler.hpp"

namespace rdamd {

using ClvMap = std::unordered_map<unsigned, unsigned>;   // keyed by CLV index

// ---- validation: a full post-order traversal ---------------------------------------------------
struct ScheduleCheck {
  enum Kind { kOk, kEmpty, kOperation, kBranch } kind = kOk;
  unsigned at = 0;             // kOperation: the first operation that is no part of a post-order traversal
                               // (an index out of range, a child not yet computed or used twice, a
                               // parent written twice); kBranch: the first bad entry of the branch list
  ClvMap producer;             // clv -> the operation that writes it
  std::vector<int> consumer;   // op -> the operation that takes its result (-1: the root operation)
  std::vector<double> brlen;   // [prob_matrices] the branch lengths by matrix index, 0 where none was given
  // A pseudo-tip's table is written into the tip-table slot of the branch above it
  // (kernels_clade.hip): that slot is only free when the branch's matrix index is used by this
  // one child.  The C ABI (like coraxlib's) lets a caller share a matrix index between
  // branches; such a list is evaluated without folding -- its tip tables are all code-indexed.
  bool matrix_shared = false;
};

inline ScheduleCheck validate_schedule(unsigned tips, unsigned clv_buffers, unsigned prob_matrices,
                                       const rdamd_operation_t *ops, unsigned n_ops, const unsigned *matrix_indices,
                                       const double *branch_lengths, unsigned n_matrices) {
  ScheduleCheck v;
  if (n_ops == 0) {
    v.kind = ScheduleCheck::kEmpty;
    return v;
  }
  const unsigned nclv = tips + clv_buffers;
  v.consumer.assign(n_ops, -1);
  for (unsigned i = 0; i < n_ops; ++i) {
    const rdamd_operation_t &o = ops[i];
    bool bad = o.parent_clv_index < tips || o.parent_clv_index >= nclv ||
               o.child1_clv_index >= nclv || o.child2_clv_index >= nclv ||
               o.child1_matrix_index >= prob_matrices || o.child2_matrix_index >= prob_matrices;
    for (unsigned ch : {o.child1_clv_index, o.child2_clv_index}) {
      if (ch < tips) continue;
      auto it = v.producer.find(ch);
      if (it == v.producer.end() || v.consumer[it->second] >= 0) bad = true;   // not yet computed / used twice
      else v.consumer[it->second] = (int)i;
    }
    if (v.producer.count(o.parent_clv_index)) bad = true;       // written twice
    if (bad) {
      v.kind = ScheduleCheck::kOperation;
      v.at = i;
      return v;
    }
    v.producer[o.parent_clv_index] = i;
  }
  v.brlen.assign(prob_matrices, 0.0);
  for (unsigned m = 0; m < n_matrices; ++m) {
    if (matrix_indices[m] >= prob_matrices || !(branch_lengths[m] >= 0.0) || !std::isfinite(branch_lengths[m])) {
      v.kind = ScheduleCheck::kBranch;
      v.at = m;
      return v;
    }
    v.brlen[matrix_indices[m]] = branch_lengths[m];
  }
  std::vector<unsigned char> uses(prob_matrices, 0);
  for (unsigned i = 0; i < n_ops; ++i)
    for (unsigned m : {ops[i].child1_matrix_index, ops[i].child2_matrix_index})
      if (uses[m]++) v.matrix_shared = true;
  return v;
}

// ---- one program from one operation list -------------------------------------------------------
struct ScheduleShape {
  unsigned tips = 0, sites = 0, tip_stride = 0, rate_cats = 0, prob_matrices = 0;
  bool k20 = false;         // the 20-state evaluator runs the program (kernels_fused_k20.hip)
  bool wide_mode = false;   // 4 states: 64-row table slots and the 16-bit code arena that goes with them
};

struct Program {
  std::vector<FusedOp> steps;
  unsigned depth = 1, reg_levels = 1, matvecs = 0;
};

// what host_logic_check replays: the compiler as the recipe left it, and place_levels' answer
struct ProgramTrace {
  Compiler c;
  unsigned runner_up = 0;
};

// `list` (its last operation the root) with the clades of pseudo_row / pseudo_wide folded into
// pseudo-tips.  Returns how many operations of the list the root operation does not reach; `out` is
// the program when that is 0.
inline unsigned compile_program(const ScheduleShape &sh, const std::vector<rdamd_operation_t> &list,
                                const ClvMap &pseudo_row, const ClvMap &pseudo_wide, Program &out,
                                ProgramTrace *trace = nullptr) {
  Compiler local;
  Compiler &c = trace ? trace->c : local;
  const bool k20 = sh.k20, wide_mode = sh.wide_mode;
  c.ops = list.data(); c.n_ops = (unsigned)list.size(); c.tips = sh.tips; c.sites = sh.sites;
  c.tip_stride = sh.tip_stride * (wide_mode ? 2u : 1u); c.rate_cats = sh.rate_cats;
  c.unit = sh.rate_cats * (k20 ? 3200u : 128u);
  c.split_park = k20;
  c.pseudo_row = pseudo_row;
  c.pseudo_wide = pseudo_wide;
  c.wide_base = 8u * sh.prob_matrices * sh.rate_cats * 16u;
  c.dma_offsets = !k20 && wide_mode;
  c.place_parks = !k20 && wide_mode;   // (the kernels of these programs: one register slot, one LDS slot, a private-segment stack)
  {   // the steps that compute the root operation's inner children (fused.hpp, 0x8000 / 0x10000)
    const rdamd_operation_t &root = list.back();
    if (root.child1_clv_index >= sh.tips) c.mark_clv[0] = root.child1_clv_index;
    if (root.child2_clv_index >= sh.tips) c.mark_clv[1] = root.child2_clv_index;
  }
  for (unsigned i = 0; i < c.n_ops; ++i) c.producer[list[i].parent_clv_index] = i;
  c.need.assign(c.n_ops, 0);
  c.compute_need(c.n_ops - 1);
  c.out.reserve(c.n_ops);
  c.emit(c.n_ops - 1, false, 0);
  // second pass: the register slot to the busiest stack level, the LDS slot to the runner-up
  // (traversal_compiler.hpp)
  // (two register levels: from 8 in-memory entries on where the kernel has private-segment
  // levels, i.e. 64-row table slots; from 3 on an all-LDS stack -- kernels_fused.hip)
  const unsigned runner_up = c.place_levels(k20 ? 0u : (wide_mode ? 1u + kFusedSpillLevels : 3u), kFusedSpillLevels - 1u);
  if (trace) trace->runner_up = runner_up;
  size_t n_real = 0;
  for (const FusedOp &f : c.out)
    if (!c.split_park || (f.flags & 3u) != kFusedPark) ++n_real;
  if (n_real != c.n_ops) return (unsigned)(c.n_ops - n_real);
  // LDS levels = stack depth minus the register levels (at least one is allocated)
  // (20 states: parking steps count as steps)
  // (parks placed one by one: the LDS slot + the private-segment entries)
  out.depth = !c.park_class.empty() ? 1u + c.mem_depth
                                    : std::max(1u, c.max_depth > c.reg_levels ? c.max_depth - c.reg_levels : 0);
  out.reg_levels = c.reg_levels;
  out.matvecs = c.matvecs;
  if (trace) out.steps = c.out;
  else out.steps = std::move(c.out);
  return 0;
}

// ---- subtree site repeats: which clades become pseudo-tips (clades.hpp) ------------------------
// A node is SMALL when the sites fall into at most class_limit classes below it; small is
// inherited downwards, so the small nodes form whole subtrees and the topmost small node
// of each is the pseudo-tip.  The root operation is never folded (a program has >= 1 step).
struct CladeSelection {
  std::vector<char> small;            // [op] folded away: inside a pseudo-tip, or one itself
  std::vector<CladeStep> steps;       // group by group, post-order inside a group; `pad` carries the node id
                                      // until the caller has uploaded the node's map
  std::vector<CladeGroup> groups;
  std::vector<unsigned> tip_ops;      // [group] the operation that is its pseudo-tip, ascending
  ClvMap pseudo_wide;                 // clv of a pseudo-tip with more than 16 classes -> its 64-row table slot
  unsigned n_wide = 0, clade_rows = 0;
  // the operations that stay in the folded program
  std::vector<rdamd_operation_t> kept(const rdamd_operation_t *ops) const {
    std::vector<rdamd_operation_t> list;
    for (size_t i = 0; i < small.size(); ++i)
      if (!small[i]) list.push_back(ops[i]);
    return list;
  }
};

// node_id / n_classes: by operation, the clade cache's id and class count of the node it computes
// (0 classes: more than the cache counts)
inline CladeSelection select_clades(const rdamd_operation_t *ops, unsigned n_ops, unsigned tips, const ScheduleCheck &v,
                                    const std::vector<unsigned> &node_id, const std::vector<unsigned> &n_classes,
                                    unsigned class_limit) {
  CladeSelection sel;
  sel.small.assign(n_ops, 0);
  // (a parent has at least as many classes as either child: small is inherited downwards
  // under any limit)
  for (unsigned i = 0; i + 1 < n_ops; ++i)
    sel.small[i] = !v.matrix_shared && n_classes[i] > 0 && n_classes[i] <= class_limit;
  // the branch above operation i: the matrix index its consumer uses for it
  auto mat_above = [&](unsigned i) {
    const rdamd_operation_t &c = ops[v.consumer[i]];
    return c.child1_clv_index == ops[i].parent_clv_index ? c.child1_matrix_index : c.child2_matrix_index;
  };
  for (unsigned i = 0; i + 1 < n_ops; ++i) {
    if (!sel.small[i] || sel.small[v.consumer[i]]) continue;     // not a pseudo-tip
    CladeGroup g;
    g.first = (unsigned)sel.steps.size();
    // post-order over the small subtree below i; local index = position inside the group
    auto walk = [&](auto &&self, unsigned j) -> unsigned {
      const rdamd_operation_t &o = ops[j];
      CladeStep st;
      memset(&st, 0, sizeof st);
      const unsigned ch[2] = {o.child1_clv_index, o.child2_clv_index};
      const unsigned mt[2] = {o.child1_matrix_index, o.child2_matrix_index};
      for (int k = 0; k < 2; ++k)
        st.src[k] = ch[k] < tips ? mt[k] : (0x80000000u | self(self, v.producer.at(ch[k])));
      st.n_classes = n_classes[j];
      st.out_mat = mat_above(j);
      st.last = j == i ? 1u : 0u;
      st.wide_slot = 0xffffffffu;
      if (j == i && n_classes[j] > 16) {
        st.wide_slot = sel.n_wide;
        sel.pseudo_wide[o.parent_clv_index] = sel.n_wide++;
      }
      st.pad = node_id[j];
      sel.clade_rows += n_classes[j];
      sel.steps.push_back(st);
      return (unsigned)sel.steps.size() - 1 - g.first;
    };
    walk(walk, i);
    g.count = (unsigned)sel.steps.size() - g.first;
    sel.groups.push_back(g);
    sel.tip_ops.push_back(i);
  }
  return sel;
}

// ---- the device block: [program | plain program | clade steps | clade groups | lengths | tip mask] ----
struct ScheduleBlock {
  size_t o_prog = 0, o_plain = 0, o_steps = 0, o_groups = 0, o_brlen = 0, o_tipmask = 0, total = 0;   // 64-byte aligned
  std::vector<char> host;   // [total] what goes to the device
};

// main_prog: what FusedJob::prog runs; plain: the plain program beside a folded one, null when the
// main program is the plain one.  ops: the caller's full list (20 states: the tip mask says which
// branches end in a tip -- only their tip tables are ever read, fused20_pmatrix_kernel).
inline ScheduleBlock pack_schedule_block(const Program &main_prog, const Program *plain, const std::vector<CladeStep> &steps,
                                         const std::vector<CladeGroup> &groups, const std::vector<double> &brlen,
                                         bool k20, unsigned tips, const rdamd_operation_t *ops, unsigned n_ops) {
  // harmless tail entries behind a program: the kernel prefetches descriptors up to i + 3
  constexpr size_t kTail = 4;
  auto up = [](size_t b) { return (b + 63) & ~(size_t)63; };
  const size_t n_main = main_prog.steps.size() + kTail, n_plain = plain ? plain->steps.size() + kTail : 0;
  const size_t prob_matrices = brlen.size();
  ScheduleBlock b;
  b.o_plain = up(b.o_prog + sizeof(FusedOp) * n_main);
  b.o_steps = up(b.o_plain + sizeof(FusedOp) * n_plain);
  b.o_groups = up(b.o_steps + sizeof(CladeStep) * steps.size());
  b.o_brlen = up(b.o_groups + sizeof(CladeGroup) * groups.size());
  b.o_tipmask = up(b.o_brlen + sizeof(double) * prob_matrices);
  b.total = up(b.o_tipmask + (k20 ? sizeof(uint32_t) * ((prob_matrices + 31) / 32) : 0));
  b.host.assign(b.total, 0);
  auto put_program = [&](size_t at, const Program &pr) {
    FusedOp *dst = (FusedOp *)(b.host.data() + at);
    memcpy(dst, pr.steps.data(), sizeof(FusedOp) * pr.steps.size());
    for (size_t k = 0; k < kTail; ++k) dst[pr.steps.size() + k] = pr.steps.back();
  };
  put_program(b.o_prog, main_prog);
  if (plain) put_program(b.o_plain, *plain);
  if (!steps.empty()) memcpy(b.host.data() + b.o_steps, steps.data(), sizeof(CladeStep) * steps.size());
  if (!groups.empty()) memcpy(b.host.data() + b.o_groups, groups.data(), sizeof(CladeGroup) * groups.size());
  if (prob_matrices) memcpy(b.host.data() + b.o_brlen, brlen.data(), sizeof(double) * prob_matrices);
  if (k20) {
    uint32_t *mask = (uint32_t *)(b.host.data() + b.o_tipmask);
    for (unsigned i = 0; i < n_ops; ++i) {
      if (ops[i].child1_clv_index < tips) mask[ops[i].child1_matrix_index >> 5] |= 1u << (ops[i].child1_matrix_index & 31u);
      if (ops[i].child2_clv_index < tips) mask[ops[i].child2_matrix_index >> 5] |= 1u << (ops[i].child2_matrix_index & 31u);
    }
  }
  return b;
}

}  // namespace rdamd
