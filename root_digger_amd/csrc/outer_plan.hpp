// The pre-order program of the OUTER vectors (kernels_outer.hip): the operation list of a rooted
// tree read backwards, with, for every operation, where the parent's outer vector comes from and
// where the two children's go.  Pure host logic over plain numbers -- no HIP, no partition -- so
// that tests/cpp/outer_plan_check.cpp can replay every plan without a GPU (as clv_plan.hpp).
//
// The outer vector of a node is made by its parent's operation and read by its own, once.  When its
// own operation is the very next of the program it stays in the lane's registers; otherwise it
// waits in a workspace slot.  Slots are handed out by liveness (a slot is free again from the
// operation that reads it, writes of that same operation included), so the workspace is "most
// vectors waiting at once" CLVs, not one per node.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/root_digger_amd.h"

namespace rdamd {

// OuterOp::parent_src
enum : unsigned { kOuterFromPi = 0, kOuterFromReg = 1, kOuterFromSlot = 2 };
// OuterOp::keep[c]
enum : unsigned { kOuterDrop = 0, kOuterKeepReg = 1, kOuterKeepSlot = 2 };

// one operation of the program, as the kernels read it.  Node k of the outputs is the parent of
// program operation k (node 0: the root); an inner child's node is the program index of its own operation.
struct OuterOp {
  unsigned op;              // index in the caller's (post-order) list
  unsigned parent_clv;
  unsigned parent_src, parent_slot;
  unsigned child_clv[2], child_mat[2];
  unsigned inner[2];        // is the child an inner node (its outer vector and posterior are wanted)
  unsigned node[2];         // ... then its node index
  unsigned keep[2], slot[2];
};

struct OuterPlan {
  int bad_op = -1;               // >= 0: the list was refused at this operation (caller's index); `why` says why
  const char *why = nullptr;
  std::vector<OuterOp> prog;     // prog[k] is the caller's operation count - 1 - k
  unsigned slots = 0;            // workspace slots the program uses
};

// The plan for a post-order list of `count` >= 1 operations over `tips` tips: a complete traversal
// of one rooted binary tree whose last operation is the root's.  That is: every parent is an inner
// CLV made once; every inner child was made by an earlier operation and is used by exactly one;
// no tip hangs under two operations; everything made is used, except the last parent.
inline OuterPlan plan_outer_program(const rdamd_operation_t *ops, unsigned count, unsigned tips) {
  OuterPlan plan;
  auto refuse = [&](unsigned i, const char *why) { plan.bad_op = (int)i; plan.why = why; plan.prog.clear(); return plan; };
  if (count == 0) return refuse(0, "an empty list");
  unsigned max_clv = 0;
  for (unsigned i = 0; i < count; ++i)
    for (unsigned c : {ops[i].parent_clv_index, ops[i].child1_clv_index, ops[i].child2_clv_index})
      if (c > max_clv) max_clv = c;
  // producer[clv]: the operation that made it (-1: none); used[clv]: already a child of some operation
  std::vector<int> producer((size_t)max_clv + 1, -1);
  std::vector<char> used((size_t)max_clv + 1, 0);
  for (unsigned i = 0; i < count; ++i) {
    const rdamd_operation_t &o = ops[i];
    if (o.parent_clv_index < tips) return refuse(i, "the parent is a tip");
    if (o.child1_clv_index == o.child2_clv_index) return refuse(i, "a child is used twice");
    for (unsigned c : {o.child1_clv_index, o.child2_clv_index}) {
      if (c >= tips && producer[c] < 0) return refuse(i, "the subtree of a child is missing (no earlier operation made it)");
      if (used[c]) return refuse(i, "a child is used twice");
      used[c] = 1;
    }
    if (producer[o.parent_clv_index] >= 0) return refuse(i, "a parent is made twice");
    if (used[o.parent_clv_index]) return refuse(i, "a parent is made after it was used");
    producer[o.parent_clv_index] = (int)i;
  }
  for (unsigned i = 0; i + 1 < count; ++i)
    if (!used[ops[i].parent_clv_index])
      return refuse(i, "the list does not end in the root operation (an earlier parent hangs under no operation)");

  plan.prog.resize(count);
  std::vector<unsigned> free_slots;   // a stack: the slot freed last is taken first
  for (unsigned k = 0; k < count; ++k) {
    const unsigned i = count - 1 - k;
    const rdamd_operation_t &o = ops[i];
    OuterOp &d = plan.prog[k];
    d.op = i;
    d.parent_clv = o.parent_clv_index;
    d.child_clv[0] = o.child1_clv_index; d.child_mat[0] = o.child1_matrix_index;
    d.child_clv[1] = o.child2_clv_index; d.child_mat[1] = o.child2_matrix_index;
    // the parent's vector: decided when its own parent's operation ran (below), except the root's
    if (k == 0) { d.parent_src = kOuterFromPi; d.parent_slot = 0; }
    if (d.parent_src == kOuterFromSlot) free_slots.push_back(d.parent_slot);   // read first, free for this operation's writes
    for (int c = 0; c < 2; ++c) {
      const unsigned clv = d.child_clv[c];
      d.inner[c] = clv >= tips ? 1u : 0u;
      d.node[c] = 0; d.keep[c] = kOuterDrop; d.slot[c] = 0;
      if (!d.inner[c]) continue;
      const unsigned kc = count - 1 - (unsigned)producer[clv];   // the child's own operation in the program (> k)
      d.node[c] = kc;
      OuterOp &child = plan.prog[kc];
      if (kc == k + 1) {
        d.keep[c] = kOuterKeepReg;
        child.parent_src = kOuterFromReg; child.parent_slot = 0;
        continue;
      }
      unsigned s;
      if (!free_slots.empty()) { s = free_slots.back(); free_slots.pop_back(); }
      else s = plan.slots++;
      d.keep[c] = kOuterKeepSlot; d.slot[c] = s;
      child.parent_src = kOuterFromSlot; child.parent_slot = s;
    }
  }
  return plan;
}

}  // namespace rdamd
