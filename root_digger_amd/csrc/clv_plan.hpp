// What the launches of rdamd_update_clvs look like for one operation list: how the list is cut into
// segments and launches, where every inner child comes from, how many LDS parking slots a launch
// gets, the padding of the 4-state kernel and the look-ahead of the 20-state one.  Pure host logic
// over plain numbers -- no HIP, no partition, no environment -- so that
// tests/cpp/host_logic_check.cpp can replay every plan without a GPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "k20_split.hpp"
#include "level_op.hpp"

namespace rdamd {

struct ClvPlanInput {
  unsigned tips = 0, clv_buffers = 0, prob_matrices = 0, scale_buffers = 0, sites = 0, tip_stride = 0;
  uint64_t clv_bytes = 0;      // bytes per CLV buffer
  bool k20 = false;            // the 20-state matrix-core kernel runs the list (CLVs in its operand layout)
  unsigned slots_whole = 0;    // parking slots a launch of one list has (clv_traversal_slots)
  unsigned chunk = 1;          // the 4-state kernel's lists are padded to a multiple of this (clv_traversal_chunk)
  // the cut (list_levels): most pieces per launch (under 2: the list stays whole), the size a piece
  // keeps, the shortest list worth cutting
  unsigned rows = 0, small = 8, min_count = 16;
  unsigned readback_tolerance_pct = 6;   // see choose_slots
  int forced_slots = -1;       // >= 0: the slot count of every launch of several pieces (timing experiments)
};

struct ClvPlan {
  int bad_op = -1;             // >= 0: this operation (in the order below) has an index out of range; nothing else is filled in
  ListLevels cut;              // the list as list_levels cut it; cut.order is the order of `lops`, empty: the caller's
  std::vector<LevelOp> lops;   // what the kernel reads: the 4-state kernel's padded, with a terminator behind
  // segment s is lops[cuts[s], cuts[s + 1]); the segments [levels[l], levels[l + 1]) run side by side as
  // launch l, with seg_slots[levels[l]] parking slots each
  std::vector<unsigned> cuts, levels, seg_slots;
  unsigned launches() const { return (unsigned)levels.size() - 1; }
  ListPieces pieces(size_t l) const {
    ListPieces pc;
    for (unsigned seg = levels[l]; seg < levels[l + 1]; ++seg) {
      pc.start[pc.n] = cuts[seg];
      pc.len[pc.n++] = cuts[seg + 1] - cuts[seg];
    }
    return pc;
  }
};

// the caller's fields of one operation (the sources and offsets are the planner's business)
inline void level_op_fields(const rdamd_operation_t &o, LevelOp &d) {
  d.parent_clv = o.parent_clv_index; d.child1_clv = o.child1_clv_index;
  d.child2_clv = o.child2_clv_index; d.child1_mat = o.child1_matrix_index;
  d.child2_mat = o.child2_matrix_index; d.parent_sc = o.parent_scaler_index;
  d.child1_sc = o.child1_scaler_index; d.child2_sc = o.child2_scaler_index;
}

// does the operation name only buffers and matrices a partition of these sizes has?
inline bool operation_in_range(const rdamd_operation_t &o, unsigned tips, unsigned clv_buffers,
                               unsigned prob_matrices, unsigned scale_buffers) {
  const unsigned nclv = tips + clv_buffers;
  return !(o.parent_clv_index < tips || o.parent_clv_index >= nclv ||
           o.child1_clv_index >= nclv || o.child2_clv_index >= nclv ||
           o.child1_matrix_index >= prob_matrices || o.child2_matrix_index >= prob_matrices ||
           o.parent_scaler_index >= (int)scale_buffers || o.child1_scaler_index >= (int)scale_buffers ||
           o.child2_scaler_index >= (int)scale_buffers);
}

namespace clv_plan_detail {

// descriptors and byte offsets, every child from a tip or from memory for now; returns the first
// operation with an index out of range, or -1
inline int describe(const ClvPlanInput &in, const rdamd_operation_t *ops, unsigned count, std::vector<LevelOp> &lops) {
  lops.resize(count);
  auto sc_off = [&](int scb) { return scb >= 0 ? (uint64_t)scb * in.sites * sizeof(unsigned) : kNoOffset; };
  auto child_off = [&](unsigned clv) {
    return clv < in.tips ? (uint64_t)clv * in.tip_stride : (uint64_t)(clv - in.tips) * in.clv_bytes;
  };
  for (unsigned i = 0; i < count; ++i) {
    const rdamd_operation_t &o = ops[i];
    if (!operation_in_range(o, in.tips, in.clv_buffers, in.prob_matrices, in.scale_buffers)) return (int)i;
    LevelOp &d = lops[i];
    level_op_fields(o, d);
    d.src1 = o.child1_clv_index < in.tips ? 0u : 1u;
    d.src2 = o.child2_clv_index < in.tips ? 0u : 1u;
    d.park = d.noop = 0;
    d.parent_off = (uint64_t)(d.parent_clv - in.tips) * in.clv_bytes;
    d.parent_sc_off = sc_off(d.parent_sc);
    d.child1_off = child_off(d.child1_clv); d.child1_sc_off = sc_off(d.child1_sc);
    d.child2_off = child_off(d.child2_clv); d.child2_sc_off = sc_off(d.child2_sc);
  }
  return -1;
}

// Segment boundaries, and the first segment of every launch.  (`cuts` splits a list into segments,
// each analysed on its own: the pieces of a split list, which run side by side with the slots their
// row count leaves them, then the operations that join them; the 4-state kernel needs no other cut --
// memory children are read at use, after every earlier store of the lane.)
// The 20-state kernel requests the operands of operation i+1 a whole
// operation ahead and stores the result of operation i one operation late:
// operation i may not read from memory what i-1 or i-2 wrote.  Their parents
// are forwarded in registers (sources 2 and 3, Segments::find_consumers) -- except where the
// value cannot be forwarded (same CLV under another scaler index, or the
// other way round, or both earlier operations wrote it): there the list is
// cut into two launches.
// (No piece of a cut list has such a place -- list_levels has checked --; the list that is left
// over, or the whole list, may.)
inline void segments(const ClvPlanInput &in, const rdamd_operation_t *ops, unsigned count, ClvPlan &plan) {
  std::vector<unsigned> &cuts = plan.cuts, &levels = plan.levels;
  cuts.assign(1, 0u);
  levels.assign(1, 0u);
  if (!plan.cut.order.empty()) {
    cuts.assign(plan.cut.seg.begin(), plan.cut.seg.end() - 1);
    levels.assign(plan.cut.level.begin(), plan.cut.level.end() - 1);
  }
  if (in.k20)
    for (unsigned i = cuts.back() + 1; i < count; ++i)
      if (k20_hazard(in.tips, ops, i, cuts.back())) {
        cuts.push_back(i);
        levels.push_back((unsigned)cuts.size() - 1);
      }
  cuts.push_back(count);
  levels.push_back((unsigned)cuts.size() - 1);
}

// Where does each inner child come from?  The parent of the operation just
// before stays in the lane's registers; an older sibling waits in one of the
// kernel's LDS parking slots when one is free (shortest wait wins: when the
// slots are full the value needed furthest in the future gives its slot up
// and is read back from HBM instead -- every CLV is written there anyway).
// A child is forwarded only when its scaler index is the producer's.
struct Segments {
  const ClvPlanInput &in;
  const rdamd_operation_t *ops;
  std::vector<LevelOp> &lops;
  // producer: clv -> op of the segment under analysis that wrote it (all -1 between calls);
  // consumer: op -> first later op reading its parent; which: ... as its child 1 (0) or 2 (1)
  std::vector<int> producer, consumer, which, slot_owner;

  Segments(const ClvPlanInput &in_, const rdamd_operation_t *ops_, std::vector<LevelOp> &lops_)
      : in(in_), ops(ops_), lops(lops_), producer(in_.tips + in_.clv_buffers, -1), consumer(lops_.size()),
        which(lops_.size()) {}

  unsigned &src(int op, int child) { return child ? lops[op].src2 : lops[op].src1; }

  // the sources (and parks) of segment [lo, hi) with `nslots` parking slots; returns the number of
  // children it reads back from memory
  unsigned analyse(unsigned lo, unsigned hi, unsigned nslots) {
    find_consumers(lo, hi);
    if (!in.k20) assign_slots(lo, hi, nslots);
    unsigned readbacks = 0;
    for (unsigned i = lo; i < hi; ++i) {
      if (consumer[i] >= 0 && src(consumer[i], which[i]) == 1u) ++readbacks;
      producer[ops[i].parent_clv_index] = -1;
    }
    return readbacks;
  }

  void find_consumers(unsigned lo, unsigned hi) {
    const unsigned tips = in.tips;
    for (unsigned i = lo; i < hi; ++i) {
      consumer[i] = -1;
      lops[i].src1 = ops[i].child1_clv_index < tips ? 0u : 1u;
      lops[i].src2 = ops[i].child2_clv_index < tips ? 0u : 1u;
      if (!in.k20) lops[i].park = 0;
    }
    for (unsigned i = lo; i < hi; ++i) {
      const rdamd_operation_t &o = ops[i];
      const unsigned ch[2] = {o.child1_clv_index, o.child2_clv_index};
      const int chsc[2] = {o.child1_scaler_index, o.child2_scaler_index};
      for (int c = 0; c < 2; ++c) {
        if (ch[c] < tips || (!in.k20 && c == 1 && ch[1] == ch[0])) continue;
        const int j = producer[ch[c]];
        if (in.k20) {
          // the 20-state kernel keeps the results of the last TWO operations in
          // registers and forwards them to every reader (source 2: the operation
          // just before, 3: the one before that)
          if (j >= 0 && (int)i - j <= 2 && ops[j].parent_scaler_index == chsc[c])
            src((int)i, c) = (int)i - j == 1 ? 2u : 3u;
          continue;
        }
        if (j >= 0 && consumer[j] < 0 && ops[j].parent_scaler_index == chsc[c]) {
          consumer[j] = (int)i;
          which[j] = c;
        }
      }
      producer[o.parent_clv_index] = (int)i;
    }
  }

  // 4-state kernel: registers for the operation right behind, a parking slot for a later one
  void assign_slots(unsigned lo, unsigned hi, unsigned nslots) {
    slot_owner.assign(nslots, -1);
    for (unsigned i = lo; i < hi; ++i) {
      for (unsigned sl = 0; sl < nslots; ++sl)      // slots whose value is consumed now
        if (slot_owner[sl] >= 0 && consumer[slot_owner[sl]] == (int)i) slot_owner[sl] = -1;
      const int c = consumer[i];
      if (c < 0) continue;
      // (consumer[i] was taken from producer[] at the time the consumer was
      // scanned, i.e. op i is the LAST writer of that CLV before it: nothing
      // in between can have overwritten the value)
      if (c == (int)i + 1) {
        src(c, which[i]) = 2u;
        // the same CLV as both children: both come from the registers
        if (ops[c].child1_clv_index == ops[c].child2_clv_index &&
            ops[c].child1_scaler_index == ops[c].child2_scaler_index)
          lops[c].src1 = lops[c].src2 = 2u;
        continue;
      }
      if (nslots == 0) continue;
      int take = -1, far = -1;
      for (unsigned sl = 0; sl < nslots; ++sl) {
        if (slot_owner[sl] < 0) { take = (int)sl; far = -1; break; }
        if (far < 0 || consumer[slot_owner[sl]] > consumer[slot_owner[far]]) far = (int)sl;
      }
      if (take < 0 && far >= 0 && consumer[slot_owner[far]] > c) {
        const int ev = slot_owner[far];             // give the slot to the shorter wait
        src(consumer[ev], which[ev]) = 1u;
        lops[ev].park = 0;
        take = far;
      }
      if (take >= 0) {
        slot_owner[take] = (int)i;
        lops[i].park = 1u + (unsigned)take;
        src(c, which[i]) = 3u + (unsigned)take;
      }
    }
  }

  // read-backs of launch [s0, s1) of `cuts` when each of its segments has `nslots` slots
  unsigned level_readbacks(const std::vector<unsigned> &cuts, unsigned s0, unsigned s1, unsigned nslots) {
    unsigned n = 0;
    for (unsigned seg = s0; seg < s1; ++seg) n += analyse(cuts[seg], cuts[seg + 1], nslots);
    return n;
  }
};

// The pieces of a launch share one slot count: the fewest slots that leave no more read-backs than
// the whole-list count would, plus 6 in 100 operations (every slot less is LDS for another resident
// block, a read-back is one exposed round trip of one piece; measured, profiles/r5_clv_pieces_ab.txt:
// c2 in 8 pieces 162 / 172 / 189 us with 1 / 2 / 3 slots and 2 / 0 / 0 read-backs; c5's shard in
// 32 pieces 1.67 / 1.60 / 1.73 ms with 74 / 31 / 13).
inline void choose_slots(const ClvPlanInput &in, Segments &segs, ClvPlan &plan) {
  const std::vector<unsigned> &cuts = plan.cuts, &levels = plan.levels;
  plan.seg_slots.assign(cuts.size() - 1, in.slots_whole);
  for (size_t l = 0; !in.k20 && l + 1 < levels.size(); ++l) {
    const unsigned s0 = levels[l], s1 = levels[l + 1];
    if (s1 - s0 < 2) continue;
    const unsigned allowed = segs.level_readbacks(cuts, s0, s1, in.slots_whole) +
                             (cuts[s1] - cuts[s0]) * in.readback_tolerance_pct / 100;
    unsigned chosen = in.slots_whole;
    while (chosen > 0 && segs.level_readbacks(cuts, s0, s1, chosen - 1) <= allowed) --chosen;
    if (in.forced_slots >= 0) chosen = (unsigned)in.forced_slots;
    for (unsigned seg = s0; seg < s1; ++seg) plan.seg_slots[seg] = chosen;
  }
}

// 4-state kernel: every segment padded to whole chunks with no-ops (a copy of its last op, stores off)
inline void pad_segments(unsigned chunk, ClvPlan &plan) {
  const std::vector<LevelOp> &lops = plan.lops;
  const std::vector<unsigned> &cuts = plan.cuts;
  std::vector<LevelOp> padded_ops;
  std::vector<unsigned> padded_cuts{0u};
  padded_ops.reserve(lops.size() + cuts.size() * chunk + 1);
  LevelOp pad{};
  for (size_t seg = 0; seg + 1 < cuts.size(); ++seg) {
    padded_ops.insert(padded_ops.end(), lops.begin() + cuts[seg], lops.begin() + cuts[seg + 1]);
    pad = lops[cuts[seg + 1] - 1];
    pad.src1 = pad.src2 = 2u;
    pad.park = 0;
    pad.noop = 1;
    while ((padded_ops.size() - padded_cuts.back()) % chunk) padded_ops.push_back(pad);
    padded_cuts.push_back((unsigned)padded_ops.size());
  }
  padded_ops.push_back(pad);   // terminator: the kernel looks one operation ahead (a segment's last
                               // operation looks at the next segment's first: tip codes it never uses)
  plan.lops.swap(padded_ops);
  plan.cuts.swap(padded_cuts);
}

// tip-code look-ahead of the 20-state kernel (LevelOp::ahead*)
inline void fill_lookahead(std::vector<LevelOp> &lops) {
  const size_t count = lops.size();
  for (size_t i = 0; i < count; ++i) {
    const bool more = i + 1 < count;
    lops[i].ahead1 = more && lops[i + 1].src1 == 0u ? lops[i + 1].child1_clv : 0u;
    lops[i].ahead2 = more && lops[i + 1].src2 == 0u ? lops[i + 1].child2_clv : 0u;
  }
}

}  // namespace clv_plan_detail

// The plan for `count` >= 1 operations, already translated to pool slots where the partition is sparse.
// Independent subtrees run side by side, level by level (k20_split.hpp, list_levels): the 20-state
// kernel always (kernels_clv_mfma.hip), the 4-state one where one row of blocks leaves the device's
// wave slots empty (kernels_clv.hip).  Each segment (normally the whole list) runs in the caller's
// order: every dependency is site-local, so the kernel needs no level structure (kernels_clv.hip).
inline ClvPlan plan_clv_traversal(const ClvPlanInput &in, const rdamd_operation_t *ops, unsigned count) {
  using namespace clv_plan_detail;
  ClvPlan plan;
  if (in.rows >= 2)
    list_levels(in.tips, in.clv_buffers, ops, count, in.rows, in.small, in.min_count, plan.cut, in.k20);
  if (!plan.cut.order.empty()) ops = plan.cut.order.data();
  plan.bad_op = describe(in, ops, count, plan.lops);
  if (plan.bad_op >= 0) return plan;
  segments(in, ops, count, plan);
  Segments segs(in, ops, plan.lops);
  choose_slots(in, segs, plan);
  for (size_t seg = 0; seg + 1 < plan.cuts.size(); ++seg)
    segs.analyse(plan.cuts[seg], plan.cuts[seg + 1], plan.seg_slots[seg]);
  if (in.k20) fill_lookahead(plan.lops);
  else pad_segments(in.chunk, plan);
  return plan;
}

// Read-backs launch `l` of a finished 4-state plan would have with `nslots` slots per piece (the
// figures behind choose_slots; `ops`, `count`: the list the plan was made from)
inline unsigned clv_plan_readbacks(const ClvPlanInput &in, const ClvPlan &plan, const rdamd_operation_t *ops,
                                   unsigned count, size_t l, unsigned nslots) {
  const std::vector<unsigned> whole{0u, count};   // (plan.cuts counts the padding in)
  const bool cut = !plan.cut.order.empty();
  std::vector<LevelOp> scratch(count);
  clv_plan_detail::Segments segs(in, cut ? plan.cut.order.data() : ops, scratch);
  return segs.level_readbacks(cut ? plan.cut.seg : whole, plan.levels[l], plan.levels[l + 1], nslots);
}

}  // namespace rdamd
