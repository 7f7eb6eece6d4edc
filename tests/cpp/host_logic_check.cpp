// CPU check of the pure host logic that shapes kernel launches (no HIP, no GPU):
//   * clade_classes (csrc/clade_classes.hpp): the pattern classes of a subtree -- what decides
//     which clades the fused evaluator folds into look-up tables -- against a brute-force count;
//   * k20_split (csrc/k20_split.hpp): cutting a post-order operation list into independent
//     subtree pieces -- against the properties the 20-state traversal kernel relies on.
//   * the traversal compiler (csrc/traversal_compiler.hpp) as the schedule planner sets it up
//     (csrc/schedule_plan.hpp, compile_program: the recipe rdamd_schedule_create hands the kernels):
//     its programs -- step order, which stack level sits in the register slot(s), which in-memory
//     entry in the LDS slot -- replayed symbolically: the running value at the end must be the
//     root's CLV expression, every pop must meet the sibling that was parked for it, for 4-state
//     (one / two register levels, pseudo-tips) and 20-state (parking as a step of its own) programs.
//   * the rest of the schedule planner: which operation lists it refuses and where, the producer /
//     consumer maps, which clades it folds into pseudo-tips (whole small subtrees, post-order,
//     64-row slots), the folded programs replayed, and the layout of the schedule's device block.
//   * the CLV traversal planner (csrc/clv_plan.hpp): every plan replayed symbolically -- each child
//     source names a value that is really there (tip, the registers of the operation(s) in front,
//     an LDS parking slot nobody has overwritten), segments, padding, slot counts and the 20-state
//     look-ahead are what the traversal kernels rely on.
//   * the launch rule of the fused 4-state evaluator (csrc/launch_plan.hpp): its defaults on the
//     benchmark's workloads against values worked out by hand from the thresholds, the LDS bound
//     over every rate count, sites per lane, table size and stack depth, and the forced values.
// prints "host logic OK <cases>" on success.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "clade_classes.hpp"
#include "clv_plan.hpp"
#include "k20_split.hpp"
#include "launch_plan.hpp"
#include "schedule_plan.hpp"

static int fail(const char *what, int a = 0, int b = 0) {
  std::printf("FAILED: %s (%d, %d)\n", what, a, b);
  return 1;
}

// random rooted binary tree with n tips as a post-order operation list (root_digger's index
// conventions: tips 0..n-1, inner CLVs n.., one matrix per child branch)
static std::vector<rdamd_operation_t> random_postorder(unsigned n, std::mt19937 &rng) {
  struct Node { int l = -1, r = -1; };
  std::vector<Node> nodes(n);            // tips
  std::vector<int> roots;
  for (unsigned i = 0; i < n; ++i) roots.push_back((int)i);
  while (roots.size() > 1) {             // join two random subtrees
    const size_t a = rng() % roots.size();
    int x = roots[a];
    roots.erase(roots.begin() + (std::ptrdiff_t)a);
    const size_t b = rng() % roots.size();
    int y = roots[b];
    roots.erase(roots.begin() + (std::ptrdiff_t)b);
    Node j;
    j.l = x; j.r = y;
    nodes.push_back(j);
    roots.push_back((int)nodes.size() - 1);
  }
  std::vector<rdamd_operation_t> ops;
  unsigned next_clv = n, next_mat = 0;
  std::vector<int> clv_of(nodes.size(), -1);
  for (unsigned i = 0; i < n; ++i) clv_of[i] = (int)i;
  // iterative post-order
  struct Frame { int node; int state; };
  std::vector<Frame> st{{roots[0], 0}};
  while (!st.empty()) {
    Frame &f = st.back();
    const Node &nd = nodes[(size_t)f.node];
    if (nd.l < 0) { st.pop_back(); continue; }
    if (f.state == 0) { f.state = 1; st.push_back({nd.l, 0}); continue; }
    if (f.state == 1) { f.state = 2; st.push_back({nd.r, 0}); continue; }
    rdamd_operation_t o;
    o.parent_clv_index = next_clv; o.parent_scaler_index = (int)(next_clv - n);
    o.child1_clv_index = (unsigned)clv_of[(size_t)nd.l]; o.child1_matrix_index = next_mat++;
    o.child1_scaler_index = nd.l < (int)n ? -1 : clv_of[(size_t)nd.l] - (int)n;
    o.child2_clv_index = (unsigned)clv_of[(size_t)nd.r]; o.child2_matrix_index = next_mat++;
    o.child2_scaler_index = nd.r < (int)n ? -1 : clv_of[(size_t)nd.r] - (int)n;
    clv_of[(size_t)f.node] = (int)next_clv++;
    ops.push_back(o);
    st.pop_back();
  }
  return ops;
}

// perfectly balanced tree with n = 2^k tips: pair up level by level
static std::vector<rdamd_operation_t> balanced_postorder(unsigned n) {
  std::vector<rdamd_operation_t> ops;
  std::vector<unsigned> level(n);
  for (unsigned i = 0; i < n; ++i) level[i] = i;
  unsigned next_clv = n, next_mat = 0;
  while (level.size() > 1) {
    std::vector<unsigned> up;
    for (size_t i = 0; i + 1 < level.size(); i += 2) {
      rdamd_operation_t o;
      o.parent_clv_index = next_clv; o.parent_scaler_index = -1;
      o.child1_clv_index = level[i]; o.child1_matrix_index = next_mat++; o.child1_scaler_index = -1;
      o.child2_clv_index = level[i + 1]; o.child2_matrix_index = next_mat++; o.child2_scaler_index = -1;
      ops.push_back(o);
      up.push_back(next_clv++);
    }
    level.swap(up);
  }
  return ops;
}

// ---- symbolic replay of a compiled program ---------------------------------------------------
// A CLV expression is a 64-bit hash: tip(row, table) for a table look-up, mv(matrix, x) for a
// matrix-vector product, x * y (commutative) for the element product.
static uint64_t mix(uint64_t a, uint64_t b) {
  a ^= b + 0x9e3779b97f4a7c15ull + (a << 6) + (a >> 2);
  a *= 0xff51afd7ed558ccdull;
  return a ^ (a >> 33);
}
static uint64_t h_tip(unsigned row, unsigned tab) { return mix(mix(1, row), tab); }
static uint64_t h_mv(unsigned mat, uint64_t x) { return mix(mix(2, mat), x); }
static uint64_t h_mul(uint64_t x, uint64_t y) { return mix(3, x < y ? mix(x, y) : mix(y, x)); }

// what the operation list says the root CLV is, in the terms the program uses (byte offsets)
static uint64_t expected(const rdamd::Compiler &c, const std::vector<rdamd_operation_t> &ops, unsigned i) {
  const rdamd_operation_t &o = ops[i];
  auto term = [&](unsigned clv, unsigned mat) -> uint64_t {
    if (!c.is_inner(clv)) {
      const unsigned tab = c.pseudo_wide.count(clv) ? c.wide_base + c.pseudo_wide.at(clv) * c.rate_cats * 512u
                                                    : mat * c.unit;
      return h_tip(c.row_of(clv) * c.tip_stride, tab);
    }
    return h_mv(mat * c.unit, expected(c, ops, c.producer.at(clv)));
  };
  return h_mul(term(o.child1_clv_index, o.child1_matrix_index), term(o.child2_clv_index, o.child2_matrix_index));
}

// runs the program the way the kernels do (kernels_fused.hip / kernels_fused_k20.hip): one or
// two register slots, the other entries on a stack addressed by the count of entries in it
// marked[k] (k = 0, 1): what the running CLV must be behind the step flagged 0x8000 << k -- the root
// operation's child k + 1 as the list defines it (0: that child is no inner node of the program,
// no step may carry the flag)
static int replay(const rdamd::Compiler &c, unsigned lds_pos, uint64_t want, unsigned &mem_depth,
                  const uint64_t marked[2] = nullptr) {
  using namespace rdamd;
  unsigned seen[2] = {0, 0};
  uint64_t run = 0, s0 = 0, s1 = 0, lds = 0;
  bool s0_full = false, s1_full = false, lds_full = false;
  const bool placed = !c.park_class.empty();   // parks with a place of their own: register slot, ONE LDS slot, the rest a stack
  std::vector<uint64_t> mem;
  mem_depth = 0;
  for (size_t i = 0; i < c.out.size(); ++i) {
    const FusedOp &f = c.out[i];
    const unsigned kind = f.flags & 3u;
    auto park = [&](uint64_t v) -> int {
      if (f.flags & 0x200u) { if (s0_full) return 1; s0 = v; s0_full = true; }
      else if (f.flags & 0x800u) { if (s1_full || c.reg_levels < 2) return 1; s1 = v; s1_full = true; }
      else if (placed && (f.flags & 0x20000u)) { if (lds_full) return 1; lds = v; lds_full = true; }
      else { mem.push_back(v); mem_depth = std::max(mem_depth, (unsigned)mem.size()); }
      if (!placed && (f.flags & 0x60000u)) return 1;
      return 0;
    };
    if (kind == kFusedPark) {
      if (!c.split_park) return fail("a park step in a 4-state program", (int)i);
      if (park(h_mv(f.pM, run))) return fail("park into an occupied register slot", (int)i);
    } else if (kind == kFusedTT) {
      if (f.flags & 0x100u) {
        if (c.split_park) return fail("a 20-state tip-tip step must not park", (int)i);
        if (park(h_mv(f.pM, run))) return fail("park into an occupied register slot", (int)i);
      }
      run = h_mul(h_tip(f.cX, f.tX), h_tip(f.cY, f.tY));
    } else if (kind == kFusedRT) {
      run = h_mul(h_mv(f.pM, run), h_tip(f.cY, f.tY));
    } else {   // kFusedRP
      uint64_t sib;
      if (f.flags & 0x400u) { if (!s0_full) return fail("pop from an empty register slot", (int)i); sib = s0; s0_full = false; }
      else if (f.flags & 0x1000u) { if (!s1_full) return fail("pop from an empty register slot 1", (int)i); sib = s1; s1_full = false; }
      else if (placed && (f.flags & 0x40000u)) { if (!lds_full) return fail("pop from an empty LDS slot", (int)i); sib = lds; lds_full = false; }
      else { if (mem.empty()) return fail("pop from an empty stack", (int)i); sib = mem.back(); mem.pop_back(); }
      run = h_mul(h_mv(f.pM, run), sib);
    }
    for (int k = 0; marked && k < 2; ++k)
      if (f.flags & (0x8000u << k)) {
        if (kind == kFusedPark || !marked[k] || run != marked[k])
          return fail("a step is flagged as the root operation's child but does not leave it in the running CLV", (int)i, k);
        ++seen[k];
      }
  }
  for (int k = 0; marked && k < 2; ++k)
    if (seen[k] != (marked[k] ? 1u : 0u)) return fail("root child: flagged steps", k, (int)seen[k]);
  if (s0_full || s1_full || lds_full || !mem.empty()) return fail("entries left on the stack");
  if (run != want) return fail("the program does not compute the root CLV");
  if (!placed && mem_depth >= 2 && c.reg_levels == 1 && lds_pos >= mem_depth) return fail("lds_pos out of range", (int)lds_pos, (int)mem_depth);
  if (placed && mem_depth != c.mem_depth) return fail("private-segment depth", (int)mem_depth, (int)c.mem_depth);
  return 0;
}

static int check_compiler(std::mt19937 &rng, int &cases) {
  unsigned long placed_total = 0, placed_in_slots = 0, placed_by_levels = 0;
  for (int rep = 0; rep < 600; ++rep) {
    const bool k20 = rep % 3 == 2;
    // shapes: random joins (deep, unbalanced), balanced (deepest stacks), caterpillar (depth 1)
    unsigned n = 3 + rng() % (rep % 10 == 0 ? 1500 : 300);
    std::vector<rdamd_operation_t> ops = random_postorder(n, rng);
    if (rep % 5 == 1) {
      n = 1u << (2 + rng() % 9);
      ops = balanced_postorder(n);
    }
    // the library's recipe (schedule_plan.hpp), for the shapes rdamd_schedule_create compiles: 20 states,
    // 4 states with 64-row table slots (kernels with private-segment levels) and with 16-row ones
    rdamd::ScheduleShape sh;
    sh.tips = n; sh.sites = 1000; sh.tip_stride = 1000; sh.rate_cats = 4; sh.prob_matrices = 2 * n;
    sh.k20 = k20; sh.wide_mode = !k20 && rep % 4 < 2;
    rdamd::ClvMap pseudo_row, pseudo_wide;
    if (!k20 && rep % 2 == 0) {   // some inner nodes become pseudo-tips (their subtrees leave the program)
      unsigned rows = n, wide = 0;
      for (unsigned i = 0; i + 1 < ops.size(); ++i)
        if (rng() % 6 == 0) {
          pseudo_row[ops[i].parent_clv_index] = rows++;
          if (rng() % 2) pseudo_wide[ops[i].parent_clv_index] = wide++;
        }
    }
    rdamd::Program prog;
    rdamd::ProgramTrace trace;
    const unsigned lost = rdamd::compile_program(sh, ops, pseudo_row, pseudo_wide, prog, &trace);
    const rdamd::Compiler &c = trace.c;
    const unsigned lds_pos = trace.runner_up;
    const unsigned beyond = k20 ? 0u : (sh.wide_mode ? 1u + rdamd::kFusedSpillLevels : 3u);
    if (c.place_parks != (!k20 && sh.wide_mode) || c.dma_offsets != c.place_parks) return fail("the recipe's 64-row switches");
    // what the first pass finds, from the list alone: the stack depth is the root's Sethi-Ullman
    // number, and every node with two inner children parks once
    const unsigned first_pass_depth = c.need[c.n_ops - 1];
    unsigned parks = 0;
    {
      std::vector<unsigned> todo{c.n_ops - 1};
      while (!todo.empty()) {
        const rdamd_operation_t &o = ops[todo.back()];
        todo.pop_back();
        unsigned inner = 0;
        for (unsigned ch : {o.child1_clv_index, o.child2_clv_index})
          if (c.is_inner(ch)) { todo.push_back(c.producer.at(ch)); ++inner; }
        parks += inner == 2;
      }
    }
    // the steps that compute the root operation's inner children carry 0x8000 / 0x10000 (the
    // exporting evaluator, rdamd_evaluate_root_children)
    uint64_t marked[2] = {0, 0};
    const bool placed = !c.park_class.empty();
    if (c.max_depth != first_pass_depth) return fail("the second pass changed the stack depth");
    unsigned parks2 = 0, busiest = 0;
    for (unsigned l = 0; l < 16; ++l) { parks2 += c.parks_at[l]; busiest = std::max(busiest, c.parks_at[l]); }
    if (parks2 != parks) return fail("the second pass changed the number of parks");
    if (!placed && c.reg_levels == 1 && c.max_depth >= 1 && c.parks_at[c.reg_level] != busiest)
      return fail("the register slot is not on the busiest level", (int)c.reg_level);
    if (placed) {   // placed park by park: never fewer in the two slots than the two busiest levels would hold
      unsigned in_slots = 0, best = 0, second = 0;
      for (const rdamd::FusedOp &f : c.out) in_slots += (f.flags & 0x100u) && (f.flags & 0x20200u);
      for (unsigned l = 0; l < 16; ++l) {
        if (c.parks_at[l] > best) { second = best; best = c.parks_at[l]; }
        else if (c.parks_at[l] > second) second = c.parks_at[l];
      }
      if (in_slots < best + second) return fail("placing the parks one by one must not lose to the level rule", (int)in_slots, (int)(best + second));
      placed_total += parks; placed_in_slots += in_slots; placed_by_levels += best + second;
    }
    if (k20 && c.reg_levels != 1) return fail("20-state programs have one register level");
    if (!k20 && (c.reg_levels == 2) != (c.max_depth > beyond)) return fail("two register levels", (int)c.max_depth);
    unsigned mem_depth = 0;
    if (!k20) {
      const rdamd_operation_t &root = ops.back();
      const unsigned kid[2] = {root.child1_clv_index, root.child2_clv_index};
      for (int k = 0; k < 2; ++k)   // (a child folded into a pseudo-tip is no step of the program)
        if (kid[k] >= n && c.is_inner(kid[k])) marked[k] = expected(c, ops, c.producer.at(kid[k]));
    }
    if (replay(c, lds_pos, expected(c, ops, c.n_ops - 1), mem_depth, k20 ? nullptr : marked)) return 1;
    if (!placed && mem_depth != (c.max_depth > c.reg_levels ? c.max_depth - c.reg_levels : 0)) return fail("in-memory depth", (int)mem_depth, (int)c.max_depth);
    if (placed && mem_depth > rdamd::kFusedSpillLevels - 1u) return fail("more private-segment entries than a wave has room for", (int)mem_depth);
    if (c.reg_levels == 1 && !k20 && mem_depth + 1 > beyond) return fail("more in-memory entries than the kernel has places for");
    // steps: one per operation left in the program (+ one per park for 20 states)
    size_t real = 0;
    for (const rdamd::FusedOp &f : c.out) real += (f.flags & 3u) != rdamd::kFusedPark || !k20;
    if (c.pseudo_row.empty() && real != c.n_ops) return fail("operations lost", (int)real, (int)c.n_ops);
    if (lost != c.n_ops - real) return fail("the recipe's count of unreachable operations", (int)lost, (int)(c.n_ops - real));
    if (!lost) {   // the program as the schedule keeps it
      if (prog.steps.size() != c.out.size() || memcmp(prog.steps.data(), c.out.data(), sizeof(rdamd::FusedOp) * c.out.size()))
        return fail("Program::steps are not the compiler's");
      if (prog.reg_levels != c.reg_levels || prog.matvecs != c.matvecs) return fail("Program: register levels / matvecs");
      // in-memory levels the launch allocates: every entry of the replayed stack (+ the LDS slot of placed parks)
      if (prog.depth != (placed ? 1u + mem_depth : std::max(1u, mem_depth))) return fail("Program::depth", (int)prog.depth, (int)mem_depth);
    }
    ++cases;
  }
  std::fprintf(stderr, "parks placed one by one: %lu of %lu in the two slots (the two busiest levels: %lu)\n", placed_in_slots,
              placed_total, placed_by_levels);
  return 0;
}


// ---- the CLV traversal planner ---------------------------------------------------------------
// one plan against what the traversal kernels (kernels_clv.hip, kernels_clv_mfma.hip) take for granted
static int replay_plan(const rdamd::ClvPlanInput &in, const std::vector<rdamd_operation_t> &given, const rdamd::ClvPlan &plan) {
  using namespace rdamd;
  const unsigned count = (unsigned)given.size(), tips = in.tips;
  const std::vector<rdamd_operation_t> &ops = plan.cut.order.empty() ? given : plan.cut.order;
  if (plan.bad_op >= 0) return fail("plan: an operation in range was refused", plan.bad_op);
  if (ops.size() != count) return fail("plan: the cut list is no permutation (size)");
  const std::vector<unsigned> &cuts = plan.cuts, &levels = plan.levels;
  if (cuts.size() < 2 || cuts.front() != 0 || levels.size() < 2 || levels.front() != 0 || levels.back() != cuts.size() - 1 ||
      plan.seg_slots.size() != cuts.size() - 1 || plan.launches() != levels.size() - 1)
    return fail("plan: segment / launch bounds");
  if (plan.lops.size() != cuts.back() + (in.k20 ? 0u : 1u)) return fail("plan: list length", (int)plan.lops.size(), (int)cuts.back());
  if (in.k20 && cuts.back() != count) return fail("plan: a 20-state list is not padded");
  const unsigned most_slots = in.forced_slots >= 0 ? std::max((unsigned)in.forced_slots, in.slots_whole) : in.slots_whole;
  unsigned next = 0;   // operations of `ops` met so far
  for (size_t l = 0; l + 1 < levels.size(); ++l) {
    const unsigned s0 = levels[l], s1 = levels[l + 1];
    if (s1 <= s0 || s1 - s0 > kMaxListPieces) return fail("plan: pieces per launch", (int)l, (int)(s1 - s0));
    const ListPieces pc = plan.pieces(l);
    if (pc.n != s1 - s0) return fail("plan: ListPieces count", (int)l);
    for (unsigned seg = s0; seg < s1; ++seg) {
      const unsigned lo = cuts[seg], hi = cuts[seg + 1], nslots = plan.seg_slots[seg];
      if (hi <= lo) return fail("plan: empty segment", (int)seg);
      if (pc.start[seg - s0] != lo || pc.len[seg - s0] != hi - lo) return fail("plan: ListPieces bounds", (int)seg);
      if (nslots != plan.seg_slots[s0] || nslots > most_slots) return fail("plan: slot count", (int)seg, (int)nslots);
      if (!in.k20 && (hi - lo) % in.chunk) return fail("plan: a segment is no whole number of chunks", (int)seg, (int)(hi - lo));
      struct Parked { unsigned clv = 0; int sc = 0, writer = -1; };
      std::vector<Parked> slot(nslots);
      std::map<unsigned, int> last_writer;   // CLV -> entry of this segment that wrote it last
      const unsigned first = next;           // (`ops` index of the segment's first operation)
      bool padding = false;
      for (unsigned i = lo; i < hi; ++i) {
        const LevelOp &d = plan.lops[i];
        if (!in.k20 && d.noop) {   // pads: behind the segment's operations, stores off, nothing read or parked
          if (d.noop != 1 || d.src1 != 2u || d.src2 != 2u || d.park != 0 || i == lo) return fail("plan: pad entry", (int)i);
          if (d.parent_clv != plan.lops[i - 1].parent_clv) return fail("plan: a pad is a copy of the segment's last operation", (int)i);
          padding = true;
          continue;
        }
        if (padding) return fail("plan: an operation behind the padding", (int)i);
        if (next >= count) return fail("plan: more operations than the list has", (int)i);
        const rdamd_operation_t &o = ops[next];
        LevelOp want;
        level_op_fields(o, want);
        if (d.parent_clv != want.parent_clv || d.child1_clv != want.child1_clv || d.child2_clv != want.child2_clv ||
            d.child1_mat != want.child1_mat || d.child2_mat != want.child2_mat || d.parent_sc != want.parent_sc ||
            d.child1_sc != want.child1_sc || d.child2_sc != want.child2_sc)
          return fail("plan: descriptor fields", (int)i);
        auto sc_off = [&](int sc) { return sc >= 0 ? (uint64_t)sc * in.sites * 4u : kNoOffset; };
        auto clv_off = [&](unsigned clv) { return clv < tips ? (uint64_t)clv * in.tip_stride : (uint64_t)(clv - tips) * in.clv_bytes; };
        if (d.parent_off != clv_off(d.parent_clv) || d.child1_off != clv_off(d.child1_clv) || d.child2_off != clv_off(d.child2_clv) ||
            d.parent_sc_off != sc_off(d.parent_sc) || d.child1_sc_off != sc_off(d.child1_sc) || d.child2_sc_off != sc_off(d.child2_sc))
          return fail("plan: byte offsets", (int)i);
        const unsigned ch[2] = {d.child1_clv, d.child2_clv}, src[2] = {d.src1, d.src2};
        const int chsc[2] = {d.child1_sc, d.child2_sc};
        for (int c = 0; c < 2; ++c) {
          if ((src[c] == 0u) != (ch[c] < tips)) return fail("plan: source 0 is a tip, every other source an inner CLV", (int)i, c);
          if (src[c] < 2u) continue;
          // registers: the parent of the operation `back` places in front, in the same segment
          const unsigned back = src[c] - 1u;
          if (in.k20 || src[c] == 2u) {
            if (back > 2u || (!in.k20 && back != 1u) || i < lo + back) return fail("plan: register source out of the segment", (int)i, c);
            const LevelOp &b = plan.lops[i - back];
            if (b.parent_clv != ch[c] || b.parent_sc != chsc[c]) return fail("plan: register source is not that operation's parent", (int)i, c);
            continue;
          }
          const unsigned s = src[c] - 3u;
          if (s >= nslots) return fail("plan: parking slot beyond the segment's slots", (int)i, (int)s);
          if (slot[s].writer < 0 || slot[s].clv != ch[c] || slot[s].sc != chsc[c] || !last_writer.count(ch[c]) ||
              last_writer[ch[c]] != slot[s].writer)
            return fail("plan: the parking slot does not hold the child's current value", (int)i, (int)s);
        }
        if (in.k20) {
          if (i > lo && k20_hazard(tips, ops.data(), next, first)) return fail("plan: a 20-state hazard inside a segment", (int)i);
          const bool more = next + 1 < count;
          const unsigned a1 = more && ops[next + 1].child1_clv_index < tips ? ops[next + 1].child1_clv_index : 0u;
          const unsigned a2 = more && ops[next + 1].child2_clv_index < tips ? ops[next + 1].child2_clv_index : 0u;
          if (d.ahead1 != a1 || d.ahead2 != a2) return fail("plan: tip-code look-ahead", (int)i);
        } else if (d.park) {
          if (d.park > nslots) return fail("plan: park beyond the segment's slots", (int)i, (int)d.park);
          slot[d.park - 1].clv = d.parent_clv; slot[d.park - 1].sc = d.parent_sc; slot[d.park - 1].writer = (int)i;
        }
        last_writer[d.parent_clv] = (int)i;
        ++next;
      }
    }
  }
  if (next != count) return fail("plan: operations lost", (int)next, (int)count);
  if (!in.k20) {
    const rdamd::LevelOp &t = plan.lops.back();
    if (t.noop != 1 || t.park != 0 || t.src1 != 2u || t.src2 != 2u) return fail("plan: terminator");
  }
  return 0;
}

// one input of the planner: a tree of 10 to 1000 tips, the list bent in the ways callers bend it
static void planner_case(std::mt19937 &rng, int rep, std::vector<rdamd_operation_t> &ops, rdamd::ClvPlanInput &in) {
  const unsigned n = 10 + rng() % 991;
  ops = random_postorder(n, rng);
  switch (rep % 5) {
    case 1:   // the same CLV as both children
      for (size_t i = 1; i < ops.size(); ++i)
        if (ops[i].child1_clv_index >= n && rng() % 4 == 0) {
          ops[i].child2_clv_index = ops[i].child1_clv_index;
          ops[i].child2_scaler_index = rng() % 8 ? ops[i].child1_scaler_index : -1;
        }
      break;
    case 2:   // a child under another scaler index than its producer's: must not be forwarded
      for (size_t i = 1; i < ops.size(); ++i) {
        if (ops[i].child1_clv_index >= n && rng() % 3 == 0) ops[i].child1_scaler_index = rng() % 2 ? -1 : (int)(rng() % n);
        if (ops[i].child2_clv_index >= n && rng() % 3 == 0) ops[i].child2_scaler_index = rng() % 2 ? -1 : (int)(rng() % n);
      }
      break;
    case 3:   // a partial list: inner children nothing in it computes
      ops.erase(ops.begin(), ops.begin() + (std::ptrdiff_t)(rng() % (ops.size() - 1)));
      break;
    default: break;
  }
  in = rdamd::ClvPlanInput();
  in.tips = n; in.clv_buffers = in.prob_matrices = in.scale_buffers = 2 * n;
  in.sites = 1 + rng() % 5000; in.tip_stride = (in.sites + 3u) & ~3u;
  in.k20 = rep % 2 == 1;
  in.clv_bytes = in.k20 ? (uint64_t)(in.sites + 15) / 16 * 16 * 4 * 20 * 8 : (uint64_t)in.sites * 4 * 4 * 8;
  in.slots_whole = in.k20 ? 0u : rng() % 7;
  in.chunk = !in.k20 && rng() % 2 ? 4u : 1u;   // (the 4-state kernel's chunk, kernels_clv.hip)
  const unsigned rows[4] = {0, 8, 16, 32};
  in.rows = rows[rng() % 4];
  in.small = in.k20 ? 24u : 4u + rng() % 12;
  in.min_count = 6 + rng() % 24;
  if (rep % 7 == 0) in.readback_tolerance_pct = rng() % 30;
  if (rep % 11 == 0) in.forced_slots = (int)(rng() % 7);
}

static int check_planner(std::mt19937 &rng, int &cases) {
  unsigned long cut_lists = 0, launches = 0;
  for (int rep = 0; rep < 600; ++rep) {
    std::vector<rdamd_operation_t> ops;
    rdamd::ClvPlanInput in;
    planner_case(rng, rep, ops, in);
    const rdamd::ClvPlan plan = rdamd::plan_clv_traversal(in, ops.data(), (unsigned)ops.size());
    if (replay_plan(in, ops, plan)) return 1;
    // the figures behind the slot choice, recomputed from the finished plan: a launch of several
    // pieces has no more read-backs than the tolerance allows over the whole-list slot count
    for (size_t l = 0; !in.k20 && in.forced_slots < 0 && l < plan.launches(); ++l) {
      const unsigned s0 = plan.levels[l], s1 = plan.levels[l + 1];
      if (s1 - s0 < 2) continue;
      const unsigned n_ops = plan.cut.seg[s1] - plan.cut.seg[s0];
      const unsigned base = rdamd::clv_plan_readbacks(in, plan, ops.data(), (unsigned)ops.size(), l, in.slots_whole);
      const unsigned got = rdamd::clv_plan_readbacks(in, plan, ops.data(), (unsigned)ops.size(), l, plan.seg_slots[s0]);
      if (got > base + n_ops * in.readback_tolerance_pct / 100) return fail("plan: read-backs over the tolerance", (int)got, (int)base);
    }
    cut_lists += !plan.cut.order.empty();
    launches += plan.launches();
    ++cases;
  }
  for (int k20 = 0; k20 < 2; ++k20) {   // an index out of range: the first such operation is named, nothing is planned
    std::vector<rdamd_operation_t> ops = random_postorder(200, rng);
    rdamd::ClvPlanInput in;
    in.tips = 200; in.clv_buffers = in.prob_matrices = in.scale_buffers = 400;
    in.sites = 100; in.tip_stride = 100; in.clv_bytes = 100 * 128; in.k20 = k20 != 0; in.rows = 8;
    ops[150].child2_matrix_index = 400;
    ops[170].parent_scaler_index = 400;
    const rdamd::ClvPlan plan = rdamd::plan_clv_traversal(in, ops.data(), (unsigned)ops.size());
    const std::vector<rdamd_operation_t> &order = plan.cut.order.empty() ? ops : plan.cut.order;
    int first_bad = -1;
    for (size_t i = 0; i < order.size() && first_bad < 0; ++i)
      if (!rdamd::operation_in_range(order[i], 200, 400, 400, 400)) first_bad = (int)i;
    if (plan.bad_op < 0 || plan.bad_op != first_bad) return fail("plan: index out of range", plan.bad_op, first_bad);
    ++cases;
  }
  std::fprintf(stderr, "planner: %lu of 600 lists cut, %lu launches\n", cut_lists, launches);
  return 0;
}

// ---- the schedule planner (csrc/schedule_plan.hpp) ------------------------------------------
// a tree of the existing generators: random joins, every fifth perfectly balanced
static std::vector<rdamd_operation_t> plan_tree(std::mt19937 &rng, int rep, unsigned most, unsigned &n) {
  n = 4 + rng() % (most - 3);
  if (rep % 5 != 1) return random_postorder(n, rng);
  n = 4;
  while (2 * n <= most && rng() % 3) n *= 2;
  return balanced_postorder(n);
}

// matrix m of the list's 2n - 2 gets length m + 0.5, in shuffled order
static void branch_list(std::mt19937 &rng, unsigned n_mat, std::vector<unsigned> &idx, std::vector<double> &len) {
  idx.resize(n_mat);
  for (unsigned m = 0; m < n_mat; ++m) idx[m] = m;
  std::shuffle(idx.begin(), idx.end(), rng);
  len.resize(n_mat);
  for (unsigned m = 0; m < n_mat; ++m) len[m] = idx[m] + 0.5;
}

static int check_validation(std::mt19937 &rng, int &cases) {
  using rdamd::ScheduleCheck;
  for (int rep = 0; rep < 150; ++rep) {
    unsigned n;
    const std::vector<rdamd_operation_t> ops = plan_tree(rng, rep, 300, n);
    const unsigned count = (unsigned)ops.size(), n_mat = 2 * n - 2, bufs = n + 3, mats = n_mat + 3;
    std::vector<unsigned> idx;
    std::vector<double> len;
    branch_list(rng, n_mat, idx, len);
    auto check = [&](const std::vector<rdamd_operation_t> &list) {
      return rdamd::validate_schedule(n, bufs, mats, list.data(), (unsigned)list.size(), idx.data(), len.data(), n_mat);
    };
    {   // the valid list passes; its maps against a direct scan
      const ScheduleCheck v = check(ops);
      if (v.kind != ScheduleCheck::kOk || v.matrix_shared) return fail("validation: a valid list was refused", (int)v.kind, (int)v.at);
      if (v.producer.size() != count || v.consumer.size() != count) return fail("validation: map sizes");
      for (unsigned i = 0; i < count; ++i) {
        if (!v.producer.count(ops[i].parent_clv_index) || v.producer.at(ops[i].parent_clv_index) != i) return fail("validation: producer", (int)i);
        int taker = -1;
        for (unsigned j = 0; j < count; ++j)
          if (ops[j].child1_clv_index == ops[i].parent_clv_index || ops[j].child2_clv_index == ops[i].parent_clv_index) taker = (int)j;
        if (v.consumer[i] != taker || (taker < 0) != (i + 1 == count)) return fail("validation: consumer", (int)i, taker);
      }
      if (v.brlen.size() != mats) return fail("validation: branch lengths (size)");
      for (unsigned m = 0; m < mats; ++m)
        if (v.brlen[m] != (m < n_mat ? m + 0.5 : 0.0)) return fail("validation: branch length", (int)m);
      ++cases;
    }
    // mutants: each refused at the first operation that, read in order, no longer fits what came before
    auto refused_at = [&](const std::vector<rdamd_operation_t> &list, unsigned want, const char *what) {
      const ScheduleCheck v = check(list);
      if (v.kind != ScheduleCheck::kOperation || v.at != want) return fail(what, (int)v.at, (int)want);
      ++cases;
      return 0;
    };
    std::vector<unsigned> inner_child;   // operations with an inner child 1 or 2
    for (unsigned i = 0; i < count; ++i)
      if (ops[i].child1_clv_index >= n || ops[i].child2_clv_index >= n) inner_child.push_back(i);
    if (!inner_child.empty()) {
      const unsigned i = inner_child[rng() % inner_child.size()];
      const unsigned c = ops[i].child1_clv_index >= n ? ops[i].child1_clv_index : ops[i].child2_clv_index;
      const unsigned made = c - n;   // (both generators: operation k writes CLV n + k)
      {   // a child used by two operations: whichever comes second is refused
        unsigned k = made + 1 + rng() % (count - made - 1);
        if (k == i) k = k + 1 < count ? k + 1 : made + 1;
        if (k != i) {
          std::vector<rdamd_operation_t> bad = ops;
          bad[k].child1_clv_index = c;
          if (refused_at(bad, std::max(k, i), "validation: a child used twice")) return 1;
        }
      }
      {   // a child in front of its producer: the two operations change places
        std::vector<rdamd_operation_t> bad = ops;
        std::swap(bad[made], bad[i]);
        if (refused_at(bad, made, "validation: a child that is not yet computed")) return 1;
      }
    }
    if (count >= 2) {   // a parent written twice
      const unsigned k = 1 + rng() % (count - 1), j = rng() % k;
      std::vector<rdamd_operation_t> bad = ops;
      bad[k].parent_clv_index = bad[j].parent_clv_index;
      if (refused_at(bad, k, "validation: a parent written twice")) return 1;
    }
    {   // an index out of range
      const unsigned k = rng() % count;
      std::vector<rdamd_operation_t> bad = ops;
      switch (rep % 4) {
        case 0: bad[k].child2_clv_index = n + bufs; break;
        case 1: bad[k].child1_matrix_index = mats; break;
        case 2: bad[k].parent_clv_index = rng() % n; break;   // (a tip is no destination)
        default: bad[k].parent_clv_index = n + bufs + rng() % 5; break;
      }
      if (refused_at(bad, k, "validation: an index out of range")) return 1;
    }
    {   // an empty list
      if (rdamd::validate_schedule(n, bufs, mats, ops.data(), 0, idx.data(), len.data(), n_mat).kind != ScheduleCheck::kEmpty)
        return fail("validation: an empty list");
      ++cases;
    }
    {   // the branch list: a length that is negative, NaN or infinite, a matrix the partition does not have
      const unsigned m = rng() % n_mat;
      std::vector<unsigned> bad_idx = idx;
      std::vector<double> bad_len = len;
      const double inf = std::numeric_limits<double>::infinity();
      switch (rep % 5) {
        case 0: bad_len[m] = -1e-300; break;
        case 1: bad_len[m] = std::numeric_limits<double>::quiet_NaN(); break;
        case 2: bad_len[m] = inf; break;
        case 3: bad_len[m] = -inf; break;
        default: bad_idx[m] = mats + rng() % 3; break;
      }
      const ScheduleCheck v = rdamd::validate_schedule(n, bufs, mats, ops.data(), count, bad_idx.data(), bad_len.data(), n_mat);
      if (v.kind != ScheduleCheck::kBranch || v.at != m) return fail("validation: a bad branch", (int)v.at, (int)m);
      ++cases;
    }
    {   // a detached subtree: a valid post-order list, but the root operation does not reach all of it
      const unsigned extra = 1 + rng() % 3;   // (the partition has buffers and matrices for three more operations)
      std::vector<rdamd_operation_t> more(ops.begin(), ops.end() - 1);
      for (unsigned e = 0; e < extra; ++e) {   // a chain over tips 0, 1, 2 .. in front of the root operation
        rdamd_operation_t o = ops[0];
        o.parent_clv_index = n + count + e; o.parent_scaler_index = -1;
        o.child1_clv_index = e ? n + count + e - 1 : 0; o.child2_clv_index = 1 + e;
        o.child1_scaler_index = o.child2_scaler_index = -1;
        o.child1_matrix_index = o.child2_matrix_index = n_mat + e;   // (a shared index: still a valid list)
        more.push_back(o);
      }
      more.push_back(ops.back());
      const ScheduleCheck v = check(more);
      if (v.kind != ScheduleCheck::kOk || !v.matrix_shared) return fail("validation: a list with a detached subtree is a valid list");
      for (int k20 = 0; k20 < 2; ++k20) {
        rdamd::ScheduleShape sh;
        sh.tips = n; sh.sites = 100; sh.tip_stride = 100; sh.rate_cats = 2; sh.prob_matrices = mats; sh.k20 = k20 != 0;
        rdamd::Program prog;
        const unsigned lost = rdamd::compile_program(sh, more, {}, {}, prog);
        if (lost != extra) return fail("unreachable operations", (int)lost, (int)extra);
      }
      ++cases;
    }
  }
  return 0;
}

// class counts of every operation's node the way the clade cache finds them (clade_intern): from the
// children's per-site classes, 0 once a subtree has more than max_classes
static std::vector<unsigned> class_counts(const std::vector<rdamd_operation_t> &ops, unsigned n, size_t sites,
                                          const std::vector<uint8_t> &tipcodes, unsigned max_classes) {
  std::vector<unsigned> count(ops.size(), 0);
  std::vector<std::vector<uint8_t>> cls(ops.size());
  std::vector<uint8_t> cmap;
  for (size_t i = 0; i < ops.size(); ++i) {
    const unsigned ch[2] = {ops[i].child1_clv_index, ops[i].child2_clv_index};
    const uint8_t *in[2];
    unsigned cnt[2];
    bool small = true;
    for (int k = 0; k < 2; ++k) {
      if (ch[k] < n) { in[k] = tipcodes.data() + (size_t)ch[k] * sites; cnt[k] = 16; continue; }
      in[k] = cls[ch[k] - n].data(); cnt[k] = count[ch[k] - n];   // (operation k writes CLV n + k)
      if (!cnt[k]) small = false;
    }
    if (small) count[i] = rdamd::clade_classes(in[0], cnt[0], in[1], cnt[1], sites, max_classes, cls[i], cmap);
  }
  return count;
}

static int check_block(const rdamd::ScheduleBlock &b, const rdamd::Program &main_prog, const rdamd::Program *plain,
                       const rdamd::CladeSelection &sel, const std::vector<double> &brlen, bool k20, unsigned n,
                       const std::vector<rdamd_operation_t> &ops) {
  using namespace rdamd;
  const size_t mask_bytes = k20 ? 4 * ((brlen.size() + 31) / 32) : 0;
  const size_t at[6] = {b.o_prog, b.o_plain, b.o_steps, b.o_groups, b.o_brlen, b.o_tipmask};
  const size_t len[6] = {sizeof(FusedOp) * (main_prog.steps.size() + 4), plain ? sizeof(FusedOp) * (plain->steps.size() + 4) : 0,
                         sizeof(CladeStep) * sel.steps.size(), sizeof(CladeGroup) * sel.groups.size(),
                         sizeof(double) * brlen.size(), mask_bytes};
  if (b.o_prog != 0 || b.host.size() != b.total || b.total % 64) return fail("block: size");
  for (int k = 0; k < 6; ++k) {
    if (at[k] % 64) return fail("block: a piece is not 64-byte aligned", k);
    if (at[k] + len[k] > (k < 5 ? at[k + 1] : b.total)) return fail("block: a piece runs into the next", k);
  }
  auto program_at = [&](size_t off, const Program &pr) {
    const FusedOp *f = (const FusedOp *)(b.host.data() + off);
    if (memcmp(f, pr.steps.data(), sizeof(FusedOp) * pr.steps.size())) return fail("block: program");
    for (size_t k = 0; k < 4; ++k)
      if (memcmp(f + pr.steps.size() + k, &pr.steps.back(), sizeof(FusedOp))) return fail("block: the four tail steps", (int)k);
    return 0;
  };
  if (program_at(b.o_prog, main_prog) || (plain && program_at(b.o_plain, *plain))) return 1;
  if (!sel.steps.empty() && memcmp(b.host.data() + b.o_steps, sel.steps.data(), len[2])) return fail("block: clade steps");
  if (!sel.groups.empty() && memcmp(b.host.data() + b.o_groups, sel.groups.data(), len[3])) return fail("block: clade groups");
  if (memcmp(b.host.data() + b.o_brlen, brlen.data(), len[4])) return fail("block: branch lengths");
  std::set<unsigned> tip_branches;
  for (const rdamd_operation_t &o : ops) {
    if (o.child1_clv_index < n) tip_branches.insert(o.child1_matrix_index);
    if (o.child2_clv_index < n) tip_branches.insert(o.child2_matrix_index);
  }
  for (size_t m = 0; m < 8 * mask_bytes; ++m) {
    const uint32_t word = ((const uint32_t *)(b.host.data() + b.o_tipmask))[m >> 5];
    if (((word >> (m & 31)) & 1u) != tip_branches.count((unsigned)m)) return fail("block: tip mask", (int)m);
  }
  return 0;
}

static int check_clade_selection(std::mt19937 &rng, int &cases) {
  using namespace rdamd;
  unsigned long folded_ops = 0, all_ops = 0, wide_tips = 0;
  for (int rep = 0; rep < 240; ++rep) {
    unsigned n;
    std::vector<rdamd_operation_t> ops = plan_tree(rng, rep, 120, n);
    const unsigned count = (unsigned)ops.size(), n_mat = 2 * n - 2;
    const bool k20 = rep % 6 == 5, shared = rep % 8 == 3;
    if (shared) ops[rng() % count].child2_matrix_index = ops[rng() % count].child1_matrix_index;
    std::vector<unsigned> idx;
    std::vector<double> len;
    branch_list(rng, n_mat, idx, len);
    const ScheduleCheck v = validate_schedule(n, n, n_mat, ops.data(), count, idx.data(), len.data(), n_mat);
    if (v.kind != ScheduleCheck::kOk || v.matrix_shared != shared) return fail("selection: the list is valid", rep);
    ScheduleShape sh;
    sh.tips = n; sh.sites = 200 + rng() % 1801; sh.tip_stride = (sh.sites + 3u) & ~3u; sh.rate_cats = 1 + rng() % 4;
    sh.prob_matrices = n_mat; sh.k20 = k20;
    const unsigned limit = rep % 2 ? 16u : 64u;   // what a table slot holds; the cache may count further (64-row tables that do not fit)
    sh.wide_mode = !k20 && limit == 64;
    Program plain, folded;
    if (compile_program(sh, ops, {}, {}, plain)) return fail("selection: the plain program");
    CladeSelection sel;
    if (!k20) {
      // tip codes: 2 to 4 symbols; half the alignments repeat a few columns (where whole clades fold)
      const unsigned symbols = 2 + rng() % 3, pool = rep % 4 < 2 ? 0 : 3 + rng() % 78;
      std::vector<uint8_t> columns((size_t)std::max(pool, 1u) * n), tipcodes((size_t)n * sh.sites);
      for (uint8_t &x : columns) x = (uint8_t)(1u << (rng() % symbols));
      for (size_t s = 0; s < sh.sites; ++s) {
        const size_t col = pool ? rng() % pool : 0;
        for (unsigned t = 0; t < n; ++t) tipcodes[(size_t)t * sh.sites + s] = pool ? columns[col * n + t] : (uint8_t)(1u << (rng() % symbols));
      }
      const std::vector<unsigned> n_classes = class_counts(ops, n, sh.sites, tipcodes, rep % 3 == 0 ? 64u : limit);
      std::vector<unsigned> node_id(count);
      for (unsigned i = 0; i < count; ++i) node_id[i] = n + 7 * i + 1;
      sel = select_clades(ops.data(), count, n, v, node_id, n_classes, limit);
      if (sel.small.size() != count || sel.small[count - 1]) return fail("selection: the root operation is never folded");
      if (shared && (!sel.groups.empty() || !sel.steps.empty() || sel.n_wide || sel.clade_rows ||
                     std::count(sel.small.begin(), sel.small.end(), 0) != (std::ptrdiff_t)count))
        return fail("selection: a shared matrix index folds nothing");
      if (sel.groups.size() != sel.tip_ops.size()) return fail("selection: one pseudo-tip per group");
      std::vector<int> seen(count, 0);
      unsigned rows = 0, wide = 0, at = 0;
      for (size_t g = 0; g < sel.groups.size(); ++g) {
        const CladeGroup &grp = sel.groups[g];
        const unsigned top = sel.tip_ops[g];
        if (grp.first != at || grp.count == 0 || grp.first + grp.count > sel.steps.size()) return fail("selection: group bounds", (int)g);
        if (g && top <= sel.tip_ops[g - 1]) return fail("selection: groups in the order of the list", (int)g);
        if (!sel.small[top] || sel.small[v.consumer[top]]) return fail("selection: a pseudo-tip is small, its consumer is not", (int)top);
        std::vector<unsigned> op_of(grp.count);
        for (unsigned k = 0; k < grp.count; ++k) {
          const CladeStep &st = sel.steps[grp.first + k];
          const unsigned j = (st.pad - n - 1) / 7;   // (the node id carries the operation)
          if (j >= count || node_id[j] != st.pad || !sel.small[j] || seen[j]++) return fail("selection: a step is a small operation, once", (int)j);
          op_of[k] = j;
          const unsigned ch[2] = {ops[j].child1_clv_index, ops[j].child2_clv_index};
          const unsigned mt[2] = {ops[j].child1_matrix_index, ops[j].child2_matrix_index};
          for (int c = 0; c < 2; ++c) {
            if (ch[c] < n) { if (st.src[c] != mt[c]) return fail("selection: a tip child's source is its matrix", (int)j, c); continue; }
            const unsigned from = st.src[c] & 0x7fffffffu;   // the whole subtree: every inner child is a step in front
            if (!(st.src[c] & 0x80000000u) || from >= k || op_of[from] != v.producer.at(ch[c])) return fail("selection: a nested source names an earlier step of the group", (int)j, c);
          }
          const rdamd_operation_t &up = ops[v.consumer[j]];
          if (st.out_mat != (up.child1_clv_index == ops[j].parent_clv_index ? up.child1_matrix_index : up.child2_matrix_index))
            return fail("selection: the branch above", (int)j);
          if (st.n_classes != n_classes[j] || st.n_classes == 0 || st.n_classes > limit || st.map_off != 0) return fail("selection: classes", (int)j);
          if (st.last != (k + 1 == grp.count ? 1u : 0u) || (st.last && j != top)) return fail("selection: `last` sits on the group's final step, the pseudo-tip", (int)j);
          // inside the group every step but the last hands its row to a later step of the group
          if (!st.last && !sel.small[v.consumer[j]]) return fail("selection: a nested step's consumer is small", (int)j);
          const bool wants_wide = st.last && st.n_classes > 16;
          if (st.wide_slot != (wants_wide ? wide : 0xffffffffu)) return fail("selection: wide slot", (int)j, (int)st.wide_slot);
          if (wants_wide && (!sel.pseudo_wide.count(ops[j].parent_clv_index) || sel.pseudo_wide.at(ops[j].parent_clv_index) != wide)) return fail("selection: pseudo_wide", (int)j);
          wide += wants_wide;
          rows += st.n_classes;
        }
        at += grp.count;
      }
      if (at != sel.steps.size() || wide != sel.n_wide || sel.pseudo_wide.size() != wide || rows != sel.clade_rows) return fail("selection: totals", (int)rows, (int)sel.clade_rows);
      const std::vector<rdamd_operation_t> kept = sel.kept(ops.data());
      size_t next = 0;   // kept: the operations that are not small, in the list's order; with the groups' every operation once
      for (unsigned i = 0; i < count; ++i) {
        if ((sel.small[i] != 0) != (seen[i] == 1)) return fail("selection: every small operation is in one group", (int)i);
        if (sel.small[i]) continue;
        if (next >= kept.size() || kept[next++].parent_clv_index != ops[i].parent_clv_index) return fail("selection: kept", (int)i);
      }
      if (next != kept.size()) return fail("selection: kept (size)");
      if (!sel.groups.empty()) {   // the folded program: the root expression over tips and pseudo-tips
        ClvMap pseudo_row;
        for (size_t g = 0; g < sel.groups.size(); ++g) pseudo_row[ops[sel.tip_ops[g]].parent_clv_index] = n + (unsigned)g;
        ProgramTrace trace;
        if (compile_program(sh, kept, pseudo_row, sel.pseudo_wide, folded, &trace)) return fail("selection: operations of the kept list are unreachable");
        unsigned mem_depth = 0;
        if (replay(trace.c, trace.runner_up, expected(trace.c, kept, (unsigned)kept.size() - 1), mem_depth)) return 1;
        if (folded.steps.size() != kept.size()) return fail("selection: one step per kept operation");
      }
      folded_ops += count - kept.size(); all_ops += count; wide_tips += sel.n_wide;
    }
    const bool is_folded = !sel.groups.empty();
    const Program &main_prog = is_folded ? folded : plain;
    const ScheduleBlock b = pack_schedule_block(main_prog, is_folded ? &plain : nullptr, sel.steps, sel.groups, v.brlen, k20, n,
                                                ops.data(), count);
    if (check_block(b, main_prog, is_folded ? &plain : nullptr, sel, v.brlen, k20, n, ops)) return 1;
    ++cases;
  }
  std::fprintf(stderr, "clade selection: %lu of %lu operations folded, %lu 64-row pseudo-tips\n", folded_ops, all_ops, wide_tips);
  if (!folded_ops || folded_ops == all_ops || !wide_tips) return fail("selection: the cases fold nothing, or everything");
  return 0;
}

// ---- the fused 4-state evaluator's launch rule (csrc/launch_plan.hpp) ---------------------------
struct LaunchCase {
  const char *name;
  unsigned R, n_jobs, sites, tips, table_rows;
  size_t arena_bytes, table_bytes;
  unsigned depth[2], reg[2];
  // expected, worked out by hand from the rule as rdamd_evaluate_batch applies it (evaluate.hip,
  // kernels_fused.hip), not from the function under test: NS = 2 from n_jobs x blocks_x >= 8192; RW for 2 <= R <= 8, an arena of
  // >= 512 MB and no speculation; job-major for n_jobs >= 16 and 4096 / (blocks_x / 2) x table
  // bytes > 16 MB; speculation up to 256 tips; the private-segment stack for 64-row tables, one
  // register level and 2..7 in-memory levels; LDS = waves x (8 TR x 8 + LDS levels x NS x 64 x 36)
  unsigned blocks_x, ns, rw, job_major, speculate;
  unsigned rl[2], sp[2];
  size_t lds[2];
};

static rdamd::FusedLaunchInput launch_input(const LaunchCase &c) {
  rdamd::FusedLaunchInput in;
  in.rate_cats = c.R; in.n_jobs = c.n_jobs; in.blocks_x = ((c.sites + 63) / 64 + 15) / 16 * 16;
  in.tipcodes_bytes = c.arena_bytes; in.table_bytes_per_job = c.table_bytes; in.table_rows = c.table_rows;
  in.tips = c.tips;
  for (int k = 0; k < 2; ++k) { in.max_depth[k] = c.depth[k]; in.reg_levels[k] = c.reg[k]; }
  return in;
}

static int check_launch_rule(int &cases) {
  using namespace rdamd;
  const size_t MB = (size_t)1 << 20;
  // Shapes: bench.py's configs (taxa, sites, R = 4, 197-job batches, 64-row tables), 2 n - 3
  // matrices per job at 512 B per (matrix, rate) plus 2 KB per (64-row pseudo-tip, rate); arenas as
  // the kernels' notes give them (c2 16 MB, c4 850 MB, c5 340 MB); c4's stack the one that makes
  // its one-wave-per-rate launch 142 KB.  The last one is test_balanced_trees_deep_stacks' big launch.
  const LaunchCase table[] = {
      //  name        R  jobs  sites   tips TR  arena      tables                      depth   reg     bx    NS RW JM SPEC RL      SP      LDS
      {"c2",          4, 197,  50000,  100, 64, 16 * MB,   197 * 2048 + 25 * 8192,     {1, 2}, {1, 1}, 784,  2, 0, 0, 1,   {1, 1}, {0, 7}, {8704, 8704}},
      {"c4",          4, 197,  500000, 500, 64, 850 * MB,  997 * 2048 + 40 * 8192,     {7, 7}, {2, 2}, 7824, 2, 1, 0, 0,   {2, 2}, {0, 0}, {145408, 145408}},
      {"c5",          4, 197,  100000, 1000, 64, 340 * MB, 1997 * 2048 + 60 * 8192,    {5, 6}, {1, 1}, 1568, 2, 0, 1, 0,   {1, 1}, {7, 7}, {8704, 8704}},
      {"c4/8",        4, 197,  62500,  500, 64, 107 * MB,  997 * 2048 + 40 * 8192,     {7, 7}, {2, 2}, 992,  2, 0, 1, 0,   {2, 2}, {0, 0}, {36352, 36352}},
      {"d125",        4, 197,  19436,  125, 64, 9 * MB,    247 * 2048 + 20 * 8192,     {2, 3}, {1, 1}, 304,  2, 0, 1, 1,   {1, 1}, {7, 7}, {8704, 8704}},
      {"balanced700", 4, 60,   700,    192, 64, 268800,    381 * 2048,                 {6, 6}, {1, 1}, 16,   1, 0, 1, 1,   {1, 1}, {7, 7}, {6400, 6400}},
  };
  for (const LaunchCase &c : table) {
    const FusedLaunchInput in = launch_input(c);
    const FusedLaunchShape s = plan_fused_launch(in);
    std::fprintf(stderr, "launch rule %-12s blocks_x %4u: NS %u RW %u job-major %u speculate %u | pass 0: RL %u SP %u LDS %zu | pass 1: RL %u SP %u LDS %zu\n",
                 c.name, in.blocks_x, s.sites_per_lane, s.rates_across_waves, s.job_major, s.speculate, s.pass[0].reg_levels,
                 s.pass[0].spill, s.pass[0].lds_bytes, s.pass[1].reg_levels, s.pass[1].spill, s.pass[1].lds_bytes);
    if (in.blocks_x != c.blocks_x) return fail("launch rule: blocks_x of a named workload", (int)in.blocks_x, (int)c.blocks_x);
    if (s.sites_per_lane != c.ns || s.rates_across_waves != c.rw || s.job_major != c.job_major || s.speculate != c.speculate ||
        s.not_honoured != 0)
      return fail(c.name, (int)s.sites_per_lane * 1000 + (int)s.rates_across_waves * 100 + (int)s.job_major * 10 + (int)s.speculate,
                  (int)s.not_honoured);
    for (int k = 0; k < 2; ++k)
      if (s.pass[k].reg_levels != c.rl[k] || s.pass[k].spill != c.sp[k] || s.pass[k].lds_bytes != c.lds[k] ||
          s.pass[k].mem_levels != c.depth[k])
        return fail(c.name, k, (int)s.pass[k].lds_bytes);
    ++cases;
  }
  // ---- the LDS bound: one wave per rate only where R waves fit 160 KB; nothing ever asks for more ----
  static_assert(kFusedLdsLimit == 163840, "160 KB: a CU's LDS on gfx950");
  static_assert(kPlanSpillLevels == kFusedSpillLevels, "launch_plan.hpp plans the stacks of kernels_fused.hip's kernels");
  unsigned dropped = 0, kept = 0;
  for (unsigned R = 1; R <= 8; ++R)
    for (unsigned ns = 1; ns <= 2; ++ns)
      for (unsigned tr : {16u, 64u})
        for (unsigned depth = 0; depth <= 12; ++depth)
          for (unsigned reg = 1; reg <= 2; ++reg)
            for (int forced = 0; forced < 2; ++forced) {
              FusedLaunchInput in;
              in.rate_cats = R; in.n_jobs = 4; in.blocks_x = 16; in.table_rows = tr; in.tips = 1000;
              in.table_bytes_per_job = 1 << 20;
              in.max_depth[0] = 1; in.reg_levels[0] = 1;         // (a shallow folded program; the plain one decides)
              in.max_depth[1] = depth; in.reg_levels[1] = reg;
              in.force_ns = (int)ns;
              if (forced) in.force_rw = 1;
              else in.tipcodes_bytes = 600 * MB;
              const FusedLaunchShape s = plan_fused_launch(in);
              // by hand: the stack levels a wave keeps in LDS, its bytes, R of them
              const bool priv = tr == 64 && reg == 1 && depth >= 2 && depth <= 7;
              const unsigned levels = priv ? 1u : std::max(depth, 1u);
              const size_t per_wave = 8u * tr * 8u + (size_t)levels * ns * 64u * 36u;
              const bool legal_r = R >= 2;
              const bool fits = per_wave * R <= 163840u && (8u * tr * 8u + ns * 64u * 36u) * (size_t)R <= 163840u;
              const unsigned want_rw = legal_r && fits;
              const unsigned want_word = !legal_r ? (forced ? kLaunchRwRates : 0u) : fits ? 0u : (forced ? kLaunchRwLds : kLaunchRuleRwLds);
              if (s.rates_across_waves != want_rw) return fail("LDS bound: one wave per rate", (int)(R * 100 + depth), (int)(ns * 100 + tr));
              if (s.not_honoured != want_word) return fail("LDS bound: the report's word", (int)s.not_honoured, (int)want_word);
              if (s.sites_per_lane != ns || (s.pass[1].spill != 0) != priv || s.pass[1].reg_levels != (priv ? 1u : reg))
                return fail("LDS bound: stack kind", (int)(R * 100 + depth), (int)(ns * 100 + tr));
              if (s.pass[1].lds_bytes != per_wave * (want_rw ? R : 1u)) return fail("LDS bound: bytes", (int)s.pass[1].lds_bytes, (int)per_wave);
              for (int k = 0; k < 2; ++k)
                if (s.pass[k].lds_bytes > kFusedLdsLimit) return fail("LDS bound: a launch beyond the limit", (int)s.pass[k].lds_bytes);
              dropped += legal_r && !fits;
              kept += want_rw;
              ++cases;
            }
  if (!dropped || !kept) return fail("LDS bound: the sweep never crosses the limit");
  {   // the two launches that could not have fitted: 1000-taxon alignments beyond 512 MB of codes
    struct { const char *name; unsigned R, ns, tr, depth, reg; size_t bytes; } named[] = {
        {"A: R 4, two sites per lane, 64-row tables, nine in-memory levels", 4, 2, 64, 9, 2, 182272},
        {"B: R 8, two sites per lane, 16-row tables, eight in-memory levels", 8, 2, 16, 8, 2, 303104},
    };
    for (const auto &c : named) {
      FusedLaunchInput in;
      in.rate_cats = c.R; in.n_jobs = 197; in.blocks_x = 1568; in.table_rows = c.tr; in.tips = 1000;
      in.tipcodes_bytes = 600 * MB;
      for (int k = 0; k < 2; ++k) { in.max_depth[k] = c.depth; in.reg_levels[k] = c.reg; }
      const size_t would = fused_pass_shape(c.tr, c.ns, c.R, c.depth, c.reg).lds_bytes;
      const FusedLaunchShape s = plan_fused_launch(in);
      std::fprintf(stderr, "launch rule LDS case %s: one wave per rate would ask for %zu B of %zu -> RW %u, one wave: %zu B\n", c.name,
                   would, (size_t)kFusedLdsLimit, s.rates_across_waves, s.pass[0].lds_bytes);
      if (would != c.bytes) return fail("LDS case: bytes of the request", (int)would, (int)c.bytes);
      if (s.sites_per_lane != c.ns || s.rates_across_waves != 0 || s.not_honoured != kLaunchRuleRwLds ||
          s.pass[0].lds_bytes != c.bytes / c.R)
        return fail("LDS case: the rule must take the one-wave form", (int)s.rates_across_waves, (int)s.not_honoured);
      in.force_rw = 1;
      if (plan_fused_launch(in).rates_across_waves != 0 || plan_fused_launch(in).not_honoured != kLaunchRwLds)
        return fail("LDS case: forced beyond the limit");
      ++cases;
    }
  }
  {   // ---- forced values: honoured when legal, reported when not -------------------------------
    FusedLaunchInput base;
    base.rate_cats = 4; base.n_jobs = 3; base.blocks_x = 16; base.table_rows = 16; base.tips = 12;
    base.table_bytes_per_job = 21 * 2048; base.tipcodes_bytes = 12 * 64;
    const FusedLaunchShape rule = plan_fused_launch(base);
    if (rule.sites_per_lane != 1 || rule.rates_across_waves || rule.job_major || !rule.speculate || rule.not_honoured)
      return fail("forced: the small batch's defaults");
    for (int ns : {1, 2})
      for (int jm : {0, 1})
        for (int rw : {0, 1})
          for (int spec : {0, 1}) {
            FusedLaunchInput in = base;
            in.force_ns = ns; in.force_job_major = jm; in.force_rw = rw; in.speculation = spec;
            const FusedLaunchShape s = plan_fused_launch(in);
            if (s.sites_per_lane != (unsigned)ns || s.job_major != (unsigned)jm || s.speculate != (unsigned)spec)
              return fail("forced: sites per lane / job-major", ns, jm);
            if (s.rates_across_waves != (unsigned)(rw && !spec)) return fail("forced: one wave per rate", rw, spec);
            if (s.not_honoured != (rw && spec ? kLaunchRwSpeculate : 0u)) return fail("forced: word", (int)s.not_honoured);
            if (s.pass[0].lds_bytes != (size_t)(s.rates_across_waves ? 4 : 1) * (1024 + ns * 2304)) return fail("forced: bytes");
            ++cases;
          }
    for (unsigned R : {1u, 9u, 16u}) {   // one wave per rate category: 2..8 categories
      FusedLaunchInput in = base;
      in.rate_cats = R; in.force_rw = 1; in.speculation = 0;
      const FusedLaunchShape s = plan_fused_launch(in);
      if (s.rates_across_waves || s.not_honoured != kLaunchRwRates) return fail("forced: R outside 2..8", (int)R);
      in.force_rw = -1; in.tipcodes_bytes = 600 * MB;
      if (plan_fused_launch(in).rates_across_waves || plan_fused_launch(in).not_honoured) return fail("rule: R outside 2..8", (int)R);
      ++cases;
    }
    {   // the exporting launch: one job, one site per lane, plain program, all-LDS
      FusedLaunchInput in = base;
      in.n_jobs = 1; in.export_children = true; in.max_depth[1] = 3; in.reg_levels[1] = 2;
      FusedLaunchShape s = plan_fused_launch(in);
      if (s.sites_per_lane != 1 || s.rates_across_waves || s.job_major || s.speculate || s.not_honoured ||
          s.pass[1].reg_levels != 2 || s.pass[1].spill || s.pass[1].lds_bytes != 1024 + 3 * 2304)
        return fail("export: defaults");
      in.force_ns = 2; in.force_rw = 1; in.force_job_major = 1;
      s = plan_fused_launch(in);
      if (s.sites_per_lane != 1 || s.rates_across_waves || s.job_major ||
          s.not_honoured != (kLaunchRwExport | kLaunchNsExport | kLaunchJobMajorExport))
        return fail("export: forced values", (int)s.not_honoured);
      ++cases;
    }
    {   // values the seam refuses never reach the rule; should one, it is the rule's choice
      FusedLaunchInput in = base;
      in.force_ns = 3; in.force_rw = 7; in.force_job_major = -5;
      const FusedLaunchShape s = plan_fused_launch(in);
      if (s.sites_per_lane != rule.sites_per_lane || s.rates_across_waves != rule.rates_across_waves || s.job_major != rule.job_major)
        return fail("forced: out-of-range values");
      ++cases;
    }
  }
  return 0;
}

int main() {
  std::mt19937 rng(20240603);
  int cases = 0;
  if (check_compiler(rng, cases)) return 1;
  // ---- clade_classes ------------------------------------------------------------------------
  for (int rep = 0; rep < 400; ++rep) {
    const unsigned na = 1 + rng() % 64, nb = 1 + rng() % 64, limit = rep % 3 == 0 ? 16 : 64;
    const size_t S = rep % 7 == 0 ? 1 : 1 + rng() % 3000;
    const unsigned ua = 1 + rng() % na, ub = 1 + rng() % nb;   // values actually used: keeps many cases under the limit
    std::vector<uint8_t> a(S), b(S), cls, cmap;
    for (size_t s = 0; s < S; ++s) { a[s] = (uint8_t)(rng() % ua); b[s] = (uint8_t)(rng() % ub); }
    const unsigned got = rdamd::clade_classes(a.data(), na, b.data(), nb, S, limit, cls, cmap);
    std::map<std::pair<int, int>, int> first;   // brute force, first appearance order
    for (size_t s = 0; s < S; ++s) first.emplace(std::make_pair(a[s], b[s]), (int)first.size());
    if (first.size() > limit) {
      if (got != 0 || !cls.empty() || !cmap.empty()) return fail("over the limit must return 0", (int)first.size(), (int)got);
    } else {
      if (got != first.size()) return fail("class count", (int)got, (int)first.size());
      if (cmap.size() != 2 * got) return fail("map size");
      std::map<std::pair<int, int>, int> order;
      for (size_t s = 0; s < S; ++s) {
        auto it = order.emplace(std::make_pair(a[s], b[s]), (int)order.size()).first;
        if (cls[s] != it->second) return fail("class id is not the order of first appearance", (int)s);
        if (cmap[2 * cls[s]] != a[s] || cmap[2 * cls[s] + 1] != b[s]) return fail("class map", (int)s);
      }
    }
    ++cases;
  }
  // ---- k20_split ----------------------------------------------------------------------------
  for (int rep = 0; rep < 300; ++rep) {
    const unsigned n = 3 + rng() % 400;
    std::vector<rdamd_operation_t> ops = random_postorder(n, rng);
    const unsigned count = (unsigned)ops.size();
    std::vector<rdamd_operation_t> order;
    std::vector<unsigned> bounds;
    rdamd::k20_split(n, 2 * n, ops.data(), count, 8, order, bounds);
    if (order.empty()) {
      if (!bounds.empty()) return fail("bounds without an order");
      // allowed: short lists, or a tree that does not split into >= 2 pieces
      if (count >= 24) {
        // a list this long only stays whole when the root's children cannot both be pieces,
        // i.e. the root operation has a tip child and so on down (a caterpillar-like top)
        ++cases;
      }
      continue;
    }
    if (order.size() != count) return fail("not a permutation (size)");
    const unsigned np = (unsigned)bounds.size() - 1, top = bounds[np];
    if (np < 2 || np > 8 || bounds[0] != 0) return fail("piece count", (int)np);
    std::set<unsigned> seen;
    std::vector<int> piece_of_clv(3 * n, -2);   // -2: tip / unknown, -1: top, k: piece k
    for (unsigned k = 0; k <= np; ++k) {
      const unsigned lo = bounds[k], hi = k < np ? bounds[k + 1] : count;
      if (k < np && k > 0 && hi - lo > bounds[k] - bounds[k - 1]) return fail("pieces must come longest first", (int)k);
      if (k < np && hi - lo > std::max(12u, count / 4) && np < 8) return fail("an oversized piece was not split", (int)(hi - lo));
      std::set<unsigned> produced;
      for (unsigned i = lo; i < hi; ++i) {
        const rdamd_operation_t &o = order[i];
        if (!seen.insert(o.parent_clv_index).second) return fail("operation twice");
        for (unsigned ch : {o.child1_clv_index, o.child2_clv_index}) {
          if (ch < n) continue;
          if (k < np) {   // a piece reads only what it produced itself, earlier
            if (!produced.count(ch)) return fail("a piece reads from outside itself", (int)k, (int)i);
          } else if (piece_of_clv[ch] == -2) {
            return fail("a top operation reads something not computed yet", (int)i);
          }
        }
        produced.insert(o.parent_clv_index);
        piece_of_clv[o.parent_clv_index] = k < np ? (int)k : -1;
        if (i > lo && rdamd::k20_hazard(n, order.data(), i, lo) && k < np) return fail("hazard inside a piece");
      }
      // a piece is a whole subtree: exactly one of its results is consumed outside it
      if (k < np) {
        unsigned leaving = 0;
        for (unsigned i = top; i < count; ++i)
          for (unsigned ch : {order[i].child1_clv_index, order[i].child2_clv_index})
            if (produced.count(ch)) ++leaving;
        if (leaving != 1) return fail("a piece must hand exactly one CLV to the top list", (int)k, (int)leaving);
      }
    }
    if (order[count - 1].parent_clv_index != ops[count - 1].parent_clv_index) return fail("the root operation must stay last");
    ++cases;
  }
  // ---- list_levels (the 4-state traversal kernel's launches) --------------------------------
  for (int rep = 0; rep < 300; ++rep) {
    const unsigned n = 3 + rng() % 600;
    std::vector<rdamd_operation_t> ops = random_postorder(n, rng);
    const unsigned count = (unsigned)ops.size();
    const unsigned max_pieces = 2 + rng() % 31, small = 4 + rng() % 12, min_count = 6 + rng() % 24;
    rdamd::ListLevels lv;
    rdamd::list_levels(n, 2 * n, ops.data(), count, max_pieces, small, min_count, lv);
    if (lv.order.empty()) {
      if (!lv.seg.empty() || !lv.level.empty()) return fail("levels without an order");
      ++cases;
      continue;
    }
    if (lv.order.size() != count) return fail("levels: not a permutation (size)");
    if (lv.seg.front() != 0 || lv.seg.back() != count) return fail("levels: segment bounds");
    if (lv.level.front() != 0 || lv.level.back() != lv.seg.size() - 1) return fail("levels: launch bounds");
    if (lv.level.size() < 3) return fail("levels: a cut list has at least two launches");
    std::set<unsigned> done_before;   // CLVs of earlier launches
    std::set<unsigned> seen;
    for (size_t l = 0; l + 1 < lv.level.size(); ++l) {
      const unsigned s0 = lv.level[l], s1 = lv.level[l + 1];
      if (s1 <= s0 || s1 - s0 > std::max(max_pieces, 1u)) return fail("levels: pieces per launch", (int)(s1 - s0));
      if (l + 2 == lv.level.size() && s1 - s0 != 1) return fail("levels: the last launch is one list");
      std::set<unsigned> this_launch;
      for (unsigned seg = s0; seg < s1; ++seg) {
        if (lv.seg[seg + 1] <= lv.seg[seg]) return fail("levels: empty segment");
        std::set<unsigned> produced;
        for (unsigned i = lv.seg[seg]; i < lv.seg[seg + 1]; ++i) {
          const rdamd_operation_t &o = lv.order[i];
          if (!seen.insert(o.parent_clv_index).second) return fail("levels: operation twice");
          for (unsigned ch : {o.child1_clv_index, o.child2_clv_index})
            if (ch >= n && !produced.count(ch) && !done_before.count(ch))
              return fail("levels: a segment reads what neither it nor an earlier launch computed", (int)l, (int)i);
          produced.insert(o.parent_clv_index);
        }
        this_launch.insert(produced.begin(), produced.end());
      }
      done_before.insert(this_launch.begin(), this_launch.end());
    }
    if (lv.order[count - 1].parent_clv_index != ops[count - 1].parent_clv_index) return fail("levels: the root operation must stay last");
    ++cases;
  }
  {   // two operations writing one scale buffer may not end up side by side -> no split
    std::vector<rdamd_operation_t> ops = random_postorder(200, rng);
    ops[40].parent_scaler_index = ops[120].parent_scaler_index = 7;
    std::vector<rdamd_operation_t> order;
    std::vector<unsigned> bounds;
    rdamd::k20_split(200, 400, ops.data(), (unsigned)ops.size(), 8, order, bounds);
    if (!order.empty() || !bounds.empty()) return fail("a shared scale buffer must keep the list whole");
    ++cases;
  }
  {   // not a post-order nest: two operations swapped across subtrees -> no split
    std::vector<rdamd_operation_t> ops = random_postorder(200, rng);
    std::swap(ops[3], ops[150]);
    std::vector<rdamd_operation_t> order;
    std::vector<unsigned> bounds;
    rdamd::k20_split(200, 400, ops.data(), (unsigned)ops.size(), 8, order, bounds);
    if (!order.empty() || !bounds.empty()) return fail("a list that is no nest of subtree ranges must not be split");
    ++cases;
  }
  if (check_planner(rng, cases)) return 1;
  if (check_validation(rng, cases) || check_clade_selection(rng, cases)) return 1;
  if (check_launch_rule(cases)) return 1;
  std::printf("host logic OK %d\n", cases);
  return 0;
}
