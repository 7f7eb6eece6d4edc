// Replays the pre-order programs of csrc/outer_plan.hpp symbolically, without a GPU: every outer
// vector is produced exactly once before it is read, it is read from where the plan says it is, no
// workspace slot is overwritten while live, and the slot count is the liveness maximum (computed
// here from the topology alone).  Malformed lists are refused.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "outer_plan.hpp"

using namespace rdamd;

static unsigned g_checks = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);     \
      std::printf(__VA_ARGS__);                                           \
      std::printf("\n");                                                  \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

// a rooted binary tree: node < tips is a tip, others have two children
struct Tree {
  unsigned tips = 0;
  std::vector<int> left, right;   // per node id of the builder (not a CLV index)
  int root = -1;
  int tip() { left.push_back(-1); right.push_back(-1); return (int)left.size() - 1; }
  int join(int a, int b) { left.push_back(a); right.push_back(b); return (int)left.size() - 1; }
};

// post-order operation list; tips get CLVs 0.., inner nodes tips.. in the order they are emitted
static std::vector<rdamd_operation_t> post_order(const Tree &t) {
  std::vector<rdamd_operation_t> ops;
  std::vector<unsigned> clv(t.left.size(), 0);
  unsigned next_tip = 0, next_inner = t.tips;
  struct Frame { int node; int stage; };
  std::vector<Frame> stack{{t.root, 0}};
  while (!stack.empty()) {
    Frame &f = stack.back();
    const int n = f.node;
    if (t.left[n] < 0) { clv[n] = next_tip++; stack.pop_back(); continue; }
    if (f.stage == 0) { f.stage = 1; stack.push_back({t.left[n], 0}); continue; }
    if (f.stage == 1) { f.stage = 2; stack.push_back({t.right[n], 0}); continue; }
    clv[n] = next_inner++;
    rdamd_operation_t o{};
    o.parent_clv_index = clv[n]; o.parent_scaler_index = (int)(clv[n] - t.tips);
    o.child1_clv_index = clv[t.left[n]]; o.child1_matrix_index = clv[t.left[n]];
    o.child1_scaler_index = t.left[t.left[n]] < 0 ? -1 : (int)(clv[t.left[n]] - t.tips);
    o.child2_clv_index = clv[t.right[n]]; o.child2_matrix_index = clv[t.right[n]];
    o.child2_scaler_index = t.left[t.right[n]] < 0 ? -1 : (int)(clv[t.right[n]] - t.tips);
    ops.push_back(o);
    stack.pop_back();
  }
  return ops;
}

static Tree caterpillar(unsigned tips, bool deep_first) {
  Tree t;
  t.tips = tips;
  int spine = t.join(t.tip(), t.tip());
  for (unsigned i = 2; i < tips; ++i) {
    const int leaf = t.tip();
    spine = deep_first ? t.join(spine, leaf) : t.join(leaf, spine);
  }
  t.root = spine;
  return t;
}

static int balanced_rec(Tree &t, unsigned depth) {
  if (depth == 0) return t.tip();
  const int a = balanced_rec(t, depth - 1), b = balanced_rec(t, depth - 1);
  return t.join(a, b);
}
static Tree balanced(unsigned depth) {
  Tree t;
  t.tips = 1u << depth;
  t.root = balanced_rec(t, depth);
  return t;
}

static Tree random_tree(unsigned tips, std::mt19937 &rng) {
  Tree t;
  t.tips = tips;
  std::vector<int> pool;
  for (unsigned i = 0; i < tips; ++i) pool.push_back(t.tip());
  while (pool.size() > 1) {
    std::uniform_int_distribution<size_t> pick(0, pool.size() - 1);
    const size_t i = pick(rng);
    const int a = pool[i];
    pool.erase(pool.begin() + (long)i);
    std::uniform_int_distribution<size_t> pick2(0, pool.size() - 1);
    const size_t j = pick2(rng);
    const int b = pool[j];
    pool[j] = t.join(a, b);
  }
  t.root = pool[0];
  return t;
}

// the liveness maximum from the list alone: the vector of an inner child waits in the workspace from
// its parent's operation to its own unless its own is the next one
static unsigned liveness_max(const std::vector<rdamd_operation_t> &ops, unsigned tips) {
  const unsigned n = (unsigned)ops.size();
  std::vector<int> own(tips + n, -1);   // clv -> program index of the operation that has it as parent
  for (unsigned k = 0; k < n; ++k) own[ops[n - 1 - k].parent_clv_index] = (int)k;
  std::vector<int> delta(n + 1, 0);
  for (unsigned k = 0; k < n; ++k) {
    const rdamd_operation_t &o = ops[n - 1 - k];
    for (unsigned c : {o.child1_clv_index, o.child2_clv_index}) {
      if (c < tips) continue;
      const unsigned kc = (unsigned)own[c];
      if (kc == k + 1) continue;
      delta[k] += 1;      // live after operation k ...
      delta[kc] -= 1;     // ... until operation kc has read it
    }
  }
  int live = 0, best = 0;
  for (unsigned k = 0; k < n; ++k) { live += delta[k]; best = std::max(best, live); }
  return (unsigned)best;
}

static unsigned replay(const std::vector<rdamd_operation_t> &ops, unsigned tips, const char *what) {
  const unsigned n = (unsigned)ops.size();
  const OuterPlan plan = plan_outer_program(ops.data(), n, tips);
  CHECK(plan.bad_op < 0, "%s: refused at %d: %s", what, plan.bad_op, plan.why ? plan.why : "");
  CHECK(plan.prog.size() == n, "%s: program length", what);
  std::vector<int> slots(plan.slots, -1);
  std::vector<int> produced(tips + n, 0), read(tips + n, 0);
  int reg = -1;
  unsigned live_max = 0;
  for (unsigned k = 0; k < n; ++k) {
    const OuterOp &d = plan.prog[k];
    const rdamd_operation_t &o = ops[n - 1 - k];
    CHECK(d.op == n - 1 - k && d.parent_clv == o.parent_clv_index, "%s: op %u is not the list read backwards", what, k);
    CHECK(d.child_clv[0] == o.child1_clv_index && d.child_clv[1] == o.child2_clv_index &&
          d.child_mat[0] == o.child1_matrix_index && d.child_mat[1] == o.child2_matrix_index, "%s: op %u children", what, k);
    // the parent's vector
    if (k == 0) {
      CHECK(d.parent_src == kOuterFromPi, "%s: the root's vector is the frequencies", what);
    } else {
      CHECK(produced[d.parent_clv] == 1, "%s: op %u reads a vector never produced", what, k);
      if (d.parent_src == kOuterFromReg) {
        CHECK(reg == (int)d.parent_clv, "%s: op %u: the registers hold %d, not %u", what, k, reg, d.parent_clv);
      } else {
        CHECK(d.parent_src == kOuterFromSlot, "%s: op %u: only the root reads the frequencies", what, k);
        CHECK(d.parent_slot < plan.slots && slots[d.parent_slot] == (int)d.parent_clv,
              "%s: op %u: slot %u does not hold %u", what, k, d.parent_slot, d.parent_clv);
        slots[d.parent_slot] = -1;
      }
      read[d.parent_clv] += 1;
    }
    reg = -1;   // the registers are overwritten by this operation's results
    unsigned in_reg = 0;
    for (int c = 0; c < 2; ++c) {
      const unsigned clv = d.child_clv[c];
      CHECK(d.inner[c] == (clv >= tips ? 1u : 0u), "%s: op %u child %d inner flag", what, k, c);
      if (!d.inner[c]) {
        CHECK(d.keep[c] == kOuterDrop, "%s: op %u keeps a tip's vector", what, k);
        continue;
      }
      CHECK(d.node[c] > k && d.node[c] < n && plan.prog[d.node[c]].parent_clv == clv, "%s: op %u child %d node", what, k, c);
      produced[clv] += 1;
      CHECK(produced[clv] == 1, "%s: the vector of %u is produced twice", what, clv);
      if (d.keep[c] == kOuterKeepReg) {
        CHECK(d.node[c] == k + 1, "%s: op %u keeps in registers what the next operation does not read", what, k);
        reg = (int)clv;
        ++in_reg;
      } else {
        CHECK(d.keep[c] == kOuterKeepSlot, "%s: op %u drops the vector of inner node %u", what, k, clv);
        CHECK(d.slot[c] < plan.slots && slots[d.slot[c]] < 0, "%s: op %u overwrites live slot %u", what, k, d.slot[c]);
        slots[d.slot[c]] = (int)clv;
      }
    }
    CHECK(in_reg <= 1, "%s: op %u keeps two vectors in one set of registers", what, k);
    live_max = std::max(live_max, (unsigned)std::count_if(slots.begin(), slots.end(), [](int v) { return v >= 0; }));
  }
  for (unsigned i = 0; i + 1 < n; ++i)
    CHECK(read[ops[i].parent_clv_index] == 1, "%s: the vector of %u is read %d times", what, ops[i].parent_clv_index,
          read[ops[i].parent_clv_index]);
  CHECK(std::all_of(slots.begin(), slots.end(), [](int v) { return v < 0; }), "%s: a slot is still live at the end", what);
  const unsigned want = liveness_max(ops, tips);
  CHECK(plan.slots == want && live_max == want, "%s: %u slots, replay saw %u live, liveness maximum %u", what, plan.slots,
        live_max, want);
  return plan.slots;
}

static void refused(std::vector<rdamd_operation_t> ops, unsigned tips, const char *what) {
  const OuterPlan plan = plan_outer_program(ops.data(), (unsigned)ops.size(), tips);
  CHECK(plan.bad_op >= 0 && plan.why && plan.prog.empty(), "%s: accepted", what);
}

int main() {
  for (unsigned tips = 4; tips <= 300; ++tips)
    for (int deep_first = 0; deep_first < 2; ++deep_first) {
      const Tree t = caterpillar(tips, deep_first != 0);
      CHECK(replay(post_order(t), tips, "caterpillar") <= 1, "a caterpillar of %u tips needs more than one slot", tips);
    }
  for (unsigned d = 1; d <= 9; ++d)
    CHECK(replay(post_order(balanced(d)), 1u << d, "balanced") <= d, "a balanced tree of depth %u needs more than %u slots", d, d);
  std::mt19937 rng(20240611u);
  for (unsigned rep = 0; rep < 400; ++rep) {
    const unsigned tips = 3 + rng() % 120;
    replay(post_order(random_tree(tips, rng)), tips, "random");
  }
  {   // two tips: one operation, the root's
    Tree t;
    t.tips = 2;
    t.root = t.join(t.tip(), t.tip());
    CHECK(replay(post_order(t), 2, "two tips") == 0, "two tips need no slot");
  }

  // ---- malformed lists -----------------------------------------------------------------
  std::mt19937 rng2(7u);
  const Tree t = random_tree(12, rng2);
  const std::vector<rdamd_operation_t> good = post_order(t);
  replay(good, 12, "the well-formed list");
  {   // root operation not last
    std::vector<rdamd_operation_t> ops = good;
    std::swap(ops[ops.size() - 1], ops[ops.size() - 2]);
    refused(ops, 12, "root operation not last");
    ops = good;
    ops.push_back(post_order(caterpillar(3, true))[0]);   // a second tree behind the root: tips 0 and 1 again
    refused(ops, 12, "operations behind the root");
    ops = good;
    ops.pop_back();   // the root operation is missing: its children hang under nothing
    if (ops.size() > 1) refused(ops, 12, "no root operation");
  }
  {   // a child used twice
    std::vector<rdamd_operation_t> ops = good;
    ops.back().child2_clv_index = ops.back().child1_clv_index;
    refused(ops, 12, "both children the same");
    ops = good;
    ops.back().child2_clv_index = ops.front().child1_clv_index;   // a tip (or clade) that already hangs elsewhere
    refused(ops, 12, "a child under two operations");
  }
  {   // a missing subtree
    std::vector<rdamd_operation_t> ops = good;
    for (size_t i = 0; i < ops.size(); ++i)
      if (ops[i].child1_clv_index >= 12 || ops[i].child2_clv_index >= 12) {
        const unsigned inner = ops[i].child1_clv_index >= 12 ? ops[i].child1_clv_index : ops[i].child2_clv_index;
        for (size_t j = 0; j < i; ++j)
          if (ops[j].parent_clv_index == inner) { ops.erase(ops.begin() + (long)j); break; }
        break;
      }
    refused(ops, 12, "a missing subtree");
    ops = good;
    ops.front().parent_clv_index = 3;   // a tip as parent
    refused(ops, 12, "a tip as parent");
    refused({}, 12, "an empty list");
  }
  std::printf("outer plan OK %u\n", g_checks);
  return 0;
}
