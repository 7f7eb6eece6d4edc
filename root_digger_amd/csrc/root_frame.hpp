// What the analyses at a root (model.hpp) read off a schedule before any kernel runs: the nodes in
// pre-order, every branch's place in the schedule's matrix list and its length, and where a
// partition's columns go in the concatenated rows.  Pure host logic -- no HIP, no model_t -- so that
// tests/cpp/root_frame_check.cpp can replay it without a GPU (as outer_plan.hpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <unordered_map>
#include <vector>

#include "outer_plan.hpp"

namespace rdamd {

// Node k is the parent of operation n_ops - 1 - k (plan_outer_program's order, which
// rdamd_marginal_ancestral_nodes hands out: the root first); branch (k, c) hangs above child c of node k.
struct RootFrame {
  int bad_op = -1;            // >= 0: not a complete post-order traversal; refused at this operation, `why` says why
  const char *why = nullptr;
  std::vector<unsigned> node_clv, node_children;   // [nodes], [nodes][2]
  std::vector<int> node_parent;                    // [nodes]; -1: the root
  std::vector<size_t> place;                       // [nodes][2]: the branch's entry in the schedule's matrix list
  std::vector<double> lengths;                     // [nodes][2]
};

// The frame of generate_operations' schedule (operations, matrix indices, branch lengths).  nodes =
// false: the branches only, and no check of the traversal.  A branch whose matrix is not in the list
// throws std::out_of_range.
inline RootFrame root_frame(const std::vector<rdamd_operation_t> &ops, const std::vector<unsigned> &pmi,
                            const std::vector<double> &brl, bool nodes = true) {
  RootFrame f;
  const unsigned n_ops = (unsigned)ops.size();
  if (nodes) {
    // (tips are the CLVs below every parent, as the tree numbers them)
    unsigned tips = ~0u;
    for (const rdamd_operation_t &o : ops) tips = std::min(tips, o.parent_clv_index);
    const OuterPlan plan = plan_outer_program(ops.data(), n_ops, tips);
    if (plan.bad_op >= 0) { f.bad_op = plan.bad_op; f.why = plan.why; return f; }
    f.node_clv.resize(n_ops);
    f.node_parent.resize(n_ops);
    f.node_children.resize(2 * (size_t)n_ops);
    f.node_parent[0] = -1;
    for (unsigned k = 0; k < n_ops; ++k) {
      const OuterOp &d = plan.prog[k];
      f.node_clv[k] = d.parent_clv;
      for (int c = 0; c < 2; ++c) {
        f.node_children[2 * k + c] = d.child_clv[c];
        if (d.inner[c]) f.node_parent[d.node[c]] = (int)k;
      }
    }
  }
  std::unordered_map<unsigned, size_t> place;
  for (size_t i = 0; i < pmi.size(); ++i) place[pmi[i]] = i;
  f.place.resize(2 * (size_t)n_ops);
  f.lengths.resize(f.place.size());
  for (unsigned k = 0; k < n_ops; ++k) {
    const rdamd_operation_t &o = ops[n_ops - 1 - k];
    const unsigned mat[2] = {o.child1_matrix_index, o.child2_matrix_index};
    for (int c = 0; c < 2; ++c) {
      f.place[2 * k + c] = place.at(mat[c]);
      f.lengths[2 * k + c] = brl[f.place[2 * k + c]];
    }
  }
  return f;
}

// One partition's [rows][sites * width] block into the concatenated rows: row r goes to
// dst[(r * total + at) * width ...], `at` the partition's first pattern of `total`.
template <class T>
void scatter_columns(const T *src, size_t rows, size_t sites, size_t width, size_t total, size_t at, T *dst) {
  for (size_t r = 0; r < rows; ++r)
    std::copy(src + r * sites * width, src + (r + 1) * sites * width, dst + (r * total + at) * width);
}

}  // namespace rdamd
