// csrc/root_frame.hpp without a device (tests/test_root_frame_host.py): the frame of hand-written
// schedules of 3, 4 and 5 tips -- caterpillars, balanced trees, a root whose child is a tip --
//   node arrays      against plan_outer_program's own output (and: node k is operation n - 1 - k)
//   place, length    of every branch against a linear search of the matrix list
//   refusals         an incomplete traversal (as plan_outer_program refuses it); a matrix not in the list
// and scatter_columns against an index-by-index loop: two and three partitions, widths 1, 4 and
// 20, a partition of 0 sites first, in the middle and last, uint8_t and double.  Prints the number
// of checks.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "root_frame.hpp"

namespace {

long checks = 0;

void expect(bool ok, const char *what, const char *name, long a = 0, long b = 0) {
  ++checks;
  if (!ok) {
    std::printf("FAIL %s: %s (%ld, %ld)\n", name, what, a, b);
    std::exit(1);
  }
}

// the matrix above CLV c (any one-to-one numbering will do; not the CLV's own number)
unsigned mat(unsigned clv) { return 40 - 3 * clv; }

rdamd_operation_t op(unsigned parent, unsigned c1, unsigned c2) {
  rdamd_operation_t o{};
  o.parent_clv_index = parent;
  o.child1_clv_index = c1; o.child1_matrix_index = mat(c1);
  o.child2_clv_index = c2; o.child2_matrix_index = mat(c2);
  o.parent_scaler_index = o.child1_scaler_index = o.child2_scaler_index = -1;
  return o;
}

struct Schedule {
  const char *name;
  unsigned tips;
  std::vector<rdamd_operation_t> ops;
};

void check_frame(const Schedule &s) {
  const unsigned n = (unsigned)s.ops.size();
  // the matrix list: every child's matrix, last operation first, and one entry no branch uses
  std::vector<unsigned> pmi;
  std::vector<double> brl;
  for (unsigned i = n; i-- > 0;)
    for (unsigned m : {s.ops[i].child2_matrix_index, s.ops[i].child1_matrix_index}) {
      if (pmi.size() == 3) { pmi.push_back(1000); brl.push_back(99.0); }
      pmi.push_back(m);
      brl.push_back(0.01 + 0.125 * (double)pmi.size());
    }
  const rdamd::RootFrame f = rdamd::root_frame(s.ops, pmi, brl);
  expect(f.bad_op < 0 && f.why == nullptr, "a complete traversal is taken", s.name, f.bad_op);
  expect(f.node_clv.size() == n && f.node_parent.size() == n && f.node_children.size() == 2 * n, "node array sizes", s.name);
  expect(f.place.size() == 2 * n && f.lengths.size() == 2 * n, "branch array sizes", s.name);

  const rdamd::OuterPlan plan = rdamd::plan_outer_program(s.ops.data(), n, s.tips);
  expect(plan.bad_op < 0 && plan.prog.size() == n, "the plan itself", s.name);
  std::vector<int> parent(n, -2);
  parent[0] = -1;
  for (unsigned k = 0; k < n; ++k) {
    const rdamd::OuterOp &d = plan.prog[k];
    expect(d.op == n - 1 - k, "node k is operation n - 1 - k", s.name, k, d.op);
    expect(f.node_clv[k] == d.parent_clv && f.node_clv[k] == s.ops[n - 1 - k].parent_clv_index, "node_clv", s.name, k);
    for (int c = 0; c < 2; ++c) {
      expect(f.node_children[2 * k + c] == d.child_clv[c], "node_children", s.name, k, c);
      if (d.inner[c]) parent[d.node[c]] = (int)k;
    }
  }
  for (unsigned k = 0; k < n; ++k) {
    expect(f.node_parent[k] == parent[k], "node_parent", s.name, k, f.node_parent[k]);
    if (k == 0) continue;
    const unsigned up = (unsigned)f.node_parent[k];
    expect(up < k && (f.node_children[2 * up] == f.node_clv[k] || f.node_children[2 * up + 1] == f.node_clv[k]),
           "a node hangs under its parent, which comes first", s.name, k, up);
  }
  for (unsigned k = 0; k < n; ++k) {
    const rdamd_operation_t &o = s.ops[n - 1 - k];
    const unsigned m[2] = {o.child1_matrix_index, o.child2_matrix_index};
    for (int c = 0; c < 2; ++c) {
      size_t found = pmi.size();
      for (size_t i = 0; i < pmi.size(); ++i)
        if (pmi[i] == m[c]) found = i;
      expect(found < pmi.size() && f.place[2 * k + c] == found, "place", s.name, k, c);
      expect(f.lengths[2 * k + c] == brl[found], "length", s.name, k, c);
    }
  }
  // the branches alone: the same places and lengths, no node arrays
  const rdamd::RootFrame g = rdamd::root_frame(s.ops, pmi, brl, false);
  expect(g.bad_op < 0 && g.node_clv.empty() && g.node_parent.empty() && g.node_children.empty(), "no nodes on request", s.name);
  expect(g.place == f.place && g.lengths == f.lengths, "the branches without the nodes", s.name);

  // an incomplete traversal: the list with one operation taken out gets plan_outer_program's
  // verdict.  (Not every such list is incomplete: the CLVs below every parent count as tips, so
  // without its first or last operation a list can be the traversal of a smaller tree.  From three
  // operations on, some inner child loses the operation that made it.)
  unsigned refused = 0;
  for (unsigned gone = 0; gone < n && n >= 2; ++gone) {
    std::vector<rdamd_operation_t> cut(s.ops);
    cut.erase(cut.begin() + gone);
    unsigned tips = ~0u;
    for (const rdamd_operation_t &o : cut) tips = std::min(tips, o.parent_clv_index);
    const rdamd::OuterPlan bad = rdamd::plan_outer_program(cut.data(), n - 1, tips);
    const rdamd::RootFrame r = rdamd::root_frame(cut, pmi, brl);
    expect(r.bad_op == bad.bad_op && r.why == bad.why, "the plan's verdict", s.name, gone, r.bad_op);
    if (r.bad_op < 0) continue;
    ++refused;
    expect(r.why != nullptr && r.node_clv.empty() && r.node_parent.empty() && r.node_children.empty() && r.place.empty() &&
               r.lengths.empty(), "a refused frame is empty", s.name, gone);
  }
  if (n >= 3) expect(refused >= 1, "a missing subtree is refused", s.name, refused);
  // a branch whose matrix is not in the list
  std::vector<unsigned> short_pmi(pmi.begin(), pmi.end() - 1);
  bool thrown = false;
  try { rdamd::root_frame(s.ops, short_pmi, brl); } catch (const std::out_of_range &) { thrown = true; }
  expect(thrown, "a missing matrix is refused", s.name);
}

template <class T>
void check_scatter(const std::vector<size_t> &sites, size_t rows, size_t width, const char *name) {
  size_t total = 0;
  for (size_t s : sites) total += s;
  const T untouched = (T)250;
  std::vector<T> got(rows * total * width, untouched), want(got);
  size_t at = 0;
  unsigned v = 1;
  for (size_t s : sites) {
    std::vector<T> block(rows * s * width);
    for (T &x : block) x = (T)(v++ % 199);   // never `untouched`
    rdamd::scatter_columns(block.data(), rows, s, width, total, at, got.data());
    for (size_t r = 0; r < rows; ++r)
      for (size_t i = 0; i < s; ++i)
        for (size_t j = 0; j < width; ++j) want[((r * total) + at + i) * width + j] = block[(r * s + i) * width + j];
    at += s;
  }
  for (size_t i = 0; i < got.size(); ++i) {
    expect(got[i] == want[i], "scatter", name, (long)i, (long)width);
    expect(got[i] != untouched, "every column is written", name, (long)i, (long)width);
  }
}

}  // namespace

int main() {
  const std::vector<Schedule> schedules = {
      {"3 tips ((0,1),2)", 3, {op(3, 0, 1), op(4, 3, 2)}},
      {"4 tips caterpillar (((0,1),2),3)", 4, {op(4, 0, 1), op(5, 4, 2), op(6, 5, 3)}},
      {"4 tips balanced ((0,1),(2,3))", 4, {op(4, 0, 1), op(5, 2, 3), op(6, 4, 5)}},
      {"4 tips, tip first (3,(2,(1,0)))", 4, {op(6, 1, 0), op(4, 2, 6), op(5, 3, 4)}},
      {"5 tips caterpillar ((((0,1),2),3),4)", 5, {op(5, 0, 1), op(6, 5, 2), op(7, 6, 3), op(8, 7, 4)}},
      {"5 tips balanced ((0,1),((2,3),4))", 5, {op(5, 0, 1), op(6, 2, 3), op(7, 6, 4), op(8, 5, 7)}},
      {"5 tips, the root's child a tip (((0,1),(2,3)),4)", 5, {op(5, 0, 1), op(6, 2, 3), op(7, 5, 6), op(8, 7, 4)}},
      {"5 tips, subtrees interleaved ((3,4),(2,(0,1)))", 5, {op(8, 0, 1), op(5, 3, 4), op(6, 2, 8), op(7, 5, 6)}},
  };
  for (const Schedule &s : schedules) check_frame(s);
  // two more lists that are no complete post-order: two cherries and no root above them; none at all
  const std::vector<unsigned> pmi = {mat(0), mat(1), mat(2), mat(3)};
  const std::vector<double> brl = {0.1, 0.2, 0.3, 0.4};
  const rdamd::RootFrame rootless = rdamd::root_frame({op(4, 0, 1), op(5, 2, 3)}, pmi, brl);
  expect(rootless.bad_op == 0 && rootless.why != nullptr && rootless.node_clv.empty(), "two cherries, no root", "refusals",
         rootless.bad_op);
  const rdamd::RootFrame none = rdamd::root_frame({}, pmi, brl);
  expect(none.bad_op == 0 && none.why != nullptr, "an empty list", "refusals", none.bad_op);

  const std::vector<std::vector<size_t>> splits = {{5, 7}, {1, 1}, {0, 6}, {6, 0}, {3, 4, 2}, {0, 3, 5}, {4, 0, 2}, {3, 2, 0}};
  for (const auto &sites : splits)
    for (size_t width : {1, 4, 20})
      for (size_t rows : {1, 3, 8}) {
        check_scatter<uint8_t>(sites, rows, width, "uint8_t");
        check_scatter<double>(sites, rows, width, "double");
      }
  std::printf("root frame OK %ld\n", checks);
  return 0;
}
