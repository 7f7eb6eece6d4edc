// What a traversal-kernel launch reads: the operation descriptor and the pieces of one launch.
// Plain data, no HIP: common.hpp hands it to the kernels, clv_plan.hpp fills it in on the host
// (and tests/cpp/host_logic_check.cpp checks that without a GPU).
#pragma once

#include <cstdint>

namespace rdamd {

struct LevelOp {   // device-side op descriptor
  unsigned parent_clv, child1_clv, child2_clv;     // absolute clv indices
  unsigned child1_mat, child2_mat;
  int parent_sc, child1_sc, child2_sc;
  // where each child comes from: 0 tip, 1 memory, 2 register (= parent of the
  // previous op), 3+s = LDS parking slot s (4-state kernel only)
  unsigned src1, src2;
  // 4-state kernel: park = 1+s: also park the parent in LDS slot s (0: do not); noop = padding
  // entry (lists are padded to whole chunks).  20-state kernel (which has neither): the tip
  // indices of the NEXT operation's children (0 where a child is no tip, or there is no
  // next operation) -- it fetches tip codes through the scalar cache two operations ahead,
  // and taking the address from the operation in front means no scalar load has to wait
  // for another one.
  union { unsigned park; unsigned ahead1; };
  union { unsigned noop; unsigned ahead2; };
  // 4-state kernel only: byte offsets worked out on the host, so the kernel's
  // scalar unit does no 64-bit index arithmetic.  *_off of a child: its row in
  // the tip codes (tip) or its CLV (memory); kNoOffset where there is none.
  uint64_t parent_off, parent_sc_off;
  uint64_t child1_off, child1_sc_off;
  uint64_t child2_off, child2_sc_off;
};
static_assert(sizeof(LevelOp) == 96, "LevelOp: 12 words + 6 offsets");
constexpr uint64_t kNoOffset = ~0ull;

// independent pieces of one operation list, run side by side (grid.y): [start, start + len) each
constexpr unsigned kMaxListPieces = 32;
struct ListPieces {
  unsigned n = 0;
  unsigned start[kMaxListPieces] = {0}, len[kMaxListPieces] = {0};
};

}  // namespace rdamd
