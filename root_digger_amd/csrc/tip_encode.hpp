// rdamd_set_tip_states' host half: one sequence checked and encoded against a COPY of the partition's
// code table, so that a refused sequence leaves nothing behind.  Host-only (no HIP): the sanitizer
// program tests/cpp/host_sanitize.cpp drives it as well.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rdamd {

struct TipEncoding {
  std::vector<uint8_t> row;         // [sites]: the state mask itself (4 states) or the mask's code
  std::vector<uint64_t> codemask;   // the table with this sequence's new masks appended
  unsigned ncodes = 0;
  bool new_code = false;
  int error = 0;                    // 0, 4 (a character without a valid state) or 5 (the table is full)
  size_t site = 0;                  // where `error` was met
};

// states: what the caller created the partition with (masks may use that many bits); direct: the
// row holds the masks themselves (4-state kernels), no table.  Sites are taken in order and the
// first refusal ends the walk, error 4 before error 5 at the same site.
inline TipEncoding encode_tip_row(const uint64_t *map, const char *sequence, size_t sites, unsigned states, bool direct,
                                  const std::vector<uint64_t> &codemask, unsigned ncodes, unsigned ncodes_cap) {
  TipEncoding t;
  t.row.resize(sites);
  t.codemask = codemask;
  t.ncodes = ncodes;
  const uint64_t full = states == 64 ? ~0ull : ((1ull << states) - 1);
  for (size_t s = 0; s < sites; ++s) {
    const uint64_t st = map[(unsigned char)sequence[s]];
    t.site = s;
    if (!st || (st & ~full)) {
      t.error = 4;
      return t;
    }
    if (direct) {
      t.row[s] = (uint8_t)st;
      continue;
    }
    unsigned c = 0;
    for (; c < t.ncodes; ++c)
      if (t.codemask[c] == st) break;
    if (c == t.ncodes) {
      if (t.ncodes >= ncodes_cap) {
        t.error = 5;
        return t;
      }
      t.codemask[t.ncodes++] = st;
      t.new_code = true;
    }
    t.row[s] = (uint8_t)c;
  }
  return t;
}

}  // namespace rdamd
