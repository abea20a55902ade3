// Test driver of kateth_amd/csrc/each_descent.hpp: the descent over a tree whose `check` is answered from a bitmap of bad leaves
// (a node passes iff no leaf of its range is bad -- what the pairing check of a node's two sums says, up to its soundness error).
// Every node handed to `check` is recorded, in order, so that the test can count them and look at which were asked.
#include <cstdint>
#include <vector>

#include "../../kateth_amd/csrc/each_descent.hpp"

extern "C" {
// bad: n bytes (non-zero = a bad leaf).  ok_each: n bytes out.  checked_level / checked_index: room for `cap` records.
// Returns the number of nodes checked (records beyond `cap` are counted, not stored), or -1 if descend returned an error.
int64_t each_descent_run(uint64_t n, const uint8_t* bad, uint8_t* ok_each, uint32_t* checked_level, uint64_t* checked_index, uint64_t cap) {
  std::vector<uint64_t> prefix(n + 1, 0);  // bad leaves before position i
  for (uint64_t i = 0; i < n; i++) prefix[i + 1] = prefix[i] + (bad[i] ? 1 : 0);
  uint64_t count = 0;
  const int32_t rc = kzg::each::descend(n, ok_each, [&](uint32_t level, const uint64_t* idx, size_t m, uint8_t* pass) -> int32_t {
    for (size_t k = 0; k < m; k++) {
      const uint64_t lo = idx[k] << level;
      uint64_t hi = (idx[k] + 1) << level;
      if (hi > n) hi = n;
      if (lo >= n) return 1;  // a node that does not exist
      pass[k] = prefix[hi] == prefix[lo] ? 1 : 0;
      if (count < cap) {
        checked_level[count] = level;
        checked_index[count] = idx[k];
      }
      count++;
    }
    return 0;
  });
  return rc ? -1 : (int64_t)count;
}
uint32_t each_descent_height(uint64_t n) { return kzg::each::tree_height(n); }
uint64_t each_descent_level_count(uint64_t n, uint32_t level) { return kzg::each::level_count(n, level); }
}
