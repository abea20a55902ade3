// The host descent of kzg_verify_*_batch_each: which leaves of a sum tree fail, given only a test of whole nodes.
//
// The tree is over n leaves, level 0 = the leaves, level l has ceil(n / 2^l) nodes, node (l, j) covers the leaves
// [j 2^l, min(n, (j + 1) 2^l)) and is the sum of its children (l - 1, 2 j) and (l - 1, 2 j + 1); a missing right child is the
// identity, so such a node EQUALS its left child.  `check` answers for a list of nodes of one level whether each passes (in the
// engine: e(-A, [tau]_2) e(B, G2) == 1 for the node's two sums -- no pairing and no HIP in here).  A node that passes clears its
// whole range.  Of a failing node the LEFT child is checked; if it passes the right child fails without a check (the parent's
// pairing value is the product of the children's), otherwise the right child is checked too.  Breadth-first: the left children
// of all failing nodes of a level go to `check` in one call, then the right children that still need one.
// With k failing leaves among n: at most 1 + 2 k ceil(log2 n) nodes are checked, never more than 2 n - 1 (no node twice).
//
// FLOOR (default 0 = the above): the descent stops at level `floor`, whose m = ceil(n / 2^floor) nodes are the GROUPS the caller wants
// a verdict for (the blob form of cell verification: floor 7, node (7, b) = blob b's 128 cells); ok_each then has m entries and
// ok_each[g] = 0 iff group g holds a failing leaf.  Nothing below the floor is ever checked: with k failing groups at most
// 1 + 2 k (height(n) - floor) nodes, height(n) - floor = ceil(log2 m) -- the bound above for m leaves -- and never more than 2 m - 1.
// A floor above the root's level asks for the one group that is the whole tree: the root's check settles it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kzg {
namespace each {

inline uint32_t tree_height(uint64_t n) {  // ceil(log2 n): the root's level
  uint32_t h = 0;
  while (((uint64_t)1 << h) < n) h++;
  return h;
}
inline uint64_t level_count(uint64_t n, uint32_t level) { return (n + ((uint64_t)1 << level) - 1) >> level; }

// check(level, idx, m, pass) -> 0 or an error code: pass[k] = 1 iff node (level, idx[k]) passes; idx ascending; never called with m = 0.
// ok_each[i] = 1 for a leaf that passes, 0 for one that fails.  Returns the first non-zero code of `check`.
template <class Check>
int32_t descend(uint64_t n, uint8_t* ok_each, Check&& check, uint32_t floor = 0) {
  if (n == 0) return 0;
  uint32_t level = tree_height(n);
  if (floor > level) floor = level;
  for (uint64_t i = 0, m = level_count(n, floor); i < m; i++) ok_each[i] = 1;
  std::vector<uint64_t> failing, next, lefts, rights;
  std::vector<uint8_t> pass(1);
  {
    const uint64_t root = 0;
    const int32_t rc = check(level, &root, (size_t)1, pass.data());
    if (rc) return rc;
    if (pass[0]) return 0;
    failing.push_back(0);
  }
  for (; level > floor; level--) {
    const uint32_t child = level - 1;
    const uint64_t cnt = level_count(n, child);
    next.clear();
    lefts.clear();
    rights.clear();
    for (uint64_t f : failing)
      if (2 * f + 1 < cnt) lefts.push_back(2 * f);
    if (!lefts.empty()) {
      pass.assign(lefts.size(), 0);
      const int32_t rc = check(child, lefts.data(), lefts.size(), pass.data());
      if (rc) return rc;
    }
    size_t k = 0;
    for (uint64_t f : failing) {
      if (2 * f + 1 >= cnt) {  // an only child is its parent
        next.push_back(2 * f);
      } else if (pass[k++]) {  // the failure is on the right
        next.push_back(2 * f + 1);
      } else {
        next.push_back(2 * f);
        rights.push_back(2 * f + 1);
      }
    }
    if (!rights.empty()) {
      pass.assign(rights.size(), 0);
      const int32_t rc = check(child, rights.data(), rights.size(), pass.data());
      if (rc) return rc;
      // merge the failing right children in, keeping `next` ascending
      std::vector<uint64_t> merged;
      merged.reserve(next.size() + rights.size());
      size_t r = 0;
      for (uint64_t v : next) {
        merged.push_back(v);
        if (r < rights.size() && rights[r] == v + 1 && !(v & 1)) {
          if (!pass[r]) merged.push_back(v + 1);
          r++;
        }
      }
      next.swap(merged);
    }
    failing.swap(next);
  }
  for (uint64_t f : failing) ok_each[f] = 0;
  return 0;
}

}  // namespace each
}  // namespace kzg
