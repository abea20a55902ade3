// The host descent with a floor level (kateth_amd/csrc/each_descent.hpp), stand-alone: no HIP, no pairing -- a node passes iff no failing
// leaf lies in its range.
//   1. floor 0 against the descent as it was before the floor existed (descend_before, kept here word for word): for every failure
//      pattern at n <= 9 the same verdicts and the same sequence of check calls, node for node.
//   2. floor f in {1, 2, 7} over n that are and are not multiples of 2^f: the verdict of group g is the OR of its leaves, no node is
//      checked twice, nothing below the floor is checked, and with k failing groups among m = ceil(n / 2^f) the count stays within
//      1 + 2 k ceil(log2 m) and 2 m - 1.
// Prints "ok <patterns walked>"; any mismatch is a message on stderr and exit status 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "../../kateth_amd/csrc/each_descent.hpp"

namespace before {
using kzg::each::level_count;
using kzg::each::tree_height;
template <class Check>
int32_t descend_before(uint64_t n, uint8_t* ok_each, Check&& check) {
  for (uint64_t i = 0; i < n; i++) ok_each[i] = 1;
  if (n == 0) return 0;
  uint32_t level = tree_height(n);
  std::vector<uint64_t> failing, next, lefts, rights;
  std::vector<uint8_t> pass(1);
  {
    const uint64_t root = 0;
    const int32_t rc = check(level, &root, (size_t)1, pass.data());
    if (rc) return rc;
    if (pass[0]) return 0;
    failing.push_back(0);
  }
  for (; level > 0; level--) {
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
      if (2 * f + 1 >= cnt) {
        next.push_back(2 * f);
      } else if (pass[k++]) {
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
}  // namespace before

using Calls = std::vector<std::pair<uint32_t, uint64_t>>;  // (level, node) in the order checked

static int die(const char* what, uint64_t n, uint32_t floor, uint64_t pattern) {
  fprintf(stderr, "%s: n = %llu, floor = %u, pattern = %llx\n", what, (unsigned long long)n, floor, (unsigned long long)pattern);
  return 1;
}

// a node passes iff none of its leaves fails
struct Oracle {
  uint64_t n;
  const std::vector<uint8_t>& bad;
  Calls calls;
  int32_t operator()(uint32_t level, const uint64_t* idx, size_t m, uint8_t* pass) {
    if (m == 0) return -100;  // never called with m = 0
    for (size_t k = 0; k < m; k++) {
      if (k && idx[k] <= idx[k - 1]) return -101;  // ascending
      if (idx[k] >= kzg::each::level_count(n, level)) return -102;
      const uint64_t lo = idx[k] << level, hi = std::min<uint64_t>(n, (idx[k] + 1) << level);
      uint8_t any = 0;
      for (uint64_t i = lo; i < hi; i++) any |= bad[i];
      pass[k] = !any;
      calls.emplace_back(level, idx[k]);
    }
    return 0;
  }
};

static int walk_floor(uint64_t n, uint32_t floor, const std::vector<uint8_t>& bad, uint64_t tag) {
  using namespace kzg::each;
  const uint32_t height = tree_height(n), stop = floor > height ? height : floor;
  const uint64_t m = level_count(n, stop);
  std::vector<uint8_t> verdict(m + 1, 0x5a);  // one guard byte behind the m verdicts
  Oracle oracle{n, bad, {}};
  const int32_t rc = descend(n, verdict.data(), oracle, floor);
  if (rc) return die("check refused its arguments", n, floor, tag);
  if (verdict[m] != 0x5a) return die("wrote past the m verdicts", n, floor, tag);
  uint64_t k = 0;
  for (uint64_t g = 0; g < m; g++) {
    uint8_t any = 0;
    for (uint64_t i = g << stop; i < std::min<uint64_t>(n, (g + 1) << stop); i++) any |= bad[i];
    if (verdict[g] != (any ? 0 : 1)) return die("a group's verdict is not the OR of its leaves", n, floor, tag);
    k += any;
  }
  std::set<std::pair<uint32_t, uint64_t>> seen;
  for (const auto& c : oracle.calls) {
    if (c.first < stop) return die("a node below the floor was checked", n, floor, tag);
    if (!seen.insert(c).second) return die("a node was checked twice", n, floor, tag);
  }
  const uint64_t count = oracle.calls.size();
  if (count > 1 + 2 * k * tree_height(m)) return die("more checks than 1 + 2 k ceil(log2 m)", n, floor, tag);
  if (count > 2 * m - 1) return die("more checks than 2 m - 1", n, floor, tag);
  if (k == 0 && count != 1) return die("a passing root must be the only check", n, floor, tag);
  return 0;
}

int main() {
  using namespace kzg::each;
  uint64_t walked = 0;
  // 1. floor 0 is the descent as it was
  for (uint64_t n = 1; n <= 9; n++)
    for (uint64_t pattern = 0; pattern < ((uint64_t)1 << n); pattern++, walked++) {
      std::vector<uint8_t> bad(n);
      for (uint64_t i = 0; i < n; i++) bad[i] = (pattern >> i) & 1;
      std::vector<uint8_t> a(n, 7), b(n, 9), c(n, 11);
      Oracle oa{n, bad, {}}, ob{n, bad, {}}, oc{n, bad, {}};
      if (before::descend_before(n, a.data(), oa) || descend(n, b.data(), ob) || descend(n, c.data(), oc, 0)) return die("check refused", n, 0, pattern);
      if (a != b || a != c) return die("floor 0: verdicts differ from the descent before", n, 0, pattern);
      if (oa.calls != ob.calls || oa.calls != oc.calls) return die("floor 0: other nodes checked than before", n, 0, pattern);
      for (uint64_t i = 0; i < n; i++)
        if (a[i] != !bad[i]) return die("floor 0: wrong verdict", n, 0, pattern);
    }
  {  // n = 0 writes nothing, whatever the floor
    uint8_t guard = 0x5a;
    const std::vector<uint8_t> none;
    Oracle o{0, none, {}};
    if (descend(0, &guard, o, 7) || guard != 0x5a || !o.calls.empty()) return die("n = 0", 0, 7, 0);
  }
  // 2. floors 1 and 2: every pattern of leaves at small n, multiples of 2^f and not
  for (uint32_t floor : {1u, 2u})
    for (uint64_t n : {1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13})
      for (uint64_t pattern = 0; pattern < ((uint64_t)1 << n); pattern++, walked++) {
        std::vector<uint8_t> bad(n);
        for (uint64_t i = 0; i < n; i++) bad[i] = (pattern >> i) & 1;
        if (walk_floor(n, floor, bad, pattern)) return 1;
      }
  // floor 7 (node (7, b) = blob b's 128 cells): every set of failing groups, the failing leaf at the group's first, last or both ends
  for (uint64_t n : {1, 100, 128, 129, 256, 300, 384, 385, 512, 640, 1000, 1024})
    for (uint32_t floor : {7u}) {
      const uint64_t m = level_count(n, floor > tree_height(n) ? tree_height(n) : floor), groups = floor > tree_height(n) ? 1 : m;
      for (uint64_t pattern = 0; pattern < ((uint64_t)1 << groups); pattern++)
        for (int where = 0; where < 3; where++, walked++) {
          std::vector<uint8_t> bad(n, 0);
          for (uint64_t g = 0; g < groups; g++) {
            if (!((pattern >> g) & 1)) continue;
            const uint64_t lo = floor > tree_height(n) ? 0 : g << floor, hi = floor > tree_height(n) ? n : std::min<uint64_t>(n, (g + 1) << floor);
            if (where != 1) bad[lo] = 1;
            if (where != 0) bad[hi - 1] = 1;
          }
          if (walk_floor(n, floor, bad, pattern * 4 + where)) return 1;
        }
    }
  printf("ok %llu\n", (unsigned long long)walked);
  return 0;
}
