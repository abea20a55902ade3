// The select forms of the cell-proof calls (kzg_*_cells_and_proofs_select_batch): what the host derives from the `want` masks before anything
// is launched -- the pair list the selected quotient kernel walks and the pass plan of the call.  Plain host logic, no HIP, like
// multi_split.hpp and each_descent.hpp: tests/hostcpp/cellproof_select.cpp checks it against a Python model without a GPU.
#pragma once
#include <stdint.h>

#include <vector>

namespace kzg {
namespace cellplan {

constexpr uint32_t CELLS = 128;      // cells, and so proofs, per item
constexpr uint32_t MASK_BYTES = 16;  // per item: cell c is bit (c & 7), least significant first, of byte (c >> 3), as in `present`
constexpr uint64_t MAX_ITEMS = 128;  // items per pass at most, as in the full calls (cellproof_pass)

inline bool wanted(const uint8_t* mask, uint32_t cell) { return (mask[cell >> 3] >> (cell & 7u)) & 1u; }
inline uint32_t popcount(const uint8_t* mask) {
  uint32_t v = 0;
  for (uint32_t c = 0; c < CELLS; c++) v += wanted(mask, c) ? 1u : 0u;
  return v;
}

// a pass of the call: `items` consecutive items and the `vectors` proofs wanted of them
struct Pass {
  uint64_t items, vectors;
};
// Consecutive items share a pass while its wanted vectors stay <= 128 P and its items <= 128.  An item is never split (its at most 128
// vectors always fit, P >= 1) and a pass holds at least one item.  All-ones masks: passes of P items and a shorter last one, the full
// call's even_plan(n, P).
inline std::vector<Pass> plan(const uint8_t* want, uint64_t n, uint64_t P) {
  if (P < 1) P = 1;
  if (P > MAX_ITEMS) P = MAX_ITEMS;
  const uint64_t cap = CELLS * P;
  std::vector<Pass> out;
  Pass cur{0, 0};
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t v = popcount(want + i * MASK_BYTES);
    if (cur.items && (cur.vectors + v > cap || cur.items == MAX_ITEMS)) {
      out.push_back(cur);
      cur = Pass{0, 0};
    }
    cur.items++;
    cur.vectors += v;
  }
  if (cur.items) out.push_back(cur);
  return out;
}

// The pairs of `items` consecutive items, written from `out` on: 128 * local_item + cell, in item order and within an item in cell order.
// local_item counts from the first item given: a pass's list is the list of its own items.  Returns the end of what was written; the
// caller's buffer holds the items' popcounts.
inline uint32_t* write_pairs(const uint8_t* want, uint64_t items, uint32_t* out) {
  for (uint64_t i = 0; i < items; i++)
    for (uint32_t c = 0; c < CELLS; c++)
      if (wanted(want + i * MASK_BYTES, c)) *out++ = (uint32_t)(CELLS * i) + c;
  return out;
}
inline uint64_t total_vectors(const std::vector<Pass>& passes) {
  uint64_t v = 0;
  for (const Pass& p : passes) v += p.vectors;
  return v;
}
// the pair lists of all passes, one behind the other (pass k's list starts at the sum of the vectors of the passes before it), into a
// buffer of total_vectors(passes) entries
inline void write_all_pairs(const uint8_t* want, const std::vector<Pass>& passes, uint32_t* out) {
  uint64_t base = 0;
  for (const Pass& p : passes) {
    out = write_pairs(want + base * MASK_BYTES, p.items, out);
    base += p.items;
  }
}

}  // namespace cellplan
}  // namespace kzg
