// The host side of the select forms of the cell-proof calls (kzg_*_cells_and_proofs_select_batch), compiled for the host: the pass plan
// and the pair list (kateth_amd/csrc/cellproof_plan.hpp, the header the engine includes), and the walk of k_cell_quotients_sel beside
// the walk of k_cell_quotients (kateth_amd/csrc/cellproof_kernels.cuh): the same KZG_HD functions in the same order, the workgroup's 512
// threads walked in a loop where the kernels have a barrier.
//   cellproof_select plan <file of 16-byte masks> <P>
//       -> stdout: u64 passes, per pass u64 items and u64 vectors, u64 pairs, then the pairs as u32, pass after pass
//   cellproof_select walk <file of blobs> <pair> ...      (pair = 128 * item + cell, any order, items of the file)
//       -> stdout: per pair, in the order given, the 131,072 bytes of compact slot s (4096 evaluations, big-endian, the blob's order).
//       Every slot is compared with the vector the full kernel's walk puts at 128 * item + cell: exit status 3 on a difference.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "../../include/kateth_amd.h"
#include "../../kateth_amd/csrc/cellproof_math.cuh"
#include "../../kateth_amd/csrc/cellproof_plan.hpp"

extern "C" void kzg_fp28_check_failed(const char* what) {
  fprintf(stderr, "bound check failed: %s\n", what);
  abort();
}

constexpr size_t BLOB = 131072;
constexpr uint32_t T = kzg::CELLS_THREADS;
constexpr size_t VEC_DWORDS = 32768;

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> data;
  FILE* f = fopen(path, "rb");
  if (!f) return data;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
  fclose(f);
  return data;
}
static void put_u64(uint64_t v) { fwrite(&v, sizeof v, 1, stdout); }

static int plan_mode(const char* path, uint64_t P) {
  const std::vector<uint8_t> file = read_file(path);
  if (file.size() % kzg::cellplan::MASK_BYTES) return 2;
  const uint64_t n = file.size() / kzg::cellplan::MASK_BYTES;
  // exactly n * 16 bytes on the heap, so that the address sanitizer sees a read past the masks
  uint8_t* masks = static_cast<uint8_t*>(malloc(file.size() ? file.size() : 1));
  if (!file.empty()) memcpy(masks, file.data(), file.size());
  const std::vector<kzg::cellplan::Pass> plan = kzg::cellplan::plan(masks, n, P);
  const uint64_t total = kzg::cellplan::total_vectors(plan);
  // ... and exactly `total` entries: a write past the popcounts is seen too
  uint32_t* pairs = static_cast<uint32_t*>(malloc(total ? total * sizeof(uint32_t) : 1));
  kzg::cellplan::write_all_pairs(masks, plan, pairs);
  put_u64(plan.size());
  for (const kzg::cellplan::Pass& p : plan) {
    put_u64(p.items);
    put_u64(p.vectors);
  }
  put_u64(total);
  fwrite(pairs, sizeof(uint32_t), total, stdout);
  free(pairs);
  free(masks);
  return 0;
}

struct Tables {
  std::vector<uint32_t> tab, ztab;
  Tables() : tab((size_t)kzg::CELLS_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY), ztab((size_t)kzg::CELLPROOF_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY) {
    for (uint32_t i = 0; i < kzg::CELLS_TAB_ENTRIES; i++) kzg::cells_tab_entry(i, tab.data() + (size_t)i * kzg::CELLS_TAB_ENTRY);
    for (uint32_t i = 0; i < kzg::CELLPROOF_TAB_ENTRIES; i++) kzg::cellproof_tab_entry(i, ztab.data() + (size_t)i * kzg::CELLS_TAB_ENTRY);
  }
};
// cell_quotient_vector (cellproof_kernels.cuh), the body both kernels share
static void quotient_vector(const Tables& tb, const uint32_t* item_coeffs, uint32_t cell, uint32_t* out) {
  std::vector<uint32_t> img(kzg::CELLS_IMAGE_DWORDS), carry(kzg::CELLPROOF_CARRY_DWORDS);
  kzg::fr29 z, z8, c[8];
  kzg::cells_tw(z, tb.ztab.data(), kzg::cellproof_zpow(cell, 1));
  kzg::cells_tw(z8, tb.ztab.data(), kzg::cellproof_zpow(cell, 8));
  for (uint32_t t = 0; t < T; t++) {
    kzg::cellproof_load_segment(c, item_coeffs, t);
    kzg::cellproof_segment_total(carry.data(), c, z, t);
  }
  for (uint32_t t = 0; t < T; t++) {
    kzg::cellproof_load_segment(c, item_coeffs, t);
    kzg::cellproof_divide(img.data(), carry.data(), c, z, z8, t);
  }
  for (int p = kzg::CELLPROOF_PASSES - 1; p >= 0; p--)
    for (uint32_t t = 0; t < T; t++) kzg::cellproof_fwd_pass(img.data(), tb.tab.data(), t, p);
  for (uint32_t t = 0; t < T; t++) kzg::cellproof_store_words(out, img.data(), t);
}

static int walk_mode(const char* path, const std::vector<uint32_t>& pairs) {
  const std::vector<uint8_t> file = read_file(path);
  if (file.empty() || file.size() % BLOB) return 2;
  const uint64_t items = file.size() / BLOB;
  for (uint32_t pair : pairs)
    if (kzg::cellproof_pair_item(pair) >= items) return 2;
  const Tables tb;
  // k_cell_coeffs over every item: the coefficient buffer exactly as large as the kernel's
  uint8_t* in = static_cast<uint8_t*>(aligned_alloc(16, BLOB));
  uint32_t* coeffs = static_cast<uint32_t*>(aligned_alloc(16, items * kzg::CELLPROOF_COEFF_BYTES));
  std::vector<uint32_t> img(kzg::CELLS_IMAGE_DWORDS);
  for (uint64_t b = 0; b < items; b++) {
    memcpy(in, file.data() + b * BLOB, BLOB);
    for (uint32_t t = 0; t < T; t++)
      if (kzg::cellproof_load_blob(img.data(), in, t)) return 2;  // accepted blobs only
    for (int p = 0; p < kzg::CELLPROOF_PASSES; p++)
      for (uint32_t t = 0; t < T; t++) kzg::cellproof_inv_pass(img.data(), tb.tab.data(), t, p);
    for (uint32_t t = 0; t < T; t++) kzg::cellproof_store_words(coeffs + b * (kzg::CELLPROOF_COEFF_BYTES / 4), img.data(), t);
  }
  // k_cell_quotients: block vec = 128 item + cell writes at q[vec * 4096 ..]; only the blocks some pair names are walked and kept
  std::map<uint32_t, std::vector<uint32_t>> full;
  for (uint32_t vec : pairs) {
    if (full.count(vec)) continue;
    std::vector<uint32_t>& q = full[vec];
    q.resize(VEC_DWORDS);
    quotient_vector(tb, coeffs + (uint64_t)(vec >> 7) * (kzg::CELLPROOF_COEFF_BYTES / 4), vec & 127u, q.data());
  }
  // k_cell_quotients_sel: block s reads pairs[s] and writes at the compact slot q[s * 4096 ..]; the buffer has exactly pairs.size() slots
  uint32_t* compact = static_cast<uint32_t*>(aligned_alloc(16, pairs.size() * VEC_DWORDS * sizeof(uint32_t)));
  for (size_t s = 0; s < pairs.size(); s++) {
    const uint32_t pair = pairs[s];
    quotient_vector(tb, coeffs + (uint64_t)kzg::cellproof_pair_item(pair) * (kzg::CELLPROOF_COEFF_BYTES / 4), kzg::cellproof_pair_cell(pair),
                    compact + s * VEC_DWORDS);
  }
  int rc = 0;
  std::vector<uint8_t> out(BLOB);
  for (size_t s = 0; s < pairs.size(); s++) {
    if (memcmp(compact + s * VEC_DWORDS, full[pairs[s]].data(), VEC_DWORDS * sizeof(uint32_t)) != 0) rc = 3;
    for (uint32_t e = 0; e < 4096; e++)
      for (int q = 0; q < 8; q++) {
        const uint32_t w = compact[s * VEC_DWORDS + 8 * e + q];
        for (int b = 0; b < 4; b++) out[32 * e + 4 * (7 - q) + (3 - b)] = (uint8_t)(w >> (8 * b));
      }
    fwrite(out.data(), 1, out.size(), stdout);
  }
  free(compact);
  free(coeffs);
  free(in);
  return rc;
}

int main(int argc, char** argv) {
  if (argc >= 4 && strcmp(argv[1], "plan") == 0) return plan_mode(argv[2], strtoull(argv[3], nullptr, 10));
  if (argc >= 4 && strcmp(argv[1], "walk") == 0) {
    std::vector<uint32_t> pairs;
    for (int a = 3; a < argc; a++) pairs.push_back((uint32_t)strtoul(argv[a], nullptr, 10));
    return walk_mode(argv[2], pairs);
  }
  return 2;
}
