// The address map of the data column calls (cells_column_major, kateth_amd/csrc/cells_math.cuh) under every phase of the k_columns_*
// kernels that moves cells, compiled for the host and walked thread by thread: k_columns_compute's store_half and zero-fill,
// k_columns_coeffs' load (cellproof_load_blob), and ALL of k_columns_recover -- recover_load_half, the stash of steps 3 and 7
// (recover_step), recover_store_half -- run once on a blob-major item and once on row `row` of column matrices of n rows, for
// n in {1, 3} and row in {0, n - 1}.  Checked:
//   - the column-major result is T of the blob-major one (T written out here, independently of the map);
//   - every byte of the output matrix outside the row's own cells keeps its sentinel, and nothing outside the matrices is touched
//     (buffers exactly as large as the kernels', on the heap: the address sanitizer sees every index);
//   - no two threads own the same stash bytes, and every stash piece lies in cells 0..63 of the row;
//   - in every phase the 64 lanes of a wave are inside one cell -- what lets the device take the cell by readfirstlane.
// The data is arbitrary canonical field elements: the walk's arithmetic does not care whether they lie on a polynomial (the consistency
// verdict is compared too).  No input; exit status 0 and one line on stdout, or a message on stderr and exit status 1.
#define KZG_FP28_CHECK 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/kateth_amd.h"
#include "../../kateth_amd/csrc/cellproof_math.cuh"

extern "C" void kzg_fp28_check_failed(const char* what) {
  fprintf(stderr, "bound check failed: %s\n", what);
  abort();
}

constexpr size_t ITEM = 262144, CELL = 2048;
constexpr uint32_t T = kzg::CELLS_THREADS;
constexpr uint8_t SENTINEL = 0xA5, POISON = 0xFF;  // POISON is no canonical element: a present-looking read of it is caught

static int failures = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      fprintf(stderr, __VA_ARGS__);   \
      fprintf(stderr, "\n");          \
      failures++;                     \
    }                                 \
  } while (0)

static uint64_t lcg = 0x7594;
static uint8_t next_byte() {
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint8_t)(lcg >> 56);
}

// T, independent of the map: cell c of the item <-> the cell of (column c, row) of a matrix of n rows
static void item_to_matrix(uint8_t* matrix, const uint8_t* item, uint64_t n, uint64_t row) {
  for (size_t c = 0; c < 128; c++) memcpy(matrix + (c * n + row) * CELL, item + c * CELL, CELL);
}
static bool row_equals_item(const uint8_t* matrix, const uint8_t* item, uint64_t n, uint64_t row, size_t cells) {
  for (size_t c = 0; c < cells; c++)
    if (memcmp(matrix + (c * n + row) * CELL, item + c * CELL, CELL)) return false;
  return true;
}
static bool others_keep(const uint8_t* matrix, uint64_t n, uint64_t row, uint8_t fill) {
  for (size_t c = 0; c < 128; c++)
    for (uint64_t b = 0; b < n; b++)
      if (b != row)
        for (size_t k = 0; k < CELL; k++)
          if (matrix[(c * n + b) * CELL + k] != fill) return false;
  return true;
}

struct Tables {
  std::vector<uint32_t> tab, rtab;
  Tables() : tab((size_t)kzg::CELLS_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY), rtab((size_t)kzg::RECOVER_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY) {
    for (uint32_t i = 0; i < kzg::CELLS_TAB_ENTRIES; i++) kzg::cells_tab_entry(i, tab.data() + (size_t)i * kzg::CELLS_TAB_ENTRY);
    for (uint32_t i = 0; i < kzg::RECOVER_TAB_ENTRIES; i++) kzg::recover_tab_entry(i, rtab.data() + (size_t)i * kzg::CELLS_TAB_ENTRY);
  }
};

// k_recover_cells / k_columns_recover up to the verdict (the zero-fill of a rejected item is walked apart): `in`, `out` and `map` as the kernel has them
template <class Map>
static int32_t recover_walk(const Tables& tb, const uint8_t* in, uint8_t* out, const uint32_t* mask, const Map map) {
  std::vector<uint32_t> img(kzg::CELLS_IMAGE_DWORDS), zs(kzg::RECOVER_ZS_DWORDS);
  int32_t bad = 0;
  for (uint32_t t = 0; t < T; t++) kzg::recover_prep_partial(img.data(), tb.rtab.data(), mask, t);
  for (uint32_t t = 0; t < T; t++) kzg::recover_prep_combine(zs.data(), img.data(), t);
  for (int k = 0; k < kzg::RECOVER_STEPS; k++) {
    if (k == 0 || k == 4) {
      for (uint32_t t = 0; t < T; t++)
        if (kzg::recover_load_half(img.data(), zs.data(), in, mask, t, (uint32_t)k >> 2, map)) bad = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
      if (bad) return bad;
    }
    for (uint32_t t = 0; t < T; t++) kzg::recover_step(img.data(), zs.data(), reinterpret_cast<uint32_t*>(out), tb.tab.data(), tb.rtab.data(), t, k, map);
  }
  for (uint32_t half = 0; half < 2; half++) {
    if (half)
      for (int k = 0; k < kzg::CELLS_STEPS; k++)
        for (uint32_t t = 0; t < T; t++) kzg::cells_step(img.data(), tb.tab.data(), t, k);
    for (uint32_t t = 0; t < T; t++)
      if (kzg::recover_store_half(img.data(), in, out, mask, t, half, map)) bad = KZG_ERR_CELLS_INCONSISTENT;
  }
  return bad;
}

// the offsets `at` (inside the item's 262,144 bytes) that lane t touches in round i of a phase, as the kernels form them
static size_t at_half(uint32_t half, uint32_t i, uint32_t t) { return ((size_t)half * 4096u + i * T + t) * 32u; }  // load_half, store_half, cellproof_load_blob (half 0)
static size_t at_stash(uint32_t i, uint32_t t) { return (size_t)(t + 512u * i) * 32u; }                              // steps 3 and 7: e = t + 512 i
static size_t at_quad(uint32_t q) { return (size_t)q * 16u; }                                                        // k_columns_compute: out(q)

static void one_case(const Tables& tb, uint64_t n, uint64_t row) {
  const size_t MATRIX = (size_t)n * ITEM;
  uint8_t* item = static_cast<uint8_t*>(aligned_alloc(16, ITEM));
  uint8_t* out_bm = static_cast<uint8_t*>(aligned_alloc(16, ITEM));
  uint8_t* in_cm = static_cast<uint8_t*>(aligned_alloc(16, MATRIX));
  uint8_t* out_cm = static_cast<uint8_t*>(aligned_alloc(16, MATRIX));
  const kzg::cells_column_major map{n, row};

  // ---- the map itself against the issue's formula, and the lanes of a wave inside one cell in every phase
  for (size_t at = 0; at < ITEM; at += 16) {
    const size_t want = ((at >> 11) * n + row) * 2048 + (at & 2047);
    CHECK(map(at) == want && map(at + 15) == want + 15, "map(%zu) at n=%llu row=%llu", at, (unsigned long long)n, (unsigned long long)row);
  }
  for (uint32_t w = 0; w < T / 64; w++)
    for (uint32_t lane = 1; lane < 64; lane++) {
      const uint32_t t0 = 64 * w, t = t0 + lane;
      for (uint32_t i = 0; i < 8; i++) {
        CHECK(at_half(0, i, t) >> 11 == at_half(0, i, t0) >> 11 && at_half(1, i, t) >> 11 == at_half(1, i, t0) >> 11, "halves: wave %u round %u leaves its cell", w, i);
        CHECK(at_stash(i, t) >> 11 == at_stash(i, t0) >> 11, "stash: wave %u round %u leaves its cell", w, i);
        for (uint32_t first : {0u, 8192u}) {
          const uint32_t q = first + 2 * (i * T + t), q0 = first + 2 * (i * T + t0);
          CHECK(at_quad(q) >> 11 == at_quad(q0) >> 11 && at_quad(q + 1) >> 11 == at_quad(q0) >> 11, "store_half: wave %u round %u leaves its cell", w, i);
        }
      }
      for (uint32_t i = 0; i < 32; i++) CHECK(at_quad(i * T + t) >> 11 == at_quad(i * T + t0) >> 11, "zero-fill: wave %u round %u leaves its cell", w, i);
    }

  // ---- k_columns_compute: store_half (both halves) and the zero-fill, a recognisable 16 bytes per quad
  auto quad_value = [](uint32_t q, uint8_t* v) {
    for (int k = 0; k < 16; k++) v[k] = (uint8_t)((q * 2654435761u) >> (8 * (k & 3))) ^ (uint8_t)k;
  };
  memset(out_bm, SENTINEL, ITEM);
  memset(out_cm, SENTINEL, MATRIX);
  for (uint32_t first : {0u, 8192u})
    for (uint32_t t = 0; t < T; t++)
      for (uint32_t i = 0; i < 8; i++) {
        const uint32_t e = i * T + t;
        for (uint32_t q : {first + 2 * e, first + 2 * e + 1}) {
          uint8_t v[16];
          quad_value(q, v);
          memcpy(out_bm + kzg::cells_blob_major{}(at_quad(q)), v, 16);
          memcpy(out_cm + map(at_quad(q)), v, 16);
        }
      }
  CHECK(row_equals_item(out_cm, out_bm, n, row, 128), "store_half: the row is not T of the blob-major cell set");
  CHECK(others_keep(out_cm, n, row, SENTINEL), "store_half: a byte outside the row's cells was written");
  memset(out_bm, SENTINEL, ITEM);
  memset(out_cm, SENTINEL, MATRIX);
  for (uint32_t t = 0; t < T; t++)
    for (uint32_t i = 0; i < 32; i++) {
      memset(out_bm + at_quad(i * T + t), 0, 16);
      memset(out_cm + map(at_quad(i * T + t)), 0, 16);
    }
  CHECK(row_equals_item(out_cm, out_bm, n, row, 128), "zero-fill: the row is not T of the blob-major cell set");
  CHECK(others_keep(out_cm, n, row, SENTINEL), "zero-fill: a byte outside the row's cells was written");

  // ---- an item of canonical elements; 64 cells present, the others POISON in both layouts, like the other rows of the input matrix
  uint32_t mask[4] = {0, 0, 0, 0};
  for (uint32_t c = 0, have = 0; c < 128 && have < 64; c++)
    if ((next_byte() & 1) || 128 - c <= 64 - have) mask[c >> 5] |= 1u << (c & 31), have++;
  for (size_t k = 0; k < ITEM; k++) item[k] = (k & 31) ? next_byte() : (uint8_t)(next_byte() & 0x3f);
  std::vector<uint8_t> first_half(item, item + ITEM / 2);  // cells 0..63 whole, for the coefficient load
  for (uint32_t c = 0; c < 128; c++)
    if (!kzg::recover_present(mask, c)) memset(item + c * CELL, POISON, CELL);
  memset(in_cm, POISON, MATRIX);
  item_to_matrix(in_cm, item, n, row);

  // ---- k_columns_recover, whole
  memset(out_bm, SENTINEL, ITEM);
  memset(out_cm, SENTINEL, MATRIX);
  const int32_t code_bm = recover_walk(tb, item, out_bm, mask, kzg::cells_blob_major{});
  const int32_t code_cm = recover_walk(tb, in_cm, out_cm, mask, map);
  CHECK(code_bm == code_cm, "recover: verdict %d blob-major, %d column-major", code_bm, code_cm);
  CHECK(code_bm == 0 || code_bm == KZG_ERR_CELLS_INCONSISTENT, "recover: the walk stopped early (%d): the phases behind the loads were not walked", code_bm);
  CHECK(row_equals_item(out_cm, out_bm, n, row, 128), "recover: the row is not T of the blob-major result");
  CHECK(others_keep(out_cm, n, row, SENTINEL), "recover: a byte outside the row's cells was written");
  for (uint32_t c = 0; c < 128; c++)
    if (kzg::recover_present(mask, c) && code_bm == 0) CHECK(!memcmp(out_bm + c * CELL, item + c * CELL, CELL), "recover: present cell %u changed", c);

  // ---- the stash alone: who owns which bytes of the output matrix
  {
    std::vector<int32_t> owner(MATRIX, -1);
    uint32_t* base = reinterpret_cast<uint32_t*>(out_cm);
    for (uint32_t t = 0; t < T; t++)
      for (uint32_t i = 0; i < 8; i++) {
        const uint32_t e = t + 512u * i;
        const size_t off = (size_t)(reinterpret_cast<uint8_t*>(kzg::recover_stash_piece(base, e, map)) - out_cm);
        CHECK(off == ((size_t)(e >> 6) * n + row) * 2048 + (size_t)(e & 63u) * 32, "stash: piece %u is at %zu", e, off);
        CHECK(off + 32 <= MATRIX && (off >> 11) / n < 64 && (off >> 11) % n == row, "stash: piece %u leaves cells 0..63 of the row", e);
        for (size_t k = off; k < off + 32 && k < MATRIX; k++) {
          CHECK(owner[k] < 0, "stash: byte %zu belongs to threads %d and %u", k, owner[k], t);
          owner[k] = (int32_t)t;
        }
      }
    size_t owned = 0;
    for (int32_t o : owner) owned += o >= 0;
    CHECK(owned == ITEM / 2, "stash: %zu bytes owned, not 131,072", owned);
  }

  // ---- k_columns_coeffs' load: cells 0..63 of the row against the same 131,072 bytes blob-major
  {
    memset(in_cm, POISON, MATRIX);
    for (size_t c = 0; c < 64; c++) memcpy(in_cm + (c * n + row) * CELL, first_half.data() + c * CELL, CELL);
    std::vector<uint32_t> img_bm(kzg::CELLS_IMAGE_DWORDS, 0), img_cm(kzg::CELLS_IMAGE_DWORDS, 1);
    bool bad_bm = false, bad_cm = false;
    for (uint32_t t = 0; t < T; t++) {
      bad_bm |= kzg::cellproof_load_blob(img_bm.data(), first_half.data(), t);
      bad_cm |= kzg::cellproof_load_blob(img_cm.data(), in_cm, t, map);
    }
    CHECK(!bad_bm && !bad_cm, "coefficient load: an element was taken for non-canonical");
    CHECK(img_bm == img_cm, "coefficient load: the images differ");
  }
  free(item);
  free(out_bm);
  free(in_cm);
  free(out_cm);
}

int main() {
  const Tables tb;
  int cases = 0;
  const uint64_t shapes[][2] = {{1, 0}, {3, 0}, {3, 2}};  // (n, row): rows 0 and n - 1 of n = 1 and n = 3
  for (const auto& s : shapes) {
    one_case(tb, s[0], s[1]);
    cases++;
  }
  // proofs: 48 bytes at 48 (c n + b), every position of a 128 x n matrix exactly once
  for (uint64_t n : {1ull, 3ull}) {
    std::vector<int> hit(128 * n, 0);
    for (uint32_t c = 0; c < 128; c++)
      for (uint64_t b = 0; b < n; b++) {
        const size_t at = kzg::proofs_column_at(n, b, c);
        CHECK(at % 48 == 0 && at / 48 == c * n + b, "proofs_column_at(%llu, %llu, %u) = %zu", (unsigned long long)n, (unsigned long long)b, c, at);
        if (at / 48 < hit.size()) hit[at / 48]++;
      }
    for (int h : hit) CHECK(h == 1, "proofs: a position is hit %d times", h);
  }
  if (failures) return 1;
  printf("datacolumns_addr: %d cases ok\n", cases);
  return 0;
}
