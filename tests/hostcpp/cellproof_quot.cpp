// The quotient vectors of the cell proofs as k_cell_coeffs and k_cell_quotients run them (kateth_amd/csrc/cellproof_kernels.cuh),
// compiled for the host: the same KZG_HD functions in the same order (cellproof_math.cuh), the workgroup's 512 threads walked in a
// loop where the kernels have a barrier, the tables built by the entry functions the setup kernels call.  With KZG_FP28_CHECK every
// limb operation is re-checked.
//   cellproof_quot <file of blobs> <cell> ...  ->  stdout, per blob: int32 status, then for an accepted blob per cell 131,072 bytes
//   (the 4096 evaluations of q_cell, big-endian, the blob's order) + 2,048 bytes (the 64 remainders c[rho, 0] + z q[rho, 0])
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

constexpr size_t BLOB = 131072;
constexpr uint32_t T = kzg::CELLS_THREADS;

static void put_be(uint8_t* p, const kzg::fr_t& v) {
  for (int q = 0; q < 8; q++)
    for (int b = 0; b < 4; b++) p[4 * (7 - q) + (3 - b)] = (uint8_t)(v.v[q] >> (8 * b));
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> cells;
  for (int a = 2; a < argc; a++) cells.push_back((uint32_t)atoi(argv[a]));
  std::vector<uint32_t> tab((size_t)kzg::CELLS_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY), ztab((size_t)kzg::CELLPROOF_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY);
  for (uint32_t i = 0; i < kzg::CELLS_TAB_ENTRIES; i++) kzg::cells_tab_entry(i, tab.data() + (size_t)i * kzg::CELLS_TAB_ENTRY);
  for (uint32_t i = 0; i < kzg::CELLPROOF_TAB_ENTRIES; i++) kzg::cellproof_tab_entry(i, ztab.data() + (size_t)i * kzg::CELLS_TAB_ENTRY);
  // exactly as large as the kernels' buffers, on the heap, so that the address sanitizer sees every index
  uint8_t* in = static_cast<uint8_t*>(aligned_alloc(16, BLOB));
  uint32_t* coeffs = static_cast<uint32_t*>(aligned_alloc(16, kzg::CELLPROOF_COEFF_BYTES));
  uint32_t* evals = static_cast<uint32_t*>(aligned_alloc(16, BLOB));
  std::vector<uint32_t> img(kzg::CELLS_IMAGE_DWORDS), carry(kzg::CELLPROOF_CARRY_DWORDS);
  std::vector<uint8_t> out(BLOB + 2048);
  while (fread(in, 1, BLOB, f) == BLOB) {
    // k_cell_coeffs
    int32_t bad = 0;
    for (uint32_t t = 0; t < T; t++)
      if (kzg::cellproof_load_blob(img.data(), in, t)) bad = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
    fwrite(&bad, sizeof bad, 1, stdout);
    if (bad) continue;
    for (int p = 0; p < kzg::CELLPROOF_PASSES; p++)
      for (uint32_t t = 0; t < T; t++) kzg::cellproof_inv_pass(img.data(), tab.data(), t, p);
    for (uint32_t t = 0; t < T; t++) kzg::cellproof_store_words(coeffs, img.data(), t);
    // k_cell_quotients
    for (uint32_t cell : cells) {
      kzg::fr29 z, z8, c[8];
      kzg::cells_tw(z, ztab.data(), kzg::cellproof_zpow(cell, 1));
      kzg::cells_tw(z8, ztab.data(), kzg::cellproof_zpow(cell, 8));
      for (uint32_t t = 0; t < T; t++) {
        kzg::cellproof_load_segment(c, coeffs, t);
        kzg::cellproof_segment_total(carry.data(), c, z, t);
      }
      for (uint32_t t = 0; t < T; t++) {
        kzg::cellproof_load_segment(c, coeffs, t);
        kzg::cellproof_divide(img.data(), carry.data(), c, z, z8, t);
      }
      // the remainder, from the quotient's coefficients as the division left them
      for (uint32_t rho = 0; rho < 64; rho++) {
        kzg::fr_t v;
        kzg::fr29 q;
        kzg::cellproof_load_segment(c, coeffs, rho);  // thread rho: segment 0, c[0] = coefficient rho
        kzg::cells_get(v, img.data(), rho);
        kzg::f29_from_bn(q, v);
        kzg::cellproof_chain(q, c[0], z);
        kzg::cells_reduce(q);
        kzg::f29_to_canonical_bn(v, q);
        put_be(out.data() + BLOB + 32 * rho, v);
      }
      for (int p = kzg::CELLPROOF_PASSES - 1; p >= 0; p--)
        for (uint32_t t = 0; t < T; t++) kzg::cellproof_fwd_pass(img.data(), tab.data(), t, p);
      for (uint32_t t = 0; t < T; t++) kzg::cellproof_store_words(evals, img.data(), t);
      for (uint32_t e = 0; e < 4096; e++) {
        kzg::fr_t v;
        for (int q = 0; q < 8; q++) v.v[q] = evals[8 * e + q];
        put_be(out.data() + 32 * e, v);
      }
      fwrite(out.data(), 1, out.size(), stdout);
    }
  }
  fclose(f);
  free(in);
  free(coeffs);
  free(evals);
  return 0;
}
