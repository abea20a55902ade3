// Cell recovery as k_recover_cells runs it (kateth_amd/csrc/cells_kernels.cuh), compiled for the host: the same KZG_HD functions in the
// same order (recover_math.cuh, then the seven steps of cells_math.cuh), the workgroup's 512 threads walked in a loop where the kernel
// has a barrier, both tables built by the entry functions the setup kernels call.  Every limb operation is re-checked (KZG_FP28_CHECK).
//   recover_ntt <file of items: 262,144 bytes of cells + 16 bytes of mask>  ->  stdout, per item: int32 status + 262,144 bytes
#define KZG_FP28_CHECK 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/kateth_amd.h"
#include "../../kateth_amd/csrc/recover_math.cuh"

extern "C" void kzg_fp28_check_failed(const char* what) {
  fprintf(stderr, "bound check failed: %s\n", what);
  abort();
}

constexpr size_t ITEM = 262144;
constexpr uint32_t T = kzg::CELLS_THREADS;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> tab((size_t)kzg::CELLS_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY), rtab((size_t)kzg::RECOVER_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY);
  for (uint32_t i = 0; i < kzg::CELLS_TAB_ENTRIES; i++) kzg::cells_tab_entry(i, tab.data() + (size_t)i * kzg::CELLS_TAB_ENTRY);
  for (uint32_t i = 0; i < kzg::RECOVER_TAB_ENTRIES; i++) kzg::recover_tab_entry(i, rtab.data() + (size_t)i * kzg::CELLS_TAB_ENTRY);
  // exactly as large as the kernel's buffers, on the heap, so that the address sanitizer sees every index
  uint8_t* in = static_cast<uint8_t*>(aligned_alloc(16, ITEM));
  uint8_t* out = static_cast<uint8_t*>(aligned_alloc(16, ITEM));
  std::vector<uint32_t> img(kzg::CELLS_IMAGE_DWORDS), zs(kzg::RECOVER_ZS_DWORDS);
  uint32_t mask[4];
  uint8_t mask_bytes[16];
  while (fread(in, 1, ITEM, f) == ITEM && fread(mask_bytes, 1, 16, f) == 16) {
    for (int q = 0; q < 4; q++) mask[q] = (uint32_t)mask_bytes[4 * q] | (uint32_t)mask_bytes[4 * q + 1] << 8 | (uint32_t)mask_bytes[4 * q + 2] << 16 | (uint32_t)mask_bytes[4 * q + 3] << 24;
    memset(out, 0xA5, ITEM);
    int32_t bad = 0;
    if (kzg::recover_count(mask) < kzg::RECOVER_MIN_CELLS) {
      bad = KZG_ERR_CELLS_NOT_ENOUGH;
    } else {
      for (uint32_t t = 0; t < T; t++) kzg::recover_prep_partial(img.data(), rtab.data(), mask, t);
      for (uint32_t t = 0; t < T; t++) kzg::recover_prep_combine(zs.data(), img.data(), t);
      for (int k = 0; k < kzg::RECOVER_STEPS; k++) {
        if (k == 0 || k == 4) {
          for (uint32_t t = 0; t < T; t++)
            if (kzg::recover_load_half(img.data(), zs.data(), in, mask, t, (uint32_t)k >> 2)) bad = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
          if (bad) break;
        }
        for (uint32_t t = 0; t < T; t++) kzg::recover_step(img.data(), zs.data(), reinterpret_cast<uint32_t*>(out), tab.data(), rtab.data(), t, k);
      }
      if (bad == 0) {
        for (uint32_t half = 0; half < 2; half++) {
          if (half)
            for (int k = 0; k < kzg::CELLS_STEPS; k++)
              for (uint32_t t = 0; t < T; t++) kzg::cells_step(img.data(), tab.data(), t, k);
          for (uint32_t t = 0; t < T; t++)
            if (kzg::recover_store_half(img.data(), in, out, mask, t, half)) bad = KZG_ERR_CELLS_INCONSISTENT;
        }
      }
    }
    if (bad) memset(out, 0, ITEM);
    fwrite(&bad, sizeof bad, 1, stdout);
    fwrite(out, 1, ITEM, stdout);
  }
  fclose(f);
  free(in);
  free(out);
  return 0;
}
