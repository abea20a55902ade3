// The blob extension of compute_cells as k_compute_cells runs it (kateth_amd/csrc/cells_kernels.cuh), compiled for the host: the same
// KZG_HD helpers and the same seven steps (cells_math.cuh), the workgroup's 512 threads walked in a loop where the kernel has a barrier,
// the twiddle table built by the entry function the setup kernel calls.  Every limb operation is re-checked (KZG_FP28_CHECK).
//   cells_ntt <file of 131,072-byte blobs>   ->  per blob one line: the 4096 x 32 bytes of the extension half (cells 64..127) in hex
#define KZG_FP28_CHECK 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../kateth_amd/csrc/cells_math.cuh"

extern "C" void kzg_fp28_check_failed(const char* what) {
  fprintf(stderr, "bound check failed: %s\n", what);
  abort();
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  alignas(16) static uint32_t tab[kzg::CELLS_TAB_ENTRIES * kzg::CELLS_TAB_ENTRY];
  for (uint32_t i = 0; i < kzg::CELLS_TAB_ENTRIES; i++) kzg::cells_tab_entry(i, tab + (size_t)i * kzg::CELLS_TAB_ENTRY);
  std::vector<uint8_t> blob(131072);
  std::vector<uint32_t> img(kzg::CELLS_IMAGE_DWORDS);
  std::vector<char> line(2 * 131072 + 2);
  while (fread(blob.data(), 1, blob.size(), f) == blob.size()) {
    for (uint32_t e = 0; e < 4096; e++) {
      kzg::fr_t v;
      kzg::fr_from_be_bytes_plain(v, blob.data() + 32 * e);
      if (!kzg::fr_is_canonical(v)) return 3;
      kzg::cells_put(img.data(), e, v);
    }
    for (int k = 0; k < kzg::CELLS_STEPS; k++)
      for (uint32_t t = 0; t < (uint32_t)kzg::CELLS_THREADS; t++) kzg::cells_step(img.data(), tab, t, k);
    for (uint32_t e = 0; e < 4096; e++) {
      kzg::fr_t v;
      uint8_t be[32];
      kzg::cells_get(v, img.data(), e);
      kzg::fr_to_be_bytes_plain(be, v);
      for (int i = 0; i < 32; i++) snprintf(&line[64 * e + 2 * i], 3, "%02x", be[i]);
    }
    line[2 * 131072] = '\n';
    fwrite(line.data(), 1, 2 * 131072 + 1, stdout);
  }
  fclose(f);
  return 0;
}
