// The interpolation half of cell verification as k_cells_interp and k_cells_reduce run it (kateth_amd/csrc/cellverify_kernels.cuh),
// compiled for the host: the same KZG_HD steps (cellverify_math.cuh), a workgroup's threads walked in a loop where the kernel has a
// barrier, the tables built by the entry functions the setup kernels call.  Every limb operation is re-checked (KZG_FP28_CHECK).
//   cellv_interp <file>   file = records of {column: 4 bytes little-endian, r^k: 32 bytes big-endian, cell: 2048 bytes}
//   ->  64 lines: -S_j in hex, S = sum over the records of r^k I_k; and one line per column 0..127: h_c^64 in hex
// The records fill workgroups of CELLV_CELLS cells in order (the last one padded with cells that contribute nothing), one partial vector
// per workgroup, summed and negated as the reduce launch does.
#define KZG_FP28_CHECK 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../kateth_amd/csrc/cellverify_math.cuh"

extern "C" void kzg_fp28_check_failed(const char* what) {
  fprintf(stderr, "bound check failed: %s\n", what);
  abort();
}

static void print_fr(const kzg::fr_t& v) {
  uint8_t be[32];
  kzg::fr_to_be_bytes_plain(be, v);
  for (int i = 0; i < 32; i++) printf("%02x", be[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  using namespace kzg;
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> ctab((size_t)CELLS_TAB_ENTRIES * CELLS_TAB_ENTRY), vtab((size_t)CELLV_TAB_ENTRIES * CELLS_TAB_ENTRY + 4);
  uint32_t* ct = ctab.data();
  uint32_t* vt = vtab.data();
  while (((uintptr_t)vt) & 15u) vt++;  // cells_tw assumes 16-byte aligned entries
  if (((uintptr_t)ct) & 15u) return 4;
  for (uint32_t i = 0; i < 63; i++) cells_tab_entry(i, ct + (size_t)i * CELLS_TAB_ENTRY);
  for (uint32_t i = 0; i < CELLV_TAB_ENTRIES; i++) cellv_tab_entry(i, vt + (size_t)i * CELLS_TAB_ENTRY);
  struct Rec {
    uint32_t c;
    fr_t rk;
    fr_t v[64];
  };
  std::vector<Rec> recs;
  for (;;) {
    uint8_t head[36], cell[2048];
    if (fread(head, 1, 36, f) != 36) break;
    if (fread(cell, 1, 2048, f) != 2048) return 3;
    Rec r;
    r.c = head[0] | (head[1] << 8) | (head[2] << 16) | ((uint32_t)head[3] << 24);
    if (r.c >= 128) return 3;
    fr_from_be_bytes_plain(r.rk, head + 4);
    for (int e = 0; e < 64; e++) {
      fr_from_be_bytes_plain(r.v[e], cell + 32 * e);
      if (!fr_is_canonical(r.v[e])) return 3;
    }
    recs.push_back(r);
  }
  fclose(f);
  const size_t groups = (recs.size() + CELLV_CELLS - 1) / CELLV_CELLS;
  std::vector<fr_t> partials(groups * 64);
  std::vector<uint32_t> img(CELLV_IMAGE_DWORDS);
  fr_t zero;
  for (int q = 0; q < 8; q++) zero.v[q] = 0;
  for (size_t g = 0; g < groups; g++) {
    for (uint32_t tid = 0; tid < (uint32_t)CELLV_THREADS; tid++) {
      const uint32_t cl = tid >> 3, t = tid & 7u;
      const size_t k = g * CELLV_CELLS + cl;
      fr_t v[8];
      for (int i = 0; i < 8; i++) v[i] = k < recs.size() ? recs[k].v[8 * t + i] : zero;
      cellv_step_a(img.data(), ct, cl, t, v);
    }
    for (uint32_t tid = 0; tid < (uint32_t)CELLV_THREADS; tid++) {
      const uint32_t cl = tid >> 3, t = tid & 7u;
      const size_t k = g * CELLV_CELLS + cl;
      cellv_step_b(img.data(), ct, vt, cl, t, k < recs.size() ? recs[k].c : 0u, k < recs.size() ? recs[k].rk : zero);
    }
    for (uint32_t j = 0; j < 64; j++) cellv_step_c(partials[g * 64 + j], img.data(), j);
  }
  for (uint32_t j = 0; j < 64; j++) {
    fr_t out;
    cellv_neg_sum(out, partials.data() + j, (uint32_t)groups, 64);
    print_fr(out);
  }
  for (uint32_t c = 0; c < 128; c++) {
    fr_t h;
    cellv_h64_plain(h, c);
    print_fr(h);
  }
  return 0;
}
