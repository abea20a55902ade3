// The coefficient-vector tree of the per-item cell verdicts as k_cells_each_leaves and k_each_vec_level build it
// (kateth_amd/csrc/cellverify_kernels.cuh), compiled for the host: the same KZG_HD steps (cellverify_math.cuh), a workgroup's threads
// walked in a loop where the kernel has a barrier, the tables built by the entry functions the setup kernels call.  Every limb operation
// is re-checked (KZG_FP28_CHECK).
//   cellv_each_leaf <file>   file = records of {column: 4 bytes little-endian, r_i: 32 bytes big-endian, cell: 2048 bytes}
//   ->  the tree's nodes level after level from the leaves (level l has ceil(n / 2^l) nodes), 64 lines of hex per node:
//       leaf i = r_i I_i, an inner node = the sum of its two children, a missing sibling being zero
// A record whose column is >= 128 stands for a rejected item: it contributes the zero vector, as the kernel's status test has it.
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
    bool live;
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
    r.live = r.c < 128;
    fr_from_be_bytes_plain(r.rk, head + 4);
    if (!fr_is_canonical(r.rk)) return 3;
    for (int e = 0; e < 64; e++) {
      fr_from_be_bytes_plain(r.v[e], cell + 32 * e);
      if (r.live && !fr_is_canonical(r.v[e])) return 3;
    }
    recs.push_back(r);
  }
  fclose(f);
  const size_t n = recs.size();
  if (n == 0) return 3;
  std::vector<size_t> off{0};
  for (size_t cnt = n;; cnt = (cnt + 1) / 2) {
    off.push_back(off.back() + cnt);
    if (cnt == 1) break;
  }
  std::vector<fr_t> tree(off.back() * 64);
  std::vector<uint32_t> img(CELLV_IMAGE_DWORDS);
  fr_t zero;
  for (int q = 0; q < 8; q++) zero.v[q] = 0;
  const size_t groups = (n + CELLV_CELLS - 1) / CELLV_CELLS;
  for (size_t g = 0; g < groups; g++) {
    auto live = [&](size_t k) { return k < n && recs[k].live; };
    for (uint32_t tid = 0; tid < (uint32_t)CELLV_THREADS; tid++) {
      const uint32_t cl = tid >> 3, t = tid & 7u;
      const size_t k = g * CELLV_CELLS + cl;
      fr_t v[8];
      for (int i = 0; i < 8; i++) v[i] = live(k) ? recs[k].v[8 * t + i] : zero;
      cellv_step_a(img.data(), ct, cl, t, v);
    }
    for (uint32_t tid = 0; tid < (uint32_t)CELLV_THREADS; tid++) {
      const uint32_t cl = tid >> 3, t = tid & 7u;
      const size_t k = g * CELLV_CELLS + cl;
      cellv_step_b(img.data(), ct, vt, cl, t, live(k) ? recs[k].c : 0u, live(k) ? recs[k].rk : zero);
    }
    for (uint32_t tid = 0; tid < (uint32_t)CELLV_THREADS; tid++)
      for (uint32_t q = 0; q < 8; q++) {
        const uint32_t flat = tid + (uint32_t)CELLV_THREADS * q, c2 = flat >> 6, j = flat & 63u;
        const size_t item = g * CELLV_CELLS + c2;
        if (item >= n) continue;
        cellv_cell_coeff(tree[item * 64 + j], img.data(), c2, j);
      }
  }
  for (size_t l = 0; l + 2 < off.size(); l++) {
    const size_t cin = off[l + 1] - off[l], cout = off[l + 2] - off[l + 1];
    const fr_t* in = tree.data() + off[l] * 64;
    fr_t* out = tree.data() + off[l + 1] * 64;
    for (size_t id = 0; id < cout * 64; id++) {
      const size_t j = id >> 6, c = id & 63u;
      fr_t acc = in[2 * j * 64 + c];
      if (2 * j + 1 < cin) cellv_vec_add(acc, in[(2 * j + 1) * 64 + c]);
      out[id] = acc;
    }
  }
  for (const fr_t& v : tree) print_fr(v);
  return 0;
}
