// The per-item status fold of the row-indexed cell verification's verdicts as k_each_rows_status runs it
// (kateth_amd/csrc/cellverify_kernels.cuh), compiled for the host: the same KZG_HD function (cellverify_math.cuh: cellv_rows_item_status)
// per item, and the kernel's two counts taken in a loop over max(n, u) "threads".
//   cellv_rows_status <file>   file = n, u (8 bytes little-endian each), then the session's four status arrays as they lie there --
//                              stride = max(n, u) words each, slot 0 cell, slot 1 commitment (u words used), slot 2 proof, slot 3 index
//                              (verify_kind.hpp's row of the cells kind) -- then n commitment indices (8 bytes little-endian)
//   ->  n lines: item i's code; then one line "rejected bad_list"
// Every array is copied into a vector of exactly the words the kernel may touch (n, or u for the commitments), so the address
// sanitizer sees a read past either.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../kateth_amd/csrc/cellverify_math.cuh"
#include "../../kateth_amd/csrc/verify_kind.hpp"

extern "C" void kzg_fp28_check_failed(const char* what) {
  fprintf(stderr, "bound check failed: %s\n", what);
  abort();
}

static uint64_t le64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}

int main(int argc, char** argv) {
  using namespace kzg;
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t head[16];
  if (fread(head, 1, 16, f) != 16) return 3;
  const uint64_t n = le64(head), u = le64(head + 8), stride = n > u ? n : u;
  if (n == 0 || stride > (1u << 20)) return 3;
  std::vector<uint8_t> raw(4 * stride * 4 + n * 8);
  if (fread(raw.data(), 1, raw.size(), f) != raw.size()) return 3;
  fclose(f);
  auto slot = [&](int entry, uint64_t words) {
    const int s = verify::facts(verify::Kind::CELLS).slot[entry];
    std::vector<int32_t> out(words);
    for (uint64_t k = 0; k < words; k++) {
      const uint8_t* p = raw.data() + ((uint64_t)s * stride + k) * 4;
      out[k] = (int32_t)(p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24));
    }
    return out;
  };
  // the record's order: cell index, commitment, cell, proof
  const std::vector<int32_t> st_index = slot(0, n), st_com = slot(1, u), st_cell = slot(2, n), st_proof = slot(3, n);
  std::vector<unsigned long long> idx(n);
  for (uint64_t i = 0; i < n; i++) idx[i] = le64(raw.data() + 4 * stride * 4 + i * 8);
  std::vector<int32_t> status(n);
  uint32_t counts[2] = {0, 0};
  for (uint64_t i = 0; i < stride; i++) {  // one kernel thread each
    if (i < n) {
      const int32_t c = cellv_rows_item_status(st_index.data(), st_com.data(), st_cell.data(), st_proof.data(), idx.data(), u, i);
      status[i] = c;
      if (c) counts[0]++;
    }
    if (i < u && st_com[i]) counts[1]++;
  }
  for (uint64_t i = 0; i < n; i++) printf("%d\n", status[i]);
  printf("%u %u\n", counts[0], counts[1]);
  return 0;
}
