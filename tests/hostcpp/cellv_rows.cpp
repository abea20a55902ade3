// The commitment scalars of the row-indexed cell verification as k_cells_row_weights and k_cells_roww_reduce run them
// (kateth_amd/csrc/cellverify_kernels.cuh), compiled for the host: the same KZG_HD steps (cellverify_math.cuh), a workgroup's threads
// walked in a loop where the kernel has a barrier, one workgroup per (commitment, tile), then the reduce launch's sum per commitment.
//   cellv_rows <file> [tile]   file = u (8 bytes little-endian), then records of {commitment index: 8 bytes little-endian,
//                              index status: 4 bytes little-endian, r^k: 32 bytes big-endian}
//   ->  u lines: w_c in hex.  `tile`: items per tile instead of cellv_roww_tile(n), a multiple of the workgroup size
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../kateth_amd/csrc/cellverify_math.cuh"

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
  if (argc != 2 && argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t head[8];
  if (fread(head, 1, 8, f) != 8) return 3;
  const uint64_t u = le64(head);
  std::vector<unsigned long long> idx;
  std::vector<int32_t> status;
  std::vector<fr_t> rpow;
  for (;;) {
    uint8_t rec[44];
    if (fread(rec, 1, 44, f) != 44) break;
    idx.push_back(le64(rec));
    status.push_back((int32_t)(rec[8] | (rec[9] << 8) | (rec[10] << 16) | ((uint32_t)rec[11] << 24)));
    fr_t v;
    fr_from_be_bytes_plain(v, rec + 12);
    if (!fr_is_canonical(v)) return 3;
    rpow.push_back(v);
  }
  fclose(f);
  const uint64_t n = idx.size();
  if (n == 0) return 3;
  const uint64_t tile = argc == 3 ? strtoull(argv[2], nullptr, 10) : cellv_roww_tile(n);
  if (tile == 0 || tile % CELLV_ROWW_THREADS) return 2;
  const uint32_t tiles = (uint32_t)((n + tile - 1) / tile);
  if (argc == 2 && tiles != cellv_roww_tiles(n)) return 4;
  std::vector<fr_t> partials((size_t)u * tiles), red(CELLV_ROWW_THREADS);
  for (uint64_t c = 0; c < u; c++)
    for (uint32_t ti = 0; ti < tiles; ti++) {
      const uint64_t lo = (uint64_t)ti * tile, hi = lo + tile < n ? lo + tile : n;
      for (uint32_t t = 0; t < (uint32_t)CELLV_ROWW_THREADS; t++) cellv_roww_thread(red[t], idx.data(), status.data(), rpow.data(), lo, hi, t, c);
      for (uint32_t w = CELLV_ROWW_THREADS / 2; w >= 1; w >>= 1)  // a barrier between the steps
        for (uint32_t t = 0; t < w; t++) cellv_roww_fold(red.data(), t, w);
      partials[(size_t)c * tiles + ti] = red[0];
    }
  for (uint64_t c = 0; c < u; c++) {
    fr_t out;
    cellv_roww_sum(out, partials.data() + (size_t)c * tiles, tiles);
    uint8_t be[32];
    fr_to_be_bytes_plain(be, out);
    for (int i = 0; i < 32; i++) printf("%02x", be[i]);
    printf("\n");
  }
  return 0;
}
