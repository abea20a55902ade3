// The host side of the blob form of cell verification (kzg_verify_blob_cell_proofs_batch), compiled for the host: the KZG_HD functions of
// kateth_amd/csrc/cellverify_math.cuh that the blob instances of the verify kernels run.
//   blob_cells addr <file>      file = n (8 bytes little-endian), then n blobs and n extension halves (131,072 bytes each)
//                               -> stdout: the 128 n cells item by item, each read through cellv_blob_cell as a lane of the front or a
//                                  thread of k_blob_cells_interp reads it (2,048 bytes from the address): the expanded cell array
//   blob_cells weights <file>   file = n (8 bytes little-endian), then 128 n powers r^k (32 bytes big-endian)
//                               -> n lines: w_b in hex, k_blob_weights' workgroup walked thread by thread
//   blob_cells code <file>      file = records of {blob status, commitment status, 128 proof statuses} (130 x 4 bytes little-endian)
//                               -> per record: the blob's code, k_each_blob_status' fold (the LDS minimum as a loop over the threads)
// Every buffer is a vector of exactly the bytes the kernels may touch, so the address sanitizer sees a read past either.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
static int32_t le32(const uint8_t* p) { return (int32_t)(p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24)); }

static std::vector<uint8_t> read_all(const char* path) {
  std::vector<uint8_t> out;
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  uint8_t buf[65536];
  for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + got);
  fclose(f);
  return out;
}

int main(int argc, char** argv) {
  using namespace kzg;
  if (argc != 3) return 2;
  const std::vector<uint8_t> raw = read_all(argv[2]);
  if (!strcmp(argv[1], "addr")) {
    if (raw.size() < 8) return 3;
    const uint64_t n = le64(raw.data());
    if (n == 0 || n > 16 || raw.size() != 8 + 2 * n * 131072) return 3;
    const std::vector<uint8_t> blobs(raw.begin() + 8, raw.begin() + 8 + n * 131072), ext(raw.begin() + 8 + n * 131072, raw.end());
    for (uint64_t i = 0; i < n * CELLV_BLOB_ITEMS; i++) {
      const uint8_t* cell = cellv_blob_cell(blobs.data(), ext.data(), i);
      // the choice is one select per item: the cell lies whole in one of the two buffers
      const bool in_blobs = cell >= blobs.data() && cell + KZG_BYTES_PER_CELL <= blobs.data() + blobs.size();
      const bool in_ext = cell >= ext.data() && cell + KZG_BYTES_PER_CELL <= ext.data() + ext.size();
      if (in_blobs == in_ext || in_blobs != ((i & 127u) < 64)) return 4;
      if (fwrite(cell, 1, KZG_BYTES_PER_CELL, stdout) != KZG_BYTES_PER_CELL) return 5;
    }
    return 0;
  }
  if (!strcmp(argv[1], "weights")) {
    if (raw.size() < 8) return 3;
    const uint64_t n = le64(raw.data());
    if (n == 0 || raw.size() != 8 + n * CELLV_BLOB_ITEMS * 32) return 3;
    std::vector<fr_t> rpow(n * CELLV_BLOB_ITEMS), red(CELLV_BLOB_ITEMS);
    for (uint64_t k = 0; k < rpow.size(); k++) {
      fr_from_be_bytes_plain(rpow[k], raw.data() + 8 + 32 * k);
      if (!fr_is_canonical(rpow[k])) return 3;
    }
    for (uint64_t b = 0; b < n; b++) {  // one workgroup each
      for (uint32_t t = 0; t < (uint32_t)CELLV_BLOB_ITEMS; t++) red[t] = rpow[b * CELLV_BLOB_ITEMS + t];
      for (uint32_t w = CELLV_BLOB_ITEMS / 2; w >= 1; w >>= 1)  // a barrier between the steps
        for (uint32_t t = 0; t < w; t++) cellv_roww_fold(red.data(), t, w);
      uint8_t be[32];
      fr_to_be_bytes_plain(be, red[0]);
      for (int i = 0; i < 32; i++) printf("%02x", be[i]);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "code")) {
    const size_t rec = (2 + CELLV_BLOB_ITEMS) * 4;
    if (raw.empty() || raw.size() % rec) return 3;
    for (size_t r = 0; r < raw.size() / rec; r++) {
      const uint8_t* p = raw.data() + r * rec;
      std::vector<int32_t> st_proof(CELLV_BLOB_ITEMS);
      for (int k = 0; k < CELLV_BLOB_ITEMS; k++) st_proof[k] = le32(p + 8 + 4 * k);
      uint32_t first = CELLV_BLOB_ITEMS;  // atomicMin over the threads with a rejected proof
      for (uint32_t t = 0; t < (uint32_t)CELLV_BLOB_ITEMS; t++)
        if (st_proof[t] && t < first) first = t;
      printf("%d\n", cellv_blob_code(le32(p), le32(p + 4), st_proof.data(), first));
    }
    return 0;
  }
  return 2;
}
