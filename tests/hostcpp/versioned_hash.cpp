// versioned_hash_words (kateth_amd/csrc/sha256.cuh) -- the block construction and byte-0 replacement that k_versioned_hash runs one
// lane per commitment -- compiled for the host: every argument is 96 hex digits (one 48-byte commitment), every output line the 64
// hex digits of 0x01 || SHA-256(commitment)[1:32].
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../kateth_amd/csrc/sha256.cuh"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    if (strlen(argv[a]) != 96) return 2;
    uint8_t com[48];
    for (int i = 0; i < 48; i++) {
      unsigned v = 0;
      if (sscanf(argv[a] + 2 * i, "%2x", &v) != 1) return 2;
      com[i] = (uint8_t)v;
    }
    uint32_t h[8];
    kzg::versioned_hash_words(com, h);
    for (int i = 0; i < 8; i++) printf("%08x", h[i]);
    printf("\n");
  }
  return 0;
}
