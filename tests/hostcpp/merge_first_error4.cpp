// Test driver for kzg::multi::merged_first_error with four kinds (kateth_amd/csrc/multi_split.hpp, header-only host code): every line of stdin is
// one case -- W, then per share `first count` and its eight err8 values (LOCAL indices, -1 = none) -- and one merged code is
// printed per case.  Built and fed by tests/test_verify_points_builder.py.
#include <stdio.h>

#include <vector>

#include "../../kateth_amd/csrc/multi_split.hpp"

int main() {
  unsigned W;
  while (scanf("%u", &W) == 1) {
    std::vector<kzg::multi::Share> shares(W);
    std::vector<int32_t> err8(8 * (size_t)W);
    for (unsigned j = 0; j < W; j++) {
      unsigned long long first, count;
      if (scanf("%llu %llu", &first, &count) != 2) return 2;
      shares[j] = kzg::multi::Share{j, first, count};
      for (int k = 0; k < 8; k++)
        if (scanf("%d", &err8[8 * j + k]) != 1) return 2;
    }
    printf("%d\n", kzg::multi::merged_first_error(shares, err8.data(), 4));
  }
  return 0;
}
