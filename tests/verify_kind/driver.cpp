// Test driver of kateth_amd/csrc/verify_kind.hpp: the table of per-kind facts, read out row by row.
#include <cstdint>

#include "../../kateth_amd/csrc/verify_kind.hpp"

using kzg::verify::facts;
using kzg::verify::Kind;

extern "C" {
int32_t verify_kind_entries(int32_t kind) { return facts((Kind)kind).entries; }
int32_t verify_kind_slot(int32_t kind, int32_t entry) { return facts((Kind)kind).slot[entry]; }
uint32_t verify_kind_tail_terms(int32_t kind) { return facts((Kind)kind).tail_terms; }
const char* verify_kind_domain(int32_t kind) { return facts((Kind)kind).domain; }
int32_t verify_kind_pair_tau64(int32_t kind) { return facts((Kind)kind).pair_tau64 ? 1 : 0; }
const char* verify_kind_trace_fused(int32_t kind) { return facts((Kind)kind).trace_fused; }
const char* verify_kind_trace_group_dev(int32_t kind) { return facts((Kind)kind).trace_group_dev; }
int32_t verify_kind_named_entry(int32_t which) {
  const int32_t e[5] = {kzg::verify::BLOBS_BLOB, kzg::verify::POINTS_Z, kzg::verify::POINTS_Y, kzg::verify::CELLS_INDEX, kzg::verify::CELLS_CELL};
  return e[which];
}
}
