// The kinds of batch verification call and everything that differs between them, stated once: plain host constants, no HIP -- kept
// apart so that a CPU test (tests/test_verify_kind.py) pins the table without a GPU.  The drivers (engine_verify.hip) read it through
// the session's kind; a new kind is a new row.
//
// A call's error record is `entries` x {local index of the first rejected item or -1, code} in the reference's parse order (`entry`
// below).  On the device a session keeps one status array of n words per entry, entry e's at `stat + slot[e] * n`: in every kind the
// point decoder writes the commitments' statuses to slot 1 and the proofs' to slot 2, and the front kernel of the kind takes what is left.
//   BLOBS  (verify_blob_proof_batch, src/kzg/setup.rs:259-271): blob, commitment, proof         = the ABI's err6
//   POINTS (verify_proof_batch, :103-109):                      proof, commitment, z, y          = the ABI's err8
//   CELLS  (verify_cell_kzg_proof_batch, EIP-7594):             cell index, commitment, cell, proof
#pragma once
#include <stdint.h>

namespace kzg {
namespace verify {

enum class Kind { BLOBS, POINTS, CELLS };

struct KindFacts {
  int entries;          // of the error record
  int slot[4];          // status slot of entry e (-1: the record has no such entry)
  uint32_t tail_terms;  // lincomb B's terms behind the 2n points: the generator, or the 64 monomial points [tau^j]_1
  char domain[17];      // 16 bytes: the spec's domain of the batch challenge r
  bool pair_tau64;      // the pairing against A takes [tau^64]_2 instead of [tau]_2
  const char *trace_fused, *trace_group_dev;  // KATETH_AMD_TRACE labels of the two drivers that name their kind
};

constexpr KindFacts KIND_FACTS[3] = {
    {3, {0, 1, 2, -1}, 1, "RCKZGBATCH___V1_", false, "verify (fused phases)", "group verify (device-resident)"},
    {4, {2, 1, 0, 3}, 1, "RCKZGBATCH___V1_", false, "verify_proof_batch (fused phases)", "group verify_proof_batch (device-resident)"},
    {4, {3, 1, 0, 2}, 64, "RCKZGCBATCH__V1_", true, "verify_cell_proof_batch (fused phases)", "group verify_cell_proof_batch (device-resident)"},
};
constexpr const KindFacts& facts(Kind kind) { return KIND_FACTS[(int)kind]; }

// the entries whose status arrays a front kernel writes or phase 2 reads by name (the decoder's two are slots 1 and 2 everywhere)
enum Entry : int { BLOBS_BLOB = 0, POINTS_Z = 2, POINTS_Y = 3, CELLS_INDEX = 0, CELLS_CELL = 2 };
static_assert(facts(Kind::BLOBS).slot[BLOBS_BLOB] == 0, "the evaluation kernel's statuses");
static_assert(facts(Kind::POINTS).slot[POINTS_Z] == 0 && facts(Kind::POINTS).slot[POINTS_Y] == 3, "k_points_leaves' two arrays");
static_assert(facts(Kind::CELLS).slot[CELLS_INDEX] == 3 && facts(Kind::CELLS).slot[CELLS_CELL] == 0, "k_cells_leaves' two arrays");

}  // namespace verify
}  // namespace kzg
