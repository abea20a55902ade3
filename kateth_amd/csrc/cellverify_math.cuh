// verify_cell_kzg_proof_batch (EIP-7594, specs/fulu/polynomial-commitments-sampling.md): the arithmetic that turns the cells of a batch
// into the 64 coefficients  S_j = sum_k r^k [X^j] I_k  of the random linear combination of their interpolation polynomials, host and
// device.  No kernels here: cellverify_kernels.cuh (engine_verify.hip) runs the steps on a 128-thread workgroup, setup_kernels.cuh
// (engine.hip) builds the table with cellv_tab_entry, tests/hostcpp/cellv_interp.cpp walks the same steps on the host.
//
// Cell c holds E[i] = p(h_c w64^brp6(i)), i < 64, with h_c = omega_8192^brp7(c) (the spec's coset_shift_for_cell) and w64 the 64th
// root of unity.  I_c is the polynomial of degree < 64 through those points; with J(X) = I_c(h_c X):
//   1. the cell as it lies in memory is the bit-reversed input of a 64-point decimation-in-time INVERSE transform with w64^-1 -- there
//      is no permutation to undo by hand -- whose natural-order output is 64 [X^j] J.  Its six stages are the first two passes of
//      compute_cells' inverse transform (cells_pass_inv, strides 1 and 8): the first six stages of a radix-2 DIT transform do not
//      depend on its length, so entries 0..62 of compute_cells' twiddle table serve as they are.
//   2. [X^j] I_c = [X^j] J * h_c^-j; coefficient j is multiplied by the table entry (c, j) = h_c^-j / 64 and by r^k.
//   3. the coefficients of the workgroup's cells are summed per j.
// Arithmetic as in cells_math.cuh: radix-2^29 limbs, PLAIN data, constants stored with the Montgomery factors the products remove.
// r^k arrives plain (k_batch_scalars' lincomb scalar), so the table entry carries 2^261 twice:
//   f29_mul(f29_mul(x, h^-j / 64 * 2^522), r^k) = x h^-j r^k / 64.
// Bounds (units of r): the passes are cells_math.cuh's with normalised inputs < 2 and a cells_reduce behind each; both products take
// an operand < 2 and a canonical one; a sum takes two normalised values < 2 (limbs < 2^30, value < 4) into cells_reduce.
#pragma once
#include "../../include/kateth_amd.h"  // KZG_ERR_COMMITMENT_INDEX (cellv_rows_item_status)
#include "cells_math.cuh"

namespace kzg {

constexpr int CELLV_CELLS = 16;                     // cells per workgroup
constexpr int CELLV_THREADS = 8 * CELLV_CELLS;      // eight threads per cell, eight elements per thread
constexpr int CELLV_PLANE = 64 * CELLV_CELLS;       // the workgroup's image: eight word planes of this many dwords (32 KiB)
constexpr int CELLV_IMAGE_DWORDS = 8 * CELLV_PLANE;
// table: entry c * 64 + j = h_c^-j / 64 * 2^522, canonical, nine limbs padded to twelve dwords like compute_cells' entries
constexpr uint32_t CELLV_TAB_ENTRIES = 128 * 64;

KZG_HD uint32_t cellv_brp7(uint32_t c) {
  uint32_t o = 0;
  KZG_UNROLL_FULL
  for (int b = 0; b < 7; b++) o |= ((c >> b) & 1u) << (6 - b);
  return o;
}

// omega_8192^e, Montgomery
KZG_HD void cellv_root_pow(fr_t& acc, uint32_t e) {
  fr_t g;
  {
    const uint32_t om[8] = KZG_FR_OMEGA8192_MONT;
    KZG_UNROLL_FULL
    for (int q = 0; q < 8; q++) g.v[q] = om[q];
  }
  acc = fr_one();
  for (int bit = 12; bit >= 0; bit--) {
    fr_sqr(acc, acc);
    if ((e >> bit) & 1u) fr_mul(acc, acc, g);
  }
}

// z of cell c in the batched check: h_c^64 = omega_128^brp7(c), plain
KZG_HD void cellv_h64_plain(fr_t& out, uint32_t c) {
  fr_t m;
  cellv_root_pow(m, 64u * cellv_brp7(c));
  from_mont<FrParams>(out, m);
}

KZG_HD void cellv_tab_entry(uint32_t idx, uint32_t* out) {
  const uint32_t c = idx >> 6, j = idx & 63u;
  const uint32_t e = (8192u - ((cellv_brp7(c) * j) & 8191u)) & 8191u;  // h_c^-j
  fr_t acc, f, c261, sixty_four = fr_one();
  cellv_root_pow(acc, e);
  {
    const uint32_t c4096[8] = KZG_FR_INV4096_MONT, a[8] = KZG_FR_R261_PLAIN;
    KZG_UNROLL_FULL
    for (int q = 0; q < 8; q++) {
      f.v[q] = c4096[q];
      c261.v[q] = a[q];
    }
  }
  for (int k = 0; k < 6; k++) fr_add(sixty_four, sixty_four, sixty_four);
  fr_mul(f, f, sixty_four);  // 1 / 64
  fr_mul(acc, acc, f);
  fr_mul(acc, acc, c261);  // (v 2^256)(2^261) / 2^256 = v 2^261
  to_mont<FrParams>(acc, acc);
  fr_mul(acc, acc, c261);  // v 2^522
  fr29 o;
  f29_from_bn(o, acc);
  KZG_UNROLL_FULL
  for (int q = 0; q < F29_N; q++) out[q] = o.l[q];
  KZG_UNROLL_FULL
  for (int q = F29_N; q < CELLS_TAB_ENTRY; q++) out[q] = 0;
}

// Dword index of element e of the workgroup's cell cl in a word plane.  A 32-lane group is four cells x eight threads; thread t holds
// e = 8 t + i in the first pass and e = t + 8 i in the second, and 32 lanes read coefficient j = lane of one cell in the sum: folding
// bits 3..5 of e onto bits 0..2 and the cell onto bits 3..4 makes each of them 32 different banks.
KZG_HD uint32_t cellv_slot(uint32_t cl, uint32_t e) { return cl * 64u + (e ^ ((e >> 3) & 7u) ^ ((cl & 3u) << 3)); }

KZG_HD void cellv_put(uint32_t* img, uint32_t cl, uint32_t e, const fr_t& v) {
  const uint32_t s = cellv_slot(cl, e);
  KZG_UNROLL_FULL
  for (int q = 0; q < 8; q++) img[q * CELLV_PLANE + s] = v.v[q];
}
KZG_HD void cellv_get(fr_t& v, const uint32_t* img, uint32_t cl, uint32_t e) {
  const uint32_t s = cellv_slot(cl, e);
  KZG_UNROLL_FULL
  for (int q = 0; q < 8; q++) v.v[q] = img[q * CELLV_PLANE + s];
}

// Step A of thread t (< 8) of cell cl: v = elements 8 t .. 8 t + 7 of the cell as they lie in memory (plain, canonical; all zero for a
// cell that contributes nothing).  Stages of half-size 1, 2, 4; the result goes to the image.
KZG_HD void cellv_step_a(uint32_t* img, const uint32_t* ctab, uint32_t cl, uint32_t t, const fr_t (&v)[8]) {
  fr29 x[8];
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) f29_from_bn(x[i], v[i]);
  cells_pass_inv(x, ctab, CELLS_TAB_INV, 1u);
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    cells_reduce(x[i]);
    fr_t o;
    f29_to_bn(o, x[i]);
    cellv_put(img, cl, 8u * t + (uint32_t)i, o);
  }
}

// Step B: elements t + 8 i, stages of half-size 8, 16, 32, then coefficient j = t + 8 i times vtab[c, j] times r^k (plain, canonical);
// back to the image, normalised, < 2r.  c < 128.
KZG_HD void cellv_step_b(uint32_t* img, const uint32_t* ctab, const uint32_t* vtab, uint32_t cl, uint32_t t, uint32_t c, const fr_t& rk_plain) {
  fr29 x[8], rk;
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    fr_t v;
    cellv_get(v, img, cl, t + 8u * (uint32_t)i);
    f29_from_bn(x[i], v);
  }
  cells_pass_inv(x, ctab, CELLS_TAB_INV + 7u + t, 8u);
  f29_from_bn(rk, rk_plain);
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    cells_reduce(x[i]);
    fr29 w;
    cells_tw(w, vtab, c * 64u + t + 8u * (uint32_t)i);
    f29_mul(x[i], x[i], w);
    cells_fence();
    f29_mul(x[i], x[i], rk);
    cells_fence();
    fr_t o;
    f29_to_bn(o, x[i]);
    cellv_put(img, cl, t + 8u * (uint32_t)i, o);
  }
}

// Step C of thread j (< 64): coefficient j summed over the workgroup's cells in cell order, canonical
KZG_HD void cellv_step_c(fr_t& out, const uint32_t* img, uint32_t j) {
  fr29 acc;
  KZG_UNROLL_FULL
  for (int i = 0; i < F29_N; i++) acc.l[i] = 0;
  for (uint32_t cl = 0; cl < (uint32_t)CELLV_CELLS; cl++) {
    fr_t v;
    fr29 x;
    cellv_get(v, img, cl, j);
    f29_from_bn(x, v);
    f29_add(acc, acc, x);
    cells_reduce(acc);
  }
  f29_to_canonical_bn(out, acc);
}

// per-item verdicts: coefficient j of the workgroup's cell cl as step B left it (r_i [X^j] I_i), canonical -- a leaf of the vector tree
KZG_HD void cellv_cell_coeff(fr_t& out, const uint32_t* img, uint32_t cl, uint32_t j) {
  fr_t v;
  fr29 x;
  cellv_get(v, img, cl, j);
  f29_from_bn(x, v);
  f29_to_canonical_bn(out, x);
}
// the vector tree's inner nodes: canonical plain values summed coefficient by coefficient, canonical again
KZG_HD void cellv_vec_add(fr_t& acc, const fr_t& other) { fr_add(acc, acc, other); }

// the reduce launch's arithmetic: partial vectors (canonical, plain) summed in their order, negated: lincomb B's scalar -S_j
KZG_HD void cellv_neg_sum(fr_t& out, const fr_t* partials, uint32_t count, uint32_t stride) {
  fr_t acc;
  KZG_UNROLL_FULL
  for (int q = 0; q < 8; q++) acc.v[q] = 0;
  for (uint32_t k = 0; k < count; k++) fr_add(acc, acc, partials[(size_t)k * stride]);
  fr_neg(out, acc);
}

// ---- the row-indexed form (kzg_verify_cell_proof_batch_rows): commitment c of a list of u takes ONE scalar in lincomb B ---------------
//   w_c = sum over the items k with commitment index c of r^(first_index + k)        (zero for a commitment nobody references)
// k_cells_row_weights runs one workgroup of CELLV_ROWW_THREADS threads per (commitment, tile of items): thread t takes the tile's items
// t, t + 256, ..., a tree in LDS sums the threads, k_cells_roww_reduce sums a commitment's tiles.  All values plain and canonical:
// fr_add is exact, every order gives the same value.  tests/hostcpp/cellv_rows.cpp walks these functions thread by thread.
constexpr int CELLV_ROWW_THREADS = 256;
// items per tile: at least 2,048 (eight per thread), a multiple of the workgroup, and never more than 32 tiles
KZG_HD uint64_t cellv_roww_tile(uint64_t n) {
  const uint64_t t = ((n + 31) / 32 + 255) / 256 * 256;
  return t < 2048 ? 2048 : t;
}
KZG_HD uint32_t cellv_roww_tiles(uint64_t n) {
  const uint64_t tile = cellv_roww_tile(n);
  return (uint32_t)((n + tile - 1) / tile);
}
// thread t's sum over items lo + t, lo + t + 256, ... < hi of commitment c; status_index (may be null): items rejected for an index
KZG_HD void cellv_roww_thread(fr_t& acc, const unsigned long long* commitment_indices, const int32_t* status_index, const fr_t* rpow_plain, uint64_t lo,
                              uint64_t hi, uint32_t t, uint64_t c) {
  KZG_UNROLL_FULL
  for (int q = 0; q < 8; q++) acc.v[q] = 0;
  for (uint64_t k = lo + t; k < hi; k += (uint64_t)CELLV_ROWW_THREADS) {
    if (commitment_indices[k] != c) continue;
    if (status_index && status_index[k] != 0) continue;
    fr_add(acc, acc, rpow_plain[k]);
  }
}
// one step of the tree: thread t < w adds its neighbour at distance w
KZG_HD void cellv_roww_fold(fr_t* red, uint32_t t, uint32_t w) {
  const fr_t a = red[t], b = red[t + w];
  fr_t s;
  fr_add(s, a, b);
  red[t] = s;
}
// a commitment's tile partials in tile order
KZG_HD void cellv_roww_sum(fr_t& out, const fr_t* partials, uint32_t tiles) {
  fr_t acc;
  KZG_UNROLL_FULL
  for (int q = 0; q < 8; q++) acc.v[q] = 0;
  for (uint32_t k = 0; k < tiles; k++) fr_add(acc, acc, partials[k]);
  out = acc;
}

// ---- per-item verdicts of the row-indexed form (kzg_verify_cell_proof_batch_rows_each): item i's code ----------------------------------
// What kzg_verify_cell_proof_batch returns for the expanded tuple alone, in its parse order: the index slot (KZG_ERR_COMMITMENT_INDEX
// ahead of KZG_ERR_CELL_INDEX, as the front wrote it), else the commitment slot AT commitment_indices[i] -- the list's other entries
// never touch the item -- else the cell slot, else the proof slot.  The index is read, and the commitment slot indexed by it, only when
// the index slot is clear: the front clears it only for a row below ncom, and a row that is not below ncom is answered with the front's
// code all the same, so nothing is indexed by an unchecked value.  The four arrays are the session's (stride max(n, ncom) apart there;
// here just four pointers): st_com has ncom words, the others n.  k_each_rows_status runs it per item, tests/hostcpp/cellv_rows_status.cpp
// on the host.
KZG_HD int32_t cellv_rows_item_status(const int32_t* st_index, const int32_t* st_com, const int32_t* st_cell, const int32_t* st_proof,
                                      const unsigned long long* commitment_indices, uint64_t ncom, uint64_t i) {
  int32_t c = st_index[i];
  if (c) return c;
  const unsigned long long row = commitment_indices[i];
  if (row >= ncom) return KZG_ERR_COMMITMENT_INDEX;
  c = st_com[row];
  if (!c) c = st_cell[i];
  if (!c) c = st_proof[i];
  return c;
}

// ---- the blob form (kzg_verify_blob_cell_proofs_batch): the row-indexed form with implicit indices ------------------------------------
// Item i is cell i & 127 of blob i >> 7: no index array exists.  Cells 0..63 are the blob's own bytes, cells 64..127 lie in the
// extension workspace (k_compute_cells_ext), 131,072 bytes per blob in both.  One select per item; for a wave that works on one cell
// it is uniform.  tests/hostcpp/blob_cells.cpp walks the map against the expanded arrays.
constexpr int CELLV_BLOB_ITEMS = 128;  // items per blob = KZG_CELLS_PER_EXT_BLOB, and the threads of the two per-blob folds below
KZG_HD const uint8_t* cellv_blob_cell(const uint8_t* blobs, const uint8_t* ext, uint64_t i) {
  const uint64_t b = i >> 7, k = i & 127u;
  return (k < 64 ? blobs : ext) + b * 131072ull + (k & 63u) * (uint64_t)KZG_BYTES_PER_CELL;
}
// The blob's code: its own status (the extension kernel's), else its commitment's, else its lowest rejected proof's.  `first_proof`:
// the lowest k < 128 whose proof status is non-zero, 128 for none.
KZG_HD int32_t cellv_blob_code(int32_t st_blob, int32_t st_com, const int32_t* st_proof128, uint32_t first_proof) {
  if (st_blob) return st_blob;
  if (st_com) return st_com;
  return first_proof < (uint32_t)CELLV_BLOB_ITEMS ? st_proof128[first_proof] : 0;
}

}  // namespace kzg
