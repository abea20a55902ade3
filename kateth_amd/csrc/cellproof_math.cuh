// compute_cells_and_kzg_proofs (EIP-7594, specs/fulu/polynomial-commitments-sampling.md) WITHOUT FK20: the arithmetic of the 128 cell
// proofs of a blob, host and device.  No kernels here: cellproof_kernels.cuh (engine_proof.hip) runs these functions on a 512-thread
// workgroup with the image in LDS, tests/hostcpp/cellproof_quot.cpp walks them on the host.
//
// The proof of cell k is the commitment of q_k = (p - I_k) / (X^64 - z_k), z_k = h_k^64 = omega_128^brp7(k).  I_k has degree < 64, so q_k
// is the plain quotient of p by X^64 - z_k, and its 4096 evaluations on the blob's own domain are a scalar vector the fixed-base MSM
// commits like any blob: the transform runs on the scalars, the group work is the MSM's as it stands.
//   coefficients (once per blob)   the four inverse passes of cells_math.cuh on the blob (bit-reversed in, natural out), then one product
//                                  by 1 / 4096 (the twist table's entry 0: g^0 / 4096) -> c_j, canonical
//   division (per blob and cell)   with j = rho + 64 i (rho, i < 64):  q[rho, 63] = 0,  q[rho, i] = c[rho, i + 1] + z q[rho, i + 1] -- 64
//                                  independent chains of 63 steps.  Thread t takes residue rho = t & 63 and the eight consecutive chain
//                                  positions i = 8 s + u (s = t >> 6: the elements of the stride-64 pass) and reads them from global
//                                  memory itself (a wave reads 2 KiB in a row).  Its segment total A_s = sum_u c[rho, 8 s + u] z^u goes to
//                                  16 KiB of LDS beside the image; after a barrier the carry from the segments above is
//                                  T_s = A_(s+1) + z^8 T_(s+1) (T_7 = 0), and the chain is run once more from it:
//                                  q[8 s + 7] = T_s,  q[8 s + u] = c[8 s + u + 1] + z q[8 s + u + 1].  Two table values (z, z^8) per cell.
//                                  The remainder c[rho, 0] + z q[rho, 0] is I_k, the coset interpolant (not needed for the proof).
//   evaluations                    the four forward passes without the twist (natural in, bit-reversed out = the blob's own order, the
//                                  order the comb table is built on); the last one leaves canonical values
// Bounds (units of r; limbs in parentheses): a product is < 2 (2^29); a product plus a canonical coefficient or a reduced total < 4
// (2^30), which is an operand the next product takes (9 x 2^30 x 2^29 + 9 x 2^58 < 2^64); everything is reduced once before it is packed.
#pragma once
#include "recover_math.cuh"  // cells_math.cuh, and the 16-byte big-endian loads

namespace kzg {

constexpr int CELLPROOF_PASSES = 4;                       // per direction
constexpr uint32_t CELLPROOF_TAB_ENTRIES = 128;           // omega_128^e * 2^261, entries shaped like cells_tab_entry's
constexpr int CELLPROOF_CARRY_DWORDS = 8 * CELLS_THREADS;  // the segment totals: eight word planes of 512 dwords, 16,384 B
constexpr uint32_t CELLPROOF_COEFF_BYTES = 131072;         // a blob's 4096 coefficients: 8 x u32 little-endian each, natural order

KZG_HD uint32_t cellproof_brp7(uint32_t k) {
  uint32_t o = 0;
  KZG_UNROLL_FULL
  for (int i = 0; i < 7; i++) o |= ((k >> i) & 1u) << (6 - i);
  return o;
}
// index of z_k^e in the table
KZG_HD uint32_t cellproof_zpow(uint32_t cell, uint32_t e) { return (e * cellproof_brp7(cell)) & 127u; }
// a pair of the select calls' list (cellproof_plan.hpp): 128 * item + cell, the item counted within its pass
KZG_HD uint32_t cellproof_pair_item(uint32_t pair) { return pair >> 7; }
KZG_HD uint32_t cellproof_pair_cell(uint32_t pair) { return pair & 127u; }

// the eight elements base + i S of thread t in the pass of stride S = 8^p
KZG_HD void cellproof_get8(fr29 (&x)[8], const uint32_t* img, uint32_t base, uint32_t sh) {
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    fr_t v;
    cells_get(v, img, base + ((uint32_t)i << sh));
    f29_from_bn(x[i], v);
  }
}
KZG_HD void cellproof_put8(uint32_t* img, const fr29 (&x)[8], uint32_t base, uint32_t sh, bool canonical) {
  uint32_t at = base;  // on the device the eight slots are computed again, not kept in registers through the pass (recover_step)
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(at));
#endif
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    fr_t v;
    f29_to_bn(v, x[i]);
    if (canonical) canonicalize<FrParams>(v);
    cells_put(img, at + ((uint32_t)i << sh), v);
  }
}

// Inverse pass p = 0..3 of thread t on the image; p = 3 also scales by 1 / 4096 and leaves the coefficients canonical.  Like cells_step
// a pass reads and writes the thread's own eight elements: one barrier between passes.
KZG_HD void cellproof_inv_pass(uint32_t* img, const uint32_t* tab, uint32_t t, int p) {
  const uint32_t sh = 3u * (uint32_t)p, S = 1u << sh;
  const uint32_t low = t & (S - 1u), base = ((t >> sh) << (sh + 3)) + low;
  fr29 x[8];
  cellproof_get8(x, img, base, sh);
  cells_pass_inv(x, tab, CELLS_TAB_INV + S - 1u + low, S);
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) cells_reduce(x[i]);
  if (p == CELLPROOF_PASSES - 1) {
    fr29 w;
    cells_tw(w, tab, CELLS_TAB_TWIST);  // g^0 / 4096
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) {
      f29_mul(x[i], x[i], w);
      cells_fence();
    }
  }
  cellproof_put8(img, x, base, sh, p == CELLPROOF_PASSES - 1);
}
// Forward pass p = 3..0 without the twist; p = 0 leaves the evaluations canonical.
KZG_HD void cellproof_fwd_pass(uint32_t* img, const uint32_t* tab, uint32_t t, int p) {
  const uint32_t sh = 3u * (uint32_t)p, S = 1u << sh;
  const uint32_t low = t & (S - 1u), base = ((t >> sh) << (sh + 3)) + low;
  fr29 x[8];
  cellproof_get8(x, img, base, sh);
  cells_pass_fwd(x, tab, CELLS_TAB_FWD + S - 1u + low, S);
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) cells_reduce(x[i]);
  cellproof_put8(img, x, base, sh, p == 0);
}

// the blob (4096 x 32 big-endian bytes, 16-byte aligned) into the image, element i 512 + t as k_compute_cells reads it; returns whether
// one of this thread's elements is >= r.  Under the column map (cells_math.cuh) `blob` is a column matrix of cells and the item is cells
// 0..63 of one of its rows.
template <class Map = cells_blob_major>
KZG_HD bool cellproof_load_blob(uint32_t* img, const uint8_t* blob, uint32_t t, const Map map = Map()) {
  bool bad = false;
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    const uint32_t e = (uint32_t)i * CELLS_THREADS + t;
    fr_t v;
    recover_ld(v, blob + map((size_t)e * 32u));
    bad |= !fr_is_canonical(v);
    cells_put(img, e, v);
  }
  return bad;
}
// the image (canonical) as 4096 x 8 little-endian words, coalesced like the load: the coefficient buffer and the MSM's scalar vectors
KZG_HD void cellproof_store_words(uint32_t* out, const uint32_t* img, uint32_t t) {
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    const uint32_t e = (uint32_t)i * CELLS_THREADS + t;
    fr_t v;
    cells_get(v, img, e);
    recover_quad* q = reinterpret_cast<recover_quad*>(out + (size_t)e * 8u);
    q[0] = recover_quad{v.v[0], v.v[1], v.v[2], v.v[3]};
    q[1] = recover_quad{v.v[4], v.v[5], v.v[6], v.v[7]};
  }
}

// thread t's segment of the blob's coefficients: c[u] = coefficient 512 s + 64 u + rho, canonical
KZG_HD void cellproof_load_segment(fr29 (&c)[8], const uint32_t* coeffs, uint32_t t) {
  const uint32_t base = ((t >> 6) << 9) + (t & 63u);
  KZG_UNROLL_FULL
  for (int u = 0; u < 8; u++) {
    const recover_quad* p = reinterpret_cast<const recover_quad*>(coeffs + (size_t)(base + 64u * (uint32_t)u) * 8u);
    const recover_quad lo = p[0], hi = p[1];
    const fr_t v{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
    f29_from_bn(c[u], v);
  }
}
// a = c + z a: a < 4r with limbs < 2^30 on entry and on exit
KZG_HD void cellproof_chain(fr29& a, const fr29& c, const fr29& z) {
  f29_mul(a, a, z);
  f29_add(a, a, c);
  cells_fence();
}
// A_s = sum_u c[u] z^u of thread t's segment into the carry planes (< 2r, 8 x 32 bits)
KZG_HD void cellproof_segment_total(uint32_t* carry, const fr29 (&c)[8], const fr29& z, uint32_t t) {
  fr29 a = c[7];
  KZG_UNROLL_FULL
  for (int u = 6; u >= 0; u--) cellproof_chain(a, c[u], z);
  cells_reduce(a);
  fr_t v;
  f29_to_bn(v, a);
  KZG_UNROLL_FULL
  for (int q = 0; q < 8; q++) carry[q * CELLS_THREADS + t] = v.v[q];
}
// After a barrier: the carry T_s from the totals of the segments above (the same residue: threads t + 64, t + 128, ...), then the
// quotient's coefficients 512 s + 64 u + rho into the image (< 2r).  s is the same for a whole wave.
KZG_HD void cellproof_divide(uint32_t* img, const uint32_t* carry, const fr29 (&c)[8], const fr29& z, const fr29& z8, uint32_t t) {
  const uint32_t s = t >> 6, base = (s << 9) + (t & 63u);
  fr29 x;
  KZG_UNROLL_FULL
  for (int i = 0; i < F29_N; i++) x.l[i] = 0;
  for (uint32_t m = 7; m > s; m--) {
    fr_t v;
    KZG_UNROLL_FULL
    for (int q = 0; q < 8; q++) v.v[q] = carry[q * CELLS_THREADS + (t & 63u) + 64u * m];
    fr29 a;
    f29_from_bn(a, v);
    cellproof_chain(x, a, z8);
  }
  KZG_UNROLL_FULL
  for (int u = 7; u >= 0; u--) {
    if (u < 7) cellproof_chain(x, c[u + 1], z);
    fr29 o = x;
    cells_reduce(o);
    fr_t v;
    f29_to_bn(v, o);
    cells_put(img, base + 64u * (uint32_t)u, v);
  }
}

// entry e of the table: omega_128^e times 2^261, canonical, nine limbs padded to twelve dwords
KZG_HD void cellproof_tab_entry(uint32_t e, uint32_t* out) {
  fr_t g, acc = fr_one(), c261;
  {
    const uint32_t om[8] = KZG_FR_OMEGA8192_MONT, a[8] = KZG_FR_R261_PLAIN;
    KZG_UNROLL_FULL
    for (int q = 0; q < 8; q++) {
      g.v[q] = om[q];
      c261.v[q] = a[q];
    }
  }
  const uint32_t ge = 64u * (e & 127u);  // omega_128 = omega_8192^64
  for (int bit = 12; bit >= 0; bit--) {
    fr_sqr(acc, acc);
    if ((ge >> bit) & 1u) fr_mul(acc, acc, g);
  }
  fr_mul(acc, acc, c261);  // (v 2^256)(2^261) / 2^256 = v 2^261
  canonicalize<FrParams>(acc);
  fr29 o;
  f29_from_bn(o, acc);
  KZG_UNROLL_FULL
  for (int q = 0; q < F29_N; q++) out[q] = o.l[q];
  KZG_UNROLL_FULL
  for (int q = F29_N; q < CELLS_TAB_ENTRY; q++) out[q] = 0;
}

}  // namespace kzg
