// recover_cells (EIP-7594, recover_polynomialcoeff of specs/fulu/polynomial-commitments-sampling.md without its 8192-point transforms):
// the arithmetic of cell recovery, host and device.  No kernels here: cells_kernels.cuh (engine_proof.hip) runs these functions on a
// 512-thread workgroup with the image in LDS, setup_kernels.cuh (engine.hip) builds the tables with recover_tab_entry,
// tests/hostcpp/recover_ntt.cpp walks the same functions on the host.
//
// E is the flat cell set: E[j] = p(w^brp(j)) for j < 4096 (cells 0..63), E[4096 + j] = p(g w^brp(j)) (cells 64..127), w = omega_4096,
// g = omega_8192.  Every element x of cell c has x^64 = W_c = omega_128^brp7(c).  With M the set of missing cells,
//   Zs(y) = prod_{m in M} (y - W_m),  Z(x) = Zs(x^64),  Q = p Z (degree < 8192),  Q = Q_lo + x^4096 Q_hi:
//   prep    Z_c = Zs(W_c) for the 128 cells, and for the 64 runs u of the coset h D0 (h = 7, Y_u = h^64 omega_64^brp6(u))
//           P_u = prod_{c present} (Y_u - W_c) = (h^8192 - 1) / Zs(Y_u): the two products are y^128 - 1 together, and y^128 is h^8192 on
//           the whole coset -- so the division by Z on the coset is a product, and no inversion is needed anywhere
//   0..3    image = E[j] Z_c on cells 0..63 (0 where absent); inverse transform -> 4096 (Q_lo + Q_hi)_k = A_k, natural order.  Thread t
//           ends with k = t + 512 i and puts A away in the item's own output region (the STASH)
//   4..7    image = E[4096 + j] Z_c; inverse transform -> 4096 g^k (Q_lo - Q_hi)_k = B_k.  In step 7 the same thread holds the same k:
//           C_k = A_k h^k (1 + s) / 8192 + B_k (h / g)^k (1 - s) / 8192 = h^k (Q_lo + s Q_hi)_k,  s = h^4096,  and the forward pass follows
//   8..10   rest of the forward transform -> Q(h w^brp(j)), bit-reversed, j >> 6 = u
//   11..14  times P_u; inverse transform -> 4096 (h^8192 - 1) h^k p_k; times h^-k / (4096 (h^8192 - 1)) -> p_k; forward pass
//   15..17  rest of the forward transform -> E[0..4095], canonical
// then the caller compares and stores cells 0..63, runs cells_step 0..6 (E[4096..]) and compares and stores cells 64..127.  If the
// present elements are not the values of one polynomial of degree < 4096, the p of step 14 (degree < 4096 by construction) must differ
// from one of them: the comparison is exact in both directions.
// Arithmetic as in cells_math.cuh: plain data < 2r in the image, every table value times 2^261.
#pragma once
#include "cells_math.cuh"

namespace kzg {

constexpr int RECOVER_STEPS = 18;
constexpr uint32_t RECOVER_MIN_CELLS = 64;
// tables, 12-dword entries like compute_cells' (value * 2^261, canonical nine limbs):
//   [0, 4096)       h^k (1 + s) / 8192                   [4096, 8192)    (h / g)^k (1 - s) / 8192
//   [8192, 12288)   h^-k / (4096 (h^8192 - 1))           [12288, 12416)  W_c = omega_128^brp7(c)       [12416, 12480)  Y_u
constexpr uint32_t RECOVER_TAB_CA = 0, RECOVER_TAB_CB = 4096, RECOVER_TAB_UNTWIST = 8192, RECOVER_TAB_W = 12288, RECOVER_TAB_Y = 12416,
                   RECOVER_TAB_ENTRIES = 12480;
// Z_c (128) and P_u (64) of the item, nine limbs each (< 2r, normalised, times 2^261)
constexpr int RECOVER_ZS_Z = 0, RECOVER_ZS_P = 128, RECOVER_ZS_DWORDS = 192 * F29_N;

struct alignas(16) recover_quad {
  uint32_t x, y, z, w;
};
// 32 big-endian bytes at a 16-byte aligned address <-> eight little-endian words
KZG_HD void recover_ld(fr_t& v, const uint8_t* p) {
  const recover_quad* q = reinterpret_cast<const recover_quad*>(p);
  const recover_quad a = q[0], b = q[1];
  v.v[7] = __builtin_bswap32(a.x);
  v.v[6] = __builtin_bswap32(a.y);
  v.v[5] = __builtin_bswap32(a.z);
  v.v[4] = __builtin_bswap32(a.w);
  v.v[3] = __builtin_bswap32(b.x);
  v.v[2] = __builtin_bswap32(b.y);
  v.v[1] = __builtin_bswap32(b.z);
  v.v[0] = __builtin_bswap32(b.w);
}
KZG_HD void recover_st(uint8_t* p, const fr_t& v) {
  recover_quad* q = reinterpret_cast<recover_quad*>(p);
  q[0] = recover_quad{__builtin_bswap32(v.v[7]), __builtin_bswap32(v.v[6]), __builtin_bswap32(v.v[5]), __builtin_bswap32(v.v[4])};
  q[1] = recover_quad{__builtin_bswap32(v.v[3]), __builtin_bswap32(v.v[2]), __builtin_bswap32(v.v[1]), __builtin_bswap32(v.v[0])};
}

// mask: the item's 16 bytes as four little-endian words, bit c & 31 of word c >> 5 = cell c
KZG_HD bool recover_present(const uint32_t* mask, uint32_t c) { return (mask[c >> 5] >> (c & 31u)) & 1u; }
KZG_HD uint32_t recover_count(const uint32_t* mask) {
  return (uint32_t)(__builtin_popcount(mask[0]) + __builtin_popcount(mask[1]) + __builtin_popcount(mask[2]) + __builtin_popcount(mask[3]));
}

KZG_HD void recover_zs_get(fr29& w, const uint32_t* zs, uint32_t idx) {
  KZG_UNROLL_FULL
  for (int i = 0; i < F29_N; i++) w.l[i] = zs[idx * F29_N + i];
}
KZG_HD void recover_zs_put(uint32_t* zs, uint32_t idx, const fr29& w) {
  KZG_UNROLL_FULL
  for (int i = 0; i < F29_N; i++) zs[idx * F29_N + i] = w.l[i];
}
// acc *= (y - W_c); y and W_c canonical, acc < 2r normalised: the difference is < 3r with limbs < 2^31
KZG_HD void recover_factor(fr29& acc, const fr29& y, const uint32_t* rtab, uint32_t c) {
  fr29 w, d;
  cells_tw(w, rtab, RECOVER_TAB_W + c);
  f29_sub_2r(d, y, w);
  f29_mul(acc, acc, d);
  cells_fence();
}

// Prep, first half: thread t's partial product into part[9 t ..] (the image is free and serves as `part`).  Threads 128 q + c take the
// missing cells 32 q .. 32 q + 31 of Z_c, then threads 64 q + u the present cells 16 q .. 16 q + 15 of P_u: a wave has one q, so its
// lanes agree on every cell they skip.
KZG_HD void recover_prep_partial(uint32_t* part, const uint32_t* rtab, const uint32_t* mask, uint32_t t) {
  fr29 y, acc;
  {
    const uint32_t c = t & 127u, q = t >> 7;
    cells_tw(y, rtab, RECOVER_TAB_W + c);
    cells_tw(acc, rtab, RECOVER_TAB_W);  // W_0 = 1
    const uint32_t bits = ~mask[q];
    for (uint32_t j = 0; j < 32; j++)
      if ((bits >> j) & 1u) recover_factor(acc, y, rtab, 32u * q + j);
    recover_zs_put(part, t, acc);
  }
  {
    const uint32_t u = t & 63u, q = t >> 6;
    cells_tw(y, rtab, RECOVER_TAB_Y + u);
    cells_tw(acc, rtab, RECOVER_TAB_W);
    const uint32_t bits = (mask[q >> 1] >> (16u * (q & 1u))) & 0xffffu;
    for (uint32_t j = 0; j < 16; j++)
      if ((bits >> j) & 1u) recover_factor(acc, y, rtab, 16u * q + j);
    recover_zs_put(part, 512u + t, acc);
  }
}
// Prep, second half (after a barrier): threads 0..127 multiply the four parts of Z_c, threads 128..191 the eight parts of P_u
KZG_HD void recover_prep_combine(uint32_t* zs, const uint32_t* part, uint32_t t) {
  if (t >= 192u) return;
  const bool z = t < 128u;
  const uint32_t first = z ? t : 512u + (t - 128u), stride = z ? 128u : 64u, parts = z ? 4u : 8u;
  fr29 acc, f;
  recover_zs_get(acc, part, first);
  for (uint32_t q = 1; q < parts; q++) {
    recover_zs_get(f, part, first + q * stride);
    f29_mul(acc, acc, f);
    cells_fence();
  }
  recover_zs_put(zs, t, acc);
}

// image = the present elements of cells 64 half .. 64 half + 63 times Z_c, zero where the cell is absent -- an absent cell's bytes are
// not read.  Returns whether one of this thread's present elements is >= r.  `map` (cells_math.cuh) says where a byte of the item lies
// from `cells` on: a wave's 64 lanes read one cell, 2 KiB in a row under either map.
template <class Map = cells_blob_major>
KZG_HD bool recover_load_half(uint32_t* img, const uint32_t* zs, const uint8_t* cells, const uint32_t* mask, uint32_t t, uint32_t half, const Map map = Map()) {
  bool bad = false;
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    const uint32_t e = (uint32_t)i * CELLS_THREADS + t, c = 64u * half + (e >> 6);
    fr_t v;
    KZG_UNROLL_FULL
    for (int q = 0; q < 8; q++) v.v[q] = 0;
    if (recover_present(mask, c)) {
      recover_ld(v, cells + map(((size_t)half * 4096u + e) * 32u));
      bad |= !fr_is_canonical(v);
      fr29 x, w;
      f29_from_bn(x, v);
      recover_zs_get(w, zs, RECOVER_ZS_Z + c);
      f29_mul(x, x, w);
      cells_fence();
      f29_to_bn(v, x);
    }
    cells_put(img, e, v);
  }
  return bad;
}

// the image (canonical) -> cells 64 half .. of `out`; returns whether it differs from one of this thread's present elements.  `map`
// goes with `cells` and with `out` alike.
template <class Map = cells_blob_major>
KZG_HD bool recover_store_half(const uint32_t* img, const uint8_t* cells, uint8_t* out, const uint32_t* mask, uint32_t t, uint32_t half, const Map map = Map()) {
  uint32_t diff = 0;
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    const uint32_t e = (uint32_t)i * CELLS_THREADS + t, c = 64u * half + (e >> 6);
    const size_t at = ((size_t)half * 4096u + e) * 32u;
    fr_t v;
    cells_get(v, img, e);
    if (recover_present(mask, c)) {
      fr_t u;
      recover_ld(u, cells + map(at));
      KZG_UNROLL_FULL
      for (int q = 0; q < 8; q++) diff |= u.v[q] ^ v.v[q];
    }
    recover_st(out + map(at), v);
  }
  return diff != 0;
}

// the eight words of the stash's piece e
template <class Map>
KZG_HD uint32_t* recover_stash_piece(uint32_t* stash, uint32_t e, const Map map) {
  return stash + map((size_t)e * 32u) / 4u;
}
// Step k = 0..17 of thread t (the list at the top).  Like cells_step it reads and writes the thread's own eight elements of the image,
// so one barrier between steps is enough; `stash` is 131,072 bytes of global memory that only steps 3 (write) and 7 (read) touch, each
// thread its own 8 x 32 bytes.  The stash is cells 0..63 of the item's own output under `map`: piece e is the 32 bytes at offset 32 e
// of the item, inside cell e >> 6, so under the column map it is row `row` of the output matrix's first 64 columns -- no two threads
// share a piece, and none leaves the item's own cells.
template <class Map = cells_blob_major>
KZG_HD void recover_step(uint32_t* img, const uint32_t* zs, uint32_t* stash, const uint32_t* tab, const uint32_t* rtab, uint32_t t, int k, const Map map = Map()) {
  const bool inv = k <= 7 || (k >= 11 && k <= 14), fwd = (k >= 7 && k <= 10) || k >= 14;
  const int p = k <= 3 ? k : (k <= 7 ? k - 4 : (k <= 10 ? 10 - k : (k <= 14 ? k - 11 : 17 - k)));
  const uint32_t sh = 3u * (uint32_t)p, S = 1u << sh;
  const uint32_t low = t & (S - 1u), base = ((t >> sh) << (sh + 3)) + low;
  const uint32_t tw = S - 1u + low;
  fr29 x[8];
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    fr_t v;
    cells_get(v, img, base + ((uint32_t)i << sh));
    f29_from_bn(x[i], v);
  }
  if (k == 11) {  // p = 0: elements 8 t + i, run u = t >> 3
    fr29 w;
    recover_zs_get(w, zs, RECOVER_ZS_P + (t >> 3));
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) {
      f29_mul(x[i], x[i], w);
      cells_fence();
    }
  }
  if (inv) {
    cells_pass_inv(x, tab, CELLS_TAB_INV + tw, S);
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) cells_reduce(x[i]);
  }
  if (k == 3) {
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) {
      fr_t v;
      f29_to_bn(v, x[i]);
      uint32_t* s = static_cast<uint32_t*>(__builtin_assume_aligned(recover_stash_piece(stash, base + ((uint32_t)i << sh), map), 16));
      KZG_UNROLL_FULL
      for (int q = 0; q < 8; q++) s[q] = v.v[q];
    }
    return;
  }
  if (k == 7) {
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) {
      const uint32_t e = base + ((uint32_t)i << sh);
      const uint32_t* s = static_cast<const uint32_t*>(__builtin_assume_aligned(recover_stash_piece(stash, e, map), 16));
      fr_t v;
      KZG_UNROLL_FULL
      for (int q = 0; q < 8; q++) v.v[q] = s[q];
      fr29 a, w;
      cells_tw(w, rtab, RECOVER_TAB_CB + e);
      f29_mul(x[i], x[i], w);
      cells_fence();
      f29_from_bn(a, v);
      cells_tw(w, rtab, RECOVER_TAB_CA + e);
      f29_mul(a, a, w);
      f29_add(x[i], x[i], a);  // < 4r, limbs < 2^30
      cells_reduce(x[i]);
      cells_fence();
    }
  }
  if (k == 14) {
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) {
      fr29 w;
      cells_tw(w, rtab, RECOVER_TAB_UNTWIST + base + ((uint32_t)i << sh));
      f29_mul(x[i], x[i], w);
      cells_fence();
    }
  }
  if (fwd) {
    cells_pass_fwd(x, tab, CELLS_TAB_FWD + tw, S);
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) cells_reduce(x[i]);
  }
  uint32_t at = base;  // on the device the eight slots are computed again, not kept in registers through the passes
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(at));
#endif
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    fr_t v;
    f29_to_bn(v, x[i]);
    if (k == RECOVER_STEPS - 1) canonicalize<FrParams>(v);
    cells_put(img, at + ((uint32_t)i << sh), v);
  }
}

// entry idx of the tables, built like cells_tab_entry
KZG_HD void recover_tab_entry(uint32_t idx, uint32_t* out) {
  auto constant = [](fr_t& r, const uint32_t (&c)[8]) {
    KZG_UNROLL_FULL
    for (int q = 0; q < 8; q++) r.v[q] = c[q];
  };
  auto power = [](fr_t& r, const fr_t& b, uint32_t e) {  // e < 2^13
    fr_t acc = fr_one();
    for (int bit = 12; bit >= 0; bit--) {
      fr_sqr(acc, acc);
      if ((e >> bit) & 1u) fr_mul(acc, acc, b);
    }
    r = acc;
  };
  auto brp = [](uint32_t v, int bits) {
    uint32_t o = 0;
    for (int i = 0; i < bits; i++) o |= ((v >> i) & 1u) << (bits - 1 - i);
    return o;
  };
  const uint32_t om[8] = KZG_FR_OMEGA8192_MONT, ch[8] = KZG_FR_RECOVER_H_MONT, chinv[8] = KZG_FR_RECOVER_HINV_MONT, ca[8] = KZG_FR_RECOVER_CA_MONT,
                 cb[8] = KZG_FR_RECOVER_CB_MONT, cu[8] = KZG_FR_RECOVER_CU_MONT, cy[8] = KZG_FR_RECOVER_H64_MONT, a261[8] = KZG_FR_R261_PLAIN;
  fr_t g, b = fr_one(), f = fr_one(), c261;
  uint32_t e = 0, ge = 0;  // b^e g^ge f
  constant(g, om);
  constant(c261, a261);
  if (idx < RECOVER_TAB_CB) {
    constant(b, ch);
    constant(f, ca);
    e = idx;
  } else if (idx < RECOVER_TAB_UNTWIST) {
    constant(b, ch);
    constant(f, cb);
    e = idx - RECOVER_TAB_CB;
    ge = (8192u - e) & 8191u;
  } else if (idx < RECOVER_TAB_W) {
    constant(b, chinv);
    constant(f, cu);
    e = idx - RECOVER_TAB_UNTWIST;
  } else if (idx < RECOVER_TAB_Y) {
    ge = 64u * brp(idx - RECOVER_TAB_W, 7);
  } else {
    constant(f, cy);
    ge = 128u * brp(idx - RECOVER_TAB_Y, 6);
  }
  fr_t acc, gp;
  power(acc, b, e);
  power(gp, g, ge);
  fr_mul(acc, acc, gp);
  fr_mul(acc, acc, f);
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
