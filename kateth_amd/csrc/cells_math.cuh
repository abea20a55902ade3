// compute_cells (EIP-7594, specs/fulu/polynomial-commitments-sampling.md): the arithmetic of the blob extension, host and device.
// No kernels here: cells_kernels.cuh (engine_proof.hip) runs cells_step on a 512-thread workgroup with the image in LDS,
// setup_kernels.cuh (engine.hip) builds the twiddle table with cells_tab_entry, tests/hostcpp/cells_ntt.cpp walks the same steps on
// the host.
//
// The blob holds the evaluations of p (degree < 4096) at roots_brp[j] = w^brp(j), w = omega_4096.  The extension half of the result is
// E[4096 + j] = p(g w^brp(j)) with g = omega_8192 = 7^((r-1)/8192), g^2 = w.  With the blob as it lies in memory:
//   1. decimation-in-time inverse transform with w^-1: bit-reversed in, natural out -> 4096 c_k
//   2. c_k *= g^k / 4096
//   3. decimation-in-frequency forward transform with w: natural in, bit-reversed out = the extension half in the output's order
// Both transforms are twelve radix-2 stages taken three at a time: a PASS of stride S = 8^p (p = 0..3) gives thread t the eight
// elements base + i S (low = t mod S, base = 8 S (t div S) + low) and runs the stages of half-size S, 2S, 4S on them in registers.
// The inverse transform takes the passes p = 0..3, the forward transform p = 3..0, and the two passes at p = 3 (with the twist between
// them) work on the same eight elements: SEVEN steps with a barrier after each, one image round trip per step.
//
// Arithmetic: radix-2^29 limbs (fr29.cuh).  The data stays PLAIN, every twiddle is stored times 2^261: f29_mul(x, w 2^261) = x w,
// so nothing is ever converted to or from Montgomery form.  Additions carry nothing; the bounds (in units of r, limbs in parentheses):
//   inverse pass, inputs < 2 (normalised):  v = x w < 2 (2^29), u + v, u + 4r - v: a stage adds at most 4 (2^30) -- after three stages
//     < 14 (3.5 x 2^30), and the operand of the third stage's product < 10 (2.5 x 2^30 < the product's limit 3.05 x 2^30)
//   forward pass, inputs < 2 (normalised):  u + v carry-passed at once, so every stage sees normalised inputs < 2, 4, 8;
//     (u + 16r - v) < 24 (1.5 x 2^30) goes into the product; the sums end < 16
//   cells_reduce brings everything below 2 again (normalised) before it is packed into 8 x 32 bits or multiplied by the twist.
// The CPU build with KZG_FP28_CHECK re-checks every limb operation at run time (rdx_mont.cuh).
#pragma once
#include "fr29.cuh"

namespace kzg {

constexpr int CELLS_THREADS = 512;         // x 8 elements = one blob
constexpr int CELLS_STEPS = 7;
constexpr int CELLS_IMAGE_DWORDS = 8 * 4096;  // the blob as eight word planes of 4096 dwords: 131,072 B
// twiddle table: 12-dword entries (nine limbs of value * 2^261, canonical; three 16-byte loads)
//   [0, 4095)        inverse passes: entry (S - 1) + slot S + low of the pass of stride S
//   [4096, 8191)     forward passes, same order
//   [8192, 12288)    twist g^k / 4096
// slots of a pass (x = exponent of w, negated for the inverse):  0: stage S, x = low 2048/S;  1 + b: stage 2S, x = (low + b S) 1024/S;
// 3 + q: stage 4S, x = (low + q S) 512/S
constexpr int CELLS_TAB_ENTRY = 12;
constexpr uint32_t CELLS_TAB_INV = 0, CELLS_TAB_FWD = 4096, CELLS_TAB_TWIST = 8192, CELLS_TAB_ENTRIES = 12288;

#define KZG_CELLS_TABLE(fn, MACRO)        \
  KZG_HD constexpr uint32_t fn(int i) {   \
    constexpr uint32_t t[F29_N] = MACRO;  \
    return t[i];                          \
  }
KZG_CELLS_TABLE(cells_4r_t1, KZG_FR29_4R_T1)
KZG_CELLS_TABLE(cells_16r_t1, KZG_FR29_16R_T1)
KZG_CELLS_TABLE(cells_neg_mod, KZG_FR29_NEG_MOD)
#undef KZG_CELLS_TABLE

// Where byte `at` of an item's 262,144-byte cell set lies, as an offset from the pointer the map goes with.  Blob-major (the cell
// calls): the pointer is the item's own cell set and the offset is `at`.  Column-major (the data column calls): the pointer is a
// column matrix of `rows` rows -- the cell of column c, row b at 2048 (c rows + b) -- and the item is row `row` of it.  A piece that
// does not cross a cell boundary (every 16- and 32-byte piece the kernels move) stays in one run of bytes under either map.
struct cells_blob_major {
  KZG_HD size_t operator()(size_t at) const { return at; }
};
struct cells_column_major {
  uint64_t rows, row;
  KZG_HD size_t operator()(size_t at) const {
    uint32_t cell = (uint32_t)(at >> 11);
#if defined(__HIP_DEVICE_COMPILE__)
    // Every phase that moves cells has the 64 lanes of a wave inside ONE cell (tests/hostcpp/datacolumns_addr.cpp walks them all), so
    // the column's base is scalar arithmetic and the lanes differ in the low eleven bits only: the accesses are as coalesced as
    // blob-major ones, and no strided address is kept in vector registers.
    cell = __builtin_amdgcn_readfirstlane(cell);
#endif
    return (size_t)(((uint64_t)cell * rows + row) << 11) + (at & 2047u);
  }
};
// the same for proofs: the 48 bytes of (cell c, row b) of a column matrix of proofs
KZG_HD size_t proofs_column_at(uint64_t rows, uint64_t row, uint32_t cell) { return (size_t)((uint64_t)cell * rows + row) * 48u; }

// Dword index of element e in a word plane.  A 32-lane group of ds_read_b32 / ds_write_b32 is conflict-free when its indices differ
// mod 32; the lanes of a group vary bits 3..7 of e at stride 1, bits 0..2 and 6..7 at stride 8, bits 0..4 at strides 64 and 512 and in
// the coalesced load and store -- folding bits 5..7 onto bits 0..2 and bits 6..7 onto bits 3..4 makes all of them 32 different banks.
KZG_HD uint32_t cells_slot(uint32_t e) { return e ^ ((e >> 5) & 7u) ^ (((e >> 6) & 3u) << 3); }

KZG_HD void cells_put(uint32_t* img, uint32_t e, const fr_t& v) {
  const uint32_t s = cells_slot(e);
  KZG_UNROLL_FULL
  for (int q = 0; q < 8; q++) img[q * 4096 + s] = v.v[q];
}
KZG_HD void cells_get(fr_t& v, const uint32_t* img, uint32_t e) {
  const uint32_t s = cells_slot(e);
  KZG_UNROLL_FULL
  for (int q = 0; q < 8; q++) v.v[q] = img[q * 4096 + s];
}

KZG_HD void cells_tw(fr29& w, const uint32_t* tab, uint32_t idx) {
  const uint32_t* p = static_cast<const uint32_t*>(__builtin_assume_aligned(tab + (size_t)idx * CELLS_TAB_ENTRY, 16));
  KZG_UNROLL_FULL
  for (int i = 0; i < F29_N; i++) w.l[i] = p[i];
}

// limbs < 2^32, value < 2^261 -> limbs 0..7 < 2^29, the top limb whatever the value leaves
KZG_HD void cells_carry(fr29& a) {
  KZG_UNROLL_FULL
  for (int i = 0; i + 1 < F29_N; i++) {
    RDX_ADDCHK(a.l[i + 1], a.l[i] >> F29_W);
    a.l[i + 1] += a.l[i] >> F29_W;
    a.l[i] &= F29_MASK;
  }
}

// limbs < 2^32, value < 64 r -> strictly normalised, value < 2r.  q = (top limb x floor(2^32 / (r >> 232 + 1))) >> 32 never exceeds
// x / r and falls short of it by less than 1.04 (the carries still waiting in the lower limbs are worth < 2^-19 r); x - q r is formed
// as x + q (2^261 - r), whose carry out of 261 bits is q itself and is dropped with the top limb's mask.
KZG_HD void cells_reduce(fr29& a) {
  const uint32_t q = (uint32_t)(((uint64_t)a.l[F29_N - 1] * KZG_FR29_TOP_RECIP) >> 32);
  uint64_t acc = 0;
  KZG_UNROLL_FULL
  for (int i = 0; i < F29_N; i++) {
    acc += (uint64_t)a.l[i] + (uint64_t)q * cells_neg_mod(i);
    a.l[i] = (uint32_t)acc & F29_MASK;
    acc >>= F29_W;
  }
#if !defined(__HIP_DEVICE_COMPILE__) && defined(KZG_FP28_CHECK)
  if (acc != q) kzg_fp28_check_failed("cells_reduce: quotient estimate out of range");
#endif
}

// Between two butterflies on the device: neither the scheduler nor the optimiser may move code across.  A stage's products are
// independent and the step's twiddle loads can all be hoisted; left alone the compiler does both and k_compute_cells spills (8 bytes of
// scratch per lane at 256 VGPRs); with one product's temporaries live at a time it does not.
KZG_HD void cells_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#endif
}

// decimation in time: (u, x) -> (u + x w, u - x w)
KZG_HD void cells_dit(fr29& lo, fr29& hi, const fr29& w) {
  fr29 v;
  f29_mul(v, hi, w);
  KZG_UNROLL_FULL
  for (int i = 0; i < F29_N; i++) {
    RDX_SUBCHK(lo.l[i], cells_4r_t1(i), v.l[i]);
    RDX_ADDCHK(lo.l[i], v.l[i]);
    hi.l[i] = lo.l[i] + cells_4r_t1(i) - v.l[i];
    lo.l[i] = lo.l[i] + v.l[i];
  }
  cells_fence();
}
// decimation in frequency: (u, v) -> (u + v, (u - v) w); u, v normalised, < 8r
KZG_HD void cells_dif(fr29& lo, fr29& hi, const fr29& w) {
  fr29 d;
  KZG_UNROLL_FULL
  for (int i = 0; i < F29_N; i++) {
    RDX_SUBCHK(lo.l[i], cells_16r_t1(i), hi.l[i]);
    d.l[i] = lo.l[i] + cells_16r_t1(i) - hi.l[i];
    lo.l[i] = lo.l[i] + hi.l[i];
  }
  cells_carry(lo);
  f29_mul(hi, d, w);
  cells_fence();
}

// the three stages of a pass on a thread's eight elements; tw = index of the pass's slot 0 for this thread, S = the pass's stride
KZG_HD void cells_pass_inv(fr29 (&x)[8], const uint32_t* tab, uint32_t tw, uint32_t S) {
  fr29 w;
  cells_tw(w, tab, tw);
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i += 2) cells_dit(x[i], x[i + 1], w);
  KZG_UNROLL_FULL
  for (int b = 0; b < 2; b++) {
    cells_tw(w, tab, tw + (1 + b) * S);
    cells_dit(x[b], x[b + 2], w);
    cells_dit(x[b + 4], x[b + 6], w);
  }
  KZG_UNROLL_FULL
  for (int q = 0; q < 4; q++) {
    cells_tw(w, tab, tw + (3 + q) * S);
    cells_dit(x[q], x[q + 4], w);
  }
}
KZG_HD void cells_pass_fwd(fr29 (&x)[8], const uint32_t* tab, uint32_t tw, uint32_t S) {
  fr29 w;
  KZG_UNROLL_FULL
  for (int q = 0; q < 4; q++) {
    cells_tw(w, tab, tw + (3 + q) * S);
    cells_dif(x[q], x[q + 4], w);
  }
  KZG_UNROLL_FULL
  for (int b = 0; b < 2; b++) {
    cells_tw(w, tab, tw + (1 + b) * S);
    cells_dif(x[b], x[b + 2], w);
    cells_dif(x[b + 4], x[b + 6], w);
  }
  cells_tw(w, tab, tw);
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i += 2) cells_dif(x[i], x[i + 1], w);
}

// Step k = 0..6 of thread t on the image: k = 0..2 inverse passes p = k; k = 3: inverse pass, twist and forward pass at p = 3;
// k = 4..6 forward passes p = 6 - k.  A step reads and writes the thread's own eight elements only, so the workgroup needs one
// barrier between steps and none inside.  The image holds values < 2r in 8 x 32 bits; the last step leaves them canonical.
KZG_HD void cells_step(uint32_t* img, const uint32_t* tab, uint32_t t, int k) {
  const int p = k <= 3 ? k : 6 - k;
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
  if (k <= 3) {
    cells_pass_inv(x, tab, CELLS_TAB_INV + tw, S);
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) cells_reduce(x[i]);
  }
  if (k == 3) {
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) {
      fr29 w;
      cells_tw(w, tab, CELLS_TAB_TWIST + base + ((uint32_t)i << sh));
      f29_mul(x[i], x[i], w);
      cells_fence();
    }
  }
  if (k >= 3) {
    cells_pass_fwd(x, tab, CELLS_TAB_FWD + tw, S);
    KZG_UNROLL_FULL
    for (int i = 0; i < 8; i++) cells_reduce(x[i]);
  }
  KZG_UNROLL_FULL
  for (int i = 0; i < 8; i++) {
    fr_t v;
    f29_to_bn(v, x[i]);
    if (k == CELLS_STEPS - 1) canonicalize<FrParams>(v);
    cells_put(img, base + ((uint32_t)i << sh), v);
  }
}

// entry idx of the twiddle table: g^e (times 1/4096 for the twist) times 2^261, canonical, nine limbs padded to twelve dwords
KZG_HD void cells_tab_entry(uint32_t idx, uint32_t* out) {
  uint32_t e;  // exponent of g = omega_8192
  const bool twist = idx >= CELLS_TAB_TWIST;
  if (twist) {
    e = idx - CELLS_TAB_TWIST;
  } else {
    const bool fwd = idx >= CELLS_TAB_FWD;
    const uint32_t j = idx - (fwd ? CELLS_TAB_FWD : CELLS_TAB_INV);
    const uint32_t sh = j < 7u ? 0u : (j < 63u ? 3u : (j < 511u ? 6u : 9u)), S = 1u << sh;
    const uint32_t off = j - (S - 1u), slot = off >> sh, low = off & (S - 1u);
    uint32_t x;  // exponent of w = g^2
    if (slot == 0)
      x = low * (2048u >> sh);
    else if (slot < 3)
      x = (low + (slot - 1u) * S) * (1024u >> sh);
    else
      x = (low + (slot - 3u) * S) * (512u >> sh);
    e = fwd ? 2u * x : (8192u - 2u * x) & 8191u;
    if (j >= 4095u) e = 0;  // the unused entry between the tables
  }
  fr_t g, acc = fr_one(), c261;
  {
    const uint32_t om[8] = KZG_FR_OMEGA8192_MONT, a[8] = KZG_FR_R261_PLAIN;
    KZG_UNROLL_FULL
    for (int q = 0; q < 8; q++) {
      g.v[q] = om[q];
      c261.v[q] = a[q];
    }
  }
  for (int bit = 12; bit >= 0; bit--) {
    fr_sqr(acc, acc);
    if ((e >> bit) & 1u) fr_mul(acc, acc, g);
  }
  if (twist) {
    fr_t f;
    const uint32_t c4096[8] = KZG_FR_INV4096_MONT;
    KZG_UNROLL_FULL
    for (int q = 0; q < 8; q++) f.v[q] = c4096[q];
    fr_mul(acc, acc, f);
  }
  fr_mul(acc, acc, c261);  // (v 2^256)(2^261) / 2^256 = v 2^261
  fr29 o;
  f29_from_bn(o, acc);
  KZG_UNROLL_FULL
  for (int q = 0; q < F29_N; q++) out[q] = o.l[q];
  KZG_UNROLL_FULL
  for (int q = F29_N; q < CELLS_TAB_ENTRY; q++) out[q] = 0;
}

}  // namespace kzg
