// TEST-ONLY: one case of a radix-2^28 / radix-2^29 operation, limbs in and limbs out, as ONE inline function that both the device
// harness (device_atoms28.hip: one case per lane) and the CPU build under the 128-bit column check (tests/hostmath/shim.cpp: a loop
// over the cases) instantiate -- so that the two sides cannot disagree about what an op number means.  Nothing of the product is
// copied: every op calls the product's own inline functions of fp28.cuh, fr29.cuh and g1_decode28.cuh.  The includer has included
// those headers.  The Python side of the op numbers and layouts is tests/fp28_cases.py.
#pragma once

namespace atoms28 {
using namespace kzg;

constexpr int L28 = F28_N, L29 = F29_N;
constexpr int ACC_WORDS = 4 * L28 + 1;  // x, y, zz, zzz, inf
constexpr int JAC_WORDS = 3 * L28 + 1;  // x, y, z, inf
constexpr int ENTRY_WORDS = 2 * L28;    // x2, y2

template <class T>
KZG_HD void ld(T& r, const uint32_t* p) {
  KZG_UNROLL_FULL
  for (int i = 0; i < (int)(sizeof(T) / 4); i++) r.l[i] = p[i];
}
template <class T>
KZG_HD void st(uint32_t* p, const T& a) {
  KZG_UNROLL_FULL
  for (int i = 0; i < (int)(sizeof(T) / 4); i++) p[i] = a.l[i];
}

// ---- fp28: four operands of 14 limbs in, two results of 14 limbs out ----------------------------------------------------------
enum {
  F28_MUL = 0, F28_SQR = 1, F28_MUL2 = 2,
  // the result ALIASES an operand, as the call sites do
  F28_ALIAS_MUL_A = 3,    // f28_mul(a, a, b)          p.zz = p.zz * pp
  F28_ALIAS_MUL_B = 4,    // f28_mul(b, a, b)          pp = p.x * pp ; T = A * T
  F28_ALIAS_MUL2_C = 5,   // f28_mul2(c, a, b, c, d)   p.y = r * pp + p.y * ppp
  F28_ALIAS_MUL2_D = 6,   // f28_mul2(d, a, b, c, d)   p.y = m * t + nw * p.y
  F28_ALIAS_SQR = 7,      // f28_sqr(a, a)             the square root's runs of squarings
  F28_SUB_4P = 10, F28_SUB_16P = 11, F28_SUB_8P3 = 12, F28_NEG_2P = 13, F28_NEG_4P = 14, F28_ADD = 15,
  F28_CARRY = 16, F28_NORMALIZE = 17,
  F28_ZERO_TESTS = 18,    // result 0 = {f28_maybe_zero, f28_is_zero_exact, f28_is_zero}(a)
  F28_TO_FP = 19,         // result 0 = 12 words
  F28_FROM_BN = 20,       // a = 12 words
  F28_TO_BN = 21,         // result 0 = 12 words (a strictly normalised)
  F28_R392 = 22,          // a = 12 words (canonical x * 2^384): result 0 = fp_to_r392 as 12 words
  F28_LOAD_ENTRY = 23,    // a, b = 12 words each, c.l[0] = neg: results x, y
};
#define ATOMS28_F28_OPS(X)                                                                                                          \
  X(F28_MUL) X(F28_SQR) X(F28_MUL2) X(F28_ALIAS_MUL_A) X(F28_ALIAS_MUL_B) X(F28_ALIAS_MUL2_C) X(F28_ALIAS_MUL2_D) X(F28_ALIAS_SQR)  \
  X(F28_SUB_4P) X(F28_SUB_16P) X(F28_SUB_8P3) X(F28_NEG_2P) X(F28_NEG_4P) X(F28_ADD) X(F28_CARRY) X(F28_NORMALIZE)                  \
  X(F28_ZERO_TESTS) X(F28_TO_FP) X(F28_FROM_BN) X(F28_TO_BN) X(F28_R392) X(F28_LOAD_ENTRY)

template <int OP>
KZG_HD void f28_case(const uint32_t* in, uint32_t* out) {
  fp28 o[4], r0, r1;
  KZG_UNROLL_FULL
  for (int k = 0; k < 4; k++) ld(o[k], in + k * L28);
  KZG_UNROLL_FULL
  for (int k = 0; k < L28; k++) r0.l[k] = r1.l[k] = 0;
  fp_t w0, w1;
  KZG_UNROLL_FULL
  for (int k = 0; k < 12; k++) {
    w0.v[k] = o[0].l[k];
    w1.v[k] = o[1].l[k];
  }
  if constexpr (OP == F28_MUL) f28_mul(r0, o[0], o[1]);
  if constexpr (OP == F28_SQR) f28_sqr(r0, o[0]);
  if constexpr (OP == F28_MUL2) f28_mul2(r0, o[0], o[1], o[2], o[3]);
  if constexpr (OP == F28_ALIAS_MUL_A) {
    f28_mul(o[0], o[0], o[1]);
    r0 = o[0];
  }
  if constexpr (OP == F28_ALIAS_MUL_B) {
    f28_mul(o[1], o[0], o[1]);
    r0 = o[1];
  }
  if constexpr (OP == F28_ALIAS_MUL2_C) {
    f28_mul2(o[2], o[0], o[1], o[2], o[3]);
    r0 = o[2];
  }
  if constexpr (OP == F28_ALIAS_MUL2_D) {
    f28_mul2(o[3], o[0], o[1], o[2], o[3]);
    r0 = o[3];
  }
  if constexpr (OP == F28_ALIAS_SQR) {
    f28_sqr(o[0], o[0]);
    r0 = o[0];
  }
  if constexpr (OP == F28_SUB_4P) f28_sub_4p(r0, o[0], o[1]);
  if constexpr (OP == F28_SUB_16P) f28_sub_16p(r0, o[0], o[1]);
  if constexpr (OP == F28_SUB_8P3) f28_sub_8p3(r0, o[0], o[1]);
  if constexpr (OP == F28_NEG_2P) f28_neg_2p(r0, o[0]);
  if constexpr (OP == F28_NEG_4P) f28_neg_4p(r0, o[0]);
  if constexpr (OP == F28_ADD) f28_add(r0, o[0], o[1]);
  if constexpr (OP == F28_CARRY) {
    r0 = o[0];
    f28_carry_pass(r0);
  }
  if constexpr (OP == F28_NORMALIZE) {
    r0 = o[0];
    f28_normalize(r0);
  }
  if constexpr (OP == F28_ZERO_TESTS) {
    r0.l[0] = f28_maybe_zero(o[0]) ? 1 : 0;
    r0.l[1] = f28_is_zero_exact(o[0]) ? 1 : 0;
    r0.l[2] = f28_is_zero(o[0]) ? 1 : 0;
  }
  if constexpr (OP == F28_TO_FP) {
    fp_t v;
    f28_to_fp(v, o[0]);
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) r0.l[k] = v.v[k];
  }
  if constexpr (OP == F28_FROM_BN) f28_from_bn(r0, w0);
  if constexpr (OP == F28_TO_BN) {
    fp_t v;
    f28_to_bn(v, o[0]);
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) r0.l[k] = v.v[k];
  }
  if constexpr (OP == F28_R392) {
    fp_t v;
    fp_to_r392(v, w0);
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) r0.l[k] = v.v[k];
  }
  if constexpr (OP == F28_LOAD_ENTRY) f28_load_entry(r0, r1, w0, w1, o[2].l[0] != 0);
  st(out, r0);
  st(out + L28, r1);
}

// ---- fr29: four operands of 9 limbs in, two results of 9 limbs out -------------------------------------------------------------
enum {
  F29_MUL = 0, F29_SQR = 1, F29_MUL2 = 2, F29_ALIAS_MUL_A = 3, F29_ALIAS_MUL2_A = 4,  // f29_mul(a, a, b); f29_mul2(a, a, b, c, d): N = N d16 + H D
  F29_ADD = 10, F29_SUB_2R = 11, F29_TO_MONT = 12,
  F29_ZERO_TESTS = 13,    // result 0 = {f29_maybe_zero, f29_is_zero_exact}(a)
  F29_FROM_BN = 14,       // a = 8 words
  F29_TO_BN = 15,         // result 0 = 8 words (a strictly normalised, < 2^256)
  F29_TO_CANONICAL = 16,  // result 0 = 8 words (a N-form)
};
#define ATOMS28_F29_OPS(X)                                                                                              \
  X(F29_MUL) X(F29_SQR) X(F29_MUL2) X(F29_ALIAS_MUL_A) X(F29_ALIAS_MUL2_A) X(F29_ADD) X(F29_SUB_2R) X(F29_TO_MONT)      \
  X(F29_ZERO_TESTS) X(F29_FROM_BN) X(F29_TO_BN) X(F29_TO_CANONICAL)

template <int OP>
KZG_HD void f29_case(const uint32_t* in, uint32_t* out) {
  fr29 o[4], r0, r1;
  KZG_UNROLL_FULL
  for (int k = 0; k < 4; k++) ld(o[k], in + k * L29);
  KZG_UNROLL_FULL
  for (int k = 0; k < L29; k++) r0.l[k] = r1.l[k] = 0;
  if constexpr (OP == F29_MUL) f29_mul(r0, o[0], o[1]);
  if constexpr (OP == F29_SQR) f29_sqr(r0, o[0]);
  if constexpr (OP == F29_MUL2) f29_mul2(r0, o[0], o[1], o[2], o[3]);
  if constexpr (OP == F29_ALIAS_MUL_A) {
    f29_mul(o[0], o[0], o[1]);
    r0 = o[0];
  }
  if constexpr (OP == F29_ALIAS_MUL2_A) {
    f29_mul2(o[0], o[0], o[1], o[2], o[3]);
    r0 = o[0];
  }
  if constexpr (OP == F29_ADD) f29_add(r0, o[0], o[1]);
  if constexpr (OP == F29_SUB_2R) f29_sub_2r(r0, o[0], o[1]);
  if constexpr (OP == F29_TO_MONT) f29_to_mont(r0, o[0]);
  if constexpr (OP == F29_ZERO_TESTS) {
    r0.l[0] = f29_maybe_zero(o[0]) ? 1 : 0;
    r0.l[1] = f29_is_zero_exact(o[0]) ? 1 : 0;
  }
  if constexpr (OP == F29_FROM_BN) {
    fr_t v;
    KZG_UNROLL_FULL
    for (int k = 0; k < 8; k++) v.v[k] = o[0].l[k];
    f29_from_bn(r0, v);
  }
  if constexpr (OP == F29_TO_BN || OP == F29_TO_CANONICAL) {
    fr_t v;
    if constexpr (OP == F29_TO_BN)
      f29_to_bn(v, o[0]);
    else
      f29_to_canonical_bn(v, o[0]);
    KZG_UNROLL_FULL
    for (int k = 0; k < 8; k++) r0.l[k] = v.v[k];
  }
  st(out, r0);
  st(out + L29, r1);
}

// ---- the XYZZ adders on raw accumulators: acc (57 words) and a second operand q (57 words: for the mixed ops x2, y2 in its first 28
// words, for the accumulator + accumulator ops a whole accumulator) in, acc out, flag = xyzz28_madd_fast's return -------------------
enum {
  X28_MADD_FAST = 0, X28_MADD_COMPLETE = 1, X28_MDBL = 2, X28_DBL_INL = 3, X28_DBL = 4,
  X28_ADD_INL_DBL_INL = 5,  // xyzz28_add_complete_inl<true>
  X28_ADD_INL = 6,          // xyzz28_add_complete_inl<false>
  X28_ADD_COMPLETE = 7,
  X28_TO_XYZZ = 8,          // out: x, y, zz, zzz as 12 words each in the first 48 words, the rest zero
  X28_FROM_XYZZ = 9,        // acc in: x, y, zz, zzz as 12 words each in the first 48 words (all zero = the identity)
};
#define ATOMS28_X28_OPS(X)                                                                                                     \
  X(X28_MADD_FAST) X(X28_MADD_COMPLETE) X(X28_MDBL) X(X28_DBL_INL) X(X28_DBL) X(X28_ADD_INL_DBL_INL) X(X28_ADD_INL)            \
  X(X28_ADD_COMPLETE) X(X28_TO_XYZZ) X(X28_FROM_XYZZ)

KZG_HD void ld_acc(g1_xyzz28& p, const uint32_t* a) {
  ld(p.x, a);
  ld(p.y, a + L28);
  ld(p.zz, a + 2 * L28);
  ld(p.zzz, a + 3 * L28);
  p.inf = a[4 * L28];
}
KZG_HD void st_acc(uint32_t* o, const g1_xyzz28& p) {
  st(o, p.x);
  st(o + L28, p.y);
  st(o + 2 * L28, p.zz);
  st(o + 3 * L28, p.zzz);
  o[4 * L28] = p.inf;
}

template <int OP>
KZG_HD void xyzz28_case(const uint32_t* a, const uint32_t* e, uint32_t* o, uint32_t* flag_out) {
  g1_xyzz28 p, q;
  uint32_t flag = 0;
  if constexpr (OP == X28_FROM_XYZZ) {
    g1_xyzz s;
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) {
      s.x.v[k] = a[k];
      s.y.v[k] = a[12 + k];
      s.zz.v[k] = a[24 + k];
      s.zzz.v[k] = a[36 + k];
    }
    xyzz28_from_xyzz(p, s);
    st_acc(o, p);
  } else {
    ld_acc(p, a);
    ld_acc(q, e);  // q.x, q.y double as x2, y2
    if constexpr (OP == X28_MADD_FAST) flag = xyzz28_madd_fast(p, q.x, q.y) ? 1 : 0;
    if constexpr (OP == X28_MADD_COMPLETE) xyzz28_madd_complete(p, q.x, q.y);
    if constexpr (OP == X28_MDBL) xyzz28_mdbl(p, q.x, q.y);
    if constexpr (OP == X28_DBL_INL) xyzz28_dbl_inl(p);
    if constexpr (OP == X28_DBL) xyzz28_dbl(p);
    if constexpr (OP == X28_ADD_INL_DBL_INL) xyzz28_add_complete_inl<true>(p, q);
    if constexpr (OP == X28_ADD_INL) xyzz28_add_complete_inl<false>(p, q);
    if constexpr (OP == X28_ADD_COMPLETE) xyzz28_add_complete(p, q);
    if constexpr (OP == X28_TO_XYZZ) {
      g1_xyzz r;
      xyzz28_to_xyzz(r, p);
      KZG_UNROLL_FULL
      for (int k = 0; k < 12; k++) {
        o[k] = r.x.v[k];
        o[12 + k] = r.y.v[k];
        o[24 + k] = r.zz.v[k];
        o[36 + k] = r.zzz.v[k];
      }
      KZG_UNROLL_FULL
      for (int k = 48; k < ACC_WORDS; k++) o[k] = 0;
    } else {
      st_acc(o, p);
    }
  }
  *flag_out = flag;
}

// ---- the subgroup ladder's Jacobian adder: acc = x, y, z, inf (43 words), entry = x2, y2 (28 words) ------------------------------
enum { J28_DBL = 0, J28_MADD = 1 };
#define ATOMS28_J28_OPS(X) X(J28_DBL) X(J28_MADD)

template <int OP>
KZG_HD void jac28_case(const uint32_t* a, const uint32_t* e, uint32_t* o) {
  g1_jac28 p;
  fp28 x2, y2;
  ld(p.x, a);
  ld(p.y, a + L28);
  ld(p.z, a + 2 * L28);
  p.inf = a[3 * L28];
  ld(x2, e);
  ld(y2, e + L28);
  if constexpr (OP == J28_DBL) jac28_dbl(p);
  if constexpr (OP == J28_MADD) jac28_madd(p, x2, y2);
  st(o, p.x);
  st(o + L28, p.y);
  st(o + 2 * L28, p.z);
  o[3 * L28] = p.inf;
}

// ---- field.cuh on 12 x 32 / 8 x 32 limbs: a, b in (F::N words each), one result and a flag out ------------------------------------
enum {
  B_MONT_MUL = 0, B_MONT_SQR, B_MONT_MUL_LAZY, B_ADD_MOD, B_SUB_MOD, B_NEG_MOD, B_DBL_MOD, B_ADD_LAZY, B_SUB_LAZY, B_CANONICALIZE,
  B_IS_ZERO_LAZY,  // flag = the answer, out = a
  B_TO_MONT, B_FROM_MONT,
  B_BN_ADD,        // flag = the carry
  B_BN_SUB,        // flag = the borrow
  B_OPS
};
#define ATOMS28_BN_OPS(X)                                                                                                         \
  X(B_MONT_MUL) X(B_MONT_SQR) X(B_MONT_MUL_LAZY) X(B_ADD_MOD) X(B_SUB_MOD) X(B_NEG_MOD) X(B_DBL_MOD) X(B_ADD_LAZY) X(B_SUB_LAZY)  \
  X(B_CANONICALIZE) X(B_IS_ZERO_LAZY) X(B_TO_MONT) X(B_FROM_MONT) X(B_BN_ADD) X(B_BN_SUB)

template <class F, int OP>
KZG_HD void bn_case(const uint32_t* a_in, const uint32_t* b_in, uint32_t* out, uint32_t* flag_out) {
  constexpr int NB = F::N;
  bn<NB> a, b, r;
  KZG_UNROLL_FULL
  for (int k = 0; k < NB; k++) {
    a.v[k] = a_in[k];
    b.v[k] = b_in[k];
    r.v[k] = 0;
  }
  uint32_t flag = 0;
  if constexpr (OP == B_MONT_MUL) mont_mul<F>(r, a, b);
  if constexpr (OP == B_MONT_SQR) mont_sqr<F>(r, a);
  if constexpr (OP == B_MONT_MUL_LAZY) mont_mul_lazy<F>(r, a, b);
  if constexpr (OP == B_ADD_MOD) add_mod<F>(r, a, b);
  if constexpr (OP == B_SUB_MOD) sub_mod<F>(r, a, b);
  if constexpr (OP == B_NEG_MOD) neg_mod<F>(r, a);
  if constexpr (OP == B_DBL_MOD) dbl_mod<F>(r, a);
  if constexpr (OP == B_ADD_LAZY) add_lazy<F>(r, a, b);
  if constexpr (OP == B_SUB_LAZY) sub_lazy<F>(r, a, b);
  if constexpr (OP == B_CANONICALIZE) {
    r = a;
    canonicalize<F>(r);
  }
  if constexpr (OP == B_IS_ZERO_LAZY) {
    r = a;
    flag = is_zero_lazy<F>(a) ? 1 : 0;
  }
  if constexpr (OP == B_TO_MONT) to_mont<F>(r, a);
  if constexpr (OP == B_FROM_MONT) from_mont<F>(r, a);
  if constexpr (OP == B_BN_ADD) flag = bn_add(r, a, b);
  if constexpr (OP == B_BN_SUB) flag = bn_sub(r, a, b);
  KZG_UNROLL_FULL
  for (int k = 0; k < NB; k++) out[k] = r.v[k];
  *flag_out = flag;
}

}  // namespace atoms28
