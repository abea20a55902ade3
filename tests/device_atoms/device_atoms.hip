// TEST-ONLY device harness of the fixed-base MSM's arithmetic (tests/test_gpu_fp30_device.py): the product's own inline
// functions -- kateth_amd/csrc/fp30.cuh (the generated v_mad_i64_i32 statements of mac30_asm.cuh in their generated orders,
// the limb-wise passes, the conversions, the XYZZ adder) and modinv30.cuh -- called one independent case per lane, limbs in and
// limbs out, so that Python integers can be the reference at every operand extreme and on every branch.  Nothing of the
// product is copied here and none of the engine's objects is linked: this unit compiles ITS OWN instances of those functions.
// What that proves and what it cannot (k_msm_comb30's register allocation around the same statements) is in DESIGN.md 5.3.
//
// Every entry takes host pointers, does its own hipMalloc / copy / ONE launch / sync / copy back, frees on every path and
// returns the HIP error code (0 = ok; -1 = an argument it does not know).  Kernels are __launch_bounds__(64); lane i of the
// grid works on case i and lanes past n leave at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../kateth_amd/csrc/fp30.cuh"
#include "../../kateth_amd/csrc/modinv30.cuh"

using namespace kzg;

namespace {

constexpr int L = F30_N;            // limbs of an operand
constexpr int ACC_WORDS = 4 * L + 2;  // x, y, zz, zzz, inf, yneg
constexpr int ENTRY_WORDS = 2 * L;    // x2, y2

// device buffers of one call: freed when the call returns, whichever way
struct dev_bufs {
  void* p[8];
  int n = 0;
  hipError_t err = hipSuccess;
  ~dev_bufs() {
    for (int i = 0; i < n; i++) (void)hipFree(p[i]);
  }
  template <class T>
  T* in(const T* host, size_t count) {
    T* d = out<T>(count);
    if (err == hipSuccess && count) err = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  T* out(size_t count) {
    void* d = nullptr;
    if (err == hipSuccess) {
      err = hipMalloc(&d, (count ? count : 1) * sizeof(T));
      if (err == hipSuccess) {
        p[n++] = d;
        err = hipMemset(d, 0, (count ? count : 1) * sizeof(T));
      }
    }
    return (T*)d;
  }
  template <class T>
  void back(T* host, const T* d, size_t count) {
    if (err == hipSuccess && count) err = hipMemcpy(host, d, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  void launched() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
};

inline unsigned blocks_of(uint32_t n) { return (n + 63u) / 64u; }

__device__ __forceinline__ void ld(fp30& r, const int32_t* p) {
  KZG_UNROLL_FULL
  for (int i = 0; i < L; i++) r.l[i] = p[i];
}
__device__ __forceinline__ void st(int32_t* p, const fp30& a) {
  KZG_UNROLL_FULL
  for (int i = 0; i < L; i++) p[i] = a.l[i];
}

// ---- products, limb-wise passes, conversions ---------------------------------------------------------------------------------
// OPS operands of 13 limbs per case in (6, or 12 for two products side by side), two results out.
enum {
  // one product: operands a, b, c, d, inj0, inj1 (tests/test_fp30_columns_generated.py, operand_sets); result 0
  OP_MUL = 0, OP_SQR = 1, OP_MUL2 = 2, OP_MUL_INJ = 3, OP_SQR_INJ2 = 4, OP_MUL_U = 5,
  // the four pairs of xyzz30_madd_fast: operands of product A, then of product B; results 0 and 1
  OP_PAIR0 = 6, OP_PAIR1 = 7, OP_PAIR2 = 8, OP_PAIR3 = 9,
  // the result ALIASES an operand, as the adder's calls do; result 0 (pairs: 0 and 1)
  OP_ALIAS_MUL_A = 10,    // f30_mul(a, a, b)             p.zz = p.zz * pp
  OP_ALIAS_MUL_B = 11,    // f30_mul(b, a, b)             pp = p.x * pp
  OP_ALIAS_MUL2_C = 12,   // f30_mul2(c, a, b, c, d)      p.y = r * pp + p.y * ppp
  OP_ALIAS_MUL2_D = 13,   // f30_mul2(d, a, b, c, d)      p.y = m * t + nw * p.y
  OP_ALIAS_SQR = 14,      // f30_sqr(a, a)
  OP_ALIAS_PAIR2 = 15,    // pair 2 with B's result in B's a     p.zz = p.zz * pp beside V
  OP_ALIAS_PAIR3 = 16,    // pair 3 with A's result in A's c, B's in B's a     p.y, p.zzz of the last pair
  OP_CARRY = 20, OP_CARRY_WIDE = 21, OP_ADD = 22, OP_SUB = 23, OP_NEG = 24,
  OP_PACK_UNPACK = 25,    // result 0 = f30_unpack(f30_pack(a)), result 1 = the 12 packed words
  OP_FROM_BN = 26,        // a = 12 words
  OP_TO_FP = 27,          // result 0 = 12 words
  OP_PACKED30 = 28,       // a = 12 words (canonical x * 2^384): result 0 = f30_unpack(fp_to_packed30(a)), result 1 = the packed words
  OP_LOAD_ENTRY = 29,     // a, b = 12 packed words each, c.l[0] = neg: results x, y
  OP_ZERO_TESTS = 30,     // result 0 = {f30_maybe_zero, f30_is_zero_exact, f30_is_zero}(a)
};

template <int OP>
constexpr int operands_of() {
  return (OP >= OP_PAIR0 && OP <= OP_PAIR3) || OP == OP_ALIAS_PAIR2 || OP == OP_ALIAS_PAIR3 ? 12 : 6;
}

template <int OP>
__global__ __launch_bounds__(64) void k_f30_op(uint32_t n, const int32_t* __restrict__ in, int32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  constexpr int NOPS = operands_of<OP>();
  fp30 o[NOPS], r0, r1;
  KZG_UNROLL_FULL
  for (int k = 0; k < NOPS; k++) ld(o[k], in + ((size_t)i * NOPS + k) * L);
  KZG_UNROLL_FULL
  for (int k = 0; k < L; k++) r0.l[k] = r1.l[k] = 0;
  if constexpr (OP == OP_MUL) f30_mul(r0, o[0], o[1]);
  if constexpr (OP == OP_SQR) f30_sqr(r0, o[0]);
  if constexpr (OP == OP_MUL2) f30_mul2(r0, o[0], o[1], o[2], o[3]);
  if constexpr (OP == OP_MUL_INJ) f30_mul_inj<-1>(r0, o[0], o[1], o[4]);
  if constexpr (OP == OP_SQR_INJ2) f30_sqr_inj2<-1, -3>(r0, o[0], o[4], o[5]);
  if constexpr (OP == OP_MUL_U) f30_mul_u(r0, o[0], o[1]);
  // template arguments as xyzz30_madd_fast gives them
  if constexpr (OP == OP_PAIR0)
    f30_mul_core2<true, false, 0, 0, false, false, false, -1, 0, false>(r0, o[0], o[1], o[2], o[3], o[4], o[5],  //
                                                                        r1, o[6], o[7], o[8], o[9], o[10], o[11]);
  if constexpr (OP == OP_PAIR1)
    f30_mul_core2<false, false, 0, 0, false, false, false, 0, 0, false>(r0, o[0], o[1], o[2], o[3], o[4], o[5],  //
                                                                        r1, o[6], o[7], o[8], o[9], o[10], o[11]);
  if constexpr (OP == OP_PAIR2)
    f30_mul_core2<true, false, -1, -3, false, false, false, 0, 0, true>(r0, o[0], o[1], o[2], o[3], o[4], o[5],  //
                                                                        r1, o[6], o[7], o[8], o[9], o[10], o[11]);
  if constexpr (OP == OP_PAIR3)
    f30_mul_core2<false, true, 0, 0, false, false, false, 0, 0, true>(r0, o[0], o[1], o[2], o[3], o[4], o[5],  //
                                                                      r1, o[6], o[7], o[8], o[9], o[10], o[11]);
  if constexpr (OP == OP_ALIAS_MUL_A) {
    f30_mul(o[0], o[0], o[1]);
    r0 = o[0];
  }
  if constexpr (OP == OP_ALIAS_MUL_B) {
    f30_mul(o[1], o[0], o[1]);
    r0 = o[1];
  }
  if constexpr (OP == OP_ALIAS_MUL2_C) {
    f30_mul2(o[2], o[0], o[1], o[2], o[3]);
    r0 = o[2];
  }
  if constexpr (OP == OP_ALIAS_MUL2_D) {
    f30_mul2(o[3], o[0], o[1], o[2], o[3]);
    r0 = o[3];
  }
  if constexpr (OP == OP_ALIAS_SQR) {
    f30_sqr(o[0], o[0]);
    r0 = o[0];
  }
  if constexpr (OP == OP_ALIAS_PAIR2) {
    f30_mul_core2<true, false, -1, -3, false, false, false, 0, 0, true>(r0, o[0], o[1], o[2], o[3], o[4], o[5],  //
                                                                        o[6], o[6], o[7], o[6], o[7], o[10], o[11]);
    r1 = o[6];
  }
  if constexpr (OP == OP_ALIAS_PAIR3) {
    f30_mul_core2<false, true, 0, 0, false, false, false, 0, 0, true>(o[2], o[0], o[1], o[2], o[3], o[4], o[5],  //
                                                                      o[6], o[6], o[7], o[6], o[7], o[10], o[11]);
    r0 = o[2];
    r1 = o[6];
  }
  if constexpr (OP == OP_CARRY) {
    r0 = o[0];
    f30_carry(r0);
  }
  if constexpr (OP == OP_CARRY_WIDE) {
    r0 = o[0];
    f30_carry<true>(r0);
  }
  if constexpr (OP == OP_ADD) f30_add(r0, o[0], o[1]);
  if constexpr (OP == OP_SUB) f30_sub(r0, o[0], o[1]);
  if constexpr (OP == OP_NEG) f30_neg(r0, o[0]);
  if constexpr (OP == OP_PACK_UNPACK) {
    uint32_t w[12];
    f30_pack(w, o[0]);
    f30_unpack(r0, w);
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) r1.l[k] = (int32_t)w[k];
  }
  if constexpr (OP == OP_FROM_BN) {
    fp_t v;
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) v.v[k] = (uint32_t)o[0].l[k];
    f30_from_bn(r0, v);
  }
  if constexpr (OP == OP_TO_FP) {
    fp_t v;
    f30_to_fp(v, o[0]);
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) r0.l[k] = (int32_t)v.v[k];
  }
  if constexpr (OP == OP_PACKED30) {
    fp_t v;
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) v.v[k] = (uint32_t)o[0].l[k];
    uint32_t w[12];
    fp_to_packed30(w, v);
    f30_unpack(r0, w);
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) r1.l[k] = (int32_t)w[k];
  }
  if constexpr (OP == OP_LOAD_ENTRY) {
    uint32_t wx[12], wy[12];
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) {
      wx[k] = (uint32_t)o[0].l[k];
      wy[k] = (uint32_t)o[1].l[k];
    }
    f30_load_entry(r0, r1, wx, wy, o[2].l[0] != 0);
  }
  if constexpr (OP == OP_ZERO_TESTS) {
    r0.l[0] = f30_maybe_zero(o[0]) ? 1 : 0;
    r0.l[1] = f30_is_zero_exact(o[0]) ? 1 : 0;
    r0.l[2] = f30_is_zero(o[0]) ? 1 : 0;
  }
  st(out + ((size_t)i * 2 + 0) * L, r0);
  st(out + ((size_t)i * 2 + 1) * L, r1);
}

template <int OP>
int run_f30_op(uint32_t n, const int32_t* in, int32_t* out) {
  dev_bufs b;
  const size_t n_in = (size_t)n * operands_of<OP>() * L, n_out = (size_t)n * 2 * L;
  const int32_t* d_in = b.in(in, n_in);
  int32_t* d_out = b.out<int32_t>(n_out);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL(k_f30_op<OP>, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_in, d_out);
    b.launched();
  }
  b.back(out, d_out, n_out);
  return (int)b.err;
}

// ---- the adder on raw accumulators ---------------------------------------------------------------------------------------------
enum { XOP_MADD_FAST = 0, XOP_MADD_COMPLETE = 1, XOP_DBL = 2, XOP_MDBL = 3, XOP_TO_XYZZ = 4 };

template <int OP>
__global__ __launch_bounds__(64) void k_xyzz30_op(uint32_t n, const int32_t* __restrict__ acc_in, const int32_t* __restrict__ entry_in,
                                                  int32_t* __restrict__ acc_out, int32_t* __restrict__ flag_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const int32_t* a = acc_in + (size_t)i * ACC_WORDS;
  const int32_t* e = entry_in + (size_t)i * ENTRY_WORDS;
  int32_t* o = acc_out + (size_t)i * ACC_WORDS;
  g1_xyzz30 p;
  fp30 x2, y2;
  ld(p.x, a);
  ld(p.y, a + L);
  ld(p.zz, a + 2 * L);
  ld(p.zzz, a + 3 * L);
  p.inf = (uint32_t)a[4 * L];
  p.yneg = (uint32_t)a[4 * L + 1];
  ld(x2, e);
  ld(y2, e + L);
  int32_t flag = 0;
  if constexpr (OP == XOP_MADD_FAST) flag = xyzz30_madd_fast(p, x2, y2) ? 1 : 0;
  if constexpr (OP == XOP_MADD_COMPLETE) xyzz30_madd_complete(p, x2, y2);
  if constexpr (OP == XOP_DBL) xyzz30_dbl(p);
  if constexpr (OP == XOP_MDBL) xyzz30_mdbl(p, x2, y2);
  if constexpr (OP == XOP_TO_XYZZ) {
    g1_xyzz r;
    xyzz30_to_xyzz(r, p);
    KZG_UNROLL_FULL
    for (int k = 0; k < 12; k++) {
      o[k] = (int32_t)r.x.v[k];
      o[12 + k] = (int32_t)r.y.v[k];
      o[24 + k] = (int32_t)r.zz.v[k];
      o[36 + k] = (int32_t)r.zzz.v[k];
    }
    KZG_UNROLL_FULL
    for (int k = 48; k < ACC_WORDS; k++) o[k] = 0;
  } else {
    st(o, p.x);
    st(o + L, p.y);
    st(o + 2 * L, p.zz);
    st(o + 3 * L, p.zzz);
    o[4 * L] = (int32_t)p.inf;
    o[4 * L + 1] = (int32_t)p.yneg;
  }
  flag_out[i] = flag;
}

template <int OP>
int run_xyzz30_op(uint32_t n, const int32_t* acc_in, const int32_t* entry_in, int32_t* acc_out, int32_t* flag_out) {
  dev_bufs b;
  const int32_t* d_acc = b.in(acc_in, (size_t)n * ACC_WORDS);
  const int32_t* d_entry = b.in(entry_in, (size_t)n * ENTRY_WORDS);
  int32_t* d_out = b.out<int32_t>((size_t)n * ACC_WORDS);
  int32_t* d_flag = b.out<int32_t>(n);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL(k_xyzz30_op<OP>, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_acc, d_entry, d_out, d_flag);
    b.launched();
  }
  b.back(acc_out, d_out, (size_t)n * ACC_WORDS);
  b.back(flag_out, d_flag, n);
  return (int)b.err;
}

// ---- signed sums of compressed points, as a lane of k_msm_comb30 adds table entries --------------------------------------------
__global__ __launch_bounds__(64) void k_g1_sum30(uint32_t n, uint32_t len, const uint8_t* __restrict__ pts48, const uint8_t* __restrict__ signs,
                                                 const uint32_t* __restrict__ lens, const uint32_t* __restrict__ doublings,
                                                 uint8_t* __restrict__ out48, int32_t* __restrict__ status, uint32_t* __restrict__ slow_calls) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t mine = lens[i] < len ? lens[i] : len;
  g1_xyzz30 acc;
  xyzz30_set_inf(acc);
  uint32_t slow = 0;
  int32_t stat = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < mine; k++) {
    fp_t x, y;
    bool inf;
    uint8_t enc[48];
    for (int q = 0; q < 48; q++) enc[q] = pts48[((size_t)i * len + k) * 48 + q];
    stat = g1_uncompress(x, y, inf, enc);
    if (stat) break;
    if (inf) continue;
    uint32_t wx[12], wy[12];
    fp_to_packed30(wx, x);
    fp_to_packed30(wy, y);
    fp30 x2, y2;
    f30_load_entry(x2, y2, wx, wy, xyzz30_entry_neg(acc, signs[(size_t)i * len + k] != 0));
    bool done = false;
    if (!acc.inf) done = xyzz30_madd_fast(acc, x2, y2);
    if (!done) {  // as the kernel does it: out of line, on a copy, the entry loaded again with the copy's sign
      g1_xyzz30 tmp = acc;
      fp30 sx, sy;
      f30_load_entry(sx, sy, wx, wy, xyzz30_entry_neg(tmp, signs[(size_t)i * len + k] != 0));
      xyzz30_madd_complete(tmp, sx, sy);
      acc = tmp;
      slow++;
    }
  }
  uint8_t enc[48];
  if (stat == 0) {
#pragma unroll 1
    for (uint32_t k = 0; k < doublings[i]; k++) {
      if (acc.inf) break;
      g1_xyzz30 tmp = acc;
      xyzz30_dbl(tmp);
      acc = tmp;
    }
    g1_xyzz r;
    xyzz30_to_xyzz(r, acc);
    g1_compress_xyzz(enc, r);
  } else {
    for (int q = 0; q < 48; q++) enc[q] = 0;
  }
  for (int q = 0; q < 48; q++) out48[(size_t)i * 48 + q] = enc[q];
  status[i] = stat;
  slow_calls[i] = slow;
}

// ---- safegcd inversion ----------------------------------------------------------------------------------------------------
// variant 0: modinv30<M> (out of line), 1: modinv30_inl<M>, 2: the Montgomery-domain fp_inv / fr_inv, 3: fr_inv_inl (Fr only)
template <class M, int VARIANT>
__global__ __launch_bounds__(64) void k_modinv30(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  constexpr int NB = M::NB;
  bn<NB> a, r;
  KZG_UNROLL_FULL
  for (int k = 0; k < NB; k++) {
    a.v[k] = in[(size_t)i * NB + k];
    r.v[k] = 0;
  }
  if constexpr (VARIANT == 0) (void)modinv30<M>(r, a);
  if constexpr (VARIANT == 1) (void)modinv30_inl<M>(r, a);
  if constexpr (VARIANT == 2) {
    if constexpr (NB == 12)
      fp_inv(r, a);
    else
      fr_inv(r, a);
  }
  if constexpr (VARIANT == 3) fr_inv_inl(r, a);
  KZG_UNROLL_FULL
  for (int k = 0; k < NB; k++) out[(size_t)i * NB + k] = r.v[k];
}

template <class M, int VARIANT>
int run_modinv30(uint32_t n, const uint32_t* in, uint32_t* out) {
  dev_bufs b;
  const uint32_t* d_in = b.in(in, (size_t)n * M::NB);
  uint32_t* d_out = b.out<uint32_t>((size_t)n * M::NB);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL((k_modinv30<M, VARIANT>), dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_in, d_out);
    b.launched();
  }
  b.back(out, d_out, (size_t)n * M::NB);
  return (int)b.err;
}

}  // namespace

// in: n cases of 6 operands (12 for the pair ops 6..9, 15, 16) of 13 int32 limbs; out: n cases of 2 results of 13 limbs
extern "C" int da_f30_op(int op, uint32_t n, const int32_t* in, int32_t* out) {
  if (!in || !out || n == 0) return -1;
  switch (op) {
#define DA_CASE(OP) \
  case OP: return run_f30_op<OP>(n, in, out);
    DA_CASE(OP_MUL)
    DA_CASE(OP_SQR)
    DA_CASE(OP_MUL2)
    DA_CASE(OP_MUL_INJ)
    DA_CASE(OP_SQR_INJ2)
    DA_CASE(OP_MUL_U)
    DA_CASE(OP_PAIR0)
    DA_CASE(OP_PAIR1)
    DA_CASE(OP_PAIR2)
    DA_CASE(OP_PAIR3)
    DA_CASE(OP_ALIAS_MUL_A)
    DA_CASE(OP_ALIAS_MUL_B)
    DA_CASE(OP_ALIAS_MUL2_C)
    DA_CASE(OP_ALIAS_MUL2_D)
    DA_CASE(OP_ALIAS_SQR)
    DA_CASE(OP_ALIAS_PAIR2)
    DA_CASE(OP_ALIAS_PAIR3)
    DA_CASE(OP_CARRY)
    DA_CASE(OP_CARRY_WIDE)
    DA_CASE(OP_ADD)
    DA_CASE(OP_SUB)
    DA_CASE(OP_NEG)
    DA_CASE(OP_PACK_UNPACK)
    DA_CASE(OP_FROM_BN)
    DA_CASE(OP_TO_FP)
    DA_CASE(OP_PACKED30)
    DA_CASE(OP_LOAD_ENTRY)
    DA_CASE(OP_ZERO_TESTS)
#undef DA_CASE
  }
  return -1;
}

// acc_in / acc_out: n x 54 int32 (x, y, zz, zzz limbs, inf, yneg); entry_in: n x 26 (x2, y2 limbs); flag_out: n (madd_fast's return).
// op 4 (xyzz30_to_xyzz) writes x, y, zz, zzz as 12 words each into the first 48 words of acc_out.
extern "C" int da_xyzz30_op(int op, uint32_t n, const int32_t* acc_in, const int32_t* entry_in, int32_t* acc_out, int32_t* flag_out) {
  if (!acc_in || !entry_in || !acc_out || !flag_out || n == 0) return -1;
  switch (op) {
    case XOP_MADD_FAST: return run_xyzz30_op<XOP_MADD_FAST>(n, acc_in, entry_in, acc_out, flag_out);
    case XOP_MADD_COMPLETE: return run_xyzz30_op<XOP_MADD_COMPLETE>(n, acc_in, entry_in, acc_out, flag_out);
    case XOP_DBL: return run_xyzz30_op<XOP_DBL>(n, acc_in, entry_in, acc_out, flag_out);
    case XOP_MDBL: return run_xyzz30_op<XOP_MDBL>(n, acc_in, entry_in, acc_out, flag_out);
    case XOP_TO_XYZZ: return run_xyzz30_op<XOP_TO_XYZZ>(n, acc_in, entry_in, acc_out, flag_out);
  }
  return -1;
}

// the device twin of tests/hostmath/shim.cpp's hm_g1_sum30, one signed sum per lane: case i adds its first lens[i] (<= len) of the
// len points at pts48[i * len * 48], point k negated when signs[i * len + k] != 0, then doubles doublings[i] times.
// status[i]: g1_uncompress's code (out48 zero then); slow_calls[i]: additions that left the fast path.
extern "C" int da_g1_sum30(uint32_t n, uint32_t len, const uint8_t* pts48, const uint8_t* signs, const uint32_t* lens, const uint32_t* doublings,
                           uint8_t* out48, int32_t* status, uint32_t* slow_calls) {
  if (!pts48 || !signs || !lens || !doublings || !out48 || !status || !slow_calls || n == 0 || len == 0) return -1;
  dev_bufs b;
  const uint8_t* d_pts = b.in(pts48, (size_t)n * len * 48);
  const uint8_t* d_signs = b.in(signs, (size_t)n * len);
  const uint32_t* d_lens = b.in(lens, n);
  const uint32_t* d_dbl = b.in(doublings, n);
  uint8_t* d_out = b.out<uint8_t>((size_t)n * 48);
  int32_t* d_status = b.out<int32_t>(n);
  uint32_t* d_slow = b.out<uint32_t>(n);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL(k_g1_sum30, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, len, d_pts, d_signs, d_lens, d_dbl, d_out, d_status, d_slow);
    b.launched();
  }
  b.back(out48, d_out, (size_t)n * 48);
  b.back(status, d_status, n);
  b.back(slow_calls, d_slow, n);
  return (int)b.err;
}

// which 0: Fp (12 words per value), 1: Fr (8 words); variants: see k_modinv30.  Variants 0, 1 take and give plain residues,
// 2 and 3 Montgomery forms (a R -> a^-1 R).
extern "C" int da_modinv30(int which, int variant, uint32_t n, const uint32_t* in, uint32_t* out) {
  if (!in || !out || n == 0) return -1;
  if (which == 0) {
    switch (variant) {
      case 0: return run_modinv30<FpInv30, 0>(n, in, out);
      case 1: return run_modinv30<FpInv30, 1>(n, in, out);
      case 2: return run_modinv30<FpInv30, 2>(n, in, out);
    }
  } else if (which == 1) {
    switch (variant) {
      case 0: return run_modinv30<FrInv30, 0>(n, in, out);
      case 1: return run_modinv30<FrInv30, 1>(n, in, out);
      case 2: return run_modinv30<FrInv30, 2>(n, in, out);
      case 3: return run_modinv30<FrInv30, 3>(n, in, out);
    }
  }
  return -1;
}
