// TEST-ONLY device harness of the radix-2^28 Fp, the radix-2^29 Fr, field.cuh's 12 x 32 / 8 x 32 limb arithmetic and the XYZZ28 /
// Jacobian adders (tests/test_gpu_fp28_device.py): the product's own inline functions -- kateth_amd/csrc/fp28.cuh, fr29.cuh, field.cuh,
// g1_decode28.cuh; on the device the products are rdx_column over the generated mad28_chain statements of mac_asm.cuh -- called one
// independent case per lane, limbs in and limbs out, so that Python integers can be the reference at every lazy-form extreme and on
// every branch.  Nothing of the product is copied here and none of the engine's objects is linked: this unit compiles ITS OWN
// instances of those functions (what that proves and what it cannot is in DESIGN.md 5.3).  The per-case bodies are
// atoms28_ops.h, which the CPU build (tests/hostmath/shim.cpp) instantiates too.  The point-level entries (sums, decoder, encoder,
// powers) are device_atoms28_points.hip.
//
// Every entry takes host pointers, does its own hipMalloc / copy / ONE launch / sync / copy back, frees on every path and returns
// the HIP error code (0 = ok; -1 = an argument it does not know).  Kernels are __launch_bounds__(64); lane i of the grid works on
// case i and lanes past n leave at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../kateth_amd/csrc/g1_decode28.cuh"
#include "../../kateth_amd/csrc/fr29.cuh"
#include "atoms28_ops.h"
#include "da_bufs.h"

using namespace kzg;
using namespace atoms28;

namespace {

// ---- fp28 / fr29: four operands in, two results out ---------------------------------------------------------------------------------
template <int OP, bool FR>
__global__ __launch_bounds__(64) void k_rdx_op(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  constexpr int L = FR ? L29 : L28;
  if constexpr (FR)
    f29_case<OP>(in + (size_t)i * 4 * L, out + (size_t)i * 2 * L);
  else
    f28_case<OP>(in + (size_t)i * 4 * L, out + (size_t)i * 2 * L);
}
template <int OP, bool FR>
int run_rdx_op(uint32_t n, const uint32_t* in, uint32_t* out) {
  constexpr int L = FR ? L29 : L28;
  dev_bufs b;
  const uint32_t* d_in = b.in(in, (size_t)n * 4 * L);
  uint32_t* d_out = b.out<uint32_t>((size_t)n * 2 * L);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL((k_rdx_op<OP, FR>), dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_in, d_out);
    b.launched();
  }
  b.back(out, d_out, (size_t)n * 2 * L);
  return (int)b.err;
}

// ---- the adders on raw accumulators ---------------------------------------------------------------------------------------------
template <int OP>
__global__ __launch_bounds__(64) void k_xyzz28_op(uint32_t n, const uint32_t* __restrict__ acc_in, const uint32_t* __restrict__ q_in,
                                                  uint32_t* __restrict__ acc_out, uint32_t* __restrict__ flag_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  xyzz28_case<OP>(acc_in + (size_t)i * ACC_WORDS, q_in + (size_t)i * ACC_WORDS, acc_out + (size_t)i * ACC_WORDS, flag_out + i);
}
template <int OP>
int run_xyzz28_op(uint32_t n, const uint32_t* acc_in, const uint32_t* q_in, uint32_t* acc_out, uint32_t* flag_out) {
  dev_bufs b;
  const uint32_t* d_acc = b.in(acc_in, (size_t)n * ACC_WORDS);
  const uint32_t* d_q = b.in(q_in, (size_t)n * ACC_WORDS);
  uint32_t* d_out = b.out<uint32_t>((size_t)n * ACC_WORDS);
  uint32_t* d_flag = b.out<uint32_t>(n);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL(k_xyzz28_op<OP>, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_acc, d_q, d_out, d_flag);
    b.launched();
  }
  b.back(acc_out, d_out, (size_t)n * ACC_WORDS);
  b.back(flag_out, d_flag, n);
  return (int)b.err;
}

template <int OP>
__global__ __launch_bounds__(64) void k_jac28_op(uint32_t n, const uint32_t* __restrict__ acc_in, const uint32_t* __restrict__ entry_in,
                                                 uint32_t* __restrict__ acc_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  jac28_case<OP>(acc_in + (size_t)i * JAC_WORDS, entry_in + (size_t)i * ENTRY_WORDS, acc_out + (size_t)i * JAC_WORDS);
}
template <int OP>
int run_jac28_op(uint32_t n, const uint32_t* acc_in, const uint32_t* entry_in, uint32_t* acc_out) {
  dev_bufs b;
  const uint32_t* d_acc = b.in(acc_in, (size_t)n * JAC_WORDS);
  const uint32_t* d_entry = b.in(entry_in, (size_t)n * ENTRY_WORDS);
  uint32_t* d_out = b.out<uint32_t>((size_t)n * JAC_WORDS);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL(k_jac28_op<OP>, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_acc, d_entry, d_out);
    b.launched();
  }
  b.back(acc_out, d_out, (size_t)n * JAC_WORDS);
  return (int)b.err;
}

// ---- field.cuh: the device carry chains (__builtin_addc / __builtin_subc), the mac_asm.cuh products, the lazy variants ---------------
template <class F, int OP>
__global__ __launch_bounds__(64) void k_bn_op(uint32_t n, const uint32_t* __restrict__ a_in, const uint32_t* __restrict__ b_in, uint32_t* __restrict__ out,
                                              uint32_t* __restrict__ flag_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  bn_case<F, OP>(a_in + (size_t)i * F::N, b_in + (size_t)i * F::N, out + (size_t)i * F::N, flag_out + i);
}
template <class F, int OP>
int run_bn_op(uint32_t n, const uint32_t* a, const uint32_t* b_, uint32_t* out, uint32_t* flag) {
  dev_bufs b;
  const uint32_t* d_a = b.in(a, (size_t)n * F::N);
  const uint32_t* d_b = b.in(b_, (size_t)n * F::N);
  uint32_t* d_out = b.out<uint32_t>((size_t)n * F::N);
  uint32_t* d_flag = b.out<uint32_t>(n);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL((k_bn_op<F, OP>), dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_a, d_b, d_out, d_flag);
    b.launched();
  }
  b.back(out, d_out, (size_t)n * F::N);
  b.back(flag, d_flag, n);
  return (int)b.err;
}
template <class F>
int bn_dispatch(int op, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flag) {
  switch (op) {
#define DA_CASE(OP) \
  case OP: return run_bn_op<F, OP>(n, a, b, out, flag);
    ATOMS28_BN_OPS(DA_CASE)
#undef DA_CASE
  }
  return -1;
}

}  // namespace

// in: n cases of 4 operands of 14 limbs; out: n cases of 2 results of 14 limbs.  Op numbers: atoms28_ops.h
extern "C" int da_f28_op(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
  if (!in || !out || n == 0) return -1;
  switch (op) {
#define DA_CASE(OP) \
  case OP: return run_rdx_op<OP, false>(n, in, out);
    ATOMS28_F28_OPS(DA_CASE)
#undef DA_CASE
  }
  return -1;
}
// the same with 9 limbs per operand
extern "C" int da_f29_op(int op, uint32_t n, const uint32_t* in, uint32_t* out) {
  if (!in || !out || n == 0) return -1;
  switch (op) {
#define DA_CASE(OP) \
  case OP: return run_rdx_op<OP, true>(n, in, out);
    ATOMS28_F29_OPS(DA_CASE)
#undef DA_CASE
  }
  return -1;
}
// field 0: Fp (12 words per value), 1: Fr (8 words); a, b, out: n values; flag: n words (carry, borrow or is_zero_lazy's answer)
extern "C" int da_bn_op(int field, int op, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flag) {
  if (!a || !b || !out || !flag || n == 0) return -1;
  if (field == 0) return bn_dispatch<FpParams>(op, n, a, b, out, flag);
  if (field == 1) return bn_dispatch<FrParams>(op, n, a, b, out, flag);
  return -1;
}
// acc_in / q_in / acc_out: n x 57 words (x, y, zz, zzz limbs, inf); flag_out: n (xyzz28_madd_fast's return).  Layouts of the
// conversions: atoms28_ops.h
extern "C" int da_xyzz28_op(int op, uint32_t n, const uint32_t* acc_in, const uint32_t* q_in, uint32_t* acc_out, uint32_t* flag_out) {
  if (!acc_in || !q_in || !acc_out || !flag_out || n == 0) return -1;
  switch (op) {
#define DA_CASE(OP) \
  case OP: return run_xyzz28_op<OP>(n, acc_in, q_in, acc_out, flag_out);
    ATOMS28_X28_OPS(DA_CASE)
#undef DA_CASE
  }
  return -1;
}
// acc_in / acc_out: n x 43 words (x, y, z limbs, inf); entry_in: n x 28 (x2, y2 limbs)
extern "C" int da_jac28_op(int op, uint32_t n, const uint32_t* acc_in, const uint32_t* entry_in, uint32_t* acc_out) {
  if (!acc_in || !entry_in || !acc_out || n == 0) return -1;
  switch (op) {
#define DA_CASE(OP) \
  case OP: return run_jac28_op<OP>(n, acc_in, entry_in, acc_out);
    ATOMS28_J28_OPS(DA_CASE)
#undef DA_CASE
  }
  return -1;
}
