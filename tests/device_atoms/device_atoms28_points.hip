// TEST-ONLY device harness, second unit (tests/test_gpu_fp28_device.py): the point-level users of the radix-2^28 field, one case per
// lane -- signed sums through xyzz28_madd_fast / xyzz28_madd_complete as the bucket kernels add decoded points, the point decoder
// g1_decompress28 (square root, sign choice, subgroup ladder: the lane-varying control flow around its long loops), the encoder
// g1_encode_xyzz28_words, and the sliding-window powers and the inversion.  Same rules as device_atoms28.hip: the product's own
// inline functions, this unit's own instances, host pointers in and out, one launch per call, everything freed on every path, the HIP
// error code back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../kateth_amd/csrc/g1_decode28.cuh"
#include "da_bufs.h"

using namespace kzg;

namespace {

// ---- signed sums of compressed points: the device twin of tests/hostmath/shim.cpp's hm_g1_sum28 -----------------------------------
__global__ __launch_bounds__(64) void k_g1_sum28(uint32_t n, uint32_t len, const uint8_t* __restrict__ pts48, const uint8_t* __restrict__ signs,
                                                 const uint32_t* __restrict__ lens, uint8_t* __restrict__ out48, int32_t* __restrict__ status,
                                                 uint32_t* __restrict__ slow_calls) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t mine = lens[i] < len ? lens[i] : len;
  g1_xyzz28 acc;
  xyzz28_set_inf(acc);
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
    fp_to_r392(x, x);
    fp_to_r392(y, y);
    fp28 x2, y2;
    f28_load_entry(x2, y2, x, y, signs[(size_t)i * len + k] != 0);
    bool done = false;
    if (!acc.inf) done = xyzz28_madd_fast(acc, x2, y2);
    if (!done) {  // out of line, on a copy
      g1_xyzz28 tmp = acc;
      xyzz28_madd_complete(tmp, x2, y2);
      acc = tmp;
      slow++;
    }
  }
  uint8_t enc[48];
  if (stat == 0) {
    g1_xyzz r;
    xyzz28_to_xyzz(r, acc);
    g1_compress_xyzz(enc, r);
  } else {
    for (int q = 0; q < 48; q++) enc[q] = 0;
  }
  for (int q = 0; q < 48; q++) out48[(size_t)i * 48 + q] = enc[q];
  status[i] = stat;
  slow_calls[i] = slow;
}

// ---- the decoder, one encoding per lane -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_g1_decompress28(uint32_t n, const uint8_t* __restrict__ in48, uint32_t r392_out, uint32_t* __restrict__ x_out,
                                                        uint32_t* __restrict__ y_out, int32_t* __restrict__ status, uint32_t* __restrict__ inf_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  uint8_t enc[48];
  for (int q = 0; q < 48; q++) enc[q] = in48[(size_t)i * 48 + q];
  fp_t x, y;
  bn_zero(x);
  bn_zero(y);
  bool inf = false;
  const int32_t st = g1_decompress28(x, y, inf, enc, r392_out != 0);
  KZG_UNROLL_FULL
  for (int k = 0; k < 12; k++) {
    x_out[(size_t)i * 12 + k] = st == 0 ? x.v[k] : 0u;
    y_out[(size_t)i * 12 + k] = st == 0 ? y.v[k] : 0u;
  }
  status[i] = st;
  inf_out[i] = inf ? 1u : 0u;
}

// ---- the encoder --------------------------------------------------------------------------------------------------------------
template <bool WANT_AFFINE>
__global__ __launch_bounds__(64) void k_g1_encode28(uint32_t n, const uint32_t* __restrict__ xyzz48, uint32_t* __restrict__ out12, uint32_t* __restrict__ aff24) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  g1_xyzz p;
  KZG_UNROLL_FULL
  for (int k = 0; k < 12; k++) {
    p.x.v[k] = xyzz48[(size_t)i * 48 + k];
    p.y.v[k] = xyzz48[(size_t)i * 48 + 12 + k];
    p.zz.v[k] = xyzz48[(size_t)i * 48 + 24 + k];
    p.zzz.v[k] = xyzz48[(size_t)i * 48 + 36 + k];
  }
  uint32_t w[12], a[24];
  KZG_UNROLL_FULL
  for (int k = 0; k < 24; k++) a[k] = 0;
  g1_encode_xyzz28_words<WANT_AFFINE>(w, a, p);
  KZG_UNROLL_FULL
  for (int k = 0; k < 12; k++) out12[(size_t)i * 12 + k] = w[k];
  KZG_UNROLL_FULL
  for (int k = 0; k < 24; k++) aff24[(size_t)i * 24 + k] = a[k];
}

// ---- powers and the inversion: N-form limbs in, N-form limbs out -------------------------------------------------------------------
// which 0: f28_inv<true>, 1: f28_inv<false>, 2: f28_inv_fermat, 3: f28_sqrt_candidate
template <int WHICH>
__global__ __launch_bounds__(64) void k_f28_pow(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  fp28 a, r;
  KZG_UNROLL_FULL
  for (int k = 0; k < F28_N; k++) {
    a.l[k] = in[(size_t)i * F28_N + k];
    r.l[k] = 0;
  }
  if constexpr (WHICH == 0) f28_inv<true>(r, a);
  if constexpr (WHICH == 1) f28_inv<false>(r, a);
  if constexpr (WHICH == 2) f28_inv_fermat(r, a);
  if constexpr (WHICH == 3) f28_sqrt_candidate(r, a);
  KZG_UNROLL_FULL
  for (int k = 0; k < F28_N; k++) out[(size_t)i * F28_N + k] = r.l[k];
}
template <int WHICH>
int run_f28_pow(uint32_t n, const uint32_t* in, uint32_t* out) {
  dev_bufs b;
  const uint32_t* d_in = b.in(in, (size_t)n * F28_N);
  uint32_t* d_out = b.out<uint32_t>((size_t)n * F28_N);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL(k_f28_pow<WHICH>, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_in, d_out);
    b.launched();
  }
  b.back(out, d_out, (size_t)n * F28_N);
  return (int)b.err;
}

}  // namespace

// case i adds its first lens[i] (<= len) of the len points at pts48[i * len * 48], point k negated when signs[i * len + k] != 0.
// status[i]: g1_uncompress's code (out48 zero then); slow_calls[i]: additions that left the fast path.
extern "C" int da_g1_sum28(uint32_t n, uint32_t len, const uint8_t* pts48, const uint8_t* signs, const uint32_t* lens, uint8_t* out48, int32_t* status,
                           uint32_t* slow_calls) {
  if (!pts48 || !signs || !lens || !out48 || !status || !slow_calls || n == 0 || len == 0) return -1;
  dev_bufs b;
  const uint8_t* d_pts = b.in(pts48, (size_t)n * len * 48);
  const uint8_t* d_signs = b.in(signs, (size_t)n * len);
  const uint32_t* d_lens = b.in(lens, n);
  uint8_t* d_out = b.out<uint8_t>((size_t)n * 48);
  int32_t* d_status = b.out<int32_t>(n);
  uint32_t* d_slow = b.out<uint32_t>(n);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL(k_g1_sum28, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, len, d_pts, d_signs, d_lens, d_out, d_status, d_slow);
    b.launched();
  }
  b.back(out48, d_out, (size_t)n * 48);
  b.back(status, d_status, n);
  b.back(slow_calls, d_slow, n);
  return (int)b.err;
}

// x, y: n x 12 words (canonical 2^384-Montgomery, or 2^392 when r392_out; zero unless status is 0); status, inf: n
extern "C" int da_g1_decompress28(uint32_t n, const uint8_t* in48, int r392_out, uint32_t* x, uint32_t* y, int32_t* status, uint32_t* inf) {
  if (!in48 || !x || !y || !status || !inf || n == 0) return -1;
  dev_bufs b;
  const uint8_t* d_in = b.in(in48, (size_t)n * 48);
  uint32_t* d_x = b.out<uint32_t>((size_t)n * 12);
  uint32_t* d_y = b.out<uint32_t>((size_t)n * 12);
  int32_t* d_status = b.out<int32_t>(n);
  uint32_t* d_inf = b.out<uint32_t>(n);
  if (b.err == hipSuccess) {
    hipLaunchKernelGGL(k_g1_decompress28, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_in, r392_out ? 1u : 0u, d_x, d_y, d_status, d_inf);
    b.launched();
  }
  b.back(x, d_x, (size_t)n * 12);
  b.back(y, d_y, (size_t)n * 12);
  b.back(status, d_status, n);
  b.back(inf, d_inf, n);
  return (int)b.err;
}

// xyzz48: n x 48 words (x, y, zz, zzz, canonical 2^384-Montgomery; zz = 0: the identity); out12: n x 12 words (the 48 output bytes in
// memory order); aff24: n x 24 words (zero unless want_affine)
extern "C" int da_g1_encode28(uint32_t n, int want_affine, const uint32_t* xyzz48, uint32_t* out12, uint32_t* aff24) {
  if (!xyzz48 || !out12 || !aff24 || n == 0) return -1;
  dev_bufs b;
  const uint32_t* d_in = b.in(xyzz48, (size_t)n * 48);
  uint32_t* d_out = b.out<uint32_t>((size_t)n * 12);
  uint32_t* d_aff = b.out<uint32_t>((size_t)n * 24);
  if (b.err == hipSuccess) {
    if (want_affine)
      hipLaunchKernelGGL(k_g1_encode28<true>, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_in, d_out, d_aff);
    else
      hipLaunchKernelGGL(k_g1_encode28<false>, dim3(blocks_of(n)), dim3(64), 0, nullptr, n, d_in, d_out, d_aff);
    b.launched();
  }
  b.back(out12, d_out, (size_t)n * 12);
  b.back(aff24, d_aff, (size_t)n * 24);
  return (int)b.err;
}

// in, out: n x 14 limbs (N-form); which: see k_f28_pow
extern "C" int da_f28_pow(int which, uint32_t n, const uint32_t* in, uint32_t* out) {
  if (!in || !out || n == 0) return -1;
  switch (which) {
    case 0: return run_f28_pow<0>(n, in, out);
    case 1: return run_f28_pow<1>(n, in, out);
    case 2: return run_f28_pow<2>(n, in, out);
    case 3: return run_f28_pow<3>(n, in, out);
  }
  return -1;
}
