// compute_cells_and_kzg_proofs / recover_cells_and_kzg_proofs (EIP-7594), the proofs half: the kernels that turn blobs into the 128
// quotient vectors the fixed-base MSM commits (compiled once: engine_proof.hip owns this header).  The arithmetic and its bounds are
// cellproof_math.cuh's; this is NOT FK20 -- no monomial setup, no G1 transform: 128 scalar transforms and 128 MSMs per blob.
#pragma once
#include "cellproof_math.cuh"

namespace kzg {
#if defined(__HIPCC__)

// one thread per entry of the omega_128 table (layout and entry function: cellproof_math.cuh)
static __global__ __launch_bounds__(64) void k_setup_cellproof_tab(uint32_t* __restrict__ ztab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= CELLPROOF_TAB_ENTRIES) return;
  uint32_t e[CELLS_TAB_ENTRY];
  cellproof_tab_entry(i, e);
#pragma unroll
  for (int q = 0; q < CELLS_TAB_ENTRY; q++) ztab[(uint64_t)i * CELLS_TAB_ENTRY + q] = e[q];
}

// The coefficients of n blobs: one 512-thread workgroup per blob, the grid loops over the blobs, the image in LDS as in k_compute_cells.
// Item b is the 131,072 bytes at items + b * stride (stride 131,072: blobs; 262,144: cells 0..63 of a cell set); its 4096 coefficients
// go to coeffs + b * 131,072 (8 x u32 little-endian each, natural order, canonical) and its 128 vector statuses to vstatus[128 b ..].
// skip_rejected = false: the item is range-checked as k_compute_cells checks it and status[b] is written (0, or
// KZG_ERR_BLOB_INVALID_FIELD_ELEMENT).  skip_rejected = true: status[b] is an earlier kernel's verdict and is only read; an item it
// rejected is not looked at.  A rejected item's coefficients are not written (k_cell_quotients does not read them).
static __global__ __launch_bounds__(CELLS_THREADS) void k_cell_coeffs(const uint8_t* __restrict__ items, uint64_t stride, uint64_t n, bool skip_rejected,
                                                                   const uint32_t* __restrict__ tab, uint32_t* __restrict__ coeffs, int32_t* __restrict__ status,
                                                                   int32_t* __restrict__ vstatus) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ int sh_pre, sh_bad;  // the earlier verdict (thread 0 writes it, everyone reads it) and this kernel's own (whoever finds one)
  for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
    uint32_t t = threadIdx.x;  // opaque per item, as in k_compute_cells
    asm volatile("" : "+v"(t));
    if (t == 0) {
      sh_pre = skip_rejected ? status[b] : 0;
      sh_bad = 0;
    }
    __syncthreads();  // also: the previous item's last reads of the image are done
    int code = sh_pre;
    if (code == 0) {  // block-uniform
      if (cellproof_load_blob(img, items + b * stride, t)) sh_bad = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
      __syncthreads();
      code = sh_bad;
    }
    if (t < 128) vstatus[b * 128u + t] = code;
    if (t == 0 && !skip_rejected) status[b] = code;
    if (code == 0) {
#pragma unroll 1
      for (int p = 0; p < CELLPROOF_PASSES; p++) {
        cellproof_inv_pass(img, tab, t, p);
        __syncthreads();
      }
      uint32_t ts = t;
      asm volatile("" : "+v"(ts));
      cellproof_store_words(coeffs + b * (uint64_t)(CELLPROOF_COEFF_BYTES / 4), img, ts);
    }
    __syncthreads();  // every wave has read the two verdicts before thread 0 replaces them for the next item
  }
}

// The quotient vector of one (blob, cell) by a 512-thread workgroup, the body k_cell_quotients and k_cell_quotients_sel share: the blob's
// coefficients come from global memory (the workgroups of a blob read the same 128 KiB: L2), the division and the four forward passes are
// cellproof_math.cuh's, and the 4096 evaluations leave as 8 x u32 little-endian words at out[e * 8 ..] -- the MSM's scalar vector, in the
// blob's own order.  `img`: the image, `carry`: the segment totals, both in LDS.
static __device__ __forceinline__ void cell_quotient_vector(uint32_t* img, uint32_t* carry, const uint32_t* __restrict__ item_coeffs,
                                                            const uint32_t* __restrict__ tab, const uint32_t* __restrict__ ztab, uint32_t cell,
                                                            uint32_t* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  {
    fr29 c[8], z, z8;
    cellproof_load_segment(c, item_coeffs, t);
    cells_tw(z, ztab, cellproof_zpow(cell, 1));
    cellproof_segment_total(carry, c, z, t);
    __syncthreads();
    cells_tw(z8, ztab, cellproof_zpow(cell, 8));
    cellproof_divide(img, carry, c, z, z8, t);
  }
  __syncthreads();
#pragma unroll 1
  for (int p = CELLPROOF_PASSES - 1; p >= 0; p--) {
    cellproof_fwd_pass(img, tab, t, p);
    __syncthreads();
  }
  uint32_t ts = t;
  asm volatile("" : "+v"(ts));
  cellproof_store_words(out, img, ts);
}

// All 128 vectors of every blob: block = 128 blob + cell, the vector at q[(128 blob + cell) * 4096 + e].  A vector whose status is non-zero
// is neither read nor written: the MSM's encoder zeroes its 48 bytes.
// LDS: the image and 16 KiB of segment totals, 147,456 B.
static __global__ __launch_bounds__(CELLS_THREADS) void k_cell_quotients(const uint32_t* __restrict__ coeffs, const uint32_t* __restrict__ tab,
                                                                      const uint32_t* __restrict__ ztab, const int32_t* __restrict__ vstatus,
                                                                      uint32_t* __restrict__ q) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ uint32_t carry[CELLPROOF_CARRY_DWORDS];
  const uint32_t vec = blockIdx.x, cell = vec & 127u;
  if (vstatus[vec] != 0) return;  // block-uniform
  cell_quotient_vector(img, carry, coeffs + (uint64_t)(vec >> 7) * (CELLPROOF_COEFF_BYTES / 4), tab, ztab, cell, q + (uint64_t)vec * 32768u);
}

// The vectors of chosen (blob, cell) pairs only (the select calls): block s takes pair = pairs[s] = 128 blob + cell (the host's list,
// cellproof_plan.hpp; the blob counted within the pass), writes its vector at the COMPACT slot q[s * 4096 + e] and hands the blob's verdict
// on as cstat[s] = vstatus[pair], whatever the code: the MSM's encoder zeroes the slots of a rejected blob.  The grid is the number of
// pairs: every block has one.  Both reads are block-uniform, like k_cell_quotients' one.  LDS as k_cell_quotients.
static __global__ __launch_bounds__(CELLS_THREADS) void k_cell_quotients_sel(const uint32_t* __restrict__ coeffs, const uint32_t* __restrict__ tab,
                                                                          const uint32_t* __restrict__ ztab, const int32_t* __restrict__ vstatus,
                                                                          const uint32_t* __restrict__ pairs, int32_t* __restrict__ cstat,
                                                                          uint32_t* __restrict__ q) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ uint32_t carry[CELLPROOF_CARRY_DWORDS];
  const uint32_t slot = blockIdx.x, pair = pairs[slot];
  const int32_t code = vstatus[pair];
  if (threadIdx.x == 0) cstat[slot] = code;
  if (code != 0) return;  // block-uniform
  cell_quotient_vector(img, carry, coeffs + (uint64_t)cellproof_pair_item(pair) * (CELLPROOF_COEFF_BYTES / 4), tab, ztab, cellproof_pair_cell(pair),
                       q + (uint64_t)slot * 32768u);
}

// The compact proofs of a pass to their places: slot s (48 bytes at compact + 48 s, three uint4) goes to proofs + 48 pairs[s], where `proofs`
// is the caller's buffer at the pass's first item.  One thread per slot; both buffers are 16-byte aligned.  Positions no pair names are
// not touched.
static __global__ __launch_bounds__(256) void k_cellproof_scatter(const uint4* __restrict__ compact, const uint32_t* __restrict__ pairs, uint32_t nslots,
                                                                  uint4* __restrict__ proofs) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  const uint4* src = compact + (uint64_t)s * 3u;
  uint4* dst = proofs + (uint64_t)pairs[s] * 3u;
  const uint4 a = src[0], b = src[1], c = src[2];
  dst[0] = a;
  dst[1] = b;
  dst[2] = c;
}

// ---- the data column forms: siblings of k_cell_coeffs and k_cellproof_scatter, whose code they leave as it was ----
// k_cell_coeffs' load out of a column matrix (recovery with proofs): item b is cells 0..63 of row row0 + b of `cells`, a matrix of
// `rows` rows (cells_column_major: a wave reads one cell, 2 KiB in a row).  status[b] is k_columns_recover's verdict and is only read; a
// row it rejected is not looked at.  Coefficients and vector statuses as k_cell_coeffs writes them.
// gfx950: 159 VGPRs, scratch 0, LDS 131,080 B, two waves per SIMD (tests/test_datacolumns_host.py).
static __global__ __launch_bounds__(CELLS_THREADS) void k_columns_coeffs(const uint8_t* __restrict__ cells, uint64_t rows, uint64_t row0, uint64_t n,
                                                                      const uint32_t* __restrict__ tab, uint32_t* __restrict__ coeffs,
                                                                      const int32_t* __restrict__ status, int32_t* __restrict__ vstatus) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ int sh_pre, sh_bad;
  for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
    uint32_t t = threadIdx.x;  // opaque per item, as in k_compute_cells
    asm volatile("" : "+v"(t));
    if (t == 0) {
      sh_pre = status[b];
      sh_bad = 0;
    }
    __syncthreads();
    int code = sh_pre;
    if (code == 0) {  // block-uniform
      if (cellproof_load_blob(img, cells, t, cells_column_major{rows, row0 + b})) sh_bad = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
      __syncthreads();
      code = sh_bad;
    }
    if (t < 128) vstatus[b * 128u + t] = code;
    if (code == 0) {
#pragma unroll 1
      for (int p = 0; p < CELLPROOF_PASSES; p++) {
        cellproof_inv_pass(img, tab, t, p);
        __syncthreads();
      }
      uint32_t ts = t;
      asm volatile("" : "+v"(ts));
      cellproof_store_words(coeffs + b * (uint64_t)(CELLPROOF_COEFF_BYTES / 4), img, ts);
    }
    __syncthreads();
  }
}

// k_cellproof_scatter into a column matrix of proofs of `rows` rows: slot s goes to the proof of (cell, row row0 + item) of pairs[s] =
// 128 item + cell, at 48 (cell rows + row0 + item).  Positions no pair names are not touched.
static __global__ __launch_bounds__(256) void k_columns_scatter(const uint4* __restrict__ compact, const uint32_t* __restrict__ pairs, uint32_t nslots,
                                                                uint8_t* __restrict__ proofs, uint64_t rows, uint64_t row0) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  const uint32_t pair = pairs[s];
  const uint4* src = compact + (uint64_t)s * 3u;
  uint4* dst = reinterpret_cast<uint4*>(proofs + proofs_column_at(rows, row0 + cellproof_pair_item(pair), cellproof_pair_cell(pair)));
  const uint4 a = src[0], b = src[1], c = src[2];
  dst[0] = a;
  dst[1] = b;
  dst[2] = c;
}

#endif
}  // namespace kzg
