// compute_cells (EIP-7594): the blob extension kernel (compiled once: engine_proof.hip owns this header).  Replaces
// compute_cells of specs/fulu/polynomial-commitments-sampling.md = c-kzg-4844's compute_cells_and_kzg_proofs(cells, NULL, blob).
// recover_cells: k_recover_cells below replaces the cells half of recover_cells_and_kzg_proofs.
#pragma once
#include "cells_math.cuh"
#include "recover_math.cuh"
#include "issue_fair.cuh"
#include "scalar_load.cuh"

namespace kzg {
#if defined(__HIPCC__)

// One 512-thread workgroup per blob, the grid loops over the blobs.  The blob is read from HBM once (16-byte big-endian loads, element
// i 512 + t: a wave reads 2 KiB in a row), range-checked as it arrives, and kept in LDS as eight word planes (131,072 B static, the
// whole CU: one workgroup = two waves per SIMD) through the seven steps of cells_math.cuh.  Once the whole blob is known to be canonical
// cells 0..63 are stored from the image -- global memory is not read a second time -- and the extension half leaves through the image
// too, so that all stores are as coalesced as the loads.  No global scratch.
// A blob with an element >= r: status KZG_ERR_BLOB_INVALID_FIELD_ELEMENT and 262,144 zero bytes.
// Shape: 512 threads x 8 elements, four image round trips per transform (seven barriers in all: the two middle passes share one).
// LDS lets one workgroup live on a CU, i.e. two waves per SIMD, so a wave may use 256 VGPRs -- a 1,024-thread workgroup (4 elements
// per thread, six round trips per transform) would have to stay within 128.
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, ROCm 7): 256 VGPRs, 0 AGPRs, 106 SGPRs (6 spilled to VGPR lanes), scratch 0,
// LDS 131,076 B static (above 64 KiB without any launch attribute), occupancy 2 waves per SIMD.
static __global__ __launch_bounds__(CELLS_THREADS) void k_compute_cells(const uint8_t* __restrict__ blobs, uint64_t n, const uint32_t* __restrict__ tab,
                                                                     uint8_t* __restrict__ out_cells, int32_t* __restrict__ status) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ int sh_bad;
  for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
    // opaque per blob: otherwise every address of the load and store phases is computed once, ahead of the blob loop, and kept in
    // registers through the steps (256 VGPRs and spills)
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const uint4* in = reinterpret_cast<const uint4*>(blobs + b * 131072ull);
    uint4* out = reinterpret_cast<uint4*>(out_cells + b * 262144ull);
    // the image as 4096 x 32 big-endian bytes, coalesced like the loads, to out[first ..]
    auto store_half = [&](uint32_t first) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const uint32_t e = (uint32_t)i * CELLS_THREADS + t;
        fr_t v;
        cells_get(v, img, e);
        out[first + 2 * e] = make_uint4(__builtin_bswap32(v.v[7]), __builtin_bswap32(v.v[6]), __builtin_bswap32(v.v[5]), __builtin_bswap32(v.v[4]));
        out[first + 2 * e + 1] = make_uint4(__builtin_bswap32(v.v[3]), __builtin_bswap32(v.v[2]), __builtin_bswap32(v.v[1]), __builtin_bswap32(v.v[0]));
      }
    };
    if (t == 0) sh_bad = 0;
    __syncthreads();  // also: the previous blob's last reads of the image are done
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t e = (uint32_t)i * CELLS_THREADS + t;
      const uint4 w0 = in[2 * e], w1 = in[2 * e + 1];
      fr_t v;
      v.v[7] = __builtin_bswap32(w0.x);
      v.v[6] = __builtin_bswap32(w0.y);
      v.v[5] = __builtin_bswap32(w0.z);
      v.v[4] = __builtin_bswap32(w0.w);
      v.v[3] = __builtin_bswap32(w1.x);
      v.v[2] = __builtin_bswap32(w1.y);
      v.v[1] = __builtin_bswap32(w1.z);
      v.v[0] = __builtin_bswap32(w1.w);
      bad |= !fr_is_canonical(v);
      cells_put(img, e, v);
    }
    if (bad) sh_bad = 1;
    __syncthreads();
    if (sh_bad) {  // block-uniform
      const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 32; i++) out[(uint32_t)i * CELLS_THREADS + t] = zero;
      if (t == 0) status[b] = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
      __syncthreads();  // every wave has read sh_bad before thread 0 clears it for the next blob
      continue;
    }
    store_half(0);  // cells 0..63: the blob itself
    if (t == 0) status[b] = 0;
#pragma unroll 1
    for (int k = 0; k < CELLS_STEPS; k++) {
      cells_step(img, tab, t, k);
      __syncthreads();
    }
    store_half(8192);  // cells 64..127
  }
}

// The extension half alone (kzg_verify_blob_cell_proofs_batch: cells 0..63 are the blob's own bytes and are read where they lie).  A
// sibling of k_compute_cells, not an instantiation of a shared body, for the reason given at the data column forms below: the same load
// phase, range check and seven steps, and ONE store phase -- cells 64..127 of blob b to out_ext + 131,072 b, coalesced through the image.
// status[b] is the blob's entry of the caller's error record: a blob with an element >= r gets KZG_ERR_BLOB_INVALID_FIELD_ELEMENT and
// 131,072 zero bytes, which nothing may read as cells -- the verify kernels take the status, not the bytes, for the blob's verdict.
// Same shape and budget as k_compute_cells (asserted by tests/test_blob_cell_proofs_host.py).
static __global__ __launch_bounds__(CELLS_THREADS) void k_compute_cells_ext(const uint8_t* __restrict__ blobs, uint64_t n, const uint32_t* __restrict__ tab,
                                                                         uint8_t* __restrict__ out_ext, int32_t* __restrict__ status) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ int sh_bad;
  for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
    uint32_t t = threadIdx.x;  // opaque per blob, as in k_compute_cells
    asm volatile("" : "+v"(t));
    const uint4* in = reinterpret_cast<const uint4*>(blobs + b * 131072ull);
    uint4* out = reinterpret_cast<uint4*>(out_ext + b * 131072ull);
    if (t == 0) sh_bad = 0;
    __syncthreads();  // also: the previous blob's last reads of the image are done
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t e = (uint32_t)i * CELLS_THREADS + t;
      const uint4 w0 = in[2 * e], w1 = in[2 * e + 1];
      fr_t v;
      v.v[7] = __builtin_bswap32(w0.x);
      v.v[6] = __builtin_bswap32(w0.y);
      v.v[5] = __builtin_bswap32(w0.z);
      v.v[4] = __builtin_bswap32(w0.w);
      v.v[3] = __builtin_bswap32(w1.x);
      v.v[2] = __builtin_bswap32(w1.y);
      v.v[1] = __builtin_bswap32(w1.z);
      v.v[0] = __builtin_bswap32(w1.w);
      bad |= !fr_is_canonical(v);
      cells_put(img, e, v);
    }
    if (bad) sh_bad = 1;
    __syncthreads();
    if (sh_bad) {  // block-uniform
      const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 16; i++) out[(uint32_t)i * CELLS_THREADS + t] = zero;
      if (t == 0) status[b] = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
      __syncthreads();  // every wave has read sh_bad before thread 0 clears it for the next blob
      continue;
    }
    if (t == 0) status[b] = 0;
#pragma unroll 1
    for (int k = 0; k < CELLS_STEPS; k++) {
      cells_step(img, tab, t, k);
      __syncthreads();
    }
    uint32_t ts = t;  // opaque again: the store phase's addresses are not to be computed ahead of the steps and kept
    asm volatile("" : "+v"(ts));
#pragma unroll
    for (int i = 0; i < 8; i++) {  // cells 64..127: the image as 4096 x 32 big-endian bytes, coalesced like the loads
      const uint32_t e = (uint32_t)i * CELLS_THREADS + ts;
      fr_t v;
      cells_get(v, img, e);
      out[2 * e] = make_uint4(__builtin_bswap32(v.v[7]), __builtin_bswap32(v.v[6]), __builtin_bswap32(v.v[5]), __builtin_bswap32(v.v[4]));
      out[2 * e + 1] = make_uint4(__builtin_bswap32(v.v[3]), __builtin_bswap32(v.v[2]), __builtin_bswap32(v.v[1]), __builtin_bswap32(v.v[0]));
    }
  }
}

// recover_cells: one 512-thread workgroup per cell set, the grid loops over the sets; the steps are those of recover_math.cuh, on the
// same LDS image as k_compute_cells, followed by that kernel's own seven steps for cells 64..127.  Global traffic per accepted item:
// the present cells are read twice (to be scaled into the image, and to be compared with at the end), 128 KiB go to the item's own
// output region and come back (the stash of steps 3 and 7: every thread reads what it wrote itself, so no fence is needed), and the
// 256 KiB of the result are written once.  The bytes of an absent cell are never read.
// Status, in this order: fewer than 64 cells present -> KZG_ERR_CELLS_NOT_ENOUGH; a present element >= r ->
// KZG_ERR_BLOB_INVALID_FIELD_ELEMENT; the recovered polynomial differs from a present element -> KZG_ERR_CELLS_INCONSISTENT.  A
// rejected item gets 262,144 zero bytes -- after the barrier that ends its last step, so they land on top of what was stored before.
// LDS: the image, 6,912 B of Z_c / P_u, the mask and the flag.
static __global__ __launch_bounds__(CELLS_THREADS) void k_recover_cells(const uint8_t* __restrict__ cells, const uint8_t* __restrict__ present, uint64_t n,
                                                                     const uint32_t* __restrict__ tab, const uint32_t* __restrict__ rtab,
                                                                     uint8_t* __restrict__ out_cells, int32_t* __restrict__ status) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ uint32_t zs[RECOVER_ZS_DWORDS];
  __shared__ uint32_t mask[4];
  __shared__ int sh_bad;
  for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
    uint32_t t = threadIdx.x;  // opaque per item, as in k_compute_cells
    asm volatile("" : "+v"(t));
    const uint8_t* in = cells + b * 262144ull;
    uint8_t* out = out_cells + b * 262144ull;
    if (t < 4) mask[t] = reinterpret_cast<const uint32_t*>(present + b * 16ull)[t];
    if (t == 0) sh_bad = 0;
    __syncthreads();  // also: the previous item's last reads of the image are done
    if (recover_count(mask) < RECOVER_MIN_CELLS) {  // block-uniform
      if (t == 0) sh_bad = KZG_ERR_CELLS_NOT_ENOUGH;
    } else {
      recover_prep_partial(img, rtab, mask, t);
      __syncthreads();
      recover_prep_combine(zs, img, t);
      __syncthreads();
#pragma unroll 1
      for (int k = 0; k < RECOVER_STEPS; k++) {
        if (k == 0 || k == 4) {
          uint32_t tl = t;  // opaque again: the addresses of a load or store phase are not to be computed ahead of the loop and kept
          asm volatile("" : "+v"(tl));
          if (recover_load_half(img, zs, in, mask, tl, (uint32_t)k >> 2)) sh_bad = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
          __syncthreads();
          if (sh_bad) break;  // block-uniform
        }
        recover_step(img, zs, reinterpret_cast<uint32_t*>(out), tab, rtab, t, k);
        __syncthreads();
      }
      if (sh_bad == 0) {
#pragma unroll 1
        for (uint32_t half = 0; half < 2; half++) {
          if (half) {
#pragma unroll 1
            for (int k = 0; k < CELLS_STEPS; k++) {
              cells_step(img, tab, t, k);
              __syncthreads();
            }
          }
          uint32_t ts = t;
          asm volatile("" : "+v"(ts));
          if (recover_store_half(img, in, out, mask, ts, half)) sh_bad = KZG_ERR_CELLS_INCONSISTENT;
          __syncthreads();
        }
      }
    }
    __syncthreads();
    const int code = sh_bad;
    if (code) {
      uint4* z = reinterpret_cast<uint4*>(out);
      const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 32; i++) z[(uint32_t)i * CELLS_THREADS + t] = zero;
    }
    if (t == 0) status[b] = code;
    __syncthreads();  // every wave has read mask and sh_bad before the next item replaces them
  }
}

// ---- the data column forms (kzg_compute_data_columns_batch, kzg_recover_data_columns_batch) ----
// The two kernels above with the cells in a COLUMN MATRIX of `rows` rows -- the cell of column c, row r at 2048 (c rows + r) -- through
// cells_column_major (cells_math.cuh); item b of a launch is row row0 + b.  They are siblings, not instantiations of one body: a shared
// body moved the blob-major kernels' code, whose figures the host tests assert ("Data columns").  In every phase that moves cells the 64 lanes of a
// wave are inside ONE cell (e >> 6 = 8 i + (t >> 6) in the halves and in the stash, q >> 7 = 4 i + (t >> 7) in the zero-fill), so the
// map's cell is scalar, the column's base is scalar arithmetic, and a wave still moves 2 KiB in a row.  t stays opaque per item and per
// phase for the reason given above.
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950, ROCm 7): k_columns_compute 256 VGPRs, k_columns_recover 244 VGPRs, both 0 AGPRs,
// scratch 0, their sibling's LDS, two waves per SIMD (asserted by tests/test_datacolumns_host.py).

// k_compute_cells, the cells of blob b to row row0 + b of out_cells; a rejected blob's row is zero bytes in all 128 columns
static __global__ __launch_bounds__(CELLS_THREADS) void k_columns_compute(const uint8_t* __restrict__ blobs, uint64_t n, const uint32_t* __restrict__ tab,
                                                                       uint8_t* __restrict__ out_cells, uint64_t rows, uint64_t row0,
                                                                       int32_t* __restrict__ status) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ int sh_bad;
  for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const uint4* in = reinterpret_cast<const uint4*>(blobs + b * 131072ull);
    const cells_column_major map{rows, row0 + b};
    // the 16 bytes at offset 16 q of the item's cell set
    auto out = [&](uint32_t q) -> uint4& { return *reinterpret_cast<uint4*>(out_cells + map((size_t)q * 16u)); };
    auto store_half = [&](uint32_t first) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const uint32_t e = (uint32_t)i * CELLS_THREADS + t;
        fr_t v;
        cells_get(v, img, e);
        out(first + 2 * e) = make_uint4(__builtin_bswap32(v.v[7]), __builtin_bswap32(v.v[6]), __builtin_bswap32(v.v[5]), __builtin_bswap32(v.v[4]));
        out(first + 2 * e + 1) = make_uint4(__builtin_bswap32(v.v[3]), __builtin_bswap32(v.v[2]), __builtin_bswap32(v.v[1]), __builtin_bswap32(v.v[0]));
      }
    };
    if (t == 0) sh_bad = 0;
    __syncthreads();
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t e = (uint32_t)i * CELLS_THREADS + t;
      const uint4 w0 = in[2 * e], w1 = in[2 * e + 1];
      fr_t v;
      v.v[7] = __builtin_bswap32(w0.x);
      v.v[6] = __builtin_bswap32(w0.y);
      v.v[5] = __builtin_bswap32(w0.z);
      v.v[4] = __builtin_bswap32(w0.w);
      v.v[3] = __builtin_bswap32(w1.x);
      v.v[2] = __builtin_bswap32(w1.y);
      v.v[1] = __builtin_bswap32(w1.z);
      v.v[0] = __builtin_bswap32(w1.w);
      bad |= !fr_is_canonical(v);
      cells_put(img, e, v);
    }
    if (bad) sh_bad = 1;
    __syncthreads();
    if (sh_bad) {  // block-uniform
      const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 32; i++) out((uint32_t)i * CELLS_THREADS + t) = zero;
      if (t == 0) status[b] = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
      __syncthreads();
      continue;
    }
    store_half(0);
    if (t == 0) status[b] = 0;
#pragma unroll 1
    for (int k = 0; k < CELLS_STEPS; k++) {
      cells_step(img, tab, t, k);
      __syncthreads();
    }
    store_half(8192);
  }
}

// k_recover_cells, rows row0 .. row0 + n - 1 of `cells` to the same rows of out_cells under the call's ONE mask, which is a kernel
// argument (four little-endian words, recover_present's order).  The stash of steps 3 and 7 goes through the map too: piece e is 32
// bytes inside cell e >> 6, so the row's own cells 0..63 of out_cells are the stash, every thread reads back what it wrote itself, and
// no workspace is needed.  out_cells must not overlap cells: the present cells are read a second time after the stash is written.
static __global__ __launch_bounds__(CELLS_THREADS) void k_columns_recover(const uint8_t* __restrict__ cells, uint4 one_mask, uint64_t n,
                                                                       const uint32_t* __restrict__ tab, const uint32_t* __restrict__ rtab,
                                                                       uint8_t* __restrict__ out_cells, uint64_t rows, uint64_t row0,
                                                                       int32_t* __restrict__ status) {
  __shared__ uint32_t img[CELLS_IMAGE_DWORDS];
  __shared__ uint32_t zs[RECOVER_ZS_DWORDS];
  __shared__ uint32_t mask[4];
  __shared__ int sh_bad;
  for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const cells_column_major map{rows, row0 + b};
    if (t == 0) {
      mask[0] = one_mask.x, mask[1] = one_mask.y, mask[2] = one_mask.z, mask[3] = one_mask.w;
      sh_bad = 0;
    }
    __syncthreads();
    if (recover_count(mask) < RECOVER_MIN_CELLS) {  // block-uniform
      if (t == 0) sh_bad = KZG_ERR_CELLS_NOT_ENOUGH;
    } else {
      recover_prep_partial(img, rtab, mask, t);
      __syncthreads();
      recover_prep_combine(zs, img, t);
      __syncthreads();
#pragma unroll 1
      for (int k = 0; k < RECOVER_STEPS; k++) {
        if (k == 0 || k == 4) {
          uint32_t tl = t;
          asm volatile("" : "+v"(tl));
          if (recover_load_half(img, zs, cells, mask, tl, (uint32_t)k >> 2, map)) sh_bad = KZG_ERR_BLOB_INVALID_FIELD_ELEMENT;
          __syncthreads();
          if (sh_bad) break;  // block-uniform
        }
        recover_step(img, zs, reinterpret_cast<uint32_t*>(out_cells), tab, rtab, t, k, map);
        __syncthreads();
      }
      if (sh_bad == 0) {
#pragma unroll 1
        for (uint32_t half = 0; half < 2; half++) {
          if (half) {
#pragma unroll 1
            for (int k = 0; k < CELLS_STEPS; k++) {
              cells_step(img, tab, t, k);
              __syncthreads();
            }
          }
          uint32_t ts = t;
          asm volatile("" : "+v"(ts));
          if (recover_store_half(img, cells, out_cells, mask, ts, half, map)) sh_bad = KZG_ERR_CELLS_INCONSISTENT;
          __syncthreads();
        }
      }
    }
    __syncthreads();
    const int code = sh_bad;
    if (code) {
      const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 32; i++) *reinterpret_cast<uint4*>(out_cells + map((size_t)((uint32_t)i * CELLS_THREADS + t) * 16u)) = zero;
    }
    if (t == 0) status[b] = code;
    __syncthreads();
  }
}

#endif
}  // namespace kzg
