// verify_cell_kzg_proof_batch (EIP-7594): the kernels of the cells kind of batch verification (compiled once: engine_verify.hip owns
// this header).  k_cells_leaves is the front; k_cells_interp and k_cells_reduce run once the challenge r is known and leave the 64
// scalars -S_j of lincomb B's monomial terms (arithmetic and layout: cellverify_math.cuh).  The row-indexed form
// (kzg_verify_cell_proof_batch_rows) adds k_cells_rows_leaves, the front with the commitment read through an index, and
// k_cells_row_weights / k_cells_roww_reduce, lincomb B's commitment scalars.  The per-item verdicts add k_cells_each_leaves,
// k_each_vec_level and k_each_gather_cells (at the end of this file); the row-indexed form's verdicts add k_each_rows_status.  The blob
// form (kzg_verify_blob_cell_proofs_batch: the rows form with implicit indices, cells 0..63 read out of the blob) adds the BLOB instances
// k_blob_cells_leaves, k_blob_cells_interp and k_blob_cells_each_leaves, and the two per-blob folds k_blob_weights and k_each_blob_status.
#pragma once
#include "cellverify_math.cuh"
#include "verify_kernels.cuh"

namespace kzg {
#if defined(__HIPCC__)

// The front: ONE LANE PER CELL.  A leaf is SHA-256(commitment48 || cell_index as 8 bytes big-endian || cell 2048 || proof48), a serial
// chain of 34 compressions over 2,152 bytes; lanes of a group could only share it through a tree, which would be another leaf.  The
// lane streams its cell once as 16-byte loads -- four per block, each 128-byte line used by two consecutive blocks of the same lane --
// and range-checks the elements word by word while they sit in the message schedule: the cell's words lie two words off the block grid
// (12 + 2 words come first), so the second half of the loaded quad that straddles a block boundary is carried to the next block.
// It writes z_k = h_c^64 (from the 128-entry table; zero for a rejected index) and y_k = 0 where k_batch_scalars reads them, the status
// words of the index (KZG_ERR_CELL_INDEX) and of the cell (KZG_ERR_BLOB_INVALID_FIELD_ELEMENT), and the leaf.
// Like k_points_leaves it runs beside two decoder waves per SIMD: sha256_block_rolled, 64 VGPRs, no scratch.
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950): the figures are in DESIGN.md and asserted by tests/test_cellverify_host.py.
//
// ROWS (k_cells_rows_leaves, the row-indexed form): the commitment is commitments48[commitment_indices[i]] of a list of `ncom` -- the
// row index is read and the address formed right where the twelve words are loaded, so nothing of it lives through the hash; an index
// >= ncom reads commitment 0 and is rejected below (KZG_ERR_COMMITMENT_INDEX, ahead of the cell index's code).  The body is shared;
// k_cells_leaves is its ROWS = false instance and compiles to what it was.
//
// BLOB (k_blob_cells_leaves, kzg_verify_blob_cell_proofs_batch): the item number IS the pair of indices -- row i >> 7, column i & 127;
// the two index pointers are null and never read.  `cells` are the BLOBS (131,072 bytes each) and cell k of blob b lies at
// cells + 131072 b + 2048 k for k < 64, at ext + 131072 b + 2048 (k - 64) otherwise (cellv_blob_cell): one select per item ahead of
// the hash, the streaming loop is the sibling's.  The cell's status is the BLOB's, as k_compute_cells_ext left it in blob_status (it
// ran ahead on the same stream) -- all 128 items of a rejected blob carry its code, its zero-filled extension is never taken for
// cells -- so the lane's own range check has no reader and the compiler drops it.
template <bool ROWS, bool BLOB = false>
__device__ __forceinline__ void cells_leaves_body(const uint8_t* __restrict__ commitments48, const unsigned long long* __restrict__ commitment_indices, uint64_t ncom,
                                                  const unsigned long long* __restrict__ cell_indices, const uint8_t* __restrict__ cells,
                                                  const uint8_t* __restrict__ proofs48, uint64_t n, const fr_t* __restrict__ h64_plain, fr_t* __restrict__ z_plain,
                                                  fr_t* __restrict__ y_plain, int32_t* __restrict__ status_index, int32_t* __restrict__ status_cell,
                                                  uint32_t* __restrict__ leaves /* n x 8 words */, const uint8_t* __restrict__ ext = nullptr,
                                                  const int32_t* __restrict__ blob_status = nullptr) {
  issue_priority_latency();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t row = i;
  if (BLOB) {
    row = i >> 7;
  } else if (ROWS) {
    const unsigned long long r = commitment_indices[i];
    row = r < ncom ? r : 0;
  }
  const uint32_t* c = reinterpret_cast<const uint32_t*>(commitments48 + row * 48);
  const uint4* cell = reinterpret_cast<const uint4*>(BLOB ? cellv_blob_cell(cells, ext, i) : cells + i * (uint64_t)KZG_BYTES_PER_CELL);
  const unsigned long long index = BLOB ? (unsigned long long)(i & 127u) : cell_indices[i];
  // The range check rides on the words as they pass, most significant first: `cmp` is the comparison of the current element's words so
  // far with r's (0 undecided, 1 below, 2 above), so that nothing of an element is kept beyond the two words a block boundary cuts off.
  uint32_t cmp = 0;
  bool bad = false;
  auto word = [&](uint32_t v, int q) {  // word q (0 = most significant) of an element; q = 7 ends it
    const uint32_t m = modulus<FrParams>().v[7 - q];
    cmp = cmp != 0u ? cmp : (v < m ? 1u : (v > m ? 2u : 0u));
    if (q == 7) {
      bad |= cmp != 1u;
      cmp = 0;
    }
  };
  sha256_state s;
  sha256_init(s);
  uint32_t w[16];
#pragma unroll
  for (int q = 0; q < 12; q++) w[q] = __builtin_bswap32(c[q]);
  w[12] = (uint32_t)(index >> 32);
  w[13] = (uint32_t)index;
  uint32_t carry0, carry1;  // words 2 and 3 of quad 4 b, loaded for block b: its first two words end block b, these begin block b + 1
  {
    const uint4 q = cell[0];
    w[14] = __builtin_bswap32(q.x);
    w[15] = __builtin_bswap32(q.y);
    carry0 = __builtin_bswap32(q.z);
    carry1 = __builtin_bswap32(q.w);
    word(w[14], 0);
    word(w[15], 1);
  }
  sha256_block_rolled(s, w);
  // block b: cell words 16 b - 14 .. 16 b + 1 = the carried two, quads 4 b - 3 .. 4 b - 1 and two words more: the first two of quad 4 b,
  // or, in block 32, of the proof; elements 2 b - 2 and 2 b - 1 end in it
  auto quads = [&](uint32_t b) {
    w[0] = carry0;
    w[1] = carry1;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const uint4 q = cell[4 * b - 3 + k];
      w[2 + 4 * k] = __builtin_bswap32(q.x);
      w[3 + 4 * k] = __builtin_bswap32(q.y);
      w[4 + 4 * k] = __builtin_bswap32(q.z);
      w[5 + 4 * k] = __builtin_bswap32(q.w);
    }
#pragma unroll
    for (int q = 0; q < 6; q++) word(w[q], 2 + q);
#pragma unroll
    for (int q = 0; q < 8; q++) word(w[6 + q], q);
  };
#pragma unroll 1
  for (uint32_t b = 1; b < 32; b++) {
    quads(b);
    const uint4 q = cell[4 * b];
    w[14] = __builtin_bswap32(q.x);
    w[15] = __builtin_bswap32(q.y);
    carry0 = __builtin_bswap32(q.z);
    carry1 = __builtin_bswap32(q.w);
    word(w[14], 0);
    word(w[15], 1);
    sha256_block_rolled(s, w);
  }
  quads(32);
  // The item's index anew, opaque to the compiler: the proof's address and the three output addresses are computed HERE and not ahead of
  // the loop, where they would be eight registers held through 33 blocks (and, at 64 registers, spilled)
  uint32_t lane = threadIdx.x;
  asm volatile("" : "+v"(lane));
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + lane;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(proofs48 + k * 48);
  w[14] = __builtin_bswap32(p[0]);
  w[15] = __builtin_bswap32(p[1]);
  sha256_block_rolled(s, w);
#pragma unroll
  for (int q = 0; q < 10; q++) w[q] = __builtin_bswap32(p[2 + q]);
  w[10] = 0x80000000u;
#pragma unroll
  for (int q = 11; q < 15; q++) w[q] = 0;
  w[15] = (48 + 8 + KZG_BYTES_PER_CELL + 48) * 8;
  sha256_block_rolled(s, w);
  status_cell[k] = BLOB ? blob_status[k >> 7] : (bad ? KZG_ERR_BLOB_INVALID_FIELD_ELEMENT : 0);
#pragma unroll
  for (int q = 0; q < 8; q++) leaves[k * 8 + q] = s.h[q];
  {  // z, y and the index's status last, from the index read anew: nothing of them is held through the hash
    const unsigned long long column = BLOB ? (unsigned long long)(k & 127u) : cell_indices[k];
    const bool good = column < (unsigned long long)KZG_CELLS_PER_EXT_BLOB;
    const uint4* h = reinterpret_cast<const uint4*>(h64_plain + (good ? (uint32_t)column : 0u));
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4 h0 = h[0], h1 = h[1];  // row 0 for a rejected index: loaded all the same, then masked
    const uint32_t keep = good ? ~0u : 0u;
    uint4* zd = reinterpret_cast<uint4*>(z_plain + k);
    uint4* yd = reinterpret_cast<uint4*>(y_plain + k);
    zd[0] = make_uint4(h0.x & keep, h0.y & keep, h0.z & keep, h0.w & keep);
    zd[1] = make_uint4(h1.x & keep, h1.y & keep, h1.z & keep, h1.w & keep);
    yd[0] = zero;
    yd[1] = zero;
    int32_t code = good ? 0 : KZG_ERR_CELL_INDEX;
    if (ROWS && !BLOB && commitment_indices[k] >= ncom) code = KZG_ERR_COMMITMENT_INDEX;
    status_index[k] = code;
  }
}
static __global__ __launch_bounds__(256, 8) void k_cells_leaves(const uint8_t* __restrict__ commitments48, const unsigned long long* __restrict__ cell_indices,
                                                                const uint8_t* __restrict__ cells, const uint8_t* __restrict__ proofs48, uint64_t n,
                                                                const fr_t* __restrict__ h64_plain, fr_t* __restrict__ z_plain, fr_t* __restrict__ y_plain,
                                                                int32_t* __restrict__ status_index, int32_t* __restrict__ status_cell,
                                                                uint32_t* __restrict__ leaves /* n x 8 words */) {
  cells_leaves_body<false>(commitments48, nullptr, 0, cell_indices, cells, proofs48, n, h64_plain, z_plain, y_plain, status_index, status_cell, leaves);
}
// the row-indexed form's front (kzg_verify_cell_proof_batch_rows): the same budget beside two decoder waves, asserted by
// tests/test_cellverify_rows_host.py
static __global__ __launch_bounds__(256, 8) void k_cells_rows_leaves(const uint8_t* __restrict__ commitments48 /* ncom x 48 */,
                                                                     const unsigned long long* __restrict__ commitment_indices, uint64_t ncom,
                                                                     const unsigned long long* __restrict__ cell_indices, const uint8_t* __restrict__ cells,
                                                                     const uint8_t* __restrict__ proofs48, uint64_t n, const fr_t* __restrict__ h64_plain,
                                                                     fr_t* __restrict__ z_plain, fr_t* __restrict__ y_plain, int32_t* __restrict__ status_index,
                                                                     int32_t* __restrict__ status_cell, uint32_t* __restrict__ leaves /* n x 8 words */) {
  cells_leaves_body<true>(commitments48, commitment_indices, ncom, cell_indices, cells, proofs48, n, h64_plain, z_plain, y_plain, status_index, status_cell, leaves);
}
// the blob form's front (kzg_verify_blob_cell_proofs_batch): the same budget beside two decoder waves, asserted by
// tests/test_blob_cell_proofs_host.py
static __global__ __launch_bounds__(256, 8) void k_blob_cells_leaves(const uint8_t* __restrict__ commitments48 /* n / 128 x 48 */, const uint8_t* __restrict__ blobs,
                                                                     const uint8_t* __restrict__ ext, const int32_t* __restrict__ blob_status,
                                                                     const uint8_t* __restrict__ proofs48, uint64_t n, const fr_t* __restrict__ h64_plain,
                                                                     fr_t* __restrict__ z_plain, fr_t* __restrict__ y_plain, int32_t* __restrict__ status_index,
                                                                     int32_t* __restrict__ status_cell, uint32_t* __restrict__ leaves /* n x 8 words */) {
  cells_leaves_body<true, true>(commitments48, nullptr, n >> 7, nullptr, blobs, proofs48, n, h64_plain, z_plain, y_plain, status_index, status_cell, leaves, ext,
                                blob_status);
}

// The row-indexed form's commitment scalars  w_c = sum_{k : index_k = c} r^k  (cellverify_math.cuh), commitment-major: workgroup
// (c, tile) -- lane t strides over the tile's indices (8-byte coalesced loads, the same lines for every c: the L2 serves them), adds
// r^k (plain, k_batch_scalars' lincomb A scalar) on a match, then an LDS tree.  No atomics: every sum has a fixed order, and Fr addition
// is exact, so any order gives the same canonical value.  An item whose index status is non-zero is skipped (an index >= ncom matches
// no workgroup anyway); nothing is indexed BY an index.  n u / 64 wave-steps: nothing for a block's shape, about a millisecond at
// u = n = 65,536, where the per-cell call is the one to use.
static __global__ __launch_bounds__(CELLV_ROWW_THREADS) void k_cells_row_weights(const unsigned long long* __restrict__ commitment_indices,
                                                                                 const int32_t* __restrict__ status_index /* null: none */,
                                                                                 const fr_t* __restrict__ rpow_plain, uint64_t n, uint64_t tile,
                                                                                 fr_t* __restrict__ partials /* gridDim.x x gridDim.y */) {
  __shared__ fr_t red[CELLV_ROWW_THREADS];
  const uint32_t t = threadIdx.x;
  const uint64_t lo = (uint64_t)blockIdx.y * tile, hi = lo + tile < n ? lo + tile : n;
  fr_t acc;
  cellv_roww_thread(acc, commitment_indices, status_index, rpow_plain, lo, hi, t, (uint64_t)blockIdx.x);
  red[t] = acc;
  __syncthreads();
  for (uint32_t w = CELLV_ROWW_THREADS / 2; w >= 1; w >>= 1) {
    if (t < w) cellv_roww_fold(red, t, w);
    __syncthreads();
  }
  if (t == 0) partials[(uint64_t)blockIdx.x * gridDim.y + blockIdx.y] = red[0];
}
// w_c = the sum of commitment c's tile partials in tile order, into lincomb B's commitment slots: one thread per commitment
static __global__ __launch_bounds__(256) void k_cells_roww_reduce(const fr_t* __restrict__ partials, uint32_t tiles, uint64_t ncom, fr_t* __restrict__ out_plain) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncom) return;
  fr_t out;
  cellv_roww_sum(out, partials + c * tiles, tiles);
  out_plain[c] = out;
}

// The row-indexed form's k_each_status (kzg_verify_cell_proof_batch_rows_each): ONE launch over max(n, ncom) threads.  Thread i < n
// folds item i's code THROUGH its commitment index (cellv_rows_item_status: the commitment slot is read only behind a clear index slot)
// and counts the rejected items in counts[0], as k_each_status does; thread c < ncom counts the rejected LISTED commitments in
// counts[1], referenced or not -- the driver must not hand a rejected point to the batch check's lincomb, and the call's *ok is 0 for a
// bad list.  The ncom commitment statuses themselves are read back from the session's array, only when the caller asks for them.
static __global__ __launch_bounds__(256) void k_each_rows_status(const int32_t* __restrict__ st_index, const int32_t* __restrict__ st_com,
                                                                const int32_t* __restrict__ st_cell, const int32_t* __restrict__ st_proof,
                                                                const unsigned long long* __restrict__ commitment_indices, uint64_t ncom, uint64_t n,
                                                                int32_t* __restrict__ status /* n */, uint32_t* __restrict__ counts /* 2 */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int32_t c = cellv_rows_item_status(st_index, st_com, st_cell, st_proof, commitment_indices, ncom, i);
    status[i] = c;
    if (c) atomicAdd(counts, 1u);
  }
  if (i < ncom && st_com[i]) atomicAdd(counts + 1, 1u);
}

// The blob form's commitment scalars (kzg_verify_blob_cell_proofs_batch): with implicit indices  w_b = sum_{k<128} r^(128 b + k)  is a
// contiguous segment sum -- one 128-thread workgroup per blob, thread k takes r^(128 b + k) (plain, k_batch_scalars' lincomb A scalar)
// and the tree of k_cells_row_weights (cellv_roww_fold) sums them.  Fr addition is exact, so the value is the one k_cells_row_weights
// gives for the explicit index array (kzg_blob_cell_weights against kzg_cell_row_weights: the test).
static __global__ __launch_bounds__(CELLV_BLOB_ITEMS) void k_blob_weights(const fr_t* __restrict__ rpow_plain /* 128 x gridDim.x */,
                                                                         fr_t* __restrict__ out_plain /* gridDim.x */) {
  __shared__ fr_t red[CELLV_BLOB_ITEMS];
  const uint32_t t = threadIdx.x;
  red[t] = rpow_plain[(uint64_t)blockIdx.x * CELLV_BLOB_ITEMS + t];
  __syncthreads();
  for (uint32_t w = CELLV_BLOB_ITEMS / 2; w >= 1; w >>= 1) {
    if (t < w) cellv_roww_fold(red, t, w);
    __syncthreads();
  }
  if (t == 0) out_plain[blockIdx.x] = red[0];
}

// The blob form's k_each_status (kzg_verify_blob_cell_proofs_batch_each): one 128-thread workgroup per blob folds (blob status,
// commitment status, 128 proof statuses) to the blob's code (cellv_blob_code: the lowest rejected proof through an LDS minimum) and
// writes it to ALL 128 items of the blob -- the terms kernel and the vector tree's leaves skip every item whose status is non-zero, so
// nothing of a rejected blob enters lincomb A, lincomb B or the vector tree -- and to blob_code[b], the caller's status[b].
// counts[0]: the rejected BLOBS.
static __global__ __launch_bounds__(CELLV_BLOB_ITEMS) void k_each_blob_status(const int32_t* __restrict__ st_blob, const int32_t* __restrict__ st_com,
                                                                             const int32_t* __restrict__ st_proof, int32_t* __restrict__ status /* 128 x gridDim.x */,
                                                                             int32_t* __restrict__ blob_code /* gridDim.x */, uint32_t* __restrict__ counts) {
  __shared__ uint32_t first;
  const uint32_t t = threadIdx.x;
  const uint64_t b = blockIdx.x, i = b * CELLV_BLOB_ITEMS + t;
  if (t == 0) first = CELLV_BLOB_ITEMS;
  __syncthreads();
  if (st_proof[i]) atomicMin(&first, t);
  __syncthreads();
  const int32_t c = cellv_blob_code(st_blob[b], st_com[b], st_proof + b * CELLV_BLOB_ITEMS, first);
  status[i] = c;
  if (t == 0) {
    blob_code[b] = c;
    if (c) atomicAdd(counts, 1u);
  }
}

// elements 8 t .. 8 t + 7 of cell k as they lie in memory (256 consecutive bytes, big-endian) -> plain limbs; zero for a cell that
// contributes nothing
__device__ __forceinline__ void cellv_load_elements(fr_t (&v)[8], const uint8_t* __restrict__ cells, uint64_t k, uint32_t t, bool live) {
  const uint4* in = reinterpret_cast<const uint4*>(cells + (live ? k : 0) * (uint64_t)KZG_BYTES_PER_CELL) + 16u * t;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4 w0 = live ? in[2 * e] : zero, w1 = live ? in[2 * e + 1] : zero;
    v[e].v[7] = __builtin_bswap32(w0.x);
    v[e].v[6] = __builtin_bswap32(w0.y);
    v[e].v[5] = __builtin_bswap32(w0.z);
    v[e].v[4] = __builtin_bswap32(w0.w);
    v[e].v[3] = __builtin_bswap32(w1.x);
    v[e].v[2] = __builtin_bswap32(w1.y);
    v[e].v[1] = __builtin_bswap32(w1.z);
    v[e].v[0] = __builtin_bswap32(w1.w);
  }
}

// S's partial vectors: one 128-thread workgroup per CELLV_CELLS cells, eight threads per cell.  A thread reads its eight elements (256
// consecutive bytes, the cell's second and last trip from memory: 2 x 2 KiB per cell in all), runs the three steps of
// cellverify_math.cuh with a barrier between them and the first 64 threads store the workgroup's 64 partial coefficients.  A cell
// whose index or elements were rejected (the front's status words), and the cells past the batch's end in the last workgroup,
// contribute zero.  r^k is lincomb A's scalar of item k as k_batch_scalars left it (plain).  No atomics: every sum has a fixed order.
// BLOB (k_blob_cells_interp, the blob form): the column is k & 127 and the cell lies where cellv_blob_cell says -- `cells` are the
// blobs, `ext` the extension workspace, the index pointer is null and never read; the eight threads of a cell share the choice.  The
// body is shared; k_cells_interp is its BLOB = false instance and compiles to what it was.
template <bool BLOB>
__device__ __forceinline__ void cells_interp_body(uint32_t* __restrict__ img, const uint8_t* __restrict__ cells, const uint8_t* __restrict__ ext,
                                                  const unsigned long long* __restrict__ cell_indices, const int32_t* __restrict__ status_index,
                                                  const int32_t* __restrict__ status_cell, const fr_t* __restrict__ rpow_plain, uint64_t n,
                                                  const uint32_t* __restrict__ ctab, const uint32_t* __restrict__ vtab, fr_t* __restrict__ partials) {
  const uint32_t cl = threadIdx.x >> 3, t = threadIdx.x & 7u;
  const uint64_t k = (uint64_t)blockIdx.x * CELLV_CELLS + cl;
  bool live = k < n;
  if (live) live = status_index[k] == 0 && status_cell[k] == 0;
  const uint32_t column = live ? (BLOB ? (uint32_t)(k & 127u) : (uint32_t)cell_indices[k]) : 0u;
  fr_t rk;
  {
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4* src = reinterpret_cast<const uint4*>(rpow_plain + (live ? k : 0));
    const uint4 lo = live ? src[0] : zero, hi = live ? src[1] : zero;
    rk.v[0] = lo.x; rk.v[1] = lo.y; rk.v[2] = lo.z; rk.v[3] = lo.w;
    rk.v[4] = hi.x; rk.v[5] = hi.y; rk.v[6] = hi.z; rk.v[7] = hi.w;
  }
  {
    fr_t v[8];
    if (BLOB)
      cellv_load_elements(v, cellv_blob_cell(cells, ext, live ? k : 0), 0, t, live);
    else
      cellv_load_elements(v, cells, k, t, live);
    cellv_step_a(img, ctab, cl, t, v);
  }
  __syncthreads();
  cellv_step_b(img, ctab, vtab, cl, t, column, rk);
  __syncthreads();
  if (threadIdx.x < 64) {
    fr_t sum;
    cellv_step_c(sum, img, threadIdx.x);
    partials[(uint64_t)blockIdx.x * 64 + threadIdx.x] = sum;
  }
}
static __global__ __launch_bounds__(CELLV_THREADS) void k_cells_interp(const uint8_t* __restrict__ cells, const unsigned long long* __restrict__ cell_indices,
                                                                   const int32_t* __restrict__ status_index, const int32_t* __restrict__ status_cell,
                                                                   const fr_t* __restrict__ rpow_plain, uint64_t n, const uint32_t* __restrict__ ctab,
                                                                   const uint32_t* __restrict__ vtab, fr_t* __restrict__ partials /* gridDim.x x 64 */) {
  __shared__ uint32_t img[CELLV_IMAGE_DWORDS];
  cells_interp_body<false>(img, cells, nullptr, cell_indices, status_index, status_cell, rpow_plain, n, ctab, vtab, partials);
}
// the blob form's instance (kzg_verify_blob_cell_proofs_batch); figures asserted by tests/test_blob_cell_proofs_host.py
static __global__ __launch_bounds__(CELLV_THREADS) void k_blob_cells_interp(const uint8_t* __restrict__ blobs, const uint8_t* __restrict__ ext,
                                                                        const int32_t* __restrict__ status_index, const int32_t* __restrict__ status_cell,
                                                                        const fr_t* __restrict__ rpow_plain, uint64_t n, const uint32_t* __restrict__ ctab,
                                                                        const uint32_t* __restrict__ vtab, fr_t* __restrict__ partials /* gridDim.x x 64 */) {
  __shared__ uint32_t img[CELLV_IMAGE_DWORDS];
  cells_interp_body<true>(img, blobs, ext, nullptr, status_index, status_cell, rpow_plain, n, ctab, vtab, partials);
}

// -S_j = -(sum of the partial vectors), j < 64, into the 64 scalar slots of lincomb B's monomial terms.  One workgroup: four threads
// per coefficient take every fourth partial vector, thread j adds the four in their order.
static __global__ __launch_bounds__(256) void k_cells_reduce(const fr_t* __restrict__ partials, uint32_t count, fr_t* __restrict__ out_neg_plain /* 64 */) {
  __shared__ fr_t red[256];
  const uint32_t j = threadIdx.x & 63u, g = threadIdx.x >> 6;
  fr_t acc;
  bn_zero(acc);
  for (uint32_t k = g; k < count; k += 4) fr_add(acc, acc, partials[(uint64_t)k * 64 + j]);
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    fr_t out;
    cellv_neg_sum(out, red + j, 4, 64);
    out_neg_plain[j] = out;
  }
}


// ---- per-item verdicts for cells (kzg_verify_cell_proof_batch_each): the monomial term of the batch check item by item ----------------
//   B_i = [r_i] C_i + [r_i h_i^64] proof_i - sum_j [v_ij] [tau^j]_1,   v_i = r_i I_i (64 coefficients)
// The two point terms are k_each_terms' (the front wrote z = h^64, y = 0).  The 64-term sum is NOT taken per item: the v_i are the
// leaves of a third sum tree whose nodes are 64 Fr values, and the points  T = sum_j [S_j] [tau^j]_1  are computed only for the nodes
// the host asks for (k_each_gather_cells).

// Leaf vectors: k_cells_interp's workgroup (16 cells, eight threads each, the same three steps and tables) with the scaled coefficients
// stored per cell instead of summed.  r_i = r^(first_index + i) comes from the seed's powers r^(2^k) (Montgomery) as in k_each_terms:
// on the rejected-items route k_batch_scalars has not run.  An item whose single-item code is non-zero (status: k_each_status' output,
// which covers the index and the elements) contributes the zero vector.
// BLOB (k_blob_cells_each_leaves, the blob form): column and cell address as in cells_interp_body<true>; k_cells_each_leaves is the
// BLOB = false instance and compiles to what it was.
template <bool BLOB>
__device__ __forceinline__ void cells_each_leaves_body(uint32_t* __restrict__ img, const uint8_t* __restrict__ cells, const uint8_t* __restrict__ ext,
                                                       const unsigned long long* __restrict__ cell_indices, const int32_t* __restrict__ status,
                                                       const fr_t* __restrict__ rpow2, uint64_t n, uint64_t first_index, const uint32_t* __restrict__ ctab,
                                                       const uint32_t* __restrict__ vtab, fr_t* __restrict__ leaves) {
  const uint32_t cl = threadIdx.x >> 3, t = threadIdx.x & 7u;
  const uint64_t k = (uint64_t)blockIdx.x * CELLV_CELLS + cl;
  bool live = k < n;
  if (live) live = status[k] == 0;
  const uint32_t column = live ? (BLOB ? (uint32_t)(k & 127u) : (uint32_t)cell_indices[k]) : 0u;
  fr_t rk;
  bn_zero(rk);
  if (live) {
    const uint64_t e = first_index + k;
    fr_t r = fr_one();
    for (int b = 0; b < 64 && (e >> b); b++)
      if ((e >> b) & 1) fr_mul(r, r, rpow2[b]);
    from_mont<FrParams>(rk, r);
  }
  {
    fr_t v[8];
    if (BLOB)
      cellv_load_elements(v, cellv_blob_cell(cells, ext, live ? k : 0), 0, t, live);
    else
      cellv_load_elements(v, cells, k, t, live);
    cellv_step_a(img, ctab, cl, t, v);
  }
  __syncthreads();
  cellv_step_b(img, ctab, vtab, cl, t, column, rk);
  __syncthreads();
  // 16 x 64 coefficients, eight per thread: consecutive threads store consecutive coefficients of one cell
#pragma unroll 1
  for (uint32_t q = 0; q < 8; q++) {
    const uint32_t flat = threadIdx.x + (uint32_t)CELLV_THREADS * q, c2 = flat >> 6, j = flat & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * CELLV_CELLS + c2;
    if (item >= n) continue;
    fr_t o;
    cellv_cell_coeff(o, img, c2, j);
    leaves[item * 64 + j] = o;
  }
}
static __global__ __launch_bounds__(CELLV_THREADS) void k_cells_each_leaves(const uint8_t* __restrict__ cells, const unsigned long long* __restrict__ cell_indices,
                                                                        const int32_t* __restrict__ status, const fr_t* __restrict__ rpow2, uint64_t n,
                                                                        uint64_t first_index, const uint32_t* __restrict__ ctab, const uint32_t* __restrict__ vtab,
                                                                        fr_t* __restrict__ leaves /* n x 64, plain, canonical */) {
  __shared__ uint32_t img[CELLV_IMAGE_DWORDS];
  cells_each_leaves_body<false>(img, cells, nullptr, cell_indices, status, rpow2, n, first_index, ctab, vtab, leaves);
}
static __global__ __launch_bounds__(CELLV_THREADS) void k_blob_cells_each_leaves(const uint8_t* __restrict__ blobs, const uint8_t* __restrict__ ext,
                                                                             const int32_t* __restrict__ status, const fr_t* __restrict__ rpow2, uint64_t n,
                                                                             uint64_t first_index, const uint32_t* __restrict__ ctab,
                                                                             const uint32_t* __restrict__ vtab, fr_t* __restrict__ leaves /* n x 64 */) {
  __shared__ uint32_t img[CELLV_IMAGE_DWORDS];
  cells_each_leaves_body<true>(img, blobs, ext, nullptr, status, rpow2, n, first_index, ctab, vtab, leaves);
}

// one level of the vector tree: out[j] = in[2 j] + in[2 j + 1] coefficient by coefficient, a missing sibling being zero; one thread per
// coefficient, k_each_level's geometry
static __global__ __launch_bounds__(256) void k_each_vec_level(const fr_t* __restrict__ in, uint64_t cnt_in, fr_t* __restrict__ out, uint64_t cnt_out) {
  const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= cnt_out * 64) return;
  const uint64_t j = id >> 6, c = id & 63u;
  fr_t acc = in[2 * j * 64 + c];
  if (2 * j + 1 < cnt_in) cellv_vec_add(acc, in[(2 * j + 1) * 64 + c]);
  out[id] = acc;
}

// The fetch of the cells kind: ONE WAVE PER REQUESTED NODE.  Lane j multiplies the monomial point M_j (affine, lincomb B's format) by
// the node's coefficient S_j -- a 255-step double-and-add as in k_each_terms, the doubling uniform over the wave, the addition masked
// by the lane's scalar bit -- and a six-step tree of complete additions through LDS sums the 64 products: T.  Lane 0 then adds B'
// (the node of k_each_terms' tree B) and lanes 0 and 1 write B' -+ T and A in the 12 x 32-limb host format, as k_each_gather does.
// `subtract` loads the bases negated (B' - T, the verdicts); without it the sum is B' + T (kzg_g1_monomial_lincomb).  tree_a / tree_b
// null: the identity in their place; idx null: node k is vector k.  S_j = 0 leaves the lane's accumulator at the identity, the zero
// vector gives T = identity, T = B' cancels in the complete adder.  Grid: exactly m workgroups.
static __global__ __launch_bounds__(64, 2) void k_each_gather_cells(const g1_xyzz28* __restrict__ tree_a, const g1_xyzz28* __restrict__ tree_b,
                                                                   const fr_t* __restrict__ vecs, const uint4* __restrict__ monomial,
                                                                   const uint32_t* __restrict__ idx, uint32_t m, bool subtract, g1_xyzz* __restrict__ out) {
  __shared__ g1_xyzz28 lds[32];
  const uint32_t node = blockIdx.x, lane = threadIdx.x;
  if (node >= m) return;  // uniform over the workgroup
  const uint64_t pos = idx ? idx[node] : node;
  fr_t s = vecs[pos * 64 + lane];
  fp28 cx, cy;
  {
    fp_t px, py;
    load_affine96(px, py, monomial, lane);
    if (bn_is_zero(px) && bn_is_zero(py)) bn_zero(s);  // a point at infinity (a context never holds one: ensure_g1_monomial rejects the setup)
    f28_load_entry(cx, cy, px, py, subtract);
  }
  g1_xyzz28 acc;
  xyzz28_set_inf(acc);
  // the scalar is below r < 2^255: bit 255 is dropped, 255 steps, bit 254 first
  auto shl1 = [](fr_t& v) {
#pragma unroll
    for (int q = 7; q > 0; q--) v.v[q] = (v.v[q] << 1) | (v.v[q - 1] >> 31);
    v.v[0] <<= 1;
  };
  shl1(s);
#pragma unroll 1
  for (int step = 0; step < 255; step++) {
    xyzz28_dbl_inl(acc);
    if (s.v[7] >> 31) {
      bool done = false;
      if (!acc.inf) done = xyzz28_madd_fast(acc, cx, cy);
      if (!done) {
        g1_xyzz28 tmp = acc;  // copy: the call takes addresses
        xyzz28_madd_complete(tmp, cx, cy);
        acc = tmp;
      }
    }
    shl1(s);
  }
#pragma unroll 1
  for (uint32_t step = 32; step >= 1; step >>= 1) {
    if (lane >= step && lane < 2 * step) lds[lane - step] = acc;
    __syncthreads();
    if (lane < step) {
      const g1_xyzz28 other = lds[lane];
      xyzz28_add_complete_inl<true>(acc, other);
    }
    __syncthreads();
  }
  if (lane >= 2) return;
  g1_xyzz28 p;
  xyzz28_set_inf(p);
  if (lane == 0) {
    if (tree_b) p = tree_b[pos];
    xyzz28_add_complete_inl<true>(p, acc);
  } else if (tree_a) {
    p = tree_a[pos];
  }
  g1_xyzz o;
  xyzz28_to_xyzz(o, p);
  out[2 * node + (lane ^ 1u)] = o;
}

#endif
}  // namespace kzg
