// The producers behind the commitment: blob proofs and proofs at a point, the blob sidecar, and the cell calls of EIP-7594 (compute_cells,
// recover_cells and their cell proofs) -- entry points, host-buffer drivers and the kernels they alone launch
#include <algorithm>

#include "engine_internal.hpp"
#include "cellproof_plan.hpp"  // the select calls' pair list and pass plan: host logic
#include "poly_kernels.cuh"  // this translation unit owns the quotient / evaluation kernels of the proof path
#include "cells_kernels.cuh"  // ... and the blob extension kernel of compute_cells
#include "cellproof_kernels.cuh"  // ... and the quotient vectors of the cell proofs

__global__ __launch_bounds__(256) void k_merge_status(int32_t* __restrict__ primary, const int32_t* __restrict__ secondary, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && primary[i] == 0) primary[i] = secondary[i];
}

// workspace of a proof call over n items: chunks of cn items, two slots of per-chunk preparation results (z, 1/(z^4096 - 1), y,
// commitment statuses, quotient scalars) and one set of MSM buffers
struct ProofLayout {
  uint64_t cn = 0;
  size_t o_z[2], o_y[2], o_cs[2], o_q[2], o_ir[2], total = 0;
  MsmBufs msm;
};
static ProofLayout proof_layout(const kzg_ctx* ctx, uint64_t n) {
  ProofLayout L;
  const uint64_t chunk_max = ctx->knobs.proof_chunk ? ctx->knobs.proof_chunk : 16384;
  L.cn = n < chunk_max ? n : chunk_max;
  Carve ws;
  for (int sl = 0; sl < 2; sl++) {
    L.o_z[sl] = ws.take(L.cn * sizeof(fr_t));
    L.o_ir[sl] = ws.take(2 * L.cn * sizeof(fr_t));  // per blob: 1 / prod (z - w_i) and (z^4096 - 1) / 4096
    L.o_y[sl] = ws.take(L.cn * sizeof(fr_t));
    L.o_cs[sl] = ws.take(L.cn * sizeof(int32_t));
    L.o_q[sl] = ws.take(L.cn * 4096 * sizeof(fr_t));
  }
  L.msm = msm_carve(ctx, ws, L.cn);
  L.total = ws.off;
  return L;
}

// proofs for n (blob, commitment) or (blob, z) items resident on the device.
//   d_commitments48 != null : blob proofs (z from the Fiat-Shamir challenge)
//   d_z32 != null           : proofs at caller-supplied points; y written to d_y32
static int32_t proof_dev_locked(const kzg_ctx* ctx, const uint8_t* d_blobs, const uint8_t* d_commitments48, const uint8_t* d_z32, uint64_t n,
                                uint8_t* d_out48, uint8_t* d_out_affine96, uint8_t* d_y32, int32_t* d_status, hipStream_t st) {
  if (n == 0) return 0;
  // Chunks of up to 16,384 blobs (quotient scratch: 128 KiB per blob = 2 GiB per chunk).  The per-chunk preparation
  // starts with ~6 ms of pure latency (one SHA-256 stream per blob, 2,050 sequential blocks) during which the GPU is
  // almost idle, and it cannot be hidden behind the previous chunk's MSM: that launch keeps every wave slot filled
  // with its own queued waves until it ends (a second stream, also at the highest stream priority, only got going
  // when the MSM finished).  So FEW, LARGE chunks win -- measured at n = 16,384, c = 12: 4 x 4,096 serial 244 ms,
  // 4 x 4,096 on two streams 242 ms, 2 x 8,192 224 ms, 8 x 2,048 279 ms (profiles/r01/proof_pipeline_variants.txt).
  // The two-stream pipeline stays selectable (KATETH_AMD_PROOF_OVERLAP=1, KATETH_AMD_PROOF_CHUNK).
  bool overlap = ctx->knobs.proof_overlap > 0;
  const ProofLayout L = proof_layout(ctx, n);
  const uint64_t cn = L.cn, nchunks = (n + cn - 1) / cn;
  int32_t rc = ws_reserve(ctx, L.total, st);
  if (rc) return rc;
  uint8_t* ws = ws_ptr(ctx);
  const size_t *o_z = L.o_z, *o_y = L.o_y, *o_cs = L.o_cs, *o_q = L.o_q, *o_ir = L.o_ir;
  hipStream_t side = overlap ? ctx->side_stream : st;
  // events come from the context's pool (guarded by ctx->lock, which the caller holds): 4 per chunk + 1, created once
  std::vector<hipEvent_t>& pool = ctx->proof_events;
  while (pool.size() < 4 * nchunks + 1) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(KZG_FAIL_HIP, "event create failed");
    pool.push_back(e);
  }
  hipEvent_t* ev_prep = pool.data();
  hipEvent_t* ev_done = pool.data() + nchunks;
  hipEvent_t* ev_fork = pool.data() + 2 * nchunks;
  hipEvent_t* ev_join = pool.data() + 3 * nchunks;
  hipEvent_t ev_start = pool[4 * nchunks];
  HIP_TRY(hipMemsetAsync(d_status, 0, n * sizeof(int32_t), st));
  (void)hipEventRecord(ev_start, st);
  (void)hipStreamWaitEvent(side, ev_start, 0);
  auto prep = [&](uint64_t k) {  // enqueue chunk k's preparation on the side stream
    const int sl = (int)(k & 1);
    const uint64_t base = k * cn;
    const uint64_t m = (n - base < cn) ? (n - base) : cn;
    fr_t* z = reinterpret_cast<fr_t*>(ws + o_z[sl]);
    fr_t* y = reinterpret_cast<fr_t*>(ws + o_y[sl]);
    fr_t* invr = reinterpret_cast<fr_t*>(ws + o_ir[sl]);
    int32_t* cstat = reinterpret_cast<int32_t*>(ws + o_cs[sl]);
    fr_t* q = reinterpret_cast<fr_t*>(ws + o_q[sl]);
    const uint8_t* blobs = d_blobs + base * (uint64_t)KZG_BYTES_PER_BLOB;
    if (k >= 2) (void)hipStreamWaitEvent(side, ev_done[k - 2], 0);  // slot reuse
    (void)hipMemsetAsync(cstat, 0, m * sizeof(int32_t), side);
    if (d_commitments48) {
      const uint8_t* com = d_commitments48 + base * 48;
      if (fused_prep_fits(ctx, m, m)) {
        // commitment check and SHA-256 challenge in one launch: both are long per-lane dependency chains and must not share SIMDs
        launch_challenge_and_decode(ctx, side, blobs, com, m, z, com, m, cstat, (const uint8_t*)nullptr, (uint64_t)0, (int32_t*)nullptr, (uint4*)nullptr,
                                    (uint8_t*)nullptr);
      } else {
        // chunks above the fused-launch limit: the commitment check (one lane per point) runs beside the SHA-256
        // challenge on a second stream
        hipStream_t dec = overlap ? side : ctx->side_stream;
        if (dec != side) {
          (void)hipEventRecord(ev_fork[k], side);
          (void)hipStreamWaitEvent(dec, ev_fork[k], 0);
        }
        launch_g1_decompress(dec, com, m, cstat, (const uint8_t*)nullptr, (uint64_t)0, (int32_t*)nullptr, (uint4*)nullptr, (uint8_t*)nullptr);
        if (dec != side) (void)hipEventRecord(ev_join[k], dec);
        launch_challenge(ctx, side, blobs, com, m, z);
        if (dec != side) (void)hipStreamWaitEvent(side, ev_join[k], 0);
      }
    } else {
      launch_fr_parse(side, d_z32 + base * 32, m, z, cstat);
    }
    {
      ProfScope ps(ctx, PROF_POLY, side);
      hipLaunchKernelGGL(k_poly_root_inverse, dim3(blocks_for(m, 64)), dim3(64), 0, side, z, m, invr);
      hipLaunchKernelGGL(k_poly<true>, dim3((unsigned)m), dim3(512), 0, side, blobs, z, ctx->d_roots_brp, invr, y, q, d_status + base);
    }
    hipLaunchKernelGGL(k_merge_status, dim3(blocks_for(m, 256)), dim3(256), 0, side, d_status + base, cstat, m);
    (void)hipEventRecord(ev_prep[k], side);
  };
  if (rc == 0) {
    prep(0);
    for (uint64_t k = 0; k < nchunks; k++) {
      if (k + 1 < nchunks) prep(k + 1);
      const int sl = (int)(k & 1);
      const uint64_t base = k * cn;
      const uint64_t m = (n - base < cn) ? (n - base) : cn;
      fr_t* y = reinterpret_cast<fr_t*>(ws + o_y[sl]);
      fr_t* q = reinterpret_cast<fr_t*>(ws + o_q[sl]);
      (void)hipStreamWaitEvent(st, ev_prep[k], 0);
      rc = msm_pipeline(ctx, false, reinterpret_cast<const uint8_t*>(q), m, d_out48 ? d_out48 + base * 48 : nullptr,
                               d_out_affine96 ? d_out_affine96 + base * 96 : nullptr, d_status + base, L.msm, ws, st);
      if (rc) break;
      if (d_y32) launch_fr_store_be(st, y, m, d_status + base, d_y32 + base * 32);
      (void)hipEventRecord(ev_done[k], st);
    }
    if (rc == 0 && hipGetLastError() != hipSuccess) rc = fail(KZG_FAIL_HIP, "proof pipeline launch failed");
  }
  if (rc != 0) (void)hipStreamSynchronize(side);
  return rc;
}

extern "C" int32_t kzg_compute_blob_proof_batch_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, uint64_t n,
                                                    void* d_out48, void* d_status, void* hip_stream) try {
  if (!ctx || (n && (!d_blobs || !d_commitments48 || !d_out48 || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  return with_workspace(ctx, st, [&] {
    return proof_dev_locked(ctx, (const uint8_t*)d_blobs, (const uint8_t*)d_commitments48, nullptr, n, (uint8_t*)d_out48, nullptr, nullptr, (int32_t*)d_status, st);
  });
} catch (...) {
  return abi_exception();
}

// Host-buffer wrapper shared by the proof entry points.  Device buffers come from the context's pools (stage_lock): two
// staging slots of up to 4,096 blobs, the small inputs and results in the host-i/o pool -- a steady-state call allocates
// nothing.
//
// The batch is walked in PASSES, double-buffered: while the device path (proof_dev_locked: hash + commitment check,
// evaluation + quotient, MSM, encoding) works on pass k on the compute stream, pass k+1 is copied in on the copy stream --
// events only, the host never waits inside the loop.  Passes are 4,096 blobs (the MSM's most efficient shape); batches
// above 5,120 blobs start with a pass of 1,024 so that only 2.3 ms of the transfer are exposed.  16,384 blobs: 105.3 k
// blobs/s (99.8 k with "copy everything, then compute"); up to 5,120 blobs one pass: copy, then compute (87-92 k at 4,096).
// Measured alternatives at 4,096 blobs (round 3, profiles/r03/host_proof_variants.json): one pass 46.2 ms; passes of 1,024 +
// 3,072: 47.0 ms (the second hash latency costs what the hidden copy saves); a pipeline of 1,024-blob chunks on four
// streams, every chunk's MSM as one wave per SIMD: 44.7 ms at 4,096 but 170 ms at 16,384 -- the short kernels of later chunks
// (k_poly: 8-wave workgroups of 126 VGPRs) find no register space beside two resident MSM chunks (2 x 232 VGPRs per SIMD)
// and wait for a whole chunk to drain, so the pipeline degenerates to two-deep serial passes.
static std::vector<uint64_t> proof_host_plan(uint64_t n) {
  constexpr uint64_t PASS = 4096;
  std::vector<uint64_t> plan;
  uint64_t rest = n;
  if (n > PASS + 1024) {  // a short first pass only where later passes can hide behind it (measured: at 4,096 blobs two passes cost what they save)
    plan.push_back(1024);
    rest -= 1024;
  }
  for (; rest > PASS; rest -= PASS) plan.push_back(PASS);
  if (rest) plan.push_back(rest);
  return plan;
}
int32_t proof_host(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* side, size_t side_bytes, bool side_is_commitment, uint64_t n,
                          uint8_t* out48, uint8_t* out_affine96, uint8_t* out_y32, int32_t* status) {
  if (n == 0) return 0;
  HostCall hc(ctx);
  const int a_side = hc.upload(side, n * side_bytes), a_out = hc.download(out48, n * 48), a_aff = hc.download(out_affine96, n * 96),
            a_y = hc.download(out_y32, n * 32), a_st = hc.download(status, n * sizeof(int32_t));
  int32_t rc = hc.open(proof_host_plan(n), KZG_BYTES_PER_BLOB);  // one pass: nothing to overlap, the copy rides on the compute stream
  if (rc) return rc;
  uint8_t *d_side = hc.dev(a_side), *d_out = hc.dev(a_out), *d_aff = hc.dev(a_aff), *d_y = hc.dev(a_y);
  int32_t* d_status = hc.dev<int32_t>(a_st);
  // one workspace slot for all passes (they follow each other on the call's stream), sized for the largest pass BEFORE anything is in
  // flight: growing it between passes would free memory under the pipeline
  rc = with_workspace(ctx, hc.st, [&] {
    const int32_t e = ws_reserve(ctx, proof_layout(ctx, hc.max_pass).total, hc.st);
    if (e) return e;
    return hc.passes(blobs, KZG_BYTES_PER_BLOB, [&](size_t, uint64_t base, uint64_t m, uint8_t* d_blobs) {
      return proof_dev_locked(ctx, d_blobs, side_is_commitment ? d_side + base * side_bytes : nullptr, side_is_commitment ? nullptr : d_side + base * side_bytes, m,
                              d_out ? d_out + base * 48 : nullptr, d_aff ? d_aff + base * 96 : nullptr, d_y ? d_y + base * 32 : nullptr, d_status + base, hc.st);
    });
  });
  return hc.close(rc);
}

// the four host-buffer proof calls: `side` is the commitments (48 bytes per item) or the evaluation points (32)
static int32_t proof_on_members(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* side, bool side_is_commitment, uint64_t n, uint8_t* out48,
                                uint8_t* out_affine96, uint8_t* out_y32, int32_t* status) {
  const size_t side_bytes = side_is_commitment ? 48 : 32;
  return on_members(ctx, n, [&](const kzg_ctx* m, uint64_t first, uint64_t count) {
    return proof_host(m, blobs + first * (size_t)KZG_BYTES_PER_BLOB, side + first * side_bytes, side_bytes, side_is_commitment, count,
                      out48 ? out48 + first * 48 : nullptr, out_affine96 ? out_affine96 + first * 96 : nullptr, out_y32 ? out_y32 + first * 32 : nullptr,
                      status + first);
  });
}
extern "C" int32_t kzg_compute_blob_proof_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, uint64_t n,
                                                uint8_t* out48, int32_t* status) try {
  if (!ctx || (n && (!blobs || !commitments48 || !out48 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return proof_on_members(ctx, blobs, commitments48, true, n, out48, nullptr, nullptr, status);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_compute_blob_proof_batch_affine(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, uint64_t n,
                                                       uint8_t* out_affine96, int32_t* status) try {
  if (!ctx || (n && (!blobs || !commitments48 || !out_affine96 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return proof_on_members(ctx, blobs, commitments48, true, n, nullptr, out_affine96, nullptr, status);
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_compute_proof_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* z32, uint64_t n, uint8_t* out_proof48,
                                           uint8_t* out_y32, int32_t* status) try {
  if (!ctx || (n && (!blobs || !z32 || !out_proof48 || !out_y32 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return proof_on_members(ctx, blobs, z32, false, n, out_proof48, nullptr, out_y32, status);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_compute_proof_batch_affine(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* z32, uint64_t n, uint8_t* out_proof_affine96,
                                                  uint8_t* out_y32, int32_t* status) try {
  if (!ctx || (n && (!blobs || !z32 || !out_proof_affine96 || !out_y32 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return proof_on_members(ctx, blobs, z32, false, n, nullptr, out_proof_affine96, out_y32, status);
} catch (...) {
  return abi_exception();
}

// ---------------------------------------------------------------------------
// blob sidecar: commitment, blob proof and versioned hash of every blob in one call
// ---------------------------------------------------------------------------
// Setup::blob_to_commitment, then Setup::blob_proof with that commitment, then kzg_to_versioned_hash, for n blobs resident on the
// device.  Chunks and workspace are proof_layout's (preparation slot 0 only); a chunk's two MSMs have the same shape and follow each
// other on `st`, so they share the lane sums, the sums and the bit-plane masks.  The challenge hashes the commitments the device has
// just written: they are valid by construction, so nothing is decoded and no commitment status is merged.
static int32_t sidecar_dev_locked(const kzg_ctx* ctx, const uint8_t* d_blobs, uint64_t n, uint8_t* d_out_commitments48, uint8_t* d_out_proofs48, uint8_t* d_out_vh32,
                                  int32_t* d_status, hipStream_t st) {
  if (n == 0) return 0;
  const ProofLayout L = proof_layout(ctx, n);
  const uint64_t cn = L.cn;
  int32_t rc = ws_reserve(ctx, L.total, st);
  if (rc) return rc;
  uint8_t* ws = ws_ptr(ctx);
  fr_t* z = reinterpret_cast<fr_t*>(ws + L.o_z[0]);
  fr_t* y = reinterpret_cast<fr_t*>(ws + L.o_y[0]);
  fr_t* invr = reinterpret_cast<fr_t*>(ws + L.o_ir[0]);
  fr_t* q = reinterpret_cast<fr_t*>(ws + L.o_q[0]);
  HIP_TRY(hipMemsetAsync(d_status, 0, n * sizeof(int32_t), st));
  for (uint64_t base = 0; base < n; base += cn) {
    const uint64_t m = (n - base < cn) ? (n - base) : cn;
    const uint8_t* blobs = d_blobs + base * (uint64_t)KZG_BYTES_PER_BLOB;
    uint8_t* com = d_out_commitments48 + base * 48;
    rc = msm_pipeline(ctx, true, blobs, m, com, nullptr, d_status + base, L.msm, ws, st);
    if (rc) return rc;
    launch_challenge(ctx, st, blobs, com, m, z);
    {
      ProfScope ps(ctx, PROF_POLY, st);
      hipLaunchKernelGGL(k_poly_root_inverse, dim3(blocks_for(m, 64)), dim3(64), 0, st, z, m, invr);
      hipLaunchKernelGGL(k_poly<true>, dim3((unsigned)m), dim3(512), 0, st, blobs, z, ctx->d_roots_brp, invr, y, q, d_status + base);
    }
    rc = msm_pipeline(ctx, false, reinterpret_cast<const uint8_t*>(q), m, d_out_proofs48 + base * 48, nullptr, d_status + base, L.msm, ws, st);
    if (rc) return rc;
    if (d_out_vh32) launch_versioned_hash(st, com, m, d_status + base, d_out_vh32 + base * 32);
  }
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "sidecar pipeline launch failed");
  return 0;
}

extern "C" int32_t kzg_blob_sidecar_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out_commitments48, void* d_out_proofs48,
                                              void* d_out_versioned_hashes32, void* d_status, void* hip_stream) try {
  if (!ctx || (n && (!d_blobs || !d_out_commitments48 || !d_out_proofs48 || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  return with_workspace(ctx, st, [&] {
    return sidecar_dev_locked(ctx, (const uint8_t*)d_blobs, n, (uint8_t*)d_out_commitments48, (uint8_t*)d_out_proofs48, (uint8_t*)d_out_versioned_hashes32,
                              (int32_t*)d_status, st);
  });
} catch (...) {
  return abi_exception();
}

// Host-buffer form, after proof_host: the blobs cross PCIe ONCE, in passes through the staging ring, and every pass goes through
// sidecar_dev_locked; the three results and the statuses come back through the host-i/o pool.  A staging slot is free again only
// when the pass's quotient kernel has read the blobs -- commit_host's release behind the bit-plane transposition would be too
// early here -- so consumed(k) follows the pass's whole enqueue.  Passes: proof_host's plan, or KATETH_AMD_SIDECAR_PASS blobs each.
int32_t sidecar_host(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_commitments48, uint8_t* out_proofs48, uint8_t* out_versioned_hashes32,
                     int32_t* status) {
  if (n == 0) return 0;
  HostCall hc(ctx);
  const int a_com = hc.download(out_commitments48, n * 48), a_prf = hc.download(out_proofs48, n * 48), a_vh = hc.download(out_versioned_hashes32, n * 32),
            a_st = hc.download(status, n * sizeof(int32_t));
  int32_t rc = hc.open(ctx->knobs.sidecar_pass ? even_plan(n, ctx->knobs.sidecar_pass) : proof_host_plan(n), KZG_BYTES_PER_BLOB);
  if (rc) return rc;
  uint8_t *d_com = hc.dev(a_com), *d_prf = hc.dev(a_prf), *d_vh = hc.dev(a_vh);
  int32_t* d_status = hc.dev<int32_t>(a_st);
  // one workspace slot for all passes, sized BEFORE anything is in flight for the pass that asks most (a short last pass may take
  // more splits, and so more lane sums, than a full one): growing it between passes would free memory under the pipeline
  rc = with_workspace(ctx, hc.st, [&] {
    size_t need = 0;
    for (uint64_t m : hc.plan) need = std::max(need, proof_layout(ctx, m).total);
    const int32_t e = ws_reserve(ctx, need, hc.st);
    if (e) return e;
    return hc.passes(blobs, KZG_BYTES_PER_BLOB, [&](size_t, uint64_t base, uint64_t m, uint8_t* d_blobs) {
      return sidecar_dev_locked(ctx, d_blobs, m, d_com + base * 48, d_prf + base * 48, d_vh ? d_vh + base * 32 : nullptr, d_status + base, hc.st);
    });
  });
  return hc.close(rc);
}

extern "C" int32_t kzg_blob_sidecar_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_commitments48, uint8_t* out_proofs48,
                                          uint8_t* out_versioned_hashes32, int32_t* status) try {
  if (!ctx || (n && (!blobs || !out_commitments48 || !out_proofs48 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return on_members(ctx, n, [&](const kzg_ctx* m, uint64_t first, uint64_t count) {
    return sidecar_host(m, blobs + first * (size_t)KZG_BYTES_PER_BLOB, count, out_commitments48 + first * 48, out_proofs48 + first * 48,
                        out_versioned_hashes32 ? out_versioned_hashes32 + first * 32 : nullptr, status + first);
  });
} catch (...) {
  return abi_exception();
}

// ---------------------------------------------------------------------------
// the cell calls (EIP-7594): compute_cells, recover_cells, and either with the 128 cell proofs of every item
// ---------------------------------------------------------------------------
// The cells of n device-resident items: compute_cells' kernel over blobs, or recover_cells' over cell sets and masks.  One launch, one workgroup
// per CU looping over the items (a workgroup holds its item in all of the CU's LDS it may claim, so a larger grid would only queue).  Either
// kernel writes every output byte and every status: nothing is cleared first.
static int32_t cells_enqueue(const kzg_ctx* ctx, const uint8_t* d_blobs, uint64_t n, uint8_t* d_out_cells, int32_t* d_status, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<uint64_t>(n, ctx->num_cus);
  hipLaunchKernelGGL(k_compute_cells, dim3(grid), dim3(CELLS_THREADS), 0, st, d_blobs, n, ctx->d_cells_tab, d_out_cells, d_status);
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "compute_cells launch failed");
  return 0;
}
// the extension half alone into a verify session's workspace (engine_internal.hpp: the verify driver's way to the kernel)
int32_t cells_ext_enqueue(const kzg_ctx* ctx, const uint8_t* d_blobs, uint64_t n, uint8_t* d_out_ext, int32_t* d_status, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<uint64_t>(n, ctx->num_cus);
  hipLaunchKernelGGL(k_compute_cells_ext, dim3(grid), dim3(CELLS_THREADS), 0, st, d_blobs, n, ctx->d_cells_tab, d_out_ext, d_status);
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "blob extension launch failed");
  return 0;
}
static int32_t recover_enqueue(const kzg_ctx* ctx, const uint8_t* d_cells, const uint8_t* d_present, uint64_t n, uint8_t* d_out_cells, int32_t* d_status,
                               hipStream_t st) {
  const unsigned grid = (unsigned)std::min<uint64_t>(n, ctx->num_cus);
  hipLaunchKernelGGL(k_recover_cells, dim3(grid), dim3(CELLS_THREADS), 0, st, d_cells, d_present, n, ctx->d_cells_tab, ctx->d_recover_tab, d_out_cells,
                     d_status);
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "recover_cells launch failed");
  return 0;
}
static int32_t cells_of(const kzg_ctx* ctx, const CellCall& d, uint64_t n, hipStream_t st) {
  return d.present ? recover_enqueue(ctx, d.in, d.present, n, d.out_cells, d.status, st) : cells_enqueue(ctx, d.in, n, d.out_cells, d.status, st);
}

// Cell proofs -- by quotient MSMs, not FK20.  The proof of cell k is the commitment of q_k = p / (X^64 - z_k) (cellproof_math.cuh): 128 scalar
// vectors per blob, which the fixed-base MSM commits as it commits blobs.  The omega_128 table the division reads is built by the context's
// FIRST cell-proof call, as the monomial points are (ensure_g1_monomial): a context that never asks for cell proofs launches and holds nothing
// for them.
static int32_t ensure_cellproof_tab(const kzg_ctx* ctx) {
  if (ctx->cellproof_ready.load(std::memory_order_acquire)) return 0;
  std::lock_guard<std::mutex> guard(ctx->cellproof_mu);
  if (ctx->cellproof_ready.load(std::memory_order_relaxed)) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  uint32_t* tab = nullptr;
  HIP_TRY(hipMalloc(&tab, (size_t)CELLPROOF_TAB_ENTRIES * CELLS_TAB_ENTRY * sizeof(uint32_t)));
  hipStream_t st = nullptr;
  hipLaunchKernelGGL(k_setup_cellproof_tab, dim3(CELLPROOF_TAB_ENTRIES / 64), dim3(64), 0, st, tab);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // once per context: every later call, on whichever stream, finds the table written
  if (e != hipSuccess) {
    (void)hipFree(tab);
    return fail(KZG_FAIL_HIP, std::string("cell-proof table: ") + hipGetErrorString(e));
  }
  ctx->d_cellproof_tab = tab;
  ctx->cellproof_ready.store(true, std::memory_order_release);
  return 0;
}

// Blobs per pass: 32 by default -- 4,096 vectors, the MSM's best shape, in 512 MiB, the size of the blob-proof path's own quotient slot;
// at most 128 (16,384 vectors: the chunk bound of the commitment path's lane sums).  KATETH_AMD_CELLPROOF_PASS overrides.
static uint64_t cellproof_pass(const kzg_ctx* ctx) { return std::min<uint64_t>(ctx->knobs.cellproof_pass ? ctx->knobs.cellproof_pass : 32, 128); }
// workspace of a pass of m blobs: their coefficients, the 128 m vector statuses and quotient vectors, and one set of MSM buffers
struct CellProofLayout {
  size_t o_coeff = 0, o_vst = 0, o_q = 0, total = 0;
  MsmBufs msm;
};
static CellProofLayout cellproof_layout(const kzg_ctx* ctx, uint64_t m) {
  CellProofLayout L;
  const uint64_t vectors = m * KZG_CELLS_PER_EXT_BLOB;
  Carve ws;
  L.o_coeff = ws.take(m * (size_t)CELLPROOF_COEFF_BYTES);
  L.o_vst = ws.take(vectors * sizeof(int32_t));
  L.o_q = ws.take(vectors * 4096 * sizeof(fr_t));
  L.msm = msm_carve(ctx, ws, vectors);
  L.total = ws.off;
  return L;
}
// what a call over n items reserves before anything is in flight: a ragged last pass may take more splits than a full one
static size_t cellproof_ws_bytes(const kzg_ctx* ctx, uint64_t n) {
  const uint64_t P = cellproof_pass(ctx), full = std::min(n, P), rest = n > P ? n % P : 0;
  return std::max(cellproof_layout(ctx, full).total, rest ? cellproof_layout(ctx, rest).total : (size_t)0);
}

// The 128 proofs of each of n items resident on the device, 48 bytes each at d_out_proofs48 + 6,144 item.  Item i is the 131,072 bytes
// at d_items + i * stride: a blob (stride 131,072; skip_rejected = false: the item is range-checked and d_status[i] written) or cells
// 0..63 of a recovered cell set (stride 262,144; skip_rejected = true: d_status[i] is k_recover_cells' verdict).  A rejected item gets
// 6,144 zero bytes.  One stream, pass after pass; the two new kernels are timed with the blob-proof path's quotient kernel (PROF_POLY).
static int32_t cellproof_dev_locked(const kzg_ctx* ctx, const uint8_t* d_items, uint64_t stride, bool skip_rejected, uint64_t n, uint8_t* d_out_proofs48,
                                    int32_t* d_status, hipStream_t st) {
  if (n == 0) return 0;
  int32_t rc = ws_reserve(ctx, cellproof_ws_bytes(ctx, n), st);
  if (rc) return rc;
  uint8_t* ws = ws_ptr(ctx);
  const uint64_t P = cellproof_pass(ctx);
  for (uint64_t base = 0; base < n; base += P) {
    const uint64_t m = std::min(n - base, P), vectors = m * KZG_CELLS_PER_EXT_BLOB;
    const CellProofLayout L = cellproof_layout(ctx, m);
    ctx->cellproof_vectors.fetch_add(vectors, std::memory_order_relaxed);
    uint32_t* coeffs = reinterpret_cast<uint32_t*>(ws + L.o_coeff);
    int32_t* vstatus = reinterpret_cast<int32_t*>(ws + L.o_vst);
    uint32_t* q = reinterpret_cast<uint32_t*>(ws + L.o_q);
    {
      ProfScope ps(ctx, PROF_POLY, st);
      hipLaunchKernelGGL(k_cell_coeffs, dim3((unsigned)std::min<uint64_t>(m, ctx->num_cus)), dim3(CELLS_THREADS), 0, st, d_items + base * stride, stride, m,
                         skip_rejected, ctx->d_cells_tab, coeffs, d_status + base, vstatus);
      hipLaunchKernelGGL(k_cell_quotients, dim3((unsigned)vectors), dim3(CELLS_THREADS), 0, st, coeffs, ctx->d_cells_tab, ctx->d_cellproof_tab, vstatus, q);
    }
    rc = msm_pipeline(ctx, false, reinterpret_cast<const uint8_t*>(q), vectors, d_out_proofs48 + base * (KZG_CELLS_PER_EXT_BLOB * 48), nullptr, vstatus, L.msm, ws,
                      st);
    if (rc) return rc;
  }
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "cell-proof pipeline launch failed");
  return 0;
}

// What the two sources of a cell call differ in.  With proofs, either takes passes of cellproof_pass items instead of `cells_pass`, and
// a staging slot holds a pass's input and, where cells are wanted, its cell sets behind it.
struct CellSource {
  // bytes per item up to the device
  size_t up_bytes;
  // items per pass of a call without proofs (KATETH_AMD_CELLS_PASS overrides)
  uint64_t cells_pass;
  // true: only cells 64..127 come down and, once the statuses are on the host, cells_first_halves fills cells 0..63;
  // false: the whole cell set comes down
  bool ext_half_down;
  // what the proof kernels read.  false: the input, a blob they range-check themselves (stride up_bytes, skip_rejected = false);
  // true: cells 0..63 of the item's own output, under the cells kernel's verdict (stride 262,144, skip_rejected = true)
  bool proofs_of_own_cells;
};
// compute: PCIe is the limit (128 KiB up and 256 KiB down per blob), so only the extension half comes back: cells 0..63 of an
// accepted blob ARE the caller's blob and are copied on the host.  recover: whole cell sets both ways, 256 KiB each per item.
constexpr CellSource CELLS_OF_BLOBS{KZG_BYTES_PER_BLOB, 512, true, false};
constexpr CellSource CELLS_OF_CELL_SETS{KZG_BYTES_PER_CELL_SET, 256, false, true};
static const CellSource& cell_source(const CellCall& c) { return c.present ? CELLS_OF_CELL_SETS : CELLS_OF_BLOBS; }
// the proofs of n device-resident items whose cells kernel has been enqueued; the caller holds a workspace (with_workspace)
static int32_t cellproofs_locked(const kzg_ctx* ctx, const CellCall& d, uint64_t n, hipStream_t st) {
  const CellSource& src = cell_source(d);
  return cellproof_dev_locked(ctx, src.proofs_of_own_cells ? d.out_cells : d.in, src.proofs_of_own_cells ? KZG_BYTES_PER_CELL_SET : src.up_bytes,
                              src.proofs_of_own_cells, n, d.out_proofs48, d.status, st);
}

// ---- the select calls: the proofs of chosen (item, cell) pairs only ----
// The host turns the `want` masks (host memory in every form) into the pass plan and the pair list (cellproof_plan.hpp).  A pass packs
// consecutive items while its wanted vectors stay <= 128 cellproof_pass, so a pass's MSM is never larger than a full call's, and with
// all-ones masks the passes ARE the full call's.  Workspace of a call: the pair lists of all its passes (a *_dev call; the host-buffer call
// keeps them in the host-i/o pool), then, for a pass of m items and V vectors, the m coefficient sets and 128 m vector statuses as in
// cellproof_layout, the V compact statuses, V x 128 KiB of vectors, 48 V bytes of compact proofs and the MSM's buffers for V vectors.
using cellplan::Pass;
struct CellSelLayout {
  size_t o_pairs = 0, o_coeff = 0, o_vst = 0, o_cst = 0, o_q = 0, o_prf = 0, total = 0;
  MsmBufs msm;
};
static CellSelLayout cellsel_layout(const kzg_ctx* ctx, uint64_t call_pairs, const Pass& p) {
  CellSelLayout L;
  Carve ws;
  L.o_pairs = ws.take(call_pairs * sizeof(uint32_t));
  L.o_coeff = ws.take(p.items * (size_t)CELLPROOF_COEFF_BYTES);
  L.o_vst = ws.take(p.items * KZG_CELLS_PER_EXT_BLOB * sizeof(int32_t));
  L.o_cst = ws.take(p.vectors * sizeof(int32_t));
  L.o_q = ws.take(p.vectors * 4096 * sizeof(fr_t));
  L.o_prf = ws.take(p.vectors * 48);
  if (p.vectors) L.msm = msm_carve(ctx, ws, p.vectors);
  L.total = ws.off;
  return L;
}
static size_t cellsel_ws_bytes(const kzg_ctx* ctx, uint64_t call_pairs, const std::vector<Pass>& plan) {
  size_t need = 0;
  for (const Pass& p : plan) need = std::max(need, cellsel_layout(ctx, call_pairs, p).total);
  return need;
}
// One pass: p.items items from d_items on (stride, skip_rejected: cellproof_dev_locked's), their p.vectors pairs at d_pairs on the device.
// The compact proofs go to d_compact (null: the workspace's own buffer) and, with d_scatter_to -- the caller's proof buffer at the pass's
// first item --, from there to their places.  A pass nobody wants a proof of launches k_cell_coeffs alone, and only where no earlier kernel
// has written the statuses (status_written).
// `col` (the data column calls): d_scatter_to is a column matrix of proofs of col->rows rows and the pass's first item its row col->row0;
// with skip_rejected, d_items is the column matrix of cells the items are rows of, in the same way, and `stride` is not used.
struct ColumnRows {
  uint64_t rows, row0;
};
static int32_t cellsel_pass(const kzg_ctx* ctx, const uint8_t* d_items, uint64_t stride, bool skip_rejected, bool status_written, const Pass& p,
                            const uint32_t* d_pairs, uint8_t* d_compact, uint8_t* d_scatter_to, int32_t* d_status, const CellSelLayout& L, uint8_t* ws,
                            hipStream_t st, const ColumnRows* col = nullptr) {
  const uint64_t m = p.items, V = p.vectors;
  if (V == 0 && status_written) return 0;
  uint32_t* coeffs = reinterpret_cast<uint32_t*>(ws + L.o_coeff);
  int32_t* vstatus = reinterpret_cast<int32_t*>(ws + L.o_vst);
  int32_t* cstat = reinterpret_cast<int32_t*>(ws + L.o_cst);
  uint32_t* q = reinterpret_cast<uint32_t*>(ws + L.o_q);
  if (!d_compact) d_compact = ws + L.o_prf;
  ctx->cellproof_vectors.fetch_add(V, std::memory_order_relaxed);
  {
    ProfScope ps(ctx, PROF_POLY, st);
    if (col && skip_rejected)
      hipLaunchKernelGGL(k_columns_coeffs, dim3((unsigned)std::min<uint64_t>(m, ctx->num_cus)), dim3(CELLS_THREADS), 0, st, d_items, col->rows, col->row0, m,
                         ctx->d_cells_tab, coeffs, d_status, vstatus);
    else
      hipLaunchKernelGGL(k_cell_coeffs, dim3((unsigned)std::min<uint64_t>(m, ctx->num_cus)), dim3(CELLS_THREADS), 0, st, d_items, stride, m, skip_rejected,
                         ctx->d_cells_tab, coeffs, d_status, vstatus);
    if (V)
      hipLaunchKernelGGL(k_cell_quotients_sel, dim3((unsigned)V), dim3(CELLS_THREADS), 0, st, coeffs, ctx->d_cells_tab, ctx->d_cellproof_tab, vstatus, d_pairs,
                         cstat, q);
  }
  if (V == 0) return 0;
  const int32_t rc = msm_pipeline(ctx, false, reinterpret_cast<const uint8_t*>(q), V, d_compact, nullptr, cstat, L.msm, ws, st);
  if (rc) return rc;
  if (d_scatter_to && col)
    hipLaunchKernelGGL(k_columns_scatter, dim3(blocks_for(V, 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(d_compact), d_pairs, (uint32_t)V,
                       d_scatter_to, col->rows, col->row0);
  else if (d_scatter_to)
    hipLaunchKernelGGL(k_cellproof_scatter, dim3(blocks_for(V, 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(d_compact), d_pairs, (uint32_t)V,
                       reinterpret_cast<uint4*>(d_scatter_to));
  return 0;
}
// A pinned host buffer of at least `bytes` for the pair list of the *_dev call being enqueued (the caller holds ctx->lock): one whose
// last upload has completed, else a new one while fewer than eight exist, else the first, once its upload has run -- only a ninth call
// behind eight unfinished ones waits.  The caller records pin->ev behind its copy.
static int32_t pair_pin_take(const kzg_ctx* ctx, size_t bytes, kzg_ctx::PairPin** out) {
  constexpr size_t MAX_PINS = 8;
  std::vector<kzg_ctx::PairPin>& pins = ctx->pair_pins;
  kzg_ctx::PairPin* pick = nullptr;
  for (size_t k = 0; k < pins.size() && !pick; k++) {
    if (hipEventQuery(pins[k].ev) == hipSuccess) pick = &pins[k];
    else (void)hipGetLastError();  // hipErrorNotReady is not an error of this call
  }
  if (!pick && pins.size() < MAX_PINS) {
    kzg_ctx::PairPin fresh;
    HIP_TRY(hipEventCreateWithFlags(&fresh.ev, hipEventDisableTiming));
    pins.push_back(fresh);
    pick = &pins.back();
  }
  if (!pick) {
    pick = &pins[0];
    HIP_TRY(hipEventSynchronize(pick->ev));
  }
  if (pick->bytes < bytes) {
    if (pick->p) (void)hipHostFree(pick->p);
    pick->p = nullptr;
    pick->bytes = 0;
    const size_t room = std::max<size_t>(bytes + bytes / 4, 65536);
    if (hipHostMalloc(&pick->p, room, hipHostMallocDefault) != hipSuccess) return fail(KZG_FAIL_HIP, "hipHostMalloc(pair list) failed");
    pick->bytes = room;
  }
  *out = pick;
  return 0;
}
// the select proofs of n device-resident items whose cells kernel has been enqueued; the caller holds a workspace (with_workspace).  `d.want` is
// read here, before the call returns: the pair list goes up from a pinned buffer of the context's.
static int32_t cellsel_dev_locked(const kzg_ctx* ctx, const CellCall& d, uint64_t n, hipStream_t st) {
  const CellSource& src = cell_source(d);
  const uint8_t* d_items = src.proofs_of_own_cells ? d.out_cells : d.in;
  const uint64_t stride = src.proofs_of_own_cells ? KZG_BYTES_PER_CELL_SET : src.up_bytes;
  const bool status_written = src.proofs_of_own_cells || d.out_cells != nullptr;
  const std::vector<Pass> plan = cellplan::plan(d.want, n, cellproof_pass(ctx));
  const uint64_t call_pairs = cellplan::total_vectors(plan);
  int32_t rc = ws_reserve(ctx, cellsel_ws_bytes(ctx, call_pairs, plan), st);
  if (rc) return rc;
  uint8_t* ws = ws_ptr(ctx);
  const uint32_t* d_pairs = reinterpret_cast<const uint32_t*>(ws);  // o_pairs == 0 in every pass's layout
  if (call_pairs) {
    kzg_ctx::PairPin* pin = nullptr;
    rc = pair_pin_take(ctx, call_pairs * sizeof(uint32_t), &pin);
    if (rc) return rc;
    cellplan::write_all_pairs(d.want, plan, static_cast<uint32_t*>(pin->p));
    HIP_TRY(hipMemcpyAsync(ws, pin->p, call_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(pin->ev, st));
  }
  uint64_t base = 0, voff = 0;
  for (const Pass& p : plan) {
    rc = cellsel_pass(ctx, d_items + base * stride, stride, src.proofs_of_own_cells, status_written, p, d_pairs + voff, nullptr,
                      d.out_proofs48 + base * (KZG_CELLS_PER_EXT_BLOB * 48), d.status + base, cellsel_layout(ctx, call_pairs, p), ws, st);
    if (rc) return rc;
    base += p.items;
    voff += p.vectors;
  }
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "cell-proof pipeline launch failed");
  return 0;
}

// The device-resident cell call: the cells by their kernel, launched first and outside the lock, then the proofs under a workspace slot.
int32_t das_dev(const kzg_ctx* ctx, const CellCall& d, uint64_t n, hipStream_t st) {
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  int32_t rc = d.out_proofs48 ? ensure_cellproof_tab(ctx) : 0;
  if (rc == 0 && d.out_cells) rc = cells_of(ctx, d, n, st);
  if (rc == 0 && d.out_proofs48) rc = with_workspace(ctx, st, [&] { return d.want ? cellsel_dev_locked(ctx, d, n, st) : cellproofs_locked(ctx, d, n, st); });
  return rc;
}

// cells 0..63 of every item of a compute call: the caller's blob, or zero bytes
static void cells_first_halves(const uint8_t* blobs, uint64_t n, const int32_t* status, uint8_t* out_cells) {
  for (uint64_t i = 0; i < n; i++) {
    if (status[i] == 0)
      memcpy(out_cells + i * KZG_BYTES_PER_CELL_SET, blobs + i * (size_t)KZG_BYTES_PER_BLOB, KZG_BYTES_PER_BLOB);
    else
      memset(out_cells + i * KZG_BYTES_PER_CELL_SET, 0, KZG_BYTES_PER_BLOB);
  }
}
// A select call's compact proofs to their places in the caller's buffer, with the pair lists the device walked and the statuses now on the
// host: the wanted positions of a rejected item get zero bytes, and no other position is written.
static void cellsel_scatter_host(const std::vector<Pass>& plan, const uint32_t* pairs, const uint8_t* compact, const int32_t* status, uint8_t* out_proofs48) {
  uint64_t base = 0, s = 0;
  for (const Pass& p : plan) {
    for (uint64_t v = 0; v < p.vectors; v++, s++) {
      const uint64_t item = base + cellproof_pair_item(pairs[s]);
      uint8_t* dst = out_proofs48 + 48 * (KZG_CELLS_PER_EXT_BLOB * item + cellproof_pair_cell(pairs[s]));
      if (status[item] == 0)
        memcpy(dst, compact + 48 * s, 48);
      else
        memset(dst, 0, 48);
    }
    base += p.items;
  }
}
// The host-buffer cell call.  The input crosses PCIe in passes through the staging ring.  The masks of the whole call go up once, and
// the proofs (6 KiB per item) and the statuses come down once, through the host-i/o pool.  A pass's cells come down behind its kernel,
// and its slot is free again behind all the pass enqueued.  With proofs a staging pass is a pass of the device path (about 28 ms of
// MSM each at the default of 32, so a pass's copy hides behind its predecessor), and one workspace slot serves all passes, sized
// before anything is in flight.  A select call (c.want) walks cellplan's passes instead, sends its pair lists up with the masks and
// brings only its 48 V selected proofs down, compact: the host puts them in their places once the statuses are there.
int32_t das_host(const kzg_ctx* ctx, const CellCall& c, uint64_t n) {
  if (n == 0) return 0;
  const CellSource& src = cell_source(c);
  const bool proofs = c.out_proofs48 != nullptr, sel = proofs && c.want != nullptr;
  int32_t rc = proofs ? ensure_cellproof_tab(ctx) : 0;
  if (rc) return rc;
  // a select call: its plan and pair lists, and the compact proofs as they come down; all three live until close() has synchronised
  std::vector<Pass> sel_plan;
  std::vector<uint32_t> pairs;
  std::vector<uint8_t> compact;
  std::vector<uint64_t> items_plan;
  if (sel) {
    sel_plan = cellplan::plan(c.want, n, cellproof_pass(ctx));
    pairs.resize(cellplan::total_vectors(sel_plan));
    cellplan::write_all_pairs(c.want, sel_plan, pairs.data());
    compact.resize(pairs.size() * 48);
    for (const Pass& p : sel_plan) items_plan.push_back(p.items);
  }
  HostCall hc(ctx);
  // the full-size proof download would overwrite the positions a select call must leave alone: its 48 V selected proofs come down instead
  const int a_mask = hc.upload(c.present, n * 16), a_prf = sel ? -1 : hc.download(c.out_proofs48, n * (KZG_CELLS_PER_EXT_BLOB * 48)),
            a_st = hc.download(c.status, n * sizeof(int32_t)), a_pairs = hc.upload(pairs.empty() ? nullptr : pairs.data(), pairs.size() * sizeof(uint32_t)),
            a_cmp = hc.download(compact.empty() ? nullptr : compact.data(), compact.size());
  const uint64_t pass = proofs ? cellproof_pass(ctx) : ctx->knobs.cells_pass ? ctx->knobs.cells_pass : src.cells_pass;
  rc = hc.open(sel ? items_plan : even_plan(n, pass), src.up_bytes + (c.out_cells ? KZG_BYTES_PER_CELL_SET : 0));
  if (rc) return rc;
  const uint8_t* d_present = hc.dev(a_mask);  // resolved after open(): opening may move the pools
  uint8_t *d_prf = hc.dev(a_prf), *d_cmp = hc.dev(a_cmp);
  const uint32_t* d_pairs = hc.dev<uint32_t>(a_pairs);
  int32_t* d_status = hc.dev<int32_t>(a_st);
  uint64_t voff = 0;  // vectors of the select passes enqueued so far
  auto enqueue = [&] {
    return hc.passes(c.in, src.up_bytes, [&](size_t k, uint64_t base, uint64_t m, uint8_t* d_in) {
      const CellCall d{d_in, d_present ? d_present + base * 16 : nullptr, c.out_cells ? d_in + hc.max_pass * src.up_bytes : nullptr,
                       d_prf ? d_prf + base * (KZG_CELLS_PER_EXT_BLOB * 48) : nullptr, d_status + base};
      if (d.out_cells) {
        const int32_t e = cells_of(ctx, d, m, hc.st);
        if (e) return e;
        uint8_t* out = c.out_cells + base * KZG_BYTES_PER_CELL_SET;
        const hipError_t down = src.ext_half_down ? hipMemcpy2DAsync(out + KZG_BYTES_PER_BLOB, KZG_BYTES_PER_CELL_SET, d.out_cells + KZG_BYTES_PER_BLOB,
                                                                     KZG_BYTES_PER_CELL_SET, KZG_BYTES_PER_BLOB, m, hipMemcpyDeviceToHost, hc.st)
                                                  : hipMemcpyAsync(out, d.out_cells, m * KZG_BYTES_PER_CELL_SET, hipMemcpyDeviceToHost, hc.st);
        if (down != hipSuccess) return fail(KZG_FAIL_HIP, "device-to-host copy failed");
      }
      if (sel) {
        const Pass& p = sel_plan[k];
        const int32_t e = cellsel_pass(ctx, src.proofs_of_own_cells ? d.out_cells : d.in, src.proofs_of_own_cells ? KZG_BYTES_PER_CELL_SET : src.up_bytes,
                                       src.proofs_of_own_cells, src.proofs_of_own_cells || d.out_cells != nullptr, p, d_pairs + voff, d_cmp + voff * 48, nullptr,
                                       d.status, cellsel_layout(ctx, 0, p), ws_ptr(ctx), hc.st);
        voff += p.vectors;
        return e;
      }
      return proofs ? cellproofs_locked(ctx, d, m, hc.st) : 0;
    });
  };
  if (proofs)
    rc = with_workspace(ctx, hc.st, [&] {
      const int32_t e = ws_reserve(ctx, sel ? cellsel_ws_bytes(ctx, 0, sel_plan) : cellproof_ws_bytes(ctx, n), hc.st);
      return e ? e : enqueue();
    });
  else
    rc = enqueue();
  if (rc == 0 && sel && hipGetLastError() != hipSuccess) rc = fail(KZG_FAIL_HIP, "cell-proof pipeline launch failed");
  rc = hc.close(rc);
  if (rc == 0 && src.ext_half_down && c.out_cells) cells_first_halves(c.in, n, c.status, c.out_cells);
  if (rc == 0 && sel) cellsel_scatter_host(sel_plan, pairs.data(), compact.data(), c.status, c.out_proofs48);
  return rc;
}

// The eight entry points: each states which of its arguments may be null (out_cells, and only where proofs are computed from blobs)
static int32_t das_on_members(const kzg_ctx* ctx, const CellCall& call, uint64_t n) {
  return on_members(ctx, n, [&](const kzg_ctx* m, uint64_t first, uint64_t count) { return das_host(m, call.advanced(first), count); });
}
static CellCall cell_call(const void* in, const void* present, void* out_cells, void* out_proofs48, void* status) {
  return CellCall{(const uint8_t*)in, (const uint8_t*)present, (uint8_t*)out_cells, (uint8_t*)out_proofs48, (int32_t*)status};
}
extern "C" int32_t kzg_compute_cells_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out_cells, void* d_status, void* hip_stream) try {
  if (!ctx || (n && (!d_blobs || !d_out_cells || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_dev(ctx, cell_call(d_blobs, nullptr, d_out_cells, nullptr, d_status), n, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_compute_cells_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_cells, int32_t* status) try {
  if (!ctx || (n && (!blobs || !out_cells || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_on_members(ctx, cell_call(blobs, nullptr, out_cells, nullptr, status), n);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_recover_cells_batch_dev(const kzg_ctx* ctx, const void* d_cells, const void* d_present, uint64_t n, void* d_out_cells, void* d_status,
                                               void* hip_stream) try {
  if (!ctx || (n && (!d_cells || !d_present || !d_out_cells || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_dev(ctx, cell_call(d_cells, d_present, d_out_cells, nullptr, d_status), n, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_recover_cells_batch(const kzg_ctx* ctx, const uint8_t* cells, const uint8_t* present, uint64_t n, uint8_t* out_cells, int32_t* status) try {
  if (!ctx || (n && (!cells || !present || !out_cells || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_on_members(ctx, cell_call(cells, present, out_cells, nullptr, status), n);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_compute_cells_and_proofs_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out_cells, void* d_out_proofs48, void* d_status,
                                                          void* hip_stream) try {
  if (!ctx || (n && (!d_blobs || !d_out_proofs48 || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_dev(ctx, cell_call(d_blobs, nullptr, d_out_cells, d_out_proofs48, d_status), n, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_compute_cells_and_proofs_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_cells, uint8_t* out_proofs48,
                                                      int32_t* status) try {
  if (!ctx || (n && (!blobs || !out_proofs48 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_on_members(ctx, cell_call(blobs, nullptr, out_cells, out_proofs48, status), n);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_recover_cells_and_proofs_batch_dev(const kzg_ctx* ctx, const void* d_cells, const void* d_present, uint64_t n, void* d_out_cells,
                                                          void* d_out_proofs48, void* d_status, void* hip_stream) try {
  if (!ctx || (n && (!d_cells || !d_present || !d_out_cells || !d_out_proofs48 || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_dev(ctx, cell_call(d_cells, d_present, d_out_cells, d_out_proofs48, d_status), n, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_recover_cells_and_proofs_batch(const kzg_ctx* ctx, const uint8_t* cells, const uint8_t* present, uint64_t n, uint8_t* out_cells,
                                                      uint8_t* out_proofs48, int32_t* status) try {
  if (!ctx || (n && (!cells || !present || !out_cells || !out_proofs48 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_on_members(ctx, cell_call(cells, present, out_cells, out_proofs48, status), n);
} catch (...) {
  return abi_exception();
}

// The select forms: `want` is host memory in all four, and a null `want` is an argument error, not the full call
static CellCall cell_call_select(const void* in, const void* present, const uint8_t* want, void* out_cells, void* inout_proofs48, void* status) {
  CellCall c = cell_call(in, present, out_cells, inout_proofs48, status);
  c.want = want;
  return c;
}
extern "C" int32_t kzg_compute_cells_and_proofs_select_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* want, uint64_t n, uint8_t* out_cells,
                                                             uint8_t* inout_proofs48, int32_t* status) try {
  if (!ctx || (n && (!blobs || !want || !inout_proofs48 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_on_members(ctx, cell_call_select(blobs, nullptr, want, out_cells, inout_proofs48, status), n);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_compute_cells_and_proofs_select_batch_dev(const kzg_ctx* ctx, const void* d_blobs, const uint8_t* want, uint64_t n, void* d_out_cells,
                                                                 void* d_inout_proofs48, void* d_status, void* hip_stream) try {
  if (!ctx || (n && (!d_blobs || !want || !d_inout_proofs48 || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_dev(ctx, cell_call_select(d_blobs, nullptr, want, d_out_cells, d_inout_proofs48, d_status), n, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_recover_cells_and_proofs_select_batch(const kzg_ctx* ctx, const uint8_t* cells, const uint8_t* present, const uint8_t* want, uint64_t n,
                                                             uint8_t* out_cells, uint8_t* inout_proofs48, int32_t* status) try {
  if (!ctx || (n && (!cells || !present || !want || !out_cells || !inout_proofs48 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_on_members(ctx, cell_call_select(cells, present, want, out_cells, inout_proofs48, status), n);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_recover_cells_and_proofs_select_batch_dev(const kzg_ctx* ctx, const void* d_cells, const void* d_present, const uint8_t* want, uint64_t n,
                                                                 void* d_out_cells, void* d_inout_proofs48, void* d_status, void* hip_stream) try {
  if (!ctx || (n && (!d_cells || !d_present || !want || !d_out_cells || !d_inout_proofs48 || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return das_dev(ctx, cell_call_select(d_cells, d_present, want, d_out_cells, d_inout_proofs48, d_status), n, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
// ---------------------------------------------------------------------------
// the data column calls: the producer's and the reconstructing node's cell calls, cells and proofs as COLUMN MATRICES
// ---------------------------------------------------------------------------
// A column matrix of a call over n rows (the block's blobs, in order) puts the cell of column c, row b at 2048 (c n + b) and its proof at
// 48 (c n + b): column c's sidecar payload is one run of bytes.  The kernels do the addressing (cells_column_major, cells_math.cuh; the
// k_columns_* siblings), a pass of m rows writes rows [base, base + m) of every column, and everything else -- pass plan, pair lists,
// workspace, MSM -- is the select calls': the ONE `want` mask of a call, repeated for its rows, goes through cellplan like n masks would,
// and the producer is the all-ones plan, whose passes are the full call's.
//   in        produce: the n blobs, blob-major.  recover (`present`): the column matrix of cells
//   present   HOST memory in either form: the call's one 16-byte mask, a kernel argument of k_columns_recover
//   want      HOST memory: the one mask of the proofs to compute; null: all of them (produce), or none (recover: out_proofs48 is null too)
struct ColumnCall {
  const uint8_t *in, *present, *want;
  uint8_t *out_commitments48, *out_cells, *out_proofs48;
  int32_t* status;
};
static std::vector<uint8_t> column_want_masks(const ColumnCall& c, uint64_t n) {
  std::vector<uint8_t> want(n * cellplan::MASK_BYTES, 0xff);
  for (uint64_t i = 0; c.want && i < n; i++) memcpy(want.data() + i * cellplan::MASK_BYTES, c.want, cellplan::MASK_BYTES);
  return want;
}
// the cells of n rows, row0 on, of column matrices of `rows` rows: either kernel writes every byte of its rows and every status
static int32_t columns_cells_enqueue(const kzg_ctx* ctx, const ColumnCall& c, const uint8_t* d_in, uint64_t n, uint8_t* d_out_cells, uint64_t rows, uint64_t row0,
                                     int32_t* d_status, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<uint64_t>(n, ctx->num_cus);
  if (c.present) {
    uint4 mask;
    memcpy(&mask, c.present, sizeof mask);
    hipLaunchKernelGGL(k_columns_recover, dim3(grid), dim3(CELLS_THREADS), 0, st, d_in, mask, n, ctx->d_cells_tab, ctx->d_recover_tab, d_out_cells, rows, row0,
                       d_status);
  } else {
    hipLaunchKernelGGL(k_columns_compute, dim3(grid), dim3(CELLS_THREADS), 0, st, d_in, n, ctx->d_cells_tab, d_out_cells, rows, row0, d_status);
  }
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "data column cells launch failed");
  return 0;
}
// The commitments of n resident blobs by the commitment path (the blobs' bytes as the MSM's scalars, chunks of 16,384 as
// kzg_blob_to_commitment_batch_dev takes them), in the workspace from ws_off on.  The statuses hold the cells kernel's verdicts already: the
// MSM's own range check finds the same blobs, and a rejected blob's commitment is 48 zero bytes.
constexpr uint64_t COLUMNS_COMMIT_CHUNK = 16384;
static size_t columns_commit_ws(const kzg_ctx* ctx, uint64_t n, size_t ws_off) {
  Carve carve;
  carve.off = ws_off;
  (void)msm_carve(ctx, carve, std::min(n, COLUMNS_COMMIT_CHUNK));
  return carve.off;
}
static int32_t columns_commit(const kzg_ctx* ctx, const uint8_t* d_blobs, uint64_t n, uint8_t* d_out48, int32_t* d_status, size_t ws_off, hipStream_t st) {
  const uint64_t cn = std::min(n, COLUMNS_COMMIT_CHUNK);
  Carve carve;
  carve.off = ws_off;
  const MsmBufs bufs = msm_carve(ctx, carve, cn);
  for (uint64_t base = 0; base < n; base += cn) {
    const int32_t rc =
        msm_pipeline(ctx, true, d_blobs + base * (uint64_t)KZG_BYTES_PER_BLOB, std::min(n - base, cn), d_out48 + base * 48, nullptr, d_status + base, bufs, ws_ptr(ctx), st);
    if (rc) return rc;
  }
  return 0;
}

// The device-resident call: the cells by their kernel, launched first and outside the lock (das_dev's order); commitments and proofs
// under one workspace slot, which a call that wants neither does not take.  Both masks are read here, before the call returns.
static int32_t columns_dev(const kzg_ctx* ctx, const ColumnCall& c, uint64_t n, hipStream_t st) {
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  const bool recover = c.present != nullptr;
  int32_t rc = c.out_proofs48 ? ensure_cellproof_tab(ctx) : 0;
  if (rc == 0) rc = columns_cells_enqueue(ctx, c, c.in, n, c.out_cells, n, 0, c.status, st);
  if (rc || (!c.out_proofs48 && !c.out_commitments48)) return rc;
  return with_workspace(ctx, st, [&] {
    const std::vector<uint8_t> want = column_want_masks(c, n);
    const std::vector<Pass> plan = cellplan::plan(want.data(), n, cellproof_pass(ctx));
    const uint64_t call_pairs = cellplan::total_vectors(plan);
    Carve head;
    head.take(call_pairs * sizeof(uint32_t));  // the pair list stays in front of everything, as in every pass's layout
    const size_t need = std::max(cellsel_ws_bytes(ctx, call_pairs, plan), c.out_commitments48 ? columns_commit_ws(ctx, n, head.off) : (size_t)0);
    int32_t e = ws_reserve(ctx, need, st);
    if (e) return e;
    uint8_t* ws = ws_ptr(ctx);
    const uint32_t* d_pairs = reinterpret_cast<const uint32_t*>(ws);
    if (call_pairs) {
      kzg_ctx::PairPin* pin = nullptr;
      e = pair_pin_take(ctx, call_pairs * sizeof(uint32_t), &pin);
      if (e) return e;
      cellplan::write_all_pairs(want.data(), plan, static_cast<uint32_t*>(pin->p));
      HIP_TRY(hipMemcpyAsync(ws, pin->p, call_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      HIP_TRY(hipEventRecord(pin->ev, st));
    }
    if (c.out_commitments48) {
      e = columns_commit(ctx, c.in, n, c.out_commitments48, c.status, head.off, st);
      if (e) return e;
    }
    uint64_t base = 0, voff = 0;
    for (const Pass& p : plan) {
      const ColumnRows rows{n, base};
      e = cellsel_pass(ctx, recover ? c.out_cells : c.in + base * (uint64_t)KZG_BYTES_PER_BLOB, KZG_BYTES_PER_BLOB, recover, true, p, d_pairs + voff, nullptr,
                       c.out_proofs48, c.status + base, cellsel_layout(ctx, call_pairs, p), ws, st, &rows);
      if (e) return e;
      base += p.items;
      voff += p.vectors;
    }
    if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "data column pipeline launch failed");
    return 0;
  });
}

// The host-buffer call on one device, over rows [first, first + n) of the caller's matrices of `rows` rows (a group member's share; the
// whole call on a single device).  A staging slot holds a pass of m rows column-major with pitch m -- the input (recover) and the cells
// behind it -- and the copies between it and the caller's matrices are 2-D, between pitch 2048 m and pitch 2048 rows: the rows of every
// column go straight to their places.  produce: the blobs go up once, blob-major, for cells, commitments and proofs alike; only columns
// 64..127 come down, and columns 0..63 are copied from the caller's blobs on the host once the statuses are there (cells_first_halves'
// reason).  Proofs: a pass's compact proofs are put column-major with pitch m in the workspace, and the wanted columns -- `want` is one
// mask, so a column is wanted for all rows or for none -- come down in runs of consecutive columns, 48 m bytes per column; the wanted
// positions of a rejected row arrive as the zero bytes the MSM's encoder wrote, and no other position of the caller's matrix is written.
static int32_t columns_host(const kzg_ctx* ctx, const ColumnCall& c, uint64_t rows, uint64_t first, uint64_t n) {
  if (n == 0) return 0;
  const bool recover = c.present != nullptr, proofs = c.out_proofs48 != nullptr;
  int32_t rc = proofs ? ensure_cellproof_tab(ctx) : 0;
  if (rc) return rc;
  std::vector<uint8_t> want;
  std::vector<Pass> sel_plan;
  std::vector<uint32_t> pairs;  // lives until close() has synchronised
  std::vector<uint64_t> items_plan;
  if (proofs) {
    want = column_want_masks(c, n);
    sel_plan = cellplan::plan(want.data(), n, cellproof_pass(ctx));
    pairs.resize(cellplan::total_vectors(sel_plan));
    cellplan::write_all_pairs(want.data(), sel_plan, pairs.data());
    for (const Pass& p : sel_plan) items_plan.push_back(p.items);
  } else {
    items_plan = even_plan(n, ctx->knobs.cells_pass ? ctx->knobs.cells_pass : CELLS_OF_CELL_SETS.cells_pass);
  }
  const size_t up_bytes = recover ? KZG_BYTES_PER_CELL_SET : (size_t)KZG_BYTES_PER_BLOB;
  HostCall hc(ctx);
  const int a_com = hc.download(c.out_commitments48 ? c.out_commitments48 + first * 48 : nullptr, n * 48), a_st = hc.download(c.status + first, n * sizeof(int32_t)),
            a_pairs = hc.upload(pairs.empty() ? nullptr : pairs.data(), pairs.size() * sizeof(uint32_t));
  rc = hc.open(items_plan, up_bytes + KZG_BYTES_PER_CELL_SET);
  if (rc) return rc;
  uint8_t* d_com = hc.dev(a_com);
  const uint32_t* d_pairs = hc.dev<uint32_t>(a_pairs);
  int32_t* d_status = hc.dev<int32_t>(a_st);
  // workspace of a pass: the select pass's layout (no pair list: it is in the host-i/o pool) and behind it the pass's proofs, column-major
  auto colprf_off = [&](const Pass& p) { return cellsel_layout(ctx, 0, p).total; };
  uint64_t voff = 0;
  auto pass_body = [&](size_t k, uint64_t base, uint64_t m, uint8_t* d_in) -> int32_t {
    uint8_t* d_cells = d_in + hc.max_pass * up_bytes;
    int32_t e = columns_cells_enqueue(ctx, c, d_in, m, d_cells, m, 0, d_status + base, hc.st);
    if (e) return e;
    const uint64_t col0 = recover ? 0 : KZG_CELLS_PER_EXT_BLOB / 2;  // produce: the extension half only
    if (hipMemcpy2DAsync(c.out_cells + (col0 * rows + first + base) * KZG_BYTES_PER_CELL, rows * KZG_BYTES_PER_CELL, d_cells + col0 * m * KZG_BYTES_PER_CELL,
                         m * KZG_BYTES_PER_CELL, m * KZG_BYTES_PER_CELL, KZG_CELLS_PER_EXT_BLOB - col0, hipMemcpyDeviceToHost, hc.st) != hipSuccess)
      return fail(KZG_FAIL_HIP, "device-to-host copy failed");
    if (d_com) {
      e = columns_commit(ctx, d_in, m, d_com + base * 48, d_status + base, 0, hc.st);
      if (e) return e;
    }
    if (!proofs) return 0;
    const Pass& p = sel_plan[k];
    uint8_t* d_colprf = ws_ptr(ctx) + colprf_off(p);
    const ColumnRows pass_rows{m, 0};
    e = cellsel_pass(ctx, recover ? d_cells : d_in, KZG_BYTES_PER_BLOB, recover, true, p, d_pairs + voff, nullptr, d_colprf, d_status + base, cellsel_layout(ctx, 0, p),
                     ws_ptr(ctx), hc.st, &pass_rows);
    voff += p.vectors;
    if (e || p.vectors == 0) return e;
    for (uint32_t c0 = 0; c0 < cellplan::CELLS;) {  // runs of wanted columns
      if (!cellplan::wanted(want.data(), c0)) {
        c0++;
        continue;
      }
      uint32_t c1 = c0 + 1;
      while (c1 < cellplan::CELLS && cellplan::wanted(want.data(), c1)) c1++;
      if (hipMemcpy2DAsync(c.out_proofs48 + ((uint64_t)c0 * rows + first + base) * 48, rows * 48, d_colprf + (uint64_t)c0 * m * 48, m * 48, m * 48, c1 - c0,
                           hipMemcpyDeviceToHost, hc.st) != hipSuccess)
        return fail(KZG_FAIL_HIP, "device-to-host copy failed");
      c0 = c1;
    }
    return 0;
  };
  auto enqueue = [&] {
    return recover ? hc.passes_of_rows(c.in + first * KZG_BYTES_PER_CELL, KZG_BYTES_PER_CELL, KZG_CELLS_PER_EXT_BLOB, rows, pass_body)
                   : hc.passes(c.in + first * (size_t)KZG_BYTES_PER_BLOB, KZG_BYTES_PER_BLOB, pass_body);
  };
  if (proofs || d_com)
    rc = with_workspace(ctx, hc.st, [&] {
      size_t need = 0;  // sized before anything is in flight, for the pass that asks most: a short last pass may take more splits than a full one
      for (uint64_t m : hc.plan) need = std::max(need, d_com ? columns_commit_ws(ctx, m, 0) : (size_t)0);
      for (const Pass& p : sel_plan) need = std::max(need, colprf_off(p) + p.items * (size_t)(KZG_CELLS_PER_EXT_BLOB * 48));
      const int32_t e = ws_reserve(ctx, need, hc.st);
      return e ? e : enqueue();
    });
  else
    rc = enqueue();
  if (rc == 0 && hipGetLastError() != hipSuccess) rc = fail(KZG_FAIL_HIP, "data column pipeline launch failed");
  rc = hc.close(rc);
  if (rc == 0 && !recover) {  // columns 0..63 of every row: the caller's blob, or zero bytes
    for (uint64_t b = first; b < first + n; b++)
      for (uint64_t col = 0; col < KZG_CELLS_PER_EXT_BLOB / 2; col++) {
        uint8_t* dst = c.out_cells + (col * rows + b) * KZG_BYTES_PER_CELL;
        if (c.status[b] == 0)
          memcpy(dst, c.in + b * (size_t)KZG_BYTES_PER_BLOB + col * KZG_BYTES_PER_CELL, KZG_BYTES_PER_CELL);
        else
          memset(dst, 0, KZG_BYTES_PER_CELL);
      }
  }
  return rc;
}
static int32_t columns_on_members(const kzg_ctx* ctx, const ColumnCall& c, uint64_t n) {
  return on_members(ctx, n, [&](const kzg_ctx* m, uint64_t first, uint64_t count) { return columns_host(m, c, n, first, count); });
}

extern "C" int32_t kzg_compute_data_columns_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_commitments48, uint8_t* out_column_cells,
                                                  uint8_t* out_column_proofs48, int32_t* status) try {
  if (!ctx || (n && (!blobs || !out_column_cells || !out_column_proofs48 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return columns_on_members(ctx, ColumnCall{blobs, nullptr, nullptr, out_commitments48, out_column_cells, out_column_proofs48, status}, n);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_compute_data_columns_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out_commitments48, void* d_out_column_cells,
                                                      void* d_out_column_proofs48, void* d_status, void* hip_stream) try {
  if (!ctx || (n && (!d_blobs || !d_out_column_cells || !d_out_column_proofs48 || !d_status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return columns_dev(ctx, ColumnCall{(const uint8_t*)d_blobs, nullptr, nullptr, (uint8_t*)d_out_commitments48, (uint8_t*)d_out_column_cells,
                                     (uint8_t*)d_out_column_proofs48, (int32_t*)d_status},
                     n, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
// recover: the proofs pointer is null iff want16 is -- then it is kzg_recover_cells_batch in the column layout, with no table built and no workspace
extern "C" int32_t kzg_recover_data_columns_batch(const kzg_ctx* ctx, const uint8_t* column_cells, const uint8_t* present16, const uint8_t* want16, uint64_t n,
                                                  uint8_t* out_column_cells, uint8_t* inout_column_proofs48, int32_t* status) try {
  if (!ctx || (n && (!column_cells || !present16 || !out_column_cells || !status || (want16 == nullptr) != (inout_column_proofs48 == nullptr))))
    return fail(KZG_FAIL_ARGUMENT, "null argument");
  return columns_on_members(ctx, ColumnCall{column_cells, present16, want16, nullptr, out_column_cells, inout_column_proofs48, status}, n);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_recover_data_columns_batch_dev(const kzg_ctx* ctx, const void* d_column_cells, const uint8_t* present16, const uint8_t* want16, uint64_t n,
                                                      void* d_out_column_cells, void* d_inout_column_proofs48, void* d_status, void* hip_stream) try {
  if (!ctx || (n && (!d_column_cells || !present16 || !d_out_column_cells || !d_status || (want16 == nullptr) != (d_inout_column_proofs48 == nullptr))))
    return fail(KZG_FAIL_ARGUMENT, "null argument");
  return columns_dev(ctx, ColumnCall{(const uint8_t*)d_column_cells, present16, want16, nullptr, (uint8_t*)d_out_column_cells, (uint8_t*)d_inout_column_proofs48,
                                     (int32_t*)d_status},
                     n, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
extern "C" uint64_t kzg_ctx_cellproof_vectors(const kzg_ctx* ctx) {
  if (!ctx) return 0;
  uint64_t total = ctx->cellproof_vectors.load(std::memory_order_relaxed);
  for (const kzg_ctx* p : ctx->peers) total += p->cellproof_vectors.load(std::memory_order_relaxed);
  return total;
}

void warm_code_object_proof() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, (const void*)k_poly_root_inverse);
  (void)hipGetLastError();
}
