// verify_blob_kzg_proof_batch and the single-item verification entry points.  Device work: per-item validation, challenges,
// evaluations, transcript digests, random-linear-combination MSMs.  Host work:
// hashing ~n/8 bytes of transcript nodes, the W-step Horner combine of the
// MSM windows, and the single two-pairing check (pairing.hpp).

#include <chrono>

#include "engine_internal.hpp"
#include "multi_split.hpp"

#include <thread>
#include "verify_kernels.cuh"
#include "cellverify_kernels.cuh"
#include "host_lincomb.hpp"
#include "each_descent.hpp"
// A verification session: device scratch for n items, a second stream (point decoding beside the evaluation kernel,
// lincomb A beside lincomb B) and its fork/join events.  Sessions are POOLED in the context (kzg_ctx::session_pool): a
// call takes one (growing its buffer if the batch is larger than any before), and kzg_verify_session_destroy hands it
// back, so steady-state verification allocates nothing and concurrent callers never share a stream or a buffer.
struct kzg_verify_session {
  const kzg_ctx* ctx = nullptr;
  uint64_t n = 0;
  // The commitments of the current use: ncom == n and rows == false in every form but the cells kind's row-indexed one
  // (kzg_verify_cell_proof_batch_rows), where the call brings a LIST of ncom commitments and an index per item.  Wherever "proofs then
  // commitments" are laid out the count is n + ncom; with ncom == n every size, offset and launch is the per-item form's.
  uint64_t ncom = 0;
  bool rows = false;
  uint64_t stride = 0;         // words per status array: max(n, ncom)
  hipStream_t st = nullptr;    // the caller's stream of the current use
  hipStream_t side = nullptr;  // owned: the point decoder
  hipStream_t aux = nullptr;   // owned: lincomb A (the decoder may still hold `side` when its sorting starts)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;  // owned
  hipEvent_t ev_nodes = nullptr, ev_stat = nullptr, ev_aux = nullptr;  // owned: transcript digests read back; statuses read back; aux fork
  uint8_t* buf = nullptr;      // owned: one device allocation of `cap` bytes, carved below
  size_t cap = 0;
  VerifyKind kind = VerifyKind::BLOBS;  // set when the session is acquired: every kind-dependent site below reads verify_kind.hpp's row of it
  uint64_t tail = 1;       // facts(kind).tail_terms: lincomb B's terms behind the 2n points, the generator or the cells kind's 64 monomial points
  uint4* aff = nullptr;    // [n+ncom+tail] affine points: proofs, commitments, generator | monomial points
  uint8_t* inf = nullptr;  // [n+ncom+tail]
  fr_t* z = nullptr;       // [n] plain
  fr_t* y = nullptr;       // [n] plain
  fr_t* scal = nullptr;    // [n+ncom+tail] plain: r_i*z_i (n), r_i (n) | rows: w_c (ncom), -sum r_i*y_i | cells: -S_j (64)
  bool glv = false;        // n >= 32,768: both lincombs on GLV-split scalars (use_glv)
  fr_t* glv_b = nullptr;   // [2 (2n+tail)]: k1 | k2 of scal
  fr_t* glv_a = nullptr;   // [2n]: k1 | k2 of the r_i
  int32_t* stat = nullptr;   // [4 stride] one status array per entry of the kind's error record (stat_of)
  unsigned long long* first4 = nullptr;  // verify_proof_batch: (index << 32) | code of the first rejected proof, commitment, z, y (k_first_errors)
  uint32_t* leaves = nullptr;  // transcript: n leaves, ceil(n / 16) mid digests, ceil(n / 256) nodes
  uint32_t* mids = nullptr;
  uint32_t* nodes = nullptr;
  uint8_t* pts48 = nullptr;  // [(n + ncom) * 48] device copy of proofs || commitments (host-buffer entry points)
  uint8_t* zy32 = nullptr;   // [2n * 32] device copy of z || y as given (host-buffer verify_proof_batch)
  uint8_t* msm_a = nullptr;  // scratch of the two lincomb MSMs (carved from buf: no allocation in phase 2)
  uint8_t* msm_b = nullptr;
  fr_t* rpow2 = nullptr;     // [64] r^(2^k)
  fr_t* ysum = nullptr;      // per-block partial sums of r_i*y_i
  // host read-back, PINNED (owned): the copies are enqueued and waited for by event, so the host can go on enqueueing while the
  // decoder still runs
  int32_t* h_stat = nullptr;    // [3n]
  uint32_t* h_nodes = nullptr;  // [ceil(n / 256) * 8]
  unsigned long long* h_first4 = nullptr;  // [4] read-back of first4
  size_t h_cap = 0;
  const uint8_t* d_cells = nullptr;  // the cells kind (front_enqueue records them): phase 2 reads the cells again
  const uint64_t* d_cell_indices = nullptr;
  fr_t* cell_part = nullptr;   // [ceil(n / CELLV_CELLS) x 64] k_cells_interp's partial coefficient vectors
  uint8_t* cells_in = nullptr; // [n * 2048 | n * 8 | rows: n * 8] device copy of cells || cell indices || commitment indices (host-buffer entry point)
  // the row-indexed form only: lincomb A's scalars r^k cannot live in B's commitment slots (those hold the ncom weights w_c)
  const uint64_t* d_com_indices = nullptr;  // front_enqueue records them: phase 2 reads them again
  fr_t* rpow = nullptr;        // [n] plain r^k: k_batch_scalars' sa, k_cells_interp's rpow_plain, lincomb A's scalars
  fr_t* roww_part = nullptr;   // [ncom x cellv_roww_tiles(n)] k_cells_row_weights' tile partials
  // the blob form only (kzg_verify_blob_cell_proofs_batch: rows with implicit indices, n = 128 ncom): no cells, no index arrays
  bool from_blobs = false;
  const uint8_t* d_blobs = nullptr;  // front_enqueue records them: cells 0..63 of every blob, read again in phase 2
  uint8_t* ext = nullptr;            // [ncom * 131072] cells 64..127 (k_compute_cells_ext)
  int32_t* blob_stat = nullptr;      // [ncom] that kernel's statuses: the blob entry of the error record
  int32_t* blob_code = nullptr;      // [ncom] per-blob codes of the *_each form (k_each_blob_status)
  // per-item verdicts (kzg_verify_*_batch_each, kzg_verify_session_tree): a device allocation of its own (owned), made on first use
  // and kept with the pooled session; carved by each_carve for the current n
  uint8_t* tree = nullptr;
  size_t tree_cap = 0;
  uint64_t tree_n = 0;             // items the trees stand for; 0 = not built in this use of the session
  int32_t* t_status = nullptr;     // [n] the single-item call's code per item (k_each_status)
  uint32_t* t_rejected = nullptr;  // [2] how many of them are non-zero; rows: [1] = how many LISTED commitments the decoder rejected
  g1_xyzz28* t_a = nullptr;        // both trees, level after level from the leaves (EachGeom::off)
  g1_xyzz28* t_b = nullptr;
  uint32_t* t_idx = nullptr;       // [EACH_GATHER] node positions of one fetch
  g1_xyzz* t_out = nullptr;        // [2 EACH_GATHER] the fetched nodes, A and B side by side
  fr_t* t_vec = nullptr;           // cells: the third tree, a node = 64 coefficients (k_cells_each_leaves, k_each_vec_level), same geometry
};

static void session_free(kzg_verify_session* s) {
  if (!s) return;
  if (s->buf) (void)hipFree(s->buf);
  if (s->tree) (void)hipFree(s->tree);
  if (s->h_stat) (void)hipHostFree(s->h_stat);
  if (s->side) (void)hipStreamDestroy(s->side);
  if (s->aux) (void)hipStreamDestroy(s->aux);
  for (hipEvent_t e : {s->ev_fork, s->ev_join, s->ev_nodes, s->ev_stat, s->ev_aux})
    if (e) (void)hipEventDestroy(e);
  delete s;
}
// the status array of entry `entry` of the session's error record (verify_kind.hpp); null for an entry the record does not have
static int32_t* stat_of(const kzg_verify_session* s, int entry) {
  const int slot = facts(s->kind).slot[entry];
  return slot < 0 ? nullptr : s->stat + (uint64_t)slot * s->stride;
}
static const host::miller_lines& lines_against_a(const kzg_ctx* ctx, VerifyKind kind) {  // the G2 point of the pairing against A
  return facts(kind).pair_tau64 ? ctx->pairing->lines_tau64 : ctx->pairing->lines_tau;
}
void session_pool_clear(const kzg_ctx* ctx) {
  std::lock_guard<std::mutex> guard(ctx->pool_lock);
  for (kzg_verify_session* s : ctx->session_pool) session_free(s);
  ctx->session_pool.clear();
}

// Waits for everything this use has enqueued on the session's three streams, ALWAYS all three (errors ignored).  Two rules, each
// stated once in code: nothing runs on a session when it re-enters the pool (kzg_verify_session_destroy, reached through SessionUse),
// and nothing runs on a Phase2's scratch when it goes (~Phase2).  The caller has set the session's device.
static void session_drain(kzg_verify_session* s) {
  (void)hipStreamSynchronize(s->st);
  (void)hipStreamSynchronize(s->aux);
  (void)hipStreamSynchronize(s->side);
}

// hands the session back to its context's pool (at most 8 are kept)
extern "C" void kzg_verify_session_destroy(kzg_verify_session* s) {
  if (!s) return;
  const kzg_ctx* ctx = s->ctx;
  (void)hipSetDevice(ctx->device);
  session_drain(s);
  std::lock_guard<std::mutex> guard(ctx->pool_lock);
  if (ctx->session_pool.size() < 8)
    ctx->session_pool.push_back(s);
  else
    session_free(s);
}

// The session of ONE use: whatever way the owner leaves -- a result, an error code, a HIP_TRY -- the session goes back to the pool,
// drained.  release(): phase 1 on its own hands the session to the caller, who ends it with kzg_verify_session_destroy.
struct SessionUse {
  kzg_verify_session* s = nullptr;
  SessionUse() = default;
  SessionUse(const SessionUse&) = delete;
  SessionUse& operator=(const SessionUse&) = delete;
  ~SessionUse() { reset(); }
  void reset() {
    kzg_verify_session_destroy(s);
    s = nullptr;
  }
  kzg_verify_session* release() {
    kzg_verify_session* out = s;
    s = nullptr;
    return out;
  }
};

// Window sizes.  Up to 32,767 terms: c = 8 (32 windows whose TOP window is full -- top raw digit 7 bits, all 128 signed
// buckets used; with e.g. c = 12 the top window has 8 distinct digits and a few buckets receive n/8 points each, a serial
// chain that dominated the batch), every bucket split over K threads, k_var_fold + k_var_windows; c = 4 for a handful of terms.
// From 32,768 terms on (measured: 8,192 items 7.06 ms flat / 6.59 ms classic, 16,384 items even, 32,768 items 13.06 / 14.09,
// 65,536 items 17.9 / 18.7) the FLAT path: c = 13, 20 windows, 4,096 buckets
// per full window = enough buckets for one thread each (no fold), 37 % fewer bucket additions, the top window's <= 232
// magnitudes handled with 16 threads per bucket, and bit sums instead of running sums (k_var_bitsums).
// Since late round 5 the flat path's full windows are summed by EQUAL SHARES of the sorted entry list per lane (k_var_buckets_seg,
// verify_kernels.cuh; g.seg entries per lane, chosen below so that all the lincombs that run side by side are one round of waves) and a
// fix-up pass for the buckets that cross share boundaries; KATETH_AMD_VAR_SEG=0 keeps one thread per bucket (k_var_buckets_flat).
// GLV (glv.cuh, round 5; KATETH_AMD_VAR_GLV=1 -- measured and NOT the default): both lincombs take their scalars split at z^2 --
// twice the terms, 128-bit scalars: c = 13, TEN windows (nine full + bits 117..127: both halves are < z^2 = 0.673 * 2^128, so a
// raw top digit <= 1,378, + 1 carry, never negated: 1,379 magnitudes with three times a full window's load each -> 3 threads per
// bucket), i.e. the same bucket additions, 130 bit sums instead of 260 and a Horner loop of 130 steps on the host.  Why it lost
// (15.04 against 14.83 ms per 65,536 triples, profiles/r05/verify_glv_rejected.json): the bit sums are ONE round of latency-bound
// workgroups whether there are 260 or 130 of them, and half the windows means half as many bucket THREADS with chains twice as
// long (A: 40,960 threads x 32 entries instead of 81,920 x 16 on a chip with 131,072 lanes at this register budget): the bucket
// kernels went from 1.13 / 0.53 ms to 1.43 / 1.26 ms, against 0.1 ms saved in the host's Horner loops.
static bool use_glv(const kzg_ctx* ctx, uint64_t n_items, bool rows = false) {  // not for the cells kind's row-indexed form
  return !rows && n_items >= 32768 && !ctx->knobs.var_msm_classic && ctx->knobs.var_glv;
}
// seg_total: the terms of ALL the lincombs whose bucket kernels run side by side (batch verification: n + 2 n + 1), so that their
// lanes together are one round of the chip: 0 = this lincomb alone.
static VarGeom choose_var_geom(const kzg_ctx* ctx, uint64_t nterms, bool glv = false, uint64_t seg_total = 0) {
  VarGeom g;
  g.top_n = 0;
  g.ktop = 1;
  g.seg = 0;
  if (glv) {
    g.c = 13u;
    g.W = 10u;
    g.half = 1u << 12;
    g.top_n = 1380u;  // both halves are below z^2 = 0.673 * 2^128: raw top digit <= 1,378, + 1 carry
    g.ktop = 3u;      // 1,379 used buckets with 4,096 / 1,379 = 2.97 times a full window's load each: three threads per bucket
    return g;
  }
  if (nterms >= 32768 && !ctx->knobs.var_msm_classic) {
    g.c = 13u;
    g.W = 20u;  // 19 full windows + bits 247..254: a scalar < r has a raw top digit <= r >> 247 = 231, + 1 carry, never negated
    g.half = 1u << 12;
    g.top_n = 256u;
    g.ktop = 16u;  // top_n * ktop = half: the top window costs k_var_bitsums what a full window does
    if (ctx->knobs.var_seg) {
      // equal shares of the sorted entry list per lane (k_var_buckets_seg): the chip holds two waves of these kernels per SIMD
      // (232 VGPRs) = 131,072 lanes on 256 CUs; 9,280 of them are the two top windows' threads, the rest is left a margin of
      // one wave in sixteen: 7/8 of the lanes for the shares (114,688 on an MI355X)
      const uint64_t entries = (seg_total ? seg_total : nterms) * (uint64_t)(g.W - 1u);
      const uint64_t lanes = (uint64_t)ctx->num_cus * 4u * 2u * 64u * 7u / 8u;
      g.seg = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((entries + lanes - 1) / lanes, 16), 4096);
      if (ctx->knobs.var_seg >= 2u) g.seg = ctx->knobs.var_seg;
      // the top window's 232 possible magnitudes (231 + a carry) over 20 threads each: a thread's strided list is then SHORTER than a
      // share (2 n / 232 / 20 = n / 2,320 entries against 3 n * 19 / 114,688 = n / 2,012) -- with 16 it was the longer lincomb's
      // longest chain (35-40 entries at 65,536 triples against shares of 33); k_var_bitsums sums 2,340 instead of 2,064 stored points
      // per top-window bit: one addition more in 18
      g.top_n = 232u;
      g.ktop = 20u;
    }
    return g;
  }
  g.c = nterms >= 64 ? 8u : 4u;
  g.W = (256 + g.c - 1) / g.c;
  g.half = 1u << (g.c - 1);
  return g;
}

// host: sum_j 2^(c*j) * window[j]   (classic path), or sum_p 2^p * T[p] over the bit sums T[c j + b] (flat path)
static void host_horner(g1_xyzz& out, const std::vector<g1_xyzz>& win, const VarGeom& g) {
  g1_xyzz acc;
  xyzz_set_inf(acc);
  if (g.top_n) {
    for (int p = (int)(g.W * g.c) - 1; p >= 0; p--) {
      xyzz_dbl(acc);
      xyzz_add(acc, win[p]);
    }
    out = acc;
    return;
  }
  for (int j = (int)g.W - 1; j >= 0; j--) {
    for (uint32_t k = 0; k < g.c; k++) xyzz_dbl(acc);
    xyzz_add(acc, win[j]);
  }
  out = acc;
}

static void host_affine_from_xyzz(host::g1_host_affine& out, const g1_xyzz& p) {
  out.inf = !xyzz_to_affine(out.x, out.y, p);
  if (out.inf) {
    bn_zero(out.x);
    bn_zero(out.y);
  }
}
static void host_affine_to_be96(uint8_t* out96, const host::g1_host_affine& a) {
  if (a.inf) {
    memset(out96, 0, 96);
    return;
  }
  fp_t xp, yp;
  from_mont<FpParams>(xp, a.x);
  from_mont<FpParams>(yp, a.y);
  fp_to_be_bytes_plain(out96, xp);
  fp_to_be_bytes_plain(out96 + 48, yp);
}
static bool host_affine_from_be96(host::g1_host_affine& a, const uint8_t* in96) {
  bool zero = true;
  for (int i = 0; i < 96; i++) zero = zero && (in96[i] == 0);
  if (zero) {
    a.inf = true;
    bn_zero(a.x);
    bn_zero(a.y);
    return true;
  }
  fp_t xp, yp;
  fp_from_be_bytes_plain(xp, in96);
  fp_from_be_bytes_plain(yp, in96 + 48);
  if (bn_geq(xp, modulus<FpParams>()) || bn_geq(yp, modulus<FpParams>())) return false;
  to_mont<FpParams>(a.x, xp);
  to_mont<FpParams>(a.y, yp);
  a.inf = false;
  return true;
}

// variable-base MSM over `nterms` device-resident terms, split into an asynchronous launch
// (kernels + window read-back enqueued on `st`) and a finish (synchronise, Horner on the host)
// so that independent MSMs can run concurrently on different streams.
struct MsmVarLayout {
  VarGeom g{};
  uint32_t nb = 0, K = 1;
  size_t o_counts = 0, o_offsets = 0, o_cursors = 0, o_entries = 0, o_part = 0, o_bsum = 0, o_win = 0, o_seg = 0, total = 0;
  uint32_t nseg = 0;  // lanes of the balanced bucket kernel (an upper bound: digits that are zero make no entry)
};
static MsmVarLayout msm_var_layout(const kzg_ctx* ctx, uint64_t nterms, bool glv = false, uint64_t seg_total = 0) {
  MsmVarLayout L;
  if (nterms == 0) return L;
  L.g = choose_var_geom(ctx, nterms, glv, seg_total);
  L.nb = L.g.W * L.g.half;
  Carve pool;
  L.o_counts = pool.take((size_t)(L.nb + 1) * 4);
  L.o_offsets = pool.take((size_t)(L.nb + 1) * 4);
  L.o_cursors = pool.take((size_t)(L.nb + 1) * 4);
  L.o_entries = pool.take((size_t)nterms * L.g.W * 4);
  // split every bucket over K threads (power of two <= 64) so that a thread chains ~16 additions
  if (L.g.top_n) {  // flat path: partials only for the top window; one output point per (window, bit)
    L.o_part = pool.take((size_t)L.g.top_n * L.g.ktop * sizeof(g1_xyzz28));
    L.o_bsum = pool.take((size_t)L.nb * sizeof(g1_xyzz28));
    L.o_win = pool.take((size_t)L.g.W * L.g.c * sizeof(g1_xyzz));
    if (L.g.seg) {
      L.nseg = (uint32_t)((nterms * (uint64_t)(L.g.W - 1u) + L.g.seg - 1u) / L.g.seg);
      L.o_seg = pool.take((size_t)L.nseg * 2u * sizeof(g1_xyzz28));
    }
    L.total = pool.off;
    return L;
  }
  uint64_t load = nterms / L.g.half + 1;
  while (L.K < 64 && (uint64_t)L.K * 16 < load) L.K <<= 1;
  L.o_part = pool.take((size_t)L.nb * L.K * sizeof(g1_xyzz28));
  L.o_bsum = pool.take((size_t)L.nb * sizeof(g1_xyzz28));
  L.o_win = pool.take((size_t)L.g.W * sizeof(g1_xyzz));
  L.total = pool.off;
  return L;
}

struct MsmVarJob {
  MsmVarLayout L{};
  uint64_t nterms = 0;
  bool trace = false;  // KATETH_AMD_TRACE (read at context creation)
  VarGeom g{};
  uint32_t nout = 0;  // points read back: W window sums, or W*c bit sums on the flat path
  uint8_t* buf = nullptr;
  bool owns_buf = false;  // no scratch was handed in: `buf` is this job's own allocation
  std::vector<g1_xyzz> win;
  const g1_xyzz* d_win = nullptr;
  hipStream_t st = nullptr;
  bool active = false;
  MsmVarJob() = default;
  MsmVarJob(const MsmVarJob&) = delete;
  MsmVarJob& operator=(const MsmVarJob&) = delete;
  ~MsmVarJob() { release(); }  // a job that is dropped with kernels enqueued: its owner has drained the streams (~Phase2)
  void release() {
    if (owns_buf && buf) (void)hipFree(buf);
    buf = nullptr;
    owns_buf = false;
  }
};

// The launch comes in two halves so that batch verification can run the first beside the point decoder:
//   msm_var_sort        -- digits, histogram, scan, scatter: needs the SCALARS only.  `d_inf` = null: points at infinity are not
//                          filtered here (their flags may not exist yet); they are all-zero entries that the bucket chains skip.
//                          `lean`: the scan kernel that fits beside two decoder waves (flat path).
//   msm_var_accumulate  -- bucket sums and bit / window sums: needs the decoded POINTS.
// `glv`: the scalars are the 128-bit halves of a GLV split (k_glv_split): terms [0, split) on points [0, split), terms [split, nterms)
// on the [z^2]-images at second_base + (t - split) (k_glv_points).
static int32_t msm_var_sort(const kzg_ctx* ctx, MsmVarJob& job, const uint8_t* d_inf, const fr_t* d_scalars, uint64_t nterms, hipStream_t st,
                            uint8_t* prealloc, bool lean, bool glv = false, uint64_t split = 0, uint64_t second_base = 0, uint64_t seg_total = 0) {
  job.active = false;
  job.st = st;
  job.nterms = nterms;
  job.trace = ctx->knobs.trace;
  if (nterms == 0) return 0;
  if (!glv) split = nterms;
  job.L = msm_var_layout(ctx, nterms, glv, seg_total);
  const MsmVarLayout& L = job.L;
  const VarGeom g = L.g;
  job.g = g;
  const uint32_t nb = L.nb;
  if (prealloc) {
    job.buf = prealloc;
    job.owns_buf = false;
  } else {
    HIP_TRY(hipMalloc(&job.buf, L.total));
    job.owns_buf = true;
  }
  uint8_t* buf = job.buf;
  uint32_t* counts = (uint32_t*)(buf + L.o_counts);
  uint32_t* offsets = (uint32_t*)(buf + L.o_offsets);
  uint32_t* cursors = (uint32_t*)(buf + L.o_cursors);
  uint32_t* entries = (uint32_t*)(buf + L.o_entries);
  job.nout = g.top_n ? g.W * g.c : g.W;
  job.win.resize(job.nout);
  job.active = true;
  HIP_TRY(hipMemsetAsync(counts, 0, (size_t)(nb + 1) * 4, st));
  hipLaunchKernelGGL(k_var_count, dim3(blocks_for(nterms, 256)), dim3(256), 0, st, d_scalars, d_inf, nterms, g, counts);
  if (g.top_n) {
    if (nb > 1024u * 80u || g.top_n * g.ktop > g.half + 1024u) return fail(KZG_FAIL_ARGUMENT, "flat MSM geometry out of range");
    if (lean)
      hipLaunchKernelGGL(k_var_scan_lean, dim3(1), dim3(256), 0, st, counts, nb, (nb / 256u + 3u) & ~3u, offsets, cursors);  // nb = 20 * 4096 = 256 * 320
    else
      hipLaunchKernelGGL(k_var_scan_wide<80>, dim3(1), dim3(1024), 0, st, counts, nb, offsets, cursors);  // nb = 20 * 4096 = 1024 * 80
  } else {
    hipLaunchKernelGGL(k_var_scan, dim3(1), dim3(1024), 0, st, counts, nb, offsets, cursors);
  }
  hipLaunchKernelGGL(k_var_scatter, dim3(blocks_for(nterms, 256)), dim3(256), 0, st, d_scalars, d_inf, nterms, g, cursors, entries, split, second_base);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int32_t msm_var_accumulate(const kzg_ctx* ctx, MsmVarJob& job, const uint4* d_points, hipStream_t st) {
  (void)ctx;
  if (!job.active) return 0;
  const MsmVarLayout& L = job.L;
  const VarGeom g = L.g;
  const uint32_t nb = L.nb, K = L.K;
  uint8_t* buf = job.buf;
  uint32_t* offsets = (uint32_t*)(buf + L.o_offsets);
  uint32_t* entries = (uint32_t*)(buf + L.o_entries);
  g1_xyzz28* bpart = (g1_xyzz28*)(buf + L.o_part);
  g1_xyzz28* bsum = (g1_xyzz28*)(buf + L.o_bsum);
  g1_xyzz* winsum = (g1_xyzz*)(buf + L.o_win);
  if (g.top_n) {
    const uint32_t regular = (g.W - 1) * g.half;
    if (g.seg) {
      g1_xyzz28* segpart = (g1_xyzz28*)(buf + L.o_seg);
      hipLaunchKernelGGL(k_var_buckets_seg, dim3(blocks_for((uint64_t)L.nseg + (uint64_t)g.top_n * g.ktop, 64)), dim3(64), 0, st, d_points, offsets, entries,
                         regular, g.seg, L.nseg, g.top_n, g.ktop, bsum, bpart, segpart);
      hipLaunchKernelGGL(k_var_seg_fixup, dim3(blocks_for(regular, 64)), dim3(64), 0, st, offsets, regular, g.seg, segpart, bsum);
    } else {
      hipLaunchKernelGGL(k_var_buckets_flat, dim3(blocks_for((uint64_t)regular + (uint64_t)g.top_n * g.ktop, 64)), dim3(64), 0, st, d_points, offsets,
                         entries, regular, g.top_n, g.ktop, bsum, bpart);
    }
    hipLaunchKernelGGL(k_var_bitsums, dim3(g.W * g.c), dim3(256), 0, st, bsum, bpart, g, winsum);
  } else {
    hipLaunchKernelGGL(k_var_buckets, dim3(blocks_for((uint64_t)nb * K, 64)), dim3(64), 0, st, d_points, offsets, entries, nb, K, bpart);
    hipLaunchKernelGGL(k_var_fold, dim3(blocks_for((uint64_t)nb * K, 64)), dim3(64), 0, st, bpart, nb, K, bsum);
    hipLaunchKernelGGL(k_var_windows, dim3(g.W), dim3(64), 0, st, bsum, g, winsum);
  }
  HIP_TRY(hipGetLastError());
  // the window sums are read back in msm_var_finish: a device-to-host copy into pageable memory blocks the host
  // until the stream has drained, which would keep a second job from being enqueued beside this one
  job.d_win = winsum;
  return 0;
}

static int32_t msm_var_launch(const kzg_ctx* ctx, MsmVarJob& job, const uint4* d_points, const uint8_t* d_inf, const fr_t* d_scalars, uint64_t nterms,
                              hipStream_t st, uint8_t* prealloc = nullptr) {
  int32_t rc = msm_var_sort(ctx, job, d_inf, d_scalars, nterms, st, prealloc, false);
  if (rc == 0) rc = msm_var_accumulate(ctx, job, d_points, st);
  return rc;
}

static int32_t msm_var_finish(MsmVarJob& job, g1_xyzz& result) {
  xyzz_set_inf(result);
  if (!job.active) return 0;
  int32_t rc = 0;
  TraceTimer tt(job.trace, job.nterms & 1 ? "msm_var_finish (B)" : "msm_var_finish (A)");
  if (hipMemcpyAsync(job.win.data(), job.d_win, (size_t)job.nout * sizeof(g1_xyzz), hipMemcpyDeviceToHost, job.st) != hipSuccess ||
      hipStreamSynchronize(job.st) != hipSuccess)
    rc = fail(KZG_FAIL_HIP, "variable-base MSM read-back failed");
  tt.mark("kernels done + read-back");
  if (rc == 0) host_horner(result, job.win, job.g);
  tt.mark("horner");
  job.release();  // here, not at the job's end: the scratch is not held through the caller's host work
  job.active = false;
  return rc;
}

static int32_t msm_var(const kzg_ctx* ctx, const uint4* d_points, const uint8_t* d_inf, const fr_t* d_scalars, uint64_t nterms, hipStream_t st,
                       g1_xyzz& result) {
  MsmVarJob job;
  const int32_t rc = msm_var_launch(ctx, job, d_points, d_inf, d_scalars, nterms, st);
  return rc ? rc : msm_var_finish(job, result);
}

static void scan_first_error(const int32_t* st, uint64_t n, int32_t* idx, int32_t* code) {
  *idx = -1;
  *code = 0;
  for (uint64_t i = 0; i < n; i++)
    if (st[i]) {
      *idx = (int32_t)i;
      *code = st[i];
      return;
    }
}

// ---- session set-up -----------------------------------------------------------------------------------------------
struct SessionLayout {
  size_t o_aff, o_inf, o_z, o_y, o_scal, o_glv_b, o_glv_a, o_stat, o_first4, o_leaves, o_mids, o_nodes, o_pts, o_zy, o_msm_a, o_msm_b, o_rpow, o_ysum, o_cell_part,
      o_cells_in, o_rpow_n, o_roww, o_ext, o_blob_stat, o_blob_code, total;
};
// `staged`: room for the device copies of a host-buffer cells call's cells and indices (points_stage_host); the other kinds have nothing
// that is carved on demand.  With one tail term the layout of the blob and points kinds is what it always was.
// `rows`: the cells kind's row-indexed form with a list of `ncom` commitments (n otherwise): n + ncom points, status arrays of
// max(n, ncom) words, and behind everything else the n powers r^k and the weights' tile partials.
// `from_blobs`: rows with implicit indices over ncom blobs (n = 128 ncom): the staged copy is the BLOBS, the weights need no partials, and
// behind everything the extension workspace and the per-blob status words.
static SessionLayout session_layout(const kzg_ctx* ctx, uint64_t n, VerifyKind kind, bool staged, bool rows, uint64_t ncom, bool from_blobs = false) {
  SessionLayout L{};
  const bool is_cells = kind == VerifyKind::CELLS;
  const uint64_t np = n + ncom, stride = std::max(n, ncom);  // proofs then commitments
  const uint64_t tail = facts(kind).tail_terms;
  const uint64_t groups = (n + 255) / 256;
  Carve pool;
  const bool glv = use_glv(ctx, n, rows);
  L.o_aff = pool.take((glv ? 2 : 1) * (np + tail) * 96);  // GLV: the [z^2]-images behind the points
  L.o_inf = pool.take(np + tail);
  L.o_z = pool.take(n * 32 + 32);
  L.o_y = pool.take(n * 32 + 32);
  L.o_scal = pool.take((np + tail) * 32);
  L.o_glv_b = pool.take(glv ? 2 * (np + tail) * 32 : 0);
  L.o_glv_a = pool.take(glv ? 2 * n * 32 : 0);
  L.o_stat = pool.take(4 * stride * 4 + 4);
  L.o_first4 = pool.take(4 * sizeof(unsigned long long));
  L.o_leaves = pool.take(n * 32 + 32);
  L.o_mids = pool.take((n / 16 + 1) * 32 + 32);
  L.o_nodes = pool.take(groups * 32 + 32);
  L.o_pts = pool.take(np * 48 + 48);
  L.o_zy = pool.take(2 * n * 32 + 32);
  L.o_msm_a = pool.take((glv ? msm_var_layout(ctx, 2 * n, true) : msm_var_layout(ctx, n, false, n + np + tail)).total + 256);
  L.o_msm_b = pool.take((glv ? msm_var_layout(ctx, 2 * (np + tail), true) : msm_var_layout(ctx, np + tail, false, n + np + tail)).total + 256);
  L.o_rpow = pool.take(64 * 32);
  L.o_ysum = pool.take(((n + 255) / 256 + 1) * 32);
  L.o_cell_part = pool.take(is_cells ? blocks_for(n, CELLV_CELLS) * (size_t)64 * sizeof(fr_t) : 0);
  L.o_cells_in = pool.take(!(is_cells && staged) ? 0 : from_blobs ? ncom * (size_t)KZG_BYTES_PER_BLOB : n * ((size_t)KZG_BYTES_PER_CELL + 8 + (rows ? 8 : 0)));
  L.o_rpow_n = pool.take(rows ? n * 32 : 0);
  L.o_roww = pool.take(rows && !from_blobs ? ncom * (size_t)cellv_roww_tiles(n) * 32 : 0);
  L.o_ext = pool.take(from_blobs ? ncom * (size_t)KZG_BYTES_PER_BLOB : 0);
  L.o_blob_stat = pool.take(from_blobs ? ncom * sizeof(int32_t) : 0);
  L.o_blob_code = pool.take(from_blobs ? ncom * sizeof(int32_t) : 0);
  L.total = pool.off;
  return L;
}

// Takes a session from the context's pool (or creates one), sized for n items of `kind`, and enqueues its initialisation on `st`.
// `staged`: session_layout's; `rows_ncom`: null, or the commitment count of the cells kind's row-indexed form.  The caller has set the device.
// `from_blobs`: the blob form of the row-indexed session (rows_ncom = its blobs, n = 128 of them each).
static int32_t session_acquire(const kzg_ctx* ctx, uint64_t n, hipStream_t st, VerifyKind kind, bool staged, kzg_verify_session** out,
                               const uint64_t* rows_ncom = nullptr, bool from_blobs = false) {
  *out = nullptr;
  const bool is_cells = kind == VerifyKind::CELLS;
  const bool rows = rows_ncom != nullptr;
  const uint64_t ncom = rows ? *rows_ncom : n, np = n + ncom;
  if (is_cells) {  // lincomb B's fixed terms, copied in below: derived by this member's first cells session
    const int32_t rc = ensure_g1_monomial(ctx);
    if (rc) return rc;
  }
  const uint64_t tail = facts(kind).tail_terms;
  const SessionLayout L = session_layout(ctx, n, kind, staged, rows, ncom, from_blobs);
  kzg_verify_session* s = nullptr;
  {
    std::lock_guard<std::mutex> guard(ctx->pool_lock);
    auto& pool = ctx->session_pool;
    int best = -1;
    for (int k = 0; k < (int)pool.size(); k++) {  // smallest pooled session that is large enough, else the largest (it is regrown)
      const bool fits = pool[k]->cap >= L.total;
      if (best < 0) best = k;
      else {
        const bool best_fits = pool[best]->cap >= L.total;
        if (fits && (!best_fits || pool[k]->cap < pool[best]->cap)) best = k;
        if (!fits && !best_fits && pool[k]->cap > pool[best]->cap) best = k;
      }
    }
    if (best >= 0) {
      s = pool[best];
      pool.erase(pool.begin() + best);
    }
  }
  if (!s) {
    s = new (std::nothrow) kzg_verify_session();
    if (!s) return fail(KZG_FAIL_ARGUMENT, "out of host memory");
    s->ctx = ctx;
    ctx->sessions_created.fetch_add(1, std::memory_order_relaxed);
    // the side stream carries the point decoder (long per-lane chains) next to the evaluation kernel's flood of short waves:
    // highest queue priority, so that its workgroups are placed first when both kernels become runnable
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithPriority(&s->side, hipStreamNonBlocking, prio_greatest) != hipSuccess ||
        hipStreamCreateWithFlags(&s->aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_nodes, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_stat, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_aux, hipEventDisableTiming) != hipSuccess) {
      session_free(s);
      return fail(KZG_FAIL_HIP, "verify session: stream/event creation failed");
    }
  }
  if (s->cap < L.total) {
    if (s->buf) (void)hipFree(s->buf);
    s->buf = nullptr;
    s->cap = 0;
    const size_t want = L.total + L.total / 8;
    if (hipMalloc(&s->buf, want) != hipSuccess) {
      session_free(s);
      return fail(KZG_FAIL_HIP, "hipMalloc(verify session) failed");
    }
    s->cap = want;
  }
  {
    const size_t hneed = 4 * sizeof(unsigned long long) + (3 * n + 1) * sizeof(int32_t) + ((n + 255) / 256 + 1) * 32;
    if (s->h_cap < hneed) {
      if (s->h_stat) (void)hipHostFree(s->h_stat);
      s->h_stat = nullptr;
      s->h_cap = 0;
      void* hp = nullptr;
      if (hipHostMalloc(&hp, hneed + hneed / 8, hipHostMallocDefault) != hipSuccess) {
        session_free(s);
        return fail(KZG_FAIL_HIP, "hipHostMalloc(verify session) failed");
      }
      s->h_stat = reinterpret_cast<int32_t*>(hp);
      s->h_cap = hneed + hneed / 8;
    }
    s->h_nodes = reinterpret_cast<uint32_t*>(s->h_stat + (3 * n + 1));
    s->h_first4 = reinterpret_cast<unsigned long long*>(reinterpret_cast<uint8_t*>(s->h_stat) + align_up((3 * n + 1) * sizeof(int32_t) + ((n + 255) / 256) * 32, 8));
  }
  if (st == KZG_SESSION_STREAM) st = s->side;
  s->n = n;
  s->ncom = ncom;
  s->rows = rows;
  s->stride = std::max(n, ncom);
  s->st = st;
  s->kind = kind;
  s->tail = tail;
  s->d_cells = nullptr;
  s->d_cell_indices = nullptr;
  s->d_com_indices = nullptr;
  s->from_blobs = from_blobs;
  s->d_blobs = nullptr;
  s->tree_n = 0;
  s->aff = (uint4*)(s->buf + L.o_aff);
  s->inf = s->buf + L.o_inf;
  s->z = (fr_t*)(s->buf + L.o_z);
  s->y = (fr_t*)(s->buf + L.o_y);
  s->scal = (fr_t*)(s->buf + L.o_scal);
  s->glv = use_glv(ctx, n, rows);
  s->glv_b = (fr_t*)(s->buf + L.o_glv_b);
  s->glv_a = (fr_t*)(s->buf + L.o_glv_a);
  s->stat = (int32_t*)(s->buf + L.o_stat);
  s->first4 = (unsigned long long*)(s->buf + L.o_first4);
  s->leaves = (uint32_t*)(s->buf + L.o_leaves);
  s->mids = (uint32_t*)(s->buf + L.o_mids);
  s->nodes = (uint32_t*)(s->buf + L.o_nodes);
  s->pts48 = s->buf + L.o_pts;
  s->zy32 = s->buf + L.o_zy;
  s->msm_a = s->buf + L.o_msm_a;
  s->msm_b = s->buf + L.o_msm_b;
  s->rpow2 = (fr_t*)(s->buf + L.o_rpow);
  s->ysum = (fr_t*)(s->buf + L.o_ysum);
  s->cell_part = (fr_t*)(s->buf + L.o_cell_part);
  s->cells_in = s->buf + L.o_cells_in;
  s->rpow = (fr_t*)(s->buf + L.o_rpow_n);
  s->roww_part = (fr_t*)(s->buf + L.o_roww);
  s->ext = s->buf + L.o_ext;
  s->blob_stat = (int32_t*)(s->buf + L.o_blob_stat);
  s->blob_code = (int32_t*)(s->buf + L.o_blob_code);
  // generator term (cells: the monomial terms), cleared flags and statuses
  const uint4* fixed = is_cells ? ctx->d_g1_monomial : ctx->d_gen_affine;  // `tail` points, their [z^2]-images behind them
  if (hipMemcpyAsync(s->aff + np * 6, fixed, tail * 96, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      (s->glv && hipMemcpyAsync(s->aff + ((np + tail) + np) * 6, fixed + tail * 6, tail * 96, hipMemcpyDeviceToDevice, st) != hipSuccess) ||  // [z^2]G
      hipMemsetAsync(s->inf, 0, np + tail, st) != hipSuccess || hipMemsetAsync(s->stat, 0, 4 * s->stride * 4 + 4, st) != hipSuccess) {
    kzg_verify_session_destroy(s);
    return fail(KZG_FAIL_HIP, "verify session init failed");
  }
  *out = s;
  return 0;
}

// A blob call of ONE item takes its lincombs and pairing on the host (verify_one_tail) unless a test forces it through the batch
// machinery: the entry points and the host-buffer front skip the transcript for it.
static bool one_item_on_host(const kzg_verify_session* s) { return s->n == 1 && !s->ctx->knobs.single_via_batch; }

// The point decoder beside the caller's stream.  `side` -- the session's side stream, or the caller's own under verify_serial -- waits
// for what the caller's stream holds at the fork (ev_fork: session initialised, inputs resident) and decodes points
// [first, first + count) of the n + ncom: proofs, then commitments.  `how`:
//   DECODE_FORKED  the caller recorded ev_fork itself, earlier on its stream (phase1_items: ahead of the hash)
//   DECODE_WHOLE   all 2n points with the one-launch decoder (k_g1_decompress) instead of a range
//   DECODE_FINISH  nothing is decoded after this: the [z^2]-images under GLV right behind the decoder (one product per point), then ev_join
enum : unsigned { DECODE_FORKED = 1u, DECODE_WHOLE = 2u, DECODE_FINISH = 4u };
static void decode_on_side(kzg_verify_session* s, hipStream_t side, uint64_t first, uint64_t count, const uint8_t* prf, const uint8_t* com, unsigned how) {
  const uint64_t n = s->n, nc = s->ncom, np = n + nc;
  int32_t *stat_prf = s->stat + 2 * s->stride, *stat_com = s->stat + s->stride;  // slots 2 and 1 in every kind (verify_kind.hpp)
  if (!(how & DECODE_FORKED)) (void)hipEventRecord(s->ev_fork, s->st);
  (void)hipStreamWaitEvent(side, s->ev_fork, 0);
  {
    ProfScope ps(s->ctx, PROF_DECODE, side);
    if (how & DECODE_WHOLE)
      launch_g1_decompress(side, prf, n, stat_prf, com, nc, stat_com, s->aff, s->inf);
    else
      launch_g1_decompress_range(side, first, count, prf, n, stat_prf, com, nc, stat_com, s->aff, s->inf);
  }
  if (!(how & DECODE_FINISH)) return;
  if (s->glv) hipLaunchKernelGGL(k_glv_points, dim3(blocks_for(np, 64)), dim3(64), 0, side, s->aff, np, np + s->tail);
  (void)hipEventRecord(s->ev_join, side);
}

// Per-item device work of items [base, base + m): Fiat-Shamir challenge z_i and evaluation y_i from blobs resident at
// `blobs` (m blobs), enqueued on `st`.  `decode_here`: the commitments/proofs of the SAME range are decoded too (fused
// launch for small m, the session's side stream otherwise); the caller joins ev_join.
static int32_t phase1_items(kzg_verify_session* s, const uint8_t* blobs, const uint8_t* com, const uint8_t* prf, uint64_t base, uint64_t m,
                            hipStream_t st, bool decode_here) {
  const kzg_ctx* ctx = s->ctx;
  const uint64_t n = s->n;
  if (m == 0) return 0;
  fr_t* z = s->z + base;
  fr_t* y = s->y + base;
  int32_t* stat_blob = stat_of(s, kzg::verify::BLOBS_BLOB) + base;
  // SHA-256 challenge first, alone: its long-lived waves (one per SIMD at n = 65,536) must be spread evenly -- launched
  // next to the decode kernel they were placed around its waves and the kernel took 3x longer (profiles/r01: 23 ms vs
  // 7.5 ms).  The point decoding then runs on the side stream concurrently with the evaluation kernel, whose short blocks
  // rebalance dynamically.  Small batches (everything together below one wave per SIMD) are latency-bound instead:
  // there hashing and decoding are ONE launch whose workgroups the dispatcher deals over different CUs.
  if (decode_here && base == 0 && m == n && fused_prep_fits(ctx, m, 2 * n)) {
    launch_challenge_and_decode(ctx, st, blobs, com, m, z, prf, n, s->stat + 2 * n, com, n, s->stat + n, s->aff, s->inf);
    (void)hipEventRecord(s->ev_join, st);
  } else {
    // The latency hash kernels claim more than half a register file per wave, so nothing shares THEIR SIMDs and the dispatcher
    // cannot pack them (left alone it put several workgroups on one CU: 4.7 ms instead of 3.7 ms per hash at 16,384 blobs,
    // 5.9 instead of 4.0 ms at 32,768).  The SIMDs they leave free -- a quarter of the chip at 16,384 blobs -- take decode waves,
    // two each: while the hash leaves SIMDs free the decode kernel is released as soon as the hash is enqueued and runs beside
    // it; when the hash fills the chip (from ~30,700 blobs on, and always with the one-lane hash) it waits for the hash and runs
    // beside the evaluation kernel.  (Decoding beside the full-chip hash with traded issue priority was measured and lost:
    // 19.2-20.5 instead of 18.1 ms per 65,536 triples, profiles/r03/verify_cohash_traded_priority_rejected.json.)
    const uint64_t hash_wgs = blocks_for(m, 64);
    const uint64_t split_max = ctx->knobs.challenge_split_max ? ctx->knobs.challenge_split_max : (uint64_t)ctx->num_cus * 128;
    // lane-pair kernel (four waves per 64 blobs), producer/consumer pairs (two), one lane per blob (one wave, 292 VGPRs)
    const uint64_t hash_waves = hash_wgs <= ctx->num_cus ? 4 * hash_wgs : (m <= split_max ? 2 * hash_wgs : hash_wgs);
    const uint64_t simds = (uint64_t)ctx->num_cus * 4;
    uint64_t beside = 0;  // points decoded beside the hash
    if (decode_here && !ctx->knobs.verify_serial && !ctx->knobs.challenge_split_max && hash_waves + 64 <= simds)
      beside = 2 * n;  // all of them: what does not fit beside the hash is at least queued AHEAD of the evaluation kernel's waves
                       // (measured, ms per call at 24,000 / 28,000 / 30,000 / 32,768 triples: only what fits 10.5 / 11.4 / 11.9 / 10.9,
                       // everything 9.0 / 10.0 / 10.6 / 11.6 -- so not when the hash fills the chip)
    hipStream_t side = ctx->knobs.verify_serial ? st : s->side;
    if (beside) (void)hipEventRecord(s->ev_fork, st);  // the inputs are ready here
    launch_challenge(ctx, st, blobs, com + base * 48, m, z);  // enqueued first: its workgroups must find their SIMDs empty
    if (beside) decode_on_side(s, side, 0, beside, prf, com, DECODE_FORKED | (beside == 2 * n ? DECODE_FINISH : 0u));
    if (decode_here && beside < 2 * n)  // the rest behind the hash (ev_fork re-recorded: the first wait is already enqueued)
      decode_on_side(s, side, beside, 2 * n - beside, prf, com, DECODE_FINISH);
  }
  bool wide_groups = m < 4096;
  if (ctx->knobs.eval_group) wide_groups = ctx->knobs.eval_group != 16;  // tests force either shape
  {
    ProfScope ps(ctx, PROF_EVAL, st);
    if (!wide_groups)  // chip full: 16 lanes per blob (four blobs per wave), shorter merge tree
      hipLaunchKernelGGL(k_eval_frac<16>, dim3(blocks_for(m, 4)), dim3(64), 0, st, blobs, z, ctx->d_roots_brp, ctx->d_eval_tab, y, stat_blob, m);
    else  // latency first: the whole wave on one blob
      hipLaunchKernelGGL(k_eval_frac<64>, dim3((unsigned)m), dim3(64), 0, st, blobs, z, ctx->d_roots_brp, ctx->d_eval_tab, y, stat_blob, m);
  }
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "verify phase 1 launch failed");
  return 0;
}

// The transcript's upper levels behind a kind's leaf kernel on the caller's stream: 16 leaves per mid digest, 16 mid digests per node,
// and the read-back of the node digests, done at ev_nodes.  Also the launch check of the leaf kernel before it.
static int32_t p1_transcript_nodes(kzg_verify_session* s) {
  const uint64_t n = s->n, nmid = (n + 15) / 16, groups = (n + 255) / 256;  // groups == ceil(nmid / 16)
  hipStream_t st = s->st;
  hipLaunchKernelGGL(k_transcript_nodes, dim3(blocks_for(nmid, 64)), dim3(64), 0, st, s->leaves, n, 16u, s->mids);
  hipLaunchKernelGGL(k_transcript_nodes, dim3(blocks_for(groups, 64)), dim3(64), 0, st, s->mids, nmid, 16u, s->nodes);
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "verify phase 1 launch failed");
  if (hipMemcpyAsync(s->h_nodes, s->nodes, groups * 32, hipMemcpyDeviceToHost, st) != hipSuccess || hipEventRecord(s->ev_nodes, st) != hipSuccess)
    return fail(KZG_FAIL_HIP, "verify phase 1 readback failed");
  return 0;
}
// ---- phase 1 in three pieces (the fused single-context call interleaves them with phase 2's, see verify_fused) -------------
// (a) transcript over all n items -- it hashes the input BYTES and (z, y): it does not wait for the decoded points -- and the
//     read-back of its node digests, enqueued on `st`
static int32_t p1_transcript(kzg_verify_session* s, const uint8_t* com, const uint8_t* prf) {
  hipLaunchKernelGGL(k_transcript_leaves, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->st, com, prf, s->z, s->y, s->n, s->leaves);
  return p1_transcript_nodes(s);
}
// (b) local transcript root = SHA-256 over the node digests (big-endian bytes); waits for (a) only -- the decoder may still run
static int32_t p1_root(kzg_verify_session* s, uint8_t* out_root32) {
  if (hipEventSynchronize(s->ev_nodes) != hipSuccess) return fail(KZG_FAIL_HIP, "verify phase 1 synchronize failed");
  const uint64_t groups = (s->n + 255) / 256;
  std::vector<uint8_t> nb(groups * 32);
  for (uint64_t k = 0; k < groups * 8; k++) store_be32(nb.data() + 4 * k, s->h_nodes[k]);
  sha256_bytes(out_root32, nb.data(), nb.size());
  return 0;
}
// ---- the kinds of call (verify_kind.hpp): what differs between them is the front and how the error record is read ----
// the device copies of a host-buffer call in its session: proofs || commitments, z || y, cells || indices (the blobs pass through the
// staging arena)
static VerifyInputs staged_inputs(const kzg_verify_session* s) {
  const uint64_t n = s->n;
  switch (s->kind) {
    case VerifyKind::BLOBS: return blob_inputs(nullptr, s->pts48 + n * 48, s->pts48, false);
    case VerifyKind::POINTS: return point_inputs(s->pts48, s->pts48 + n * 48, s->zy32, s->zy32 + n * 32, false);
    case VerifyKind::CELLS: break;
  }
  if (s->from_blobs) return blob_cell_inputs(s->cells_in, s->ncom, s->pts48 + n * 48, s->pts48, false);
  const uint8_t* idx = s->cells_in + n * (size_t)KZG_BYTES_PER_CELL;
  if (s->rows) return cell_rows_inputs(s->pts48 + n * 48, s->ncom, idx + n * 8, idx, s->cells_in, s->pts48, false);
  return cell_inputs(s->pts48 + n * 48, idx, s->cells_in, s->pts48, false);
}
static void err_clear(int32_t* err, int kinds) {
  for (int k = 0; k < 2 * kinds; k++) err[k] = (k % 2 == 0) ? -1 : 0;
}
// first-error-wins in the reference's parse order (src/kzg/setup.rs:259-271; :103-109 lifted to arrays the same way): the first kind with an entry
static int32_t first_error_code(const int32_t* err, int kinds) {
  for (int k = 0; k < 2 * kinds; k += 2)
    if (err[k] >= 0) return err[k + 1];
  return 0;
}
// The code of a session's error record.  The blob form reads the cells kind's record {index, commitment, cell, proof} in ITS order: the
// cell entry is the blob's (the front writes the extension kernel's status to all 128 items of a blob, so its lowest position is the
// lowest rejected blob), and every blob comes before any commitment, every commitment before any proof; the index entry is never set.
static int32_t session_error_code(const kzg_verify_session* s, const int32_t* err) {
  if (!s->from_blobs) return first_error_code(err, facts(s->kind).entries);
  for (int k : {(int)kzg::verify::CELLS_CELL, 1, 3})
    if (err[2 * k] >= 0) return err[2 * k + 1];
  return 0;
}
// Everything of phase 1 that can be enqueued at once.  When this returns z, y and the statuses are being produced, the decoder's
// end is ev_join and the transcript's node digests are on their way back behind ev_nodes (p1_root).
//   BLOBS:  hash, [decoder] || evaluation, transcript (phase1_items, p1_transcript)
//   CELLS:  as POINTS, with k_cells_leaves (cellverify_kernels.cuh) in k_points_leaves' place
//   POINTS: neither hash nor evaluation: [decoder for all 2n points on the side stream] || k_points_leaves (parses z and y and writes
//           their statuses) -> k_transcript_nodes x 2.  The statuses never cross to the host (front_status).
// `in`: device-resident inputs of the session's kind.
static int32_t front_enqueue(kzg_verify_session* s, const VerifyInputs& in) {
  const kzg_ctx* ctx = s->ctx;
  const uint64_t n = s->n;
  hipStream_t st = s->st;
  const uint8_t *com = in.commitments48, *prf = in.proofs48;
  switch (s->kind) {
    case VerifyKind::BLOBS: {
      const int32_t rc = phase1_items(s, in.blobs, com, prf, 0, n, st, true);
      return rc ? rc : p1_transcript(s, com, prf);
    }
    case VerifyKind::POINTS:
    case VerifyKind::CELLS: {
      // CELLS: the points call's launch order with k_cells_leaves as the front kernel: it parses the index and the cell, writes
      // z = h^64 and y = 0, and hashes the 34-block leaf; the cells are read again in phase 2
      s->d_cells = in.cells;
      s->d_cell_indices = in.cell_indices;
      s->d_com_indices = in.commitment_indices;
      // the decoder is ONE launch over proofs and commitments: no event after the proof half for lincomb A to wait on instead of ev_join
      decode_on_side(s, s->side, 0, n + s->ncom, prf, com, DECODE_FINISH | (fused_prep_fits(ctx, n, n + s->ncom) ? DECODE_WHOLE : 0u));
      if (hipMemsetAsync(s->first4, 0xff, 4 * sizeof(unsigned long long), s->side) != hipSuccess)  // for k_first_errors, later on this stream
        return fail(KZG_FAIL_HIP, "verify_proof_batch: fork failed");
      if (s->from_blobs) {  // the blob form: the extension half into the session, then the front over implicit indices
        s->d_blobs = in.blobs;
        const int32_t rc = cells_ext_enqueue(ctx, in.blobs, s->ncom, s->ext, s->blob_stat, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_blob_cells_leaves, dim3(blocks_for(n, 256)), dim3(256), 0, st, com, in.blobs, s->ext, s->blob_stat, prf, n, ctx->d_cellv_h64, s->z, s->y,
                           stat_of(s, kzg::verify::CELLS_INDEX), stat_of(s, kzg::verify::CELLS_CELL), s->leaves);
      } else if (s->rows)  // the row-indexed form: the commitment through the item's index, the index's status with the cell index's
        hipLaunchKernelGGL(k_cells_rows_leaves, dim3(blocks_for(n, 256)), dim3(256), 0, st, com, reinterpret_cast<const unsigned long long*>(in.commitment_indices),
                           s->ncom, reinterpret_cast<const unsigned long long*>(in.cell_indices), in.cells, prf, n, ctx->d_cellv_h64, s->z, s->y,
                           stat_of(s, kzg::verify::CELLS_INDEX), stat_of(s, kzg::verify::CELLS_CELL), s->leaves);
      else if (s->kind == VerifyKind::CELLS)
        hipLaunchKernelGGL(k_cells_leaves, dim3(blocks_for(n, 256)), dim3(256), 0, st, com, reinterpret_cast<const unsigned long long*>(in.cell_indices), in.cells, prf, n,
                           ctx->d_cellv_h64, s->z, s->y, stat_of(s, kzg::verify::CELLS_INDEX), stat_of(s, kzg::verify::CELLS_CELL), s->leaves);
      else
        hipLaunchKernelGGL(k_points_leaves, dim3(blocks_for(n, 256)), dim3(256), 0, st, com, prf, in.z32, in.y32, n, s->z, s->y, stat_of(s, kzg::verify::POINTS_Z),
                           stat_of(s, kzg::verify::POINTS_Y), s->leaves);
      return p1_transcript_nodes(s);
    }
  }
  return fail(KZG_FAIL_ARGUMENT, "unknown kind of verification call");
}
// The first rejected item of each entry of the error record -> err = entries x {local index, code}.  Both ride on the DECODER's stream, right behind the
// decoder, not on the caller's: there they would queue up behind the bucket kernels of phase 2.
//   BLOBS:  3n status words come back and the host scans them beside the bucket kernels (the blob statuses were written by the
//           evaluation kernel, which ended before the root was read)
//   POINTS, CELLS: k_first_errors (it also waits for k_points_leaves' two status arrays: ev_nodes was recorded after it) and 32 bytes come back
static int32_t front_status(kzg_verify_session* s, int32_t* err) {
  const uint64_t n = s->n;
  hipStream_t side = s->side;
  switch (s->kind) {
    case VerifyKind::BLOBS:
      if (hipStreamWaitEvent(side, s->ev_join, 0) != hipSuccess || hipMemcpyAsync(s->h_stat, s->stat, 3 * n * 4, hipMemcpyDeviceToHost, side) != hipSuccess ||
          hipEventRecord(s->ev_stat, side) != hipSuccess || hipEventSynchronize(s->ev_stat) != hipSuccess)
        return fail(KZG_FAIL_HIP, "verify phase 1 status readback failed");
      for (int k = 0; k < 3; k++) scan_first_error(s->h_stat + (uint64_t)facts(s->kind).slot[k] * n, n, &err[2 * k], &err[2 * k + 1]);
      return 0;
    case VerifyKind::POINTS:
    case VerifyKind::CELLS:
      if (hipStreamWaitEvent(side, s->ev_nodes, 0) != hipSuccess) return fail(KZG_FAIL_HIP, "verify_proof_batch: status wait failed");
      // over the arrays' stride: the row-indexed form's commitment statuses are ncom words, which may be more than n (the rest is clear)
      hipLaunchKernelGGL(k_first_errors, dim3(blocks_for(s->stride, 256)), dim3(256), 0, side, stat_of(s, 0), stat_of(s, 1), stat_of(s, 2), stat_of(s, 3), s->stride,
                         s->first4);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(s->h_first4, s->first4, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, side) != hipSuccess ||
          hipEventRecord(s->ev_stat, side) != hipSuccess || hipEventSynchronize(s->ev_stat) != hipSuccess)
        return fail(KZG_FAIL_HIP, "verify_proof_batch: status readback failed");
      for (int k = 0; k < 4; k++) {
        const unsigned long long w = s->h_first4[k];
        err[2 * k] = w == ~0ull ? -1 : (int32_t)(w >> 32);
        err[2 * k + 1] = w == ~0ull ? 0 : (int32_t)(uint32_t)w;
      }
      return 0;
  }
  return fail(KZG_FAIL_ARGUMENT, "unknown kind of verification call");
}
// the body of the two kzg_verify_*phase1_dev entry points
static int32_t phase1_entry(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, hipStream_t st, uint8_t* out_root32, int32_t* err, kzg_verify_session** session) {
  if (!ctx || !out_root32 || !err || !session || (n && in.any_null())) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return verify_phase1(ctx, in, n, st, out_root32, err, session);
}
extern "C" int32_t kzg_verify_phase1_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_proofs48,
                                         uint64_t n, uint8_t* out_root32, int32_t* err6, kzg_verify_session** session, void* hip_stream) try {
  return phase1_entry(ctx, blob_inputs(d_blobs, d_commitments48, d_proofs48, false), n, (hipStream_t)hip_stream, out_root32, err6, session);
} catch (...) {
  return abi_exception();
}

// Host-buffer phase 1: the blobs cross PCIe in chunks through the context's staging arena (slots of `chunk` blobs) on the
// copy stream while the per-blob kernels (challenge + evaluation are per blob) of earlier chunks run on rotating compute
// streams -- the n * 128 KiB never have to be resident at once and the transfer overlaps the hashing.  Commitments and
// proofs (96 B per item) are copied whole and decoded once on the session's side stream.
static int32_t verify_phase1_host(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* proofs48, uint64_t n,
                                  uint8_t* out_root32, int32_t* err6, kzg_verify_session** session) {
  *session = nullptr;
  TraceTimer tt(ctx->knobs.trace, "phase1(host buffers)");
  if (err6) err_clear(err6, 3);
  std::lock_guard<std::mutex> guard(ctx->stage_lock);  // the arena and the copy/compute streams below are shared
  // Chunk size: the SHA-256 kernel of a chunk is latency-bound (~3.7 ms whether it hashes 512 or 16,384 blobs), so chunks
  // are LARGE -- a quarter of the batch, between 512 and 4,096 blobs (512 MiB, ~9 ms of PCIe) -- and the copy of chunk k+1
  // hides the hash + evaluation of chunk k (measured with 512-blob chunks on four streams: 63 ms per 16,384 blobs, the
  // hashes of 32 chunks queue up four at a time; profiles/r02/hostapi_*.json).
  uint64_t chunk = ctx->knobs.verify_chunk;
  if (!chunk) {
    chunk = (n + 3) / 4;
    chunk = (chunk + 63) / 64 * 64;
    chunk = chunk < 512 ? 512 : (chunk > 4096 ? 4096 : chunk);
  }
  const uint64_t nchunks = (n + chunk - 1) / chunk;
  // Compute streams the chunks rotate over: TWO.  With a hardware queue per stream (GPU_MAX_HW_QUEUES >= 8) four independent
  // chunk streams put four chunks' hash and evaluation kernels on the chip at once and the LAST chunk's latency-bound hash --
  // the call's critical path: it cannot start before its copy ends -- shares SIMDs with its predecessors' waves: 16.5 instead of
  // 15.0 ms per 4,096 triples (two or three streams: 15.0; one: 18.9; at 16,384 triples all the same, 44.2).  Round 3's four
  // streams only did well because the runtime's default of four hardware queues folded them onto fewer.
  const uint64_t nstreams = ctx->knobs.verify_streams ? ctx->knobs.verify_streams : 2;
  StageRing ring;
  int32_t rc = ring.open(ctx, nchunks < KZG_STAGE_SLOTS ? nchunks : KZG_STAGE_SLOTS, (size_t)chunk * KZG_BYTES_PER_BLOB, 0, nchunks > 1);
  if (rc) return rc;
  hipStream_t st = ctx->verify_stream;
  SessionUse use;  // declared behind the lock: a failed call's session is drained and pooled before the arena is handed on
  rc = session_acquire(ctx, n, st, VerifyKind::BLOBS, false, &use.s);
  if (rc) return rc;
  kzg_verify_session* s = use.s;
  do {
    uint8_t* prf = s->pts48;
    uint8_t* com = s->pts48 + n * 48;
    uint8_t* d_chunk = nullptr;
    if (hipMemcpyAsync(prf, proofs48, n * 48, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(com, commitments48, n * 48, hipMemcpyHostToDevice, st) != hipSuccess) {
      rc = fail(KZG_FAIL_HIP, "host-to-device copy failed");
      break;
    }
    if (nchunks == 1) {
      // a single chunk (small batches, single items): nothing to overlap -- one copy on the session's stream, then the device path's
      // launches (hash and point decoding fused in one launch: the latency-optimal shape)
      rc = ring.feed(0, blobs, n * (size_t)KZG_BYTES_PER_BLOB, st, &d_chunk);
      if (rc == 0) rc = phase1_items(s, d_chunk, com, prf, 0, n, st, true);
    } else {
      // all points decoded once, beside the chunk pipeline
      decode_on_side(s, s->side, 0, 2 * n, prf, com, DECODE_WHOLE | DECODE_FINISH);
      // session initialised, points resident: decode_on_side has recorded ev_fork (all stage streams wait: the join below is over all)
      for (int r = 0; r < KZG_STAGE_STREAMS && rc == 0; r++)
        if (hipStreamWaitEvent(ctx->stage_streams[r], s->ev_fork, 0) != hipSuccess) rc = fail(KZG_FAIL_HIP, "stream wait failed");
      for (uint64_t k = 0; k < nchunks && rc == 0; k++) {
        const uint64_t base = k * chunk;
        const uint64_t m = (n - base < chunk) ? (n - base) : chunk;
        hipStream_t comp = ctx->stage_streams[k % nstreams];
        rc = ring.feed(k, blobs + base * (size_t)KZG_BYTES_PER_BLOB, m * (size_t)KZG_BYTES_PER_BLOB, comp, &d_chunk);
        if (rc == 0) rc = phase1_items(s, d_chunk, com, prf, base, m, comp, false);
        if (rc == 0) rc = ring.consumed(k, comp);
      }
      // join the compute streams into the session's stream
      for (int r = 0; r < KZG_STAGE_STREAMS && rc == 0; r++) rc = stream_after(st, ctx->stage_streams[r], ctx->stage_join[r]);
    }
    if (rc) break;
    tt.mark("enqueue copies + per-chunk kernels");
    // err6 == null (the fused single-context call): only the transcript and its root here -- once the root is known every blob
    // has been hashed and evaluated, so the staging arena can be handed on; the statuses are read by the caller, later
    if (!err6 && one_item_on_host(s)) {
      // one item: no batch challenge (r^0 = 1), hence no transcript; the arena is free once the item's kernels have run
      memset(out_root32, 0, 32);
      if (hipStreamSynchronize(st) != hipSuccess) rc = fail(KZG_FAIL_HIP, "verify phase 1 synchronize failed");
      break;
    }
    rc = p1_transcript(s, com, prf);
    if (rc == 0) rc = p1_root(s, out_root32);
    if (rc == 0 && err6) rc = front_status(s, err6);
    tt.mark("gpu kernels + readback + root hash (+ status scan)");
  } while (0);
  if (rc) {
    stage_drain(ctx);  // the chunk kernels on the arena's own streams, which no session drains
    return rc;
  }
  *session = use.release();
  return 0;
}

// Host cells (CELLS): 2,152 bytes per tuple the same way, the cells and indices into the session's cells_in.
// Host points: 160 bytes per tuple cross PCIe whole into the session's own staging (proofs || commitments, z || y) on the
// context's verification stream; nothing of the blob calls' staging arena is used, so stage_lock is held for stage_init only.
static int32_t points_stage_host(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, kzg_verify_session** out) {
  *out = nullptr;
  {
    std::lock_guard<std::mutex> guard(ctx->stage_lock);
    const int32_t rc = stage_init(ctx);
    if (rc) return rc;
  }
  SessionUse use;
  const bool is_cells = in.kind == VerifyKind::CELLS;
  const int32_t rc = session_acquire(ctx, n, ctx->verify_stream, in.kind, true, &use.s, in.rows() ? &in.ncom : nullptr, in.from_blobs);
  if (rc) return rc;
  kzg_verify_session* s = use.s;
  if (hipMemcpyAsync(s->pts48, in.proofs48, n * 48, hipMemcpyHostToDevice, s->st) != hipSuccess ||
      hipMemcpyAsync(s->pts48 + n * 48, in.commitments48, s->ncom * 48, hipMemcpyHostToDevice, s->st) != hipSuccess)
    return fail(KZG_FAIL_HIP, "host-to-device copy failed");
  if (s->from_blobs) {  // the blobs, commitments and proofs are all that crosses: 128 KiB + 48 B + 6 KiB per blob
    if (hipMemcpyAsync(s->cells_in, in.blobs, s->ncom * (size_t)KZG_BYTES_PER_BLOB, hipMemcpyHostToDevice, s->st) != hipSuccess)
      return fail(KZG_FAIL_HIP, "host-to-device copy failed");
    *out = use.release();
    return 0;
  }
  if (s->rows && hipMemcpyAsync(s->cells_in + n * ((size_t)KZG_BYTES_PER_CELL + 8), in.commitment_indices, n * 8, hipMemcpyHostToDevice, s->st) != hipSuccess)
    return fail(KZG_FAIL_HIP, "host-to-device copy failed");
  if (is_cells ? (hipMemcpyAsync(s->cells_in, in.cells, n * (size_t)KZG_BYTES_PER_CELL, hipMemcpyHostToDevice, s->st) != hipSuccess ||
               hipMemcpyAsync(s->cells_in + n * (size_t)KZG_BYTES_PER_CELL, in.cell_indices, n * 8, hipMemcpyHostToDevice, s->st) != hipSuccess)
            : (hipMemcpyAsync(s->zy32, in.z32, n * 32, hipMemcpyHostToDevice, s->st) != hipSuccess ||
               hipMemcpyAsync(s->zy32 + n * 32, in.y32, n * 32, hipMemcpyHostToDevice, s->st) != hipSuccess))
    return fail(KZG_FAIL_HIP, "host-to-device copy failed");
  *out = use.release();
  return 0;
}

// Phase 1 on its own, behind kzg_verify_*phase1_dev and the host-buffer shares of a group: a session with device-resident inputs comes
// to be, the front runs to its root and error record, and the session becomes the caller's.  n = 0: the empty transcript's root.
int32_t verify_phase1(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, hipStream_t st, uint8_t* out_root32, int32_t* err, kzg_verify_session** session) {
  *session = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  if (in.on_host && in.kind == VerifyKind::BLOBS)  // through the staging arena: front and root while stage_lock is held
    return verify_phase1_host(ctx, in.blobs, in.commitments48, in.proofs48, n, out_root32, err, session);
  TraceTimer tt(ctx->knobs.trace, "phase1");
  err_clear(err, facts(in.kind).entries);
  SessionUse use;
  int32_t rc = in.on_host ? points_stage_host(ctx, in, n, &use.s) : session_acquire(ctx, n, st, in.kind, false, &use.s, in.rows() ? &in.ncom : nullptr, in.from_blobs);
  if (rc) return rc;
  kzg_verify_session* s = use.s;
  tt.mark("session");
  if (n) {
    rc = front_enqueue(s, in.on_host ? staged_inputs(s) : in);
    if (rc == 0) rc = p1_root(s, out_root32);
    if (rc == 0) rc = front_status(s, err);
    tt.mark("gpu kernels + readback + first errors + root hash");
  } else {
    sha256_bytes(out_root32, nullptr, 0);
    if (hipStreamSynchronize(s->st) != hipSuccess) rc = fail(KZG_FAIL_HIP, "verify phase 1 synchronize failed");
  }
  if (rc) return rc;
  *session = use.release();
  return 0;
}

// P1::decompress for n points (src/bls.rs:505-531): the decoder of the verification path with its result in the 2^384-
// Montgomery domain, as blst_p1_affine images
__global__ __launch_bounds__(64) void k_g1_decompress_public(const uint8_t* __restrict__ in48, uint64_t n, uint8_t* __restrict__ out_affine96,
                                                             int32_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t buf[48];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(in48 + i * 48);
#pragma unroll
  for (int q = 0; q < 12; q++) {
    const uint32_t w = src[q];
    buf[4 * q] = (uint8_t)w;
    buf[4 * q + 1] = (uint8_t)(w >> 8);
    buf[4 * q + 2] = (uint8_t)(w >> 16);
    buf[4 * q + 3] = (uint8_t)(w >> 24);
  }
  fp_t x, y;
  bool is_inf = false;
  const int32_t st = g1_decompress28(x, y, is_inf, buf, false);
  status[i] = st;
  if (st != 0 || is_inf) {
    bn_zero(x);
    bn_zero(y);
  }
  uint32_t* o = reinterpret_cast<uint32_t*>(out_affine96 + i * 96);
#pragma unroll
  for (int q = 0; q < 12; q++) {
    o[q] = x.v[q];
    o[12 + q] = y.v[q];
  }
}

extern "C" int32_t kzg_g1_decompress_batch(const kzg_ctx* ctx, const uint8_t* in48, uint64_t n, uint8_t* out_affine96, int32_t* status) try {
  if (!ctx || (n && (!in48 || !out_affine96 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return on_members(ctx, n, [&](const kzg_ctx* m, uint64_t first, uint64_t count) {
    return g1_decompress_single(m, in48 + first * 48, count, out_affine96 + first * 96, status + first);
  });
} catch (...) {
  return abi_exception();
}
// pooled device buffers and an idle stream of the host-buffer pipelines; nothing crosses the staging arena
int32_t g1_decompress_single(const kzg_ctx* ctx, const uint8_t* in48, uint64_t n, uint8_t* out_affine96, int32_t* status) {
  if (n == 0) return 0;
  HostCall hc(ctx);
  const int a_in = hc.upload(in48, (size_t)n * 48), a_out = hc.download(out_affine96, (size_t)n * 96), a_st = hc.download(status, (size_t)n * sizeof(int32_t));
  int32_t rc = hc.open({}, 0);
  if (rc) return rc;
  {
    ProfScope ps(ctx, PROF_DECODE, hc.st);
    hipLaunchKernelGGL(k_g1_decompress_public, dim3(blocks_for(n, 64)), dim3(64), 0, hc.st, hc.dev(a_in), n, hc.dev(a_out), hc.dev<int32_t>(a_st));
  }
  if (hipGetLastError() != hipSuccess) rc = fail(KZG_FAIL_HIP, "point decoding: launch failed");
  return hc.close(rc);
}

// Polynomial::evaluate (src/kzg/poly.rs:10-33) for n (blob, z) pairs from host buffers, through the evaluation kernel of the
// verification path.  (In verify_blob_kzg_proof_batch z is a hash output; an evaluation point ON the domain -- poly.rs:14-18 --
// reaches k_eval_frac only through this entry point.)
extern "C" int32_t kzg_evaluate_blobs(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* z32, uint64_t n, uint8_t* out_y32, int32_t* status) try {
  if (!ctx || (n && (!blobs || !z32 || !out_y32 || !status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return on_members(ctx, n, [&](const kzg_ctx* m, uint64_t first, uint64_t count) {
    return evaluate_blobs_single(m, blobs + first * (size_t)KZG_BYTES_PER_BLOB, z32 + first * 32, count, out_y32 + first * 32, status + first);
  });
} catch (...) {
  return abi_exception();
}
// The blobs cross PCIe through the staging arena in chunks of up to 2,048 (two slots: the copy of chunk k+1 beside the
// evaluation of chunk k; the copy stream even for one chunk); only z, y and the statuses live in the small host-i/o pool, so a
// large call pins nothing.
int32_t evaluate_blobs_single(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* z32, uint64_t n, uint8_t* out_y32, int32_t* status) {
  if (n == 0) return 0;
  HostCall hc(ctx);
  const int a_z32 = hc.upload(z32, (size_t)n * 32), a_y32 = hc.download(out_y32, (size_t)n * 32), a_z = hc.scratch((size_t)n * sizeof(fr_t)),
            a_y = hc.scratch((size_t)n * sizeof(fr_t)), a_st = hc.download(status, (size_t)n * sizeof(int32_t));
  int32_t rc = hc.open(even_plan(n, 2048), KZG_BYTES_PER_BLOB, true);
  if (rc) return rc;
  fr_t *d_z = hc.dev<fr_t>(a_z), *d_y = hc.dev<fr_t>(a_y);
  int32_t* d_st = hc.dev<int32_t>(a_st);
  hipStream_t st = hc.st;
  if (hipMemsetAsync(d_st, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess) return hc.close(fail(KZG_FAIL_HIP, "memset failed"));
  launch_fr_parse(st, hc.dev(a_z32), n, d_z, d_st);
  bool wide_groups = n < 4096;
  if (ctx->knobs.eval_group) wide_groups = ctx->knobs.eval_group != 16;
  rc = hc.passes(blobs, KZG_BYTES_PER_BLOB, [&](size_t, uint64_t base, uint64_t m, uint8_t* d_blobs) {
    ProfScope ps(ctx, PROF_EVAL, st);
    if (!wide_groups)
      hipLaunchKernelGGL(k_eval_frac<16>, dim3(blocks_for(m, 4)), dim3(64), 0, st, d_blobs, d_z + base, ctx->d_roots_brp, ctx->d_eval_tab, d_y + base, d_st + base,
                         m);
    else
      hipLaunchKernelGGL(k_eval_frac<64>, dim3((unsigned)m), dim3(64), 0, st, d_blobs, d_z + base, ctx->d_roots_brp, ctx->d_eval_tab, d_y + base, d_st + base, m);
    return 0;
  });
  if (rc == 0) {
    launch_fr_store_be(st, d_y, n, d_st, hc.dev(a_y32));
    if (hipGetLastError() != hipSuccess) rc = fail(KZG_FAIL_HIP, "evaluation: launch failed");
  }
  return hc.close(rc);
}

// ---- ONE item: the lincombs on the host ---------------------------------------------------------------------------------
// verify_blob_proof / verify_proof (src/kzg/setup.rs:96-113, 208-221) are the batch check with n = 1, where r^0 = 1:
//     e(proof, [tau]_2) == e(commitment - [y]G + [z]proof, G2).
// Through the batch machinery that is a transcript, seven sorting / bucket / window kernels per lincomb for one and three
// terms, two read-backs and two Horner loops: 0.6 ms on a chip with nothing to do (profiles/r04/single_verify_kernel_timeline.txt).
// Here the two decoded points, z and y come back in one copy and the host -- which already runs the Horner loops and the pairing
// -- takes S = [z]proof - [y]G as ONE double-scalar multiplication (4-bit windows, shared doublings: 14 + 252 + <= 128 point
// operations, ~0.2 ms), B = S + commitment and its Miller loop on one thread while a second thread runs the proof's Miller loop.
// The point decoding itself (square root, subgroup check: the reference's P1::decompress decisions) stays on the device.
namespace {
using host::host_point_from_r392;
using host::host_double_scalar_mul;

// proof / commitment: 24 limbs each as the decoder left them (x || y, 2^392 domain); z, y plain
int32_t verify_one_on_host(const kzg_ctx* ctx, const uint32_t* prf24, bool prf_inf, const uint32_t* com24, bool com_inf, const fr_t& z, const fr_t& y,
                           int32_t* ok) {
  TraceTimer tt(ctx->knobs.trace, "one item: host lincomb + pairing");
  host::g1_host_affine P, C;
  host_point_from_r392(P, prf24, prf_inf);
  host_point_from_r392(C, com24, com_inf);
  host::fp12 fa = host::f12_one(), fb = host::f12_one();
  (void)run_on_helpers(2, [&](uint32_t k) -> int32_t {
    if (k == 1) {  // f_{|z|,[tau]_2}(-proof)
      host::g1_host_affine np = P;
      if (!np.inf) fp_neg(np.y, np.y);
      const host::miller_lines* ls[1] = {&ctx->pairing->lines_tau};
      fa = host::multi_miller(&np, ls, 1);
      return 0;
    }
    g1_xyzz S;
    host_double_scalar_mul(S, z, P, y);  // [z]proof - [y]G
    if (!C.inf) xyzz_madd(S, C.x, C.y);
    host::g1_host_affine B;
    host_affine_from_xyzz(B, S);
    const host::miller_lines* ls[1] = {&ctx->pairing->lines_g2};
    fb = host::multi_miller(&B, ls, 1);
    return 0;
  });
  tt.mark("double-scalar multiplication, two miller loops (two threads)");
  *ok = host::final_exp_is_one(host::f12_mul(fa, fb), ctx->pairing->fc) ? 1 : 0;
  tt.mark("final exponentiation");
  return 0;
}

}  // namespace

// ---- phase 2 in four pieces ---------------------------------------------------------------------------------------------
// The two lincomb jobs of one phase 2 on session `s`.  A Phase2 that goes while a job is still active -- an error return, a rejected
// input whose sums are discarded -- drains the session first: nothing runs on its scratch when it goes.
struct Phase2 {
  kzg_verify_session* s;
  MsmVarJob ja, jb;
  explicit Phase2(kzg_verify_session* session) : s(session) {}
  ~Phase2() {
    if (ja.active || jb.active) session_drain(s);
  }
};
// (a) r = hash_to_fr("RCKZGBATCH___V1_" || u128(4096) || u128(n_total) || roots); scalars r_i, r_i z_i, -sum r_i y_i on `st`
//     p2_seed: r and its powers r^(2^k) into the session, on `st` (also the seed of the per-item terms, kzg_verify_session_tree)
static int32_t p2_seed(kzg_verify_session* s, const uint8_t* roots32, uint64_t world, uint64_t n_total) {
  hipStream_t st = s->st;
  std::vector<uint8_t> msg(48 + 32 * world);
  memcpy(msg.data(), facts(s->kind).domain, 16);  // the spec's domain of the blob batch or the cell batch
  memset(msg.data() + 16, 0, 32);
  msg[30] = 0x10;  // 4096 as u128 big-endian
  for (int k = 0; k < 8; k++) msg[47 - k] = (uint8_t)(n_total >> (8 * k));
  memcpy(msg.data() + 48, roots32, 32 * world);
  uint8_t digest[32];
  sha256_bytes(digest, msg.data(), msg.size());
  fr_t r;
  fr_from_be_bytes_plain(r, digest);
  fr_reduce_256(r);
  to_mont<FrParams>(r, r);
  fr_t rpow2[64];
  rpow2[0] = r;
  for (int k = 1; k < 64; k++) fr_sqr(rpow2[k], rpow2[k - 1]);
  if (hipMemcpyAsync(s->rpow2, rpow2, sizeof(rpow2), hipMemcpyHostToDevice, st) != hipSuccess) return fail(KZG_FAIL_HIP, "copy");  // pageable source: staged before the call returns
  return 0;
}
static int32_t p2_scalars(kzg_verify_session* s, const uint8_t* roots32, uint64_t world, uint64_t first_index, uint64_t n_total) {
  hipStream_t st = s->st;
  const uint64_t n = s->n;
  const int32_t rc = p2_seed(s, roots32, world, n_total);
  if (rc) return rc;
  const unsigned nblk = blocks_for(n, 256);
  // lincomb A's scalars r^k: B's commitment slots, or in the row-indexed form (whose ncom slots take the weights) an array of their own
  fr_t* rk = s->rows ? s->rpow : s->scal + n;
  fr_t* tail_scal = s->scal + n + s->ncom;
  hipLaunchKernelGGL(k_batch_scalars, dim3(nblk), dim3(256), 0, st, s->rpow2, s->z, s->y, n, first_index, rk, s->scal, s->ysum);
  if (s->from_blobs) {  // w_b = the sum of blob b's 128 consecutive powers
    ProfScope ps(s->ctx, PROF_POLY, st);
    hipLaunchKernelGGL(k_blob_weights, dim3((unsigned)s->ncom), dim3(CELLV_BLOB_ITEMS), 0, st, rk, s->scal + n);
  } else if (s->rows) {  // w_c = sum of the r^k whose item points at commitment c: B's ncom commitment scalars
    const uint32_t tiles = cellv_roww_tiles(n);
    ProfScope ps(s->ctx, PROF_POLY, st);  // no class of their own: a verification call launches nothing else of the k_poly class
    hipLaunchKernelGGL(k_cells_row_weights, dim3((unsigned)s->ncom, tiles), dim3(CELLV_ROWW_THREADS), 0, st, reinterpret_cast<const unsigned long long*>(s->d_com_indices),
                       stat_of(s, kzg::verify::CELLS_INDEX), rk, n, cellv_roww_tile(n), s->roww_part);
    hipLaunchKernelGGL(k_cells_roww_reduce, dim3(blocks_for(s->ncom, 256)), dim3(256), 0, st, s->roww_part, tiles, s->ncom, s->scal + n);
  }
  if (s->kind == VerifyKind::CELLS) {
    // y = 0: the generator's slot is S_0's.  The 64 scalars -S_j of the monomial terms: r^k (s->scal + n, just written) times the
    // interpolation polynomial of cell k, summed per workgroup, then over the workgroups
    const unsigned ngrp = blocks_for(n, CELLV_CELLS);
    if (s->from_blobs)
      hipLaunchKernelGGL(k_blob_cells_interp, dim3(ngrp), dim3(CELLV_THREADS), 0, st, s->d_blobs, s->ext, stat_of(s, kzg::verify::CELLS_INDEX),
                         stat_of(s, kzg::verify::CELLS_CELL), rk, n, s->ctx->d_cells_tab, s->ctx->d_cellv_tab, s->cell_part);
    else
      hipLaunchKernelGGL(k_cells_interp, dim3(ngrp), dim3(CELLV_THREADS), 0, st, s->d_cells, reinterpret_cast<const unsigned long long*>(s->d_cell_indices),
                         stat_of(s, kzg::verify::CELLS_INDEX), stat_of(s, kzg::verify::CELLS_CELL), rk, n, s->ctx->d_cells_tab, s->ctx->d_cellv_tab, s->cell_part);
    hipLaunchKernelGGL(k_cells_reduce, dim3(1), dim3(256), 0, st, s->cell_part, ngrp, tail_scal);
  } else {
    hipLaunchKernelGGL(k_batch_ysum_finish, dim3(1), dim3(256), 0, st, s->ysum, nblk, tail_scal);
  }
  if (s->glv) hipLaunchKernelGGL(k_glv_split, dim3(blocks_for(2 * n + s->tail, 256)), dim3(256), 0, st, s->scal, n, s->tail, s->glv_b, s->glv_a);
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "verify phase 2 launch failed");
  return 0;
}
// (b) the sorting halves of the two lincombs  A = sum r_i proof_i  (aux stream)  and
//     B = sum (r_i z_i) proof_i + sum r_i commitment_i - (sum r_i y_i) G  (the caller's stream; the longer one, enqueued first).
//     They need the scalars only: `beside_decoder` uses the kernels that fit next to two decoder waves and ignores the
//     infinity flags (which the decoder may not have written yet).
static int32_t p2_sort(kzg_verify_session* s, Phase2& p2, bool beside_decoder) {
  const kzg_ctx* ctx = s->ctx;
  const uint64_t n = s->n, nb = n + s->ncom + s->tail;  // lincomb B's terms
  (void)hipEventRecord(s->ev_aux, s->st);
  (void)hipStreamWaitEvent(s->aux, s->ev_aux, 0);
  const uint8_t* inf = beside_decoder ? nullptr : s->inf;
  int32_t rc = 0;
  if (s->glv) {  // (points at infinity are all-zero entries, theirs and their images': the bucket chains skip them, no flags needed)
    {
      ProfScope psb(ctx, PROF_VAR_MSM, s->st);
      rc = msm_var_sort(ctx, p2.jb, nullptr, s->glv_b, 2 * nb, s->st, s->msm_b, beside_decoder, true, nb, nb);
    }
    if (rc == 0) {
      ProfScope psa(ctx, PROF_VAR_MSM, s->aux);
      rc = msm_var_sort(ctx, p2.ja, nullptr, s->glv_a, 2 * n, s->aux, s->msm_a, beside_decoder, true, n, nb);
    }
    return rc;
  }
  {
    ProfScope psb(ctx, PROF_VAR_MSM, s->st);
    rc = msm_var_sort(ctx, p2.jb, inf, s->scal, nb, s->st, s->msm_b, beside_decoder, false, 0, 0, n + nb);
  }
  if (rc == 0) {
    ProfScope psa(ctx, PROF_VAR_MSM, s->aux);
    rc = msm_var_sort(ctx, p2.ja, inf, s->rows ? s->rpow : s->scal + n, n, s->aux, s->msm_a, beside_decoder, false, 0, 0, n + nb);
  }
  return rc;
}
// (c) bucket sums and bit sums: both streams wait for the decoded points first
static int32_t p2_accumulate(kzg_verify_session* s, Phase2& p2) {
  const kzg_ctx* ctx = s->ctx;
  (void)hipStreamWaitEvent(s->st, s->ev_join, 0);
  (void)hipStreamWaitEvent(s->aux, s->ev_join, 0);
  int32_t rc = 0;
  {
    ProfScope psb(ctx, PROF_VAR_MSM, s->st);
    rc = msm_var_accumulate(ctx, p2.jb, s->aff, s->st);
  }
  if (rc == 0) {
    ProfScope psa(ctx, PROF_VAR_MSM, s->aux);
    rc = msm_var_accumulate(ctx, p2.ja, s->aff, s->aux);
  }
  return rc;
}
// (d) read-backs and the host's Horner loops over the window / bit sums (0.25-0.3 ms each at 65,536 items) side by side: B's
//     here, A's on a helper thread (both jobs finish on the GPU within 0.2 ms of each other, so one after the other the second
//     loop was exposed in full); a helper's error text is re-published on this thread and a helper that cannot be started
//     runs inline (run_on_helpers).  out192 = A || B, affine big-endian.
static int32_t p2_finish(kzg_verify_session* s, Phase2& p2, uint8_t* out192) {
  const kzg_ctx* ctx = s->ctx;
  g1_xyzz Ax, Bx;
  int32_t rca = 0, rcb = 0;
  if (p2.ja.active && p2.jb.active && (p2.ja.nout + p2.jb.nout) >= 64) {
    const int device = ctx->device;
    (void)run_on_helpers(2, [&](uint32_t k) -> int32_t {
      if (k == 0) return rcb = msm_var_finish(p2.jb, Bx);
      (void)hipSetDevice(device);
      return rca = msm_var_finish(p2.ja, Ax);
    });
  } else {
    rca = msm_var_finish(p2.ja, Ax);
    rcb = msm_var_finish(p2.jb, Bx);
  }
  TraceTimer tt(ctx->knobs.trace, "phase2 finish");
  (void)hipStreamSynchronize(s->st);
  tt.mark("stream drained");
  if (rcb || rca) return rcb ? rcb : rca;
  host::g1_host_affine A, B;
  host_affine_from_xyzz(A, Ax);
  host_affine_from_xyzz(B, Bx);
  host_affine_to_be96(out192, A);
  host_affine_to_be96(out192 + 96, B);
  tt.mark("two inversions + encoding");
  return 0;
}

// (d') the single-context call's ending: each host thread takes ONE lincomb from the read-back to its Miller loop -- Horner over
//      the bit sums, to affine, f_A = f_{|z|,[tau]_2}(-A) or f_B = f_{|z|,G2}(B) -- and the caller multiplies the two and runs the
//      final exponentiation.  e(-A,[tau]_2) e(B,G2) = 1 exactly as verify_pairings_fixed checks it (the product of the two loops
//      is the shared-squaring loop's value: (f_A^2 l_A)(f_B^2 l_B) = (f_A f_B)^2 l_A l_B), 0.13 ms sooner: the loops run side by side.
static int32_t p2_finish_and_pair(kzg_verify_session* s, Phase2& p2, int32_t* ok) {
  const kzg_ctx* ctx = s->ctx;
  *ok = 0;
  if (!(p2.ja.active && p2.jb.active && (p2.ja.nout + p2.jb.nout) >= 64)) {  // a handful of terms: the plain path
    uint8_t partial[192];
    int32_t rc = p2_finish(s, p2, partial);
    return rc ? rc : verify_batch_finish(ctx, partial, 1, s->kind, ok);
  }
  TraceTimer tt(ctx->knobs.trace, "phase2 finish + pairing");
  host::fp12 fa = host::f12_one(), fb = host::f12_one();
  int32_t rca = 0, rcb = 0;
  const int device = ctx->device;
  auto one = [&](MsmVarJob& job, const host::miller_lines& lines, bool negate, host::fp12& f) -> int32_t {
    g1_xyzz sum;
    int32_t rc = msm_var_finish(job, sum);
    if (rc) return rc;
    host::g1_host_affine p;
    host_affine_from_xyzz(p, sum);
    if (negate && !p.inf) fp_neg(p.y, p.y);
    const host::miller_lines* ls[1] = {&lines};
    f = host::multi_miller(&p, ls, 1);
    return 0;
  };
  (void)run_on_helpers(2, [&](uint32_t k) -> int32_t {
    if (k == 0) return rcb = one(p2.jb, ctx->pairing->lines_g2, false, fb);
    (void)hipSetDevice(device);
    return rca = one(p2.ja, lines_against_a(ctx, s->kind), true, fa);
  });
  (void)hipStreamSynchronize(s->st);
  tt.mark("read-backs, horner, miller loops (two threads)");
  if (rcb || rca) return rcb ? rcb : rca;
  *ok = host::final_exp_is_one(host::f12_mul(fa, fb), ctx->pairing->fc) ? 1 : 0;
  tt.mark("final exponentiation");
  return 0;
}

extern "C" int32_t kzg_verify_phase2_dev(kzg_verify_session* s, const uint8_t* roots32, uint64_t world, uint64_t first_index, uint64_t n_total,
                                         uint8_t* out192) try {
  if (!s || !roots32 || !out192 || world == 0) return fail(KZG_FAIL_ARGUMENT, "null argument");
  const kzg_ctx* ctx = s->ctx;
  TraceTimer tt(ctx->knobs.trace, "phase2");
  HIP_TRY(hipSetDevice(ctx->device));
  if (s->n == 0) {
    memset(out192, 0, 192);  // A = B = infinity
    return 0;
  }
  Phase2 p2(s);
  int32_t rc = p2_scalars(s, roots32, world, first_index, n_total);
  tt.mark("seed + scalars enqueue");
  if (rc == 0) rc = p2_sort(s, p2, false);
  if (rc == 0) rc = p2_accumulate(s, p2);
  if (rc == 0) rc = p2_finish(s, p2, out192);
  tt.mark("msm A || msm B (incl. host horner)");
  return rc;
} catch (...) {
  return abi_exception();
}

// one item of a single-context call after phase 1: read back the two decoded points, z, y and the three statuses; the rest on the host
static int32_t verify_one_tail(kzg_verify_session* s, int32_t* ok) {
  *ok = 0;
  struct {
    uint32_t aff[48];  // proof, commitment: x || y each
    fr_t z, y;
    int32_t stat[3];   // blob, commitment, proof
    uint8_t inf[2];
  } h;
  hipStream_t st = s->st;
  if (hipStreamWaitEvent(st, s->ev_join, 0) != hipSuccess ||  // the decoder (its own stream when the launch was not the fused one)
      hipMemcpyAsync(h.aff, s->aff, sizeof(h.aff), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(&h.z, s->z, sizeof(fr_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(&h.y, s->y, sizeof(fr_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(h.stat, s->stat, sizeof(h.stat), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(h.inf, s->inf, sizeof(h.inf), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return fail(KZG_FAIL_HIP, "single-item read-back failed");
  for (int k = 0; k < 3; k++)  // first-error-wins: blob, commitment, proof (src/kzg/setup.rs:259-271)
    if (h.stat[k]) return h.stat[k];
  return verify_one_on_host(s->ctx, h.aff, h.inf[0] != 0, h.aff + 24, h.inf[1] != 0, h.z, h.y, ok);
}

// The single-context call, phases interleaved: everything that does not need the decoded POINTS -- transcript, root, r, the
// scalars, and the digit / histogram / scan / scatter halves of both lincombs -- is enqueued while the point decoder still runs
// on the session's side stream (its 2 x 224-VGPR waves leave every SIMD 64 registers, and each of those kernels fits in 64),
// so the bucket kernels start the moment the decoder ends.  Before, all of that queued up behind it: a host round trip and
// ~0.7 ms of short kernels on a nearly idle chip (profiles/r03/verify65536_kernel_timeline.txt).  The statuses are read after
// the bucket kernels are enqueued; a rejected input still wins (its code is returned, the sums are discarded).
// `in`: device-resident inputs of the session's kind; `root_done`: the host-buffer blob path, whose front ran -- and whose root was
// taken -- while the staging arena was still locked (verify_phase1_host).
static int32_t verify_fused(kzg_verify_session* s, const VerifyInputs& in, int32_t* ok, const uint8_t* root_done) {
  const kzg_ctx* ctx = s->ctx;
  const int kinds = facts(s->kind).entries;
  TraceTimer tt(ctx->knobs.trace, facts(s->kind).trace_fused);
  uint8_t root[32];
  int32_t err[8];
  err_clear(err, kinds);
  Phase2 p2(s);
  int32_t rc = 0;
  if (root_done) {
    memcpy(root, root_done, 32);
  } else {
    rc = front_enqueue(s, in);
    if (rc == 0) rc = p1_root(s, root);
  }
  tt.mark("front + transcript, root");
  if (rc == 0) rc = p2_scalars(s, root, 1, 0, s->n);
  if (rc == 0) rc = p2_sort(s, p2, true);
  if (rc == 0) rc = p2_accumulate(s, p2);
  if (rc == 0) rc = front_status(s, err);
  tt.mark("decoder done, first errors");
  const int32_t code = rc == 0 ? session_error_code(s, err) : 0;
  if (rc == 0 && code == 0) rc = p2_finish_and_pair(s, p2, ok);
  tt.mark("lincombs + host horner + pairing");
  return rc ? rc : code;  // a rejected input wins: its code is returned, the sums are discarded
}

// introspection: challenge z_i and evaluation y_i of items [first, first + count) of a session after phase 1
extern "C" int32_t kzg_verify_session_zy(kzg_verify_session* s, uint64_t first, uint64_t count, uint8_t* out_z32, uint8_t* out_y32) try {
  if (!s || !out_z32 || !out_y32 || first + count > s->n) return fail(KZG_FAIL_ARGUMENT, "bad argument");
  if (count == 0) return 0;
  HIP_TRY(hipSetDevice(s->ctx->device));
  std::vector<fr_t> hz(count), hy(count);
  HIP_TRY(hipStreamSynchronize(s->st));
  HIP_TRY(hipMemcpy(hz.data(), s->z + first, count * sizeof(fr_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hy.data(), s->y + first, count * sizeof(fr_t), hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < count; i++)
    for (int q = 0; q < 8; q++) {
      store_be32(out_z32 + 32 * i + 4 * q, hz[i].v[7 - q]);
      store_be32(out_y32 + 32 * i + 4 * q, hy[i].v[7 - q]);
    }
  return 0;
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_batch_finish(const kzg_ctx* ctx, const uint8_t* partials192, uint64_t world, int32_t* ok) try {
  if (!ctx || !ok || (world && !partials192)) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return verify_batch_finish(ctx, partials192, world, VerifyKind::BLOBS, ok);  // the blob and points kinds' pairing: partials carry no kind
} catch (...) {
  return abi_exception();
}
int32_t verify_batch_finish(const kzg_ctx* ctx, const uint8_t* partials192, uint64_t world, VerifyKind kind, int32_t* ok) {
  *ok = 0;
  g1_xyzz A, B;
  xyzz_set_inf(A);
  xyzz_set_inf(B);
  for (uint64_t k = 0; k < world; k++) {
    host::g1_host_affine a, b;
    if (!host_affine_from_be96(a, partials192 + 192 * k) || !host_affine_from_be96(b, partials192 + 192 * k + 96))
      return fail(KZG_FAIL_ARGUMENT, "malformed partial point");
    if (!a.inf) xyzz_madd(A, a.x, a.y);
    if (!b.inf) xyzz_madd(B, b.x, b.y);
  }
  host::g1_host_affine a, b;
  TraceTimer tt(ctx->knobs.trace, "finish");
  host_affine_from_xyzz(a, A);
  host_affine_from_xyzz(b, B);
  *ok = host::verify_pairings_fixed(*ctx->pairing, lines_against_a(ctx, kind), a, b) ? 1 : 0;
  tt.mark("pairing");
  return 0;
}

// The answer every batch entry point gives before anything else is looked at: the empty batch verifies (reference quirk Q4).
static int32_t empty_batch(int32_t* ok) {
  *ok = 1;
  return 0;
}
// The body of the twelve kzg_verify_*_batch[_each][_dev] entry points: `each` = the per-item forms' outputs, `st` = the caller's stream
// of the _dev forms.  Host buffers on a group context go over its members; device pointers stay on the context they were given to.
static int32_t batch_entry(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, const VerifyEach* each, int32_t* ok, hipStream_t st) {
  if (!ctx || !ok || (n && (in.any_null() || (each && (!each->ok_each || !each->status))))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  if (n == 0) return empty_batch(ok);
  if (in.on_host && is_group(ctx)) return each ? multi_verify_each(ctx, in, n, *each, ok) : multi_verify_batch(ctx, in, n, ok);
  return verify_batch_single(ctx, in, n, st, each, ok);
}

extern "C" int32_t kzg_verify_blob_proof_batch_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_proofs48,
                                                   uint64_t n, int32_t* ok, void* hip_stream) try {
  return batch_entry(ctx, blob_inputs(d_blobs, d_commitments48, d_proofs48, false), n, nullptr, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

// Setup::verify_blob_proof_batch (src/kzg/setup.rs:223-275) or Setup::verify_proof_batch (:115-161) over device-resident shares of a
// group context, all of one kind, phases interleaved PER MEMBER as in verify_fused: round 1 enqueues the front on every member and
// returns the members' roots while the decoders still run; round 2 seeds ONE challenge with all roots and, per member, enqueues
// the scalars (global powers r^i), the sorting halves of both lincombs beside the decoder, the bucket kernels behind it, reads the
// first errors and takes the member's two partial sums.  Then the first-error merge in the reference's order over GLOBAL indices
// (multi_split.hpp) and one pairing check.  Two fork/joins of pooled host threads per call.
int32_t verify_group_dev(const kzg_ctx* ctx, const std::vector<GroupDevShare>& shares, uint64_t n_total, int32_t* ok) {
  *ok = 0;
  const uint32_t W = (uint32_t)shares.size();
  if (W == 0) return empty_batch(ok);
  const VerifyKind kind = shares[0].in.kind;
  // one share: exactly the single-device call (one root seeds the challenge)
  if (W == 1) return verify_batch_single(shares[0].member, shares[0].in, shares[0].count, shares[0].st, nullptr, ok);
  TraceTimer tt(ctx->knobs.trace, facts(kind).trace_group_dev);
  const int kinds = facts(kind).entries;
  const size_t stride = 2 * (size_t)kinds;
  std::vector<uint8_t> roots(32 * (size_t)W), partials(192 * (size_t)W);
  std::vector<int32_t> err(stride * W);
  for (uint32_t j = 0; j < W; j++) err_clear(err.data() + stride * j, kinds);
  std::vector<SessionUse> uses(W);
  auto release = [&]() {  // handing a session back may fail on its own: the error the caller is told about stays the first one
    const ErrorSnapshot keep = error_snapshot();
    for (SessionUse& u : uses) u.reset();
    error_publish(keep);
  };
  int32_t rc = run_on_helpers(W, [&](uint32_t j) -> int32_t {
    const GroupDevShare& sh = shares[j];
    if (hipSetDevice(sh.member->device) != hipSuccess) return fail(KZG_FAIL_HIP, "hipSetDevice failed");
    int32_t r = session_acquire(sh.member, sh.count, sh.st, kind, false, &uses[j].s);
    if (r == 0) r = front_enqueue(uses[j].s, sh.in);
    if (r == 0) r = p1_root(uses[j].s, roots.data() + 32 * (size_t)j);
    return r;
  });
  tt.mark("round 1: front, transcript, roots (decoders still running)");
  if (rc) {
    release();
    return rc;
  }
  std::vector<int32_t> codes(W, 0);
  rc = run_on_helpers(W, [&](uint32_t j) -> int32_t {
    const GroupDevShare& sh = shares[j];
    kzg_verify_session* s = uses[j].s;
    int32_t* e = err.data() + stride * j;
    if (hipSetDevice(sh.member->device) != hipSuccess) return fail(KZG_FAIL_HIP, "hipSetDevice failed");
    Phase2 p2(s);
    int32_t r = p2_scalars(s, roots.data(), W, sh.first, n_total);
    if (r == 0) r = p2_sort(s, p2, true);
    if (r == 0) r = p2_accumulate(s, p2);
    if (r == 0) r = front_status(s, e);
    if (r == 0) codes[j] = first_error_code(e, kinds);
    if (r == 0 && codes[j] == 0) r = p2_finish(s, p2, partials.data() + 192 * (size_t)j);  // a rejected input's sums are discarded
    return r;
  });
  tt.mark("round 2: scalars, lincombs, first errors, partial sums");
  release();
  if (rc) return rc;
  std::vector<kzg::multi::Share> ms(W);
  for (uint32_t j = 0; j < W; j++) ms[j] = kzg::multi::Share{j, shares[j].first, shares[j].count};
  const int32_t code = kzg::multi::merged_first_error(ms, err.data(), kinds);
  if (code) return code;
  rc = verify_batch_finish(ctx, partials.data(), W, kind, ok);
  tt.mark("sum of partials + pairing");
  return rc;
}

extern "C" int32_t kzg_verify_blob_proof_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* proofs48,
                                               uint64_t n, int32_t* ok) try {
  return batch_entry(ctx, blob_inputs(blobs, commitments48, proofs48, true), n, nullptr, ok, nullptr);
} catch (...) {
  return abi_exception();
}

// Setup::verify_blob_proof (src/kzg/setup.rs:208-221): a batch of one (the random
// coefficient is r^0 = 1, so this is exactly verify_proof_inner's equation)
extern "C" int32_t kzg_verify_blob_proof(const kzg_ctx* ctx, const uint8_t* blob, const uint8_t* commitment48, const uint8_t* proof48, int32_t* ok) try {
  return kzg_verify_blob_proof_batch(ctx, blob, commitment48, proof48, 1, ok);
} catch (...) {
  return abi_exception();
}

// Setup::verify_proof (src/kzg/setup.rs:96-113).  e(pi, [tau]_2 - z G2) == e(C - y G, G2)
// is checked in the equivalent fixed-G2 form  e(pi, [tau]_2) == e(C - y G + z pi, G2): a one-item session whose z and y
// come from the caller instead of the challenge/evaluation kernels (the batch coefficient of item 0 is r^0 = 1).
// Error order of the reference: proof, commitment, z, y.
extern "C" int32_t kzg_verify_proof(const kzg_ctx* ctx, const uint8_t* proof48, const uint8_t* commitment48, const uint8_t* z32, const uint8_t* y32,
                                    int32_t* ok) try {
  if (!ctx || !proof48 || !commitment48 || !z32 || !y32 || !ok) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return (is_group(ctx) ? multi_verify_proof : verify_proof_single)(ctx, proof48, commitment48, z32, y32, ok);
} catch (...) {
  return abi_exception();
}
int32_t verify_proof_single(const kzg_ctx* ctx, const uint8_t* proof48, const uint8_t* commitment48, const uint8_t* z32, const uint8_t* y32, int32_t* ok) {
  *ok = 0;
  HIP_TRY(hipSetDevice(ctx->device));
  SessionUse use;
  // a private stream per call would cost a creation; the session's own stream carries the whole single-item call
  // (POINTS: the one-item session is read by phase 2 only, where blobs and points do not differ)
  int32_t rc = session_acquire(ctx, 1, KZG_SESSION_STREAM, VerifyKind::POINTS, false, &use.s);
  if (rc) return rc;
  kzg_verify_session* s = use.s;
  hipStream_t st = s->st;
  int32_t h_stat[2] = {0, 0};
  uint32_t h_aff[48];  // proof, commitment as decoded
  uint8_t h_inf[2] = {0, 0};
  fr_t zy[2];
  do {
    fr_from_be_bytes_plain(zy[0], z32);
    fr_from_be_bytes_plain(zy[1], y32);
    uint8_t in[96];
    memcpy(in, proof48, 48);
    memcpy(in + 48, commitment48, 48);
    if (hipMemcpyAsync(s->pts48, in, 96, hipMemcpyHostToDevice, st) != hipSuccess) { rc = fail(KZG_FAIL_HIP, "copy"); break; }
    launch_g1_decompress(st, s->pts48, (uint64_t)1, s->stat + 2, s->pts48 + 48, (uint64_t)1, s->stat + 1, s->aff, s->inf);
    if (hipMemcpyAsync(h_stat, s->stat + 1, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(h_aff, s->aff, sizeof(h_aff), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(h_inf, s->inf, sizeof(h_inf), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      rc = fail(KZG_FAIL_HIP, "copy");
      break;
    }
    if (h_stat[1]) { rc = h_stat[1]; break; }  // proof first (src/kzg/setup.rs:103)
    if (h_stat[0]) { rc = h_stat[0]; break; }
    if (!fr_is_canonical(zy[0]) || !fr_is_canonical(zy[1])) { rc = KZG_ERR_FF_NOT_IN_FIELD; break; }
    if (!ctx->knobs.single_via_batch) break;  // the lincomb and the pairing on the host (verify_one_on_host)
    if (hipMemcpyAsync(s->z, &zy[0], 32, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(s->y, &zy[1], 32, hipMemcpyHostToDevice, st) != hipSuccess) { rc = fail(KZG_FAIL_HIP, "copy"); break; }
  } while (0);
  uint8_t partial[192];
  if (rc == 0 && ctx->knobs.single_via_batch) {
    const uint8_t root[32] = {0};
    rc = kzg_verify_phase2_dev(s, root, 1, 0, 1, partial);
  }
  use.reset();  // the host's part needs no session
  if (rc) return rc;
  if (!ctx->knobs.single_via_batch) return verify_one_on_host(ctx, h_aff, h_inf[0] != 0, h_aff + 24, h_inf[1] != 0, zy[0], zy[1], ok);
  return kzg_verify_batch_finish(ctx, partial, 1, ok);
}

// ---- Setup::verify_proof_batch (src/kzg/setup.rs:115-161) as a public batch call: n caller-supplied (proof, commitment, z, y) -------
// The blob batch's drivers (verify_batch_single, verify_phase1, verify_fused, verify_group_dev) over point_inputs: only the front and the
// reading of the four-kind error record differ -- front_enqueue / front_status, POINTS.
extern "C" int32_t kzg_verify_proof_phase1_dev(const kzg_ctx* ctx, const void* d_proofs48, const void* d_commitments48, const void* d_z32, const void* d_y32,
                                               uint64_t n, uint8_t* out_root32, int32_t* err8, kzg_verify_session** session, void* hip_stream) try {
  return phase1_entry(ctx, point_inputs(d_proofs48, d_commitments48, d_z32, d_y32, false), n, (hipStream_t)hip_stream, out_root32, err8, session);
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_proof_batch_dev(const kzg_ctx* ctx, const void* d_proofs48, const void* d_commitments48, const void* d_z32, const void* d_y32,
                                              uint64_t n, int32_t* ok, void* hip_stream) try {
  return batch_entry(ctx, point_inputs(d_proofs48, d_commitments48, d_z32, d_y32, false), n, nullptr, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_proof_batch(const kzg_ctx* ctx, const uint8_t* proofs48, const uint8_t* commitments48, const uint8_t* z32, const uint8_t* y32,
                                          uint64_t n, int32_t* ok) try {
  return batch_entry(ctx, point_inputs(proofs48, commitments48, z32, y32, true), n, nullptr, ok, nullptr);
} catch (...) {
  return abi_exception();
}

// ---- per-item verdicts: kzg_verify_*_batch_each, kzg_verify_session_tree(_range) ------------------------------------------------------
// What the reference's users do when a batch is false -- a loop over Setup::verify_blob_proof / verify_proof (src/kzg/setup.rs:208-221,
// :96-113) -- answered from ONE phase 1: per item the single call's code (k_each_status over the session's status arrays) and its boolean.
// Fast path: nothing rejected and the batch check true -> every item true, the terms kernel never runs.  Otherwise the per-item terms
// A_i, B_i (k_each_terms) and their two sum trees (k_each_level) are built in the session and the host descends from the root
// (each_descent.hpp), paying one two-pairing check per visited node: O(k log n) checks for k false items.  An inner node that hides a
// false item passes with probability <= n / 2^255 -- the batch call's own soundness statement, per subtree.
constexpr uint32_t EACH_GATHER = 4096;  // nodes per fetch (2 x 192 bytes each)
struct EachGeom {
  uint32_t height = 0;        // the root's level
  std::vector<uint64_t> off;  // off[l]: position of level l's first node; off[height + 1] = all nodes
};
static EachGeom each_geom(uint64_t n) {
  EachGeom g;
  g.height = kzg::each::tree_height(n);
  g.off.assign(g.height + 2, 0);
  for (uint32_t l = 0; l <= g.height; l++) g.off[l + 1] = g.off[l] + kzg::each::level_count(n, l);
  return g;
}
// the session's tree storage for its current n (about 50 MB at 65,536 items; grown on demand, freed with the session).  The cells kind
// carves its vector tree BEHIND everything else (2 KiB per node, about 4 KiB per item: 268 MB at 65,536 items); the other kinds' carve
// is what it was.
static int32_t each_reserve(kzg_verify_session* s, const EachGeom& g) {
  const uint64_t n = s->n, total = g.off[g.height + 1];
  if (total >> 32) return fail(KZG_FAIL_ARGUMENT, "per-item verdicts: batch too large");
  Carve c;
  const size_t o_status = c.take(n * sizeof(int32_t)), o_rej = c.take(2 * sizeof(uint32_t)), o_a = c.take(total * sizeof(g1_xyzz28)),
               o_b = c.take(total * sizeof(g1_xyzz28)), o_idx = c.take(EACH_GATHER * sizeof(uint32_t)), o_out = c.take(2 * EACH_GATHER * sizeof(g1_xyzz));
  const bool is_cells = s->kind == VerifyKind::CELLS;
  const size_t o_vec = is_cells ? c.take(total * 64 * sizeof(fr_t)) : 0;
  if (s->tree_cap < c.off) {
    if (s->tree) (void)hipFree(s->tree);
    s->tree = nullptr;
    s->tree_cap = 0;
    const size_t want = c.off + c.off / 8;
    if (hipMalloc(&s->tree, want) != hipSuccess) return fail(KZG_FAIL_HIP, "hipMalloc(per-item verdict trees) failed");
    s->tree_cap = want;
  }
  s->t_status = reinterpret_cast<int32_t*>(s->tree + o_status);
  s->t_rejected = reinterpret_cast<uint32_t*>(s->tree + o_rej);
  s->t_a = reinterpret_cast<g1_xyzz28*>(s->tree + o_a);
  s->t_b = reinterpret_cast<g1_xyzz28*>(s->tree + o_b);
  s->t_idx = reinterpret_cast<uint32_t*>(s->tree + o_idx);
  s->t_out = reinterpret_cast<g1_xyzz*>(s->tree + o_out);
  s->t_vec = is_cells ? reinterpret_cast<fr_t*>(s->tree + o_vec) : nullptr;
  return 0;
}
// per-item codes in the single-item call's parse order, which is the error record's (verify_kind.hpp; a three-entry record has no fourth
// array) -- on the caller's stream, behind the front's kernels there and the decoder (ev_join)
static int32_t each_status_enqueue(kzg_verify_session* s) {
  const uint64_t n = s->n;
  hipStream_t st = s->st;
  if (hipStreamWaitEvent(st, s->ev_join, 0) != hipSuccess || hipMemsetAsync(s->t_rejected, 0, (s->rows ? 2 : 1) * sizeof(uint32_t), st) != hipSuccess)
    return fail(KZG_FAIL_HIP, "per-item verdicts: status enqueue failed");
  if (s->from_blobs) {  // the blob's code (blob, commitment, lowest rejected proof) for all 128 items of it; counts[0] = the rejected blobs
    hipLaunchKernelGGL(k_each_blob_status, dim3((unsigned)s->ncom), dim3(CELLV_BLOB_ITEMS), 0, st, s->blob_stat, stat_of(s, 1), stat_of(s, 3), s->t_status,
                       s->blob_code, s->t_rejected);
    if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "per-item verdicts: status launch failed");
    return 0;
  }
  if (s->rows) {  // the commitment's code through the item's index, and the rejected entries of the list counted beside the rejected items
    hipLaunchKernelGGL(k_each_rows_status, dim3(blocks_for(s->stride, 256)), dim3(256), 0, st, stat_of(s, 0), stat_of(s, 1), stat_of(s, 2), stat_of(s, 3),
                       reinterpret_cast<const unsigned long long*>(s->d_com_indices), s->ncom, n, s->t_status, s->t_rejected);
    if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "per-item verdicts: status launch failed");
    return 0;
  }
  hipLaunchKernelGGL(k_each_status, dim3(blocks_for(n, 256)), dim3(256), 0, st, stat_of(s, 0), stat_of(s, 1), stat_of(s, 2), stat_of(s, 3), n, s->t_status,
                     s->t_rejected);
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "per-item verdicts: status launch failed");
  return 0;
}
// terms and both trees -- cells: the vector tree as well -- on the caller's stream behind each_status_enqueue and the seed (p2_seed)
static int32_t each_build(kzg_verify_session* s, const EachGeom& g, uint64_t first_index) {
  const uint64_t n = s->n;
  hipStream_t st = s->st;
  if (s->from_blobs)  // the commitment of blob i >> 7 out of the list behind the n proofs
    hipLaunchKernelGGL(k_each_blob_terms, dim3(2 * blocks_for(n, 64)), dim3(64), 0, st, s->rpow2, s->z, s->y, s->aff, s->t_status, s->ncom, n, first_index, s->t_a,
                       s->t_b);
  else if (s->rows)  // the commitment gathered through the item's index out of the list behind the n proofs
    hipLaunchKernelGGL(k_each_rows_terms, dim3(2 * blocks_for(n, 64)), dim3(64), 0, st, s->rpow2, s->z, s->y, s->aff, s->t_status,
                       reinterpret_cast<const unsigned long long*>(s->d_com_indices), s->ncom, n, first_index, s->t_a, s->t_b);
  else
    hipLaunchKernelGGL(k_each_terms, dim3(2 * blocks_for(n, 64)), dim3(64), 0, st, s->rpow2, s->z, s->y, s->aff, s->t_status, n, first_index, s->t_a, s->t_b);
  for (uint32_t l = 0; l < g.height; l++) {
    const uint64_t cin = g.off[l + 1] - g.off[l], cout = g.off[l + 2] - g.off[l + 1];
    hipLaunchKernelGGL(k_each_level, dim3(blocks_for(2 * cout, 64)), dim3(64), 0, st, s->t_a + g.off[l], s->t_b + g.off[l], cin, s->t_a + g.off[l + 1],
                       s->t_b + g.off[l + 1], cout);
  }
  if (s->kind == VerifyKind::CELLS) {  // the monomial term's coefficient vectors r_i I_i and their sums; the points are taken per fetched node (each_fetch)
    if (s->from_blobs)
      hipLaunchKernelGGL(k_blob_cells_each_leaves, dim3(blocks_for(n, CELLV_CELLS)), dim3(CELLV_THREADS), 0, st, s->d_blobs, s->ext, s->t_status, s->rpow2, n,
                         first_index, s->ctx->d_cells_tab, s->ctx->d_cellv_tab, s->t_vec);
    else
      hipLaunchKernelGGL(k_cells_each_leaves, dim3(blocks_for(n, CELLV_CELLS)), dim3(CELLV_THREADS), 0, st, s->d_cells,
                         reinterpret_cast<const unsigned long long*>(s->d_cell_indices), s->t_status, s->rpow2, n, first_index, s->ctx->d_cells_tab,
                         s->ctx->d_cellv_tab, s->t_vec);
    for (uint32_t l = 0; l < g.height; l++) {
      const uint64_t cin = g.off[l + 1] - g.off[l], cout = g.off[l + 2] - g.off[l + 1];
      hipLaunchKernelGGL(k_each_vec_level, dim3(blocks_for(cout * 64, 256)), dim3(256), 0, st, s->t_vec + g.off[l] * 64, cin, s->t_vec + g.off[l + 1] * 64, cout);
    }
  }
  if (hipGetLastError() != hipSuccess) return fail(KZG_FAIL_HIP, "per-item verdicts: tree launch failed");
  s->tree_n = n;
  return 0;
}
// nodes at `pos` (positions in the node arrays) of both trees -> out[2 k] = A's, out[2 k + 1] = B's; synchronous.  Cells: B's node
// minus the monomial term of the node's coefficient vector, one wave per node (k_each_gather_cells)
static int32_t each_fetch(kzg_verify_session* s, const std::vector<uint32_t>& pos, std::vector<g1_xyzz>& out) {
  hipStream_t st = s->st;
  out.resize(2 * pos.size());
  for (size_t done = 0; done < pos.size(); done += EACH_GATHER) {
    const uint32_t m = (uint32_t)std::min<size_t>(EACH_GATHER, pos.size() - done);
    if (hipMemcpyAsync(s->t_idx, pos.data() + done, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) != hipSuccess)
      return fail(KZG_FAIL_HIP, "per-item verdicts: node fetch failed");
    if (s->kind == VerifyKind::CELLS)
      hipLaunchKernelGGL(k_each_gather_cells, dim3(m), dim3(64), 0, st, s->t_a, s->t_b, s->t_vec, s->ctx->d_g1_monomial, s->t_idx, m, true, s->t_out);
    else
      hipLaunchKernelGGL(k_each_gather, dim3(blocks_for(2 * (uint64_t)m, 64)), dim3(64), 0, st, s->t_a, s->t_b, s->t_idx, m, s->t_out);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out.data() + 2 * done, s->t_out, 2 * (size_t)m * sizeof(g1_xyzz), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return fail(KZG_FAIL_HIP, "per-item verdicts: node fetch failed");
  }
  return 0;
}
// The descent over the session's trees: ok_each[i] = the leaf check of item i -- the blob form: of BLOB i, the node (7, i); the descent
// stops at that floor and never enters a blob's 128 cells.  A level's nodes come back in one fetch and are checked
// side by side on the helper pool: to affine, two Miller loops, one final exponentiation each (host::verify_pairings_fixed).
static int32_t each_descend(kzg_verify_session* s, const EachGeom& g, uint8_t* ok_each) {
  const kzg_ctx* ctx = s->ctx;
  TraceTimer tt(ctx->knobs.trace, "per-item verdicts: descent");
  uint64_t checks = 0;
  std::vector<uint32_t> pos;
  std::vector<g1_xyzz> nodes;
  const int32_t rc = kzg::each::descend(s->n, ok_each, [&](uint32_t level, const uint64_t* idx, size_t m, uint8_t* pass) -> int32_t {
    pos.resize(m);
    for (size_t k = 0; k < m; k++) pos[k] = (uint32_t)(g.off[level] + idx[k]);
    const int32_t r = each_fetch(s, pos, nodes);
    if (r) return r;
    checks += m;
    std::atomic<size_t> next{0};
    const uint32_t hw = std::thread::hardware_concurrency();
    const uint32_t workers = (uint32_t)std::min<size_t>(m, std::max(1u, std::min(16u, hw)));
    return run_on_helpers(workers, [&](uint32_t) -> int32_t {
      for (size_t k = next.fetch_add(1); k < m; k = next.fetch_add(1)) {
        host::g1_host_affine a, b;
        host_affine_from_xyzz(a, nodes[2 * k]);
        host_affine_from_xyzz(b, nodes[2 * k + 1]);
        pass[k] = host::verify_pairings_fixed(*ctx->pairing, lines_against_a(ctx, s->kind), a, b) ? 1 : 0;
      }
      return 0;
    });
  }, s->from_blobs ? 7u : 0u);
  ctx->each_checks.fetch_add(checks, std::memory_order_relaxed);
  tt.mark("done");
  return rc;
}

extern "C" int32_t kzg_verify_session_tree(kzg_verify_session* s, const uint8_t* roots32, uint64_t world, uint64_t first_index, uint64_t n_total) try {
  if (!s || !roots32 || world == 0) return fail(KZG_FAIL_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(s->ctx->device));
  s->tree_n = 0;
  if (s->n == 0) return 0;
  const EachGeom g = each_geom(s->n);
  int32_t rc = each_reserve(s, g);
  if (rc == 0) rc = p2_seed(s, roots32, world, n_total);
  if (rc == 0) rc = each_status_enqueue(s);
  if (rc == 0) rc = each_build(s, g, first_index);
  if (rc == 0 && hipStreamSynchronize(s->st) != hipSuccess) rc = fail(KZG_FAIL_HIP, "per-item verdicts: tree build failed");
  if (rc) s->tree_n = 0;
  return rc;
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_session_tree_range(kzg_verify_session* s, uint64_t lo, uint64_t hi, uint8_t* out192) try {
  if (!s || !out192 || lo > hi || hi > s->n) return fail(KZG_FAIL_ARGUMENT, "bad argument");
  if (s->n && s->tree_n != s->n) return fail(KZG_FAIL_ARGUMENT, "kzg_verify_session_tree has not been called on this session");
  HIP_TRY(hipSetDevice(s->ctx->device));
  g1_xyzz A, B;
  xyzz_set_inf(A);
  xyzz_set_inf(B);
  if (lo < hi) {
    // [lo, hi) as at most 2 log2 n whole subtrees
    const EachGeom g = each_geom(s->n);
    std::vector<uint32_t> pos;
    uint64_t a = lo, b = hi;
    for (uint32_t l = 0; a < b; l++, a >>= 1, b >>= 1) {
      if (a & 1) pos.push_back((uint32_t)(g.off[l] + a++));
      if (b & 1) pos.push_back((uint32_t)(g.off[l] + --b));
    }
    std::vector<g1_xyzz> nodes;
    const int32_t rc = each_fetch(s, pos, nodes);
    if (rc) return rc;
    for (size_t k = 0; k < pos.size(); k++) {
      xyzz_add(A, nodes[2 * k]);
      xyzz_add(B, nodes[2 * k + 1]);
    }
  }
  host::g1_host_affine a, b;
  host_affine_from_xyzz(a, A);
  host_affine_from_xyzz(b, B);
  host_affine_to_be96(out192, a);
  host_affine_to_be96(out192 + 96, b);
  return 0;
} catch (...) {
  return abi_exception();
}

extern "C" uint64_t kzg_verify_each_checks(const kzg_ctx* ctx) {
  if (!ctx) return 0;
  uint64_t total = ctx->each_checks.load(std::memory_order_relaxed);
  for (const kzg_ctx* p : ctx->peers) total += p->each_checks.load(std::memory_order_relaxed);
  return total;
}
extern "C" uint64_t kzg_ctx_sessions_created(const kzg_ctx* ctx) {
  if (!ctx) return 0;
  uint64_t total = ctx->sessions_created.load(std::memory_order_relaxed);
  for (const kzg_ctx* p : ctx->peers) total += p->sessions_created.load(std::memory_order_relaxed);
  return total;
}

// The ending of the per-item calls: the session's front is enqueued and its root taken (n >= 2; the row-indexed form: n >= 1).
// The row-indexed form (s->rows): a rejected LISTED commitment, referenced or not, makes *ok 0 and keeps the batch check from running
// -- it would sum a rejected point -- while an item's verdict depends on its own commitment alone: the tree settles the items.
static int32_t each_finish(kzg_verify_session* s, const uint8_t* root, const VerifyEach& out, int32_t* ok) {
  const uint64_t n = s->n;
  const uint64_t verdicts = s->from_blobs ? s->ncom : n;  // the blob form answers per blob: status and ok_each have ncom entries
  *ok = 0;
  const EachGeom g = each_geom(n);
  uint32_t counts[2] = {0, 0};  // rejected items (the blob form: blobs); rows: rejected listed commitments
  int32_t rc = each_reserve(s, g);
  if (rc == 0) rc = each_status_enqueue(s);
  if (rc == 0 && (hipMemcpyAsync(out.status, s->from_blobs ? s->blob_code : s->t_status, verdicts * sizeof(int32_t), hipMemcpyDeviceToHost, s->st) != hipSuccess ||
                  hipMemcpyAsync(counts, s->t_rejected, (s->rows && !s->from_blobs ? 2 : 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s->st) != hipSuccess ||
                  (s->rows && out.commitment_status &&
                   hipMemcpyAsync(out.commitment_status, stat_of(s, 1), s->ncom * sizeof(int32_t), hipMemcpyDeviceToHost, s->st) != hipSuccess) ||
                  hipStreamSynchronize(s->st) != hipSuccess))
    rc = fail(KZG_FAIL_HIP, "per-item verdicts: status read-back failed");
  if (rc) return rc;
  const uint32_t rejected = counts[0], bad_list = counts[1];
  if (rejected == 0 && bad_list == 0) {  // today's batch check first: true = every item true
    Phase2 p2(s);
    int32_t all = 0;
    rc = p2_scalars(s, root, 1, 0, n);
    if (rc == 0) rc = p2_sort(s, p2, false);
    if (rc == 0) rc = p2_accumulate(s, p2);
    if (rc == 0) rc = p2_finish_and_pair(s, p2, &all);
    if (rc) return rc;
    if (all) {
      memset(out.ok_each, 1, verdicts);
      *ok = 1;
      return 0;
    }
  } else {
    rc = p2_seed(s, root, 1, n);
  }
  if (rc == 0) rc = each_build(s, g, 0);
  if (rc == 0) rc = each_descend(s, g, out.ok_each);
  if (rc) return rc;
  for (uint64_t i = 0; i < verdicts; i++)
    if (out.status[i]) out.ok_each[i] = 0;
  return 0;  // *ok = 0: an item or a listed commitment was rejected, or the batch check was false
}

// The single-device batch call (engine_internal.hpp).  What differs between the routes: how the session with device-resident inputs
// comes to be, the single-item shortcuts, and the ending.
int32_t verify_batch_single(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, hipStream_t st, const VerifyEach* each, int32_t* ok) {
  *ok = 0;
  const bool blobs = in.kind == VerifyKind::BLOBS;
  // (not the row-indexed form: its boolean call validates the whole LIST, and a listed commitment the item does not reference must not
  // become the item's status -- one item goes through each_finish like any other count)
  if (each && n == 1 && !in.rows()) {  // per-item verdicts of one item: the boolean call's answer in the per-item outputs
    int32_t one = 0;
    const int32_t rc = verify_batch_single(ctx, in, 1, st, nullptr, &one);
    if (rc < 0) return rc;
    each->status[0] = rc;
    *ok = each->ok_each[0] = (rc == 0 && one) ? 1 : 0;
    return 0;
  }
  // one tuple from host buffers: z and y parsed on the host, the lincombs there too (verify_one_on_host)
  if (n == 1 && in.on_host && in.kind == VerifyKind::POINTS) return verify_proof_single(ctx, in.proofs48, in.commitments48, in.z32, in.y32, ok);
  HIP_TRY(hipSetDevice(ctx->device));
  SessionUse use;
  uint8_t root[32];
  int32_t err6[6];
  // Host blobs pass through the staging arena, so their front runs -- and the root is taken -- while it is locked.  The per-item
  // ending asks for the statuses there although each_finish reads its own: kept as it was, a candidate for removal.
  const bool front_done = in.on_host && blobs;
  int32_t rc = front_done   ? verify_phase1_host(ctx, in.blobs, in.commitments48, in.proofs48, n, root, each ? err6 : nullptr, &use.s)
               : in.on_host ? points_stage_host(ctx, in, n, &use.s)
                            : session_acquire(ctx, n, st, in.kind, false, &use.s, in.rows() ? &in.ncom : nullptr, in.from_blobs);
  if (rc) return rc;
  kzg_verify_session* s = use.s;
  const VerifyInputs dev = in.on_host ? staged_inputs(s) : in;
  if (blobs && one_item_on_host(s)) {  // no transcript: the item's kernels, then the host (verify_one_tail)
    if (!front_done) rc = phase1_items(s, dev.blobs, dev.commitments48, dev.proofs48, 0, 1, s->st, true);
    return rc ? rc : verify_one_tail(s, ok);
  }
  if (!each) return verify_fused(s, dev, ok, front_done ? root : nullptr);
  if (!front_done) {
    rc = front_enqueue(s, dev);
    if (rc == 0) rc = p1_root(s, root);
  }
  return rc ? rc : each_finish(s, root, *each, ok);
}

extern "C" int32_t kzg_verify_blob_proof_batch_each_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_proofs48, uint64_t n,
                                                        uint8_t* ok_each, int32_t* status, int32_t* ok, void* hip_stream) try {
  const VerifyEach each{ok_each, status};
  return batch_entry(ctx, blob_inputs(d_blobs, d_commitments48, d_proofs48, false), n, &each, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_proof_batch_each_dev(const kzg_ctx* ctx, const void* d_proofs48, const void* d_commitments48, const void* d_z32, const void* d_y32,
                                                   uint64_t n, uint8_t* ok_each, int32_t* status, int32_t* ok, void* hip_stream) try {
  const VerifyEach each{ok_each, status};
  return batch_entry(ctx, point_inputs(d_proofs48, d_commitments48, d_z32, d_y32, false), n, &each, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_blob_proof_batch_each(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* proofs48, uint64_t n,
                                                    uint8_t* ok_each, int32_t* status, int32_t* ok) try {
  const VerifyEach each{ok_each, status};
  return batch_entry(ctx, blob_inputs(blobs, commitments48, proofs48, true), n, &each, ok, nullptr);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_verify_proof_batch_each(const kzg_ctx* ctx, const uint8_t* proofs48, const uint8_t* commitments48, const uint8_t* z32, const uint8_t* y32,
                                               uint64_t n, uint8_t* ok_each, int32_t* status, int32_t* ok) try {
  const VerifyEach each{ok_each, status};
  return batch_entry(ctx, point_inputs(proofs48, commitments48, z32, y32, true), n, &each, ok, nullptr);
} catch (...) {
  return abi_exception();
}

// ---- verify_cell_kzg_proof_batch (EIP-7594) as the third kind of batch call: n (commitment, cell index, cell, proof) tuples -------------
// The points batch's drivers over cell_inputs: the front (k_cells_leaves), the 64 scalars of the monomial terms in p2_scalars
// (k_cells_interp, k_cells_reduce), lincomb B's 2n + 64 terms and the pairing against [tau^64]_2 differ -- each behind the session's kind.
extern "C" int32_t kzg_verify_cell_proof_batch_dev(const kzg_ctx* ctx, const void* d_commitments48, const void* d_cell_indices, const void* d_cells,
                                                   const void* d_proofs48, uint64_t n, int32_t* ok, void* hip_stream) try {
  return batch_entry(ctx, cell_inputs(d_commitments48, d_cell_indices, d_cells, d_proofs48, false), n, nullptr, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_cell_proof_batch(const kzg_ctx* ctx, const uint8_t* commitments48, const uint64_t* cell_indices, const uint8_t* cells,
                                               const uint8_t* proofs48, uint64_t n, int32_t* ok) try {
  return batch_entry(ctx, cell_inputs(commitments48, cell_indices, cells, proofs48, true), n, nullptr, ok, nullptr);
} catch (...) {
  return abi_exception();
}

// ---- the row-indexed form: a block's list of u commitments and an index per item (include/kateth_amd.h) ------------------------------
// The cells kind with ncom = u in the session: the front reads the commitment through the index (k_cells_rows_leaves), the decoder runs
// on n + u points, lincomb B has n + u + 64 terms whose u commitment scalars are the weights w_c (k_cells_row_weights), and lincomb A's
// scalars r^k live in an array of their own.  Transcript, r and both sums are the per-cell call's on the expanded arrays.
// `each`: the per-item form's outputs (kzg_verify_cell_proof_batch_rows_each), null for the boolean call.
static int32_t rows_entry(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, const VerifyEach* each, int32_t* ok, hipStream_t st) {
  if (!ctx || !ok) return fail(KZG_FAIL_ARGUMENT, "null argument");
  if (n == 0) return empty_batch(ok);
  *ok = 0;
  if (!in.commitment_indices || !in.cell_indices || !in.cells || !in.proofs48 || (in.ncom && !in.commitments48) || (each && (!each->ok_each || !each->status)))
    return fail(KZG_FAIL_ARGUMENT, "null argument");
  if (in.ncom == 0) {  // every index is out of range: nothing is launched
    if (!each) return KZG_ERR_COMMITMENT_INDEX;
    for (uint64_t i = 0; i < n; i++) {
      each->status[i] = KZG_ERR_COMMITMENT_INDEX;
      each->ok_each[i] = 0;
    }
    return 0;
  }
  if (in.ncom >> 31) return fail(KZG_FAIL_ARGUMENT, "too many commitments");  // one workgroup column per commitment
  return batch_entry(ctx, in, n, each, ok, st);
}
extern "C" int32_t kzg_verify_cell_proof_batch_rows(const kzg_ctx* ctx, const uint8_t* commitments48, uint64_t u, const uint64_t* commitment_indices,
                                                    const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs48, uint64_t n, int32_t* ok) try {
  return rows_entry(ctx, cell_rows_inputs(commitments48, u, commitment_indices, cell_indices, cells, proofs48, true), n, nullptr, ok, nullptr);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_verify_cell_proof_batch_rows_dev(const kzg_ctx* ctx, const void* d_commitments48, uint64_t u, const void* d_commitment_indices,
                                                        const void* d_cell_indices, const void* d_cells, const void* d_proofs48, uint64_t n, int32_t* ok,
                                                        void* hip_stream) try {
  return rows_entry(ctx, cell_rows_inputs(d_commitments48, u, d_commitment_indices, d_cell_indices, d_cells, d_proofs48, false), n, nullptr, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

// Per-item verdicts of the row-indexed form: the rows session as it stands through each_finish.  What learns the indirection is the
// status fold (k_each_rows_status: the commitment's code through the item's index, the list's rejected entries counted beside) and the
// terms kernel (k_each_rows_terms: the commitment gathered out of the list); levels, vector tree, fetches and descent are the per-cell
// form's.  The challenge is the rows call's, which is the per-cell call's on the expanded arrays, so are both trees.
extern "C" int32_t kzg_verify_cell_proof_batch_rows_each(const kzg_ctx* ctx, const uint8_t* commitments48, uint64_t u, const uint64_t* commitment_indices,
                                                         const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs48, uint64_t n, uint8_t* ok_each,
                                                         int32_t* status, int32_t* commitment_status, int32_t* ok) try {
  const VerifyEach each{ok_each, status, commitment_status};
  return rows_entry(ctx, cell_rows_inputs(commitments48, u, commitment_indices, cell_indices, cells, proofs48, true), n, &each, ok, nullptr);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_verify_cell_proof_batch_rows_each_dev(const kzg_ctx* ctx, const void* d_commitments48, uint64_t u, const void* d_commitment_indices,
                                                             const void* d_cell_indices, const void* d_cells, const void* d_proofs48, uint64_t n, uint8_t* ok_each,
                                                             int32_t* status, int32_t* commitment_status, int32_t* ok, void* hip_stream) try {
  const VerifyEach each{ok_each, status, commitment_status};
  return rows_entry(ctx, cell_rows_inputs(d_commitments48, u, d_commitment_indices, d_cell_indices, d_cells, d_proofs48, false), n, &each, ok,
                    (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

// ---- the blob form: a blob's 128 cell proofs against the blob itself (include/kateth_amd.h) -------------------------------------------
// The row-indexed session with ncom = the blobs and n = 128 of them each, under another address map: the extension half goes into the
// session (k_compute_cells_ext, through cells_ext_enqueue), the front, k_cells_interp and the per-item kernels run as instances that
// take the item number for the pair of indices and read cells 0..63 out of the blob (cellv_blob_cell), the commitment scalars are
// 128-term segment sums (k_blob_weights).  Transcript, r and both sums are the rows call's on the expanded arrays.  `each`: the
// per-BLOB outputs of the *_each forms -- the status fold gives all 128 items of a blob its code (k_each_blob_status) and the descent
// stops at level 7.
static int32_t blob_cells_entry(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t nblobs, const VerifyEach* each, int32_t* ok, hipStream_t st) {
  if (!ctx || !ok) return fail(KZG_FAIL_ARGUMENT, "null argument");
  if (nblobs == 0) return empty_batch(ok);
  *ok = 0;
  if (in.any_null() || (each && (!each->ok_each || !each->status))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  // a cells session numbers its tree nodes, about two per item, in 32 bits
  if (nblobs >> 24) return fail(KZG_FAIL_ARGUMENT, "too many blobs: their 128 cells each exceed a cell verification session");
  const uint64_t n = nblobs * KZG_CELLS_PER_EXT_BLOB;
  if (in.on_host && is_group(ctx)) return each ? multi_verify_each(ctx, in, n, *each, ok) : multi_verify_batch(ctx, in, n, ok);
  return verify_batch_single(ctx, in, n, st, each, ok);
}
extern "C" int32_t kzg_verify_blob_cell_proofs_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* cell_proofs48, uint64_t n,
                                                     int32_t* ok) try {
  return blob_cells_entry(ctx, blob_cell_inputs(blobs, n, commitments48, cell_proofs48, true), n, nullptr, ok, nullptr);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_verify_blob_cell_proofs_batch_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_cell_proofs48, uint64_t n,
                                                         int32_t* ok, void* hip_stream) try {
  return blob_cells_entry(ctx, blob_cell_inputs(d_blobs, n, d_commitments48, d_cell_proofs48, false), n, nullptr, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_verify_blob_cell_proofs_batch_each(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* cell_proofs48,
                                                          uint64_t n, uint8_t* ok_each, int32_t* status, int32_t* ok) try {
  const VerifyEach each{ok_each, status};
  return blob_cells_entry(ctx, blob_cell_inputs(blobs, n, commitments48, cell_proofs48, true), n, &each, ok, nullptr);
} catch (...) {
  return abi_exception();
}
extern "C" int32_t kzg_verify_blob_cell_proofs_batch_each_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_cell_proofs48,
                                                              uint64_t n, uint8_t* ok_each, int32_t* status, int32_t* ok, void* hip_stream) try {
  const VerifyEach each{ok_each, status};
  return blob_cells_entry(ctx, blob_cell_inputs(d_blobs, n, d_commitments48, d_cell_proofs48, false), n, &each, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

// Introspection: the blob form's commitment scalars through phase 2's launch sequence -- k_batch_scalars for the powers, then
// k_blob_weights.  Scratch of its own, freed here; member 0 of a group.
extern "C" int32_t kzg_blob_cell_weights(const kzg_ctx* ctx, const uint8_t* r32, uint64_t first_index, uint64_t n_blobs, uint8_t* out_w32) try {
  if (!ctx || !r32 || (n_blobs && !out_w32)) return fail(KZG_FAIL_ARGUMENT, "null argument");
  fr_t r;
  fr_from_be_bytes_plain(r, r32);
  if (!fr_is_canonical(r)) return KZG_ERR_FF_NOT_IN_FIELD;
  if (n_blobs == 0) return 0;
  if (n_blobs >> 24) return fail(KZG_FAIL_ARGUMENT, "too many blobs");
  HIP_TRY(hipSetDevice(ctx->device));
  const uint64_t n = n_blobs * KZG_CELLS_PER_EXT_BLOB;
  const unsigned nblk = blocks_for(n, 256);
  Carve c;
  const size_t o_rpow2 = c.take(64 * sizeof(fr_t)), o_zero = c.take(n * sizeof(fr_t)), o_rk = c.take(n * sizeof(fr_t)), o_sb = c.take(n * sizeof(fr_t)),
               o_ysum = c.take(((size_t)nblk + 1) * sizeof(fr_t)), o_w = c.take((size_t)n_blobs * sizeof(fr_t));
  struct Scratch {
    uint8_t* p = nullptr;
    ~Scratch() {
      if (p) (void)hipFree(p);
    }
  } d;
  HIP_TRY(hipMalloc(&d.p, c.off));
  to_mont<FrParams>(r, r);
  fr_t rpow2[64];
  rpow2[0] = r;
  for (int k = 1; k < 64; k++) fr_sqr(rpow2[k], rpow2[k - 1]);
  hipStream_t st = nullptr;  // an introspection call, waited for here
  fr_t *d_rpow2 = (fr_t*)(d.p + o_rpow2), *d_zero = (fr_t*)(d.p + o_zero), *d_rk = (fr_t*)(d.p + o_rk), *d_sb = (fr_t*)(d.p + o_sb), *d_ysum = (fr_t*)(d.p + o_ysum),
       *d_w = (fr_t*)(d.p + o_w);
  HIP_TRY(hipMemcpyAsync(d_rpow2, rpow2, sizeof(rpow2), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_zero, 0, n * sizeof(fr_t), st));
  hipLaunchKernelGGL(k_batch_scalars, dim3(nblk), dim3(256), 0, st, d_rpow2, d_zero, d_zero, n, first_index, d_rk, d_sb, d_ysum);
  hipLaunchKernelGGL(k_blob_weights, dim3((unsigned)n_blobs), dim3(CELLV_BLOB_ITEMS), 0, st, d_rk, d_w);
  HIP_TRY(hipGetLastError());
  std::vector<fr_t> w(n_blobs);
  HIP_TRY(hipMemcpyAsync(w.data(), d_w, (size_t)n_blobs * sizeof(fr_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (uint64_t k = 0; k < n_blobs; k++) fr_to_be_bytes_plain(out_w32 + 32 * k, w[k]);
  return 0;
} catch (...) {
  return abi_exception();
}

// Introspection: the weights through phase 2's launch sequence -- k_batch_scalars (with z = y = 0: only its r^k are read), then
// k_cells_row_weights and its reduce launch.  Scratch of its own, freed here; member 0 of a group.
extern "C" int32_t kzg_cell_row_weights(const kzg_ctx* ctx, const uint8_t* r32, uint64_t first_index, const uint64_t* commitment_indices, uint64_t n, uint64_t u,
                                        uint8_t* out_w32) try {
  if (!ctx || !r32 || (n && !commitment_indices) || (u && !out_w32)) return fail(KZG_FAIL_ARGUMENT, "null argument");
  fr_t r;
  fr_from_be_bytes_plain(r, r32);
  if (!fr_is_canonical(r)) return KZG_ERR_FF_NOT_IN_FIELD;
  for (uint64_t k = 0; k < n; k++)
    if (commitment_indices[k] >= u) return KZG_ERR_COMMITMENT_INDEX;
  if (u == 0) return 0;
  if (n == 0) {
    memset(out_w32, 0, (size_t)u * 32);
    return 0;
  }
  if (u >> 31) return fail(KZG_FAIL_ARGUMENT, "too many commitments");
  HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t tiles = cellv_roww_tiles(n);
  const unsigned nblk = blocks_for(n, 256);
  Carve c;
  const size_t o_rpow2 = c.take(64 * sizeof(fr_t)), o_zero = c.take(n * sizeof(fr_t)), o_rk = c.take(n * sizeof(fr_t)), o_sb = c.take(n * sizeof(fr_t)),
               o_ysum = c.take(((size_t)nblk + 1) * sizeof(fr_t)), o_idx = c.take(n * 8), o_part = c.take((size_t)u * tiles * sizeof(fr_t)),
               o_w = c.take((size_t)u * sizeof(fr_t));
  struct Scratch {
    uint8_t* p = nullptr;
    ~Scratch() {
      if (p) (void)hipFree(p);
    }
  } d;
  HIP_TRY(hipMalloc(&d.p, c.off));
  to_mont<FrParams>(r, r);
  fr_t rpow2[64];
  rpow2[0] = r;
  for (int k = 1; k < 64; k++) fr_sqr(rpow2[k], rpow2[k - 1]);
  hipStream_t st = nullptr;  // an introspection call, waited for here
  fr_t *d_rpow2 = (fr_t*)(d.p + o_rpow2), *d_zero = (fr_t*)(d.p + o_zero), *d_rk = (fr_t*)(d.p + o_rk), *d_sb = (fr_t*)(d.p + o_sb), *d_ysum = (fr_t*)(d.p + o_ysum),
       *d_part = (fr_t*)(d.p + o_part), *d_w = (fr_t*)(d.p + o_w);
  unsigned long long* d_idx = (unsigned long long*)(d.p + o_idx);
  HIP_TRY(hipMemcpyAsync(d_rpow2, rpow2, sizeof(rpow2), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_idx, commitment_indices, n * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_zero, 0, n * sizeof(fr_t), st));
  hipLaunchKernelGGL(k_batch_scalars, dim3(nblk), dim3(256), 0, st, d_rpow2, d_zero, d_zero, n, first_index, d_rk, d_sb, d_ysum);
  {
    ProfScope ps(ctx, PROF_POLY, st);
    hipLaunchKernelGGL(k_cells_row_weights, dim3((unsigned)u, tiles), dim3(CELLV_ROWW_THREADS), 0, st, d_idx, (const int32_t*)nullptr, d_rk, n, cellv_roww_tile(n), d_part);
    hipLaunchKernelGGL(k_cells_roww_reduce, dim3(blocks_for(u, 256)), dim3(256), 0, st, d_part, tiles, u, d_w);
  }
  HIP_TRY(hipGetLastError());
  std::vector<fr_t> w(u);
  HIP_TRY(hipMemcpyAsync(w.data(), d_w, (size_t)u * sizeof(fr_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (uint64_t k = 0; k < u; k++) fr_to_be_bytes_plain(out_w32 + 32 * k, w[k]);
  return 0;
} catch (...) {
  return abi_exception();
}

// Per-item verdicts for cells: the third kind through the same driver (each_finish); what differs lies behind the session's kind --
// the order of the status arrays, the vector tree beside the two point trees, the fetch kernel and the pairing against [tau^64]_2.
extern "C" int32_t kzg_verify_cell_proof_batch_each_dev(const kzg_ctx* ctx, const void* d_commitments48, const void* d_cell_indices, const void* d_cells,
                                                        const void* d_proofs48, uint64_t n, uint8_t* ok_each, int32_t* status, int32_t* ok, void* hip_stream) try {
  const VerifyEach each{ok_each, status};
  return batch_entry(ctx, cell_inputs(d_commitments48, d_cell_indices, d_cells, d_proofs48, false), n, &each, ok, (hipStream_t)hip_stream);
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_cell_proof_batch_each(const kzg_ctx* ctx, const uint8_t* commitments48, const uint64_t* cell_indices, const uint8_t* cells,
                                                    const uint8_t* proofs48, uint64_t n, uint8_t* ok_each, int32_t* status, int32_t* ok) try {
  const VerifyEach each{ok_each, status};
  return batch_entry(ctx, cell_inputs(commitments48, cell_indices, cells, proofs48, true), n, &each, ok, nullptr);
} catch (...) {
  return abi_exception();
}

// Introspection: sum_j s_j [tau^j]_1 per 64-scalar vector THROUGH k_each_gather_cells -- the vectors stand where the vector tree's nodes
// do, no point trees (B' = identity), the bases not negated.  On a group context member 0 answers.  Scratch of its own, freed here.
extern "C" int32_t kzg_g1_monomial_lincomb(const kzg_ctx* ctx, const uint8_t* scalars32, uint64_t m, uint8_t* out96) try {
  if (!ctx || (m && (!scalars32 || !out96))) return fail(KZG_FAIL_ARGUMENT, "null argument");
  if (m == 0) return 0;
  std::vector<fr_t> vecs((size_t)m * 64);
  for (size_t k = 0; k < vecs.size(); k++) {
    fr_from_be_bytes_plain(vecs[k], scalars32 + 32 * k);
    if (!fr_is_canonical(vecs[k])) return KZG_ERR_FF_NOT_IN_FIELD;
  }
  const int32_t rc = ensure_g1_monomial(ctx);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  struct Scratch {
    fr_t* vec = nullptr;
    g1_xyzz* out = nullptr;
    ~Scratch() {
      if (vec) (void)hipFree(vec);
      if (out) (void)hipFree(out);
    }
  } d;
  const uint64_t chunk = std::min<uint64_t>(m, EACH_GATHER);
  HIP_TRY(hipMalloc(&d.vec, chunk * 64 * sizeof(fr_t)));
  HIP_TRY(hipMalloc(&d.out, 2 * chunk * sizeof(g1_xyzz)));
  hipStream_t st = nullptr;  // as the derivation of the points itself: an introspection call, waited for here
  std::vector<g1_xyzz> nodes(2 * chunk);
  for (uint64_t done = 0; done < m; done += chunk) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk, m - done);
    HIP_TRY(hipMemcpyAsync(d.vec, vecs.data() + done * 64, (size_t)cnt * 64 * sizeof(fr_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_each_gather_cells, dim3(cnt), dim3(64), 0, st, (const g1_xyzz28*)nullptr, (const g1_xyzz28*)nullptr, d.vec, ctx->d_g1_monomial,
                       (const uint32_t*)nullptr, cnt, false, d.out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(nodes.data(), d.out, 2 * (size_t)cnt * sizeof(g1_xyzz), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < cnt; k++) {
      host::g1_host_affine t;
      host_affine_from_xyzz(t, nodes[2 * k + 1]);
      host_affine_to_be96(out96 + 96 * (done + k), t);
    }
  }
  return 0;
} catch (...) {
  return abi_exception();
}

void launch_glv_points(hipStream_t st, uint4* aff, uint64_t npts, uint64_t phi_off) {
  if (npts) hipLaunchKernelGGL(k_glv_points, dim3(blocks_for(npts, 64)), dim3(64), 0, st, aff, npts, phi_off);
}

void warm_code_object_verify() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, (const void*)k_batch_ysum_finish);
  (void)hipGetLastError();
}
