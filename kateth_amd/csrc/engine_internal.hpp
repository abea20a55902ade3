// Shared by the engine translation units (engine.hip, engine_blob.hip, engine_proof.hip, engine_verify.hip, engine_multi.hip).  Besides the
// kernels below, engine.hip owns the context's pools -- the workspace slots (ws_*) and the host-buffer staging (stage_*, StageRing, and the
// HostCall driver that every host-buffer producer call runs through) -- and tears them down in kzg_ctx_destroy.
#pragma once
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/kateth_amd.h"
// Host-side headers only: field / curve types and single-source math, the comb's geometry, SHA-256, the host pairing.  Every
// KERNEL header is included by exactly one translation unit, which exports host launchers for what the others need (round 5:
// the library used to carry each kernel once per engine*.hip that included its header):
//   engine.hip        setup_kernels.cuh, msm_comb.cuh, msm_fixed.cuh   -> msm_launch / msm_finish / msm_pipeline
//   engine_blob.hip   blob_kernels.cuh (hash, point decoding, scalars) -> launch_challenge*, launch_g1_decompress*, launch_fr_*
//   engine_proof.hip  poly_kernels.cuh, cells_kernels.cuh, cellproof_kernels.cuh   (its only user)
//   engine_verify.hip verify_kernels.cuh, cellverify_kernels.cuh      (its only user)      -> launch_glv_points
#include "comb_geom.hpp"
#include "comb_balance.hpp"
#include "g1.cuh"
#include "sha256.cuh"
#include "pairing.hpp"
#include "verify_kind.hpp"

using namespace kzg;

int32_t fail(int32_t code, const std::string& msg);
// The handler of every int32_t entry point's function-try-block: an exception on its way out of the library (std::bad_alloc from a
// std::vector, std::system_error from a thread start) becomes KZG_FAIL_HOST with its text as kzg_last_error(); nothing unwinds
// into the caller's C frames.
int32_t abi_exception() noexcept;
const std::string& last_error_text();
// kzg_last_error / kzg_last_error_code are thread-local: work done on a helper thread hands its error to the calling thread
struct ErrorSnapshot {
  std::string text;
  int32_t detail = 0;
};
ErrorSnapshot error_snapshot();
void error_publish(const ErrorSnapshot& e);

// Persistent helper threads of the process (engine.hip): a job goes to an idle worker, or to a new one while fewer than the
// cap exist; `false` = no worker to be had, the caller runs the job itself.  Workers never block on other jobs' results, so nested
// use (a group call whose members each split their ending over two threads) cannot deadlock.  ADVICE r04: run_on_helpers used to
// start a std::thread per job -- thread creation and a first hipSetDevice on the latency path of every group call and of every
// single-item verification.
bool helper_dispatch(std::function<void()> fn);

// Runs job(k) for k < count: job 0 on the calling thread, the others on pooled helper threads (a job no helper can take runs
// inline: nothing throws across the C boundary).  Returns the first non-zero code in k order, with THAT job's error text
// re-published on the calling thread.
template <class Job>
static int32_t run_on_helpers(uint32_t count, Job&& job) {
  if (count == 0) return 0;
  std::vector<int32_t> rc(count, 0);
  std::vector<ErrorSnapshot> err(count);
  std::vector<char> handed(count, 0);
  std::mutex mu;
  std::condition_variable cv;
  uint32_t pending = 0;
  for (uint32_t k = 1; k < count; k++) {
    {
      std::lock_guard<std::mutex> g(mu);
      pending++;
    }
    bool ok = false;
    try {
      ok = helper_dispatch([&, k]() {
        rc[k] = job(k);
        if (rc[k]) err[k] = error_snapshot();
        std::lock_guard<std::mutex> g(mu);  // notified under the lock: the waiter cannot destroy `cv` before this returns
        pending--;
        cv.notify_one();
      });
    } catch (...) {  // std::bad_alloc building the closure
    }
    if (ok) {
      handed[k] = 1;
    } else {
      std::lock_guard<std::mutex> g(mu);
      pending--;
    }
  }
  rc[0] = job(0);
  if (rc[0]) err[0] = error_snapshot();
  for (uint32_t k = 1; k < count; k++)
    if (!handed[k]) {
      rc[k] = job(k);
      if (rc[k]) err[k] = error_snapshot();
    }
  {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return pending == 0; });
  }
  for (uint32_t k = 0; k < count; k++)
    if (rc[k]) {
      error_publish(err[k]);
      return rc[k];
    }
  return 0;
}

#define HIP_TRY(expr)                                                                                      \
  do {                                                                                                     \
    hipError_t _e = (expr);                                                                                \
    if (_e != hipSuccess) return fail(KZG_FAIL_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));  \
  } while (0)

// Environment knobs are read ONCE, at kzg_ctx_create, into the context -- never on a call path.
struct EnvKnobs {
  bool trace = false;            // KATETH_AMD_TRACE
  uint64_t proof_chunk = 0;      // KATETH_AMD_PROOF_CHUNK (0 = default)
  int proof_overlap = -1;        // KATETH_AMD_PROOF_OVERLAP (-1 = default)
  int eval_group = 0;            // KATETH_AMD_EVAL_GROUP: 16 | 64 (0 = automatic)
  bool verify_serial = false;    // KATETH_AMD_VERIFY_SERIAL
  bool single_via_batch = false; // KATETH_AMD_SINGLE_VIA_BATCH: a single-item verification takes the batch machinery (the cross-check of the host lincomb)
  bool var_glv = false;          // KATETH_AMD_VAR_GLV=1: both lincombs of a batch of >= 32,768 items take their scalars GLV-split (built, measured and
                                 // NOT adopted in round 5: +0.2 ms per 65,536 triples, profiles/r05/verify_glv_rejected.json; kept as an independent cross-check)
  uint32_t var_seg = 1;          // 1 = on, share size chosen by the engine; >= 2: that many entries per lane (tuning sweeps); KATETH_AMD_VAR_SEG=0: the flat path's bucket sums with one thread per bucket (k_var_buckets_flat) instead of equal shares of
                                 // the sorted entry list per lane (k_var_buckets_seg): the cross-check of the balanced kernel
  bool var_msm_classic = false;  // KATETH_AMD_VAR_MSM=classic: c = 8 with per-bucket partials for every batch size (cross-check of the flat path)
  uint64_t verify_chunk = 0;     // KATETH_AMD_VERIFY_CHUNK: blobs per host-buffer staging chunk (0 = default)
  uint32_t verify_streams = 0;   // KATETH_AMD_VERIFY_STREAMS: compute streams the host-buffer verification rotates its chunks over (1..4; 0 = default)
  uint32_t comb_fair = 20;       // KATETH_AMD_COMB_FAIR=s: the MSM waves of a SIMD trade issue priority every 2^s cycles; 0 = hardware default (measurement aid)
  bool lat_table = true;         // KATETH_AMD_LAT_TABLE=0: no latency comb beside a class-22 table (measurement aid)
  bool comb_full_wave = false;   // KATETH_AMD_COMB_FULL_WAVE: never use the comb's two-blobs-per-wave mode (measurement aid)
  bool comb_half_wave = false;   // KATETH_AMD_COMB_HALF_WAVE=1: two blobs per wave from two blobs on, not only where msm_shape finds it cheaper (tests of the half-wave paths at small batches)
  int comb_balance = 1;          // KATETH_AMD_COMB_BALANCE=off|auto|<partner>:<shed> -> 0 | 1 | 2: the balance plan of half-wave launches (comb_balance.hpp); 2 = comb_balance_forced on every
  CombBalance comb_balance_forced = comb_balance_none();  // launch it is valid for (tests, A/B runs)
  uint32_t msm_splits = 0;       // KATETH_AMD_MSM_SPLITS: force the (blob, split) decomposition of the fixed-base MSM (power of two <= 64; 0 = automatic)
  uint64_t challenge_split_max = 0;  // KATETH_AMD_CHALLENGE_SPLIT_MAX: largest batch hashed by the two-wave SHA-256 kernel (0 = default)
  uint64_t sidecar_pass = 0;     // KATETH_AMD_SIDECAR_PASS: blobs per staging pass of kzg_blob_sidecar_batch (0 = the plan of the host-buffer proof call)
  uint64_t cells_pass = 0;       // KATETH_AMD_CELLS_PASS: items per staging pass of kzg_compute_cells_batch and kzg_recover_cells_batch (0 = default)
  uint64_t cellproof_pass = 0;   // KATETH_AMD_CELLPROOF_PASS: items per pass of the cell-proof calls, on the device and through the staging ring (0 = default: 32)
};
EnvKnobs read_env_knobs();

struct TraceTimer {  // KATETH_AMD_TRACE=1: host-side wall-clock marks on stderr
  bool on;
  std::chrono::steady_clock::time_point t0;
  const char* what;
  TraceTimer(bool enabled, const char* w) : on(enabled), t0(std::chrono::steady_clock::now()), what(w) {}
  void mark(const char* label) {
    if (!on) return;
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[kateth_amd trace] %s: %s +%.3f ms\n", what, label, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

constexpr int KZG_STAGE_SLOTS = 4;    // x up to 4,096 blobs x 128 KiB = 2 GiB of staging at most
constexpr int KZG_STAGE_STREAMS = 4;  // per-chunk kernels rotate over these (a chunk's SHA-256 streams are latency-bound: several in flight)
#define KZG_SESSION_STREAM (reinterpret_cast<hipStream_t>(static_cast<intptr_t>(-1)))  // session_acquire: run on the session's own stream
enum ProfKind { PROF_MSM_FIXED = 0, PROF_CHALLENGE, PROF_EVAL, PROF_DECODE, PROF_POLY, PROF_VAR_MSM, PROF_REDUCE_COMPRESS, PROF_TRANSPOSE, PROF_KINDS };
static_assert(PROF_KINDS == KZG_PROF_KINDS, "include/kateth_amd.h and ProfKind disagree");
struct ProfEvent {
  int kind;
  hipEvent_t e0, e1;
};

struct kzg_verify_session;
struct kzg_ctx;
constexpr int KZG_WS_SLOTS = 3;
struct WsSlot {
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;  // recorded after the last enqueued user of the slot; the next user's stream waits on it
  hipStream_t last_st = nullptr;  // the stream of that user: a call on the SAME stream is ordered behind it anyway and reuses the slot
  bool used = false;
};
// Extension point for the TEST-ONLY library (tests/window_msm/window_msm.hip = the product objects + one more translation
// unit): an alternative fixed-base MSM -- round 1's window-table kernels as independent cross-checks of the comb, and a
// time-stamping instance of the comb kernel.  The product library never sets g_msm_override_hook: kzg_ctx_create then has one
// path, and none of that code is in kateth_amd/csrc.
struct MsmOverride {
  const char* kernel_name;
  bool replaces_table;     // true: build() fills ctx->d_table / table_bytes / window_class instead of the comb build
  uint64_t adds_per_blob;  // reported by kzg_ctx_adds_per_blob when the table is replaced
  int32_t (*build)(kzg_ctx* ctx);
  // the MSM alone: 64 lane sums per (blob, split) unit into partials[unit * 64 + lane]; scratch = msm_scratch_bytes(ctx, n) bytes
  int32_t (*launch)(const kzg_ctx* ctx, bool be_bytes, const uint8_t* d_scalars, uint64_t n, int32_t* d_status, g1_xyzz* partials, uint32_t splits,
                    uint32_t lpb, void* scratch, hipStream_t st);
  void (*destroy)(kzg_ctx* ctx);
};
extern const MsmOverride* (*g_msm_override_hook)(kzg_ctx* ctx, uint32_t window_bits);  // nullptr in the product library

// The fixed-base tables a context computes with: the main comb, (class 22) the latency comb, their constant terms.
struct CombTables {
  CombGeom comb{}, comb_lat{};
  uint4 *d_table = nullptr, *d_table_lat = nullptr, *d_comb_k = nullptr, *d_comb_k_lat = nullptr;
  uint64_t table_bytes = 0;
  uint32_t window_class = 0;
};
struct TableChoice {  // a candidate (class, plane groups) of the automatic ladder and the free HBM it asks for
  uint32_t c, G;
  size_t need;
};

struct kzg_ctx {
  int device = 0;
  // GROUP context (kzg_config.ndev != 0): this context is member 0, `peers` are the members on the other listed devices
  // (owned, single-device contexts).  The host-buffer entry points shard over {this, peers...} (engine_multi.hip).
  std::vector<kzg_ctx*> peers;
  mutable std::atomic<uint32_t> rr{0};  // calls with fewer items than members start at a rotating member
  // KZG_CFG_BUILD_ASYNC: the chosen table is built by `build_thread` and swapped in under `lock`; the tables it replaces
  // stay allocated until kzg_ctx_destroy (launches already enqueued may still read them)
  std::thread build_thread;
  std::atomic<bool> build_cancel{false};
  mutable std::mutex build_mu;
  mutable std::condition_variable build_cv;
  bool build_running = false;  // guarded by build_mu
  int32_t build_rc = 0;
  ErrorSnapshot build_err;
  std::vector<CombTables> retired;
  uint4* d_table = nullptr;      // fixed-base comb table (msm_comb.cuh): comb_table_entries(comb) * 96 B
  bool use_comb = true;          // false only under a test override that replaces the table
  CombGeom comb{};
  const MsmOverride* msm_override = nullptr;  // test-only library, see above
  void* override_state = nullptr;
  // class 22 only: a second, small comb for latency (blocks of 8 points, 64 plane groups of 4 planes: 3 doublings per lane
  // instead of 31, 403 MB) used by calls of at most KZG_LAT_MAX_BLOBS blobs, where a lane's chain -- not the chip -- is the cost
  CombGeom comb_lat{};
  uint4* d_table_lat = nullptr;
  // the comb's constant term K = [(2^256-1)/2] * (sum of the setup points) as the STARTING VALUE of one lane per blob: that lane
  // doubles its accumulator H - 1 times, so the stored point is [c0 / 2^(H-1)] S (affine, table format: packed centred 30-bit digits of x * 2^390, 96 B -- fp30.cuh;
  // null = identity), one per table geometry
  uint4* d_comb_k = nullptr;
  uint4* d_comb_k_lat = nullptr;
  uint32_t window_class = 0;     // what kzg_ctx_window_bits reports
  uint4* d_bases_brp = nullptr;  // 4096 affine Lagrange points, BRP order
  fr_t* d_roots_brp = nullptr;   // 4096 roots of unity, Montgomery, BRP order
  uint32_t* d_eval_tab = nullptr;  // 256 hexes x twenty 9-limb slots in radix-2^29 limbs (layout: fr29.cuh; k_eval_frac, verify_kernels.cuh)
  uint32_t* d_cells_tab = nullptr;  // compute_cells' twiddles: 12,288 entries of twelve dwords (layout: cells_math.cuh; k_compute_cells, cells_kernels.cuh)
  uint32_t* d_recover_tab = nullptr;  // recover_cells' twists, omega_128 powers and coset points: 12,480 such entries (layout: recover_math.cuh; k_recover_cells)
  uint32_t* d_cellv_tab = nullptr;  // cell verification's h_c^-j / 64: 8,192 such entries (layout: cellverify_math.cuh; k_cells_interp, cellverify_kernels.cuh)
  fr_t* d_cellv_h64 = nullptr;  // h_c^64 of the 128 columns, plain: z of a cell in the batched check (k_cells_leaves)
  // The first 64 monomial setup points [tau^j]_1, derived as the commitments of the blobs of X^j (ensure_g1_monomial, engine.hip) by the
  // context's FIRST cell verification or kzg_ctx_g1_monomial call -- not at kzg_ctx_create: a context that never verifies cells launches and
  // holds nothing for them.  64 affine points as lincomb B reads them (2^392-Montgomery, the decoder's output), their 64 [z^2]-images behind
  // them (GLV route), and the 48-byte encodings for kzg_ctx_g1_monomial; written once under g1_monomial_mu, then read-only.
  mutable std::mutex g1_monomial_mu;
  mutable std::atomic<bool> g1_monomial_ready{false};
  mutable uint4* d_g1_monomial = nullptr;
  mutable uint8_t g1_monomial48[KZG_G1_MONOMIAL_POINTS * 48] = {};
  // cell proofs' omega_128 powers: 128 such entries (layout: cellproof_math.cuh; k_cell_quotients), built by the context's first cell-proof call
  // (ensure_cellproof_tab, engine_proof.hip); written once under cellproof_mu, then read-only
  mutable std::mutex cellproof_mu;
  mutable std::atomic<bool> cellproof_ready{false};
  mutable uint32_t* d_cellproof_tab = nullptr;
  mutable std::atomic<uint64_t> cellproof_vectors{0};  // quotient vectors committed by the cell-proof calls so far, by launch size (kzg_ctx_cellproof_vectors)
  // Pinned host buffers of the select calls' pair lists (engine_proof.hip: pair_pin_take), guarded by `lock`.  A *_dev call fills one on
  // the host, enqueues its upload and returns: the buffer is the call's until `ev`, recorded behind that copy, has completed.
  struct PairPin {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
  };
  mutable std::vector<PairPin> pair_pins;
  uint4* d_gen_affine = nullptr; // G1 generator and its [z^2]-image (GLV cross-check path), affine, 2^392-Montgomery (2 x 96 B): a term of batch verification's second lincomb
  host::pairing_ctx* pairing = nullptr;  // host: Frobenius constants + Miller lines of G2 and [tau]_2
  uint64_t table_bytes = 0;
  uint32_t num_cus = 256;
  hipStream_t side_stream = nullptr;  // non-blocking stream for work that overlaps the caller's stream
  hipStream_t copy_stream = nullptr;  // non-blocking stream for the chunked host-to-device copies of the host-buffer entry points
  EnvKnobs knobs;  // read once at kzg_ctx_create
  // Balance of the comb's half-wave launches (msm_launch / msm_finish, engine.hip; comb_balance.hpp), guarded by bal_lock.  Every
  // launch that fills most of one round takes the next sequence number and with it one of KZG_BAL_RING device records, which its
  // waves fold their times into and its lane-sum kernel forwards to the pinned ring entry of the same index; the host remembers
  // what it issued there.  The next such launch takes the newest entry that is complete (both sequence words, all units
  // reported) -- it never waits for one -- and, with KATETH_AMD_COMB_BALANCE=auto, moves bal_plan by it.  Each launch carries its
  // own copy of the plan by value, so calls in flight on several streams do not see each other's.
  static constexpr uint32_t KZG_BAL_RING = 16;
  struct BalIssued {
    uint64_t seq = 0, units = 0;
    uint32_t total = 0, bpo = 0;
    CombBalance ran = comb_balance_none();
  };
  mutable std::mutex bal_lock;
  mutable CombBalance bal_plan = comb_balance_none();
  mutable uint64_t bal_seq = 0;   // records issued so far
  mutable uint64_t bal_seen = 0;  // newest record taken
  mutable BalIssued bal_issued[KZG_BAL_RING];
  mutable unsigned long long bal_last[COMB_REC_WORDS + 2] = {};  // that record: its sequence number, the COMB_REC_ words, its units (kzg_ctx_comb_balance)
  mutable CombBalance bal_last_ran = comb_balance_none();
  unsigned long long* d_bal_rec = nullptr;  // KZG_BAL_RING x COMB_REC_WORDS, cleared by the kernel that forwards them
  unsigned long long* h_bal_msg = nullptr;  // pinned: KZG_BAL_RING x {seq, COMB_REC_WORDS, seq}
  // workspace (grown on demand, guarded by lock)
  mutable std::mutex lock;
  // KZG_WS_SLOTS workspaces for commitment / proof calls: a call takes the LOWEST slot whose previous user has completed or ran
  // on the call's own stream (a caller that runs one call at a time, or queues its calls on one stream, lives in slot 0, and only
  // slot 0 is ever allocated), else the slots in turn; its
  // stream waits for the previous user of ITS slot only, so calls enqueued on several streams run side by side (one call's
  // hash and quotient kernels in the shadow of the other's MSM) instead of queueing behind one shared buffer.  Each slot
  // grows by itself, to the largest call it has served.
  mutable WsSlot wss[KZG_WS_SLOTS];
  mutable uint32_t ws_next = 0;  // next slot in turn when every slot is busy
  mutable uint32_t ws_cur = 0;   // slot of the call being enqueued (between ws_begin and ws_end, under `lock`)
  mutable std::vector<hipEvent_t> proof_events;  // pooled fork/join events of the proof path's chunk pipeline (guarded by lock)
  // profiling (kzg_profile_begin/end): event pairs around the launches of the kernels named by ProfKind, each pair on the
  // stream its kernel runs on; own lock (the verify entry points do not take `lock`)
  mutable std::mutex prof_lock;
  mutable std::atomic<bool> profiling{false};  // read without prof_lock by ProfScope on every launch
  mutable std::vector<ProfEvent> prof_events;
  mutable size_t prof_used = 0;
  mutable unsigned long long* d_clock_probe = nullptr;  // kzg_clock_probe_launch / _read (guarded by prof_lock)
  mutable hipStream_t probe_stream = nullptr;
  // pooled verify sessions (device scratch + side stream + events), engine_verify.hip
  mutable std::mutex pool_lock;
  mutable std::vector<kzg_verify_session*> session_pool;
  mutable std::atomic<uint64_t> each_checks{0};  // pairing checks spent by the per-item verdict calls so far (kzg_verify_each_checks)
  mutable std::atomic<uint64_t> sessions_created{0};  // sessions constructed so far; a steady state creates none (kzg_ctx_sessions_created)
  // host-buffer pipelines (verification, evaluation: engine_verify.hip; commitments: engine.hip; proofs: engine_proof.hip), guarded by
  // stage_lock, so that a steady-state host-buffer call allocates nothing: a staging arena of up to
  // KZG_STAGE_SLOTS chunk slots, a copy stream, rotating compute streams and their events; created on first use (StageRing)
  mutable std::mutex stage_lock;
  mutable uint8_t* stage = nullptr;
  mutable size_t stage_bytes = 0;
  mutable uint8_t* hostio = nullptr;  // pooled device buffers for the small inputs/outputs of the host-buffer commit/proof calls (48-96 B per item)
  mutable size_t hostio_bytes = 0;
  mutable bool stage_ready = false;
  mutable hipStream_t verify_stream = nullptr, stage_copy_stream = nullptr, stage_streams[KZG_STAGE_STREAMS] = {};
  mutable hipEvent_t stage_copied[KZG_STAGE_SLOTS] = {}, stage_done[KZG_STAGE_SLOTS] = {}, stage_join[KZG_STAGE_STREAMS] = {};
};
void session_pool_clear(const kzg_ctx* ctx);

// ---- single-device implementations behind the host-buffer entry points.  The extern "C" producers reach them through on_members, which
// hands a group's call to engine_multi.hip; the verification calls shard over a group in engine_multi.hip (multi_verify_*) ----
static inline bool is_group(const kzg_ctx* ctx) { return ctx && !ctx->peers.empty(); }
constexpr size_t KZG_BYTES_PER_CELL_SET = (size_t)KZG_CELLS_PER_EXT_BLOB * KZG_BYTES_PER_CELL;  // the 128 cells of one extended blob
int32_t ctx_create_single(const uint8_t* g1_lagrange, const uint8_t* g2_monomial, const kzg_config* cfg, int device, kzg_ctx** out);  // engine.hip
int32_t commit_host(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out48, uint8_t* out_affine96, int32_t* status);    // engine.hip
int32_t proof_host(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* side, size_t side_bytes, bool side_is_commitment, uint64_t n, uint8_t* out48,
                   uint8_t* out_affine96, uint8_t* out_y32, int32_t* status);  // engine_proof.hip
int32_t sidecar_host(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_commitments48, uint8_t* out_proofs48, uint8_t* out_versioned_hashes32,
                     int32_t* status);  // engine_proof.hip
// One cell call (EIP-7594) over n items, all of it in the caller's host buffers (das_host) or all of it device-resident (das_dev):
//   in            the blobs (131,072 bytes per item), or with `present` the cell sets (262,144)
//   present       16-byte masks: recover the absent cells; null: compute the cells of blobs
//   out_cells     the 128 cells of every item; null (compute with proofs only): no cells wanted
//   out_proofs48  the 128 proofs of every item, 6,144 bytes; null: cells only -- the call takes neither ctx->lock nor a workspace slot
//   want          HOST memory in either form, 16-byte masks: the select calls -- only the wanted proofs are computed and written, the rest
//                 of out_proofs48 stays as the caller laid it down; null: the full call
struct CellCall {
  const uint8_t *in, *present;
  uint8_t *out_cells, *out_proofs48;
  int32_t* status;
  const uint8_t* want = nullptr;
  CellCall advanced(uint64_t first) const {  // the same call from item `first` on
    return CellCall{in + first * (present ? KZG_BYTES_PER_CELL_SET : (size_t)KZG_BYTES_PER_BLOB), present ? present + first * 16 : nullptr,
                    out_cells ? out_cells + first * KZG_BYTES_PER_CELL_SET : nullptr,
                    out_proofs48 ? out_proofs48 + first * (KZG_CELLS_PER_EXT_BLOB * 48) : nullptr, status + first, want ? want + first * 16 : nullptr};
  }
};
int32_t das_host(const kzg_ctx* ctx, const CellCall& call, uint64_t n);                // engine_proof.hip
int32_t das_dev(const kzg_ctx* ctx, const CellCall& call, uint64_t n, hipStream_t st);  // engine_proof.hip
int32_t verify_proof_single(const kzg_ctx* ctx, const uint8_t* proof48, const uint8_t* commitment48, const uint8_t* z32, const uint8_t* y32, int32_t* ok);
int32_t g1_decompress_single(const kzg_ctx* ctx, const uint8_t* in48, uint64_t n, uint8_t* out_affine96, int32_t* status);
int32_t evaluate_blobs_single(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* z32, uint64_t n, uint8_t* out_y32, int32_t* status);
// engine_multi.hip
int32_t group_create(const uint8_t* g1_lagrange, const uint8_t* g2_monomial, const kzg_config* cfg, kzg_ctx** out);
int32_t multi_verify_proof(const kzg_ctx* ctx, const uint8_t* proof48, const uint8_t* commitment48, const uint8_t* z32, const uint8_t* y32, int32_t* ok);
// The member dispatch of the producer calls: fn(member, first, count) once per share of the n items, each share on its member's own host
// thread, the first failing share's code and text returned (run_on_helpers); a call of fewer items than members starts at a rotating
// member.  `fn` advances the caller's pointers to item `first` and calls the single-device implementation on `member`.  A single-device
// context is its own only member: fn(ctx, 0, n) on the calling thread, with no shares, no helper thread and no allocation.
using MemberCall = std::function<int32_t(const kzg_ctx* member, uint64_t first, uint64_t count)>;
int32_t on_group_members(const kzg_ctx* ctx, uint64_t n, const MemberCall& fn);
template <class Fn>
static inline int32_t on_members(const kzg_ctx* ctx, uint64_t n, Fn&& fn) {
  return is_group(ctx) ? on_group_members(ctx, n, std::ref(fn)) : fn(ctx, (uint64_t)0, n);
}
// The inputs of one batch verification call, in the caller's host buffers (`on_host`) or device-resident.  What the kinds differ in --
// the error record among it -- is verify_kind.hpp's table:
//   BLOBS  (verify_blob_proof_batch): blobs, commitments48, proofs48
//   POINTS (verify_proof_batch):      proofs48, commitments48, z32, y32
//   CELLS  (verify_cell_proof_batch): commitments48, cell_indices, cells, proofs48
using VerifyKind = kzg::verify::Kind;
using kzg::verify::facts;
static_assert(facts(VerifyKind::CELLS).tail_terms == KZG_G1_MONOMIAL_POINTS, "lincomb B's fixed terms of the cells kind are the context's monomial points");
struct VerifyInputs {
  VerifyKind kind;
  const uint8_t *blobs, *commitments48, *proofs48, *z32, *y32;
  bool on_host;
  const uint64_t* cell_indices = nullptr;
  const uint8_t* cells = nullptr;
  // CELLS, the row-indexed form (kzg_verify_cell_proof_batch_rows): commitments48 is a LIST of ncom points and item k's commitment is
  // entry commitment_indices[k] of it.  Null: the per-cell form, one commitment per item.
  const uint64_t* commitment_indices = nullptr;
  uint64_t ncom = 0;
  // CELLS, the blob form (kzg_verify_blob_cell_proofs_batch): the row-indexed form with IMPLICIT indices over `blobs` -- ncom blobs, one
  // commitment each, 128 ncom items; item i is cell i & 127 of blob i >> 7.  No index array and no cell array exists: cells 0..63 are
  // the blob's bytes, cells 64..127 the session's extension workspace.
  bool from_blobs = false;
  bool rows() const { return commitment_indices != nullptr || from_blobs; }
  bool any_null() const {
    if (from_blobs) return !commitments48 || !proofs48 || !blobs;
    return !commitments48 || !proofs48 || (kind == VerifyKind::BLOBS ? !blobs : kind == VerifyKind::POINTS ? (!z32 || !y32) : (!cell_indices || !cells));
  }
  VerifyInputs blob_share(uint64_t first_blob, uint64_t count) const {  // `count` blobs of the blob form from blob `first_blob` on: every array advances
    VerifyInputs a = *this;
    a.ncom = count;
    a.blobs = blobs + first_blob * (size_t)KZG_BYTES_PER_BLOB;
    a.commitments48 = commitments48 + first_blob * 48;
    a.proofs48 = proofs48 + first_blob * (size_t)(KZG_CELLS_PER_EXT_BLOB * 48);
    return a;
  }
  VerifyInputs advanced(uint64_t first) const {  // the same inputs from item `first` on (the row-indexed form's commitment list stays whole)
    VerifyInputs a{kind, blobs ? blobs + first * (size_t)KZG_BYTES_PER_BLOB : nullptr, rows() ? commitments48 : commitments48 + first * 48, proofs48 + first * 48,
                   z32 ? z32 + first * 32 : nullptr, y32 ? y32 + first * 32 : nullptr, on_host};
    a.cell_indices = cell_indices ? cell_indices + first : nullptr;
    a.cells = cells ? cells + first * (size_t)KZG_BYTES_PER_CELL : nullptr;
    a.commitment_indices = rows() ? commitment_indices + first : nullptr;
    a.ncom = ncom;
    return a;
  }
};
static inline VerifyInputs blob_inputs(const void* blobs, const void* commitments48, const void* proofs48, bool on_host) {
  return VerifyInputs{VerifyKind::BLOBS, (const uint8_t*)blobs, (const uint8_t*)commitments48, (const uint8_t*)proofs48, nullptr, nullptr, on_host};
}
static inline VerifyInputs point_inputs(const void* proofs48, const void* commitments48, const void* z32, const void* y32, bool on_host) {
  return VerifyInputs{VerifyKind::POINTS, nullptr, (const uint8_t*)commitments48, (const uint8_t*)proofs48, (const uint8_t*)z32, (const uint8_t*)y32, on_host};
}
static inline VerifyInputs cell_inputs(const void* commitments48, const void* cell_indices, const void* cells, const void* proofs48, bool on_host) {
  VerifyInputs in{VerifyKind::CELLS, nullptr, (const uint8_t*)commitments48, (const uint8_t*)proofs48, nullptr, nullptr, on_host};
  in.cell_indices = (const uint64_t*)cell_indices;
  in.cells = (const uint8_t*)cells;
  return in;
}
static inline VerifyInputs cell_rows_inputs(const void* commitments48, uint64_t ncom, const void* commitment_indices, const void* cell_indices, const void* cells,
                                            const void* proofs48, bool on_host) {
  VerifyInputs in = cell_inputs(commitments48, cell_indices, cells, proofs48, on_host);
  in.commitment_indices = (const uint64_t*)commitment_indices;
  in.ncom = ncom;
  return in;
}
static inline VerifyInputs blob_cell_inputs(const void* blobs, uint64_t n_blobs, const void* commitments48, const void* cell_proofs48, bool on_host) {
  VerifyInputs in{VerifyKind::CELLS, (const uint8_t*)blobs, (const uint8_t*)commitments48, (const uint8_t*)cell_proofs48, nullptr, nullptr, on_host};
  in.from_blobs = true;
  in.ncom = n_blobs;
  return in;
}
// the blob form's way to k_compute_cells_ext (cells_kernels.cuh is compiled once, in engine_proof.hip): cells 64..127 of n blobs to
// d_out_ext (131,072 bytes per blob) and the blobs' statuses, enqueued on `st`
int32_t cells_ext_enqueue(const kzg_ctx* ctx, const uint8_t* d_blobs, uint64_t n, uint8_t* d_out_ext, int32_t* d_status, hipStream_t st);
// the wanted ending of a batch call: one boolean (no VerifyEach), or the per-item verdicts of kzg_verify_*_batch_each beside it (the
// blob form of the cells kind: per BLOB, ncom entries each)
struct VerifyEach {
  uint8_t* ok_each;
  int32_t* status;
  // the row-indexed cells form (kzg_verify_cell_proof_batch_rows_each) only: the decoder's code per LISTED commitment (ncom words), or
  // null for a caller who does not ask -- a rejected listed commitment makes the call's *ok 0 either way
  int32_t* commitment_status = nullptr;
};
// The single-device batch call behind every route -- {blobs, points} x {host buffers, device pointers} x {one boolean, per-item verdicts};
// n >= 1, `st`: the caller's stream of the device routes -- and phase 1 alone, whose session becomes the caller's (engine_verify.hip).
int32_t verify_batch_single(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, hipStream_t st, const VerifyEach* each, int32_t* ok);
int32_t verify_phase1(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, hipStream_t st, uint8_t* out_root32, int32_t* err, kzg_verify_session** session);
// the same over a group's members, from host buffers (engine_multi.hip)
int32_t multi_verify_batch(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, int32_t* ok);
int32_t multi_verify_each(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, const VerifyEach& each, int32_t* ok);
// the context's monomial G1 points stand (derived by the first caller, engine.hip); every cells session of a member passes through here
int32_t ensure_g1_monomial(const kzg_ctx* ctx);
// kzg_verify_batch_finish with the pairing of `kind`: the summed partials against [tau]_2 or [tau^64]_2 (engine_verify.hip)
int32_t verify_batch_finish(const kzg_ctx* ctx, const uint8_t* partials192, uint64_t world, VerifyKind kind, int32_t* ok);
// one member's device-resident share of a group verification (kzg_verify_*_batch_group_dev): global range [first, first + count),
// inputs resident on member->device
struct GroupDevShare {
  const kzg_ctx* member;
  VerifyInputs in;
  uint64_t first, count;
  hipStream_t st;
};
int32_t verify_group_dev(const kzg_ctx* ctx, const std::vector<GroupDevShare>& shares, uint64_t n_total, int32_t* ok);  // engine_verify.hip
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct Carve {  // hands out 256-byte aligned offsets into a pooled buffer; `off` = the bytes asked of the pool so far
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; }
};
// ---- host-buffer staging (engine.hip), all of it with ctx->stage_lock held ----
int32_t stage_init(const kzg_ctx* ctx);                                          // streams and events, on first use
int32_t stage_reserve(const kzg_ctx* ctx, size_t arena_bytes, size_t io_bytes);  // the arena and the host-i/o pool only grow
void stage_drain(const kzg_ctx* ctx);  // verify_phase1_host's failure path: the host waits for the copy stream and every stage stream
void stage_destroy(const kzg_ctx* ctx);
// record `ev` on `signaller`, then `waiter` waits for it
int32_t stream_after(hipStream_t waiter, hipStream_t signaller, hipEvent_t ev);
// The slot protocol of the host-buffer pipelines, stated once.  Its users are HostCall (below: the producer calls) and
// verify_phase1_host (engine_verify.hip).
// The caller's blobs cross PCIe in chunks through `slots` equal slots of the context's staging arena; chunk k lives in slot k % slots:
//   feed(k)      the copy stream waits for the slot's previous consumer (done_event(k - slots), when k >= slots), copies the chunk in and
//                records the slot's `copied` event, for which `comp` -- the stream the caller enqueues the chunk's work on -- waits;
//   consumed(k)  records done_event(k) on `comp` behind that work.  A consumer that is done with the slot earlier records done_event(k)
//                itself (msm_launch's scalars_consumed).
// Streams are ordered by events only: the host never waits.  `overlap` = false (a plan of ONE chunk: nothing to overlap): the copy rides
// on `comp` itself and stream order does it all -- every event between two streams is a packet on one hardware queue waiting for a signal
// from another (~0.1 ms each with a queue per stream).
// overlap = false requires a single compute stream: every feed() of the call names the same `comp`.
struct StageRing {
  const kzg_ctx* ctx = nullptr;
  uint64_t slots = 1;
  size_t slot_bytes = 0;
  bool overlap = true;
  int32_t open(const kzg_ctx* c, uint64_t nslots, size_t bytes_per_slot, size_t io_bytes, bool overlap_copies);  // stage_init + stage_reserve
  int32_t feed(uint64_t k, const uint8_t* host_src, size_t bytes, hipStream_t comp, uint8_t** d_chunk);
  // feed() of a chunk that lies in the caller's memory as `height` runs of `width` bytes, host_pitch apart; it arrives packed (pitch = width)
  int32_t feed_pitched(uint64_t k, const uint8_t* host_src, size_t host_pitch, size_t width, size_t height, hipStream_t comp, uint8_t** d_chunk);
  hipEvent_t done_event(uint64_t k) const;
  int32_t consumed(uint64_t k, hipStream_t comp);
};

// The driver of a host-buffer producer call on one device (commit_host; proof_host, sidecar_host, das_host; evaluate_blobs_single,
// g1_decompress_single: six implementations under thirteen entry points), which owns the call's StageRing:
//   upload / download / scratch   register the call's small per-item arrays in the host-i/o pool by host pointer and byte count, BEFORE the
//                                 pools are sized; the statuses are one more downloaded array.  A null host pointer (an output the caller does
//                                 not want) registers nothing: its handle resolves to a null device pointer and nothing is copied.
//   open(plan, item_slot_bytes)   hipSetDevice, stage_lock (held until the driver goes out of scope), the pools -- slots of the largest pass x
//                                 item_slot_bytes, two when the plan has more than one pass, which is also when copies overlap unless `overlap` says
//                                 otherwise -- and the uploads, enqueued on `st`.  An empty plan opens no arena.
//   dev(handle)                   the array's device pointer, resolved at the time of the call and null before open(): opening may move the pools.
//   passes(src, item_bytes, body) per pass k of m items from item `base` on: feed(k), body(k, base, m, d_chunk), consumed(k); stops at the first
//                                 non-zero code.  The body enqueues on `st`; the slot is released behind all of it.
//   close(rc)                     the one exit of the call, `rc` = the code of the steps since open(): the downloads and the synchronisation of `st`,
//                                 or, after any failure (its own included), a wait for the whole device -- copies into and out of the caller's buffers
//                                 may be in flight -- and the first code, its text untouched.  A failing open() has taken this exit already.
// Workspaces and ctx->lock are the caller's business, between open() and close() (with_workspace).  commit_host runs its two-stream loop on `ring` itself.
struct HostCall {
  const kzg_ctx* ctx;
  StageRing ring;
  hipStream_t st = nullptr;    // stage_streams[0], from open() on: an idle non-blocking stream (the null stream would serialise against every
                               // blocking stream of the process)
  std::vector<uint64_t> plan;  // items per pass
  uint64_t max_pass = 0;
  explicit HostCall(const kzg_ctx* c) : ctx(c) {}
  int upload(const void* host, size_t bytes) { return add(UP, const_cast<void*>(host), bytes); }
  int download(void* host, size_t bytes) { return add(DOWN, host, bytes); }
  int scratch(size_t bytes) { return add(SCRATCH, nullptr, bytes); }
  template <class T = uint8_t>
  T* dev(int handle) const {
    return opened && handle >= 0 ? reinterpret_cast<T*>(ctx->hostio + arrays[handle].off) : nullptr;
  }
  int32_t open(std::vector<uint64_t> passes_plan, size_t item_slot_bytes, bool overlap);
  int32_t open(std::vector<uint64_t> passes_plan, size_t item_slot_bytes) {
    const bool piped = passes_plan.size() > 1;
    return open(std::move(passes_plan), item_slot_bytes, piped);
  }
  template <class Body>
  int32_t passes(const uint8_t* src, size_t item_bytes, Body&& body) {
    int32_t rc = 0;
    uint64_t base = 0;
    for (size_t k = 0; k < plan.size() && rc == 0; base += plan[k], k++) {
      uint8_t* d_chunk = nullptr;
      rc = ring.feed(k, src + base * item_bytes, plan[k] * item_bytes, st, &d_chunk);
      if (rc == 0) rc = body(k, base, plan[k], d_chunk);
      if (rc == 0) rc = ring.consumed(k, st);
    }
    return rc;
  }
  // passes() over the rows of a column matrix of `rows` rows in the caller's memory (`columns` columns of piece_bytes per row): a pass of
  // m rows from row `base` on arrives as a column matrix of m rows
  template <class Body>
  int32_t passes_of_rows(const uint8_t* matrix, size_t piece_bytes, size_t columns, uint64_t rows, Body&& body) {
    int32_t rc = 0;
    uint64_t base = 0;
    for (size_t k = 0; k < plan.size() && rc == 0; base += plan[k], k++) {
      uint8_t* d_chunk = nullptr;
      rc = ring.feed_pitched(k, matrix + base * piece_bytes, rows * piece_bytes, plan[k] * piece_bytes, columns, st, &d_chunk);
      if (rc == 0) rc = body(k, base, plan[k], d_chunk);
      if (rc == 0) rc = ring.consumed(k, st);
    }
    return rc;
  }
  int32_t close(int32_t rc);

 private:
  enum Kind { UP, DOWN, SCRATCH };
  struct Array {
    Kind kind;
    void* host;
    size_t bytes, off;
  };
  static constexpr int MAX_ARRAYS = 8;
  Array arrays[MAX_ARRAYS];
  int count = 0;
  bool opened = false, too_many = false;  // more than MAX_ARRAYS registrations: open() refuses
  Carve io;
  std::unique_lock<std::mutex> stage_guard;
  int add(Kind kind, void* host, size_t bytes) {
    if (kind != SCRATCH && !host) return -1;
    if (count == MAX_ARRAYS) {
      too_many = true;
      return -1;
    }
    arrays[count] = Array{kind, host, bytes, io.take(bytes)};
    return count++;
  }
};
// passes of `pass` items and a shorter last one
static inline std::vector<uint64_t> even_plan(uint64_t n, uint64_t pass) {
  std::vector<uint64_t> plan;
  for (uint64_t rest = n; rest; rest -= plan.back()) plan.push_back(rest < pass ? rest : pass);
  return plan;
}

// workspace of the call being enqueued (caller holds ctx->lock from ws_begin to ws_end)
int32_t ws_begin(const kzg_ctx* ctx, hipStream_t st);    // takes the next slot; `st` waits for the slot's previous user
int32_t ws_wait(const kzg_ctx* ctx, hipStream_t st);     // a further stream of the same call waits for it too
int32_t ws_reserve(const kzg_ctx* ctx, size_t bytes, hipStream_t st);  // grows THIS slot only (waits for its previous user on the host first); if the
                                                                        // device has no room, falls back to a slot that is large enough already and makes `st` wait for it
int32_t ws_end(const kzg_ctx* ctx, hipStream_t st);      // records the slot's event on `st`
// ws_begin ... ws_end of one call; an error return in between still records the slot's event (kernels of the failed call that
// were already enqueued are then ordered before the slot's next user -- ADVICE r04)
struct WsCall {
  const kzg_ctx* ctx;
  hipStream_t st;
  bool open = false;
  WsCall(const kzg_ctx* c, hipStream_t s) : ctx(c), st(s) {}
  int32_t begin() {
    const int32_t rc = ws_begin(ctx, st);
    open = rc == 0;
    return rc;
  }
  int32_t end() {
    open = false;
    return ws_end(ctx, st);
  }
  ~WsCall() {
    if (open) (void)ws_end(ctx, st);
  }
};
static inline uint8_t* ws_ptr(const kzg_ctx* ctx) { return reinterpret_cast<uint8_t*>(ctx->wss[ctx->ws_cur].p); }
// The workspace bracket of a call on one stream: ctx->lock and a slot are held while body() ENQUEUES on `st` -- ws_reserve, then the
// launches -- and given back before the host waits for anything: the slot's event orders its next user behind this call.  Returns the
// first non-zero code.
template <class Body>
static inline int32_t with_workspace(const kzg_ctx* ctx, hipStream_t st, Body&& body) {
  std::lock_guard<std::mutex> guard(ctx->lock);
  WsCall ws(ctx, st);
  int32_t rc = ws.begin();
  if (rc == 0) rc = body();
  if (rc == 0) rc = ws.end();
  return rc;
}
int32_t prof_next(const kzg_ctx* ctx, int kind, hipEvent_t* e0, hipEvent_t* e1);
// brackets the launches enqueued on `st` during its lifetime with an event pair (no-op unless profiling)
struct ProfScope {
  hipEvent_t e1 = nullptr;
  hipStream_t st;
  ProfScope(const kzg_ctx* ctx, int kind, hipStream_t s) : st(s) {
    hipEvent_t e0 = nullptr;
    if (ctx->profiling.load(std::memory_order_relaxed) && prof_next(ctx, kind, &e0, &e1) == 0 && e0) (void)hipEventRecord(e0, st);
  }
  ~ProfScope() {
    if (e1) (void)hipEventRecord(e1, st);
  }
};
uint32_t choose_splits(const kzg_ctx* ctx, uint64_t n);
static inline unsigned blocks_for(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// Every translation unit carries its kernels in a code object of its own, which the HIP runtime loads at the unit's FIRST launch --
// behind whatever the runtime is doing then: with KZG_CFG_BUILD_ASYNC that is the background thread's 96- / 192-GiB allocation, and the
// first commitment after kzg_ctx_create waited 1.5-4.7 s for it (profiles/r05/first_use_regression.json).  kzg_ctx_create therefore
// touches one kernel of every unit (hipFuncGetAttributes) before it starts the background build.
void warm_code_object_blob();    // engine_blob.hip
void warm_code_object_proof();   // engine_proof.hip
void warm_code_object_verify();  // engine_verify.hip
// ---- launchers of engine_blob.hip (hash, point decoding, scalar parsing: blob_kernels.cuh) --------------------------------
// Fiat-Shamir challenges of n blobs (Blob::challenge, src/blob.rs:78-97) into z (plain limbs)
void launch_challenge(const kzg_ctx* ctx, hipStream_t st, const uint8_t* blobs, const uint8_t* commitments48, uint64_t n, fr_t* z);
// Small batches: challenges of n blobs and decoding of n_a + n_b points in one launch
bool fused_prep_fits(const kzg_ctx* ctx, uint64_t n_blobs, uint64_t n_points);
void launch_challenge_and_decode(const kzg_ctx* ctx, hipStream_t st, const uint8_t* blobs, const uint8_t* commitments48, uint64_t n, fr_t* z, const uint8_t* in_a,
                                 uint64_t n_a, int32_t* status_a, const uint8_t* in_b, uint64_t n_b, int32_t* status_b, uint4* affine, uint8_t* inf);
// P1::decompress (src/bls.rs:505-531) of n_a + n_b points (two input arrays, one output array), all of them or the range [first, first + count)
void launch_g1_decompress(hipStream_t st, const uint8_t* in_a, uint64_t n_a, int32_t* status_a, const uint8_t* in_b, uint64_t n_b, int32_t* status_b, uint4* affine,
                          uint8_t* inf);
void launch_g1_decompress_range(hipStream_t st, uint64_t first, uint64_t count, const uint8_t* in_a, uint64_t n_a, int32_t* status_a, const uint8_t* in_b, uint64_t n_b,
                                int32_t* status_b, uint4* affine, uint8_t* inf);
// Fr::from_be_slice (src/bls.rs:130-139) for n caller-supplied 32-byte values; plain limbs -> 32 big-endian bytes
void launch_fr_parse(hipStream_t st, const uint8_t* in32, uint64_t n, fr_t* out_plain, int32_t* status);
void launch_fr_store_be(hipStream_t st, const fr_t* plain, uint64_t n, const int32_t* status, uint8_t* out32);
// kzg_to_versioned_hash (EIP-4844) of n commitments: 0x01 || SHA-256(commitment48)[1:32]; 32 zero bytes where status[i] != 0
void launch_versioned_hash(hipStream_t st, const uint8_t* commitments48, uint64_t n, const int32_t* status, uint8_t* out32);
// [z^2]-images of points [0, npts) of `aff` at [phi_off, phi_off + npts) (engine_verify.hip: k_glv_points)
void launch_glv_points(hipStream_t st, uint4* aff, uint64_t npts, uint64_t phi_off);
void launch_synth_blobs(hipStream_t st, uint64_t seed, uint64_t first_index, uint64_t n, uint8_t* d_blobs);
constexpr uint64_t KZG_FUSED_PREP_MAX = 16384;  // the two-wave kernel's limit: 512 hash waves + 512 decode waves (verify), one wave per SIMD on 256 CUs

// The comb's half-wave mode: when two blobs per wave is the cheaper shape (engine.hip, msm_shape: from num_CUs x 16 = 4,096
// blobs per launch on, when that fills whole rounds), a blob takes 32 lanes (each lane owns twice the blocks for the same
// number of Horner doublings).  Units = waves of the MSM kernel = rows of 64 lane sums.
constexpr uint64_t KZG_LAT_MAX_BLOBS = 16;
// Units per blob on the latency comb (512 blocks x 4 planes per blob): 256 for up to 4 blobs (a lane chains 8 additions + 3
// doublings, and 1,024 waves are one per SIMD), 128 up to 8, 64 up to 16.  The main class-22 comb never splits more than 24
// ways (24 blocks per lane), so a split count >= 64 names the table.
static inline uint32_t lat_splits(uint64_t n) { return n <= 4 ? 256u : (n <= 8 ? 128u : 64u); }
static inline bool msm_uses_lat(const kzg_ctx* ctx, uint32_t splits) { return ctx->d_table_lat != nullptr && splits >= 64u; }
uint32_t msm_lanes_per_blob(const kzg_ctx* ctx, uint64_t n, uint32_t splits);  // engine.hip (msm_shape)
static inline uint64_t msm_units(uint64_t n, uint32_t splits, uint32_t lpb) { return lpb == 64 ? n * splits : (n + 1) / 2; }

// Scratch the fixed-base MSM needs besides the lane sums: the comb's bit-plane masks (the blob transposed, 128 KiB per blob).
// Behind them, the second lane sums of a balanced half-wave launch (comb_geom.hpp CombBalance): one row of 64 per unit, 6 KiB per blob.
static inline size_t msm_scratch_bytes(const kzg_ctx* ctx, uint64_t n) {
  return ctx->use_comb ? (size_t)n * KZG_BYTES_PER_BLOB + (size_t)((n + 1) / 2) * 64 * sizeof(g1_xyzz) : 0;
}
// What msm_launch decided for one launch and msm_finish must know: the plan the launch runs under, its second lane sums, and the
// timing record it folds into (seq = 0: none).
struct MsmCall {
  CombBalance plan = comb_balance_none();
  g1_xyzz* partials2 = nullptr;
  uint64_t seq = 0;
};

// ---- launchers of engine.hip (fixed-base MSM: msm_comb.cuh, msm_fixed.cuh) ---------------------------------------------------
// The fixed-base MSM alone over `n` scalar vectors on the device: 64 lane sums per (blob, split) unit into
// partials[unit * 64 + lane].  `be_bytes`: the scalars are raw blob bytes (big-endian, canonicity checked into d_status) or
// plain little-endian limbs.  `scratch`: msm_scratch_bytes(ctx, n) bytes.  `scalars_consumed` (optional): recorded on `st` as
// soon as d_scalars is no longer read (after the bit-plane transposition; the MSM kernel reads the masks), so that a staging
// buffer can be refilled while the MSM runs.
int32_t msm_launch(const kzg_ctx* ctx, bool be_bytes, const uint8_t* d_scalars, uint64_t n, int32_t* d_status, g1_xyzz* partials, uint32_t splits, uint32_t lpb,
                   void* scratch, hipStream_t st, MsmCall& call, hipEvent_t scalars_consumed = nullptr);
// Lane sums of n blobs -> 48-byte encodings.  Two tree stages: the 64 lane sums of every (blob, split) unit, then the units
// of a blob.  `partials` must have room for n * splits unit sums after the n * splits * 64 lane sums.  `call`: as msm_launch left it.
int32_t msm_finish(const kzg_ctx* ctx, uint64_t n, uint8_t* d_out48, uint8_t* d_out_affine96, const int32_t* d_status, g1_xyzz* partials, g1_xyzz* sums,
                   uint32_t splits, uint32_t lpb, hipStream_t st, const MsmCall& call);
// The buffers of one MSM + reduce + compress over up to n scalar vectors, as offsets into a workspace: the lane sums (64 lane sums + 1 unit
// sum per (vector, split)), the n sums and msm_scratch_bytes; `splits` is choose_splits(ctx, n).
struct MsmBufs {
  uint32_t splits = 1;
  size_t o_part = 0, o_sum = 0, o_scratch = 0;
};
static inline MsmBufs msm_carve(const kzg_ctx* ctx, Carve& ws, uint64_t n) {
  MsmBufs b;
  b.splits = choose_splits(ctx, n);
  b.o_part = ws.take((size_t)n * b.splits * 65 * sizeof(g1_xyzz));
  b.o_sum = ws.take((size_t)n * sizeof(g1_xyzz));
  b.o_scratch = ws.take(msm_scratch_bytes(ctx, n));
  return b;
}
// MSM + reduce + compress of n vectors in the buffers `bufs` of the workspace at `ws`
int32_t msm_pipeline(const kzg_ctx* ctx, bool be_bytes, const uint8_t* d_scalars, uint64_t n, uint8_t* d_out48, uint8_t* d_out_affine96, int32_t* d_status,
                     const MsmBufs& bufs, uint8_t* ws, hipStream_t st);
