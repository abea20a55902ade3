/*
 * kateth_amd -- MI355X (gfx950) EIP-4844 KZG engine: C ABI.
 *
 * This is the drop-in boundary for kateth's hot path.  kateth has no FFI of its
 * own below its public Rust API other than the per-operation blst calls
 * (src/bls.rs:8-19), which are too fine-grained to put a GPU behind, so the
 * entry points here are batch-level and sit directly under the crate's public
 * methods; each one names the reference function it
 * replaces.  Byte layouts are exactly the reference's wire formats: a blob is
 * 4096 x 32-byte big-endian field elements (src/blob.rs:23-37), a commitment or
 * proof is a 48-byte ZCash-compressed G1 point (src/bls.rs:491-531), a field
 * element is 32 bytes big-endian (src/bls.rs:130-149).
 *
 * Plain C: pointers and sizes only.  Nothing unwinds across this boundary.
 * A kzg_ctx is immutable after creation and may be used from several host
 * threads at once, matching `&self` + `Arc<Setup>` in the reference
 * (src/kzg/setup.rs:323): commitment and proof calls hold an internal lock only
 * while they enqueue and take one of the context's three GPU workspaces (the lowest
 * one whose last user has completed or ran on the call's own stream), so calls
 * enqueued on several streams run side by side; every verification call takes its
 * own pooled session (device scratch + streams) and runs beside the others; the
 * host-buffer calls additionally serialise on the staging arena.  A context
 * created with kzg_config.devices / ndev spans several GPUs (below).
 *
 * Streams and hardware queues: the HIP runtime multiplexes all streams of a
 * process onto GPU_MAX_HW_QUEUES hardware queues (4 unless set) and streams
 * that share a queue run one after the other.  The variable is read when the
 * PROCESS first touches HIP, so it is the host program's to set: the library
 * never changes the environment.  kzg_recommended_env() returns the setting
 * the measured configurations ran with ("GPU_MAX_HW_QUEUES=16"); with
 * KATETH_AMD_TRACE set, kzg_ctx_create says once when it is missing or below
 * 8.  Results never depend on it -- only how many
 * calls kept in flight on different streams really overlap.
 *
 * Return value of every call: 0 on success, a positive KZG_ERR_* code when an
 * input is rejected the way the reference returns Err, a negative KZG_FAIL_*
 * code for a runtime (HIP / allocation / argument) failure.
 */
#ifndef KATETH_AMD_H
#define KATETH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZG_FIELD_ELEMENTS_PER_BLOB 4096
#define KZG_BYTES_PER_FIELD_ELEMENT 32
#define KZG_BYTES_PER_BLOB 131072 /* Blob::<4096>::BYTES, src/blob.rs:24 */
#define KZG_BYTES_PER_G1 48       /* P1::COMPRESSED, src/bls.rs:552 */
#define KZG_BYTES_PER_G2 96       /* P2::COMPRESSED, src/bls.rs:569 */
#define KZG_SETUP_G1_POINTS 4096  /* Setup<4096, 65>, benches/kzg.rs:12 */
#define KZG_SETUP_G2_POINTS 65
#define KZG_CELLS_PER_EXT_BLOB 128     /* EIP-7594: the blob extended to 8192 elements, cut into cells */
#define KZG_FIELD_ELEMENTS_PER_CELL 64
#define KZG_BYTES_PER_CELL 2048
#define KZG_G1_MONOMIAL_POINTS 64      /* the monomial G1 points [tau^j]_1, j < 64, a context derives on first use (kzg_ctx_g1_monomial) */

/* per-item / per-call rejection codes; they rebuild the reference's enums */
#define KZG_OK 0
#define KZG_ERR_BLOB_INVALID_LEN 1           /* blob::Error::InvalidLen            src/blob.rs:9   */
#define KZG_ERR_BLOB_INVALID_FIELD_ELEMENT 2 /* blob::Error::InvalidFieldElement   src/blob.rs:8   */
#define KZG_ERR_EC_INVALID_ENCODING 3        /* ECGroupError::InvalidEncoding      src/bls.rs:29  */
#define KZG_ERR_EC_NOT_ON_CURVE 4            /* ECGroupError::NotOnCurve           src/bls.rs:31  */
#define KZG_ERR_EC_NOT_IN_GROUP 5            /* ECGroupError::NotInGroup           src/bls.rs:30  */
#define KZG_ERR_FF_INVALID_ENCODING 6        /* FiniteFieldError::InvalidEncoding  src/bls.rs:23  */
#define KZG_ERR_FF_NOT_IN_FIELD 7            /* FiniteFieldError::NotInFiniteField src/bls.rs:24  */
/* kzg_recover_cells_batch only; the reference has no cell recovery */
#define KZG_ERR_CELLS_NOT_ENOUGH 8           /* fewer than 64 cells present */
#define KZG_ERR_CELLS_INCONSISTENT 9         /* the present cells are not the evaluations of one polynomial of degree < 4096 */
/* kzg_verify_cell_proof_batch only */
#define KZG_ERR_CELL_INDEX 10                /* a cell index >= 128 */
/* kzg_verify_cell_proof_batch_rows, kzg_cell_row_weights only */
#define KZG_ERR_COMMITMENT_INDEX 11          /* a commitment index >= the number of commitments given */

#define KZG_FAIL_ARGUMENT (-1)
#define KZG_FAIL_HIP (-2)
#define KZG_FAIL_NO_DEVICE (-3)
#define KZG_FAIL_SETUP_G1 (-4) /* LoadSetupError::Bls on a g1_lagrange point, src/kzg/setup.rs:59-64 */
#define KZG_FAIL_SETUP_G2 (-5) /* LoadSetupError::Bls on a g2_monomial point, src/kzg/setup.rs:67-72 */
/* A setup the comb table cannot represent: some +-1 combination of a block of consecutive g1_lagrange points is the point
 * at infinity (repeated / opposite points).  The reference would load it; no ceremony output or set of independent points
 * is affected.  Rejected at creation instead of producing wrong commitments. */
#define KZG_FAIL_SETUP_UNSUPPORTED (-6)
/* The host side of a call failed: out of host memory, or a C++ exception nobody expected (kzg_last_error() has its text).
 * Every int32_t entry point catches what its body throws -- nothing unwinds into the caller's frames. */
#define KZG_FAIL_HOST (-7)

typedef struct kzg_ctx kzg_ctx;

/*
 * The fixed-base MSM table is a subset-sum comb (kateth_amd/csrc/msm_comb.cuh): the 4096 Lagrange points are cut into blocks
 * of t consecutive points, a table entry (96 B, affine) is one +-1 combination of a block, and the 256 bit planes of the
 * scalars are cut into G plane groups with a table each.  Table bytes = G * 64 * e * 96 with e entries per 64 points and
 * group; mixed additions per blob = 256 * (blocks per 64 points) * 64; a lane doubles its accumulator 256/G - 1 times.
 *
 *   class | blocks per 64 points | e        | default G | resident table   | additions per blob
 *   ------+----------------------+----------+-----------+------------------+-------------------
 *    22   | 22 + 21 + 21 points  | 2^22     | 8 (or 4)  | 192 GiB (96 GiB) | 49,152
 *    16   | 4 x 16               | 4 * 2^15 | 16        | 12.9 GB          | 65,536
 *     8   | 8 x 8                | 8 * 2^7  | 16        | 100.7 MB         | 131,072
 *     4   | 16 x 4               | 16 * 2^3 | 16        | 12.6 MB          | 262,144
 *
 * Class 22 also keeps a 403-MB latency comb (blocks of 8 points, 64 plane groups) for calls of at most 16 blobs.  Building
 * a table needs up to 13 GB of transient device scratch (XYZZ staging for the batch normalisation) on top of it.
 *
 * AUTOMATIC choice (window_bits = 0, what the Rust shim's Setup::load_json passes): the fastest class whose table is within
 * the caller's BUDGET and fits the HBM that is free when the context is created, with room left for the build scratch, the
 * call workspace and the caller's blobs:
 *     class 22, G = 8 (192 GiB)  if the budget allows it and >= 232 GiB are free
 *     class 22, G = 4 ( 96 GiB)  if the budget allows it and >= 136 GiB are free
 *     class 16        (12.9 GB)  if the budget allows it and >=  21 GiB are free
 *     class 8         (100 MB)   otherwise
 * The budget is table_budget_bytes; 0 means the DEFAULT budget of 100 GiB -- so an unconfigured context never takes more
 * than the 96-GiB table (2.4 % slower than the 192-GiB one), whatever the device has free -- unless flags carries
 * KZG_CFG_TABLE_MAX, which lifts the cap (bench.py opts in; 192 GiB on an idle MI355X).  An explicit window_bits /
 * plane_groups is honoured as given and fails if it cannot be built.  PRECEDENCE, one rule: a non-zero field of kzg_config
 * beats the environment (KATETH_AMD_WINDOW_BITS, KATETH_AMD_COMB_GROUPS, KATETH_AMD_TABLE_BUDGET_GIB -- an operator's cap on
 * the automatic choice of an unconfigured drop-in, e.g. 16 for the 12.9-GB table), which beats the automatic choice.
 * kzg_ctx_window_bits / kzg_ctx_plane_groups / kzg_ctx_table_bytes report what was built.
 */
#define KZG_CFG_TABLE_MAX 0x1   /* flags: the automatic choice may take the largest table the device has room for (192 GiB) */
#define KZG_CFG_BUILD_ASYNC 0x2 /* flags: kzg_ctx_create returns as soon as a small first-use table (class 8, 100 MB) stands and
                                 * builds the chosen table on a background thread, swapping it in between calls; results are
                                 * identical before and after the swap (kzg_ctx_ready / kzg_ctx_wait_ready) */
#define KZG_ALL_DEVICES 0xffffffffu /* ndev: every HIP device visible to the process */
typedef struct kzg_config {
  uint32_t struct_size; /* = sizeof(kzg_config) of the header the caller was compiled against (KZG_CONFIG_INIT sets it): the library
                         * rejects a size it does not know instead of reading fields the caller never wrote (the struct has grown
                         * between rounds and will again) */
  int32_t device;       /* HIP device ordinal this context lives on (ignored when ndev != 0) */
  int32_t window_bits;  /* table class: 22, 16..21 (-> 16), 8..15 (-> 8), 4..7 (-> 4); 0 = automatic (above) */
  int32_t flags;        /* KZG_CFG_* bits */
  int32_t plane_groups; /* G: 1, 2, 4, 8 or 16; 0 = automatic (class 22: 8 or 4 as above; the other classes: 16) */
  uint64_t table_budget_bytes; /* cap on the table the AUTOMATIC choice may build; 0 = default (100 GiB, or none with KZG_CFG_TABLE_MAX) */
  /* Multi-GPU (`kzg_ctx_create(g1, g2, devices[], ndev, &ctx)`): ndev != 0 makes the context a GROUP
   * with one member per listed ordinal (an ordinal may be listed more than once: two members on one card).  Every member
   * holds the full tables; the HOST-BUFFER entry points split a batch into contiguous ranges, one per member, run them on
   * one host thread per member and write the results straight into the caller's buffers (blobs are independent, src/kzg/
   * setup.rs:235-242: no collective); batch verification runs phase 1 / phase 2 per member with global indices, merges the
   * first-error records in the reference's order (src/kzg/setup.rs:259-271) and does ONE pairing check.  The *_dev entry
   * points, sessions, profiling and introspection act on member 0 (device pointers belong to one device);
   * kzg_ctx_member(ctx, k) lends member k's single-device context to callers that keep data resident on that GPU. */
  const int32_t* devices; /* ndev ordinals, or NULL with ndev = KZG_ALL_DEVICES */
  uint32_t ndev;          /* 0 = a single-device context on `device` */
  uint32_t reserved;      /* must be 0 */
} kzg_config;
#define KZG_CONFIG_INIT {(uint32_t)sizeof(kzg_config), 0, 0, 0, 0, 0, NULL, 0, 0} /* kzg_config cfg = KZG_CONFIG_INIT; then set fields */

/* "NAME=value" of the one environment variable of the HIP runtime the measured configurations depend on (see "Streams and
 * hardware queues" above); static storage.  The library itself never calls setenv. */
const char* kzg_recommended_env(void);

/* Thread-local text for the last negative return on this thread ("" if none). */
const char* kzg_last_error(void);
/* When that return was KZG_FAIL_SETUP_G1 / KZG_FAIL_SETUP_G2: the KZG_ERR_EC_* code of the rejected setup point, so that
 * the caller can rebuild LoadSetupError::Bls(bls::Error::ECGroup(..)) exactly (src/kzg/setup.rs:59-72); otherwise 0. */
int32_t kzg_last_error_code(void);

/*
 * Replaces Setup::<4096,65>::load_json after JSON/hex parsing
 * (src/kzg/setup.rs:52-81): decompresses and subgroup-checks the 4096 G1
 * Lagrange points and the 65 G2 monomial points (given in FILE order),
 * bit-reversal-permutes G1, derives the 4096 roots of unity (src/math.rs:16-29)
 * and builds the resident device tables.
 *   g1_lagrange : 4096 * 48 bytes      g2_monomial : 65 * 96 bytes
 */
int32_t kzg_ctx_create(const uint8_t* g1_lagrange, const uint8_t* g2_monomial, const kzg_config* cfg, kzg_ctx** out);
/* The same with the device list as arguments, the shape SURVEY.md section 8(b) wrote down: cfg's devices / ndev are replaced
 * by the arguments (cfg may be NULL); devices = NULL with ndev = KZG_ALL_DEVICES takes every visible device. */
int32_t kzg_ctx_create_multi(const uint8_t* g1_lagrange, const uint8_t* g2_monomial, const int32_t* devices, uint32_t ndev, const kzg_config* cfg,
                             kzg_ctx** out);
void kzg_ctx_destroy(kzg_ctx* ctx);
/* HIP devices visible to the process (what KZG_ALL_DEVICES expands to); negative = KZG_FAIL_* */
int32_t kzg_device_count(void);
/* members of a group context (1 for a single-device context), member k's device ordinal, and member k as a single-device
 * context (borrowed: owned and destroyed by `ctx`; member 0 of a single-device context is the context itself) */
uint32_t kzg_ctx_members(const kzg_ctx* ctx);
int32_t kzg_ctx_member_device(const kzg_ctx* ctx, uint32_t k);
const kzg_ctx* kzg_ctx_member(const kzg_ctx* ctx, uint32_t k);
/* KZG_CFG_BUILD_ASYNC: 1 once the chosen table is in use (always 1 without the flag), 0 while the first-use table serves;
 * kzg_ctx_wait_ready blocks until then and returns 0, or the KZG_FAIL_* code the background build ended with (the context
 * then stays on the first-use table).  On a group: all members. */
int32_t kzg_ctx_ready(const kzg_ctx* ctx);
int32_t kzg_ctx_wait_ready(const kzg_ctx* ctx);

/* introspection for benches / tests */
int32_t kzg_ctx_window_bits(const kzg_ctx* ctx);
const char* kzg_ctx_msm_kernel_name(const kzg_ctx* ctx); /* the dominant kernel bench.py names in `roofline` */
int32_t kzg_ctx_plane_groups(const kzg_ctx* ctx);
uint64_t kzg_ctx_table_bytes(const kzg_ctx* ctx);
/* bytes of commitment / proof workspace slot `slot` (0..2) as allocated so far: a caller that runs one call at a time only ever
 * grows slot 0; slots 1 and 2 are allocated when calls are found in flight side by side (tests, memory accounting) */
uint64_t kzg_ctx_workspace_bytes(const kzg_ctx* ctx, uint32_t slot);
/* The balance plan of the fixed-base MSM's two-blobs-per-wave launches (KATETH_AMD_COMB_BALANCE=off|auto|<partner>:<shed>) and the
 * newest timing record a launch has taken, as 44 words: [0..7] partner and [8..15] steps shed of the eight unit classes (unit
 * index mod 8) as the next launch would get them; [16] the record's sequence number (0: none yet), [17] earliest start and
 * [18..25] latest end per class on the device's 100-MHz counter, [26] units that reported, [27] units launched; [28..43] the
 * partner and shed words that launch ran under. */
int32_t kzg_ctx_comb_balance(const kzg_ctx* ctx, uint64_t* out44);

/*
 * Replaces Setup::blob_to_commitment + Compress::compress for n blobs
 * (src/kzg/setup.rs:167-171, src/blob.rs:26-53, src/bls.rs:491-503).
 *   blobs  : n * 131072 bytes          out48  : n * 48 bytes
 *   status : n * int32 ; 0 or KZG_ERR_BLOB_INVALID_FIELD_ELEMENT per blob
 *            (a rejected blob's 48 output bytes are zeroed)
 * Host-pointer form copies in/out; the *_dev form takes HIP device pointers
 * resident on ctx's device and enqueues on `hip_stream` (a hipStream_t, NULL =
 * default stream) without synchronising.
 * `blob_len` lets the caller forward a wrong-length slice the way the Rust
 * shim would: blob_len != 131072 -> every status = KZG_ERR_BLOB_INVALID_LEN.
 */
int32_t kzg_blob_to_commitment_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out48, int32_t* status);
int32_t kzg_blob_to_commitment_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out48, void* d_status, void* hip_stream);

/*
 * The same producers with the result as the reference returns it -- a POINT, `Commitment = Proof = P1`
 * (src/kzg/mod.rs:9-10; Setup::blob_to_commitment / blob_proof / proof, src/kzg/setup.rs:167,177,185) -- instead of its
 * 48-byte encoding: 96 bytes per item = blst_p1_affine, i.e. x || y, each 6 x uint64 little-endian limbs of the
 * 2^384-Montgomery residue (infinity = 96 zero bytes, as blst encodes it).  The Rust side rebuilds the `P1` with
 * blst_p1_from_affine -- no square root on the CPU -- and callers such as benches/kzg.rs:24-32 can keep calling
 * `.compress()` on it.  Rejected items get 96 zero bytes and their status code.
 */
int32_t kzg_blob_to_commitment_batch_affine(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_affine96, int32_t* status);
int32_t kzg_compute_blob_proof_batch_affine(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, uint64_t n, uint8_t* out_affine96, int32_t* status);
int32_t kzg_compute_proof_batch_affine(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* z32, uint64_t n, uint8_t* out_proof_affine96, uint8_t* out_y32, int32_t* status);

/*
 * Replaces P1::decompress -- the crate's public `Decompress` trait on G1 points, i.e. on `Commitment` / `Proof`
 * (src/lib.rs:5, src/bls.rs:505-531: ZCash decoding, on-curve check, SUBGROUP check) -- for n compressed points:
 *   in48         : n * 48 bytes
 *   out_affine96 : n * 96 bytes, blst_p1_affine images as above (infinity = 96 zero bytes, status 0)
 *   status       : per point 0 or KZG_ERR_EC_INVALID_ENCODING / KZG_ERR_EC_NOT_ON_CURVE / KZG_ERR_EC_NOT_IN_GROUP
 *                  (a rejected point's 96 output bytes are zeroed)
 * The same decoder the verification entry points run on their commitments and proofs.
 */
int32_t kzg_g1_decompress_batch(const kzg_ctx* ctx, const uint8_t* in48, uint64_t n, uint8_t* out_affine96, int32_t* status);

/*
 * Replaces Polynomial::evaluate (src/kzg/poly.rs:10-33; with Blob::from_slice, src/blob.rs:26-37) for n (blob, z) pairs --
 * the evaluation step of the verification path on its own (there z is a hash output; an evaluation point on the domain,
 * poly.rs:14-18, reaches that kernel only through this call).  Any n: the blobs stream through the staging arena in chunks.
 *   blobs   : n * 131072 bytes          z32 : n * 32 bytes, big-endian canonical
 *   out_y32 : n * 32 bytes, big-endian (zero bytes for a rejected item)
 *   status  : per item 0, KZG_ERR_BLOB_INVALID_FIELD_ELEMENT, or KZG_ERR_FF_NOT_IN_FIELD for z
 */
int32_t kzg_evaluate_blobs(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* z32, uint64_t n, uint8_t* out_y32, int32_t* status);

/*
 * Replaces Setup::blob_proof + compress for n (blob, commitment) pairs
 * (src/kzg/setup.rs:177-183, src/blob.rs:55-97, src/kzg/poly.rs:10-71).
 *   status : per item 0, KZG_ERR_BLOB_*, or KZG_ERR_EC_* for the commitment
 */
int32_t kzg_compute_blob_proof_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, uint64_t n, uint8_t* out48, int32_t* status);
int32_t kzg_compute_blob_proof_batch_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, uint64_t n, void* d_out48, void* d_status, void* hip_stream);

/*
 * The blob sidecar of n blobs in one call: Setup::blob_to_commitment (src/kzg/setup.rs:167-171) followed by Setup::blob_proof
 * (:177-183) on the same blob, plus EIP-4844's kzg_to_versioned_hash of each commitment.  The blobs cross PCIe once, and the
 * proof's challenge hashes the commitments the device has just written (nothing is decoded or subgroup-checked again).
 *   blobs                  : n * 131072 bytes
 *   out_commitments48      : n * 48 bytes        out_proofs48 : n * 48 bytes
 *   out_versioned_hashes32 : n * 32 bytes, or NULL = not wanted
 *   status                 : n * int32 ; 0 or KZG_ERR_BLOB_INVALID_FIELD_ELEMENT per blob
 * Outputs: out_commitments48, out_proofs48 and status equal, byte for byte, what kzg_blob_to_commitment_batch followed by
 *   kzg_compute_blob_proof_batch(blobs, those commitments) write.  A rejected blob gets 48 + 48 + 32 zero bytes.
 * Versioned hash: for an accepted blob 0x01 || SHA-256(commitment48)[1:32]; the point at infinity (c0 00 ...) is hashed like any
 *   other commitment.
 * Bounds: nothing beyond n items is written; n == 0 returns 0.
 * Null pointers: a null required pointer with n > 0 returns KZG_FAIL_ARGUMENT; only the versioned-hash pointer may be null.
 * The *_dev form takes HIP device pointers resident on ctx's device (16-byte aligned), enqueues on `hip_stream` and returns without
 *   synchronising, like the other producer *_dev calls; it takes a workspace slot of its own, so calls on different streams run
 *   side by side.
 * Group contexts: the host-buffer call cuts the batch into the same contiguous shares as kzg_compute_blob_proof_batch; the *_dev
 *   call acts on member 0.
 */
int32_t kzg_blob_sidecar_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_commitments48, uint8_t* out_proofs48,
                               uint8_t* out_versioned_hashes32 /* may be NULL */, int32_t* status);
int32_t kzg_blob_sidecar_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out_commitments48, void* d_out_proofs48,
                                   void* d_out_versioned_hashes32 /* may be NULL */, void* d_status, void* hip_stream);

/*
 * The cells of n blobs (EIP-7594, PeerDAS): compute_cells of specs/fulu/polynomial-commitments-sampling.md, which is c-kzg-4844's
 * compute_cells_and_kzg_proofs(cells, NULL, blob).  The blob's polynomial p -- the one Polynomial::evaluate reads
 * (src/kzg/poly.rs:10-33) -- is evaluated at the 8192 powers of omega_8192 = 7^((r-1)/8192), in bit-reversed order: E[j] = blob
 * element j and E[4096 + j] = p(omega_8192 * roots_brp[j]) for j < 4096.  Cell c is E[64 c .. 64 c + 63], 32 bytes big-endian
 * canonical per element.
 *   blobs     : n * 131072 bytes
 *   out_cells : n * 128 * 2048 bytes; cells 0..63 of an accepted blob are the blob, byte for byte
 *   status    : n * int32 ; 0 or KZG_ERR_BLOB_INVALID_FIELD_ELEMENT per blob.  A rejected blob gets 262144 zero bytes.
 * With the cell proofs: kzg_compute_cells_and_proofs_batch.  Cell recovery is kzg_recover_cells_batch, cell verification
 *   kzg_verify_cell_proof_batch.
 * Bounds: nothing beyond n items is written; n == 0 returns 0.  A null pointer with n > 0 returns KZG_FAIL_ARGUMENT.
 * The *_dev form takes HIP device pointers resident on ctx's device (16-byte aligned), enqueues one kernel on `hip_stream` and returns
 *   without synchronising; it needs no workspace and takes no lock, so calls on different streams run side by side.
 * The host-buffer form streams the blobs through the staging ring in passes (KATETH_AMD_CELLS_PASS blobs each), downloads the
 *   extension half only and copies cells 0..63 from the caller's own blob.
 * Group contexts: the host-buffer call cuts the batch into the same contiguous shares as kzg_blob_to_commitment_batch; the *_dev
 *   call acts on member 0.
 */
int32_t kzg_compute_cells_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_cells /* n * 128 * 2048 */, int32_t* status);
int32_t kzg_compute_cells_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out_cells, void* d_status, void* hip_stream);

/*
 * The missing cells of n cell sets (EIP-7594, PeerDAS): the cells half of recover_cells_and_kzg_proofs of
 * specs/fulu/polynomial-commitments-sampling.md (c-kzg-4844's recover_cells_and_kzg_proofs without its proofs).  A node that holds at
 * least 64 of a blob's 128 cells rebuilds the others: the present elements determine the polynomial p of degree < 4096, and the
 * absent cells are its evaluations, as kzg_compute_cells_batch would give them.
 *   cells     : n * 128 * 2048 bytes, laid out like kzg_compute_cells_batch's output: cell c of an item at byte 2048 c
 *   present   : n * 16 bytes, a 128-bit mask per item: cell c is present iff bit (c & 7), least significant first, of byte (c >> 3)
 *               is set.  The bytes of an absent cell are never read: they may be anything, non-canonical garbage included.
 *   out_cells : n * 128 * 2048 bytes; for an accepted item all 128 cells, the present ones byte for byte as they came
 *   status    : n * int32 ; per item 0 or, in this order of precedence,
 *               KZG_ERR_CELLS_NOT_ENOUGH            fewer than 64 cells present
 *               KZG_ERR_BLOB_INVALID_FIELD_ELEMENT  an element >= r in a present cell
 *               KZG_ERR_CELLS_INCONSISTENT          the recovered polynomial disagrees with a present element
 *               A rejected item gets 262144 zero bytes; its neighbours are untouched.
 * The consistency check is an ADDITION to the specification: recover_polynomialcoeff truncates silently when the present cells do not
 *   lie on one polynomial of degree < 4096, so what it returns then depends on the algorithm.  Here every present element is compared
 *   with the recovered polynomial as the result is stored, which makes the call well-defined.  With exactly 64 cells present every
 *   input is consistent; the check can fire from 65 cells on.
 * out_cells must not overlap cells.  The kernel uses an item's own output region as scratch before the final stores: while a call
 *   is in flight the region holds intermediate values.
 * With the proofs half of recovery: kzg_recover_cells_and_proofs_batch.
 * Bounds: nothing beyond n items is written; n == 0 returns 0.  A null pointer with n > 0 returns KZG_FAIL_ARGUMENT.
 * The *_dev form takes HIP device pointers resident on ctx's device (16-byte aligned), enqueues one kernel on `hip_stream` and returns
 *   without synchronising; it needs no workspace and takes no lock, so calls on different streams run side by side.
 * The host-buffer form streams the cell sets through the staging ring in passes (KATETH_AMD_CELLS_PASS items each); every pass
 *   uploads and downloads whole cell sets.
 * Group contexts: the host-buffer call cuts the batch into the same contiguous shares as kzg_blob_to_commitment_batch; the *_dev
 *   call acts on member 0.
 */
int32_t kzg_recover_cells_batch(const kzg_ctx* ctx, const uint8_t* cells /* n * 128 * 2048 */, const uint8_t* present /* n * 16 */, uint64_t n,
                                uint8_t* out_cells /* n * 128 * 2048 */, int32_t* status);
int32_t kzg_recover_cells_batch_dev(const kzg_ctx* ctx, const void* d_cells, const void* d_present, uint64_t n, void* d_out_cells, void* d_status,
                                    void* hip_stream);

/*
 * The cells of n blobs AND their 128 cell proofs (EIP-7594, PeerDAS): compute_cells_and_kzg_proofs of
 * specs/fulu/polynomial-commitments-sampling.md; and recover_cells_and_kzg_proofs, both halves, for n cell sets.
 * Cells: out_cells and status are byte for byte what kzg_compute_cells_batch / kzg_recover_cells_batch write (their kernels run first);
 *   inputs, masks, statuses and their precedence are those calls'.
 * Proofs: proof k of an item is at byte 48 * (128 * item + k) of out_proofs48: the 48-byte encoding of the commitment of
 *   q_k = (p - I_k) / (X^64 - z_k), z_k = omega_128^brp7(k), with I_k the interpolant of cell k -- what verify_cell_kzg_proof_batch
 *   checks.  The point at infinity (c0 00 ...) is an ordinary proof (every proof of a blob of degree < 64).
 *   Method: q_k is the plain quotient of p by X^64 - z_k; its evaluations on the blob's domain are a scalar vector that the fixed-base
 *   MSM commits like a blob -- 128 scalar transforms and 128 MSMs per blob.  This is not FK20: no monomial setup and no G1 transform.
 *   out_cells    : n * 128 * 2048 bytes; of the compute call may be NULL (proofs only)
 *   out_proofs48 : n * 128 * 48 bytes
 *   status       : n * int32
 * Rejected items: the item's status code, 128 * 48 zero bytes of proofs and the zero cells it gets today; its neighbours are untouched.
 * Recovery: a recovered item's blob is cells 0..63 of its own output; items kzg_recover_cells_batch rejects are not looked at again.
 *   out_cells must not overlap cells.
 * Bounds: nothing beyond n items is written; n == 0 returns 0.  A null required pointer with n > 0 returns KZG_FAIL_ARGUMENT; only
 *   out_cells of the compute call may be null.
 * The *_dev forms take HIP device pointers resident on ctx's device (16-byte aligned), enqueue on `hip_stream` and return without
 *   synchronising (a context's first cell-proof call builds a 6 KiB table and waits for it); they take a workspace slot like the proof
 *   *_dev calls.  The batch is walked in passes of KATETH_AMD_CELLPROOF_PASS items (default 32: 4,096 vectors, 512 MiB of them).
 * The host-buffer forms stream the items through the staging ring in the same passes: blobs up, the extension half and 6 KiB of
 *   proofs down, cells 0..63 copied from the caller's blob (compute); whole cell sets up and down (recovery).
 * Group contexts: the host-buffer calls cut the batch into the same contiguous shares as kzg_blob_to_commitment_batch; the *_dev
 *   calls act on member 0.
 * Not here: FK20; a *_group_dev form; cell proofs without the transforms, for callers who hold coefficients.
 */
int32_t kzg_compute_cells_and_proofs_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_cells /* n * 128 * 2048, may be NULL */,
                                           uint8_t* out_proofs48 /* n * 128 * 48 */, int32_t* status);
int32_t kzg_compute_cells_and_proofs_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out_cells /* may be NULL */, void* d_out_proofs48,
                                               void* d_status, void* hip_stream);
int32_t kzg_recover_cells_and_proofs_batch(const kzg_ctx* ctx, const uint8_t* cells, const uint8_t* present, uint64_t n, uint8_t* out_cells,
                                           uint8_t* out_proofs48, int32_t* status);
int32_t kzg_recover_cells_and_proofs_batch_dev(const kzg_ctx* ctx, const void* d_cells, const void* d_present, uint64_t n, void* d_out_cells,
                                               void* d_out_proofs48, void* d_status, void* hip_stream);

/*
 * The select forms of the two calls above: the proofs of CHOSEN cells.  A node that rebuilds a blob from 64 or more columns holds the
 * proofs of the cells it received and needs those of the absent ones only; a node that serves its custody columns needs 8 of 128.  Only
 * the wanted (item, cell) pairs are divided, transformed and committed -- one MSM per wanted proof instead of 128 per item -- and the
 * results go where the full calls put them.  A caller writes the proofs it holds into the buffer, calls once, and holds the complete set.
 *   want           : n * 16 bytes, a 128-bit mask per item in the bit order of `present`: cell c is wanted iff bit (c & 7), least
 *                    significant first, of byte (c >> 3) is set.  HOST memory in every form, the *_dev ones included: it shapes the
 *                    launches (the host must know how many vectors a pass commits, as it knows n).  It is read before the call
 *                    returns; the caller may free or overwrite it then.  Independent of `present`: proofs of present cells may be wanted.
 *   inout_proofs48 : n * 128 * 48 bytes.  For an accepted item every wanted position 48 * (128 * item + k) holds exactly the bytes the
 *                    full call writes there; for a rejected item the wanted positions hold 48 zero bytes.  Unwanted positions are not
 *                    written: the caller's bytes stay.
 *   out_cells, status : byte for byte the full calls', whatever the masks say: an item with an empty mask is still range-checked or
 *                    recovered and gets its status.  out_cells of the compute forms may be NULL; out_cells must not overlap cells.
 * Bounds: nothing beyond n items is written; n == 0 returns 0.  A null required pointer with n > 0 returns KZG_FAIL_ARGUMENT, `want`
 *   included; only out_cells of the compute forms may be null.
 * Passes: consecutive items share a pass while its wanted proofs stay <= 128 * KATETH_AMD_CELLPROOF_PASS (default 32: 4,096 vectors)
 *   and its items <= 128; an item is never split.  With all-ones masks the passes are the full call's.
 * The *_dev forms take HIP device pointers resident on ctx's device (16-byte aligned) for everything but `want`, enqueue on `hip_stream`
 *   and return without synchronising on the device: the list of wanted pairs goes up through a pinned buffer the context keeps.  They
 *   take a workspace slot like the full *_dev calls.
 * The host-buffer forms bring only the selected proofs down (48 bytes each) and put them in place on the host.
 * Group contexts: the host-buffer calls cut the batch into the same contiguous shares as the full calls, `want` advanced with the items;
 *   the *_dev calls act on member 0.
 * kzg_ctx_cellproof_vectors: the quotient vectors `ctx` and its members have committed in cell-proof calls so far, the full calls
 *   included at 128 per item (measurement aid, like kzg_verify_each_checks).  The count is by launch size: the wanted vectors of a
 *   rejected item count.
 * Not here: a device-resident `want` (it would need a device-built pair list and worst-case launches); FK20; *_group_dev forms.
 */
int32_t kzg_compute_cells_and_proofs_select_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* want /* n * 16, HOST */, uint64_t n,
                                                  uint8_t* out_cells /* n * 128 * 2048, may be NULL */, uint8_t* inout_proofs48 /* n * 128 * 48 */,
                                                  int32_t* status);
int32_t kzg_compute_cells_and_proofs_select_batch_dev(const kzg_ctx* ctx, const void* d_blobs, const uint8_t* want /* n * 16, HOST */, uint64_t n,
                                                      void* d_out_cells /* may be NULL */, void* d_inout_proofs48, void* d_status, void* hip_stream);
int32_t kzg_recover_cells_and_proofs_select_batch(const kzg_ctx* ctx, const uint8_t* cells, const uint8_t* present, const uint8_t* want /* n * 16, HOST */,
                                                  uint64_t n, uint8_t* out_cells, uint8_t* inout_proofs48, int32_t* status);
int32_t kzg_recover_cells_and_proofs_select_batch_dev(const kzg_ctx* ctx, const void* d_cells, const void* d_present, const uint8_t* want /* n * 16, HOST */,
                                                      uint64_t n, void* d_out_cells, void* d_inout_proofs48, void* d_status, void* hip_stream);
uint64_t kzg_ctx_cellproof_vectors(const kzg_ctx* ctx);

/*
 * The data column forms of the cell calls: cells and proofs as COLUMN MATRICES, the layout a block producer's column sidecars and
 * kzg_verify_cell_proof_batch_rows' callers hold.  The consensus specs' compute_matrix / get_data_column_sidecars (produce) and
 * recover_matrix (recover) for one block.
 *   n                : the number of rows: the block's blobs, in order.
 *   column matrix    : of cells, 128 * n * 2048 bytes, the cell of column c, row b at 2048 * (c * n + b); of proofs, 128 * n * 48
 *                      bytes, the proof of (c, b) at 48 * (c * n + b).  Column c's sidecar payload is one run of n * 2048 and one of
 *                      n * 48 bytes.  With T the permutation from the blob-major layout of the cell calls to this one:
 * kzg_compute_data_columns_batch: out_column_cells, out_column_proofs48 and status are byte for byte T of
 *   kzg_compute_cells_and_proofs_batch(blobs), out_commitments48 (n * 48, may be NULL) byte for byte kzg_blob_to_commitment_batch(blobs).
 *   A rejected blob: KZG_ERR_BLOB_INVALID_FIELD_ELEMENT, its row zero bytes in all 128 columns of cells and of proofs, its commitment 48
 *   zero bytes; the other rows are untouched by it.  The blobs cross PCIe once for the three results.
 * kzg_recover_data_columns_batch: a node holds whole columns, so the masks are given ONCE and apply to every row (a caller with ragged
 *   cell sets keeps to the blob-major calls).
 *   present16, want16 : one 16-byte mask each, the bit order of `present` and `want` above.  HOST memory in every form, the *_dev ones
 *                      included: they travel as kernel arguments and through the pass plan and are read before the call returns.
 *   want16 == NULL   : cells only -- inout_column_proofs48 must be NULL too (and only then): no cell-proof table is built and no
 *                      workspace slot taken, as in kzg_recover_cells_batch.
 *   With the two masks repeated n times, out_column_cells, inout_column_proofs48 and status are exactly T of
 *   kzg_recover_cells_and_proofs_select_batch(T^-1 column_cells, present x n, want x n, T^-1 inout_column_proofs48): all 128 columns of
 *   an accepted row are written, the present ones byte for byte as they came; wanted proof positions hold the full call's bytes, those of
 *   a rejected row 48 zero bytes; unwanted proof positions keep the caller's bytes; status precedence, the consistency check and the
 *   zeroing of a rejected row's cells are that call's.  The bytes of an absent column are never interpreted.  out_column_cells must not
 *   overlap column_cells.
 * Bounds: nothing outside the matrices, the n commitments and the n statuses is written; n == 0 returns 0.  A null required pointer with
 *   n > 0 returns KZG_FAIL_ARGUMENT; only out_commitments48, and want16 together with the proofs, may be null.
 * The *_dev forms take HIP device pointers resident on ctx's device (16-byte aligned) for the matrices, commitments and statuses,
 *   enqueue on `hip_stream` and return without synchronising on the device.  They take a workspace slot only when proofs or commitments
 *   are computed.
 * Group contexts: the host-buffer forms cut the ROWS into the members' usual contiguous shares, and each member writes its rows of every
 *   column straight into the caller's matrices; the *_dev forms act on member 0.
 * Passes are those of the select calls above (KATETH_AMD_CELLPROOF_PASS); a pass of m rows writes rows [base, base + m) of every column.
 *   kzg_ctx_cellproof_vectors counts these calls like the others.
 * Not here: per-row masks, a device-resident want16, *_group_dev forms, a verification call with implicit indices
 *   (kzg_verify_cell_proof_batch_rows serves).
 */
int32_t kzg_compute_data_columns_batch(const kzg_ctx* ctx, const uint8_t* blobs, uint64_t n, uint8_t* out_commitments48 /* n * 48, may be NULL */,
                                       uint8_t* out_column_cells /* 128 * n * 2048 */, uint8_t* out_column_proofs48 /* 128 * n * 48 */, int32_t* status);
int32_t kzg_compute_data_columns_batch_dev(const kzg_ctx* ctx, const void* d_blobs, uint64_t n, void* d_out_commitments48 /* may be NULL */,
                                           void* d_out_column_cells, void* d_out_column_proofs48, void* d_status, void* hip_stream);
int32_t kzg_recover_data_columns_batch(const kzg_ctx* ctx, const uint8_t* column_cells /* 128 * n * 2048 */, const uint8_t* present16 /* 16, HOST */,
                                       const uint8_t* want16 /* 16, HOST, may be NULL */, uint64_t n, uint8_t* out_column_cells /* 128 * n * 2048 */,
                                       uint8_t* inout_column_proofs48 /* 128 * n * 48; NULL iff want16 is NULL */, int32_t* status);
int32_t kzg_recover_data_columns_batch_dev(const kzg_ctx* ctx, const void* d_column_cells, const uint8_t* present16 /* 16, HOST */,
                                           const uint8_t* want16 /* 16, HOST, may be NULL */, uint64_t n, void* d_out_column_cells,
                                           void* d_inout_column_proofs48 /* NULL iff want16 is NULL */, void* d_status, void* hip_stream);

/*
 * Replaces Setup::proof for n (blob, z) pairs (src/kzg/setup.rs:185-194):
 *   z32 : n * 32 bytes big-endian ; out_proof48 : n * 48 ; out_y32 : n * 32
 *   status : per item 0, KZG_ERR_BLOB_*, KZG_ERR_FF_NOT_IN_FIELD for z
 */
int32_t kzg_compute_proof_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* z32, uint64_t n, uint8_t* out_proof48, uint8_t* out_y32, int32_t* status);

/*
 * Replaces Setup::verify_blob_proof_batch (src/kzg/setup.rs:247-275).
 * Returns KZG_OK with *ok = 0/1, or -- like the reference's first-error-wins
 * collect (src/kzg/setup.rs:259-271: all blobs, then all commitments, then all
 * proofs) -- the KZG_ERR_* of the first rejected input, *ok = 0.
 * n == 0 -> *ok = 1.  The length-equality assert of the reference
 * (src/kzg/setup.rs:256-257) stays in the caller: the ABI takes a single n.
 */
int32_t kzg_verify_blob_proof_batch(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* proofs48, uint64_t n, int32_t* ok);
int32_t kzg_verify_blob_proof_batch_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_proofs48, uint64_t n, int32_t* ok, void* hip_stream);

/* Replaces Setup::verify_blob_proof (src/kzg/setup.rs:208-221): one item. */
int32_t kzg_verify_blob_proof(const kzg_ctx* ctx, const uint8_t* blob, const uint8_t* commitment48, const uint8_t* proof48, int32_t* ok);

/* Replaces Setup::verify_proof (src/kzg/setup.rs:96-113). */
int32_t kzg_verify_proof(const kzg_ctx* ctx, const uint8_t* proof48, const uint8_t* commitment48, const uint8_t* z32, const uint8_t* y32, int32_t* ok);

/*
 * Setup::verify_proof for n (proof, commitment, z, y) tuples in one call: the reference's private Setup::verify_proof_batch
 * (src/kzg/setup.rs:115-161) behind verify_proof's parsing (src/kzg/setup.rs:103-109), for callers that hold openings but
 * no blobs.  Argument order as kzg_verify_proof; every array has n items, contiguous: 48 bytes per point, 32 bytes big-endian
 * per scalar.  Device pointers (*_dev) are resident on ctx's device, z and y 16-byte aligned; the calls are synchronous like
 * kzg_verify_blob_proof_batch_dev (they return the boolean); hip_stream = NULL is the default stream.
 *   *ok = 1  iff  e(sum r^i proof_i, [tau]_2) == e(sum r^i (commitment_i - [y_i]G) + sum r^i z_i proof_i, G2)
 *            (src/kzg/setup.rs:151-160), r being the ENGINE's challenge: bound to every input through the transcript tree of the
 *            blob batch (leaf = H(commitment || z || y || proof)), powers r^0 .. r^(n-1) over GLOBAL indices -- the deviations
 *            Q1 / Q2 from the reference that kzg_verify_blob_proof_batch documents.  Hence: true iff every tuple passes
 *            kzg_verify_proof (up to the 2^-255 soundness error of the random combination).
 *   n == 0   *ok = 1 (as kzg_verify_blob_proof_batch).  n == 1: exactly kzg_verify_proof's boolean and code.
 *   rejected inputs: the positive KZG_ERR_* code of the FIRST rejected input, *ok = 0.  First = verify_proof's parse order
 *            (proof, commitment, point, evaluation) lifted to arrays the way verify_blob_proof_batch lifts its own
 *            (src/kzg/setup.rs:259-271): every proof before any commitment, every commitment before any z, every z before any
 *            y; the lowest index within the first kind that has an error.  z or y >= r: KZG_ERR_FF_NOT_IN_FIELD; points:
 *            KZG_ERR_EC_* as kzg_g1_decompress_batch reports them.  The length checks of the reference stay in the caller.
 * On a GROUP context the host-buffer call cuts the batch into contiguous shares, one per member, like
 * kzg_verify_blob_proof_batch; kzg_verify_proof_batch_group_dev takes member k's share resident on member k's GPU (arrays of
 * kzg_ctx_members(ctx) entries, global order = member order, n_local[k] may be 0) like kzg_verify_blob_proof_batch_group_dev.
 * One share is exactly the single-device call; several shares seed r with all their roots: same boolean, same code.
 */
int32_t kzg_verify_proof_batch(const kzg_ctx* ctx, const uint8_t* proofs48, const uint8_t* commitments48, const uint8_t* z32, const uint8_t* y32, uint64_t n,
                               int32_t* ok);
int32_t kzg_verify_proof_batch_dev(const kzg_ctx* ctx, const void* d_proofs48, const void* d_commitments48, const void* d_z32, const void* d_y32, uint64_t n,
                                   int32_t* ok, void* hip_stream);
int32_t kzg_verify_proof_batch_group_dev(const kzg_ctx* ctx, const void* const* d_proofs48, const void* const* d_commitments48, const void* const* d_z32,
                                         const void* const* d_y32, const uint64_t* n_local, int32_t* ok, void* const* hip_streams);

/*
 * Introspection: the 48-byte encodings of the monomial G1 setup points [tau^j]_1, first <= j < first + count, first + count <= 64.
 * A Setup<4096, 65> file carries the Lagrange form only; the context derives these 64 on the device as the commitments of the
 * blobs of X^j (element i = roots_brp[i]^j) through its own commitment path, on whichever table stands then -- ONCE, in its first
 * kzg_verify_cell_proof_batch[_each][_dev], kzg_g1_monomial_lincomb or kzg_ctx_g1_monomial call (64 commitments, about a millisecond), not in kzg_ctx_create: a
 * context that never verifies cells launches nothing for them.  Point 0 is the G1 generator.  They are the fixed terms of cell
 * verification's second lincomb; a group context's members each derive and hold a copy (this call reads member 0's).
 */
int32_t kzg_ctx_g1_monomial(const kzg_ctx* ctx, uint32_t first, uint32_t count, uint8_t* out48);

/*
 * verify_cell_kzg_proof_batch of specs/fulu/polynomial-commitments-sampling.md (EIP-7594, PeerDAS) with c-kzg-4844's argument shape:
 * n (commitment, cell index, cell, proof) tuples, ONE commitment per cell (a caller with many cells of one blob repeats it; the same
 * tuple may occur more than once).  Every array has n items, contiguous: 48 bytes per point, a uint64 per index, 2048 bytes per cell
 * (64 elements, 32 bytes big-endian each, as kzg_compute_cells_batch lays a cell out).  Device pointers (*_dev) are resident on ctx's
 * device and 16-byte aligned; the calls are synchronous like kzg_verify_proof_batch_dev (they return the boolean); hip_stream = NULL
 * is the default stream.
 *   Cell c holds p(h_c w64^brp6(i)), i < 64, with h_c = omega_8192^brp7(c) (coset_shift_for_cell).  With I_k the polynomial of degree
 *   < 64 through cell k and r the challenge:
 *   *ok = 1  iff  e(sum r^k proof_k, [tau^64]_2) ==
 *                 e(sum r^k commitment_k + sum r^k h_k^64 proof_k - sum_{j<64} S_j [tau^j]_1, G2),   S = sum_k r^k I_k,
 *            i.e. kzg_verify_proof_batch's check with z_k = h_k^64, y_k = 0, 64 monomial terms in place of the generator term and
 *            g2_monomial[64] in place of g2_monomial[1].  r is the ENGINE's challenge, bound to every input like the blob and points
 *            batches' (deviations Q1 / Q2): leaf k of the transcript tree = SHA-256(commitment48 || cell_index as 8 bytes big-endian
 *            || cell 2048 || proof48), and the seed message starts with the spec's cell domain "RCKZGCBATCH__V1_", so a cells root
 *            never reproduces a blob batch's r.  The boolean is therefore the spec's, up to the 2^-255 soundness error of the random
 *            combination; the transcript is not r-for-r the spec's.
 *   n == 0   *ok = 1.  A null required pointer with n > 0 returns KZG_FAIL_ARGUMENT.
 *   rejected inputs: the positive code of the FIRST rejected input, *ok = 0.  First = the spec's order of assertions lifted to
 *            arrays the way the other batch calls lift theirs: every cell index before any commitment, every commitment before any
 *            cell, every cell before any proof; the lowest index within the first kind that has an error.
 *              1. cell index >= 128                 KZG_ERR_CELL_INDEX
 *              2. commitment                        KZG_ERR_EC_* as kzg_g1_decompress_batch reports them
 *              3. cell: an element >= r             KZG_ERR_BLOB_INVALID_FIELD_ELEMENT
 *              4. proof                             KZG_ERR_EC_*
 *            The point at infinity is a valid commitment and a valid proof, as everywhere else in this ABI.  The length checks of
 *            the specification stay in the caller: the ABI takes a single n.
 * On a GROUP context the host-buffer call cuts the batch into contiguous shares, one per member, like kzg_verify_proof_batch; every
 * member's partial second lincomb carries its own monomial terms, so the partials add.  The *_dev call acts on member 0.
 * Per-item verdicts: kzg_verify_cell_proof_batch_each[_dev], below with the other *_each calls.
 * Not here: a sharded phase-1 entry point for cells and a *_group_dev form.  A caller who holds a block's list of commitments and not
 * one per cell uses kzg_verify_cell_proof_batch_rows, below: the commitments are decoded once each.
 */
int32_t kzg_verify_cell_proof_batch(const kzg_ctx* ctx, const uint8_t* commitments48, const uint64_t* cell_indices, const uint8_t* cells /* n * 2048 */,
                                    const uint8_t* proofs48, uint64_t n, int32_t* ok);
int32_t kzg_verify_cell_proof_batch_dev(const kzg_ctx* ctx, const void* d_commitments48, const void* d_cell_indices, const void* d_cells,
                                        const void* d_proofs48, uint64_t n, int32_t* ok, void* hip_stream);

/*
 * THE ROW-INDEXED FORM of kzg_verify_cell_proof_batch: what a PeerDAS node holds is a block's list of u commitments (one per blob) and
 * column sidecars whose cells each belong to one of them -- the consensus specs' earlier argument shape (row_commitments, row_indices,
 * column_indices, cells, proofs).  Tuple k is (commitments48[commitment_indices[k]], cell_indices[k], cells[k], proofs48[k]); the
 * commitments are u x 48 bytes, both index arrays n native uint64, cells and proofs as above.  Device pointers (*_dev) are resident on
 * ctx's device and 16-byte aligned.  u may exceed n, a commitment may be listed twice, and the point at infinity is a valid commitment.
 *   The check: with w_c = sum_{k : commitment_indices[k] = c} r^k,  sum_k r^k C_{index_k} = sum_{c<u} w_c C_c, so it is the check above
 *   with u commitment terms in place of n: the decoder runs on n + u points and the second lincomb has n + u + 64 terms.
 *   The transcript: leaf k stays SHA-256(commitment48 || cell index || cell || proof48) with the commitment looked up through the index,
 *   so root, seed and r are those of kzg_verify_cell_proof_batch on the expanded arrays and both sums are the same points: *ok and the
 *   return code are EXACTLY that call's whenever every commitment index is in range and every listed commitment is referenced.  The
 *   two calls are interchangeable.
 *   n == 0   *ok = 1, whatever u is.  u == 0 with n > 0 returns KZG_ERR_COMMITMENT_INDEX without a launch.  A null required pointer with
 *            n > 0 returns KZG_FAIL_ARGUMENT; commitments48 may be null only when u == 0.
 *   rejected inputs: first-error-wins over four entries, in this order, the lowest position within the first entry that has an error:
 *              1. indices, per item: commitment index >= u  KZG_ERR_COMMITMENT_INDEX, else cell index >= 128  KZG_ERR_CELL_INDEX
 *                 (an item with a bad commitment index is hashed with commitment 0; nothing is read out of bounds)
 *              2. commitments: ALL u, in list order, referenced or not   KZG_ERR_EC_* as kzg_g1_decompress_batch reports them
 *              3. cell: an element >= r             KZG_ERR_BLOB_INVALID_FIELD_ELEMENT
 *              4. proof                             KZG_ERR_EC_*
 * On a GROUP context the host-buffer call cuts the ITEMS into the members' usual contiguous shares; every member gets all u
 * commitments (each validates them: the merged record takes the list positions from the first share) and its slice of both index
 * arrays; the powers of r run over global item indices.  The *_dev call acts on member 0.
 * Cost of the weights: n u / 64 wave-steps of an index compare -- nothing for a block's shape (u up to a few hundred), about a
 * millisecond in the degenerate u ~ n = 65,536 case: there, use the per-cell call.
 * Per-item verdicts: kzg_verify_cell_proof_batch_rows_each[_dev], below behind the other *_each calls.
 * Not here: a *_group_dev form, and the GLV route (KATETH_AMD_VAR_GLV does not apply to this form).
 */
int32_t kzg_verify_cell_proof_batch_rows(const kzg_ctx* ctx, const uint8_t* commitments48 /* u * 48 */, uint64_t u, const uint64_t* commitment_indices /* n */,
                                         const uint64_t* cell_indices /* n */, const uint8_t* cells /* n * 2048 */, const uint8_t* proofs48 /* n * 48 */,
                                         uint64_t n, int32_t* ok);
int32_t kzg_verify_cell_proof_batch_rows_dev(const kzg_ctx* ctx, const void* d_commitments48, uint64_t u, const void* d_commitment_indices,
                                             const void* d_cell_indices, const void* d_cells, const void* d_proofs48, uint64_t n, int32_t* ok,
                                             void* hip_stream);
/*
 * Introspection: the row-indexed form's commitment scalars.  out_w32[c] = sum_{k<n, commitment_indices[k] = c} r^(first_index + k) mod
 * the group order, c < u, 32 bytes big-endian canonical; an unreferenced commitment gives zero.  It runs through the launch sequence
 * phase 2 uses -- k_batch_scalars for the powers, then k_cells_row_weights and its reduce launch -- which pins that kernel exactly.
 * Host memory in and out; synchronous; a group context answers from member 0.  r >= the modulus: KZG_ERR_FF_NOT_IN_FIELD; an index
 * >= u: KZG_ERR_COMMITMENT_INDEX.
 */
int32_t kzg_cell_row_weights(const kzg_ctx* ctx, const uint8_t* r32, uint64_t first_index, const uint64_t* commitment_indices /* n, HOST */, uint64_t n,
                             uint64_t u, uint8_t* out_w32 /* u * 32 */);

/*
 * PER-ITEM VERDICTS: which items of a batch are bad.  What a caller of the reference does when Setup::verify_blob_proof_batch is
 * false -- a loop over Setup::verify_blob_proof (src/kzg/setup.rs:208-221) or Setup::verify_proof (:96-113) -- answered from one
 * batch call.  Inputs as kzg_verify_blob_proof_batch(_dev) / kzg_verify_proof_batch(_dev); ok_each (n bytes), status (n x int32)
 * and ok are HOST memory in all four; the *_dev calls are synchronous like kzg_verify_*_batch_dev.
 *   status[i]  the code kzg_verify_blob_proof / kzg_verify_proof returns for item i ALONE: 0, or the positive KZG_ERR_* of that
 *              item's first rejected input in the single-item call's own parse order -- blob, commitment, proof
 *              (src/kzg/setup.rs:214-217) or proof, commitment, z, y (:103-109).
 *   ok_each[i] that call's *ok; 0 whenever status[i] != 0.
 *   *ok        1 iff every status[i] == 0 and every ok_each[i] == 1.
 *   n == 0     *ok = 1.  n == 1: the single-item call.
 *   return     0, or a negative KZG_FAIL_*.  A rejected ITEM never makes the call return a positive code: it is reported in
 *              status[], as the producers report theirs, and the other items still get their verdicts.
 * How: one phase 1 for the whole batch.  If no item is rejected, the batch check runs first and true means every item is true.
 * Otherwise the device computes per item A_i = [r_i] proof_i and B_i = [r_i] commitment_i + [r_i z_i] proof_i - [r_i y_i] G
 * (r_i = r^i as in the batch check; a rejected item contributes the point at infinity), sums both level by level into a tree,
 * and the host descends from the root spending one two-pairing check e(-A, [tau]_2) e(B, G2) == 1 per visited node: a node
 * that passes clears its range; of a failing node the left child is checked and, if it passes, the right child fails without
 * a check.  k false items among n cost at most 1 + 2 k ceil(log2 n) checks.  The leaf check is verify_proof_inner's equation
 * (src/kzg/setup.rs:84-94) scaled by r_i != 0: the reference's boolean exactly.  An inner node that hides a false item passes
 * with probability <= n / 2^255, the soundness statement of the batch call.
 * GROUP context, host-buffer calls: the batch is cut into the same contiguous shares as kzg_verify_*_batch; each member runs
 * the single-device call on its share as its own batch with its own challenge, writes its outputs in place, and *ok is the
 * AND (a verdict does not depend on r: nothing is merged).  The *_dev calls act on member 0.
 * kzg_verify_each_checks: the two-pairing checks these calls have spent on `ctx` so far (all members; measurement aid).
 * kzg_ctx_sessions_created: the verification sessions `ctx` and its members have ever constructed.  Every verification call takes a
 * pooled session and returns it on every exit, so calls made one at a time stop creating sessions after the first of each route; a
 * session that regrows its buffer is not a new one (measurement aid).
 */
int32_t kzg_verify_blob_proof_batch_each(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* proofs48, uint64_t n,
                                         uint8_t* ok_each, int32_t* status, int32_t* ok);
int32_t kzg_verify_blob_proof_batch_each_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_proofs48, uint64_t n,
                                             uint8_t* ok_each, int32_t* status, int32_t* ok, void* hip_stream);
int32_t kzg_verify_proof_batch_each(const kzg_ctx* ctx, const uint8_t* proofs48, const uint8_t* commitments48, const uint8_t* z32, const uint8_t* y32, uint64_t n,
                                    uint8_t* ok_each, int32_t* status, int32_t* ok);
int32_t kzg_verify_proof_batch_each_dev(const kzg_ctx* ctx, const void* d_proofs48, const void* d_commitments48, const void* d_z32, const void* d_y32, uint64_t n,
                                        uint8_t* ok_each, int32_t* status, int32_t* ok, void* hip_stream);
uint64_t kzg_verify_each_checks(const kzg_ctx* ctx);
uint64_t kzg_ctx_sessions_created(const kzg_ctx* ctx);

/*
 * PER-ITEM VERDICTS FOR CELLS: which (commitment, cell index, cell, proof) tuples of a kzg_verify_cell_proof_batch are bad -- what a
 * PeerDAS node needs to drop the cells, down-score their senders and reconstruct from the rest.  Inputs as
 * kzg_verify_cell_proof_batch(_dev); the outputs and the contract are those of the *_each calls above:
 *   status[i]  what kzg_verify_cell_proof_batch returns for item i ALONE: 0, or the positive code of its first rejected input in the
 *              order cell index, commitment, cell, proof.
 *   ok_each[i] that call's *ok; 0 whenever status[i] != 0.
 *   *ok        the AND of all verdicts.  n == 0: *ok = 1.  n == 1: the boolean call.  A null required pointer with n > 0 returns
 *              KZG_FAIL_ARGUMENT; a rejected item never makes the call return a positive code.
 *   ok_each (n bytes), status (n x int32) and ok are HOST memory; the *_dev call is synchronous.
 * How: nothing rejected -> the batch check runs first and true means every item is true.  Otherwise per item
 *   A_i = [r_i] proof_i      B_i = [r_i] commitment_i + [r_i h_i^64] proof_i - sum_{j<64} [v_ij] [tau^j]_1,   v_i = r_i I_i,
 * and e(-A_i, [tau^64]_2) e(B_i, G2) == 1 is the spec's single-cell check scaled by r_i != 0.  The two point terms are the leaves of
 * the two point trees above (z_i = h_i^64, y_i = 0).  The 64-term sum is NOT computed per item: the coefficient vectors v_i are the
 * leaves of a third sum tree (a node = 64 field elements, about 4 KiB of session storage per item), and the point sum_j [S_j] [tau^j]_1
 * is computed only for the nodes the host's descent asks for, O(k log n) of them for k false items, one wave per node.  The bound on
 * the two-pairing checks is the same 1 + 2 k ceil(log2 n).
 * GROUP context: the host-buffer call cuts the batch into the members' shares like the other *_each calls; the *_dev call acts on
 * member 0.  Not here: a kzg_verify_session_tree form for cells and a *_group_dev form.
 */
int32_t kzg_verify_cell_proof_batch_each(const kzg_ctx* ctx, const uint8_t* commitments48, const uint64_t* cell_indices, const uint8_t* cells /* n * 2048 */,
                                         const uint8_t* proofs48, uint64_t n, uint8_t* ok_each, int32_t* status, int32_t* ok);
int32_t kzg_verify_cell_proof_batch_each_dev(const kzg_ctx* ctx, const void* d_commitments48, const void* d_cell_indices, const void* d_cells,
                                             const void* d_proofs48, uint64_t n, uint8_t* ok_each, int32_t* status, int32_t* ok, void* hip_stream);

/*
 * PER-ITEM VERDICTS FOR THE ROW-INDEXED FORM: which cells of a kzg_verify_cell_proof_batch_rows are bad, from the shape block import
 * holds -- the list of u commitments is decoded once and nothing is expanded.  Inputs exactly as kzg_verify_cell_proof_batch_rows(_dev);
 * ok_each (n bytes), status (n x int32), commitment_status (u x int32, may be NULL) and ok are HOST memory; the *_dev call is synchronous.
 *   status[i]  commitment_indices[i] >= u: KZG_ERR_COMMITMENT_INDEX.  Otherwise what kzg_verify_cell_proof_batch returns for the
 *              expanded tuple (commitments48[commitment_indices[i]], cell_indices[i], cells[i], proofs48[i]) ALONE: 0, or its first
 *              rejection in the order cell index (KZG_ERR_CELL_INDEX), commitment (KZG_ERR_EC_*), cell
 *              (KZG_ERR_BLOB_INVALID_FIELD_ELEMENT), proof (KZG_ERR_EC_*).  A listed commitment that item i does not reference never
 *              touches item i -- the deliberate difference from the boolean rows call, which validates the whole list.
 *   ok_each[i] that call's *ok; 0 whenever status[i] != 0.
 *   commitment_status[c]  c < u: the decoder's code for listed commitment c, 0 or KZG_ERR_EC_*, referenced or not: how a caller learns
 *              that the LIST is bad.  May be NULL.
 *   *ok        1 iff every ok_each[i] == 1 AND every listed commitment is valid: 1 exactly when kzg_verify_cell_proof_batch_rows on the
 *              same arguments returns KZG_OK with *ok = 1, whether or not commitment_status is NULL.
 *   return     0, or a negative KZG_FAIL_*.  A rejected item or commitment never makes the call return a positive code.
 *   n == 0     *ok = 1, no launch, no output array is written, whatever u is.  u == 0 with n > 0: every status[i] =
 *              KZG_ERR_COMMITMENT_INDEX, every ok_each[i] = 0, *ok = 0, return 0, no launch.  u >= 2^31: KZG_FAIL_ARGUMENT.  A null
 *              required pointer with n > 0 returns KZG_FAIL_ARGUMENT; commitments48 may be null only when u == 0; only
 *              commitment_status is optional.  n == 1 obeys the same contract: the item sees only its own commitment.
 * Whenever every commitment index is in range, ok_each and status are byte for byte those of kzg_verify_cell_proof_batch_each on the
 * expanded arrays (the challenge is the same, so are both trees), and the bound on the two-pairing checks is the same
 * 1 + 2 k ceil(log2 n) (kzg_verify_each_checks).
 * How: the rows call's session (n + u decoded points).  No item and no listed commitment rejected -> the rows batch check runs first
 * and true settles every item.  Otherwise -- also when only an unreferenced commitment is bad: the batch check is never asked to sum a
 * rejected point -- the per-item terms are built with the commitment gathered through the item's index, and the descent is that of
 * the *_each calls above.
 * GROUP context: the host-buffer call cuts the ITEMS into the members' usual shares; every member gets all u commitments and its slice
 * of both index arrays, runs the single-device call on its share with its own challenge and writes ok_each and status in place;
 * commitment_status is written once, by the member that serves the first share (every member validates the same list); *ok is the AND.
 * The *_dev call acts on member 0.  Not here: a *_group_dev form, a kzg_verify_session_tree form, and the GLV route
 * (KATETH_AMD_VAR_GLV does not apply to this form).
 */
int32_t kzg_verify_cell_proof_batch_rows_each(const kzg_ctx* ctx, const uint8_t* commitments48 /* u * 48 */, uint64_t u,
                                              const uint64_t* commitment_indices /* n */, const uint64_t* cell_indices /* n */,
                                              const uint8_t* cells /* n * 2048 */, const uint8_t* proofs48 /* n * 48 */, uint64_t n,
                                              uint8_t* ok_each /* n, HOST */, int32_t* status /* n, HOST */,
                                              int32_t* commitment_status /* u, HOST, may be NULL */, int32_t* ok);
int32_t kzg_verify_cell_proof_batch_rows_each_dev(const kzg_ctx* ctx, const void* d_commitments48, uint64_t u, const void* d_commitment_indices,
                                                  const void* d_cell_indices, const void* d_cells, const void* d_proofs48, uint64_t n,
                                                  uint8_t* ok_each /* n, HOST */, int32_t* status /* n, HOST */,
                                                  int32_t* commitment_status /* u, HOST, may be NULL */, int32_t* ok, void* hip_stream);

/*
 * THE BLOB FORM (transaction-pool form): a blob's 128 cell proofs checked against the blob itself -- what an execution client does
 * with a blob transaction of network wrapper version 1 (BlobsBundleV2, engine_getBlobsV2; go-ethereum's kzg4844.VerifyCellProofs)
 * before its pool admits it.  n blobs (n * 131072 bytes), their n commitments (n * 48) and n * 128 cell proofs (n * 128 * 48; proof k
 * of blob b at 48 (128 b + k), the layout kzg_compute_cells_and_proofs_batch writes).  Device pointers (*_dev) are resident on ctx's
 * device and 16-byte aligned.  Synchronous like every verify call: the pairing is on the host.
 *   Definition: for canonical blobs *ok and the return code are EXACTLY those of kzg_verify_cell_proof_batch_rows with u = n and the
 *   same commitment list, commitment_indices[i] = i >> 7, cell_indices[i] = i & 127, cells = kzg_compute_cells_batch(blobs) and the
 *   same proofs: leaf i of the transcript is that call's leaf of tuple i, so root, seed, r and both sums are the same points.  The
 *   calls are interchangeable bit for bit.  What differs is what moves: no cell array and no index array exists on host or device;
 *   cells 0..63 are read out of the blob, cells 64..127 (128 KiB per blob) are computed into the session's workspace, and the
 *   host-buffer form uploads blobs, commitments and proofs only.
 *   n == 0   *ok = 1.  A null required pointer with n > 0 returns KZG_FAIL_ARGUMENT; so does n >= 2^24, whose 128 n items exceed what a
 *            cell verification session takes.
 *   rejected inputs: first-error-wins over three entries -- every blob before any commitment, every commitment before any proof, the
 *            lowest position within the first entry that has an error:
 *              1. blob: an element >= r      KZG_ERR_BLOB_INVALID_FIELD_ELEMENT (never taken for a blob of zeros)
 *              2. commitment                 KZG_ERR_EC_* as kzg_g1_decompress_batch reports them
 *              3. proof                      KZG_ERR_EC_*
 *            Index errors cannot occur.  The point at infinity is a valid commitment and a valid proof.
 * PER-BLOB VERDICTS (*_each): which transaction to drop.  ok_each (n bytes), status (n x int32) and ok are HOST memory in both.
 *   status[b]  blob b's own first code in the order blob, commitment, proof (lowest k); 0 if there is none.
 *   ok_each[b] 1 iff status[b] == 0 and the blob's 128 tuples pass on their own: for canonical, decodable inputs the AND of
 *              kzg_verify_cell_proof_batch_rows_each's 128 verdicts of that blob.
 *   *ok        1 iff every ok_each[b] == 1.  A rejected blob never makes the call return a positive code.
 *   A blob with a non-zero status contributes nothing to any sum -- all 128 of its items, not only a rejected proof's -- and its
 *   neighbours are judged as if it were absent.  The descent stops at the blobs (level 7 of the tree over the 128 n items): k bad
 *   blobs among n cost at most 1 + 2 k ceil(log2 n) two-pairing checks (kzg_verify_each_checks counts them with the others').
 * GROUP context: the host-buffer forms cut the BLOBS into the members' usual contiguous shares -- a blob is never split -- each member
 * gets its slice of commitments and proofs, and the powers of r run over global item indices; the *_each form runs each share as its
 * own batch, as the other *_each calls do.  The *_dev forms act on member 0.  Not here: a *_group_dev form, a phase-1 / session-tree
 * form, and the GLV route.
 */
int32_t kzg_verify_blob_cell_proofs_batch(const kzg_ctx* ctx, const uint8_t* blobs /* n * 131072 */, const uint8_t* commitments48 /* n * 48 */,
                                          const uint8_t* cell_proofs48 /* n * 128 * 48 */, uint64_t n, int32_t* ok);
int32_t kzg_verify_blob_cell_proofs_batch_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_cell_proofs48, uint64_t n,
                                              int32_t* ok, void* hip_stream);
int32_t kzg_verify_blob_cell_proofs_batch_each(const kzg_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* cell_proofs48, uint64_t n,
                                               uint8_t* ok_each /* n, HOST */, int32_t* status /* n, HOST */, int32_t* ok);
int32_t kzg_verify_blob_cell_proofs_batch_each_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_cell_proofs48, uint64_t n,
                                                   uint8_t* ok_each /* n, HOST */, int32_t* status /* n, HOST */, int32_t* ok, void* hip_stream);
/*
 * Introspection: the blob form's commitment scalars.  out_w32[b] = sum_{k<128} r^(first_index + 128 b + k) mod the group order, b <
 * n_blobs, 32 bytes big-endian canonical: kzg_cell_row_weights' values for commitment_indices[i] = i >> 7, through the launch sequence
 * phase 2 of the blob form uses (k_batch_scalars, then k_blob_weights).  Host memory in and out; synchronous; a group context answers
 * from member 0.  r >= the modulus: KZG_ERR_FF_NOT_IN_FIELD.
 */
int32_t kzg_blob_cell_weights(const kzg_ctx* ctx, const uint8_t* r32, uint64_t first_index, uint64_t n_blobs, uint8_t* out_w32 /* n_blobs * 32 */);

/*
 * Introspection: out96[k] = sum_{j<64} s_kj [tau^j]_1 for m vectors of 64 scalars (scalars32: m x 64 x 32 bytes big-endian, canonical;
 * a scalar >= r is rejected with KZG_ERR_FF_NOT_IN_FIELD), in kzg_verify_phase2_dev's point format: x || y big-endian, all-zero = the
 * point at infinity.  It runs through the kernel that computes the monomial term of a fetched node in the cells *_each calls, which
 * pins that kernel exactly; the monomial points are derived on first use like kzg_ctx_g1_monomial's.  Host memory in and out;
 * synchronous; a group context answers from member 0.
 */
int32_t kzg_g1_monomial_lincomb(const kzg_ctx* ctx, const uint8_t* scalars32, uint64_t m, uint8_t* out96);

/*
 * DEVICE-RESIDENT sharded calls on a GROUP context (kzg_config.devices / ndev): member k's share of the batch is resident on
 * member k's GPU -- what a node keeps when blobs arrive over the network or are produced on the devices, and the only way a
 * group verifies faster than PCIe delivers (host-buffer verification tops out near 0.37 M blobs/s per GPU, device-resident
 * verification runs at 4.4 M).  Every array argument has kzg_ctx_members(ctx) entries, indexed by member; the GLOBAL order of
 * the batch is member order (member 0's n_local[0] items first), which is what the powers r^i of the batch check and the
 * first-error-wins order (src/kzg/setup.rs:259-271: lowest global index of the first kind with an error) are taken over.
 * n_local[k] may be 0.  hip_streams may be NULL (every member's default stream) or one hipStream_t per member, created on that
 * member's device.
 *   commit / proof : enqueue on every member and return WITHOUT synchronising, like the *_dev calls
 *                    (src/kzg/setup.rs:167-171, 177-183 per item); results and per-item statuses stay on each member's device.
 *   verify         : synchronous like kzg_verify_blob_proof_batch_dev: per member hash, evaluation, decoding and transcript,
 *                    the members' roots seed ONE challenge, per member the two partial lincombs (bucket kernels start the
 *                    moment that member's decoder ends, as in the single-device call), one pairing check
 *                    (src/kzg/setup.rs:223-275).  Same boolean and same first-error code as the single-device call over the
 *                    concatenated batch.
 * On a single-device context they are the *_dev calls with one-element arrays.
 */
int32_t kzg_blob_to_commitment_batch_group_dev(const kzg_ctx* ctx, const void* const* d_blobs, const uint64_t* n_local, void* const* d_out48,
                                               void* const* d_status, void* const* hip_streams);
int32_t kzg_compute_blob_proof_batch_group_dev(const kzg_ctx* ctx, const void* const* d_blobs, const void* const* d_commitments48, const uint64_t* n_local,
                                               void* const* d_out48, void* const* d_status, void* const* hip_streams);
int32_t kzg_verify_blob_proof_batch_group_dev(const kzg_ctx* ctx, const void* const* d_blobs, const void* const* d_commitments48,
                                              const void* const* d_proofs48, const uint64_t* n_local, int32_t* ok, void* const* hip_streams);

/*
 * Multi-GPU batch verification.  Blobs are sharded by
 * contiguous global index ranges; each rank runs
 *   phase 1 : per-item work on its n_local items (validation, challenge z_i,
 *             evaluation y_i) and a 32-byte transcript root over them;
 *             err6 = {blob_idx, blob_code, commitment_idx, commitment_code,
 *             proof_idx, proof_code} with LOCAL index of the first rejected
 *             input of each kind (-1 = none), so the caller can rebuild the
 *             reference's first-error-wins order (src/kzg/setup.rs:259-271)
 *             across ranks;
 *   (the caller gathers the `world` roots -- RCCL all-gather of 32 B per rank)
 *   phase 2 : the rank's share of the two random linear combinations, with the
 *             challenge seeded by ALL roots; 2 x 96 bytes (affine big-endian
 *             x||y, all-zero = infinity);
 *   finish  : on one rank, sums the gathered partials (192 B per rank) and runs
 *             the single two-pairing check.
 * A session owns its device buffers and stream and may not be used concurrently; kzg_verify_session_destroy hands it
 * back to the context's pool (steady-state verification allocates nothing).
 */
typedef struct kzg_verify_session kzg_verify_session;
int32_t kzg_verify_phase1_dev(const kzg_ctx* ctx, const void* d_blobs, const void* d_commitments48, const void* d_proofs48, uint64_t n_local,
                              uint8_t* out_root32, int32_t* err6, kzg_verify_session** session, void* hip_stream);
int32_t kzg_verify_phase2_dev(kzg_verify_session* session, const uint8_t* roots32, uint64_t world, uint64_t first_index, uint64_t n_total,
                              uint8_t* out192);
void kzg_verify_session_destroy(kzg_verify_session* session);
/* introspection (tests, debugging): the Fiat-Shamir challenges z_i (Blob::challenge, src/blob.rs:78-97) and evaluations
 * y_i (Polynomial::evaluate, src/kzg/poly.rs:10-33) phase 1 computed for items [first, first+count), 32 B big-endian each */
int32_t kzg_verify_session_zy(kzg_verify_session* session, uint64_t first, uint64_t count, uint8_t* out_z32, uint8_t* out_y32);
int32_t kzg_verify_batch_finish(const kzg_ctx* ctx, const uint8_t* partials192, uint64_t world, int32_t* ok);
/*
 * The per-item terms of a session after phase 1 and their sum trees (the device half of kzg_verify_*_batch_each, for the
 * per-rank protocol and for tests).  kzg_verify_session_tree seeds r exactly as kzg_verify_phase2_dev does and builds, in the
 * session, A_i and B_i of every LOCAL item with r_i = r^(first_index + i) and both sum trees; a rejected item contributes the
 * point at infinity to both.  kzg_verify_session_tree_range returns A || B summed over the local items [lo, hi), composed
 * from whole tree nodes, as 2 x 96 bytes in kzg_verify_phase2_dev's format: with every item accepted, the range [0, n_local)
 * is byte for byte that call's out192 on the same session.  The tree storage (about 50 MB at 65,536 items) belongs to the
 * session: allocated on first use, handed back to the pool with it; a caller that never asks for it pays nothing.
 */
int32_t kzg_verify_session_tree(kzg_verify_session* session, const uint8_t* roots32, uint64_t world, uint64_t first_index, uint64_t n_total);
int32_t kzg_verify_session_tree_range(kzg_verify_session* session, uint64_t lo, uint64_t hi, uint8_t* out192);
/*
 * Phase 1 of kzg_verify_proof_batch for a rank's n_local tuples (z and y from the caller instead of the hash and the
 * evaluation): err8 = {proof_idx, proof_code, commitment_idx, commitment_code, z_idx, z_code, y_idx, y_code}, LOCAL index of
 * the first rejected input of each kind (-1 = none), found on the device.  The session is an ordinary kzg_verify_session:
 * kzg_verify_phase2_dev, kzg_verify_session_zy (the parsed z_i, y_i; zero for a rejected one), kzg_verify_batch_finish and
 * kzg_verify_session_destroy work on it unchanged, and its root is the one kzg_verify_phase1_dev returns for blobs whose
 * challenges and evaluations are these z and y.
 */
int32_t kzg_verify_proof_phase1_dev(const kzg_ctx* ctx, const void* d_proofs48, const void* d_commitments48, const void* d_z32, const void* d_y32,
                                    uint64_t n_local, uint8_t* out_root32, int32_t* err8, kzg_verify_session** session, void* hip_stream);

/*
 * Synthetic-input generator used by bench.py and the parity tests
 * (counterpart of Blob::random, src/blob.rs:66-76, but seeded):
 *   element(b, i) = SHA-256(seed_le64 || b_le64 || i_le32) mod r, 32 B big-endian
 * Fills n blobs with indices first_index .. first_index+n-1 into d_blobs.
 */
int32_t kzg_synth_blobs_dev(const kzg_ctx* ctx, uint64_t seed, uint64_t first_index, uint64_t n, void* d_blobs, void* hip_stream);

/*
 * Device micro-benchmarks (measurement support for bench.py's roofline object):
 * runs `iters` dependent Fp Montgomery multiplications per lane on `lanes`
 * lanes -- with the multiply of the fixed-base MSM kernel the context uses
 * (radix-2^28 limbs by default) -- and returns the elapsed milliseconds
 * measured with HIP events.
 */
int32_t kzg_microbench_fp_mul(const kzg_ctx* ctx, uint64_t lanes, uint64_t iters, float* ms);
/*
 * The VALU issue interval the roofline is priced with: SIMD cycles per wave-instruction of v_mad_u64_u32 (the
 * instruction 76-80 % of the MSM / evaluation / decoding streams consist of) with `waves_per_simd` (1..4) co-resident
 * waves on every SIMD of the chip, 8 independent chains per wave, `iters` x 32 instructions per lane (median over the
 * waves, by the shader-clock counter), and the shader clock in GHz the chip sustains under that load (shader-clock
 * ticks per 100-MHz real-time tick).  floor of a kernel = SQ_INSTS_VALU / SIMDs x cycles_per_inst / clock.
 */
int32_t kzg_microbench_valu_issue(const kzg_ctx* ctx, uint32_t waves_per_simd, uint32_t iters, double* cycles_per_inst, double* clock_ghz);
/*
 * The shader clock under a REAL workload: kzg_clock_probe_launch enqueues eight sleeping single-wave workgroups (one per
 * XCD) on a stream of the context's own; for `duration_us` they compare the shader-clock counter with the 100-MHz real-time
 * counter while the caller's kernels run beside them (a probe wave needs a handful of registers and issues one instruction
 * every 2 us).  kzg_clock_probe_read waits for them and returns the mean / lowest / highest XCD clock in GHz.
 */
int32_t kzg_clock_probe_launch(const kzg_ctx* ctx, uint32_t duration_us);
int32_t kzg_clock_probe_read(const kzg_ctx* ctx, double* ghz_mean, double* ghz_min, double* ghz_max);

/*
 * On-device self-test of the hand-scheduled multiply: every lane multiplies
 * `iters` pseudo-random operand pairs with the inline-asm v_mad_u64_u32 chains
 * and with a plain-C multiply the compiler schedules (hazard wait states and
 * all); *mismatches counts disagreements (Fp and Fr).  The same operands also go
 * through the carry-free radix-2^28 (Fp) and radix-2^29 (Fr) multipliers of the
 * hot loops (product, squaring, two products with one reduction) and must agree
 * with the 32-bit-limb result.  Expected: 0.
 */
int32_t kzg_selftest_field_mul(const kzg_ctx* ctx, uint64_t lanes, uint64_t iters, uint64_t* mismatches);
/* Test hook for the guard described at KZG_FAIL_HOST: throws std::bad_alloc (kind 0), std::runtime_error (1) or an int (2) inside
 * an entry point; expected return KZG_FAIL_HOST with the exception's text in kzg_last_error().  Touches no GPU. */
int32_t kzg_selftest_exception_guard(int32_t kind);

/*
 * Kernel timing for bench.py's `roofline` object: between begin and end every
 * launch of the timed kernel classes (below) is bracketed by HIP events on the
 * stream it is launched on.  end() synchronises those events and returns the
 * summed milliseconds and the number of launches of the fixed-base MSM kernel
 * (k_msm_comb30).  A profiling interval must not overlap calls still being
 * enqueued from other threads (their unfinished event pairs are skipped).
 */
int32_t kzg_profile_begin(const kzg_ctx* ctx);
int32_t kzg_profile_end(const kzg_ctx* ctx, double* msm_ms_total, uint64_t* msm_launches);
/*
 * The same for every timed kernel class: ms[k] / launches[k] for k < KZG_PROF_KINDS (kzg_profile_kind_name(k) names
 * the class: the fixed-base MSM, the SHA-256 challenge, the barycentric evaluation, point decoding, the quotient
 * kernel, the variable-base MSMs of batch verification, lane-sum trees + encoding).  Ends the profiling interval.
 */
#define KZG_PROF_KINDS 8
int32_t kzg_profile_end_kinds(const kzg_ctx* ctx, double* ms, uint64_t* launches);
const char* kzg_profile_kind_name(int32_t kind);
/* mixed additions the fixed-base MSM performs per blob: 256 bit planes x (blocks per 64 points) x 64 (table above) */
uint64_t kzg_ctx_adds_per_blob(const kzg_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* KATETH_AMD_H */
