// Multi-GPU behind the C ABI (`kzg_ctx_create(g1, g2, devices[], ndev, &ctx)`).
//
// A GROUP context is member 0 -- a complete single-device context -- plus one peer context per further listed device, each
// holding the full tables (the setup is 4096 + 65 points: replicated, never sharded).  Blobs are independent in all three
// operations (the reference walks them one by one: src/kzg/setup.rs:235-242), so the host-buffer entry points cut a batch
// into contiguous ranges, one per member, run the single-device implementation of each range on a host thread of its own and
// let it write straight into the caller's buffers: no collective, no gather (on_members, engine_internal.hpp: the producer's
// own lambda advances its pointers to the range).  The only cross-member step is the end of batch
// verification (src/kzg/setup.rs:152-160): every member returns its transcript root and first-error records, the roots of
// ALL members seed the batch challenge, every member returns its two partial sums with GLOBAL powers r^i, and one member sums
// the partials and runs the single pairing check -- the same phase1 / roots / phase2 / finish protocol that
// kateth_amd/dist.py drives across processes with RCCL, here inside one process.
#include "engine_internal.hpp"
#include "multi_split.hpp"

using kzg::multi::Share;
using kzg::multi::merged_first_error;

namespace {

inline const kzg_ctx* member_of(const kzg_ctx* ctx, uint32_t k) { return k == 0 ? ctx : ctx->peers[k - 1]; }

// the shares of a call over this group's members (multi_split.hpp); calls smaller than the group start at a rotating member
std::vector<Share> shares_of(const kzg_ctx* ctx, uint64_t n) {
  const uint32_t S = 1u + (uint32_t)ctx->peers.size();
  const uint32_t rotate = (n && n < S) ? ctx->rr.fetch_add((uint32_t)n, std::memory_order_relaxed) : 0u;
  return kzg::multi::shares_of(n, S, rotate);
}

}  // namespace

int32_t group_create(const uint8_t* g1_lagrange, const uint8_t* g2_monomial, const kzg_config* cfg, kzg_ctx** out) {
  *out = nullptr;
  const int32_t visible = kzg_device_count();
  if (visible < 0) return visible;
  std::vector<int> devices;
  if (cfg->ndev == KZG_ALL_DEVICES) {
    for (int d = 0; d < visible; d++) devices.push_back(d);
  } else {
    if (!cfg->devices) return fail(KZG_FAIL_ARGUMENT, "kzg_config.devices is null with ndev != KZG_ALL_DEVICES");
    if (cfg->ndev > 64) return fail(KZG_FAIL_ARGUMENT, "kzg_config.ndev: at most 64 members");
    for (uint32_t k = 0; k < cfg->ndev; k++) {
      if (cfg->devices[k] < 0 || cfg->devices[k] >= visible) return fail(KZG_FAIL_ARGUMENT, "device ordinal out of range in kzg_config.devices");
      devices.push_back(cfg->devices[k]);
    }
  }
  // every member decodes the setup and builds its tables on its own device, all at once (one host thread per member)
  std::vector<kzg_ctx*> members(devices.size(), nullptr);
  const int32_t rc = run_on_helpers((uint32_t)devices.size(), [&](uint32_t k) -> int32_t {
    return ctx_create_single(g1_lagrange, g2_monomial, cfg, devices[k], &members[k]);
  });
  if (rc) {
    const ErrorSnapshot keep = error_snapshot();
    for (kzg_ctx* m : members)
      if (m) kzg_ctx_destroy(m);
    error_publish(keep);
    return rc;
  }
  kzg_ctx* head = members[0];
  head->peers.assign(members.begin() + 1, members.end());
  *out = head;
  return 0;
}

int32_t on_group_members(const kzg_ctx* ctx, uint64_t n, const MemberCall& fn) {
  const std::vector<Share> shares = shares_of(ctx, n);
  return run_on_helpers((uint32_t)shares.size(), [&](uint32_t j) -> int32_t { return fn(member_of(ctx, shares[j].member), shares[j].first, shares[j].count); });
}

// Setup::verify_proof (src/kzg/setup.rs:96-113) is one item: any member serves it
int32_t multi_verify_proof(const kzg_ctx* ctx, const uint8_t* proof48, const uint8_t* commitment48, const uint8_t* z32, const uint8_t* y32, int32_t* ok) {
  const uint32_t S = 1u + (uint32_t)ctx->peers.size();
  return verify_proof_single(member_of(ctx, ctx->rr.fetch_add(1u, std::memory_order_relaxed) % S), proof48, commitment48, z32, y32, ok);
}

// Setup::verify_blob_proof_batch (src/kzg/setup.rs:247-275), Setup::verify_proof_batch (:115-161) or verify_cell_proof_batch from host buffers over the members'
// shares; one share is exactly the single-device call on that member.  Otherwise every share runs the single-device phase 1
// (verify_phase1) on its member; the challenge is seeded by all the shares' roots, so r differs from the single-device call's while the
// boolean and the first-error code are the same.
// The blob form of the cells kind (in.from_blobs, kzg_verify_blob_cell_proofs_batch): the shares are cut over the BLOBS -- a blob's 128
// items are never split -- every array advances by the share's blobs, and the powers of r still run over global item indices.
int32_t multi_verify_batch(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, int32_t* ok) {
  *ok = 0;
  const uint64_t per = in.from_blobs ? KZG_CELLS_PER_EXT_BLOB : 1;  // items per unit of the split
  const std::vector<Share> shares = shares_of(ctx, n / per);
  if (shares.size() == 1) return verify_batch_single(member_of(ctx, shares[0].member), in, n, nullptr, nullptr, ok);
  const uint32_t W = (uint32_t)shares.size();
  const int kinds = facts(in.kind).entries;
  const size_t stride = 2 * (size_t)kinds;
  std::vector<uint8_t> roots(32 * (size_t)W), partials(192 * (size_t)W);
  std::vector<int32_t> err(stride * W);
  std::vector<kzg_verify_session*> sessions(W, nullptr);  // phase 1 hands them to this call
  int32_t rc = run_on_helpers(W, [&](uint32_t j) -> int32_t {
    const kzg_ctx* m = member_of(ctx, shares[j].member);
    if (hipSetDevice(m->device) != hipSuccess) return fail(KZG_FAIL_HIP, "hipSetDevice failed");
    const VerifyInputs share = in.from_blobs ? in.blob_share(shares[j].first, shares[j].count) : in.advanced(shares[j].first);
    return verify_phase1(m, share, shares[j].count * per, nullptr, roots.data() + 32 * (size_t)j, err.data() + stride * j, &sessions[j]);
  });
  // the row-indexed cells form: every member validated the WHOLE commitment list, so that entry of a record carries list positions,
  // not item positions -- it must not get a share's offset: the first share's (offset 0) stands for all
  if (rc == 0 && in.rows() && !in.from_blobs)
    for (uint32_t j = 1; j < W; j++) err[stride * j + 2] = -1;
  int32_t code = 0;
  if (rc == 0 && in.from_blobs) {
    // the blob form's order over the cells kind's record: blob (the cell entry: item positions), commitment (blob positions), proof
    // (item positions).  The shares are contiguous in blobs, so within an entry positions in either unit order the same way: all in items
    std::vector<Share> items(shares);
    std::vector<int32_t> err3(6 * (size_t)W);
    for (uint32_t j = 0; j < W; j++) {
      items[j].first *= per;
      items[j].count *= per;
      const int32_t* e = err.data() + stride * j;
      const int32_t rec[6] = {e[4], e[5], e[2] < 0 ? -1 : e[2] * (int32_t)per, e[3], e[6], e[7]};
      memcpy(err3.data() + 6 * (size_t)j, rec, sizeof rec);
    }
    code = merged_first_error(items, err3.data(), 3);
  } else if (rc == 0) {
    code = merged_first_error(shares, err.data(), kinds);
  }
  if (rc == 0 && code == 0)
    rc = run_on_helpers(W, [&](uint32_t j) -> int32_t {
      return kzg_verify_phase2_dev(sessions[j], roots.data(), W, shares[j].first * per, n, partials.data() + 192 * (size_t)j);
    });
  {  // handing a session back may fail on its own: the error the caller is told about stays the first one
    const ErrorSnapshot keep = error_snapshot();
    for (kzg_verify_session* s : sessions) kzg_verify_session_destroy(s);
    error_publish(keep);
  }
  if (rc || code) return rc ? rc : code;
  return verify_batch_finish(ctx, partials.data(), W, in.kind, ok);
}

// Per-item verdicts (kzg_verify_*_batch_each) over the members: the same contiguous shares, each member's share its own batch with its
// own challenge -- an item's verdict does not depend on r, so the outputs land in place and nothing is merged but the AND.  The
// row-indexed cells form: every member gets the whole commitment list and validates it, so each member's boolean already carries the
// list's verdict and the list's statuses are written once, by the member that serves the first share.
// The blob form (in.from_blobs): shares of whole blobs, and the outputs are per blob.
int32_t multi_verify_each(const kzg_ctx* ctx, const VerifyInputs& in, uint64_t n, const VerifyEach& each, int32_t* ok) {
  *ok = 0;
  const uint64_t per = in.from_blobs ? KZG_CELLS_PER_EXT_BLOB : 1;
  const std::vector<Share> shares = shares_of(ctx, n / per);
  std::vector<int32_t> oks(shares.size(), 0);
  const int32_t rc = run_on_helpers((uint32_t)shares.size(), [&](uint32_t j) -> int32_t {
    const Share& sh = shares[j];
    const VerifyEach out{each.ok_each + sh.first, each.status + sh.first, j == 0 ? each.commitment_status : nullptr};
    const VerifyInputs share = in.from_blobs ? in.blob_share(sh.first, sh.count) : in.advanced(sh.first);
    return verify_batch_single(member_of(ctx, sh.member), share, sh.count * per, nullptr, &out, &oks[j]);
  });
  if (rc) return rc;
  *ok = 1;
  for (int32_t o : oks) *ok &= o;
  return 0;
}

// ---- device-resident sharded calls (include/kateth_amd.h: kzg_*_group_dev) -------------------------------------------------
// Member k's share is resident on member k's GPU.  Commitments and proofs only ENQUEUE (like the *_dev calls), one pooled host
// thread per member so that the members' launches go out side by side; nothing is gathered -- results stay where they were
// computed.  Batch verification: engine_verify.hip (verify_group_dev).
namespace {
template <class Call>
int32_t group_enqueue(const kzg_ctx* ctx, const uint64_t* n_local, Call&& call) {
  const uint32_t S = 1u + (uint32_t)ctx->peers.size();
  std::vector<uint32_t> busy;
  for (uint32_t k = 0; k < S; k++)
    if (n_local[k]) busy.push_back(k);
  return run_on_helpers((uint32_t)busy.size(), [&](uint32_t j) -> int32_t { return call(busy[j], member_of(ctx, busy[j])); });
}
}  // namespace

extern "C" int32_t kzg_blob_to_commitment_batch_group_dev(const kzg_ctx* ctx, const void* const* d_blobs, const uint64_t* n_local, void* const* d_out48,
                                                          void* const* d_status, void* const* hip_streams) try {
  if (!ctx || !d_blobs || !n_local || !d_out48 || !d_status) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return group_enqueue(ctx, n_local, [&](uint32_t k, const kzg_ctx* m) -> int32_t {
    return kzg_blob_to_commitment_batch_dev(m, d_blobs[k], n_local[k], d_out48[k], d_status[k], hip_streams ? hip_streams[k] : nullptr);
  });
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_compute_blob_proof_batch_group_dev(const kzg_ctx* ctx, const void* const* d_blobs, const void* const* d_commitments48,
                                                          const uint64_t* n_local, void* const* d_out48, void* const* d_status, void* const* hip_streams) try {
  if (!ctx || !d_blobs || !d_commitments48 || !n_local || !d_out48 || !d_status) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return group_enqueue(ctx, n_local, [&](uint32_t k, const kzg_ctx* m) -> int32_t {
    return kzg_compute_blob_proof_batch_dev(m, d_blobs[k], d_commitments48[k], n_local[k], d_out48[k], d_status[k], hip_streams ? hip_streams[k] : nullptr);
  });
} catch (...) {
  return abi_exception();
}

// the GroupDevShare list of the two *_group_dev calls: member k's pointers (an array the kind does not have is null) and its global range
namespace {
int32_t verify_group_shares(const kzg_ctx* ctx, VerifyKind kind, const void* const* blobs, const void* const* commitments48, const void* const* proofs48,
                            const void* const* z32, const void* const* y32, const uint64_t* n_local, void* const* hip_streams, int32_t* ok) {
  *ok = 0;
  const uint32_t S = 1u + (uint32_t)ctx->peers.size();
  auto at = [](const void* const* a, uint32_t k) { return a ? (const uint8_t*)a[k] : nullptr; };
  std::vector<GroupDevShare> shares;
  uint64_t total = 0;
  for (uint32_t k = 0; k < S; k++) {
    if (n_local[k] == 0) continue;
    const VerifyInputs in{kind, at(blobs, k), at(commitments48, k), at(proofs48, k), at(z32, k), at(y32, k), false};
    if (in.any_null()) return fail(KZG_FAIL_ARGUMENT, "null device pointer for a member with items");
    shares.push_back(GroupDevShare{member_of(ctx, k), in, total, n_local[k], hip_streams ? (hipStream_t)hip_streams[k] : nullptr});
    total += n_local[k];
  }
  return verify_group_dev(ctx, shares, total, ok);
}
}  // namespace

extern "C" int32_t kzg_verify_blob_proof_batch_group_dev(const kzg_ctx* ctx, const void* const* d_blobs, const void* const* d_commitments48,
                                                         const void* const* d_proofs48, const uint64_t* n_local, int32_t* ok, void* const* hip_streams) try {
  if (!ctx || !ok || !d_blobs || !d_commitments48 || !d_proofs48 || !n_local) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return verify_group_shares(ctx, VerifyKind::BLOBS, d_blobs, d_commitments48, d_proofs48, nullptr, nullptr, n_local, hip_streams, ok);
} catch (...) {
  return abi_exception();
}

extern "C" int32_t kzg_verify_proof_batch_group_dev(const kzg_ctx* ctx, const void* const* d_proofs48, const void* const* d_commitments48,
                                                    const void* const* d_z32, const void* const* d_y32, const uint64_t* n_local, int32_t* ok,
                                                    void* const* hip_streams) try {
  if (!ctx || !ok || !d_proofs48 || !d_commitments48 || !d_z32 || !d_y32 || !n_local) return fail(KZG_FAIL_ARGUMENT, "null argument");
  return verify_group_shares(ctx, VerifyKind::POINTS, nullptr, d_commitments48, d_proofs48, d_z32, d_y32, n_local, hip_streams, ok);
} catch (...) {
  return abi_exception();
}
