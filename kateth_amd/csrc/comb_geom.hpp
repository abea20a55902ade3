// Geometry of the fixed-base subset-sum comb (msm_comb.cuh): plain host/device data and index arithmetic, no kernels -- shared by
// the host code of every translation unit; the kernels themselves are compiled ONCE (engine.hip owns msm_comb.cuh).
#pragma once
#include <stdint.h>

#include "field.cuh"

namespace kzg {

struct CombGeom {
  uint32_t nb;    // blocks per 64 points: 3 (22 + 21 + 21 points), 4 (16 each), 8 (8 each), 16 (4 each)
  uint32_t G;     // plane groups = tables; H = 256 / G planes each
  uint32_t H;
  uint32_t lpg;   // lanes per group = 64 / G
  uint32_t ep64;  // table entries per 64 points (one group): sum over the blocks of 2^(t-1)
  uint32_t epg;   // entries per group = 64 * ep64
  uint32_t fair;  // s > 0: the two waves of a SIMD trade issue priority every 2^s shader cycles (k_msm_comb30); 0: hardware default (oldest first)
};

KZG_HD uint32_t comb_tbits(uint32_t nb, uint32_t r) { return nb == 3u ? (r == 0u ? 22u : 21u) : 64u / nb; }
KZG_HD uint32_t comb_point_off(uint32_t nb, uint32_t r) { return nb == 3u ? (r == 0u ? 0u : (r == 1u ? 22u : 43u)) : r * (64u / nb); }
KZG_HD uint32_t comb_entry_off(uint32_t nb, uint32_t r) {
  return nb == 3u ? (r == 0u ? 0u : (r == 1u ? (1u << 21) : (1u << 21) + (1u << 20))) : r << (64u / nb - 1u);
}
KZG_HD CombGeom comb_make_geom(uint32_t nb, uint32_t G) {
  CombGeom g;
  g.nb = nb;
  g.G = G;
  g.H = 256u / G;
  g.lpg = 64u / G;
  g.ep64 = nb == 3u ? (1u << 22) : nb << (64u / nb - 1u);
  g.epg = 64u * g.ep64;
  g.fair = 20u;
  return g;
}
KZG_HD uint64_t comb_table_entries(const CombGeom& g) { return (uint64_t)g.G * g.epg; }

// ---- the lane walk of k_msm_comb30 --------------------------------------------------------------------------------------
// A lane owns blocks [b0, b0 + bpo) of the 64 nb blocks and visits them once per plane, planes counting down.  CombWalk is
// the part of a position that is THE SAME IN EVERY LANE of a wave -- plane h, block counter s -- and, when every lane's
// first block opens a chunk (b0 % nb == 0: "wide" shapes, bpo a multiple of 4 nb, every production shape), also the block
// within its chunk r and the number of chunks dq past the lane's first chunk q0 = b0 / nb.  The kernel keeps it in scalar
// registers and adds the lane's q0 where a position is used.  CombLanePos is the per-lane (chunk, block in chunk) the other
// shapes need instead of (dq, r).
struct CombWalk {
  uint32_t h, s, r, dq;
};
// blocks per lane of a launch shape, and whether the shape is wide
KZG_HD uint32_t comb_blocks_per_lane(const CombGeom& g, uint32_t splits, uint32_t lpb) { return (64u * g.nb) / (splits * (lpb / g.G)); }
KZG_HD bool comb_shape_is_wide(const CombGeom& g, uint32_t splits, uint32_t lpb) { return comb_blocks_per_lane(g, splits, lpb) % (4u * g.nb) == 0u; }
// k_msm_comb30 is compiled per kind of shape, so that neither instance carries the other's registers and branches: the product
// launches COMB_SHAPE_WIDE or COMB_SHAPE_NARROW; COMB_SHAPE_ANY decides at run time (the test-only timed instance).
enum : int { COMB_SHAPE_ANY = 0, COMB_SHAPE_WIDE = 1, COMB_SHAPE_NARROW = 2 };
struct CombLanePos {
  uint32_t q, r;
};
KZG_HD void comb_walk_start(CombWalk& w, uint32_t H) {
  w.h = H - 1u;
  w.s = 0;
  w.r = 0;
  w.dq = 0;
}
// to the next step; true when the lane wrapped to its first block on the next plane down
KZG_HD bool comb_walk_advance(CombWalk& w, uint32_t nb, uint32_t bpo) {
  w.s++;
  w.r++;
  if (w.r == nb) {
    w.r = 0;
    w.dq++;
  }
  if (w.s != bpo) return false;
  w.s = 0;
  w.r = 0;
  w.dq = 0;
  w.h--;
  return true;
}
KZG_HD void comb_lane_advance(CombLanePos& p, uint32_t nb, bool wrapped, uint32_t b0) {
  p.r++;
  if (p.r == nb) {
    p.r = 0;
    p.q++;
  }
  if (wrapped) {
    p.q = b0 / nb;
    p.r = b0 % nb;
  }
}
// Wide shapes: a lane's chunks come in aligned groups of four whose masks are ONE 32-byte load (mb0..mb3), issued when w opens
// a group; the step at w cuts its pattern from slot dq % 4 of them.
KZG_HD bool comb_walk_loads_masks(const CombWalk& w) { return w.r == 0u && (w.dq & 3u) == 0u; }
KZG_HD uint32_t comb_walk_mask_slot(const CombWalk& w) { return w.dq & 3u; }
// Horner doubling in front of the step at w: on a lane's first block of every plane but the first
KZG_HD bool comb_walk_doubles(const CombWalk& w, uint32_t H) { return w.s == 0u && w.h != H - 1u; }
// largest `splits` the geometry supports: a lane must own a whole number of blocks
KZG_HD uint32_t comb_max_splits(const CombGeom& g) { return (64u * g.nb) / g.lpg; }

// ---- a walk that starts at step t (the second pass of a balanced launch, below) ----------------------------------------------
// the position of step t of a lane's bpo * H steps; the lane's own (chunk, block) there for the shapes that carry one
KZG_HD void comb_walk_at(CombWalk& w, uint32_t H, uint32_t nb, uint32_t bpo, uint32_t t) {
  w.h = H - 1u - t / bpo;
  w.s = t % bpo;
  w.r = w.s % nb;  // meaningful in wide shapes only (b0 % nb == 0)
  w.dq = w.s / nb;
}
KZG_HD void comb_lane_at(CombLanePos& p, uint32_t nb, uint32_t b0, const CombWalk& w) {
  p.q = (b0 + w.s) / nb;
  p.r = (b0 + w.s) % nb;
}
// Wide shapes: the first of the four chunks (counted from the lane's first chunk, like dq) whose masks the 32-byte load covering
// the step at w holds.  A walk that starts inside a group of four issues that load itself; from then on comb_walk_loads_masks.
KZG_HD uint32_t comb_walk_mask_base(const CombWalk& w) { return w.dq & ~3u; }

// ---- balance plan of a half-wave launch (lpb = 32, splits = 1) ------------------------------------------------------------
// Workgroups are dealt round-robin to the chip's eight XCDs, which do not clock alike: CLASS r = unit % 8 ends early or late as
// a whole.  A plan pairs classes (partner is an involution) and lets the slower member of a pair leave out its LAST shed[r]
// steps -- plane 0 of the lane's group, blocks [bpo - d, bpo): nothing is doubled after them, so d <= bpo - 1 -- which the unit
// of class partner[r] of the same group of eight consecutive units then walks in a second pass, from the identity, on the
// giver's two blobs, into a second array of lane sums.  No wave reads what another wave of the launch writes.  One byte per
// class, packed: by value in two scalar register pairs.
struct CombBalance {
  uint64_t partner;  // byte r = partner of class r
  uint64_t shed;     // byte r = steps class r leaves to its partner (non-zero for at most one member of a pair)
};
constexpr uint64_t COMB_BALANCE_IDENTITY = 0x0706050403020100ull;
KZG_HD CombBalance comb_balance_none() { return CombBalance{COMB_BALANCE_IDENTITY, 0}; }
KZG_HD uint32_t comb_balance_partner(const CombBalance& b, uint32_t r) { return (uint32_t)(b.partner >> (8u * r)) & 0xffu; }
KZG_HD uint32_t comb_balance_shed(const CombBalance& b, uint32_t r) { return (uint32_t)(b.shed >> (8u * r)) & 0xffu; }
KZG_HD bool comb_balance_empty(const CombBalance& b) { return b.shed == 0; }
// a plan the kernel may run with lanes of bpo blocks: an involution without fixed points that shed, sheds <= bpo - 1 and on one side only
KZG_HD bool comb_balance_valid(const CombBalance& b, uint32_t bpo) {
  for (uint32_t r = 0; r < 8u; r++) {
    const uint32_t p = comb_balance_partner(b, r), d = comb_balance_shed(b, r);
    if (p >= 8u || comb_balance_partner(b, p) != r) return false;
    if (d != 0u && (p == r || d + 1u > bpo || comb_balance_shed(b, p) != 0u)) return false;
  }
  return true;
}
// The timing record of one launch, 64-bit words: earliest start and, per class, latest end of its units on the constant 100-MHz
// counter, and how many units reported.  k_msm_comb30 folds into it, the lane-sum kernel behind it hands it to the host and
// clears it (msm_reduce_kernels.cuh).
enum : uint32_t { COMB_REC_START = 0, COMB_REC_END = 1, COMB_REC_UNITS = 9, COMB_REC_WORDS = 10 };
// units [0, comb_balance_units(n)) of a half-wave launch over n blobs take part: whole groups of eight units with all sixteen blobs
KZG_HD uint64_t comb_balance_units(uint64_t n) { return (n / 16u) * 8u; }

}  // namespace kzg
