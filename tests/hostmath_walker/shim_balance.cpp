// CPU build of what a balanced launch of k_msm_comb30 adds (kateth_amd/csrc/comb_geom.hpp: comb_walk_at, comb_lane_at,
// comb_walk_mask_base; kateth_amd/csrc/comb_balance.hpp: the planner), for tests/test_comb_balance_host.py.
//
// hmb_walk runs steps [first, first + count) of a lane through the kernel's pipeline order -- position the walk, issue the first
// mask load whatever the position, gather, next mask, then per step: gather the next entry, fetch the mask after it -- and
// records per step the nine fields of shim_walker.cpp: h, s, q, r, entry offset of block r, doubling flag, mask slot, and the
// (plane, chunk) tag of the mask register the pattern is cut from as the registers hold it at that moment.
#include <stdint.h>

#include "../../kateth_amd/csrc/comb_balance.hpp"
#include "../../kateth_amd/csrc/comb_geom.hpp"

using namespace kzg;

namespace {

constexpr int FIELDS = 9;
struct Tag {
  uint32_t plane, chunk;
};
struct Lane {
  CombWalk w, p1;
  CombLanePos lw, lp1;
  Tag mb[4];
};

}  // namespace

extern "C" {

// returns the steps written (count), 0 when the shape is not a launch shape or the range is not inside the walk
uint32_t hmb_walk(uint32_t nb, uint32_t G, uint32_t lpb, uint32_t splits, uint32_t lane, uint32_t split, uint32_t first, uint32_t count, uint32_t* out) {
  const CombGeom g = comb_make_geom(nb, G);
  const uint32_t lpg = lpb / G;
  if (lpg == 0 || (64u * nb) % (splits * lpg) != 0u) return 0;
  const uint32_t l = lane % lpb, owner = split * lpg + l % lpg;
  const uint32_t bpo = comb_blocks_per_lane(g, splits, lpb), b0 = owner * bpo, kbase = (l / lpg) * g.H, total = g.H * bpo;
  const bool wide = comb_shape_is_wide(g, splits, lpb);
  if (count == 0u || first + count > total) return 0;
  const uint32_t q0 = b0 / nb;
  Lane s;
  for (auto& t : s.mb) t = Tag{~0u, ~0u};
  auto next_mask = [&](bool is_first) {
    if (wide) {
      if (is_first || comb_walk_loads_masks(s.w)) {
        const uint32_t base = is_first ? comb_walk_mask_base(s.w) : s.w.dq;
        for (uint32_t k = 0; k < 4; k++) s.mb[k] = Tag{kbase + s.w.h, q0 + base + k};
      }
    } else {
      s.mb[0] = Tag{kbase + s.w.h, s.lw.q};
    }
    s.p1 = s.w;
    const bool wrapped = comb_walk_advance(s.w, nb, bpo);
    if (!wide) {
      s.lp1 = s.lw;
      comb_lane_advance(s.lw, nb, wrapped, b0);
    }
  };
  uint32_t n = 0;
  auto gather = [&]() {
    uint32_t* o = out + FIELDS * n++;
    const uint32_t k = wide ? comb_walk_mask_slot(s.p1) : 0u;
    const uint32_t q = wide ? q0 + s.p1.dq : s.lp1.q, r = wide ? s.p1.r : s.lp1.r;
    o[0] = s.p1.h;
    o[1] = s.p1.s;
    o[2] = q;
    o[3] = r;
    o[4] = comb_entry_off(nb, r);
    o[5] = comb_walk_doubles(s.p1, g.H) ? 1u : 0u;
    o[6] = k;
    o[7] = s.mb[k].plane;
    o[8] = s.mb[k].chunk;
  };
  comb_walk_at(s.w, g.H, nb, bpo, first);
  comb_lane_at(s.lw, nb, b0, s.w);
  s.lp1 = s.lw;
  next_mask(true);
  gather();
  if (count > 1u) next_mask(false);
  for (uint32_t t = 0; t < count; t++) {
    if (t + 1u < count) {
      gather();
      if (t + 2u < count) next_mask(false);
    }
  }
  return n;
}

// comb_balance_next on unpacked plans; returns 1 when the plan it gives is valid for bpo
int32_t hmb_plan_next(const uint32_t* ran_partner, const uint32_t* ran_shed, const double* t, uint32_t total, uint32_t bpo, uint32_t* partner, uint32_t* shed) {
  const CombBalance next = comb_balance_next(comb_balance_pack(ran_partner, ran_shed), t, total, bpo);
  for (uint32_t r = 0; r < 8u; r++) {
    partner[r] = comb_balance_partner(next, r);
    shed[r] = comb_balance_shed(next, r);
  }
  return comb_balance_valid(next, bpo) ? 1 : 0;
}

// KATETH_AMD_COMB_BALANCE's forced form; 1 when the text parses
int32_t hmb_plan_parse(const char* text, uint32_t bpo, uint32_t* partner, uint32_t* shed, int32_t* valid) {
  CombBalance b = comb_balance_none();
  if (!comb_balance_parse(text, b)) return 0;
  for (uint32_t r = 0; r < 8u; r++) {
    partner[r] = comb_balance_partner(b, r);
    shed[r] = comb_balance_shed(b, r);
  }
  *valid = comb_balance_valid(b, bpo) ? 1 : 0;
  return 1;
}
}
