// CPU build of the comb kernel's lane walk (kateth_amd/csrc/comb_geom.hpp: CombWalk, CombLanePos and their functions -- the
// code k_msm_comb30 compiles) beside the per-lane walker it replaced, for tests/test_comb_walker_host.py.
//
// Both models go through the kernel's pipeline order -- fetch the mask of step w, p1 = w, advance, gather the entry of p1 --
// and record for every step of a lane, in the order the additions happen:
//   h, s, q, r, entry offset of block r, doubling flag, mask slot, and the (plane, chunk) of the mask the pattern is cut from
// as the mask registers hold it at that moment (a load tags the registers it fills), so a gather that ran after the load
// which overwrites its mask, or cut from the wrong slot, shows as a wrong tag.
#include <stdint.h>

#include "../../kateth_amd/csrc/comb_geom.hpp"

using namespace kzg;

namespace {

constexpr int FIELDS = 9;
struct Tag {
  uint32_t plane, chunk;
};
struct Shape {
  CombGeom g;
  uint32_t bpo, b0, kbase, total;
  bool wide;
};

bool make_shape(Shape& sh, uint32_t nb, uint32_t G, uint32_t lpb, uint32_t splits, uint32_t lane, uint32_t split) {
  sh.g = comb_make_geom(nb, G);
  const uint32_t lpg = lpb / G;
  if (lpg == 0 || (64u * nb) % (splits * lpg) != 0u) return false;
  const uint32_t l = lane % lpb;
  const uint32_t owner = split * lpg + l % lpg;
  sh.bpo = comb_blocks_per_lane(sh.g, splits, lpb);
  sh.b0 = owner * sh.bpo;
  sh.kbase = (l / lpg) * sh.g.H;
  sh.total = sh.g.H * sh.bpo;
  sh.wide = comb_shape_is_wide(sh.g, splits, lpb);
  return true;
}

void emit(uint32_t* o, uint32_t h, uint32_t s, uint32_t q, uint32_t r, uint32_t nb, bool dbl, uint32_t slot, Tag t) {
  o[0] = h;
  o[1] = s;
  o[2] = q;
  o[3] = r;
  o[4] = comb_entry_off(nb, r);
  o[5] = dbl ? 1u : 0u;
  o[6] = slot;
  o[7] = t.plane;
  o[8] = t.chunk;
}

// ---- the walker before: every field per lane, the mask chosen by a four-way select on (q - q0) % 4 -------------------------
struct OldWalker {
  uint32_t h, s, q, r;
};
uint32_t run_old(const Shape& sh, uint32_t* out) {
  const uint32_t nb = sh.g.nb, bpo = sh.bpo, b0 = sh.b0;
  OldWalker w{sh.g.H - 1u, 0u, b0 / nb, b0 % nb};
  auto advance = [&]() {
    w.s++;
    w.r++;
    if (w.r == nb) {
      w.r = 0;
      w.q++;
    }
    if (w.s == bpo) {
      w.s = 0;
      w.h--;
      w.q = b0 / nb;
      w.r = b0 % nb;
    }
  };
  const uint32_t q0 = b0 / nb;
  Tag mb[4] = {{~0u, ~0u}, {~0u, ~0u}, {~0u, ~0u}, {~0u, ~0u}};
  auto fetch = [&]() {
    if (sh.wide) {
      if (w.r == 0u && ((w.q - q0) & 3u) == 0u)
        for (uint32_t k = 0; k < 4; k++) mb[k] = Tag{sh.kbase + w.h, w.q + k};
    } else {
      mb[0] = Tag{sh.kbase + w.h, w.q};
    }
  };
  uint32_t n = 0;
  OldWalker p1;
  auto gather = [&]() {
    const uint32_t k = sh.wide ? ((p1.q - q0) & 3u) : 0u;
    emit(out + FIELDS * n++, p1.h, p1.s, p1.q, p1.r, nb, p1.s == 0u && p1.h != sh.g.H - 1u, k, mb[k]);
  };
  fetch();
  p1 = w;
  advance();
  gather();
  if (sh.total > 1u) {
    fetch();
    p1 = w;
    advance();
  }
  for (uint32_t t = 0; t < sh.total; t++) {
    if (t + 1u < sh.total) {
      gather();
      if (t + 2u < sh.total) {
        fetch();
        p1 = w;
        advance();
      }
    }
  }
  return n;
}

// ---- the walk as the kernel does it now: comb_next_mask / comb_gather of msm_comb.cuh, on tags instead of masks -------------
struct NewLane {
  CombWalk w, p1;
  CombLanePos lw, lp1;
  Tag mb[4];
};
void next_mask(const Shape& sh, NewLane& s, uint32_t q0) {
  if (sh.wide) {
    if (comb_walk_loads_masks(s.w))
      for (uint32_t k = 0; k < 4; k++) s.mb[k] = Tag{sh.kbase + s.w.h, q0 + s.w.dq + k};
  } else {
    s.mb[0] = Tag{sh.kbase + s.w.h, s.lw.q};
  }
  s.p1 = s.w;
  const bool wrapped = comb_walk_advance(s.w, sh.g.nb, sh.bpo);
  if (!sh.wide) {
    s.lp1 = s.lw;
    comb_lane_advance(s.lw, sh.g.nb, wrapped, sh.b0);
  }
}
uint32_t run_new(const Shape& sh, uint32_t* out) {
  const uint32_t nb = sh.g.nb, q0 = sh.b0 / nb;
  NewLane s;
  comb_walk_start(s.w, sh.g.H);
  s.lw = CombLanePos{q0, sh.b0 % nb};
  s.lp1 = s.lw;
  for (auto& t : s.mb) t = Tag{~0u, ~0u};
  uint32_t n = 0;
  auto gather = [&]() {
    const bool dbl = comb_walk_doubles(s.p1, sh.g.H);
    if (sh.wide) {
      const uint32_t k = comb_walk_mask_slot(s.p1);
      emit(out + FIELDS * n++, s.p1.h, s.p1.s, q0 + s.p1.dq, s.p1.r, nb, dbl, k, s.mb[k]);
    } else {
      emit(out + FIELDS * n++, s.p1.h, s.p1.s, s.lp1.q, s.lp1.r, nb, dbl, 0u, s.mb[0]);
    }
  };
  next_mask(sh, s, q0);
  gather();
  if (sh.total > 1u) next_mask(sh, s, q0);
  for (uint32_t t = 0; t < sh.total; t++) {
    if (t + 1u < sh.total) {
      gather();
      if (t + 2u < sh.total) next_mask(sh, s, q0);
    }
  }
  return n;
}

}  // namespace

extern "C" {
// steps of one lane; 0 when the shape is not a launch shape
uint32_t hmw_steps(uint32_t nb, uint32_t G, uint32_t lpb, uint32_t splits) {
  Shape sh;
  return make_shape(sh, nb, G, lpb, splits, 0, 0) ? sh.total : 0u;
}
int32_t hmw_is_wide(uint32_t nb, uint32_t G, uint32_t lpb, uint32_t splits) {
  Shape sh;
  return make_shape(sh, nb, G, lpb, splits, 0, 0) ? (sh.wide ? 1 : 0) : -1;
}
// which = 0: the walker before, 1: the walk of comb_geom.hpp.  out: hmw_steps() x 9 words.  Returns the steps written.
uint32_t hmw_walk(uint32_t which, uint32_t nb, uint32_t G, uint32_t lpb, uint32_t splits, uint32_t lane, uint32_t split, uint32_t* out) {
  Shape sh;
  if (!make_shape(sh, nb, G, lpb, splits, lane, split)) return 0;
  return which == 0u ? run_old(sh, out) : run_new(sh, out);
}
}
