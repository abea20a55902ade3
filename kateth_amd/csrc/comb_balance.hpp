// The balance plan of the comb's half-wave launches (comb_geom.hpp CombBalance) as the host makes it: plain functions on plain
// data, no HIP -- engine.hip calls them under the context's balance lock, tests/hostmath_walker builds them for the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "comb_geom.hpp"

namespace kzg {

constexpr double COMB_BALANCE_DAMP = 0.5;        // a shed moves this fraction of the way to its target per record
constexpr double COMB_BALANCE_HYSTERESIS = 4.0;  // steps: a new pairing must beat the standing one's predicted end by this much

inline CombBalance comb_balance_pack(const uint32_t partner[8], const uint32_t shed[8]) {
  CombBalance b{0, 0};
  for (uint32_t r = 0; r < 8u; r++) {
    b.partner |= (uint64_t)(partner[r] & 0xffu) << (8u * r);
    b.shed |= (uint64_t)(shed[r] & 0xffu) << (8u * r);
  }
  return b;
}

// The next plan from one launch's record.  t[r]: time from the launch's earliest start to the latest end of class r (any unit, all
// positive); `ran`: the plan that launch ran under; a lane walked `total` steps, bpo of them per plane.
//   * tau = mean(t) / total is the launch's time per step, and nat[r] = t[r] + tau * (steps r shed - steps r took over) is what
//     class r would have needed for its own work;
//   * candidate pairing: slowest with fastest by nat.  It replaces the pairing of `ran` only where that one has no pairs or its
//     predicted end (the largest pair mean, a lone class counting for itself) is worse by COMB_BALANCE_HYSTERESIS steps: noise
//     of a step or two between near-equal classes does not reshuffle the pairs;
//   * a pair (a, b) sheds, signed, (nat[a] - nat[b]) / (2 tau) steps from a to b at equal ends; the plan moves from the shed it
//     ran with COMB_BALANCE_DAMP of the way there, rounded, clamped to bpo - 1.  A pair whose shed comes out 0 is dissolved, so
//     classes that read alike never pair and equal times give the empty plan.
inline CombBalance comb_balance_next(const CombBalance& ran, const double t[8], uint32_t total, uint32_t bpo) {
  double mean = 0;
  for (uint32_t r = 0; r < 8u; r++) {
    if (!(t[r] > 0)) return comb_balance_none();
    mean += t[r] / 8.0;
  }
  if (total == 0u || bpo < 2u || !comb_balance_valid(ran, bpo)) return comb_balance_none();
  const double tau = mean / total;
  double nat[8];
  uint32_t old_partner[8];
  bool old_pairs = false;
  for (uint32_t r = 0; r < 8u; r++) {
    old_partner[r] = comb_balance_partner(ran, r);
    old_pairs = old_pairs || old_partner[r] != r;
    nat[r] = t[r] + tau * ((double)comb_balance_shed(ran, r) - (double)comb_balance_shed(ran, old_partner[r]));
  }
  uint32_t order[8];
  for (uint32_t r = 0; r < 8u; r++) order[r] = r;
  for (uint32_t i = 1; i < 8u; i++)  // insertion sort, ascending, stable: ties keep the class order
    for (uint32_t j = i; j > 0u && nat[order[j]] < nat[order[j - 1u]]; j--) {
      const uint32_t x = order[j];
      order[j] = order[j - 1u];
      order[j - 1u] = x;
    }
  uint32_t cand[8];
  for (uint32_t i = 0; i < 4u; i++) {
    cand[order[i]] = order[7u - i];
    cand[order[7u - i]] = order[i];
  }
  auto predicted_end = [&](const uint32_t* partner) {
    double worst = 0;
    for (uint32_t r = 0; r < 8u; r++) {
      const double e = 0.5 * (nat[r] + nat[partner[r]]);
      worst = e > worst ? e : worst;
    }
    return worst;
  };
  const bool keep = old_pairs && predicted_end(old_partner) <= predicted_end(cand) + COMB_BALANCE_HYSTERESIS * tau;
  const uint32_t* pairing = keep ? old_partner : cand;
  uint32_t partner[8], shed[8];
  for (uint32_t r = 0; r < 8u; r++) {
    partner[r] = r;
    shed[r] = 0;
  }
  for (uint32_t a = 0; a < 8u; a++) {
    const uint32_t b = pairing[a];
    if (b <= a) continue;
    const double before = old_partner[a] == b ? (double)comb_balance_shed(ran, a) - (double)comb_balance_shed(ran, b) : 0.0;
    const double target = (nat[a] - nat[b]) / (2.0 * tau);
    const double x = before + COMB_BALANCE_DAMP * (target - before);
    long d = (long)(target >= before ? floor(x + 0.5) : ceil(x - 0.5));  // to the nearest step, a tie towards the target: a shed of 1 can go
    const long cap = bpo - 1u < 255u ? (long)bpo - 1 : 255;  // a shed is a byte of the plan
    d = d > cap ? cap : (d < -cap ? -cap : d);
    if (d == 0) continue;
    partner[a] = b;
    partner[b] = a;
    shed[d > 0 ? a : b] = (uint32_t)labs(d);
  }
  return comb_balance_pack(partner, shed);
}

// KATETH_AMD_COMB_BALANCE=<partner>:<shed> -- eight digits, digit r the partner of class r, then eight comma-separated step counts,
// e.g. 10325476:0,47,0,0,5,0,0,0.  False when the text is no such plan (the caller then checks it against the launch's bpo).
inline bool comb_balance_parse(const char* text, CombBalance& out) {
  if (text == nullptr || strlen(text) < 10u || text[8] != ':') return false;
  uint32_t partner[8], shed[8];
  for (uint32_t r = 0; r < 8u; r++) {
    if (text[r] < '0' || text[r] > '7') return false;
    partner[r] = (uint32_t)(text[r] - '0');
  }
  const char* p = text + 9;
  for (uint32_t r = 0; r < 8u; r++) {
    char* end = nullptr;
    const unsigned long v = strtoul(p, &end, 10);
    if (end == p || v > 255ul || *end != (r == 7u ? '\0' : ',')) return false;
    shed[r] = (uint32_t)v;
    p = end + 1;
  }
  out = comb_balance_pack(partner, shed);
  return true;
}

}  // namespace kzg
