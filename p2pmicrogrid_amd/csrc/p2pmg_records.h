// p2pmg_records.h — one agent-step of the records the last episode launch left on the device, read from
// either layout: the plain [T][A] arrays (general, tile, shared, role, rule and DQN launches) or the
// packed 32-B rows of episode_fast_kernel / episode_sq16_kernel.  Shared by the post-passes over those
// records (p2pmg_summary.hip, p2pmg_dayprof.hip); device code only.
#pragma once
#include "p2pmg_internal.h"

namespace p2pmg {
namespace {

// One packed record row of episode_fast_kernel / episode_sq16_kernel (FastRec in p2pmg_fastmath.h)
struct PackedRow {
  float reward, cost, grid, p2p, tin;
  uint32_t actions;  // byte r: action of round r
  uint32_t bins, ips;
};
static_assert(sizeof(PackedRow) == kFastRecBytes, "the packed record row is 32 B");

struct Step {
  float cost, reward, grid, p2p, tin, load, pv;
  uint32_t act;  // the final round's action
};

template <bool PACKED>
__device__ __forceinline__ Step load_step(const SummaryParams& p, size_t t, size_t a) {
  Step s;
  const size_t k = t * (size_t)p.A + a;
  if constexpr (PACKED) {
    const uint4* row = reinterpret_cast<const uint4*>(p.rec_pack) + 2 * k;
    const uint4 lo = row[0];
    const uint2 hi = *reinterpret_cast<const uint2*>(row + 1);
    s.reward = __uint_as_float(lo.x);
    s.cost = __uint_as_float(lo.y);
    s.grid = __uint_as_float(lo.z);
    s.p2p = __uint_as_float(lo.w);
    s.tin = __uint_as_float(hi.x);
    s.act = (hi.y >> (8 * p.R)) & 0xFFu;
  } else {
    s.cost = p.cost[k];
    s.reward = p.has_reward ? p.reward[k] : 0.0f;
    s.grid = p.grid[k];
    s.p2p = p.p2p[k];
    s.tin = p.tin[k];
    s.act = p.action[(t * (size_t)(p.R + 1) + (size_t)p.R) * (size_t)p.A + a];
  }
  if (!p.has_reward) s.reward = 0.0f;
  const float2 lp = p.prof[k];
  s.load = lp.x;
  s.pv = lp.y;
  return s;
}

}  // namespace
}  // namespace p2pmg
