// p2pmg_dayprof.cpp — see p2pmg_dayprof.h.  No HIP call and no device.
#include "p2pmg_dayprof.h"

#include <algorithm>

namespace p2pmg {

const char* dayprof_resolve(const p2pmg_day_profile_args* a, int T, int S, DayProfRange* r) {
  if (!a || !r || T < 1 || S < 1) return "bad arguments";
  if (a->period < 0 || a->period > T) return "period outside [0, T]";
  r->P = a->period ? a->period : T;
  const int64_t tc = a->step_count < 0 ? (int64_t)T - a->step_first : a->step_count;
  if (a->step_first < 0 || a->step_first > T || tc < 0 || a->step_first + tc > T)
    return "step range outside [0, T]";
  const int64_t sc = a->scen_count < 0 ? (int64_t)S - a->scen_first : a->scen_count;
  if (a->scen_first < 0 || a->scen_first > S || sc < 0 || a->scen_first + sc > S)
    return "scenario range outside [0, S]";
  r->t0 = a->step_first, r->t1 = (int)(a->step_first + tc);
  r->s0 = a->scen_first, r->s1 = (int)(a->scen_first + sc);
  if (a->n_groups < 0) return "n_groups is negative";
  r->labelled = a->groups != nullptr;
  int32_t lo = 0, hi = 0;
  if (a->groups) {
    lo = hi = a->groups[0];
    for (int s = 1; s < S; ++s) lo = std::min(lo, a->groups[s]), hi = std::max(hi, a->groups[s]);
  }
  if (hi == INT32_MAX) return "a label outside [-1, n_groups)";
  r->G = a->n_groups ? a->n_groups : std::max(hi, 0) + 1;
  if (lo < -1 || hi >= r->G) return "a label outside [-1, n_groups)";
  return nullptr;
}

std::vector<int64_t> dayprof_histogram(const int32_t* groups, const DayProfRange& r) {
  std::vector<int64_t> hist((size_t)r.G, 0);
  if (!groups) {
    hist[0] = r.s1 - r.s0;
    return hist;
  }
  for (int s = r.s0; s < r.s1; ++s)
    if (groups[s] >= 0) ++hist[(size_t)groups[s]];
  return hist;
}

const char* dayprof_check_samples(const int64_t* hist, int G, int64_t steps, int P) {
  int64_t most = 0;
  for (int g = 0; g < G; ++g) most = std::max(most, hist[g]);
  const int64_t per_slot = (steps + P - 1) / P;  // steps of the range that share a slot, at most
  if (most > 0 && per_slot > 0 && most > kDayProfMaxSamples / per_slot)  // most * per_slot > 2^24, without the product
    return "more than 2^24 samples in one (group, slot, role): split by scenario range and merge the parts";
  return nullptr;
}

DayProfPlan dayprof_plan(int G, int P, int N, int64_t agents, int steps, size_t budget) {
  DayProfPlan p;
  budget = std::min(budget, kDayProfTileMax);
  p.tile_agents = (kDayProfBlock / N) * N;
  p.n_tiles = (int)((agents + p.tile_agents - 1) / p.tile_agents);
  const size_t slot_bytes = (size_t)G * (size_t)N * kDayProfRowBytes;  // one slot of every group
  const int64_t cap = (int64_t)(budget / slot_bytes);                  // slots a tile may hold
  p.lds = cap >= 1;
  p.fold = p.lds && P <= cap;
  const int64_t max_slice = !p.lds || p.fold ? steps : std::min<int64_t>(cap, steps);
  const int64_t pairs = (int64_t)p.n_tiles * steps;
  const int64_t per_block = std::max<int64_t>(kDayProfMinPairs, (pairs + kDayProfTargetBlocks - 1) / kDayProfTargetBlocks);
  p.tiles_per_run = (int)std::min<int64_t>({(int64_t)p.n_tiles, (int64_t)kDayProfMaxRun, per_block});
  p.n_runs = (p.n_tiles + p.tiles_per_run - 1) / p.tiles_per_run;
  p.slice_steps = (int)std::min<int64_t>(max_slice, (per_block + p.tiles_per_run - 1) / p.tiles_per_run);
  p.n_slices = (steps + p.slice_steps - 1) / p.slice_steps;
  if (p.lds) {
    p.tile_slots = p.fold ? P : p.slice_steps;
    p.tile_bytes = slot_bytes * (size_t)p.tile_slots;
  }
  return p;
}

}  // namespace p2pmg
