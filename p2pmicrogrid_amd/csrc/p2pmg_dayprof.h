// p2pmg_dayprof.h — the host side of p2pmg_day_profile that needs no device: the check of its arguments,
// P and G, the overflow bound and the launch shape for a tile budget (p2pmg_dayprof.cpp), plus the two
// number maps the kernels (p2pmg_dayprof.hip) share with the host: fix and the f32 <-> ordered-u32 image.
// No HIP call, so a program without a GPU can check all of it under a sanitizer (tests/dayprof_check.cpp,
// built and run by tests/test_cpu_day_profile_device.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "p2pmg.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define P2PMG_HD __host__ __device__
#else
#define P2PMG_HD
#endif

namespace p2pmg {

constexpr int kDayProfSums = 16, kDayProfExtrema = 8, kDayProfComSums = 4, kDayProfComExtrema = 2;
constexpr size_t kDayProfRowBytes = kDayProfSums * 8 + kDayProfExtrema * 4;  // one (group, slot, agent) row of a tile
constexpr int kDayProfBlock = 256;                   // threads of a workgroup = agents of a full tile
constexpr size_t kDayProfTileDefault = 32u << 10;    // P2PMG_DAYPROF_TILE_BYTES when unset
constexpr size_t kDayProfTileMax = 64u << 10;        // what a workgroup may ask of LDS without an attribute
constexpr int64_t kDayProfMaxSamples = (int64_t)1 << 24;  // per (group, slot) row: no sum reaches 2^63
constexpr int kDayProfShiftW = 16, kDayProfShiftDeg = 24, kDayProfShiftMoney = 28;
// the launch shape aims at this many workgroups, none with fewer (tile, step) pairs than kDayProfMinPairs,
// and a workgroup walks at most kDayProfMaxRun agent tiles per step (their per-agent rows stay in L2)
constexpr int kDayProfTargetBlocks = 1024, kDayProfMinPairs = 32, kDayProfMaxRun = 16;

// fix(x, k) = rint(f64(x) * 2^k) to nearest even as int64; f32 x 2^k is exact in f64, so one rounding.
// |x| < 2^(62 - k) (p2pmg.h: magnitudes below 2^23 W, 2^15 degC, 2^11 money).
P2PMG_HD inline long long dayprof_fix(float x, int k) {
  const double scaled = (double)x * (double)(1ull << k);
  // rint to nearest even (v_rndne_f64 on the device, the default rounding mode on the host), then an exact
  // conversion: what __double2ll_rn and llrint give
  return (long long)__builtin_rint(scaled);
}

// The order-preserving image of a non-NaN f32: a < b  <=>  ord(a) < ord(b) as unsigned, -0.0 below +0.0
// (the kernels add +0.0f first, so zeros arrive as +0.0).  dayprof_unord is its inverse.
P2PMG_HD inline uint32_t dayprof_ord(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
P2PMG_HD inline float dayprof_unord(uint32_t u) {
  const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  float x;
  __builtin_memcpy(&x, &b, 4);
  return x;
}
constexpr uint32_t kDayProfOrdPosInf = 0xFF800000u;  // dayprof_ord(+inf): where a minimum starts
constexpr uint32_t kDayProfOrdNegInf = 0x007FFFFFu;  // dayprof_ord(-inf): where a maximum starts

// The arguments resolved against a context of T steps and S scenarios.
struct DayProfRange {
  int G = 1, P = 1;
  int t0 = 0, t1 = 0, s0 = 0, s1 = 0;  // half-open step and scenario ranges
  bool labelled = false;               // groups given: the kernels read one label per scenario
};
// Null and *r, or what is wrong (P2PMG_E_INVALID): period outside [0, T], a range outside [0, T] / [0, S],
// n_groups < 0, a label outside [-1, G).  Reads groups[0 .. S) when it is not null, and nothing else.
const char* dayprof_resolve(const p2pmg_day_profile_args* a, int T, int S, DayProfRange* r);
// Scenarios per group among [s0, s1) (label -1 counted nowhere): hist [G].  groups null: all in group 0.
std::vector<int64_t> dayprof_histogram(const int32_t* groups, const DayProfRange& r);
// Null, or the overflow message: a (group, slot) row would hold more than kDayProfMaxSamples samples,
// max(hist) * ceil(steps / P).
const char* dayprof_check_samples(const int64_t* hist, int G, int64_t steps, int P);

// The launch shape of dayprof_agent_kernel.  The agents [s0 N, s1 N) are cut into tiles of tile_agents (a
// multiple of N, so a lane keeps its agent position from tile to tile); the steps [t0, t1) into slices of
// slice_steps.  Workgroup (x, y) walks the tiles [x tiles_per_run, ...) over the steps of slice y, and
// holds, when lds, an LDS tile of G * tile_slots * N rows it flushes once.
struct DayProfPlan {
  int lds = 0;          // 1: accumulate in an LDS tile; 0: no slot of G * N rows fits the budget, global atomics
  int fold = 0;         // lds: 1: the tile holds all P slots, row slot = t % P; 0: it holds the slice's own
                        // steps, row slot = t - (first step of the slice) < tile_slots <= P
  int tile_slots = 0;   // lds: slots per group the tile holds
  int tile_agents = 0, n_tiles = 0, tiles_per_run = 0, n_runs = 0;
  int slice_steps = 0, n_slices = 0;
  size_t tile_bytes = 0;  // lds: G * tile_slots * N * kDayProfRowBytes <= budget
};
// N in [1, kDayProfBlock], agents = (s1 - s0) * N and steps = t1 - t0, both > 0; budget is clamped to
// kDayProfTileMax.
DayProfPlan dayprof_plan(int G, int P, int N, int64_t agents, int steps, size_t budget);
// The row slot of step t in the LDS tile of the slice that begins at step slice_t0.
P2PMG_HD inline int dayprof_tile_slot(int fold, int P, int t, int slice_t0) { return fold ? t % P : t - slice_t0; }

}  // namespace p2pmg
