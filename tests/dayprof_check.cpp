// dayprof_check.cpp — stand-alone check of the host side of p2pmg_day_profile (csrc/p2pmg_dayprof.cpp and the
// inline maps of p2pmg_dayprof.h): argument validation, P and G, the 2^24 bound, the launch shape for a tile
// budget, fix and the ordered-u32 image of an f32.  No HIP device is taken.  Every label array handed to the
// code under test is a heap block of exactly S entries, so that under -fsanitize=address,undefined a read
// past it is a report.  Built and run by tests/test_cpu_day_profile_device.py.  Prints "sizeof ..." (the
// argument struct's layout), one "fix <f32 bits> <shift> <value>" line per probed value (the test compares
// them with tests/day_profile_ref.fix), then "ok <n>" and exits 0 when every case holds.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <set>
#include <utility>
#include <vector>

#include "p2pmg.h"
#include "p2pmg_dayprof.h"

using namespace p2pmg;

static int failures = 0, checks = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++checks;                                                        \
    if (!(cond)) {                                                   \
      ++failures;                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
    }                                                                \
  } while (0)

static bool says(const char* msg, const char* what) { return msg && std::strstr(msg, what); }

// resolve with an exact-size copy of the labels (empty: NULL)
static const char* resolve(int period, int t0, int tc, int s0, int sc, int n_groups, const std::vector<int32_t>& lab, int T, int S,
                           DayProfRange* r) {
  std::unique_ptr<int32_t[]> g(new int32_t[lab.size()]);
  if (!lab.empty()) std::memcpy(g.get(), lab.data(), lab.size() * sizeof(int32_t));
  p2pmg_day_profile_args a{period, t0, tc, s0, sc, n_groups, lab.empty() ? nullptr : g.get()};
  return dayprof_resolve(&a, T, S, r);
}

static float from_bits(uint32_t b) {
  float x;
  std::memcpy(&x, &b, 4);
  return x;
}
static uint32_t bits_of(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return b;
}

static void print_fix(float x, int k) { std::printf("fix %08x %d %lld\n", bits_of(x), k, dayprof_fix(x, k)); }

// the shape covers every (tile, step) pair and every (group, slot of a step) once, within the budget
static void check_plan(int G, int P, int N, int64_t agents, int steps, size_t budget) {
  const DayProfPlan p = dayprof_plan(G, P, N, agents, steps, budget);
  const size_t bound = budget < kDayProfTileMax ? budget : kDayProfTileMax;
  CHECK(p.tile_agents > 0 && p.tile_agents <= kDayProfBlock && p.tile_agents % N == 0 && p.tile_agents + N > kDayProfBlock);
  CHECK((int64_t)p.n_tiles * p.tile_agents >= agents && (int64_t)(p.n_tiles - 1) * p.tile_agents < agents);
  CHECK(p.tiles_per_run >= 1 && p.tiles_per_run <= kDayProfMaxRun);
  CHECK((int64_t)p.n_runs * p.tiles_per_run >= p.n_tiles && (int64_t)(p.n_runs - 1) * p.tiles_per_run < p.n_tiles);
  CHECK(p.slice_steps >= 1 && (int64_t)p.n_slices * p.slice_steps >= steps && (int64_t)(p.n_slices - 1) * p.slice_steps < steps);
  const size_t slot_bytes = (size_t)G * N * kDayProfRowBytes;
  CHECK(p.lds == (slot_bytes <= bound));
  if (!p.lds) {
    CHECK(p.tile_bytes == 0 && p.fold == 0);
    return;
  }
  CHECK(p.tile_bytes == slot_bytes * (size_t)p.tile_slots && p.tile_bytes <= bound && p.tile_slots >= 1);
  CHECK(p.fold == ((size_t)P * slot_bytes <= bound));
  CHECK(p.fold ? p.tile_slots == P : (p.tile_slots == p.slice_steps && p.tile_slots < P));
  // per slice: every step has a row slot inside the tile, and two steps share one only when they share t % P
  // (so each (group, slot) the slice touches has exactly one row of the tile: g * tile_slots + row slot)
  const int t0 = 3;  // the map must not depend on where the range begins
  std::set<std::pair<int, int>> seen;  // (slice, t)
  for (int j = 0; j < p.n_slices; ++j) {
    const int a = t0 + j * p.slice_steps, b = a + p.slice_steps < t0 + steps ? a + p.slice_steps : t0 + steps;
    std::vector<int> owner((size_t)p.tile_slots, -1);
    bool ok = a < b;
    for (int t = a; t < b; ++t) {
      const int ls = dayprof_tile_slot(p.fold, P, t, a);
      ok = ok && ls >= 0 && ls < p.tile_slots;
      if (!ok) break;
      ok = owner[(size_t)ls] < 0 || owner[(size_t)ls] == t % P;
      owner[(size_t)ls] = t % P;
      ok = ok && seen.insert({j, t}).second;
    }
    CHECK(ok);
    if (steps > 4096) break;  // one slice is enough for a long range
  }
  if (steps <= 4096) CHECK((int)seen.size() == steps);
}

int main() {
  std::printf("sizeof %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(p2pmg_day_profile_args), offsetof(p2pmg_day_profile_args, period),
              offsetof(p2pmg_day_profile_args, step_first), offsetof(p2pmg_day_profile_args, step_count),
              offsetof(p2pmg_day_profile_args, scen_first), offsetof(p2pmg_day_profile_args, scen_count),
              offsetof(p2pmg_day_profile_args, n_groups), offsetof(p2pmg_day_profile_args, groups));

  // ---- arguments: T = 96, S = 6
  const int T = 96, S = 6;
  DayProfRange r;
  CHECK(!resolve(0, 0, -1, 0, -1, 0, {}, T, S, &r) && r.P == T && r.G == 1 && r.t0 == 0 && r.t1 == T && r.s0 == 0 && r.s1 == S && !r.labelled);
  CHECK(!resolve(T, 0, -1, 0, -1, 0, {}, T, S, &r) && r.P == T);
  CHECK(!resolve(1, 0, -1, 0, -1, 0, {}, T, S, &r) && r.P == 1);
  CHECK(says(resolve(T + 1, 0, -1, 0, -1, 0, {}, T, S, &r), "period"));
  CHECK(says(resolve(-1, 0, -1, 0, -1, 0, {}, T, S, &r), "period"));
  // ranges: empty ones are valid, anywhere in [0, T] / [0, S]
  CHECK(!resolve(0, 5, 0, 0, -1, 0, {}, T, S, &r) && r.t0 == 5 && r.t1 == 5);
  CHECK(!resolve(0, T, 0, 0, -1, 0, {}, T, S, &r) && r.t0 == T && r.t1 == T);
  CHECK(!resolve(0, T, -1, 0, -1, 0, {}, T, S, &r) && r.t0 == T && r.t1 == T);
  CHECK(!resolve(0, 5, 82, 0, -1, 0, {}, T, S, &r) && r.t0 == 5 && r.t1 == 87);
  CHECK(!resolve(0, 0, -1, S, 0, 0, {}, T, S, &r) && r.s0 == S && r.s1 == S);
  CHECK(!resolve(0, 0, -1, 2, 3, 0, {}, T, S, &r) && r.s0 == 2 && r.s1 == 5);
  CHECK(says(resolve(0, -1, 1, 0, -1, 0, {}, T, S, &r), "step range"));
  CHECK(says(resolve(0, T + 1, 0, 0, -1, 0, {}, T, S, &r), "step range"));
  CHECK(says(resolve(0, 90, 7, 0, -1, 0, {}, T, S, &r), "step range"));
  CHECK(says(resolve(0, 1, std::numeric_limits<int32_t>::max(), 0, -1, 0, {}, T, S, &r), "step range"));
  CHECK(says(resolve(0, 0, -1, -1, 1, 0, {}, T, S, &r), "scenario range"));
  CHECK(says(resolve(0, 0, -1, 4, 3, 0, {}, T, S, &r), "scenario range"));
  CHECK(says(resolve(0, 0, -1, S + 1, -1, 0, {}, T, S, &r), "scenario range"));
  // labels
  CHECK(!resolve(0, 0, -1, 0, -1, 0, {0, 1, 2, 0, 1, 2}, T, S, &r) && r.G == 3 && r.labelled);
  CHECK(!resolve(0, 0, -1, 0, -1, 0, {-1, -1, -1, -1, -1, -1}, T, S, &r) && r.G == 1);
  CHECK(!resolve(0, 0, -1, 0, -1, 4, {0, -1, 3, 0, 1, 3}, T, S, &r) && r.G == 4);
  CHECK(!resolve(0, 0, -1, 0, -1, 5, {}, T, S, &r) && r.G == 5 && !r.labelled);
  CHECK(says(resolve(0, 0, -1, 0, -1, 3, {0, 1, 2, 3, 1, 2}, T, S, &r), "label"));   // label G
  CHECK(says(resolve(0, 0, -1, 0, -1, 0, {0, 1, -2, 0, 1, 2}, T, S, &r), "label"));  // label -2
  CHECK(says(resolve(0, 0, -1, 0, -1, 0, {0, 1, 2, 0, 1, std::numeric_limits<int32_t>::max()}, T, S, &r), "label"));
  CHECK(says(resolve(0, 0, -1, 0, -1, -1, {}, T, S, &r), "n_groups"));
  // a label outside the scenario range is checked all the same (as the host form does)
  CHECK(says(resolve(0, 0, -1, 0, 2, 2, {0, 1, 0, 1, 0, 2}, T, S, &r), "label"));
  CHECK(says(dayprof_resolve(nullptr, T, S, &r), "bad arguments"));

  // ---- the histogram and the 2^24 bound
  {
    CHECK(!resolve(0, 0, -1, 1, 4, 4, {0, -1, 3, 0, 1, 3}, T, S, &r));
    std::unique_ptr<int32_t[]> g(new int32_t[S]{0, -1, 3, 0, 1, 3});
    const std::vector<int64_t> h = dayprof_histogram(g.get(), r);  // scenarios 1..4
    CHECK(h.size() == 4 && h[0] == 1 && h[1] == 1 && h[2] == 0 && h[3] == 1);
    CHECK(!resolve(0, 0, -1, 1, 4, 0, {}, T, S, &r));
    const std::vector<int64_t> one = dayprof_histogram(nullptr, r);
    CHECK(one.size() == 1 && one[0] == 4);
    const int64_t M = kDayProfMaxSamples;
    const int64_t even[3] = {M, 5, 0}, over[3] = {7, M + 1, 0}, half[3] = {M / 2, M / 2 + 1, 1}, none[2] = {0, 0};
    CHECK(!dayprof_check_samples(even, 3, 96, 96));            // one step per slot: 2^24 samples exactly
    CHECK(says(dayprof_check_samples(over, 3, 96, 96), "2^24"));
    CHECK(says(dayprof_check_samples(over, 3, 96, 96), "split by scenario range and merge"));
    CHECK(says(dayprof_check_samples(even, 3, 97, 96), "2^24"));  // two steps share slot 0
    CHECK(!dayprof_check_samples(half, 1, 192, 96));           // 2^23 x 2
    CHECK(says(dayprof_check_samples(half, 2, 192, 96), "2^24"));
    CHECK(!dayprof_check_samples(half, 2, 96, 96));
    CHECK(!dayprof_check_samples(none, 2, 1 << 30, 1));         // nobody sampled
    CHECK(!dayprof_check_samples(over, 3, 0, 96));              // no step
    const int64_t year[1] = {512};
    CHECK(!dayprof_check_samples(year, 1, 35040, 96));         // 512 x 365
    const int64_t big[1] = {(int64_t)1 << 40};
    CHECK(says(dayprof_check_samples(big, 1, (int64_t)1 << 30, 1), "2^24"));  // no overflow of the product
  }

  // ---- launch shapes
  const size_t budgets[] = {200, 800, 1000, 2560, 4096, 12800, kDayProfTileDefault, kDayProfTileMax, (size_t)1 << 30};
  const int Ns[] = {1, 5, 16, 64};
  for (size_t budget : budgets)
    for (int N : Ns)
      for (int G : {1, 3, 70})
        for (int P : {1, 7, 60, 96})
          for (int steps : {1, 46, 60, 96})
            if (P <= 96)
              for (int64_t scen : {(int64_t)1, (int64_t)70, (int64_t)4099}) check_plan(G, P, N, scen * N, steps, budget);
  check_plan(1, 96, 4, 2048, 35040, kDayProfTileDefault);  // a year folded onto a day
  check_plan(1, 35040, 16, (int64_t)125000 * 16, 35040, kDayProfTileDefault);
  {
    const DayProfPlan p = dayprof_plan(1, 96, 16, (int64_t)16384 * 16, 96, kDayProfTileDefault);
    CHECK(p.lds && p.n_tiles == 1024 && p.tiles_per_run == kDayProfMaxRun && p.n_runs * p.n_slices >= kDayProfTargetBlocks / 2);
    const DayProfPlan q = dayprof_plan(70, 60, 16, 70 * 16, 60, kDayProfTileDefault);  // one slot of 70 groups: 179 KB
    CHECK(!q.lds);
    const DayProfPlan s = dayprof_plan(1, 60, 16, 70 * 16, 60, 2560);  // one slot fits: one step per slice
    CHECK(s.lds && !s.fold && s.slice_steps == 1 && s.n_slices == 60 && s.tiles_per_run == 5);
  }

  // ---- fix: ties to even at each shift, negatives, the largest magnitudes
  CHECK(dayprof_fix(0x1p-29f, 28) == 0 && dayprof_fix(3 * 0x1p-29f, 28) == 2 && dayprof_fix(5 * 0x1p-29f, 28) == 2);
  CHECK(dayprof_fix(-0x1p-29f, 28) == 0 && dayprof_fix(-3 * 0x1p-29f, 28) == -2);
  CHECK(dayprof_fix(0x1p-25f, 24) == 0 && dayprof_fix(3 * 0x1p-25f, 24) == 2 && dayprof_fix(-3 * 0x1p-25f, 24) == -2);
  CHECK(dayprof_fix(0x1p-17f, 16) == 0 && dayprof_fix(3 * 0x1p-17f, 16) == 2 && dayprof_fix(7 * 0x1p-17f, 16) == 4);
  CHECK(dayprof_fix(0.0f, 28) == 0 && dayprof_fix(-0.0f, 16) == 0 && dayprof_fix(1.0f, 28) == (1ll << 28));
  CHECK(dayprof_fix(0x1p23f, 16) == (1ll << 39) && dayprof_fix(-0x1p23f, 16) == -(1ll << 39));
  CHECK(dayprof_fix(0x1p15f, 24) == (1ll << 39) && dayprof_fix(0x1p11f, 28) == (1ll << 39));
  CHECK(dayprof_fix(std::nextafterf(0x1p23f, 0.0f), 16) == (1ll << 39) - (1ll << 15));
  CHECK(dayprof_fix(1.5f * 0x1p-28f, 28) == 2 && dayprof_fix(2.5f * 0x1p-28f, 28) == 2 && dayprof_fix(0.75f * 0x1p-28f, 28) == 1);
  {
    uint32_t z = 12345u;
    for (int n = 0; n < 4000; ++n) {  // a fixed pseudo-random sweep of bit patterns, magnitudes inside the bound of each shift
      z = z * 1664525u + 1013904223u;
      const int k = n % 3 == 0 ? 16 : (n % 3 == 1 ? 24 : 28);
      const int top = k == 16 ? 23 : (k == 24 ? 15 : 11);
      const uint32_t expo = 127u + (uint32_t)top - 1u - (z >> 8) % 64u;  // 2^(top - 64) <= |x| < 2^top
      print_fix(from_bits((z & 0x807FFFFFu) | (expo << 23)), k);
    }
    for (int k : {16, 24, 28})
      for (int m = -9; m <= 9; ++m) print_fix((float)m * std::ldexp(1.0f, -k - 1), k);  // every tie around zero
  }

  // ---- the ordered image: strictly monotone and round-tripping
  {
    std::vector<float> v = {-std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::max(), -1.0f,
                            -std::numeric_limits<float>::min(), -from_bits(0x007FFFFFu), -from_bits(1u), 0.0f, from_bits(1u),
                            from_bits(0x007FFFFFu), std::numeric_limits<float>::min(), 1.0f, std::numeric_limits<float>::max(),
                            std::numeric_limits<float>::infinity()};
    for (size_t k = 0; k < v.size(); ++k) {
      CHECK(bits_of(dayprof_unord(dayprof_ord(v[k]))) == bits_of(v[k]));
      if (k) CHECK(dayprof_ord(v[k - 1]) < dayprof_ord(v[k]));
    }
    CHECK(dayprof_ord(std::numeric_limits<float>::infinity()) == kDayProfOrdPosInf);
    CHECK(dayprof_ord(-std::numeric_limits<float>::infinity()) == kDayProfOrdNegInf);
    // the +0 rule: the kernels add +0.0f first, so -0.0 arrives as +0.0; the raw images keep -0.0 below +0.0
    const float nz = -0.0f;
    CHECK(bits_of(nz + 0.0f) == 0u && dayprof_ord(nz + 0.0f) == dayprof_ord(0.0f) && dayprof_ord(nz) < dayprof_ord(0.0f));
    CHECK(bits_of(dayprof_unord(dayprof_ord(nz))) == 0x80000000u);
    bool mono = true, trip = true;
    float prev = -std::numeric_limits<float>::infinity();
    for (uint32_t b = 0xFF7FFFFFu; b > 0x80000000u; b -= 0x0001F3C7u) {  // the negatives, ascending
      const float x = from_bits(b);
      mono = mono && dayprof_ord(prev) < dayprof_ord(x);
      trip = trip && bits_of(dayprof_unord(dayprof_ord(x))) == b;
      prev = x;
    }
    for (uint32_t b = 0u; b < 0x7F800000u; b += 0x0001F3C7u) {  // +0, the denormals, the positives
      const float x = from_bits(b);
      mono = mono && dayprof_ord(prev) < dayprof_ord(x);
      trip = trip && bits_of(dayprof_unord(dayprof_ord(x))) == b;
      prev = x;
    }
    CHECK(mono);
    CHECK(trip);
  }

  if (failures) {
    std::printf("%d of %d checks failed\n", failures, checks);
    return 1;
  }
  std::printf("ok %d\n", checks);
  return 0;
}
