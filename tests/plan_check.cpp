// plan_check.cpp — stand-alone check of the launch planner (csrc/p2pmg_plan.cpp): which kernel family,
// Philox source, scenarios per wave and record layout a configuration gets.  No HIP device is taken.
// The expected values are read off the conditions the runtime has always applied, not off the planner.
// Built and run by tests/test_cpu_plan.py; exits 0 and prints "ok <n>" when every case holds.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "p2pmg.h"
#include "p2pmg_plan.h"

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

// 256 compute units, default config, mi_ok, margin 1, no overrides
static PlanFacts facts(int S, int N, int R, int shared_q = 0) {
  PlanFacts f;
  // what p2pmg_config_default sets, of the fields the choice reads
  f.cfg.q_dtype = P2PMG_Q_F64;
  f.cfg.n_time_states = f.cfg.n_temp_states = f.cfg.n_balance_states = f.cfg.n_p2p_states = 20;
  f.cfg.temp_margin = 1.0f;
  f.cfg.minutes_per_hour = 60.0f;
  f.cfg.horizon = 96;
  f.cfg.n_scenarios = S;
  f.cfg.n_agents = N;
  f.cfg.rounds = R;
  f.cfg.shared_q = shared_q;
  f.S = S, f.N = N, f.R = R, f.T = f.cfg.horizon, f.A = S * N;
  f.n_cu = 256;
  f.n_env = 1;
  f.mi_ok = true;
  f.roles = shared_q == P2PMG_SHARED_ROLE;
  return f;
}

static p2pmg_episode_args greedy(int record = 0, int flags = 0) {
  p2pmg_episode_args a{};
  a.mode = P2PMG_MODE_GREEDY;
  a.record = record;
  a.flags = flags;
  return a;
}

static p2pmg_episode_args train(int rng, double eps = 0.81, int flags = 0) {
  p2pmg_episode_args a{};
  a.mode = P2PMG_MODE_TRAIN;
  a.rng = rng;
  a.epsilon = eps;
  a.flags = flags;
  return a;
}

static EpisodePlan plan(const PlanFacts& f, const p2pmg_episode_args& a, bool chained = false, Overrides ov = {}) {
  return plan_episode(f, a, chained, ov);
}

int main() {
  {  // the fast kernel and what turns it off
    const PlanFacts f = facts(4096, 2, 1);
    EpisodePlan p = plan(f, greedy());
    CHECK(p.family == Family::Fast && p.want_ipc && p.packed_records && p.speculate && !p.error);
    CHECK(plan(f, greedy(0, P2PMG_FLAG_GENERAL_KERNEL)).family == Family::General);
    CHECK(plan(f, greedy(0, P2PMG_FLAG_PHILOX_INKERNEL)).family == Family::General);
    Overrides gen;
    gen.general = true;
    CHECK(plan(f, greedy(), false, gen).family == Family::General);
    CHECK(!plan(f, greedy(), false, gen).packed_records && !plan(f, greedy(), false, gen).want_ipc);
    CHECK(plan(f, greedy(0, P2PMG_FLAG_TILE_KERNEL)).family == Family::Tile);
    Overrides nospec;
    nospec.no_spec = true;
    CHECK(plan(f, greedy(), false, nospec).family == Family::Fast && !plan(f, greedy(), false, nospec).speculate);
    CHECK(plan(facts(64, 8, 3), greedy()).family == Family::Fast);
    CHECK(!plan(facts(64, 8, 3), greedy()).want_ipc);
    CHECK(plan(facts(64, 8, 4), greedy()).family == Family::General);
    CHECK(plan(facts(64, 9, 1), greedy()).family == Family::Tile);
    CHECK(plan(facts(64, 16, 1), greedy()).family == Family::General);
    PlanFacts b = facts(64, 2, 1);
    b.battery = true;
    CHECK(plan(b, greedy()).family == Family::Fast && !plan(b, greedy()).want_ipc);
    b.R = b.cfg.rounds = 2;
    CHECK(plan(b, greedy()).family == Family::General);
    PlanFacts m = facts(64, 2, 1);
    m.cfg.temp_margin = 2.0f;
    CHECK(plan(m, greedy()).family != Family::Fast);
    m = facts(64, 2, 1);
    m.mi_ok = false;
    CHECK(plan(m, greedy()).family != Family::Fast);
    m = facts(64, 2, 1);
    m.cfg.n_time_states = 64, m.cfg.n_temp_states = 32, m.cfg.n_balance_states = 32;  // product 65536
    CHECK(plan(m, greedy()).family != Family::Fast);
    m.cfg.n_balance_states = 31;  // just below it
    CHECK(plan(m, greedy()).family == Family::Fast);
  }
  {  // the 16-agent shared-table kernel: 20^4 states (the default), thermal never set
    const PlanFacts f = facts(64, 16, 1, 1);
    CHECK(plan(f, greedy()).family == Family::Sq16 && plan(f, greedy()).packed_records && !plan(f, greedy()).speculate);
    PlanFacts g = f;
    g.thermal_set = true;
    CHECK(plan(g, greedy()).family == Family::General);
    CHECK(plan(facts(64, 16, 2, 1), greedy()).family == Family::General);
    CHECK(plan(facts(64, 16, 1, P2PMG_SHARED_ROLE), greedy()).family == Family::General);
    g = f;
    g.cfg.n_p2p_states = 10;
    CHECK(plan(g, greedy()).family == Family::General);
    CHECK(plan(f, train(P2PMG_RNG_PHILOX)).philox == Philox::InKernel);
    CHECK(plan(f, train(P2PMG_RNG_REPLAY)).philox == Philox::None);
    // an explicit pre-pass request keeps the kernel and moves its draws to the code-word pre-pass
    const EpisodePlan pp = plan(f, train(P2PMG_RNG_PHILOX, 0.81, P2PMG_FLAG_PHILOX_PREPASS));
    CHECK(pp.family == Family::Sq16 && pp.philox == Philox::CodesPrepass && pp.packed_records);
    CHECK(plan(f, train(P2PMG_RNG_PHILOX, 0.81, P2PMG_FLAG_PHILOX_INKERNEL)).philox == Philox::InKernel);
  }
  {  // where a general launch draws its Philox codes: the pre-pass below 2^18 agents
    const int gen = P2PMG_FLAG_GENERAL_KERNEL;
    const PlanFacts small = facts((1 << 17) - 1, 2, 1), big = facts(1 << 17, 2, 1);
    CHECK(small.A == (1 << 18) - 2 && big.A == (1 << 18));
    CHECK(plan(small, train(P2PMG_RNG_PHILOX, 0.81, gen)).family == Family::General);
    CHECK(plan(small, train(P2PMG_RNG_PHILOX, 0.81, gen)).philox == Philox::CodesPrepass);
    CHECK(plan(big, train(P2PMG_RNG_PHILOX, 0.81, gen)).philox == Philox::InKernel);
    for (const PlanFacts* f : {&small, &big}) {
      CHECK(plan(*f, train(P2PMG_RNG_PHILOX, 0.81, gen | P2PMG_FLAG_PHILOX_PREPASS)).philox == Philox::CodesPrepass);
      CHECK(plan(*f, train(P2PMG_RNG_PHILOX, 0.81, gen | P2PMG_FLAG_PHILOX_INKERNEL)).philox == Philox::InKernel);
      CHECK(plan(*f, train(P2PMG_RNG_REPLAY, 0.81, gen)).philox == Philox::None);
      CHECK(plan(*f, greedy(0, gen)).philox == Philox::None);
      CHECK(plan(*f, train(P2PMG_RNG_PHILOX)).philox == Philox::FastPrepass);  // the fast kernel's own
      CHECK(plan(*f, train(P2PMG_RNG_REPLAY)).philox == Philox::None);
    }
  }
  {  // scenarios per wave
    CHECK(plan(facts(4096, 2, 1), train(P2PMG_RNG_PHILOX, 0.6)).spw == 16);
    CHECK(plan(facts(4096, 2, 1), train(P2PMG_RNG_PHILOX, 0.39)).spw == 8);
    CHECK(plan(facts(8192, 2, 1), train(P2PMG_RNG_PHILOX, 0.6)).spw == 32);
    CHECK(plan(facts(8192, 2, 1), train(P2PMG_RNG_PHILOX, 0.39)).spw == 32);
    CHECK(plan(facts(4096, 2, 1), greedy()).spw == 16);
    p2pmg_episode_args a = greedy();
    a.scen_per_wave = 5;
    CHECK(plan(facts(4096, 2, 1), a).spw == 5);
    a.scen_per_wave = 100;  // an explicit value is not clamped
    CHECK(plan(facts(4096, 2, 1), a).spw == 100);
    Overrides env;
    env.spw = 7;
    CHECK(plan(facts(4096, 2, 1), greedy(), false, env).spw == 7 && plan(facts(4096, 2, 1), a, false, env).spw == 100);
  }
  {  // the narrow {reward, cost} record rows
    const PlanFacts f = facts(64, 2, 1);
    CHECK(plan(f, greedy(0)).rec_narrow == 1);
    CHECK(plan(f, greedy(P2PMG_REC_REWARD | P2PMG_REC_COST)).rec_narrow == 1);
    CHECK(plan(f, greedy(P2PMG_REC_COST | P2PMG_REC_GRID)).rec_narrow == 0);
    CHECK(plan(facts(64, 16, 1, 1), greedy(P2PMG_REC_COST)).rec_narrow == 1);
    for (int mask : {0, P2PMG_REC_REWARD | P2PMG_REC_COST, P2PMG_REC_COST | P2PMG_REC_GRID, 127})
      CHECK(plan(f, greedy(mask, P2PMG_FLAG_GENERAL_KERNEL)).rec_narrow == 0);
  }
  {  // chained launches: the fast kernel and Philox training only
    const PlanFacts f = facts(4096, 2, 1);
    const char* msg = "run_episode: a chained launch needs the fast kernel and Philox training";
    CHECK(!plan(f, train(P2PMG_RNG_PHILOX), true).error && plan(f, train(P2PMG_RNG_PHILOX), true).family == Family::Fast);
    CHECK(plan(f, greedy(), true).error && !std::strcmp(plan(f, greedy(), true).error, msg));
    CHECK(plan(f, train(P2PMG_RNG_REPLAY), true).error != nullptr);
    const EpisodePlan g = plan(f, train(P2PMG_RNG_PHILOX, 0.81, P2PMG_FLAG_GENERAL_KERNEL), true);
    CHECK(g.error && !std::strcmp(g.error, msg));
  }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
