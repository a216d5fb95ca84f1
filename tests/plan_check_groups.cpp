// plan_check_groups.cpp — stand-alone check of how many chained episodes per wave the launch planner
// (csrc/p2pmg_plan.cpp) chooses: four (a quarter episode apart), two (half an episode apart) or the serial
// chain, by horizon T, hazard distance D, chain length and the P2PMG_INTERLEAVE override.  No HIP device is
// taken.  Built and run by tests/test_cpu_plan_groups.py; exits 0 and prints "ok <n>" when every case holds.
#include <cstdio>

#include "p2pmg.h"
#include "p2pmg_plan.h"

using namespace p2pmg;

static int failures = 0, checks = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    ++checks;                                               \
    if (!(cond)) {                                          \
      ++failures;                                           \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                       \
  } while (0)

// configs[1]'s shape at horizon T with hazard distance D, as the runtime derives the two facts from D
static PlanFacts facts(int T, int D, int S = 4096) {
  PlanFacts f;
  f.cfg.q_dtype = P2PMG_Q_F64;
  f.cfg.n_time_states = f.cfg.n_temp_states = f.cfg.n_balance_states = f.cfg.n_p2p_states = 20;
  f.cfg.temp_margin = 1.0f;
  f.cfg.minutes_per_hour = 60.0f;
  f.cfg.horizon = T;
  f.cfg.n_scenarios = S;
  f.cfg.n_agents = 2;
  f.cfg.rounds = 1;
  f.S = S, f.N = 2, f.R = 1, f.T = T, f.A = S * 2;
  f.n_cu = 256;
  f.n_env = 1;
  f.mi_ok = true;
  f.chain_lag_ok = D >= 0 && D + 4 <= T / 2;
  f.chain_lag_ok4 = D >= 0 && D + 4 <= T / 4;
  return f;
}

static EpisodePlan plan(const PlanFacts& f, int n_chain, double eps = 0.73, int flags = P2PMG_FLAG_RESET_T0,
                        Overrides ov = {}) {
  p2pmg_episode_args a{};
  a.mode = P2PMG_MODE_TRAIN;
  a.rng = P2PMG_RNG_PHILOX;
  a.epsilon = eps;
  a.flags = flags;
  return plan_episode(f, a, true, ov, n_chain);
}

static int groups(const PlanFacts& f, int n_chain, Overrides ov = {}) {
  const EpisodePlan p = plan(f, n_chain, 0.73, P2PMG_FLAG_RESET_T0, ov);
  CHECK(!p.error && p.family == Family::Fast);
  CHECK(p.interleave == (p.groups > 1));
  return p.groups;
}

int main() {
  // the hazard distance against a quarter and a half of the horizon
  CHECK(groups(facts(96, 20), 20) == 4);  // D + 4 = T/4
  CHECK(groups(facts(96, 21), 20) == 2);  // one past it: two groups (D + 4 <= T/2)
  CHECK(groups(facts(96, 5), 50) == 4);
  CHECK(groups(facts(96, 44), 20) == 2);  // D + 4 = T/2
  CHECK(groups(facts(96, 45), 20) == 1);
  CHECK(groups(facts(96, -1), 20) == 1);  // not computed
  // the horizon: T % 12 for four groups (each phase keeps the input ring's rotation), T % 6 for two
  CHECK(groups(facts(90, 5), 20) == 2);
  CHECK(groups(facts(84, 5), 20) == 4);
  CHECK(groups(facts(48, 8), 20) == 4 && groups(facts(48, 9), 20) == 2);
  CHECK(groups(facts(24, 2), 20) == 4 && groups(facts(24, 3), 20) == 2);
  CHECK(groups(facts(12, 0), 20) == 2);   // T/4 = 3 < D + 4 for every D
  CHECK(groups(facts(10, 0), 20) == 1);
  // the chain fills every group
  CHECK(groups(facts(96, 5), 4) == 4);
  CHECK(groups(facts(96, 5), 3) == 2);
  CHECK(groups(facts(96, 5), 2) == 2);
  CHECK(groups(facts(96, 5), 1) == 1);
  // the override: 0 = serial, 2 = at most two
  Overrides serial, two;
  serial.no_interleave = true;
  two.max_groups = 2;
  CHECK(groups(facts(96, 5), 20, serial) == 1);
  CHECK(groups(facts(96, 5), 20, two) == 2);
  CHECK(groups(facts(96, 45), 20, two) == 1);
  // what two groups ask for, four ask for as well: the reset flag, no battery, N = 2, at most 32 temperature bins
  CHECK(plan(facts(96, 5), 20, 0.73, 0).groups == 1 && !plan(facts(96, 5), 20, 0.73, 0).interleave);
  {
    PlanFacts b = facts(96, 5);
    b.battery = true;
    CHECK(groups(b, 20) == 1);
    PlanFacts t = facts(96, 5);
    t.cfg.n_temp_states = 33;
    CHECK(groups(t, 20) == 1);
    PlanFacts n4 = facts(96, 5);
    n4.N = n4.cfg.n_agents = 4, n4.A = n4.S * 4;
    CHECK(groups(n4, 20) == 1);
  }
  // scenarios per wave: a scenario's two lanes stay inside a group of 64 / groups lanes
  CHECK(plan(facts(96, 5), 20, 0.73).spw == 8 && plan(facts(96, 5), 20, 0.1).spw == 8);
  CHECK(plan(facts(96, 21), 20, 0.73).spw == 16 && plan(facts(96, 21), 20, 0.1).spw == 8);
  CHECK(plan(facts(96, 5, 8192), 20, 0.73).spw == 8 && plan(facts(96, 21, 8192), 20, 0.73).spw == 16);
  CHECK(plan(facts(96, 5, 20), 20, 0.73).spw == 8);
  {
    Overrides env;
    env.spw = 4;
    CHECK(plan(facts(96, 5), 20, 0.73, P2PMG_FLAG_RESET_T0, env).spw == 4);
    env.spw = 16;  // clamped to the group's width
    CHECK(plan(facts(96, 5), 20, 0.73, P2PMG_FLAG_RESET_T0, env).spw == 8);
  }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
