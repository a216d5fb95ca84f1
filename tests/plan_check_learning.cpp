// plan_check_learning.cpp — stand-alone check of the launch planner's two learner facts
// (csrc/p2pmg_plan.cpp): learning_set (p2pmg_set_learning uploaded values) and eps_table (the launch
// belongs to a p2pmg_run_episodes_eps call).  Both take episode_sq16_kernel out of the choice and
// leave every other choice where it was; eps_table also turns the speculative pre-pass off.
// No HIP device is taken.  Built and run by tests/test_cpu_learning.py; prints "ok <n>".
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

static PlanFacts facts(int S, int N, int R, int T, int shared_q = 0) {
  PlanFacts f;
  f.cfg.q_dtype = P2PMG_Q_F64;
  f.cfg.n_time_states = f.cfg.n_temp_states = f.cfg.n_balance_states = f.cfg.n_p2p_states = 20;
  f.cfg.temp_margin = 1.0f;
  f.cfg.minutes_per_hour = 60.0f;
  f.cfg.horizon = T;
  f.cfg.n_scenarios = S;
  f.cfg.n_agents = N;
  f.cfg.rounds = R;
  f.cfg.shared_q = shared_q;
  f.S = S, f.N = N, f.R = R, f.T = T, f.A = S * N;
  f.n_cu = 256;
  f.n_env = 1;
  f.mi_ok = true;
  return f;
}

static p2pmg_episode_args train(int flags = 0, double eps = 0.81) {
  p2pmg_episode_args a{};
  a.mode = P2PMG_MODE_TRAIN;
  a.rng = P2PMG_RNG_PHILOX;
  a.epsilon = eps;
  a.flags = flags;
  return a;
}

int main() {
  const Overrides ov{};
  {  // defaults: a context that never calls the setter plans as before
    const PlanFacts f = facts(64, 16, 1, 96, 1);
    CHECK(!f.learning_set && !f.eps_table);
    CHECK(plan_episode(f, train(), false, ov).family == Family::Sq16);
  }
  {  // sq16 is refused once either fact is set, and comes back with it
    PlanFacts f = facts(64, 16, 1, 96, 1);
    f.learning_set = true;
    EpisodePlan p = plan_episode(f, train(), false, ov);
    CHECK(p.family == Family::General && !p.packed_records && p.philox == Philox::CodesPrepass);
    p2pmg_episode_args g{};
    g.mode = P2PMG_MODE_GREEDY;
    CHECK(plan_episode(f, g, false, ov).family == Family::General);
    f.learning_set = false;
    CHECK(plan_episode(f, train(), false, ov).family == Family::Sq16);
    f.eps_table = true;
    CHECK(plan_episode(f, train(), false, ov).family == Family::General);
  }
  for (int learning = 0; learning < 2; ++learning)
    for (int table = 0; table < 2; ++table) {  // the fast family and the interleave stay where they were
      PlanFacts f = facts(4096, 2, 1, 96);
      f.learning_set = learning != 0;
      f.eps_table = table != 0;
      EpisodePlan p = plan_episode(f, train(), false, ov);
      CHECK(p.family == Family::Fast && p.philox == Philox::FastPrepass && p.want_ipc && p.packed_records);
      CHECK(p.speculate == !table);  // a table call does not speculate the next launch's pre-pass
      CHECK(p.spw == 16 && !p.interleave);
      CHECK(plan_episode(f, train(P2PMG_FLAG_GENERAL_KERNEL), false, ov).family == Family::General);
      CHECK(plan_episode(facts(64, 9, 1, 96), train(), false, ov).family == Family::Tile);
      EpisodePlan c = plan_episode(f, train(P2PMG_FLAG_RESET_T0), true, ov, 6);
      CHECK(!c.error && c.family == Family::Fast && !c.interleave);  // hazard distance unknown: serial
      f.chain_lag_ok = true;
      c = plan_episode(f, train(P2PMG_FLAG_RESET_T0), true, ov, 6);
      CHECK(!c.error && c.interleave && c.spw <= 16);
      CHECK(!plan_episode(f, train(), true, ov, 6).interleave);                        // no T0 reset
      CHECK(!plan_episode(f, train(P2PMG_FLAG_RESET_T0), true, ov, 1).interleave);    // one episode
      PlanFacts odd = f;
      odd.T = odd.cfg.horizon = 10;
      CHECK(!plan_episode(odd, train(P2PMG_FLAG_RESET_T0), true, ov, 6).interleave);  // T % 6 != 0
    }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
