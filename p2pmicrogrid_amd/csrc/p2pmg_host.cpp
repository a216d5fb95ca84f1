// p2pmg_host.cpp — the entry points that touch neither HIP nor a context, and the config check
// p2pmg_create makes before its first device call.  No HIP include: tests/host_check.cpp links this file
// alone into a program that runs under sanitizers.
#include "p2pmg_host.h"

#include <cmath>
#include <cstdint>
#include <cstring>

namespace p2pmg {

int validate_config(const p2pmg_config* cfg, std::string* why) {
  if (why) why->clear();
  if (!cfg) return P2PMG_E_INVALID;
  if (cfg->n_scenarios <= 0 || cfg->n_agents <= 0 || cfg->rounds < 0 || cfg->horizon <= 0) return P2PMG_E_INVALID;
  if (cfg->rounds + 1 > kMaxRounds1) return P2PMG_E_UNSUPPORTED;
  // 2 actions: a context that holds tables (set_q, get_q, the table digests) but runs no episode
  if (cfg->n_actions != 3 && !(cfg->n_actions == 2 && cfg->learner == P2PMG_LEARNER_TABULAR)) return P2PMG_E_UNSUPPORTED;
  // any community size a scenario's wave holds (get_community takes any n_agents, community.py:198-204)
  if (cfg->n_agents > kMaxAgents) return P2PMG_E_UNSUPPORTED;
  if (cfg->q_dtype != P2PMG_Q_F64 && cfg->q_dtype != P2PMG_Q_F32) return P2PMG_E_INVALID;
  if (cfg->shared_q == P2PMG_SHARED_ROLE && cfg->learner == P2PMG_LEARNER_DQN) {
    if (why) *why = "create: shared_q = P2PMG_SHARED_ROLE needs learner = TABULAR (a Q-network per role is not built)";
    return P2PMG_E_UNSUPPORTED;
  }
  return P2PMG_OK;
}

int validate_dqn_learning(const DqnLearn* rows, int n_nets, const float* penw, int n_agents, std::string* why) {
  if (why) why->clear();
  auto bad = [&](const char* what, const char* unit, int k) {
    if (why) *why = std::string("dqn_set_learning: ") + what + " for " + unit + " " + std::to_string(k);
    return P2PMG_E_INVALID;
  };
  for (int k = 0; k < n_nets; ++k) {
    const DqnLearn& r = rows[k];
    if (!(std::isfinite(r.gamma) && r.gamma >= 0.0 && r.gamma <= 1.0)) return bad("gamma outside [0, 1]", "network", k);
    if (!(std::isfinite(r.tau) && r.tau >= 0.0 && r.tau <= 1.0)) return bad("tau outside [0, 1]", "network", k);
    if (!(std::isfinite(r.lr) && r.lr >= 0.0)) return bad("negative or non-finite lr", "network", k);
    if (!(std::isfinite(r.clip) && r.clip > 0.0)) return bad("clip not positive and finite", "network", k);
  }
  for (int a = 0; a < n_agents; ++a)
    if (!(std::isfinite(penw[a]) && penw[a] >= 0.0f)) return bad("negative or non-finite penalty weight", "agent", a);
  return P2PMG_OK;
}

int validate_dqn_roles_world(const char* call, int nranks, bool communicator, std::string* why) {
  if (why) why->clear();
  if (!communicator && nranks <= 1) return P2PMG_OK;
  if (why)
    *why = std::string(call) + ": a role context (p2pmg_dqn_setup_roles) trains on one rank (per-role networks over "
                               "several ranks are not built)";
  return P2PMG_E_UNSUPPORTED;
}

int validate_dqn_roles(const p2pmg_config* cfg, const p2pmg_dqn_config* dq, bool set_up, int nranks, bool has_comm,
                       std::string* why) {
  if (why) why->clear();
  auto bad = [&](int code, const char* what) {
    if (why) *why = std::string("dqn_setup_roles: ") + what;
    return code;
  };
  if (!cfg || !dq) return P2PMG_E_INVALID;
  if (cfg->learner != P2PMG_LEARNER_DQN) return bad(P2PMG_E_STATE, "create the context with learner = P2PMG_LEARNER_DQN");
  if (set_up) return bad(P2PMG_E_STATE, "already set up");
  if (cfg->shared_q == 0)
    return bad(P2PMG_E_INVALID, "create the context with shared_q = 1 (shared_q = 0 holds a network per agent: p2pmg_dqn_setup)");
  if (dq->batch != 32) return bad(P2PMG_E_UNSUPPORTED, "batch must be 32");
  if (dq->capacity < 32 || dq->capacity > 65535) return bad(P2PMG_E_INVALID, "capacity must be in [32, 65535]");
  if (dq->agents_per_block < 0 || dq->grad_segments < 0) return bad(P2PMG_E_INVALID, "negative layout");
  if (dq->grad_segments > 1)
    return bad(P2PMG_E_INVALID, "grad_segments must be 0 or 1 (a role's gradient is one segment; segments are the "
                                "several-rank layout, which per-role networks do not have)");
  return validate_dqn_roles_world("dqn_setup_roles", nranks, has_comm, why);
}

int validate_policy_set(int count, const uint8_t* policies, const int32_t* policy_of, size_t n_states, int n_actions,
                        int n_agents, int n_scenarios, int32_t* map_out, std::string* why) {
  if (why) why->clear();
  auto bad = [&](const std::string& what) {
    if (why) *why = "set_policy_set: " + what;
    return P2PMG_E_INVALID;
  };
  if (count < 1) return bad("count must be positive");
  if (n_agents < 1 || n_scenarios < 1 || n_actions < 1 || n_actions >= P2PMG_POLICY_UNVISITED)
    return bad("bad context shape");
  const long long A = (long long)n_agents * n_scenarios;
  if (policy_of) {
    for (long long a = 0; a < A; ++a) {
      if (policy_of[a] < 0 || policy_of[a] >= count)
        return bad("policy_of[" + std::to_string(a) + "] = " + std::to_string(policy_of[a]) + " outside [0, " +
                   std::to_string(count) + ")");
      if (map_out) map_out[a] = policy_of[a];
    }
  } else if (count == A) {
    for (long long a = 0; map_out && a < A; ++a) map_out[a] = (int32_t)a;
  } else if (count == n_agents) {
    for (long long a = 0; map_out && a < A; ++a) map_out[a] = (int32_t)(a % n_agents);  // role i of every scenario
  } else if (count == 1) {
    for (long long a = 0; map_out && a < A; ++a) map_out[a] = 0;
  } else {
    return bad("without policy_of, count must be A, N or 1");
  }
  if (policies) {
    const size_t total = (size_t)count * n_states;
    for (size_t k = 0; k < total; ++k) {
      const uint8_t b = policies[k];
      if (b >= n_actions && b != P2PMG_POLICY_UNVISITED)
        return bad("byte " + std::to_string((int)b) + " at policy " + std::to_string(k / n_states) + ", state " +
                   std::to_string(k % n_states) + " is neither an action nor P2PMG_POLICY_UNVISITED");
    }
  }
  return P2PMG_OK;
}

}  // namespace p2pmg

extern "C" {

int p2pmg_abi_version(void) { return P2PMG_ABI_VERSION; }

int p2pmg_config_default(p2pmg_config* cfg) {
  if (!cfg) return P2PMG_E_INVALID;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->n_scenarios = 1;
  cfg->n_agents = 2;   // setup.py:33
  cfg->rounds = 1;     // setup.py:34
  cfg->horizon = 96;   // one day of 15-minute slots
  cfg->q_dtype = P2PMG_Q_F64;
  cfg->n_time_states = cfg->n_temp_states = cfg->n_balance_states = cfg->n_p2p_states = 20;
  cfg->n_actions = 3;
  cfg->alpha = 1e-5;
  cfg->gamma = 0.9;
  const double levels[3] = {0.0, 0.5, 1.0};
  for (int k = 0; k < 3; ++k) cfg->hp_levels[k] = (float)(levels[k] * 3e3);
  cfg->setpoint = 21.0f;
  cfg->temp_margin = 1.0f;
  cfg->lower_bound = 20.0f;
  cfg->upper_bound = 22.0f;
  const double Ci = 2.44e6 * 2, Cm = 9.4e7, Ri = 8.64e-4, Re = 1.05e-2, Rvent = 7.98e-3, gA = 11.468, f_rad = 0.3;
  cfg->inv_ci = (float)(1 / Ci);
  cfg->inv_cm = (float)(1 / Cm);
  cfg->inv_ri = (float)(1 / Ri);
  cfg->inv_re = (float)(1 / Re);
  cfg->inv_rvent = (float)(1 / Rvent);
  cfg->one_minus_frad = (float)(1 - f_rad);
  cfg->frad = (float)f_rad;
  cfg->solar_gain = (float)(gA * 0.0);
  cfg->hp_cop = 3.0f;
  cfg->seconds_per_minute = 60.0f;
  cfg->time_slot = 15.0f;
  cfg->minutes_per_hour = 60.0f;
  cfg->kilo = (float)1e-3;
  cfg->penalty_weight = 10.0f;
  cfg->seed = 42;
  cfg->scenario_offset = 0;
  return P2PMG_OK;
}

int p2pmg_dqn_config_default(p2pmg_dqn_config* cfg) {
  if (!cfg) return P2PMG_E_INVALID;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->gamma = 0.95;  // agent.py:309
  cfg->tau = 0.005;
  cfg->lr = 1e-5;     // agent.py:310
  cfg->beta1 = 0.9;
  cfg->beta2 = 0.999;
  cfg->adam_eps = 1e-7;
  cfg->clip = 1.0;    // rl.py:329
  cfg->batch = 32;    // agent.py:308
  cfg->capacity = 5000;
  cfg->agents_per_block = 0;
  return P2PMG_OK;
}

int p2pmg_replay_decode(const uint32_t* words, size_t n_words, size_t n_decisions, const double* eps, size_t n_eps,
                        uint8_t* codes, size_t* consumed) {
  if (!words || !eps || n_eps == 0 || !codes) return P2PMG_E_INVALID;
  size_t pos = 0;
  for (size_t k = 0; k < n_decisions; ++k) {
    // RandomState.rand(): (a * 2^26 + b) / 2^53 with a = w0 >> 5, b = w1 >> 6 (mt19937 next_double)
    if (pos + 2 > n_words) return P2PMG_E_INVALID;
    const uint32_t a = words[pos] >> 5, b = words[pos + 1] >> 6;
    pos += 2;
    const double u = ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    if (u < eps[k % n_eps]) {
      // RandomState.choice(3) -> randint(0, 3): masked rejection, mask 3, one word per try
      uint32_t v;
      do {
        if (pos >= n_words) return P2PMG_E_INVALID;
        v = words[pos++] & 3u;
      } while (v > 2u);
      codes[k] = (uint8_t)v;
    } else {
      codes[k] = P2PMG_GREEDY;
    }
  }
  if (consumed) *consumed = pos;
  return P2PMG_OK;
}

}  // extern "C"
