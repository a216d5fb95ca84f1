// dqn_roles_check.cpp — the argument checks of p2pmg_dqn_setup_roles and of a role context's world
// (csrc/p2pmg_host.cpp::validate_dqn_roles, validate_dqn_roles_world) as a program of its own: no HIP call, no
// context.  tests/test_cpu_dqn_roles.py builds it with -fsanitize=address,undefined and runs it; it prints
// "ok <checks>" and exits 0, or names the failed check.  It also pins what p2pmg_create keeps refusing.
#include <cstdio>
#include <string>

#include "p2pmg.h"
#include "p2pmg_host.h"

static int n_checks = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++n_checks;                                                  \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                  \
    }                                                            \
  } while (0)

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

int main() {
  p2pmg_config cfg;
  p2pmg_dqn_config dq;
  CHECK(p2pmg_config_default(&cfg) == P2PMG_OK && p2pmg_dqn_config_default(&dq) == P2PMG_OK);
  cfg.learner = P2PMG_LEARNER_DQN;
  cfg.shared_q = 1;
  std::string why = "stale";
  // the route: a DQN context created with shared_q = 1, not set up, one rank; grad_segments 0 or 1
  CHECK(p2pmg::validate_config(&cfg, &why) == P2PMG_OK);
  CHECK(p2pmg::validate_dqn_roles(&cfg, &dq, false, 1, false, &why) == P2PMG_OK && why.empty());
  dq.grad_segments = 1;
  CHECK(p2pmg::validate_dqn_roles(&cfg, &dq, false, 1, false, &why) == P2PMG_OK && why.empty());
  CHECK(p2pmg::validate_dqn_roles(&cfg, &dq, false, 1, false, nullptr) == P2PMG_OK);
  dq.agents_per_block = 16;
  dq.capacity = 32;
  CHECK(p2pmg::validate_dqn_roles(&cfg, &dq, false, 1, false, &why) == P2PMG_OK);
  dq.capacity = 65535;
  CHECK(p2pmg::validate_dqn_roles(&cfg, &dq, false, 1, false, &why) == P2PMG_OK);
  CHECK(p2pmg::validate_dqn_roles(nullptr, &dq, false, 1, false, &why) == P2PMG_E_INVALID);
  CHECK(p2pmg::validate_dqn_roles(&cfg, nullptr, false, 1, false, &why) == P2PMG_E_INVALID);
  // gradient segments are the several-rank layout: refused with a reason, whatever else is right
  for (int g : {2, 3, 64}) {
    p2pmg_dqn_config d2 = dq;
    d2.grad_segments = g;
    CHECK(p2pmg::validate_dqn_roles(&cfg, &d2, false, 1, false, &why) == P2PMG_E_INVALID);
    CHECK(has(why, "dqn_setup_roles") && has(why, "grad_segments"));
    CHECK(p2pmg::validate_dqn_roles(&cfg, &d2, false, 1, false, nullptr) == P2PMG_E_INVALID);
  }
  {
    p2pmg_dqn_config d2 = dq;
    d2.grad_segments = -1;
    CHECK(p2pmg::validate_dqn_roles(&cfg, &d2, false, 1, false, &why) == P2PMG_E_INVALID && has(why, "negative"));
    d2 = dq;
    d2.agents_per_block = -2;
    CHECK(p2pmg::validate_dqn_roles(&cfg, &d2, false, 1, false, &why) == P2PMG_E_INVALID && has(why, "negative"));
    d2 = dq;
    d2.capacity = 31;
    CHECK(p2pmg::validate_dqn_roles(&cfg, &d2, false, 1, false, &why) == P2PMG_E_INVALID && has(why, "capacity"));
    d2.capacity = 65536;
    CHECK(p2pmg::validate_dqn_roles(&cfg, &d2, false, 1, false, &why) == P2PMG_E_INVALID && has(why, "capacity"));
    d2 = dq;
    d2.batch = 64;
    CHECK(p2pmg::validate_dqn_roles(&cfg, &d2, false, 1, false, &why) == P2PMG_E_UNSUPPORTED && has(why, "batch"));
  }
  {  // the context's own state: tabular, already set up, a network per agent
    p2pmg_config c2 = cfg;
    c2.learner = P2PMG_LEARNER_TABULAR;
    CHECK(p2pmg::validate_dqn_roles(&c2, &dq, false, 1, false, &why) == P2PMG_E_STATE && has(why, "LEARNER_DQN"));
    c2.shared_q = P2PMG_SHARED_ROLE;  // a tabular role context is still a tabular context
    CHECK(p2pmg::validate_dqn_roles(&c2, &dq, false, 1, false, &why) == P2PMG_E_STATE);
    CHECK(p2pmg::validate_dqn_roles(&cfg, &dq, true, 1, false, &why) == P2PMG_E_STATE && has(why, "already set up"));
    c2 = cfg;
    c2.shared_q = 0;
    CHECK(p2pmg::validate_dqn_roles(&c2, &dq, false, 1, false, &why) == P2PMG_E_INVALID && has(why, "shared_q"));
    // state before arguments: a set-up context says so even with a bad layout
    p2pmg_dqn_config d2 = dq;
    d2.grad_segments = 2;
    CHECK(p2pmg::validate_dqn_roles(&cfg, &d2, true, 1, false, &why) == P2PMG_E_STATE);
  }
  // one rank: a communicator, or a host exchange over several ranks, is refused by name
  CHECK(p2pmg::validate_dqn_roles(&cfg, &dq, false, 2, false, &why) == P2PMG_E_UNSUPPORTED && has(why, "one rank"));
  CHECK(p2pmg::validate_dqn_roles(&cfg, &dq, false, 1, true, &why) == P2PMG_E_UNSUPPORTED && has(why, "one rank"));
  CHECK(p2pmg::validate_dqn_roles_world("comm_init", 1, true, &why) == P2PMG_E_UNSUPPORTED && has(why, "comm_init"));
  CHECK(p2pmg::validate_dqn_roles_world("comm_init", 4, true, &why) == P2PMG_E_UNSUPPORTED);
  CHECK(p2pmg::validate_dqn_roles_world("dqn_set_exchange", 2, false, &why) == P2PMG_E_UNSUPPORTED &&
        has(why, "dqn_set_exchange"));
  CHECK(p2pmg::validate_dqn_roles_world("dqn_set_exchange", 2, false, nullptr) == P2PMG_E_UNSUPPORTED);
  why = "stale";
  CHECK(p2pmg::validate_dqn_roles_world("dqn_set_exchange", 1, false, &why) == P2PMG_OK && why.empty());
  {  // p2pmg_create's own refusal stays: status and reason
    p2pmg_config c2 = cfg;
    c2.shared_q = P2PMG_SHARED_ROLE;
    CHECK(p2pmg::validate_config(&c2, &why) == P2PMG_E_UNSUPPORTED);
    CHECK(why == "create: shared_q = P2PMG_SHARED_ROLE needs learner = TABULAR (a Q-network per role is not built)");
  }
  std::printf("ok %d\n", n_checks);
  return 0;
}
