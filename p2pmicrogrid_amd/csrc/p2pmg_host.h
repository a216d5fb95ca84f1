// p2pmg_host.h — what the runtime decides without HIP and without a context (p2pmg_host.cpp): the bounds
// of a config and their check.  Includes no HIP header, so a program without a GPU can check it
// (tests/test_cpu_host_unit.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "p2pmg.h"

namespace p2pmg {

constexpr int kMaxAgents = 64;  // agents per scenario: one 64-lane wave holds a scenario (general kernel)
// R + 1 rounds: no kernel limit (rounds 8 and above read their codes per round); the bound only keeps
// the per-step code and record arrays ([T][ceil((R+1)/4)][A], [T][R+1][A]) in 32-bit row counts
constexpr int kMaxRounds1 = 4096;

// What p2pmg_create checks before it allocates a context: P2PMG_OK, or the status create returns, with
// *why (cleared first) the message p2pmg_last_error(NULL) then gives, where there is one.  Not exported.
__attribute__((visibility("hidden"))) int validate_config(const p2pmg_config* cfg, std::string* why);

// One network's learner constants as p2pmg_dqn_set_learning takes them
struct DqnLearn {
  double gamma, tau, lr, clip;
};
// What p2pmg_dqn_set_learning checks before it uploads: P2PMG_OK, or P2PMG_E_INVALID with *why naming the first
// offending network (rows [n_nets]) or agent (penw [n_agents]).  Not exported.
__attribute__((visibility("hidden"))) int validate_dqn_learning(const DqnLearn* rows, int n_nets, const float* penw,
                                                                int n_agents, std::string* why);

// What p2pmg_dqn_setup_roles checks before its first device call, from the context's config and state:
// set_up = a DQN setup call already succeeded, nranks / has_comm = the world the context was given.
// P2PMG_E_STATE (tabular context, or set up), P2PMG_E_INVALID (shared_q = 0, a negative layout, grad_segments
// other than 0 or 1, batch / capacity out of range) or P2PMG_E_UNSUPPORTED (batch != 32, several ranks or a
// communicator), with *why the reason.  Not exported.
__attribute__((visibility("hidden"))) int validate_dqn_roles(const p2pmg_config* cfg, const p2pmg_dqn_config* dq, bool set_up,
                                                             int nranks, bool has_comm, std::string* why);
// A role context refuses a world of several ranks (p2pmg_comm_init, p2pmg_dqn_set_exchange with nranks > 1):
// P2PMG_E_UNSUPPORTED with *why naming `call`; P2PMG_OK for one rank without a communicator.  Not exported.
__attribute__((visibility("hidden"))) int validate_dqn_roles_world(const char* call, int nranks, bool communicator,
                                                                   std::string* why);

// What p2pmg_set_policy_set checks before its first device call: count M >= 1 policies [M][n_states] (or null:
// M empty slots) and the map policy_of [n_agents * n_scenarios] (or null: the default map).  Legal bytes are
// 0 .. n_actions-1 and P2PMG_POLICY_UNVISITED; map entries lie in [0, M).  On P2PMG_OK map_out (where non-null,
// [A]) holds the map in use: policy_of, or the default a (M == A), a % N (M == N), 0 (M == 1), tested in that
// order.  Else P2PMG_E_INVALID with *why naming the first offending byte or entry, and map_out unspecified.
// Not exported.
__attribute__((visibility("hidden"))) int validate_policy_set(int count, const uint8_t* policies, const int32_t* policy_of,
                                                              size_t n_states, int n_actions, int n_agents, int n_scenarios,
                                                              int32_t* map_out, std::string* why);

}  // namespace p2pmg
