// p2pmg_plan.h — which kernel family an episode launch gets and what it needs, decided by one pure
// function: no HIP call and no environment read, so a program without a GPU can check it
// (tests/test_cpu_plan.py).  The runtime prepares, launches and records along the plan.
#pragma once
#include "p2pmg.h"

namespace p2pmg {

// The facts of a context the choice depends on.  p2pmg_ctx derives from this: the planner reads the
// context itself, not a copy of it.
struct PlanFacts {
  p2pmg_config cfg{};
  int S = 0, N = 0, R = 0, T = 0, A = 0;
  int n_cu = 256;  // compute units of the device (multiProcessorCount)
  int n_env = 0;
  bool mi_ok = false;        // every max_in inside the fast division range (fdiv in p2pmg_fastmath.h)
  bool battery = false;
  bool roles = false;        // cfg.shared_q == P2PMG_SHARED_ROLE
  bool thermal_set = false;  // p2pmg_set_thermal uploaded values (false: the config's, where sq16 applies)
  bool learning_set = false;  // p2pmg_set_learning uploaded values (false: the config's, where sq16 applies)
  // the launch belongs to a p2pmg_run_episodes_eps call: thresholds per scenario from a device table
  // (no sq16 kernel, no speculative pre-pass for the next launch)
  bool eps_table = false;
  // the uploaded inputs' hazard distance D allows two chained episodes per wave, half an episode apart:
  // D + 4 <= T / 2 (chain_lag_kernel in p2pmg_small.hip, once per upload)
  bool chain_lag_ok = false;
  // ... and four, a quarter episode apart: D + 4 <= T / 4 (adjacent episodes decide)
  bool chain_lag_ok4 = false;
};

// the environment overrides (the runtime reads them once per process)
struct Overrides {
  bool general = false;  // P2PMG_KERNEL=general: neither the fast nor the sq16 kernel
  int spw = 0;           // P2PMG_SPW: scenarios per wave where the arguments leave it automatic
  bool no_spec = false;  // P2PMG_NO_SPEC=1 (profiling only): no producer blocks, so the episode kernel's counters are its own
  bool no_interleave = false;  // P2PMG_INTERLEAVE=0 (A/B runs): chained launches run their episodes one after the other
  int max_groups = 4;          // P2PMG_INTERLEAVE=2 (A/B runs, tests): at most two chained episodes per wave
};

enum class Family { General, Tile, Fast, Sq16 };  // Tile: the general kernel's LDS-tile form
enum class Philox { None, CodesPrepass, InKernel, FastPrepass };  // where a Philox training launch draws

struct EpisodePlan {
  Family family = Family::General;
  Philox philox = Philox::None;
  bool want_ipc = false;        // fast, N = 2: the pre-pass writes round-1 bins per partner action (the kernel's CAND path)
  int spw = 0;                  // scenarios per 64-lane wave
  int rec_narrow = 0;           // fast / sq16: only {reward, cost} requested -> 8-B record rows
  bool packed_records = false;  // the launch writes packed rows (rec_pack) and stamps its own timing events
  bool speculate = false;       // fast: extra workgroups compute the next launch's pre-pass
  bool interleave = false;      // fast, chained: consecutive episodes of an agent in the lane groups of a wave, T / groups steps apart
  int groups = 1;               // ... how many: 1 (serial), 2 (halves of the wave) or 4 (quarters)
  const char* error = nullptr;  // the request is refused (P2PMG_E_INVALID) with this message
};

// n_chain: the episodes of a chained launch
EpisodePlan plan_episode(const PlanFacts& c, const p2pmg_episode_args& args, bool chained, const Overrides& ov,
                         int n_chain = 1);

}  // namespace p2pmg
