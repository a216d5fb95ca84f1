// p2pmg_plan.cpp — the launch plan (p2pmg_plan.h).  Pure: arithmetic on its arguments only.
#include "p2pmg_plan.h"

#include <algorithm>
#include <cmath>

#include "p2pmg_internal.h"

namespace p2pmg {
namespace {

// divisors the fast kernel divides by with the range-free quotient (fdiv_b in p2pmg_fastmath.h)
bool host_div_range(float b) {
  const float m = std::fabs(b);
  return m >= 0x1p-40f && m <= 0x1p40f;
}

// fast per-agent-table path (episode_fast_kernel): automatic whenever it applies
bool fast_applies(const PlanFacts& c, const p2pmg_episode_args& args, const Overrides& ov) {
  const p2pmg_config& g = c.cfg;
  return !g.shared_q && (!c.battery || c.R + 1 <= kFastBatMaxR1) && c.N <= 8 && c.R + 1 <= 4 && c.mi_ok &&
         (long long)g.n_time_states * g.n_temp_states * g.n_balance_states < 65536 &&
         // a wave's 64 tables span < 4 GiB (the gathers' 32-bit offsets)
         64LL * g.n_time_states * g.n_temp_states * g.n_balance_states * g.n_p2p_states * 4 * (g.q_dtype == 0 ? 8 : 4) <
             (1LL << 32) &&
         (long long)c.T * c.A < (1LL << 32) && host_div_range(g.minutes_per_hour) &&
         g.temp_margin == 1.0f &&  // heating.py:90 (the kernel skips the / margin)
         !(args.flags & (P2PMG_FLAG_GENERAL_KERNEL | P2PMG_FLAG_TILE_KERNEL | P2PMG_FLAG_PHILOX_INKERNEL)) &&
         !ov.general;
}

}  // namespace

EpisodePlan plan_episode(const PlanFacts& c, const p2pmg_episode_args& args, bool chained, const Overrides& ov,
                         int n_chain) {
  const p2pmg_config& g = c.cfg;
  const bool train = args.mode == P2PMG_MODE_TRAIN;
  const bool philox = train && args.rng == P2PMG_RNG_PHILOX;
  const bool fast = fast_applies(c, args, ov);
  EpisodePlan pl;
  if (chained && !(fast && philox)) {
    pl.error = "run_episode: a chained launch needs the fast kernel and Philox training";
    return pl;
  }
  // shared table, 16-agent scenarios (configs[2]): episode_sq16_kernel
  const bool sq16 = g.shared_q && !c.roles && c.N == 16 && c.R <= 1 && c.mi_ok && host_div_range(g.minutes_per_hour) &&
                    (long long)c.T * c.A < (1LL << 32) && (long long)c.T * c.n_env * kEnvStride < (1LL << 32) &&
                    host_div_range(g.temp_margin) && g.n_time_states == 20 && g.n_temp_states == 20 &&
                    g.n_balance_states == 20 && g.n_p2p_states == 20 &&
                    !c.thermal_set &&  // per-agent thermal parameters: the general kernel's shared-table form
                    !c.learning_set && !c.eps_table &&  // ... as for per-agent learner constants, per-scenario epsilon
                    !(args.flags & (P2PMG_FLAG_GENERAL_KERNEL | P2PMG_FLAG_TILE_KERNEL)) && !ov.general;
  // the general kernel's LDS-tile form: every N outside {1..8, 16}, or any N on request
  const bool tile = !fast && !sq16 &&
                    ((args.flags & P2PMG_FLAG_TILE_KERNEL) != 0 || !((c.N >= 1 && c.N <= 8) || c.N == 16));
  pl.family = fast ? Family::Fast : sq16 ? Family::Sq16 : tile ? Family::Tile : Family::General;
  if (fast) {
    pl.philox = philox ? Philox::FastPrepass : Philox::None;
  } else if (philox) {
    bool prepass = c.A < (1 << 18) && !sq16;  // sq16: throughput-bound, draws in the kernel
    if (args.flags & P2PMG_FLAG_PHILOX_PREPASS) prepass = true;
    if (args.flags & P2PMG_FLAG_PHILOX_INKERNEL) prepass = false;
    pl.philox = prepass ? Philox::CodesPrepass : Philox::InKernel;
  }
  pl.want_ipc = fast && c.N == 2 && c.R >= 1 && !c.battery;
  pl.packed_records = fast || sq16;
  pl.rec_narrow = (fast || sq16) && (args.record & ~(P2PMG_REC_REWARD | P2PMG_REC_COST)) == 0 ? 1 : 0;
  pl.speculate = fast && !ov.no_spec && !c.eps_table;
  // two chained episodes per wave (episode_fast_kernel's PIPE form, instantiated for N = 2): the later
  // episode starts from its own T0 draw (the reset), and the uploaded inputs keep the two episodes'
  // table rows apart (chain_lag_ok)
  pl.interleave = fast && chained && n_chain >= 2 && philox && (args.flags & P2PMG_FLAG_RESET_T0) != 0 && !c.battery &&
                  c.T % 6 == 0 && g.n_temp_states <= 32 && c.N == 2 && c.chain_lag_ok && !ov.no_interleave;
  // four, a quarter episode apart, where the phases keep the input ring's rotation (T % 12 == 0), the
  // hazard distance fits a quarter (chain_lag_ok4) and the chain fills every group; else two under the
  // rule above, else the serial chain
  const bool quad = pl.interleave && c.T % 12 == 0 && c.chain_lag_ok4 && n_chain >= 4 && ov.max_groups >= 4;
  pl.groups = quad ? 4 : pl.interleave ? 2 : 1;
  int spw = args.scen_per_wave > 0 ? args.scen_per_wave : ov.spw;
  if (spw <= 0) {  // automatic: full waves, or spread a small batch over all CUs (one wave per CU)
    const int full = 64 / (c.N <= 1 ? 1 : c.N <= 2 ? 2 : c.N <= 4 ? 4 : 8);
    const int waves = (c.S + full - 1) / full;
    spw = waves >= c.n_cu ? full : std::max(full / 4, (c.S + c.n_cu - 1) / c.n_cu);
    // below epsilon 0.5 most lanes are greedy (a round-0 row gather and two argmaxes on every step):
    // there half-filled waves, two per CU, measured faster (configs[1], chained: 80.7 -> 77.9 us per
    // episode at epsilon 0.1, 76.1 -> 75.0 at 0.39, even at 0.53), above it one wave per CU
    // (71.7 against 73.9 us at 0.729): profiles/r05_chain/spw_epsilon.txt
    if (fast && train && args.epsilon < 0.5 && waves < c.n_cu) spw = std::max(full / 4, (spw + 1) / 2);
    spw = std::min(spw, full);
  }
  if (pl.interleave) spw = std::min(spw, 64 / pl.groups / 2);  // a scenario's lanes stay inside one lane group (N = 2)
  pl.spw = spw;
  return pl;
}

}  // namespace p2pmg
