// p2pmg_rt_episode.cpp — the episode launch path of the tabular learner and the rule agent:
// validate -> plan (p2pmg_plan.cpp) -> prepare the plan's family -> launch -> finish_launch.
#include <algorithm>
#include <cmath>

#include "p2pmg_ctx.h"

using namespace p2pmg::rt;
using p2pmg::EpisodeParams;
using p2pmg::EpisodePlan;
using p2pmg::Family;

// the unpacked record arrays as they exist now (ensure_records allocates them on demand)
static void bind_records(p2pmg_ctx* c, EpisodeParams& p) {
  p.rec_reward = c->rec_f32[0];
  p.rec_cost = c->rec_f32[1];
  p.rec_grid = c->rec_f32[2];
  p.rec_p2p = c->rec_f32[3];
  p.rec_tin = c->rec_f32[4];
  p.rec_action = c->rec_action;
  p.rec_index = c->rec_index;
}

namespace p2pmg::rt {

EpisodeParams episode_params(p2pmg_ctx* c, const p2pmg_episode_args* args) {
  const bool train = args->mode != P2PMG_MODE_GREEDY;
  const p2pmg_config& g = c->cfg;
  EpisodeParams p{};
  p.S = c->S;
  p.N = c->N;
  p.R = c->R;
  p.T = c->T;
  p.A = c->A;
  p.mode = args->mode;
  p.rng = 0;
  p.episode = args->episode;
  p.record = args->record;
  p.n_env = c->n_env;
  p.env = c->env;
  p.prof = c->prof;
  p.max_in = c->max_in;
  p.t_in = c->t_in;
  p.t_m = c->t_m;
  p.q = c->q;
  p.codes = c->codes;
  p.eps = args->epsilon;
  p2pmg::eps_threshold(p.eps, p.eps_thr, p.eps_all);
  if (train && args->rng == P2PMG_RNG_PHILOX) p.rng = 1;  // in-kernel unless the pre-pass below runs
  p.seed_lo = (uint32_t)(g.seed & 0xFFFFFFFFu);
  p.seed_hi = (uint32_t)(g.seed >> 32);
  p.agent_offset = (uint32_t)(g.scenario_offset * c->N);
  bind_records(c, p);
  p.ep_reward = c->ep_reward;
  p.shared_q = c->roles ? 2 : g.shared_q ? 1 : 0;
  p.qdelta = c->qdelta;
  p.battery = c->battery ? 1 : 0;
  p.bat_safe = (c->battery && c->bat_domain && c->prof_bounded && c->hp_bounded) ? 1 : 0;
  p.soc = c->soc;
  p.bat_cap = c->bat_cap;
  p.bat_min = c->bat_min;
  p.bat_max = c->bat_max;
  p.bat_sqrt_eff = c->bat_sqrt_eff;
  p.hp_lv = c->hp_lv;
  p.thermal = c->thermal;
  p.learn = c->learn;
  p.eps_tab = c->eps_table ? c->eps_cur : nullptr;
  p.dummy = c->dummy;
  p.nt = g.n_time_states;
  p.nT = g.n_temp_states;
  p.nb = g.n_balance_states;
  p.np = g.n_p2p_states;
  p.alpha = g.alpha;
  p.gamma = g.gamma;
  for (int k = 0; k < 4; ++k) p.hp_levels[k] = g.hp_levels[k];
  p.setpoint = g.setpoint;
  p.margin = g.temp_margin;
  p.lower = g.lower_bound;
  p.upper = g.upper_bound;
  p.inv_ci = g.inv_ci;
  p.inv_cm = g.inv_cm;
  p.inv_ri = g.inv_ri;
  p.inv_re = g.inv_re;
  p.inv_rvent = g.inv_rvent;
  p.c_in = g.one_minus_frad;
  p.c_m = g.frad;
  p.solar = g.solar_gain;
  p.cop = g.hp_cop;
  p.spm = g.seconds_per_minute;
  p.slot = g.time_slot;
  p.mph = g.minutes_per_hour;
  p.kilo = g.kilo;
  p.penw = g.penalty_weight;
  return p;
}

}  // namespace p2pmg::rt

namespace {

// a chained fast-path launch (p2pmg_run_episodes): n episodes at eps[0..n), the caller's guess of
// the next chain (next_n episodes at next_eps) for the speculative pre-pass, rewards [n][S] on device
struct ChainReq {
  int n;
  const double* eps;
  int next_n;
  const double* next_eps;
  float* rewards;
  int reserve;  // code-word capacity to allocate, in episodes (every chain of the call fits)
};

// fast / sq16 write packed rows (rec_pack) that p2pmg_get_record unpacks into one staging buffer, so
// those launches allocate no [T][A] arrays per record (configs[3] at full size: 35 GB less)
int ensure_rec_pack(p2pmg_ctx* c, const p2pmg_episode_args* args) {
  if (args->record && !c->rec_pack) HIP_TRY(c, c->rec_pack.alloc((size_t)c->T * c->A * p2pmg::kFastRecBytes));
  return P2PMG_OK;
}

// The fast kernel: both pre-pass slots and their code words, this slot's pre-pass unless the previous
// launch computed it, and the next slot's description (next) for this launch's producer workgroups.
int prepare_fast(p2pmg_ctx* c, const p2pmg_episode_args* args, const ChainReq* ch, const EpisodePlan& plan,
                 EpisodeParams& p, p2pmg::PrepOut* next) {
  const int ps = c->pslot;
  const size_t ta = (size_t)c->T * c->A;
  const size_t wpe = ta * ((c->R + 4) / 4);  // code words per episode
  const bool philox = plan.philox == p2pmg::Philox::FastPrepass;
  // this launch's chain (one episode unless chained) and the caller's guess of the next launch's:
  // P2PMG_FLAG_NEXT_EPSILON: next_epsilon is the guess as given (0 included); without it a
  // positive next_epsilon is the guess and anything else means "the same epsilon"
  std::vector<double> cur(ch ? ch->eps : &args->epsilon, ch ? ch->eps + ch->n : &args->epsilon + 1);
  std::vector<double> nxt_eps;
  if (ch) {
    if (ch->next_n > 0) nxt_eps.assign(ch->next_eps, ch->next_eps + ch->next_n);
    else nxt_eps.assign(cur.size(), cur.back());
  } else {
    const bool have_next = (args->flags & P2PMG_FLAG_NEXT_EPSILON) != 0 || args->next_epsilon > 0.0;
    nxt_eps.assign(1, have_next ? args->next_epsilon : args->epsilon);
  }
  const int n_ep = (int)cur.size(), n_next = (int)nxt_eps.size();
  for (int k = 0; k < 2; ++k) {  // both slots (the launch writes the other one)
    if (!c->pre[k]) HIP_TRY(c, c->pre[k].alloc(ta));
    if (plan.want_ipc && !c->pre_ipc[k]) HIP_TRY(c, c->pre_ipc[k].alloc(ta));
    const size_t need = wpe * (size_t)std::max(n_ep, n_next);
    if (philox && c->pcodes[k].cap() < need) {  // chains: their full capacity at once (no reallocation later)
      c->spec_valid[k] = false;
      HIP_TRY(c, c->pcodes[k].alloc(std::max(need, wpe * (size_t)(ch ? ch->reserve : 1))));
    }
  }
  p.pre_ipc = plan.want_ipc ? c->pre_ipc[ps].get() : nullptr;
  if (philox) p.codes = c->pcodes[ps];
  p.rng = 0;
  p.chain = n_ep;
  p.codes_stride = wpe;
  p.chain_rewards = ch ? ch->rewards : nullptr;
  RC_TRY(ensure_rec_pack(c, args));
  auto prep_out = [&](int slot, int episode, const std::vector<double>& eps) {
    p2pmg::PrepOut o{c->pre[slot], plan.want_ipc ? c->pre_ipc[slot].get() : nullptr,
                     philox ? c->pcodes[slot].get() : nullptr, episode, eps[0], 0u, 0};
    p2pmg::eps_threshold(eps[0], o.eps_thr, o.eps_all);
    o.n_ep = (int)eps.size();
    o.words_stride = wpe;
    o.eps_tab = nullptr;
    o.ep_all = 0;
    for (int k = 0; k < o.n_ep; ++k) {
      int all = 0;
      p2pmg::eps_threshold(eps[k], o.ep_thr[k], all);
      o.ep_all |= (uint64_t)all << k;
    }
    return o;
  };
  // this slot's pre-pass: computed by the previous launch if it guessed these arguments
  if (c->eps_table) {
    // a per-scenario epsilon table: this launch's own pre-pass from its rows, no speculation, and
    // neither slot left for a later plain launch to take as a hit
    p2pmg::PrepOut o = prep_out(ps, args->episode, cur);
    o.eps_tab = c->eps_cur;
    HIP_TRY(c, p2pmg::launch_step_prepass(p, o, c->stream));
    *next = prep_out(ps ^ 1, args->episode + n_ep, nxt_eps);  // unused: the plan does not speculate
    c->spec_misses++;
    c->spec_valid[0] = c->spec_valid[1] = false;
    return P2PMG_OK;
  }
  const bool hit = c->spec_valid[ps] && c->spec_version[ps] == c->inputs_version &&
                   (!philox || (c->spec_episode[ps] == args->episode && c->spec_chain[ps] == cur));
  if (!hit) HIP_TRY(c, p2pmg::launch_step_prepass(p, prep_out(ps, args->episode, cur), c->stream));
  // the next slot, for the episodes after this launch's at the caller's guess (the decay schedule
  // is known, community.py:279-286).  Philox draws only when this one has them.
  const int ns = ps ^ 1;
  *next = prep_out(ns, args->episode + n_ep, nxt_eps);
  if (hit) c->spec_hits++;
  else c->spec_misses++;
  c->spec_valid[ns] = plan.speculate;
  c->spec_version[ns] = c->inputs_version;
  c->spec_episode[ns] = philox ? args->episode + n_ep : -1;
  c->spec_chain[ns] = nxt_eps;
  return P2PMG_OK;
}

// The Philox code words of a launch whose plan draws them ahead of it (Philox::CodesPrepass): the
// kernel then reads them like uploaded replay codes (p.rng = 0)
int codes_prepass(p2pmg_ctx* c, EpisodeParams& p) {
  RC_TRY(ensure_codes(c));
  p.codes = c->codes;
  HIP_TRY(c, p2pmg::launch_philox_codes(p, c->codes, c->stream));
  c->code_src = 2;
  c->have_codes = false;  // a replay upload must be repeated after a pre-pass overwrote it
  p.rng = 0;
  return P2PMG_OK;
}

// The sq16 kernel: the step words {balance, time / balance row offset}, recomputed after any input upload;
// the Philox draws in the kernel unless the caller asked for the pre-pass (P2PMG_FLAG_PHILOX_PREPASS)
int prepare_sq16(p2pmg_ctx* c, const p2pmg_episode_args* args, const EpisodePlan& plan, EpisodeParams& p) {
  RC_TRY(ensure_rec_pack(c, args));
  p.rec_pack = c->rec_pack;
  if (!c->sqp) HIP_TRY(c, c->sqp.alloc((size_t)c->T * c->A));
  if (c->sqp_version != c->inputs_version) {
    HIP_TRY(c, p2pmg::launch_sq16_prep(p, c->sqp, c->stream));
    c->sqp_version = c->inputs_version;
  }
  p.sqp = c->sqp;
  return plan.philox == p2pmg::Philox::CodesPrepass ? codes_prepass(c, p) : P2PMG_OK;
}

// The general kernel (either form): unpacked record arrays, and the Philox code words where the
// plan draws them ahead of the launch
int prepare_general(p2pmg_ctx* c, const p2pmg_episode_args* args, const EpisodePlan& plan, EpisodeParams& p) {
  RC_TRY(ensure_records(c, args->record));
  bind_records(c, p);
  return plan.philox == p2pmg::Philox::CodesPrepass ? codes_prepass(c, p) : P2PMG_OK;
}

// The hazard distance of the uploaded inputs, from the pre-pass words the launch is about to read: one
// small kernel and a 4-byte read-back per upload (the inputs stay put between launches in real use).
int update_chain_lag(p2pmg_ctx* c, const uint2* pre) {
  if (c->lag_version == c->inputs_version) return P2PMG_OK;
  c->chain_lag = -1;
  if (c->T <= p2pmg::kChainLagMaxT) {
    if (!c->d_lag) HIP_TRY(c, c->d_lag.alloc(1));
    HIP_TRY(c, p2pmg::launch_chain_lag(c->T, c->A, pre, c->d_lag, c->stream));
    RC_TRY(download(c, {{&c->chain_lag, c->d_lag, sizeof(int)}}));
  }
  c->chain_lag_ok = c->chain_lag >= 0 && c->chain_lag + 4 <= c->T / 2;
  c->chain_lag_ok4 = c->chain_lag >= 0 && c->chain_lag + 4 <= c->T / 4;
  c->lag_version = c->inputs_version;
  return P2PMG_OK;
}

// validate -> plan -> prepare the plan's family -> launch -> finish_launch
int run_episode_impl(p2pmg_ctx* c, const p2pmg_episode_args* args, const ChainReq* ch) {
  if (!c || !args) return P2PMG_E_INVALID;
  if (c->dqn) return dqn_run_episode(c, args);
  if (c->cfg.n_actions != 3) return fail(c, P2PMG_E_UNSUPPORTED, "run_episode: the kernels act on 3 actions (this context only holds tables)");
  if (!c->have_env || !c->have_prof || !c->have_params)
    return fail(c, P2PMG_E_STATE, "run_episode: env, profiles and agent params must be set first");
  const bool train = args->mode == P2PMG_MODE_TRAIN;
  if (args->mode != P2PMG_MODE_TRAIN && args->mode != P2PMG_MODE_GREEDY) return fail(c, P2PMG_E_INVALID, "mode");
  if (train && args->rng != P2PMG_RNG_REPLAY && args->rng != P2PMG_RNG_PHILOX) return fail(c, P2PMG_E_INVALID, "rng");
  if (train && args->rng == P2PMG_RNG_REPLAY && !c->have_codes)
    return fail(c, P2PMG_E_STATE, "run_episode: replay mode needs p2pmg_set_replay_codes");
  EpisodePlan plan = p2pmg::plan_episode(*c, *args, ch != nullptr, overrides(), ch ? ch->n : 1);
  if (plan.error) return fail(c, P2PMG_E_INVALID, plan.error);
  const p2pmg_config& g = c->cfg;
  const bool fast = plan.family == Family::Fast, sq16 = plan.family == Family::Sq16, tile = plan.family == Family::Tile;
  const bool ext = plan.packed_records;
  EpisodeParams p = episode_params(c, args);
  const int ps = c->pslot;
  p2pmg::PrepOut next{};
  RC_TRY(fast ? prepare_fast(c, args, ch, plan, p, &next) : sq16 ? prepare_sq16(c, args, plan, p) : prepare_general(c, args, plan, p));
  if (fast && ch && c->lag_version != c->inputs_version) {  // the first chained launch after an upload
    RC_TRY(update_chain_lag(c, c->pre[ps]));
    plan = p2pmg::plan_episode(*c, *args, true, overrides(), ch->n);  // ... with the fact it was missing
  }
  p.interleave = plan.interleave ? plan.groups : 0;
  p.rec_narrow = plan.rec_narrow;
  const bool reset = (args->flags & P2PMG_FLAG_RESET_T0) != 0;
  p.reset_t0 = (ext && reset) ? 1 : 0;
  p.reset_sigma = args->reset_sigma;
  Timed tm;
  RC_TRY(begin_timed(c, true, !ext, &tm));
  hipError_t e = fast   ? p2pmg::launch_episode_fast(p, c->pre[ps], c->rec_pack, g.q_dtype, plan.spw,
                                                    plan.speculate ? &next : nullptr, tm.e0, tm.e1, c->stream)
                 : sq16 ? p2pmg::launch_episode_sq16(p, g.q_dtype, tm.e0, tm.e1, c->stream)
                        : p2pmg::launch_episode(p, g.q_dtype, tile, c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("episode launch: ") + hipGetErrorString(e));
  RC_TRY(end_timed(c, tm, !ext));
  if (fast) c->pslot ^= 1;
  if (reset && !ext) {  // general kernel: the reset as its own launch
    const uint32_t off = (uint32_t)(g.scenario_offset * c->N);
    HIP_TRY(c, p2pmg::launch_t0_philox(c->A, c->t_in, c->t_m, p.seed_lo, p.seed_hi, args->episode + 1, off,
                                       c->thermal, args->reset_sigma, c->stream));
  }
  finish_launch(c, tm,
                std::string(fast ? "episode_fast_kernel<" : sq16 ? "episode_sq16_kernel<" : "episode_kernel<") +
                    std::to_string(c->N) + (tile ? ",tile" + std::to_string(p2pmg::general_tile_cap(c->N)) : "") + "," +
                    (g.q_dtype == 0 ? "f64" : "f32") + ",R1=" + std::to_string(c->R + 1) +
                    (ext ? (train ? ",train" : ",greedy") : "") + (g.shared_q ? ",shared" : "") + (c->roles ? ",roles" : "") +
                    // sq16 draws in the kernel by default: a launch that read pre-pass code words instead says so
                    (sq16 && plan.philox == p2pmg::Philox::CodesPrepass ? ",philox-prepass" : "") +
                    (c->battery ? (ext && !p.bat_safe ? ",battery,range-checked>" : ",battery>")
                                : plan.interleave ? ",K=" + std::to_string(plan.groups) + ",interleaved>" : ">"),
                args->record, ext ? (args->record & 127) : 0, plan.rec_narrow);
  return P2PMG_OK;
}

// n episodes at epsilons[k]; with c->eps_table, at the rows of c->eps_tab instead (epsilons: scenario 0's)
int run_episodes_impl(p2pmg_ctx* c, const p2pmg_episode_args* args, int n, const double* epsilons, int next_n,
                      const double* next_epsilons) {
  if (c->cfg.n_actions != 3) return fail(c, P2PMG_E_UNSUPPORTED, "run_episodes: the kernels act on 3 actions (this context only holds tables)");
  if (!c->dqn && (!c->have_env || !c->have_prof || !c->have_params))
    return fail(c, P2PMG_E_STATE, "run_episodes: env, profiles and agent params must be set first");
  // at least one full chain's worth, so a caller's chains never reallocate
  HIP_TRY(c, c->chain_rew.grow((size_t)std::max(n, p2pmg::kMaxChain) * c->S));
  c->chain_n = 0;
  const bool chain = !c->dqn && p2pmg::plan_episode(*c, *args, false, overrides()).philox == p2pmg::Philox::FastPrepass;
  p2pmg_episode_args a = *args;
  if (!chain) {  // one launch per episode, the same results
    for (int k = 0; k < n; ++k) {
      a.episode = args->episode + k;
      a.epsilon = epsilons[k];
      a.flags = args->flags | P2PMG_FLAG_NEXT_EPSILON;
      a.next_epsilon = k + 1 < n ? epsilons[k + 1] : next_n > 0 ? next_epsilons[0] : epsilons[k];
      if (c->eps_table) c->eps_cur = c->eps_tab + (size_t)k * c->S;  // this episode's row
      RC_TRY(run_episode_impl(c, &a, nullptr));
      HIP_TRY(c, hipMemcpyAsync(c->chain_rew + (size_t)k * c->S, c->ep_reward,
                                (size_t)c->S * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    c->chain_n = n;
    return P2PMG_OK;
  }
  // chains of at most kMaxChain episodes whose code words fit 1 GiB per slot
  const size_t wpe_bytes = (size_t)c->T * c->A * ((c->R + 4) / 4) * sizeof(uint32_t);
  const int per = (int)std::max<size_t>(1, std::min<size_t>(p2pmg::kMaxChain, ((size_t)1 << 30) / wpe_bytes));
  for (int k0 = 0; k0 < n; k0 += per) {
    const int m = std::min(per, n - k0);
    const int k1 = k0 + m;
    ChainReq req{m, epsilons + k0, 0, nullptr, c->chain_rew + (size_t)k0 * c->S, per};
    if (k1 < n) {
      req.next_n = std::min(per, n - k1);
      req.next_eps = epsilons + k1;
    } else if (next_n > 0) {
      req.next_n = std::min(per, next_n);
      req.next_eps = next_epsilons;
    }
    a.episode = args->episode + k0;
    a.epsilon = epsilons[k0];
    if (c->eps_table) c->eps_cur = c->eps_tab + (size_t)k0 * c->S;  // this part's rows
    RC_TRY(run_episode_impl(c, &a, &req));
  }
  c->chain_n = n;
  return P2PMG_OK;
}

}  // namespace

extern "C" {

int p2pmg_run_episode(p2pmg_ctx* c, const p2pmg_episode_args* args) {
  if (c) c->chain_n = 0;  // p2pmg_get_episode_rewards covers p2pmg_run_episodes calls only
  return run_episode_impl(c, args, nullptr);
}

int p2pmg_run_episodes(p2pmg_ctx* c, const p2pmg_episode_args* args, int n, const double* epsilons, int next_n,
                       const double* next_epsilons) {
  if (!c || !args || n < 1 || !epsilons || (next_n > 0 && !next_epsilons)) return P2PMG_E_INVALID;
  return run_episodes_impl(c, args, n, epsilons, next_n, next_epsilons);
}

int p2pmg_run_episodes_eps(p2pmg_ctx* c, const p2pmg_episode_args* args, int n, const double* eps) {
  if (!c || !args || n < 1 || !eps) return P2PMG_E_INVALID;
  if (c->dqn) return fail(c, P2PMG_E_UNSUPPORTED, "run_episodes_eps: tabular contexts only");
  if (args->mode != P2PMG_MODE_TRAIN || args->rng != P2PMG_RNG_PHILOX)
    return fail(c, P2PMG_E_INVALID, "run_episodes_eps: Philox training only (replay codes carry each agent's own epsilon)");
  const size_t S = (size_t)c->S, cells = (size_t)n * S;
  std::vector<uint2> tab(cells);
  std::vector<double> first((size_t)n);  // scenario 0's schedule: what the plan's heuristics read
  for (size_t k = 0; k < cells; ++k) {
    if (!(std::isfinite(eps[k]) && eps[k] >= 0.0 && eps[k] <= 1.0))
      return fail(c, P2PMG_E_INVALID, "run_episodes_eps: epsilon outside [0, 1] at entry " + std::to_string(k));
    int all = 0;
    p2pmg::eps_threshold(eps[k], tab[k].x, all);
    tab[k].y = (uint32_t)all;
  }
  for (int k = 0; k < n; ++k) first[(size_t)k] = eps[(size_t)k * S];
  HIP_TRY(c, c->eps_tab.grow(cells));
  RC_TRY(upload(c, {{c->eps_tab, tab.data(), cells * sizeof(uint2)}}));
  c->eps_table = true;
  c->eps_cur = c->eps_tab;
  const int rc = run_episodes_impl(c, args, n, first.data(), 0, nullptr);
  c->eps_table = false;
  c->eps_cur = nullptr;
  return rc;
}

int p2pmg_chain_lag(p2pmg_ctx* c, int* distance, int* safe) {
  if (!c) return P2PMG_E_INVALID;
  if (c->lag_version != c->inputs_version)
    return fail(c, P2PMG_E_STATE, "chain_lag: no chained launch has run since the last input upload");
  if (distance) *distance = c->chain_lag;
  if (safe) *safe = c->chain_lag_ok ? 1 : 0;
  return P2PMG_OK;
}

int p2pmg_run_rule_episode(p2pmg_ctx* c, int record) {
  if (!c) return P2PMG_E_INVALID;
  if (c->dqn) return fail(c, P2PMG_E_STATE, "run_rule_episode: DQN context");
  if (!c->have_env || !c->have_prof || !c->have_params)
    return fail(c, P2PMG_E_STATE, "run_rule_episode: env, profiles and agent params must be set first");
  if (c->R != 0)  // the reference's tensor_diag_part on the (N, 1) stack fails for rounds > 0
    return fail(c, P2PMG_E_INVALID, "run_rule_episode: RuleAgent communities run with rounds = 0");
  if (c->N > 64) return fail(c, P2PMG_E_INVALID, "run_rule_episode: N <= 64");
  const int rec = record & (P2PMG_REC_COST | P2PMG_REC_GRID | P2PMG_REC_P2P | P2PMG_REC_TEMP | P2PMG_REC_ACTION);
  int rc = ensure_records(c, rec);
  if (rc == P2PMG_OK) rc = ensure_hp_on(c);
  if (rc != P2PMG_OK) return rc;
  p2pmg_episode_args args{};
  args.mode = P2PMG_MODE_GREEDY;
  args.record = rec;
  EpisodeParams p = episode_params(c, &args);
  Timed tm;
  RC_TRY(begin_timed(c, false, true, &tm));
  HIP_TRY(c, p2pmg::launch_rule_episode(p, c->hp_on, c->stream));
  RC_TRY(end_timed(c, tm, true));
  finish_launch(c, tm, "rule_episode_kernel<" + std::to_string(c->N) + ">", rec, 0, 0);
  return P2PMG_OK;
}

}  // extern "C"
