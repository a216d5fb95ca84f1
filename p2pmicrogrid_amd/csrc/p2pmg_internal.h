// Internal declarations shared by the kernel units (device code + launchers: p2pmg_general.hip,
// p2pmg_fast.hip, p2pmg_sq16.hip, p2pmg_small.hip, p2pmg_dqn_*.hip, p2pmg_summary.hip, p2pmg_tables.hip) and
// the runtime units (p2pmg_rt_*.cpp: context, C ABI; their own shared header is p2pmg_ctx.h).  Not part of
// the public ABI (include/p2pmg.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p2pmg_host.h"  // kMaxAgents, kMaxRounds1

namespace p2pmg {

constexpr int kEnvStride = 8;  // floats per env row: time, t_out, buy, inj, p2p, pad x3
constexpr int kQPad = 4;       // Q row padded to 4 actions: 32-B (f64) / 16-B (f32) aligned rows
constexpr int kWave = 64;      // one wave per workgroup
// capacity of the general kernel's LDS-tile form for n agents (16, 32 or 64)
inline constexpr int general_tile_cap(int n) { return n <= 16 ? 16 : (n <= 32 ? 32 : 64); }
constexpr double kDeltaScale = 1099511627776.0;  // 2^40: shared-table TD deltas in int64 fixed point
// shared-table delta replicas: workgroup b accumulates into copy (b % 8), i.e. its own XCD\'s copy
// (blocks are dealt round-robin over the 8 XCDs); the copies are folded before use
constexpr int kDeltaCopies = 8;

// One agent's learner constants, a 32-B row (p2pmg_set_learning): two 16-B loads in a kernel's prologue
struct LearnRow {
  double alpha, gamma;
  float penw, pad[3];
};
static_assert(sizeof(LearnRow) == 32, "learning rows are 32 bytes");

// Everything the episode kernel needs, passed by value in the kernarg segment.
struct EpisodeParams {
  int S, N, R, T, A;
  int mode, rng, episode, record;  // rng: 0 = code words buffer, 1 = in-kernel Philox
  int n_env;                 // 1 (shared environment) or S (one per scenario)
  const float* env;          // [T][n_env][kEnvStride] time-major
  const float2* prof;        // [T][A] {load_w, pv_w}
  const uint2* sqp;          // sq16 path: [T][A] {bits(balance), it * 8000 + ib * 20} (sq16_prep_kernel)
  const float* max_in;       // [A]
  float* t_in;               // [A] in/out
  float* t_m;                // [A] in/out
  void* q;                   // [A][n_states][kQPad] f64 | f32
  const uint32_t* codes;     // [T][W][A] code words, W = ceil((R+1)/4), one byte per round (255 = greedy)
  double eps;
  // explore test u < eps of a Philox word w (u = w / 2^32, exact) as an integer compare:
  // eps_all || w < eps_thr (eps_threshold below, set with eps)
  uint32_t eps_thr;
  int eps_all;
  uint32_t seed_lo, seed_hi;
  uint32_t agent_offset;     // global id of local agent 0 (Philox counter)
  float* rec_reward;         // [T][A]
  float* rec_cost;
  float* rec_grid;
  float* rec_p2p;
  float* rec_tin;
  uint8_t* rec_action;       // [T][R+1][A]
  int32_t* rec_index;        // [T][R+1][A]
  float* ep_reward;          // [S]
  // shared policy (config 3): every agent reads one frozen table; TD deltas accumulate in
  // int64 fixed point (2^-40) with device atomics, applied at episode end (p2pmg_apply_q_delta)
  int shared_q;              // 0 per-agent tables, 1 one table, 2 one table per role (agent position): [N] tables
  long long* qdelta;         // [kDeltaCopies][tables][n_states][kQPad] int64 (one replica per XCD)
  // battery (agent.py:138-153 rule, storage.py:36-76 bookkeeping), f64 like the reference
  int battery;
  double* soc;               // [A] in/out
  const double* bat_cap;     // [A] capacity in J (0 = no battery)
  double bat_min, bat_max, bat_sqrt_eff;
  int bat_safe;              // the battery operands lie in battery_rule_r<false>'s verified domain
  const float4* hp_lv;       // [A] per-agent heat-pump power of actions 0..2 (agent.py:268, heating.py:124)
  // [A] per-agent {setpoint, lower bound, upper bound, COP} (HPHeating / HeatPump, heating.py:92-130).
  // Every kernel but episode_sq16_kernel reads these, not the scalars below (which fill the array
  // at p2pmg_create and stay the sq16 kernel's SGPR constants).
  const float4* thermal;
  // [A] per-agent learner constants (QActor's own alpha and gamma, rl.py:58-71, and the agent's comfort
  // weight): every tabular kernel but episode_sq16_kernel reads these, not alpha / gamma / penw below
  // (which fill the array at p2pmg_create and stay the sq16 kernel's constants)
  const LearnRow* learn;
  // per-scenario exploration thresholds of this launch (p2pmg_run_episodes_eps): [chain rows][S]
  // {eps_thr, eps_all}, row k for episode + k; null: eps_thr / eps_all above for every scenario
  const uint2* eps_tab;
  void* dummy;               // >= 2 * kWave * 32 B scratch: target of the fast kernel's masked-off stores
  uint32_t* pre_ipc;         // fast path, N = 2: [T][A] round-1 p2p bins for the partner's 3 round-0 actions
  void* rec_pack;            // fast paths: packed records [T][A] x 32 B
  int rec_narrow;            // fast / sq16: only reward + cost requested -> records are [T][A] float2
  int reset_t0;              // fast path: draw T0 for episode + 1 at the end (P2PMG_FLAG_RESET_T0)
  double reset_sigma;
  // fast path, chained launch (p2pmg_run_episodes): `chain` consecutive training episodes
  // (episode + k, k < chain) in one launch, each wave running them back to back; episode k reads
  // its code words at codes + k * codes_stride and writes its episode reward to
  // chain_rewards[k * S + s] (when non-null).  0 or 1: one episode.
  int chain;
  // chained launch: episodes e and e + 1 of an agent run in the two halves of a wave, T / 2 steps
  // apart (the plan's interleave; the kernel's PIPE form): the lane groups per wave, 0 (serial), 2 or 4
  int interleave;
  size_t codes_stride;
  float* chain_rewards;
  int nt, nT, nb, np;
  double alpha, gamma;
  float hp_levels[4];
  float setpoint, margin, lower, upper;
  float inv_ci, inv_cm, inv_ri, inv_re, inv_rvent, c_in, c_m, solar, cop, spm, slot;
  float mph, kilo, penw;
};

// ---- DQN variant (rl.py:135-359): QNetwork 5 -> 64 -> 64 -> 1 in Keras weight order
constexpr int kNetStride = 4672;  // floats per network slot (4609 used; 64-float aligned)
constexpr int kOffW1 = 0, kOffB1 = 320, kOffW2 = 384, kOffB2 = 4480, kOffW3 = 4544, kOffB3 = 4608;
constexpr int kDqnParams = 4609;
constexpr int kDqnBatch = 32;     // agent.py:308
constexpr int kTrans = 10;        // floats per transition: s[4], a, r, ns[4]
constexpr uint32_t kTagSample = 0x5EED0100u;  // + j: replay-buffer sample draws (oracle/philox.py)

struct DqnParams {
  EpisodeParams e;           // simulation inputs, state, records and constants (q unused)
  int t;                     // timestep of this launch
  int n_nets;                // A (per-agent networks, the reference), 1 (shared, config 5) or N (one per role)
  int roles;                 // 0, or N on a role context (p2pmg_dqn_setup_roles): agent a = s N + i uses network i
  float* theta;              // [n_nets][kNetStride] online network
  float* target;             // [n_nets][kNetStride] target network
  float* adam_m;
  float* adam_v;
  float* grad;               // shared: [blocks][kNetStride] train-workgroup partial sums
  float* segs;               // shared: [n_segs][kNetStride] gradient segments of every rank (global order)
  int seg_first;             // global index of this context's first segment
  int n_segs;                // segments over every rank
  int seg_agents;            // agents per segment (a segment is whole scenarios)
  int bps;                   // train workgroups per segment: ceil(seg_agents / apb); roles: per role, ceil(S / apb)
  float* buf;                // [A][cap][kTrans] replay rings
  int32_t* added;            // [A] transitions ever added
  int cap;
  const uint16_t* samples;   // replay mode: [T][A][32] deque indices; null = Philox (Floyd)
  float* smp;                // this step's sampled ring slots, int32 [A][32] (dqn_sample_kernel)
  int fused_sample;          // 1: dqn_act_kernel draws them (training env steps); 0: the sample kernel
  int act_wave;              // shared network: 1 = one wave per agent (dqn_act_kernel) instead of the MFMA act kernel
  int act_agw;               // shared network, MFMA act kernel: agent slots per workgroup (16, or 8 for N <= 8)
  float* rec_loss;           // [T][A] or null
  float* ep_acc;             // [S] running sum_t mean_i r
  // the learner constants of every network when they are equal (always so for one shared network), as f32
  // casts of p2pmg_dqn_config / p2pmg_dqn_set_learning's doubles; tau_c = 1 - tau
  float gamma, tau, tau_c, lr_t, b1c, b2c, adam_eps, clip;
  // per-agent networks whose constants differ: [n_nets] rows {gamma, tau, tau_c, clip}, one 16-B scalar
  // load per train workgroup (its network is uniform); else null: the scalars above
  const float4* hyp;
  const float* penw;         // [A] per-agent comfort weight of the reward (p2pmg_dqn_set_learning)
  const float* lr_net;       // per-agent networks whose Adam step counts differ: [n_nets] step sizes (else null: lr_t)
  float inv_agents;          // shared: 1 / (agents over all ranks); roles: 1 / S (a role's agents)
  int apb;                   // agents per train workgroup
  const float* batch;        // explicit [32][kTrans] batch (p2pmg_dqn_train_batch) or null
  int net;                   // network of the explicit batch
  float* loss_out;           // explicit batch: [1]
  // shared network over segments / ranks: where the post-exchange Adam step stores the new weights,
  // target and moments (the inputs themselves, or the other half of the runtime's double buffer)
  float *theta_out, *target_out, *m_out, *v_out;
  int adam_pending;          // 1: this act launch first applies the previous env step's gathered Adam step
  int adam_tpb;              // post-exchange Adam launch: threads per workgroup (256 default; 64, 128)
  int fold_spt;              // segment fold: runs per thread (0 auto: 4 for runs <= 8, else 1 = the reduce kernel)
};
hipError_t launch_dqn_act(const DqnParams& p, hipStream_t stream);
// launch_dqn_act's branch for one shared network on MFMA tiles, taken when act_shared_mfma(p)
bool act_shared_mfma(const DqnParams& p);
hipError_t launch_dqn_act_shared(const DqnParams& p, hipStream_t stream);
hipError_t launch_dqn_sample(const DqnParams& p, hipStream_t stream);
// every env step's Philox replay draws of the episode p describes, as deque indices [T][A][32] u16
// (the replay-mode sample layout), from the episode-start counts d.added
hipError_t launch_dqn_sample_prepass(const DqnParams& p, uint16_t* out, hipStream_t stream);
hipError_t launch_dqn_train(const DqnParams& p, int blocks, bool shared_partials, hipStream_t stream);
// the role form (p.roles = N networks): workgroup role * p.bps + j chains agents (j apb + ag) N + role,
// ag < apb, of scenarios below S, and writes partial [role][j]; blocks = N * p.bps
hipError_t launch_dqn_train_roles(const DqnParams& p, hipStream_t stream);
int dqn_train_blocks_per_cu();  // train workgroups resident per CU (the build's occupancy target)
// each local segment's sum of its train-workgroup partials -> segs[seg_first + j] (segments = local
// segment count); adam (one segment over every rank): the Adam step on it directly
hipError_t launch_dqn_reduce_adam(const DqnParams& p, int segments, bool adam, hipStream_t stream);
// one launch for the p.roles networks of a role context: role i's p.bps partials in the reduce kernel's
// order, times p.inv_agents, clip, Adam at its own step size (p.lr_net[i], else p.lr_t) and soft update
// at its own row (p.hyp[i], else the scalars), on network i of theta / target / adam_m / adam_v
hipError_t launch_dqn_reduce_adam_roles(const DqnParams& p, hipStream_t stream);
// sum of the n_segs segments in global order, then mean, clip, Adam, soft update
hipError_t launch_dqn_adam_shared(const DqnParams& p, hipStream_t stream);
// segments the act kernel's fused Adam step sums (more take the standalone launch)
constexpr int kActAdamSegs = 8;
// true when launch_dqn_act(p) with p.adam_pending = 1 can apply the pending Adam step itself (the shared
// network's MFMA act kernel, at most kActAdamSegs segments)
bool dqn_act_fuses_adam(const DqnParams& p);
hipError_t launch_dqn_forward(const float* theta, int n, const float* x, float* q, hipStream_t stream);

// the frozen-policy episode (p2pmg_dqn_eval.hip, p2pmg_dqn_run_greedy): T greedy env steps in one launch
struct DqnEvalParams {
  EpisodeParams e;           // as for a greedy dqn_act_kernel launch (mode, rng, codes unused)
  const float* nets;         // [count][kNetStride] the networks the episode reads
  const int32_t* net_of;     // [A] agent -> network of `nets`; null: the context's own arrays (one_net)
  int one_net;               // net_of == null: 1 = every agent reads network 0, 0 = agent a reads network a
  const float* penw;         // [A] per-agent comfort weight of the recorded rewards (as DqnParams::penw)
  float* ep_acc;             // [S] left as the stepwise episode leaves it (= ep_reward)
};
// dqn_greedy_episode_kernel<N>: one workgroup per scenario, any N in 1..kMaxAgents
hipError_t launch_dqn_greedy_episode(const DqnEvalParams& p, hipStream_t stream);

// the DQN policy map (p2pmg_dqn_map.hip): p2pmg_dqn_policy_map, p2pmg_dqn_map_stats, p2pmg_dqn_policy_mark
// and p2pmg_dqn_policy_changes are one pass over `count` networks and the states [g_begin, g_begin +
// g_count) of the grid, with different outputs switched on
constexpr int kDqnMapStats = 8;
struct DqnMapPart {      // one block's results over its states of one network
  float lo, hi, gap;     // min / max over the Q values, min over states of q[greedy] - max(the other two)
  uint32_t n_g[3];       // states per greedy action
  uint32_t n_chg;        // compare: states whose greedy action differs from the snapshot's
  uint32_t pad;
};
struct DqnMapParams {
  const float* theta;    // [count][kNetStride]: the first network of the launch
  int count;
  unsigned bpn;          // blocks per network (dqn_map_blocks): a block never spans networks
  uint32_t n[4];         // grid shape (time, temp, balance, p2p), time slowest
  const float* axes;     // [n0 + n1 + n2 + n3] axis values, time | temp | balance | p2p
  uint32_t g_begin, g_count;  // the states of the launch; the outputs below are indexed from g_begin
  int dword;             // 1: policy / snapshot bytes move as dwords (g_count % 4 == 0, 4-byte aligned bases)
  int remark;            // compare: overwrite the snapshot with the current map in the same pass
  uint8_t* policy;       // [count][g_count] or null
  float* q;              // [count][g_count][3] or null
  uint8_t* snap;         // compare: [count][g_count] snapshot of the same networks, or null
  DqnMapPart* part;      // [count][bpn] block partials (stats, compare) or null
  double* stat_out;      // [count][kDqnMapStats] or null
  long long* chg_out;    // [count] or null
};
unsigned dqn_map_blocks(int count, uint32_t g_count);
// count <= 0 or g_count == 0 launches nothing
hipError_t launch_dqn_map(const DqnMapParams& p, hipStream_t stream);

struct RcParams {
  float inv_ci, inv_cm, inv_ri, inv_re, inv_rvent, c_in, c_m, solar, cop, spm, slot;
};

// tile != 0: the LDS-tile form at any N (else registers for N in {1..8, 16}, tiles for the rest)
hipError_t launch_episode(const EpisodeParams& p, int q_dtype, int tile, hipStream_t stream);
// fast per-agent-table path: step pre-pass ([T][A] {balw, bins}; optionally the Philox code
// words) + episode_fast_kernel (N <= 8, R + 1 <= 4, or <= 2 with a battery, no shared table)
// Where one step pre-pass writes: its buffers and the episode its Philox draws are for.
constexpr int kMaxChain = 64;  // episodes per chained launch (their thresholds travel in the kernarg)
struct PrepOut {
  uint2* pre;      // [T][A]
  uint32_t* ipc;   // [T][A] or null (N != 2)
  uint32_t* words; // [T][W][A] or null (no Philox draws); a chain: n_ep such buffers, words_stride apart
  int episode;
  double eps;      // the epsilon its Philox draws are for
  uint32_t eps_thr;  // its integer threshold (eps_threshold)
  int eps_all;
  // a chain of n_ep > 1 episodes (episode + k): episode k's threshold ep_thr[k], all-explore bit k of
  // ep_all (eps / eps_thr / eps_all unused)
  int n_ep;
  size_t words_stride;
  uint32_t ep_thr[kMaxChain];
  uint64_t ep_all;
  // per-scenario thresholds [n_ep][S] {thr, all} (p2pmg_run_episodes_eps); null: the values above
  const uint2* eps_tab;
};
// w / 2^32 < eps  <=>  w < ceil(eps * 2^32) for every 32-bit w (w / 2^32 and eps * 2^32 are exact in
// f64): thr = that ceiling, clamped to [0, 2^32]; all = (thr == 2^32), when every w explores
inline void eps_threshold(double eps, uint32_t& thr, int& all) {
  double c = __builtin_ceil(eps * 4294967296.0);
  if (!(c > 0.0)) c = 0.0;  // eps <= 0 or NaN: never
  all = c >= 4294967296.0 ? 1 : 0;
  thr = all ? 0xFFFFFFFFu : (uint32_t)c;
}
hipError_t launch_step_prepass(const EpisodeParams& p, const PrepOut& o, hipStream_t stream);
// *out = the hazard distance D of an interleaved chain over the pre-pass words pre [T][A]
// (chain_lag_kernel); T <= kChainLagMaxT (the kernel is O(T^2) per agent)
constexpr int kChainLagMaxT = 512;
hipError_t launch_chain_lag(int T, int A, const uint2* pre, int* out, hipStream_t stream);
// next != null: the launch also runs the step pre-pass of the next episode (episode p.episode + 1,
// same epsilon) into *next, in extra workgroups beside the episode's own
// ev0 / ev1: timing events stamped by the dispatch (hipExtLaunchKernel)
hipError_t launch_episode_fast(const EpisodeParams& p, const uint2* pre, void* recs, int q_dtype, int spw,
                               const PrepOut* next, hipEvent_t ev0, hipEvent_t ev1, hipStream_t stream);
// the slice launchers behind launch_episode_fast (p2pmg_fast.hip, one per P2PMG_FAST_SLICE; N = 1-2 / 3-4 /
// 5-6 / 7-8) and launch_episode (p2pmg_general.hip, one per P2PMG_GENERAL_SLICE)
#define P2PMG_DECL_FAST(name)                                                                                     \
  hipError_t name(const EpisodeParams& p, const uint2* pre, void* recs, int q_dtype, int spw, const PrepOut* next, \
                  hipEvent_t ev0, hipEvent_t ev1, hipStream_t stream);
P2PMG_DECL_FAST(launch_fast_n12)
P2PMG_DECL_FAST(launch_fast_n34)
P2PMG_DECL_FAST(launch_fast_n56)
P2PMG_DECL_FAST(launch_fast_n78)
// N compiled in (registers), then the LDS-tile form for up to nc = 16 / 32 and 64 agents
hipError_t launch_general_n1_4(const EpisodeParams& p, int q_dtype, hipStream_t stream);
hipError_t launch_general_n5_8(const EpisodeParams& p, int q_dtype, hipStream_t stream);
hipError_t launch_general_n16(const EpisodeParams& p, int q_dtype, hipStream_t stream);
hipError_t launch_general_tile16(const EpisodeParams& p, int q_dtype, int nc, hipStream_t stream);
hipError_t launch_general_tile32_64(const EpisodeParams& p, int q_dtype, int nc, hipStream_t stream);
// per-role tables (p.shared_q == 2); nc = 0: the register form
hipError_t launch_role_n1_4(const EpisodeParams& p, int q_dtype, hipStream_t stream);
hipError_t launch_role_n5_8(const EpisodeParams& p, int q_dtype, hipStream_t stream);
hipError_t launch_role_n16_tile16(const EpisodeParams& p, int q_dtype, int nc, hipStream_t stream);
hipError_t launch_role_tile32_64(const EpisodeParams& p, int q_dtype, int nc, hipStream_t stream);
// the policy episode (p2pmg_policy.hip, p2pmg_run_policy): a greedy episode whose actions are bytes of the
// context's policy set, not argmaxes of Q rows
struct PolicyParams {
  EpisodeParams e;        // as for a greedy episode_kernel launch (q, qdelta, codes, eps and the seeds unused)
  const uint8_t* pol;     // [M][n_states] packed policies: action, or 255 = action 0
  const int32_t* pol_of;  // [A] agent -> policy, values in [0, M)
};
// policy_episode_kernel: registers for N in {1..8, 16}, LDS tiles for every other N <= 64 (and for any N
// when tile != 0); one launcher per P2PMG_POLICY_SLICE behind it
hipError_t launch_policy_episode(const PolicyParams& p, int tile, hipStream_t stream);
hipError_t launch_policy_n1_8(const PolicyParams& p, hipStream_t stream);
hipError_t launch_policy_n16_tiles(const PolicyParams& p, int nc, hipStream_t stream);  // nc = 0: registers, N = 16
// RuleAgent community run (R = 0): rule_episode_kernel; hp_on [A] hysteresis state in/out
hipError_t launch_rule_episode(const EpisodeParams& p, float* hp_on, hipStream_t stream);
// shared table, N = 16, R <= 1 (configs[2]): episode_sq16_kernel; records packed like the fast path
hipError_t launch_episode_sq16(const EpisodeParams& p, int q_dtype, hipEvent_t ev0, hipEvent_t ev1, hipStream_t stream);
// its per-upload pre-pass: out = p.sqp's contents from p.env, p.prof, p.max_in
hipError_t launch_sq16_prep(const EpisodeParams& p, uint2* out, hipStream_t stream);
constexpr size_t kFastRecBytes = 32;  // one packed record row per agent-step (FastRec)
constexpr int kFastBatMaxR1 = 2;      // episode_fast_kernel's battery variants: R + 1 <= 2
// which: 0..4 reward, cost, grid, p2p, tin ([T][A] f32); 5 action (u8), 6 index (i32) [T][R+1][A]
hipError_t launch_fast_rec_unpack(int T, int R1, int A, uint32_t tb, const void* recs, int narrow, int which, void* out,
                                  hipStream_t stream);
// p2pmg_episode_summary (p2pmg_summary.hip): the last launch's records reduced over time
constexpr int kSummaryFields = 16;  // P2PMG_SUMMARY_FIELDS
struct SummaryParams {
  int S, N, R, T, A;
  int packed;                 // 1: the records are rec_pack's 32-B rows (fast / sq16 launches), else the plain arrays
  int has_reward;             // 0: the launch recorded no reward (field 1 = 0)
  const float* cost;          // [T][A] plain arrays (packed = 0)
  const float* reward;
  const float* grid;
  const float* p2p;
  const float* tin;
  const uint8_t* action;      // [T][R+1][A]
  const void* rec_pack;       // [T][A] x kFastRecBytes (packed = 1)
  const float2* prof;         // [T][A] {load_w, pv_w}
  const float4* hp_lv;        // [A]
  const float4* thermal;      // [A] {setpoint, lower bound, upper bound, COP}
  double* agent_out;          // [A][kSummaryFields]
  double* scen_out;           // [S][kSummaryFields]
};
// summary_agent_kernel then summary_scenario_kernel (which reads agent_out) on the stream
hipError_t launch_episode_summary(const SummaryParams& p, hipStream_t stream);
// p2pmg_day_profile (p2pmg_dayprof.hip): the last launch's records reduced over scenarios, per (group,
// slot = t % P, agent position).  The launch shape is a DayProfPlan's (p2pmg_dayprof.h), by value here.
struct DayProfParams {
  SummaryParams rec;          // the records (agent_out and scen_out unused)
  int G, P, t0, t1, s0, s1;   // groups, slots, the half-open step and scenario ranges
  const int32_t* labels;      // [S] group of each scenario, -1: left out; null: every scenario in group 0
  int lds, fold, tile_slots, tile_agents, n_tiles, tiles_per_run, slice_steps, n_slices;
  size_t tile_bytes;
  int com_slice_steps, com_n_slices;  // dayprof_community_kernel: steps per workgroup and slices of the range
  unsigned long long* sums;   // [G][P][N][16] int64 sums (two's complement adds)
  uint32_t* ext;              // [G][P][N][8] ordered images of the f32 extrema; dayprof_decode_kernel turns them into f32 in place
  unsigned long long* com_sums;  // [G][P][4]
  uint32_t* com_ext;          // [G][P][2]
};
// init (sums 0, extrema +inf / -inf), dayprof_agent_kernel, dayprof_community_kernel, decode, on the stream;
// an empty step or scenario range launches init and decode only
hipError_t launch_day_profile(const DayProfParams& p, hipStream_t stream);
// the table digests (p2pmg_tables.hip): p2pmg_table_stats, p2pmg_greedy_policy, p2pmg_policy_mark and
// p2pmg_policy_changes are one pass over `count` padded tables with different outputs switched on
constexpr int kTableStats = 8;  // P2PMG_TABLE_STATS
struct TableDigestParams {
  const void* q;         // the first table of the range: [count][n_states][kQPad] f64 | f32
  size_t n_states;
  int n_actions, count;
  unsigned bpt;          // blocks per table (table_digest_blocks): a block never spans tables
  int dword;             // 1: policy / snapshot bytes move as dwords (n_states % 4 == 0, 4-byte aligned bases)
  int remark;            // compare: overwrite the snapshot with the current policy in the same pass
  uint8_t* policy;       // [count][n_states] out, or null
  uint8_t* snap;         // compare: [count][n_states] snapshot of the same tables
  double* stat_part;     // stats: [count][bpt][kTableStats] block partials (null: no stats)
  double* stat_out;      // stats: [count][kTableStats]
  long long* chg_part;   // compare: [count][bpt][2] {changed, newly visited} (null: no compare)
  long long* chg_out;    // compare: [count][2]
};
unsigned table_digest_blocks(int count, size_t n_states);
// stats and compare exclude each other; the fold launch follows the pass on the stream
hipError_t launch_table_digest(const TableDigestParams& p, int q_dtype, hipStream_t stream);
// the sparse table checkpoints (p2pmg_tables.hip): p2pmg_sparse_count, p2pmg_get_q_sparse and
// p2pmg_set_q_sparse.  A row is STORED iff one of its n_actions entries has a non-zero bit pattern.
// Export is a count pass (stored rows per block), an offset pass (one wave per table: the block counts
// become exclusive offsets inside their table, and the table's total) and a scatter pass with the count
// pass's block-to-rows mapping; the order of the output comes from the scan, never from atomics.
struct SparseParams {
  const void* q;         // the first table of the launch: [count][n_states][kQPad] f64 | f32
  size_t n_states;
  int n_actions, count;
  unsigned bpt;          // blocks per table (sparse_blocks): a block never spans tables
  unsigned rpb;          // rows per block, a multiple of the pass's tile: block b owns rows [b * rpb, (b + 1) * rpb) of its table
  uint32_t* blk;         // [count][bpt]: the count pass's stored rows per block, then (offset pass) their exclusive scan per table
  long long* total;      // offset pass: [count] stored rows per table
  const long long* base; // scatter: [count] where each table's rows begin in out_rows / out_vals
  int32_t* out_rows;     // scatter: state indices of the stored rows, table after table, ascending
  void* out_vals;        // scatter: their [n_actions] entries in the host dtype
};
// bpt and rpb for `count` tables of n_states rows; one call of the C ABI uses one mapping for all its passes
void sparse_blocks(int count, size_t n_states, unsigned* bpt, unsigned* rpb);
// count pass then offset pass on the stream; count <= 0 or n_states == 0 launches nothing
hipError_t launch_sparse_count(const SparseParams& p, int q_dtype, hipStream_t stream);
// p.blk as launch_sparse_count left it for these tables (the tables unchanged since)
hipError_t launch_sparse_scatter(const SparseParams& p, int q_dtype, int host_dtype, hipStream_t stream);
// import: one thread per listed row i < total writes one padded row (padding 0) of table t, where
// base[t] <= i < base[t + 1] (base[count] stands for total and is not read); rows within [0, n_states)
// and without duplicates inside a table (the host checked)
struct SparseImportParams {
  void* q;               // the first table of the launch
  size_t n_states;
  int n_actions, count;
  long long total;
  const long long* base; // [count] exclusive scan of the tables' row counts
  const int32_t* rows;   // [total]
  const void* vals;      // [total][n_actions] in the host dtype
};
hipError_t launch_sparse_import(const SparseImportParams& p, int q_dtype, int host_dtype, hipStream_t stream);
hipError_t launch_apply_delta(void* q, long long* qdelta, size_t n, int q_dtype, hipStream_t stream);
hipError_t launch_fold_delta(long long* qdelta, size_t n, hipStream_t stream);
hipError_t launch_battery_seq(int agents, int steps, const double* bal, double* out_bal, double* soc_hist,
                              double* soc, const double* cap, double smin, double smax, double sqrt_eff,
                              hipStream_t stream);
hipError_t launch_philox_codes(const EpisodeParams& p, uint32_t* words, hipStream_t stream);
hipError_t launch_pack_codes(int T, int R1, int A, const uint8_t* in, uint32_t* words, hipStream_t stream);
hipError_t launch_rc_step(int n, const float* t_out, const float* t_in, const float* t_m, const float* hp,
                          float* t_in_new, float* t_m_new, RcParams rc, hipStream_t stream);
// ... with per-element COP (cop null: rc.cop) and the caller's solar term in rc.solar
hipError_t launch_rc_step_ex(int n, const float* t_out, const float* t_in, const float* t_m, const float* hp,
                             const float* cop, float* t_in_new, float* t_m_new, RcParams rc, hipStream_t stream);
hipError_t launch_state_indices(int n, const float* obs, int32_t* idx, int nt, int nT, int nb, int np,
                                hipStream_t stream);
hipError_t launch_t0_philox(int A, float* t_in, float* t_m, uint32_t seed_lo, uint32_t seed_hi, int episode,
                            uint32_t agent_offset, const float4* thermal /* [A], .x = mean */, double sigma,
                            hipStream_t stream);
hipError_t launch_q_pack(int count, size_t n_states, int n_actions, const void* src_ref, void* dst_pad,
                         int q_dtype, int src_dtype, hipStream_t stream);
hipError_t launch_q_unpack(int count, size_t n_states, int n_actions, const void* src_pad, void* dst_ref,
                           int q_dtype, int dst_dtype, hipStream_t stream);
struct QCallParams {
  int n, train, q_dtype;
  const int32_t* agents;
  const float* s_obs;
  const uint8_t* codes;
  const float* rewards;
  const float* ns_obs;
  int32_t* actions;
  double* q_out;
  void* q;
  uint32_t n_states;
  int nt, nT, nb, np;
  const LearnRow* learn;  // [A], indexed by agents[k]
};
hipError_t launch_q_calls(const QCallParams& p, hipStream_t stream);
hipError_t launch_metrics(int S, const float* ep, double* out, hipStream_t stream);
hipError_t launch_table_hash(const void* q, size_t bytes, unsigned long long* out, hipStream_t stream);
hipError_t launch_fdiv_check(int n, const float* a, const float* b, float* out, hipStream_t stream);
hipError_t launch_fdiv64_check(int n, const double* a, const double* b, double* out, hipStream_t stream);
hipError_t launch_prof_pack(int A, int T, const float* load_w, const float* pv_w, float2* prof,
                            hipStream_t stream);

}  // namespace p2pmg
