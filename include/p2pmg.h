/*
 * p2pmg.h — C ABI of libp2pmg.so, the MI355X (gfx950) batched simulator/trainer for the
 * P2PMicrogrid hot path: per-timestep community rollout + tabular Q-learning update,
 * vectorised over S independent community scenarios x N agents.
 *
 * Reference interfaces replaced (paths relative to /root/reference/microgrid):
 *   p2pmg_run_episode(TRAIN)   CommunityMicrogrid.train_episode          community.py:149-182
 *                              (+ _run :67-93, _assign_powers :45-54, _compute_costs :56-65,
 *                               RLAgent.__call__/_divide_power/get_reward agent.py:172-232,
 *                               QAgent._act/train agent.py:271-298, QActor rl.py:89-129,
 *                               HPHeating.step / temperature_simulation heating.py:37-56,138-143)
 *   p2pmg_run_episode(GREEDY)  CommunityMicrogrid.run                    community.py:95-123
 *                              (QAgent.take_decision agent.py:277-289, QActor.greedy_action rl.py:113-117)
 *   p2pmg_set_env              env.setup(dataset) / GridAgent prices     environment.py:26-45, agent.py:59-67
 *   p2pmg_set_profiles         agent load / Prosumer PV streams          agent.py:78-79,100-103, production.py:23-41
 *   p2pmg_set_agent_params     get_community max_in                      community.py:216-227
 *   p2pmg_set_temperatures     HPHeating.__init__/reset T0               heating.py:101-104,145-152
 *   p2pmg_get_q / p2pmg_set_q  QActor.q_table / set_qtable               rl.py:76-81 (layout (20,20,20,20,3))
 *   p2pmg_get_q_sparse / p2pmg_set_q_sparse   QActor.save_to_file / load_from_file, for a batch   rl.py:83-87
 *   p2pmg_rc_step              heating.temperature_simulation (batched)  heating.py:37-56
 *   p2pmg_state_indices        QActor._get_state_indices (batched)       rl.py:89-95
 *   p2pmg_replay_decode        np.random rand()/choice(3) consumption    rl.py:100-111 (legacy MT19937)
 *
 * Conventions: every function returns an int status (P2PMG_OK = 0); no C++ exception crosses
 * the ABI; a per-context error string is available from p2pmg_last_error().  A context owns
 * one device, one HIP stream and every device buffer; host pointers are borrowed for the
 * duration of the call only (copied in/out).  Calls are stream-ordered; p2pmg_sync() (or any
 * p2pmg_get_*) completes outstanding work before host reads.  A context is not thread-safe:
 * use one process per GPU for multi-GPU (scenarios are sharded across ranks).
 */
#ifndef P2PMG_H
#define P2PMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2PMG_ABI_VERSION 9  /* 3: p2pmg_episode_args.next_epsilon; 4: P2PMG_FLAG_NEXT_EPSILON, p2pmg_prepass_stats, per-network Adam steps; 5: p2pmg_collective_ms; 6: DQN gradient segments, p2pmg_dqn_set_exchange, p2pmg_dqn_grad_layout; 7: p2pmg_run_episodes, p2pmg_get_episode_rewards; 8: N up to 64 and any R, P2PMG_FLAG_TILE_KERNEL; 9: p2pmg_set_thermal, p2pmg_get_thermal, p2pmg_rc_step_ex, p2pmg_get_hp_levels (added since without a bump: P2PMG_SHARED_ROLE, p2pmg_episode_summary, p2pmg_chain_lag, p2pmg_set_learning, p2pmg_get_learning, p2pmg_run_episodes_eps, p2pmg_table_stats, p2pmg_greedy_policy, p2pmg_policy_mark, p2pmg_policy_changes, n_actions = 2 table-only contexts, p2pmg_sparse_count, p2pmg_get_q_sparse, p2pmg_set_q_sparse, p2pmg_copy_q, p2pmg_day_profile_shape, p2pmg_day_profile, P2PMG_DQN_POLICY_SET, p2pmg_dqn_set_policy_nets, p2pmg_dqn_get_policy_nets, p2pmg_dqn_run_greedy) */

typedef struct p2pmg_ctx p2pmg_ctx;

/* status codes */
#define P2PMG_OK 0
#define P2PMG_E_INVALID 1     /* bad argument / shape */
#define P2PMG_E_HIP 2         /* HIP runtime error (message in p2pmg_last_error) */
#define P2PMG_E_NOMEM 3       /* device allocation failed */
#define P2PMG_E_STATE 4       /* missing prerequisite (e.g. profiles not set) */
#define P2PMG_E_UNSUPPORTED 5 /* configuration not supported (e.g. N > 64) */

/* Q-table element type: f64 = the reference's np.zeros table (rl.py:73), bit-exact;
 * f32 = throughput mode (TD update in f32, held to 1e-5 relative). */
#define P2PMG_Q_F64 0
#define P2PMG_Q_F32 1

#define P2PMG_MODE_TRAIN 0  /* train_episode: epsilon-greedy + TD update */
#define P2PMG_MODE_GREEDY 1 /* run(): greedy actions, no update, no RNG */
#define P2PMG_MODE_FILL 2   /* DQN init_buffers (community.py:125-147): act + store memory, no training */

#define P2PMG_RNG_REPLAY 0 /* exploration codes supplied by the host (reference stream) */
#define P2PMG_RNG_PHILOX 1 /* counter-keyed Philox4x32-10 on (seed, episode, agent, t, round): one 32-bit
                              word per round, explore if w / 2^32 < epsilon, action w % 3 (round-4
                              layout, oracle/philox.py::decision_draws) */

/* per-step records (bit mask for p2pmg_episode_args.record and p2pmg_get_record) */
#define P2PMG_REC_REWARD 1   /* f32 [T][A] reward (agent.py:225-232) */
#define P2PMG_REC_COST 2     /* f32 [T][A] cost   (community.py:56-65) */
#define P2PMG_REC_GRID 4     /* f32 [T][A] p_grid (community.py:51) */
#define P2PMG_REC_P2P 8      /* f32 [T][A] p_p2p  (community.py:52) */
#define P2PMG_REC_TEMP 16    /* f32 [T][A] T_in before the step's RC update (heating.py:139) */
#define P2PMG_REC_ACTION 32  /* u8  [T][R+1][A] action index (decisions, community.py:88-89) */
#define P2PMG_REC_INDEX 64   /* i32 [T][R+1][A] packed state index it | iT<<8 | ib<<16 | ip<<24 */
#define P2PMG_REC_LOSS 128   /* f32 [T][A] DQN loss of the agent's train step (rl.py:331) */

#define P2PMG_GREEDY 255 /* replay code: no exploration in this (t, round, agent) */

typedef struct p2pmg_config {
  int32_t n_scenarios;      /* S */
  int32_t n_agents;         /* N agents per scenario, 1..64 (a scenario is one 64-lane wave) */
  int32_t rounds;           /* R >= 0: negotiation runs R+1 rounds (community.py:75); R + 1 <= 4096 */
  int32_t horizon;          /* T timesteps per episode */
  int32_t q_dtype;          /* P2PMG_Q_F64 | P2PMG_Q_F32 */
  int32_t n_time_states;    /* 20 (agent.py:258-261) */
  int32_t n_temp_states;    /* 20 */
  int32_t n_balance_states; /* 20 */
  int32_t n_p2p_states;     /* 20 */
  int32_t n_actions;        /* 3; 2: a tabular context that holds tables (set_q, get_q, the table digests) but
                               runs no episode and no p2pmg_q_calls (P2PMG_E_UNSUPPORTED) */
  double alpha;             /* 1e-5 (rl.py:60); per agent: p2pmg_set_learning */
  double gamma;             /* 0.9  (rl.py:59); per agent: p2pmg_set_learning */
  float hp_levels[4];       /* f32(level * max_power) = {0, 1500, 3000} W (agent.py:268, heating.py:124) */
  float setpoint;           /* 21 (community.py:226) */
  float temp_margin;        /* 1  (heating.py:90) */
  float lower_bound;        /* 20 (heating.py:93) */
  float upper_bound;        /* 22 */
  /* RC model, f32 casts of the Python doubles (heating.py:23-56) */
  float inv_ci, inv_cm, inv_ri, inv_re, inv_rvent;
  float one_minus_frad; /* f32(1 - f_rad) */
  float frad;           /* f32(f_rad) */
  float solar_gain;     /* f32(gA * solar_rad) = 0 */
  float hp_cop;         /* f32(3.0) */
  float seconds_per_minute; /* 60 */
  float time_slot;          /* 15 */
  /* costs (community.py:63) and reward (agent.py:230) */
  float minutes_per_hour; /* 60 */
  float kilo;             /* f32(1e-3) */
  float penalty_weight;   /* 10; per agent: p2pmg_set_learning */
  uint64_t seed;          /* Philox key */
  int64_t scenario_offset; /* global index of this context's scenario 0 (multi-GPU sharding):
                              Philox counters use global agent ids so results do not depend
                              on how scenarios are split over ranks */
  int32_t shared_q;        /* 0: one table per agent (the reference, rl.py:73);
                              1: one shared policy table for every agent of every scenario
                              (config 3, build-defined): frozen during an episode, TD deltas summed
                              in int64 fixed point (2^-40) and applied by p2pmg_apply_q_delta;
                              with learner = DQN: one shared Q-network (config 5, data-parallel);
                              P2PMG_SHARED_ROLE (2): one table per role, see below.  Any other non-zero
                              value means 1, as every non-zero value did before 2 was defined */
  int32_t learner;        /* P2PMG_LEARNER_TABULAR (QAgent) | P2PMG_LEARNER_DQN (DQNAgent) */
} p2pmg_config;

#define P2PMG_LEARNER_TABULAR 0
#define P2PMG_LEARNER_DQN 1

/* p2pmg_config.shared_q = P2PMG_SHARED_ROLE: one policy table per ROLE, a role being an agent's
 * position i in its community (the reference's one QActor per agent of ONE community, rl.py:73,
 * agent.py:263, run over S scenarios: days, weather, T0 draws, exploration streams).  The context
 * holds exactly N tables and agent (s, i) of every scenario s reads table i.  Like shared_q = 1 the
 * tables are frozen during an episode; in TRAIN mode agent (s, i)'s update
 * llrint(alpha * ((r + gamma * max Q_i[ns]) - Q_i[s, a]) * 2^40) is summed into role i's int64
 * delta and p2pmg_apply_q_delta does Q_i += delta_i * 2^-40 for every role; GREEDY only reads.  At
 * N = 1 this is shared_q = 1 bit for bit.
 *   - p2pmg_set_q / get_q / zero_q address tables 0..N-1; p2pmg_get_q_delta / set_q_delta move
 *     [N][n_states][n_actions]; apply_q_delta, allreduce_q_delta and table_hash_allgather cover all N.
 *   - the general episode kernel's shared-table form runs it (p2pmg_last_kernel: "...,shared,roles>"),
 *     never episode_fast_kernel or episode_sq16_kernel; p2pmg_set_battery, p2pmg_set_hp_levels and
 *     p2pmg_set_thermal work as with shared_q = 1.
 *   - learner = DQN: p2pmg_create returns P2PMG_E_UNSUPPORTED (p2pmg_last_error(NULL) on the calling
 *     thread says why); a Q-network per role is not built.  (It is built another way: create with
 *     shared_q = 1 and learner = DQN, then p2pmg_dqn_setup_roles instead of p2pmg_dqn_setup.)
 *   - memory: N tables of n_states x 4 elements (5.1 MB each in f64 at 20^4 states) and a delta
 *     buffer of 8 copies x N x 5.1 MB of int64 (2.6 GB at N = 64). */
#define P2PMG_SHARED_ROLE 2

typedef struct p2pmg_episode_args {
  int32_t mode;     /* P2PMG_MODE_TRAIN | P2PMG_MODE_GREEDY */
  int32_t rng;      /* P2PMG_RNG_REPLAY | P2PMG_RNG_PHILOX (TRAIN only) */
  int32_t episode;  /* episode index (Philox counter) */
  int32_t record;   /* P2PMG_REC_* mask */
  double epsilon;   /* exploration rate shared by every agent (QActor._epsilon) */
  int32_t flags;    /* P2PMG_FLAG_* (0 = automatic choice) */
  int32_t scen_per_wave; /* fast kernel: scenarios per 64-lane wave (0 = automatic: 64 / pow2ceil(N)) */
  double reset_sigma;    /* with P2PMG_FLAG_RESET_T0: sigma of the T0 draw */
  double next_epsilon;   /* TRAIN + Philox, fast kernel: epsilon of the NEXT episode, for the
                            speculative pre-pass this launch writes (see P2PMG_FLAG_NEXT_EPSILON;
                            without the flag <= 0 means the same epsilon).  A wrong guess only
                            costs a pre-pass launch next time, never results
                            (p2pmg_prepass_stats counts hits and misses). */
} p2pmg_episode_args;

/* Philox placement: a parallel pre-pass writing per-step code words (latency-bound batches:
 * the episode loop only loads a prefetched word) or inline in the episode kernel (bandwidth-
 * bound batches: no extra HBM traffic).  Automatic: pre-pass below 2^18 agents (the shared-table
 * N = 16 kernel: inline); either flag overrides it on the general and shared-table kernels (a pre-pass launch
 * of the shared-table N = 16 kernel reads p2pmg_last_kernel: "...,philox-prepass...>").  Same stream. */
#define P2PMG_FLAG_PHILOX_PREPASS 1
#define P2PMG_FLAG_PHILOX_INKERNEL 2
/* Kernel choice.  Automatic: the fast per-agent-table kernel (step pre-pass + rounds unrolled at
 * compile time) whenever it applies (N <= 8, R + 1 <= 4, or R + 1 <= 2 with a battery, no shared
 * table, in-range max_in); GENERAL forces the general episode kernel (same results, bit for bit). */
#define P2PMG_FLAG_GENERAL_KERNEL 4
/* End the episode with HPHeating.reset (community.py:181 -> heating.py:145-152): T0 for episode + 1
 * drawn as p2pmg_reset_temperatures_philox(ctx, episode + 1, reset_sigma) would, fused into the
 * episode (no extra launch). */
#define P2PMG_FLAG_RESET_T0 8
/* next_epsilon holds the caller's guess as given, 0.0 included (DQN-style schedules decay to 0).
 * Without this flag only a positive next_epsilon is a guess; anything else means "same epsilon". */
#define P2PMG_FLAG_NEXT_EPSILON 16
/* The general kernel's LDS-tile form (the scenario's P in two LDS tiles, any N <= 64; the form every
 * N outside {1..8, 16} runs) at any N: the cross-check of the register form, same results bit for bit. */
#define P2PMG_FLAG_TILE_KERNEL 32

/* version / defaults */
int p2pmg_abi_version(void);
int p2pmg_device_count(int* count); /* visible HIP devices (0 on a host without GPUs) */
int p2pmg_config_default(p2pmg_config* cfg); /* the reference constants, S = 1, N = 2, R = 1, T = 96 */

/* lifetime */
int p2pmg_create(const p2pmg_config* cfg, int device, p2pmg_ctx** out);
int p2pmg_destroy(p2pmg_ctx* ctx);
const char* p2pmg_last_error(const p2pmg_ctx* ctx);
int p2pmg_sync(p2pmg_ctx* ctx);
int p2pmg_device_info(p2pmg_ctx* ctx, char* name, size_t name_len, size_t* total_mem);
/* which kernel the last episode launch ran, e.g. "episode_fast_kernel<2,f64,R1=2,train>" */
const char* p2pmg_last_kernel(const p2pmg_ctx* ctx);

/* inputs (host arrays, copied to HBM) */
int p2pmg_set_env(p2pmg_ctx* ctx, int n_env, const float* time, const float* t_out,
                  const float* price_buy, const float* price_inj, const float* price_p2p);
                  /* each [n_env][T], n_env in {1, S} */
int p2pmg_set_profiles(p2pmg_ctx* ctx, const float* load_w, const float* pv_w); /* [A][T], A = S*N */
int p2pmg_set_agent_params(p2pmg_ctx* ctx, const float* max_in);              /* [A] */
int p2pmg_set_temperatures(p2pmg_ctx* ctx, const float* t_in, const float* t_m); /* [A] */
int p2pmg_get_temperatures(p2pmg_ctx* ctx, float* t_in, float* t_m);
int p2pmg_reset_temperatures_philox(p2pmg_ctx* ctx, int episode, double sigma); /* T0 ~ N(setpoint of the agent, sigma) */
int p2pmg_set_replay_codes(p2pmg_ctx* ctx, const uint8_t* codes);            /* [T][R+1][A] */

/* Q-tables in the reference layout (n_time, n_temp, n_bal, n_p2p, n_actions) per agent */
int p2pmg_zero_q(p2pmg_ctx* ctx);
int p2pmg_set_q(p2pmg_ctx* ctx, int first_agent, int count, const void* host, int host_dtype);
int p2pmg_get_q(p2pmg_ctx* ctx, int first_agent, int count, void* host, int host_dtype);

/* Table digests: what a sweep asks of its learned tables, computed ON THE DEVICE by one streaming pass
 * over the tables where they lie, so that 8 doubles per table, one byte per state or two counts per
 * table reach the host instead of the tables (5.1 MB each in f64 at 20^4 states).
 *
 * All four calls address tables 0 .. n_tables-1 as p2pmg_get_q does (A per-agent tables, 1 shared table
 * or N role tables), are stream-ordered after earlier launches and synchronise before returning.  They
 * read the tables as they are at the call: the pending int64 delta of a shared or role context is NOT
 * applied (p2pmg_apply_q_delta first, if wanted).  DQN context: P2PMG_E_STATE (no Q-table).
 * first < 0, count < 0, first + count > n_tables or a NULL output (where not marked optional):
 * P2PMG_E_INVALID.  count == 0: P2PMG_OK, nothing written.
 *
 * Definitions.  A table has n_states ROWS, one per state, in the reference's (time, temp, balance, p2p)
 * order, time slowest: the order of p2pmg_get_q.  A row's ENTRIES are its n_actions Q-values (the first
 * n_actions of the 4 stored; the padding is never read into any result).
 *   visited        a row is visited iff any entry != 0.0.  -0.0 == 0.0, so a row of +-0.0 only is not.
 *   greedy action  g = 0; for k = 1 .. n_actions-1 in order: if entry[k] > entry[g] then g = k.  The
 *                  FIRST maximum: the strict-> scan of the episode kernels (QActor.greedy_action,
 *                  rl.py:113-117).  An unvisited row's greedy action is therefore 0.
 *   Tables are assumed NaN-free; with NaN entries the results are whatever these comparisons give.
 * Every result is a count, a minimum or a maximum: none depends on any order of evaluation, and "equal"
 * below means bit for bit.  f32 tables widen to f64 exactly.
 *
 * p2pmg_table_stats: P2PMG_TABLE_STATS f64 values per table, stats[k][.] for table first + k:
 *    0 visited     number of visited rows
 *    1 q_min       minimum over all n_states x n_actions entries
 *    2 q_max       maximum over the same entries
 *    3 abs_max     maximum of |entry| over the same entries (= max(-q_min, q_max)): the normaliser of the
 *                  reference's plots, np.abs(q_table).max() (data_analysis.py plot_q_values_com / _no_com)
 *    4..7 greedy[a]  number of VISITED rows whose greedy action is a; 0 for a >= n_actions
 *                  (fields 4..7 sum to field 0)
 * Counts are exact in f64.  A zero value of fields 1-3 is returned as +0.0, whatever the signs of the
 * zeros in the table. */
#define P2PMG_TABLE_STATS 8
int p2pmg_table_stats(p2pmg_ctx* ctx, int first, int count, double* stats /* [count][P2PMG_TABLE_STATS] */);
/* The packed greedy policy: one byte per row, the row's greedy action (0 .. n_actions-1) if the row is
 * visited, else P2PMG_POLICY_UNVISITED.  1/32 of an f64 table (1/16 of an f32 one). */
#define P2PMG_POLICY_UNVISITED 255
int p2pmg_greedy_policy(p2pmg_ctx* ctx, int first, int count, uint8_t* policy /* [count][n_states] */);
/* Policy churn.  p2pmg_policy_mark stores the packed policy (as p2pmg_greedy_policy defines it) of EVERY
 * table in a snapshot [n_tables][n_states] u8 that the context owns on the device; it is allocated by
 * the first call (P2PMG_E_NOMEM if that fails, and there is then no snapshot).  p2pmg_set_q and
 * p2pmg_zero_q do not touch the snapshot.
 * p2pmg_policy_changes compares the tables as they are now with the snapshot, per table first + k:
 *    changed[k]        number of rows whose greedy action differs from the snapshot's, where a snapshot
 *                      byte 255 stands for action 0 (an unvisited row's greedy action) and the current
 *                      side is the greedy action whether or not the row is visited
 *    newly_visited[k]  number of rows whose snapshot byte is 255 and that are visited now
 *                      (newly_visited may be NULL)
 * remark != 0: the same pass overwrites the snapshot of tables [first, first + count), and of no other,
 * with the current packed policy; each table is read once.  Before the first p2pmg_policy_mark:
 * P2PMG_E_STATE. */
int p2pmg_policy_mark(p2pmg_ctx* ctx);
int p2pmg_policy_changes(p2pmg_ctx* ctx, int first, int count, int64_t* changed /* [count] */,
                         int64_t* newly_visited /* [count] or NULL */, int remark);

/* Sparse table checkpoints: the tables taken home and brought back without their zeros.  p2pmg_get_q and
 * p2pmg_set_q move count x n_states x n_actions elements whatever the tables hold; a table that training
 * has touched in a few hundred or thousand of its 160 000 rows travels here as those rows only, compacted
 * ON THE DEVICE by a streaming pass like the digests', and comes back by a scatter.
 *
 * All four calls address tables as p2pmg_get_q does (A per-agent tables, 1 shared table or N role
 * tables), are stream-ordered after earlier launches and synchronise before returning.  They do not apply
 * the pending int64 delta of a shared or role context and do not touch the policy snapshot.  DQN context:
 * P2PMG_E_STATE.  first < 0, count < 0, first + count > n_tables or a NULL required pointer:
 * P2PMG_E_INVALID.  count == 0: P2PMG_OK, nothing read or written.  n_states > 2^31 - 1 (row indices are
 * int32): P2PMG_E_UNSUPPORTED.
 *
 * Definitions, bit for bit.
 *   stored row   a row is stored iff at least one of its n_actions entries has a NON-ZERO BIT PATTERN.  An
 *                entry of -0.0 therefore counts.  The padding columns never count and are never exported.
 *                This is a superset of the digests' "visited" (any entry != 0.0): the two differ exactly
 *                in the rows whose entries are all zeros with at least one -0.0, which are stored and not
 *                visited.  NaN entries are non-zero bits like any other.
 *   sparse form  of tables [first, first + count), three arrays:
 *                  n_rows[count]            int64, the stored rows of each table
 *                  rows[total]              int32, the state indices (row numbers in p2pmg_get_q's order) of
 *                                           the stored rows, table after table, STRICTLY ASCENDING inside
 *                                           each table; total = sum of n_rows
 *                  values[total][n_actions] host dtype, the entries of those rows in the same order
 *                Conversion between the table's dtype and the host dtype is p2pmg_get_q's / p2pmg_set_q's
 *                (a C cast per entry; same dtype: the bits).  Storedness is always decided on the TABLE's
 *                own bits, before any conversion.  The order is part of the definition: the same tables
 *                give the same bytes whatever the launch shape (positions come from an ordered scan of
 *                counts, never from atomics).
 *   round trip   zero the tables, then import the sparse form taken in the table's own dtype: the
 *                n_actions entries of every row are reproduced bit for bit (an all-+0.0 row is simply
 *                absent).
 *
 * Staging.  Neither direction allocates by n_states: the device staging of a call holds one RUN of whole
 * tables whose stored rows fit P2PMG_SPARSE_STAGE_BYTES, at 4 + n_actions * sizeof(host dtype) bytes a
 * row; a run always holds at least one table, so a single table with more stored rows than that is a run
 * of its own and the staging grows to it.  The context keeps the staging for the next call.
 *
 * p2pmg_sparse_count: one counting pass; n_rows[k] = stored rows of table first + k.
 * p2pmg_get_q_sparse: counts, then exports.  It ALWAYS writes n_rows.  If the total exceeds `capacity` (the
 *   rows that `rows` and `values` have room for) it returns P2PMG_E_INVALID with `rows` and `values`
 *   untouched: size the buffers from n_rows (or from p2pmg_sparse_count) and call again.  rows and values
 *   are required only when the total is not 0.
 * p2pmg_set_q_sparse: the host checks the whole form BEFORE anything is uploaded or zeroed: every
 *   n_rows[k] in [0, n_states], every index in [0, n_states), indices strictly ascending inside each table
 *   (so no duplicates, and the scatter has no write race).  A violation returns P2PMG_E_INVALID and the
 *   tables are unchanged.  zero_first != 0 zeroes tables [first, first + count) first, padding included
 *   (not the pending delta: that is p2pmg_zero_q's); zero_first == 0 overlays: only the listed rows are
 *   overwritten.  The padding of a written row is 0.  rows and values are required only when the total
 *   is not 0.
 * p2pmg_copy_q: tables [dst_first, dst_first + dst_count) become bit copies of table src, padding
 *   included, device to device (warm-starting many communities from one).  src outside 0 .. n_tables-1 or
 *   inside the destination range: P2PMG_E_INVALID. */
#define P2PMG_SPARSE_STAGE_BYTES (8u << 20)
int p2pmg_sparse_count(p2pmg_ctx* ctx, int first, int count, int64_t* n_rows /* [count] */);
int p2pmg_get_q_sparse(p2pmg_ctx* ctx, int first, int count, int64_t capacity, int64_t* n_rows /* [count] */,
                       int32_t* rows /* [capacity] */, void* values /* [capacity][n_actions] */, int host_dtype);
int p2pmg_set_q_sparse(p2pmg_ctx* ctx, int first, int count, const int64_t* n_rows /* [count] */,
                       const int32_t* rows /* [total] */, const void* values /* [total][n_actions] */, int host_dtype,
                       int zero_first);
int p2pmg_copy_q(p2pmg_ctx* ctx, int src, int dst_first, int dst_count);

/* the hot path */
int p2pmg_run_episode(p2pmg_ctx* ctx, const p2pmg_episode_args* args);
/* n consecutive episodes: the loop body of CommunityMicrogrid's training loop (community.py:279-286,
 * train_episode x n), episode args->episode + k at epsilons[k], every other field of args as in
 * p2pmg_run_episode.  Training with Philox draws, where the fast kernel applies, runs as chained
 * launches (up to 64 episodes per launch, every wave running its episodes back to back); anything
 * else as n launches.  Results, tables, T0 resets and the records left behind (the last episode's)
 * are those of the n p2pmg_run_episode calls, bit for bit.  next_n / next_epsilons: the caller's
 * guess of the NEXT call's epsilons for the speculative pre-pass (as next_epsilon; next_n = 0: the
 * same as this call's last).  p2pmg_get_episode_reward returns the last episode's reward. */
int p2pmg_run_episodes(p2pmg_ctx* ctx, const p2pmg_episode_args* args, int n, const double* epsilons, int next_n,
                       const double* next_epsilons);
/* p2pmg_run_episodes with one epsilon per SCENARIO: scenario s explores at eps[k][s] in episode
 * args->episode + k (eps is [n][S]); args->epsilon is ignored.  The agents of one community share
 * their decay schedule (community.py:285-286; QActor.decay rl.py:83-87), so a batch of communities at
 * different points of different schedules (a sweep) is one call.  P2PMG_MODE_TRAIN with
 * P2PMG_RNG_PHILOX only, anything else P2PMG_E_INVALID (replay codes already carry each agent's own
 * epsilon); every value finite and in [0, 1], else P2PMG_E_INVALID.  The rule is p2pmg_run_episode's,
 * per scenario: word w explores iff w < ceil(eps 2^32) (eps = 1: every word), and below eps = 2^-8 the
 * action comes from its own Philox block.  The thresholds travel in a device table [n][S] that the
 * step pre-pass, the code-word pre-pass and the general kernel's in-kernel draws read; chained and
 * interleaved launches are planned as for p2pmg_run_episodes, and calls of more than 64 episodes split
 * the same way.  With every row one repeated value the call equals p2pmg_run_episodes at that
 * schedule, bit for bit.  The call does not speculate the next call's pre-pass and leaves no
 * speculative slot valid, so the next plain launch computes its own.  A shared-table N = 16 context
 * runs the general kernel's shared-table form for this call, not episode_sq16_kernel.
 * p2pmg_get_episode_rewards works as after p2pmg_run_episodes.  DQN contexts: P2PMG_E_UNSUPPORTED. */
int p2pmg_run_episodes_eps(p2pmg_ctx* ctx, const p2pmg_episode_args* args, int n, const double* eps /* [n][S] */);
/* [n][S] episode rewards (community.py:179) of the first n episodes of the last p2pmg_run_episodes or
 * p2pmg_run_episodes_eps call */
int p2pmg_get_episode_rewards(p2pmg_ctx* ctx, int n, float* host);
/* one P2PMG_REC_* bit of the LAST episode launch; P2PMG_E_STATE if that launch did not record it */
int p2pmg_get_record(p2pmg_ctx* ctx, int which, void* host);
/* Episode summary: the records of the LAST episode launch reduced over time ON THE DEVICE to
 * P2PMG_SUMMARY_FIELDS f64 values per agent and per scenario (the totals behind the reference's
 * figures: daily cost per agent, self-consumption, grid load; data_analysis.py:188-209, 324-420,
 * 775-846), so that only [A][16] + [S][16] doubles are copied to the host instead of the per-step
 * records.  A post-pass over what the launch wrote: that launch must have recorded every bit of
 * P2PMG_SUMMARY_RECORDS (else P2PMG_E_STATE, p2pmg_last_error names what is missing; the fast and
 * sq16 kernels' narrow reward + cost form and "no episode yet" included).  P2PMG_REC_REWARD is
 * optional: without it field 1 is 0 (rule episodes never record it).  After p2pmg_run_episodes it
 * describes the last episode of the chain, whose records remain.  load and pv are read from the
 * context's profile buffer, hp levels and comfort bounds from the per-agent arrays, as they are at
 * the call.  Stream-ordered, synchronises before returning (like p2pmg_get_record).
 *
 * Per agent a = s N + i, every field accumulated in f64 SEQUENTIALLY over t = 0..T-1 from +0.0, each
 * term formed in f32 as written and then widened (max(x, 0) is x > 0 ? x : +0); this order is the
 * definition:
 *    0 cost              cost[t,a]                                         (currency of the prices)
 *    1 reward            reward[t,a]
 *    2 grid_import       max(grid[t,a], 0)                                 W-steps
 *    3 grid_export       max(-grid[t,a], 0)
 *    4 p2p_import        max(p2p[t,a], 0)
 *    5 p2p_export        max(-p2p[t,a], 0)
 *    6 hp                hp_levels[a][action[t,R,a]]: the final round's action, the power the RC step used
 *    7 load              load_w[a][t]
 *    8 pv                pv_w[a][t]
 *    9 self_consumption  power = grid + p2p (one f32 add, what run() returns); power < 0 ? pv + power : pv
 *                        (data_analysis.py:195)
 *   10 discomfort_deg    d = max(max(0, lower_a - T_in), max(0, T_in - upper_a)), T_in before the step's
 *                        RC update, the agent's own bounds (p2pmg_set_thermal)
 *   11 discomfort_steps  d > 0 ? 1 : 0
 *   12 t_in_min          running minimum of T_in (not a sum)
 *   13 t_in_max          running maximum of T_in
 *   14 peak_import       running maximum of max(grid, 0), W
 *   15 peak_export       running maximum of max(-grid, 0)
 * The comfort penalty of the reward (agent.py:225-232) summed over the episode is
 * penalty_weight * (field 10 + field 11).
 * Per scenario s: fields 0-11 are the sequential f64 sum over i = 0..N-1 of the agents' values, 12 the
 * minimum and 13 the maximum over the agents' 12 and 13, 14 and 15 the COMMUNITY's peaks
 * max_t max(G_t, 0) and max_t max(-G_t, 0), G_t the sequential f32 sum over i of grid[t, s N + i] from
 * +0.0: the net load the community puts on the grid (plot_grid_load). */
#define P2PMG_SUMMARY_FIELDS 16
#define P2PMG_SUMMARY_RECORDS (P2PMG_REC_COST | P2PMG_REC_GRID | P2PMG_REC_P2P | P2PMG_REC_TEMP | P2PMG_REC_ACTION)
/* per_agent [A][16] f64 and/or per_scenario [S][16] f64 (either may be NULL, not both) */
int p2pmg_episode_summary(p2pmg_ctx* ctx, double* per_agent, double* per_scenario);
/* Day profile: the records of the LAST episode launch reduced over SCENARIOS ON THE DEVICE, where
 * p2pmg_episode_summary reduces them over time: one row per (group g, slot p = t % P, agent position i) and
 * one per (g, p) for the community's net grid load (the means and bands behind the reference's make_day_plot,
 * make_baseline_day_plot, make_decisions_comparison_plot and plot_grid_load, data_analysis.py), so that only
 * [G][P][N] rows are copied to the host instead of the per-step records.  A post-pass over what the launch
 * wrote, with p2pmg_episode_summary's requirements: every bit of P2PMG_SUMMARY_RECORDS (else P2PMG_E_STATE,
 * p2pmg_last_error names what is missing; the narrow reward + cost form and "no episode has run" included),
 * P2PMG_REC_REWARD optional (without it column 2 is 0).  After p2pmg_run_episodes it describes the last
 * episode of the chain.  load and pv are read from the context's profile buffer, hp levels and comfort
 * bounds from the per-agent arrays, as they are at the call.  Tabular, rule and DQN contexts alike.
 * Stream-ordered, synchronises before returning.
 *
 * A sample is a pair (s, t) with s in the scenario range, groups[s] = g >= 0, t in the step range and
 * t % P = p; for each agent i (a = s N + i) it adds to row [g][p][i], with fix(x, k) = rint(f64(x) * 2^k) to
 * nearest even as int64 (f32 * 2^k is exact in f64: one rounding) and max(x, 0) = x > 0 ? x : +0:
 *   sums [G][P][N][16] int64
 *      0 samples            1
 *      1 cost               fix(cost[t,a], 28)
 *      2 reward             fix(reward[t,a], 28)              (0 when not recorded)
 *      3 grid_import        fix(max(grid[t,a], 0), 16)        W
 *      4 grid_export        fix(max(-grid[t,a], 0), 16)
 *      5 p2p_import         fix(max(p2p[t,a], 0), 16)
 *      6 p2p_export         fix(max(-p2p[t,a], 0), 16)
 *      7 hp                 fix(hp_levels[a][action[t,R,a]], 16): the final round's action
 *      8 load               fix(load_w[a][t], 16)
 *      9 pv                 fix(pv_w[a][t], 16)
 *     10 t_in               fix(T_in[t,a], 24)                degC
 *     11 discomfort_deg     fix(d, 24), d = max(max(0, lower_a - T_in), max(0, T_in - upper_a)) as field 10 of
 *                           p2pmg_episode_summary
 *     12 discomfort_steps   d > 0
 *     13 action1            action[t,R,a] == 1
 *     14 action2            action[t,R,a] == 2
 *     15 importing          grid[t,a] > 0
 *   extrema [G][P][N][8] f32: min, max of T_in, grid, p2p, cost over the row's samples, zeros as +0.0; a row
 *      without samples holds +inf, -inf
 *   com_sums [G][P][4] int64: samples; fix(max(G_t, 0), 16); fix(max(-G_t, 0), 16); G_t > 0, with G_t the
 *      sequential f32 sum over i = 0..N-1 of grid[t, s N + i] from +0.0 (plot_grid_load); this order is part of
 *      the definition
 *   com_extrema [G][P][2] f32: min, max of G_t (zeros as +0.0; +inf, -inf without samples)
 * Every entry is an exact integer or an extremum, so none depends on the order of the reduction, and the
 * arrays of disjoint scenario sets merge exactly (integers add, minima and maxima combine).  Records are
 * finite.  With magnitudes below 2^23 W, 2^15 degC and 2^11 money and at most 2^24 samples per row no sum
 * reaches 2^63: a call whose largest group times ceil(steps / P) exceeds 2^24 is P2PMG_E_INVALID (split by
 * scenario range and merge the parts).  A bad period, range or label is P2PMG_E_INVALID with a message.
 * The LDS a workgroup may use for its tile of rows is P2PMG_DAYPROF_TILE_BYTES (environment, read at every
 * call; default 32768, at most 65536); when one slot of every group does not fit, the pass adds to the
 * output with global atomics directly. */
typedef struct p2pmg_day_profile_args {
  int32_t period;                  /* P slots, slot(t) = t % P; 0: T (no folding); else 1..T */
  int32_t step_first, step_count;  /* half-open range of steps; count < 0: to T; 0 is valid (empty rows) */
  int32_t scen_first, scen_count;  /* the same over scenarios */
  int32_t n_groups;                /* G; 0: max label + 1, at least 1 */
  const int32_t* groups;           /* host [S], labels in [-1, G), -1 leaves a scenario out; NULL: all 0 */
} p2pmg_day_profile_args;
/* G and P of a call with these arguments (either may be NULL); the arguments are checked as by the call */
int p2pmg_day_profile_shape(p2pmg_ctx* ctx, const p2pmg_day_profile_args* args, int32_t* G, int32_t* P);
/* any output may be NULL, not all four */
int p2pmg_day_profile(p2pmg_ctx* ctx, const p2pmg_day_profile_args* args, int64_t* sums /* [G][P][N][16] */,
                      float* extrema /* [G][P][N][8] */, int64_t* com_sums /* [G][P][4] */,
                      float* com_extrema /* [G][P][2] */);
/* fast path: episode launches whose step pre-pass the previous launch had already produced (hits)
 * and launches that had to run it themselves (misses), since the context was created */
int p2pmg_prepass_stats(p2pmg_ctx* ctx, int64_t* hits, int64_t* misses);
/* RuleAgent community run (get_rule_based_community community.py:237-238 -> run() community.py:95-123,
 * RuleAgent agent.py:106-136): hysteresis heat pump at the heat pump's max power (level 2 of
 * p2pmg_set_hp_levels), no policy, R = 0.  Records: COST, GRID, P2P, TEMP, ACTION (0 off / 2 on). */
int p2pmg_run_rule_episode(p2pmg_ctx* ctx, int record);
/* HeatPump.power of each RuleAgent (0 or 1; persists across runs like the reference's): [A] */
int p2pmg_set_hp_state(p2pmg_ctx* ctx, const float* on);
int p2pmg_get_hp_state(p2pmg_ctx* ctx, float* on);
int p2pmg_get_episode_reward(p2pmg_ctx* ctx, float* host);     /* [S]: sum_t mean_i r (community.py:179) */
int p2pmg_last_kernel_ms(p2pmg_ctx* ctx, float* ms);           /* HIP-event time of the last episode kernel */
/* HIP-event durations (ms) of the episode kernels launched since the last reset, oldest first
 * (ring of the last 4096 launches, on the context's stream); *count = entries written. */
int p2pmg_kernel_times(p2pmg_ctx* ctx, float* ms, int max, int* count);
int p2pmg_reset_kernel_times(p2pmg_ctx* ctx);
/* Sum of the HIP-event durations (ms) of the data-path collectives (shared-table delta
 * all-reduce, DQN gradient-segment all-gather; not the episode metrics) enqueued since
 * p2pmg_reset_kernel_times; *count = collectives summed (all of them: older ring slots are folded
 * into a running total before reuse).  No reference counterpart (the reference is one process);
 * the multi-GPU bench line reports it. */
int p2pmg_collective_ms(p2pmg_ctx* ctx, double* total_ms, int* count);
/* Stamp the episode kernel's timing events on every period-th episode launch only (default 1 =
 * every launch; the counter restarts here and at p2pmg_reset_kernel_times, so the next launch is
 * timed).  Timing-only: results do not depend on it. */
int p2pmg_set_timing_period(p2pmg_ctx* ctx, int period);

/* batched primitives (device) for unit parity against the reference functions */
int p2pmg_rc_step(p2pmg_ctx* ctx, int n, const float* t_out, const float* t_in, const float* t_m,
                  const float* hp, float* t_in_new, float* t_m_new);
/* p2pmg_rc_step with per-element COP (NULL = config) and solar_gain = f32(gA * solar_rad) */
int p2pmg_rc_step_ex(p2pmg_ctx* ctx, int n, const float* t_out, const float* t_in, const float* t_m,
                     const float* hp, const float* cop, float solar_gain, float* t_in_new, float* t_m_new);
int p2pmg_state_indices(p2pmg_ctx* ctx, int n, const float* obs /* [n][4] */, int32_t* idx /* [n][4] */);
/* The kernels' fast divisions next to the IEEE operator, for the division fuzz test (the quotients
 * the reference takes in agent.py:175,193,203, community.py:63 and storage.py:58,61,64).
 * f32: out [n][4] = {fdiv_b, the divide-power form, the packed sq16 form, IEEE a / b};
 * f64: out [n][3] = {fdiv64, qcore64 under the battery rule's guard, IEEE a / b}. */
int p2pmg_fdiv_check(p2pmg_ctx* ctx, int n, const float* a, const float* b, float* out);
int p2pmg_fdiv64_check(p2pmg_ctx* ctx, int n, const double* a, const double* b, double* out);

/* heterogeneous agents and storage (configs 3-4) */
int p2pmg_set_hp_levels(p2pmg_ctx* ctx, const float* levels /* [A][3] W per action */);
int p2pmg_get_hp_levels(p2pmg_ctx* ctx, float* levels /* [A][3] */);
/* per-agent comfort and heat pump (HPHeating / HeatPump, heating.py:92-130): [A][4] =
 * {setpoint, lower_bound, upper_bound, cop}; NULL restores the config's values.  The bounds are the
 * caller's: the reference forms setpoint -/+ 1.0 in f64 and casts to f32 afterwards, which differs
 * from an f32 subtraction for a setpoint such as 21.3.  Non-finite values and lower > upper:
 * P2PMG_E_INVALID.  Every episode kernel reads these (rule, tabular, DQN), as do the T0 draws; a
 * shared-table N = 16 context with values set here runs the general kernel's shared-table form
 * instead of episode_sq16_kernel (same results, bit for bit) until NULL restores the config's. */
int p2pmg_set_thermal(p2pmg_ctx* ctx, const float* params);
int p2pmg_get_thermal(p2pmg_ctx* ctx, float* params);
/* per-agent learner constants: each QActor's own alpha and gamma (rl.py:58-71, used in QActor.train
 * rl.py:125-128) and the comfort weight of the agent's reward (agent.py:225-232).  Each argument is [A],
 * or NULL for the config's value of that field; all three NULL restores the config's values.  Values
 * must be finite with 0 <= alpha <= 1, 0 <= gamma <= 1 and penalty_weight >= 0, else P2PMG_E_INVALID,
 * and a rejected call changes nothing.  Every tabular episode kernel and p2pmg_q_calls read these
 * (f32 tables cast alpha and gamma to f32 in the kernel, as before); p2pmg_create fills them from the
 * config, so a context that never calls this computes the same bits as with the broadcast constants.
 * A shared-table N = 16 context with values set here runs the general kernel's shared-table form
 * instead of episode_sq16_kernel (same results, bit for bit) until the all-NULL call restores the
 * config's.  DQN contexts: P2PMG_E_UNSUPPORTED (their call is p2pmg_dqn_set_learning). */
int p2pmg_set_learning(p2pmg_ctx* ctx, const double* alpha, const double* gamma, const float* penalty_weight);
/* the values in use, each [A]; any output may be NULL */
int p2pmg_get_learning(p2pmg_ctx* ctx, double* alpha, double* gamma, float* penalty_weight);
/* Battery per agent (storage.py:36-76, rule agent.py:138-153, f64): capacity [A] in J (0 = none;
 * NULL disables storage), SoC bounds, round-trip efficiency, initial SoC [A] (NULL = 0.5). */
int p2pmg_set_battery(p2pmg_ctx* ctx, const double* capacity, double min_soc, double max_soc,
                      double efficiency, const double* soc0);
int p2pmg_get_soc(p2pmg_ctx* ctx, double* soc);
int p2pmg_battery_seq(p2pmg_ctx* ctx, int agents, int steps, const double* balance /* [agents][steps] */,
                      double* out_balance, double* soc_hist, double* soc /* [agents] in/out */,
                      const double* capacity, double min_soc, double max_soc, double efficiency);

/* shared policy table (config.shared_q = 1), or the N per-role tables (P2PMG_SHARED_ROLE) */
int p2pmg_apply_q_delta(p2pmg_ctx* ctx);            /* Q += delta * 2^-40; delta = 0 */
int p2pmg_get_q_delta(p2pmg_ctx* ctx, int64_t* host); /* [n_states][n_actions] fixed point ([N][...] per role) */
int p2pmg_set_q_delta(p2pmg_ctx* ctx, const int64_t* host); /* e.g. after a host-side (gloo) sum */

/* multi-GPU exchange of the shared-table deltas over RCCL (xGMI), loaded at run time */
int p2pmg_comm_unique_id(uint8_t id[128]);
int p2pmg_comm_init(p2pmg_ctx* ctx, const uint8_t id[128], int rank, int nranks);
int p2pmg_allreduce_q_delta(p2pmg_ctx* ctx);        /* int64 sum over ranks, in place, on the stream */
int p2pmg_comm_destroy(p2pmg_ctx* ctx);
/* ranks of the context's communicator (ncclCommCount; 1 without one) */
int p2pmg_comm_nranks(p2pmg_ctx* ctx, int* nranks);
/* episode metrics of the last episode over every rank: out = {sum over scenarios of the episode
 * reward (community.py:179), number of scenarios}; the local sum in f64 on the device, then an
 * RCCL all-reduce (sum) when a communicator exists.  Synchronises. */
int p2pmg_allreduce_metrics(p2pmg_ctx* ctx, double* out /* [2] */);
/* 64-bit fingerprint of the context's Q-table bits, all-gathered over the communicator:
 * out[nranks] in rank order (out[0] alone without one); replicas of a shared table agree. */
int p2pmg_table_hash_allgather(p2pmg_ctx* ctx, uint64_t* out);

/* Standalone QActor calls (rl.py:89-129) on the context's per-agent tables, applied IN ORDER
 * by one device thread: for entry k, s = indices(s_obs[k]); a = codes[k] == P2PMG_GREEDY ?
 * argmax Q[agent[k], s] (first max) : codes[k]; q_out[k] = greedy ? Q[s, a] : 0 (select_action /
 * greedy_action); if train, Q[s, a] += alpha * ((reward[k] + gamma * max Q[ns]) - Q[s, a])
 * (QActor.train), alpha and gamma being agent[k]'s own (p2pmg_set_learning).  ns_obs/rewards may be
 * NULL when train == 0. */
int p2pmg_q_calls(p2pmg_ctx* ctx, int n, const int32_t* agents, const float* s_obs /* [n][4] */,
                  const uint8_t* codes, const float* rewards, const float* ns_obs /* [n][4] */,
                  int train, int32_t* actions_out, double* q_out);

/* host-only: decode a block of legacy-MT19937 32-bit words into replay codes, consuming words
 * exactly as rand() (2 words) and choice(3) (masked rejection, 1 word per try) do.
 * eps for decision k is eps[k % n_eps].  Returns P2PMG_E_INVALID if the words run out. */
int p2pmg_replay_decode(const uint32_t* words, size_t n_words, size_t n_decisions,
                        const double* eps, size_t n_eps, uint8_t* codes, size_t* consumed);

/* ---- DQN variant (rl.py:135-359, agent.py:301-350; BASELINE.json configs[4]) -------------
 * create with config.learner = P2PMG_LEARNER_DQN (no Q-table is allocated), then
 * p2pmg_dqn_setup.  Per agent (or ONE network with config.shared_q = 1, or one per ROLE with
 * p2pmg_dqn_setup_roles, below): online and target
 * QNetwork 5->64->64->1 (Keras weight order, P2PMG_DQN_PARAMS floats), Adam state and a replay
 * ring of `capacity` transitions (s[4], a, r, ns[4]).  p2pmg_run_episode dispatches to the DQN
 * step pipeline: per timestep an act kernel (negotiation rounds with the Q-MLP, market, memory)
 * then, in TRAIN mode, the train kernel (sample 32, target/online forward + backward on f32
 * MFMA, clip, Adam, soft update). */
#define P2PMG_DQN_PARAMS 4609
#define P2PMG_DQN_ONLINE 0
#define P2PMG_DQN_TARGET 1
#define P2PMG_DQN_ADAM_M 2
#define P2PMG_DQN_ADAM_V 3

typedef struct p2pmg_dqn_config {
  double gamma;    /* 0.95 agent.py:309 */
  double tau;      /* 0.005 soft update agent.py:309 */
  double lr;       /* 1e-5 Adam agent.py:310 */
  double beta1, beta2, adam_eps; /* Keras Adam defaults .9, .999, 1e-7 */
  double clip;     /* 1.0: first kernel's gradient clipped to [-clip, clip] (rl.py:329) */
  int32_t batch;   /* 32 (agent.py:308); the only supported value */
  int32_t capacity; /* 5000 (agent.py:308) */
  int32_t agents_per_block; /* shared network: agents whose gradients one workgroup sums (0 = auto:
                               ceil(A / (CUs x workgroups per CU)), i.e. device- and shard-dependent) */
  int32_t grad_segments;    /* shared network: the context's agents split into this many contiguous
                               gradient segments of whole scenarios (0 = 1).  The gradient of an env
                               step is sum over segments (in global segment order) of the segment's
                               sum over its agents_per_block blocks (16 slices, fixed order): with
                               agents_per_block and the TOTAL segment count fixed, 1 rank x G segments
                               == W ranks x G/W segments bit for bit (rl.py:307-333 averaged over
                               agents, build-defined) */
} p2pmg_dqn_config;

int p2pmg_dqn_config_default(p2pmg_dqn_config* cfg);
int p2pmg_dqn_setup(p2pmg_ctx* ctx, const p2pmg_dqn_config* cfg);
/* which = P2PMG_DQN_*; nets [first, first+count) of [count][P2PMG_DQN_PARAMS] f32 */
int p2pmg_dqn_set_weights(p2pmg_ctx* ctx, int which, int first, int count, const float* host);
int p2pmg_dqn_get_weights(p2pmg_ctx* ctx, int which, int first, int count, float* host);
/* Adam iterations done (Keras `iterations`).  Each network has its own count (one optimizer per
 * DQNAgent, agent.py:310): set_step sets every network's, get_step reads network 0's, an episode's
 * env step advances every network's and p2pmg_dqn_train_batch only the network it trains. */
int p2pmg_dqn_set_step(p2pmg_ctx* ctx, int64_t step);
int p2pmg_dqn_get_step(p2pmg_ctx* ctx, int64_t* step);
int p2pmg_dqn_get_net_steps(p2pmg_ctx* ctx, int first, int count, int64_t* steps);
/* replay mode: deque indices (0 = oldest) of random.sample(buffer, 32) (rl.py:238) [T][A][32] */
int p2pmg_dqn_set_samples(p2pmg_ctx* ctx, const uint16_t* samples);
/* replay memory of agents [first, first+count): [count][capacity][10] f32 ring + added[count] */
int p2pmg_dqn_get_buffer(p2pmg_ctx* ctx, int first, int count, float* host, int32_t* added);
int p2pmg_dqn_set_buffer(p2pmg_ctx* ctx, int first, int count, const float* host, const int32_t* added);
/* QNetwork.call (rl.py:147-148) of one network on n rows x = concat(state, action) [n][5] */
int p2pmg_dqn_forward(p2pmg_ctx* ctx, int net, int n, const float* x, float* q);
/* Trainer._train + update_targets (rl.py:307-359) of one network on a given batch [32][10] */
int p2pmg_dqn_train_batch(p2pmg_ctx* ctx, int net, const float* batch, float* loss);
/* Per-network learner constants of the DQN learner: each DQNAgent's own Trainer(gamma, tau, Adam(learning_rate))
 * (agent.py:306-311, rl.py:253-266), the first kernel's gradient clip (rl.py:329) and the comfort weight of each
 * agent's reward (agent.py:225-232).  gamma, tau, lr and clip are [n_nets] (A rows for per-agent networks, one row
 * for the shared network, N rows on a role context); penalty_weight is [A], per AGENT, in either case.  A NULL pointer leaves that field as
 * it is; all five NULL restore what p2pmg_dqn_setup filled in: every row from p2pmg_dqn_config, every weight from
 * config.penalty_weight.  The whole input is checked on the host before anything is uploaded: values must be
 * finite with 0 <= gamma <= 1, 0 <= tau <= 1, lr >= 0, clip > 0 and penalty_weight >= 0, else P2PMG_E_INVALID
 * (p2pmg_last_error names the network or agent) and the state stays untouched.  A tabular context, or a call
 * before p2pmg_dqn_setup: P2PMG_E_STATE.
 * Each value reaches the kernels as the f32 cast of the double (tau_c = 1.0f - (float)tau per row); betas and
 * adam_eps stay the context's.  dqn_train_kernel reads gamma (the target), clip (the first kernel's gradient)
 * and tau (the soft update): for per-agent networks each workgroup loads its network's row as wave-uniform
 * scalars, and only when the rows differ (equal rows take the scalar kernel arguments: the same bits as a
 * context that never calls this).  The Adam step size of a network follows its own lr and its own iteration
 * count; when either differs between networks the episode uploads a [T][n_nets] step-size table.  The shared
 * network's reduce / Adam kernels (and the act kernel's fused Adam step) and p2pmg_dqn_train_batch read row 0,
 * or row `net`.  Both act kernels and the greedy evaluation (p2pmg_dqn_run_greedy) read the per-agent comfort
 * weight; of a greedy episode only the recorded rewards depend on it.  A change takes effect at the next launch
 * (a train episode or p2pmg_dqn_train_batch): a learning-rate or tau schedule across episodes needs no new
 * context, and the Adam moments and iteration counts are not reset.  Over several ranks every rank of a shared
 * network must be given the same row, as it must hold the same weights. */
int p2pmg_dqn_set_learning(p2pmg_ctx* ctx, const double* gamma, const double* tau, const double* lr,
                           const double* clip, const float* penalty_weight /* [A], per AGENT */);
/* the values in use: gamma, tau, lr, clip [n_nets], penalty_weight [A]; any output may be NULL */
int p2pmg_dqn_get_learning(p2pmg_ctx* ctx, double* gamma, double* tau, double* lr, double* clip,
                           float* penalty_weight);
/* One DQN episode with one exploration rate per scenario, eps [S] in [0, 1]: modes TRAIN and FILL with
 * P2PMG_RNG_PHILOX only (replay codes already carry each agent's decision: REPLAY and GREEDY return
 * P2PMG_E_INVALID).  args->epsilon is not read.  Each scenario's {threshold, explore-all} pair is formed exactly
 * as p2pmg_run_episodes_eps forms it and read by both act kernels (the MFMA act kernel per agent slot: a
 * workgroup's slots may span scenarios), so scenario s explores as a p2pmg_run_episode at epsilon = eps[s]
 * would, bit for bit. */
int p2pmg_dqn_run_episode_eps(p2pmg_ctx* ctx, const p2pmg_episode_args* args, const double* eps /* [S] */);

/* The DQN policy map: what the table digests are for a Q-table, for a Q-network.  For each network the
 * Q-MLP is evaluated ON THE DEVICE at every state of a rectangular grid of observations and at the three
 * action values (ActorModel.greedy_action rl.py:188-196 over the state grid of data_analysis.py's
 * plot_q_values_* and compare_decisions*), and only what was asked for reaches the host: one byte per
 * state, eight numbers per network, the Q values themselves, or one count per network against a snapshot.
 *
 * Grid.  Four axes of f32 values, time[n0], temp[n1], balance[n2], p2p[n3].  State
 * g = ((i0 n1 + i1) n2 + i2) n3 + i3 has the observation (time[i0], temp[i1], balance[i2], p2p[i3]): the
 * reference's (time, temp, balance, p2p) order, time slowest, the order of p2pmg_get_q and
 * p2pmg_greedy_policy.  G = n0 n1 n2 n3, every n >= 1, G <= 2^31 - 1 (else P2PMG_E_INVALID).
 * p2pmg_dqn_set_grid uploads the axes; all four axes NULL (n is then ignored) restores the DEFAULT grid:
 * the context's table shape (n_time_states .. n_p2p_states), each axis at its bins' centres, formed in f64
 * and cast to f32: time (k + 1/2) / K, temp 2 (k - 1/2) / (K - 2) - 1, balance and p2p 2 (k + 1/2) / K - 1.
 * The default needs n_temp_states >= 3 (else P2PMG_E_INVALID from every call until axes are set) and is in
 * use until p2pmg_dqn_set_grid says otherwise.  On it, state g of a map is the state of row g of a table's
 * packed policy (each centre falls in its own bin), so tabular and DQN policies compare byte for byte.
 * p2pmg_dqn_get_grid returns the shape and, if axes != NULL, the n0 + n1 + n2 + n3 values in use,
 * time | temp | balance | p2p.
 *
 * Q values.  q[g][a], a = 0, 1, 2 (action values 0, 1/2, 1), is what dqn_act_kernel and
 * dqn_act_shared_kernel compute for that observation, bit for bit (oracle/dqn.py::act_q): layer 1 starts
 * from p2p W1[3], then fmaf with balance, temp and time; the action term is z + b1, fmaf(0.5, W1[4], z) + b1
 * or (z + W1[4]) + b1; layer 2 is the fmaf chain over k = 0..63 from +0 (the f32 MFMA's k order); layer 3
 * is the pairwise tree over the 64 units, then + b3.  A byte of the map is therefore the action the act
 * kernel takes at that observation when it does not explore.
 *   greedy action  g = 0; for k = 1, 2 in order: if q[k] > q[g] then g = k.  The FIRST maximum.  There is no
 *                  "unvisited" value: every byte is 0, 1 or 2.
 * Networks are assumed NaN-free.  Every statistic is a count, a minimum or a maximum, so no launch shape
 * or fold order changes a bit; f32 widens to f64 exactly; zeros are returned as +0.0.
 *
 * All calls: `which` is P2PMG_DQN_ONLINE or P2PMG_DQN_TARGET (else P2PMG_E_INVALID); networks are
 * addressed as p2pmg_dqn_get_weights addresses them (A per-agent networks or 1 shared; first < 0,
 * count < 0 or first + count > n_nets: P2PMG_E_INVALID); they are stream-ordered after earlier launches,
 * synchronise before returning and read the weights as they are at the call.  Tabular context, or before
 * p2pmg_dqn_setup: P2PMG_E_STATE.  count == 0: P2PMG_OK, nothing written.  A NULL output (both, for
 * p2pmg_dqn_policy_map, which needs only one): P2PMG_E_INVALID.
 *
 * p2pmg_dqn_policy_map walks the networks (and, for grids beyond the bound, one network's states) in
 * chunks: its device staging never exceeds P2PMG_DQN_MAP_STAGE_BYTES, whatever count x G is.
 *
 * p2pmg_dqn_map_stats: P2PMG_DQN_MAP_STATS f64 values per network, stats[k][.] for network first + k:
 *    0 G           number of grid states
 *    1 q_min       minimum over all G x 3 Q values
 *    2 q_max       maximum over the same values
 *    3 abs_max     maximum of |q| over the same values (= max(-q_min, q_max))
 *    4..6 greedy[a]  number of states whose greedy action is a (fields 4..6 sum to field 0)
 *    7 min_gap     minimum over the states of the f32 difference q[greedy] - max(the other two)
 *
 * Churn.  p2pmg_dqn_policy_mark stores the packed map of EVERY network of `which` in a snapshot
 * [n_nets][G] u8 that the context owns on the device (one snapshot, whichever array it was taken of); the
 * first call allocates it (P2PMG_E_NOMEM if that fails, and there is then no snapshot).
 * p2pmg_dqn_policy_changes gives changed[k], the number of states of network first + k of `which` whose
 * greedy action now differs from the snapshot's; remark != 0 overwrites the snapshot of networks
 * [first, first + count), and of no other, in the same pass.  p2pmg_dqn_set_grid drops the snapshot.
 * Before a mark, or after a grid change: P2PMG_E_STATE. */
#define P2PMG_DQN_MAP_STATS 8
#define P2PMG_DQN_MAP_STAGE_BYTES (32u << 20)
int p2pmg_dqn_set_grid(p2pmg_ctx* ctx, const int32_t* n /* [4] */, const float* time, const float* temp,
                       const float* balance, const float* p2p);
int p2pmg_dqn_get_grid(p2pmg_ctx* ctx, int32_t* n /* [4] */, float* axes /* [n0 + n1 + n2 + n3] or NULL */);
int p2pmg_dqn_policy_map(p2pmg_ctx* ctx, int which, int first, int count, uint8_t* policy /* [count][G] or NULL */,
                         float* q /* [count][G][3] or NULL */);
int p2pmg_dqn_map_stats(p2pmg_ctx* ctx, int which, int first, int count, double* stats /* [count][P2PMG_DQN_MAP_STATS] */);
int p2pmg_dqn_policy_mark(p2pmg_ctx* ctx, int which);
int p2pmg_dqn_policy_changes(p2pmg_ctx* ctx, int which, int first, int count, int64_t* changed /* [count] */,
                             int remark);

/* DQN evaluation: frozen networks, one launch per greedy episode.  p2pmg_run_episode(P2PMG_MODE_GREEDY) on a
 * DQN context is T act launches, each streaming every agent's network again although nothing changes a
 * weight.  p2pmg_dqn_run_greedy runs the same T greedy env steps in ONE launch of
 * dqn_greedy_episode_kernel (one workgroup per scenario, the time loop inside; a wave loads its agent's
 * network once, T_in / T_m stay on the chip between steps), on the context's own networks or on a POLICY
 * SET: M networks and a map agent -> network that the context owns on the device beside the learner's
 * online, target and Adam arrays.  No training call reads or writes the set, so one community of N trained
 * networks is evaluated over S scenarios (days) at once with the role map a -> a % N.  Per-role networks
 * are TRAINED by a role context (p2pmg_dqn_setup_roles, on a context created with shared_q = 1), whose
 * ONLINE / TARGET sources here read network a % N for agent a; p2pmg_create with P2PMG_SHARED_ROLE and the
 * DQN learner is still refused, p2pmg_dqn_setup_roles is the route.
 *
 * p2pmg_dqn_set_policy_nets uploads count networks [count][P2PMG_DQN_PARAMS] and the map net_of [A], values
 * in [0, count).  The whole map is checked on the host before anything is uploaded: a value out of range is
 * P2PMG_E_INVALID and leaves the current set as it was.  net_of == NULL is the default map: a % count (role
 * i of every scenario) when count == N, the identity when count == A, all 0 when count == 1, and otherwise
 * P2PMG_E_INVALID.  count == 0 drops the set (weights and net_of are then ignored); count < 0 or NULL
 * weights: P2PMG_E_INVALID.  p2pmg_dqn_get_policy_nets returns the set: *count (0: none; nothing else is
 * then written) and, where non-NULL, the weights and the map in use.
 *
 * p2pmg_dqn_run_greedy: source = P2PMG_DQN_ONLINE or P2PMG_DQN_TARGET (the context's own array: agent a's
 * network, or network 0 of a shared context) or P2PMG_DQN_POLICY_SET; record = the P2PMG_REC_* mask of
 * REWARD, COST, GRID, P2P, TEMP and ACTION (same buffers and layouts as an episode's).  Stream-ordered and
 * timed like an episode: p2pmg_get_record, p2pmg_get_episode_reward, p2pmg_episode_summary,
 * p2pmg_day_profile and p2pmg_last_kernel_ms work after it, and p2pmg_last_kernel reads
 * "dqn_greedy_episode_kernel<N>".  Results, records, final temperatures and episode rewards are, bit for
 * bit, those of p2pmg_run_episode(P2PMG_MODE_GREEDY) on a per-agent DQN context whose network a is a copy
 * of the mapped network: every value is formed by the act kernels' expression sequence (the act_q order
 * above, the sequential sums over j, _divide_power, the pair exchange, cost, reward and RC update at the
 * agent's own thermal values and heat-pump levels, sum_t mean_i r in step order).  Any N in 1..64, any R
 * with R + 1 <= 4096, n_env 1 or S.  Greedy only: no RNG, no replay codes, no replay-memory append; every
 * weight array, the Adam step counts, the replay rings, their `added` counts and the replay-code state
 * are left as they were.  T_in / T_m move as in any episode.
 * Which form to prefer (MI355X, HIP events, profiles/dqn_eval/README.md): with per-agent networks, or a policy
 * set, this call: 1.4x to 2.0x faster than the stepwise episode at every shape measured, 5 to 4096
 * scenarios, one day to one year.  For ONE SHARED network over thousands of agents prefer
 * p2pmg_run_episode(P2PMG_MODE_GREEDY): its MFMA act kernel forwards 16 agents per workgroup on the matrix
 * cores and was 2.5x faster than this call's one wave per agent at configs[4]'s shape (4096 x 2, T = 96).
 * Errors: NULL context P2PMG_E_INVALID; tabular context, or before p2pmg_dqn_setup, P2PMG_E_STATE;
 * P2PMG_DQN_POLICY_SET without a set, or before env, profiles and agent params are set, P2PMG_E_STATE;
 * P2PMG_REC_LOSS (or any other bit outside the six records) or an unknown source P2PMG_E_INVALID. */
#define P2PMG_DQN_POLICY_SET 4
int p2pmg_dqn_set_policy_nets(p2pmg_ctx* ctx, int count, const float* weights /* [count][P2PMG_DQN_PARAMS] */,
                              const int32_t* net_of /* [A], values in [0, count), or NULL */);
int p2pmg_dqn_get_policy_nets(p2pmg_ctx* ctx, int* count, float* weights /* or NULL */, int32_t* net_of /* or NULL */);
int p2pmg_dqn_run_greedy(p2pmg_ctx* ctx, int source, int record);

/* Shared network over several ranks (config 5): the gradient segments of every rank are gathered
 * once per env step, then every rank sums all of them in global segment order and takes the same
 * Adam step, so the replicas stay bit-identical.  With an RCCL communicator (p2pmg_comm_init) the
 * gather is an in-place ncclAllGather on the context's stream (xGMI).  Without one, a host exchange
 * function does it: `segments` is [nranks][floats_per_rank] f32 host memory with this rank's part
 * filled in; the function fills every other rank's part (an all-gather over any transport, e.g.
 * gloo) and returns 0 (non-zero aborts the episode with P2PMG_E_STATE).  It is called
 * synchronously from p2pmg_run_episode, on the calling thread, once per training env step.
 * fn = NULL removes it (rank 0 of 1).  No reference counterpart (one process, rl.py:307-333). */
typedef int (*p2pmg_exchange_fn)(void* user, float* segments, int64_t floats_per_rank, int rank, int nranks);
int p2pmg_dqn_set_exchange(p2pmg_ctx* ctx, p2pmg_exchange_fn fn, void* user, int rank, int nranks);
/* the shared-network gradient layout in use: segments of this context, agents per train
 * workgroup, train workgroups per env step (a role context: 1, agents per workgroup, N x workgroups per role) */
int p2pmg_dqn_grad_layout(p2pmg_ctx* ctx, int* segments, int* agents_per_block, int* blocks);

/* One Q-network per ROLE: the reference's DQN community (get_community(DQNAgent, n): N DQNAgents, each with
 * its own Trainer, network and replay buffer, agent.py:301-311) trained over S scenarios (days, weather draws,
 * exploration streams) at once.  p2pmg_dqn_setup_roles takes the place of p2pmg_dqn_setup on a DQN context
 * created with shared_q = 1.  The context then holds N networks (online, target, Adam m and v and one Adam
 * iteration count each) and agent a = s N + i uses network i = a % N everywhere; replay rings, sample draws,
 * temperatures and records stay per agent.
 *   Errors: a tabular context, or after p2pmg_dqn_setup / p2pmg_dqn_setup_roles, P2PMG_E_STATE; a context
 *   created with shared_q = 0, P2PMG_E_INVALID; cfg->grad_segments other than 0 or 1, P2PMG_E_INVALID; a
 *   context that already has a communicator or a host exchange over several ranks, P2PMG_E_UNSUPPORTED.  On a
 *   role context p2pmg_comm_init, and p2pmg_dqn_set_exchange with nranks > 1, return P2PMG_E_UNSUPPORTED:
 *   per-role networks over several ranks or gradient segments are not built.  p2pmg_last_error gives the reason.
 * Definition of a training env step (build-defined, like the shared network's), for every role i on its own:
 * its agents a = k N + i, k = 0..S-1 in scenario order, are split into blocks of agents_per_block
 * consecutive k (0: the runtime's choice, ceil(S N / (CUs x workgroups per CU)), as for the shared network).
 * One train workgroup per block of a role chains the batch gradients of the block's agents in its
 * registers, as the shared network's workgroups do, and writes one partial.  The role's gradient is its
 * partials summed in dqn_reduce_adam_kernel's order (16 slices of ceil(blocks / 16) consecutive partials,
 * each from +0.0 in order, then the slices in order) times 1.0f / (float)S; then the first kernel's clip,
 * the Adam step at the role's own lr and iteration count and the soft update at its own tau (the
 * expressions every other DQN context uses).  So a role context with N = 1 is the shared-network context
 * bit for bit, and one with S = 1 the per-agent context bit for bit (one partial plus zeros, times 1).
 * Every entry point that takes a network index or range works on [0, N): p2pmg_dqn_set_weights /
 * get_weights, get_net_steps, dqn_forward, dqn_train_batch, the policy map calls.  p2pmg_dqn_set_learning /
 * get_learning take gamma, tau, lr and clip as [N] rows (the comfort weight stays [A]);
 * p2pmg_dqn_run_episode_eps works; p2pmg_dqn_run_greedy with ONLINE / TARGET evaluates agent a on network
 * a % N, the policy set staying independent.  Episodes run dqn_act_kernel, one wave per agent
 * (p2pmg_last_kernel: "dqn_act_kernel<N,roles>"), a train launch of N x blocks workgroups and ONE reduce + Adam
 * launch for all N roles.
 * p2pmg_dqn_roles: *n_roles = N on a role context, 0 on any other. */
int p2pmg_dqn_setup_roles(p2pmg_ctx* ctx, const p2pmg_dqn_config* cfg);
int p2pmg_dqn_roles(p2pmg_ctx* ctx, int* n_roles);

/* Interleaved chains.  A chained launch (p2pmg_run_episodes) of the fast kernel may run TWO of an
 * agent's consecutive episodes per 64-lane wave, episode e in lanes 0-31 and e + 1 in lanes 32-63,
 * T / 2 steps behind (p2pmg_last_kernel: "...,interleaved>"), where the results stay those of the
 * episodes run one after the other, bit for bit: Philox training with P2PMG_FLAG_RESET_T0 (the later
 * episode starts from its own T0 draw), N = 2, no battery, T % 6 == 0, n_temp_states <= 32, and
 * inputs whose hazard distance D allows it.  D is the largest u - v over an agent's steps u (of the
 * earlier episode) and v (of the later) that touch Q rows of one (time bin, balance bin) key with a
 * write involved; the launch interleaves iff D + 4 <= T / 2.  D depends only on what
 * p2pmg_set_env / set_profiles / set_agent_params uploaded and is computed on the device by the first
 * chained launch after an upload (T <= 512; beyond that D = -1 and the chain runs serially).
 * P2PMG_INTERLEAVE=0 in the environment (read once per process) turns the form off.
 * distance, safe (D + 4 <= T / 2): either may be NULL.  P2PMG_E_STATE before the first chained launch
 * after an upload. */
int p2pmg_chain_lag(p2pmg_ctx* ctx, int* distance, int* safe);

/* Policy sets: greedy episodes that act from PACKED BYTE POLICIES, not from Q rows.  A greedy episode needs
 * each row's greedy action and nothing else of the row; p2pmg_greedy_policy already defines that action as one
 * byte per state (160 KB per 20^4 table against 5.12 MB in f64).  A tabular context owns, beside its tables, a
 * POLICY SET: M packed policies [M][n_states] u8 and a map policy_of [A], agent -> policy.  No training call,
 * p2pmg_set_q, p2pmg_zero_q, p2pmg_policy_mark or table digest reads or writes the set, and nothing here reads
 * or writes a table (p2pmg_policy_set_capture reads tables), the policy-mark snapshot, a delta or a code buffer.
 * All four calls: NULL context P2PMG_E_INVALID; DQN context P2PMG_E_STATE (p2pmg_dqn_set_policy_nets serves
 * those).  A context that never calls them computes and launches exactly what it did before.
 *
 * Definitions, bit for bit.
 *   rows           a policy's bytes are in p2pmg_greedy_policy's order: state (it, iT, ib, ip) at
 *                  ((it * n_temp + iT) * n_balance + ib) * n_p2p + ip.
 *   legal bytes    0 .. n_actions-1 and P2PMG_POLICY_UNVISITED (255).  255 ACTS AS ACTION 0, an unvisited row's
 *                  greedy action (as p2pmg_policy_changes reads a snapshot byte).
 *   default map    policy_of == NULL: a when M == A; a % N (role i of every scenario) when M == N; 0 when
 *                  M == 1; tested in that order; any other M is P2PMG_E_INVALID.
 *
 * p2pmg_set_policy_set(count M, policies, policy_of): the whole input is checked on the host first
 * (validate_policy_set): a byte outside the legal set, a map entry outside [0, M), M < 0, or M without a default
 * map and policy_of == NULL give P2PMG_E_INVALID, nothing is uploaded and the set the context held stays as it
 * was.  policies == NULL allocates M slots filled with 255.  M == 0 frees the set (the other arguments are
 * ignored).  Memory: M * n_states + 4 * A bytes on the device; if that allocation fails, P2PMG_E_NOMEM, and the
 * set the context held stays as it was.
 * p2pmg_get_policy_set: *count (0: no set; nothing else is then written) and, where non-NULL, the M policies
 * and the map in use.
 * p2pmg_policy_set_capture(first_table, count, first_slot): slot first_slot + k becomes the packed greedy policy
 * of table first_table + k, exactly the bytes p2pmg_greedy_policy returns for it, by the same kernel
 * (table_digest_kernel) writing straight into the set: on the context's stream, no host round trip, no staging
 * buffer.  Per-agent, shared and role tables, f64 and f32, any n_actions the context holds.  It does not apply a
 * pending shared-table delta.  No set: P2PMG_E_STATE; first_table < 0, count < 0, first_table + count >
 * n_tables, first_slot < 0 or first_slot + count > M: P2PMG_E_INVALID.  count == 0: P2PMG_OK.
 *
 * p2pmg_run_policy(record): ONE greedy episode of every scenario in one launch of policy_episode_kernel.  Agent
 * a takes, in every round of every step, the action policies[policy_of[a]][state], where state is the row a
 * greedy p2pmg_run_episode would have gathered at that point: the same time, temperature and balance bins, and
 * the p2p bin of the round (that of p2p = 0 in round 0).  Everything else is the greedy episode of the general
 * kernel, expression for expression: the Jacobi rounds, _divide_power, the battery rule where one is set, the
 * pair exchange, costs, the reward at the agent's own comfort weight, the RC step at its own thermal values and
 * heat-pump levels, sum_t mean_i r.  So with policy p the packed greedy policy of agent a's table, records,
 * final T_in / T_m / SoC and episode rewards equal p2pmg_run_episode(P2PMG_MODE_GREEDY)'s bit for bit.  No RNG,
 * no update.  record = a P2PMG_REC_* mask without LOSS (P2PMG_E_INVALID otherwise).  It is "the last episode
 * launch": p2pmg_get_record, p2pmg_get_episode_reward, p2pmg_episode_summary, p2pmg_day_profile and
 * p2pmg_last_kernel_ms work after it; p2pmg_last_kernel reads "policy_episode_kernel<N,R1=..>" (",tileNC" after
 * N in the LDS-tile form, ",battery" with one).  Any N in 1..64 (registers for N in {1..8, 16}, LDS tiles for
 * the rest) and any R the context accepts.  p2pmg_run_policy_ex(record, flags): flags = 0 is p2pmg_run_policy;
 * P2PMG_FLAG_TILE_KERNEL runs the LDS-tile form at any N (the cross-check of the two forms); any other flag
 * P2PMG_E_INVALID.
 * Errors: no set, or before env, profiles and agent params are set, P2PMG_E_STATE; an n_actions == 2 context
 * P2PMG_E_UNSUPPORTED, as for episodes. */
int p2pmg_set_policy_set(p2pmg_ctx* ctx, int count, const uint8_t* policies /* [count][n_states] or NULL */,
                         const int32_t* policy_of /* [A], values in [0, count), or NULL */);
int p2pmg_get_policy_set(p2pmg_ctx* ctx, int* count, uint8_t* policies /* or NULL */, int32_t* policy_of /* or NULL */);
int p2pmg_policy_set_capture(p2pmg_ctx* ctx, int first_table, int count, int first_slot);
int p2pmg_run_policy(p2pmg_ctx* ctx, int record);
int p2pmg_run_policy_ex(p2pmg_ctx* ctx, int record, int flags);

#ifdef __cplusplus
}
#endif
#endif /* P2PMG_H */
