// p2pmg_ctx.h — the context behind the C ABI of libp2pmg.so (include/p2pmg.h) and what the runtime units
// (p2pmg_rt_*.cpp) share: its buffer, event and stream types, the error macros, and the helpers more than
// one unit calls.  Private to those units: no .hip file includes it.  No C++ exception crosses the ABI:
// every entry point returns a status and records a message in the context.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "p2pmg.h"
#include "p2pmg_internal.h"
#include "p2pmg_plan.h"

// A device (or pinned host) array its holder owns: freed with the holder, move-only.
template <typename T, bool Pinned = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {  // o takes what this held, and frees it
    return std::swap(p_, o.p_), std::swap(cap_, o.cap_), *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr, cap_ = 0;
  }
  // n elements (at least 16 bytes); what it held is freed first, and a failure leaves {null, 0}
  hipError_t alloc(size_t n) {
    release();
    const size_t bytes = n * sizeof(T) > 0 ? n * sizeof(T) : 16;
    const hipError_t e = Pinned ? hipHostMalloc(reinterpret_cast<void**>(&p_), bytes, hipHostMallocDefault)
                                : hipMalloc(reinterpret_cast<void**>(&p_), bytes);
    if (e == hipSuccess) cap_ = n;
    else p_ = nullptr;
    return e;
  }
  // at least n elements: kept when it already holds them, else reallocated (contents lost)
  hipError_t grow(size_t n) { return p_ && cap_ >= n ? hipSuccess : alloc(n); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
template <typename T>
using PinBuf = DevBuf<T, true>;

// Start / stop event pairs, created on first use; the k-th timed interval uses pair k % slots.
struct EventRing {
  std::vector<hipEvent_t> ev;
  ~EventRing() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t ensure(int slots) {
    if (!ev.empty()) return hipSuccess;
    ev.assign(2 * (size_t)slots, nullptr);
    for (auto& e : ev) {
      const hipError_t rc = hipEventCreate(&e);
      if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
  }
  hipEvent_t* pair(long long k) { return &ev[2 * (size_t)(k % (long long)(ev.size() / 2))]; }
  hipError_t elapsed(long long k, float* ms) {  // waits for the interval's stop event
    const hipError_t e = hipEventSynchronize(pair(k)[1]);
    return e != hipSuccess ? e : hipEventElapsedTime(ms, pair(k)[0], pair(k)[1]);
  }
};

struct Stream {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
};

// What the last episode launch left behind (finish_launch writes it; tabular, rule and DQN alike).
struct LastLaunch {
  int mask = 0;         // records it wrote (p2pmg_get_record checks it)
  int packed_mask = 0;  // ... those of them that live packed in rec_pack (fast / sq16 launches)
  int narrow = 0;       // ... as [T][A] float2 {reward, cost} (fast / sq16 with only those two requested)
  bool timed = false;   // a launch has run since the context was created
  std::string kernel;
};

// Members are destroyed in reverse order: every buffer is freed before the events and the stream,
// which are declared first (p2pmg_destroy synchronises the stream before the delete).
struct p2pmg_ctx : p2pmg::PlanFacts {
  int device = 0;
  size_t n_states = 0;
  size_t q_elem = 8;
  Stream stream;
  static constexpr int kRing = 4096;
  EventRing ring;                 // start/stop of each episode kernel
  long long n_timed = 0;          // launches recorded since the last reset
  static constexpr int kCRing = 1024;
  EventRing cring;                // start/stop of each data-path RCCL all-reduce
  long long n_coll = 0;           // collectives recorded since the last reset
  double coll_folded_ms = 0.0;    // durations of ring slots already reused (p2pmg_collective_ms)
  long long n_coll_folded = 0;    // collectives whose durations are in coll_folded_ms
  int timing_period = 1;          // episode launches: stamp timing events on every k-th one
  long long n_launch = 0;         // episode launches since the last reset
  LastLaunch last;
  // device buffers
  DevBuf<float> env;
  DevBuf<float2> prof;
  DevBuf<uint2> sqp;                // sq16 path: per-upload step words (launch_sq16_prep), lazily allocated
  long long sqp_version = -1;       // inputs_version they were computed for
  DevBuf<float> max_in, t_in, t_m;
  DevBuf<char> q;
  DevBuf<uint32_t> codes;  // code words [T][W][A]
  // fast path: step pre-pass outputs, double-buffered.  Episode e's launch also computes, in extra
  // workgroups, slot (e+1)'s pre-pass for episode e + 1 at the same epsilon (it reads only inputs,
  // never Q or T); run_episode(e + 1) uses it when its arguments match (spec_*), else recomputes.
  DevBuf<uint2> pre[2];        // [T][A] {balw, bins}
  DevBuf<uint32_t> pre_ipc[2]; // N = 2: [T][A] round-1 bins per partner action
  DevBuf<uint32_t> pcodes[2];  // Philox code words [T][W][A], one per episode of a chain
  int pslot = 0;
  bool spec_valid[2] = {false, false};
  int spec_episode[2] = {0, 0};
  std::vector<double> spec_chain[2];  // the epsilons of the chain a slot holds (one: {eps})
  DevBuf<float> chain_rew;            // p2pmg_run_episodes: [n][S] episode rewards of the last call (capacity in floats)
  int chain_n = 0;
  // pinned host staging of the small per-episode read-backs (episode rewards, metrics): a pageable
  // destination takes HIP's staged copy path (~26 us for 16 KB with the device idle)
  PinBuf<char> h_small;
  long long spec_version[2] = {-1, -1};
  long long inputs_version = 0;  // bumped by every input upload (env, profiles, max_in, hp levels)
  long long spec_hits = 0, spec_misses = 0;  // fast-path launches whose pre-pass was / was not ready
  // hazard distance of an interleaved chain over the uploaded inputs (launch_chain_lag), computed by
  // the first chained launch after an upload; chain_lag_ok (PlanFacts) is its verdict
  DevBuf<int> d_lag;
  int chain_lag = -1;            // -1: not computed (T > kChainLagMaxT)
  long long lag_version = -1;    // inputs_version it was computed for
  DevBuf<char> dummy;        // fast path: target of masked-off stores (2 * 64 * 32 B)
  DevBuf<char> rec_pack;     // fast path: packed records [T][A] x 32 B
  int code_src = 0;          // what the code buffer holds: 0 none, 1 replay upload, 2 Philox pre-pass
  DevBuf<float> ep_reward;
  DevBuf<float> rec_f32[5];  // reward, cost, grid, p2p, tin
  DevBuf<uint8_t> rec_action;
  DevBuf<int32_t> rec_index;
  DevBuf<char> rec_stage;    // fast / sq16 launches: one staging buffer the packed rows unpack into
  DevBuf<double> sum_agent, sum_scen;  // p2pmg_episode_summary: [A][16] and [S][16], allocated on first use
  // p2pmg_day_profile: the four outputs of the last call ([G][P][N][16], [G][P][N][8], [G][P][4], [G][P][2]) and
  // the uploaded labels [S]; allocated or grown on first use, re-initialised on the stream at every call
  DevBuf<unsigned long long> dp_sums, dp_csums;
  DevBuf<uint32_t> dp_ext, dp_cext;
  DevBuf<int32_t> dp_labels;
  // the table digests (p2pmg_table_stats & co.): block partials and folded results of the last call, and
  // the packed-policy snapshot [n_tables][n_states] u8 of p2pmg_policy_mark; all allocated on first use
  DevBuf<double> td_part, td_out;
  DevBuf<long long> td_cpart, td_cout;
  DevBuf<uint8_t> policy_snap;
  // the policy set (p2pmg_set_policy_set): pset_count packed policies and the agent -> policy map, read by
  // p2pmg_run_policy and written by p2pmg_policy_set_capture alone; no training call, table call or digest
  // reads or writes them
  DevBuf<uint8_t> pset;          // [pset_count][n_states]
  DevBuf<int32_t> pset_map;      // [A]
  std::vector<int32_t> h_pset_map;
  int pset_count = 0;            // 0: no set
  // the sparse table checkpoints (p2pmg_get_q_sparse & co.): block counts / offsets, per-table totals and
  // bases of the last call, and the staging of one run (at most P2PMG_SPARSE_STAGE_BYTES, unless one
  // table alone holds more); all allocated on first use
  DevBuf<uint32_t> sp_blk;
  DevBuf<long long> sp_total, sp_base;
  DevBuf<int32_t> sp_rows;
  DevBuf<char> sp_vals;
  DevBuf<float4> hp_lv;     // [A] per-agent heat-pump levels
  DevBuf<float4> thermal;    // [A] per-agent {setpoint, lower bound, upper bound, COP} (p2pmg_set_thermal)
  DevBuf<p2pmg::LearnRow> learn;  // [A] per-agent {alpha, gamma, comfort weight} (p2pmg_set_learning)
  std::vector<p2pmg::LearnRow> h_learn;  // its host copy (p2pmg_get_learning, partial updates)
  DevBuf<uint2> eps_tab;     // p2pmg_run_episodes_eps: [n][S] {threshold, explore-all} of the call
  const uint2* eps_cur = nullptr;  // ... the rows of the launch being prepared (eps_table, PlanFacts)
  DevBuf<float> hp_on;       // [A] RuleAgent heat-pump state (lazily allocated, starts off)
  DevBuf<double> soc, bat_cap;  // [A]
  // operand domains of the battery rule's range-test-free variant (battery_rule_r<false>):
  bool bat_domain = false;   // capacities, SoC bounds, sqrt(eff) and SoC0 in range (set_battery)
  bool prof_bounded = false; // every |load|, |pv| <= 2^100 and finite (set_profiles)
  bool hp_bounded = true;    // every heat-pump level |x| <= 2^100 and finite (defaults: 0 .. 3 kW)
  double bat_min = 0.1, bat_max = 0.9, bat_sqrt_eff = 1.0;
  size_t n_tables = 0;         // Q-tables held: A (shared_q = 0), 1 (1), N (P2PMG_SHARED_ROLE); 0 with the DQN learner
  DevBuf<long long> qdelta;    // shared table deltas [kDeltaCopies][n_tables][n_states][4]
  size_t delta_n() const { return n_tables * n_states * p2pmg::kQPad; }  // entries of one delta replica
  void* comm = nullptr;        // ncclComm_t
  int rank = 0, nranks = 1;    // this context's rank and the world (RCCL communicator or DQN host exchange)
  p2pmg_exchange_fn xfn = nullptr;  // DQN shared network: host gather of the gradient segments
  void* xuser = nullptr;
  DevBuf<double> d_metrics;            // [2] episode-metric sum and count (p2pmg_allreduce_metrics)
  DevBuf<unsigned long long> d_hash;   // [nranks] table fingerprints (p2pmg_table_hash_allgather)
  bool have_env = false, have_prof = false, have_params = false, have_codes = false;
  // DQN learner (config.learner = P2PMG_LEARNER_DQN)
  bool dqn = false;
  p2pmg_dqn_config dcfg{};
  int n_nets = 0;
  // p2pmg_dqn_setup_roles: n_nets = N networks, agent a on network a % N (d_role_map [A], what
  // p2pmg_dqn_run_greedy hands the evaluation kernel as net_of); d_bps / d_blocks count per role / in all
  bool dqn_roles = false;
  DevBuf<int32_t> d_role_map;
  DevBuf<float> d_theta, d_target, d_m, d_v;  // [n_nets][kNetStride]
  DevBuf<float> d_grad;   // shared network: [d_blocks][kNetStride] partials
  DevBuf<float> d_alt;    // shared network: the other half of the Adam double buffer, [4][kNetStride]
                          // (online, target, m, v) for the act kernel's fused post-exchange Adam step
  DevBuf<float> d_segs;   // [nranks * d_seg_local][kNetStride] gradient segments, global order
  PinBuf<float> h_segs;   // pinned host copy of d_segs (host exchange)
  DevBuf<float> d_smp;    // [A][32] int32 ring slots sampled for the current step
  int d_blocks = 0, d_apb = 1;
  int d_seg_local = 1, d_seg_agents = 0, d_bps = 0;  // gradient segments of this context (p2pmg_dqn_config)
  DevBuf<float> d_buf;       // [A][capacity][10]
  DevBuf<int32_t> d_added;   // [A]
  DevBuf<uint16_t> d_samples;     // [T][A][32]
  DevBuf<uint16_t> d_samples_px;  // [T][A][32]: a Philox training episode's draws (dqn_sample_prepass_kernel)
  bool have_samples = false;
  DevBuf<float> d_ep_acc;  // [S]
  DevBuf<float> rec_loss;  // [T][A]
  // the DQN policy map (p2pmg_dqn_policy_map & co.): the grid axes in use (time | temp | balance | p2p,
  // set on first use or by p2pmg_dqn_set_grid), block partials and folded results of the last call, and
  // the packed-map snapshot [n_nets][map_G] u8 of p2pmg_dqn_policy_mark
  uint32_t map_n[4] = {0, 0, 0, 0};
  size_t map_G = 0;
  std::vector<float> h_map_axes;
  DevBuf<float> map_axes;
  DevBuf<p2pmg::DqnMapPart> map_part;
  DevBuf<double> map_out;
  DevBuf<long long> map_cout;
  DevBuf<uint8_t> map_snap;
  // the evaluation policy set (p2pmg_dqn_set_policy_nets): pol_count networks and the agent -> network map,
  // read by p2pmg_dqn_run_greedy(P2PMG_DQN_POLICY_SET) alone; no training call reads or writes them
  DevBuf<float> d_pol;          // [pol_count][kNetStride]
  DevBuf<int32_t> d_pol_map;    // [A]
  std::vector<int32_t> h_pol_map;
  int pol_count = 0;            // 0: no set
  std::vector<int64_t> d_steps;  // Adam iterations done, per network (agent.py:310: one optimizer per agent)
  // p2pmg_dqn_set_learning: each network's {gamma, tau, lr, clip} and each agent's comfort weight, their
  // device forms ([n_nets] {gamma, tau, 1 - tau, clip} as f32, [A] f32), and whether two rows differ in
  // what the train kernel reads (d_hyp_mixed: it then loads its row) or in lr (d_lr_mixed: the lr table)
  std::vector<p2pmg::DqnLearn> h_dlearn;
  std::vector<float> h_penw;
  DevBuf<float4> d_hyp;
  DevBuf<float> d_penw;
  bool d_hyp_mixed = false, d_lr_mixed = false;
  DevBuf<float> d_lr;      // [T][n_nets] per-network step sizes of one episode when the counts differ
  std::vector<float> h_lr;
  int64_t d_added_min = 0;    // every ring holds at least this many transitions
  std::string err;
};

inline int fail(p2pmg_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIP_TRY(ctx, expr)                                                                       \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess)                                                                        \
      return fail((ctx), _e == hipErrorOutOfMemory ? P2PMG_E_NOMEM : P2PMG_E_HIP,                \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                            \
  } while (0)

#define RC_TRY(expr)                      \
  do {                                    \
    const int _rc = (expr);               \
    if (_rc != P2PMG_OK) return _rc;      \
  } while (0)

// ---- RCCL, resolved at run time (torch may already have loaded its own librccl; dlopen by
// SONAME then reuses it, and the library stays loadable on hosts without RCCL)
struct Id128 {  // ncclUniqueId, passed by value to ncclCommInitRank
  char b[128];
};
struct Rccl {
  void* h = nullptr;
  int (*getUniqueId)(void*) = nullptr;
  int (*commInitRank)(void**, int, Id128, int) = nullptr;
  int (*allReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;  // ncclDataType_t, ncclRedOp_t as int
  int (*commDestroy)(void*) = nullptr;
  const char* (*getErrorString)(int) = nullptr;
  int (*allGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*commCount)(const void*, int*) = nullptr;
};

// What more than one unit calls.  Each is defined once, in the unit named; the per-process state behind
// overrides() and rccl() lives in that unit alone.  RT_LOCAL: the library exports what include/p2pmg.h
// declares, and a definition takes its visibility from the declaration here.
#define RT_LOCAL __attribute__((visibility("hidden")))
namespace p2pmg::rt {

// ---- p2pmg_rt_core.cpp
RT_LOCAL int ensure_records(p2pmg_ctx* c, int mask);  // every record buffer in mask exists (lazily allocated, kept)
RT_LOCAL const Overrides& overrides();  // the environment overrides, read once per process on first use

// The ring pair a launch is timed with; null events: this launch carries none (timing period).
struct Timed {
  hipEvent_t e0 = nullptr, e1 = nullptr;
};
// sampled: only every timing_period-th launch carries events (dispatch-stamped events cost ~4 us per
// launch at configs[1], ~5 % of an episode).  record: stamp the start here (launches that do not
// stamp their own events).
RT_LOCAL int begin_timed(p2pmg_ctx* c, bool sampled, bool record, Timed* t);
RT_LOCAL int end_timed(p2pmg_ctx* c, const Timed& t, bool record);
// what an episode launch left behind: the one writer of c->last
RT_LOCAL void finish_launch(p2pmg_ctx* c, const Timed& t, std::string kernel, int mask, int packed_mask, int narrow);

// Copies on the context's stream, in order, then one synchronisation: host -> device / device -> host.
struct Copy {
  void* dst;
  const void* src;
  size_t bytes;
};
RT_LOCAL int upload(p2pmg_ctx* c, std::initializer_list<Copy> copies);
RT_LOCAL int download(p2pmg_ctx* c, std::initializer_list<Copy> copies);
// device -> caller's host memory through the pinned staging buffer (stream-ordered, then synced)
RT_LOCAL int read_small(p2pmg_ctx* c, void* host, const void* dev, size_t bytes);

RT_LOCAL size_t table_bytes(const p2pmg_ctx* c, size_t count = 1);  // count whole tables
RT_LOCAL char* table_ptr(p2pmg_ctx* c, size_t table);
RT_LOCAL int ensure_codes(p2pmg_ctx* c);
RT_LOCAL int ensure_hp_on(p2pmg_ctx* c);

// ---- p2pmg_rt_episode.cpp
RT_LOCAL EpisodeParams episode_params(p2pmg_ctx* c, const p2pmg_episode_args* args);

// ---- p2pmg_rt_tables.cpp
// tables [first, first + count) as a digest call addresses them: P2PMG_OK, or the status and message of `what`
RT_LOCAL int digest_range(p2pmg_ctx* c, int first, int count, const char* what);
// one table_digest_kernel pass over that range with no output switched on yet
RT_LOCAL p2pmg::TableDigestParams digest_params(p2pmg_ctx* c, int first, int count);

// ---- p2pmg_rt_dqn.cpp
RT_LOCAL int dqn_ready(p2pmg_ctx* c, const char* what);
RT_LOCAL float* dqn_array(p2pmg_ctx* c, int which);  // P2PMG_DQN_ONLINE .. P2PMG_DQN_ADAM_V, else null
RT_LOCAL int dqn_run_episode(p2pmg_ctx* c, const p2pmg_episode_args* args);

// ---- p2pmg_rt_comm.cpp
RT_LOCAL Rccl* rccl();  // null: no usable librccl
// HIP events around each data-path collective (shared-table delta, DQN gradient): end = 0 before, 1 after
RT_LOCAL hipError_t coll_mark(p2pmg_ctx* c, int end);

}  // namespace p2pmg::rt
