// p2pmg_rt_core.cpp — the context's life (create, destroy, errors, sync), the input and per-agent
// parameter accessors, timing and record read-backs, and the helpers every runtime unit shares
// (declared in p2pmg_ctx.h).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "p2pmg_ctx.h"
#include "p2pmg_dayprof.h"

using namespace p2pmg::rt;
using p2pmg::kEnvStride;
using p2pmg::kQPad;

// the rec_f32 slot of a float record, -1 for the others
static int rec_slot(int which) {
  switch (which) {
    case P2PMG_REC_REWARD: return 0;
    case P2PMG_REC_COST: return 1;
    case P2PMG_REC_GRID: return 2;
    case P2PMG_REC_P2P: return 3;
    case P2PMG_REC_TEMP: return 4;
    default: return -1;
  }
}

namespace p2pmg::rt {

int ensure_records(p2pmg_ctx* c, int mask) {
  const size_t ta = (size_t)c->T * c->A;
  for (int b = 0; b < 5; ++b)
    if ((mask & (1 << b)) && !c->rec_f32[b]) HIP_TRY(c, c->rec_f32[b].alloc(ta));
  const size_t tra = (size_t)c->T * (c->R + 1) * c->A;
  if ((mask & P2PMG_REC_ACTION) && !c->rec_action) HIP_TRY(c, c->rec_action.alloc(tra));
  if ((mask & P2PMG_REC_INDEX) && !c->rec_index) HIP_TRY(c, c->rec_index.alloc(tra));
  if ((mask & P2PMG_REC_LOSS) && !c->rec_loss) HIP_TRY(c, c->rec_loss.alloc(ta));
  return P2PMG_OK;
}

const Overrides& overrides() {
  static const Overrides ov = [] {
    const char *k = getenv("P2PMG_KERNEL"), *w = getenv("P2PMG_SPW"), *n = getenv("P2PMG_NO_SPEC");
    const char* il = getenv("P2PMG_INTERLEAVE");
    // P2PMG_INTERLEAVE: 0 = serial chains, 2 = at most two episodes per wave, anything else = the plan's choice
    return Overrides{k && !strcmp(k, "general"), w ? atoi(w) : 0, n && atoi(n) != 0, il && atoi(il) == 0,
                     il && atoi(il) == 2 ? 2 : 4};
  }();
  return ov;
}

int begin_timed(p2pmg_ctx* c, bool sampled, bool record, Timed* t) {
  HIP_TRY(c, c->ring.ensure(p2pmg_ctx::kRing));
  if (sampled && (c->n_launch++ % c->timing_period) != 0) return P2PMG_OK;
  t->e0 = c->ring.pair(c->n_timed)[0];
  t->e1 = c->ring.pair(c->n_timed)[1];
  if (record) HIP_TRY(c, hipEventRecord(t->e0, c->stream));
  return P2PMG_OK;
}

int end_timed(p2pmg_ctx* c, const Timed& t, bool record) {
  if (record && t.e1) HIP_TRY(c, hipEventRecord(t.e1, c->stream));
  return P2PMG_OK;
}

void finish_launch(p2pmg_ctx* c, const Timed& t, std::string kernel, int mask, int packed_mask, int narrow) {
  c->last.kernel = std::move(kernel);
  c->last.mask = mask;
  c->last.packed_mask = packed_mask;
  c->last.narrow = narrow;
  c->last.timed = true;
  if (t.e1) c->n_timed++;
}

static int copy_sync(p2pmg_ctx* c, std::initializer_list<Copy> copies, hipMemcpyKind kind) {
  for (const Copy& k : copies) HIP_TRY(c, hipMemcpyAsync(k.dst, k.src, k.bytes, kind, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int upload(p2pmg_ctx* c, std::initializer_list<Copy> copies) { return copy_sync(c, copies, hipMemcpyHostToDevice); }

int download(p2pmg_ctx* c, std::initializer_list<Copy> copies) { return copy_sync(c, copies, hipMemcpyDeviceToHost); }

int read_small(p2pmg_ctx* c, void* host, const void* dev, size_t bytes) {
  HIP_TRY(c, c->h_small.grow(bytes));
  RC_TRY(download(c, {{c->h_small, dev, bytes}}));
  std::memcpy(host, c->h_small, bytes);
  return P2PMG_OK;
}

size_t table_bytes(const p2pmg_ctx* c, size_t count) { return count * c->n_states * kQPad * c->q_elem; }

char* table_ptr(p2pmg_ctx* c, size_t table) { return c->q.get() + table_bytes(c, table); }

int ensure_codes(p2pmg_ctx* c) {
  if (!c->codes) HIP_TRY(c, c->codes.alloc((size_t)c->T * ((c->R + 4) / 4) * c->A));
  return P2PMG_OK;
}

int ensure_hp_on(p2pmg_ctx* c) {
  if (c->hp_on) return P2PMG_OK;
  HIP_TRY(c, c->hp_on.alloc((size_t)c->A));
  HIP_TRY(c, hipMemsetAsync(c->hp_on, 0, (size_t)c->A * sizeof(float), c->stream));
  return P2PMG_OK;
}

}  // namespace p2pmg::rt

// why the calling thread's last p2pmg_create failed, where it says (no context exists to hold it)
static thread_local std::string create_err;

extern "C" {

int p2pmg_device_count(int* count) {
  if (!count) return P2PMG_E_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return P2PMG_OK;
}

int p2pmg_create(const p2pmg_config* cfg, int device, p2pmg_ctx** out) {
  if (!cfg || !out) return P2PMG_E_INVALID;
  *out = nullptr;
  RC_TRY(p2pmg::validate_config(cfg, &create_err));
  const int N = cfg->n_agents;
  p2pmg_ctx* c = new (std::nothrow) p2pmg_ctx();
  if (!c) return P2PMG_E_NOMEM;
  c->cfg = *cfg;
  c->device = device;
  c->S = cfg->n_scenarios;
  c->N = N;
  c->R = cfg->rounds;
  c->T = cfg->horizon;
  c->A = c->S * c->N;
  c->n_states = (size_t)cfg->n_time_states * cfg->n_temp_states * cfg->n_balance_states * cfg->n_p2p_states;
  c->q_elem = cfg->q_dtype == P2PMG_Q_F64 ? 8 : 4;
  auto bail = [&](int code) {
    p2pmg_destroy(c);
    return code;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return bail(P2PMG_E_HIP);
  hipDeviceProp_t prop{};
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking) != hipSuccess) return bail(P2PMG_E_HIP);
  const size_t A = (size_t)c->A;
  if (c->prof.alloc((size_t)c->T * A) != hipSuccess || c->max_in.alloc(A) != hipSuccess ||
      c->t_in.alloc(A) != hipSuccess || c->t_m.alloc(A) != hipSuccess || c->ep_reward.alloc((size_t)c->S) != hipSuccess)
    return bail(P2PMG_E_NOMEM);
  // the code-word buffer always exists: greedy episodes read (and ignore) it, which keeps the
  // kernel's code loads unconditional
  const size_t ncw = (size_t)c->T * ((c->R + 4) / 4) * A;
  if (c->codes.alloc(ncw) != hipSuccess) return bail(P2PMG_E_NOMEM);
  if (c->dummy.alloc(2 * 64 * p2pmg::kFastRecBytes) != hipSuccess) return bail(P2PMG_E_NOMEM);
  if (hipMemsetAsync(c->codes, 0xFF, ncw * 4, c->stream) != hipSuccess) return bail(P2PMG_E_HIP);
  if (cfg->learner != P2PMG_LEARNER_TABULAR && cfg->learner != P2PMG_LEARNER_DQN) return bail(P2PMG_E_INVALID);
  c->dqn = cfg->learner == P2PMG_LEARNER_DQN;
  c->roles = cfg->shared_q == P2PMG_SHARED_ROLE;
  c->n_tables = c->dqn ? 0 : (c->roles ? (size_t)N : cfg->shared_q ? 1 : A);
  const size_t qbytes = table_bytes(c, c->n_tables);
  if (c->q.alloc(qbytes) != hipSuccess) return bail(P2PMG_E_NOMEM);
  if (cfg->shared_q && !c->dqn) {
    if (c->qdelta.alloc(p2pmg::kDeltaCopies * c->delta_n()) != hipSuccess) return bail(P2PMG_E_NOMEM);
    if (hipMemsetAsync(c->qdelta, 0, p2pmg::kDeltaCopies * c->delta_n() * 8, c->stream) != hipSuccess)
      return bail(P2PMG_E_HIP);
  }
  if (c->hp_lv.alloc(A) != hipSuccess || c->soc.alloc(A) != hipSuccess || c->thermal.alloc(A) != hipSuccess ||
      c->learn.alloc(A) != hipSuccess)
    return bail(P2PMG_E_NOMEM);
  {
    // the config's alpha, gamma and comfort weight for every agent: a context that never calls
    // p2pmg_set_learning computes what the broadcast kernel arguments did
    c->h_learn.assign(A, p2pmg::LearnRow{cfg->alpha, cfg->gamma, cfg->penalty_weight, {0.0f, 0.0f, 0.0f}});
    if (hipMemcpyAsync(c->learn, c->h_learn.data(), A * sizeof(p2pmg::LearnRow), hipMemcpyHostToDevice, c->stream) !=
        hipSuccess)
      return bail(P2PMG_E_HIP);
    std::vector<float4> lv(A, make_float4(cfg->hp_levels[0], cfg->hp_levels[1], cfg->hp_levels[2], 0.0f));
    // the config's scalars for every agent: a context that never calls p2pmg_set_thermal computes
    // what the broadcast kernel arguments did
    std::vector<float4> th(A, make_float4(cfg->setpoint, cfg->lower_bound, cfg->upper_bound, cfg->hp_cop));
    std::vector<double> s0(A, 0.5);
    if (hipMemcpyAsync(c->hp_lv, lv.data(), A * sizeof(float4), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(c->thermal, th.data(), A * sizeof(float4), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(c->soc, s0.data(), A * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return bail(P2PMG_E_HIP);
  }
  if (qbytes && hipMemsetAsync(c->q, 0, qbytes, c->stream) != hipSuccess) return bail(P2PMG_E_HIP);
  std::vector<float> t0(A, cfg->setpoint);
  if (hipMemcpyAsync(c->t_in, t0.data(), A * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(c->t_m, t0.data(), A * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return bail(P2PMG_E_HIP);
  *out = c;
  return P2PMG_OK;
}

int p2pmg_destroy(p2pmg_ctx* c) {
  if (!c) return P2PMG_OK;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm && rccl()) rccl()->commDestroy(c->comm);
  delete c;
  return P2PMG_OK;
}

const char* p2pmg_last_error(const p2pmg_ctx* c) {
  if (c) return c->err.c_str();
  return create_err.empty() ? "null context" : create_err.c_str();
}

int p2pmg_sync(p2pmg_ctx* c) {
  if (!c) return P2PMG_E_INVALID;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_device_info(p2pmg_ctx* c, char* name, size_t name_len, size_t* total_mem) {
  if (!c) return P2PMG_E_INVALID;
  hipDeviceProp_t prop;
  HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
  if (name && name_len) {
    std::snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (total_mem) *total_mem = prop.totalGlobalMem;
  return P2PMG_OK;
}

int p2pmg_set_env(p2pmg_ctx* c, int n_env, const float* time, const float* t_out, const float* buy, const float* inj,
                  const float* p2p) {
  if (c) c->inputs_version++;  // invalidates the speculative pre-pass slots
  if (!c || !time || !t_out || !buy || !inj || !p2p) return P2PMG_E_INVALID;
  if (n_env != 1 && n_env != c->S) return fail(c, P2PMG_E_INVALID, "n_env must be 1 or S");
  const size_t T = c->T;
  std::vector<float> h((size_t)n_env * T * kEnvStride, 0.0f);
  for (int s = 0; s < n_env; ++s)
    for (size_t t = 0; t < T; ++t) {
      float* r = &h[((size_t)t * n_env + s) * kEnvStride];  // time-major [T][n_env][8]
      const size_t k = (size_t)s * T + t;
      r[0] = time[k];
      r[1] = t_out[k];
      r[2] = buy[k];
      r[3] = inj[k];
      r[4] = p2p[k];
    }
  if (c->n_env != n_env) {
    HIP_TRY(c, c->env.alloc(h.size()));
    c->n_env = n_env;
  }
  RC_TRY(upload(c, {{c->env, h.data(), h.size() * 4}}));
  c->have_env = true;
  return P2PMG_OK;
}

int p2pmg_set_profiles(p2pmg_ctx* c, const float* load_w, const float* pv_w) {
  if (c) c->inputs_version++;  // invalidates the speculative pre-pass slots
  if (!c || !load_w || !pv_w) return P2PMG_E_INVALID;
  const size_t n = (size_t)c->A * c->T;
  DevBuf<float> dl, dp;
  HIP_TRY(c, dl.alloc(n));
  hipError_t e = dp.alloc(n);
  if (e != hipSuccess) return fail(c, P2PMG_E_NOMEM, "profile staging");
  {  // the battery rule's range-test-free variant needs bounded, finite balances (p2pmg_kernels.hip)
    bool ok = true;
    for (size_t k = 0; k < n; ++k) ok = ok && std::fabs(load_w[k]) <= 0x1p100f && std::fabs(pv_w[k]) <= 0x1p100f;
    c->prof_bounded = ok;
  }
  e = hipMemcpyAsync(dl, load_w, n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dp, pv_w, n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = p2pmg::launch_prof_pack(c->A, c->T, dl, dp, c->prof, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("set_profiles: ") + hipGetErrorString(e));
  c->have_prof = true;
  return P2PMG_OK;
}

int p2pmg_set_agent_params(p2pmg_ctx* c, const float* max_in) {
  if (c) c->inputs_version++;  // invalidates the speculative pre-pass slots
  if (!c || !max_in) return P2PMG_E_INVALID;
  RC_TRY(upload(c, {{c->max_in, max_in, (size_t)c->A * 4}}));
  c->mi_ok = true;
  for (int a = 0; a < c->A; ++a) {
    const float m = std::fabs(max_in[a]);
    if (!(m >= 0x1p-40f && m <= 0x1p40f)) c->mi_ok = false;
  }
  c->have_params = true;
  return P2PMG_OK;
}

int p2pmg_set_temperatures(p2pmg_ctx* c, const float* t_in, const float* t_m) {
  if (!c || !t_in || !t_m) return P2PMG_E_INVALID;
  return upload(c, {{c->t_in, t_in, (size_t)c->A * 4}, {c->t_m, t_m, (size_t)c->A * 4}});
}

int p2pmg_get_temperatures(p2pmg_ctx* c, float* t_in, float* t_m) {
  if (!c || !t_in || !t_m) return P2PMG_E_INVALID;
  return download(c, {{t_in, c->t_in, (size_t)c->A * 4}, {t_m, c->t_m, (size_t)c->A * 4}});
}

int p2pmg_reset_temperatures_philox(p2pmg_ctx* c, int episode, double sigma) {
  if (!c) return P2PMG_E_INVALID;
  const uint32_t off = (uint32_t)(c->cfg.scenario_offset * c->N);
  HIP_TRY(c, p2pmg::launch_t0_philox(c->A, c->t_in, c->t_m, (uint32_t)(c->cfg.seed & 0xFFFFFFFFu),
                                     (uint32_t)(c->cfg.seed >> 32), episode, off, c->thermal, sigma, c->stream));
  return P2PMG_OK;
}

int p2pmg_set_replay_codes(p2pmg_ctx* c, const uint8_t* codes) {
  if (!c || !codes) return P2PMG_E_INVALID;
  const size_t n = (size_t)c->T * (c->R + 1) * c->A;
  RC_TRY(ensure_codes(c));
  DevBuf<uint8_t> staging;
  HIP_TRY(c, staging.alloc(n));
  hipError_t e = hipMemcpyAsync(staging, codes, n, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = p2pmg::launch_pack_codes(c->T, c->R + 1, c->A, staging, c->codes, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("set_replay_codes: ") + hipGetErrorString(e));
  c->have_codes = true;
  c->code_src = 1;
  return P2PMG_OK;
}

int p2pmg_get_episode_rewards(p2pmg_ctx* c, int n, float* host) {
  if (!c || !host || n < 0) return P2PMG_E_INVALID;
  if (n > c->chain_n) return fail(c, P2PMG_E_STATE, "get_episode_rewards: the last run_episodes call ran fewer episodes");
  return download(c, {{host, c->chain_rew, (size_t)n * c->S * sizeof(float)}});
}

int p2pmg_get_episode_reward(p2pmg_ctx* c, float* host) {
  if (!c || !host) return P2PMG_E_INVALID;
  return read_small(c, host, c->ep_reward, (size_t)c->S * 4);
}

int p2pmg_set_timing_period(p2pmg_ctx* c, int period) {
  if (!c || period < 1) return P2PMG_E_INVALID;
  c->timing_period = period;
  c->n_launch = 0;
  return P2PMG_OK;
}

int p2pmg_set_hp_state(p2pmg_ctx* c, const float* on) {
  if (!c || !on) return P2PMG_E_INVALID;
  RC_TRY(ensure_hp_on(c));
  return upload(c, {{c->hp_on, on, (size_t)c->A * sizeof(float)}});
}

int p2pmg_get_hp_state(p2pmg_ctx* c, float* on) {
  if (!c || !on) return P2PMG_E_INVALID;
  RC_TRY(ensure_hp_on(c));
  return download(c, {{on, c->hp_on, (size_t)c->A * sizeof(float)}});
}

const char* p2pmg_last_kernel(const p2pmg_ctx* c) { return c ? c->last.kernel.c_str() : ""; }

int p2pmg_last_kernel_ms(p2pmg_ctx* c, float* ms) {
  if (!c || !ms) return P2PMG_E_INVALID;
  if (!c->last.timed || c->n_timed == 0) return fail(c, P2PMG_E_STATE, "no episode launched yet");
  HIP_TRY(c, c->ring.elapsed(c->n_timed - 1, ms));  // the ring pair of the last launch
  return P2PMG_OK;
}

int p2pmg_kernel_times(p2pmg_ctx* c, float* ms, int max, int* count) {
  if (!c || !ms || max < 0 || !count) return P2PMG_E_INVALID;
  const long long n = c->n_timed < p2pmg_ctx::kRing ? c->n_timed : p2pmg_ctx::kRing;
  const long long first = c->n_timed - n;
  int w = 0;
  for (long long k = first; k < c->n_timed && w < max; ++k, ++w) HIP_TRY(c, c->ring.elapsed(k, &ms[w]));
  *count = w;
  return P2PMG_OK;
}

int p2pmg_reset_kernel_times(p2pmg_ctx* c) {
  if (!c) return P2PMG_E_INVALID;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->n_timed = 0;
  c->n_launch = 0;
  c->n_coll = 0;
  c->coll_folded_ms = 0.0;
  c->n_coll_folded = 0;
  return P2PMG_OK;
}

int p2pmg_get_record(p2pmg_ctx* c, int which, void* host) {
  if (!c || !host) return P2PMG_E_INVALID;
  const size_t ta = (size_t)c->T * c->A;
  const size_t tra = (size_t)c->T * (c->R + 1) * c->A;
  const void* src = nullptr;
  size_t bytes = 0;
  const int slot = rec_slot(which);
  if (slot >= 0) {
    src = c->rec_f32[slot];
    bytes = ta * 4;
  } else if (which == P2PMG_REC_ACTION) {
    src = c->rec_action;
    bytes = tra;
  } else if (which == P2PMG_REC_INDEX) {
    src = c->rec_index;
    bytes = tra * 4;
  } else if (which == P2PMG_REC_LOSS) {
    src = c->rec_loss;
    bytes = ta * 4;
  } else {
    return fail(c, P2PMG_E_INVALID, "get_record: unknown record");
  }
  if (!(c->last.mask & which))
    return fail(c, P2PMG_E_STATE, "get_record: the last episode launch did not record this");
  if (c->last.packed_mask & which) {  // the last episode ran the fast / sq16 kernel: unpack its rows
    HIP_TRY(c, c->rec_stage.grow(bytes));
    const int w = slot >= 0 ? slot : (which == P2PMG_REC_ACTION ? 5 : 6);
    const uint32_t tb = (uint32_t)(c->cfg.n_temp_states * c->cfg.n_balance_states);
    HIP_TRY(c, p2pmg::launch_fast_rec_unpack(c->T, c->R + 1, c->A, tb, c->rec_pack, c->last.narrow, w, c->rec_stage,
                                             c->stream));
    src = c->rec_stage;
  }
  if (!src) return fail(c, P2PMG_E_STATE, "get_record: no record buffer");
  return download(c, {{host, src, bytes}});
}

// What the post-passes over the last launch's records share (p2pmg_episode_summary, p2pmg_day_profile):
// the launch recorded P2PMG_SUMMARY_RECORDS (else P2PMG_E_STATE naming what is missing), and where they lie.
static int record_params(p2pmg_ctx* c, const std::string& who, p2pmg::SummaryParams* out) {
  if (c->last.kernel.empty()) return fail(c, P2PMG_E_STATE, who + ": no episode has run (cost, grid, p2p, t_in and action records are needed)");
  const int missing = P2PMG_SUMMARY_RECORDS & ~c->last.mask;
  if (missing) {
    static const struct { int bit; const char* name; } names[] = {{P2PMG_REC_COST, "cost"}, {P2PMG_REC_GRID, "grid"},
                                                                  {P2PMG_REC_P2P, "p2p"}, {P2PMG_REC_TEMP, "t_in"},
                                                                  {P2PMG_REC_ACTION, "action"}};
    std::string list;
    for (const auto& n : names)
      if (missing & n.bit) list += (list.empty() ? "" : ", ") + std::string(n.name);
    return fail(c, P2PMG_E_STATE, who + ": the last episode launch did not record " + list);
  }
  p2pmg::SummaryParams p{};
  p.S = c->S;
  p.N = c->N;
  p.R = c->R;
  p.T = c->T;
  p.A = c->A;
  // a fast / sq16 launch packs every record it was asked for into rec_pack's rows (all of them here:
  // the narrow {reward, cost} form lacks the records checked above)
  p.packed = (c->last.packed_mask & P2PMG_SUMMARY_RECORDS) ? 1 : 0;
  p.has_reward = (c->last.mask & P2PMG_REC_REWARD) ? 1 : 0;
  p.reward = c->rec_f32[0];
  p.cost = c->rec_f32[1];
  p.grid = c->rec_f32[2];
  p.p2p = c->rec_f32[3];
  p.tin = c->rec_f32[4];
  p.action = c->rec_action;
  p.rec_pack = c->rec_pack;
  p.prof = c->prof;
  p.hp_lv = c->hp_lv;
  p.thermal = c->thermal;
  if (p.packed ? !p.rec_pack : (!p.cost || !p.grid || !p.p2p || !p.tin || !p.action || (p.has_reward && !p.reward)))
    return fail(c, P2PMG_E_STATE, who + ": no record buffer");
  *out = p;
  return P2PMG_OK;
}

int p2pmg_episode_summary(p2pmg_ctx* c, double* per_agent, double* per_scenario) {
  if (!c) return P2PMG_E_INVALID;
  if (!per_agent && !per_scenario) return fail(c, P2PMG_E_INVALID, "episode_summary: both outputs are null");
  p2pmg::SummaryParams p{};
  RC_TRY(record_params(c, "episode_summary", &p));
  const size_t A = (size_t)c->A, S = (size_t)c->S;
  if (!c->sum_agent) HIP_TRY(c, c->sum_agent.alloc(A * P2PMG_SUMMARY_FIELDS));
  if (!c->sum_scen) HIP_TRY(c, c->sum_scen.alloc(S * P2PMG_SUMMARY_FIELDS));
  p.agent_out = c->sum_agent;
  p.scen_out = c->sum_scen;
  HIP_TRY(c, p2pmg::launch_episode_summary(p, c->stream));
  if (per_agent)
    HIP_TRY(c, hipMemcpyAsync(per_agent, c->sum_agent, A * P2PMG_SUMMARY_FIELDS * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
  if (per_scenario)
    HIP_TRY(c, hipMemcpyAsync(per_scenario, c->sum_scen, S * P2PMG_SUMMARY_FIELDS * sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_day_profile_shape(p2pmg_ctx* c, const p2pmg_day_profile_args* args, int32_t* G, int32_t* P) {
  if (!c) return P2PMG_E_INVALID;
  p2pmg::DayProfRange r;
  if (const char* bad = p2pmg::dayprof_resolve(args, c->T, c->S, &r)) return fail(c, P2PMG_E_INVALID, std::string("day_profile: ") + bad);
  if (G) *G = r.G;
  if (P) *P = r.P;
  return P2PMG_OK;
}

// P2PMG_DAYPROF_TILE_BYTES, read at every call: the LDS a workgroup of dayprof_agent_kernel may use
static size_t dayprof_tile_budget() {
  const char* v = getenv("P2PMG_DAYPROF_TILE_BYTES");
  if (!v || !*v) return p2pmg::kDayProfTileDefault;
  char* end = nullptr;
  const unsigned long long n = strtoull(v, &end, 10);
  return end == v || *end ? p2pmg::kDayProfTileDefault : (size_t)n;
}

int p2pmg_day_profile(p2pmg_ctx* c, const p2pmg_day_profile_args* args, int64_t* sums, float* extrema, int64_t* com_sums,
                      float* com_extrema) {
  if (!c) return P2PMG_E_INVALID;
  if (!sums && !extrema && !com_sums && !com_extrema) return fail(c, P2PMG_E_INVALID, "day_profile: all four outputs are null");
  p2pmg::DayProfParams p{};
  RC_TRY(record_params(c, "day_profile", &p.rec));
  p2pmg::DayProfRange r;
  if (const char* bad = p2pmg::dayprof_resolve(args, c->T, c->S, &r)) return fail(c, P2PMG_E_INVALID, std::string("day_profile: ") + bad);
  const int steps = r.t1 - r.t0, scen = r.s1 - r.s0;
  const std::vector<int64_t> hist = p2pmg::dayprof_histogram(args->groups, r);
  if (const char* bad = p2pmg::dayprof_check_samples(hist.data(), r.G, steps, r.P))
    return fail(c, P2PMG_E_INVALID, std::string("day_profile: ") + bad);
  const size_t crows = (size_t)r.G * (size_t)r.P, rows = crows * (size_t)c->N;
  HIP_TRY(c, c->dp_sums.grow(rows * p2pmg::kDayProfSums));
  HIP_TRY(c, c->dp_ext.grow(rows * p2pmg::kDayProfExtrema));
  HIP_TRY(c, c->dp_csums.grow(crows * p2pmg::kDayProfComSums));
  HIP_TRY(c, c->dp_cext.grow(crows * p2pmg::kDayProfComExtrema));
  if (r.labelled) {
    HIP_TRY(c, c->dp_labels.grow((size_t)c->S));
    HIP_TRY(c, hipMemcpyAsync(c->dp_labels, args->groups, (size_t)c->S * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  p.G = r.G, p.P = r.P, p.t0 = r.t0, p.t1 = r.t1, p.s0 = r.s0, p.s1 = r.s1;
  p.labels = r.labelled ? c->dp_labels.get() : nullptr;
  if (steps > 0 && scen > 0) {
    const p2pmg::DayProfPlan plan = p2pmg::dayprof_plan(r.G, r.P, c->N, (int64_t)scen * c->N, steps, dayprof_tile_budget());
    p.lds = plan.lds, p.fold = plan.fold, p.tile_slots = plan.tile_slots, p.tile_agents = plan.tile_agents;
    p.n_tiles = plan.n_tiles, p.tiles_per_run = plan.tiles_per_run, p.slice_steps = plan.slice_steps, p.n_slices = plan.n_slices;
    p.tile_bytes = plan.tile_bytes;
  }
  p.sums = c->dp_sums, p.ext = c->dp_ext, p.com_sums = c->dp_csums, p.com_ext = c->dp_cext;
  HIP_TRY(c, p2pmg::launch_day_profile(p, c->stream));
  const struct { void* host; const void* dev; size_t bytes; } outs[] = {
      {sums, c->dp_sums, rows * p2pmg::kDayProfSums * 8}, {extrema, c->dp_ext, rows * p2pmg::kDayProfExtrema * 4},
      {com_sums, c->dp_csums, crows * p2pmg::kDayProfComSums * 8}, {com_extrema, c->dp_cext, crows * p2pmg::kDayProfComExtrema * 4}};
  for (const auto& o : outs)
    if (o.host) HIP_TRY(c, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_prepass_stats(p2pmg_ctx* c, int64_t* hits, int64_t* misses) {
  if (!c) return P2PMG_E_INVALID;
  if (hits) *hits = c->spec_hits;
  if (misses) *misses = c->spec_misses;
  return P2PMG_OK;
}

int p2pmg_set_hp_levels(p2pmg_ctx* c, const float* levels) {
  if (c) c->inputs_version++;  // invalidates the speculative pre-pass slots
  if (!c || !levels) return P2PMG_E_INVALID;
  std::vector<float4> lv((size_t)c->A);
  bool ok = true;
  for (size_t a = 0; a < lv.size(); ++a) {
    lv[a] = make_float4(levels[3 * a], levels[3 * a + 1], levels[3 * a + 2], 0.0f);
    for (int k = 0; k < 3; ++k) ok &= std::fabs(levels[3 * a + k]) <= 0x1p100f;
  }
  c->hp_bounded = ok;
  return upload(c, {{c->hp_lv, lv.data(), lv.size() * sizeof(float4)}});
}

int p2pmg_get_hp_levels(p2pmg_ctx* c, float* levels) {
  if (!c || !levels) return P2PMG_E_INVALID;
  std::vector<float4> lv((size_t)c->A);
  RC_TRY(download(c, {{lv.data(), c->hp_lv, lv.size() * sizeof(float4)}}));
  for (size_t a = 0; a < lv.size(); ++a) {
    levels[3 * a] = lv[a].x;
    levels[3 * a + 1] = lv[a].y;
    levels[3 * a + 2] = lv[a].z;
  }
  return P2PMG_OK;
}

int p2pmg_set_thermal(p2pmg_ctx* c, const float* params) {
  if (!c) return P2PMG_E_INVALID;
  const p2pmg_config& g = c->cfg;
  std::vector<float4> th((size_t)c->A, make_float4(g.setpoint, g.lower_bound, g.upper_bound, g.hp_cop));
  if (params) {
    for (size_t a = 0; a < th.size(); ++a) {
      const float* v = params + 4 * a;
      if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(v[3])))
        return fail(c, P2PMG_E_INVALID, "set_thermal: non-finite value for agent " + std::to_string(a));
      if (v[1] > v[2])
        return fail(c, P2PMG_E_INVALID, "set_thermal: lower bound above upper bound for agent " + std::to_string(a));
      th[a] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  // the step pre-pass reads none of these (it depends on the inputs and heat-pump levels only), so the
  // speculative slots stay valid
  RC_TRY(upload(c, {{c->thermal, th.data(), th.size() * sizeof(float4)}}));
  c->thermal_set = params != nullptr;
  return P2PMG_OK;
}

int p2pmg_get_thermal(p2pmg_ctx* c, float* params) {
  if (!c || !params) return P2PMG_E_INVALID;
  static_assert(sizeof(float4) == 4 * sizeof(float), "thermal rows are 4 packed floats");
  return download(c, {{params, c->thermal, (size_t)c->A * sizeof(float4)}});
}

int p2pmg_set_learning(p2pmg_ctx* c, const double* alpha, const double* gamma, const float* penalty_weight) {
  if (!c) return P2PMG_E_INVALID;
  if (c->dqn) return fail(c, P2PMG_E_UNSUPPORTED, "set_learning: tabular contexts only");
  const p2pmg_config& g = c->cfg;
  std::vector<p2pmg::LearnRow> lr((size_t)c->A, p2pmg::LearnRow{g.alpha, g.gamma, g.penalty_weight, {0.0f, 0.0f, 0.0f}});
  for (size_t a = 0; a < lr.size(); ++a) {  // validated in full before anything changes
    if (alpha) lr[a].alpha = alpha[a];
    if (gamma) lr[a].gamma = gamma[a];
    if (penalty_weight) lr[a].penw = penalty_weight[a];
    if (!(std::isfinite(lr[a].alpha) && lr[a].alpha >= 0.0 && lr[a].alpha <= 1.0))
      return fail(c, P2PMG_E_INVALID, "set_learning: alpha outside [0, 1] for agent " + std::to_string(a));
    if (!(std::isfinite(lr[a].gamma) && lr[a].gamma >= 0.0 && lr[a].gamma <= 1.0))
      return fail(c, P2PMG_E_INVALID, "set_learning: gamma outside [0, 1] for agent " + std::to_string(a));
    if (!(std::isfinite(lr[a].penw) && lr[a].penw >= 0.0f))
      return fail(c, P2PMG_E_INVALID, "set_learning: negative or non-finite penalty weight for agent " + std::to_string(a));
  }
  // no kernel's pre-pass reads these, so the speculative slots stay valid
  RC_TRY(upload(c, {{c->learn, lr.data(), lr.size() * sizeof(p2pmg::LearnRow)}}));
  c->h_learn = std::move(lr);
  c->learning_set = alpha || gamma || penalty_weight;
  return P2PMG_OK;
}

int p2pmg_get_learning(p2pmg_ctx* c, double* alpha, double* gamma, float* penalty_weight) {
  if (!c) return P2PMG_E_INVALID;
  if (c->dqn) return fail(c, P2PMG_E_UNSUPPORTED, "get_learning: tabular contexts only");
  for (size_t a = 0; a < c->h_learn.size(); ++a) {
    if (alpha) alpha[a] = c->h_learn[a].alpha;
    if (gamma) gamma[a] = c->h_learn[a].gamma;
    if (penalty_weight) penalty_weight[a] = c->h_learn[a].penw;
  }
  return P2PMG_OK;
}

int p2pmg_set_battery(p2pmg_ctx* c, const double* capacity, double min_soc, double max_soc, double efficiency,
                      const double* soc0) {
  if (!c) return P2PMG_E_INVALID;
  c->inputs_version++;  // the fast path's pre-pass writes the N = 2 round-1 bins only without a battery
  if (!capacity) {
    c->battery = false;
    return P2PMG_OK;
  }
  if (!(efficiency > 0.0) || !(min_soc <= max_soc)) return fail(c, P2PMG_E_INVALID, "set_battery: bad parameters");
  const size_t A = (size_t)c->A;
  if (!c->bat_cap) HIP_TRY(c, c->bat_cap.alloc(A));
  std::vector<double> s0(A, 0.5);
  RC_TRY(upload(c, {{c->bat_cap, capacity, A * 8}, {c->soc, soc0 ? soc0 : s0.data(), A * 8}}));
  {  // battery_rule_r<false>'s domain (see its comment in p2pmg_kernels.hip)
    auto in = [](double x, double lo, double hi) { return x >= lo && x <= hi; };
    const double se = std::sqrt(efficiency);
    bool ok = in(min_soc, 0x1p-100, 0x1p10) && in(max_soc, 0x1p-100, 0x1p10) && in(se, 0x1p-10, 0x1p10);
    for (size_t a = 0; a < A && ok; ++a) {
      ok = capacity[a] == 0.0 || in(capacity[a], 0x1p-20, 0x1p60);
      ok = ok && in(soc0 ? soc0[a] : 0.5, 0.0, 0x1p10);
    }
    c->bat_domain = ok;
  }
  c->battery = true;
  c->bat_min = min_soc;
  c->bat_max = max_soc;
  c->bat_sqrt_eff = std::sqrt(efficiency);  // np.sqrt(self.battery.efficiency), storage.py:86-100
  return P2PMG_OK;
}

int p2pmg_get_soc(p2pmg_ctx* c, double* soc) {
  if (!c || !soc) return P2PMG_E_INVALID;
  return download(c, {{soc, c->soc, (size_t)c->A * 8}});
}

}  // extern "C"
