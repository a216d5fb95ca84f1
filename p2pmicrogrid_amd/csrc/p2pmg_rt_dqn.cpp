// p2pmg_rt_dqn.cpp — the DQN learner: setup, weights, replay buffers and samples, the episode loop
// (act launch, train step, gradient exchange, Adam) and the single-batch parity calls.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "p2pmg_ctx.h"

using namespace p2pmg::rt;
using p2pmg::EpisodeParams;

namespace p2pmg::rt {

float* dqn_array(p2pmg_ctx* c, int which) {
  switch (which) {
    case P2PMG_DQN_ONLINE: return c->d_theta;
    case P2PMG_DQN_TARGET: return c->d_target;
    case P2PMG_DQN_ADAM_M: return c->d_m;
    case P2PMG_DQN_ADAM_V: return c->d_v;
    default: return nullptr;
  }
}

int dqn_ready(p2pmg_ctx* c, const char* what) {
  if (!c) return P2PMG_E_INVALID;
  if (!c->dqn || !c->d_theta) return fail(c, P2PMG_E_STATE, std::string(what) + ": p2pmg_dqn_setup first");
  return P2PMG_OK;
}

}  // namespace p2pmg::rt

namespace {

int dqn_refresh_added_min(p2pmg_ctx* c) {
  std::vector<int32_t> h(c->A);
  RC_TRY(download(c, {{h.data(), c->d_added, (size_t)c->A * 4}}));
  int64_t m = INT64_MAX;
  for (int32_t v : h) m = v < m ? v : m;
  c->d_added_min = c->A ? m : 0;
  return P2PMG_OK;
}

p2pmg::DqnParams dqn_params(p2pmg_ctx* c, const EpisodeParams& e) {
  p2pmg::DqnParams d{};
  const p2pmg_dqn_config& q = c->dcfg;
  d.e = e;
  d.n_nets = c->n_nets;
  d.theta = c->d_theta;
  d.target = c->d_target;
  d.adam_m = c->d_m;
  d.adam_v = c->d_v;
  d.grad = c->d_grad;
  d.smp = c->d_smp;
  d.segs = c->d_segs;
  d.seg_first = c->rank * c->d_seg_local;
  d.n_segs = c->nranks * c->d_seg_local;
  d.seg_agents = c->d_seg_agents;
  d.bps = c->d_bps;
  d.buf = c->d_buf;
  d.added = c->d_added;
  d.cap = q.capacity;
  d.samples = nullptr;
  d.rec_loss = (e.record & P2PMG_REC_LOSS) ? c->rec_loss : nullptr;
  d.ep_acc = c->d_ep_acc;
  // row 0: every row when they are equal, and what the shared network's kernels read
  const p2pmg::DqnLearn& r0 = c->h_dlearn[0];
  d.gamma = (float)r0.gamma;
  d.tau = (float)r0.tau;
  d.tau_c = 1.0f - (float)r0.tau;
  d.b1c = 1.0f - (float)q.beta1;
  d.b2c = 1.0f - (float)q.beta2;
  d.adam_eps = (float)q.adam_eps;
  d.clip = (float)r0.clip;
  d.hyp = c->d_hyp_mixed ? c->d_hyp.get() : nullptr;
  d.penw = c->d_penw;
  d.roles = c->dqn_roles ? c->N : 0;
  // the mean's divisor: every agent of every rank for the shared network, a role's S agents on a role context
  d.inv_agents = 1.0f / (float)(c->dqn_roles ? (double)c->S : (double)c->A * c->nranks);
  d.apb = c->d_apb;
  d.theta_out = d.theta;  // the Adam steps store in place unless the episode loop binds the double buffer
  d.target_out = d.target;
  d.m_out = d.adam_m;
  d.v_out = d.adam_v;
  d.adam_pending = 0;
  d.fold_spt = 0;  // auto (launch_dqn_reduce_adam)
  d.adam_tpb = 256;
  return d;
}

// the network state an Adam step reads (in) and writes (out): online, target, m, v
void dqn_bind(p2pmg::DqnParams& d, float* const in[4], float* const out[4]) {
  d.theta = in[0];
  d.target = in[1];
  d.adam_m = in[2];
  d.adam_v = in[3];
  d.theta_out = out[0];
  d.target_out = out[1];
  d.m_out = out[2];
  d.v_out = out[3];
}

// Keras Adam step size for iteration `step` (1-based), float64 -> float32 (oracle/dqn.py::adam_lr)
// at the network's own learning rate lr
float adam_lr(const p2pmg_dqn_config& q, double lr, int64_t step) {
  const double t = (double)step;
  return (float)(lr * std::sqrt(1.0 - std::pow(q.beta2, t)) / (1.0 - std::pow(q.beta1, t)));
}

// every network takes the same Adam step size: the iteration counts the same and lr the same
bool dqn_steps_same(const p2pmg_ctx* c) {
  for (int64_t st : c->d_steps)
    if (st != c->d_steps[0]) return false;
  return !c->d_lr_mixed;
}

// h_dlearn / h_penw to the device, and what the rows have in common
int dqn_upload_learning(p2pmg_ctx* c) {
  std::vector<float4> hyp(c->h_dlearn.size());
  c->d_hyp_mixed = c->d_lr_mixed = false;
  for (size_t k = 0; k < hyp.size(); ++k) {
    const p2pmg::DqnLearn& r = c->h_dlearn[k];
    hyp[k] = make_float4((float)r.gamma, (float)r.tau, 1.0f - (float)r.tau, (float)r.clip);
    if (std::memcmp(&hyp[k], &hyp[0], sizeof(float4)) != 0) c->d_hyp_mixed = true;
    if (r.lr != c->h_dlearn[0].lr) c->d_lr_mixed = true;
  }
  return upload(c, {{c->d_hyp, hyp.data(), hyp.size() * sizeof(float4)}, {c->d_penw, c->h_penw.data(), c->h_penw.size() * 4}});
}

// p2pmg_dqn_train_batch advanced some networks on their own, so their Adam step counts differ, or
// p2pmg_dqn_set_learning gave them different learning rates.
// Every env step advances every network by one, so an episode's per-network step sizes are known
// up front: one [T][n_nets] table, uploaded once per episode (not a copy + sync per env step).
int dqn_upload_lr_table(p2pmg_ctx* c) {
  const size_t n = c->d_steps.size(), need = (size_t)c->T * n;
  HIP_TRY(c, c->d_lr.grow(need));
  c->h_lr.resize(need);
  for (int t = 0; t < c->T; ++t)
    for (size_t k = 0; k < n; ++k) c->h_lr[(size_t)t * n + k] = adam_lr(c->dcfg, c->h_dlearn[k].lr, c->d_steps[k] + 1 + t);
  return upload(c, {{c->d_lr, c->h_lr.data(), need * 4}});  // synced: h_lr is rewritten by the next such episode
}

// The shared network's gradient segments of every rank in d_segs ([nranks * d_seg_local][kNetStride]),
// allocated for the current world (comm_init / set_exchange may come after dqn_setup)
int dqn_ensure_segs(p2pmg_ctx* c, p2pmg::DqnParams& d) {
  const size_t need = (size_t)c->nranks * c->d_seg_local * p2pmg::kNetStride;
  HIP_TRY(c, c->d_segs.grow(need));
  if (c->xfn && !c->comm) HIP_TRY(c, c->h_segs.grow(need));
  d.segs = c->d_segs;
  d.seg_first = c->rank * c->d_seg_local;
  d.n_segs = c->nranks * c->d_seg_local;
  return P2PMG_OK;
}

// every rank's segments into d_segs: RCCL all-gather in place (xGMI), or the host exchange function
int dqn_gather_segments(p2pmg_ctx* c) {
  const size_t per = (size_t)c->d_seg_local * p2pmg::kNetStride;  // floats per rank
  if (c->comm) {
    Rccl* r = rccl();
    if (!r->allGather) return fail(c, P2PMG_E_UNSUPPORTED, "ncclAllGather not found");
    // ncclFloat32 = 7; in place: this rank's part already sits at d_segs + rank * per
    HIP_TRY(c, coll_mark(c, 0));
    const int rc = r->allGather(c->d_segs + (size_t)c->rank * per, c->d_segs, per, 7, c->comm, c->stream);
    if (rc != 0) return fail(c, P2PMG_E_HIP, std::string("dqn gradient all-gather: ") +
                                                 (r->getErrorString ? r->getErrorString(rc) : "?"));
    HIP_TRY(c, coll_mark(c, 1));
    return P2PMG_OK;
  }
  if (!c->xfn) return fail(c, P2PMG_E_STATE, "dqn: several ranks but neither a communicator nor an exchange");
  float* own = c->h_segs + (size_t)c->rank * per;
  RC_TRY(download(c, {{own, c->d_segs + (size_t)c->rank * per, per * 4}}));
  if (c->xfn(c->xuser, c->h_segs, (int64_t)per, c->rank, c->nranks) != 0)
    return fail(c, P2PMG_E_STATE, "dqn: the host gradient exchange failed");
  return upload(c, {{c->d_segs, c->h_segs, (size_t)c->nranks * per * 4}});  // synced: h_segs is rewritten by the next env step
}

// defer (the shared network's split path, act kernel able to fuse it): the post-exchange Adam step is
// left pending (d.adam_pending) for the next env step's act launch, or the episode loop's settle
int dqn_train_step(p2pmg_ctx* c, p2pmg::DqnParams& d, bool same, bool defer) {
  // one env step trains every network once (community.py:158-168); the Adam step counters advance
  // only once every launch of the step is enqueued (a failed exchange leaves weights and counters
  // at the previous step: the Adam launch that would change the weights was not issued)
  d.lr_t = adam_lr(c->dcfg, c->h_dlearn[0].lr, c->d_steps[0] + 1);
  d.lr_net = same ? nullptr : c->d_lr + (size_t)d.t * c->d_steps.size();
  if (!d.fused_sample) HIP_TRY(c, p2pmg::launch_dqn_sample(d, c->stream));
  if (c->dqn_roles) {  // N networks: each role's partials, then every role's sum + Adam in one launch
    HIP_TRY(c, p2pmg::launch_dqn_train_roles(d, c->stream));
    HIP_TRY(c, p2pmg::launch_dqn_reduce_adam_roles(d, c->stream));
  } else if (c->n_nets == 1) {
    HIP_TRY(c, p2pmg::launch_dqn_train(d, c->d_blocks, true, c->stream));
    if (c->nranks == 1 && c->d_seg_local == 1) {  // one segment in all: its sum + Adam in one launch
      HIP_TRY(c, p2pmg::launch_dqn_reduce_adam(d, 1, true, c->stream));
    } else {
      HIP_TRY(c, p2pmg::launch_dqn_reduce_adam(d, c->d_seg_local, false, c->stream));
      if (c->nranks > 1 || c->comm) {  // a communicator gathers even at world 1 (the RCCL path, tested)
        RC_TRY(dqn_gather_segments(c));
      }
      if (defer) d.adam_pending = 1;
      else HIP_TRY(c, p2pmg::launch_dqn_adam_shared(d, c->stream));
    }
  } else {
    HIP_TRY(c, p2pmg::launch_dqn_train(d, c->A, false, c->stream));
  }
  for (auto& st : c->d_steps) ++st;
  return P2PMG_OK;
}

}  // namespace

int p2pmg::rt::dqn_run_episode(p2pmg_ctx* c, const p2pmg_episode_args* args) {
  RC_TRY(dqn_ready(c, "run_episode"));
  const int mode = args->mode;
  if (mode != P2PMG_MODE_TRAIN && mode != P2PMG_MODE_GREEDY && mode != P2PMG_MODE_FILL)
    return fail(c, P2PMG_E_INVALID, "mode");
  const bool acting = mode != P2PMG_MODE_GREEDY;
  if (acting && args->rng != P2PMG_RNG_REPLAY && args->rng != P2PMG_RNG_PHILOX) return fail(c, P2PMG_E_INVALID, "rng");
  if (acting && args->rng == P2PMG_RNG_REPLAY && !c->have_codes)
    return fail(c, P2PMG_E_STATE, "run_episode: replay mode needs p2pmg_set_replay_codes");
  if (mode == P2PMG_MODE_TRAIN && args->rng == P2PMG_RNG_REPLAY && !c->have_samples)
    return fail(c, P2PMG_E_STATE, "run_episode: DQN replay training needs p2pmg_dqn_set_samples");
  if (mode == P2PMG_MODE_TRAIN && c->d_added_min + 1 < p2pmg::kDqnBatch)
    return fail(c, P2PMG_E_STATE, "run_episode: fill the replay memory first (>= 31 transitions per agent, "
                                  "community.init_buffers)");
  RC_TRY(ensure_records(c, args->record));
  EpisodeParams e = episode_params(c, args);
  e.rng = (acting && args->rng == P2PMG_RNG_PHILOX) ? 1 : 0;
  p2pmg::DqnParams d = dqn_params(c, e);
  if (mode == P2PMG_MODE_TRAIN && args->rng == P2PMG_RNG_REPLAY) d.samples = c->d_samples;
  if (mode == P2PMG_MODE_TRAIN && c->n_nets == 1 && (c->nranks > 1 || c->d_seg_local > 1)) {
    RC_TRY(dqn_ensure_segs(c, d));
  }
  d.fused_sample = (mode == P2PMG_MODE_TRAIN) ? 1 : 0;  // the act launch of each env step draws the samples
  {  // P2PMG_DQN_ACT=wave: the one-wave-per-agent act kernel for a shared network too (tests, A/B)
    const char* v = getenv("P2PMG_DQN_ACT");
    d.act_wave = (v && !strcmp(v, "wave")) ? 1 : 0;
    const char* g = getenv("P2PMG_ACT_AGW");  // 8: the 8-slot MFMA act workgroups (tests, A/B)
    d.act_agw = (g && atoi(g) == 8) ? 8 : 16;
    const char* f = getenv("P2PMG_FOLD_SPT");  // segment fold runs per thread: 1, 2, 4, 8, 16 (A/B); else auto
    const int fs = f ? atoi(f) : 0;
    d.fold_spt = (fs == 1 || fs == 2 || fs == 4 || fs == 8 || fs == 16) ? fs : 0;
    const char* at = getenv("P2PMG_ADAM_TPB");  // post-exchange Adam workgroup size: 64, 128, 256 (default)
    d.adam_tpb = at ? atoi(at) : 256;
  }
  const bool same = mode != P2PMG_MODE_TRAIN || dqn_steps_same(c);
  if (!same) {
    RC_TRY(dqn_upload_lr_table(c));
  }
  // The shared network's split path (segments / ranks): env step t's post-exchange Adam step runs
  // inside env step t + 1's act launch, which reads the state from one half of a double buffer and
  // stores the stepped state into the other (every act workgroup needs the new weights; workgroup 0
  // stores them); the episode's last step, or any early return, settles into the primary arrays.
  // Opt-in (P2PMG_DQN_ADAM=act): measured on the MI355X the fused form costs the act launch far more
  // than the standalone Adam launch it saves, so the default is that launch.
  const char* adam_env = getenv("P2PMG_DQN_ADAM");
  const bool defer = mode == P2PMG_MODE_TRAIN && c->n_nets == 1 && (c->nranks > 1 || c->d_seg_local > 1) &&
                     c->d_alt && p2pmg::dqn_act_fuses_adam(d) && adam_env && !strcmp(adam_env, "act");
  const size_t NS = p2pmg::kNetStride;
  float* const prim[4] = {c->d_theta, c->d_target, c->d_m, c->d_v};
  float* const alt[4] = {c->d_alt, c->d_alt + NS, c->d_alt + 2 * NS, c->d_alt + 3 * NS};
  bool on_alt = false;  // the current state sits in the alt half
  auto settle = [&]() -> int {
    float* const* cur = on_alt ? alt : prim;
    if (d.adam_pending) {  // the pending step, from the current half into the primary arrays
      dqn_bind(d, cur, prim);
      d.adam_pending = 0;
      HIP_TRY(c, p2pmg::launch_dqn_adam_shared(d, c->stream));
    } else if (on_alt) {
      for (int k = 0; k < 4; ++k)
        HIP_TRY(c, hipMemcpyAsync(prim[k], alt[k], NS * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    on_alt = false;
    dqn_bind(d, prim, prim);
    return P2PMG_OK;
  };
  Timed tm;
  RC_TRY(begin_timed(c, false, true, &tm));
  // Philox training: every env step's replay draws in one throughput launch ahead of the episode,
  // read by the act launches like uploaded samples (P2PMG_DQN_SAMPLE_PREPASS=0: drawn in each act
  // launch's tail, as the episode's first form did)
  {
    const char* px_env = getenv("P2PMG_DQN_SAMPLE_PREPASS");
    const bool no_px = px_env && !strcmp(px_env, "0");
    const size_t n = (size_t)c->T * c->A * p2pmg::kDqnBatch;
    if (mode == P2PMG_MODE_TRAIN && args->rng == P2PMG_RNG_PHILOX && !no_px && n <= ((size_t)1 << 30)) {
      if (!c->d_samples_px) HIP_TRY(c, c->d_samples_px.alloc(n));
      HIP_TRY(c, p2pmg::launch_dqn_sample_prepass(d, c->d_samples_px, c->stream));
      d.samples = c->d_samples_px;
    }
  }
  for (int t = 0; t < c->T; ++t) {
    d.t = t;
    d.e.mode = mode;
    if (d.adam_pending) dqn_bind(d, on_alt ? alt : prim, on_alt ? prim : alt);
    const hipError_t e = p2pmg::launch_dqn_act(d, c->stream);
    if (e != hipSuccess) {
      (void)settle();
      return fail(c, P2PMG_E_HIP, std::string("dqn act launch: ") + hipGetErrorString(e));
    }
    if (d.adam_pending) {  // applied: the stepped state is the current one
      on_alt = !on_alt;
      d.adam_pending = 0;
      dqn_bind(d, on_alt ? alt : prim, on_alt ? alt : prim);
    }
    if (mode == P2PMG_MODE_TRAIN) {
      const int rc = dqn_train_step(c, d, same, defer);
      if (rc != P2PMG_OK) {
        (void)settle();
        return rc;
      }
    }
  }
  RC_TRY(settle());
  RC_TRY(end_timed(c, tm, true));
  finish_launch(c, tm, std::string(c->n_nets == 1 && !c->dqn_roles && !d.act_wave ? "dqn_act_shared_kernel<" : "dqn_act_kernel<") +
                           std::to_string(c->N) + (c->dqn_roles ? ",roles>" : ">"), args->record, 0, 0);
  if (acting) c->d_added_min += c->T;
  if (acting && args->rng == P2PMG_RNG_REPLAY) c->have_codes = c->code_src == 1;
  return P2PMG_OK;
}

namespace {

// p2pmg_dqn_setup, and p2pmg_dqn_setup_roles (roles: N networks, every argument checked by validate_dqn_roles)
int dqn_setup_impl(p2pmg_ctx* c, const p2pmg_dqn_config* cfg, bool roles) {
  if (!c || !cfg) return P2PMG_E_INVALID;
  if (!c->dqn) return fail(c, P2PMG_E_STATE, "dqn_setup: create the context with learner = P2PMG_LEARNER_DQN");
  if (cfg->batch != p2pmg::kDqnBatch) return fail(c, P2PMG_E_UNSUPPORTED, "dqn_setup: batch must be 32");
  if (cfg->capacity < p2pmg::kDqnBatch || cfg->capacity > 65535)
    return fail(c, P2PMG_E_INVALID, "dqn_setup: capacity must be in [32, 65535]");
  if (c->d_theta) return fail(c, P2PMG_E_STATE, "dqn_setup: already set up");
  c->dcfg = *cfg;
  const size_t A = (size_t)c->A, NS = p2pmg::kNetStride;
  c->n_nets = roles ? c->N : (c->cfg.shared_q ? 1 : c->A);
  const size_t nn = (size_t)c->n_nets * NS;
  for (DevBuf<float>* b : {&c->d_theta, &c->d_target, &c->d_m, &c->d_v}) HIP_TRY(c, b->alloc(nn));
  for (DevBuf<float>* b : {&c->d_theta, &c->d_target, &c->d_m, &c->d_v})
    HIP_TRY(c, hipMemsetAsync(b->get(), 0, nn * 4, c->stream));
  if (cfg->agents_per_block < 0 || cfg->grad_segments < 0) return fail(c, P2PMG_E_INVALID, "dqn_setup: negative layout");
  if (roles) {
    // per role: its S agents in blocks of apb consecutive scenarios, one partial each; N * d_bps train
    // workgroups in all, so the automatic apb fills one wave of workgroups as the shared network's does
    const size_t slots = (size_t)c->n_cu * (size_t)p2pmg::dqn_train_blocks_per_cu();
    const int apb = cfg->agents_per_block > 0 ? cfg->agents_per_block : (int)((A + slots - 1) / slots);
    c->d_apb = apb < 1 ? 1 : apb;
    c->d_seg_local = 1;
    c->d_seg_agents = c->A;
    c->d_bps = (c->S + c->d_apb - 1) / c->d_apb;
    c->d_blocks = c->N * c->d_bps;
    HIP_TRY(c, c->d_grad.alloc((size_t)c->d_blocks * NS));
    std::vector<int32_t> map(A);
    for (int a = 0; a < c->A; ++a) map[(size_t)a] = a % c->N;
    HIP_TRY(c, c->d_role_map.alloc(A));
    RC_TRY(upload(c, {{c->d_role_map.get(), map.data(), A * sizeof(int32_t)}}));
    c->dqn_roles = true;
  } else if (c->cfg.shared_q) {
    // gradient segments: contiguous runs of whole scenarios; the train workgroups never straddle two
    const int G = cfg->grad_segments > 0 ? cfg->grad_segments : 1;
    if (c->S % G) return fail(c, P2PMG_E_INVALID, "dqn_setup: grad_segments must divide the scenarios");
    c->d_seg_local = G;
    c->d_seg_agents = c->A / G;
    // default: one wave of train workgroups (2 per CU in the default build: 512 on 256 CUs)
    const size_t slots = (size_t)c->n_cu * (size_t)p2pmg::dqn_train_blocks_per_cu();
    int apb = cfg->agents_per_block > 0 ? cfg->agents_per_block : (int)((A + slots - 1) / slots);
    c->d_apb = apb < 1 ? 1 : apb;
    c->d_bps = (c->d_seg_agents + c->d_apb - 1) / c->d_apb;
    c->d_blocks = G * c->d_bps;
    HIP_TRY(c, c->d_grad.alloc((size_t)c->d_blocks * NS));
    HIP_TRY(c, c->d_alt.alloc(4 * NS));
  } else {
    c->d_apb = 1;
    c->d_blocks = c->A;
    c->d_seg_local = 1;
    c->d_seg_agents = c->A;
    c->d_bps = c->A;
  }
  HIP_TRY(c, c->d_buf.alloc(A * (size_t)cfg->capacity * p2pmg::kTrans));
  HIP_TRY(c, c->d_added.alloc(A));
  HIP_TRY(c, c->d_smp.alloc(A * p2pmg::kDqnBatch));
  HIP_TRY(c, hipMemsetAsync(c->d_added, 0, A * 4, c->stream));
  HIP_TRY(c, c->d_ep_acc.alloc((size_t)c->S));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->d_steps.assign((size_t)c->n_nets, 0);
  c->d_added_min = 0;
  HIP_TRY(c, c->d_hyp.alloc((size_t)c->n_nets));
  HIP_TRY(c, c->d_penw.alloc(A));
  c->h_dlearn.assign((size_t)c->n_nets, p2pmg::DqnLearn{cfg->gamma, cfg->tau, cfg->lr, cfg->clip});
  c->h_penw.assign(A, c->cfg.penalty_weight);
  return dqn_upload_learning(c);
}

}  // namespace

extern "C" {

int p2pmg_dqn_setup(p2pmg_ctx* c, const p2pmg_dqn_config* cfg) { return dqn_setup_impl(c, cfg, false); }

int p2pmg_dqn_setup_roles(p2pmg_ctx* c, const p2pmg_dqn_config* cfg) {
  if (!c || !cfg) return P2PMG_E_INVALID;
  std::string why;
  const int rc = p2pmg::validate_dqn_roles(&c->cfg, cfg, c->d_theta.get() != nullptr, c->nranks, c->comm != nullptr, &why);
  if (rc != P2PMG_OK) return fail(c, rc, why);
  return dqn_setup_impl(c, cfg, true);
}

int p2pmg_dqn_roles(p2pmg_ctx* c, int* n_roles) {
  if (!c || !n_roles) return P2PMG_E_INVALID;
  *n_roles = c->dqn_roles ? c->N : 0;
  return P2PMG_OK;
}

int p2pmg_dqn_set_learning(p2pmg_ctx* c, const double* gamma, const double* tau, const double* lr, const double* clip,
                           const float* penalty_weight) {
  if (!c) return P2PMG_E_INVALID;
  if (!c->dqn || !c->d_theta) return fail(c, P2PMG_E_STATE, "dqn_set_learning: a DQN context after p2pmg_dqn_setup");
  const bool restore = !gamma && !tau && !lr && !clip && !penalty_weight;
  const p2pmg_dqn_config& q = c->dcfg;
  std::vector<p2pmg::DqnLearn> rows = c->h_dlearn;
  std::vector<float> penw = c->h_penw;
  if (restore) {
    rows.assign(rows.size(), p2pmg::DqnLearn{q.gamma, q.tau, q.lr, q.clip});
    penw.assign(penw.size(), c->cfg.penalty_weight);
  }
  for (size_t k = 0; k < rows.size(); ++k) {
    if (gamma) rows[k].gamma = gamma[k];
    if (tau) rows[k].tau = tau[k];
    if (lr) rows[k].lr = lr[k];
    if (clip) rows[k].clip = clip[k];
  }
  if (penalty_weight) std::copy(penalty_weight, penalty_weight + penw.size(), penw.begin());
  std::string why;  // validated in full before anything changes
  if (!restore && p2pmg::validate_dqn_learning(rows.data(), (int)rows.size(), penw.data(), (int)penw.size(), &why) != P2PMG_OK)
    return fail(c, P2PMG_E_INVALID, why);
  std::swap(c->h_dlearn, rows);
  std::swap(c->h_penw, penw);
  const int rc = dqn_upload_learning(c);
  if (rc != P2PMG_OK) {  // the upload failed: the host copies go back too
    std::swap(c->h_dlearn, rows);
    std::swap(c->h_penw, penw);
    (void)dqn_upload_learning(c);
  }
  return rc;
}

int p2pmg_dqn_get_learning(p2pmg_ctx* c, double* gamma, double* tau, double* lr, double* clip, float* penalty_weight) {
  if (!c) return P2PMG_E_INVALID;
  if (!c->dqn || !c->d_theta) return fail(c, P2PMG_E_STATE, "dqn_get_learning: a DQN context after p2pmg_dqn_setup");
  for (size_t k = 0; k < c->h_dlearn.size(); ++k) {
    if (gamma) gamma[k] = c->h_dlearn[k].gamma;
    if (tau) tau[k] = c->h_dlearn[k].tau;
    if (lr) lr[k] = c->h_dlearn[k].lr;
    if (clip) clip[k] = c->h_dlearn[k].clip;
  }
  if (penalty_weight) std::copy(c->h_penw.begin(), c->h_penw.end(), penalty_weight);
  return P2PMG_OK;
}

int p2pmg_dqn_run_episode_eps(p2pmg_ctx* c, const p2pmg_episode_args* args, const double* eps) {
  if (!c || !args || !eps) return P2PMG_E_INVALID;
  if (!c->dqn || !c->d_theta) return fail(c, P2PMG_E_STATE, "dqn_run_episode_eps: a DQN context after p2pmg_dqn_setup");
  if ((args->mode != P2PMG_MODE_TRAIN && args->mode != P2PMG_MODE_FILL) || args->rng != P2PMG_RNG_PHILOX)
    return fail(c, P2PMG_E_INVALID, "dqn_run_episode_eps: Philox train or fill episodes only (replay codes carry each "
                                    "agent's own decision, a greedy episode draws none)");
  const size_t S = (size_t)c->S;
  std::vector<uint2> tab(S);
  for (size_t s = 0; s < S; ++s) {
    if (!(std::isfinite(eps[s]) && eps[s] >= 0.0 && eps[s] <= 1.0))
      return fail(c, P2PMG_E_INVALID, "dqn_run_episode_eps: epsilon outside [0, 1] for scenario " + std::to_string(s));
    int all = 0;
    p2pmg::eps_threshold(eps[s], tab[s].x, all);
    tab[s].y = (uint32_t)all;
  }
  HIP_TRY(c, c->eps_tab.grow(S));
  RC_TRY(upload(c, {{c->eps_tab, tab.data(), S * sizeof(uint2)}}));
  c->chain_n = 0;
  c->eps_table = true;  // episode_params binds the row (EpisodeParams::eps_tab)
  c->eps_cur = c->eps_tab;
  p2pmg_episode_args a = *args;
  a.epsilon = eps[0];
  const int rc = dqn_run_episode(c, &a);
  c->eps_table = false;
  c->eps_cur = nullptr;
  return rc;
}

int p2pmg_dqn_set_weights(p2pmg_ctx* c, int which, int first, int count, const float* host) {
  RC_TRY(dqn_ready(c, "dqn_set_weights"));
  float* dst = dqn_array(c, which);
  if (!dst || !host || first < 0 || count < 0 || first + count > c->n_nets)
    return fail(c, P2PMG_E_INVALID, "dqn_set_weights: bad array/range");
  HIP_TRY(c, hipMemcpy2DAsync(dst + (size_t)first * p2pmg::kNetStride, p2pmg::kNetStride * 4, host,
                              p2pmg::kDqnParams * 4, p2pmg::kDqnParams * 4, count, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_dqn_get_weights(p2pmg_ctx* c, int which, int first, int count, float* host) {
  RC_TRY(dqn_ready(c, "dqn_get_weights"));
  const float* src = dqn_array(c, which);
  if (!src || !host || first < 0 || count < 0 || first + count > c->n_nets)
    return fail(c, P2PMG_E_INVALID, "dqn_get_weights: bad array/range");
  HIP_TRY(c, hipMemcpy2DAsync(host, p2pmg::kDqnParams * 4, src + (size_t)first * p2pmg::kNetStride,
                              p2pmg::kNetStride * 4, p2pmg::kDqnParams * 4, count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_dqn_set_step(p2pmg_ctx* c, int64_t step) {
  RC_TRY(dqn_ready(c, "dqn_set_step"));
  if (step < 0) return P2PMG_E_INVALID;
  std::fill(c->d_steps.begin(), c->d_steps.end(), step);  // every network
  return P2PMG_OK;
}

int p2pmg_dqn_get_step(p2pmg_ctx* c, int64_t* step) {
  RC_TRY(dqn_ready(c, "dqn_get_step"));
  if (!step) return P2PMG_E_INVALID;
  *step = c->d_steps[0];
  return P2PMG_OK;
}

int p2pmg_dqn_get_net_steps(p2pmg_ctx* c, int first, int count, int64_t* steps) {
  RC_TRY(dqn_ready(c, "dqn_get_net_steps"));
  if (!steps || first < 0 || count < 0 || first + count > c->n_nets) return fail(c, P2PMG_E_INVALID, "dqn_get_net_steps");
  for (int k = 0; k < count; ++k) steps[k] = c->d_steps[(size_t)first + k];
  return P2PMG_OK;
}

int p2pmg_dqn_set_samples(p2pmg_ctx* c, const uint16_t* samples) {
  RC_TRY(dqn_ready(c, "dqn_set_samples"));
  if (!samples) return P2PMG_E_INVALID;
  const size_t n = (size_t)c->T * c->A * p2pmg::kDqnBatch;
  if (!c->d_samples) HIP_TRY(c, c->d_samples.alloc(n));
  RC_TRY(upload(c, {{c->d_samples, samples, n * 2}}));
  c->have_samples = true;
  return P2PMG_OK;
}

int p2pmg_dqn_get_buffer(p2pmg_ctx* c, int first, int count, float* host, int32_t* added) {
  RC_TRY(dqn_ready(c, "dqn_get_buffer"));
  if (first < 0 || count < 0 || first + count > c->A) return fail(c, P2PMG_E_INVALID, "dqn_get_buffer: range");
  const size_t per = (size_t)c->dcfg.capacity * p2pmg::kTrans;
  if (host)
    HIP_TRY(c, hipMemcpyAsync(host, c->d_buf + (size_t)first * per, (size_t)count * per * 4, hipMemcpyDeviceToHost,
                              c->stream));
  if (added)
    HIP_TRY(c, hipMemcpyAsync(added, c->d_added + first, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_dqn_set_buffer(p2pmg_ctx* c, int first, int count, const float* host, const int32_t* added) {
  RC_TRY(dqn_ready(c, "dqn_set_buffer"));
  if (first < 0 || count < 0 || first + count > c->A) return fail(c, P2PMG_E_INVALID, "dqn_set_buffer: range");
  const size_t per = (size_t)c->dcfg.capacity * p2pmg::kTrans;
  if (host)
    HIP_TRY(c, hipMemcpyAsync(c->d_buf + (size_t)first * per, host, (size_t)count * per * 4, hipMemcpyHostToDevice,
                              c->stream));
  if (added)
    HIP_TRY(c, hipMemcpyAsync(c->d_added + first, added, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return dqn_refresh_added_min(c);
}

int p2pmg_dqn_forward(p2pmg_ctx* c, int net, int n, const float* x, float* q) {
  RC_TRY(dqn_ready(c, "dqn_forward"));
  if (net < 0 || net >= c->n_nets || n < 0 || (n > 0 && (!x || !q))) return fail(c, P2PMG_E_INVALID, "dqn_forward");
  if (n == 0) return P2PMG_OK;
  DevBuf<float> dx, dq;
  HIP_TRY(c, dx.alloc((size_t)n * 5));
  hipError_t e = dq.alloc((size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(dx, x, (size_t)n * 20, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = p2pmg::launch_dqn_forward(c->d_theta + (size_t)net * p2pmg::kNetStride, n, dx, dq, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(q, dq, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("dqn_forward: ") + hipGetErrorString(e));
  return P2PMG_OK;
}

int p2pmg_dqn_train_batch(p2pmg_ctx* c, int net, const float* batch, float* loss) {
  RC_TRY(dqn_ready(c, "dqn_train_batch"));
  if (net < 0 || net >= c->n_nets || !batch) return fail(c, P2PMG_E_INVALID, "dqn_train_batch");
  DevBuf<float> db;
  HIP_TRY(c, db.alloc((size_t)p2pmg::kDqnBatch * p2pmg::kTrans + 1));
  p2pmg_episode_args args{P2PMG_MODE_TRAIN, P2PMG_RNG_PHILOX, 0, 0, 0.0, 0, 0};
  p2pmg::DqnParams d = dqn_params(c, episode_params(c, &args));
  d.batch = db;
  d.net = net;
  d.loss_out = db + p2pmg::kDqnBatch * p2pmg::kTrans;
  d.lr_t = adam_lr(c->dcfg, c->h_dlearn[(size_t)net].lr, ++c->d_steps[(size_t)net]);  // only this network's Adam iterates
  hipError_t e = hipMemcpyAsync(db, batch, (size_t)p2pmg::kDqnBatch * p2pmg::kTrans * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = p2pmg::launch_dqn_train(d, 1, false, c->stream);
  float l = 0.0f;
  if (e == hipSuccess) e = hipMemcpyAsync(&l, d.loss_out, 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("dqn_train_batch: ") + hipGetErrorString(e));
  if (loss) *loss = l;
  return P2PMG_OK;
}

int p2pmg_dqn_grad_layout(p2pmg_ctx* c, int* segments, int* agents_per_block, int* blocks) {
  RC_TRY(dqn_ready(c, "dqn_grad_layout"));
  if (segments) *segments = c->d_seg_local;
  if (agents_per_block) *agents_per_block = c->d_apb;
  if (blocks) *blocks = c->d_blocks;
  return P2PMG_OK;
}

}  // extern "C"
