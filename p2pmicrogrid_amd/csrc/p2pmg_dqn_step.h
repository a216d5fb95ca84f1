// p2pmg_dqn_step.h — the pieces of one DQN env step that more than one DQN unit needs
// (p2pmg_dqn_act.hip, p2pmg_dqn_act_shared.hip, p2pmg_dqn_train.hip, p2pmg_dqn_shared.hip, p2pmg_dqn_eval.hip): the batch
// size, the replay sample draw, the act kernels' replayed codes and settlement, the one Adam / soft-update
// rounding sequence (bit for bit oracle/dqn.py's) with the shared network's post-exchange step, and the
// trace builds' phase stamp.  Included inside the including unit's anonymous namespace, after
// p2pmg_device.h and p2pmg_dqn_ops.h.
constexpr int kB = kDqnBatch;

// timing-only probe (-DP2PMG_TRACE, scripts/gpu_dqn_trace.sh): adds the s_memtime cycles since `last`
// to phase k of the kernel's `acc` array
#ifndef P2PMG_TRACE
#define P2PMG_TRACE 0
#endif
#if P2PMG_TRACE
#define P2PMG_STAMP(acc, last, k)                                                \
  do {                                                                           \
    uint64_t t_;                                                                 \
    asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
    acc[k] += t_ - last;                                                         \
    last = t_;                                                                   \
  } while (0)
#else
#define P2PMG_STAMP(acc, last, k) \
  do {                            \
  } while (0)
#endif

// replay mode's exploration codes of env step t (EpisodeParams::codes, [T][W][A] words): agent a's
// word w4 (rounds 4 w4 .. 4 w4 + 3), and round r's byte of it (255 = greedy)
__device__ __forceinline__ uint32_t replay_word(const EpisodeParams& p, int t, int W, size_t A, int w4, int a) {
  return p.codes[((size_t)t * W + w4) * A + a];
}
__device__ __forceinline__ int replay_code(const EpisodeParams& p, int t, int W, size_t A, int r, int a) {
  return (int)((replay_word(p, t, W, A, r >> 2, a) >> (8 * (r & 3))) & 0xFFu);
}

// _compute_costs community.py:56-65; RLAgent.get_reward agent.py:225-232 (pre-update T_in) from the
// agent's grid and p2p power, its thermal {setpoint, lower, upper, cop} and its own comfort weight penw
// (DqnParams::penw / DqnEvalParams::penw, p2pmg_dqn_set_learning)
struct Settled {
  float cost, rw;
};
__device__ __forceinline__ Settled settle(const EpisodeParams& p, float gg, float pp, float buy, float inj, float p2pp,
                                          float tin, float4 thermal, float penw) {
  float cost = (gg >= 0.0f) ? gg * buy : gg * inj;
  cost = cost + pp * p2pp;
  cost = (cost * p.slot) / p.mph;
  cost = cost * p.kilo;
  float pen = fmaxf(fmaxf(0.0f, thermal.y - tin), fmaxf(0.0f, tin - thermal.z));
  pen = pen > 0.0f ? pen + 1.0f : 0.0f;
  return Settled{cost, -(cost + penw * pen)};
}

// Keras Adam (beta1 .9, beta2 .999, eps 1e-7; rl.py:335-354) on one parameter, Trainer._soft_update, and
// the shared network's gradient: the mean over every agent of every rank, the first kernel clipped
struct AdamStep {
  float m, v, w;
};
__device__ __forceinline__ AdamStep adam_step(const DqnParams& d, float m, float v, float w, float g, float lr) {
  m = m + (g - m) * d.b1c;
  v = v + (g * g - v) * d.b2c;
  w = w - (m * lr) / (sqrtf(v) + d.adam_eps);
  return AdamStep{m, v, w};
}
__device__ __forceinline__ float soft_update(float tau, float tau_c, float tg, float w) { return tau_c * tg + tau * w; }
__device__ __forceinline__ float soft_update(const DqnParams& d, float tg, float w) { return soft_update(d.tau, d.tau_c, tg, w); }
// the exploration thresholds of scenario s: the launch's scalars, or the scenario's own pair of the
// per-scenario table (p2pmg_dqn_run_episode_eps), {thr, all} as eps_threshold forms them
__device__ __forceinline__ uint2 dqn_eps_of(const EpisodeParams& p, int s) {
  return p.eps_tab ? p.eps_tab[s] : make_uint2(p.eps_thr, (uint32_t)p.eps_all);
}
__device__ __forceinline__ float shared_grad(const DqnParams& d, int k, float t) {
  float gk = t * d.inv_agents;
  if (k < kOffB1) gk = fminf(fmaxf(gk, -d.clip), d.clip);
  return gk;
}

// ReplayBuffer.sample_batch rl.py:226-241 for every agent of the step, ahead of the train kernel:
// one wave per agent draws 32 distinct deque indices (replayed, or Philox + Floyd as in
// oracle/philox.py::sample_draws) and writes their ring slots to d.smp (as int32 [A][32]); the
// train kernel gathers each agent's 32 transitions from the ring one agent ahead (double-buffered),
// so neither kernel waits on the random ring reads behind the serial 32-step selection loop.
// One wave draws agent a's 32 slots; n_added = the agent's transitions including this step's.
__device__ __forceinline__ void sample_slots(const DqnParams& d, int a, int l, int n_added) {
  const EpisodeParams& p = d.e;
  const size_t A = (size_t)p.A;
  const int count = n_added < d.cap ? n_added : d.cap;
  const int first = n_added - count;
  int idx = 0;
  if (d.samples) {
    idx = l < kB ? (int)d.samples[((size_t)d.t * A + a) * kB + l] : 0;
  } else {
    uint32_t c0 = (uint32_t)d.t, c1 = (uint32_t)p.episode, c2 = p.agent_offset + (uint32_t)a,
             c3 = kTagSample + (uint32_t)(l & 31);
    philox4x32_10(c0, c1, c2, c3, p.seed_lo, p.seed_hi);
    const int mj = count - kB + (l & 31);
    const int rj = (int)__umulhi(c0, (uint32_t)(mj + 1));
    idx = rj;
    for (int j = 0; j < kB; ++j) {
      const int r = __builtin_amdgcn_readlane(rj, j);  // lane j's draw (j is uniform: an SGPR read, no LDS trip)
      const bool taken = __ballot(l < j && idx == r) != 0;
      if (l == j) idx = taken ? count - kB + j : r;
    }
  }
  if (l < kB) reinterpret_cast<int*>(d.smp)[(size_t)a * kB + l] = (first + idx) % d.cap;
}

// The shared network's post-exchange Adam step of parameter k (NSEG >= d.n_segs): the gathered
// segments summed in global segment order, the mean over every agent of every rank, clip, Keras Adam
// (beta1 .9, beta2 .999) and Trainer._soft_update (rl.py:307-359).  Every segment's value and the Adam
// state are loaded before the first add (one memory round trip).  Returns the new weight; `store`:
// writes the new moments, weight and soft-updated target to the *_out arrays.  One function for the
// standalone launch and the act kernel's fused form, so both give the same bits.
template <int NSEG>
__device__ __forceinline__ float adam_shared_param(const DqnParams& d, int k, bool store) {
  const int n = d.n_segs;
  float sv[NSEG];
#pragma unroll
  for (int g = 0; g < NSEG; ++g) sv[g] = g < n ? d.segs[(size_t)g * kNetStride + k] : 0.0f;
  const float m0 = d.adam_m[k], v0 = d.adam_v[k], w0 = d.theta[k];
  const float tg0 = store ? d.target[k] : 0.0f;
  float t = sv[0];
#pragma unroll
  for (int g = 1; g < NSEG; ++g) t = g < n ? t + sv[g] : t;  // segs 0 + 1 + ... + n-1, in order
  const AdamStep s = adam_step(d, m0, v0, w0, shared_grad(d, k, t), d.lr_t);
  if (store) {
    d.m_out[k] = s.m;
    d.v_out[k] = s.v;
    d.theta_out[k] = s.w;
    d.target_out[k] = soft_update(d, tg0, s.w);
  }
  return s.w;
}
