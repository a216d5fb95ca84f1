// p2pmg_policy.hip — policy_episode_kernel: one greedy episode of every scenario whose actions are bytes of the
// context's policy set (p2pmg_run_policy), not argmaxes of Q rows.  Lane = agent and the step of episode_kernel
// (p2pmg_general.hip).  The proposal-matrix types (PRegs / PTile, group_sum_n) are shared with that kernel; the
// step helpers of p2pmg_episode_step.h (round_p2p_bin, divide_power, market_reward) are called by THIS kernel
// only: episode_kernel keeps the same expressions written out in its own body, so an edit to a helper does not
// change the general kernel, and an edit to either copy must be mirrored in the other.  What differs is the
// action source:
//   * where the general kernel gathers a 32-B row and runs argmax3, this one loads ONE BYTE,
//     pol[policy_of[a] * n_states + strip + ip] (a 64-bit policy offset: M * n_states can pass 2^32), and maps
//     255 (unvisited) to action 0 with a select;
//   * the loads are unconditional: masked-off and out-of-group lanes read agent 0's policy at valid states;
//   * round 0's p2p bin is the constant ip_zero, so the NEXT step's round-0 byte is issued right after this
//     step's final action, before its market work (the way the general kernel prefetches row0); rounds r > 0
//     load the byte their own p2p bin selects;
//   * no codes buffer, no Philox, no TD, no delta hash, no table pointer.
#include "p2pmg_episode_step.h"

namespace p2pmg {
namespace {

// the action a policy byte stands for: 255 (P2PMG_POLICY_UNVISITED) acts as action 0
__device__ __forceinline__ int policy_action(uint32_t b) { return b == 255u ? 0 : (int)b; }

// policy_episode_kernel<NC, WIDE, B20>: WIDE = false: N = NC agents per scenario compiled in (PRegs);
// WIDE = true: n = p.N <= NC agents (PTile).  One wave per workgroup, kWave / pow2ceil(NC) scenarios per wave.
template <int NC, bool WIDE, bool B20>
__global__ __launch_bounds__(kWave) void policy_episode_kernel(const PolicyParams pp) {
  const EpisodeParams& p = pp.e;
  constexpr int G = pow2ceil(NC);
  constexpr int SPW = kWave / G;
  constexpr int PW = step_p_floats<NC, WIDE>();
  constexpr int RW = step_r_floats<NC, WIDE>();
  __shared__ float shP[PW];
  __shared__ float shR[RW];

  const int lane = (int)threadIdx.x;
  const int sl = lane / G;
  const int i = lane % G;
  const int n = WIDE ? p.N : NC;  // agents per scenario
  const Community<NC, WIDE> C{p.N, (float)n};
  const int s = blockIdx.x * SPW + sl;
  const bool active = (i < n) && (s < p.S);
  const int a = active ? s * n + i : 0;
  const int s_env = p.n_env == 1 ? 0 : (s < p.S ? s : 0);
  const int T = p.T;
  const int R1 = p.R + 1;
  const bool margin_one = p.margin == 1.0f;
  const uint32_t rec = (uint32_t)p.record;
  const size_t A = (size_t)p.A;
  // loop constants in VGPRs; setpoint, comfort band, COP and the comfort weight are the agent's own (inactive
  // and out-of-group lanes: agent 0's)
  const KC k = pin_constants(p, p.thermal[a], p.learn[a]);
  const Dims<B20> D{k.nt, k.nT, k.nb, k.np};
  std::conditional_t<WIDE, PTile<NC>, PRegs<NC>> P;
  if constexpr (WIDE) {
    P.base = shP + sl * 2 * PTile<NC>::kTile;
    P.i = i;
    P.rd = 0;
    P.wr = 0;
    // lanes i >= n read columns and rows no put() writes (their results are dropped, but the values
    // reach idx_plain and a load address): give them zeros, once
    for (int k2 = lane; k2 < PW; k2 += kWave) shP[k2] = 0.0f;
    wave_lds_fence();
  } else {
    P.sh = shP;
    P.i = i;
    P.sl = sl;
  }

  // the agent's policy: inactive and out-of-group lanes read agent 0's (a = 0)
  const size_t n_states = (size_t)p.nt * (size_t)p.nT * (size_t)p.nb * (size_t)p.np;
  const uint8_t* __restrict__ pol = pp.pol + (size_t)pp.pol_of[a] * n_states;
  const float mi = active ? p.max_in[a] : 1.0f;
  const float4 lv = p.hp_lv[a];  // heat-pump power of actions 0..2 for this agent
  const bool bat = p.battery != 0;
  const double bcap = bat ? p.bat_cap[a] : 0.0;
  double soc = bat ? p.soc[a] : 0.0;
  float tin = active ? p.t_in[a] : k.setpoint;
  float tm = active ? p.t_m[a] : k.setpoint;
  // round 0 has p2p = mean(-0 ... -0) / max_in = 0 (agent.py:203, community.py:161)
  const int ip_zero = idx_plain(C.divn(0.0f) / mi, D.p());

  // running offsets (no 64-bit multiplies in the loop)
  const float* envb = p.env + (size_t)s_env * kEnvStride;
  const size_t env_step = (size_t)p.n_env * kEnvStride;
  const size_t env_end = env_step * T;
  const float2* profb = p.prof + a;
  const size_t prof_end = A * T;
  float* rec_reward = p.rec_reward + a;
  float* rec_cost = p.rec_cost + a;
  float* rec_grid = p.rec_grid + a;
  float* rec_p2p = p.rec_p2p + a;
  float* rec_tin = p.rec_tin + a;
  uint8_t* rec_action = p.rec_action + a;
  int32_t* rec_index = p.rec_index + a;
  auto adv = [](size_t off, size_t step, size_t end) { off += step; return off >= end ? off - end : off; };
  size_t e1o = adv(0, env_step, env_end), e2o = adv(e1o, env_step, env_end);
  size_t f1o = adv(0, A, prof_end), f2o = adv(f1o, A, prof_end);

  EnvRow e0 = load_env(envb);
  EnvRow e1 = load_env(envb + e1o);
  const float2 f0 = profb[0];
  float2 f1 = profb[f1o];
  StepIdx st = make_step(k, D, margin_one, e0.time, e1.time, FDIV(f0.x - f0.y, mi), f1, tin, mi, ip_zero);
  uint32_t b0 = pol[st.strip + (uint32_t)ip_zero];  // round 0's byte of step 0
  float ep_sum = 0.0f;
  size_t tA = 0;

  for (int t = 0; t < T; ++t, tA += A) {
    // prefetch ahead: env / profile two steps
    const EnvRow e2 = load_env(envb + e2o);
    const float2 f2 = profb[f2o];

    P.clear();
    int act = 0, ip = ip_zero;
    float hp = 0.0f;
    double soc_r = soc;  // tentative SoC of the current round
    uint32_t bR = b0;    // the byte of the round's state

    for (int r = 0; r < R1; ++r) {
      if (r > 0) {
        P.next_round();  // Jacobi: read the previous round's column (community.py:84-86)
        ip = round_p2p_bin(P, C, i, mi, D.p());
        bR = pol[st.strip + (uint32_t)ip];
      }
      act = policy_action(bR);
      hp = hp_of(lv, act);

      // RLAgent._divide_power agent.py:186-195 on out = bal * max_in + hp (agent.py:210);
      // with a battery the rule adjusts the net power first (SoC committed by the last round)
      float out = (st.bal * mi) + hp;
      if (bat && bcap > 0.0) {
        soc_r = soc;
        out = (float)battery_rule((double)out, soc_r, bcap, p.bat_min, p.bat_max, p.bat_sqrt_eff);
      }
      divide_power(P, C, i, r, out);
      if (active && (rec & 96u)) {
        const size_t kk = (tA * R1) + (size_t)r * A;
        if (rec & 32u) rec_action[kk] = (uint8_t)act;
        if (rec & 64u) rec_index[kk] = st.it | (st.iT << 8) | (st.ib << 16) | (ip << 24);
      }
    }

    soc = soc_r;  // BatteryStorage state after the final round's decision
    // CommunityMicrogrid._step -> HPHeating.step (community.py:184-188, heating.py:138-143):
    // computed now so the next step's byte can be issued before this step's market work
    float tin1 = tin, tm1 = tm;
    rc_update(k, e0.t_out, hp, tin1, tm1);
    // (after the last step this prefetches a wrapped, unused step: a harmless valid address)
    const StepIdx st1 = make_step(k, D, margin_one, e1.time, e2.time, st.baln, f2, tin1, mi, ip_zero);
    const uint32_t b0n = pol[st1.strip + (uint32_t)ip_zero];

    P.next_round();
    const StepOutcome mk = market_reward(P, C, k, e0, tin);

    if (active && (rec & 31u)) {
      if (rec & 1u) rec_reward[tA] = mk.rw;
      if (rec & 2u) rec_cost[tA] = mk.cost;
      if (rec & 4u) rec_grid[tA] = mk.g;
      if (rec & 8u) rec_p2p[tA] = mk.pp;
      if (rec & 16u) rec_tin[tA] = tin;
    }
    // avg_reward = sum_t mean_i r (community.py:179), canonical sequential order
    float m;
    if constexpr (WIDE) m = group_sum_n<NC>(mk.rw, i, sl, n, shR);
    else m = group_sum<NC>(mk.rw, lane, i, sl, shR);
    ep_sum = ep_sum + C.divn(m);

    tin = tin1;
    tm = tm1;
    e0 = e1;
    e1 = e2;
    f1 = f2;
    e2o = adv(e2o, env_step, env_end);
    f2o = adv(f2o, A, prof_end);
    st = st1;
    b0 = b0n;
  }
  if (active) {
    p.t_in[a] = tin;
    p.t_m[a] = tm;
    if (bat) p.soc[a] = soc;
    if (i == 0) p.ep_reward[s] = ep_sum;
  }
}

template <int NC, bool WIDE>
hipError_t launch_policy(const PolicyParams& p, hipStream_t st) {
  constexpr int SPW = kWave / pow2ceil(NC);
  if (p.e.N < 1 || p.e.N > NC || (!WIDE && p.e.N != NC) || !p.pol || !p.pol_of) return hipErrorInvalidValue;
  const int blocks = (p.e.S + SPW - 1) / SPW;
  if (p.e.nt == 20 && p.e.nT == 20 && p.e.nb == 20 && p.e.np == 20)
    hipLaunchKernelGGL((policy_episode_kernel<NC, WIDE, true>), dim3(blocks), dim3(kWave), 0, st, p);
  else
    hipLaunchKernelGGL((policy_episode_kernel<NC, WIDE, false>), dim3(blocks), dim3(kWave), 0, st, p);
  return hipGetLastError();
}

}  // namespace

// _build.py compiles this file once per slice (-DP2PMG_POLICY_SLICE=k, in parallel), as it does the general
// kernel's: a slice defines one launcher, slice 0 the dispatcher as well.
#if P2PMG_POLICY_SLICE == 0
hipError_t launch_policy_n1_8(const PolicyParams& p, hipStream_t stream) {
  switch (p.e.N) {
    case 1: return launch_policy<1, false>(p, stream);
    case 2: return launch_policy<2, false>(p, stream);
    case 3: return launch_policy<3, false>(p, stream);
    case 4: return launch_policy<4, false>(p, stream);
    case 5: return launch_policy<5, false>(p, stream);
    case 6: return launch_policy<6, false>(p, stream);
    case 7: return launch_policy<7, false>(p, stream);
    case 8: return launch_policy<8, false>(p, stream);
    default: return hipErrorInvalidValue;
  }
}
// registers for N in {1..8, 16}, LDS tiles for every other N <= 64 (and for any N <= 64 when tile != 0)
hipError_t launch_policy_episode(const PolicyParams& p, int tile, hipStream_t stream) {
  if (p.e.N < 1 || p.e.N > kMaxAgents) return hipErrorInvalidValue;
  if (!tile) {
    if (p.e.N <= 8) return launch_policy_n1_8(p, stream);
    if (p.e.N == 16) return launch_policy_n16_tiles(p, 0, stream);
  }
  return launch_policy_n16_tiles(p, general_tile_cap(p.e.N), stream);
}
#endif
#if P2PMG_POLICY_SLICE == 1
hipError_t launch_policy_n16_tiles(const PolicyParams& p, int nc, hipStream_t stream) {
  switch (nc) {
    case 0: return launch_policy<16, false>(p, stream);
    case 16: return launch_policy<16, true>(p, stream);
    case 32: return launch_policy<32, true>(p, stream);
    case 64: return launch_policy<64, true>(p, stream);
    default: return hipErrorInvalidValue;
  }
}
#endif

}  // namespace p2pmg
