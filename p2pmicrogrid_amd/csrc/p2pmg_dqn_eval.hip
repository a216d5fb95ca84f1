// p2pmg_dqn_eval.hip — the frozen-policy episode of the DQN variant: the whole greedy episode
// (CommunityMicrogrid.run community.py:95-123 with DQNAgent.take_decision agent.py:344-350) of a batch in
// ONE launch.  dqn_greedy_episode_kernel is dqn_act_kernel's env step in mode == 1 (p2pmg_dqn_act.hip:
// the same expression sequence, value for value, from the act_q order of include/p2pmg.h through the
// sequential j sums, _divide_power, the fmed3 pair exchange, settle and rc_update to ep_reward) with the
// time loop inside the kernel: nothing changes a weight in greedy mode, so a wave loads its agent's
// network once instead of once per env step, and T_in / T_m never leave the chip between steps.
// No RNG, no replay codes, no replay-memory append.  The network of agent a is
// nets + net_of[a] * kNetStride (net_of null: the context's own arrays, agent a's network or the one
// shared network), so S scenarios can share N (or any M) networks.
#include "p2pmg_internal.h"

namespace p2pmg {
namespace {
#include "p2pmg_device.h"
#include "p2pmg_dqn_ops.h"
#include "p2pmg_dqn_step.h"

// dqn_greedy_episode_kernel<NC, WIDE, W2REG>: one workgroup per scenario, dqn_act_kernel's two forms.
// WIDE = false: NC = N agents compiled in, ONE WAVE PER AGENT; lane j is hidden unit j of the agent's
// Q-MLP and holds its first-layer column, biases and output weight in registers for the whole episode,
// and with W2REG its W2 column (64 values) too; T_in, T_m and the step's observation are wave-uniform
// registers.  WIDE = true: any n = p.N <= NC, 16 waves, wave w acting for agents w, w + 16, ...; the
// agents' state lives in per-agent LDS slots only their wave touches, and the units are read where used
// (frozen weights: L2 hits), as in dqn_act_kernel.
// P stays in the two LDS tiles.  Round 0 reads P = 0 (community.py:74): the zeros are substituted where
// the act kernel reads its zeroed tile, so no tile is cleared per step.  The workgroup synchronises once
// per round (the new P) and once per step (the agents' rewards; it also orders the step's last reads of
// P before the next step's first writes).  Wave 0 carries the running episode reward.
// Step t + 1's env and profile rows are loaded ahead of step t's rounds (t + 1 == T: row 0, unused).
template <int NC, bool WIDE>
constexpr int dqn_eval_waves() {
  return WIDE ? 16 : NC;
}
template <int NC, bool WIDE, bool W2REG>
__global__ __launch_bounds__((dqn_eval_waves<NC, WIDE>() * kWave)) void dqn_greedy_episode_kernel(const DqnEvalParams d) {
  static_assert(!(WIDE && W2REG), "the wide form reads its units where used");
  constexpr int NW = dqn_eval_waves<NC, WIDE>();  // waves
  constexpr int APW = (NC + NW - 1) / NW;         // agents per wave
  const EpisodeParams& p = d.e;
  __shared__ float shP[2][NC * NC];
  __shared__ float4 shH[NW][kH];
  __shared__ float shR[NC];
  const int n = WIDE ? p.N : NC;
  const float nf = (float)n;
  auto divn = [&](float x) -> float {
    if constexpr (WIDE) return x / nf;
    else return div_n<NC>(x);
  };
  const int s = blockIdx.x;
  const int w = threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  const int T = p.T, R1 = p.R + 1;
  const size_t A = (size_t)p.A;
  const int s_env = p.n_env == 1 ? 0 : s;
  // the wave's agents: what an episode keeps of each (registers for one agent per wave, LDS for several)
  struct Ag {
    int a;
    float mi, tin, tm, bal, tnorm;
    float4 lv;
    float4 th;  // the agent's {setpoint, lower, upper, cop} (EpisodeParams::thermal)
    float penw;  // its comfort weight (DqnEvalParams::penw): only the recorded rewards depend on it
    int act;
    float hp, p2pf;
    float2 fnext;      // the agent's profile row of the next step
    const float* net;  // its network
  };
  struct Unit {
    float w10, w11, w12, w13, w14, b1, b2, w3, b3;
    const float* w2col;
  };
  auto load_unit = [&](const float* th) -> Unit {
    return Unit{th[kOffW1 + 0 * kH + lane], th[kOffW1 + 1 * kH + lane], th[kOffW1 + 2 * kH + lane],
                th[kOffW1 + 3 * kH + lane], th[kOffW1 + 4 * kH + lane], th[kOffB1 + lane],
                th[kOffB2 + lane],          th[kOffW3 + lane],          th[kOffB3],
                th + kOffW2 + lane};
  };
  __shared__ Ag sAg[WIDE ? NC : 1];
  Ag rAg;
  auto agent = [&](int i) -> Ag& {
    if constexpr (WIDE) return sAg[i];
    else return rAg;
  };
  Unit ru{};
  float w2r[W2REG ? kH : 1];
  for (int k = 0; k < APW; ++k) {
    const int i = w + k * NW;
    if (i >= n) break;  // wave-uniform
    Ag& g = agent(i);
    g.a = s * n + i;
    g.mi = p.max_in[g.a];
    g.tin = p.t_in[g.a];
    g.tm = p.t_m[g.a];
    g.th = p.thermal[g.a];
    g.penw = d.penw[g.a];
    g.lv = p.hp_lv[g.a];
    g.act = 0;
    g.hp = 0.0f;
    g.p2pf = 0.0f;
    g.fnext = p.prof[g.a];  // step 0
    g.net = d.nets + (size_t)(d.net_of ? d.net_of[g.a] : (d.one_net ? 0 : g.a)) * kNetStride;
    if constexpr (!WIDE) {
      ru = load_unit(g.net);
      if constexpr (W2REG) {
#pragma unroll
        for (int kk = 0; kk < kH; ++kk) w2r[kk] = ru.w2col[kk * kH];
      }
    }
  }
  const float* en = p.env + (size_t)s_env * kEnvStride;  // step 0
  float time_n = en[0], tout_n = en[1], buy_n = en[2], inj_n = en[3], p2pp_n = en[4];
  float ep = 0.0f;  // wave 0: sum_t mean_i r so far
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    const int tn = (t + 1 == T) ? 0 : t + 1;
    const float time_t = time_n, t_out = tout_n, buy = buy_n, inj = inj_n, p2pp = p2pp_n;
    en = p.env + ((size_t)tn * p.n_env + s_env) * kEnvStride;
    time_n = en[0], tout_n = en[1], buy_n = en[2], inj_n = en[3], p2pp_n = en[4];
    for (int k = 0; k < APW; ++k) {
      const int i = w + k * NW;
      if (i >= n) break;  // wave-uniform
      Ag& g = agent(i);
      const float2 f0 = g.fnext;
      g.fnext = p.prof[(size_t)tn * A + g.a];
      g.bal = (f0.x - f0.y) / g.mi;  // RLAgent._get_balance agent.py:172-176
      g.tnorm = (g.tin - g.th.x) / p.margin;  // HPHeating.normalized_temperature heating.py:118-120
    }
    for (int r = 0; r < R1; ++r) {
      const float* P = shP[cur];
      for (int k = 0; k < APW; ++k) {
        const int i = w + k * NW;
        if (i >= n) break;  // wave-uniform
        Ag& g = agent(i);
        const int a = g.a;
        // powers = -P[:, i], diagonal zeroed (community.py:76,81); p2p = mean / max_in (agent.py:203)
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < n; ++j) acc = acc + (-((j == i || r == 0) ? 0.0f : P[j * n + i]));
        g.p2pf = divn(acc) / g.mi;
        {
          // ActorModel.greedy_action rl.py:188-196: Q(obs, a) for a in (0, .5, 1), argmax (first max)
          const Unit u = WIDE ? load_unit(g.net) : ru;
          float z = g.p2pf * u.w13;
          z = fmaf(g.bal, u.w12, z);
          z = fmaf(g.tnorm, u.w11, z);
          z = fmaf(time_t, u.w10, z);
          const float h0 = relu(z + u.b1), h1 = relu(fmaf(0.5f, u.w14, z) + u.b1), h2 = relu((z + u.w14) + u.b1);
          shH[w][lane] = make_float4(h0, h1, h2, 0.0f);
          wave_lds_fence();
          float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
          if constexpr (W2REG) {
#pragma unroll
            for (int kk = 0; kk < kH; ++kk) {
              const float4 hk = shH[w][kk];
              a0 = fmaf(hk.x, w2r[kk], a0);
              a1 = fmaf(hk.y, w2r[kk], a1);
              a2 = fmaf(hk.z, w2r[kk], a2);
            }
          } else {
#pragma unroll 8
            for (int kk = 0; kk < kH; ++kk) {
              const float wk = u.w2col[kk * kH];
              const float4 hk = shH[w][kk];
              a0 = fmaf(hk.x, wk, a0);
              a1 = fmaf(hk.y, wk, a1);
              a2 = fmaf(hk.z, wk, a2);
            }
          }
          wave_lds_fence();
          const float q0 = wave_sum(relu(a0 + u.b2) * u.w3) + u.b3;
          const float q1 = wave_sum(relu(a1 + u.b2) * u.w3) + u.b3;
          const float q2 = wave_sum(relu(a2 + u.b2) * u.w3) + u.b3;
          g.act = 0;
          float best = q0;
          if (q1 > best) { best = q1; g.act = 1; }
          if (q2 > best) g.act = 2;
        }
        g.hp = g.act == 0 ? g.lv.x : (g.act == 1 ? g.lv.y : g.lv.z);  // heating.set_power(action) -> hp.power * max_power
        // RLAgent._divide_power agent.py:186-195 on out = balance * max_in + hp (agent.py:210)
        const float out = (g.bal * g.mi) + g.hp;
        const float so = sgn(out);
        float tot = 0.0f, fj = 0.0f;
#pragma unroll
        for (int j = 0; j < n; ++j) {
          const float pw = -((j == i || r == 0) ? 0.0f : P[j * n + i]);
          const float f = (so != sgn(pw)) ? pw : 0.0f;
          tot = tot + f;
          if (j == lane) fj = f;
        }
        tot = fabsf(tot);
        if (lane < n) {
          float v;
          if (tot == 0.0f) v = divn(out * 1.0f);
          else v = (lane == i) ? (tot == tot ? out * 0.0f : tot) : (out * fabsf(fj)) / tot;
          shP[cur ^ 1][i * n + lane] = v;
        }
        if (lane == 0 && (p.record & 32)) p.rec_action[((size_t)t * R1 + r) * A + a] = (uint8_t)g.act;
      }
      __syncthreads();
      cur ^= 1;
    }
    const float* P = shP[cur];
    for (int k = 0; k < APW; ++k) {
      const int i = w + k * NW;
      if (i >= n) break;  // wave-uniform
      Ag& g = agent(i);
      const int a = g.a;
      // CommunityMicrogrid._assign_powers community.py:45-54 (final P, diagonal kept)
      float gg = 0.0f, pp = 0.0f;
#pragma unroll
      for (int j = 0; j < n; ++j) {
        const float pij = P[i * n + j], pji = P[j * n + i];
        const float ex = __builtin_amdgcn_fmed3f(pij, -pji, 0.0f);  // pair_exchange (p2pmg_kernels.hip)
        gg = gg + (pij - ex);
        pp = pp + ex;
      }
      const Settled st = settle(p, gg, pp, buy, inj, p2pp, g.tin, g.th, g.penw);
      if (lane == 0) {
        const size_t kr = (size_t)t * A + a;
        if (p.record & 1) p.rec_reward[kr] = st.rw;
        if (p.record & 2) p.rec_cost[kr] = st.cost;
        if (p.record & 4) p.rec_grid[kr] = gg;
        if (p.record & 8) p.rec_p2p[kr] = pp;
        if (p.record & 16) p.rec_tin[kr] = g.tin;
        shR[i] = st.rw;
      }
      float tin = g.tin, tm = g.tm;
      // HPHeating.step heating.py:138-143 at the agent's COP
      const RcParams rc{p.inv_ci, p.inv_cm, p.inv_ri, p.inv_re, p.inv_rvent, p.c_in, p.c_m, p.solar, g.th.w, p.spm, p.slot};
      rc_update(rc, t_out, g.hp, tin, tm);
      g.tin = tin;
      g.tm = tm;
    }
    __syncthreads();
    if (w == 0) {  // avg_reward = sum_t mean_i r (community.py:179), canonical order
      float m = 0.0f;
#pragma unroll
      for (int j = 0; j < n; ++j) m = m + shR[j];
      ep = ep + divn(m);
    }
  }
  for (int k = 0; k < APW; ++k) {
    const int i = w + k * NW;
    if (i >= n) break;  // wave-uniform
    const Ag& g = agent(i);
    if (lane == 0) {
      p.t_in[g.a] = g.tin;
      p.t_m[g.a] = g.tm;
    }
  }
  if (threadIdx.x == 0 && T > 0) {
    d.ep_acc[s] = ep;
    p.ep_reward[s] = ep;
  }
}

}  // namespace

hipError_t launch_dqn_greedy_episode(const DqnEvalParams& d, hipStream_t st) {
  const int N = d.e.N;
  if (N < 1 || N > kMaxAgents || d.e.S < 1) return hipErrorInvalidValue;
  const dim3 grid(d.e.S), wide(16 * kWave);
  switch (N) {
  // W2 columns in registers up to N = 8; at N = 16 (1024 threads, 128 VGPRs per lane) the 64 values spill,
  // so that size reads W2 where used, like the wide form
#define P2PMG_DQN_EVAL(NN)                                                                                          \
  case NN:                                                                                                          \
    hipLaunchKernelGGL((dqn_greedy_episode_kernel<NN, false, (NN <= 8)>), grid, dim3(NN * kWave), 0, st, d);        \
    break;
    P2PMG_DQN_EVAL(1) P2PMG_DQN_EVAL(2) P2PMG_DQN_EVAL(3) P2PMG_DQN_EVAL(4) P2PMG_DQN_EVAL(5) P2PMG_DQN_EVAL(6)
    P2PMG_DQN_EVAL(7) P2PMG_DQN_EVAL(8) P2PMG_DQN_EVAL(16)
#undef P2PMG_DQN_EVAL
    default: {  // every other community size: wave w acts for agents w, w + 16, ...
      const int nc = general_tile_cap(N);
      if (nc == 16) hipLaunchKernelGGL((dqn_greedy_episode_kernel<16, true, false>), grid, wide, 0, st, d);
      else if (nc == 32) hipLaunchKernelGGL((dqn_greedy_episode_kernel<32, true, false>), grid, wide, 0, st, d);
      else hipLaunchKernelGGL((dqn_greedy_episode_kernel<64, true, false>), grid, wide, 0, st, d);
    }
  }
  return hipGetLastError();
}

}  // namespace p2pmg
