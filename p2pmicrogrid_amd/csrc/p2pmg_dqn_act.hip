// p2pmg_dqn_act.hip — gfx950 kernels of the DQN variant (BASELINE.json configs[4]), the env step:
//   QNetwork rl.py:135-148, ActorModel rl.py:151-197, ReplayBuffer rl.py:200-248,
//   Trainer._train / _soft_update rl.py:307-359, DQNAgent agent.py:301-350.
//
// One environment step = two launches (plus, for one shared network, one reduce + Adam launch):
//   dqn_act_kernel<N>    one workgroup per scenario, ONE WAVE PER AGENT; lane j is hidden unit j
//                        of the agent's Q-MLP (weights streamed as coalesced 256-B rows), the
//                        R+1 Jacobi rounds exchange the proposal matrix through LDS, then market,
//                        reward, replay-memory append and the RC update (community.py:67-93,
//                        149-182; agent.py:200-213, 225-232; heating.py:37-56).
//                        One shared network: dqn_act_shared_kernel (p2pmg_dqn_act_shared.hip).
//   dqn_train_kernel     p2pmg_dqn_train.hip; the shared network's reduce, fold and Adam kernels and
//                        the object API's forward: p2pmg_dqn_shared.hip.
// Layouts (HBM): networks [n_nets][4672] f32 (Keras order W1[5][64] b1 W2[64][64] b2 W3[64] b3),
// replay rings [A][cap][10] f32 (s[4], a, r, ns[4]), added [A].
#include "p2pmg_internal.h"

namespace p2pmg {
namespace {
#include "p2pmg_device.h"
#include "p2pmg_dqn_ops.h"
#include "p2pmg_dqn_step.h"

__global__ __launch_bounds__(kWave) void dqn_sample_kernel(const DqnParams d) {
  sample_slots(d, blockIdx.x, threadIdx.x, d.added[blockIdx.x]);
}

// ReplayBuffer.sample_batch (rl.py:226-241) of every env step of a Philox training episode in ONE
// throughput launch ahead of it: thread = (step t, agent a), the 32 draws of
// oracle/philox.py::sample_draws with Floyd's rule walked in order (draw q takes count - 32 + q when
// r_q equals an earlier draw's final index), written as deque indices [T][A][32] u16 -- the layout
// replay mode uploads (p2pmg_dqn_set_samples), which the act kernels read instead of drawing in
// their latency-bound tail.  Every training env step appends one transition per agent before it
// samples (agent.py:338-342), so step t's count follows from the episode-start count.
__global__ __launch_bounds__(256) void dqn_sample_prepass_kernel(const DqnParams d, uint16_t* __restrict__ out) {
  const EpisodeParams& p = d.e;
  const size_t A = (size_t)p.A;
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (size_t)p.T * A) return;
  const int t = (int)(k / A), a = (int)(k % A);
  const int n_add = d.added[a] + t + 1;
  const int count = n_add < d.cap ? n_add : d.cap;
  int idx[kB];
#pragma unroll
  for (int q = 0; q < kB; ++q) {
    uint32_t c0 = (uint32_t)t, c1 = (uint32_t)p.episode, c2 = p.agent_offset + (uint32_t)a, c3 = kTagSample + (uint32_t)q;
    philox4x32_10(c0, c1, c2, c3, p.seed_lo, p.seed_hi);
    const int r = (int)__umulhi(c0, (uint32_t)(count - kB + q + 1));
    bool taken = false;
#pragma unroll
    for (int l = 0; l < q; ++l) taken = taken || idx[l] == r;
    idx[q] = taken ? count - kB + q : r;
  }
  uint4* o = reinterpret_cast<uint4*>(out + k * kB);
#pragma unroll
  for (int v = 0; v < kB / 8; ++v) {
    const int* x = idx + 8 * v;
    o[v] = make_uint4((uint32_t)x[0] | ((uint32_t)x[1] << 16), (uint32_t)x[2] | ((uint32_t)x[3] << 16),
                      (uint32_t)x[4] | ((uint32_t)x[5] << 16), (uint32_t)x[6] | ((uint32_t)x[7] << 16));
  }
}

// ----------------------------------------------------------------- act: one env step
// dqn_act_kernel<NC, WIDE>: one workgroup per scenario.  WIDE = false: NC = N agents compiled in
// (N <= 16), one wave per agent.  WIDE = true: any n = p.N <= NC (the community sizes 9..15 and
// 17..64), NW = 16 waves, wave w acting for agents w, w + 16, ... in turn in each round
// (a round is Jacobi: every agent reads the previous round's P, community.py:84-86, so the order of
// the agents within a round does not matter).  Both forms sum over j = 0..n-1 in order and divide
// by n as IEEE quotients: the same bits.
template <int NC, bool WIDE>
constexpr int dqn_act_waves() {
  return WIDE ? 16 : NC;
}
template <int NC, bool WIDE>
__global__ __launch_bounds__((dqn_act_waves<NC, WIDE>() * kWave)) void dqn_act_kernel(const DqnParams d) {
  constexpr int NW = dqn_act_waves<NC, WIDE>();  // waves
  constexpr int APW = (NC + NW - 1) / NW;    // agents per wave
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
  const int t = d.t, T = p.T, tn = (t + 1 == T) ? 0 : t + 1;
  const int R1 = p.R + 1, W = (R1 + 3) >> 2;
  const size_t A = (size_t)p.A;
  const int s_env = p.n_env == 1 ? 0 : s;
  const float* e0 = p.env + ((size_t)t * p.n_env + s_env) * kEnvStride;
  const float* e1 = p.env + ((size_t)tn * p.n_env + s_env) * kEnvStride;
  const float time_t = e0[0], t_out = e0[1], buy = e0[2], inj = e0[3], p2pp = e0[4];
  const float time_n = e1[0];
  const bool greedy_mode = p.mode == 1;
  const uint2 eps_s = dqn_eps_of(p, s);  // the scenario's exploration thresholds (workgroup-uniform)
  // the wave's agents: wave-uniform scalars (registers for one agent per wave, LDS for several) and
  // this lane's hidden unit of the agent's network (rl.py:139-141): first-layer column, biases,
  // output weight (registers for one agent per wave, read where used for several: L2 hits)
  struct Ag {
    int a;
    float mi, tin, tm, bal, baln, tnorm;
    float4 lv;
    float4 th;  // the agent's {setpoint, lower, upper, cop} (EpisodeParams::thermal)
    float penw;  // its comfort weight (DqnParams::penw)
    int act;
    float hp, p2pf;
  };
  struct Unit {
    float w10, w11, w12, w13, w14, b1, b2, w3, b3;
    const float* w2col;
  };
  auto load_unit = [&](int a) -> Unit {
    // the agent's network: its role's (a % N = a - s N) on a role context, the shared one, or its own
    const float* th = d.theta + (size_t)(d.roles ? a - s * n : (d.n_nets == 1 ? 0 : a)) * kNetStride;
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
  for (int k = 0; k < APW; ++k) {
    const int i = w + k * NW;
    if (i >= n) break;  // wave-uniform
    Ag& g = agent(i);
    g.a = s * n + i;
    const float2 f0 = p.prof[(size_t)t * A + g.a], f1 = p.prof[(size_t)tn * A + g.a];
    g.mi = p.max_in[g.a];
    g.tin = p.t_in[g.a];
    g.tm = p.t_m[g.a];
    g.bal = (f0.x - f0.y) / g.mi;  // RLAgent._get_balance agent.py:172-176
    g.baln = (f1.x - f1.y) / g.mi;
    g.th = p.thermal[g.a];
    g.penw = d.penw[g.a];
    g.tnorm = (g.tin - g.th.x) / p.margin;  // HPHeating.normalized_temperature heating.py:118-120
    g.lv = p.hp_lv[g.a];
    g.act = 0;
    g.hp = 0.0f;
    g.p2pf = 0.0f;
    if constexpr (!WIDE) ru = load_unit(g.a);
  }

  for (int k2 = threadIdx.x; k2 < NC * NC; k2 += NW * kWave) shP[0][k2] = 0.0f;  // round 0 reads P = 0
  __syncthreads();
  int cur = 0;
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
      for (int j = 0; j < n; ++j) acc = acc + (-((j == i) ? 0.0f : P[j * n + i]));
      g.p2pf = divn(acc) / g.mi;
      int code = 255;  // ActorModel.select_action rl.py:174-183: explore draw, else greedy
      if (!greedy_mode) {
        if (p.rng == 0) {
          code = replay_code(p, t, W, A, r, a);
        } else {
          // word k = t (R + 1) + r of the agent's decision stream (p2pmg_device.h, oracle/philox.py::decision_draws)
          code = (int)philox_round_code(t, R1, r, (uint32_t)p.episode, p.agent_offset + (uint32_t)a, eps_s.x,
                                        (int)eps_s.y, p.seed_lo, p.seed_hi);
        }
      }
      if (code == 255) {
        // ActorModel.greedy_action rl.py:188-196: Q(obs, a) for a in (0, .5, 1), argmax (first max)
        const Unit u = WIDE ? load_unit(a) : ru;
        float z = g.p2pf * u.w13;
        z = fmaf(g.bal, u.w12, z);
        z = fmaf(g.tnorm, u.w11, z);
        z = fmaf(time_t, u.w10, z);
        const float h0 = relu(z + u.b1), h1 = relu(fmaf(0.5f, u.w14, z) + u.b1), h2 = relu((z + u.w14) + u.b1);
        shH[w][lane] = make_float4(h0, h1, h2, 0.0f);
        wave_lds_fence();
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll 8
        for (int kk = 0; kk < kH; ++kk) {
          const float wk = u.w2col[kk * kH];
          const float4 hk = shH[w][kk];
          a0 = fmaf(hk.x, wk, a0);
          a1 = fmaf(hk.y, wk, a1);
          a2 = fmaf(hk.z, wk, a2);
        }
        wave_lds_fence();
        const float q0 = wave_sum(relu(a0 + u.b2) * u.w3) + u.b3;
        const float q1 = wave_sum(relu(a1 + u.b2) * u.w3) + u.b3;
        const float q2 = wave_sum(relu(a2 + u.b2) * u.w3) + u.b3;
        g.act = 0;
        float best = q0;
        if (q1 > best) { best = q1; g.act = 1; }
        if (q2 > best) g.act = 2;
      } else {
        g.act = code;
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
    const float cost = st.cost, rw = st.rw;

    if (p.mode != 1) {
      // DQNAgent.save_memory agent.py:332-336 -> ReplayBuffer.add rl.py:208-212
      const int32_t n_added = d.added[a];
      float* slot = d.buf + ((size_t)a * d.cap + (size_t)(n_added % d.cap)) * kTrans;
      if (lane < kTrans) {
        const float av = g.act == 0 ? 0.0f : (g.act == 1 ? 0.5f : 1.0f);
        float v;
        switch (lane) {
          case 0: v = time_t; break;
          case 1: v = g.tnorm; break;
          case 2: v = g.bal; break;
          case 3: v = g.p2pf; break;
          case 4: v = av; break;
          case 5: v = rw; break;
          case 6: v = time_n; break;
          case 7: v = g.tnorm; break;  // next state: same (pre-update) temperature (community.py:161)
          case 8: v = g.baln; break;
          default: v = 0.0f / g.mi; break;  // next state p2p = mean(zeros) / max_in
        }
        slot[lane] = v;
      }
      if (lane == 0) d.added[a] = n_added + 1;
      // Trainer.train -> ReplayBuffer.sample_batch (rl.py:299-305, 226-241) right after the append
      // (agent.py:338-342): the same wave draws the agent's 32 slots, no separate launch
      if (p.mode == 0 && d.fused_sample) sample_slots(d, a, lane, n_added + 1);
    }
    if (lane == 0) {
      const size_t kr = (size_t)t * A + a;
      if (p.record & 1) p.rec_reward[kr] = rw;
      if (p.record & 2) p.rec_cost[kr] = cost;
      if (p.record & 4) p.rec_grid[kr] = gg;
      if (p.record & 8) p.rec_p2p[kr] = pp;
      if (p.record & 16) p.rec_tin[kr] = g.tin;
      float tin = g.tin, tm = g.tm;
      // HPHeating.step heating.py:138-143 at the agent's COP
      const RcParams rc{p.inv_ci, p.inv_cm, p.inv_ri, p.inv_re, p.inv_rvent, p.c_in, p.c_m, p.solar, g.th.w, p.spm, p.slot};
      rc_update(rc, t_out, g.hp, tin, tm);
      p.t_in[a] = tin;
      p.t_m[a] = tm;
      shR[i] = rw;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // avg_reward = sum_t mean_i r (community.py:179), canonical order
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < n; ++j) m = m + shR[j];
    const float ep = (t == 0 ? 0.0f : d.ep_acc[s]) + divn(m);
    d.ep_acc[s] = ep;
    p.ep_reward[s] = ep;
  }
}

}  // namespace

hipError_t launch_dqn_act(const DqnParams& d, hipStream_t st) {
  if (d.adam_pending && !dqn_act_fuses_adam(d)) return hipErrorInvalidValue;
  if (act_shared_mfma(d)) return launch_dqn_act_shared(d, st);  // p2pmg_dqn_act_shared.hip
  const dim3 grid(d.e.S), wide(16 * kWave), wide64(dqn_act_waves<64, true>() * kWave);
  switch (d.e.N) {
#define P2PMG_DQN_ACT(NN) \
  case NN: hipLaunchKernelGGL((dqn_act_kernel<NN, false>), grid, dim3(NN * kWave), 0, st, d); break;
    P2PMG_DQN_ACT(1) P2PMG_DQN_ACT(2) P2PMG_DQN_ACT(3) P2PMG_DQN_ACT(4) P2PMG_DQN_ACT(5) P2PMG_DQN_ACT(6)
    P2PMG_DQN_ACT(7) P2PMG_DQN_ACT(8) P2PMG_DQN_ACT(16)
#undef P2PMG_DQN_ACT
    default: {  // every other community size: wave w acts for agents w, w + NW, ...
      const int nc = general_tile_cap(d.e.N);
      if (d.e.N < 1 || d.e.N > kMaxAgents) return hipErrorInvalidValue;
      if (nc == 16) hipLaunchKernelGGL((dqn_act_kernel<16, true>), grid, wide, 0, st, d);
      else if (nc == 32) hipLaunchKernelGGL((dqn_act_kernel<32, true>), grid, wide, 0, st, d);
      else hipLaunchKernelGGL((dqn_act_kernel<64, true>), grid, wide64, 0, st, d);
    }
  }
  return hipGetLastError();
}

hipError_t launch_dqn_sample_prepass(const DqnParams& d, uint16_t* out, hipStream_t st) {
  const size_t n = (size_t)d.e.T * (size_t)d.e.A;
  if (n == 0 || d.cap < kB || d.cap > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dqn_sample_prepass_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, out);
  return hipGetLastError();
}

hipError_t launch_dqn_sample(const DqnParams& d, hipStream_t st) {
  hipLaunchKernelGGL(dqn_sample_kernel, dim3(d.e.A), dim3(kWave), 0, st, d);
  return hipGetLastError();
}

}  // namespace p2pmg
