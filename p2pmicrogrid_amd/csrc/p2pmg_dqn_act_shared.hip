// p2pmg_dqn_act_shared.hip — the DQN env step for one network shared by every agent, on MFMA tiles
// (the per-agent form and the step's layouts: p2pmg_dqn_act.hip).
#include "p2pmg_internal.h"

namespace p2pmg {
namespace {
#include "p2pmg_device.h"
#include "p2pmg_dqn_ops.h"
#include "p2pmg_dqn_step.h"

// ----------------------------------------------------------------- act, one shared network
// dqn_act_shared_kernel<N, AGW>: the same env step as dqn_act_kernel for ONE network shared by
// every agent (configs[4]), with the greedy forwards of AGW agents on MFMA tiles.  A 256-thread
// workgroup owns AGW / N scenarios.  Per round, thread j < AGW does agent j's scalar work
// (observation, divide-power row); the 3 AGW greedy rows (3 actions x AGW agents) go
// through layer 1 on VALU (thread = hidden unit x AGW / 4 agents), layer 2 as Z2^T = W2^T H1^T on
// v_mfma_f32_16x16x4_f32 (wave w owns hidden units 16w..16w+15; its 16 W2 operands stay in
// registers for the launch; the shared W2 is read once per workgroup instead of once per agent and
// round), layer 3 in-lane.  Bitwise the same Q values as dqn_act_kernel: the f32 MFMA accumulates
// its K products as an fmaf chain in k order (the VALU loop's order), and layer 3's sum over the 64
// units is the same pairwise tree (4 units in-lane, the 16-lane row groups over lane ^ 16 and
// lane ^ 32, then the 4 waves pairwise) as wave_sum over lane = unit.
// AGW agent slots per workgroup (16, or 8 for more, shorter workgroups); row = action * AGW + slot,
// in MT = ceil(3 AGW / 16) row tiles.  -DP2PMG_TRACE (timing-only): phase splits of wave 0.
//
// ADAM: the previous env step's shared Adam step is still pending (the multi-segment / multi-rank
// path): every workgroup computes the new value of each weight it reads from the gathered segments
// (adam_shared_param, the same bits as dqn_adam_shared_kernel), and workgroup 0, whose threads cover
// every parameter once, stores the new state into the other half of the runtime's double buffer, so
// no workgroup of this launch reads a value another one wrote.  This replaces a 4,609-parameter launch
// per env step (one launch plus a memory round trip) with loads issued among the act prologue's own.
template <int N, int AGW, bool ADAM>
__global__ __launch_bounds__(256) void dqn_act_shared_kernel(const DqnParams d) {
  static_assert(AGW == 8 || AGW == 16, "8 or 16 agent slots per workgroup");
  constexpr int SPW = AGW / N;          // scenarios per workgroup
  constexpr int AG = SPW * N;           // agents per workgroup (<= AGW)
  constexpr int MT = (3 * AGW + 15) / 16;  // row tiles of the greedy forward
  constexpr int SPT = AGW / 4;          // layer-1 agent slots per thread (4 waves)
  const EpisodeParams& p = d.e;
#if P2PMG_TRACE
  uint64_t atr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, alast;
  asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(alast)::"memory");
#endif
  __shared__ float shP[2][AG * N];
  __shared__ float4 shX[AGW];   // time, normalised T_in, balance, p2p of agent slot j
  __shared__ float H1[16 * MT][kLdsRow];
  __shared__ float qpart[4][64];  // 4 tiles of reduce4_groups (MT used)
  __shared__ float shR[AG];
  __shared__ int shN[AGW];
  __shared__ float shEp[AGW];
  __shared__ int shFlag[2];
  __shared__ __attribute__((aligned(16))) int shI[AGW][kB];  // Floyd draws of the replay sample
  const int tid = threadIdx.x;
  const int w = tid / kWave, l = tid % kWave;
  const int c16 = l & 15, g4 = l >> 4;
  const int t = d.t, T = p.T, tn = (t + 1 == T) ? 0 : t + 1;
  const int R1 = p.R + 1, W = (R1 + 3) >> 2;
  // act_shared_mfma, the launch's gate: every round's code fits codes_pack, so the per-scenario thresholds
  // are dead after the prologue (no per-lane pair held across the rounds)
  __builtin_assume(R1 <= 8);
  const size_t A = (size_t)p.A;
  const bool greedy_mode = p.mode == 1;
  const int s0 = blockIdx.x * SPW;
  const float* th = d.theta;

  // agent thread j < AG: agent a = s0 * N + j of scenario s0 + j / N (agent i = j % N)
  const int j = tid;
  const int sl = j / N, i = j % N;
  const int s = s0 + sl;
  const bool agent_thr = j < AG && s < p.S;
  const int a = agent_thr ? s * N + i : 0;
  const int s_env = p.n_env == 1 ? 0 : (agent_thr ? s : 0);
  const float* e0 = p.env + ((size_t)t * p.n_env + s_env) * kEnvStride;
  const float* e1 = p.env + ((size_t)tn * p.n_env + s_env) * kEnvStride;
  float buy = 0.0f, inj = 0.0f, p2pp = 0.0f;
  float time_t = 0.0f, t_out = 0.0f, time_n = 0.0f, mi = 1.0f, tin = 0.0f, tm = 0.0f, bal = 0.0f, baln = 0.0f,
        tnorm = 0.0f;
  float4 lv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 tp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // the agent's {setpoint, lower, upper, cop}
  float penw = 0.0f;                                // its comfort weight (DqnParams::penw)
  if (agent_thr) {
    time_t = e0[0];
    t_out = e0[1];
    buy = e0[2];
    inj = e0[3];
    p2pp = e0[4];
    time_n = e1[0];
    const float2 f0 = p.prof[(size_t)t * A + a], f1 = p.prof[(size_t)tn * A + a];
    mi = p.max_in[a];
    tin = p.t_in[a];
    tm = p.t_m[a];
    bal = (f0.x - f0.y) / mi;  // RLAgent._get_balance agent.py:172-176
    baln = (f1.x - f1.y) / mi;
    tp = p.thermal[a];
    penw = d.penw[a];
    tnorm = (tin - tp.x) / p.margin;  // HPHeating.normalized_temperature heating.py:118-120
    lv = p.hp_lv[a];
  }
  // loaded with the inputs: a load issued after the step's stores would wait for their completion
  // (vmcnt counts loads and stores in issue order)
  const int32_t n_added = (agent_thr && p.mode != 1) ? d.added[a] : 0;
  const float ep_prev = (tid < SPW && s0 + tid < p.S && t != 0) ? d.ep_acc[s0 + tid] : 0.0f;
  // weight k as this launch uses it; ADAM: after the pending step, stored by workgroup 0's owner
  // thread of k (layer 1: wave 0; W2: every thread; b2 / W3: lanes c16 = 0; b3: thread 0)
  const bool blk0 = ADAM && blockIdx.x == 0;
  auto wt = [&](int k, bool owner) -> float {
    if constexpr (ADAM) return adam_shared_param<kActAdamSegs>(d, k, blk0 && owner);
    else return th[k];
  };
  // layer 1 (thread = hidden unit u of agent slots 4 * (tid / 64) .. + 3): W1 column and b1
  const int u = l;
  const float w10 = wt(kOffW1 + 0 * kH + u, w == 0), w11 = wt(kOffW1 + 1 * kH + u, w == 0),
              w12 = wt(kOffW1 + 2 * kH + u, w == 0), w13 = wt(kOffW1 + 3 * kH + u, w == 0),
              w14 = wt(kOffW1 + 4 * kH + u, w == 0), b1 = wt(kOffB1 + u, w == 0);
  // layer 2 / 3 (wave w, lane: A operand W2[4 kk + g4][16 w + c16]; accumulator units 16 w + 4 g4 + r)
  float w2[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) w2[kk] = wt(kOffW2 + (4 * kk + g4) * kH + 16 * w + c16, true);
  float b2[4], w3[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    b2[r] = wt(kOffB2 + 16 * w + 4 * g4 + r, c16 == 0);
    w3[r] = wt(kOffW3 + 16 * w + 4 * g4 + r, c16 == 0);
  }
  const float b3 = wt(kOffB3, tid == 0);
  // every round's exploration draw (or replayed code) ahead of the rounds: they depend only on
  // (t, episode, agent), so they run under the prologue's load latency, off the rounds' chain
  uint64_t codes_pack = ~0ull;  // byte r: code of round r < 8 (255 = greedy); later rounds are drawn in the loop
  // the agent's scenario's exploration thresholds: a workgroup's agent slots may span scenarios
  uint2 eps_s = make_uint2(p.eps_thr, (uint32_t)p.eps_all);
  if (agent_thr && !greedy_mode) {
    if (p.rng == 0) {
      for (int w4 = 0; w4 < W && w4 < 2; ++w4)
        codes_pack = (codes_pack & ~(0xFFFFFFFFull << (32 * w4))) |
                     ((uint64_t)replay_word(p, t, W, A, w4, a) << (32 * w4));
    } else {
      // every round's code of step t (p2pmg_device.h, oracle/philox.py::decision_draws)
      eps_s = dqn_eps_of(p, s);
      codes_pack = philox_step_codes(t, R1, (uint32_t)p.episode, p.agent_offset + (uint32_t)a, eps_s.x, (int)eps_s.y,
                                     p.seed_lo, p.seed_hi);
    }
  }
  const int tag4 = reduce4_tag();

  if (tid < AG * N) shP[0][tid] = 0.0f;
  // consumed here, before the rounds' record stores: a later first use would wait for those stores
  if (agent_thr) shN[j] = n_added + 1;
  if (tid < SPW) shEp[tid] = ep_prev;
  __syncthreads();
  P2PMG_STAMP(atr, alast, 0);
  int cur = 0, act = 0, code = 255;
  float hp = 0.0f, p2pf = 0.0f;
  uint64_t act_pack = 0;
  for (int r = 0; r < R1; ++r) {
    const float* P = shP[cur] + sl * N * N;  // this agent's scenario
    bool greedy = false;
    if (agent_thr) {
      // powers = -P[:, i], diagonal zeroed (community.py:76,81); p2p = mean / max_in (agent.py:203)
      float acc = 0.0f;
#pragma unroll
      for (int jj = 0; jj < N; ++jj) acc = acc + (-((jj == i) ? 0.0f : P[jj * N + i]));
      p2pf = div_n<N>(acc) / mi;
      code = 255;  // ActorModel.select_action rl.py:174-183: explore draw, else greedy
      if (!greedy_mode) {
        if (r < 8) code = (int)((codes_pack >> (8 * r)) & 0xFFu);
        else if (p.rng == 0) code = replay_code(p, t, W, A, r, a);
        else
          code = (int)philox_round_code(t, R1, r, (uint32_t)p.episode, p.agent_offset + (uint32_t)a, eps_s.x,
                                        (int)eps_s.y, p.seed_lo, p.seed_hi);
      }
      greedy = code == 255;
      shX[j] = make_float4(time_t, tnorm, bal, p2pf);
    }
    P2PMG_STAMP(atr, alast, 1);
    if (__syncthreads_or(greedy)) {
      // layer 1: the three action rows of agent slots SPT w .. + SPT - 1 at unit u
#pragma unroll
      for (int q = 0; q < SPT; ++q) {
        const int ag = SPT * w + q;
        const float4 x = shX[ag];
        float z = x.w * w13;
        z = fmaf(x.z, w12, z);
        z = fmaf(x.y, w11, z);
        z = fmaf(x.x, w10, z);
        H1[ag][u] = relu(z + b1);
        H1[AGW + ag][u] = relu(fmaf(0.5f, w14, z) + b1);
        H1[2 * AGW + ag][u] = relu((z + w14) + b1);
      }
      __syncthreads();
      f32x4 acc[MT];
#pragma unroll
      for (int rt = 0; rt < MT; ++rt) acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int rt = 0; rt < MT; ++rt) acc[rt] = mfma4(w2[kk], H1[16 * rt + c16][4 * kk + g4], acc[rt]);
      float sq[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int rt = 0; rt < MT; ++rt) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = relu(acc[rt][q] + b2[q]) * w3[q];
        sq[rt] = (v[0] + v[1]) + (v[2] + v[3]);  // wave_sum's tree: 4 units in-lane, ...
      }
      qpart[w][16 * tag4 + c16] = reduce4_groups(sq[0], sq[1], sq[2], 0.0f);  // ... the 4 row groups
      __syncthreads();
    }
    P2PMG_STAMP(atr, alast, 2);
    if (agent_thr) {
      if (greedy) {
        // ActorModel.greedy_action rl.py:188-196: Q(obs, a) for a in (0, .5, 1), argmax (first max)
        float qv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int row = AGW * k + j;
          qv[k] = ((qpart[0][row] + qpart[1][row]) + (qpart[2][row] + qpart[3][row])) + b3;
        }
        act = 0;
        float best = qv[0];
        if (qv[1] > best) { best = qv[1]; act = 1; }
        if (qv[2] > best) act = 2;
      } else {
        act = code;
      }
      hp = act == 0 ? lv.x : (act == 1 ? lv.y : lv.z);  // heating.set_power(action) -> hp.power * max_power
      // RLAgent._divide_power agent.py:186-195 on out = balance * max_in + hp (agent.py:210)
      const float out = (bal * mi) + hp;
      const float so = sgn(out);
      float f[N];
      float tot = 0.0f;
#pragma unroll
      for (int jj = 0; jj < N; ++jj) {
        const float pw = -((jj == i || r == 0) ? 0.0f : P[jj * N + i]);
        f[jj] = (so != sgn(pw)) ? pw : 0.0f;
        tot = tot + f[jj];
      }
      tot = fabsf(tot);
      float* Pn = shP[cur ^ 1] + sl * N * N + i * N;
#pragma unroll
      for (int jj = 0; jj < N; ++jj) {
        float v;
        if (tot == 0.0f) v = div_n<N>(out * 1.0f);
        else v = (jj == i) ? (tot == tot ? out * 0.0f : tot) : (out * fabsf(f[jj])) / tot;
        Pn[jj] = v;
      }
      if (p.record & 32) act_pack |= (uint64_t)act << (8 * r);  // stored with the other records at the end
    }
    __syncthreads();
    cur ^= 1;
    P2PMG_STAMP(atr, alast, 3);
  }
  // the step's stores all go out at the end of the kernel, after the replay draws: nothing after them
  // waits on vmcnt (which counts stores and loads alike)
  float g = 0.0f, pp = 0.0f, cost = 0.0f, rw = 0.0f, tin0 = tin;
  if (agent_thr) {
    // CommunityMicrogrid._assign_powers community.py:45-54 (final P, diagonal kept)
    const float* P = shP[cur] + sl * N * N;
#pragma unroll
    for (int jj = 0; jj < N; ++jj) {
      const float pij = P[i * N + jj], pji = P[jj * N + i];
      const float ex = __builtin_amdgcn_fmed3f(pij, -pji, 0.0f);  // pair_exchange (p2pmg_kernels.hip)
      g = g + (pij - ex);
      pp = pp + ex;
    }
    const Settled st = settle(p, g, pp, buy, inj, p2pp, tin, tp, penw);
    cost = st.cost;
    rw = st.rw;
    // HPHeating.step heating.py:138-143 at the agent's COP
    const RcParams rc{p.inv_ci, p.inv_cm, p.inv_ri, p.inv_re, p.inv_rvent, p.c_in, p.c_m, p.solar, tp.w, p.spm, p.slot};
    rc_update(rc, t_out, hp, tin, tm);
    shR[j] = rw;
  }
  __syncthreads();
  P2PMG_STAMP(atr, alast, 4);
  float ep = 0.0f;
  if (tid < SPW) {  // avg_reward = sum_t mean_i r (community.py:179), canonical order
    float m = 0.0f;
#pragma unroll
    for (int jj = 0; jj < N; ++jj) m = m + shR[tid * N + jj];
    ep = shEp[tid] + div_n<N>(m);
  }
  // Trainer.train -> ReplayBuffer.sample_batch (rl.py:299-305, 226-241) right after the append
  // (agent.py:338-342).  Floyd's draw j keeps r_j unless an earlier draw l < j ended on r_j, when it
  // takes count - 32 + j.  Sixteen threads per agent (draws q and q + 16) solve that recurrence as a
  // fixpoint over the agent's 32 indices in LDS: every pass recomputes each draw from the current
  // indices of the earlier ones, so after pass k the first k draws are final and a pass that changes
  // nothing has reached the sequential result (typically 2 passes instead of 32 serial steps).
  if (p.mode == 0 && d.fused_sample) {
    // AGW = 16: 16 threads per agent, draws q0 and q0 + 16; AGW = 8: 32 threads per agent, one draw
    // each (the second draw duplicates the first: same result, written twice)
    constexpr int TPA = 256 / AGW;
    const int aj = tid / TPA, q0 = tid % TPA, q1 = TPA == 16 ? q0 + 16 : q0;
    const bool va = aj < AG && s0 + aj / N < p.S;
    const int a2 = va ? s0 * N + aj : 0;
    const int n_add = va ? shN[aj] : kB;
    const int count = n_add < d.cap ? n_add : d.cap;
    const int fm = (n_add - count) % d.cap;  // ring slot of the deque's first element
    int i0, i1;
    if (d.samples) {
      i0 = va ? (int)d.samples[((size_t)t * A + a2) * kB + q0] : 0;
      i1 = va ? (int)d.samples[((size_t)t * A + a2) * kB + q1] : 0;
    } else {
      int r[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 1 && TPA != 16) {
          r[1] = r[0];
          break;
        }
        const int q = h ? q1 : q0;
        uint32_t c0 = (uint32_t)t, c1 = (uint32_t)p.episode, c2 = p.agent_offset + (uint32_t)a2, c3 = kTagSample + (uint32_t)q;
        philox4x32_10(c0, c1, c2, c3, p.seed_lo, p.seed_hi);
        r[h] = (int)__umulhi(c0, (uint32_t)(count - kB + q + 1));
      }
      i0 = r[0];
      i1 = r[1];
      shI[aj][q0] = i0;
      shI[aj][q1] = i1;
      if (tid == 0) shFlag[0] = 0;
      __syncthreads();
      // branch-free pass: bit l of hit_h says draw l's current index equals r_h; only l < q counts
      const uint32_t early0 = (1u << q0) - 1u, early1 = (q1 == 31 ? 0x7FFFFFFFu : (1u << q1) - 1u);
      for (int pass = 0;; ++pass) {
        uint32_t hit0 = 0u, hit1 = 0u;
#pragma unroll
        for (int v = 0; v < kB / 4; ++v) {
          const int4 x = *reinterpret_cast<const int4*>(&shI[aj][4 * v]);
          const int xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            hit0 |= xs[e] == r[0] ? 1u << (4 * v + e) : 0u;
            hit1 |= xs[e] == r[1] ? 1u << (4 * v + e) : 0u;
          }
        }
        const int n0 = (hit0 & early0) ? count - kB + q0 : r[0], n1 = (hit1 & early1) ? count - kB + q1 : r[1];
        const bool ch = n0 != i0 || n1 != i1;
        __syncthreads();  // every read of this pass before any write
        i0 = n0;
        i1 = n1;
        shI[aj][q0] = i0;
        shI[aj][q1] = i1;
        if (ch) shFlag[pass & 1] = 1;
        if (tid == 0) shFlag[(pass + 1) & 1] = 0;
        __syncthreads();
        if (shFlag[pass & 1] == 0) break;  // workgroup-uniform: nothing changed in this pass
      }
    }
    if (va) {
      int* out = reinterpret_cast<int*>(d.smp) + (size_t)a2 * kB;
      const int sl0 = fm + i0, sl1 = fm + i1;
      out[q0] = sl0 >= d.cap ? sl0 - d.cap : sl0;
      out[q1] = sl1 >= d.cap ? sl1 - d.cap : sl1;
    }
  }
  if (agent_thr) {
    if (p.mode != 1) {
      // DQNAgent.save_memory agent.py:332-336 -> ReplayBuffer.add rl.py:208-212
      const int n_added = shN[j] - 1;
      float2* slot = reinterpret_cast<float2*>(d.buf + ((size_t)a * d.cap + (size_t)(n_added % d.cap)) * kTrans);
      const float av = act == 0 ? 0.0f : (act == 1 ? 0.5f : 1.0f);
      slot[0] = make_float2(time_t, tnorm);
      slot[1] = make_float2(bal, p2pf);
      slot[2] = make_float2(av, rw);
      slot[3] = make_float2(time_n, tnorm);  // next state: same (pre-update) temperature (community.py:161)
      slot[4] = make_float2(baln, 0.0f / mi);  // next state p2p = mean(zeros) / max_in
      d.added[a] = n_added + 1;
    }
    const size_t k = (size_t)t * A + a;
    if (p.record & 1) p.rec_reward[k] = rw;
    if (p.record & 2) p.rec_cost[k] = cost;
    if (p.record & 4) p.rec_grid[k] = g;
    if (p.record & 8) p.rec_p2p[k] = pp;
    if (p.record & 16) p.rec_tin[k] = tin0;
    if (p.record & 32)
      for (int r = 0; r < R1; ++r) p.rec_action[((size_t)t * R1 + r) * A + a] = (uint8_t)(act_pack >> (8 * r));
    p.t_in[a] = tin;
    p.t_m[a] = tm;
  }
  if (tid < SPW && s0 + tid < p.S) {
    d.ep_acc[s0 + tid] = ep;
    p.ep_reward[s0 + tid] = ep;
  }
#if P2PMG_TRACE
  P2PMG_STAMP(atr, alast, 5);
  if (l == 0 && w == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2) && (d.t == 50 || d.t == 51))
    printf("ACTTRACE blk %d t %d mode %d: prologue %llu agentA %llu forward %llu agentB %llu epilogue %llu sample %llu\n",
           (int)blockIdx.x, d.t, p.mode, (unsigned long long)atr[0], (unsigned long long)atr[1],
           (unsigned long long)atr[2], (unsigned long long)atr[3], (unsigned long long)atr[4],
           (unsigned long long)atr[5]);
#endif
}

}  // namespace

bool act_shared_mfma(const DqnParams& d) {
  // sizes the MFMA act kernel is built for (its action records pack 8 rounds)
  const bool mfma_n = ((d.e.N >= 1 && d.e.N <= 8) || d.e.N == 16) && d.e.R + 1 <= 8;
  // (a role context, N = 1 included, takes dqn_act_kernel: a wave of this kernel holds ONE network)
  return d.n_nets == 1 && !d.roles && !d.act_wave && mfma_n;
}

bool dqn_act_fuses_adam(const DqnParams& d) { return act_shared_mfma(d) && d.n_segs >= 1 && d.n_segs <= kActAdamSegs; }

hipError_t launch_dqn_act_shared(const DqnParams& d, hipStream_t st) {
  // one shared network: AGW agents per workgroup on MFMA tiles
  // AGW = 16 agent slots per workgroup (default), or 8 (d.act_agw, P2PMG_ACT_AGW=8: more, shorter
  // workgroups; N <= 8 only) -- the same results bit for bit.  A pending Adam step: AGW = 16.
  switch (d.e.N) {
#define P2PMG_DQN_ACT_SHARED(NN)                                                                                     \
  case NN: {                                                                                                         \
    constexpr int spw = 16 / NN;                                                                                     \
    if (d.adam_pending) {                                                                                            \
      hipLaunchKernelGGL((dqn_act_shared_kernel<NN, 16, true>), dim3((d.e.S + spw - 1) / spw), dim3(256), 0, st, d); \
    } else if (NN <= 8 && d.act_agw == 8) {                                                                          \
      constexpr int agw = NN <= 8 ? 8 : 16, spw8 = agw / NN;                                                         \
      hipLaunchKernelGGL((dqn_act_shared_kernel<NN, agw, false>), dim3((d.e.S + spw8 - 1) / spw8), dim3(256), 0, st, \
                         d);                                                                                         \
    } else {                                                                                                         \
      hipLaunchKernelGGL((dqn_act_shared_kernel<NN, 16, false>), dim3((d.e.S + spw - 1) / spw), dim3(256), 0, st, d); \
    }                                                                                                                \
    break;                                                                                                           \
  }
    P2PMG_DQN_ACT_SHARED(1) P2PMG_DQN_ACT_SHARED(2) P2PMG_DQN_ACT_SHARED(3) P2PMG_DQN_ACT_SHARED(4)
    P2PMG_DQN_ACT_SHARED(5) P2PMG_DQN_ACT_SHARED(6) P2PMG_DQN_ACT_SHARED(7) P2PMG_DQN_ACT_SHARED(8)
    P2PMG_DQN_ACT_SHARED(16)
#undef P2PMG_DQN_ACT_SHARED
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace p2pmg
