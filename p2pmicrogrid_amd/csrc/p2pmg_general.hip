// p2pmg_general.hip — episode_kernel, the general tabular episode kernel: any community size up to 64
// agents, any number of rounds, per-agent / shared / per-role tables, battery, every record.
#include "p2pmg_episode_step.h"

namespace p2pmg {
namespace {

// ----------------------------------------------------------------- the episode kernel
// One launch = one episode of T timesteps for every scenario (train_episode / run).
// Latency structure per step (one dependent Q gather per extra round):
//   * env rows, profiles and exploration codes are prefetched ahead;
//   * round 0 always sees P = 0, so its p2p index is the constant ip_zero and its Q row, like
//     the next-state row, is known as soon as the previous step's final action is: both are
//     issued right after that action, before the previous step's market/reward/TD work;
//   * a TD store that hits one of those prefetched rows patches the register copy.
// The shared-table forms sum their TD deltas in the workgroup's LDS hash (p2pmg_tabular.h).
// The proposal matrix P of one scenario (PRegs / PTile) and the run-time group sum are
// p2pmg_episode_step.h's, shared with policy_episode_kernel (p2pmg_policy.hip).
// MIRROR: the step body below (a round's p2p bin, _divide_power, the market, the cost and the reward) is
// restated, expression for expression, by that header's round_p2p_bin / divide_power / market_reward, which
// policy_episode_kernel calls and this kernel does not.  Any edit to those expressions here must be made there
// too (tests/test_gpu_policy_set.py compares the two kernels bit for bit after a capture).

// exploration code of round r >= 8 of step t (the 64-bit code word holds rounds 0..7): the replay
// word (r / 4) of the step, or Philox word k = t (R + 1) + r (p2pmg_device.h, oracle/philox.py)
__device__ __forceinline__ int late_code(const EpisodeParams& p, const uint32_t* codes_a, size_t step_off, int t,
                                         int r, int a, bool active, const EpsThr& e) {
  if (p.mode != 0 || !active) return 255;
  if (p.rng == 1)
    return (int)philox_round_code(t, p.R + 1, r, (uint32_t)p.episode, p.agent_offset + (uint32_t)a, e.thr, e.all,
                                  p.seed_lo, p.seed_hi);
  return (int)((codes_a[step_off + (size_t)(r >> 2) * p.A] >> (8 * (r & 3))) & 0xFFu);
}
// workgroup shape of the general kernel: one wave, or (shared table) kSqWaves waves around one LDS
// delta hash; the 64-agent tiles (33 KB per wave) take two
template <int NC, bool WIDE, bool SQ>
constexpr int general_wpb() {
  return SQ ? ((WIDE && NC > 32) ? 2 : kSqWaves) : 1;
}

// episode_kernel<NC, WIDE, QT, B20, SQ>: WIDE = false: N = NC agents per scenario compiled in
// (PRegs); WIDE = true: n = p.N <= NC agents (PTile), the community sizes 9..15 and 17..64.  Both
// sum over j = 0..n-1 in order from +0.0 and divide by n as IEEE quotients, so a scenario gives the
// same bits either way (tests/test_gpu_parity.py runs the tile form at the register form's sizes).
// ROLE (with SQ): one frozen table per agent position ("role") i instead of one for all: lane i
// reads table i and its delta keys are offset by i tables, inside a delta replica of n tables.
template <int NC, bool WIDE, typename QT, bool B20, bool SQ, bool ROLE = false>
__global__ __launch_bounds__((kWave * general_wpb<NC, WIDE, SQ>())) void episode_kernel(const EpisodeParams p) {
  constexpr int G = pow2ceil(NC);
  constexpr int SPW = kWave / G;
  static_assert(SQ || !ROLE, "per-role tables are a shared-table form");
  constexpr int WPB = general_wpb<NC, WIDE, SQ>();  // waves per workgroup
  constexpr int PW = WIDE ? SPW * 2 * PTile<NC>::kTile : (G > 8 ? SPW * NC * NC : 1);
  constexpr int RW = (WIDE || G > 8) ? SPW * NC : 1;
  __shared__ float shPall[WPB * PW];
  __shared__ float shRall[WPB * RW];
  __shared__ uint32_t hkey[SQ ? kSqSlots : 1];
  __shared__ unsigned long long hval[SQ ? kSqSlots : 1];

  const int wv = SQ ? (int)(threadIdx.x / kWave) : 0;
  const int lane = SQ ? (int)(threadIdx.x % kWave) : (int)threadIdx.x;
  float* const shP = shPall + wv * PW;  // this wave's exchange tiles
  float* const shR = shRall + wv * RW;
  const int sl = lane / G;
  const int i = lane % G;
  const int n = WIDE ? p.N : NC;  // agents per scenario
  const float nf = (float)n;
  // x / n (mean over the community, the even split): div_n's power-of-two multiply is the IEEE quotient
  auto divn = [&](float x) -> float {
    if constexpr (WIDE) return x / nf;
    else return div_n<NC>(x);
  };
  const int s = (blockIdx.x * WPB + wv) * SPW + sl;
  const bool in_group = i < n;
  const bool active = in_group && (s < p.S);
  const int a = active ? s * n + i : 0;
  const int s_env = p.n_env == 1 ? 0 : (s < p.S ? s : 0);
  const int T = p.T;
  const int R1 = p.R + 1;
  const int W = (R1 + 3) >> 2;
  const bool train = p.mode == 0;
  const bool margin_one = p.margin == 1.0f;
  const uint32_t rec = (uint32_t)p.record;
  const size_t A = (size_t)p.A;
  // loop constants in VGPRs (no SGPR spill reloads on the chain); setpoint, comfort band, COP, alpha,
  // gamma and the comfort weight are the agent's own (inactive and out-of-group lanes: agent 0's)
  const KC k = pin_constants(p, p.thermal[a], p.learn[a]);
  // the scenario's explore threshold for the in-kernel Philox draws (its own under p2pmg_run_episodes_eps)
  const EpsThr ethr = eps_of(p, active ? s : 0);
  const Dims<B20> D{k.nt, k.nT, k.nb, k.np};
  std::conditional_t<WIDE, PTile<NC>, PRegs<NC>> P;
  if constexpr (WIDE) {
    P.base = shP + sl * 2 * PTile<NC>::kTile;
    P.i = i;
    P.rd = 0;
    P.wr = 0;
    // lanes i >= n read columns and rows no put() writes (their results are dropped, but the values
    // reach idx_plain and a gather address): give them zeros, once
    for (int k2 = lane; k2 < PW; k2 += kWave) shP[k2] = 0.0f;
    wave_lds_fence();
  } else {
    P.sh = shP;
    P.i = i;
    P.sl = sl;
  }

  const uint32_t n_states = (uint32_t)(p.nt * p.nT * p.nb * p.np);
  constexpr bool shared = SQ;
  // per-role tables: at most 64 x 640,000 entries, so a role's key offset fits 32 bits well below
  // kSqEmpty; inactive and out-of-group lanes read role 0
  const uint32_t role_off = ROLE ? (uint32_t)(active ? i : 0) * n_states * kQPad : 0u;
  QT* __restrict__ q = reinterpret_cast<QT*>(p.q) + (shared ? (size_t)role_off : (size_t)a * n_states * kQPad);
  unsigned long long* const dbase = reinterpret_cast<unsigned long long*>(p.qdelta) +
      (shared ? (size_t)(blockIdx.x % kDeltaCopies) * (ROLE ? (size_t)n : (size_t)1) * n_states * kQPad : (size_t)0);
  if constexpr (SQ) {
    for (int k2 = threadIdx.x; k2 < kSqSlots; k2 += WPB * kWave) {
      hkey[k2] = kSqEmpty;
      hval[k2] = 0;
    }
    __syncthreads();
  }
  const float mi = active ? p.max_in[a] : 1.0f;
  const float4 lv = p.hp_lv[a];  // heat-pump power of actions 0..2 for this agent
  const bool bat = p.battery != 0;
  const double bcap = bat ? p.bat_cap[a] : 0.0;
  double soc = bat ? p.soc[a] : 0.0;
  float tin = active ? p.t_in[a] : k.setpoint;
  float tm = active ? p.t_m[a] : k.setpoint;
  // round 0 and the next state both have p2p = mean(-0 ... -0) / max_in = 0 (agent.py:203, community.py:161)
  const int ip_zero = idx_plain(divn(0.0f) / mi, D.p());

  // running offsets (no 64-bit multiplies in the loop)
  const float* envb = p.env + (size_t)s_env * kEnvStride;
  const size_t env_step = (size_t)p.n_env * kEnvStride;
  const size_t env_end = env_step * T;
  const float2* profb = p.prof + a;
  const size_t prof_end = A * T;
  auto prof_at = [&](size_t off) { return profb[off]; };  // inactive lanes read agent 0 (a = 0)
  const uint32_t* codes_a = p.codes + a;
  const size_t code_step = (size_t)W * A;
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
  size_t c1o = (T > 1) ? code_step : 0;  // code words of step t + 1 (wrapping to 0 on the last step)

  EnvRow e0 = load_env(envb);
  EnvRow e1 = load_env(envb + e1o);
  const float2 f0 = prof_at(0);
  float2 f1 = prof_at(f1o);
  StepIdx st = make_step(k, D, margin_one, e0.time, e1.time, FDIV(f0.x - f0.y, mi), f1, tin, mi, ip_zero);
  uint64_t cw = code_word(p, step_codes(p, codes_a, 0, 0, a, W, ethr), active);
  // Q rows are loaded unconditionally (a load under a divergent branch is waited for at the
  // join, which would serialise the prefetch); a row that is not needed aliases one that is
  // loaded anyway, so it costs no HBM traffic.  Inactive lanes read agent 0's table.
  auto row0_addr = [&](const StepIdx& x, uint64_t c) -> uint32_t {
    const bool need = ((c & 0xFF) == 255) || (train && R1 == 1);  // greedy, or the TD target itself
    return need ? x.strip + (uint32_t)ip_zero : x.nrow;
  };
  uint32_t a0 = row0_addr(st, cw);
  uint32_t aN = train ? st.nrow : a0;
  Row4<QT> row0 = gather_row(q + a0 * kQPad);
  Row4<QT> rowN = gather_row(q + aN * kQPad);
  Patch<QT> pat{0xFFFFFFFFu, 0, (QT)0};
  float ep_sum = 0.0f;
  size_t tA = 0;

  for (int t = 0; t < T; ++t, tA += A) {
    // prefetch ahead: env/profile two steps, exploration codes one step
#if P2PMG_ABLATE >= 3
    const EnvRow e2 = load_env(envb);
    const float2 f2 = prof_at(0);
#else
    const EnvRow e2 = load_env(envb + e2o);
    const float2 f2 = prof_at(f2o);
#endif
    const CodeWords cw1r = step_codes(p, codes_a, c1o, t + 1 == T ? 0 : t + 1, a, W, ethr);

    P.clear();
    int act = 0, ip = ip_zero;
    float hp = 0.0f;
    double soc_r = soc;  // tentative SoC of the current round
    row0 = patched(row0, a0, pat);  // the previous step's TD store may have hit a prefetched row
    rowN = patched(rowN, aN, pat);
    Row4<QT> rowR = row0;  // Q row of the final round's state (TD target Q[s, a])

    for (int r = 0; r < R1; ++r) {
      const int code = r < 8 ? (int)((cw >> (8 * r)) & 0xFF) : late_code(p, codes_a, tA * W, t, r, a, active, ethr);
      if (r > 0) {
        P.next_round();  // Jacobi: read the previous round's column (community.py:84-86)
        // powers = -P[:, i] with the diagonal zeroed (community.py:76,81); p2p = mean / max_in (agent.py:203)
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < n; ++j) acc = acc + (-((j == i) ? 0.0f : P.colv(j)));
        ip = idx_plain(FDIV(divn(acc), mi), D.p());
        // the final round's row is needed for the TD update even when exploring
        const bool need = code == 255 || (train && r == R1 - 1);
        rowR = gather_row(q + (need ? st.strip + (uint32_t)ip : a0) * kQPad);
      }
      act = code == 255 ? argmax3(rowR) : code;  // QAgent._act / take_decision (agent.py:271-289)
      hp = hp_of(lv, act);

      // RLAgent._divide_power agent.py:186-195 on out = bal * max_in + hp (agent.py:210);
      // with a battery the rule adjusts the net power first (SoC committed by the last round)
      float out = (st.bal * mi) + hp;
      if (bat && bcap > 0.0) {
        soc_r = soc;
        out = (float)battery_rule((double)out, soc_r, bcap, p.bat_min, p.bat_max, p.bat_sqrt_eff);
      }
      const float so = sgn(out);
      // filtered_j: powers_j where its sign differs from out's (agent.py:187-189)
      auto filt = [&](int j) -> float {
        const float pw = -((j == i || r == 0) ? 0.0f : P.colv(j));
        return (so != sgn(pw)) ? pw : 0.0f;
      };
      float tot = 0.0f;
#pragma unroll
      for (int j = 0; j < n; ++j) tot = tot + filt(j);
      tot = fabsf(tot);
      if (tot == 0.0f) {
        const float ev = divn(out * 1.0f);
#pragma unroll
        for (int j = 0; j < n; ++j) P.put(j, ev);
      } else {
        // |f_ii| = 0 (own power is -0): (out * 0) / tot == out * 0 exactly for any non-NaN tot
#pragma unroll
        for (int j = 0; j < n; ++j)
          P.put(j, (j == i) ? (tot == tot ? out * 0.0f : tot) : FDIV(nabs_out(out) * filt(j), tot));
      }
      if (active && (rec & 96u)) {
        const size_t kk = (tA * R1) + (size_t)r * A;
        if (rec & 32u) rec_action[kk] = (uint8_t)act;
        if (rec & 64u) rec_index[kk] = st.it | (st.iT << 8) | (st.ib << 16) | (ip << 24);
      }
    }

    soc = soc_r;  // BatteryStorage state after the final round's decision
    // CommunityMicrogrid._step -> HPHeating.step (community.py:184-188, heating.py:138-143):
    // computed now so the next step's rows can be issued before this step's market work
    float tin1 = tin, tm1 = tm;
    rc_update(k, e0.t_out, hp, tin1, tm1);
    // (after the last step this prefetches a wrapped, unused step: harmless valid addresses)
    const StepIdx st1 = make_step(k, D, margin_one, e1.time, e2.time, st.baln, f2, tin1, mi, ip_zero);
    const uint64_t cw1 = code_word(p, cw1r, active);
    const uint32_t a0n = row0_addr(st1, cw1);
    const uint32_t aNn = train ? st1.nrow : a0n;
    const Row4<QT> row0n = gather_row(q + a0n * kQPad);
    const Row4<QT> rowNn = gather_row(q + aNn * kQPad);
    pat.row = 0xFFFFFFFFu;

    // CommunityMicrogrid._assign_powers community.py:45-54 on the final P (diagonal kept)
    P.next_round();
    float g = 0.0f, pp = 0.0f;
#pragma unroll
    for (int j = 0; j < n; ++j) {
      const float pij = P.rowv(j), pji = P.colv(j);
      const float ex = pair_exchange(pij, pji);
      g = g + (pij - ex);
      pp = pp + ex;
    }
    // CommunityMicrogrid._compute_costs community.py:56-65
    float cost = (g >= 0.0f) ? g * e0.buy : g * e0.inj;
    cost = cost + pp * e0.p2p;
    cost = FDIV(cost * k.slot, k.mph);
    cost = cost * k.kilo;
    // RLAgent.get_reward agent.py:225-232 (pre-update T_in)
    float pen = fmaxf(fmaxf(0.0f, k.lower - tin), fmaxf(0.0f, tin - k.upper));
    pen = pen > 0.0f ? pen + 1.0f : 0.0f;
    const float rw = -(cost + k.penw * pen);

    if (train && active && !shared) {
      // QAgent.train agent.py:293-298 -> QActor.train rl.py:119-129
      const uint32_t srow = st.strip + ip;
      const QT qsa = sel3(act, rowR.v[0], rowR.v[1], rowR.v[2]);
      const QT qnew = td_update(qsa, rw, max3(rowN), k.alpha, k.gamma);
      q[srow * kQPad + act] = qnew;
      pat = Patch<QT>{srow, act, qnew};  // rows issued before this store see the old value
    }
    if (shared && train && active) {
      // frozen shared table: delta = alpha * ((r + gamma * max Q[ns]) - Q[s, a]) in f64, summed in
      // int64 fixed point (order-independent, so every launch and every rank sums identically)
      const QT qsa = sel3(act, rowR.v[0], rowR.v[1], rowR.v[2]);
      const double d = k.alpha * (((double)rw + k.gamma * (double)max3(rowN)) - (double)qsa);
      const long long v = __double2ll_rn(d * kDeltaScale);
#if P2PMG_ABLATE == 5
      if (v == 12345)  // timing-only: drop the accumulation (never true in practice)
#endif
      lds_add_by_key(hkey, hval, role_off + (st.strip + (uint32_t)ip) * kQPad + (uint32_t)act, v, dbase);
    }
    if (active && (rec & 31u)) {
      if (rec & 1u) rec_reward[tA] = rw;
      if (rec & 2u) rec_cost[tA] = cost;
      if (rec & 4u) rec_grid[tA] = g;
      if (rec & 8u) rec_p2p[tA] = pp;
      if (rec & 16u) rec_tin[tA] = tin;
    }
    // avg_reward = sum_t mean_i r (community.py:179), canonical sequential order
    float m;
    if constexpr (WIDE) m = group_sum_n<NC>(rw, i, sl, n, shR);
    else m = group_sum<NC>(rw, lane, i, sl, shR);
    ep_sum = ep_sum + divn(m);
    if constexpr (SQ) {
      if (train && (t % kSqFlushSteps == kSqFlushSteps - 1 || t + 1 == T)) lds_hash_flush(hkey, hval, dbase, WPB * kWave);
    }

    tin = tin1;
    tm = tm1;
    e0 = e1;
    e1 = e2;
    f1 = f2;
    e2o = adv(e2o, env_step, env_end);
    f2o = adv(f2o, A, prof_end);
    c1o = (t + 2 >= T) ? (size_t)0 : c1o + code_step;
    st = st1;
    cw = cw1;
    a0 = a0n;
    aN = aNn;
    row0 = row0n;
    rowN = rowNn;
  }
  if (active) {
    p.t_in[a] = tin;
    p.t_m[a] = tm;
    if (bat) p.soc[a] = soc;
    if (i == 0) p.ep_reward[s] = ep_sum;
  }
}

template <int NC, bool WIDE, typename QT, bool SQ, bool ROLE = false>
void launch_nq(const EpisodeParams& p, hipStream_t st) {
  constexpr int SPW = kWave / pow2ceil(NC);
  constexpr int WPB = general_wpb<NC, WIDE, SQ>();
  const int waves = (p.S + SPW - 1) / SPW;
  const int blocks = (waves + WPB - 1) / WPB;
  if (p.nt == 20 && p.nT == 20 && p.nb == 20 && p.np == 20)
    hipLaunchKernelGGL((episode_kernel<NC, WIDE, QT, true, SQ, ROLE>), dim3(blocks), dim3(kWave * WPB), 0, st, p);
  else
    hipLaunchKernelGGL((episode_kernel<NC, WIDE, QT, false, SQ, ROLE>), dim3(blocks), dim3(kWave * WPB), 0, st, p);
}

template <int NC, bool WIDE, typename QT>
hipError_t launch_n(const EpisodeParams& p, hipStream_t st) {
  if (p.shared_q)
    launch_nq<NC, WIDE, QT, true>(p, st);
  else
    launch_nq<NC, WIDE, QT, false>(p, st);
  return hipGetLastError();
}

// N compiled in (registers): N in {1..8, 16}
template <int N>
hipError_t launch_nd(const EpisodeParams& p, int q_dtype, hipStream_t st) {
  return q_dtype == 0 ? launch_n<N, false, double>(p, st) : launch_n<N, false, float>(p, st);
}
// any N <= NC at run time (LDS tiles)
template <int NC>
hipError_t launch_wide(const EpisodeParams& p, int q_dtype, hipStream_t st) {
  if (p.N < 1 || p.N > NC) return hipErrorInvalidValue;
  return q_dtype == 0 ? launch_n<NC, true, double>(p, st) : launch_n<NC, true, float>(p, st);
}

// per-role tables (shared_q = 2): the shared-table form with a table per agent position
template <int N>
hipError_t launch_role_nd(const EpisodeParams& p, int q_dtype, hipStream_t st) {
  if (q_dtype == 0) launch_nq<N, false, double, true, true>(p, st);
  else launch_nq<N, false, float, true, true>(p, st);
  return hipGetLastError();
}
template <int NC>
hipError_t launch_role_wide(const EpisodeParams& p, int q_dtype, hipStream_t st) {
  if (p.N < 1 || p.N > NC) return hipErrorInvalidValue;
  if (q_dtype == 0) launch_nq<NC, true, double, true, true>(p, st);
  else launch_nq<NC, true, float, true, true>(p, st);
  return hipGetLastError();
}

}  // namespace

// _build.py compiles this file once per slice (-DP2PMG_GENERAL_SLICE=k, in parallel): a slice defines one
// of the launchers below, so each episode_kernel instantiation is compiled in one slice only; slice 0
// (also what an undefined macro selects) holds the dispatcher as well.
#if P2PMG_GENERAL_SLICE == 0
hipError_t launch_general_n1_4(const EpisodeParams& p, int q_dtype, hipStream_t stream) {
  switch (p.N) {
    case 1: return launch_nd<1>(p, q_dtype, stream);
    case 2: return launch_nd<2>(p, q_dtype, stream);
    case 3: return launch_nd<3>(p, q_dtype, stream);
    case 4: return launch_nd<4>(p, q_dtype, stream);
    default: return hipErrorInvalidValue;
  }
}
#endif
#if P2PMG_GENERAL_SLICE == 1
hipError_t launch_general_n5_8(const EpisodeParams& p, int q_dtype, hipStream_t stream) {
  switch (p.N) {
    case 5: return launch_nd<5>(p, q_dtype, stream);
    case 6: return launch_nd<6>(p, q_dtype, stream);
    case 7: return launch_nd<7>(p, q_dtype, stream);
    case 8: return launch_nd<8>(p, q_dtype, stream);
    default: return hipErrorInvalidValue;
  }
}
#endif
#if P2PMG_GENERAL_SLICE == 2
hipError_t launch_general_n16(const EpisodeParams& p, int q_dtype, hipStream_t stream) {
  return p.N == 16 ? launch_nd<16>(p, q_dtype, stream) : hipErrorInvalidValue;
}
#endif
#if P2PMG_GENERAL_SLICE == 3
hipError_t launch_general_tile16(const EpisodeParams& p, int q_dtype, int nc, hipStream_t stream) {
  return nc == 16 ? launch_wide<16>(p, q_dtype, stream) : hipErrorInvalidValue;
}
#endif
#if P2PMG_GENERAL_SLICE == 4
hipError_t launch_general_tile32_64(const EpisodeParams& p, int q_dtype, int nc, hipStream_t stream) {
  return nc == 32 ? launch_wide<32>(p, q_dtype, stream) : nc == 64 ? launch_wide<64>(p, q_dtype, stream)
                                                                   : hipErrorInvalidValue;
}
#endif
#if P2PMG_GENERAL_SLICE == 5
hipError_t launch_role_n1_4(const EpisodeParams& p, int q_dtype, hipStream_t stream) {
  switch (p.N) {
    case 1: return launch_role_nd<1>(p, q_dtype, stream);
    case 2: return launch_role_nd<2>(p, q_dtype, stream);
    case 3: return launch_role_nd<3>(p, q_dtype, stream);
    case 4: return launch_role_nd<4>(p, q_dtype, stream);
    default: return hipErrorInvalidValue;
  }
}
#endif
#if P2PMG_GENERAL_SLICE == 6
hipError_t launch_role_n5_8(const EpisodeParams& p, int q_dtype, hipStream_t stream) {
  switch (p.N) {
    case 5: return launch_role_nd<5>(p, q_dtype, stream);
    case 6: return launch_role_nd<6>(p, q_dtype, stream);
    case 7: return launch_role_nd<7>(p, q_dtype, stream);
    case 8: return launch_role_nd<8>(p, q_dtype, stream);
    default: return hipErrorInvalidValue;
  }
}
#endif
#if P2PMG_GENERAL_SLICE == 7
hipError_t launch_role_n16_tile16(const EpisodeParams& p, int q_dtype, int nc, hipStream_t stream) {
  if (nc == 0) return p.N == 16 ? launch_role_nd<16>(p, q_dtype, stream) : hipErrorInvalidValue;
  return nc == 16 ? launch_role_wide<16>(p, q_dtype, stream) : hipErrorInvalidValue;
}
#endif
#if P2PMG_GENERAL_SLICE == 8
hipError_t launch_role_tile32_64(const EpisodeParams& p, int q_dtype, int nc, hipStream_t stream) {
  return nc == 32 ? launch_role_wide<32>(p, q_dtype, stream) : nc == 64 ? launch_role_wide<64>(p, q_dtype, stream)
                                                                        : hipErrorInvalidValue;
}
#endif
#if P2PMG_GENERAL_SLICE == 0
// the general kernel: registers for N in {1..8, 16}, LDS tiles for every other N <= 64 (and for any
// N <= 64 when tile != 0, the cross-check of the two forms)
hipError_t launch_episode(const EpisodeParams& p, int q_dtype, int tile, hipStream_t stream) {
  if (p.N < 1 || p.N > kMaxAgents) return hipErrorInvalidValue;
  if (p.shared_q == 2) {  // per-role tables
    if (!tile) {
      if (p.N <= 4) return launch_role_n1_4(p, q_dtype, stream);
      if (p.N <= 8) return launch_role_n5_8(p, q_dtype, stream);
      if (p.N == 16) return launch_role_n16_tile16(p, q_dtype, 0, stream);
    }
    const int nc = general_tile_cap(p.N);
    return nc == 16 ? launch_role_n16_tile16(p, q_dtype, nc, stream) : launch_role_tile32_64(p, q_dtype, nc, stream);
  }
  if (!tile) {
    if (p.N <= 4) return launch_general_n1_4(p, q_dtype, stream);
    if (p.N <= 8) return launch_general_n5_8(p, q_dtype, stream);
    if (p.N == 16) return launch_general_n16(p, q_dtype, stream);
  }
  const int nc = general_tile_cap(p.N);
  return nc == 16 ? launch_general_tile16(p, q_dtype, nc, stream) : launch_general_tile32_64(p, q_dtype, nc, stream);
}
#endif

}  // namespace p2pmg
