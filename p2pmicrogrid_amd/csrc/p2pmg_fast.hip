// p2pmg_fast.hip — episode_fast_kernel, the latency-bound per-agent-table path (N <= 8, R + 1 <= 4).
#include "p2pmg_fastmath.h"

namespace p2pmg {
namespace {

// ----------------------------------------------------------------- the fast per-agent-table path
// timing-only ablations of the fast kernel's gathers: 7 = round-R gather fake, 8 = prefetched rows fake
template <typename QT>
__device__ __forceinline__ Row4<QT> fake_row(const QT* p) {
  const uint32_t x = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 5);
  return Row4<QT>{{(QT)(x & 3), (QT)((x >> 2) & 3), (QT)((x >> 4) & 3), (QT)0}};
}

// round 1 after an all-even round 0: every lane's row is ev (agent.py:190-191), so the column is
// the group's ev values (one shuffle per partner instead of a row exchange)
template <int N, int D, int G>
__device__ __forceinline__ void gather_even(float ev, float (&col)[N], int i) {
  if constexpr (D < G) {
    const float got = shfl_xor_c<D>(ev);
    const int src = i ^ D;
#pragma unroll
    for (int k = 0; k < N; ++k) col[k] = (k == src) ? got : col[k];
    gather_even<N, D + 1, G>(ev, col, i);
  }
}

// episode_fast_kernel: episode_kernel's per-agent-table path (no shared table, G <= 8,
// R + 1 <= 4, or <= 2 with a battery, code words from a pre-pass) with the rounds unrolled at compile time and the
// policy-independent per-step work (balance, time / balance bins, the next state's bins) read
// from step_prepass_kernel's output.  Same op order, same results, bit for bit (tests compare
// both kernels with the oracle).  Latency structure per step:
//   * round 0 always sees P = 0: its row and the next-state row are issued at the end of the
//     previous step (as in episode_kernel), round 0 is an even split, and round 1's column is
//     the group's round-0 even values;
//   * the next step's pre-pass word, env row and code word are issued right after the dependent
//     round-R gather, so waiting for that gather never waits for them (vmcnt counts in order);
//   * every store is unconditional (inactive lanes and disabled records write a per-lane dummy
//     slot), so the number of memory ops behind each load is static and the loop-top wait for
//     the prefetched rows is vmcnt(3), not a vmcnt(0) drain of the step's stores;
//   * records go out as ONE 32-B row per agent-step (FastRec), or as an 8-B {reward, cost} row
//     when only those are requested, and are unpacked on request;
//   * division by max_in / 60 / N uses the hoisted reciprocal (fdiv_b, p2pmg_fastmath.h);
//   * BAT (configs[3] mixes): every round's net power goes through the battery rule first (f64,
//     SoC committed by the final round, agent.py:138-153), with the capacity / sqrt(eff) / 900 s
//     divisions through hoisted reciprocals (battery_rule_r); agents with capacity 0 skip it.
// spw = scenarios per wave (<= 64 / G): fewer scenarios per wave spread the waves over more CUs.
#ifndef P2PMG_BAT_SPEC  // 1: the final round's battery rule for all 3 actions inside its row's round trip
#define P2PMG_BAT_SPEC 1  // configs[3] 59.6 -> 58.7 ms (profiles/r04_battery_ab.txt)
#endif
// BAT: 0 none, 1 battery with per-lane range tests, 2 battery in the launcher-verified domain
// KG > 1 (PIPE; chained training launches, no battery; the plan's `groups`): KG = 2 or 4 chained episodes
// per wave, in KG lane groups of 64 / KG lanes.  Group g runs episodes g, g + KG, g + 2 KG, ... of the SAME
// agents as every other group, in lockstep, L = T / KG steps behind group g - 1.  What follows describes
// KG = 2 (lanes 0-31 and 32-63, half an episode apart); the last paragraph says what KG = 4 adds.
// An agent's consecutive episodes are
// coupled only through its table (the later one starts from its own T0 draw), and the launcher sends
// this form only inputs whose hazard distance keeps every conflicting pair of row accesses at least
// four steps apart in the order of the serial chain (chain_lag_kernel).  Lockstep time runs in phases
// of L steps; at a phase boundary one half is at an episode boundary and runs the epilogue and the
// prologue under a divergent branch.  What was wave-uniform per episode (step offsets, code-word
// base) is per lane.  The one access whose serial order cannot be kept, step T - 1's next-state
// row (key of step 0, which the follower episode has been writing since its own step 0), is served
// from the follower's undo log: the first time the follower stores into a row (key of step 0,
// temperature bin, p2p = 0) it leaves max3 of the row as it read it in LDS (one slot per half and
// bin, one bit per bin in a per-lane mask), and the leader's step T - 1 takes that value where the
// bit is set and its own loaded row where it is clear.  The hazard rule puts every such store at least
// four steps before the leader loads the row, and every leader store to those rows before the
// follower's first read, so the logged value is what the serial chain reads.
//
// KG = 4 (a quarter episode apart; the launcher sends T % 12 == 0 and D + 4 <= T / 4).  Episode e lives in
// group e % 4 for its whole life; in phase ph group ph % 4 is at an episode boundary and group (ph + 1) % 4
// in its episode's last quarter; the loop ends after phase n_chain + 2, and a group without an episode
// (fill, drain) runs masked to the dummy slots.  Hazards: steps u of episode e and v of episode e + j run at
// lockstep times u and j L + v.  A conflicting pair (chain_lag_kernel) has u - v <= D <= L - 4 <= j L - 4, so
// u's access precedes v's by at least four steps for j = 1, and by more for j = 2, 3: adjacent episodes
// decide.  The wrap row of episode e (key of step 0, bin iT of its step T - 1, p2p = 0) may by then hold
// stores of e + 1, e + 2 (earlier phases) and e + 3 (this phase; every step on step 0's key is a step
// v <= D <= L - 4 of its episode, so it ran before this lockstep step).  Each group keeps its own log and
// mask for the life of its episode (reset in its own prologue), and the leader takes the value of the
// EARLIEST follower that logged the bin: group grp + 1's, else grp + 2's, else grp + 3's, else its own
// loaded row.  Why that is the serial value: a follower's first read of the row runs at least L >= D + 4
// steps after the last store of every earlier episode to a row of that key (those are steps <= D of
// episodes that began at least L steps before it), so it has seen them all; if no earlier follower stored
// into the row, what it read is what episode e left, which is what the serial chain reads at e's step
// T - 1 (e's own stores to the key are steps <= D of its first quarter).  If no follower logged the bin,
// none stored into the row and the loaded row is the serial one.  Whether a follower's store has landed
// when the row is loaded does not matter: the loaded row is used only where no follower stored at all.
template <int N, typename QT, int R1, bool TRAIN, int BAT, bool NARROW, int KG = 1>
__global__ __launch_bounds__(kWave) void episode_fast_kernel(const EpisodeParams p, const uint2* __restrict__ pre,
                                                             FastRec* __restrict__ recs, int spw, int n_cons,
                                                             const PrepOut nxt) {
  // Blocks past the consumer grid are producers: the next episode's step pre-pass (speculating the
  // same epsilon), run beside this episode's latency-bound waves on otherwise idle SIMDs, so the
  // next launch needs neither a pre-pass launch nor a cross-stream wait.
  if ((int)blockIdx.x >= n_cons) {
    const size_t n = (size_t)p.T * p.A, stride = (size_t)(gridDim.x - n_cons) * kWave;
    const int n_ep = nxt.n_ep > 1 ? nxt.n_ep : 1;  // the next launch's chain
    for (int ep = 0; ep < n_ep; ++ep)
      for (size_t k2 = (size_t)(blockIdx.x - n_cons) * kWave + threadIdx.x; k2 < n; k2 += stride)
        prepass_one(p, nxt, k2, ep);
    return;
  }
  constexpr int G = pow2ceil(N);
  static_assert(G <= 8 && R1 >= 1 && R1 <= 4, "fast path: G <= 8, R + 1 <= 4");
  constexpr bool PIPE = KG > 1;    // KG lane groups, each running its own episode of the chain
  constexpr int GW = kWave / KG;   // lanes per group
  static_assert(KG == 1 || KG == 2 || KG == 4, "lane groups per wave: 1 (off), 2 or 4");
  static_assert(!PIPE || (TRAIN && BAT == 0), "several episodes per wave: chained training launches without a battery");
  static_assert(!PIPE || GW % G == 0, "a scenario's lanes stay inside one group");
  // N = 2: round 1's Q row is one of three (by the partner's round-0 action) whose bins the
  // pre-pass wrote; all three are issued a step ahead, so round 1 waits for no gather
  // (not with a battery: the partner's round-0 power then depends on its state of charge)
  constexpr bool CAND = N == 2 && R1 >= 2 && BAT == 0;
  const int lane = (int)threadIdx.x;
  const int grp = PIPE ? lane / GW : 0;    // PIPE: the lane group (episodes grp, grp + KG, ... of the chain)
  const int hl = PIPE ? lane % GW : lane;  // ... and the lane inside it: every exchange stays inside a group
  const int sl = hl / G;
  const int i = hl % G;
  const int s = (int)blockIdx.x * spw + sl;
  const bool active = i < N && sl < spw && s < p.S;
  const int a = active ? s * N + i : 0;
  const int s_env = p.n_env == 1 ? 0 : (active ? s : 0);
  const int T = p.T;
  const size_t A = (size_t)p.A;
  // the agent's setpoint, comfort band and COP, and its learner's alpha, gamma and comfort weight:
  // loaded here, before the chain loop, with hp_lv[a], max_in[a] and t_in[a]; the step loop reads them
  // as the VGPRs the pinned arguments were
  const KC k = pin_constants(p, p.thermal[a], p.learn[a]);
  const uint32_t n_states = (uint32_t)(p.nt * p.nT * p.nb * p.np);
  QT* __restrict__ q = reinterpret_cast<QT*>(p.q) + (size_t)a * n_states * kQPad;  // TD stores
  // Row gathers as ONE 32-bit offset from the wave's first table (global_load's SGPR-base + VGPR-offset
  // form: a v_lshl_add_u32 per row instead of a 64-bit address on the act -> gather chain).  The
  // launcher only sends this kernel tables whose 64-lane span fits 4 GiB.  Masked-off lanes read the
  // wave's first table.
  const int a_first = (int)blockIdx.x * spw * N;
  constexpr uint32_t kRowShift = sizeof(QT) == 8 ? 5 : 4;  // padded row: 32 B (f64) / 16 B (f32)
  const char* const qwave = reinterpret_cast<const char*>(p.q) + ((size_t)a_first * n_states << kRowShift);
  const uint32_t qlane = active ? (uint32_t)(a - a_first) * (n_states << kRowShift) : 0u;
  auto gat = [&](uint32_t row) __attribute__((always_inline)) {
    return gather_row(reinterpret_cast<const QT*>(qwave + (qlane + (row << kRowShift))));
  };
  const int np = k.np;
  const int nbv = k.nb;
  const float km1_T = (float)(k.nT - 1), km2_T = (float)(k.nT - 2), km1_p = (float)(np - 1), kp = (float)np;
  const float mi = active ? p.max_in[a] : 1.0f;
  const Recip rmi = recip(mi), rmph = recip(k.mph), rn = recip((float)N);
  const float4 lv = p.hp_lv[a];
  // the heat-pump terms of heating.py:44-45 per action: (c_in hp) cop and (c_m hp) cop, the same ops
  // rc_update applies to the chosen level, hoisted out of the episode
  const float hin[3] = {(k.c_in * lv.x) * k.cop, (k.c_in * lv.y) * k.cop, (k.c_in * lv.z) * k.cop};
  const float hm[3] = {(k.c_m * lv.x) * k.cop, (k.c_m * lv.y) * k.cop, (k.c_m * lv.z) * k.cop};
  float tin = active ? p.t_in[a] : k.setpoint;
  float tm = active ? p.t_m[a] : k.setpoint;
  double bcap = 0.0, soc = 0.0;
  BatK bk{};
  Recip64 rcap{};
  if constexpr (BAT != 0) {
    bcap = active ? p.bat_cap[a] : 0.0;
    soc = active ? p.soc[a] : 0.0;
    bk = BatK{p.bat_min, p.bat_max, p.bat_sqrt_eff, recip64_u(p.bat_sqrt_eff), kR900};
    rcap = recip64(bcap > 0.0 ? bcap : 1.0);
  }
  const int ip_zero = idx_plain(div_n<N>(0.0f) / mi, np);  // round 0 and next state: p2p = 0 (agent.py:203)
  // stores of inactive lanes (and every record when none is requested) go to a per-lane dummy slot
  QT* const q_dummy = reinterpret_cast<QT*>(p.dummy) + lane * kQPad;
  // records: FastRec rows, or only {reward, cost} as float2 when nothing else was requested.
  // A compile-time choice: with a run-time branch between the two store sequences the compiler's
  // vmcnt bookkeeping takes the shortest path through the branch, and the mid-step wait for the
  // round-1 rows then also waits for the previous step's TD store to complete (an HBM write ack).
  constexpr bool narrow = NARROW;
  const size_t rec_bytes = narrow ? sizeof(float2) : sizeof(FastRec);
  char* const rec_dummy = reinterpret_cast<char*>(reinterpret_cast<FastRec*>(p.dummy) + kWave + lane);
  const bool rec_on = p.record != 0 && active;
  const size_t rec_step = rec_on ? A * rec_bytes : 0;

  // idx_temp((T_in - setpoint) / margin) heating.py:118-120, rl.py:93; the launcher sends this
  // kernel the reference's margin of 1 only (x / 1 == x exactly), other margins take episode_kernel
  auto temp_bin = [&](float t_in) {
    const float x = t_in - k.setpoint;
    return clamp_bin_f(((x + 1.0f) / 2.0f) * km2_T + 1.0f, km1_T);
  };
  auto p2p_bin = [&](float x) { return clamp_bin_f(((x + 1.0f) / 2.0f) * kp, km1_p); };

  const float* envb = p.env + (size_t)s_env * kEnvStride;
  const size_t env_step = (size_t)p.n_env * kEnvStride;
  const uint2* preb = pre + a;
  const uint32_t* ipc_a = p.pre_ipc + a;  // read only when CAND
  const int t1 = T > 1 ? 1 : 0, t2 = 2 % T;
  // A chained launch runs p.chain episodes back to back in every wave (no launch boundary between
  // them, and each wave starts its next episode as soon as its own ends): T_in / T_m carry over
  // in registers (with the end-of-episode T0 reset when requested), the Q rows through memory.
  const int n_chain = p.chain > 1 ? p.chain : 1;
  // The state of the episode a lane runs: set by begin_episode, advanced by step.  PIPE: the two
  // halves of the wave are L steps apart, so all of it is per lane there.
  bool st_on = active;           // the lane stores (PIPE: and its half has an episode running)
  size_t rec_adv = rec_step;     // record pointer advance per step
  bool wrap_l = false;           // PIPE: this lane's step T - 1 takes max3 of the next-state row from the follower's log
  bool wrap_it = false;          // PIPE: the loop's last iteration of a phase (uniform)
  // PIPE: the undo log of the rows (key of step 0, temperature bin, p2p = 0) this lane's episode has
  // stored into: max3 of each row as first read, [KG groups][32 bins][GW lanes] and a dummy slot per lane
  // (a step that logs nothing writes there: the LDS store is unconditional); bit iT of wlog_m = logged
  QT* wlog = nullptr;
  uint32_t* wlog_mask = nullptr;  // [64 lanes] every lane's wlog_m, for the other groups' step T - 1
  uint32_t wlog_m = 0u, key0 = 0u;
  if constexpr (PIPE) {
    __shared__ QT wlog_lds[KG * 32 * GW + kWave];
    __shared__ uint32_t wlog_mask_lds[kWave];
    wlog = wlog_lds;
    wlog_mask = wlog_mask_lds;
  }
  const uint32_t* codes_a;
  char* rec_ptr;
  uint32_t TA, env_st, env_end, o3, eo3;
  EnvV eS[3];
  uint2 pS[3];
  uint32_t cS[3];
  uint32_t cw, strip, a0, aN;
  int iT;
  Row4<QT> row0, rowN;
  uint32_t iS[3] = {0u, 0u, 0u};
  Row4<QT> cand[3];
  Patch<QT> pat{0xFFFFFFFFu, 0, (QT)0};
  float ep_sum = 0.0f;
  float t0_in = tin, t0_m = tm;
  // masked-off lanes may explore too: they read agent 0's rows and store only to the dummy slots
  auto code_of = [&](uint32_t w) { return TRAIN ? w : 0xFFFFFFFFu; };
  // row arithmetic in 24-bit multiplies (full-rate v_mul_u32_u24; every operand < 2^24)
  auto strip_of = [&](uint32_t base, int it_) { return __umul24(base + __umul24((uint32_t)it_, (uint32_t)nbv), (uint32_t)np); };
  auto row0_addr = [&](uint32_t st, uint32_t nr, uint32_t c) -> uint32_t {
    const bool need = ((c & 0xFF) == 255) || (TRAIN && R1 == 1);  // greedy, or the TD target itself
    return need ? st + (uint32_t)ip_zero : nr;
  };
#if P2PMG_TRACE  // timing-only probe: per-step s_memtime splits of one wave, printed at the end
  uint64_t trW = 0, trC = 0, trR = 0, trLast = 0, trA0 = 0, trWC = 0, trA1 = 0, trMid = 0, trCal = 0;
#define P2PMG_STAMP(v) asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(v)::"memory")
#endif
  // An episode's prologue (ep: its index in the chain): ring fill, first rows, the T0 draw.  PIPE: runs
  // under the divergent branch of a phase boundary, for one half of the wave.
  auto begin_episode = [&](int ep) __attribute__((always_inline)) {
    if constexpr (PIPE) {
      if (ep >= 1 && st_on) {  // the reset at the end of episode ep - 1: drawn in this half's previous prologue
        tin = t0_in;
        tm = t0_m;
      }
    }
    codes_a = p.codes + (size_t)(PIPE && ep < 0 ? 0 : ep) * p.codes_stride + a;
    if constexpr (PIPE) {
      rec_ptr = rec_on && st_on ? reinterpret_cast<char*>(recs) + (size_t)a * rec_bytes : rec_dummy;
      rec_adv = st_on ? rec_step : 0;
    } else {
      rec_ptr = rec_on ? reinterpret_cast<char*>(recs) + (size_t)a * rec_bytes : rec_dummy;
    }
    // The per-step inputs (env row, pre-pass word, code word, round-1 bins) are fresh HBM lines every
    // step, loaded three steps ahead into a 3-slot ring: slot t % 3 holds step t's, and step t
    // refills its own slot with step t + 3's once those are dead.  The step loop is unrolled by three,
    // so every slot is a fixed register set (no copies at the back edge, which would wait for the
    // loads), and the refills are issued after the step's row gathers: loads complete in issue order,
    // so a stream load issued ahead of the gathers would hold up the wait for them.
    // Running (uniform, 32-bit) offsets of step t + 3, wrapping at T: T * A < 2^32 on this path.
    TA = (uint32_t)T * (uint32_t)A, env_st = (uint32_t)env_step, env_end = env_st * (uint32_t)T;
    o3 = (uint32_t)(3 % T) * (uint32_t)A, eo3 = (uint32_t)(3 % T) * env_st;

    // ring slots as vector values, so each stays one register tuple (a 16-B load's destination)
    eS[0] = load_envv(envb), eS[1] = load_envv(envb + (size_t)t1 * env_step), eS[2] = load_envv(envb + (size_t)t2 * env_step);
    pS[0] = preb[0], pS[1] = preb[(size_t)t1 * A], pS[2] = preb[(size_t)t2 * A];
    cS[0] = codes_a[0], cS[1] = codes_a[(size_t)t1 * A], cS[2] = codes_a[(size_t)t2 * A];
    cw = code_of(cS[0]);
    iT = temp_bin(tin);
    strip = strip_of(pS[0].y & 0xFFFFu, iT);
    const uint32_t nrow = strip_of(pS[0].y >> 16, iT) + (uint32_t)ip_zero;
    a0 = row0_addr(strip, nrow, cw);
    aN = TRAIN ? nrow : a0;
    row0 = gat(a0);
    rowN = gat(aN);
    if constexpr (CAND) {
      iS[0] = ipc_a[0];
      iS[1] = ipc_a[(size_t)t1 * A];
      iS[2] = ipc_a[(size_t)t2 * A];
#pragma unroll
      for (int b = 0; b < 3; ++b) cand[b] = gat((strip + ((iS[0] >> (8 * b)) & 0xFFu)));
    }
    pat = Patch<QT>{0xFFFFFFFFu, 0, (QT)0};
    ep_sum = 0.0f;
    if constexpr (!PIPE) {
      // the end-of-episode T0 reset depends only on (seed, episode + 1, agent): drawn here, while the
      // first rows are in flight, and applied at the end (the f64 transcendentals off the episode tail)
      t0_in = tin, t0_m = tm;
      if (p.reset_t0 && active)
        t0_draw(p.seed_lo, p.seed_hi, p.episode + ep + 1, p.agent_offset + (uint32_t)a, k.setpoint, p.reset_sigma, t0_in,
                t0_m);
    } else {
      // this episode's undo log starts empty (read by the other half L steps later, at its step T - 1)
      key0 = pS[0].y & 0xFFFFu;
      wlog_m = 0u;
      wlog_mask[lane] = 0u;
      // the T0 this group's NEXT episode (ep + KG) starts from, or the one the chain leaves behind: drawn
      // while the first rows are in flight
#if P2PMG_ABLATE != 13  // 13 (timing-only): no draw at the phase boundary (what moving it off the wave could save)
      if (active)
        t0_draw(p.seed_lo, p.seed_hi, p.episode + (ep + KG < n_chain ? ep + KG : n_chain), p.agent_offset + (uint32_t)a,
                k.setpoint, p.reset_sigma, t0_in, t0_m);
#endif
    }
  };
  // the end of an episode (non-PIPE)
  auto end_episode = [&](int ep) __attribute__((always_inline)) {
    if (active) {
      if (p.reset_t0) {  // agent.reset() at the end of train_episode (community.py:181), fused
        tin = t0_in;
        tm = t0_m;
      }
      if (i == 0) {
        if (p.chain_rewards) p.chain_rewards[(size_t)ep * p.S + s] = ep_sum;
        if (ep == n_chain - 1) p.ep_reward[s] = ep_sum;
      }
    }
  };

  // one step; the loop below runs it three times per iteration (a manual unroll: the DPP exchanges
  // are convergent, so the compiler will not unroll a loop with a runtime trip count): the input
  // ring's slots and the prefetched rows' alternating registers stay put
  auto step = [&](auto par) __attribute__((always_inline)) {
    constexpr int P = decltype(par)::value, P1 = (P + 1) % 3;  // slots of step t and of step t + 1
    const EnvV ev = eS[P];
    const EnvRow e0{0.0f, ev.x, ev.y, ev.z, ev.w};
    const uint2 p0 = pS[P], p1 = pS[P1];
    const uint32_t c1 = cS[P1], ipc0 = iS[P], ipc1 = iS[P1];
    const float balw = __uint_as_float(p0.x);
    float row[N];
    float col[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { row[j] = 0.0f; col[j] = 0.0f; }
    // the next step's T_in, temperature bin and table strips for each of the 3 actions
    // (heating.py:37-56, rl.py:93): they need only this step's state, so they run while the rows
    // are in flight, and the final action then merely selects one set (issue_next)
    float tinA[3];
    uint32_t iTA[3], stA[3], nrA[3];
    {
      const float ain = k.inv_ri * (tm - tin) + k.inv_rvent * (e0.t_out - tin);
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const float d_in = k.inv_ci * (ain + hin[x]);
        tinA[x] = tin + (d_in * k.spm) * k.slot;
        iTA[x] = (uint32_t)temp_bin(tinA[x]);
        stA[x] = strip_of(p1.y & 0xFFFFu, (int)iTA[x]);
        nrA[x] = strip_of(p1.y >> 16, (int)iTA[x]) + (uint32_t)ip_zero;
      }
    }
    // Between the rows' arrival and the next step's gathers the wave issues on the critical path
    // (the gathers' latency is the rest of the step): only what those addresses need goes there;
    // the TD target row's patch, T_m, the records and the market wait until the gathers are out.
    const Patch<QT> pprev = pat;    // the previous step's TD store
#if P2PMG_TRACE
    uint64_t tr0, tr1;
    P2PMG_STAMP(tr0);
    if (trLast) trR += tr0 - trLast;
    asm volatile("" ::"v"(row0.v[0]), "v"(row0.v[1]), "v"(row0.v[2]));
    P2PMG_STAMP(tr1);
    trW += tr1 - tr0;
    {  // calibration: the cost of one stamp (two back to back)
      uint64_t tcal;
      P2PMG_STAMP(tcal);
      trCal += tcal - tr1;
      tr1 = tcal;
    }
    trMid = tr1;  // no candidate rows (N != 2 or a battery): "round1" runs from the rows' arrival
#endif
    double soc_r = soc;  // tentative SoC of the current round
    BatPre bpre{};
    if constexpr (BAT == 2) bpre = bat_pre(soc, bcap, bk);  // shared by the step's rounds
    auto bat_rule = [&](float o, double& sr) -> float {
      if constexpr (BAT == 2) return (float)battery_rule_pre((double)o, sr, rcap, bk, bpre);
      return (float)battery_rule_r<true>((double)o, sr, bcap, rcap, bk);
    };
    // (round 0's rule for all 3 actions ahead of the rows' wait measured slower: configs[3] 57.1 ->
    // 59.5 ms, profiles/r05_ab/bat_spec0_ab.txt)
    row0 = patched(row0, a0, pat);  // ... may have hit a prefetched row

    // round 0 (P = 0: every filtered power is -0, tot = 0, even split)
    int code = (int)(cw & 0xFF);
    int act = code == 255 ? argmax3(row0) : code;
    float hp = hp_of(lv, act);
    int ip = ip_zero;
    Row4<QT> rowR = row0;
    uint32_t acts = (uint32_t)act, ips = (uint32_t)ip_zero;
    // CommunityMicrogrid._step -> HPHeating.step (community.py:184-188, heating.py:138-143) needs
    // only the final round's heat-pump power: it and the next step's row gathers are issued as soon
    // as that is known, ahead of the final round's divide-power and this step's market work
    float tin1 = tin, tm1 = tm;
    int iT1 = 0;
    uint32_t strip1 = 0, cw1 = 0, a0n = 0, aNn = 0;
    Row4<QT> row0n, rowNn, candn[3];
    Sel3M mnext{};
    auto issue_next = [&](int act_final) {
      const Sel3M m = sel3_masks(act_final);
      mnext = m;
      strip1 = __float_as_uint(sel3(m, __uint_as_float(stA[0]), __uint_as_float(stA[1]), __uint_as_float(stA[2])));
      const uint32_t nrow1 =
          __float_as_uint(sel3(m, __uint_as_float(nrA[0]), __uint_as_float(nrA[1]), __uint_as_float(nrA[2])));
      cw1 = code_of(c1);
      a0n = row0_addr(strip1, nrow1, cw1);
      aNn = TRAIN ? nrow1 : a0n;
#if P2PMG_ABLATE == 8 || P2PMG_ABLATE == 10
      row0n = fake_row(q + a0n * kQPad);
      rowNn = fake_row(q + aNn * kQPad);
#else
      // the rows round 0 and round 1 wait for first, the TD's next-state row last.  Round 0's row
      // only for the lanes that read it (a greedy round 0, or the TD target at R = 0): an exploring
      // lane's gather would be address work in the CU's memory pipeline for nothing (an exec-masked
      // load; configs[1] 79.8 -> 79.0 us, configs[3] 66.2 -> 65.3 ms at the bench's epsilon)
      {
        Row4<QT> r0{};
        if (((cw1 & 0xFF) == 255) || (TRAIN && R1 == 1)) r0 = gat(a0n);
        row0n = r0;
      }
#endif
      if constexpr (CAND) {
#pragma unroll
        for (int b = 0; b < 3; ++b) candn[b] = gat((strip1 + ((ipc1 >> (8 * b)) & 0xFFu)));
      }
#if !(P2PMG_ABLATE == 8 || P2PMG_ABLATE == 10)
      rowNn = gat(aNn);
#endif
    };
    // step t + 3's code word and round-1 bins into this step's slots (dead since step t - 1 / round 1)
    auto refill_words = [&]() {
      cS[P] = codes_a[o3];
      if constexpr (CAND) iS[P] = ipc_a[o3];
    };
    // the rest of HPHeating.step for the chosen level, once the gathers are out
    auto settle_next = [&]() {
      const Sel3M& m = mnext;
      iT1 = (int)__float_as_uint(sel3(m, __uint_as_float(iTA[0]), __uint_as_float(iTA[1]), __uint_as_float(iTA[2])));
      tin1 = sel3(m, tinA[0], tinA[1], tinA[2]);
      const float d_m = k.inv_cm * (((k.inv_ri * (tin - tm) + k.inv_re * (e0.t_out - tm)) + k.solar) +
                                    sel3(m, hm[0], hm[1], hm[2]));  // heating.py:45,48
      tm1 = tm + (d_m * k.spm) * k.slot;
    };
    if constexpr (R1 == 1) {
      issue_next(act);
      refill_words();
      settle_next();
    }
    float out0 = balw + hp;
    if constexpr (BAT != 0) {
      if (bcap > 0.0) out0 = bat_rule(out0, soc_r);
    }
    const float ev0 = div_n_r<N>(out0 * 1.0f, rn);
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] = ev0;
#pragma unroll
    for (int r = 1; r < R1; ++r) {
      if (r == 1) {
        gather_even<N, 1, G>(ev0, col, i);
      } else {
        exchange<N>(row, col, i, sl, nullptr);
      }
      code = (int)((cw >> (8 * r)) & 0xFF);
      if (CAND && r == 1) {
        // the partner's round-0 action picks the prefetched row (its bin is byte b of ipc0)
        // (a DPP quad_perm inside the scenario's G = 2 lanes: a lane group of 32 or 16 lanes never splits a pair)
        const int b = __float_as_int(shfl_xor_c<1>(__int_as_float(act)));
#if P2PMG_TRACE
        {
          uint64_t ta, tb;
          asm volatile("" ::"v"(b));
          P2PMG_STAMP(ta);
          asm volatile("" ::"v"(cand[0].v[0]), "v"(cand[1].v[0]), "v"(cand[2].v[0]), "v"(cand[0].v[2]), "v"(cand[1].v[2]),
                       "v"(cand[2].v[2]));
          P2PMG_STAMP(tb);
          trA0 += ta - tr1;
          trWC += tb - ta;
          trMid = tb;
        }
#endif
        ip = (int)((ipc0 >> (8 * b)) & 0xFFu);
        rowR = patched(sel_row(b, cand[0], cand[1], cand[2]), strip + (uint32_t)ip, pat);
      } else {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) acc = acc + (-((j == i) ? 0.0f : col[j]));
        ip = p2p_bin(fdiv_b(div_n_r<N>(acc, rn), rmi));
        const bool need = code == 255 || (TRAIN && r == R1 - 1);
#if P2PMG_ABLATE == 7
        rowR = fake_row(q + (need ? strip + (uint32_t)ip : a0) * kQPad);
#else
        rowR = gat((need ? strip + (uint32_t)ip : a0));
#endif
      }
#if P2PMG_BAT_SPEC
      // the final round's battery rule for each of the 3 actions while its row is in flight (it
      // needs only balw, the level and this step's SoC): the action then only selects
      float outA[3];
      double socA[3];
      if constexpr (BAT != 0) {
        if (r == R1 - 1) {
#pragma unroll
          for (int x = 0; x < 3; ++x) {
            socA[x] = soc;
            outA[x] = balw + hp_of(lv, x);
            if (bcap > 0.0) outA[x] = bat_rule(outA[x], socA[x]);
          }
        }
      }
#endif
      act = code == 255 ? argmax3(rowR) : code;
      acts |= (uint32_t)act << (8 * r);
      ips |= (uint32_t)ip << (8 * r);
      hp = hp_of(lv, act);
      if (r == R1 - 1) {
#if P2PMG_TRACE
        {
          uint64_t tc;
          asm volatile("" ::"v"(act));
          P2PMG_STAMP(tc);
          trA1 += tc - trMid;
          trMid = tc;
        }
#endif
        issue_next(act);
#if P2PMG_TRACE
        P2PMG_STAMP(trLast);
        trC += trLast - trMid;
#endif
        refill_words();
        settle_next();
      }
      float out = balw + hp;
      if constexpr (BAT != 0) {
#if P2PMG_BAT_SPEC
        if (r == R1 - 1) {
          const Sel3M m = sel3_masks(act);
          out = sel3(m, outA[0], outA[1], outA[2]);
          soc_r = sel3(m, socA[0], socA[1], socA[2]);
        } else
#endif
        {
          soc_r = soc;
          if (bcap > 0.0) out = bat_rule(out, soc_r);
        }
      }
#if P2PMG_ABLATE == 11  // timing-only: no final-round divide-power and no market (cost from out alone)
      if (r == R1 - 1) {
        row[0] = out;
        continue;
      }
#endif
      // _divide_power's filter keeps pw where sign(out) != sign(pw) (agent.py:187-188): for out > 0
      // that is pw <= 0, for out < 0 pw >= 0, for out = 0 any pw.  A kept pw = +-0 and a dropped
      // one (0) are interchangeable: every later use is |f| or a sum that already holds +0.
      // As one clamp: f = med3(pw, out < 0 ? 0 : -inf, out > 0 ? 0 : +inf).
      const float flo = out < 0.0f ? 0.0f : -__builtin_inff(), fhi = out > 0.0f ? 0.0f : __builtin_inff();
      float f[N];
      float tot = 0.0f;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float pw = -((j == i) ? 0.0f : col[j]);
        f[j] = __builtin_amdgcn_fmed3f(pw, flo, fhi);
        tot = tot + f[j];
      }
      tot = fabsf(tot);
      const float ev = div_n_r<N>(out * 1.0f, rn);
      // out * |f_j| / tot for every j: the diagonal's f_ii = +-0 gives out * 0 / tot = out * 0, the
      // reference's value for it (agent.py:193-194), for any tot > 0.  One range guard per round.
      const Recip rt = recip(tot == 0.0f ? 1.0f : tot);  // the tot = 0 lanes take ev
      const float nout = nabs_out(out);
      float num[N];
      bool bad = !rt.ok;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        num[j] = nout * f[j];
        row[j] = fdiv_core(num[j], rt);
        bad = bad || !fdiv_ok(num[j]);
      }
      if (bad) {
#pragma unroll
        for (int j = 0; j < N; ++j) row[j] = fdiv_ieee(num[j], rt.b);
      }
#pragma unroll
      for (int j = 0; j < N; ++j) row[j] = (tot == 0.0f) ? ev : row[j];
    }
    soc = soc_r;  // BatteryStorage state after the final round's decision
    pat.row = 0xFFFFFFFFu;  // the next step's rows were issued after the previous TD store

    // CommunityMicrogrid._assign_powers community.py:45-54 on the final P (diagonal kept)
    float g = 0.0f, pp = 0.0f;
#if P2PMG_ABLATE == 11
    g = row[0];
#else
    exchange<N>(row, col, i, sl, nullptr);  // inside the scenario's G lanes, whatever the lane group's width
#pragma unroll
    for (int j = 0; j < N; ++j) {
      // ex = sign(pij) * min(|pij|, |pji|) where the signs differ (community.py:48-50)
      const float pij = row[j], pji = col[j];
      const float ex = pair_exchange(pij, pji);
      g = g + (pij - ex);
      pp = pp + ex;
    }
#endif
    // CommunityMicrogrid._compute_costs community.py:56-65
    float cost = (g >= 0.0f) ? g * e0.buy : g * e0.inj;
    cost = cost + pp * e0.p2p;
    cost = fdiv_b(cost * k.slot, rmph);
    cost = cost * k.kilo;
    // RLAgent.get_reward agent.py:225-232 (pre-update T_in)
    float pen = fmaxf(fmaxf(0.0f, k.lower - tin), fmaxf(0.0f, tin - k.upper));
    pen = pen > 0.0f ? pen + 1.0f : 0.0f;
    const float rw = -(cost + k.penw * pen);

    if constexpr (TRAIN) {
      // QAgent.train agent.py:293-298 -> QActor.train rl.py:119-129
      const uint32_t srow = strip + (uint32_t)ip;
      const QT qsa = sel3(act, rowR.v[0], rowR.v[1], rowR.v[2]);
      QT qmax = max3(patched(rowN, aN, pprev));
      if constexpr (PIPE && P == 2) {
        // step T - 1 of an episode with a follower: its next-state row (key of step 0) has been
        // written by the follower since its own step 0, every such store issued before the row's load;
        // where the follower logged the row, the log holds what the serial chain reads here
        if (wrap_it) {
          if constexpr (KG == 2) {
            const QT sv = wlog[((grp ^ 1) * 32 + iT) * 32 + hl];
            const uint32_t fm = wlog_mask[lane ^ 32];
#if P2PMG_ABLATE != 12  // 12 (test-only): the loaded row, which the follower has overwritten; the dense-collision test must then fail
            qmax = wrap_l && ((fm >> iT) & 1u) != 0u ? sv : qmax;
#endif
          } else {
            // three followers (episodes e + 1, e + 2, e + 3 in groups grp + 1, + 2, + 3 mod 4) may have stored
            // into the row: the EARLIEST one that logged the bin read it as the serial chain leaves it for
            // this step (a later follower's first read has seen the earlier follower's stores).  A group
            // without a successor episode (the chain's end, the drain) reset its mask in its prologue and
            // never logs, so it reads as "not logged".  Selected from the last follower down to the first.
            QT pick = qmax;
#pragma unroll
            for (int j = KG - 1; j >= 1; --j) {
              const int gj = (grp + j) % KG;
              const QT sv = wlog[(gj * 32 + iT) * GW + hl];
              const uint32_t fm = wlog_mask[gj * GW + hl];
              pick = ((fm >> iT) & 1u) != 0u ? sv : pick;
            }
#if P2PMG_ABLATE != 12
            qmax = wrap_l ? pick : qmax;
#endif
          }
        }
      }
      if constexpr (PIPE) {
        // the first store of this episode into a row the leader's step T - 1 may read: log max3 of the
        // row as this step read it (rowR holds the lane's own previous store).  The hazard rule keeps
        // such steps out of an episode's second half.
        const bool first = st_on && (p0.y & 0xFFFFu) == key0 && ip == ip_zero && ((wlog_m >> iT) & 1u) == 0u;
        wlog[first ? (grp * 32 + iT) * GW + hl : KG * 32 * GW + lane] = max3(rowR);
        wlog_m |= first ? 1u << iT : 0u;
        wlog_mask[lane] = wlog_m;
      }
      const QT qnew = td_update(qsa, rw, qmax, k.alpha, k.gamma);
      *((PIPE ? st_on : active) ? q + srow * kQPad + act : q_dummy) = qnew;
#if P2PMG_ABLATE == 9 || P2PMG_ABLATE == 10
      pat = Patch<QT>{0xFFFFFFFFu, 0, (QT)0};  // timing-only: the next step does not wait for this TD
#else
      pat = Patch<QT>{srow, act, qnew};  // rows issued before this store see the old value
#endif
    }
    if constexpr (narrow) {
      *reinterpret_cast<float2*>(__builtin_assume_aligned(rec_ptr, 8)) = make_float2(rw, cost);
    } else {
      const uint32_t bins = (p0.y & 0xFFFFu) | ((uint32_t)iT << 16);  // it * nT*nb + ib | iT << 16
      float4* rp = reinterpret_cast<float4*>(__builtin_assume_aligned(rec_ptr, 16));
      rp[0] = make_float4(rw, cost, g, pp);
      rp[1] = make_float4(tin, __uint_as_float(acts), __uint_as_float(bins), __uint_as_float(ips));
    }
    rec_ptr += PIPE ? rec_adv : rec_step;
    // step t's env row and pre-pass word are dead: step t + 3's into their slots (the barrier keeps
    // the scheduler from hoisting the loads above the old values' last use, which would need a
    // second register set and a copy at the loop's back edge)
    asm volatile("" ::: "memory");
    eS[P] = load_envv(envb + eo3);
    pS[P] = preb[o3];
    // avg_reward = sum_t mean_i r (community.py:179), canonical sequential order
    const float m = group_sum<N>(rw, lane, i, sl, nullptr);
    ep_sum = ep_sum + div_n_r<N>(m, rn);

    tin = tin1;
    tm = tm1;
    iT = iT1;
    o3 += (uint32_t)A;
    o3 = o3 == TA ? 0u : o3;
    eo3 += env_st;
    eo3 = eo3 == env_end ? 0u : eo3;
    strip = strip1;
    cw = cw1;
    a0 = a0n;
    aN = aNn;
    row0 = row0n;
    rowN = rowNn;
    if constexpr (CAND) {
#pragma unroll
      for (int b = 0; b < 3; ++b) cand[b] = candn[b];
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  using S2 = std::integral_constant<int, 2>;
  if constexpr (!PIPE) {
    for (int ep = 0; ep < n_chain; ++ep) {
      begin_episode(ep);
      __builtin_amdgcn_s_waitcnt(0);  // enter the loop with nothing in flight (static waits inside)
      int t = 0;
      for (; t + 3 <= T; t += 3) {
        step(S0{});
        step(S1{});
        step(S2{});
      }
      if (t < T) step(S0{});
      if (t + 1 < T) step(S1{});
#if P2PMG_TRACE
      if (threadIdx.x == 0 && (blockIdx.x == 0 || (int)blockIdx.x == n_cons / 2 || (int)blockIdx.x == n_cons - 1))
        printf("TRACE blk %d/%d T %d: per step wait %.1f round0 %.1f waitcand %.1f round1 %.1f issue %.1f rest %.1f "
               "(one stamp %.1f)\n",
               (int)blockIdx.x, n_cons, T, (double)trW / T, (double)trA0 / T, (double)trWC / T, (double)trA1 / T,
               (double)trC / T, (double)trR / (T - 1), (double)trCal / T);
      trW = trC = trR = trLast = trA0 = trWC = trA1 = trMid = trCal = 0;
#endif
      end_episode(ep);
    }  // chain
    if (active) {
      p.t_in[a] = tin;
      p.t_m[a] = tm;
      if constexpr (BAT != 0) p.soc[a] = soc;
    }
  } else {
    // Phase ph (L = T / KG lockstep steps; the launcher sends T % (3 KG) == 0, so the ring's rotation holds
    // across phases): episode ph runs its first L steps in group ph % KG of the wave, episodes ph - 1 ..
    // ph - KG + 1 their later phases in the other groups.  A group without an episode (fill: the groups
    // above 0 until their first phase; drain: the groups whose next episode would be past the chain) runs
    // masked to the dummy slots, as inactive lanes do.
    const int L = T / KG;
    int ep_l = grp == 0 ? 0 : grp - KG;  // the episode this lane's group runs (< 0: none yet; its prologue draws episode grp's T0)
    st_on = active && grp == 0;
    begin_episode(ep_l);  // the other groups: only their ring, rows and their first episode's T0 draw
    __builtin_amdgcn_s_waitcnt(0);
    for (int ph = 0;; ++ph) {
      if (ph > 0) {
        if (grp == (int)((unsigned)ph % KG)) {  // this group is at an episode boundary
          if (st_on && i == 0) {
            if (p.chain_rewards) p.chain_rewards[(size_t)ep_l * p.S + s] = ep_sum;
            if (ep_l == n_chain - 1) p.ep_reward[s] = ep_sum;
          }
          if (ph <= n_chain + KG - 2) {
            ep_l = ph;
            st_on = active && ph < n_chain;
            begin_episode(ph < n_chain ? ph : n_chain - 1);
          }
        }
        // every group enters the loop with nothing in flight (the other groups' rows sit through this)
        __builtin_amdgcn_s_waitcnt(0);
        if (ph > n_chain + KG - 2) break;
      }
      wrap_l = st_on && grp == (int)((unsigned)(ph + 1) % KG) && ep_l + 1 < n_chain;  // the group in its episode's last phase
      for (int t = 0; t < L; t += 3) {
        wrap_it = t + 3 >= L;
        step(S0{});
        step(S1{});
        step(S2{});
      }
    }
    // the T0 the chain leaves behind: drawn in the last episode's prologue
    if (active && grp == (int)((unsigned)(n_chain - 1) % KG)) {
      p.t_in[a] = t0_in;
      p.t_m[a] = t0_m;
    }
  }
}

// the community sizes the several-episodes-per-wave forms (KG = 2, 4) are instantiated for (the plan asks the same)
template <int N>
constexpr bool kFastPipe = N == 2;

// hipExtLaunchKernel stamps the start / stop events from the dispatch itself: no marker packets
// between back-to-back episodes
template <int N, typename QT, int R1, int BAT, bool NARROW>
void launch_fast_nw(const EpisodeParams& p, const uint2* pre, FastRec* recs, int blocks, int spw, int prod,
                    const PrepOut& nxt, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  if constexpr (kFastPipe<N> && BAT == 0) {
    if (p.mode == 0 && p.interleave == 4)
      return hipExtLaunchKernelGGL((episode_fast_kernel<N, QT, R1, true, BAT, NARROW, 4>), dim3(blocks + prod),
                                   dim3(kWave), 0, st, ev0, ev1, 0, p, pre, recs, spw, blocks, nxt);
    if (p.mode == 0 && p.interleave)
      return hipExtLaunchKernelGGL((episode_fast_kernel<N, QT, R1, true, BAT, NARROW, 2>), dim3(blocks + prod),
                                   dim3(kWave), 0, st, ev0, ev1, 0, p, pre, recs, spw, blocks, nxt);
  }
  if (p.mode == 0)
    hipExtLaunchKernelGGL((episode_fast_kernel<N, QT, R1, true, BAT, NARROW>), dim3(blocks + prod), dim3(kWave), 0, st,
                          ev0, ev1, 0, p, pre, recs, spw, blocks, nxt);
  else
    hipExtLaunchKernelGGL((episode_fast_kernel<N, QT, R1, false, BAT, NARROW>), dim3(blocks + prod), dim3(kWave), 0, st,
                          ev0, ev1, 0, p, pre, recs, spw, blocks, nxt);
}
template <int N, typename QT, int R1, int BAT>
void launch_fast_b(const EpisodeParams& p, const uint2* pre, FastRec* recs, int blocks, int spw, int prod,
                   const PrepOut& nxt, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  if (p.rec_narrow) return launch_fast_nw<N, QT, R1, BAT, true>(p, pre, recs, blocks, spw, prod, nxt, ev0, ev1, st);
  launch_fast_nw<N, QT, R1, BAT, false>(p, pre, recs, blocks, spw, prod, nxt, ev0, ev1, st);
}
template <int N, typename QT, int R1>
void launch_fast_r(const EpisodeParams& p, const uint2* pre, FastRec* recs, int blocks, int spw, int prod,
                   const PrepOut& nxt, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  if constexpr (R1 <= kFastBatMaxR1) {
    if (p.battery && p.bat_safe) return launch_fast_b<N, QT, R1, 2>(p, pre, recs, blocks, spw, prod, nxt, ev0, ev1, st);
    if (p.battery) return launch_fast_b<N, QT, R1, 1>(p, pre, recs, blocks, spw, prod, nxt, ev0, ev1, st);
  }
  launch_fast_b<N, QT, R1, 0>(p, pre, recs, blocks, spw, prod, nxt, ev0, ev1, st);
}

template <int N, typename QT>
hipError_t launch_fast_n(const EpisodeParams& p, const uint2* pre, void* recs, int spw, const PrepOut* nxt,
                         hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  constexpr int G = pow2ceil(N);
  // several episodes per wave (p.interleave = 2 or 4 lane groups) need what the plan promises; anything
  // else is a caller's error
  const int kg = p.interleave;
  if (kg && !((kg == 2 || kg == 4) && kFastPipe<N> && p.mode == 0 && !p.battery && p.chain >= kg && p.reset_t0 &&
              p.T % (3 * kg) == 0 && p.nT <= 32 && spw > 0 && spw <= kWave / kg / G))
    return hipErrorInvalidValue;
  if (spw <= 0 || spw > kWave / G) spw = kWave / G;
  const int blocks = (p.S + spw - 1) / spw;
  const size_t n = (size_t)p.T * p.A;
  const int prod = nxt ? (int)std::min<size_t>(2048, (n + kWave - 1) / kWave) : 0;
  const PrepOut none{nullptr, nullptr, nullptr, 0, 0.0};
  FastRec* r = reinterpret_cast<FastRec*>(recs);
  switch (p.R + 1) {
    case 1: launch_fast_r<N, QT, 1>(p, pre, r, blocks, spw, prod, nxt ? *nxt : none, ev0, ev1, st); break;
    case 2: launch_fast_r<N, QT, 2>(p, pre, r, blocks, spw, prod, nxt ? *nxt : none, ev0, ev1, st); break;
    case 3: launch_fast_r<N, QT, 3>(p, pre, r, blocks, spw, prod, nxt ? *nxt : none, ev0, ev1, st); break;
    case 4: launch_fast_r<N, QT, 4>(p, pre, r, blocks, spw, prod, nxt ? *nxt : none, ev0, ev1, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// agents per scenario N0 and N0 + 1, f64 or f32 table
template <int N0>
hipError_t launch_fast_pair(const EpisodeParams& p, const uint2* pre, void* recs, int q_dtype, int spw,
                            const PrepOut* nxt, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  if (p.N == N0)
    return q_dtype == 0 ? launch_fast_n<N0, double>(p, pre, recs, spw, nxt, ev0, ev1, st)
                        : launch_fast_n<N0, float>(p, pre, recs, spw, nxt, ev0, ev1, st);
  if (p.N == N0 + 1)
    return q_dtype == 0 ? launch_fast_n<N0 + 1, double>(p, pre, recs, spw, nxt, ev0, ev1, st)
                        : launch_fast_n<N0 + 1, float>(p, pre, recs, spw, nxt, ev0, ev1, st);
  return hipErrorInvalidValue;
}

}  // namespace

// _build.py compiles this file once per slice (-DP2PMG_FAST_SLICE=k, in parallel): slice k defines the
// launcher for N = 2k + 1 and 2k + 2, so each episode_fast_kernel instantiation is compiled in one slice
// only; slice 0 (also what an undefined macro selects) holds the dispatcher as well.
#define P2PMG_FAST_LAUNCHER(name, N0)                                                                             \
  hipError_t name(const EpisodeParams& p, const uint2* pre, void* recs, int q_dtype, int spw, const PrepOut* next, \
                  hipEvent_t ev0, hipEvent_t ev1, hipStream_t stream) {                                           \
    return launch_fast_pair<N0>(p, pre, recs, q_dtype, spw, next, ev0, ev1, stream);                              \
  }
#if P2PMG_FAST_SLICE == 0
P2PMG_FAST_LAUNCHER(launch_fast_n12, 1)
#endif
#if P2PMG_FAST_SLICE == 1
P2PMG_FAST_LAUNCHER(launch_fast_n34, 3)
#endif
#if P2PMG_FAST_SLICE == 2
P2PMG_FAST_LAUNCHER(launch_fast_n56, 5)
#endif
#if P2PMG_FAST_SLICE == 3
P2PMG_FAST_LAUNCHER(launch_fast_n78, 7)
#endif
#if P2PMG_FAST_SLICE == 0
hipError_t launch_episode_fast(const EpisodeParams& p, const uint2* pre, void* recs, int q_dtype, int spw,
                               const PrepOut* next, hipEvent_t ev0, hipEvent_t ev1, hipStream_t stream) {
  auto f = p.N <= 2 ? launch_fast_n12 : p.N <= 4 ? launch_fast_n34 : p.N <= 6 ? launch_fast_n56 : launch_fast_n78;
  if (p.N < 1 || p.N > 8) return hipErrorInvalidValue;
  return f(p, pre, recs, q_dtype, spw, next, ev0, ev1, stream);
}
#endif

}  // namespace p2pmg
