// p2pmg_tabular.h — device helpers shared by the tabular kernel families (p2pmg_general.hip,
// p2pmg_fast.hip, p2pmg_sq16.hip, p2pmg_small.hip).
//
// Build flags that are part of the numerics contract:
//   -ffp-contract=off   every f32/f64 op rounds separately, as TF eager and NumPy do
//   (default)           correctly-rounded f32 division, f32 denormals kept
//
// Layout (HBM):
//   prof  [T][A] float2 {load_w, pv_w}   time-major: one coalesced 8-B load per lane per step
//   env   [S_env][T][8] f32              time, t_out, buy, inj, p2p (shared when S_env == 1)
//   q     [A][n_states][4] f64|f32       per-agent table, rows padded 3 -> 4 actions so a
//                                        greedy gather is ONE aligned 32-B (f64) / 16-B (f32) sector
//   t_in, t_m, max_in [A] f32            register-resident across the whole episode
// Mapping: one lane per agent; a scenario's N agents occupy a lane group of G = pow2ceil(N)
// lanes inside one wave (64 / G scenarios per wave, one wave per workgroup); the Jacobi
// proposal matrix P never leaves the chip — each lane keeps its row in registers and reads
// its column through a per-wave LDS tile (community.py:75-86).
#pragma once
#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>

#include "p2pmg_internal.h"

namespace p2pmg {
namespace {

#include "p2pmg_device.h"

template <typename QT>
struct Row4 {
  QT v[4];
};

// x[a] for a in {0,1,2} as two v_cndmask: written in asm because hipcc turns a select chain
// on a runtime index into a scratch/LDS lookup table (a memory round trip + vmcnt(0) drain)
// 3-way select by a per-lane index a in {0, 1, 2}, as asm so that hipcc never turns it into a
// scratch-indexed array.  The two lane masks are separate (non-volatile) asm: every select on the
// same index shares them (CSE), e.g. the six 32-bit halves of a selected f64 row.
struct Sel3M {
  uint64_t m1, m2;
};
__device__ __forceinline__ Sel3M sel3_masks(int a) {
  uint64_t m1, m2;
  asm("v_cmp_eq_u32_e64 %0, 1, %1" : "=s"(m1) : "v"(a));
  asm("v_cmp_eq_u32_e64 %0, 2, %1" : "=s"(m2) : "v"(a));
  return Sel3M{m1, m2};
}
__device__ __forceinline__ float sel3(const Sel3M& m, float x0, float x1, float x2) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3\n\tv_cndmask_b32_e64 %0, %0, %4, %5"
      : "=&v"(r)
      : "v"(x0), "v"(x1), "s"(m.m1), "v"(x2), "s"(m.m2));
  return r;
}
__device__ __forceinline__ double sel3(const Sel3M& m, double x0, double x1, double x2) {
  const uint64_t b0 = (uint64_t)__double_as_longlong(x0), b1 = (uint64_t)__double_as_longlong(x1),
                 b2 = (uint64_t)__double_as_longlong(x2);
  const uint32_t lo = __float_as_uint(sel3(m, __uint_as_float((uint32_t)b0), __uint_as_float((uint32_t)b1),
                                           __uint_as_float((uint32_t)b2)));
  const uint32_t hi = __float_as_uint(sel3(m, __uint_as_float((uint32_t)(b0 >> 32)),
                                           __uint_as_float((uint32_t)(b1 >> 32)),
                                           __uint_as_float((uint32_t)(b2 >> 32))));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
template <typename T>
__device__ __forceinline__ T sel3(int a, T x0, T x1, T x2) {
  return sel3(sel3_masks(a), x0, x1, x2);
}
// Timing-only ablation builds (scripts/dev/latency_ablation.py): -DP2PMG_ABLATE=1 replaces the
// episode kernel's Q-row gathers by values derived from the address (no memory access),
// -DP2PMG_ABLATE=2 replaces f32 divisions by reciprocal multiplies; in the fast kernel =8 fakes the
// next step's rows, =9 cuts the TD -> next-step patch dependency, =10 both, =11 drops the final
// round's divide-power and the market (the cost from the net power alone).  Never shipped.
#ifndef P2PMG_ABLATE
#define P2PMG_ABLATE 0
#endif
#if P2PMG_ABLATE == 2
#define FDIV(a, b) ((a) * __frcp_rn(b))
#else
#define FDIV(a, b) ((a) / (b))
#endif
__device__ __forceinline__ Row4<double> load_row(const double* p) {
  const double2 a = *reinterpret_cast<const double2*>(p);
  const double2 b = *reinterpret_cast<const double2*>(p + 2);
  return Row4<double>{{a.x, a.y, b.x, b.y}};
}
__device__ __forceinline__ Row4<float> load_row(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  return Row4<float>{{a.x, a.y, a.z, a.w}};
}
// argmax over 3 actions, first max wins (rl.py:116)
template <typename QT>
__device__ __forceinline__ int argmax3(const Row4<QT>& r) {
  int a = 0;
  QT b = r.v[0];
  if (r.v[1] > b) { b = r.v[1]; a = 1; }
  if (r.v[2] > b) { a = 2; }
  return a;
}
// max over 3 actions (rl.py:127, np.max): two v_max.  Table entries are never NaN and never -0
// (tables start at +0 and a TD step q + alpha * d is +0 when q = +0 and d = -0), so the value is
// the sequential compare's
template <typename QT>
__device__ __forceinline__ QT max3(const Row4<QT>& r) {
  return fmax(fmax(r.v[0], r.v[1]), r.v[2]);
}
// QActor.train rl.py:125-129 under NumPy 2: f64 TD arithmetic on double(reward)
__device__ __forceinline__ double td_update(double qsa, float rw, double qmax, double alpha, double gamma) {
  return qsa + alpha * (((double)rw + gamma * qmax) - qsa);
}
__device__ __forceinline__ float td_update(float qsa, float rw, float qmax, double alpha, double gamma) {
  return qsa + (float)alpha * ((rw + (float)gamma * qmax) - qsa);
}

// ----------------------------------------------------------------- scenario-group exchange
// Lane i of a scenario group owns row i of the proposal matrix P.  exchange() gives every lane
// its column: col[j] = P[j][i].  G <= 8: cross-lane shuffles (no LDS, no barrier — a
// __syncthreads() would also drain every in-flight global load with vmcnt(0)).  G = 16: a
// per-wave LDS tile ordered by wavefront-scope fences (one wave per workgroup, DS ops of a
// wave execute in order).
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// xor-shuffle inside a lane group: DPP quad_perm for partners within a quad (a VALU op),
// ds_bpermute beyond
template <int D>
__device__ __forceinline__ float shfl_xor_c(float v) {
  if constexpr (D == 1) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));  // [1,0,3,2]
  } else if constexpr (D == 2) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false));  // [2,3,0,1]
  } else if constexpr (D == 3) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x1B, 0xF, 0xF, false));  // [3,2,1,0]
  } else {
    return __shfl_xor(v, D, 64);
  }
}

template <int N, int D>
__device__ __forceinline__ void exchange_step(const float (&row)[N], float (&col)[N], int i) {
  const int src = i ^ D;  // partner lane in the group; it sends its row[i]
  float v = 0.0f;
#pragma unroll
  for (int k = 0; k < N; ++k) v = (k == src) ? row[k] : v;  // what my partner wants: row[src]
  const float got = shfl_xor_c<D>(v);
#pragma unroll
  for (int k = 0; k < N; ++k) col[k] = (k == src) ? got : col[k];
}

template <int N, int D, int G>
__device__ __forceinline__ void exchange_all(const float (&row)[N], float (&col)[N], int i) {
  if constexpr (D < G) {
    exchange_step<N, D>(row, col, i);
    exchange_all<N, D + 1, G>(row, col, i);
  }
}

template <int N>
__device__ __forceinline__ void exchange(const float (&row)[N], float (&col)[N], int i, int sl, float* sh) {
  constexpr int G = pow2ceil(N);
  if constexpr (G <= 8) {
#pragma unroll
    for (int k = 0; k < N; ++k) col[k] = (k == i) ? row[k] : 0.0f;
    exchange_all<N, 1, G>(row, col, i);
  } else {
    if (i < N) {
#pragma unroll
      for (int j = 0; j < N; ++j) sh[(sl * N + i) * N + j] = row[j];
    }
    wave_lds_fence();
    if (i < N) {
#pragma unroll
      for (int j = 0; j < N; ++j) col[j] = sh[(sl * N + j) * N + i];
    }
    wave_lds_fence();
  }
}

// sum_{j=0..N-1} v_j over the scenario group, sequential from +0.0 (canonical order)
template <int N>
__device__ __forceinline__ float group_sum(float v, int lane, int i, int sl, float* sh) {
  constexpr int G = pow2ceil(N);
  float m = 0.0f;
  if constexpr (G == 1) {
    m = m + v;
  } else if constexpr (G == 2) {
    const float o = shfl_xor_c<1>(v);
    m = m + (i == 0 ? v : o);
    m = m + (i == 0 ? o : v);
  } else if constexpr (G <= 8) {
    const int base = lane - i;
#pragma unroll
    for (int k = 0; k < N; ++k) m = m + __shfl(v, base + k, 64);
  } else {
    if (i < N) sh[sl * N + i] = v;
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < N; ++k) m = m + sh[sl * N + k];
    wave_lds_fence();
  }
  return m;
}

struct EnvRow {
  float time, t_out, buy, inj, p2p;
};
// {t_out, buy, inj, p2p} of an env row as one 16-B load (the fast kernel's input ring)
typedef float EnvV __attribute__((ext_vector_type(4)));
__device__ __forceinline__ EnvV load_envv(const float* e) {
  EnvV v;
  __builtin_memcpy(&v, e + 1, sizeof(v));
  return v;
}
__device__ __forceinline__ EnvRow load_env(const float* e) {
  const float4 v = *reinterpret_cast<const float4*>(e);
  return EnvRow{v.x, v.y, v.z, v.w, e[4]};
}

// Loop constants pinned in VGPRs.  The kernel-argument struct has ~60 fields: left in SGPRs
// they overflow the scalar file and hipcc reloads them from VGPR lanes (v_readlane) on the
// step's dependency chain.  An opaque v_mov at entry makes each one a VGPR for the whole
// episode (one wave per SIMD leaves ample VGPRs).
__device__ __forceinline__ float vpin(float x) {
  float r;
  asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}
__device__ __forceinline__ int vpin(int x) {
  int r;
  asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}
__device__ __forceinline__ double vpin(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)vpin((int)(uint32_t)b), hi = (uint32_t)vpin((int)(uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
struct KC {
  float setpoint, margin, lower, upper;
  float inv_ci, inv_cm, inv_ri, inv_re, inv_rvent, c_in, c_m, solar, cop, spm, slot;
  float mph, kilo, penw;
  double alpha, gamma;
  int nt, nT, nb, np;
};
// Per-agent comfort and heat pump (HPHeating / HeatPump, heating.py:92-130): thermal[a] =
// {setpoint, lower, upper, cop}, one 16-B load per lane in the kernel's prologue.  The load is
// unconditional (masked-off lanes read agent 0's entry, as for hp_lv), so its wait is not tied to a
// branch; the four values are per-lane VGPRs from then on, where the broadcast arguments were pinned.
// The learner's alpha, gamma and comfort weight (QActor rl.py:58-71, agent.py:225-232) are the
// agent's own in the same way: lr = learn[a], loaded beside thermal[a].
__device__ __forceinline__ KC pin_constants(const EpisodeParams& p, const float4 th, const LearnRow lr) {
  KC k;
  k.setpoint = th.x; k.margin = vpin(p.margin); k.lower = th.y; k.upper = th.z;
  k.inv_ci = vpin(p.inv_ci); k.inv_cm = vpin(p.inv_cm); k.inv_ri = vpin(p.inv_ri); k.inv_re = vpin(p.inv_re);
  k.inv_rvent = vpin(p.inv_rvent); k.c_in = vpin(p.c_in); k.c_m = vpin(p.c_m); k.solar = vpin(p.solar);
  k.cop = th.w; k.spm = vpin(p.spm); k.slot = vpin(p.slot); k.mph = vpin(p.mph); k.kilo = vpin(p.kilo);
  k.penw = lr.penw;
  k.alpha = lr.alpha; k.gamma = lr.gamma;
  k.nt = vpin(p.nt); k.nT = vpin(p.nT); k.nb = vpin(p.nb); k.np = vpin(p.np);
  return k;
}

// The same constants left to the compiler (kernel arguments stay in SGPRs): the throughput-bound
// sq16 kernel runs several waves per SIMD, where VGPRs, not the scalar-operand latency, set the pace.
__device__ __forceinline__ KC scalar_constants(const EpisodeParams& p) {
  return KC{p.setpoint, p.margin, p.lower, p.upper, p.inv_ci, p.inv_cm, p.inv_ri, p.inv_re, p.inv_rvent,
            p.c_in,     p.c_m,    p.solar, p.cop,   p.spm,    p.slot,   p.mph,    p.kilo,   p.penw,
            p.alpha,    p.gamma,  p.nt,    p.nT,    p.nb,     p.np};
}
// ... with the agent's own thermal parameters (rule_episode_kernel)
__device__ __forceinline__ KC scalar_constants(const EpisodeParams& p, const float4 th) {
  KC k = scalar_constants(p);
  k.setpoint = th.x; k.lower = th.y; k.upper = th.z; k.cop = th.w;
  return k;
}

// Everything about step t that is known before its negotiation starts.
struct StepIdx {
  float bal;        // (load - pv) / max_in of this step    agent.py:172-176
  float baln;       // ... of the next step (= next step's bal)
  int it, iT, ib;   // s indices except p2p                 rl.py:89-95
  uint32_t strip;   // row of (it, iT, ib, 0) in the agent's table
  uint32_t nrow;    // next-state row (time_{t+1}, same T_in, bal_{t+1}, p2p = 0)  agent.py:293-296
};
// Q-table dimensions: the reference's 20 x 20 x 20 x 20 (agent.py:258-261) compile to shifts and
// adds; other sizes use the runtime values
template <bool B20>
struct Dims {
  int nt, nT, nb, np;
  __device__ __forceinline__ int t() const { return B20 ? 20 : nt; }
  __device__ __forceinline__ int T() const { return B20 ? 20 : nT; }
  __device__ __forceinline__ int b() const { return B20 ? 20 : nb; }
  __device__ __forceinline__ int p() const { return B20 ? 20 : np; }
};

template <bool B20>
__device__ __forceinline__ StepIdx make_step(const KC& p, const Dims<B20>& D, bool margin_one, float time_t,
                                             float time_n, float bal, float2 f_n, float tin, float mi, int ip_zero) {
  StepIdx st;
  st.bal = bal;
  st.baln = FDIV(f_n.x - f_n.y, mi);
  const float dt = tin - p.setpoint;  // heating.py:118-120 (x / 1.0 == x exactly)
  const float tnorm = margin_one ? dt : dt / p.margin;
  st.it = idx_time(time_t, D.t());
  st.iT = idx_temp(tnorm, D.T());
  st.ib = idx_plain(bal, D.b());
  st.strip = (uint32_t)(((st.it * D.T() + st.iT) * D.b() + st.ib) * D.p());
  const int itn = idx_time(time_n, D.t());
  const int ibn = idx_plain(st.baln, D.b());
  st.nrow = (uint32_t)(((itn * D.T() + st.iT) * D.b() + ibn) * D.p() + ip_zero);
  return st;
}

// Philox exploration codes of every round of step t (p2pmg_device.h::philox_step_codes, layout
// oracle/philox.py::decision_draws): byte r = code of round r, 255 = greedy (QActor.select_action
// rl.py:100-111)
// The explore threshold of a lane's scenario: the launch's scalars, or row `row`, scenario s of the
// per-scenario table (p2pmg_run_episodes_eps).  {thr, all} as eps_threshold forms them.
struct EpsThr {
  uint32_t thr;
  int all;
};
__device__ __forceinline__ EpsThr eps_of(const EpisodeParams& p, int s, int row = 0) {
  EpsThr e{p.eps_thr, p.eps_all};
  if (p.eps_tab) {
    const uint2 v = p.eps_tab[(size_t)row * p.S + s];
    e.thr = v.x;
    e.all = (int)v.y;
  }
  return e;
}
__device__ __forceinline__ uint64_t philox_codes_of(const EpisodeParams& p, int t, uint32_t gid, const EpsThr& e) {
  return philox_step_codes(t, p.R + 1, (uint32_t)p.episode, gid, e.thr, e.all, p.seed_lo, p.seed_hi);
}
__device__ __forceinline__ uint64_t philox_codes_of(const EpisodeParams& p, int t, uint32_t gid) {
  return philox_codes_of(p, t, gid, EpsThr{p.eps_thr, p.eps_all});
}

// all rounds' codes of step t packed one byte per round (round r in bits 8r..8r+7)
// The code-word buffer always exists (greedy runs read and ignore it), so the loads are
// unconditional and branch-free: a load whose destination is touched under a branch before
// its use is waited for at that branch.  The in-kernel Philox words are built separately.
struct CodeWords {
  uint32_t w0, w1;  // loaded words
  uint64_t gen;     // in-kernel Philox word (p.rng == 1)
};
__device__ __forceinline__ CodeWords step_codes(const EpisodeParams& p, const uint32_t* codes_a, size_t off, int t,
                                                int a, int W, const EpsThr& e, bool gen = true) {
  // code words [T][W][A] (replay upload or Philox pre-pass); off = t * W * A
  CodeWords c;
  c.w0 = codes_a[off];
  c.w1 = codes_a[W > 1 ? off + (size_t)p.A : off];
  c.gen = ~0ull;
  if (gen && p.rng == 1) c.gen = philox_codes_of(p, t, p.agent_offset + (uint32_t)a, e);
  return c;
}
__device__ __forceinline__ CodeWords step_codes(const EpisodeParams& p, const uint32_t* codes_a, size_t off, int t,
                                                int a, int W, bool gen = true) {
  return step_codes(p, codes_a, off, t, a, W, EpsThr{p.eps_thr, p.eps_all}, gen);
}
__device__ __forceinline__ uint64_t code_word(const EpisodeParams& p, const CodeWords& c, bool active) {
  const int R1 = p.R + 1;
  uint64_t w = (uint64_t)c.w0 | ((R1 > 4 ? (uint64_t)c.w1 : 0xFFFFFFFFull) << 32);
  w |= (R1 < 8 ? ~0ull << (8 * R1) : 0ull);
  if (p.rng == 1) w = c.gen;
  return (p.mode != 0 || !active) ? ~0ull : w;
}

// the sq16 kernel's code word: its TRAIN launches are exactly p.mode == 0 (launch_sq16_nw), and a
// masked-off lane's draws reach only its dummy stores, so no per-lane mask stays live in the loop
template <bool TRAIN>
__device__ __forceinline__ uint64_t code_word_t(const EpisodeParams& p, const CodeWords& c) {
  if constexpr (!TRAIN) return ~0ull;
  const int R1 = p.R + 1;
  uint64_t w = (uint64_t)c.w0 | ((R1 > 4 ? (uint64_t)c.w1 : 0xFFFFFFFFull) << 32);
  w |= (R1 < 8 ? ~0ull << (8 * R1) : 0ull);
  if (p.rng == 1) w = c.gen;
  return w;
}

// A TD store can hit a row whose prefetch was issued before it.  The prefetched registers
// are not touched (that would force a wait for the load); the patch is applied at use.
template <typename QT>
struct Patch {
  uint32_t row;  // 0xFFFFFFFF = none
  int act;
  QT val;
};
template <typename QT>
__device__ __forceinline__ Row4<QT> sel_row(int b, const Row4<QT>& x0, const Row4<QT>& x1, const Row4<QT>& x2) {
  Row4<QT> r;
  const Sel3M m = sel3_masks(b);
#pragma unroll
  for (int k = 0; k < 3; ++k) r.v[k] = sel3(m, x0.v[k], x1.v[k], x2.v[k]);
  r.v[3] = (QT)0;
  return r;
}
template <typename QT>
__device__ __forceinline__ Row4<QT> patched(Row4<QT> r, uint32_t addr, const Patch<QT>& pt) {
  if (pt.row == addr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) r.v[k] = (pt.act == k) ? pt.val : r.v[k];
  }
  return r;
}

// heat-pump power of an action without a dynamically indexed kernarg array (that compiles to
// a global load + vmcnt(0) on the critical path)
__device__ __forceinline__ float hp_of(const float4& lv, int act) { return sel3(act, lv.x, lv.y, lv.z); }

// community.py:45-54's bilateral exchange of one pair, sign(pij) * min(|pij|, |pji|) where the
// signs differ and 0 where they agree, as ONE v_med3(pij, -pji, 0): with opposite signs pij and
// -pji share a sign and the median of {0, pij, -pji} is the one nearer 0 (min for positives, max
// for negatives); with equal signs 0 lies between them.  Where the reference's value is 0 the
// median may be -0 instead of +0 (and vice versa): the market sums g and pp start at +0, and
// adding a zero of either sign to a sum that starts at +0 never changes its value, so g, pp and
// everything downstream are the same.  (Operands are never NaN.)
__device__ __forceinline__ float pair_exchange(float pij, float pji) {
  return __builtin_amdgcn_fmed3f(pij, -pji, 0.0f);
}
// _divide_power's numerator out * |f_j| (agent.py:193) as (-|out|) * f_j: the filter keeps f_j <= 0
// for out > 0 and f_j >= 0 for out < 0, so f_j = -sign(out) |f_j| and the two products are the same
// IEEE product up to the sign of a zero (out = 0 or f_j = 0: a zero quotient either way); one
// hoisted -|out| replaces an |.| per column.
__device__ __forceinline__ float nabs_out(float out) { return -fabsf(out); }

// ----------------------------------------------------------------- shared-table TD deltas
// Shared-table variant: each workgroup sums its agents' int64 TD deltas for the whole episode in
// an LDS hash table (linear probing, ds_cmpst + ds_add_u64) and flushes one global atomic per
// occupied slot at the end.  All agents of a step share the time bin, so the episode's deltas
// hit only a few thousand entries: without the table, millions of same-address global atomics
// per step serialise.  Exact integer sums, so the grouping never changes the result.
constexpr int kSqWaves = 4;          // waves per workgroup
constexpr int kSqSlotBits = 11;      // 2048 slots: 8 KB keys + 16 KB sums
constexpr int kSqSlots = 1 << kSqSlotBits;
constexpr uint32_t kSqEmpty = 0xFFFFFFFFu;
constexpr int kSqProbes = 16;      // linear-probe limit before the global fallback
constexpr int kSqFlushSteps = 8;    // steps between flushes of the LDS table

__device__ __forceinline__ void lds_add_by_key(uint32_t* hk, unsigned long long* hv, uint32_t key, long long v,
                                               unsigned long long* gbase) {
  if (v == 0) return;
  uint32_t h = (key * 2654435761u) >> (32 - kSqSlotBits);
#pragma nounroll
  for (int probe = 0; probe < kSqProbes; ++probe) {
    const uint32_t prev = atomicCAS(hk + h, kSqEmpty, key);
    if (prev == kSqEmpty || prev == key) {
      atomicAdd(hv + h, (unsigned long long)v);
      return;
    }
    h = (h + 1) & (kSqSlots - 1);
  }
  atomicAdd(gbase + key, (unsigned long long)v);  // crowded run of slots: straight to the global replica
}
// Block-uniform: move the table's sums into the XCD's replica and empty it.  Called every
// kSqFlushSteps steps, not once per episode: a 32-scenario workgroup touches ~3.2k distinct
// (state, action) keys per 96-step episode (more than the 2048 slots) but only ~600 in any
// 8-step window, because the time bin moves on; the total number of global atomics grows by
// ~15 % while the table stays below a third full, so a probe run is ~1 slot long.
__device__ __forceinline__ void lds_hash_flush(uint32_t* hk, unsigned long long* hv, unsigned long long* gbase,
                                               int nthreads) {
  __syncthreads();
  for (int k2 = threadIdx.x; k2 < kSqSlots; k2 += nthreads) {
    const uint32_t key = hk[k2];
    if (key != kSqEmpty) {
      const long long x = (long long)hv[k2];
      if (x != 0) atomicAdd(gbase + key, (unsigned long long)x);
      hk[k2] = kSqEmpty;
      hv[k2] = 0;
    }
  }
  __syncthreads();
}

// every episode kernel's Q-row gather (timing-only ablations 1 and 4: the row from its address, no load)
template <typename QT>
__device__ __forceinline__ Row4<QT> gather_row(const QT* p) {
#if P2PMG_ABLATE == 1 || P2PMG_ABLATE == 4
  const uint32_t x = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 5);
  return Row4<QT>{{(QT)(x & 3), (QT)((x >> 2) & 3), (QT)((x >> 4) & 3), (QT)0}};
#else
  return load_row(p);
#endif
}

inline unsigned grid_for(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace
}  // namespace p2pmg
