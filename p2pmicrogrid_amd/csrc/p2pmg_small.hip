// p2pmg_small.hip — the tabular path's utility kernels (table deltas, code words, step pre-pass, record
// unpack, packing, metrics, the standalone reference primitives) and rule_episode_kernel, with their launchers.
#include "p2pmg_fastmath.h"

namespace p2pmg {
namespace {

// Q += delta * 2^-40 (f64), delta = 0: the end-of-episode update of the shared table, after the
// optional all-reduce of the int64 deltas over ranks
template <typename QT>
__global__ void apply_delta_kernel(QT* __restrict__ q, long long* __restrict__ d, size_t n) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const long long x = d[k];
  if (x != 0) {
    q[k] = (QT)((double)q[k] + (double)x * (1.0 / kDeltaScale));
    d[k] = 0;
  }
}

// sum the per-XCD delta replicas into copy 0 (and clear the others)
__global__ void fold_delta_kernel(long long* __restrict__ d, size_t n) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  long long x = d[k];
#pragma unroll
  for (int c = 1; c < kDeltaCopies; ++c) {
    const long long y = d[(size_t)c * n + k];
    if (y != 0) {
      x += y;
      d[(size_t)c * n + k] = 0;
    }
  }
  d[k] = x;
}

// battery rule over per-agent sequences (unit parity with storage.py / agent.py:138-153)
__global__ void battery_seq_kernel(int agents, int steps, const double* bal, double* out_bal, double* soc_hist,
                                   double* soc, const double* cap, double smin, double smax, double sqrt_eff) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= agents) return;
  double s_ = soc[a];
  for (int t = 0; t < steps; ++t) {
    const size_t k = (size_t)a * steps + t;
    out_bal[k] = battery_rule(bal[k], s_, cap[a], smin, smax, sqrt_eff);
    soc_hist[k] = s_;
  }
  soc[a] = s_;
}

// Philox pre-pass: every (t, agent) code word of an episode in one parallel launch, so the
// latency-bound episode loop only loads a prefetched word instead of computing R+1 blocks.
__global__ void philox_codes_kernel(const EpisodeParams p, uint32_t* __restrict__ words) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // k = t * A + a
  if (k >= (size_t)p.T * p.A) return;
  const int t = (int)(k / p.A), a = (int)(k % p.A);
  const int R1 = p.R + 1, W = (R1 + 3) >> 2;
  const uint32_t gid = p.agent_offset + (uint32_t)a;
  const EpsThr e = eps_of(p, a / p.N);  // the scenario's own threshold under p2pmg_run_episodes_eps
  const uint64_t codes = philox_codes_of(p, t, gid, e);
  for (int w = 0; w < W; ++w)
    words[((size_t)t * W + w) * p.A + a] =
        w < 2 ? (uint32_t)(codes >> (32 * w))
              : philox_code_word(t, R1, w, (uint32_t)p.episode, gid, e.thr, e.all, p.seed_lo, p.seed_hi);
}

// host replay codes u8 [T][R1][A] -> code words [T][W][A]
__global__ void pack_codes_kernel(int T, int R1, int A, const uint8_t* __restrict__ in, uint32_t* __restrict__ words) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (size_t)T * A) return;
  const int t = (int)(k / A), a = (int)(k % A);
  const int W = (R1 + 3) >> 2;
  for (int w = 0; w < W; ++w) {
    uint32_t word = 0xFFFFFFFFu;
    for (int b = 0; b < 4 && 4 * w + b < R1; ++b) {
      const uint32_t c = in[((size_t)t * R1 + 4 * w + b) * A + a];
      word = (word & ~(0xFFu << (8 * b))) | (c << (8 * b));
    }
    words[((size_t)t * W + w) * A + a] = word;
  }
}

// the step pre-pass as its own launch (prepass_one)
__global__ void step_prepass_kernel(const EpisodeParams p, const PrepOut o) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // k = t * A + a
  if (k >= (size_t)p.T * p.A) return;
  prepass_one(p, o, k, (int)blockIdx.y);  // blockIdx.y: the chain's episode (uniform per workgroup)
}

// Hazard distance of an interleaved chain (episode_fast_kernel's PIPE form), from the pre-pass words:
// step u of an agent's earlier episode and step v of its later one conflict when they touch rows of
// one (time bin, balance bin) key with a write involved: lo(u) == lo(v) (the step's own rows, read
// and written), lo(u) == hi(v) or hi(u) == lo(v) (hi: the next-state row, read only).  Step T - 1's
// next-state read alone does not count: the kernel serves it from the follower's undo log.  *out =
// max u - v over every agent's conflicting pairs (atomicMax; the caller presets it to 0, what u == v gives).
// One thread per agent, O(T^2) compares, the words read through the caches.
__global__ void chain_lag_kernel(int T, int A, const uint2* __restrict__ pre, int* __restrict__ out) {
  const int a = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (a >= A) return;
  int best = 0;
  for (int u = T - 1; u > best; --u) {
    const uint32_t wu = pre[(size_t)u * A + a].y;
    const uint32_t lu = wu & 0xFFFFu, hu = u == T - 1 ? 0xFFFFFFFFu : wu >> 16;
    for (int v = 0; v < u - best; ++v) {
      const uint32_t wv = pre[(size_t)v * A + a].y;
      const uint32_t lv = wv & 0xFFFFu, hv = wv >> 16;
      if (lu == lv || lu == hv || hu == lv) {
        best = u - v;
        break;
      }
    }
  }
  atomicMax(out, best);
}

// FastRec rows -> the general record buffers (reward, cost, grid, p2p, tin [T][A]; action u8 and
// packed index i32 [T][R+1][A]), for the records the caller asks for
__global__ void fast_rec_unpack_kernel(int T, int R1, int A, uint32_t tb, const FastRec* __restrict__ recs, int narrow,
                                       int which, void* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // k = t * A + a
  if (k >= (size_t)T * A) return;
  if (narrow) {  // [T][A] float2 {reward, cost}
    const float2 v = reinterpret_cast<const float2*>(recs)[k];
    reinterpret_cast<float*>(out)[k] = which == 0 ? v.x : v.y;
    return;
  }
  const FastRec r = recs[k];
  if (which < 5) {
    const float v[5] = {r.reward, r.cost, r.grid, r.p2p, r.tin};
    reinterpret_cast<float*>(out)[k] = v[which];
    return;
  }
  const size_t t = k / A, a = k % A;
  for (int rr = 0; rr < R1; ++rr) {
    const size_t kk = (t * R1 + rr) * A + a;
    if (which == 5)
      reinterpret_cast<uint8_t*>(out)[kk] = (uint8_t)(r.actions >> (8 * rr));
    else
      reinterpret_cast<int32_t*>(out)[kk] = (int32_t)(((r.bins & 0xFFFFu) / tb) | ((r.bins >> 16) << 8) |
                                                      (((r.bins & 0xFFFFu) % tb) << 16) | (((r.ips >> (8 * rr)) & 0xFFu) << 24));
  }
}

// ----------------------------------------------------------------- RuleAgent communities
// CommunityMicrogrid.run (community.py:95-123) of get_rule_based_community (community.py:237-238):
// every agent is a RuleAgent (agent.py:106-136), so there is no policy and no exchange round.
// Per step: the hysteresis rule on the pre-update T_in (on at T_in <= the agent's lower bound, off at
// T_in >= its upper bound, else unchanged; agent.py:130-136), net power (load - pv) + hp
// (agent.py:119-128), the market on the (N, 1) stack (TF broadcasts it against its transpose:
// ex_ij = sign(P_i) min(|P_i|, |P_j|) on differing signs, p_grid_i = sum_j (P_i - ex_ij),
// community.py:45-54), costs (community.py:56-65), then HPHeating.step (heating.py:138-143).
// One lane per agent, G lanes per scenario, the group's P through LDS; hp_on persists.
template <int G>
__global__ __launch_bounds__(kWave) void rule_episode_kernel(const EpisodeParams p, float* __restrict__ hp_on) {
  constexpr int SPW = kWave / G;
  __shared__ float shP[kWave];
  const int lane = (int)threadIdx.x;
  const int sl = lane / G, i = lane % G;
  const int N = p.N;
  const int s = (int)blockIdx.x * SPW + sl;
  const bool active = i < N && s < p.S;
  const int a = active ? s * N + i : 0;
  const int s_env = p.n_env == 1 ? 0 : (s < p.S ? s : 0);
  const size_t A = (size_t)p.A;
  const KC k = scalar_constants(p, p.thermal[a]);  // the agent's own thresholds and COP
  const Recip rmph = recip(k.mph);
  const float hpmax = p.hp_lv[a].z;  // HeatPump.max_power (hp.power in {0, 1})
  float on = active ? hp_on[a] : 0.0f;
  float tin = active ? p.t_in[a] : k.setpoint;
  float tm = active ? p.t_m[a] : k.setpoint;
  const float* envb = p.env + (size_t)s_env * kEnvStride;
  const size_t env_step = (size_t)p.n_env * kEnvStride;
  const uint32_t rec = (uint32_t)p.record;
  for (int t = 0; t < p.T; ++t) {
    const EnvRow e = load_env(envb + (size_t)t * env_step);
    const float2 f = p.prof[(size_t)t * A + a];
    on = tin <= k.lower ? 1.0f : (tin >= k.upper ? 0.0f : on);
    const float hp = on * hpmax;
    const float P = (f.x - f.y) + hp;
    shP[lane] = P;
    wave_lds_fence();
    float g = 0.0f, pp = 0.0f;
    for (int j = 0; j < N; ++j) {
      const float pj = shP[sl * G + j];
      const float ex = pair_exchange(P, pj);
      g = g + (P - ex);
      pp = pp + ex;
    }
    wave_lds_fence();
    float cost = (g >= 0.0f) ? g * e.buy : g * e.inj;
    cost = cost + pp * e.p2p;
    cost = fdiv_b(cost * k.slot, rmph);
    cost = cost * k.kilo;
    if (active) {
      const size_t tA = (size_t)t * A + a;
      if (rec & 2u) p.rec_cost[tA] = cost;
      if (rec & 4u) p.rec_grid[tA] = g;
      if (rec & 8u) p.rec_p2p[tA] = pp;
      if (rec & 16u) p.rec_tin[tA] = tin;
      if (rec & 32u) p.rec_action[tA] = on != 0.0f ? 2 : 0;  // action 2 = 1.0 x max_power
    }
    rc_update(k, e.t_out, hp, tin, tm);
  }
  if (active) {
    p.t_in[a] = tin;
    p.t_m[a] = tm;
    hp_on[a] = on;
  }
}

template <int G>
void launch_rule_g(const EpisodeParams& p, float* hp_on, hipStream_t st) {
  constexpr int SPW = kWave / G;
  hipLaunchKernelGGL(rule_episode_kernel<G>, dim3((p.S + SPW - 1) / SPW), dim3(kWave), 0, st, p, hp_on);
}

// ----------------------------------------------------------------- small kernels
__global__ void rc_step_kernel(int n, const float* t_out, const float* t_in, const float* t_m, const float* hp,
                               float* t_in_new, float* t_m_new, RcParams rc) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  float a = t_in[k], b = t_m[k];
  rc_update(rc, t_out[k], hp[k], a, b);
  t_in_new[k] = a;
  t_m_new[k] = b;
}
// ... with one COP per element (cop == null: rc.cop) and the caller's solar term in rc.solar
// (heating.temperature_simulation with hp_cop / solar_rad, heating.py:37-56)
__global__ void rc_step_ex_kernel(int n, const float* t_out, const float* t_in, const float* t_m, const float* hp,
                                  const float* cop, float* t_in_new, float* t_m_new, RcParams rc) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  if (cop) rc.cop = cop[k];
  float a = t_in[k], b = t_m[k];
  rc_update(rc, t_out[k], hp[k], a, b);
  t_in_new[k] = a;
  t_m_new[k] = b;
}

__global__ void state_indices_kernel(int n, const float* obs, int32_t* idx, int nt, int nT, int nb, int np) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float4 o = reinterpret_cast<const float4*>(obs)[k];
  idx[4 * k + 0] = idx_time(o.x, nt);
  idx[4 * k + 1] = idx_temp(o.y, nT);
  idx[4 * k + 2] = idx_plain(o.z, nb);
  idx[4 * k + 3] = idx_plain(o.w, np);
}

__global__ void t0_philox_kernel(int A, float* t_in, float* t_m, uint32_t k0, uint32_t k1, int episode,
                                 uint32_t agent_offset, const float4* __restrict__ thermal, double sigma) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= A) return;
  // T0 ~ N(setpoint_a, sigma): the agent's own mean (t0_draw widens it to f64 before the add)
  t0_draw(k0, k1, episode, agent_offset + (uint32_t)k, thermal[k].x, sigma, t_in[k], t_m[k]);
}

// reference layout [count][n_states][n_actions] (host dtype) <-> padded device layout
template <typename D, typename S>
__global__ void q_pack_kernel(size_t rows, int na, const S* src, D* dst) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= rows) return;
#pragma unroll
  for (int c = 0; c < kQPad; ++c) dst[k * kQPad + c] = c < na ? (D)src[k * na + c] : (D)0;
}
template <typename D, typename S>
__global__ void q_unpack_kernel(size_t rows, int na, const S* src, D* dst) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= rows) return;
  for (int c = 0; c < na; ++c) dst[k * na + c] = (D)src[k * kQPad + c];
}

// [A][T] load / pv (the host's per-agent rows) -> [T][A] float2 (time-major, one coalesced 8-B load
// per lane per step): a 32 x 32 tile transposed through LDS, so the reads are 128-B runs of one
// agent's steps and the writes 256-B runs of one step's agents (round 5; the per-element form read
// with stride T, 32x the input in fetched sectors).  Block (32, 8), tile [agent][step] padded to 33.
__global__ __launch_bounds__(256) void prof_pack_kernel(int A, int T, const float* __restrict__ load_w,
                                                        const float* __restrict__ pv_w, float2* __restrict__ prof) {
  __shared__ float tl[32][33], tv[32][33];
  const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
  const int a0 = (int)blockIdx.x * 32, t0 = (int)blockIdx.y * 32;  // grid.x: agents (grid.y <= 65535)
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const int a = a0 + ty + k, t = t0 + tx;
    if (a < A && t < T) {
      const size_t src = (size_t)a * T + t;
      tl[ty + k][tx] = load_w[src];
      tv[ty + k][tx] = pv_w[src];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const int t = t0 + ty + k, a = a0 + tx;
    if (a < A && t < T) prof[(size_t)t * A + a] = make_float2(tl[tx][ty + k], tv[tx][ty + k]);
  }
}

// The fast quotients of the episode kernels next to the IEEE operator, for the division fuzz test
// (tests/test_gpu_division.py): exactly the guarded sequences the kernels run.
//   f32 out[0] fdiv_b (hoisted reciprocal of a divisor checked on the host, IEEE when the numerator
//              is out of range)            - max_in, 60, N, the comfort margin
//       out[1] the divide-power form: recip of a data-dependent divisor, fdiv_core, IEEE when the
//              divisor or the numerator is out of range
//       out[2] the packed sq16 form (fdiv_core_pk) under its range-19 guard, else out[1]'s form
//       out[3] IEEE a / b
//   f64 out[0] fdiv64 (hoisted Recip64 + range test), out[1] qcore64 under q64_ok (battery_rule_r's
//       guard), out[2] IEEE n / d
__global__ void fdiv_check_kernel(int n, const float* __restrict__ a, const float* __restrict__ b,
                                  float* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float x = a[k], d = b[k];
  const Recip r = recip(d);
  out[4 * (size_t)k + 0] = r.ok ? fdiv_b(x, r) : fdiv_ieee(x, d);
  float q1 = fdiv_core(x, r);
  if (!r.ok || !fdiv_ok(x)) q1 = fdiv_ieee(x, d);
  out[4 * (size_t)k + 1] = q1;
  float q2 = q1;
  if (r.ok && in_range19(x) && in_range19(d) && d > 0.0f) {  // the kernel's divisor is tot = |sum| > 0
    const pkf2 y2 = {r.y, r.y}, b2 = {d, d};
    q2 = fdiv_core_pk(pkf2{x, x}, b2, y2).x;
  }
  out[4 * (size_t)k + 2] = q2;
  out[4 * (size_t)k + 3] = fdiv_ieee(x, d);
}
__global__ void fdiv64_check_kernel(int n, const double* __restrict__ a, const double* __restrict__ b,
                                    double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double x = a[k], d = b[k];
  const Recip64 r = recip64(d);
  out[3 * (size_t)k + 0] = fdiv64(x, r);
  double q1 = qcore64(x, r);
  if (!(r.ok && q64_ok(x))) q1 = fdiv64_ieee(x, d);
  out[3 * (size_t)k + 1] = q1;
  out[3 * (size_t)k + 2] = fdiv64_ieee(x, d);
}

// Episode metrics of the context (community.py:179 avg_reward per scenario): out = {sum_s ep_reward[s],
// S} in f64, one workgroup, a fixed reduction tree (deterministic), ready for the RCCL all-reduce.
__global__ __launch_bounds__(256) void metrics_kernel(int S, const float* __restrict__ ep, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int s = threadIdx.x; s < S; s += 256) acc += (double)ep[s];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = sh[0];
    out[1] = (double)S;
  }
}
// Order-independent 64-bit fingerprint of a table's bit pattern (sum over words of a splitmix of
// (word, index)): equal on every rank iff the replicas hold the same bits (up to hash collisions)
__global__ void table_hash_kernel(const uint32_t* __restrict__ w, size_t n, unsigned long long* __restrict__ out) {
  unsigned long long acc = 0;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
    unsigned long long x = ((unsigned long long)w[k] << 32) ^ (k * 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    acc += x ^ (x >> 31);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

// Standalone QActor calls, applied in order by a single thread (rl.py:89-129).
template <typename QT>
__global__ void q_calls_kernel(const QCallParams p) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int k = 0; k < p.n; ++k) {
    QT* q = reinterpret_cast<QT*>(p.q) + (size_t)p.agents[k] * p.n_states * kQPad;
    const float* o = p.s_obs + 4 * k;
    const uint32_t srow = (uint32_t)(((idx_time(o[0], p.nt) * p.nT + idx_temp(o[1], p.nT)) * p.nb +
                                      idx_plain(o[2], p.nb)) * p.np + idx_plain(o[3], p.np));
    const Row4<QT> row = load_row(q + srow * kQPad);
    const int code = p.codes[k];
    const int a = code == 255 ? argmax3(row) : code;
    p.actions[k] = a;
    p.q_out[k] = code == 255 ? (double)row.v[a] : 0.0;
    if (p.train) {
      const float* n = p.ns_obs + 4 * k;
      const uint32_t nrow = (uint32_t)(((idx_time(n[0], p.nt) * p.nT + idx_temp(n[1], p.nT)) * p.nb +
                                        idx_plain(n[2], p.nb)) * p.np + idx_plain(n[3], p.np));
      const QT qmax = max3(load_row(q + nrow * kQPad));
      const LearnRow lr = p.learn[p.agents[k]];  // the agent's own alpha and gamma (rl.py:125-128)
      q[srow * kQPad + a] = td_update(q[srow * kQPad + a], p.rewards[k], qmax, lr.alpha, lr.gamma);
    }
  }
}

}  // namespace

hipError_t launch_philox_codes(const EpisodeParams& p, uint32_t* words, hipStream_t stream) {
  const size_t n = (size_t)p.T * p.A;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(philox_codes_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, p, words);
  return hipGetLastError();
}

hipError_t launch_pack_codes(int T, int R1, int A, const uint8_t* in, uint32_t* words, hipStream_t stream) {
  const size_t n = (size_t)T * A;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(pack_codes_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, T, R1, A, in, words);
  return hipGetLastError();
}

hipError_t launch_fold_delta(long long* qdelta, size_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fold_delta_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, qdelta, n);
  return hipGetLastError();
}

hipError_t launch_apply_delta(void* q, long long* qdelta, size_t n, int q_dtype, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (q_dtype == 0)
    hipLaunchKernelGGL(apply_delta_kernel<double>, dim3(grid_for(n, 256)), dim3(256), 0, stream, (double*)q, qdelta, n);
  else
    hipLaunchKernelGGL(apply_delta_kernel<float>, dim3(grid_for(n, 256)), dim3(256), 0, stream, (float*)q, qdelta, n);
  return hipGetLastError();
}

hipError_t launch_battery_seq(int agents, int steps, const double* bal, double* out_bal, double* soc_hist, double* soc,
                              const double* cap, double smin, double smax, double sqrt_eff, hipStream_t stream) {
  if (agents <= 0) return hipSuccess;
  hipLaunchKernelGGL(battery_seq_kernel, dim3(grid_for(agents, 64)), dim3(64), 0, stream, agents, steps, bal, out_bal,
                     soc_hist, soc, cap, smin, smax, sqrt_eff);
  return hipGetLastError();
}

hipError_t launch_step_prepass(const EpisodeParams& p, const PrepOut& o, hipStream_t stream) {
  const size_t n = (size_t)p.T * p.A;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(step_prepass_kernel, dim3(grid_for(n, 256), o.n_ep > 1 ? o.n_ep : 1), dim3(256), 0, stream, p, o);
  return hipGetLastError();
}

hipError_t launch_chain_lag(int T, int A, const uint2* pre, int* out, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(out, 0, sizeof(int), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(chain_lag_kernel, dim3(grid_for((size_t)A, 64)), dim3(64), 0, stream, T, A, pre, out);
  return hipGetLastError();
}

hipError_t launch_fast_rec_unpack(int T, int R1, int A, uint32_t tb, const void* recs, int narrow, int which, void* out,
                                  hipStream_t stream) {
  const size_t n = (size_t)T * A;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(fast_rec_unpack_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, T, R1, A, tb,
                     reinterpret_cast<const FastRec*>(recs), narrow, which, out);
  return hipGetLastError();
}

hipError_t launch_rule_episode(const EpisodeParams& p, float* hp_on, hipStream_t stream) {
  const int n = p.N;
  if (n <= 1) launch_rule_g<1>(p, hp_on, stream);
  else if (n <= 2) launch_rule_g<2>(p, hp_on, stream);
  else if (n <= 4) launch_rule_g<4>(p, hp_on, stream);
  else if (n <= 8) launch_rule_g<8>(p, hp_on, stream);
  else if (n <= 16) launch_rule_g<16>(p, hp_on, stream);
  else if (n <= 32) launch_rule_g<32>(p, hp_on, stream);
  else if (n <= 64) launch_rule_g<64>(p, hp_on, stream);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_rc_step(int n, const float* t_out, const float* t_in, const float* t_m, const float* hp,
                          float* t_in_new, float* t_m_new, RcParams rc, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(rc_step_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, n, t_out, t_in, t_m, hp, t_in_new,
                     t_m_new, rc);
  return hipGetLastError();
}
hipError_t launch_rc_step_ex(int n, const float* t_out, const float* t_in, const float* t_m, const float* hp,
                             const float* cop, float* t_in_new, float* t_m_new, RcParams rc, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(rc_step_ex_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, n, t_out, t_in, t_m, hp, cop,
                     t_in_new, t_m_new, rc);
  return hipGetLastError();
}

hipError_t launch_state_indices(int n, const float* obs, int32_t* idx, int nt, int nT, int nb, int np,
                                hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(state_indices_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, n, obs, idx, nt, nT, nb, np);
  return hipGetLastError();
}

hipError_t launch_t0_philox(int A, float* t_in, float* t_m, uint32_t seed_lo, uint32_t seed_hi, int episode,
                            uint32_t agent_offset, const float4* thermal, double sigma, hipStream_t stream) {
  if (A <= 0) return hipSuccess;
  hipLaunchKernelGGL(t0_philox_kernel, dim3(grid_for(A, 256)), dim3(256), 0, stream, A, t_in, t_m, seed_lo, seed_hi,
                     episode, agent_offset, thermal, sigma);
  return hipGetLastError();
}

hipError_t launch_q_pack(int count, size_t n_states, int n_actions, const void* src_ref, void* dst_pad, int q_dtype,
                         int src_dtype, hipStream_t stream) {
  const size_t rows = (size_t)count * n_states;
  if (rows == 0) return hipSuccess;
  const dim3 g(grid_for(rows, 256)), b(256);
  if (q_dtype == 0 && src_dtype == 0)
    hipLaunchKernelGGL((q_pack_kernel<double, double>), g, b, 0, stream, rows, n_actions, (const double*)src_ref, (double*)dst_pad);
  else if (q_dtype == 0)
    hipLaunchKernelGGL((q_pack_kernel<double, float>), g, b, 0, stream, rows, n_actions, (const float*)src_ref, (double*)dst_pad);
  else if (src_dtype == 0)
    hipLaunchKernelGGL((q_pack_kernel<float, double>), g, b, 0, stream, rows, n_actions, (const double*)src_ref, (float*)dst_pad);
  else
    hipLaunchKernelGGL((q_pack_kernel<float, float>), g, b, 0, stream, rows, n_actions, (const float*)src_ref, (float*)dst_pad);
  return hipGetLastError();
}

hipError_t launch_q_unpack(int count, size_t n_states, int n_actions, const void* src_pad, void* dst_ref, int q_dtype,
                           int dst_dtype, hipStream_t stream) {
  const size_t rows = (size_t)count * n_states;
  if (rows == 0) return hipSuccess;
  const dim3 g(grid_for(rows, 256)), b(256);
  if (q_dtype == 0 && dst_dtype == 0)
    hipLaunchKernelGGL((q_unpack_kernel<double, double>), g, b, 0, stream, rows, n_actions, (const double*)src_pad, (double*)dst_ref);
  else if (q_dtype == 0)
    hipLaunchKernelGGL((q_unpack_kernel<float, double>), g, b, 0, stream, rows, n_actions, (const double*)src_pad, (float*)dst_ref);
  else if (dst_dtype == 0)
    hipLaunchKernelGGL((q_unpack_kernel<double, float>), g, b, 0, stream, rows, n_actions, (const float*)src_pad, (double*)dst_ref);
  else
    hipLaunchKernelGGL((q_unpack_kernel<float, float>), g, b, 0, stream, rows, n_actions, (const float*)src_pad, (float*)dst_ref);
  return hipGetLastError();
}

hipError_t launch_q_calls(const QCallParams& p, hipStream_t stream) {
  if (p.n <= 0) return hipSuccess;
  if (p.q_dtype == 0)
    hipLaunchKernelGGL(q_calls_kernel<double>, dim3(1), dim3(64), 0, stream, p);
  else
    hipLaunchKernelGGL(q_calls_kernel<float>, dim3(1), dim3(64), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_metrics(int S, const float* ep, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(metrics_kernel, dim3(1), dim3(256), 0, stream, S, ep, out);
  return hipGetLastError();
}
hipError_t launch_table_hash(const void* q, size_t bytes, unsigned long long* out, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(out, 0, 8, stream);
  if (e != hipSuccess) return e;
  const size_t n = bytes / 4;
  hipLaunchKernelGGL(table_hash_kernel, dim3((unsigned)std::min<size_t>(2048, grid_for(n, 256))), dim3(256), 0, stream,
                     reinterpret_cast<const uint32_t*>(q), n, out);
  return hipGetLastError();
}

hipError_t launch_fdiv_check(int n, const float* a, const float* b, float* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fdiv_check_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, n, a, b, out);
  return hipGetLastError();
}
hipError_t launch_fdiv64_check(int n, const double* a, const double* b, double* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fdiv64_check_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, n, a, b, out);
  return hipGetLastError();
}

hipError_t launch_prof_pack(int A, int T, const float* load_w, const float* pv_w, float2* prof, hipStream_t stream) {
  if ((size_t)A * T == 0) return hipSuccess;
  if ((T + 31) / 32 > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prof_pack_kernel, dim3((A + 31) / 32, (T + 31) / 32), dim3(32, 8), 0, stream, A, T, load_w, pv_w,
                     prof);
  return hipGetLastError();
}

}  // namespace p2pmg
