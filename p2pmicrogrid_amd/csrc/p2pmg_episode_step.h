// p2pmg_episode_step.h — what the lane-per-agent episode kernels share: episode_kernel (p2pmg_general.hip) and
// policy_episode_kernel (p2pmg_policy.hip).  The two kernels differ in where a round's action comes from (an
// argmax over a gathered Q row or an exploration code; a byte of a packed policy) and in what follows the reward
// (a TD update; nothing).
//   * The proposal matrix of a scenario in registers or LDS tiles (PRegs / PTile) and the run-time group sum:
//     defined here once, used by both kernels.
//   * The step between a round's action and the reward (the p2p bin of a round, _divide_power, the market, the
//     cost and the reward) as __forceinline__ helpers: policy_episode_kernel's body.  They restate, expression
//     for expression and in the same order, what episode_kernel's body writes out; episode_kernel keeps its own
//     text because calling the helpers from it moved the register allocation of 94 of its instantiations by a
//     few VGPRs ("Policy evaluation").  tests/test_gpu_policy_set.py holds the two to each other
//     bit for bit (capture, then run_policy against run_episode("greedy")), in both forms.
#pragma once
#include "p2pmg_tabular.h"

namespace p2pmg {
namespace {

// The proposal matrix P of one scenario as the kernels hold it (community.py:75-86): lane i
// owns row i; round r reads column i of round r - 1's P (Jacobi: every agent answers the previous
// round's proposals) and writes its new row; the market reads row i and column i of the final P.
//   PRegs<N>  N <= 16 compiled in: row and column in registers, the column by exchange<N>
//   PTile<NC> any community size n <= NC (16, 32, 64) at run time: the scenario's P in two LDS
//             tiles (the round being read, the round being written) with an odd row stride, so the
//             column read (lane i at j * stride + i) and the row read (lane i at i * stride + j) are
//             both conflict-free.  Every agent of a scenario is a lane of the same wave, so a
//             wavefront-scope fence orders the tiles (no workgroup barrier, no vmcnt drain).
template <int N>
struct PRegs {
  float row[N], col[N];
  float* sh;
  int i, sl;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < N; ++j) { row[j] = 0.0f; col[j] = 0.0f; }
  }
  __device__ __forceinline__ void next_round() { exchange<N>(row, col, i, sl, sh); }
  __device__ __forceinline__ float colv(int j) const { return col[j]; }
  __device__ __forceinline__ float rowv(int j) const { return row[j]; }
  __device__ __forceinline__ void put(int j, float v) { row[j] = v; }
};
template <int NC>
struct PTile {
  static constexpr int kStride = NC + 1;
  static constexpr int kTile = NC * kStride;
  float* base;  // this scenario's two tiles
  int i, rd, wr;
  __device__ __forceinline__ void clear() {}  // round 0 reads no column (its powers are all -0)
  __device__ __forceinline__ void next_round() {
    wave_lds_fence();  // every lane's row of the round just written is visible
    rd = wr;
    wr ^= 1;
  }
  __device__ __forceinline__ float colv(int j) const { return base[rd * kTile + j * kStride + i]; }
  __device__ __forceinline__ float rowv(int j) const { return base[rd * kTile + i * kStride + j]; }
  __device__ __forceinline__ void put(int j, float v) { base[wr * kTile + i * kStride + j] = v; }
};
// sum_{k < n} v_k over a scenario group of run-time size n through LDS, sequential from +0.0
template <int NC>
__device__ __forceinline__ float group_sum_n(float v, int i, int sl, int n, float* sh) {
  if (i < n) sh[sl * NC + i] = v;
  wave_lds_fence();
  float m = 0.0f;
  for (int k = 0; k < n; ++k) m = m + sh[sl * NC + k];
  wave_lds_fence();
  return m;
}

// LDS floats of one wave's exchange: the tiles (WIDE), exchange<N>'s tile for N = 16, else none; and of its
// group sums
template <int NC, bool WIDE>
constexpr int step_p_floats() {
  constexpr int G = pow2ceil(NC), SPW = kWave / G;
  return WIDE ? SPW * 2 * PTile<NC>::kTile : (G > 8 ? SPW * NC * NC : 1);
}
template <int NC, bool WIDE>
constexpr int step_r_floats() {
  constexpr int G = pow2ceil(NC), SPW = kWave / G;
  return (WIDE || G > 8) ? SPW * NC : 1;
}

// The community of a lane: n agents (NC compiled in, or p.N <= NC at run time), and x / n (the mean over the
// community, the even split): div_n's power-of-two multiply is the IEEE quotient
template <int NC, bool WIDE>
struct Community {
  int n_rt;
  float nf;
  __device__ __forceinline__ int n() const { return WIDE ? n_rt : NC; }
  __device__ __forceinline__ float divn(float x) const {
    if constexpr (WIDE) return x / nf;
    else return div_n<NC>(x);
  }
};

// the p2p bin of round r > 0, after P.next_round(): powers = -P[:, i] with the diagonal zeroed
// (community.py:76,81); p2p = mean / max_in (agent.py:203)
template <int NC, bool WIDE, typename PT>
__device__ __forceinline__ int round_p2p_bin(const PT& P, const Community<NC, WIDE>& C, int i, float mi, int np) {
  const int n = C.n();
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < n; ++j) acc = acc + (-((j == i) ? 0.0f : P.colv(j)));
  return idx_plain(FDIV(C.divn(acc), mi), np);
}

// RLAgent._divide_power agent.py:186-195 on the net power `out` of round r: the lane's new row of P
template <int NC, bool WIDE, typename PT>
__device__ __forceinline__ void divide_power(PT& P, const Community<NC, WIDE>& C, int i, int r, float out) {
  const int n = C.n();
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
    const float ev = C.divn(out * 1.0f);
#pragma unroll
    for (int j = 0; j < n; ++j) P.put(j, ev);
  } else {
    // |f_ii| = 0 (own power is -0): (out * 0) / tot == out * 0 exactly for any non-NaN tot
#pragma unroll
    for (int j = 0; j < n; ++j)
      P.put(j, (j == i) ? (tot == tot ? out * 0.0f : tot) : FDIV(nabs_out(out) * filt(j), tot));
  }
}

// CommunityMicrogrid._assign_powers community.py:45-54 on the final P (diagonal kept), after P.next_round();
// _compute_costs community.py:56-65; RLAgent.get_reward agent.py:225-232 (pre-update T_in)
struct StepOutcome {
  float g, pp, cost, rw;
};
template <int NC, bool WIDE, typename PT>
__device__ __forceinline__ StepOutcome market_reward(const PT& P, const Community<NC, WIDE>& C, const KC& k,
                                                     const EnvRow& e0, float tin) {
  const int n = C.n();
  float g = 0.0f, pp = 0.0f;
#pragma unroll
  for (int j = 0; j < n; ++j) {
    const float pij = P.rowv(j), pji = P.colv(j);
    const float ex = pair_exchange(pij, pji);
    g = g + (pij - ex);
    pp = pp + ex;
  }
  float cost = (g >= 0.0f) ? g * e0.buy : g * e0.inj;
  cost = cost + pp * e0.p2p;
  cost = FDIV(cost * k.slot, k.mph);
  cost = cost * k.kilo;
  float pen = fmaxf(fmaxf(0.0f, k.lower - tin), fmaxf(0.0f, tin - k.upper));
  pen = pen > 0.0f ? pen + 1.0f : 0.0f;
  return StepOutcome{g, pp, cost, -(cost + k.penw * pen)};
}

}  // namespace
}  // namespace p2pmg
